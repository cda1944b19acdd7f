// The reference's experimental sorting cache (PathPlanner(..., experimental_performance_improvements=True)), per planner:
//   core_trace_sorter.py:57-87   cone_arrays_are_similar
//                       :101-110 ConeSortingCacheEntry
//                       :189-195 the entry is replaced at the end of every sort_left_right call
//                       :218-250 input_is_very_similar_to_previous_input
//                       :293-300 the check, after the start cones are selected and before the search
// One entry per planner, double-buffered in HBM: the kernels of a call read `prev` and write `next`, the host swaps the two
// after the whole call (every chunk of it), so both sides of a frame — and a pass that has to be repeated — see the same
// previous entry.
#pragma once

#include "fsdp_device.h"

namespace fsdp {

struct SortCacheHdr {
  int32_t valid;         // an entry exists
  int32_t n;             // cones of the entry: rows [off[planner], off[planner] + n) of the entry's cone store
  int32_t has[2];        // per side (0 left, 1 right): a result — its starting cones are not None
  int32_t n_start[2];    // 1 or 2 starting cones
  int32_t best_len[2];   // best configuration (before combine_traces), as the search left it
  int32_t n_configs[2];  // len(configs)
  double best_cost[2];   // scores[0]
  double start[2][2][3];  // starting cones (x, y, type)
  int16_t best[2][MAX_LEN];
};

struct SortCacheView {
  const SortCacheHdr* prev = nullptr;
  SortCacheHdr* next = nullptr;
  const double* prev_xyt = nullptr;   // cone stores (x, y, type rows), one region per planner
  const int32_t* prev_off = nullptr;
  double* next_xyt = nullptr;
  const int32_t* next_off = nullptr;  // (a region holds the most cones the planner was ever given: room for its previous entry too)
  int8_t* hits = nullptr;             // (planners, 2): 1 reused, 0 checked and computed, -1 returned before the check
  int base = 0;                       // planner of the launch's frame 0 (a chunk of a blocking call)
};

// What a frame carries from the start of its sorting stage to the end (registers; the LDS frame state does not grow).
struct SortCacheFrame {
  const SortCacheView* v = nullptr;
  int planner = 0;
  bool all_similar = false;  // cone_arrays_are_similar(cones_flat, cached cones_flat, 0.1), with an entry present
  int hit[2] = {-1, -1};
};

// threshold * threshold of the reference, in double: 0.010000000000000002
constexpr double CACHE_THR2 = 0.1 * 0.1;

// cone_arrays_are_similar for ONE current row against `m` cached rows (row stride 3): the smallest squared distance must
// be < 0.1 * 0.1 (np.min propagates a NaN, which fails), and the first row at that distance (np.argmin) must have the
// row's type.  Distances in my_cdist_sq_euclidean's expansion form (cdist_sq: NumPy's dot of the (m,6) / (6,n) operands
// is the same FMA chain for every shape that occurs here — one row or two, as for the n rows of a frame).
// CAST: the rows are a caller's cone rows, whose type column the sorting stage narrows on its way into the frame state
// (sort_frame: (uint8_t)(int)type); an entry's cone store holds the narrowed values already.
template <bool CAST = false>
__device__ __forceinline__ bool cache_row_similar(double x, double y, double t, const double* rows, int m) {
  double best = INFINITY;
  int arg = 0;
  bool nan = false;
  for (int j = 0; j < m; j++) {
    const double d = cdist_sq(x, y, rows[3 * j], rows[3 * j + 1]);
    nan = nan || d != d;
    if (d < best) {
      best = d;
      arg = j;
    }
  }
  if constexpr (CAST) return !nan && best < CACHE_THR2 && t == (double)(uint8_t)(int)rows[3 * arg + 2];
  return !nan && best < CACHE_THR2 && t == rows[3 * arg + 2];
}

// ---- fsdp_plan_sequence_cached (sequence_cache_kernel.h): what the speculative instantiation of the sorting kernels (SPEC) leaves
// per frame next to its SortOut — both sides searched fresh, each side's result as SortCacheHdr holds it BEFORE combine_sides — and
// what the chain kernel adds to it.  frame = step * n_planners + planner.
struct SeqSpecRec {
  int32_t n;             // cones the stage saw (0: more than the frame state holds)
  int32_t sim_prev;      // cone_arrays_are_similar(this frame's cones, the cones of frame - n_planners; step 0: the planner's entry)
  int32_t status[2];     // the side's own status; the right side is evaluated whatever the left one raised
  int32_t best_len[2];
  int32_t n_configs[2];
  int32_t first_k[2][2];  // starting cones (-1: none; both -1: the side returned before the cache check)
  double best_cost[2];
  int16_t best[2][MAX_LEN];
  // seq_cache_mark_kernel:
  int32_t hit[2];        // 1 / 0 / -1 as fsdp_sort_cache_hits defines them
  int32_t src[2];        // a hit side's result: the frame whose record holds it, -1: the planner's entry in front of the call
  int32_t resolved;      // the frame's sorting status with the cache on
  int32_t pad;
};
struct SeqSpecView {
  SeqSpecRec* rec = nullptr;
  int n_planners = 0;
  const SortCacheHdr* prev = nullptr;  // the planners' entries in front of the call (step 0's sim_prev)
  const double* prev_xyt = nullptr;
  const int32_t* prev_off = nullptr;
};

}  // namespace fsdp
