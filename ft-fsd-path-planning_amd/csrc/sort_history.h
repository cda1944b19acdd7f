// Search history of the sorting stage (include/fsdp.h fsdp_sort_batch_history): what the reference hands to the callers of
//   calc_scores_and_end_configurations(..., return_history=True)     find_configs_and_scores.py:41,96
//   _impl_find_all_end_configurations(store_all_end_configurations)  end_configurations.py:358-361,411-429
// — every configuration the depth-first search visited, in visiting order, and whether it was an end configuration — plus what
// the reference leaves to reading its code: for every neighbour of the popped cone the first predicate of
// neighbor_bool_mask_can_be_added_to_attempt (:108-223) that rejected it.  The history instantiations of the sorting kernels
// (sort_kernel.h, template flag HIST) record one row per pop of sort_dfs_both.
#pragma once

#include "fsdp_device.h"

namespace fsdp {

// = the FSDP_CAND_* codes of include/fsdp.h, in the order the reference evaluates the predicates
enum CandVerdict {
  CAND_ADDED = 0,
  CAND_IN_ATTEMPT = 1,
  CAND_OUTSIDE_ELLIPSE = 2,
  CAND_WRONG_SIDE = 3,
  CAND_SKIPS_NEIGHBOUR = 4,
  CAND_ABSOLUTE_ANGLE = 5,
  CAND_DIRECTIONAL_ANGLE = 6,
  CAND_ZIGZAG = 7,
  CAND_BEHIND_START = 8,
  CAND_CROSSES_CAR = 9
};

// The outputs of a call (device memory).  The host fills rows / cand with 0xFF bytes (-1 indices), is_end / verdict with 0xFF
// and the two count arrays with zeros in front of the kernels: a side that is not searched writes nothing.
struct SortHistView {
  int rows_cap = 0;
  int32_t* n_rows = nullptr;         // (n_frames, 2) rows visited, never truncated
  int32_t* target_length = nullptr;  // (n_frames, 2)
  int32_t* rows = nullptr;           // (n_frames, 2, rows_cap, MAX_LEN)
  uint8_t* is_end = nullptr;         // (n_frames, 2, rows_cap)
  int32_t* cand = nullptr;           // (n_frames, 2, rows_cap, KNN) or NULL ...
  uint8_t* verdict = nullptr;        // ... together with the codes
};

// What a frame's wavefront carries through the stage (registers).  Nothing of the history lives in the frame state.
struct SortHistFrame {
  const SortHistView* v = nullptr;
  int frame = 0;
};

// One pop of one side's search: called by the 32 lanes of the side (sl = lane within the side), `row` = pops of this side so far
// (side-uniform).  A row at or beyond rows_cap is counted by the caller and not stored.  Lanes sl < MAX_LEN store the attempt
// from consecutive lanes, lane 0 the end flag, lanes sl < n_nb the neighbour and its code.
__device__ __forceinline__ void sort_hist_store(const SortHistFrame& h, int side, int sl, int row, const int16_t* attempt, bool is_end,
                                                int n_nb, int nb, int code) {
  const SortHistView& v = *h.v;
  if (row >= v.rows_cap) return;
  const size_t at = (size_t)(2 * h.frame + side) * (size_t)v.rows_cap + (size_t)row;
  if (sl < MAX_LEN) v.rows[at * MAX_LEN + sl] = (int32_t)attempt[sl];
  if (sl == 0) v.is_end[at] = is_end ? 1 : 0;
  if (v.cand != nullptr && sl < n_nb) {
    v.cand[at * KNN + sl] = (int32_t)nb;
    v.verdict[at * KNN + sl] = (uint8_t)code;
  }
}

// End of a side's search: the counts (a side that was never popped reports 0 / 0).
__device__ __forceinline__ void sort_hist_close(const SortHistFrame& h, int side, int n_rows, int target_length) {
  const SortHistView& v = *h.v;
  v.n_rows[2 * (size_t)h.frame + side] = n_rows;
  v.target_length[2 * (size_t)h.frame + side] = n_rows > 0 ? target_length : 0;
}

}  // namespace fsdp
