// Ranked end configurations of the sorting stage (include/fsdp.h fsdp_sort_batch_ranked): what the reference hands to the
// callers of
//   calc_scores_and_end_configurations             find_configs_and_scores.py:29-112  (costs, configurations) in cost order
//   cost_configurations(return_individual_costs=True)   cost_function.py:283-302      the seven weighted cost columns
// and what the product kernels compute and drop once they have picked the winner.  The ranked instantiations of the sorting
// kernels (sort_kernel.h, template flag RANKED) keep it: per frame and side the number of configurations after the post
// filters, and the first top_k of them in ascending (cost, row) order with their costs and cost terms.
#pragma once

#include "fsdp_device.h"

namespace fsdp {

constexpr int RANK_MAX = 64;    // = FSDP_RANK_MAX: rows per side a call can ask for (the LDS route's raw end-configuration capacity)
constexpr int COST_TERMS = 7;   // = FSDP_COST_TERMS: cost_function.py:287-296 column order

// The outputs of a call (device memory).  The host fills configs / costs / terms with 0xFF bytes (-1 indices, NaNs) and
// counts with zeros in front of the kernels: a side without a result writes nothing.
struct SortRankView {
  int top_k = 0;
  int32_t* counts = nullptr;    // (n_frames, 2)
  int32_t* configs = nullptr;   // (n_frames, 2, top_k, MAX_LEN)
  double* costs = nullptr;      // (n_frames, 2, top_k)
  double* terms = nullptr;      // (n_frames, 2, top_k, COST_TERMS) or NULL
};

// Where a frame's cost terms wait for the ranking, and the ranking itself.  NOT part of the sorting stage's frame state
// (SortSharedT): the ranked LDS kernels declare one of their own next to it, sort_big_kernel_ranked gets one per block in
// global memory — the frame state of the kernels without the ranking does not grow by a byte.
template <int ENDS_>
struct SortRankScratchT {
  double terms[ENDS_][COST_TERMS];  // per raw configuration, written by the cost step's lane a == 0
  int32_t order[RANK_MAX];          // order[r] = raw configuration of rank r
};

// What a frame's wavefront carries through the stage (registers).
struct SortRankFrame {
  const SortRankView* v = nullptr;
  int frame = 0;
  double* terms = nullptr;   // SortRankScratchT::terms, flat
  int32_t* order = nullptr;  // SortRankScratchT::order
};

// The ranking of one side, after its argmin (cost / keep are shared by the sides: the next side overwrites them).
// Lanes = kept configurations in chunks of 64, as in the post filters: a lane's rank is the number of kept configurations in
// front of it under (cost, -1 padded row) — the order of np.argsort over np.unique's rows, which is the argmin's own tie rule
// (sort_side_finish), so rank 0 is the side's winner.  Rows are distinct after np.unique, hence the ranks are a permutation
// (a NaN cost sorts behind every number, like np.argsort).  Then the first min(C, top_k) rows go out element by element:
// consecutive lanes store consecutive words of the frame's output block.
template <class SH>
__device__ inline void sort_rank_side(const SH& S, const SortRankFrame& rk, int side, int n_ends, int C) {
  const int lane = lane_id();
  const SortRankView& v = *rk.v;
  const int K = v.top_k;
  const int rows = C < K ? C : K;
  for (int c0 = 0; c0 < n_ends; c0 += WAVE) {
    const int c = c0 + lane;
    if (c < n_ends && S.keep[c]) {
      int16_t mine[MAX_LEN];  // static indexing only (fully unrolled loops): registers
#pragma unroll
      for (int l = 0; l < MAX_LEN; l++) mine[l] = S.ends[side][c][l];
      const double mc = S.cost[c];
      const bool mnan = mc != mc;
      int rank = 0;
      for (int o = 0; o < n_ends; o++) {
        if (o == c || !S.keep[o]) continue;
        const double oc = S.cost[o];
        const bool onan = oc != oc;
        bool before = !onan && (mnan || oc < mc);
        if ((onan && mnan) || oc == mc) {
          bool decided = false;
#pragma unroll
          for (int l = 0; l < MAX_LEN; l++) {
            const int16_t b = S.ends[side][o][l];
            if (!decided && b != mine[l]) {
              before = b < mine[l];
              decided = true;
            }
          }
        }
        rank += before ? 1 : 0;
      }
      if (rank < K) rk.order[rank] = c;
    }
  }
  __syncthreads();
  const size_t block = (size_t)(2 * rk.frame + side) * (size_t)K;
  int32_t* cfg = v.configs + block * MAX_LEN;
  for (int e = lane; e < rows * MAX_LEN; e += WAVE) {
    const int r = e / MAX_LEN, l = e - r * MAX_LEN;
    cfg[e] = (int32_t)S.ends[side][rk.order[r]][l];
  }
  double* co = v.costs + block;
  for (int e = lane; e < rows; e += WAVE) co[e] = S.cost[rk.order[e]];
  if (v.terms != nullptr) {
    double* tr = v.terms + block * COST_TERMS;
    for (int e = lane; e < rows * COST_TERMS; e += WAVE) {
      const int r = e / COST_TERMS, t = e - r * COST_TERMS;
      tr[e] = rk.terms[(size_t)rk.order[r] * COST_TERMS + t];
    }
  }
  __syncthreads();
}

// End of a frame: the counts, and — a frame whose status is not 0 reports nothing — the padding again over whatever a side wrote
// before the frame failed (all-ones words: -1 indices, the NaN the host's fill leaves).
__device__ inline void sort_rank_close(const SortRankFrame& rk, int status, int n_left, int n_right) {
  const int lane = lane_id();
  const SortRankView& v = *rk.v;
  if (lane < 2) v.counts[2 * (size_t)rk.frame + lane] = status == ST_OK ? (lane == 0 ? n_left : n_right) : 0;
  if (status == ST_OK) return;
  const size_t block = (size_t)(2 * rk.frame) * (size_t)v.top_k;  // both sides: 2 * top_k rows
  const int rows = 2 * v.top_k;
  int32_t* cfg = v.configs + block * MAX_LEN;
  for (int e = lane; e < rows * MAX_LEN; e += WAVE) cfg[e] = -1;
  int32_t* co = reinterpret_cast<int32_t*>(v.costs + block);
  for (int e = lane; e < rows * 2; e += WAVE) co[e] = -1;
  if (v.terms != nullptr) {
    int32_t* tr = reinterpret_cast<int32_t*>(v.terms + block * COST_TERMS);
    for (int e = lane; e < rows * COST_TERMS * 2; e += WAVE) tr[e] = -1;
  }
}

}  // namespace fsdp
