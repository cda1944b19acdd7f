// The ranked instantiations of the sorting kernels (sort_kernel.h, template flag RANKED; sort_rank.h).  A header of its own,
// included after every other kernel: the code object keeps the kernels that existed before in the order they had.
#pragma once

#include "sort_kernel.h"

namespace fsdp {

// ---- the same three kernels reporting the ranked end configurations (sort_rank.h): launched only by fsdp_sort_batch_ranked; the
// cost terms wait for the ranking in a block of their own (LDS here, global memory for sort_big_kernel_ranked), never in the
// frame state.  No sorting cache: a hit has no candidates to report. ----
using SortRankScratch = SortRankScratchT<MAX_ENDS>;
using SortRankScratchBig = SortRankScratchT<BIG_ENDS>;
__global__ void __launch_bounds__(64) sort_kernel_ranked(int n_frames, const int32_t* __restrict__ cone_offsets, const double* __restrict__ cones_xyt,
                                                         const double* __restrict__ poses, SortOut* __restrict__ out, int* __restrict__ big,
                                                         const Params* __restrict__ prm, SortRankView rank) {
  __shared__ SortShared S;
  __shared__ SortRankScratch R;
  SortRankFrame rk;
  rk.v = &rank;
  rk.terms = &R.terms[0][0];
  rk.order = R.order;
  sort_kernel_body<SortShared, false, true>(S, n_frames, cone_offsets, cones_xyt, poses, out, big, prm, StageIn(), nullptr, &rk);
}
__global__ void __launch_bounds__(64) sort_kernel_128_ranked(int n_frames, const int32_t* __restrict__ cone_offsets,
                                                             const double* __restrict__ cones_xyt, const double* __restrict__ poses,
                                                             SortOut* __restrict__ out, int* __restrict__ big, const Params* __restrict__ prm,
                                                             SortRankView rank) {
  __shared__ SortShared128 S;
  __shared__ SortRankScratch R;
  SortRankFrame rk;
  rk.v = &rank;
  rk.terms = &R.terms[0][0];
  rk.order = R.order;
  sort_kernel_body<SortShared128, false, true>(S, n_frames, cone_offsets, cones_xyt, poses, out, big, prm, StageIn(), nullptr, &rk);
}
// (a frame of this route can hold up to 4096 configurations after the post filters; still only top_k rows are stored)
__global__ void __launch_bounds__(64) sort_big_kernel_ranked(const int32_t* __restrict__ cone_offsets, const double* __restrict__ cones_xyt,
                                                             const double* __restrict__ poses, SortOut* __restrict__ out,
                                                             const int* __restrict__ big, SortSharedBig* __restrict__ state,
                                                             const Params* __restrict__ prm, SortRankView rank,
                                                             SortRankScratchBig* __restrict__ scratch) {
  const int n = big[0];
  SortSharedBig& S = state[blockIdx.x];
  SortRankScratchBig& R = scratch[blockIdx.x];
  SortRankFrame rk;
  rk.v = &rank;
  rk.terms = &R.terms[0][0];
  rk.order = R.order;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    sort_frame<SortSharedBig, false, true>(S, *prm, big[1 + i], cone_offsets, cones_xyt, poses, out, StageIn(), nullptr, &rk);
    __syncthreads();
  }
}

}  // namespace fsdp
