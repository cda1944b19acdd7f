// The history instantiations of the sorting kernels (sort_kernel.h, template flag HIST; sort_history.h): launched only by
// fsdp_sort_batch_history, compiled by sort_history_lib.hip into a code object of their own.  The frame state is the plain
// kernels'; the history goes straight from the search's registers to the call's arrays.  No sorting cache: a hit has no search.
#pragma once

#include "sort_kernel.h"

namespace fsdp {

__global__ void __launch_bounds__(64) sort_kernel_history(int n_frames, const int32_t* __restrict__ cone_offsets, const double* __restrict__ cones_xyt,
                                                          const double* __restrict__ poses, SortOut* __restrict__ out, int* __restrict__ big,
                                                          const Params* __restrict__ prm, SortHistView hist) {
  __shared__ SortShared S;
  SortHistFrame hf;
  hf.v = &hist;
  sort_kernel_body<SortShared, false, false, true>(S, n_frames, cone_offsets, cones_xyt, poses, out, big, prm, StageIn(), nullptr, nullptr, &hf);
}
__global__ void __launch_bounds__(64) sort_kernel_128_history(int n_frames, const int32_t* __restrict__ cone_offsets,
                                                              const double* __restrict__ cones_xyt, const double* __restrict__ poses,
                                                              SortOut* __restrict__ out, int* __restrict__ big, const Params* __restrict__ prm,
                                                              SortHistView hist) {
  __shared__ SortShared128 S;
  SortHistFrame hf;
  hf.v = &hist;
  sort_kernel_body<SortShared128, false, false, true>(S, n_frames, cone_offsets, cones_xyt, poses, out, big, prm, StageIn(), nullptr, nullptr, &hf);
}
// (a frame handed over by the LDS kernels is traced again from its first pop: the rows it left there are a prefix of these)
__global__ void __launch_bounds__(64) sort_big_kernel_history(const int32_t* __restrict__ cone_offsets, const double* __restrict__ cones_xyt,
                                                              const double* __restrict__ poses, SortOut* __restrict__ out,
                                                              const int* __restrict__ big, SortSharedBig* __restrict__ state,
                                                              const Params* __restrict__ prm, SortHistView hist) {
  const int n = big[0];
  SortSharedBig& S = state[blockIdx.x];
  SortHistFrame hf;
  hf.v = &hist;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    sort_frame<SortSharedBig, false, false, false, true>(S, *prm, big[1 + i], cone_offsets, cones_xyt, poses, out, StageIn(), nullptr, nullptr, nullptr, &hf);
    __syncthreads();
  }
}

}  // namespace fsdp
