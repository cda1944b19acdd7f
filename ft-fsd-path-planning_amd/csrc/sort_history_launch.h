// The seam between the host library (fsdp_lib.hip) and the history instantiations of the sorting kernels
// (sort_history_kernels.h), which are compiled as a translation unit of their own (sort_history_lib.hip).
#pragma once

#include <stdint.h>

#ifndef FSDP_EMU
#include <hip/hip_runtime.h>
#endif

#include "sort_history.h"  // SortHistView

namespace fsdp {
struct SortOut;
}  // namespace fsdp

#ifndef FSDP_EMU  // (the host emulator launches the kernels itself: tests/emu/emu_history.cpp)
struct fsdp_sort_hist_launch_args {
  int n_frames;
  const int32_t* off;  // the batch as the sorting stage plans it (filtered when use_unknown_cones = 0)
  const double* cones;
  const double* poses;
  fsdp::SortOut* sorted;
  int* big;         // the big route's list
  void* big_state;  // SortSharedBig blocks, `big_blocks` of them
  int big_blocks;
  bool small;       // no frame holds more than 128 cones
  const fsdp::Params* prm;
  fsdp::SortHistView view;
};
// sort_kernel_128_history | sort_kernel_history, and sort_big_kernel_history, on `stream`.  Weak: a library built from
// fsdp_lib.hip alone (the variant builds of tools/) has no history kernels, and fsdp_sort_batch_history says so.
extern "C" __attribute__((weak)) void fsdp_sort_hist_launch(hipStream_t stream, const fsdp_sort_hist_launch_args* a);
extern "C" __attribute__((weak)) void fsdp_sort_hist_launch_big(hipStream_t stream, const fsdp_sort_hist_launch_args* a);
#endif
