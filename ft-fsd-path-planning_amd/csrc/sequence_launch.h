// The seam between the host library (fsdp_lib.hip) and the chain kernels of a sequence pass (sequence_kernel.h), which are
// compiled as a translation unit of their own (sequence_lib.hip).
#pragma once

#include <stdint.h>

#ifndef FSDP_EMU
#include <hip/hip_runtime.h>
#endif

namespace fsdp {
struct MatchOut;
struct PathOut;
struct Params;
// the list block of a sequence pass: [0] heads appended, [1] frames planned again (a 16-byte header, zeroed by one memset per
// pass), then (frame, predecessor) per head: SEQ_LIST + 2 * frames ints
constexpr int SEQ_HEADS = 0, SEQ_REPLANNED = 1, SEQ_LIST = 4;
}  // namespace fsdp

#ifndef FSDP_EMU  // (the host emulator launches the kernels itself: tests/emu/emu_sequence.cpp)
struct fsdp_seq_launch_args {
  int n_planners, n_steps;
  const double* poses;
  const fsdp::MatchOut* matched;
  const double* initial_prev;  // (n_planners, PATH_POINTS, 4) or NULL
  const double* gpath;
  int n_gpath;
  double* arena;
  fsdp::PathOut* out;
  int* seq;                // the list block
  double* final_prev;      // (n_planners, PATH_POINTS, 4)
  int32_t* replanned_out;  // device view of the pass trailer's spare word
  const fsdp::Params* prm;
};
// header memset -> seq_mark_kernel -> seq_chain_kernel -> seq_final_kernel on `stream`.  Weak: a library built from fsdp_lib.hip
// alone (the variant builds of tools/) has no sequence kernels, and fsdp_plan_sequence says so.
extern "C" __attribute__((weak)) void fsdp_seq_launch(hipStream_t stream, const fsdp_seq_launch_args* a);
#endif
