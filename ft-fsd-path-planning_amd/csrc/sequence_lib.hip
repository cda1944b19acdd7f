// The chain kernels of fsdp_plan_sequence (sequence_kernel.h) and their launches: a translation unit, and so a code object, of
// their own next to fsdp_lib.hip, built into the same shared library (__graft_entry__.py).  As part of fsdp_lib.hip's module a
// second user of the whole-wavefront path stage moved path_retry_kernel's register allocation; here nothing the earlier kernels
// are compiled from changes.  The code object holds the three chain kernels, the two staging kernels of a
// planner slice (fsdp_submit_sequence) and nothing else: path_kernel.h leaves out its kernels
// that are no templates (FSDP_SEQUENCE_UNIT), which belong to fsdp_lib.hip.
#include <hip/hip_runtime.h>

#define FSDP_SEQUENCE_UNIT 1
#include "sequence_kernel.h"

// The grid of seq_chain_kernel follows its list like path_retry_kernel's (grid-stride, one wavefront per SIMD at most).
extern "C" void fsdp_seq_launch(hipStream_t stream, const fsdp_seq_launch_args* a) {
  using namespace fsdp;
  const long long n = (long long)a->n_planners * a->n_steps;
  (void)hipMemsetAsync(a->seq, 0, sizeof(int) * SEQ_LIST, stream);
  hipLaunchKernelGGL(seq_mark_kernel, dim3((unsigned)((n + WAVE - 1) / WAVE)), dim3(WAVE), 0, stream, a->n_planners, a->n_steps,
                     (const PathOut*)a->out, a->seq);
  hipLaunchKernelGGL(seq_chain_kernel, dim3((unsigned)(n < 1024 ? n : 1024)), dim3(WAVE), 0, stream, a->n_planners, a->n_steps, a->poses, a->matched,
                     a->initial_prev, a->gpath, a->n_gpath, a->arena, a->out, a->seq, a->prm);
  hipLaunchKernelGGL(seq_final_kernel, dim3((unsigned)a->n_planners), dim3(WAVE), 0, stream, a->n_planners, a->n_steps, (const PathOut*)a->out,
                     a->initial_prev, a->final_prev, (const int*)a->seq, a->replanned_out);
}

// The first and the last step of fsdp_seq_launch on their own, for a pass whose chain kernel lives in another code object
// (sequence_table_lib.hip: a sequence with per-frame global paths).  Host code only: the kernels are the ones above.
extern "C" void fsdp_seq_launch_mark(hipStream_t stream, const fsdp_seq_launch_args* a) {
  using namespace fsdp;
  const long long n = (long long)a->n_planners * a->n_steps;
  (void)hipMemsetAsync(a->seq, 0, sizeof(int) * SEQ_LIST, stream);
  hipLaunchKernelGGL(seq_mark_kernel, dim3((unsigned)((n + WAVE - 1) / WAVE)), dim3(WAVE), 0, stream, a->n_planners, a->n_steps,
                     (const PathOut*)a->out, a->seq);
}
extern "C" void fsdp_seq_launch_final(hipStream_t stream, const fsdp_seq_launch_args* a) {
  using namespace fsdp;
  hipLaunchKernelGGL(seq_final_kernel, dim3((unsigned)a->n_planners), dim3(WAVE), 0, stream, a->n_planners, a->n_steps, (const PathOut*)a->out,
                     a->initial_prev, a->final_prev, (const int*)a->seq, a->replanned_out);
}

// The staging kernels of a planner slice.  In: the grid of stage_in_kernel (256 workgroups keep ~1 MB of loads on the wire).
// Out: stores towards host memory leave at the link's pace — the cap launch_assemble applies (128 workgroups).
extern "C" void fsdp_seq_launch_slice_in(hipStream_t stream, const fsdp_seq_slice_in_args* a) {
  hipLaunchKernelGGL(fsdp::seq_slice_in_kernel, dim3(256), dim3(256), 0, stream, *a);
}
extern "C" void fsdp_seq_launch_slice_out(hipStream_t stream, const fsdp_seq_slice_out_args* a) {
  long long blocks = (a->s.frames() + 3) / 4;  // one wavefront per record, four per workgroup
  blocks = blocks > 128 ? 128 : (blocks < 1 ? 1 : blocks);
  hipLaunchKernelGGL(fsdp::seq_slice_out_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, *a);
}
