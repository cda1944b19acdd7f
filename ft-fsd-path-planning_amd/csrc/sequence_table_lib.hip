// The TABLE twin of seq_chain_kernel (sequence_table_kernel.h) and its launch: a translation unit, and so a code object, of its own
// next to fsdp_lib.hip, built into the same shared library (__graft_entry__.py).  Nothing the earlier kernels are compiled from
// changes; the code object holds seq_chain_table_kernel and nothing else.
#include <hip/hip_runtime.h>

#define FSDP_SEQUENCE_UNIT 1   // (path_kernel.h: its kernels that are no templates belong to fsdp_lib.hip)
#define FSDP_SEQ_TABLE_UNIT 1  // (sequence_kernel.h, gpath_table_kernel.h: theirs belong to sequence_lib.hip and gpath_table_lib.hip)
#include "sequence_table_kernel.h"
#include "sequence_table_launch.h"

// The grid follows the head list like seq_chain_kernel's (grid-stride, one wavefront per SIMD at most).
extern "C" void fsdp_seqt_launch_chain(hipStream_t stream, const fsdp_seq_launch_args* a, const double* table_xy, const int32_t* table_off,
                                       int n_paths, const int32_t* ids) {
  using namespace fsdp;
  const long long n = (long long)a->n_planners * a->n_steps;
  const GpathTable t{table_xy, table_off, ids, n_paths};
  hipLaunchKernelGGL(seq_chain_table_kernel, dim3((unsigned)(n < 1024 ? n : 1024)), dim3(WAVE), 0, stream, a->n_planners, a->n_steps, a->poses,
                     a->matched, a->initial_prev, t, a->arena, a->out, a->seq, a->prm);
}
