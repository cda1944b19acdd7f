// The kernels of fsdp_sort_batch_history (sort_history_kernels.h) and their launches: a translation unit, and so a code object,
// of their own next to fsdp_lib.hip, built into the same shared library.  It holds the history instantiations of the three
// sorting kernels and nothing else: sort_kernel.h leaves out its own kernels (FSDP_SORT_HISTORY_UNIT), which belong to
// fsdp_lib.hip — the code object of the kernels a pass launches does not grow by an instruction.
#include <hip/hip_runtime.h>

#define FSDP_SORT_HISTORY_UNIT 1
#include "sort_history_kernels.h"
#include "sort_history_launch.h"

extern "C" void fsdp_sort_hist_launch(hipStream_t stream, const fsdp_sort_hist_launch_args* a) {
  using namespace fsdp;
  hipLaunchKernelGGL((a->small ? sort_kernel_128_history : sort_kernel_history), dim3((unsigned)a->n_frames), dim3(WAVE), 0, stream, a->n_frames,
                     a->off, a->cones, a->poses, a->sorted, a->big, a->prm, a->view);
}

extern "C" void fsdp_sort_hist_launch_big(hipStream_t stream, const fsdp_sort_hist_launch_args* a) {
  using namespace fsdp;
  hipLaunchKernelGGL(sort_big_kernel_history, dim3((unsigned)a->big_blocks), dim3(WAVE), 0, stream, a->off, a->cones, a->poses, a->sorted,
                     (const int*)a->big, (SortSharedBig*)a->big_state, a->prm, a->view);
}
