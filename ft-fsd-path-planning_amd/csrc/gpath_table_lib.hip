// The TABLE twins of the path stage's wrappers (gpath_table_kernel.h) and their launches: a translation unit, and so a code object,
// of their own next to fsdp_lib.hip, built into the same shared library (__graft_entry__.py).  Nothing the earlier kernels are
// compiled from changes.
#include <hip/hip_runtime.h>

#define FSDP_SEQUENCE_UNIT 1  // (path_kernel.h: its kernels that are no templates belong to fsdp_lib.hip)
#include "gpath_table_kernel.h"
#include "gpath_table_launch.h"

extern "C" void fsdp_gpt_launch(hipStream_t stream, const fsdp_gpt_launch_args* a) {
  using namespace fsdp;
  const GpathTable t{a->table_xy, a->table_off, a->ids, a->n_paths};
  const int n = a->n_frames;
  if (a->form == 64)
    hipLaunchKernelGGL(path_table_kernel<PATH_G_SMALL>, dim3(n), dim3(WAVE), 0, stream, n, a->poses, a->matched, a->default_path, a->prev_paths, t, a->arena,
                       a->out, a->retry, a->prm);
  else if (a->form == 16)
    hipLaunchKernelGGL(path_table_kernel<PATH_G_LATENCY>, dim3((n + WAVE / PATH_G_LATENCY - 1) / (WAVE / PATH_G_LATENCY)), dim3(WAVE), 0, stream, n, a->poses,
                       a->matched, a->default_path, a->prev_paths, t, a->arena, a->out, a->retry, a->prm);
  else if (a->form == 8)
    hipLaunchKernelGGL((path_table_prep_kernel<PATH_G_SPLIT, WIDE_KNOTS>), dim3((n + WAVE / PATH_G_SPLIT - 1) / (WAVE / PATH_G_SPLIT)), dim3(WAVE), 0, stream, n,
                       a->poses, a->matched, a->default_path, a->prev_paths, t, a->arena, a->out, a->mid, a->retry, a->prm);
  else
    hipLaunchKernelGGL(path_table_retry_kernel, dim3(a->blocks), dim3(WAVE), 0, stream, a->poses, a->matched, a->default_path, a->prev_paths, t, a->arena,
                       a->out, a->retry, a->prm);
}

extern "C" void fsdp_gpt_launch_ids_scan(hipStream_t stream, int n_frames, int n_paths, const int32_t* ids, int32_t* bad_frame) {
  hipLaunchKernelGGL(fsdp::path_ids_scan_kernel, dim3(1), dim3(1024), 0, stream, n_frames, n_paths, ids, bad_frame);
}
