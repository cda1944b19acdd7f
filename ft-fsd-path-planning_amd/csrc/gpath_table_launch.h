// The seam between the host library (fsdp_lib.hip) and the TABLE twins of the path stage's wrappers (gpath_table_kernel.h), which are
// compiled as a translation unit of their own (gpath_table_lib.hip), like the device ticket kernels behind device_io_launch.h:
// every earlier kernel compiles to what it was.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace fsdp {
struct MatchOut;
struct PathOut;
struct PathMid;
struct Params;
}  // namespace fsdp

// One launch of a pass that carries path ids.  form: which wrapper — the one-kernel stage with a wavefront (64) or 16 lanes per frame, the
// first of the three kernels with 8 lanes per frame and 32 knots per fit (8), or the retry route (0: `blocks` workgroups walk the list).
struct fsdp_gpt_launch_args {
  int form;
  int n_frames;
  unsigned blocks;               // form 0 only
  const double* poses;
  const fsdp::MatchOut* matched;
  const double* default_path;
  const double* prev_paths;      // or NULL
  const double* table_xy;        // the context's table (device memory) ...
  const int32_t* table_off;
  int n_paths;
  const int32_t* ids;            // ... and the pass's ids: device memory, or the device view of page-locked host memory
  double* arena;
  fsdp::PathOut* out;
  fsdp::PathMid* mid;            // form 8 only
  int* retry;
  const fsdp::Params* prm;
};
// Weak: a library built from fsdp_lib.hip alone (the variant builds of tools/) has no such kernels, and fsdp_submit_paths says so.
extern "C" __attribute__((weak)) void fsdp_gpt_launch(hipStream_t stream, const fsdp_gpt_launch_args* a);
// path_ids_scan_kernel in front of a device ticket's pass: bad_frame is the device view of one page-locked word
extern "C" __attribute__((weak)) void fsdp_gpt_launch_ids_scan(hipStream_t stream, int n_frames, int n_paths, const int32_t* ids, int32_t* bad_frame);
