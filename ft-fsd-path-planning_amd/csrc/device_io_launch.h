// The seam between the host library (fsdp_lib.hip) and the kernels of a device ticket (device_io_kernel.h), which are compiled as
// a translation unit of their own (device_io_lib.hip), like the sequence kernels behind sequence_launch.h: every earlier kernel
// compiles to what it was.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace fsdp {
struct MatchOut;
struct PathOut;
struct SortOut;
}  // namespace fsdp

// In front of the pass, on `stream`: device_scan_kernel -> device_gather_kernel.  The first five pointers are the caller's device
// arrays; the rest the slot's copies, with room for n_frames * cone_capacity cone rows.
struct fsdp_dio_in_args {
  int n_frames, cone_capacity;
  const int32_t* counts;
  const double* cones;   // NULL when cone_capacity = 0
  const double* poses;
  const double* prev;    // or NULL
  int32_t* bad_frame;    // device view of one page-locked word: the lowest frame with a count outside [0, cone_capacity], or -1
  int32_t* dst_off;
  double* dst_cones;
  double* dst_poses;
  double* dst_prev;
};
// Behind the pass's assembly: device_out_kernel.
struct fsdp_dio_out_args {
  int n_frames;
  const fsdp::SortOut* sorted;
  const fsdp::MatchOut* matched;
  const fsdp::PathOut* paths;
  const double* prev;          // the slot's copy, or NULL
  const double* default_path;
  double* out_paths;
  int32_t* out_status;
  double* next_prev;           // or NULL
};
// Weak: a library built from fsdp_lib.hip alone (the variant builds of tools/) has no such kernels, and fsdp_submit_device says so.
extern "C" __attribute__((weak)) void fsdp_dio_launch_in(hipStream_t stream, const fsdp_dio_in_args* a);
extern "C" __attribute__((weak)) void fsdp_dio_launch_out(hipStream_t stream, const fsdp_dio_out_args* a);
