// The seam between the host library (fsdp_lib.hip) and the kernels of a skidpad device ticket (skid_device_kernel.h, and the way in
// of device_io_kernel.h), which are compiled in the device tickets' translation unit (device_io_lib.hip): every earlier kernel
// compiles to what it was.
#pragma once

#include "device_io_launch.h"

namespace fsdp {
struct SkidInfo;
struct SkidState;
}  // namespace fsdp

// In front of the step, on `stream`: skid_device_reset_kernel over the caller's mask.
struct fsdp_skid_dio_reset_args {
  int n_inst;
  const int32_t* reset;
  fsdp::SkidState* states;
  const double* default_path;
};
// Behind the step's path kernels: skid_device_out_kernel.
struct fsdp_skid_dio_out_args {
  int n_inst;
  const fsdp::PathOut* paths;  // the slot's records of the step
  const fsdp::SkidInfo* info;
  double* out_paths;           // the caller's arrays
  int32_t* out_status;
  fsdp::SkidInfo* out_info;    // or NULL
  fsdp::PathOut* out_records;  // or NULL
  int32_t* not_reloc;          // device view of one page-locked word
};
// Weak, like the launches of device_io_launch.h.  fsdp_skid_dio_launch_in: device_scan_kernel -> device_gather_kernel as
// fsdp_dio_launch_in launches them; with_cones = 0 (every planner is relocalized: the cones have no reader) gives the gather no
// room for cone rows, so that it moves the poses alone, while the scan still checks every count against cone_capacity.
extern "C" __attribute__((weak)) void fsdp_skid_dio_launch_reset(hipStream_t stream, const fsdp_skid_dio_reset_args* a);
extern "C" __attribute__((weak)) void fsdp_skid_dio_launch_in(hipStream_t stream, const fsdp_dio_in_args* a, int with_cones);
extern "C" __attribute__((weak)) void fsdp_skid_dio_launch_out(hipStream_t stream, const fsdp_skid_dio_out_args* a);
