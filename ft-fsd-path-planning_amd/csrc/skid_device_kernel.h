// Skidpad device tickets (fsdp_skidpad_submit_device, include/fsdp.h): what a skidpad step needs besides the way in of a device
// ticket (device_scan_kernel, device_gather_kernel: device_io_kernel.h, used as they are).  Two kernels, compiled in the device
// tickets' translation unit (device_io_lib.hip) and launched through skid_device_launch.h:
//
//   skid_device_reset_kernel  in front of the step's relocalization attempt: planner i with reset[i] != 0 becomes a fresh planner —
//                             the bytes fsdp_skidpad_reset writes for every planner (state zeroed, previous path = the context's
//                             default path); every other planner's state is not touched
//   skid_device_out_kernel    behind the step's path kernels: the step's PathOut and SkidInfo records as plain arrays in the
//                             caller's memory, and one word for the host: whether any planner is still not relocalized
//
// Pure data movement, one wavefront per planner and trip, grid-stride: no workgroup waits for another.
#pragma once

#include <stddef.h>

#include "device_io_kernel.h"
#include "skid_state.h"

namespace fsdp {

static_assert(offsetof(SkidState, prev) % 8 == 0 && offsetof(SkidState, prev) / 8 <= WAVE && sizeof(SkidState) == offsetof(SkidState, prev) + sizeof(double) * PATH_POINTS * 4,
              "skid_device_reset_kernel zeroes the state in front of prev as 8-byte words, one per lane, and prev ends the state");
static_assert(sizeof(SkidInfo) == 32 && sizeof(PathOut) % 8 == 0, "skid_device_out_kernel copies the records as 8-byte words");

struct SkidDeviceResetArgs {
  int n_inst;
  const int32_t* reset;        // the caller's mask (device memory), (n_inst)
  SkidState* states;           // the context's planners
  const double* default_path;  // the context's constant initial path (PATH_POINTS, 4)
};
__global__ void __launch_bounds__(256) skid_device_reset_kernel(SkidDeviceResetArgs a) {
  const int lane = (int)(threadIdx.x & 63), waves_per_block = (int)(blockDim.x >> 6);
  const long long wave0 = (long long)blockIdx.x * waves_per_block + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * waves_per_block;
  constexpr int HEAD_WORDS = (int)(offsetof(SkidState, prev) / 8);
  for (long long i = wave0; i < a.n_inst; i += n_waves) {
    if (a.reset[i] == 0) continue;
    SkidState* st = &a.states[i];
    if (lane < HEAD_WORDS) ((unsigned long long*)st)[lane] = 0ull;
    dio_copy(&st->prev[0][0], a.default_path, PATH_POINTS * 4, lane);
  }
}

struct SkidDeviceOutArgs {
  int n_inst;
  const PathOut* paths;    // the step's records (the slot's, written by skid_path_kernel or skid_commit_kernel)
  const SkidInfo* info;
  double* out_paths;       // the caller's arrays (device memory): (n_inst, PATH_POINTS, 4)
  int32_t* out_status;     // (n_inst)
  SkidInfo* out_info;      // (n_inst) in the layout of fsdp_skidpad_info, or NULL
  PathOut* out_records;    // (n_inst) in the layout of fsdp_path_result, or NULL
  int32_t* not_reloc;      // device view of one page-locked word the host zeroed: 1 when a planner is not relocalized after this step
};
// The status of a skidpad step is its path record's.  not_reloc: a relaxed system-scope store from one lane of every wavefront that
// meets such a planner (the same value from all of them), as device_scan_kernel writes bad_out.
__global__ void __launch_bounds__(256) skid_device_out_kernel(SkidDeviceOutArgs a) {
  const int lane = (int)(threadIdx.x & 63), waves_per_block = (int)(blockDim.x >> 6);
  const long long wave0 = (long long)blockIdx.x * waves_per_block + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * waves_per_block;
  constexpr long long ROW = PATH_POINTS * 4;
  for (long long i = wave0; i < a.n_inst; i += n_waves) {
    const PathOut* p = &a.paths[i];
    if (lane == 0) {
      a.out_status[i] = p->status;
      if (a.info[i].relocalized == 0) __hip_atomic_store(a.not_reloc, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    dio_copy(a.out_paths + i * ROW, &p->path[0][0], ROW, lane);
    if (a.out_info != nullptr && lane < (int)(sizeof(SkidInfo) / 8)) ((unsigned long long*)&a.out_info[i])[lane] = ((const unsigned long long*)&a.info[i])[lane];
    if (a.out_records != nullptr) dio_copy((double*)&a.out_records[i], (const double*)p, (long long)(sizeof(PathOut) / 8), lane);
  }
}

}  // namespace fsdp
