// TEST INFRASTRUCTURE — the kernels of a skidpad device ticket (csrc/skid_device_kernel.h: skid_device_reset_kernel,
// skid_device_out_kernel) under the host SIMT emulator, launched the way device_io_lib.hip launches them around a step.  The
// emulator runs workgroups of 64 lanes: one wavefront per workgroup instead of four.  Libraries of their own,
// libfsdp_emu_skid_device[_wide].so (skid_device.mk).  Never loaded by the package.
#include "hip_emu.h"

#include "../../ft-fsd-path-planning_amd/csrc/skid_device_kernel.h"

extern "C" {
int emu_skid_device_path_points() { return fsdp::PATH_POINTS; }
int emu_skid_state_bytes() { return (int)sizeof(fsdp::SkidState); }
int emu_skid_state_prev_offset() { return (int)offsetof(fsdp::SkidState, prev); }
int emu_skid_info_bytes() { return (int)sizeof(fsdp::SkidInfo); }
int emu_skid_path_out_bytes() { return (int)sizeof(fsdp::PathOut); }

// skid_device_reset_kernel over `states` (n_inst records of emu_skid_state_bytes() bytes); blocks: the grid (any grid walks any fleet)
void emu_skid_device_reset(int n_inst, const int32_t* reset, void* states, const double* default_path, int blocks) {
  fsdp::SkidDeviceResetArgs a;
  a.n_inst = n_inst;
  a.reset = reset;
  a.states = (fsdp::SkidState*)states;
  a.default_path = default_path;
  emu::launch((unsigned)(blocks > 0 ? blocks : 1), 64, [&]() { fsdp::skid_device_reset_kernel(a); });
}

// skid_device_out_kernel over the step's records (n_inst PathOut and SkidInfo records as bytes); out_info / out_records may be NULL.
// Returns the word the host zeroed before the launch.
int emu_skid_device_out(int n_inst, const void* path_records, const void* info_records, double* out_paths, int32_t* out_status, void* out_info,
                        void* out_records, int blocks) {
  int32_t word = 0;
  fsdp::SkidDeviceOutArgs a;
  a.n_inst = n_inst;
  a.paths = (const fsdp::PathOut*)path_records;
  a.info = (const fsdp::SkidInfo*)info_records;
  a.out_paths = out_paths;
  a.out_status = out_status;
  a.out_info = (fsdp::SkidInfo*)out_info;
  a.out_records = (fsdp::PathOut*)out_records;
  a.not_reloc = &word;
  emu::launch((unsigned)(blocks > 0 ? blocks : 1), 64, [&]() { fsdp::skid_device_out_kernel(a); });
  return word;
}
}
