// The kernels of a device ticket (device_io_kernel.h; a skidpad context's: skid_device_kernel.h) and their launches: a translation unit, and so a code object, of their own
// next to fsdp_lib.hip, built into the same shared library (__graft_entry__.py).  Nothing the earlier kernels are compiled from
// changes.
#include <hip/hip_runtime.h>

#include "device_io_kernel.h"
#include "device_io_launch.h"
#include "skid_device_kernel.h"
#include "skid_device_launch.h"

// one wavefront per frame, four per workgroup, grid-stride beyond the cap launch_assemble applies to stores into device memory
static unsigned dio_blocks(int n_frames) {
  long long blocks = ((long long)n_frames + 3) / 4;
  return (unsigned)(blocks > 16384 ? 16384 : (blocks < 1 ? 1 : blocks));
}

// rows: the cone rows the gather may write (none: it moves poses and previous paths only)
static void dio_launch_in(hipStream_t stream, const fsdp_dio_in_args* a, long long rows) {
  using namespace fsdp;
  hipLaunchKernelGGL(device_scan_kernel, dim3(1), dim3(DIO_SCAN_CHUNK), 0, stream, a->n_frames, a->cone_capacity, a->counts, a->dst_off, a->bad_frame);
  DeviceGatherArgs g;
  g.n_frames = a->n_frames;
  g.cap = a->cone_capacity;
  g.rows = rows;
  g.counts = a->counts;
  g.cones = a->cones;
  g.poses = a->poses;
  g.prev = a->prev;
  g.off = a->dst_off;
  g.dst_cones = a->dst_cones;
  g.dst_poses = a->dst_poses;
  g.dst_prev = a->dst_prev;
  hipLaunchKernelGGL(device_gather_kernel, dim3(dio_blocks(a->n_frames)), dim3(256), 0, stream, g);
}

extern "C" void fsdp_dio_launch_in(hipStream_t stream, const fsdp_dio_in_args* a) { dio_launch_in(stream, a, (long long)a->n_frames * a->cone_capacity); }

extern "C" void fsdp_dio_launch_out(hipStream_t stream, const fsdp_dio_out_args* a) {
  using namespace fsdp;
  DeviceOutArgs o;
  o.n_frames = a->n_frames;
  o.sorted = a->sorted;
  o.matched = a->matched;
  o.paths = a->paths;
  o.prev = a->prev;
  o.default_path = a->default_path;
  o.out_paths = a->out_paths;
  o.out_status = a->out_status;
  o.next_prev = a->next_prev;
  hipLaunchKernelGGL(device_out_kernel, dim3(dio_blocks(a->n_frames)), dim3(256), 0, stream, o);
}

// ---- skidpad device tickets (skid_device_kernel.h) ----
extern "C" void fsdp_skid_dio_launch_reset(hipStream_t stream, const fsdp_skid_dio_reset_args* a) {
  using namespace fsdp;
  SkidDeviceResetArgs r;
  r.n_inst = a->n_inst;
  r.reset = a->reset;
  r.states = a->states;
  r.default_path = a->default_path;
  hipLaunchKernelGGL(skid_device_reset_kernel, dim3(dio_blocks(a->n_inst)), dim3(256), 0, stream, r);
}

extern "C" void fsdp_skid_dio_launch_in(hipStream_t stream, const fsdp_dio_in_args* a, int with_cones) {
  dio_launch_in(stream, a, with_cones ? (long long)a->n_frames * a->cone_capacity : 0);
}

extern "C" void fsdp_skid_dio_launch_out(hipStream_t stream, const fsdp_skid_dio_out_args* a) {
  using namespace fsdp;
  SkidDeviceOutArgs o;
  o.n_inst = a->n_inst;
  o.paths = a->paths;
  o.info = a->info;
  o.out_paths = a->out_paths;
  o.out_status = a->out_status;
  o.out_info = a->out_info;
  o.out_records = a->out_records;
  o.not_reloc = a->not_reloc;
  hipLaunchKernelGGL(skid_device_out_kernel, dim3(dio_blocks(a->n_inst)), dim3(256), 0, stream, o);
}
