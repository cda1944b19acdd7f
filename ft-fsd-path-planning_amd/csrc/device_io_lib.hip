// The kernels of a device ticket (device_io_kernel.h) and their launches: a translation unit, and so a code object, of their own
// next to fsdp_lib.hip, built into the same shared library (__graft_entry__.py).  Nothing the earlier kernels are compiled from
// changes.
#include <hip/hip_runtime.h>

#include "device_io_kernel.h"
#include "device_io_launch.h"

// one wavefront per frame, four per workgroup, grid-stride beyond the cap launch_assemble applies to stores into device memory
static unsigned dio_blocks(int n_frames) {
  long long blocks = ((long long)n_frames + 3) / 4;
  return (unsigned)(blocks > 16384 ? 16384 : (blocks < 1 ? 1 : blocks));
}

extern "C" void fsdp_dio_launch_in(hipStream_t stream, const fsdp_dio_in_args* a) {
  using namespace fsdp;
  hipLaunchKernelGGL(device_scan_kernel, dim3(1), dim3(DIO_SCAN_CHUNK), 0, stream, a->n_frames, a->cone_capacity, a->counts, a->dst_off, a->bad_frame);
  DeviceGatherArgs g;
  g.n_frames = a->n_frames;
  g.cap = a->cone_capacity;
  g.rows = (long long)a->n_frames * a->cone_capacity;
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
