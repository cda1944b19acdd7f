// Device tickets (fsdp_submit_device, include/fsdp.h): the way in and the way out of a pass whose batch and results live in the
// caller's GPU memory.  Three kernels, a translation unit of their own (device_io_lib.hip), launched through device_io_launch.h:
//
//   device_scan_kernel    counts (n) -> the slot's CSR offsets (n + 1), and the lowest frame whose count lies outside
//                         [0, cone_capacity] (or -1) into one word of the ticket's page-locked block
//   device_gather_kernel  the frames' first counts[f] rows of the (n, cone_capacity, 3) tensor -> the slot's gap-free cone rows;
//                         poses and previous paths into the slot's copies
//   device_out_kernel     behind the pass's assembly: status (n), paths (n, PATH_POINTS, 4) and the planners' next previous
//                         paths as plain arrays
//
// A count outside [0, cone_capacity] reads as 0 in both the scan and the gather (the same function: dio_count): nothing is read
// outside the caller's rows, and fsdp_collect reports the frame.  Pure data movement and one tiny scan: no workgroup waits for
// another, nothing spins; the kernels of a ticket are ordered by their stream alone.
#pragma once

#include "fsdp_device.h"

namespace fsdp {

constexpr int DIO_SCAN_CHUNK = 1024;  // counts per trip of device_scan_kernel (= its workgroup on the device: one count per lane)

__device__ __forceinline__ int dio_count(int32_t c, int cap) { return (c < 0 || c > cap) ? 0 : c; }

struct alignas(16) DioPair {
  double a, b;
};
// nd doubles from src to dst by the lanes of one wavefront: 16 bytes per lane where both are 16-byte aligned, 8 where not (a
// cone row is 24 bytes: whether a frame's rows start on a 16-byte border depends on the parity of the row index)
__device__ __forceinline__ void dio_copy(double* __restrict__ dst, const double* __restrict__ src, long long nd, int lane) {
  if ((((unsigned long long)src | (unsigned long long)dst) & 15ull) == 0) {
    const long long n2 = nd >> 1;
    for (long long k = lane; k < n2; k += WAVE) ((DioPair*)dst)[k] = ((const DioPair*)src)[k];
    if ((nd & 1) && lane == 0) dst[nd - 1] = src[nd - 1];
  } else {
    for (long long k = lane; k < nd; k += WAVE) dst[k] = src[k];
  }
}

// ONE workgroup (1024 lanes on the device, like filter_scan_kernel; any multiple of 64 that divides DIO_SCAN_CHUNK works — the host
// emulator runs 64, sixteen counts per lane): the exclusive prefix sum of the clamped counts, a chunk of DIO_SCAN_CHUNK per trip
// (lane t owns the chunk's counts [t * per, (t + 1) * per)), the running total carried from chunk to chunk.  Within a chunk: a
// shuffle scan inside every wavefront, the wavefronts' totals through LDS.  bad_out: the lowest frame with a count outside
// [0, cap], or -1 — one store at the end.
__global__ void __launch_bounds__(1024) device_scan_kernel(int n_frames, int cap, const int32_t* __restrict__ counts, int32_t* __restrict__ off,
                                                           int32_t* __restrict__ bad_out) {
  __shared__ int wave_total[16];
  __shared__ int wave_bad[16];
  const int t = (int)threadIdx.x, T = (int)blockDim.x, lane = t & 63, wave = t >> 6, n_waves = T >> 6;
  const int per = DIO_SCAN_CHUNK / T;
  int carry = 0, bad = 0x7fffffff;
  for (int base = 0; base < n_frames; base += DIO_SCAN_CHUNK) {
    const int lo = base + t * per;
    int own = 0;
    for (int j = 0; j < per; j++) {
      const int i = lo + j;
      if (i < n_frames) {
        const int32_t c = counts[i];
        if ((c < 0 || c > cap) && i < bad) bad = i;
        own += dio_count(c, cap);
      }
    }
    int incl = own;  // inclusive scan over the wavefront's lanes
    for (int d = 1; d < WAVE; d <<= 1) {
      const int up = __shfl_up(incl, (unsigned)d);
      if (lane >= d) incl += up;
    }
    if (lane == WAVE - 1) wave_total[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < n_waves; w++) {
      const int v = wave_total[w];
      if (w < wave) before += v;
      total += v;
    }
    __syncthreads();  // (the totals are read before the next trip writes them)
    int acc = carry + before + incl - own;
    for (int j = 0; j < per; j++) {
      const int i = lo + j;
      if (i < n_frames) {
        off[i] = acc;
        acc += dio_count(counts[i], cap);
      }
    }
    carry += total;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const int o = __shfl_xor(bad, d);
    bad = o < bad ? o : bad;
  }
  if (lane == 0) wave_bad[wave] = bad;
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < n_waves; w++) bad = wave_bad[w] < bad ? wave_bad[w] : bad;
    off[n_frames] = carry;
    if (bad_out != nullptr) __hip_atomic_store(bad_out, bad == 0x7fffffff ? -1 : bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

struct DeviceGatherArgs {
  int n_frames, cap;
  long long rows;            // cone rows the slot's d_cones holds for this pass (n_frames * cap): no store goes beyond
  const int32_t* counts;     // the caller's arrays (device memory)
  const double* cones;       // (n_frames, cap, 3) or NULL when cap = 0
  const double* poses;       // (n_frames, 4)
  const double* prev;        // (n_frames, PATH_POINTS, 4) or NULL
  const int32_t* off;        // the slot's offsets (device_scan_kernel)
  double* dst_cones;         // the slot's copies
  double* dst_poses;
  double* dst_prev;
};
// One wavefront per frame and trip, grid-stride (the manner of seq_slice_in_kernel): the frame's rows to their place in the
// gap-free cone array, its pose and, if given, its previous path.  The offset the scan wrote is clamped again to the copies' extent.
__global__ void __launch_bounds__(256) device_gather_kernel(DeviceGatherArgs a) {
  const int lane = (int)(threadIdx.x & 63), waves_per_block = (int)(blockDim.x >> 6);
  const long long wave0 = (long long)blockIdx.x * waves_per_block + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * waves_per_block;
  for (long long f = wave0; f < a.n_frames; f += n_waves) {
    long long d0 = a.off[f], cnt = dio_count(a.counts[f], a.cap);
    d0 = d0 < 0 ? 0 : (d0 > a.rows ? a.rows : d0);
    cnt = cnt > a.rows - d0 ? a.rows - d0 : cnt;
    if (lane < 4) a.dst_poses[4 * f + lane] = a.poses[4 * f + lane];
    if (cnt > 0) dio_copy(a.dst_cones + 3 * d0, a.cones + 3 * f * a.cap, 3 * cnt, lane);
    if (a.prev != nullptr) dio_copy(a.dst_prev + f * (PATH_POINTS * 4), a.prev + f * (PATH_POINTS * 4), PATH_POINTS * 4, lane);
  }
}

struct DeviceOutArgs {
  int n_frames;
  const SortOut* sorted;       // the pass's stage records
  const MatchOut* matched;
  const PathOut* paths;
  const double* prev;          // the slot's copy of the previous paths (device_gather_kernel), or NULL
  const double* default_path;  // the context's constant initial path (PATH_POINTS, 4)
  double* out_paths;           // the caller's arrays (device memory): (n_frames, PATH_POINTS, 4)
  int32_t* out_status;         // (n_frames)
  double* next_prev;           // (n_frames, PATH_POINTS, 4) or NULL; may be the array the gather read `prev` from
};
// One wavefront per frame and trip.  status: the latest stage that reported decides (assemble_kernel's rule).  next_prev: the new
// path when the status is 0, else the frame's previous path as the slot copied it, else the context's default path.
__global__ void __launch_bounds__(256) device_out_kernel(DeviceOutArgs a) {
  const int lane = (int)(threadIdx.x & 63), waves_per_block = (int)(blockDim.x >> 6);
  const long long wave0 = (long long)blockIdx.x * waves_per_block + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * waves_per_block;
  constexpr long long ROW = PATH_POINTS * 4;
  for (long long f = wave0; f < a.n_frames; f += n_waves) {
    int st = a.sorted[f].status;
    if (a.matched[f].status != 0) st = a.matched[f].status;
    if (a.paths[f].status != 0) st = a.paths[f].status;
    const double* path = &a.paths[f].path[0][0];
    if (lane == 0) a.out_status[f] = st;
    dio_copy(a.out_paths + f * ROW, path, ROW, lane);
    if (a.next_prev != nullptr) dio_copy(a.next_prev + f * ROW, st == ST_OK ? path : (a.prev != nullptr ? a.prev + f * ROW : a.default_path), ROW, lane);
  }
}

}  // namespace fsdp
