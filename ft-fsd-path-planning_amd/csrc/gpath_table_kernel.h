// Per-frame global paths (fsdp_set_global_path_table, fsdp_submit_paths, fsdp_submit_device_paths; include/fsdp.h): the TABLE twins of
// the path stage's kernel wrappers that hand a global path to path_front / path_frame — path_kernel<64> / <16>, path_prep_kernel<8,
// WIDE_KNOTS> and path_retry_kernel (path_kernel.h).  A twin resolves the pair (gpath, n_gpath) per frame, once the frame index is
// known, from the context's path table and the pass's ids instead of taking it from the launch arguments; everything below the
// wrapper (path_front, path_frame, the fits) is the same code.  fit_kernel and path_finish_kernel read no global path: a pass with
// ids launches the plain ones.
//
// KEEP EACH TWIN THE SAME AS ITS PLAIN WRAPPER, statement for statement, but for the lookup.  They are bodies of their own, in a
// translation unit and code object of their own (gpath_table_lib.hip, launched through gpath_table_launch.h), because a flag on the
// plain wrappers — a template parameter, or a shared body — changes their names or moved their register allocation, and the earlier
// kernels are to compile to exactly what they were (tools/kernel_code_diff.py).  tests/test_gpath_table_cpu.py and
// tests/test_gpath_table_gpu.py hold the twins against the plain route: one context per path.
//
// Divergence inside a wavefront.  With a context-wide path every lane group of a wavefront took the same side of path_front's
// `gpath != nullptr` with the same n_gpath.  Here the groups (8 or 16 lanes per frame; the retry kernel's four frames per wavefront)
// hold different pairs: some run the window loops, with different trip counts, some select_side_to_use.  That is the divergence
// BETWEEN groups device_prims.h allows, and nothing in path_front reaches across a group: Grp<G>::ballot keeps the group's own bits
// of the wavefront's mask (the inactive lanes of other groups read as 0 there, and are shifted out anyway); argmin's and bcast's
// exchanges name lanes of the aligned group only, all of which are active together, since the lanes of a group resolve the same frame
// and so the same pair; sync() of a group smaller than the wavefront is a fence and a scheduling barrier, no s_barrier.  The
// pointers are per-lane values (VGPRs): every read of a path is a vector load.  The tests put a cone-planned frame, a short, a long,
// an empty and an overfull path into the same wavefront on every route.
#pragma once

#include "path_kernel.h"

namespace fsdp {

// the table and a pass's ids as the kernels take them
struct GpathTable {
  const double* xy;     // n_paths polylines one behind the other, (off[n_paths], 2); never NULL, also when every entry is empty
  const int32_t* off;   // (n_paths + 1), off[0] = 0, non-decreasing: path k is the points [off[k], off[k + 1])
  const int32_t* ids;   // (n_frames): device memory, or the device view of page-locked host memory
  int n_paths;
};
// ids[frame] = k >= 0: the frame follows path k (an empty one keeps a pointer: path_front answers 103, the argmin of an empty array);
// -1, and whatever else names no path (a device ticket's ids are checked by path_ids_scan_kernel only): no global path, the frame
// plans from its matches
__device__ __forceinline__ void table_lookup(const GpathTable& t, int frame, const double*& gpath, int& n_gpath) {
  const int32_t id = t.ids[frame];
  const bool named = id >= 0 && id < t.n_paths;
  const int32_t lo = named ? t.off[id] : 0;
  gpath = named ? t.xy + 2 * (size_t)lo : nullptr;
  n_gpath = named ? t.off[id + 1] - lo : 0;
}

// path_kernel<G> (FAST)
template <int G>
__global__ void __launch_bounds__(64, PATH_WAVES) path_table_kernel(int n_frames, const double* __restrict__ poses, const MatchOut* __restrict__ matched,
                                                                    const double* __restrict__ default_path, const double* __restrict__ prev_paths,
                                                                    GpathTable table, double* __restrict__ arena, PathOut* __restrict__ out,
                                                                    int* __restrict__ retry, const Params* __restrict__ prm) {
  __shared__ PathShared<G, false, G == WAVE ? NK_BIG : 0> S_all[WAVE / G];  // (a frame with the wavefront to itself: 256 knots)
  const int frame = blockIdx.x * (WAVE / G) + Grp<G>::index();
  if (frame < n_frames) {
    const double* gpath;
    int n_gpath;
    table_lookup(table, frame, gpath, n_gpath);
    path_frame<G, true>(S_all[Grp<G>::index()], frame, poses, matched, default_path, prev_paths, gpath, n_gpath, arena, out, prm);
    if (retry != nullptr && Grp<G>::lane() == 0 && (out[frame].status == ST_OVERFLOW_KNOTS || out[frame].status == ST_RETRY))
      retry[1 + atomicAdd(&retry[0], 1)] = frame;
  }  // (retry list on the device: used by the emulator harness; the library collects the list on the host)
}

// path_prep_kernel<G, NKC>
template <int G, int NKC>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) path_table_prep_kernel(int n_frames, const double* __restrict__ poses, const MatchOut* __restrict__ matched,
                                                                                                     const double* __restrict__ default_path, const double* __restrict__ prev_paths,
                                                                                                     GpathTable table, double* __restrict__ arena, PathOut* __restrict__ out,
                                                                                                     PathMid* __restrict__ mid, int* __restrict__ retry, const Params* __restrict__ prm) {
  using GR = Grp<G>;
  __shared__ PathShared<G, true, NKC> S_all[WAVE / G];
  const int frame = blockIdx.x * (WAVE / G) + GR::index();
  if (frame < n_frames) {
    PathShared<G, true, NKC>& S = S_all[GR::index()];
    const Arena A = frame_arena(arena, frame, prm);
    const double px = poses[4 * frame + 0], py = poses[4 * frame + 1], dx = poses[4 * frame + 2], dy = poses[4 * frame + 3];
    const double* prev = prev_paths ? prev_paths + (size_t)frame * (PATH_POINTS * 4) : default_path;
    const double* gpath;
    int n_gpath;
    table_lookup(table, frame, gpath, n_gpath);
    int fallback = 0, n1 = 0, off = 0, n = 0;
    int status = path_front<G, true, true>(S, A, &matched[frame], px, py, prev, gpath, n_gpath, &fallback, &n1);
    bool plain = false;
    if (status == ST_OK && n1 > 0) {
      n1 = overwrite_if_too_far<G>(A, n1, px, py, prev, &fallback);
      const int rc = mpc_prepare<G>(S, A, n1, px, py, dx, dy, &fallback, &off, &n);
      plain = rc == 0 && n >= 4;  // degree 3 needs 4 points; everything else takes the exact route
      if (plain) build_parameter<G>(S, A, off, n);
    }
    const bool final_status = status != ST_OK && status != ST_RETRY && status != ST_OVERFLOW_KNOTS;
    if (final_status) write_path_status<G>(&out[frame], status, fallback, 0);  // sorting / matching / fit #1 decided the frame
    if (GR::lane() == 0) {
      PathMid m;
      m.status = plain ? ST_OK : (final_status ? status : ST_RETRY);
      m.fallback = fallback;
      m.off = off;
      m.n = n;
      mid[frame] = m;
      if (!plain && !final_status) push_retry(retry, frame);
    }
  }
}

// (FSDP_SEQ_TABLE_UNIT: csrc/sequence_table_lib.hip compiles this header for table_lookup alone — the kernels below, which are no
// templates, belong to gpath_table_lib.hip)
#ifndef FSDP_SEQ_TABLE_UNIT
// path_retry_kernel: four frames per wavefront with 16 lanes each, and the whole wavefront for what that form hands on (or, a list
// of up to retry_pack_min frames, for every frame).  The lookup follows the frame: a group's own in the first level, the wavefront's
// in the second.
constexpr int TABLE_RETRY_WAVES = 1;  // (path_kernel.h RETRY_WAVES)
__global__ void __launch_bounds__(64, TABLE_RETRY_WAVES) path_table_retry_kernel(const double* __restrict__ poses, const MatchOut* __restrict__ matched,
                                                                                 const double* __restrict__ default_path, const double* __restrict__ prev_paths,
                                                                                 GpathTable table, double* __restrict__ arena, PathOut* __restrict__ out,
                                                                                 const int* __restrict__ retry, const Params* __restrict__ prm) {
  constexpr int G1 = 16, PER = WAVE / G1;
  union Shared {
    PathShared<G1, false, NK_MAX> quad[PER];
    PathShared<WAVE, false, NK_BIG> whole;
    __device__ Shared() {}
  };
  __shared__ Shared S;
  const int n = retry[0];
  const double* gpath;
  int n_gpath;
  if (n <= prm->retry_pack_min) {
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
      const int frame = retry[1 + i];
      table_lookup(table, frame, gpath, n_gpath);
      path_frame<WAVE, false>(S.whole, frame, poses, matched, default_path, prev_paths, gpath, n_gpath, arena, out, prm);
      __syncthreads();
    }
    return;
  }
  const int g = Grp<G1>::index();
  for (int base = blockIdx.x * PER; base < n; base += gridDim.x * PER) {
    const int i = base + g;
    const int frame = i < n ? retry[1 + i] : -1;
    int st = ST_OK;
    if (frame >= 0) {
      table_lookup(table, frame, gpath, n_gpath);
      st = path_frame<G1, true>(S.quad[g], frame, poses, matched, default_path, prev_paths, gpath, n_gpath, arena, out, prm);
    }
    __syncthreads();
    for (int q = 0; q < PER; q++) {
      const int fq = __shfl(frame, q * G1), sq = __shfl(st, q * G1);
      if (fq >= 0 && (sq == ST_OVERFLOW_KNOTS || sq == ST_RETRY)) {
        table_lookup(table, fq, gpath, n_gpath);
        path_frame<WAVE, false>(S.whole, fq, poses, matched, default_path, prev_paths, gpath, n_gpath, arena, out, prm);
        __syncthreads();
      }
    }
  }
}

// A device ticket's ids, which the host cannot read: the lowest frame whose id lies outside [-1, n_paths), or -1, into one word of
// the ticket's page-locked block (the rule of device_scan_kernel for counts; such a frame is planned as -1, table_lookup).  One
// workgroup, one store at the end.
__global__ void __launch_bounds__(1024) path_ids_scan_kernel(int n_frames, int n_paths, const int32_t* __restrict__ ids, int32_t* __restrict__ bad_out) {
  __shared__ int wave_bad[16];
  const int t = (int)threadIdx.x, T = (int)blockDim.x, lane = t & 63, wave = t >> 6, n_waves = T >> 6;
  int bad = 0x7fffffff;
  for (int i = t; i < n_frames; i += T) {
    const int32_t id = ids[i];
    if ((id < -1 || id >= n_paths) && i < bad) bad = i;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const int o = __shfl_xor(bad, d);
    bad = o < bad ? o : bad;
  }
  if (lane == 0) wave_bad[wave] = bad;
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < n_waves; w++) bad = wave_bad[w] < bad ? wave_bad[w] : bad;
    __hip_atomic_store(bad_out, bad == 0x7fffffff ? -1 : bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

#endif  // FSDP_SEQ_TABLE_UNIT

}  // namespace fsdp
