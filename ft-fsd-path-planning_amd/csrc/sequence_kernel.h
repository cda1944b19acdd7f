// Sequences of consecutive steps in one pass (fsdp_plan_sequence): frame f = step * n_planners + planner, planner i's
// steps chained through previous_paths[-1] (core_calculate_path.py:572-573) exactly as n_steps calls of
// fsdp_plan_batch_sequential chain them.
//
// The reference reads the previous path in its fallbacks only (:203, 218-221, 235-236, 531-536, 564-570), and each of those
// reads sets one of the four FB_READ_PREVIOUS bits of PathOut.fallback (path_kernel.h: path_front bits 1 and 2,
// overwrite_if_too_far bit 4, finish_path bit 8 — mpc_finish's "previous array handed on" return is that retry, bit 8).
// So the pass first plans every frame with the constant initial path (prev_paths == nullptr, like fsdp_plan_batch); a frame
// without such a bit never looked at its previous path and its result is final.  Then
//
//   seq_mark_kernel   lanes = frames: the heads of the runs of flagged frames, appended to a device list,
//   seq_chain_kernel  one wavefront per run: the path stage of the run's flagged frames once more, in order, each with the
//                     path its planner's most recent successful step really left,
//   seq_final_kernel  one wavefront per planner: the path the planner hands to the step after the sequence; the re-plan
//                     count into the pass trailer.
//
// A frame is one of three things to its planner's chain (seq_class):
//   SETTLED      not flagged, status 0: final, and the previous path of what follows,
//   TRANSPARENT  not flagged, status != 0: the reference raised, the chain is left untouched (planner.py:271-274) — and a frame
//                still carrying ST_RETRY: the pass lacked its retry route and is about to run again,
//   FLAGGED      read the previous path, whatever its status (a frame that failed on the constant path may succeed on the true
//                one): final only once everything flagged directly before it is.
// These kernels are a translation unit of their own (sequence_lib.hip), i.e. a code object of their own inside the library: the
// kernels of fsdp_lib.hip compile to exactly what they were (a second user of the whole-wavefront path stage in their module
// moved path_retry_kernel's register allocation).
// A run is a maximal sequence of one planner's flagged frames with nothing but transparent frames between them; only runs
// serialize, and every run has a wavefront of its own.
#pragma once

#include "path_kernel.h"
#include "sequence_launch.h"

namespace fsdp {

enum { SEQ_SETTLED = 0, SEQ_TRANSPARENT = 1, SEQ_FLAGGED = 2 };


__device__ __forceinline__ int seq_class(int status, int fallback) {
  if (status == ST_RETRY) return SEQ_TRANSPARENT;
  if (fallback & FB_READ_PREVIOUS) return SEQ_FLAGGED;
  return status == ST_OK ? SEQ_SETTLED : SEQ_TRANSPARENT;
}

// Status and flags of a frame another kernel — or this wavefront, a moment ago — wrote: loads that stay vector loads whatever
// the compiler knows about the address (the scalar cache is not coherent with vector stores)
__device__ __forceinline__ int seq_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int seq_class_of(const PathOut* out, size_t frame) {
  return seq_class(seq_load(&out[frame].status), seq_load(&out[frame].fallback));
}

// Where the chain of `planner` stands in front of step `step`: walks back over the transparent frames.  Returns the class of
// the frame the walk stops at (SEQ_TRANSPARENT: it ran off the start) and that frame in *at (-1: none).
__device__ __forceinline__ int seq_walk_back(const PathOut* out, int n_planners, int planner, int step, int* at) {
  for (int s = step - 1; s >= 0; s--) {
    const size_t f = (size_t)s * n_planners + planner;
    const int c = seq_class_of(out, f);
    if (c != SEQ_TRANSPARENT) {
      *at = (int)f;
      return c;
    }
  }
  *at = -1;
  return SEQ_TRANSPARENT;
}

// (FSDP_SEQ_TABLE_UNIT: csrc/sequence_table_lib.hip compiles this header for the chain rule's helpers above alone — the kernels
// below belong to sequence_lib.hip)
#ifndef FSDP_SEQ_TABLE_UNIT
// grid = ceil(n_frames / 64).  A flagged frame is a run head when the walk back from it stops at a settled frame or runs off
// the start; not when it stops at a flagged frame, whose result is not final yet.
__global__ void __launch_bounds__(64) seq_mark_kernel(int n_planners, int n_steps, const PathOut* __restrict__ out, int* __restrict__ seq) {
  const long long n_frames = (long long)n_planners * n_steps;
  const long long frame = (long long)blockIdx.x * WAVE + lane_id();
  bool head = false;
  int pred = -1;
  if (frame < n_frames && seq_class_of(out, (size_t)frame) == SEQ_FLAGGED) {
    const int step = (int)(frame / n_planners), planner = (int)(frame % n_planners);
    head = seq_walk_back(out, n_planners, planner, step, &pred) != SEQ_FLAGGED;
  }
  // one atomic per wavefront (ballot + prefix count), like the retry list's push
  const unsigned long long m = __ballot(head);
  if (m == 0) return;
  const int lane = lane_id();
  int base = 0;
  if (lane == __ffsll((long long)m) - 1) base = atomicAdd(&seq[SEQ_HEADS], __popcll(m));
  base = __shfl(base, __ffsll((long long)m) - 1, WAVE);
  if (head) {
    const int k = base + __popcll(m & ((1ull << lane) - 1ull));
    seq[SEQ_LIST + 2 * (size_t)k] = (int)frame;
    seq[SEQ_LIST + 2 * (size_t)k + 1] = pred;
  }
}

// One wavefront per run (grid-stride over the head list, one wavefront per SIMD like path_retry_kernel's whole-wavefront form):
// the path stage of the run's flagged frames from their MatchOut, in their own arenas, by the exact form path_frame<WAVE, false>
// (256 knots, all degrees, plain divisions: results do not depend on the route a frame took).
// initial_prev (optional): (n_planners, PATH_POINTS, 4), a row whose [0][0] is NaN = none.
__global__ void __launch_bounds__(64, 1) seq_chain_kernel(int n_planners, int n_steps, const double* __restrict__ poses,
                                                          const MatchOut* __restrict__ matched, const double* __restrict__ initial_prev,
                                                          const double* __restrict__ gpath, int n_gpath, double* arena, PathOut* out,
                                                          int* seq, const Params* __restrict__ prm) {
  __shared__ PathShared<WAVE, false, NK_BIG> S;
  const int n_heads = wave_uniform(seq_load(&seq[SEQ_HEADS]));
  int replanned = 0;
#pragma unroll 1
  for (int k = blockIdx.x; k < n_heads; k += gridDim.x) {
    const int head = wave_uniform(seq_load(&seq[SEQ_LIST + 2 * (size_t)k])), pred = wave_uniform(seq_load(&seq[SEQ_LIST + 2 * (size_t)k + 1]));
    const int planner = head % n_planners;
    // the path in front of the run: the settled frame's, the caller's row, or none (the run's frames then stand as they are
    // until one of them succeeds: the constant initial path they were planned with is what a fresh planner reads)
    const double* prev = nullptr;
    if (pred >= 0) {
      prev = &out[pred].path[0][0];
    } else if (initial_prev != nullptr) {
      const double* row = initial_prev + (size_t)planner * (PATH_POINTS * 4);
      if (!isnan(row[0])) prev = row;
    }
#pragma unroll 1
    for (int s = head / n_planners; s < n_steps; s++) {
      const size_t frame = (size_t)s * n_planners + planner;
      const int c = wave_uniform(seq_class_of(out, frame));
      if (c == SEQ_TRANSPARENT) continue;
      if (c == SEQ_SETTLED) break;
      int status;
      if (prev != nullptr) {
        status = wave_uniform(path_frame<WAVE, false>(S, (int)frame, poses, matched, prev, gpath, n_gpath, arena, out, prm));
        replanned++;
        // the frame's path has left the wavefront before the next frame of the run loads it as its previous path
        __syncthreads();
        stores_acknowledged();
      } else {
        status = wave_uniform(seq_load(&out[frame].status));
      }
      if (status == ST_OK) prev = &out[frame].path[0][0];
    }
  }
  if (replanned > 0 && lane_id() == 0) atomicAdd(&seq[SEQ_REPLANNED], replanned);
}

// grid = n_planners.  final_prev[planner] = the path of the planner's last successful step, else its initial_prev row, else NaN
// (none yet: the next call starts it as a fresh planner).  Block 0 hands the re-plan count to the host: replanned_out is the
// spare word of the pass trailer (assemble_kernel.h PassTrailer::pad, which assemble_kernel leaves alone; the trailer's seq,
// written last and in stream order behind this kernel, publishes it).
__global__ void __launch_bounds__(64) seq_final_kernel(int n_planners, int n_steps, const PathOut* __restrict__ out,
                                                       const double* __restrict__ initial_prev, double* __restrict__ final_prev,
                                                       const int* __restrict__ seq, int32_t* __restrict__ replanned_out) {
  const int planner = blockIdx.x, lane = lane_id();
  if (planner == 0 && lane == 0 && replanned_out != nullptr)
    __hip_atomic_store(replanned_out, seq[SEQ_REPLANNED], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (planner >= n_planners || final_prev == nullptr) return;
  const double* src = nullptr;
  for (int s = n_steps - 1; s >= 0 && src == nullptr; s--) {
    const PathOut* o = &out[(size_t)s * n_planners + planner];
    if (o->status == ST_OK) src = &o->path[0][0];
  }
  if (src == nullptr && initial_prev != nullptr && !isnan(initial_prev[(size_t)planner * (PATH_POINTS * 4)]))
    src = initial_prev + (size_t)planner * (PATH_POINTS * 4);
  double* dst = final_prev + (size_t)planner * (PATH_POINTS * 4);
  for (int i = lane; i < PATH_POINTS * 4; i += WAVE) dst[i] = src ? src[i] : NAN;
}

#ifndef FSDP_EMU
// ---- planner slices of a recording (fsdp_submit_sequence, sequence_slice.h) -----------------------------------------------------
// A slice is n_steps segments `total` frames apart; the direct routes of a pass (sort_kernel's StageIn, assemble_kernel writing
// into the caller's buffer) move one contiguous segment only.  These two kernels move a slice between the caller's page-locked
// arrays and the slot's dense device copies, in front of the pass and behind its assembly: pure data movement over PCIe, no
// LDS, any grid walks any slice.

// grid = 256 x 256 like stage_in_kernel (~1 MB of loads on the wire).  One wavefront per frame and trip: its offset (rebased into
// the gap-free device CSR), its pose and its cone rows — 24 bytes each, so whether the source and the destination of a frame
// are 16-byte aligned depends on the parity of the two row indices: 16 bytes per lane where both are, 8 where not.  What the
// host checked at submit (sequence_slice.h seq_slice_segments) is clamped again: the caller's arrays are his not to touch, but a
// touched offset must not send a store beyond the device copies.
__global__ void __launch_bounds__(256) seq_slice_in_kernel(fsdp_seq_slice_in_args a) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  const int lane = (int)(threadIdx.x & 63), waves_per_block = (int)(blockDim.x >> 6);
  const long long wave0 = (long long)blockIdx.x * waves_per_block + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * waves_per_block;
  const long long nf = a.s.frames(), rows = a.rows;
  for (long long f = wave0; f < nf; f += n_waves) {
    const long long step = f / a.s.n;
    const long long r = step * a.s.total + (f - step * a.s.n);  // (relative to the slice's first frame: the sources start there)
    const SeqSeg g = a.seg[step];
    const int32_t o0 = a.src_off[r], o1 = a.src_off[r + 1];
    long long d0 = seq_dense_offset(g, o0), cnt = (long long)o1 - o0, s0 = (long long)o0 - a.cone_base;
    d0 = d0 < 0 ? 0 : (d0 > rows ? rows : d0);
    cnt = cnt < 0 ? 0 : (cnt > rows - d0 ? rows - d0 : cnt);
    if (s0 < 0 || s0 + cnt > a.src_rows) cnt = 0;
    if (lane == 0) {
      a.dst_off[f] = (int32_t)d0;
      if (f == nf - 1) a.dst_off[nf] = (int32_t)rows;
    }
    if (lane < 4) a.dst_poses[4 * f + lane] = __builtin_nontemporal_load(a.src_poses + 4 * r + lane);
    const double* src = a.src_cones + 3 * s0;
    double* dst = a.dst_cones + 3 * d0;
    const long long nd = 3 * cnt;
    if ((((unsigned long long)src | (unsigned long long)dst) & 15ull) == 0) {
      const long long n2 = nd >> 1;
      for (long long k = lane; k < n2; k += WAVE) ((d2*)dst)[k] = __builtin_nontemporal_load((const d2*)src + k);
      if ((nd & 1) && lane == 0) dst[nd - 1] = __builtin_nontemporal_load(src + nd - 1);
    } else {
      for (long long k = lane; k < nd; k += WAVE) dst[k] = __builtin_nontemporal_load(src + k);
    }
  }
  // the slice's initial_prev rows: adjacent in the recording's block (planners lo .. lo + n)
  if (a.src_init != nullptr) {
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
    const long long nd = (long long)a.s.n * (PATH_POINTS * 4);
    if ((((unsigned long long)a.src_init | (unsigned long long)a.dst_init) & 15ull) == 0) {
      for (long long k = tid; k < (nd >> 1); k += nth) ((d2*)a.dst_init)[k] = __builtin_nontemporal_load((const d2*)a.src_init + k);
    } else {
      for (long long k = tid; k < nd; k += nth) a.dst_init[k] = __builtin_nontemporal_load(a.src_init + k);
    }
  }
}

// Behind the pass's assembly, which left the records (full or compact, rec_bytes each) dense in the slot's result block: the
// records of step t to results[t * total + lo ...] and the slice's final_prev rows to theirs, in the caller's page-locked arrays.
// One wavefront per record and trip, like assemble_kernel: consecutive lanes on consecutive 8-byte words of the destination (a
// record is a multiple of 8 bytes, not of 16), one division per record; the grid is capped like launch_assemble's for stores
// towards host memory.
__global__ void __launch_bounds__(256) seq_slice_out_kernel(fsdp_seq_slice_out_args a) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
  const int lane = (int)(threadIdx.x & 63), waves_per_block = (int)(blockDim.x >> 6), rec = a.rec_bytes / 8;
  const long long wave0 = (long long)blockIdx.x * waves_per_block + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * waves_per_block;
  const long long nf = a.s.frames();
  const unsigned long long* src = (const unsigned long long*)a.src_records;
  unsigned long long* dst = (unsigned long long*)a.dst_records;  // (the slice's first record: planner lo of step 0)
  for (long long f = wave0; f < nf; f += n_waves) {
    const long long step = f / a.s.n;
    const unsigned long long* s = src + f * rec;
    unsigned long long* d = dst + (step * a.s.total + (f - step * a.s.n)) * rec;
    for (int w = lane; w < rec; w += WAVE) d[w] = s[w];
  }
  if (a.dst_final != nullptr) {
    const long long nd = (long long)a.s.n * (PATH_POINTS * 4);
    for (long long k = tid; k < nd; k += nth) a.dst_final[k] = a.src_final[k];
  }
}
#endif  // FSDP_EMU
#endif  // FSDP_SEQ_TABLE_UNIT

}  // namespace fsdp
