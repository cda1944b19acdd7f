// Sequences with the sorting cache on (fsdp_plan_sequence_cached): frame f = step * n_planners + planner, planner i's steps
// chained through its cache entry (core_trace_sorter.py:189-195, 218-250, 293-300) exactly as n_steps lock-step calls
// (fsdp_plan_batch_sequential on a context with fsdp_sort_cache_reset) chain them.
//
// What a step reads of its predecessor: (1) cone_arrays_are_similar of ALL its cones against the entry's cones — n^2 distances,
// and the entry's cones are almost always the previous step's INPUT; (2) the same for its one or two start cones against the
// entry's start cones — and a hit stores the cached start cones again (:298-301), so these really chain: a run of hits compares
// against the start cones of the run's first miss; (3) on a hit, the side's configuration, which is the one the run's first miss
// searched.  So
//
//   sort_kernel[_128]_spec, sort_big_kernel_spec   every frame searched fresh on both sides, each side's result before
//                     combine_sides and the frame's similarity to the previous step's cones into a SeqSpecRec (sort_cache.h):
//                     all steps in parallel,
//   seq_cache_mark_kernel     one wavefront per planner walks its steps in order over those records: a few words per step — the
//                     entry's identity (whose cones, whose result per side), its start cones, the hit codes, the status with the
//                     cache on, and whether the step replaces, keeps (101 / 102) or drops (capacity refusal) the entry,
//                     sort_cache_commit's rule; at the end the planner's entry into the `next` buffers and the last step's codes,
//   seq_cache_resolve_kernel  one wavefront per frame with a hit side, in parallel: the hit side's configuration from its source,
//                     the other side's from the frame's own record, combine_sides on the frame's own cones, the SortOut rewritten
//                     with the stored diagnostics as the cached kernels report them.  Frames without a hit keep their SortOut.
//
// Irregular frames (counted): the entry's cones are NOT the previous step's — after a step the reference raised on (the entry
// was kept) or a dropped entry.  The precomputed similarity is then the wrong comparison; the walking wavefront computes the right
// one itself (lanes = the frame's cones), in order.  A hit over a side whose fresh search raised needs nothing in order here: the
// speculative pass evaluates the right side whatever the left one raised, so every side's own result and status are on record.
// A frame still waiting for sort_big_kernel_spec in a pass that was not given it carries a capacity status in its record: it
// drops the entry and is never a source; that pass is run again.
#pragma once

#include "sequence_launch.h"
#include "sort_kernel.h"

namespace fsdp {

// ---- the speculative instantiations of the three sorting kernels ----
template <class SH>
__device__ __forceinline__ void sort_spec_body(SH& S, int n_frames, const int32_t* __restrict__ cone_offsets, const double* __restrict__ cones_xyt,
                                               const double* __restrict__ poses, SortOut* __restrict__ out, int* __restrict__ big,
                                               const Params* __restrict__ prm, const SeqSpecView* spec) {
  const int frame = blockIdx.x;
  if (frame >= n_frames) return;
  sort_frame<SH, false, false, true>(S, *prm, frame, cone_offsets, cones_xyt, poses, out, StageIn(), nullptr, nullptr, spec);
  if (big != nullptr && lane_id() == 0 && (out[frame].status == ST_OVERFLOW_CONES || out[frame].status == ST_OVERFLOW_ENDS))
    big[1 + atomicAdd(&big[0], 1)] = frame;
}
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3)))
sort_kernel_spec(int n_frames, const int32_t* __restrict__ cone_offsets, const double* __restrict__ cones_xyt, const double* __restrict__ poses,
                 SortOut* __restrict__ out, int* __restrict__ big, const Params* __restrict__ prm, SeqSpecView spec) {
  __shared__ SortShared S;
  sort_spec_body(S, n_frames, cone_offsets, cones_xyt, poses, out, big, prm, &spec);
}
__global__ void __launch_bounds__(64) FSDP_WAVES_PER_EU(SORT_WAVES_128)
sort_kernel_128_spec(int n_frames, const int32_t* __restrict__ cone_offsets, const double* __restrict__ cones_xyt,
                     const double* __restrict__ poses, SortOut* __restrict__ out, int* __restrict__ big, const Params* __restrict__ prm,
                     SeqSpecView spec) {
  __shared__ SortShared128 S;
  sort_spec_body(S, n_frames, cone_offsets, cones_xyt, poses, out, big, prm, &spec);
}
__global__ void __launch_bounds__(64) sort_big_kernel_spec(const int32_t* __restrict__ cone_offsets, const double* __restrict__ cones_xyt,
                                                           const double* __restrict__ poses, SortOut* __restrict__ out,
                                                           const int* __restrict__ big, SortSharedBig* __restrict__ state,
                                                           const Params* __restrict__ prm, SeqSpecView spec) {
  const int n = big[0];
  SortSharedBig& S = state[blockIdx.x];
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    sort_frame<SortSharedBig, false, false, true>(S, *prm, big[1 + i], cone_offsets, cones_xyt, poses, out, StageIn(), nullptr, nullptr, &spec);
    __syncthreads();
  }
}

// a caller's cone row as the sorting stage sees it
__device__ __forceinline__ double seq_cone_type(const double* rows, int i) { return (double)(uint8_t)(int)rows[3 * (size_t)i + 2]; }

// grid = n_planners, one wavefront each.  Reads cache.prev*, writes cache.next* and cache.hits (the last step's codes); hits_out:
// (n_steps * n_planners, 2); resorted[planner]: the planner's irregular frames.
__global__ void __launch_bounds__(64) seq_cache_mark_kernel(int n_planners, int n_steps, const int32_t* __restrict__ cone_offsets,
                                                            const double* __restrict__ cones_xyt, SeqSpecRec* rec, SortCacheView cache,
                                                            int8_t* __restrict__ hits_out, int32_t* __restrict__ resorted) {
  const int p = blockIdx.x, lane = lane_id();
  if (p >= n_planners) return;
  const SortCacheHdr& e0 = cache.prev[p];
  const double* rows0 = cache.prev_xyt + 3 * (size_t)cache.prev_off[p];
  // the entry: whose cones (frame, -1: e0's), and per side whose result (src, -1: e0's) and which start cones
  int valid = e0.valid != 0, ent_frame = -1, ent_n = e0.n;
  int has[2], n_start[2], src[2];
  double start[2][2][3];
  for (int sd = 0; sd < 2; sd++) {
    has[sd] = valid ? e0.has[sd] : 0;
    n_start[sd] = e0.n_start[sd];
    src[sd] = -1;
    for (int k = 0; k < 6; k++) start[sd][k / 3][k % 3] = e0.start[sd][k / 3][k % 3];
  }
  int n_irregular = 0;
  int h[2] = {-1, -1};
#pragma unroll 1
  for (int s = 0; s < n_steps; s++) {
    const size_t f = (size_t)s * n_planners + p;
    SeqSpecRec& r = rec[f];
    const int n = r.n;
    const double* rows = cones_xyt + 3 * (size_t)cone_offsets[f];
    bool all_similar = valid && n >= 3 && ent_n == n;
    if (all_similar) {
      if (ent_frame == (s == 0 ? -1 : (int)(f - n_planners))) {
        all_similar = r.sim_prev != 0;
      } else {
        // the entry is older than the previous step: this frame's cones against the entry's real cones, here and now
        n_irregular++;
        const double* erows = ent_frame < 0 ? rows0 : cones_xyt + 3 * (size_t)cone_offsets[ent_frame];
        for (int i0 = 0; i0 < n && all_similar; i0 += WAVE) {
          const int i = i0 + lane;
          const bool bad = i < n && !cache_row_similar<true>(rows[3 * (size_t)i], rows[3 * (size_t)i + 1], seq_cone_type(rows, i), erows, n);
          all_similar = __ballot(bad) == 0ull;
        }
      }
    }
    int st[2], nf[2];
    for (int sd = 0; sd < 2; sd++) {
      const int fk0 = r.first_k[sd][0], fk1 = r.first_k[sd][1];
      nf[sd] = fk1 >= 0 ? 2 : 1;
      h[sd] = -1;
      st[sd] = r.status[sd];
      if (n < 3 || fk0 < 0) continue;  // returned before the check
      bool hit = all_similar && has[sd] != 0 && n_start[sd] == nf[sd];
      for (int k = 0; k < nf[sd] && hit; k++) {
        const int c = k == 0 ? fk0 : fk1;
        hit = cache_row_similar(rows[3 * (size_t)c], rows[3 * (size_t)c + 1], seq_cone_type(rows, c), &start[sd][0][0], nf[sd]);
      }
      h[sd] = hit ? 1 : 0;
      if (hit) st[sd] = ST_OK;  // a reused side is neither searched nor costed
    }
    const int status = st[0] != ST_OK ? st[0] : st[1];
    if (lane == 0) {
      r.hit[0] = h[0];
      r.hit[1] = h[1];
      r.src[0] = h[0] == 1 ? src[0] : (int)f;
      r.src[1] = h[1] == 1 ? src[1] : (int)f;
      r.resolved = status;
      hits_out[2 * f + 0] = (int8_t)h[0];
      hits_out[2 * f + 1] = (int8_t)h[1];
    }
    // sort_cache_commit's rule
    if (status == ST_REF_UNDEFINED_SET_DIFF || status == ST_REF_UNDEFINED_DFS_OOB) continue;
    if (status != ST_OK) {
      valid = 0;
      has[0] = has[1] = 0;
      continue;
    }
    valid = 1;
    ent_frame = (int)f;
    ent_n = n;
    for (int sd = 0; sd < 2; sd++) {
      if (h[sd] == 1) continue;  // the cached triple is stored again
      src[sd] = (int)f;
      has[sd] = h[sd] == 0 && r.n_configs[sd] > 0;
      n_start[sd] = nf[sd];
      for (int k = 0; k < 2; k++) {
        const int c = r.first_k[sd][k];
        const bool set = h[sd] == 0 && k < nf[sd];
        start[sd][k][0] = set ? rows[3 * (size_t)c] : 0.0;
        start[sd][k][1] = set ? rows[3 * (size_t)c + 1] : 0.0;
        start[sd][k][2] = set ? seq_cone_type(rows, c) : 0.0;
      }
    }
  }
  // the entry the planner's next call reads, and the last step's hit codes
  if (lane == 0) {
    cache.hits[2 * (size_t)p + 0] = (int8_t)h[0];
    cache.hits[2 * (size_t)p + 1] = (int8_t)h[1];
    resorted[p] = n_irregular;
  }
  SortCacheHdr& o = cache.next[p];
  double* dst = cache.next_xyt + 3 * (size_t)cache.next_off[p];
  if (!valid) {
    if (lane == 0) o.valid = 0;
    return;
  }
  if (ent_frame < 0) {  // every step kept the entry
    for (int k = lane; k < 3 * ent_n; k += WAVE) dst[k] = rows0[k];
    const int32_t* hs = reinterpret_cast<const int32_t*>(&e0);
    int32_t* hd = reinterpret_cast<int32_t*>(&o);
    for (int k = lane; k < (int)(sizeof(SortCacheHdr) / 4); k += WAVE) hd[k] = hs[k];
    return;
  }
  const double* erows = cones_xyt + 3 * (size_t)cone_offsets[ent_frame];
  for (int i = lane; i < ent_n; i += WAVE) {
    dst[3 * (size_t)i + 0] = erows[3 * (size_t)i + 0];
    dst[3 * (size_t)i + 1] = erows[3 * (size_t)i + 1];
    dst[3 * (size_t)i + 2] = seq_cone_type(erows, i);
  }
  for (int sd = 0; sd < 2; sd++) {
    const SeqSpecRec* sr = src[sd] >= 0 ? &rec[src[sd]] : nullptr;
    if (lane < MAX_LEN) o.best[sd][lane] = sr ? sr->best[sd][lane] : e0.best[sd][lane];
    if (lane < 6) o.start[sd][lane / 3][lane % 3] = start[sd][lane / 3][lane % 3];
    if (lane == 0) {
      o.has[sd] = has[sd];
      o.n_start[sd] = n_start[sd];
      o.best_len[sd] = sr ? sr->best_len[sd] : e0.best_len[sd];
      o.n_configs[sd] = sr ? sr->n_configs[sd] : e0.n_configs[sd];
      o.best_cost[sd] = sr ? sr->best_cost[sd] : e0.best_cost[sd];
    }
  }
  if (lane == 0) {
    o.n = ent_n;
    o.valid = 1;
  }
}

// What combine_sides reads of a frame state, over the frame's cone rows in global memory (a handful of cones are touched)
struct SeqConeColumn {
  const double* rows;
  __device__ __forceinline__ double operator[](int i) const { return rows[3 * (size_t)i]; }
};
struct SeqCombineState {
  SeqConeColumn x, y;
  int16_t best[2][MAX_LEN];
  int32_t best_len[2];
};

// grid = n_frames, one wavefront per frame; frames without a hit side return at once.
__global__ void __launch_bounds__(64) seq_cache_resolve_kernel(int n_frames, int n_planners, const int32_t* __restrict__ cone_offsets,
                                                                const double* __restrict__ cones_xyt, const SeqSpecRec* __restrict__ rec,
                                                                const SortCacheHdr* __restrict__ prev, SortOut* __restrict__ out) {
  __shared__ SeqCombineState S;
  const int lane = lane_id();
  const int f = blockIdx.x;
  if (f >= n_frames) return;
  const SeqSpecRec& r = rec[f];
  if (r.hit[0] != 1 && r.hit[1] != 1) return;
  const SortCacheHdr& e0 = prev[f % n_planners];
  int n_configs[2];
  double best_cost[2];
  for (int sd = 0; sd < 2; sd++) {
    const int s = r.hit[sd] == 1 ? r.src[sd] : f;
    const SeqSpecRec* sr = s >= 0 ? &rec[s] : nullptr;
    if (lane < MAX_LEN) S.best[sd][lane] = sr ? sr->best[sd][lane] : e0.best[sd][lane];
    if (lane == 0) S.best_len[sd] = sr ? sr->best_len[sd] : e0.best_len[sd];
    n_configs[sd] = sr ? sr->n_configs[sd] : e0.n_configs[sd];
    best_cost[sd] = sr ? sr->best_cost[sd] : e0.best_cost[sd];
  }
  const double* rows = cones_xyt + 3 * (size_t)cone_offsets[f];
  if (lane == 0) {
    S.x.rows = rows;
    S.y.rows = rows + 1;
  }
  __syncthreads();
  const int status = r.resolved;
  int nl = 0, nr = 0;
  if (status == ST_OK) combine_sides<SeqCombineState, true>(S, nl, nr);
  SortOut* o = &out[f];
  if (lane == 0) {
    o->status = status;
    o->n_left = nl;
    o->n_right = nr;
    o->n_configs_left = n_configs[0];
    o->n_configs_right = n_configs[1];
    o->first_k_left[0] = r.first_k[0][0];
    o->first_k_left[1] = r.first_k[0][1];
    o->first_k_right[0] = r.first_k[1][0];
    o->first_k_right[1] = r.first_k[1][1];
    o->best_cost_left = best_cost[0];
    o->best_cost_right = best_cost[1];
  }
  if (lane < MAX_LEN) {
    o->left_idx[lane] = (status == ST_OK && lane < nl) ? (int32_t)S.best[0][lane] : -1;
    o->right_idx[lane] = (status == ST_OK && lane < nr) ? (int32_t)S.best[1][lane] : -1;
  }
}

}  // namespace fsdp
