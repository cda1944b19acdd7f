// Sequences with per-frame global paths (fsdp_plan_sequence_paths, fsdp_submit_sequence_paths; include/fsdp.h): the TABLE twin of
// seq_chain_kernel (sequence_kernel.h), by the rule gpath_table_kernel.h states for its twins.  seq_chain_kernel takes one pair
// (gpath, n_gpath) for the whole launch; the twin resolves the pair of each frame it plans again from the context's path table and
// the pass's ids, in front of that frame's path_frame<WAVE, false>.  Everything else of a sequence pass with ids is what exists:
// the speculative pass through the path table wrappers (prev_paths == nullptr), seq_mark_kernel and seq_final_kernel, none of
// which reads a global path here.
//
// KEEP THE BODY THE SAME AS seq_chain_kernel's, statement for statement, but for the lookup.  It is a body of its own, in a
// translation unit and code object of its own (sequence_table_lib.hip, launched through sequence_table_launch.h): a flag on
// seq_chain_kernel, or a second kernel in its module, would change what the earlier kernels compile to (tools/kernel_code_diff.py).
// A unit that wants this kernel alone defines FSDP_SEQ_TABLE_UNIT: sequence_kernel.h and gpath_table_kernel.h then leave out their
// kernels that are no templates, which belong to sequence_lib.hip and gpath_table_lib.hip.
//
// The id is wave-uniform: a run has its wavefront to itself, and `frame` is a function of the run's head.  It is loaded the way
// seq_load loads the status words — a vector load whatever the compiler knows about the address — and made uniform again, so that
// the pair stays in scalar registers like seq_chain_kernel's launch arguments and path_front's window loops keep uniform bounds.
//
// Why the speculative results are still final where no FB_READ_PREVIOUS bit is set: DESIGN.md §8, "Finality with a global path".
#pragma once

#include "gpath_table_kernel.h"
#include "sequence_kernel.h"

namespace fsdp {

// table_lookup for one frame of a run (whole wavefront)
__device__ __forceinline__ void seq_table_lookup(const GpathTable& t, size_t frame, const double*& gpath, int& n_gpath) {
  const int32_t id = wave_uniform(seq_load(&t.ids[frame]));
  const GpathTable one{t.xy, t.off, &id, t.n_paths};
  table_lookup(one, 0, gpath, n_gpath);
}

// seq_chain_kernel
__global__ void __launch_bounds__(64, 1) seq_chain_table_kernel(int n_planners, int n_steps, const double* __restrict__ poses,
                                                                const MatchOut* __restrict__ matched, const double* __restrict__ initial_prev,
                                                                GpathTable table, double* arena, PathOut* out, int* seq,
                                                                const Params* __restrict__ prm) {
  __shared__ PathShared<WAVE, false, NK_BIG> S;
  const int n_heads = wave_uniform(seq_load(&seq[SEQ_HEADS]));
  int replanned = 0;
#pragma unroll 1
  for (int k = blockIdx.x; k < n_heads; k += gridDim.x) {
    const int head = wave_uniform(seq_load(&seq[SEQ_LIST + 2 * (size_t)k])), pred = wave_uniform(seq_load(&seq[SEQ_LIST + 2 * (size_t)k + 1]));
    const int planner = head % n_planners;
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
        const double* gpath;
        int n_gpath;
        seq_table_lookup(table, frame, gpath, n_gpath);
        status = wave_uniform(path_frame<WAVE, false>(S, (int)frame, poses, matched, prev, gpath, n_gpath, arena, out, prm));
        replanned++;
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

}  // namespace fsdp
