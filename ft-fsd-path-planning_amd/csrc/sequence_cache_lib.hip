// The kernels of fsdp_plan_sequence_cached (sequence_cache_kernel.h) and their launches: a translation unit, and so a code
// object, of their own next to fsdp_lib.hip and sequence_lib.hip, built into the same shared library.  It holds the speculative
// instantiations of the three sorting kernels and the two chain kernels of the sorting cache, and nothing else: sort_kernel.h
// leaves out its own kernels (FSDP_SEQUENCE_CACHE_UNIT), which belong to fsdp_lib.hip — nothing the earlier kernels are compiled
// from changes.
#include <hip/hip_runtime.h>

#define FSDP_SEQUENCE_CACHE_UNIT 1
#include "sequence_cache_kernel.h"

static fsdp::SeqSpecView spec_view(const fsdp_seqc_launch_args* a) {
  fsdp::SeqSpecView v;
  v.rec = a->rec;
  v.n_planners = a->n_planners;
  v.prev = a->cache.prev;
  v.prev_xyt = a->cache.prev_xyt;
  v.prev_off = a->cache.prev_off;
  return v;
}

extern "C" void fsdp_seqc_launch_sort(hipStream_t stream, const fsdp_seqc_launch_args* a) {
  using namespace fsdp;
  const int n = a->n_planners * a->n_steps;
  hipLaunchKernelGGL((a->small ? sort_kernel_128_spec : sort_kernel_spec), dim3((unsigned)n), dim3(WAVE), 0, stream, n, a->off, a->cones, a->poses,
                     a->sorted, a->big, a->prm, spec_view(a));
}

extern "C" void fsdp_seqc_launch_sort_big(hipStream_t stream, const fsdp_seqc_launch_args* a) {
  using namespace fsdp;
  hipLaunchKernelGGL(sort_big_kernel_spec, dim3((unsigned)a->big_blocks), dim3(WAVE), 0, stream, a->off, a->cones, a->poses, a->sorted,
                     (const int*)a->big, (SortSharedBig*)a->big_state, a->prm, spec_view(a));
}

extern "C" void fsdp_seqc_launch_chain(hipStream_t stream, const fsdp_seqc_launch_args* a) {
  using namespace fsdp;
  const int n = a->n_planners * a->n_steps;
  hipLaunchKernelGGL(seq_cache_mark_kernel, dim3((unsigned)a->n_planners), dim3(WAVE), 0, stream, a->n_planners, a->n_steps, a->off, a->cones,
                     a->rec, a->cache, a->hits, a->resorted);
  hipLaunchKernelGGL(seq_cache_resolve_kernel, dim3((unsigned)n), dim3(WAVE), 0, stream, n, a->n_planners, a->off, a->cones,
                     (const SeqSpecRec*)a->rec, a->cache.prev, a->sorted);
}
