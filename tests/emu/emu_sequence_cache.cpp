// TEST INFRASTRUCTURE — the sorting side of a fsdp_plan_sequence_cached pass (csrc/sequence_cache_kernel.h: the speculative
// instantiations of the three sorting kernels, seq_cache_mark_kernel, seq_cache_resolve_kernel) under the host SIMT emulator,
// launched the way the library launches them (csrc/sequence_cache_lib.hip), planners starting from empty cache entries.  A
// translation unit of libfsdp_emu[_wide].so like emu_ranked.cpp; parameters, sort128 switch and filter come from emu_kernels.cpp
// (emu_shared.h).  Never loaded by the package.
#include "emu_shared.h"

#include "../../ft-fsd-path-planning_amd/csrc/sequence_cache_kernel.h"

#include <algorithm>

extern "C" {
int emu_sizeof_seq_spec_rec() { return (int)sizeof(fsdp::SeqSpecRec); }

// out: (frames) SortOut with indices of the caller's cone arrays; hits: (frames, 2); resorted: the irregular frames.
// kernels (optional): bit 0 / 1 / 2 = sort_kernel_128_spec / sort_kernel_spec / sort_big_kernel_spec ran.
// Returns the frames the big route planned.
int emu_sequence_cache(int n_planners, int n_steps, const int32_t* offsets, const double* cones, const double* poses, fsdp::SortOut* out,
                       int8_t* hits, long long* resorted, int* kernels) {
  using namespace fsdp;
  const int n = n_planners * n_steps;
  const int32_t* off = offsets;
  const double* xyt = cones;
  if (!g_prm.use_unknown_cones) {
    emu_filter(n, offsets, cones);
    off = g_f_off.data();
    xyt = g_f_cones.data();
  }
  // the two cache buffers: empty entries in front of the call, regions for every planner's largest frame behind it
  std::vector<SortCacheHdr> prev((size_t)n_planners), next((size_t)n_planners);
  memset((void*)prev.data(), 0, sizeof(SortCacheHdr) * prev.size());
  memset((void*)next.data(), 0xff, sizeof(SortCacheHdr) * next.size());
  std::vector<int32_t> prev_off((size_t)n_planners + 1, 0), next_off((size_t)n_planners + 1, 0);
  for (int p = 0; p < n_planners; p++) {
    int m = 0;
    for (int s = 0; s < n_steps; s++) m = std::max(m, (int)(off[s * n_planners + p + 1] - off[s * n_planners + p]));
    next_off[(size_t)p + 1] = next_off[(size_t)p] + m;
  }
  std::vector<double> prev_xyt(3, 0.0), next_xyt(3 * (size_t)next_off[(size_t)n_planners] + 3, 0.0);
  std::vector<SeqSpecRec> rec((size_t)n);
  memset((void*)rec.data(), 0xff, sizeof(SeqSpecRec) * rec.size());
  SeqSpecView spec;
  spec.rec = rec.data();
  spec.n_planners = n_planners;
  spec.prev = prev.data();
  spec.prev_xyt = prev_xyt.data();
  spec.prev_off = prev_off.data();
  std::vector<int> big((size_t)n + 1, 0);
  const bool small = emu_sort128(n, off);
  if (small)
    emu::launch((unsigned)n, 64, [&]() { sort_kernel_128_spec(n, off, xyt, poses, out, big.data(), &g_prm, spec); });
  else
    emu::launch((unsigned)n, 64, [&]() { sort_kernel_spec(n, off, xyt, poses, out, big.data(), &g_prm, spec); });
  g_last_big = big[0];
  if (kernels) *kernels = (small ? 1 : 2) | (big[0] > 0 ? 4 : 0);
  if (big[0] > 0) {
    std::vector<SortSharedBig> state(2);
    emu::launch(2, 64, [&]() { sort_big_kernel_spec(off, xyt, poses, out, big.data(), state.data(), &g_prm, spec); });
  }
  SortCacheView v;
  v.prev = prev.data();
  v.next = next.data();
  v.prev_xyt = prev_xyt.data();
  v.prev_off = prev_off.data();
  v.next_xyt = next_xyt.data();
  v.next_off = next_off.data();
  std::vector<int8_t> last((size_t)2 * n_planners, 0);
  v.hits = last.data();
  std::vector<int32_t> res((size_t)n_planners, 0);
  emu::launch((unsigned)n_planners, 64, [&]() { seq_cache_mark_kernel(n_planners, n_steps, off, xyt, rec.data(), v, hits, res.data()); });
  emu::launch((unsigned)n, 64, [&]() { seq_cache_resolve_kernel(n, n_planners, off, xyt, rec.data(), prev.data(), out); });
  long long sum = 0;
  for (int32_t r : res) sum += r;
  if (resorted) *resorted = sum;
  emu_sort_remap(n, out);
  return big[0];
}
}
