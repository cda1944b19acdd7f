// TEST INFRASTRUCTURE — the ranked instantiations of the sorting kernels (csrc/sort_rank_kernels.h sort_kernel_128_ranked /
// sort_kernel_ranked / sort_big_kernel_ranked) under the host SIMT emulator, launched the way emu_kernels.cpp emu_sort_plain
// launches the plain ones and wrapped like the library's fsdp_sort_batch_ranked (csrc/fsdp_lib.hip: fill, filter, kernels,
// indices back to the caller's array).  A translation unit of its own so that the two compile side by side; parameters,
// switches and filter come from emu_kernels.cpp (emu_shared.h).  Never loaded by the package.
#include "emu_shared.h"

#include "../../ft-fsd-path-planning_amd/csrc/sort_rank_kernels.h"

static int g_last_kernels = 0;  // bit 0: sort_kernel_128_ranked, bit 1: sort_kernel_ranked, bit 2: sort_big_kernel_ranked planned a frame

extern "C" {
int emu_ranked_last_kernels() { return g_last_kernels; }

// returns 0, or 1 for a top_k outside 1..RANK_MAX; terms may be NULL
int emu_sort_ranked(int n_frames, const int32_t* offsets, const double* cones, const double* poses, fsdp::SortOut* out, int top_k,
                    int32_t* counts, int32_t* configs, double* costs, double* terms) {
  if (top_k < 1 || top_k > fsdp::RANK_MAX) return 1;
  const size_t per_frame = 2 * (size_t)top_k * fsdp::MAX_LEN, rows = (size_t)n_frames * 2 * (size_t)top_k;
  memset(counts, 0, sizeof(int32_t) * 2 * (size_t)n_frames);
  memset(configs, 0xff, sizeof(int32_t) * rows * fsdp::MAX_LEN);
  memset(costs, 0xff, sizeof(double) * rows);
  if (terms) memset(terms, 0xff, sizeof(double) * rows * fsdp::COST_TERMS);
  const bool filtered = !g_prm.use_unknown_cones;
  if (filtered) {
    emu_filter(n_frames, offsets, cones);
    offsets = g_f_off.data();
    cones = g_f_cones.data();
  }
  fsdp::SortRankView v;
  v.top_k = top_k;
  v.counts = counts;
  v.configs = configs;
  v.costs = costs;
  v.terms = terms;
  std::vector<int> big((size_t)n_frames + 1, 0);
  if (emu_sort128(n_frames, offsets)) {
    emu::launch((unsigned)n_frames, 64, [&]() { fsdp::sort_kernel_128_ranked(n_frames, offsets, cones, poses, out, big.data(), &g_prm, v); });
    g_last_kernels = 1;
  } else {
    emu::launch((unsigned)n_frames, 64, [&]() { fsdp::sort_kernel_ranked(n_frames, offsets, cones, poses, out, big.data(), &g_prm, v); });
    g_last_kernels = 2;
  }
  g_last_big = big[0];
  if (big[0] > 0) {
    std::vector<fsdp::SortSharedBig> state(2);
    std::vector<fsdp::SortRankScratchBig> scratch(2);
    memset((void*)scratch.data(), 0xff, sizeof(fsdp::SortRankScratchBig) * 2);  // (whatever the allocator left)
    emu::launch(2, 64, [&]() { fsdp::sort_big_kernel_ranked(offsets, cones, poses, out, big.data(), state.data(), &g_prm, v, scratch.data()); });
    g_last_kernels |= 4;
  }
  if (filtered) {
    emu_sort_remap(n_frames, out);
    for (int f = 0; f < n_frames; f++) emu_map_back(f, configs + (size_t)f * per_frame, per_frame);
  }
  return 0;
}
}
