// TEST INFRASTRUCTURE — the ranked instantiations of the sorting kernels (csrc/sort_rank_kernels.h sort_kernel_128_ranked /
// sort_kernel_ranked / sort_big_kernel_ranked) under the host SIMT emulator (tests/emu/hip_emu.h), launched the way
// tests/emu/emu_kernels.cpp emu_sort_plain launches the plain ones and wrapped like the library's fsdp_sort_batch_ranked
// (csrc/fsdp_lib.hip: fill, filter, kernels, indices back to the caller's array).  A translation unit of its own so that the
// existing emulator library stays as it is.  Never loaded by the package.
#include "../emu/hip_emu.h"

#include "../../ft-fsd-path-planning_amd/csrc/sort_kernel.h"
#include "../../ft-fsd-path-planning_amd/csrc/sort_rank_kernels.h"
#include "../../ft-fsd-path-planning_amd/csrc/filter_kernel.h"

#include <algorithm>
#include <vector>

static fsdp::Params g_prm = {5, 12, 6.5, 6.0, 40 * FSDP_DEG, 65 * FSDP_DEG, 3.0, 5.0, 50 * FSDP_DEG, 0.2, 0.1, 5.0, 20.0, 3, 40, 0, 1};
static bool g_no_sort128 = false;
static int g_last_big = 0;
static int g_last_kernels = 0;  // bit 0: sort_kernel_128_ranked, bit 1: sort_kernel_ranked, bit 2: sort_big_kernel_ranked planned a frame

extern "C" {
int emu_ranked_sizeof_sort_out() { return (int)sizeof(fsdp::SortOut); }
int emu_ranked_max_len() { return fsdp::MAX_LEN; }
int emu_ranked_last_big() { return g_last_big; }
int emu_ranked_last_kernels() { return g_last_kernels; }
void emu_ranked_set_no_sort128(int on) { g_no_sort128 = on != 0; }
// the 17 configuration constants in oracle_lib.PARAM_ORDER (like emu_set_params of the existing library)
void emu_ranked_set_params(const double* v) {
  g_prm = fsdp::Params{(int32_t)v[0], (int32_t)v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12],
                       (int32_t)v[13], (int32_t)v[14], (int32_t)v[15], (int32_t)v[16]};
}

// returns 0, or 1 for a top_k outside 1..RANK_MAX; terms may be NULL
int emu_sort_ranked(int n_frames, const int32_t* offsets, const double* cones, const double* poses, fsdp::SortOut* out, int top_k,
                    int32_t* counts, int32_t* configs, double* costs, double* terms) {
  if (top_k < 1 || top_k > fsdp::RANK_MAX) return 1;
  const size_t rows = (size_t)n_frames * 2 * (size_t)top_k;
  memset(counts, 0, sizeof(int32_t) * 2 * (size_t)n_frames);
  memset(configs, 0xff, sizeof(int32_t) * rows * fsdp::MAX_LEN);
  memset(costs, 0xff, sizeof(double) * rows);
  if (terms) memset(terms, 0xff, sizeof(double) * rows * fsdp::COST_TERMS);
  std::vector<int32_t> f_off, f_map;
  std::vector<double> f_cones;
  const bool filtered = !g_prm.use_unknown_cones;
  if (filtered) {
    std::vector<int32_t> cnt((size_t)n_frames + 1, 0);
    f_off.assign((size_t)n_frames + 1, 0);
    const size_t total = (size_t)offsets[n_frames];
    f_cones.assign(3 * total + 3, 0.0);
    f_map.assign(total + 1, 0);
    emu::launch((unsigned)n_frames, 64, [&]() { fsdp::filter_count_kernel(n_frames, offsets, cones, cnt.data()); });
    emu::launch(1, 64, [&]() { fsdp::filter_scan_kernel(n_frames, cnt.data(), f_off.data()); });
    emu::launch((unsigned)n_frames, 64, [&]() { fsdp::filter_scatter_kernel(n_frames, offsets, cones, f_off.data(), f_cones.data(), f_map.data()); });
    offsets = f_off.data();
    cones = f_cones.data();
  }
  fsdp::SortRankView v;
  v.top_k = top_k;
  v.counts = counts;
  v.configs = configs;
  v.costs = costs;
  v.terms = terms;
  std::vector<int> big((size_t)n_frames + 1, 0);
  int max_cones = 0;
  for (int f = 0; f < n_frames; f++) max_cones = std::max(max_cones, (int)(offsets[f + 1] - offsets[f]));
  g_last_kernels = 0;
  if (max_cones <= fsdp::SortShared128::MAX_N && !g_no_sort128) {
    emu::launch((unsigned)n_frames, 64, [&]() { fsdp::sort_kernel_128_ranked(n_frames, offsets, cones, poses, out, big.data(), &g_prm, v); });
    g_last_kernels |= 1;
  } else {
    emu::launch((unsigned)n_frames, 64, [&]() { fsdp::sort_kernel_ranked(n_frames, offsets, cones, poses, out, big.data(), &g_prm, v); });
    g_last_kernels |= 2;
  }
  g_last_big = big[0];
  if (big[0] > 0) {
    std::vector<fsdp::SortSharedBig> state(2);
    std::vector<fsdp::SortRankScratchBig> scratch(2);
    memset((void*)scratch.data(), 0xff, sizeof(fsdp::SortRankScratchBig) * 2);  // (whatever the allocator left)
    emu::launch(2, 64, [&]() { fsdp::sort_big_kernel_ranked(offsets, cones, poses, out, big.data(), state.data(), &g_prm, v, scratch.data()); });
    g_last_kernels |= 4;
  }
  if (filtered)
    for (int f = 0; f < n_frames; f++) {
      auto back = [&](int32_t& x) {
        if (x >= 0) x = f_map[(size_t)f_off[f] + x];
      };
      for (int k = 0; k < fsdp::MAX_LEN; k++) {
        back(out[f].left_idx[k]);
        back(out[f].right_idx[k]);
      }
      for (int k = 0; k < 2; k++) {
        back(out[f].first_k_left[k]);
        back(out[f].first_k_right[k]);
      }
      int32_t* r = configs + (size_t)f * 2 * (size_t)top_k * fsdp::MAX_LEN;
      for (size_t k = 0; k < 2 * (size_t)top_k * fsdp::MAX_LEN; k++) back(r[k]);
    }
  return 0;
}
}
