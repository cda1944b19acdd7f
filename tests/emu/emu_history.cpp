// TEST INFRASTRUCTURE — the history instantiations of the sorting kernels (csrc/sort_history_kernels.h sort_kernel_128_history /
// sort_kernel_history / sort_big_kernel_history) under the host SIMT emulator, launched the way emu_kernels.cpp emu_sort_plain
// launches the plain ones and wrapped like the library's fsdp_sort_batch_history (csrc/fsdp_lib.hip: fill, filter, kernels,
// indices back to the caller's array).  Built by history.mk into a library of its own together with emu_kernels.cpp, where the
// parameters, the no_sort128 switch and the filter live (emu_shared.h).  Never loaded by the package.
#include "emu_shared.h"

#include "../../ft-fsd-path-planning_amd/csrc/sort_history_kernels.h"

static int g_last_kernels = 0;  // bit 0: sort_kernel_128_history, bit 1: sort_kernel_history, bit 2: sort_big_kernel_history planned a frame

extern "C" {
int emu_history_last_kernels() { return g_last_kernels; }
int emu_history_max_neighbors() { return fsdp::KNN; }

// returns 0, or 1 for what the library refuses: rows_cap < 1, a NULL array, exactly one of cand / verdict, too many rows
int emu_sort_history(int n_frames, const int32_t* offsets, const double* cones, const double* poses, fsdp::SortOut* out, int rows_cap,
                     int32_t* n_rows, int32_t* target_length, int32_t* rows, uint8_t* is_end, int32_t* cand, uint8_t* verdict) {
  if (rows_cap < 1 || !n_rows || !target_length || !rows || !is_end || (cand == nullptr) != (verdict == nullptr)) return 1;
  if ((long long)n_frames * 2 * (long long)rows_cap > 2147483647ll) return 1;
  const size_t total = (size_t)n_frames * 2 * (size_t)rows_cap, per_frame = 2 * (size_t)rows_cap;
  memset(n_rows, 0, sizeof(int32_t) * 2 * (size_t)n_frames);
  memset(target_length, 0, sizeof(int32_t) * 2 * (size_t)n_frames);
  memset(rows, 0xff, sizeof(int32_t) * total * fsdp::MAX_LEN);
  memset(is_end, 0xff, total);
  if (cand) {
    memset(cand, 0xff, sizeof(int32_t) * total * fsdp::KNN);
    memset(verdict, 0xff, total * fsdp::KNN);
  }
  const bool filtered = !g_prm.use_unknown_cones;
  if (filtered) {
    emu_filter(n_frames, offsets, cones);
    offsets = g_f_off.data();
    cones = g_f_cones.data();
  }
  fsdp::SortHistView v;
  v.rows_cap = rows_cap;
  v.n_rows = n_rows;
  v.target_length = target_length;
  v.rows = rows;
  v.is_end = is_end;
  v.cand = cand;
  v.verdict = verdict;
  std::vector<int> big((size_t)n_frames + 1, 0);
  if (emu_sort128(n_frames, offsets)) {
    emu::launch((unsigned)n_frames, 64, [&]() { fsdp::sort_kernel_128_history(n_frames, offsets, cones, poses, out, big.data(), &g_prm, v); });
    g_last_kernels = 1;
  } else {
    emu::launch((unsigned)n_frames, 64, [&]() { fsdp::sort_kernel_history(n_frames, offsets, cones, poses, out, big.data(), &g_prm, v); });
    g_last_kernels = 2;
  }
  g_last_big = big[0];
  if (big[0] > 0) {
    std::vector<fsdp::SortSharedBig> state(2);
    emu::launch(2, 64, [&]() { fsdp::sort_big_kernel_history(offsets, cones, poses, out, big.data(), state.data(), &g_prm, v); });
    g_last_kernels |= 4;
  }
  if (filtered) {
    emu_sort_remap(n_frames, out);
    for (int f = 0; f < n_frames; f++) {
      emu_map_back(f, rows + (size_t)f * per_frame * fsdp::MAX_LEN, per_frame * fsdp::MAX_LEN);
      if (cand) emu_map_back(f, cand + (size_t)f * per_frame * fsdp::KNN, per_frame * fsdp::KNN);
    }
  }
  return 0;
}
}
