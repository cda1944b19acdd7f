// TEST INFRASTRUCTURE — the TABLE twins of the path stage's wrappers (csrc/gpath_table_kernel.h: per-frame global paths) under the
// host SIMT emulator, launched the way fsdp_lib.hip launches them for a pass that carries path ids.  Built by gpath_table.mk into a
// library of its own together with emu_kernels.cpp, where the parameters and the default path live (emu_shared.h).  Never loaded
// by the package.
#include "emu_shared.h"

#include "../../ft-fsd-path-planning_amd/csrc/gpath_table_kernel.h"

#include <cstdlib>
#include <cstring>

extern "C" void emu_default_path(double* out);

namespace {
struct Arena64 {  // 64-byte aligned scratch like hipMalloc's (the basis records of the arena are alignas(64))
  double* p;
  explicit Arena64(size_t n) : p((double*)aligned_alloc(64, ((n * sizeof(double) + 63) / 64) * 64)) { memset(p, 0, n * sizeof(double)); }
  ~Arena64() { free(p); }
};
int g_gpt_retries = 0;
}  // namespace

extern "C" {
// frames the last emu_gpt_path launch handed to the retry route (form 0: the length of the list it was given)
int emu_gpt_last_retries() { return g_gpt_retries; }

// One path stage over n frames with per-frame global paths.  form: 64 / 16 = path_table_kernel<64> / <16> (+ the retry route for 16),
// 8 = path_table_prep_kernel<8, 32> -> fit_kernel<8, 32> -> path_finish_kernel<8, 32> -> the retry route, 0 = the retry route alone
// over a list of all frames (retry_pack_min = 0: its four-frames-per-wavefront form, the whole wavefront behind it).
// prev: (n, PATH_POINTS, 4) or NULL.  Returns 1 for an unknown form.
int emu_gpt_path(int form, int n, const double* poses, const fsdp::MatchOut* matched, const double* prev, const double* table_xy,
                 const int32_t* table_off, int n_paths, const int32_t* ids, fsdp::PathOut* out) {
  using namespace fsdp;
  static double default_path[PATH_POINTS * 4];
  emu_default_path(default_path);
  const GpathTable t{table_xy, table_off, ids, n_paths};
  Arena64 arena((size_t)ARENA_DOUBLES * n);
  std::vector<int> retry((size_t)n + 1, 0);
  std::vector<PathMid> mid((size_t)n);
  auto run_retry = [&]() {
    g_gpt_retries = retry[0];
    emu::launch(8, 64, [&]() { path_table_retry_kernel(poses, matched, default_path, prev, t, arena.p, out, retry.data(), &g_prm); });
  };
  if (form == 64) {
    emu::launch((unsigned)n, 64, [&]() { path_table_kernel<64>(n, poses, matched, default_path, prev, t, arena.p, out, nullptr, &g_prm); });
    g_gpt_retries = 0;
  } else if (form == 16) {
    emu::launch(((unsigned)n + 3) / 4, 64, [&]() { path_table_kernel<16>(n, poses, matched, default_path, prev, t, arena.p, out, retry.data(), &g_prm); });
    run_retry();
  } else if (form == 8) {
    constexpr int G = PATH_G_SPLIT;
    const unsigned blocks = ((unsigned)n + 64 / G - 1) / (64 / G);
    emu::launch(blocks, 64, [&]() { path_table_prep_kernel<G, WIDE_KNOTS>(n, poses, matched, default_path, prev, t, arena.p, out, mid.data(), retry.data(), &g_prm); });
    emu::launch(blocks, 64, [&]() { fit_kernel<G, WIDE_KNOTS>(n, arena.p, mid.data(), retry.data(), &g_prm, nullptr, nullptr); });
    emu::launch(blocks, 64, [&]() { path_finish_kernel<G, WIDE_KNOTS>(n, arena.p, mid.data(), out, retry.data(), &g_prm); });
    run_retry();
  } else if (form == 0) {
    retry[0] = n;
    for (int f = 0; f < n; f++) retry[1 + (size_t)f] = f;
    run_retry();
  } else {
    return 1;
  }
  return 0;
}

// path_ids_scan_kernel: the lowest frame whose id lies outside [-1, n_paths), or -1
int emu_gpt_ids_scan(int n, int n_paths, const int32_t* ids) {
  int32_t bad = -2;
  emu::launch(1, 64, [&]() { fsdp::path_ids_scan_kernel(n, n_paths, ids, &bad); });
  return bad;
}
}
