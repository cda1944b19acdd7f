// TEST INFRASTRUCTURE — the chain kernels of a sequence pass (csrc/sequence_kernel.h: seq_mark_kernel, seq_chain_kernel,
// seq_final_kernel) under the host SIMT emulator, launched the way the library's launch_sequence launches them behind the path
// stage (csrc/fsdp_lib.hip).  A translation unit of libfsdp_emu[_wide].so like emu_ranked.cpp; the parameters come from emu_kernels.cpp
// (g_prm, emu_shared.h), and path_kernel.h's kernels, which that unit compiles too, are weak (hip_emu.h).  Never loaded by the package.
#include "emu_shared.h"

#include "../../ft-fsd-path-planning_amd/csrc/match_kernel.h"
#include "../../ft-fsd-path-planning_amd/csrc/sequence_kernel.h"

#include <cstdlib>

extern "C" {
// Test entry point of the head rule alone: frames carry nothing but the injected status / fallback words.  heads: room for
// 2 * n_frames ints, filled with (frame, predecessor) pairs in list order; returns their number.
int emu_sequence_mark(int n_planners, int n_steps, const int32_t* status, const int32_t* fallback, int32_t* heads) {
  const size_t n = (size_t)n_planners * n_steps;
  std::vector<fsdp::PathOut> out(n);
  for (size_t f = 0; f < n; f++) {
    memset((void*)&out[f], 0, sizeof(fsdp::PathOut));
    out[f].status = status[f];
    out[f].fallback = fallback[f];
  }
  std::vector<int> seq(fsdp::SEQ_LIST + 2 * n, 0);
  emu::launch((unsigned)((n + 63) / 64), 64, [&]() { fsdp::seq_mark_kernel(n_planners, n_steps, out.data(), seq.data()); });
  memcpy(heads, seq.data() + fsdp::SEQ_LIST, sizeof(int) * 2 * (size_t)seq[fsdp::SEQ_HEADS]);
  return seq[fsdp::SEQ_HEADS];
}

// The three kernels over the speculative results of a pass (out: every frame planned with the constant initial path, e.g. by
// emu_path_g with no previous paths set); out is resolved in place.  initial_prev / final_prev: (n_planners, PATH_POINTS, 4), the
// first may be NULL.  blocks: grid of seq_chain_kernel (any grid walks any list).  Returns the frames planned again.
int emu_sequence_chain(int n_planners, int n_steps, const double* poses, const fsdp::MatchOut* matched, const double* initial_prev,
                       fsdp::PathOut* out, double* final_prev, int blocks) {
  const size_t n = (size_t)n_planners * n_steps;
  double* arena = (double*)aligned_alloc(64, sizeof(double) * fsdp::ARENA_DOUBLES * n);
  memset(arena, 0xff, sizeof(double) * fsdp::ARENA_DOUBLES * n);  // (whatever the pass left: the chain plans from the MatchOut)
  std::vector<int> seq(fsdp::SEQ_LIST + 2 * n, 0);
  int32_t replanned = -1;
  emu::launch((unsigned)((n + 63) / 64), 64, [&]() { fsdp::seq_mark_kernel(n_planners, n_steps, out, seq.data()); });
  emu::launch((unsigned)(blocks > 0 ? blocks : 1), 64, [&]() {
    fsdp::seq_chain_kernel(n_planners, n_steps, poses, matched, initial_prev, nullptr, 0, arena, out, seq.data(), &g_prm);
  });
  emu::launch((unsigned)n_planners, 64, [&]() { fsdp::seq_final_kernel(n_planners, n_steps, out, initial_prev, final_prev, seq.data(), &replanned); });
  free(arena);
  return replanned;
}
}
