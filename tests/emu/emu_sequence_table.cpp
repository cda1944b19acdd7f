// TEST INFRASTRUCTURE — the chain kernels of a sequence pass with per-frame global paths (csrc/sequence_table_kernel.h:
// seq_chain_table_kernel between seq_mark_kernel and seq_final_kernel of csrc/sequence_kernel.h) under the host SIMT emulator,
// launched the way the library's launch_sequence launches them behind the path stage of a pass with ids (csrc/fsdp_lib.hip).  Built
// by sequence_table.mk into a library of its own together with emu_kernels.cpp (the parameters, emu_shared.h) and
// emu_gpath_table.cpp (the speculative pass: emu_gpt_path).  Never loaded by the package.
#include "emu_shared.h"

#include "../../ft-fsd-path-planning_amd/csrc/sequence_table_kernel.h"

#include <cstdlib>
#include <cstring>

extern "C" {
// The three kernels over the speculative results of a pass with ids (out: every frame planned with the constant initial path and
// its own table entry, e.g. by emu_gpt_path without previous paths); out is resolved in place.  ids: (n_planners * n_steps),
// step-major.  initial_prev / final_prev: (n_planners, PATH_POINTS, 4), the first may be NULL.  blocks: grid of the chain kernel
// (any grid walks any list).  plain_path >= 0: seq_chain_kernel itself with that table entry as the launch's one pair, in the place
// of the twin (what a context with that path set context-wide runs).  Returns the frames planned again.
int emu_seqt_chain(int n_planners, int n_steps, const double* poses, const fsdp::MatchOut* matched, const double* initial_prev,
                   const double* table_xy, const int32_t* table_off, int n_paths, const int32_t* ids, fsdp::PathOut* out, double* final_prev,
                   int blocks, int plain_path) {
  using namespace fsdp;
  const size_t n = (size_t)n_planners * n_steps;
  const GpathTable t{table_xy, table_off, ids, n_paths};
  double* arena = (double*)aligned_alloc(64, sizeof(double) * ARENA_DOUBLES * n);
  memset(arena, 0xff, sizeof(double) * ARENA_DOUBLES * n);  // (whatever the pass left: the chain plans from the MatchOut)
  std::vector<int> seq(SEQ_LIST + 2 * n, 0);
  int32_t replanned = -1;
  emu::launch((unsigned)((n + 63) / 64), 64, [&]() { seq_mark_kernel(n_planners, n_steps, out, seq.data()); });
  if (plain_path >= 0 && plain_path < n_paths) {
    const double* gpath = table_xy + 2 * (size_t)table_off[plain_path];
    const int n_gpath = table_off[plain_path + 1] - table_off[plain_path];
    emu::launch((unsigned)(blocks > 0 ? blocks : 1), 64,
                [&]() { seq_chain_kernel(n_planners, n_steps, poses, matched, initial_prev, gpath, n_gpath, arena, out, seq.data(), &g_prm); });
  } else {
    emu::launch((unsigned)(blocks > 0 ? blocks : 1), 64,
                [&]() { seq_chain_table_kernel(n_planners, n_steps, poses, matched, initial_prev, t, arena, out, seq.data(), &g_prm); });
  }
  emu::launch((unsigned)n_planners, 64, [&]() { seq_final_kernel(n_planners, n_steps, out, initial_prev, final_prev, seq.data(), &replanned); });
  free(arena);
  return replanned;
}
}
