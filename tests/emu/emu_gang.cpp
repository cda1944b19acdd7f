// TEST INFRASTRUCTURE — the gang twins of the plain sorting kernels (csrc/sort_kernel.h sort_kernel_128_gang / sort_kernel_gang)
// under the host SIMT emulator, next to the plain kernels with a StageIn: both stage a batch from a source into device copies,
// the twins the batches of several members one behind the other.  Built by gang.mk into a library of its own together with
// emu_kernels.cpp, where the parameters live (emu_shared.h).  Never loaded by the package.
#include "emu_shared.h"

static int g_gang_small = 0;

extern "C" {
// 1: the last emu_sort_gang took the 128-cone state (what emu_sort_staged is to be given for the same members)
int emu_gang_last_small() { return g_gang_small; }

// Member m: n[m] frames, offsets off[m] (off[m][0] may be > 0: a slice), cones[m] = row 0 of the array the offsets index, poses[m].
// The copies (sum of n frames, the members' rows one behind the other) go to dst_*, the records to out.  Returns 1 for too many members.
int emu_sort_gang(int n_members, const int* n, const int32_t* const* off, const double* const* cones, const double* const* poses,
                  int32_t* dst_off, double* dst_cones, double* dst_poses, fsdp::SortOut* out) {
  if (n_members < 1 || n_members > fsdp::GANG_MAX) return 1;
  fsdp::StageGang g;
  int frames = 0, rows = 0, max_cones = 0;
  for (int m = 0; m < n_members; m++) {
    fsdp::StageMember& sm = g.m[g.n_members++];
    sm.src_off = off[m];
    sm.base = off[m][0];
    sm.src_cones = cones[m] + 3 * (size_t)sm.base;
    sm.src_poses = poses[m];
    sm.first_frame = frames;
    sm.first_row = rows;
    for (int f = 0; f < n[m]; f++) max_cones = std::max(max_cones, (int)(off[m][f + 1] - off[m][f]));
    frames += n[m];
    rows += off[m][n[m]] - off[m][0];
  }
  g.dst_off = dst_off;
  g.dst_cones = dst_cones;
  g.dst_poses = dst_poses;
  g.n_frames = frames;
  std::vector<int> big((size_t)frames + 1, 0);
  g_gang_small = max_cones <= fsdp::SortShared128::MAX_N;
  if (g_gang_small)
    emu::launch((unsigned)frames, 64, [&]() { fsdp::sort_kernel_128_gang(g, out, big.data(), &g_prm); });
  else
    emu::launch((unsigned)frames, 64, [&]() { fsdp::sort_kernel_gang(g, out, big.data(), &g_prm); });
  g_last_big = big[0];
  if (big[0] > 0) {  // (from the copies, like any pass)
    std::vector<fsdp::SortSharedBig> state(2);
    emu::launch(2, 64, [&]() { fsdp::sort_big_kernel(dst_off, dst_cones, dst_poses, out, big.data(), state.data(), &g_prm); });
  }
  return 0;
}

// one batch through the plain kernels with a StageIn (what a page-locked ticket's pass does); small: the 128-cone state
void emu_sort_staged(int n, const int32_t* off, const double* cones, const double* poses, int32_t* dst_off, double* dst_cones,
                     double* dst_poses, fsdp::SortOut* out, int small) {
  fsdp::StageIn st;
  st.src_off = off;
  st.base = off[0];
  st.src_cones = cones + 3 * (size_t)st.base;
  st.src_poses = poses;
  st.dst_off = dst_off;
  st.dst_cones = dst_cones;
  st.dst_poses = dst_poses;
  st.n_frames = n;
  std::vector<int> big((size_t)n + 1, 0);
  if (small)
    emu::launch((unsigned)n, 64, [&]() { fsdp::sort_kernel_128(n, dst_off, dst_cones, dst_poses, out, big.data(), &g_prm, st); });
  else
    emu::launch((unsigned)n, 64, [&]() { fsdp::sort_kernel(n, dst_off, dst_cones, dst_poses, out, big.data(), &g_prm, st); });
  if (big[0] > 0) {
    std::vector<fsdp::SortSharedBig> state(2);
    emu::launch(2, 64, [&]() { fsdp::sort_big_kernel(dst_off, dst_cones, dst_poses, out, big.data(), state.data(), &g_prm); });
  }
}
}
