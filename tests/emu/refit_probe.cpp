// TEST INFRASTRUCTURE — what the refit is handed: path_prep_kernel run on the host SIMT emulator, then per frame the
// polyline's place in the arena and its parameter values (the U that fit_kernel fits).  A library of its own
// (tests/refit_probe.py builds it), so that tests can say which knot intervals the points of a residual super-chunk fall into.
#include "hip_emu.h"

#include "../../ft-fsd-path-planning_amd/csrc/path_kernel.h"

#include <cstring>
#include <vector>

// (built with -fvisibility=hidden -fno-gnu-unique, tests/refit_probe.py: the kernels' __shared__ blocks and the emulator's state in
// this library are its own, whichever emulator library the process loaded before or loads after it)
#define PROBE_API __attribute__((visibility("default")))

extern "C" {
PROBE_API int probe_path_cap() { return fsdp::PATH_CAP; }
// params17: the configuration constants in the order of fsdp::Params (ints as doubles); default_path: PATH_POINTS x 4
// (emu_default_path of the same parameters).  mid_out: n_frames x 4 int32 (status, fallback, off, n); u_out: n_frames x PATH_CAP
// (the first n entries of a frame with status 0 are its parameter values).  gpath: (n_gpath, 2) or NULL — a context with a global
// path, whose three kernels are the 32-knot instantiations; prev_paths: n_frames x PATH_POINTS x 4 or NULL.
PROBE_API void probe_refit_polyline(int n_frames, const double* poses, const void* matched, const double* default_path, const double* v,
                          int32_t* mid_out, double* u_out, const double* gpath, int n_gpath, const double* prev_paths) {
  const fsdp::Params prm = {(int32_t)v[0], (int32_t)v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12],
                            (int32_t)v[13], (int32_t)v[14], (int32_t)v[15], (int32_t)v[16]};
  constexpr int G = fsdp::PATH_G_SPLIT;
  std::vector<double> arena((size_t)fsdp::ARENA_DOUBLES * n_frames + 8, 0.0);
  double* ar = (double*)(((uintptr_t)arena.data() + 63) & ~(uintptr_t)63);
  std::vector<fsdp::PathMid> mid(n_frames);
  std::vector<fsdp::PathOut> out(n_frames);
  std::vector<int> retry((size_t)n_frames + 1, 0);
  const unsigned per = 64 / G;
  emu::launch(((unsigned)n_frames + per - 1) / per, 64, [&]() {
    if (gpath)
      fsdp::path_prep_kernel<G, fsdp::WIDE_KNOTS>(n_frames, poses, (const fsdp::MatchOut*)matched, default_path, prev_paths, gpath, n_gpath, ar,
                                                  out.data(), mid.data(), retry.data(), &prm);
    else
      fsdp::path_prep_kernel<G, fsdp::FIT_KNOTS>(n_frames, poses, (const fsdp::MatchOut*)matched, default_path, prev_paths, nullptr, 0, ar,
                                                 out.data(), mid.data(), retry.data(), &prm);
  });
  for (int f = 0; f < n_frames; f++) {
    memcpy(mid_out + 4 * f, &mid[f], sizeof(fsdp::PathMid));
    if (mid[f].status != fsdp::ST_OK) continue;
    const fsdp::Arena A = fsdp::frame_arena(ar, f, &prm);
    memcpy(u_out + (size_t)f * fsdp::PATH_CAP, A.u + mid[f].off, sizeof(double) * mid[f].n);
  }
}
}
