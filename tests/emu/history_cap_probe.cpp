// TEST INFRASTRUCTURE — a stand-alone program (make -f history.mk history_cap_probe, built with -fsanitize=address,undefined)
// that drives emu_sort_history (emu_history.cpp) on the capacity cases: every output array is a heap block of exactly the size
// the call documents, so a store beyond rows_cap, beyond a side or beyond the batch is the sanitizer's to report.  A lattice
// frame with R rows on a side at rows_cap = 1, R - 1, R, R + 1 and in full, with and without the verdicts, alone and between two
// small frames; n_rows stays R and the stored prefix is bit-equal.  Exit status 0 and "history_cap_probe ok" when all hold.
#include "emu_shared.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" int emu_sort_history(int n_frames, const int32_t* offsets, const double* cones, const double* poses, fsdp::SortOut* out, int rows_cap,
                                int32_t* n_rows, int32_t* target_length, int32_t* rows, uint8_t* is_end, int32_t* cand, uint8_t* verdict);

struct Call {
  std::vector<fsdp::SortOut> out;
  std::vector<int32_t> n_rows, target, rows, cand;
  std::vector<uint8_t> is_end, verdict;
  int cap = 0;
};

static Call run(const std::vector<int32_t>& off, const std::vector<double>& cones, const std::vector<double>& poses, int cap, bool verdicts) {
  const size_t n = off.size() - 1, total = n * 2 * (size_t)cap;
  Call c;
  c.cap = cap;
  c.out.resize(n);
  c.n_rows.assign(2 * n, -5);
  c.target.assign(2 * n, -5);
  c.rows.assign(total * fsdp::MAX_LEN, -5);
  c.is_end.assign(total, 7);
  if (verdicts) {
    c.cand.assign(total * fsdp::KNN, -5);
    c.verdict.assign(total * fsdp::KNN, 7);
  }
  const int rc = emu_sort_history((int)n, off.data(), cones.data(), poses.data(), c.out.data(), cap, c.n_rows.data(), c.target.data(), c.rows.data(),
                                  c.is_end.data(), verdicts ? c.cand.data() : nullptr, verdicts ? c.verdict.data() : nullptr);
  if (rc != 0) {
    fprintf(stderr, "emu_sort_history refused rows_cap %d\n", cap);
    exit(1);
  }
  return c;
}

#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #x); \
      exit(1);                                                \
    }                                                         \
  } while (0)

// frame f, side s of a call at a smaller cap against the full one: the stored prefix, and the padding behind it
static void same_prefix(const Call& a, const Call& full, int f, int s, bool verdicts) {
  const int n = full.n_rows[2 * f + s];
  CHECK(a.n_rows[2 * f + s] == n && a.target[2 * f + s] == full.target[2 * f + s]);
  for (int r = 0; r < a.cap; r++) {
    const size_t ia = ((size_t)(2 * f + s) * a.cap + r), ib = ((size_t)(2 * f + s) * full.cap + r);
    const bool stored = r < n;
    for (int l = 0; l < fsdp::MAX_LEN; l++) CHECK(a.rows[ia * fsdp::MAX_LEN + l] == (stored ? full.rows[ib * fsdp::MAX_LEN + l] : -1));
    CHECK(a.is_end[ia] == (stored ? full.is_end[ib] : 0xFF));
    if (verdicts)
      for (int q = 0; q < fsdp::KNN; q++) {
        CHECK(a.cand[ia * fsdp::KNN + q] == (stored ? full.cand[ib * fsdp::KNN + q] : -1));
        CHECK(a.verdict[ia * fsdp::KNN + q] == (stored ? full.verdict[ib * fsdp::KNN + q] : 0xFF));
      }
  }
}

int main() {
  // a colourless, jittered 6 x 7 lattice of 3 m in front of the car (some forty rows on its longer side), between two frames of three
  // cones a side
  std::vector<double> small;
  for (int i = 0; i < 3; i++) {
    const double l[3] = {1.0 + 3.0 * i, 1.5, 2.0}, r[3] = {1.0 + 3.0 * i, -1.5, 1.0};
    small.insert(small.end(), l, l + 3);
    small.insert(small.end(), r, r + 3);
  }
  std::vector<double> lattice;
  unsigned long long st = 4;  // (a fixed linear congruential sequence: the cones are moved off the grid by up to 0.6 m)
  auto jitter = [&]() {
    st = (st * 1103515245ull + 12345ull) % (1ull << 31);
    return (double)((st >> 8) % 1000ull) / 1000.0 - 0.5;
  };
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 7; j++) {
      const double jx = jitter(), jy = jitter();
      const double c[3] = {1.0 + 3.0 * i + 1.2 * jx, -9.0 + 3.0 * j + 1.2 * jy, 0.0};
      lattice.insert(lattice.end(), c, c + 3);
    }
  std::vector<double> cones(small);
  cones.insert(cones.end(), lattice.begin(), lattice.end());
  cones.insert(cones.end(), small.begin(), small.end());
  const std::vector<int32_t> off = {0, 6, 48, 54};
  std::vector<double> poses;
  for (int f = 0; f < 3; f++) {
    const double p[4] = {0.0, 0.0, 1.0, 0.0};
    poses.insert(poses.end(), p, p + 4);
  }
  const std::vector<int32_t> off1 = {0, 42};
  const std::vector<double> pose1(poses.begin(), poses.begin() + 4);
  int checked = 0;
  for (int v = 0; v < 2; v++) {
    const bool verdicts = v == 0;
    const Call full = run(off, cones, poses, 8192, verdicts);
    const int R = std::max(full.n_rows[2], full.n_rows[3]);
    CHECK(R >= 20 && R <= 8192 && full.n_rows[0] == 3 && full.n_rows[1] == 3 && full.n_rows[4] == 3 && full.n_rows[5] == 3);
    for (int f = 0; f < 3; f++)
      for (int s = 0; s < 2; s++) same_prefix(full, full, f, s, verdicts);
    const int caps[] = {1, R - 1, R, R + 1};
    for (int cap : caps) {
      const Call a = run(off, cones, poses, cap, verdicts);
      for (int f = 0; f < 3; f++)
        for (int s = 0; s < 2; s++) same_prefix(a, full, f, s, verdicts);
      // the lattice frame alone: the same rows at the same caps
      const Call b = run(off1, lattice, pose1, cap, verdicts);
      for (int s = 0; s < 2; s++) {
        CHECK(b.n_rows[s] == full.n_rows[2 + s]);
        for (int r = 0; r < std::min(cap, b.n_rows[s]); r++)
          for (int l = 0; l < fsdp::MAX_LEN; l++)
            CHECK(b.rows[((size_t)s * cap + r) * fsdp::MAX_LEN + l] == full.rows[((size_t)(2 + s) * full.cap + r) * fsdp::MAX_LEN + l]);
      }
      checked++;
    }
  }
  printf("history_cap_probe ok: %d capacity cases\n", checked);
  return 0;
}
