// TEST INFRASTRUCTURE — the shortened FP64 sequences of csrc/device_prims.h compiled for the host as they are written for the
// device (FSDP_SEQ_MODEL: rcp_refined, div_rcp, sqrt_1_2, givens_dd_rd keep their device bodies; fma is the host's exact fma), and
// with them fpgivs_guarded<true> of spline_device.h, guard expression included.  The two hardware seeds are a MODEL: the
// correctly rounded value times (1 + eps), eps settable (seq_set_seed_eps).  What v_rcp_f64 / v_rsq_f64 return on gfx950 is
// not measured anywhere in this repository; the GPU test (tests/test_hard_rounding_gpu.py) is the verdict, this library is
// what lets the CPU suite run the arithmetic at all.  A library of its own (tests/seq_model.py builds it on demand).
#include "hip_emu.h"

#define FSDP_SEQ_MODEL 1

namespace fsdp {
static double g_eps_rcp = 0.0, g_eps_rsq = 0.0;
// 1 / d is one IEEE division: correctly rounded
inline double seq_model_rcp(double d) { return (1.0 / d) * (1.0 + g_eps_rcp); }
// 1 / sqrt(x) evaluated with a 64-bit significand and rounded once more: correctly rounded unless that value falls within
// 2^-11 ulp of a midpoint (x in [1, 2] here: no range concerns)
inline double seq_model_rsq(double x) { return (double)(1.0L / sqrtl((long double)x)) * (1.0 + g_eps_rsq); }
}  // namespace fsdp

#include "../../ft-fsd-path-planning_amd/csrc/spline_device.h"

#define SEQ_API __attribute__((visibility("default")))

// v moved by `ulps` representable values (away from / towards zero for positive / negative counts)
static double moved(double v, int ulps) {
  for (int k = 0; k < (ulps < 0 ? -ulps : ulps); k++) v = std::nextafter(v, ulps > 0 ? (v > 0 ? INFINITY : -INFINITY) : 0.0);
  return v;
}

extern "C" {
SEQ_API void seq_set_seed_eps(double eps_rcp, double eps_rsq) {
  fsdp::g_eps_rcp = eps_rcp;
  fsdp::g_eps_rsq = eps_rsq;
}
SEQ_API void seq_rcp_refined(int n, const double* d, double* out) {
  for (int i = 0; i < n; i++) out[i] = fsdp::rcp_refined(d[i]);
}
// out[i] = div_rcp(a, b, rcp_refined(b)) — what fpbspl3's quot and math_selftest_kernel compute; r_ulps != 0: the mutation,
// the refined reciprocal moved by that many representable values before the quotient uses it
SEQ_API void seq_div(int n, const double* a, const double* b, double* out, int r_ulps) {
  for (int i = 0; i < n; i++) out[i] = fsdp::div_rcp(a[i], b[i], moved(fsdp::rcp_refined(b[i]), r_ulps));
}
SEQ_API void seq_sqrt_1_2(int n, const double* x, double* out) {
  for (int i = 0; i < n; i++) out[i] = fsdp::sqrt_1_2(x[i]);
}
// out = [cs | sn | dd | guard (1 = inside the band)] of fpgivs_guarded<true>(piv, ww); rd_ulps != 0: the mutation — the same
// statements with rd moved between givens_dd_rd and the two quotients
SEQ_API void seq_givens(int n, const double* piv, const double* ww, double* out, int rd_ulps) {
  for (int i = 0; i < n; i++) {
    double w = ww[i], cs, sn;
    int bad = 0;
    if (rd_ulps == 0) {
      fsdp::fpgivs_guarded<true>(piv[i], w, cs, sn, bad);
    } else {
      const double den = fsdp::max_abs_nn(piv[i], w), num = fsdp::min_abs_nn(piv[i], w);
      bad |= (int)!((den >= 0x1p-255) & (den <= 0x1p+255) & ((num == 0.0) | (num >= 0x1p-255)));
      double dd, rd;
      fsdp::givens_dd_rd(den, num, dd, rd);
      rd = moved(rd, rd_ulps);
      cs = fsdp::div_rcp(w, dd, rd);
      sn = fsdp::div_rcp(piv[i], dd, rd);
      w = dd;
    }
    out[i] = cs;
    out[(size_t)n + i] = sn;
    out[2 * (size_t)n + i] = w;
    out[3 * (size_t)n + i] = bad ? 0.0 : 1.0;
  }
}
// in_div_band(a) && in_div_band(b), the flag of math_selftest_kernel
SEQ_API void seq_in_band(int n, const double* a, const double* b, double* out) {
  for (int i = 0; i < n; i++) out[i] = (fsdp::in_div_band(a[i]) && fsdp::in_div_band(b[i])) ? 1.0 : 0.0;
}
}
