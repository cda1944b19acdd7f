// The seam between the two builds of the kernel sources: hipcc for gfx950 (the product) and the host SIMT emulator of the
// CPU tests (tests/emu, whose shim header defines FSDP_EMU).  Every function that has a device definition and an emulator
// definition is here, the two side by side — and with them all the inline assembly and every __builtin_amdgcn_* call the
// library emits.  The kernel headers hold neither: what a kernel does is the same text in both builds.
//
// Two kinds of hardware primitive need no second form and so no branch: the HIP wave intrinsics (__shfl, __shfl_xor,
// __ballot, __syncthreads, atomics) and the builtins the emulator declares under their own names as host functions
// (__builtin_amdgcn_readfirstlane: the identity on a value every lane holds; __builtin_amdgcn_fence / s_waitcnt / s_sleep:
// nothing, its workgroups run one after the other).  fsdp_device.h's wave primitives (wave_bcast, wave_uniform, wave_argmin)
// use the former and readfirstlane as they are; the release / back-off pair of the skidpad hand-off is below, unbranched.
//
// The emulator keeps direct IEEE forms (a / b, sqrt) where the device runs a shortened sequence from a hardware rcp / rsq
// seed: the sequences return the correctly rounded result (held against the IEEE operations on the device by
// fsdp_selftest_math / givens / absminmax, tests/test_gpu_parity.py; on operands built to be hard to round and on the band's
// edges, tests/test_hard_rounding_gpu.py), so both builds compute the same bits.
//
// A third build reads the sequences themselves on the host: with FSDP_SEQ_MODEL next to FSDP_EMU (tests/emu/seq_model.cpp)
// rcp_refined, div_rcp, sqrt_1_2 and givens_dd_rd keep their DEVICE bodies, and the two seed instructions in them,
// v_rcp_f64 and v_rsq_f64, are a model the including file provides (fsdp::seq_model_rcp / seq_model_rsq).  Everything else
// keeps its emulator form.  FSDP_RCP_SEED / FSDP_RSQ_SEED are the builtins themselves in the device build.
#pragma once

#include <stdint.h>

#ifndef FSDP_EMU
#include <hip/hip_runtime.h>
#endif

#if defined(FSDP_EMU) && !defined(FSDP_SEQ_MODEL)
#define FSDP_EMU_IEEE_FORMS 1  // the emulator's a / b and sqrt in place of the shortened sequences
#endif
#ifdef FSDP_SEQ_MODEL
#define FSDP_RCP_SEED(x) seq_model_rcp(x)
#define FSDP_RSQ_SEED(x) seq_model_rsq(x)
#else
#define FSDP_RCP_SEED(x) __builtin_amdgcn_rcp(x)
#define FSDP_RSQ_SEED(x) __builtin_amdgcn_rsq(x)
#endif

namespace fsdp {

constexpr int WAVE = 64;

// wavefronts per SIMD a kernel is compiled for (its register budget)
#ifdef FSDP_EMU
#define FSDP_WAVES_PER_EU(n)  // (the host emulator's compiler does not parse an expression in an attribute it does not know)
#else
#define FSDP_WAVES_PER_EU(n) __attribute__((amdgpu_waves_per_eu(n)))
#endif

// ------------------------------------------------------------------------------------------
// lane groups: G lanes per frame, WAVE / G frames per wavefront
// ------------------------------------------------------------------------------------------
// The sorting / matching kernels give a frame the whole wavefront (G = 64).  The path stage is dominated by
// serial FP64 chains (spline QR) that keep 1-4 lanes busy, so it packs WAVE / G frames into one wavefront
// (G = 16: four frames, one per DPP row): a serial instruction then advances four frames at once.  Groups are
// aligned; control flow is uniform WITHIN a group and may diverge BETWEEN groups (the hardware runs the union of
// the paths, masked).  Cross-lane traffic never leaves a group.  sync() orders LDS / scratch hand-offs between the
// lanes of a group: with one wavefront per workgroup the lanes run in lock-step, so only the compiler and the memory
// counters need a fence (no s_barrier, which must not sit in divergent code).
template <int G>
struct Grp {
  static_assert(G == 4 || G == 8 || G == 16 || G == 32 || G == 64, "group size");
  static constexpr int SIZE = G;
  static constexpr int PER_WAVE = WAVE / G;
  static __device__ __forceinline__ int lane() { return (int)(threadIdx.x & (G - 1)); }
  static __device__ __forceinline__ int index() { return (int)((threadIdx.x & 63) / G); }
  static __device__ __forceinline__ void sync() {
#ifdef FSDP_EMU
    emu::gbarrier(G);
#else
    if constexpr (G == WAVE) {
      __syncthreads();
    } else {
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __builtin_amdgcn_wave_barrier();
    }
#endif
  }
  // bit i = lane i of this group
  static __device__ __forceinline__ unsigned long long ballot(bool p) {
#ifdef FSDP_EMU
    return emu::gballot(p, G);
#else
    unsigned long long m = __ballot(p);
    if constexpr (G == WAVE)
      return m;
    else
      return (m >> (index() * G)) & ((1ull << G) - 1ull);
#endif
  }
  // value of group lane `src` (group-uniform src)
  template <class T>
  static __device__ __forceinline__ T bcast(T v, int src) {
#ifdef FSDP_EMU
    return emu::gexchange(v, (emu::B->cur & ~(G - 1)) | src, G);
#else
    return __shfl(v, (int)((threadIdx.x & 63) & ~(G - 1)) | src, WAVE);
#endif
  }
  template <class T>
  static __device__ __forceinline__ T shfl_xor(T v, int mask) {
#ifdef FSDP_EMU
    return emu::gexchange(v, emu::B->cur ^ mask, G);
#else
    return __shfl_xor(v, mask, WAVE);
#endif
  }
  // value of the previous lane of the group (lane 0 keeps its own)
  template <class T>
  static __device__ __forceinline__ T shfl_up1(T v) {
#ifdef FSDP_EMU
    return emu::gexchange(v, lane() > 0 ? emu::B->cur - 1 : emu::B->cur, G);
#else
    int me = (int)(threadIdx.x & 63);
    return __shfl(v, lane() > 0 ? me - 1 : me, WAVE);
#endif
  }
  // value of the next lane of the group (the last lane keeps its own)
  template <class T>
  static __device__ __forceinline__ T shfl_down1(T v) {
#ifdef FSDP_EMU
    return emu::gexchange(v, lane() < G - 1 ? emu::B->cur + 1 : emu::B->cur, G);
#else
    int me = (int)(threadIdx.x & 63);
    return __shfl(v, lane() < G - 1 ? me + 1 : me, WAVE);
#endif
  }
  // argmin over (value, index) pairs with "first smallest" semantics; lanes holding no candidate pass idx = -1.  A NaN is
  // larger than every number and NaNs order by index (np.argsort's order; a caller that wants np.argmin's, the first NaN, maps
  // its NaNs below its numbers first): a total order, so every lane of the group ends with the same pair whatever the values
  // are — with `<` and `==` alone a NaN left each lane with a candidate of its own.
  static __device__ __forceinline__ void argmin(double& v, int& idx) {
    for (int off = G / 2; off >= 1; off >>= 1) {
      double ov = shfl_xor(v, off);
      int oi = shfl_xor(idx, off);
      const bool vn = v != v;
      const bool before = (ov != ov) ? (vn && oi < idx) : (vn || ov < v || (ov == v && oi < idx));
      bool take = (oi >= 0) && (idx < 0 || before);
      if (take) {
        v = ov;
        idx = oi;
      }
    }
  }
};

// ---- DPP moves of the Givens pipelines (spline_device.h giv_step) ----------------------------------------
__device__ __forceinline__ double quad_prev(double d) {  // value of the previous lane of the quad (lane 0 <- lane 3)
#ifdef FSDP_EMU
  int l = emu::B->cur;
  return emu::gexchange(d, (l & ~3) | ((l + 3) & 3), 4);
#else
  int lo = __double2loint(d), hi = __double2hiint(d);
  lo = __builtin_amdgcn_mov_dpp(lo, 0x93, 0xf, 0xf, true);  // quad_perm:[3,0,1,2]
  hi = __builtin_amdgcn_mov_dpp(hi, 0x93, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
#endif
}
// DPP moves of a double inside a row of 16 lanes.  CTRL: 0x124 = row_ror:4 (lane i <- lane i - 4 mod 16), 0x00 = quad_perm
// [0,0,0,0], 0xE9 = quad_perm [1,2,2,3]
template <int CTRL>
__device__ __forceinline__ double dpp_row16(double d) {
#ifdef FSDP_EMU
  const int l = emu::B->cur, r = l & 15, base = l & ~15;
  int src;
  if (CTRL == 0x124)
    src = base | ((r + 12) & 15);
  else if (CTRL == 0x00)
    src = l & ~3;
  else
    src = (l & ~3) | ((l & 3) == 0 ? 1 : ((l & 3) == 3 ? 3 : 2));
  return emu::gexchange(d, src, 16);
#else
  int lo = __double2loint(d), hi = __double2hiint(d);
  lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, true);
  hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
#endif
}

// ---- exact division without the range scaling ---------------------------------------------------------
// An IEEE double division on gfx950 is a software sequence: v_div_scale (x2), v_rcp_f64, two Newton steps, a quotient
// with one correction (v_div_fmas) and v_div_fixup.  The scaling and the fix-up only act when an exponent sits near the
// limits of the format; for operands in a safe band the sequence below is that arithmetic without them, with one Newton
// step more on the reciprocal (the compiler's two leave it an ulp off for some divisors, and the quotient then one ulp off
// for some numerators: rcp_newton2) — the correctly rounded quotient with 10 instead of 11 instructions, and two quotients
// over one denominator share the refined reciprocal (13 instead of 22).  The guard: callers flag operands outside [2^-255, 2^255]
// (float compares on the operands; the knot differences once per knot set) and such a frame is re-planned with plain
// divisions (ST_RETRY, path_kernel.h).
// max(|a|, b) / min(|a|, b) of numbers that are never NaN: one v_max_f64 / v_min_f64 each (the absolute value is a source
// modifier; fmax() would first quiet both operands)
__device__ __forceinline__ double max_abs_nn(double a, double b) {
#ifdef FSDP_EMU
  return fabs(a) >= b ? fabs(a) : b;
#else
  double r;
  asm("v_max_f64 %0, |%1|, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
#endif
}
__device__ __forceinline__ double min_abs_nn(double a, double b) {
#ifdef FSDP_EMU
  return fabs(a) >= b ? b : fabs(a);
#else
  double r;
  asm("v_min_f64 %0, |%1|, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
#endif
}
// v_rcp_f64 and two Newton steps: what the compiler's division refines its reciprocal to.  Within an ulp of 1 / d but NOT always
// the correctly rounded one (measured on gfx950: d = 0x1.ffffffffffffb 2^k comes out one ulp low), and a quotient corrected
// with such an r can land on the wrong side of a rounding midpoint (0x1.6666666666663 / 0x1.ffffffffffffb did, in this
// sequence and in the compiler's: tests/test_hard_rounding_gpu.py).
__device__ __forceinline__ double rcp_newton2(double d) {
#ifdef FSDP_EMU_IEEE_FORMS
  return d;  // (the emulator divides directly, see div_rcp)
#else
  double r = FSDP_RCP_SEED(d);
  double e = fma(-d, r, 1.0);
  r = fma(r, e, r);
  e = fma(-d, r, 1.0);
  r = fma(r, e, r);
  return r;
#endif
}
// One more Newton step on a reciprocal that is within an ulp: the correctly rounded 1 / d (Markstein: for every d whose
// mantissa is not all ones; for that one the two steps above already return it on this hardware and the step keeps it).
__device__ __forceinline__ double rcp_newton_last(double d, double r) {
#ifdef FSDP_EMU_IEEE_FORMS
  return r;
#else
  const double e = fma(-d, r, 1.0);
  return fma(r, e, r);
#endif
}
// the correctly rounded reciprocal: what div_rcp needs to return the correctly rounded quotient
__device__ __forceinline__ double rcp_refined(double d) { return rcp_newton_last(d, rcp_newton2(d)); }
// n / d given r = rcp_refined(d)
__device__ __forceinline__ double div_rcp(double n, double d, double r) {
#ifdef FSDP_EMU_IEEE_FORMS
  (void)r;
  return n / d;
#else
  const double q = n * r;
  const double rem = fma(-d, q, n);
  return fma(rem, r, q);
#endif
}
// n / d given r2 = rcp_newton2(d), for a quotient at the head of a dependent chain: the product and its exact remainder take r2
// as it is, the last Newton step runs next to them (it needs r2 only), and the correction takes the correctly rounded
// reciprocal.  Two instructions more than div_rcp, no link more.
__device__ __forceinline__ double div_rcp_late(double n, double d, double r2) {
#ifdef FSDP_EMU_IEEE_FORMS
  (void)r2;
  return n / d;
#else
  const double q = n * r2;
  const double rem = fma(-d, q, n);
  return fma(rem, rcp_newton_last(d, r2), q);
#endif
}

// a / b for the plain-division route (ST_RETRY) and wherever the fast route's counterpart is div_rcp: the compiler's division,
// whose result is within an ulp but on gfx950 not always the correctly rounded one (above), followed by the choice between it
// and its neighbour on the side of the exact remainder — the one with the smaller remainder is the correctly rounded quotient
// (a quotient of two doubles is never a midpoint: no ties).  Operands whose remainders could underflow or overflow keep
// the compiler's result.
__device__ __forceinline__ double div_exact(double a, double b) {
#ifdef FSDP_EMU
  return a / b;
#else
  const double q = a / b;
  const double aa = fabs(a), aq = fabs(q);
  const double rem = fma(-b, q, a);  // exact
  const bool safe = (aa >= 0x1p-900) & (aa <= 0x1p900) & (aq >= 0x1p-900) & (aq <= 0x1p900) & (rem != 0.0);
  const bool grow = ((rem > 0.0) == (b > 0.0)) == (q > 0.0);  // the exact quotient lies beyond q in magnitude
  const double qn = __longlong_as_double(__double_as_longlong(q) + (grow ? 1ll : -1ll));
  const double remn = fma(-b, qn, a);
  return (safe & (fabs(remn) < fabs(rem))) ? qn : q;
#endif
}

// sqrt for arguments in [1, 2] (1 + r^2 with |r| <= 1): the correctly rounded result, i.e. what sqrt() returns; on the
// device this is the compiler's own v_rsq_f64 + Goldschmidt sequence without the range scaling that [1, 2] never needs
// (checked against sqrt() on the GPU: tests/test_gpu_parity.py::test_device_math_helpers)
__device__ __forceinline__ double sqrt_1_2(double x) {
#ifdef FSDP_EMU_IEEE_FORMS
  return sqrt(x);
#else
  double y = FSDP_RSQ_SEED(x);
  double g = x * y;
  double h = y * 0.5;
  double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  double d = fma(-g, g, x);
  g = fma(d, h, g);
  d = fma(-g, g, x);
  g = fma(d, h, g);
  return g;
#endif
}

// The middle of fpgivs for operands in the divisions' safe band: den = max(|piv|, ww), num = min(|piv|, ww) ->
//   dd = den * sqrt(1 + (num / den)^2)   and   rd = a refined reciprocal of dd for the two quotients cs = ww / dd, sn = piv / dd.
// The reciprocal is the head of the second half of the step's dependent chain (rcp_refined(dd): v_rcp_f64 and two Newton steps, five
// links after dd is known).  Its seed need not wait for dd: 1 / dd = (1 / den) * (1 / sqrt(x)), and both factors exist while the square
// root is still being corrected — rq = rcp_refined(den) from the first quotient, and h, the half reciprocal square root the
// Goldschmidt iteration refines next to g (relative error ~2^-45 after its coupled step, what v_rcp_f64 + ONE Newton step gives).
// r0 = (2 rq) h is formed in the shadow of sqrt's last two corrections, and ONE Newton step against dd itself (error^2 ~ 2^-90, then
// the rounding of the fma) makes it the reciprocal rcp_refined returns for all the quotients care: two links after dd instead of
// five, three instructions less per step.  The quotients are div_rcp's (product, exact remainder, correction): correctly rounded
// with either reciprocal (fsdp_selftest_givens holds cs / sn / dd against the IEEE operations on the device: tests/test_gpu_parity.py).
// The form before it, dd = den * sqrt_1_2(x) and rd = rcp_refined(dd) from v_rcp_f64 again, was the A side of the measurement that
// kept the seed (p50 885 -> 857 us, profiles/r05_givens_step.txt).
__device__ __forceinline__ void givens_dd_rd(double den, double num, double& dd, double& rd) {
#ifdef FSDP_EMU_IEEE_FORMS
  const double q = num / den;
  dd = den * sqrt(1.0 + q * q);
  rd = dd;  // (the emulator's div_rcp divides directly)
#else
  const double rq = rcp_newton2(den);  // (as a SEED for rd below an ulp is nothing; the quotient corrects with the last step's)
  const double q = div_rcp_late(num, den, rq);
  const double x = 1.0 + q * q;
  // sqrt_1_2(x), keeping h
  double y = FSDP_RSQ_SEED(x);
  double g = x * y;
  double h = y * 0.5;
  double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  const double r0 = (rq + rq) * h;  // ~ 1 / (den sqrt(x)), off the chain
  double d = fma(-g, g, x);
  g = fma(d, h, g);
  d = fma(-g, g, x);
  g = fma(d, h, g);
  dd = den * g;
  const double e = fma(-dd, r0, 1.0);
  rd = fma(r0, e, r0);
#endif
}

// 1 / sqrt(n2) for the normalised edge of inside_ellipse_of_edge (sort_kernel.h): the reciprocal square root with one Newton
// step, no libm call (a few ulp: the criterion it feeds decides only outside 1e-6 of its boundary)
__device__ __forceinline__ double rsq_newton(double n2) {
#ifdef FSDP_EMU
  return 1.0 / sqrt(n2);
#else
  double rn = __builtin_amdgcn_rsq(n2);  // (n2 = 0: inf / NaN below -> the exact path)
  rn = rn * (1.5 - 0.5 * n2 * rn * rn);
  return rn;
#endif
}

// The arc cosine behind acos_less / acos_greater (fsdp_device.h), evaluated only when a cosine lies within 1e-9 of its threshold.
// On the device it is a CALL: inlined, every predicate carried its own copy of the device library's acos, and
// the polynomial's coefficients — shared by the copies, hoisted to the top of the sorting kernel — stayed alive across the whole kernel
// and were spilled to scratch (18 registers, re-read by eight dependent scratch loads inside every acos of the cost phase).
#ifdef FSDP_EMU
__device__ __forceinline__ double acos_cold(double c) { return acos(c); }
#else
__device__ __attribute__((noinline)) inline double acos_cold(double c) { return acos(c); }
#endif

// fit_kernel, optional (fsdp_time_runs): when did the launch's first wavefront start and its last one end, on the device's
// constant-rate clock — the kernel's duration as a kernel trace reports it, without the wait of its queue that an event bracket
// includes.  The emulator has no such clock and notes nothing.
__device__ __forceinline__ void note_clock_first(unsigned long long* clock_first) {
#ifndef FSDP_EMU
  if (clock_first && threadIdx.x == 0) atomicMin(clock_first, (unsigned long long)wall_clock64());
#endif
}
__device__ __forceinline__ void note_clock_last(unsigned long long* clock_last) {
#ifndef FSDP_EMU
  if (clock_last && threadIdx.x == 0) atomicMax(clock_last, (unsigned long long)wall_clock64());
#endif
}

// skid_path_kernel's hand-off between workgroups (skidpad_kernel.h), one form for both builds (see the top of this file):
// the pause between two polls of a flag, and "the stores above have left the wavefront (they are acknowledged)" before a flag
// goes out — no cache write-back: nothing else the wavefront wrote is anybody's before the launch ends
__device__ __forceinline__ void poll_pause() { __builtin_amdgcn_s_sleep(8); }
__device__ __forceinline__ void stores_acknowledged() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_waitcnt(0);
}

}  // namespace fsdp
