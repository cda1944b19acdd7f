// TEST INFRASTRUCTURE — CPU oracle for the PathPlanner hot path.  Never shipped, never
// imported by the product package (ft-fsd-path-planning_amd/); only tests/, bench.py's
// cpu_baseline leg and __graft_entry__.smoke() may load the library built from oracle/.
//
// np_compat.h: small helpers that restate the NumPy semantics the reference relies on
// (summation order, arange/linspace fill rules, Python min/max with NaN, floored modulo).
// Each helper names the NumPy behaviour it mirrors; none of this is reference source.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include <algorithm>

namespace fsdo {

struct Vec2 {
  double x, y;
};

// Exceptions mirroring the Python control flow of the reference.
//  PyValueError  : raised where the reference raises ValueError (or a subclass such as
//                  numpy.linalg.LinAlgError) — caught by the same try/except sites
//                  (calculate_path/core_calculate_path.py:214-221, :561-570).
//  RefUndefined  : the reference raises an exception that propagates out of
//                  calculate_path_in_global_frame (IndexError etc., SURVEY.md §8a quirks
//                  8/10) or would corrupt memory under numba.  Carries a status code.
struct PyValueError {
  int where;
};
struct RefUndefined {
  int code;
};

static const double PI = 3.14159265358979323846;  // == numpy.pi

inline double deg2rad(double d) { return d * (PI / 180.0); }  // numpy.deg2rad: x * (pi/180)

// numpy pairwise summation (numpy/core/src/umath/loops_utils.h.src, DOUBLE_pairwise_sum):
// n < 8 sequential; n <= 128 eight-way unrolled; otherwise recursive halves.
inline double np_pairwise(const double* a, long n, long stride = 1) {
  if (n < 8) {
    double res = 0.;
    for (long i = 0; i < n; i++) res += a[i * stride];
    return res;
  } else if (n <= 128) {
    double r[8];
    for (int j = 0; j < 8; j++) r[j] = a[j * stride];
    long i;
    for (i = 8; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; j++) r[j] += a[(i + j) * stride];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += a[i * stride];
    return res;
  } else {
    long n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise(a, n2, stride) + np_pairwise(a + n2 * stride, n - n2, stride);
  }
}
// add.reduce over a contiguous/strided 1-D run: identity 0 + pairwise
inline double np_sum(const double* a, long n, long stride = 1) { return 0.0 + np_pairwise(a, n, stride); }
inline double np_sum(const std::vector<double>& v) { return np_sum(v.data(), (long)v.size()); }

// Python's builtin max/min on floats (first argument wins unless the other compares
// strictly greater/smaller) — matters only for NaN propagation.
inline double py_max(double a, double b) { return (b > a) ? b : a; }
inline double py_min(double a, double b) { return (b < a) ? b : a; }

// numpy float remainder for positive divisor (npy_divmod): fmod then sign fix-up.
inline double np_mod(double a, double b) {
  double m = std::fmod(a, b);
  if (m != 0.0) {
    if ((b < 0) != (m < 0)) m += b;
  } else {
    m = std::copysign(0.0, b);
  }
  return m;
}
// utils/math_utils.py:663-676 and trace_sorter/end_configurations.py:303-317
inline double angle_difference(double a1, double a2) { return np_mod(a1 - a2 + 3 * PI, 2 * PI) - PI; }

inline double np_sign(double v) { return (v > 0) ? 1.0 : ((v < 0) ? -1.0 : (v == 0 ? 0.0 : v)); }

// --- BLAS-backed NumPy calls -----------------------------------------------------------------
// np.dot (hence utils/math_utils.py rotate / my_cdist_sq_euclidean) and np.linalg.norm of a
// 1-D vector (sqrt(dot(x,x))) go through OpenBLAS.  On the machine the golden vectors were
// captured on (AVX-512, OpenBLAS SkylakeX kernels) every such inner product is accumulated
// as a fused-multiply-add chain in k order:  acc = a0*b0; acc = fma(a_k, b_k, acc)
// (checked against np.dot on 20k random operands: 100 % agreement for ddot/dgemv/dgemm, see
// tests/test_oracle_numpy_semantics.py).  fma() is exact by IEEE-754, so the restatement is
// portable; on a BLAS without FMA the reference itself would differ in the last bit.
inline double blas_dot2(double a0, double b0, double a1, double b1) { return std::fma(a1, b1, a0 * b0); }
// np.dot of ONE point with a 2 x 2 matrix (a 1-D vector, or a (1, 2) array): NumPy hands that to gemv, whose OpenBLAS kernel
// forms the products in the other order — fma(a0, b0, a1 * b1); from two rows on it is gemm: blas_dot2.  Measured on the
// build container's NumPy (tests/test_oracle_numpy_semantics.py::test_dot_of_a_single_point_is_gemv_order); where it matters:
// the skidpad mission rotates the car's position as a single point (skidpad_relocalizer.py:140-153, math_utils.py:103-117)
// — round 3 attributed the 2 / 341 sample-count flips of the skidpad replay to glibc's sin / cos; they were this.
inline double blas_dot2_single_row(double a0, double b0, double a1, double b1) { return std::fma(a0, b0, a1 * b1); }

// np.linalg.norm of a 1-D 2-vector: sqrt(x.dot(x))  (BLAS ddot)
inline double norm2(double x, double y) { return std::sqrt(blas_dot2(x, x, y, y)); }
// np.linalg.norm(v, axis=-1) on an (n,2) array: sqrt(add.reduce(v*v)) — not BLAS
inline double norm2_axis(double x, double y) { return std::sqrt(x * x + y * y); }

// utils/math_utils.py:70-100 vec_angle_between for one pair of 2-vectors:
//   cos = sum(v1*v2); cos /= (sqrt(sum(v1*v1)) * sqrt(sum(v2*v2))); clip; arccos
inline double vec_angle_between(double ax, double ay, double bx, double by) {
  double c = ax * bx + ay * by;
  c /= std::sqrt(ax * ax + ay * ay) * std::sqrt(bx * bx + by * by);
  if (c < -1) c = -1;
  if (c > 1) c = 1;
  return std::acos(c);
}

// utils/math_utils.py:103-117 rotate: points @ [[c,-s],[s,c]].T
struct Rot {
  double c, s;
  explicit Rot(double theta) : c(std::cos(theta)), s(std::sin(theta)) {}
  // points @ [[c, s], [-s, c]]  (BLAS gemm/gemv, K = 2)
  inline Vec2 apply(double x, double y) const { return Vec2{blas_dot2(x, c, y, -s), blas_dot2(x, s, y, c)}; }
};

// utils/math_utils.py:120-150 my_cdist_sq_euclidean, one entry: the expansion form
// [1,1,ax,ay,ax^2,ay^2] . [bx^2,by^2,-2bx,-2by,1,1] handed to BLAS dgemm (K = 6): an FMA
// chain in k order, see the BLAS note above.
inline double cdist_sq(double ax, double ay, double bx, double by) {
  double acc = 1.0 * (bx * bx);
  acc = std::fma(1.0, by * by, acc);
  acc = std::fma(ax, -2 * bx, acc);
  acc = std::fma(ay, -2 * by, acc);
  acc = std::fma(ax * ax, 1.0, acc);
  acc = std::fma(ay * ay, 1.0, acc);
  return acc;
}

// numpy.arange(0, stop, step) for Python floats: length ceil(stop/step), value i*step
inline long arange_len(double stop, double step) {
  double q = stop / step;
  if (!(q > 0)) return 0;
  return (long)std::ceil(q);
}

// stable argsort of a short array (NumPy's default sort is insertion sort for n<=16 and
// otherwise only differs from stable on exact ties).  NaN sorts last, as in NumPy (and `<` alone would be no ordering).
inline std::vector<int> argsort(const std::vector<double>& v) {
  std::vector<int> idx(v.size());
  for (size_t i = 0; i < v.size(); i++) idx[i] = (int)i;
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return v[a] < v[b] || (v[b] != v[b] && v[a] == v[a]); });
  return idx;
}
// np.argmin / np.min of a non-empty run: the first smallest, and a NaN is smaller than everything (the first NaN wins; np.min
// returns it)
inline int np_argmin(const std::vector<double>& v) {
  int best = 0;
  for (size_t j = 1; j < v.size(); j++) {
    if (v[best] != v[best]) break;
    if (v[j] < v[best] || v[j] != v[j]) best = (int)j;
  }
  return best;
}

// sign of det([[1,x0,y0],[1,x1,y1],[1,x2,y2]]) the way numpy.linalg.det gets it:
// LAPACK dgetrf (partial pivoting, column-major), product of the diagonal, sign flips.
inline double det3_lu(const double m_in[3][3]) {
  const double x0 = m_in[0][1], y0 = m_in[0][2], x1 = m_in[1][1], y1 = m_in[1][2], x2 = m_in[2][1], y2 = m_in[2][2];
#define FABS std::fabs
#define FMA std::fma
  // OpenBLAS' unblocked LU (lapack/getf2/getf2.c: what dgetrf runs for n <= DTB_ENTRIES / 2), left-looking, on the
  // column-major copy NumPy hands to LAPACK; only the SIGN of the determinant is used by the callers.
  //   column 0 = (1,1,1): pivot row 0, multipliers 1 * (1 / 1) = 1.
  //   column 1: b_i = x_i - 1 * x_0 (gemv, alpha = -1); pivot = first largest |b_i|; rows swapped in columns 0..1;
  //             multiplier l21 = b_2 * (1 / b_1)  — scaled by the RECIPROCAL of the pivot (dscal), two roundings.
  //   column 2: pivots applied; u12 = y_1 - 1 * y_0 (forward substitution, ddot of one element);
  //             u22 = y_2 - t with t = fma(l21, u12, fma(l20, y_0, 0)) — dgemv_n's scalar tail for one row accumulates
  //             temp += a * x (contracted to an fma by the compiler the library is built with), then y += alpha * temp.
  // Checked against numpy.linalg.det on 64 000 exactly / nearly collinear and general triples: same sign on all of them
  // (tests/test_oracle_numpy_semantics.py); the textbook right-looking order agrees on 98 % only.
  double b1 = x1 - x0, b2 = x2 - x0;  // (l10 = l20 = 1)
  double ya = y1, yb = y2;
  int sign = 1;
  if (!(FABS(b1) >= FABS(b2))) {  // idamax: first of the largest
    double t = b1;
    b1 = b2;
    b2 = t;
    ya = y2;
    yb = y1;
    sign = -1;
  }
  if (b1 == 0.0) return 0.0;  // singular (info > 0): numpy returns 0
  const double l21 = b2 * (1.0 / b1);
  const double u12 = ya - y0;
  const double t = FMA(l21, u12, y0);  // fma(l20 = 1, y0, 0) = y0 exactly
  const double u22 = yb - t;
  return (double)sign * b1 * u22;
#undef FABS
#undef FMA
}

}  // namespace fsdo
