// TEST INFRASTRUCTURE (oracle) — see np_compat.h header.
//
// Restatement of the smoothing-spline arithmetic the reference reaches through SciPy:
//   utils/spline_fit.py:117  splprep(trace.T, s=..., k=..., u=u_fit, per=False)
//   utils/spline_fit.py:61   splev(u_eval, tck, der=0)
// SciPy is a third-party dependency (unpinned in the reference's pyproject.toml:9 /
// requirements.txt:4; the build container holds scipy 1.15.3 as compiled FITPACK only).
// The algorithm restated here is P. Dierckx's published FITPACK: parcur -> fppara
// (knot placement fpknot, Givens QR fpgivs/fprota, back-substitution fpback, jump matrix
// fpdisc, rational root step fprati), B-spline basis fpbspl, evaluation splev.
// Pinned by tests against scipy.interpolate.splprep/splev outputs (tests/golden).
#pragma once
#include <vector>

namespace fsdo {

struct Spline {
  int k = 3;               // degree
  int n = 0;               // number of knots
  int ier = 0;             // FITPACK ier (0, -1, -2 ok; 1,2,3 warnings scipy still returns)
  double fp = 0;           // weighted sum of squared residuals
  unsigned branches = 0;   // which ways parcur_fit took (FitBranch bits; test coverage of the control flow, no effect on the fit)
  std::vector<double> t;   // knots (n)
  std::vector<double> cx;  // coefficients dim 0 (n-k-1 meaningful)
  std::vector<double> cy;  // coefficients dim 1
};

// The ways through fppara's control flow, one bit each (Spline::branches; tests/path_support.py family F)
enum FitBranch : unsigned {
  FB_POLYNOMIAL = 1u << 0,      // ier -2: the least-squares polynomial suffices
  FB_INTERPOLANT = 1u << 1,     // ier -1: n reached nmax, the interpolating spline
  FB_ACCEPT_AT_ONCE = 1u << 2,  // ier 0, |fp - s| < acc for a knot set of part 1 (n > nmin)
  FB_PART2 = 1u << 3,           // fp < s after knots were added: the root search of part 2 ran
  FB_RATIONAL = 1u << 4,        // ... and called fprati at least once
  FB_IER1 = 1u << 5,            // n reached nest
  FB_IER2 = 1u << 6,            // f2 outside (f3, f1)
  FB_IER3 = 1u << 7,            // MAXIT iterations
  FB_NPLUS_RATIO = 1u << 8,     // fpold - fp > acc: the increment from the ratio
  FB_NPLUS_DOUBLE = 1u << 9,    // ... not: twice the last increment
  FB_NPLUS_MIN = 1u << 10,      // min(nplus * 2, .) cut the ratio's value down
  FB_NPLUS_MAX = 1u << 11,      // max(., nplus / 2, 1) lifted it
  FB_ICH1 = 1u << 12,           // fprati bracket flags
  FB_ICH3 = 1u << 13,
  FB_NO_ICH = 1u << 14,         // part 2 ended with neither set
  FB_SINGLE_POINT = 1u << 15,   // fpknot split an interval that held a single point
  FB_KNOT_TIE = 1u << 16,       // fpknot met a second interval with the largest residual sum (the first one keeps it)
  FB_BITS = 17
};

// parcur with iopt=0, ipar=1, idim=2, w=1, ub=u[0], ue=u[m-1], nest=m+2k (what
// scipy.interpolate.splprep passes for task=0, _fitpack_impl.py:160-168).
// Returns false where scipy raises ValueError (ier=10: u not strictly increasing, ...).
bool parcur_fit(const double* u, const double* x, const double* y, int m, int k, double s, Spline& out);

// splev(der=0, ext=0) for both coordinates at one parameter value (sequential-search
// state `l` is carried by the caller exactly like FITPACK's loop over x(i)).
void splev_points(const Spline& sp, const double* u_eval, long n_eval, double* out_x, double* out_y);

}  // namespace fsdo
