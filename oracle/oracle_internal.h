// TEST INFRASTRUCTURE (oracle) — internal declarations shared by the oracle's translation units.
#pragma once
#include <cmath>
#include <vector>

#include "fsd_oracle.h"
#include "np_compat.h"
#include "fitpack.h"

namespace fsdo {

// The reference's configuration constants (fsd_path_planning/config.py:33-41,48,55-59,124-129); defaults = the factories'
// values.  One process-wide set (fsdo_set_params), read-only while frames are planned.
struct OParams {
  int max_n_neighbors = 5, max_length = 12;
  double max_dist = 6.5, max_dist_to_first = 6.0, threshold_directional_angle = 40 * (PI / 180.0),
         threshold_absolute_angle = 65 * (PI / 180.0);
  double min_track_width = 3.0, max_search_range = 5.0, max_search_angle = 50 * (PI / 180.0);
  double smoothing = 0.2, predict_every = 0.1, maximal_distance_for_valid_path = 5.0, mpc_path_length = 20.0;
  // config.py:48 max_deg, :58 mpc_prediction_horizon, :124-146 matches_should_be_monotonic (the pipeline's choice: False,
  // full_pipeline.py:65), :40 use_unknown_cones
  int max_deg = 3, horizon = 40, matches_should_be_monotonic = 0, use_unknown_cones = 1;
};
extern OParams g_prm;
struct Spline;
extern thread_local std::vector<Spline>* g_fit_capture;
void rebuild_default_previous_path();

struct Frame {
  std::vector<int> orig;  // index of every cone in the caller's array (cones of type UNKNOWN are dropped when use_unknown_cones is off)
  int n = 0;
  std::vector<double> x, y;
  std::vector<int> type;
  double px = 0, py = 0, dx = 1, dy = 0;
};

struct Config {
  int L = 12;            // target_length of the search that produced it
  int v[FSDO_MAX_LEN];   // -1 padded
};

struct SideResult {
  bool has = false;
  std::vector<Config> configs;  // sorted by cost
  std::vector<double> costs;
  int first_k[2] = {-1, -1};
};

typedef std::vector<Vec2> Pts;

// Decision margins of the sorting stage (diagnostics, tools/sort_margins.py): every discrete decision that hangs on a libm
// value — atan2 / acos compared with a threshold, or the arg-min over configuration costs that hold such values — records
// how far the value was from the threshold / the runner-up.  Off unless fsdo_margins_enable(1); single-threaded use.
enum MarginClass {
  MG_START_BEARING = 0,   // core_trace_sorter.py:379-407: bearing sign, pi/10, pi - pi/5
  MG_SECOND_SIDE = 1,     // end_configurations.py:260-278: sign of the bearing difference, 5 deg
  MG_ABS_ANGLE = 2,       // :172-205 |difference| vs threshold_absolute_angle
  MG_DIR_ANGLE = 3,       // :172-205 difference vs +-threshold_directional_angle
  MG_SIGN_FLIP = 4,       // :196-205 sign(difference) vs sign(difference_2), |difference - difference_2| vs 1.3
  MG_ACOS_THRESHOLDS = 5, // vec_angle_between vs 150 deg / 90 deg / search_angle / 2 / 40 deg (in the cosine: |cos - cos thr|)
  MG_WRONG_DIRECTION = 6, // cost_function.py:149-188 sign and 40 deg of the turn angles
  MG_COST_ARGMIN = 7,     // relative gap between the best and the second-best configuration cost
  MG_COMBINE = 8,         // combine_traces.py:150-257 angle signs / 5 deg
  // The thresholds that hold no libm value: the start ellipse and the (6, 3) ellipse of an edge (criterion vs 1), the nearest start
  // cone vs max_dist_to_first, the start pair vs 1.1 max_dist and 1.4, a listed neighbour's squared distance vs max_dist^2, dc / dl
  // vs 6 and the edge length vs 4 of the search, the squared distance vs 36 of the cost's nearby-cone search, dl / dr vs 3 of the
  // combination.  (The two ellipses rotate by an angle: sin / cos enter the criterion, which is still compared with a constant.)
  MG_ARITHMETIC = 9,
  // The path stage's decisions (path.cpp; tools/path_margins.py).  None holds a libm value; each is recorded relative to its
  // threshold (|value / threshold - 1|, or the absolute value where the threshold is 0).
  MG_PATH_TOO_FAR = 10,       // closest dense sample vs maximal_distance_for_valid_path
  MG_PATH_CONNECT_DIST = 11,  // first path point vs 0.5 m
  MG_PATH_CONNECT_ANGLE = 12, // its bearing vs 90 deg
  MG_PATH_FRONT_DOT = 13,     // dot(car -> point, direction) vs 0, every point of the path (absolute)
  MG_PATH_PLEN = 14,          // path length in front vs mpc_path_length
  MG_PATH_RADIUS = 15,        // fitted radius vs 10 / 80 / 100
  MG_PATH_TRIM_ARGMIN = 16,   // remove_path_behind_car: closest vs second closest distance
  MG_PATH_CUT = 17,           // cumulative length vs mpc_path_length at the cut and one sample before it
  MG_PATH_SKIP_FRAC = 18,     // distance of the skip quotient from the next integer (absolute)
  MG_PATH_DENSE_FRAC = 19,    // ... of max_u / predict_every of the parameterisation's samples
  MG_PATH_CURV_CLAMP = 20,    // window radius vs 1 and 3000
  MG_PATH_GLOBAL_30M = 21,    // global-path point vs 30 m
  MG_PATH_GLOBAL_ARGMIN = 22, // global path: closest vs second closest distance
  MG_CLASSES = 23
};
struct MarginRec {
  bool on = false;
  double min_margin[MG_CLASSES];
  long long n[MG_CLASSES], below_1e6[MG_CLASSES], below_1e9[MG_CLASSES], below_1e12[MG_CLASSES], zero[MG_CLASSES];
};
extern MarginRec g_margins;
static inline void margin(int cls, double value, double thr) {
  if (!g_margins.on) return;
  const double m = std::fabs(value - thr);
  if (!(m == m)) return;
  MarginRec& r = g_margins;
  r.n[cls]++;
  if (m == 0.0) {  // value == threshold exactly: equal operands (straight / lattice tracks), the same bits under any libm
    r.zero[cls]++;
    return;
  }
  if (m < r.min_margin[cls]) r.min_margin[cls] = m;
  if (m < 1e-6) r.below_1e6[cls]++;
  if (m < 1e-9) r.below_1e9[cls]++;
  if (m < 1e-12) r.below_1e12[cls]++;
}

static inline void margin_rel(int cls, double value, double thr) { margin(cls, value / thr, 1.0); }

// What the path stage decided on one frame, value by value (fsdo_path_full's optional record; tests/path_support.py proves with it
// that a pair of cases straddles the threshold it is named after).  NaN = the frame did not get there.  The MPC step's entries
// are those of its last run (the retry with the previous path, where there was one).
enum PathRecField {
  PR_N_CENTER = 0,     // points handed to fit #1 (before any fallback)
  PR_TOO_FAR,          // distance of the closest dense sample
  PR_CONNECT_DIST,     // distance of the first path point
  PR_CONNECT_ANGLE,    // its bearing
  PR_FIRST_FRONT,      // index of the first point in front of the car (-1: none), in the path after connect_path_to_car
  PR_FRONT_DOT,        // the dot product of smallest magnitude
  PR_N_IN_FRONT,       // points of mask_path_is_in_front_of_car
  PR_PLEN,             // path length in front
  PR_RADIUS,           // fitted radius before the clamps
  PR_ARC_SIGN,         // +1 / -1: the arc turns left / right
  PR_TRIM_INDEX,       // arg-min of remove_path_behind_car
  PR_TRIM_GAP,         // second smallest distance - smallest (0: a bit-equal tie)
  PR_N_REFIT,          // points handed to the refit
  PR_CUT_INDEX,        // first segment whose cumulative length exceeds mpc_path_length (= points kept)
  PR_CUT_OVER,         // that cumulative length
  PR_CUT_UNDER,        // the one before it
  PR_SKIP_QUOTIENT,    // predict_every / mean distance of _refit_spline
  PR_SKIP,
  PR_N_SKIPPED,        // points handed to fit #3
  PR_DENSE_QUOTIENT,   // max_u / predict_every of fit #3
  PR_N_DENSE,
  PR_WINDOW,           // curvature window
  PR_RADIUS_MIN,       // smallest / largest window radius before the clamps
  PR_RADIUS_MAX,
  PR_CURV_ZERO,        // windows whose determinant is exactly 0
  PR_GLOBAL_ARGMIN,    // global path: index of the closest point
  PR_GLOBAL_GAP,       // second smallest distance - smallest
  PR_GLOBAL_KEPT,      // points within 30 m
  PR_GLOBAL_30M,       // the distance closest to 30 m
  PR_FIT_BRANCHES,     // FitBranch masks of the frame's fits, in call order (up to 6)
  PR_FIT_IER = PR_FIT_BRANCHES + 6,
  PR_FIT_KNOTS = PR_FIT_IER + 6,  // ... their numbers of knots
  PR_N_FITS = PR_FIT_KNOTS + 6,
  PR_FIELDS
};
struct PathRec {
  double v[PR_FIELDS];
};
extern thread_local PathRec* g_path_rec;
static inline void prec(int field, double value) {
  if (g_path_rec) g_path_rec->v[field] = value;
}

// What a skidpad step decided (skidpad.cpp relocalize / skidpad_step), value by value; NaN: not reached.  Kept per planner,
// overwritten by every step, read through fsdo_skidpad_record.  A "margin" is the signed distance of a value to its
// threshold, positive on the accepting side; over many subsets / pairs the one of smallest magnitude is kept.
constexpr int SKR_MAX_SIZES = 16;
enum SkidRecField {
  SKR_ATTEMPT = 0,      // 1: the step attempted a relocalization
  SKR_SUCCESS,          // ... and it succeeded
  SKR_M,                // cones selected, min(n, 20)
  SKR_SELECT_GAP,       // distance of the 21st nearest cone - that of the 20th (n > 20)
  SKR_N_ACCEPTED,       // subsets accepted by circle_fit_powerset
  SKR_RADIUS_MARGIN,    // 1 - |radius - 7.625|
  SKR_SPACING_MARGIN,   // 1.5 - |mean nearest distance - 2.4|
  SKR_RESIDUAL_MARGIN,  // 0.4 - residual
  SKR_N_CENTERS,
  SKR_EPS_MARGIN,       // 3 - distance of a pair of centres
  SKR_N_CLUSTERS,
  SKR_CLUSTER_SIZE0,    // sizes of the first SKR_MAX_SIZES clusters, in label order
  SKR_BEST_DISTANCE = SKR_CLUSTER_SIZE0 + SKR_MAX_SIZES,  // |18.25 - d| of the chosen pair
  SKR_RUNNER_UP,        // the next smallest one (inf: one pair only)
  SKR_PAIR_A,           // labels of the chosen pair
  SKR_PAIR_B,
  SKR_SIDE0,            // v.y of the two centres in the latched car frame
  SKR_SIDE1,
  SKR_LO,               // window of the known path: [lo, hi)
  SKR_HI,
  SKR_ARGMIN,           // its closest point
  SKR_ARGMIN_GAP,       // second smallest distance - smallest (0: a bit-equal tie)
  SKR_N1,               // points of the path update
  SKR_MEDIAN_SPLIT0,    // per cluster (the first SKR_MAX_SIZES): 1 if the members that hold the x median (the middle one, or the
                        // middle two of an even size) are not the members that hold the y median, 0 if they are the same
  SKR_COUNT = SKR_MEDIAN_SPLIT0 + SKR_MAX_SIZES
};

// sorting.cpp
SideResult configs_for_one_side(const Frame& f, int cone_type);
void sort_frame(const Frame& f, std::vector<int>& left, std::vector<int>& right, SideResult* l = nullptr,
                SideResult* r = nullptr);
Vec2 search_direction(double x0, double y0, double x1, double y1, int cone_type);
bool segments_intersect(Vec2 a0, Vec2 a1, Vec2 b0, Vec2 b1);

// matching.cpp
void match_cones(const Pts& left, const Pts& right, Vec2 car_pos, Pts& left_v, Pts& right_v, std::vector<int>& l2r,
                 std::vector<int>& r2l);

// path.cpp
struct PathOut {
  double p[FSDO_PATH_POINTS][4];
  int fallback = 0;
};
const double (*default_previous_path())[4];
void calculate_path(const Pts& left_v, const Pts& right_v, const std::vector<int>& l2r, const std::vector<int>& r2l,
                    Vec2 pos, Vec2 dir, PathOut& out, const double (*prev)[4] = nullptr, const Pts* global_path = nullptr);

void finish_path(Pts path_update, const Pts& prev_xy, Vec2 pos, Vec2 dir, PathOut& out);
Pts almost_straight_path();
void circle_fit(const Pts& p, double& ocx, double& ocy, double& orad);
void do_all_mpc(const Pts& path_update, Vec2 pos, Vec2 dir, double out[][4], int* flags);
double m_atan2(double y, double x);
double m_cos(double a);
double m_sin(double a);

}  // namespace fsdo
