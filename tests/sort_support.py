"""Constructed inputs for the sorting stage (csrc/sort_kernel.h against oracle/sorting.cpp).  TEST INFRASTRUCTURE, modelled on
tests/match_support.py.

A case is (xyt (n, 3), pose (4,)).  The families are built without randomness (one seeded heading apart).  `as_batch` lays a
family out as ONE batch (off, cones, poses); the run_* functions hand it to a route in one launch; `run_oracle` calls
fsdo_sort_frame per case in det-math mode; `assert_equal` compares status, n_left, n_right, left_idx, right_idx, first_k_* and
n_configs_* with array_equal and best_cost_* within `cost_rtol` (0: bit for bit).

Offsets from a threshold
  REL = 1e-9 relative (match_support.REL: the device libm is pinned to 2 ulp, nine orders below).
  FAR = 1e-5 relative.
The kernels decide three kinds of predicate through a shortcut that falls back to the reference's own formulation inside a band:
the (6, 3) ellipse of an edge (band 1e-6 in the criterion, which is quadratic in the distance: an offset s moves it by 2 s) and
the arc cosines against 150 / 90 degrees (band 1e-9 in the cosine).  An angle offset of 1e-9 RELATIVE moves the cosine at 90 and
150 degrees by 1.6e-9 and 1.3e-9: outside the band.  The pairs at an arc-cosine threshold therefore offset the COSINE by s / 2
(`_acos_angle`): 5e-10 at REL (inside the band: the slow path decides), 5e-6 at FAR (outside: the cosine decides).

What cannot be observed with the default parameters (worked out from oracle/sorting.cpp, each checked on the oracle while this
file was written; no pair exists for them, the on-threshold cases below still run the code):
  * start ellipse on its MAJOR axis (9 m): the start cone must also lie within max_dist_to_first = 6 m; the ellipse boundary is
    within 6 m of the car only at bearings beyond 33.7 degrees.  Taken on the minor axis and at 50 degrees instead.
  * bearing sign of an UNKNOWN start cone at 0 and at pi: masked by |ang| > pi / 10 and |ang| < pi - pi / 5.
  * position 0, sign of the bearing difference at 0: masked by |diff| < 5 degrees; at pi the next edge would turn by more than
    threshold_absolute_angle.  The 5 degree threshold is taken.
  * edge ellipse on its MINOR axis: a candidate at 90 degrees to the edge fails threshold_absolute_angle (65 degrees) first.
    Taken at 60 and at 64 degrees.
  * same signs with |difference - difference_2| beyond 1.3: both turns are within 65 degrees, so same signs differ by at most
    1.13 rad.
  * the `under` count of the angle cost (interior angle below 40 degrees, a turn of more than 140): no configuration turns by more
    than 65 degrees.
  * wrong-direction turn sign at 0: masked by its own 40 degree threshold.
"""
from __future__ import annotations

import numpy as np

REL, FAR = 1e-9, 1e-5
UNKNOWN, RIGHT, LEFT = 0.0, 1.0, 2.0
POSE0 = np.array([0.0, 0.0, 1.0, 0.0])
DEG = np.pi / 180.0
MAX_DIST, MAX_DIST_TO_FIRST = 6.5, 6.0  # reference defaults (oracle_lib.PARAM_DEFAULTS)

INDEX_FIELDS = ("status", "n_left", "n_right", "left_idx", "right_idx", "first_k_left", "first_k_right", "n_configs_left", "n_configs_right")
PAD_SIZES = (64, 65, 128, 129, 255, 256, 300)


# ---------------------------------------------------------------------------------------------------------------------
# cases and their transformations
# ---------------------------------------------------------------------------------------------------------------------
def case(left=(), right=(), unknown=(), pose=POSE0):
    """cones in the order left..., right..., unknown..."""
    rows = [(x, y, t) for pts, t in ((left, LEFT), (right, RIGHT), (unknown, UNKNOWN)) for x, y in pts]
    return np.array(rows, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(pose, dtype=np.float64).reshape(4)


def typed(rows, pose=POSE0):
    """cones given as (x, y, type) in the caller's own order"""
    return np.array(rows, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(pose, dtype=np.float64).reshape(4)


def mirrored(c):
    """Reflected at the car's axis (the x axis of the canonical pose), LEFT <-> RIGHT."""
    xyt, p = c
    out = xyt * np.array([1.0, -1.0, 1.0])
    t = xyt[:, 2]
    out[:, 2] = np.where(t == LEFT, RIGHT, np.where(t == RIGHT, LEFT, t))
    return out, p * np.array([1.0, -1.0, 1.0, -1.0])


def mirrored_observable(obs):
    return obs.replace("left", "\0").replace("right", "left").replace("\0", "right")


def colourless(c):
    xyt, p = c
    out = xyt.copy()
    out[:, 2] = UNKNOWN
    return out, p


def moved(c, heading, shift=(0.0, 0.0)):
    """The case rigidly moved: rotated by `heading` about the origin, then shifted.  heading = pi is a negation (exact)."""
    xyt, p = c
    if heading == np.pi:
        cs, sn = -1.0, 0.0
    else:
        cs, sn = np.cos(heading), np.sin(heading)
    out = xyt.copy()
    out[:, 0] = cs * xyt[:, 0] - sn * xyt[:, 1] + shift[0]
    out[:, 1] = sn * xyt[:, 0] + cs * xyt[:, 1] + shift[1]
    q = np.array([cs * p[0] - sn * p[1] + shift[0], sn * p[0] + cs * p[1] + shift[1], cs * p[2] - sn * p[3], sn * p[2] + cs * p[3]])
    return out, q


HEADING_NEAR_PI = np.pi - 5e-4  # consecutive edges' atan2 values straddle the branch cut


def headings():
    """[(name, heading, shift)] of the two further poses of every pair: within 1e-3 of pi, and one seeded at random"""
    rng = np.random.default_rng(20240607)
    return [("near pi", HEADING_NEAR_PI, (0.0, 0.0)), ("seeded", float(rng.uniform(-np.pi, np.pi)), tuple(rng.uniform(-20.0, 20.0, 2)))]


def padded(c, n):
    """UNKNOWN filler cones on an 8 m grid 200 m from the car up to n cones: no neighbour within max_dist, none within 6 m of a
    configuration, outside the start ellipse."""
    xyt, p = c
    k = n - len(xyt)
    assert k >= 0
    i = np.arange(k)
    fill = np.column_stack([p[0] + 200.0 + 8.0 * (i % 16), p[1] + 200.0 + 8.0 * (i // 16), np.zeros(k)])
    return np.concatenate([xyt, fill]), p


# ---------------------------------------------------------------------------------------------------------------------
# geometry helpers
# ---------------------------------------------------------------------------------------------------------------------
L3 = [(1.0, 1.5), (5.5, 1.5), (10.0, 1.5)]
R3 = [(1.0, -1.5), (5.5, -1.5), (10.0, -1.5)]


def _polar(origin, r, a):
    return (origin[0] + r * np.cos(a), origin[1] + r * np.sin(a))


def _ellipse_radius(a, major, minor):
    return 1.0 / np.sqrt((np.cos(a) / major) ** 2 + (np.sin(a) / minor) ** 2)


def _acos_angle(thr, s):
    """the angle whose cosine is cos(thr) - s / 2 (to first order)"""
    return thr + 0.5 * s / np.sin(thr)


def _exact_edge(origin, length, a):
    """A point at direction `a` from `origin` whose distance from it is `length` EXACTLY as the stage computes it — sqrt(fma(dy, dy,
    dx * dx)) (norm_blas) and sqrt(dx * dx + dy * dy) alike: the y coordinate is moved by ulps until both round to `length`."""
    from fractions import Fraction

    x0, y0 = origin[0] + length * np.cos(a), origin[1] + length * np.sin(a)
    for i in range(64):
        x = x0
        for _ in range(i):
            x = np.nextafter(x, np.inf)
        dx = x - origin[0]
        y = y0
        for _ in range(64):
            y = np.nextafter(y, -np.inf)
        for _ in range(128):
            dy = y - origin[1]
            fused = float(Fraction(dy) * Fraction(dy) + Fraction(dx * dx)) ** 0.5
            if fused == length and (dx * dx + dy * dy) ** 0.5 == length:
                return (float(x), float(y))
            y = np.nextafter(y, np.inf)
    raise AssertionError("no exactly representable edge found")


def fourth(d, a, right=R3):
    """the issue's frame: three cones a side and a fourth left one at distance d, direction a from the third"""
    return case(L3 + [_polar(L3[2], d, a)], right)


def _two_sided(build, both):
    """[(suffix, below, above)] at REL and, for the shortcuts, at FAR"""
    return [(f" ({nm})", build(-s), build(+s)) for nm, s in ((("REL", REL), ("FAR", FAR)) if both else (("REL", REL),))]


# ---------------------------------------------------------------------------------------------------------------------
# threshold pairs
# ---------------------------------------------------------------------------------------------------------------------
MARGIN_CLASS = {}  # pair name -> class of oracle_lib.margins() whose minimum on the REL members is below MARGIN_BOUND
# (absolute margins: 1e-9 relative of an angle or a cosine is below 1e-8; of a squared distance of 42.25 it is 8.5e-8)
MARGIN_BOUND = {"arithmetic": 1e-7}
COLOUR_READING = set()  # names of the pairs that also get a colourless twin


def _search_pairs(eps_scale=1.0):
    P = []

    def add(name, obs, build, both=False, cls=None):
        for suffix, lo, hi in _two_sided(build, both):
            P.append((name + suffix, obs, lo, hi))
            if cls:
                MARGIN_CLASS[name + suffix] = cls

    add("directional angle", "left_idx", lambda s: fourth(4.005, 40 * DEG * (1 + s)), cls="dir_angle")
    add("absolute angle +", "left_idx", lambda s: fourth(3.0, 65 * DEG * (1 + s)), cls="abs_angle")
    add("absolute angle -", "left_idx", lambda s: fourth(3.0, -65 * DEG * (1 + s)), cls="abs_angle")
    add("edge ellipse, major axis", "left_idx", lambda s: fourth(6.0 * (1 + s), 0.0), both=True, cls="arithmetic")
    for deg in (60, 64, -35):
        add(f"edge ellipse at {deg} degrees", "left_idx", lambda s, a=deg * DEG: fourth(_ellipse_radius(a, 6, 3) * (1 + s), a), both=True, cls="arithmetic")
    add("edge length 4 beyond the directional angle", "left_idx", lambda s: fourth(4.0 * (1 + s), 40.05 * DEG), cls="arithmetic")

    # "between" (position 0: no ellipse).  A = start, nb a near neighbour, the candidate seen from nb at `ang` to A.
    def between(dl, dc, ang, tail):
        a = (1.0, 1.5)
        nb = _polar(a, dl, 20 * DEG) if dl > 1 else (a[0] + dl, a[1])
        back = np.arctan2(a[1] - nb[1], a[0] - nb[0])
        cand = _polar(nb, dc, back - ang)
        return case([a, nb, cand, _polar(cand, 3.0, tail * DEG)], R3)

    add("between, dc at 6", "n_configs_left", lambda s: between(0.5, 6.0 * (1 + s), 160 * DEG, 20), cls="arithmetic")
    add("between, dl at 6", "n_configs_left", lambda s: between(6.0 * (1 + s), 0.5, 160 * DEG, 25), cls="arithmetic")
    add("between, 150 degrees", "n_configs_left", lambda s: between(0.5, 5.5, _acos_angle(150 * DEG, s), 30), both=True, cls="acos_thresholds")

    # position 0: the second cone 5 degrees to the wrong side of the car's axis
    def second_side(s):
        b = _polar((0.0, 0.0), 5.5, -5 * DEG * (1 + s))
        return case([(1.0, 1.5), b, (10.0, b[1])], R3[:1] + [(5.5, -3.0), (10.0, -3.0)])

    add("position 0, 5 degrees", "left_idx", second_side, cls="second_side")

    # position >= 2: opposite signs, |difference - difference_2| at 1.3
    def sign_flip(s):
        t2 = 37 * DEG
        c = _polar(L3[1], 3.5, t2)
        d = _polar(c, 3.5, t2 - (1.3 * (1 + s) - t2))
        return case([L3[0], L3[1], c, d], R3)

    add("sign flip, 1.3 rad", "left_idx", sign_flip, cls="sign_flip")

    # position 1: the candidate at 90 degrees to the car's direction, seen from the start cone
    def ninety(s):
        a = (1.0, 1.5)
        return case([a, (2.5, 4.0), _polar(a, 5.3, _acos_angle(90 * DEG, s))], R3)

    add("position 1, 90 degrees", "left_idx", ninety, both=True, cls="acos_thresholds")

    # the car's segment [p - 1.05 n, p + 2.1 n]: the intersection test admits 1e-6 beyond either end — in the world's x and in
    # its y (line_segment_intersection.py compares with the segments' bounding boxes), i.e. 1e-6 / max(|cos h|, |sin h|) along a
    # car heading h: eps_scale, which posed_pairs() sets for the heading it moves the pair to
    eps = 1e-6 * eps_scale
    def car_front(s):
        b, x = (0.0, 2.0), (2.1 + eps + 2.1 * s, 0.0)
        return case([(-3.0, 3.0), b, (b[0] + 1.3 * (x[0] - b[0]), b[1] + 1.3 * (x[1] - b[1]))], [(3.0, -3.0), (7.0, -3.0), (11.0, -3.0)])

    def car_rear(s):
        # (position 0: a LEFT start cone below the axis, the edge to the second cone passes behind the car)
        b, x = (-1.6, -0.6), (-1.05 - eps - 1.05 * s, 0.0)
        c = (b[0] + 7.7 * (x[0] - b[0]), b[1] + 7.7 * (x[1] - b[1]))
        return case([b, c, (c[0] + 2.9, c[1] + 1.5)], [(3.0, -3.0), (7.0, -3.0), (11.0, -3.0)])

    add("car segment, front end", "left_idx", car_front)
    add("car segment, rear end", "left_idx", car_rear)
    return P


def _start_pairs():
    P = []

    def add(name, obs, build, both=False, cls=None, colour=True):
        for suffix, lo, hi in _two_sided(build, both):
            P.append((name + suffix, obs, lo, hi))
            if cls:
                MARGIN_CLASS[name + suffix] = cls
            if colour:
                COLOUR_READING.add(name + suffix)

    def with_start(s_pt, s_type, chain, right=R3):
        return typed([(*s_pt, s_type)] + [(x, y, LEFT) for x, y in chain] + [(x, y, RIGHT) for x, y in right])

    for nm, t in (("coloured", LEFT), ("UNKNOWN", UNKNOWN)):
        add(f"start ellipse, minor axis, {nm}", "first_k_left", lambda s, t=t: with_start((0.0, 4.0 * (1 + s)), t, [(3.5, 4.5), (7.0, 4.5), (10.5, 4.5)]),
            cls="arithmetic", colour=False)
        r50 = _ellipse_radius(50 * DEG, 9.0, 4.0)
        add(f"start ellipse at 50 degrees, {nm}", "first_k_left",
            lambda s, t=t: with_start(_polar((0, 0), r50 * (1 + s), 50 * DEG), t, [(6.5, 4.5), (10.0, 4.5), (13.5, 4.5)]), cls="arithmetic", colour=False)
    add("start bearing, pi / 10", "first_k_left", lambda s: with_start(_polar((0, 0), 3.0, np.pi / 10 * (1 + s)), UNKNOWN, [(6.5, 1.5), (10.0, 1.5), (13.5, 1.5)]),
        cls="start_bearing", colour=False)
    add("start bearing, pi - pi / 5", "first_k_left",
        lambda s: with_start(_polar((0, 0), 3.0, (np.pi - np.pi / 5) * (1 + s)), UNKNOWN, [(1.5, 2.0), (5.5, 2.0), (9.5, 2.0)]), cls="start_bearing", colour=False)
    add("first start cone at max_dist_to_first", "first_k_left",
        lambda s: with_start(_polar((0, 0), MAX_DIST_TO_FIRST * (1 + s), 25 * DEG), LEFT, [(9.5, 2.5), (13.0, 2.5), (16.5, 2.5)]), cls="arithmetic")
    near = [(0.5, 1.5), (5.0, 1.5), (9.5, 1.5)]  # (the first start cone within max_dist of the second: the second is where the search starts)
    add("second start cone at max_dist_to_first", "first_k_left",
        lambda s: with_start(_polar((0, 0), MAX_DIST_TO_FIRST * (1 + s), 155 * DEG), LEFT, near), cls="arithmetic", colour=False)
    # (no colourless twins of this pair and of the one at 1.1 max_dist: an UNKNOWN second start cone has a bearing between 90 and 144
    # degrees, where the start ellipse ends 4.9 m from the car and less)
    add("second start cone abeam", "first_k_left", lambda s: with_start(_polar((0, 0), 3.0, _acos_angle(90 * DEG, s)), LEFT, L3), both=True)
    add("start pair, swap", "first_k_left", lambda s: with_start((-1.0 + 2.0 * s, 3.5), LEFT, [(-1.0, 1.5), (3.0, 1.5), (7.0, 1.5)]))
    # (a start pair between max_dist and 1.1 max_dist apart is no edge: an UNKNOWN cone behind the car — no start cone at a bearing
    # beyond pi - pi / 5 — links the two, else the search starts at a cone that reaches nothing and the reference raises: structural())
    add("start pair at 1.1 max_dist", "first_k_left",
        lambda s: typed(with_start(_polar(L3[0], 1.1 * MAX_DIST * (1 + s), 200 * DEG), LEFT, L3)[0].tolist() + [(-3.0, 0.3, UNKNOWN)]), cls="arithmetic", colour=False)
    add("start pair at 1.4", "first_k_left",
        lambda s: with_start(_polar((-0.2, 1.5), 1.4 * (1 + s), 170 * DEG), LEFT, [(-0.2, 1.5), (3.5, 1.5), (7.5, 1.5)]), cls="arithmetic")
    return P


def kth_neighbour(k, s, contested_first, opposite_colour=False):
    """A hub C with the start cone and k - 1 clutter cones nearer than 4 m, the chain's next cone F at 4 m and a contested cone G
    at 4 (1 + s) m: C lists F among its k nearest only if G is farther (F always lists C: the pair with and without the mutual
    edge).  contested_first: G's index below F's.  opposite_colour: one clutter cone RIGHT — it takes no slot, F is listed."""
    hub, start, f, h = (5.0, 1.5), (1.5, 1.5), (9.0, 1.5), (13.0, 1.5)
    g = _polar(hub, 4.0 * (1 + s), 100 * DEG)
    clutter = [_polar(hub, 2.4, a * DEG) for a in np.linspace(76, 104, k - 2)]
    rows = [(*start, LEFT), (*hub, LEFT)]
    rows += [(*g, UNKNOWN), (*f, LEFT)] if contested_first else [(*f, LEFT), (*g, UNKNOWN)]
    rows += [(*h, LEFT)] + [(*c, RIGHT if opposite_colour and i == 0 else UNKNOWN) for i, c in enumerate(clutter)]
    return typed(rows)


def _adjacency_pairs(k):
    P = []
    nm = "neighbour at max_dist (REL)"
    P.append((nm, "left_idx", *[case([(1.0, 1.5), (1.0 + MAX_DIST * (1 + s), 1.5), (5.0 + MAX_DIST * (1 + s), 1.5), (8.5 + MAX_DIST * (1 + s), 1.5)], R3) for s in (-REL, REL)]))
    MARGIN_CLASS[nm] = "arithmetic"
    COLOUR_READING.add(nm)
    for first in (True, False):
        nm = f"k-th neighbour, k = {k}, contested cone {'first' if first else 'last'} (REL)"
        P.append((nm, "n_configs_left", kth_neighbour(k, -REL, first), kth_neighbour(k, REL, first)))
    return P


def _cost_pairs():
    """Cost-only predicates: observed in best_cost_left, which jumps (by far more than the 1e-9 a smooth term moves)."""
    P = []

    def add(name, build, both=False, cls=None):
        for suffix, lo, hi in _two_sided(build, both):
            P.append((name + suffix, "best_cost_left", lo, hi))
            if cls:
                MARGIN_CLASS[name + suffix] = cls

    # a RIGHT cone (no neighbour of the left side) at 6 m from the last cone only, in its search direction
    add("nearby cone at 6 m", lambda s: case(L3, [(10.0, 1.5 - 6.0 * (1 + s))]), cls="arithmetic")
    # ... at 3 m from the middle cone, 60 degrees from its search direction (0, -1) and from the negated one
    add("good cone at 60 degrees", lambda s: case(L3, [_polar(L3[1], 3.0, -90 * DEG + _acos_angle(60 * DEG, s))]), both=True, cls="acos_thresholds")
    # (with one configuration a negative good - bad count costs what 0 costs: a good cone straight in the search direction as well)
    add("bad cone at 60 degrees", lambda s: case(L3, [_polar(L3[1], 3.0, 90 * DEG + _acos_angle(60 * DEG, s)), (5.5, -1.5)]), both=True, cls="acos_thresholds")

    # wrong direction: a left side of four cones turning right by 40 degrees
    def wrong(s):
        c = _polar(L3[1], 3.5, -40 * DEG * (1 + s))
        return case([L3[0], L3[1], c, _polar(c, 3.5, -40 * DEG * (1 + s))], [(1.0, -3.0), (4.0, -4.5), (5.5, -7.5)])

    add("wrong direction, 40 degrees", wrong, cls="wrong_direction")
    return P


def _combine_frame(dl, dr_extra=0.05, tilt=0.0, left_tail=True, right_tail=True, right_more=0):
    """Both sides run into one UNKNOWN cone U: dl from the left side's third cone; the right side's third cone is dr_extra
    farther.  Behind U a LEFT and a RIGHT cone, so that U is interior to both winners."""
    l2 = (10.0, 1.5)
    u = _polar(l2, dl, -30 * DEG)
    r2 = (10.0 - 2.0 * dr_extra, -1.5)
    left = L3 + ([_polar(u, 3.85, (3 + tilt) * DEG)] if left_tail else [])  # (beyond max_dist of the third cones: only through U)
    right = [(1.0, r2[1]), (5.5, r2[1]), r2] + ([_polar(u, 3.85, -3 * DEG)] if right_tail else [])
    right += [_polar(right[-1], 3.5 * (i + 1), -3 * DEG) for i in range(right_more)]  # (the right side longer: |nl - nr|)
    return case(left, right, [u])


def _combine_turns(c):
    """(|al|, |ar|) of combine_traces.py:260-275 at the shared cone of a _combine_frame with both tails: cones 0-3 left, 4-7 right, 8 U"""
    xy = c[0][:, :2]

    def turn(p, nx):
        a_next = np.arctan2(xy[nx, 1] - xy[8, 1], xy[nx, 0] - xy[8, 0])
        a_prev = np.arctan2(xy[p, 1] - xy[8, 1], xy[p, 0] - xy[8, 0])
        return abs((a_next - a_prev + 3 * np.pi) % (2 * np.pi) - np.pi)

    return turn(2, 3), turn(6, 7)


def _tilt_for_turn_gap(gap):
    """the left tail's tilt at which ||al| - |ar|| of _combine_frame(3.2, tilt) is `gap` (bisection: the gap grows with the tilt)"""
    f = lambda t: abs(np.subtract(*_combine_turns(_combine_frame(3.2, tilt=t)))) - gap
    lo, hi = 0.0, 5.0
    assert f(lo) < 0 < f(hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) < 0 else (lo, mid)
    return 0.5 * (lo + hi)


def _combine_pairs():
    P = [("combine, dl at 3 (REL)", "left_idx", _combine_frame(3.0 * (1 - REL)), _combine_frame(3.0 * (1 + REL)))]
    MARGIN_CLASS[P[0][0]] = "arithmetic"
    # opposite turn signs, equal lengths: the side that turns more by over 5 degrees is cut at the shared cone, else both are
    P.append(("combine, turn angles 5 degrees apart (REL)", "right_idx",
              *[_combine_frame(3.2, tilt=_tilt_for_turn_gap(5 * DEG * (1 + s))) for s in (-REL, REL)]))
    return P


def threshold_pairs(k=5, eps_scale=1.0):
    """[(name, observable, below, above)]: a cone on either side of every threshold the sorting stage decides with, at REL and, for
    the kernels' shortcuts, at FAR.  `observable` is the field of the record that differs between the two members (best_cost_*:
    by more than 1e-6 relative).  k = max_n_neighbors of the build (the k-th neighbour pairs)."""
    return _search_pairs(eps_scale) + _start_pairs() + _adjacency_pairs(k) + _cost_pairs() + _combine_pairs()


def all_pairs(k=5, eps_scale=1.0):
    """threshold_pairs with the mirrored twin of every pair and the colourless twin of those that read cone colour"""
    out = []
    for name, obs, lo, hi in threshold_pairs(k, eps_scale):
        out.append((name, obs, lo, hi))
        out.append((name + ", mirrored", mirrored_observable(obs), mirrored(lo), mirrored(hi)))
        if name in COLOUR_READING:
            out.append((name + ", colourless", obs, colourless(lo), colourless(hi)))
    return out


def posed_pairs(k=5):
    """all_pairs at the canonical pose and rigidly moved to the two further headings"""
    out = list(all_pairs(k))
    for hname, heading, shift in headings():
        scale = 1.0 / max(abs(np.cos(heading)), abs(np.sin(heading)))
        out += [(f"{name} [{hname}]", obs, moved(lo, heading, shift), moved(hi, heading, shift)) for name, obs, lo, hi in all_pairs(k, scale)]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# on-threshold cases: the quantity equals its threshold exactly in binary64 (half-metre, axis-aligned coordinates)
# ---------------------------------------------------------------------------------------------------------------------
def on_threshold():
    """[(name, case)] — where `<` and `<=` differ"""
    out = [
        ("squared neighbour distance 42.25", case([(1.0, 1.5), (7.5, 1.5), (11.5, 1.5)], R3)),
        ("edge length 4.0", case(L3 + [(10.0 + 4.0 * 0.75, 1.5 + 4.0 * 0.0)], R3)),  # (replaced below: see edge_len)
        ("ellipse criterion 36 / 36 + 0", fourth(6.0, 0.0)),
        ("start ellipse 81 / 81 + 0", case([(9.0, 0.0), (12.5, 0.0), (16.0, 0.0)], R3)),
        ("start ellipse 16 / 16 + 0", case([(0.0, 4.0), (3.5, 4.5), (7.0, 4.5), (10.5, 4.5)], R3)),
        ("start distance 6.0", case([(6.0, 0.0), (9.5, 0.0), (13.0, 0.0)], [(1.0, -3.0), (5.0, -3.0), (9.0, -3.0)])),
        ("start pair 1.4", case([(0.0, 1.5), (-1.4, 1.5), (3.5, 1.5), (7.5, 1.5)], R3)),
        ("bearing exactly 0", case(L3, R3, [(3.0, 0.0)])),
        ("bearing exactly pi", case(L3, R3, [(-3.0, 0.0)])),
        ("bearing exactly -pi", case(L3, R3, [(-3.0, -0.0)])),
        ("second start cone exactly abeam", case([(0.0, 3.0)] + L3, R3)),
        # position 1 at 90 degrees: the candidate one ulp ahead of abeam of the start cone — its cosine is positive, its arc
        # cosine rounds to pi / 2 (not below it)
        ("position 1, one ulp inside 90 degrees", case([(1.0, 1.5), (2.5, 4.0), (np.nextafter(1.0, 2.0), 6.8)], R3)),
    ]
    # edge length exactly 4.0 at a turn beyond the directional threshold.  The (6, 3) ellipse admits a 4 m edge only up to 40.2
    # degrees, which no half-metre coordinates reach: the fourth cone's y is chosen by ulps so that the length rounds to 4.0
    out[1] = ("edge length 4.0", case(L3 + [_exact_edge(L3[2], 4.0, 40.1 * DEG)], R3))
    # dc = 6.0 exactly: nb half a metre from the start cone, the candidate 6 m from nb on a 3-4-5 direction (angle 143: not between;
    # the case pins dc < 6.0 against <= only where the angle passes — so a second one nearly straight behind)
    out.append(("between, dc = 6.0", case([(1.0, 1.5), (1.5, 1.5), (7.5, 1.5), (11.0, 1.5)], R3)))
    out.append(("between, dl = 6.0", case([(1.0, 1.5), (7.0, 1.5), (7.5, 1.5), (11.0, 1.5)], R3)))
    # the combination: the shared cone exactly 3.0 from the left side's cone before it
    # (dl < 3.0 fails, dr = 3.6: the turn angles decide — the right side runs straight through the shared cone, the left side turns by
    # 30 degrees there and is cut; with dl counted as within 3 the right side would be cut instead)
    out.append(("combine distance 3.0", typed([(1.0, 1.5, LEFT), (5.5, 1.5, LEFT), (10.0, 1.5, LEFT), (13.0, 1.5, UNKNOWN), (*_polar((13.0, 1.5), 4.4, 30 * DEG), LEFT),
                                               (2.5, -1.5, RIGHT), (6.0, -0.5, RIGHT), (9.5, 0.5, RIGHT), (16.5, 2.5, RIGHT)])))
    # exact ties: lowest index first (include/fsdp.h), in both index orders
    for first in (True, False):
        tie = kth_neighbour(5, 0.0, first)
        g = 2 if first else 3
        tie[0][g, :2] = (5.0, 5.5)  # 4.0 above the hub: the squared distance is 16 exactly, like F's
        out.append((f"k-th neighbour tie, contested cone {'first' if first else 'last'}", tie))
    for order in ((0, 1), (1, 0)):
        pts = [(1.5, 2.0), (1.5, -2.0)]  # two LEFT cones ahead, the same distance to the car: the lower index starts
        rows = [(*pts[order[0]], LEFT), (*pts[order[1]], LEFT), (5.0, 2.0, LEFT), (8.5, 2.0, LEFT), (5.0, -2.0, LEFT), (8.5, -2.0, LEFT)]
        out.append((f"start distance tie, order {order}", typed(rows)))
    return out


def on_threshold_posed():
    """on_threshold, their mirrored twins, and both at the heading pi (a negation: still exact)"""
    base = on_threshold()
    out = base + [(n + ", mirrored", mirrored(c)) for n, c in base]
    return out + [(n + " [pi]", moved(c, np.pi)) for n, c in out]


# ---------------------------------------------------------------------------------------------------------------------
# structural families (no offset)
# ---------------------------------------------------------------------------------------------------------------------
def chain(n, y, t, spacing=3.0, x0=1.0):
    return [(x0 + spacing * i, y, t) for i in range(n)]


def structural(max_len=12):
    """[(name, case)]"""
    out = []
    # frames of 3 .. 7 cones: n_neighbors = min(max_n_neighbors, n - 1)
    for n in (3, 4, 5, 6, 7):
        nl = (n + 1) // 2 if n > 3 else 3
        out.append((f"{n} cones", typed(chain(nl, 1.5, LEFT) + chain(n - nl, -1.5, RIGHT))))
        out.append((f"{n} cones, colourless", colourless(typed(chain(nl, 1.5, LEFT) + chain(n - nl, -1.5, RIGHT)))))
    # target_length = min(n_reach, max_length)
    for n in range(max_len - 1, max_len + 3):
        out.append((f"straight chains of {n}", typed(chain(n, 1.5, LEFT) + chain(n, -1.5, RIGHT))))
        out.append((f"straight chains of {n}, colourless", colourless(typed(chain(n, 1.5, LEFT) + chain(n, -1.5, RIGHT)))))
    # post-filters
    out.append(("every end shorter than 3", typed(chain(2, 1.5, LEFT) + chain(4, -1.5, RIGHT))))
    out.append(("last cone UNKNOWN, dropped to 2", typed(chain(2, 1.5, LEFT) + [(7.0, 1.5, UNKNOWN)] + chain(4, -1.5, RIGHT))))
    out.append(("last cone UNKNOWN, dropped to 3", typed(chain(3, 1.5, LEFT) + [(10.0, 1.5, UNKNOWN)] + chain(4, -1.5, RIGHT))))
    out.append(("last cone of the other colour", typed(chain(3, 1.5, LEFT) + [(10.0, 1.5, RIGHT)] + chain(4, -1.5, RIGHT))))
    out.append(("a fork: ends that share a prefix", typed(chain(3, 1.5, LEFT) + [(9.8, 2.5, LEFT), (9.8, 0.6, LEFT), (12.6, 3.4, LEFT)] + chain(4, -1.5, RIGHT))))
    out.append(("a prefix of another end after the colour drop", typed(chain(3, 1.5, LEFT) + [(10.0, 1.5, UNKNOWN), (13.0, 1.5, UNKNOWN)] + chain(4, -1.5, RIGHT))))
    out.append(("first_k filter", typed([(-2.0, 1.5, LEFT)] + chain(4, 1.5, LEFT) + [(-2.0, -1.5, RIGHT)] + chain(4, -1.5, RIGHT))))
    out.append(("opposite colour among the k nearest", kth_neighbour(5, -REL, True, opposite_colour=True)))
    out.append(("start pair beyond max_dist, the first reaches nothing", typed([(*_polar(L3[0], 7.0, 200 * DEG), LEFT)] + [(x, y, LEFT) for x, y in L3]
                                                                             + [(x, y, RIGHT) for x, y in R3])))
    out.append(("car segment crossed", case([(-3.0, 3.0), (0.0, 2.0), (1.5, -0.8)], [(3.0, -3.0), (7.0, -3.0), (11.0, -3.0)])))
    # cost: len == 3 against 4 with a right turn beyond 40 degrees on the left side
    c = _polar(L3[1], 3.5, -50 * DEG)
    out.append(("wrong direction, three cones", case([L3[0], L3[1], c], [(1.0, -3.0), (4.0, -4.5), (5.5, -7.5)])))
    out.append(("wrong direction, four cones", case([L3[0], L3[1], c, _polar(c, 3.5, -50 * DEG)], [(1.0, -3.0), (4.0, -4.5), (5.5, -7.5)])))
    # combining the sides
    out.append(("combine: both within 3", _combine_frame(2.9, dr_extra=0.0)))
    out.append(("combine: neither within 3, opposite signs", _combine_frame(3.2)))
    out.append(("combine: turn angles 5 degrees apart", _combine_frame(3.2, tilt=12.0)))
    out.append(("combine: lengths 2 apart", _combine_frame(3.2, right_more=2)))
    out.append(("combine: lengths 3 apart", _combine_frame(3.2, right_more=3)))
    out.append(("combine: shared cone last on the left", _combine_frame(3.2, left_tail=False)))
    out.append(("combine: shared cone last on the right", _combine_frame(3.2, right_tail=False)))
    out.append(("combine: shared cone last on both", _combine_frame(3.2, left_tail=False, right_tail=False)))
    out.append(("combine: colourless, lengths apart", colourless(typed(chain(7, 1.5, LEFT) + chain(3, -1.5, RIGHT) + [(9.5, 0.0, UNKNOWN)]))))
    return out + [(n + ", mirrored", mirrored(c)) for n, c in out]


def padded_family(k=5, max_len=12):
    """[(name, unpadded case, padded case)]: every pair member of 7 or more cones, on-threshold and structural case of 7 or more
    cones, each at one size of PAD_SIZES (taken in turn, so every size occurs many times)"""
    base = []
    for name, _obs, lo, hi in all_pairs(k):
        base += [(name + " below", lo), (name + " above", hi)]
    base += on_threshold() + structural(max_len)
    out, i = [], 0
    for name, c in base:
        if len(c[0]) < 7:
            continue
        n = PAD_SIZES[i % len(PAD_SIZES)]
        i += 1
        out.append((f"{name} padded to {n}", c, padded(c, n)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# adapters and comparison
# ---------------------------------------------------------------------------------------------------------------------
def as_batch(cases):
    """-> (off (F + 1,) i4, cones (total, 3), poses (F, 4))"""
    off = np.concatenate([[0], np.cumsum([len(x) for x, _p in cases])]).astype(np.int32)
    return off, np.concatenate([x for x, _p in cases]).reshape(-1, 3), np.array([p for _x, p in cases]).reshape(-1, 4)


def run_oracle(oracle, cases, require_ok=True):
    """fsdo_sort_frame per case in det-math mode (as every kernel-against-oracle comparison of the suite)"""
    out = np.zeros(len(cases), oracle.RESULT_DTYPE)
    with oracle.math_mode(1):
        for f, (xyt, p) in enumerate(cases):
            out[f] = oracle.sort_frame(xyt, p)
    if require_ok:
        assert (out["status"] == 0).all(), np.flatnonzero(out["status"] != 0)[:8]
    return out


def run_emu(emu, cases):
    return emu.sort(*as_batch(cases))


def run_emu_ranked(emu, cases, top_k=64):
    return emu.sort_ranked(*as_batch(cases), top_k=top_k, terms=True)


def run_emu_cached(emu, cases):
    """the cache-enabled kernels (sort_kernel*_cached), one planner per case with an empty entry: no side can hit, that
    instantiation's own copies of the stage's functions search"""
    out, hits = emu.sort_cached(*as_batch(cases))
    assert not (hits == 1).any()
    return out


def run_emu_speculative(emu, cases):
    """the speculative instantiation of fsdp_plan_sequence_cached: one planner per case, a single step"""
    off, cones, poses = as_batch(cases)
    out, hits, _resorted, _kernels, _big = emu.sequence_cache(len(cases), off, cones, poses)
    assert not (hits == 1).any()
    return out


def observable_differs(a, b, obs):
    if obs.startswith("best_cost"):
        return abs(float(a[obs]) - float(b[obs])) > 1e-6 * max(abs(float(a[obs])), abs(float(b[obs])))
    side = obs.rsplit("_", 1)[-1] if obs.endswith(("left", "right")) else None
    if obs.startswith(("left_idx", "right_idx")):
        s = obs.split("_")[0]
        return int(a[f"n_{s}"]) != int(b[f"n_{s}"]) or not np.array_equal(a[obs], b[obs])
    assert side is not None, obs
    return not np.array_equal(a[obs], b[obs])


def assert_equal(got, ref, what="", cost_rtol=0.0, names=None):
    """Index fields with array_equal; best_cost_* where the side has configurations: bit for bit at cost_rtol = 0 (NaN equals NaN),
    else within cost_rtol * max(1, |ref|) (tests/parity.py assert_intermediates_equal)."""
    assert len(got) == len(ref)
    ok = ref["status"] == 0  # (a frame on which the reference raises has its status alone, as in tests/parity.py)
    for k in INDEX_FIELDS:
        if np.array_equal(got[k], ref[k]) if k == "status" else np.array_equal(got[k][ok], ref[k][ok]):
            continue
        bad = [f for f in range(len(ref)) if (ok[f] or k == "status") and not np.array_equal(got[k][f], ref[k][f])]
        label = "" if names is None else f" ({names[bad[0]]})"
        raise AssertionError(f"{what}: {k} differs on {len(bad)} of {len(ref)} cases, first {bad[:8]}{label}: got {got[k][bad[0]]!r} want {ref[k][bad[0]]!r}")
    for side in ("left", "right"):
        has = (ref["status"] == 0) & (ref[f"n_configs_{side}"] > 0)
        a, b = got[f"best_cost_{side}"][has], ref[f"best_cost_{side}"][has]
        if cost_rtol == 0.0:
            ok = (a == b) | (np.isnan(a) & np.isnan(b))
        else:
            ok = (np.abs(a - b) <= cost_rtol * np.maximum(1.0, np.abs(b))) | (np.isnan(a) & np.isnan(b))
        if not ok.all():
            f = int(np.flatnonzero(has)[np.flatnonzero(~ok)[0]])
            raise AssertionError(f"{what}: best_cost_{side} differs on {int((~ok).sum())} cases, first {f}: got {got[f'best_cost_{side}'][f]!r} "
                                 f"want {ref[f'best_cost_{side}'][f]!r}")


def records_equal_but_for_padding(padded_rec, plain_rec):
    """every field of the sort record equal (best_cost_* bit for bit)"""
    for k in INDEX_FIELDS + ("best_cost_left", "best_cost_right"):
        if not np.array_equal(padded_rec[k], plain_rec[k], equal_nan=True):
            return k
    return None
