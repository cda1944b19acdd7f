"""TEST INFRASTRUCTURE of tests/test_path_constructed_{cpu,gpu}.py: inputs built for the path stage (csrc/path_kernel.h,
spline_device.h) — one case at every branch, pairs of cases either side of every threshold — with what the oracle says about them.

The stage's entry points take everything that matters as free inputs: the match record, the pose, the previous path and the
global path.  Three of them give exact control of the polyline that enters fit #1:

  identity matches   left_v == right_v == P, l2r == r2l == arange: the centres are exactly P ((a + a) / 2 == a), <= MAX_MATCH points
  a previous path    its PATH_POINTS rows, when both sides are shorter than 3 (path_fallback bit 1)
  a global path      a table of up to 1408 points

The pose enters only after fit #1 (too far, connect, extend, remove behind), so a pose threshold is placed by moving the car
until the oracle's own record of the decision value (oracle_lib.path(record=True): oracle_internal.h PathRec) reads
threshold (1 -+ 1e-9): `solve` below.  Thresholds on a quantity that went through a smoothing fit (fitted radius, plen, the cut)
are placed the same way, by the scale of the scene.  Every pair is then proved on the oracle: `Pair.check`.

Every family is built in a canonical frame (car near the origin, looking along +x) and then moved: its mirrored twin (y -> -y,
sides swapped), three poses (canonical, heading within 1e-3 of pi, a seeded rigid motion), and for a subset a copy translated
by (5e5, 5e6) m.  Thresholds are solved AFTER the motion, in the moved frame, so a pair straddles there as well.

path_fallback: bit 8 (the MPC step raises on the update and is retried with the previous path) is reached twice over: by a path
update of two dense samples 0.1 m apart whose arc extension, at a heading next to pi, leaves the refit a parameter that does not
increase (C/short/2, status 0, fallback 8 | 16: it goes to the GPU), and by tracks at 1e17 m, where consecutive dense samples round
to the same point (B/far_track: emulator only).  Bit 2 is reached by coincident, NaN and infinite centres.

What cannot be produced, with the reason (tests/test_path_constructed_cpu.py::test_coverage_of_the_stage asserts on the oracle's records
that these stay unreached, so a change that makes one reachable shows up):
  * fallback 4 | 16, 4 | 32 and 1 | 16 on a fresh planner's default previous path with the car near it: that path is 62.8 m long, so more
    than 20 m of it lie in front of any car that is not past its end.  They are built with a caller's previous path instead.
  * parcur_fit ier 1: nest = m + 2 k >= nmax = m + k + 1 for k >= 1, so n reaches nmax first.
  * parcur_fit ier -1: at n = nmax the spline interpolates, fp = 0 < s, and fp - s < 0 is tested before n == nmax: the fit goes on to
    part 2 (or, with m = k + 1, where nmin == nmax, ends with -2).  Only s = 0 would reach it; fsdp_create wants smoothing > 0.
ier 2 and ier 3 are reached (F_PICKS), as every other way through parcur_fit that FIT_BRANCHES names.
"""
from __future__ import annotations

import functools
from importlib import import_module

import numpy as np

REL = 1e-9
REL_SHORTCUT = 1e-5
MAP_FRAME = np.array([5e5, 5e6])


def libs(wide=False):
    return (import_module("oracle_lib_wide"), import_module("emu_lib_wide")) if wide else (import_module("oracle_lib"), import_module("emu_lib"))


# ---- a case -----------------------------------------------------------------------------------------------------------------
class Case:
    """One frame of the path stage.  expect: the status the case was built to give (0 unless built to raise); gpu: False for a raising
    case that cannot be shown from the kernel source to stay inside its arrays (non-finite centres, tracks at 1e17)."""

    __slots__ = ("name", "family", "lv", "rv", "l2r", "r2l", "pose", "prev", "gpath", "prm", "expect", "gpu", "kind", "on")

    def __init__(self, name, family, lv, rv, l2r, r2l, pose, prev=None, gpath=None, prm=None, expect=0, gpu=True, kind="case"):
        self.name, self.family, self.kind = name, family, kind
        self.lv, self.rv = np.asarray(lv, np.float64).reshape(-1, 2), np.asarray(rv, np.float64).reshape(-1, 2)
        self.l2r, self.r2l = np.asarray(l2r, np.int32).reshape(-1), np.asarray(r2l, np.int32).reshape(-1)
        self.pose = np.asarray(pose, np.float64)
        self.prev = None if prev is None else np.asarray(prev, np.float64)
        self.gpath = None if gpath is None else np.ascontiguousarray(gpath, np.float64).reshape(-1, 2)
        self.prm, self.expect, self.gpu = dict(prm or {}), expect, gpu
        self.on = None  # (record field, value): a case built to sit exactly ON a threshold; the oracle's record must read that value

    def key(self):
        """cases that can share a launch: the same parameters and the same global path"""
        return (tuple(sorted(self.prm.items())), None if self.gpath is None else self.gpath.tobytes())

    def moved(self, m, suffix):
        c = Case(self.name + suffix, self.family, m.pts(self.rv if m.mirror else self.lv), m.pts(self.lv if m.mirror else self.rv),
                 self.r2l if m.mirror else self.l2r, self.l2r if m.mirror else self.r2l, m.pose(self.pose),
                 None if self.prev is None else m.prev(self.prev), None if self.gpath is None else m.pts(self.gpath), self.prm, self.expect, self.gpu, self.kind)
        c.on = self.on
        return c


def identity(name, family, P, pose, **kw):
    """centres exactly P.  (Fewer than three points: both sides get unmatched cones up to three, or the stage would take the
    previous path — path_fallback bit 1 — before it looked at a match.)"""
    P = np.asarray(P, np.float64).reshape(-1, 2)
    extra = max(0, 3 - len(P))
    V = np.concatenate([P, P[-1] + np.arange(1, extra + 1)[:, None] * [0.7, 0.4]]) if extra else P
    idx = np.concatenate([np.arange(len(P)), np.full(extra, -1)])
    return Case(name, family, V, V, idx, idx, pose, **kw)


def no_cones(name, family, pose, **kw):
    """both sides empty: the first fit runs on the previous path (bit 1), or on the global path"""
    return Case(name, family, np.zeros((0, 2)), np.zeros((0, 2)), [], [], pose, **kw)


class Motion:
    """mirror (y -> -y), then rotate by theta, then shift"""

    def __init__(self, mirror=False, theta=0.0, shift=(0.0, 0.0)):
        self.mirror, self.theta, self.shift = mirror, theta, np.asarray(shift, np.float64)
        c, s = np.cos(theta), np.sin(theta)
        self.R = np.array([[c, -s], [s, c]]) if theta != 0.0 else np.eye(2)
        if theta == np.pi / 2:  # a quarter turn, exactly
            self.R = np.array([[0.0, -1.0], [1.0, 0.0]])

    def vec(self, v):
        v = np.asarray(v, np.float64) * (np.array([1.0, -1.0]) if self.mirror else 1.0)
        return v @ self.R.T

    def pts(self, p):
        p = np.asarray(p, np.float64).reshape(-1, 2)
        return self.vec(p) + self.shift if len(p) else p.copy()

    def pose(self, q):
        return np.concatenate([self.pts(q[:2])[0], self.vec(q[2:])])

    def prev(self, p):
        out = p.copy()
        out[:, 1:3] = self.pts(p[:, 1:3])
        if self.mirror:
            out[:, 3] = -out[:, 3]
        return out


def motions(seed, map_frame=False):
    """[(suffix, Motion)]: canonical and mirrored, each at three poses; with map_frame the canonical one moved to map-frame coordinates"""
    rng = np.random.default_rng(seed)
    th, sh = rng.uniform(-np.pi, np.pi), rng.uniform(-40, 40, 2)
    out = []
    for mir in (False, True):
        tag = "/mirror" if mir else ""
        out += [(tag + "/canon", Motion(mir)), (tag + "/pi", Motion(mir, np.pi - 1e-3 * rng.uniform(0.1, 1.0))), (tag + "/rigid", Motion(mir, th, sh))]
    if map_frame:
        out.append(("/map", Motion(False, 0.0, MAP_FRAME)))
    return out


POSE0 = np.array([0.0, 0.0, 1.0, 0.0])


def line(n, step, x0=0.0, y0=0.0):
    return np.column_stack([x0 + np.arange(n) * step, np.full(n, y0)])


def arc(n, step, radius, x0=0.0):
    """n points `step` apart along a circle of signed radius (positive: turning left), starting at (x0, 0) along +x"""
    a = np.arange(n) * step / radius
    return np.column_stack([x0 + radius * np.sin(a), radius * (1 - np.cos(a))])


def prev_from(xy, rows):
    """a previous path (rows, 4) through the points xy (resampled to `rows` rows): [s, x, y, curvature 0]"""
    xy = np.asarray(xy, np.float64)
    s = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(xy, axis=0), axis=1))])
    at = np.linspace(0.0, s[-1], rows)
    out = np.zeros((rows, 4))
    out[:, 0], out[:, 1], out[:, 2] = at, np.interp(at, s, xy[:, 0]), np.interp(at, s, xy[:, 1])
    return out


# ---- the oracle on cases ----------------------------------------------------------------------------------------------------
def oracle_one(o, c, record=True):
    """the oracle in det mode under the case's parameters -> (row, decision record)"""
    with o.params(c.prm), o.math_mode(1):
        return o.path(c.lv, c.rv, c.l2r, c.r2l, c.pose, prev=_pad_prev(o, c.prev), global_path=c.gpath, record=record)


def _pad_prev(o, prev):
    if prev is None:
        return None
    out = np.full((o.PATH_POINTS, 4), np.nan)
    out[: len(prev)] = prev
    return out


def run_oracle(o, cases):
    """-> (records, [decision record]) in case order; one parameter switch per group of cases"""
    rows, recs = np.zeros(len(cases), o.RESULT_DTYPE), [None] * len(cases)
    for key, idx in groups(cases).items():
        with o.params(cases[idx[0]].prm), o.math_mode(1):
            for i in idx:
                c = cases[i]
                rows[i], recs[i] = o.path(c.lv, c.rv, c.l2r, c.r2l, c.pose, prev=_pad_prev(o, c.prev), global_path=c.gpath, record=True)
    return rows, recs


def groups(cases):
    out = {}
    for i, c in enumerate(cases):
        out.setdefault(c.key(), []).append(i)
    return out


def match_rows(dtype, cases, idx, max_match):
    m = np.zeros(len(idx), dtype)
    m["l2r"], m["r2l"] = -1, -1
    for k, i in enumerate(idx):
        c = cases[i]
        assert len(c.lv) <= max_match and len(c.rv) <= max_match  # (nothing in the kernel checks the counts)
        m["n_left_v"][k], m["n_right_v"][k] = len(c.lv), len(c.rv)
        m["left_v"][k, : len(c.lv)], m["right_v"][k, : len(c.rv)] = c.lv, c.rv
        m["l2r"][k, : len(c.lv)], m["r2l"][k, : len(c.rv)] = c.l2r, c.r2l
    return m


def prev_rows(o, cases, idx, default):
    """per-frame previous paths of a launch, or None when no frame of it has one"""
    if all(cases[i].prev is None for i in idx):
        return None
    return np.stack([default if cases[i].prev is None else _pad_prev(o, cases[i].prev) for i in idx])


def run_emu(o, e, cases, group):
    """-> emu_lib.PATH_DTYPE records in case order"""
    out = np.zeros(len(cases), e.PATH_DTYPE)
    by_prm = {}
    for key, idx in groups(cases).items():
        by_prm.setdefault(key[0], []).append(idx)
    for launches in by_prm.values():  # (one parameter switch per parameter set: it rebuilds the default previous path on both sides)
        with o.params(cases[launches[0][0]].prm), e.params(cases[launches[0][0]].prm):
            default = o.default_path()
            for idx in launches:
                m = match_rows(e.MATCH_DTYPE, cases, idx, e.MAX_MATCH)
                poses = np.stack([cases[i].pose for i in idx])
                out[idx] = e.path(poses, m, group, prev_paths=prev_rows(o, cases, idx, default), global_path=cases[idx[0]].gpath)
    return out


def run_gpu(make_context, o, cases):
    """make_context(prm) -> an open context; -> result records in case order.  One launch per (parameters, global path)."""
    assert all(c.gpu for c in cases)
    out = None
    for key, idx in groups(cases).items():
        c0 = cases[idx[0]]
        ctx = make_context(c0.prm)
        if out is None:
            out = np.zeros(len(cases), ctx.result_dtype)
        with o.params(c0.prm):
            prev = prev_rows(o, cases, idx, o.default_path())
        rows = match_rows(ctx.result_dtype, cases, idx, ctx.shapes.max_match)
        ctx.set_global_path(c0.gpath)
        try:
            out[idx] = ctx.path_batch(np.stack([cases[i].pose for i in idx]), rows, prev)
        finally:
            ctx.set_global_path(None)
    return out


KNOTS_MAX = 256  # include/fsdp.h FSDP_OVERFLOW_KNOTS: a spline of more knots is refused with 204, never truncated
OVERFLOW_KNOTS = 204


def expected(rows, recs):
    """what a library with that capacity must return: the oracle's records, except that a frame one of whose fits has more than 256 knots
    (by the oracle's own count) is refused with 204 (one refit of family F: 273 knots); a frame without a path has NaN in every row"""
    want = rows.copy()
    for i, r in enumerate(recs):
        if want["status"][i] == 0 and max(r["fit_knots"], default=0) > KNOTS_MAX:
            want["status"][i] = OVERFLOW_KNOTS
    want["path"][want["status"] != 0] = np.nan
    return want


# ---- placing a threshold ----------------------------------------------------------------------------------------------------
def solve(value, lo, hi, target, rtol=1e-10, iters=200):
    """t in [lo, hi] with |value(t) / target - 1| <= rtol, for a value that is continuous and monotonic there (Illinois false position
    with bisection steps); value(lo) and value(hi) must bracket the target"""
    flo, fhi = value(lo) - target, value(hi) - target
    assert np.isfinite(flo) and np.isfinite(fhi) and flo * fhi < 0, (lo, hi, flo + target, fhi + target, target)
    side = 0
    for it in range(iters):
        t = (lo * fhi - hi * flo) / (fhi - flo) if it % 3 != 2 else 0.5 * (lo + hi)
        if not (min(lo, hi) < t < max(lo, hi)):
            t = 0.5 * (lo + hi)
        f = value(t) - target
        if not np.isfinite(f):
            raise AssertionError((t, f))
        if abs(f) <= rtol * abs(target):
            return t
        if f * flo > 0:
            lo, flo = t, f
            if side == -1:
                fhi /= 2
            side = -1
        else:
            hi, fhi = t, f
            if side == 1:
                flo /= 2
            side = 1
    raise AssertionError(("no convergence", lo, hi, flo, fhi))


class Pair:
    """Two cases built to sit threshold (1 - rel) and threshold (1 + rel) on the recorded value `field`; `flips`: the record entry or
    result field that must differ between them ("fallback", "path", or a PathRec name)."""

    def __init__(self, name, family, below, above, field, threshold, rel, flips):
        self.name, self.family, self.below, self.above, self.field, self.threshold, self.rel, self.flips = name, family, below, above, field, threshold, rel, flips
        below.kind = above.kind = "pair"

    def check(self, o):
        (ra, da), (rb, db) = oracle_one(o, self.below), oracle_one(o, self.above)
        va, vb = da[self.field], db[self.field]
        assert ra["status"] == self.below.expect and rb["status"] == self.above.expect, (self.name, ra["status"], rb["status"])
        if self.field == "trim_index":  # the car 1e-9 m (map frame: 1e-6 m) either side of the bisector of two neighbours
            lim = 1e-5 if abs(self.below.pose[0]) > 1e5 else 1e-8
            assert vb == va + 1 and 0 < da["trim_gap"] <= lim and 0 < db["trim_gap"] <= lim, (self.name, va, vb, da["trim_gap"], db["trim_gap"])
            return
        if self.field == "cut_index":  # adjacent scene scales: the cumulative length that decides stands within 1e-9 of the threshold on both
            near = lambda d: min(abs(d["cut_over"] / 20.0 - 1), abs(d["cut_under"] / 20.0 - 1))
            assert va != vb and near(da) <= REL and near(db) <= REL, (self.name, va, vb, near(da), near(db))
            return
        assert va < self.threshold < vb or (self.threshold == 0 and va < 0 < vb), (self.name, va, vb, self.threshold)
        scale = abs(self.threshold) if self.threshold else 1.0
        assert abs(va - self.threshold) <= 1.1 * self.rel * scale and abs(vb - self.threshold) <= 1.1 * self.rel * scale, (self.name, va, vb)
        assert ra["status"] == self.below.expect and rb["status"] == self.above.expect, (self.name, ra["status"], rb["status"])
        if self.flips == "fallback":
            assert ra["path_fallback"] != rb["path_fallback"], (self.name, int(ra["path_fallback"]))
        elif self.flips == "path":
            assert not np.array_equal(ra["path"], rb["path"], equal_nan=True), self.name
        else:
            assert da[self.flips] != db[self.flips], (self.name, self.flips, da[self.flips])


def pair_by(o, name, family, build, field, threshold, lo, hi, flips, rels=(REL,)):
    """build(t) -> Case; the recorded `field` is monotonic in t on [lo, hi] -> [Pair] at every rel"""
    value = lambda t: oracle_one(o, build(t))[1][field]
    out = []
    for rel in rels:
        tb = solve(value, lo, hi, threshold * (1 - rel) if threshold else -rel, rtol=rel / 10)
        ta = solve(value, lo, hi, threshold * (1 + rel) if threshold else rel, rtol=rel / 10)
        a, b = build(tb), build(ta)
        a.name, b.name = f"{name}@-{rel:g}", f"{name}@+{rel:g}"
        out.append(Pair(f"{name}@{rel:g}", family, a, b, field, threshold, rel, flips))
    return out


def dense_of(o, P, prm=None):
    """the dense samples of fit #1 on the centres P, as the oracle evaluates them"""
    prm = prm or {}
    k = min(max(len(P) - 1, 1), int(prm.get("max_deg", 3)))
    rc, u, t, cx, cy, _ier, _fp = o.splprep(P, float(prm.get("smoothing", 0.2)), k)
    assert rc == 0
    pe = float(prm.get("predict_every", 0.1))
    n = int(np.ceil(u[-1] / pe))
    return o.splev(t, cx, cy, k, np.arange(n) * pe)


# ---- family A: choice of centre points --------------------------------------------------------------------------------------
def family_a(max_match):
    """(cases, pairs).  Sides 1.5 m either side of the x axis, 0.9 m between cones; the car at the first cones."""
    cases = []
    sides = lambda n, y: line(n, 0.9, 0.3, y)
    counts = sorted({0, 1, 2, 3, 4, max_match})
    for nl in counts:
        for nr in counts:
            for matched in sorted({0, 1, 2, 3, max(nl, nr)}):
                l2r = [min(i, nr - 1) if i < matched and nr > 0 else -1 for i in range(nl)]
                r2l = [min(i, nl - 1) if i < matched and nl > 0 else -1 for i in range(nr)]
                cases.append(Case(f"A/counts/{nl}x{nr}/m{matched}", "A", sides(nl, 1.5), sides(nr, -1.5), l2r, r2l, POSE0))
    L, R = sides(5, 1.5), sides(5, -1.5)
    sel = {"more_right": ([0, 1, -1, -1, -1], [0, 1, 2, -1, -1]), "sum_right": ([0, 1, 2, -1, -1], [0, 1, 3, -1, -1]), "full_tie": ([0, 1, 2, -1, -1], [0, 1, 2, -1, -1]),
           "sum_left": ([0, 1, 4, -1, -1], [0, 1, 2, -1, -1]),
           # values other than -1 that are negative wrap like NumPy indices, count as matches and enter the sum
           "wrap_-2": ([0, 1, -2, -1, -1], [0, 1, 2, -1, -1]), "wrap_all": ([-5, -4, -3, -2, -2], [0, 1, 2, -1, -1]),
           "negative_sum_left": ([-2, -3, -1, -1, -1], [0, 1, -1, -1, -1]), "sum_-1_hands_over": ([-2, 1, -1, -1, -1], [0, 0, -1, -1, -1]),
           "negative_sum_tie": ([-2, -3, -1, -1, -1], [-3, -2, -1, -1, -1])}
    for k, (a, b) in sel.items():
        cases.append(Case(f"A/select/{k}", "A", L, R, a, b, POSE0))
    for k, (a, b) in {"past_end": ([0, 1, 5, -1, -1], [0, -1, -1, -1, -1]), "past_start": ([0, -6, 2, -1, -1], [0, -1, -1, -1, -1]),
                      "far": ([0, 1, 2**31 - 1, -1, -1], [-1] * 5), "far_negative": ([0, 1, -(2**31), -1, -1], [-1] * 5),
                      "bad_after_good": ([0, 1, 2, 3, 7], [-1] * 5), "unused_side_bad": ([0, 1, 2, -1, -1], [9, -1, -1, -1, -1])}.items():
        cases.append(Case(f"A/index/{k}", "A", L, R, a, b, POSE0, expect=None))
    # equal counts, and an index sum that leaves 32 bits: NumPy adds in int64, so 2 (2^31 - 1) + 5 beats 3 and the right side is used
    # (and raises on its indices), -2^32 + 4 loses to 3 and the left side is used.  A 32-bit sum wraps to 3 / 4 and takes the other side.
    BIG = 2**31 - 1
    wide = {"sum_beyond_int32": ([0, 1, 2, -1, -1], [BIG, BIG, 5, -1, -1]), "sum_below_int32": ([0, 1, 2, -1, -1], [-BIG - 1, -BIG - 1, 4, -1, -1]),
            "sum_beyond_int32_left": ([BIG, BIG, 5, -1, -1], [0, 1, 2, -1, -1]), "sum_wraps_to_tie": ([0, 1, 2, -1, -1], [-BIG - 1, -BIG - 1, 3, -1, -1])}
    for k, (a, b) in wide.items():
        c = Case(f"A/select/{k}", "A", L, R, a, b, POSE0, expect=None)
        cases += [c, c.moved(Motion(True), "/twin")]
    # a used side with an empty other side; one long side with a short other one
    cases.append(Case("A/empty_other/unmatched", "A", L, np.zeros((0, 2)), [-1] * 5, [], POSE0, expect=None))
    cases.append(Case("A/short_other/1", "A", sides(max_match, 1.5), sides(1, -1.5), [0] * max_match, [0], POSE0, expect=None))
    cases.append(Case("A/short_other/2", "A", sides(max_match, 1.5), sides(2, -1.5), [0, 1] + [-1] * (max_match - 2), [0, 1], POSE0, expect=None))
    out = []
    # the choice is made on counts and indices alone, the pose has no say in it: every case canonical; the grid's cases with unequal
    # sides also as their mirrored twin (the sides swapped), moved in rotation; every other case with a moved twin
    for k, c in enumerate(cases):
        out.append(c)
        if "/counts/" not in c.name:
            suffix, m = motions(100 + k)[1 + k % 5]
            out.append(c.moved(m, suffix))
        elif len(c.lv) != len(c.rv):
            suffix, m = motions(100 + k)[3 + k % 3]
            out.append(c.moved(m, suffix))
    for c in out:
        c.expect = status_of_choice(c)
    return out, []


def status_of_choice(c):
    """select_side_to_use and the fancy index other_side_cones[matches] (core_calculate_path.py:151-205), restated for the expectation
    alone: 104 where NumPy raises IndexError — a twin can differ from its case, since the left side wins a full tie"""
    nl, nr = len(c.lv), len(c.rv)
    if nl < 3 and nr < 3:
        return 0
    score = lambda m: (int((m != -1).sum()), int(m[m != -1].astype(np.int64).sum()))
    use_left = not score(c.r2l) > score(c.l2r)
    m, no = (c.l2r, nr) if use_left else (c.r2l, nl)
    if len(m) and no == 0:
        return 104
    return 104 if any(not -no <= int(v) < no for v in m) else 0


# ---- family B: fit #1 and its fallbacks -------------------------------------------------------------------------------------
def family_b(o):
    cases = []
    own_prev = prev_from(arc(60, 0.5, 25.0, -2.0), o.PATH_POINTS)  # a caller's previous path: 30 m on a 25 m arc -> extended on an arc
    bad_prev = own_prev.copy()
    bad_prev[7, 1:3] = bad_prev[6, 1:3]  # ... one that raises as well
    for deg in (3, 2, 1):
        prm = {} if deg == 3 else {"max_deg": deg}
        for n in (2, 3, 4, 5):
            P = arc(n, 1.1, 30.0, 0.2)
            for tag, prev in (("default", None), ("own", own_prev)):
                cases.append(identity(f"B/points/{n}/deg{deg}/{tag}", "B", P, POSE0, prev=prev, prm=prm))
        P = arc(6, 1.0, 30.0, 0.2)
        twin, nan, inf = P.copy(), P.copy(), P.copy()
        twin[3] = twin[2]
        nan[2, 1], inf[4, 0] = np.nan, np.inf
        for tag, prev, expect in (("default", None, 0), ("own", own_prev, 0), ("raising", bad_prev, None)):
            cases.append(identity(f"B/coincident/deg{deg}/{tag}", "B", twin, POSE0, prev=prev, prm=prm, expect=expect, gpu=tag != "raising"))
            cases.append(identity(f"B/nan/deg{deg}/{tag}", "B", nan, POSE0, prev=prev, prm=prm, expect=expect, gpu=False))
            cases.append(identity(f"B/inf/deg{deg}/{tag}", "B", inf, POSE0, prev=prev, prm=prm, expect=expect, gpu=False))
    # fallback values: previous path used (1), too far (4) with and without an extension of the previous path, and their unions
    far = np.array([0.0, 9.0, 1.0, 0.0])
    beyond = np.array([31.0, 12.0, 1.0, 0.0])  # past the end of own_prev: nothing of it in front -> extended
    cases += [no_cones("B/fallback/1", "B", POSE0), no_cones("B/fallback/1|16", "B", np.array([27.0, 9.0, np.cos(1.0), np.sin(1.0)]), prev=own_prev),
              no_cones("B/fallback/1|4", "B", far), identity("B/fallback/4", "B", line(6, 1.0, 0.2), far),
              identity("B/fallback/4|16", "B", line(6, 1.0, 0.2) + [0.0, 40.0], beyond, prev=own_prev),
              identity("B/fallback/2|4|16", "B", np.repeat(line(3, 1.0, 0.2), 2, axis=0) + [0.0, 40.0], beyond, prev=own_prev),
              identity("B/fallback/4|32", "B", line(6, 1.0, 0.2) + [0.0, 40.0], np.array([25.0, 0.5, 1.0, 0.0]), prev=prev_from(line(40, 0.5, 0.0), o.PATH_POINTS)),
              no_cones("B/fallback/1|32", "B", np.array([15.0, 0.2, 1.0, 0.0]), prev=prev_from(line(40, 0.5, 0.0), o.PATH_POINTS)),
              identity("B/fallback/16", "B", arc(12, 0.9, 20.0, 0.1), POSE0), identity("B/fallback/32", "B", line(12, 0.9, 0.1), POSE0),
              identity("B/fallback/0", "B", arc(24, 0.95, 40.0, 0.1), POSE0)]
    # bit 8: dense samples that coincide because the track lies at 1e17 (emulator only)
    # (one ulp there is 16 m / 64 m; three centres, so that the dense update stays below the working polyline's 1357 samples)
    for shift, step in ((1e17, 32.0), (-3e17, 64.0)):
        cases.append(identity(f"B/far_track/{shift:g}", "B", line(3, step, 0.0) + shift, np.array([shift, shift, 1.0, 0.0]), expect=None, gpu=False))
        cases.append(identity(f"B/far_track/prev/{shift:g}", "B", line(3, step, 0.0) + shift, np.array([0.0, 0.0, 1.0, 0.0]), expect=None, gpu=False))
    out = []
    for k, c in enumerate(cases):
        out.append(c)
        if np.isfinite(c.lv).all() and np.abs(c.lv).max(initial=0) < 1e6:
            # (map frame: only with a caller's previous path — the default one lies at the origin, 5e6 m from such a car)
            for suffix, m in motions(200 + k, map_frame=c.prev is not None and c.expect == 0)[1:]:
                out.append(c.moved(m, suffix))
    return out, []


# ---- family C: pose thresholds ----------------------------------------------------------------------------------------------
FRONT_INDICES = (0, 3, 4, 7, 8, 15, 16, 63, 64)


def family_c(o, max_match):
    cases, pairs = [], []
    track = arc(16, 0.95, 45.0, 0.0)  # 14.25 m of centres: 143 dense samples
    for suffix, m in motions(300, map_frame=True):
        P = m.pts(track)
        D = dense_of(o, P)
        n = len(D)
        tan = lambda i: (D[min(i + 1, n - 1)] - D[max(i - 1, 0)]) / np.linalg.norm(D[min(i + 1, n - 1)] - D[max(i - 1, 0)])
        nrm = lambda i: np.array([-tan(i)[1], tan(i)[0]])
        rel = (REL,) if suffix != "/map" else (1e-7,)  # (one ulp of a map-frame coordinate is 1e-9 m: the pair stands 1e-7 off there)
        # the closest dense sample at 5 m: the car beside sample 60, moved along the normal
        at = lambda t, i=60: identity("C/too_far" + suffix, "C", P, np.concatenate([D[i] + t * nrm(i), tan(i)]))
        if suffix != "/map":  # (beyond 5 m the default previous path takes over, which lies at the origin)
            pairs += pair_by(o, "C/too_far" + suffix, "C", at, "too_far", 5.0, 4.5, 5.5, "fallback", rel)
        # the first path point 0.5 m from the car (behind the start, on the tangent), and its bearing at 90 deg
        near = lambda t: identity("C/connect_dist" + suffix, "C", P, np.concatenate([D[0] - t * tan(0), tan(0)]))
        pairs += pair_by(o, "C/connect_dist" + suffix, "C", near, "connect_dist", 0.5, 0.4, 0.6, "n_refit", rel + ((REL_SHORTCUT,) if suffix != "/map" else ()))
        turn = lambda t: identity("C/connect_angle" + suffix, "C", P, np.concatenate([D[0] - 0.8 * tan(0) + 0.3 * nrm(0), m.vec([np.cos(t), np.sin(t)]) if not m.mirror else m.vec([np.cos(t), -np.sin(t)])]))
        if suffix != "/map":
            pairs += pair_by(o, "C/connect_angle" + suffix, "C", turn, "connect_angle", np.pi / 2, 1.0, 2.2, "n_refit", (REL, REL_SHORTCUT))
        # the first point in front of the car at chosen indices of the polyline, and at none
        for i in FRONT_INDICES + (n - 21, n - 20, n - 19):
            pos = 0.5 * (D[i] + D[i - 1]) + 0.3 * nrm(i) if i > 0 else D[0] - 0.2 * tan(0) + 0.3 * nrm(0)
            cases.append(identity(f"C/first_front/{i if i < 70 else f'n{i - n}'}" + suffix, "C", P, np.concatenate([pos, tan(i)])))
        cases.append(identity("C/first_front/none" + suffix, "C", P, np.concatenate([D[n - 1] + 0.3 * tan(n - 1) + 0.2 * nrm(n - 1), tan(n - 1)])))
        cases.append(identity("C/first_front/none_reversed" + suffix, "C", P, np.concatenate([D[0] + 0.1 * nrm(0), -tan(0)])))
        # the closest point for the trim: near-ties between neighbours i and i + 1 (the car 1e-9 m either side of their bisector)
        for i in FRONT_INDICES + (n - 21,):
            mid, t = 0.5 * (D[i] + D[i + 1]), (D[i + 1] - D[i]) / np.linalg.norm(D[i + 1] - D[i])
            d = 1e-9 if suffix != "/map" else 1e-6
            a, b = (identity(f"C/trim_tie/{i}{s}" + suffix, "C", P, np.concatenate([mid + e * t, t])) for s, e in (("-", -d), ("+", d)))
            pairs.append(Pair(f"C/trim_tie/{i}" + suffix, "C", a, b, "trim_index", None, None, "trim_index"))
        # ... and with the prepended connect point as the winner: the car 0.2 m from it, 0.8 m before the path
        cases.append(identity("C/trim/connect_point_wins" + suffix, "C", P, np.concatenate([D[0] - 0.8 * tan(0), tan(0)])))
    # paths shorter than 20 points; one point in front (nin < 2: status)
    for suffix, m in motions(310):
        for n in (2, 5, 19, 20, 21):
            P = m.pts(line(2, (n - 0.5) * 0.1, 0.1))
            cases.append(identity(f"C/short/{n}" + suffix, "C", P, m.pose(POSE0)))
            cases.append(identity(f"C/short/{n}/behind" + suffix, "C", P, m.pose(np.array([n * 0.1 + 0.3, 0.0, 1.0, 0.0]))))
        cases.append(identity("C/one_point" + suffix, "C", m.pts(line(2, 0.05, 0.1)), m.pose(POSE0), expect=103))
        cases.append(identity("C/one_point/connected" + suffix, "C", m.pts(line(2, 0.05, 0.8)), m.pose(POSE0)))
        # the straight extension from the two last points, arcs turning left and right
        cases.append(identity("C/extend/straight_two_points" + suffix, "C", m.pts(line(2, 0.15, 0.1)), m.pose(POSE0)))
        for r in (25.0, -25.0, 9.0, -9.0):
            cases.append(identity(f"C/extend/arc/{r:g}" + suffix, "C", m.pts(arc(14, 0.9, r, 0.1)), m.pose(POSE0)))
        # path length in front at 20 m: a straight track scaled; fitted radius at 10, 80, 100: an arc of that radius
        rel = (REL,)
        # (201 dense samples whatever t: plen is 200 steps of 0.1 in the fit's parameter times the speed of the curve, which a 3000 m
        # arc lifts 4e-9 above 1 and a zigzag of the centres, flattened by the smoothing, lowers continuously)
        zig = np.column_stack([np.zeros(max_match), (-1.0) ** np.arange(max_match)])
        grow = lambda t, m=m: identity("C/plen" + suffix, "C", m.pts(arc(max_match, 20.05 / (max_match - 1), 3000.0, 0.05) + t * zig), m.pose(POSE0))
        pairs += pair_by(o, "C/plen" + suffix, "C", grow, "plen", 20.0, 0.0, 2e-4, "fallback", rel)
        for thr, flips in ((10.0, "path"), (80.0, "fallback"), (100.0, "path")):
            bend = lambda t, m=m: identity(f"C/radius/{thr:g}" + suffix, "C", m.pts(arc(20, 0.5, t, 0.05)), m.pose(POSE0))
            pairs += pair_by(o, f"C/radius/{thr:g}" + suffix, "C", bend, "radius", thr, thr * 0.9, thr * 1.1, flips, rel)
    # The first point in front of the car made OBSERVABLE at every lane boundary of mpc_prepare's ballot: below n - 20 the index only enters
    # through plen, so the track holds exactly 200 dense steps from sample i to its end (n = 201 + i samples) and the zigzag of the plen pair
    # puts those 200 steps at 20 m (1 -+ 1e-9).  An index one too large counts 199 steps (19.9 m: extended on both members), one too small 201
    # (20.1 m: extended on neither), so a ballot or lane loop that is off by one at i fails one member of the pair.
    for i in FRONT_INDICES:
        for suffix, m in motions(320 + i)[:: 2]:
            def at_index(t, i=i, m=m, suffix=suffix):
                P = m.pts(arc(max_match, (20.05 + 0.1 * i) / (max_match - 1), 3000.0, 0.05) + t * zig)
                D = dense_of(o, P)
                assert len(D) == 201 + i
                tg = (D[i + 1] - D[max(i - 1, 0)]) / np.linalg.norm(D[i + 1] - D[max(i - 1, 0)])
                side = np.array([-tg[1], tg[0]])
                pos = 0.5 * (D[i] + D[i - 1]) + 0.3 * side if i > 0 else D[0] - 0.2 * tg + 0.3 * side
                return identity(f"C/first_front_plen/{i}" + suffix, "C", P, np.concatenate([pos, tg]))
            new = pair_by(o, f"C/first_front_plen/{i}" + suffix, "C", at_index, "plen", 20.0, 0.0, 2e-4, "fallback", (REL,))
            for p in new:
                for member in (p.below, p.above):
                    d = oracle_one(o, member)[1]
                    assert d["first_front"] == i and d["n_in_front"] == 201, (member.name, d["first_front"], d["n_in_front"])
            pairs += new
    # ... and at n - 21, the last index before mask[-20:] takes over: 20 steps in front, observable where mpc_path_length is 2 m
    for suffix, m in motions(330)[:: 2]:
        def at_tail(t, m=m, suffix=suffix):
            P = m.pts(arc(max_match, 14.25 / (max_match - 1), 1500.0, 0.05) + t * zig)
            D = dense_of(o, P)
            i = len(D) - 21
            tg = (D[i + 1] - D[i - 1]) / np.linalg.norm(D[i + 1] - D[i - 1])
            pos = 0.5 * (D[i] + D[i - 1]) + 0.3 * np.array([-tg[1], tg[0]])
            return identity("C/first_front_plen/n-21" + suffix, "C", P, np.concatenate([pos, tg]), prm={"mpc_path_length": 2.0})
        new = pair_by(o, "C/first_front_plen/n-21" + suffix, "C", at_tail, "plen", 2.0, 0.0, 2e-4, "fallback", (REL,))
        for p in new:
            for member in (p.below, p.above):
                d = oracle_one(o, member)[1]
                assert d["first_front"] == 122 and d["n_in_front"] == 21, (member.name, d["first_front"], d["n_in_front"])
        pairs += new
    # exactly on the threshold where it is representable: an axis-parallel track, the car 5.0 m beside it / 0.5 m before it
    straight = line(12, 1.0, 0.0)
    exact = {"too_far/exact": (straight, [3.0, 5.0, 1.0, 0.0], ("too_far", 5.0)), "too_far/exact_below": (straight, [3.0, -5.0, 1.0, 0.0], ("too_far", 5.0)),
             # (three and two centres: the fit returns its first sample bit for bit)
             "connect_dist/exact": (line(3, 2.0, 0.0), [-0.5, 0.0, 1.0, 0.0], ("connect_dist", 0.5)), "connect_angle/exact": (line(2, 3.0, 0.0), [0.0, -0.75, 1.0, 0.0], ("connect_angle", np.pi / 2)),
             "front_dot/exact": (line(3, 2.0, 0.0), [0.0, 0.25, 1.0, 0.0], ("front_dot", 0.0)),
             # 200 steps of the dense update that add up to 20.0 bit for bit (found by a scan over straight tracks)
             "plen/exact": (line(21, 1.0015, 0.05), POSE0, ("plen", 20.0)), "plen/exact_shifted": (line(21, 1.0015, 0.125), POSE0, ("plen", 20.0)),
             # arcs whose last 20 dense samples fit a circle of radius 80.0 bit for bit (found by stepping the arc's radius ulp by ulp around
             # the solution of the 80 m pair): `r_use < 80` is false there, the extension is straight
             "radius/80/exact": (arc(20, 0.5, float.fromhex("0x1.4041b5f2f1c80p+6"), 0.05), POSE0, ("radius", 80.0)),
             "radius/80/exact_2": (arc(20, 0.5, float.fromhex("0x1.4041b5f2f1cd7p+6"), 0.05), POSE0, ("radius", 80.0))}
    # two points of the polyline at bit-equal distance from the car in ONE lane's loop of closest_point: a path too far from the car puts the
    # rows of a caller's previous path into the polyline as they are; rows 3 and 11 of a U are mirror images in the car's axis and the closest
    u_turn = np.array([[6.0 - abs(t) * 0.8, np.sign(t) * (0.3 + 0.2 * abs(t))] for t in range(-7, 8)] + [[0.4, 1.7 + 0.8 * k] for k in range(1, 26)])
    prev_u = np.zeros((40, 4))
    prev_u[:, 1:3] = u_turn
    c = identity("C/trim_tie/same_lane", "C", line(6, 1.0, 0.2) + [0.0, 40.0], np.array([2.8, 0.0, 1.0, 0.0]), prev=prev_u)
    c.kind, c.on = "on", ("trim_gap", 0.0)
    cases += [c, c.moved(Motion(True), "/mirror"), c.moved(Motion(False, np.pi / 2), "/quarter")]
    for name, (P, pose, on) in exact.items():
        c = identity("C/" + name, "C", P, np.array(pose))
        c.kind, c.on = "on", on
        cases += [c, c.moved(Motion(True), "/mirror"), c.moved(Motion(False, np.pi / 2), "/quarter")]
    return cases, pairs


# ---- family D: the cut and the parameterisation -----------------------------------------------------------------------------
D_PREDICT_EVERY = (0.1, 0.08, 0.079, 0.078, 0.0552, 0.055, 0.0548)  # skip 1, 2, 2, 2, 3, 3, 3 with (n - 1) mod skip over all residues


def family_d(o, max_match):
    cases, pairs = [], []
    for pe in D_PREDICT_EVERY:
        prm = {} if pe == 0.1 else {"predict_every": pe}
        for k, (suffix, m) in enumerate(motions(400)[:: 1 if pe == 0.1 else 3]):
            for r in (30.0, -55.0, 400.0):
                cases.append(identity(f"D/skip/pe{pe:g}/r{r:g}" + suffix, "D", m.pts(arc(24, 0.9, r, 0.05)), m.pose(POSE0), prm=prm))
    for suffix, m in motions(410, map_frame=True):
        cases.append(identity("D/straight/x" + suffix, "D", m.pts(line(max_match, 0.9, 0.05)), m.pose(POSE0)))
        for r in (2900.0, 3100.0, -2999.0, 5000.0):  # a nearly straight path: the clamp at 3000
            cases.append(identity(f"D/nearly_straight/{r:g}" + suffix, "D", m.pts(arc(max_match, 0.9, r, 0.05)), m.pose(POSE0)))
        # a hairpin: the window radius falls below 1; an S: the curvature changes sign inside the filter window
        a = np.linspace(0, np.pi, 12)
        hair = np.concatenate([line(6, 0.9, 0.05), [5.0, 0.0] + 0.5 * np.column_stack([np.sin(a[1:]), 1 - np.cos(a[1:])]), line(6, -0.9, 4.1, 1.0)])
        cases.append(identity("D/hairpin" + suffix, "D", m.pts(hair), m.pose(POSE0)))
        x = np.arange(max_match) * 0.9 + 0.05
        for amp in (0.3, 1.0):
            cases.append(identity(f"D/s_curve/{amp:g}" + suffix, "D", m.pts(np.column_stack([x, amp * np.sin(x * 2 * np.pi / 7.0)])), m.pose(POSE0)))
    # horizon: the smallest and the largest mpc_prediction_horizon a context takes in this build
    for h in (1, 2, 3, o.PATH_POINTS):
        for r in (30.0, -400.0):
            cases.append(identity(f"D/horizon/{h}/r{r:g}", "D", arc(24, 0.9, r, 0.05), POSE0, prm={"mpc_prediction_horizon": h}))
    # the 20 m cut: between radii of 5 and 8 m the cumulative length of the 199th segment crosses 20 m (the cut index goes 199 -> 198)
    for suffix, m in motions(420):
        bend = lambda t, m=m: identity("D/cut" + suffix, "D", m.pts(arc(24, 0.9, t, 0.05)), m.pose(POSE0))
        pairs += cut_pair(o, "D/cut" + suffix, bend, 5.0, 8.0)
    return cases, pairs


def cut_pair(o, name, build, lo, hi):
    """bisect the scene scale until the cut index moves between two adjacent scales; the pair is proved by its recorded cumulative length"""
    idx = lambda t: oracle_one(o, build(t))[1]["cut_index"]
    ilo, ihi = idx(lo), idx(hi)
    assert ilo != ihi
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if idx(mid) == ilo:
            lo = mid
        else:
            hi = mid
    a, b = build(lo), build(hi)
    a.name, b.name = name + "@lo", name + "@hi"
    return [Pair(name, "D", a, b, "cut_index", None, None, "cut_index")]


# ---- family E: the global-path route ----------------------------------------------------------------------------------------
def family_e(o):
    cases = []
    car = np.array([1.0, 0.5, 1.0, 0.0])
    tables = {n: arc(n, 0.7, 60.0, -5.0) for n in (1, 2, 3, 63, 64, 65)}
    for n, tb in tables.items():
        cases.append(no_cones(f"E/table/{n}", "E", car, gpath=tb, expect=103 if n < 2 else 0))
        cases.append(no_cones(f"E/table/{n}/far_end", "E", np.array([tb[-1, 0], tb[-1, 1] + 0.5, 1.0, 0.0]), gpath=tb, expect=103 if n < 2 else 0))
    # two table points at bit-equal distance from the car (mirror images in the car's x axis), in the same lane group and in different ones
    # (a lane takes the indices lane, lane + G, ...: 3 and 11 meet in one lane's own loop at 8 lanes per frame, 3 and 19 also at 16, 1 and 65
    # at every group size; the others meet in the reduction across lanes)
    for n, (i, j) in {64: (3, 5), 65: (3, 40), 63: (7, 8), 40: (2, 38), 30: (3, 11), 41: (3, 19), 70: (1, 65)}.items():
        # (a line 0.5 m between points, none of them within 0.25 m of the car; the two 0.2 m either side of it)
        tb = np.column_stack([-7.75 + 0.5 * np.arange(n), np.full(n, 3.0)])
        tb[i], tb[j] = [2.0, 3.2], [2.0, 2.8]
        for tag, t in (("first", tb), ("swapped", tb[::-1].copy())):
            cases.append(no_cones(f"E/tie/{n}/{i}-{j}/{tag}", "E", np.array([2.0, 3.0, 1.0, 0.0]), gpath=t))
    # a table point at exactly 30.0 m (18, 24), one ulp inside, one ulp outside; fewer than two points kept
    for tag, y in (("exact", 24.0), ("inside", np.nextafter(24.0, 0.0)), ("outside", np.nextafter(24.0, 100.0))):
        tb = np.concatenate([line(20, 1.0, -3.0, 0.5), [[18.0, y]], line(10, 1.0, 19.0, 26.0)])
        cases.append(no_cones(f"E/30m/{tag}", "E", np.array([0.0, 0.0, 1.0, 0.0]), gpath=tb))
    cases.append(no_cones("E/kept/0", "E", np.array([200.0, 0.0, 1.0, 0.0]), gpath=tables[64], expect=103))
    cases.append(no_cones("E/kept/1", "E", np.array([-5.0 - 29.9, 0.0, 1.0, 0.0]), gpath=tables[64], expect=103))
    cases.append(no_cones("E/kept/2", "E", np.array([-5.0 - 29.2, 0.0, 1.0, 0.0]), gpath=tables[64]))
    for n in (30, 31, 32):  # n % 3 for the roll, the closest point at both ends and in the middle
        tb = arc(n, 0.8, -35.0, -2.0)
        for i in (0, n // 2, n - 1):
            cases.append(no_cones(f"E/roll/{n}/{i}", "E", np.array([tb[i, 0], tb[i, 1] + 0.3, 1.0, 0.0]), gpath=tb))
    out = list(cases)
    for k, c in enumerate(cases):  # (a moved twin has a table of its own, i.e. a launch of its own: one each, in rotation)
        suffix, m = motions(500 + k)[1 + k % 5]
        out.append(c.moved(m, suffix))
    return out, []


# ---- family F: FITPACK control flow -----------------------------------------------------------------------------------------
F_SEARCH = 40000

def _polyline(i):
    rng = np.random.default_rng([6, i])
    m = int(rng.choice([4, 5, 6, 8, 12, 24, 40, 64]))
    kind = rng.integers(4)
    step = rng.uniform(0.2, 1.5)
    x = np.cumsum(np.full(m, step) * (1 if kind != 3 else rng.uniform(0.05, 2.0, m)))
    if kind == 0:
        P = np.column_stack([x, rng.uniform(0.2, 3.0) * np.sin(x * rng.uniform(0.2, 2.0))])
    elif kind == 1:
        P = arc(m, step, rng.choice([-1, 1]) * rng.uniform(2.0, 60.0))
    else:
        P = np.column_stack([x, np.cumsum(rng.normal(0, rng.uniform(0.01, 0.6), m))])
    P = P + rng.normal(0, rng.choice([0.0, 1e-3, 0.03, 0.2]), P.shape)
    if rng.integers(8) == 0:  # a lattice: equal residual sums in fpknot
        P = np.round(P * 2) / 2
        keep = np.concatenate([[True], (np.diff(P, axis=0) != 0).any(axis=1)])
        P = P[keep]
    return P


def search_fit_polylines(o, n=F_SEARCH):
    """the search that chose F_PICKS: for every way through parcur_fit the first two candidates per smoothing that take it, by the
    oracle's branch recorder -> [(candidate, smoothing)]"""
    have, out = {}, []
    for i in range(n):
        P = _polyline(i)
        if len(P) < 4:
            continue
        s = (0.2, 0.01)[i % 2]
        mask = o.splprep_branches(P, s, 3)
        new = [b for b in range(len(o.FIT_BRANCHES)) if mask >= 0 and mask >> b & 1 and have.get((b, s), 0) < 2]
        for b in new:
            have[b, s] = have.get((b, s), 0) + 1
        if new:
            out.append((i, s))
    return out


F_PICKS = (0, 1, 2, 3, 5, 6, 7, 9, 14, 20, 128, 449, 634, 809, 1210, 1447, 1737, 3580, 4103, 4122, 5017, 5527, 5611, 6534, 15973, 17778, 20058,
           32075)  # search_fit_polylines(oracle_lib): candidate numbers, smoothing (0.2, 0.01)[i % 2]


@functools.lru_cache(maxsize=None)
def fit_polylines(wide=False):
    """[(polyline, smoothing, branch mask on the oracle)] of F_PICKS"""
    o, _ = libs(wide)
    return [(_polyline(i), (0.2, 0.01)[i % 2], o.splprep_branches(_polyline(i), (0.2, 0.01)[i % 2], 3)) for i in F_PICKS]


def branches_reached(o, masks):
    return {name for b, name in enumerate(o.FIT_BRANCHES) if any(m >> b & 1 for m in masks)}


def family_f(o):
    """the polylines of fit_polylines through the whole stage: as a global-path table (<= 64 points, all within 30 m of the car), as
    centres when they have <= MAX_MATCH points, as a previous path when they have PATH_POINTS points.  (The refit of such a noisy
    previous path needs 63 to 273 knots — the last is refused with 204, `expected` — and costs the emulator 5 to 14 s a frame.)"""
    cases = []
    for k, (P, s, _mask) in enumerate(fit_polylines(o.MAX_MATCH != 24)):
        prm = {} if s == 0.2 else {"smoothing": s}
        P = P - P[0] + [0.3, 0.0]
        if np.linalg.norm(P, axis=1).max() < 29.0:
            cases.append(no_cones(f"F/{k}/table", "F", POSE0, gpath=P, prm=prm, expect=None))
        if len(P) <= o.MAX_MATCH:
            cases.append(identity(f"F/{k}/centres", "F", P, POSE0, prm=prm, expect=None))
        elif len(P) == o.PATH_POINTS:
            prev = np.zeros((len(P), 4))
            prev[:, 1:3] = P
            cases.append(no_cones(f"F/{k}/previous", "F", POSE0, prev=prev, prm=prm, expect=None))
    return cases, []


def canonical(c):
    """the member of a case's motions that tests/golden/path_constructed.npz pins to the reference: not moved, finite, of ordinary size"""
    moved = any(tag in c.name for tag in ("/mirror", "/pi", "/rigid", "/map", "/quarter", "/twin"))
    return not moved and np.isfinite(c.lv).all() and np.abs(c.lv).max(initial=0.0) < 1e6


# ---- all of it --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def everything(wide=False):
    """-> {family: (cases, pairs)}; the cases of the pairs are part of the cases"""
    o, _ = libs(wide)
    fam = {"A": family_a(o.MAX_MATCH), "B": family_b(o), "C": family_c(o, o.MAX_MATCH), "D": family_d(o, o.MAX_MATCH), "E": family_e(o), "F": family_f(o)}
    return {k: (cases + [c for p in pairs for c in (p.below, p.above)], pairs) for k, (cases, pairs) in fam.items()}


@functools.lru_cache(maxsize=None)
def reference(wide=False):
    """-> {family: (oracle records, decision records)} of everything(wide), computed once and shared"""
    o, _ = libs(wide)
    return {k: run_oracle(o, cases) for k, (cases, _pairs) in everything(wide).items()}


def table(wide=False):
    """per family: cases, pairs, on-threshold cases, raising cases; the fallback values and the parcur_fit branches reached"""
    o, _ = libs(wide)
    lines, fallbacks, masks = [], set(), []
    for k, (cases, pairs) in everything(wide).items():
        rows, recs = reference(wide)[k]
        lines.append((k, len(cases), len(pairs), sum(c.kind == "on" for c in cases), int((rows["status"] != 0).sum())))
        fallbacks |= {int(v) for v in rows["path_fallback"][rows["status"] == 0]}
        masks += [b for r in recs for b in r["fit_branches"]]
    return lines, sorted(fallbacks), sorted(branches_reached(o, masks))
