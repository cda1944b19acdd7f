"""TEST INFRASTRUCTURE of tests/test_polyline_capacity.py: the frames at the edge of the working polyline's capacity, what the
oracle (which has no capacity) says about them, and the comparison of a batch of records with that expectation."""
from __future__ import annotations

import ctypes
from importlib import import_module

import numpy as np

import parity

# csrc/path_kernel.h: the arena of a frame keeps PATH_CAP points of the working polyline.  path_front (:1075) refuses a frame whose
# first fit yields n1 dense samples with n1 + 1 + 50 > PATH_CAP: the 1 is the point connect_path_to_car may put in front
# (core_calculate_path.py:430-457), the 50 the points extend_path may append (:261-334: it appends 49 on an arc or 29 on a line).
PATH_CAP = 1408
RESERVE = 51
N1_MAX = PATH_CAP - RESERVE  # 1357 dense samples are planned, 1358 are refused
OVERFLOW_PATH = 203  # include/fsdp.h FSDP_OVERFLOW_PATH
FB_PREVIOUS = 1 | 2  # path_fallback bits a frame can carry when it reaches the guard (the first fit ran on the previous path)

SORT_MATCH_FIELDS = ("n_left", "n_right", "left_idx", "right_idx", "n_configs_left", "n_configs_right", "first_k_left", "first_k_right",
                     "n_left_v", "n_right_v", "left_v", "right_v", "l2r", "r2l")


def libs(wide=False):
    return (import_module("oracle_lib_wide"), import_module("emu_lib_wide")) if wide else (import_module("oracle_lib"), import_module("emu_lib"))


def take(batch, frames):
    """the frames `frames` of batch = (offsets, cones, poses[, prev]) as a batch of their own"""
    off, cones, poses = batch[:3]
    parts = [cones[off[f] : off[f + 1]] for f in frames]
    o = np.concatenate([[0], np.cumsum([len(c) for c in parts])]).astype(np.int32)
    out = (o, np.concatenate(parts) if parts else np.zeros((0, 3)), np.ascontiguousarray(poses[frames]))
    return out + ((np.ascontiguousarray(batch[3][frames]),) if len(batch) > 3 and batch[3] is not None else ())


class Case:
    """One parameter set and its frames: the oracle's records and fits, every frame's n1 by the reference's own rule
    (np.arange(0, max_u, predict_every) of fit #1, utils/spline_fit.py) and the records a library with PATH_CAP must return:
    the oracle's, except that a frame with n1 > N1_MAX has status 203 and no path."""

    def __init__(self, prm, off, cones, poses, prev=None, wide=False, global_path=None):
        self.prm, self.wide, self.prev, self.global_path = dict(prm), wide, prev, global_path
        self.off, self.cones, self.poses = np.asarray(off, np.int32), np.asarray(cones, np.float64), np.asarray(poses, np.float64)
        o, _ = libs(wide)
        n = len(self.poses)
        pe = float(self.prm.get("predict_every", 0.1))
        self.ref = np.zeros(n, o.RESULT_DTYPE)
        self.fits, self.nf = [], []
        with o.params(self.prm), o.math_mode(1):
            for f in range(n):
                row, nf, fits = o.plan_frame_capture(self.cones[self.off[f] : self.off[f + 1]], self.poses[f], None if prev is None else prev[f], global_path)
                self.ref[f] = row
                self.fits.append(fits)
                self.nf.append(nf)
        self.n1 = np.array([len(np.arange(0, fits[0][2][-1], pe)) if fits else 0 for fits in self.fits])
        self.refused = self.n1 > N1_MAX
        self.want = self.ref.copy()
        self.want["status"][self.refused & (self.ref["status"] == 0)] = OVERFLOW_PATH
        self.want["path"][self.want["status"] != 0] = np.nan
        self.want["path_fallback"][self.refused] &= FB_PREVIOUS

    def batch(self, frames=None):
        b = (self.off, self.cones, self.poses, self.prev)
        return b if frames is None else take(b, list(frames)) + ((None,) if self.prev is None else ())

    def retries(self, frames, knots):
        """frames of `frames` the three-kernel path stage hands to the exact kernel, as their fits explain it: a fit of a degree
        below 3 or with more knots than its packed kernels keep (`knots`); a refused frame gets as far as its first fit"""
        n = 0
        for f in frames:
            fits = self.fits[f][:1] if self.refused[f] else self.fits[f]
            n += any(k < 3 or nk > knots for k, nk, *_ in fits)
        return n

    def emulate(self, frames, group):
        """the frames through the host emulator's kernels (emu_lib.plan, lanes per frame `group`) -> records"""
        _, e = libs(self.wide)
        off, cones, poses, prev = self.batch(frames)
        d = ctypes.POINTER(ctypes.c_double)
        gp = None if self.global_path is None else np.ascontiguousarray(self.global_path, np.float64)
        if prev is not None:
            e.lib().emu_set_prev_paths(prev.ctypes.data_as(d))
        if gp is not None:
            e.lib().emu_set_global_path(gp.ctypes.data_as(d), ctypes.c_int(len(gp)))
        try:
            with e.params(self.prm):
                res, _ = e.plan(off, cones, poses, group)
        finally:
            e.lib().emu_set_prev_paths(None)
            e.lib().emu_set_global_path(None, ctypes.c_int(0))
        return res


def check(case, res, frames=None):
    """records `res` of the frames `frames` of `case` against the expectation: status; the path bit for bit (refused: every row NaN);
    the fallback bits; and the sorting and matching outputs of EVERY frame, refused ones included — those stages finished"""
    want = case.want if frames is None else case.want[list(frames)]
    assert np.array_equal(res["status"], want["status"]), (res["status"].tolist(), want["status"].tolist())
    ok = want["status"] == 0
    assert np.array_equal(res["path"][ok], want["path"][ok], equal_nan=True), np.flatnonzero(ok)[[not np.array_equal(a, b, equal_nan=True) for a, b in zip(res["path"][ok], want["path"][ok])]]
    assert np.isnan(res["path"][~ok]).all()
    assert np.array_equal(res["path_fallback"], want["path_fallback"])
    if "n_dense" in res.dtype.names:
        assert (res["n_dense"][~ok] == 0).all() and (res["n_dense"][ok] > 0).all()
    for k in SORT_MATCH_FIELDS:
        assert np.array_equal(res[k], want[k]), k
    parity.assert_intermediates_equal(res, want, np.ones(len(want), bool), cost_rtol=1e-12)  # (the device's own atan2 / acos: tests/parity.py)


def check_refit(case, frames, refit):
    """refit(i) -> (n, knots, coefficients x | y at [0, n) and [n, 2 n)) of the i-th of `frames` against the oracle's fit #2"""
    for i, f in enumerate(frames):
        k, n, t, cx, cy = case.fits[f][1]
        nk, tt, cc = refit(i)
        assert k == 3 and nk == n, (f, nk, n)
        assert np.array_equal(tt[:n], t), f
        assert np.array_equal(cc[: n - 4], cx[: n - 4]) and np.array_equal(cc[n : 2 * n - 4], cy[: n - 4]), f


# ---- frames whose first fit runs on a previous path the caller hands in -----------------------------------------------------
def previous_path_frames(predict_every, spec, rows=40, seed=4):
    """Frames without cones: the first fit runs on the planner's previous path (core_calculate_path.py:531-536), here an arc of
    `rows` points whose chord lengths add up to (n1 - 1/2) predict_every, so that the fit yields n1 dense samples.  spec: list of
    (n1, radius, pose kind): "start" = the car on the first point looking along the path; "before" = one metre in front of it
    (connect_path_to_car puts a point in front: n1 + 1 points); "back" = a tenth of a metre in front of it looking the other way (no point
    of the path in front of the car: extend_path appends 49 points, and remove_path_behind_car trims none: n1 + 49 points).
    Every frame is moved rigidly to a place of its own.  -> (offsets, cones, poses, prev (n, rows, 4))"""
    rng = np.random.default_rng(seed)
    poses, prev = np.zeros((len(spec), 4)), np.zeros((len(spec), rows, 4))
    for i, (n1, radius, kind) in enumerate(spec):
        a = np.linspace(0.0, 1.0, rows) * (n1 * predict_every / radius)
        xy = np.column_stack([radius * np.sin(a), radius * (1 - np.cos(a))])
        xy *= (n1 - 0.5) * predict_every / np.linalg.norm(np.diff(xy, axis=0), axis=1).sum()
        pos, head = {"start": ((0.0, 0.0), (1.0, 0.0)), "before": ((-1.0, 0.0), (1.0, 0.0)), "back": ((-0.1, 0.0), (-1.0, 0.0))}[kind]
        th, shift = rng.uniform(-np.pi, np.pi), rng.uniform(-50, 50, 2)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        xy = xy @ R.T + shift
        poses[i] = np.concatenate([np.array(pos) @ R.T + shift, np.array(head) @ R.T])
        prev[i, :, 1:3] = xy
        prev[i, 1:, 0] = np.cumsum(np.linalg.norm(np.diff(xy, axis=0), axis=1))
    return np.zeros(len(spec) + 1, np.int32), np.zeros((0, 3)), poses, prev


def merge(a, b, order):
    """two batches (offsets, cones, poses, prev) as one, frames in `order`: ("a" | "b", frame)"""
    parts = [take(a if s == "a" else b, [f]) for s, f in order]
    off = np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])]).astype(np.int32)
    return off, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts])


# ---- global paths whose slice within 30 m of the car holds a given number of points -----------------------------------------
def arc_table(spacing, n=4800, radius=200.0):
    a = (np.arange(n) - n // 2) * spacing / radius
    return np.ascontiguousarray(np.column_stack([radius * np.sin(a), radius * (1 - np.cos(a))]))


def slice_count(table, pose):
    """the reference's rule (core_calculate_path.py:514-529): the points of the global path closer than 30 m to the car"""
    return int((np.hypot(table[:, 0] - pose[0], table[:, 1] - pose[1]) < 30).sum())


def spacing_with(count, lo=0.0424, hi=0.0429, step=1e-6):
    """a spacing in [lo, hi] at which the slice around the pose (spacing / 4, 0) holds `count` points"""
    for sp in np.arange(hi, lo, -step):
        if slice_count(arc_table(sp), (sp / 4, 0.0)) == count:
            return float(sp)
    raise AssertionError(f"no spacing with {count} points")
