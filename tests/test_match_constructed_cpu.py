"""The match kernel (csrc/match_kernel.h, under the host emulator) against the oracle (fsdo_match) on sides built for it:
tests/match_support.py.  Standard and wide build.  Every comparison is bit for bit, over every case of a family; in every
family but the degenerate one the oracle's status is 0 on every case (asserted by run_oracle).  CPU-only."""
import functools

import numpy as np
import pytest

import emu_lib
import emu_lib_wide
import match_support as ms
import oracle_lib
import oracle_lib_wide

BUILDS = {"standard": (emu_lib, oracle_lib), "wide": (emu_lib_wide, oracle_lib_wide)}
GRID_REPS = {"standard": 8, "wide": 3}  # 13 x 13 x 8 = 1352 and 17 x 17 x 3 = 867 cases per family
MONOTONIC = dict(matches_should_be_monotonic=1)


@functools.lru_cache(maxsize=None)
def _grid(name, build):
    return ms.grid(name, BUILDS[build][0].MAX_LEN, GRID_REPS[build])


def _check(build, cases, what, params=None):
    emu, oracle = BUILDS[build]
    if params:
        with oracle.params(params), emu.params(params):
            ref = ms.run_oracle(oracle, cases)
            got = ms.run_emu(emu, cases)
    else:
        ref = ms.run_oracle(oracle, cases)
        got = ms.run_emu(emu, cases)
    ms.assert_equal(got, ref, what)
    return ref


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", list(ms.GENERATORS))
def test_grid(name, build):
    """Every (n_left, n_right) in 0..MAX_LEN squared: plain, wide, crossing / reversed and grid-snapped sides."""
    ref = _check(build, _grid(name, build), f"{name} grid ({build})")
    assert ref["n_left_v"].max() > BUILDS[build][0].MAX_LEN  # virtual cones were inserted


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", list(ms.GENERATORS))
def test_grid_monotonic(name, build):
    """The same with matches_should_be_monotonic = True in the kernel's parameter block and in the oracle's."""
    cases = _grid(name, build)[::2]
    ref = _check(build, cases, f"{name} grid, monotonic ({build})", MONOTONIC)
    if name == "crossing":  # the parameter arrived: sides that cross have matches that run backwards
        assert ms.differs(ref, ms.run_oracle(BUILDS[build][1], cases))


@pytest.mark.parametrize("build", list(BUILDS))
def test_discard_rule(build):
    """Length pairs at and next to the ratio 2: (1,2) (2,4) (3,6) (5,10) (6,12) keep both sides, (2,5) (3,7) (5,11) drop the
    shorter one, which then holds virtual cones only."""
    cases = ms.discard_rule()
    ref = _check(build, cases, f"discard rule ({build})")
    for c, r in zip(cases, ref):
        nl, nr = len(c[0]), len(c[1])
        if min(nl, nr) >= 2 and max(nl, nr) > 2 * min(nl, nr):  # the shorter side's cones are gone from its list
            short, lst = (c[0], r["left_v"][: r["n_left_v"]]) if nl < nr else (c[1], r["right_v"][: r["n_right_v"]])
            assert not any((lst == p).all(axis=1).any() for p in short)


@pytest.mark.parametrize("build", list(BUILDS))
def test_single_other_side_cone(build):
    """m = 1 (empty direction mask), and the `ne == 1` insertion with the car on either side of the tie."""
    _check(build, ms.single_other_cone(), f"single other-side cone ({build})")
    oracle = BUILDS[build][1]
    tie = ms.run_oracle(oracle, ms.ne_one_tie())
    for k in range(0, len(tie), 4):  # [nearer to R0, mirrored, nearer to V, mirrored]
        assert tie["n_right_v"][k] == 2 and tie["n_left_v"][k + 1] == 2
        assert np.array_equal(tie["right_v"][k][:2], tie["right_v"][k + 2][1::-1]) and not np.array_equal(tie["right_v"][k][0], tie["right_v"][k][1])
        assert np.array_equal(tie["left_v"][k + 1][:2], tie["left_v"][k + 3][1::-1])


@pytest.mark.parametrize("build", list(BUILDS))
def test_thresholds(build):
    """An other-side cone 1e-9 (relative) on either side of the ellipse, the 50 deg search angle, the 90 deg opposing-direction
    test, the 90 deg "between" test and the 85 deg drop rule: the two sides of every threshold give different results (on the
    oracle), and the kernel gives the oracle's on both."""
    oracle = BUILDS[build][1]
    for name, lo, hi in ms.threshold_pairs():
        for a, b in ((lo, hi), (ms.mirrored(lo), ms.mirrored(hi))):
            r = ms.run_oracle(oracle, [a, b])
            assert ms.differs(r[:1], r[1:]), name
    _check(build, ms.thresholds(), f"thresholds ({build})")


@pytest.mark.parametrize("build", list(BUILDS))
def test_non_adjacent_nearest_pair(build):
    """Sides that fold back: the two real cones nearest to a virtual one are not neighbours, and it is not inserted."""
    fb = ms.fold_back()
    cases = [c for c, _m in fb] + [ms.mirrored(c) for c, _m in fb]
    ref = _check(build, cases, f"fold back ({build})")
    n = len(fb)
    assert [int(v) for v in ref["n_right_v"][:n]] == [m for _c, m in fb] and [int(v) for v in ref["n_left_v"][n:]] == [m for _c, m in fb]


@pytest.mark.parametrize("build", list(BUILDS))
def test_capacity(build):
    """Lists that reach MAX_MATCH cones with the virtual ones (24; 32 in the wide build), on both sides."""
    emu = BUILDS[build][0]
    ref = _check(build, ms.capacity(emu.MAX_LEN), f"capacity ({build})")
    assert (ref["n_left_v"] == emu.MAX_MATCH).all() and (ref["n_right_v"] == emu.MAX_MATCH).all()


@pytest.mark.parametrize("build", list(BUILDS))
def test_degenerate_sides(build):
    """Coincident cones: a zero chord makes a search direction 0 / 0, the cone's virtual cone NaN, and NaN keys and distances
    reach the ranking and the arg-mins of the insertion.  The oracle is pinned to the reference on these sides
    (test_oracle_golden.py::test_oracle_matches_reference_on_degenerate_sides); the kernel returns the oracle's lists, NaN
    cones included.  Before the ranking and Grp::argmin ordered NaN, the lanes of a frame disagreed here and the emulator
    stopped at a dead-locked rendezvous."""
    emu, oracle = BUILDS[build]
    named = ms.degenerate()
    cases = [c for _n, c in named]
    ref = ms.run_oracle(oracle, cases)  # (the reference raises on none of them: status 0)
    assert np.isnan(ref["left_v"]).any() and np.isnan(ref["right_v"]).any()
    ms.assert_equal(ms.run_emu(emu, cases), ref, f"degenerate ({build})")
    with oracle.params(MONOTONIC), emu.params(MONOTONIC):
        ms.assert_equal(ms.run_emu(emu, cases), ms.run_oracle(oracle, cases), f"degenerate, monotonic ({build})")


def test_path_stage_on_lists_with_nan_cones():
    """What the match stage returns for the degenerate sides goes on to the path stage: the path kernel (eight lanes per frame)
    against fsdo_path in det-math mode on those lists, NaN cones included — status, fallback and every path value equal."""
    cases = [c for _n, c in ms.degenerate()]
    ref = ms.run_oracle(oracle_lib, cases)
    want = np.zeros(len(cases), oracle_lib.RESULT_DTYPE)
    with oracle_lib.math_mode(1):
        for k, (c, r) in enumerate(zip(cases, ref)):
            nl, nr = int(r["n_left_v"]), int(r["n_right_v"])
            want[k] = oracle_lib.path(r["left_v"][:nl], r["right_v"][:nr], r["l2r"][:nl], r["r2l"][:nr], c[2])
    m = np.zeros(len(cases), emu_lib.MATCH_DTYPE)
    for f in ("n_left_v", "n_right_v", "left_v", "right_v", "l2r", "r2l"):
        m[f] = ref[f]
    got = emu_lib.path(np.array([c[2] for c in cases]), m, 8)
    assert np.array_equal(got["status"], want["status"]) and (want["status"] == 0).all()
    assert np.array_equal(got["fallback"], want["path_fallback"])
    assert np.array_equal(got["path"], want["path"], equal_nan=True)


def test_duplicated_cone_frames_through_the_pipeline():
    """64 frames in which one of the 8 cones nearest the car is reported twice: sorting (a configuration that steps onto the
    twin costs NaN and goes last), matching and path kernels against the oracle, frame by frame."""
    off, cones, poses = ms.duplicated_cone_frames(ms.load_synth())
    with oracle_lib.math_mode(1):
        ref = oracle_lib.plan_batch(off, cones, poses)
    got, _n_dense = emu_lib.plan(off, cones, poses)
    assert (ref["status"] == 0).all()
    for k in ("status", "n_left", "n_right", "left_idx", "right_idx", "n_left_v", "n_right_v", "left_v", "right_v", "l2r", "r2l", "path_fallback"):
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
    assert np.array_equal(np.isnan(got["path"]), np.isnan(ref["path"]))
    assert np.nanmax(np.abs(got["path"] - ref["path"])) <= 1e-9  # (the bar of the emulated pipeline's other comparisons)
    twins = sum(len(set(map(tuple, cones[off[k] : off[k + 1]][r[s + "_idx"][: r["n_" + s]], :2]))) < r["n_" + s]
                for k, r in enumerate(ref) for s in ("left", "right"))
    assert twins >= 1  # a side that holds a cone and its twin
