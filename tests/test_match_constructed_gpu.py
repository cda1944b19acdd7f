"""fsdp_match_batch and fsdp_path_batch on sides built for the match stage (tests/match_support.py), against the oracle's
fsdo_match / fsdo_path, in the standard and the wide build, with and without matches_should_be_monotonic.  Every test is one
launch of a few thousand tiny frames.  The comparisons of the match stage are bit for bit; the oracle's status is 0 on every
case of every family (asserted), none is left out.  Run with -m gpu on an MI355X."""
import importlib

import numpy as np
import pytest

import match_support as ms
import oracle_lib
import oracle_lib_wide

pytestmark = pytest.mark.gpu

MONOTONIC = dict(matches_should_be_monotonic=1)
VARIANTS = [("standard", False), ("standard", True), ("wide", False), ("wide", True)]
IDS = ["standard", "standard-monotonic", "wide", "wide-monotonic"]
GRID_REPS = {"standard": 4, "wide": 2}  # 13 x 13 x 4 x 4 families = 2704, 17 x 17 x 2 x 4 = 2312 cases


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("ft-fsd-path-planning_amd")


@pytest.fixture(scope="module")
def contexts(pkg):
    made = {}

    def get(build, monotonic):
        if (build, monotonic) not in made:
            made[build, monotonic] = pkg.Context(device=0, mission=int(pkg.MissionTypes.trackdrive), params=dict(MONOTONIC) if monotonic else None,
                                                 shapes=pkg.WIDE if build == "wide" else None)
            assert (made[build, monotonic].shapes is pkg.WIDE) == (build == "wide")
        return made[build, monotonic]

    yield get
    for c in made.values():
        c.close()


def _oracle(build):
    return oracle_lib_wide if build == "wide" else oracle_lib


_cache = {}


def _ordinary(build, monotonic):
    """(cases, oracle match records) of every family but the degenerate one: computed once, shared by the match and the path test"""
    if (build, monotonic) not in _cache:
        oracle = _oracle(build)
        cases = []
        for name in ms.GENERATORS:
            cases += ms.grid(name, oracle.MAX_LEN, GRID_REPS[build])
        cases += ms.discard_rule(reps=2) + ms.single_other_cone() + ms.thresholds() + ms.capacity(oracle.MAX_LEN)
        fb = [c for c, _m in ms.fold_back()]
        cases += fb + [ms.mirrored(c) for c in fb]
        with oracle.params(MONOTONIC if monotonic else {}):
            ref = ms.run_oracle(oracle, cases)  # asserts status 0 on every case
        assert ref["n_left_v"].max() == oracle.MAX_MATCH
        _cache[build, monotonic] = (cases, ref)
    return _cache[build, monotonic]


@pytest.mark.parametrize("build,monotonic", VARIANTS, ids=IDS)
def test_match_batch_on_constructed_sides(contexts, build, monotonic):
    """Grid (plain, wide, crossing, snapped), discard rule, single other-side cone, thresholds, fold-back sides and capacity."""
    cases, ref = _ordinary(build, monotonic)
    got = ms.run_gpu(contexts(build, monotonic), cases)
    ms.assert_equal(got, ref, f"constructed sides ({build}{', monotonic' if monotonic else ''})")


@pytest.mark.parametrize("build,monotonic", VARIANTS, ids=IDS)
def test_path_batch_on_the_match_records(contexts, build, monotonic):
    """fsdp_path_batch on those match records (fresh planners) against fsdo_path in det-math mode: status and path_fallback
    equal, the same NaN rows, and the path within 1e-9 — the bar every kernel-against-oracle comparison of the path stage in this
    suite holds (test_gpu_parity.py _assert_equal_to_oracle: the float chain holds no libm value in that mode)."""
    cases, ref = _ordinary(build, monotonic)
    oracle = _oracle(build)
    ctx = contexts(build, monotonic)
    want = np.zeros(len(cases), oracle.RESULT_DTYPE)
    with oracle.params(MONOTONIC if monotonic else {}), oracle.math_mode(1):
        for k, (c, r) in enumerate(zip(cases, ref)):
            nl, nr = int(r["n_left_v"]), int(r["n_right_v"])
            want[k] = oracle.path(r["left_v"][:nl], r["right_v"][:nr], r["l2r"][:nl], r["r2l"][:nr], c[2])
    rows = np.zeros(len(cases), ctx.result_dtype)
    for f in ("n_left_v", "n_right_v", "left_v", "right_v", "l2r", "r2l"):
        rows[f] = ref[f]
    got = ctx.path_batch(np.array([c[2] for c in cases]), rows)
    assert np.array_equal(got["status"], want["status"]), np.flatnonzero(got["status"] != want["status"])[:8]
    ok = want["status"] == 0
    assert ok.mean() > 0.9
    assert np.array_equal(got["path_fallback"][ok], want["path_fallback"][ok])
    assert np.array_equal(np.isnan(got["path"][ok]), np.isnan(want["path"][ok]))
    err = np.nan_to_num(np.abs(got["path"][ok] - want["path"][ok]), nan=0.0).reshape(int(ok.sum()), -1).max(axis=1)
    print(f"path_batch on {int(ok.sum())} match records ({build}, monotonic={monotonic}): max |path - oracle| = {err.max():.3e}")
    assert (err <= 1e-9).all(), (float(err.max()), int((err > 1e-9).sum()))


@pytest.mark.parametrize("build,monotonic", VARIANTS, ids=IDS)
def test_match_batch_on_degenerate_sides(contexts, build, monotonic):
    """Coincident cones (NaN search directions and virtual cones): the kernel returns the lists of the oracle, which
    test_oracle_golden.py pins to the reference on these sides.  The emulator runs them to completion
    (test_match_constructed_cpu.py::test_degenerate_sides)."""
    oracle = _oracle(build)
    cases = [c for _n, c in ms.degenerate()]
    with oracle.params(MONOTONIC if monotonic else {}):
        ref = ms.run_oracle(oracle, cases)
    assert np.isnan(ref["left_v"]).any() and np.isnan(ref["right_v"]).any()
    ms.assert_equal(ms.run_gpu(contexts(build, monotonic), cases), ref, f"degenerate sides ({build})")


def test_plan_batch_on_duplicated_cone_frames(pkg, contexts):
    """64 frames with one cone reported twice through fsdp_plan_batch, against fsdo_plan_batch in det-math mode."""
    off, cones, poses = ms.duplicated_cone_frames(pkg.synth)
    got = contexts("standard", False).plan_batch(off, cones, poses)
    with oracle_lib.math_mode(1):
        ref = oracle_lib.plan_batch(off, cones, poses, n_threads=4)
    assert (ref["status"] == 0).all()
    for k in ("status", "n_left", "n_right", "left_idx", "right_idx", "n_left_v", "n_right_v", "left_v", "right_v", "l2r", "r2l", "path_fallback"):
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
    assert np.array_equal(np.isnan(got["path"]), np.isnan(ref["path"]))
    assert np.nanmax(np.abs(got["path"] - ref["path"])) <= 1e-9
