"""The sorting kernels through the library on the frames built for the stage (tests/sort_support.py: threshold pairs at 1e-9 and
1e-5 with their mirrored / colourless twins at three poses, on-threshold and structural cases, and all of them padded across the
routes' size limits), against the oracle's fsdo_sort_frame in det-math mode.  One launch per route.  Index fields are compared
with array_equal, best_cost_* within the suite's GPU_RTOL = 1e-12 (tests/test_sort_ranked_gpu.py: the costs hold the device
libm's atan2 / acos); no case is left out.  That every pair flips on the oracle is asserted by test_sort_constructed_cpu.py.
Run with -m gpu on an MI355X."""
import importlib

import numpy as np
import pytest

import oracle_lib
import oracle_lib_wide
import sort_ranked_support as srs
import sort_support as ss

pytestmark = pytest.mark.gpu

GPU_RTOL = 1e-12
WIDE_PARAMS = dict(max_n_neighbors=8, max_length=16)
BUILDS = {"standard": (oracle_lib, {}, 5, 12), "wide": (oracle_lib_wide, WIDE_PARAMS, 8, 16)}
RAISES = "start pair beyond max_dist, the first reaches nothing"  # FSDO_REF_UNDEFINED_DFS_OOB = 102


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("ft-fsd-path-planning_amd")


@pytest.fixture(scope="module")
def contexts(pkg):
    made = {}

    def get(build, **options):
        key = (build, tuple(sorted(options.items())))
        if key not in made:
            made[key] = pkg.Context(device=0, mission=int(pkg.MissionTypes.trackdrive), params=dict(BUILDS[build][1]) or None,
                                    shapes=pkg.WIDE if build == "wide" else None, options=options or None)
            assert (made[key].shapes is pkg.WIDE) == (build == "wide")
        return made[key]

    yield get
    for c in made.values():
        c.close()


_cache = {}


def _unpadded(build):
    """(names, cases, oracle records) of pairs, on-threshold and structural cases: computed once per build, shared by the routes"""
    if build not in _cache:
        oracle, prm, k, max_len = BUILDS[build]
        pairs = ss.posed_pairs(k)
        named = [(f"{n} {m}", c) for n, _o, lo, hi in pairs for m, c in (("below", lo), ("above", hi))] + ss.on_threshold_posed() + ss.structural(max_len)
        names, cases = [n for n, _c in named], [c for _n, c in named]
        with oracle.params(prm):
            ref = ss.run_oracle(oracle, cases, require_ok=False)
        want = np.array([102 if n.startswith(RAISES) else 0 for n in names])
        assert np.array_equal(ref["status"], want)
        ref.setflags(write=False)
        _cache[build] = (names, cases, ref)
    return _cache[build]


def _padded(build):
    """(names, padded cases, oracle records): a few hundred frames of 64 to 300 cones"""
    if ("padded", build) not in _cache:
        oracle, prm, k, max_len = BUILDS[build]
        fam = ss.padded_family(k, max_len)
        cases = [p for _n, _c, p in fam]
        with oracle.params(prm):
            ref = ss.run_oracle(oracle, cases, require_ok=False)
            plain = ss.run_oracle(oracle, [c for _n, c, _p in fam], require_ok=False)
        for i in range(len(fam)):
            assert ss.records_equal_but_for_padding(ref[i], plain[i]) is None, fam[i][0]
        ref.setflags(write=False)
        _cache["padded", build] = ([n for n, _c, _p in fam], cases, ref)
    return _cache["padded", build]


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("route", ["default", "no_sort128", "cached"])
def test_sort_batch_on_constructed_frames(contexts, route, build):
    """Context.sort_batch: the 128-cone state (default options), the 255-cone state (no_sort128), and the cache-enabled kernels
    (sort_cache_reset(n): one planner per frame, empty entries — every side is searched by that instantiation)."""
    names, cases, ref = _unpadded(build)
    ctx = contexts(build, **({"no_sort128": 1} if route == "no_sort128" else {}))
    off, cones, poses = ss.as_batch(cases)
    assert np.diff(off).max() <= 36  # (the wide build's straight chains of 18 a side)
    if route == "cached":
        ctx.sort_cache_reset(len(cases))
    try:
        got = ctx.sort_batch(off, cones, poses)
        if route == "cached":
            assert not (ctx.sort_cache_hits() == 1).any()
    finally:
        if route == "cached":
            ctx.sort_cache_reset(0)
    ss.assert_equal(got, ref, f"sort_batch, {route} ({build})", cost_rtol=GPU_RTOL, names=names)


@pytest.mark.parametrize("build", list(BUILDS))
def test_sort_batch_ranked_on_constructed_frames(contexts, build):
    """Context.sort_batch_ranked(top_k=64, terms=True): the records, and every side's configurations, costs and terms against
    fsdo_side_configs (the cost-only pairs row by row)."""
    oracle, prm = BUILDS[build][:2]
    names, cases, ref = _unpadded(build)
    off, cones, poses = ss.as_batch(cases)
    got = contexts(build).sort_batch_ranked(off, cones, poses, top_k=64, terms=True)
    ss.assert_equal(got[0], ref, f"sort_batch_ranked ({build})", cost_rtol=GPU_RTOL, names=names)
    with oracle.params(prm), oracle.math_mode(1):
        n_multi, _ties = srs.check_against_oracle(oracle, off, cones, poses, got, GPU_RTOL)
    assert n_multi > 20


@pytest.mark.parametrize("build", list(BUILDS))
def test_padded_frames_on_every_route(contexts, build):
    """The padded family (64 / 65, 128 / 129, 255 / 256, 300 cones) in one sort_batch launch — the 255-cone state and, for the frames
    beyond it, global memory — in one ranked launch, and through plan_batch, whose pass reports that the big route was taken."""
    names, cases, ref = _padded(build)
    ctx = contexts(build)
    off, cones, poses = ss.as_batch(cases)
    assert len({int(n) for n in np.diff(off)}) == len(ss.PAD_SIZES) and np.diff(off).max() == 300
    ss.assert_equal(ctx.sort_batch(off, cones, poses), ref, f"padded ({build})", cost_rtol=GPU_RTOL, names=names)
    ss.assert_equal(ctx.sort_batch_ranked(off, cones, poses, top_k=8, terms=False)[0], ref, f"padded, ranked ({build})", cost_rtol=GPU_RTOL, names=names)
    small = [i for i, c in enumerate(cases) if len(c[0]) <= 128]
    ss.assert_equal(ctx.sort_batch(*ss.as_batch([cases[i] for i in small])), ref[small], f"padded, 128 state ({build})", cost_rtol=GPU_RTOL)
    res = ctx.plan_batch(off, cones, poses)
    assert ctx.route_stats()[0]  # sort_big_kernel ran
    ok = ref["status"] == 0
    for k in ("n_left", "n_right", "left_idx", "right_idx"):
        assert np.array_equal(res[k][ok], ref[k][ok]), k


def test_plan_batch_on_the_pairs(contexts):
    """plan_batch end to end on every pair member at the three poses: status and sorted indices equal to fsdo_plan_batch in det-math
    mode, the path within the suite's 1e-9."""
    pairs = ss.posed_pairs(5)
    cases = [c for _n, _o, lo, hi in pairs for c in (lo, hi)]
    off, cones, poses = ss.as_batch(cases)
    with oracle_lib.math_mode(1):
        ref = oracle_lib.plan_batch(off, cones, poses, n_threads=4)
    got = contexts("standard").plan_batch(off, cones, poses)
    assert np.array_equal(got["status"], ref["status"]), np.flatnonzero(got["status"] != ref["status"])[:8]
    ok = ref["status"] == 0
    assert ok.mean() > 0.8
    for k in ("n_left", "n_right", "left_idx", "right_idx", "path_fallback"):
        assert np.array_equal(got[k][ok], ref[k][ok]), k
    assert np.array_equal(np.isnan(got["path"][ok]), np.isnan(ref["path"][ok]))
    err = np.nan_to_num(np.abs(got["path"][ok] - ref["path"][ok]), nan=0.0).max()
    print(f"plan_batch on {int(ok.sum())} pair members: max |path - oracle| = {err:.3e}")
    assert err <= 1e-9


def test_coloured_pairs_without_unknown_cones(pkg):
    """use_unknown_cones = 0: the coloured pairs whose frames hold no UNKNOWN cone, with UNKNOWN cones mixed in between their rows
    (near the track: they would be neighbours).  The filter kernels drop them, the indices come back in the caller's array: the
    records of the oracle with the same parameter, and each pair still flips."""
    rng = np.random.default_rng(77)
    chosen = [(n, o, lo, hi) for n, o, lo, hi in ss.all_pairs(5) if "colourless" not in n and (lo[0][:, 2] != ss.UNKNOWN).all()]
    assert len(chosen) > 60

    def mixed(c):
        xyt, p = c
        rows = []
        for r in xyt:
            if rng.random() < 0.5:
                rows.append((r[0] + rng.uniform(-2.0, 2.0), r[1] + rng.uniform(-2.0, 2.0), ss.UNKNOWN))
            rows.append(tuple(r))
        return ss.typed(rows + [(4.0, 0.3, ss.UNKNOWN)], p)

    cases, obs = [], []
    for _n, o, lo, hi in chosen:
        state = rng.bit_generator.state
        cases.append(mixed(lo))
        rng.bit_generator.state = state  # (the same UNKNOWN cones in both members)
        cases.append(mixed(hi))
        obs.append(o)
    prm = dict(use_unknown_cones=0)
    with oracle_lib.params(prm):
        ref = ss.run_oracle(oracle_lib, cases)
    for i, o in enumerate(obs):
        assert ss.observable_differs(ref[2 * i], ref[2 * i + 1], o), chosen[i][0]
    ctx = pkg.Context(device=0, mission=int(pkg.MissionTypes.trackdrive), params=prm)
    try:
        got = ctx.sort_batch(*ss.as_batch(cases))
    finally:
        ctx.close()
    ss.assert_equal(got, ref, "use_unknown_cones = 0", cost_rtol=GPU_RTOL)
