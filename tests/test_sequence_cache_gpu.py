"""fsdp_plan_sequence_cached on the GPU: byte for byte against the lock-step calls (fsdp_sort_cache_reset +
fsdp_plan_batch_sequential, chained by sequence_support.lockstep) — the reference's captures, a raising step inside a run, drift
against the run head, continuation across calls in any mix, the regimes of a fleet, refusals that leave the cache alone, the
planner object, determinism."""
import ctypes
import importlib

import numpy as np
import pytest

import sequence_cache_support as cs
import sequence_support as ss
from parity import PATH_TOL

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("ft-fsd-path-planning_amd")
NEW_KERNELS = ("seq_cache_mark_kernel", "seq_cache_resolve_kernel")


def context(n_planners, params=None):
    ctx = pkg._capi.Context(device=0, params=params)
    if n_planners:
        ctx.sort_cache_reset(n_planners)
    return ctx


def both(off, cones, poses, n, params=None, initial_prev=None):
    """one call on a fresh cache-on context, and the lock-step expectation on a second one -> (call, expectation, ctx, twin)"""
    ctx, twin = context(n, params), context(n, params)
    got = ctx.plan_sequence_cached(off, cones, poses, n, initial_prev=initial_prev)
    want = cs.lockstep(twin, off, cones, poses, n, initial_prev=initial_prev)
    return got, want, ctx, twin


def assert_equal(got, want):
    res, final, again, hits = got[:4]
    wres, wfinal, wagain, whits = want
    assert np.array_equal(hits, whits), np.flatnonzero((hits != whits).any(axis=1))
    assert cs.same(res, wres), (cs.differing(res, wres), np.flatnonzero(res["status"] != wres["status"]))
    assert final.tobytes() == wfinal.tobytes() and again == wagain


@pytest.mark.parametrize("name", cs.FIXTURES + ["colourless", "wide"])
def test_fixture_equals_lockstep_and_reference(golden_dir, name):
    g = cs.load(golden_dir, name)
    n = int(g["n_planners"])
    got, want, ctx, _twin = both(g["offsets"], g["cones"], g["poses"], n, g["params"])
    names = ctx.stage_names()
    names = names if isinstance(names, str) else ",".join(names)
    res, _final, _again, hits, resorted = got
    print(name, "hits", int((hits == 1).sum()), "resorted", resorted, "stages", names)
    assert_equal(got, want)
    for k in NEW_KERNELS:
        assert names.count(k) == 1, names
    assert names.count("_spec") >= 1 and "_cached" not in names
    ok = g["sort_ok"]
    assert np.array_equal(hits[ok], g["hits"][ok])
    good = g["exc"] == "ok"
    assert np.array_equal(res["status"] == 0, good)
    assert np.abs(res["path"][good][:, : ctx.horizon] - g["path"][good]).max() <= PATH_TOL
    # the reuse is real: some frame's path is not the one a cache-off sequence gives
    plain = context(0, g["params"]).plan_sequence(g["offsets"], g["cones"], g["poses"], n)[0]
    if name in ("mapped", "wide"):
        both_ok = (res["status"] == 0) & (plain["status"] == 0)
        h = ctx.horizon  # (rows beyond the horizon are NaN)
        assert (np.abs(res["path"][both_ok][:, :h] - plain["path"][both_ok][:, :h]).max(axis=(1, 2)) > PATH_TOL).any()


def stage_string(ctx):
    buf = ctypes.create_string_buffer(512)
    assert ctx._lib.fsdp_stage_names(ctx._h, buf, 512) == 0
    return buf.value.decode()


def test_stage_names_of_the_sequence_passes(golden_dir):
    """fsdp_stage_names character for character behind fsdp_plan_sequence and fsdp_plan_sequence_cached: 3 planners x 6 steps of
    ss.fleet (48 cones or 2 per frame: the 128-cone state, no route kernel), and with always_route the four 272-cone steps of the
    `big` fixture (the 255-cone state, and both route kernels with every pass)."""
    path = "match_kernel<32>,path_kernel<64>,"  # (18 frames and 4: a wavefront per frame)
    chain = "seq_mark_kernel,seq_chain_kernel,seq_final_kernel,assemble_kernel"
    cache = "seq_cache_mark_kernel,seq_cache_resolve_kernel,"
    off, cones, poses = ss.fleet(3, 6)
    assert set(np.diff(off).tolist()) == {2, 48}
    ctx = context(0)
    ctx.plan_sequence(off, cones, poses, 3)
    print("plan_sequence:", stage_string(ctx))
    assert stage_string(ctx) == "sort_kernel_128," + path + chain
    ctx.close()
    ctx = context(3)
    ctx.plan_sequence_cached(off, cones, poses, 3)
    print("plan_sequence_cached:", stage_string(ctx))
    assert stage_string(ctx) == "sort_kernel_128_spec," + cache + path + chain
    ctx.close()
    g = cs.load(golden_dir, "big")
    assert int(g["n_planners"]) == 1 and (np.diff(g["offsets"]) > 255).all()
    routed = pkg._capi.Context(device=0, options={"always_route": 1})
    routed.sort_cache_reset(1)
    routed.plan_sequence_cached(g["offsets"], g["cones"], g["poses"], 1)
    print("always_route, 272 cones:", stage_string(routed))
    assert stage_string(routed) == "sort_kernel_spec,sort_big_kernel_spec," + cache + path + "path_retry_kernel," + chain
    routed.close()


def raising_sequence(fuzz_frame, golden_dir, seed=3, jitter_seed=None):
    """A, A jittered, R, A jittered, A jittered (one planner): R = a frame of tests/golden/fuzz.npz the reference raises on"""
    fz = np.load(golden_dir / "fuzz.npz")
    R = (fz["cones"][fz["offsets"][fuzz_frame] : fz["offsets"][fuzz_frame + 1]], fz["poses"][fuzz_frame])
    A, pose = cs.track_frame(seed)
    rng = np.random.default_rng(seed if jitter_seed is None else jitter_seed)

    def jit():
        x = A.copy()
        x[:, :2] += rng.uniform(-0.02, 0.02, (len(A), 2))
        return x, pose

    return [(A, pose), jit(), R, jit(), jit()]


@pytest.mark.parametrize("fuzz_frame, n_cones", [(153, 7), (297, 12)])
def test_raising_step_inside_a_run(golden_dir, fuzz_frame, n_cones):
    frames = raising_sequence(fuzz_frame, golden_dir)
    assert len(frames[2][0]) == n_cones
    off, cones, poses = cs.pack(frames)
    got, want, _ctx, _twin = both(off, cones, poses, 1)
    wres, _f, _a, whits = want
    print("lock-step status", wres["status"], "hits", whits.tolist(), "resorted", got[4])
    assert int(wres["status"][2]) == 102  # the reference raises inside the search: the entry of step 1 is kept
    assert (whits[3] == 1).any()          # ... and step 3 hits against it
    assert_equal(got, want)
    assert got[4] >= 1


def test_raising_steps_of_three_staggered_planners(golden_dir):
    seqs = [raising_sequence(153, golden_dir, jitter_seed=10 + i) for i in range(3)]  # (the same track, each planner its own jitter)
    T = 5 + 2
    frames = []
    for t in range(T):
        for i in range(3):  # planner i runs its sequence from step i on; before and after it sees its first / last frame again
            frames.append(seqs[i][min(max(t - i, 0), 4)])
    off, cones, poses = cs.pack(frames)
    got, want, _ctx, _twin = both(off, cones, poses, 3)
    wres, whits = want[0], want[3]
    for i in range(3):
        assert int(wres["status"][(2 + i) * 3 + i]) == 102 and (whits[(3 + i) * 3 + i] == 1).any()
    assert_equal(got, want)
    assert got[4] >= 3


def test_drift_against_the_run_head():
    A, pose = cs.track_frame(5)
    frames = []
    for t in range(12):  # 0.06 m per step: within 0.1 m of the predecessor, 0.12 m from the run's head after two steps
        x = A.copy()
        x[:, 0] += 0.06 * t
        frames.append((x, pose))
    off, cones, poses = cs.pack(frames)
    got, want, _ctx, _twin = both(off, cones, poses, 1)
    print("hits", want[3].tolist())
    assert (want[3][1:] == 1).any() and (want[3][1:] == 0).any()
    assert_equal(got, want)


def test_continuation_in_any_mix(golden_dir):
    g = cs.load(golden_dir, "lockstep")
    n = int(g["n_planners"])
    off, cones, poses = g["offsets"], g["cones"], g["poses"]
    cut = lambda a, b: (off[a * n : b * n + 1], cones, poses[a * n : b * n])  # noqa: E731

    def seq(ctx, a, b, prev):
        r = ctx.plan_sequence_cached(*cut(a, b), n, initial_prev=prev)
        assert np.array_equal(ctx.sort_cache_hits(), r[3][-n:])
        return r[0], r[1], r[3]

    def lock(ctx, a, b, prev):
        r = cs.lockstep(ctx, *cut(a, b), n, initial_prev=prev)
        assert np.array_equal(ctx.sort_cache_hits(), r[3][-n:])
        return r[0], r[1], r[3]

    def run(parts):
        ctx, prev, res, hits = context(n), None, [], []
        for fn, a, b in parts:
            r, prev, h = fn(ctx, a, b, prev)
            res.append(r)
            hits.append(h)
        return np.concatenate(res), prev, np.concatenate(hits)

    one = run([(seq, 0, 6)])
    assert (one[2] == 1).any()
    for parts in ([(seq, 0, 2), (seq, 2, 6)], [(lock, 0, 2), (seq, 2, 6)], [(seq, 0, 3), (lock, 3, 6)], [(lock, 0, 6)]):
        other = run(parts)
        assert cs.same(one[0], other[0]), (parts, cs.differing(one[0], other[0]))
        assert one[1].tobytes() == other[1].tobytes() and np.array_equal(one[2], other[2])


@pytest.mark.parametrize("n_planners", [12, 130])
def test_fleet_regimes(n_planners):
    off, cones, poses = cs.jittered_fleet(n_planners, 100)
    got, want, ctx, _twin = both(off, cones, poses, n_planners)
    hits = got[3]
    print("hit sides", int((hits == 1).sum()), "of", hits.size, "replanned", got[2], "resorted", got[4])
    assert_equal(got, want)
    assert (hits == 1).any() and (hits == 0).any()  # (a frame behind a drop-out has another cone count: a miss)
    assert int(ctx._lib.fsdp_resident_frames(ctx._h)) == n_planners * 100  # one pass


def test_use_unknown_cones_off():
    """tests/test_sequence_gpu.py test_use_unknown_cones_off's batch: a quarter of every full frame's cones lose their colour and are
    dropped before sorting, so the cache sees the compacted cones and the indices are mapped back"""
    n, steps = 3, 24
    off, cones, poses = ss.fleet(n, steps, seed=8)
    cones = cones.copy()
    rng = np.random.default_rng(3)
    for f in range(len(poses)):
        lo, hi = off[f], off[f + 1]
        if hi - lo > 2:
            blk = cones[lo:hi]
            blk[rng.random(hi - lo) < 0.25, 2] = 0.0
            cones[lo:hi] = blk[np.argsort(blk[:, 2], kind="stable")]
    got, want, _ctx, _twin = both(off, cones, poses, n, params=dict(use_unknown_cones=False))
    print("hit sides", int((got[3] == 1).sum()), "checked", int((got[3] >= 0).sum()))
    assert_equal(got, want)


def test_refusals_leave_cache_and_context_alone():
    A, pose = cs.track_frame(7)
    off, cones, poses = cs.pack([(A, pose)] * 4)
    step = cs.pack([(A, pose)] * 2)
    # cache off
    ctx = context(0)
    with pytest.raises(RuntimeError, match="sorting cache"):
        ctx.plan_sequence_cached(off, cones, poses, 2)
    with pytest.raises(RuntimeError, match="sorting cache"):
        ctx.n_cache = 2  # (past the Python check: the library's own refusal)
        try:
            ctx.plan_sequence_cached(off, cones, poses, 2)
        finally:
            ctx.n_cache = 0
    assert cs.same(ctx.plan_batch(*step), context(0).plan_batch(*step))
    # cache on for another planner count; uncollected ticket
    ctx, twin = context(2), context(2)
    for c in (ctx, twin):
        c.plan_batch_sequential(*step, None)
    with pytest.raises(RuntimeError, match="sorting cache"):
        ctx.n_cache = 4
        try:
            ctx.plan_sequence_cached(off, cones, poses, 4)
        finally:
            ctx.n_cache = 2
    ticket = ctx.submit(*step)
    with pytest.raises(RuntimeError, match="not collected"):
        ctx.plan_sequence_cached(off, cones, poses, 2)
    ctx.collect(ticket)
    with pytest.raises(RuntimeError, match="sorting cache"):
        ctx.plan_sequence(off, cones, poses, 2)
    a, b = ctx.plan_batch_sequential(*step, None), twin.plan_batch_sequential(*step, None)
    assert cs.same(a, b) and np.array_equal(ctx.sort_cache_hits(), twin.sort_cache_hits()) and (ctx.sort_cache_hits() == 1).any()
    # ... and a sequence call after all that equals the twin's lock-step steps
    got = ctx.plan_sequence_cached(off, cones, poses, 2)
    assert_equal(got, cs.lockstep(twin, off, cones, poses, 2))


def test_skidpad_context_refuses():
    ctx = pkg.Context(device=0, mission=int(pkg.MissionTypes.skidpad))
    A, pose = cs.track_frame(7)
    off, cones, poses = cs.pack([(A, pose)] * 2)
    ctx.n_cache = 1  # (past the Python check: a skidpad context never has the cache on)
    with pytest.raises(pkg.FsdpError, match="skidpad"):
        ctx.plan_sequence_cached(off, cones, poses, 1)
    ctx.n_cache = 0
    with pytest.raises(pkg.FsdpError, match="skidpad"):  # (still answering, with the error it always gives)
        ctx.plan_batch(off, cones, poses)
    ctx.close()


def test_planner_object_continues_its_state(golden_dir):
    g = cs.load(golden_dir, "mapped")
    planner = pkg.PathPlanner(pkg.MissionTypes.trackdrive, True, device=0)
    twin = pkg.PathPlanner(pkg.MissionTypes.trackdrive, True, device=0)

    def single(p, k):
        xyt = g["cones"][g["offsets"][k] : g["offsets"][k + 1]]
        try:
            return p.calculate_path_in_global_frame(xyt, g["poses"][k][:2], g["poses"][k][2:])
        except Exception as e:  # noqa: BLE001
            return type(e).__name__

    want = [single(twin, k) for k in range(40)]
    first = single(planner, 0)
    assert np.array_equal(first, want[0])
    res, _final, _again, hits, _resorted = planner.plan_sequence_cached(g["offsets"][1:41], g["cones"], g["poses"][1:40], continue_state=True)
    assert (hits == 1).any()
    for k in range(1, 40):
        if isinstance(want[k], str):
            assert int(res["status"][k - 1]) != 0, k
        else:
            assert int(res["status"][k - 1]) == 0 and res["path"][k - 1][: planner._ctx.horizon].tobytes() == want[k].tobytes(), k
    a, b = single(planner, 40), single(twin, 40)
    assert type(a) is type(b) and (a == b if isinstance(a, str) else a.tobytes() == b.tobytes())
    assert np.array_equal(planner._ctx.sort_cache_hits(), twin._ctx.sort_cache_hits())
    with pytest.raises(RuntimeError):
        pkg.PathPlanner(pkg.MissionTypes.trackdrive, device=0).plan_sequence_cached(g["offsets"][:3], g["cones"], g["poses"][:2])


def test_deterministic_and_independent_of_the_other_planners():
    n, T = 12, 30
    off, cones, poses = cs.jittered_fleet(n, T)
    ctx = context(n)
    a = ctx.plan_sequence_cached(off, cones, poses, n)
    ctx.sort_cache_reset(n)
    b = ctx.plan_sequence_cached(off, cones, poses, n)
    assert cs.same(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[3], b[3]) and (a[2], a[4]) == (b[2], b[4])
    # a subset of the planners gives the subset of the results
    keep = [1, 4, 5, 10]
    frames = [(cones[off[t * n + i] : off[t * n + i + 1]], poses[t * n + i]) for t in range(T) for i in keep]
    sub = context(len(keep)).plan_sequence_cached(*cs.pack(frames), len(keep))
    sel = np.array([t * n + i for t in range(T) for i in keep])
    assert cs.same(sub[0], a[0][sel]) and np.array_equal(sub[3], a[3][sel])
    assert sub[1].tobytes() == a[1][keep].tobytes()
