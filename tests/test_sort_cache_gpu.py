"""The experimental sorting cache on the GPU (PathPlanner(mission, experimental_performance_improvements=True),
include/fsdp.h fsdp_sort_cache_reset): against the reference's goldens (tests/golden/make_golden_sort_cache.py), at scale
against the cache-off kernels and the hit rule restated on the host, and isolated from every entry point that must not
see it."""
import ctypes
import importlib
import json

import numpy as np
import pytest

from parity import PATH_TOL
from test_sort_cache_cpu import NAMES, similar

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("ft-fsd-path-planning_amd")
SINGLE = ["mapped", "colourless", "no_unknown", "wide", "big"]


def load(golden_dir, name):
    g = dict(np.load(golden_dir / f"sort_cache_{name}.npz"))
    g["params"] = json.loads(str(g["params"])) or None
    return g


def frame(g, k):
    return g["cones"][g["offsets"][k] : g["offsets"][k + 1]], g["poses"][k]


def raised_as(exc, name):
    return name in [c.__name__ for c in type(exc).__mro__]


def default_path(ctx):
    out = np.zeros((ctx.shapes.path_points, 4))
    assert ctx._lib.fsdp_default_path(ctx._h, ctypes.c_void_p(out.ctypes.data)) == 0
    return out


def bits(a):
    """a structured result array as raw bytes per field (NaN payloads included)"""
    return {f: np.ascontiguousarray(a[f]).tobytes() for f in a.dtype.names}


def same(a, b):
    return bits(a) == bits(b)


@pytest.mark.parametrize("name", SINGLE)
def test_flagged_planner_matches_reference(golden_dir, name):
    g = load(golden_dir, name)
    planner = pkg.PathPlanner(pkg.MissionTypes.trackdrive, experimental_performance_improvements=True, device=0, params=g["params"])
    plain = pkg.PathPlanner(pkg.MissionTypes.trackdrive, device=0, params=g["params"])
    differs_checked = 0
    for k in range(len(g["poses"])):
        xyt, pose = frame(g, k)
        try:
            path, sl, sr = planner.calculate_path_in_global_frame(xyt, pose[:2], pose[2:], return_intermediate_results=True)[:3]
            exc = "ok"
        except Exception as e:  # noqa: BLE001
            exc, path = e, None
        hits = planner._ctx.sort_cache_hits()[0]
        if g["sort_ok"][k]:
            assert np.array_equal(hits, g["hits"][k]), (k, hits, g["hits"][k])
        if g["exc"][k] != "ok":
            assert exc != "ok" and raised_as(exc, str(g["exc"][k])), (k, exc, g["exc"][k])
            continue
        assert exc == "ok", (k, exc)
        assert np.abs(path - g["path"][k]).max() <= PATH_TOL, k
        nl, nr = (g["left_idx"][k] >= 0).sum(), (g["right_idx"][k] >= 0).sum()
        assert np.array_equal(sl, xyt[g["left_idx"][k][:nl], :2]) and np.array_equal(sr, xyt[g["right_idx"][k][:nr], :2]), k
        try:
            upath = plain.calculate_path_in_global_frame(xyt, pose[:2], pose[2:])
        except Exception:  # noqa: BLE001
            upath = None
        if g["uncached_exc"][k] == "ok" and np.abs(g["path"][k] - g["uncached_path"][k]).max() > 1e-5:
            assert upath is not None and np.abs(path - upath).max() > PATH_TOL, k  # the cached configuration really was reused
            differs_checked += 1
    if name in ("mapped", "wide"):
        assert differs_checked >= 1


def lockstep(g, ctx, n_planners):
    """the golden's frames through Context.plan_batch_sequential with the cache on: (results per frame, hit codes per frame)"""
    ctx.sort_cache_reset(n_planners)
    prev = [None] * n_planners
    res, hits = [None] * len(g["poses"]), np.zeros((len(g["poses"]), 2), np.int8)
    for s0 in range(0, len(g["poses"]), n_planners):
        ks = list(range(s0, s0 + n_planners))
        assert [int(g["planner"][k]) for k in ks] == list(range(n_planners))
        xs = [frame(g, k)[0] for k in ks]
        off = np.zeros(n_planners + 1, np.int32)
        off[1:] = np.cumsum([len(x) for x in xs])
        poses = np.array([g["poses"][k] for k in ks])
        pp = None if all(p is None for p in prev) else np.array([default_path(ctx) if p is None else p for p in prev])
        r = ctx.plan_batch_sequential(off, np.concatenate(xs), poses, pp)
        h = ctx.sort_cache_hits()
        for i, k in enumerate(ks):
            res[k], hits[k] = r[i], h[i]
            if int(r[i]["status"]) == 0:
                prev[i] = np.array(r[i]["path"])
    return res, hits


@pytest.mark.parametrize("name", NAMES)
def test_lockstep_context_matches_reference(golden_dir, name):
    """Every fixture through Context.sort_cache_reset(n) + plan_batch_sequential (standard build, or the wide one for max_length
    16): status, path, sorted indices, hit codes and the sorting diagnostics (n_configs, best_cost, first_k) per frame."""
    g = load(golden_dir, name)
    n = int(g["n_planners"])
    ctx = pkg._capi.Context(device=0, params=g["params"])
    if "wide" in name:
        assert ctx.shapes is pkg._capi.WIDE
    res, hits = lockstep(g, ctx, n)
    L = ctx.shapes.max_len
    for k, r in enumerate(res):
        if g["sort_ok"][k]:
            assert np.array_equal(hits[k], g["hits"][k]), (k, hits[k], g["hits"][k])
            assert np.array_equal(r["left_idx"], np.pad(g["left_idx"][k], (0, max(0, L - 16)), constant_values=-1)[:L]), k
            assert np.array_equal(r["right_idx"], np.pad(g["right_idx"][k], (0, max(0, L - 16)), constant_values=-1)[:L]), k
            assert [int(r["n_configs_left"]), int(r["n_configs_right"])] == list(g["n_configs"][k]), k
            # (costs hold the device libm's atan2 / acos: within 1e-12 like tests/test_gpu_parity.py; a reused cost is the stored one)
            assert np.allclose([r["best_cost_left"], r["best_cost_right"]], g["best_cost"][k], rtol=1e-12, atol=1e-12), k
            assert list(r["first_k_left"]) == list(g["first_k"][k][0]) and list(r["first_k_right"]) == list(g["first_k"][k][1]), k
        if g["exc"][k] != "ok":
            assert int(r["status"]) != 0, k
            continue
        assert int(r["status"]) == 0, k
        assert np.abs(r["path"][: ctx.horizon] - g["path"][k]).max() <= PATH_TOL, k


def test_cone_sorting_stage_chains_like_trace_sorter(golden_dir):
    g = load(golden_dir, "mapped")
    cs = pkg.ConeSorting(device=0, experimental_performance_improvements=True)
    for k in range(len(g["poses"])):
        xyt, pose = frame(g, k)
        cs.set_new_input(pkg.stages.ConeSortingInput(xyt, pose[:2], pose[2:]))
        if not g["sort_ok"][k]:
            with pytest.raises(Exception):
                cs.run_cone_sorting()
            continue
        sl, sr = cs.run_cone_sorting()
        nl, nr = (g["left_idx"][k] >= 0).sum(), (g["right_idx"][k] >= 0).sum()
        assert np.array_equal(sl, xyt[g["left_idx"][k][:nl], :2]) and np.array_equal(sr, xyt[g["right_idx"][k][:nr], :2]), k


# ---- scale ---------------------------------------------------------------------------------------------------------------
N_SCALE, STEPS = 16384, 5


def scale_batches(seed=7):
    """N_SCALE planners on four mapped tracks, each planner at its own place along its track, five steps of 0.45 m with the map
    jittered by up to 0.02 m per coordinate and step; every 97th planner loses a cone at step 3 (a count miss)."""
    rng = np.random.default_rng(seed)
    tracks = []
    for t in range(4):
        left, right, centre = pkg.synth.closed_track(48, 100 + t)
        tracks.append((np.concatenate([np.column_stack([right, np.ones(len(right))]), np.column_stack([left, np.full(len(left), 2.0)])]), centre))
    n_c = len(tracks[0][0])
    s0 = (np.arange(N_SCALE) // 4) / (N_SCALE // 4)
    out = []
    for step in range(STEPS):
        cones = np.empty((N_SCALE, n_c, 3))
        poses = np.empty((N_SCALE, 4))
        for t, (base, centre) in enumerate(tracks):
            sel = np.arange(t, N_SCALE, 4)
            cones[sel] = base
            pos, tan = centre(s0[sel] + step * 0.45 / (48 * 4.5))
            poses[sel] = np.column_stack([pos, tan])
        cones[:, :, :2] += rng.uniform(-0.02, 0.02, size=(N_SCALE, n_c, 2))
        keep = [np.delete(cones[i], 5, axis=0) if (step == 3 and i % 97 == 0) else cones[i] for i in range(N_SCALE)]
        off = np.zeros(N_SCALE + 1, np.int32)
        off[1:] = np.cumsum([len(c) for c in keep])
        out.append((off, np.concatenate(keep), poses))
    return out


def run_steps(ctxs, batches):
    """the batches through contexts that share the planners in contiguous blocks; (results, hits, prev used) per step"""
    n_each = N_SCALE // len(ctxs)
    for c in ctxs:
        c.sort_cache_reset(n_each)
    prev, steps = None, []
    for off, cones, poses in batches:
        rs, hs = [], []
        for j, c in enumerate(ctxs):
            lo, hi = j * n_each, (j + 1) * n_each
            o = off[lo : hi + 1] - off[lo]
            rs.append(c.plan_batch_sequential(o, cones[off[lo] : off[hi]], poses[lo:hi], None if prev is None else prev[lo:hi]))
            hs.append(c.sort_cache_hits())
        r = np.concatenate(rs)
        steps.append((r, np.concatenate(hs), prev))
        prev = np.where((r["status"] == 0)[:, None, None], r["path"], default_path(ctxs[0])[None] if prev is None else prev)
    return steps


@pytest.fixture(scope="module")
def scale():
    batches = scale_batches()
    one = run_steps([pkg._capi.Context(device=0)], batches)  # 16 384 frames: the blocking call's chunked form
    four = run_steps([pkg._capi.Context(device=0) for _ in range(4)], batches)
    return batches, one, four


def test_scale_chunked_equals_split_contexts(scale):
    _, one, four = scale
    for (r1, h1, _), (r4, h4, _) in zip(one, four):
        assert np.array_equal(h1, h4)
        assert same(r1, r4)


def test_scale_misses_are_the_uncached_kernels(scale):
    batches, one, _ = scale
    plain = pkg._capi.Context(device=0)
    n_hit = 0
    for (off, cones, poses), (r, h, prev) in zip(batches, one):
        miss = np.flatnonzero((h != 1).all(axis=1))
        n_hit += int((h == 1).sum())
        ref = plain.plan_batch_sequential(off, cones, poses, prev)
        assert same(r[miss], ref[miss])
    assert n_hit > N_SCALE  # the mapped track hits on most frames


def test_scale_hit_codes_follow_the_rule(scale):
    """The hit rule restated on the host (test_sort_cache_cpu.similar) on every frame, from the device's own start cones."""
    batches, one, _ = scale
    entries = [None] * N_SCALE
    near = 0
    for (off, cones, poses), (r, h, _) in zip(batches, one):
        for i in range(N_SCALE):
            flat = cones[off[i] : off[i + 1]]
            e = entries[i]
            new = dict(cones=flat, start=[None, None])
            ok_a, m_a = similar(flat, None if e is None else e["cones"]) if len(flat) >= 3 else (False, np.inf)
            for s, fk in enumerate((r[i]["first_k_left"], r[i]["first_k_right"])):
                if len(flat) < 3 or fk[0] < 0:
                    assert h[i, s] == -1
                    continue
                start = flat[fk[fk >= 0]]
                ok_s, m_s = similar(start, None if e is None else e["start"][s])
                if min(m_s, m_a) < 1e-12:
                    near += 1
                    continue
                assert h[i, s] == (1 if ok_s and ok_a else 0), (i, s)
                nc = r[i]["n_configs_left"] if s == 0 else r[i]["n_configs_right"]
                new["start"][s] = e["start"][s] if h[i, s] == 1 else (start if nc > 0 else None)
            if int(r[i]["status"]) not in (101, 102):
                entries[i] = new
    assert near == 0


def test_rerun_chunk_of_a_cached_call_keeps_its_planners(golden_dir):
    """A chunk of a cached lock-step call that has to run again, and whose first planner is not 0: 2048 planners replay the first
    three frames of the mapped fixture, except one in the last of four chunks (planners 1536..2047), which replays 272-cone frames
    that need sort_big_kernel.  The chunked context's first call lacks that route, so fsdp_collect runs the last chunk again; a
    context that never cuts and always carries both routes plans the same bytes and the same hit codes."""
    n, steps, big_planner = 2048, 3, 1700
    small, big = load(golden_dir, "mapped"), load(golden_dir, "big")
    assert all(e == "ok" for e in small["exc"][:steps]) and all(e == "ok" for e in big["exc"][:steps])
    a = pkg._capi.Context(device=0, options={"plan_chunks": 4})
    b = pkg._capi.Context(device=0, options={"plan_chunks": 1, "always_route": 1})
    out = []
    for ctx in (a, b):
        ctx.sort_cache_reset(n)
        prev, rs = None, []
        for k in range(steps):
            xs, ps = [frame(small, k)[0]] * n, np.tile(small["poses"][k], (n, 1))
            xs[big_planner], ps[big_planner] = frame(big, k)
            assert len(xs[big_planner]) > 255
            off = np.zeros(n + 1, np.int32)
            off[1:] = np.cumsum([len(x) for x in xs])
            r = ctx.plan_batch_sequential(off, np.concatenate(xs), ps, prev)
            rs.append((r, ctx.sort_cache_hits()))
            prev = np.where((r["status"] == 0)[:, None, None], r["path"], default_path(ctx)[None] if prev is None else prev)
        out.append(rs)
    for k, ((ra, ha), (rb, hb)) in enumerate(zip(*out)):
        assert same(ra, rb), k
        assert np.array_equal(ha, hb), k
        assert int(ra["status"][big_planner]) == 0, k
    assert (out[0][1][1] == 1).any()  # the small frames hit after step 0
    assert a.route_stats()[2] >= 1 and b.route_stats()[2] == 0


# ---- isolation -----------------------------------------------------------------------------------------------------------
def test_other_entry_points_do_not_see_the_cache(golden_dir):
    g = load(golden_dir, "lockstep")
    n = int(g["n_planners"])
    cached, plain = pkg._capi.Context(device=0), pkg._capi.Context(device=0)
    cached.sort_cache_reset(n)
    steps = []
    for s0 in range(0, len(g["poses"]), n):
        xs = [frame(g, k)[0] for k in range(s0, s0 + n)]
        off = np.zeros(n + 1, np.int32)
        off[1:] = np.cumsum([len(x) for x in xs])
        steps.append((off, np.concatenate(xs), g["poses"][s0 : s0 + n]))
    off, cones, poses = steps[0]
    cached.plan_batch_sequential(off, cones, poses, None)  # entries exist from here on
    h0 = cached.sort_cache_hits()
    for off, cones, poses in steps[1:3]:
        assert same(cached.plan_batch(off, cones, poses), plain.plan_batch(off, cones, poses))
        assert same(cached.plan_batch(off, cones, poses, compact=True), plain.plan_batch(off, cones, poses, compact=True))
        t1, t2 = cached.submit(off, cones, poses), plain.submit(off, cones, poses)
        assert same(cached.collect(t1), plain.collect(t2))
        assert np.array_equal(cached.sort_cache_hits(), h0)  # none of them touched the codes either
    # a call with the wrong frame count: an error, and the cache as if it never happened
    off, cones, poses = steps[1]
    with pytest.raises(pkg._capi.FsdpError):
        cached.plan_batch_sequential(off[: n], cones[: off[n - 1]], poses[: n - 1], None)
    r_a = cached.plan_batch_sequential(off, cones, poses, None)
    h_a = cached.sort_cache_hits()
    again = pkg._capi.Context(device=0)
    again.sort_cache_reset(n)
    again.plan_batch_sequential(*steps[0], None)
    assert same(again.plan_batch_sequential(off, cones, poses, None), r_a) and np.array_equal(again.sort_cache_hits(), h_a)
    assert (h_a == 1).any()
    # switched off: the results of a context that never had it
    cached.sort_cache_reset(0)
    for off, cones, poses in steps[2:4]:
        assert same(cached.plan_batch_sequential(off, cones, poses, None), plain.plan_batch_sequential(off, cones, poses, None))


def test_skidpad_context_refuses_the_cache():
    ctx = pkg._capi.Context(device=0, mission=int(pkg.MissionTypes.skidpad))
    with pytest.raises(pkg._capi.FsdpError):
        ctx.sort_cache_reset(1)


def test_flag_is_accepted_where_nothing_is_sorted():
    for m in (pkg.MissionTypes.acceleration, pkg.MissionTypes.ebs_test, pkg.MissionTypes.skidpad):
        p = pkg.PathPlanner(m, True, device=0)
        assert not p._sort_cache
        if m != pkg.MissionTypes.skidpad:
            assert p._ctx.n_cache == 0
