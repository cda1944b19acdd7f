"""fsdp_submit_sequence on the GPU: sequence calls as tickets, whole or as planner slices of a recording, on one context or
sharded over several (MultiPlanner).  Expected values are blocking fsdp_plan_sequence calls, which tests/test_sequence_gpu.py
holds to the lock-step calls, the oracle and the reference; every comparison here is byte for byte."""
import ctypes
import importlib

import numpy as np
import pytest

import sequence_support as ss

pytestmark = pytest.mark.gpu

PATTERN = 0xA5


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("ft-fsd-path-planning_amd")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fix(golden_dir):
    g = ss.fixture(golden_dir)
    return g["offsets"], g["cones"], g["poses"], int(g["n_planners"])


@pytest.fixture(scope="module")
def fleet130():
    return ss.fleet(130, 20)


def same(a, b):
    """byte for byte, field by field (the bytes between the fields of a record are nobody's)"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.names:
        return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in a.dtype.names)
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def is_pattern(a):
    """every byte of every field (a copy of a record array does not carry the bytes between the fields)"""
    if a.dtype.names:
        return all(is_pattern(a[k]) for k in a.dtype.names)
    return bool((np.ascontiguousarray(a).view(np.uint8) == PATTERN).all())


def recording(pkg, c, off, cones, poses, total, pin, compact=False):
    """the recording's arrays as a caller holds them (page-locked or pageable) + result and final_prev arrays filled with PATTERN"""
    put = pkg.pinned_copy if pin else (lambda a, dtype=None: np.array(a, dtype=dtype))
    new = pkg.pinned_empty if pin else np.empty
    out = new(len(poses), c.compact_dtype if compact else c.result_dtype)
    final = new((total, c.shapes.path_points, 4), np.float64)
    out.view(np.uint8)[...] = PATTERN
    final.view(np.uint8)[...] = PATTERN
    return put(off, np.int32), put(np.asarray(cones, np.float64).reshape(-1, 3)), put(poses), out, final


def planners_of(off, cones, poses, total, lo, hi):
    """planners [lo, hi) of a step-major recording as a recording of their own"""
    frames = [t * total + p for t in range(len(poses) // total) for p in range(lo, hi)]
    sub = np.zeros(len(frames) + 1, np.int32)
    sub[1:] = np.cumsum([off[f + 1] - off[f] for f in frames])
    return sub, np.concatenate([cones[off[f] : off[f + 1]] for f in frames]), poses[frames], frames


def check_slices(pkg, c, off, cones, poses, total, slices, pin=True, compact=False):
    """the slices as tickets in flight together on c, collected in reverse order, against one blocking call on c"""
    whole, wfinal, wagain = c.plan_sequence(off, cones, poses, total, compact=compact)
    o, x, p, out, final = recording(pkg, c, off, cones, poses, total, pin, compact)
    tickets = [c.submit_sequence(o, x, p, hi - lo, compact=compact, planner_lo=lo, planners_total=total, out=out, final_prev_out=final)
               for lo, hi in slices if hi > lo]
    again = 0
    for t in reversed(tickets):
        r, f, a = c.collect(t)
        assert r is out and f is final
        again += a
    assert same(out, whole) and same(final, wfinal) and again == wagain, (again, wagain)
    return whole, wfinal, wagain


# ---- 1. the whole call ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("pin", [True, False])
def test_whole_call_as_a_ticket(pkg, ctx, fix, pin, compact):
    off, cones, poses, n = fix
    want, wfinal, wagain = ctx.plan_sequence(off, cones, poses, n, compact=compact)
    o, x, p, out, final = recording(pkg, ctx, off, cones, poses, n, pin, compact)
    t = ctx.submit_sequence(o, x, p, n, compact=compact, out=out, final_prev_out=final)
    res, got_final, again = ctx.collect(t)
    assert res is out and same(res, want) and same(got_final, wfinal) and again == wagain and again > 0
    # ... and with an initial_prev block, one row of it NaN
    init = np.stack([ctx.default_path()] * n)
    init[1, :, 1] += 0.25
    init[2] = np.nan
    want, wfinal, wagain = ctx.plan_sequence(off, cones, poses, n, initial_prev=init, compact=compact)
    t = ctx.submit_sequence(o, x, p, n, initial_prev=pkg.pinned_copy(init) if pin else init, compact=compact, out=out, final_prev_out=final)
    res, got_final, again = ctx.collect(t)
    assert same(res, want) and same(got_final, wfinal) and again == wagain


# ---- 2. planner slices on one context -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("pin", [True, False])
def test_two_planner_slices_in_flight_collected_in_reverse(pkg, ctx, fix, pin, compact):
    """A ticket writes its own rows only.  With pageable arrays results leave the ticket's block at collect, so the rows of the slice
    not collected yet hold the pattern while both tickets are in flight.  Page-locked arrays are written in place by the GPU as soon
    as a ticket's pass ends, collected or not: there the same is shown with the first slice in flight alone, and the two in flight
    together are held to the whole call."""
    off, cones, poses, n = fix
    assert n == 3
    whole, wfinal, wagain = ctx.plan_sequence(off, cones, poses, n, compact=compact)
    o, x, p, out, final = recording(pkg, ctx, off, cones, poses, n, pin, compact)
    rows = np.arange(len(poses)) % n
    if pin:
        r, f, a0 = ctx.collect(ctx.submit_sequence(o, x, p, 1, compact=compact, planner_lo=0, planners_total=n, out=out, final_prev_out=final))
        assert same(out[rows == 0], whole[rows == 0]) and same(final[0], wfinal[0])
        assert is_pattern(out[rows != 0]) and is_pattern(final[1:])
        out.view(np.uint8)[...] = PATTERN
        final.view(np.uint8)[...] = PATTERN
    ta = ctx.submit_sequence(o, x, p, 1, compact=compact, planner_lo=0, planners_total=n, out=out, final_prev_out=final)
    tb = ctx.submit_sequence(o, x, p, 2, compact=compact, planner_lo=1, planners_total=n, out=out, final_prev_out=final)
    _, _, ab = ctx.collect(tb)
    assert same(out[rows != 0], whole[rows != 0]) and same(final[1:], wfinal[1:])
    if not pin:
        assert is_pattern(out[rows == 0]) and is_pattern(final[0])
    _, _, aa = ctx.collect(ta)
    assert same(out, whole) and same(final, wfinal) and aa + ab == wagain


# ---- 3. a fleet in four slices --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [{}, {"poison": 1}, {"path_mode": 1}, {"path_mode": 2, "pack": 1}], ids=["default", "poison", "mono", "split-pack1"])
def test_fleet_in_four_slices(pkg, fleet130, options):
    off, cones, poses = fleet130
    c = pkg.Context(device=0, options=options)
    c.set_overlap(2)
    slices = pkg.multi.planner_slices(130, 4)
    assert [hi - lo for lo, hi in slices] == [32, 33, 32, 33]
    whole, _, again = check_slices(pkg, c, off, cones, poses, 130, slices)
    flagged = ((whole["path_fallback"] & ss.FB_READ_PREVIOUS) != 0).reshape(20, 130)
    assert (flagged[1:] & flagged[:-1]).any() and again > 0  # runs of consecutive flagged steps
    c.close()


# ---- 4. cut in time and by planner ------------------------------------------------------------------------------------------------
def test_cut_both_ways(pkg, ctx, fix):
    off, cones, poses, n = fix
    whole, wfinal, wagain = ctx.plan_sequence(off, cones, poses, n)
    cut = 17 * n
    o, x, p, _, _ = recording(pkg, ctx, off, cones, poses, n, True)
    first = recording(pkg, ctx, off[: cut + 1], cones, poses[:cut], n, True)[3:]
    second = recording(pkg, ctx, off[cut:], cones, poses[cut:], n, True)[3:]
    slices = [(0, 1), (1, 3)]
    c = pkg.Context(device=0)
    c.set_overlap(2)
    firsts = [c.submit_sequence(o[: cut + 1], x, p[:cut], hi - lo, planner_lo=lo, planners_total=n, out=first[0], final_prev_out=first[1]) for lo, hi in slices]
    again, seconds = 0, []
    for (lo, hi), t in zip(slices, firsts):
        again += c.collect(t)[2]
        # (this slice's rows of the first half's final_prev are final: its second half reads them, the other slice's are not read)
        seconds.append(c.submit_sequence(o[cut:], x, p[cut:], hi - lo, initial_prev=first[1], planner_lo=lo, planners_total=n, out=second[0],
                                         final_prev_out=second[1]))
    for t in seconds:
        again += c.collect(t)[2]
    assert same(np.concatenate([first[0], second[0]]), whole) and same(second[1], wfinal) and again == wagain
    c.close()


# ---- 5. the rerun route -----------------------------------------------------------------------------------------------------------
def test_slice_ticket_is_repeated_with_the_big_route(pkg, golden_dir):
    g = np.load(golden_dir / "big_frames.npz")
    big = [f for f in range(len(g["ok"])) if g["ok"][f] and g["offsets"][f + 1] - g["offsets"][f] > 255][:2]
    assert len(big) == 2
    frames = []
    for kind in ("big0", "drop", "drop", "big1", "drop", "big0", "drop", "drop"):
        f = big[1] if kind == "big1" else big[0]
        xyt = g["cones"][g["offsets"][f] : g["offsets"][f + 1]]
        frames.append((xyt[:2] if kind == "drop" else xyt, g["poses"][f, :2], g["poses"][f, 2:]))
    off, cones, poses = pkg.pack_frames(frames)  # two planners x four steps; planner 1: drop, big1, big0, drop
    ref = pkg.Context(device=0)
    s_off, s_cones, s_poses, rows = planners_of(off, cones, poses, 2, 1, 2)
    want, wfinal, wagain = ref.plan_sequence(s_off, s_cones, s_poses, 1)
    ref.close()
    for pin in (True, False):
        c = pkg.Context(device=0)  # fresh: no route expected, the ticket's first pass lacks sort_big_kernel
        assert c.route_stats() == (False, False, 0)
        o, x, p, out, final = recording(pkg, c, off, cones, poses, 2, pin)
        res, got_final, again = c.collect(c.submit_sequence(o, x, p, 1, planner_lo=1, planners_total=2, out=out, final_prev_out=final))
        expect_big, _, reruns = c.route_stats()
        assert expect_big and reruns == 1
        assert same(res[rows], want) and same(got_final[1], wfinal[0]) and again == wagain
        assert is_pattern(res[0::2]) and is_pattern(got_final[0])
        c.close()


# ---- 6. variants ------------------------------------------------------------------------------------------------------------------
def test_use_unknown_cones_off(pkg):
    c = pkg.Context(device=0, params=dict(use_unknown_cones=False))
    n, steps = 3, 24
    off, cones, poses = ss.fleet(n, steps, seed=8)
    cones = cones.copy()
    rng = np.random.default_rng(3)
    for f in range(len(poses)):  # a quarter of every full frame's cones lose their colour, in the flattened order (UNKNOWN first)
        lo, hi = off[f], off[f + 1]
        if hi - lo > 2:
            blk = cones[lo:hi]
            blk[rng.random(hi - lo) < 0.25, 2] = 0.0
            cones[lo:hi] = blk[np.argsort(blk[:, 2], kind="stable")]
    check_slices(pkg, c, off, cones, poses, n, [(0, 2), (2, 3)])
    check_slices(pkg, c, off, cones, poses, n, [(0, 3)], pin=False)
    c.close()


def test_global_path_context(pkg, golden_dir):
    g = np.load(golden_dir / "global_path.npz")
    c = pkg.Context(device=0)
    c.set_global_path(g["gp_track"])
    poses = g["gp_poses"].copy()
    for t in (10, 11, 25):  # the car 7 m beside the path it follows: beyond maximal_distance_for_valid_path
        poses[t, :2] += 7.0 * np.array([poses[t, 3], -poses[t, 2]]) / np.hypot(poses[t, 2], poses[t, 3])
    _, _, again = check_slices(pkg, c, g["gp_offsets"], g["gp_cones"], poses, 2, [(0, 1), (1, 2)])
    assert again > 0
    c.close()


def test_wide_build(pkg):
    c = pkg.Context(device=0, shapes=pkg.WIDE)
    off, cones, poses = ss.fleet(3, 24, seed=6)
    check_slices(pkg, c, off, cones, poses, 3, [(0, 1), (1, 3)])
    check_slices(pkg, c, off, cones, poses, 3, [(0, 2), (2, 3)], pin=False, compact=True)
    c.close()


# ---- 7. mixed traffic -----------------------------------------------------------------------------------------------------------
def test_a_batch_ticket_and_a_sequence_ticket_on_one_context(pkg, ctx, fix):
    off, cones, poses, n = fix
    b_off, b_cones, b_poses = ss.fleet(5, 3, seed=2)
    want_batch = ctx.plan_batch(b_off, b_cones, b_poses)
    whole, wfinal, wagain = ctx.plan_sequence(off, cones, poses, n)
    o, x, p, out, final = recording(pkg, ctx, off, cones, poses, n, True)
    for order in (0, 1):
        out.view(np.uint8)[...] = PATTERN
        tb = ctx.submit(pkg.pinned_copy(b_off, np.int32), pkg.pinned_copy(b_cones), pkg.pinned_copy(b_poses)) if order == 0 else None
        ts = ctx.submit_sequence(o, x, p, 2, planner_lo=1, planners_total=n, out=out, final_prev_out=final)
        if tb is None:
            tb = ctx.submit(pkg.pinned_copy(b_off, np.int32), pkg.pinned_copy(b_cones), pkg.pinned_copy(b_poses))
        assert ctx.ticket_done(ts) in (True, False)
        first, second = (tb, ts) if order else (ts, tb)
        got = {id(t): ctx.collect(t) for t in (first, second)}
        assert same(got[id(tb)], want_batch)
        res = got[id(ts)][0]
        rows = np.arange(len(poses)) % n
        assert same(res[rows != 0], whole[rows != 0]) and same(got[id(ts)][1][1:], wfinal[1:])


# ---- 8. capacity and refusals -----------------------------------------------------------------------------------------------------
def test_capacity_and_refusals(pkg, fix):
    off, cones, poses, n = fix
    c = pkg.Context(device=0)
    whole, wfinal, wagain = c.plan_sequence(off, cones, poses, n)
    o, x, p, out, final = recording(pkg, c, off, cones, poses, n, True)

    def still_fine():
        r, f, a = c.collect(c.submit_sequence(o, x, p, n, out=out, final_prev_out=final))
        assert same(r, whole) and same(f, wfinal) and a == wagain

    assert c.ticket_capacity == 2
    held = [c.submit_sequence(o, x, p, n) for _ in range(2)]
    with pytest.raises(pkg.FsdpError, match=r"failed \(4\)"):
        c.submit_sequence(o, x, p, n)
    # a blocking call while sequence tickets are outstanding
    with pytest.raises(pkg.FsdpError, match="not collected"):
        c.plan_sequence(off, cones, poses, n)
    with pytest.raises(pkg.FsdpError, match="not collected"):
        c.plan_batch(off, cones, poses)
    assert same(c.collect(held[0])[0], whole)
    third = c.submit_sequence(o, x, p, n)  # room again after one collect
    for t in (third, held[1]):
        r, f, a = c.collect(t)
        assert same(r, whole) and same(f, wfinal) and a == wagain

    skid = pkg.Context(device=0, mission=int(pkg.MissionTypes.skidpad))
    with pytest.raises(pkg.FsdpError, match="skidpad"):
        skid.submit_sequence(o, x, p, n)
    skid.close()
    c.sort_cache_reset(n)
    with pytest.raises(pkg.FsdpError, match="sorting cache"):
        c.submit_sequence(o, x, p, n)
    c.sort_cache_reset(0)
    still_fine()

    def raw(n_planners, n_steps, lo, total, results=out.ctypes.data, ticket=True):
        t = ctypes.c_longlong(77)
        rc = c._lib.fsdp_submit_sequence(c._h, n_planners, n_steps, lo, total, o.ctypes.data, x.ctypes.data, p.ctypes.data, None, results,
                                         final.ctypes.data, ctypes.cast(None, ctypes.POINTER(ctypes.c_longlong)),
                                         ctypes.byref(t) if ticket else ctypes.cast(None, ctypes.POINTER(ctypes.c_longlong)))
        return rc, t.value

    steps = len(poses) // n
    # counts below 1, slices outside the recording, a frame count beyond the pass's index range, NULL results / ticket: refused
    # before anything is read or enqueued
    for args in ((0, steps, 0, n), (n, 0, 0, n), (-1, steps, 0, n), (1, steps, -1, n), (2, steps, 2, n), (n, steps, 0, n - 1), (1, steps, n, n),
                 (1 << 16, 1 << 15, 0, 1 << 16), (2, steps, 2**31 - 2, 2**31 - 1)):
        rc, t = raw(*args)
        assert rc != 0 and rc != 4 and t == -1 and c._lib.fsdp_last_error(c._h), args
        still_fine()
    assert raw(n, steps, 0, n, results=None)[0] != 0
    assert raw(n, steps, 0, n, ticket=False)[0] != 0
    still_fine()
    # a frame count the device has no memory for (4 M frames: ~95 KB of path-stage scratch each): an error code, nothing
    # enqueued, and the context plans on
    n_planners, n_steps = 4000, 1000
    huge = n_planners * n_steps
    with pytest.raises(pkg.FsdpError, match="fsdp_submit_sequence failed"):
        c.submit_sequence(np.zeros(huge + 1, np.int32), np.zeros((0, 3)), np.zeros((huge, 4)), n_planners, out=np.zeros(huge, c.result_dtype),
                          final_prev_out=np.zeros((n_planners, c.shapes.path_points, 4)))
    still_fine()
    assert same(c.plan_sequence(off, cones, poses, n)[0], whole)
    c.close()


# ---- 9. MultiPlanner ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contexts", [3, 4])
def test_multi_planner_shards_by_planner(pkg, ctx, fix, contexts):
    mp = pkg.MultiPlanner(devices=[0] * contexts)
    off, cones, poses, n = fix
    cases = [(off, cones, poses, n)]
    if contexts == 3:
        cases.append((*ss.fleet(10, 30), 10))
    for off, cones, poses, n in cases:
        whole, wfinal, wagain = ctx.plan_sequence(off, cones, poses, n)
        for pin in (False, True):
            arrays = (pkg.pinned_copy(off, np.int32), pkg.pinned_copy(cones), pkg.pinned_copy(poses)) if pin else (off, cones, poses)
            res, final, again = mp.plan_sequence(*arrays, n)
            assert same(res, whole) and same(final, wfinal) and again == wagain
        cres, cfinal, _ = mp.plan_sequence(off, cones, poses, n, compact=True)
        assert same(cres, ctx.plan_sequence(off, cones, poses, n, compact=True)[0]) and same(cfinal, wfinal)
    assert mp.zero_copy_batches > 0 and mp.staged_batches > 0
    # continuation through final_prev, sharded
    cut = 13 * n
    _, afinal, a = mp.plan_sequence(off[: cut + 1], cones, poses[:cut], n)
    b, bfinal, bb = mp.plan_sequence(off[cut:], cones, poses[cut:], n, initial_prev=afinal.copy())
    assert same(np.asarray(b), whole[cut:]) and same(bfinal, wfinal) and a + bb == wagain
    mp.close()


# ---- 10. replays kept in flight ---------------------------------------------------------------------------------------------------
def test_recordings_in_flight_equal_the_one_recording_replay(pkg, golden_dir):
    g = np.load(golden_dir / "trackdrive_sequence.npz")
    off, cones, poses = g["offsets"], g["cones"], g["poses"]
    obs = [[cones[off[f] : off[f + 1]][cones[off[f] : off[f + 1], 2] == t, :2] for t in range(5)] for f in range(len(poses))]
    mission = pkg.MissionTypes.trackdrive
    recs = [(poses[lo:hi, :2], poses[lo:hi, 2:], obs[lo:hi]) for lo, hi in ((0, 90), (0, 37), (20, 90), (5, 6))]
    # the one-recording form (blocking calls), chunks of 16 steps joined by final_prev -> initial_prev
    want = [pkg.replay.replay_stateful_batched(mission, *r, device=0, batch_frames=16) for r in recs]
    assert sum(w[2] for w in want) > 0
    # one context: its two ticket entries hold chunks of different recordings; a recording's next chunk follows its collect
    got, _, again = pkg.replay.replay_stateful_batched(mission, None, None, None, device=0, batch_frames=16, recordings=recs)
    assert len(got) == len(recs) and all(same(a, w[0]) for a, w in zip(got, want)) and again == sum(w[2] for w in want)
    # two contexts sharing the recordings, and one recording alone through them
    mp = pkg.MultiPlanner(devices=[0, 0], mission=int(mission))
    got, _, again = pkg.replay.replay_stateful_batched(mission, None, None, None, batch_frames=16, recordings=recs, multi=mp)
    assert all(same(a, w[0]) for a, w in zip(got, want)) and again == sum(w[2] for w in want)
    one, _, again = pkg.replay.replay_stateful_batched(mission, *recs[0], batch_frames=16, multi=mp)
    assert same(one, want[0][0]) and again == want[0][2]
    mp.close()
    with pytest.raises(ValueError):
        pkg.replay.replay_stateful_batched(mission, None, None, None, device=0, recordings=recs, cache=True)
