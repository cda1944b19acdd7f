"""fsdp_plan_sequence on the GPU: n planners x T consecutive steps in one pass, the previous-path chains resolved by the
device kernels of csrc/sequence_kernel.h.  Expected values are T calls of plan_batch_sequential on the same kind of context
(sequence_support.lockstep), which the existing tests hold to the oracle and the reference; every comparison with them is byte
for byte."""
import importlib

import numpy as np
import pytest

import sequence_support as ss

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("ft-fsd-path-planning_amd")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(device=0)
    yield c
    c.close()


def same(a, b):
    """byte for byte, field by field (the bytes between the fields of a record are nobody's)"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.names:
        return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in a.dtype.names)
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def expected(c, off, cones, poses, n, initial_prev=None, compact=False):
    step = lambda o, x, p, prev: c.plan_batch(o, x, p, prev_paths=prev, compact=compact)  # noqa: E731
    return ss.lockstep(step, off, cones, poses, n, c.default_path(), initial_prev)


def check(c, off, cones, poses, n, initial_prev=None, want_replans=True):
    """one sequence call against the lock-step calls; returns the call's results"""
    res, final, again = c.plan_sequence(off, cones, poses, n, initial_prev=initial_prev)
    check.names, check.frames = ",".join(c.stage_names()), int(c._lib.fsdp_resident_frames(c._h))  # (of the sequence call's pass)
    ref, ref_final, ref_again = expected(c, off, cones, poses, n, initial_prev)
    differs = np.zeros(len(res), bool)
    for k in res.dtype.names:
        differs |= np.array([x.tobytes() != y.tobytes() for x, y in zip(res[k], ref[k])])
    bad = np.flatnonzero(differs)
    fields = [k for k in res.dtype.names if len(bad) and res[k][bad[0]].tobytes() != ref[k][bad[0]].tobytes()]
    assert len(bad) == 0, (f"frames {bad[:8]} (step, planner {[(int(b) // n, int(b) % n) for b in bad[:8]]}) of {len(res)} differ; frame {bad[0]}: "
                           + "; ".join(f"{k} {res[k][bad[0]]} != {ref[k][bad[0]]}" for k in fields)[:1500])
    assert same(final, ref_final)
    assert again == ref_again, (again, ref_again)
    assert not want_replans or again > 0
    return res, final, again


def test_fixture_three_planners_full_and_compact(ctx, golden_dir):
    g = ss.fixture(golden_dir)
    n = int(g["n_planners"])
    res, final, again = check(ctx, g["offsets"], g["cones"], g["poses"], n)
    # the patterns the fixture was built for, from the flags this pass saw
    shape = (len(res) // n, n)
    got = ss.patterns(g["event"].reshape(shape), res["path_fallback"].reshape(shape), (res["status"] == 0).reshape(shape))
    assert all(got.values()) and all(ss.fixture_patterns(g).values()), got
    assert np.array_equal(res["status"] == 0, g["ok"])
    err = np.abs(res["path"][g["ok"]] - g["path"][g["ok"]]).max()
    print("fixture: L-inf vs the reference planners", err, "frames planned again", again)
    assert err < 1e-5  # (the bound the stateful single-frame planner is held to on the GPU: tests/test_sequence.py)
    # final_prev = the last successful path of every planner
    for i in range(n):
        last = max(f for f in range(i, len(res), n) if res["status"][f] == 0)
        assert same(final[i], res["path"][last])
    cres, cfinal, cagain = ctx.plan_sequence(g["offsets"], g["cones"], g["poses"], n, compact=True)
    cref, _, _ = expected(ctx, g["offsets"], g["cones"], g["poses"], n, compact=True)
    assert same(cres, cref) and same(cfinal, final) and cagain == again
    assert same(cres["path"], res["path"])


def test_one_planner_ninety_steps_equal_reference_recording(ctx, golden_dir):
    g = np.load(golden_dir / "trackdrive_sequence.npz")
    res, final, again = check(ctx, g["offsets"], g["cones"], g["poses"], 1)
    assert (res["status"] == 0).all() and g["ok"].all()
    err = np.abs(res["path"] - g["path"]).max()
    print("trackdrive_sequence: L-inf vs the reference", err, "frames planned again", again)
    assert err < 1e-5  # (as tests/test_sequence.py holds the stateful planner to this recording)
    assert again >= 15


def test_continuation_through_final_prev(ctx, golden_dir):
    g = ss.fixture(golden_dir)
    n = int(g["n_planners"])
    off, cones, poses = g["offsets"], g["cones"], g["poses"]
    whole, wfinal, wagain = ctx.plan_sequence(off, cones, poses, n)
    cut = 13 * n
    a, afinal, aagain = ctx.plan_sequence(off[: cut + 1], cones, poses[:cut], n)
    b, bfinal, bagain = ctx.plan_sequence(off[cut:], cones, poses[cut:], n, initial_prev=afinal)  # (offsets with a base > 0)
    assert same(np.concatenate([a, b]), whole) and same(bfinal, wfinal)
    # planner 2 raised at step 0 and dropped out at step 1: in one call that frame meets no path and is not counted, in the cut
    # form likewise (its final_prev row after 13 steps is real only because later steps succeeded)
    assert aagain + bagain == wagain
    # an initial_prev with one NaN row
    init = np.stack([ctx.default_path()] * n)
    init[1, :, 1] += 0.25
    init[2] = np.nan
    res, _, _ = check(ctx, off, cones, poses, n, initial_prev=init)
    assert not same(res["path"][1], whole["path"][1])  # planner 1 drops out at step 0: it read its row
    assert same(res[2::n], whole[2::n])  # planner 2 started as a fresh planner both times


@pytest.mark.parametrize("n,steps,kernel", [(12, 100, "path_prep_kernel<16>"), (130, 100, "path_prep_kernel<8>"), (3, 40, "path_kernel<64>")])
def test_packing_regimes_of_the_speculative_pass(pkg, n, steps, kernel):
    c = pkg.Context(device=0)
    off, cones, poses = ss.fleet(n, steps)
    check(c, off, cones, poses, n)
    names = check.names
    assert kernel in names and "seq_mark_kernel,seq_chain_kernel,seq_final_kernel,assemble" in names, names
    c.close()


def test_one_run_of_every_step_next_to_a_planner_with_none(ctx):
    n, steps = 2, 40
    off, cones, poses = ss.fleet(n, steps, drop=None, drop_all_of=0)
    res, final, again = check(ctx, off, cones, poses, n)
    flagged = (res["path_fallback"] & ss.FB_READ_PREVIOUS) != 0
    assert flagged[0::n].all() and not flagged[1::n].any()
    # step 0 of the run meets no path at all; whether the later ones do depends on a step having succeeded — the lock-step
    # calls say how many, and check() holds the call to that count and to their bytes; a planner without flags is never planned again
    assert again <= steps - 1


def test_twenty_thousand_frames_are_one_pass(pkg):
    c = pkg.Context(device=0)
    n, steps = 200, 100
    off, cones, poses = ss.fleet(n, steps)
    res, _, again = check(c, off, cones, poses, n)
    assert check.frames == n * steps  # (the most recent pass held every frame: not a chunk)
    flagged = (res["path_fallback"] & ss.FB_READ_PREVIOUS) != 0
    assert flagged[-n:].any() and flagged[:n].any()  # chains reach across what the blocking calls would cut into four chunks
    c.close()


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
    check(c, off, cones, poses, n)
    c.close()


def test_global_path_context(pkg, golden_dir):
    g = np.load(golden_dir / "global_path.npz")
    c = pkg.Context(device=0)
    c.set_global_path(g["gp_track"])
    poses = g["gp_poses"].copy()
    for t in (10, 11, 25):  # the car 7 m beside the path it follows: beyond maximal_distance_for_valid_path
        poses[t, :2] += 7.0 * np.array([poses[t, 3], -poses[t, 2]]) / np.hypot(poses[t, 2], poses[t, 3])
    res, _, again = check(c, g["gp_offsets"], g["gp_cones"], poses, 1)
    assert (res["path_fallback"][[10, 11, 25]] & 4).all()
    n = 2  # ... and as two planners x 20 steps
    check(c, g["gp_offsets"], g["gp_cones"], poses, n)
    c.close()


@pytest.mark.parametrize("options,kernel", [({"path_mode": 1}, "path_kernel<64>"), ({"path_mode": 2, "pack": 1}, "path_prep_kernel<16>"),
                                            ({"path_mode": 2, "pack": 2}, "path_prep_kernel<8>")])
def test_wide_build(pkg, options, kernel):
    c = pkg.Context(device=0, shapes=pkg.WIDE, options=options)
    n, steps = 3, 24
    off, cones, poses = ss.fleet(n, steps, seed=6)
    check(c, off, cones, poses, n)
    assert kernel in check.names, check.names
    c.close()


def test_frames_beyond_the_lds_capacities_inside_a_run(pkg, golden_dir):
    g = np.load(golden_dir / "big_frames.npz")
    big = [f for f in range(len(g["ok"])) if g["ok"][f] and g["offsets"][f + 1] - g["offsets"][f] > 255][:2]
    assert len(big) == 2
    frames = []
    for kind in ("big0", "drop", "drop", "big1", "drop", "big0", "drop", "drop"):
        f = big[1] if kind == "big1" else big[0]
        xyt = g["cones"][g["offsets"][f] : g["offsets"][f + 1]]
        frames.append((xyt[:2] if kind == "drop" else xyt, g["poses"][f, :2], g["poses"][f, 2:]))
    off, cones, poses = pkg.pack_frames(frames)
    c = pkg.Context(device=0)
    res, _, again = check(c, off, cones, poses, 1)
    assert "sort_big_kernel" in check.names and again >= 4, (check.names, again)
    check(c, off, cones, poses, 2)  # two planners x four steps of the same frames
    c.close()


def test_refusals_leave_the_context_usable(pkg):
    import ctypes

    off, cones, poses = ss.fleet(2, 6)
    plain = pkg.Context(device=0)
    want = plain.plan_batch(off, cones, poses)

    def still_fine(c):
        assert same(c.plan_batch(off, cones, poses), want)

    skid = pkg.Context(device=0, mission=int(pkg.MissionTypes.skidpad))
    with pytest.raises(pkg.FsdpError, match="skidpad"):
        skid.plan_sequence(off, cones, poses, 2)
    with pytest.raises(pkg.FsdpError, match="skidpad"):  # (a skidpad context has no plan_batch to fall back on: the refusal left it
        skid.plan_batch(off, cones, poses)               # answering, with the error it always gives — tests/test_skidpad_gpu.py plans with such contexts)
    skid.close()
    c = pkg.Context(device=0)
    c.sort_cache_reset(2)
    with pytest.raises(pkg.FsdpError, match="sorting cache"):
        c.plan_sequence(off, cones, poses, 2)
    c.sort_cache_reset(0)
    still_fine(c)
    t = c.submit(off, cones, poses)
    with pytest.raises(pkg.FsdpError, match="not collected"):
        c.plan_sequence(off, cones, poses, 2)
    assert same(c.collect(t), want)
    still_fine(c)
    # counts below 1 and a frame count beyond the pass's index range: refused before anything is read
    out = np.zeros(len(poses), c.result_dtype)
    for n_planners, n_steps in ((0, 6), (2, 0), (-1, 6), (1 << 16, 1 << 15)):
        rc = c._lib.fsdp_plan_sequence(c._h, n_planners, n_steps, off.ctypes.data, cones.ctypes.data, poses.ctypes.data, None, out.ctypes.data, None,
                                       ctypes.cast(None, ctypes.POINTER(ctypes.c_longlong)))
        assert rc != 0 and c._lib.fsdp_last_error(c._h)
        still_fine(c)
    with pytest.raises(ValueError):
        c.plan_sequence(off, cones, poses, 5)  # 12 frames are no whole number of steps of 5 planners
    # a frame count the device has no memory for (4 M frames: ~95 KB of path-stage scratch each): an error code, and the
    # context plans on
    n_planners, n_steps = 4000, 1000
    huge = n_planners * n_steps
    with pytest.raises(pkg.FsdpError, match="fsdp_plan_sequence failed"):
        c.plan_sequence(np.zeros(huge + 1, np.int32), np.zeros((0, 3)), np.zeros((huge, 4)), n_planners)
    still_fine(c)
    res, _, _ = c.plan_sequence(off, cones, poses, 2)
    assert same(res, expected(c, off, cones, poses, 2)[0])
    c.close()
    plain.close()


def test_deterministic_and_independent_of_the_other_planners(ctx):
    n, steps = 12, 100
    off, cones, poses = ss.fleet(n, steps)
    a, afinal, aagain = ctx.plan_sequence(off, cones, poses, n)
    b, bfinal, bagain = ctx.plan_sequence(off, cones, poses, n)
    assert same(a, b) and same(afinal, bfinal) and aagain == bagain
    pick = [3, 7]
    frames = [t * n + i for t in range(steps) for i in pick]
    sub_off = np.zeros(len(frames) + 1, np.int32)
    sub_off[1:] = np.cumsum([off[f + 1] - off[f] for f in frames])
    sub_cones = np.concatenate([cones[off[f] : off[f + 1]] for f in frames])
    s, sfinal, _ = ctx.plan_sequence(sub_off, sub_cones, poses[frames], len(pick))
    assert same(s, a[frames]) and same(sfinal, afinal[pick])


def test_planner_object_and_replay(pkg, golden_dir):
    g = np.load(golden_dir / "trackdrive_sequence.npz")
    step = pkg.PathPlanner(pkg.MissionTypes.trackdrive, device=0)
    want = [step.calculate_path_in_global_frame(g["cones"][g["offsets"][t] : g["offsets"][t + 1]], g["poses"][t, :2], g["poses"][t, 2:]) for t in range(40)]
    seq = pkg.PathPlanner(pkg.MissionTypes.trackdrive, device=0)
    first = seq.calculate_path_in_global_frame(g["cones"][: g["offsets"][1]], g["poses"][0, :2], g["poses"][0, 2:])
    res, final, _ = seq.plan_sequence(g["offsets"][1:41], g["cones"], g["poses"][1:40], continue_state=True)
    assert same(first, want[0]) and same(np.ascontiguousarray(res["path"][:, : seq._ctx.horizon]), np.array(want[1:]))
    assert same(seq._prev, want[-1])
    untouched = pkg.PathPlanner(pkg.MissionTypes.trackdrive, device=0)
    untouched.plan_sequence(g["offsets"][:41], g["cones"], g["poses"][:40])
    assert untouched._prev is None
    with pytest.raises(RuntimeError):
        pkg.PathPlanner(pkg.MissionTypes.trackdrive, True, device=0).plan_sequence(g["offsets"][:41], g["cones"], g["poses"][:40])
