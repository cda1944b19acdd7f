"""fsdp_plan_sequence_paths / fsdp_submit_sequence_paths on the GPU: sequence calls whose frames carry one path id each, the
previous-path chains resolved by seq_chain_table_kernel (csrc/sequence_table_kernel.h).  Expected values: every planner of the
constructed recording (tests/sequence_table_support.py) stepped frame by frame on the oracle, and T Context.submit(prev_paths=,
path_ids=) calls chained on the host — the route tests/test_gpath_table_gpu.py holds; every comparison is byte for byte.
AccelerationBatch.plan_sequence against a second batch stepped, and against the golden acceleration recording."""
import ctypes
import faulthandler
import importlib

import numpy as np
import pytest

import gpath_table_support as gts
import sequence_support as ss
import sequence_table_support as st

pytestmark = pytest.mark.gpu

PATTERN = 0xA5


@pytest.fixture(autouse=True)
def time_limit():
    """every test under a limit of its own: a pass that hangs ends the process instead of the session's time"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("ft-fsd-path-planning_amd")


@pytest.fixture(scope="module")
def rec():
    r = st.Recording()
    got = r.preconditions()
    assert all(got.values()), got
    return r


@pytest.fixture(scope="module")
def ctx(pkg, rec):
    c = pkg.Context(device=0)
    c.set_global_path_table(rec.paths)
    yield c
    c.close()


@pytest.fixture(scope="module")
def whole(ctx, rec):
    """the whole call, full records: (results, final_prev, n_replanned), held to the oracle by test_whole_call_*"""
    return ctx.plan_sequence(rec.off, rec.cones, rec.poses, rec.n, path_ids=rec.ids)


def same(a, b):
    """byte for byte, field by field (the bytes between the fields of a record are nobody's)"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.names:
        return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in a.dtype.names)
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def chained_submits(c, rec, ids, compact=False, initial_prev=None):
    """T lock-step Context.submit(prev_paths=, path_ids=) calls, planner i's prev row the path of its most recent successful step
    (sequence_support.lockstep's rule, with the step's ids) -> (records, final_prev, flagged frames that met a real path)"""
    n, T = rec.n, rec.T
    rows = c.shapes.path_points
    have = np.full((n, rows, 4), np.nan)
    if initial_prev is not None:
        have[:, : np.shape(initial_prev)[1]] = initial_prev
    default = c.default_path()
    out, again = [], 0
    for t in range(T):
        lo, hi = t * n, (t + 1) * n
        real = ~np.isnan(have[:, 0, 0])
        prev = np.where(real[:, None, None], have, default[None])
        r = c.collect(c.submit((rec.off[lo : hi + 1] - rec.off[lo]).astype(np.int32), rec.cones[rec.off[lo] : rec.off[hi]], rec.poses[lo:hi],
                               prev_paths=prev, path_ids=ids[lo:hi], compact=compact)).copy()
        if "path_fallback" in r.dtype.names:
            again += int((((r["path_fallback"] & ss.FB_READ_PREVIOUS) != 0) & real).sum())
        ok = r["status"] == 0
        have[ok] = r["path"][ok]
        out.append(r)
    return np.concatenate(out), have, again


# ---- 1. the whole call ----------------------------------------------------------------------------------------------------------
def test_whole_call_equals_the_stepped_oracle_and_the_chained_submits(ctx, rec, whole):
    res, final, again = whole
    names = ",".join(ctx.stage_names())
    assert "seq_mark_kernel,seq_chain_table_kernel,seq_final_kernel,assemble" in names and "path_table" in names, names
    ref, ref_final, ref_again, _ = rec.stepped()
    st.check(ref, res["status"], res["path"], res["path_fallback"], what="whole")
    assert final.tobytes() == ref_final.tobytes()
    assert again == ref_again and again > 0
    want, wfinal, wagain = chained_submits(ctx, rec, rec.ids)
    assert same(res, want) and same(final, wfinal) and again == wagain
    # compact records
    cres, cfinal, cagain = ctx.plan_sequence(rec.off, rec.cones, rec.poses, rec.n, path_ids=rec.ids, compact=True)
    cwant, _, _ = chained_submits(ctx, rec, rec.ids, compact=True)
    assert same(cres, cwant) and same(cfinal, final) and cagain == again
    st.check(ref, cres["status"], cres["path"], what="compact")
    # the plain call on the same context does not read the table
    plain = ctx.plan_sequence(rec.off, rec.cones, rec.poses, rec.n)[0]
    fresh = ctx.plan_sequence(rec.off, rec.cones, rec.poses, rec.n, path_ids=np.full(len(rec.ids), -1, np.int32))[0]
    assert same(plain, fresh) and not same(plain, res)


def test_initial_prev_rows_one_of_them_nan(ctx, rec, whole):
    init = np.stack([ctx.default_path()] * rec.n)
    init[:, :, 2] += 0.05 * (1 + np.arange(rec.n))[:, None]
    init[st.D] = np.nan
    res, final, again = ctx.plan_sequence(rec.off, rec.cones, rec.poses, rec.n, initial_prev=init, path_ids=rec.ids)
    ref, ref_final, ref_again, _ = rec.stepped(initial_prev=init)
    st.check(ref, res["status"], res["path"], res["path_fallback"], what="initial_prev")
    assert final.tobytes() == ref_final.tobytes() and again == ref_again
    assert not same(res, whole[0])


# ---- 2. planner slices, MultiPlanner ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("pin", [True, False])
def test_planner_slices_equal_the_rows_of_the_whole_call(pkg, ctx, rec, whole, pin, compact):
    want, wfinal, wagain = whole if not compact else ctx.plan_sequence(rec.off, rec.cones, rec.poses, rec.n, path_ids=rec.ids, compact=True)
    put = pkg.pinned_copy if pin else (lambda a, dtype=None: np.array(a, dtype=dtype))
    new = pkg.pinned_empty if pin else np.empty
    out = new(len(rec.poses), ctx.compact_dtype if compact else ctx.result_dtype)
    final = new((rec.n, ctx.shapes.path_points, 4), np.float64)
    out.view(np.uint8)[...] = PATTERN
    final.view(np.uint8)[...] = PATTERN
    o, x, p, ids = put(rec.off, np.int32), put(rec.cones), put(rec.poses), put(rec.ids, np.int32)
    again = 0
    for pair in (((0, 2), (2, 5)), ((5, 6),)):  # (two tickets per context in flight)
        tickets = [ctx.submit_sequence(o, x, p, hi - lo, compact=compact, planner_lo=lo, planners_total=rec.n, out=out, final_prev_out=final,
                                       path_ids=ids) for lo, hi in pair]
        for t in reversed(tickets):
            again += ctx.collect(t)[2]
    assert same(out, want) and same(final, wfinal) and again == wagain


def test_multi_planner_with_two_contexts(pkg, rec, whole):
    want, wfinal, wagain = whole
    mp = pkg.MultiPlanner(devices=[0, 0])
    try:
        mp.set_global_path_table(rec.paths)
        for pin in (False, True):
            arrays = (pkg.pinned_copy(rec.off, np.int32), pkg.pinned_copy(rec.cones), pkg.pinned_copy(rec.poses)) if pin else (rec.off, rec.cones, rec.poses)
            res, final, again = mp.plan_sequence(*arrays, rec.n, path_ids=rec.ids)
            assert same(np.asarray(res), want) and same(np.asarray(final), wfinal) and again == wagain
    finally:
        mp.close()


# ---- 3. continuation ----------------------------------------------------------------------------------------------------------------
def test_cut_after_step_three_and_joined_through_final_prev(ctx, rec, whole):
    want, wfinal, wagain = whole
    cut = 4 * rec.n  # (steps 0-3 | 4-7: inside the runs of (d), (e) and (f))
    a, afinal, aagain = ctx.plan_sequence(rec.off[: cut + 1], rec.cones, rec.poses[:cut], rec.n, path_ids=rec.ids[:cut])
    b, bfinal, bagain = ctx.plan_sequence(rec.off[cut:], rec.cones, rec.poses[cut:], rec.n, initial_prev=afinal, path_ids=rec.ids[cut:])
    assert same(np.concatenate([a, b]), want) and same(bfinal, wfinal) and aagain + bagain == wagain


# ---- 4. the rerun, tickets in flight ------------------------------------------------------------------------------------------------
def zigzag_ids(rec):
    """(c) follows ZIGZAG instead of ACC: first fits of more than 32 knots, frames only the retry route can plan"""
    ids = rec.ids.copy().reshape(rec.T, rec.n)
    ids[3:, st.C] = gts.ZIGZAG
    return np.ascontiguousarray(ids.reshape(-1))


def test_a_pass_that_lacks_its_retry_route_is_run_again_with_the_tickets_own_ids(pkg, rec):
    ids = zigzag_ids(rec)
    ref, ref_final, ref_again, _ = rec.stepped(ids=ids)
    out = {}
    for name, options in (("rerun", {"path_mode": 2, "pack": 2, "retry_pack_min": 1}), ("routed", {"path_mode": 2, "pack": 2, "retry_pack_min": 1, "always_route": 1})):
        c = pkg.Context(device=0, options=options)
        try:
            c.set_global_path_table(rec.paths)
            before = c.route_stats()[2]
            t = c.submit_sequence(rec.off, rec.cones, rec.poses, rec.n, path_ids=ids)
            other = c.submit_sequence(rec.off, rec.cones, rec.poses, rec.n, path_ids=np.full(len(ids), -1, np.int32))  # (other ids on the context meanwhile)
            res, final, again = c.collect(t)
            out[name] = (res.copy(), final.copy(), again)
            names = ",".join(c.stage_names())
            c.collect(other)
            assert c.route_stats()[2] - before >= (1 if name == "rerun" else 0), name
            if name == "routed":
                assert c.route_stats()[2] == before
            assert "path_table_retry_kernel" in names and "seq_chain_table_kernel" in names, names
        finally:
            c.close()
    assert same(out["rerun"][0], out["routed"][0]) and same(out["rerun"][1], out["routed"][1]) and out["rerun"][2] == out["routed"][2]
    res, final, again = out["rerun"]
    st.check(ref, res["status"], res["path"], res["path_fallback"], what="rerun")
    assert final.tobytes() == ref_final.tobytes() and again == ref_again
    assert (res["status"].reshape(rec.T, rec.n)[3:, st.C] == 0).all()


def test_two_sequence_tickets_with_different_ids_in_flight(ctx, rec, whole):
    other_ids = np.where(rec.ids == gts.ACC, gts.SKID, rec.ids).astype(np.int32)
    want_other = ctx.plan_sequence(rec.off, rec.cones, rec.poses, rec.n, path_ids=other_ids)
    ta = ctx.submit_sequence(rec.off, rec.cones, rec.poses, rec.n, path_ids=rec.ids)
    tb = ctx.submit_sequence(rec.off, rec.cones, rec.poses, rec.n, path_ids=other_ids)
    rb, fb, ab = ctx.collect(tb)
    ra, fa, aa = ctx.collect(ta)
    assert same(ra, whole[0]) and same(fa, whole[1]) and aa == whole[2]
    assert same(rb, want_other[0]) and same(fb, want_other[1]) and ab == want_other[2]
    assert not same(ra, rb)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_context_usable(pkg, rec, golden_dir):
    c = pkg.Context(device=0)
    args = (rec.off, rec.cones, rec.poses, rec.n)
    plain = c.plan_sequence(*args)

    def still_fine():
        r, f, a = c.plan_sequence(*args)
        assert same(r, plain[0]) and same(f, plain[1]) and a == plain[2]
        assert "seq_chain_kernel" in ",".join(c.stage_names())

    def refused(match, fn, *a, **kw):
        c.plan_sequence(*args)  # (the stage names of a pass that ran: a refused call must leave them alone)
        with pytest.raises(pkg.FsdpError, match=match):
            fn(*a, **kw)
        assert "seq_chain_kernel," in ",".join(c.stage_names())  # nothing was launched
        still_fine()

    # no table on the context
    refused("no path table", c.plan_sequence, *args, path_ids=rec.ids)
    refused("no path table", c.submit_sequence, *args, path_ids=rec.ids)
    c.set_global_path_table(rec.paths)
    # an id outside [-1, n_paths): the message names the frame by its index in the recording
    bad = rec.ids.copy()
    bad[3 * rec.n + 4] = len(rec.paths)
    refused(rf"path_ids\[{3 * rec.n + 4}\] = {len(rec.paths)} lies outside", c.plan_sequence, *args, path_ids=bad)
    refused(rf"path_ids\[{3 * rec.n + 4}\]", c.submit_sequence, rec.off, rec.cones, rec.poses, 3, planner_lo=2, planners_total=rec.n, path_ids=bad)
    bad[3 * rec.n + 4] = -2
    refused(rf"path_ids\[{3 * rec.n + 4}\] = -2", c.plan_sequence, *args, path_ids=bad)
    # ... and a slice reads its own planners' entries only
    r, f, a = c.collect(c.submit_sequence(rec.off, rec.cones, rec.poses, 2, planner_lo=0, planners_total=rec.n, path_ids=bad))
    want = c.plan_sequence(*args, path_ids=rec.ids)[0]
    rows = rec.slice_rows(0, 2)
    assert same(r[rows], want[rows])
    # path_ids NULL, through the ABI itself
    out, final, again = np.zeros(len(rec.poses), c.result_dtype), np.zeros((rec.n, c.shapes.path_points, 4)), ctypes.c_longlong(0)
    rc = c._lib.fsdp_plan_sequence_paths(c._h, rec.n, rec.T, rec.off.ctypes.data, rec.cones.ctypes.data, rec.poses.ctypes.data, None, None,
                                         out.ctypes.data, final.ctypes.data, ctypes.byref(again))
    assert rc == 1 and b"path_ids is NULL" in c._lib.fsdp_last_error(c._h)
    still_fine()
    # a device pointer
    dev = c._lib.fsdp_device_alloc(c._h, 4 * len(rec.ids))
    assert dev
    try:
        rc = c._lib.fsdp_plan_sequence_paths(c._h, rec.n, rec.T, rec.off.ctypes.data, rec.cones.ctypes.data, rec.poses.ctypes.data, None, dev,
                                             out.ctypes.data, final.ctypes.data, ctypes.byref(again))
        assert rc != 0 and b"path_ids" in c._lib.fsdp_last_error(c._h)
    finally:
        c._lib.fsdp_device_free(c._h, dev)
    still_fine()
    # the sorting cache on
    c.sort_cache_reset(rec.n)
    with pytest.raises(pkg.FsdpError, match="sorting cache"):
        c.plan_sequence(*args, path_ids=rec.ids)
    c.sort_cache_reset(0)
    still_fine()
    # a context-wide global path together with the table
    c.set_global_path(np.load(golden_dir / "global_path.npz")["gp_track"])
    with pytest.raises(pkg.FsdpError, match=r"also has a context-wide global path \(fsdp_set_global_path\)"):
        c.plan_sequence(*args, path_ids=rec.ids)
    with pytest.raises(pkg.FsdpError, match="context-wide global path"):
        c.submit_sequence(*args, path_ids=rec.ids)
    c.set_global_path(None)
    still_fine()
    # what fsdp_submit_sequence refuses: a slice outside the recording; a blocking call with tickets outstanding
    with pytest.raises(pkg.FsdpError, match="no slice of a recording"):
        c.submit_sequence(rec.off, rec.cones, rec.poses, 3, planner_lo=4, planners_total=rec.n, path_ids=rec.ids)
    t = c.submit_sequence(*args, path_ids=rec.ids)
    with pytest.raises(pkg.FsdpError, match="not collected"):
        c.plan_sequence(*args, path_ids=rec.ids)
    assert same(c.collect(t)[0], want)
    still_fine()
    c.close()
    # a skidpad context
    skid = pkg.Context(device=0, mission=int(pkg.MissionTypes.skidpad))
    try:
        with pytest.raises(pkg.FsdpError, match="skidpad"):
            skid.plan_sequence(*args, path_ids=rec.ids)
        with pytest.raises(pkg.FsdpError, match="skidpad"):
            skid.submit_sequence(*args, path_ids=rec.ids)
    finally:
        skid.close()


# ---- 6. AccelerationBatch.plan_sequence ---------------------------------------------------------------------------------------------
def acceleration_log(golden_dir, n):
    g = np.load(golden_dir / "global_path.npz")
    o = g["acc_offsets"]
    T = len(o) - 1
    per = [g["acc_cones"][o[t] : o[t + 1]] for t in range(T)]
    counts = np.array([len(per[t]) for t in range(T) for _ in range(n)])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    cones = np.concatenate([per[t] for t in range(T) for _ in range(n)])
    poses = np.repeat(g["acc_poses"], n, axis=0)
    return g, off, cones, poses, T


def test_acceleration_batch_plan_sequence_equals_thirty_steps(pkg, golden_dir):
    acc = importlib.import_module("ft-fsd-path-planning_amd.acceleration")
    n = 3
    g, off, cones, poses, T = acceleration_log(golden_dir, n)
    assert T == 30
    seeds = [int(g["acc_seed"]), int(g["acc_seed"]) + 1, 5]
    stepped, whole, cut = (acc.AccelerationBatch(n, pkg.MissionTypes.acceleration, seeds=seeds, device=0) for _ in range(3))
    try:
        want_p, want_s, first = [], [], np.full(n, T)
        for t in range(T):
            lo, hi = t * n, (t + 1) * n
            p, s = stepped.step(off[lo : hi + 1] - off[lo], cones[off[lo] : off[hi]], poses[lo:hi])
            want_p.append(p)
            want_s.append(s)
            first = np.where(stepped.relocalized & (first == T), t, first)
        want_p, want_s = np.array(want_p), np.array(want_s)
        assert 0 < first.min() and first.max() < T  # (ids of -1 and of 0 in the one call)
        paths, status = whole.plan_sequence(off, cones, poses)
        assert "seq_chain_table_kernel" in ",".join(whole._ctx.stage_names())
        assert paths.shape == want_p.shape and paths.tobytes() == want_p.tobytes() and np.array_equal(status, want_s)
        assert np.array_equal(whole.relocalized, stepped.relocalized) and whole.angles.tobytes() == stepped.angles.tobytes()
        assert (status[:, 0] == 0).all() and np.abs(paths[:, 0] - g["acc_path"]).max() < 1e-5  # (tests/test_global_path.py's tolerance)
        # 12 steps by plan_sequence, then 18 by step()
        k = 12 * n
        p0, s0 = cut.plan_sequence(off[: k + 1], cones[: off[k]], poses[:k])
        assert p0.tobytes() == want_p[:12].tobytes() and np.array_equal(s0, want_s[:12])
        for t in range(12, T):
            lo, hi = t * n, (t + 1) * n
            p, s = cut.step(off[lo : hi + 1] - off[lo], cones[off[lo] : off[hi]], poses[lo:hi])
            assert p.tobytes() == want_p[t].tobytes() and np.array_equal(s, want_s[t]), t
        assert np.array_equal(cut.relocalized, stepped.relocalized) and cut.angles.tobytes() == stepped.angles.tobytes()
    finally:
        for b in (stepped, whole, cut):
            b.close()


# ---- 7. the wide build --------------------------------------------------------------------------------------------------------------
def test_wide_build(pkg, rec, whole):
    c = pkg.Context(device=0, shapes=pkg.WIDE)
    try:
        c.set_global_path_table(rec.paths)
        res, final, again = c.plan_sequence(rec.off, rec.cones, rec.poses, rec.n, path_ids=rec.ids)
        assert "seq_chain_table_kernel" in ",".join(c.stage_names())
        import oracle_lib_wide

        ref, ref_final, ref_again, _ = rec.stepped(oracle=oracle_lib_wide)  # (the wide build's record shapes)
        st.check(ref, res["status"], res["path"], res["path_fallback"], what="wide", rows=c.horizon)
        assert final[:, : c.horizon].tobytes() == ref_final[:, : c.horizon].tobytes() and again == ref_again
        assert np.array_equal(res["status"], whole[0]["status"]) and same(res["path"][:, : c.horizon], whole[0]["path"][:, : c.horizon])
        want, wfinal, wagain = chained_submits(c, rec, rec.ids)
        assert same(res, want) and same(final, wfinal) and again == wagain
    finally:
        c.close()
