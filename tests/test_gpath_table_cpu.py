"""Per-frame global paths (fsdp_set_global_path_table / fsdp_submit_paths): the TABLE twins of the path stage's wrappers
(csrc/gpath_table_kernel.h) under the host SIMT emulator.  The lane groups of one wavefront hold different paths here — some enter
path_front's window loops, with different trip counts, some select_side_to_use — on every route form a pass with ids can take.
Expected values: the oracle with each frame's own path alone (tests/gpath_table_support.py), and the reference's golden recording."""
import numpy as np
import pytest

import gpath_table_support as gs


@pytest.fixture(scope="module")
def mixed():
    return gs.Mixed()


def test_the_mixed_batch_holds_what_it_is_built_for(mixed):
    """the pairs that share a wavefront (8 lanes per frame: frames 0-7 / 8-15; 16 lanes per frame and the retry form: fours), the
    sizes of the paths, and the statuses the oracle gives the frames"""
    ids, sizes = mixed.ids, [len(p) for p in mixed.paths]
    assert sizes[gs.ACC] == 1650 and 0 < sizes[gs.SHORT] < 8 and sizes[gs.ZERO] == 0 and sizes[gs.DENSE] > gs.PATH_CAP
    near = np.hypot(*(mixed.paths[gs.DENSE] - mixed.poses[7, :2]).T) < 30
    assert near.sum() > gs.PATH_CAP
    fours = [set(ids[k : k + 4]) for k in range(0, 16, 4)]
    assert any({gs.CONES, gs.ACC} <= s for s in fours) and any({gs.SHORT, gs.ACC} <= s for s in fours)
    assert all(len(fours[k // 4]) > 1 for k in np.nonzero(ids == gs.ZERO)[0])
    st = mixed.ref["status"]
    assert (st[ids == gs.ZERO] == gs.ST_REF_UNDEFINED_PATH).all()
    assert st[8] == gs.ST_REF_UNDEFINED_PATH and np.hypot(*(mixed.paths[gs.ACC] - mixed.poses[8, :2]).T).min() > 30
    assert (st[ids == gs.CONES] == 0).all() and (mixed.ref["path_fallback"][9] & 1) == 1  # frame 9: neither cones nor path
    assert st[[0, 1, 2, 3, 5, 6, 10, 11, 12, 13]].tolist() == [0] * 10


@pytest.mark.parametrize("form", list(gs.FORMS))
def test_mixed_batch_on_every_route_form_equals_the_oracle(mixed, form):
    status, out, retries = gs.emulate(form, mixed.off, mixed.cones, mixed.poses, mixed.prev, mixed.xy, mixed.path_off, mixed.ids)
    mixed.check(status, out["path"], what=form)
    if form == "retry":
        assert retries == mixed.n  # every frame through path_table_retry_kernel (retry_pack_min = 0: four frames per wavefront)
    if form == "prep8":
        assert retries < mixed.n // 2  # the packed kernels themselves planned the batch


@pytest.mark.parametrize("form", list(gs.FORMS))
def test_statuses_of_the_refused_frames_and_their_neighbours(mixed, form):
    """103 for the empty path and for a car more than 30 m from its path, 203 for the overfull path, 0 for the frames that share
    their wavefront — a fresh planner's history this time (no previous paths)"""
    ref = mixed.oracle(None)
    status, out, _ = gs.emulate(form, mixed.off, mixed.cones, mixed.poses, None, mixed.xy, mixed.path_off, mixed.ids)
    assert status[[4, 15]].tolist() == [gs.ST_REF_UNDEFINED_PATH] * 2 and status[8] == gs.ST_REF_UNDEFINED_PATH
    assert status[7] == gs.ST_OVERFLOW_PATH
    assert status[[5, 6]].tolist() == [0, 0] and status[[0, 1, 2, 3]].tolist() == [0] * 4 and status[[9, 10, 11, 12, 13]].tolist() == [0] * 5
    mixed.check(status, out["path"], ref=ref, what=form)


def test_ids_that_name_nothing_plan_from_the_cones(mixed):
    """the device form's rule (the host cannot read a device ticket's ids): an id outside [-1, n_paths) is planned as -1, and
    path_ids_scan_kernel names the lowest such frame"""
    ids = mixed.ids.copy()
    ids[[6, 13]] = [len(mixed.paths), -7]
    assert gs.ids_scan(ids, len(mixed.paths)) == 6 and gs.ids_scan(mixed.ids, len(mixed.paths)) == -1
    assert gs.ids_scan(np.full(1500, 2, np.int32), 3) == -1 and gs.ids_scan(np.r_[np.full(1499, 2), 3].astype(np.int32), 3) == 1499
    status, out, _ = gs.emulate("prep8", mixed.off, mixed.cones, mixed.poses, mixed.prev, mixed.xy, mixed.path_off, ids)
    mixed.check(status, out["path"], what="bad ids")  # (frames 6 and 13 plan from their cones anyway)


def test_frames_the_packed_kernels_hand_on_keep_their_paths():
    """the zigzag path's first fit needs more knots than the packed kernels keep: those frames reach path_table_retry_kernel through
    the device list, next to frames without a path, and come back as the oracle plans them"""
    rb = gs.RetryBatch()
    status, out, retries = gs.emulate("prep8", rb.off, rb.cones, rb.poses, None, rb.xy, rb.path_off, rb.ids)
    assert retries == int((rb.ids == gs.ZIGZAG).sum())
    assert (rb.ref["status"] == 0).all() and status.tolist() == [0] * rb.n
    assert out["path"].tobytes() == rb.ref["path"].tobytes()


@pytest.mark.parametrize("form", ["prep8", "mono16", "retry"])
def test_golden_recording_through_a_table(form):
    """tests/golden/global_path.npz: the reference's trackdrive planner with a global path, here as entry 2 of 3 — the golden bytes"""
    g = np.load(gs.GOLDEN / "global_path.npz")
    p = gs.paths()
    xy, path_off = gs.table([p[gs.SHORT], p[gs.ACC], p[gs.TRACK]])
    n = len(g["gp_poses"])
    prev = np.concatenate([gs.oracle_lib.default_path()[None], g["gp_path"][:-1]])  # the recording's own chain
    status, out, _ = gs.emulate(form, g["gp_offsets"], g["gp_cones"], g["gp_poses"], prev, xy, path_off, np.full(n, 2, np.int32))
    assert (status == 0).all()
    assert out["path"].tobytes() == np.ascontiguousarray(g["gp_path"]).tobytes()
