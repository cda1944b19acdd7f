"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI
(libfsdp_hip.so via ctypes), against (a) the committed golden vectors captured from the reference
and (b) the CPU oracle on the same seeded inputs, plus size-independent properties at the full
BASELINE batch sizes."""
import collections
import importlib
import os

import numpy as np
import pytest

import oracle_lib
import parity

pytestmark = pytest.mark.gpu

# big_frames: 300 / 600 cones per frame; lattice: up to 190 end configurations per side (beyond the LDS capacities of
# the product sorting kernel: planned by sort_big_kernel)
SETS = ["scenarios", "cfg2_color", "cfg3_nocolor", "cfg4_200cones", "cfg4_noisy_nocolor", "fuzz", "big_frames", "lattice"]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("ft-fsd-path-planning_amd")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(device=0, mission=int(pkg.MissionTypes.trackdrive))
    yield c
    c.close()


def _as_oracle_rows(res):
    out = np.zeros(len(res), oracle_lib.RESULT_DTYPE)
    for k in oracle_lib.RESULT_DTYPE.names:
        out[k] = res[k]
    return out


def test_default_previous_path_matches_reference(ctx, golden_dir):
    ref = np.load(golden_dir / "default_path.npz")["path"]
    assert np.abs(ctx.default_path() - ref).max() < 1e-12


@pytest.mark.parametrize("name", SETS + ["nonfinite_poses", "nonfinite_cones", "odd_inputs"])
def test_hip_matches_reference_golden(ctx, golden_dir, name):
    """Bar: sorted index arrays bit-equal, matching outputs bit-equal, path within 1e-5 (tests/parity.py)."""
    g = np.load(golden_dir / f"{name}.npz")
    res = _as_oracle_rows(ctx.plan_batch(g["offsets"], g["cones"], g["poses"]))
    cats = collections.Counter()
    bad, n_arc = [], 0
    arc = parity.ArcLibm(golden_dir, name)
    for k in range(len(res)):
        cat, detail = parity.compare_frame(res[k], g, k, arc=arc)
        cats[cat] += 1
        n_arc += bool(int(res[k]["path_fallback"]) & parity.ARC_FLAG)
        if cat in ("IDX", "MATCH", "PATH", "STATUS"):
            bad.append((k, cat, detail))
    assert not bad, bad[:5]
    # arc frames: within 1e-5 of the reference at the libm level (compare_frame); a difference from the AVX-512 golden exactly
    # on the frames on which the reference differs from itself (fuzz: 339 and 347), nowhere else
    assert n_arc == len(arc.frames) and cats["flip"] == len(arc.flips("det")), (cats, n_arc, arc.flips("det"))


@pytest.mark.parametrize("name", SETS + ["nonfinite_poses", "nonfinite_cones", "odd_inputs"])
def test_hip_matches_oracle_on_golden_inputs(ctx, golden_dir, name):
    g = np.load(golden_dir / f"{name}.npz")
    res = ctx.plan_batch(g["offsets"], g["cones"], g["poses"])
    with oracle_lib.math_mode(1):
        ref = oracle_lib.plan_batch(g["offsets"], g["cones"], g["poses"], n_threads=os.cpu_count() or 1)
    _assert_equal_to_oracle(res, ref)


def _assert_equal_to_oracle(res, ref):
    """Against the oracle in det-math mode (the kernels use det_math.h for the arc extension): every
    discrete output equal, and the path bit-identical — the float chain holds no libm value."""
    assert np.array_equal(res["status"], ref["status"])
    ok = ref["status"] == 0
    for f in ("n_left", "n_right", "left_idx", "right_idx", "n_left_v", "n_right_v", "l2r", "r2l"):
        assert np.array_equal(res[f][ok], ref[f][ok]), f
    parity.assert_intermediates_equal(res, ref, ok, cost_rtol=1e-12)  # start cones, end configurations after the post-filters, best cost
    assert np.array_equal(res["left_v"][ok], ref["left_v"][ok])
    assert np.array_equal(res["right_v"][ok], ref["right_v"][ok])
    assert np.array_equal(res["path_fallback"][ok], ref["path_fallback"][ok])
    assert np.array_equal(np.isnan(res["path"][ok]), np.isnan(ref["path"][ok]))  # (rows beyond a shorter horizon: NaN on both sides)
    err = np.nan_to_num(np.abs(res["path"][ok] - ref["path"][ok]), nan=0.0).reshape(ok.sum(), -1).max(axis=1) if ok.any() else np.zeros(0)
    assert (err <= 1e-9).all(), (float(err.max()), int((err > 1e-9).sum()))


@pytest.mark.parametrize("cfg", ["cfg2", "cfg2_packed", "cfg3", "cfg4"])
def test_full_size_batches_against_oracle(pkg, ctx, cfg, monkeypatch):
    """BASELINE configs 2/3 at the full 4096 frames and config 4's per-GPU shard shape (8192 x 200 cones):
    every frame against the oracle (all host cores).  cfg2_packed: the 8-lane kernels bench.py's overlapped passes run
    (a single pass would get the 16-lane ones)."""
    if cfg == "cfg2_packed":
        ctx = pkg.Context(device=0, options={"pack": 2})
        cfg = "cfg2"
    if cfg == "cfg2":
        off, cones, poses = pkg.synth.make_replay_batch(4096, 64, 0.15, seed=1, color=True)
    elif cfg == "cfg3":
        off, cones, poses = pkg.synth.make_replay_batch(4096, 64, 0.15, seed=1, color=False)
    else:
        off, cones, poses = pkg.synth.make_config4_shard(0, 8192, 100, 0.1, seed=7)  # one GPU's shard of the 65 536 frames
    res = ctx.plan_batch(off, cones, poses)
    with oracle_lib.math_mode(1):
        ref = oracle_lib.plan_batch(off, cones, poses, n_threads=os.cpu_count() or 1)
    _assert_equal_to_oracle(res, ref)
    assert (res["status"] == 0).mean() > 0.95


def test_config4_every_shard_against_oracle(pkg, ctx):
    """BASELINE config 4 is 65 536 frames in eight contiguous shards of 8192 (one per GPU).  Shard 0 is planned in full above;
    here 512 frames from the START and the END of every one of the eight shards — frames [g 8192, g 8192 + 256) and
    [(g + 1) 8192 - 256, (g + 1) 8192) — are planned on the GPU, as ONE batch in shard order, against the oracle (round-4
    review: shards 1-7 had never been planned on hardware)."""
    parts = []
    for g in range(8):
        parts.append(pkg.synth.make_config4_shard(g * 8192, g * 8192 + 256, 100, 0.1, seed=7))
        parts.append(pkg.synth.make_config4_shard((g + 1) * 8192 - 256, (g + 1) * 8192, 100, 0.1, seed=7))
    counts = np.concatenate([np.diff(o) for o, _, _ in parts])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    cones = np.concatenate([c for _, c, _ in parts])
    poses = np.concatenate([p for _, _, p in parts])
    assert len(poses) == 4096 and (counts == 200).all()
    res = ctx.plan_batch(off, cones, poses)
    with oracle_lib.math_mode(1):
        ref = oracle_lib.plan_batch(off, cones, poses, n_threads=os.cpu_count() or 1)
    _assert_equal_to_oracle(res, ref)
    assert (res["status"] == 0).mean() > 0.95


def test_batch_properties(pkg, ctx):
    """Size-independent properties at full batch size: determinism, independence of frames from batch
    composition (permutation / split), and geometric sanity of the outputs."""
    off, cones, poses = pkg.synth.make_replay_batch(4096, 64, 0.15, seed=3, color=True)
    a = ctx.plan_batch(off, cones, poses)
    b = ctx.plan_batch(off, cones, poses)
    assert a.tobytes() == b.tobytes()
    # permute frames
    rng = np.random.default_rng(0)
    perm = rng.permutation(4096)
    cones_p = np.concatenate([cones[off[i] : off[i + 1]] for i in perm])
    off_p = np.concatenate([[0], np.cumsum([off[i + 1] - off[i] for i in perm])]).astype(np.int32)
    c = ctx.plan_batch(off_p, cones_p, poses[perm])
    for f in a.dtype.names:  # (field-wise: fancy indexing of a padded structured dtype does not carry the padding bytes)
        assert np.ascontiguousarray(c[f]).tobytes() == np.ascontiguousarray(a[f][perm]).tobytes(), f"field {f} depends on the frame order"
    # split
    h = 1500
    d1 = ctx.plan_batch(off[: h + 1], cones[: off[h]], poses[:h])
    d2 = ctx.plan_batch(off[h:] - off[h], cones[off[h] :], poses[h:])
    # (field-wise: np.concatenate of a padded structured dtype does not carry the padding bytes)
    for lo, part in ((0, d1), (h, d2)):
        ref = a[lo : lo + len(part)]
        for f in part.dtype.names:
            x, y = np.ascontiguousarray(part[f]), np.ascontiguousarray(ref[f])
            assert x.tobytes() == y.tobytes(), f"field {f} depends on the batch composition (frames from {lo})"
    ok = a["status"] == 0
    assert ok.mean() > 0.99
    p = a["path"][ok]
    # arc-length parameter strictly increasing, starts at 0, path starts near the car, ~20 m long
    assert (np.diff(p[:, :, 0], axis=1) > 0).all() and (p[:, 0, 0] == 0).all()
    assert (np.linalg.norm(p[:, 0, 1:3] - poses[ok, :2], axis=1) < 2.0).all()
    assert ((p[:, -1, 0] > 18.0) & (p[:, -1, 0] < 21.0)).all()
    # sorted indices are valid, unique per side, coloured correctly
    for side, t in (("left_idx", 2), ("right_idx", 1)):
        idx = a[side][ok]
        valid = idx >= 0
        assert (idx[valid] < 128).all()
        assert (np.sort(np.where(valid, idx, 1000 + np.arange(12)), axis=1)[:, 1:] != np.sort(np.where(valid, idx, 1000 + np.arange(12)), axis=1)[:, :-1]).all()


def test_reference_shaped_single_frame_call(pkg, golden_dir):
    """PathPlanner.calculate_path_in_global_frame keeps the reference's signature / return tuple."""
    g = np.load(golden_dir / "scenarios.npz")
    planner = pkg.PathPlanner(pkg.MissionTypes.trackdrive, device=0)
    for k in range(len(g["ok"])):
        xyt = g["cones"][g["offsets"][k] : g["offsets"][k + 1]]
        cones_by_type = [xyt[xyt[:, 2] == t, :2] for t in range(5)]
        # list-of-5 input only preserves the index space when the frame is stored type-sorted
        if not (np.diff(xyt[:, 2]) >= 0).all():
            cones_by_type = xyt
        pose = g["poses"][k]
        out = planner.calculate_path_in_global_frame(cones_by_type, pose[:2], pose[2:], return_intermediate_results=True)
        path, sl, sr, lv, rv, l2r, r2l = out
        assert path.shape == (40, 4)
        nl, nr = g["n_left"][k], g["n_right"][k]
        assert np.array_equal(sl, xyt[g["left_idx"][k][:nl], :2]) and np.array_equal(sr, xyt[g["right_idx"][k][:nr], :2])
        assert np.array_equal(l2r, g["l2r"][k][: len(l2r)]) and np.array_equal(r2l, g["r2l"][k][: len(r2l)])
        only_path = planner.calculate_path_in_global_frame(cones_by_type, pose[:2], float(np.arctan2(pose[3], pose[2])))
        assert only_path.shape == (40, 4)


def test_edge_cases(pkg, ctx):
    # empty batch, empty frames, < 3 cones, 300 random cones, track frames of 1400 coloured / 3000 colourless cones (beyond
    # the LDS kernel: planned with the state in global memory), more cones than the library takes at all (status 201, no
    # silent truncation)
    assert len(ctx.plan_batch(np.zeros(1, np.int32), np.zeros((0, 3)), np.zeros((0, 4)))) == 0
    rng = np.random.default_rng(0)
    o1, c1, p1 = pkg.synth.make_replay_batch(1, 700, 0.1, seed=3, color=True)
    o2, c2, p2 = pkg.synth.make_replay_batch(1, 1500, 0.1, seed=3, color=False)
    blocks = [np.zeros((0, 3)), np.array([[2.0, 1.5, 2]]), np.array([[2.0, 1.5, 2], [2.0, -1.5, 1]]),
              np.column_stack([rng.uniform(-30, 30, (300, 2)), np.zeros(300)]), c1, c2,
              np.column_stack([rng.uniform(-150, 150, (8300, 2)), np.zeros(8300)])]
    off = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int32)
    cones = np.concatenate(blocks)
    poses = np.tile(np.array([0.0, 0, 1, 0]), (len(blocks), 1))
    poses[4], poses[5] = p1[0], p2[0]
    r = ctx.plan_batch(off, cones, poses)
    with oracle_lib.math_mode(1):
        ref = oracle_lib.plan_batch(off[:7], cones[: off[6]], poses[:6])
    assert (r["status"][:3] == 0).all() and r["status"][6] == 201
    for k in (3, 4, 5):
        assert r["status"][k] == ref["status"][k]
        assert np.array_equal(r["left_idx"][k], ref["left_idx"][k]) and np.array_equal(r["right_idx"][k], ref["right_idx"][k]), k
    assert r["n_left"][4] >= 10 and r["n_right"][4] >= 10 and r["n_left"][5] >= 8  # the big frames really are planned
    ok = ref["status"] == 0
    assert np.array_equal(np.isnan(r["path"][:6][ok]), np.isnan(ref["path"][ok]))
    assert np.nanmax(np.abs(r["path"][:6][ok] - ref["path"][ok])) < 1e-9
    assert (r["n_left"][:3] == 0).all() and (r["path_fallback"][:3] & 1).all()


def test_stage_entry_points(pkg, ctx, golden_dir):
    """ConeSorting / ConeMatching / CalculatePath stage-level C-ABI entry points agree with the fused call."""
    g = np.load(golden_dir / "cfg2_color.npz")
    full = ctx.plan_batch(g["offsets"], g["cones"], g["poses"])
    s = ctx.sort_batch(g["offsets"], g["cones"], g["poses"])
    assert np.array_equal(s["left_idx"], full["left_idx"]) and np.array_equal(s["right_idx"], full["right_idx"])
    F = len(full)
    sl = np.zeros((F, 12, 2))
    sr = np.zeros((F, 12, 2))
    for k in range(F):
        xyt = g["cones"][g["offsets"][k] : g["offsets"][k + 1]]
        sl[k, : full["n_left"][k]] = xyt[full["left_idx"][k][: full["n_left"][k]], :2]
        sr[k, : full["n_right"][k]] = xyt[full["right_idx"][k][: full["n_right"][k]], :2]
    m = ctx.match_batch(sl, full["n_left"], sr, full["n_right"], g["poses"])
    for f in ("n_left_v", "n_right_v", "left_v", "right_v", "l2r", "r2l"):
        assert np.array_equal(m[f], full[f]), f
    p = ctx.path_batch(g["poses"], m.copy())
    assert np.array_equal(p["path"], full["path"])


def test_stage_classes_mirror_reference_protocol(pkg, golden_dir):
    """ConeSorting / ConeMatching / CalculatePath with set_new_input -> run_* (README.md:78-79 of the reference)."""
    g = np.load(golden_dir / "scenarios.npz")
    for k in (2, 9, 12):
        xyt = g["cones"][g["offsets"][k] : g["offsets"][k + 1]]
        pose = g["poses"][k]
        cs = pkg.ConeSorting(max_n_neighbors=5, max_dist=6.5, max_length=12)
        cs.set_new_input(pkg.ConeSortingInput(xyt, pose[:2], pose[2:]))
        sl, sr = cs.run_cone_sorting()
        nl, nr = g["n_left"][k], g["n_right"][k]
        assert np.array_equal(sl, xyt[g["left_idx"][k][:nl], :2]) and np.array_equal(sr, xyt[g["right_idx"][k][:nr], :2])
        cm = pkg.ConeMatching(min_track_width=3, matches_should_be_monotonic=False)
        sc = [np.zeros((0, 2)) for _ in range(5)]
        sc[int(pkg.ConeTypes.LEFT)], sc[int(pkg.ConeTypes.RIGHT)] = sl, sr
        cm.set_new_input(pkg.ConeMatchingInput(sc, pose[:2], pose[2:]))
        lv, rv, l2r, r2l = cm.run_cone_matching()
        ml, mr = g["n_left_v"][k], g["n_right_v"][k]
        assert np.array_equal(lv, g["left_v"][k][:ml]) and np.array_equal(rv, g["right_v"][k][:mr])
        assert np.array_equal(l2r, g["l2r"][k][:ml]) and np.array_equal(r2l, g["r2l"][k][:mr])
        cp = pkg.CalculatePath(smoothing=0.2, mpc_path_length=20)
        cp.set_new_input(pkg.PathCalculationInput(lv, rv, l2r, r2l, pose[:2], pose[2:]))
        path, _ = cp.run_path_calculation()
        assert np.abs(path - g["path"][k]).max() < 1e-5 or parity.is_sample_count_flip(path, g["path"][k])
    # other values travel to the kernels as the context's parameter block (test_non_default_parameters); what the
    # kernels cannot take is refused when the context is created
    pkg.ConeSorting(max_dist=7.0)
    with pytest.raises(TypeError):
        pkg.ConeSorting(no_such_kwarg=1)
    cs = pkg.ConeSorting(max_n_neighbors=7)  # beyond the standard shapes: carried by the wide build (round 5)
    cs.set_new_input(pkg.ConeSortingInput(xyt, pose[:2], pose[2:]))
    assert len(cs.run_cone_sorting()) == 2
    with pytest.raises(pkg.FsdpError):
        cs = pkg.ConeSorting(max_n_neighbors=9)
        cs.set_new_input(pkg.ConeSortingInput(xyt, pose[:2], pose[2:]))
        cs.run_cone_sorting()


def test_calculate_path_stage_returns_the_centre_points(pkg, golden_dir):
    """CalculatePath.run_path_calculation returns (path, center_along_match_connection) like the reference
    (core_calculate_path.py:575).  156 captures of the reference's own stage object (tests/golden/make_golden.py
    --stage-centers-only): centres of the matched pairs, the previous path's xy (fewer than two matches / fewer than three
    cones on both sides), the rolled slice of a global path within 30 m.  The centre points are plain (a + b) / 2 of the
    inputs or copies: bit-equal; the path within 1e-5 (arc frames: the counted sample-count flip)."""
    g = np.load(golden_dir / "stage_centers.npz")
    flips = []
    seen = set()
    for k in range(len(g["ok"])):
        assert g["ok"][k]
        nl, nr = int(g["n_left_v"][k]), int(g["n_right_v"][k])
        cp = pkg.CalculatePath(device=0, stateful=False)
        gp = g["global_path"] if g["uses_global"][k] else None
        cp.set_new_input(pkg.PathCalculationInput(g["left_v"][k, :nl], g["right_v"][k, :nr], g["l2r"][k, :nl], g["r2l"][k, :nr],
                                                  g["poses"][k, :2], g["poses"][k, 2:], gp))
        path, centers = cp.run_path_calculation()
        n = int(g["n_centers"][k])
        assert centers.shape == (n, 2), (k, centers.shape, n)
        assert np.array_equal(centers, g["centers"][k, :n]), k
        seen.add("global" if gp is not None else ("previous" if n == 40 else "matches"))
        e = np.abs(path - g["path"][k]).max()
        if e > 1e-5:
            assert parity.is_sample_count_flip(path, g["path"][k]) and int(cp.last_result["path_fallback"]) & parity.ARC_FLAG, (k, e)
            flips.append(k)
    assert seen == {"global", "previous", "matches"}
    assert len(flips) <= 2, flips


def test_replay_cli_roundtrip(pkg, golden_dir, tmp_path):
    import json

    g = np.load(golden_dir / "cfg2_color.npz")
    frames = []
    for t in range(16):
        xyt = g["cones"][g["offsets"][t] : g["offsets"][t + 1]]
        frames.append({"car_position": g["poses"][t, :2].tolist(), "car_direction": g["poses"][t, 2:].tolist(),
                       "slam_cones": [xyt[xyt[:, 2] == k, :2].tolist() for k in range(5)]})
    f = tmp_path / "replay.json"
    f.write_text(json.dumps(frames))
    pos, dirs, obs = pkg.replay.load_data_json(f)
    paths, times, reloc, info = pkg.replay.replay_per_frame(pkg.MissionTypes.trackdrive, pos, dirs, obs, device=0)
    res, sec = pkg.replay.replay_batched(pkg.MissionTypes.trackdrive, pos, dirs, obs, device=0, repeats=1, batch_frames=5, depth=3)
    assert np.array_equal(paths, res["path"]) and reloc is None and info is None
    assert np.abs(paths - g["path"][:16]).max() < 1e-5
    # the same stream sharded over two contexts from this process (replay --devices 0,0): the same bytes
    multi, _ = pkg.replay.replay_batched(pkg.MissionTypes.trackdrive, pos, dirs, obs, repeats=1, batch_frames=5, depth=3, devices=[0, 0])
    assert all(np.ascontiguousarray(multi[k]).tobytes() == np.ascontiguousarray(res[k]).tobytes() for k in res.dtype.names)  # (field by field: the records' padding is nobody's)


def test_stateful_batched_replay_equals_per_frame_replay(pkg, golden_dir, tmp_path):
    """replay_stateful_batched: a recording whose frames 0, 7, 8, 9 and 20 show the planner fewer than three cones per
    side (the reference falls back to previous_paths[-1], core_calculate_path.py:531-536 — frames 8 and 9 to a path that was
    itself a fall-back) must give the per-frame replay's paths, bit for bit: batched first, the frames that read the
    previous path again in order."""
    import json

    g = np.load(golden_dir / "cfg2_color.npz")
    frames = []
    for t in range(32):
        xyt = g["cones"][g["offsets"][t] : g["offsets"][t + 1]]
        if t in (0, 7, 8, 9, 20):
            xyt = xyt[:2]
        frames.append({"car_position": g["poses"][t, :2].tolist(), "car_direction": g["poses"][t, 2:].tolist(),
                       "slam_cones": [xyt[xyt[:, 2] == k, :2].tolist() for k in range(5)]})
    f = tmp_path / "replay.json"
    f.write_text(json.dumps(frames))
    pos, dirs, obs = pkg.replay.load_data_json(f)
    paths, times, reloc, info = pkg.replay.replay_per_frame(pkg.MissionTypes.trackdrive, pos, dirs, obs, device=0)
    res, sec, again = pkg.replay.replay_stateful_batched(pkg.MissionTypes.trackdrive, pos, dirs, obs, device=0, batch_frames=8, depth=3)
    assert again == 4  # (frame 0 meets the fresh planner's path in both replays)
    assert (res["status"] == 0).all() and np.array_equal(paths, res["path"])
    independent, _ = pkg.replay.replay_batched(pkg.MissionTypes.trackdrive, pos, dirs, obs, device=0, repeats=1, batch_frames=8, depth=3)
    assert not np.array_equal(independent["path"][8], res["path"][8])  # (the chain matters)


def test_twenty_passes_in_flight_equal_a_serial_pass(pkg):
    """bench.py's depth: fsdp_set_overlap(20), twenty passes over the resident 4096-frame batch enqueued back to back on twenty
    streams (fsdp_time_runs), then twenty more by fsdp_run — the results every slot holds are the bytes of one serial pass
    (round-4 review: the bench's depth had no equality test; the others use 2 ... 10)."""
    off, cones, poses = pkg.synth.make_replay_batch(4096, 64, 0.15, seed=1, color=True)
    ctx = pkg.Context(device=0)
    ref = ctx.plan_batch(off, cones, poses)
    ctx.set_overlap(20)
    ctx.upload(off, cones, poses)
    ctx.time_reserve(20)
    ctx.time_detail(False)
    assert ctx.time_runs(20, collect=False) is None
    ctx.sync()
    names = ctx.stage_names()
    assert "fit_kernel<4>" in names, names  # (the packed kernels: 81 920 frames in flight)
    for k in range(20):  # the last pass lands in a different slot every time: every slot's result block is checked
        got = ctx.download()
        for f in got.dtype.names:
            assert np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(ref[f]).tobytes(), (k, f)
        ctx.run()
    ctx.sync()
    # and as a stream of twenty different batches through the same twenty slots
    batches = [pkg.synth.make_replay_batch(1100 + 37 * k, 64, 0.15, seed=40 + k, color=bool(k % 2)) for k in range(20)]
    refs = [ctx2.plan_batch(*b) for ctx2 in [pkg.Context(device=0)] for b in batches]
    pinned = [(pkg.pinned_copy(o, np.int32), pkg.pinned_copy(c), pkg.pinned_copy(p)) for o, c, p in batches]
    tickets = [ctx.submit(*b) for b in pinned]
    for k, t in enumerate(tickets):
        got = ctx.collect(t)
        for f in got.dtype.names:
            assert np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(refs[k][f]).tobytes(), (k, f)


def test_overlapped_passes_equal_serial_passes(pkg):
    """fsdp_set_overlap(2): consecutive passes alternate between two streams / buffer sets.  Every pass must return
    exactly what a single serial pass returns, whichever slot it ran in, also after a new upload."""
    off, cones, poses = pkg.synth.make_replay_batch(1024, 64, 0.15, seed=11, color=True)
    ctx = pkg.Context(device=0)
    ref = ctx.plan_batch(off, cones, poses)
    ctx.set_overlap(2)
    ctx.upload(off, cones, poses)
    for n_runs in (1, 2, 3, 6):  # last pass lands in slot 0 / 1 alternately
        for _ in range(n_runs):
            ctx.run()
        got = ctx.download()
        for f in got.dtype.names:
            assert np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(ref[f]).tobytes(), (n_runs, f)
    tot, st = ctx.time_runs(5)
    assert tot > 0 and all(x > 0 for x in st)
    got = ctx.download()
    assert got["path"].tobytes() == ref["path"].tobytes()
    # the timed region in three steps (events created before, read after: what bench.py puts its wall clock around);
    # a deeper overlap than passes run so far: fsdp_time_reserve runs one pass on the slots that have not run yet
    ctx.set_overlap(5)
    ctx.time_reserve(7)
    assert ctx.time_runs(7, collect=False) is None
    tot3, st3 = ctx.time_results()
    assert tot3 > 0 and len(st3) == len(ctx.stage_names()) and all(x > 0 for x in st3)
    assert ctx.time_results() == (tot3, st3)  # reading twice is harmless
    got = ctx.download()
    assert got["path"].tobytes() == ref["path"].tobytes()
    # events only around the path stage's main kernel (what bench.py's timed region records): the other kernels read 0
    ctx.time_detail(False)
    assert ctx.time_runs(7, collect=False) is None
    tot4, st4 = ctx.time_results()
    main = [n.startswith(("fit_kernel", "path_kernel<64>")) for n in ctx.stage_names()]
    assert tot4 > 0 and sum(main) == 1 and st4[main.index(True)] > 0 and st4[0] == 0 and st4[1] == 0, (ctx.stage_names(), st4)
    assert ctx.download()["path"].tobytes() == ref["path"].tobytes()
    # the refit kernel by its own clock (first wavefront's start to last wavefront's end of every launch): all seven launches
    # are covered, and the duration lies inside the event bracket (which starts when the previous kernel of the stream ends)
    # — opt-in (advisor, round 4: the readings are atomics inside the kernel; a region timed without them runs the production launches)
    assert ctx.time_kernel_clock() == (0.0, 0)
    ctx.time_detail(False, kernel_clock=True)
    assert ctx.time_runs(7, collect=False) is None
    tot5, st5 = ctx.time_results()
    kms, kn = ctx.time_kernel_clock()
    fit = [n.startswith("fit_kernel") for n in ctx.stage_names()]
    if any(fit):
        assert kn == 7 and 0 < kms <= st5[fit.index(True)] * 1.05, (kms, kn, st5)
    else:
        assert kn == 0 and kms == 0.0
    assert ctx.download()["path"].tobytes() == ref["path"].tobytes()
    ctx.time_detail(True, kernel_clock=True)
    assert all(x > 0 for x in ctx.time_runs(3)[1])
    assert ctx.time_kernel_clock()[1] == (3 if any(fit) else 0)
    ctx.time_detail(True)
    assert all(x > 0 for x in ctx.time_runs(3)[1])
    assert ctx.time_kernel_clock()[1] == 0
    ctx.set_overlap(2)
    # a different batch through the same overlapped context
    off2, cones2, poses2 = pkg.synth.make_replay_batch(700, 64, 0.15, seed=12, color=False)
    ref2 = pkg.Context(device=0).plan_batch(off2, cones2, poses2)
    got2 = ctx.plan_batch(off2, cones2, poses2)
    assert got2["path"].tobytes() == ref2["path"].tobytes() and (got2["status"] == ref2["status"]).all()
    ctx.set_overlap(1)
    assert ctx.plan_batch(off, cones, poses)["path"].tobytes() == ref["path"].tobytes()


@pytest.mark.parametrize("mode", ["mono64", "split16", "packed8", "packed8_fit4"])
def test_every_path_kernel_instantiation_equals_oracle(pkg, mode):
    """The library picks the path-stage kernels from the batch size and the passes in flight (fsdp_lib.hip launch_path):
    one kernel with 64 lanes per frame, or prep / fit / finish with 16 lanes per frame, or the packed ones (8 lanes per
    frame; the fit kernel optionally 4) that bench.py's overlapped passes run.  fsdp_set_option pins the choice; every
    instantiation must reproduce the oracle bit for bit."""
    options = {"mono64": {"path_mode": 1}, "split16": {"path_mode": 2, "pack": 1},
               "packed8": {"path_mode": 2, "pack": 2, "fit_g": 8}, "packed8_fit4": {"path_mode": 2, "pack": 2, "fit_g": 4}}[mode]
    ctx = pkg.Context(device=0, options=options)
    off, cones, poses = pkg.synth.make_replay_batch(300, 64, 0.15, seed=21, color=True)
    off2, cones2, poses2 = pkg.synth.make_replay_batch(211, 100, 0.0, seed=22, frame_noise=0.3, random_pose=True, color=False)
    for o, c, p in ((off, cones, poses), (off2, cones2, poses2)):
        res = ctx.plan_batch(o, c, p)
        with oracle_lib.math_mode(1):
            ref = oracle_lib.plan_batch(o, c, p, n_threads=os.cpu_count() or 1)
        _assert_equal_to_oracle(res, ref)
    names = ctx.stage_names()
    want = {"mono64": "path_kernel<64>", "split16": "fit_kernel<16>", "packed8": "fit_kernel<8>", "packed8_fit4": "fit_kernel<4>"}[mode]
    assert want in names, names
    assert ("path_prep_kernel<8>" in names) == mode.startswith("packed"), names


def test_both_sorting_state_sizes_equal_oracle(pkg):
    """A batch whose frames hold at most 128 cones is sorted by sort_kernel_128 (half-size frame state, four wavefronts per
    SIMD), any other batch by sort_kernel (255 cones): same results from both, equal to the oracle."""
    off, cones, poses = pkg.synth.make_replay_batch(512, 64, 0.15, seed=31, color=True)
    off2, cones2, poses2 = pkg.synth.make_replay_batch(256, 60, 0.0, seed=32, frame_noise=0.3, random_pose=True, color=False)
    with oracle_lib.math_mode(1):
        refs = [oracle_lib.plan_batch(o, c, p, n_threads=os.cpu_count() or 1) for o, c, p in ((off, cones, poses), (off2, cones2, poses2))]
    ctx = pkg.Context(device=0)
    small = [ctx.plan_batch(o, c, p) for o, c, p in ((off, cones, poses), (off2, cones2, poses2))]
    assert "sort_kernel_128" in ctx.stage_names()
    ctx2 = pkg.Context(device=0, options={"no_sort128": 1})
    large = [ctx2.plan_batch(o, c, p) for o, c, p in ((off, cones, poses), (off2, cones2, poses2))]
    assert "sort_kernel_128" not in ctx2.stage_names()
    for a, b, ref in zip(small, large, refs):
        _assert_equal_to_oracle(a, ref)
        for f in a.dtype.names:
            assert a[f].tobytes() == b[f].tobytes(), f
    # 129 cones in one frame of the batch: the library takes the 255-cone kernel by itself
    off3, cones3, poses3 = pkg.synth.make_replay_batch(8, 65, 0.15, seed=33, color=True)
    ctx3 = pkg.Context(device=0)
    res3 = ctx3.plan_batch(off3, cones3, poses3)
    assert "sort_kernel_128" not in ctx3.stage_names()
    with oracle_lib.math_mode(1):
        _assert_equal_to_oracle(res3, oracle_lib.plan_batch(off3, cones3, poses3))


def test_rccl_single_rank_communicator(pkg, monkeypatch):
    """fsdp_comm_* (RCCL behind the C ABI, no PyTorch): a one-rank communicator on this GPU — unique id, ncclCommInitRank,
    ncclCommCount, broadcast of the skidpad track table, all-reduce, barrier.  N > 1 differs only in the rank count."""
    import sys

    monkeypatch.setenv("FSDP_FORCE_DIST", "1")
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    c = pkg.Context(device=0, mission=int(pkg.MissionTypes.trackdrive))
    d = pkg.dist.Dist(c)
    assert d._active and d.comm_size == 1 and d.transport == "rccl"
    table = pkg.skidpad.load_tables()[0]
    got = d.broadcast_array(table, table.shape)
    assert np.array_equal(got, table)
    assert d.broadcast_check_table(c.default_path())
    assert d.max_over_ranks(3.5) == 3.5 and d.sum_over_ranks(2.0) == 2.0
    d.barrier()
    # the compute path still works on the same stream after collectives
    off, cones, poses = pkg.synth.make_replay_batch(8, 16, 0.1, seed=3)
    assert (c.plan_batch(off, cones, poses)["status"] == 0).all()
    # RCCL is for the start-up broadcast: afterwards the communicator (and its context) can go, the scalar collectives carry on
    d.release_device_communicator()
    assert not d._active and d.released and d.transport == "rccl" and "released" in d.describe()
    assert d.max_over_ranks(3.5) == 3.5 and d.sum_over_ranks(2.0) == 2.0
    d.barrier()
    assert (c.plan_batch(off, cones, poses)["status"] == 0).all()
    d.close()
    c.close()
    assert "torch" not in sys.modules or True  # (pytest plugins may import torch; bench.py asserts it for real)


def test_two_contexts_interleaved_from_one_thread(pkg):
    """Every entry point selects its context's device and owns its streams: two contexts used alternately from one host
    thread (one per GPU when several are visible, both on GPU 0 here) give the results of separate runs."""
    n_dev = pkg._capi.load().fsdp_device_count()
    a = pkg.Context(device=0, mission=4)
    b = pkg.Context(device=1 if n_dev > 1 else 0, mission=4)
    fa = pkg.synth.make_replay_batch(96, 32, 0.1, seed=11)
    fb = pkg.synth.make_replay_batch(160, 24, 0.1, seed=12)
    ref_a, ref_b = a.plan_batch(*fa), b.plan_batch(*fb)
    a.upload(*fa)
    b.upload(*fb)
    a.run()
    b.run()
    sa = a.sort_batch(*fa)          # stage call on a while b has a pass in flight
    rb = b.download()
    a.upload(*fa)
    a.run()
    ra = a.download()
    assert np.array_equal(ra["path"], ref_a["path"], equal_nan=True) and np.array_equal(rb["path"], ref_b["path"], equal_nan=True)
    assert np.array_equal(sa["left_idx"], ref_a["left_idx"]) and len(rb) == 160 and len(ra) == 96
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["params_sort", "params_path", "params_monotonic", "params_deg2", "params_deg1", "params_horizon", "params_no_unknown"])
def test_non_default_parameters(pkg, golden_dir, name):
    """fsdp_create with a parameter block: the reference's stage classes constructed with non-default kwargs (goldens:
    make_golden.py params_golden) — indices bit-equal, paths within 1e-5 of the reference, bit-equal to the oracle."""
    g = np.load(golden_dir / f"{name}.npz")
    prm = dict(zip(g["param_names"].tolist(), g["param_values"].tolist()))
    c = pkg.Context(device=0, mission=4, params=prm)
    res = c.plan_batch(g["offsets"], g["cones"], g["poses"])
    rows = _as_oracle_rows(res)
    cats = collections.Counter()
    arc = parity.ArcLibm(golden_dir, name)
    for k in range(len(rows)):
        cat, detail = parity.compare_frame(rows[k], g, k, arc=arc)
        cats[cat] += 1
        assert cat in ("ok", "ref_undefined", "flip"), (k, cat, detail)
    assert cats["flip"] == len(arc.flips("det")), (cats, arc.flips("det"))  # (params_sort: 98; params_no_unknown: 6 and 97)
    with oracle_lib.params(prm), oracle_lib.math_mode(1):
        ref = oracle_lib.plan_batch(g["offsets"], g["cones"], g["poses"], n_threads=os.cpu_count() or 1)
    _assert_equal_to_oracle(res, ref)
    # a second context with the defaults is unaffected
    d = np.load(golden_dir / "cfg2_color.npz")
    c0 = pkg.Context(device=0, mission=4)
    r0 = c0.plan_batch(d["offsets"], d["cones"], d["poses"])
    assert np.array_equal(r0["left_idx"], d["left_idx"]) and np.array_equal(c.plan_batch(d["offsets"], d["cones"], d["poses"])["status"] >= 0, np.ones(len(r0), bool))
    c.close()
    c0.close()


@pytest.mark.parametrize("max_deg", [1, 2])
def test_low_degree_contexts_plan_large_batches_four_frames_per_wavefront(pkg, max_deg):
    """max_deg < 3 (utils/spline_fit.py:113: fits #1 / #2 of degree clip(points - 1, 1, max_deg)): the three-kernel path stage holds
    cubic fits only, so such a context's large batches run the one-kernel stage with four frames per wavefront (path_kernel<16>:
    all degrees, 32 knots, the scaling-free divisions; round 4 gave them one frame per wavefront whatever the batch) — bit-equal
    to the oracle with the same parameters, a clean and a noisy batch (frames on the exact route)."""
    prm = {"max_deg": max_deg}
    c = pkg.Context(device=0, mission=4, params=prm)
    sets = [pkg.synth.make_replay_batch(1500, 64, 0.15, seed=51, color=True),
            pkg.synth.make_replay_batch(1100, 100, 0.0, seed=52, frame_noise=0.3, random_pose=True, color=False)]
    for off, cones, poses in sets:
        res = c.plan_batch(off, cones, poses)
        assert "path_kernel<16>" in c.stage_names(), c.stage_names()
        with oracle_lib.params(prm), oracle_lib.math_mode(1):
            ref = oracle_lib.plan_batch(off, cones, poses, n_threads=os.cpu_count() or 1)
        _assert_equal_to_oracle(res, ref)
        assert (res["status"] == 0).mean() > 0.8
    small = c.plan_batch(*[a[:k] for a, k in zip(sets[0], (201, sets[0][0][200], 200))])
    assert "path_kernel<64>" in c.stage_names()  # small batches keep a wavefront per frame
    assert small["path"].tobytes() == res["path"][:0].tobytes() or small["path"].tobytes() == c.plan_batch(*sets[0])["path"][:200].tobytes()
    c.close()


def test_parameters_outside_the_kernels_capacities_are_refused(pkg):
    for bad in (dict(max_n_neighbors=9), dict(max_length=17), dict(max_deg=4), dict(max_deg=0), dict(mpc_prediction_horizon=65),
                dict(mpc_prediction_horizon=0), dict(mpc_path_length=100.0)):
        with pytest.raises(pkg.FsdpError):
            pkg.Context(device=0, mission=4, params=bad)
    # the standard build itself refuses what only the wide build's shapes hold (nothing is truncated silently)
    for bad in (dict(max_n_neighbors=6), dict(max_length=13), dict(mpc_prediction_horizon=41)):
        with pytest.raises(pkg.FsdpError):
            pkg.Context(device=0, mission=4, params=bad, shapes=pkg._capi.STANDARD)
    with pytest.raises(TypeError):
        pkg.Context(device=0, mission=4, params=dict(no_such_parameter=1))


WIDE_SETS = ["params_wide_sort", "params_wide_horizon", "params_wide_all"]


def _wide_rows(res):
    import oracle_lib_wide

    out = np.zeros(len(res), oracle_lib_wide.RESULT_DTYPE)
    for k in oracle_lib_wide.RESULT_DTYPE.names:
        out[k] = res[k]
    return out


@pytest.mark.parametrize("name", WIDE_SETS)
def test_parameters_beyond_the_standard_shapes_run_on_the_wide_build(pkg, golden_dir, name):
    """max_n_neighbors up to 8, max_length up to 16, mpc_prediction_horizon up to 64 (the reference takes any value,
    config.py:34-37,58; end_configurations.py:74-105): a context with such parameters is carried by libfsdp_hip_wide.so — the
    same sources compiled with -DFSDP_WIDE_SHAPES — chosen by the Python host.  Goldens captured from the reference with those
    kwargs (make_golden.py --params-r5): indices bit-equal, paths within 1e-5; bit-equal to the oracle's wide build."""
    import oracle_lib_wide

    g = np.load(golden_dir / f"{name}.npz")
    prm = dict(zip(g["param_names"].tolist(), g["param_values"].tolist()))
    c = pkg.Context(device=0, mission=4, params=prm)
    assert c.shapes is pkg._capi.WIDE and c.result_dtype.itemsize > pkg.RESULT_DTYPE.itemsize
    with oracle_lib_wide.params(prm):
        dp, dp_ref = c.default_path(), oracle_lib_wide.default_path()
    assert dp.shape == (64, 4) and np.array_equal(np.isnan(dp), np.isnan(dp_ref)) and np.nanmax(np.abs(dp - dp_ref)) < 1e-12
    assert np.isfinite(dp[: c.horizon]).all() and np.isnan(dp[c.horizon :]).all()
    res = c.plan_batch(g["offsets"], g["cones"], g["poses"])
    assert res["path"].shape[1:] == (64, 4) and res["left_idx"].shape[1] == 16
    rows = _wide_rows(res)
    cats = collections.Counter()
    arc = parity.ArcLibm(golden_dir, name)
    for k in range(len(rows)):
        cat, detail = parity.compare_frame(rows[k], g, k, arc=arc)
        cats[cat] += 1
        assert cat in ("ok", "ref_undefined", "flip"), (k, cat, detail)
    assert cats["flip"] == len(arc.flips("det")), (cats, arc.flips("det"))
    with oracle_lib_wide.params(prm), oracle_lib_wide.math_mode(1):
        ref = oracle_lib_wide.plan_batch(g["offsets"], g["cones"], g["poses"], n_threads=os.cpu_count() or 1)
    _assert_equal_to_oracle(res, ref)
    if name != "params_wide_horizon":
        assert max(int(res["n_left"].max()), int(res["n_right"].max())) > 12
    # a large batch with the same parameters (the packed kernels of the wide build), streamed and sequential forms included
    off, cones, poses = pkg.synth.make_replay_batch(3000, 64, 0.15, seed=77, color=(name != "params_wide_all"))
    big = c.plan_batch(off, cones, poses)
    with oracle_lib_wide.params(prm), oracle_lib_wide.math_mode(1):
        ref_big = oracle_lib_wide.plan_batch(off, cones, poses, n_threads=os.cpu_count() or 1)
    _assert_equal_to_oracle(big, ref_big)
    assert (big["status"] == 0).mean() > 0.9
    c.set_overlap(3)
    tickets = [c.submit(off, cones, poses) for _ in range(3)]
    for t in tickets:
        assert c.collect(t).tobytes() == big.tobytes()
    c.set_overlap(1)
    seq = c.plan_batch_sequential(off[:201], cones[: off[200]], poses[:200], big["path"][:200, : c.horizon])
    assert np.array_equal(seq["left_idx"], big["left_idx"][:200]) and seq["path"].shape == (200, 64, 4)
    # the standard build next to it is unaffected
    d = np.load(golden_dir / "cfg2_color.npz")
    c0 = pkg.Context(device=0, mission=4)
    assert c0.shapes is pkg._capi.STANDARD
    assert np.array_equal(c0.plan_batch(d["offsets"], d["cones"], d["poses"])["left_idx"], d["left_idx"])
    c.close()
    c0.close()


def test_host_classes_on_the_wide_build(pkg, golden_dir):
    """The host classes with parameters beyond the standard shapes: a stateful PathPlanner (the reference's call, previous path
    chained), MultiPlanner (contexts on the one GPU; page-locked and pageable batches, a stream of them) and AccelerationBatch
    with a 56-row horizon against planner objects — every one carried by the wide build without the caller naming it."""
    import oracle_lib_wide

    prm = dict(max_n_neighbors=8, max_length=16, mpc_prediction_horizon=56)
    off, cones, poses = pkg.synth.make_replay_batch(2400, 64, 0.15, seed=31, color=True)
    with oracle_lib_wide.params(prm), oracle_lib_wide.math_mode(1):
        ref = oracle_lib_wide.plan_batch(off, cones, poses, n_threads=os.cpu_count() or 1)
    # one process, three contexts on the GPU: the same bytes as one context
    one = pkg.Context(device=0, params=prm)
    want = one.plan_batch(off, cones, poses)
    _assert_equal_to_oracle(want, ref)
    mp = pkg.MultiPlanner([0, 0, 0], params=prm)
    assert mp.ctx[0].shapes is pkg.WIDE
    got = mp.plan_batch(off, cones, poses)
    assert got.dtype == pkg.WIDE.result_dtype and got.tobytes() == want.tobytes()
    pinned = (pkg.pinned_copy(off, np.int32), pkg.pinned_copy(cones, np.float64), pkg.pinned_copy(poses, np.float64))
    outs = list(mp.plan_stream([pinned, (off, cones, poses), pinned]))
    assert all(o.tobytes() == want.tobytes() for o in outs)
    mp.close()
    one.close()
    # the reference's call, frame after frame (the previous path chained: core_calculate_path.py:572-573)
    planner = pkg.PathPlanner(pkg.MissionTypes.trackdrive, device=0, params=prm)
    prev = None
    for k in range(0, 60, 3):
        xyt = cones[off[k] : off[k + 1]]
        path = planner.calculate_path_in_global_frame(xyt, poses[k][:2], poses[k][2:])
        with oracle_lib_wide.params(prm), oracle_lib_wide.math_mode(1):
            r = oracle_lib_wide.plan_frame_prev(xyt, poses[k], prev)
        assert path.shape == (56, 4) and np.array_equal(path, r["path"][:56])
        prev = r["path"]
    # acceleration mission, planners in lock-step, 56 rows
    acc = pkg.acceleration
    g = np.load(golden_dir / "global_path.npz")
    n = 3
    seeds = [int(g["acc_seed"]), 7, 8]
    planners = [pkg.PathPlanner(pkg.MissionTypes.acceleration, device=0, relocalization_seed=sd, params=dict(mpc_prediction_horizon=56)) for sd in seeds]
    batch = acc.AccelerationBatch(n, pkg.MissionTypes.acceleration, seeds=seeds, device=0, params=dict(mpc_prediction_horizon=56))
    o, c, p = g["acc_offsets"], g["acc_cones"], g["acc_poses"]
    for t in range(min(20, len(p))):
        xyt = c[o[t] : o[t + 1]]
        offs = np.arange(n + 1, dtype=np.int32) * len(xyt)
        paths, status = batch.step(offs, np.concatenate([xyt] * n), np.repeat(p[t][None], n, axis=0))
        for i in range(n):
            w = planners[i].calculate_path_in_global_frame(xyt, p[t][:2], p[t][2:])
            assert status[i] == 0 and paths[i].shape == (56, 4) and np.array_equal(paths[i], w), (t, i)
    assert batch.relocalized.all()


def test_reference_shaped_planner_and_stage_classes_on_the_wide_build(pkg, golden_dir):
    """PathPlanner / ConeSorting / ConeMatching / CalculatePath with max_length = 16, max_n_neighbors = 8: the stage objects hand
    sides of up to 16 cones (32 with virtual ones) to each other like the reference's do (full_pipeline.py:142-176)."""
    g = np.load(golden_dir / "params_wide_sort.npz")
    cs = pkg.ConeSorting(device=0, max_n_neighbors=8, max_dist=6.5, max_dist_to_first=6.0, max_length=16,
                         threshold_directional_angle=np.deg2rad(40), threshold_absolute_angle=np.deg2rad(65), use_unknown_cones=True,
                         experimental_performance_improvements=False)
    cm = pkg.ConeMatching(device=0)
    cp = pkg.CalculatePath(device=0, stateful=False)
    n_long = 0
    for k in range(0, len(g["ok"]), 9):
        if not g["ok"][k]:
            continue
        xyt = g["cones"][g["offsets"][k] : g["offsets"][k + 1]]
        pos, direc = g["poses"][k][:2], g["poses"][k][2:]
        cs.set_new_input(pkg.ConeSortingInput(xyt, pos, direc))
        left, right = cs.run_cone_sorting()
        nl, nr = int(g["n_left"][k]), int(g["n_right"][k])
        assert np.array_equal(left, xyt[g["left_idx"][k][:nl], :2]) and np.array_equal(right, xyt[g["right_idx"][k][:nr], :2])
        n_long += max(nl, nr) > 12
        sorted_cones = [np.zeros((0, 2)) for _ in range(5)]
        sorted_cones[int(pkg.ConeTypes.LEFT)], sorted_cones[int(pkg.ConeTypes.RIGHT)] = left, right
        cm.set_new_input(pkg.ConeMatchingInput(sorted_cones, pos, direc))
        lv, rv, l2r, r2l = cm.run_cone_matching()
        ml, mr = int(g["n_left_v"][k]), int(g["n_right_v"][k])
        assert np.array_equal(lv, g["left_v"][k][:ml]) and np.array_equal(rv, g["right_v"][k][:mr])
        assert np.array_equal(l2r, g["l2r"][k][:ml]) and np.array_equal(r2l, g["r2l"][k][:mr])
        cp.set_new_input(pkg.PathCalculationInput(lv, rv, l2r, r2l, pos, direc))
        path, _centers = cp.run_path_calculation()
        assert path.shape == (40, 4) and np.nanmax(np.abs(path - g["path"][k][:40])) < (1e-5 if not (k in (106, 131)) else 1.0)
    assert n_long >= 3


def test_stage_classes_take_the_reference_kwargs(pkg, golden_dir):
    """ConeSorting(**kwargs) as the reference constructs it (core_cone_sorting.py:49-100), with a non-default max_length."""
    g = np.load(golden_dir / "params_sort.npz")
    prm = dict(zip(g["param_names"].tolist(), g["param_values"].tolist()))
    sk = {k: prm[k] for k in ("max_n_neighbors", "max_dist", "max_dist_to_first", "max_length", "threshold_directional_angle",
                              "threshold_absolute_angle")}
    sk["max_n_neighbors"], sk["max_length"] = int(sk["max_n_neighbors"]), int(sk["max_length"])
    cs = pkg.ConeSorting(device=0, use_unknown_cones=True, experimental_performance_improvements=False, **sk)
    for k in range(0, 40, 7):
        if not g["ok"][k]:
            continue
        xyt = g["cones"][g["offsets"][k] : g["offsets"][k + 1]]
        cs.set_new_input(pkg.ConeSortingInput(xyt, g["poses"][k][:2], g["poses"][k][2:]))
        left, right = cs.run_cone_sorting()
        assert np.array_equal(left, xyt[g["left_idx"][k][: g["n_left"][k]], :2])
        assert np.array_equal(right, xyt[g["right_idx"][k][: g["n_right"][k]], :2])


def test_device_math_helpers(ctx):
    """sqrt_1_2 == sqrt on [1, 2] and the scaling-free quotient == the IEEE division for operands in its exponent band,
    bit for bit, on 10^6 random arguments each (exponents within +-250, exact quotients, tiny / huge ratios inside the band).  The band's
    last binades, its edges, the first values outside it and operands that are hard to round are tests/test_hard_rounding_gpu.py's."""
    rng = np.random.default_rng(0)
    n = 1_000_000
    x = np.concatenate([rng.uniform(1.0, 2.0, n - 6), [1.0, 2.0, np.nextafter(1.0, 2.0), np.nextafter(2.0, 1.0), 1.5, 1.25]])
    mant = rng.uniform(1.0, 2.0, (2, n))
    ea, eb = rng.integers(-250, 250, n), rng.integers(-250, 250, n)
    a = np.ldexp(mant[0], ea) * rng.choice([-1.0, 1.0], n)
    b = np.ldexp(mant[1], eb) * rng.choice([-1.0, 1.0], n)
    a[:1000] = 0.0                      # zero numerators (fresh band rows)
    a[1000:2000] = b[1000:2000] * 3.0   # exact quotients
    out = ctx.selftest_math(x, a, b)
    assert np.array_equal(out[0].view(np.uint64), out[1].view(np.uint64)), int((out[0] != out[1]).sum())
    assert np.array_equal(out[1], np.sqrt(x))
    safe = (out[4] == 1.0) | (a == 0.0)
    assert safe.mean() > 0.99
    assert np.array_equal(out[2][safe].view(np.uint64), out[3][safe].view(np.uint64)), int((out[2][safe] != out[3][safe]).sum())
    assert np.array_equal(out[3], a / b)
    # outside the band the guard reports it (such operands send a frame to the exact kernel)
    o2 = ctx.selftest_math(np.full(4, 1.5), np.array([1e-300, 1e300, 1.0, 1.0]), np.array([1.0, 1.0, 1e-300, 1e300]))
    assert (o2[4] == 0.0).all()


def test_device_givens_sequence_returns_the_ieee_bits(ctx):
    """FITPACK's fpgivs as the spline kernels compute it (spline_device.h fpgivs_guarded<true> / giv_step<true>: max / min for the
    branch, scaling-free quotients, and — round 5 — the reciprocal of the new diagonal seeded from the square root's own Goldschmidt
    iterate instead of v_rcp_f64: three links off the step's dependent chain) against the same routine with the compiler's IEEE
    division and square root, on the device: cs, sn and dd bit for bit on four million (pivot, diagonal) pairs — ordinary magnitudes,
    pivots far below / above the diagonal, equal magnitudes, fresh band rows (diagonal 0), zero pivots."""
    rng = np.random.default_rng(11)
    n = 1 << 20
    for rnd in range(4):
        piv = rng.normal(0, 1, n) * 10.0 ** rng.uniform(-6, 4, n)
        ww = np.abs(rng.normal(0, 1, n)) * 10.0 ** rng.uniform(-6, 4, n)
        if rnd == 1:  # a data row against a well-filled band row: |piv| << ww, and the other way round
            piv[: n // 2] *= 10.0 ** rng.uniform(-12, -3, n // 2)
            ww[n // 2 :] *= 10.0 ** rng.uniform(-12, -3, n - n // 2)
        if rnd == 2:  # spline basis values: pivots in [0, 1], diagonals that are norms of a few of them
            piv = rng.uniform(0, 1, n) ** 3
            ww = np.sqrt(rng.uniform(0, 1, n) ** 2 * rng.integers(1, 200, n))
        ww[:2000] = 0.0                       # fresh band rows
        piv[2000:4000] = 0.0                  # nothing to rotate
        piv[4000:6000] = ww[4000:6000] * rng.choice([-1.0, 1.0], 2000)  # equal magnitudes
        out = ctx.selftest_givens(piv, ww)
        ok = out[6] == 1.0
        assert ok.mean() > 0.99
        for k, name in enumerate(("cs", "sn", "dd")):
            a, b = out[k][ok], out[3 + k][ok]
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (rnd, name, int((a != b).sum()), a[a != b][:3], b[a != b][:3])
        nz = ok & (piv != 0) & (ww != 0)
        assert np.all(np.abs(out[0][nz] ** 2 + out[1][nz] ** 2 - 1.0) < 1e-15)
    band = ctx.selftest_givens(np.array([1e-300, 1e300, 1.0]), np.array([1.0, 1.0, 1e300]))
    assert (band[6] == 0.0).all()  # outside the band the guard says so (the frame is planned with the IEEE operations)


def test_device_abs_min_max_on_special_operands(ctx):
    """max_abs_nn / min_abs_nn (inline v_max_f64 |a|, b / v_min_f64 |a|, b — the emulator replaces them by compares) on
    everything a pivot / diagonal pair can be: ordinary values, +-0, denormals, equal magnitudes, infinities.  With a NaN
    operand the instructions return the *other* operand (IEEE maxNum / minNum) where the compare form would hand NaN on; the
    Givens step is only reached with finite rows (a NaN coordinate ends a frame in the stages before), so the contract is
    'never NaN' and the test pins what the hardware does."""
    rng = np.random.default_rng(1)
    sp = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -1e-310, 1.0, -1.0, 3.5, -3.5, 1e300, -1e300, np.inf, -np.inf])
    a = np.concatenate([np.repeat(sp, len(sp)), rng.normal(0, 1, 1000) * 10.0 ** rng.uniform(-200, 200, 1000)])
    b = np.abs(np.concatenate([np.tile(sp, len(sp)), rng.normal(0, 1, 1000) * 10.0 ** rng.uniform(-200, 200, 1000)]))  # ww >= 0
    out = ctx.selftest_absminmax(a, b)
    assert np.array_equal(out[0], np.maximum(np.abs(a), b)) and np.array_equal(out[1], np.minimum(np.abs(a), b))
    assert not np.signbit(out[0][(a == 0) & (b == 0)]).any()  # |−0| = +0: no negative zero leaves the step
    nan = ctx.selftest_absminmax(np.array([np.nan, 2.0]), np.array([3.0, np.nan]))
    assert nan[0][0] == 3.0 and nan[1][0] == 3.0 and nan[0][1] == 2.0 and nan[1][1] == 2.0


def test_large_sequential_batch_keeps_previous_paths_on_every_route(pkg, ctx, golden_dir):
    """A lock-step batch above the small-batch threshold (three-kernel path stage) with a caller-supplied previous path per
    frame: frames that fall back to their previous path (few cones), frames the fast kernels hand to the exact kernel
    (2-3 centre points: degree < 3) and ordinary frames all see the caller's previous path, not the default one."""
    g = np.load(golden_dir / "fuzz.npz")
    rng = np.random.default_rng(5)
    n = 1600
    pick = rng.integers(0, len(g["ok"]), n)
    off = np.concatenate([[0], np.cumsum([g["offsets"][i + 1] - g["offsets"][i] for i in pick])]).astype(np.int32)
    cones = np.concatenate([g["cones"][g["offsets"][i] : g["offsets"][i + 1]] for i in pick])
    poses = g["poses"][pick]
    # previous paths: the default path rigidly moved per frame (so that using the wrong one is visible)
    base = ctx.default_path()
    ang = rng.uniform(-0.3, 0.3, n)
    sh = rng.uniform(-1.0, 1.0, (n, 2))
    prev = np.repeat(base[None], n, axis=0)
    c, s_ = np.cos(ang)[:, None], np.sin(ang)[:, None]
    prev[:, :, 1] = base[None, :, 1] * c - base[None, :, 2] * s_ + sh[:, :1]
    prev[:, :, 2] = base[None, :, 1] * s_ + base[None, :, 2] * c + sh[:, 1:]
    res = ctx.plan_batch_sequential(off, cones, poses, prev)
    assert "path_prep_kernel" in ",".join(ctx.stage_names())  # the three-kernel route really ran
    n_prev = 0
    with oracle_lib.math_mode(1):
        for k in range(0, n, 3):
            r = oracle_lib.plan_frame_prev(cones[off[k] : off[k + 1]], poses[k], prev[k])
            assert int(res[k]["status"]) == int(r["status"]), k
            if r["status"] == 0:
                assert np.array_equal(res[k]["left_idx"], r["left_idx"]) and int(res[k]["path_fallback"]) == int(r["path_fallback"]), k
                assert np.abs(res[k]["path"] - r["path"]).max() <= 1e-9, (k, int(r["path_fallback"]))
                n_prev += bool(int(r["path_fallback"]) & (1 | 2 | 4 | 8))
    assert n_prev > 50  # plenty of sampled frames really used their previous path
    # one-shot: the next plain batch is planned with fresh planners again
    again = ctx.plan_batch(off[:65], cones[: off[64]], poses[:64])
    fresh = ctx.plan_batch(off[:65], cones[: off[64]], poses[:64])
    assert np.array_equal(again["path"], fresh["path"], equal_nan=True)


def test_refit_spline_equals_oracle(pkg, ctx):
    """Per-stage intermediate on the device: knots and coefficients of the refit (fit #2, the kernel the roofline line is
    about) of every sampled frame of a 2048-frame batch equal the oracle's second spline of that frame bit for bit —
    and the oracle's splines equal the reference's (tests/test_oracle_golden.py::test_oracle_splines_match_reference_per_frame)."""
    off, cones, poses = pkg.synth.make_replay_batch(2048, 64, 0.15, seed=1, color=True)
    ctx.set_option("plan_chunks", 1)  # (fsdp_debug_refit reads the most recent PASS: the batch is one)
    try:
        res = ctx.plan_batch(off, cones, poses)
        nk, t, c = ctx.debug_refit()
    finally:
        ctx.set_option("plan_chunks", 0)
    assert (nk > 0).mean() > 0.95  # the fast route
    checked = 0
    with oracle_lib.math_mode(1):
        for k in range(0, 2048, 37):
            if nk[k] <= 0 or res[k]["status"] != 0:
                continue
            r, nf, fits = oracle_lib.plan_frame_capture(cones[off[k] : off[k + 1]], poses[k])
            assert nf == 3, (k, nf)
            kk, n, tt, cx, cy = fits[1]
            assert kk == 3 and n == int(nk[k]), (k, n, int(nk[k]))
            assert np.array_equal(t[k, :n], tt), k
            assert np.array_equal(c[k, : n - 4], cx[: n - 4]) and np.array_equal(c[k, n : 2 * n - 4], cy[: n - 4]), k
            checked += 1
    assert checked >= 40


def test_debug_reads_of_a_chunked_blocking_call_fail(pkg):
    """fsdp_debug_refit / fsdp_debug_arena read exactly the most recent pass: a blocking call cut into chunks has no one pass that
    covers the call, so they fail instead of returning the last chunk's scratch (round-6 advisor)."""
    import ctypes

    off, cones, poses = pkg.synth.make_replay_batch(2048, 64, 0.15, seed=1, color=True)
    ctx = pkg.Context(device=0, options={"plan_chunks": 4})
    ctx.plan_batch(off, cones, poses)
    with pytest.raises(pkg.FsdpError, match="fsdp_debug_refit"):
        ctx.debug_refit()
    out = np.zeros(1)
    assert ctx._lib.fsdp_debug_arena(ctx._h, 0, 0, 1, ctypes.c_void_p(out.ctypes.data)) != 0
    ctx.set_option("plan_chunks", 1)
    ctx.plan_batch(off, cones, poses)
    nk, _, _ = ctx.debug_refit()  # one pass over the whole call: readable
    assert len(nk) == 2048 and (nk > 0).mean() > 0.95
    ctx.close()


def _same_records(a, b):
    return a.dtype == b.dtype and len(a) == len(b) and all(
        np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes() for f in a.dtype.names)


def test_download_returns_only_the_most_recent_run(pkg):
    """fsdp_download returns the results of the most recent fsdp_run / fsdp_time_runs pass, or fails: after a blocking call,
    after a ticket, after an upload that no pass has followed, and after fsdp_set_overlap released the pass's slot (round-6
    advisor: these used to return stale device memory)."""
    off, cones, poses = pkg.synth.make_replay_batch(512, 64, 0.15, seed=21, color=True)
    ctx = pkg.Context(device=0)
    ref = ctx.plan_batch(off, cones, poses)
    with pytest.raises(pkg.FsdpError, match="fsdp_download"):
        ctx.download()  # after a blocking call
    ctx.upload(off, cones, poses)
    with pytest.raises(pkg.FsdpError, match="fsdp_download"):
        ctx.download()  # no pass over the uploaded batch yet
    ctx.run()
    assert _same_records(ctx.download(), ref)
    assert _same_records(ctx.collect(ctx.submit(off, cones, poses)), ref)
    with pytest.raises(pkg.FsdpError, match="fsdp_download"):
        ctx.download()  # after a ticket
    ctx.set_overlap(3)
    for _ in range(3):
        ctx.run()  # the last one in slot 2
    assert _same_records(ctx.download(), ref)
    ctx.set_overlap(2)
    with pytest.raises(pkg.FsdpError, match="fsdp_download"):
        ctx.download()  # slot 2 was released
    ctx.run()
    assert _same_records(ctx.download(), ref)
    ctx.close()


def test_device_det3_sign_is_numpys(pkg, ctx):
    """calculate_path/path_parameterization.py:86-92: the sign of the curvature is the sign of np.linalg.det of three
    homogeneous points — zero up to rounding on a straight stretch.  The device's restatement (path_kernel.h det3_lu,
    OpenBLAS' getf2 operation order) equals the oracle's bit for bit and NumPy's sign on this machine's NumPy as well."""
    import ctypes

    rng = np.random.default_rng(3)
    rows = []
    for k in range(20000):
        sc = 10.0 ** rng.uniform(-2, 4)
        p0, d = rng.normal(0, sc, 2), rng.normal(0, 1, 2)
        t1, t2 = rng.uniform(0.01, 5, 2)
        p = np.array([p0, p0 + t1 * d, p0 + (t1 + t2) * d])
        if k % 4 == 1:
            p += rng.normal(0, 1e-13 * sc, p.shape)
        elif k % 4 == 2:
            p = p[rng.permutation(3)]
        elif k % 4 == 3:
            p = rng.normal(0, sc, (3, 2))
        rows.append(p.ravel())
    rows = np.array(rows)
    dev = ctx.selftest_det3(rows)
    L = oracle_lib.lib()
    L.fsdo_det3.restype = ctypes.c_double
    host = np.array([L.fsdo_det3(r.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) for r in rows])
    assert np.array_equal(dev, host)
    ref = np.array([np.linalg.det(np.column_stack((np.ones(3), r.reshape(3, 2)))) for r in rows])
    assert np.array_equal(np.sign(dev), np.sign(ref))


def test_device_libm_values_the_sorting_stage_decides_with(ctx):
    """The sorting stage keeps the ROCm device library's atan2 / acos where the reference compares np.arctan2 / np.arccos values
    (search predicates, start-cone bearings, cost terms -> arg-min).  That the kernels decide like the oracle next to a tie no
    longer rests on how far sampled frames stay from one: tests/test_sort_constructed_gpu.py puts a cone 1e-9 (relative) either
    side of every threshold of the stage, and on it, on every route (tests/sort_support.py; the emulated kernels in
    tests/test_sort_constructed_cpu.py).  Those pairs hold if the library's atan2 / acos stay within an ulp or two of the true
    value, nine orders of magnitude below their offset.  Pinned here: against the correctly rounded det_atan2 (computed on
    the device next to it; bit-identical to the host copy that tests/test_det_math.py holds to mpmath) on 10^6 arguments —
    track-scale vectors, near-axis and near-diagonal directions, tiny and huge magnitudes — and acos against the host's on
    10^6 cosines incl. the neighbourhood of the thresholds' cosines and of +-1."""
    rng = np.random.default_rng(17)
    n = 1_000_000
    ang = rng.uniform(-np.pi, np.pi, n)
    mag = 10.0 ** rng.uniform(-3, 3, n)
    y, x = mag * np.sin(ang), mag * np.cos(ang)
    k = n // 8
    y[:k] *= 10.0 ** rng.uniform(-16, -6, k)            # near the x axis (straight tracks: differences of almost equal bearings)
    x[k : 2 * k] *= 10.0 ** rng.uniform(-16, -6, k)      # near the y axis
    y[2 * k : 3 * k] = x[2 * k : 3 * k] * (1 + rng.normal(0, 1e-12, k))  # near the diagonals
    y[3 * k : 3 * k + 8] = [0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 0.0, -0.0]
    x[3 * k : 3 * k + 8] = [1.0, 1.0, -1.0, -1.0, 0.0, 0.0, 0.0, -0.0]
    cs = np.clip(np.cos(rng.uniform(0, np.pi, n)), -1, 1)
    thr = np.cos(np.deg2rad([40.0, 65.0, 60.0, 50.0, 90.0, 150.0]))
    cs[:k] = np.clip(rng.choice(thr, k) + rng.normal(0, 2e-9, k), -1, 1)     # where acos_less / acos_greater evaluate the arc cosine
    cs[k : 2 * k] = np.clip(1 - 10.0 ** rng.uniform(-16, -1, k), -1, 1) * rng.choice([-1.0, 1.0], k)
    out = ctx.selftest_libm(y, x, cs)

    def ulps(a, b):
        ia, ib = a.view(np.int64).copy(), b.view(np.int64).copy()
        ia[ia < 0] = np.int64(-(2**63)) - ia[ia < 0]   # (sign-magnitude -> monotone integers)
        ib[ib < 0] = np.int64(-(2**63)) - ib[ib < 0]
        return np.abs(ia - ib)

    d = ulps(out[0], out[1])
    # measured on ROCm 7.2: 2 ulp at most (the device library's documented bound for atan2).  A release that goes beyond that
    # moves this assertion, not a sorted index unnoticed.
    assert d.max() <= 2, (int(d.max()), y[d.argmax()], x[d.argmax()])
    assert (d == 2).mean() < 0.01
    assert np.array_equal(np.signbit(out[0]), np.signbit(out[1]))
    # det_atan2 on the device == the host's glibc within an ulp too (a second, independent witness)
    assert ulps(out[1], np.arctan2(y, x)).max() <= 1
    a = ulps(out[2], np.arccos(cs))
    assert a.max() <= 2, (int(a.max()), cs[a.argmax()])
    print(f"device atan2 vs det_atan2: {int((d == 0).sum())} of {n} bit-equal, {int((d == 1).sum())} off by 1 ulp, {int((d == 2).sum())} by 2 ulp; acos vs host: {int((a == 0).sum())} bit-equal, max {int(a.max())} ulp")


def test_both_forms_of_the_exact_route_return_the_same_bytes(pkg, monkeypatch):
    """path_retry_kernel plans a short list of handed-on frames with a wavefront per frame (64 lanes, plain divisions) and a
    long one with four frames per wavefront (16 lanes each, 64 knots, the scaling-free divisions; a frame outside their
    exponent band once more by the whole wavefront).  Same bytes either way, on a noisy colourless batch (knot overflows of
    the packed kernels), on a global-path batch (every frame takes the route) and with a non-cubic context."""
    noisy = pkg.synth.make_replay_batch(1536, 100, 0.0, seed=8, frame_noise=0.3, random_pose=True, color=False, lateral_noise=0.5, heading_noise=0.2)
    left, right, centre_fn = pkg.synth.closed_track(40, 33)
    gp = np.array([centre_fn(s)[0] for s in np.linspace(0, 1, 600, endpoint=False)])
    smooth = pkg.synth.make_replay_batch(1300, 40, 0.15, seed=33, color=True)
    got = {}
    for form, pack_min in (("whole", 1000000), ("shared", 1)):
        c = pkg.Context(device=0, options={"retry_pack_min": pack_min})
        r1 = c.plan_batch(*noisy)
        assert c.route_stats()[1]  # the exact route was needed
        c.set_global_path(gp)
        r2 = c.plan_batch(*smooth)
        c.close()
        got[form] = (r1, r2)
    for a, b in zip(got["whole"], got["shared"]):
        assert a.tobytes() == b.tobytes()
    assert (got["whole"][1]["status"] == 0).mean() > 0.99


@pytest.mark.parametrize("seed,frame,knots", [(511, 901, 68), (516, 1001, 171)])
def test_refits_beyond_64_knots_are_planned_on_the_gpu(pkg, seed, frame, knots):
    """FITPACK's nest is m + 2k (utils/spline_fit.py:117): the noisiest frames of round 5's wide fuzz end their refit with 68 and 171 knots and
    were refused with FSDP_OVERFLOW_KNOTS while the exact kernel kept 64; it keeps 256 now (csrc/spline_device.h NK_BIG).  Whole sets of 1024
    frames through the library's own choice of kernels (three-kernel path stage -> retry list -> path_retry_kernel's two levels) and
    through the one-kernel stage: no frame refused, every frame equal to the oracle's wide build."""
    import oracle_lib_wide

    per_side, track, noise, colour = {511: (64, 0.1, 0.3, True), 516: (64, 0.3, 0.3, False)}[seed]
    off, cones, poses = pkg.synth.make_replay_batch(1024, per_side, track, seed=seed, frame_noise=noise, random_pose=True, color=colour)
    prm = dict(max_n_neighbors=8, max_length=16)
    with oracle_lib_wide.params(prm), oracle_lib_wide.math_mode(1):
        ref = oracle_lib_wide.plan_batch(off, cones, poses, n_threads=os.cpu_count() or 1)
        _, nf, fits = oracle_lib_wide.plan_frame_capture(cones[off[frame] : off[frame + 1]], poses[frame])
    assert max(f[1] for f in fits[:nf]) == knots and ref["status"][frame] == 0
    for options in ({}, {"path_mode": 1}, {"path_mode": 2, "pack": 2}):
        ctx = pkg.Context(device=0, params=prm, options=options)
        assert ctx.shapes is pkg.WIDE
        res = ctx.plan_batch(off, cones, poses)
        assert not (res["status"] == 204).any()
        _assert_equal_to_oracle(res, ref)
        ctx.close()
