"""Sequence calls with per-frame global paths, without a GPU: seq_chain_table_kernel (csrc/sequence_table_kernel.h) under the host
SIMT emulator (tests/emu/emu_sequence_table.cpp) behind the speculative pass of the path table wrappers, against every planner of
the constructed recording (tests/sequence_table_support.py) stepped frame by frame on the oracle; the twin against seq_chain_kernel
with one path context-wide; the host part of AccelerationBatch.plan_sequence against the host flow of the planner object with the
oracle as path stage; the four new symbols of the C ABI."""
import importlib
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gpath_table_support as gts
import oracle_lib
import sequence_support as ss
import sequence_table_support as st
import test_global_path as tgp

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def rec():
    return st.Recording()


def test_the_constructed_recording_holds_what_the_tests_need(rec):
    got = rec.preconditions()
    assert all(got.values()), got


def initial_rows(rec):
    """an initial_prev block: a path of its own for every planner, none (NaN) for (d)"""
    init = np.stack([oracle_lib.default_path()] * rec.n)
    init[:, :, 2] += 0.05 * (1 + np.arange(rec.n))[:, None]
    init[st.D] = np.nan
    return init


@pytest.mark.parametrize("form,blocks,with_init", [("mono16", 8, False), ("prep8", 1, True)])
def test_emulated_sequence_with_ids_equals_the_stepped_oracle(rec, form, blocks, with_init):
    assert all(rec.preconditions().values())
    init = initial_rows(rec) if with_init else None
    ref, ref_final, ref_again, _real = rec.stepped(initial_prev=init)
    with oracle_lib.math_mode(1):
        status, out, final, again = st.emu_plan_sequence(rec, initial_prev=init, form=form, blocks=blocks)
    st.check(ref, status, out["path"], out["fallback"], what=form)
    assert final.tobytes() == ref_final.tobytes()
    assert again == ref_again and again > 0
    if with_init:  # (the rows were read: other bytes than without them)
        assert rec.stepped()[0]["path"].tobytes() != ref["path"].tobytes()


def test_twin_with_one_path_equals_the_plain_chain_kernel(rec):
    """all ids = SHORT (five points: quick under the emulator; the cars of (d) and (e) are more than 5 m from its end, those of (f)
    beside it): the bytes of seq_chain_kernel with SHORT as the launch's one pair"""
    ids = np.full(rec.n * rec.T, gts.SHORT, np.int32)
    with oracle_lib.math_mode(1):
        s_t, out_t, final_t, again_t = st.emu_plan_sequence(rec, ids=ids)
        s_p, out_p, final_p, again_p = st.emu_plan_sequence(rec, ids=ids, plain_path=gts.SHORT)
    assert again_t == again_p and again_t > 0
    assert np.array_equal(s_t, s_p) and out_t.tobytes() == out_p.tobytes() and final_t.tobytes() == final_p.tobytes()
    ref, ref_final, ref_again, _ = rec.stepped(ids=ids)
    st.check(ref, s_t, out_t["path"], out_t["fallback"], what="all SHORT")
    assert again_t == ref_again


# ---- AccelerationBatch.plan_sequence: the host part -----------------------------------------------------------------------------------
def acceleration_log(golden_dir, n=3):
    """the golden acceleration recording (30 steps) fed to n planners, step-major"""
    g = np.load(golden_dir / "global_path.npz")
    frames = list(tgp._frames(g, "acc"))
    T = len(frames)
    counts = np.array([len(frames[t][1]) for t in range(T) for _ in range(n)])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    cones = np.concatenate([frames[t][1] for t in range(T) for _ in range(n)])
    poses = np.array([frames[t][2] for t in range(T) for _ in range(n)])
    return g, off, cones, poses, T


def oracle_path_stage(known):
    def stage(pose_k, ids, prev):
        n = len(prev)
        have = prev.copy()
        path = np.zeros((len(pose_k), *prev.shape[1:]))
        status = np.zeros(len(pose_k), np.int32)
        for f in range(len(pose_k)):
            r = oracle_lib.plan_frame_global(np.zeros((0, 3)), pose_k[f], have[f % n], known if ids[f] == 0 else None)
            path[f], status[f] = r["path"], r["status"]
            if r["status"] == 0:
                have[f % n] = r["path"]
        return path, status, have
    return stage


class HostBatch:
    """the state AccelerationBatch keeps, without its context"""

    def __init__(self, acc, seeds):
        self.acc, self.n = acc, len(seeds)
        self.relocalizers = [acc.AccelerationRelocalizer(s) for s in seeds]
        self.reloc, self.angle, self.orig = np.zeros(self.n, bool), np.zeros(self.n), np.zeros((self.n, 2))
        self.prev = np.repeat(oracle_lib.default_path()[None], self.n, axis=0)
        self.stage = oracle_path_stage(acc.known_path())

    def plan_sequence(self, off, cones, poses):
        return self.acc.plan_sequence_on(self.relocalizers, self.reloc, self.angle, self.orig, self.prev, off, cones, poses, self.stage)


def test_acceleration_sequence_host_part_equals_the_planner_objects_host_flow(golden_dir):
    acc = importlib.import_module("ft-fsd-path-planning_amd.acceleration")
    g, off, cones, poses, T = acceleration_log(golden_dir)
    seeds = [int(g["acc_seed"]), int(g["acc_seed"]) + 1, 5]
    n = len(seeds)

    def plan(pose, prev, gp):
        r = oracle_lib.plan_frame_global(np.zeros((0, 3)), pose, prev, gp)
        assert r["status"] == 0
        return r["path"]

    batch = HostBatch(acc, seeds)
    paths, status = batch.plan_sequence(off, cones, poses)
    assert paths.shape == (T, n, 40, 4) and status.shape == (T, n) and (status == 0).all()
    first = []
    for i, seed in enumerate(seeds):
        want, flags, reloc = tgp._accelerate_with(plan, g, seed)
        assert np.array_equal(paths[:, i], want), (i, np.abs(paths[:, i] - want).max())
        assert batch.reloc[i] == reloc.is_relocalized and batch.angle[i] == reloc.angle_to_fix
        # the planner's RandomState stands where the planner object's stands: the next draw is the same
        assert batch.relocalizers[i]._rng.randint(1 << 30) == reloc._rng.randint(1 << 30)
        first.append(int(np.argmax(flags)))
    assert 0 < min(first) < T  # (ids of -1 and of 0 in the one call)
    assert np.abs(paths[:, 0] - g["acc_path"]).max() < 1e-5
    # 12 steps, then 18: the batch continues as if it had been stepped
    cut = HostBatch(acc, seeds)
    k = 12 * n
    p0, s0 = cut.plan_sequence(off[: k + 1], cones[: off[k]], poses[:k])
    p1, s1 = cut.plan_sequence(off[k:] - off[k], cones[off[k] :], poses[k:])
    assert np.array_equal(np.concatenate([p0, p1]), paths) and np.array_equal(np.concatenate([s0, s1]), status)
    assert np.array_equal(cut.prev, batch.prev) and np.array_equal(cut.angle, batch.angle)


def test_abi_exports_the_sequence_calls_with_path_ids():
    pkg = importlib.import_module("ft-fsd-path-planning_amd")
    names = ("fsdp_plan_sequence_paths", "fsdp_plan_sequence_paths_compact", "fsdp_submit_sequence_paths", "fsdp_submit_sequence_paths_compact")
    assert set(names) <= set(pkg._capi.EXPORTED_SYMBOLS)
    header = (ROOT / "include" / "fsdp.h").read_text()
    for name in ("libfsdp_hip.so", "libfsdp_hip_wide.so"):
        lib = ROOT / "ft-fsd-path-planning_amd" / "lib" / name
        assert lib.exists(), f"{lib} missing: run python __graft_entry__.py"
        syms = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
        for sym in names:
            assert f" T {sym}\n" in syms, (name, sym)
            assert f"int {sym}(" in header
    import inspect

    for fn in (pkg.Context.plan_sequence, pkg.Context.submit_sequence, pkg.MultiPlanner.plan_sequence, pkg.MultiPlanner.submit_sequence,
               pkg.replay.replay_stateful_batched):
        assert "path_ids" in inspect.signature(fn).parameters, fn
    assert hasattr(pkg.MultiPlanner, "set_global_path_table") and hasattr(pkg.AccelerationBatch, "plan_sequence")
