"""fsdp_plan_sequence without a GPU: the chain kernels of csrc/sequence_kernel.h under the host SIMT emulator
(tests/emu/emu_sequence.cpp) against the reference fixture (tests/golden/sequence_chain.npz: three PathPlanner(trackdrive)
objects x 40 steps, make_golden_sequence.py) and against the oracle stepped along the same chains; the run-head rule against
its host restatement; the two new symbols of the C ABI."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_lib
import sequence_support as ss

ROOT = Path(__file__).resolve().parent.parent
FB_ARC = 16  # FSDP_FB_ARC_EXTENSION: the frames whose path goes through the device's own libm level (arc_libm_level.npz)


@pytest.fixture(scope="module")
def chain(golden_dir):
    g = ss.fixture(golden_dir)
    with oracle_lib.math_mode(1):
        emu = ss.emu_plan_sequence(g["offsets"], g["cones"], g["poses"], int(g["n_planners"]))
        ref = ss.lockstep(ss.oracle_step, g["offsets"], g["cones"], g["poses"], int(g["n_planners"]), oracle_lib.default_path())
    return g, emu, ref


def test_fixture_holds_every_pattern(chain):
    g, (res, _final, _again), _ref = chain
    got = ss.fixture_patterns(g)
    assert all(got.values()), got
    # ... and the emulated pass sees the same flags the fixture recorded
    assert np.array_equal((res["path_fallback"] & ss.FB_READ_PREVIOUS) != 0, (g["fallback"] & ss.FB_READ_PREVIOUS) != 0)


def test_emulated_sequence_equals_reference_planners(chain):
    g, (res, _final, _again), _ref = chain
    assert np.array_equal(res["status"] == 0, g["ok"])
    ok = g["ok"]
    err = np.abs(res["path"][ok] - g["path"][ok]).max(axis=(1, 2))
    plain = (res["path_fallback"][ok] & FB_ARC) == 0
    print("L-inf per frame vs the reference: max", err.max(), "outside arc frames", err[plain].max(), "arc frames", int((~plain).sum()))
    assert err.max() <= 1e-9
    assert plain.any() and err[plain].max() == 0.0  # (outside the arc extension the emulated kernels give the reference's own bits)
    assert np.isnan(res["path"][~ok]).all()


def test_emulated_sequence_equals_oracle_stepped_with_prev(chain):
    g, (res, final, again), (ref, ref_final, ref_again) = chain
    assert np.array_equal(res["status"], ref["status"]) and np.array_equal(res["path_fallback"], ref["path_fallback"])
    assert res["path"].tobytes() == ref["path"].tobytes()
    assert final.tobytes() == ref_final.tobytes()
    assert again == ref_again and again > 0
    # the chain matters: without it (every frame a fresh planner) flagged frames get other paths
    with oracle_lib.math_mode(1):
        fresh = oracle_lib.plan_batch(g["offsets"], g["cones"], g["poses"])
    assert fresh["path"].tobytes() != ref["path"].tobytes()


def test_emulated_sequence_packed_speculation_and_initial_prev(chain):
    """the speculative pass through the packed kernels (16 lanes per frame), one wavefront for every run, and an initial_prev
    with one NaN row: planner 1 drops out at step 0 and reads its row, planner 2's flagged step 1 meets none and stands"""
    g, _emu, _ref = chain
    n = int(g["n_planners"])
    steps = 20  # (the first half of the fixture: the drop-out at step 0, the raise at step 0, two runs)
    off, poses = g["offsets"][: steps * n + 1], g["poses"][: steps * n]
    init = np.stack([oracle_lib.default_path()] * n)
    init[1, :, 1] += 0.25
    init[2] = np.nan
    with oracle_lib.math_mode(1):
        res, final, again = ss.emu_plan_sequence(off, g["cones"], poses, n, initial_prev=init, group=16, blocks=1)
        ref, ref_final, ref_again = ss.lockstep(ss.oracle_step, off, g["cones"], poses, n, oracle_lib.default_path(), initial_prev=init)
    assert np.array_equal(res["status"], ref["status"]) and res["path"].tobytes() == ref["path"].tobytes()
    assert final.tobytes() == ref_final.tobytes() and again == ref_again
    assert res["path"][1].tobytes() != _emu[0]["path"][1].tobytes()  # (the row was read)


def test_run_heads_equal_host_restatement():
    rng = np.random.default_rng(7)
    seen = 0
    for _ in range(200):
        n, T = int(rng.integers(1, 5)), int(rng.integers(1, 25))
        flagged = rng.random(n * T) < rng.choice([0.1, 0.4, 0.8])
        status = np.where(rng.random(n * T) < 0.25, rng.choice([1, 2, 203, ss.ST_RETRY], n * T), 0).astype(np.int32)
        fallback = (np.where(flagged, rng.choice([1, 2, 4, 8, 5, 9], n * T), 0) | rng.choice([0, 16, 32], n * T)).astype(np.int32)
        want = ss.host_heads(status, fallback, n)
        assert ss.emu_heads(status, fallback, n) == want, (n, T, status, fallback)
        seen += len(want)
    assert seen > 200
    # more than one wavefront of frames, and the wide build's kernels
    n, T = 4, 70
    status = np.where(rng.random(n * T) < 0.2, 1, 0).astype(np.int32)
    fallback = np.where(rng.random(n * T) < 0.3, 1, 0).astype(np.int32)
    assert ss.emu_heads(status, fallback, n) == ss.host_heads(status, fallback, n)
    assert ss.emu_heads(status, fallback, n, wide=True) == ss.host_heads(status, fallback, n)


def test_abi_exports_the_sequence_calls():
    pkg = __import__("importlib").import_module("ft-fsd-path-planning_amd")
    assert {"fsdp_plan_sequence", "fsdp_plan_sequence_compact"} <= set(pkg._capi.EXPORTED_SYMBOLS)
    header = (ROOT / "include" / "fsdp.h").read_text()
    for name in ("libfsdp_hip.so", "libfsdp_hip_wide.so"):
        lib = ROOT / "ft-fsd-path-planning_amd" / "lib" / name
        assert lib.exists(), f"{lib} missing: run python __graft_entry__.py"
        syms = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
        for sym in ("fsdp_plan_sequence", "fsdp_plan_sequence_compact"):
            assert f" T {sym}\n" in syms, (name, sym)
            assert f"int {sym}(" in header
