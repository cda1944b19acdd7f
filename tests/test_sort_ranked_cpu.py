"""Ranked sorting candidates (include/fsdp.h fsdp_sort_batch_ranked) without a GPU: the ranked kernel sources under the host
SIMT emulator (tests/emu/emu_ranked.cpp) against the oracle's side_configs and the reference capture tests/golden/sort_ranked.npz,
bit for bit (same libm: the equality tests/test_kernel_logic_emulated.py applies to best_cost_*); the fixture; the exported
symbol and the host-side helpers."""
import ctypes
import importlib
from pathlib import Path

import numpy as np
import pytest

import emu_lib
import emu_lib_wide
import oracle_lib
import oracle_lib_wide
import sort_ranked_support as sup

ROOT = Path(__file__).resolve().parent.parent
EMU_RTOL = 0.0  # parity.assert_intermediates_equal's default: bit-equal costs under the emulator
GPU_RTOL = 1e-12  # tests/test_gpu_parity.py:82


def emu_run(lib):
    return lambda off, cones, poses, top_k=64, terms=True: lib.sort_ranked(off, cones, poses, top_k, terms)


def emu_plain(lib):
    def plain(off, cones, poses):
        s = lib.sort(off, cones, poses)
        lib.lib().emu_sort_remap(ctypes.c_int(len(s)), ctypes.c_void_p(s.ctypes.data))
        return s

    return plain


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return sup.fixture_batches(golden_dir)


def test_fixture_holds_what_it_was_made_for(fixture):
    g, batches = fixture
    src = g["source"].tolist()
    assert src.count("scenarios") == 25 and src.count("cfg2_color") == 24 and src.count("cfg3_nocolor") == 8
    for name, first in (("scenarios", 25), ("cfg2_color", 24), ("cfg3_nocolor", 8)):
        assert g["source_frame"][g["source"] == name].tolist() == list(range(first))
    assert (g["exc"] == "ok").all() and g["terms"].shape == (len(g["costs"]), 7) and (g["terms"][:, 4] == 0).all()
    assert g["terms_libm"].shape == g["terms"].shape and sup.close(g["terms"], g["terms_libm"], 1e-15) and sup.close(g["costs"], g["costs_libm"], 1e-15)
    assert int((g["n_rows"] > 1).sum()) >= 8 and g["n_rows"].max() > 32  # sides with runners-up, some of them long
    for k in range(len(g["n_rows"])):
        for s in range(2):
            c = g["costs"][g["row_off"][k, s] : g["row_off"][k, s] + g["n_rows"][k, s]]
            assert (np.diff(c) >= 0).all()  # sorted by cost
    assert (ROOT / "tests" / "golden" / "sort_ranked.npz").stat().st_size < 256 * 1024


@pytest.mark.parametrize("no_sort128", [False, True])
def test_emulated_ranking_equals_oracle_and_reference_terms(fixture, no_sort128):
    """items 1-3 on the frames of sort_ranked.npz; no_sort128: the 255-cone state for every frame"""
    g, batches = fixture
    e = emu_lib
    e.lib().emu_set_no_sort128(ctypes.c_int(int(no_sort128)))
    kernels, multi, ties, rows, left_out = 0, 0, 0, 0, 0
    try:
        for frames, off, cones, poses in batches:
            got = e.sort_ranked(off, cones, poses, 64, True)
            kernels |= e.last_kernels()
            with oracle_lib.math_mode(1):
                m, t = sup.check_against_oracle(oracle_lib, off, cones, poses, got, EMU_RTOL)
            multi, ties = multi + m, ties + t
            # bit for bit the reference at the libm level of NumPy's dispatch (the libm the emulated kernels call); its default
            # dispatch (NumPy's own arctan2 / arccos) differs from that in a last bit: the GPU test's bound holds there
            r, o = sup.check_terms_against_fixture(g, frames, got, EMU_RTOL, "_libm")
            rows, left_out = rows + r, left_out + o
            assert sup.check_terms_against_fixture(g, frames, got, GPU_RTOL) == (r, o)
            sup.check_call_invariants(emu_run(e), emu_plain(e), off, cones, poses, got)
    finally:
        e.lib().emu_set_no_sort128(ctypes.c_int(0))
    assert multi >= 8 and rows >= 300 and left_out <= 2  # (two sides of the hairpin scenarios' colourless variants: knn_tie)
    assert kernels & 2 and bool(kernels & 1) != no_sort128  # sort_kernel_ranked ran; sort_kernel_128_ranked unless switched off


def test_emulated_big_route(golden_dir):
    """two frames of big_frames.npz (300 cones) and a lattice frame with more than 64 raw end configurations:
    sort_big_kernel_ranked, where a side can hold more candidates than the 64 rows a call stores"""
    e = emu_lib
    _, off, cones, poses = sup.npz_batch(golden_dir, "big_frames", (0, 1))
    got = e.sort_ranked(off, cones, poses, 64, True)
    assert e.last_kernels() & 4 and e.lib().emu_last_big() == 2
    with oracle_lib.math_mode(1):
        sup.check_against_oracle(oracle_lib, off, cones, poses, got, EMU_RTOL)
    sup.check_call_invariants(emu_run(e), emu_plain(e), off, cones, poses, got)
    _, off, cones, poses = sup.npz_batch(golden_dir, "lattice", (5,))
    got = e.sort_ranked(off, cones, poses, 64, True)
    assert e.lib().emu_last_big() == 1 and got[1].max() > 64  # the count is never truncated
    with oracle_lib.math_mode(1):
        multi, _ = sup.check_against_oracle(oracle_lib, off, cones, poses, got, EMU_RTOL)
    assert multi == 2
    sup.check_call_invariants(emu_run(e), emu_plain(e), off, cones, poses, got)


def test_emulated_wide_build(golden_dir):
    """the first 8 frames of params_wide_sort.npz on the wide shapes against the oracle's wide build"""
    g, off, cones, poses = sup.npz_batch(golden_dir, "params_wide_sort", range(8))
    prm = dict(zip(g["param_names"].tolist(), g["param_values"].tolist()))
    e = emu_lib_wide
    with e.params(prm):
        got = e.sort_ranked(off, cones, poses, 64, True)
        assert got[2].shape[-1] == 16
        with oracle_lib_wide.params(prm), oracle_lib_wide.math_mode(1):
            sup.check_against_oracle(oracle_lib_wide, off, cones, poses, got, EMU_RTOL)
        sup.check_call_invariants(emu_run(e), emu_plain(e), off, cones, poses, got)


def test_emulated_without_unknown_cones(golden_dir):
    """item 4: use_unknown_cones = False — indices point at the caller's non-UNKNOWN cones, rows equal the oracle's on the
    filtered array, as coordinates"""
    off, cones, poses = sup.retyped_unknown(golden_dir)
    views = sup.filtered_views(off, cones)
    prm = dict(use_unknown_cones=0)
    e = emu_lib
    with e.params(prm):
        got = e.sort_ranked(off, cones, poses, 64, True)
        with oracle_lib.params(prm), oracle_lib.math_mode(1):
            sup.check_against_oracle(oracle_lib, off, cones, poses, got, EMU_RTOL, oracle_cones=views)
            check_filtered_coordinates(oracle_lib, off, cones, poses, got, views)
        sup.check_call_invariants(emu_run(e), emu_plain(e), off, cones, poses, got)


def check_filtered_coordinates(oracle, off, cones, poses, got, views):
    _res, counts, configs, _costs, _terms = got
    stored = 0
    for f in range(len(poses)):
        xyt = cones[off[f] : off[f + 1]]
        for s, t in enumerate(sup.SIDE_TYPES):
            c, ocfg, _oc, _fk = oracle.side_configs(views[f][0], poses[f], t, 64)
            for r in range(min(int(counts[f, s]), 64)):
                idx = configs[f, s, r][configs[f, s, r] >= 0]
                assert (xyt[idx, 2] != 0).all()
                assert np.array_equal(xyt[idx], views[f][0][ocfg[r][ocfg[r] >= 0]])
                stored += 1
    assert stored >= 8  # (with a third of the cones gone many sides have no result: the rest is what this checks)


def test_emulated_refuses_top_k_outside_the_range(golden_dir):
    _, off, cones, poses = sup.npz_batch(golden_dir, "cfg2_color", (0,))
    for k in (0, 65, -1):
        with pytest.raises(ValueError):
            emu_lib.sort_ranked(off, cones, poses, k)


def test_decision_margin_and_symbols():
    pkg = importlib.import_module("ft-fsd-path-planning_amd")
    assert "fsdp_sort_batch_ranked" in pkg._capi.EXPORTED_SYMBOLS
    header = (ROOT / "include" / "fsdp.h").read_text()
    assert "#define FSDP_RANK_MAX 64" in header and "#define FSDP_COST_TERMS 7" in header and "fsdp_sort_batch_ranked" in header
    assert (pkg._capi.RANK_MAX, pkg._capi.COST_TERMS, len(pkg._capi.COST_TERM_NAMES)) == (64, 7, 7)
    costs = np.array([[[2.0, 3.0, np.nan], [0.0, 1e-310, 5.0]], [[4.0, np.nan, np.nan], [np.nan, np.nan, np.nan]]])
    m = pkg.decision_margin(costs)
    assert m.shape == (2, 2) and m[0, 0] == 0.5 and m[0, 1] == 1e-310 / 1e-300 and np.isinf(m[1]).all()
    assert np.isinf(pkg.decision_margin(np.array([[1.0]]))).all()
    for name in ("libfsdp_hip.so", "libfsdp_hip_wide.so"):  # both builds export the entry point
        lib = ROOT / "ft-fsd-path-planning_amd" / "lib" / name
        assert lib.exists(), f"{name}: run __graft_entry__.build()"
        assert hasattr(ctypes.CDLL(str(lib)), "fsdp_sort_batch_ranked")
