"""The sorting kernels (csrc/sort_kernel.h, under the host emulator) against the oracle (fsdo_sort_frame, det-math mode) on frames
built for the stage: tests/sort_support.py — a cone 1e-9 (and, for the kernels' shortcuts, 1e-5) either side of every threshold the
stage decides with, cases exactly on a threshold, structural cases, and all of them padded across the routes' size limits.
Standard build, and the wide build with max_n_neighbors = 8, max_length = 16.  Index fields are compared with array_equal,
best_cost_* bit for bit, over every case of a family; no case is filtered anywhere.  CPU-only."""
import ctypes
import functools

import numpy as np
import pytest

import emu_lib
import emu_lib_wide
import oracle_lib
import oracle_lib_wide
import sort_ranked_support as srs
import sort_support as ss

WIDE_PARAMS = dict(max_n_neighbors=8, max_length=16)
BUILDS = {"standard": (emu_lib, oracle_lib, {}, 5, 12), "wide": (emu_lib_wide, oracle_lib_wide, WIDE_PARAMS, 8, 16)}
RAISES = {"start pair beyond max_dist, the first reaches nothing": 102}  # structural cases built to raise: FSDO_REF_UNDEFINED_DFS_OOB
SUFFIXES = (", mirrored", ", colourless")


class _params:
    def __init__(self, build):
        self.emu, self.oracle, self.prm = BUILDS[build][:3]

    def __enter__(self):
        self.ctx = [self.oracle.params(self.prm), self.emu.params(self.prm)] if self.prm else []
        for c in self.ctx:
            c.__enter__()

    def __exit__(self, *a):
        for c in reversed(self.ctx):
            c.__exit__(*a)


def _expected_status(name):
    for k, v in RAISES.items():
        if name.startswith(k):
            return v
    return 0


@functools.lru_cache(maxsize=None)
def _families(build):
    """name -> ([case names], [cases]) of the unpadded families"""
    _emu, _oracle, _prm, k, max_len = BUILDS[build]
    pairs = ss.posed_pairs(k)
    fam = {"pairs": ([f"{n} {m}" for n, _o, _lo, _hi in pairs for m in ("below", "above")], [c for _n, _o, lo, hi in pairs for c in (lo, hi)])}
    for key, named in (("on threshold", ss.on_threshold_posed()), ("structural", ss.structural(max_len))):
        fam[key] = ([n for n, _c in named], [c for _n, c in named])
    return fam


@functools.lru_cache(maxsize=None)
def _unpadded(build):
    """(names, cases, oracle records) of every unpadded family in one list; the oracle's status is 0 on every case but the ones built
    to raise"""
    names, cases = [], []
    for fn, fc in _families(build).values():
        names += fn
        cases += fc
    with _params(build):
        ref = ss.run_oracle(BUILDS[build][1], cases, require_ok=False)
    want = np.array([_expected_status(n) for n in names])
    assert np.array_equal(ref["status"], want), [names[i] for i in np.flatnonzero(ref["status"] != want)[:8]]
    assert (want != 0).sum() == 2  # (the raising case and its mirrored twin)
    ref.setflags(write=False)
    return names, cases, ref


@functools.lru_cache(maxsize=None)
def _padded(build):
    """(names, unpadded cases, padded cases, oracle records of the padded ones); the wide build takes a fixed third"""
    _emu, oracle, _prm, k, max_len = BUILDS[build]
    fam = ss.padded_family(k, max_len)
    if build == "wide":
        fam = fam[::3]
    with _params(build):
        ref = ss.run_oracle(oracle, [p for _n, _c, p in fam], require_ok=False)
    ref.setflags(write=False)
    return [n for n, _c, _p in fam], [c for _n, c, _p in fam], [p for _n, _c, p in fam], ref


def _base_name(name):
    name = name.split(" [")[0]
    for s in SUFFIXES:
        name = name.replace(s, "")
    return name


@pytest.mark.parametrize("build", list(BUILDS))
def test_every_pair_flips_on_the_oracle(build):
    """A condition on the constructors: the two members of EVERY pair — its mirrored and colourless twins, at the canonical pose, at
    a heading within 1e-3 of pi and at a seeded one — differ in the pair's named observable, with status 0 on both.  Where the
    oracle's margin recorder has a class for the predicate, the class's smallest margin on a REL pair is below 1e-8 (1e-7 for the
    arithmetic class, whose largest threshold is a squared distance of 42.25): the members sit where they were meant to."""
    _emu, oracle, _prm, k, _max_len = BUILDS[build]
    pairs = ss.posed_pairs(k)
    assert len(pairs) == 3 * len(ss.all_pairs(k)) and len(ss.all_pairs(k)) >= 2 * len(ss.threshold_pairs(k))
    missed, checked = [], 0
    with _params(build):
        for name, obs, lo, hi in pairs:
            with oracle.margins() as m:
                r = ss.run_oracle(oracle, [lo, hi])  # (asserts status 0)
            if not ss.observable_differs(r[0], r[1], obs):
                missed.append((name, obs))
            cls = ss.MARGIN_CLASS.get(_base_name(name))
            if cls and "(REL)" in name:
                checked += 1
                assert m.min[cls] < ss.MARGIN_BOUND.get(cls, 1e-8), (name, cls, m.min[cls])
    assert not missed, missed
    assert checked > len(pairs) // 2
    print(f"{len(pairs)} pairs flip ({build}); margin classes checked on {checked}")


ROUTES = {
    "sort128": lambda emu, cases: ss.run_emu(emu, cases),
    "sort255": lambda emu, cases: _no_sort128(emu, cases),
    "cached": lambda emu, cases: ss.run_emu_cached(emu, cases),
    "speculative": lambda emu, cases: ss.run_emu_speculative(emu, cases),
}


def _no_sort128(emu, cases):
    emu.lib().emu_set_no_sort128(ctypes.c_int(1))  # (the library's option "no_sort128")
    try:
        return ss.run_emu(emu, cases)
    finally:
        emu.lib().emu_set_no_sort128(ctypes.c_int(0))


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("route", list(ROUTES))
def test_emulated_kernels_equal_oracle(route, build):
    """Pairs, on-threshold and structural cases in ONE launch per route: the 128-cone state, the 255-cone state, the cache-enabled
    instantiation (empty entries: every side is searched) and the speculative one of the cached sequences."""
    names, cases, ref = _unpadded(build)
    with _params(build):
        got = ROUTES[route](BUILDS[build][0], cases)
    ss.assert_equal(got, ref, f"{route} ({build})", names=names)


@pytest.mark.parametrize("build", list(BUILDS))
def test_emulated_ranked_kernels_equal_oracle(build):
    """sort_kernel_128_ranked on the same cases: the records are the oracle's, and every side's configurations and costs (bit for
    bit) are fsdo_side_configs' in its order, the terms adding up to the cost — which covers the cost-only pairs row by row."""
    emu, oracle = BUILDS[build][:2]
    names, cases, ref = _unpadded(build)
    off, cones, poses = ss.as_batch(cases)
    with _params(build):
        got = emu.sort_ranked(off, cones, poses, top_k=64, terms=True)
        ss.assert_equal(got[0], ref, f"ranked ({build})", names=names)
        assert emu.last_kernels() == 1
        with oracle.math_mode(1):
            n_multi, _ties = srs.check_against_oracle(oracle, off, cones, poses, got, 0.0)
    assert n_multi > 20  # sides with a runner-up


def _by_route(padded):
    """indices of the padded cases by the state that holds them: 128 cones, 255 cones, global memory"""
    n = np.array([len(c[0]) for c in padded])
    return {"128": np.flatnonzero(n <= 128), "255": np.flatnonzero((n > 128) & (n <= 255)), "big": np.flatnonzero(n > 255)}


@pytest.mark.parametrize("build", list(BUILDS))
def test_padding_changes_nothing(build):
    """UNKNOWN filler cones 200 m away, up to 64 / 65 (the lane-strided loops), 128 / 129 (the two LDS states), 255 / 256 (LDS against
    global memory) and 300 cones: every field of the record equals the unpadded case's on the oracle, and the kernels return the
    oracle's records on each route the sizes select."""
    emu = BUILDS[build][0]
    names, plain, padded, ref = _padded(build)
    all_names, _cases, all_ref = _unpadded(build)
    assert len({len(c[0]) for c in padded}) == len(ss.PAD_SIZES)
    with _params(build):
        ref_plain = ss.run_oracle(BUILDS[build][1], plain, require_ok=False)
    for i in range(len(names)):
        assert ss.records_equal_but_for_padding(ref[i], ref_plain[i]) is None, (names[i], ss.records_equal_but_for_padding(ref[i], ref_plain[i]))
    for route, idx in _by_route(padded).items():
        assert len(idx) > 10
        with _params(build):
            got = ss.run_emu(emu, [padded[i] for i in idx])
        assert (emu.lib().emu_last_big() > 0) == (route == "big"), route
        if route == "big":
            assert emu.lib().emu_last_big() == len(idx)
        ss.assert_equal(got, ref[idx], f"padded, {route} route ({build})", names=[names[i] for i in idx])


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("route", ["cached", "speculative", "ranked"])
def test_padded_cases_on_the_other_instantiations(route, build):
    """A fixed third of the padded cases through the cache-enabled, the speculative and the ranked kernels (255-cone state and
    global memory in one launch)."""
    emu = BUILDS[build][0]
    names, _plain, padded, ref = _padded(build)
    idx = np.arange(1, len(padded), 3)
    cases = [padded[i] for i in idx]
    with _params(build):
        if route == "ranked":
            got = emu.sort_ranked(*ss.as_batch(cases), top_k=8, terms=False)[0]
            assert emu.last_kernels() & 4
        else:
            got = (ss.run_emu_cached if route == "cached" else ss.run_emu_speculative)(emu, cases)
    assert emu.lib().emu_last_big() > 0
    ss.assert_equal(got, ref[idx], f"padded, {route} ({build})", names=[names[i] for i in idx])
