"""Pin the CPU oracle (oracle/) against golden vectors captured from the reference
(tests/golden/make_golden.py).  CPU-only."""
import collections

import os
import warnings

import numpy as np
import pytest

import oracle_lib
import oracle_lib_wide
import parity

# parameter sets beyond the standard shapes (max_n_neighbors 8, max_length 16, mpc_prediction_horizon 64: make_golden.py
# --params-r5): held against the oracle built with the wide record shapes (oracle/Makefile liboracle_wide.so)
WIDE_SETS = ["params_wide_sort", "params_wide_horizon", "params_wide_all"]


def _oracle(name):
    return oracle_lib_wide if name in WIDE_SETS else oracle_lib


# big_frames: 300 / 600 cones per frame; lattice: up to 190 end configurations per side (beyond the LDS capacities of
# the product sorting kernel: planned by sort_big_kernel)
SETS = ["scenarios", "cfg2_color", "cfg3_nocolor", "cfg4_200cones", "cfg4_noisy_nocolor", "fuzz", "big_frames", "lattice"]


@pytest.mark.parametrize("mode", [0, 1], ids=["libm", "detmath"])
@pytest.mark.parametrize("name", SETS + ["nonfinite_poses", "nonfinite_cones", "odd_inputs"])  # (a NaN / inf component in the pose: raises for positions, plans for directions; in cones: plans around them)
def test_oracle_matches_reference_golden(golden_dir, name, mode):
    """mode 0: libm sin/cos/atan2 (what NumPy calls); mode 1: det_math.h (what the HIP kernels use)."""
    g = np.load(golden_dir / f"{name}.npz")
    with oracle_lib.math_mode(mode):
        res = oracle_lib.plan_batch(g["offsets"], g["cones"], g["poses"], n_threads=4)
    cats = collections.Counter()
    bad = []
    n_arc = 0
    arc = parity.ArcLibm(golden_dir, name)
    for k in range(len(res)):
        cat, detail = parity.compare_frame(res[k], g, k, arc=arc, math="det" if mode else "libm")
        cats[cat] += 1
        n_arc += bool(int(res[k]["path_fallback"]) & parity.ARC_FLAG)
        if cat in ("IDX", "MATCH", "PATH", "STATUS"):
            bad.append((k, cat, detail))
    assert not bad, bad[:5]
    # sample-count flips only on arc-extension frames, and only a small share of those
    # arc frames: within 1e-5 of the reference at the libm level (compare_frame); a difference from the AVX-512 golden exactly
    # on the frames on which the reference differs from itself (fuzz: 339 and 347), nowhere else
    assert n_arc == len(arc.frames) and cats["flip"] == len(arc.flips("det" if mode else "libm")), (cats, n_arc, arc.flips("det" if mode else "libm"))


def test_default_previous_path(golden_dir):
    """core_calculate_path.py:103-107: the constant initial previous path."""
    ref = np.load(golden_dir / "default_path.npz")["path"]
    assert np.abs(oracle_lib.default_path() - ref).max() < 1e-12


def test_empty_and_tiny_frames():
    """N < 3 cones: both sides have no result (core_trace_sorter.py:272-273) and the path is
    the previous path run through the MPC step (core_calculate_path.py:531-536)."""
    for n in range(0, 3):
        xyt = np.array([[3.0 * i + 2, 1.5, 2.0] for i in range(n)]).reshape(-1, 3)
        r = oracle_lib.plan_frame(xyt, np.array([0.0, 0, 1, 0]))
        assert r["status"] == 0 and r["n_left"] == 0 and r["n_right"] == 0
        assert r["path_fallback"] & 1
        assert np.isfinite(r["path"]).all()


@pytest.mark.parametrize("name", ["params_sort", "params_path", "params_monotonic", "params_deg2", "params_deg1", "params_horizon", "params_no_unknown"] + WIDE_SETS)
def test_oracle_with_non_default_parameters(golden_dir, name):
    """The reference's stage classes constructed with non-default kwargs (fixtures: make_golden.py params_golden): the
    oracle with the same constants (fsdo_set_params) reproduces indices, matches and paths."""
    g = np.load(golden_dir / f"{name}.npz")
    oracle_lib = _oracle(name)
    prm = dict(zip(g["param_names"].tolist(), g["param_values"].tolist()))
    with oracle_lib.params(prm):
        res = oracle_lib.plan_batch(g["offsets"], g["cones"], g["poses"], n_threads=4)
    cats = collections.Counter()
    bad = []
    arc = parity.ArcLibm(golden_dir, name)
    for k in range(len(res)):
        cat, detail = parity.compare_frame(res[k], g, k, arc=arc, math="libm")
        cats[cat] += 1
        if cat in ("IDX", "MATCH", "PATH", "STATUS"):
            bad.append((k, cat, detail))
    assert not bad, bad[:5]
    assert cats["flip"] == len(arc.flips("libm")), (cats, arc.flips("libm"))  # (params_no_unknown: frame 97, where the reference differs from itself)
    # and the defaults are back afterwards
    d = np.load(golden_dir / "cfg2_color.npz")
    r = oracle_lib.plan_batch(d["offsets"][:3], d["cones"][: d["offsets"][2]], d["poses"][:2])
    assert np.array_equal(r["left_idx"][:, :12], d["left_idx"][:2]) and (r["left_idx"][:, 12:] == -1).all()


@pytest.mark.parametrize("name", SETS + ["params_sort", "params_path", "params_monotonic", "params_deg2", "params_deg1", "params_horizon", "params_no_unknown"] + WIDE_SETS)
def test_oracle_splines_match_reference_per_frame(golden_dir, name):
    """Per-stage intermediates of the path stage: every smoothing spline a frame fits — fit #1 of the centre
    points, the refit, the parameterization fit, plus the fallback fits where they happen — captured from the reference's
    scipy.splprep calls inside calculate_path_in_global_frame; the oracle's FITPACK restatement gives the same degree,
    the same knots and the same coefficients, bit for bit, in the same call order."""
    g = np.load(golden_dir / f"{name}.npz")
    oracle_lib = _oracle(name)
    prm = dict(zip(g["param_names"].tolist(), g["param_values"].tolist())) if "param_names" in g else None
    n_frames = n_fits = 0
    with oracle_lib.params(prm or {}):
        for k in range(0, len(g["ok"]), 2 if len(g["ok"]) > 100 else 1):
            if not g["ok"][k]:
                continue
            xyt = g["cones"][g["offsets"][k] : g["offsets"][k + 1]]
            r, nf, fits = oracle_lib.plan_frame_capture(xyt, g["poses"][k])
            if int(r["path_fallback"]) & parity.ARC_FLAG:
                continue  # libm values (atan2 / sin / cos) enter the polyline of the refit on these frames
            assert nf == int(g["n_fits"][k]), (k, nf, int(g["n_fits"][k]))
            for q, (kk, n, t, cx, cy) in enumerate(fits):
                assert kk == int(g["fit_k"][k, q]) and n == int(g["fit_n"][k, q]), (k, q)
                nn = min(n, 48)
                assert np.array_equal(t, g["fit_t"][k, q, :nn]), (k, q, "knots")
                nc = n - kk - 1  # meaningful coefficients (the rest of scipy's array is padding)
                assert np.array_equal(cx[:nc], g["fit_cx"][k, q, :nc]) and np.array_equal(cy[:nc], g["fit_cy"][k, q, :nc]), (k, q, "coefficients")
                n_fits += 1
            n_frames += 1
    assert n_frames > 5 and n_fits >= 3 * n_frames - 3


@pytest.mark.parametrize("name", SETS + ["nonfinite_poses", "nonfinite_cones", "odd_inputs", "params_sort", "params_path", "params_monotonic",
                                         "params_deg2", "params_deg1", "params_horizon", "params_no_unknown"] + WIDE_SETS)
def test_oracle_with_host_libm_is_the_reference_bit_for_bit(golden_dir, name):
    """Every value of every path — arc length, x, y AND curvature, 40 x 4 doubles — of every frame the reference plans, in all
    eighteen golden sets (1 774 frames): the oracle in host-libm mode returns the reference's bits.  On arc-extension frames the
    reference is taken at the libm level of its NumPy (arc_libm_level.npz), elsewhere from the committed goldens (no libm value
    in their float chain but one: the circle fit squares its centre with C pow(), np.float64 ** 2, which host-libm mode
    follows).  What separates the kernels (det mode) from this is therefore libm alone: correctly rounded sin / cos / atan2 and
    x * x where glibc is one bit off."""
    if not parity.host_libm_is_the_fixture_machines(golden_dir):
        msg = "this host's libm returns other last bits than the machine the goldens were captured on"
        if os.environ.get("FSDP_REQUIRE_FIXTURE_LIBM") == "1":
            pytest.fail(msg + " (FSDP_REQUIRE_FIXTURE_LIBM=1)")
        warnings.warn("host-libm bit-for-bit test skipped: " + msg)
        pytest.skip(msg)
    g = np.load(golden_dir / f"{name}.npz")
    oracle_lib = _oracle(name)
    prm = dict(zip(g["param_names"].tolist(), g["param_values"].tolist())) if "param_names" in g else None
    with oracle_lib.math_mode(0):
        if prm:
            with oracle_lib.params(prm):
                res = oracle_lib.plan_batch(g["offsets"], g["cones"], g["poses"], n_threads=4)
        else:
            res = oracle_lib.plan_batch(g["offsets"], g["cones"], g["poses"], n_threads=4)
    arc = parity.ArcLibm(golden_dir, name)
    n = 0
    for k in range(len(res)):
        if not g["ok"][k]:
            continue
        assert int(res[k]["status"]) == 0, k
        ref = arc.path(k) if k in arc else g["path"][k]
        assert np.array_equal(res[k]["path"], ref, equal_nan=True), (k, np.nanmax(np.abs(res[k]["path"] - ref)))
        n += 1
    assert n == int(g["ok"].sum())


def test_oracle_matches_reference_on_degenerate_sides(golden_dir):
    """Sides with coincident cones (match_support.degenerate(); make_golden.py --match-degenerate-only runs the reference's
    ConeMatching stage object on them).  A zero chord makes the reference's search direction 0 / 0; it raises nothing and goes
    on with NaN: the cone finds no match, its virtual cone is NaN, np.min / np.argmin return the NaN, np.argsort puts it last,
    every comparison with it is False.  The oracle returns the reference's lists and matches bit for bit, NaN for NaN —
    except where an exact tie of finite distances is decided by NumPy's unstable argsort (stage_tie, recorded by the generator:
    coincident cones among the EXISTING cones of an insertion are equally far from everything), where the reference's result
    belongs to its NumPy build, like first_k_tie / knn_tie of the frame sets."""
    import match_support

    g = np.load(golden_dir / "match_degenerate.npz")
    named = match_support.degenerate()
    assert [n for n, _c in named] == g["stage_names"].tolist()
    assert g["stage_ok"].all() and 3 * int(g["stage_tie"].sum()) < len(named)  # the reference raised nowhere; most cases are pinned
    n_nan = 0
    for k, (name, (left, right, pose)) in enumerate(named):
        assert np.array_equal(left, g["stage_left"][k, : g["stage_n_left"][k]]) and np.array_equal(right, g["stage_right"][k, : g["stage_n_right"][k]])
        assert np.array_equal(pose, g["stage_poses"][k])
        r = oracle_lib.match(left, right, pose)
        assert int(r["status"]) == 0, name
        if g["stage_tie"][k]:
            continue
        for f in ("n_left_v", "n_right_v", "left_v", "right_v", "l2r", "r2l"):
            assert np.array_equal(r[f], g["stage_" + f][k], equal_nan=True), (name, f, r[f], g["stage_" + f][k])
        n_nan += bool(np.isnan(r["left_v"]).any() or np.isnan(r["right_v"]).any())
    assert n_nan >= 20  # NaN virtual cones are what this pins


@pytest.mark.parametrize("mode", [0, 1], ids=["libm", "detmath"])
def test_oracle_matches_reference_on_duplicated_cone_frames(golden_dir, mode):
    """64 frames with one cone reported twice, through the reference's whole planner (match_degenerate.npz plan_*).  Which of
    the two twins a sorted side names is the reference's unstable argsort's choice (every frame has knn_tie): the sides are
    compared by coordinates, everything after them as usual."""
    g = np.load(golden_dir / "match_degenerate.npz")
    off, cones, poses = g["plan_offsets"], g["plan_cones"], g["plan_poses"]
    assert g["plan_ok"].all()
    with oracle_lib.math_mode(mode):
        res = oracle_lib.plan_batch(off, cones, poses, n_threads=4)
    assert (res["status"] == 0).all()
    for k in range(len(res)):
        xy = cones[off[k] : off[k + 1], :2]
        for s in ("left", "right"):
            n = int(g[f"plan_n_{s}"][k])
            assert int(res[f"n_{s}"][k]) == n, (k, s)
            assert np.array_equal(xy[res[f"{s}_idx"][k][:n]], xy[g[f"plan_{s}_idx"][k][:n]]), (k, s)
        for f in ("n_left_v", "n_right_v", "left_v", "right_v", "l2r", "r2l"):
            assert np.array_equal(res[f][k], g["plan_" + f][k], equal_nan=True), (k, f)
        p, q = res["path"][k], g["plan_path"][k]
        e = float(np.nanmax(np.abs(p - q)))
        assert e <= parity.PATH_TOL or (int(res["path_fallback"][k]) & parity.ARC_FLAG and parity.is_sample_count_flip(p, q)), (k, e)


@pytest.mark.parametrize("mode", [0, 1], ids=["libm", "detmath"])
def test_oracle_matches_reference_on_constructed_sorting_frames(golden_dir, mode):
    """The constructed frames of the sorting stage (tests/sort_support.py: every member of every threshold pair at the canonical pose
    with its mirrored and colourless twins, the on-threshold and the structural cases) through the reference's planner
    (make_golden.py --sort-constructed-only): the oracle returns the reference's sorted sides, start cones, configuration counts and
    best costs on ALL of them — the members 1e-9 either side of a threshold included, so oracle and reference decide every pair the
    same way — but for the frames named in tie_names (an exact tie in one of the reference's unstable argsorts: built as such),
    which are held to the final sides only.  Where the reference raises in the sorting stage, the oracle raises."""
    import sort_support as ss

    g = np.load(golden_dir / "sort_constructed.npz")
    named = []
    for name, _obs, lo, hi in ss.all_pairs():
        named += [(name + " below", lo), (name + " above", hi)]
    named += ss.on_threshold() + [(n + ", mirrored", ss.mirrored(c)) for n, c in ss.on_threshold()] + ss.structural()
    assert [n for n, _c in named] == g["names"].tolist()
    off, cones, poses = ss.as_batch([c for _n, c in named])
    assert np.array_equal(off, g["offsets"]) and np.array_equal(cones, g["cones"]) and np.array_equal(poses, g["poses"])
    ties = set(g["tie_names"].tolist())
    assert ties == {n for n in g["names"].tolist() if "tie" in n or n.startswith("combine: colourless")}, sorted(ties)
    print(f"{len(named)} frames, {len(ties)} named argsort ties")
    with oracle_lib.math_mode(mode):
        res = np.array([oracle_lib.sort_frame(*c) for _n, c in named])
    for k, (name, _c) in enumerate(named):
        r = res[k]
        if not g["sort_ok"][k]:
            assert str(g["exc"][k]) == "IndexError" and int(r["status"]) == 102, (name, g["exc"][k], int(r["status"]))
            continue
        assert int(r["status"]) == 0, name
        for s in ("left", "right"):
            n = int(g[f"n_{s}"][k])
            assert int(r[f"n_{s}"]) == n and np.array_equal(r[f"{s}_idx"][:n], g[f"{s}_idx"][k][:n]), (name, s, r[f"{s}_idx"], g[f"{s}_idx"][k])
            if name in ties:
                continue
            assert np.array_equal(r[f"first_k_{s}"], g[f"first_k_{s}"][k]), (name, s, r[f"first_k_{s}"], g[f"first_k_{s}"][k])
            assert int(r[f"n_configs_{s}"]) == int(g[f"n_configs_{s}"][k]), (name, s, int(r[f"n_configs_{s}"]), int(g[f"n_configs_{s}"][k]))
            if g[f"n_configs_{s}"][k] > 0:
                a, b = float(r[f"best_cost_{s}"]), float(g[f"best_cost_{s}"][k])
                assert abs(a - b) <= 1e-9 * max(1.0, abs(b)), (name, s, a, b)  # (the bar of parity.compare_frame)


@pytest.mark.parametrize("mode", [0, 1], ids=["libm", "detmath"])
def test_oracle_matches_reference_on_constructed_path_inputs(golden_dir, mode):
    """tests/path_support.py's canonical cases of families A-E (every branch of the path stage, both members of every threshold pair)
    through the reference's CalculatePath (make_golden.py path_constructed_golden): the oracle raises where the reference raises,
    with the status the case was built for, and gives its path elsewhere, within the 1e-5 this file holds paths to (the arc
    extension's libm values; 0 is expected outside arc frames and printed).  The cases are rebuilt from their names: none may be missing."""
    import path_support as ps

    g = np.load(golden_dir / "path_constructed.npz")
    cases = {c.name: c for fam in "ABCDE" for c in ps.everything()[fam][0]}
    canonical = {n for n, c in cases.items() if ps.canonical(c)}
    assert len(g["names"]) >= 250 and set(g["names"].tolist()) == canonical, sorted(canonical ^ set(g["names"].tolist()))[:5]  # none unpinned
    rows = g["rows"]
    worst = worst_plain = 0.0
    for k, name in enumerate(g["names"]):
        c = cases[name]
        with oracle_lib.params(c.prm), oracle_lib.math_mode(mode):
            r = oracle_lib.path(c.lv, c.rv, c.l2r, c.r2l, c.pose, prev=ps._pad_prev(oracle_lib, c.prev), global_path=c.gpath)
        if not g["ok"][k]:
            # (IndexError: a match index outside the other side, 104 — family A — or cumsum([])[-1] of a single point in front, 103)
            assert r["status"] == (104 if g["exc"][k] == "IndexError" and name.startswith("A/") else 103), (name, int(r["status"]), str(g["exc"][k]))
            assert c.expect in (None, int(r["status"])), (name, c.expect)
            continue
        assert r["status"] == 0 and c.expect in (None, 0), (name, int(r["status"]), c.expect)
        want = g["paths"][g["path_of"][k]]
        h = int(c.prm.get("mpc_prediction_horizon", 40))
        got = r["path"][rows]
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(r["path"][h:]).all(), name  # (an exactly straight path: NaN curvature, in both)
        err = float(np.nan_to_num(np.abs(got - want)).max())
        assert err <= 1e-5, (name, err)
        worst = max(worst, err)
        if not int(r["path_fallback"]) & parity.ARC_FLAG:
            worst_plain = max(worst_plain, err)
    print(f"constructed path inputs, mode {mode}: {int(g['ok'].sum())} paths, max |oracle - reference| = {worst:.3e} ({worst_plain:.3e} outside arc frames)")


# exact distance ties among n > 16 cones: which of two equally distant cones comes first is NumPy's introsort's business (the oracle
# sorts stably); the subsets then get each other's noise.  Final results only, within SKIDPAD_UNSTABLE_TOL: the noise moves a cone by
# 1e-3 m (sigma; 4e-3 at most), a three-cone fit at 2.4 m spacing amplifies that by about (radius / chord)^2 = 2.5 for the centre, so
# a cluster median moves by less than 1e-2 m: the translation by 1e-2 m, the rotation by 2e-2 / 18.25 rad, which over the 40 m lever
# of the farthest path point is another 4.4e-2 m.
SKIDPAD_UNSTABLE_TOL = 1e-2 + 4.4e-2
# Of the seven cases built with equal keys, NumPy's order is another than the stable one on three (SKIDPAD_ORDER_DIFFERS; measured against
# the fixture: information and path differ by 1.7e-3, 9.9e-4 and 5.6e-3 — the bound has a factor of ten in hand); on the other four it is
# the stable order, and they are held to the usual bounds.  The window index is the reference's on all seven.
SKIDPAD_ORDER_DIFFERS = ("ties-reversed", "ties-shuffled", "ties-64-apart")
SKIDPAD_UNSTABLE_SORT = ("ties-interleaved", "ties-reversed", "ties-shuffled", "tie-20-21", "tie-20-21-swapped", "ties-64-apart", "pose-inf-x-later")


def test_oracle_matches_reference_on_constructed_skidpad_sequences(golden_dir):
    """tests/golden/skidpad_constructed.npz = the reference itself (a PathPlanner(MissionTypes.skidpad) per case, exceptions caught) on
    the canonical-frame cases of tests/skidpad_constructed_support.py, families A-F, both members of every threshold pair: the oracle
    (libm mode) raises where the reference raises, relocalizes at the same step, holds the same window index after every step —
    raising ones included —, reports the relocalization information within 1e-12 and the path within 1e-5 (the bounds of
    tests/test_skidpad_cpu.py)."""
    import skidpad_constructed_support as sc

    g = np.load(golden_dir / "skidpad_constructed.npz")
    cases = [c for c in sc.build()[0] if c.frame == "canonical"]
    assert [c.name for c in cases] == g["names"].tolist()
    f = 0
    loose = 0
    for k, c in enumerate(cases):
        assert c.unstable_sort == (c.name.split(" [")[0] in SKIDPAD_UNSTABLE_SORT)
        unstable = c.name.split(" [")[0] in SKIDPAD_ORDER_DIFFERS
        assert not unstable or c.unstable_sort
        res = sc.run_oracle(c, mode=0)
        for s, ((xyt, pose), (r, info, index, _, _)) in enumerate(zip(c.steps, res)):
            assert (g["case_of"][f], g["step_of"][f]) == (k, s)
            assert np.array_equal(g["cones"][g["offsets"][f] : g["offsets"][f + 1]], xyt, equal_nan=True) and np.array_equal(g["poses"][f], pose, equal_nan=True), c.name
            tag = (c.name, s, str(g["exc"][f]))
            assert (int(r["status"]) == 0) == bool(g["ok"][f]), tag
            assert index == int(g["index_along_path"][f]), tag
            if g["ok"][f]:
                assert bool(info[0]) == bool(g["relocalized"][f]), tag
                tol_info, tol_path = (1e-12, 1e-5) if not unstable else (SKIDPAD_UNSTABLE_TOL, SKIDPAD_UNSTABLE_TOL)
                loose += unstable
                if g["relocalized"][f]:
                    assert np.abs(info[1:4] - g["info"][f]).max() < tol_info, tag
                assert np.array_equal(np.isnan(r["path"]), np.isnan(g["path"][f])), tag
                assert np.nanmax(np.abs(r["path"] - g["path"][f])) <= tol_path, tag
            f += 1
    assert f == len(g["ok"]) and loose == len(SKIDPAD_ORDER_DIFFERS)
