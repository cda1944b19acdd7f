"""The path stage's kernels (csrc/path_kernel.h, spline_device.h, under the host emulator) against the oracle in det mode on the inputs
of tests/path_support.py: a case at every branch of the stage and a pair of cases 1e-9 either side of every threshold, each with its
mirrored twin at three poses, a subset in map-frame coordinates.  Every lane-group size of emu_lib.PATH_GROUP_SIZES, the wide
build, max_deg 1 and 2 (family B), predict_every and mpc_prediction_horizon other than the default (family D).

The bar is the emulator's everywhere in this suite: status, path_fallback, n_dense, the NaN pattern and every path value bit for bit.
No case is skipped; every pair is proved on the oracle's own record of the decision value (path_support.Pair.check).  CPU-only."""
import numpy as np
import pytest

import emu_lib
import path_support as ps

FAMILIES = ("A", "B", "C", "D", "E", "F")
# every case runs on 8, 64 (the one-kernel stage, packed and whole wavefront), 1004 (three kernels, four-lane fit) and, through the
# frames those hand on, the exact route; the other group sizes run one family each — the pose thresholds at 16 lanes, the
# parameterisation through the other two three-kernel forms, the global paths through the 32-knot kernels their contexts launch
# (a frame costs the emulator 25 ms at 8 lanes and 0.2 s at 64)
THIN = {16: ("C",), 1008: ("D",), 1016: ("D",), 2008: ("E",)}
RUNS = [(f, g) for g in emu_lib.PATH_GROUP_SIZES for f in FAMILIES if g not in THIN or f in THIN[g]]


def _assert_equal(got, rows, recs, cases, what):
    rows = ps.expected(rows, recs)
    assert np.array_equal(got["status"], rows["status"]), (what, [(cases[i].name, int(got["status"][i]), int(rows["status"][i])) for i in np.flatnonzero(got["status"] != rows["status"])[:6]])
    ok = rows["status"] == 0
    bad = np.flatnonzero(got["fallback"][ok] != rows["path_fallback"][ok])
    assert len(bad) == 0, (what, [(cases[np.flatnonzero(ok)[i]].name, int(got["fallback"][ok][i]), int(rows["path_fallback"][ok][i])) for i in bad[:6]])
    n_dense = np.array([int(r["n_dense"]) if s == 0 else 0 for r, s in zip(recs, rows["status"])])
    assert np.array_equal(got["n_dense"], n_dense), (what, [cases[i].name for i in np.flatnonzero(got["n_dense"] != n_dense)[:6]])
    want = rows["path"]
    diff = [i for i in range(len(cases)) if not np.array_equal(got["path"][i], want[i], equal_nan=True)]
    assert not diff, (what, len(diff), [(cases[i].name, float(np.nanmax(np.abs(got["path"][i] - want[i])))) for i in diff[:6]])


@pytest.mark.parametrize("family,group", RUNS, ids=[f"{f}-{g}" for f, g in RUNS])
def test_kernels_equal_the_oracle(family, group):
    o, e = ps.libs()
    cases, _pairs = ps.everything()[family]
    rows, recs = ps.reference()[family]
    _assert_equal(ps.run_emu(o, e, cases, group), rows, recs, cases, f"family {family}, group {group}")


@pytest.mark.parametrize("family,group", [(f, 8) for f in FAMILIES] + [("C", 1004)], ids=lambda v: str(v))
def test_kernels_equal_the_oracle_wide_build(family, group):
    """PATH_POINTS = 64, MAX_MATCH = 32, 200 dense samples: the same families built for those shapes, eight lanes per frame; the pose
    thresholds also through the three kernels"""
    o, e = ps.libs(wide=True)
    cases, _pairs = ps.everything(True)[family]
    rows, recs = ps.reference(True)[family]
    _assert_equal(ps.run_emu(o, e, cases, group), rows, recs, cases, f"family {family}, group {group}, wide")


@pytest.mark.parametrize("wide", [False, True], ids=["standard", "wide"])
def test_every_pair_straddles_its_threshold(wide):
    """On the oracle: the recorded decision value lies within the pair's distance of the threshold on both sides, on opposite sides,
    and the decision it is named after flips."""
    o, _ = ps.libs(wide)
    n = 0
    for _family, (_cases, pairs) in ps.everything(wide).items():
        for p in pairs:
            p.check(o)
            n += 1
    assert n >= 100


@pytest.mark.parametrize("wide", [False, True], ids=["standard", "wide"])
def test_statuses_are_the_expected_ones(wide):
    """The oracle's status is 0 except on the cases built to raise, each of which gives its expected status; at least 90 % of all
    cases have status 0.  (expect None: a caller's previous path that raises as well, a track at 1e17, a polyline of the FITPACK
    search — whatever the oracle gives.)"""
    total = good = 0
    for family, (cases, _pairs) in ps.everything(wide).items():
        rows, _ = ps.reference(wide)[family]
        for c, r in zip(cases, rows):
            assert c.expect is None or r["status"] == c.expect, (c.name, int(r["status"]), c.expect)
        total, good = total + len(cases), good + int((rows["status"] == 0).sum())
    assert good >= 0.9 * total, (good, total)


def test_on_threshold_cases_sit_on_their_threshold():
    """The cases built exactly ON a threshold: the oracle's record reads the threshold bit for bit (`>` against `>=`)."""
    n = 0
    for family, (cases, _pairs) in ps.everything().items():
        for c, r in zip(cases, ps.reference()[family][1]):
            if c.on is not None:
                assert r[c.on[0]] == c.on[1], (c.name, c.on, r[c.on[0]])
                n += 1
    assert n >= 21


def test_coverage_of_the_stage():
    """What the issue's tally of the sampled fixtures lacked, counted on the oracle's records of these cases."""
    o, _ = ps.libs()
    lines, fallbacks, branches = ps.table()
    for line in lines:
        print("family %s: %d cases, %d pairs, %d on-threshold, %d raising" % line)
    print("path_fallback values:", fallbacks)
    print("parcur_fit branches:", branches)
    assert {0, 1, 2, 4, 5, 8, 16, 32, 33, 1 | 16, 4 | 16, 4 | 32, 2 | 4 | 16, 8 | 16} <= set(fallbacks), fallbacks
    assert set(branches) == set(o.FIT_BRANCHES) - {"ier1", "interpolant"}, sorted(set(o.FIT_BRANCHES) - set(branches))
    # a fresh planner (no caller's previous path) never extends its default previous path: 4 | 16, 4 | 32 and 1 | 16 stay unreached there
    fresh = {int(r["path_fallback"]) for f, (cases, _p) in ps.everything().items() for c, r in zip(cases, ps.reference()[f][0]) if c.prev is None and r["status"] == 0}
    assert not fresh & {4 | 16, 4 | 32, 1 | 16}, sorted(fresh)
    recs = [r for f in ps.reference().values() for r, s in zip(f[1], f[0]["status"]) if s == 0]
    assert {int(r["n_dense"]) for r in recs} >= {120, 121}
    skips = {(int(r["skip"]), (int(r["cut_index"]) - 1) % int(r["skip"])) for r in recs if r["skip"] == r["skip"] and r["skip"] <= 3}
    assert skips >= {(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)}, sorted(skips)
    assert any(r["radius_min"] < 1.0 for r in recs) and any(r["radius_max"] > 3000.0 for r in recs) and any(r["curv_zero"] == r["n_dense"] for r in recs)
    assert {int(r["fit_ier"][0]) for r in recs if r["fit_ier"]} >= {-2, 0, 2, 3}
    first = {int(r["first_front"]) for r in recs if r["first_front"] == r["first_front"]}
    assert first >= {-1, 0, 3, 4, 7, 8, 15, 16, 63, 64}, sorted(first)


def test_fitpack_polylines_against_the_oracle():
    """Family F's polylines through fit_polyline<64> alone (emu_fit) against the oracle's splprep: knots, coefficients, ier and fp, bit
    for bit — every way through parcur_fit that FIT_BRANCHES names and s > 0 can reach."""
    o, e = ps.libs()
    masks = []
    for P, s, mask in ps.fit_polylines():
        rc, u, t, cx, cy, ier, fp = o.splprep(P, s, 3)
        grc, k, n, gt, gcx, gcy, gier, gfp, max_u = e.fit(P, s)
        masks.append(mask)
        if len(t) > e.FIT_TEST_KNOTS:  # (the one polyline of 66 knots: this workspace hands it on; the stage plans it with 256, family F)
            assert grc == 204
            continue
        assert rc == 0 and grc == 0 and k == 3 and n == len(t) and gier == ier, (len(P), s, rc, grc, n, len(t), gier, ier)
        assert np.array_equal(gt, t) and np.array_equal(gcx[: n - 4], cx[: n - 4]) and np.array_equal(gcy[: n - 4], cy[: n - 4])
        assert gfp == fp and max_u == u[-1]
    assert ps.branches_reached(o, masks) == set(o.FIT_BRANCHES) - {"ier1", "interpolant"}
