"""Skidpad stage on constructed inputs, on the CPU (tests/skidpad_constructed_support.py): the kernel sources under the host SIMT
emulator against the oracle in det-math mode, on every route a step can take — one launch per step, groups of steps in one
skid_path_kernel launch with the case's decisive step first, second and last in its group, the packed route at 16 and 8 lanes, and the
wide build with mpc_prediction_horizon = 56.  Status, fallback bits, relocalized, window index (also after a failed step) and the
transform are equal, every path bit for bit; the planners' states after a sequence are the same bytes on every route.  The flip proofs
of the threshold pairs and the structural claims of the support file are assertions here; no pair is skipped."""
import numpy as np
import pytest

import emu_lib
import oracle_lib
import skidpad_constructed_support as S

FRAMES = [f.name for f in S.frames()]
WIDE = dict(mpc_prediction_horizon=56)
EXACT_FRAMES = ("canonical", "mirrored", "yaw pi")  # rigid motions that keep equal distances bit-equal

_oracle = {}


@pytest.fixture(scope="module")
def built():
    return S.build()


@pytest.fixture(scope="module")
def constants():
    table, noise = S.tables()
    ref, md = emu_lib.skidpad_constants(table)
    return table, noise, ref, md


def _cases(built, frame):
    return [c for c in built[0] if c.frame == frame]


def oracle_results(built, frame, wide=False):
    if (frame, wide) not in _oracle:
        if wide:
            import oracle_lib_wide

            with oracle_lib_wide.params(WIDE):
                _oracle[(frame, wide)] = {c.name: S.run_oracle(c, oracle_lib_wide) for c in _cases(built, frame)}
        else:
            _oracle[(frame, wide)] = {c.name: S.run_oracle(c) for c in _cases(built, frame)}
    return _oracle[(frame, wide)]


def test_every_pair_flips_and_none_is_skipped(built):
    """Each threshold pair, in each frame: both sides within REL of the threshold on the oracle's decision record, and the oracle reports
    something else on either side (relocalized or not, another window index, another transform)."""
    cases, pairs = built
    names = sorted({p.name for p in pairs})
    assert names == sorted(["radius-6.625", "radius-8.625", "spacing-0.9", "spacing-3.9", "centres-2-3", "eps-3.0", "pair-17.75", "pair-18.75",
                            "pair-near-tie", "right-centre-on-axis", "left-centre-on-axis", "angle-branch-cut", "equidistant"])
    assert len(pairs) == len(names) * len(FRAMES)  # none skipped
    for p in pairs:
        assert all(abs(v) <= S.REL * p.scale for v in p.values), (p.name, p.frame, p.key, p.values)
        assert S.flips(p.below, p.above), (p.name, p.frame)
    per_family = {f: sum(c.family == f for c in cases) for f in S.FAMILIES}
    print("cases per family:", per_family, "pairs:", len(pairs))
    assert all(per_family.values())


def test_the_scenes_are_what_their_names_say(built):
    """The structural cases on the oracle's decision record: numbers of cones, centres and clusters, the chosen pair, the tie of the
    20th and the 21st cone, the window's clamps."""
    for frame in FRAMES:
        res = oracle_results(built, frame)
        rec = lambda name, s=0: res[f"{name} [{frame}]"][s][4]
        out = lambda name: res[f"{name} [{frame}]"]
        for n in S.CONE_COUNTS:
            assert rec(f"count-{n}")["m"] == min(n, 20)
            assert bool(out(f"count-{n}")[0][1][0]) == (n >= 19), n
        assert rec("centres-64")["n_centers"] == 64 and rec("centres-65")["n_centers"] == 65 and rec("centres-max")["n_centers"] == 236
        # the smallest label crosses more than 64 / 128 centre indices on its way through the chain, everything ends in one cluster
        assert rec("chain-64")["n_centers"] - 2 > 64 and rec("chain-128")["n_centers"] - 2 > 128
        assert rec("chain-64")["cluster_sizes"][1:] == [1] and rec("chain-128")["cluster_sizes"][1:] == [1]
        assert rec("one-cluster")["n_clusters"] == 1 and rec("one-cluster")["success"] == 0
        assert rec("sizes-1-2")["cluster_sizes"] == [2, 1] and rec("sizes-odd")["cluster_sizes"] == [3, 7]
        assert rec("clusters-most")["n_clusters"] == 6
        # an even and an odd cluster whose x and y medians are held by different members
        med = rec("medians-x-y-differ")
        assert med["cluster_sizes"] == [10, 7] and med["median_split"] == [1, 1] and med["success"] == 1
        # a rotation within 1e-9 (relative) of +pi: one at or below it (the double pi itself where the bisection meets it), one above
        ra, rb = sorted(out(f"rotation-pi/{k}")[0][3][2] for k in "ab")
        assert ra <= np.pi < rb and max(abs(ra - np.pi), abs(rb - np.pi)) <= S.REL * np.pi
        assert (rec("three-clusters")["n_clusters"], rec("three-clusters")["pair_a"], rec("three-clusters")["pair_b"]) == (3, 1, 2)
        assert (rec("four-clusters")["n_clusters"], rec("four-clusters")["pair_a"], rec("four-clusters")["pair_b"]) == (4, 1, 2)
        for nm in ("both-left-of-the-car", "both-right-of-the-car"):  # (the mirrored frame swaps the two)
            assert rec(nm)["side0"] * rec(nm)["side1"] > 0 and rec(nm)["success"] == 0 and rec(nm)["best_distance"] < 0.5
        assert rec("both-left-of-the-car")["side0"] * rec("both-right-of-the-car")["side0"] < 0
        if frame == "canonical":  # values ON their thresholds, bit for bit (S.EXACT_SCENES)
            assert rec("radius-exactly-8.625")["radius_margin"] == 0.0 and rec("radius-exactly-8.625")["success"] == 0
            assert rec("eps-exactly-3.0")["eps_margin"] == 0.0 and rec("eps-exactly-3.0")["cluster_sizes"] == [2, 4]
            tie = rec("pair-exact-tie")
            assert tie["runner_up"] == tie["best_distance"] and (tie["n_clusters"], tie["pair_a"], tie["pair_b"], tie["success"]) == (3, 0, 1, 1)  # the first pair
        if frame in EXACT_FRAMES:
            assert rec("tie-20-21")["select_gap"] == 0.0 and rec("tie-20-21-swapped")["select_gap"] == 0.0
            assert out("tie-20-21")[0][3].tobytes() != out("tie-20-21-swapped")[0][3].tobytes()  # the lower index is taken: another cone
        # the latch: the transform is the one of pose A; seen from pose B the sides are the other way round
        assert out("latch")[1][1][0] == 1 and rec("latch", 1)["side0"] * rec("latch", 1)["side1"] < 0
        # a NaN pose at a later attempt: relocalized from the first twenty cones in index order
        later = out("pose-nan-x-later")
        assert [int(r["status"]) for r, *_ in later] == [0, 103, 0, 103] and later[2][1][0] == 1
        assert [int(r["status"]) for r, *_ in out("pose-nan-x-first")] == [103, 0, 0] and not any(x[1][0] for x in out("pose-nan-x-first"))
        # the window: lo clamp, the last reachable index, the drive to the end (fin clamp, n1 down to 1, the index moved by a failed step)
        assert rec("index-0", 1)["lo"] == 0 and rec("index-0", 1)["argmin"] == 0
        assert [rec(f"ahead-{k}", 1)["argmin"] for k in (197, 198, 199, 200)] == [248, 249, 249, 249] and rec("ahead-199", 1)["hi"] == 250
        drive = out("drive-to-the-end")
        assert len(drive) == 16 and drive[-1][2] == 2892 and int(drive[-1][0]["status"]) == 103 and drive[-1][4]["n1"] == 1
        assert drive[-2][4]["n1"] < 249 and int(drive[-2][0]["path_fallback"]) & 32 and drive[-1][4]["hi"] == 2893
        assert rec("crossing", 1)["argmin"] == 200 and rec("jump-beyond-the-window", 3)["argmin"] == 198


ROUTES = ["single", "first", "second", "last", "whole", "packed-16", "packed-8"]
ROUTES += ["wide-" + r for r in ROUTES]  # the same routes with the wide build's shapes


def _run_route(cases, route, constants, emu, want, single_states=None):
    """every bucket of `cases` through one route; returns {bucket: states bytes}"""
    table, noise, ref, md = constants
    states = {}
    for key, bucket in sorted(S.buckets(cases).items()):
        n_steps, decisive = key
        frames, rows = S.layout(bucket)
        n = len(frames[0][2])
        em = emu.SkidpadEmu(n, table, noise, ref, md)
        if route.startswith("packed"):
            got, _ = em.steps_packed(frames, int(route.split("-")[1]))
        else:
            parts = S.partitions(n_steps, decisive)
            if route not in parts:
                continue
            got, t = [], 0
            for k in parts[route]:
                got += em.steps(frames[t : t + k])
                t += k
        for c, row in zip(bucket, rows):
            S.compare(c, want[c.name], [g[0][row] for g in got], [g[1][row] for g in got], em.states[row], route)
        states[key] = em.states.tobytes()
    return states


_single_states = {}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("frame", FRAMES)
def test_emulated_kernels_equal_oracle(built, constants, frame, route):
    """Every case of one frame through one route: equal to the oracle (S.compare), and the planners' states are the bytes the
    one-launch-per-step route leaves."""
    wide = route.startswith("wide")
    cases = _cases(built, frame)
    want = oracle_results(built, frame, wide)
    if wide:
        import emu_lib_wide

        with emu_lib_wide.params(WIDE):
            states = _run_route(cases, route[5:], constants, emu_lib_wide, want)
            ref = _single_states.get((frame, True)) or (states if route == "wide-single" else _run_route(cases, "single", constants, emu_lib_wide, want))
        _single_states[(frame, True)] = ref
    else:
        states = _run_route(cases, route, constants, emu_lib, want)
        ref = _single_states.get((frame, False)) or (states if route == "single" else _run_route(cases, "single", constants, emu_lib, want))
        _single_states[(frame, False)] = ref
    assert states
    for key, b in states.items():
        assert b == ref[key], (frame, route, key)


@pytest.mark.parametrize("frame", FRAMES)
def test_not_finite_cases_as_planner_zero(built, constants, frame):
    """The cases with cones or poses that are not finite once more, each as planner 0 of a batch of its own (no planner in front of it):
    what it reads can then only come from in front of the cone buffer."""
    table, noise, ref, md = constants
    want = oracle_results(built, frame)
    n = 0
    for c in _cases(built, frame):
        if c.neighbour is None:
            continue
        em = emu_lib.SkidpadEmu(1, table, noise, ref, md)
        got = [em.step(np.array([0, len(x)], np.int32), x, p[None]) for x, p in c.steps]
        S.compare(c, want[c.name], [g[0][0] for g in got], [g[1][0] for g in got], em.states[0], "planner 0")
        n += 1
    assert n == 16


def test_a_neighbours_cones_do_not_matter(built, constants):
    """The defect this suite was written for: with fewer than min(n, 20) distances that are not NaN, the selection read the cone in
    front of the planner's own — the last cone of the planner before it.  Two neighbours, one completing the ring: the same result."""
    table, noise, ref, md = constants
    c = [x for x in _cases(built, "canonical") if x.name.startswith("nan-one-of-20 ")][0]
    res = []
    for last in (c.neighbour[-1], np.array([500.0, 500.0, 0.0])):
        nb = c.neighbour.copy()
        nb[-1] = last
        em = emu_lib.SkidpadEmu(2, table, noise, ref, md)
        out, info = em.step(np.array([0, len(nb), len(nb) + len(c.steps[0][0])], np.int32), np.concatenate([nb, c.steps[0][0]]),
                            np.stack([c.steps[0][1]] * 2))
        res.append((out[1].tobytes(), info[1].tobytes(), em.states[1].tobytes()))
    assert res[0] == res[1]


def test_a_noise_table_too_short_for_the_subsets(built, constants):
    """fsdp_skidpad_set_tables with fewer noise rows than subsets (the reference's randn(len(idxs), 3, 2) always has enough): the oracle
    reports FSDO_REF_UNDEFINED_OTHER (109), the kernel ST_REF_UNDEFINED_PATH (103) — both a failed step, no relocalization, the index
    and the previous path untouched; with exactly enough rows (C(10, 3) = 120) both relocalize alike."""
    table, noise, ref, md = constants
    c = [x for x in _cases(built, "canonical") if x.name.startswith("count-20 ")][0]
    ten = S._case(S.frames()[0], "ten", "B", [(np.concatenate([S.right(5), S.left(5)]), S.POSE0)])
    for case, rows, ok in ((c, 1139, False), (c, 1140, True), (ten, 119, False), (ten, 120, True)):
        short = noise[:rows]
        want = S.run_oracle(case, noise=short)
        em = emu_lib.SkidpadEmu(1, table, short, ref, md)
        x, p = case.steps[0]
        out, info = em.step(np.array([0, len(x)], np.int32), x, p[None])
        if ok:
            S.compare(case, want, [out[0]], [info[0]], em.states[0], "noise")
            assert int(out[0]["status"]) == 0
        else:
            assert int(want[0][0]["status"]) == 109 and int(out[0]["status"]) == 103
            assert np.isnan(out[0]["path"]).all() and int(em.states[0]["relocalized"]) == 0 and int(em.states[0]["index_along_path"]) == 0
            assert np.array_equal(em.states[0]["prev"], emu_lib.default_path())
