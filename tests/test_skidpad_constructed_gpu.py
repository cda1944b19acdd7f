"""Skidpad stage on constructed inputs, on the MI355X (tests/skidpad_constructed_support.py; the CPU twin of this file proves the
flips and runs the kernel sources under the emulator): the same cases through SkidpadBatch, all cases of one length in one batch of
planners, against the oracle in det-math mode — integers equal, paths and planner information bit for bit.  Routes: one blocking
step at a time, replays submitted 3 and 16 steps ahead, groups of 3 steps (skid_group), and the packed kernels from the first pair
(skid_pack_min = 1); both builds (the wide one with mpc_prediction_horizon = 56)."""
import importlib

import numpy as np
import pytest

import oracle_lib
import skidpad_constructed_support as S

pytestmark = pytest.mark.gpu

WIDE = dict(mpc_prediction_horizon=56)

# fsdp_skidpad_info.rotation is atan2 of the device's libm here and of the host's in the oracle (std::atan2, as the reference's NumPy):
# on these (case, step) the two differ in the last bit (measured on an MI355X, both builds alike: 4.4e-16 at most, one ulp at |rotation|
# next to pi; the list is also in DESIGN.md 6.2).  They are held to the project's 1e-9 for that one field (tests/test_skidpad_gpu.py); every other step, and every other
# field of these, to the bits.  DESIGN.md 6.2.
ROTATION_LAST_BIT = {
    ("centres-2-3/a [canonical]", 0), ("centres-64 [canonical]", 0), ("centres-64 [yaw pi]", 0), ("centres-max [mirrored]", 0),
    ("chain-64 [canonical]", 0), ("chain-64 [mirrored]", 0), ("clusters-most [mirrored]", 0), ("clusters-most [yaw pi]", 0),
    ("coincident-three [seeded]", 0), ("coincident-three [yaw pi]", 0), ("eps-exactly-3.0 [mirrored]", 0), ("eps-exactly-3.0 [seeded]", 0),
    ("eps-exactly-3.0 [yaw pi]", 0), ("four-clusters [canonical]", 0), ("four-clusters [seeded]", 0), ("inf-and-nan-of-25 [yaw pi]", 0),
    ("inf-one-of-20 [canonical]", 0), ("left-centre-on-axis/a [seeded]", 0), ("medians-x-y-differ [mirrored]", 0),
    ("medians-x-y-differ [seeded]", 0), ("nan-one-of-19 [mirrored]", 0), ("nan-one-of-20 [canonical]", 0),
    ("nan-several-of-20 [canonical]", 0), ("nan-several-of-20 [seeded]", 0), ("nan-several-of-20 [yaw pi]", 0),
    ("nan-several-of-25 [canonical]", 0), ("nan-several-of-25 [yaw pi]", 0), ("pair-17.75/b [mirrored]", 0), ("pair-exact-tie [seeded]", 0),
    ("pair-near-tie/b [canonical]", 0), ("pair-near-tie/b [yaw pi]", 0), ("pose-nan-x-later [yaw pi]", 2),
    ("radius-6.625/b [canonical]", 0), ("radius-6.625/b [mirrored]", 0), ("radius-6.625/b [yaw pi]", 0),
    ("right-centre-on-axis/b [canonical]", 0), ("sizes-1-2 [seeded]", 0), ("sizes-1-2 [yaw pi]", 0), ("sizes-odd [mirrored]", 0),
    ("sizes-odd [seeded]", 0), ("sizes-odd [yaw pi]", 0), ("spacing-3.9/a [yaw pi]", 0), ("three-clusters [mirrored]", 0),
    ("three-clusters [seeded]", 0), ("three-clusters [yaw pi]", 0), ("tie-20-21 [canonical]", 0), ("tie-20-21 [seeded]", 0),
    ("tie-20-21-swapped [seeded]", 0), ("ties-64-apart [mirrored]", 0), ("ties-interleaved [mirrored]", 0),
    ("ties-reversed [canonical]", 0), ("ties-reversed [yaw pi]", 0), ("ties-shuffled [canonical]", 0),
}


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("ft-fsd-path-planning_amd")


@pytest.fixture(scope="module")
def built():
    return S.build()


_want = {}


def oracle_results(built, wide):
    """computed once per build, shared by the routes, never written to"""
    if wide not in _want:
        if wide:
            import oracle_lib_wide

            with oracle_lib_wide.params(WIDE):
                _want[wide] = {c.name: S.run_oracle(c, oracle_lib_wide) for c in built[0]}
        else:
            _want[wide] = {c.name: S.run_oracle(c) for c in built[0]}
    return _want[wide]


ROUTES = {
    # name: (replay depth or None for blocking steps, skid_group, skid_pack_min)
    "steps": (None, None, None),
    "replay-3": (3, None, None),
    "replay-16": (16, None, None),
    "group-3": (16, 3, 1000000),
    "packed": (16, None, 1),
}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("build", ["standard", "wide"])
def test_constructed_cases_equal_oracle(pkg, built, monkeypatch, build, route):
    depth, group, pack_min = ROUTES[route]
    if group:
        monkeypatch.setitem(pkg._capi.DEFAULT_OPTIONS, "skid_group", group)
    if pack_min:
        monkeypatch.setitem(pkg._capi.DEFAULT_OPTIONS, "skid_pack_min", pack_min)
    wide = build == "wide"
    want = oracle_results(built, wide)
    n_cases = 0
    for key, bucket in sorted(S.buckets(built[0]).items()):
        frames, rows = S.layout(bucket)
        n = len(frames[0][2])
        # Batches stay within a few hundred planners.  Steps: 8 at the most for every case but one — `drive-to-the-end` cannot reach
        # the table's last index in fewer than 16 (the window lets the index advance by 198 per step over 2893 points), so its batch
        # of four planners has 16 steps on purpose; it also goes through replay depth 16 and skid_group 3 like the others.
        assert n <= 400 and (key[0] <= 8 or (key[0] == 16 and n == 4 and all(c.name.startswith("drive-to-the-end") for c in bucket)))
        batch = pkg.SkidpadBatch(n, device=0, params=WIDE if wide else None)
        assert (batch._ctx.shapes is pkg.WIDE) == wide
        if depth is None:
            got = [tuple(a.copy() for a in batch.step(*f)) for f in frames]
        else:
            got = [(r.copy(), i.copy()) for r, i in batch.replay(frames, depth)]
        for c, row in zip(bucket, rows):
            loose = {s for n, s in ROTATION_LAST_BIT if n == c.name}
            S.compare(c, want[c.name], [g[0][row] for g in got], [g[1][row] for g in got], None, f"{build} {route}", (loose, 1e-9) if loose else None)
            n_cases += 1
        batch.close()
    assert n_cases == len(built[0])


def test_any_number_of_cones_per_planner(pkg):
    """The selection keeps nothing per cone (csrc/skidpad_kernel.h): a planner with more cones than its workspace has doubles leaves
    the planner behind it alone.  Planner 0: 12000 cones; planner 1: the base scene, with and without planner 0's crowd in front."""
    fr = S.frames()[0]
    big = S._case(fr, "big", "A", [(np.concatenate([S.base20(), S.filler(11980)]), S.POSE0)])
    base = S._case(fr, "base", "A", [(S.base20(), S.POSE0)])
    res = []
    for first in (big, base):
        batch = pkg.SkidpadBatch(2, device=0)
        x0, x1 = first.steps[0][0], base.steps[0][0]
        out, info = batch.step(np.array([0, len(x0), len(x0) + len(x1)], np.int32), np.concatenate([x0, x1]), np.stack([S.POSE0, S.POSE0]))
        res.append((out[1]["path"].copy(), info[1].copy()))
        S.compare(base, S.run_oracle(base), [out[1]], [info[1]], None, "behind 12000 cones")
        batch.close()
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1].tobytes() == res[1][1].tobytes()
