"""The host library's buffers across calls whose sizes go up, down and up again on ONE long-lived context (csrc/host_buffers.h:
every block is owned by a DeviceBuf / PinnedBuf that is replaced when a call needs more than it holds): every result equals, byte
for byte and field by field, the same call on a fresh context.  Small frames (synth, 16 cones) — what is tested is which buffer a
call finds, not the planning.  Allocation FAILURE is not provoked here: tests/test_host_buffers_cpu.py covers it on the CPU."""
import importlib

import numpy as np
import pytest

from test_sequence_tickets_gpu import same

pytestmark = pytest.mark.gpu

SIZES = (3, 40, 5, 70)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("ft-fsd-path-planning_amd")


@pytest.fixture(scope="module")
def frames(pkg):
    """n -> (offsets, cones, poses) of n frames with 16 cones each (computed once per size)"""
    made = {}

    def get(n):
        if n not in made:
            made[n] = pkg.synth.make_replay_batch(n, 8, 0.15, seed=100 + n, color=True)
        return made[n]

    return get


def fresh(pkg, call, **kw):
    """call(context) on a context of its own"""
    c = pkg.Context(device=0, **kw)
    try:
        return call(c)
    finally:
        c.close()


def all_same(got, want):
    got, want = (got if isinstance(got, tuple) else (got,)), (want if isinstance(want, tuple) else (want,))
    return len(got) == len(want) and all(g == w if isinstance(g, int) else same(np.asarray(g), np.asarray(w)) for g, w in zip(got, want))


@pytest.mark.parametrize("params", [None, dict(use_unknown_cones=False)], ids=["default", "no-unknown"])
def test_blocking_calls_up_down_up(pkg, frames, params):
    ctx = pkg.Context(device=0, params=params)
    for n in SIZES:
        call = lambda c: c.plan_batch(*frames(n))
        assert all_same(call(ctx), fresh(pkg, call, params=params)), n
    ctx.close()


def stage_inputs(full, off, cones, max_len):
    """the sorted sides of every frame as match_batch takes them"""
    sl, sr = np.zeros((len(full), max_len, 2)), np.zeros((len(full), max_len, 2))
    for k in range(len(full)):
        xyt = cones[off[k] : off[k + 1]]
        sl[k, : full["n_left"][k]] = xyt[full["left_idx"][k][: full["n_left"][k]], :2]
        sr[k, : full["n_right"][k]] = xyt[full["right_idx"][k][: full["n_right"][k]], :2]
    return sl, sr


def test_stage_level_calls_up_down_up(pkg, frames):
    ctx = pkg.Context(device=0)
    for n in SIZES:
        off, cones, poses = frames(n)
        full = fresh(pkg, lambda c: c.plan_batch(off, cones, poses))
        sl, sr = stage_inputs(full, off, cones, ctx.shapes.max_len)
        calls = {
            "sort": lambda c: c.sort_batch(off, cones, poses),
            "match": lambda c: c.match_batch(sl, full["n_left"], sr, full["n_right"], poses),
            "path": lambda c: c.path_batch(poses, full.copy()),
            "path+prev": lambda c: c.path_batch(poses, full.copy(), prev_paths=np.tile(c.default_path(), (n, 1, 1))),
        }
        for name, call in calls.items():
            assert all_same(call(ctx), fresh(pkg, call)), (name, n)
    ctx.close()


def test_tickets_with_pageable_arrays(pkg, frames):
    ctx = pkg.Context(device=0)
    for n in (4, 33):
        off, cones, poses = frames(n)
        call = lambda c: c.collect(c.submit(off, cones, poses, out=np.zeros(n, dtype=c.result_dtype))).copy()
        assert all_same(call(ctx), fresh(pkg, call)), n
    ctx.close()


def test_sequences_up(pkg, frames):
    ctx = pkg.Context(device=0)
    for planners, steps in ((2, 3), (5, 4)):
        call = lambda c: c.plan_sequence(*frames(planners * steps), n_planners=planners)
        assert all_same(call(ctx), fresh(pkg, call)), (planners, steps)
    ctx.close()


def test_sorting_cache_reset_up_and_off(pkg, frames):
    def lockstep(c, n):
        """reset for n planners (0: off), then two lock-step calls: the second finds the entries of the first"""
        c.sort_cache_reset(n)
        m = n if n else 3
        prev = None if n else np.tile(c.default_path(), (m, 1, 1))
        out = []
        for _ in range(2):
            out.append(c.plan_batch_sequential(*frames(m), prev))
            if n:
                out.append(c.sort_cache_hits())
        return tuple(out)

    ctx = pkg.Context(device=0)
    for n in (2, 5, 0):
        assert all_same(lockstep(ctx, n), fresh(pkg, lambda c: lockstep(c, n))), n
    ctx.close()


def test_skidpad_reset_up_and_down(pkg, frames):
    def two_steps(batch, n):
        batch.n = n
        batch.reset()
        out = []
        for seed in (0, 1):
            off, cones, poses = frames(n)
            res, info = batch.step(off, cones, poses + np.array([0.25 * seed, 0.0, 0.0, 0.0]))
            out += [res, info]
        return tuple(out)

    batch = pkg.SkidpadBatch(2, device=0)
    for n in (2, 5, 3):
        one = pkg.SkidpadBatch(n, device=0)
        assert all_same(two_steps(batch, n), two_steps(one, n)), n
        one.close()
    batch.close()
