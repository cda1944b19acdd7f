"""What the experimental sorting cache saves (include/fsdp.h fsdp_sort_cache_reset), one JSON line:

  lockstep : 4096 planners advanced in lock-step for 50 steps on a seeded mapped track (the SLAM map as input, jittered by up
             to 0.02 m per coordinate and step, the cars 0.45 m further each step) through plan_batch_sequential, cache on and
             off: frames/s (wall clock around each blocking call, which ends with a device synchronise) and the cache's hit rate;
  single   : single-frame p50 of a flagged PathPlanner against an unflagged one on the same sequence.

  python tools/bench_sort_cache.py [--planners 4096] [--steps 50] [--single 200]
"""
from __future__ import annotations

import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
pkg = importlib.import_module("ft-fsd-path-planning_amd")


def mapped_steps(n_planners: int, steps: int, seed: int = 3):
    rng = np.random.default_rng(seed)
    left, right, centre = pkg.synth.closed_track(48, seed)
    base = np.concatenate([np.column_stack([right, np.ones(len(right))]), np.column_stack([left, np.full(len(left), 2.0)])])
    s0 = np.arange(n_planners) / n_planners
    off = np.arange(n_planners + 1, dtype=np.int32) * len(base)
    for k in range(steps):
        cones = np.repeat(base[None], n_planners, axis=0)
        cones[:, :, :2] += rng.uniform(-0.02, 0.02, size=(n_planners, len(base), 2))
        pos, tan = centre(s0 + k * 0.45 / (48 * 4.5))
        yield off, cones.reshape(-1, 3), np.column_stack([pos, tan])


def lockstep(n_planners: int, steps: int, cache: bool):
    ctx = pkg._capi.Context(device=0)
    if cache:
        ctx.sort_cache_reset(n_planners)
    batches = list(mapped_steps(n_planners, steps))
    prev, secs, hits, checks = None, 0.0, 0, 0
    for off, cones, poses in batches:
        t0 = time.perf_counter()
        r = ctx.plan_batch(off, cones, poses, prev_paths=prev, _sequential=True)
        secs += time.perf_counter() - t0
        if cache:
            h = ctx.sort_cache_hits()
            hits, checks = hits + int((h == 1).sum()), checks + int((h >= 0).sum())
        prev = np.array(r["path"])
    ctx.close()
    return n_planners * steps / secs, (hits / checks if checks else 0.0)


def single(n: int, cache: bool):
    planner = pkg.PathPlanner(pkg.MissionTypes.trackdrive, experimental_performance_improvements=cache, device=0)
    times = []
    for off, cones, poses in mapped_steps(1, n):
        t0 = time.perf_counter()
        planner.calculate_path_in_global_frame(cones, poses[0, :2], poses[0, 2:])
        times.append(time.perf_counter() - t0)
    return float(np.median(times[5:]) * 1e6)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--planners", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--single", type=int, default=200)
    a = ap.parse_args(argv)
    lockstep(a.planners, 3, True)  # warm-up (module load, first launches)
    off_fps, _ = lockstep(a.planners, a.steps, False)
    on_fps, rate = lockstep(a.planners, a.steps, True)
    off_fps2, _ = lockstep(a.planners, a.steps, False)
    on_fps2, _ = lockstep(a.planners, a.steps, True)
    p50_off, p50_on = single(a.single, False), single(a.single, True)
    print(json.dumps(dict(planners=a.planners, steps=a.steps, hit_rate=round(rate, 4),
                          frames_per_s_cache_off=[round(off_fps), round(off_fps2)], frames_per_s_cache_on=[round(on_fps), round(on_fps2)],
                          speedup=round((on_fps + on_fps2) / (off_fps + off_fps2), 4),
                          single_frame_p50_us_cache_off=round(p50_off, 1), single_frame_p50_us_cache_on=round(p50_on, 1))))


if __name__ == "__main__":
    main()
