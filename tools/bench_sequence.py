"""What planning whole stateful sequences in one call saves (include/fsdp.h fsdp_plan_sequence), one JSON line per shape:

  1 x 4096    one planner, a 4096-step log,
  64 x 256    a small fleet,
  4096 x 20   the sort-cache bench's shape (tools/bench_sort_cache.py), at drop-out rates 0, 2 and 10 %,

every frame 96 cones of a seeded mapped track (jittered per step, the cars 0.45 m further each step); a drop-out frame shows the
planner two cones, so it reads previous_paths[-1].  Per shape, `--reps` repetitions each (all of them are printed):

  sequence  : Context.plan_sequence, one call (skipped where the package has none: the parent commit),
  lockstep  : the same inputs through T plan_batch_sequential calls, the host carrying the planners' previous paths,
  replay    : n = 1 only: replay.replay_stateful_batched (wall clock around the call, as a user of it waits).

  python tools/bench_sequence.py [--reps 5] [--shapes 1x4096,64x256,4096x20] [--package-root DIR]

--package-root: import the package from another checkout (the parent commit's, built) — its lock-step and replay numbers are
the baselines of profiles/sequence.md.  The results of the sequence call are compared with the lock-step calls' byte for byte."""
from __future__ import annotations

import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np


def inputs(pkg, n: int, steps: int, drop_rate: float, seed: int = 3):
    rng = np.random.default_rng(seed)
    left, right, centre = pkg.synth.closed_track(48, seed)
    base = np.concatenate([np.column_stack([right, np.ones(len(right))]), np.column_stack([left, np.full(len(left), 2.0)])])
    far = np.concatenate([base[:1], base[len(right):len(right) + 1]])
    s0 = np.arange(n) / n if n > 1 else np.array([0.1])
    drop = rng.random((steps, n)) < drop_rate
    cones, counts, poses = [], np.where(drop, len(far), len(base)).ravel(), []
    for k in range(steps):
        c = np.repeat(base[None], n, axis=0)
        c[:, :, :2] += rng.uniform(-0.02, 0.02, size=(n, len(base), 2))
        pos, tan = centre(s0 + k * 0.45 / (48 * 4.5))
        poses.append(np.column_stack([pos, tan]))
        if drop[k].any():
            cones.extend(far if drop[k, i] else c[i] for i in range(n))
        else:
            cones.append(c.reshape(-1, 3))
    off = np.zeros(n * steps + 1, np.int32)
    np.cumsum(counts, out=off[1:])
    return off, np.concatenate(cones), np.concatenate(poses), int(drop.sum())


def lockstep(ctx, off, cones, poses, n):
    steps = (len(off) - 1) // n
    default = ctx.default_path()
    have = np.full((n,) + default.shape, np.nan)
    out = np.zeros(n * steps, ctx.result_dtype)
    t0 = time.perf_counter()
    for t in range(steps):
        lo, hi = t * n, (t + 1) * n
        real = ~np.isnan(have[:, 0, 0])
        prev = np.where(real[:, None, None], have, default[None])
        r = ctx.plan_batch_sequential(off[lo:hi + 1] - off[lo], cones[off[lo]:off[hi]], poses[lo:hi], prev)
        ok = r["status"] == 0
        have[ok] = r["path"][ok]
        out[lo:hi] = r
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="1x4096,64x256,4096x20")
    ap.add_argument("--package-root", type=Path, default=Path(__file__).resolve().parents[1])
    ap.add_argument("--no-lockstep", action="store_true", help="the sequence call alone (for a kernel trace)")
    a = ap.parse_args()
    sys.path.insert(0, str(a.package_root))
    pkg = importlib.import_module("ft-fsd-path-planning_amd")
    for shape in a.shapes.split(","):
        n, steps = (int(x) for x in shape.split("x"))
        for rate in ((0.0, 0.02, 0.10) if n == 4096 else (0.02,)):
            off, cones, poses, dropped = inputs(pkg, n, steps, rate)
            ctx = pkg._capi.Context(device=0)
            row = {"planners": n, "steps": steps, "drop_rate": rate, "drop_out_frames": dropped, "package_root": str(a.package_root)}
            ref = None
            if not a.no_lockstep:
                lockstep(ctx, off, cones, poses, n)  # warm-up
                secs = []
                for _ in range(a.reps):
                    sec, ref = lockstep(ctx, off, cones, poses, n)
                    secs.append(sec)
                row.update(lockstep_s=secs, lockstep_frames_per_s=n * steps / float(np.median(secs)))
            if hasattr(ctx, "plan_sequence"):
                res, _, again = ctx.plan_sequence(off, cones, poses, n)  # warm-up
                secs = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    res, _, again = ctx.plan_sequence(off, cones, poses, n)
                    secs.append(time.perf_counter() - t0)
                row.update(sequence_s=secs, sequence_frames_per_s=n * steps / float(np.median(secs)), n_replanned=again)
                if ref is not None:
                    row.update(equal_bytes=bool(res.tobytes() == ref.tobytes()))
            ctx.close()
            if n == 1 and not a.no_lockstep:
                obs = [[cones[off[f]:off[f + 1]][cones[off[f]:off[f + 1], 2] == t, :2] for t in range(5)] for f in range(steps)]
                secs = []
                for _ in range(a.reps + 1):  # (the first one warms up)
                    t0 = time.perf_counter()
                    _, _, again = pkg.replay.replay_stateful_batched(pkg.MissionTypes.trackdrive, poses[:, :2], poses[:, 2:], obs, device=0)
                    secs.append(time.perf_counter() - t0)
                row.update(replay_s=secs[1:], replay_frames_per_s=steps / float(np.median(secs[1:])), replay_planned_again=again)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
