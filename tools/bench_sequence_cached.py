"""fsdp_plan_sequence_cached against the lock-step calls it replaces, one JSON line per workload:

  1 planner x 1000 steps and 4096 planners x 50 steps of tools/bench_sort_cache.py's workload (a seeded mapped track, 96 cones per
  frame, the map jittered by up to 0.02 m per coordinate and step, the cars 0.45 m further each step); wall clock around blocking
  calls, which end with a device synchronise; one warm-up, then --reps repetitions: median (min-max) milliseconds per whole sequence.

  python tools/bench_sequence_cached.py [--reps 5] [--no-lockstep] [--no-sequence] [--package DIR]

--package: the directory that holds the package to measure (default: this tree) — the lock-step loop is timed on the parent
commit's build by pointing it at a checkout of the parent with --no-sequence.
"""
from __future__ import annotations

import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-lockstep", action="store_true")
    ap.add_argument("--no-sequence", action="store_true")
    ap.add_argument("--package", type=Path, default=Path(__file__).resolve().parents[1])
    a = ap.parse_args(argv)
    sys.path.insert(0, str(a.package))
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    pkg = importlib.import_module("ft-fsd-path-planning_amd")
    from bench_sort_cache import mapped_steps

    def stats(ms):
        return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))

    for n, steps in ((1, 1000), (4096, 50)):
        batches = list(mapped_steps(n, steps))
        off = np.arange(n * steps + 1, dtype=np.int32) * (len(batches[0][1]) // n)
        cones = np.concatenate([b[1] for b in batches])
        poses = np.concatenate([b[2] for b in batches])
        line = dict(planners=n, steps=steps, cones_per_frame=int(off[1]), reps=a.reps)
        ctx = pkg._capi.Context(device=0)
        want = None
        if not a.no_lockstep:
            ms = []
            for rep in range(a.reps + 1):
                ctx.sort_cache_reset(n)
                prev, res, hits = None, [], []
                t0 = time.perf_counter()
                for o, c, p in batches:
                    r = ctx.plan_batch(o, c, p, prev_paths=prev, _sequential=True)
                    prev = np.array(r["path"])  # (no frame of this workload raises: every step hands its path on)
                    res.append(r)
                    hits.append(ctx.sort_cache_hits())
                ms.append((time.perf_counter() - t0) * 1e3)
            want, hits = np.concatenate(res), np.concatenate(hits)
            line.update(lockstep=stats(ms[1:]), hit_rate=round(float((hits == 1).sum() / max(1, (hits >= 0).sum())), 4),
                        all_ok=bool((want["status"] == 0).all()))
        if not a.no_sequence:
            ms = []
            for rep in range(a.reps + 1):
                ctx.sort_cache_reset(n)
                t0 = time.perf_counter()
                got = ctx.plan_sequence_cached(off, cones, poses, n)
                ms.append((time.perf_counter() - t0) * 1e3)
            line.update(sequence=stats(ms[1:]), n_replanned=got[2], n_resorted=got[4],
                        hit_rate_sequence=round(float((got[3] == 1).sum() / max(1, (got[3] >= 0).sum())), 4), stages=",".join(ctx.stage_names()))
            if want is not None:
                line.update(bytes_equal_lockstep=all(np.ascontiguousarray(got[0][f]).tobytes() == np.ascontiguousarray(want[f]).tobytes()
                                                     for f in want.dtype.names),
                            speedup_median=round(line["lockstep"]["median_ms"] / line["sequence"]["median_ms"], 2))
        ctx.close()
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
