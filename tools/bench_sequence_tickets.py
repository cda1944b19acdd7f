"""What sequence calls as tickets and as planner slices buy (include/fsdp.h fsdp_submit_sequence), one JSON line per row; the
inputs are tools/bench_sequence.py's (96 cones a frame, 2 % drop-out frames), every buffer page-locked:

  a  K recordings of 64 planners x 100 steps, and of 1 planner x 1000 steps: K blocking fsdp_plan_sequence calls against the same K
     as tickets, `depth` of them in flight (2, 4, 8; the context's overlap depth = depth),
  b  one 4096 x 50 recording: one blocking call against four planner slices on four contexts of the one GPU (MultiPlanner),
  c  a single blocking Context.plan_sequence per shape — the one part that also runs on the parent commit's package
     (--package-root): run it alternately on both trees in one session and compare the medians with the spread of the parent's
     own repeats.

  python tools/bench_sequence_tickets.py --part a|b|c [--reps 7] [--recordings 16] [--package-root DIR]

Every timed window ends in a collect or a blocking call (both wait for the device); results and final_prev of the ticket forms are compared with
the blocking call's byte for byte, field by field, and a mismatch ends the run with an error."""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from bench_sequence import inputs  # noqa: E402


def spread(secs):
    s = np.sort(np.asarray(secs))
    return {"median_s": float(np.median(s)), "min_s": float(s[0]), "max_s": float(s[-1]), "all_s": [float(x) for x in secs]}


def same(a, b):
    """byte for byte, field by field: the bytes between the fields of a record are nobody's (a copy of a record array does not carry them)"""
    if a.dtype.names:
        return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in a.dtype.names)
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def must_equal(what, got, want):
    """results and final_prev of a ticket form against the blocking call's; a mismatch ends the measurement"""
    bad = [name for name, g, w in (("results", got[0], want[0]), ("final_prev", got[1], want[1])) if not same(g, w)]
    if bad:
        raise SystemExit(f"{what}: {', '.join(bad)} differ from the blocking call's")
    return True


def pinned_recording(pkg, ctx, n, steps, seed):
    off, cones, poses, _ = inputs(pkg, n, steps, 0.02, seed)
    return (pkg.pinned_copy(off, np.int32), pkg.pinned_copy(cones), pkg.pinned_copy(poses), pkg.pinned_empty(n * steps, ctx.result_dtype),
            pkg.pinned_empty((n, ctx.shapes.path_points, 4)))


def blocking(ctx, n, rec):
    off, cones, poses, out, final = rec
    again = ctypes.c_longlong(0)
    ctx._check(ctx._lib.fsdp_plan_sequence(ctx._h, n, len(poses) // n, off.ctypes.data, cones.ctypes.data, poses.ctypes.data, None, out.ctypes.data,
                                           final.ctypes.data, ctypes.byref(again)), "fsdp_plan_sequence")
    return int(again.value)


def part_a(pkg, reps, k):
    for n, steps in ((64, 100), (1, 1000)):
        ctx = pkg._capi.Context(device=0)
        recs = [pinned_recording(pkg, ctx, n, steps, 3 + i) for i in range(k)]
        want = []
        for rec in recs:  # warm-up of the shape, and the expected bytes
            blocking(ctx, n, rec)
            want.append((rec[3].copy(), rec[4].copy()))
        secs = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for rec in recs:
                blocking(ctx, n, rec)
            secs.append(time.perf_counter() - t0)
        base = float(np.median(secs))
        print(json.dumps({"part": "a", "planners": n, "steps": steps, "recordings": k, "form": "blocking", "frames_per_s": k * n * steps / base,
                          **spread(secs)}), flush=True)
        for depth in (2, 4, 8):
            ctx.set_overlap(depth)

            def run():
                inflight = []
                for rec in recs:
                    if len(inflight) == depth:
                        ctx.collect(inflight.pop(0))
                    inflight.append(ctx.submit_sequence(rec[0], rec[1], rec[2], n, out=rec[3], final_prev_out=rec[4]))
                for t in inflight:
                    ctx.collect(t)

            run()  # warm-up: every slot's streams and buffers
            secs = []
            for _ in range(reps):
                t0 = time.perf_counter()
                run()
                secs.append(time.perf_counter() - t0)
            equal = all(must_equal(f"{n} x {steps}, depth {depth}, recording {i}", (r[3], r[4]), w) for i, (r, w) in enumerate(zip(recs, want)))
            med = float(np.median(secs))
            print(json.dumps({"part": "a", "planners": n, "steps": steps, "recordings": k, "form": "tickets", "depth": depth, "equal_bytes": equal,
                              "frames_per_s": k * n * steps / med, "speedup_over_blocking": base / med, **spread(secs)}), flush=True)
        ctx.close()


def part_b(pkg, reps):
    n, steps = 4096, 50
    ctx = pkg._capi.Context(device=0)
    rec = pinned_recording(pkg, ctx, n, steps, 3)
    blocking(ctx, n, rec)
    want = (rec[3].copy(), rec[4].copy())
    secs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        blocking(ctx, n, rec)
        secs.append(time.perf_counter() - t0)
    base = float(np.median(secs))
    print(json.dumps({"part": "b", "planners": n, "steps": steps, "form": "one blocking call", "frames_per_s": n * steps / base, **spread(secs)}), flush=True)
    ctx.close()
    mp = pkg.MultiPlanner(devices=[0, 0, 0, 0])
    res, final, _ = mp.plan_sequence(rec[0], rec[1], rec[2], n)  # warm-up
    equal = must_equal("four planner slices", (res, final), want)
    del res, final
    secs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = mp.plan_sequence(rec[0], rec[1], rec[2], n)
        secs.append(time.perf_counter() - t0)
        must_equal("four planner slices (timed run)", got[:2], want)
        del got
    med = float(np.median(secs))
    print(json.dumps({"part": "b", "planners": n, "steps": steps, "form": "four planner slices on four contexts", "equal_bytes": bool(equal),
                      "zero_copy": mp.zero_copy_batches, "frames_per_s": n * steps / med, "speedup_over_one_call": base / med, **spread(secs)}), flush=True)
    mp.close()


def part_c(pkg, reps, root):
    for n, steps in ((64, 100), (1, 1000), (4096, 20)):
        ctx = pkg._capi.Context(device=0)
        off, cones, poses, _ = inputs(pkg, n, steps, 0.02)
        ctx.plan_sequence(off, cones, poses, n)
        ctx.plan_sequence(off, cones, poses, n)
        secs = []
        for _ in range(reps):
            t0 = time.perf_counter()
            res, _, again = ctx.plan_sequence(off, cones, poses, n)
            secs.append(time.perf_counter() - t0)
        import hashlib

        print(json.dumps({"part": "c", "package_root": str(root), "planners": n, "steps": steps, "n_replanned": again,
                          "results_sha1": hashlib.sha1(b"".join(np.ascontiguousarray(res[k]).tobytes() for k in res.dtype.names)).hexdigest()[:12], "frames_per_s": n * steps / float(np.median(secs)), **spread(secs)}),
              flush=True)
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=("a", "b", "c"), required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--recordings", type=int, default=16)
    ap.add_argument("--package-root", type=Path, default=Path(__file__).resolve().parents[1])
    a = ap.parse_args()
    sys.path.insert(0, str(a.package_root))
    pkg = importlib.import_module("ft-fsd-path-planning_amd")
    if a.part == "a":
        part_a(pkg, a.reps, a.recordings)
    elif a.part == "b":
        part_b(pkg, a.reps)
    else:
        part_c(pkg, a.reps, a.package_root)


if __name__ == "__main__":
    main()
