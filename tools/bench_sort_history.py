#!/usr/bin/env python3
"""What the search history costs (include/fsdp.h fsdp_sort_batch_history) next to fsdp_sort_batch, by kernel trace:
4096 frames x 128 cones (synth.make_replay_batch), rows_cap 32 / 256 with and without the verdicts.  A diagnostic route:
there is no gate on these numbers.

  python tools/bench_sort_history.py [--frames 4096] [--rounds 7] [--out DIR]     (on the GPU box)

The parent runs itself once more under `rocprofv3 --kernel-trace` (child: the calls of every round in a fixed order, the
variants interleaved), reads the dispatches of the sorting kernels back from the trace database in start order — the n-th
dispatch of sort_kernel_128[_history] belongs to the n-th call — and prints one JSON line: per variant the median and the
minimum kernel duration over the rounds, in microseconds, and the ratio of the medians to fsdp_sort_batch's kernel.
"""
from __future__ import annotations

import argparse
import glob
import importlib
import json
import os
import sqlite3
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
VARIANTS = [("sort_batch", None, None)] + [(f"history_cap{k}_{'verdicts' if v else 'noverdicts'}", k, v) for k in (32, 256) for v in (True, False)]


def child(frames: int, rounds: int):
    sys.path.insert(0, str(ROOT))
    pkg = importlib.import_module("ft-fsd-path-planning_amd")
    off, cones, poses = pkg.synth.make_replay_batch(frames, 64, 0.15, seed=1, color=True)
    ctx = pkg._capi.Context(device=0)
    for _ in range(rounds + 1):  # (round 0: warm-up, dropped by the parent)
        for _name, k, v in VARIANTS:
            if k is None:
                ctx.sort_batch(off, cones, poses)
            else:
                ctx.sort_batch_history(off, cones, poses, rows_cap=k, verdicts=v)
    ctx.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", type=Path, default=None, help="where the trace goes (default: a temporary directory)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.child:
        child(a.frames, a.rounds)
        return
    tmp = None
    if a.out is None:
        tmp = tempfile.TemporaryDirectory()
        a.out = Path(tmp.name)
    a.out.mkdir(parents=True, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "-d", str(a.out), "-o", "history", "--", sys.executable, str(Path(__file__).resolve()), "--child",
           "--frames", str(a.frames), "--rounds", str(a.rounds)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, env=dict(os.environ))
    con = sqlite3.connect(glob.glob(f"{a.out}/**/*.db", recursive=True)[0])
    rows = [(str(n), int(s), int(e)) for n, s, e in con.execute("select name, start, end from kernels order by start")]
    main_k = [(n, e - s) for n, s, e in rows if "sort_kernel" in n and "sort_big" not in n]
    big_k = [(n, e - s) for n, s, e in rows if "sort_big_kernel" in n]
    per = len(VARIANTS)
    assert len(main_k) == per * (a.rounds + 1) == len(big_k), (len(main_k), len(big_k))
    out = {"frames": a.frames, "cones_per_frame": 128, "rounds": a.rounds, "unit": "us of kernel time per call (rocprofv3 --kernel-trace)", "variants": {}}
    base = None
    for v, (name, k, _v) in enumerate(VARIANTS):
        d = np.array([main_k[r * per + v][1] for r in range(1, a.rounds + 1)]) * 1e-3
        b = np.array([big_k[r * per + v][1] for r in range(1, a.rounds + 1)]) * 1e-3
        kernel = main_k[per + v][0].split("(")[0].split("::")[-1]
        assert ("history" in kernel) == (k is not None), kernel
        med = float(np.median(d))
        base = med if base is None else base
        out["variants"][name] = {"kernel": kernel, "median_us": round(med, 1), "min_us": round(float(d.min()), 1), "vs_sort_batch": round(med / base, 3),
                                 "empty_big_route_kernel_median_us": round(float(np.median(b)), 1)}
    print(json.dumps(out))
    if tmp:
        tmp.cleanup()


if __name__ == "__main__":
    main()
