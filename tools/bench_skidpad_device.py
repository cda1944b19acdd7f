#!/usr/bin/env python3
"""Skidpad device tickets against the live car's route, on BASELINE config 5's shape: 1024 perturbed planners x the 341 recorded
frames (profiles/skidpad_device.md).

  device   SkidpadDeviceFleet.step: every tick's counts / cones / poses uploaded beforehand, paths and status into a ring of
           device arrays, nothing collected beyond what the slots force; the clock stops behind fleet.wait()
  host     the same ticks through SkidpadBatch.submit + collect, one step at a time (= SkidpadBatch.step, fsdp_skidpad_step), with
           page-locked inputs and results: the live car's route, which a device ticket does not change — the yardstick

The two legs alternate, REPS times each, after a warm-up of both; means and the spread (min .. max) are printed as one JSON line.
Both legs must end on the same bytes.   python tools/bench_skidpad_device.py [n_planners] [reps]
FSDP_SKID_DEVICE_LEGS=device: the device leg alone, once (for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/...)."""
import importlib
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import device_io_support as dio  # noqa: E402
import skidpad_support as sk  # noqa: E402

pkg = importlib.import_module("ft-fsd-path-planning_amd")
pkg._capi.DEFAULT_OPTIONS.update(pkg._capi.options_from_env())

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
ONLY_DEVICE = os.environ.get("FSDP_SKID_DEVICE_LEGS") == "device"
DEPTH = 8
g = sk.load_sequence(ROOT / "tests" / "golden")
tf = sk.perturbed_instances(g, n)
T = int(os.environ.get("FSDP_SKID_DEVICE_TICKS", len(g["poses"])))
frames = [sk.batch_for_step(g, t, tf) for t in range(T)]
cap = max(int(np.diff(f[0]).max()) for f in frames)

fleet = pkg.SkidpadDeviceFleet(n, cap, device=0, depth=DEPTH)
ctx = fleet.ctx
ins = []
for off, cones, poses in frames:
    counts, tensor = dio.pad_frames(off, cones, cap, fill=np.nan)
    ins.append((pkg.device_array(ctx, counts, np.int32), pkg.device_array(ctx, tensor, np.float64), pkg.device_array(ctx, poses, np.float64)))
ring = [(pkg.DeviceArray(ctx, (n, ctx.shapes.path_points, 4)), pkg.DeviceArray(ctx, (n,), np.int32)) for _ in range(DEPTH + 1)]

host = pkg.SkidpadBatch(n, device=0)
pinned = [tuple(pkg.pinned_copy(a, dt) for a, dt in zip(f, (np.int32, np.float64, np.float64))) for f in frames]
out = pkg.pinned_empty(n, pkg.RESULT_DTYPE)
info = pkg.pinned_empty(n, pkg.skidpad.INFO_DTYPE)


def device_leg():
    fleet.reset()
    t0 = time.perf_counter()
    for t in range(T):
        paths, status, _ = fleet.step(*ins[t], paths=ring[t % (DEPTH + 1)][0], status=ring[t % (DEPTH + 1)][1])
    fleet.wait()  # (fsdp_collect of the last ticket: an event synchronise behind its out kernel)
    el = time.perf_counter() - t0
    return el, paths.numpy(), status.numpy()


def host_leg():
    host.reset()
    t0 = time.perf_counter()
    for t in range(T):
        res, _ = host.collect(host.submit(*pinned[t], out=out, info=info))
    el = time.perf_counter() - t0
    return el, res["path"].copy(), res["status"].copy()


device_leg()  # warm-up: code objects, the slots' buffers, both routes' first launches
if ONLY_DEVICE:
    el, _, _ = device_leg()
    print(json.dumps({"leg": "device", "planners": n, "ticks": T, "us_per_tick": el / T * 1e6}))
    fleet.close()
    sys.exit(0)
host_leg()
dev, hst = [], []
for _ in range(REPS):
    el, p_d, s_d = device_leg()
    dev.append(el)
    el, p_h, s_h = host_leg()
    hst.append(el)
    assert p_d.tobytes() == p_h.tobytes() and s_d.tobytes() == s_h.tobytes(), "the device route and the host route differ"


def stats(els):
    us = np.array(els) / T * 1e6
    return {"us_per_tick_mean": float(us.mean()), "us_per_tick_min": float(us.min()), "us_per_tick_max": float(us.max()),
            "ticks_per_s_mean": float((T / np.array(els)).mean()), "frames_per_s_mean": float((n * T / np.array(els)).mean())}


print(json.dumps({"config": f"skidpad, {n} perturbed planners x {T} frames, cone_capacity {cap}, {REPS} alternating repetitions",
                  "device_fleet": {**stats(dev), "depth": DEPTH}, "host_one_step_at_a_time_pinned": stats(hst),
                  "device_over_host_ticks_per_s": float(np.mean(hst) / np.mean(dev)),
                  "note": "the clock is the host's, around work that ends in an event synchronise; the last tick's paths and status are byte-equal on both routes"}))
fleet.close()
host.close()
