#!/usr/bin/env python3
"""Decision margins of the path stage: how close does the sampled workload come to each threshold of the stage (too far, connect,
in front, plen, the radius clamps, the trim arg-min, the 20 m cut, the skip and dense-count quotients, the curvature clamps)?  None
of these holds a libm value; a kernel decides differently from the oracle only where its arithmetic differs, and tests/path_support.py
builds inputs 1e-9 either side of each.  This table records how far the committed goldens and fresh synthetic sets stay from them.
CPU only (the oracle, single thread).   python tools/path_margins.py > profiles/path_decision_margins.txt"""
import ctypes, importlib, sys
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import oracle_lib
pkg = importlib.import_module("ft-fsd-path-planning_amd")
NAMES = {"path_too_far": "closest dense sample vs 5 m (relative)", "path_connect_dist": "first path point vs 0.5 m (relative)",
         "path_connect_angle": "its bearing vs 90 deg (relative)", "path_front_dot": "dot(car -> point, direction) vs 0 (absolute, m)",
         "path_plen": "path length in front vs 20 m (relative)", "path_radius": "fitted radius vs 10 / 80 / 100 (relative)",
         "path_trim_argmin": "trim arg-min: second closest / closest - 1", "path_cut": "cumulative length vs 20 m at the cut and before it (relative)",
         "path_skip_frac": "skip quotient to the next integer (absolute)", "path_dense_frac": "dense-count quotient to the next integer (absolute)",
         "path_curv_clamp": "window radius vs 1 and 3000 (relative)", "path_global_30m": "global-path point vs 30 m (relative)",
         "path_global_argmin": "global path arg-min: second closest / closest - 1"}
sets = []
for name in ("scenarios", "cfg2_color", "cfg3_nocolor", "cfg4_200cones", "cfg4_noisy_nocolor", "fuzz", "lattice"):
    g = np.load(ROOT / "tests" / "golden" / f"{name}.npz")
    sets.append((f"golden {name}", g["offsets"], g["cones"], g["poses"]))
k = 0
for per_side in (24, 64):
    for tn, fn in ((0.15, 0.0), (0.3, 0.0), (0.0, 0.1), (0.0, 0.3)):
        k += 1
        sets.append((f"synthetic {per_side}/side", *pkg.synth.make_replay_batch(1024, per_side, tn, seed=7000 + k, color=True, frame_noise=fn, random_pose=fn > 0)))
frames = 0
with oracle_lib.math_mode(1), oracle_lib.margins() as m:
    for name, off, cones, poses in sets:
        oracle_lib.plan_batch(off, cones, poses, n_threads=1)
        frames += len(off) - 1
    out = np.zeros(6 * len(oracle_lib.MARGIN_CLASSES))
    oracle_lib.lib().fsdo_margins_get_n(out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_int(len(oracle_lib.MARGIN_CLASSES)))
print(f"{frames} frames in {len(sets)} sets (7 golden sets + 8 fresh synthetic sets of 1024 frames), fresh planners, no global path")
print(f"{'decision class':66s} {'decisions':>11s} {'exactly 0':>10s} {'min margin > 0':>15s} {'< 1e-6':>8s} {'< 1e-9':>8s} {'< 1e-12':>8s}")
for i, key in enumerate(oracle_lib.MARGIN_CLASSES):
    if key in NAMES:
        mm, cnt, a, b, c, z = out[6 * i: 6 * i + 6]
        print(f"{NAMES[key]:66s} {int(cnt):11d} {int(z):10d} {(mm if cnt > z else float('nan')):15.3e} {int(a):8d} {int(b):8d} {int(c):8d}")
print("'exactly 0' on the curvature clamps' row would be a radius of exactly 1 or 3000; on the quotients' rows an integer quotient (the dense count")
print("of a path whose length is an exact multiple of its sampling step).  No global path is set in these sets: its two rows stay empty.")
