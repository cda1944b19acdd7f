"""TEST INFRASTRUCTURE: the polyline the refit (fit #2) is handed, from the kernel sources on the host SIMT emulator
(tests/emu/refit_probe.cpp: path_prep_kernel, then the frame's parameter values out of its arena), and what the refit's
residual / f(p) passes make of it: which knot intervals the points of a half super-chunk fall into."""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

import emu_lib
import oracle_lib

EMU_DIR = Path(__file__).resolve().parent / "emu"
LIB = EMU_DIR / "librefit_probe.so"
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = EMU_DIR / "refit_probe.cpp"
        deps = [src, EMU_DIR / "hip_emu.h", *sorted((EMU_DIR.parent.parent / "ft-fsd-path-planning_amd" / "csrc").glob("*.h"))]
        if not LIB.exists() or any(LIB.stat().st_mtime < d.stat().st_mtime for d in deps):
            subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-fvisibility=hidden", "-fno-gnu-unique",
                            "-shared", str(src),
                            "-o", str(LIB)], check=True, cwd=str(EMU_DIR))
        _lib = ctypes.CDLL(str(LIB))
    return _lib


def polylines(offsets, cones, poses, prm=None, global_path=None, prev_paths=None):
    """[(status, m, U[0..m))] per frame: what path_prep_kernel hands the refit under the parameters prm (a dict of overrides);
    global_path: (n, 2) as Context.set_global_path takes it, or None; prev_paths: (frames, PATH_POINTS, 4) or None."""
    cap = lib().probe_path_cap()
    with emu_lib.params(prm or {}):
        s = emu_lib.sort(offsets, cones, poses)
        m = emu_lib.match(offsets, cones, poses, s)
        dp = emu_lib.default_path()
    n = len(offsets) - 1
    poses = np.ascontiguousarray(poses, np.float64)
    mid = np.zeros((n, 4), np.int32)
    u = np.zeros((n, cap))
    v = oracle_lib.param_vector(prm)
    d = ctypes.POINTER(ctypes.c_double)
    pv = None if prev_paths is None else np.ascontiguousarray(prev_paths, np.float64)
    assert pv is None or pv.shape == (n, emu_lib.PATH_POINTS, 4)
    gp = None if global_path is None else np.ascontiguousarray(global_path, np.float64).reshape(-1, 2)
    lib().probe_refit_polyline(ctypes.c_int(n), poses.ctypes.data_as(d), ctypes.c_void_p(m.ctypes.data), dp.ctypes.data_as(d),
                               v.ctypes.data_as(d), mid.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), u.ctypes.data_as(d),
                               None if gp is None else gp.ctypes.data_as(d), ctypes.c_int(0 if gp is None else len(gp)),
                               None if pv is None else pv.ctypes.data_as(d))
    return [(int(mid[f, 0]), int(mid[f, 3]), u[f, : mid[f, 3]].copy()) for f in range(n)]


def chunk_boundaries(u, knots, group=4, rounds=4):
    """Per half super-chunk of the residual / f(p) passes at `group` lanes per frame (rounds x group consecutive points; the
    tail clamped to the last point as ResidualBatch::load does): (number of knot-interval boundaries inside the chunk, whether
    some lane's consecutive rounds — points `group` apart — lie in different intervals).  knots: the oracle's (0-based array of
    FITPACK's t(1..n)); the interval of u is the largest l in [4, n-4] with t(l) <= u, as the kernels' forward search finds it."""
    n = len(knots)
    inner = np.asarray(knots[4 : n - 4])  # t(5) .. t(n-4): entering interval l means passing t(l)
    l = 4 + np.searchsorted(inner, u, side="right")
    sc = group * rounds
    out = []
    for base in range(0, len(u), sc):
        idx = np.minimum(base + np.arange(sc), len(u) - 1)
        li = l[idx]
        across = bool((li[group:] != li[:-group]).any())
        out.append((int(len(np.unique(li))) - 1, across))
    return out
