"""TEST INFRASTRUCTURE: the kernels of a device ticket (csrc/device_io_kernel.h) under the host SIMT emulator
(tests/emu/emu_device_io.cpp, built by tests/emu/device_io.mk into libraries of their own), and their NumPy restatements."""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

EMU_DIR = Path(__file__).resolve().parent / "emu"


class _Emu:
    """one build of the emulated kernels: the standard shapes or the wide ones"""

    def __init__(self, wide):
        self.name = "libfsdp_emu_device_io_wide.so" if wide else "libfsdp_emu_device_io.so"
        self.PATH_POINTS = 64 if wide else 40
        self._lib = None

    def lib(self):
        if self._lib is None:
            subprocess.run(["make", "-s", "-f", "device_io.mk", "-C", str(EMU_DIR)], check=True)
            self._lib = ctypes.CDLL(str(EMU_DIR / self.name))
            assert self._lib.emu_device_io_path_points() == self.PATH_POINTS
        return self._lib


_EMU = {False: _Emu(False), True: _Emu(True)}


def emu(wide: bool = False):
    return _EMU[bool(wide)]


def _p(a, t):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))


def scan(counts, cap, wide=False):
    """device_scan_kernel -> (offsets (n + 1), lowest frame with a count outside [0, cap] or -1)"""
    counts = np.ascontiguousarray(counts, np.int32)
    off = np.full(len(counts) + 1, -7, np.int32)
    bad = emu(wide).lib().emu_device_scan(ctypes.c_int(len(counts)), ctypes.c_int(cap), _p(counts, ctypes.c_int32), _p(off, ctypes.c_int32))
    return off, int(bad)


def gather(counts, cones, poses, prev=None, wide=False, blocks=7, fill=np.nan):
    """scan + device_gather_kernel -> (offsets, cone rows (n * cap, 3) with untouched rows = `fill`, poses, prev copy or None, bad)"""
    m = emu(wide)
    counts = np.ascontiguousarray(counts, np.int32)
    n = len(counts)
    cones = np.ascontiguousarray(cones, np.float64).reshape(n, -1, 3)
    cap = cones.shape[1]
    poses = np.ascontiguousarray(poses, np.float64).reshape(n, 4)
    off = np.full(n + 1, -7, np.int32)
    d_cones = np.full((n * cap + 1, 3), fill)  # (+1: a guard row nothing may write)
    d_poses = np.full((n, 4), fill)
    d_prev = None
    if prev is not None:
        prev = np.ascontiguousarray(prev, np.float64).reshape(n, m.PATH_POINTS, 4)
        d_prev = np.full(prev.shape, fill)
    bad = m.lib().emu_device_gather(ctypes.c_int(n), ctypes.c_int(cap), _p(counts, ctypes.c_int32), _p(cones, ctypes.c_double) if cap else None,
                                    _p(poses, ctypes.c_double), _p(prev, ctypes.c_double), _p(off, ctypes.c_int32), _p(d_cones, ctypes.c_double),
                                    _p(d_poses, ctypes.c_double), _p(d_prev, ctypes.c_double), ctypes.c_int(blocks))
    return off, d_cones, d_poses, d_prev, int(bad)


def out(sort_status, match_status, path_status, path_rows, prev, default_path, want_next=True, wide=False, blocks=5):
    """device_out_kernel -> (paths, status, next_prev or None)"""
    m = emu(wide)
    st = [np.ascontiguousarray(s, np.int32) for s in (sort_status, match_status, path_status)]
    n = len(st[0])
    rows = np.ascontiguousarray(path_rows, np.float64).reshape(n, m.PATH_POINTS, 4)
    prev = None if prev is None else np.ascontiguousarray(prev, np.float64).reshape(n, m.PATH_POINTS, 4)
    default_path = np.ascontiguousarray(default_path, np.float64).reshape(m.PATH_POINTS, 4)
    paths = np.zeros_like(rows)
    status = np.full(n, -9, np.int32)
    nxt = np.zeros_like(rows) if want_next else None
    m.lib().emu_device_out(ctypes.c_int(n), *[_p(s, ctypes.c_int32) for s in st], _p(rows, ctypes.c_double), _p(prev, ctypes.c_double),
                           _p(default_path, ctypes.c_double), _p(paths, ctypes.c_double), _p(status, ctypes.c_int32), _p(nxt, ctypes.c_double),
                           ctypes.c_int(blocks))
    return paths, status, nxt


# ---- NumPy restatements ----
def np_clamp(counts, cap):
    counts = np.asarray(counts, np.int64)
    return np.where((counts < 0) | (counts > cap), 0, counts)


def np_scan(counts, cap):
    counts = np.asarray(counts, np.int64)
    off = np.concatenate([[0], np.cumsum(np_clamp(counts, cap))]).astype(np.int32)
    bad = np.flatnonzero((counts < 0) | (counts > cap))
    return off, (int(bad[0]) if len(bad) else -1)


def np_gather(counts, cones):
    """the frames' first counts[f] rows, in order"""
    cones = np.asarray(cones, np.float64)
    c = np_clamp(counts, cones.shape[1])
    keep = np.arange(cones.shape[1])[None, :] < c[:, None]
    return cones[keep]


def pad_frames(offsets, cones, cap=None, fill=np.nan):
    """a CSR batch -> (counts (n) int32, (n, cap, 3) tensor whose padding rows hold `fill`)"""
    offsets = np.asarray(offsets, np.int64)
    cones = np.asarray(cones, np.float64).reshape(-1, 3)
    counts = np.diff(offsets).astype(np.int32)
    cap = int(counts.max(initial=0)) if cap is None else int(cap)
    out = np.full((len(counts), cap, 3), fill)
    keep = np.arange(cap)[None, :] < counts[:, None]
    out[keep] = cones[offsets[0]:offsets[-1]]
    return counts, out
