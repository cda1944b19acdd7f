"""Inputs and expectations of the per-frame global path tests (tests/test_gpath_table_cpu.py, tests/test_gpath_table_gpu.py), and
the ctypes binding of the TABLE twins of the path wrappers under the host SIMT emulator (tests/emu/emu_gpath_table.cpp, built by
tests/emu/gpath_table.mk).  TEST INFRASTRUCTURE.

The table holds paths of deliberately different sizes, so that the lane groups of one wavefront run the window loops of
csrc/path_kernel.h path_front with different trip counts, or not at all:

  ACC    the shipped acceleration path (1650 points, a U of two 160 m lanes)
  SKID   a slice of the shipped skidpad table (every fourth point of a 1600-point stretch)
  SHORT  five points, fewer than the lanes of the smallest group
  ZERO   no point at all: status 103 (the reference's argmin of an empty array)
  DENSE  1500 points on 20 m: more than PATH_CAP = 1408 within 30 m of the car, status 203
  TRACK  the closed track of tests/golden/global_path.npz
  ZIGZAG 60 points left and right of a line: a first fit of more than the 32 knots the packed kernels keep, so the frame is handed to
         the retry route (RetryBatch)

Expected values never come from the code under test: each frame is planned by the oracle with that path alone
(oracle_lib.plan_frame_global, as tests/test_global_path.py uses it)."""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

import emu_lib
import oracle_lib

ROOT = Path(__file__).resolve().parent.parent
DATA = ROOT / "ft-fsd-path-planning_amd" / "data"
EMU_DIR = ROOT / "tests" / "emu"
GOLDEN = ROOT / "tests" / "golden"

PATH_CAP = 1408
ST_REF_UNDEFINED_PATH, ST_OVERFLOW_PATH = 103, 203
ACC, SKID, SHORT, ZERO, DENSE, TRACK, ZIGZAG = range(7)
CONES = -1  # the id of a frame that plans from its cones


def paths():
    """The table's polylines, in id order."""
    g = np.load(GOLDEN / "global_path.npz")
    short = np.column_stack([np.arange(5) * 2.5, 0.05 * np.arange(5) ** 2])
    dense = np.column_stack([np.linspace(0.0, 20.0, 1500), np.zeros(1500)])
    zigzag = np.column_stack([0.7 * np.arange(60), 0.3 * (2.0 * (np.arange(60) % 2) - 1.0)])
    return [np.load(DATA / "acceleration_path.npy"), np.ascontiguousarray(np.load(DATA / "skidpad_path.npy")[1000:2600:4]), short, np.zeros((0, 2)), dense,
            np.ascontiguousarray(g["gp_track"]), zigzag]


class RetryBatch:
    """Eight frames without cones, five of them on the zigzag path: the packed kernels hand those to the retry route, whose
    four-frame form then holds frames with and without a path in one wavefront.  Expected values: the oracle, frame by frame."""

    IDS = np.array([ZIGZAG, CONES, ZIGZAG, SHORT, ZIGZAG, ZIGZAG, CONES, ZIGZAG], np.int32)

    def __init__(self):
        self.paths = paths()
        self.xy, self.path_off = table(self.paths)
        self.ids = self.IDS.copy()
        self.n = len(self.ids)
        self.off = np.zeros(self.n + 1, np.int32)
        self.cones = np.zeros((0, 3))
        self.poses = np.array([[3.0 + 2.0 * i, 0.1, 1.0, 0.0] for i in range(self.n)])
        self.ref = np.zeros(self.n, oracle_lib.RESULT_DTYPE)
        with oracle_lib.math_mode(1):
            for f in range(self.n):
                self.ref[f] = oracle_lib.plan_frame_global(self.cones, self.poses[f], None, None if self.ids[f] < 0 else self.paths[self.ids[f]])


def table(path_list):
    """(xy (sum, 2), offsets (n + 1) int32) of fsdp_set_global_path_table"""
    off = np.zeros(len(path_list) + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p in path_list])
    xy = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p in path_list]))
    return xy, off


class Mixed:
    """The 16-frame mixed batch.  Its ids put, into the same wavefront on every route — 8 lanes per frame (frames 0-7, 8-15), 16 lanes
    per frame and the retry kernel's four-frame form (frames 4k .. 4k + 3) — a cone-planned frame next to a long path (0, 1), a short
    path next to a long one (2, 3), the empty path next to others (4; 15), the overfull path between planned frames (7 between 6 and
    8 / 5), a car more than 30 m from its path (8), and a frame without cones or path, which falls back on its previous path (9)."""

    IDS = np.array([CONES, ACC, SHORT, ACC, ZERO, SKID, CONES, DENSE, ACC, CONES, TRACK, SHORT, SKID, CONES, ACC, ZERO], np.int32)

    def __init__(self):
        g = np.load(GOLDEN / "global_path.npz")
        self.paths = paths()
        self.xy, self.path_off = table(self.paths)
        self.ids = self.IDS.copy()
        n = len(self.ids)
        skid = self.paths[SKID]
        off, cones, poses = [0], [], np.zeros((n, 4))
        for f, pid in enumerate(self.ids):
            t = (3 * f) % 40  # the golden recording's frame whose cones (and, for CONES / TRACK, pose) the frame takes
            xyt = g["gp_cones"][g["gp_offsets"][t] : g["gp_offsets"][t + 1]]
            if pid in (CONES, TRACK):
                poses[f] = g["gp_poses"][t]
            elif pid == ACC:
                poses[f] = [12.5 * f + 3.0, 0.2 - 0.03 * f, np.cos(0.02 * f), np.sin(0.02 * f)]
            elif pid == SKID:
                k = 40 * (f % 7) + 60
                d = skid[k + 1] - skid[k]
                poses[f] = [*(skid[k] + [0.1, -0.2]), *(d / np.hypot(*d))]
            elif pid == SHORT:
                poses[f] = [1.0 + 0.5 * f, 0.3, 1.0, 0.0]
            elif pid == DENSE:
                poses[f] = [10.0, 0.5, 1.0, 0.0]
            else:  # ZERO
                poses[f] = [float(f), 1.0, 0.0, 1.0]
                xyt = xyt[:0]
            if f == 9:
                xyt = xyt[:0]  # no cones, no path: the previous path
            if pid not in (CONES, TRACK):
                xyt = xyt[:0]  # (a car on another path is nowhere near the recording's cones: none, as for a relocalized planner)
            cones.append(xyt)
            off.append(off[-1] + len(xyt))
        poses[8, :2] = [75.0, 40.0]  # more than 30 m from every point of ACC
        self.off = np.array(off, np.int32)
        self.cones = np.ascontiguousarray(np.concatenate(cones).reshape(-1, 3))
        self.poses = poses
        self.n = n
        rng = np.random.default_rng(11)
        self.prev = np.repeat(oracle_lib.default_path()[None], n, axis=0)
        self.prev[:, :, 1:3] += rng.normal(0, 0.02, (n, self.prev.shape[1], 2))  # a previous path of its own per frame
        self.ref = self.oracle(self.prev)

    def frame_cones(self, f):
        return self.cones[self.off[f] : self.off[f + 1]]

    def oracle(self, prev, ids=None):
        """every frame by the oracle with its own path alone (math mode 1: the kernels' deterministic libm)"""
        ids = self.ids if ids is None else ids
        out = np.zeros(self.n, oracle_lib.RESULT_DTYPE)
        with oracle_lib.math_mode(1):
            for f in range(self.n):
                gp = None if ids[f] < 0 else self.paths[ids[f]]
                out[f] = oracle_lib.plan_frame_global(self.frame_cones(f), self.poses[f], None if prev is None else prev[f], gp)
        return out

    def check(self, status, path, ref=None, what=""):
        """status / path of all frames against the oracle's; the overfull path is the library's own refusal (the oracle has no capacity)"""
        ref = self.ref if ref is None else ref
        for f in range(self.n):
            if self.ids[f] == DENSE:
                assert int(status[f]) == ST_OVERFLOW_PATH and np.isnan(path[f]).all(), (what, f, int(status[f]))
                continue
            assert int(status[f]) == int(ref["status"][f]), (what, f, int(status[f]), int(ref["status"][f]))
            if ref["status"][f] == 0:
                assert np.asarray(path[f]).tobytes() == ref["path"][f].tobytes(), (what, f, np.nanmax(np.abs(path[f] - ref["path"][f])))
            else:
                assert np.isnan(path[f]).all(), (what, f)


# ---- the emulator -----------------------------------------------------------------------------------------------------------------
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-f", "gpath_table.mk", "-C", str(EMU_DIR)], check=True)
        _lib = ctypes.CDLL(str(EMU_DIR / "libfsdp_emu_gpath_table.so"))
        assert _lib.emu_sizeof_path_out() == emu_lib.PATH_DTYPE.itemsize and _lib.emu_sizeof_match_out() == emu_lib.MATCH_DTYPE.itemsize
    return _lib


FORMS = {"prep8": 8, "mono16": 16, "mono64": 64, "retry": 0}


def emulate(form, off, cones, poses, prev, xy, path_off, ids):
    """sort -> match (tests/emu_lib.py: the plain kernels) -> the path stage of a pass with ids in the given form -> (status, path
    records, frames handed to the retry route)"""
    poses = np.ascontiguousarray(poses, np.float64)
    s = emu_lib.sort(off, cones, poses)
    m = emu_lib.match(off, cones, poses, s)
    n = len(poses)
    out = np.zeros(n, emu_lib.PATH_DTYPE)
    out["path"] = 7.0  # (what the kernels do not write would show)
    prev = None if prev is None else np.ascontiguousarray(prev, np.float64)
    xy = np.ascontiguousarray(xy, np.float64)
    xy_arg = xy if len(xy) else np.zeros((1, 2))  # (the library keeps room for one point: an empty entry still has an address)
    path_off = np.ascontiguousarray(path_off, np.int32)
    ids = np.ascontiguousarray(ids, np.int32)
    dp = ctypes.POINTER(ctypes.c_double)
    ip = ctypes.POINTER(ctypes.c_int32)
    rc = lib().emu_gpt_path(ctypes.c_int(FORMS[form]), ctypes.c_int(n), poses.ctypes.data_as(dp), ctypes.c_void_p(m.ctypes.data),
                            None if prev is None else prev.ctypes.data_as(dp), xy_arg.ctypes.data_as(dp), path_off.ctypes.data_as(ip),
                            ctypes.c_int(len(path_off) - 1), ids.ctypes.data_as(ip), ctypes.c_void_p(out.ctypes.data))
    assert rc == 0
    status = np.where(out["status"] != 0, out["status"], np.where(m["status"] != 0, m["status"], s["status"]))
    return status, out, int(lib().emu_gpt_last_retries())


def ids_scan(ids, n_paths):
    ids = np.ascontiguousarray(ids, np.int32)
    return int(lib().emu_gpt_ids_scan(ctypes.c_int(len(ids)), ctypes.c_int(n_paths), ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
