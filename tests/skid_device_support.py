"""TEST INFRASTRUCTURE: the kernels of a skidpad device ticket (csrc/skid_device_kernel.h) under the host SIMT emulator
(tests/emu/emu_skid_device.cpp, built by tests/emu/skid_device.mk into libraries of their own), and their NumPy restatements."""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

EMU_DIR = Path(__file__).resolve().parent / "emu"
SKID_HIST = 32  # csrc/skid_state.h


class _Emu:
    """one build of the emulated kernels: the standard shapes or the wide ones"""

    def __init__(self, wide):
        self.name = "libfsdp_emu_skid_device_wide.so" if wide else "libfsdp_emu_skid_device.so"
        self.PATH_POINTS = 64 if wide else 40
        self._lib = None
        # NumPy mirrors of the records the kernels move (csrc/skid_state.h SkidState / SkidInfo, csrc/fsdp_device.h PathOut)
        self.state_dtype = np.dtype([("has_original", "<i4"), ("relocalized", "<i4"), ("index_along_path", "<i4"), ("reloc_step", "<i4"),
                                     ("index_hist", "<i4", (SKID_HIST,)), ("orig", "<f8", (4,)), ("translation", "<f8", (2,)),
                                     ("right_calc", "<f8", (2,)), ("rotation", "<f8"), ("prev", "<f8", (self.PATH_POINTS, 4))], align=True)
        self.info_dtype = np.dtype([("relocalized", "<i4"), ("index_along_path", "<i4"), ("translation", "<f8", (2,)), ("rotation", "<f8")], align=True)
        self.path_out_dtype = np.dtype([("path", "<f8", (self.PATH_POINTS, 4)), ("status", "<i4"), ("fallback", "<i4"), ("n_dense", "<i4"), ("pad", "<i4")],
                                       align=True)

    def lib(self):
        if self._lib is None:
            subprocess.run(["make", "-s", "-f", "skid_device.mk", "-C", str(EMU_DIR)], check=True)
            self._lib = ctypes.CDLL(str(EMU_DIR / self.name))
            assert self._lib.emu_skid_device_path_points() == self.PATH_POINTS
            assert self._lib.emu_skid_state_bytes() == self.state_dtype.itemsize
            assert self._lib.emu_skid_state_prev_offset() == self.state_dtype.fields["prev"][1]
            assert self._lib.emu_skid_info_bytes() == self.info_dtype.itemsize
            assert self._lib.emu_skid_path_out_bytes() == self.path_out_dtype.itemsize
        return self._lib


_EMU = {False: _Emu(False), True: _Emu(True)}


def emu(wide: bool = False):
    return _EMU[bool(wide)]


def _v(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def reset(mask, states, default_path, wide=False, blocks=2):
    """skid_device_reset_kernel -> the states afterwards (a copy; `states` itself is left alone)"""
    m = emu(wide)
    mask = np.ascontiguousarray(mask, np.int32)
    out = np.ascontiguousarray(states, m.state_dtype).copy()
    assert len(out) == len(mask)
    default_path = np.ascontiguousarray(default_path, np.float64).reshape(m.PATH_POINTS, 4)
    m.lib().emu_skid_device_reset(ctypes.c_int(len(mask)), _v(mask), _v(out), _v(default_path), ctypes.c_int(blocks))
    return out


def out(path_records, info_records, want_info=True, want_records=True, wide=False, blocks=2):
    """skid_device_out_kernel -> (paths, status, info or None, records or None, the not-relocalized word)"""
    m = emu(wide)
    p = np.ascontiguousarray(path_records, m.path_out_dtype)
    i = np.ascontiguousarray(info_records, m.info_dtype)
    n = len(p)
    paths = np.full((n + 1, m.PATH_POINTS, 4), -7.0)  # (+1: a guard row nothing may write)
    status = np.full(n + 1, -9, np.int32)
    o_info = np.frombuffer(bytes([0xAB]) * (m.info_dtype.itemsize * (n + 1)), m.info_dtype).copy() if want_info else None
    o_rec = np.frombuffer(bytes([0xCD]) * (m.path_out_dtype.itemsize * (n + 1)), m.path_out_dtype).copy() if want_records else None
    word = m.lib().emu_skid_device_out(ctypes.c_int(n), _v(p), _v(i), _v(paths), _v(status), _v(o_info), _v(o_rec), ctypes.c_int(blocks))
    assert (paths[n] == -7.0).all() and status[n] == -9
    assert o_info is None or o_info[n:].tobytes() == bytes([0xAB]) * m.info_dtype.itemsize
    assert o_rec is None or o_rec[n:].tobytes() == bytes([0xCD]) * m.path_out_dtype.itemsize
    return paths[:n], status[:n], None if o_info is None else o_info[:n], None if o_rec is None else o_rec[:n], int(word)


# ---- NumPy restatements ----
def np_fresh_states(n, default_path, wide=False):
    """the bytes fsdp_skidpad_reset writes for n planners: everything zero, previous path = the default path"""
    m = emu(wide)
    s = np.zeros(n, m.state_dtype)
    s["prev"] = np.asarray(default_path, np.float64).reshape(m.PATH_POINTS, 4)
    return s


def np_reset(mask, states, default_path, wide=False):
    s = np.array(states, copy=True)
    hit = np.asarray(mask) != 0
    s[hit] = np_fresh_states(int(hit.sum()), default_path, wide)
    return s


def random_states(n, rng, wide=False):
    """planners in mid-run: every byte of the state random (finite doubles or not: the kernel moves bytes)"""
    m = emu(wide)
    return np.frombuffer(rng.integers(0, 256, n * m.state_dtype.itemsize, dtype=np.uint8).tobytes(), m.state_dtype).copy()


def step_records(n, rng, horizon=None, wide=False, relocalized=None, bad_status=()):
    """a step's records as the skidpad path kernels leave them: rows beyond the horizon NaN, planners in `bad_status`
    {planner: status} with NaN paths"""
    m = emu(wide)
    horizon = m.PATH_POINTS if horizon is None else horizon
    p = np.zeros(n, m.path_out_dtype)
    p["path"] = rng.normal(size=(n, m.PATH_POINTS, 4))
    p["path"][:, horizon:] = np.nan
    p["fallback"] = rng.integers(0, 64, n)
    p["n_dense"] = rng.integers(0, 2000, n)
    for k, st in dict(bad_status).items():
        p["status"][k] = st
        p["path"][k] = np.nan
    i = np.zeros(n, m.info_dtype)
    i["relocalized"] = 1 if relocalized is None else relocalized
    i["index_along_path"] = rng.integers(0, 2893, n)
    i["translation"] = rng.normal(size=(n, 2))
    i["rotation"] = rng.normal(size=n)
    not_reloc = i["relocalized"] == 0
    i["translation"][not_reloc] = np.nan
    i["rotation"][not_reloc] = np.nan
    return p, i
