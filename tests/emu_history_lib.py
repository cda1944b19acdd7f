"""TEST INFRASTRUCTURE: the history instantiations of the sorting kernels (csrc/sort_history_kernels.h) under the host SIMT
emulator (tests/emu/emu_history.cpp, built by tests/emu/history.mk into libraries of their own together with emu_kernels.cpp)."""
from __future__ import annotations

import contextlib
import ctypes
import subprocess
from pathlib import Path

import numpy as np

EMU_DIR = Path(__file__).resolve().parent / "emu"
GUARD32, GUARD8 = -77, 0x5A  # the guard row behind every array of a call: nothing may write it


def _p(a, t):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))


class _Emu:
    """one build of the emulated kernels: the standard shapes or the wide ones"""

    def __init__(self, wide):
        self.wide = bool(wide)
        self.name = "libfsdp_emu_history_wide.so" if wide else "libfsdp_emu_history.so"
        self.MAX_LEN, self.MAX_NEIGHBORS = (16, 8) if wide else (12, 5)
        self._lib = None

    def lib(self):
        if self._lib is None:
            subprocess.run(["make", "-s", "-f", "history.mk", "-C", str(EMU_DIR)], check=True)
            self._lib = ctypes.CDLL(str(EMU_DIR / self.name))
            assert self._lib.emu_history_max_neighbors() == self.MAX_NEIGHBORS
            assert self._lib.emu_sizeof_sort_out() == self.plain_lib().SORT_DTYPE.itemsize
        return self._lib

    def plain_lib(self):
        """tests/emu_lib.py of the same shapes (record layout, the ranked call)"""
        import emu_lib
        import emu_lib_wide

        return emu_lib_wide if self.wide else emu_lib

    def oracle(self):
        import oracle_lib
        import oracle_lib_wide

        return oracle_lib_wide if self.wide else oracle_lib

    @contextlib.contextmanager
    def params(self, overrides):
        """the configuration constants of this library's kernels and of tests/emu_lib.py's (the ranked call of the checks)"""
        o = self.oracle()
        v, d = o.param_vector(overrides), o.param_vector(None)
        with self.plain_lib().params(overrides):
            self.lib().emu_set_params(_p(v, ctypes.c_double))
            try:
                yield
            finally:
                self.lib().emu_set_params(_p(d, ctypes.c_double))

    @contextlib.contextmanager
    def no_sort128(self, on=True):
        self.lib().emu_set_no_sort128(ctypes.c_int(int(on)))
        try:
            yield
        finally:
            self.lib().emu_set_no_sort128(ctypes.c_int(0))

    def last_kernels(self):
        """bit 0 / 1 / 2: sort_kernel_128_history / sort_kernel_history / sort_big_kernel_history ran in the last call"""
        return int(self.lib().emu_history_last_kernels())

    def last_big(self):
        return int(self.lib().emu_last_big())

    def _inputs(self, offsets, cones, poses):
        return (np.ascontiguousarray(offsets, np.int32), np.ascontiguousarray(cones, np.float64), np.ascontiguousarray(poses, np.float64))

    def sort(self, offsets, cones, poses):
        """the plain kernels on the same route, indices in the caller's array: what fsdp_sort_batch returns"""
        offsets, cones, poses = self._inputs(offsets, cones, poses)
        n = len(offsets) - 1
        out = np.zeros(n, self.plain_lib().SORT_DTYPE)
        self.lib().emu_sort(ctypes.c_int(n), _p(offsets, ctypes.c_int32), _p(cones, ctypes.c_double), _p(poses, ctypes.c_double),
                            ctypes.c_void_p(out.ctypes.data))
        self.lib().emu_sort_remap(ctypes.c_int(n), ctypes.c_void_p(out.ctypes.data))
        return out

    def sort_history(self, offsets, cones, poses, rows_cap=256, verdicts=True):
        """The history kernels, wrapped like the library's fsdp_sort_batch_history -> (sort records, dict of n_rows (n,2),
        target_length (n,2), rows (n,2,rows_cap,MAX_LEN), is_end (n,2,rows_cap), cand / verdict (n,2,rows_cap,MAX_NEIGHBORS) or
        None).  Every array is allocated with a guard row behind it, which is checked here.  Raises ValueError for a call the
        kernels' wrapper refuses."""
        offsets, cones, poses = self._inputs(offsets, cones, poses)
        n = len(offsets) - 1
        k = max(1, int(rows_cap))
        L, K = self.MAX_LEN, self.MAX_NEIGHBORS
        out = np.zeros(n, self.plain_lib().SORT_DTYPE)
        n_rows = np.full(2 * n + 1, GUARD32, np.int32)
        target = np.full(2 * n + 1, GUARD32, np.int32)
        rows = np.full((2 * n * k + 1) * L, GUARD32, np.int32)
        is_end = np.full(2 * n * k + 1, GUARD8, np.uint8)
        cand = np.full((2 * n * k + 1) * K, GUARD32, np.int32) if verdicts else None
        verdict = np.full((2 * n * k + 1) * K, GUARD8, np.uint8) if verdicts else None
        rc = self.lib().emu_sort_history(ctypes.c_int(n), _p(offsets, ctypes.c_int32), _p(cones, ctypes.c_double), _p(poses, ctypes.c_double),
                                         ctypes.c_void_p(out.ctypes.data), ctypes.c_int(int(rows_cap)), _p(n_rows, ctypes.c_int32),
                                         _p(target, ctypes.c_int32), _p(rows, ctypes.c_int32), _p(is_end, ctypes.c_uint8),
                                         _p(cand, ctypes.c_int32), _p(verdict, ctypes.c_uint8))
        if rc != 0:
            raise ValueError(f"rows_cap = {rows_cap} refused")
        assert n_rows[-1] == GUARD32 and target[-1] == GUARD32 and (rows[-L:] == GUARD32).all() and is_end[-1] == GUARD8
        h = dict(n_rows=n_rows[:-1].reshape(n, 2), target_length=target[:-1].reshape(n, 2), rows=rows[:-L].reshape(n, 2, k, L),
                 is_end=is_end[:-1].reshape(n, 2, k), cand=None, verdict=None)
        if verdicts:
            assert (cand[-K:] == GUARD32).all() and (verdict[-K:] == GUARD8).all()
            h["cand"], h["verdict"] = cand[:-K].reshape(n, 2, k, K), verdict[:-K].reshape(n, 2, k, K)
        return out, h


_EMU = {False: _Emu(False), True: _Emu(True)}


def emu(wide: bool = False):
    return _EMU[bool(wide)]
