"""ctypes binding of the ranked sorting kernels under the host SIMT emulator (tests/emu_ranked/emu_ranked.cpp): the
kernel sources behind fsdp_sort_batch_ranked executed on the CPU, standard and wide (-DFSDP_WIDE_SHAPES) shapes.
TEST INFRASTRUCTURE: built with the compiler flags of tests/emu/Makefile into tests/emu_ranked/*.so (git-ignored)."""
from __future__ import annotations

import ctypes
import os
import re
import shlex
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SRC_DIR = ROOT / "tests" / "emu_ranked"
SRC = SRC_DIR / "emu_ranked.cpp"
RANK_MAX, COST_TERMS = 64, 7


def _makefile_flags():
    text = (ROOT / "tests" / "emu" / "Makefile").read_text()
    return shlex.split(re.search(r"^CXXFLAGS \?= (.*)$", text, re.M).group(1))


def _lib_path(wide):
    return SRC_DIR / ("libfsdp_emu_ranked_wide.so" if wide else "libfsdp_emu_ranked.so")


def build(wide=None):
    """Compile the library (both when wide is None) unless it is newer than every source it includes."""
    deps = [SRC, ROOT / "tests" / "emu" / "hip_emu.h", ROOT / "include" / "fsdp.h", *sorted((ROOT / "ft-fsd-path-planning_amd" / "csrc").glob("*.h"))]
    newest = max(d.stat().st_mtime for d in deps)
    jobs = []
    for w in ((False, True) if wide is None else (wide,)):
        out = _lib_path(w)
        if out.exists() and out.stat().st_mtime >= newest:
            continue
        cmd = [os.environ.get("CXX", "g++"), *_makefile_flags(), *(["-DFSDP_WIDE_SHAPES"] if w else []), "-shared", str(SRC), "-o", str(out)]
        jobs.append(subprocess.Popen(cmd))
    for j in jobs:
        assert j.wait() == 0, "emu_ranked build failed"


def _p(a, t=ctypes.c_double):
    return a.ctypes.data_as(ctypes.POINTER(t))


class Emu:
    """One build of the emulated ranked kernels."""

    def __init__(self, wide=False):
        build(wide)
        self.wide = wide
        self.lib = ctypes.CDLL(str(_lib_path(wide)))
        self.max_len = int(self.lib.emu_ranked_max_len())
        assert self.max_len == (16 if wide else 12)
        import emu_lib_wide, emu_lib  # noqa: E401 (the record layouts)

        self.sort_dtype = (emu_lib_wide if wide else emu_lib).SORT_DTYPE
        assert self.lib.emu_ranked_sizeof_sort_out() == self.sort_dtype.itemsize

    def set_params(self, overrides):
        import oracle_lib

        self.lib.emu_ranked_set_params(_p(oracle_lib.param_vector(overrides)))

    def set_no_sort128(self, on):
        self.lib.emu_ranked_set_no_sort128(ctypes.c_int(1 if on else 0))

    def last_kernels(self):
        """bit 0 / 1 / 2: sort_kernel_128_ranked / sort_kernel_ranked / sort_big_kernel_ranked ran in the last call"""
        return int(self.lib.emu_ranked_last_kernels())

    def last_big(self):
        return int(self.lib.emu_ranked_last_big())

    def sort_ranked(self, offsets, cones, poses, top_k=8, terms=True):
        """-> (sort records, counts (n,2), configs (n,2,top_k,MAX_LEN), costs (n,2,top_k), terms (n,2,top_k,7) or None);
        raises ValueError for a top_k the kernels refuse"""
        offsets = np.ascontiguousarray(offsets, np.int32)
        cones = np.ascontiguousarray(cones, np.float64)
        poses = np.ascontiguousarray(poses, np.float64)
        n = len(offsets) - 1
        k = max(1, min(int(top_k), RANK_MAX))
        out = np.zeros(n, self.sort_dtype)
        counts = np.zeros((n, 2), np.int32)
        configs = np.zeros((n, 2, k, self.max_len), np.int32)
        costs = np.zeros((n, 2, k))
        tm = np.zeros((n, 2, k, COST_TERMS)) if terms else None
        rc = self.lib.emu_sort_ranked(ctypes.c_int(n), _p(offsets, ctypes.c_int32), _p(cones), _p(poses), ctypes.c_void_p(out.ctypes.data),
                                      ctypes.c_int(int(top_k)), _p(counts, ctypes.c_int32), _p(configs, ctypes.c_int32), _p(costs),
                                      _p(tm) if terms else None)
        if rc != 0:
            raise ValueError(f"top_k = {top_k} refused")
        return out, counts, configs, costs, tm


_emus = {}


def emu(wide=False):
    if wide not in _emus:
        _emus[wide] = Emu(wide)
    return _emus[wide]


if __name__ == "__main__":
    build()
    print("emu_ranked build ok")
