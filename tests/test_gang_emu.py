"""The gang twins of the plain sorting kernels (csrc/sort_kernel.h sort_kernel_128_gang / sort_kernel_gang) without a GPU: the
kernel sources under the host SIMT emulator (tests/emu/emu_gang.cpp, built by tests/emu/gang.mk).  One twin launch over three
members of different sizes in different places — one of them a slice of a larger batch, cone_offsets[0] != 0 — against three
plain launches that stage one member each: the SortOut records and the staged offsets, cones and poses are equal."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import emu_lib

EMU_DIR = Path(__file__).resolve().parent / "emu"
GUARD = -77.0


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-f", "gang.mk", "-C", str(EMU_DIR)], check=True)
    so = ctypes.CDLL(str(EMU_DIR / "libfsdp_emu_gang.so"))
    assert so.emu_sizeof_sort_out() == emu_lib.SORT_DTYPE.itemsize
    return so


def _ptr(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def members(golden_dir, with_big):
    """[(n, offsets view, cone array the offsets index, poses)]: a whole batch, a slice that keeps its offsets, a third batch"""
    f = np.load(golden_dir / "fuzz.npz")
    off, cones, poses = f["offsets"].astype(np.int32), np.ascontiguousarray(f["cones"], np.float64), np.ascontiguousarray(f["poses"], np.float64)
    a_off = np.ascontiguousarray(off[:12] - off[0])
    a = (11, a_off, np.ascontiguousarray(cones[: a_off[-1]]), np.ascontiguousarray(poses[:11]))
    lo, hi = 50, 57
    assert off[lo] != 0
    b = (hi - lo, np.ascontiguousarray(off[lo : hi + 1]), cones, np.ascontiguousarray(poses[lo:hi]))
    if with_big:  # frames beyond the LDS state of either kernel: sort_big_kernel plans them from the copies
        g = np.load(golden_dir / "big_frames.npz")
        goff = g["offsets"].astype(np.int32)
        assert np.diff(goff[:4]).max() > 255
        c = (3, np.ascontiguousarray(goff[:4]), np.ascontiguousarray(g["cones"], np.float64), np.ascontiguousarray(g["poses"][:3], np.float64))
    else:
        c_off = np.ascontiguousarray(off[300:306] - off[300])
        c = (5, c_off, np.ascontiguousarray(cones[off[300] : off[305]]), np.ascontiguousarray(poses[300:305]))
    return [a, b, c]


def copies(n, rows):
    """destination arrays with a guard element behind each"""
    return np.full(n + 2, int(GUARD), np.int32), np.full(3 * rows + 1, GUARD), np.full(4 * n + 1, GUARD)


@pytest.mark.parametrize("with_big", [False, True], ids=["state128", "state255-big-route"])
def test_gang_twin_equals_three_staged_launches(lib, golden_dir, with_big):
    ms = members(golden_dir, with_big)
    ns = [m[0] for m in ms]
    rows = [int(m[1][-1] - m[1][0]) for m in ms]
    n_all, rows_all = sum(ns), sum(rows)
    d_off, d_cones, d_poses = copies(n_all, rows_all)
    out = np.zeros(n_all, emu_lib.SORT_DTYPE)
    arr_n = (ctypes.c_int * 3)(*ns)
    arr_off = (ctypes.POINTER(ctypes.c_int32) * 3)(*[_ptr(m[1], ctypes.c_int32) for m in ms])
    arr_cones = (ctypes.POINTER(ctypes.c_double) * 3)(*[_ptr(m[2], ctypes.c_double) for m in ms])
    arr_poses = (ctypes.POINTER(ctypes.c_double) * 3)(*[_ptr(m[3], ctypes.c_double) for m in ms])
    rc = lib.emu_sort_gang(3, arr_n, arr_off, arr_cones, arr_poses, _ptr(d_off, ctypes.c_int32), _ptr(d_cones, ctypes.c_double),
                           _ptr(d_poses, ctypes.c_double), ctypes.c_void_p(out.ctypes.data))
    assert rc == 0
    small = lib.emu_gang_last_small()
    assert small == (0 if with_big else 1)
    assert (lib.emu_last_big() > 0) == with_big
    # nothing written behind the copies
    assert d_off[n_all + 1] == int(GUARD) and d_cones[-1] == GUARD and d_poses[-1] == GUARD
    first_frame = first_row = 0
    for (n, off, cones, poses), r in zip(ms, rows):
        p_off, p_cones, p_poses = copies(n, r)
        p_out = np.zeros(n, emu_lib.SORT_DTYPE)
        lib.emu_sort_staged(n, _ptr(off, ctypes.c_int32), _ptr(cones, ctypes.c_double), _ptr(poses, ctypes.c_double), _ptr(p_off, ctypes.c_int32),
                            _ptr(p_cones, ctypes.c_double), _ptr(p_poses, ctypes.c_double), ctypes.c_void_p(p_out.ctypes.data), small)
        assert (p_off[: n + 1] == off - off[0]).all()  # (the plain staging itself: rebased to 0)
        assert out[first_frame : first_frame + n].tobytes() == p_out.tobytes()
        assert (d_off[first_frame : first_frame + n + 1] == p_off[: n + 1] + first_row).all()
        assert d_cones[3 * first_row : 3 * (first_row + r)].tobytes() == p_cones[: 3 * r].tobytes()
        assert d_poses[4 * first_frame : 4 * (first_frame + n)].tobytes() == p_poses[: 4 * n].tobytes()
        first_frame += n
        first_row += r
    assert d_off[n_all] == rows_all  # the closing offset, written by the gang's last frame
    # the records are real: most frames of the fixture sort
    assert (out["status"] == 0).sum() >= n_all // 2
