"""TEST INFRASTRUCTURE: the shortened FP64 sequences of csrc/device_prims.h on the host (tests/emu/seq_model.cpp: the device
bodies, compiled with g++ -ffp-contract=off and the host's exact fma), with the two hardware seeds modelled as the correctly
rounded value times (1 + eps).  Built on demand, like refit_probe."""
from __future__ import annotations

import contextlib
import ctypes
import subprocess
from pathlib import Path

import numpy as np

EMU_DIR = Path(__file__).resolve().parent / "emu"
LIB = EMU_DIR / "libseq_model.so"
_lib = None
_D = ctypes.POINTER(ctypes.c_double)


def lib():
    global _lib
    if _lib is None:
        src = EMU_DIR / "seq_model.cpp"
        deps = [src, EMU_DIR / "hip_emu.h", *sorted((EMU_DIR.parent.parent / "ft-fsd-path-planning_amd" / "csrc").glob("*.h"))]
        if not LIB.exists() or any(LIB.stat().st_mtime < d.stat().st_mtime for d in deps):
            subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-fvisibility=hidden",
                            "-fno-gnu-unique", "-shared", str(src), "-o", str(LIB)], check=True, cwd=str(EMU_DIR))
        _lib = ctypes.CDLL(str(LIB))
        _lib.seq_set_seed_eps.argtypes = [ctypes.c_double, ctypes.c_double]
    return _lib


@contextlib.contextmanager
def seed_eps(eps_rcp, eps_rsq=None):
    """The modelled seeds are RN(1 / d) (1 + eps_rcp) and RN(1 / sqrt(x)) (1 + eps_rsq) inside the block (eps_rsq = eps_rcp by default)."""
    lib().seq_set_seed_eps(float(eps_rcp), float(eps_rcp if eps_rsq is None else eps_rsq))
    try:
        yield
    finally:
        lib().seq_set_seed_eps(0.0, 0.0)


def _in(v):
    return np.ascontiguousarray(v, np.float64)


def _p(a):
    return a.ctypes.data_as(_D)


def rcp_refined(d):
    d = _in(d)
    out = np.empty_like(d)
    lib().seq_rcp_refined(ctypes.c_int(len(d)), _p(d), _p(out))
    return out


def div(a, b, r_ulps=0):
    """div_rcp(a, b, rcp_refined(b)); r_ulps: the refined reciprocal moved by that many representable values (the mutation)."""
    a, b = _in(a), _in(b)
    out = np.empty_like(a)
    lib().seq_div(ctypes.c_int(len(a)), _p(a), _p(b), _p(out), ctypes.c_int(r_ulps))
    return out


def sqrt_1_2(x):
    x = _in(x)
    out = np.empty_like(x)
    lib().seq_sqrt_1_2(ctypes.c_int(len(x)), _p(x), _p(out))
    return out


def givens(piv, ww, rd_ulps=0):
    """(4, n): cs, sn, dd, guard of fpgivs_guarded<true>; rd_ulps: the seeded reciprocal of dd moved (the mutation)."""
    piv, ww = _in(piv), _in(ww)
    out = np.empty((4, len(piv)))
    lib().seq_givens(ctypes.c_int(len(piv)), _p(piv), _p(ww), _p(out), ctypes.c_int(rd_ulps))
    return out


def in_band(a, b):
    a, b = _in(a), _in(b)
    out = np.empty_like(a)
    lib().seq_in_band(ctypes.c_int(len(a)), _p(a), _p(b), _p(out))
    return out


# the seed errors the CPU test runs the model at (index = the key in tests/golden/seq_model_known.npz)
EPS = (0.0, 2.0**-20, -(2.0**-20), 2.0**-24, -(2.0**-24), 2.0**-28, -(2.0**-28))


def failing_operands(eps):
    """{"div|<set>": (k, 2) a, b; "sqrt|<set>": (k,) x; "giv|<set>": (k, 2) piv, ww}: the operands of tests/hard_rounding.py on
    which the model with seed error eps differs from the exact reference (a Givens pair counts when cs, sn or dd differs)."""
    import hard_rounding as hr

    out = {}
    with seed_eps(eps):
        for k, (a, b) in hr.division_sets().items():
            bad = hr.bits(div(a, b)) != hr.bits(hr.division_references()[k])
            out["div|" + k] = np.stack([a[bad], b[bad]], axis=1)
        for k, x in hr.sqrt_sets().items():
            out["sqrt|" + k] = x[hr.bits(sqrt_1_2(x)) != hr.bits(hr.sqrt_references()[k])]
        for k, (p, w) in hr.givens_sets().items():
            o, ref = givens(p, w), hr.givens_references()[k]
            bad = (hr.bits(o[:3]) != hr.bits(ref)).any(axis=0)
            out["giv|" + k] = np.stack([p[bad], w[bad]], axis=1)
    return out
