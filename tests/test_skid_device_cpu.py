"""CPU-side checks of the skidpad device tickets (fsdp_skidpad_submit_device): the two kernels of csrc/skid_device_kernel.h under
the host SIMT emulator against NumPy, in both builds — the out kernel's arrays, optional records and relocalized word over grids
smaller than the fleet, the reset kernel's masks against the bytes fsdp_skidpad_reset writes — and the ABI's declaration against
both built libraries and the binding, with the refusals that need no GPU."""
import ctypes
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

import skid_device_support as sds

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [1, 3, 5, 64, 67])
def test_out_kernel_hands_over_the_records_of_a_step(n, wide):
    m = sds.emu(wide)
    rng = np.random.default_rng(100 + n)
    horizon = m.PATH_POINTS - 8  # rows beyond the horizon are NaN, and stay NaN
    bad = {k: st for k, st in ((0, 103), (n // 2, 205), (n - 1, 206)) if n >= 5}  # (status != 0 rows: NaN paths)
    p, i = sds.step_records(n, rng, horizon=horizon, wide=wide, bad_status=bad)
    blocks = 1 if n == 1 else 2  # two wavefronts walk n planners: (n + 1) // 2 trips each
    for want_info in (True, False):
        for want_records in (True, False):
            paths, status, info, rec, word = sds.out(p, i, want_info, want_records, wide=wide, blocks=blocks)
            assert paths.tobytes() == p["path"].tobytes()
            assert np.isnan(paths[:, horizon:]).all() and not np.isnan(paths[[k for k in range(n) if k not in bad], :horizon]).any()
            assert status.tobytes() == p["status"].tobytes()
            assert (info is None) == (not want_info) and (rec is None) == (not want_records)
            if want_info:
                assert info.tobytes() == i.tobytes()
            if want_records:
                assert rec.tobytes() == p.tobytes()
            assert word == 0
    if n >= 5:
        assert sorted(set(status.tolist())) == [0, 103, 205, 206]
        assert np.isnan(paths[list(bad)]).all()
    # any grid walks any fleet
    for blocks in (1, 3, n, n + 5):
        got = sds.out(p, i, wide=wide, blocks=blocks)
        assert got[0].tobytes() == p["path"].tobytes() and got[2].tobytes() == i.tobytes() and got[3].tobytes() == p.tobytes()


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [1, 3, 5, 64, 67])
def test_relocalized_word_is_zero_only_when_every_planner_is_relocalized(n, wide):
    rng = np.random.default_rng(200 + n)
    blocks = 1 if n == 1 else 2
    for who in sorted({0, n // 2, n - 1, min(63, n - 1), min(64, n - 1)}):
        reloc = np.ones(n, np.int32)
        p, i = sds.step_records(n, rng, wide=wide, relocalized=reloc)
        assert sds.out(p, i, wide=wide, blocks=blocks)[4] == 0
        reloc[who] = 0
        p, i = sds.step_records(n, rng, wide=wide, relocalized=reloc)
        paths, status, info, rec, word = sds.out(p, i, wide=wide, blocks=blocks)
        assert word == 1, who
        assert info.tobytes() == i.tobytes() and np.isnan(info["rotation"][who])
        assert sds.out(p, i, want_info=False, want_records=False, wide=wide, blocks=blocks)[4] == 1  # (the word does not need the info array)
    p, i = sds.step_records(n, rng, wide=wide, relocalized=np.zeros(n, np.int32))
    assert sds.out(p, i, wide=wide, blocks=blocks)[4] == 1


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [1, 64, 65, 131])
def test_reset_kernel_writes_fresh_planners_and_touches_no_other(n, wide):
    m = sds.emu(wide)
    rng = np.random.default_rng(300 + n)
    states = sds.random_states(n, rng, wide)
    default = rng.normal(size=(m.PATH_POINTS, 4))
    default[m.PATH_POINTS - 3:] = np.nan  # (rows beyond a shorter horizon)
    fresh = sds.np_fresh_states(n, default, wide)
    masks = [np.zeros(n, np.int32), np.ones(n, np.int32)]
    for k in sorted({0, n - 1, min(63, n - 1), min(64, n - 1)}):
        one = np.zeros(n, np.int32)
        one[k] = 1
        masks.append(one)
    if n > 64:
        both = np.zeros(n, np.int32)
        both[[63, 64]] = (-1, 7)  # any non-zero entry resets
        masks.append(both)
    for mask in masks:
        for blocks in (1, 2, n + 3):
            got = sds.reset(mask, states, default, wide=wide, blocks=blocks)
            hit = mask != 0
            assert got[~hit].tobytes() == states[~hit].tobytes()  # untouched planners byte-equal
            assert got[hit].tobytes() == fresh[hit].tobytes()     # reset planners: the bytes fsdp_skidpad_reset writes
            assert got.tobytes() == sds.np_reset(mask, states, default, wide).tobytes()
    assert sds.reset(masks[0], states, default, wide=wide).tobytes() == states.tobytes()
    assert sds.reset(masks[1], states, default, wide=wide).tobytes() == fresh.tobytes()


def test_fresh_state_is_what_the_host_reset_writes():
    """fsdp_skidpad_reset (csrc/fsdp_lib.hip): memset(&s, 0, sizeof(s)); memcpy(s.prev, default_path, sizeof(default_path)) — the
    restatement the reset kernel is held to, read from the source so that the two cannot drift apart unnoticed."""
    src = (ROOT / "ft-fsd-path-planning_amd" / "csrc" / "fsdp_lib.hip").read_text()
    body = re.search(r"int fsdp_skidpad_reset\(.*?\n}\n", src, re.S).group(0)
    assert re.search(r"memset\(&s, 0, sizeof\(s\)\);\s*memcpy\(s\.prev, def, sizeof\(def\)\);", body)
    for wide in (False, True):
        m = sds.emu(wide)
        m.lib()
        assert m.state_dtype.fields["prev"][1] + 8 * 4 * m.PATH_POINTS == m.state_dtype.itemsize  # prev ends the state: no tail


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge

    ge.build_hip()
    return importlib.import_module("ft-fsd-path-planning_amd")


def test_symbol_is_declared_exported_and_bound(pkg):
    header = (ROOT / "include" / "fsdp.h").read_text()
    declared = set(re.findall(r"\b(fsdp_[a-z0-9_]+)\s*\(", header))
    sym = "fsdp_skidpad_submit_device"
    assert sym in declared and sym in pkg._capi.EXPORTED_SYMBOLS
    for shapes in (pkg._capi.STANDARD, pkg._capi.WIDE):
        assert hasattr(ctypes.CDLL(str(shapes.lib_path)), sym), shapes.name
        assert len(pkg._capi.load(shapes).fsdp_skidpad_submit_device.argtypes) == 13
    proto = re.search(r"int fsdp_skidpad_submit_device\((.*?)\);", header, re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in proto.replace("\n", " ").split(",")]
    assert names == ["ctx", "n_instances", "cone_capacity", "counts", "cones", "poses", "reset", "paths", "status", "info", "records",
                     "after_stream", "ticket"]
    assert callable(pkg.SkidpadBatch.submit_device) and callable(pkg.SkidpadDeviceFleet.step)
    assert "skidpad calls" not in re.search(r"Not offered \(see DESIGN.md 9\)(.*?)\*/", header, re.S).group(1)
    # the binding's records are the ABI's
    assert pkg.skidpad.INFO_DTYPE.itemsize == 32 and pkg.skidpad.INFO_DTYPE == sds.emu(False).info_dtype


def test_refusals_that_need_no_gpu(pkg):
    t = ctypes.c_longlong(7)
    for shapes in (pkg._capi.STANDARD, pkg._capi.WIDE):
        lib = pkg._capi.load(shapes)
        # no context, no ticket word: an error code, nothing dereferenced
        assert lib.fsdp_skidpad_submit_device(None, 4, 8, None, None, None, None, None, None, None, None, None, ctypes.byref(t)) == 1
        assert t.value == 7
    # the binding refuses host arrays by type, before it looks at the context
    batch = object.__new__(pkg.SkidpadBatch)
    with pytest.raises(TypeError, match="submit_device takes device arrays.*submit"):
        pkg.SkidpadBatch.submit_device(batch, np.zeros(4, np.int32), np.zeros((4, 8, 3)), np.zeros((4, 4)))
    with pytest.raises(TypeError, match="submit_device takes device arrays"):
        pkg.SkidpadBatch.submit_device(batch, [0, 0], None, None)
    with pytest.raises(ValueError, match="n_planners >= 1"):
        pkg.SkidpadDeviceFleet(0, 8)
    with pytest.raises(ValueError, match="cone_capacity >= 0"):
        pkg.SkidpadDeviceFleet(2, -1)
    # an array of records passes as_device_ptr by its item size, and only by it
    class Fake:
        def __init__(self, shape, typestr):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (0x1000, False), "version": 3, "strides": None}

    info = pkg.skidpad.INFO_DTYPE
    assert pkg.as_device_ptr(Fake((4,), "|V32"), (4,), info, writable=True) == 0x1000
    with pytest.raises(ValueError, match="dtype"):
        pkg.as_device_ptr(Fake((4,), "|V24"), (4,), info)
    with pytest.raises(ValueError, match="dtype"):
        pkg.as_device_ptr(Fake((4,), "|V8"), (4,), np.float64)
    if pkg._capi.load().fsdp_device_count() == 0:
        with pytest.raises(pkg.FsdpError, match="no HIP device"):
            pkg.SkidpadDeviceFleet(2, 8)
