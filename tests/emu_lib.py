"""ctypes binding of the host-SIMT-emulated kernels (tests/emu/libfsdp_emu.so).
TEST INFRASTRUCTURE: executes the kernel sources of ft-fsd-path-planning_amd/csrc on the CPU
(one fiber per lane) so their logic can be compared with the oracle without a GPU."""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
EMU_DIR = ROOT / "tests" / "emu"
# tests/emu_lib_wide.py runs this file a second time as its own module with WIDE_SHAPES preset: the kernel sources compiled
# with -DFSDP_WIDE_SHAPES (tests/emu/Makefile libfsdp_emu_wide.so), compared with oracle_lib_wide
WIDE_SHAPES = bool(globals().get("WIDE_SHAPES", False))
LIB = EMU_DIR / ("libfsdp_emu_wide.so" if WIDE_SHAPES else "libfsdp_emu.so")

MAX_LEN, MAX_MATCH, PATH_POINTS = (16, 32, 64) if WIDE_SHAPES else (12, 24, 40)

SORT_DTYPE = np.dtype(
    [
        ("status", "<i4"), ("n_left", "<i4"), ("n_right", "<i4"),
        ("left_idx", "<i4", (MAX_LEN,)), ("right_idx", "<i4", (MAX_LEN,)),
        ("n_configs_left", "<i4"), ("n_configs_right", "<i4"),
        ("first_k_left", "<i4", (2,)), ("first_k_right", "<i4", (2,)),
        ("best_cost_left", "<f8"), ("best_cost_right", "<f8"),
    ],
    align=True,
)
MATCH_DTYPE = np.dtype(
    [
        ("status", "<i4"), ("n_left_v", "<i4"), ("n_right_v", "<i4"), ("pad", "<i4"),
        ("left_v", "<f8", (MAX_MATCH, 2)), ("right_v", "<f8", (MAX_MATCH, 2)),
        ("l2r", "<i4", (MAX_MATCH,)), ("r2l", "<i4", (MAX_MATCH,)),
    ],
    align=True,
)
PATH_DTYPE = np.dtype(
    [("path", "<f8", (PATH_POINTS, 4)), ("status", "<i4"), ("fallback", "<i4"), ("n_dense", "<i4"), ("pad", "<i4")],
    align=True,
)

_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", str(EMU_DIR)], check=True)
        _lib = ctypes.CDLL(str(LIB))
        assert _lib.emu_sizeof_sort_out() == SORT_DTYPE.itemsize
    return _lib


def _p(a, t=ctypes.c_double):
    return a.ctypes.data_as(ctypes.POINTER(t))


def sort(offsets, cones, poses):
    offsets = np.ascontiguousarray(offsets, np.int32)
    cones = np.ascontiguousarray(cones, np.float64)
    poses = np.ascontiguousarray(poses, np.float64)
    n = len(offsets) - 1
    out = np.zeros(n, SORT_DTYPE)
    lib().emu_sort(ctypes.c_int(n), _p(offsets, ctypes.c_int32), _p(cones), _p(poses), ctypes.c_void_p(out.ctypes.data))
    return out


def sort_cached(offsets, cones, poses):
    """The sorting kernels' cache-enabled instantiation (sort_kernel_128_cached / sort_kernel_cached / sort_big_kernel_cached), one
    planner per frame with an empty entry: every side is searched by that instantiation's own code -> (sort records, hits (n, 2))"""
    offsets = np.ascontiguousarray(offsets, np.int32)
    cones = np.ascontiguousarray(cones, np.float64)
    poses = np.ascontiguousarray(poses, np.float64)
    n = len(offsets) - 1
    out = np.zeros(n, SORT_DTYPE)
    hits = np.full((n, 2), -1, np.int8)
    lib().emu_sort_cached(ctypes.c_int(n), _p(offsets, ctypes.c_int32), _p(cones), _p(poses), ctypes.c_void_p(out.ctypes.data),
                          ctypes.c_void_p(hits.ctypes.data))
    return out, hits


RANK_MAX, COST_TERMS = 64, 7


def last_kernels():
    """bit 0 / 1 / 2: sort_kernel_128_ranked / sort_kernel_ranked / sort_big_kernel_ranked ran in the last sort_ranked call"""
    return int(lib().emu_ranked_last_kernels())


def sort_ranked(offsets, cones, poses, top_k=8, terms=True):
    """The ranked sorting kernels, wrapped like the library's fsdp_sort_batch_ranked (tests/emu/emu_ranked.cpp) -> (sort records,
    counts (n,2), configs (n,2,top_k,MAX_LEN), costs (n,2,top_k), terms (n,2,top_k,7) or None); raises ValueError for a top_k
    the kernels refuse"""
    offsets = np.ascontiguousarray(offsets, np.int32)
    cones = np.ascontiguousarray(cones, np.float64)
    poses = np.ascontiguousarray(poses, np.float64)
    n = len(offsets) - 1
    k = max(1, min(int(top_k), RANK_MAX))
    out = np.zeros(n, SORT_DTYPE)
    counts = np.zeros((n, 2), np.int32)
    configs = np.zeros((n, 2, k, MAX_LEN), np.int32)
    costs = np.zeros((n, 2, k))
    tm = np.zeros((n, 2, k, COST_TERMS)) if terms else None
    rc = lib().emu_sort_ranked(ctypes.c_int(n), _p(offsets, ctypes.c_int32), _p(cones), _p(poses), ctypes.c_void_p(out.ctypes.data),
                               ctypes.c_int(int(top_k)), _p(counts, ctypes.c_int32), _p(configs, ctypes.c_int32), _p(costs),
                               _p(tm) if terms else None)
    if rc != 0:
        raise ValueError(f"top_k = {top_k} refused")
    return out, counts, configs, costs, tm


def match(offsets, cones, poses, sorted_out):
    offsets = np.ascontiguousarray(offsets, np.int32)
    cones = np.ascontiguousarray(cones, np.float64)
    poses = np.ascontiguousarray(poses, np.float64)
    n = len(offsets) - 1
    assert lib().emu_sizeof_match_out() == MATCH_DTYPE.itemsize
    out = np.zeros(n, MATCH_DTYPE)
    lib().emu_match(ctypes.c_int(n), _p(offsets, ctypes.c_int32), _p(cones), _p(poses),
                    ctypes.c_void_p(sorted_out.ctypes.data), ctypes.c_void_p(out.ctypes.data))
    return out


# lanes per frame of the one-kernel path stage (8 / 16 / 64), and the three-kernel path stage the library launches for
# large batches with 4 or 8 lanes per frame in its fit kernel (1004 / 1008)
PATH_GROUP_SIZES = (8, 16, 64, 1004, 1008, 1016, 2008)  # 2008: the wide (32-knot) three kernels


def last_retries():
    """Frames the last split-pipeline launch handed to the exact re-plan kernel."""
    return int(lib().emu_last_retries())


def path(poses, matched, group=8, prev_paths=None, global_path=None):
    """prev_paths (n, PATH_POINTS, 4): every frame's previous path; global_path (m, 2): the context's.  None leaves what the caller set
    with emu_set_prev_paths / emu_set_global_path as it is (nothing set: fresh planners, no global path)."""
    poses = np.ascontiguousarray(poses, np.float64)
    n = len(poses)
    assert lib().emu_sizeof_path_out() == PATH_DTYPE.itemsize
    out = np.zeros(n, PATH_DTYPE)
    prev = None if prev_paths is None else np.ascontiguousarray(prev_paths, np.float64)
    assert prev is None or prev.shape == (n, PATH_POINTS, 4)
    gp = None if global_path is None else np.ascontiguousarray(global_path, np.float64).reshape(-1, 2)
    if prev is not None:
        lib().emu_set_prev_paths(_p(prev))
    if gp is not None:
        lib().emu_set_global_path(_p(gp), ctypes.c_int(len(gp)))
    try:
        rc = lib().emu_path_g(ctypes.c_int(group), ctypes.c_int(n), _p(poses), ctypes.c_void_p(matched.ctypes.data),
                              ctypes.c_void_p(out.ctypes.data))
    finally:  # (only what this call set: a caller that set the emulator's previous or global path itself keeps it across calls)
        if prev is not None:
            lib().emu_set_prev_paths(None)
        if gp is not None:
            lib().emu_set_global_path(None, ctypes.c_int(0))
    assert rc == 0, f"no path kernel for group size {group}"
    return out


FIT_TEST_KNOTS = 64  # knot_capacity<64>() of csrc/spline_device.h: knots fit_test_kernel's workspace keeps (status 204 beyond)


def fit(trace, smoothing):
    """fit_polyline<64> on one polyline (emu_fit / fit_test_kernel) -> (rc, k, n, knots (n,), cx (n,), cy (n,), ier, fp, max_u); rc 1
    where splprep raises, 204 where the fit needs more than FIT_TEST_KNOTS knots.  Degree min(len - 1, 3)."""
    trace = np.ascontiguousarray(trace, np.float64).reshape(-1, 2)
    t, c = np.zeros(FIT_TEST_KNOTS), np.zeros(2 * FIT_TEST_KNOTS)
    info, fp = np.zeros(4, np.int32), np.zeros(2)
    lib().emu_fit(_p(trace), ctypes.c_int(len(trace)), ctypes.c_double(smoothing), _p(t), _p(c), _p(info, ctypes.c_int32), _p(fp))
    rc, n, ier, k = (int(v) for v in info)
    n = min(max(n, 0), FIT_TEST_KNOTS)
    return rc, k, n, t[:n].copy(), c[:n].copy(), c[FIT_TEST_KNOTS : FIT_TEST_KNOTS + n].copy(), ier, float(fp[0]), float(fp[1])


def default_path():
    out = np.zeros((PATH_POINTS, 4))
    lib().emu_default_path(_p(out))
    return out


def plan(offsets, cones, poses, group=8):
    """Full emulated pipeline; returns a structured array shaped like oracle_lib.RESULT_DTYPE.  group = lanes per frame
    of the path kernel (8: eight frames per wavefront, 16, or 64: one frame per wavefront)."""
    s = sort(offsets, cones, poses)
    m = match(offsets, cones, poses, s)
    lib().emu_sort_remap(ctypes.c_int(len(s)), ctypes.c_void_p(s.ctypes.data))  # (use_unknown_cones = False: indices back to the caller's array)
    p = path(poses, m, group)
    return records(s, m, p), p["n_dense"]


def records(s, m, p):
    """The sort, match and path records of the same frames as one structured array shaped like oracle_lib.RESULT_DTYPE."""
    if WIDE_SHAPES:
        import oracle_lib_wide as oracle_lib
    else:
        import oracle_lib

    res = np.zeros(len(s), oracle_lib.RESULT_DTYPE)
    for k in ("n_left", "n_right", "left_idx", "right_idx", "n_configs_left", "n_configs_right", "first_k_left",
              "first_k_right", "best_cost_left", "best_cost_right"):
        res[k] = s[k]
    for k in ("n_left_v", "n_right_v", "left_v", "right_v", "l2r", "r2l"):
        res[k] = m[k]
    res["path"] = p["path"]
    res["path_fallback"] = p["fallback"]
    st = s["status"].copy()
    st = np.where(m["status"] != 0, m["status"], st)
    st = np.where(p["status"] != 0, p["status"], st)
    res["status"] = st
    return res


# ---- the kernels of fsdp_plan_sequence[_cached] (tests/emu/emu_sequence.cpp, emu_sequence_cache.cpp); frames step-major ----
def sequence_mark(n_planners, status, fallback):
    """seq_mark_kernel over injected status / fallback words -> sorted list of (head frame, predecessor frame or -1)"""
    status = np.ascontiguousarray(status, np.int32)
    fallback = np.ascontiguousarray(fallback, np.int32)
    n = len(status)
    heads = np.zeros(2 * n + 2, np.int32)
    k = lib().emu_sequence_mark(ctypes.c_int(n_planners), ctypes.c_int(n // n_planners), _p(status, ctypes.c_int32), _p(fallback, ctypes.c_int32),
                                _p(heads, ctypes.c_int32))
    return sorted((int(heads[2 * j]), int(heads[2 * j + 1])) for j in range(k))


def sequence_chain(n_planners, poses, matched, paths, initial_prev=None, blocks=8):
    """seq_mark -> seq_chain (grid `blocks`) -> seq_final over `paths`, the path records of a pass planned without previous paths,
    resolved in place; initial_prev: (n_planners, <= PATH_POINTS, 4) or None -> (final_prev, frames planned again)"""
    poses = np.ascontiguousarray(poses, np.float64)
    init = None
    if initial_prev is not None:
        init = np.full((n_planners, PATH_POINTS, 4), np.nan)
        init[:, : np.shape(initial_prev)[1]] = initial_prev
    final = np.zeros((n_planners, PATH_POINTS, 4))
    again = lib().emu_sequence_chain(ctypes.c_int(n_planners), ctypes.c_int(len(poses) // n_planners), _p(poses), ctypes.c_void_p(matched.ctypes.data),
                                     None if init is None else _p(init), ctypes.c_void_p(paths.ctypes.data), _p(final), ctypes.c_int(blocks))
    return final, int(again)


def sequence_cache(n_planners, offsets, cones, poses):
    """speculative sort -> [big] -> seq_cache_mark -> seq_cache_resolve, planners with empty entries ->
    (SortOut records, hits (frames, 2), n_resorted, kernels bit mask, frames of the big route)"""
    offsets = np.ascontiguousarray(offsets, np.int32)
    cones = np.ascontiguousarray(cones, np.float64)
    poses = np.ascontiguousarray(poses, np.float64)
    n = len(poses)
    out = np.zeros(n, SORT_DTYPE)
    hits = np.zeros((n, 2), np.int8)
    resorted, kernels = ctypes.c_longlong(-1), ctypes.c_int(0)
    big = lib().emu_sequence_cache(ctypes.c_int(n_planners), ctypes.c_int(n // n_planners), _p(offsets, ctypes.c_int32), _p(cones), _p(poses),
                                   ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(hits.ctypes.data), ctypes.byref(resorted), ctypes.byref(kernels))
    return out, hits, int(resorted.value), int(kernels.value), int(big)


SKID_STATE_DTYPE = np.dtype(
    [("has_original", "<i4"), ("relocalized", "<i4"), ("index_along_path", "<i4"), ("reloc_step", "<i4"), ("index_hist", "<i4", (32,)),
     ("orig", "<f8", (4,)),
     ("translation", "<f8", (2,)), ("right_calc", "<f8", (2,)), ("rotation", "<f8"), ("prev", "<f8", (PATH_POINTS, 4))],
    align=True,
)
SKID_INFO_DTYPE = np.dtype([("relocalized", "<i4"), ("index_along_path", "<i4"), ("translation", "<f8", (2,)), ("rotation", "<f8")], align=True)


def skidpad_constants(table):
    """(reference centres (2,2) [right, left], table spacing) from csrc/skidpad_kernel.h skid_centers_kernel."""
    table = np.ascontiguousarray(table, np.float64)
    out = np.zeros(5)
    lib().emu_skidpad_constants(_p(table), ctypes.c_int(len(table)), _p(out))
    return out[:4].reshape(2, 2).copy(), float(out[4])


class SkidpadEmu:
    """The skidpad kernels under the emulator: n planner instances, stateful."""

    def __init__(self, n, table, noise, ref, mean_distance):
        assert lib().emu_sizeof_skid_state() == SKID_STATE_DTYPE.itemsize and lib().emu_sizeof_skid_info() == SKID_INFO_DTYPE.itemsize
        self.n = n
        self.half = np.ascontiguousarray(table[::2], np.float64)
        self.noise = np.ascontiguousarray(noise, np.float64).ravel()
        self.ref = np.ascontiguousarray(ref, np.float64).ravel()
        self.md = float(mean_distance)
        self.states = np.zeros(n, SKID_STATE_DTYPE)
        self.states["prev"] = default_path()
        self.sync = np.zeros(n + 1, np.uint32)  # ticket counter + steps published per instance
        self.ticket_base = np.zeros(1, np.uint32)
        self.step_no = 0

    def step(self, offsets, cones, poses):
        (res,) = self.steps([(offsets, cones, poses)])
        return res

    def steps_packed(self, frames, lanes=16):
        """The same as ``steps`` through the packed kernels (select -> prep -> fit -> finish -> commit, lanes per frame 16
        or 8 with a 4-lane fit) -> ([(out, info), ...], number of steps the planners' own wavefronts had to plan)."""
        k = len(frames)
        offs = [np.ascontiguousarray(f[0], np.int32) for f in frames]
        cones = [np.ascontiguousarray(f[1], np.float64).reshape(-1, 3) for f in frames]
        poses = [np.ascontiguousarray(f[2], np.float64) for f in frames]
        outs = [np.zeros(self.n, PATH_DTYPE) for _ in range(k)]
        infos = [np.zeros(self.n, SKID_INFO_DTYPE) for _ in range(k)]
        ptrs = lambda arrs: (ctypes.c_void_p * k)(*[a.ctypes.data for a in arrs])
        serial = lib().emu_skidpad_steps_packed(
            ctypes.c_int(lanes), ctypes.c_int(self.n), ctypes.c_int(k), ctypes.c_int(self.step_no), ptrs(offs), ptrs(cones), ptrs(poses),
            ctypes.c_void_p(self.states.ctypes.data), _p(self.half), ctypes.c_int(len(self.half)), _p(self.noise),
            ctypes.c_int(len(self.noise)), _p(self.ref), ctypes.c_double(self.md), ptrs(outs), ptrs(infos),
            ctypes.c_void_p(self.sync.ctypes.data))
        self.step_no += k
        return list(zip(outs, infos)), int(serial)

    def steps(self, frames):
        """len(frames) <= 16 consecutive steps [(offsets, cones, poses), ...] in one skid_path_kernel launch (one wavefront
        per (instance, step): csrc/skidpad_kernel.h "Steps in flight") -> [(out, info), ...]."""
        k = len(frames)
        offs = [np.ascontiguousarray(f[0], np.int32) for f in frames]
        cones = [np.ascontiguousarray(f[1], np.float64).reshape(-1, 3) for f in frames]
        poses = [np.ascontiguousarray(f[2], np.float64) for f in frames]
        outs = [np.zeros(self.n, PATH_DTYPE) for _ in range(k)]
        infos = [np.zeros(self.n, SKID_INFO_DTYPE) for _ in range(k)]
        ptrs = lambda arrs: (ctypes.c_void_p * k)(*[a.ctypes.data for a in arrs])
        lib().emu_skidpad_steps(
            ctypes.c_int(self.n), ctypes.c_int(k), ctypes.c_int(self.step_no), ptrs(offs), ptrs(cones), ptrs(poses),
            ctypes.c_void_p(self.states.ctypes.data), _p(self.half), ctypes.c_int(len(self.half)), _p(self.noise),
            ctypes.c_int(len(self.noise)), _p(self.ref), ctypes.c_double(self.md), ptrs(outs), ptrs(infos),
            ctypes.c_void_p(self.sync.ctypes.data), ctypes.c_void_p(self.ticket_base.ctypes.data))
        self.step_no += k
        return list(zip(outs, infos))


class params:
    """with emu_lib.params(dict(max_dist=5.5)): ... — the kernel sources with non-default configuration constants."""

    def __init__(self, overrides):
        import oracle_lib

        self.v = oracle_lib.param_vector(overrides)
        self.d = oracle_lib.param_vector(None)

    def __enter__(self):
        lib().emu_set_params(_p(self.v))

    def __exit__(self, *a):
        lib().emu_set_params(_p(self.d))
