"""Inputs and expectations of the tests of the sequence calls with per-frame global paths (tests/test_sequence_paths_cpu.py,
tests/test_sequence_paths_gpu.py), and the ctypes binding of seq_chain_table_kernel under the host SIMT emulator
(tests/emu/emu_sequence_table.cpp, built by tests/emu/sequence_table.mk).  TEST INFRASTRUCTURE.

The constructed recording: 6 planners x 8 steps, step-major, on the path table of tests/gpath_table_support.paths().

  (a) id -1 throughout; cones of tests/golden/sequence_chain.npz (planner 1, steps 0-7: a drop-out that reads the previous path)
  (b) TRACK throughout, the frames of tests/golden/global_path.npz
  (c) no cones; id -1 on steps 0-2, ACC from step 3 on: the acceleration pattern (plans from its previous path, then along the path)
  (d) ACC throughout; on steps 2-4 the car is 7 m beside the path (on the side away from its return lane), further than
      maximal_distance_for_valid_path = 5 m from the path update, so overwrite_if_too_far reads the previous path: a run of flagged
      frames that all carry a path
  (e) like (d), with the ZERO path (status 103, transparent) on step 3, in the middle of the run
  (f) steps 2-5 beside SHORT and TRACK in turn: a run whose frames name two different paths, so the lookup changes inside one
      wavefront's loop

Expected values never come from the code under test: every planner is stepped frame by frame on the oracle
(oracle_lib.plan_frame_global with its previous path, advanced only on status 0)."""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

import emu_lib
import gpath_table_support as gts
import oracle_lib
import sequence_support as ss

ROOT = Path(__file__).resolve().parent.parent
EMU_DIR = ROOT / "tests" / "emu"
GOLDEN = ROOT / "tests" / "golden"

N_PLANNERS, N_STEPS = 6, 8
A, B, C, D, E, F = range(6)  # the planners' rows


class Recording:
    def __init__(self):
        gp = np.load(GOLDEN / "global_path.npz")
        sc = np.load(GOLDEN / "sequence_chain.npz")
        self.paths = gts.paths()
        self.xy, self.path_off = gts.table(self.paths)
        n, T = N_PLANNERS, N_STEPS
        self.n, self.T = n, T
        ids = np.full((T, n), gts.CONES, np.int32)
        poses = np.zeros((T, n, 4))
        cones = [[np.zeros((0, 3))] * n for _ in range(T)]
        acc, track, short = self.paths[gts.ACC], self.paths[gts.TRACK], self.paths[gts.SHORT]
        sc_n = int(sc["n_planners"])
        for t in range(T):
            f = t * sc_n + 1  # (a): planner 1 of the fixture
            cones[t][A] = sc["cones"][sc["offsets"][f] : sc["offsets"][f + 1]]
            poses[t, A] = sc["poses"][f]
            ids[t, B] = gts.TRACK
            cones[t][B] = gp["gp_cones"][gp["gp_offsets"][t] : gp["gp_offsets"][t + 1]]
            poses[t, B] = gp["gp_poses"][t]
            ids[t, C] = gts.ACC if t >= 3 else gts.CONES
            poses[t, C] = [2.0 + 1.5 * t, 0.1, 1.0, 0.0]
            away = 2 <= t <= 4
            ids[t, D] = gts.ACC
            poses[t, D] = [5.0 + 2.0 * t, -7.0 if away else 0.2, 1.0, 0.0]
            ids[t, E] = gts.ZERO if t == 3 else gts.ACC
            poses[t, E] = [30.0 + 2.5 * t, -7.5 if away else -0.3, np.cos(0.03), np.sin(0.03)]
            # (f): on SHORT (steps 0, 1), beside SHORT and beside TRACK in turn (2-5), on SHORT again
            if t in (3, 5):
                k = 10 + 4 * t
                d = track[k + 1] - track[k]
                d = d / np.hypot(*d)
                ids[t, F] = gts.TRACK
                poses[t, F] = [*(track[k] + 7.0 * np.array([-d[1], d[0]])), *d]
            else:
                ids[t, F] = gts.SHORT
                poses[t, F] = [1.0 + 0.8 * t, 7.0 if t in (2, 4) else 0.3, 1.0, 0.0]
        self.ids = np.ascontiguousarray(ids.reshape(-1))
        self.poses = np.ascontiguousarray(poses.reshape(-1, 4))
        flat = [cones[t][p] for t in range(T) for p in range(n)]
        self.off = np.zeros(n * T + 1, np.int32)
        self.off[1:] = np.cumsum([len(c) for c in flat])
        self.cones = np.ascontiguousarray(np.concatenate(flat).reshape(-1, 3))
        self._stepped = {}

    def frame_cones(self, f):
        return self.cones[self.off[f] : self.off[f + 1]]

    def path_of(self, f, ids=None):
        i = int((self.ids if ids is None else ids)[f])
        return None if i < 0 else self.paths[i]

    def stepped(self, initial_prev=None, steps=None, ids=None, oracle=oracle_lib):
        """Every planner stepped on the oracle (math mode 1: the kernels' deterministic libm) -> (records step-major, final_prev
        (n, PATH_POINTS, 4) with NaN rows for planners without a path, re-plan count: flagged frames that met a real previous path,
        the frames' `real` flags).  initial_prev: (n, rows, 4), a row starting with NaN = none.  steps: the first so many.  oracle:
        oracle_lib, or oracle_lib_wide for the wide build's shapes."""
        key = (None if initial_prev is None else initial_prev.tobytes(), steps, None if ids is None else ids.tobytes(), oracle.__name__)
        if key in self._stepped:
            return self._stepped[key]
        n, T = self.n, self.T if steps is None else steps
        rows = oracle.default_path().shape[0]
        have = np.full((n, rows, 4), np.nan)
        if initial_prev is not None:
            have[:] = initial_prev
        out = np.zeros(n * T, oracle.RESULT_DTYPE)
        real = np.zeros(n * T, bool)
        with oracle.math_mode(1):
            for t in range(T):
                for p in range(n):
                    f = t * n + p
                    real[f] = not np.isnan(have[p, 0, 0])
                    out[f] = oracle.plan_frame_global(self.frame_cones(f), self.poses[f], have[p] if real[f] else None, self.path_of(f, ids))
                    if out[f]["status"] == 0:
                        have[p] = out[f]["path"]
        flagged = (out["path_fallback"] & ss.FB_READ_PREVIOUS) != 0
        self._stepped[key] = (out, have, int((flagged & real).sum()), real)
        return self._stepped[key]

    def constant(self):
        """every frame as a fresh planner plans it (the constant initial path): what the speculative pass computes"""
        if "constant" not in self._stepped:
            out = np.zeros(self.n * self.T, oracle_lib.RESULT_DTYPE)
            with oracle_lib.math_mode(1):
                for f in range(len(out)):
                    out[f] = oracle_lib.plan_frame_global(self.frame_cones(f), self.poses[f], None, self.path_of(f))
            self._stepped["constant"] = out
        return self._stepped["constant"]

    def preconditions(self):
        """What the recording must hold for the tests to prove anything, from the oracle alone -> dict of booleans"""
        ref, _final, again, real = self.stepped()
        const = self.constant()
        n, T = self.n, self.T
        flagged = ((ref["path_fallback"] & ss.FB_READ_PREVIOUS) != 0).reshape(T, n)
        with_id = (self.ids >= 0).reshape(T, n)
        run = any((flagged & with_id)[t, p] and (flagged & with_id)[t + 1, p] for t in range(T - 1) for p in range(n))
        differs = [f for f in range(n * T) if flagged.reshape(-1)[f] and (ref["status"][f] != const["status"][f] or
                                                                           ref["path"][f].tobytes() != const["path"][f].tobytes())]
        purpose = (self.ids == gts.ZERO) | (self.ids == gts.DENSE)
        return {
            "run of >= 2 flagged frames with ids": bool(run),
            "a flagged frame whose true previous path changes its result": len(differs) > 0,
            "a flagged frame with id -1": bool((flagged & ~with_id).any()),
            "re-plans expected": again > 0,
            "no 203 / 204 but on purpose": not np.isin(ref["status"][~purpose], (203, 204)).any(),
            "flags do not depend on the previous path": bool(np.array_equal(flagged.reshape(-1), (const["path_fallback"] & ss.FB_READ_PREVIOUS) != 0)),
            "the run of (f) names two paths": bool(all(flagged[t, F] for t in (2, 3, 4, 5))),
            "the run of (e) holds a transparent frame": bool(flagged[2, E] and flagged[4, E] and not flagged[3, E] and ref["status"][3 * n + E] == 103),
        }

    def slice_rows(self, lo, hi):
        """the recording's frames of planners [lo, hi), in recording order"""
        return np.concatenate([np.arange(t * self.n + lo, t * self.n + hi) for t in range(self.T)])


def check(ref, status, path, fallback=None, what="", rows=None):
    """status / path (/ fallback) of frames against the stepped oracle's, bit for bit; rows: the first so many path rows (the horizon
    of a build whose records hold more)"""
    assert np.array_equal(np.asarray(status, np.int64), ref["status"].astype(np.int64)), (what, np.asarray(status), ref["status"])
    if fallback is not None:
        assert np.array_equal(np.asarray(fallback, np.int64), ref["path_fallback"].astype(np.int64)), (what, np.asarray(fallback), ref["path_fallback"])
    for f in range(len(ref)):
        if ref["status"][f] == 0:
            assert np.asarray(path[f][:rows]).tobytes() == ref["path"][f][:rows].tobytes(), (what, f, np.nanmax(np.abs(path[f] - ref["path"][f])))
        else:
            assert np.isnan(path[f]).all(), (what, f)


# ---- the emulator -----------------------------------------------------------------------------------------------------------------
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-f", "sequence_table.mk", "-C", str(EMU_DIR)], check=True)
        _lib = ctypes.CDLL(str(EMU_DIR / "libfsdp_emu_sequence_table.so"))
        assert _lib.emu_sizeof_path_out() == emu_lib.PATH_DTYPE.itemsize and _lib.emu_sizeof_match_out() == emu_lib.MATCH_DTYPE.itemsize
    return _lib


def emu_plan_sequence(rec, ids=None, initial_prev=None, form="mono16", blocks=8, plain_path=-1, steps=None):
    """The kernels of a sequence pass with ids under the emulator: sort -> match (tests/emu_lib.py) -> the path stage of a pass with
    ids and no previous paths (form: gpath_table_support.FORMS) -> seq_mark -> seq_chain_table (plain_path >= 0: seq_chain_kernel
    with that entry as the launch's one pair) -> seq_final.  -> (status, path records, final_prev, frames planned again)"""
    n, T = rec.n, rec.T if steps is None else steps
    nf = n * T
    off, poses = rec.off[: nf + 1], np.ascontiguousarray(rec.poses[:nf])
    ids = np.ascontiguousarray((rec.ids if ids is None else ids)[:nf], np.int32)
    s = emu_lib.sort(off, rec.cones, poses)
    m = emu_lib.match(off, rec.cones, poses, s)
    out = np.zeros(nf, emu_lib.PATH_DTYPE)
    out["path"] = 7.0  # (what the kernels do not write would show)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    xy, path_off = np.ascontiguousarray(rec.xy), np.ascontiguousarray(rec.path_off, np.int32)
    L = lib()
    rc = L.emu_gpt_path(ctypes.c_int(gts.FORMS[form]), ctypes.c_int(nf), poses.ctypes.data_as(dp), ctypes.c_void_p(m.ctypes.data), None,
                        xy.ctypes.data_as(dp), path_off.ctypes.data_as(ip), ctypes.c_int(len(path_off) - 1), ids.ctypes.data_as(ip),
                        ctypes.c_void_p(out.ctypes.data))
    assert rc == 0
    init = None
    if initial_prev is not None:
        init = np.full((n, emu_lib.PATH_POINTS, 4), np.nan)
        init[:, : np.shape(initial_prev)[1]] = initial_prev
    final = np.zeros((n, emu_lib.PATH_POINTS, 4))
    again = L.emu_seqt_chain(ctypes.c_int(n), ctypes.c_int(T), poses.ctypes.data_as(dp), ctypes.c_void_p(m.ctypes.data),
                             None if init is None else init.ctypes.data_as(dp), xy.ctypes.data_as(dp), path_off.ctypes.data_as(ip),
                             ctypes.c_int(len(path_off) - 1), ids.ctypes.data_as(ip), ctypes.c_void_p(out.ctypes.data), final.ctypes.data_as(dp),
                             ctypes.c_int(blocks), ctypes.c_int(plain_path))
    status = np.where(out["status"] != 0, out["status"], np.where(m["status"] != 0, m["status"], s["status"]))
    return status, out, final, int(again)
