"""Fixture of the ranked sorting candidates (include/fsdp.h fsdp_sort_batch_ranked): the REFERENCE's sorted costs and
configurations per side (calc_scores_and_end_configurations, find_configs_and_scores.py:29-112) and the matrix of the seven
weighted cost columns of cost_configurations(..., return_individual_costs=True) (cost_function.py:283-302), rows in the
same order.

    python tests/golden/make_golden_ranked.py      (build container: needs the reference, refharness.py)

Frames: the eight demo scenarios of scenarios.npz (all 25 frames: three variants each and the notebook's frame), the first
24 frames of cfg2_color.npz, the first 8 of cfg3_nocolor.npz — and, because every replay frame among those has exactly one
configuration per side, five frames of lattice.npz (3 .. 61 configurations per side, exact cost ties) and three of
cfg4_noisy_nocolor.npz (200 cones: the 255-cone kernel) for sides with runners-up.  source[k], source_frame[k] name them; the
inputs are stored again so that the file stands alone.  Writes
tests/golden/sort_ranked.npz: per frame k and side s (0 = left, 1 = right) the rows [row_off[k, s], row_off[k, s] + n_rows[k, s])
of costs (R,), configs (R, 12; -1 padded) and terms (R, 7).  A side the reference returns None for, or a frame it raises on
(exc[k] != "ok"), has no rows.  Indices are in the caller's index space (the frame's flattened cones).

costs / terms are the reference with NumPy's default CPU dispatch (as every golden here); costs_libm / terms_libm the same run
at the libm level of the dispatch (arc_libm_golden.py), where NumPy's arctan2 / arccos are the host libm's: the values the
emulated kernels, which call the same libm, reproduce bit for bit.  The two levels differ in a last bit of columns 0, 3 and 6 on
a third of the rows.  knn_tie[k]: refharness.knn_boundary_tie — the reference's adjacency on such a frame is its unstable
argsort's, and with it the set of configurations (tests/parity.py skips the configuration counts there as well).
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))

import refharness  # noqa: E402

MAX_LEN = 12
SOURCES = (("scenarios", range(25)), ("cfg2_color", range(24)), ("cfg3_nocolor", range(8)), ("lattice", (0, 1, 2, 3, 13)), ("cfg4_noisy_nocolor", (0, 2, 5)))
SIZE_CAP = 256 * 1024


def capture_frame(m, xyt, pose):
    """-> (exception name or "ok", [per side: (costs (C,), configs (C, L), terms (C, 7)) or None])"""
    import fsd_path_planning.sorting_cones.trace_sorter.find_configs_and_scores as fcs

    orig = fcs.cost_configurations
    seen = []

    def wrapper(points, configurations, cone_type, vehicle_position, vehicle_direction, *, return_individual_costs):
        ind = orig(points, configurations, cone_type, vehicle_position, vehicle_direction, return_individual_costs=True)
        if len(configurations):
            seen.append((int(cone_type), np.array(configurations), np.array(ind)))
            return ind.sum(axis=-1)  # (cost_function.py:304: what the call returns without the flag)
        return ind

    fcs.cost_configurations = wrapper
    try:
        r = refharness.run_frame(xyt, pose)
    finally:
        fcs.cost_configurations = orig
    sides = [None, None]
    for s, (t, name) in enumerate(((2, "left"), (1, "right"))):
        costs, configs = r.get(f"{name}_costs"), r.get(f"{name}_configs")
        if costs is None or configs is None or len(costs) == 0:
            continue
        (rec,) = [x for x in seen if x[0] == t]
        _, raw_cfg, ind = rec
        order = np.argsort(ind.sum(axis=-1))  # (find_configs_and_scores.py:108, the same call on the same values)
        assert np.array_equal(raw_cfg[order], configs) and np.array_equal(ind.sum(axis=-1)[order], costs)
        sides[s] = (np.asarray(costs, np.float64), np.asarray(configs, np.int64), np.asarray(ind[order], np.float64))
    return r["status"], sides


LIBM_LEVEL = "AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX2 FMA3"  # (arc_libm_golden.py: NumPy calls libm)


def capture_all():
    m = refharness.load()
    out = {k: [] for k in ("source", "source_frame", "cones", "poses", "exc", "knn_tie", "n_rows", "costs", "configs", "terms")}
    for name, frames in SOURCES:
        g = np.load(HERE / f"{name}.npz")
        for k in frames:
            xyt = np.ascontiguousarray(g["cones"][g["offsets"][k] : g["offsets"][k + 1]], dtype=np.float64)
            pose = np.ascontiguousarray(g["poses"][k], dtype=np.float64)
            exc, sides = capture_frame(m, xyt, pose)
            n_rows = [0, 0]
            for s, side in enumerate(sides):
                if side is None or exc != "ok":
                    continue
                costs, configs, terms = side
                pad = np.full((len(costs), MAX_LEN), -1, np.int16)
                pad[:, : configs.shape[1]] = configs
                n_rows[s] = len(costs)
                out["costs"].append(costs)
                out["configs"].append(pad)
                out["terms"].append(terms)
            for key, v in (("source", name), ("source_frame", k), ("cones", xyt), ("poses", pose), ("exc", exc), ("n_rows", n_rows),
                           ("knn_tie", refharness.knn_boundary_tie(xyt))):
                out[key].append(v)
    n_rows = np.array(out["n_rows"], np.int32)
    row_off = np.concatenate([[0], np.cumsum(n_rows.ravel())])[:-1].reshape(-1, 2).astype(np.int32)
    offsets = np.zeros(len(out["cones"]) + 1, np.int32)
    offsets[1:] = np.cumsum([len(c) for c in out["cones"]])
    return dict(source=np.array(out["source"]), source_frame=np.array(out["source_frame"], np.int32), offsets=offsets,
                cones=np.concatenate(out["cones"]), poses=np.array(out["poses"]), exc=np.array(out["exc"]), knn_tie=np.array(out["knn_tie"]),
                n_rows=n_rows, row_off=row_off, costs=np.concatenate(out["costs"]), configs=np.concatenate(out["configs"]),
                terms=np.concatenate(out["terms"]))


def main():
    import os
    import subprocess
    import tempfile

    if os.environ.get("RANKED_CHILD"):
        np.savez(os.environ["RANKED_CHILD"], **capture_all())
        return
    # two captures of the same reference run, one child process per level of NumPy's CPU dispatch (it is fixed at import): the
    # default one (AVX-512 here: NumPy's own arctan2 / arccos) and the libm level, where NumPy calls the libm the oracle and the
    # emulated kernels call — the level at which host results can equal the reference bit for bit (arc_libm_golden.py)
    caps = {}
    with tempfile.TemporaryDirectory() as tmp:
        for level, dis in (("default", None), ("libm", LIBM_LEVEL)):
            env = dict(os.environ, RANKED_CHILD=str(Path(tmp) / f"{level}.npz"))
            if dis:
                env["NPY_DISABLE_CPU_FEATURES"] = dis
            subprocess.run([sys.executable, str(Path(__file__).resolve())], env=env, check=True)
            caps[level] = dict(np.load(env["RANKED_CHILD"]))
    res, lm = caps["default"], caps["libm"]
    for k in res:
        if k not in ("costs", "terms"):
            assert np.array_equal(res[k], lm[k]), k  # the same rows in the same order at both levels
    res["costs_libm"], res["terms_libm"] = lm["costs"], lm["terms"]
    res["libm_level"] = np.array("NPY_DISABLE_CPU_FEATURES=" + LIBM_LEVEL)
    n_rows = res["n_rows"]
    f = HERE / "sort_ranked.npz"
    np.savez_compressed(f, **res)
    size = f.stat().st_size
    rel = np.abs(res["terms"] - lm["terms"]) / np.maximum(1.0, np.abs(lm["terms"]))
    print(f"{f.name}: {len(n_rows)} frames, {len(res['costs'])} rows, at most {n_rows.max()} per side, {int((n_rows > 1).sum())} sides with a runner-up, "
          f"{int(res['knn_tie'].sum())} frames with a nearest-neighbour tie, {size} bytes; exceptions: {sorted(set(res['exc'].tolist()))}")
    print(f"default dispatch vs libm level: terms differ in any bit on {int((rel > 0).any(axis=1).sum())} rows (columns {np.flatnonzero((rel > 0).any(axis=0)).tolist()}), "
          f"at most {rel.max():.3g} relative; costs on {int((res['costs'] != lm['costs']).sum())} rows")
    assert size < SIZE_CAP, size  # (larger: drop cfg2_color frames from the end)
    assert (res["terms"][:, 4] == 0).all() and int((n_rows > 1).sum()) >= 8


if __name__ == "__main__":
    main()
