"""Generate the golden fixtures under tests/golden/ by RUNNING THE REFERENCE
(/root/reference imported read-only; identity-jit numba stub in _refstubs/).

Build-container only (the reference does not exist on the GPU box).  What is committed are
the .npz data files: inputs (frames) and the reference's outputs for them.  No reference
source is stored.  Re-run:  python tests/golden/make_golden.py

Fixture layout (all frame sets share it; arrays are padded, lengths given explicitly):
  offsets (F+1,) i4, cones (total,3) f8 [x,y,type], poses (F,4) f8 [px,py,dx,dy]
  ok (F,) bool            reference returned normally (False: it raised, `exc` holds the class name)
  n_left/n_right (F,) i4, left_idx/right_idx (F,12) i4   = left_config/right_config of
                          trace_sorter/core_trace_sorter.py:197-214 (the bit-exact parity target)
  n_left_v/n_right_v (F,) i4, left_v/right_v (F,24,2) f8, l2r/r2l (F,24) i4   (matching outputs)
  path (F,40,4) f8        [u, x, y, curvature]
"""
from __future__ import annotations

import importlib
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(HERE))

import refharness  # noqa: E402

synth = importlib.import_module("ft-fsd-path-planning_amd.synth")

MAX_LEN, MAX_MATCH = 12, 24


def capture(offsets, cones, poses, frames=None, params=None, flattened=True, shapes=None):
    """shapes = (max_len, max_match, path_points) of the padded arrays (default: the standard build's 12 / 24 / 40; the wide
    parameter sets store 16 / 32 / 64).
    flattened=False: the frame goes to the reference as the five per-type lists (its cones must be stored in type order, so
    that the reference's flattened index space is the stored one); with use_unknown_cones=False the reference's indices then
    count from the first known cone and are shifted by the frame's number of UNKNOWN cones into the stored index space."""
    if frames is None:
        frames = range(len(offsets) - 1)
    frames = list(frames)
    F = len(frames)
    MAX_LEN, MAX_MATCH, PATH_ROWS = shapes or (12, 24, 40)
    out = dict(
        ok=np.zeros(F, bool),
        exc=np.array([""] * F, dtype="U24"),
        n_left=np.zeros(F, np.int32),
        n_right=np.zeros(F, np.int32),
        left_idx=np.full((F, MAX_LEN), -1, np.int32),
        right_idx=np.full((F, MAX_LEN), -1, np.int32),
        n_left_v=np.zeros(F, np.int32),
        n_right_v=np.zeros(F, np.int32),
        left_v=np.zeros((F, MAX_MATCH, 2)),
        right_v=np.zeros((F, MAX_MATCH, 2)),
        l2r=np.full((F, MAX_MATCH), -1, np.int32),
        r2l=np.full((F, MAX_MATCH), -1, np.int32),
        path=np.full((F, PATH_ROWS, 4), np.nan),
        # per-stage intermediates: start cones per side (select_first_k_starting_cones), number of end
        # configurations per side after the post-filters and the cost of the best one (cost_configurations)
        first_k_left=np.full((F, 2), -1, np.int32),
        first_k_right=np.full((F, 2), -1, np.int32),
        first_k_tie=np.zeros((F, 2), bool),  # [left, right]: exact distance tie of the closest start candidates (unstable argsort)
        knn_tie=np.zeros(F, bool),  # exact tie among a cone's nearest neighbours (unstable argsort decides the adjacency)
        n_configs_left=np.zeros(F, np.int32),
        n_configs_right=np.zeros(F, np.int32),
        best_cost_left=np.zeros(F),
        best_cost_right=np.zeros(F),
        # the smoothing splines the frame fitted (scipy splprep inside the call), in call order, up to 6: degree, number
        # of knots, knots, x / y coefficients (padded to 48)
        n_fits=np.zeros(F, np.int32),
        fit_k=np.zeros((F, 6), np.int32),
        fit_n=np.zeros((F, 6), np.int32),
        fit_t=np.zeros((F, 6, 48)),
        fit_cx=np.zeros((F, 6, 48)),
        fit_cy=np.zeros((F, 6, 48)),
    )
    sub_cones, sub_off = [], [0]
    for k, f in enumerate(frames):
        xyt = cones[offsets[f] : offsets[f + 1]]
        sub_cones.append(xyt)
        sub_off.append(sub_off[-1] + len(xyt))
        r = refharness.run_frame(xyt, poses[f], params=params, flattened=flattened)
        shift = int((xyt[:, 2] == 0).sum()) if (not flattened and params and params.get("use_unknown_cones") is False) else 0
        if not flattened:
            assert np.all(np.diff(xyt[:, 2]) >= 0), "cones must be stored in type order"
        for side, t in (("left", 2), ("right", 1)):
            out["first_k_tie"][k, 0 if side == "left" else 1] = bool((r.get("first_k_tie") or {}).get(t, False))
            fk = (r.get("first_k") or {}).get(t)
            if fk is not None:
                out[f"first_k_{side}"][k, : len(fk)] = np.asarray(fk) + shift
            costs = r.get(f"{side}_costs")
            if costs is not None and len(costs):
                out[f"n_configs_{side}"][k] = len(costs)
                out[f"best_cost_{side}"][k] = costs[0]
        out["knn_tie"][k] = refharness.knn_boundary_tie(xyt)
        fits = r.get("fits") or []
        out["n_fits"][k] = len(fits)
        for q, (kk, t, cx, cy) in enumerate(fits[:6]):
            nn = min(len(t), 48)
            out["fit_k"][k, q], out["fit_n"][k, q] = kk, len(t)
            out["fit_t"][k, q, :nn] = t[:nn]
            out["fit_cx"][k, q, : min(len(cx), 48)] = cx[:48]
            out["fit_cy"][k, q, : min(len(cy), 48)] = cy[:48]
        if r["status"] != "ok":
            out["exc"][k] = r["status"]
            continue
        out["ok"][k] = True
        lc, rc = r["left_config"], r["right_config"]
        out["n_left"][k], out["n_right"][k] = len(lc), len(rc)
        out["left_idx"][k, : len(lc)] = lc + shift
        out["right_idx"][k, : len(rc)] = rc + shift
        lv, rv = r["left_v"], r["right_v"]
        assert len(lv) <= MAX_MATCH and len(rv) <= MAX_MATCH
        out["n_left_v"][k], out["n_right_v"][k] = len(lv), len(rv)
        out["left_v"][k, : len(lv)] = lv
        out["right_v"][k, : len(rv)] = rv
        out["l2r"][k, : len(lv)] = r["l2r"]
        out["r2l"][k, : len(rv)] = r["r2l"]
        out["path"][k, : len(r["path"])] = r["path"]  # (mpc_prediction_horizon rows; the rest stays NaN)
    out["offsets"] = np.array(sub_off, np.int32)
    out["cones"] = np.concatenate(sub_cones).reshape(-1, 3) if sub_cones else np.zeros((0, 3))
    out["poses"] = np.ascontiguousarray(poses[frames])
    return out


def scenario_frames():
    """The reference's 8 hard-coded demo scenarios, +/- its deterministic shuffle
    (demo/streamlit_demo/common.py:72-324), plus the notebook variant (Simple Corner with
    4 coloured cones, rest unknown) and a no-colour variant of each."""
    import matplotlib

    matplotlib.use("Agg")
    refharness.load()
    from fsd_path_planning.demo.streamlit_demo.common import get_cones_for_configuration

    frames, names = [], []
    for name in ["Straight", "Simple Corner", "Corner Missing Blue", "Corner Missing Blue Alt", "Hairpin",
                 "Hairpin Extreme", "Wrong sort", "Skidpad"]:
        for sh in (False, True):
            pos, d, cones = get_cones_for_configuration(name, sh)
            xyt = np.concatenate([np.column_stack([np.asarray(c, float).reshape(-1, 2), np.full(len(c), float(t))])
                                  for t, c in enumerate(cones)])
            frames.append((xyt, np.concatenate([pos, d])))
            names.append(f"{name}|shuffle={sh}")
            if not sh:
                nc = xyt.copy()
                nc[:, 2] = 0.0
                frames.append((nc, np.concatenate([pos, d])))
                names.append(f"{name}|nocolor")
    # notebook scenario (demo/simple_application.ipynb cells 3-15): 2 coloured per side
    pos, d, cones = get_cones_for_configuration("Simple Corner", False)
    left, right = np.asarray(cones[2]), np.asarray(cones[1])
    unknown = np.concatenate([left[2:], right[2:]])
    xyt = np.concatenate([np.column_stack([unknown, np.zeros(len(unknown))]),
                          np.column_stack([right[:2], np.ones(2)]), np.column_stack([left[:2], np.full(2, 2.0)])])
    frames.append((xyt, np.concatenate([pos, d])))
    names.append("notebook")
    off = np.concatenate([[0], np.cumsum([len(f[0]) for f in frames])]).astype(np.int32)
    return off, np.concatenate([f[0] for f in frames]), np.array([f[1] for f in frames]), names


def fuzz_frames(seed, n):
    """Small irregular frames around the origin (so the previous-path fallbacks are
    exercised the way the reference's demo scenarios exercise them) + noisy loop frames."""
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(n):
        kind = rng.integers(0, 4)
        if kind == 0:
            m = rng.integers(0, 30)
            xy = rng.uniform(-15, 25, (m, 2))
            t = rng.integers(0, 5, m)
        elif kind == 1:
            nl, nr = rng.integers(0, 9), rng.integers(0, 9)
            xl, xr = np.sort(rng.uniform(-6, 30, nl)), np.sort(rng.uniform(-6, 30, nr))
            curv = rng.uniform(-0.06, 0.06)

            def bend(x, off):
                return np.column_stack([x, off + 0.5 * curv * x * x]) + rng.normal(0, 0.2, (len(x), 2))

            xy = np.concatenate([bend(xl, 1.5), bend(xr, -1.5)])
            t = np.concatenate([np.full(nl, 2), np.full(nr, 1)])
            if rng.random() < 0.4:
                t[:] = 0
            if rng.random() < 0.3 and len(t):
                t[rng.integers(0, len(t))] = rng.integers(0, 5)
        elif kind == 2:
            off, cones, poses = synth.make_replay_batch(
                1, int(rng.integers(8, 40)), float(rng.uniform(0, 0.4)), seed=int(rng.integers(1 << 30)),
                color=bool(rng.random() < 0.6), random_pose=True, lateral_noise=float(rng.uniform(0, 1)),
                heading_noise=float(rng.uniform(0, 0.5)))
            frames.append((cones, poses[0]))
            continue
        else:
            m = rng.integers(2, 12)
            sp = rng.uniform(2.5, 6)
            x = np.arange(m) * sp - rng.uniform(0, 8)
            curv = rng.uniform(-0.05, 0.05)
            yl, yr = 1.5 + 0.5 * curv * x * x, -1.5 + 0.5 * curv * x * x
            xy = np.concatenate([np.column_stack([x, yl]), np.column_stack([x + rng.uniform(-1, 1), yr])])
            xy = xy + rng.normal(0, 0.1, (2 * m, 2))
            t = np.concatenate([np.full(m, 2), np.full(m, 1)])
            drop = rng.random(2 * m) < rng.uniform(0, 0.4)
            xy, t = xy[~drop], t[~drop]
            if rng.random() < 0.3:
                t[:] = 0
        order = np.argsort(t, kind="stable")
        xyt = np.column_stack([xy[order], t[order].astype(float)]) if len(t) else np.zeros((0, 3))
        a = rng.normal(0, 0.3)
        frames.append((xyt, np.array([rng.normal(0, 0.5), rng.normal(0, 0.5), np.cos(a), np.sin(a)])))
    off = np.concatenate([[0], np.cumsum([len(f[0]) for f in frames])]).astype(np.int32)
    return off, np.concatenate([f[0].reshape(-1, 3) for f in frames]), np.array([f[1] for f in frames])


def spline_fixtures(seed=0, n=90):
    """scipy.interpolate.splprep/splev outputs (the FITPACK arithmetic the reference reaches
    through utils/spline_fit.py:117,61) for the three fit shapes of the pipeline."""
    from scipy.interpolate import splev, splprep

    rng = np.random.default_rng(seed)
    items = {}
    for i in range(n):
        mode = i % 3
        if mode == 0:
            m, length, noise, s = int(rng.integers(2, 15)), None, 0.3, 0.2
            length = m * 3.0
        elif mode == 1:
            m, length, noise, s = int(rng.integers(300, 600)), 50.0, 0.004, 0.2
        else:
            m, length, noise, s = int(rng.integers(150, 250)), 20.0, 0.001, 0.01
        ss = np.linspace(0, length, m)
        th = rng.uniform(-0.08, 0.08) * ss + rng.uniform(-3, 3) + 0.3 * np.sin(ss / 7 + rng.uniform(0, 6))
        tr = np.column_stack([np.cumsum(np.cos(th)), np.cumsum(np.sin(th))]) * (length / m) + rng.normal(0, noise, (m, 2))
        k = int(np.clip(m - 1, 1, 3))
        u = np.concatenate(([0.0], np.cumsum(np.linalg.norm(np.diff(tr, axis=0), axis=1))))
        (tck, _), fp, ier, _ = splprep(tr.T, s=s, k=k, u=u, full_output=1)
        ue = np.arange(0, u[-1] * 1.1, u[-1] / 57.0)
        ev = np.array(splev(ue, tck)).T
        items[f"trace_{i}"] = tr
        items[f"s_{i}"] = np.array([s, k, ier, fp])
        items[f"t_{i}"] = tck[0]
        items[f"c_{i}"] = np.array(tck[1])
        items[f"ue_{i}"] = ue
        items[f"ev_{i}"] = ev
    items["n"] = np.array(n)
    return items


def lattice_frames(seed=7, trials=400, want=24):
    """Colourless staggered lattices (2-4.5 m spacing): the depth-first search of the sorter finds up to ~200 raw end
    configurations per side on them — the frames that exceed the 64 the product kernel holds in LDS (sort_big_kernel)."""
    rng = np.random.default_rng(seed)
    frames = []
    for trial in range(trials):
        sp = rng.uniform(2.0, 4.5)
        nx, ny = int(rng.integers(6, 14)), int(rng.integers(3, 8))
        gx, gy = np.meshgrid(np.arange(nx) * sp, (np.arange(ny) - (ny - 1) / 2) * sp * rng.uniform(0.6, 1.0))
        if trial % 2:
            gx = gx + (np.arange(ny)[:, None] % 2) * sp / 2
        xy = np.column_stack([gx.ravel() + rng.uniform(-1, 3), gy.ravel()]) + rng.normal(0, rng.uniform(0, 0.3), (nx * ny, 2))
        pose = np.array([0.0, rng.uniform(-1, 1), 1.0, 0.0])
        if trial in (7, 33, 43, 143, 145, 181, 197, 203, 207, 221, 231, 265, 269, 275, 293, 301, 305, 317, 327, 331, 2, 4, 6, 8):
            frames.append((np.column_stack([xy, np.zeros(len(xy))]), pose))
    frames = frames[:want]
    off = np.concatenate([[0], np.cumsum([len(f[0]) for f in frames])]).astype(np.int32)
    return off, np.concatenate([f[0] for f in frames]), np.array([f[1] for f in frames])


def capacity_golden():
    """Frames beyond the product kernels' LDS capacities: 300 and 600 cones (coloured and colourless; a whole SLAM map
    handed in every frame, demo/json_demo.py:255-275) and lattices with more than 64 raw end configurations."""
    refharness.load()
    sets = {}
    parts = []
    for n_side, seed in ((150, 21), (300, 22)):
        for color in (True, False):
            parts.append(synth.make_replay_batch(4, n_side, 0.15, seed=seed, color=color, random_pose=True))
    off = np.concatenate([[0]] + [p[0][1:] + sum(int(q[0][-1]) for q in parts[:i]) for i, p in enumerate(parts)]).astype(np.int32)
    sets["big_frames"] = capture(off, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]))
    sets["lattice"] = capture(*lattice_frames())
    for name, d in sets.items():
        np.savez_compressed(HERE / f"{name}.npz", **d)
        print(name, "frames", len(d["ok"]), "ok", int(d["ok"].sum()), "exc", sorted(set(d["exc"].tolist()) - {""}),
              "cones", np.diff(d["offsets"]).tolist()[:20], "configs", d["n_configs_left"].tolist(), d["n_configs_right"].tolist())


PARAM_SETS = {
    # two non-default parameter sets: a tighter sorter, and a smoother / shorter path
    "params_sort": dict(max_dist=5.5, max_length=10, max_dist_to_first=5.0, max_n_neighbors=4,
                        threshold_directional_angle=float(np.deg2rad(35)), threshold_absolute_angle=float(np.deg2rad(60)),
                        min_track_width=2.8, max_search_range=4.5, max_search_angle=float(np.deg2rad(45))),
    "params_path": dict(smoothing=0.1, mpc_path_length=15, predict_every=0.125, maximal_distance_for_valid_path=4),
}


def params_golden():
    """The reference with non-default constructor kwargs of its stage classes, on coloured / colourless replay frames and
    fuzz frames; the parameter values are stored with the frames."""
    refharness.load()
    o2, c2, p2 = synth.make_replay_batch(4096, 64, 0.15, seed=1, color=True)
    o3, c3, p3 = synth.make_replay_batch(4096, 64, 0.15, seed=1, color=False)
    of, cf, pf = fuzz_frames(12, 120)
    for name, prm in PARAM_SETS.items():
        parts = [capture(o2, c2, p2, range(0, 4096, 128), params=prm), capture(o3, c3, p3, range(64, 4096, 256), params=prm),
                 capture(of, cf, pf, params=prm)]
        d = {}
        for k in parts[0]:
            if k == "offsets":
                offs, base = [np.zeros(1, np.int32)], 0
                for q in parts:
                    offs.append(q["offsets"][1:] + base)
                    base += int(q["offsets"][-1])
                d[k] = np.concatenate(offs).astype(np.int32)
            else:
                d[k] = np.concatenate([q[k] for q in parts])
        d["param_names"] = np.array(list(prm.keys()))
        d["param_values"] = np.array([float(v) for v in prm.values()])
        np.savez_compressed(HERE / f"{name}.npz", **d)
        print(name, "frames", len(d["ok"]), "ok", int(d["ok"].sum()), "exc", sorted(set(d["exc"].tolist()) - {""}))


PARAM_SETS_R3 = {
    # round 3: the values the library used to refuse
    "params_monotonic": dict(matches_should_be_monotonic=True),
    "params_deg2": dict(max_deg=2),
    "params_deg1": dict(max_deg=1),
    "params_horizon": dict(mpc_prediction_horizon=25),
    "params_no_unknown": dict(use_unknown_cones=False),
}


PARAM_SETS_R5 = {
    # round 5 (VERDICT r4 "missing" 1): structural parameters beyond the standard shapes — the library's wide build
    # (include/fsdp.h FSDP_WIDE_SHAPES: max_n_neighbors <= 8, max_length <= 16, mpc_prediction_horizon <= 64)
    "params_wide_sort": dict(max_n_neighbors=8, max_length=16),
    "params_wide_horizon": dict(mpc_prediction_horizon=64, mpc_path_length=30),
    "params_wide_all": dict(max_n_neighbors=7, max_length=15, max_dist=7.0, mpc_prediction_horizon=55),
}
WIDE_SHAPES = (16, 32, 64)


def params_golden_r5():
    refharness.load()
    o2, c2, p2 = synth.make_replay_batch(4096, 64, 0.15, seed=1, color=True)
    o3, c3, p3 = synth.make_replay_batch(4096, 64, 0.15, seed=1, color=False)
    of, cf, pf = fuzz_frames(14, 100)
    for name, prm in PARAM_SETS_R5.items():
        parts = [capture(o2, c2, p2, range(0, 4096, 128), params=prm, shapes=WIDE_SHAPES),
                 capture(o3, c3, p3, range(64, 4096, 256), params=prm, shapes=WIDE_SHAPES),
                 capture(of, cf, pf, params=prm, shapes=WIDE_SHAPES)]
        d = {}
        for k in parts[0]:
            if k == "offsets":
                offs, base = [np.zeros(1, np.int32)], 0
                for q in parts:
                    offs.append(q["offsets"][1:] + base)
                    base += int(q["offsets"][-1])
                d[k] = np.concatenate(offs).astype(np.int32)
            else:
                d[k] = np.concatenate([q[k] for q in parts])
        d["param_names"] = np.array(list(prm.keys()))
        d["param_values"] = np.array([float(v) for v in prm.values()])
        np.savez_compressed(HERE / f"{name}.npz", **d)
        print(name, "frames", len(d["ok"]), "ok", int(d["ok"].sum()), "exc", sorted(set(d["exc"].tolist()) - {""}),
              "longest side", int(max(d["n_left"].max(), d["n_right"].max())), "with virtual", int(max(d["n_left_v"].max(), d["n_right_v"].max())))


if __name__ == "__main__" and "--params-r5" in sys.argv:
    params_golden_r5()
    sys.exit(0)


def with_unknown_cones(off, cones, frac, seed):
    """A copy of the batch in which a random `frac` of every frame's cones is of type UNKNOWN, rows of a frame in type
    order (the order the reference flattens per-type lists in)."""
    rng = np.random.default_rng(seed)
    out = cones.copy()
    for f in range(len(off) - 1):
        a, b = off[f], off[f + 1]
        blk = out[a:b]
        blk[rng.random(b - a) < frac, 2] = 0.0
        out[a:b] = blk[np.argsort(blk[:, 2], kind="stable")]
    return out


def params_golden_r3():
    refharness.load()
    o2, c2, p2 = synth.make_replay_batch(4096, 64, 0.15, seed=1, color=True)
    o3, c3, p3 = synth.make_replay_batch(4096, 64, 0.15, seed=1, color=False)
    of, cf, pf = fuzz_frames(13, 100)
    for name, prm in PARAM_SETS_R3.items():
        if name == "params_no_unknown":
            cu2, cuf = with_unknown_cones(o2, c2, 0.3, 5), with_unknown_cones(of, cf, 0.3, 6)
            parts = [capture(o2, cu2, p2, range(0, 4096, 128), params=prm, flattened=False), capture(of, cuf, pf, params=prm, flattened=False)]
        else:
            parts = [capture(o2, c2, p2, range(0, 4096, 128), params=prm), capture(o3, c3, p3, range(64, 4096, 256), params=prm),
                     capture(of, cf, pf, params=prm)]
        d = {}
        for k in parts[0]:
            if k == "offsets":
                offs, base = [np.zeros(1, np.int32)], 0
                for q in parts:
                    offs.append(q["offsets"][1:] + base)
                    base += int(q["offsets"][-1])
                d[k] = np.concatenate(offs).astype(np.int32)
            else:
                d[k] = np.concatenate([q[k] for q in parts])
        d["param_names"] = np.array(list(prm.keys()))
        d["param_values"] = np.array([float(v) for v in prm.values()])
        np.savez_compressed(HERE / f"{name}.npz", **d)
        print(name, "frames", len(d["ok"]), "ok", int(d["ok"].sum()), "exc", sorted(set(d["exc"].tolist()) - {""}))


if __name__ == "__main__" and "--params-r3" in sys.argv:
    params_golden_r3()
    sys.exit(0)


def add_intermediates():
    """Re-run the reference on the committed frame sets and add the per-stage intermediates; every field the files already
    hold must come out identical."""
    refharness.load()
    for name in ("scenarios", "cfg2_color", "cfg3_nocolor", "cfg4_200cones", "cfg4_noisy_nocolor", "fuzz"):
        old = dict(np.load(HERE / f"{name}.npz"))
        new = capture(old["offsets"], old["cones"], old["poses"])
        for k, v in old.items():
            if k in new:
                assert np.array_equal(v, new[k], equal_nan=v.dtype.kind == "f"), (name, k)
            else:
                new[k] = v
        np.savez_compressed(HERE / f"{name}.npz", **new)
        print(name, "frames", len(new["ok"]), "first_k", int((new["first_k_left"][:, 0] >= 0).sum()), "max configs",
              int(new["n_configs_left"].max()), int(new["n_configs_right"].max()))


def main():
    refharness.load()
    sets = {}
    off, cones, poses, names = scenario_frames()
    sets["scenarios"] = capture(off, cones, poses)
    sets["scenarios"]["names"] = np.array(names)
    o, c, p = synth.make_replay_batch(4096, 64, 0.15, seed=1, color=True)
    sets["cfg2_color"] = capture(o, c, p, range(0, 4096, 64))
    o, c, p = synth.make_replay_batch(4096, 64, 0.15, seed=1, color=False)
    sets["cfg3_nocolor"] = capture(o, c, p, range(0, 4096, 64))
    o, c, p = synth.make_replay_batch(48, 100, 0.0, seed=7, frame_noise=0.1, random_pose=True)
    sets["cfg4_200cones"] = capture(o, c, p)
    o, c, p = synth.make_replay_batch(48, 100, 0.0, seed=8, frame_noise=0.3, random_pose=True, color=False,
                                      lateral_noise=0.5, heading_noise=0.2)
    sets["cfg4_noisy_nocolor"] = capture(o, c, p)
    o, c, p = fuzz_frames(11, 400)
    sets["fuzz"] = capture(o, c, p)
    for name, d in sets.items():
        np.savez_compressed(HERE / f"{name}.npz", **d)
        print(name, "frames", len(d["ok"]), "ok", int(d["ok"].sum()), "exc", sorted(set(d["exc"].tolist()) - {""}))
    np.savez_compressed(HERE / "splines.npz", **spline_fixtures())
    # constant initial previous path (core_calculate_path.py:103-107)
    m = refharness.load()
    pp = m["PathPlanner"](m["MissionTypes"].trackdrive)
    np.savez_compressed(HERE / "default_path.npz", path=np.array(pp.pathing.previous_paths[0]))
    # numpy/BLAS semantics probes used by the oracle's np_compat.h
    rng = np.random.default_rng(5)
    v = rng.uniform(-60, 60, (400, 2))
    m2 = rng.uniform(-1, 1, (2, 2))
    from fsd_path_planning.utils.math_utils import my_cdist_sq_euclidean, rotate

    np.savez_compressed(
        HERE / "numpy_semantics.npz", v=v, m2=m2, dot=np.dot(v, m2), norm1d=np.array([np.linalg.norm(r) for r in v]),
        cdist=my_cdist_sq_euclidean(v[:40], v[:40]), rot=rotate(v, 0.7), rot_theta=np.array(0.7),
        sums=np.array([v[:k, 0].sum() for k in range(1, 400)]),
    )
    skidpad_golden()




def skidpad_golden():
    """demo/skidpad.json (341 frames) replayed through ONE reference PathPlanner(MissionTypes.skidpad): the stateful
    sequence (relocalizes at frame 16).  Stored: inputs as CSR + per-frame path, relocalization info, index_along_path."""
    import json

    m = refharness.load()
    d = json.load(open("/root/reference/fsd_path_planning/demo/skidpad.json"))
    pp = m["PathPlanner"](m["MissionTypes"].skidpad)
    cones_all, off, poses, paths, reloc, info, idx = [], [0], [], [], [], [], []
    for f in d:
        cones = [np.array(c, dtype=float).reshape(-1, 2) for c in f["slam_cones"]]
        xyt = np.concatenate([np.column_stack([c, np.full(len(c), float(t))]) for t, c in enumerate(cones)])
        pos, dr = np.array(f["car_position"], float), np.array(f["car_direction"], float)
        path = pp.calculate_path_in_global_frame(cones, pos, dr)
        cones_all.append(xyt.reshape(-1, 3))
        off.append(off[-1] + len(xyt))
        poses.append(np.concatenate([pos, dr]))
        paths.append(np.array(path))
        ri = pp.relocalization_info
        reloc.append(ri is not None)
        info.append([np.nan] * 3 if ri is None else [ri.translation[0], ri.translation[1], ri.rotation])
        idx.append(pp.pathing.index_along_path)
    np.savez_compressed(
        HERE / "skidpad_sequence.npz", offsets=np.array(off, np.int32), cones=np.concatenate(cones_all), poses=np.array(poses),
        path=np.array(paths), relocalized=np.array(reloc), info=np.array(info), index_along_path=np.array(idx, np.int32),
        reference_centers=np.array(pp.relocalizer.reference_centers),
    )
    print("skidpad_sequence frames", len(d), "relocalized from frame", int(np.argmax(reloc)))


if __name__ == "__main__" and "--skidpad-only" in sys.argv:
    skidpad_golden()


def trackdrive_sequence_golden():
    """ONE reference PathPlanner(trackdrive) driven along a synthetic loop for 90 consecutive frames with cone drop-outs,
    so that the stateful previous-path fallbacks (core_calculate_path.py:203,531-536,568-573) are exercised."""
    m = refharness.load()
    rng = np.random.default_rng(21)
    left, right, centre_fn = synth.closed_track(40, 21)
    left = left + rng.normal(0, 0.1, left.shape)
    right = right + rng.normal(0, 0.1, right.shape)
    pp = m["PathPlanner"](m["MissionTypes"].trackdrive)
    cones_all, off, poses, paths, ok = [], [0], [], [], []
    for t in range(90):
        pos, tan = centre_fn(0.1 + t * 0.0035)
        l, r = left, right
        if t % 9 in (4, 5):  # perception drop-out: nothing but two far cones
            l, r = left[:1], right[:1]
        if t % 13 == 7:  # only one side visible
            l = left[:0]
        xyt = np.concatenate([np.column_stack([r, np.full(len(r), 1.0)]), np.column_stack([l, np.full(len(l), 2.0)])])
        try:
            path = pp.calculate_path_in_global_frame(xyt, np.array(pos), np.array(tan))
            ok.append(True)
        except Exception:  # noqa
            path = np.full((40, 4), np.nan)
            ok.append(False)
        cones_all.append(xyt)
        off.append(off[-1] + len(xyt))
        poses.append(np.concatenate([pos, tan]))
        paths.append(np.array(path))
    np.savez_compressed(HERE / "trackdrive_sequence.npz", offsets=np.array(off, np.int32), cones=np.concatenate(cones_all),
                        poses=np.array(poses), path=np.array(paths), ok=np.array(ok))
    print("trackdrive_sequence frames", len(ok), "ok", int(np.sum(ok)))


if __name__ == "__main__" and "--sequence-only" in sys.argv:
    trackdrive_sequence_golden()


def global_path_golden():
    """(1) ONE reference PathPlanner(trackdrive) with set_global_path(centre line of a synthetic loop): 40 consecutive
    frames (core_calculate_path.py:514-529: the path follows the global path, sorting / matching results are ignored).
    (2) ONE reference PathPlanner(acceleration) driven down a synthetic acceleration lane.  Its relocalizer draws from
    NumPy's global RNG (acceleration_relocalization.py:32); np.random.seed(ACCEL_SEED) right before the first call pins
    the draw, which is what the build's explicit seed parameter reproduces.  Also stored: the relocalizer's known path
    table BASE_ACCELERATION_PATH (data) and the relocalization angle."""
    m = refharness.load()
    # ---- (1) trackdrive + global path
    left, right, centre_fn = synth.closed_track(40, 33)
    gp = np.array([centre_fn(s)[0] for s in np.linspace(0, 1, 600, endpoint=False)])
    pp = m["PathPlanner"](m["MissionTypes"].trackdrive)
    pp.set_global_path(gp)
    cones_all, off, poses, paths = [], [0], [], []
    rng = np.random.default_rng(5)
    for t in range(40):
        pos, tan = centre_fn(0.05 + t * 0.004)
        pos = np.array(pos) + rng.normal(0, 0.3, 2)
        xyt = np.concatenate([np.column_stack([right, np.full(len(right), 1.0)]), np.column_stack([left, np.full(len(left), 2.0)])])
        path = pp.calculate_path_in_global_frame(xyt, pos, np.array(tan))
        cones_all.append(xyt)
        off.append(off[-1] + len(xyt))
        poses.append(np.concatenate([pos, tan]))
        paths.append(np.array(path))
    out = dict(gp_track=gp, gp_offsets=np.array(off, np.int32), gp_cones=np.concatenate(cones_all), gp_poses=np.array(poses),
               gp_path=np.array(paths))
    # ---- (2) acceleration mission
    from fsd_path_planning.relocalization.acceleration.acceleration_relocalization import BASE_ACCELERATION_PATH

    ACCEL_SEED = 1234
    world_yaw, world_t = 0.7, np.array([12.0, -3.0])
    c, s = np.cos(world_yaw), np.sin(world_yaw)
    R = np.array([[c, -s], [s, c]])
    xs = np.arange(-5.0, 80.0, 5.0)
    rng = np.random.default_rng(6)
    lane_l = np.column_stack([xs, np.full(len(xs), 1.5)]) + rng.normal(0, 0.05, (len(xs), 2))
    lane_r = np.column_stack([xs, np.full(len(xs), -1.5)]) + rng.normal(0, 0.05, (len(xs), 2))
    to_world = lambda p: p @ R.T + world_t
    pp = m["PathPlanner"](m["MissionTypes"].acceleration)
    cones_all, off, poses, paths, reloc, angle = [], [0], [], [], [], []
    np.random.seed(ACCEL_SEED)
    for t in range(30):
        x = -8.0 + 1.5 * t  # the first frames see fewer than 4 cones in the left band: relocalization comes later
        pos_l = np.array([x, 0.1 * np.sin(0.3 * t)])
        yaw_l = 0.02 * np.cos(0.2 * t)
        vis = lambda lane: lane[(lane[:, 0] > x + 0.5) & (lane[:, 0] < x + 0.5 + (6.0 if t < 3 else 25.0))]
        cones = [np.zeros((0, 2)), to_world(vis(lane_r)), to_world(vis(lane_l)), np.zeros((0, 2)), np.zeros((0, 2))]
        pos = to_world(pos_l[None])[0]
        dr = np.array([np.cos(yaw_l + world_yaw), np.sin(yaw_l + world_yaw)])
        path = pp.calculate_path_in_global_frame(cones, pos, dr)
        xyt = np.concatenate([np.column_stack([cc, np.full(len(cc), float(tt))]) for tt, cc in enumerate(cones)])
        cones_all.append(xyt.reshape(-1, 3))
        off.append(off[-1] + len(xyt))
        poses.append(np.concatenate([pos, dr]))
        paths.append(np.array(path))
        reloc.append(pp.relocalizer.is_relocalized)
        if pp.relocalizer.is_relocalized:
            p0, y0 = pp.relocalizer.transform_to_known_map_frame(np.zeros(2), 0.0)
            angle.append(-y0)
        else:
            angle.append(np.nan)
    out.update(acc_table=np.array(BASE_ACCELERATION_PATH), acc_seed=np.array(ACCEL_SEED), acc_offsets=np.array(off, np.int32),
               acc_cones=np.concatenate(cones_all), acc_poses=np.array(poses), acc_path=np.array(paths),
               acc_relocalized=np.array(reloc), acc_angle=np.array(angle))
    np.savez_compressed(HERE / "global_path.npz", **out)
    print("global_path: trackdrive frames", len(out["gp_path"]), "| acceleration frames", len(paths), "relocalized from frame",
          int(np.argmax(reloc)), "angle", angle[-1])


if __name__ == "__main__" and "--global-path-only" in sys.argv:
    global_path_golden()
if __name__ == "__main__" and "--capacity-only" in sys.argv:
    capacity_golden()
if __name__ == "__main__" and "--params-only" in sys.argv:
    params_golden()
if __name__ == "__main__" and "--intermediates-only" in sys.argv:
    add_intermediates()


if __name__ == "__main__" and not any(a.endswith("-only") for a in sys.argv[1:]):
    main()
    trackdrive_sequence_golden()
    global_path_golden()


def skidpad_awkward_golden():
    """tests/skidpad_support.py awkward_frames (46 frames of demo/skidpad.json for three rigidly perturbed planners, with a
    car 60 m off the track, positions / directions that are not finite, a car moved 15 m along the track) through three
    reference PathPlanner(MissionTypes.skidpad) objects, exceptions caught the way a caller would: what a step that falls
    back or raises leaves behind (path, index_along_path — moved although the step raised —, the later steps)."""
    sys.path.insert(0, str(HERE.parent))
    import skidpad_support as sk

    m = refharness.load()
    g = np.load(HERE / "skidpad_sequence.npz")
    tf = sk.perturbed_instances(g, 3)
    frames = sk.awkward_frames(g, tf, 46)
    planners = [m["PathPlanner"](m["MissionTypes"].skidpad) for _ in tf]
    T, n = len(frames), len(tf)
    ok = np.zeros((T, n), bool)
    exc = np.zeros((T, n), "U24")
    path = np.full((T, n, 40, 4), np.nan)
    idx = np.zeros((T, n), np.int32)
    reloc = np.zeros((T, n), bool)
    for t, (off, cones, poses) in enumerate(frames):
        for i, pp in enumerate(planners):
            xyt = cones[off[i] : off[i + 1]]
            by_type = [xyt[xyt[:, 2] == k, :2] for k in range(5)]
            try:
                with np.errstate(all="ignore"):
                    path[t, i] = pp.calculate_path_in_global_frame(by_type, poses[i, :2], poses[i, 2:])
                ok[t, i] = True
            except Exception as e:  # noqa: BLE001
                exc[t, i] = type(e).__name__
            idx[t, i] = pp.pathing.index_along_path
            reloc[t, i] = pp.relocalization_info is not None
    np.savez_compressed(HERE / "skidpad_awkward.npz", ok=ok, exc=exc, path=path, index_along_path=idx, relocalized=reloc)
    print("skidpad_awkward: raised", int((~ok).sum()), "of", ok.size, "steps:", sorted(set(exc[~ok].tolist())), "index after raising steps", idx[~ok].tolist())


if __name__ == "__main__" and "--skidpad-awkward" in sys.argv:
    skidpad_awkward_golden()


def nonfinite_poses_golden():
    """24 autocross frames (12 coloured, 12 without colour) whose pose has one component that is NaN / +inf / -inf: the
    reference raises ValueError for a position that is not finite and plans normally for a direction that is not."""
    refharness.load()
    sets = []
    for color in (True, False):
        o, c, p = synth.make_replay_batch(12, 64, 0.15, seed=1, color=color)
        p = p.copy()
        for k in range(12):
            p[k, k % 4] = [np.nan, np.inf, -np.inf][k // 4]
        sets.append((o, c, p))
    off = np.concatenate([sets[0][0], sets[0][0][-1] + sets[1][0][1:]]).astype(np.int32)
    cones = np.concatenate([sets[0][1], sets[1][1]])
    poses = np.concatenate([sets[0][2], sets[1][2]])
    with np.errstate(all="ignore"):
        d = capture(off, cones, poses)
    np.savez_compressed(HERE / "nonfinite_poses.npz", **d)
    print("nonfinite_poses frames", len(d["ok"]), "ok", int(d["ok"].sum()), "exc", sorted(set(d["exc"].tolist()) - {""}))


if __name__ == "__main__" and "--nonfinite" in sys.argv:
    nonfinite_poses_golden()


def nonfinite_cones_golden():
    """48 autocross frames (24 coloured, 24 without colour) in which one to three cones — the closest to the car, or any —
    have a coordinate that is NaN / +inf / -inf: the reference plans around them (they end up with no neighbours:
    np.argsort puts their distances last, adjacency_matrix.py:56)."""
    refharness.load()
    sets = []
    rng = np.random.default_rng(0)
    vals = [np.nan, np.inf, -np.inf]
    for color in (True, False):
        o, c, p = synth.make_replay_batch(24, 64, 0.15, seed=2, color=color)
        c = c.copy()
        for k in range(24):
            lo, hi = o[k], o[k + 1]
            d = np.hypot(c[lo:hi, 0] - p[k, 0], c[lo:hi, 1] - p[k, 1])
            pick = np.argsort(d)[: 1 + k % 3] if k % 2 == 0 else rng.choice(hi - lo, 1 + k % 3, replace=False)
            for j in pick:
                c[lo + j, (k // 2) % 2] = vals[k % 3]
        sets.append((o, c, p))
    off = np.concatenate([sets[0][0], sets[0][0][-1] + sets[1][0][1:]]).astype(np.int32)
    cones = np.concatenate([sets[0][1], sets[1][1]])
    poses = np.concatenate([sets[0][2], sets[1][2]])
    with np.errstate(all="ignore"):
        d = capture(off, cones, poses)
    np.savez_compressed(HERE / "nonfinite_cones.npz", **d)
    print("nonfinite_cones frames", len(d["ok"]), "ok", int(d["ok"].sum()), "exc", sorted(set(d["exc"].tolist()) - {""}))


if __name__ == "__main__" and "--nonfinite-cones" in sys.argv:
    nonfinite_cones_golden()


def odd_inputs_golden():
    """21 autocross frames with finite but unusual inputs: a zero / tiny / huge direction vector, coordinates offset by 1e7
    and 1e12 (the reference raises IndexError there: the sorting search runs out of its buffers), 20 duplicated cones
    (no-colour: no ties that NumPy's unstable argsort would decide), all cones on one point, collinear cones, a single
    colour, a cone exactly at the car, the track scaled by 0.2 and by 1e-3, denormal coordinates, a pose of -0.0, and
    frames of 0 / 1 / 2 / 3 / 5 cones."""
    refharness.load()

    def base(color=True):
        o, c, p = synth.make_replay_batch(1, 64, 0.15, seed=1, color=color)
        return c[o[0] : o[1]].copy(), p[0].copy()

    frames, names = [], []

    def add(name, c, p):
        frames.append((c, p))
        names.append(name)

    c, p = base(); p[2:] = 0; add("direction zero", c, p)
    c, p = base(); p[2:] *= 1e-300; add("direction 1e-300", c, p)
    c, p = base(); p[2:] *= 1e150; add("direction 1e150", c, p)
    c, p = base(); c[:, :2] += 1e7; p[:2] += 1e7; add("offset 1e7", c, p)
    c, p = base(); c[:, :2] += 1e12; p[:2] += 1e12; add("offset 1e12", c, p)
    c, p = base(False); c = np.concatenate([c, c[:20]]); add("20 duplicates, no colour", c, p)
    c, p = base(); c[:, :2] = p[:2] + np.array([3.0, 1.0]); add("all cones on one point", c, p)
    c, p = base(); t = np.linspace(1, 60, len(c)); c[:, 0] = p[0] + t * p[2]; c[:, 1] = p[1] + t * p[3]; add("collinear", c, p)
    c, p = base(); c[:, 2] = 1; add("all right", c, p)
    c, p = base(); c[:, 2] = 3; add("all orange small", c, p)
    c, p = base(); c[0, :2] = p[:2]; add("cone at the car", c, p)
    c, p = base(False); c[0, :2] = p[:2]; add("cone at the car, no colour", c, p)
    c, p = base(); c[:, :2] = p[:2] + (c[:, :2] - p[:2]) * 1e-3; add("track scaled 1e-3", c, p)
    c, p = base(); c[:, :2] = p[:2] + (c[:, :2] - p[:2]) * 0.2; add("track scaled 0.2", c, p)
    c, p = base(); c[:5, 0] = 5e-324; add("denormal x", c, p)
    c, p = base(); c[:, :2] -= p[:2]; p[:2] = -0.0; add("pose -0.0", c, p)
    for k in (0, 1, 2, 3, 5):
        c, p = base(); d = np.hypot(c[:, 0] - p[0], c[:, 1] - p[1]); add(f"{k} cones", c[np.argsort(d)[:k]], p)
    off = np.concatenate([[0], np.cumsum([len(c) for c, _ in frames])]).astype(np.int32)
    cones = np.concatenate([c.reshape(-1, 3) for c, _ in frames])
    poses = np.array([p for _, p in frames])
    with np.errstate(all="ignore"):
        d = capture(off, cones, poses)
    d["names"] = np.array(names)
    np.savez_compressed(HERE / "odd_inputs.npz", **d)
    print("odd_inputs frames", len(d["ok"]), "ok", int(d["ok"].sum()), "exc", sorted(set(d["exc"].tolist()) - {""}))


if __name__ == "__main__" and "--odd-inputs" in sys.argv:
    odd_inputs_golden()


def stage_centers_golden():
    """The reference's CalculatePath stage class on its own (README.md:78-79): run_path_calculation returns
    (path, center_along_match_connection) — core_calculate_path.py:575.  Inputs: the matching outputs the reference produced
    for the frames of fuzz.npz and scenarios.npz (every branch that picks the centre points: matches of the better side,
    < 2 matches -> previous path, < 3 cones on both sides -> previous path), a fresh stage object per frame, plus 12 frames
    with a global path (the slice within 30 m, rolled).  Stored: the inputs' frame indices, the centre points (padded) and
    the path."""
    m = refharness.load()
    from fsd_path_planning.calculate_path.core_calculate_path import PathCalculationInput
    from fsd_path_planning import config as cfg

    mission = m["MissionTypes"].trackdrive
    rows = []
    for name in ("fuzz", "scenarios", "odd_inputs"):
        g = np.load(HERE / f"{name}.npz")
        idx = np.flatnonzero(g["ok"])
        if name == "fuzz":
            idx = idx[::4]
        for f in idx:
            nl, nr = int(g["n_left_v"][f]), int(g["n_right_v"][f])
            rows.append((name, int(f), g["left_v"][f, :nl], g["right_v"][f, :nr], g["l2r"][f, :nl].astype(np.int64),
                         g["r2l"][f, :nr].astype(np.int64), g["poses"][f], None))
    left, right, centre_fn = synth.closed_track(40, 33)
    gp = np.array([centre_fn(s)[0] for s in np.linspace(0, 1, 600, endpoint=False)])
    rng = np.random.default_rng(9)
    for t in range(12):
        pos, tan = centre_fn(0.03 + t * 0.07)
        rows.append(("global", t, np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0, np.int64), np.zeros(0, np.int64),
                     np.concatenate([np.array(pos) + rng.normal(0, 0.3, 2), tan]), gp))
    F = len(rows)
    CAP = 640
    out = dict(set=np.array([r[0] for r in rows]), frame=np.array([r[1] for r in rows], np.int32), ok=np.zeros(F, bool),
               exc=np.array([""] * F, dtype="U24"), poses=np.array([r[6] for r in rows]), n_left_v=np.zeros(F, np.int32),
               n_right_v=np.zeros(F, np.int32), left_v=np.zeros((F, MAX_MATCH, 2)), right_v=np.zeros((F, MAX_MATCH, 2)),
               l2r=np.full((F, MAX_MATCH), -1, np.int32), r2l=np.full((F, MAX_MATCH), -1, np.int32),
               uses_global=np.zeros(F, bool), global_path=gp, n_centers=np.zeros(F, np.int32), centers=np.zeros((F, CAP, 2)),
               path=np.full((F, 40, 4), np.nan))
    for k, (name, f, lv, rv, l2r, r2l, pose, gpath) in enumerate(rows):
        out["n_left_v"][k], out["n_right_v"][k] = len(lv), len(rv)
        out["left_v"][k, : len(lv)], out["right_v"][k, : len(rv)] = lv, rv
        out["l2r"][k, : len(lv)], out["r2l"][k, : len(rv)] = l2r, r2l
        out["uses_global"][k] = gpath is not None
        stage = cfg.create_default_pathing(mission)
        stage.set_new_input(PathCalculationInput(lv, rv, l2r, r2l, pose[:2], pose[2:], gpath))
        try:
            with np.errstate(all="ignore"):
                path, centers = stage.run_path_calculation()
        except Exception as e:  # noqa: BLE001 (which class is part of the fixture)
            out["exc"][k] = type(e).__name__
            continue
        out["ok"][k] = True
        assert len(centers) <= CAP
        out["n_centers"][k] = len(centers)
        out["centers"][k, : len(centers)] = centers
        out["path"][k] = path
    np.savez_compressed(HERE / "stage_centers.npz", **out)
    print("stage_centers frames", F, "ok", int(out["ok"].sum()), "exc", sorted(set(out["exc"].tolist()) - {""}),
          "centre counts", sorted(set(out["n_centers"].tolist()))[:12], "...")


if __name__ == "__main__" and "--stage-centers-only" in sys.argv:
    stage_centers_golden()


def gemv_semantics_golden():
    """np.dot of ONE point with a 2 x 2 matrix (gemv) versus rows of a 2-D array (gemm), as this NumPy / OpenBLAS build
    evaluates them — what utils/math_utils.py:103-117 rotate() returns for a single position (the skidpad mission's pose
    transform, skidpad_relocalizer.py:140-153) and for arrays of points.  Values only."""
    rng = np.random.default_rng(21)
    v = rng.uniform(-700, 700, (300, 2))
    th = rng.uniform(-3.2, 3.2, 300)
    from fsd_path_planning.utils.math_utils import rotate

    single = np.array([rotate(v[i], th[i]) for i in range(300)])             # 1-D point
    one_row = np.array([rotate(v[i : i + 1], th[i])[0] for i in range(300)])  # (1, 2) array
    two_rows = np.array([rotate(v[i : i + 2], th[i])[0] for i in range(299)])  # first row of a (2, 2) array
    many = rotate(v, 0.7)
    np.savez_compressed(HERE / "numpy_semantics_gemv.npz", v=v, th=th, cos=np.cos(th), sin=np.sin(th), single=single, one_row=one_row,
                        two_rows=two_rows, many=many, cos07=np.cos(0.7), sin07=np.sin(0.7))
    print("gemv semantics: 300 single points, 300 one-row arrays, 299 two-row arrays, one 300-row array")


if __name__ == "__main__" and "--gemv-only" in sys.argv:
    refharness.load()
    gemv_semantics_golden()


def match_degenerate_golden():
    """Sides with coincident cones (tests/match_support.py degenerate(): a pair at the start, the end, the interior of a side,
    a side of two coincident cones, triples, a cone shared by both sides) through the reference's ConeMatching stage object
    (the pipeline's parameters: cfg.get_default_matching_kwargs, non-monotonic), and 64 frames with one cone reported twice
    (match_support.duplicated_cone_frames) through the whole planner.  A zero chord makes the reference's search direction
    0 / 0: it goes on with NaN (warnings, no exception) — what it returns then, or which exception it raises, is the fixture:
    stage_* arrays for the sides, the usual frame layout with the prefix plan_ for the frames."""
    m = refharness.load()
    sys.path.insert(0, str(ROOT / "tests"))
    import match_support
    from fsd_path_planning import config as cfg
    from fsd_path_planning.cone_matching.core_cone_matching import ConeMatching, ConeMatchingInput

    import fsd_path_planning.cone_matching.functional_cone_matching as fcm

    # Exact ties of FINITE values in the two argsorts of the insertion (the order of the cones to insert; the two nearest
    # existing cones, where a tie among the three smallest distances can change the pair or its order): NumPy's default
    # argsort is not stable, which of the tied entries comes first depends on its build (this one: AVX-512).  Recorded per
    # case as stage_tie, like first_k_tie / knn_tie of the frame sets: the oracle's stable order is not pinned there.
    ties = [False]

    class Watched(np.ndarray):
        first_three_only = False

        def argsort(self, *a, **kw):
            v = np.sort(np.asarray(self)[np.isfinite(np.asarray(self))])
            if (np.diff(v[:3] if self.first_three_only else v) == 0).any():
                ties[0] = True
            return np.asarray(self).argsort(*a, **kw)

    class WatchedNorm(Watched):
        first_three_only = True

    class Linalg:
        @staticmethod
        def norm(x, *a, **kw):
            r = np.linalg.norm(x, *a, **kw)
            return r.view(WatchedNorm) if isinstance(r, np.ndarray) and r.ndim == 1 else r

    class NumpyProxy:
        linalg = Linalg()

        def __getattr__(self, name):
            return getattr(np, name)

    orig_np, orig_cdist = fcm.np, fcm.my_cdist_sq_euclidean
    fcm.np = NumpyProxy()
    fcm.my_cdist_sq_euclidean = lambda a, b: orig_cdist(a, b).view(Watched)
    mission = m["MissionTypes"].trackdrive
    mk = cfg.get_default_matching_kwargs(mission)
    mk["matches_should_be_monotonic"] = False  # the pipeline's choice (full_pipeline.py:65)
    cases = match_support.degenerate()
    F = len(cases)
    out = dict(stage_names=np.array([n for n, _ in cases]), stage_ok=np.zeros(F, bool), stage_exc=np.array([""] * F, dtype="U24"),
               stage_n_left=np.zeros(F, np.int32), stage_n_right=np.zeros(F, np.int32), stage_left=np.zeros((F, MAX_LEN, 2)),
               stage_right=np.zeros((F, MAX_LEN, 2)), stage_poses=np.zeros((F, 4)), stage_n_left_v=np.zeros(F, np.int32),
               stage_n_right_v=np.zeros(F, np.int32), stage_left_v=np.zeros((F, MAX_MATCH, 2)), stage_right_v=np.zeros((F, MAX_MATCH, 2)),
               stage_l2r=np.full((F, MAX_MATCH), -1, np.int32), stage_r2l=np.full((F, MAX_MATCH), -1, np.int32), stage_tie=np.zeros(F, bool))
    for k, (_name, (l, r, p)) in enumerate(cases):
        ties[0] = False
        out["stage_n_left"][k], out["stage_n_right"][k] = len(l), len(r)
        out["stage_left"][k, : len(l)], out["stage_right"][k, : len(r)], out["stage_poses"][k] = l, r, p
        sc = [np.zeros((0, 2)) for _ in range(5)]
        sc[int(m["ConeTypes"].LEFT)], sc[int(m["ConeTypes"].RIGHT)] = l.copy(), r.copy()
        stage = ConeMatching(**mk)
        stage.set_new_input(ConeMatchingInput(sc, p[:2].copy(), p[2:].copy()))
        try:
            with np.errstate(all="ignore"):
                lv, rv, l2r, r2l = stage.run_cone_matching()
        except Exception as e:  # noqa: BLE001 (which class is part of the fixture)
            out["stage_exc"][k] = type(e).__name__
            continue
        finally:
            out["stage_tie"][k] = ties[0]
        out["stage_ok"][k] = True
        assert len(lv) <= MAX_MATCH and len(rv) <= MAX_MATCH
        out["stage_n_left_v"][k], out["stage_n_right_v"][k] = len(lv), len(rv)
        out["stage_left_v"][k, : len(lv)], out["stage_right_v"][k, : len(rv)] = lv, rv
        out["stage_l2r"][k, : len(lv)], out["stage_r2l"][k, : len(rv)] = l2r, r2l
    fcm.np, fcm.my_cdist_sq_euclidean = orig_np, orig_cdist
    off, cones, poses = match_support.duplicated_cone_frames(synth)
    with np.errstate(all="ignore"):
        d = capture(off, cones, poses)
    for key, v in d.items():
        if not key.startswith("fit_"):  # (the splines are pinned on the ordinary sets)
            out["plan_" + key] = v
    np.savez_compressed(HERE / "match_degenerate.npz", **out)
    print("match_degenerate sides", F, "ok", int(out["stage_ok"].sum()), "exc", sorted(set(out["stage_exc"].tolist()) - {""}), "ties", int(out["stage_tie"].sum()),
          "NaN in the lists of", int(sum(np.isnan(out["stage_left_v"][k]).any() or np.isnan(out["stage_right_v"][k]).any() for k in range(F))),
          "| frames", len(d["ok"]), "ok", int(d["ok"].sum()), "exc", sorted(set(d["exc"].tolist()) - {""}))


if __name__ == "__main__" and "--match-degenerate-only" in sys.argv:  # (-only: without it the frame sets above are captured again first)
    match_degenerate_golden()


def sort_constructed_golden():
    """The constructed frames of the sorting stage (tests/sort_support.py: every member of every threshold pair with its mirrored
    and colourless twins, the on-threshold and the structural cases, at the canonical pose) through the reference's planner:
    left_config / right_config as calc_final_configs_for_left_and_right returns them, the start cones, the number of end
    configurations and the best cost per side -> sort_constructed.npz.  A frame on which a later stage raises keeps its sorting
    result (sort_ok); one on which the sorting stage itself raises has sort_ok False and the exception's class in exc.  Frames with
    an exact tie in one of the reference's unstable argsorts (first_k_tie / knn_tie) are listed by name in tie_names.
    knn_tie here is the condition under which the unstable argsort can change the adjacency, not refharness.knn_boundary_tie's wider
    one (any two equal distances among a cone's eight smallest — true of every chain with equal spacings): some cone's k-th and
    (k + 1)-th smallest squared distances, in either side's matrix (the other colour's rows and columns infinite), are equal, finite
    and within max_dist^2, k = min(5, n - 1).  Equal distances inside the k nearest leave the set of neighbours as it is."""
    sys.path.insert(0, str(ROOT / "tests"))
    import sort_support as ss

    refharness.load()
    from fsd_path_planning.utils.math_utils import my_cdist_sq_euclidean

    def knn_tie(xyt):
        n = len(xyt)
        k = min(5, n - 1)
        if n < 3 or k >= n - 1:
            return False
        xy = np.ascontiguousarray(xyt[:, :2], dtype=float)
        for other in (1.0, 2.0):
            d = my_cdist_sq_euclidean(xy, xy).copy()
            np.fill_diagonal(d, np.inf)
            d[xyt[:, 2] == other, :] = np.inf
            d[:, xyt[:, 2] == other] = np.inf
            d.sort(axis=1)
            if ((d[:, k - 1] == d[:, k]) & np.isfinite(d[:, k]) & (d[:, k] <= 6.5 * 6.5)).any():
                return True
        return False

    named = []
    for name, _obs, lo, hi in ss.all_pairs():
        named += [(name + " below", lo), (name + " above", hi)]
    named += ss.on_threshold() + [(n + ", mirrored", ss.mirrored(c)) for n, c in ss.on_threshold()] + ss.structural()
    F = len(named)
    out = dict(names=np.array([n for n, _c in named]), sort_ok=np.zeros(F, bool), exc=np.array([""] * F, dtype="U24"),
               n_left=np.zeros(F, np.int32), n_right=np.zeros(F, np.int32), left_idx=np.full((F, MAX_LEN), -1, np.int32),
               right_idx=np.full((F, MAX_LEN), -1, np.int32), first_k_left=np.full((F, 2), -1, np.int32), first_k_right=np.full((F, 2), -1, np.int32),
               first_k_tie=np.zeros((F, 2), bool), knn_tie=np.zeros(F, bool), n_configs_left=np.zeros(F, np.int32), n_configs_right=np.zeros(F, np.int32),
               best_cost_left=np.zeros(F), best_cost_right=np.zeros(F))
    off, cones, poses = ss.as_batch([c for _n, c in named])
    out.update(offsets=off, cones=cones, poses=poses)
    for k, (_name, (xyt, pose)) in enumerate(named):
        with np.errstate(all="ignore"):
            r = refharness.run_frame(xyt, pose)
        out["exc"][k] = "" if r["status"] == "ok" else r["status"]
        out["knn_tie"][k] = knn_tie(xyt)
        for si, (side, t) in enumerate((("left", 2), ("right", 1))):
            out["first_k_tie"][k, si] = bool((r.get("first_k_tie") or {}).get(t, False))
            fk = (r.get("first_k") or {}).get(t)
            if fk is not None:
                out[f"first_k_{side}"][k, : len(fk)] = fk
            costs = r.get(f"{side}_costs")
            if costs is not None and len(costs):
                out[f"n_configs_{side}"][k], out[f"best_cost_{side}"][k] = len(costs), costs[0]
        if "left_config" not in r:
            continue
        out["sort_ok"][k] = True
        lc, rc = np.asarray(r["left_config"]), np.asarray(r["right_config"])
        lc, rc = lc[lc != -1], rc[rc != -1]
        out["n_left"][k], out["n_right"][k] = len(lc), len(rc)
        out["left_idx"][k, : len(lc)], out["right_idx"][k, : len(rc)] = lc, rc
    tie = out["knn_tie"] | out["first_k_tie"].any(axis=1)
    out["tie_names"] = out["names"][tie]
    np.savez_compressed(HERE / "sort_constructed.npz", **out)
    print("sort_constructed frames", F, "sorted", int(out["sort_ok"].sum()), "exc", sorted(set(out["exc"].tolist()) - {""}), "argsort ties", int(tie.sum()))


if __name__ == "__main__" and "--sort-constructed-only" in sys.argv:
    sort_constructed_golden()


def path_constructed_golden():
    """The constructed inputs of the path stage (tests/path_support.py, families A-E: the canonical member of every case and of every
    threshold pair, standard shapes) through the reference's CalculatePath stage class, a fresh object per frame, built with the
    case's parameters and handed the case's previous path where it has one -> path_constructed.npz: the names, the exception's class
    where the reference raises, and the path (distinct paths once).  Data only; the inputs are rebuilt from the names by the test."""
    sys.path.insert(0, str(ROOT / "tests"))
    import path_support as ps

    refharness.load()
    from fsd_path_planning.calculate_path.core_calculate_path import CalculatePath, PathCalculationInput

    defaults = dict(smoothing=0.2, predict_every=0.1, max_deg=3, maximal_distance_for_valid_path=5, mpc_path_length=20, mpc_prediction_horizon=40)
    cases = [c for fam in "ABCDE" for c in ps.everything()[fam][0] if ps.canonical(c)]
    F = len(cases)
    out = dict(names=np.array([c.name for c in cases]), ok=np.zeros(F, bool), exc=np.array([""] * F, dtype="U24"), path=np.full((F, 40, 4), np.nan))
    assert len(set(out["names"].tolist())) == F
    for k, c in enumerate(cases):
        stage = CalculatePath(**{**defaults, **c.prm})
        if c.prev is not None:
            stage.previous_paths = [np.array(c.prev)]
        stage.set_new_input(PathCalculationInput(c.lv, c.rv, c.l2r.astype(np.int64), c.r2l.astype(np.int64), c.pose[:2], c.pose[2:], c.gpath))
        try:
            with np.errstate(all="ignore"):
                path, _centers = stage.run_path_calculation()
        except Exception as e:  # noqa: BLE001 (which class is part of the fixture)
            out["exc"][k] = type(e).__name__
            continue
        out["ok"][k] = True
        out["path"][k, : len(path)] = path
    # cases that share their centre points share their path: each distinct path once (paths), and which one a frame has (path_of)
    # (and of each path the rows `rows`: every second one and the last — the fixture's size; a decision that flips moves every row)
    out["rows"] = np.unique(np.concatenate([np.arange(0, 40, 2), [39]]))  # (all 40 rows of all cases: 181 KB)
    uniq, inverse = np.unique(out.pop("path")[:, out["rows"]].reshape(F, -1), axis=0, return_inverse=True, equal_nan=True)
    out["paths"], out["path_of"] = uniq.reshape(-1, len(out["rows"]), 4), inverse.astype(np.int32).reshape(F)
    np.savez_compressed(HERE / "path_constructed.npz", **out)
    print("path_constructed frames", F, "distinct paths", len(uniq), "ok", int(out["ok"].sum()), "exc", sorted(set(out["exc"].tolist()) - {""}))


if __name__ == "__main__" and "--path-constructed-only" in sys.argv:
    path_constructed_golden()


def skidpad_constructed_golden():
    """The constructed inputs of the skidpad stage (tests/skidpad_constructed_support.py, families A-F: every case and both members of
    every threshold pair in the canonical frame), each through a reference PathPlanner(MissionTypes.skidpad) of its own, step by step,
    exceptions caught the way a caller would -> skidpad_constructed.npz: the names, the inputs (cones as CSR over (case, step), poses),
    per step the exception's class where the reference raises, the path, relocalized, the relocalization information and
    index_along_path as the planner holds it after the step.  Data only."""
    sys.path.insert(0, str(ROOT / "tests"))
    import skidpad_constructed_support as sc

    m = refharness.load()
    cases = [c for c in sc.build()[0] if c.frame == "canonical"]
    steps = [(k, s) for k, c in enumerate(cases) for s in range(c.n_steps)]
    F = len(steps)
    out = dict(names=np.array([c.name for c in cases]), case_of=np.array([k for k, _ in steps], np.int32), step_of=np.array([s for _, s in steps], np.int32),
               ok=np.zeros(F, bool), exc=np.array([""] * F, dtype="U24"), path=np.full((F, 40, 4), np.nan), relocalized=np.zeros(F, bool),
               info=np.full((F, 3), np.nan), index_along_path=np.zeros(F, np.int32), poses=np.zeros((F, 4)))
    cones, off = [], [0]
    f = 0
    for c in cases:
        pp = m["PathPlanner"](m["MissionTypes"].skidpad)
        for xyt, pose in c.steps:
            by_type = [xyt[:, :2].copy()] + [np.zeros((0, 2)) for _ in range(4)]
            try:
                with np.errstate(all="ignore"):
                    out["path"][f] = pp.calculate_path_in_global_frame(by_type, pose[:2].copy(), pose[2:].copy())
                out["ok"][f] = True
            except Exception as e:  # noqa: BLE001 (which class is part of the fixture)
                out["exc"][f] = type(e).__name__
            ri = pp.relocalization_info
            out["relocalized"][f] = ri is not None
            if ri is not None:
                out["info"][f] = [ri.translation[0], ri.translation[1], ri.rotation]
            out["index_along_path"][f] = pp.pathing.index_along_path
            out["poses"][f] = pose
            cones.append(xyt)
            off.append(off[-1] + len(xyt))
            f += 1
    out["offsets"], out["cones"] = np.array(off, np.int32), np.concatenate(cones)
    np.savez_compressed(HERE / "skidpad_constructed.npz", **out)
    print("skidpad_constructed cases", len(cases), "steps", F, "ok", int(out["ok"].sum()), "exc", sorted(set(out["exc"].tolist()) - {""}),
          "relocalized", int(out["relocalized"].sum()))


if __name__ == "__main__" and "--skidpad-constructed-only" in sys.argv:
    skidpad_constructed_golden()
