"""Fixture of the sorting stage's search history (include/fsdp.h fsdp_sort_batch_history): what the REFERENCE records with
store_all_end_configurations=True (end_configurations.py:358-361,411-429; calc_scores_and_end_configurations(...,
return_history=True), find_configs_and_scores.py:41,96) — every configuration the depth-first search visited, in visiting
order, and whether it was an end configuration — plus, per visited row, the popped cone's neighbours and for each the first
predicate of neighbor_bool_mask_can_be_added_to_attempt (:108-223) that rejects it.

    python tests/golden/make_golden_history.py      (build container: needs the reference, refharness.py)

Frames: the 65 frames of sort_ranked.npz under the same source / source_frame names, frames 0 and 8 of big_frames.npz (300 and
600 cones: the big route) and up to four frames of the other fixtures on which the reference raises (exc != "ok").  The inputs
are stored again so that the file stands alone.  Writes tests/golden/sort_history.npz: per frame k and side s (0 = left,
1 = right) n_rows[k, s], target_length[k, s] and the rows [row_off[k, s], row_off[k, s] + n_rows[k, s]) of rows (R, 12; -1
padded), is_end (R,), cand (R, 5; -1 padded) and verdict (R, 5; 0xFF padded).  searched[k, s]: the reference reached the side's
search (a frame it raises on while evaluating the left side never searches the right one).  A side whose search leaves no
configuration (NoPathError, which the reference catches itself) keeps its rows: they are captured from
_impl_find_all_end_configurations, before find_all_end_configurations raises.

The codes are computed row by row with the reference's own functions called one at a time (my_in1d,
calculate_mask_within_ellipse, mask_second_in_attempt_is_on_right_vehicle_side,
check_if_neighbor_lies_between_last_in_attempt_and_candidate, angle_difference, vec_angle_between,
lines_segments_intersect_indicator) with this script's glue between them; on every row the script asserts that code 0 <=>
neighbor_bool_mask_can_be_added_to_attempt returns True for the neighbour, which pins the glue to the reference.
knn_tie[k]: refharness.knn_boundary_tie — the reference's adjacency on such a frame is its unstable argsort's.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))

import refharness  # noqa: E402

MAX_LEN, MAX_NEIGHBORS = 12, 5
BIG_FRAMES = (0, 8)
SIZE_CAP = 256 * 1024
KNN_TIE_CAP = 19  # counted on sort_ranked.npz: 19 of its 65 frames, all of them from `scenarios`


def verdicts(ec, trace, cone_type, attempt, pos, neighbors, thr_dir, thr_abs, car_pos, car_dir, car_size):
    """the first rejecting predicate per neighbour, in the order of end_configurations.py:108-223 (0: none)"""
    from fsd_path_planning.utils.cone_types import ConeTypes

    n = len(neighbors)
    code = np.zeros(n, np.uint8)
    car_dir_n = car_dir / np.linalg.norm(car_dir)
    pts = trace[neighbors]
    in_attempt = ec.my_in1d(neighbors, attempt[: pos + 1])  # :126
    ellipse = ec.calculate_mask_within_ellipse(trace, attempt, pos, pts) if pos >= 1 else np.ones(n, bool)  # :129-132
    side = ec.mask_second_in_attempt_is_on_right_vehicle_side(cone_type, car_pos, car_dir_n, pts) if pos == 0 else np.ones(n, bool)  # :134-141
    for i in range(n):
        if in_attempt[i]:
            code[i] = 1
            continue
        if not ellipse[i]:
            code[i] = 2
            continue
        if not side[i]:
            code[i] = 3
            continue
        mask = np.ones(n, bool)
        ec.check_if_neighbor_lies_between_last_in_attempt_and_candidate(trace, attempt, pos, neighbors, mask, i, neighbors[i])  # :152-160
        if not mask[i]:
            code[i] = 4
            continue
        cand = trace[neighbors[i]]
        if pos >= 1:
            second_to_last, last = trace[attempt[pos - 1]], trace[attempt[pos]]
            e1, e2 = last - second_to_last, cand - last
            angle_1, angle_2 = np.arctan2(e1[1], e1[0]), np.arctan2(e2[1], e2[0])
            difference = ec.angle_difference(angle_2, angle_1)
            length = np.linalg.norm(e2)
            if np.abs(difference) > thr_abs:  # :184
                code[i] = 5
                continue
            if cone_type == ConeTypes.LEFT:  # :186-189
                ok = difference < thr_dir or length < 4.0
            else:
                ok = difference > -thr_dir or length < 4.0
            if not ok:
                code[i] = 6
                continue
            if pos >= 2:  # :194-205
                e0 = second_to_last - trace[attempt[pos - 2]]
                difference_2 = ec.angle_difference(angle_1, np.arctan2(e0[1], e0[0]))
                if np.sign(difference) != np.sign(difference_2) and np.abs(difference - difference_2) > 1.3:
                    code[i] = 7
                    continue
        if pos == 1:  # :207-211
            if not ec.vec_angle_between(car_dir, cand - trace[attempt[0]]) < np.pi / 2:
                code[i] = 8
                continue
        car_start, car_end = car_pos - car_dir_n * car_size / 2, car_pos + car_dir_n * car_size
        if ec.lines_segments_intersect_indicator(trace[attempt[pos]], cand, car_start, car_end):  # :213-221
            code[i] = 9
    return code


def capture_frame(xyt, pose):
    """-> (exception name or "ok", [per side: dict or None])"""
    refharness.load()
    import fsd_path_planning.sorting_cones.trace_sorter.end_configurations as ec
    import fsd_path_planning.sorting_cones.trace_sorter.find_configs_and_scores as fcs

    orig_find, orig_impl = fcs.find_all_end_configurations, ec._impl_find_all_end_configurations
    seen = []

    def find_wrapper(*args, **kw):
        kw["store_all_end_configurations"] = True
        return orig_find(*args, **kw)

    def impl_wrapper(*args):
        out = orig_impl(*args)
        assert args[12] is True
        seen.append((args, out[1]))
        return out

    fcs.find_all_end_configurations = find_wrapper
    ec._impl_find_all_end_configurations = impl_wrapper
    try:
        r = refharness.run_frame(xyt, pose)
    finally:
        fcs.find_all_end_configurations = orig_find
        ec._impl_find_all_end_configurations = orig_impl
    sides = [None, None]
    for args, (all_cfg, is_end) in seen:
        trace, cone_type, _start, flat, borders, target, thr_dir, thr_abs, _first_k, car_pos, car_dir, car_size, _store = args
        s = 0 if int(cone_type) == 2 else 1
        assert sides[s] is None and all_cfg.shape[1] == target and len(all_cfg) == len(is_end) >= 1
        R = len(all_cfg)
        rows = np.full((R, MAX_LEN), -1, np.int16)
        rows[:, :target] = all_cfg
        cand = np.full((R, MAX_NEIGHBORS), -1, np.int16)
        verdict = np.full((R, MAX_NEIGHBORS), 0xFF, np.uint8)
        for r_ in range(R):
            attempt = np.ascontiguousarray(all_cfg[r_])
            pos = int((attempt >= 0).sum()) - 1
            node = int(attempt[pos])
            nb = flat[borders[node] : borders[node + 1]]
            assert len(nb) <= MAX_NEIGHBORS and (np.diff(nb) > 0).all()
            code = verdicts(ec, trace, cone_type, attempt, pos, nb, thr_dir, thr_abs, car_pos, car_dir, car_size)
            mask = ec.neighbor_bool_mask_can_be_added_to_attempt(trace, cone_type, attempt, pos, nb, thr_dir, thr_abs, car_pos, car_dir, car_size)
            assert np.array_equal(code == 0, mask), (r_, code, mask)  # the glue above against the reference's own function
            assert bool(is_end[r_]) == (pos == target - 1 or not mask.any())
            cand[r_, : len(nb)] = nb
            verdict[r_, : len(nb)] = code
        sides[s] = dict(target=int(target), rows=rows, is_end=np.asarray(is_end, np.uint8), cand=cand, verdict=verdict)
    return r["status"], sides, r


def raising_frames(limit=4):
    """up to `limit` frames of the existing fixtures on which the reference raises"""
    refharness.load()
    out = []
    for f in sorted(HERE.glob("*.npz")):
        # (fixtures recorded with the default parameters and finite inputs; the sequence and path fixtures hold no single frames)
        if f.name.startswith(("sort_", "params_", "nonfinite_", "sequence_", "path_")):
            continue
        g = np.load(f)
        if not all(k in g.files for k in ("exc", "offsets", "cones", "poses")) or g["cones"].ndim != 2 or g["cones"].shape[1] != 3:
            continue
        # (no frame with a nearest-neighbour tie: those are skipped by the comparison, and the count of them is pinned below)
        hits = [int(k) for k in np.flatnonzero(~np.isin(g["exc"], ("", "ok"))) if g["offsets"][k + 1] - g["offsets"][k] <= 255
                and not refharness.knn_boundary_tie(g["cones"][g["offsets"][k] : g["offsets"][k + 1]])]
        out += [(f.stem, k) for k in hits[:2]]  # (two a file: more than one source)
    return out[:limit]


def main():
    ranked = np.load(HERE / "sort_ranked.npz")
    frames = [(str(n), int(k)) for n, k in zip(ranked["source"], ranked["source_frame"])]
    assert len(frames) == 65
    frames += [("big_frames", k) for k in BIG_FRAMES]
    raising = raising_frames()
    print(f"frames of the existing fixtures on which the reference raises: {raising if raising else 'none'}")
    frames += raising
    out = {k: [] for k in ("source", "source_frame", "cones", "poses", "exc", "knn_tie", "n_rows", "target_length", "searched", "no_config")}
    parts = {k: [] for k in ("rows", "is_end", "cand", "verdict")}
    files = {}
    for name, k in frames:
        g = files.setdefault(name, np.load(HERE / f"{name}.npz"))
        xyt = np.ascontiguousarray(g["cones"][g["offsets"][k] : g["offsets"][k + 1]], dtype=np.float64)
        pose = np.ascontiguousarray(g["poses"][k], dtype=np.float64)
        exc, sides, r = capture_frame(xyt, pose)
        n_rows, target, searched, no_config = [0, 0], [0, 0], [False, False], [False, False]
        for s, side in enumerate(sides):
            if side is None:
                continue
            n_rows[s], target[s], searched[s] = len(side["rows"]), side["target"], True
            # the search ran and the post filters left nothing: the reference returns no result for the side
            no_config[s] = exc == "ok" and r.get(("left", "right")[s] + "_configs") is None
            for key in parts:
                parts[key].append(side[key])
        for key, v in (("source", name), ("source_frame", k), ("cones", xyt), ("poses", pose), ("exc", exc), ("n_rows", n_rows),
                       ("target_length", target), ("searched", searched), ("no_config", no_config), ("knn_tie", refharness.knn_boundary_tie(xyt))):
            out[key].append(v)
    n_rows = np.array(out["n_rows"], np.int32)
    row_off = np.concatenate([[0], np.cumsum(n_rows.ravel())])[:-1].reshape(-1, 2).astype(np.int32)
    offsets = np.zeros(len(out["cones"]) + 1, np.int32)
    offsets[1:] = np.cumsum([len(c) for c in out["cones"]])
    res = dict(source=np.array(out["source"]), source_frame=np.array(out["source_frame"], np.int32), offsets=offsets,
               cones=np.concatenate(out["cones"]), poses=np.array(out["poses"]), exc=np.array(out["exc"]), knn_tie=np.array(out["knn_tie"]),
               n_rows=n_rows, row_off=row_off, target_length=np.array(out["target_length"], np.int32), searched=np.array(out["searched"]),
               no_config=np.array(out["no_config"]), **{k: np.concatenate(v) for k, v in parts.items()})
    f = HERE / "sort_history.npz"
    np.savez_compressed(f, **res)
    size = f.stat().st_size
    ends = np.array([[int(res["is_end"][row_off[k, s] : row_off[k, s] + n_rows[k, s]].sum()) for s in range(2)] for k in range(len(n_rows))])
    hist = np.bincount(res["verdict"][res["verdict"] != 0xFF], minlength=10)
    print(f"{f.name}: {len(n_rows)} frames, {int(n_rows.sum())} rows, at most {n_rows.max()} per side, {int((ends > 1).sum())} sides with more than one end row, "
          f"{int(res['no_config'].sum())} sides whose search leaves no configuration, {int(res['knn_tie'].sum())} frames with a nearest-neighbour tie, "
          f"{size} bytes; exceptions: {sorted(set(res['exc'].tolist()))}; codes 0..9: {hist.tolist()}")
    print(f"the sources hold a side whose search leaves no configuration: {bool(res['no_config'].any())}")
    assert size < SIZE_CAP, size
    assert int((ends > 1).sum()) >= 8 and n_rows.max() >= 200
    big = res["source"] == "big_frames"
    assert big.sum() == 2 and (n_rows[big] > 0).all()  # both big frames traced, on both sides
    tie = res["knn_tie"]
    assert tie.sum() <= KNN_TIE_CAP and (res["source"][tie] == "scenarios").all()


if __name__ == "__main__":
    main()
