"""JSON replay loader + timing CLI — this build's counterpart of the reference's only benchmark harness
(demo/json_demo.py: load_data_json :255-275, select_mission_by_filename :38-51, warm-up :89-94, timed per-frame
loop :103-131).  Same file schema: a list of {"car_position":[x,y], "car_direction":[dx,dy], "slam_cones":[5 lists of [x,y]]}.

  python -m fsd_path_planning_amd.replay --data-path fsg_19_2_laps.json [--remove-color-info] [--batched] [--output-path out.npz]
                                          [--experimental-performance-improvements]  (per-frame mode only)
                                          [--ranked K]  (per frame: decision margins and deciding cost terms of the sorting stage)
                                          [--history ROWS]  (per side: where the sorting stage's searches went and what rejected candidates)

Two replay modes:
  per-frame : one PathPlanner, one calculate_path_in_global_frame call per frame, wall-clock per call (what the
              reference's demo measures; for the skidpad mission this is the stateful sequence);
  --batched : the frames of the recording as a stream of batches of independent frames (fresh-planner semantics per
              frame; trackdrive/autocross recordings only), several batches in flight (fsdp_submit / fsdp_collect);
              with --stateful the frames that read the previous path are planned again in order with the path their
              predecessor left: the per-frame replay's results at the batched replay's speed.
"""
from __future__ import annotations

import argparse
import json
import time
from pathlib import Path
from typing import List, Tuple

import numpy as np

from .planner import ConeTypes, MissionTypes, PathPlanner, pack_frames


def select_mission_by_filename(filename: str) -> MissionTypes:
    """"skidpad" in the name -> skidpad, "accel" -> acceleration, else trackdrive (json_demo.py:38-51)."""
    if "skidpad" in filename:
        return MissionTypes.skidpad
    if "accel" in filename:
        return MissionTypes.acceleration
    return MissionTypes.trackdrive


class Recording:
    """A JSON recording in the layout the C ABI takes (include/fsdp.h): one (N, 3) [x, y, type] cone array for all frames
    in the reference's flatten order (UNKNOWN, RIGHT, LEFT, ORANGE_SMALL, ORANGE_BIG — core_trace_sorter.py:37-54), CSR
    offsets (F + 1,) and poses (F, 4) [px, py, dx, dy].  File schema (what demo/json_demo.py reads): a list of frames
    {"car_position": [x, y], "car_direction": [dx, dy], "slam_cones": [5 lists of [x, y], one per ConeTypes value]}."""

    N_TYPES = len(ConeTypes)

    def __init__(self, offsets: np.ndarray, cones: np.ndarray, poses: np.ndarray):
        self.offsets, self.cones, self.poses = offsets, cones, poses

    @classmethod
    def from_json(cls, data_path: Path) -> "Recording":
        frames = json.loads(Path(data_path).read_text())
        counts = np.array([[len(lst) for lst in f["slam_cones"]] for f in frames], dtype=np.int64).reshape(len(frames), cls.N_TYPES)
        offsets = np.zeros(len(frames) + 1, dtype=np.int32)
        np.cumsum(counts.sum(axis=1), out=offsets[1:])
        cones = np.empty((int(offsets[-1]), 3))
        poses = np.empty((len(frames), 4))
        for k, f in enumerate(frames):
            poses[k, :2] = f["car_position"]
            poses[k, 2:] = f["car_direction"]
            at = int(offsets[k])
            for cone_type, lst in enumerate(f["slam_cones"]):
                if lst:
                    cones[at:at + len(lst), :2] = lst
                    cones[at:at + len(lst), 2] = cone_type
                    at += len(lst)
        return cls(offsets, cones, poses)

    def without_color(self) -> "Recording":
        """Every cone UNKNOWN.  The cones of a frame are already stacked in type order, which is the order the reference's
        colour stripping leaves them in (json_demo.py:266-273), so only the type column changes."""
        cones = self.cones.copy()
        cones[:, 2] = float(ConeTypes.UNKNOWN)
        return Recording(self.offsets, cones, self.poses)

    def __len__(self) -> int:
        return len(self.poses)

    def frame_cones_by_type(self, k: int) -> List[np.ndarray]:
        """Frame k as the five per-type (n, 2) arrays `calculate_path_in_global_frame` takes."""
        block = self.cones[self.offsets[k]:self.offsets[k + 1]]
        return [block[block[:, 2] == t, :2] for t in range(self.N_TYPES)]


def load_data_json(data_path: Path, remove_color_info: bool = False) -> Tuple[np.ndarray, np.ndarray, List[List[np.ndarray]]]:
    """(positions (F, 2), directions (F, 2), per frame the five per-type cone arrays) — the tuple the reference's loader
    returns, cut out of a `Recording`."""
    rec = Recording.from_json(data_path)
    if remove_color_info:
        rec = rec.without_color()
    return rec.poses[:, :2].copy(), rec.poses[:, 2:].copy(), [rec.frame_cones_by_type(k) for k in range(len(rec))]


def replay_per_frame(mission, positions, directions, observations, device=None, experimental_performance_improvements: bool = False):
    flag = experimental_performance_improvements  # the reference's sorting cache (json_demo.py:68,75)
    warm = PathPlanner(mission, flag, device=device)  # warm-up on a throw-away planner (json_demo.py:89-94)
    warm.calculate_path_in_global_frame(observations[0], positions[0], directions[0])
    planner = PathPlanner(mission, flag, device=device)
    paths, times, reloc_frame = [], [], None
    for i, (p, d, c) in enumerate(zip(positions, directions, observations)):
        if reloc_frame is None and planner.relocalization_info is not None:
            reloc_frame = i
        t0 = time.perf_counter()
        paths.append(planner.calculate_path_in_global_frame(c, p, d))
        times.append(time.perf_counter() - t0)
    return np.array(paths), np.array(times), reloc_frame, planner.relocalization_info


def replay_batched(mission, positions, directions, observations, device=None, repeats: int = 5, batch_frames: int = 4096, depth: int = 4,
                   devices=None):
    """The recording as a stream of batches of `batch_frames` frames, `depth` of them in flight (fsdp_submit /
    fsdp_collect: a batch's transfers run under the other batches' kernels; page-locked buffers).  Returns the results of
    all frames in recording order and the seconds one replay of the whole recording took (host buffers to host buffers).
    devices (a list of GPU indices or "all"): every batch is cut into contiguous frame ranges, one per GPU, all driven from
    this process (multi.MultiPlanner.plan_stream) — the same bytes."""
    from . import _capi

    if devices is not None:
        from .multi import MultiPlanner

        mp = MultiPlanner(None if devices == "all" else devices, mission=int(mission), overlap=depth)
        frames = list(zip(observations, positions, directions))
        chunks = [pack_frames(frames[lo:lo + batch_frames]) for lo in range(0, len(frames), batch_frames)]
        got = list(mp.plan_stream(chunks))  # warm-up
        t0 = time.perf_counter()
        for _ in range(repeats):
            got = list(mp.plan_stream(chunks))
        sec = (time.perf_counter() - t0) / repeats
        mp.close()
        return (np.concatenate(got) if got else np.zeros(0, _capi.RESULT_DTYPE)), sec
    planner = PathPlanner(mission, device=device)
    ctx = planner._ctx
    frames = list(zip(observations, positions, directions))
    chunks = []
    for lo in range(0, len(frames), batch_frames):
        off, cones, poses = pack_frames(frames[lo:lo + batch_frames])
        chunks.append((_capi.pinned_copy(off, np.int32), _capi.pinned_copy(cones, np.float64), _capi.pinned_copy(poses, np.float64),
                       _capi.pinned_empty(len(poses), ctx.result_dtype)))
    depth = max(1, min(depth, len(chunks)))
    ctx.set_overlap(depth)

    def one_replay():
        inflight = []
        for off, cones, poses, out in chunks:
            if len(inflight) == ctx.ticket_capacity:
                ctx.collect(inflight.pop(0))
            inflight.append(ctx.submit(off, cones, poses, out=out))
        for t in inflight:
            ctx.collect(t)

    one_replay()  # warm-up
    t0 = time.perf_counter()
    for _ in range(repeats):
        one_replay()
    sec = (time.perf_counter() - t0) / repeats
    res = np.concatenate([np.array(c[3]) for c in chunks]) if chunks else np.zeros(0, ctx.result_dtype)
    ctx.set_overlap(1)
    return res, sec


def replay_ranked(mission, positions, directions, observations, top_k: int, device=None, batch_frames: int = 4096):
    """The recording's frames as independent frames through fsdp_sort_batch_ranked: per frame and side (left, right) the
    decision margin (c1 - c0) / max(|c0|, 1e-300) of the sorting stage's choice (inf: fewer than two candidates) and the
    deciding term — the column of the seven weighted costs (cost_function.py:287-296) in which the runner-up differs most from
    the winner, -1 without a runner-up.  Returns (status (F,), counts (F, 2), margins (F, 2), deciding (F, 2))."""
    from . import _capi

    planner = PathPlanner(mission, device=device)
    ctx = planner._ctx
    frames = list(zip(observations, positions, directions))
    k = max(2, int(top_k))
    status, counts, margins, deciding = [], [], [], []
    for lo in range(0, len(frames), batch_frames):
        off, cones, poses = pack_frames(frames[lo:lo + batch_frames])
        res, cnt, _cfg, costs, terms = ctx.sort_batch_ranked(off, cones, poses, top_k=k)
        m = _capi.decision_margin(costs)
        with np.errstate(invalid="ignore"):
            diff = terms[:, :, 1, :] - terms[:, :, 0, :]
        d = np.where(np.isfinite(m), np.argmax(np.nan_to_num(diff, nan=-np.inf), axis=-1), -1)
        status.append(res["status"].copy())
        counts.append(cnt)
        margins.append(m)
        deciding.append(d)
    cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dt)  # noqa: E731
    return cat(status, 0, np.int32), cat(counts, (0, 2), np.int32), cat(margins, (0, 2), np.float64), cat(deciding, (0, 2), np.int64)


def replay_history(mission, positions, directions, observations, rows_cap: int, device=None, batch_frames: int = 4096):
    """The recording's frames as independent frames through fsdp_sort_batch_history: where every side's depth-first search went
    and which predicate turned each neighbour away.  Returns (status (F,), n_rows (F, 2), no_configuration (F, 2) bool — the side
    was searched and the frame has no configuration for it — and histograms (F, 2, 10): how often each CandVerdict code occurred in
    the side's stored rows).  A side that visited more than rows_cap rows contributes its first rows_cap to the histogram."""
    planner = PathPlanner(mission, device=device)
    ctx = planner._ctx
    frames = list(zip(observations, positions, directions))
    # (the calls' arrays are (frames, 2, rows_cap, ...) at 73 bytes a row: batches of at most 2^18 rows a side keep them below 40 MB)
    step = max(1, min(int(batch_frames), (1 << 18) // max(1, int(rows_cap))))
    status, n_rows, none_left, hist = [], [], [], []
    for lo in range(0, len(frames), step):
        off, cones, poses = pack_frames(frames[lo:lo + step])
        res, h = ctx.sort_batch_history(off, cones, poses, rows_cap=int(rows_cap))
        v = h["verdict"].reshape(len(poses), 2, -1)
        hist.append(np.stack([(v == code).sum(axis=-1) for code in range(10)], axis=-1))
        status.append(res["status"].copy())
        n_rows.append(h["n_rows"])
        none_left.append((h["n_rows"] > 0) & (np.stack([res["n_configs_left"], res["n_configs_right"]], axis=-1) == 0))
    cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dt)  # noqa: E731
    return cat(status, 0, np.int32), cat(n_rows, (0, 2), np.int32), cat(none_left, (0, 2), bool), cat(hist, (0, 2, 10), np.int64)


FB_READ_PREVIOUS = 1 | 2 | 4 | 8  # path_fallback bits of the branches that read previous_paths[-1] (include/fsdp.h; the frames fsdp_plan_sequence plans again)


def _replay_recordings_in_flight(ctxs, chunked, chunked_ids=None):
    """Recordings (each a list of consecutive chunks (offsets, cones, poses) of one planner) as sequence tickets
    (fsdp_submit_sequence) over the contexts `ctxs`: as many chunks in flight as the contexts' ticket capacities allow, a
    recording's next chunk submitted — to the context that planned the previous one — as soon as that one is collected, with the
    path it left (final_prev -> initial_prev).  chunked_ids: per recording the chunks' path ids (fsdp_submit_sequence_paths), or
    None.  -> (per recording the list of its chunks' results, frames planned again)"""
    from ._capi import pinned_empty

    results = [[None] * len(chunks) for chunks in chunked]
    # two page-locked final_prev rows per recording, taken in turn: the one chunk k left is read by chunk k + 1 while that writes its own
    finals = [[pinned_empty((1, ctxs[0].shapes.path_points, 4)) for _ in range(2 if len(chunks) > 1 else 1)] for chunks in chunked]
    room = [c.ticket_capacity for c in ctxs]
    waiting = [r for r, chunks in enumerate(chunked) if chunks]
    inflight, again = [], 0

    def start(r, k, g, prev):
        inflight.append((g, r, k, ctxs[g].submit_sequence(*chunked[r][k], 1, initial_prev=prev, final_prev_out=finals[r][k % len(finals[r])],
                                                          path_ids=None if chunked_ids is None else chunked_ids[r][k])))
        room[g] -= 1

    while waiting or inflight:
        while waiting and max(room) > 0:
            start(waiting.pop(0), 0, room.index(max(room)), None)
        g, r, k, ticket = inflight.pop(0)
        res, final, n = ctxs[g].collect(ticket)
        room[g] += 1
        again += n
        results[r][k] = res
        if k + 1 < len(chunked[r]):
            start(r, k + 1, g, final)
    return results, again


def replay_stateful_batched(mission, positions, directions, observations, device=None, batch_frames: int = 4096, depth: int = 4,
                            cache: bool = False, multi=None, recordings=None, path_ids=None, path_table=None):
    """The recording as ONE planner sees it — consecutive frames chain through previous_paths[-1] (core_calculate_path.py:
    572-573), which the reference reads in its fallbacks only (:202-203, 218-221, 235-236, 531-536, 564-570) — at the speed
    of a batched replay: the recording cut into consecutive calls of `batch_frames` steps of fsdp_plan_sequence (one planner),
    each handing the path it leaves to the next (final_prev -> initial_prev).  A call plans all its frames as independent
    frames first and then, on the device, the frames that did read the previous path once more, in order, with the path
    their predecessor really left (a frame the reference raises on leaves none).  Returns the results in recording order, the
    seconds of the replay and the number of frames planned again.  (depth: kept for callers of the earlier form, which
    streamed the independent frames; a sequence call is one pass.)
    cache: the planner of a recording made with experimental_performance_improvements=True (fsdp_plan_sequence_cached: the
    sorting cache chained on the device as well, its entry carried from call to call by the context).
    recordings: a list of (positions, directions, observations) INSTEAD of the one recording (pass None for those three) — every
    recording its own fresh planner, their chunks kept in flight as sequence tickets up to the ticket capacity (a blocking call
    per chunk leaves the GPU idle between calls); returns a list of result arrays.  multi: a MultiPlanner whose contexts share
    the recordings (several contexts or GPUs; also for one recording, whose chunks then simply run as tickets on the first
    context).  Neither goes with cache: the cache-on sequence call has no ticket form.
    path_ids: one int32 id per frame of the recording (with recordings: a list of such arrays) — the entry of the path table the
    frame follows, or -1 for a frame that plans from its cones (fsdp_plan_sequence_paths: a car that maps its track part-way through
    the log).  path_table: the list of (k, 2) polylines the ids name, set on the contexts the replay creates; a MultiPlanner's
    contexts keep the table its caller set (MultiPlanner.set_global_path_table) unless one is given here.  Not with cache."""
    if path_ids is not None and cache:
        raise ValueError("replay_stateful_batched: path ids do not go with the sorting cache (fsdp_plan_sequence_cached takes none)")
    ids_of = None
    if path_ids is not None:
        per_rec = list(path_ids) if recordings is not None else [path_ids]
        lens = [len(r[0]) for r in recordings] if recordings is not None else [len(positions)]
        per_rec = [np.ascontiguousarray(i, dtype=np.int32) for i in per_rec]
        if [i.shape for i in per_rec] != [(m,) for m in lens]:
            raise ValueError("replay_stateful_batched: path_ids holds one id per frame of every recording")
        ids_of = [[i[lo:lo + batch_frames] for lo in range(0, len(i), batch_frames)] for i in per_rec]
    if multi is not None or recordings is not None:
        if cache:
            raise ValueError("replay_stateful_batched: the sorting cache has no ticket form (cache=True goes with one recording and no MultiPlanner)")
        from ._capi import pinned_copy

        many = recordings if recordings is not None else [(positions, directions, observations)]
        own = None if multi is not None else PathPlanner(mission, False, device=device)
        ctxs = multi.ctx if multi is not None else [own._ctx]
        if path_table is not None:
            for c in ctxs:
                c.set_global_path_table(path_table)
        chunked = []
        for pos, dirs, obs in many:
            frames = list(zip(obs, pos, dirs))
            packed = [pack_frames(frames[lo:lo + batch_frames]) for lo in range(0, len(frames), batch_frames)]
            chunked.append([(pinned_copy(o, np.int32), pinned_copy(c), pinned_copy(p)) for o, c, p in packed])  # (page-locked: read in place)
        if chunked and chunked[0]:
            for c in ctxs:
                c.plan_sequence(*chunked[0][0], 1, path_ids=None if ids_of is None else ids_of[0][0])  # warm-up, like replay_batched's
        t0 = time.perf_counter()
        parts, again = _replay_recordings_in_flight(ctxs, chunked, ids_of)
        sec = time.perf_counter() - t0
        res = [np.concatenate(p) if p else np.zeros(0, ctxs[0].result_dtype) for p in parts]
        return (res if recordings is not None else res[0]), sec, again
    planner = PathPlanner(mission, cache, device=device)
    ctx = planner._ctx
    if path_table is not None:
        ctx.set_global_path_table(path_table)
    frames = list(zip(observations, positions, directions))
    chunks = [pack_frames(frames[lo:lo + batch_frames]) for lo in range(0, len(frames), batch_frames)]

    def one_replay():
        parts, prev, again = [], None, 0
        if cache:
            ctx.sort_cache_reset(1)  # (a fresh planner: the warm-up left an entry)
        for j, (off, cones, poses) in enumerate(chunks):
            if cache:
                res, prev, k = ctx.plan_sequence_cached(off, cones, poses, 1, initial_prev=prev)[:3]
            else:
                res, prev, k = ctx.plan_sequence(off, cones, poses, 1, initial_prev=prev, path_ids=None if ids_of is None else ids_of[0][j])
            parts.append(res)
            again += k
        return parts, again

    if chunks:
        if cache:  # warm-up, like replay_batched's
            ctx.plan_sequence_cached(*chunks[0], 1)
        else:
            ctx.plan_sequence(*chunks[0], 1, path_ids=None if ids_of is None else ids_of[0][0])
    t0 = time.perf_counter()
    parts, again = one_replay()
    sec = time.perf_counter() - t0
    res = np.concatenate(parts) if parts else np.zeros(0, ctx.result_dtype)
    return res, sec, again


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data-path", "-i", type=Path, required=True)
    ap.add_argument("--remove-color-info", action="store_true")
    ap.add_argument("--batched", action="store_true")
    ap.add_argument("--stateful", action="store_true", help="--batched: one planner's view of the recording (frames chain through the previous path)")
    ap.add_argument("--cache", action="store_true", help="--batched --stateful: the planner has the reference's sorting cache on (fsdp_plan_sequence_cached)")
    ap.add_argument("--copies", type=int, default=1, help="--batched --stateful: replay this many copies of the recording, each a planner of its own, "
                                                          "kept in flight as sequence tickets (fsdp_submit_sequence)")
    ap.add_argument("--output-path", "-o", type=Path, default=None)
    ap.add_argument("--device", type=int, default=None)
    ap.add_argument("--devices", type=str, default=None, help='--batched: GPUs the stream is sharded over from this process, e.g. "0,1,2,3" or "all"')
    ap.add_argument("--batch-frames", type=int, default=4096, help="--batched: frames per batch of the stream")
    ap.add_argument("--depth", type=int, default=4, help="--batched: batches in flight")
    ap.add_argument("--experimental-performance-improvements", action="store_true",
                    help="per-frame replay: the reference's sorting cache (PathPlanner(mission, True))")
    ap.add_argument("--ranked", type=int, default=None, metavar="K",
                    help="instead of a timed replay: rank the K best end configurations of every frame and side and print, per frame, the "
                         "decision margins (left, right) and the deciding cost terms (trackdrive / autocross recordings)")
    ap.add_argument("--history", type=int, default=None, metavar="ROWS",
                    help="instead of a timed replay: trace the sorting stage's depth-first search of every frame and side, up to ROWS visited "
                         "configurations each, and print per side how far the searches went and which predicates turned candidates away; with "
                         "--output-path the per-frame histograms are written too (trackdrive / autocross recordings)")
    a = ap.parse_args(argv)
    if a.history is not None:
        from ._capi import CandVerdict

        mission = select_mission_by_filename(a.data_path.name)
        positions, directions, observations = load_data_json(a.data_path, a.remove_color_info)
        status, n_rows, none_left, hist = replay_history(mission, positions, directions, observations, a.history, a.device, a.batch_frames)
        sides = {}
        for s, name in enumerate(("left", "right")):
            sides[name] = {"frames_searched": int((n_rows[:, s] > 0).sum()), "rows_visited": int(n_rows[:, s].sum()),
                           "most_rows_in_a_frame": int(n_rows[:, s].max()) if len(n_rows) else 0,
                           "frames_without_a_configuration": int(none_left[:, s].sum()),
                           "rejections": {CandVerdict(code).name.lower(): int(hist[:, s, code].sum()) for code in range(1, 10)}}
        if a.output_path:
            np.savez_compressed(a.output_path, status=status, n_rows=n_rows, no_configuration=none_left, verdict_histogram=hist)
        print(json.dumps({"file": str(a.data_path), "mission": mission.name, "frames": len(status), "mode": "history", "rows_cap": a.history,
                          "frames_beyond_rows_cap": int((n_rows > a.history).any(axis=1).sum()), **sides}))
        return
    if a.ranked is not None:
        from ._capi import COST_TERM_NAMES

        mission = select_mission_by_filename(a.data_path.name)
        positions, directions, observations = load_data_json(a.data_path, a.remove_color_info)
        status, counts, margins, deciding = replay_ranked(mission, positions, directions, observations, a.ranked, a.device, a.batch_frames)
        for f in range(len(status)):
            print(json.dumps({"frame": f, "status": int(status[f]), "candidates": [int(c) for c in counts[f]],
                              "margin": [float(m) if np.isfinite(m) else None for m in margins[f]],
                              "deciding_term": [int(d) for d in deciding[f]],
                              "deciding_term_name": [COST_TERM_NAMES[d] if d >= 0 else None for d in deciding[f]]}))
        fin = margins[np.isfinite(margins)]
        print(json.dumps({"file": str(a.data_path), "mission": mission.name, "frames": len(status), "mode": "ranked", "top_k": max(2, a.ranked),
                          "sides_with_a_runner_up": int(fin.size), "smallest_margin": float(fin.min()) if fin.size else None}))
        return
    if a.batched and a.experimental_performance_improvements:
        ap.error("--experimental-performance-improvements is state of one planner: per-frame replay, or --batched --stateful --cache")
    if a.cache and not (a.batched and a.stateful):
        ap.error("--cache goes with --batched --stateful (per-frame replay: --experimental-performance-improvements)")
    mission = select_mission_by_filename(a.data_path.name)
    positions, directions, observations = load_data_json(a.data_path, a.remove_color_info)
    out = {"file": str(a.data_path), "mission": mission.name, "frames": len(positions)}
    if a.batched:
        if a.stateful:
            if a.copies > 1:
                many, sec, again = replay_stateful_batched(mission, None, None, None, a.device, batch_frames=a.batch_frames, cache=a.cache,
                                                           recordings=[(positions, directions, observations)] * a.copies)
                res = np.concatenate(many)
            else:
                res, sec, again = replay_stateful_batched(mission, positions, directions, observations, a.device, batch_frames=a.batch_frames, depth=a.depth,
                                                          cache=a.cache)
            out.update(frames_planned_again_with_their_predecessors_path=again, sorting_cache=a.cache)
        else:
            devs = None if a.devices is None else ("all" if a.devices == "all" else [int(x) for x in a.devices.split(",")])
            res, sec = replay_batched(mission, positions, directions, observations, a.device, batch_frames=a.batch_frames, depth=a.depth, devices=devs)
        out.update(mode="batched", seconds_per_batch=sec, frames_per_s=len(res) / sec,
                   status_histogram={int(k): int(v) for k, v in zip(*np.unique(res["status"], return_counts=True))})
        paths = res["path"]
    else:
        paths, times, reloc_frame, info = replay_per_frame(mission, positions, directions, observations, a.device,
                                                           a.experimental_performance_improvements)
        out.update(mode="per-frame", experimental_performance_improvements=a.experimental_performance_improvements, p50_us=float(np.median(times) * 1e6), mean_us=float(times.mean() * 1e6),
                   max_us=float(times.max() * 1e6), frames_over_100ms=int((times > 0.1).sum()), relocalized_at_frame=reloc_frame)
        if info is not None:
            out.update(translation=[float(x) for x in info.translation], rotation_deg=float(np.rad2deg(info.rotation)))
    if a.output_path:
        np.savez_compressed(a.output_path, path=paths)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
