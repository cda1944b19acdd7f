"""Shared checks of the sorting stage's search history (include/fsdp.h fsdp_sort_batch_history) for
tests/test_sort_history_cpu.py (the kernel sources under the emulator) and tests/test_sort_history_gpu.py (the library).
TEST INFRASTRUCTURE.

A `run` callable is one way to execute a batch: run(off, cones, poses, rows_cap=256, verdicts=True) -> (sort records, h) with
h = dict(n_rows (n,2), target_length (n,2), rows (n,2,rows_cap,L), is_end (n,2,rows_cap), cand / verdict (n,2,rows_cap,K) or
None); plain(off, cones, poses) -> the records of fsdp_sort_batch on the same route; ranked(off, cones, poses) -> what
sort_batch_ranked returns at top_k = 64.
"""
from __future__ import annotations

import numpy as np

import sort_support as ss
from sort_ranked_support import same_bits, same_records  # noqa: F401  (re-exported for the tests)

KEYS = ("n_rows", "target_length", "rows", "is_end", "cand", "verdict")
ADDED, IN_ATTEMPT, OUTSIDE_ELLIPSE, WRONG_SIDE, SKIPS_NEIGHBOUR, ABSOLUTE_ANGLE, DIRECTIONAL_ANGLE, ZIGZAG, BEHIND_START, CROSSES_CAR = range(10)
STOPPED = (102, 202)  # frame statuses of a search that stopped early: its rows are a prefix, the stack is not empty at the end

# Check 3: the code each threshold pair of sort_support._search_pairs() flips, by the pair's name — read off sort_support.py and
# the order of the predicates in end_configurations.py:108-223, not run.
PAIR_CODES = (
    ("directional angle", DIRECTIONAL_ANGLE),
    ("edge length 4 beyond the directional angle", DIRECTIONAL_ANGLE),
    ("absolute angle", ABSOLUTE_ANGLE),
    ("edge ellipse", OUTSIDE_ELLIPSE),
    ("between", SKIPS_NEIGHBOUR),
    ("position 0, 5 degrees", WRONG_SIDE),
    ("sign flip, 1.3 rad", ZIGZAG),
    ("position 1, 90 degrees", BEHIND_START),
    ("car segment", CROSSES_CAR),
)


def expected_code(pair_name):
    hits = [code for prefix, code in PAIR_CODES if pair_name.startswith(prefix)]
    assert len(hits) == 1, pair_name
    return hits[0]


def side_trace(h, f, s):
    """the stored part of one side as (rows, is_end, cand, verdict), n_rows, target_length"""
    n, cap = int(h["n_rows"][f, s]), h["rows"].shape[2]
    m = min(n, cap)
    cv = (None, None) if h["cand"] is None else (h["cand"][f, s, :m], h["verdict"][f, s, :m])
    return (h["rows"][f, s, :m], h["is_end"][f, s, :m], *cv), n, int(h["target_length"][f, s])


def check_padding(h, f, s):
    """Unused entries hold -1 / 0xFF: the rows behind the stored ones, and in a stored row the positions behind the attempt and
    the neighbours behind the popped cone's"""
    (rows, is_end, cand, verdict), n, target = side_trace(h, f, s)
    m = len(rows)
    assert (h["rows"][f, s, m:] == -1).all() and (h["is_end"][f, s, m:] == 0xFF).all(), (f, s)
    assert n >= 0 and (target == 0) == (n == 0) and target <= h["rows"].shape[3], (f, s, n, target)
    assert (rows[:, target:] == -1).all() and np.isin(is_end, (0, 1)).all(), (f, s)
    if cand is not None:
        assert (h["cand"][f, s, m:] == -1).all() and (h["verdict"][f, s, m:] == 0xFF).all(), (f, s)
        assert ((cand == -1) == (verdict == 0xFF)).all() and (verdict[cand >= 0] <= CROSSES_CAR).all(), (f, s)


def check_replay(h, f, s, status):
    """Check 2, the stack machine: from the first row, a non-end row pushes cand[verdict == 0] in ascending order and the next row
    is the top of the stack.  Reproduces `rows` exactly, is_end == (position == target_length - 1 or no verdict is 0), and — for a
    side stored in full whose search was not stopped — reaches exactly n_rows rows.  Returns the rows replayed."""
    check_padding(h, f, s)
    (rows, is_end, cand, verdict), n, target = side_trace(h, f, s)
    if n == 0:
        return 0
    assert cand is not None
    first = int((rows[0] >= 0).sum())
    assert first in (1, 2) and (rows[0, :first] >= 0).all(), (f, s, rows[0])
    stack, attempt = [], rows[0].copy()
    for r in range(len(rows)):
        if r == 0:
            pos = first - 1
        else:
            assert stack, (f, s, r, "a row beyond an empty stack")
            node, pos = stack.pop()
            attempt[pos] = node
            attempt[pos + 1 :] = -1
        assert np.array_equal(rows[r], attempt), (f, s, r, rows[r], attempt)
        k = int((cand[r] >= 0).sum())
        nb, vd = cand[r, :k], verdict[r, :k]
        assert (cand[r, k:] == -1).all() and (np.diff(nb) > 0).all(), (f, s, r, cand[r])  # adjacency order: ascending
        assert int(attempt[pos]) not in nb.tolist()
        assert (vd[np.isin(nb, attempt[: pos + 1])] == IN_ATTEMPT).all() and (np.isin(nb, attempt[: pos + 1]) | (vd != IN_ATTEMPT)).all()
        # position-bound predicates
        assert not (pos >= 1 and (vd == WRONG_SIDE).any()) and not (pos == 0 and np.isin(vd, (OUTSIDE_ELLIPSE, ABSOLUTE_ANGLE, DIRECTIONAL_ANGLE)).any())
        assert not (pos < 2 and (vd == ZIGZAG).any()) and not (pos != 1 and (vd == BEHIND_START).any()), (f, s, r, pos, vd)
        end = pos == target - 1 or not (vd == ADDED).any()
        assert bool(is_end[r]) == end, (f, s, r, is_end[r], pos, target, vd)
        if not end:
            stack += [(int(c), pos + 1) for c in nb[vd == ADDED]]
    if len(rows) == n and status not in STOPPED:
        assert not stack, (f, s, "rows left on the stack", stack)
    return len(rows)


def check_against_ranked(h, f, s, side_type, xyt, counts, configs):
    """Every configuration the ranked call returns for the side is an end row, or an end row without its last cone (the type rule
    of end_configurations.py:491-500)"""
    (rows, is_end, _c, _v), n, _t = side_trace(h, f, s)
    assert len(rows) == n
    ends = {tuple(int(v) for v in r) for r in rows[is_end == 1]}
    L = rows.shape[1]
    cut = set()
    for e in ends:
        k = sum(v >= 0 for v in e)
        if k >= 1 and xyt[e[k - 1], 2] != side_type:
            cut.add(e[: k - 1] + (-1,) * (L - k + 1))
    for r in range(min(int(counts[f, s]), configs.shape[2])):
        c = tuple(int(v) for v in configs[f, s, r])
        assert c in ends or c in cut, (f, s, r, c)
    return int(counts[f, s])


def check_batch(run, plain, ranked, off, cones, poses, rows_cap=256, got=None):
    """Check 2 for one batch; returns (rows replayed, sides searched, ranked configurations found among the end rows)"""
    res, h = got if got is not None else run(off, cones, poses, rows_cap=rows_cap, verdicts=True)
    assert same_records(res, plain(off, cones, poses))
    _r, counts, configs, _costs, _terms = ranked(off, cones, poses)
    n_rows = n_sides = n_ranked = 0
    for f in range(len(poses)):
        xyt = cones[off[f] : off[f + 1]]
        for s, t in enumerate((2, 1)):
            assert h["n_rows"][f, s] <= rows_cap, (f, s, h["n_rows"][f, s])  # (the caller chose rows_cap for the batch)
            n_rows += check_replay(h, f, s, int(res["status"][f]))
            n_sides += h["n_rows"][f, s] > 0
            if res["status"][f] == 0:
                n_ranked += check_against_ranked(h, f, s, t, xyt, counts, configs)
    # the call without the verdicts: everything else unchanged
    res2, h2 = run(off, cones, poses, rows_cap=rows_cap, verdicts=False)
    assert same_records(res2, res) and h2["cand"] is None and h2["verdict"] is None
    assert all(same_bits(h2[k], h[k]) for k in KEYS[:4])
    return n_rows, int(n_sides), n_ranked


def same_history(a, b, sides=None):
    """two calls' arrays, bit for bit (sides: a boolean (n, 2) selection)"""
    for k in KEYS:
        if a[k] is None or b[k] is None:
            assert a[k] is b[k], k
            continue
        x, y = (a[k], b[k]) if sides is None else (a[k][sides], b[k][sides])
        assert same_bits(x, y), (k, np.argwhere(np.asarray(x) != np.asarray(y))[:4])


def neighbours_per_row(h):
    """(n, 2, rows_cap): how many neighbours each stored row's popped cone has"""
    return (h["cand"] >= 0).sum(axis=-1)


def raw_ends(h, f, s):
    """raw end configurations of a side stored in full"""
    (rows, is_end, _c, _v), n, _t = side_trace(h, f, s)
    assert len(rows) == n
    return int((is_end == 1).sum())


def first_difference(h, fa, fb, s):
    """the first entry, in row order and then neighbour order, at which the traces of two frames of a batch differ on side s ->
    (row, neighbour, verdict in fa, verdict in fb), or None.  Everything in front of it is equal: rows, end flags, neighbours."""
    (ra, ea, ca, va), na, ta = side_trace(h, fa, s)
    (rb, eb, cb, vb), nb, tb = side_trace(h, fb, s)
    for r in range(min(len(ra), len(rb))):
        assert np.array_equal(ra[r], rb[r]) and np.array_equal(ca[r], cb[r]), (fa, fb, s, r, "the traces part before a verdict does")
        d = np.flatnonzero(va[r] != vb[r])
        if len(d):
            return r, int(d[0]), int(va[r, d[0]]), int(vb[r, d[0]])
        assert ea[r] == eb[r]
    assert na == nb and ta == tb
    return None


def pair_side(obs):
    return 1 if obs.endswith("right") or obs.startswith("right") else 0


def check_search_pairs(run, pairs):
    """Check 3 on [(name, observable, below, above)]: one batch, the two members of a pair next to each other"""
    cases = [c for _n, _o, lo, hi in pairs for c in (lo, hi)]
    off, cones, poses = ss.as_batch(cases)
    _res, h = run(off, cones, poses, rows_cap=64, verdicts=True)
    seen = {}
    for i, (name, obs, _lo, _hi) in enumerate(pairs):
        d = first_difference(h, 2 * i, 2 * i + 1, pair_side(obs))
        assert d is not None, (name, "the members' traces are equal")
        want = expected_code(name)
        assert sorted(d[2:]) == [ADDED, want], (name, d, want)
        seen[want] = seen.get(want, 0) + 1
    return seen


def search_pairs_with_twins():
    """sort_support._search_pairs() with the mirrored twin of every pair and the colourless twin of every pair but one: the
    rear-end pair's LEFT start cone lies below the car's axis, where only its colour makes it a left start cone
    (core_trace_sorter.py:379-407) — without colours the left side starts elsewhere and never meets the threshold."""
    out = []
    for name, obs, lo, hi in ss._search_pairs():
        out.append((name, obs, lo, hi))
        out.append((name + ", mirrored", ss.mirrored_observable(obs), ss.mirrored(lo), ss.mirrored(hi)))
        if not name.startswith("car segment, rear end"):
            out.append((name + ", colourless", obs, ss.colourless(lo), ss.colourless(hi)))
    return out


def family_batches(k=5, max_len=12):
    """check 2's constructed inputs as [(name, (off, cones, poses))]: every family of tests/sort_support.py, the padded one split
    by frame size so that each batch takes one kernel"""
    fam = [
        ("all_pairs", [c for _n, _o, lo, hi in ss.all_pairs(k) for c in (lo, hi)]),
        ("posed_pairs", [c for _n, _o, lo, hi in ss.posed_pairs(k)[len(ss.all_pairs(k)) :] for c in (lo, hi)]),
        ("on_threshold", [c for _n, c in ss.on_threshold_posed()]),
        ("structural", [c for _n, c in ss.structural(max_len)]),
    ]
    padded = [p for _n, _c, p in ss.padded_family(k, max_len)]
    for lo, hi in ((0, 128), (129, 255), (256, 10**6)):
        sel = [c for c in padded if lo <= len(c[0]) <= hi]
        if sel:
            fam.append((f"padded_family, {lo}..{hi} cones", sel))
    return [(name, ss.as_batch(cases)) for name, cases in fam]


def npz_frames(golden_dir, name, frames):
    g = np.load(golden_dir / f"{name}.npz")
    xs = [g["cones"][g["offsets"][k] : g["offsets"][k + 1]] for k in frames]
    off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32)
    return off, np.concatenate(xs), g["poses"][list(frames)]


def fixture_batches(golden_dir):
    """sort_history.npz as (g, [(frame numbers, off, cones, poses)]): frames of up to 128 cones, of up to 255, and beyond, apart"""
    g = np.load(golden_dir / "sort_history.npz")
    n = np.diff(g["offsets"])
    out = []
    for sel in (np.flatnonzero(n <= 128), np.flatnonzero((n > 128) & (n <= 255)), np.flatnonzero(n > 255)):
        if len(sel) == 0:
            continue
        xs = [g["cones"][g["offsets"][k] : g["offsets"][k + 1]] for k in sel]
        off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32)
        out.append((sel, off, np.concatenate(xs), g["poses"][sel]))
    return g, out


def check_against_fixture(g, frames, h):
    """Check 1: on every side of a frame not flagged knn_tie the arrays equal the reference capture.  Returns (sides compared,
    rows compared, frames skipped)."""
    sides = rows = skipped = 0
    L, K = h["rows"].shape[3], h["cand"].shape[3]
    for i, k in enumerate(frames):
        if g["knn_tie"][k]:
            skipped += 1
            continue
        for s in range(2):
            if g["exc"][k] != "ok" and not g["searched"][k, s]:
                continue  # (the reference raised on the left side and never came to this one; the kernels search both)
            n, at = int(g["n_rows"][k, s]), int(g["row_off"][k, s])
            assert h["n_rows"][i, s] == n, (k, s, h["n_rows"][i, s], n)
            assert h["target_length"][i, s] == g["target_length"][k, s], (k, s)
            assert n <= h["rows"].shape[2], (k, s, n)
            assert np.array_equal(h["rows"][i, s, :n], g["rows"][at : at + n, :L]), (k, s)
            assert np.array_equal(h["is_end"][i, s, :n], g["is_end"][at : at + n]), (k, s)
            assert np.array_equal(h["cand"][i, s, :n], g["cand"][at : at + n, :K]), (k, s)
            assert np.array_equal(h["verdict"][i, s, :n], g["verdict"][at : at + n, :K]), (k, s)
            sides += n > 0
            rows += n
    return sides, rows, skipped
