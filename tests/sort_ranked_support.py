"""Shared checks of the ranked sorting candidates (include/fsdp.h fsdp_sort_batch_ranked) for tests/test_sort_ranked_cpu.py
(the kernel sources under the emulator) and tests/test_sort_ranked_gpu.py (the library).  TEST INFRASTRUCTURE.

A `run` callable is one way to execute a batch: run(off, cones, poses, top_k=64, terms=True) -> (sort records, counts (n,2),
configs (n,2,top_k,L), costs (n,2,top_k), terms (n,2,top_k,7) or None); plain(off, cones, poses) -> the records of the
unranked call on the same route.
"""
from __future__ import annotations

import numpy as np

SIDE_TYPES = (2, 1)  # side 0 = left (ConeTypes.LEFT = 2), side 1 = right (1)
SIDE_NAMES = ("left", "right")


def close(a, b, rtol):
    """the comparison tests/parity.py assert_intermediates_equal applies to best_cost_* (rtol 0: bit-equal values)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.abs(a - b) <= rtol * np.maximum(1.0, np.abs(b))).all())


def fixture_batches(golden_dir):
    """sort_ranked.npz as batches [(frame numbers, off, cones, poses)]: the frames of up to 128 cones (sort_kernel_128) and the
    200-cone ones (sort_kernel) apart, as a caller of the library would hand them over for either kernel to be chosen."""
    g = np.load(golden_dir / "sort_ranked.npz")
    n = np.diff(g["offsets"])
    out = []
    for sel in (np.flatnonzero(n <= 128), np.flatnonzero(n > 128)):
        xs = [g["cones"][g["offsets"][k] : g["offsets"][k + 1]] for k in sel]
        off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32)
        out.append((sel, off, np.concatenate(xs), g["poses"][sel]))
    return g, out


def npz_batch(golden_dir, name, frames):
    g = np.load(golden_dir / f"{name}.npz")
    xs = [g["cones"][g["offsets"][k] : g["offsets"][k + 1]] for k in frames]
    off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32)
    return g, off, np.concatenate(xs), g["poses"][list(frames)]


def lex_sorted(rows):
    rows = [tuple(int(v) for v in r) for r in rows]
    return rows == sorted(rows)


def check_against_oracle(oracle, off, cones, poses, got, cost_rtol, top_k=64, oracle_cones=None):
    """Items 1 and 3 of the issue for one batch.  got = run(...) at top_k.  oracle_cones: per frame the array the oracle sees and
    a map from its indices to the caller's (use_unknown_cones = False), else the frame's own cones.  Returns the number of
    (frame, side) pairs with a runner-up and the number of exact cost ties met (what the batch exercised)."""
    res, counts, configs, costs, terms = got
    n_multi = n_ties = 0
    for f in range(len(poses)):
        xyt = cones[off[f] : off[f + 1]]
        oxyt, back = (xyt, None) if oracle_cones is None else oracle_cones[f]
        side = [oracle.side_configs(oxyt, poses[f], t, 64) for t in SIDE_TYPES]
        neg = [-c for c, *_ in side if c < 0]
        st = int(res["status"][f])
        if neg:
            # (the sides are evaluated left first: the frame's status is the first side's code)
            assert st == neg[0], (f, st, neg)
        for s, (c, ocfg, ocost, _fk) in enumerate(side):
            name = SIDE_NAMES[s]
            if c <= 0 or st != 0:
                assert counts[f, s] == 0, (f, s, counts[f, s], c, st)
                m = 0
            else:
                assert counts[f, s] == c, (f, s, counts[f, s], c)
                assert counts[f, s] == res[f"n_configs_{name}"][f]
                m = min(c, top_k)
                assert len(ocost) >= m  # (the oracle call returns up to 64 rows: every stored row has its counterpart)
                ours = configs[f, s, :m]
                theirs = ocfg[:m] if back is None else np.where(ocfg[:m] >= 0, back[np.maximum(ocfg[:m], 0)], -1)
                assert close(costs[f, s, :m], ocost[:m], cost_rtol), (f, s, costs[f, s, :m], ocost[:m])
                # rows in the oracle's order; inside a run of exactly equal oracle costs as a set, ours in lexicographic order
                i = 0
                while i < m:
                    j = i + 1
                    while j < len(ocost) and ocost[j] == ocost[i]:
                        j += 1
                    if j - i == 1:
                        assert np.array_equal(ours[i], theirs[i]), (f, s, i, ours[i], theirs[i])
                    else:
                        n_ties += 1
                        full = ocfg[i:j] if back is None else np.where(ocfg[i:j] >= 0, back[np.maximum(ocfg[i:j], 0)], -1)
                        jj = min(j, m)
                        assert {tuple(r) for r in ours[i:jj]} <= {tuple(r) for r in full}, (f, s, i, j)
                        assert len({tuple(r) for r in ours[i:jj]}) == jj - i
                        if j <= m:
                            assert {tuple(r) for r in ours[i:j]} == {tuple(r) for r in full}, (f, s, i, j)
                        assert lex_sorted(ours[i:jj]), (f, s, i, j, ours[i:jj])  # (the way back from a filtered frame is monotonic)
                    i = j
                n_multi += c > 1
                # invariants: the winner is row 0, and the terms add up to the cost in column order, bit for bit
                assert costs[f, s, 0].tobytes() == np.float64(res[f"best_cost_{name}"][f]).tobytes(), (f, s)
                if terms is not None:
                    acc = np.zeros(m)
                    for k in range(terms.shape[-1]):
                        acc = acc + terms[f, s, :m, k]
                    assert acc.tobytes() == np.ascontiguousarray(costs[f, s, :m]).tobytes(), (f, s)
                    assert (terms[f, s, :m, 4] == 0).all()
            # unused rows
            assert (configs[f, s, m:] == -1).all() and np.isnan(costs[f, s, m:]).all(), (f, s)
            if terms is not None:
                assert np.isnan(terms[f, s, m:]).all(), (f, s)
    return n_multi, n_ties


def same_bits(a, b):
    if a is None or b is None:
        return a is b
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def same_records(a, b):
    """every field of the records, byte for byte"""
    return a.dtype == b.dtype and all(same_bits(a[k], b[k]) for k in a.dtype.names)


def check_call_invariants(run, plain, off, cones, poses, got):
    """Item 3: the records are those of the unranked call; top_k = 3 is the head of top_k = 64; terms = NULL changes nothing else."""
    res, counts, configs, costs, terms = got
    assert same_records(res, plain(off, cones, poses))
    r3, c3, g3, k3, t3 = run(off, cones, poses, top_k=3, terms=True)
    assert same_records(r3, res) and np.array_equal(c3, counts)
    assert same_bits(g3, configs[:, :, :3]) and same_bits(k3, costs[:, :, :3]) and same_bits(t3, terms[:, :, :3])
    rn, cn, gn, kn, tn = run(off, cones, poses, top_k=64, terms=False)
    assert tn is None and same_records(rn, res) and np.array_equal(cn, counts) and same_bits(gn, configs) and same_bits(kn, costs)


def check_terms_against_fixture(g, frames, got, rtol, level=""):
    """Item 2: the (C, 7) matrices of the reference capture, row for row.  level "": the reference with NumPy's default CPU
    dispatch; "_libm": the same run at the libm level of the dispatch (tests/golden/make_golden_ranked.py).  On a frame with a
    nearest-neighbour tie (knn_tie) the reference's set of configurations is its unstable argsort's: a side whose count differs
    there is left out, as tests/parity.py leaves out the configuration counts.  Returns (rows compared, sides left out)."""
    _res, counts, configs, costs, terms = got
    rows = skipped = 0
    for i, k in enumerate(frames):
        for s in range(2):
            n, at = int(g["n_rows"][k, s]), int(g["row_off"][k, s])
            if g["knn_tie"][k] and counts[i, s] != n:
                skipped += 1
                continue
            assert counts[i, s] == n, (k, s, counts[i, s], n)
            m = min(n, terms.shape[2])
            ref_t, ref_cfg, ref_c = g["terms" + level][at : at + m], g["configs"][at : at + m], g["costs" + level][at : at + m]
            # the reference's argsort leaves a run of equal costs in an order of its own: pair the rows by configuration
            for r in range(m):
                hit = np.flatnonzero((ref_cfg == configs[i, s, r][None, : ref_cfg.shape[1]]).all(axis=1))
                assert len(hit) == 1, (k, s, r)
                h = int(hit[0])
                assert h == r or ref_c[h] == ref_c[r], (k, s, r, h)
                assert close(terms[i, s, r], ref_t[h], rtol), (k, s, r, terms[i, s, r], ref_t[h])
                assert close(costs[i, s, r], ref_c[h], rtol), (k, s, r)
                assert terms[i, s, r, 4] == 0
            rows += m
    return rows, skipped


def retyped_unknown(golden_dir, n_frames=16, seed=5):
    """item 4: the first frames of cfg2_color with a third of the cones retyped UNKNOWN"""
    g, off, cones, poses = npz_batch(golden_dir, "cfg2_color", range(n_frames))
    cones = cones.copy()
    rng = np.random.default_rng(seed)
    cones[rng.random(len(cones)) < 1 / 3, 2] = 0.0
    return off, cones, poses


def filtered_views(off, cones):
    """per frame: (the frame without its UNKNOWN cones, indices of the kept cones in the caller's frame)"""
    out = []
    for f in range(len(off) - 1):
        xyt = cones[off[f] : off[f + 1]]
        keep = np.flatnonzero(xyt[:, 2] != 0)
        out.append((xyt[keep], keep.astype(np.int32)))
    return out
