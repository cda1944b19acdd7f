"""The hard-to-round operand sets of tests/hard_rounding.py: their own claims re-checked in integer arithmetic, and the device's
shortened FP64 sequences run on them on the host (tests/seq_model.py: the device bodies of csrc/device_prims.h with the host's
exact fma, and a MODEL of the two hardware seeds).

The model is a model: what v_rcp_f64 and v_rsq_f64 return on gfx950 is not measured anywhere in this repository, so a seed
error eps here stands for an assumption, not for the hardware.  tests/test_hard_rounding_gpu.py, on the device, is the verdict
on the sequences; what this file proves is that the operand sets are what they claim to be, that they catch a sequence that is
one ulp off (which random operands do not), and where the sequences' correctness depends on the quality of the seed."""
import math
import random
from fractions import Fraction

import numpy as np
import pytest

import hard_rounding as hr
import seq_model

P52, P53 = hr.P52, hr.P53


# ---- the exact references themselves --------------------------------------------------------------------------------
def test_exact_rounding_primitives():
    """Round-half-even to a double: ties, gradual underflow, and Python's own correctly rounded int / int on random rationals;
    the exact square root on perfect squares, next to them, and against the host's IEEE sqrt."""
    rn = hr.round_half_even
    assert rn(Fraction(P53 + 1)) == float(P53) and rn(Fraction(P53 + 3)) == float(P53 + 4)  # ties to even
    assert rn(Fraction(2 * P53 + 2)) == float(2 * P53) and rn(Fraction(2 * P53 + 6)) == float(2 * P53 + 8)
    assert rn(Fraction(2 * P53 + 3)) == float(2 * P53 + 4) and rn(Fraction(-(P53 + 3))) == -float(P53 + 4)
    assert rn(Fraction(1, 1 << 1074)) == 5e-324 and rn(Fraction(1, 1 << 1075)) == 0.0 and rn(Fraction(3, 1 << 1075)) == 1e-323
    assert rn(Fraction(0)) == 0.0
    rng = random.Random(5)
    for _ in range(3000):
        n, d = rng.randrange(1, 1 << rng.randrange(1, 200)), rng.randrange(1, 1 << rng.randrange(1, 200))
        assert rn(Fraction(n, d)) == n / d  # (int / int is correctly rounded in Python)
        a, b = math.ldexp(rng.random() + 0.5, rng.randrange(-300, 300)), math.ldexp(rng.random() + 0.5, rng.randrange(-300, 300))
        assert hr.div(a, -b) == a / -b and hr.mul(a, b) == a * b and hr.add(a, -b) == a - b and hr.sqrt(a) == math.sqrt(a)
    for m in (3, P52 + 12345, (1 << 26) + 1):
        assert hr.sqrt(float(m * m)) == float(m)
    assert hr.sqrt(float((1 << 26) + 1) ** 2 + 1.0) == float((1 << 26) + 1) and hr.sqrt(0.0) == 0.0 and hr.sqrt(5e-324) == math.sqrt(5e-324)


# ---- the generators' claims -----------------------------------------------------------------------------------------
def test_fixture_divisors_satisfy_their_identity():
    """tests/golden/hard_divisors.npz: every D M = 2^106 + rho with M odd, |rho| <= 64 and D a 53-bit mantissa — 2^106 / D, the
    reciprocal's significand with one bit to spare, is M - rho / D: |rho| / D half-ulps from a rounding midpoint."""
    fx = hr.fixture_divisors()
    assert len(fx) == 371 and len({d for d, _, _ in fx}) == 371
    for D, M, rho in fx:
        assert D * M == (1 << 106) + rho and M & 1 and abs(rho) <= 64 and P52 <= D < P53 and P53 < M <= 2 * P53
        assert rho != 0
        want = M - 1 if rho > 0 else M + 1  # 2^106 / D = M - rho / D: the even neighbour of the midpoint M on that side
        assert hr.div(1.0, float(D)) == math.ldexp(want, -106)
    assert (hr.ALL_ONES, P53 + 1, -1) in fx  # 1 / (2 - 2^-52): Markstein's exceptional divisor is one of them


def test_hard_quotients_lie_where_they_claim():
    """2^sh N = D M + rho with N / D in (1/2, 1) (sh = 54) or (1, 2) (sh = 53): the exact quotient is (M + rho / D) 2^-sh with M
    a 54-bit integer — odd M: |rho| / D half-ulps from the midpoint M, and the correctly rounded quotient is the even neighbour
    on rho's side; even M: that close to the representable M."""
    mid, rep = hr.midpoint_quotients(), hr.representable_quotients()
    assert len(hr.odd_divisors()) > 3000 and {hr.ALL_ONES, hr.ONE_PLUS} <= set(hr.odd_divisors())
    assert len(mid) > 15000 and len(rep) > 15000  # about 0.69 of the 8 residues per divisor (the share of N that lands in range)
    for cases, odd in ((mid, 1), (rep, 0)):
        for N, D, rho, sh, M in cases:
            assert (N << sh) == D * M + rho and M & 1 == odd and abs(rho) <= 8 and D & 1 and P52 <= D < P53
            assert (P52 <= N < D) if sh == 54 else (D < N < P53)
            assert P53 < M < 2 * P53
            want = (M + 1 if rho > 0 else M - 1) if odd else M
            assert hr.div(float(N), float(D)) == math.ldexp(want, -sh)
    assert {abs(c[2]) for c in mid} == {1, 3, 5, 7} and {abs(c[2]) for c in rep} == {2, 4, 6, 8}
    assert {c[3] for c in mid} == {53, 54}


def test_division_operands_fill_the_band_to_its_edges():
    """Every operand lies inside [2^-255, 2^255]; the extreme binades [2^-255, 2^-254) and [2^254, 2^255) are populated on both
    sides of the quotient, with both signs; the outside pairs have an operand outside."""
    for name, (a, b) in hr.division_sets().items():
        for v in (a, b):
            m = np.abs(v)
            assert ((m >= hr.BAND_LO) & (m <= hr.BAND_HI)).all(), name
            assert (m < 2 * hr.BAND_LO).sum() > 100 and (m >= hr.BAND_HI / 2).sum() > 100, name
            assert (v < 0).any() and (v > 0).any(), name
    a, b = hr.division_sets()["one_over"]
    assert (np.frexp(np.abs(a))[0] == 0.5).all()  # numerators 2^k
    a, b = hr.outside_band_pairs()
    inb = lambda v: (np.abs(v) >= hr.BAND_LO) & (np.abs(v) <= hr.BAND_HI)
    assert not (inb(a) & inb(b)).any()
    assert math.nextafter(hr.BAND_LO, 0.0) in a and math.nextafter(hr.BAND_HI, math.inf) in b


def test_hard_square_roots_lie_where_they_claim():
    """1 + k 2^-52, odd k: with X = 2^52 + k, ((2^53 + k) / 2)^2 - X 2^52 = k^2 / 4 — the root lies k^2 2^-55 ulp below the
    midpoint (2^53 + k) / 2 and rounds down.  The family: X 2^52 = M^2 + M + j = (M + 1/2)^2 + j - 1/4, so the root lies
    |j - 1/4| / (sqrt + M + 1/2) ulp from the midpoint M + 1/2 (below 7.2e-15 ulp for |j| <= 64) and rounds up exactly when j > 0."""
    s = hr.sqrt_sets()
    assert len(s["above_one"]) == len(s["below_two"]) == 4096 and s["above_one"][0] == 1.0 + 2.0**-52 and s["below_two"][0] == 2.0 - 2.0**-52
    for k in range(1, hr.K_MAX + 1, 2):
        X = P52 + k
        assert (P53 + k) ** 2 - 4 * (X << 52) == k * k and math.isqrt(4 * (X << 52)) == P53 + k - 1
        assert hr.sqrt(math.ldexp(X, -52)) == math.ldexp(P52 + (k - 1) // 2, -52)
    fam = hr.sqrt_family()
    assert len(fam) == 3417
    for X, M, j in fam:
        assert (X << 52) == M * M + M + j and P52 <= X < P53 and P52 <= M < P53 and j % 2 == 0 and abs(j) <= hr.J_MAX
        assert hr.sqrt(math.ldexp(X, -52)) == math.ldexp(M + 1 if j > 0 else M, -52)
        if abs(j) <= 64:
            assert Fraction(abs(4 * j - 1), 4 * 2 * M) < Fraction(72, 10**16)  # (the two roots sum to more than 2 M)
    assert len({j for _, _, j in fam}) > 2000


def test_hard_square_root_arguments_are_reachable_from_a_givens_step():
    """x = RN(1 + RN(q q)) for a double q in (0, 1) for at least 85 % of the family (RN(sqrt(x - 1)) and eight neighbours on either
    side are tried), so the square-root regime of the Givens sets is not a handful of arguments."""
    ra = hr.reachable_sqrt_arguments()
    assert len(ra) >= 0.85 * len(hr.sqrt_family()), len(ra)
    fam = {math.ldexp(X, -52) for X, _, _ in hr.sqrt_family()}
    for x, q in ra:
        assert 0.0 < q < 1.0 and x in fam and hr.add(1.0, hr.mul(q, q)) == x


def _fpgivs_numpy(piv, ww):
    """fpgivs with numpy's IEEE operations (the statement of spline_device.h fpgivs)."""
    big = np.abs(piv) >= ww
    num, den, scale = np.where(big, ww, piv), np.where(big, piv, ww), np.where(big, np.abs(piv), ww)
    r = num / den
    dd = scale * np.sqrt(1.0 + r * r)
    return np.stack([ww / dd, piv / dd, dd])


def test_givens_operands_are_the_regimes_they_claim():
    """tiny pivot / tiny diagonal: dd is the large operand exactly and sn (cs) is the exact hard quotient N / D; the square-root
    regime hands sqrt a family argument; every pair passes the guard's condition, the outside pairs do not; the extreme binades
    are there."""
    g, ref = hr.givens_sets(), hr.givens_references()
    cases = hr.midpoint_quotients() + hr.representable_quotients()
    assert len(g["tiny_piv"][0]) == len(g["tiny_ww"][0]) == len(cases)
    (p, w), r = g["tiny_piv"], ref["tiny_piv"]
    assert np.array_equal(r[2], w) and np.array_equal(r[0], np.ones(len(w)))
    assert np.array_equal(np.abs(r[1]), np.array([math.ldexp(hr.div(float(c[0]), float(c[1])), -60) for c in cases]))
    (p, w), r = g["tiny_ww"], ref["tiny_ww"]
    assert np.array_equal(r[2], np.abs(p)) and np.array_equal(np.abs(r[1]), np.ones(len(w)))
    assert np.array_equal(r[0], np.array([math.ldexp(hr.div(float(c[0]), float(c[1])), -60) for c in cases]))
    assert (g["tiny_piv"][0] < 0).any() and (g["tiny_piv"][0] > 0).any() and (g["tiny_ww"][0] < 0).any()
    p, w = g["sqrt"]
    assert len(p) == 4 * len(hr.reachable_sqrt_arguments())
    q = np.minimum(np.abs(p), w) / np.maximum(np.abs(p), w)  # (a power of two divides exactly)
    assert set((1.0 + q * q).tolist()) == {x for x, _ in hr.reachable_sqrt_arguments()}
    p, w = g["equal"]
    assert np.array_equal(np.abs(p), w) and len(p) == 2 * 3 * 373
    lo = hi = 0
    for name, (p, w) in g.items():
        den, num = np.maximum(np.abs(p), w), np.minimum(np.abs(p), w)
        assert (w >= 0).all() and ((den >= hr.BAND_LO) & (den <= hr.BAND_HI) & ((num == 0) | (num >= hr.BAND_LO))).all(), name
        lo, hi = lo + int(((num > 0) & (num < 2 * hr.BAND_LO)).sum()), hi + int((den >= hr.BAND_HI / 2).sum())
    assert lo > 1000 and hi > 1000
    p, w = g["edges"]
    assert {hr.BAND_LO, hr.BAND_HI, math.nextafter(hr.BAND_LO, 1.0), math.nextafter(hr.BAND_HI, 1.0)} <= set(np.maximum(np.abs(p), w).tolist())
    p, w = hr.givens_outside_band()
    den, num = np.maximum(np.abs(p), w), np.minimum(np.abs(p), w)
    assert not ((den >= hr.BAND_LO) & (den <= hr.BAND_HI) & ((num == 0) | (num >= hr.BAND_LO))).any()


def test_numpy_ieee_operations_equal_the_exact_references():
    """The host's IEEE division and square root return the exact references on every operand (so a device mismatch is the
    device's), and FITPACK's chain with one rounding per operation is fpgivs with IEEE operations."""
    for k, (a, b) in hr.division_sets().items():
        assert np.array_equal(hr.bits(a / b), hr.bits(hr.division_references()[k])), k
    for k, x in hr.sqrt_sets().items():
        assert np.array_equal(hr.bits(np.sqrt(x)), hr.bits(hr.sqrt_references()[k])), k
    for k, (p, w) in hr.givens_sets().items():
        assert np.array_equal(hr.bits(_fpgivs_numpy(p, w)), hr.bits(hr.givens_references()[k])), k


# ---- the sequences on the host, under a model of the seeds -----------------------------------------------------------
@pytest.fixture(scope="module")
def known():
    g = np.load(hr.GOLDEN / "seq_model_known.npz")
    assert tuple(g["eps"].tolist()) == seq_model.EPS
    return g


def _rows(v):
    return {tuple(r) for r in hr.bits(v).reshape(len(v), -1).tolist()} if len(v) else set()


@pytest.mark.parametrize("i", range(len(seq_model.EPS)))
def test_sequences_under_the_seed_model_equal_the_exact_reference(known, i, capsys):
    """rcp_refined / div_rcp, sqrt_1_2 and fpgivs_guarded<true> (givens_dd_rd inside) as csrc/device_prims.h states them, with seeds
    RN(1 / d) (1 + eps) and RN(1 / sqrt(x)) (1 + eps), eps in {0, +-2^-20, +-2^-24, +-2^-28}, on every operand set: the exact
    reference bit for bit, except on the operands pinned in tests/golden/seq_model_known.npz (make_seq_model_known.py) — nothing
    outside that list may fail, so it can only shrink.  What the list holds (operands per set):

        eps       div midpoint  div one_over  sqrt family  giv tiny_piv / tiny_ww  giv sqrt  giv edges
        0               0             0            0              0 / 0               0          0
        +-2^-28         6            36            0              1 / 1               0          4
        +2^-24          6            36           14              2 / 2              48          4
        -2^-24          6            36           13              2 / 2              44          4
        +-2^-20         6            36         1708              2 / 2            6200          4

    - every failing division has the all-ones divisor mantissa (2^53 - 1) 2^m under a numerator 2^k: the reciprocal sticks at
      2^-m-1 however many Newton steps follow (Markstein's exceptional case) and the last fma meets an exact tie; with the correctly
      rounded seed (eps = 0) it comes out right — as it does on the device, whose seed for this divisor is evidently good enough.
      Before rcp_refined took its third Newton step the list also held 0x1.6666666666663 / 0x1.ffffffffffffb from |eps| = 2^-24 on
      (the reciprocal one ulp low): the operand the device misrounded, and the reason for that step.  The Givens rows are the
      all-ones quotient again (cs or sn over dd) and, from 2^-24 on, that second pair through the SEEDED reciprocal rd, which has
      one Newton step only (exact on the device);
    - the square root's last correction g + d h takes h from ONE coupled Goldschmidt step: its relative error is about
      1.5 eps^2, and an argument whose root lies 2^-47 ulp from a midpoint needs it below that — so the family fails from
      |eps| = 2^-24 on, and half of it at 2^-20.

    THE MODEL IS A MODEL.  The hardware's seeds are unmeasured here; the GPU test (tests/test_hard_rounding_gpu.py) is the verdict."""
    eps = seq_model.EPS[i]
    fails = seq_model.failing_operands(eps)
    report = {k: len(v) for k, v in fails.items() if len(v)}
    with capsys.disabled():
        print(f"\n  seed model eps = {eps:+.3e}: misrounded operands per set: {report or 'none'}")
    for k, v in fails.items():
        key = f"{i}|{k}"
        pinned = _rows(known[key]) if key in known.files else set()
        new = _rows(v) - pinned
        assert not new, (eps, k, len(new), [tuple(np.array(r, np.uint64).view(np.float64).tolist()) for r in sorted(new)[:4]])
    if eps == 0.0:
        assert not report
    with seed_eps_ctx(eps):
        for k, (p, w) in hr.givens_sets().items():
            assert (seq_model.givens(p, w)[3] == 1.0).all(), k  # the guard accepts the whole band
        for k, (a, b) in hr.division_sets().items():
            assert (seq_model.in_band(a, b) == 1.0).all(), k
        assert (seq_model.givens(*hr.givens_outside_band())[3] == 0.0).all()
        assert (seq_model.in_band(*hr.outside_band_pairs()) == 0.0).all()


def seed_eps_ctx(eps):
    return seq_model.seed_eps(eps)


def test_known_failures_of_the_division_are_the_all_ones_divisor(known):
    """The pinned division failures, at every eps: numerator 2^k over the all-ones mantissa 2^53 - 1, nothing else."""
    for key in known.files:
        if "|div|" in key:
            a, b = known[key][:, 0], known[key][:, 1]
            assert (np.frexp(np.abs(a))[0] == 0.5).all() and (np.frexp(np.abs(b))[0] * 2.0**53 == hr.ALL_ONES).all(), key


@pytest.mark.parametrize("ulps", [1, -1])
def test_one_ulp_in_a_reciprocal_is_caught(ulps):
    """The mutation check.  The refined reciprocal r of div_rcp(a, b, rcp_refined(b)), or the seeded reciprocal rd that
    givens_dd_rd hands the two quotients of a Givens step, moved by ONE representable value: at least 10 % of the hard
    quotients come out wrong (random operands: none of 20 000), in the division's set and — through sn and cs — in the Givens
    sets.  So a shortening that leaves the reciprocal one ulp off fails tests/test_hard_rounding_gpu.py."""
    a, b = hr.division_sets()["midpoint"]
    wrong = hr.bits(seq_model.div(a, b, ulps)) != hr.bits(hr.division_references()["midpoint"])
    print(f"r {ulps:+d} ulp: {wrong.mean():.3f} of the midpoint quotients misround")
    assert wrong.mean() >= 0.10, wrong.mean()
    rng = np.random.default_rng(0)
    ra, rb = rng.uniform(1.0, 2.0, 20000), rng.uniform(1.0, 2.0, 20000)
    assert (seq_model.div(ra, rb, ulps) != ra / rb).mean() <= 0.001
    assert np.array_equal(seq_model.div(ra, rb), ra / rb)
    n_mid = len(hr.midpoint_quotients())  # (the tiny sets list the midpoint quotients first)
    for name, col in (("tiny_piv", 1), ("tiny_ww", 0)):
        p, w = hr.givens_sets()[name]
        out, ref = seq_model.givens(p, w, ulps), hr.givens_references()[name]
        wrong = hr.bits(out[col])[:n_mid] != hr.bits(ref[col])[:n_mid]
        print(f"rd {ulps:+d} ulp: {wrong.mean():.3f} of {name}'s midpoint quotients misround")
        assert wrong.mean() >= 0.10, (name, wrong.mean())
        assert np.array_equal(hr.bits(out[2]), hr.bits(ref[2]))  # (dd does not pass through rd)
