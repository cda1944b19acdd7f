"""TEST INFRASTRUCTURE: operands on which a shortened FP64 sequence shows a wrong last bit, and exact references for them.

The device's scaling-free division (rcp_refined / div_rcp), its square root on [1, 2] (sqrt_1_2) and the Givens step built from
them (givens_dd_rd, fpgivs_guarded<true>; csrc/device_prims.h, spline_device.h) must return the correctly rounded IEEE result.
A final correction fma(rem, r, q) goes wrong only when the exact quotient lies within about 2^-52 ulp of a rounding midpoint,
which a random operand pair does with probability of that order: random operands cannot see a reciprocal that is one ulp off.
The operands here are constructed to lie as close to a midpoint (or to a representable value) as the format allows, and at the
edges of the exponent band [2^-255, 2^255] the sequences' guards accept.

The references are integer arithmetic throughout (Python int, fractions.Fraction, math.isqrt); a float appears only as the
container of a finished result, filled by an exact ldexp.  tests/test_hard_rounding_cpu.py checks the generators' own claims,
tests/test_hard_rounding_gpu.py holds the device against the references."""
from __future__ import annotations

import functools
import math
import random
from fractions import Fraction
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
P52, P53 = 1 << 52, 1 << 53
BAND_LO, BAND_HI = math.ldexp(1.0, -255), math.ldexp(1.0, 255)


# ------------------------------------------------------------------------------------------------------------------
# exact rounding
# ------------------------------------------------------------------------------------------------------------------
def _rn(num: int, den: int) -> float:
    """Round-half-even of the rational num / den (den > 0) to a double; gradual underflow as IEEE has it."""
    if num == 0:
        return 0.0
    neg, num = num < 0, abs(num)
    e = num.bit_length() - den.bit_length() - 53  # num / den = q 2^e with q in [2^52, 2^53) after at most one step
    while True:
        e = max(e, -1074)
        n2, d2 = (num << -e, den) if e < 0 else (num, den << e)
        q, r = divmod(n2, d2)
        if q >= P53:
            e += 1
        elif q < P52 and e > -1074:
            e -= 1
        else:
            break
    if 2 * r > d2 or (2 * r == d2 and (q & 1)):
        q += 1
    v = math.ldexp(q, e)  # exact: q <= 2^53
    return -v if neg else v


def round_half_even(v: Fraction) -> float:
    return _rn(v.numerator, v.denominator)


def div(a: float, b: float) -> float:
    """RN(a / b) for finite a, b != 0."""
    na, da = a.as_integer_ratio()
    nb, db = b.as_integer_ratio()
    return _rn(na * db, da * nb) if nb > 0 else _rn(-na * db, -da * nb)


def mul(a: float, b: float) -> float:
    na, da = a.as_integer_ratio()
    nb, db = b.as_integer_ratio()
    return _rn(na * nb, da * db)


def add(a: float, b: float) -> float:
    na, da = a.as_integer_ratio()
    nb, db = b.as_integer_ratio()
    return _rn(na * db + nb * da, da * db)


def sqrt(x: float) -> float:
    """RN(sqrt(x)) for finite x >= 0, through math.isqrt."""
    n, d = x.as_integer_ratio()  # d = 2^k
    if n == 0:
        return 0.0
    k = d.bit_length() - 1
    if k & 1:
        n, k = n << 1, k + 1
    s_ = max(0, 70 - n.bit_length() // 2)  # isqrt below has >= 69 bits: its +1/2 stand-in cannot sit on a 53-bit midpoint
    s = math.isqrt(n << (2 * s_))
    exact = s * s == n << (2 * s_)
    # sqrt(x) = sqrt(n 2^2s_) / 2^(s_ + k/2); an inexact root lies strictly inside (s, s + 1): s + 1/2 rounds the same way
    return _rn(2 * s + (0 if exact else 1), 1 << (s_ + k // 2 + 1))


def givens(piv: float, ww: float):
    """FITPACK's fpgivs as the oracle states it (oracle/fitpack.cpp), one rounding per operation -> (cs, sn, dd)."""
    store = abs(piv)
    if store >= ww:
        q, scale = div(ww, piv), store
    else:
        q, scale = div(piv, ww), ww
    x = add(1.0, mul(q, q))
    dd = mul(scale, sqrt(x))
    return div(ww, dd), div(piv, dd), dd


def div_all(a, b):
    return np.array([div(float(p), float(q)) for p, q in zip(a, b)])


def sqrt_all(x):
    return np.array([sqrt(float(v)) for v in x])


def givens_all(piv, ww):
    """(3, n): cs, sn, dd"""
    return np.array([givens(float(p), float(w)) for p, w in zip(piv, ww)]).T.copy()


# ------------------------------------------------------------------------------------------------------------------
# divisors
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def fixture_divisors():
    """[(D, M, rho)]: the 53-bit D with D M = 2^106 + rho, M odd, |rho| <= 64 (tests/golden/make_hard_divisors.py): the divisors
    whose own reciprocal lies |rho| / D half-ulps from a midpoint."""
    g = np.load(GOLDEN / "hard_divisors.npz")
    return [(int(d), int(m), int(r)) for d, m, r in zip(g["D"], g["M"], g["rho"])]


ALL_ONES, ONE_PLUS = P53 - 1, P52 + 1
N_RANDOM_DIVISORS = 3000


@functools.lru_cache(None)
def odd_divisors():
    """Odd 53-bit divisor mantissas: 2^53 - 1 (all ones: Markstein's exceptional reciprocal), 2^52 + 1, 3000 random ones with a
    fixed seed, and the odd ones of the fixture."""
    rng = random.Random(20250611)
    ds = [ALL_ONES, ONE_PLUS] + [rng.randrange(P52, P53) | 1 for _ in range(N_RANDOM_DIVISORS)]
    ds += [d for d, _, _ in fixture_divisors() if d & 1]
    return list(dict.fromkeys(ds))


# ------------------------------------------------------------------------------------------------------------------
# hard quotients
# ------------------------------------------------------------------------------------------------------------------
MIDPOINT_RESIDUES = (1, -1, 3, -3, 5, -5, 7, -7)
REPRESENTABLE_RESIDUES = (2, -2, 4, -4, 6, -6, 8, -8)


def quotients_of(D: int, residues):
    """[(N, D, rho, sh, M)] with 2^sh N = D M + rho: sh = 54 and 2^52 <= N < D (N / D in (1/2, 1)), or sh = 53 and D < N < 2^53
    (N / D in (1, 2)).  Either way 2^sh N / D = M + rho / D lies in (2^53, 2^54): the quotient's 53-bit significand is M / 2
    and rho / D, in half-ulps, is what is left over — |rho| / D is the closest a quotient by D can come.  D odd: M has the
    parity of rho.  M odd (odd rho): the quotient lies next to a rounding MIDPOINT; M even: next to a REPRESENTABLE value."""
    out = []
    for sh in (54, 53):
        inv = pow(1 << sh, -1, D)
        for rho in residues:
            N = (rho * inv) % D
            if sh == 53:
                N += D
                if not D < N < P53:
                    continue
            elif not P52 <= N < D:
                continue
            out.append((N, D, rho, sh, ((N << sh) - rho) // D))
    return out


@functools.lru_cache(None)
def midpoint_quotients():
    return [c for D in odd_divisors() for c in quotients_of(D, MIDPOINT_RESIDUES)]


@functools.lru_cache(None)
def representable_quotients():
    return [c for D in odd_divisors() for c in quotients_of(D, REPRESENTABLE_RESIDUES)]


# exponents (of the operand's binade: magnitude in [2^e, 2^(e+1))) of numerator and divisor; the band's extreme binades
# [2^-255, 2^-254) and [2^254, 2^255) in every combination, and ordinary ones
EXP_PAIRS = ((0, 0), (-255, -255), (254, 254), (-255, 254), (254, -255), (31, -17), (-120, 77), (254, 0), (0, -255))


def _scaled(cases, per_case):
    """a, b (numpy) from [(N, D, ...)]: every pair with both signs of the numerator at `per_case` exponent pairs, the
    starting pair and the divisor's sign rotating with the case's index."""
    a, b = [], []
    for i, c in enumerate(cases):
        N, D = c[0], c[1]
        for j in range(per_case):
            ea, eb = EXP_PAIRS[(i + j) % len(EXP_PAIRS)]
            sb = -1.0 if (i + j) & 1 else 1.0
            for sa in (1.0, -1.0):
                a.append(sa * math.ldexp(N, ea - 52))
                b.append(sb * math.ldexp(D, eb - 52))
    return np.array(a), np.array(b)


@functools.lru_cache(None)
def division_sets():
    """{name: (a, b)}: operand arrays for a / b, all inside the band.
    midpoint / representable: the hard quotients, scaled and signed; one_over: numerator 2^k (fpbspl3's quot(1.0, den))
    over every fixture divisor, the all-ones mantissa and 2^52 + 1, at every exponent pair, both signs."""
    one = [(P52, D) for D in [ALL_ONES, ONE_PLUS] + [d for d, _, _ in fixture_divisors()]]
    return {"midpoint": _scaled(midpoint_quotients(), 3), "representable": _scaled(representable_quotients(), 2),
            "one_over": _scaled(one, len(EXP_PAIRS))}


def outside_band_pairs():
    """(a, b) with at least one operand outside [2^-255, 2^255]: the first values past either edge, and far ones."""
    lo, hi = math.nextafter(BAND_LO, 0.0), math.nextafter(BAND_HI, math.inf)
    out = [lo, -lo, hi, -hi, math.ldexp(1.0, -256), math.ldexp(1.0, 256), 1e-300, 1e300, 5e-324]
    inside = [1.0, -1.5, BAND_LO, BAND_HI]
    pairs = [(o, i) for o in out for i in inside] + [(i, o) for o in out for i in inside] + [(lo, hi), (hi, lo)]
    return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])


# ------------------------------------------------------------------------------------------------------------------
# hard square roots on [1, 2]
# ------------------------------------------------------------------------------------------------------------------
K_MAX = 4096
J_MAX = 4096


def _roots(j: int, n: int = 52):
    """All t mod 2^n with t^2 + t + j = 0 (mod 2^n), lifted bit by bit (j even: two of them)."""
    sol = [t for t in range(2) if (t * t + t + j) % 2 == 0]
    for b in range(1, n):
        m = 1 << (b + 1)
        sol = [u for t in sol for u in (t, t + (1 << b)) if (u * u + u + j) % m == 0]
    return sol


@functools.lru_cache(None)
def sqrt_family():
    """[(X, M, j)]: x = X 2^-52 in [1, 2) with X 2^52 = M^2 + M + j = (M + 1/2)^2 + j - 1/4, even |j| <= 4096: sqrt(X 2^52)
    lies |j - 1/4| / (2 M + 1) ulp from the midpoint M + 1/2 (below 7.2e-15 ulp for |j| <= 64)."""
    out = []
    for j in range(-J_MAX, J_MAX + 1, 2):
        for t in _roots(j):
            M = P52 + t
            v = M * M + M + j
            if v < (1 << 105):
                out.append((v >> 52, M, j))
    return out


@functools.lru_cache(None)
def sqrt_sets():
    """{name: x}: above_one: 1 + k 2^-52 (odd k: sqrt(x) lies k^2 2^-55 ulp below a midpoint), below_two: 2 - k 2^-52,
    k = 1 .. 4096; special; family: sqrt_family()."""
    return {"above_one": np.array([math.ldexp(P52 + k, -52) for k in range(1, K_MAX + 1)]),
            "below_two": np.array([math.ldexp(P53 - k, -52) for k in range(1, K_MAX + 1)]),
            "special": np.array([1.0, 2.0, 1.25, 1.5]),
            "family": np.array([math.ldexp(X, -52) for X, _, _ in sqrt_family()])}


# ------------------------------------------------------------------------------------------------------------------
# Givens operands (piv, ww): ww >= 0 is the band row's diagonal, piv the incoming row's element
# ------------------------------------------------------------------------------------------------------------------
REACH_NEIGHBOURS = 8


@functools.lru_cache(None)
def reachable_sqrt_arguments():
    """[(x, q)]: the arguments of sqrt_family() that a Givens step can hand its square root, x = RN(1 + RN(q q)) for a
    double q in (0, 1): RN(sqrt(x - 1)) and its eight neighbours on either side are tried, the first that reaches x is kept."""
    out = []
    for X, _, _ in sqrt_family():
        x = math.ldexp(X, -52)
        q0 = sqrt(math.ldexp(X - P52, -52))  # x - 1 is exact
        for s in sorted(range(-REACH_NEIGHBOURS, REACH_NEIGHBOURS + 1), key=abs):
            q = q0
            for _ in range(abs(s)):
                q = math.nextafter(q, 1.0 if s > 0 else 0.0)
            if add(1.0, mul(q, q)) == x:
                out.append((x, q))
                break
    return out


E_TINY = (-52, -247, 202, -130, 90)  # den = D 2^e in [2^(e+52), 2^(e+53)); num = N 2^(e-60): -247 and 202 are the band's extreme binades
E_SQRT = (0, 255, -200, 77, -30)     # den = 2^e
E_EQUAL = (-52, -307, 202)


@functools.lru_cache(None)
def givens_sets():
    """{name: (piv, ww)}, all inside the band:
    tiny_piv: ww = D 2^e, |piv| = N 2^(e-60) over every hard quotient (midpoint and representable): x = 1, dd = ww exactly and
              sn = piv / dd is the hard quotient N / D, computed with the SEEDED reciprocal rd;  tiny_ww: the roles swapped,
              the hard quotient is cs = ww / dd;
    sqrt:     den = 2^e, num = q 2^e with RN(1 + RN(q q)) a hard square-root argument; both orders of (|piv|, ww), both signs;
    equal:    piv = +-ww, ww = D 2^e over the fixture divisors, the all-ones mantissa and 2^52 + 1;
    edges:    den in {2^-255, its successor, 2^255, its predecessor}, num in {0, 2^-255, den}, both orders, both signs."""
    cases = midpoint_quotients() + representable_quotients()
    tp, tw, sp, sw = [], [], [], []
    for i, c in enumerate(cases):
        N, D = c[0], c[1]
        e = E_TINY[i % len(E_TINY)]
        s = -1.0 if (i // len(E_TINY)) & 1 else 1.0
        big, small = math.ldexp(D, e), math.ldexp(N, e - 60)
        tp.append((s * small, big))
        tw.append((s * big, small))
    for i, (x, q) in enumerate(reachable_sqrt_arguments()):
        e = E_SQRT[i % len(E_SQRT)]
        den, num = math.ldexp(1.0, e), math.ldexp(q, e)
        sp += [(den, num), (-den, num), (num, den), (-num, den)]
    eq = []
    for D in [ALL_ONES, ONE_PLUS] + [d for d, _, _ in fixture_divisors()]:
        for e in E_EQUAL:
            w = math.ldexp(D, e)
            eq += [(w, w), (-w, w)]
    ed = []
    for den in (BAND_LO, math.nextafter(BAND_LO, 1.0), BAND_HI, math.nextafter(BAND_HI, 1.0)):
        for num in (0.0, BAND_LO, den):
            ed += [(den, num), (-den, num), (num, den)] + ([(-num, den)] if num else [])
    arr = lambda ps: (np.array([p[0] for p in ps]), np.array([p[1] for p in ps]))
    return {"tiny_piv": arr(tp), "tiny_ww": arr(tw), "sqrt": arr(sp), "equal": arr(eq), "edges": arr(ed)}


def givens_outside_band():
    """(piv, ww) the guard must refuse: den just below 2^-255 or just above 2^255, or 0 < num < 2^-255."""
    lo, hi = math.nextafter(BAND_LO, 0.0), math.nextafter(BAND_HI, math.inf)
    ps = [(lo, 0.0), (-lo, 0.0), (0.0, lo), (lo, lo), (-lo, lo),                          # den below the band
          (hi, 1.0), (-hi, 1.0), (1.0, hi), (hi, hi), (0.0, hi), (hi, 0.0), (math.ldexp(1.0, 256), BAND_HI),  # den above it
          (lo, 1.0), (-lo, 1.0), (1.0, lo), (lo, BAND_LO), (BAND_LO, lo), (lo, BAND_HI), (BAND_HI, lo),  # 0 < num < 2^-255
          (math.ldexp(1.0, -256), 1.0), (1.0, math.ldexp(1.0, -256)), (5e-324, 1.0), (1.0, 5e-324), (1e-300, 1.0), (1.0, 1e-300)]
    return np.array([p[0] for p in ps]), np.array([p[1] for p in ps])


@functools.lru_cache(None)
def division_references():
    return {k: div_all(a, b) for k, (a, b) in division_sets().items()}


@functools.lru_cache(None)
def sqrt_references():
    return {k: sqrt_all(x) for k, x in sqrt_sets().items()}


@functools.lru_cache(None)
def givens_references():
    return {k: givens_all(p, w) for k, (p, w) in givens_sets().items()}


def bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)
