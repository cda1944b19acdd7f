"""The device's shortened FP64 sequences (csrc/device_prims.h: rcp_refined / div_rcp, sqrt_1_2, givens_dd_rd; spline_device.h:
in_div_band, the guard of fpgivs_guarded<true>) on the operands of tests/hard_rounding.py: quotients and square roots that lie as
close to a rounding midpoint as the format allows, the divisors whose reciprocal is hardest to round, 1.0 over each of them
(fpbspl3's quot(1.0, den)), and the first and last binades of the guards' exponent band with the first values outside it.
Every result is held against an exact integer reference, bit for bit — random operands (tests/test_gpu_parity.py) cannot see a
sequence that is one ulp off.

Three different findings have three different messages:
  fast != device IEEE   the shortened sequence and the compiler's own operation disagree: the two routes of a frame differ;
  device IEEE != exact  the compiler's division / square root misrounds: the plain-division route (ST_RETRY) is wrong too;
  fast != exact         the shortened sequence misrounds.

WHAT THESE TESTS FOUND (MI355X, gfx950, ROCm 7.2.0: HIP 7.2.26015, AMD clang 22.0.0git roc-7.2.0), and what was changed for it.
On ONE mantissa pair, N / D = 0x1.6666666666663 / 0x1.ffffffffffffb (D = 2^53 - 5; D (2^53 + 5) = 2^106 - 25: the reciprocal of D
is itself next to a midpoint; 2^54 N = D M + 1: the quotient lies 1 / D half-ulps above the midpoint M), at every scale and sign,
the compiler's a / b AND div_rcp(a, b, rcp_refined(b)) — then v_rcp_f64 and two Newton steps, the compiler's own refinement —
returned 0x1.6666666666666p-1 2^k where the exact quotient is 0x1.6666666666667p-1 2^k (6 of 101 766 midpoint operands); in the
Givens step the seeded reciprocal rd returned the exact sn / cs and fpgivs with the compiler's division the wrong one.  The host
model (tests/test_hard_rounding_cpu.py) gave the same wrong bits from a seed error of 2^-24 on: the two Newton steps leave r one
ulp below the correctly rounded 1 / D and the final fma(rem, r, q) falls on the wrong side of the midpoint.  Since then
rcp_refined takes a third Newton step (the correctly rounded reciprocal; the Givens step's first quotient runs it next to the
product and the remainder, off its chain: div_rcp_late), and the plain-division route divides with div_exact — the compiler's
a / b, then the choice between it and its neighbour by the exact remainders (csrc/device_prims.h).  The "device IEEE" column of
fsdp_selftest_math is div_exact.  Everything else was exact from the start: 2^k over all 373 hard divisors — 1.0 / (2 - 2^-52)
included: fast = IEEE = exact = 0x1.0000000000001p-1, the hardware's seed does not leave the reciprocal stuck at 0.5 —, all
11 613 square roots, the Givens square-root / equal / edge sets, every guard and band flag."""
import importlib

import numpy as np
import pytest

import hard_rounding as hr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    pkg = importlib.import_module("ft-fsd-path-planning_amd")
    c = pkg.Context(device=0, mission=int(pkg.MissionTypes.trackdrive))
    yield c
    c.close()


def _hexes(arrays, idx):
    return [tuple(float(a[i]).hex() for a in arrays) for i in idx[:4]]


def _three_way(what, fast, ieee, exact, operands, names):
    """The three comparisons of one quantity, as uint64; operands: the input arrays the examples are printed from."""
    f, d, e = hr.bits(fast), hr.bits(ieee), hr.bits(exact)
    msgs = []
    for title, p, q, pv, qv in (("fast sequence != device IEEE", f, d, fast, ieee), ("device IEEE != exact", d, e, ieee, exact),
                                ("fast sequence != exact", f, e, fast, exact)):
        bad = np.nonzero(p != q)[0]
        if len(bad):
            msgs.append(f"{what}: {title} on {len(bad)} of {len(p)} operands; ({', '.join(names)}, left, right) = "
                        f"{_hexes((*operands, pv, qv), bad)}")
    return msgs


@pytest.fixture(scope="module")
def math_run(ctx):
    """One launch over every division set and every square-root set (the shorter side repeats its operands)."""
    dsets, ssets = hr.division_sets(), hr.sqrt_sets()
    dref, sref = hr.division_references(), hr.sqrt_references()
    a = np.concatenate([dsets[k][0] for k in dsets])
    b = np.concatenate([dsets[k][1] for k in dsets])
    q = np.concatenate([dref[k] for k in dsets])
    x = np.concatenate([ssets[k] for k in ssets])
    s = np.concatenate([sref[k] for k in ssets])
    where = {}
    for kind, sets in (("div", dsets), ("sqrt", ssets)):
        at = 0
        for k, v in sets.items():
            n_k = len(v[0]) if kind == "div" else len(v)
            where[kind, k] = slice(at, at + n_k)
            at += n_k
    n = max(len(a), len(x))
    ia, ix = np.arange(n) % len(a), np.arange(n) % len(x)
    a, b, q, x, s = a[ia], b[ia], q[ia], x[ix], s[ix]
    return dict(a=a, b=b, q=q, x=x, s=s, out=ctx.selftest_math(x, a, b), where=where)


@pytest.mark.parametrize("name", ["above_one", "below_two", "special", "family"])
def test_square_root_on_1_2_is_correctly_rounded_on_hard_arguments(math_run, name):
    """sqrt_1_2 and the compiler's sqrt on 1 + k 2^-52, 2 - k 2^-52 (k <= 4096), 1, 2, 1.25, 1.5 and the 3417 arguments whose root
    lies within |j - 1/4| / (2 M + 1) ulp of a midpoint: both equal the exact root."""
    r, w = math_run, math_run["where"]["sqrt", name]
    msgs = _three_way("sqrt", r["out"][0][w], r["out"][1][w], r["s"][w], (r["x"][w],), ("x",))
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("name", ["midpoint", "representable", "one_over"])
def test_scaling_free_quotient_is_correctly_rounded_on_hard_operands(math_run, name):
    """div_rcp(a, b, rcp_refined(b)) and the compiler's a / b on the hard quotients (next to a midpoint, next to a representable
    value), both signs, the band's extreme binades included, and on 2^k over the divisors with the hardest reciprocals — among them
    1.0 / (2 - 2^-52), Markstein's exceptional case: both equal the exact quotient, and the band flag is 1 on every one of them."""
    r, w = math_run, math_run["where"]["div", name]
    a, b = r["a"][w], r["b"][w]
    msgs = _three_way("quotient", r["out"][2][w], r["out"][3][w], r["q"][w], (a, b), ("a", "b"))
    off = np.nonzero(r["out"][4][w] != 1.0)[0]
    if len(off):
        msgs.append(f"band flag 0 on {len(off)} in-band operand pairs: {_hexes((a, b), off)}")
    assert not msgs, "\n".join(msgs)


def test_band_flag_refuses_the_first_values_outside(ctx):
    """in_div_band: 0 as soon as one operand leaves [2^-255, 2^255] — the neighbours of the edges, 2^-256, 2^256, a denormal."""
    a, b = hr.outside_band_pairs()
    out = ctx.selftest_math(np.full(len(a), 1.5), a, b)
    on = np.nonzero(out[4] != 0.0)[0]
    assert len(on) == 0, f"band flag 1 outside the band: {_hexes((a, b), on)}"


@pytest.fixture(scope="module")
def givens_run(ctx):
    gsets, gref = hr.givens_sets(), hr.givens_references()
    piv = np.concatenate([gsets[k][0] for k in gsets])
    ww = np.concatenate([gsets[k][1] for k in gsets])
    ref = np.concatenate([gref[k] for k in gsets], axis=1)
    where, at = {}, 0
    for k, v in gsets.items():
        where[k] = slice(at, at + len(v[0]))
        at += len(v[0])
    return dict(piv=piv, ww=ww, ref=ref, out=ctx.selftest_givens(piv, ww), where=where)


@pytest.mark.parametrize("name", ["tiny_piv", "tiny_ww", "sqrt", "equal", "edges"])
def test_givens_step_returns_the_exact_chain(givens_run, name):
    """fpgivs_guarded<true> (max / min, the first quotient, sqrt on [1, 2], the reciprocal of dd seeded from the square root's iterate,
    two quotients) and fpgivs with the compiler's operations, against FITPACK's chain with one exact rounding per operation:
    tiny pivots / tiny diagonals (cs or sn is a hard quotient taken with the SEEDED reciprocal), hard square-root arguments, equal
    magnitudes, the band's edges."""
    r, w = givens_run, givens_run["where"][name]
    msgs = []
    for k, what in enumerate(("cs", "sn", "dd")):
        msgs += _three_way(what, r["out"][k][w], r["out"][3 + k][w], r["ref"][k][w], (r["piv"][w], r["ww"][w]), ("piv", "ww"))
    assert not msgs, "\n".join(msgs)


def test_givens_guard_accepts_the_whole_band_and_nothing_outside(ctx, givens_run):
    r = givens_run
    off = np.nonzero(r["out"][6] != 1.0)[0]
    assert len(off) == 0, f"guard refuses {len(off)} in-band operand pairs: {_hexes((r['piv'], r['ww']), off)}"
    piv, ww = hr.givens_outside_band()
    out = ctx.selftest_givens(piv, ww)
    on = np.nonzero(out[6] != 0.0)[0]
    assert len(on) == 0, f"guard accepts operands outside the band: {_hexes((piv, ww), on)}"
