"""Writes tests/golden/hard_divisors.npz: the 53-bit divisors whose own reciprocal is hardest to round.

A double d = D 2^e with 2^52 <= D < 2^53 has 1 / d = 2^106 / D 2^(-106 - e), and 2^106 / D lies in (2^53, 2^54]: its 54-bit
integer part M is odd exactly when the quotient sits next to a rounding midpoint of the 53-bit format.  With
    D M = 2^106 + rho,   M odd,
the exact reciprocal, (M - rho / D) 2^(-106 - e), lies |rho| / D half-ulps from that midpoint: for |rho| <= 64 that is below
2^-46 of a half-ulp, the closest a reciprocal can get.  Finding these D means factorising 2^106 + rho for every rho (sympy.divisors, about half a
minute in all), which is why the result is a committed fixture; tests/test_hard_rounding_cpu.py re-checks every identity
in integer arithmetic, so the fixture is trusted for nothing.

    python tests/golden/make_hard_divisors.py
"""
from pathlib import Path

import numpy as np
from sympy import divisors

RHO_MAX = 64


def hard_divisors(rho_max=RHO_MAX):
    found = []
    for rho in range(-rho_max, rho_max + 1):
        n = 2**106 + rho
        for D in divisors(n):
            if 2**52 <= D < 2**53 and (n // D) % 2 == 1:
                found.append((D, n // D, rho))
    return sorted(found)


if __name__ == "__main__":
    rows = hard_divisors()
    out = Path(__file__).resolve().parent / "hard_divisors.npz"
    np.savez(out, D=np.array([r[0] for r in rows], np.uint64), M=np.array([r[1] for r in rows], np.uint64),
             rho=np.array([r[2] for r in rows], np.int64))
    print(f"{len(rows)} divisors -> {out}")
