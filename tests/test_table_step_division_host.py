"""The table position's division by the photo tables' step, (lt - minlogtau)/dlogtau, by two roundings:
quo = fma(num, Ch, num * Cl) with Ch = RN(1/dlogtau), Cl = RN(1/dlogtau - Ch) (csrc/c2ray_device.hpp: rdlogtau_hi,
rdlogtau_lo, div_by_table_step, table_position_of_log).  The reference divides, so quo has to be the correctly rounded
quotient for every numerator; for a divisor known in advance that is a property of the constant (Brisebarre, Muller and
Raina 2004; Brisebarre and Muller 2008), and it is proven here for this one, in exact integer arithmetic:

 1. Ch and Cl are derived from dlogtau and compared with the header's literals.
 2. Before its last rounding the form is off the true quotient by less than ERR ulp of the quotient (the bound is computed
    from the constants and asserted to lie below 2^-54).
 3. With dlogtau = D * 2^e, D odd, the quotient of a numerator with the 53-bit significand X is, in units of its own ulp,
    X * 2^g / D (g = 51 where X is at least dlogtau's significand, 52 below it), so its distance from a rounding midpoint
    is |2 (X * 2^g mod D) - D| / (2 D) ulp.  Only where that is below ERR can the form misround.  Every residue r with
    |r - D/2| < K + 1 is taken, X = r * (2^g)^-1 mod D solved for, every such X in [2^52, 2^53) put through the two roundings
    in integers and compared with the correctly rounded X / dlogtau.  Every other significand keeps its quotient at least
    K / D ulp from any midpoint, which the test requires to exceed ERR 1000-fold.  D is odd, so no quotient is a tie.
    Powers of two scale both sides exactly, so the result holds wherever num * Cl does not underflow (|num| >= 2^-900).

The window is K = 20 000 (K / D = 2^-37.3 ulp against ERR < 2^-54): 53 336 significands, under a second in integers.

Then the compiled host functions against a true division: seeded arguments, both neighbours of every row boundary, the
clamp at -20 and its neighbours, +-0, arguments up to 308, +inf."""
import ctypes as C
import re
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "c2-ray3dm1d_helium_amd" / "csrc" / "c2ray_device.hpp"
dp = C.POINTER(C.c_double)

NTAU = 2000
MINLOGTAU = -20.0
DLOGTAU = float(np.float64(24.0) / np.float64(np.float32(NTAU)))      # radiation_tables.f90:59-61
WINDOW = 20000


def _int_and_exponent(x):
    """x = m * 2^e exactly, m a 53-bit integer (x normal)"""
    m, e = np.frexp(x)
    return int(np.ldexp(m, 53)), int(e) - 53


def _derived_constants():
    inv = 1 / Fraction(DLOGTAU)
    ch = float(inv)                       # Fraction -> float is correctly rounded
    cl = float(inv - Fraction(ch))
    return ch, cl


@pytest.fixture(scope="module")
def step():
    """The device functions under test compiled for the host (test-only build)."""
    so = ROOT / "tests" / "_table_step_harness.so"
    src = ROOT / "tests" / "table_step_harness.cpp"
    hdrs = list((ROOT / "c2-ray3dm1d_helium_amd" / "csrc").glob("*.hpp"))
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(src)],
                       check=True)
    return C.CDLL(str(so))


def _divide(step, num):
    num = np.ascontiguousarray(num, dtype=np.float64)
    quo = np.empty_like(num)
    step.ts_divide(C.c_int(num.size), num.ctypes.data_as(dp), quo.ctypes.data_as(dp))
    return quo


def _position(step, lt):
    lt = np.ascontiguousarray(lt, dtype=np.float64)
    ipos, res = np.empty(lt.size, dtype=np.int32), np.empty(lt.size)
    step.ts_position(C.c_int(lt.size), lt.ctypes.data_as(dp), ipos.ctypes.data_as(C.POINTER(C.c_int)), res.ctypes.data_as(dp))
    return ipos, res


def _position_by_division(lt):
    """radiation_photoionrates.f90:299-301 with a true division (the max with 0 cannot bind for lt >= -20 - a few ulp)"""
    with np.errstate(invalid="ignore"):
        odpos = np.minimum(float(NTAU), 1.0 + (np.asarray(lt, dtype=np.float64) - MINLOGTAU) / DLOGTAU)
    ipos = odpos.astype(np.int32)
    return ipos, odpos - ipos


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _assert_positions(step, lt):
    ipos, res = _position(step, lt)
    ipos_ref, res_ref = _position_by_division(lt)
    bad = np.flatnonzero((ipos != ipos_ref) | (res.view(np.uint64) != res_ref.view(np.uint64)))
    assert bad.size == 0, (bad.size, float(np.asarray(lt)[bad[0]]).hex())


# ---------------------------------------------------------------------------------------------------------------------
# 1. the constants

def test_the_headers_literals_are_the_reciprocal_in_two_pieces(step):
    assert DLOGTAU.hex() == "0x1.89374bc6a7efap-7"
    ch, cl = _derived_constants()
    text = HEADER.read_text()
    lit = {k: float.fromhex(re.search(rf"constexpr double {k} = (-?0x[0-9a-fA-F.]+p[+-]?\d+);", text).group(1))
           for k in ("rdlogtau_hi", "rdlogtau_lo")}
    assert lit["rdlogtau_hi"].hex() == ch.hex() == "0x1.4d55555555555p+6"
    assert lit["rdlogtau_lo"].hex() == cl.hex() == "0x1.b0aaaaaaaaaabp-49"
    got = np.empty(5)
    step.ts_constants(got.ctypes.data_as(dp))
    assert _same(got, np.array([DLOGTAU, ch, cl, MINLOGTAU, float(NTAU)]))


# ---------------------------------------------------------------------------------------------------------------------
# 2. and 3. the proof

def _error_bound_in_ulp():
    """An upper bound, as a Fraction in ulp of the quotient, of |num * Ch + RN(num * Cl) - num / dlogtau|:
    the constant's own error, |1/d - Ch - Cl| * |num|, is d * |1/d - Ch - Cl| of the quotient and a quotient is below
    2^53 of its ulp; the product's rounding is at most 2^-53 * |num * Cl| = 2^-53 * |Cl| * d of the quotient."""
    ch, cl = _derived_constants()
    d = Fraction(DLOGTAU)
    e_const = abs(1 / d - Fraction(ch) - Fraction(cl)) * d * 2 ** 53
    e_round = abs(Fraction(cl)) * d
    return e_const + e_round


def _two_roundings(X, chm, che, clm, cle):
    """RN(X * Ch + RN(X * Cl)) for the integer X, in integers; int -> float and int / int are correctly rounded"""
    t = int(float(X * clm))                                   # RN(X * Cl) / 2^cle
    assert che > cle
    return float(np.ldexp(float((X * chm << (che - cle)) + t), cle))


def _near_midpoint_significands(D, Y, K):
    """(X, g) for every 53-bit significand X whose quotient by dlogtau lies within K / D ulp of a rounding midpoint"""
    lo = (D - 1) // 2 - K        # D/2 is a half-integer: the K + 1 residues on either side of it
    out = []
    for g, (x_lo, x_hi) in ((51, (Y, 1 << 53)), (52, (1 << 52, Y))):
        inv = pow(1 << g, -1, D)
        for r in range(lo, lo + 2 * K + 2):
            x0 = r * inv % D
            X = x0 + (x_lo - x0 + D - 1) // D * D             # the first X = x0 (mod D) at or above x_lo
            while X < x_hi:
                out.append((X, g, r))
                X += D
    return out


def test_two_roundings_give_the_correctly_rounded_quotient_for_every_numerator():
    ch, cl = _derived_constants()
    (chm, che), (clm, cle) = _int_and_exponent(ch), _int_and_exponent(cl)
    Y, ye = _int_and_exponent(DLOGTAU)
    D, twos = Y, 0
    while D % 2 == 0:
        D, twos = D // 2, twos + 1
    assert D % 2 == 1 and twos == 1 and Y == 2 * D
    err = _error_bound_in_ulp()
    print(f"error before the last rounding < 2^{np.log2(float(err)):.2f} ulp; window K = {WINDOW}: K / D = 2^{np.log2(WINDOW / D):.2f} ulp")
    assert err < Fraction(1, 2 ** 54)
    assert Fraction(WINDOW, D) > 1000 * err                   # what the window leaves out cannot be misrounded
    cases = _near_midpoint_significands(D, Y, WINDOW)
    print(len(cases), "significands within the window")
    assert len(cases) == 53336                                 # 2 K + 2 residues, 4/3 significands to each on average
    closest, wrong = None, []
    for X, g, r in cases:
        assert 1 << 52 <= X < 1 << 53 and (X << g) % D == r
        assert 2 * r != D                                      # no tie
        dist = Fraction(abs(2 * r - D), 2 * D)
        closest = dist if closest is None else min(closest, dist)
        true = (X << -ye) / Y                                  # RN(X / dlogtau): dlogtau = Y * 2^ye, ye < 0
        # that g is this quotient's scale: X 2^g / D, the quotient in units of its ulp, has 53 bits
        assert 1 << 52 <= (X << g) // D < 1 << 53
        if _two_roundings(X, chm, che, clm, cle) != true:
            wrong.append(X)
    print(f"closest quotient 2^{np.log2(float(closest)):.2f} ulp from a midpoint")
    assert closest == Fraction(1, 2 * D)
    assert not wrong, (len(wrong), hex(wrong[0]))


def test_the_compiled_division_on_the_significands_next_to_a_midpoint(step):
    """the same significands through the compiled function, in several binades, against numpy's division"""
    Y, _ = _int_and_exponent(DLOGTAU)
    D = Y // 2
    X = np.array([c[0] for c in _near_midpoint_significands(D, Y, 1000)], dtype=np.float64)
    for e in (-100, -53, -48, -4, 0, 40):
        num = np.ldexp(X, e - 52)
        for s in (num, -num):
            assert _same(_divide(step, s), s / DLOGTAU), e


# ---------------------------------------------------------------------------------------------------------------------
# the compiled functions against a true division

def test_seeded_logarithms_from_the_clamp_to_beyond_the_last_row(step):
    rng = np.random.default_rng(20261020)
    lt = rng.uniform(-20.0, 4.5, 2_000_000)
    assert _same(_divide(step, lt - MINLOGTAU), (lt - MINLOGTAU) / DLOGTAU)
    _assert_positions(step, lt)
    ipos, _ = _position(step, lt)
    assert ipos.min() == 1 and ipos.max() == NTAU


def test_both_neighbours_of_every_row_boundary(step):
    z = np.arange(0, NTAU + 2, dtype=np.float64)              # rows 0 .. 2001
    num = z * DLOGTAU
    num3 = np.concatenate([np.nextafter(num, -np.inf), num, np.nextafter(num, np.inf)])
    assert _same(_divide(step, num3), num3 / DLOGTAU)
    lt = MINLOGTAU + num
    lt3 = np.concatenate([np.nextafter(lt, -np.inf), lt, np.nextafter(lt, np.inf)])
    assert _same(_divide(step, lt3 - MINLOGTAU), (lt3 - MINLOGTAU) / DLOGTAU)
    _assert_positions(step, lt3)
    ipos, res = _position(step, lt3)
    assert ipos.min() == 0 and ipos.max() == NTAU             # the neighbour below -20: row 0, residual just below 1
    assert (res[ipos == NTAU] == 0.0).all()


def test_the_clamp_zero_large_arguments_and_infinity(step):
    below = np.nextafter(MINLOGTAU, -np.inf)
    lt = np.array([MINLOGTAU, below, np.nextafter(below, -np.inf), np.nextafter(MINLOGTAU, np.inf), 0.0, -0.0])
    _assert_positions(step, lt)
    ipos, res = _position(step, lt)
    assert ipos[0] == 1 and res[0] == 0.0                     # tau at the clamp: row 1 exactly
    assert ipos[1] == 0 and 1.0 - res[1] < 1.0e-12            # log10 rounded below -20: 1 + quo just below 1
    assert ipos[3] == 1 and 0.0 < res[3] < 1.0e-12
    assert ipos[4] == ipos[5] and _same(res[4:5], res[5:6])
    # numerators of 0 and of a few ulp of 20, either sign
    tiny = np.array([0.0, -0.0, 2.0 ** -48, -2.0 ** -48, 3 * 2.0 ** -48, -3 * 2.0 ** -48])
    got = _divide(step, tiny)
    assert _same(got, tiny / DLOGTAU) and np.signbit(got[1])
    # every num >= 24 is beyond the last row; log10 of a double is at most 308.3
    rng = np.random.default_rng(20261021)
    big = np.concatenate([rng.uniform(4.0, 308.3, 200_000), [4.0, np.nextafter(4.0, 5.0), 308.0, 308.25, 308.3]])
    assert _same(_divide(step, big - MINLOGTAU), (big - MINLOGTAU) / DLOGTAU)
    _assert_positions(step, big)
    ipos, res = _position(step, big)
    assert (ipos == NTAU).all() and (res == 0.0).all()
    # +inf: what max(tau, 1e-20) lets through
    assert _divide(step, [np.inf])[0] == np.inf
    ipos, res = _position(step, [np.inf])
    assert ipos[0] == NTAU and res[0] == 0.0
