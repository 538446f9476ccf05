"""The folded log table and the one-subtraction split of the all-periodic isothermal one-SED rates kernel, on the host.
 - gm::LogFold (csrc/c2ray_math.hpp): an entry of the log's 256-case table whose reciprocal carries the case's power of two,
   invc * 2^-k, so that r = fma(x', invc * 2^-k, -1) needs neither z = x' * 2^-k nor the entry's kshift.  Entry by entry it
   must be ldexp(invc, -k) exactly, beside make_log_entry's w and c.
 - gm::log10_split_fold: hx by a select between the exponent fields of [0.5, 1) and [1, 2), and the exponent table's byte
   offset ky << 4 from hi - hx.  Against gm::log10_split, and the table path against gm::log_table_path4, bit for bit.
 - log10 through the whole route against gm::log10_ and against the platform's log10.
+inf (which max(tau, 1e-20) lets through) has no log10 through either table route -- both read the pair of ky = 1024 and
return a finite number beyond the photo tables' last row, where gm::log10_ returns +inf --: for it the route is compared
with the route it replaces, value and table position (the tables' last row)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
dp = C.POINTER(C.c_double)
CLASSES = ("split", "table path", "log10 vs gm::log10_", "log10 vs platform", "log10 vs replaced route", "table positions")


@pytest.fixture(scope="module")
def fold():
    """The device functions under test compiled for the host (test-only build)."""
    so = ROOT / "tests" / "_log_fold_harness.so"
    src = ROOT / "tests" / "log_fold_harness.cpp"
    hdrs = list((ROOT / "c2-ray3dm1d_helium_amd" / "csrc").glob("*.hpp"))
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(src)],
                       check=True)
    return C.CDLL(str(so))


def _check(fold, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert (x > 0).all()
    bad, first = (C.c_int * 6)(), (C.c_int * 6)()
    total = fold.lf_check(C.c_int(x.size), x.ctypes.data_as(dp), bad, first)
    report = {CLASSES[c]: (bad[c], float(x[first[c]]).hex()) for c in range(6) if bad[c]}
    assert total == 0 and not report, report


def test_every_entry_is_the_scaled_reciprocal_beside_w_and_c(fold):
    f, e = np.empty((256, 4)), np.empty((256, 4))
    assert fold.lf_tables(f.ctypes.data_as(dp), e.ctypes.data_as(dp)) == 256
    k = e[:, 3].astype(np.int64)
    E = np.arange(256)
    assert np.array_equal(k, (E - 0x30) >> 7) and set(k) == {-1, 0, 1}
    assert np.array_equal(f[:, 0].view(np.uint64), np.ldexp(e[:, 0], -k).view(np.uint64))
    assert np.array_equal(f[:, 1].view(np.uint64), e[:, 1].view(np.uint64))
    assert np.array_equal(f[:, 2].view(np.uint64), e[:, 2].view(np.uint64))
    assert (f[:, 3] == 0).all()
    # the scaling is exact: scaling back gives invc again
    assert np.array_equal(np.ldexp(f[:, 0], k).view(np.uint64), e[:, 0].view(np.uint64))


def test_seeded_arguments_from_the_clamp_to_two_to_the_132(fold):
    rng = np.random.default_rng(20261020)
    n = 4_200_000
    lo, hi = np.log2(1.0e-20), 132.0
    x = np.exp2(rng.uniform(lo, hi, n))
    x = np.clip(x, 1.0e-20, 2.0 ** 132)
    assert x.size >= 4_000_000 and x.min() >= 1.0e-20 and x.max() <= 2.0 ** 132
    _check(fold, x)


def test_both_sides_of_every_case_boundary_in_every_binade(fold):
    # the 257 boundaries of the 256 cases (hx = 0x3FE00000 + (E << 13), E = 0 .. 256), the last number below each and the
    # boundary itself, scaled into every binade from 2^-67 to 2^60
    hx = (np.uint64(0x3FE00000) + (np.arange(257, dtype=np.uint64) << np.uint64(13))) << np.uint64(32)
    edges = np.concatenate([(hx - np.uint64(1)).view(np.float64), hx.view(np.float64)])
    assert edges.size == 2 * 257 and np.isfinite(edges).all() and (edges > 0).all()
    # (a binade holds the cases of [1, 2) at its own scale and those of [0.5, 1) at the next one; below 2^-68, where ky would
    # be -68, neither exponent table has an entry -- the kernels never get there, they clamp at 1e-20 > 2^-67)
    x = np.concatenate([np.ldexp(edges, int(s)) for s in range(-67, 62)])
    x = x[x >= 2.0 ** -68]
    assert x.size >= 128 * 514 and x.min() == 2.0 ** -68 and x.max() == 2.0 ** 62
    _check(fold, x)


def test_the_clamp_one_and_its_neighbours_the_near_one_window_and_infinity(fold):
    one = np.array([np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0)])     # the k < 0 / k >= 0 switch of the select
    window = np.array([0x3FEE0000, 0x3FF10900], dtype=np.uint64) << np.uint64(32)
    window = np.concatenate([(window - np.uint64(1)).view(np.float64), window.view(np.float64)])
    scaled = np.concatenate([np.ldexp(np.concatenate([one, window]), s) for s in (-66, -20, -1, 0, 1, 20, 131)])
    _check(fold, np.concatenate([[1.0e-20, np.nextafter(1.0e-20, 1.0)], one, window, scaled, [np.inf],
                                 [np.finfo(np.float64).max, 2.0 ** 132]]))
