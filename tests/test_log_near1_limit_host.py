"""The near-1 test of the folded log route by a limit kept in the log table, on the host.
gm::log10_near1 asks whether hx, the high word of the argument scaled into [0.5, 2), lies in [0x3FEE0000, 0x3FF10900):
`hx - 0x3FEE0000u < 0x00030900u`, a subtraction and a compare.  The window starts on the boundary of entry 112 of the
256-entry folded table (entry E covers hx in 0x3FE00000 + [E << 13, (E + 1) << 13)) and ends inside entry 136, so a limit
per entry (gm::LogFold::lim: 0 below entry 112 and above 136, all ones for 112 .. 135, 0x3FF10900 for 136) makes the test
`hx < lim`.  Checked here: the 256 limits; the new test against the old one at both ends of every entry and around both
ends of the window; and seeded arguments from 1e-20 to 2^132 through gm::log10_split_fold -- the test, the limit that
gm::log_table_path_fold hands back, log10 through the whole folded route against gm::log10_, and the table positions.
The entry keeps its 32 bytes."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
dp = C.POINTER(C.c_double)
up = C.POINTER(C.c_uint32)
LO, HI = 0x3FEE0000, 0x3FF10900
CLASSES = ("limit handed back", "near-1 test", "log10 vs gm::log10_", "table positions")


@pytest.fixture(scope="module")
def lib():
    """The device functions under test compiled for the host (test-only build)."""
    so = ROOT / "tests" / "_log_near1_limit_harness.so"
    src = ROOT / "tests" / "log_near1_limit_harness.cpp"
    hdrs = list((ROOT / "c2-ray3dm1d_helium_amd" / "csrc").glob("*.hpp"))
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(src)],
                       check=True)
    return C.CDLL(str(so))


def _check_hx(lib, hx):
    hx = np.ascontiguousarray(hx, dtype=np.uint32)
    first = C.c_int()
    bad = lib.nl_check_hx(C.c_int(hx.size), hx.ctypes.data_as(up), C.byref(first))
    assert bad == 0, (bad, hex(int(hx[first.value])))


def _check(lib, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert (x > 0).all() and np.isfinite(x).all()
    bad, first = (C.c_int * 4)(), (C.c_int * 4)()
    total = lib.nl_check(C.c_int(x.size), x.ctypes.data_as(dp), bad, first)
    report = {CLASSES[c]: (bad[c], float(x[first[c]]).hex()) for c in range(4) if bad[c]}
    assert total == 0 and not report, report


def test_the_entry_keeps_its_size(lib):
    assert lib.nl_sizeof_entry() == 32


def test_the_256_limits(lib):
    lim, pad = np.empty(256, np.uint32), np.empty(256, np.uint32)
    assert lib.nl_limits(lim.ctypes.data_as(up), pad.ctypes.data_as(up)) == 256
    E = np.arange(256)
    want = np.where((E >= 112) & (E <= 135), 0xFFFFFFFF, 0).astype(np.uint32)
    want[136] = HI
    assert np.array_equal(lim, want)
    assert (pad == 0).all()
    # the window starts with entry 112 and ends inside entry 136
    assert 0x3FE00000 + (112 << 13) == LO and 0x3FE00000 + (136 << 13) < HI < 0x3FE00000 + (137 << 13)


def test_both_ends_of_every_entry_and_of_the_window(lib):
    E = np.arange(256, dtype=np.int64)
    first = 0x3FE00000 + (E << 13)
    hx = np.concatenate([first, first + 1, first + (1 << 13) - 1, first + (1 << 12),
                         [LO - 1, LO, LO + 1, HI - 1, HI, HI + 1]])
    assert hx.min() == 0x3FE00000 and hx.max() == 0x3FFFFFFF
    _check_hx(lib, hx)
    # ... and every hx of the entries around the window's two ends
    _check_hx(lib, np.arange(0x3FE00000 + (110 << 13), 0x3FE00000 + (114 << 13)))
    _check_hx(lib, np.arange(0x3FE00000 + (134 << 13), 0x3FE00000 + (139 << 13)))


def test_seeded_arguments_from_the_clamp_to_two_to_the_132(lib):
    rng = np.random.default_rng(20261021)
    n = 4_000_000
    lo, hi = np.log2(1.0e-20), 132.0
    x = np.exp2(rng.uniform(lo, hi, n))
    x[0], x[1] = 1.0e-20, 2.0 ** 132
    # a tenth of them within a few per cent of a power of two, where the window lies, whatever the power
    m = n // 10
    x[2:2 + m] = np.ldexp(rng.uniform(0.93, 1.07, m), rng.integers(-66, 132, m))
    # ... and the doubles next to the window's ends, under several exponents
    ends = np.array([LO << 32, HI << 32], dtype=np.uint64).view(np.float64)
    near = np.concatenate([np.nextafter(ends, 0.0), ends, np.nextafter(ends, 4.0)])
    edge = np.concatenate([np.ldexp(near, 2 * k) for k in (-33, -8, -1, 0, 1, 9, 65)])
    edge = edge[(edge >= 1.0e-20) & (edge <= 2.0 ** 132)]
    x[2 + m:2 + m + edge.size] = edge
    assert x.min() >= 1.0e-20 and x.max() <= 2.0 ** 132
    _check(lib, x)
