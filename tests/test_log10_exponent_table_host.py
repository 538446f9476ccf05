"""What the isothermal one-SED rates kernel reads where it used to compute, on the host and in the code object.
 - The table of log10's exponent terms (gm::Log10Exp, csrc/c2ray_math.hpp): the pair (y * log10_2lo, y * log10_2hi) per
   power of two y, which replaces a conversion and two products per logarithm.  Entry by entry it must be the two
   products, and log10 through it must be gm::log10_ bit for bit.
 - The two kernels in the built library: LDS small enough for five blocks per compute unit, no private segment."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from code_object import READELF, kernel_notes

ROOT = Path(__file__).resolve().parent.parent
dp = C.POINTER(C.c_double)
LOG10_2HI = float.fromhex("0x1.34413509f6p-2")           # 0x3FD34413509F6000
LOG10_2LO = np.uint64(0x3D59FEF311F12B36).view(np.float64)
KY_LO, KY_HI = -67, 1023                                 # every power of two of a positive normal double >= 1e-20


@pytest.fixture(scope="module")
def parked():
    """The device functions under test compiled for the host (test-only build)."""
    so = ROOT / "tests" / "_host_harness_parked.so"
    src = ROOT / "tests" / "host_harness_parked.cpp"
    hdrs = list((ROOT / "c2-ray3dm1d_helium_amd" / "csrc").glob("*.hpp"))
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(src)],
                       check=True)
    return C.CDLL(str(so))


def _check_log10(parked, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    what = (C.c_int * 1)(-1)
    bad = parked.hp_check_log10_through_table(C.c_int(x.size), x.ctypes.data_as(dp), what)
    assert bad == 0, (bad, what[0], float(x[what[0]]).hex())


def test_every_entry_is_the_pair_of_products(parked):
    lo, hi = C.c_int(), C.c_int()
    out = np.empty(2 * 2048)
    n = parked.hp_exponent_table(C.byref(lo), C.byref(hi), out.ctypes.data_as(dp), C.c_int(2048))
    assert lo.value <= KY_LO and hi.value >= KY_HI and n == hi.value - lo.value + 1
    assert float(LOG10_2HI).hex() == "0x1.34413509f6000p-2"
    y = np.arange(lo.value, hi.value + 1, dtype=np.float64)
    pairs = out[:2 * n].reshape(n, 2)
    assert np.array_equal(pairs[:, 0].view(np.uint64), (y * LOG10_2LO).view(np.uint64))
    assert np.array_equal(pairs[:, 1].view(np.uint64), (y * LOG10_2HI).view(np.uint64))
    assert np.array_equal(y[KY_LO - lo.value:KY_HI - lo.value + 1], np.arange(KY_LO, KY_HI + 1))


def test_log10_through_the_table_around_every_power_of_two(parked):
    p = np.ldexp(1.0, np.arange(-67, 61))
    _check_log10(parked, np.concatenate([np.nextafter(p, 0.0), p, np.nextafter(p, np.inf)]))
    # every exponent the table holds, away from the edges of a binade as well
    rng = np.random.default_rng(5)
    e = np.arange(-66, 1024)
    _check_log10(parked, np.ldexp(1.0 + rng.random(e.size) * 0.999, e))
    _check_log10(parked, np.ldexp(0.5 + rng.random(200_000) * 1.5, rng.integers(-66, 1023, 200_000)))


def test_log10_through_the_table_at_the_clamp(parked):
    _check_log10(parked, np.array([1.0e-20, np.nextafter(1.0e-20, 1.0)]))


def test_log10_through_the_table_on_the_boundaries_of_the_folded_log_table(parked):
    # every boundary of the 256 cases of gm::LogEntry, one ulp either side, in several binades
    hx = (np.uint64(0x3FE00000) + (np.arange(257, dtype=np.uint64) << np.uint64(13))) << np.uint64(32)
    edges = np.concatenate([(hx - np.uint64(1)).view(np.float64), hx.view(np.float64)])
    assert edges.size == 2 * 257 and np.isfinite(edges).all() and (edges > 0).all()
    _check_log10(parked, np.concatenate([np.ldexp(edges, s) for s in (0, -66, -40, -1, 1, 7, 60, 1000)]))


def test_lds_and_private_segment_of_the_isothermal_one_sed_rates_kernels(pkg, record_property):
    if not Path(READELF).exists():
        pytest.skip("llvm-readelf not present")
    notes = kernel_notes(pkg.build())
    iso = {name: v for name, v in notes.items() if re.search(r"7k_ratesILb0ELb0ELb[01]E", name)}
    assert len(iso) == 2, sorted(notes)
    for name, v in iso.items():
        print(f"{name}: {v['vgpr']} VGPRs, {v['lds']} bytes of LDS, private segment {v['private_segment']}")
        record_property(name, f"vgpr={v['vgpr']} lds={v['lds']}")
        # 160 KB of LDS per compute unit, five blocks of 256 lanes (five waves per SIMD): 32 KB each
        assert v["lds"] <= 160 * 1024 // 5, (name, v)
        assert v["private_segment"] == 0, (name, v)
