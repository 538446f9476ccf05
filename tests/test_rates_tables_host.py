"""The two tables that the rates kernels read instead of computing, on the CPU: where an entry stands.

 * The pair copy of the photo table: entry (band b, row r) is {c[r], c[r + 1] - c[r]}, 16 bytes, at b * 2002 + r; a
   position is read at the byte offset ipos << 4 of its band's column, and the interpolation c + d * residual gives the
   bits of read_table's a + (b - a) * residual on the column itself -- on ordinary rows, on equal neighbours, on the
   duplicated last row and where the difference is subnormal.
 * The shell volumes: an axis of n cells whose offsets run from -l to n - 1 - l (l = n / 2) holds the magnitudes
   0 .. max(l, n - 1 - l), and (|di|, |dj|, |dk|) -> |di| + e1 * (|dj| + e2 * |dk|) fills [0, e1 * e2 * e3) exactly once.
Through a small harness of its own (tests/rates_tables_harness.cpp)."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NFREQ = 47


@pytest.fixture(scope="module")
def rt():
    so = ROOT / "tests" / "_rates_tables_harness.so"
    src = ROOT / "tests" / "rates_tables_harness.cpp"
    hdrs = list((ROOT / "c2-ray3dm1d_helium_amd" / "csrc").glob("*.hpp"))
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(src)],
                       check=True)
    lib = C.CDLL(str(so))
    lib.rt_pair_index.restype = C.c_longlong
    lib.rt_shell_index.restype = C.c_longlong
    lib.rt_read_pairs.restype = C.c_double
    lib.rt_read_pairs.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_double, C.POINTER(C.c_longlong)]
    lib.rt_read_table.restype = C.c_double
    lib.rt_read_table.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_double]
    return lib


def test_pair_entries_are_16_bytes_band_after_band(rt):
    ntau, pitch = rt.rt_ntau(), rt.rt_pitch()
    assert (ntau, pitch) == (2000, 2002)
    assert rt.rt_pair_size() == 16 and rt.rt_pair_align() == 16
    seen = set()
    for b in range(NFREQ):
        for r in (0, 1, ntau - 1, ntau, ntau + 1):
            q = rt.rt_pair_index(b, r)
            assert q == b * pitch + r
            seen.add(q)
    assert len(seen) == NFREQ * 5 and max(seen) == NFREQ * pitch - 1
    assert rt.rt_pair_index(NFREQ, 0) == NFREQ * pitch            # entries of the whole copy


def test_pairs_interpolate_to_the_bits_of_the_table(rt):
    ntau, pitch = rt.rt_ntau(), rt.rt_pitch()
    rng = np.random.default_rng(20261020)
    col = np.sort(10.0 ** rng.uniform(-30.0, 3.0, pitch))[::-1].copy()
    col[100:104] = col[100]                    # equal neighbours: difference +0
    col[1500] = 3.0e-310                       # two neighbours whose difference is subnormal
    col[1501] = 1.0e-310
    col[1502:] = 0.0                           # a run of exact zeros at the end
    col[ntau + 1] = col[ntau]                  # the duplicated row
    pc = col.ctypes.data_as(C.POINTER(C.c_double))
    off = C.c_longlong(-1)
    rows = [0, 1, 99, 100, 101, 103, 1499, 1500, 1501, 1502, ntau - 1, ntau] + [int(r) for r in rng.integers(0, ntau + 1, 200)]
    for ipos in rows:
        for res in [0.0, 0.5, float(np.nextafter(1.0, 0.0))] + [float(x) for x in rng.uniform(0.0, 1.0, 5)]:
            got = rt.rt_read_pairs(pc, ipos, res, C.byref(off))
            want = rt.rt_read_table(pc, ipos, res)
            assert off.value == 16 * ipos
            assert np.float64(got).tobytes() == np.float64(want).tobytes(), (ipos, res, got, want)
    assert rt.rt_read_pairs(pc, ntau, 0.75, C.byref(off)) == col[ntau]      # the last used row: difference exactly 0


@pytest.mark.parametrize("mesh", [(1, 1, 1), (2, 2, 2), (9, 7, 5)], ids=lambda m: "x".join(map(str, m)))
def test_shell_volume_extents_and_positions(rt, mesh):
    assert rt.rt_shell_size() == 16
    ext = []
    for n in mesh:
        l = n // 2
        e = rt.rt_shell_extent(n, l)
        mags = {abs(o) for o in range(-l, n - l)}          # every offset of the axis: -l .. n - 1 - l
        assert len(range(-l, n - l)) == n
        assert mags == set(range(e)), (n, e)               # all of them fit, and the largest one is used
        ext.append(e)
    assert ext == {(1, 1, 1): [1, 1, 1], (2, 2, 2): [2, 2, 2], (9, 7, 5): [5, 4, 3]}[mesh]
    e1, e2, e3 = ext
    pos = [rt.rt_shell_index(ia, ja, ka, e1, e2) for ka, ja, ia in itertools.product(range(e3), range(e2), range(e1))]
    assert pos == list(range(e1 * e2 * e3))                # |di| fastest, no gaps, nothing twice
    assert rt.rt_shell_index(0, 0, 0, e1, e2) == 0         # the source's own cell
