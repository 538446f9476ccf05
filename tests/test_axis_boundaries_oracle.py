"""The premise of tests/test_gpu_axis_boundaries.py, checked on the oracle alone (no GPU): the rates of a region at the
ORIGIN of a periodic mesh that has the region's extent on some axes and at least twice its extent on the others do not
depend on how large those others are or on the gas outside the region, bit for bit.  That makes the periodic oracle an
exact reference for a mesh that is periodic on the first kind of axis and open on the second
(tests/axis_boundary_cases.py)."""
import numpy as np
import pytest

import axis_boundary_cases as ab

DT = 1.0e6 * 3.15576e7  # s


@pytest.mark.parametrize("name", list(ab.CASES))
def test_origin_embedding_does_not_depend_on_the_open_axes_extent(pkg, orc, otables, name):
    case = ab.CASES[name](pkg)
    dt = DT if name == "E" else None
    a = case.oracle_pass(pkg, orc, otables, dt=dt)
    m2, pad_kind = ab.OTHER_EMBEDDING[name]
    assert all(x >= y for x, y in zip(m2, case.m)) and m2 != case.m
    b = case.oracle_pass(pkg, orc, otables, dt=dt, m=m2, big=case.embedding(pkg, m2, ab.OTHER_PAD_SEED, pad_kind))
    keys = ("phih_grid", "phihe_grid") + (("phiheat",) + ab.ITER_STATE if name == "E" else ())
    for k in keys:
        assert np.array_equal(a[k], b[k]), (name, k, int(np.count_nonzero(a[k] != b[k])))
    assert a["sum_nbox"] == ab.ORACLE_SUM_NBOX[name]
    if name == "F":
        # both sources stop after their first round; the cells beyond it were never traced: exact zeros
        assert a["phih_grid"].size == 13824 and np.count_nonzero(a["phih_grid"] == 0.0) == 4122
        assert np.count_nonzero(b["phih_grid"] == 0.0) == 4122
    else:
        assert np.all(a["phih_grid"] > 0)       # every cell of the region is reached
    if name == "E":
        assert np.all(a["phiheat"] > 0)
    if name == "C":
        # the columns of the source swept last (tests/test_gpu_axis_boundaries.py compares c2r_download_columns with them)
        for k in ("coldensh_out", "coldenshe_out"):
            assert np.array_equal(a[k], b[k]) and np.all(a[k] > 0), k


def test_rounds_the_product_is_expected_to_need(pkg):
    """Sum over sources of ceil(max_d(|l_d|, r_d) / subboxsize) with the reach per axis: not the oracle's count, which keeps
    growing in z up to M_z/2."""
    assert ab.case_a(pkg).expected_rounds() == 3 + 3 + 3 + 2 + 3 == 14
    assert ab.case_a(pkg).reach(3) == ([-12, -12, -11], [11, 11, 12])
    assert ab.case_b(pkg).expected_rounds() == 2 + 2 + 2 + 2
    assert ab.case_b(pkg).reach(2) == ([-5, -12, -12], [5, 11, 11])
    assert ab.case_c(pkg).expected_rounds() == 8
    assert ab.case_d(pkg).expected_rounds() == 3 + 3 + 2 + 3
    assert ab.case_e(pkg).expected_rounds() == 4
    assert ab.case_e(pkg).reach(0) == ([-5, -5, 0], [5, 5, 10])


def test_embedding_helpers_round_trip_on_a_mesh_that_is_no_cube():
    rng = np.random.default_rng(5)
    n, m = (3, 2, 4), (7, 2, 9)
    region, pad = rng.random(2 * ab.cells(n)), rng.random(2 * ab.cells(m))
    big = ab.embed3(region, n, m, pad)
    assert np.array_equal(ab.extract3(big, n, m), region)
    # cell (i, j, k) = (2, 1, 3) (0-based) of component 1 sits at i + m1 (j + m2 k) in the large mesh
    assert big[ab.cells(m) + 2 + 7 * (1 + 2 * 3)] == region[ab.cells(n) + 2 + 3 * (1 + 2 * 3)]
    assert big[ab.cells(m) + 3] == pad[ab.cells(m) + 3] and big[7 * 2 * 4] == pad[7 * 2 * 4]
    same = ab.embed3(region, n, n, rng.random(2 * ab.cells(n)))
    assert np.array_equal(same, region)
