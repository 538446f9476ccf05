"""The premise of tests/test_gpu_open_boundaries.py, checked on the oracle alone (no GPU): the rates of an N^3 region
at the ORIGIN of a periodic M^3 mesh, M >= 2 N, do not depend on M or on the gas outside the region, bit for bit --
a cell's rates depend only on the cells between it and the source.  That makes the periodic oracle an exact
reference for a box whose boundaries are open."""
import numpy as np
import pytest

import open_boundary_cases as ob


@pytest.mark.parametrize("which,m2,pad_kind", [("one_round", 31, "ionised"), ("several_rounds", 50, "mixed"), ("early_stop", 50, "opaque")])
def test_origin_embedding_does_not_depend_on_the_mesh_around_it(pkg, orc, otables, which, m2, pad_kind):
    case = {"one_round": ob.case_one_round, "several_rounds": ob.case_several_rounds, "early_stop": ob.case_early_stop}[which](pkg)
    a = case.oracle_pass(pkg, orc, otables)
    m, big = case.other_embedding(pkg, m2, pad_seed=77, pad_kind=pad_kind)
    b = case.oracle_pass(pkg, orc, otables, m=m, big=big)
    for k in ("phih_grid", "phihe_grid"):
        assert np.array_equal(a[k], b[k]), k
    if which == "early_stop":
        # both sources stop after their first round; cells beyond it were never traced: exact zeros
        assert a["sum_nbox"] == b["sum_nbox"] == 2
        assert 0.3 < np.count_nonzero(a["phih_grid"]) / a["phih_grid"].size < 0.9
    else:
        assert np.all(a["phih_grid"] > 0)       # every cell of the region is reached
    if which == "several_rounds":
        # every source goes through all three rounds of the periodic mesh, and the open box needs as many from a corner
        for ns in range(len(case.flux)):
            st, s = case.oracle_step(pkg, orc)
            nbox, loss = orc.do_source(otables, st, s, ns + 1)
            assert nbox == 3 and loss > 0.1 * case.flux[ns] * case.s_star
        assert case.expected_rounds() == 3 + 3 + 3 + 3 + 2


def test_embedding_helpers_round_trip():
    rng = np.random.default_rng(5)
    n, m = 3, 7
    region, pad = rng.random(2 * n ** 3), rng.random(2 * m ** 3)
    big = ob.embed(region, n, m, pad)
    assert np.array_equal(ob.extract(big, n, m), region)
    # cell (i, j, k) = (2, 1, 0) (0-based) of component 1 sits at i + m (j + m k) in the large mesh
    assert big[m ** 3 + 2 + m * 1] == region[n ** 3 + 2 + n * 1]
    assert big[m ** 3 + n] == pad[m ** 3 + n]
