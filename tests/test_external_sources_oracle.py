"""The premise of tests/test_gpu_external_sources.py, checked on the oracle alone (no GPU): with a source OUTSIDE an n^3 region
that sits at the origin of a periodic M^3 mesh of vacuum (ndens = 0 around the region), the source at its position as given
(positions <= 0 included), the rates of the region's cells do not depend on M or on the fractions stored in the vacuum, bit for
bit, and every one of them is finite and positive.  That makes the periodic oracle an exact reference for
c2r_set_sources_external (tests/external_source_cases.py)."""
import numpy as np
import pytest

import external_source_cases as xc


@pytest.mark.parametrize("kind", list(xc.PREMISE_SOURCES))
def test_vacuum_embedding_does_not_depend_on_the_mesh_around_it(pkg, orc, otables, kind):
    """n = 8, log-normal "mixed" gas; a source beyond a high face, beyond a low face (a position <= 0), beyond an edge, and an
    outside source together with an inside one: M = 24 and M = 28 (other fractions in the vacuum) give identical bits."""
    case = xc.case_premise(pkg, kind)
    assert any(case.is_external(ns) for ns in range(len(case.flux)))
    with np.errstate(all="ignore"):
        a = case.oracle_pass(pkg, orc, otables)
        b = case.oracle_pass(pkg, orc, otables, m=(28, 28, 28), big=case.embedding(pkg, (28, 28, 28), 77, "ionised"))
    for k in ("phih_grid", "phihe_grid"):
        assert np.array_equal(a[k], b[k]), (kind, k)
        assert np.all(np.isfinite(a[k])) and np.all(a[k] > 0), (kind, k)


def test_the_vacuum_is_vacuum(pkg):
    case = xc.case_premise(pkg, "beyond_low")
    nd = case.big[0].reshape(24, 24, 24)
    assert np.all(nd[:8, :8, :8] > 0) and np.count_nonzero(nd) == 8 ** 3
    assert case.reach(0) == ([-3, -4, 0], [4, 3, 10])                 # (4,5,-2) in 8^3: through two cells of vacuum to k = 8
    assert case.virtual_bounds() == ([1, 1, -2], [8, 8, 8]) and case.virtual_shift() == [0, 0, 3]
