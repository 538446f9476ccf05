"""Open (non-periodic) mesh boundaries, c2r_set_boundaries(ctx, 0), against the oracle.  python -m pytest tests -m gpu.

The oracle is periodic only; tests/open_boundary_cases.py explains why its run on an M^3 mesh, M >= 2 N, with the box
at the mesh origin is nevertheless an exact reference for the open N^3 box (tests/test_open_boundaries_oracle.py checks
that premise on the oracle alone).  The bar is the project's: every grid bit for bit; the kept photon loss, one sum
whose order differs, to 1e-13 relative.
"""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import open_boundary_cases as ob
from conftest import rel_err

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
DT = 1.0e6 * 3.15576e7  # s


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


@pytest.fixture(scope="module")
def one_round(pkg):
    return ob.case_one_round(pkg)


@pytest.fixture(scope="module")
def several_rounds(pkg, orc, otables):
    case = ob.case_several_rounds(pkg)
    return case, case.oracle_pass(pkg, orc, otables)


def open_pass(e):
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    return e.download_rates()


def assert_grids_equal(got, ref, keys=("phih_grid", "phihe_grid")):
    for k in keys:
        assert np.array_equal(got[k], ref[k]), (k, float(np.max(rel_err(got[k], ref[k]))), int(np.count_nonzero(got[k] != ref[k])))


def shell_order(n, src):
    """The cells (1-based) of an n^3 box in L-infinity shells around `src`: upstream cells come first."""
    cells = [(i, j, k) for k in range(1, n + 1) for j in range(1, n + 1) for i in range(1, n + 1)]
    return sorted(cells, key=lambda c: max(abs(c[0] - src[0]), abs(c[1] - src[1]), abs(c[2] - src[2])))


def trace_by_point(e, n, src, ns=1):
    """c2r_evolve0d for every cell of the n^3 box at the mesh origin, in shell order; returns the losses of the cells
    on the box's boundary (index 1 or n along some axis), in call order."""
    losses = []
    for cell in shell_order(n, src):
        surface = any(x in (1, n) for x in cell)
        pos = (C.c_int * 3)(*cell)
        loss = C.c_double(0.0)
        e._chk(e.lib.c2r_evolve0d(e.h, pos, ns, 1, int(surface), C.byref(loss)))
        if surface:
            losses.append(loss.value)
    return np.array(losses)


@pytest.mark.parametrize("sources", [[0], [1], [2], [3], [4], [0, 1, 2, 3, 4]], ids=["corner", "opposite_corner", "edge", "face", "interior", "all"])
def test_one_round_every_kind_of_position(pkg, orc, otables, tables, one_round, sources):
    """N = 11 (every offset within the first sub-box), log-normal density, mixed ionisation; a source in a corner, in the
    opposite corner, on an edge, on a face, in the interior, and all together: rate grids after c2r_pass_sources, then the
    iteration state after one c2r_global_pass, equal to the oracle's on M = 24."""
    case = one_round
    ref = case.oracle_pass(pkg, orc, otables, sources, dt=DT)
    e = case.engine(pkg, tables, sources)
    assert e.periodic is False
    got = open_pass(e)
    assert_grids_equal(got, ref)
    assert np.all(got["phih_grid"] > 0)
    assert got["sum_nbox"] == len(sources)          # one round reaches every face
    e.global_pass(DT)
    assert_grids_equal(e.download_iter_state(), ref, ("xh_av", "xhe_av", "xh_intermed", "xhe_intermed"))
    e.close()


@pytest.mark.parametrize("batch", [1, 256])
def test_several_rounds_with_per_source_boxes(pkg, tables, several_rounds, batch):
    """N = 24, highly ionised gas, three corners, an edge and an interior cell: every source runs to its own reach, so
    the boxes of one round differ from source to source.  Grids equal to the oracle's on M = 48 whether the sources are
    swept one per batch or all in one; sum_nbox is the sum over sources of ceil(max_d(|l_d|, r_d) / subboxsize)."""
    case, ref = several_rounds
    e = case.engine(pkg, tables)
    e.set_batch(batch)
    got = open_pass(e)
    assert_grids_equal(got, ref)
    assert got["sum_nbox"] == case.expected_rounds() == 14
    # a second pass, now with what the first one learnt (block sizes, rounds swept without waiting for their loss)
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    again = e.download_rates()
    assert_grids_equal(again, ref)
    assert again["sum_nbox"] == 14 and again["photon_loss"][0] == got["photon_loss"][0]
    e.close()


_GENERIC_SNIPPET = r'''
import sys, numpy as np
sys.path.insert(0, "{root}"); sys.path.insert(0, "{root}/tests")
import __graft_entry__ as ge
import open_boundary_cases as ob
pkg = ge.load_package()
case = ob.case_several_rounds(pkg)
e = case.engine(pkg, pkg.RadiationTables.load())
e.begin_step(); e.set_rates_to_zero(); e.pass_sources(1, 1)
np.savez("{out}", **e.download_rates())
'''


def test_several_rounds_through_the_general_sweep_kernel(pkg, tables, several_rounds, tmp_path):
    """The same case with C2R_SWEEP_GENERIC=1 (read once per process, so in a process of its own): the open
    instantiation of k_sweep_shell for every shell instead of k_sweep_shell_fast -- the same bits."""
    case, ref = several_rounds
    out = tmp_path / "generic.npz"
    r = subprocess.run([sys.executable, "-c", _GENERIC_SNIPPET.format(root=str(ROOT), out=str(out))],
                       env={**os.environ, "C2R_SWEEP_GENERIC": "1"}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    assert_grids_equal(got, ref)
    assert int(got["sum_nbox"]) == 14


def test_early_stop_next_to_a_face(pkg, orc, otables, tables):
    """N = 24, opaque gas, sources at (3,12,12) and (12,12,12).  The oracle on M = 48 with opaque padding stops both after
    round 1.  The loss that decides in open mode is a subset of the oracle's non-negative terms, so open mode stops there
    too: sum_nbox == 2 and the same grids, exact zeros outside the first boxes included.  The photons that leave
    through the mesh face two cells from the first source are far more than 1e-10 of its flux (asserted below on the kept
    loss): if they counted for the decision, that source would sweep on."""
    case = ob.case_early_stop(pkg)
    ref = case.oracle_pass(pkg, orc, otables)
    assert ref["sum_nbox"] == 2
    e = case.engine(pkg, tables)
    got = open_pass(e)
    assert got["sum_nbox"] == 2
    assert_grids_equal(got, ref)
    assert 0 < np.count_nonzero(got["phih_grid"] == 0.0) == np.count_nonzero(ref["phih_grid"] == 0.0)
    e.close()
    # the kept loss of the first source alone: through the whole surface of its box, the mesh face at i = 1 included
    e = case.engine(pkg, tables, [0])
    alone = open_pass(e)
    assert alone["sum_nbox"] == 1
    print("kept loss / flux of the source at (3,12,12):", alone["photon_loss"][0] / (case.flux[0] * case.s_star))
    assert alone["photon_loss"][0] > 1e-10 * case.flux[0] * case.s_star
    e.close()


def test_heating(pkg, orc, otables, tables):
    """The one-round case with isothermal = 0, two sources (a corner and an edge): phiheat as well."""
    case = ob.case_one_round(pkg, heat=True)
    sources = [0, 2]
    ref = case.oracle_pass(pkg, orc, otables, sources, dt=DT)
    e = case.engine(pkg, tables, sources)
    got = open_pass(e)
    assert_grids_equal(got, ref, ("phih_grid", "phihe_grid", "phiheat"))
    assert np.all(got["phiheat"] > 0)
    e.global_pass(DT)
    assert_grids_equal(e.download_iter_state(), ref, ("xh_av", "xhe_av", "xh_intermed", "xhe_intermed"))
    e.close()


def test_heating_three_seds(pkg, orc, gold):
    """Black-body, power-law and quasar-like SEDs on sources of mixed kinds (the reference's -DPL -DQUASARS build), heating on."""
    if not (GOLD / "rad_tables_pl_qpl.npz").exists():
        pytest.skip("rad_tables_pl_qpl.npz not present")
    t = pkg.RadiationTables.load().add_sed_file(GOLD / "rad_tables_pl_qpl.npz")
    with np.load(pkg.evolve.DEFAULT_TABLES) as z:
        d = {k: z[k] for k in z.files}
    zz = gold("rad_tables_pl_qpl.npz")
    d.update({k: zz[k] for k in zz.files})
    T = orc.Tables(d)
    case = ob.case_one_round(pkg, heat=True, seds=True)
    ref = case.oracle_pass(pkg, orc, T)
    e = case.engine(pkg, t)
    got = open_pass(e)
    assert_grids_equal(got, ref, ("phih_grid", "phihe_grid", "phiheat"))
    e.close()


def test_kept_loss_is_the_sum_over_the_mesh_boundary(pkg, tables, one_round):
    """One source in the corner of the N = 11 box: photon_loss(1) is photo_out*vol/vol_ph summed over the cells on the
    mesh's boundary.  Expected value: the pinned per-cell route, c2r_evolve0d(..., on_surface, &loss), on a PERIODIC
    context of the M = 24 embedding, summed here.  1e-13 relative: the project's bound for this one sum, whose order
    differs (tests/test_gpu_parity.py)."""
    case = one_round
    n = case.n
    pe = case.periodic_engine_on_m(pkg, tables, [0])
    pe.begin_step()
    pe.set_rates_to_zero()
    terms = trace_by_point(pe, n, tuple(case.srcpos[0]))
    pe.close()
    assert terms.size == n ** 3 - (n - 2) ** 3 and np.all(terms >= 0) and np.count_nonzero(terms) > terms.size // 2
    expected = float(np.sum(np.sort(terms)))
    e = case.engine(pkg, tables, [0])
    got = open_pass(e)["photon_loss"][0]
    e.close()
    print("kept loss", got, "expected", expected, "rel", rel_err(got, expected))
    assert rel_err(got, expected) <= 1e-13


def test_the_switch_is_clean(pkg, tables, one_round):
    """Periodic, then open, then periodic again on one context: the two periodic results are identical and equal to a
    fresh context's; the open one equals a fresh open context's.  c2r_set_boundaries inside an open slab pass fails."""
    case = one_round
    fresh_p = case.engine(pkg, tables, periodic=True)
    ref_p = open_pass(fresh_p)
    fresh_p.close()
    fresh_o = case.engine(pkg, tables)
    ref_o = open_pass(fresh_o)
    fresh_o.close()
    assert not np.array_equal(ref_p["phih_grid"], ref_o["phih_grid"])    # a corner source lights the other corners up
    e = case.engine(pkg, tables, periodic=True)
    assert e.periodic is True
    keys = ("phih_grid", "phihe_grid", "photon_loss")
    p1 = open_pass(e)
    e.set_boundaries(False)
    assert e.periodic is False
    o = open_pass(e)
    e.set_boundaries(True)
    p2 = open_pass(e)
    for k in keys:
        assert np.array_equal(p1[k], ref_p[k]) and np.array_equal(p2[k], ref_p[k]) and np.array_equal(o[k], ref_o[k]), k
    assert p1["sum_nbox"] == p2["sum_nbox"] == ref_p["sum_nbox"] and o["sum_nbox"] == ref_o["sum_nbox"]
    e.set_rates_to_zero()
    e.pass_sources_begin(1, 1, 2)
    with pytest.raises(pkg.C2RayHipError, match="c2r_set_boundaries.*pass"):
        e.set_boundaries(False)
    e.pass_sources_end()
    assert e.periodic is True
    for k in keys:
        assert np.array_equal(e.download_rates()[k], ref_p[k]), k
    e.close()


def test_per_point_route(pkg, tables, one_round):
    """c2r_do_source and c2r_evolve0d in open mode reproduce the batched pass for the corner source of the one-round
    case: the same rate grids; the losses c2r_evolve0d returns for the boundary cells add up to the kept loss."""
    case = one_round
    n = case.n
    e = case.engine(pkg, tables, [0])
    ref = open_pass(e)
    e.set_rates_to_zero()
    e.do_source(1)
    got = e.download_rates()
    assert_grids_equal(got, ref)
    assert got["sum_nbox"] == 1 and got["photon_loss"][0] == ref["photon_loss"][0]
    e.set_rates_to_zero()
    terms = trace_by_point(e, n, tuple(case.srcpos[0]))
    assert_grids_equal(e.download_rates(), ref)
    assert rel_err(float(np.sum(np.sort(terms))), ref["photon_loss"][0]) <= 1e-13
    # a cell beyond the source's reach does not exist: refused, not wrapped
    pos = (C.c_int * 3)(n + 1, 1, 1)
    assert e.lib.c2r_evolve0d(e.h, pos, 1, 1, 0, None) != 0
    e.close()
