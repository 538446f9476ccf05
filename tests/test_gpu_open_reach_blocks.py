"""Open boundaries: column blocks and shell launches sized by each source's reach (the reach-cut shell order of
csrc/c2ray_shell.hpp), and c2r_get_source_trace.  python -m pytest tests -m gpu.

Expected values are the oracle's, or the product's own PERIODIC run on an embedding mesh (the pinned path), as
tests/open_boundary_cases.py explains; every grid bit for bit.  What a source's trace cost -- entries of its block, threads
of its shell launches -- is compared with what its reach allows, worked out here.
"""
import ctypes as C

import numpy as np
import pytest

import open_boundary_cases as ob
from conftest import rel_err

pytestmark = pytest.mark.gpu
DT = 1.0e6 * 3.15576e7  # s
BLOCK = 256             # threads of a sweep block


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


@pytest.fixture(scope="module")
def several_rounds(pkg, orc, otables):
    case = ob.case_several_rounds(pkg)
    return case, case.oracle_pass(pkg, orc, otables)


def one_pass(e):
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    return e.download_rates()


def assert_grids_equal(got, ref, keys=("phih_grid", "phihe_grid")):
    for k in keys:
        assert np.array_equal(got[k], ref[k]), (k, float(np.max(rel_err(got[k], ref[k]))), int(np.count_nonzero(got[k] != ref[k])))


def cut_cells(mesh, pos, cap):
    """Cells of the shells 0..cap around `pos` (1-based) within an open mesh: prod_d (min(cap, r_d) + min(cap, -l_d) + 1)."""
    return int(np.prod([min(cap, n - p) + min(cap, p - 1) + 1 for n, p in zip(mesh, pos)]))


@pytest.mark.parametrize("batch", [1, 256])
def test_block_holds_the_cells_within_reach(pkg, tables, several_rounds, batch):
    """N = 24, three corners, an edge and an interior cell: after the pass every source's block has
    prod_d (min(cap, r_d) + min(cap, -l_d) + 1) entries per array, cap = the shells it holds -- never more than the 24^3
    cells of the mesh (uncut, a corner source's block at the mesh limit has 47^3 = 103 823 entries, the interior source's
    35^3 = 42 875).  Grids equal to the oracle's."""
    case, ref = several_rounds
    n = case.n
    e = case.engine(pkg, tables)
    e.set_batch(batch)
    for ns in range(1, len(case.flux) + 1):           # nothing swept yet: the reach, and zeros
        t = e.source_trace(ns)
        assert t["nbox"] == 0 and t["block_cells"] == 0 and t["sweep_threads"] == 0
        assert t["reach_r"] == [n - int(p) for p in case.srcpos[ns - 1]]
    got = one_pass(e)
    assert_grids_equal(got, ref)
    assert got["sum_nbox"] == case.expected_rounds()
    nbox = 0
    for ns in range(1, len(case.flux) + 1):
        pos = [int(p) for p in case.srcpos[ns - 1]]
        t = e.source_trace(ns)
        print(ns, pos, t)
        assert t["reach_l"] == [1 - p for p in pos] and t["reach_r"] == [n - p for p in pos]
        reach = max(max(p - 1, n - p) for p in pos)
        assert t["block_shells"] >= reach              # ionised gas: the source ran to its reach
        assert t["block_cells"] == cut_cells((n, n, n), pos, t["block_shells"])
        assert t["block_cells"] <= n ** 3
        assert t["box_lo"] == t["reach_l"] and t["box_hi"] == t["reach_r"]
        assert t["swept_cells"] == n ** 3
        assert t["nbox"] == -(-reach // ob.SUBBOXSIZE)
        nbox += t["nbox"]
    assert nbox == got["sum_nbox"]
    e.close()


def test_shell_launches_hold_the_cut_shells(pkg, tables, several_rounds):
    """One source in the corner (1,1,1) of the N = 24 box, swept alone: it traces 24^3 cells, and each of its 24 shell
    launches rounds the cells of the cut shell up by less than one block (uncut shells: 107 520 threads)."""
    case, ref_all = several_rounds
    n = case.n
    e = case.engine(pkg, tables, [0])
    e.set_batch(1)
    one_pass(e)
    t = e.source_trace(1)
    print(t)
    assert t["swept_cells"] == n ** 3 == 13824
    expected = sum(-(-((s + 1) ** 3 - s ** 3) // BLOCK) * BLOCK for s in range(n))
    assert t["sweep_threads"] == expected
    assert t["sweep_threads"] < t["swept_cells"] + BLOCK * n
    e.close()


def test_a_block_that_moves(pkg, tables):
    """N = 56, ionised gas, one source at (1,1,1): its reach is 55, the first block of four rounds holds 40 shells and
    moves in round 5 (a prefix of each half of a cut block is a cut block).  Rate grids equal, bit for bit, the product's
    periodic run on M = 112 (112/2 - 1 = 55); a second pass, with the block size the first one learnt, gives the same bits."""
    n, m = 56, 112
    case = ob.Case(pkg, n, m, "ionised", np.array([[1, 1, 1]], dtype=np.int32), np.array([2.0e7]), seed=5656)
    pe = case.periodic_engine_on_m(pkg, tables)
    big = one_pass(pe)
    pe.close()
    ref = {k: ob.extract(big[k], n, m) for k in ("phih_grid", "phihe_grid")}
    e = case.engine(pkg, tables)
    moves0 = e.arena_stats()["block_moves"]
    got = one_pass(e)
    t = e.source_trace(1)
    print(t, e.arena_stats())
    assert e.arena_stats()["block_moves"] - moves0 >= 1
    assert_grids_equal(got, ref)
    assert np.all(got["phih_grid"] > 0)
    assert got["sum_nbox"] == 6 and t["nbox"] == 6
    assert t["block_shells"] >= 55 and t["block_cells"] == cut_cells((n, n, n), (1, 1, 1), t["block_shells"]) == n ** 3
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    again = e.download_rates()
    assert_grids_equal(again, ref)
    assert again["sum_nbox"] == 6 and again["photon_loss"][0] == got["photon_loss"][0]
    assert e.source_trace(1)["block_cells"] == n ** 3
    e.close()


# -- a mesh that is no cube -------------------------------------------------------------------------------------------
def embed3(region, n, m, pad):
    """The (n1,n2,n3) region (components, i fastest) at the origin of an (m1,m2,m3) mesh filled with `pad`."""
    region, pad = np.asarray(region), np.asarray(pad)
    ncomp = region.size // (n[0] * n[1] * n[2])
    out = pad.reshape(ncomp, m[2], m[1], m[0]).copy()
    out[:, :n[2], :n[1], :n[0]] = region.reshape(ncomp, n[2], n[1], n[0])
    return out.reshape(-1)


def extract3(big, n, m):
    big = np.asarray(big)
    ncomp = big.size // (m[0] * m[1] * m[2])
    return np.ascontiguousarray(big.reshape(ncomp, m[2], m[1], m[0])[:, :n[2], :n[1], :n[0]]).reshape(-1)


def engine3(pkg, tables, mesh, gas, dr, vol, srcpos, flux, periodic):
    hp = pkg.hostphys
    ndens, xh, xhe, _ = gas
    mat = pkg.Material(ndens, xh.copy(), xhe.copy(), None, True, 1.0e4, 1.0, hp.reccoef(1.0e4))
    e = pkg.HipEngine(tuple(mesh), 0)
    e.set_boundaries(periodic)
    e.set_tables(tables)
    e.set_step(mat, pkg.GridProps(tuple(mesh), dr, vol), pkg.Cosmology(ob.ZRED, hp.H0, hp.Omega0))
    e.set_sources(pkg.SourceProps(srcpos, flux, 1.0e48))
    e.upload_state(mat)
    return e


def test_non_cubic_mesh_with_lopsided_reaches(pkg, tables):
    """An open 13 x 9 x 6 mesh, sources in two opposite corners, on a face and inside: reaches that differ per axis and
    per side.  Against the product's periodic run on 28 x 24 x 24 with the box at the origin (M_d >= 2 N_d, M_d/2 - 1 no
    multiple of 10): rate grids, then xh_av / xhe_av after one global pass."""
    n, m = (13, 9, 6), (28, 24, 24)
    srcpos = np.array([[1, 1, 1], [13, 9, 6], [4, 9, 2], [7, 5, 3]], dtype=np.int32)
    flux = np.array([2.0e7, 1.0e7, 1.5e7, 3.0e7])
    dr, vol = pkg.hostphys.test_grid(13, ob.ZRED)
    region = ob.gas(pkg, n[0] * n[1] * n[2], np.random.default_rng(1396), "ionised", False)
    pad = ob.gas(pkg, m[0] * m[1] * m[2], np.random.default_rng(2396), "ionised", False)
    big = [embed3(a, n, m, b) for a, b in zip(region[:3], pad[:3])] + [None]
    pe = engine3(pkg, tables, m, big, dr, vol, srcpos, flux, True)
    ref = one_pass(pe)
    pe.global_pass(DT)
    ref.update(pe.download_iter_state())
    pe.close()
    e = engine3(pkg, tables, n, region, dr, vol, srcpos, flux, False)
    got = one_pass(e)
    for k in ("phih_grid", "phihe_grid"):
        assert np.array_equal(got[k], extract3(ref[k], n, m)), (k, int(np.count_nonzero(got[k] != extract3(ref[k], n, m))))
    assert np.all(got["phih_grid"] > 0)
    cells = n[0] * n[1] * n[2]
    for ns in range(1, 5):
        pos = [int(p) for p in srcpos[ns - 1]]
        t = e.source_trace(ns)
        print(ns, pos, t)
        assert t["reach_l"] == [1 - p for p in pos] and t["reach_r"] == [a - p for a, p in zip(n, pos)]
        assert t["box_lo"] == t["reach_l"] and t["box_hi"] == t["reach_r"] and t["swept_cells"] == cells
        assert t["block_cells"] == cut_cells(n, pos, t["block_shells"]) == cells
    e.global_pass(DT)
    st = e.download_iter_state()
    for k in ("xh_av", "xhe_av"):
        assert np.array_equal(st[k], extract3(ref[k], n, m)), k
    e.close()


# -- columns and the per-point route ----------------------------------------------------------------------------------
def shell_order(n, src):
    cells = [(i, j, k) for k in range(1, n + 1) for j in range(1, n + 1) for i in range(1, n + 1)]
    return sorted(cells, key=lambda c: max(abs(c[0] - src[0]), abs(c[1] - src[1]), abs(c[2] - src[2])))


def trace_by_point(e, n, src, ns=1):
    """c2r_evolve0d for every cell of the n^3 box, in shell order; the losses of the cells on the box's boundary."""
    losses = []
    for cell in shell_order(n, src):
        surface = any(x in (1, n) for x in cell)
        pos = (C.c_int * 3)(*cell)
        loss = C.c_double(0.0)
        e._chk(e.lib.c2r_evolve0d(e.h, pos, ns, 1, int(surface), C.byref(loss)))
        if surface:
            losses.append(loss.value)
    return np.array(losses)


def test_downloaded_columns_of_a_corner_source(pkg, tables):
    """c2r_download_columns after an open N = 11 pass of the corner source: the columns of the periodic M = 24 run on the
    same region."""
    case = ob.case_one_round(pkg)
    pe = case.periodic_engine_on_m(pkg, tables, [0])
    one_pass(pe)
    ref = pe.download_columns()
    pe.close()
    e = case.engine(pkg, tables, [0])
    one_pass(e)
    got = e.download_columns()
    e.close()
    for k in ("coldensh_out", "coldenshe_out"):
        want = ob.extract(ref[k], case.n, case.m)
        assert np.all(want > 0)
        assert np.array_equal(got[k], want), (k, int(np.count_nonzero(got[k] != want)))


def test_per_point_route_of_an_edge_source(pkg, tables):
    """c2r_do_source and c2r_evolve0d in open mode for the source on an edge, (5,11,1) of the N = 11 box: the rate grids of
    the batched pass; the losses c2r_evolve0d returns for the boundary cells add up to the kept loss (1e-13 relative, the
    project's bound for this one sum, whose order differs)."""
    case = ob.case_one_round(pkg)
    n = case.n
    e = case.engine(pkg, tables, [2])
    ref = one_pass(e)
    e.set_rates_to_zero()
    e.do_source(1)
    got = e.download_rates()
    assert_grids_equal(got, ref)
    assert got["sum_nbox"] == 1 and got["photon_loss"][0] == ref["photon_loss"][0]
    e.set_rates_to_zero()
    terms = trace_by_point(e, n, tuple(case.srcpos[2]))
    assert_grids_equal(e.download_rates(), ref)
    assert rel_err(float(np.sum(np.sort(terms))), ref["photon_loss"][0]) <= 1e-13
    e.close()


def test_source_trace_with_periodic_boundaries(pkg, tables, several_rounds):
    """Periodic mode keeps its layout: block_cells == (2 block_shells + 1)^3, the rounds add up to sum_nbox, the reach is
    the mesh's."""
    case, _ = several_rounds
    n = case.n
    e = case.engine(pkg, tables, periodic=True)
    got = one_pass(e)
    nbox = 0
    for ns in range(1, len(case.flux) + 1):
        t = e.source_trace(ns)
        assert t["reach_l"] == [-(n // 2)] * 3 and t["reach_r"] == [n // 2 - 1] * 3
        assert t["nbox"] >= 1 and t["block_cells"] == (2 * t["block_shells"] + 1) ** 3
        assert t["swept_cells"] == int(np.prod([h - l + 1 for l, h in zip(t["box_lo"], t["box_hi"])]))
        assert t["sweep_threads"] >= t["swept_cells"]
        nbox += t["nbox"]
    assert nbox == got["sum_nbox"]
    with pytest.raises(pkg.C2RayHipError, match="c2r_get_source_trace"):
        e.source_trace(len(case.flux) + 1)
    e.close()
