"""Mesh boundaries per axis, c2r_set_boundaries_axes: periodic on some axes, open on the others, against the oracle.
python -m pytest tests -m gpu.

The oracle is periodic only; tests/axis_boundary_cases.py explains why its run on a mesh with the product's extent on the
periodic axes and at least twice that on the open ones, the region at the origin, is nevertheless an exact reference
(tests/test_axis_boundaries_oracle.py checks that premise on the oracle alone).  The bar is the project's: every grid bit
for bit; the kept photon loss, one sum whose order differs, to 1e-13 relative.
"""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import axis_boundary_cases as ab
from conftest import rel_err

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
DT = 1.0e6 * 3.15576e7  # s
RATES = ("phih_grid", "phihe_grid")


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


@pytest.fixture(scope="module")
def case_a(pkg, orc, otables):
    case = ab.case_a(pkg)
    return case, case.oracle_pass(pkg, orc, otables)


def one_pass(e):
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    return e.download_rates()


def assert_grids_equal(got, ref, keys=RATES):
    for k in keys:
        assert np.array_equal(got[k], ref[k]), (k, float(np.max(rel_err(got[k], ref[k]))), int(np.count_nonzero(got[k] != ref[k])))


@pytest.mark.parametrize("batch", [1, 256])
def test_a_z_open(pkg, tables, case_a, batch):
    """A: 24^3, z open, highly ionised gas, two corners, an edge, an interior cell and a face.  Grids equal to the oracle's
    on (24,24,48) whether the sources are swept one per batch or all in one; sum_nbox is the sum over sources of
    ceil(max_d(|l_d|, r_d) / subboxsize), not the oracle's 15; a second pass, with what the first one learnt, gives the same
    bits and the same kept loss."""
    case, ref = case_a
    e = case.engine(pkg, tables)
    assert e.periodic is None and e.periodic_axes == (True, True, False)
    e.set_batch(batch)
    got = one_pass(e)
    assert_grids_equal(got, ref)
    assert got["sum_nbox"] == case.expected_rounds() == 14
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    again = e.download_rates()
    assert_grids_equal(again, ref)
    assert again["sum_nbox"] == 14 and again["photon_loss"][0] == got["photon_loss"][0]
    e.close()


@pytest.mark.parametrize("name", ["B", "C", "D"])
def test_other_masks_on_meshes_that_are_no_cubes(pkg, orc, otables, tables, name):
    """B: (11,24,24) with x open, C: (11,11,24) with x and y open, D: (11,24,24) with x and z open."""
    case = ab.CASES[name](pkg)
    ref = case.oracle_pass(pkg, orc, otables)
    e = case.engine(pkg, tables)
    assert e.periodic_axes == case.periodic
    got = one_pass(e)
    assert_grids_equal(got, ref)
    assert np.all(got["phih_grid"] > 0)
    assert got["sum_nbox"] == case.expected_rounds() == {"B": 8, "C": 8, "D": 11}[name]
    e.close()


def test_e_heating(pkg, orc, otables, tables):
    """E: 11^3, z open, mixed ionisation, isothermal = 0: phiheat as well, then the iteration state after one global pass."""
    case = ab.case_e(pkg)
    ref = case.oracle_pass(pkg, orc, otables, dt=DT)
    e = case.engine(pkg, tables)
    got = one_pass(e)
    assert_grids_equal(got, ref, RATES + ("phiheat",))
    assert np.all(got["phiheat"] > 0)
    assert got["sum_nbox"] == case.expected_rounds() == 4
    e.global_pass(DT)
    assert_grids_equal(e.download_iter_state(), ref, ab.ITER_STATE)
    e.close()


def test_e_heating_three_seds(pkg, orc, gold):
    """E with black-body, power-law and quasar-like SEDs on sources of mixed kinds (the reference's -DPL -DQUASARS build)."""
    if not (GOLD / "rad_tables_pl_qpl.npz").exists():
        pytest.skip("rad_tables_pl_qpl.npz not present")
    t = pkg.RadiationTables.load().add_sed_file(GOLD / "rad_tables_pl_qpl.npz")
    with np.load(pkg.evolve.DEFAULT_TABLES) as z:
        d = {k: z[k] for k in z.files}
    zz = gold("rad_tables_pl_qpl.npz")
    d.update({k: zz[k] for k in zz.files})
    case = ab.case_e(pkg, seds=True)
    ref = case.oracle_pass(pkg, orc, orc.Tables(d))
    e = case.engine(pkg, t)
    got = one_pass(e)
    assert_grids_equal(got, ref, RATES + ("phiheat",))
    e.close()


def test_f_early_stop_next_to_the_open_face(pkg, orc, otables, tables):
    """F: 24^3, z open, opaque gas, sources at (12,12,3) and (12,12,12).  The oracle on (24,24,48) with opaque padding stops
    both after round 1; the loss that decides in the product is a subset of the oracle's non-negative terms, so it stops
    there too: the same grids, exact zeros outside the first boxes included.  The photons that leave through the open face
    two cells from the first source are far more than 1e-10 of its flux: if they counted for the decision, it would sweep on."""
    case = ab.case_f(pkg)
    ref = case.oracle_pass(pkg, orc, otables)
    assert ref["sum_nbox"] == 2
    e = case.engine(pkg, tables)
    got = one_pass(e)
    assert got["sum_nbox"] == 2
    assert_grids_equal(got, ref)
    assert np.count_nonzero(got["phih_grid"] == 0.0) == np.count_nonzero(ref["phih_grid"] == 0.0) == 4122
    e.close()
    e = case.engine(pkg, tables, [0])
    alone = one_pass(e)
    assert alone["sum_nbox"] == 1
    print("kept loss / flux of the source at (12,12,3):", alone["photon_loss"][0] / (case.flux[0] * case.s_star))
    assert alone["photon_loss"][0] > 1e-10 * case.flux[0] * case.s_star
    e.close()


_GENERIC_SNIPPET = r'''
import sys, numpy as np
sys.path.insert(0, "{root}"); sys.path.insert(0, "{root}/tests")
import __graft_entry__ as ge
import axis_boundary_cases as ab
pkg = ge.load_package()
case = ab.case_a(pkg)
e = case.engine(pkg, pkg.RadiationTables.load())
e.begin_step(); e.set_rates_to_zero(); e.pass_sources(1, 1)
np.savez("{out}", **e.download_rates())
e.close()
'''


def test_a_through_the_general_sweep_kernel(case_a, tmp_path):
    """A with C2R_SWEEP_GENERIC=1 (read once per process, so in a process of its own): the open instantiation of
    k_sweep_shell for every shell instead of k_sweep_shell_fast -- the same bits."""
    case, ref = case_a
    out = tmp_path / "generic.npz"
    r = subprocess.run([sys.executable, "-c", _GENERIC_SNIPPET.format(root=str(ROOT), out=str(out))],
                       env={**os.environ, "C2R_SWEEP_GENERIC": "1"}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    assert_grids_equal(got, ref)
    assert int(got["sum_nbox"]) == 14


def test_kept_loss_is_the_sum_over_the_surface_of_the_final_box(pkg, tables):
    """E's corner source (1,1,1) alone, isothermal: its final box is [-5,5] x [-5,5] x [0,10] -- the whole of both periodic
    axes, the open one from face to face -- and photon_loss(1) is photo_out*vol/vol_ph summed over its whole surface.
    Expected value: the pinned per-cell route, c2r_evolve0d(..., on_surface, &loss), on an all-periodic context of the
    (11,11,24) embedding, over the cells of that box in shell order, summed here.  1e-13 relative: the project's bound for
    this one sum, whose order differs (tests/test_gpu_parity.py)."""
    case = ab.case_e(pkg, heat=False)
    lo, hi = case.reach(0)
    assert (lo, hi) == ([-5, -5, 0], [5, 5, 10])
    offsets = [(i, j, k) for k in range(lo[2], hi[2] + 1) for j in range(lo[1], hi[1] + 1) for i in range(lo[0], hi[0] + 1)]
    offsets.sort(key=lambda o: max(abs(o[0]), abs(o[1]), abs(o[2])))       # upstream cells come first
    pe = case.periodic_engine_on_m(pkg, tables, [0])
    pe.begin_step()
    pe.set_rates_to_zero()
    terms = []
    for o in offsets:
        surface = any(x in (a, b) for x, a, b in zip(o, lo, hi))
        pos = (C.c_int * 3)(*(int(p) + x for p, x in zip(case.srcpos[0], o)))   # not wrapped: rtpos - srcpos is the offset
        loss = C.c_double(0.0)
        pe._chk(pe.lib.c2r_evolve0d(pe.h, pos, 1, 1, int(surface), C.byref(loss)))
        if surface:
            terms.append(loss.value)
    pe.close()
    terms = np.array(terms)
    assert terms.size == 11 ** 3 - 9 ** 3 and np.all(terms >= 0) and np.count_nonzero(terms) > terms.size // 2
    expected = float(np.sum(np.sort(terms)))
    e = case.engine(pkg, tables, [0])
    got = one_pass(e)
    e.close()
    assert got["sum_nbox"] == 1
    print("kept loss", got["photon_loss"][0], "expected", expected, "rel", rel_err(got["photon_loss"][0], expected))
    assert rel_err(got["photon_loss"][0], expected) <= 1e-13


def test_the_switch(pkg, tables):
    """{0,0,0} through the new entry point is c2r_set_boundaries(ctx, 0), {1,1,1} a fresh periodic context; periodic ->
    z-open -> periodic -> z-open on one context matches fresh contexts each time; the call is refused inside an open slab
    pass; c2r_get_boundaries tells the three kinds of mode apart and c2r_get_boundaries_axes gives back what was set."""
    case = ab.case_e(pkg, heat=False)
    keys = RATES + ("photon_loss",)

    def fresh(boundaries):
        e = case.engine(pkg, tables, boundaries=boundaries)
        out = one_pass(e)
        e.close()
        return out

    ref_p, ref_o, ref_z = fresh(None), fresh(False), fresh((True, True, False))
    assert not np.array_equal(ref_p["phih_grid"], ref_z["phih_grid"]) and not np.array_equal(ref_o["phih_grid"], ref_z["phih_grid"])

    def same(got, ref):
        for k in keys:
            assert np.array_equal(got[k], ref[k]), k
        assert got["sum_nbox"] == ref["sum_nbox"]

    same(fresh((False, False, False)), ref_o)
    same(fresh((True, True, True)), ref_p)
    same(fresh(True), ref_p)
    e = case.engine(pkg, tables, boundaries=None)
    assert e.periodic is True and e.periodic_axes == (True, True, True) and e.lib.c2r_get_boundaries(e.h) == 1
    for boundaries, ref in (((1, 1, 1), ref_p), ((1, 1, 0), ref_z), ((1, 1, 1), ref_p), ((1, 1, 0), ref_z)):
        e.set_boundaries(boundaries)
        assert e.periodic_axes == tuple(bool(b) for b in boundaries)
        assert e.lib.c2r_get_boundaries(e.h) == (1 if all(boundaries) else 2)
        same(one_pass(e), ref)
    assert e.periodic is None
    for axes in [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]:
        e._chk(e.lib.c2r_set_boundaries_axes(e.h, (C.c_int * 3)(*axes)))
        out = (C.c_int * 3)(7, 7, 7)
        assert e.lib.c2r_get_boundaries_axes(e.h, out) == 0 and tuple(out) == axes
        assert e.lib.c2r_get_boundaries(e.h) == (1 if sum(axes) == 3 else (0 if sum(axes) == 0 else 2))
    e.set_boundaries(False)
    assert e.periodic is False and e.periodic_axes == (False, False, False)
    same(one_pass(e), ref_o)
    e.set_boundaries((True, True, False))
    e.set_rates_to_zero()
    e.pass_sources_begin(1, 1, 2)
    with pytest.raises(pkg.C2RayHipError, match="c2r_set_boundaries.*pass"):
        e.set_boundaries((True, False, False))
    with pytest.raises(pkg.C2RayHipError, match="c2r_set_boundaries.*pass"):
        e.set_boundaries(True)
    e.pass_sources_end()
    assert e.periodic_axes == (True, True, False)
    same(e.download_rates(), ref_z)
    e.close()


def test_c_columns_and_source_trace(pkg, orc, otables, tables):
    """C: (11,11,24), x and y open.  Per source: the reach per axis, a block of prod_d(r_d - l_d + 1) entries, which is the
    whole mesh, as many cells traced as the mesh has.  c2r_download_columns: the columns of the source swept last, which
    equal the oracle's coldensh_out / coldenshe_out on the region."""
    case = ab.case_c(pkg)
    ref = case.oracle_pass(pkg, orc, otables)
    e = case.engine(pkg, tables)
    for ns in range(len(case.flux)):            # nothing swept yet: the reach, and zeros
        t = e.source_trace(ns + 1)
        assert t["nbox"] == 0 and t["block_cells"] == 0
        assert (t["reach_l"], t["reach_r"]) == case.reach(ns)
    got = one_pass(e)
    assert_grids_equal(got, ref)
    nbox = 0
    for ns in range(len(case.flux)):
        t = e.source_trace(ns + 1)
        print(ns + 1, case.srcpos[ns], t)
        l, r = case.reach(ns)
        assert l[2] == -12 and r[2] == 11 and l[:2] == [1 - int(p) for p in case.srcpos[ns][:2]]
        assert (t["reach_l"], t["reach_r"]) == (l, r) and (t["box_lo"], t["box_hi"]) == (l, r)
        assert t["block_shells"] >= max(max(-a for a in l), max(r))
        assert t["block_cells"] == int(np.prod([b - a + 1 for a, b in zip(l, r)])) == ab.cells(case.n)
        assert t["swept_cells"] == ab.cells(case.n)
        nbox += t["nbox"]
    assert nbox == got["sum_nbox"] == 8
    cols = e.download_columns()
    e.close()
    for k in ("coldensh_out", "coldenshe_out"):
        assert np.all(ref[k] > 0)
        assert np.array_equal(cols[k], ref[k]), (k, int(np.count_nonzero(cols[k] != ref[k])))
