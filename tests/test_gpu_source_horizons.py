"""Photon horizons (c2r_set_source_horizons) on the GPU against the reference of tests/horizon_reference.py: the oracle's
do_source per source, a NumPy restatement of the predicate of csrc/c2ray_horizon.hpp, the fold in source order
(tests/test_source_horizons_host.py checks both on the CPU).   python -m pytest tests -m gpu.

The bar is tests/test_gpu_source_beams.py's: every grid and every map bit for bit (np.array_equal), sum_nbox and the rounds per
source exactly; a loss that the device sums in another order than its reference to 1e-13 relative, the project's bound for
such a sum.  Meshes are 16^3 (reach 8 < subboxsize 10: one geometric round) and 24^3 (two rounds).
"""
import ctypes as C
import math

import numpy as np
import pytest

import axis_boundary_cases as ab
import beam_reference as br
import horizon_reference as hr
import mix_reference as mr
from conftest import rel_err
from test_gpu_source_beams import CONE_Z45, DT, assert_grids_equal, case16, one_pass, sed_tables

pytestmark = pytest.mark.gpu
INF = float("inf")
THRESHOLD = float(np.float32(1e-10))       # of the source's flux: the sub-box loop's while-test (evolve_source.F90:122-128)


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


# -- periodic 16^3, two sources, one round ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["isothermal", "heating", "three_seds"])
def test_periodic_16_horizon_and_plain_source(pkg, orc, otables, gold, tables, mode):
    """Source 1 with a horizon of 4.5 cells, source 2 with none: phih, phihe, phiheat and sum_nbox against the reference, and
    less is lost than without.  Both sources with radius 1e200 (R2 = +inf) give, through k_rates_beam, the unhorizoned bits and
    the unhorizoned photon_loss(1).  With the horizons taken away again the pass is the oracle's own."""
    t, ot = (tables, otables) if mode != "three_seds" else sed_tables(pkg, orc, gold)
    case = case16(pkg, mode)
    dr = float(case.dr[0])
    horizons = [4.5 * dr, None]
    ref = hr.compose(pkg, orc, ot, case, "gpu16_" + mode, horizons)
    bare = br.compose(pkg, orc, ot, case, "gpu16_" + mode, [None, None])
    within = hr.within_cells(case, 0, horizons[0])
    assert ref["nbox"] == [1, 1] and 0 < within.sum() < within.size // 4
    e = case.engine(pkg, t)
    plain = one_pass(e)
    assert_grids_equal(plain, bare, mode + ", before any horizon")
    e.set_source_horizons(horizons)
    got = one_pass(e)
    assert_grids_equal(got, ref, mode)
    assert got["sum_nbox"] == 2
    assert got["phiheat"].any() == (mode != "isothermal")
    print("photon_loss(1)", got["photon_loss"][0], "unhorizoned", plain["photon_loss"][0])
    assert 0 < got["photon_loss"][0] < plain["photon_loss"][0]
    e.set_source_horizons([1e200, 1e200])
    huge = one_pass(e)
    assert_grids_equal(huge, bare, mode + ", radius 1e200")
    assert huge["sum_nbox"] == 2 and huge["photon_loss"][0] == plain["photon_loss"][0]
    e.set_source_horizons(None)
    off = one_pass(e)
    assert_grids_equal(off, bare, mode + ", horizons off")
    assert off["photon_loss"][0] == plain["photon_loss"][0] and off["sum_nbox"] == 2
    whole = case.oracle_pass(pkg, orc, ot)
    assert_grids_equal(off, whole, mode + ", the oracle's pass")
    e.set_source_horizons([INF, None])                       # inf and None are "no horizon" as well
    same = one_pass(e)
    assert_grids_equal(same, bare, mode + ", inf")
    assert same["photon_loss"][0] == plain["photon_loss"][0]
    e.close()


# -- the horizon ends the sub-box loop ------------------------------------------------------------------------------------------
def test_horizon_ends_the_box_loop(pkg, orc, otables, tables):
    """Periodic 24^3 (two rounds: +-10, then the mesh, as beam_reference.wall_case documents for this geometry), one source at
    (12,12,12) in thin ionised gas.  With radius 6 dr no cell of the first box's surface is lit: one round, photon_loss(1) ==
    0.0, the grids are the masked oracle grids inside the first box.  With radius 11.5 dr the lit part of that surface loses
    far more than the threshold (asserted on the reference's per-cell terms), so the second round runs."""
    case = br.periodic_case(pkg, 24, "ionised", [(12, 12, 12)], [2.0e7])
    key, dr = "hz24", float(case.dr[0])
    assert br.compose(pkg, orc, otables, case, key, [None])["nbox"] == [2]
    e = case.engine(pkg, tables)
    plain = one_pass(e)
    assert plain["sum_nbox"] == 2 and e.source_trace(1)["nbox"] == 2 and plain["photon_loss"][0] > 0
    assert_grids_equal(plain, br.compose(pkg, orc, otables, case, key, [None]), "unhorizoned")
    # radius 6 cells: the sphere lies inside the first box
    ref = hr.compose(pkg, orc, otables, case, key, [6.0 * dr], inside={1: br.first_box(case)})
    e.set_source_horizons([6.0 * dr])
    for again in range(2):          # the second pass starts from what the first learnt about the source
        got = one_pass(e)
        assert got["sum_nbox"] == 1 and e.source_trace(1)["nbox"] == 1
        assert got["photon_loss"][0] == 0.0
        assert_grids_equal(got, ref, f"radius 6, pass {again}")
    assert np.count_nonzero(got["phih_grid"]) == int(hr.within_cells(case, 0, 6.0 * dr).sum())
    # radius 11.5 cells: the sphere cuts the first box's surface
    terms = hr.box_surface_terms(pkg, orc, otables, case, key)
    lit = [term for o, term in terms if bool(hr.within_offsets(11.5 * dr, case.dr, *o))]
    lit_loss, flux = math.fsum(lit), float(case.flux[0]) * case.s_star
    print("surface cells", len(terms), "lit", len(lit), "their loss", lit_loss, "of the flux", lit_loss / flux, "threshold", THRESHOLD)
    assert 0 < len(lit) < len(terms) and lit_loss > THRESHOLD * flux
    ref = hr.compose(pkg, orc, otables, case, key, [11.5 * dr])
    e.set_source_horizons([11.5 * dr])
    got = one_pass(e)
    assert got["sum_nbox"] == 2 and e.source_trace(1)["nbox"] == 2
    assert_grids_equal(got, ref, "radius 11.5")
    outside = ~br.first_box(case)
    assert got["phih_grid"][outside].any() and got["photon_loss"][0] < plain["photon_loss"][0]
    e.close()


# -- cells that are no cubes ----------------------------------------------------------------------------------------------------
def test_cells_that_are_no_cubes(pkg, orc, otables, tables):
    """dr = (d, 1.25 d, 0.75 d): the lit set follows physical lengths, not cell counts."""
    case = br.periodic_case(pkg, 16, "mixed", [(5, 6, 4), (12, 9, 11)], [3.0e7, 8.0e6], cubic=False)
    d = float(case.dr[0])
    horizons = [4.4 * d, 6.1 * d]
    ref = hr.compose(pkg, orc, otables, case, "hz16_box", horizons)
    di, dj, dk = br.offsets(case.n, case.srcpos[0], case.periodic)
    within = hr.within_cells(case, 0, horizons[0]).reshape(di.shape)
    assert within[(di == 0) & (dj == 0) & (dk == 5)].all() and not within[(di == 0) & (dj == 4) & (dk == 0)].any()
    assert not np.array_equal(within, di * di + dj * dj + dk * dk <= 4.4 ** 2)
    e = case.engine(pkg, tables)
    e.set_source_horizons(horizons)
    got = one_pass(e)
    assert_grids_equal(got, ref, "non-cubic")
    assert got["sum_nbox"] == 2
    e.close()


# -- open and mixed boundaries, escape maps ---------------------------------------------------------------------------------------
def open_case(pkg, which):
    if which == "all_open":      # open_boundary_cases.case_one_round's box, mix_reference's "xyz" meshes
        case = mr.make_case(pkg, "xyz", [(3, 6, 5), (9, 2, 11)], [3.0e7, 8.0e6])
        radii = [4.0, None]      # (3,6,5): the sphere reaches x = 1 (2 d away) and z = 1 (4 * 0.75 d), not y (5 * 1.25 d), x = 11, z = 11
        return case, "open_xyz", radii
    case = mr.case_a(pkg)        # (11,11,11), z open, x and y periodic: sources (1,1,1), (11,11,11), (5,11,1), (6,6,6)
    return case, "mix_a", [3.2, None, INF, 4.5]      # (6,6,6): z = 1 and z = 11 are 5 * 0.75 d away


@pytest.mark.parametrize("which", ["all_open", "z_open"])
def test_open_faces_with_escape_maps(pkg, orc, otables, tables, which):
    """Grids and maps against the reference with the horizon in the mask; unlit face cells are exactly 0.0; the six totals
    against the maps; with every axis open the maps' sum is photon_loss(1) to rounding (c2r_get_face_loss's identity)."""
    case, key, radii = open_case(pkg, which)
    d = float(case.dr[0])
    horizons = [r if r is None or r == INF else r * d for r in radii]
    ref = hr.compose(pkg, orc, otables, case, key, horizons)
    maps, per_source = hr.compose_maps(pkg, orc, otables, case, key, horizons)
    bare, _ = br.compose_maps(pkg, orc, otables, case, key, [None] * len(radii))
    e = case.engine(pkg, tables)
    e.enable_face_loss()
    e.set_source_horizons(horizons)
    got = one_pass(e)
    assert_grids_equal(got, ref, which)
    assert got["sum_nbox"] == len(radii)
    for f in maps:
        m = e.face_loss_map(f)
        print(which, "face", f, "non-zero", int(np.count_nonzero(m)), "of", m.size, "differ", int(np.count_nonzero(m != maps[f])))
        assert np.array_equal(m, maps[f]), f
    # the first source alone: the sphere reaches part of an open face, and the face cells beyond it are exactly 0.0
    lit_faces = [f for f in per_source[0] if per_source[0][f].any()]
    assert lit_faces and all(0 < np.count_nonzero(per_source[0][f]) < np.count_nonzero(bare[f]) for f in lit_faces)
    totals, loss = e.face_loss(), got["photon_loss"][0]
    for f in range(6):
        want = math.fsum(maps[f].reshape(-1)) if f in maps else 0.0
        assert rel_err(totals[f], want) <= 1e-13 if want > 0 else totals[f] == 0.0, f
    total = math.fsum(totals)
    print(which, "sum of the maps", total, "photon_loss(1)", loss)
    if which == "all_open":
        assert loss > 0 and rel_err(total, loss) <= 1e-13
    else:                        # the faces of the periodic axes count in photon_loss(1) and in no map
        assert 0 < total <= loss
    e.close()
    e = case.engine(pkg, tables, sources=[0])
    e.enable_face_loss()
    e.set_source_horizons(horizons[:1])
    alone = one_pass(e)
    for f in per_source[0]:
        m = e.face_loss_map(f)
        assert np.array_equal(m, per_source[0][f]), f
        assert m.any() == (f in lit_faces)
    if which == "all_open":
        assert rel_err(math.fsum(e.face_loss()), alone["photon_loss"][0]) <= 1e-13
    e.close()


# -- a beam and a horizon on one source ---------------------------------------------------------------------------------------------
def test_beam_and_horizon_on_one_source(pkg, orc, otables, tables):
    """A 45-degree cone along +z with a radius inside the box: lit iff both; the second source has a horizon only."""
    case = case16(pkg, "isothermal")
    dr = float(case.dr[0])
    beams, horizons = [CONE_Z45, None], [5.5 * dr, 6.0 * dr]
    ref = hr.compose(pkg, orc, otables, case, "gpu16_isothermal", horizons, beams=beams)
    both = br.lit_cells(case, 0, CONE_Z45) & hr.within_cells(case, 0, horizons[0])
    assert 0 < both.sum() < min(br.lit_cells(case, 0, CONE_Z45).sum(), hr.within_cells(case, 0, horizons[0]).sum())
    e = case.engine(pkg, tables)
    e.set_source_horizons(horizons)
    e.set_source_beams(beams)                                  # (the beams keep the horizons)
    got = one_pass(e)
    assert_grids_equal(got, ref, "cone and horizon")
    assert got["sum_nbox"] == 2
    e.set_source_beams(None)
    assert_grids_equal(one_pass(e), hr.compose(pkg, orc, otables, case, "gpu16_isothermal", horizons), "horizon alone")
    e.set_source_horizons(None)
    e.set_source_beams(beams)
    assert_grids_equal(one_pass(e), br.compose(pkg, orc, otables, case, "gpu16_isothermal", beams), "cone alone")
    e.close()


# -- every route ----------------------------------------------------------------------------------------------------------------
def test_every_route_honours_the_horizon(pkg, orc, otables, tables):
    """c2r_do_source source by source, the slab-wise pass, c2r_pass_allreduce_chemistry, c2r_iteration, and c2r_evolve3d against
    an evolve driven by its pieces, on the 16^3 case."""
    case = case16(pkg, "isothermal")
    dr = float(case.dr[0])
    horizons = [4.5 * dr, None]
    ref = hr.compose(pkg, orc, otables, case, "gpu16_isothermal", horizons)
    e = case.engine(pkg, tables)
    e.set_source_horizons(horizons)
    whole = one_pass(e)
    assert_grids_equal(whole, ref, "pass")
    conv = e.global_pass(DT)
    state = e.download_iter_state()
    e.begin_step()
    e.set_rates_to_zero()
    e.do_source(1)
    e.do_source(2)
    assert_grids_equal(e.download_rates(), ref, "do_source")
    e.begin_step()
    e.set_rates_to_zero()
    for s in range(e.pass_sources_begin(1, 1, 3)):
        e.pass_wait_slab(s)
    e.pass_sources_end()
    slabs = e.download_rates()
    assert_grids_equal(slabs, ref, "slab-wise")
    assert slabs["photon_loss"][0] == whole["photon_loss"][0]
    e.begin_step()
    e.set_rates_to_zero()
    assert e.pass_allreduce_chemistry(DT, 1, 1, 2) == conv
    fused = e.download_iter_state()
    for k in state:
        assert np.array_equal(fused[k], state[k]), ("pass_allreduce_chemistry", k)
    assert_grids_equal(e.download_rates(), ref, "pass_allreduce_chemistry")
    e.begin_step()
    e.set_rates_to_zero()
    rep = e.iteration(DT, 1, 1, 2)
    assert rep["conv_flag"] == conv and rep["sum_nbox"] == 2 and rep["photon_loss"][0] == whole["photon_loss"][0]
    it = e.download_iter_state()
    for k in state:
        assert np.array_equal(it[k], state[k]), ("iteration", k)
    e.close()

    def final_state(e_):
        mat = pkg.Material(case.region[0], None, None, None, True, 1.0e4, 1.0, case.reccoef)
        e_.download_state(mat)
        e_.close()
        return mat.xh

    def evolve(horizons_):
        e_ = case.engine(pkg, tables)
        if horizons_ is not None:
            e_.set_source_horizons(horizons_)
        niter, flags = e_.evolve3d(DT)
        return niter, flags, final_state(e_)

    def evolve_by_pieces(horizons_):        # evolve.F90:78-229 with the context's own calls
        e_ = case.engine(pkg, tables)
        e_.set_source_horizons(horizons_)
        criterion = min(int(pkg.evolve.convergence_fraction * ab.cells(case.n)), len(case.flux))
        e_.begin_step()
        niter, flags = 0, [ab.cells(case.n)]
        while not (flags[-1] < criterion and niter > 1) and niter <= 500:
            niter += 1
            e_.set_rates_to_zero()
            e_.pass_sources(1, 1)
            flags.append(e_.global_pass(DT))
        e_.end_step()
        return niter, flags[1:], final_state(e_)

    _, _, plain = evolve(None)
    _, _, huge = evolve([1e200, 1e200])
    niter, flags, cut = evolve(horizons)
    pieces = evolve_by_pieces(horizons)
    print("evolve3d: iterations", niter, "flags", flags, "by pieces", pieces[0], pieces[1])
    assert np.array_equal(plain, huge) and not np.array_equal(plain, cut)
    assert (niter, flags) == pieces[:2] and np.array_equal(cut, pieces[2])


def test_evolve0d_cell_by_cell_is_do_source(pkg, tables):
    """One source with a horizon at 8^3, periodic, cells that are no cubes: c2r_evolve0d over the cells of its reach in shell
    order gives the bits of c2r_do_source; the loss of an unlit surface cell is 0.0, and the losses add up to photon_loss(1)."""
    case = br.periodic_case(pkg, 8, "ionised", [(3, 6, 2)], [2.0e7], cubic=False)
    radius = 3.6 * float(case.dr[0])
    e = case.engine(pkg, tables)
    e.set_source_horizons([radius])
    e.begin_step()
    e.set_rates_to_zero()
    e.do_source(1)
    ref = e.download_rates()
    assert ref["sum_nbox"] == 1
    e.begin_step()
    e.set_rates_to_zero()
    offs = [(i, j, k) for k in range(-4, 4) for j in range(-4, 4) for i in range(-4, 4)]
    offs.sort(key=lambda o: max(abs(o[0]), abs(o[1]), abs(o[2])))
    lit_terms, dark_terms = [], []
    for o in offs:
        surface = any(x in (-4, 3) for x in o)
        pos = (C.c_int * 3)(*(int(p) + x for p, x in zip(case.srcpos[0], o)))
        loss = C.c_double(-1.0)
        e._chk(e.lib.c2r_evolve0d(e.h, pos, 1, 1, int(surface), C.byref(loss)))
        if surface:
            (lit_terms if bool(hr.within_offsets(radius, case.dr, *o)) else dark_terms).append(loss.value)
    got = e.download_rates()
    assert_grids_equal(got, ref, "evolve0d")
    assert np.count_nonzero(got["phih_grid"]) == int(hr.within_cells(case, 0, radius).sum())
    print("surface cells lit", len(lit_terms), "dark", len(dark_terms))
    assert len(dark_terms) > len(lit_terms) > 10
    assert all(x == 0.0 for x in dark_terms) and all(x > 0.0 for x in lit_terms)
    expected = float(np.sum(np.sort(np.array(lit_terms))))
    print("photon_loss(1)", ref["photon_loss"][0], "sum of the per-cell losses", expected, "rel", rel_err(ref["photon_loss"][0], expected))
    assert rel_err(ref["photon_loss"][0], expected) <= 1e-13
    e.close()


def test_two_replicas_on_one_device(pkg, orc, otables, tables):
    """c2r_create_multi([0, 0]): device 0 sweeps source 1, device 1 source 2; the horizons reach both."""
    case = case16(pkg, "isothermal")
    dr = float(case.dr[0])
    horizons = [4.5 * dr, 6.0 * dr]
    ref = hr.compose(pkg, orc, otables, case, "gpu16_isothermal", horizons)      # (0 + a) + (0 + b): the sum of the two devices' grids
    hp = pkg.hostphys
    ndens, xh, xhe, _ = case.region
    mat = pkg.Material(ndens, xh.copy(), xhe.copy(), None, True, 1.0e4, 1.0, case.reccoef)
    e = pkg.HipEngine(case.n, [0, 0])
    e.set_tables(tables)
    e.set_step(mat, pkg.GridProps(case.n, case.dr, case.vol), pkg.Cosmology(ab.ZRED, hp.H0, hp.Omega0))
    e.set_sources(pkg.SourceProps(case.srcpos, case.flux, case.s_star))
    e.upload_state(mat)
    e.comm_init_local()
    assert e.num_devices() == 2
    e.set_source_horizons(horizons)
    assert e.get_source_horizon(2) == horizons[1]
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    e.allreduce_rates()
    got = e.download_rates()
    assert_grids_equal(got, ref, "two replicas")
    assert got["sum_nbox"] == 2
    e.close()


# -- a physical length ------------------------------------------------------------------------------------------------------------
def test_radius_is_a_physical_length(pkg, orc, otables, tables):
    """After c2r_set_step_scalars with dr doubled the same radius lights the cells with half the offset: the grids equal the
    reference composed with the new dr (the oracle run with it)."""
    case = case16(pkg, "isothermal")
    dr = float(case.dr[0])
    horizons = [6.0 * dr, None]
    wide = case16(pkg, "isothermal")
    wide.dr = tuple(2.0 * float(x) for x in case.dr)
    wide.vol = wide.dr[0] * wide.dr[1] * wide.dr[2]
    di, dj, dk = br.offsets(case.n, case.srcpos[0], case.periodic)
    assert np.array_equal(hr.within_cells(wide, 0, horizons[0]), hr.within_offsets(3.0 * dr, case.dr, di, dj, dk).reshape(-1))
    e = case.engine(pkg, tables)
    e.set_source_horizons(horizons)
    assert_grids_equal(one_pass(e), hr.compose(pkg, orc, otables, case, "gpu16_isothermal", horizons), "dr")
    hp = pkg.hostphys
    mat = pkg.Material(case.region[0], None, None, None, True, 1.0e4, 1.0, case.reccoef)
    e.set_step_scalars(mat, pkg.GridProps(case.n, wide.dr, wide.vol), pkg.Cosmology(ab.ZRED, hp.H0, hp.Omega0))
    assert e.get_source_horizon(1) == horizons[0]
    got = one_pass(e)
    ref = hr.compose(pkg, orc, otables, wide, "gpu16_isothermal_2dr", horizons)
    assert_grids_equal(got, ref, "2 dr")
    assert np.count_nonzero(hr.within_cells(wide, 0, horizons[0])) < np.count_nonzero(hr.within_cells(case, 0, horizons[0]))
    e.close()


# -- lifetime and refusals --------------------------------------------------------------------------------------------------------
def test_lifetime_and_refusals(pkg, tables):
    case = case16(pkg, "isothermal")
    e = case.engine(pkg, tables)
    assert e.get_source_horizon(1) == INF and e.get_source_horizon(2) == INF
    e.set_source_horizons([2.5e24, None])
    assert e.get_source_horizon(1) == 2.5e24 and e.get_source_horizon(2) == INF
    for ns in (0, 3, -1):
        with pytest.raises(pkg.C2RayHipError, match="c2r_get_source_horizon"):
            e.get_source_horizon(ns)
    e.set_boundaries((True, True, False))                       # the boundaries keep the horizons
    assert e.get_source_horizon(1) == 2.5e24
    e.set_boundaries(True)
    e.set_source_beams([CONE_Z45, None])                        # and so do the beams
    assert e.get_source_horizon(1) == 2.5e24
    e.set_source_beams(None)
    nan = float("nan")
    bad = [[nan, None], [None, nan], [-1.0, None], [1.0e24, -1.0e-300], [-INF, 1.0],
           [1.0e24], [1.0e24, None, None]]                      # the last two: nsrc != NumSrc
    for radii in bad:
        with pytest.raises(pkg.C2RayHipError, match="c2r_set_source_horizons"):
            e.set_source_horizons(radii)
        assert e.get_source_horizon(1) == 2.5e24 and e.get_source_horizon(2) == INF, radii      # a refused call changes nothing
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources_begin(1, 1, 2)
    with pytest.raises(pkg.C2RayHipError, match="still open"):
        e.set_source_horizons(None)
    with pytest.raises(pkg.C2RayHipError, match="still open"):
        e.set_source_horizons([1.0, 1.0])
    e.pass_sources_end()
    assert e.get_source_horizon(1) == 2.5e24
    e.set_source_horizons([0.0, 1e200])                         # the ends are allowed
    assert e.get_source_horizon(1) == 0.0 and e.get_source_horizon(2) == 1e200
    e.set_sources(pkg.SourceProps(case.srcpos, case.flux, case.s_star))    # c2r_set_sources clears the horizons
    assert e.get_source_horizon(1) == INF and e.get_source_horizon(2) == INF
    e.set_source_horizons([None, 3.0e24])
    e.set_source_horizons(None)
    assert e.get_source_horizon(2) == INF
    e.close()
