"""Source light curves (c2r_set_source_curves) on the GPU against the reference of tests/curve_reference.py: per source and per
shell the oracle's do_source with the source's fluxes times the shell's factor, a NumPy restatement of the rule of
csrc/c2ray_curve.hpp, the fold in source order (tests/test_source_curves_host.py checks both on the CPU).
python -m pytest tests -m gpu.   C2R_CURVE_FUZZ_CASES / C2R_CURVE_FUZZ_SEED widen or move the seeded list at the end.

The bar is tests/test_gpu_source_horizons.py's: every grid and every map bit for bit (np.array_equal), sum_nbox and the rounds
per source exactly; a loss that the device sums in another order than its reference to 1e-13 relative, the project's bound for
such a sum.  Meshes are 16^3 (reach 8 < subboxsize 10: one geometric round in every run, oracle and product), 24^3 (two rounds,
decided as asserted from the reference's per-cell terms) and the small open and mixed cases of the horizon tests (one round).
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import axis_boundary_cases as ab
import beam_reference as br
import curve_reference as cr
import horizon_reference as hr
import rim_reference as rr
from conftest import rel_err
from test_gpu_source_beams import CONE_Z45, DT, assert_grids_equal, case16, one_pass, sed_tables
from test_gpu_source_horizons import THRESHOLD, open_case

pytestmark = pytest.mark.gpu
INF = float("inf")
FACTORS = (0.0, 0.25, 0.5, 1.0, 2.0, 3.0 / 7.0, 1.9)


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


def rounds(e, nsrc):
    return [e.source_trace(ns)["nbox"] for ns in range(1, nsrc + 1)]


def one_round_everywhere(ref):
    return all(nb == 1 for per in ref["nbox"] for nb in per)


# -- 1. periodic 16^3, two sources, one round -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["isothermal", "heating", "three_seds"])
def test_periodic_16_curve_and_plain_source(pkg, orc, otables, gold, tables, mode):
    """Source 1 with radii (3.5, 6.5) dr and factors (1.0, 0.3, 2.5), source 2 with no curve: phih, phihe, phiheat and the rounds
    against the reference.  Then all factors 1.0 (the bare bits through k_rates_curve), the curves removed, and the oracle's
    own pass.  A single source with nstep = 0 and factor 0.5 gives exactly 0.5 x its grids and its loss."""
    t, ot = (tables, otables) if mode != "three_seds" else sed_tables(pkg, orc, gold)
    case = case16(pkg, mode)
    dr = float(case.dr[0])
    curves = [([3.5 * dr, 6.5 * dr], [1.0, 0.3, 2.5]), None]
    ref = cr.compose(pkg, orc, ot, case, "gpu16_" + mode, curves)
    bare = br.compose(pkg, orc, ot, case, "gpu16_" + mode, [None, None])
    shell = cr.shell_cells(case, 0, curves[0])
    assert ref["runs"] == [[1.0, 0.3, 2.5], [1.0]] and one_round_everywhere(ref) and all((shell == b).sum() > 50 for b in range(3))
    e = case.engine(pkg, t)
    plain = one_pass(e)
    assert_grids_equal(plain, bare, mode + ", before any curve")
    e.set_source_curves(curves)
    got = one_pass(e)
    assert_grids_equal(got, ref, mode)
    assert got["sum_nbox"] == 2 and rounds(e, 2) == [1, 1]
    assert got["phiheat"].any() == (mode != "isothermal")
    assert not np.array_equal(got["phih_grid"], plain["phih_grid"])
    print("photon_loss(1)", got["photon_loss"][0], "uncurved", plain["photon_loss"][0])
    assert got["photon_loss"][0] > plain["photon_loss"][0] > 0            # the surface of source 1's box lies in the shell of 2.5
    e.set_source_curves([([3.5 * dr, 6.5 * dr], [1.0, 1.0, 1.0]), ([2.0 * dr], [1.0, 1.0])])
    ones = one_pass(e)
    assert_grids_equal(ones, bare, mode + ", all factors 1.0")
    assert ones["sum_nbox"] == 2 and ones["photon_loss"][0] == plain["photon_loss"][0]
    e.set_source_curves([([3.5 * dr, 6.5 * dr], [1.0, 1.0, 1.0]), None])    # a curved and an uncurved source in k_rates_curve
    mixed = one_pass(e)
    assert_grids_equal(mixed, bare, mode + ", factors 1.0 beside an uncurved source")
    assert mixed["photon_loss"][0] == plain["photon_loss"][0]
    e.set_source_curves(None)
    off = one_pass(e)
    assert_grids_equal(off, bare, mode + ", curves off")
    assert off["photon_loss"][0] == plain["photon_loss"][0] and off["sum_nbox"] == 2
    whole = case.oracle_pass(pkg, orc, ot)
    assert_grids_equal(off, whole, mode + ", the oracle's pass")
    e.close()
    e = case.engine(pkg, t, sources=[0])
    base = one_pass(e)
    e.set_source_curves([([], [0.5])])
    half = one_pass(e)
    for k in cr.GRIDS:
        assert np.array_equal(half[k], 0.5 * base[k]), (mode, k)
    assert half["photon_loss"][0] == 0.5 * base["photon_loss"][0] and base["photon_loss"][0] > 0 and half["sum_nbox"] == 1
    e.close()


# -- 2. a step to zero is a horizon -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [6.0, 11.5])
def test_step_to_zero_is_a_horizon(pkg, orc, otables, tables, cells):
    """Periodic 24^3, one source (tests/test_gpu_source_horizons.py's case): {1, {R}, {1, 0}} against c2r_set_source_horizons(R).
    R = 6 dr: one round and photon_loss(1) == 0.0; R = 11.5 dr: two rounds.  Grids, photon_loss, sum_nbox and the rounds bit
    for bit between the two product runs and against horizon_reference.compose."""
    case = br.periodic_case(pkg, 24, "ionised", [(12, 12, 12)], [2.0e7])
    key, R = "hz24", cells * float(case.dr[0])
    inside = {1: br.first_box(case)} if cells == 6.0 else None
    ref = hr.compose(pkg, orc, otables, case, key, [R], inside=inside)
    runs = {}
    for how in ("curve", "horizon"):
        e = case.engine(pkg, tables)
        if how == "curve":
            e.set_source_curves([([R], [1.0, 0.0])])
        else:
            e.set_source_horizons([R])
        for again in range(2):          # the second pass starts from what the first learnt about the source
            got = one_pass(e)
            assert_grids_equal(got, ref, f"{how}, R = {cells} dr, pass {again}")
            assert got["sum_nbox"] == rounds(e, 1)[0] == (1 if cells == 6.0 else 2)
        runs[how] = got
        e.close()
    for k in cr.GRIDS:
        assert np.array_equal(runs["curve"][k], runs["horizon"][k]), k
    assert np.array_equal(runs["curve"]["photon_loss"], runs["horizon"]["photon_loss"])
    print("R", cells, "photon_loss(1)", runs["curve"]["photon_loss"][0])
    assert (runs["curve"]["photon_loss"][0] == 0.0) == (cells == 6.0)


# -- 3. the deciding loss sees the factor -------------------------------------------------------------------------------------------
def test_the_deciding_loss_sees_the_factor(pkg, orc, otables, tables):
    """Periodic 24^3, thin ionised gas.  The surface of the first box loses far more than THRESHOLD * flux, and the same terms
    times 2^-40 do not (asserted on the reference's per-cell terms).  A curve with factor 2^-40 beyond 8.5 dr -- every cell of
    that surface -- therefore ends the loop after one round: the kept loss is the fsum of the scaled terms, the grids are the
    reference's inside the first box.  Without the curve there are two rounds."""
    case = br.periodic_case(pkg, 24, "ionised", [(12, 12, 12)], [2.0e7])
    key, dr, tiny = "hz24", float(case.dr[0]), 2.0 ** -40
    terms = hr.box_surface_terms(pkg, orc, otables, case, key)
    flux = float(case.flux[0]) * case.s_star
    plain_loss, scaled = math.fsum(t for _, t in terms), [tiny * t for _, t in terms]
    print("surface cells", len(terms), "their loss / flux", plain_loss / flux, "scaled", math.fsum(scaled) / flux, "threshold", THRESHOLD)
    assert plain_loss > THRESHOLD * flux and not math.fsum(scaled) > THRESHOLD * flux and math.fsum(scaled) > 0
    curve = ([8.5 * dr], [1.0, tiny])
    assert all(int(cr.shell_offsets(curve, case.dr, *o)) == 1 for o, _ in terms)
    ref = cr.compose(pkg, orc, otables, case, key, [curve], inside={1: br.first_box(case)})
    e = case.engine(pkg, tables)
    plain = one_pass(e)
    assert plain["sum_nbox"] == 2 and rounds(e, 1) == [2]
    e.set_source_curves([curve])
    for again in range(2):
        got = one_pass(e)
        assert got["sum_nbox"] == 1 and rounds(e, 1) == [1]
        assert_grids_equal(got, ref, f"factor 2^-40, pass {again}")
        print("kept loss", got["photon_loss"][0], "fsum of the scaled terms", math.fsum(scaled), "rel", rel_err(got["photon_loss"][0], math.fsum(scaled)))
        assert rel_err(got["photon_loss"][0], math.fsum(scaled)) <= 1e-13
    assert not got["phih_grid"][~br.first_box(case)].any()
    e.set_source_curves(None)
    assert one_pass(e)["sum_nbox"] == 2
    e.close()


# -- 4. cells that are no cubes -----------------------------------------------------------------------------------------------------
def test_cells_that_are_no_cubes(pkg, orc, otables, tables):
    """dr = (d, 1.25 d, 0.75 d), two curved sources: the shells follow physical lengths, not cell counts."""
    case = br.periodic_case(pkg, 16, "mixed", [(5, 6, 4), (12, 9, 11)], [3.0e7, 8.0e6], cubic=False)
    d = float(case.dr[0])
    curves = [([3.3 * d, 6.1 * d], [2.0, 1.0, 0.25]), ([4.4 * d], [0.5, 3.0 / 7.0])]
    ref = cr.compose(pkg, orc, otables, case, "hz16_box", curves)
    assert one_round_everywhere(ref)
    di, dj, dk = br.offsets(case.n, case.srcpos[0], case.periodic)
    shell = cr.shell_cells(case, 0, curves[0]).reshape(di.shape)
    r2 = di * di + dj * dj + dk * dk
    assert not np.array_equal(shell, (r2 > 3.3 ** 2).astype(np.int64) + (r2 > 6.1 ** 2))
    assert (shell[(di == 0) & (dj == 0) & (dk == 4)] == 0).all() and (shell[(di == 0) & (dj == 3) & (dk == 0)] == 1).all()     # 3 d, 3.75 d
    e = case.engine(pkg, tables)
    e.set_source_curves(curves)
    got = one_pass(e)
    assert_grids_equal(got, ref, "non-cubic")
    assert got["sum_nbox"] == 2
    e.close()


# -- 5. open and mixed boundaries, escape maps ---------------------------------------------------------------------------------------
def open_curves(which, d):
    if which == "all_open":      # sources (3,6,5) and (9,2,11) of an 11^3-like open box
        return [([2.5 * d, 5.0 * d], [1.0, 0.3, 0.0]), ([6.0 * d], [2.0, 1.0])]
    return [([3.2 * d], [1.0, 0.25]), None, ([2.0 * d, 4.0 * d], [1.9, 0.0, 0.5]), ([4.5 * d], [1.0, 3.0 / 7.0])]


@pytest.mark.parametrize("which", ["all_open", "z_open"])
def test_open_faces_with_escape_maps(pkg, orc, otables, tables, which):
    """Grids, the map of every open face and c2r_get_face_loss against the reference; face cells in a shell of factor 0 are
    exactly 0.0; with every axis open the maps' sum is photon_loss(1) to rounding."""
    case, key, _ = open_case(pkg, which)
    curves = open_curves(which, float(case.dr[0]))
    ref = cr.compose(pkg, orc, otables, case, key, curves)
    maps, per_source = cr.compose_maps(pkg, orc, otables, case, key, curves)
    bare, bare_per = br.compose_maps(pkg, orc, otables, case, key, [None] * len(curves))
    assert one_round_everywhere(ref)
    e = case.engine(pkg, tables)
    e.enable_face_loss()
    e.set_source_curves(curves)
    got = one_pass(e)
    assert_grids_equal(got, ref, which)
    assert got["sum_nbox"] == len(curves) and rounds(e, len(curves)) == [1] * len(curves)
    for f in maps:
        m = e.face_loss_map(f)
        print(which, "face", f, "non-zero", int(np.count_nonzero(m)), "of", m.size, "differ", int(np.count_nonzero(m != maps[f])))
        assert np.array_equal(m, maps[f]), f
    assert any(not np.array_equal(maps[f], bare[f]) for f in maps)
    dark = 0 if which == "all_open" else 2           # the source with a shell of factor 0: some of its face cells are dark
    assert any(np.count_nonzero(per_source[dark][f]) < np.count_nonzero(bare_per[dark][f]) for f in maps)
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


# -- 6. beam, horizon and curve on one source, with the horizon loss ------------------------------------------------------------------
def test_beam_horizon_and_curve_with_the_horizon_loss(pkg, orc, otables, tables):
    """Source 1: a 45-degree cone, a horizon of 5.5 dr and a curve whose last radius (5.1 dr) cuts through the rim -- rim cells
    beyond it lie in a shell of factor 0 and have no face, the others form their po with 0.3 x the flux.  Source 2: a horizon
    and a curve.  Grids, c2r_download_horizon_rim and c2r_get_horizon_loss against the reference."""
    case = case16(pkg, "isothermal")
    key, dr = "gpu16_isothermal", float(case.dr[0])
    beams, horizons = [CONE_Z45, None], [5.5 * dr, 6.0 * dr]
    curves = [([3.0 * dr, 5.1 * dr], [1.0, 0.3, 0.0]), ([5.2 * dr], [2.0, 0.5])]
    ref = cr.compose(pkg, orc, otables, case, key, curves, horizons=horizons, beams=beams)
    assert one_round_everywhere(ref)
    lit = cr.lit_cells(case, 0, curves[0], horizons[0], CONE_Z45)
    assert 0 < lit.sum() < (br.lit_cells(case, 0, CONE_Z45) & hr.within_cells(case, 0, horizons[0])).sum()
    e = case.engine(pkg, tables)
    e.enable_horizon_loss()
    e.set_source_horizons(horizons)
    e.set_source_beams(beams)
    e.set_source_curves(curves)                                # (beams and horizons are kept)
    got = one_pass(e)
    assert_grids_equal(got, ref, "cone, horizon and curve")
    assert got["sum_nbox"] == 2
    want = []
    for ns in (1, 2):
        tr = e.source_trace(ns)
        lo, hi = rr.final_box(case, ns - 1, tr["nbox"])
        assert lo == tr["box_lo"] and hi == tr["box_hi"]
        terms, face = cr.rim_terms(pkg, orc, otables, case, key, ns - 1, curves[ns - 1], horizons[ns - 1], lo, hi, beams[ns - 1])
        plain_face = rr.columns(horizons[ns - 1], case.dr, lo, hi, beams[ns - 1])["face"]
        print("source", ns, "faces", int(face.sum()), "without the curve", int(plain_face.sum()))
        assert 10 < face.sum() and np.all(terms[face] > 0)
        if ns == 1:
            assert face.sum() < plain_face.sum()              # the rim cells beyond 5.1 dr have no face
        want.append(terms)
    got_ns, got_ext, rim = e.horizon_rim()
    assert got_ns == 2 and np.array_equal(rim, want[1])
    per, total = e.horizon_loss()
    print("horizon loss", per, "expected", [rr.face_sum(w) for w in want])
    assert per[0] == rr.face_sum(want[0]) and per[1] == rr.face_sum(want[1]) and total == per[0] + per[1]
    e.close()
    e = case.engine(pkg, tables, sources=[0])                  # source 1 alone: its rim terms, cell by cell
    e.enable_horizon_loss()
    e.set_source_horizons(horizons[:1])
    e.set_source_beams(beams[:1])
    e.set_source_curves(curves[:1])
    one_pass(e)
    got_ns, _, rim = e.horizon_rim()
    assert got_ns == 1 and np.array_equal(rim, want[0])
    e.set_source_beams(None)                                   # the features come off one by one
    e.set_source_horizons(None)
    assert_grids_equal(one_pass(e), cr.compose(pkg, orc, otables, case, key, curves, sources=[1]), "curve alone")
    e.close()


# -- 7. routes and bookkeeping ---------------------------------------------------------------------------------------------------------
def test_every_route_honours_the_curve(pkg, orc, otables, tables):
    """c2r_do_source source by source, the slab-wise pass, c2r_pass_allreduce_chemistry, c2r_iteration, and c2r_evolve3d against
    an evolve driven by its pieces, on the 16^3 case."""
    case = case16(pkg, "isothermal")
    dr = float(case.dr[0])
    curves = [([3.5 * dr, 6.5 * dr], [1.0, 0.3, 2.5]), None]
    ref = cr.compose(pkg, orc, otables, case, "gpu16_isothermal", curves)
    e = case.engine(pkg, tables)
    e.set_source_curves(curves)
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

    def evolve(curves_):
        e_ = case.engine(pkg, tables)
        if curves_ is not None:
            e_.set_source_curves(curves_)
        niter, flags = e_.evolve3d(DT)
        return niter, flags, final_state(e_)

    def evolve_by_pieces(curves_):        # evolve.F90:78-229 with the context's own calls
        e_ = case.engine(pkg, tables)
        e_.set_source_curves(curves_)
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
    _, _, ones = evolve([([3.5 * dr], [1.0, 1.0]), None])
    niter, flags, curved = evolve(curves)
    pieces = evolve_by_pieces(curves)
    print("evolve3d: iterations", niter, "flags", flags, "by pieces", pieces[0], pieces[1])
    assert np.array_equal(plain, ones) and not np.array_equal(plain, curved)
    assert (niter, flags) == pieces[:2] and np.array_equal(curved, pieces[2])


def test_evolve0d_cell_by_cell_is_do_source(pkg, tables):
    """One curved source at 8^3, periodic, cells that are no cubes: c2r_evolve0d over the cells of its reach in shell order gives
    the bits of c2r_do_source; the loss of a surface cell in the shell of factor 0 is 0.0, and the losses add up to
    photon_loss(1)."""
    case = br.periodic_case(pkg, 8, "ionised", [(3, 6, 2)], [2.0e7], cubic=False)
    d = float(case.dr[0])
    curve = ([2.0 * d, 3.6 * d], [0.5, 0.0, 3.0 / 7.0])
    e = case.engine(pkg, tables)
    e.set_source_curves([curve])
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
            (lit_terms if float(cr.factor_offsets(curve, case.dr, *o)) != 0.0 else dark_terms).append(loss.value)
    got = e.download_rates()
    assert_grids_equal(got, ref, "evolve0d")
    assert np.count_nonzero(got["phih_grid"]) == int((cr.factor_cells(case, 0, curve) != 0.0).sum())
    print("surface cells lit", len(lit_terms), "dark", len(dark_terms))
    assert len(dark_terms) > 10 and len(lit_terms) > 10
    assert all(x == 0.0 for x in dark_terms) and all(x > 0.0 for x in lit_terms)
    expected = float(np.sum(np.sort(np.array(lit_terms))))
    print("photon_loss(1)", ref["photon_loss"][0], "sum of the per-cell losses", expected, "rel", rel_err(ref["photon_loss"][0], expected))
    assert rel_err(ref["photon_loss"][0], expected) <= 1e-13
    e.close()


def test_two_replicas_on_one_device(pkg, orc, otables, tables):
    """c2r_create_multi([0, 0]): device 0 sweeps source 1, device 1 source 2; the curves reach both."""
    case = case16(pkg, "isothermal")
    dr = float(case.dr[0])
    curves = [([3.5 * dr, 6.5 * dr], [1.0, 0.3, 2.5]), ([4.5 * dr], [0.25, 1.9])]
    ref = cr.compose(pkg, orc, otables, case, "gpu16_isothermal", curves)      # (0 + a) + (0 + b): the sum of the two devices' grids
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
    e.set_source_curves(curves)
    assert e.source_curve(2) == ([4.5 * dr], [0.25, 1.9])
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    e.allreduce_rates()
    got = e.download_rates()
    assert_grids_equal(got, ref, "two replicas")
    assert got["sum_nbox"] == 2
    e.close()


def test_radius_is_a_physical_length(pkg, orc, otables, tables):
    """After c2r_set_step_scalars with dr doubled the same radii hold the cells with half the offset: the grids equal the
    reference composed with the new dr (the oracle run with it)."""
    case = case16(pkg, "isothermal")
    dr = float(case.dr[0])
    curves = [([3.0 * dr, 6.0 * dr], [1.0, 0.3, 2.0]), None]
    wide = case16(pkg, "isothermal")
    wide.dr = tuple(2.0 * float(x) for x in case.dr)
    wide.vol = wide.dr[0] * wide.dr[1] * wide.dr[2]
    half = ([1.5 * dr, 3.0 * dr], curves[0][1])
    assert np.array_equal(cr.shell_cells(wide, 0, curves[0]), cr.shell_cells(case, 0, half))
    e = case.engine(pkg, tables)
    e.set_source_curves(curves)
    assert_grids_equal(one_pass(e), cr.compose(pkg, orc, otables, case, "gpu16_isothermal", curves), "dr")
    hp = pkg.hostphys
    mat = pkg.Material(case.region[0], None, None, None, True, 1.0e4, 1.0, case.reccoef)
    e.set_step_scalars(mat, pkg.GridProps(case.n, wide.dr, wide.vol), pkg.Cosmology(ab.ZRED, hp.H0, hp.Omega0))
    assert e.source_curve(1) == curves[0]
    got = one_pass(e)
    ref = cr.compose(pkg, orc, otables, wide, "gpu16_isothermal_2dr", curves)
    assert one_round_everywhere(ref)
    assert_grids_equal(got, ref, "2 dr")
    e.close()


def raw_set(e, pkg, records):
    """c2r_set_source_curves with records (nstep, radii, factors) as they are, past the checks of the Python layer."""
    arr = (pkg._lib.SourceCurve * len(records))()
    for rec, (nstep, radii, factors) in zip(arr, records):
        rec.nstep = nstep
        for k, r in enumerate(radii):
            rec.radius[k] = r
        for k, f in enumerate(factors):
            rec.factor[k] = f
    e._chk(e.lib.c2r_set_source_curves(e.h, len(records), arr))


def test_lifetime_getter_and_refusals(pkg, orc, otables, tables):
    case = case16(pkg, "isothermal")
    e = case.engine(pkg, tables)
    none = ([], [1.0])
    assert e.source_curve(1) == none and e.source_curve(2) == none
    mine = ([2.5e24, 7.5e24], [1.0, 0.3, 2.5])
    e.set_source_curves([mine, None])
    assert e.source_curve(1) == mine and e.source_curve(2) == none
    c = pkg._lib.SourceCurve()
    e._chk(e.lib.c2r_get_source_curve(e.h, 1, C.byref(c)))
    assert c.nstep == 2 and list(c.radius) == [2.5e24, 7.5e24] + [0.0] * 6 and list(c.factor) == [1.0, 0.3, 2.5] + [0.0] * 6
    e._chk(e.lib.c2r_get_source_curve(e.h, 2, C.byref(c)))
    assert c.nstep == 0 and list(c.radius) == [0.0] * 8 and list(c.factor) == [1.0] + [0.0] * 8
    for ns in (0, 3, -1):
        with pytest.raises(pkg.C2RayHipError, match="c2r_get_source_curve"):
            e.source_curve(ns)
    e.set_boundaries((True, True, False))                       # the boundaries keep the curves
    assert e.source_curve(1) == mine
    e.set_boundaries(True)
    e.set_source_beams([CONE_Z45, None])                        # and so do the beams and the horizons
    e.set_source_horizons([1.0e25, None])
    assert e.source_curve(1) == mine
    e.set_source_beams(None)
    e.set_source_horizons(None)
    assert e.source_curve(1) == mine
    nan = float("nan")
    ok = (1, [1.0e24], [1.0, 0.5])
    bad = [([(1, [nan], [1.0, 1.0]), ok], "negative or not finite"), ([ok, (1, [-1.0], [1.0, 1.0])], "negative or not finite"),
           ([(1, [INF], [1.0, 1.0]), ok], "negative or not finite"), ([(2, [2.0e24, 2.0e24], [1.0, 1.0, 1.0]), ok], "is not above"),
           ([(3, [1.0e24, 3.0e24, 2.0e24], [1.0] * 4), ok], "is not above"), ([ok, (1, [1.0e24], [1.0, -0.5])], "factor"),
           ([(0, [], [nan]), ok], "factor"), ([(1, [1.0e24], [INF, 1.0]), ok], "factor"), ([(9, [], [1.0]), ok], "nstep = 9"),
           ([ok, (-1, [], [1.0])], "nstep = -1"), ([(0, [], [0.0]), ok], "zeroed record"),
           ([ok], "nsrc = 1"), ([ok, ok, ok], "nsrc = 3")]
    for records, text in bad:
        with pytest.raises(pkg.C2RayHipError, match="c2r_set_source_curves.*" + text):
            raw_set(e, pkg, records)
        assert e.source_curve(1) == mine and e.source_curve(2) == none, records      # a refused call changes nothing
    with pytest.raises(pkg.C2RayHipError, match="nstep = 9"):
        e.set_source_curves([([float(k + 1) for k in range(9)], [1.0] * 10), None])
    assert e.source_curve(1) == mine
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources_begin(1, 1, 2)
    with pytest.raises(pkg.C2RayHipError, match="still open"):
        e.set_source_curves(None)
    with pytest.raises(pkg.C2RayHipError, match="still open"):
        e.set_source_curves([mine, mine])
    e.pass_sources_end()
    assert e.source_curve(1) == mine and e.source_curve(2) == none
    dark = ([0.0], [0.0, 0.0])                                    # the ends are allowed: radius 0, a source gone dark, 8 steps
    full = ([float(k + 1) * 1.0e24 for k in range(8)], [1.0, 0.0, 2.0, 0.0, 0.5, 1.9, 0.25, 3.0 / 7.0, 0.0])
    e.set_source_curves([dark, full])
    assert e.source_curve(1) == dark and e.source_curve(2) == full
    got = one_pass(e)
    assert_grids_equal(got, cr.compose(pkg, orc, otables, case, "gpu16_isothermal", [dark, full]), "a dark source and eight steps")
    lit = cr.factor_cells(case, 1, full) != 0.0
    assert got["sum_nbox"] == 2 and 0 < lit.sum() < lit.size and not got["phih_grid"][~lit].any()
    e.set_sources(pkg.SourceProps(case.srcpos, case.flux, case.s_star))    # c2r_set_sources clears the curves
    assert e.source_curve(1) == none and e.source_curve(2) == none
    e.set_source_curves([None, mine])
    e.set_source_curves(None)
    assert e.source_curve(2) == none
    e.close()


# -- 8. a seeded list of random curves ---------------------------------------------------------------------------------------------------
FUZZ_CASES = int(os.environ.get("C2R_CURVE_FUZZ_CASES", "6"))
FUZZ_SEED = int(os.environ.get("C2R_CURVE_FUZZ_SEED", "2"))


def random_curve(rng, d):
    """None one time in five; else 0..8 ascending radii between 0.4 and 9 cells and factors drawn from FACTORS (a curve without
    a step never draws 0: that record is refused)."""
    if rng.random() < 0.2:
        return None
    nstep = int(rng.integers(0, 9))
    radii = sorted(float(x) * d for x in rng.uniform(0.4, 9.0, size=nstep))
    assert all(b > a for a, b in zip(radii, radii[1:]))
    pool = FACTORS if nstep > 0 else FACTORS[1:]
    return radii, [float(pool[int(k)]) for k in rng.integers(0, len(pool), size=nstep + 1)]


@pytest.mark.parametrize("ic", range(FUZZ_CASES))
def test_random_curves(pkg, orc, otables, tables, ic):
    """Even ids: the periodic 16^3 case; odd ids: the all-open mesh with its escape maps.  One geometric round everywhere."""
    rng = np.random.default_rng([FUZZ_SEED, ic])
    if ic % 2 == 0:
        case, key = case16(pkg, "isothermal"), "gpu16_isothermal"
    else:
        case, key, _ = open_case(pkg, "all_open")
    nsrc, d = len(case.flux), float(case.dr[0])
    curves = [random_curve(rng, d) for _ in range(nsrc)]
    print("case", ic, "seed", FUZZ_SEED, "curves", curves)
    ref = cr.compose(pkg, orc, otables, case, key, curves)
    assert one_round_everywhere(ref)
    e = case.engine(pkg, tables)
    if ic % 2:
        e.enable_face_loss()
    e.set_source_curves(curves)
    got = one_pass(e)
    assert_grids_equal(got, ref, f"fuzz {ic}")
    assert got["sum_nbox"] == nsrc and rounds(e, nsrc) == [1] * nsrc
    if ic % 2:
        maps, _ = cr.compose_maps(pkg, orc, otables, case, key, curves)
        for f in maps:
            assert np.array_equal(e.face_loss_map(f), maps[f]), (ic, f)
    e.close()
