"""Horizon loss (c2r_enable_horizon_loss) on the GPU against tests/rim_reference.py: the restated rule of csrc/c2ray_rim.hpp
composed with the oracle -- the oracle's columns of the source alone, orc_cinterp, the oracle's photoion_rates(...)[20] at the
rim cells (tests/test_horizon_loss_host.py checks the rule itself on the CPU).   python -m pytest tests -m gpu.

The bar: the downloaded terms bit for bit (np.array_equal), a source's loss == the Python face_sum of the expected terms.
Meshes are 16^3 and 11^3 / 24^3-embedded boxes, every reach one geometric round.
"""
import ctypes as C

import numpy as np
import pytest

import axis_boundary_cases as ab
import beam_reference as br
import face_loss_reference as fl
import mix_reference as mr
import rim_reference as rr
from test_gpu_source_beams import CONE_Z45, DT, GRIDS, case16, one_pass, sed_tables
from test_gpu_source_horizons import open_case

pytestmark = pytest.mark.gpu
INF = float("inf")
SIGMA_HI = float(np.float32(6.346e-18))


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


def expected(pkg, orc, ot, case, key, e, ns, radius, beam=None):
    """The expected terms of source ns (1-based) for the final box the context reports, which must be the rule's."""
    tr = e.source_trace(ns)
    lo, hi = rr.final_box(case, ns - 1, tr["nbox"])
    assert tr["nbox"] >= 1 and lo == tr["box_lo"] and hi == tr["box_hi"], (tr, lo, hi)
    terms, rule = rr.source_terms(pkg, orc, ot, case, key, ns - 1, radius, lo, hi, beam)
    return terms, rule, rr.extents(lo, hi)


def check_last(e, ns, ext, terms, what):
    got_ns, got_ext, got = e.horizon_rim()
    bad = int(np.count_nonzero(got != terms)) if got.shape == terms.shape else -1
    print(what, "source", got_ns, "extents", got_ext, "terms", got.size, "faces", int(np.count_nonzero(terms)), "differ", bad,
          "sum", rr.face_sum(got))
    assert got_ns == ns and got_ext == ext
    assert np.array_equal(got, terms), (what, bad)
    assert not np.signbit(got).any()


def snapshot(e, got, faces=()):
    """Everything the feature must not change: grids, photon_loss, sum_nbox and the escape maps of `faces`."""
    out = {k: got[k].copy() for k in GRIDS}
    out["photon_loss"], out["sum_nbox"] = e.get_loss()[0].copy(), got["sum_nbox"]
    for f in faces:
        out[f"face{f}"] = e.face_loss_map(f)
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


# -- 1. periodic 16^3, one horizoned and one plain source ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["isothermal", "heating", "three_seds"])
def test_periodic_16_horizon_and_plain_source(pkg, orc, otables, gold, tables, mode):
    t, ot = (tables, otables) if mode != "three_seds" else sed_tables(pkg, orc, gold)
    case = case16(pkg, mode)
    radius = 5.3 * float(case.dr[0])
    e = case.engine(pkg, t)
    e.enable_horizon_loss()
    assert e.horizon_loss_enabled
    e.set_source_horizons([radius, None])
    one_pass(e)
    terms, rule, ext = expected(pkg, orc, ot, case, "rim16_" + mode, e, 1, radius)
    assert ext == [16, 16, 16] and terms.size == 6 * 256 and 100 < rule["face"].sum() and np.all(terms[rule["face"]] > 0)
    check_last(e, 1, ext, terms, mode)
    per, total = e.horizon_loss()
    want = rr.face_sum(terms)
    print(mode, "horizon loss", per, "expected", want, "photon_loss(1)", e.get_loss()[0][0], "flux", float(case.flux[0]) * case.s_star)
    assert per[0] == want and per[0] > 0
    assert per[1] == 0.0 and total == per[0] + per[1]
    e.close()


# -- 2. identity -------------------------------------------------------------------------------------------------------------------
def test_feature_changes_nothing_else(pkg, tables):
    case, key, radii = open_case(pkg, "all_open")
    d = float(case.dr[0])
    horizons = [r if r is None or r == INF else r * d for r in radii]
    snaps, launches = {}, {}
    for on in (False, True):
        e = case.engine(pkg, tables)
        e.enable_face_loss()
        if on:
            e.enable_horizon_loss()
        e.set_source_horizons(horizons)
        got = one_pass(e)
        snaps[on] = snapshot(e, got, fl.open_faces(case.periodic))
        launches[on, "finite"] = e.timing().sweep_launches
        e.set_source_horizons([INF, None])
        one_pass(e)
        launches[on, "none"] = e.timing().sweep_launches
        e.set_source_horizons(None)
        one_pass(e)
        launches[on, "unset"] = e.timing().sweep_launches
        if on:
            assert np.all(e.horizon_loss()[0] == 0.0)
        e.close()
    assert_same(snaps[False], snaps[True], "feature on against off")
    assert sum(k.startswith("face") for k in snaps[True]) == 6 and snaps[True]["face0"].any()
    print("sweep launches", launches)
    assert launches[True, "none"] == launches[False, "none"] and launches[True, "unset"] == launches[False, "unset"]
    assert launches[True, "finite"] == launches[False, "finite"] + 2          # k_horizon_rim and its finishing launch
    case = case16(pkg, "isothermal")
    for on in (False, True):
        e = case.engine(pkg, tables)
        if on:
            e.enable_horizon_loss()
        e.set_source_horizons([5.3 * float(case.dr[0]), None])
        snaps[on] = snapshot(e, one_pass(e))
        e.close()
    assert_same(snaps[False], snaps[True], "periodic, feature on against off")


# -- 3. the box cut by the mesh ----------------------------------------------------------------------------------------------------
def cut_case(pkg, which):
    if which == "all_open":       # (3,6,5) of the 11^3 box: two cells from the face x = 1, radius 4 d
        return open_case(pkg, "all_open")
    case = mr.make_case(pkg, "z", [(6, 6, 3), (2, 9, 9)], [3.0e7, 8.0e6])       # (6,6,3): two cells of 0.75 d from the face z = 1
    return case, "rim_z", [4.0, None]


@pytest.mark.parametrize("which", ["all_open", "z_open"])
def test_box_cut_by_the_mesh(pkg, orc, otables, tables, which):
    case, key, radii = cut_case(pkg, which)
    d = float(case.dr[0])
    horizons = [r if r is None or r == INF else r * d for r in radii]
    maps = {}
    for on in (False, True):
        e = case.engine(pkg, tables)
        e.enable_face_loss()
        if on:
            e.enable_horizon_loss()
        e.set_source_horizons(horizons)
        got = one_pass(e)
        maps[on] = snapshot(e, got, fl.open_faces(case.periodic))
        if not on:
            e.close()
    assert_same(maps[False], maps[True], which + ": escape maps, grids and losses")
    terms, rule, ext = expected(pkg, orc, otables, case, "rim_" + key, e, 1, horizons[0])
    lo, hi = rr.final_box(case, 0, 1)
    assert 2 in [-x for x in lo] + list(hi)                      # the source sits two cells from a face of the mesh
    ended_on_surface = np.array([k >= 0 and any(c[a] in (lo[a], hi[a]) for a in range(3)) for c, k in zip(rule["cell"], rule["kstar"])])
    print(which, "box", lo, hi, "columns", terms.size, "faces", int(rule["face"].sum()), "columns that end on the surface", int(ended_on_surface.sum()))
    assert ended_on_surface.sum() > 0 and not rule["face"][ended_on_surface].any() and np.all(terms[ended_on_surface] == 0.0)
    check_last(e, 1, ext, terms, which)
    per, total = e.horizon_loss()
    assert per[0] == rr.face_sum(terms) and per[0] > 0 and np.all(per[1:] == 0.0)
    e.close()


# -- 4. cells that are no cubes ----------------------------------------------------------------------------------------------------
def test_cells_that_are_no_cubes(pkg, orc, otables, tables):
    case = br.periodic_case(pkg, 16, "mixed", [(5, 6, 4), (12, 9, 11)], [3.0e7, 8.0e6], cubic=False)
    d = float(case.dr[0])
    horizons = [4.4 * d, 6.1 * d]
    e = case.engine(pkg, tables)
    e.enable_horizon_loss()
    e.set_source_horizons(horizons)
    one_pass(e)
    per, total = e.horizon_loss()
    for ns in (1, 2):
        terms, rule, ext = expected(pkg, orc, otables, case, "rim16_box", e, ns, horizons[ns - 1])
        assert per[ns - 1] == rr.face_sum(terms) and per[ns - 1] > 0, ns
    check_last(e, 2, ext, terms, "non-cubic")                   # the source swept last
    assert total == per[0] + per[1]
    e.close()


# -- 5. a beam and a horizon on one source -----------------------------------------------------------------------------------------
def test_beam_and_horizon_on_one_source(pkg, orc, otables, tables):
    case = case16(pkg, "isothermal")
    dr = float(case.dr[0])
    beams, horizons = [None, CONE_Z45], [6.0 * dr, 5.5 * dr]
    e = case.engine(pkg, tables)
    e.enable_horizon_loss()
    e.set_source_horizons(horizons)
    e.set_source_beams(beams)
    one_pass(e)
    terms, rule, ext = expected(pkg, orc, otables, case, "rim16_isothermal", e, 2, horizons[1], CONE_Z45)
    bare = rr.columns(horizons[1], case.dr, *rr.final_box(case, 1, 1))
    unlit = bare["face"] & ~rule["face"]
    print("faces", int(bare["face"].sum()), "of them beam-unlit", int(unlit.sum()))
    assert 0 < unlit.sum() < bare["face"].sum() and np.all(terms[unlit] == 0.0) and not np.signbit(terms[unlit]).any()
    check_last(e, 2, ext, terms, "cone and horizon")
    per, _ = e.horizon_loss()
    assert per[1] == rr.face_sum(terms)
    assert per[0] == rr.face_sum(expected(pkg, orc, otables, case, "rim16_isothermal", e, 1, horizons[0])[0])
    e.close()


# -- 6. radius 0 and radius below the smallest dr ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", ["cubic", "box"])
def test_own_cell_only(pkg, orc, otables, tables, cells):
    case = br.periodic_case(pkg, 16, "mixed", [(5, 6, 4), (12, 9, 11)], [3.0e7, 8.0e6], cubic=cells == "cubic")
    key = "rim16_isothermal" if cells == "cubic" else "rim16_box"
    e = case.engine(pkg, tables)
    e.enable_horizon_loss()
    for radius in (0.0, 0.6 * min(float(x) for x in case.dr)):
        e.set_source_horizons([None, radius])
        one_pass(e)
        terms, rule, ext = expected(pkg, orc, otables, case, key, e, 2, radius)
        po = rr.cell_photo_out(pkg, orc, otables, case, key, 1, (0, 0, 0))
        assert rule["face"].sum() == 6 and np.all(terms[rule["face"]] == po * (1.0 / 6.0)) and po > 0
        check_last(e, 2, ext, terms, f"radius {radius}")
        per, _ = e.horizon_loss()
        print(cells, "radius", radius, "loss", per[1], "po", po, "loss / po", per[1] / po)
        assert per[1] == rr.face_sum(np.full(6, po * (1.0 / 6.0))) == rr.face_sum(terms) and per[0] == 0.0
    e.close()


# -- 7. three sources, batches, passes ---------------------------------------------------------------------------------------------
def test_three_sources_batches_and_passes(pkg, orc, otables, tables):
    case = br.periodic_case(pkg, 16, "mixed", [(5, 6, 4), (12, 9, 11), (3, 14, 8)], [3.0e7, 8.0e6, 1.5e7])
    dr = float(case.dr[0])
    horizons = [5.3 * dr, 3.7 * dr, 6.2 * dr]
    e = case.engine(pkg, tables)
    e.enable_horizon_loss()
    e.set_source_horizons(horizons)
    one_pass(e)
    one, total = e.horizon_loss()
    for ns in (1, 2, 3):
        terms, _, ext = expected(pkg, orc, otables, case, "rim16_three", e, ns, horizons[ns - 1])
        assert one[ns - 1] == rr.face_sum(terms) and one[ns - 1] > 0, ns
    check_last(e, 3, ext, terms, "three sources")
    assert total == (one[0] + one[1]) + one[2]
    e.pass_sources(1, 1)                                         # a second pass: loss = loss + (the same sum)
    twice, _ = e.horizon_loss()
    assert np.array_equal(twice, one + one)
    e.set_rates_to_zero()
    assert np.all(e.horizon_loss()[0] == 0.0) and e.horizon_loss()[1] == 0.0
    e.set_batch(1)
    one_pass(e)
    assert np.array_equal(e.horizon_loss()[0], one)
    check_last(e, 3, ext, terms, "batch of 1")
    e.set_batch(2)
    one_pass(e, 1, 2)                                            # sources 1 and 3, then source 2: the last one swept is 2
    one_pass_2 = e.horizon_loss()[0]
    assert one_pass_2[0] == one[0] and one_pass_2[2] == one[2] and one_pass_2[1] == 0.0
    e.pass_sources(2, 2)
    assert np.array_equal(e.horizon_loss()[0], one) and e.horizon_rim()[0] == 2
    e.close()


# -- 8. every route ----------------------------------------------------------------------------------------------------------------
def test_every_route_gives_the_same_bits(pkg, tables):
    case = case16(pkg, "isothermal")
    dr = float(case.dr[0])
    horizons = [5.3 * dr, 6.0 * dr]
    e = case.engine(pkg, tables)
    e.enable_horizon_loss()
    e.set_source_horizons(horizons)
    one_pass(e)
    ref, ref_total = e.horizon_loss()
    assert np.all(ref > 0)
    e.begin_step()
    e.set_rates_to_zero()
    e.do_source(1)
    assert np.array_equal(e.horizon_loss()[0], [ref[0], 0.0]) and e.horizon_rim()[0] == 1
    e.do_source(2)
    assert np.array_equal(e.horizon_loss()[0], ref)
    e.begin_step()
    e.set_rates_to_zero()
    for s in range(e.pass_sources_begin(1, 1, 3)):
        e.pass_wait_slab(s)
    with pytest.raises(pkg.C2RayHipError, match="still open"):
        e.horizon_loss()
    with pytest.raises(pkg.C2RayHipError, match="still open"):
        e.horizon_rim()
    e.pass_sources_end()
    assert np.array_equal(e.horizon_loss()[0], ref)
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_allreduce_chemistry(DT, 1, 1, 2)
    assert np.array_equal(e.horizon_loss()[0], ref)
    e.close()
    # c2r_iteration and c2r_evolve3d against the same steps driven by their pieces (the columns change with the iterations)
    e = case.engine(pkg, tables)
    e.enable_horizon_loss()
    e.set_source_horizons(horizons)
    one_pass(e)
    e.global_pass(DT)
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    second = e.horizon_loss()[0]
    e.close()
    e = case.engine(pkg, tables)
    e.enable_horizon_loss()
    e.set_source_horizons(horizons)
    e.begin_step()
    e.set_rates_to_zero()
    e.iteration(DT, 1, 1, 2)
    assert np.array_equal(e.horizon_loss()[0], ref)
    e.set_rates_to_zero()
    e.iteration(DT, 1, 1, 2)
    assert np.array_equal(e.horizon_loss()[0], second) and not np.array_equal(second, ref)
    e.close()

    def by_pieces():
        e_ = case.engine(pkg, tables)
        e_.enable_horizon_loss()
        e_.set_source_horizons(horizons)
        criterion = min(int(pkg.evolve.convergence_fraction * ab.cells(case.n)), len(case.flux))
        e_.begin_step()
        niter, flag = 0, ab.cells(case.n)
        while not (flag < criterion and niter > 1) and niter <= 500:
            niter += 1
            e_.set_rates_to_zero()
            e_.pass_sources(1, 1)
            flag = e_.global_pass(DT)
        e_.end_step()
        out = e_.horizon_loss()[0]
        e_.close()
        return niter, out

    e = case.engine(pkg, tables)
    e.enable_horizon_loss()
    e.set_source_horizons(horizons)
    niter, _ = e.evolve3d(DT)
    last = e.horizon_loss()[0]
    e.close()
    pieces = by_pieces()
    print("evolve3d: iterations", niter, "horizon loss of the last pass", last, "by pieces", pieces)
    assert niter == pieces[0] and np.array_equal(last, pieces[1]) and np.all(last > 0)


def test_two_replicas_on_one_device(pkg, tables):
    """c2r_create_multi([0, 0]): device 0 sweeps source 1, device 1 source 2; each answers for its own source."""
    case = case16(pkg, "isothermal")
    dr = float(case.dr[0])
    horizons = [5.3 * dr, 6.0 * dr]
    e = case.engine(pkg, tables)
    e.enable_horizon_loss()
    e.set_source_horizons(horizons)
    one_pass(e)
    ref, ref_total = e.horizon_loss()
    e.close()
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
    e.enable_horizon_loss()
    e.set_source_horizons(horizons)
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    e.allreduce_rates()
    per, total = e.horizon_loss()
    assert np.array_equal(per, ref) and total == ref_total
    assert e.horizon_rim()[0] in (1, 2)
    e.close()


# -- 9. the thin limit: the horizon closes the budget -------------------------------------------------------------------------------
def test_thin_limit_closes_the_budget(pkg, orc, otables, tables):
    case = br.periodic_case(pkg, 16, "mixed", [(8, 8, 8)], [3.0e7])
    radius = 5.3 * float(case.dr[0])
    e = case.engine(pkg, tables)
    e.enable_horizon_loss()
    e.set_source_horizons([radius])
    one_pass(e)
    cols = e.download_columns()
    thickest = max(float(cols["coldensh_out"].max()), float(cols["coldenshe_out"].max()))
    e.scale_ndens(thickest * 1.0e-17 * 1.0e12)                   # every column below 1e-12 of 1e17 cm^-2 ~ 1/sigma
    one_pass(e)
    cols = e.download_columns()
    thickest = max(float(cols["coldensh_out"].max()), float(cols["coldenshe_out"].max()))
    print("thickest column", thickest, "times sigma_HI", thickest * SIGMA_HI)
    assert 0 < thickest * SIGMA_HI < 1.0e-6
    loss = e.horizon_loss()[0][0]
    lo, hi = rr.final_box(case, 0, 1)
    sum_w = rr.face_sum(rr.columns(radius, case.dr, lo, hi)["w"])
    po0 = float(orc.photoion_rates(otables, [0.0] * 6, float(case.vol), float(case.flux[0]), 1.0, True)[20])
    print("loss", loss, "po at zero columns", po0, "loss / po", loss / po0, "sum of w", sum_w, "photon_loss(1)", e.get_loss()[0][0])
    assert po0 > 0 and abs(loss / po0 - sum_w) <= 1e-9
    assert abs(sum_w - 1.0) <= 1e-3
    assert e.get_loss()[0][0] == 0.0                             # nothing reaches the box's surface: the horizon loss is all
    e.close()


# -- 10. lifetime and refusals -------------------------------------------------------------------------------------------------------
def test_lifetime_and_refusals(pkg, tables):
    case = case16(pkg, "isothermal")
    dr = float(case.dr[0])
    e = case.engine(pkg, tables)
    assert not e.horizon_loss_enabled
    for call in (e.horizon_loss, e.horizon_rim):                 # off: refused
        with pytest.raises(pkg.C2RayHipError, match="c2r_enable_horizon_loss"):
            call()
    e.enable_horizon_loss()
    e.enable_horizon_loss()                                      # twice is once
    assert e.horizon_loss_enabled and np.array_equal(e.horizon_loss()[0], [0.0, 0.0])
    with pytest.raises(pkg.C2RayHipError, match="no source with a finite horizon"):
        e.horizon_rim()
    one_pass(e)                                                  # no horizons: still nothing to download
    with pytest.raises(pkg.C2RayHipError, match="no source with a finite horizon"):
        e.horizon_rim()
    e.set_source_horizons([5.3 * dr, None])
    one_pass(e)
    first = e.horizon_loss()[0]
    assert first[0] > 0 and first[1] == 0.0
    per, tot = np.zeros(3), C.c_double(0.0)
    dp = C.POINTER(C.c_double)
    for nsrc in (1, 3):                                          # nsrc != NumSrc
        assert e.lib.c2r_get_horizon_loss(e.h, nsrc, per.ctypes.data_as(dp), C.byref(tot)) != 0
        assert "nsrc" in e.lib.c2r_last_error(e.h).decode()
    assert e.lib.c2r_get_horizon_loss(e.h, 2, None, C.byref(tot)) == 0 and tot.value == first[0]      # per_source may be NULL
    ns, ext, out = C.c_int(0), (C.c_int * 3)(), np.zeros(6 * 256)
    for cap in (0, 6 * 256 - 1):                                 # capacity < T: refused, T reported
        assert e.lib.c2r_download_horizon_rim(e.h, C.byref(ns), ext, out.ctypes.data_as(dp), cap) != 0
        assert "T = 1536" in e.lib.c2r_last_error(e.h).decode() and ns.value == 1 and list(ext) == [16, 16, 16]
    assert e.lib.c2r_download_horizon_rim(e.h, C.byref(ns), ext, out.ctypes.data_as(dp), 6 * 256) == 0 and out.any()
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources_begin(1, 1, 2)
    for on in (False, True):                                     # between begin and end: refused
        with pytest.raises(pkg.C2RayHipError, match="still open"):
            e.enable_horizon_loss(on)
    e.pass_sources_end()
    assert np.array_equal(e.horizon_loss()[0], first)
    e.set_source_horizons([5.3 * dr, 4.0 * dr])                  # new horizons zero the values ...
    assert np.all(e.horizon_loss()[0] == 0.0)
    one_pass(e)
    assert np.all(e.horizon_loss()[0] > 0)
    e.set_boundaries((True, True, False))                        # ... so does a change of boundary mode ...
    assert np.all(e.horizon_loss()[0] == 0.0)
    e.set_boundaries(True)
    one_pass(e)
    assert np.all(e.horizon_loss()[0] > 0)
    e.set_sources(pkg.SourceProps(case.srcpos, case.flux, case.s_star))       # ... and c2r_set_sources (which clears the horizons)
    assert np.all(e.horizon_loss()[0] == 0.0)
    with pytest.raises(pkg.C2RayHipError, match="no source with a finite horizon"):
        e.horizon_rim()
    e.enable_horizon_loss(False)
    assert not e.horizon_loss_enabled
    with pytest.raises(pkg.C2RayHipError, match="c2r_enable_horizon_loss"):
        e.horizon_loss()
    e.set_source_horizons([5.3 * dr, None])
    one_pass(e)                                                  # off again: the pass runs as it always did
    e.close()
