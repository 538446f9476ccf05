"""Beamed point sources (c2r_set_source_beams) on the GPU against the reference of tests/beam_reference.py: the oracle's
do_source per source, a NumPy restatement of the predicate, the fold in source order (tests/test_source_beams_host.py checks
both on the CPU).   python -m pytest tests -m gpu.

The bar: every grid and every map bit for bit (np.array_equal), sum_nbox and the rounds per source exactly; a loss that the
device sums in another order than its reference to 1e-13 relative, the project's bound for such a sum.

The 45-degree cone: no double squares to exactly 0.5, so its cos_half is the double below sqrt(1/2), which lights the cells
with di^2 + dj^2 == dk^2; the beam whose edge is exact in floating point is axis (1,1,0) with cos_half = 0.5 (K = 0.5), used
for the bicone of the three-source case.  tests/test_source_beams_host.py has the arithmetic.
"""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

import axis_boundary_cases as ab
import beam_reference as br
import mix_reference as mr
from conftest import rel_err

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
GRIDS = br.GRIDS
C45 = 0.7071067811865475                    # the double below sqrt(1/2): the cells at exactly 45 degrees are lit
CONE_Z45 = (br.CONE, (0.0, 0.0, 1.0), C45)
FULL_BICONE = (br.BICONE, (0.3, -1.0, 2.0), 0.0)
DT = 1.0e6 * 3.15576e7  # s


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


def sed_tables(pkg, orc, gold):
    t = pkg.RadiationTables.load().add_sed_file(GOLD / "rad_tables_pl_qpl.npz")
    with np.load(pkg.evolve.DEFAULT_TABLES) as z:
        d = {k: z[k] for k in z.files}
    zz = gold("rad_tables_pl_qpl.npz")
    d.update({k: zz[k] for k in zz.files})
    return t, orc.Tables(d)


def one_pass(e, first=1, stride=1):
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources(first, stride)
    return e.download_rates()


def assert_grids_equal(got, ref, what=""):
    for k in GRIDS:
        bad = int(np.count_nonzero(got[k] != ref[k]))
        print(what, k, "cells", got[k].size, "non-zero", int(np.count_nonzero(ref[k])), "differ", bad,
              "worst rel", float(np.max(rel_err(got[k], ref[k]))))
        assert np.array_equal(got[k], ref[k]), (what, k, bad)


# -- periodic 16^3, two sources, one round ------------------------------------------------------------------------------------
def case16(pkg, mode):
    kw = dict(pl=np.array([1e6, 2e6]), qpl=np.array([5e5, 1e6])) if mode == "three_seds" else {}
    return br.periodic_case(pkg, 16, "mixed", [(5, 6, 4), (12, 9, 11)], [3.0e7, 8.0e6], heat=mode != "isothermal", **kw)


@pytest.mark.parametrize("mode", ["isothermal", "heating", "three_seds"])
def test_periodic_16_cone_and_plain_source(pkg, orc, otables, gold, tables, mode):
    """A 45-degree cone along +z on cubic cells and an unbeamed source, every reach one (geometric) round: phih, phihe, phiheat
    and sum_nbox against the reference; the second source as a bicone with cos_half = 0, through k_rates_beam's lit path, gives
    the bits it gives unbeamed; with the beams taken away again the pass is the oracle's own."""
    t, ot = (tables, otables) if mode != "three_seds" else sed_tables(pkg, orc, gold)
    case = case16(pkg, mode)
    beams = [CONE_Z45, None]
    ref = br.compose(pkg, orc, ot, case, "gpu16_" + mode, beams)
    lit = br.lit_cells(case, 0, CONE_Z45)
    assert ref["nbox"] == [1, 1] and 0 < lit.sum() < lit.size // 2
    e = case.engine(pkg, t)
    e.set_source_beams(beams)
    got = one_pass(e)
    assert_grids_equal(got, ref, mode)
    assert got["sum_nbox"] == 2
    assert got["phiheat"].any() == (mode != "isothermal")
    loss = got["photon_loss"][0]
    e.set_source_beams([CONE_Z45, FULL_BICONE])
    again = one_pass(e)
    assert_grids_equal(again, ref, mode + ", full bicone")
    assert again["sum_nbox"] == 2 and again["photon_loss"][0] == loss and loss > 0
    e.set_source_beams(None)
    plain = one_pass(e)
    assert_grids_equal(plain, br.compose(pkg, orc, ot, case, "gpu16_" + mode, [None, None]), mode + ", beams off")
    assert plain["photon_loss"][0] > loss
    # every kind == 0 is no beam as well, and a full bicone on both sources gives those bits through the beamed kernel
    for beams_ in ([(0, (0.0, 0.0, 0.0), 0.0), None], [FULL_BICONE, FULL_BICONE]):
        e.set_source_beams(beams_)
        same = one_pass(e)
        assert_grids_equal(same, plain, mode + ", " + str(beams_[0][0]))
        assert same["photon_loss"][0] == plain["photon_loss"][0] and same["sum_nbox"] == 2
    e.close()


def test_every_route_honours_the_beam(pkg, orc, otables, tables):
    """c2r_do_source source by source, the slab-wise pass, c2r_iteration and c2r_evolve3d on the 16^3 case."""
    case = case16(pkg, "isothermal")
    beams = [CONE_Z45, None]
    ref = br.compose(pkg, orc, otables, case, "gpu16_isothermal", beams)
    e = case.engine(pkg, tables)
    e.set_source_beams(beams)
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
    rep = e.iteration(DT, 1, 1, 2)
    assert rep["conv_flag"] == conv and rep["sum_nbox"] == 2 and rep["photon_loss"][0] == whole["photon_loss"][0]
    it = e.download_iter_state()
    for k in state:
        assert np.array_equal(it[k], state[k]), k
    e.close()

    def evolve(beams_):
        e_ = case.engine(pkg, tables)
        if beams_ is not None:
            e_.set_source_beams(beams_)
        niter, _ = e_.evolve3d(DT)
        mat = pkg.Material(case.region[0], None, None, None, True, 1.0e4, 1.0, case.reccoef)
        e_.download_state(mat)
        e_.close()
        return niter, mat.xh

    _, plain = evolve(None)
    _, full = evolve([FULL_BICONE, FULL_BICONE])
    _, beamed = evolve(beams)
    assert np.array_equal(plain, full) and not np.array_equal(plain, beamed)


# -- periodic 32^3, ionised gas, three sources, two rounds each ------------------------------------------------------------------
BEAMS32 = [(br.CONE, (1.0, 2.0, -1.0), float(np.cos(np.radians(30.0)))), (br.BICONE, (1.0, 1.0, 0.0), 0.5), None]


@pytest.fixture(scope="module")
def case32(pkg):
    return br.periodic_case(pkg, 32, "ionised", [(4, 30, 9), (17, 16, 20), (28, 7, 31)], [2.0e7, 1.0e7, 1.5e7])


@pytest.mark.parametrize("how", ["one_batch", "batch_of_1", "stride_2"])
def test_periodic_32_ionised_cone_and_bicone(pkg, orc, otables, tables, case32, how):
    """Every source runs both of its rounds, lit or not: c2r_get_source_trace's nbox equals the oracle's, the grids the
    reference's, for one batch, for c2r_set_batch(1) and for a stride-2 deal (sources 1 and 3, then 2: folded in that order)."""
    case = case32
    order = [1, 3, 2] if how == "stride_2" else [1, 2, 3]
    ref = br.compose(pkg, orc, otables, case, "gpu32", BEAMS32, sources=order)
    assert ref["nbox"] == [2, 2, 2]
    e = case.engine(pkg, tables)
    e.set_source_beams(BEAMS32)
    if how == "batch_of_1":
        e.set_batch(1)
    if how == "stride_2":
        one_pass(e, 1, 2)
        assert [e.source_trace(ns)["nbox"] for ns in (1, 3)] == [2, 2] and e.get_loss()[1] == 4
        e.pass_sources(2, 2)                                    # no zeroing in between: grids, loss and sum_nbox add up
        got = e.download_rates()
        assert got["sum_nbox"] == 6
    else:
        got = one_pass(e)
        assert got["sum_nbox"] == 6
    assert [e.source_trace(ns)["nbox"] for ns in (1, 2, 3)] == ref["nbox"]
    assert_grids_equal(got, ref, how)
    for ns in (1, 2):       # a beam leaves most of the mesh dark, and a bicone lights more than nothing on both sides
        lit = br.lit_cells(case, ns - 1, BEAMS32[ns - 1])
        assert 0 < lit.sum() < lit.size // 2
    e.close()


# -- an opaque wall in front of the cone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("heat", [False, True], ids=["isothermal", "heating"])
def test_wall_in_front_of_the_cone_ends_the_box_loop(pkg, orc, otables, tables, heat):
    """tests/beam_reference.py's wall case (the CPU test asserts its columns): unbeamed, oracle and product need both rounds;
    beamed, every lit surface cell of the first box loses exactly 0.0, the product stops after round 1 with photon_loss(1) ==
    0.0, and the grids are the masked oracle grids inside the first box and 0 outside."""
    case = br.wall_case(pkg, heat=heat)
    key = "wall_heat" if heat else "wall"
    ref = br.compose(pkg, orc, otables, case, key, [br.WALL_BEAM], inside={1: br.first_box(case)})
    assert ref["nbox"] == [2]
    e = case.engine(pkg, tables)
    plain = one_pass(e)
    assert plain["sum_nbox"] == 2 and e.source_trace(1)["nbox"] == 2 and plain["photon_loss"][0] > 0
    assert_grids_equal(plain, br.compose(pkg, orc, otables, case, key, [None]), "unbeamed")
    e.set_source_beams([br.WALL_BEAM])
    for again in range(2):          # the second pass starts from what the first learnt about the source
        got = one_pass(e)
        assert got["sum_nbox"] == 1 and e.source_trace(1)["nbox"] == 1
        assert got["photon_loss"][0] == 0.0
        assert_grids_equal(got, ref, f"beamed, pass {again}")
    outside = ~br.first_box(case)
    assert outside.any() and not got["phih_grid"][outside].any() and got["phih_grid"].any()
    e.close()


# -- all axes open, escape maps ------------------------------------------------------------------------------------------------
OPEN_SOURCES, OPEN_FLUX = [(3, 6, 5), (9, 2, 11)], [3.0e7, 8.0e6]
OPEN_CONE = (br.CONE, (1.0, 0.25, -0.1), float(np.cos(np.radians(25.0))))


def test_all_axes_open_with_escape_maps(pkg, orc, otables, tables):
    """open_boundary_cases.case_one_round's box (11^3 in 24^3, mix_reference's "xyz" meshes, cells that are no cubes), two
    sources, the first beamed: grids and maps against the reference; the maps' sum is photon_loss(1) to rounding (isothermal:
    the loss comes from the terms k_rates_beam left behind, 0.0 for the unlit surface cells); the beamed source alone leaves
    the faces no lit cell touches at zero."""
    case = mr.make_case(pkg, "xyz", OPEN_SOURCES, OPEN_FLUX)
    beams = [OPEN_CONE, None]
    ref = br.compose(pkg, orc, otables, case, "open_xyz", beams)
    maps, per_source = br.compose_maps(pkg, orc, otables, case, "open_xyz", beams)
    e = case.engine(pkg, tables)
    e.enable_face_loss()
    e.set_source_beams(beams)
    got = one_pass(e)
    assert_grids_equal(got, ref, "open")
    assert got["sum_nbox"] == 2
    for f in range(6):
        assert np.array_equal(e.face_loss_map(f), maps[f]), f
    total, loss = math.fsum(e.face_loss()), got["photon_loss"][0]
    want = math.fsum(float(x) for f in maps for x in maps[f].reshape(-1))
    print("sum of the maps", total, "photon_loss(1)", loss, "reference", want, "rel", rel_err(total, loss), rel_err(loss, want))
    assert loss > 0 and rel_err(total, loss) <= 1e-13 and rel_err(loss, want) <= 1e-13
    e.close()
    # the beamed source alone: the cone leaves through x = 11 (face 1) and leaves x = 1 (face 0) and others dark
    dark = [f for f in range(6) if not per_source[0][f].any()]
    assert 0 in dark and 1 not in dark and per_source[0][1].any()
    e = case.engine(pkg, tables, sources=[0])
    e.enable_face_loss()
    e.set_source_beams([OPEN_CONE])
    alone = one_pass(e)
    for f in range(6):
        m = e.face_loss_map(f)
        assert np.array_equal(m, per_source[0][f]), f
        assert m.any() == (f not in dark)
    assert rel_err(math.fsum(e.face_loss()), alone["photon_loss"][0]) <= 1e-13
    e.close()


# -- a mixed mode: z open, x and y periodic -------------------------------------------------------------------------------------
def test_mixed_mode_cone_across_a_periodic_face(pkg, orc, otables, tables):
    """mix_reference.case_a (11^3, z open): the source at (1,1,1) beams towards -x, -y and +z, so its cone lives on the images
    beyond the periodic x and y faces: the predicate sees the offsets within the periodic reach, not the mesh differences."""
    case = mr.case_a(pkg)
    cone = (br.CONE, (-1.0, -0.5, 1.0), float(np.cos(np.radians(40.0))))
    beams = [cone, None, (br.BICONE, (0.0, 1.0, 0.2), 0.8), None]
    ref = br.compose(pkg, orc, otables, case, "mix_a", beams)
    di, dj, dk = br.offsets(case.n, case.srcpos[0], case.periodic)
    lit = br.lit_cells(case, 0, cone).reshape(di.shape)
    assert np.any(lit & (di < 0)) and not np.any(lit & (di > 0) & (dj > 0))       # lit cells sit at mesh x = 7..11: images
    e = case.engine(pkg, tables)
    e.set_source_beams(beams)
    got = one_pass(e)
    assert_grids_equal(got, ref, "mixed")
    assert got["sum_nbox"] == 4
    e.close()


# -- c2r_evolve0d cell by cell ---------------------------------------------------------------------------------------------------
def test_evolve0d_cell_by_cell_is_do_source(pkg, tables):
    """One beamed source at 8^3, periodic: c2r_evolve0d over the cells of its reach in shell order gives the bits of
    c2r_do_source; the loss of an unlit surface cell is 0.0, and the losses add up to photon_loss(1)."""
    case = br.periodic_case(pkg, 8, "ionised", [(3, 6, 2)], [2.0e7], cubic=False)
    beam = (br.CONE, (1.0, -1.0, 0.5), float(np.cos(np.radians(50.0))))
    e = case.engine(pkg, tables)
    e.set_source_beams([beam])
    e.begin_step()
    e.set_rates_to_zero()
    e.do_source(1)
    ref = e.download_rates()
    assert ref["sum_nbox"] == 1
    e.begin_step()
    e.set_rates_to_zero()
    lo, hi = case.reach(0)
    assert (lo, hi) == ([-4] * 3, [3] * 3)
    offs = [(i, j, k) for k in range(-4, 4) for j in range(-4, 4) for i in range(-4, 4)]
    offs.sort(key=lambda o: max(abs(o[0]), abs(o[1]), abs(o[2])))
    lit_terms, dark_terms = [], []
    for o in offs:
        surface = any(x in (-4, 3) for x in o)
        pos = (C.c_int * 3)(*(int(p) + x for p, x in zip(case.srcpos[0], o)))
        loss = C.c_double(-1.0)
        e._chk(e.lib.c2r_evolve0d(e.h, pos, 1, 1, int(surface), C.byref(loss)))
        if surface:
            (lit_terms if bool(br.lit_offsets(beam, case.dr, *o)) else dark_terms).append(loss.value)
    got = e.download_rates()
    assert_grids_equal(got, ref, "evolve0d")
    assert len(dark_terms) > len(lit_terms) > 10
    assert all(x == 0.0 for x in dark_terms) and all(x > 0.0 for x in lit_terms)
    expected = float(np.sum(np.sort(np.array(lit_terms))))
    print("photon_loss(1)", ref["photon_loss"][0], "sum of the per-cell losses", expected, "rel", rel_err(ref["photon_loss"][0], expected))
    assert rel_err(ref["photon_loss"][0], expected) <= 1e-13
    e.close()


# -- several devices -----------------------------------------------------------------------------------------------------------
def two_device_pass(pkg, orc, otables, tables, devices):
    case = case16(pkg, "isothermal")
    beams = [CONE_Z45, (br.BICONE, (1.0, 1.0, 0.0), 0.5)]
    ref = br.compose(pkg, orc, otables, case, "gpu16_isothermal", beams)     # (0 + a) + (0 + b): the sum of the two devices' grids
    hp = pkg.hostphys
    ndens, xh, xhe, _ = case.region
    mat = pkg.Material(ndens, xh.copy(), xhe.copy(), None, True, 1.0e4, 1.0, case.reccoef)
    e = pkg.HipEngine(case.n, devices)
    e.set_tables(tables)
    e.set_step(mat, pkg.GridProps(case.n, case.dr, case.vol), pkg.Cosmology(ab.ZRED, hp.H0, hp.Omega0))
    e.set_sources(pkg.SourceProps(case.srcpos, case.flux, case.s_star))
    e.upload_state(mat)
    e.comm_init_local()
    assert e.num_devices() == 2
    e.set_source_beams(beams)
    assert e.source_beam(2)["kind"] == br.BICONE
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    e.allreduce_rates()
    got = e.download_rates()
    assert_grids_equal(got, ref, f"devices {devices}")
    assert got["sum_nbox"] == 2
    e.close()


def test_two_replicas_on_one_device(pkg, orc, otables, tables):
    """c2r_create_multi([0, 0]): device 0 sweeps the cone's source, device 1 the bicone's; the beams reach both."""
    two_device_pass(pkg, orc, otables, tables, [0, 0])


def test_two_devices(pkg, orc, otables, tables):
    if int(pkg._lib.load().c2r_device_count()) < 2:
        pytest.skip("needs two HIP devices")
    two_device_pass(pkg, orc, otables, tables, [0, 1])


# -- lifetime and refusals --------------------------------------------------------------------------------------------------------
def test_lifetime_and_refusals(pkg, tables):
    case = case16(pkg, "isothermal")
    e = case.engine(pkg, tables)
    none = {"kind": 0, "axis": [0.0, 0.0, 0.0], "cos_half": 0.0}
    assert e.source_beam(1) == none and e.source_beam(2) == none
    e.set_source_beams([{"kind": "cone", "axis": (1.0, 2.0, -1.0), "cos_half": 0.25}, None])
    assert e.source_beam(1) == {"kind": 1, "axis": [1.0, 2.0, -1.0], "cos_half": 0.25} and e.source_beam(2) == none
    with pytest.raises(pkg.C2RayHipError):
        e.source_beam(3)
    e.set_boundaries((True, True, False))                       # the boundaries keep the beams
    assert e.source_beam(1)["kind"] == 1
    e.set_boundaries(True)
    good = e.source_beam(1)
    nan, inf = float("nan"), float("inf")
    bad = [[(3, (0.0, 0.0, 1.0), 0.5), None], [(-1, (0.0, 0.0, 1.0), 0.5), None],
           [(1, (nan, 0.0, 1.0), 0.5), None], [None, (2, (0.0, inf, 1.0), 0.5)],
           [(1, (0.0, 0.0, 0.0), 0.5), None], [(1, (1.0e-170, 0.0, 0.0), 0.5), None], [(1, (1.0e200, 0.0, 0.0), 0.5), None],
           [(1, (0.0, 0.0, 1.0), -0.1), None], [(1, (0.0, 0.0, 1.0), 1.0000001), None], [(2, (0.0, 0.0, 1.0), nan), None],
           [(1, (0.0, 0.0, 1.0), 0.5)], [(1, (0.0, 0.0, 1.0), 0.5), None, None]]      # the last two: nsrc != NumSrc
    for beams in bad:
        with pytest.raises(pkg.C2RayHipError, match="c2r_set_source_beams"):
            e.set_source_beams(beams)
        assert e.source_beam(1) == good, beams                  # a refused call changes nothing
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources_begin(1, 1, 2)
    with pytest.raises(pkg.C2RayHipError, match="still open"):
        e.set_source_beams(None)
    e.pass_sources_end()
    assert e.source_beam(1) == good
    e.set_source_beams([(1, (0.0, 0.0, 1.0), 0.0), (2, (0.0, 0.0, 1.0), 1.0)])      # the ends of [0, 1] are allowed
    e.set_sources(pkg.SourceProps(case.srcpos, case.flux, case.s_star))    # c2r_set_sources clears the beams
    assert e.source_beam(1) == none and e.source_beam(2) == none
    e.set_source_beams([None, CONE_Z45])
    e.set_source_beams(None)
    assert e.source_beam(2) == none
    e.close()
