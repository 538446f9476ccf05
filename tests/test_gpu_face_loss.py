"""Escape maps (c2r_enable_face_loss): the kept photon loss of open boxes per cell of the open mesh face it leaves through, on
the GPU, against the reference of tests/face_loss_reference.py (the oracle's columns, cinterp and photoion_rates per face
cell, a NumPy restatement of the attribution rule; tests/test_face_loss_host.py checks both on the CPU).
python -m pytest tests -m gpu.

The bar: every map bit for bit (np.array_equal); the six totals of c2r_get_face_loss, and where the identity holds (all axes
open, every final box its source's whole reach) their sum against photon_loss(1), to 1e-13 relative -- the project's bound
for one loss summed in another order.
"""
import math
from pathlib import Path

import numpy as np
import pytest

import axis_boundary_cases as ab
import face_loss_reference as fr
import open_boundary_cases as ob
import plane_reference as pr
from conftest import rel_err

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
GRIDS = ("phih_grid", "phihe_grid", "phiheat")


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


def make_engine(pkg, tables, case, devices=0, lls=None, sources=None):
    """A context of the case's mesh and boundaries with the case's gas and sources (`sources`: 0-based subset)."""
    hp = pkg.hostphys
    n, _, periodic = fr.geometry(case)
    idx = np.arange(len(case.flux)) if sources is None else np.asarray(sources)
    ndens, xh, xhe, temp = (case.ndens, case.xh, case.xhe, case.temp) if hasattr(case, "ndens") else case.region
    mat = pkg.Material(ndens, xh.copy(), xhe.copy(), None if temp is None else temp.copy(), not case.heat, 1.0e4, 1.0, case.reccoef)
    if lls is not None:
        mat.use_LLS, mat.coldensh_LLS = True, float(lls)
    src = pkg.SourceProps(case.srcpos[idx], case.flux[idx], case.s_star)
    if case.pl is not None:
        src.NormFluxPL, src.pl_S_star = case.pl[idx], case.pl_s_star
        src.NormFluxQPL, src.qpl_S_star = case.qpl[idx], case.qpl_s_star
    e = pkg.HipEngine(n, devices)
    e.set_boundaries(periodic)
    e.set_tables(tables)
    e.set_step(mat, pkg.GridProps(n, case.dr, case.vol), pkg.Cosmology(ob.ZRED, hp.H0, hp.Omega0))
    e.set_sources(src)
    e.upload_state(mat)
    return e


def one_pass(e):
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources(1, 1)


def assert_maps_equal(e, ref, what=""):
    for face in range(6):
        if face not in ref:
            continue
        got = e.face_loss_map(face)
        assert got.shape == ref[face].shape
        bad = int(np.count_nonzero(got != ref[face]))
        print(what, "face", face, "cells", got.size, "non-zero", int(np.count_nonzero(ref[face])), "differ", bad,
              "worst rel", float(np.max(rel_err(got, ref[face]))) if got.size else 0.0)
        assert np.array_equal(got, ref[face]), (what, face, bad)


def assert_totals(e, ref, loss=None):
    """The six totals against math.fsum of the reference maps; their sum against photon_loss(1) where `loss` is given."""
    tot = e.face_loss()
    for face in range(6):
        want = math.fsum(ref[face].reshape(-1)) if face in ref else 0.0
        print("face", face, "total", tot[face], "reference", want, "rel", rel_err(tot[face], want) if want > 0 else 0.0)
        assert rel_err(tot[face], want) <= 1e-13 if want > 0 else tot[face] == 0.0
    if loss is not None:
        s = math.fsum(tot)
        print("sum of the totals", s, "photon_loss(1)", loss, "rel", rel_err(s, loss))
        assert loss > 0 and rel_err(s, loss) <= 1e-13
    return tot


def sed_tables(pkg, orc, gold):
    t = pkg.RadiationTables.load().add_sed_file(GOLD / "rad_tables_pl_qpl.npz")
    with np.load(pkg.evolve.DEFAULT_TABLES) as z:
        d = {k: z[k] for k in z.files}
    zz = gold("rad_tables_pl_qpl.npz")
    d.update({k: zz[k] for k in zz.files})
    return t, orc.Tables(d)


# -- N = 11, one round: every attribution tie ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["isothermal", "heating", "three_seds"])
def test_one_round_every_face_edge_and_corner(pkg, orc, otables, gold, tables, mode):
    """case_one_round: five sources at a corner, the opposite corner, an edge, a face and the interior of an open 11^3 box,
    all swept in round 1 -- corner and edge cells of the mesh and sources on them: every tie of the rule.  Isothermal (the
    rates launch then overwrites N_in(HI) of the surface cells behind the maps' kernel), with heating, with three SEDs."""
    t, ot = (tables, otables) if mode != "three_seds" else sed_tables(pkg, orc, gold)
    case = ob.case_one_round(pkg, heat=mode != "isothermal", seds=mode == "three_seds")
    ref, _ = fr.expected(pkg, orc, ot, case, "one_round_" + mode)
    e = make_engine(pkg, t, case)
    assert not e.face_loss_enabled
    e.enable_face_loss()
    assert e.face_loss_enabled
    one_pass(e)
    assert_maps_equal(e, ref, mode)
    assert_totals(e, ref, loss=e.get_loss()[0][0])
    assert all(np.count_nonzero(ref[f]) > ref[f].size // 2 for f in ref)
    e.close()


# -- N = 24, several rounds, batches -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def several(pkg, orc, otables):
    case = ob.case_several_rounds(pkg)
    return case, fr.expected(pkg, orc, otables, case, "several_rounds")[0]


@pytest.mark.parametrize("batch", [1, 2, None, "slabs"])
def test_several_rounds_same_bits_for_every_batch(pkg, tables, several, batch):
    """case_several_rounds: per-source boxes over three rounds, every source to its reach; set_batch(1), set_batch(2), the
    default, and the slab-wise pass with 3 slabs give the reference's bits."""
    case, ref = several
    e = make_engine(pkg, tables, case)
    e.enable_face_loss()
    if isinstance(batch, int):
        e.set_batch(batch)
    e.begin_step()
    e.set_rates_to_zero()
    if batch == "slabs":
        for s in range(e.pass_sources_begin(1, 1, 3)):
            e.pass_wait_slab(s)
        e.pass_sources_end()
    else:
        e.pass_sources(1, 1)
    assert_maps_equal(e, ref, f"batch {batch}")
    assert_totals(e, ref, loss=e.get_loss()[0][0])
    e.close()


# -- early stop ----------------------------------------------------------------------------------------------------------------
def test_early_stop_keeps_the_near_face_only(pkg, orc, otables, tables):
    """case_early_stop: opaque gas, a source three cells from the face x = 1 and one in the middle; both boxes stop after round
    1 (+-10 cells).  The near face holds its loss; the faces no box reaches hold exactly 0.0; the maps' total is below
    photon_loss(1), which also counts the boxes' inner surfaces."""
    case = ob.case_early_stop(pkg)
    ref, _ = fr.expected(pkg, orc, otables, case, "early_stop")
    e = make_engine(pkg, tables, case)
    e.enable_face_loss()
    one_pass(e)
    assert_maps_equal(e, ref, "early stop")
    tot = assert_totals(e, ref)
    loss = e.get_loss()[0][0]
    near = e.face_loss_map(0)
    assert np.count_nonzero(near) > 0 and tot[0] > 0
    # the first source's box is x 1..13, y and z 2..22; the second's 2..22 on every axis: no face but x = 1 is reached
    for face in range(1, 6):
        assert not e.face_loss_map(face).any() and tot[face] == 0.0
    print("maps' total", math.fsum(tot), "photon_loss(1)", loss)
    assert 0 < math.fsum(tot) < loss
    e.close()


# -- mixed boundaries ----------------------------------------------------------------------------------------------------------
def test_z_open_x_and_y_periodic(pkg, orc, otables, tables):
    """axis_boundary_cases.case_a: 24^3, z open, x and y periodic, sources at (1,1,1), (24,24,24), ... whose boxes wrap across
    x and y.  Only faces 4 and 5 have maps, the wrapped cells land at their mesh positions, downloading face 0 is an error,
    and the faces of the periodic axes at +-N/2 count in photon_loss(1) and in no map."""
    case = ab.case_a(pkg)
    ref, per_source = fr.expected(pkg, orc, otables, case, "axis_a")
    assert sorted(ref) == [4, 5]
    # the first source sits at x = 1: what it sends through z = 24 at x = 24 comes from the cell one step across the seam
    assert per_source[0][5][:, 23].all() and per_source[0][5][:, 11].all()
    e = make_engine(pkg, tables, case)
    e.enable_face_loss()
    one_pass(e)
    assert_maps_equal(e, ref, "z open")
    tot = assert_totals(e, ref)
    for face in range(4):
        with pytest.raises(pkg.C2RayHipError):
            e.face_loss_map(face)
        assert tot[face] == 0.0
    with pytest.raises(pkg.C2RayHipError):
        e.face_loss_map(6)
    loss = e.get_loss()[0][0]
    print("maps' total", math.fsum(tot), "photon_loss(1)", loss)
    assert 0 < math.fsum(tot) < loss
    e.close()


# -- planes ----------------------------------------------------------------------------------------------------------------------
PLANE_FLUX = 3.0e-41


@pytest.mark.parametrize("from_high", [0, 1])
def test_plane_terms_land_on_the_far_face_before_the_point_sources(pkg, orc, otables, tables, from_high):
    """A plane along z through a (6,5,7) mesh (z open, x and y periodic) plus a point source: the far face holds the per-line
    terms of tests/plane_reference.py with the point source's terms added after them, the near face the point source's alone;
    the far face's total minus the point source's part is c2r_get_plane_loss."""
    case = ab.AxisCase(pkg, (6, 5, 7), "z", (6, 5, 16), "mixed", np.array([[2, 4, 3]], dtype=np.int32), np.array([2.0e5]))
    ndens, xh, xhe, _ = case.region
    plane = pr.plane_pass(orc, otables, case.n, case.dr, case.vol, ndens, xh, xhe, 2, from_high, PLANE_FLUX)
    point, _ = fr.expected(pkg, orc, otables, case, "plane_mesh")
    far, near = 5 - from_high, 4 + from_high
    ref = {far: plane["terms"].reshape(5, 6) + point[far], near: point[near]}
    e = make_engine(pkg, tables, case)
    e.set_plane_sources([(2, from_high, PLANE_FLUX)])
    e.enable_face_loss()
    one_pass(e)
    assert_maps_equal(e, ref, f"plane from_high={from_high}")
    tot = assert_totals(e, ref)
    point_part = math.fsum(point[far].reshape(-1))
    plane_loss = e.plane_loss(1)
    print("far face", tot[far], "point source's part", point_part, "plane loss", plane_loss, "rel", rel_err(tot[far] - point_part, plane_loss))
    assert plane_loss > 0 and rel_err(tot[far] - point_part, plane_loss) <= 1e-13
    # the plane's own scalar and photon_loss(1) are what they are without the maps
    e2 = make_engine(pkg, tables, case)
    e2.set_plane_sources([(2, from_high, PLANE_FLUX)])
    one_pass(e2)
    assert e2.plane_loss(1) == plane_loss and np.array_equal(e2.get_loss()[0], e.get_loss()[0])
    e.close()
    e2.close()


# -- LLS -------------------------------------------------------------------------------------------------------------------------
def test_scalar_lls_fog(pkg, orc, otables, tables):
    """case_one_round, isothermal, use_LLS with the scalar coldensh_LLS: the fog is in the columns the kernel reads."""
    case = ob.case_one_round(pkg)
    lls = 2.0e16
    ref, _ = fr.expected(pkg, orc, otables, case, "one_round_isothermal", coldensh_lls=lls)
    plain, _ = fr.expected(pkg, orc, otables, case, "one_round_isothermal")
    assert all(np.all(ref[f] <= plain[f]) for f in ref) and any(np.any(ref[f] < plain[f]) for f in ref)
    e = make_engine(pkg, tables, case, lls=lls)
    e.enable_face_loss()
    one_pass(e)
    assert_maps_equal(e, ref, "LLS")
    assert_totals(e, ref, loss=e.get_loss()[0][0])
    e.close()


# -- lifetime and the off state --------------------------------------------------------------------------------------------------
def test_lifetime_follows_photon_loss(pkg, orc, otables, tables):
    """set_rates_to_zero clears the maps; two passes without it accumulate cell by cell, in source order; a change of boundary mode re-sizes and
    zeroes them; enabling is refused inside an open slab-wise pass; downloads are refused while the feature is off."""
    case = ob.case_one_round(pkg)
    ref, per_source = fr.expected(pkg, orc, otables, case, "one_round_isothermal")
    e = make_engine(pkg, tables, case)
    with pytest.raises(pkg.C2RayHipError):
        e.face_loss_map(0)
    with pytest.raises(pkg.C2RayHipError):
        e.face_loss()
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources_begin(1, 1, 2)
    with pytest.raises(pkg.C2RayHipError):
        e.enable_face_loss()
    e.pass_sources_end()
    assert not e.face_loss_enabled
    e.enable_face_loss()
    assert not any(e.face_loss_map(f).any() for f in range(6))
    one_pass(e)
    first = {f: e.face_loss_map(f) for f in range(6)}
    assert all(np.array_equal(first[f], ref[f]) for f in range(6))
    e.pass_sources(1, 1)                                    # no zeroing in between
    # map = map + term goes on in source order: ((first + s1) + s2) + ..., which is first + first only where one source
    # lights the cell (the one-source context below)
    second = {f: first[f].copy() for f in range(6)}
    for one in per_source:
        for f in range(6):
            second[f] = second[f] + one[f]
    assert all(np.array_equal(e.face_loss_map(f), second[f]) for f in range(6))
    e.do_source(3)                                          # c2r_do_source adds as well: the third source's terms once more
    assert all(np.array_equal(e.face_loss_map(f), second[f] + per_source[2][f]) for f in range(6))
    e.set_rates_to_zero()
    assert not any(e.face_loss_map(f).any() for f in range(6)) and not e.face_loss().any()
    one_pass(e)
    assert all(np.array_equal(e.face_loss_map(f), first[f]) for f in range(6))
    e.set_boundaries((True, True, False))                   # other faces now: new maps, zeroed
    assert e.face_loss_enabled and not e.face_loss_map(4).any() and not e.face_loss_map(5).any()
    with pytest.raises(pkg.C2RayHipError):
        e.face_loss_map(0)
    e.enable_face_loss(False)
    assert not e.face_loss_enabled
    e.close()
    # one source: two passes without a zeroing in between give first + first, added cell by cell
    e = make_engine(pkg, tables, case, sources=[0])
    e.enable_face_loss()
    one_pass(e)
    first = {f: e.face_loss_map(f) for f in range(6)}
    assert all(np.array_equal(first[f], per_source[0][f]) for f in range(6)) and any(first[f].any() for f in range(6))
    e.pass_sources(1, 1)
    assert all(np.array_equal(e.face_loss_map(f), first[f] + first[f]) for f in range(6))
    e.close()


def test_switched_off_nothing_changes(pkg, tables):
    """Rate grids, photon_loss / sum_nbox and the arena's statistics of a pass with the feature off equal, bit for bit, those of
    a context that never enabled it -- and so do those of a pass with it on (the maps' kernel only reads)."""
    case = ob.case_several_rounds(pkg)

    def run(switch):
        e = make_engine(pkg, tables, case)
        out = []
        for on in switch:
            if on is not None:
                e.enable_face_loss(on)
            one_pass(e)
            loss, nbox = e.get_loss()
            out.append((e.download_rates(), loss.copy(), nbox, e.arena_stats()))
        e.close()
        return out

    never = run([None, None])
    toggled = run([True, False])
    for (g0, l0, n0, a0), (g1, l1, n1, a1) in zip(never, toggled):
        for k in GRIDS:
            assert np.array_equal(g0[k], g1[k]), k
        assert np.array_equal(l0, l1) and n0 == n1 and a0 == a1


# -- several devices -----------------------------------------------------------------------------------------------------------
def test_two_replicas_are_added_in_device_order(pkg, orc, otables, tables):
    """c2r_create_multi([0, 0]) (the rehearsal mode: two replicas on one device): device 0 sweeps sources 1, 3, 5 and device 1
    sources 2, 4; a download is device 0's maps plus device 1's, in that association."""
    case = ob.case_one_round(pkg)
    dev0, _ = fr.expected(pkg, orc, otables, case, "one_round_isothermal", sources=[0, 2, 4])
    dev1, _ = fr.expected(pkg, orc, otables, case, "one_round_isothermal", sources=[1, 3])
    ref = {f: dev0[f] + dev1[f] for f in dev0}
    e = make_engine(pkg, tables, case, devices=[0, 0])
    e.comm_init_local()
    assert e.num_devices() == 2
    e.enable_face_loss()
    one_pass(e)
    assert_maps_equal(e, ref, "two replicas")
    assert_totals(e, ref)
    e.set_rates_to_zero()
    assert not any(e.face_loss_map(f).any() for f in range(6))
    e.close()
