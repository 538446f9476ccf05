"""Plane light curves (c2r_set_plane_curve) on the GPU, against the reference of tests/plane_curve_reference.py (the rule of
include/c2ray_hip.h in Python floats with the oracle's per-cell routines; tests/test_plane_curve_host.py holds the product's
host-compiled rule header to it on the CPU).  python -m pytest tests -m gpu.

The bar is that of tests/test_gpu_plane_sources.py, whose helpers this file uses: every grid, the exit columns, the exit
flux and the escape map of the far face bit for bit; c2r_get_plane_loss, one sum whose order differs from math.fsum's, to
1e-13 relative.  The meshes are (12,10,9) and (9,7,5).
"""
from pathlib import Path

import numpy as np
import pytest

import curve_reference as cr
import mix_reference as mx
import plane_curve_reference as pcr
import plane_reference as pr
import test_gpu_plane_mix as tpm
import test_gpu_plane_sources as tps
from test_gpu_oblique_planes import make_gas
from test_gpu_plane_sources import FLUX, GRIDS, PAIRS, assert_grids_equal, assert_plane_equals_reference, make_engine, start

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
OPEN = (False, False, False)
TILT = (0.35, -0.6)
ALL = GRIDS + ("phiheat", "photon_loss")


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


@pytest.fixture(scope="module")
def gas_1(pkg):
    return make_gas(pkg, (12, 10, 9), 11)


def gap_curve(gas, axis):
    """A dark gap with light beyond it: {3, {1.2, 2.6, 4.1} * dr[axis], {1, 0.3, 0, 0.5}} -- layers 0 | 1, 2 | 3 | 4 ..."""
    d = gas.dr[axis]
    return ([1.2 * d, 2.6 * d, 4.1 * d], [1.0, 0.3, 0.0, 0.5])


def make_map(gas, axis, seed, seds=1):
    """A random map around FLUX with a block of dark cells and one dark line of the face: (3, face)."""
    a, b = pr.face_axes(axis)
    fa, fb = gas.mesh[a], gas.mesh[b]
    rng = np.random.default_rng(seed)
    m = np.zeros((3, fb, fa))
    m[:seds] = FLUX * rng.uniform(0.3, 2.0, (seds, fb, fa))
    m[:, 2:4, 1:4] = 0.0
    m[:, fb - 2, :] = 0.0
    return m.reshape(3, -1)


def reference(orc, otables, gas, axis, from_high, curve, fmap=None, flux=FLUX, tilt=None, periodic=OPEN, entry=None):
    return pcr.curve_pass(orc, otables, gas.mesh, gas.dr, gas.vol, gas.ndens, gas.xh_av, gas.xhe_av, axis, from_high,
                          normflux=None if fmap is not None else flux, flux_map=fmap, curve=curve, tilt=tilt, periodic=periodic, heat=gas.heat,
                          entry=entry)


def run_plane(pkg, tables, gas, periodic, axis, from_high, curve, fmap=None, tilt=None, entry=None, flux=FLUX, maps=True, timing=False,
              set_curve=True):
    """One pass of one plane on a fresh engine, the curve set last: (engine, rates)."""
    e = make_engine(pkg, tables, gas, periodic)
    if maps:
        e.enable_face_loss()
    if timing:
        e.enable_timing()
    e.set_plane_sources([dict(axis=axis, from_high=from_high, normflux=flux)])
    if set_curve:
        e.set_plane_curve(1, curve)
    if tilt is not None:
        e.set_plane_tilt(1, tilt)
    if fmap is not None:
        e.set_plane_flux_map(1, fmap)
    if entry is not None:
        e.set_plane_entry_columns(1, entry)
    start(e, gas)
    e.pass_sources(1, 1)
    return e, e.download_rates()


def far_face(axis, from_high):
    return 2 * axis + (1 - from_high)


def assert_equals_reference(e, got, ref, axis, from_high, heat=False, mapped=False, maps=True):
    assert_plane_equals_reference(e, got, ref, heat=heat)
    if mapped:
        assert np.array_equal(e.plane_exit_flux(1), ref["exit_flux"])
    if maps:
        have = e.face_loss_map(far_face(axis, from_high))
        assert np.array_equal(have, ref["terms"].reshape(have.shape))


def state(e, axis, from_high):
    return e.download_rates(), e.plane_exit_columns(1), e.plane_loss(1), e.face_loss_map(far_face(axis, from_high))


def assert_same_state(got, want):
    assert_grids_equal(got[0], want[0], ALL)
    assert np.array_equal(got[1], want[1]) and got[2] == want[2] and np.array_equal(got[3], want[3])


# -- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis,from_high", PAIRS)
def test_1_every_face_with_a_dark_gap(pkg, orc, otables, tables, gas_1, axis, from_high):
    """(12,10,9), all axes open, uniform flux, a plane through each of the six faces with the dark-gap curve: the cells of the
    unlit layer hold exactly 0, the layers behind the gap are lit again."""
    curve = gap_curve(gas_1, axis)
    ref = reference(orc, otables, gas_1, axis, from_high, curve)
    na = gas_1.mesh[axis]
    assert list(ref["factors"]) == ([1.0, 0.3, 0.3, 0.0] + [0.5] * (na - 4))
    e, got = run_plane(pkg, tables, gas_1, False, axis, from_high, curve)
    assert_equals_reference(e, got, ref, axis, from_high)
    cells = pr.column_cells(gas_1.mesh, axis, from_high)                 # [face cell, step]
    for k in GRIDS + ("phiheat",):
        assert not got[k].reshape(-1, gas_1.n)[:, cells[:, 3]].any(), k
    lit = np.delete(cells, 3, axis=1)
    assert np.all(got["phih_grid"][lit] > 0) and got["photon_loss"][0] > 0
    assert e.plane_curve(1) == (curve[0], curve[1], 0, 0.0)
    e.close()


# -- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis,from_high", [(0, 1), (2, 0)])
def test_2_off_and_all_ones(pkg, tables, gas_1, axis, from_high):
    """The None curve, the {0, .., {1.0}} record and an all-ones two-step curve give the uncurved plane's bits in the rates, the exit
    columns, the loss and the escape map; the first two through the uncurved launches."""
    e, _ = run_plane(pkg, tables, gas_1, False, axis, from_high, None, timing=True, set_curve=False)
    want, launches = state(e, axis, from_high), e.timing().rates_launches
    e.close()
    assert want[2] > 0 and np.all(want[3] > 0) and launches > 0
    d = gas_1.dr[axis]
    for curve, curved in ((None, False), (([], [1.0]), False), (([1.5 * d, 4.0 * d], [1.0, 1.0, 1.0], 2, 0.5 * d), True)):
        e, _ = run_plane(pkg, tables, gas_1, False, axis, from_high, curve, timing=True)
        assert_same_state(state(e, axis, from_high), want)
        assert e.timing().rates_launches == launches
        assert (e.plane_curve(1) != ([], [1.0], 0, 0.0)) == curved
        e.close()


# -- 3 ---------------------------------------------------------------------------------------------------------------------
def test_3_a_depth_horizon_before_the_last_layer(pkg, orc, otables, tables, gas_1):
    """{1, {D}, {1, 0}} with D = 5 layers of 9: the loss is exactly 0.0, the escape map all 0.0, the exit columns those of the
    uncurved plane; the layers within D have the uncurved bits and the layers beyond exactly zero rates."""
    axis, from_high = 2, 1
    e, plain = run_plane(pkg, tables, gas_1, False, axis, from_high, None, set_curve=False)
    plain_exit = e.plane_exit_columns(1)
    e.close()
    curve = ([5.0 * gas_1.dr[axis]], [1.0, 0.0])
    ref = reference(orc, otables, gas_1, axis, from_high, curve)
    assert list(ref["factors"]) == [1.0] * 5 + [0.0] * 4
    e, got = run_plane(pkg, tables, gas_1, False, axis, from_high, curve)
    assert_equals_reference(e, got, ref, axis, from_high)
    assert e.plane_loss(1) == 0.0 and got["photon_loss"][0] == 0.0 and not e.face_loss_map(far_face(axis, from_high)).any()
    assert np.array_equal(e.plane_exit_columns(1), plain_exit)
    cells = pr.column_cells(gas_1.mesh, axis, from_high)
    near, far = cells[:, :5].reshape(-1), cells[:, 5:].reshape(-1)
    for k in GRIDS:
        g, p = got[k].reshape(-1, gas_1.n), plain[k].reshape(-1, gas_1.n)
        assert np.array_equal(g[:, near], p[:, near]) and not g[:, far].any() and p[:, far].any(), k
    e.close()


# -- 4 ---------------------------------------------------------------------------------------------------------------------
def test_4_tilted_heating_three_seds_wrap_and_side(pkg, orc, gold, tables):
    """(9,7,5) along z, tilted, heating, a map per SED, a curve with factors that are no powers of two, layer0 and depth0: x wraps
    and y is open, then the other way round on the same context."""
    gas = make_gas(pkg, (9, 7, 5), 33, heat=True)
    t = pkg.RadiationTables.load().add_sed_file(GOLD / "rad_tables_pl_qpl.npz")
    with np.load(pkg.evolve.DEFAULT_TABLES) as z:
        d = {k: z[k] for k in z.files}
    zz = gold("rad_tables_pl_qpl.npz")
    d.update({k: zz[k] for k in zz.files})
    ot = orc.Tables(d)
    fmap = make_map(gas, 2, 3, seds=3)
    fmap[1] *= 0.5
    fmap[2] *= 0.25
    fmap[2, 40] = 0.0
    path = pcr.plane_path(gas.dr, 2, TILT)
    curve = ([3.2 * path, 4.1 * path, 5.3 * path], [0.7, 1.3, 0.0, 0.45], 2, 0.5 * path)      # centres 3, 4, 5, 6, 7 paths deep
    first, second = (True, False, False), (False, True, False)
    ref1 = reference(orc, ot, gas, 2, 1, curve, fmap=fmap, tilt=TILT, periodic=first)
    assert list(ref1["factors"]) == [0.7, 1.3, 0.0, 0.45, 0.45]
    e, got = run_plane(pkg, t, gas, first, 2, 1, curve, fmap=fmap, tilt=TILT)
    assert_equals_reference(e, got, ref1, 2, 1, heat=True, mapped=True)
    assert np.any(got["phiheat"] > 0)
    e.set_boundaries(second)
    assert e.plane_curve(1) == curve and e.plane_flux_map_set(1) and e.plane_tilt(1) == TILT
    start(e, gas)
    e.pass_sources(1, 1)
    ref2 = reference(orc, ot, gas, 2, 1, curve, fmap=fmap, tilt=TILT, periodic=second)
    assert_equals_reference(e, e.download_rates(), ref2, 2, 1, heat=True, mapped=True, maps=False)
    assert not np.array_equal(ref1["exit_flux"], ref2["exit_flux"])
    e.close()


# -- 5 ---------------------------------------------------------------------------------------------------------------------
def test_5_two_slabs_equal_one_mesh(pkg, tables):
    """(9,7,5) along z against (9,7,3) into (9,7,2) with layer0 = 3, tilted with a map, x periodic: the exit columns and the
    unscaled exit flux are handed on; the rates of both parts, the final exit columns, the exit flux and the loss bit for bit."""
    gas = make_gas(pkg, (9, 7, 5), 55)
    fmap = make_map(gas, 2, 5)
    per = (True, False, False)
    path = pcr.plane_path(gas.dr, 2, TILT)
    depths, factors, depth0 = [1.5 * path, 3.7 * path, 4.5 * path], [1.0, 0.6, 0.0, 1.7], 0.25 * path
    assert [pcr.layer_factor((depths, factors, 0, depth0), m, path) for m in range(5)] == [1.0, 0.6, 0.6, 0.0, 1.7]
    runs, entry, flux = [], None, fmap
    for g, layer0 in ((gas, 0), (tps.half(gas, pkg, 0, 3), 0), (tps.half(gas, pkg, 3, 5), 3)):
        e, rates = run_plane(pkg, tables, g, per, 2, 0, (depths, factors, layer0, depth0), fmap=flux if layer0 else fmap, tilt=TILT,
                             entry=entry if layer0 else None)
        runs.append((rates, e.plane_exit_columns(1), e.plane_loss(1), e.plane_exit_flux(1), e.face_loss_map(5)))
        if g.mesh[2] == 3:
            entry, flux = runs[-1][1], runs[-1][3]
        e.close()
    (big, big_exit, big_loss, big_flux, big_map), (lower, _, _, lower_flux, _), (upper, upper_exit, upper_loss, upper_flux, upper_map) = runs
    for k in GRIDS:
        b = big[k].reshape(-1, 5, 7, 9)
        assert np.array_equal(b[:, :3].reshape(-1), lower[k]) and np.array_equal(b[:, 3:].reshape(-1), upper[k]), k
        assert not b[:, 3].any() and b[:, 4].any(), k
    assert np.array_equal(upper_exit, big_exit) and np.array_equal(upper_flux, big_flux) and np.array_equal(upper_map, big_map)
    assert not np.array_equal(lower_flux, fmap.reshape(-1)) and not np.array_equal(lower_flux, upper_flux)
    assert upper_loss == big_loss == upper["photon_loss"][0] and big_loss > 0


# -- 6 ---------------------------------------------------------------------------------------------------------------------
def test_6_curved_and_uncurved_planes_with_a_curved_point_source(pkg, orc, otables, tables):
    """(12,10,9), all axes open: a curved plane, an uncurved plane with a map through the same face and a point source that carries
    a source curve (no step, factor 0.5: the source with half its flux everywhere), in one c2r_pass_sources -- the fold in plane
    order, then the point source on top through the oracle; then c2r_do_source(NumSrc + 1): the curved plane alone."""
    case = mx.make_case(pkg, "xyz", [(6, 5, 5)], [2.0e7], mesh=((12, 10, 9), (24, 24, 24)), seed=616)
    ndens, xh, xhe, _ = case.region
    curve = ([1.5 * case.dr[2], 4.2 * case.dr[2]], [0.8, 0.0, 1.9], 1, 0.0)
    planes = [dict(axis=2, from_high=1, normflux=FLUX), dict(axis=2, from_high=1, normflux=0.6 * FLUX, fmap=mx.make_map(case, 2, 61))]
    refs = {1: pcr.curve_pass(orc, otables, case.n, case.dr, case.vol, ndens, xh, xhe, 2, 1, normflux=FLUX, curve=curve),
            2: mx.plane_alone(orc, otables, case, planes[1])}
    assert list(refs[1]["factors"]) == [0.8, 0.0, 0.0] + [1.9] * 6                # centres 1.5, 2.5, .. cells deep
    want, nbox, _, _ = mx.point_sources_on_top(pkg, orc, otables, cr.scaled_case(case, 1, 0.5), mx.fold_planes(case, refs, [1, 2]), [1])
    assert all(mx.same_cells(case, [1], nbox))
    e = tpm.make_engine(pkg, tables, case, planes, maps=True)
    e.set_plane_curve(1, curve)
    e.set_source_curves([([], [0.5])])
    got = tpm.run_pass(e)
    assert_grids_equal(got, want, GRIDS)
    assert got["sum_nbox"] == 1
    terms = refs[1]["terms"] + refs[2]["terms"]
    for p in (1, 2):
        assert np.array_equal(e.plane_exit_columns(p), refs[p]["exit"])
        assert tps.rel_err(e.plane_loss(p), refs[p]["loss"]) <= 1e-13 and refs[p]["loss"] > 0
    assert np.array_equal(e.plane_exit_flux(2), refs[2]["exit_flux"])
    e.begin_step()
    e.set_rates_to_zero()
    e.do_source(2)                                       # NumSrc + 1: plane 1 alone
    alone = e.download_rates()
    assert_grids_equal(alone, refs[1], GRIDS)
    have = e.face_loss_map(far_face(2, 1))
    assert np.array_equal(have, refs[1]["terms"].reshape(have.shape)) and terms.any()
    e.close()


# -- 7 ---------------------------------------------------------------------------------------------------------------------
def test_7_refusals_and_lifetime(pkg, orc, otables, tables):
    """Every refusal returns an error with a text and changes nothing -- the pass that follows gives the bits of the curve set
    before; set_plane_sources drops the curve; plane_curve returns what was set."""
    E = pkg.C2RayHipError
    gas = make_gas(pkg, (9, 7, 5), 77)
    d = gas.dr[0]
    curve = ([1.3 * d, 3.4 * d], [1.0, 0.0, 0.6], 1, 0.25 * d)
    ref = reference(orc, otables, gas, 0, 0, curve)
    assert list(ref["factors"]) == [0.0, 0.0] + [0.6] * 7                        # centres 1.75, 2.75, .. cells deep
    e = make_engine(pkg, tables, gas, False)
    e.enable_face_loss()
    with pytest.raises(E, match="c2r_set_plane_curve.*plane 1 not in"):
        e.set_plane_curve(1, curve)                       # no planes yet
    e.set_plane_sources([(0, 0, FLUX)])
    assert e.plane_curve(1) == ([], [1.0], 0, 0.0)
    e.set_plane_curve(1, curve)
    assert e.plane_curve(1) == curve
    nan, inf = float("nan"), float("inf")
    bad = [(0, curve, "plane 0 not in"), (2, curve, "plane 2 not in"),
           (1, ([1.0 * d], [1.0, 1.0], -1, 0.0), "layer0"),
           (1, ([1.0 * d], [1.0, 1.0], 0, -1.0), "depth0"), (1, ([1.0 * d], [1.0, 1.0], 0, nan), "depth0"), (1, ([1.0 * d], [1.0, 1.0], 0, inf), "depth0"),
           (1, ([-1.0], [1.0, 1.0]), r"depth\[0\]"), (1, ([d, inf], [1.0, 1.0, 1.0]), r"depth\[1\]"), (1, ([d, nan], [1.0, 1.0, 1.0]), r"depth\[1\]"),
           (1, ([2.0 * d, 2.0 * d], [1.0, 1.0, 1.0]), "not above"), (1, ([2.0 * d, d], [1.0, 1.0, 1.0]), "not above"),
           (1, ([d], [1.0, -0.5]), r"factor\[1\]"), (1, ([d], [nan, 1.0]), r"factor\[0\]"), (1, ([d], [1.0, inf]), r"factor\[1\]"),
           (1, ([], [0.0]), "zeroed record"),
           (1, ([d * (k + 1) for k in range(9)], [1.0] * 10), "nstep = 9")]
    for p, c, text in bad:
        with pytest.raises(E, match="c2r_set_plane_curve.*" + text):
            e.set_plane_curve(p, c)
    rec = pkg._lib.PlaneCurve()
    rec.nstep, rec.factor[0] = -1, 1.0
    assert e.lib.c2r_set_plane_curve(e.h, 1, rec) != 0 and b"nstep = -1" in e.lib.c2r_last_error(e.h)
    assert e.lib.c2r_get_plane_curve(e.h, 3, rec) != 0 and b"c2r_get_plane_curve" in e.lib.c2r_last_error(e.h)
    start(e, gas)
    e.pass_sources_begin(1, 1, 2)
    with pytest.raises(E, match="c2r_set_plane_curve.*pass"):
        e.set_plane_curve(1, None)
    e.pass_sources_end()
    assert e.plane_curve(1) == curve                       # nothing changed: the pass gives the curve's bits
    e.set_plane_tilt(1, None)                              # these keep the curve
    e.set_plane_flux_map(1, None)
    e.set_plane_entry_columns(1, None)
    e.set_boundaries(OPEN)
    assert e.plane_curve(1) == curve
    start(e, gas)
    e.pass_sources(1, 1)
    assert_equals_reference(e, e.download_rates(), ref, 0, 0)
    e.set_plane_curve(1, ([0.0], [0.0, 0.0]))             # a plane that has gone dark
    start(e, gas)
    e.pass_sources(1, 1)
    dark = e.download_rates()
    assert not dark["phih_grid"].any() and not dark["phihe_grid"].any() and dark["photon_loss"][0] == 0.0 and e.plane_loss(1) == 0.0
    e.set_plane_curve(1, curve)
    e.set_plane_sources([(0, 0, FLUX)])                   # a new list: no curve
    assert e.plane_curve(1) == ([], [1.0], 0, 0.0)
    start(e, gas)
    e.pass_sources(1, 1)
    plain = pr.plane_pass(orc, otables, gas.mesh, gas.dr, gas.vol, gas.ndens, gas.xh_av, gas.xhe_av, 0, 0, FLUX)
    assert_plane_equals_reference(e, e.download_rates(), plain)
    e.close()
