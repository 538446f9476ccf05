"""Plane flux maps (c2r_set_plane_flux_map) on the GPU, against the reference of tests/flux_reference.py (the rule of
include/c2ray_hip.h in Python floats with the oracle's per-cell routines; tests/test_flux_reference_host.py holds the
product's host-compiled functions to it on the CPU).  python -m pytest tests -m gpu.

The bar is that of tests/test_gpu_plane_sources.py, whose helpers this file uses: every grid, the exit columns and the exit
flux bit for bit; the loss, one sum whose order differs from math.fsum's, to 1e-13 relative.
"""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import flux_reference as fr
import oblique_reference as obr
import plane_reference as pr
import test_gpu_plane_sources as tps
from test_gpu_oblique_planes import make_gas
from test_gpu_plane_sources import DT, FLUX, GRIDS, ITER_STATE, PAIRS, SRC3, assert_grids_equal, assert_plane_equals_reference, make_engine, start

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
OPEN = (False, False, False)
Z_OPEN = (True, True, False)
TILT = (0.35, -0.6)


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


def make_map(gas, axis, seed, seds=1):
    """A random map around FLUX with a block of dark cells and one dark line of the face: (3, face)."""
    a, b = pr.face_axes(axis)
    fa, fb = gas.mesh[a], gas.mesh[b]
    rng = np.random.default_rng(seed)
    m = np.zeros((3, fb, fa))
    m[:seds] = FLUX * rng.uniform(0.3, 2.0, (seds, fb, fa))
    m[:, 2:5, 1:4] = 0.0
    m[:, fb - 2, :] = 0.0
    return m.reshape(3, -1)


def reference(orc, otables, gas, axis, from_high, fmap, tilt=None, periodic=OPEN, **kw):
    return fr.flux_pass(orc, otables, gas.mesh, gas.dr, gas.vol, gas.ndens, gas.xh_av, gas.xhe_av, axis, from_high, fmap, tilt=tilt,
                        periodic=periodic, heat=gas.heat, **kw)


def run_plane(pkg, tables, gas, periodic, axis, from_high, fmap, tilt=None, entry=None, flux=FLUX, maps=False, **kw):
    """One pass of one plane with a flux map on a fresh engine: (engine, rates)."""
    e = make_engine(pkg, tables, gas, periodic, **kw)
    if maps:
        e.enable_face_loss()
    e.set_plane_sources([dict(axis=axis, from_high=from_high, normflux=flux)])
    if tilt is not None:
        e.set_plane_tilt(1, tilt)
    if fmap is not None:
        e.set_plane_flux_map(1, fmap)
    if entry is not None:
        e.set_plane_entry_columns(1, entry)
    start(e, gas)
    e.pass_sources(1, 1)
    return e, e.download_rates()


def assert_equals_reference(e, got, ref, heat=False):
    assert_plane_equals_reference(e, got, ref, heat=heat)
    assert np.array_equal(e.plane_exit_flux(1), ref["exit_flux"])


# -- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gas_1(pkg):
    return make_gas(pkg, (12, 10, 9), 11)


@pytest.mark.parametrize("axis,from_high", PAIRS)
def test_1_every_face_at_normal_incidence(pkg, orc, otables, tables, gas_1, axis, from_high):
    """(12,10,9), all axes open, a plane through each of the six faces, a random map with a block of dark cells and a dark line."""
    fmap = make_map(gas_1, axis, 100 + axis)
    ref = reference(orc, otables, gas_1, axis, from_high, fmap)
    e, got = run_plane(pkg, tables, gas_1, False, axis, from_high, fmap)
    assert e.plane_flux_map_set(1)
    assert_equals_reference(e, got, ref)
    assert np.array_equal(e.plane_exit_flux(1), fmap.reshape(-1))
    lit = fmap[0] > 0
    cells = pr.column_cells(gas_1.mesh, axis, from_high)                 # [face cell, step]
    assert np.all(got["phih_grid"][cells[lit]] > 0) and not got["phih_grid"][cells[~lit]].any() and (~lit).any()
    e.close()


# -- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis,from_high", [(0, 1), (2, 0)])
def test_2_a_uniform_map_is_the_uniform_plane(pkg, tables, gas_1, axis, from_high):
    """map == normflux everywhere: every grid, the exit columns, c2r_get_plane_loss and the far face's escape map have the
    uniform plane's bits; set_plane_flux_map(1, None) on the same context gives them again."""
    def state(e):
        r = e.download_rates()
        return r, e.plane_exit_columns(1), e.plane_loss(1), e.face_loss_map(2 * axis + (1 - from_high))
    e, _ = run_plane(pkg, tables, gas_1, False, axis, from_high, None, maps=True)
    want = state(e)
    e.close()
    assert want[2] > 0 and np.all(want[3] > 0)
    fmap = np.zeros((3, pr.face_cells(gas_1.mesh, axis)))
    fmap[0] = FLUX
    e, _ = run_plane(pkg, tables, gas_1, False, axis, from_high, fmap, maps=True)
    for back in (False, True):
        if back:
            e.set_plane_flux_map(1, None)
            assert not e.plane_flux_map_set(1)
            start(e, gas_1)
            e.pass_sources(1, 1)
        got = state(e)
        assert_grids_equal(got[0], want[0], GRIDS + ("phiheat", "photon_loss"))
        assert np.array_equal(got[1], want[1]) and got[2] == want[2] and np.array_equal(got[3], want[3])
    e.close()


# -- 3 ---------------------------------------------------------------------------------------------------------------------
def test_3_tilted_heating_three_seds_wrap_and_side(pkg, orc, gold, tables):
    """(9,7,5) along z, tilt (0.35, -0.6), heating, a map per SED: x wraps and y takes zero flux from outside, then the other way
    round on the same context."""
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
    first, second = (True, False, False), (False, True, False)
    e, got = run_plane(pkg, t, gas, first, 2, 1, fmap, tilt=TILT)
    ref1 = reference(orc, ot, gas, 2, 1, fmap, tilt=TILT, periodic=first)
    assert_equals_reference(e, got, ref1, heat=True)
    assert np.any(got["phiheat"] > 0)
    e.set_boundaries(second)
    assert e.plane_flux_map_set(1) and e.plane_tilt(1) == TILT
    start(e, gas)
    e.pass_sources(1, 1)
    ref2 = reference(orc, ot, gas, 2, 1, fmap, tilt=TILT, periodic=second)
    assert_equals_reference(e, e.download_rates(), ref2, heat=True)
    assert not np.array_equal(ref1["exit_flux"], ref2["exit_flux"])
    e.close()


# -- 4 ---------------------------------------------------------------------------------------------------------------------
def test_4_layers_wider_than_one_block(pkg, orc, otables, tables):
    """(20,20,6) along z, tilted: a layer is 400 lanes in five blocks of 64 x 4, the flux's neighbours sit in other blocks and
    waves."""
    gas = make_gas(pkg, (20, 20, 6), 22)
    fmap = make_map(gas, 2, 4)
    ref = reference(orc, otables, gas, 2, 0, fmap, tilt=TILT, periodic=Z_OPEN)
    e, got = run_plane(pkg, tables, gas, Z_OPEN, 2, 0, fmap, tilt=TILT)
    assert_equals_reference(e, got, ref)
    e.close()


# -- 5 ---------------------------------------------------------------------------------------------------------------------
def test_5_a_spot_shifts_one_cell_per_layer(pkg, orc, otables, tables):
    """a_f == 1.0 and a_g == 0 (test_4_a_f_exactly_one's set-up): a one-cell spot moves one cell along x per layer and wraps.  The
    rate grids are exactly 0.0 outside the five cells it visits and the reference's inside."""
    gas = make_gas(pkg, (9, 7, 5), 44, factors=(1.0, 1.25, 1.0))
    a_f, a_g, s, _, _, _ = obr.geometry((1.0, 0.0), gas.dr, 2)
    assert a_f == 1.0 and a_g == 0.0 and s == (0.0, 0.0, 1.0, 0.0)
    u0, v0 = 6, 3
    fmap = np.zeros((3, 63))
    fmap[0, u0 + 9 * v0] = FLUX
    ref = reference(orc, otables, gas, 2, 0, fmap, tilt=(1.0, 0.0), periodic=Z_OPEN)
    e, got = run_plane(pkg, tables, gas, Z_OPEN, 2, 0, fmap, tilt=(1.0, 0.0))
    assert_equals_reference(e, got, ref)
    visited = np.zeros(gas.n, dtype=bool)
    for m in range(5):
        visited[(u0 + m + 1) % 9 + 9 * (v0 + 7 * m)] = True
    for k in GRIDS:
        g = got[k].reshape(-1, gas.n)
        assert not g[:, ~visited].any() and np.all(g[:, visited] > 0), k
    want = np.zeros((3, 63))
    want[0, (u0 + 5) % 9 + 9 * v0] = FLUX
    assert np.array_equal(e.plane_exit_flux(1), want.reshape(-1))
    e.close()


# -- 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic", [Z_OPEN, OPEN])
def test_6_two_slabs_equal_one_mesh(pkg, tables, periodic):
    """(10,8,6) along z against two engines of (10,8,3) that hold its halves, the second fed with the first's exit columns and
    exit flux, the same tilt on all three: rates of both halves, final exit columns, exit flux and downstream loss bit for bit."""
    gas = make_gas(pkg, (10, 8, 6), 66)
    fmap = make_map(gas, 2, 6)
    runs, entry, flux = [], None, fmap
    for g in (gas, tps.half(gas, pkg, 0, 3), tps.half(gas, pkg, 3, 6)):
        e, rates = run_plane(pkg, tables, g, periodic, 2, 0, flux if g.mesh[2] == 3 else fmap, tilt=TILT, entry=entry if g.mesh[2] == 3 else None)
        runs.append((rates, e.plane_exit_columns(1), e.plane_loss(1), e.plane_exit_flux(1)))
        if g.mesh[2] == 3 and entry is None:
            entry, flux = runs[-1][1], runs[-1][3]
        e.close()
    (big, big_exit, big_loss, big_flux), (lower, _, _, lower_flux), (upper, upper_exit, upper_loss, upper_flux) = runs
    for k in GRIDS:
        b = big[k].reshape(-1, 6, 8, 10)
        assert np.array_equal(b[:, :3].reshape(-1), lower[k]), k
        assert np.array_equal(b[:, 3:].reshape(-1), upper[k]), k
    assert np.array_equal(upper_exit, big_exit) and np.array_equal(upper_flux, big_flux)
    assert not np.array_equal(lower_flux, fmap.reshape(-1)) and not np.array_equal(lower_flux, upper_flux)
    assert upper_loss == big_loss == upper["photon_loss"][0] and big_loss > 0


# -- 7 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("from_high", [0, 1])
def test_7_escape_map_of_the_far_face(pkg, orc, otables, tables, gas_1, from_high):
    """c2r_enable_face_loss, all axes open, a tilted plane along y with a map: the far face's map is the reference's per-line
    terms bit for bit, every other map stays zero.  The map is dark for x < 5 and the beam leans towards +x through an open
    side face, so those lines stay dark to the last layer: their terms are exactly 0.0."""
    fmap = make_map(gas_1, 1, 7)
    fmap.reshape(3, gas_1.mesh[2], gas_1.mesh[0])[:, :, :5] = 0.0
    ref = reference(orc, otables, gas_1, 1, from_high, fmap, tilt=TILT)
    e, got = run_plane(pkg, tables, gas_1, False, 1, from_high, fmap, tilt=TILT, maps=True)
    far = 2 * 1 + (1 - from_high)
    assert np.array_equal(e.face_loss_map(far), ref["terms"].reshape(gas_1.mesh[2], gas_1.mesh[0]))
    dark = ref["terms"].reshape(gas_1.mesh[2], gas_1.mesh[0])[:, :5]
    assert not dark.any() and np.count_nonzero(ref["terms"]) == ref["terms"].size - dark.size
    for face in range(6):
        if face != far:
            assert not e.face_loss_map(face).any(), face
    assert_equals_reference(e, got, ref)
    e.close()


# -- 8 ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gas_8(pkg):
    return make_gas(pkg, (16, 16, 16), 99)


@pytest.fixture(scope="module")
def map_8(gas_8):
    return make_map(gas_8, 2, 8)


def engine_8(pkg, tables, gas, fmap, sources=SRC3):
    e = make_engine(pkg, tables, gas, Z_OPEN, sources)
    e.set_plane_sources([(2, 1, FLUX)])
    e.set_plane_flux_map(1, fmap)                       # the map first, the tilt second: the tilt call makes the flux buffers
    e.set_plane_tilt(1, TILT)
    return e


@pytest.fixture(scope="module")
def run_8(pkg, tables, gas_8, map_8):
    """The tilted plane with its map and three point sources in one c2r_pass_sources, then the global pass."""
    e = engine_8(pkg, tables, gas_8, map_8)
    start(e, gas_8)
    e.pass_sources(1, 1)
    rates = e.download_rates()
    conv = e.global_pass(DT)
    out = SimpleNamespace(rates=rates, conv=conv, state=e.download_iter_state(), plane_loss=e.plane_loss(1), exit=e.plane_exit_columns(1),
                          exit_flux=e.plane_exit_flux(1))
    e.close()
    return out


def test_8_do_source_runs_the_plane_alone(pkg, orc, otables, tables, gas_8, map_8, run_8):
    """c2r_do_source(NumSrc + 1): the plane only, equal to the reference; its loss is the plane's share of the full pass."""
    ref = reference(orc, otables, gas_8, 2, 1, map_8, tilt=TILT, periodic=Z_OPEN)
    e = engine_8(pkg, tables, gas_8, map_8)
    start(e, gas_8)
    e.do_source(4)
    assert_equals_reference(e, e.download_rates(), ref)
    assert e.plane_loss(1) == run_8.plane_loss and np.array_equal(run_8.exit, ref["exit"]) and np.array_equal(run_8.exit_flux, ref["exit_flux"])
    assert run_8.rates["sum_nbox"] > 0 and 0 < run_8.plane_loss < run_8.rates["photon_loss"][0]
    e.close()


def test_8_slab_wise_allreduce_and_fused_routes(pkg, tables, gas_8, map_8, run_8):
    """The same pass through c2r_pass_sources_begin / wait / end, c2r_pass_allreduce_chemistry and c2r_iteration."""
    e = engine_8(pkg, tables, gas_8, map_8)
    start(e, gas_8)
    nslab = e.pass_sources_begin(1, 1, 2)
    assert nslab == 2
    for s in range(nslab):
        e.pass_wait_slab(s)
    e.pass_sources_end()
    tps.same_pass(e.download_rates(), run_8.rates)
    assert e.global_pass(DT) == run_8.conv
    assert_grids_equal(e.download_iter_state(), run_8.state, ITER_STATE)
    start(e, gas_8)
    assert e.pass_allreduce_chemistry(DT, 1, 1, 2) == run_8.conv
    tps.same_pass(e.download_rates(), run_8.rates)
    assert_grids_equal(e.download_iter_state(), run_8.state, ITER_STATE)
    start(e, gas_8)
    rep = e.iteration(DT)
    assert rep["conv_flag"] == run_8.conv and rep["sum_nbox"] == run_8.rates["sum_nbox"]
    assert np.array_equal(rep["photon_loss"], run_8.rates["photon_loss"])
    tps.same_pass(e.download_rates(), run_8.rates)
    assert_grids_equal(e.download_iter_state(), run_8.state, ITER_STATE)
    assert np.array_equal(e.plane_exit_columns(1), run_8.exit) and np.array_equal(e.plane_exit_flux(1), run_8.exit_flux)
    e.close()


def test_8_evolve3d_with_a_mapped_plane_only(pkg, orc, tables):
    """NumSrc = 0 and one tilted plane with a map: c2r_evolve3d equals the loop of the single-purpose calls -- same iteration
    count, same flags, state bit for bit -- and differs from the run without the map."""
    gas = make_gas(pkg, (16, 16, 16), 707)
    gas.xh, gas.xhe = gas.xh_av, gas.xhe_av
    fmap = make_map(gas, 2, 9)
    dt = 1.0e5 * 3.15576e7
    mat = pkg.Material(gas.ndens, None, None)

    def engine(with_map):
        e = make_engine(pkg, tables, gas, Z_OPEN)
        e.set_plane_sources([(2, 0, FLUX)])
        e.set_plane_tilt(1, TILT)
        if with_map:
            e.set_plane_flux_map(1, fmap)
        return e
    whole = {}
    for with_map in (True, False):
        e = engine(with_map)
        niter, flags = e.evolve3d(dt)
        e.download_state(mat)
        whole[with_map] = (niter, flags, mat.xh.copy(), mat.xhe.copy())
        e.close()
    e = engine(True)
    criterion = min(int(float(orc.constants()[31]) * gas.n), e.plane_count)
    e.begin_step()
    n, conv, seen = 0, gas.n, []
    while True:
        if conv < criterion and n > 1:
            e.end_step()
            break
        if n > 500:
            break
        n += 1
        e.set_rates_to_zero()
        e.pass_sources(1, 1)
        conv = e.global_pass(dt)
        seen.append(conv)
    e.download_state(mat)
    e.close()
    niter, flags, xh, xhe = whole[True]
    assert criterion == 1 and 2 <= niter < 500 and (n, seen) == (niter, flags)
    assert np.array_equal(mat.xh, xh) and np.array_equal(mat.xhe, xhe)
    assert not np.array_equal(xh, whole[False][2])


def test_8_the_map_reaches_every_device(pkg, tables, gas_8, map_8):
    """c2r_create_multi([0, 0]), one point source and the plane: device 0 sweeps the source, device 1 runs the plane -- with the
    map, or the sum of the two devices would not equal the one-device pass."""
    one = (SRC3[0][:1], SRC3[1][:1])
    single = engine_8(pkg, tables, gas_8, map_8, one)
    start(single, gas_8)
    single.pass_sources(1, 1)
    want = (single.download_rates(), single.plane_exit_columns(1), single.plane_loss(1), single.plane_exit_flux(1))
    single.close()
    hp = pkg.hostphys
    mat = pkg.Material(gas_8.ndens, gas_8.xh.copy(), gas_8.xhe.copy(), None, True, 1.0e4, 1.0, hp.reccoef(1.0e4))
    e = pkg.HipEngine(gas_8.mesh, [0, 0])
    e.set_boundaries(Z_OPEN)
    e.set_tables(tables)
    e.set_step(mat, pkg.GridProps(gas_8.mesh, gas_8.dr, gas_8.vol), pkg.Cosmology(tps.ZRED, hp.H0, hp.Omega0))
    e.set_sources(pkg.SourceProps(np.asarray(one[0], dtype=np.int32), np.asarray(one[1], dtype=np.float64), 1.0e48))
    e.upload_state(mat)
    e.comm_init_local()
    assert e.num_devices() == 2
    e.set_plane_sources([(2, 1, FLUX)])
    e.set_plane_tilt(1, TILT)
    e.set_plane_flux_map(1, map_8)
    start(e, gas_8)
    e.pass_sources(1, 1)
    e.allreduce_rates()
    tps.same_pass(e.download_rates(), want[0])
    assert np.array_equal(e.plane_exit_columns(1), want[1]) and e.plane_loss(1) == want[2]
    assert np.array_equal(e.plane_exit_flux(1), want[3])
    e.close()


# -- 9 ---------------------------------------------------------------------------------------------------------------------
def test_9_refusals_and_lifetime(pkg, orc, otables, tables, gas_8, map_8):
    """Each refusal returns an error with a text, and the context goes on working; a new plane list drops the map, a boundary
    change keeps it."""
    E = pkg.C2RayHipError
    e = make_engine(pkg, tables, gas_8, Z_OPEN)
    with pytest.raises(E, match="c2r_set_plane_flux_map.*plane 1 not in"):
        e.set_plane_flux_map(1, None)                   # no planes yet
    e.set_plane_sources([(2, 1, FLUX)])
    for bad in (0, 2):
        with pytest.raises(E, match=f"c2r_set_plane_flux_map.*plane {bad} not in"):
            e.set_plane_flux_map(bad, None)
    assert e.lib.c2r_get_plane_flux_map_set(e.h, 0) == 0 and e.lib.c2r_get_plane_flux_map_set(e.h, 2) == 0
    for value in (-1.0e-45, float("nan"), float("inf")):
        m = map_8.copy()
        m[0, 17] = value
        with pytest.raises(E, match="c2r_set_plane_flux_map.*finite and not negative"):
            e.set_plane_flux_map(1, m)
    for k in (1, 2):
        m = map_8.copy()
        m[k, 5] = FLUX
        with pytest.raises(E, match=f"c2r_set_plane_flux_map.*SED {k}.*c2r_set_sed_tables"):
            e.set_plane_flux_map(1, m)
    assert not e.plane_flux_map_set(1)
    with pytest.raises(E, match="c2r_download_plane_exit_flux.*no pass has run plane 1 with a flux map"):
        e.plane_exit_flux(1)
    start(e, gas_8)
    e.pass_sources(1, 1)                                # a pass without a map does not make an exit flux either
    with pytest.raises(E, match="c2r_download_plane_exit_flux.*no pass has run plane 1 with a flux map"):
        e.plane_exit_flux(1)
    start(e, gas_8)
    e.pass_sources_begin(1, 1, 2)
    with pytest.raises(E, match="c2r_set_plane_flux_map.*pass"):
        e.set_plane_flux_map(1, map_8)
    with pytest.raises(E, match="c2r_download_plane_exit_flux.*pass"):
        e.plane_exit_flux(1)
    e.pass_sources_end()
    assert not e.plane_flux_map_set(1)
    e.set_plane_flux_map(1, map_8)                      # the context is usable: normal incidence with the map
    e.set_boundaries(OPEN)                              # a boundary change keeps the map
    assert e.plane_flux_map_set(1)
    start(e, gas_8)
    e.pass_sources(1, 1)
    ref = reference(orc, otables, gas_8, 2, 1, map_8)
    assert_equals_reference(e, e.download_rates(), ref)
    e.set_plane_sources([(2, 0, FLUX)])                 # a new list: no map, and no exit flux
    assert not e.plane_flux_map_set(1)
    with pytest.raises(E, match="c2r_download_plane_exit_flux.*no pass"):
        e.plane_exit_flux(1)
    e.close()
