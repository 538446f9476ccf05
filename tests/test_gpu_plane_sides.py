"""Side faces of a tilted plane on the GPU: side entry (c2r_set_plane_side_entry), side exit (c2r_enable_plane_side_exit) and
side loss (c2r_enable_plane_side_loss), against one mesh of the combined width and against the reference of
tests/plane_side_reference.py (tests/test_plane_side_host.py holds that reference to the references it extends on the CPU).
python -m pytest tests -m gpu.

The bar is that of tests/test_gpu_plane_flux_maps.py: every grid, strip, exit buffer and map bit for bit (np.array_equal);
one loss summed in another order to 1e-13 relative.  The meshes are tiny on purpose.
"""
import math
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import plane_side_reference as psr
import test_gpu_plane_sources as tps
from conftest import rel_err
from test_gpu_oblique_planes import make_gas
from test_gpu_plane_sources import DT, FLUX, GRIDS, ITER_STATE, PAIRS, SRC3, assert_grids_equal, make_engine, start

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
OPEN = (False, False, False)
SIGNS = [(1, 1), (1, -1), (-1, 1), (-1, -1)]


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


@pytest.fixture(scope="module")
def tables3(pkg):
    return pkg.RadiationTables.load().add_sed_file(GOLD / "rad_tables_pl_qpl.npz")


def make_map(mesh, axis, seed, seds=1):
    """A random map around FLUX with a few dark cells: (3, face)."""
    f_ax, g_ax = psr.face_axes(axis)
    rng = np.random.default_rng(seed)
    m = np.zeros((3, mesh[g_ax], mesh[f_ax]))
    m[:seds] = FLUX * rng.uniform(0.3, 2.0, (seds, mesh[g_ax], mesh[f_ax])) * np.array([1.0, 0.5, 0.25])[:seds, None, None]
    m[:, 1, 1:3] = 0.0
    return m.reshape(3, -1)


def box_gas(gas, lo, hi):
    """The box lo <= index < hi of a gas as a gas of its own."""
    cut = lambda a: None if a is None else psr.box_field(gas.mesh, lo, hi, a)
    mesh = tuple(hi[d] - lo[d] for d in range(3))
    return SimpleNamespace(mesh=mesh, n=int(np.prod(mesh)), ndens=cut(gas.ndens), xh=cut(gas.xh), xhe=cut(gas.xhe), xh_av=cut(gas.xh_av),
                           xhe_av=cut(gas.xhe_av), temp=cut(gas.temp), heat=gas.heat, dr=gas.dr, vol=gas.vol)


def set_ghost(e, ghost, plane=1):
    for side, cols in ((ghost or {}).get("cols") or {}).items():
        e.set_plane_side_entry(plane, side, cols, ((ghost.get("flux") or {}).get(side)))


def side_strips(e, tilt, periodic, axis, mapped, plane=1):
    """(side_cols, side_flux) of the last pass in the reference's form: a list per side, None where the side is not live."""
    live = psr.live_sides(tilt, periodic, axis)
    got = [e.plane_side_exit(plane, s, flux=mapped) if live[s] else (None, None) for s in range(2)]
    return [g[0] for g in got], [g[1] for g in got]


def run_plane(pkg, tables, gas, periodic, axis, from_high, tilt, fmap=None, flux=FLUX, ghost=None, entry=None, side_exit=False,
              side_loss=False, maps=False, curve=None, **kw):
    """One pass of one tilted plane on a fresh engine; returns the engine and what the comparisons need."""
    e = make_engine(pkg, tables, gas, periodic, **kw)
    if maps:
        e.enable_face_loss()
    if side_loss:
        e.enable_plane_side_loss()
    e.set_plane_sources([dict(axis=axis, from_high=from_high, normflux=flux)])
    e.set_plane_tilt(1, tilt)
    if fmap is not None:
        e.set_plane_flux_map(1, fmap)
    if entry is not None:
        e.set_plane_entry_columns(1, entry)
    if curve is not None:
        e.set_plane_curve(1, curve)
    set_ghost(e, ghost)
    if side_exit:
        e.enable_plane_side_exit(1)
    start(e, gas)
    e.pass_sources(1, 1)
    return e, collect(e, tilt, periodic, axis, from_high, fmap is not None, side_exit, maps)


def collect(e, tilt, periodic, axis, from_high, mapped, side_exit, maps):
    out = dict(rates=e.download_rates(), exit=e.plane_exit_columns(1), exit_flux=e.plane_exit_flux(1) if mapped else None,
               loss=e.plane_loss(1), side_cols=None, side_flux=None)
    if side_exit:
        out["side_cols"], out["side_flux"] = side_strips(e, tilt, periodic, axis, mapped)
    if maps:
        out["far_map"] = e.face_loss_map(2 * axis + (1 - from_high)).reshape(-1)
    return out


def assert_tile_equals_crop(gas, axis, lo, hi, got, whole, heat=False):
    for k in GRIDS + (("phiheat",) if heat else ()):
        assert np.array_equal(got["rates"][k], psr.box_field(gas.mesh, lo, hi, whole["rates"][k])), (k, lo)
    for k in ("exit", "exit_flux", "far_map"):
        if whole.get(k) is not None:
            assert np.array_equal(got[k], psr.box_face(gas.mesh, axis, lo, hi, whole[k])), (k, lo)


def run_tiles(pkg, tables, gas, periodic, axis, from_high, tilt, fmap, cut_f, cut_g, entry=None, **kw):
    """The tiles of `gas` cut across the plane's face axes, each on an engine of its own, upstream first, with side exit on."""
    def run(lo, hi, ghost):
        e, got = run_plane(pkg, tables, box_gas(gas, lo, hi), periodic, axis, from_high, tilt, fmap=psr.box_face(gas.mesh, axis, lo, hi, fmap),
                           ghost=ghost, entry=None if entry is None else psr.box_face(gas.mesh, axis, lo, hi, entry), side_exit=True, **kw)
        e.close()
        return got
    return psr.tiled(gas.mesh, axis, tilt, cut_f, cut_g, run)


# -- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gas_1(pkg):
    return make_gas(pkg, (8, 6, 5), 11)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("axis,from_high", PAIRS)
def test_1_two_tiles_side_by_side_equal_one_mesh(pkg, tables, gas_1, axis, from_high, sign):
    """(8,6,5), all axes open, a mapped plane through each face, tilted along one face axis only (f for from_high = 0, g for
    from_high = 1), both signs: the mesh cut in two across that axis, the upstream tile's side exit given to the downstream tile
    as side entry.  Rate grids, exit columns, exit flux and the far face's escape map of both tiles are the crops of the one
    mesh; the upstream tile ran the storing instance, so that instance changes no bit."""
    side = from_high
    tilt = (0.35 * sign, 0.0) if side == 0 else (0.0, 0.35 * sign)
    fmap = make_map(gas_1.mesh, axis, 100 + axis)
    e, whole = run_plane(pkg, tables, gas_1, OPEN, axis, from_high, tilt, fmap=fmap, maps=True)
    e.close()
    n = gas_1.mesh[psr.face_axes(axis)[side]]
    cut = (n + 1) // 2 - 1
    tiles = run_tiles(pkg, tables, gas_1, OPEN, axis, from_high, tilt, fmap, cut if side == 0 else None, cut if side == 1 else None, maps=True)
    assert len(tiles) == 2
    for lo, hi, got in tiles.values():
        assert_tile_equals_crop(gas_1, axis, lo, hi, got, whole)
        assert got["side_cols"][side] is not None and got["side_cols"][1 - side] is None
    assert np.all(whole["rates"]["phih_grid"] >= 0) and whole["loss"] > 0


# -- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e_f,e_g", SIGNS)
def test_2_two_by_two_tiles(pkg, tables, gas_1, e_f, e_g):
    """(8,6,5) along z cut at x = 3 and y = 2, both tilt components non-zero, the four sign pairs: the corner line of the tile
    downstream in both comes from the diagonal tile's strip."""
    tilt = (0.35 * e_f, 0.6 * e_g)
    fmap = make_map(gas_1.mesh, 2, 21)
    e, whole = run_plane(pkg, tables, gas_1, OPEN, 2, 0, tilt, fmap=fmap, maps=True)
    e.close()
    tiles = run_tiles(pkg, tables, gas_1, OPEN, 2, 0, tilt, fmap, 3, 2, maps=True)
    assert len(tiles) == 4
    for lo, hi, got in tiles.values():
        assert_tile_equals_crop(gas_1, 2, lo, hi, got, whole)


def test_2_heating_three_seds_fog_and_curve(pkg, tables3):
    """The same 2 x 2 tiling along y from the high side with heating, a map per SED, the LLS fog and a plane curve that the tiles
    share with its layer0 and depth0."""
    gas = make_gas(pkg, (8, 5, 6), 23, heat=True)
    tilt, curve = (-0.35, 0.5), ((2.5 * gas.dr[1], 4.5 * gas.dr[1]), (1.0, 0.5, 0.0), 1, 0.25 * gas.dr[1])
    fmap = make_map(gas.mesh, 1, 22, seds=3)
    kw = dict(maps=True, curve=curve, lls=1.0e16)
    e, whole = run_plane(pkg, tables3, gas, OPEN, 1, 1, tilt, fmap=fmap, **kw)
    e.close()
    tiles = run_tiles(pkg, tables3, gas, OPEN, 1, 1, tilt, fmap, 3, 2, **kw)
    for lo, hi, got in tiles.values():
        assert_tile_equals_crop(gas, 1, lo, hi, got, whole, heat=True)
    assert np.any(whole["rates"]["phiheat"] > 0) and whole["exit_flux"].reshape(3, -1)[2].any()


# -- 3 ---------------------------------------------------------------------------------------------------------------------
def test_3_layers_wider_than_a_block(pkg, tables):
    """(140,6,3) along z in tiles of (70,3,3): the edge lanes sit in the middle of a 64-wide block row (u = 69 of the tiles) and in
    a partial block (u = 139 of the one mesh), the ghost reads at the start of a row."""
    gas = make_gas(pkg, (140, 6, 3), 31)
    tilt = (0.35, -0.6)
    fmap = make_map(gas.mesh, 2, 32)
    e, whole = run_plane(pkg, tables, gas, OPEN, 2, 0, tilt, fmap=fmap, maps=True, side_exit=True)
    e.close()
    tiles = run_tiles(pkg, tables, gas, OPEN, 2, 0, tilt, fmap, 70, 3, maps=True)
    for lo, hi, got in tiles.values():
        assert_tile_equals_crop(gas, 2, lo, hi, got, whole)
    lo, hi, far = tiles[(1, 0)]                                     # downstream in both: x high, y low
    assert np.array_equal(far["side_cols"][0], whole["side_cols"][0][:, :, lo[1]:hi[1]])
    assert np.array_equal(far["side_flux"][1], whole["side_flux"][1][:, :, lo[0]:hi[0]])


# -- 4 ---------------------------------------------------------------------------------------------------------------------
def test_4_stacked_and_tiled(pkg, tables):
    """(8,6,6) along z as two slabs of two tiles each.  The downstream slab takes its entry columns and its map from the upstream
    slab's exit columns and exit flux, tile by tile; slot 0 of the strip its tile A hands on is then the upstream neighbour's
    exit columns and exit flux at the edge."""
    gas = make_gas(pkg, (8, 6, 6), 41)
    tilt = (0.35, 0.0)
    fmap = make_map(gas.mesh, 2, 42)
    e, whole = run_plane(pkg, tables, gas, OPEN, 2, 0, tilt, fmap=fmap, maps=True)
    e.close()
    lower, upper = tps.half(gas, pkg, 0, 3), tps.half(gas, pkg, 3, 6)
    first = run_tiles(pkg, tables, lower, OPEN, 2, 0, tilt, fmap, 3, None)
    entry, flux = np.zeros((3, 6, 8)), np.zeros((3, 6, 8))
    for lo, hi, got in first.values():
        assert np.array_equal(got["rates"]["phih_grid"], psr.box_field(gas.mesh, lo, (hi[0], hi[1], 3), whole["rates"]["phih_grid"]))
        entry[:, :, lo[0]:hi[0]] = got["exit"].reshape(3, 6, -1)
        flux[:, :, lo[0]:hi[0]] = got["exit_flux"].reshape(3, 6, -1)
    second = run_tiles(pkg, tables, upper, OPEN, 2, 0, tilt, flux.reshape(3, -1), 3, None, entry=entry.reshape(-1), maps=True)
    for lo, hi, got in second.values():
        lo3, hi3 = (lo[0], lo[1], 3), (hi[0], hi[1], 6)
        for k in GRIDS:
            assert np.array_equal(got["rates"][k], psr.box_field(gas.mesh, lo3, hi3, whole["rates"][k])), (k, lo)
        for k in ("exit", "exit_flux", "far_map"):
            assert np.array_equal(got[k], psr.box_face(gas.mesh, 2, lo, hi, whole[k])), (k, lo)
    a1, a2 = first[(0, 0)][2], second[(0, 0)][2]
    assert np.array_equal(a2["side_cols"][0][0], a1["exit"].reshape(3, 6, 3)[:, :, 2])
    assert np.array_equal(a2["side_flux"][0][0], a1["exit_flux"].reshape(3, 6, 3)[:, :, 2])


# -- 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapped", [True, False])
def test_5_exit_strips_against_the_reference(pkg, orc, otables, tables, mapped):
    """(7,6,4) along x from the high side, random ghost strips in, entry columns: every slot of both exit strips -- columns, and
    for the mapped plane fluxes -- is the reference's; for the uniform plane flux = NULL.  The rate grids too."""
    gas = make_gas(pkg, (7, 6, 4), 51)
    tilt = (0.4, -0.5)
    rng = np.random.default_rng(52)
    fmap = make_map(gas.mesh, 0, 53) if mapped else None
    entry = 1.0e17 * rng.uniform(0.0, 2.0, 3 * 24)
    ghost = {"cols": {s: 1.0e17 * rng.uniform(0.0, 2.0, (7, 3, L)) for s, L in ((0, 4), (1, 6), (2, 1))},
             "flux": {s: FLUX * rng.uniform(0.0, 2.0, (7, 3, L)) * np.array([1.0, 0.0, 0.0])[None, :, None] for s, L in ((0, 4), (1, 6), (2, 1))}}
    ref = psr.side_pass(orc, otables, gas.mesh, gas.dr, gas.vol, gas.ndens, gas.xh_av, gas.xhe_av, 0, 1, tilt, flux_map=fmap,
                        normflux=None if mapped else FLUX, entry=entry, ghost=ghost)
    e, got = run_plane(pkg, tables, gas, OPEN, 0, 1, tilt, fmap=fmap, ghost=ghost, entry=entry, side_exit=True)
    assert_grids_equal(got["rates"], ref)
    assert np.array_equal(got["exit"], ref["exit"])
    for s in range(2):
        assert np.array_equal(got["side_cols"][s], ref["side_cols"][s]), s
        if mapped:
            assert np.array_equal(got["side_flux"][s], ref["side_flux"][s]), s
    if mapped:
        assert np.array_equal(got["exit_flux"], ref["exit_flux"])
    else:
        with pytest.raises(pkg.C2RayHipError, match="c2r_download_plane_side_exit.*without a flux map"):
            e.plane_side_exit(1, 0, flux=True)
    assert np.array_equal(ref["side_cols"][0][0], entry.reshape(3, 4, 6)[:, :, 5])     # slot 0: the entry columns at the edge
    e.close()


# -- 6, 7 ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gas_6(pkg):
    return make_gas(pkg, (8, 6, 5), 61)


@pytest.mark.parametrize("axis,from_high,tilt", [(2, 0, (0.35, -0.6)), (1, 1, (-0.3, 0.5)), (0, 0, (0.4, 0.45))])
def test_6_side_loss(pkg, orc, otables, tables, gas_6, axis, from_high, tilt):
    """All axes open, side loss and escape maps on: both side faces' maps are the reference's terms bit for bit, the far face's
    map is unchanged, c2r_get_plane_side_loss is the terms' sum, photon_loss(1) is ((far) + side 0) + side 1 of the engine's own
    three numbers, and the six maps add up to photon_loss(1).  With side loss off: the same rate grids, empty side maps,
    photon_loss(1) the far loss."""
    fmap = make_map(gas_6.mesh, axis, 62)
    ref = psr.side_pass(orc, otables, gas_6.mesh, gas_6.dr, gas_6.vol, gas_6.ndens, gas_6.xh_av, gas_6.xhe_av, axis, from_high, tilt, flux_map=fmap)
    e, on = run_plane(pkg, tables, gas_6, OPEN, axis, from_high, tilt, fmap=fmap, maps=True, side_loss=True)
    assert e.plane_side_loss_enabled
    assert_grids_equal(on["rates"], ref)
    assert np.array_equal(on["far_map"], ref["terms"])
    e_sign = (1 if tilt[0] > 0 else -1, 1 if tilt[1] > 0 else -1)
    faces = [psr.side_face(axis, s, e_sign[s]) for s in range(2)]
    far = 2 * axis + (1 - from_high)
    for s in range(2):
        assert np.array_equal(e.face_loss_map(faces[s]).reshape(-1), ref["side_terms"][s]), s
        assert np.count_nonzero(ref["side_terms"][s]) > 0
    for face in range(6):
        if face not in faces + [far]:
            assert not e.face_loss_map(face).any(), face
    side = e.plane_side_loss(1)
    for s in range(2):
        print("side", s, side[s], "reference", ref["side_loss"][s], "rel", rel_err(side[s], ref["side_loss"][s]))
        assert rel_err(side[s], ref["side_loss"][s]) <= 1e-13
    loss = on["rates"]["photon_loss"][0]
    assert e.plane_loss(1) == on["loss"] and rel_err(on["loss"], ref["loss"]) <= 1e-13
    assert loss == ((0.0 + on["loss"]) + side[0]) + side[1] and not on["rates"]["photon_loss"][1:].any()
    total = math.fsum(float(x) for x in e.face_loss())
    print("maps", total, "photon_loss(1)", loss, "rel", rel_err(total, loss))
    assert rel_err(total, loss) <= 1e-13
    e.close()
    e, off = run_plane(pkg, tables, gas_6, OPEN, axis, from_high, tilt, fmap=fmap, maps=True)
    assert not e.plane_side_loss_enabled
    assert_grids_equal(off["rates"], on["rates"])
    for s in range(2):
        assert not e.face_loss_map(faces[s]).any()
    assert np.array_equal(off["far_map"], on["far_map"])
    assert off["rates"]["photon_loss"][0] == off["loss"] == on["loss"]
    with pytest.raises(pkg.C2RayHipError, match="c2r_get_plane_side_loss.*off"):
        e.plane_side_loss(1)
    e.close()


@pytest.mark.parametrize("sign", [1, -1])
def test_7_loss_under_tiling(pkg, tables, gas_6, sign):
    """(8,6,5) along z cut at x = 3, tilted along x: the one mesh's downstream side map is the downstream tile's, the far-face maps
    of the tiles side by side are the one mesh's, and what the upstream tile loses through its side is what crosses the cut."""
    tilt = (0.35 * sign, 0.0)
    fmap = make_map(gas_6.mesh, 2, 71)
    e, whole = run_plane(pkg, tables, gas_6, OPEN, 2, 0, tilt, fmap=fmap, maps=True, side_loss=True)
    face = psr.side_face(2, 0, sign)
    side_map, side = e.face_loss_map(face), e.plane_side_loss(1)
    e.close()
    assert side[0] > 0 and side[1] == 0.0
    got = {}

    def run(lo, hi, ghost):
        e, out = run_plane(pkg, tables, box_gas(gas_6, lo, hi), OPEN, 2, 0, tilt, fmap=psr.box_face(gas_6.mesh, 2, lo, hi, fmap), ghost=ghost,
                           side_exit=True, maps=True, side_loss=True)
        got[lo[0]] = (e.face_loss_map(face), e.plane_side_loss(1))
        e.close()
        return out
    tiles = psr.tiled(gas_6.mesh, 2, tilt, 3, None, run)
    for lo, hi, out in tiles.values():
        assert np.array_equal(out["far_map"], psr.box_face(gas_6.mesh, 2, lo, hi, whole["far_map"]))
    down = 3 if sign > 0 else 0
    assert np.array_equal(got[down][0], side_map) and got[down][1] == side
    assert got[3 - down][1][0] > 0


# -- 8 ---------------------------------------------------------------------------------------------------------------------
TILT_8 = (0.35, -0.6)


@pytest.fixture(scope="module")
def gas_8(pkg):
    return make_gas(pkg, (16, 16, 16), 81)


@pytest.fixture(scope="module")
def setup_8(gas_8):
    rng = np.random.default_rng(82)
    ghost = {"cols": {s: 1.0e17 * rng.uniform(0.0, 2.0, (16, 3, L)) for s, L in ((0, 16), (1, 16), (2, 1))},
             "flux": {s: FLUX * rng.uniform(0.0, 2.0, (16, 3, L)) * np.array([1.0, 0.0, 0.0])[None, :, None] for s, L in ((0, 16), (1, 16), (2, 1))}}
    return SimpleNamespace(fmap=make_map(gas_8.mesh, 2, 83), ghost=ghost)


def prepare_8(e, setup):
    e.enable_face_loss()
    e.enable_plane_side_loss()
    e.set_plane_sources([(2, 1, FLUX)])
    e.set_plane_flux_map(1, setup.fmap)
    e.set_plane_tilt(1, TILT_8)
    set_ghost(e, setup.ghost)
    e.enable_plane_side_exit(1)


def engine_8(pkg, tables, gas, setup, sources=SRC3):
    e = make_engine(pkg, tables, gas, OPEN, sources)
    prepare_8(e, setup)
    return e


def state_8(e):
    return SimpleNamespace(rates=e.download_rates(), loss=e.plane_loss(1), side=e.plane_side_loss(1), exit=e.plane_exit_columns(1),
                           exit_flux=e.plane_exit_flux(1), strips=side_strips(e, TILT_8, OPEN, 2, True), maps=[e.face_loss_map(f) for f in range(6)])


def assert_same_8(got, want, maps=True):
    tps.same_pass(got.rates, want.rates)
    assert got.loss == want.loss and got.side == want.side
    assert np.array_equal(got.exit, want.exit) and np.array_equal(got.exit_flux, want.exit_flux)
    for s in range(2):
        assert np.array_equal(got.strips[0][s], want.strips[0][s]) and np.array_equal(got.strips[1][s], want.strips[1][s])
    if maps:
        for f in range(6):
            assert np.array_equal(got.maps[f], want.maps[f]), f


@pytest.fixture(scope="module")
def run_8(pkg, tables, gas_8, setup_8):
    """The plane with ghost strips, side exit and side loss, and three point sources, in one c2r_pass_sources; then the global pass."""
    e = engine_8(pkg, tables, gas_8, setup_8)
    start(e, gas_8)
    e.pass_sources(1, 1)
    out = state_8(e)
    out.conv = e.global_pass(DT)
    out.state = e.download_iter_state()
    e.close()
    return out


def test_8_do_source_and_the_order_of_the_additions(pkg, orc, otables, tables, gas_8, setup_8, run_8):
    """c2r_do_source(NumSrc + 1) runs the plane alone: the reference's grids and strips, the same three losses as in the full pass.
    With ONE point source in the pass photon_loss(1) is (((far) + side 0) + side 1) + the source's own loss."""
    ref = psr.side_pass(orc, otables, gas_8.mesh, gas_8.dr, gas_8.vol, gas_8.ndens, gas_8.xh_av, gas_8.xhe_av, 2, 1, TILT_8,
                        flux_map=setup_8.fmap, ghost=setup_8.ghost)
    e = engine_8(pkg, tables, gas_8, setup_8)
    start(e, gas_8)
    e.do_source(4)
    alone = state_8(e)
    assert_grids_equal(alone.rates, ref)
    for s in range(2):
        assert np.array_equal(alone.strips[0][s], ref["side_cols"][s]) and np.array_equal(alone.strips[1][s], ref["side_flux"][s])
        assert rel_err(alone.side[s], ref["side_loss"][s]) <= 1e-13 and alone.side[s] > 0
    assert (alone.loss, alone.side) == (run_8.loss, run_8.side)
    assert alone.rates["photon_loss"][0] == ((0.0 + alone.loss) + alone.side[0]) + alone.side[1] < run_8.rates["photon_loss"][0]
    e.close()
    one = (SRC3[0][:1], SRC3[1][:1])
    e = make_engine(pkg, tables, gas_8, OPEN, one)
    e.enable_face_loss()
    start(e, gas_8)
    e.pass_sources(1, 1)
    src_loss = e.download_rates()["photon_loss"][0]
    prepare_8(e, setup_8)
    start(e, gas_8)
    e.pass_sources(1, 1)
    assert src_loss > 0 and e.download_rates()["photon_loss"][0] == (((0.0 + alone.loss) + alone.side[0]) + alone.side[1]) + src_loss
    e.close()


def test_8_slab_wise_allreduce_and_fused_routes(pkg, tables, gas_8, setup_8, run_8):
    """The same pass through c2r_pass_sources_begin / wait / end, c2r_pass_allreduce_chemistry and c2r_iteration."""
    e = engine_8(pkg, tables, gas_8, setup_8)
    start(e, gas_8)
    nslab = e.pass_sources_begin(1, 1, 2)
    for s in range(nslab):
        e.pass_wait_slab(s)
    e.pass_sources_end()
    assert_same_8(state_8(e), run_8)
    assert e.global_pass(DT) == run_8.conv
    start(e, gas_8)
    assert e.pass_allreduce_chemistry(DT, 1, 1, 2) == run_8.conv
    assert_same_8(state_8(e), run_8)
    assert_grids_equal(e.download_iter_state(), run_8.state, ITER_STATE)
    start(e, gas_8)
    rep = e.iteration(DT)
    assert rep["conv_flag"] == run_8.conv and np.array_equal(rep["photon_loss"], run_8.rates["photon_loss"])
    assert_same_8(state_8(e), run_8)
    assert_grids_equal(e.download_iter_state(), run_8.state, ITER_STATE)
    e.close()


def test_8_the_strips_reach_every_device(pkg, tables, gas_8, setup_8):
    """c2r_create_multi([0, 0]), one point source and the plane: device 0 sweeps the source, device 1 runs the plane -- with the
    ghost strips, the exit strips and the side loss, or the two devices' sum would not be the one-device pass."""
    one = (SRC3[0][:1], SRC3[1][:1])
    single = engine_8(pkg, tables, gas_8, setup_8, one)
    start(single, gas_8)
    single.pass_sources(1, 1)
    want = state_8(single)
    single.close()
    hp = pkg.hostphys
    mat = pkg.Material(gas_8.ndens, gas_8.xh.copy(), gas_8.xhe.copy(), None, True, 1.0e4, 1.0, hp.reccoef(1.0e4))
    e = pkg.HipEngine(gas_8.mesh, [0, 0])
    e.set_boundaries(OPEN)
    e.set_tables(tables)
    e.set_step(mat, pkg.GridProps(gas_8.mesh, gas_8.dr, gas_8.vol), pkg.Cosmology(tps.ZRED, hp.H0, hp.Omega0))
    e.set_sources(pkg.SourceProps(np.asarray(one[0], dtype=np.int32), np.asarray(one[1], dtype=np.float64), 1.0e48))
    e.upload_state(mat)
    e.comm_init_local()
    assert e.num_devices() == 2
    prepare_8(e, setup_8)
    start(e, gas_8)
    e.pass_sources(1, 1)
    e.allreduce_rates()
    assert_same_8(state_8(e), want)
    e.close()


# -- 9 ---------------------------------------------------------------------------------------------------------------------
def test_9_refusals_and_lifetime(pkg, orc, otables, tables, gas_1):
    """Every refusal has a text and leaves the state unchanged; c2r_set_plane_sources drops everything; the tilt's sign moves the
    upstream side; a periodic axis makes its strip unread and a download of it refused."""
    E = pkg.C2RayHipError
    gas, tilt = gas_1, (0.35, -0.6)
    rng = np.random.default_rng(91)
    fmap = make_map(gas.mesh, 2, 92)
    ghost = {"cols": {s: 1.0e17 * rng.uniform(0.0, 2.0, (5, 3, L)) for s, L in ((0, 6), (1, 8), (2, 1))},
             "flux": {s: FLUX * rng.uniform(0.0, 2.0, (5, 3, L)) * np.array([1.0, 0.0, 0.0])[None, :, None] for s, L in ((0, 6), (1, 8), (2, 1))}}

    def reference(t, periodic=OPEN, gh=ghost):
        return psr.side_pass(orc, otables, gas.mesh, gas.dr, gas.vol, gas.ndens, gas.xh_av, gas.xhe_av, 2, 0, t, flux_map=fmap, ghost=gh,
                             periodic=periodic)

    def rerun(e):
        start(e, gas)
        e.pass_sources(1, 1)
        return e.download_rates()
    e = make_engine(pkg, tables, gas, False)
    with pytest.raises(E, match="c2r_set_plane_side_entry.*plane 1 not in"):
        e.set_plane_side_entry(1, 0, None)                                # no planes yet
    with pytest.raises(E, match="c2r_enable_plane_side_exit.*plane 1 not in"):
        e.enable_plane_side_exit(1)
    e.set_plane_sources([(2, 0, FLUX)])
    e.set_plane_tilt(1, tilt)
    e.set_plane_flux_map(1, fmap)
    set_ghost(e, ghost)
    want = reference(tilt)
    assert_grids_equal(rerun(e), want)
    for bad in (0, 2):
        with pytest.raises(E, match=f"c2r_set_plane_side_entry.*plane {bad} not in"):
            e.set_plane_side_entry(bad, 0, ghost["cols"][0])
    for bad in (-1, 3):
        with pytest.raises(E, match=f"c2r_set_plane_side_entry.*side {bad}"):
            e.set_plane_side_entry(1, bad, ghost["cols"][0])
    with pytest.raises(E, match="c2r_set_plane_side_entry.*flux strip without a column strip"):
        e.set_plane_side_entry(1, 0, None, ghost["flux"][0])
    for value in (-1.0e-45, float("nan"), float("inf")):
        f = ghost["flux"][1].copy()
        f[2, 0, 3] = value
        with pytest.raises(E, match="c2r_set_plane_side_entry.*finite and not negative"):
            e.set_plane_side_entry(1, 1, 0.0 * ghost["cols"][1], f)
    for k in (1, 2):
        f = ghost["flux"][0].copy()
        f[1, k, 2] = FLUX
        with pytest.raises(E, match=f"c2r_set_plane_side_entry.*SED {k}.*c2r_set_sed_tables"):
            e.set_plane_side_entry(1, 0, 0.0 * ghost["cols"][0], f)
    with pytest.raises(E, match="c2r_download_plane_side_exit.*no pass has run plane 1 with the side exit enabled"):
        e.plane_side_exit(1, 0)
    e.enable_plane_side_exit(1)
    with pytest.raises(E, match="c2r_download_plane_side_exit.*no pass has run plane 1 with the side exit enabled"):
        e.plane_side_exit(1, 0)
    with pytest.raises(E, match="c2r_download_plane_side_exit.*side 2"):
        e.plane_side_exit(1, 2)
    start(e, gas)
    e.pass_sources_begin(1, 1, 2)
    for call in (lambda: e.set_plane_side_entry(1, 0, None), lambda: e.enable_plane_side_exit(1, False), lambda: e.plane_side_exit(1, 0),
                 lambda: e.enable_plane_side_loss()):
        with pytest.raises(E, match="c2r_.*side.*pass"):
            call()
    e.pass_sources_end()
    assert_grids_equal(e.download_rates(), want)                          # every refused call left the strips as they were
    for s in range(2):
        cols, flux = e.plane_side_exit(1, s)
        assert np.array_equal(cols, want["side_cols"][s]) and np.array_equal(flux, want["side_flux"][s])
    # the other sign: the upstream sides are the opposite ones, the same strips are read there
    e.set_plane_tilt(1, (-tilt[0], -tilt[1]))
    flipped = reference((-tilt[0], -tilt[1]))
    assert_grids_equal(rerun(e), flipped)
    assert not np.array_equal(flipped["phih_grid"], want["phih_grid"])
    assert np.array_equal(e.plane_side_exit(1, 1)[0], flipped["side_cols"][1])
    e.set_plane_tilt(1, tilt)
    # x periodic: side 0 is not live -- its strip and the corner line are kept and not read, a download of side 0 is refused
    e.set_boundaries((True, False, False))
    per = reference(tilt, periodic=(True, False, False))
    assert_grids_equal(rerun(e), per)
    assert_grids_equal(per, reference(tilt, periodic=(True, False, False), gh={"cols": {1: ghost["cols"][1]}, "flux": {1: ghost["flux"][1]}}))
    with pytest.raises(E, match="c2r_download_plane_side_exit.*side 0 of plane 1 was not live"):
        e.plane_side_exit(1, 0)
    assert np.array_equal(e.plane_side_exit(1, 1)[1], per["side_flux"][1])
    e.set_boundaries(OPEN)
    assert_grids_equal(rerun(e), want)                                    # ... and kept: open again, the first pass again
    e.set_plane_side_entry(1, 2, None)                                    # clearing one strip: that one reads 0.0
    cleared = reference(tilt, gh={"cols": {s: ghost["cols"][s] for s in (0, 1)}, "flux": {s: ghost["flux"][s] for s in (0, 1)}})
    assert_grids_equal(rerun(e), cleared)
    assert not np.array_equal(cleared["phih_grid"], want["phih_grid"])
    e.set_plane_sources([(2, 0, FLUX)])                                   # a new list drops strips, side exit and all
    e.set_plane_tilt(1, tilt)
    e.set_plane_flux_map(1, fmap)
    assert_grids_equal(rerun(e), reference(tilt, gh=None))
    with pytest.raises(E, match="c2r_download_plane_side_exit.*no pass has run plane 1 with the side exit enabled"):
        e.plane_side_exit(1, 0)
    e.close()
