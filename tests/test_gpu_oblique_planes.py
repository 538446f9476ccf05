"""Tilted plane-parallel sources (c2r_set_plane_tilt) on the GPU, against the reference of tests/oblique_reference.py (the
layered march of include/c2ray_hip.h in Python floats with the oracle's per-cell routines;
tests/test_oblique_reference_host.py holds the product's host-compiled functions to it on the CPU).
python -m pytest tests -m gpu.

The bar is that of tests/test_gpu_plane_sources.py, whose helpers this file uses: every grid and the exit columns bit for
bit; the loss, one sum whose order differs from math.fsum's, to 1e-13 relative.  The cells are no cubes, dr = (d, 1.25 d,
0.8 d), chosen so that the tilts of the cases stay within one cell per layer along every axis.
"""
from pathlib import Path

import numpy as np
import pytest

import oblique_reference as obr
import plane_reference as pr
import test_gpu_plane_sources as tps
from test_gpu_plane_sources import DT, FLUX, GRIDS, ITER_STATE, PAIRS, SRC3, assert_grids_equal, assert_plane_equals_reference, make_engine, start

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
OPEN = (False, False, False)
Z_OPEN = (True, True, False)
TILT = (0.35, -0.6)


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


def make_gas(pkg, mesh, seed, factors=(1.0, 1.25, 0.8), **kw):
    gas = tps.make_gas(pkg, mesh, seed, **kw)
    d = gas.dr[0]
    gas.dr = tuple(k * d for k in factors)
    gas.vol = gas.dr[0] * gas.dr[1] * gas.dr[2]
    return gas


def reference(orc, otables, gas, axis, from_high, tilt, periodic=OPEN, flux=FLUX, **kw):
    return obr.oblique_pass(orc, otables, gas.mesh, gas.dr, gas.vol, gas.ndens, gas.xh_av, gas.xhe_av, axis, from_high, flux, tilt,
                            periodic=periodic, heat=gas.heat, **kw)


def run_plane(pkg, tables, gas, periodic, axis, from_high, tilt, flux=FLUX, entry=None, **kw):
    """One pass of one tilted plane on a fresh engine: (engine, rates)."""
    e = make_engine(pkg, tables, gas, periodic, **kw)
    e.set_plane_sources([dict(axis=axis, from_high=from_high, normflux=flux)])
    e.set_plane_tilt(1, tilt)
    if entry is not None:
        e.set_plane_entry_columns(1, entry)
    start(e, gas)
    e.pass_sources(1, 1)
    return e, e.download_rates()


# -- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gas_1(pkg):
    return make_gas(pkg, (12, 10, 9), 11)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("axis,from_high", PAIRS)
def test_1_every_face_both_tilt_signs(pkg, orc, otables, tables, gas_1, axis, from_high, sign):
    """(12,10,9), all axes open: a plane through each of the six faces, tilt (+0.35, -0.6) and its negative."""
    tilt = (sign * TILT[0], sign * TILT[1])
    ref = reference(orc, otables, gas_1, axis, from_high, tilt)
    e, got = run_plane(pkg, tables, gas_1, False, axis, from_high, tilt)
    assert e.plane_tilt(1) == tilt
    assert_plane_equals_reference(e, got, ref)
    assert np.all(got["phih_grid"] > 0) and not got["phiheat"].any()
    e.close()


# -- 2 ---------------------------------------------------------------------------------------------------------------------
def test_2_layers_wider_than_one_block(pkg, orc, otables, tables):
    """(20,20,6) along z: a layer is 400 lanes in five blocks of 64 x 4, neighbours sit in other blocks and waves."""
    gas = make_gas(pkg, (20, 20, 6), 22)
    ref = reference(orc, otables, gas, 2, 0, TILT, periodic=Z_OPEN)
    e, got = run_plane(pkg, tables, gas, Z_OPEN, 2, 0, TILT)
    assert_plane_equals_reference(e, got, ref)
    e.close()


# -- 3 ---------------------------------------------------------------------------------------------------------------------
def test_3_wrap_and_side_entry_together(pkg, orc, otables, tables):
    """(9,7,5) along z, tilted along both face axes: x wraps and y takes zeros from outside; then the other way round, on the
    same context (c2r_set_boundaries_axes between two passes: the next pass takes the new wrap)."""
    gas = make_gas(pkg, (9, 7, 5), 33)
    first, second = (True, False, False), (False, True, False)
    e, got = run_plane(pkg, tables, gas, first, 2, 1, TILT)
    assert_plane_equals_reference(e, got, reference(orc, otables, gas, 2, 1, TILT, periodic=first))
    e.set_boundaries(second)
    assert e.plane_tilt(1) == TILT
    start(e, gas)
    e.pass_sources(1, 1)
    ref2 = reference(orc, otables, gas, 2, 1, TILT, periodic=second)
    assert_plane_equals_reference(e, e.download_rates(), ref2)
    assert not np.array_equal(got["phih_grid"], ref2["phih_grid"])
    e.close()


# -- 4 ---------------------------------------------------------------------------------------------------------------------
def test_4_a_f_exactly_one(pkg, orc, otables, tables):
    """dr[2] == dr[0] and tilt (1, 0): a_f == 1.0 and a_g == 0, only c3 carries weight."""
    gas = make_gas(pkg, (9, 7, 5), 44, factors=(1.0, 1.25, 1.0))
    a_f, a_g, s, _, _, _ = obr.geometry((1.0, 0.0), gas.dr, 2)
    assert a_f == 1.0 and a_g == 0.0 and s == (0.0, 0.0, 1.0, 0.0)
    e, got = run_plane(pkg, tables, gas, Z_OPEN, 2, 0, (1.0, 0.0))
    assert_plane_equals_reference(e, got, reference(orc, otables, gas, 2, 0, (1.0, 0.0), periodic=Z_OPEN))
    e.close()


def test_4_the_smallest_positive_tilt(pkg, orc, otables, tables):
    """tilt[0] = 4.9e-324: tilted (the layered march, e_f = +1) although path == dr[axis] and s_4 == 1.0."""
    gas = make_gas(pkg, (9, 7, 5), 45)
    tiny = (5e-324, 0.0)
    _, _, s, path, e_f, _ = obr.geometry(tiny, gas.dr, 2)
    assert tiny[0] > 0 and path == gas.dr[2] and s[3] == 1.0 and e_f == 1
    e, got = run_plane(pkg, tables, gas, False, 2, 0, tiny)
    assert e.plane_tilt(1) == tiny
    assert_plane_equals_reference(e, got, reference(orc, otables, gas, 2, 0, tiny))
    e.close()


# -- 5 ---------------------------------------------------------------------------------------------------------------------
def test_5_heating_three_seds(pkg, orc, gold, tables):
    """Black-body, power-law and quasar-like flux on a tilted plane, heating (phiheat as well)."""
    gas = make_gas(pkg, (9, 8, 6), 55, heat=True)
    t = pkg.RadiationTables.load().add_sed_file(GOLD / "rad_tables_pl_qpl.npz")
    with np.load(pkg.evolve.DEFAULT_TABLES) as z:
        d = {k: z[k] for k in z.files}
    zz = gold("rad_tables_pl_qpl.npz")
    d.update({k: zz[k] for k in zz.files})
    ot = orc.Tables(d)
    flux = [FLUX, 0.5 * FLUX, 0.25 * FLUX]
    ref = reference(orc, ot, gas, 2, 1, TILT, periodic=Z_OPEN, flux=flux)
    e, got = run_plane(pkg, t, gas, Z_OPEN, 2, 1, TILT, flux=flux)
    assert_plane_equals_reference(e, got, ref, heat=True)
    assert np.all(got["phiheat"] > 0)
    e.close()


@pytest.mark.parametrize("kind", ["uniform", "grid"])
def test_5_lls_fog(pkg, orc, otables, tables, kind):
    """The fog of c2r_set_lls with the tilted path, as a scalar and as the REAL(4) grid; a plane from the high side of x."""
    gas = make_gas(pkg, (7, 9, 8), 56)
    grid = (10.0 ** np.random.default_rng(7).uniform(15.5, 17, gas.n)).astype(np.float32) if kind == "grid" else None
    kw = dict(lls_grid=grid) if kind == "grid" else dict(coldensh_lls=2.0e16)
    ref = reference(orc, otables, gas, 0, 1, TILT, **kw)
    plain = reference(orc, otables, gas, 0, 1, TILT)
    assert np.all(ref["phih_grid"] < plain["phih_grid"])
    e, got = run_plane(pkg, tables, gas, False, 0, 1, TILT, lls=kw.get("coldensh_lls"), lls_grid=grid)
    assert_plane_equals_reference(e, got, ref)
    e.close()


def test_5_opaque_beyond_max_coldensh(pkg, orc, otables, tables):
    """(8,9,16) along z, gas so dense that the incoming HI column passes max_coldensh about half-way (built as
    test_e_opaque_beyond_max_coldensh builds it): exact zeros behind that point, a loss of exactly 0."""
    abu_he, _ = pr.constants(orc)
    probe = make_gas(pkg, (8, 9, 16), 404)
    own = (probe.ndens * probe.xh_av[:probe.n]).reshape(16, -1) * probe.dr[2] * (1.0 - abu_he)
    gas = make_gas(pkg, (8, 9, 16), 404, scale=pr.MAX_COLDENSH / float(np.median(np.sum(own[:8], axis=0))))
    ref = reference(orc, otables, gas, 2, 0, TILT, periodic=Z_OPEN)
    dark = ref["cin_HI"] >= pr.MAX_COLDENSH
    cin = ref["cin_HI"].reshape(16, 9 * 8)
    first_dark = np.argmax(cin >= pr.MAX_COLDENSH, axis=0)
    print("first dark cell per line: min", first_dark.min(), "max", first_dark.max())
    assert np.all(cin[-1] >= pr.MAX_COLDENSH) and first_dark.min() >= 2 and first_dark.max() <= 14
    assert ref["loss"] == 0.0 and not ref["phih_grid"][dark].any() and ref["phih_grid"][~dark].any()
    e, got = run_plane(pkg, tables, gas, Z_OPEN, 2, 0, TILT)
    assert_plane_equals_reference(e, got, ref)
    assert got["photon_loss"][0] == 0.0 and e.plane_loss(1) == 0.0
    for k in GRIDS:
        assert not got[k].reshape(-1, gas.n)[:, dark].any()
    e.close()


# -- 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic", [Z_OPEN, OPEN])
def test_6_two_slabs_equal_one_mesh(pkg, tables, periodic):
    """(10,8,12) along z against two engines of (10,8,6) that hold its halves, the second fed with the first's exit columns,
    the same tilt on all three: rates of both halves, final exit columns and downstream loss bit for bit."""
    gas = make_gas(pkg, (10, 8, 12), 66)
    runs, entry = [], None
    for g in (gas, tps.half(gas, pkg, 0, 6), tps.half(gas, pkg, 6, 12)):
        e, rates = run_plane(pkg, tables, g, periodic, 2, 0, TILT, entry=entry if g.mesh[2] == 6 else None)
        runs.append((rates, e.plane_exit_columns(1), e.plane_loss(1)))
        if g.mesh[2] == 6 and entry is None:
            entry = runs[-1][1]
        e.close()
    (big, big_exit, big_loss), (lower, _, lower_loss), (upper, upper_exit, upper_loss) = runs
    for k in GRIDS:
        b = big[k].reshape(-1, 12, 8, 10)
        assert np.array_equal(b[:, :6].reshape(-1), lower[k]), k
        assert np.array_equal(b[:, 6:].reshape(-1), upper[k]), k
    assert np.array_equal(upper_exit, big_exit)
    assert upper_loss == big_loss == upper["photon_loss"][0] and big_loss > 0
    if all(periodic[:2]):           # nothing comes in or goes out sideways: the second half can only absorb
        assert lower_loss > big_loss


# -- 7 ---------------------------------------------------------------------------------------------------------------------
def test_7_zero_tilt_is_the_old_plane(pkg, tables, gas_1):
    """A tilted pass, then set_plane_tilt(1, (0, 0)) (and None) and a pass: every grid, exit column and loss equal to those of a
    context that never heard of tilts."""
    fresh = make_engine(pkg, tables, gas_1, False)
    fresh.set_plane_sources([(1, 0, FLUX)])
    start(fresh, gas_1)
    fresh.pass_sources(1, 1)
    want = (fresh.download_rates(), fresh.plane_exit_columns(1), fresh.plane_loss(1))
    fresh.close()
    e, tilted = run_plane(pkg, tables, gas_1, False, 1, 0, TILT)
    assert not np.array_equal(tilted["phih_grid"], want[0]["phih_grid"])
    for zero in ((0.0, 0.0), None):
        e.set_plane_tilt(1, TILT)
        e.set_plane_tilt(1, zero)
        assert e.plane_tilt(1) == (0.0, 0.0)
        start(e, gas_1)
        e.pass_sources(1, 1)
        got = e.download_rates()
        assert_grids_equal(got, want[0], GRIDS + ("phiheat", "photon_loss"))
        assert np.array_equal(e.plane_exit_columns(1), want[1]) and e.plane_loss(1) == want[2]
    e.close()


# -- 8 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("from_high", [0, 1])
def test_8_escape_map_of_the_far_face(pkg, orc, otables, tables, gas_1, from_high):
    """c2r_enable_face_loss, all axes open, a plane along y: the far face's map is the reference's per-line terms bit for bit,
    every other map stays zero (what crosses a side face is in no map), and the scalars are what they are without maps."""
    ref = reference(orc, otables, gas_1, 1, from_high, TILT)
    e = make_engine(pkg, tables, gas_1, False)
    e.enable_face_loss()
    e.set_plane_sources([(1, from_high, FLUX)])
    e.set_plane_tilt(1, TILT)
    start(e, gas_1)
    e.pass_sources(1, 1)
    far = 2 * 1 + (1 - from_high)
    assert np.array_equal(e.face_loss_map(far), ref["terms"].reshape(gas_1.mesh[2], gas_1.mesh[0]))
    for face in range(6):
        if face != far:
            assert not e.face_loss_map(face).any(), face
    assert_plane_equals_reference(e, e.download_rates(), ref)
    e.close()


# -- 9 ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gas_9(pkg):
    return make_gas(pkg, (16, 16, 16), 99)


def engine_9(pkg, tables, gas, sources=SRC3):
    e = make_engine(pkg, tables, gas, Z_OPEN, sources)
    e.set_plane_sources([(2, 1, FLUX)])
    e.set_plane_tilt(1, TILT)
    return e


@pytest.fixture(scope="module")
def run_9(pkg, tables, gas_9):
    """The tilted plane and three point sources in one c2r_pass_sources, then the global pass."""
    from types import SimpleNamespace
    e = engine_9(pkg, tables, gas_9)
    start(e, gas_9)
    e.pass_sources(1, 1)
    rates = e.download_rates()
    conv = e.global_pass(DT)
    out = SimpleNamespace(rates=rates, conv=conv, state=e.download_iter_state(), plane_loss=e.plane_loss(1), exit=e.plane_exit_columns(1))
    e.close()
    return out


def test_9_do_source_runs_the_tilted_plane_alone(pkg, orc, otables, tables, gas_9, run_9):
    """c2r_do_source(NumSrc + 1): the plane only, equal to the reference; its loss is the plane's share of the full pass."""
    ref = reference(orc, otables, gas_9, 2, 1, TILT, periodic=Z_OPEN)
    e = engine_9(pkg, tables, gas_9)
    start(e, gas_9)
    e.do_source(4)
    assert_plane_equals_reference(e, e.download_rates(), ref)
    assert e.plane_loss(1) == run_9.plane_loss and np.array_equal(run_9.exit, ref["exit"])
    assert run_9.rates["sum_nbox"] > 0 and 0 < run_9.plane_loss < run_9.rates["photon_loss"][0]
    e.close()


def test_9_slab_wise_allreduce_and_fused_routes(pkg, tables, gas_9, run_9):
    """The same pass through c2r_pass_sources_begin / wait / end, c2r_pass_allreduce_chemistry and c2r_iteration: the same
    grids, loss, conv_flag and iteration state."""
    e = engine_9(pkg, tables, gas_9)
    start(e, gas_9)
    nslab = e.pass_sources_begin(1, 1, 2)
    assert nslab == 2
    for s in range(nslab):
        e.pass_wait_slab(s)
    e.pass_sources_end()
    tps.same_pass(e.download_rates(), run_9.rates)
    assert e.global_pass(DT) == run_9.conv
    assert_grids_equal(e.download_iter_state(), run_9.state, ITER_STATE)
    start(e, gas_9)
    assert e.pass_allreduce_chemistry(DT, 1, 1, 2) == run_9.conv
    tps.same_pass(e.download_rates(), run_9.rates)
    assert_grids_equal(e.download_iter_state(), run_9.state, ITER_STATE)
    start(e, gas_9)
    rep = e.iteration(DT)
    assert rep["conv_flag"] == run_9.conv and rep["sum_nbox"] == run_9.rates["sum_nbox"]
    assert np.array_equal(rep["photon_loss"], run_9.rates["photon_loss"])
    tps.same_pass(e.download_rates(), run_9.rates)
    assert_grids_equal(e.download_iter_state(), run_9.state, ITER_STATE)
    assert np.array_equal(e.plane_exit_columns(1), run_9.exit)
    e.close()


def test_9_evolve3d_with_a_tilted_plane_only(pkg, orc, tables):
    """NumSrc = 0 and one tilted plane: c2r_evolve3d equals the loop of the single-purpose calls, as
    test_h_evolve3d_with_a_plane_only has it -- same iteration count, same flags, state bit for bit -- and differs from the
    untilted run."""
    gas = make_gas(pkg, (16, 16, 16), 707)
    gas.xh, gas.xhe = gas.xh_av, gas.xhe_av
    dt = 1.0e5 * 3.15576e7
    mat = pkg.Material(gas.ndens, None, None)
    whole = {}
    for tilt in (TILT, None):
        e = make_engine(pkg, tables, gas, Z_OPEN)
        e.set_plane_sources([(2, 0, FLUX)])
        e.set_plane_tilt(1, tilt)
        niter, flags = e.evolve3d(dt)
        e.download_state(mat)
        whole[tilt] = (niter, flags, mat.xh.copy(), mat.xhe.copy())
        e.close()
    e = make_engine(pkg, tables, gas, Z_OPEN)
    e.set_plane_sources([(2, 0, FLUX)])
    e.set_plane_tilt(1, TILT)
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
    niter, flags, xh, xhe = whole[TILT]
    assert criterion == 1 and 2 <= niter < 500 and (n, seen) == (niter, flags)
    assert np.array_equal(mat.xh, xh) and np.array_equal(mat.xhe, xhe)
    assert not np.array_equal(xh, whole[None][2])


def test_9_the_tilt_reaches_every_device(pkg, tables, gas_9):
    """c2r_create_multi([0, 0]), one point source and the plane: device 0 sweeps the source, device 1 runs the plane -- with the
    tilt, or the sum of the two devices would not equal the one-device pass."""
    one = (SRC3[0][:1], SRC3[1][:1])
    single = engine_9(pkg, tables, gas_9, one)
    start(single, gas_9)
    single.pass_sources(1, 1)
    want = (single.download_rates(), single.plane_exit_columns(1), single.plane_loss(1))
    single.close()
    hp = pkg.hostphys
    mat = pkg.Material(gas_9.ndens, gas_9.xh.copy(), gas_9.xhe.copy(), None, True, 1.0e4, 1.0, hp.reccoef(1.0e4))
    e = pkg.HipEngine(gas_9.mesh, [0, 0])
    e.set_boundaries(Z_OPEN)
    e.set_tables(tables)
    e.set_step(mat, pkg.GridProps(gas_9.mesh, gas_9.dr, gas_9.vol), pkg.Cosmology(tps.ZRED, hp.H0, hp.Omega0))
    e.set_sources(pkg.SourceProps(np.asarray(one[0], dtype=np.int32), np.asarray(one[1], dtype=np.float64), 1.0e48))
    e.upload_state(mat)
    e.comm_init_local()
    assert e.num_devices() == 2
    e.set_plane_sources([(2, 1, FLUX)])
    e.set_plane_tilt(1, TILT)
    start(e, gas_9)
    e.pass_sources(1, 1)
    e.allreduce_rates()                                # the sum over the two devices, as one device adds the two: a + b
    tps.same_pass(e.download_rates(), want[0])
    assert np.array_equal(e.plane_exit_columns(1), want[1]) and e.plane_loss(1) == want[2]
    e.close()


# -- 10 --------------------------------------------------------------------------------------------------------------------
def test_10_refusals(pkg, orc, otables, tables, gas_9):
    """Each refusal returns an error with a text, and the context goes on working."""
    E = pkg.C2RayHipError
    e = make_engine(pkg, tables, gas_9, Z_OPEN)
    with pytest.raises(E, match="c2r_set_plane_tilt.*plane 1 not in"):
        e.set_plane_tilt(1, TILT)                      # no planes yet
    e.set_plane_sources([(2, 1, FLUX)])
    with pytest.raises(E, match="c2r_set_plane_tilt.*more than 1"):
        e.set_plane_tilt(1, (0.2, 1.6))                # a_g = 1.6 * 0.8 / 1.25 > 1
    with pytest.raises(E, match="c2r_set_plane_tilt.*not finite"):
        e.set_plane_tilt(1, (float("nan"), 0.0))
    with pytest.raises(E, match="c2r_set_plane_tilt.*not finite"):
        e.set_plane_tilt(1, (0.0, float("inf")))
    with pytest.raises(E, match="c2r_set_plane_tilt.*plane 0 not in"):
        e.set_plane_tilt(0, TILT)
    with pytest.raises(E, match="c2r_set_plane_tilt.*plane 2 not in"):
        e.set_plane_tilt(2, TILT)
    assert e.plane_tilt(1) == (0.0, 0.0)
    start(e, gas_9)
    e.pass_sources_begin(1, 1, 2)
    with pytest.raises(E, match="c2r_set_plane_tilt.*pass"):
        e.set_plane_tilt(1, TILT)
    e.pass_sources_end()
    assert e.plane_tilt(1) == (0.0, 0.0)
    # a tilt that fits today's cells, then cells twice as deep along the axis: the pass refuses, the old cells work again
    steep = (1.2, 0.0)                                 # a_f = 1.2 * 0.8 = 0.96
    e.set_plane_tilt(1, steep)
    hp = pkg.hostphys
    mat = pkg.Material(gas_9.ndens, gas_9.xh.copy(), gas_9.xhe.copy(), None, True, 1.0e4, 1.0, hp.reccoef(1.0e4))
    cosmo = pkg.Cosmology(tps.ZRED, hp.H0, hp.Omega0)
    deep = (gas_9.dr[0], gas_9.dr[1], 2.0 * gas_9.dr[2])
    e.set_step_scalars(mat, pkg.GridProps(gas_9.mesh, deep, gas_9.vol), cosmo)
    start(e, gas_9)
    with pytest.raises(E, match="plane 1.*more than 1"):
        e.pass_sources(1, 1)
    e.set_step_scalars(mat, pkg.GridProps(gas_9.mesh, gas_9.dr, gas_9.vol), cosmo)
    start(e, gas_9)
    e.pass_sources(1, 1)
    assert_plane_equals_reference(e, e.download_rates(), reference(orc, otables, gas_9, 2, 1, steep, periodic=Z_OPEN))
    e.set_plane_sources([(2, 0, FLUX)])               # a new list: every tilt is {0, 0} again
    assert e.plane_tilt(1) == (0.0, 0.0)
    e.close()
