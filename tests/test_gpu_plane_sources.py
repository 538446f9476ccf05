"""Plane-parallel sources (c2r_set_plane_sources): a plane wave entering through an open mesh face, on the GPU, against the
reference of tests/plane_reference.py (the 1-D march of include/c2ray_hip.h with the oracle's per-cell routines;
tests/test_plane_reference_host.py checks its premise and the product's per-cell functions on the CPU).
python -m pytest tests -m gpu.

The bar is the project's: every grid bit for bit; the loss, one sum whose order differs from math.fsum's, to 1e-13 relative.
Every case has a log-normal density and mixed ionisation, put into xh_av / xhe_av with upload_iter_state; the cells are no
cubes (dr = d, 1.25 d, 0.75 d), so that the path, the fog's dr(1) and vol_ph each have to pick their own.
"""
import ctypes as C
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import plane_reference as pr
from conftest import rel_err

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
ZRED = 9.0
DT = 1.0e6 * 3.15576e7  # s
FLUX = 3.0e-41          # per cm^2 of face, in units of S_star = 1e48 photons / s: 3e7 photons / s / cm^2
GRIDS = ("phih_grid", "phihe_grid")
ITER_STATE = ("xh_av", "xhe_av", "xh_intermed", "xhe_intermed")
Z_OPEN = (True, True, False)
PAIRS = [(a, s) for a in range(3) for s in (0, 1)]


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


def make_gas(pkg, mesh, seed, heat=False, scale=1.0):
    """ndens; the state a step starts from (nearly neutral); the mixed time-averaged fractions the pass sees."""
    n = int(np.prod(mesh))
    rng = np.random.default_rng(seed)
    ndens = scale * pkg.hostphys.test_density(ZRED) * np.exp(rng.normal(0.0, 0.7, n))
    x0 = np.full(n, 1.0e-4)
    x = 10.0 ** rng.uniform(-6, -0.3, n)
    temp = np.tile((1e4 * np.exp(rng.normal(0, 0.2, n))).astype(np.float32), 3) if heat else None
    d = pkg.hostphys.test_grid(24, ZRED)[0][0]
    dr = (d, 1.25 * d, 0.75 * d)
    return SimpleNamespace(mesh=tuple(mesh), n=n, ndens=ndens, xh=np.concatenate([1.0 - x0, x0]), xhe=np.concatenate([1.0 - x0, 0.8 * x0, 0.2 * x0]),
                           xh_av=np.concatenate([1.0 - x, x]), xhe_av=np.concatenate([1.0 - x, 0.8 * x, 0.2 * x]), temp=temp, heat=heat,
                           dr=dr, vol=dr[0] * dr[1] * dr[2])


NO_SOURCES = (np.zeros((0, 3), dtype=np.int32), np.zeros(0))


def make_engine(pkg, tables, gas, periodic, sources=NO_SOURCES, lls=None, lls_grid=None):
    hp = pkg.hostphys
    mat = pkg.Material(gas.ndens, gas.xh.copy(), gas.xhe.copy(), None if gas.temp is None else gas.temp.copy(), not gas.heat, 1.0e4, 1.0,
                       hp.reccoef(1.0e4))
    if lls is not None or lls_grid is not None:
        mat.use_LLS, mat.coldensh_LLS, mat.LLS_grid = True, float(lls or 0.0), lls_grid
    e = pkg.HipEngine(gas.mesh, 0)
    e.set_boundaries(periodic)
    e.set_tables(tables)
    e.set_step(mat, pkg.GridProps(gas.mesh, gas.dr, gas.vol), pkg.Cosmology(ZRED, hp.H0, hp.Omega0))
    e.set_sources(pkg.SourceProps(np.asarray(sources[0], dtype=np.int32), np.asarray(sources[1], dtype=np.float64), 1.0e48))
    e.upload_state(mat)
    return e


def start(e, gas):
    e.begin_step()
    e.upload_iter_state(gas.xh_av, gas.xhe_av)
    e.set_rates_to_zero()


def reference(orc, otables, gas, axis, from_high, flux=FLUX, **kw):
    return pr.plane_pass(orc, otables, gas.mesh, gas.dr, gas.vol, gas.ndens, gas.xh_av, gas.xhe_av, axis, from_high, flux, heat=gas.heat, **kw)


def assert_grids_equal(got, ref, keys=GRIDS):
    for k in keys:
        assert np.array_equal(got[k], ref[k]), (k, float(np.max(rel_err(got[k], ref[k]))), int(np.count_nonzero(got[k] != ref[k])))


def assert_plane_equals_reference(e, got, ref, heat=False, plane=1):
    assert_grids_equal(got, ref, GRIDS + (("phiheat",) if heat else ()))
    assert got["sum_nbox"] == 0
    loss = got["photon_loss"][0]
    print("loss", loss, "reference", ref["loss"], "rel", rel_err(loss, ref["loss"]))
    assert rel_err(loss, ref["loss"]) <= 1e-13 if ref["loss"] > 0 else loss == 0.0
    assert not got["photon_loss"][1:].any()
    assert e.plane_loss(plane) == loss
    assert np.array_equal(e.plane_exit_columns(plane), ref["exit"])


# -- a ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gas_a(pkg):
    return make_gas(pkg, (11, 16, 24), 101)


@pytest.mark.parametrize("axis,from_high", PAIRS)
def test_a_every_face_of_an_open_mesh(pkg, orc, otables, tables, gas_a, axis, from_high):
    """(11,16,24), all axes open, isothermal: a plane through each of the six faces."""
    ref = reference(orc, otables, gas_a, axis, from_high)
    e = make_engine(pkg, tables, gas_a, False)
    e.set_plane_sources([(axis, from_high, FLUX)])
    assert e.plane_count == 1
    start(e, gas_a)
    e.pass_sources(1, 1)
    got = e.download_rates()
    assert_plane_equals_reference(e, got, ref)
    assert np.all(got["phih_grid"] > 0) and not got["phiheat"].any()
    e.close()


# -- b, c ------------------------------------------------------------------------------------------------------------------
def oracle_global_pass(pkg, orc, otables, gas, ref, dt):
    """The oracle's global pass on a State whose rate arrays are the reference's and whose iteration state is the engine's."""
    hp = pkg.hostphys
    st = orc.Step(gas.mesh, gas.dr, gas.vol, ZRED, hp.H0, hp.Omega0, not gas.heat, 1.0e4, 1.0, np.array([[1, 1, 1]], dtype=np.int32),
                  np.array([1.0]), 1.0e48, gas.ndens, hp.reccoef(1.0e4))
    s = orc.State(st, gas.xh, gas.xhe, gas.temp)
    orc.begin_step(s)
    s.xh_av[:], s.xhe_av[:] = gas.xh_av, gas.xhe_av
    s.phih[:], s.phihe[:], s.phiheat[:] = ref["phih_grid"], ref["phihe_grid"], ref["phiheat"]
    conv = orc.global_pass(otables, st, s, dt)
    return conv, {k: getattr(s, k).copy() for k in ITER_STATE}


@pytest.fixture(scope="module")
def gas_b(pkg):
    return make_gas(pkg, (16, 16, 16), 202, heat=True)


def test_b_heating_and_the_global_pass(pkg, orc, otables, tables, gas_b):
    """16^3, z open, x and y periodic, heating: phiheat as well; then the iteration state after one global pass."""
    ref = reference(orc, otables, gas_b, 2, 0)
    e = make_engine(pkg, tables, gas_b, Z_OPEN)
    e.set_plane_sources([(2, 0, FLUX)])
    start(e, gas_b)
    e.pass_sources(1, 1)
    got = e.download_rates()
    assert_plane_equals_reference(e, got, ref, heat=True)
    assert np.all(got["phiheat"] > 0)
    conv_ref, state_ref = oracle_global_pass(pkg, orc, otables, gas_b, ref, DT)
    assert e.global_pass(DT) == conv_ref
    assert_grids_equal(e.download_iter_state(), state_ref, ITER_STATE)
    e.close()


def test_c_heating_three_seds(pkg, orc, gold, gas_b):
    """b with black-body, power-law and quasar-like flux on the plane (the reference's -DPL -DQUASARS build)."""
    if not (GOLD / "rad_tables_pl_qpl.npz").exists():
        pytest.skip("rad_tables_pl_qpl.npz not present")
    t = pkg.RadiationTables.load().add_sed_file(GOLD / "rad_tables_pl_qpl.npz")
    with np.load(pkg.evolve.DEFAULT_TABLES) as z:
        d = {k: z[k] for k in z.files}
    zz = gold("rad_tables_pl_qpl.npz")
    d.update({k: zz[k] for k in zz.files})
    ot = orc.Tables(d)
    flux = [FLUX, 0.5 * FLUX, 0.25 * FLUX]
    ref = reference(orc, ot, gas_b, 2, 1, flux)
    e = make_engine(pkg, t, gas_b, Z_OPEN)
    e.set_plane_sources([dict(axis=2, from_high=1, normflux=flux)])
    start(e, gas_b)
    e.pass_sources(1, 1)
    got = e.download_rates()
    assert_plane_equals_reference(e, got, ref, heat=True)
    conv_ref, state_ref = oracle_global_pass(pkg, orc, ot, gas_b, ref, DT)
    assert e.global_pass(DT) == conv_ref
    assert_grids_equal(e.download_iter_state(), state_ref, ITER_STATE)
    e.close()


# -- d ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "grid"])
def test_d_lls_fog(pkg, orc, otables, tables, kind):
    """11^3, x open, a plane from the high side of x: the fog of c2r_set_lls on every cell's incoming HI column, as a scalar
    and as the REAL(4) grid."""
    gas = make_gas(pkg, (11, 11, 11), 303)
    grid = (10.0 ** np.random.default_rng(7).uniform(15.5, 17, gas.n)).astype(np.float32) if kind == "grid" else None
    kw = dict(lls_grid=grid) if kind == "grid" else dict(coldensh_lls=2.0e16)
    ref = reference(orc, otables, gas, 0, 1, **kw)
    plain = reference(orc, otables, gas, 0, 1)
    assert np.all(ref["phih_grid"] < plain["phih_grid"])
    e = make_engine(pkg, tables, gas, (False, True, True), lls=kw.get("coldensh_lls"), lls_grid=grid)
    e.set_plane_sources([(0, 1, FLUX)])
    start(e, gas)
    e.pass_sources(1, 1)
    assert_plane_equals_reference(e, e.download_rates(), ref)
    e.close()


# -- e ---------------------------------------------------------------------------------------------------------------------
def test_e_opaque_beyond_max_coldensh(pkg, orc, otables, tables):
    """(8,9,16), z open, gas so dense that the incoming HI column passes max_coldensh about half-way: exact zeros behind that
    point, a loss of exactly 0."""
    abu_he, _ = pr.constants(orc)
    probe = make_gas(pkg, (8, 9, 16), 404)
    # the column in front of cell 8 of the median line of cells is max_coldensh
    own = (probe.ndens * probe.xh_av[:probe.n]).reshape(16, -1) * probe.dr[2] * (1.0 - abu_he)
    gas = make_gas(pkg, (8, 9, 16), 404, scale=pr.MAX_COLDENSH / float(np.median(np.sum(own[:8], axis=0))))
    ref = reference(orc, otables, gas, 2, 0)
    dark = ref["cin_HI"] >= pr.MAX_COLDENSH
    cin = ref["cin_HI"].reshape(16, 9 * 8)
    first_dark = np.argmax(cin >= pr.MAX_COLDENSH, axis=0)
    print("first dark cell per column: min", first_dark.min(), "max", first_dark.max())
    assert np.all(cin[-1] >= pr.MAX_COLDENSH) and first_dark.min() >= 3 and first_dark.max() <= 14
    assert ref["loss"] == 0.0 and not ref["phih_grid"][dark].any() and np.all(ref["phih_grid"][~dark] >= 0) and ref["phih_grid"][~dark].any()
    e = make_engine(pkg, tables, gas, Z_OPEN)
    e.set_plane_sources([(2, 0, FLUX)])
    start(e, gas)
    e.pass_sources(1, 1)
    got = e.download_rates()
    assert_plane_equals_reference(e, got, ref)
    assert got["photon_loss"][0] == 0.0 and e.plane_loss(1) == 0.0
    for k in GRIDS:
        assert not got[k].reshape(-1, gas.n)[:, dark].any()
    e.close()


# -- f ---------------------------------------------------------------------------------------------------------------------
def half(gas, pkg, lo, hi):
    """The k-planes [lo, hi) of a gas as a gas of its own."""
    cut = lambda a: None if a is None else np.ascontiguousarray(a.reshape(-1, gas.mesh[2], gas.mesh[1], gas.mesh[0])[:, lo:hi]).reshape(-1)
    mesh = (gas.mesh[0], gas.mesh[1], hi - lo)
    return SimpleNamespace(mesh=mesh, n=int(np.prod(mesh)), ndens=cut(gas.ndens), xh=cut(gas.xh), xhe=cut(gas.xhe), xh_av=cut(gas.xh_av),
                           xhe_av=cut(gas.xhe_av), temp=cut(gas.temp), heat=gas.heat, dr=gas.dr, vol=gas.vol)


def test_f_two_slabs_handing_over_equal_one_mesh(pkg, tables):
    """(16,16,32), z open, a plane from the low side of z, against two engines of (16,16,16) that hold its halves, the second
    fed with the first's exit columns: rate grids of the halves bit-equal to the halves of the big run, the second engine's
    loss bit-equal to the big run's."""
    gas = make_gas(pkg, (16, 16, 32), 505)
    runs = []
    entry = None
    for g in (gas, half(gas, pkg, 0, 16), half(gas, pkg, 16, 32)):
        e = make_engine(pkg, tables, g, Z_OPEN)
        e.set_plane_sources([(2, 0, FLUX)])
        if g.mesh[2] == 16 and entry is not None:
            e.set_plane_entry_columns(1, entry)
        start(e, g)
        e.pass_sources(1, 1)
        runs.append((e.download_rates(), e.plane_exit_columns(1), e.plane_loss(1)))
        if g.mesh[2] == 16 and entry is None:
            entry = runs[-1][1]
        e.close()
    (big, big_exit, big_loss), (lower, _, lower_loss), (upper, upper_exit, upper_loss) = runs
    for k in GRIDS:
        b = big[k].reshape(-1, 32, 16, 16)
        assert np.array_equal(b[:, :16].reshape(-1), lower[k]), k
        assert np.array_equal(b[:, 16:].reshape(-1), upper[k]), k
    assert np.array_equal(upper_exit, big_exit)
    assert upper_loss == big_loss == upper["photon_loss"][0] and big_loss > 0 and lower_loss > big_loss


# -- g ---------------------------------------------------------------------------------------------------------------------
SRC3 = (np.array([[3, 4, 2], [12, 9, 14], [8, 16, 7]], dtype=np.int32), np.array([2.0e7, 1.0e7, 1.5e7]))


@pytest.fixture(scope="module")
def gas_g(pkg):
    return make_gas(pkg, (16, 16, 16), 606)


@pytest.fixture(scope="module")
def run_g(pkg, tables, gas_g):
    """A: the plane and three point sources in one pass (batch 256), then the global pass."""
    e = make_engine(pkg, tables, gas_g, Z_OPEN, SRC3)
    e.set_plane_sources([(2, 1, FLUX)])
    start(e, gas_g)
    e.pass_sources(1, 1)
    rates = e.download_rates()
    conv = e.global_pass(DT)
    out = SimpleNamespace(rates=rates, conv=conv, state=e.download_iter_state(), plane_loss=e.plane_loss(1))
    e.close()
    return out


def same_pass(got, ref):
    assert_grids_equal(got, ref, GRIDS + ("photon_loss",))
    assert got["sum_nbox"] == ref["sum_nbox"]


def test_g_planes_before_point_sources(pkg, tables, gas_g, run_g):
    """A with one source per batch; B: a plane-only pass (c2r_do_source(NumSrc + 1)), the planes removed, then the point
    sources on top with no zeroing in between.  All bit-equal: the plane is added first, everything else accumulates."""
    assert run_g.rates["sum_nbox"] > 0 and 0 < run_g.plane_loss < run_g.rates["photon_loss"][0]
    e = make_engine(pkg, tables, gas_g, Z_OPEN, SRC3)
    e.set_plane_sources([(2, 1, FLUX)])
    e.set_batch(1)
    start(e, gas_g)
    e.pass_sources(1, 1)
    same_pass(e.download_rates(), run_g.rates)
    start(e, gas_g)
    e.do_source(4)
    only = e.download_rates()
    assert only["sum_nbox"] == 0 and only["photon_loss"][0] == run_g.plane_loss
    e.set_plane_sources([])
    assert e.plane_count == 0
    e.pass_sources(1, 1)
    same_pass(e.download_rates(), run_g.rates)
    e.close()


def test_g_slab_wise_and_fused_routes(pkg, tables, gas_g, run_g):
    """A through c2r_pass_sources_begin(nslab = 2) / wait / end, and through c2r_iteration: the same grids, loss and conv_flag."""
    e = make_engine(pkg, tables, gas_g, Z_OPEN, SRC3)
    e.set_plane_sources([(2, 1, FLUX)])
    start(e, gas_g)
    nslab = e.pass_sources_begin(1, 1, 2)
    assert nslab == 2
    for s in range(nslab):
        e.pass_wait_slab(s)
    e.pass_sources_end()
    same_pass(e.download_rates(), run_g.rates)
    assert e.global_pass(DT) == run_g.conv
    assert_grids_equal(e.download_iter_state(), run_g.state, ITER_STATE)
    start(e, gas_g)
    rep = e.iteration(DT)
    assert rep["conv_flag"] == run_g.conv and rep["sum_nbox"] == run_g.rates["sum_nbox"]
    assert np.array_equal(rep["photon_loss"], run_g.rates["photon_loss"])
    same_pass(e.download_rates(), run_g.rates)
    assert_grids_equal(e.download_iter_state(), run_g.state, ITER_STATE)
    e.close()


def test_g_a_plane_only_slab_wise_pass(pkg, orc, otables, tables, gas_g):
    """A pass with a plane and no point source through the slab-wise route: its slab events come behind the plane."""
    ref = reference(orc, otables, gas_g, 2, 1)
    e = make_engine(pkg, tables, gas_g, Z_OPEN)
    e.set_plane_sources([(2, 1, FLUX)])
    start(e, gas_g)
    for s in range(e.pass_sources_begin(1, 1, 2)):
        e.pass_wait_slab(s)
    e.pass_sources_end()
    assert_plane_equals_reference(e, e.download_rates(), ref)
    e.close()


# -- h ---------------------------------------------------------------------------------------------------------------------
def test_h_evolve3d_with_a_plane_only(pkg, orc, tables):
    """NumSrc = 0 and one plane: c2r_evolve3d equals the loop of the single-purpose calls (evolve.F90:147-217, a plane
    counting as a source in the convergence criterion) -- same iteration count, same flags, state bit for bit."""
    gas = make_gas(pkg, (16, 16, 16), 707)
    gas.xh, gas.xhe = gas.xh_av, gas.xhe_av        # evolve3D starts from the state itself
    dt = 1.0e5 * 3.15576e7
    mat = pkg.Material(gas.ndens, None, None)
    e = make_engine(pkg, tables, gas, Z_OPEN)
    e.set_plane_sources([(2, 0, FLUX)])
    niter, flags = e.evolve3d(dt)
    e.download_state(mat)
    whole = (mat.xh.copy(), mat.xhe.copy())
    e.close()
    e = make_engine(pkg, tables, gas, Z_OPEN)
    e.set_plane_sources([(2, 0, FLUX)])
    criterion = min(int(float(orc.constants()[31]) * gas.mesh[0] * gas.mesh[1] * gas.mesh[2]), 0 + e.plane_count)
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
    print("iterations", niter, "flags", flags)
    assert criterion == 1 and 2 <= niter < 500
    assert (n, seen) == (niter, flags)
    assert np.array_equal(mat.xh, whole[0]) and np.array_equal(mat.xhe, whole[1])
    assert not np.array_equal(mat.xh, gas.xh)


# -- i ---------------------------------------------------------------------------------------------------------------------
def test_i_the_deal_gives_a_plane_to_one_caller(pkg, orc, otables, tables, gas_g):
    """NumSrc = 1 plus one plane dealt over two callers: c2r_pass_sources(1, 2) holds the source only and equals a run
    without planes; c2r_pass_sources(2, 2) holds "source 2", the plane, only."""
    one = (SRC3[0][:1], SRC3[1][:1])
    e0 = make_engine(pkg, tables, gas_g, Z_OPEN, one)
    start(e0, gas_g)
    e0.pass_sources(1, 1)
    without = e0.download_rates()
    e0.close()
    assert without["sum_nbox"] > 0
    got = []
    for first in (1, 2):
        e = make_engine(pkg, tables, gas_g, Z_OPEN, one)
        e.set_plane_sources([(2, 1, FLUX)])
        start(e, gas_g)
        e.pass_sources(first, 2)
        got.append(e.download_rates())
        if first == 2:
            assert_plane_equals_reference(e, got[-1], reference(orc, otables, gas_g, 2, 1))
        e.close()
    same_pass(got[0], without)


# -- j ---------------------------------------------------------------------------------------------------------------------
def test_j_refusals(pkg, orc, otables, tables, gas_g):
    """Each refusal returns an error with a text, and the context goes on working."""
    E = pkg.C2RayHipError
    e = make_engine(pkg, tables, gas_g, Z_OPEN, SRC3)
    with pytest.raises(E, match="axis 0.*periodic"):
        e.set_plane_sources([(0, 0, FLUX)])
    with pytest.raises(E, match="axis 3"):
        e.set_plane_sources([(3, 0, FLUX)])
    with pytest.raises(E, match="7 planes"):
        e.set_plane_sources([(2, 0, FLUX)] * 7)
    with pytest.raises(E, match="SED 1.*tables"):
        e.set_plane_sources([(2, 0, [FLUX, FLUX, 0.0])])
    assert e.plane_count == 0
    e.set_plane_sources([(2, 1, FLUX)])
    with pytest.raises(E, match="c2r_set_boundaries.*plane source 1.*axis 2"):
        e.set_boundaries(True)
    with pytest.raises(E, match="c2r_set_boundaries.*plane"):
        e.set_boundaries((False, False, True))
    assert e.periodic_axes == Z_OPEN and e.plane_count == 1
    start(e, gas_g)
    e.pass_sources_begin(1, 1, 2)
    with pytest.raises(E, match="c2r_set_plane_sources.*pass"):
        e.set_plane_sources([])
    with pytest.raises(E, match="c2r_set_plane_entry_columns.*pass"):
        e.set_plane_entry_columns(1, None)
    e.pass_sources_end()
    with pytest.raises(E, match="plane 2 not in"):
        e.plane_loss(2)
    assert e.plane_count == 1
    e.set_sources(pkg.SourceProps(*NO_SOURCES))      # c2r_set_sources leaves the planes alone
    assert e.plane_count == 1
    start(e, gas_g)
    e.pass_sources(1, 1)
    assert_plane_equals_reference(e, e.download_rates(), reference(orc, otables, gas_g, 2, 1))
    e.set_plane_sources([])
    e.set_boundaries(True)                           # nothing stands in the way any more
    assert e.periodic is True
    e.close()
