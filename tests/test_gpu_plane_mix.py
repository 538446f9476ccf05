"""Several planes at once, with point sources, on the GPU, against the composition of tests/mix_reference.py: every plane from
the reference of its kind (plane_reference, oblique_reference, flux_reference), folded in plane order, the point sources on
top through the oracle's do_source on the periodic embedding, the escape maps from the planes' terms and
face_loss_reference.  tests/test_mix_reference_host.py holds that composition to account on the CPU.
python -m pytest tests -m gpu.

The bar: phih_grid, phihe_grid, phiheat where heating is on, the exit columns of every plane, the exit flux of every mapped
plane, the escape maps and sum_nbox bit for bit; c2r_get_plane_loss to 1e-13 relative against that plane's reference loss
(one sum in another order than math.fsum's); photon_loss(1) to 1e-12 relative against math.fsum of the planes' losses and the
point sources' kept terms WHERE THAT REFERENCE EXISTS: all axes open and every source's final box its whole reach (the "xyz"
mesh).  On every other mesh of this file a periodic axis has box faces at +-N/2 that lose photons no map holds, or a box
stops short of its reach: there photon_loss(1) is checked through its parts only -- the per-plane losses and the maps --
and is asserted to be no smaller than the planes' share.

The gas is axis_boundary_cases' kind "mixed", the pass runs right after begin_step (the oracle and the engine see the same
xh_av), the cells are no cubes.  A point source is only used where mix_reference.same_cells holds: the oracle on the embedding
and the product on the open mesh then trace the same cells (asserted on the CPU side of every case).  In mixed gas that keeps
every point source of cases a to i to ONE round; case j, in ionised gas, is the one where point sources that need several
rounds meet planes.
Measured on one MI355X: the 31 cases of this file take 6.9 s, references included; none takes more than 0.6 s.
"""
import os
from pathlib import Path

import numpy as np
import pytest

import axis_boundary_cases as ab
import mix_reference as mx
import oblique_reference as obr
import plane_reference as pr
from conftest import rel_err

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
DT = 1.0e6 * 3.15576e7
DEFAULT_CASES, DEFAULT_SEED = 12, 20261019
ROUTES = ("plain", "slabs", "iteration")


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


@pytest.fixture(scope="module")
def tables3(pkg):
    return pkg.RadiationTables.load().add_sed_file(GOLD / "rad_tables_pl_qpl.npz")


@pytest.fixture(scope="module")
def otables3(pkg, orc, gold):
    with np.load(pkg.evolve.DEFAULT_TABLES) as z:
        d = {k: z[k] for k in z.files}
    zz = gold("rad_tables_pl_qpl.npz")
    d.update({k: zz[k] for k in zz.files})
    return orc.Tables(d)


def make_engine(pkg, tables, case, planes, coldensh_lls=None, lls_grid=None, maps=False, batch=None):
    """A context of the case's mesh, boundaries, gas and point sources with `planes` set: tilts, maps and entry columns too."""
    hp = pkg.hostphys
    ndens, xh, xhe, temp = case.region
    mat = pkg.Material(ndens, xh.copy(), xhe.copy(), None if temp is None else temp.copy(), not case.heat, 1.0e4, 1.0, case.reccoef)
    if coldensh_lls is not None or lls_grid is not None:
        mat.use_LLS, mat.coldensh_LLS, mat.LLS_grid = True, float(coldensh_lls or 0.0), lls_grid
    src = pkg.SourceProps(case.srcpos, case.flux, case.s_star)
    if case.pl is not None:
        src.NormFluxPL, src.pl_S_star = case.pl, case.pl_s_star
        src.NormFluxQPL, src.qpl_S_star = case.qpl, case.qpl_s_star
    e = pkg.HipEngine(case.n, 0)
    e.set_boundaries(case.periodic)
    e.set_tables(tables)
    e.set_step(mat, pkg.GridProps(case.n, case.dr, case.vol), pkg.Cosmology(ab.ZRED, hp.H0, hp.Omega0))
    e.set_sources(src)
    e.upload_state(mat)
    if maps:
        e.enable_face_loss()
    if batch is not None:
        e.set_batch(batch)
    e.set_plane_sources([dict(axis=p["axis"], from_high=p["from_high"], normflux=p["normflux"]) for p in planes])
    assert e.plane_count == len(planes)
    for k, p in enumerate(planes, start=1):                 # odd planes: the map first, the tilt second; even ones the other way
        for what in (("fmap", "tilt") if k % 2 else ("tilt", "fmap")):
            if p.get(what) is not None:
                (e.set_plane_flux_map if what == "fmap" else e.set_plane_tilt)(k, p[what])
        if p.get("entry") is not None:
            e.set_plane_entry_columns(k, p["entry"])
    for k, p in enumerate(planes, start=1):
        tilted, mapped = mx.plane_kind(p)
        assert e.plane_flux_map_set(k) == mapped and e.plane_tilt(k) == (tuple(p["tilt"]) if tilted else (0.0, 0.0)), k
    return e


def run_pass(e, route="plain", first=1, stride=1):
    """One pass of caller (first, stride) from zeroed rates, right after begin_step: what c2r_download_rates returns."""
    e.begin_step()
    e.set_rates_to_zero()
    if route == "plain":
        e.pass_sources(first, stride)
    elif route == "slabs":
        nslab = e.pass_sources_begin(first, stride, 2)
        assert nslab == 2
        for s in range(nslab):
            e.pass_wait_slab(s)
        e.pass_sources_end()
    elif route == "iteration":
        rep = e.iteration(DT, first, stride)
        got = e.download_rates()
        assert rep["sum_nbox"] == got["sum_nbox"] and np.array_equal(rep["photon_loss"], got["photon_loss"])
        return got
    else:
        raise ValueError(route)
    return e.download_rates()


def assert_equals_composition(e, got, mix, case, planes, maps=False, tag=""):
    """The bar of this file (the module's docstring)."""
    assert all(mix["same_cells"]), (tag, mix["nbox"])                          # the embedding: both trace the same cells
    for k in ("phih_grid", "phihe_grid") + (("phiheat",) if case.heat else ()):
        bad = int(np.count_nonzero(got[k] != mix[k]))
        print(tag, k, "cells", got[k].size, "differ", bad, "worst rel", float(np.max(rel_err(got[k], mix[k]))))
        assert np.array_equal(got[k], mix[k]), (tag, k, bad)
    if not case.heat:
        assert not got["phiheat"].any(), tag
    assert got["sum_nbox"] == mix["sum_nbox"], (tag, got["sum_nbox"], mix["sum_nbox"])
    for p in mix["planes"]:
        ref = mix["plane"][p]
        assert np.array_equal(e.plane_exit_columns(p), ref["exit"]), (tag, p)
        if mx.plane_kind(planes[p - 1])[1]:
            assert np.array_equal(e.plane_exit_flux(p), ref["exit_flux"]), (tag, p)
        loss = e.plane_loss(p)
        print(tag, "plane", p, "loss", loss, "reference", ref["loss"], "rel", rel_err(loss, ref["loss"]) if ref["loss"] > 0 else 0.0)
        assert rel_err(loss, ref["loss"]) <= 1e-13 if ref["loss"] > 0 else loss == 0.0, (tag, p)
    if maps:
        for f, want in mix["maps"].items():
            have = e.face_loss_map(f)
            bad = int(np.count_nonzero(have != want))
            print(tag, "face", f, "cells", want.size, "non-zero", int(np.count_nonzero(want)), "differ", bad)
            assert have.shape == want.shape and np.array_equal(have, want), (tag, f, bad)
    loss = got["photon_loss"][0]
    assert not got["photon_loss"][1:].any()
    planes_share = float(np.sum([mix["plane"][p]["loss"] for p in mix["planes"]]))
    if mix["loss"] is not None:
        print(tag, "photon_loss(1)", loss, "reference", mix["loss"], "rel", rel_err(loss, mix["loss"]) if mix["loss"] > 0 else 0.0)
        assert rel_err(loss, mix["loss"]) <= 1e-12 if mix["loss"] > 0 else loss == 0.0, tag
    else:                                                   # no reference for the point sources' share: the parts only
        assert loss >= planes_share * (1.0 - 1e-13), (tag, loss, planes_share)
        if not mix["sources"]:
            assert rel_err(loss, planes_share) <= 1e-12 if planes_share > 0 else loss == 0.0, tag


# -- a ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case_a(pkg):
    return mx.case_a(pkg)


@pytest.fixture(scope="module")
def mix_a(pkg, orc, otables, case_a):
    return mx.compose(pkg, orc, otables, case_a, mx.PLANES_A, "mix_a")


@pytest.mark.parametrize("route", ["batch_1", "batch_256", "slabs", "iteration"])
def test_a_two_planes_through_opposite_faces(pkg, tables, case_a, mix_a, route):
    """(11,11,11), z open, planes through z = 1 and z = 11 with different fluxes, four point sources, escape maps on: one source
    per batch, one batch, the slab-wise route and c2r_iteration, each against the composition."""
    assert mix_a["planes"] == [1, 2] and mix_a["sources"] == [1, 2, 3, 4] and mix_a["sum_nbox"] == 4
    e = make_engine(pkg, tables, case_a, mx.PLANES_A, maps=True, batch={"batch_1": 1, "batch_256": 256}.get(route))
    got = run_pass(e, route if route in ROUTES else "plain")
    assert_equals_composition(e, got, mix_a, case_a, mx.PLANES_A, maps=True, tag=route)
    assert np.all(got["phih_grid"] > 0) and all(mix_a["maps"][f].any() for f in (4, 5))
    e.close()


# -- b ---------------------------------------------------------------------------------------------------------------------
def test_b_faces_of_different_sizes_smaller_face_first(pkg, orc, otables, tables):
    """(11,24,24), x and z open: plane 1 along z (a face of 264 cells, more than one block), plane 2 along x (576 cells), tilted,
    its y axis wrapping and its z side open, plane 3 along z from the other side; the buffers all planes share are sized by
    the largest face, and only plane 2 has a tilt."""
    case = mx.make_case(pkg, "xz", [(1, 1, 1), (11, 24, 24), (6, 1, 12), (11, 13, 1)], ab.FLUX4)
    planes = [dict(axis=2, from_high=0, normflux=mx.FLUX), dict(axis=0, from_high=0, normflux=0.8 * mx.FLUX, tilt=mx.TILT),
              dict(axis=2, from_high=1, normflux=0.5 * mx.FLUX)]
    a_f, a_g = obr.geometry(mx.TILT, case.dr, 0)[:2]
    assert 0 < a_f <= 1 and 0 < a_g <= 1 and [pr.face_cells(case.n, p["axis"]) for p in planes] == [264, 576, 264]
    mix = mx.compose(pkg, orc, otables, case, planes, "mix_b")
    e = make_engine(pkg, tables, case, planes, maps=True)
    assert_equals_composition(e, run_pass(e), mix, case, planes, maps=True, tag="b")
    e.close()


# -- c ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tilted,mapped", [((2, 4), (3, 4)), ((3,), (2,))])
def test_c_every_kind_of_plane_in_one_list(pkg, orc, otables, tables, tilted, mapped):
    """(11,11,24), x and y open, four planes through four faces: plain, tilted, mapped, tilted and mapped, two different maps with
    dark cells; and the same list with only the third tilted and only the second mapped -- the per-plane flags do not slide.
    Planes 2 and 3 have entry columns, planes 1 and 4 none."""
    case = mx.case_c(pkg)
    planes = mx.planes_c(case, tilted, mapped)
    for p in planes:
        if mx.plane_kind(p)[0]:
            a_f, a_g = obr.geometry(p["tilt"], case.dr, p["axis"])[:2]
            assert 0 < a_f <= 1 and 0 < a_g <= 1
    mix = mx.compose(pkg, orc, otables, case, planes, "mix_c")
    e = make_engine(pkg, tables, case, planes, maps=True)
    assert_equals_composition(e, run_pass(e), mix, case, planes, maps=True, tag=f"c {tilted} {mapped}")
    for p in range(1, 5):
        if p not in mapped:
            with pytest.raises(pkg.C2RayHipError, match="no pass has run plane"):
                e.plane_exit_flux(p)
    e.close()


# -- d ---------------------------------------------------------------------------------------------------------------------
def test_d_two_planes_through_the_same_face(pkg, orc, otables, tables, case_a):
    """Both planes enter through z = 11 with different fluxes: the rates and the map of the face z = 1 receive both, in plane
    order, and each plane keeps its own exit columns and loss."""
    mix = mx.compose(pkg, orc, otables, case_a, mx.PLANES_D, "mix_a")
    e = make_engine(pkg, tables, case_a, mx.PLANES_D, maps=True)
    got = run_pass(e)
    assert_equals_composition(e, got, mix, case_a, mx.PLANES_D, maps=True, tag="d")
    assert e.plane_loss(1) > e.plane_loss(2) > 0 and np.array_equal(e.plane_exit_columns(1), e.plane_exit_columns(2))
    e.close()


# -- e ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("who", ["both", "planes_only", "sources_only"])
def test_e_heating_with_three_seds(pkg, orc, otables3, tables3, who):
    """(11,11,11), z open, heating: plane 1 black body only, plane 2 power-law and quasar-like flux, the point sources those of
    axis_boundary_cases.case_e(seds=True); then only a plane uses SED 1 and 2 while the point sources use none (the planes'
    own set of tables), and the reverse."""
    kw = dict(pl=np.array([1e6, 2e6, 0.0, 5e5]), qpl=np.array([0.0, 1e6, 3e6, 5e5])) if who != "planes_only" else {}
    flux = np.array([3e6, 0.0, 1e6, 2e6]) if who != "planes_only" else mx.FLUX_E
    case = mx.make_case(pkg, "z", ab.E_SOURCES, flux, heat=True, **kw)
    second = [0.0, 0.5 * mx.FLUX, 0.25 * mx.FLUX] if who != "sources_only" else [0.7 * mx.FLUX, 0.0, 0.0]
    planes = [dict(axis=2, from_high=0, normflux=[mx.FLUX, 0.0, 0.0]), dict(axis=2, from_high=1, normflux=second)]
    mix = mx.compose(pkg, orc, otables3, case, planes, "mix_e_" + who)
    e = make_engine(pkg, tables3, case, planes, maps=True)
    got = run_pass(e)
    assert_equals_composition(e, got, mix, case, planes, maps=True, tag="e " + who)
    assert np.all(got["phiheat"] > 0)
    e.close()


# -- f ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "grid"])
def test_f_lls_fog(pkg, orc, otables, tables, case_a, mix_a, kind):
    """Case a's list with the fog of c2r_set_lls, as a scalar and as the REAL(4) grid: the planes fog by path / dr(1) of a line
    along z, the point sources by their own path, in the same pass."""
    grid = (10.0 ** np.random.default_rng(7).uniform(15.5, 17, ab.cells(case_a.n))).astype(np.float32) if kind == "grid" else None
    kw = dict(lls_grid=grid) if kind == "grid" else dict(coldensh_lls=2.0e16)
    mix = mx.compose(pkg, orc, otables, case_a, mx.PLANES_A, "mix_a", **kw)
    assert np.all(mix["phih_grid"] < mix_a["phih_grid"])
    e = make_engine(pkg, tables, case_a, mx.PLANES_A, maps=True, **kw)
    assert_equals_composition(e, run_pass(e), mix, case_a, mx.PLANES_A, maps=True, tag="f " + kind)
    e.close()


# -- g ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case_g(pkg):
    return mx.make_case(pkg, "z", ab.E_SOURCES[:3], mx.FLUX_E[:3])


def test_g_do_source_runs_the_second_plane_alone(pkg, orc, otables, tables, case_g):
    """c2r_do_source(NumSrc + 2): plane 2 only, equal to its reference alone; plane 1 has not run."""
    alone = mx.plane_alone(orc, otables, case_g, mx.PLANES_A[1])
    e = make_engine(pkg, tables, case_g, mx.PLANES_A)
    e.begin_step()
    e.set_rates_to_zero()
    e.do_source(5)
    got = e.download_rates()
    for k in ("phih_grid", "phihe_grid"):
        assert np.array_equal(got[k], alone[k]), k
    assert got["sum_nbox"] == 0 and np.array_equal(e.plane_exit_columns(2), alone["exit"])
    assert rel_err(e.plane_loss(2), alone["loss"]) <= 1e-13 and got["photon_loss"][0] == e.plane_loss(2) > 0
    assert e.plane_loss(1) == 0.0 and not e.plane_exit_columns(1).any()
    e.close()


@pytest.mark.parametrize("first", [1, 2])
def test_g_the_deal_gives_the_planes_to_different_callers(pkg, orc, otables, tables, case_g, first):
    """Three point sources and two planes dealt over two callers on one device: c2r_pass_sources(1, 2) holds sources 1 and 3
    and plane 2, c2r_pass_sources(2, 2) source 2 and plane 1.  Each caller's grids, maps and losses are the composition over
    its own share; the plane a caller did not run has, on a context that never ran it, a loss of 0.0 and exit columns of 0.0."""
    mix = mx.compose(pkg, orc, otables, case_g, mx.PLANES_A, "mix_g", first=first, stride=2)
    assert (mix["sources"], mix["planes"]) == (([1, 3], [2]) if first == 1 else ([2], [1]))
    e = make_engine(pkg, tables, case_g, mx.PLANES_A, maps=True)
    got = run_pass(e, first=first, stride=2)
    assert_equals_composition(e, got, mix, case_g, mx.PLANES_A, maps=True, tag=f"g caller {first}")
    other = 3 - mix["planes"][0]
    assert e.plane_loss(other) == 0.0 and not e.plane_exit_columns(other).any()
    e.close()


# -- h ---------------------------------------------------------------------------------------------------------------------
def test_h_whole_evolve3d(pkg, orc, otables, tables):
    """Two planes and two point sources: c2r_evolve3d equals the loop of the single-purpose calls -- same iteration count,
    same flags, state bit for bit --, the criterion counts the planes as sources, and the first iteration's rates are the
    composition.  (24,24,24), z open: the smallest mesh of this file on which convergence_fraction * ncell, 3 here, is no
    longer 0 -- and with NumSrc = 2 it is the two planes that keep the criterion at 3 instead of 2."""
    case = mx.make_case(pkg, "z", [(7, 13, 12), (20, 5, 3)], mx.FLUX_E[2:], mesh=((24, 24, 24), (24, 24, 48)))
    dt = 1.0e5 * 3.15576e7
    mat = pkg.Material(case.region[0], None, None)
    e = make_engine(pkg, tables, case, mx.PLANES_A)
    niter, flags = e.evolve3d(dt)
    e.download_state(mat)
    whole = (mat.xh.copy(), mat.xhe.copy())
    e.close()
    mix = mx.compose(pkg, orc, otables, case, mx.PLANES_A, "mix_h", with_maps=False)
    e = make_engine(pkg, tables, case, mx.PLANES_A)
    criterion = min(int(float(orc.constants()[31]) * ab.cells(case.n)), len(case.flux) + e.plane_count)
    e.begin_step()
    n, conv, seen = 0, ab.cells(case.n), []
    while True:
        if conv < criterion and n > 1:
            e.end_step()
            break
        if n > 500:
            break
        n += 1
        e.set_rates_to_zero()
        e.pass_sources(1, 1)
        if n == 1:
            assert_equals_composition(e, e.download_rates(), mix, case, mx.PLANES_A, tag="h")
        conv = e.global_pass(dt)
        seen.append(conv)
    e.download_state(mat)
    e.close()
    print("iterations", niter, "flags", flags, "criterion", criterion)
    assert len(case.flux) == 2 and criterion == 3 and 2 <= niter < 500 and seen[-1] < criterion <= min(seen[1:-1] + [criterion])
    assert (n, seen) == (niter, flags)
    assert np.array_equal(mat.xh, whole[0]) and np.array_equal(mat.xhe, whole[1])
    assert not np.array_equal(mat.xh, case.region[1])


# -- j ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 256])
def test_j_planes_with_point_sources_that_need_several_rounds(pkg, orc, otables, tables, batch):
    """(11,24,24), x and z open, ionised gas (axis_boundary_cases.case_d): every point source runs to its reach, three rounds from
    a corner, 11 in all, on top of a plain plane along z and a tilted one along x; one source per batch and all in one."""
    case = mx.case_j(pkg)
    mix = mx.compose(pkg, orc, otables, case, mx.PLANES_J, "mix_j")
    assert mix["sum_nbox"] == case.expected_rounds() == 11 and mix["nbox"] == [3, 3, 3, 3]
    e = make_engine(pkg, tables, case, mx.PLANES_J, maps=True, batch=batch)
    assert_equals_composition(e, run_pass(e), mix, case, mx.PLANES_J, maps=True, tag=f"j batch {batch}")
    e.close()


# -- i ---------------------------------------------------------------------------------------------------------------------
def _draw(rng):
    """One random case: the mask, 1 to 4 planes on open axes, 0 to 4 point sources anywhere, the switches."""
    mask = str(rng.choice(["z", "xy", "xz", "xyz"]))
    n, _ = mx.MESHES[mask]
    heat, multi = bool(rng.random() < 0.4), bool(rng.random() < 0.3)
    cs = dict(mask=mask, heat=heat, multi=multi, seed=int(rng.integers(1 << 30)), batch=int(rng.integers(1, 9)), lls=int(rng.integers(0, 3)),
              route=str(rng.choice(ROUTES)), maps=bool(rng.random() < 0.5))
    open_axes = ["xyz".index(ch) for ch in mask]
    shape = SimpleCase(n)
    planes = []
    for k in range(int(rng.integers(1, 5))):
        axis = int(rng.choice(open_axes))
        flux = [mx.FLUX * float(10.0 ** rng.uniform(-0.5, 0.5)), 0.0, 0.0]
        if multi:
            flux[1:] = [mx.FLUX * float(rng.uniform(0.1, 1.0)) * float(rng.random() < 0.6) for _ in range(2)]
            flux[0] *= float(rng.random() < 0.8)
        pl = dict(axis=axis, from_high=int(rng.integers(0, 2)), normflux=flux)
        if rng.random() < 0.4:                           # the beam moves a_f and a_g <= 0.95 cells sideways per layer
            f, g = pr.face_axes(axis)
            a = [float(rng.uniform(0.05, 0.95)) * float(rng.choice([-1.0, 1.0])) for _ in range(2)]
            if rng.random() < 0.2:
                a[int(rng.integers(0, 2))] = 0.0
            pl["tilt"] = (a[0] * mx.DR_FACTORS[f] / mx.DR_FACTORS[axis], a[1] * mx.DR_FACTORS[g] / mx.DR_FACTORS[axis])
            if pl["tilt"] == (0.0, 0.0):
                del pl["tilt"]
        if rng.random() < 0.4:
            pl["fmap"] = mx.make_map(shape, axis, int(rng.integers(1 << 30)), seds=3 if multi else 1, scale=float(rng.uniform(0.5, 1.5)))
        planes.append(pl)
    erng = np.random.default_rng(cs["seed"] + 11)       # entry columns, from a stream of their own
    for k, pl in enumerate(planes):
        if erng.random() < 0.3:
            pl["entry"] = mx.make_entry(shape, pl["axis"], cs["seed"] + 20 + k)
    nsrc = int(rng.integers(0, 5))
    srcpos = np.stack([rng.integers(1, nd + 1, size=nsrc) for nd in n], axis=1).astype(np.int32).reshape(-1, 3)
    if nsrc > 1 and rng.random() < 0.3:
        srcpos[1] = srcpos[0]                            # two sources in one cell
    if nsrc > 0 and rng.random() < 0.4:
        srcpos[0] = [(1, nd)[int(rng.integers(0, 2))] for nd in n]      # a corner
    flux = 10.0 ** rng.uniform(6.5, 7.5, nsrc)
    pl_ = qpl = None
    if multi and nsrc > 0:
        pl_ = np.where(rng.random(nsrc) < 0.6, 10.0 ** rng.uniform(5.5, 6.5, nsrc), 0.0)
        qpl = np.where(rng.random(nsrc) < 0.6, 10.0 ** rng.uniform(5.5, 6.5, nsrc), 0.0)
    lrng = np.random.default_rng(cs["seed"] + 7)
    cs["lls_kw"] = {} if cs["lls"] == 0 else (dict(coldensh_lls=float(10.0 ** lrng.uniform(15, 17))) if cs["lls"] == 1 else
                                              dict(lls_grid=(10.0 ** lrng.uniform(15.5, 17, ab.cells(n))).astype(np.float32)))
    cs.update(planes=planes, srcpos=srcpos, flux=flux, pl=pl_, qpl=qpl)
    return cs


class SimpleCase:
    """What mix_reference.make_map reads of a case: the mesh."""
    def __init__(self, n):
        self.n = n


def build_case(pkg, cs):
    return mx.make_case(pkg, cs["mask"], cs["srcpos"], cs["flux"], heat=cs["heat"], pl=cs["pl"], qpl=cs["qpl"], seed=cs["seed"])


def random_cases(pkg, orc, otables3, ncases, seed):
    """The seeded list, and how many drawn cases the embedding ruled out: a case is redrawn, before any GPU work, when
    mix_reference.same_cells fails for one of its point sources.  Every tilt is within one cell per layer
    by construction, asserted from oblique_reference.geometry.  At most a quarter of the drawn cases may be redrawn."""
    rng = np.random.default_rng(seed)
    kept, redrawn = [], 0
    while len(kept) < ncases:
        cs = _draw(rng)
        case = build_case(pkg, cs)
        for p in cs["planes"]:
            assert not case.periodic[p["axis"]]
            if mx.plane_kind(p)[0]:
                a_f, a_g = obr.geometry(p["tilt"], case.dr, p["axis"])[:2]
                assert 0.0 <= a_f <= 1.0 and 0.0 <= a_g <= 1.0 and a_f + a_g > 0.0, (a_f, a_g)
        _, nbox, _, _ = mx.point_sources_on_top(pkg, orc, otables3, case, None, range(1, len(cs["flux"]) + 1), **cs["lls_kw"])
        if not all(mx.same_cells(case, range(1, len(cs["flux"]) + 1), nbox)):
            redrawn += 1
            assert redrawn <= ncases, "the embedding rules out every case"
            continue
        kept.append(cs)
    assert 4 * redrawn <= len(kept) + redrawn, (redrawn, len(kept))
    return kept, redrawn


NCASES = int(os.environ.get("C2R_FUZZ_CASES", str(DEFAULT_CASES)))
SEED = int(os.environ.get("C2R_FUZZ_SEED", str(DEFAULT_SEED)))


@pytest.fixture(scope="module")
def fuzz_list(pkg, orc, otables3):
    return random_cases(pkg, orc, otables3, NCASES, SEED)[0]


@pytest.mark.parametrize("ic", range(NCASES))
def test_i_a_seeded_random_list(pkg, orc, otables3, tables3, fuzz_list, ic):
    """A seeded random list of planes and point sources (C2R_FUZZ_CASES / C2R_FUZZ_SEED widen or move it): the mask from
    {z, xy, xz, xyz}, 1 to 4 planes on open axes, each with its own chance of a tilt and of a map, 0 to 4 point sources
    anywhere, entry columns on some planes, any batch, heating, three SEDs, the fog as a scalar or a grid, the route and the escape maps drawn too."""
    cs = fuzz_list[ic]
    case = build_case(pkg, cs)
    tag = f"case {ic}: " + str({k: cs[k] for k in ("mask", "heat", "multi", "seed", "batch", "lls", "route", "maps")}) + \
          f" planes {[(p['axis'], p['from_high'], mx.plane_kind(p)) for p in cs['planes']]} sources {cs['srcpos'].tolist()}"
    print(tag)
    mix = mx.compose(pkg, orc, otables3, case, cs["planes"], f"fuzz_{SEED}_{ic}", **cs["lls_kw"])
    e = make_engine(pkg, tables3, case, cs["planes"], maps=cs["maps"], batch=cs["batch"], **cs["lls_kw"])
    got = run_pass(e, cs["route"])
    assert_equals_composition(e, got, mix, case, cs["planes"], maps=cs["maps"], tag=f"case {ic}")
    e.close()
