"""Plane flux maps (c2r_set_plane_flux_map) on the CPU: the product's plane_layer_flux / plane_dark (csrc/c2ray_plane.hpp) and
the existing per-cell functions, compiled for the host (tests/flux_harness.cpp) and marched over whole meshes the way the
device kernels do, against the Python reference (tests/flux_reference.py): every rate grid, the incoming HI columns, the
exit columns, the flux of every cell, the exit flux and every line's loss term bit for bit; the loss as math.fsum of
those terms.  Then the two exact properties of the advection rule, on the reference and on the product's function alike.
"""
import ctypes as C
import math
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import flux_reference as fr
import oblique_reference as obr
import plane_reference as pr
from test_oblique_reference_host import make_slab

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
OPEN = (False, False, False)
dp = C.POINTER(C.c_double)
KEYS = ("phih_grid", "phihe_grid", "phiheat", "cin_HI", "exit", "terms", "exit_flux")
CXX = ["g++", "-O2", "-ffp-contract=off", "-mfma", "-std=c++17"]


def _p(a):
    return a.ctypes.data_as(dp)


@pytest.fixture(scope="module")
def fx(pkg, gold):
    so = ROOT / "tests" / "_flux_harness.so"
    srcs = [ROOT / "tests" / "flux_harness.cpp", ROOT / "tests" / "plane_harness.cpp"]
    hdrs = list((ROOT / "c2-ray3dm1d_helium_amd" / "csrc").glob("*.hpp"))
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in srcs + hdrs):
        r = subprocess.run(CXX + ["-fPIC", "-shared", "-o", str(so), str(srcs[0])], capture_output=True, text=True)
        if r.returncode != 0:
            pytest.fail("tests/flux_harness.cpp does not compile against csrc/c2ray_plane.hpp:\n" + r.stderr[-2000:])
    lib = C.CDLL(str(so))
    t = pkg.RadiationTables.load()
    keep = [t.fvec[k] for k in pkg.evolve.FVEC_ORDER]
    fv = (dp * 12)(*[_p(a) for a in keep])
    lib.ph_set_tables(_p(t.photo_thick), _p(t.photo_thin), _p(t.heat_thick), _p(t.heat_thin), _p(t.sigma_HI), _p(t.sigma_HeI),
                      _p(t.sigma_HeII), fv, C.c_int(t.bb_upper))
    z = gold("rad_tables_pl_qpl.npz")
    seds = []
    for idx, pre in ((1, "pl_"), (2, "qpl_")):
        a = [np.ascontiguousarray(z[pre + k]) for k in ("photo_thick", "photo_thin", "heat_thick", "heat_thin")]
        lib.fx_set_sed(idx, *[_p(x) for x in a], C.c_int(int(z[pre + "limits"][0])), C.c_int(int(z[pre + "limits"][1])))
        seds.append(a)
    lib._keep = (t, keep, seds)
    return lib


@pytest.fixture(scope="module")
def otables3(pkg, orc, gold):
    """The oracle's tables with the power-law and quasar-like SEDs of the fixture the plane tests use."""
    with np.load(pkg.evolve.DEFAULT_TABLES) as z:
        d = {k: z[k] for k in z.files}
    zz = gold("rad_tables_pl_qpl.npz")
    d.update({k: zz[k] for k in zz.files})
    return orc.Tables(d)


def harness_march(fx, slab, mesh, axis, from_high, fmap, tilt=(0.0, 0.0), periodic=OPEN, heat=False, entry=None):
    (ndens, xh_av, xhe_av), dr, vol = slab
    n = ndens.size
    face = pr.face_cells(mesh, axis)
    rates, exit3, terms, cin = np.zeros(4 * n), np.zeros(3 * face), np.zeros(face), np.zeros(n)
    cflux, fexit = np.zeros(3 * n), np.zeros(3 * face)
    fmap = np.ascontiguousarray(fmap, dtype=np.float64).reshape(-1)
    rc = fx.fx_march((C.c_int * 3)(*mesh), (C.c_double * 3)(*dr), C.c_double(vol), _p(ndens), _p(xh_av), _p(xhe_av), axis, from_high,
                     _p(fmap), (C.c_double * 2)(*tilt), (C.c_int * 3)(*[int(b) for b in periodic]), int(heat), 0, C.c_double(0.0), None,
                     None if entry is None else _p(entry), _p(rates), _p(exit3), _p(terms), _p(cin), _p(cflux), _p(fexit))
    assert rc == 0, f"fx_march returned {rc}"
    return dict(phih_grid=rates[:n], phihe_grid=rates[n:3 * n], phiheat=rates[3 * n:], exit=exit3, terms=terms, cin_HI=cin, exit_flux=fexit,
                cell_flux=cflux.reshape(n, 3))


def cell_flux_of(ref, mesh, axis, from_high):
    """The reference's layer_flux (layer, SED, face cell) as (mesh cell, SED)."""
    cells = pr.column_cells(mesh, axis, from_high)                         # [f, m]
    out = np.zeros((int(np.prod(mesh)), 3))
    for m in range(cells.shape[1]):
        out[cells[:, m]] = ref["layer_flux"][m].T
    return out


def make_map(face, seed, seds=1, lo=1.0e-41, hi=6.0e-41):
    """A random map with a block of dark cells and some isolated ones."""
    rng = np.random.default_rng(seed)
    m = np.zeros((3, face))
    m[:seds] = rng.uniform(lo, hi, (seds, face))
    m[:, face // 3: face // 3 + 5] = 0.0
    m[:, ::11] = 0.0
    return m


def compare(fx, orc, otables, slab, mesh, axis, from_high, fmap, **kw):
    (ndens, xh_av, xhe_av), dr, vol = slab
    ref = fr.flux_pass(orc, otables, mesh, dr, vol, ndens, xh_av, xhe_av, axis, from_high, fmap, **kw)
    got = harness_march(fx, slab, mesh, axis, from_high, fmap, **{k: v for k, v in kw.items() if k != "tilt" or v is not None})
    for k in KEYS:
        assert np.array_equal(got[k], ref[k]), (k, int(np.count_nonzero(got[k] != ref[k])))
    assert np.array_equal(got["cell_flux"], cell_flux_of(ref, mesh, axis, from_high))
    assert math.fsum(got["terms"]) == ref["loss"]
    return ref


@pytest.mark.parametrize("axis,from_high", [(0, 1), (1, 0), (2, 0)])
def test_normal_incidence(fx, orc, otables, pkg, axis, from_high):
    """(7,6,5), normal incidence: every cell of a line sees its map entry; dark lines add exactly nothing."""
    mesh = (7, 6, 5)
    slab = make_slab(pkg, mesh, 2026, (1.0, 1.3, 0.8))
    face = pr.face_cells(mesh, axis)
    fmap = make_map(face, 1)
    ref = compare(fx, orc, otables, slab, mesh, axis, from_high, fmap)
    dark = cell_flux_of(ref, mesh, axis, from_high)[:, 0] == 0.0
    assert dark.any() and not ref["phih_grid"][dark].any() and np.all(ref["phih_grid"][~dark] > 0)
    assert np.array_equal(ref["exit_flux"], fmap.reshape(-1)) and not ref["terms"][fmap[0] == 0.0].any()


def test_uniform_map_is_the_uniform_plane(fx, orc, otables, pkg):
    """A map whose every entry is normflux: plane_reference.plane_pass' bits, from the reference and from the harness."""
    mesh = (7, 6, 5)
    slab = make_slab(pkg, mesh, 2026, (1.0, 1.3, 0.8))
    (ndens, xh_av, xhe_av), dr, vol = slab
    face = pr.face_cells(mesh, 2)
    fmap = np.zeros((3, face))
    fmap[0] = 4.0e5
    old = pr.plane_pass(orc, otables, mesh, dr, vol, ndens, xh_av, xhe_av, 2, 0, 4.0e5)
    ref = compare(fx, orc, otables, slab, mesh, 2, 0, fmap)
    for k in ("phih_grid", "phihe_grid", "phiheat", "cin_HI", "exit", "terms"):
        assert np.array_equal(ref[k], old[k]), k
    assert ref["loss"] == old["loss"]


@pytest.mark.parametrize("periodic", [OPEN, (True, True, False), (True, False, False)])
def test_tilted_one_sed(fx, orc, otables, pkg, periodic):
    """(7,6,5) along z, tilt (0.4, -0.7), with entry columns: the flux moves with the beam, zero from outside an open side."""
    mesh = (7, 6, 5)
    slab = make_slab(pkg, mesh, 2027, (1.0, 1.3, 0.8))
    face = pr.face_cells(mesh, 2)
    rng = np.random.default_rng(5)
    entry = np.concatenate([10.0 ** rng.uniform(15, 17, face), 10.0 ** rng.uniform(14, 16, face), 10.0 ** rng.uniform(12, 15, face)])
    ref = compare(fx, orc, otables, slab, mesh, 2, 1, make_map(face, 2), tilt=(0.4, -0.7), periodic=periodic, entry=entry)
    assert ref["phih_grid"].any() and not ref["phiheat"].any()


def test_tilted_heating_three_seds(fx, orc, otables3, pkg):
    """(6,5,4), heating, black-body, power-law and quasar-like maps of their own, tilted along x from the high side and normal."""
    mesh = (6, 5, 4)
    slab = make_slab(pkg, mesh, 2028, (1.0, 1.3, 0.8))
    face = pr.face_cells(mesh, 0)
    fmap = make_map(face, 3, seds=3)
    fmap[1, 7] = 0.0                                     # a cell with two of its three SEDs
    ref = compare(fx, orc, otables3, slab, mesh, 0, 1, fmap, tilt=(0.0, 0.55), heat=True)
    assert np.any(ref["phiheat"] > 0)
    compare(fx, orc, otables3, slab, mesh, 0, 1, fmap, heat=True)


def product_layers(fx, mesh, dr, axis, tilt, periodic, fmap):
    """The flux of every layer from the product's plane_layer_flux (fx_columns over made-up gas)."""
    n = int(np.prod(mesh))
    face = pr.face_cells(mesh, axis)
    ndens, xh, xhe = np.full(n, 1.0e-4), np.concatenate([np.full(n, 0.9), np.full(n, 0.1)]), np.concatenate([np.full(n, 0.9), np.full(n, 0.08), np.full(n, 0.02)])
    cin, cflux, exit3, fexit = np.zeros(3 * n), np.zeros(3 * n), np.zeros(3 * face), np.zeros(3 * face)
    fmap = np.ascontiguousarray(fmap, dtype=np.float64).reshape(-1)
    bad = fx.fx_columns((C.c_int * 3)(*mesh), (C.c_double * 3)(*dr), _p(ndens), _p(xh), _p(xhe), axis, 0, (C.c_double * 2)(*tilt),
                        (C.c_int * 3)(*[int(b) for b in periodic]), 0, C.c_double(0.0), None, None, _p(fmap), _p(cin), _p(cflux), _p(exit3),
                        _p(fexit))
    assert bad == 0
    cells = pr.column_cells(mesh, axis, 0)
    layers = np.stack([cflux.reshape(n, 3)[cells[:, m]].T for m in range(cells.shape[1])])      # (layer, SED, face cell)
    assert np.array_equal(layers[-1].reshape(-1), fexit)
    return layers


def test_exact_conservation(fx):
    """Equal dr, tilt (0.5, 0.5): every s_i == 0.25; periodic face axes and a map of small integers -- the face sum of the flux
    of every one of the 4 layers equals the map's sum exactly (the values stay dyadic: multiples of 4^-4)."""
    mesh, dr, tilt, per = (6, 5, 4), (1.0e22, 1.0e22, 1.0e22), (0.5, 0.5), (True, True, False)
    _, _, s, _, _, _ = obr.geometry(tilt, dr, 2)
    assert s == (0.25, 0.25, 0.25, 0.25)
    fmap = np.random.default_rng(8).integers(0, 9, (3, 30)).astype(np.float64)
    ref = fr.flux_pass(None, None, mesh, dr, 1.0, None, None, None, 2, 0, fmap, tilt=tilt, periodic=per, rates=False)["layer_flux"]
    got = product_layers(fx, mesh, dr, 2, tilt, per, fmap)
    assert np.array_equal(got, ref) and ref.shape == (4, 3, 30)
    for layers in (ref, got):
        for m in range(4):
            for k in range(3):
                assert np.sum(layers[m, k]) == np.sum(fmap[k]) and math.fsum(layers[m, k]) == math.fsum(fmap[k]), (m, k)
    assert np.array_equal(ref * 256.0, np.round(ref * 256.0))
    open_ref = fr.flux_pass(None, None, mesh, dr, 1.0, None, None, None, 2, 0, fmap, tilt=tilt, periodic=OPEN, rates=False)["layer_flux"]
    assert np.sum(open_ref[-1, 0]) < np.sum(fmap[0])       # an open side face lets flux out and none in


def test_exact_shift(fx):
    """a_f == 1.0, a_g == 0.0 (the set-up of test_4_a_f_exactly_one): a one-cell spot moves exactly one cell along f per layer
    and wraps; every other cell has flux 0.0."""
    mesh, dr, tilt, per = (9, 7, 5), (1.0e22, 1.25e22, 1.0e22), (1.0, 0.0), (True, True, False)
    a_f, a_g, s, _, _, _ = obr.geometry(tilt, dr, 2)
    assert a_f == 1.0 and a_g == 0.0 and s == (0.0, 0.0, 1.0, 0.0)
    fmap = np.zeros((3, 63))
    u0, v0 = 6, 3
    fmap[:, u0 + 9 * v0] = (3.0e-41, 2.0e-41, 1.0e-41)
    ref = fr.flux_pass(None, None, mesh, dr, 1.0, None, None, None, 2, 0, fmap, tilt=tilt, periodic=per, rates=False)["layer_flux"]
    got = product_layers(fx, mesh, dr, 2, tilt, per, fmap)
    assert np.array_equal(got, ref)
    for m in range(5):
        want = np.zeros((3, 63))
        want[:, (u0 + m + 1) % 9 + 9 * v0] = fmap[:, u0 + 9 * v0]
        assert np.array_equal(ref[m], want), m
    assert (u0 + 5) % 9 < u0                              # the spot did wrap


def test_the_harness_alone_is_clean_under_host_sanitizers(tmp_path):
    """tests/flux_harness.cpp as a stand-alone program (-DFLUX_MAIN) under AddressSanitizer and UBSan: every index the marches
    form, for every face, tilt sign and wrap."""
    exe = tmp_path / "flux_main"
    r = subprocess.run(CXX + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DFLUX_MAIN", "-o", str(exe),
                              str(ROOT / "tests" / "flux_harness.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "cells missed or repeated: 0" in r.stdout
