"""Plane-parallel sources on the CPU.

1. The premise of tests/plane_reference.py, on the oracle alone: a plane wave marched cell by cell with the oracle's
   photoion_rates and vol_ph = dr[axis] neither makes nor loses photons -- what the cells absorb plus what leaves the last
   one is what entered.
2. The product's per-cell rule (csrc/c2ray_plane.hpp) and its cell map, compiled for the host (tests/plane_harness.cpp)
   and marched over a whole mesh the way the three device kernels do, against that reference: every rate grid, the exit
   columns and every column's loss term bit for bit.
3. The notes of the gfx950 code object: which plane kernels the library holds, and that they keep nothing in scratch memory.
"""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import plane_reference as pr
from code_object import READELF, kernel_notes

ROOT = Path(__file__).resolve().parent.parent
ZRED = 9.0
dp = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(dp)


def slab_gas(pkg, n, seed, heat=False):
    """Log-normal density and mixed ionisation: ndens (n), xh_av (2n), xhe_av (3n)."""
    rng = np.random.default_rng(seed)
    ndens = pkg.hostphys.test_density(ZRED) * np.exp(rng.normal(0.0, 0.7, n))
    x = 10.0 ** rng.uniform(-6, -0.3, n)
    return ndens, np.concatenate([1.0 - x, x]), np.concatenate([1.0 - x, 0.8 * x, 0.2 * x])


# total HI optical depth at the threshold of the 16-cell march, and the ionised fraction of its gas
@pytest.mark.parametrize("tau_HI,ionised", [(2.0e2, 1.0e-4), (2.0e3, 0.5), (2.0e4, 1.0e-4)])
def test_a_march_conserves_photons(orc, otables, pkg, tau_HI, ionised):
    """Isothermal, entry columns 0: sum over cells of (photo_HI + photo_HeI + photo_HeII) * dr[a], plus photo_out of the last
    cell, equals photo_out at zero columns -- the photons that enter -- to 1e-12 relative.  (Not so with heating, where
    secondary ionisations add to the rates.)"""
    ncell, flux = 16, 3.0e6
    (dr, _, _), vol = pkg.hostphys.test_grid(16, ZRED)
    sigma = float(orc.constants()[19])
    abu_he, _ = pr.constants(orc)
    rng = np.random.default_rng(11)
    shape = np.exp(rng.normal(0.0, 0.5, ncell))
    ndens = shape * tau_HI / (sigma * dr * (1.0 - abu_he) * (1.0 - ionised) * shape.sum())
    x = np.full(ncell, ionised)
    ref = pr.plane_pass(orc, otables, (1, 1, ncell), (dr, dr, dr), vol, ndens, np.concatenate([1.0 - x, x]),
                        np.concatenate([1.0 - x, 0.8 * x, 0.2 * x]), 2, 0, flux)
    _, eps = pr.constants(orc)
    # the rates are divided by neufrac * ndens * abundance: undo it
    u = [np.maximum(1.0 - x, eps) * ndens * (1.0 - abu_he), np.maximum(1.0 - x, eps) * ndens * abu_he, np.maximum(0.8 * x, eps) * ndens * abu_he]
    absorbed = (ref["phih_grid"] * u[0] + ref["phihe_grid"][:ncell] * u[1] + ref["phihe_grid"][ncell:] * u[2]) * dr
    left = ref["terms"][0] * dr / vol
    entered = orc.photoion_rates(otables, [0.0] * 6, dr, flux, 1.0e-4, True)[20]
    total = float(np.sum(absorbed)) + left
    print("tau_HI", tau_HI, "entered", entered, "absorbed + left", total, "rel", abs(total - entered) / entered, "left / entered", left / entered)
    assert entered > 0 and abs(total - entered) <= 1e-12 * entered


@pytest.fixture(scope="module")
def ph(pkg):
    so = ROOT / "tests" / "_plane_harness.so"
    src = ROOT / "tests" / "plane_harness.cpp"
    hdrs = list((ROOT / "c2-ray3dm1d_helium_amd" / "csrc").glob("*.hpp"))
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in [src] + hdrs):
        r = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(src)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            pytest.fail("tests/plane_harness.cpp does not compile against csrc/c2ray_plane.hpp:\n" + r.stderr[-2000:])
    lib = C.CDLL(str(so))
    t = pkg.RadiationTables.load()
    keep = [t.fvec[k] for k in pkg.evolve.FVEC_ORDER]
    fv = (dp * 12)(*[_p(a) for a in keep])
    lib.ph_set_tables(_p(t.photo_thick), _p(t.photo_thin), _p(t.heat_thick), _p(t.heat_thin), _p(t.sigma_HI), _p(t.sigma_HeI),
                      _p(t.sigma_HeII), fv, C.c_int(t.bb_upper))
    lib._keep = (t, keep)
    return lib


MESH = (6, 5, 7)


@pytest.fixture(scope="module")
def slab(pkg):
    n = int(np.prod(MESH))
    (dr, _, _), vol = pkg.hostphys.test_grid(24, ZRED)
    # cells that are no cubes: the path, the fog and vol_ph each pick their own dr
    return slab_gas(pkg, n, 2024), (dr, 1.25 * dr, 0.75 * dr), vol


def harness_march(ph, slab, axis, from_high, flux, heat, coldensh_lls=None, lls_grid=None, entry=None):
    (ndens, xh_av, xhe_av), dr, vol = slab
    n = ndens.size
    face = pr.face_cells(MESH, axis)
    rates, exit3, terms = np.zeros(4 * n), np.zeros(3 * face), np.zeros(face)
    mesh = (C.c_int * 3)(*MESH)
    drv = (C.c_double * 3)(*dr)
    lls = None if lls_grid is None else np.ascontiguousarray(lls_grid, dtype=np.float32)
    use_lls = coldensh_lls is not None or lls is not None
    rc = ph.ph_march(mesh, drv, C.c_double(vol), _p(ndens), _p(xh_av), _p(xhe_av), axis, from_high, C.c_double(flux), int(heat),
                     int(use_lls), C.c_double(coldensh_lls or 0.0), None if lls is None else lls.ctypes.data_as(C.POINTER(C.c_float)),
                     None if entry is None else _p(entry), _p(rates), _p(exit3), _p(terms))
    assert rc == 0, f"the cell map of plane_geometry / plane_cell missed or repeated {rc - 1} cells"
    return dict(phih_grid=rates[:n], phihe_grid=rates[n:3 * n], phiheat=rates[3 * n:], exit=exit3, terms=terms)


@pytest.mark.parametrize("heat", [False, True])
@pytest.mark.parametrize("lls", [None, 2.0e16])
@pytest.mark.parametrize("axis,from_high", [(a, s) for a in range(3) for s in (0, 1)])
def test_the_per_cell_rule_marched_over_a_mesh_equals_the_reference(ph, orc, otables, slab, axis, from_high, lls, heat):
    """(6,5,7) cells, all six (axis, side) pairs, isothermal and heating, uniform LLS fog on and off: rates, exit columns and
    per-column loss terms of the product's functions equal the Python reference bit for bit."""
    (ndens, xh_av, xhe_av), dr, vol = slab
    flux = 4.0e5
    ref = pr.plane_pass(orc, otables, MESH, dr, vol, ndens, xh_av, xhe_av, axis, from_high, flux, heat=heat, coldensh_lls=lls)
    got = harness_march(ph, slab, axis, from_high, flux, heat, coldensh_lls=lls)
    for k in ("phih_grid", "phihe_grid", "phiheat", "exit", "terms"):
        assert np.array_equal(got[k], ref[k]), (k, int(np.count_nonzero(got[k] != ref[k])))
    assert np.all(ref["phih_grid"] > 0) and np.all(ref["terms"] > 0) and np.all(ref["exit"] > 0)
    assert np.all(ref["phiheat"] > 0) if heat else not ref["phiheat"].any()


def test_entry_columns_and_a_fog_grid(ph, orc, otables, slab):
    """The same with entry columns and a per-cell LLS grid (REAL(4)), heating, from the high side of y."""
    (ndens, xh_av, xhe_av), dr, vol = slab
    rng = np.random.default_rng(5)
    face = pr.face_cells(MESH, 1)
    entry = np.concatenate([10.0 ** rng.uniform(15, 17, face), 10.0 ** rng.uniform(14, 16, face), 10.0 ** rng.uniform(12, 15, face)])
    grid = (10.0 ** rng.uniform(15, 17, ndens.size)).astype(np.float32)
    ref = pr.plane_pass(orc, otables, MESH, dr, vol, ndens, xh_av, xhe_av, 1, 1, 4.0e5, heat=True, lls_grid=grid, entry=entry)
    got = harness_march(ph, slab, 1, 1, 4.0e5, True, lls_grid=grid, entry=entry)
    for k in ("phih_grid", "phihe_grid", "phiheat", "exit", "terms"):
        assert np.array_equal(got[k], ref[k]), k
    plain = pr.plane_pass(orc, otables, MESH, dr, vol, ndens, xh_av, xhe_av, 1, 1, 4.0e5, heat=True)
    assert np.all(ref["phih_grid"] < plain["phih_grid"])


def test_plane_kernels_keep_nothing_in_scratch_memory(pkg):
    """The gfx950 code object inside the built library (no device needed): k_plane_columns, the two k_plane_layer, the eight
    k_plane_exit and the six isothermal k_plane_rates instantiations have no private segment; the six heating k_plane_rates
    exist and are reported."""
    if not Path(READELF).exists():
        pytest.skip("llvm-readelf not present")
    seg = {name: v["private_segment"] for name, v in kernel_notes(pkg.build()).items() if "k_plane_" in name}
    print(seg)
    count = lambda pattern: len([n for n in seg if re.search(pattern, n)])
    assert count(r"15k_plane_columnsE") == 1 and count(r"13k_plane_layerILb[01]EE") == 2, sorted(seg)
    assert count(r"12k_plane_exitILb[01]ELb[01]ELb[01]EE") == 8, sorted(seg)
    cold = [n for n in seg if re.search(r"k_plane_columns|k_plane_layer|k_plane_exit|k_plane_ratesILb0E", n)]
    heating = [n for n in seg if re.search(r"k_plane_ratesILb1E", n)]
    assert len(cold) == 1 + 2 + 8 + 6 and len(heating) == 6 and len(seg) == 23, sorted(seg)
    assert {n: seg[n] for n in cold if seg[n]} == {}
    print("private segment of the heating instantiations:", {n: seg[n] for n in heating})
