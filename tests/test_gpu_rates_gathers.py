"""The band loop of the rates kernels where its table look-ups can go wrong: optically thin and thick bands in
neighbouring lanes of one wave, table positions clamped at NumTau, bands beyond their last non-zero table entry,
and the source cells themselves -- one 16^3 state that holds all of it, three sources (one in a mesh corner, so that
the periodic wrap is exercised), run through the isothermal and the heating kernels with one SED and with three, and
compared bit for bit with the oracle behind tests/oracle_engine.py.

The state:
 (a) everywhere the neutral fractions of H, He I and He II alternate cell by cell between 1e-12 and 1e-5 (He almost
     fully doubly ionised): in most bands the cell's own optical depth is below tau_photo_limit = 1e-7 in one cell
     and above it in its neighbour, so both branches of the look-up run in every 4 x 4 x 4 cube (one wave);
 (b) a slab of fully neutral cells at 30 times the density, three cells deep: optical depths pass 1e4, the table
     positions clamp at NumTau, both rows of an interpolation come from the duplicated last row, and the soft bands
     lie beyond the depth from which their tables hold exact zeros (BandData::tau_zero);
 (c) the three source cells, where the incoming columns are 0 and tau_in is raised to 1e-20.
That the inputs do this is asserted on the CPU before anything is compared (conditions 1-3 below), from the state, the
cross sections and the oracle's outgoing columns; the path of a ray through a cell lies in [dr/2, sqrt(3) dr]."""
from pathlib import Path

import numpy as np
import pytest

from oracle_engine import OracleEngine

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).parent / "golden"

N = 16
ZRED = 9.0
ABU_HE = 0.074            # cgsconstants: abu_he
NUMTAU, MINLOGTAU, DLOGTAU = 2000, -20.0, 0.012   # radiation_sizes.f90 / radiation_tables.f90
TAU_PHOTO_LIMIT = 1.0e-7
SLAB = slice(9, 12)       # 0-based planes of the first mesh axis
X_LO, X_HI = 1.0e-12, 1.0e-5


class _OracleEngineSeds(OracleEngine):
    """OracleEngine hands the black-body flux to the oracle; this one the power-law and quasar-like fluxes as well."""

    def upload_state(self, mat):
        import oracle as orc
        m, g, c, s = self._mat, self._grid, self._cosmo, self._src
        self.st = orc.Step(g.mesh, g.dr, g.vol, c.zred, c.H0, c.Omega0, m.isothermal, m.temper_val, m.clumping,
                           s.srcpos, s.NormFlux, s.S_star, m.ndens, m.reccoef, normflux_pl=s.NormFluxPL,
                           normflux_qpl=s.NormFluxQPL, pl_s_star=s.pl_S_star, qpl_s_star=s.qpl_S_star)
        self.s = orc.State(self.st, mat.xh, mat.xhe, mat.temperature_grid)


def _tables(pkg, orc, multi):
    t = pkg.RadiationTables.load()
    with np.load(pkg.evolve.DEFAULT_TABLES) as z:
        d = {k: z[k] for k in z.files}
    if multi:
        t.add_sed_file(GOLD / "rad_tables_pl_qpl.npz")
        with np.load(GOLD / "rad_tables_pl_qpl.npz") as z:
            d.update({k: z[k] for k in z.files})
    return t, orc.Tables(d)


def _inputs(hp):
    """The state of the module docstring: (ndens, xh, xhe, srcpos, dr, vol), Fortran layout (first axis fastest)."""
    nc = N ** 3
    dr, vol = hp.test_grid(N, ZRED)
    k, j, i = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")   # [k, j, i]: i fastest when flattened
    odd = ((i + j + k) % 2 == 1).reshape(-1)
    slab = np.zeros((N, N, N), dtype=bool)
    slab[:, :, SLAB] = True
    slab = slab.reshape(-1)
    x = np.where(odd, X_HI, X_LO)
    x_HI = np.where(slab, 1.0, x)
    x_HeI = np.where(slab, 1.0, x)
    x_HeII = np.where(slab, 0.0, x[::-1])    # the other phase of the alternation: H and He II differ within a cell
    ndens = np.full(nc, hp.test_density(ZRED)) * np.where(slab, 30.0, 1.0)
    xh = np.concatenate([x_HI, 1.0 - x_HI])
    xhe = np.concatenate([x_HeI, x_HeII, 1.0 - x_HeI - x_HeII])
    rng = np.random.default_rng(20261019)
    srcpos = rng.integers(1, N + 1, size=(3, 3)).astype(np.int32)
    srcpos[2] = (1, N, 1)                                                             # a mesh corner
    return ndens, xh, xhe, srcpos, dr, vol


def _tau_zero(cols):
    """BandData::tau_zero of one band: the depth one table step above the last non-zero row of all its columns."""
    z = 0
    for c in cols:
        nz = np.flatnonzero(c)
        z = max(z, int(nz[-1]) + 1 if nz.size else 0)
    return np.inf if z > NUMTAU else 10.0 ** (MINLOGTAU + z * DLOGTAU)


def _assert_inputs_do_their_job(t, heat, ndens, xh, xhe, dr, colh_out, colhe_out):
    nc = N ** 3
    nb = int(t.bb_upper)
    sig = np.stack([t.sigma_HI, t.sigma_HeI, t.sigma_HeII])[:, :nb]                   # [species, band]
    dens = np.stack([ndens * (1.0 - ABU_HE) * xh[:nc], ndens * ABU_HE * xhe[:nc], ndens * ABU_HE * xhe[nc:2 * nc]])
    per_cm = np.einsum("sb,sc->cb", sig, dens)                                         # optical depth per cm, [cell, band]
    dtau_min, dtau_max = per_cm * 0.5 * min(dr), per_cm * np.sqrt(3.0) * max(dr)
    # condition 1: an aligned 4 x 4 x 4 cube and a band with cells on both sides of tau_photo_limit
    thin = (dtau_max <= TAU_PHOTO_LIMIT).reshape(N // 4, 4, N // 4, 4, N // 4, 4, nb)
    thick = (dtau_min > TAU_PHOTO_LIMIT).reshape(N // 4, 4, N // 4, 4, N // 4, 4, nb)
    mixed = thin.any(axis=(1, 3, 5)) & thick.any(axis=(1, 3, 5))
    assert mixed.any(), "no cube of a wave holds both optically thin and thick cells in any band"
    # the oracle's outgoing columns (those of the source it handled last) give tau_out exactly and, less the cell's
    # own depth at its longest path, a lower bound of tau_in.  Conditions 2 and 3 are existence tests on that one
    # source and on the black-body tables and bands (which every case runs): the other sources and SEDs can only add
    # such cell.bands, never take these away
    cols = np.stack([colh_out, colhe_out[:nc], colhe_out[nc:2 * nc]])
    tau_out = np.einsum("sb,sc->cb", sig, cols)
    # condition 2: a table position clamped at NumTau
    assert (tau_out >= 1.0e4).any(), "no optical depth reaches the end of the tables"
    # condition 3: a dead band -- tau_in at or beyond the band's tau_zero
    pt, pn = t.photo_thick.reshape(-1, NUMTAU + 1), t.photo_thin.reshape(-1, NUMTAU + 1)
    tau_zero = np.empty(nb)
    for b in range(nb):
        cols_b = [pt[b], pn[b]]
        if heat:
            ns = 1 if b < 1 else (2 if b < 27 else 3)
            c0 = b if b < 1 else (2 * (b + 1) - 3 if b < 27 else 3 * (b + 1) - 26 - 2 - 3)
            ht, hn = t.heat_thick.reshape(-1, NUMTAU + 1), t.heat_thin.reshape(-1, NUMTAU + 1)
            cols_b += [ht[c0 + s] for s in range(ns)] + [hn[c0 + s] for s in range(ns)]
        tau_zero[b] = _tau_zero(cols_b)
    assert np.isfinite(tau_zero).any()
    assert ((tau_out - dtau_max) >= tau_zero[None, :]).any(), "no band of any cell lies beyond its tables' last non-zero entry"


@pytest.fixture(scope="module")
def inputs(pkg):
    return _inputs(pkg.hostphys)


@pytest.mark.parametrize("heat,multi", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["iso-1sed", "iso-3seds", "heat-1sed", "heat-3seds"])
def test_rates_bit_for_bit_where_the_gathers_differ(pkg, orc, inputs, heat, multi):
    hp = pkg.hostphys
    ndens, xh, xhe, srcpos, dr, vol = inputs
    nc = N ** 3
    t, T = _tables(pkg, orc, multi)
    temp = np.tile(np.full(nc, 1.0e4, dtype=np.float32), 3) if heat else None
    flux = np.array([3.0e6, 1.0e5, 2.0e7])
    pl = np.array([1.0e6, 0.0, 4.0e6]) if multi else None
    qpl = np.array([2.0e5, 3.0e6, 0.0]) if multi else None
    mat = pkg.Material(ndens, xh, xhe, temp, not heat, 1.0e4, 1.0, hp.reccoef(1.0e4))
    grid = pkg.GridProps((N, N, N), dr, vol)
    src = pkg.SourceProps(srcpos, flux, 1.0e48, NormFluxPL=pl, pl_S_star=1.5e48, NormFluxQPL=qpl, qpl_S_star=0.7e48)
    cosmo = pkg.Cosmology(ZRED, hp.H0, hp.Omega0)

    def run(e):
        e.set_tables(t)
        e.set_step(mat, grid, cosmo)
        e.set_sources(src)
        e.upload_state(mat)
        e.begin_step()
        e.set_rates_to_zero()
        e.pass_sources(1, 1)
        return e.download_rates()

    ref_engine = _OracleEngineSeds((N, N, N), T)
    ref = run(ref_engine)
    _assert_inputs_do_their_job(t, heat, ndens, xh, xhe, dr, ref_engine.s.coldensh_out, ref_engine.s.coldenshe_out)
    for k in ("phih_grid", "phihe_grid") + (("phiheat",) if heat else ()):
        assert np.isfinite(ref[k]).all() and (ref[k] > 0).any(), k

    e = pkg.HipEngine((N, N, N), 0)
    try:
        got = run(e)
    finally:
        e.close()
    assert got["sum_nbox"] == ref["sum_nbox"]
    for k in ("phih_grid", "phihe_grid") + (("phiheat",) if heat else ()):
        assert np.array_equal(got[k], ref[k]), (k, int((got[k] != ref[k]).sum()))
