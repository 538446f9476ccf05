"""The all-periodic isothermal one-SED rates kernel with its folded log table (gm::LogFold: the reciprocal carries the case's
power of two) and its one-subtraction split (hx by a select -- one v_cmp and one v_cndmask_b32 on the device --, the exponent
table's byte offset from hi - hx).  One 16^3 periodic state, three sources, rate grids and photon loss compared with the
oracle behind tests/oracle_engine.py by numpy.array_equal, once with all three sources in one launch and once with a launch
per source.  16^3 is the smallest mesh on which a 4 x 4 x 4 cube (one wave) holds a source cell, a wrapped offset and a
surface cell of the sources' boxes at once.

The state is that of tests/test_gpu_rates_parked.py -- neutral fractions log-uniform over seven decades, the sources' cube
with planes of 1e-12 of the density (depths below the clamp at 1e-20), two cells of 4e10 times the density (columns of
1e30) -- and what is asserted of it on the CPU, from the oracle's outgoing columns of the source it handled last, is, per
wave (cube) and band:
 - optical depths on both sides of 1.0 (the select's switch between the exponent fields of [0.5, 1) and [1, 2));
 - depths on both sides of another power of two (the exponent table's offset changes, the log table's case wraps);
 - depths on both sides, within a factor of two, of both edges of the log's near-1 window (high words 0x3FEE0000 and
   0x3FF10900: the table path beside the polynomial path);
 - exponents more than 20 binades apart;
 - depths below the clamp beside depths above it; columns of 1e30 beside ordinary ones."""
import numpy as np
import pytest

from oracle_engine import OracleEngine

pytestmark = pytest.mark.gpu

N = 16
ZRED = 9.0
ABU_HE = 0.074
SRCPOS = np.array([[3, 14, 4], [4, 16, 1], [2, 15, 2]], dtype=np.int32)   # 1-based (i, j, k): one cube, near three mesh faces
CUBE_LAST = (slice(0, 4), slice(12, 16), slice(0, 4))                     # [k, j, i] of the sources' 4 x 4 x 4 cube
DENSE = [(9, 5, 10), (13, 9, 3)]                                          # [k, j, i] of the two dense cells
NEAR1_LO = float(np.array([0x3FEE0000 << 32], dtype=np.uint64).view(np.float64)[0])   # 1 - 2^-4
NEAR1_HI = float(np.array([0x3FF10900 << 32], dtype=np.uint64).view(np.float64)[0])   # 1 + 0x1.09p-4


def _inputs(hp):
    """(ndens, xh, xhe, dr, vol), Fortran layout (first axis fastest)."""
    nc = N ** 3
    dr, vol = hp.test_grid(N, ZRED)
    rng = np.random.default_rng(20261020)
    x_HI, x_HeI, x_HeII = (10.0 ** rng.uniform(-9.0, -2.0, (N, N, N)) for _ in range(3))
    ndens = np.full((N, N, N), hp.test_density(ZRED))
    k0, j0, i0 = CUBE_LAST
    for x in (x_HI, x_HeI, x_HeII):
        x[k0, j0, i0] = 1.0e-10
        x[k0, j0, i0.start + 1:i0.stop:2] = 1.0e-12          # i = 1 and 3 (0-based): two of the sources sit there
    ndens[k0, j0, i0.start + 1:i0.stop:2] *= 1.0e-12
    for c in DENSE:
        ndens[c] *= 4.0e10
        x_HI[c], x_HeI[c], x_HeII[c] = 1.0, 1.0, 0.0
    x_HI, x_HeI, x_HeII, ndens = (a.reshape(-1) for a in (x_HI, x_HeI, x_HeII, ndens))
    xh = np.concatenate([x_HI, 1.0 - x_HI])
    xhe = np.concatenate([x_HeI, x_HeII, 1.0 - x_HeI - x_HeII])
    assert ndens.size == nc
    return ndens, xh, xhe, dr, vol


def _cubes(a):
    """[cell, ...] in mesh order -> [cube, lane, ...]"""
    rest = a.shape[1:]
    a = a.reshape(N // 4, 4, N // 4, 4, N // 4, 4, *rest)
    return np.moveaxis(a, (0, 2, 4, 1, 3, 5), (0, 1, 2, 3, 4, 5)).reshape((N // 4) ** 3, 64, *rest)


def _straddled(tau, traced, edge):
    """some wave, some band: a lane in [edge / 2, edge) beside a lane in [edge, 2 edge)"""
    below = _cubes(traced & (tau >= 0.5 * edge) & (tau < edge)).any(axis=1)
    above = _cubes(traced & (tau >= edge) & (tau < 2.0 * edge)).any(axis=1)
    return bool((below & above).any())


def _assert_inputs_do_their_job(t, ndens, xh, xhe, colh_out, colhe_out):
    nc = N ** 3
    nb = int(t.bb_upper)
    sig = np.stack([t.sigma_HI, t.sigma_HeI, t.sigma_HeII])[:, :nb]                   # [species, band]
    cols = np.stack([colh_out, colhe_out[:nc], colhe_out[nc:2 * nc]])
    tau = np.einsum("sb,sc->cb", sig, cols)                                            # [cell, band], the last source
    traced = (colh_out < 2.0e29)[:, None] & (tau > 0.0)
    assert _straddled(tau, traced, 1.0), "no wave with depths on both sides of 1.0"
    assert any(_straddled(tau, traced, 2.0 ** n) for n in (-3, -2, -1, 1, 2, 3)), "no wave straddles another power of two"
    assert _straddled(tau, traced, NEAR1_LO) and _straddled(tau, traced, NEAR1_HI), "no wave at an edge of the near-1 window"
    near = traced & (tau >= NEAR1_LO) & (tau < NEAR1_HI)
    assert (_cubes(near).any(axis=1) & _cubes(traced & ~near).any(axis=1)).any(), "no wave with both paths of the log"
    e = np.where(traced, np.floor(np.log2(np.maximum(tau, 1.0e-20))), np.nan)
    ec = _cubes(e)
    assert (np.nanmax(ec, axis=1) - np.nanmin(ec, axis=1) > 20).any(), "no wave with exponents 20 binades apart"
    last = np.zeros((N, N, N), dtype=bool)
    last[CUBE_LAST] = True
    last = last.reshape(-1)
    assert (tau[last] < 1.0e-20).any() and (tau[last] > 1.0e-20).any(), "no depths on both sides of the clamp"
    big = _cubes(colh_out[:, None] >= 1.0e30)[:, :, 0]
    small = _cubes(colh_out[:, None] < 1.0e25)[:, :, 0]
    assert (big.any(axis=1) & small.any(axis=1)).any(), "no wave with a column of 1e30 beside ordinary ones"


@pytest.fixture(scope="module")
def case(pkg, otables):
    hp = pkg.hostphys
    ndens, xh, xhe, dr, vol = _inputs(hp)
    t = pkg.RadiationTables.load()
    mat = pkg.Material(ndens, xh, xhe, None, True, 1.0e4, 1.0, hp.reccoef(1.0e4))
    grid = pkg.GridProps((N, N, N), dr, vol)
    src = pkg.SourceProps(SRCPOS, np.array([3.0e6, 1.0e5, 2.0e7]), 1.0e48)
    cosmo = pkg.Cosmology(ZRED, hp.H0, hp.Omega0)

    def run(e, batch=None):
        e.set_tables(t)
        e.set_step(mat, grid, cosmo)
        e.set_sources(src)
        if batch is not None:
            e.set_batch(batch)
        e.upload_state(mat)
        e.begin_step()
        e.set_rates_to_zero()
        e.pass_sources(1, 1)
        return e.download_rates()

    ref_engine = OracleEngine((N, N, N), otables)
    ref = run(ref_engine)
    _assert_inputs_do_their_job(t, ndens, xh, xhe, ref_engine.s.coldensh_out, ref_engine.s.coldenshe_out)
    for k in ("phih_grid", "phihe_grid"):
        assert np.isfinite(ref[k]).all() and (ref[k] > 0).any(), k
        ref[k].setflags(write=False)
    assert ref["photon_loss"][0] > 0
    ref["photon_loss"].setflags(write=False)
    return run, ref


@pytest.mark.parametrize("batch", [1, 3], ids=["a-launch-per-source", "one-launch"])
def test_rates_and_photon_loss_bit_for_bit_with_the_folded_log_table(pkg, case, batch):
    run, ref = case
    e = pkg.HipEngine((N, N, N), 0)
    try:
        got = run(e, batch)
    finally:
        e.close()
    for k in ("phih_grid", "phihe_grid"):
        print(k, "cells that differ:", int((got[k] != ref[k]).sum()), "of", got[k].size)
    print("photon_loss", float(got["photon_loss"][0]).hex(), "oracle", float(ref["photon_loss"][0]).hex())
    assert got["sum_nbox"] == ref["sum_nbox"]
    for k in ("phih_grid", "phihe_grid"):
        assert np.array_equal(got[k], ref[k]), (k, int((got[k] != ref[k]).sum()))
    assert np.array_equal(got["photon_loss"], ref["photon_loss"])
