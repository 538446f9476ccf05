"""The isothermal one-SED rates kernel where its parked values and its tabulated exponent terms can go wrong.  k_rates
keeps the cell's three denominators in LDS, one column per lane, and reads the two exponent terms of log10's tail
(y * log10_2lo, y * log10_2hi) from an LDS table indexed by the argument's power of two.  One 16^3 state, three sources,
compared bit for bit with the oracle behind tests/oracle_engine.py, once with all three sources in one launch and once
with a launch per source (the second and third launch then start from the sums in the rate grids).

The state puts into single waves (aligned 4 x 4 x 4 cubes):
 (a) neutral fractions drawn per cell, log-uniform over seven decades: neighbouring lanes index the exponent table far
     apart, a cell's two optical depths lie in different binades, and arguments within the log's near-1 interval
     [1 - 2^-4, 1 + 0x1.09p-4) stand beside arguments of its table path;
 (b) all three sources in one cube, whose planes alternate between fractions of 1e-10 and fractions of 1e-12 at 1e-12 of
     the density: optical depths below the clamp at 1e-20 beside depths above it, for every source.  (The thin planes see
     only columns of the cube itself in front of them, small enough that their own are not rounded away: a cell whose
     column vanishes in the sum has a species split of 0/0 in the reference as well.)
 (c) two cells of 4e10 times the density, fully neutral: an outgoing column of 1e30, an exponent far from those of the
     other lanes (the cells behind them are beyond max_coldensh and get nothing);
 (d) the source cells themselves: incoming columns 0, the volume of the cell as the shell volume.
That the inputs do this is asserted on the CPU, from the oracle's outgoing columns of the source it handled last,
before anything is compared."""
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
NEAR1_LO, NEAR1_HI = 1.0 - 2.0 ** -4, 1.0 + float.fromhex("0x1.09p-4")


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


def _assert_inputs_do_their_job(t, ndens, xh, xhe, dr, colh_out, colhe_out):
    nc = N ** 3
    nb = int(t.bb_upper)
    sig = np.stack([t.sigma_HI, t.sigma_HeI, t.sigma_HeII])[:, :nb]                   # [species, band]
    dens = np.stack([ndens * (1.0 - ABU_HE) * xh[:nc], ndens * ABU_HE * xhe[:nc], ndens * ABU_HE * xhe[nc:2 * nc]])
    cols = np.stack([colh_out, colhe_out[:nc], colhe_out[nc:2 * nc]])
    tau_out = np.einsum("sb,sc->cb", sig, cols)                                        # [cell, band], the last source
    dtau_min = np.einsum("sb,sc->cb", sig, dens) * 0.5 * min(dr)                       # the shortest path through a cell
    traced = (colh_out < 2.0e29)[:, None] & (tau_out > 0.0)
    # (a) a cell whose own depth is more than half its outgoing depth: tau_in < tau_out / 2, another binade
    assert (traced & (dtau_min > 0.5 * tau_out) & (tau_out > 1.0e-20)).any()
    # (a) one cube, one band: lanes whose exponents lie more than 20 binades apart
    e = np.where(traced, np.floor(np.log2(np.maximum(tau_out, 1.0e-20))), np.nan)
    ec = _cubes(e)
    assert (np.nanmax(ec, axis=1) - np.nanmin(ec, axis=1) > 20).any()
    # (a) one cube, one band: an argument of the near-1 path beside one of the table path
    near = traced & (tau_out >= NEAR1_LO) & (tau_out < NEAR1_HI)
    assert (_cubes(near).any(axis=1) & _cubes(traced & ~near).any(axis=1)).any(), "no wave with both paths of the log"
    # (b) the last source's cube: depths below the clamp beside depths above it
    last = np.zeros((N, N, N), dtype=bool)
    last[CUBE_LAST] = True
    last = last.reshape(-1)
    assert (tau_out[last] < 1.0e-20).any() and (tau_out[last] > 1.0e-20).any()
    # (c) columns of 1e30 beside ordinary ones
    big = _cubes(colh_out[:, None] >= 1.0e30)[:, :, 0]
    small = _cubes(colh_out[:, None] < 1.0e25)[:, :, 0]
    assert (big.any(axis=1) & small.any(axis=1)).any()


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
    _assert_inputs_do_their_job(t, ndens, xh, xhe, dr, ref_engine.s.coldensh_out, ref_engine.s.coldenshe_out)
    for k in ("phih_grid", "phihe_grid"):
        assert np.isfinite(ref[k]).all() and (ref[k] > 0).any(), k
        ref[k].setflags(write=False)
    return run, ref


@pytest.mark.parametrize("batch", [1, 3], ids=["a-launch-per-source", "one-launch"])
def test_rates_bit_for_bit_with_parked_values_and_tabulated_exponents(pkg, case, batch):
    run, ref = case
    e = pkg.HipEngine((N, N, N), 0)
    try:
        got = run(e, batch)
    finally:
        e.close()
    assert got["sum_nbox"] == ref["sum_nbox"]
    for k in ("phih_grid", "phihe_grid"):
        assert np.array_equal(got[k], ref[k]), (k, int((got[k] != ref[k]).sum()))
