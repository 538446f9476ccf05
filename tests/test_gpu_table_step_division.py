"""The rates kernels with the table position's division by the table step done in two roundings (csrc/c2ray_device.hpp:
div_by_table_step; tests/test_table_step_division_host.py proves the constant).  One 16^3 periodic state, three sources,
rate grids, photon loss and the sub-box count compared with the oracle behind tests/oracle_engine.py by
numpy.array_equal, once with all three sources in one launch and once with a launch per source, isothermal and with
heating (the heating kernel and its tables share the position).

The state is that of tests/test_gpu_rates_logfold.py -- neutral fractions log-uniform over seven decades, the sources'
4 x 4 x 4 cube (one wave) with thin planes, cells of 4e10 times the density -- with four additions:
 - the thin planes' fractions are drawn log-uniform from [1e-12, 1e-9] where that state has 1e-12, so that their depths
   lie on both sides of the clamp at 1e-20, within a factor of two of it, and in the tables' first row above it;
 - a slab of 32 fully neutral cells of 10 to 300 times the density, whose depths run through the tables' last rows;
 - a cell of 4e10 times the density inside the sources' cube, beside its thin cells;
 - the surface planes of the three sources' boxes at that density too, but for one cell per source (_walls): the kept
   loss, one sum in the implementation's own order, then has one non-zero term per source and is the same number in any
   order -- asserted on the oracle, whose two orders of summation must agree for eight thread counts -- so that it can
   be compared bit for bit like the grids.
What is asserted of it on the CPU, from the oracle's outgoing columns of the last source run alone (a cell counts where
that source's rate is positive: its positions were formed), per band:
 - depths in [0.5e-20, 1e-20) and in [1e-20, 2e-20);
 - a depth above the clamp whose position lies in row 1, and one in row 2;
 - positions in rows NumTau - 1 and NumTau (the latter from a depth below 1e4), and depths beyond 1e4;
 - one wave with a depth below 2e-20 beside a depth beyond 1e4 (the dense cell: its rates are positive, so it was done);
 - one wave that holds the source cell."""
import numpy as np
import pytest

from oracle_engine import OracleEngine

pytestmark = pytest.mark.gpu

N = 16
ZRED = 9.0
NTAU = 2000
DLOGTAU = float(np.float64(24.0) / np.float64(np.float32(NTAU)))
SRCPOS = np.array([[3, 14, 4], [4, 16, 1], [2, 15, 2]], dtype=np.int32)   # 1-based (i, j, k): one cube, near three mesh faces
CUBE_LAST = (slice(0, 4), slice(12, 16), slice(0, 4))                     # [k, j, i] of the sources' 4 x 4 x 4 cube
DENSE = [(13, 9, 3), (3, 12, 0)]                                          # [k, j, i]; the last one in the sources' cube
SLAB = (5, slice(8, 12), slice(0, 8))                                     # [k, j, i] of the 32 thick cells
REACH_L, REACH_R = N // 2, N // 2 - 1                                     # a source's box: src - 8 .. src + 7 on every axis
WINDOWS = [(3, 5, 4), (4, 8, 1), (9, 15, 2)]                              # 1-based (i, j, k), one per source: see _walls


def _walls():
    """[k, j, i] mask of the cells of 4e10 times the density that make the kept loss a sum of ONE non-zero term per source.
    The loss of a source adds photo_out * vol / vol_ph over the surface cells of its final box (evolve_point.F90:310-315),
    here the 1352 cells with a coordinate at src - 8 or src + 7 (mod 16), in sweep order by the oracle and in block order
    by the device; the oracle's own two orders of that sum differ in the last bits on every state that was tried, so a
    comparison bit for bit needs a sum that no order can change.  Every such plane of every source is made opaque --
    photo_out is exactly 0.0 behind a depth of 1e12, and a cell whose incoming column exceeds max_coldensh adds 0.0 --
    except one cell per source, straight along an axis from it with ordinary cells in between and on no other source's
    surface: x + 0.0 + ... + 0.0 is x in any order, and the three sources' losses are added source by source by both."""
    wall = np.zeros((N, N, N), dtype=bool)
    for src in SRCPOS:
        for axis, c in enumerate(src):                        # axis 0 = i (last index of [k, j, i])
            for plane in ((c - REACH_L - 1) % N, (c + REACH_R - 1) % N):
                wall[(slice(None),) * (2 - axis) + (plane,)] = True
    for (i, j, k), src in zip(WINDOWS, SRCPOS):
        assert wall[k - 1, j - 1, i - 1] and np.count_nonzero(np.array([i, j, k]) != src) == 1
        wall[k - 1, j - 1, i - 1] = False
    return wall


def _inputs(hp):
    """(ndens, xh, xhe, dr, vol), Fortran layout (first axis fastest)."""
    nc = N ** 3
    dr, vol = hp.test_grid(N, ZRED)
    rng = np.random.default_rng(20261020)
    x_HI, x_HeI, x_HeII = (10.0 ** rng.uniform(-9.0, -2.0, (N, N, N)) for _ in range(3))
    ndens = np.full((N, N, N), hp.test_density(ZRED))
    k0, j0, i0 = CUBE_LAST
    thin = (k0, j0, slice(i0.start + 1, i0.stop, 2))          # i = 1 and 3 (0-based): two of the sources sit there
    for x in (x_HI, x_HeI, x_HeII):
        x[k0, j0, i0] = 1.0e-10
        x[thin] = 10.0 ** rng.uniform(-12.0, -9.0, x[thin].shape)
    ndens[thin] *= 1.0e-12
    ndens[SLAB] *= 10.0 ** rng.uniform(1.0, 2.5, ndens[SLAB].shape)
    x_HI[SLAB], x_HeI[SLAB], x_HeII[SLAB] = 1.0, 1.0, 0.0
    wall = _walls()
    assert not wall[CUBE_LAST].any() and not wall[SLAB].any()
    for c in DENSE:
        wall[c] = True
    ndens[wall] = hp.test_density(ZRED) * 4.0e10
    x_HI[wall], x_HeI[wall], x_HeII[wall] = 1.0, 1.0, 0.0
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


def _assert_inputs_do_their_job(t, colh_out, colhe_out, phih):
    nc = N ** 3
    nb = int(t.bb_upper)
    sig = np.stack([t.sigma_HI, t.sigma_HeI, t.sigma_HeII])[:, :nb]                   # [species, band]
    cols = np.stack([colh_out, colhe_out[:nc], colhe_out[nc:2 * nc]])
    tau = np.einsum("sb,sc->cb", sig, cols)                                            # [cell, band], the last source
    done = (phih > 0.0)[:, None] & (tau > 0.0)                                         # cells whose positions were formed
    odpos = np.minimum(float(NTAU), 1.0 + (np.log10(np.maximum(tau, 1.0e-20)) + 20.0) / DLOGTAU)
    row = np.where(done, odpos.astype(np.int64), -1)
    assert (done & (tau >= 0.5e-20) & (tau < 1.0e-20)).any() and (done & (tau >= 1.0e-20) & (tau < 2.0e-20)).any(), \
        "no depths within a factor of two of the clamp on both of its sides"
    assert ((row == 1) & (tau > 1.0e-20)).any() and (row == 2).any(), "no position in rows 1 and 2 above the clamp"
    assert (row == NTAU - 1).any(), "no position in row NumTau - 1"
    assert ((row == NTAU) & (tau < 1.0e4)).any(), "no position in row NumTau from a depth below 1e4"
    assert (done & (tau > 1.0e4)).any(), "no depth beyond the tables"
    thin, thick = _cubes(done & (tau < 2.0e-20)).any(axis=(1, 2)), _cubes(done & (tau > 1.0e4)).any(axis=(1, 2))
    assert (thin & thick).any(), "no wave with a thin and a thick cell"
    cube = np.zeros((N, N, N), dtype=bool)
    cube[CUBE_LAST] = True
    k, j, i = SRCPOS[-1, 2] - 1, SRCPOS[-1, 1] - 1, SRCPOS[-1, 0] - 1
    assert cube[k, j, i] and done.reshape(N, N, N, nb)[k, j, i].any(), "the source cell is not in the cube"


def _reference(pkg, orc, otables, isothermal):
    """(run, the oracle's results, the names of the grids to compare); the inputs checked on the way"""
    hp = pkg.hostphys
    ndens, xh, xhe, dr, vol = _inputs(hp)
    t = pkg.RadiationTables.load()
    assert t.heat_thick is not None and t.heat_thin is not None        # the fixture set has heating tables
    temp = None if isothermal else np.full(3 * N ** 3, 1.0e4, dtype=np.float32)
    mat = pkg.Material(ndens, xh, xhe, temp, isothermal, 1.0e4, 1.0, hp.reccoef(1.0e4))
    grid = pkg.GridProps((N, N, N), dr, vol)
    flux = np.array([3.0e6, 1.0e5, 2.0e7])
    cosmo = pkg.Cosmology(ZRED, hp.H0, hp.Omega0)
    grids = ("phih_grid", "phihe_grid") if isothermal else ("phih_grid", "phihe_grid", "phiheat")

    def run(e, batch=None, last_only=False):
        e.set_tables(t)
        e.set_step(mat, grid, cosmo)
        e.set_sources(pkg.SourceProps(SRCPOS[-1:], flux[-1:], 1.0e48) if last_only else pkg.SourceProps(SRCPOS, flux, 1.0e48))
        if batch is not None:
            e.set_batch(batch)
        e.upload_state(mat)
        e.begin_step()
        e.set_rates_to_zero()
        e.pass_sources(1, 1)
        return e.download_rates()

    # the last source alone: its columns and the cells it reached
    alone = OracleEngine((N, N, N), otables)
    reached = run(alone, last_only=True)["phih_grid"]
    _assert_inputs_do_their_job(t, alone.s.coldensh_out, alone.s.coldenshe_out, reached)
    whole = OracleEngine((N, N, N), otables)
    ref = run(whole)
    # the kept loss is the same number in whatever order its terms are added (_walls): the oracle's second order, per-thread
    # partial sums over shells, gives the bits of its sweep order for every number of threads
    for nthreads in (1, 2, 3, 4, 5, 7, 8, 16):
        orc.begin_step(whole.s)
        orc.pass_all_sources_shells(otables, whole.st, whole.s, nthreads)
        assert whole.s.photon_loss[0] == ref["photon_loss"][0], (nthreads, float(whole.s.photon_loss[0]).hex())
    for k in grids:
        assert np.isfinite(ref[k]).all() and (ref[k] > 0).any(), k
        ref[k].setflags(write=False)
    assert ref["photon_loss"][0] > 0
    ref["photon_loss"].setflags(write=False)
    return run, ref, grids


@pytest.fixture(scope="module", params=[True, False], ids=["isothermal", "heating"])
def case(request, pkg, orc, otables):
    return _reference(pkg, orc, otables, request.param)


@pytest.fixture(scope="module", params=[1, 3], ids=["a-launch-per-source", "one-launch"])
def results(request, pkg, case):
    run, ref, grids = case
    e = pkg.HipEngine((N, N, N), 0)
    try:
        got = run(e, request.param)
    finally:
        e.close()
    return got, ref, grids


def test_rates_loss_and_box_count_bit_for_bit_with_the_two_rounding_position(results):
    got, ref, grids = results
    for k in grids:
        print(k, "cells that differ:", int((got[k] != ref[k]).sum()), "of", got[k].size)
    print("photon_loss", float(got["photon_loss"][0]).hex(), "oracle", float(ref["photon_loss"][0]).hex())
    print("sum_nbox", got["sum_nbox"], "oracle", ref["sum_nbox"])
    assert got["sum_nbox"] == ref["sum_nbox"]
    for k in grids:
        assert np.array_equal(got[k], ref[k]), (k, int((got[k] != ref[k]).sum()))
    assert np.array_equal(got["photon_loss"], ref["photon_loss"])
