"""The all-periodic isothermal one-SED rates kernel with its band's two table rows fetched by index-scaled buffer loads
(csrc/c2ray_device.hpp: load_rows with a band offset) and the near-1 test of its logarithms taken from the log table
(csrc/c2ray_math.hpp: gm::LogFold::lim; tests/test_log_near1_limit_host.py checks the limit on the host).  One 16^3
periodic isothermal state, three sources, rate grids, photon loss and the sub-box count compared with the oracle behind
tests/oracle_engine.py by numpy.array_equal, once with all three sources in one launch and once with a launch per source.

The state is that of tests/test_gpu_table_step_division.py -- its thin planes, dense cells, slab and walls, so that the
kept loss has one non-zero term per source and is the same number in any order, asserted on the oracle there and here --
with the three source cells tuned: a neutral fraction of a source's own cell sets its outgoing depth in one band (hydrogen
in band 0, one product; neutral helium in band 1 and ionised helium in the first band in which it absorbs, a sum of
products), and each is moved, ulp by ulp, until the depth's high word hx, scaled into [0.5, 2), lies next to an end of the
near-1 window [0x3FEE0000, 0x3FF10900) on a chosen side (TARGETS).  The incoming depth of a source cell is 0, below the
clamp at 1e-20.
What is asserted of the state on the CPU, from the oracle's columns of each source run alone (a cell counts where that
source's rate is positive: its positions were formed), per band:
 - everything tests/test_gpu_table_step_division.py asserts of its state: depths on both sides of the clamp, positions in
   rows 1, 2, NumTau - 1 and NumTau, depths beyond the tables (columns of 1e30 behind the walls), a thin and a thick cell in
   one wave, the source cell in the cube;
 - a depth within 4 ulp of each end of the window on each side of it (four depths);
 - waves (4 x 4 x 4 cubes) in which, for one band, only incoming depths, only outgoing depths, both and neither take the
   near-1 path."""
import numpy as np
import pytest

import test_gpu_table_step_division as base
from oracle_engine import OracleEngine
from plane_reference import constants

pytestmark = pytest.mark.gpu

N = base.N
LO, HI = 0x3FEE0000 << 32, 0x3FF10900 << 32     # the window's ends as bit patterns of doubles in [0.5, 2)
# (source, band) -> the bit pattern the outgoing depth of the source's own cell is to have, but for a power of two
# (hx has the exponent field of [0.5, 1) for every depth below 1 and that of [1, 2) from 1 on: the window's lower end is met by
# depths below 1, its upper end by depths of at least 1.  Sources 1 and 2 sit in thin planes, depths of 1e-20 and a little
# more: the lower end, by their hydrogen (band 0) and neutral helium (band 1).  Source 0 sits in an ordinary cell, whose
# helium fractions of 1e-10 become a few per cent for a depth of 1: the upper end, by its neutral helium in band 1 and
# its singly ionised helium in the first band in which that absorbs.  Its hydrogen stays as it is: behind a cell that is
# thick in every species of a band the thin cells' own columns vanish in the sums, and the reference's species split
# divides 0 by 0.)
HE2 = "first He II band"
TARGETS = {(0, 1): HI + 1, (0, HE2): HI - 2, (1, 0): LO - 2, (1, 1): LO + 1, (2, 0): LO + 1, (2, 1): LO - 1}
FEW = 4


def _scaled(tau):
    """Bit patterns of tau scaled by a power of two into [0.5, 2) as the kernel's split scales it: mantissa under the
    exponent field of [0.5, 1) for tau < 1 and of [1, 2) otherwise."""
    bits = np.asarray(tau, dtype=np.float64).view(np.uint64).astype(np.int64)
    field = np.where(np.asarray(tau) < 1.0, 0x3FE, 0x3FF).astype(np.int64) << 52
    return (bits & ((1 << 52) - 1)) | field


def _near1(tau):
    hx = _scaled(np.maximum(tau, 1.0e-20)) >> 32
    return (hx >= (LO >> 32)) & (hx < (HI >> 32))


def _tune(x0, depth_of, target):
    """A double within a few binades above x0 for which depth_of(x) -- a + x * slope up to rounding, growing with x -- has
    the scaled bit pattern `target`, or a pattern as near to the window's end that target is next to, on target's side."""
    t = float(np.array([target], dtype=np.int64).view(np.float64)[0])   # in [0.5, 2)
    end = LO if abs(target - LO) < abs(target - HI) else HI
    above = target >= end
    a, b = float(depth_of(np.array([0.0]))[0]), float(depth_of(np.array([x0]))[0])
    least = max(b, 2.0 * a, 2.0e-20)                                     # above the clamp, and not all of it the fixed part
    least = max(least, 1.0) if end == HI else least                      # (the upper end: depths of at least 1)
    goal = t * 2.0 ** np.ceil(np.log2(least / t))
    assert (goal >= 1.0) == (end == HI), (goal, hex(target))
    slope = (float(depth_of(np.array([0.25]))[0]) - a) / 0.25            # (from a large fraction: b - a may cancel)
    x = (goal - a) / slope
    for _ in range(4):
        x = x + (goal - float(depth_of(np.array([x]))[0])) / slope
    for _ in range(8):
        cand = (np.array([x]).view(np.int64)[0] + np.arange(-4096, 4097)).view(np.float64)
        got = _scaled(depth_of(cand))
        ok = ((got >= end) == above) & (np.abs(got - end) <= FEW)
        if ok.any():
            return float(cand[ok][np.argmin(np.abs(got[ok] - target))])
        x = float(cand[np.argmin(np.abs(got - target))])
    raise AssertionError(("no fraction puts the depth next to the window's end", hex(target)))


def _inputs(hp, t, abu_he):
    """base._inputs with the three source cells' neutral fractions tuned (TARGETS)."""
    ndens, xh, xhe, dr, vol = base._inputs(hp)
    nc = N ** 3
    path = 0.5 * dr[0]
    for s, (i, j, k) in enumerate(base.SRCPOS):
        q = (i - 1) + N * ((j - 1) + N * (k - 1))
        nd = ndens[q]
        # doric.f90's coldens: neufrac * ndens * path * abundance, from the left; the source cell's incoming columns are 0
        col_HI = lambda x: 0.0 + x * nd * path * (1.0 - abu_he)
        col_HeI = lambda x: 0.0 + x * nd * path * abu_he
        col_HeII = col_HeI
        x_HI, x_HeI, x_HeII = xh[q], xhe[q], xhe[q + nc]
        if (s, 0) in TARGETS:
            x_HI = _tune(x_HI, lambda x: col_HI(x) * t.sigma_HI[0], TARGETS[(s, 0)])
        part = float(col_HI(np.array([x_HI]))[0] * t.sigma_HI[1])
        x_HeI = _tune(x_HeI, lambda x: part + col_HeI(x) * t.sigma_HeI[1], TARGETS[(s, 1)])
        if (s, HE2) in TARGETS:
            b2 = int(np.flatnonzero(t.sigma_HeII > 0.0)[0])
            part = float(col_HI(np.array([x_HI]))[0] * t.sigma_HI[b2] + col_HeI(np.array([x_HeI]))[0] * t.sigma_HeI[b2])
            x_HeII = _tune(x_HeII, lambda x: part + col_HeII(x) * t.sigma_HeII[b2], TARGETS[(s, HE2)])
        assert 0.0 < x_HI < 0.5 and 0.0 < x_HeI and 0.0 < x_HeII and x_HeI + x_HeII < 0.9, (x_HI, x_HeI, x_HeII)
        xh[q], xh[q + nc] = x_HI, 1.0 - x_HI
        xhe[q], xhe[q + nc], xhe[q + 2 * nc] = x_HeI, x_HeII, 1.0 - x_HeI - x_HeII
    return ndens, xh, xhe, dr, vol


def _cell_columns(src, ndens, xh, xhe, dr, abu_he):
    """What each cell adds to the three columns of source `src` (1-based position): doric.f90's coldens over the path through
    the cell, 0.5 dr in the source's own cell and dr * |d| / max|d_axis| elsewhere (offsets wrapped into -8 .. 7)."""
    ax = [((np.arange(N) + 1 - c + N // 2) % N - N // 2).astype(np.float64) for c in src]
    dk, dj, di = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    longest = np.maximum(np.maximum(np.abs(di), np.abs(dj)), np.abs(dk))
    path = np.where(longest > 0, np.sqrt(di * di + dj * dj + dk * dk) / np.maximum(longest, 1.0), 0.5).reshape(-1) * dr[0]
    nc = N ** 3
    return np.stack([xh[:nc] * ndens * path * (1.0 - abu_he), xhe[:nc] * ndens * path * abu_he, xhe[nc:2 * nc] * ndens * path * abu_he])


def _window_sides(tau, rel):
    """(certainly inside, certainly outside) the near-1 window for depths known to a relative error `rel`"""
    tau = np.maximum(tau, 1.0e-20)
    m = _scaled(tau).view(np.float64)
    lo, hi = (np.array([e], dtype=np.int64).view(np.float64)[0] for e in (LO, HI))
    known = rel < 1.0e-3
    inside = known & (m >= lo * (1.0 + rel)) & (m <= hi * (1.0 - rel))
    outside = known & ((m <= lo * (1.0 - rel)) | (m >= hi * (1.0 + rel)))
    return inside, outside


def _assert_window_is_exercised(t, alone_runs):
    """alone_runs: per source (its columns added per cell [species, cell], coldensh_out, coldenshe_out, phih) of the source run
    alone.  The outgoing depths are the kernel's own, bit for bit; the incoming ones are formed here as outgoing column minus
    the cell's own, good to a relative error of a few ulp times outgoing over incoming, and a wave is counted for a kind only
    where that error cannot change the answer of any of its lanes."""
    nc = N ** 3
    nb = int(t.bb_upper)
    sig = np.stack([t.sigma_HI, t.sigma_HeI, t.sigma_HeII])[:, :nb]
    assert sig[1, 0] == 0.0 and sig[2, 0] == 0.0 and sig[1, 1] > 0.0 and sig[2, 1] == 0.0   # bands 0 and 1 as _inputs takes them
    ends = {("lo", False): False, ("lo", True): False, ("hi", False): False, ("hi", True): False}
    waves = {"in only": False, "out only": False, "both": False, "neither": False}
    for own, h_out, he_out, phih in alone_runs:
        done = (phih > 0.0)[:, None]
        cout = np.stack([h_out, he_out[:nc], he_out[nc:2 * nc]])
        cin = np.maximum(cout - own, 0.0)
        # the kernel's own sums: species by species from the left, no fma (a species that cannot absorb adds exactly 0)
        tout = cout[0][:, None] * sig[0] + cout[1][:, None] * sig[1] + cout[2][:, None] * sig[2]
        tin = cin[0][:, None] * sig[0] + cin[1][:, None] * sig[1] + cin[2][:, None] * sig[2]
        live = done & (tout >= 1.0e-20) & np.isfinite(tout)
        pat = _scaled(np.where(live, tout, 1.5))
        for name, end in (("lo", LO), ("hi", HI)):
            d = pat - end
            ends[(name, False)] |= bool((live & (d < 0) & (d >= -FEW)).any())
            ends[(name, True)] |= bool((live & (d >= 0) & (d <= FEW)).any())
        with np.errstate(divide="ignore", invalid="ignore"):
            rel_in = np.where(tin > 0.5e-20, 1.0e-15 * tout / tin, np.where(tout < 0.5e-20, 0.0, 1.0))
        rel_in = np.where(np.isfinite(tin) & np.isfinite(tout), rel_in + 1.0e-12, 1.0)
        rel_in = np.where(tin < 0.25e-20, 0.0, rel_in)                       # far below the clamp: the clamp's own value, outside
        a_in, a_out = _window_sides(np.where(np.isfinite(tin), tin, 1.0), rel_in)
        b_in, b_out = _window_sides(np.where(np.isfinite(tout), tout, 1.0), np.where(np.isfinite(tout), 0.0, 1.0))
        lanes = base._cubes(done).any(axis=1)                                # [cube, band]: the wave ran the band
        # lanes that did not run the band count for nothing: certainly outside
        some = lambda m_: base._cubes(m_ & done).any(axis=1)
        none = lambda m_: base._cubes(m_ | ~done).all(axis=1)
        waves["in only"] |= bool((lanes & some(a_in) & none(b_out)).any())
        waves["out only"] |= bool((lanes & none(a_out) & some(b_in)).any())
        waves["both"] |= bool((lanes & some(a_in) & some(b_in)).any())
        waves["neither"] |= bool((lanes & none(a_out) & none(b_out)).any())
    assert all(ends.values()), ("no depth within a few ulp of an end of the near-1 window", ends)
    assert all(waves.values()), ("near-1 path: a kind of wave is missing", waves)


def _reference(pkg, orc, otables):
    """(run, the oracle's results); the inputs checked on the way"""
    hp = pkg.hostphys
    t = pkg.RadiationTables.load()
    abu_he, _ = constants(orc)
    ndens, xh, xhe, dr, vol = _inputs(hp, t, abu_he)
    mat = pkg.Material(ndens, xh, xhe, None, True, 1.0e4, 1.0, hp.reccoef(1.0e4))
    grid = pkg.GridProps((N, N, N), dr, vol)
    flux = np.array([3.0e6, 1.0e5, 2.0e7])
    cosmo = pkg.Cosmology(base.ZRED, hp.H0, hp.Omega0)
    grids = ("phih_grid", "phihe_grid")

    def run(e, batch=None, only=None):
        e.set_tables(t)
        e.set_step(mat, grid, cosmo)
        e.set_sources(pkg.SourceProps(base.SRCPOS, flux, 1.0e48) if only is None else pkg.SourceProps(base.SRCPOS[only:only + 1], flux[only:only + 1], 1.0e48))
        if batch is not None:
            e.set_batch(batch)
        e.upload_state(mat)
        e.begin_step()
        e.set_rates_to_zero()
        e.pass_sources(1, 1)
        return e.download_rates()

    alone_runs = []
    for s in range(3):
        alone = OracleEngine((N, N, N), otables)
        reached = run(alone, only=s)["phih_grid"]
        alone_runs.append((_cell_columns(base.SRCPOS[s], ndens, xh, xhe, dr, abu_he), alone.s.coldensh_out.copy(),
                           alone.s.coldenshe_out.copy(), reached.copy()))
        if s == 2:
            base._assert_inputs_do_their_job(t, alone.s.coldensh_out, alone.s.coldenshe_out, reached)
    _assert_window_is_exercised(t, alone_runs)
    whole = OracleEngine((N, N, N), otables)
    ref = run(whole)
    # the kept loss is the same number in whatever order its terms are added (base._walls)
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


@pytest.fixture(scope="module")
def case(pkg, orc, otables):
    return _reference(pkg, orc, otables)


@pytest.fixture(scope="module", params=[1, 3], ids=["a-launch-per-source", "one-launch"])
def results(request, pkg, case):
    run, ref, grids = case
    e = pkg.HipEngine((N, N, N), 0)
    try:
        got = run(e, request.param)
    finally:
        e.close()
    return got, ref, grids


def test_rates_loss_and_box_count_bit_for_bit_with_indexed_gathers_and_the_tabulated_near1_test(results):
    got, ref, grids = results
    for k in grids:
        print(k, "cells that differ:", int((got[k] != ref[k]).sum()), "of", got[k].size)
    print("photon_loss", float(got["photon_loss"][0]).hex(), "oracle", float(ref["photon_loss"][0]).hex())
    print("sum_nbox", got["sum_nbox"], "oracle", ref["sum_nbox"])
    assert got["sum_nbox"] == ref["sum_nbox"]
    for k in grids:
        assert np.array_equal(got[k], ref[k]), (k, int((got[k] != ref[k]).sum()))
    assert np.array_equal(got["photon_loss"], ref["photon_loss"])
