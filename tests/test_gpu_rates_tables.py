"""The two tables that the isothermal one-SED rates kernel reads instead of computing, where they can go wrong.  k_rates
reads the black-body photo table as (value, forward difference) pairs, a device copy remade whenever the table is set or
built, and, on an all-periodic mesh, the shell volume of a cell.source and its reciprocal from a table per offset
(|di|, |dj|, |dk|), remade when the cell sizes change.  Every comparison is bit for bit, with the oracle behind
tests/oracle_engine.py or with a context that has seen nothing else:

 * geometry indexing: non-cubic meshes smaller than, and ragged against, the kernel's 8 x 8 x 4 tile, cell sizes that differ
   per axis (a transposed index then reads another volume), sources in both far corners and in the centre, so that every
   wrapped offset of every axis occurs, the source's own cell included;
 * stale geometry: one context, another redshift (other cell sizes) between two passes, and back;
 * stale pairs: one context, another photo table between two passes, uploaded and built on the device;
 * awkward table rows: equal neighbours (difference +0), a run of exact zeros at the end, a subnormal difference;
 * volumes below 1: cells of 0.1 cm, where Markstein's sequence is not allowed and every lane divides."""
from pathlib import Path

import numpy as np
import pytest

from oracle_engine import OracleEngine

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).parent / "golden"

ZRED = 9.0
ABU_HE = 0.074
NUMTAU, MINLOGTAU, DLOGTAU = 2000, -20.0, 0.012


def _state(nc, seed, lo=-8.0, hi=-1.0):
    """Neutral fractions drawn per cell, log-uniform over [10^lo, 10^hi): (xh, xhe), Fortran layout."""
    rng = np.random.default_rng(seed)
    x_HI, x_HeI, x_HeII = (10.0 ** rng.uniform(lo, hi, nc) for _ in range(3))
    return np.concatenate([x_HI, 1.0 - x_HI]), np.concatenate([x_HeI, x_HeII, 1.0 - x_HeI - x_HeII])


def _one_pass(e, mat, grid, cosmo, src, tables=None, batch=None):
    if tables is not None:
        e.set_tables(tables)
    e.set_step(mat, grid, cosmo)
    e.set_sources(src)
    if batch is not None:
        e.set_batch(batch)
    e.upload_state(mat)
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    return e.download_rates()


def _same(got, want):
    assert got["sum_nbox"] == want["sum_nbox"]
    for k in ("phih_grid", "phihe_grid"):
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


def _case(pkg, mesh, dr, ndens, xh, xhe, srcpos, flux, zred=ZRED):
    hp = pkg.hostphys
    vol = dr[0] * dr[1] * dr[2]
    mat = pkg.Material(ndens, xh, xhe, None, True, 1.0e4, 1.0, hp.reccoef(1.0e4))
    grid = pkg.GridProps(tuple(mesh), tuple(dr), vol)
    src = pkg.SourceProps(np.asarray(srcpos, dtype=np.int32), np.asarray(flux, dtype=np.float64), 1.0e48)
    cosmo = pkg.Cosmology(zred, hp.H0, hp.Omega0)
    return mat, grid, cosmo, src


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", [(12, 8, 6), (9, 7, 5)], ids=lambda m: "x".join(map(str, m)))
@pytest.mark.parametrize("batch", [1, 3], ids=["a-launch-per-source", "one-launch"])
def test_shell_volumes_are_read_where_they_were_written(pkg, otables, mesh, batch):
    hp = pkg.hostphys
    nc = int(np.prod(mesh))
    d0 = hp.test_grid(8, ZRED)[0][0]
    dr = (d0, 1.25 * d0, 0.75 * d0)                       # per axis: |di|, |dj|, |dk| are not interchangeable
    xh, xhe = _state(nc, 20261021 + nc)
    ndens = np.full(nc, hp.test_density(ZRED))
    srcpos = [(1, 1, 1), tuple(mesh), tuple((n + 1) // 2 for n in mesh)]
    case = _case(pkg, mesh, dr, ndens, xh, xhe, srcpos, [3.0e6, 1.0e5, 2.0e7])
    ref = _one_pass(OracleEngine(mesh, otables), *case)
    # every source reaches the whole mesh: all wrapped offsets -l .. n - l - 1 of every axis occur, for every source
    assert ref["sum_nbox"] >= 3 and (ref["phih_grid"] > 0).all() and np.isfinite(ref["phih_grid"]).all()
    for s in range(3):
        alone = _case(pkg, mesh, dr, ndens, xh, xhe, srcpos[s:s + 1], [1.0e6])
        r1 = _one_pass(OracleEngine(mesh, otables), *alone)
        assert (r1["phih_grid"] > 0).all(), s
    e = pkg.HipEngine(tuple(mesh), 0)
    try:
        got = _one_pass(e, *case, tables=pkg.RadiationTables.load(), batch=batch)
    finally:
        e.close()
    _same(got, ref)


# ---------------------------------------------------------------------------------------------------------------------
def test_shell_volumes_follow_the_cell_sizes(pkg, otables):
    hp = pkg.hostphys
    n = 8
    mesh, nc = (n, n, n), n ** 3
    xh, xhe = _state(nc, 7)
    t = pkg.RadiationTables.load()
    cases, fresh = {}, {}
    for z in (9.0, 6.0):
        dr, _ = hp.test_grid(n, z)
        cases[z] = _case(pkg, mesh, dr, np.full(nc, hp.test_density(z)), xh, xhe, [(3, 6, 2)], [3.0e6], zred=z)
        e = pkg.HipEngine(mesh, 0)
        try:
            fresh[z] = _one_pass(e, *cases[z], tables=t)
        finally:
            e.close()
        _same(fresh[z], _one_pass(OracleEngine(mesh, otables), *cases[z]))
    assert cases[9.0][1].dr != cases[6.0][1].dr and not np.array_equal(fresh[9.0]["phih_grid"], fresh[6.0]["phih_grid"])
    e = pkg.HipEngine(mesh, 0)
    try:
        e.set_tables(t)
        for z in (9.0, 6.0, 9.0, 9.0, 6.0):                # another redshift, back, the same once more, and again
            _same(_one_pass(e, *cases[z]), fresh[z])
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
def _scaled_tables(pkg, factor):
    t = pkg.RadiationTables.load()
    t.photo_thick = np.ascontiguousarray(t.photo_thick * factor)
    return t


def test_pairs_follow_the_table(pkg, otables, gold):
    hp = pkg.hostphys
    n = 8
    mesh, nc = (n, n, n), n ** 3
    xh, xhe = _state(nc, 11)
    dr, _ = hp.test_grid(n, ZRED)
    case = _case(pkg, mesh, dr, np.full(nc, hp.test_density(ZRED)), xh, xhe, [(2, 7, 5)], [3.0e6])
    t_a, t_b = _scaled_tables(pkg, 0.5), pkg.RadiationTables.load()    # A: other values in photo_thick only
    fresh = {}
    for name, t in (("a", t_a), ("b", t_b)):
        e = pkg.HipEngine(mesh, 0)
        try:
            fresh[name] = _one_pass(e, *case, tables=t)
        finally:
            e.close()
    _same(fresh["b"], _one_pass(OracleEngine(mesh, otables), *case))
    assert not np.array_equal(fresh["a"]["phih_grid"], fresh["b"]["phih_grid"])
    # the black-body tables built on the device are the shipped ones bit for bit (test_table_construction_on_device)
    t_built = pkg.RadiationTables.load()
    t_built.setup, t_built.build_on_device = dict(gold("sed_setup.npz")), True
    e = pkg.HipEngine(mesh, 0)
    try:
        _same(_one_pass(e, *case, tables=t_a), fresh["a"])
        _same(_one_pass(e, *case, tables=t_b), fresh["b"])            # uploaded over A
        _same(_one_pass(e, *case, tables=t_a), fresh["a"])
        _same(_one_pass(e, *case, tables=t_built), fresh["b"])        # built on the device over A
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
ZROW = 1700          # first row of the run of zeros; rows ZROW - 2 and ZROW - 1 differ by a subnormal number


def _awkward(photo_thick):
    pt = photo_thick.reshape(-1, NUMTAU + 1).copy()
    pt[:, 1::2] = pt[:, 0:NUMTAU:2]          # row 2k + 1 = row 2k: the difference at every even row is +0
    pt[:, ZROW - 2] = 3.0e-310
    pt[:, ZROW - 1] = 1.0e-310
    pt[:, ZROW:] = 0.0
    return np.ascontiguousarray(pt.reshape(-1))


def test_awkward_table_rows(pkg, orc):
    hp = pkg.hostphys
    n = 8
    mesh, nc = (n, n, n), n ** 3
    xh, xhe = _state(nc, 13, lo=-8.0, hi=-0.5)
    dr, _ = hp.test_grid(n, ZRED)
    ndens = np.full(nc, hp.test_density(ZRED))
    wall = np.arange(nc) % n == 6            # a plane of neutral cells at 30 times the density: depths beyond 1e4
    xh[:nc][wall], xh[nc:][wall] = 1.0, 0.0
    xhe[:nc][wall], xhe[nc:2 * nc][wall], xhe[2 * nc:][wall] = 1.0, 0.0, 0.0
    ndens[wall] *= 30.0
    case = _case(pkg, mesh, dr, ndens, xh, xhe, [(1, 8, 3), (5, 4, 6)], [3.0e6, 2.0e7])
    t = pkg.RadiationTables.load()
    t.photo_thick = _awkward(t.photo_thick)
    with np.load(pkg.evolve.DEFAULT_TABLES) as z:
        d = {k: z[k] for k in z.files}
    d["photo_thick"] = t.photo_thick.copy()
    ref_engine = OracleEngine(mesh, orc.Tables(d))
    ref = _one_pass(ref_engine, *case)
    assert np.isfinite(ref["phih_grid"]).all() and (ref["phih_grid"] > 0).any()
    # the cells land on those rows: the outgoing depths of the source handled last, band by band
    nb = int(t.bb_upper)
    sig = np.stack([t.sigma_HI, t.sigma_HeI, t.sigma_HeII])[:, :nb]
    cols = np.stack([ref_engine.s.coldensh_out, ref_engine.s.coldenshe_out[:nc], ref_engine.s.coldenshe_out[nc:2 * nc]])
    tau = np.einsum("sb,sc->cb", sig, cols)
    row = np.minimum(NUMTAU, np.floor(1.0 + (np.log10(np.maximum(tau, 1.0e-20)) - MINLOGTAU) / DLOGTAU)).astype(int)
    assert ((row < ZROW - 2) & (row % 2 == 0)).any(), "no position on a pair of equal neighbours"
    assert ((row < ZROW - 2) & (row % 2 == 1)).any(), "no position on an ordinary pair"
    assert ((row == ZROW - 2) | (row == ZROW - 1)).any(), "no position on the subnormal difference"
    assert (row >= ZROW).any() and (row == NUMTAU).any(), "no position in the run of zeros, or none on the last row"
    e = pkg.HipEngine(mesh, 0)
    try:
        got = _one_pass(e, *case, tables=t)
    finally:
        e.close()
    _same(got, ref)


# ---------------------------------------------------------------------------------------------------------------------
def test_shell_volumes_below_one(pkg, otables):
    n = 8
    mesh, nc = (n, n, n), n ** 3
    dr = (0.1, 0.1, 0.1)
    # vol_ph = 4 pi d^2 path with path <= sqrt(3) dr: below 1 for the cell itself and for most offsets (the corner offset (4,4,4) has 1.04)
    o = np.minimum(np.arange(n), n - np.arange(n)).astype(float)
    d2 = 0.01 * (o[:, None, None] ** 2 + o[None, :, None] ** 2 + o[None, None, :] ** 2)
    assert dr[0] * dr[1] * dr[2] < 1.0 and (4.0 * np.pi * d2 * 0.1 * np.sqrt(3.0) < 1.0).mean() > 0.5
    xh, xhe = _state(nc, 17, lo=-3.0, hi=0.0)
    xhe = np.concatenate([xhe[:nc] * 0.5, xhe[nc:2 * nc] * 0.5, 1.0 - 0.5 * (xhe[:nc] + xhe[nc:2 * nc])])
    ndens = np.full(nc, 1.0e18)                          # columns of 1e14 .. 1e17 per cell: depths of 1e-3 .. 1
    case = _case(pkg, mesh, dr, ndens, xh, xhe, [(4, 4, 4), (8, 1, 2)], [3.0e6, 1.0e6])
    ref = _one_pass(OracleEngine(mesh, otables), *case)
    assert np.isfinite(ref["phih_grid"]).all() and (ref["phih_grid"] > 0).any()
    e = pkg.HipEngine(mesh, 0)
    try:
        got = _one_pass(e, *case, tables=pkg.RadiationTables.load())
    finally:
        e.close()
    _same(got, ref)
