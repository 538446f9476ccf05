"""Cases for the open (non-periodic) mesh boundaries, shared by tests/test_open_boundaries_oracle.py (CPU) and
tests/test_gpu_open_boundaries.py (GPU).  Not a test module.

The oracle only knows periodic boundaries, yet it gives exact expected values for an open N^3 box: a cell's rates
depend only on the cells between it and the source, so the open run equals, bit for bit on its N^3 cells, the
oracle's PERIODIC run on an M^3 mesh with M >= 2 N that holds the box AT THE MESH ORIGIN (cells 1..N; cinterp forms
its crossing points in absolute coordinates, a shifted region changes bits) and arbitrary gas elsewhere -- provided
both runs trace the same cells.  M must avoid (M/2 - 1) mod 10 == 0.
"""
import numpy as np

ZRED = 9.0
SUBBOXSIZE = 10


def embed(region, n, m, pad):
    """The n^3 region (components of n^3 cells each, i fastest) at the origin of an m^3 mesh filled with `pad`."""
    region, pad = np.asarray(region), np.asarray(pad)
    ncomp = region.size // n ** 3
    out = pad.reshape(ncomp, m, m, m).copy()          # [component, k, j, i]
    out[:, :n, :n, :n] = region.reshape(ncomp, n, n, n)
    return out.reshape(-1)


def extract(big, n, m):
    """The region at the origin of an m^3 mesh, same layout."""
    big = np.asarray(big)
    ncomp = big.size // m ** 3
    return np.ascontiguousarray(big.reshape(ncomp, m, m, m)[:, :n, :n, :n]).reshape(-1)


def gas(pkg, ncell, rng, kind, heat):
    """Density and state of `ncell` cells: 'mixed' (log-normal density, ionised fractions 1e-6 .. 0.5), 'ionised'
    (neutral fractions 1e-4.5 .. 1e-3.5: every box runs to its reach) or 'opaque' (neutral, 1.5 times denser: ten cells
    let through some 1e-19 of a source's photons, two cells 1e-4 of them -- boxes stop after their first round, and
    a mesh face two cells from a source still loses far more than the 1e-10 of the while-test)."""
    hp = pkg.hostphys
    ndens = hp.test_density(ZRED) * np.exp(rng.normal(0.0, 0.7, ncell))
    if kind == "mixed":
        x = 10.0 ** rng.uniform(-6, -0.3, ncell)
    elif kind == "ionised":
        x = 1.0 - 10.0 ** rng.uniform(-4.5, -3.5, ncell)
    elif kind == "opaque":
        x = 10.0 ** rng.uniform(-6, -5, ncell)
        ndens = ndens * 1.5
    else:
        raise ValueError(kind)
    xh = np.concatenate([1.0 - x, x])
    xhe = np.concatenate([1.0 - x, 0.8 * x, 0.2 * x])
    temp = np.tile((1e4 * np.exp(rng.normal(0, 0.2, ncell))).astype(np.float32), 3) if heat else None
    return ndens, xh, xhe, temp


class Case:
    """An open n^3 box and its embedding at the origin of a periodic m^3 mesh."""

    def __init__(self, pkg, n, m, kind, srcpos, flux, seed, heat=False, pad_seed=None, pad_kind=None, pl=None, qpl=None):
        assert m >= 2 * n and (m // 2 - 1) % SUBBOXSIZE != 0
        hp = pkg.hostphys
        self.n, self.m, self.heat = n, m, heat
        self.dr, self.vol = hp.test_grid(n, ZRED)      # the same cells in both meshes
        self.srcpos = np.asarray(srcpos, dtype=np.int32).reshape(-1, 3)
        self.flux = np.asarray(flux, dtype=np.float64)
        self.pl = None if pl is None else np.asarray(pl, dtype=np.float64)
        self.qpl = None if qpl is None else np.asarray(qpl, dtype=np.float64)
        self.s_star, self.pl_s_star, self.qpl_s_star = 1.0e48, 2.0e48, 0.5e48
        self.ndens, self.xh, self.xhe, self.temp = gas(pkg, n ** 3, np.random.default_rng(seed), kind, heat)
        pad = gas(pkg, m ** 3, np.random.default_rng(seed + 1000 if pad_seed is None else pad_seed), pad_kind or kind, heat)
        self.big = [embed(a, n, m, b) if a is not None else None for a, b in zip((self.ndens, self.xh, self.xhe, self.temp), pad)]
        self.reccoef = hp.reccoef(1.0e4)

    # -- the product, open boundaries ---------------------------------------------------------------------
    def engine(self, pkg, tables, sources=None, periodic=False):
        hp = pkg.hostphys
        n = self.n
        idx = np.arange(len(self.flux)) if sources is None else np.asarray(sources)
        mat = pkg.Material(self.ndens, self.xh.copy(), self.xhe.copy(), None if self.temp is None else self.temp.copy(),
                           not self.heat, 1.0e4, 1.0, self.reccoef)
        src = pkg.SourceProps(self.srcpos[idx], self.flux[idx], self.s_star)
        if self.pl is not None:
            src.NormFluxPL, src.pl_S_star = self.pl[idx], self.pl_s_star
            src.NormFluxQPL, src.qpl_S_star = self.qpl[idx], self.qpl_s_star
        e = pkg.HipEngine((n, n, n), 0)
        e.set_boundaries(periodic)
        e.set_tables(tables)
        e.set_step(mat, pkg.GridProps((n, n, n), self.dr, self.vol), pkg.Cosmology(ZRED, hp.H0, hp.Omega0))
        e.set_sources(src)
        e.upload_state(mat)
        return e

    def periodic_engine_on_m(self, pkg, tables, sources=None):
        """The embedding on the device: a PERIODIC context of the m^3 mesh (the pinned path)."""
        hp = pkg.hostphys
        m = self.m
        idx = np.arange(len(self.flux)) if sources is None else np.asarray(sources)
        nd, xh, xhe, temp = self.big
        mat = pkg.Material(nd, xh.copy(), xhe.copy(), None if temp is None else temp.copy(), not self.heat, 1.0e4, 1.0, self.reccoef)
        e = pkg.HipEngine((m, m, m), 0)
        e.set_tables(tables)
        e.set_step(mat, pkg.GridProps((m, m, m), self.dr, self.vol), pkg.Cosmology(ZRED, hp.H0, hp.Omega0))
        e.set_sources(pkg.SourceProps(self.srcpos[idx], self.flux[idx], self.s_star))
        e.upload_state(mat)
        return e

    # -- the oracle, periodic on the m^3 mesh --------------------------------------------------------------
    def oracle_step(self, pkg, orc, sources=None, m=None, big=None):
        hp = pkg.hostphys
        m = m or self.m
        nd, xh, xhe, temp = big or self.big
        idx = np.arange(len(self.flux)) if sources is None else np.asarray(sources)
        kw = {}
        if self.pl is not None:
            kw = dict(normflux_pl=self.pl[idx], normflux_qpl=self.qpl[idx], pl_s_star=self.pl_s_star, qpl_s_star=self.qpl_s_star)
        st = orc.Step((m, m, m), self.dr, self.vol, ZRED, hp.H0, hp.Omega0, not self.heat, 1.0e4, 1.0, self.srcpos[idx],
                      self.flux[idx], self.s_star, nd, self.reccoef, **kw)
        s = orc.State(st, xh, xhe, temp)
        orc.begin_step(s)
        return st, s

    def oracle_pass(self, pkg, orc, otables, sources=None, dt=None, m=None, big=None):
        """Rates of the region from the oracle's periodic pass on the m^3 mesh (and, with dt, its global pass):
        dict of region-sized arrays plus sum_nbox and the oracle's own photon_loss."""
        m = m or self.m
        st, s = self.oracle_step(pkg, orc, sources, m, big)
        orc.pass_all_sources(otables, st, s)
        out = {"phih_grid": extract(s.phih, self.n, m), "phihe_grid": extract(s.phihe, self.n, m),
               "phiheat": extract(s.phiheat, self.n, m), "sum_nbox": int(s.c.sum_nbox), "photon_loss": float(s.photon_loss[0])}
        if dt is not None:
            orc.global_pass(otables, st, s, dt)
            for k in ("xh_av", "xhe_av", "xh_intermed", "xhe_intermed"):
                out[k] = extract(getattr(s, k), self.n, m)
        return out

    def other_embedding(self, pkg, m, pad_seed, pad_kind):
        """The same region in another mesh with other padding: (m, big) for oracle_pass."""
        assert m >= 2 * self.n and (m // 2 - 1) % SUBBOXSIZE != 0
        pad = gas(pkg, m ** 3, np.random.default_rng(pad_seed), pad_kind, self.heat)
        return m, [embed(a, self.n, m, b) if a is not None else None for a, b in zip((self.ndens, self.xh, self.xhe, self.temp), pad)]

    def expected_rounds(self, sources=None):
        """Sum over sources of ceil(max_d(|l_d|, r_d) / subboxsize): the rounds of sources that run to their reach."""
        idx = np.arange(len(self.flux)) if sources is None else np.asarray(sources)
        reach = np.maximum(self.srcpos[idx] - 1, self.n - self.srcpos[idx]).max(axis=1)
        return int(np.sum(-(-reach // SUBBOXSIZE)))


def positions(n):
    """A corner, the opposite corner, an edge, a face and the interior of an n^3 box."""
    return np.array([[1, 1, 1], [n, n, n], [n // 2, n, 1], [n // 2 - 1, n, n // 4 + 1], [n // 2 + 2, n // 2 + 1, n // 2 + 1]], dtype=np.int32)


def case_one_round(pkg, heat=False, seds=False):
    """N = 11: every offset is <= subboxsize, so both runs trace the whole region in round 1 whatever the loss."""
    n = 11
    flux = np.array([3.0e7, 8.0e6, 1.5e7, 5.0e6, 2.0e7])
    kw = {}
    if seds:
        kw = dict(pl=np.array([1e6, 2e6, 0.0, 0.0, 5e5]), qpl=np.array([0.0, 1e6, 3e6, 2e6, 5e5]))
        flux = np.array([3e6, 0.0, 1e6, 0.0, 2e6])
    return Case(pkg, n, 24, "mixed", positions(n), flux, seed=1111 + int(heat) + 2 * int(seds), heat=heat, **kw)


# three corners, an edge and an interior cell
FIVE_SOURCES_24 = np.array([[1, 1, 1], [24, 24, 24], [24, 1, 24], [12, 1, 24], [7, 13, 12]], dtype=np.int32)


def case_several_rounds(pkg):
    """N = 24, highly ionised gas: every source runs to its reach (3 rounds from a corner), per-source boxes."""
    return Case(pkg, 24, 48, "ionised", FIVE_SOURCES_24, np.array([2.0e7, 1.0e7, 1.5e7, 8.0e6, 3.0e7]), seed=2424)


def case_early_stop(pkg):
    """N = 24, opaque gas, one source three cells from a face and one in the middle: both stop after round 1."""
    return Case(pkg, 24, 48, "opaque", np.array([[3, 12, 12], [12, 12, 12]], dtype=np.int32), np.array([1.0e4, 1.0e4]), seed=2403)
