"""Cases for mesh boundaries per axis (c2r_set_boundaries_axes), shared by tests/test_axis_boundaries_oracle.py (CPU) and
tests/test_gpu_axis_boundaries.py (GPU).  Not a test module.

The oracle is periodic only, takes a mesh that is no cube and uses the periodic reach per axis.  A product run on
(n1,n2,n3) with some axes open therefore equals, bit for bit on its cells, the oracle's periodic run on a mesh with the same
extent on the periodic axes, an extent M_d >= 2 n_d on the open ones, the region at the mesh origin and any gas elsewhere
(tests/open_boundary_cases.py has the argument for the all-open mode) -- provided both trace the same cells:
  * the oracle's while-test looks at z only and stops when the z faces reach M_z/2, so an axis that is open while z is
    periodic is traced only as far as the rounds z needs: two rounds, +-20 cells, for n_z = 24.  Such axes have 11 cells;
  * (M_z/2 - 1) mod 10 must not be 0 (the reference's last round is then never swept).
"""
import numpy as np

import open_boundary_cases as ob

ZRED = ob.ZRED
SUBBOXSIZE = ob.SUBBOXSIZE
S_STAR = 1.0e48
REGION_SEED, PAD_SEED, OTHER_PAD_SEED = 4242, 5242, 77


def cells(mesh):
    return int(mesh[0]) * int(mesh[1]) * int(mesh[2])


def embed3(region, n, m, pad):
    """The (n1,n2,n3) region (components of n1 n2 n3 cells each, i fastest) at the origin of an (m1,m2,m3) mesh filled with `pad`."""
    region, pad = np.asarray(region), np.asarray(pad)
    ncomp = region.size // cells(n)
    out = pad.reshape(ncomp, m[2], m[1], m[0]).copy()       # [component, k, j, i]
    out[:, :n[2], :n[1], :n[0]] = region.reshape(ncomp, n[2], n[1], n[0])
    return out.reshape(-1)


def extract3(big, n, m):
    """The region at the origin of an (m1,m2,m3) mesh, same layout."""
    big = np.asarray(big)
    ncomp = big.size // cells(m)
    return np.ascontiguousarray(big.reshape(ncomp, m[2], m[1], m[0])[:, :n[2], :n[1], :n[0]]).reshape(-1)


def axis_reach(mesh, pos, periodic, max_subbox=1150):
    """(l, r) of include/c2ray_hip.h for one axis."""
    if periodic:
        return -min(max_subbox, mesh // 2), min(max_subbox, mesh // 2 - 1 + mesh % 2)
    return -min(max_subbox, pos - 1), min(max_subbox, mesh - pos)


class AxisCase:
    """A product mesh n = (n1,n2,n3) with the axes of `open_axes` (letters of "xyz") open, and its embedding at the origin
    of a periodic mesh m: m_d == n_d on the periodic axes, m_d >= 2 n_d on the open ones."""

    def __init__(self, pkg, n, open_axes, m, kind, srcpos, flux, heat=False, pad_kind=None, pad_seed=PAD_SEED, pl=None, qpl=None):
        hp = pkg.hostphys
        self.n, self.m, self.heat, self.kind = tuple(n), tuple(m), heat, kind
        self.periodic = tuple(ax not in open_axes for ax in "xyz")
        self.check_embedding(self.m)
        self.dr, self.vol = hp.test_grid(24, ZRED)
        self.srcpos = np.asarray(srcpos, dtype=np.int32).reshape(-1, 3)
        self.flux = np.asarray(flux, dtype=np.float64)
        self.pl = None if pl is None else np.asarray(pl, dtype=np.float64)
        self.qpl = None if qpl is None else np.asarray(qpl, dtype=np.float64)
        self.s_star, self.pl_s_star, self.qpl_s_star = S_STAR, 2.0e48, 0.5e48
        self.region = ob.gas(pkg, cells(n), np.random.default_rng(REGION_SEED), kind, heat)
        self.big = self.embedding(pkg, self.m, pad_seed, pad_kind or kind)
        self.reccoef = hp.reccoef(1.0e4)

    def check_embedding(self, m):
        for nd, md, per in zip(self.n, m, self.periodic):
            assert md == nd if per else md >= 2 * nd, (self.n, m, self.periodic)
        assert (m[2] // 2 - 1) % SUBBOXSIZE != 0
        if self.periodic[2]:        # the oracle grows a box for as many rounds as z needs: open axes must be done by then
            rounds = -(-(m[2] // 2) // SUBBOXSIZE)
            assert all(per or nd - 1 <= SUBBOXSIZE * rounds for nd, per in zip(self.n, self.periodic))

    def embedding(self, pkg, m, pad_seed, pad_kind):
        """[ndens, xh, xhe, temperature] of the region in the mesh m, padded with gas of `pad_kind` from `pad_seed`."""
        self.check_embedding(m)
        pad = ob.gas(pkg, cells(m), np.random.default_rng(pad_seed), pad_kind, self.heat)
        return [embed3(a, self.n, m, b) if a is not None else None for a, b in zip(self.region, pad)]

    def _sources(self, sources):
        return np.arange(len(self.flux)) if sources is None else np.asarray(sources)

    # -- the product -----------------------------------------------------------------------------------------
    def _engine(self, pkg, tables, mesh, gas, boundaries, idx):
        hp = pkg.hostphys
        ndens, xh, xhe, temp = gas
        mat = pkg.Material(ndens, xh.copy(), xhe.copy(), None if temp is None else temp.copy(), not self.heat, 1.0e4, 1.0, self.reccoef)
        src = pkg.SourceProps(self.srcpos[idx], self.flux[idx], self.s_star)
        if self.pl is not None:
            src.NormFluxPL, src.pl_S_star = self.pl[idx], self.pl_s_star
            src.NormFluxQPL, src.qpl_S_star = self.qpl[idx], self.qpl_s_star
        e = pkg.HipEngine(tuple(mesh), 0)
        if boundaries is not None:
            e.set_boundaries(boundaries)
        e.set_tables(tables)
        e.set_step(mat, pkg.GridProps(tuple(mesh), self.dr, self.vol), pkg.Cosmology(ZRED, hp.H0, hp.Omega0))
        e.set_sources(src)
        e.upload_state(mat)
        return e

    def engine(self, pkg, tables, sources=None, boundaries="case"):
        """A context of the product mesh with this case's boundaries (or `boundaries`: a bool, three of them, or None to
        leave the context as it was created)."""
        return self._engine(pkg, tables, self.n, self.region, self.periodic if isinstance(boundaries, str) else boundaries,
                            self._sources(sources))

    def periodic_engine_on_m(self, pkg, tables, sources=None):
        """The embedding on the device: an all-periodic context of the mesh m (the pinned path)."""
        return self._engine(pkg, tables, self.m, self.big, None, self._sources(sources))

    # -- the oracle, periodic on the mesh m --------------------------------------------------------------------
    def oracle_pass(self, pkg, orc, otables, sources=None, dt=None, m=None, big=None):
        """Rates of the region from the oracle's periodic pass on the mesh m (and, with dt, its global pass): region-sized
        arrays plus sum_nbox, the oracle's own photon_loss and the columns of the source it swept last."""
        hp = pkg.hostphys
        m = self.m if m is None else tuple(m)
        nd, xh, xhe, temp = self.big if big is None else big
        idx = self._sources(sources)
        kw = {}
        if self.pl is not None:
            kw = dict(normflux_pl=self.pl[idx], normflux_qpl=self.qpl[idx], pl_s_star=self.pl_s_star, qpl_s_star=self.qpl_s_star)
        st = orc.Step(m, self.dr, self.vol, ZRED, hp.H0, hp.Omega0, not self.heat, 1.0e4, 1.0, self.srcpos[idx], self.flux[idx],
                      self.s_star, nd, self.reccoef, **kw)
        s = orc.State(st, xh, xhe, temp)
        orc.begin_step(s)
        orc.pass_all_sources(otables, st, s)
        out = {k: extract3(getattr(s, a), self.n, m) for k, a in (("phih_grid", "phih"), ("phihe_grid", "phihe"), ("phiheat", "phiheat"),
                                                                   ("coldensh_out", "coldensh_out"), ("coldenshe_out", "coldenshe_out"))}
        out["sum_nbox"], out["photon_loss"] = int(s.c.sum_nbox), float(s.photon_loss[0])
        if dt is not None:
            orc.global_pass(otables, st, s, dt)
            for k in ITER_STATE:
                out[k] = extract3(getattr(s, k), self.n, m)
        return out

    # -- what the product is expected to report ------------------------------------------------------------------
    def reach(self, ns):
        """([l_x, l_y, l_z], [r_x, r_y, r_z]) of source ns (0-based)."""
        lr = [axis_reach(nd, int(p), per) for nd, p, per in zip(self.n, self.srcpos[ns], self.periodic)]
        return [a for a, _ in lr], [b for _, b in lr]

    def expected_rounds(self, sources=None):
        """Sum over sources of ceil(max_d(|l_d|, r_d) / subboxsize): the rounds of sources that run to their reach."""
        total = 0
        for ns in self._sources(sources):
            l, r = self.reach(int(ns))
            total += -(-max(max(-a for a in l), max(r)) // SUBBOXSIZE)
        return total


ITER_STATE = ("xh_av", "xhe_av", "xh_intermed", "xhe_intermed")
FLUX4 = np.array([2.0e7, 1.0e7, 1.5e7, 8.0e6])


def _src(*pos):
    return np.array(pos, dtype=np.int32)


# name -> (constructor, the second, larger embedding with other padding (mesh, kind of its padding), the oracle's sum_nbox)
def case_a(pkg):
    """24^3, z open, ionised gas: two corners, an edge, an interior cell and a face; every source runs to its reach."""
    return AxisCase(pkg, (24, 24, 24), "z", (24, 24, 48), "ionised", _src((1, 1, 1), (24, 24, 24), (12, 1, 24), (7, 13, 12), (24, 12, 1)),
                    np.array([2.0e7, 1.0e7, 1.5e7, 8.0e6, 3.0e7]))


def case_b(pkg):
    """(11,24,24), x open."""
    return AxisCase(pkg, (11, 24, 24), "x", (24, 24, 24), "ionised", _src((1, 1, 1), (11, 24, 24), (6, 1, 12), (11, 13, 7)), FLUX4)


def case_c(pkg):
    """(11,11,24), x and y open."""
    return AxisCase(pkg, (11, 11, 24), "xy", (24, 24, 24), "ionised", _src((1, 1, 1), (11, 11, 24), (6, 11, 12), (3, 5, 7)), FLUX4)


def case_d(pkg):
    """(11,24,24), x and z open."""
    return AxisCase(pkg, (11, 24, 24), "xz", (24, 24, 48), "ionised", _src((1, 1, 1), (11, 24, 24), (6, 1, 12), (11, 13, 1)), FLUX4)


E_SOURCES = _src((1, 1, 1), (11, 11, 11), (5, 11, 1), (6, 6, 6))


def case_e(pkg, heat=True, seds=False):
    """11^3, z open, mixed ionisation, heating (or isothermal; or with the three SEDs of the -DPL -DQUASARS build)."""
    flux, kw = np.array([3.0e7, 8.0e6, 1.5e7, 2.0e7]), {}
    if seds:
        kw = dict(pl=np.array([1e6, 2e6, 0.0, 5e5]), qpl=np.array([0.0, 1e6, 3e6, 5e5]))
        flux = np.array([3e6, 0.0, 1e6, 2e6])
    return AxisCase(pkg, (11, 11, 11), "z", (11, 11, 24), "mixed", E_SOURCES, flux, heat=heat, **kw)


def case_f(pkg):
    """24^3, z open, opaque gas, a source two cells from the open face and one in the middle: both stop after round 1."""
    return AxisCase(pkg, (24, 24, 24), "z", (24, 24, 48), "opaque", _src((12, 12, 3), (12, 12, 12)), np.array([1.0e4, 1.0e4]))


CASES = {"A": case_a, "B": case_b, "C": case_c, "D": case_d, "E": case_e, "F": case_f}
OTHER_EMBEDDING = {"A": ((24, 24, 50), "mixed"), "B": ((26, 24, 24), "mixed"), "C": ((26, 31, 24), "mixed"), "D": ((31, 24, 50), "mixed"),
                   "E": ((11, 11, 31), "ionised"), "F": ((24, 24, 50), "opaque")}
ORACLE_SUM_NBOX = {"A": 15, "B": 8, "C": 8, "D": 12, "E": 4, "F": 2}
