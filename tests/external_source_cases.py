"""Cases for point sources outside the mesh (c2r_set_sources_external), shared by tests/test_external_sources_oracle.py (CPU)
and tests/test_gpu_external_sources.py (GPU).  Not a test module.

The reference.  A product run on an open region n whose sources may stand outside it equals, bit for bit on the region's
cells, the oracle's PERIODIC run on a mesh m with
  * m_d >= 2 * (the largest virtual extent along d: region and sources together) on the open axes, m_d == n_d on the periodic
    ones, and (m_z/2 - 1) mod 10 != 0,
  * the region at the mesh origin and ndens = 0 everywhere else -- vacuum,
  * every source at its position AS GIVEN, positions <= 0 included: the oracle wraps cells with fmodulo and hands the source
    position to cinterp unwrapped.
(tests/open_boundary_cases.py has the argument for sources inside; tests/test_external_sources_oracle.py checks this premise on
the oracle alone.)  The oracle's vacuum cells hold 0/0 and are never compared.

The oracle's own sum_nbox and photon_loss follow its periodic, z-only rule and are no reference for those two.  Theirs is the
product's pinned open path on the VIRTUAL mesh: the region extended by ndens = 0 cells up to the bounding box of region and
sources, so that every source stands inside, set with c2r_set_sources (ExternalCase.virtual_engine).  That run traces the same
cells with the same block numbering.  Where a source stands beyond a LOW face the virtual mesh has to shift the region, and
cinterp forms its crossing points from absolute coordinates: virtual_shift() says by how much.
"""
import numpy as np

import axis_boundary_cases as ab
import open_boundary_cases as ob

SUBBOXSIZE = ob.SUBBOXSIZE
MAX_SUBBOX = 1150
embed, extract, gas = ob.embed, ob.extract, ob.gas          # (cubes; embed3 / extract3 of axis_boundary_cases for the others)


def external_reach(mesh, pos, periodic, max_subbox=MAX_SUBBOX):
    """(l, r) of include/c2ray_hip.h for one axis of a source that may stand outside the mesh."""
    if periodic:
        return -min(max_subbox, mesh // 2), min(max_subbox, mesh // 2 - 1 + mesh % 2)
    return -min(max_subbox, max(pos - 1, 0)), min(max_subbox, max(mesh - pos, 0))


class ExternalCase(ab.AxisCase):
    """An AxisCase whose sources may stand outside the region along its open axes; the embedding is vacuum around the region."""

    def virtual_bounds(self, sources=None):
        """(lo, hi), 1-based and inclusive: the bounding box of the region and the sources along each axis."""
        pos = self.srcpos[self._sources(sources)]
        lo = [min(1, int(pos[:, d].min())) for d in range(3)]
        hi = [max(int(self.n[d]), int(pos[:, d].max())) for d in range(3)]
        return lo, hi

    def check_embedding(self, m):
        # the largest virtual extent: of the region together with ONE source (each source sees the region within the
        # periodic reach of the mesh m on its own)
        ext = list(self.n)
        for ns in range(len(self.srcpos) if hasattr(self, "srcpos") else 0):
            lo, hi = self.virtual_bounds([ns])
            ext = [max(e, h - l + 1) for e, l, h in zip(ext, lo, hi)]
        for nd, md, per, e in zip(self.n, m, self.periodic, ext):
            assert md == nd if per else md >= 2 * e, (self.n, m, self.periodic, ext)
        assert (m[2] // 2 - 1) % SUBBOXSIZE != 0

    def embedding(self, pkg, m, pad_seed, pad_kind):
        """The region at the origin of the mesh m; fractions (and temperatures) of `pad_kind` gas around it, density 0.0."""
        big = super().embedding(pkg, m, pad_seed, pad_kind)
        big[0] = ab.embed3(self.region[0], self.n, m, np.zeros(ab.cells(m)))
        return big

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.check_embedding(self.m)         # (now that the sources are known)
        for p in self.srcpos:
            assert all((1 <= int(p[d]) <= self.n[d]) or not self.periodic[d] for d in range(3)), p

    def is_external(self, ns):
        return any(not 1 <= int(self.srcpos[ns][d]) <= self.n[d] for d in range(3))

    # -- the product ---------------------------------------------------------------------------------------------------
    def _engine(self, pkg, tables, mesh, gas_, boundaries, idx, external=True, srcpos=None):
        hp = pkg.hostphys
        ndens, xh, xhe, temp = gas_
        mat = pkg.Material(ndens, xh.copy(), xhe.copy(), None if temp is None else temp.copy(), not self.heat, 1.0e4, 1.0, self.reccoef)
        src = pkg.SourceProps((self.srcpos if srcpos is None else srcpos)[idx], self.flux[idx], self.s_star)
        if self.pl is not None:
            src.NormFluxPL, src.pl_S_star = self.pl[idx], self.pl_s_star
            src.NormFluxQPL, src.qpl_S_star = self.qpl[idx], self.qpl_s_star
        e = pkg.HipEngine(tuple(mesh), 0)
        if boundaries is not None:
            e.set_boundaries(boundaries)
        e.set_tables(tables)
        e.set_step(mat, pkg.GridProps(tuple(mesh), self.dr, self.vol), pkg.Cosmology(ab.ZRED, hp.H0, hp.Omega0))
        if external:
            e.set_sources_external(src)
        else:
            e.set_sources(src)
        e.upload_state(mat)
        return e

    def periodic_engine_on_m(self, pkg, tables, sources=None):
        raise NotImplementedError("a periodic context refuses a source outside the mesh")

    def virtual_shift(self, sources=None):
        lo, _ = self.virtual_bounds(sources)
        return [1 - x for x in lo]

    def virtual_engine(self, pkg, tables, sources=None, lls_grid=None):
        """The pinned open path: an open context (this case's boundaries) of the virtual mesh, the region inside it at
        virtual_shift(), vacuum around it, the sources shifted likewise and set with c2r_set_sources.  Returns (engine, mesh).
        lls_grid: a REAL(4) fog grid of the region, 0 in the vacuum."""
        lo, hi = self.virtual_bounds(sources)
        v = tuple(hi[d] - lo[d] + 1 for d in range(3))
        sh = self.virtual_shift(sources)
        pad = ob.gas(pkg, ab.cells(v), np.random.default_rng(ab.PAD_SEED + 1), self.kind, self.heat)
        gas_ = []
        for a, b in zip(self.region, pad):
            if a is None:
                gas_.append(None)
                continue
            ncomp = a.size // ab.cells(self.n)
            out = (np.zeros(b.size) if a is self.region[0] else b).reshape(ncomp, v[2], v[1], v[0]).copy()
            out[:, sh[2]:sh[2] + self.n[2], sh[1]:sh[1] + self.n[1], sh[0]:sh[0] + self.n[0]] = a.reshape(ncomp, self.n[2], self.n[1], self.n[0])
            gas_.append(out.reshape(-1))
        srcpos = self.srcpos + np.array(sh, dtype=np.int32)
        e = self._engine(pkg, tables, v, gas_, self.periodic, self._sources(sources), external=False, srcpos=srcpos)
        if lls_grid is not None:
            fog = np.zeros((v[2], v[1], v[0]), dtype=np.float32)
            fog[sh[2]:sh[2] + self.n[2], sh[1]:sh[1] + self.n[1], sh[0]:sh[0] + self.n[0]] = np.asarray(lls_grid, dtype=np.float32).reshape(self.n[2], self.n[1], self.n[0])
            mat = pkg.Material(gas_[0], gas_[1], gas_[2], gas_[3], not self.heat, 1.0e4, 1.0, self.reccoef)
            mat.use_LLS, mat.LLS_grid = True, fog.reshape(-1)
            e.set_lls(mat)
        return e, v

    def extract_virtual(self, grid, v, sources=None):
        """The region's cells of a grid of the virtual mesh v."""
        sh = self.virtual_shift(sources)
        grid = np.asarray(grid)
        ncomp = grid.size // ab.cells(v)
        g = grid.reshape(ncomp, v[2], v[1], v[0])
        return np.ascontiguousarray(g[:, sh[2]:sh[2] + self.n[2], sh[1]:sh[1] + self.n[1], sh[0]:sh[0] + self.n[0]]).reshape(-1)

    # -- the oracle, source by source --------------------------------------------------------------------------------------
    # The oracle's while-test (evolve_source.F90:136-139) counts what leaves through every face of its box, the faces that
    # lie in the vacuum included, so a source outside the region always runs to the oracle's reach.  The product's test runs
    # over the faces that can still move, and a box stops where the gas has absorbed the light.  So the grids of a case
    # whose gas may stop a box are COMPOSED, as tests/beam_reference.py composes its own: every source alone through
    # orc.do_source from zeroed grids, cut to the cells the source traces -- its final box, known from the rounds of the
    # product's pinned open path on the virtual mesh (c2r_set_sources) --, folded in source order from 0.0.
    def _oracle_step(self, pkg, orc, lls_grid=None):
        hp = pkg.hostphys
        nd, xh, xhe, temp = self.big
        kw = {}
        if self.pl is not None:
            kw = dict(normflux_pl=self.pl, normflux_qpl=self.qpl, pl_s_star=self.pl_s_star, qpl_s_star=self.qpl_s_star)
        if lls_grid is not None:     # the fog of the region, none in the vacuum
            kw["lls_grid"] = ab.embed3(np.asarray(lls_grid, dtype=np.float32), self.n, self.m, np.zeros(ab.cells(self.m), dtype=np.float32))
        st = orc.Step(self.m, self.dr, self.vol, ab.ZRED, hp.H0, hp.Omega0, not self.heat, 1.0e4, 1.0, self.srcpos, self.flux, self.s_star,
                      nd, self.reccoef, **kw)
        s = orc.State(st, xh, xhe, temp)
        orc.begin_step(s)
        return st, s

    def box_mask(self, ns, nbox):
        """Flat bool array over the region (i fastest): the cells of source ns (0-based) after nbox rounds."""
        l, r = self.reach(ns)
        axes = []
        for d in range(3):
            m1 = np.arange(1, self.n[d] + 1, dtype=np.int64)
            if self.periodic[d]:
                h = self.n[d] // 2
                off = (m1 - int(self.srcpos[ns][d]) + h) % self.n[d] - h
            else:
                off = m1 - int(self.srcpos[ns][d])
            axes.append((off >= max(l[d], -SUBBOXSIZE * nbox)) & (off <= min(r[d], SUBBOXSIZE * nbox)) & (nbox > 0))
        return (axes[2][:, None, None] & axes[1][None, :, None] & axes[0][None, None, :]).reshape(-1)

    def compose(self, pkg, orc, otables, rounds, lls_grid=None, dt=None):
        """The grids folded over the sources in order, source ns cut to its box after rounds[ns] rounds; with dt, the
        oracle's global pass on those grids as well."""
        ncell = ab.cells(self.n)
        out = dict(phih_grid=np.zeros(ncell), phihe_grid=np.zeros(2 * ncell), phiheat=np.zeros(ncell))
        attrs = (("phih", "phih_grid"), ("phihe", "phihe_grid"), ("phiheat", "phiheat"))
        with np.errstate(all="ignore"):     # (the oracle's vacuum cells hold 0/0; they are never read)
            for ns in range(len(self.flux)):
                st, s = self._oracle_step(pkg, orc, lls_grid)
                orc.do_source(otables, st, s, ns + 1)
                inside = self.box_mask(ns, rounds[ns])
                for a, k in attrs:
                    term = ab.extract3(getattr(s, a), self.n, self.m)
                    out[k] = out[k] + np.where(np.tile(inside, term.size // ncell), term, 0.0)
            if dt is not None:
                st, s = self._oracle_step(pkg, orc, lls_grid)
                for a, k in attrs:
                    getattr(s, a)[:] = ab.embed3(out[k], self.n, self.m, np.zeros(getattr(s, a).size))
                orc.global_pass(otables, st, s, dt)
                for k in ab.ITER_STATE:
                    out[k] = ab.extract3(getattr(s, k), self.n, self.m)
        return out

    # -- what the product is expected to report --------------------------------------------------------------------------
    def reach(self, ns):
        lr = [external_reach(nd, int(p), per) for nd, p, per in zip(self.n, self.srcpos[ns], self.periodic)]
        return [a for a, _ in lr], [b for _, b in lr]


def _src(*pos):
    return np.array(pos, dtype=np.int32)


# -- the premise's own cases: n = 8 ------------------------------------------------------------------------------------------
PREMISE_SOURCES = {"beyond_high": [(4, 5, 11)], "beyond_low": [(4, 5, -2)], "beyond_an_edge": [(11, 5, -1)],
                   "outside_and_inside": [(4, 5, 11), (3, 3, 3)]}


def case_premise(pkg, kind_of_position, m=24):
    pos = PREMISE_SOURCES[kind_of_position]
    return ExternalCase(pkg, (8, 8, 8), "xyz", (m, m, m), "mixed", _src(*pos), np.array([3.0e7, 1.5e7][:len(pos)]))


# -- one round, every kind of position: n = 11, M = 32 -------------------------------------------------------------------
ONE_N, ONE_M = 11, 32
_INSIDE = (4, 5, 7)      # the coordinates along the axes on which a source stands inside


def _beyond(axis, high, dist):
    p = list(_INSIDE)
    p[axis] = ONE_N + dist if high else 1 - dist
    return tuple(p)


ONE_ROUND_SOURCES = {f"{'xyz'[a]}{'+' if h else '-'}{d}": [_beyond(a, h, d)] for a in range(3) for h in (0, 1) for d in (1, 4)}
ONE_ROUND_SOURCES["edge"] = [(-1, 13, 6)]
ONE_ROUND_SOURCES["corner"] = [(13, -2, 14)]
ONE_ROUND_SOURCES["all"] = [p[0] for p in list(ONE_ROUND_SOURCES.values())] + [(3, 3, 3), (8, 6, 9)]


def case_one_round(pkg, which, heat=False, seds=False):
    pos = ONE_ROUND_SOURCES[which] if isinstance(which, str) else list(which)
    rng = np.random.default_rng(1100 + len(pos))
    flux, kw = rng.uniform(5.0e6, 3.0e7, len(pos)), {}
    if seds:
        kw = dict(pl=rng.uniform(5.0e5, 2.0e6, len(pos)), qpl=rng.uniform(5.0e5, 3.0e6, len(pos)))
        flux = flux / 10.0
    return ExternalCase(pkg, (ONE_N,) * 3, "xyz", (ONE_M,) * 3, "mixed", _src(*pos), flux, heat=heat, **kw)


TWO_EXTERNAL = [(4, 5, 13), (-1, 6, 3)]       # the heating cases: beyond +z and beyond -x


# -- several rounds: n = 24, M = 64 --------------------------------------------------------------------------------------
SEVERAL_SOURCES = [(12, 12, 30), (-2, 7, 13), (7, 13, 12)]     # 6 cells beyond +z, 3 cells beyond -x, one inside


def case_several_rounds(pkg, sources=SEVERAL_SOURCES):
    return ExternalCase(pkg, (24, 24, 24), "xyz", (64, 64, 64), "ionised", _src(*sources), np.array([2.0e7, 1.5e7, 1.0e7][:len(sources)]))


def case_early_stop(pkg):
    """(24, 11, 11), opaque gas, a source 2 cells beyond the -x face at the middle of it: the side faces of its first box are
    mesh faces (5 cells away), so the one face that can still move lies behind nine cells of gas, and it stops after its
    first round.  (On a wider mesh the side faces of the first box could still move, and through their two columns of vacuum
    cells the light leaves unabsorbed: the source would sweep on.)"""
    return ExternalCase(pkg, (24, 11, 11), "xyz", (64, 24, 24), "opaque", _src((-1, 6, 6)), np.array([1.0e4]))


def case_mixed_boundaries(pkg):
    """Periodic in x and y, open in z, a source 3 cells beyond +z and one inside; the oracle on (n, n, M)."""
    return ExternalCase(pkg, (24, 24, 11), "z", (24, 24, 32), "ionised", _src((5, 20, 14), (12, 7, 4)), np.array([2.0e7, 1.0e7]))
