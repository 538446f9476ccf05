"""Cases for the point-source hand-over across edges and corners (c2r_set_source_halo), used by tests/test_gpu_source_halo.py
and tests/test_source_halo_host.py.  Not a test module.

tests/source_handover_cases.py cuts a deep mesh W along z; a Tiling cuts it along any axes.  W = (n1, n2, n3) is open along the
axes it is cut along (and any others named), has gas from tests/open_boundary_cases.py and point sources inside it.  A PART is the
box lo..hi (1-based, inclusive, per axis) of W as a mesh of its own, with the same gas and boundaries, placed with
c2r_set_mesh_origin (origin = lo - 1), the sources at their positions relative to the part -- inside it or outside beyond one, two
or three faces (c2r_set_sources_external).  The reference of every test is W itself, run by the product's open path with the
sources inside (c2r_set_sources).

halo_of_deep cuts a part's halo out of W's own downloaded columns ("deep"); run_tiling runs a tiling of two parts per cut axis
as a host would, every part taking what its neighbours towards the source hand over ("handed").
"""
import itertools

import numpy as np

import axis_boundary_cases as ab
import external_source_cases as xc
from source_handover_cases import one_pass  # noqa: F401  (the pass of every test)

X_LOW, X_HIGH, Y_LOW, Y_HIGH, Z_LOW, Z_HIGH = range(6)          # face = 2 * axis + high
COLS = ("coldensh_out", "coldenshe_out")


def ran_to_reach(trace):
    return trace["box_lo"] == trace["reach_l"] and trace["box_hi"] == trace["reach_r"]


class Tiling:
    def __init__(self, pkg, n, open_axes, kind, srcpos, flux, heat=False):
        # (the embedding mesh of the oracle, which these tests never run: any that the case's checks accept)
        m = tuple(2 * nd if ax in open_axes else nd for nd, ax in zip(n, "xyz"))
        self.case = xc.ExternalCase(pkg, tuple(n), open_axes, m, kind, np.array(srcpos, dtype=np.int32).reshape(-1, 3),
                                    np.asarray(flux, dtype=np.float64), heat=heat)
        self.n = tuple(n)
        self.whole = ((1, 1, 1), self.n)

    def _box(self, a, lo, hi):
        """The cells lo..hi of an array of W with any number of components, as (ncomp, z, y, x)."""
        a = np.asarray(a)
        g = a.reshape(a.size // ab.cells(self.n), self.n[2], self.n[1], self.n[0])
        return g[:, lo[2] - 1:hi[2], lo[1] - 1:hi[1], lo[0] - 1:hi[0]]

    def gas(self, lo, hi):
        """[ndens, xh, xhe, temperature] of the part lo..hi."""
        return [None if a is None else np.ascontiguousarray(self._box(a, lo, hi)).reshape(-1) for a in self.case.region]

    def shifted(self, lo):
        """The sources' positions relative to a part that begins at lo."""
        return self.case.srcpos - (np.array(lo, dtype=np.int32) - 1)

    def engine(self, pkg, tables, lo=None, hi=None, sources=None, batch=None, placed=True):
        """A context of the part lo..hi (default: W) with the sources `sources` (0-based indices; default: all); placed: told
        where it lies in W (c2r_set_mesh_origin)."""
        lo, hi = (self.whole[0] if lo is None else tuple(lo)), (self.whole[1] if hi is None else tuple(hi))
        for d in range(3):
            assert 1 <= lo[d] <= hi[d] <= self.n[d] and (not self.case.periodic[d] or (lo[d], hi[d]) == (1, self.n[d])), (lo, hi)
        idx = self.case._sources(sources)
        pos = self.shifted(lo)
        mesh = tuple(h - l + 1 for l, h in zip(lo, hi))
        outside = any(not 1 <= int(pos[i][d]) <= mesh[d] for i in idx for d in range(3))
        e = self.case._engine(pkg, tables, mesh, self.gas(lo, hi), self.case.periodic, idx, external=outside, srcpos=pos)
        if batch is not None:
            e.set_batch(batch)
        if placed and tuple(lo) != (1, 1, 1):
            e.set_mesh_origin(tuple(l - 1 for l in lo))
        return e

    def part_of(self, grid, lo, hi):
        """The cells lo..hi of a grid of W (any number of components), flat."""
        return np.ascontiguousarray(self._box(grid, lo, hi)).reshape(-1)

    def cells(self, cols, fixed, lo, hi):
        """(3, n): W's outgoing columns (HipEngine.download_columns) of the cells whose index along axis d is fixed[d] for the
        axes named there and runs over lo..hi along the others, the lowest free axis fastest: the strip of a face (one axis
        fixed), an edge line (two) or a corner (three) in the layout c2r_set_source_halo takes."""
        l, h = list(lo), list(hi)
        for d, at in fixed.items():
            assert 1 <= at <= self.n[d], (d, at)
            l[d] = h[d] = at
        hi_ = self._box(cols["coldensh_out"], l, h).reshape(-1)
        he = self._box(cols["coldenshe_out"], l, h).reshape(2, -1)
        return np.stack([hi_, he[0], he[1]])

    def layer_strip(self, cols, face, lo=None, hi=None):
        """The strip (3, F) that the layer of `face` of the part lo..hi (default: W) makes of W's downloaded columns."""
        lo, hi = (self.whole[0] if lo is None else lo), (self.whole[1] if hi is None else hi)
        axis, high = face >> 1, face & 1
        return self.cells(cols, {axis: hi[axis] if high else lo[axis]}, lo, hi)

    def beyond(self, lo, hi, ns=0):
        """{axis: high} for the axes along which source ns stands outside the part lo..hi."""
        p = self.case.srcpos[ns]
        return {d: int(p[d] > hi[d]) for d in range(3) if not lo[d] <= int(p[d]) <= hi[d]}

    def halo_of_deep(self, cols, lo, hi, ns=0):
        """dict(faces, edges, corner) of the part lo..hi for source ns, cut from W's own columns: every ghost cell is a cell of W."""
        B = self.beyond(lo, hi, ns)
        ghost = {d: hi[d] + 1 if h else lo[d] - 1 for d, h in B.items()}
        faces = {2 * d + h: self.cells(cols, {d: ghost[d]}, lo, hi) for d, h in B.items()}
        edges = {}
        for e in range(3):
            a, b = [d for d in range(3) if d != e]
            if a in B and b in B:
                edges[e] = self.cells(cols, {a: ghost[a], b: ghost[b]}, lo, hi)
        corner = self.cells(cols, ghost, lo, hi).reshape(3) if len(B) == 3 else None
        return dict(faces=faces, edges=edges, corner=corner)

    # -- a tiling of two parts per cut axis ------------------------------------------------------------------------------
    def parts(self, cuts):
        """{t: (lo, hi)} for cuts = {axis: c} (the cut lies between c and c + 1): t_d = 0 for the low part along d, 1 for the
        high one, 0 along an axis that is not cut."""
        out = {}
        for t in itertools.product(*[(0, 1) if d in cuts else (0,) for d in range(3)]):
            lo = tuple(cuts[d] + 1 if t[d] else 1 for d in range(3))
            hi = tuple(self.n[d] if (t[d] or d not in cuts) else cuts[d] for d in range(3))
            out[t] = (lo, hi)
        return out


def set_halo(e, halo, rounds, ns=1):
    e.set_source_halo(ns, faces=halo["faces"], edges=halo["edges"], corner=halo["corner"], rounds=rounds)


def collect(e, ns=1):
    """One pass of a part: its rate grids, outgoing columns and the trace of source ns."""
    out = one_pass(e)
    out.update(e.download_columns())
    out["trace"] = e.source_trace(ns)
    return out


def run_tiling(pkg, tables, tiling, cuts, rounds, batch=None):
    """The cascade a host runs for source 1 of `tiling` cut at `cuts`: the part that holds the source first, then the parts
    beyond one face of it, two, three.  Every part selects the source for exit through its faces towards parts further from the
    source, and takes from the parts nearer to it the strips through their faces towards itself (c2r_set_source_face_entry for one
    face, c2r_set_source_halo for several), the edge lines and the corner cut from the diagonal neighbours' strips
    (handover.edge_of_strip, corner_of_strip), with W's rounds.  Returns {t: dict(rates, columns, trace, halo, strips, lo, hi)}."""
    ho = pkg.handover
    parts = tiling.parts(cuts)
    src = tuple(int(tiling.case.srcpos[0][d] > cuts[d]) if d in cuts else 0 for d in range(3))
    done = {}

    def flip(t, axes):
        return tuple(1 - t[d] if d in axes else t[d] for d in range(3))

    for t in sorted(parts, key=lambda t: sum(a != b for a, b in zip(t, src))):
        lo, hi = parts[t]
        mesh = tuple(h - l + 1 for l, h in zip(lo, hi))
        B = {d: src[d] for d in range(3) if t[d] != src[d]}             # axis -> the side the source stands on
        assert B == tiling.beyond(lo, hi)
        out_face = {d: 2 * d + (1 - src[d]) for d in cuts}                # the face through which a part nearer the source hands on along d
        e = tiling.engine(pkg, tables, lo, hi, batch=batch)
        exits = [out_face[d] for d in cuts if t[d] == src[d]]
        for f in exits:
            e.select_source_face_exit(f, [1])
        halo = None
        if B:
            halo = dict(faces={}, edges={}, corner=None)
            for d, h in B.items():
                halo["faces"][2 * d + h] = done[flip(t, {d})]["strips"][out_face[d]]
            for ax in range(3):
                a, b = [d for d in range(3) if d != ax]
                if a in B and b in B:
                    nb = done[flip(t, {a, b})]
                    nmesh = tuple(h - l + 1 for l, h in zip(nb["lo"], nb["hi"]))
                    line = ho.edge_of_strip(nb["strips"][out_face[a]], out_face[a], nmesh, out_face[b])
                    # (the same line out of the neighbour's other strip)
                    assert np.array_equal(line, ho.edge_of_strip(nb["strips"][out_face[b]], out_face[b], nmesh, out_face[a])), (t, ax)
                    halo["edges"][ax] = line
            if len(B) == 3:
                nb = done[flip(t, {0, 1, 2})]
                nmesh = tuple(h - l + 1 for l, h in zip(nb["lo"], nb["hi"]))
                halo["corner"] = ho.corner_of_strip(nb["strips"][out_face[0]], out_face[0], nmesh, out_face[1], out_face[2])
                for f, g1, g2 in ((1, 0, 2), (2, 0, 1)):
                    assert np.array_equal(halo["corner"], ho.corner_of_strip(nb["strips"][out_face[f]], out_face[f], nmesh, out_face[g1], out_face[g2]))
            if len(B) == 1:     # one face: the call that existed
                (face, strip), = halo["faces"].items()
                e.set_source_face_entry(1, face, strip, rounds)
            else:
                set_halo(e, halo, rounds)
        res = collect(e)
        res.update(lo=lo, hi=hi, mesh=mesh, halo=halo, strips={})
        for f in exits:
            strip, r, reached = e.download_source_face_exit(f, 1)
            assert reached, (t, f)
            res["strips"][f] = strip
        e.close()
        done[t] = res
    return done


# -- the ghost classification, restated (tests/test_source_halo_host.py) ------------------------------------------------------
def classify(mesh, srcpos, i, j, k):
    """The header's rule in NumPy for cells at 0-based mesh indices (i, j, k) (arrays), all outside the mesh: (class, array,
    entry, stride) per cell -- class 0 (vacuum; array, entry and stride then -1) or |O|; array: axis of the face strip, 3 +
    axis of the edge line, 6 for the corner; entry within one species; stride from one species to the next."""
    x = [np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64), np.asarray(k, dtype=np.int64)]
    n = [int(v) for v in mesh]
    B = {d: int(srcpos[d] > n[d]) for d in range(3) if not 1 <= srcpos[d] <= n[d]}
    m = [v + 1 for v in x]                                        # 1-based, as the rule is written
    out_ = [(m[d] < 1) | (m[d] > n[d]) for d in range(3)]
    ghost = np.ones(x[0].shape, dtype=bool)
    for d in range(3):
        g = (n[d] + 1 if B[d] else 0) if d in B else None
        ghost &= ~out_[d] | (False if g is None else m[d] == g)
    nout = out_[0].astype(np.int64) + out_[1] + out_[2]
    assert np.all(nout >= 1)
    cls = np.where(ghost, nout, 0)
    array = np.full(x[0].shape, -1, dtype=np.int64)
    entry = np.full(x[0].shape, -1, dtype=np.int64)
    stride = np.full(x[0].shape, -1, dtype=np.int64)
    for d in range(3):                                             # a face strip: the lower of the two other axes fastest
        a, b = [c for c in range(3) if c != d]
        sel = (cls == 1) & out_[d]
        array[sel], entry[sel], stride[sel] = d, (x[a] + n[a] * x[b])[sel], n[a] * n[b]
    for e in range(3):                                             # an edge line along e
        a, b = [c for c in range(3) if c != e]
        sel = (cls == 2) & out_[a] & out_[b]
        array[sel], entry[sel], stride[sel] = 3 + e, x[e][sel], n[e]
    sel = cls == 3
    array[sel], entry[sel], stride[sel] = 6, 0, 1
    return cls, array, entry, stride
