"""Cases for the point-source hand-over between meshes stacked along z (c2r_select_source_face_exit,
c2r_set_source_face_entry), used by tests/test_gpu_source_handover.py.  Not a test module.

A Stack is one deep mesh W = (n1, n2, N), open along z, with gas from tests/open_boundary_cases.py and point sources inside
it, and any PART of it: the layers z_lo..z_hi as a mesh of their own with the same gas and the same boundaries, the sources at
their positions relative to the part -- inside it, or outside beyond a z face (c2r_set_sources_external).  The reference of
every test is W itself, run by the product's open path with the sources inside.
"""
import numpy as np

import axis_boundary_cases as ab
import external_source_cases as xc

Z_LOW, Z_HIGH = 4, 5          # face = 2 * axis + high


class Stack:
    def __init__(self, pkg, n, open_axes, kind, srcpos, flux, heat=False):
        assert "z" in open_axes
        # (the embedding mesh of the oracle, which these tests never run: any that the case's checks accept)
        m = tuple(2 * nd if ax in open_axes else nd for nd, ax in zip(n, "xyz"))
        self.case = xc.ExternalCase(pkg, tuple(n), open_axes, m, kind, np.array(srcpos, dtype=np.int32).reshape(-1, 3),
                                    np.asarray(flux, dtype=np.float64), heat=heat)
        self.n = tuple(n)

    def gas(self, z_lo, z_hi):
        """[ndens, xh, xhe, temperature] of the layers z_lo..z_hi (1-based, inclusive)."""
        out = []
        for a in self.case.region:
            if a is None:
                out.append(None)
                continue
            ncomp = a.size // ab.cells(self.n)
            out.append(np.ascontiguousarray(a.reshape(ncomp, self.n[2], self.n[1], self.n[0])[:, z_lo - 1:z_hi]).reshape(-1))
        return out

    def engine(self, pkg, tables, z_lo=1, z_hi=None, sources=None, batch=None, placed=False):
        """A context of the part z_lo..z_hi (default: W) with the sources `sources` (0-based indices; default: all).  placed:
        the part is told where it lies in W (c2r_set_mesh_origin)."""
        z_hi = self.n[2] if z_hi is None else z_hi
        idx = self.case._sources(sources)
        pos = self.case.srcpos.copy()
        pos[:, 2] -= z_lo - 1
        mesh = (self.n[0], self.n[1], z_hi - z_lo + 1)
        outside = any(not 1 <= int(pos[i][2]) <= mesh[2] for i in idx)
        e = self.case._engine(pkg, tables, mesh, self.gas(z_lo, z_hi), self.case.periodic, idx, external=outside, srcpos=pos)
        if batch is not None:
            e.set_batch(batch)
        if placed:
            e.set_mesh_origin((0, 0, z_lo - 1))
        return e

    def part_of(self, grid, z_lo, z_hi):
        """The layers z_lo..z_hi of a grid of W (any number of components), flat."""
        g = np.asarray(grid)
        ncomp = g.size // ab.cells(self.n)
        return np.ascontiguousarray(g.reshape(ncomp, self.n[2], self.n[1], self.n[0])[:, z_lo - 1:z_hi]).reshape(-1)

    def layer_strip(self, cols, z):
        """The strip (3, n1 n2) that the layer z of W's downloaded columns (HipEngine.download_columns) makes."""
        hi = np.asarray(cols["coldensh_out"]).reshape(self.n[2], -1)[z - 1]
        he = np.asarray(cols["coldenshe_out"]).reshape(2, self.n[2], -1)[:, z - 1]
        return np.stack([hi, he[0], he[1]])


def one_pass(e):
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    return e.download_rates()


def part_columns(stack, cols, z_lo, z_hi):
    return {k: stack.part_of(cols[k], z_lo, z_hi) for k in ("coldensh_out", "coldenshe_out")}
