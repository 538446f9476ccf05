"""Point-source hand-over across edges and corners (c2r_set_source_halo, include/c2ray_hip.h): the edge lines and the corner
of a halo, cut out of a neighbour's exit strip.  Pure NumPy; a host that assembles a tiling never re-derives the strip layout.

A STRIP of face = 2 * axis + high is (3, F): species slowest, the face cells with the lower of the two other axes fastest.
The ghost cells that a part's halo holds beyond an edge or a corner are layer cells of the part's diagonal neighbour, and
that neighbour's exit strips hold them: an edge line is the row of a strip that lies in the layer of a second face, the
corner the one cell of it that lies in the layers of two more faces.  Either of the strips that hold a cell gives the same
numbers, as for planes, where the corner line is read out of either strip.
"""
import numpy as np


def _axis_side(face):
    face = int(face)
    if not 0 <= face <= 5:
        raise ValueError(f"face {face} not in 0..5")
    return face >> 1, face & 1


def strip_grid(strip, face, mesh):
    """The strip of `face` of a mesh of `mesh` cells as (3, n_b, n_a) -- a < b the two other axes -- and (a, b)."""
    axis, _ = _axis_side(face)
    a, b = [d for d in range(3) if d != axis]
    s = np.asarray(strip, dtype=np.float64)
    if s.size != 3 * int(mesh[a]) * int(mesh[b]):
        raise ValueError(f"a strip of face {face} of mesh {tuple(mesh)} has 3 x {int(mesh[a]) * int(mesh[b])} values, not {s.size}")
    return s.reshape(3, int(mesh[b]), int(mesh[a])), (a, b)


def edge_of_strip(strip, face, mesh, other_face):
    """The edge line (3, mesh[e]) along the remaining axis e: the cells of the strip of `face` (of a mesh of `mesh` cells) that
    lie in the layer of `other_face` of the same mesh."""
    axis, _ = _axis_side(face)
    oaxis, ohigh = _axis_side(other_face)
    if oaxis == axis:
        raise ValueError(f"faces {face} and {other_face} belong to the same axis")
    grid, (a, b) = strip_grid(strip, face, mesh)
    at = int(mesh[oaxis]) - 1 if ohigh else 0
    return np.ascontiguousarray(grid[:, :, at] if oaxis == a else grid[:, at, :])


def corner_of_strip(strip, face, mesh, other_face_1, other_face_2):
    """The corner (3,): the cell of the strip of `face` that lies in the layers of the two other faces of the same mesh."""
    axis, _ = _axis_side(face)
    (a1, h1), (a2, h2) = _axis_side(other_face_1), _axis_side(other_face_2)
    if len({axis, a1, a2}) != 3:
        raise ValueError(f"faces {face}, {other_face_1} and {other_face_2} do not belong to three axes")
    grid, (a, b) = strip_grid(strip, face, mesh)
    at = {a1: int(mesh[a1]) - 1 if h1 else 0, a2: int(mesh[a2]) - 1 if h2 else 0}
    return np.ascontiguousarray(grid[:, at[b], at[a]])
