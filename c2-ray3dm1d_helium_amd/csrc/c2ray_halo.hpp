// Source halos (c2r_set_source_halo, include/c2ray_hip.h): which array of a point source's halo, and
// which entry of it, a box cell OUTSIDE the mesh stores as N_out.
//
// The source stands outside the mesh along the axes of B (1 to 3 of them).  ghost_d is the 0-based ghost index along axis d:
// -1 where the source stands below the mesh, mesh_d where it stands above, HALO_INSIDE where it stands inside along d.  A
// cell at 0-based mesh index x lies outside the mesh along the axes of O (not empty: the caller has asked).  It is a GHOST
// cell iff x_d == ghost_d for every d in O -- HALO_INSIDE is no index of any cell, so O is then a subset of B -- and reads
//   |O| = 1, O = {d}:  the face strip of axis d (array d) at the face cell, the lower of the two other axes fastest,
//                      species stride F = the face's cells;
//   |O| = 2:           the edge line along the remaining axis e (array 3 + e) at x_e, species stride mesh_e;
//   |O| = 3:           the corner (array 6) at 0, species stride 1.
// Every other cell outside the mesh is a vacuum cell (class 0).
//
// Like c2ray_curve.hpp this file compiles with a host C++ compiler: tests/halo_harness.cpp runs halo_classify on the CPU over
// every cell of a box around a mesh, and the halo sweep kernels of c2ray_hip.hip run the same function per lane.  The cell is
// classified with selects on values: an array indexed by the axis would go to scratch memory.
#pragma once

#include <stddef.h>
#include <limits.h>

#include "c2ray_device.hpp"

namespace c2r {

constexpr int HALO_INSIDE = INT_MIN; // ghost index of an axis along which the source stands inside the mesh
constexpr int HALO_ARRAYS = 7;       // face strips 0..2 (by axis), edge lines 3..5 (3 + axis), the corner 6

// 0-based ghost index of axis d for a source at 1-based position pos along a mesh of n cells
C2R_HD int halo_ghost_index(int pos, int n) { return pos > n ? n : (pos < 1 ? -1 : HALO_INSIDE); }

// The class of the cell (i, j, k) (0-based, outside the mesh along at least one axis): 0 vacuum, else |O|; for a ghost cell
// also the array, the entry within one species of it and the stride from one species to the next.
C2R_HD int halo_classify(int i, int j, int k, int n1, int n2, int n3, int g0, int g1, int g2, int &array, size_t &entry, size_t &stride) {
  const bool o0 = (unsigned)i >= (unsigned)n1, o1 = (unsigned)j >= (unsigned)n2, o2 = (unsigned)k >= (unsigned)n3;
  if ((o0 && i != g0) || (o1 && j != g1) || (o2 && k != g2)) return 0;
  const int nout = (int)o0 + (int)o1 + (int)o2;
  if (nout == 1) {
    const int d = o0 ? 0 : (o1 ? 1 : 2);
    const int xa = d == 0 ? j : i, xb = d == 2 ? j : k; // the two other axes, the lower one first
    const int na = d == 0 ? n2 : n1, nb = d == 2 ? n2 : n3;
    array = d;
    entry = (size_t)xa + (size_t)na * (size_t)xb;
    stride = (size_t)na * (size_t)nb;
  } else if (nout == 2) {
    const int e = !o0 ? 0 : (!o1 ? 1 : 2);
    array = 3 + e;
    entry = (size_t)(e == 0 ? i : (e == 1 ? j : k));
    stride = (size_t)(e == 0 ? n1 : (e == 1 ? n2 : n3));
  } else {
    array = 6;
    entry = 0;
    stride = 1;
  }
  return nout;
}

} // namespace c2r
