// Escape maps (c2r_enable_face_loss, include/c2ray_hip.h): which open mesh face a cell's share of
// the kept photon loss belongs to, where that face cell sits in the face's map, and the fixed order in which a map is
// added up.
//
// Faces are numbered face = 2 * axis + high: high = 0 is the face at mesh index 1, high = 1 the one at index mesh[axis].
// A face's map holds one double per face cell, the face cells in mesh order of the two remaining axes, the lower axis
// fastest (the layout of c2r_set_plane_entry_columns without the species index).  The maps of the open faces lie one
// behind the other, in face order, in one buffer.
//
// Like c2ray_shell.hpp this file compiles with a host C++ compiler: tests/face_harness.cpp runs these functions
// exhaustively on the CPU, and k_face_loss (c2ray_hip.hip) runs the same ones per lane.  Nothing here indexes an array
// with a number the compiler does not know: every loop unrolls to constant indices, so a kernel that holds mesh, offsets
// and cell sizes in registers keeps them there (no private segment).
#pragma once

#include <stddef.h>

#include "c2ray_device.hpp"

namespace c2r {

constexpr int FACE_BLOCK = 256; // face cells per block of k_face_loss and per block of the fixed-order sum

// the two remaining axes of a face across `axis`, the lower one first (it runs fastest over the face)
C2R_HD int face_axis_a(int axis) { return axis == 0 ? 1 : 0; }
C2R_HD int face_axis_b(int axis) { return axis == 2 ? 1 : 2; }

C2R_HD int face_pick(int axis, int v0, int v1, int v2) { return axis == 0 ? v0 : (axis == 1 ? v1 : v2); }

// cells of a face across `axis` of the mesh n
C2R_HD int face_cells(const int (&n)[3], int axis) { return face_pick(axis, n[1], n[0], n[0]) * face_pick(axis, n[2], n[2], n[1]); }

// where the map of `face` begins in the buffer of all open faces' maps (face = 6: the size of that buffer)
C2R_HD int face_map_offset(const int (&n)[3], const int (&open)[3], int face) {
  int off = 0;
  for (int q = 0; q < 6; q++)
    if (q < face && open[q >> 1]) off += face_cells(n, q >> 1);
  return off;
}

// The face cell of the mesh cell m (0-based) on a face across `axis`: the two other indices, the lower axis fastest.
C2R_HD int face_cell_index(const int (&n)[3], int axis, const int (&m)[3]) {
  const int a = face_pick(axis, m[1], m[0], m[0]), b = face_pick(axis, m[2], m[2], m[1]);
  return a + face_pick(axis, n[1], n[0], n[0]) * b;
}

// ... and back: the mesh cell (0-based) of face cell f of `face`
C2R_HD void face_cell_decode(const int (&n)[3], int face, int f, int (&m)[3]) {
  const int axis = face >> 1;
  const int na = face_pick(axis, n[1], n[0], n[0]);
  const int b = f / na, a = f - b * na;
  const int on = (face & 1) ? face_pick(axis, n[0], n[1], n[2]) - 1 : 0;
  m[0] = axis == 0 ? on : a;
  m[1] = axis == 1 ? on : (axis == 0 ? a : b);
  m[2] = axis == 2 ? on : b;
}

// The attribution rule.  m: the cell's 0-based mesh indices; o: its offset from the source; dr: the cell sizes.
// Candidates are (d, low) for every open axis d with m[d] on the mesh's first layer and (d, high) with m[d] on its last.
// A cell without candidate belongs to no face (-1).  Of several candidates the one whose axis has the largest
// |o[d]| * dr[d] (compared as doubles, the product as written) -- the face the ray from the source leaves through --, on
// a tie the lowest axis, within one axis (a mesh one cell deep) low before high.
C2R_HD int face_of_cell(const int (&n)[3], const int (&open)[3], const int (&m)[3], const int (&o)[3], const double (&dr)[3]) {
  int best = -1;
  double best_w = -1.0;
  for (int d = 0; d < 3; d++) {
    if (!open[d] || !(m[d] == 0 || m[d] == n[d] - 1)) continue;
    const double w = (double)(o[d] < 0 ? -o[d] : o[d]) * dr[d];
    if (w > best_w) { best_w = w; best = d; }
  }
  if (best < 0) return -1;
  return 2 * best + (m[best] == 0 ? 0 : 1);
}

// The fixed order of c2r_get_face_loss, the shape of the device's loss sums (block_sum and k_loss_finish, c2ray_hip.hip):
// a block of 256 consecutive values is added by a tree -- per 64 values x[l] += x[l + off] for off = 32, 16, .. 1, then
// the four results in order --, lane t of the final block adds the block sums t, t + 256, .. in order, and the same tree
// adds the lanes.
inline double face_block_tree(const double *v, size_t count) {
  double x[FACE_BLOCK];
  for (int t = 0; t < FACE_BLOCK; t++) x[t] = (size_t)t < count ? v[t] : 0.0;
  double r = 0.0;
  for (int w = 0; w < FACE_BLOCK / 64; w++) {
    double *y = x + 64 * w;
    for (int off = 32; off > 0; off >>= 1)
      for (int l = 0; l < off; l++) y[l] += y[l + off];
    r += y[0];
  }
  return r;
}
inline double face_sum(const double *map, size_t n) {
  double lane[FACE_BLOCK];
  for (int t = 0; t < FACE_BLOCK; t++) lane[t] = 0.0;
  const size_t nblk = (n + FACE_BLOCK - 1) / FACE_BLOCK;
  for (size_t b = 0; b < nblk; b++) {
    const size_t left = n - b * FACE_BLOCK;
    lane[b % FACE_BLOCK] += face_block_tree(map + b * FACE_BLOCK, left < (size_t)FACE_BLOCK ? left : (size_t)FACE_BLOCK);
  }
  return face_block_tree(lane, FACE_BLOCK);
}

} // namespace c2r
