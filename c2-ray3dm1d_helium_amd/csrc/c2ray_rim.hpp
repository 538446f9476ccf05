// Horizon loss (c2r_enable_horizon_loss, include/c2ray_hip.h): what crosses a point source's photon
// horizon (c2ray_horizon.hpp), per source.  The cells within the horizon are a closed staircase around the source; its
// boundary is made of cell faces whose solid angles add up to 4 pi, so a weight per EXPOSED FACE, taken at the face centre,
// tiles the sphere (measured sum of the weights: DESIGN.md section 3.1).
//
// For one point source with a finite horizon: R2, the dr of the pass and the final sub-box lo[3]..hi[3] (offsets from the
// source, as in its device record).
//
// Sheets.  Six sheets, fc = 2*d + (s > 0 ? 1 : 0) for axis d and sign s = -1, +1: the face numbering of the escape maps
// (c2ray_face.hpp).  Sheet fc has one entry per pair of transverse offsets (oa, ob); the two other axes are a < b, a
// fastest; the offsets run over the box's extents E_a = hi_a - lo_a + 1 and E_b; the entry index is
// (oa - lo_a) + E_a*(ob - lo_b).  The six sheets lie one behind the other in face order: T = 2*(E1*E2 + E0*E2 + E0*E1).
//
// The face of a sheet column.  Along the column cells have the offset o_d = s*k, k = 0, 1, ...  horizon_within forms d2
// rounded as written and is monotone in k, so the within-cells of a column are a prefix.  If the k = 0 cell is not within,
// the column has no face.  Otherwise k* is the largest k whose cell is within and inside the box, and the cell at k* is the
// column's cell.  The column has a face iff
//   * the cell is not on the surface of the final box on any axis: lo_e < o_e < hi_e for all e (a surface cell gives its
//     term to the kept loss already),
//   * the cell at k* + 1 is not within, and
//   * cut_lit lights the cell (a beam-unlit cell has no face).
// The two sheets of an axis both see the k = 0 cell; each owns its own face of it.
//
// Weight: the solid angle over 4 pi of that face seen from the source, at the face centre; every product and sum rounded as
// written and evaluated from the left, no contraction (pi: the project's constant, c2ray_device.hpp):
//     xa = dr_a*(double)oa     xb = dr_b*(double)ob     fd = dr_d*((double)k* + 0.5)
//     f2 = (xa*xa + xb*xb) + fd*fd
//     w  = ((dr_a*dr_b)*fd) / ((4.0*pi)*(f2*sqrt(f2)))
// The source's own cell (oa = ob = 0, k* = 0) takes w = 1.0/6.0 instead.
//
// Term: po * w, po the photo_out of the cell from its six stored columns (0.0 where N_in(HI) >= max_coldensh); a column
// without a face has the term +0.0.  The T terms of a source are added in the fixed order of face_sum (c2ray_face.hpp).
//
// Like c2ray_horizon.hpp this file compiles with a host C++ compiler: tests/rim_harness.cpp runs these functions on the CPU
// over every sheet column of a box, and k_horizon_rim (c2ray_hip.hip) runs the same ones per lane.  Nothing here indexes an
// array with a number the compiler does not know.
#pragma once

#include "c2ray_face.hpp"
#include "c2ray_horizon.hpp"

namespace c2r {

// extent of the box along one axis (an empty box, hi < lo, has none)
C2R_HD int rim_extent(int lo, int hi) { return hi >= lo ? hi - lo + 1 : 0; }

C2R_HD double rim_pick(int axis, double v0, double v1, double v2) { return axis == 0 ? v0 : (axis == 1 ? v1 : v2); }

// entries of one sheet across `axis`, of all six sheets
C2R_HD int rim_sheet_cells(int e0, int e1, int e2, int axis) { return face_pick(axis, e1, e0, e0) * face_pick(axis, e2, e2, e1); }
C2R_HD long long rim_total(int e0, int e1, int e2) {
  return 2LL * ((long long)e1 * e2 + (long long)e0 * e2 + (long long)e0 * e1);
}

// entry t in [0, T) of a source's sheets -> (fc, oa, ob); false: t is beyond the last sheet
C2R_HD bool rim_decode(const int (&lo)[3], const int (&hi)[3], long long t, int &fc, int &oa, int &ob) {
  const int e0 = rim_extent(lo[0], hi[0]), e1 = rim_extent(lo[1], hi[1]), e2 = rim_extent(lo[2], hi[2]);
  const long long c0 = (long long)e1 * e2, c1 = (long long)e0 * e2, c2 = (long long)e0 * e1;
  if (t < 0 || t >= 2 * (c0 + c1 + c2)) return false;
  int axis;
  long long u = t;
  if (u < 2 * c0) axis = 0;
  else if (u < 2 * (c0 + c1)) { axis = 1; u -= 2 * c0; }
  else { axis = 2; u -= 2 * (c0 + c1); }
  const long long cells = axis == 0 ? c0 : (axis == 1 ? c1 : c2);
  const int high = u >= cells ? 1 : 0;
  if (high) u -= cells;
  const int ea = face_pick(axis, e1, e0, e0);
  const int rb = (int)(u / ea), ra = (int)(u - (long long)rb * ea);
  fc = 2 * axis + high;
  oa = ra + face_pick(axis, lo[1], lo[0], lo[0]);
  ob = rb + face_pick(axis, lo[2], lo[2], lo[1]);
  return true;
}

// ... and back: where the column (fc, oa, ob) sits among the T entries
C2R_HD long long rim_index(const int (&lo)[3], const int (&hi)[3], int fc, int oa, int ob) {
  const int e0 = rim_extent(lo[0], hi[0]), e1 = rim_extent(lo[1], hi[1]), e2 = rim_extent(lo[2], hi[2]);
  const long long c0 = (long long)e1 * e2, c1 = (long long)e0 * e2, c2 = (long long)e0 * e1;
  const int axis = fc >> 1;
  const long long base = axis == 0 ? 0 : (axis == 1 ? 2 * c0 : 2 * (c0 + c1));
  const long long cells = axis == 0 ? c0 : (axis == 1 ? c1 : c2);
  const int ea = face_pick(axis, e1, e0, e0);
  return base + ((fc & 1) ? cells : 0) + (oa - face_pick(axis, lo[1], lo[0], lo[0])) +
         (long long)ea * (ob - face_pick(axis, lo[2], lo[2], lo[1]));
}

// the offset of the cell k steps along the column (fc, oa, ob)
C2R_HD void rim_cell(int fc, int oa, int ob, int k, int &o0, int &o1, int &o2) {
  const int axis = fc >> 1, od = (fc & 1) ? k : -k;
  o0 = axis == 0 ? od : oa;
  o1 = axis == 1 ? od : (axis == 0 ? oa : ob);
  o2 = axis == 2 ? od : ob;
}

C2R_HD bool rim_within(double R2, double dr1, double dr2, double dr3, int fc, int oa, int ob, int k) {
  int o0, o1, o2;
  rim_cell(fc, oa, ob, k, o0, o1, o2);
  return horizon_within(R2, dr1, dr2, dr3, o0, o1, o2);
}

// k* of the column, -1 if its k = 0 cell is not within.  A square-root guess, then the exact predicate decides: the
// within-cells are a prefix, so stepping up while the next cell is within and down while this one is not ends at the largest
// k within the horizon and inside the box, whatever the guess was.
C2R_HD int rim_kstar(double R2, double dr1, double dr2, double dr3, const int (&lo)[3], const int (&hi)[3], int fc, int oa,
                     int ob) {
  if (!rim_within(R2, dr1, dr2, dr3, fc, oa, ob, 0)) return -1;
  const int axis = fc >> 1;
  const int kmax = (fc & 1) ? face_pick(axis, hi[0], hi[1], hi[2]) : -face_pick(axis, lo[0], lo[1], lo[2]);
  const double dra = rim_pick(axis, dr2, dr1, dr1), drb = rim_pick(axis, dr3, dr3, dr2), drd = rim_pick(axis, dr1, dr2, dr3);
  const double xa = dra * (double)oa, xb = drb * (double)ob;
  const double rem = R2 - (xa * xa + xb * xb);
  const double guess = rem > 0.0 ? sqrt(rem) / drd : 0.0;
  int k = guess >= (double)kmax ? kmax : (int)guess; // (an infinite R2, or dr_d = 0: the box decides)
  if (k < 0) k = 0;
  while (k < kmax && rim_within(R2, dr1, dr2, dr3, fc, oa, ob, k + 1)) k++;
  while (k > 0 && !rim_within(R2, dr1, dr2, dr3, fc, oa, ob, k)) k--;
  return k;
}

// the weight of the face at k + 1/2 along the column
C2R_HD double rim_weight(double dr1, double dr2, double dr3, int fc, int oa, int ob, int k) {
  if (oa == 0 && ob == 0 && k == 0) return 1.0 / 6.0;
  const int axis = fc >> 1;
  const double dra = rim_pick(axis, dr2, dr1, dr1), drb = rim_pick(axis, dr3, dr3, dr2), drd = rim_pick(axis, dr1, dr2, dr3);
  const double xa = dra * (double)oa, xb = drb * (double)ob, fd = drd * ((double)k + 0.5);
  const double f2 = (xa * xa + xb * xb) + fd * fd;
  return ((dra * drb) * fd) / ((4.0 * pi) * (f2 * sqrt(f2)));
}

// The whole rule for one sheet column of a source whose cut word has CUT_HORIZON: true iff the column has a face; then k is
// k*, (o0, o1, o2) the offset of the column's cell and w the weight.  Without a face k is k* (or -1) and w is 0.0.
C2R_HD bool rim_column(int cut, double a_x, double a_y, double a_z, double K, double R2, double dr1, double dr2, double dr3,
                       const int (&lo)[3], const int (&hi)[3], int fc, int oa, int ob, int &k, int &o0, int &o1, int &o2,
                       double &w) {
  w = 0.0;
  o0 = o1 = o2 = 0;
  k = rim_kstar(R2, dr1, dr2, dr3, lo, hi, fc, oa, ob);
  if (k < 0) return false;
  rim_cell(fc, oa, ob, k, o0, o1, o2);
  const bool interior = lo[0] < o0 && o0 < hi[0] && lo[1] < o1 && o1 < hi[1] && lo[2] < o2 && o2 < hi[2];
  if (!interior) return false;
  if (rim_within(R2, dr1, dr2, dr3, fc, oa, ob, k + 1)) return false;
  if (!cut_lit(cut, a_x, a_y, a_z, K, R2, dr1, dr2, dr3, o0, o1, o2)) return false;
  w = rim_weight(dr1, dr2, dr3, fc, oa, ob, k);
  return true;
}

} // namespace c2r
