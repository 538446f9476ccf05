// Side faces of a tilted plane (include/c2ray_hip.h: c2r_set_plane_side_entry, c2r_enable_plane_side_exit,
// c2r_enable_plane_side_loss): which side is live in a pass, where its edges are, and which share of a
// cell's outgoing beam leaves through which open side face.
//
// Side 0 is the face axis f, side 1 the face axis g (f < g).  A side is live iff its tilt component is non-zero and its axis
// is open.  The beam moves towards +e along a face axis: the upstream ghost index of a live side is -1 for e = +1 and n for
// e = -1 (where plane_upstream returns -1), its downstream edge is the cell index n - 1 for e = +1 and 0 for e = -1, and the
// mesh face it leaves through is 2 * axis + (e > 0).
//
// Like c2ray_face.hpp this file compiles with a host C++ compiler, and nothing here indexes an array with a number the
// compiler does not know.
#pragma once

#include "c2ray_face.hpp"
#include "c2ray_plane.hpp"

namespace c2r {

C2R_HD bool pside_live(double tilt_component, int wrap) { return tilt_component != 0.0 && !wrap; }
C2R_HD int pside_edge(int e, int n) { return e > 0 ? n - 1 : 0; }
C2R_HD int pside_face(int axis, int e) { return 2 * axis + (e > 0 ? 1 : 0); }

// The side a displaced target (tu, tv) in the next layer gives its weight to: an index wraps on a periodic face axis; a
// target that then lies outside the mesh along f belongs to side 0 (also when it lies outside along g as well: the lowest
// axis, the escape maps' tie rule), outside along g only to side 1; -1: it is a cell of the mesh.
C2R_HD int pside_of_target(const PlaneTilt &T, int fa, int fb, int tu, int tv) {
  const bool out_f = !T.wrap_f && (tu < 0 || tu >= fa), out_g = !T.wrap_g && (tv < 0 || tv >= fb);
  return out_f ? 0 : (out_g ? 1 : -1);
}

// The weights w_0, w_1 of cell (u, v): the targets (u + e_f, v + e_g), (u, v + e_g), (u + e_f, v) carry s1, s2, s3.
// w_0 = s3 + s1 (a target outside along f takes the diagonal with it), w_1 = s2 + s1, or s2 alone on the line where side 0
// takes the diagonal; 0.0 for a cell that is on no downstream edge.  One rounded sum each.
C2R_HD void pside_weights(const PlaneTilt &T, int fa, int fb, int u, int v, double &w0, double &w1) {
  const int diag = pside_of_target(T, fa, fb, u + T.e_f, v + T.e_g);
  w0 = pside_of_target(T, fa, fb, u + T.e_f, v) == 0 ? T.s[2] + T.s[0] : 0.0;
  w1 = pside_of_target(T, fa, fb, u, v + T.e_g) == 1 ? (diag == 1 ? T.s[1] + T.s[0] : T.s[1]) : 0.0;
}

// the term of a cell for a side: one rounded product of its far-face term (plane_exit_term) with the side's weight
C2R_HD double pside_term(double base, double w) { return base * w; }

} // namespace c2r
