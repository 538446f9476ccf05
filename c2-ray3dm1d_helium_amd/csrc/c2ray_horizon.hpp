// Photon horizons (c2r_set_source_horizons, include/c2ray_hip.h): a maximum ray length per point
// source -- a mean free path set by unresolved absorbers, or the causal front c*(t - t_on) of a source that has just
// switched on.  Like a beam (c2ray_beam.hpp) a horizon switches a source's contribution to a cell on or off and never
// alters it: one predicate per cell.source, no square root, no division.
//
// A horizon is one double per source, radius, in the length unit of dr: a PHYSICAL length, so a pass uses the dr of that
// pass (a host that wants a comoving horizon rescales it as it rescales dr).  radius = +infinity: the source has none.
// When the horizons are set the host forms one double per source (horizon_R2):
//     R2 = radius*radius
// For a cell at offset (di, dj, dk) from the source -- the offset exactly as the kernel in question already forms it: the
// image within the reach on a periodic axis, the plain difference on an open one -- and the dr of the pass, every product
// and sum rounded as written and evaluated from the left, the beam's own xs, ys, zs, d2 (horizon_within):
//     xs = dr1*(double)di    ys = dr2*(double)dj    zs = dr3*(double)dk
//     d2 = (xs*xs + ys*ys) + zs*zs
//     within  iff  d2 <= R2
// A cell exactly on the sphere is within; the source's own cell always is (0 <= R2); radius = 0 lights the own cell only; a
// radius so large that R2 overflows to +infinity lights everything.
//
// A cell that is NOT within is UNLIT for that source, in exactly the sense c2ray_beam.hpp defines: it adds nothing to phih,
// phihe or phiheat, and its loss term photo_out*vol/vol_ph is 0.0 in the loss that decides whether the box grows, in the loss
// that is kept, in photon_loss(1) and in the escape maps.  A LIT cell gets the bits it gets without a horizon.  A source with
// a beam and a horizon lights a cell iff both predicates hold; d2 is formed once (cut_lit).
//
// What a horizon does not do.  The columns are swept as before, over the whole box: a cell within the sphere only ever
// interpolates from cells nearer the source, which are within it too, so the sweep need not know.  The threshold 1e-10 *
// total_source_flux of the sub-box loop and the way sum_nbox counts rounds are what they were: the loop ends at the first
// sub-box that contains the sphere because the deciding loss becomes 0.0.  Reaches, column blocks and tile lists are
// untouched (an unlit lane leaves the source loop before any column load).  Planes are untouched.
// THERE IS NO HORIZON LOSS unless c2r_enable_horizon_loss.  Photons cut off at the sphere appear in no loss and no map, and
// with a horizon set photon_loss alone does not close the photon budget.  The horizon loss does (c2ray_rim.hpp): the cells
// within the horizon are a closed staircase whose boundary is made of cell faces, and a weight per exposed face at the face
// centre -- w = ((dr_a*dr_b)*fd) / ((4.0*pi)*(f2*sqrt(f2))), f2 = (xa*xa + xb*xb) + fd*fd, fd = dr_d*((double)k* + 0.5), 1/6
// for the faces of the source's own cell -- tiles the sphere; a source's loss is the fixed-order sum of po * w over its faces.
//
// Identities.
//   Horizons off.  With no horizons set, or every radius +infinity, every grid, loss, map and sum_nbox has the bits, and the
//     pass the launches, it has without this file.
//   Infinite R2.  A finite radius whose square overflows lights every cell: the same bits, through the beamed kernels.
//   Several sources.  grid = grid + where(lit_s, term_s, 0.0), folded in source order, as for beams.
//
// Like c2ray_beam.hpp this file compiles with a host C++ compiler: tests/horizon_harness.cpp runs these functions on the CPU
// over every offset of a cube, and the kernels of c2ray_hip.hip run the same ones per lane.
#pragma once

#include "c2ray_beam.hpp"

namespace c2r {

// What cuts a source's light short, in one word of its device record: the beam's kind in the low two bits (BEAM_NONE,
// BEAM_CONE, BEAM_BICONE) and CUT_HORIZON where the source has a finite horizon.  0: nothing does.
constexpr int CUT_NONE = 0, CUT_BEAM_MASK = 3, CUT_HORIZON = 4;

// the host's half of the rule
C2R_HD double horizon_R2(double radius) { return radius * radius; }

// the predicate of the horizon alone
C2R_HD bool horizon_within(double R2, double dr1, double dr2, double dr3, int di, int dj, int dk) {
  const double xs = dr1 * (double)di, ys = dr2 * (double)dj, zs = dr3 * (double)dk;
  const double d2 = (xs * xs + ys * ys) + zs * zs;
  return d2 <= R2;
}

// both predicates of a source whose cut word is not CUT_NONE (a source with neither never asks): beam_lit where it has a
// beam, horizon_within where it has a horizon, with xs, ys, zs and d2 formed once
C2R_HD bool cut_lit(int cut, double a_x, double a_y, double a_z, double K, double R2, double dr1, double dr2, double dr3, int di,
                    int dj, int dk) {
  const double xs = dr1 * (double)di, ys = dr2 * (double)dj, zs = dr3 * (double)dk;
  const double d2 = (xs * xs + ys * ys) + zs * zs;
  bool lit = true;
  const int kind = cut & CUT_BEAM_MASK;
  if (kind != BEAM_NONE) {
    const double dot = (xs * a_x + ys * a_y) + zs * a_z;
    lit = (kind == BEAM_BICONE || dot >= 0.0) && dot * dot >= K * d2;
  }
  if (cut & CUT_HORIZON) lit = lit && d2 <= R2;
  return lit;
}

} // namespace c2r
