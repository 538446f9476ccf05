// Beamed point sources (c2r_set_source_beams, include/c2ray_hip.h): an emission cone or bicone per
// point source.  A beam switches a source's contribution to a cell on or off and never alters it: one predicate per
// cell.source, no square root, no division.
//
// A beam belongs to one point source: kind (0 none, 1 cone, 2 bicone), axis[3] in the physical directions x, y, z (it need
// not be normalised) and cos_half, the cosine of the half opening angle, 0 <= cos_half <= 1.  When the beams are set the
// host forms one double per source (beam_K):
//     K = (cos_half*cos_half) * ((a_x*a_x + a_y*a_y) + a_z*a_z)
// For a cell at offset (di, dj, dk) from the source -- the offset exactly as the kernel in question already forms it: the
// image within the reach on a periodic axis, the plain difference on an open one -- and the dr of the pass, every product
// and sum rounded as written and evaluated from the left (beam_lit):
//     xs = dr1*(double)di    ys = dr2*(double)dj    zs = dr3*(double)dk
//     dot = (xs*a_x + ys*a_y) + zs*a_z
//     d2  = (xs*xs + ys*ys) + zs*zs
//     cone:    lit  iff  dot >= 0.0  &&  dot*dot >= K*d2
//     bicone:  lit  iff  dot*dot >= K*d2
// A cell exactly on the cone is lit; the source's own cell is lit without a special case (0 >= 0).
//
// An UNLIT cell behaves, for that source only, exactly like a cell with N_in(HI) >= max_coldensh: it adds nothing to phih,
// phihe or phiheat, and its loss term photo_out*vol/vol_ph is 0.0 in the loss that decides whether the box grows, in the loss
// that is kept, in photon_loss(1) and in the escape maps.  A LIT cell gets the bits it gets without a beam.
//
// What a beam does not do.  NormFlux stays the isotropic-equivalent flux: nothing is rescaled to conserve photons.  The
// threshold 1e-10 * total_source_flux of the sub-box loop is what it was.  The columns are swept as before, over the whole
// box, lit or not (an unlit cell still shadows nothing: columns do not depend on the beam), and the tile lists of the rates
// launch hold unlit cells too.  sum_nbox counts rounds as before.  Planes are untouched.
//
// Identities.
//   Beams off.  With no beams set, or every kind == 0, every grid, loss, map and sum_nbox has the bits, and the pass the
//     launches, it has without this file.
//   Full bicone.  A bicone with cos_half = 0 (K = 0) lights every cell: the same bits, through the beamed kernels.
//   One beamed source, from zeroed grids.  Every rate grid equals the unbeamed source's grid where the cell is lit and
//     +0.0 elsewhere, provided both runs trace the same rounds (a beam may end the sub-box loop earlier: less is lost).
//   Several sources.  grid = grid + where(lit_s, term_s, 0.0), folded in source order.
//
// Like c2ray_face.hpp this file compiles with a host C++ compiler: tests/beam_harness.cpp runs these functions on the CPU
// over every offset of a cube, and the kernels of c2ray_hip.hip run the same ones per lane.
#pragma once

#include "c2ray_device.hpp"

namespace c2r {

constexpr int BEAM_NONE = 0, BEAM_CONE = 1, BEAM_BICONE = 2;

// the host's half of the rule: cos^2 of the half opening angle times the squared length of the axis
C2R_HD double beam_K(double cos_half, double a_x, double a_y, double a_z) {
  return (cos_half * cos_half) * ((a_x * a_x + a_y * a_y) + a_z * a_z);
}

// the predicate; kind must be BEAM_CONE or BEAM_BICONE (a source without a beam never asks)
C2R_HD bool beam_lit(int kind, double a_x, double a_y, double a_z, double K, double dr1, double dr2, double dr3, int di, int dj,
                     int dk) {
  const double xs = dr1 * (double)di, ys = dr2 * (double)dj, zs = dr3 * (double)dk;
  const double dot = (xs * a_x + ys * a_y) + zs * a_z;
  const double d2 = (xs * xs + ys * ys) + zs * zs;
  return (kind == BEAM_BICONE || dot >= 0.0) && dot * dot >= K * d2;
}

} // namespace c2r
