// Source light curves (c2r_set_source_curves, include/c2ray_hip.h): a flux factor per shell of
// distance, per point source.  A cell at distance r sees a source at the retarded time t - r/c; a host that knows the
// source's history hands it over as a piecewise-constant curve, radius = c*(t - t_k) and factor = L(t_k)/L(t).  A horizon
// (c2ray_horizon.hpp) is the crudest such curve: factor 1 within the sphere, 0 beyond it.  Where a beam and a horizon switch
// a source's contribution to a cell on or off, a curve also scales it: one factor per cell.source, found by compares and
// selects, no square root, no division.
//
// A curve is nstep radii (0 .. CURVE_MAX_STEPS of them, physical lengths in the unit of dr, strictly ascending: a pass uses
// the dr of that pass) and nstep + 1 factors, finite and >= 0; factor[b] holds in shell b, and the shells are [0, r0],
// (r0, r1], ..., (r_{nstep-1}, infinity).  When the curves are set the host forms (curve_fill)
//     R2[k] = radius[k]*radius[k]   for k < nstep,   +infinity for the steps the curve does not have
// For a cell at offset (di, dj, dk) from the source -- the offset exactly as the kernel in question already forms it, as for
// a beam -- and the dr of the pass, every product and sum rounded as written and evaluated from the left, the horizon's own
// xs, ys, zs, d2:
//     xs = dr1*(double)di    ys = dr2*(double)dj    zs = dr3*(double)dk
//     d2 = (xs*xs + ys*ys) + zs*zs
//     b  = the number of k < nstep with d2 > R2[k]
//     f  = factor[b]
// A cell exactly on a radius belongs to the inner shell; the source's own cell is always shell 0 (0 > R2 never holds).  The
// radii ascend, so R2 does not descend and the k with d2 > R2[k] are a prefix: f is the factor behind the last of them, which
// is what curve_factor's chain of selects leaves.  A step the curve does not have (R2 = +infinity) is never beyond.
//
// A cell with f == 0.0 is UNLIT for that source, in exactly the sense c2ray_beam.hpp defines: it adds nothing to phih, phihe
// or phiheat, its loss term photo_out*vol/vol_ph is 0.0 in the loss that decides whether the box grows, in the loss that is
// kept, in photon_loss(1), in the escape maps and in the horizon rim (a cell with f = 0 has no face), and it leaves the
// source loop before any column is loaded.  Any other cell runs the per-cell routine the source always ran, with the same
// columns and vol_ph, and NormFlux*f in the place of NormFlux (in a three-SED run NormFluxPL*f and NormFluxQPL*f as well):
// one rounded product per SED, nothing else.  f == 1.0 therefore gives the uncurved bits.  With a beam or a horizon the
// cell is lit iff it is lit for every feature set; d2 is formed once (cut_flux).
//
// What a curve does not do.  The columns are swept as before.  The threshold 1e-10 * total_source_flux of the sub-box loop
// uses the unscaled fluxes; sum_nbox, reaches, column blocks and tile lists are untouched; planes are untouched.  Nothing is
// rescaled to conserve anything.
//
// Identities.
//   Curves off.  With no curves set, or every source nstep = 0 and factor[0] = 1.0, every grid, loss, map and sum_nbox has
//     the bits, and the pass the launches, it has without this file.
//   All factors 1.0.  The same bits, through the curved kernel.
//   Step to zero.  {1, {R}, {1, 0}} is the horizon R, bit for bit, sub-box loop included.
//   Powers of two.  A factor 2^n scales phih, phihe, phiheat and the loss terms exactly.
//   Several sources.  grid = grid + term_s(NormFlux_s*f), folded in source order, as for beams.
//
// Like c2ray_horizon.hpp this file compiles with a host C++ compiler: tests/curve_harness.cpp runs these functions on the
// CPU over every offset of a cube, and the kernels of c2ray_hip.hip run the same ones per lane.  Nothing here indexes an
// array with a number the compiler does not know: the tables are read at constant places of the source's record.
#pragma once

#include <cmath>

#include "c2ray_horizon.hpp"

namespace c2r {

// the third flag of a source's cut word (c2ray_horizon.hpp): the source has a curve
constexpr int CUT_CURVE = 8;
constexpr int CURVE_MAX_STEPS = 8; // C2R_CURVE_MAX_STEPS of the public header

// the host's half of the rule
C2R_HD double curve_R2(double radius) { return radius * radius; }

// the tables of a source's record from a curve as it was set: R2 of its steps, +infinity behind them; its factors, 0.0 behind
C2R_HD void curve_fill(int nstep, const double *radius, const double *factor, double (&R2)[CURVE_MAX_STEPS],
                       double (&fac)[CURVE_MAX_STEPS + 1]) {
  for (int k = 0; k < CURVE_MAX_STEPS; k++) R2[k] = k < nstep ? curve_R2(radius[k]) : (double)INFINITY;
  for (int k = 0; k <= CURVE_MAX_STEPS; k++) fac[k] = k <= nstep ? factor[k] : 0.0;
}

// the factor of the shell that holds d2: eight compares and selects on values (unrolled: every table entry is read at a
// constant place, from scalar registers on the device)
C2R_HD double curve_factor(double d2, const double (&R2)[CURVE_MAX_STEPS], const double (&fac)[CURVE_MAX_STEPS + 1]) {
  double f = fac[0];
#pragma unroll
  for (int k = 0; k < CURVE_MAX_STEPS; k++) f = d2 > R2[k] ? fac[k + 1] : f;
  return f;
}

// the factor of the curve alone
C2R_HD double curve_factor_at(const double (&R2)[CURVE_MAX_STEPS], const double (&fac)[CURVE_MAX_STEPS + 1], double dr1, double dr2,
                              double dr3, int di, int dj, int dk) {
  const double xs = dr1 * (double)di, ys = dr2 * (double)dj, zs = dr3 * (double)dk;
  const double d2 = (xs * xs + ys * ys) + zs * zs;
  return curve_factor(d2, R2, fac);
}

// Everything a source whose cut word is not CUT_NONE asks about a cell: cut_lit's two predicates and, where it has a curve,
// the factor f of the cell's shell (1.0 without a curve), with xs, ys, zs and d2 formed once.  true: the cell is lit, and
// f != 0.0 scales the source's fluxes; false: the cell is unlit for this source.
C2R_HD bool cut_flux(int cut, double a_x, double a_y, double a_z, double K, double R2, const double (&cR2)[CURVE_MAX_STEPS],
                     const double (&cfac)[CURVE_MAX_STEPS + 1], double dr1, double dr2, double dr3, int di, int dj, int dk,
                     double &f) {
  const double xs = dr1 * (double)di, ys = dr2 * (double)dj, zs = dr3 * (double)dk;
  const double d2 = (xs * xs + ys * ys) + zs * zs;
  bool lit = true;
  const int kind = cut & CUT_BEAM_MASK;
  if (kind != BEAM_NONE) {
    const double dot = (xs * a_x + ys * a_y) + zs * a_z;
    lit = (kind == BEAM_BICONE || dot >= 0.0) && dot * dot >= K * d2;
  }
  if (cut & CUT_HORIZON) lit = lit && d2 <= R2;
  f = 1.0;
  if (cut & CUT_CURVE) {
    f = curve_factor(d2, cR2, cfac);
    lit = lit && f != 0.0;
  }
  return lit;
}

} // namespace c2r
