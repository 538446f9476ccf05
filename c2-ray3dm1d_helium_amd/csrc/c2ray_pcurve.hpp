// Plane light curves (c2r_set_plane_curve, include/c2ray_hip.h): a flux factor per shell of depth
// along a plane's beam.  A layer at depth d behind the place the beam set out from sees the plane at the retarded time
// t - d/c; a host that knows the plane's history hands it over as a piecewise-constant curve, depth = c*(t - t_k) and factor
// = F(t_k)/F(t), exactly as c2ray_curve.hpp does for the distance shells of a point source.  A depth horizon is the crudest
// such curve, {1, {D}, {1, 0}}.
//
// A curve is nstep depths (0 .. PCURVE_MAX_STEPS of them, lengths along the beam in the unit of dr, strictly ascending),
// nstep + 1 factors, finite and >= 0, and where the mesh begins on the beam: layer0 layers of this plane's path, and the
// length depth0 before those.  When the curve is set the host forms (pcurve_fill) the table depth[k] for k < nstep, +infinity
// for the steps the curve does not have.  For layer m = 0 .. mesh[axis]-1 in travel order and the per-layer path of the pass
// (dr[axis], or PlaneTilt::path of a tilted plane), every operation rounded as written, no fused multiply-add:
//     d = depth0 + ((double)(layer0 + m) + 0.5) * path
//     b = the number of k < nstep with d > depth[k]
//     f = factor[b]
// The shells are [0, depth[0]], (depth[0], depth[1]], ..., (depth[nstep-1], infinity): a layer whose centre lies exactly on a depth
// belongs to the nearer shell.  No square root, no division; f is uniform over a layer and is what curve_factor's chain of
// selects leaves.  A step the curve does not have (+infinity) is never beyond.
//
// A cell of a layer with f == 0.0 is UNLIT: it adds nothing to phih, phihe or phiheat, no per-cell routine runs for it, and
// if it lies in the last layer its line's loss term is 0.0 -- in photon_loss(1), in c2r_get_plane_loss and in the far face's
// escape map.  Any other cell is the plane's cell with nf[k]*f in the place of nf[k] (pcurve_flux), one rounded product per
// SED, nf being whatever the cell uses without a curve: the plane's normflux, the map entry of its line, or what the layers
// of a tilted mapped plane left at the cell.  A cell is skipped iff its unscaled fluxes are dark (plane_dark) or f == 0.0;
// whether the plane takes the three-SED routine is decided from the unscaled fluxes.
//
// What a curve does not touch: the march, the fog, the columns, the exit columns and the max_coldensh guard; vol_ph = path;
// the carried flux of a tilted mapped plane and the exit flux (both unscaled: the slab downstream applies its own curve with
// its own layer0 / depth0); sum_nbox and the deal of planes.  Nothing is rescaled to conserve anything.
//
// Like c2ray_curve.hpp this file compiles with a host C++ compiler: tests/plane_curve_harness.cpp marches whole meshes with
// these functions on the CPU, and the kernels of c2ray_planes.inc run the same ones per lane.  Nothing here indexes an array
// with a number the compiler does not know: the tables are read at constant places of the plane's record.
#pragma once

#include "c2ray_curve.hpp"
#include "c2ray_plane.hpp"

namespace c2r {

constexpr int PCURVE_MAX_STEPS = CURVE_MAX_STEPS; // C2R_PLANE_CURVE_MAX_STEPS of the public header: curve_factor's table

// a plane's curve as the kernels read it: a kernel argument, uniform over the launch
struct PlaneCurveDev {
  double depth[PCURVE_MAX_STEPS];   // the steps, +infinity behind them
  double fac[PCURVE_MAX_STEPS + 1]; // the factors, 0.0 behind them
  double depth0;
  int layer0;
};

// the tables of a plane's record from a curve as it was set (curve_fill without the square)
C2R_HD void pcurve_fill(int nstep, const double *depth, const double *factor, int layer0, double depth0, PlaneCurveDev &cv) {
  for (int k = 0; k < PCURVE_MAX_STEPS; k++) cv.depth[k] = k < nstep ? depth[k] : (double)INFINITY;
  for (int k = 0; k <= PCURVE_MAX_STEPS; k++) cv.fac[k] = k <= nstep ? factor[k] : 0.0;
  cv.depth0 = depth0;
  cv.layer0 = layer0;
}

// the depth of the centre of layer m (travel order) along the beam
C2R_HD double pcurve_depth(double depth0, int layer0, int m, double path) { return depth0 + ((double)(layer0 + m) + 0.5) * path; }

// the factor of layer m
C2R_HD double pcurve_factor(const PlaneCurveDev &cv, int m, double path) {
  return curve_factor(pcurve_depth(cv.depth0, cv.layer0, m, path), cv.depth, cv.fac);
}

// How a mesh cell (i, j, k) finds its layer in travel order: along = i * li + j * lj + k * lk (one coefficient is 1), counted
// from the far end for a plane that enters at the high side.
struct PlaneLayerIndex {
  int li, lj, lk;
  int na, from_high;
};
C2R_HD PlaneLayerIndex plane_layer_index(int axis, int from_high, int na) {
  return PlaneLayerIndex{axis == 0 ? 1 : 0, axis == 1 ? 1 : 0, axis == 2 ? 1 : 0, na, from_high};
}
C2R_HD int pcurve_layer(const PlaneLayerIndex &lx, int i, int j, int k) {
  const int along = i * lx.li + j * lx.lj + k * lx.lk;
  return lx.from_high ? lx.na - 1 - along : along;
}

// the flux of SED k of a curved plane's cell: one rounded product
C2R_HD double pcurve_flux(double nf, double f) { return nf * f; }
C2R_HD void pcurve_fluxes(const double (&nf)[NSED], double f, double (&out)[NSED]) {
  out[0] = pcurve_flux(nf[0], f);
  out[1] = pcurve_flux(nf[1], f);
  out[2] = pcurve_flux(nf[2], f);
}

// The three fluxes of a curved plane's cell formed where they are used -- the same rounded product every time -- for the
// three-SED heating kernel, which has no registers to keep three more values per lane through its band loops (the LaneFlux
// device of c2ray_rates_body.inc).  nf0..nf2: the unscaled fluxes (named members: nothing is indexed).
struct PlaneCurveFlux {
  double nf0, nf1, nf2, f;
  C2R_HD double operator[](int k) const { return pcurve_flux(k == 0 ? nf0 : (k == 1 ? nf1 : nf2), f); }
};

// plane_cell_rates (c2ray_plane.hpp, step 6) with the fluxes of a PlaneCurveFlux: the same statements, nf[k] read through it
template <bool HEAT, bool MULTI, class LT, class BD>
C2R_HD bool plane_cell_rates(const BD &bd, const SedSet &ss, double cin_HI, double cout_HI, double cin_HeI, double cout_HeI,
                             double cin_HeII, double cout_HeII, double vol_ph, const PlaneCurveFlux &nf, double h_av1, double u_HI,
                             double u_HeI, double u_HeII, double (&add)[4], const LT *logtab, const gm::LogPins *pins = nullptr) {
  if (!(cin_HI < max_coldensh)) return false;
  Ricotti ric = {};
  if (HEAT) ric = ricotti_parameters(dmax(h_av1, epsilon));
  PhotoOut o;
  if (MULTI)
    photoion_rates_multi<HEAT>(bd, ss, cin_HI, cout_HI, cin_HeI, cout_HeI, cin_HeII, cout_HeII, vol_ph, nf, ric, o, logtab, pins);
  else
    photoion_rates<HEAT>(bd, ss.photo_thick[0], ss.photo_thin[0], ss.heat_thick[0], ss.heat_thin[0], cin_HI, cout_HI, cin_HeI,
                         cout_HeI, cin_HeII, cout_HeII, vol_ph, nf[0], ric, o, logtab, pins);
  add[0] = o.photo_HI / (u_HI * (1.0 - abu_he));
  add[1] = o.photo_HeI / (u_HeI * abu_he);
  add[2] = o.photo_HeII / (u_HeII * abu_he);
  add[3] = HEAT ? o.heat : 0.0;
  return true;
}

} // namespace c2r
