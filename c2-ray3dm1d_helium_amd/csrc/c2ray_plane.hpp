// Plane-parallel sources: the per-cell rule of a plane wave that enters through an open mesh face and travels along
// one axis (include/c2ray_hip.h c2r_set_plane_sources).
//
// Every line of cells along the axis is a 1-D problem of its own: no cinterp (the incoming column of a cell is the
// outgoing column of the cell before it), no 1/r^2 dilution (NormFlux per cm^2 of face enters a column of cross-section
// A and is absorbed in the volume A * dr[axis]: vol_ph = dr[axis]).  Everything per cell is what a point source gets:
// coldens, the LLS fog, the max_coldensh guard, photoion_rates / photoion_rates_multi, the secondary-ionisation
// parameters, the denominators of evolve_point.F90:288-296 -- the functions of c2ray_device.hpp, unchanged.
//
// Like c2ray_device.hpp this file compiles with a host C++ compiler (tests/plane_harness.cpp marches whole meshes with
// these functions on the CPU against a NumPy reference built from the oracle's per-cell routines).
#pragma once

#include "c2ray_device.hpp"

namespace c2r {

constexpr int PLANE_MAX = 6; // most planes of a context: one per face of the mesh

// Step 1: neufrac * ndens of the three species with the fractions clamped at epsilon (evolve_point.F90:132-136), the
// first product of coldens (doric.f90:358-372) -- what sweep_cell_state reads or forms for a point source.
C2R_HD void plane_cell_state(double nd, double xh_av0, double xhe_av0, double xhe_av1, double &u_HI, double &u_HeI, double &u_HeII) {
  u_HI = dmax(xh_av0, epsilon) * nd;
  u_HeI = dmax(xhe_av0, epsilon) * nd;
  u_HeII = dmax(xhe_av1, epsilon) * nd;
}

// Step 4: the Lyman-limit-system fog on the incoming HI column (evolve_point.F90:177-180), every cell of the march
C2R_HD double plane_fog(double cin_HI, double coldensh_LLS, double path, double dr1) { return cin_HI + coldensh_LLS * path / dr1; }

// Step 5: the outgoing columns, coldens evaluated from the left (neufrac * ndens * path * abundance)
C2R_HD void plane_cell_out(double cin_HI, double cin_HeI, double cin_HeII, double u_HI, double u_HeI, double u_HeII, double path,
                           double &cout_HI, double &cout_HeI, double &cout_HeII) {
  cout_HI = cin_HI + u_HI * path * (1.0 - abu_he);
  cout_HeI = cin_HeI + u_HeI * path * abu_he;
  cout_HeII = cin_HeII + u_HeII * path * abu_he;
}

// Steps 1-5 for one cell of a march: `cin_*` come in as the outgoing columns of the cell before (or the entry columns)
// and leave with the fog applied, as every later step sees them.
C2R_HD void plane_cell_columns(double nd, double xh_av0, double xhe_av0, double xhe_av1, double path, double dr1, int use_lls,
                               double coldensh_LLS, double &cin_HI, double cin_HeI, double cin_HeII, double &cout_HI,
                               double &cout_HeI, double &cout_HeII) {
  double u_HI, u_HeI, u_HeII;
  plane_cell_state(nd, xh_av0, xhe_av0, xhe_av1, u_HI, u_HeI, u_HeII);
  if (use_lls) cin_HI = plane_fog(cin_HI, coldensh_LLS, path, dr1);
  plane_cell_out(cin_HI, cin_HeI, cin_HeII, u_HI, u_HeI, u_HeII, path, cout_HI, cout_HeI, cout_HeII);
}

// Step 6: what the plane adds to the four rate grids of one cell (add = phih, phihe0, phihe1, phiheat terms).  Returns
// false -- nothing is added -- where the incoming HI column has reached max_coldensh (evolve_point.F90:246).
// u_*: the cell's neufrac * ndens (plane_cell_state); the denominators of evolve_point.F90:288-296,
// neufrac * ndens * abundance from the left, are their products with the abundances.  h_av1: xh_av(q,1), the ionised
// fraction the secondary-ionisation parameters depend on (:255).  nf: NormFlux per cm^2 of face of the three SEDs;
// MULTI: the power-law or the quasar-like flux is non-zero (photoion_rates_multi).
template <bool HEAT, bool MULTI, class LT, class BD>
C2R_HD bool plane_cell_rates(const BD &bd, const SedSet &ss, double cin_HI, double cout_HI, double cin_HeI, double cout_HeI,
                             double cin_HeII, double cout_HeII, double vol_ph, const double (&nf)[NSED], double h_av1, double u_HI,
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

// Step 7: what one column of the plane loses through the far face, from the columns of its last cell
// (evolve_point.F90:310-315 with vol_ph = dr[axis]); 0 where that cell is beyond max_coldensh.
template <bool MULTI>
C2R_HD double plane_exit_term(const BandData &bd, const SedSet &ss, double cin_HI, double cout_HI, double cin_HeI, double cout_HeI,
                              double cin_HeII, double cout_HeII, const double (&nf)[NSED], double vol, double dr_axis) {
  if (!(cin_HI < max_coldensh)) return 0.0;
  const double po = MULTI ? photo_out_multi(bd, ss, cin_HI, cout_HI, cin_HeI, cout_HeI, cin_HeII, cout_HeII, nf)
                          : photo_out_only(bd, ss.photo_thick[0], ss.photo_thin[0], cin_HI, cout_HI, cin_HeI, cout_HeI, cin_HeII,
                                           cout_HeII, nf[0]);
  return po * vol / dr_axis;
}

// The cells of a march.  Column f of the face (mesh order of the two remaining axes, the lower axis fastest), step m in
// travel order: the 0-based mesh cell number.  from_high: the wave enters at index mesh[axis] and travels towards 1.
struct PlaneGeom {
  int n[3];      // mesh
  int axis, from_high;
  int na;        // cells along the axis
  int fa, fb;    // extents of the two remaining axes (lower first)
  size_t sa, sf, sg; // strides, in cells, of the axis and of the two face axes
};
C2R_HD PlaneGeom plane_geometry(int n1, int n2, int n3, int axis, int from_high) {
  PlaneGeom G;
  G.n[0] = n1; G.n[1] = n2; G.n[2] = n3;
  G.axis = axis; G.from_high = from_high;
  const size_t stride[3] = {1, (size_t)n1, (size_t)n1 * (size_t)n2};
  const int a = axis, f = axis == 0 ? 1 : 0, g = axis == 2 ? 1 : 2;
  G.na = G.n[a]; G.fa = G.n[f]; G.fb = G.n[g];
  G.sa = stride[a]; G.sf = stride[f]; G.sg = stride[g];
  return G;
}
C2R_HD size_t plane_cell(const PlaneGeom &G, int f, int m) {
  const int along = G.from_high ? G.na - 1 - m : m;
  return (size_t)(f % G.fa) * G.sf + (size_t)(f / G.fa) * G.sg + (size_t)along * G.sa;
}

// Oblique incidence (c2r_set_plane_tilt, include/c2ray_hip.h): the beam leans towards the two face axes f < g by the
// tangents tilt[0], tilt[1].  The incoming column of a cell is then cinterp's weighted mean over four cells of the layer
// before it (column_density.f90:116-163) with the weights s1..s4 of a source at infinity: the same for every cell, host
// doubles formed once per pass from the current dr.  Everything behind N_in is the normal plane's cell with this `path`.
struct PlaneTilt {
  double a_f, a_g; // cells moved sideways per layer, 0 <= a <= 1
  double s[4];     // weights of c1 (diagonal), c2 (displaced along g), c3 (displaced along f), c4 (straight behind)
  double path;     // dr[axis] / cos(theta)
  int e_f, e_g;    // the upstream neighbour lies at index - e
  int wrap_f, wrap_g; // the face axis is periodic: an index outside the mesh wraps (else that corner's columns are 0)

  PlaneTilt() = default;
  C2R_HD PlaneTilt(const double tilt[2], const double dr[3], int axis, const int periodic[3]) {
    const int f = axis == 0 ? 1 : 0, g = axis == 2 ? 1 : 2;
    a_f = (fabs(tilt[0]) * dr[axis]) / dr[f];
    a_g = (fabs(tilt[1]) * dr[axis]) / dr[g];
    s[0] = a_f * a_g;
    s[1] = (1.0 - a_f) * a_g;
    s[2] = a_f * (1.0 - a_g);
    s[3] = (1.0 - a_f) * (1.0 - a_g);
    path = dr[axis] * sqrt(1.0 + (tilt[0] * tilt[0] + tilt[1] * tilt[1]));
    e_f = tilt[0] > 0.0 ? 1 : -1;
    e_g = tilt[1] > 0.0 ? 1 : -1;
    wrap_f = periodic[f] != 0;
    wrap_g = periodic[g] != 0;
  }
  // the axis is still the dominant one (cinterp's own case split); false for a non-finite tilt too
  C2R_HD bool valid() const { return a_f <= 1.0 && a_g <= 1.0; }
};
C2R_HD bool plane_tilted(const double tilt[2]) { return tilt[0] != 0.0 || tilt[1] != 0.0; }

// The upstream index u - e along a face axis of n cells, e = +-1: wrapped on a periodic axis (a compare and an add),
// -1 where the ray came in through an open side of the mesh.
C2R_HD int plane_upstream(int u, int e, int n, int wrap) {
  int uu = u - e;
  if (uu < 0) uu = wrap ? uu + n : -1;
  else if (uu >= n) uu = wrap ? uu - n : -1;
  return uu;
}

// cinterp's weighted mean of one species (column_density.f90:145-163, weightf :351-376) with the plane's weights; no
// sqrt2 / sqrt3 factor (that belongs to cells adjacent to a source).  Never used when both tilts are zero: it would
// give c * w / w instead of c.
C2R_HD double plane_interp(const double (&s)[4], double c1, double c2, double c3, double c4, double sig) {
  const double w1 = s[0] * weightf(c1, sig), w2 = s[1] * weightf(c2, sig), w3 = s[2] * weightf(c3, sig), w4 = s[3] * weightf(c4, sig);
  return (c1 * w1 + c2 * w2 + c3 * w3 + c4 * w4) / (w1 + w2 + w3 + w4);
}

// N_in of the three species of face cell (u, v) from the outgoing columns of the layer before (`prev`: 3 x face, species
// slowest, u fastest; null: all zero -- a first layer without entry columns).
C2R_HD void plane_layer_in(const PlaneTilt &T, int fa, int fb, int u, int v, const double *prev, double &c_HI, double &c_HeI,
                           double &c_HeII) {
  const int uu = plane_upstream(u, T.e_f, fa, T.wrap_f), vv = plane_upstream(v, T.e_g, fb, T.wrap_g);
  const int face = fa * fb;
  // c1 .. c4: (u - e_f, v - e_g), (u, v - e_g), (u - e_f, v), (u, v)
  const int at[4] = {uu >= 0 && vv >= 0 ? uu + fa * vv : -1, vv >= 0 ? u + fa * vv : -1, uu >= 0 ? uu + fa * v : -1, u + fa * v};
  double c[3][4];
  for (int k = 0; k < 3; k++)
    for (int i = 0; i < 4; i++) c[k][i] = prev && at[i] >= 0 ? prev[k * face + at[i]] : 0.0;
  c_HI = plane_interp(T.s, c[0][0], c[0][1], c[0][2], c[0][3], sigma_HI_at_ion_freq);
  c_HeI = plane_interp(T.s, c[1][0], c[1][1], c[1][2], c[1][3], sigma_HeI_at_ion_freq);
  c_HeII = plane_interp(T.s, c[2][0], c[2][1], c[2][2], c[2][3], sigma_HeII_at_ion_freq);
}

// Flux maps (c2r_set_plane_flux_map, include/c2ray_hip.h): the NormFlux of a plane as a field over its face, 3 x face
// doubles, SED slowest, the face cells in the order of the entry columns.
//
// A dark cell -- all three fluxes == 0.0 -- adds nothing to any rate grid and its line's loss term is 0.0: it is skipped,
// no per-cell function is evaluated.
C2R_HD bool plane_dark(const double (&nf)[NSED]) { return nf[0] == 0.0 && nf[1] == 0.0 && nf[2] == 0.0; }

// The flux of face cell (u, v) of a tilted plane's layer from the fluxes of the layer before (`fprev`: 3 x face, or the
// map itself in front of the first layer): the corners c1 .. c4 of plane_layer_in with the geometric weights alone,
// F = F1 s1 + F2 s2 + F3 s3 + F4 s4, every product rounded, the sums from the left.  No optical-depth factor: with it
// the face total of a periodic face would not be conserved.  A corner outside an open side face carries flux 0.
C2R_HD void plane_layer_flux(const PlaneTilt &T, int fa, int fb, int u, int v, const double *fprev, double (&nf)[NSED]) {
  const int uu = plane_upstream(u, T.e_f, fa, T.wrap_f), vv = plane_upstream(v, T.e_g, fb, T.wrap_g);
  const int face = fa * fb;
  const int at[4] = {uu >= 0 && vv >= 0 ? uu + fa * vv : -1, vv >= 0 ? u + fa * vv : -1, uu >= 0 ? uu + fa * v : -1, u + fa * v};
  for (int k = 0; k < NSED; k++) {
    double F[4];
    for (int i = 0; i < 4; i++) F[i] = at[i] >= 0 ? fprev[k * face + at[i]] : 0.0;
    nf[k] = F[0] * T.s[0] + F[1] * T.s[1] + F[2] * T.s[2] + F[3] * T.s[3];
  }
}

// Side entry (c2r_set_plane_side_entry, include/c2ray_hip.h): what a corner that falls outside an open side face reads
// instead of 0.0 -- the ghost cells of the layer before, handed in by the mesh that stands there.  One slot of the strips:
// side[0]: 3 x fb values at the corner's index along g (outside along f only), side[1]: 3 x fa values at its index along f
// (outside along g only), corner: 3 values (outside along both); the species or the SED slowest.  A null pointer is a strip
// that is not set, or whose side is not live in this pass: 0.0, as ever.
struct PlaneGhost {
  const double *side[2];
  const double *corner;
};

// the value of species or SED k at the corner (uu, vv) of plane_layer_in (-1: outside an open side face); `prev` null: zero
C2R_HD double plane_corner_value(const double *prev, const PlaneGhost &gh, int k, int fa, int fb, int uu, int vv) {
  if (uu >= 0 && vv >= 0) return prev ? prev[k * (fa * fb) + uu + fa * vv] : 0.0;
  if (vv >= 0) return gh.side[0] ? gh.side[0][k * fb + vv] : 0.0;
  if (uu >= 0) return gh.side[1] ? gh.side[1][k * fa + uu] : 0.0;
  return gh.corner ? gh.corner[k] : 0.0;
}

// plane_layer_in with ghost cells: the same four corners, the same plane_interp
C2R_HD void plane_layer_in(const PlaneTilt &T, int fa, int fb, int u, int v, const double *prev, const PlaneGhost &gh, double &c_HI,
                           double &c_HeI, double &c_HeII) {
  const int uu = plane_upstream(u, T.e_f, fa, T.wrap_f), vv = plane_upstream(v, T.e_g, fb, T.wrap_g);
  double c[3][4];
  for (int k = 0; k < 3; k++) {
    c[k][0] = plane_corner_value(prev, gh, k, fa, fb, uu, vv);
    c[k][1] = plane_corner_value(prev, gh, k, fa, fb, u, vv);
    c[k][2] = plane_corner_value(prev, gh, k, fa, fb, uu, v);
    c[k][3] = plane_corner_value(prev, gh, k, fa, fb, u, v);
  }
  c_HI = plane_interp(T.s, c[0][0], c[0][1], c[0][2], c[0][3], sigma_HI_at_ion_freq);
  c_HeI = plane_interp(T.s, c[1][0], c[1][1], c[1][2], c[1][3], sigma_HeI_at_ion_freq);
  c_HeII = plane_interp(T.s, c[2][0], c[2][1], c[2][2], c[2][3], sigma_HeII_at_ion_freq);
}

// plane_layer_flux with ghost cells (`gh`: the flux strips)
C2R_HD void plane_layer_flux(const PlaneTilt &T, int fa, int fb, int u, int v, const double *fprev, const PlaneGhost &gh,
                             double (&nf)[NSED]) {
  const int uu = plane_upstream(u, T.e_f, fa, T.wrap_f), vv = plane_upstream(v, T.e_g, fb, T.wrap_g);
  for (int k = 0; k < NSED; k++) {
    const double F1 = plane_corner_value(fprev, gh, k, fa, fb, uu, vv), F2 = plane_corner_value(fprev, gh, k, fa, fb, u, vv),
                 F3 = plane_corner_value(fprev, gh, k, fa, fb, uu, v), F4 = plane_corner_value(fprev, gh, k, fa, fb, u, v);
    nf[k] = F1 * T.s[0] + F2 * T.s[1] + F3 * T.s[2] + F4 * T.s[3];
  }
}

} // namespace c2r
