// TEST-ONLY: plane light curves (c2r_set_plane_curve; c2-ray3dm1d_helium_amd/csrc/c2ray_pcurve.hpp) compiled with the host
// C++ compiler, marching a whole mesh the way k_plane_columns or k_plane_layer, k_pcurve_rates and k_pcurve_exit do on the
// device for a plane with a curve, so that tests/test_plane_curve_host.py can hold it to the Python reference
// (tests/plane_curve_reference.py) bit for bit before the code reaches a GPU.  Nothing in the product links this file.
//   g++ -O2 -ffp-contract=off -mfma -fPIC -shared -std=c++17 -o _plane_curve_harness.so plane_curve_harness.cpp
// With -DPCURVE_MAIN it is a stand-alone program that finds the layer and the factor of every cell of a small mesh for every
// face (the geometry and the rule only, no tables): the form in which a host sanitizer is applied to this code.
#include "flux_harness.cpp" // fx_columns, fx_set_sed and, through plane_harness.cpp, ph_set_tables and the tables

#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_pcurve.hpp"

namespace {
// k_pcurve_rates<HEAT, MULTI, ..>: every cell finds its layer from its own (i, j, k)
template <bool HEAT, bool MULTI>
static int pc_rates(const int *mesh, const PlaneLayerIndex &lx, const PlaneCurveDev &cv, double path, const SedSet &ss, const double *ndens,
                    const double *xh_av, const double *xhe_av, const double *cin, const double *cell_flux, double *rates, int *layer_of) {
  const size_t nc = (size_t)mesh[0] * mesh[1] * mesh[2];
  int unlit = 0;
  for (int k = 0; k < mesh[2]; k++)
    for (int j = 0; j < mesh[1]; j++)
      for (int i = 0; i < mesh[0]; i++) {
        const size_t q = (size_t)i + (size_t)mesh[0] * ((size_t)j + (size_t)mesh[1] * (size_t)k);
        const int m = pcurve_layer(lx, i, j, k);
        layer_of[q] = m;
        const double cf = pcurve_factor(cv, m, path);
        if (cf == 0.0) { unlit++; continue; }
        const double nfu[NSED] = {cell_flux[3 * q], cell_flux[3 * q + 1], cell_flux[3 * q + 2]};
        if (plane_dark(nfu)) continue;
        double u_HI, u_HeI, u_HeII, cout_HI, cout_HeI, cout_HeII, add[4];
        plane_cell_state(ndens[q], xh_av[q], xhe_av[q], xhe_av[q + nc], u_HI, u_HeI, u_HeII);
        plane_cell_out(cin[3 * q], cin[3 * q + 1], cin[3 * q + 2], u_HI, u_HeI, u_HeII, path, cout_HI, cout_HeI, cout_HeII);
        bool lit;
        if constexpr (HEAT && MULTI) { // each product formed where it is used, band by band
          lit = plane_cell_rates<HEAT, MULTI>(T.bd, ss, cin[3 * q], cout_HI, cin[3 * q + 1], cout_HeI, cin[3 * q + 2], cout_HeII, path,
                                              PlaneCurveFlux{nfu[0], nfu[1], nfu[2], cf}, xh_av[q + nc], u_HI, u_HeI, u_HeII, add, C2R_LOGTAB_DEFAULT);
        } else {
          double nf[NSED];
          pcurve_fluxes(nfu, cf, nf);
          lit = plane_cell_rates<HEAT, MULTI>((const BandData &)T.bd, ss, cin[3 * q], cout_HI, cin[3 * q + 1], cout_HeI, cin[3 * q + 2], cout_HeII,
                                              path, nf, xh_av[q + nc], u_HI, u_HeI, u_HeII, add, C2R_LOGTAB_DEFAULT);
        }
        if (!lit) continue;
        rates[q] = rates[q] + add[0];
        rates[q + nc] = rates[q + nc] + add[1];
        rates[q + 2 * nc] = rates[q + 2 * nc] + add[2];
        if (HEAT) rates[q + 3 * nc] = rates[q + 3 * nc] + add[3];
      }
  return unlit;
}
} // namespace

extern "C" {

// the factor of each of `na` layers, by the functions the kernels and the host of the product use
void pc_layer_factors(int nstep, const double *depth, const double *factor, int layer0, double depth0, double path, int na, double *out) {
  PlaneCurveDev cv;
  pcurve_fill(nstep, depth, factor, layer0, depth0, cv);
  for (int m = 0; m < na; m++) out[m] = pcurve_factor(cv, m, path);
}

// One plane with a curve over a whole mesh, the device kernels' work in their order.  nflux3: the uniform normflux (map3
// null), or map3: 3 x face.  Everything else as fx_march of tests/flux_harness.cpp; factors: mesh[axis] doubles, the f of
// every layer.  Returns 0; -1 for a refused tilt, -2 for fluxes that need tables fx_set_sed has not been given, -3 where a
// cell's layer is not the layer of its place in the march; or 1 + the number of cells not visited exactly once.
int pc_march(const int *mesh, const double *dr, double vol, const double *ndens, const double *xh_av, const double *xhe_av, int axis,
             int from_high, const double *nflux3, const double *map3, int nstep, const double *depth, const double *factor, int layer0,
             double depth0, const double *tilt, const int *periodic, int heat, int use_lls, double coldensh_lls, const float *lls_grid,
             const double *entry3, double *rates, double *exit3, double *terms, double *cin_HI, double *cell_flux, double *exit_flux,
             double *factors) {
  const size_t nc = (size_t)mesh[0] * mesh[1] * mesh[2];
  const PlaneGeom G = plane_geometry(mesh[0], mesh[1], mesh[2], axis, from_high);
  const int face = G.fa * G.fb;
  double path = dr[axis];
  if (plane_tilted(tilt)) {
    const PlaneTilt Tl(tilt, dr, axis, periodic);
    if (!Tl.valid()) return -1;
    path = Tl.path;
  }
  const bool mapped = map3 != nullptr;
  std::vector<double> uniform(3 * (size_t)face);
  if (!mapped)
    for (int i = 0; i < 3 * face; i++) uniform[i] = nflux3[i / face];
  const double *unscaled = mapped ? map3 : uniform.data();
  bool uses[2] = {false, false};
  for (int i = face; i < 3 * face; i++)
    if (unscaled[i] != 0.0) uses[i / face - 1] = true;
  const bool multi = uses[0] || uses[1];
  SedSet ss{};
  ss.photo_thick[0] = T.pthick.data(); ss.photo_thin[0] = T.pthin.data();
  ss.heat_thick[0] = T.hthick_il.data(); ss.heat_thin[0] = T.hthin_il.data();
  ss.lo[0] = 0; ss.hi[0] = T.bd.bb_upper;
  for (int k = 0; k < 2; k++) {
    if (uses[k] && !S_set[k]) return -2;
    if (!S_set[k]) continue;
    ss.photo_thick[k + 1] = S_pt[k].data(); ss.photo_thin[k + 1] = S_pn[k].data();
    ss.heat_thick[k + 1] = S_ht_il[k].data(); ss.heat_thin[k + 1] = S_hn_il[k].data();
    ss.lo[k + 1] = S_lo[k]; ss.hi[k + 1] = S_hi[k];
  }
  // the march is the uncurved plane's (a uniform plane carries no flux: its cells and its exit see normflux)
  std::vector<double> cin(3 * nc, -1.0);
  if (const int bad = fx_columns(mesh, dr, ndens, xh_av, xhe_av, axis, from_high, tilt, periodic, use_lls, coldensh_lls, lls_grid, entry3,
                                 unscaled, cin.data(), cell_flux, exit3, exit_flux))
    return 1 + bad;
  if (!mapped) {
    for (size_t q = 0; q < nc; q++)
      for (int k = 0; k < NSED; k++) cell_flux[3 * q + k] = nflux3[k];
    for (int i = 0; i < 3 * face; i++) exit_flux[i] = uniform[i];
  }
  for (size_t q = 0; q < nc; q++) cin_HI[q] = cin[3 * q];
  PlaneCurveDev cv;
  pcurve_fill(nstep, depth, factor, layer0, depth0, cv);
  for (int m = 0; m < G.na; m++) factors[m] = pcurve_factor(cv, m, path);
  const PlaneLayerIndex lx = plane_layer_index(axis, from_high, G.na);
  std::vector<int> layer_of(nc, -1);
  if (heat) multi ? pc_rates<true, true>(mesh, lx, cv, path, ss, ndens, xh_av, xhe_av, cin.data(), cell_flux, rates, layer_of.data())
                  : pc_rates<true, false>(mesh, lx, cv, path, ss, ndens, xh_av, xhe_av, cin.data(), cell_flux, rates, layer_of.data());
  else multi ? pc_rates<false, true>(mesh, lx, cv, path, ss, ndens, xh_av, xhe_av, cin.data(), cell_flux, rates, layer_of.data())
             : pc_rates<false, false>(mesh, lx, cv, path, ss, ndens, xh_av, xhe_av, cin.data(), cell_flux, rates, layer_of.data());
  for (int f = 0; f < face; f++)
    for (int m = 0; m < G.na; m++)
      if (layer_of[plane_cell(G, f, m)] != m) return -3;
  const BandData &bd = T.bd;
  const double cf = pcurve_factor(cv, G.na - 1, path); // (the host of the product forms the last layer's factor like this)
  for (int f = 0; f < face; f++) { // k_pcurve_exit
    const double nfu[NSED] = {exit_flux[f], exit_flux[face + f], exit_flux[2 * face + f]};
    terms[f] = 0.0;
    if (cf == 0.0 || plane_dark(nfu)) continue;
    double nf[NSED];
    pcurve_fluxes(nfu, cf, nf);
    const size_t q = plane_cell(G, f, G.na - 1);
    terms[f] = multi ? plane_exit_term<true>(bd, ss, cin[3 * q], exit3[f], cin[3 * q + 1], exit3[face + f], cin[3 * q + 2], exit3[2 * face + f],
                                             nf, vol, path)
                     : plane_exit_term<false>(bd, ss, cin[3 * q], exit3[f], cin[3 * q + 1], exit3[face + f], cin[3 * q + 2], exit3[2 * face + f],
                                              nf, vol, path);
  }
  return 0;
}
}

#ifdef PCURVE_MAIN
// Stand-alone: for every (axis, side) of a 7 x 6 x 5 mesh, every cell's layer by pcurve_layer against its place in the march,
// and the factor of every layer for curves of 0, 3 and 8 steps with layer0 and depth0.  Prints a checksum; a sanitizer build
// of this program checks every index and every table read the rule forms.
#include <cstdio>
int main() {
  const int mesh[3] = {7, 6, 5};
  const double dr[3] = {1.0e22, 1.3e22, 0.8e22};
  const size_t nc = 7 * 6 * 5;
  double sum = 0.0;
  int bad = 0;
  for (int axis = 0; axis < 3; axis++)
    for (int side = 0; side < 2; side++) {
      const PlaneGeom G = plane_geometry(mesh[0], mesh[1], mesh[2], axis, side);
      const PlaneLayerIndex lx = plane_layer_index(axis, side, G.na);
      std::vector<int> seen(nc, 0);
      for (int f = 0; f < G.fa * G.fb; f++)
        for (int m = 0; m < G.na; m++) {
          const size_t q = plane_cell(G, f, m);
          if (q >= nc) { bad++; continue; }
          seen[q]++;
          const int i = (int)(q % 7), j = (int)((q / 7) % 6), k = (int)(q / 42);
          if (pcurve_layer(lx, i, j, k) != m) bad++;
        }
      for (size_t q = 0; q < nc; q++)
        if (seen[q] != 1) bad++;
      for (int nstep : {0, 3, PCURVE_MAX_STEPS}) {
        double depth[PCURVE_MAX_STEPS], factor[PCURVE_MAX_STEPS + 1];
        for (int s = 0; s < nstep; s++) depth[s] = (0.7 + 0.9 * s) * dr[axis];
        for (int s = 0; s <= nstep; s++) factor[s] = s % 3 == 2 ? 0.0 : 1.0 / (1.0 + s);
        std::vector<double> out((size_t)G.na);
        pc_layer_factors(nstep, depth, factor, 2, 0.25 * dr[axis], dr[axis], G.na, out.data());
        for (double x : out) sum += x;
      }
    }
  std::printf("cells missed or repeated: %d, checksum %.17g\n", bad, sum);
  return bad != 0;
}
#endif
