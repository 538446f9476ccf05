// TEST-ONLY: plane flux maps (c2r_set_plane_flux_map; plane_layer_flux and plane_dark of
// c2-ray3dm1d_helium_amd/csrc/c2ray_plane.hpp) compiled with the host C++ compiler, marching a whole mesh the way
// k_plane_columns or k_plane_layer<true>, k_plane_rates and k_plane_exit do on the device for a plane with a map, so that
// tests/test_flux_reference_host.py can hold it to the Python reference (tests/flux_reference.py) bit for bit before the
// code reaches a GPU.  Nothing in the product links this file.
//   g++ -O2 -ffp-contract=off -mfma -fPIC -shared -std=c++17 -o _flux_harness.so flux_harness.cpp
// With -DFLUX_MAIN it is a stand-alone program that marches columns and fluxes of a small mesh of made-up gas (the geometry
// and the advection only, no tables): the form in which a host sanitizer is applied to this code.
#include "plane_harness.cpp" // ph_set_tables and the tables it fills

namespace {
std::vector<double> S_pt[2], S_pn[2], S_ht[2], S_hn[2], S_ht_il[2], S_hn_il[2];
int S_lo[2] = {0, 0}, S_hi[2] = {0, 0};
bool S_set[2] = {false, false};

template <bool HEAT, bool MULTI>
static void fx_rates(size_t nc, double path, const SedSet &ss, const double *ndens, const double *xh_av, const double *xhe_av,
                     const double *cin, const double *cell_flux, double *rates) {
  for (size_t q = 0; q < nc; q++) { // k_plane_rates<.., PlaneFlux::by_cell>
    const double nf[NSED] = {cell_flux[3 * q], cell_flux[3 * q + 1], cell_flux[3 * q + 2]};
    if (plane_dark(nf)) continue;
    double u_HI, u_HeI, u_HeII, cout_HI, cout_HeI, cout_HeII, add[4];
    plane_cell_state(ndens[q], xh_av[q], xhe_av[q], xhe_av[q + nc], u_HI, u_HeI, u_HeII);
    plane_cell_out(cin[3 * q], cin[3 * q + 1], cin[3 * q + 2], u_HI, u_HeI, u_HeII, path, cout_HI, cout_HeI, cout_HeII);
    bool lit;
    if constexpr (HEAT && MULTI) // band by band, as the three-SED heating kernel reads the band data
      lit = plane_cell_rates<HEAT, MULTI>(T.bd, ss, cin[3 * q], cout_HI, cin[3 * q + 1], cout_HeI, cin[3 * q + 2], cout_HeII, path, nf,
                                          xh_av[q + nc], u_HI, u_HeI, u_HeII, add, C2R_LOGTAB_DEFAULT);
    else
      lit = plane_cell_rates<HEAT, MULTI>((const BandData &)T.bd, ss, cin[3 * q], cout_HI, cin[3 * q + 1], cout_HeI, cin[3 * q + 2], cout_HeII,
                                          path, nf, xh_av[q + nc], u_HI, u_HeI, u_HeII, add, C2R_LOGTAB_DEFAULT);
    if (!lit) continue;
    rates[q] = rates[q] + add[0];
    rates[q + nc] = rates[q + nc] + add[1];
    rates[q + 2 * nc] = rates[q + 2 * nc] + add[2];
    if (HEAT) rates[q + 3 * nc] = rates[q + 3 * nc] + add[3];
  }
}
} // namespace

extern "C" {

// the tables of SED 1 (power law) or 2 (quasar-like), as c2r_set_sed_tables prepares them; after ph_set_tables
void fx_set_sed(int sed, const double *pthick, const double *pthin, const double *hthick, const double *hthin, int lower, int upper) {
  const int k = sed - 1;
  pitch(pthick, NFREQ, S_pt[k]);
  pitch(pthin, NFREQ, S_pn[k]);
  pitch(hthick, NHEAT, S_ht[k]);
  pitch(hthin, NHEAT, S_hn[k]);
  S_lo[k] = lower - 1;
  S_hi[k] = upper;
  for (int b = 0; b < NFREQ; b++) {
    const double *cols[8];
    int n = 0;
    cols[n++] = &S_pt[k][(size_t)b * NTAUP];
    cols[n++] = &S_pn[k][(size_t)b * NTAUP];
    for (int i = 0; i < heat_species(b); i++) {
      cols[n++] = &S_ht[k][(size_t)(heat_first_col(b) + i) * NTAUP];
      cols[n++] = &S_hn[k][(size_t)(heat_first_col(b) + i) * NTAUP];
    }
    T.bd.tau_zero[sed][b] = band_tau_zero(cols, n);
  }
  S_ht_il[k].resize(S_ht[k].size());
  S_hn_il[k].resize(S_hn[k].size());
  heat_interleave(S_ht[k].data(), S_ht_il[k].data());
  heat_interleave(S_hn[k].data(), S_hn_il[k].data());
  S_set[k] = true;
}

// Columns and fluxes of a plane with a map over a whole mesh.  Tilted: layer by layer, two alternating face buffers for the
// columns and two for the flux (k_plane_layer<true>); untilted: every line on its own (k_plane_columns), the flux of a cell its
// line's map entry.  cin, cell_flux: 3 per cell; exit3, exit_flux: 3 x face.  Returns the number of cells not visited once.
int fx_columns(const int *mesh, const double *dr, const double *ndens, const double *xh_av, const double *xhe_av, int axis, int from_high,
               const double *tilt, const int *periodic, int use_lls, double coldensh_lls, const float *lls_grid, const double *entry3,
               const double *map3, double *cin, double *cell_flux, double *exit3, double *exit_flux) {
  const size_t nc = (size_t)mesh[0] * mesh[1] * mesh[2];
  const PlaneGeom G = plane_geometry(mesh[0], mesh[1], mesh[2], axis, from_high);
  const int face = G.fa * G.fb;
  std::vector<int> visits(nc, 0);
  int bad = 0;
  if (plane_tilted(tilt)) {
    const PlaneTilt Tl(tilt, dr, axis, periodic);
    std::vector<double> buf[2] = {std::vector<double>(3 * (size_t)face), std::vector<double>(3 * (size_t)face)};
    std::vector<double> fbuf[2] = {std::vector<double>(3 * (size_t)face), std::vector<double>(3 * (size_t)face)};
    const double *prev = entry3, *fprev = map3;
    for (int m = 0; m < G.na; m++) {
      double *next = m == G.na - 1 ? exit3 : buf[m & 1].data();
      double *fnext = m == G.na - 1 ? exit_flux : fbuf[m & 1].data();
      const int along = G.from_high ? G.na - 1 - m : m;
      for (int v = 0; v < G.fb; v++)
        for (int u = 0; u < G.fa; u++) {
          const size_t q = (size_t)u * G.sf + (size_t)v * G.sg + (size_t)along * G.sa;
          if (q >= nc || q != plane_cell(G, u + G.fa * v, m)) { bad++; continue; }
          visits[q]++;
          double c_HI, c_HeI, c_HeII, o_HI, o_HeI, o_HeII, nf[NSED];
          plane_layer_in(Tl, G.fa, G.fb, u, v, prev, c_HI, c_HeI, c_HeII);
          plane_layer_flux(Tl, G.fa, G.fb, u, v, fprev, nf);
          const double lls = use_lls ? (lls_grid ? (double)lls_grid[q] : coldensh_lls) : 0.0;
          plane_cell_columns(ndens[q], xh_av[q], xhe_av[q], xhe_av[q + nc], Tl.path, dr[0], use_lls, lls, c_HI, c_HeI, c_HeII, o_HI, o_HeI,
                             o_HeII);
          cin[3 * q] = c_HI; cin[3 * q + 1] = c_HeI; cin[3 * q + 2] = c_HeII;
          const int f = u + G.fa * v;
          next[f] = o_HI; next[face + f] = o_HeI; next[2 * face + f] = o_HeII;
          for (int k = 0; k < NSED; k++) cell_flux[3 * q + k] = fnext[k * face + f] = nf[k];
        }
      prev = next;
      fprev = fnext;
    }
  } else {
    const double path = dr[axis];
    for (int f = 0; f < face; f++) {
      double c_HI = entry3 ? entry3[f] : 0.0, c_HeI = entry3 ? entry3[face + f] : 0.0, c_HeII = entry3 ? entry3[2 * face + f] : 0.0;
      for (int m = 0; m < G.na; m++) {
        const size_t q = plane_cell(G, f, m);
        if (q >= nc) { bad++; continue; }
        visits[q]++;
        const double lls = use_lls ? (lls_grid ? (double)lls_grid[q] : coldensh_lls) : 0.0;
        double o_HI, o_HeI, o_HeII;
        plane_cell_columns(ndens[q], xh_av[q], xhe_av[q], xhe_av[q + nc], path, dr[0], use_lls, lls, c_HI, c_HeI, c_HeII, o_HI, o_HeI, o_HeII);
        cin[3 * q] = c_HI; cin[3 * q + 1] = c_HeI; cin[3 * q + 2] = c_HeII;
        for (int k = 0; k < NSED; k++) cell_flux[3 * q + k] = map3[k * face + f];
        c_HI = o_HI; c_HeI = o_HeI; c_HeII = o_HeII;
      }
      exit3[f] = c_HI; exit3[face + f] = c_HeI; exit3[2 * face + f] = c_HeII;
      for (int k = 0; k < NSED; k++) exit_flux[k * face + f] = map3[k * face + f];
    }
  }
  for (size_t q = 0; q < nc; q++)
    if (visits[q] != 1) bad++;
  return bad;
}

// One plane with the flux map map3 over a whole mesh, the device kernels' work in their order.  Arguments as ob_march of
// tests/oblique_harness.cpp with map3 for nflux (tilt {0, 0}: normal incidence), plus cell_flux (3 per cell) and exit_flux
// (3 x face).  Returns 0; -1 for a refused tilt, -2 for a map that needs tables fx_set_sed has not been given; or 1 + the
// number of cells not visited exactly once.
int fx_march(const int *mesh, const double *dr, double vol, const double *ndens, const double *xh_av, const double *xhe_av, int axis,
             int from_high, const double *map3, const double *tilt, const int *periodic, int heat, int use_lls, double coldensh_lls,
             const float *lls_grid, const double *entry3, double *rates, double *exit3, double *terms, double *cin_HI, double *cell_flux,
             double *exit_flux) {
  const size_t nc = (size_t)mesh[0] * mesh[1] * mesh[2];
  const PlaneGeom G = plane_geometry(mesh[0], mesh[1], mesh[2], axis, from_high);
  const int face = G.fa * G.fb;
  double path = dr[axis];
  if (plane_tilted(tilt)) {
    const PlaneTilt Tl(tilt, dr, axis, periodic);
    if (!Tl.valid()) return -1;
    path = Tl.path;
  }
  bool uses[2] = {false, false};
  for (int i = face; i < 3 * face; i++)
    if (map3[i] != 0.0) uses[i / face - 1] = true;
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
  std::vector<double> cin(3 * nc, -1.0);
  if (const int bad = fx_columns(mesh, dr, ndens, xh_av, xhe_av, axis, from_high, tilt, periodic, use_lls, coldensh_lls, lls_grid, entry3, map3,
                                 cin.data(), cell_flux, exit3, exit_flux))
    return 1 + bad;
  for (size_t q = 0; q < nc; q++) cin_HI[q] = cin[3 * q];
  if (heat) multi ? fx_rates<true, true>(nc, path, ss, ndens, xh_av, xhe_av, cin.data(), cell_flux, rates)
                  : fx_rates<true, false>(nc, path, ss, ndens, xh_av, xhe_av, cin.data(), cell_flux, rates);
  else multi ? fx_rates<false, true>(nc, path, ss, ndens, xh_av, xhe_av, cin.data(), cell_flux, rates)
             : fx_rates<false, false>(nc, path, ss, ndens, xh_av, xhe_av, cin.data(), cell_flux, rates);
  const BandData &bd = T.bd;
  for (int f = 0; f < face; f++) { // k_plane_exit<.., MAPPED>
    const double nf[NSED] = {exit_flux[f], exit_flux[face + f], exit_flux[2 * face + f]};
    if (plane_dark(nf)) { terms[f] = 0.0; continue; }
    const size_t q = plane_cell(G, f, G.na - 1);
    terms[f] = multi ? plane_exit_term<true>(bd, ss, cin[3 * q], exit3[f], cin[3 * q + 1], exit3[face + f], cin[3 * q + 2], exit3[2 * face + f],
                                             nf, vol, path)
                     : plane_exit_term<false>(bd, ss, cin[3 * q], exit3[f], cin[3 * q + 1], exit3[face + f], cin[3 * q + 2], exit3[2 * face + f],
                                              nf, vol, path);
  }
  return 0;
}
}

#ifdef FLUX_MAIN
// Stand-alone: columns and fluxes of every (axis, side), both tilt signs and no tilt, wrapped and open face axes, on a
// 7 x 6 x 5 mesh of made-up gas with a map that has a dark block.  Prints a checksum; a sanitizer build of this program
// checks every index the marches form.
#include <cstdio>
int main() {
  const int mesh[3] = {7, 6, 5};
  const double dr[3] = {1.0e22, 1.3e22, 0.8e22};
  const size_t nc = 7 * 6 * 5;
  std::vector<double> ndens(nc), xh(2 * nc), xhe(3 * nc), cin(3 * nc), cflux(3 * nc);
  for (size_t q = 0; q < nc; q++) {
    ndens[q] = 1.0e-4 * (1.0 + 0.1 * (double)(q % 13));
    xh[q] = 0.9; xh[nc + q] = 0.1;
    xhe[q] = 0.9; xhe[nc + q] = 0.08; xhe[2 * nc + q] = 0.02;
  }
  double sum = 0.0;
  int bad = 0;
  for (int axis = 0; axis < 3; axis++)
    for (int side = 0; side < 2; side++)
      for (int sign = -1; sign <= 1; sign++)
        for (int wrap = 0; wrap < 4; wrap++) {
          const int f = axis == 0 ? 1 : 0, g = axis == 2 ? 1 : 2;
          int per[3] = {0, 0, 0};
          per[f] = wrap & 1; per[g] = wrap >> 1;
          const double tilt[2] = {0.4 * sign, -0.6 * sign};
          if (!PlaneTilt(tilt, dr, axis, per).valid()) bad++;
          const int face = mesh[f] * mesh[g];
          std::vector<double> exit3(3 * (size_t)face), map3(3 * (size_t)face), fexit(3 * (size_t)face);
          for (int i = 0; i < 3 * face; i++) map3[i] = i % 5 == 0 ? 0.0 : 1.0 + (double)(i % 7);
          bad += fx_columns(mesh, dr, ndens.data(), xh.data(), xhe.data(), axis, side, tilt, per, 1, 1.0e16, nullptr, nullptr, map3.data(),
                            cin.data(), cflux.data(), exit3.data(), fexit.data());
          for (double x : exit3) sum += x * 1.0e-18;
          for (double x : fexit) sum += x;
          for (double x : cflux) sum += x * 1.0e-3;
        }
  std::printf("cells missed or repeated: %d, checksum %.17g\n", bad, sum);
  return bad != 0;
}
#endif
