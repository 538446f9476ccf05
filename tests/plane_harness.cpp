// TEST-ONLY: the per-cell rule of the plane-parallel sources (c2-ray3dm1d_helium_amd/csrc/c2ray_plane.hpp) compiled with
// the host C++ compiler, marching a whole mesh the way k_plane_columns / k_plane_rates / k_plane_exit do on the device,
// so that tests/test_plane_reference_host.py can hold it to the NumPy reference (tests/plane_reference.py) bit for bit
// before the code reaches a GPU.  Nothing in the product links this file.
//   g++ -O2 -ffp-contract=off -mfma -fPIC -shared -std=c++17 -o _plane_harness.so plane_harness.cpp
#include <cstddef>
#include <cstring>
#include <vector>

#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_device.hpp"
#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_plane.hpp"

using namespace c2r;

namespace {
struct Tables {
  BandDataByRow bd;
  std::vector<double> pthick, pthin, hthick, hthin, hthick_il, hthin_il;
};
Tables T;

void pitch(const double *src, int ncol, std::vector<double> &dst) {
  dst.assign((size_t)ncol * NTAUP, 0.0);
  for (int c = 0; c < ncol; c++) {
    std::memcpy(&dst[(size_t)c * NTAUP], src + (size_t)c * (NTAU + 1), sizeof(double) * (NTAU + 1));
    dst[(size_t)c * NTAUP + NTAU + 1] = src[(size_t)c * (NTAU + 1) + NTAU];
  }
}
} // namespace

extern "C" {

// the black-body tables, as c2r_set_tables prepares them (pitch, tau_zero, interleaved heating tables)
void ph_set_tables(const double *pthick, const double *pthin, const double *hthick, const double *hthin, const double *sHI,
                   const double *sHeI, const double *sHeII, const double *const f[12], int bb_upper) {
  std::memset(&T.bd, 0, sizeof T.bd);
  pitch(pthick, NFREQ, T.pthick);
  pitch(pthin, NFREQ, T.pthin);
  pitch(hthick, NHEAT, T.hthick);
  pitch(hthin, NHEAT, T.hthin);
  std::memcpy(T.bd.sigma_HI, sHI, sizeof T.bd.sigma_HI);
  std::memcpy(T.bd.sigma_HeI, sHeI, sizeof T.bd.sigma_HeI);
  std::memcpy(T.bd.sigma_HeII, sHeII, sizeof T.bd.sigma_HeII);
  double *dst[12] = {T.bd.f1ion_HI, T.bd.f1ion_HeI, T.bd.f1ion_HeII, T.bd.f2ion_HI, T.bd.f2ion_HeI, T.bd.f2ion_HeII,
                     T.bd.f1heat_HI, T.bd.f1heat_HeI, T.bd.f1heat_HeII, T.bd.f2heat_HI, T.bd.f2heat_HeI, T.bd.f2heat_HeII};
  for (int i = 0; i < 12; i++) std::memcpy(dst[i], f[i], sizeof(double) * (NFREQ - 1));
  T.bd.bb_upper = bb_upper;
  band_rows_fill(T.bd);
  for (int b = 0; b < NFREQ; b++) {
    const double *cols[8];
    int n = 0;
    cols[n++] = &T.pthick[(size_t)b * NTAUP];
    cols[n++] = &T.pthin[(size_t)b * NTAUP];
    for (int k = 0; k < heat_species(b); k++) {
      cols[n++] = &T.hthick[(size_t)(heat_first_col(b) + k) * NTAUP];
      cols[n++] = &T.hthin[(size_t)(heat_first_col(b) + k) * NTAUP];
    }
    T.bd.tau_zero[0][b] = band_tau_zero(cols, n);
    T.bd.tau_zero[1][b] = T.bd.tau_zero[2][b] = (double)INFINITY;
  }
  T.hthick_il.resize(T.hthick.size());
  T.hthin_il.resize(T.hthin.size());
  heat_interleave(T.hthick.data(), T.hthick_il.data());
  heat_interleave(T.hthin.data(), T.hthin_il.data());
}

// One plane (black-body flux `nflux` per cm^2 of face) over a whole mesh, the three device kernels' work in their order:
// the march of every column (incoming columns of every cell, exit columns), the rates of every cell, the exit term of
// every column.  rates: [phih | phihe0 | phihe1 | phiheat] of ncell each, ADDED to what is there; exit3: 3 x face;
// terms: face.  entry3 / lls_grid may be null.  Returns 0, or 1 + the number of mesh cells the marches did not visit
// exactly once (the cell map of plane_geometry / plane_cell, which the kernels index device memory with).
int ph_march(const int *mesh, const double *dr, double vol, const double *ndens, const double *xh_av, const double *xhe_av, int axis,
             int from_high, double nflux, int heat, int use_lls, double coldensh_lls, const float *lls_grid, const double *entry3,
             double *rates, double *exit3, double *terms) {
  const size_t nc = (size_t)mesh[0] * mesh[1] * mesh[2];
  const PlaneGeom G = plane_geometry(mesh[0], mesh[1], mesh[2], axis, from_high);
  const int face = G.fa * G.fb;
  const double path = dr[axis];
  const double nf[NSED] = {nflux, 0.0, 0.0};
  SedSet ss{};
  ss.photo_thick[0] = T.pthick.data(); ss.photo_thin[0] = T.pthin.data();
  ss.heat_thick[0] = T.hthick_il.data(); ss.heat_thin[0] = T.hthin_il.data();
  ss.lo[0] = 0; ss.hi[0] = T.bd.bb_upper;
  const BandData &bd = T.bd;
  std::vector<double> cin(3 * nc, -1.0);
  std::vector<int> visits(nc, 0);
  int bad = 0;
  for (int f = 0; f < face; f++) { // k_plane_columns
    double c_HI = entry3 ? entry3[f] : 0.0, c_HeI = entry3 ? entry3[face + f] : 0.0, c_HeII = entry3 ? entry3[2 * face + f] : 0.0;
    for (int m = 0; m < G.na; m++) {
      const size_t q = plane_cell(G, f, m);
      if (q >= nc) { bad++; continue; }
      visits[q]++;
      const double lls = use_lls ? (lls_grid ? (double)lls_grid[q] : coldensh_lls) : 0.0;
      double o_HI, o_HeI, o_HeII;
      plane_cell_columns(ndens[q], xh_av[q], xhe_av[q], xhe_av[q + nc], path, dr[0], use_lls, lls, c_HI, c_HeI, c_HeII, o_HI, o_HeI, o_HeII);
      cin[3 * q] = c_HI; cin[3 * q + 1] = c_HeI; cin[3 * q + 2] = c_HeII;
      c_HI = o_HI; c_HeI = o_HeI; c_HeII = o_HeII;
    }
    exit3[f] = c_HI; exit3[face + f] = c_HeI; exit3[2 * face + f] = c_HeII;
  }
  for (size_t q = 0; q < nc; q++)
    if (visits[q] != 1) bad++;
  if (bad) return 1 + bad;
  for (size_t q = 0; q < nc; q++) { // k_plane_rates
    double u_HI, u_HeI, u_HeII, cout_HI, cout_HeI, cout_HeII, add[4];
    plane_cell_state(ndens[q], xh_av[q], xhe_av[q], xhe_av[q + nc], u_HI, u_HeI, u_HeII);
    plane_cell_out(cin[3 * q], cin[3 * q + 1], cin[3 * q + 2], u_HI, u_HeI, u_HeII, path, cout_HI, cout_HeI, cout_HeII);
    const bool lit = heat ? plane_cell_rates<true, false>(bd, ss, cin[3 * q], cout_HI, cin[3 * q + 1], cout_HeI, cin[3 * q + 2], cout_HeII, path,
                                                          nf, xh_av[q + nc], u_HI, u_HeI, u_HeII, add, C2R_LOGTAB_DEFAULT)
                          : plane_cell_rates<false, false>(bd, ss, cin[3 * q], cout_HI, cin[3 * q + 1], cout_HeI, cin[3 * q + 2], cout_HeII, path,
                                                           nf, xh_av[q + nc], u_HI, u_HeI, u_HeII, add, C2R_LOGTAB_DEFAULT);
    if (!lit) continue;
    rates[q] = rates[q] + add[0];
    rates[q + nc] = rates[q + nc] + add[1];
    rates[q + 2 * nc] = rates[q + 2 * nc] + add[2];
    if (heat) rates[q + 3 * nc] = rates[q + 3 * nc] + add[3];
  }
  for (int f = 0; f < face; f++) { // k_plane_exit
    const size_t q = plane_cell(G, f, G.na - 1);
    terms[f] = plane_exit_term<false>(bd, ss, cin[3 * q], exit3[f], cin[3 * q + 1], exit3[face + f], cin[3 * q + 2], exit3[2 * face + f], nf,
                                      vol, path);
  }
  return 0;
}
}
