// TEST-ONLY: the tilted plane (c2r_set_plane_tilt; PlaneTilt, plane_layer_in and plane_interp of
// c2-ray3dm1d_helium_amd/csrc/c2ray_plane.hpp) compiled with the host C++ compiler, marching a whole mesh layer by layer
// the way k_plane_layer / k_plane_rates / k_plane_exit do on the device, so that tests/test_oblique_reference_host.py can
// hold it to the Python reference (tests/oblique_reference.py) bit for bit before the code reaches a GPU.  Nothing in the
// product links this file.
//   g++ -O2 -ffp-contract=off -mfma -fPIC -shared -std=c++17 -o _oblique_harness.so oblique_harness.cpp
// With -DOBLIQUE_MAIN it is a stand-alone program that marches a small mesh of made-up tables-free columns (the geometry
// and the interpolation only): the form in which a host sanitizer is applied to this code.
#include "plane_harness.cpp" // ph_set_tables and the tables it fills

extern "C" {

// the geometry as the product forms it: out = a_f, a_g, s1..s4, path, e_f, e_g, wrap_f, wrap_g, valid
void ob_geometry(const double *tilt, const double *dr, int axis, const int *periodic, double *out) {
  const PlaneTilt Tl(tilt, dr, axis, periodic);
  const double v[12] = {Tl.a_f, Tl.a_g, Tl.s[0], Tl.s[1], Tl.s[2], Tl.s[3], Tl.path, (double)Tl.e_f, (double)Tl.e_g,
                        (double)Tl.wrap_f, (double)Tl.wrap_g, Tl.valid() ? 1.0 : 0.0};
  for (int i = 0; i < 12; i++) out[i] = v[i];
}

// The columns of a tilted plane over a whole mesh, one layer after the other with two alternating face buffers, the last
// layer into exit3: cin (3 per cell, fogged) and exit3 (3 x face).  Returns the number of mesh cells not visited exactly once.
int ob_columns(const int *mesh, const double *dr, const double *ndens, const double *xh_av, const double *xhe_av, int axis, int from_high,
               const double *tilt, const int *periodic, int use_lls, double coldensh_lls, const float *lls_grid, const double *entry3,
               double *cin, double *exit3) {
  const size_t nc = (size_t)mesh[0] * mesh[1] * mesh[2];
  const PlaneGeom G = plane_geometry(mesh[0], mesh[1], mesh[2], axis, from_high);
  const PlaneTilt Tl(tilt, dr, axis, periodic);
  const int face = G.fa * G.fb;
  std::vector<double> buf[2] = {std::vector<double>(3 * (size_t)face), std::vector<double>(3 * (size_t)face)};
  std::vector<int> visits(nc, 0);
  const double *prev = entry3;
  int bad = 0;
  for (int m = 0; m < G.na; m++) {
    double *next = m == G.na - 1 ? exit3 : buf[m & 1].data();
    const int along = G.from_high ? G.na - 1 - m : m;
    for (int v = 0; v < G.fb; v++)
      for (int u = 0; u < G.fa; u++) {
        const size_t q = (size_t)u * G.sf + (size_t)v * G.sg + (size_t)along * G.sa;
        if (q >= nc || q != plane_cell(G, u + G.fa * v, m)) { bad++; continue; }
        visits[q]++;
        double c_HI, c_HeI, c_HeII, o_HI, o_HeI, o_HeII;
        plane_layer_in(Tl, G.fa, G.fb, u, v, prev, c_HI, c_HeI, c_HeII);
        const double lls = use_lls ? (lls_grid ? (double)lls_grid[q] : coldensh_lls) : 0.0;
        plane_cell_columns(ndens[q], xh_av[q], xhe_av[q], xhe_av[q + nc], Tl.path, dr[0], use_lls, lls, c_HI, c_HeI, c_HeII, o_HI, o_HeI,
                           o_HeII);
        cin[3 * q] = c_HI; cin[3 * q + 1] = c_HeI; cin[3 * q + 2] = c_HeII;
        const int f = u + G.fa * v;
        next[f] = o_HI; next[face + f] = o_HeI; next[2 * face + f] = o_HeII;
      }
    prev = next;
  }
  for (size_t q = 0; q < nc; q++)
    if (visits[q] != 1) bad++;
  return bad;
}

// One tilted plane (black-body flux `nflux` per cm^2 perpendicular to the beam) over a whole mesh, the device kernels' work
// in their order: the layers, the rates of every cell (k_plane_rates with the tilted path), the exit term of every line.
// Arguments as ph_march, plus tilt[2], periodic[3] and cin_HI (ncell, out).  Returns 0, or 1 + the number of cells the
// layers did not visit exactly once.
int ob_march(const int *mesh, const double *dr, double vol, const double *ndens, const double *xh_av, const double *xhe_av, int axis,
             int from_high, double nflux, const double *tilt, const int *periodic, int heat, int use_lls, double coldensh_lls,
             const float *lls_grid, const double *entry3, double *rates, double *exit3, double *terms, double *cin_HI) {
  const size_t nc = (size_t)mesh[0] * mesh[1] * mesh[2];
  const PlaneGeom G = plane_geometry(mesh[0], mesh[1], mesh[2], axis, from_high);
  const PlaneTilt Tl(tilt, dr, axis, periodic);
  if (!Tl.valid() || !plane_tilted(tilt)) return -1;
  const int face = G.fa * G.fb;
  const double path = Tl.path;
  const double nf[NSED] = {nflux, 0.0, 0.0};
  SedSet ss{};
  ss.photo_thick[0] = T.pthick.data(); ss.photo_thin[0] = T.pthin.data();
  ss.heat_thick[0] = T.hthick_il.data(); ss.heat_thin[0] = T.hthin_il.data();
  ss.lo[0] = 0; ss.hi[0] = T.bd.bb_upper;
  const BandData &bd = T.bd;
  std::vector<double> cin(3 * nc, -1.0);
  if (const int bad = ob_columns(mesh, dr, ndens, xh_av, xhe_av, axis, from_high, tilt, periodic, use_lls, coldensh_lls, lls_grid, entry3,
                                 cin.data(), exit3))
    return 1 + bad;
  for (size_t q = 0; q < nc; q++) { // k_plane_rates
    cin_HI[q] = cin[3 * q];
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

#ifdef OBLIQUE_MAIN
// Stand-alone: the columns of every (axis, side), both tilt signs, wrapped and open face axes, on a 7 x 6 x 5 mesh of made-up
// gas.  Prints a checksum; a sanitizer build of this program checks every index the march forms.
#include <cstdio>
int main() {
  const int mesh[3] = {7, 6, 5};
  const double dr[3] = {1.0e22, 1.3e22, 0.8e22};
  const size_t nc = 7 * 6 * 5;
  std::vector<double> ndens(nc), xh(2 * nc), xhe(3 * nc), cin(3 * nc);
  for (size_t q = 0; q < nc; q++) {
    ndens[q] = 1.0e-4 * (1.0 + 0.1 * (double)(q % 13));
    xh[q] = 0.9; xh[nc + q] = 0.1;
    xhe[q] = 0.9; xhe[nc + q] = 0.08; xhe[2 * nc + q] = 0.02;
  }
  double sum = 0.0;
  int bad = 0;
  for (int axis = 0; axis < 3; axis++)
    for (int side = 0; side < 2; side++)
      for (int sign = -1; sign <= 1; sign += 2)
        for (int wrap = 0; wrap < 4; wrap++) {
          const int f = axis == 0 ? 1 : 0, g = axis == 2 ? 1 : 2;
          int per[3] = {0, 0, 0};
          per[f] = wrap & 1; per[g] = wrap >> 1;
          const double tilt[2] = {0.4 * sign, -0.6 * sign}; // a <= 1 for every axis with these cell sizes
          if (!PlaneTilt(tilt, dr, axis, per).valid()) bad++;
          const int face = mesh[f] * mesh[g];
          std::vector<double> exit3(3 * (size_t)face);
          bad += ob_columns(mesh, dr, ndens.data(), xh.data(), xhe.data(), axis, side, tilt, per, 1, 1.0e16, nullptr, nullptr, cin.data(),
                            exit3.data());
          for (double x : exit3) sum += x * 1.0e-18;
        }
  std::printf("cells missed or repeated: %d, checksum %.17g\n", bad, sum);
  return bad != 0;
}
#endif
