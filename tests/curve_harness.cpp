// Host build of csrc/c2ray_curve.hpp for tests/test_source_curves_host.py: the functions the kernels run per lane, over every
// offset of a cube around the source.   g++ -O2 -ffp-contract=off -fPIC -shared
#include <cmath>

#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_curve.hpp"

extern "C" {

double ch_curve_R2(double radius) { return c2r::curve_R2(radius); }

// f[(dk + half) * w * w + (dj + half) * w + (di + half)], w = 2 * half + 1, for every offset with |d| <= half: the factor of the
// curve alone, from the tables as the host fills a source's record
void ch_factor_cube(int nstep, const double *radius, const double *factor, const double *dr, int half, double *f) {
  double R2[c2r::CURVE_MAX_STEPS], fac[c2r::CURVE_MAX_STEPS + 1];
  c2r::curve_fill(nstep, radius, factor, R2, fac);
  const int w = 2 * half + 1;
  for (int dk = -half; dk <= half; dk++)
    for (int dj = -half; dj <= half; dj++)
      for (int di = -half; di <= half; di++)
        f[((dk + half) * w + (dj + half)) * w + (di + half)] = c2r::curve_factor_at(R2, fac, dr[0], dr[1], dr[2], di, dj, dk);
}

// the same cube through cut_flux, the one function the kernels call for a curved source: beam kind (0: none), a horizon where
// hradius is finite and the curve; lit[] and, where lit, f[] (0.0 where unlit)
void ch_cut_cube(int kind, const double *axis, double cos_half, double hradius, int nstep, const double *radius, const double *factor,
                 const double *dr, int half, unsigned char *lit, double *f) {
  const double K = kind == c2r::BEAM_NONE ? 0.0 : c2r::beam_K(cos_half, axis[0], axis[1], axis[2]);
  const int cut = kind | (std::isfinite(hradius) ? c2r::CUT_HORIZON : 0) | c2r::CUT_CURVE;
  const double hR2 = c2r::horizon_R2(hradius);
  double R2[c2r::CURVE_MAX_STEPS], fac[c2r::CURVE_MAX_STEPS + 1];
  c2r::curve_fill(nstep, radius, factor, R2, fac);
  const int w = 2 * half + 1;
  for (int dk = -half; dk <= half; dk++)
    for (int dj = -half; dj <= half; dj++)
      for (int di = -half; di <= half; di++) {
        const int at = ((dk + half) * w + (dj + half)) * w + (di + half);
        double ff = -1.0;
        const bool l = c2r::cut_flux(cut, axis[0], axis[1], axis[2], K, hR2, R2, fac, dr[0], dr[1], dr[2], di, dj, dk, ff);
        lit[at] = l ? 1 : 0;
        f[at] = l ? ff : 0.0;
      }
}
}
