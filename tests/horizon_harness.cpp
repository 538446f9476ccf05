// Host build of csrc/c2ray_horizon.hpp for tests/test_source_horizons_host.py: the predicates the kernels run per lane, over
// every offset of a cube around the source.   g++ -O2 -ffp-contract=off -fPIC -shared
#include <cmath>

#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_horizon.hpp"

extern "C" {

double hh_horizon_R2(double radius) { return c2r::horizon_R2(radius); }

// within[(dk + half) * w * w + (dj + half) * w + (di + half)], w = 2 * half + 1, for every offset with |d| <= half
void hh_within_cube(double radius, const double *dr, int half, unsigned char *within) {
  const double R2 = c2r::horizon_R2(radius);
  const int w = 2 * half + 1;
  for (int dk = -half; dk <= half; dk++)
    for (int dj = -half; dj <= half; dj++)
      for (int di = -half; di <= half; di++)
        within[((dk + half) * w + (dj + half)) * w + (di + half)] = c2r::horizon_within(R2, dr[0], dr[1], dr[2], di, dj, dk) ? 1 : 0;
}

// the same cube through cut_lit, the one function the kernels call: beam kind (0: none) and a horizon where radius is finite,
// as the host fills a source's record; a source with neither is lit everywhere without asking
void hh_cut_cube(int kind, const double *axis, double cos_half, double radius, const double *dr, int half, unsigned char *lit) {
  const double K = kind == c2r::BEAM_NONE ? 0.0 : c2r::beam_K(cos_half, axis[0], axis[1], axis[2]);
  const int cut = kind | (std::isfinite(radius) ? c2r::CUT_HORIZON : 0);
  const double R2 = c2r::horizon_R2(radius);
  const int w = 2 * half + 1;
  for (int dk = -half; dk <= half; dk++)
    for (int dj = -half; dj <= half; dj++)
      for (int di = -half; di <= half; di++)
        lit[((dk + half) * w + (dj + half)) * w + (di + half)] =
            cut == c2r::CUT_NONE || c2r::cut_lit(cut, axis[0], axis[1], axis[2], K, R2, dr[0], dr[1], dr[2], di, dj, dk) ? 1 : 0;
}
}
