// Host build of csrc/c2ray_beam.hpp for tests/test_source_beams_host.py: the predicate the kernels run per lane, over every
// offset of a cube around the source.   g++ -O2 -ffp-contract=off -fPIC -shared
#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_beam.hpp"

extern "C" {

double bh_beam_K(double cos_half, const double *axis) { return c2r::beam_K(cos_half, axis[0], axis[1], axis[2]); }

// lit[(dk + half) * w * w + (dj + half) * w + (di + half)], w = 2 * half + 1, for every offset with |d| <= half
void bh_lit_cube(int kind, const double *axis, double cos_half, const double *dr, int half, unsigned char *lit) {
  const double K = c2r::beam_K(cos_half, axis[0], axis[1], axis[2]);
  const int w = 2 * half + 1;
  for (int dk = -half; dk <= half; dk++)
    for (int dj = -half; dj <= half; dj++)
      for (int di = -half; di <= half; di++)
        lit[((dk + half) * w + (dj + half)) * w + (di + half)] =
            c2r::beam_lit(kind, axis[0], axis[1], axis[2], K, dr[0], dr[1], dr[2], di, dj, dk) ? 1 : 0;
}
}
