// Host build of csrc/c2ray_rim.hpp for tests/test_horizon_loss_host.py: the rule k_horizon_rim runs per lane, over every
// sheet column of a box.   g++ -O2 -ffp-contract=off -fPIC -shared
// With -DRIM_HARNESS_MAIN it is a program of its own that walks a few boxes (for a run under a host sanitizer).
#include <cmath>
#include <cstdio>
#include <vector>

#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_rim.hpp"

extern "C" {

long long rh_total(const int *lo, const int *hi) {
  return c2r::rim_total(c2r::rim_extent(lo[0], hi[0]), c2r::rim_extent(lo[1], hi[1]), c2r::rim_extent(lo[2], hi[2]));
}

// Every sheet column t = 0 .. T-1 of the box lo..hi of a source with a finite horizon `radius` and a beam of `kind`
// (0: none): kstar[t], face[t], w[t], the column's cell in cell[3 t ..] and its (fc, oa, ob) in col[3 t ..].
// Returns the number of columns whose rim_index is not t (0 if the decode and its inverse agree).
int rh_columns(int kind, const double *axis, double cos_half, double radius, const double *dr, const int *lo_, const int *hi_,
               int *kstar, unsigned char *face, double *w, int *cell, int *col) {
  const int lo[3] = {lo_[0], lo_[1], lo_[2]}, hi[3] = {hi_[0], hi_[1], hi_[2]};
  const double K = kind == c2r::BEAM_NONE ? 0.0 : c2r::beam_K(cos_half, axis[0], axis[1], axis[2]);
  const int cut = kind | c2r::CUT_HORIZON;
  const double R2 = c2r::horizon_R2(radius);
  const long long T = rh_total(lo, hi);
  int bad = 0;
  for (long long t = 0; t < T; t++) {
    int fc, oa, ob;
    if (!c2r::rim_decode(lo, hi, t, fc, oa, ob)) { bad++; continue; }
    if (c2r::rim_index(lo, hi, fc, oa, ob) != t) bad++;
    int k, o0, o1, o2;
    double wt;
    const bool f = c2r::rim_column(cut, axis[0], axis[1], axis[2], K, R2, dr[0], dr[1], dr[2], lo, hi, fc, oa, ob, k, o0, o1, o2, wt);
    kstar[t] = k;
    face[t] = f ? 1 : 0;
    w[t] = wt;
    cell[3 * t] = o0; cell[3 * t + 1] = o1; cell[3 * t + 2] = o2;
    col[3 * t] = fc; col[3 * t + 1] = oa; col[3 * t + 2] = ob;
  }
  int fc, oa, ob;
  if (c2r::rim_decode(lo, hi, T, fc, oa, ob) || c2r::rim_decode(lo, hi, -1, fc, oa, ob)) bad++;
  return bad;
}

double rh_face_sum(const double *v, long long n) { return c2r::face_sum(v, (size_t)n); }
}

#ifdef RIM_HARNESS_MAIN
int main() {
  const double axis[3] = {1.0, 2.0, -1.0};
  const double drs[2][3] = {{1.0, 1.0, 1.0}, {1.0, 1.3, 0.7}};
  const int boxes[3][6] = {{-12, -12, -12, 12, 12, 12}, {-2, -9, -4, 9, 3, 12}, {0, 0, 0, 0, 0, 0}};
  const double radii[] = {0.0, 0.5, 1.0, 2.3, 3.0, 5.0, 7.7, 1e200};
  for (const auto &dr : drs)
    for (const auto &b : boxes)
      for (double r : radii)
        for (int kind = 0; kind < 3; kind++) {
          const long long T = rh_total(b, b + 3);
          std::vector<int> ks((size_t)T), cell((size_t)3 * T), col((size_t)3 * T);
          std::vector<unsigned char> face((size_t)T);
          std::vector<double> w((size_t)T);
          const int bad = rh_columns(kind, axis, 0.5, r, dr, b, b + 3, ks.data(), face.data(), w.data(), cell.data(), col.data());
          if (bad) { std::printf("decode mismatch: %d\n", bad); return 1; }
          std::printf("dr %g %g %g box %d..%d radius %g kind %d: T %lld sum w %.9f\n", dr[0], dr[1], dr[2], b[0], b[3], r, kind, T,
                      rh_face_sum(w.data(), T));
        }
  return 0;
}
#endif
