// TEST-ONLY: the reach-cut shell order of c2-ray3dm1d_helium_amd/csrc/c2ray_shell.hpp (open boundaries) compiled with
// the host C++ compiler, and its checks over whole boxes (tests/test_reach_shell_host.py).  Nothing in the product
// links this file.
//   g++ -O2 -ffp-contract=off -mfma -fPIC -shared -std=c++17 -o _reach_shell_harness.so reach_shell_harness.cpp
#include <cstddef>
#include <vector>

#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_device.hpp"
#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_shell.hpp"

using namespace c2r;

namespace {
int box_smax(const int *l, const int *r) {
  int m = 0;
  for (int d = 0; d < 3; d++) {
    if (-l[d] > m) m = -l[d];
    if (r[d] > m) m = r[d];
  }
  return m;
}
int linf(int i, int j, int k) {
  const int a = i < 0 ? -i : i, b = j < 0 ? -j : j, c = k < 0 ? -k : k;
  return a > b ? (a > c ? a : c) : (b > c ? b : c);
}
} // namespace

extern "C" {

long long rs_cells(const int l[3], const int r[3], int s) { return reach_cells(l, r, s); }
long long rs_shell_cells(const int l[3], const int r[3], int s) { return reach_shell(l, r, s).cnt; }
long long rs_position(const int l[3], const int r[3], int di, int dj, int dk) { return (long long)reach_position(l, r, di, dj, dk); }

// The thread map of the box [l, r]: 0 if decode o position is the identity on every cell, every thread of every shell
// decodes to a cell of that shell within the reach, shell s fills [E(s-1), E(s)) and the positions fill
// [0, E(smax)) exactly once; else the number of the first check that failed.
int rs_check_box(const int l[3], const int r[3]) {
  const int smax = box_smax(l, r);
  const long long total = reach_cells(l, r, smax);
  long long cells = 1;
  for (int d = 0; d < 3; d++) cells *= r[d] - l[d] + 1;
  if (total != cells) return 1;
  std::vector<int> seen((size_t)total, 0);
  for (int s = 0; s <= smax; s++) {
    const ReachShell G = reach_shell(l, r, s);
    const long long lo = reach_cells(l, r, s - 1), hi = reach_cells(l, r, s);
    if ((long long)G.off != lo || (long long)G.cnt != hi - lo) return 2;
    for (int t = 0; t < G.cnt; t++) {
      int di, dj, dk;
      const int face = reach_decode(G, t, di, dj, dk);
      if (linf(di, dj, dk) != s) return 3;
      if (di < l[0] || di > r[0] || dj < l[1] || dj > r[1] || dk < l[2] || dk > r[2]) return 4;
      const int ka = dk < 0 ? -dk : dk, ja = dj < 0 ? -dj : dj;
      if (s > 0 && face != (ka == s ? 0 : (ja == s ? 1 : 2))) return 5;
      const long long p = (long long)reach_position(l, r, di, dj, dk);
      if (p != lo + t) return 6;
      if (reach_position_in_shell(G, di, dj, dk) != t) return 7;
      if (seen[(size_t)p]++) return 8;
    }
  }
  for (long long p = 0; p < total; p++)
    if (seen[(size_t)p] != 1) return 9;
  // ... and from the cells' side: every cell of the box has a position in its own shell's range
  for (int dk = l[2]; dk <= r[2]; dk++)
    for (int dj = l[1]; dj <= r[1]; dj++)
      for (int di = l[0]; di <= r[0]; di++) {
        const int s = linf(di, dj, dk);
        const long long p = (long long)reach_position(l, r, di, dj, dk);
        if (p < reach_cells(l, r, s - 1) || p >= reach_cells(l, r, s)) return 10;
        int ei, ej, ek;
        reach_decode(reach_shell(l, r, s), (int)(p - reach_cells(l, r, s - 1)), ei, ej, ek);
        if (ei != di || ej != dj || ek != dk) return 11;
      }
  return 0;
}

// l = -cap, r = cap: the uncut order, entry for entry
int rs_check_uncut(int cap) {
  const int l[3] = {-cap, -cap, -cap}, r[3] = {cap, cap, cap};
  for (int s = 0; s <= cap; s++) {
    if (reach_cells(l, r, s - 1) != shell_offset(s) || reach_shell(l, r, s).cnt != shell_count(s)) return 1;
    const ReachShell G = reach_shell(l, r, s);
    for (int t = 0; t < G.cnt; t++) {
      int di, dj, dk, ei, ej, ek;
      reach_decode(G, t, di, dj, dk);
      shell_decode(s, t, ei, ej, ek);
      if (di != ei || dj != ej || dk != ek) return 2;
    }
  }
  for (int dk = -cap; dk <= cap; dk++)
    for (int dj = -cap; dj <= cap; dj++)
      for (int di = -cap; di <= cap; di++)
        if (reach_position(l, r, di, dj, dk) != shell_position(di, dj, dk)) return 3;
  return 0;
}

// The fast sweep's corners for every cell of the shells >= 2 of the box [l, r], the source at mesh position 1 - l:
// weights and path are the bits of shell_short_characteristic; every corner position is below E(s-1); where the weight
// is non-zero the corner cell of the general short_characteristic lies within the reach and the position is its general
// one (reach_position).  0, or the number of the first check that failed; *checked counts the cells looked at.
int rs_check_corners(const int l[3], const int r[3], long long *checked) {
  const int smax = box_smax(l, r);
  const int i0 = 1 - l[0], j0 = 1 - l[1], k0 = 1 - l[2];
  long long n = 0;
  for (int s = 2; s <= smax; s++) {
    const ShellGeom SG = shell_geometry(s);
    const ReachShell G = reach_shell(l, r, s), Gp = reach_shell(l, r, s - 1);
    const long long below = reach_cells(l, r, s - 1);
    for (int t = 0; t < G.cnt; t++, n++) {
      int di, dj, dk;
      const int face = reach_decode(G, t, di, dj, dk);
      ShellCorners c4, u4;
      reach_short_characteristic(SG, Gp, l, r, face, i0, j0, k0, di, dj, dk, c4);
      shell_short_characteristic(SG, face, i0, j0, k0, di, dj, dk, u4);
      ShortChar s4;
      short_characteristic(i0, j0, k0, di, dj, dk, s4);
      if (c4.path != u4.path) return 1;
      for (int c = 0; c < 4; c++) {
        if (c4.s[c] != u4.s[c] || c4.s[c] != s4.s[c]) return 2;
        if ((long long)c4.p[c] >= below) return 3;
        if (s4.s[c] != 0.0) {
          if (s4.ci[c] < l[0] || s4.ci[c] > r[0] || s4.cj[c] < l[1] || s4.cj[c] > r[1] || s4.ck[c] < l[2] || s4.ck[c] > r[2]) return 4;
          if ((size_t)c4.p[c] != reach_position(l, r, s4.ci[c], s4.cj[c], s4.ck[c])) return 5;
        }
      }
    }
  }
  if (checked) *checked = n;
  return 0;
}

// The HI column of every cell of the open box [l, r] around a source at mesh position 1 - l, swept twice on the host with
// the product's own functions: in mesh order with the general short_characteristic (a corner outside the box counts 0.0,
// its weight is 0), and in the cut shell order as the kernels do it -- shells 0 and 1 through the general path with
// corners clamped into the reach, shells >= 2 through reach_short_characteristic.  u: neufrac * ndens * abundance of the
// cells in mesh order (i fastest).  Returns the number of cells whose outgoing column differs in any bit.
long long rs_check_sweep(const int l[3], const int r[3], const double *u) {
  const int n1 = r[0] - l[0] + 1, n2 = r[1] - l[1] + 1;
  const int i0 = 1 - l[0], j0 = 1 - l[1], k0 = 1 - l[2];
  const int smax = box_smax(l, r);
  const size_t total = (size_t)reach_cells(l, r, smax);
  auto q = [&](int di, int dj, int dk) { return (size_t)(di - l[0]) + (size_t)n1 * ((size_t)(dj - l[1]) + (size_t)n2 * (size_t)(dk - l[2])); };
  auto in_reach = [&](int di, int dj, int dk) { return di >= l[0] && di <= r[0] && dj >= l[1] && dj <= r[1] && dk >= l[2] && dk <= r[2]; };
  std::vector<double> mesh(total, 0.0), cut(total, 0.0);
  for (int s = 0; s <= smax; s++) {
    const ReachShell G = reach_shell(l, r, s);
    const ShellGeom SG = shell_geometry(s);
    for (int t = 0; t < G.cnt; t++) {
      int di, dj, dk;
      const int face = reach_decode(G, t, di, dj, dk);
      double cin_m = 0.0, cin_c = 0.0, path = 0.5;
      if (s > 0) {
        ShortChar s4;
        short_characteristic(i0, j0, k0, di, dj, dk, s4);
        double cm[4], cc[4];
        for (int c = 0; c < 4; c++) {
          cm[c] = in_reach(s4.ci[c], s4.cj[c], s4.ck[c]) ? mesh[q(s4.ci[c], s4.cj[c], s4.ck[c])] : 0.0;
          cc[c] = cut[reach_position(l, r, reach_clamp(s4.ci[c], l[0], r[0]), reach_clamp(s4.cj[c], l[1], r[1]),
                                     reach_clamp(s4.ck[c], l[2], r[2]))];
        }
        cin_m = interp_column(s4, cm[0], cm[1], cm[2], cm[3], sigma_HI_at_ion_freq);
        path = s4.path;
        if (s >= 2) {
          ShellCorners c4;
          reach_short_characteristic(SG, reach_shell(l, r, s - 1), l, r, face, i0, j0, k0, di, dj, dk, c4);
          cin_c = interp_column_fast(c4.s, cut[c4.p[0]], cut[c4.p[1]], cut[c4.p[2]], cut[c4.p[3]], sigma_HI_at_ion_freq);
          if (c4.path != s4.path) return -1;
        } else {
          cin_c = interp_column(s4, cc[0], cc[1], cc[2], cc[3], sigma_HI_at_ion_freq);
        }
      }
      mesh[q(di, dj, dk)] = cin_m + u[q(di, dj, dk)] * path;
      cut[(size_t)G.off + (size_t)t] = cin_c + u[q(di, dj, dk)] * path;
    }
  }
  long long bad = 0;
  for (int dk = l[2]; dk <= r[2]; dk++)
    for (int dj = l[1]; dj <= r[1]; dj++)
      for (int di = l[0]; di <= r[0]; di++) {
        const double a = mesh[q(di, dj, dk)], b = cut[reach_position(l, r, di, dj, dk)];
        if (!(a == b) || !(a > 0.0)) bad++;
      }
  return bad;
}

} // extern "C"
