// TEST-ONLY: the near-1 test of the folded log route by the limit of the argument's own table entry (gm::LogFold::lim),
// compiled with the host C++ compiler (tests/test_log_near1_limit_host.py).  Nothing in the product links this file.
//   g++ -O2 -ffp-contract=off -mfma -fPIC -shared -o _log_near1_limit_harness.so log_near1_limit_harness.cpp
#include <cmath>
#include <cstring>

#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_device.hpp"

using namespace c2r;

namespace {
gm::LogFold tabf[256];
gm::Log10Exp exptab[gm::LOG10_NEXP];
const gm::FoldPins fold = gm::pin_fold_constants();
bool filled = false;
void fill() {
  if (filled) return;
  for (int E = 0; E < 256; E++) tabf[E] = gm::make_log_fold(E); // as the kernel fills it
  for (int e = 0; e < gm::LOG10_NEXP; e++) exptab[e] = gm::make_log10_exp(gm::LOG10_KY_LO + e);
  filled = true;
}
bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
// the test this one replaces, written out
bool window(uint32_t hx) { return hx - 0x3FEE0000u < 0x00030900u; }
} // namespace

extern "C" {
int nl_sizeof_entry() { return (int)sizeof(gm::LogFold); }
// lim[E], pad[E] of the 256 entries
int nl_limits(uint32_t *lim, uint32_t *pad) {
  fill();
  for (int E = 0; E < 256; E++) {
    lim[E] = tabf[E].lim;
    pad[E] = tabf[E].pad;
  }
  return 256;
}
// hx in [0x3FE00000, 0x40000000), what a split yields: the new test, with the limit of hx's own entry, against the old one.
// Returns the number of mismatches; *first = index of the first.
int nl_check_hx(int n, const uint32_t *hx, int *first) {
  fill();
  int bad = 0;
  *first = -1;
  for (int i = 0; i < n; i++) {
    gm::Log10ArgFold a;
    a.hx = hx[i];
    a.lo = 0;
    a.xoff = 0;
    const uint32_t E = (hx[i] - 0x3FE00000u) >> 13;
    if (E >= 256u || gm::log10_near1(a, tabf[E].lim) != window(hx[i]) || gm::log10_near1(a) != window(hx[i])) {
      if (bad++ == 0) *first = i;
    }
  }
  return bad;
}
// Positive normal finite arguments, through log10_split_fold.  Per argument:
//   bad[0]  the limit that log_table_path_fold hands back is the limit of hx's entry, and the value it returns is the one
//           it returns without being asked for the limit
//   bad[1]  the new near-1 test against hx - 0x3FEE0000u < 0x00030900u
//   bad[2]  log10 through the folded route, its path chosen by the new test, against gm::log10_
//   bad[3]  tau_table_positions with the folded pair type (which chooses the new test) against the position of gm::log10_'s
//           value (arguments >= 1e-20)
int nl_check(int n, const double *x, int *bad, int *first) {
  fill();
  const gm::LogFoldExp route = {tabf, exptab - gm::LOG10_KY_LO, &fold};
  for (int c = 0; c < 4; c++) { bad[c] = 0; first[c] = -1; }
  auto miss = [&](int c, int i) { if (bad[c]++ == 0) first[c] = i; };
  for (int i = 0; i < n; i++) {
    const gm::Log10ArgFold f = gm::log10_split_fold(x[i], &fold);
    uint32_t lim = 0xDEADBEEFu;
    const double v = gm::log_table_path_fold(f, tabf, nullptr, &lim);
    if (lim != tabf[((f.hx - 0x3FE00000u) >> 13) & 255u].lim || !same(v, gm::log_table_path_fold(f, tabf))) miss(0, i);
    const bool near1 = gm::log10_near1(f, lim);
    if (near1 != window(f.hx)) miss(1, i);
    const double lg = near1 ? gm::log_near1(gm::log10_arg_value(f)) : v;
    if (!same(gm::log10_finish(f, lg, route.exp0), gm::log10_(x[i]))) miss(2, i);
    if (x[i] >= 1.0e-20) {
      TauPos p0, p1;
      const double y = x[i] * 3.0;
      tau_table_positions(x[i], y, &route, p0, p1);
      const TauPos q0 = table_position_of_log(gm::log10_(x[i])), q1 = table_position_of_log(gm::log10_(y));
      if (!(p0.ipos == q0.ipos && same(p0.residual, q0.residual) && p1.ipos == q1.ipos && same(p1.residual, q1.residual))) miss(3, i);
    }
  }
  int total = 0;
  for (int c = 0; c < 4; c++) total += bad[c];
  return total;
}
}
