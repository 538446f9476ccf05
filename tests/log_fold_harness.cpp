// TEST-ONLY: the folded log table and the one-subtraction split of the isothermal one-SED rates kernel, compiled with the
// host C++ compiler (tests/test_log_folded_entry_host.py).  Nothing in the product links this file.
//   g++ -O2 -ffp-contract=off -mfma -fPIC -shared -o _log_fold_harness.so log_fold_harness.cpp
#include <cmath>
#include <cstring>

#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_device.hpp"

using namespace c2r;

namespace {
gm::LogEntry tab4[256];
gm::LogFold tabf[256];
gm::Log10Exp exptab[gm::LOG10_NEXP];
const gm::FoldPins fold = gm::pin_fold_constants();
const gm::LogFoldExp with_pins = {tabf, exptab - gm::LOG10_KY_LO, &fold}, without_pins = {tabf, exptab - gm::LOG10_KY_LO, nullptr};
const gm::LogEntryExp parent = {tab4, exptab};
bool filled = false;
void fill() {
  if (filled) return;
  for (int E = 0; E < 256; E++) { // as the kernels fill them
    tab4[E] = gm::make_log_entry(E);
    tabf[E] = gm::make_log_fold(E);
  }
  for (int e = 0; e < gm::LOG10_NEXP; e++) exptab[e] = gm::make_log10_exp(gm::LOG10_KY_LO + e);
  filled = true;
}
bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
bool same(const TauPos &a, const TauPos &b) { return a.ipos == b.ipos && same(a.residual, b.residual); }
} // namespace

extern "C" {
// the 256 entries of both tables: fold[4 * E] = {invc', w, c, pad as a number}, entry[4 * E] = {invc, w, c, k}
int lf_tables(double *fold_out, double *entry_out) {
  fill();
  static_assert(sizeof(gm::LogFold) == sizeof(gm::LogEntry) && sizeof(gm::LogFold) == 32, "the pitch stays");
  for (int E = 0; E < 256; E++) {
    fold_out[4 * E] = tabf[E].invc;
    fold_out[4 * E + 1] = tabf[E].w;
    fold_out[4 * E + 2] = tabf[E].c;
    fold_out[4 * E + 3] = (double)tabf[E].pad;
    entry_out[4 * E] = tab4[E].invc;
    entry_out[4 * E + 1] = tab4[E].w;
    entry_out[4 * E + 2] = tab4[E].c;
    entry_out[4 * E + 3] = (double)((int32_t)tab4[E].kshift >> 20);
  }
  return 256;
}
// Positive normal arguments >= 2^-68 (+inf included).  Per argument, bit for bit:
//   bad[0]  the new split against log10_split: hx, lo, offset == ky << 4 (with the select's constants handed down and without)
//   bad[1]  the new table path against log_table_path4 (every argument, whichever path the log takes for it)
//   bad[2]  log10 through the whole new route against gm::log10_ (finite arguments)
//   bad[3]  ... against the platform's log10 (finite arguments)
//   bad[4]  ... against the route it replaces (LogEntry, Log10Exp; every argument, +inf too)
//   bad[5]  tau_table_positions with the new pair type against the LogEntryExp one (+inf too) and, where finite, against the
//           position of gm::log10_'s value (arguments >= 1e-20, the kernel's own entry)
// first[c] = index of the first mismatch of class c.  Returns the total.
int lf_check(int n, const double *x, int *bad, int *first) {
  fill();
  for (int c = 0; c < 6; c++) { bad[c] = 0; first[c] = -1; }
  auto miss = [&](int c, int i) { if (bad[c]++ == 0) first[c] = i; };
  for (int i = 0; i < n; i++) {
    const gm::Log10Arg a = gm::log10_split(x[i]);
    const gm::Log10ArgFold f = gm::log10_split_fold(x[i], &fold), g = gm::log10_split_fold(x[i]);
    if (!(f.hx == a.hx && f.lo == a.lo && f.xoff == a.ky * 16 && g.hx == a.hx && g.lo == a.lo && g.xoff == f.xoff &&
          gm::log10_near1(f) == gm::log10_near1(a) && same(gm::log10_arg_value(f), gm::log10_arg_value(a))))
      miss(0, i);
    const double u = gm::log_table_path4(a, tab4), v = gm::log_table_path_fold(f, tabf);
    if (!same(u, v)) miss(1, i);
    const double lg = gm::log10_near1(f) ? gm::log_near1(gm::log10_arg_value(f)) : v;
    const double lgp = gm::log10_near1(a) ? gm::log_near1(gm::log10_arg_value(a)) : u;
    const double r = gm::log10_finish(f, lg, with_pins.exp0);
    if (std::isfinite(x[i])) {
      if (!same(r, gm::log10_(x[i]))) miss(2, i);
      if (!same(r, log10(x[i]))) miss(3, i);
    }
    if (!same(r, gm::log10_finish(a, lgp, exptab))) miss(4, i);
    if (x[i] >= 1.0e-20) {
      TauPos p0, p1, q0, q1, s0, s1;
      const double y = x[i] * 3.0;
      tau_table_positions(x[i], y, &parent, p0, p1);
      tau_table_positions(x[i], y, &with_pins, q0, q1);
      tau_table_positions(x[i], y, &without_pins, s0, s1);
      bool ok = same(p0, q0) && same(p1, q1) && same(q0, s0) && same(q1, s1);
      if (std::isfinite(x[i])) ok = ok && same(q0, table_position_of_log(gm::log10_(x[i])));
      if (std::isfinite(y)) ok = ok && same(q1, table_position_of_log(gm::log10_(y)));
      if (!ok) miss(5, i);
    }
  }
  int total = 0;
  for (int c = 0; c < 6; c++) total += bad[c];
  return total;
}
}
