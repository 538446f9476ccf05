// TEST-ONLY: the table of log10's exponent terms that the isothermal one-SED rates kernel reads where it used to multiply,
// compiled with the host C++ compiler (tests/test_log10_exponent_table_host.py).  Nothing in the product links this file.
//   g++ -O2 -ffp-contract=off -mfma -fPIC -shared -o _host_harness_parked.so host_harness_parked.cpp
#include <cstring>

#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_device.hpp"

using namespace c2r;

namespace {
gm::LogEntry tab4[256];
gm::Log10Exp exptab[gm::LOG10_NEXP];
gm::LogEntryExp both = {tab4, exptab};
bool filled = false;
void fill() {
  if (filled) return;
  for (int E = 0; E < 256; E++) tab4[E] = gm::make_log_entry(E);
  for (int e = 0; e < gm::LOG10_NEXP; e++) exptab[e] = gm::make_log10_exp(gm::LOG10_KY_LO + e); // as the kernel fills it
  filled = true;
}
bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
} // namespace

extern "C" {
// the table's range and its entries, as the kernel fills them: out[2 * e] = ylo, out[2 * e + 1] = yhi of ky = lo + e
int hp_exponent_table(int *lo, int *hi, double *out, int n) {
  fill();
  *lo = gm::LOG10_KY_LO;
  *hi = gm::LOG10_KY_HI;
  for (int e = 0; e < gm::LOG10_NEXP && e < n; e++) {
    out[2 * e] = exptab[e].ylo;
    out[2 * e + 1] = exptab[e].yhi;
  }
  return gm::LOG10_NEXP;
}
// log10 of positive normal arguments >= 2^-68 as the kernel forms it -- split, near-1 or folded table path, the tail
// through the exponent table -- against gm::log10_, and the table positions of tau_table_positions with both table
// types against each other.  Returns the number of mismatches; what[0] = index of the first.
int hp_check_log10_through_table(int n, const double *x, int *what) {
  fill();
  int bad = 0;
  for (int i = 0; i < n; i++) {
    const gm::Log10Arg a = gm::log10_split(x[i]);
    const double lg = gm::log10_near1(a) ? gm::log_near1(gm::log10_arg_value(a)) : gm::log_table_path4(a, tab4);
    const double f = gm::log10_finish(a, lg, exptab), g = gm::log10_(x[i]), h = gm::log10_finish(a, lg);
    bool ok = same(f, g) && same(f, h);
    if (x[i] >= 1.0e-20) { // the kernel's own entry, which clamps below that
      TauPos p0, p1, q0, q1;
      tau_table_positions(x[i], x[i] * 3.0, &tab4[0], p0, p1);
      tau_table_positions(x[i], x[i] * 3.0, &both, q0, q1);
      ok = ok && p0.ipos == q0.ipos && p1.ipos == q1.ipos && same(p0.residual, q0.residual) && same(p1.residual, q1.residual);
    }
    if (!ok && bad++ == 0 && what) what[0] = i;
  }
  return bad;
}
}
