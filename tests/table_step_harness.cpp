// TEST-ONLY: the division by the photo tables' step and the table position built on it, compiled with the host C++
// compiler (tests/test_table_step_division_host.py).  Nothing in the product links this file.
//   g++ -O2 -ffp-contract=off -mfma -fPIC -shared -o _table_step_harness.so table_step_harness.cpp
#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_device.hpp"

using namespace c2r;

extern "C" {
// {dlogtau, rdlogtau_hi, rdlogtau_lo, minlogtau, NTAU} as the header has them
void ts_constants(double *out) {
  out[0] = dlogtau;
  out[1] = rdlogtau_hi;
  out[2] = rdlogtau_lo;
  out[3] = minlogtau;
  out[4] = (double)NTAU;
}
// quo[i] = div_by_table_step(num[i])
void ts_divide(int n, const double *num, double *quo) {
  for (int i = 0; i < n; i++) quo[i] = div_by_table_step(num[i]);
}
// the position of lt[i]: row and residual
void ts_position(int n, const double *lt, int *ipos, double *residual) {
  for (int i = 0; i < n; i++) {
    const TauPos p = table_position_of_log(lt[i]);
    ipos[i] = p.ipos;
    residual[i] = p.residual;
  }
}
}
