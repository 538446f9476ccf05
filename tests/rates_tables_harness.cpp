// TEST-ONLY: the index arithmetic of the two tables that the rates kernels read instead of computing -- the pair copy of
// the photo table (TablePair, c2-ray3dm1d_helium_amd/csrc/c2ray_device.hpp) and the shell volumes per offset (ShellVol,
// csrc/c2ray_shell.hpp) -- compiled with the host C++ compiler (tests/test_rates_tables_host.py).  Nothing in the product
// links this file.
//   g++ -O2 -ffp-contract=off -mfma -fPIC -shared -std=c++17 -o _rates_tables_harness.so rates_tables_harness.cpp
#include <cstddef>
#include <cstdint>

#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_device.hpp"
#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_shell.hpp"

using namespace c2r;

extern "C" {

int rt_ntau(void) { return NTAU; }
int rt_pitch(void) { return (int)TABLE_PAIR_PITCH; }
int rt_pair_size(void) { return (int)sizeof(TablePair); }
int rt_pair_align(void) { return (int)alignof(TablePair); }
long long rt_pair_index(int b, int r) { return (long long)table_pair_index(b, r); }

// what load_rows and interpolate_rows make of a column of pairs built from `col` (NTAUP rows) the way k_table_pairs builds
// it, at position (ipos, residual); *byte_offset: where load_rows reads, in bytes from the column's first pair
double rt_read_pairs(const double *col, int ipos, double residual, long long *byte_offset) {
  static TablePair pairs[NTAUP];
  for (int r = 0; r < NTAUP; r++) {
    pairs[r].c = col[r];
    pairs[r].d = r + 1 < NTAUP ? col[r + 1] - col[r] : 0.0;
  }
  TauPos p;
  p.ipos = ipos;
  p.residual = residual;
  const TableRows rows = load_rows(pairs, p);
  *byte_offset = (long long)((unsigned)ipos << 4);
  return interpolate_rows(rows, p);
}
// ... and what read_table makes of the column itself
double rt_read_table(const double *col, int ipos, double residual) {
  TauPos p;
  p.ipos = ipos;
  p.residual = residual;
  return read_table(col, p);
}

int rt_shell_extent(int n, int l) { return shell_vol_extent(n, l); }
long long rt_shell_index(int ia, int ja, int ka, int e1, int e2) { return (long long)shell_vol_index(ia, ja, ka, e1, e2); }
int rt_shell_size(void) { return (int)sizeof(ShellVol); }

} // extern "C"
