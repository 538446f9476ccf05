// TEST-ONLY: the per-axis boundary helpers of c2-ray3dm1d_helium_amd/csrc/c2ray_shell.hpp (axis_reach, axis_mesh_index,
// axis_offset) and the reach-cut shell order on mixed reaches, compiled with the host C++ compiler
// (tests/test_axis_shell_host.py).  Nothing in the product links this file.
//   g++ -O2 -ffp-contract=off -mfma -fPIC -shared -std=c++17 -o _axis_shell_harness.so axis_shell_harness.cpp
#include <cstddef>
#include <vector>

#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_device.hpp"
#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_shell.hpp"

using namespace c2r;

extern "C" {

int ax_wrap_extent(int mesh, int periodic) { return axis_wrap_extent(mesh, periodic); }
void ax_reach(int mesh, int pos, int periodic, int max_subbox, int *l, int *r) { axis_reach(mesh, pos, periodic, max_subbox, *l, *r); }
int ax_mesh_index(int pos, int off, int w) { return axis_mesh_index(pos, off, w); }
int ax_offset(int cell, int pos, int w) { return axis_offset(cell, pos, w); }

// A source at `src` (1-based) of the mesh `mesh` with the axes of `periodic` wrapping, reach cut at max_subbox: 0 if
//   * reach_position / reach_decode are inverse to each other on the source's reach and the positions fill
//     [0, prod_d(r_d - l_d + 1)) exactly once,
//   * offset -> mesh index sends the cells of the reach to distinct cells of the mesh, and cell -> offset sends each of
//     them back,
//   * every other cell of the mesh gets an offset outside the reach,
// else the number of the first check that failed.  *reached: how many cells of the mesh the reach holds.
int ax_check_mixed_box(const int mesh[3], const int src[3], const int periodic[3], int max_subbox, long long *reached) {
  int l[3], r[3], w[3];
  for (int d = 0; d < 3; d++) {
    axis_reach(mesh[d], src[d], periodic[d], max_subbox, l[d], r[d]);
    w[d] = axis_wrap_extent(mesh[d], periodic[d]);
    if (l[d] > 0 || r[d] < 0) return 1;
  }
  int smax = 0;
  for (int d = 0; d < 3; d++) {
    if (-l[d] > smax) smax = -l[d];
    if (r[d] > smax) smax = r[d];
  }
  long long cells = 1;
  for (int d = 0; d < 3; d++) cells *= r[d] - l[d] + 1;
  if (reach_cells(l, r, smax) != cells) return 2;
  if (cells > (long long)mesh[0] * mesh[1] * mesh[2]) return 3;
  std::vector<int> seen((size_t)cells, 0);
  std::vector<int> hit((size_t)mesh[0] * mesh[1] * mesh[2], 0);
  for (int s = 0; s <= smax; s++) {
    const ReachShell G = reach_shell(l, r, s);
    if ((long long)G.off != reach_cells(l, r, s - 1) || (long long)G.cnt != reach_cells(l, r, s) - reach_cells(l, r, s - 1)) return 4;
    for (int t = 0; t < G.cnt; t++) {
      int o[3];
      reach_decode(G, t, o[0], o[1], o[2]);
      for (int d = 0; d < 3; d++)
        if (o[d] < l[d] || o[d] > r[d]) return 5;
      const long long p = (long long)reach_position(l, r, o[0], o[1], o[2]);
      if (p != (long long)G.off + t) return 6;
      if (seen[(size_t)p]++) return 7;
      int m[3];
      for (int d = 0; d < 3; d++) {
        m[d] = axis_mesh_index(src[d], o[d], w[d]);
        if (m[d] < 0 || m[d] >= mesh[d]) return 8;
        if (axis_offset(m[d], src[d], w[d]) != o[d]) return 9;
      }
      if (hit[(size_t)m[0] + (size_t)mesh[0] * ((size_t)m[1] + (size_t)mesh[1] * (size_t)m[2])]++) return 10;
    }
  }
  for (long long p = 0; p < cells; p++)
    if (seen[(size_t)p] != 1) return 11;
  // the cells of the mesh the reach does not hold: an offset outside the reach along some axis
  for (int k = 0; k < mesh[2]; k++)
    for (int j = 0; j < mesh[1]; j++)
      for (int i = 0; i < mesh[0]; i++) {
        const int m[3] = {i, j, k};
        bool inside = true;
        for (int d = 0; d < 3; d++) {
          const int o = axis_offset(m[d], src[d], w[d]);
          inside = inside && o >= l[d] && o <= r[d];
        }
        if (inside != (hit[(size_t)i + (size_t)mesh[0] * ((size_t)j + (size_t)mesh[1] * (size_t)k)] == 1)) return 12;
      }
  if (reached) *reached = cells;
  return 0;
}

} // extern "C"
