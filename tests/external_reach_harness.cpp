// Host build of what c2r_set_sources_external adds to csrc/c2ray_shell.hpp, for tests/test_external_reach_host.py:
//   g++ -O2 -ffp-contract=off -mfma -fPIC -shared -std=c++17 -o tests/_external_reach_harness.so tests/external_reach_harness.cpp
#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_shell.hpp"

using namespace c2r;

extern "C" {

void xr_axis_reach(int mesh, int pos, int periodic, int max_subbox, int *lr) { axis_reach(mesh, pos, periodic, max_subbox, lr[0], lr[1]); }

void xr_axis_reach_external(int mesh, int pos, int periodic, int max_subbox, int *lr) {
  axis_reach_external(mesh, pos, periodic, max_subbox, lr[0], lr[1]);
}

// the sweep's predicate for the cell at offset `off` from a source at `pos`: the wrap of mesh0<true>, then the compare
int xr_in_mesh(int mesh, int pos, int off, int periodic) {
  return axis_in_mesh(axis_mesh_index(pos, off, axis_wrap_extent(mesh, periodic)), mesh) ? 1 : 0;
}

int xr_refusal(const int *l, const int *r) { return external_reach_refusal(l, r); }

long long xr_reach_cells(const int *l, const int *r, int s) { return reach_cells(l, r, s); }

// thread t of the cut shell s -> (di, dj, dk, face); returns the cells of the shell
int xr_reach_decode(const int *l, const int *r, int s, int t, int *out) {
  const ReachShell G = reach_shell(l, r, s);
  if (t >= 0 && t < G.cnt) out[3] = reach_decode(G, t, out[0], out[1], out[2]);
  return G.cnt;
}

long long xr_reach_position(const int *l, const int *r, int di, int dj, int dk) { return (long long)reach_position(l, r, di, dj, dk); }

}
