// TEST-ONLY: the escape maps' attribution rule, face-cell index and fixed-order sum (c2-ray3dm1d_helium_amd/csrc/c2ray_face.hpp)
// compiled with the host C++ compiler and run exhaustively, so that tests/test_face_loss_host.py can hold the code
// k_face_loss runs per lane to the rule of include/c2ray_hip.h before it reaches a GPU.  Nothing in the product links this file.
//   g++ -O2 -ffp-contract=off -mfma -fPIC -shared -std=c++17 -o _face_harness.so face_harness.cpp
// With -DFACE_HARNESS_MAIN it is a program of its own that runs the same sweep (for a run under -fsanitize=address,undefined).
#include <cstddef>
#include <cstdio>
#include <vector>

#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_face.hpp"
#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_shell.hpp"

using namespace c2r;

namespace {

// The rule of include/c2ray_hip.h once more, as a list of candidates in (axis, low before high) order that is searched for
// the largest weight with a strict comparison: written apart from face_of_cell, to be compared with it.
int rule(const int n[3], const int open[3], const int m[3], const int o[3], const double dr[3], int *ncand, int cand[6]) {
  *ncand = 0;
  for (int d = 0; d < 3; d++) {
    if (!open[d]) continue;
    if (m[d] + 1 == 1) cand[(*ncand)++] = 2 * d;
    if (m[d] + 1 == n[d]) cand[(*ncand)++] = 2 * d + 1;
  }
  int pick = -1;
  double best = 0.0;
  for (int c = 0; c < *ncand; c++) {
    const int d = cand[c] >> 1;
    const double w = (double)(o[d] < 0 ? -o[d] : o[d]) * dr[d];
    if (pick < 0 || w > best) { pick = cand[c]; best = w; }
  }
  return pick;
}

} // namespace

extern "C" {

// counts[0] cell.source pairs looked at; [1] pairs with a candidate; [2] pairs at a mesh edge or corner (several candidates);
// [3] pairs decided by a tie rule.  bad[0] a cell with candidates got no face or several; [1] the face is no candidate;
// [2] a cell without candidate got a face; [3] the face differs from the rule's; [4] face cell index / decode / offsets are
// no bijection onto the map; [5] an offset is not the one axis_offset gives back.
int fh_sweep(int nmax, const double *dr, long long counts[4], long long bad[6]) {
  for (int k = 0; k < 4; k++) counts[k] = 0;
  for (int k = 0; k < 6; k++) bad[k] = 0;
  const double drv[3] = {dr[0], dr[1], dr[2]};
  for (int n1 = 1; n1 <= nmax; n1++)
    for (int n2 = 1; n2 <= nmax; n2++)
      for (int n3 = 1; n3 <= nmax; n3++)
        for (int mask = 1; mask < 8; mask++) {
          const int n[3] = {n1, n2, n3};
          const int open[3] = {mask & 1, (mask >> 1) & 1, (mask >> 2) & 1};
          // the maps: every open face's cells, decoded and indexed back, fill [0, total) exactly once
          const int total = face_map_offset(n, open, 6);
          std::vector<int> seen((size_t)total, 0);
          for (int face = 0; face < 6; face++) {
            if (!open[face >> 1]) continue;
            const int off = face_map_offset(n, open, face), cells = face_cells(n, face >> 1);
            if (off < 0 || off + cells > total) { bad[4]++; continue; }
            for (int f = 0; f < cells; f++) {
              int m[3];
              face_cell_decode(n, face, f, m);
              const int on = (face & 1) ? n[face >> 1] - 1 : 0;
              bool ok = m[face >> 1] == on;
              for (int d = 0; d < 3; d++) ok = ok && m[d] >= 0 && m[d] < n[d];
              if (!ok || face_cell_index(n, face >> 1, m) != f) bad[4]++;
              seen[(size_t)(off + f)]++;
            }
          }
          for (int v : seen)
            if (v != 1) bad[4]++;
          // every source position and every cell of its reach
          int l[3], r[3], w[3];
          for (int s1 = 1; s1 <= n1; s1++)
            for (int s2 = 1; s2 <= n2; s2++)
              for (int s3 = 1; s3 <= n3; s3++) {
                const int pos[3] = {s1, s2, s3};
                for (int d = 0; d < 3; d++) {
                  axis_reach(n[d], pos[d], !open[d], 1 << 20, l[d], r[d]);
                  w[d] = axis_wrap_extent(n[d], !open[d]);
                }
                for (int o1 = l[0]; o1 <= r[0]; o1++)
                  for (int o2 = l[1]; o2 <= r[1]; o2++)
                    for (int o3 = l[2]; o3 <= r[2]; o3++) {
                      const int o[3] = {o1, o2, o3};
                      int m[3];
                      for (int d = 0; d < 3; d++) {
                        m[d] = axis_mesh_index(pos[d], o[d], w[d]);
                        if (axis_offset(m[d], pos[d], w[d]) != o[d]) bad[5]++; // (what k_face_loss forms from the face cell)
                      }
                      counts[0]++;
                      int ncand, cand[6];
                      const int want = rule(n, open, m, o, drv, &ncand, cand);
                      const int got = face_of_cell(n, open, m, o, drv);
                      if (ncand == 0) {
                        if (got != -1) bad[2]++;
                        continue;
                      }
                      counts[1]++;
                      if (ncand > 1) counts[2]++;
                      // exactly one face: of the six faces only `got` claims the cell (the kernel's test is got == face)
                      int claims = 0;
                      bool is_cand = false;
                      for (int face = 0; face < 6; face++) claims += got == face ? 1 : 0;
                      for (int c = 0; c < ncand; c++) is_cand = is_cand || cand[c] == got;
                      if (claims != 1) bad[0]++;
                      if (!is_cand) bad[1]++;
                      if (got != want) bad[3]++;
                      // the tie rules, spelt out: no candidate has a larger weight; of those with the same weight none
                      // has a lower axis, nor the same axis and the low side
                      if (got >= 0) {
                        const double wg = (double)(o[got >> 1] < 0 ? -o[got >> 1] : o[got >> 1]) * drv[got >> 1];
                        bool tie = false;
                        for (int c = 0; c < ncand; c++) {
                          const int d = cand[c] >> 1;
                          const double wc = (double)(o[d] < 0 ? -o[d] : o[d]) * drv[d];
                          if (wc > wg) bad[3]++;
                          if (cand[c] != got && wc == wg) {
                            tie = true;
                            if (cand[c] < got) bad[3]++;
                          }
                        }
                        if (tie) counts[3]++;
                      }
                    }
              }
        }
  long long nbad = 0;
  for (int k = 0; k < 6; k++) nbad += bad[k];
  return nbad == 0 ? 0 : 1;
}

int fh_face_of_cell(const int *n, const int *open, const int *m, const int *o, const double *dr) {
  const int n_[3] = {n[0], n[1], n[2]}, open_[3] = {open[0], open[1], open[2]}, m_[3] = {m[0], m[1], m[2]}, o_[3] = {o[0], o[1], o[2]};
  const double dr_[3] = {dr[0], dr[1], dr[2]};
  return face_of_cell(n_, open_, m_, o_, dr_);
}

int fh_face_cell_index(const int *n, int axis, const int *m) {
  const int n_[3] = {n[0], n[1], n[2]}, m_[3] = {m[0], m[1], m[2]};
  return face_cell_index(n_, axis, m_);
}

int fh_face_map_offset(const int *n, const int *open, int face) {
  const int n_[3] = {n[0], n[1], n[2]}, open_[3] = {open[0], open[1], open[2]};
  return face_map_offset(n_, open_, face);
}

double fh_face_sum(const double *map, long long count) { return face_sum(map, (size_t)count); }
}

#ifdef FACE_HARNESS_MAIN
int main() {
  const double dr[3] = {1.0, 1.25, 0.75};
  long long counts[4], bad[6];
  const int rc = fh_sweep(6, dr, counts, bad);
  std::vector<double> v(1000);
  for (size_t i = 0; i < v.size(); i++) v[i] = 1.0 / (double)(i + 1);
  double s = 0.0;
  for (size_t cnt : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)1000}) s += fh_face_sum(v.data(), (long long)cnt);
  std::printf("pairs %lld with candidates %lld edges %lld ties %lld bad %lld %lld %lld %lld %lld %lld sums %.17g\n", counts[0], counts[1],
              counts[2], counts[3], bad[0], bad[1], bad[2], bad[3], bad[4], bad[5], s);
  return rc;
}
#endif
