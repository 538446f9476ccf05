// Host build of csrc/c2ray_halo.hpp for tests/test_source_halo_host.py: the classification the halo sweep kernels run per
// lane, over every cell of a box that reaches `pad` cells beyond the mesh.   g++ -O2 -ffp-contract=off -fPIC -shared
#include "../c2-ray3dm1d_helium_amd/csrc/c2ray_halo.hpp"

extern "C" {

int hh_halo_inside() { return c2r::HALO_INSIDE; }
int hh_ghost_index(int pos, int n) { return c2r::halo_ghost_index(pos, n); }

// For the box [-pad, n + pad) per axis, x fastest: cls, array, entry, stride of every cell OUTSIDE the mesh (an in-mesh cell
// gets -2 in cls and is otherwise left alone: the kernels never ask for it), for a source at the 1-based position srcpos.
void hh_classify_box(const int *mesh, const int *srcpos, int pad, int *cls, int *array, long long *entry, long long *stride) {
  const int g0 = c2r::halo_ghost_index(srcpos[0], mesh[0]), g1 = c2r::halo_ghost_index(srcpos[1], mesh[1]),
            g2 = c2r::halo_ghost_index(srcpos[2], mesh[2]);
  size_t at = 0;
  for (int k = -pad; k < mesh[2] + pad; k++)
    for (int j = -pad; j < mesh[1] + pad; j++)
      for (int i = -pad; i < mesh[0] + pad; i++, at++) {
        const bool in_mesh = i >= 0 && i < mesh[0] && j >= 0 && j < mesh[1] && k >= 0 && k < mesh[2];
        if (in_mesh) {
          cls[at] = -2;
          continue;
        }
        int a = -1;
        size_t f = (size_t)-1, F = (size_t)-1;
        cls[at] = c2r::halo_classify(i, j, k, mesh[0], mesh[1], mesh[2], g0, g1, g2, a, f, F);
        array[at] = a;
        entry[at] = (long long)f;
        stride[at] = (long long)F;
      }
}
}
