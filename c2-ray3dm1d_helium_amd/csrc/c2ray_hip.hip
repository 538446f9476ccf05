// MI355X (gfx950) implementation of C2-Ray's evolve3D hot path behind the C ABI of
// include/c2ray_hip.h.  See DESIGN.md for the data layout and the kernel list.
//
//   column sweep   k_sweep_shell   one launch per L-infinity shell around the sources of a batch:
//                                  short-characteristics interpolation of the three incoming
//                                  columns (cinterp) + the cell's own columns (evolve0D, first half);
//                                  k_sweep_shell_ext, k_sweep_shell_fast_ext for a batch with a source outside the mesh
//                                  (c2r_set_sources_external): cells of its box beyond the mesh are vacuum;
//                                  k_sweep_shell_entry, k_sweep_shell_fast_entry for a batch with a source that has entry
//                                  columns (c2r_set_source_face_entry): the ghost layer of its face holds the strip of the
//                                  mesh upstream; k_sweep_shell_halo, k_sweep_shell_fast_halo for a batch with a source whose
//                                  halo has several faces (c2r_set_source_halo): ghost layers, edge lines and the corner
//                                  (c2ray_halo.hpp); k_source_face_exit gathers the exit strips (c2ray_handover.inc)
//   rates          k_rates         all cells x all sources of the batch, no dependencies:
//                                  photoion_rates + accumulation into the rate grids in source order
//                                  (evolve0D, second half)
//   boundary loss  k_loss_probe_rounds  a lower bound of the photon loss through a sub-box surface from a sample of the
//                                  stored columns (decides "this source goes on" for several rounds in one launch);
//                  k_loss, k_loss_finish   the full, block-ordered sum where the bound does not decide or the loss is kept;
//                  k_loss_stored   the kept loss of a final round, left behind by k_rates in the unused N_in(HI) slots
//   chemistry      k_chemistry     evolve0D_global / do_chemistry / doric / thermal per cell
//   statistics     k_state_sums, k_total_rates, k_stat_finish   the grid sums of photonstatistics.f90
//   tables         k_build_tables  spec_integration: the photo-ionisation / heating tables of one SED
//   plane sources  k_plane_columns, k_plane_layer, k_plane_rates, k_plane_exit   a plane wave entering through an open mesh
//                                  face (c2ray_planes.inc): the march along the axis, its rates, what leaves through the far face
//                                  (and, k_pside_loss, through the open side faces of a tilted plane)
//   escape maps    k_face_loss     the kept loss of an open box per cell of the mesh face it leaves through
//                                  (c2r_enable_face_loss): a gather, one lane per face cell, the sources in source order
//   horizon loss   k_horizon_rim   what crosses the photon horizon of each source that has one (c2r_enable_horizon_loss): one
//                                  lane per column of the six sheets around the source, k_loss_finish adds the block sums
//
// Compile: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/c2ray_hip.h"
#include "c2ray_device.hpp"
#include "c2ray_beam.hpp"
#include "c2ray_horizon.hpp"
#include "c2ray_curve.hpp"
#include "c2ray_face.hpp"
#include "c2ray_rim.hpp"
#include "c2ray_plane.hpp"
#include "c2ray_pcurve.hpp"
#include "c2ray_pside.hpp"
#include "c2ray_shell.hpp"
#include "c2ray_halo.hpp"

using namespace c2r;

namespace {

constexpr int BATCH_MAX = 4096; // sources in flight per batch (device-resident records, no kernel-argument limit)
constexpr int BLOCK = 256;

struct Grid {
  int n1, n2, n3;
  int l1, l2, l3; // left extent mesh/2 (evolve_source.F90:105)
  size_t ncell;
  size_t colsize; // entries of one shell-ordered column array that holds the whole mesh: (2*smax+1)^3
  int smax;       // largest L-infinity shell index, max(l1,l2,l3)
};

// One source of the batch in flight, in device memory (read through the scalar cache: uniform per block).
struct SrcDev {
  int i0, j0, k0;      // 1-based mesh position (srcpos); < 1 or > mesh along an open axis for a source that stands outside the
                       // mesh (c2r_set_sources_external): an ordinary operand of short_characteristic, vol_ph and the path
  int lo[3], hi[3];    // FINAL sub-box as offsets last_l - srcpos, last_r - srcpos (set before the rates launch)
  double nflux;        // NormFlux(ns)
  double nflux_sed[2]; // NormFluxPL(ns), NormFluxQPL(ns) (-DPL / -DQUASARS builds), else 0
  double *cols;        // this source's column block in the scratch arena
  size_t cz;           // entries per column array of that block, cap = shells it can hold: (2*cap+1)^3, or with open
                       // boundaries the cells of those shells within the source's reach (reach_cells, c2ray_shell.hpp)
  int loss_lo;         // >= 0: the rates launch leaves, for every surface cell of the final sub-box in shells >= loss_lo,
                       // the photons that leave the box through it in the cell's N_in(HI) slot (k_loss_stored adds
                       // them up); -1: no such request (set before the rates launch)
  int rl[3], rr[3];    // open and mixed boundaries only: the source's reach per axis (axis_reach, c2ray_shell.hpp: the else
                       // branch of evolve_source.F90:103-109 on an open axis, the then-branch on a periodic one); the
                       // all-periodic kernels never read them
  int wn[3];           // likewise: the wrap extent of each axis (axis_wrap_extent: the mesh extent if the axis is periodic
                       // while another is open, 0 if it is open)
  int cut;             // what cuts the source's light short (c2ray_horizon.hpp): its beam's kind (c2r_set_source_beams;
                       // c2ray_beam.hpp: BEAM_NONE, BEAM_CONE or BEAM_BICONE) | CUT_HORIZON where it has a finite horizon
                       // (c2r_set_source_horizons); CUT_NONE: neither ...
  double bax, bay, baz; // ... the beam's axis as given ...
  double bK;           // ... beam_K, cos^2 of the half opening angle times the axis's squared length (0 without a beam) ...
  double hR2;          // ... and horizon_R2, the squared radius of the horizon (+infinity without one)
  // cut & CUT_CURVE: the source has a light curve (c2r_set_source_curves; c2ray_curve.hpp), else the tables are never read:
  double cR2[CURVE_MAX_STEPS];      // curve_fill: the squared radii of its steps, +infinity behind the last
  double cfac[CURVE_MAX_STEPS + 1]; // ... and the factor of each shell
};
// Entry columns of one source of the batch in flight (c2r_set_source_face_entry), a record beside its SrcDev that only the
// kernels of a batch with such a source are given (k_sweep_shell_entry, k_sweep_shell_fast_entry, k_loss_entry).
struct SrcEntry {
  int on;             // 0: the source has no entry; else 1 + face, face = 2 * axis + high
  const double *cols; // its strip: 3 F doubles, species slowest, the face cells with the lower of the two other axes fastest
  int origin[3];      // c2r_set_mesh_origin: the deep mesh's index of this mesh's cell (1,1,1), minus 1, per axis
  // Read by the halo kernels only (c2r_set_source_halo; k_sweep_shell_halo, k_sweep_shell_fast_halo), filled for every source with
  // an entry -- one face is the halo of one face:
  int ghost[3];                     // per axis the 0-based ghost index (-1 or mesh), HALO_INSIDE where the source stands inside
  const double *part[HALO_ARRAYS];  // the face strips by axis, the edge lines by axis (3 + axis), the corner; null: none
};
// The source's position as cinterp sees it: cinterp forms its crossing points from absolute coordinates, so a part of a deep mesh
// reproduces the deep mesh's bits only with the deep mesh's coordinates -- the source's own, moved by the mesh's origin
// (c2r_set_mesh_origin; a context with an origin runs every batch through the kernels that are given these records).  Nothing
// else reads these three numbers: cells, offsets and blocks stay this mesh's.
__device__ __forceinline__ void entry_cinterp_position(const SrcEntry &E, int &i0, int &j0, int &k0) {
  i0 += E.origin[0];
  j0 += E.origin[1];
  k0 += E.origin[2];
}
// The column that a box cell OUTSIDE the mesh of a source with an entry stores as N_out: the strip's, if the cell lies in
// the ghost layer of the entry's face (one step outside it), else `vacuum`, its N_in.  (i, j, k): the cell's 0-based mesh
// index; the source stands beyond that face only, so the cell's two other coordinates lie in the mesh.
__device__ __forceinline__ void entry_columns(const SrcEntry &E, const Grid &g, int i, int j, int k, double &c_HI, double &c_HeI,
                                              double &c_HeII) {
  // (selects on values, as in shell_decode_fast: arrays indexed by the axis would go to scratch memory)
  const int face = E.on - 1, axis = face >> 1, high = face & 1;
  const int xc = axis == 0 ? i : (axis == 1 ? j : k), nc = axis == 0 ? g.n1 : (axis == 1 ? g.n2 : g.n3);
  if (xc != (high ? nc : -1)) return;
  const int xa = axis == 0 ? j : i, xb = axis == 2 ? j : k;   // the two other axes, the lower one first
  const int na = axis == 0 ? g.n2 : g.n1, nb = axis == 2 ? g.n2 : g.n3;
  const size_t F = (size_t)na * (size_t)nb, f = (size_t)xa + (size_t)na * (size_t)xb;
  c_HI = E.cols[f];
  c_HeI = E.cols[F + f];
  c_HeII = E.cols[2 * F + f];
}
// The same for a source with a halo (c2r_set_source_halo): the cell's class, array and entry from halo_classify
// (c2ray_halo.hpp), the array's address by selects on the record's seven pointers (uniform per source), three loads for a
// ghost cell and none for a vacuum cell.
__device__ __forceinline__ void halo_columns(const SrcEntry &E, const Grid &g, int i, int j, int k, double &c_HI, double &c_HeI,
                                             double &c_HeII) {
  int array;
  size_t f, F;
  if (!halo_classify(i, j, k, g.n1, g.n2, g.n3, E.ghost[0], E.ghost[1], E.ghost[2], array, f, F)) return;
  const double *face = array == 0 ? E.part[0] : (array == 1 ? E.part[1] : E.part[2]);
  const double *edge = array == 3 ? E.part[3] : (array == 4 ? E.part[4] : E.part[5]);
  const double *cols = array < 3 ? face : (array < 6 ? edge : E.part[6]);
  c_HI = cols[f];
  c_HeI = cols[F + f];
  c_HeII = cols[2 * F + f];
}
// Is the cell at offset (di, dj, dk) lit by source S?  Uniform branch on S.cut (a scalar register: the record is read through
// the scalar cache), so a source with neither beam nor horizon costs a wave one scalar compare; the loss and per-cell kernels
// ask this beside their in-box test.  (k_rates never asks: batches with such a source run k_rates_beam or k_rates_curve.)
// They go on to use the source's fluxes, so the answer comes with f: the factor of the cell's shell where the source has a
// curve (c2ray_curve.hpp; a shell with f == 0.0 is unlit), 1.0 where it has none -- one more uniform branch.
__device__ __forceinline__ bool source_flux(const SrcDev &S, double dr1, double dr2, double dr3, int di, int dj, int dk, double &f) {
  f = 1.0;
  if (S.cut == CUT_NONE) return true;
  if (!(S.cut & CUT_CURVE)) return cut_lit(S.cut, S.bax, S.bay, S.baz, S.bK, S.hR2, dr1, dr2, dr3, di, dj, dk);
  return cut_flux(S.cut, S.bax, S.bay, S.baz, S.bK, S.hR2, S.cR2, S.cfac, dr1, dr2, dr3, di, dj, dk, f);
}
// NormFlux, NormFluxPL or NormFluxQPL of the source as a cell in a shell of factor f sees it: one rounded product where the
// source has a curve (uniform), the flux itself where it has none
__device__ __forceinline__ double curve_scaled(const SrcDev &S, double nflux, double f) {
  return (S.cut & CUT_CURVE) ? nflux * f : nflux;
}
// the sub-box of the round in flight: the same for every active source of a batch (all are in the same round)
struct Box {
  int lo[3], hi[3];
};
// Open (non-periodic) boundaries: nothing wraps, so a source's sub-box is the round's box cut at the source's own reach,
// and it differs from source to source within a round.  OPEN is a template parameter of every kernel that looks at a
// box: the periodic instantiations are the code they were before the open ones existed.
// Mixed boundaries (c2r_set_boundaries_axes: some axes periodic, the others open) run on the OPEN instantiations: a
// periodic axis there is an axis whose reach is the mesh's and whose mesh index wraps by SrcDev::wn, a value that is
// uniform over a block and 0 on an open axis, where the wrap is then the identity (axis_wrap, c2ray_shell.hpp).
__device__ __forceinline__ Box source_box(const Box &box, const SrcDev &S) {
  Box b;
  for (int d = 0; d < 3; d++) {
    b.lo[d] = box.lo[d] > S.rl[d] ? box.lo[d] : S.rl[d];
    b.hi[d] = box.hi[d] < S.rr[d] ? box.hi[d] : S.rr[d];
  }
  return b;
}

struct StepScalars {
  double dr1, dr2, dr3, vol;
  double cellvol;       // dr1 * dr2 * dr3 (vol_ph of a source's own cell, evolve_point.F90:203), formed on the host: a product of
                        // uniform numbers has no scalar instruction, and hoisted out of k_rates' source loop it costs two vector registers
  double clumping;
  double temper_val;
  RecCoef rc;
  CoolData cd;
  int use_lls;          // c2ray_parameters: use_LLS
  double coldensh_lls;  // material: coldensh_LLS (type_of_LLS = 1)
};

// 0-based periodic index of x in [-n, 2n) (axis_wrap, c2ray_shell.hpp)
__device__ __forceinline__ int wrap0(int x, int n) { return axis_wrap(x, n); }

// 0-based mesh index of the cell at offset x from the origin: periodic, or (open and mixed boundaries: a cell of a source's
// box lies in the mesh along an open axis) wrapped by the axis's wrap extent w, which is 0 on an open axis
template <bool OPEN>
__device__ __forceinline__ int mesh0(int x, int n, int w) { return OPEN ? axis_wrap(x, w) : wrap0(x, n); }

// Does a surface cell of the sub-box `b` count?  Periodic boundaries, and the loss that is KEPT (photon_loss) in open
// ones: every cell with a coordinate on a face.  The loss that DECIDES whether an open box grows once more (movable_only):
// only cells on a face still short of the source's reach -- photons that leave through a mesh face are lost whatever the
// box does and must not make a source next to an edge sweep the whole mesh.  This replaces the while-test of
// evolve_source.F90:136-139, which looks at z only and is wrong without periodicity.
template <bool OPEN>
__device__ __forceinline__ bool on_counted_face(const Box &b, const SrcDev &S, int di, int dj, int dk, int movable_only) {
  if (OPEN && movable_only)
    return (di == b.lo[0] && b.lo[0] > S.rl[0]) || (dj == b.lo[1] && b.lo[1] > S.rl[1]) || (dk == b.lo[2] && b.lo[2] > S.rl[2]) ||
           (di == b.hi[0] && b.hi[0] < S.rr[0]) || (dj == b.hi[1] && b.hi[1] < S.rr[1]) || (dk == b.hi[2] && b.hi[2] < S.rr[2]);
  return di == b.lo[0] || dj == b.lo[1] || dk == b.lo[2] || di == b.hi[0] || dj == b.hi[1] || dk == b.hi[2];
}

__device__ __forceinline__ double block_sum(double x, double *sh) {
  // fixed-shape tree: wave shuffle, then the 4 wave sums in order -> deterministic
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) sh[w] = x;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0) {
    for (int i = 0; i < BLOCK / 64; i++) r += sh[i];
  }
  return r; // valid in thread 0
}

// path length of cinterp for an offset, without the corner work (column_density.f90:194,269,341)
__device__ __forceinline__ double sc_path(int idel, int jdel, int kdel) {
  const int ia = idel < 0 ? -idel : idel, ja = jdel < 0 ? -jdel : jdel, ka = kdel < 0 ? -kdel : kdel;
  const double di = (double)idel, dj = (double)jdel, dk = (double)kdel;
  if (ka >= ja && ka >= ia) return sqrt((di * di + dj * dj) / (dk * dk) + 1.0);
  if (ja >= ia && ja >= ka) return sqrt((di * di + dk * dk) / (dj * dj) + 1.0);
  return sqrt(1.0 + (dj * dj + dk * dk) / (di * di));
}

// What the rates kernels read instead of computing it per cell and source, made on the device from inputs that change
// seldom (the photo table: per table set; the cell sizes: per time step):
//   pairs     the black-body photo_thick table as (value, forward difference) pairs (TablePair, c2ray_device.hpp) for the
//             gathers-first readers: the isothermal one-SED k_rates, k_rates_beam and k_rates_curve;
//   shellvol  vol_ph and its reciprocal per (|di|, |dj|, |dk|) (ShellVol, c2ray_shell.hpp), extents e1 x e2 x ..., for the
//             all-periodic one-SED k_rates; `big`: every entry satisfies Recip::ok_big.  Where one does not, every lane takes
//             div_by_vol's plain divisions, which give the bits that Markstein's sequence gives where it is allowed.
struct RatesTables {
  const TablePair *pairs;
  const ShellVol *shellvol;
  int e1, e2, big;
};
// pairs[b][r] = {c[r], c[r + 1] - c[r]}: the subtraction of read_table, once per entry; row NumTau gets c[2001] - c[2000],
// +0 by the duplicated row, and row 2001, which no position reaches, a difference of 0 as well
__global__ void __launch_bounds__(BLOCK)
k_table_pairs(const double *__restrict__ tab, TablePair *__restrict__ pairs) {
  const int r = blockIdx.x * BLOCK + threadIdx.x, b = blockIdx.y;
  if (r >= NTAUP) return;
  const double *col = tab + (size_t)b * NTAUP;
  TablePair p;
  p.c = col[r];
  p.d = r + 1 < NTAUP ? col[r + 1] - col[r] : 0.0;
  pairs[table_pair_index(b, r)] = p;
}
// shellvol[|di|, |dj|, |dk|]: the expressions of the rates body and of make_recip, once per offset; *not_big is raised where
// an entry fails Recip::ok_big (one atomic per wave that has such an entry)
__global__ void __launch_bounds__(BLOCK)
k_shell_volumes(double dr1, double dr2, double dr3, double cellvol, int e1, int e2, int e3, ShellVol *__restrict__ tab,
                int *__restrict__ not_big) {
  const size_t q = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (q >= (size_t)e1 * e2 * e3) return;
  const int di = (int)(q % e1), dj = (int)((q / e1) % e2), dk = (int)(q / ((size_t)e1 * e2));
  double vol_ph;
  if (di == 0 && dj == 0 && dk == 0) {
    vol_ph = cellvol;
  } else {
    const double path = sc_path(di, dj, dk) * dr1;
    const double xs = dr1 * (double)di, ys = dr2 * (double)dj, zs = dr3 * (double)dk;
    const double dist2 = xs * xs + ys * ys + zs * zs;
    vol_ph = 4.0 * pi * dist2 * path;
  }
  const Recip R = make_recip(vol_ph);
  ShellVol v;
  v.vol = R.b;
  v.rvol = R.y;
  tab[shell_vol_index(di, dj, dk, e1, e2)] = v;
  const bool bad = !R.ok_big;
  const unsigned long long m = __ballot(bad);
  if (bad && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicOr(not_big, 1);
}

// A pointer that comes out of a record in memory (SrcDev::cols) is a generic pointer to the compiler, which then uses
// flat loads and stores; the column blocks are device memory.
typedef __attribute__((address_space(1))) double global_double;

// Where the six columns of the cell at shell position p live in a source's block of 6 cz doubles: the three incoming
// columns of a cell side by side (24 bytes), then all outgoing ones likewise.  The rates kernel, whose 4 x 4 x 4 cubes
// read rows of four cells, then uses 96 of every 128 bytes it touches instead of 32 (-0.3..0.5 ms per launch at
// 256^3 x 8); the sweep's stores become three strided ones per triple (+0.05..0.1 ms per pass).
__host__ __device__ inline size_t col_in(size_t p, int k, size_t) { return 3 * p + (size_t)k; }
__host__ __device__ inline size_t col_out(size_t p, int k, size_t cz) { return 3 * cz + 3 * p + (size_t)k; }

// The sweep's stores of a cell's six columns.  The incoming columns, which only the rates launch reads, long after, are
// stored non-temporally: they then do not sit dirty in the L2s until the end of the launch, when every XCD writes its
// cache back before the next shell may start (a launch per shell: up to 32 MB each time).  The outgoing ones, which the
// next shells interpolate from, are stored plainly.  Measured at 256^3 x 8, same box, ms per pass (sweep | rates), with
// plain stores / incoming ones non-temporal / all six non-temporal: isothermal 3.98-4.03 | 18.5, 3.82 | 18.5,
// 3.78-3.83 | 18.4; with heating 3.86 | 27.9, 3.63 | 28.0-28.1, 3.69 | 28.3 -- the rates launch reads non-temporally
// written columns a little slower, so only the incoming ones are stored that way.
// (Non-temporal LOADS of the columns in the rates kernel: +0.4 ms per launch, neighbouring cubes share their lines.)
__device__ __forceinline__ void store_columns(global_double *cs, size_t p, size_t cz, double cin_HI, double cin_HeI, double cin_HeII,
                                              double cout_HI, double cout_HeI, double cout_HeII) {
  __builtin_nontemporal_store(cin_HI, &cs[col_in(p, 0, cz)]);
  __builtin_nontemporal_store(cin_HeI, &cs[col_in(p, 1, cz)]);
  __builtin_nontemporal_store(cin_HeII, &cs[col_in(p, 2, cz)]);
  cs[col_out(p, 0, cz)] = cout_HI;
  cs[col_out(p, 1, cz)] = cout_HeI;
  cs[col_out(p, 2, cz)] = cout_HeII;
}

// ---------------------------------------------------------------------------------------------
// What the sweep needs of a cell's state, once per pass instead of once per cell.source: the three products
// neufrac * ndens of coldens (doric.f90:358-372: neufrac*ndens*path*abundance is evaluated from the left, so the
// first product does not depend on the source) for HI, HeI, HeII with the fractions clamped at epsilon
// (evolve_point.F90:132-136) -- 24 bytes per cell.source instead of 32 --, in mesh order (`packed`, index
// i + n1*(j + n2*k)) and, for the i-faces of a shell (fixed i, consecutive j), in (j,i,k) order (`packedT`, index
// j + n2*(i + n1*k)); three arrays of ncell each.  32x32 tiles of a k-plane through LDS.
__global__ void __launch_bounds__(BLOCK)
k_pack_state(Grid g, const double *__restrict__ ndens, const double *__restrict__ xh_av, const double *__restrict__ xhe_av,
             double *__restrict__ packed, double *__restrict__ packedT) {
  __shared__ double tile[3][32][33];
  const size_t nc = g.ncell;
  const int k = blockIdx.z;
  const size_t plane = (size_t)k * g.n1 * g.n2;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5; // 32 x 8
  const int i0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
  for (int r = ty; r < 32; r += 8) {
    const int i = i0 + tx, j = j0 + r;
    if (i < g.n1 && j < g.n2) {
      const size_t q = plane + (size_t)i + (size_t)g.n1 * j;
      const double nd = ndens[q];
      const double u0 = dmax(xh_av[q], epsilon) * nd, u1 = dmax(xhe_av[q], epsilon) * nd, u2 = dmax(xhe_av[q + nc], epsilon) * nd;
      packed[q] = u0; packed[q + nc] = u1; packed[q + 2 * nc] = u2;
      tile[0][r][tx] = u0; tile[1][r][tx] = u1; tile[2][r][tx] = u2;
    }
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int j = j0 + tx, i = i0 + r;
    if (i < g.n1 && j < g.n2) {
      const size_t qT = plane + (size_t)j + (size_t)g.n2 * i;
      packedT[qT] = tile[0][tx][r]; packedT[qT + nc] = tile[1][tx][r]; packedT[qT + 2 * nc] = tile[2][tx][r];
    }
  }
}

// packed -> packedT alone, when the global pass has left `packed` up to date (k_chemistry writes it with the
// fractions it stores): 24 bytes read and written per cell instead of 32 and 48
__global__ void __launch_bounds__(BLOCK)
k_transpose_packed(Grid g, const double *__restrict__ packed, double *__restrict__ packedT) {
  __shared__ double tile[32][33];
  const int a = blockIdx.z / g.n3, k = blockIdx.z % g.n3;
  const double *src = packed + (size_t)a * g.ncell + (size_t)k * g.n1 * g.n2;
  double *dst = packedT + (size_t)a * g.ncell + (size_t)k * g.n1 * g.n2;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5; // 32 x 8
  const int i0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
  for (int r = ty; r < 32; r += 8) {
    const int i = i0 + tx, j = j0 + r;
    if (i < g.n1 && j < g.n2) tile[r][tx] = src[(size_t)i + (size_t)g.n1 * j];
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int j = j0 + tx, i = i0 + r;
    if (i < g.n1 && j < g.n2) dst[(size_t)j + (size_t)g.n2 * i] = tile[tx][r];
  }
}

// ---------------------------------------------------------------------------------------------
// The photon loss through the surface of the current sub-box (evolve_point.F90:310-315) from the columns the
// sweep has stored, for all shells [s_lo, s_hi] of the round in ONE launch.  A block takes 256 consecutive cells
// of one shell (the sweep's own thread <-> cell map); its partial sum goes to partial[source][block number
// within the round], and k_loss_finish adds the partials in that order: the same bits on every run and for
// every batch composition.
// `sample` > 1: only every sample-th block is evaluated (blockIdx.x counts those).  Every term is >= 0, so this
// is a lower bound: enough to show that the loss of a round that cannot be a source's last for geometric
// reasons exceeds the threshold of evolve_source.F90:136.  Anything a sample does not decide is redone with
// sample = 1, and only such full sums are ever kept.
// (Inside k_sweep_shell this work sat in a sixteenth of the waves, all of them on two of the eight XCDs: the
// last shell of every round took twice as long as its neighbours.  Here every lane of every wave has a cell.)
// OPEN: `box` is the round's box before it is cut at each source's reach; MOVABLE: the sum that decides (on_counted_face).
// ENTRY (k_loss_entry, a batch with a source that has entry columns, c2r_set_source_face_entry): of such a source only the
// surface cells that are mesh cells count -- what its vacuum surface "loses" is the upstream mesh's business.
template <bool OPEN, bool MOVABLE, bool ENTRY>
__device__ __forceinline__ void loss_block(const Grid &g, const SrcDev *__restrict__ src, const int *__restrict__ list, int multi, int s_lo,
                                           int s_hi, const Box &box_, const StepScalars &sc, const BandData *__restrict__ bd,
                                           const SedSet &ss, const int *__restrict__ block_base, double *__restrict__ loss_partial,
                                           int pitch, int sample, int first_block, const SrcEntry *__restrict__ ent) {
  // first_block: the blocks before it hold no surface cell (the host has set their partials to zero and does not
  // launch them); block numbers, and with them the order of the sum, stay what they are
  __shared__ double sh[BLOCK / 64];
  const SrcDev &S = src[list[blockIdx.y]];
  Box cut_;
  if constexpr (OPEN) cut_ = source_box(box_, S);
  const Box &box = OPEN ? cut_ : box_; // (periodic: the launch's box itself)
  const int bx = first_block + (int)blockIdx.x;
  const int B = block_base[s_lo] + bx * sample;
  int lo = s_lo, hi = s_hi; // largest shell with block_base[shell] <= B
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (block_base[mid] <= B) lo = mid; else hi = mid - 1;
  }
  const int shell = lo;
  ReachShell RS{}; // (open boundaries: the shell cut at the source's reach; its blocks are the first of the uncut shell's)
  if constexpr (OPEN) RS = reach_shell(S.rl, S.rr, shell);
  const long long cnt = OPEN ? (long long)RS.cnt : shell_count(shell);
  const long long t = (long long)(B - block_base[shell]) * BLOCK + threadIdx.x;
  double loss = 0.0;
  if (t < cnt) {
    int di, dj, dk;
    if constexpr (OPEN) reach_decode(RS, (int)t, di, dj, dk);
    else shell_decode(shell, (int)t, di, dj, dk);
    const bool inside = di >= box.lo[0] && di <= box.hi[0] && dj >= box.lo[1] && dj <= box.hi[1] && dk >= box.lo[2] &&
                        dk <= box.hi[2];
    bool boundary = on_counted_face<OPEN>(box, S, di, dj, dk, MOVABLE ? 1 : 0);
    if constexpr (ENTRY) {
      if (ent[list[blockIdx.y]].on) // (uniform per block)
        boundary = boundary && axis_in_mesh(mesh0<OPEN>(S.i0 - 1 + di, g.n1, S.wn[0]), g.n1) &&
                   axis_in_mesh(mesh0<OPEN>(S.j0 - 1 + dj, g.n2, S.wn[1]), g.n2) && axis_in_mesh(mesh0<OPEN>(S.k0 - 1 + dk, g.n3, S.wn[2]), g.n3);
    }
    // (an unlit cell of a beamed source loses nothing: its term is 0.0, as beyond max_coldensh)
    // (likewise a cell in a shell of factor 0 of a curved source; any other shell scales the source's fluxes)
    double cf;
    if (inside && boundary && source_flux(S, sc.dr1, sc.dr2, sc.dr3, di, dj, dk, cf)) {
      const size_t cz = S.cz;
      const size_t p = (OPEN ? (size_t)RS.off : (size_t)shell_offset(shell)) + (size_t)t;
      const global_double *cs = (const global_double *)S.cols;
      const double cin_HI = cs[col_in(p, 0, cz)], cin_HeI = cs[col_in(p, 1, cz)], cin_HeII = cs[col_in(p, 2, cz)];
      const double cout_HI = cs[col_out(p, 0, cz)], cout_HeI = cs[col_out(p, 1, cz)], cout_HeII = cs[col_out(p, 2, cz)];
      if (cin_HI < max_coldensh) {
        double vol_ph;
        if (shell == 0) {
          vol_ph = sc.dr1 * sc.dr2 * sc.dr3;
        } else {
          const double path = sc_path(di, dj, dk) * sc.dr1;
          const double xs = sc.dr1 * (double)di, ys = sc.dr2 * (double)dj, zs = sc.dr3 * (double)dk;
          const double dist2 = xs * xs + ys * ys + zs * zs;
          vol_ph = 4.0 * pi * dist2 * path;
        }
        double po;
        if (multi) {
          const double nf[NSED] = {curve_scaled(S, S.nflux, cf), curve_scaled(S, S.nflux_sed[0], cf), curve_scaled(S, S.nflux_sed[1], cf)};
          po = photo_out_multi(*bd, ss, cin_HI, cout_HI, cin_HeI, cout_HeI, cin_HeII, cout_HeII, nf);
        } else {
          po = photo_out_only(*bd, ss.photo_thick[0], ss.photo_thin[0], cin_HI, cout_HI, cin_HeI, cout_HeI, cin_HeII,
                              cout_HeII, curve_scaled(S, S.nflux, cf));
        }
        loss = po * sc.vol / vol_ph;
      }
    }
  }
  const double bs = block_sum(loss, sh);
  if (threadIdx.x == 0) loss_partial[(size_t)blockIdx.y * pitch + bx] = bs;
}
template <bool OPEN, bool MOVABLE>
__global__ void __launch_bounds__(BLOCK)
k_loss(Grid g, const SrcDev *__restrict__ src, const int *__restrict__ list, int multi, int s_lo, int s_hi, Box box_,
       StepScalars sc, const BandData *__restrict__ bd, SedSet ss,
       const int *__restrict__ block_base, double *__restrict__ loss_partial, int pitch, int sample, int first_block) {
  loss_block<OPEN, MOVABLE, false>(g, src, list, multi, s_lo, s_hi, box_, sc, bd, ss, block_base, loss_partial, pitch, sample, first_block,
                                   nullptr);
}
// the kept loss of a batch that holds a source with entry columns (ent: one record per source of the batch, beside src)
__global__ void __launch_bounds__(BLOCK)
k_loss_entry(Grid g, const SrcDev *__restrict__ src, const int *__restrict__ list, int multi, int s_lo, int s_hi, Box box_,
             StepScalars sc, const BandData *__restrict__ bd, SedSet ss,
             const int *__restrict__ block_base, double *__restrict__ loss_partial, int pitch, int sample, int first_block,
             const SrcEntry *__restrict__ ent) {
  loss_block<true, false, true>(g, src, list, multi, s_lo, s_hi, box_, sc, bd, ss, block_base, loss_partial, pitch, sample, first_block, ent);
}

// ---------------------------------------------------------------------------------------------
// The same sum from values the rates kernel has left behind.  The loss that is KEPT for a source whose last round
// ended for geometric reasons (the box cannot grow any further, evolve_source.F90:136-139) decides nothing, and
// its terms -- photo_out * vol / vol_ph of the surface cells, evolve_point.F90:310-315 -- are quantities k_rates
// computes anyway for every cell.source (the reference takes them from the same photoion_rates call, phi%photo_out).
// So k_rates stores them (SrcDev::loss_lo) in the cell's N_in(HI) slot of the column block, which nobody reads
// after it, and this kernel adds them up with k_loss's thread <-> cell map, block partials and block order: the
// same bits as k_loss gives, without evaluating a single band a second time.
// (OPEN: the kept loss of an open box runs over its whole surface, mesh faces included, and over all its shells.)
template <bool OPEN>
__global__ void __launch_bounds__(BLOCK)
k_loss_stored(Grid g, const SrcDev *__restrict__ src, const int *__restrict__ list, int s_lo, int s_hi, Box box_,
              const int *__restrict__ block_base, double *__restrict__ loss_partial, int pitch, int first_block) {
  __shared__ double sh[BLOCK / 64];
  const SrcDev &S = src[list[blockIdx.y]];
  Box cut_;
  if constexpr (OPEN) cut_ = source_box(box_, S);
  const Box &box = OPEN ? cut_ : box_; // (periodic: the launch's box itself)
  const int bx = first_block + (int)blockIdx.x;
  const int B = block_base[s_lo] + bx;
  int lo = s_lo, hi = s_hi; // largest shell with block_base[shell] <= B
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (block_base[mid] <= B) lo = mid; else hi = mid - 1;
  }
  const int shell = lo;
  ReachShell RS{}; // (open boundaries: the shell cut at the source's reach; its blocks are the first of the uncut shell's)
  if constexpr (OPEN) RS = reach_shell(S.rl, S.rr, shell);
  const long long cnt = OPEN ? (long long)RS.cnt : shell_count(shell);
  const long long t = (long long)(B - block_base[shell]) * BLOCK + threadIdx.x;
  double loss = 0.0;
  if (t < cnt) {
    int di, dj, dk;
    if constexpr (OPEN) reach_decode(RS, (int)t, di, dj, dk);
    else shell_decode(shell, (int)t, di, dj, dk);
    const bool inside = di >= box.lo[0] && di <= box.hi[0] && dj >= box.lo[1] && dj <= box.hi[1] && dk >= box.lo[2] &&
                        dk <= box.hi[2];
    const bool boundary = on_counted_face<OPEN>(box, S, di, dj, dk, 0);
    if (inside && boundary) {
      const size_t p = (OPEN ? (size_t)RS.off : (size_t)shell_offset(shell)) + (size_t)t;
      loss = ((const global_double *)S.cols)[col_in(p, 0, S.cz)];
    }
  }
  const double bs = block_sum(loss, sh);
  if (threadIdx.x == 0) loss_partial[(size_t)blockIdx.y * pitch + bx] = bs;
}


// ---------------------------------------------------------------------------------------------
// Column sweep of one shell for every active source of the batch (blockIdx.y counts `active`).
// evolve0D, files_for_3D/evolve_point.F90:114-168 and :237-244, with cinterp (column_density.f90:28-345).
// A source's column block in the arena: 6 cz doubles = N_in(HI,HeI,HeII) of every cell, then N_out(HI,HeI,HeII)
// (col_in / col_out), the cells in SHELL ORDER (shell_position of the cell's offset from its source): thread t of
// shell s owns entry shell_offset(s)+t, so the stores of a wave cover one contiguous range and -- because the
// corners of consecutive cells are consecutive cells of the previous shell on every face, the i-faces included --
// so do the corner loads.  (In mesh order the i-faces of a shell are one cell per 128-byte line.)
#ifndef C2R_SWEEP_WAVES
#define C2R_SWEEP_WAVES 1
#endif
// what every cell of a sweep launch is given
struct SweepArgs {
  Grid g;
  Box box;
  StepScalars sc;
  const double *ndens, *xh_av, *xhe_av;
  const double *packed, *packedT; // neufrac * ndens of the three species in mesh and in (j,i,k) order (k_pack_state,
                                  // k_chemistry, k_transpose_packed); null while they are being made
  const float *lls_grid;
};

// neufrac * ndens of the three species for the cell at mesh position (i,j,k), 0-based (k_pack_state), or from the
// grids while the packed copies of this pass are still being made (the inner shells); iface: the cell lies on an
// i-face of its shell, where consecutive lanes have consecutive j -> the (j,i,k)-ordered copy
__device__ __forceinline__ void sweep_cell_state(const SweepArgs &A, int i, int j, int k, bool iface, double &u_HI, double &u_HeI,
                                                 double &u_HeII) {
  const Grid &g = A.g;
  const size_t nc = g.ncell;
  if (A.packed) {
    const bool tr = iface && A.packedT; // (the inner shells run before the (j,i,k)-ordered copy exists: strided reads)
    const double *P = tr ? A.packedT : A.packed;
    // a mesh has fewer than 2^31 cells (c2r_create): the cell number in 32 bits, one widening for the address
    const unsigned q = tr ? (unsigned)j + (unsigned)g.n2 * ((unsigned)i + (unsigned)g.n1 * (unsigned)k)
                          : (unsigned)i + (unsigned)g.n1 * ((unsigned)j + (unsigned)g.n2 * (unsigned)k);
    u_HI = P[q];
    u_HeI = P[q + nc];
    u_HeII = P[q + 2 * nc];
  } else {
    const size_t q = (size_t)i + (size_t)g.n1 * ((size_t)j + (size_t)g.n2 * (size_t)k);
    const double nd = A.ndens[q];
    u_HI = dmax(A.xh_av[q], epsilon) * nd;
    u_HeI = dmax(A.xhe_av[q], epsilon) * nd;
    u_HeII = dmax(A.xhe_av[q + nc], epsilon) * nd;
  }
}

// evolve0D's column part (files_for_3D/evolve_point.F90:114-168, :237-244) for cell t of shell `shell` around source
// S, any shell: cinterp through the general short_characteristic / shell_position
// OPEN: the round's box cut at the source's reach, no modulo: a shell cell outside the reach does not exist, and the
// upstream cells of a cell in the mesh lie in the mesh (corners of weight exactly 0 may be read from a slot that was
// never written: finite, as everything in the arena).
// EXT (open and mixed boundaries, a batch with a source outside the mesh, c2r_set_sources_external): the box of such a
// source is cut at a reach that runs through vacuum up to the source, so a cell of it may lie outside the mesh along an open
// axis -- a VACUUM cell: neufrac * ndens is exactly 0.0 for the three species and there is no LLS fog, N_out = N_in +
// 0 * path * abundance, and nothing is loaded from the state grids.  A mesh cell gets the arithmetic it always got.
// ENTRY (EXT kernels of a batch with a source that has entry columns, c2r_set_source_face_entry; E: its record): a vacuum cell
// in the ghost layer of the entry's face stores the strip's columns as N_out instead of N_in (entry_columns) -- the one
// change to the vacuum rule; every other vacuum cell stays vacuum, and nobody downstream of the ghost layer reads one.
// HALO (ENTRY kernels of a batch with a source whose halo has several faces, c2r_set_source_halo): the ghost cells are those of
// halo_columns -- the ghost layers of up to three faces, the edge lines and the corner cell where they meet.
template <bool OPEN, bool EXT = false, bool ENTRY = false, bool HALO = false>
__device__ __forceinline__ void sweep_cell(const SweepArgs &A, const SrcDev &S, int shell, int t, const SrcEntry *E = nullptr) {
  static_assert(EXT || !ENTRY, "entry columns belong to a source outside the mesh");
  static_assert(ENTRY || !HALO, "a halo is a kind of entry");
  static_assert(OPEN || !EXT, "a source outside the mesh needs an open axis");
  const Grid &g = A.g;
  const StepScalars &sc = A.sc;
  int di, dj, dk;
  ReachShell RS{}; // (open boundaries: t counts the cells of the shell cut at the source's reach)
  if constexpr (OPEN) {
    RS = reach_shell(S.rl, S.rr, shell);
    reach_decode(RS, t, di, dj, dk);
  } else {
    shell_decode(shell, t, di, dj, dk);
  }
  Box cut_;
  if constexpr (OPEN) cut_ = source_box(A.box, S);
  const Box &box = OPEN ? cut_ : A.box; // (periodic: the launch's box itself)
  const bool inside = di >= box.lo[0] && di <= box.hi[0] && dj >= box.lo[1] && dj <= box.hi[1] && dk >= box.lo[2] &&
                      dk <= box.hi[2];
  if (!inside) return;
  const size_t cz = S.cz;
  const size_t p = (OPEN ? (size_t)RS.off : (size_t)shell_offset(shell)) + (size_t)t;
  global_double *cs = (global_double *)S.cols;
  const int i = mesh0<OPEN>(S.i0 - 1 + di, g.n1, S.wn[0]), j = mesh0<OPEN>(S.j0 - 1 + dj, g.n2, S.wn[1]),
            k = mesh0<OPEN>(S.k0 - 1 + dk, g.n3, S.wn[2]);
  const int w_ = 2 * shell + 1;
  // (EXT: one unsigned compare per axis, after the wrap -- a periodic axis of a mixed run always passes)
  const bool in_mesh = !EXT || (axis_in_mesh(i, g.n1) && axis_in_mesh(j, g.n2) && axis_in_mesh(k, g.n3));
  double u_HI = 0.0, u_HeI = 0.0, u_HeII = 0.0;
  if (in_mesh) sweep_cell_state(A, i, j, k, shell > 0 && t >= (OPEN ? RS.b4 : 2 * w_ * w_ + 2 * (w_ - 2) * w_), u_HI, u_HeI, u_HeII);
  double cin_HI, cin_HeI, cin_HeII, path;
  if (shell == 0) {
    cin_HI = cin_HeI = cin_HeII = 0.0;
    path = 0.5 * sc.dr1;
  } else {
    ShortChar s4;
    int ci0 = S.i0, cj0 = S.j0, ck0 = S.k0;
    if constexpr (ENTRY) entry_cinterp_position(*E, ci0, cj0, ck0);
    short_characteristic(ci0, cj0, ck0, di, dj, dk, s4);
    size_t qc[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      // (open boundaries: a corner beyond the reach has weight exactly 0 -- the nearest cell that exists instead)
      if constexpr (OPEN)
        qc[c] = reach_position(S.rl, S.rr, reach_clamp(s4.ci[c], S.rl[0], S.rr[0]), reach_clamp(s4.cj[c], S.rl[1], S.rr[1]),
                               reach_clamp(s4.ck[c], S.rl[2], S.rr[2]));
      else
        qc[c] = shell_position(s4.ci[c], s4.cj[c], s4.ck[c]);
    }
    cin_HI = interp_column(s4, cs[col_out(qc[0], 0, cz)], cs[col_out(qc[1], 0, cz)], cs[col_out(qc[2], 0, cz)],
                           cs[col_out(qc[3], 0, cz)], sigma_HI_at_ion_freq);
    cin_HeI = interp_column(s4, cs[col_out(qc[0], 1, cz)], cs[col_out(qc[1], 1, cz)], cs[col_out(qc[2], 1, cz)],
                            cs[col_out(qc[3], 1, cz)], sigma_HeI_at_ion_freq);
    cin_HeII = interp_column(s4, cs[col_out(qc[0], 2, cz)], cs[col_out(qc[1], 2, cz)], cs[col_out(qc[2], 2, cz)],
                             cs[col_out(qc[3], 2, cz)], sigma_HeII_at_ion_freq);
    path = s4.path * sc.dr1;
    if (sc.use_lls && in_mesh) {
      // Lyman-limit-system fog on the incoming HI column (evolve_point.F90:177-180); the per-cell
      // grid is LLS_point of type_of_LLS = 2 (REAL(4), mat_ini_cubep3m.F90:859-870)
      const double coldensh_LLS =
          A.lls_grid ? (double)A.lls_grid[(size_t)i + (size_t)g.n1 * ((size_t)j + (size_t)g.n2 * (size_t)k)] : sc.coldensh_lls;
      cin_HI = cin_HI + coldensh_LLS * path / sc.dr1;
    }
  }
  // coldens (doric.f90:358-372): neufrac * ndens * path * abundance, from the left
  double cout_HI = cin_HI + u_HI * path * (1.0 - abu_he);
  double cout_HeI = cin_HeI + u_HeI * path * abu_he;
  double cout_HeII = cin_HeII + u_HeII * path * abu_he;
  if constexpr (ENTRY) {
    if (E->on && !in_mesh) {
      if constexpr (HALO) halo_columns(*E, g, i, j, k, cout_HI, cout_HeI, cout_HeII);
      else entry_columns(*E, g, i, j, k, cout_HI, cout_HeI, cout_HeII);
    }
  }
  store_columns(cs, p, cz, cin_HI, cin_HeI, cin_HeII, cout_HI, cout_HeI, cout_HeII);
}

// The same for a shell s >= 2, with everything that is common to the cells of one shell taken out of the cell's
// work (ShellGeom, c2ray_shell.hpp): no integer division in the thread -> cell map, cinterp's alam as a per-launch
// constant, the path's division by s^2 as three fma, the 12 reciprocals of weightf without the division's operand
// scaling, and the corners' positions from the face formulas of shell s-1 instead of four general inverse maps
// (corners of weight exactly 0 on the edges of a face are read from the nearest cell of shell s-1).  Bit for bit
// the columns of sweep_cell (tests/test_gpu_parity.py::test_fast_sweep_equals_the_general_sweep runs that one for every
// shell, C2R_SWEEP_GENERIC=1, in a process of its own and compares the columns).
// EXT, ENTRY: as in sweep_cell.
template <bool OPEN, bool EXT = false, bool ENTRY = false, bool HALO = false>
__device__ __forceinline__ void sweep_cell_fast(const SweepArgs &A, const SrcDev &S, const ShellGeom &G, int t, const SrcEntry *E = nullptr) {
  static_assert(EXT || !ENTRY, "entry columns belong to a source outside the mesh");
  static_assert(ENTRY || !HALO, "a halo is a kind of entry");
  static_assert(OPEN || !EXT, "a source outside the mesh needs an open axis");
  const Grid &g = A.g;
  const StepScalars &sc = A.sc;
  int di, dj, dk;
  ReachShell RS{}; // (open boundaries: t counts the cells of the shell cut at the source's reach)
  if constexpr (OPEN) RS = reach_shell(S.rl, S.rr, G.s);
  const int face = OPEN ? reach_decode(RS, t, di, dj, dk) : shell_decode_fast(G, t, di, dj, dk);
  Box cut_;
  if constexpr (OPEN) cut_ = source_box(A.box, S);
  const Box &box = OPEN ? cut_ : A.box; // (periodic: the launch's box itself)
  const bool inside = di >= box.lo[0] && di <= box.hi[0] && dj >= box.lo[1] && dj <= box.hi[1] && dk >= box.lo[2] &&
                      dk <= box.hi[2];
  if (!inside) return;
  const size_t cz = S.cz;
  const size_t p = (OPEN ? (size_t)RS.off : (size_t)G.off) + (size_t)t;
  global_double *cs = (global_double *)S.cols;
  const int i = mesh0<OPEN>(S.i0 - 1 + di, g.n1, S.wn[0]), j = mesh0<OPEN>(S.j0 - 1 + dj, g.n2, S.wn[1]),
            k = mesh0<OPEN>(S.k0 - 1 + dk, g.n3, S.wn[2]);
  const bool in_mesh = !EXT || (axis_in_mesh(i, g.n1) && axis_in_mesh(j, g.n2) && axis_in_mesh(k, g.n3));
  double u_HI = 0.0, u_HeI = 0.0, u_HeII = 0.0;
  if (in_mesh) sweep_cell_state(A, i, j, k, face == 2, u_HI, u_HeI, u_HeII);
  ShellCorners c4;
  int ci0 = S.i0, cj0 = S.j0, ck0 = S.k0;
  if constexpr (ENTRY) entry_cinterp_position(*E, ci0, cj0, ck0);
  if constexpr (OPEN) reach_short_characteristic(G, reach_shell(S.rl, S.rr, G.sp), S.rl, S.rr, face, ci0, cj0, ck0, di, dj, dk, c4);
  else shell_short_characteristic(G, face, S.i0, S.j0, S.k0, di, dj, dk, c4);
  double cin_HI = interp_column_fast(c4.s, cs[col_out((size_t)c4.p[0], 0, cz)], cs[col_out((size_t)c4.p[1], 0, cz)],
                                     cs[col_out((size_t)c4.p[2], 0, cz)], cs[col_out((size_t)c4.p[3], 0, cz)], sigma_HI_at_ion_freq);
  const double cin_HeI = interp_column_fast(c4.s, cs[col_out((size_t)c4.p[0], 1, cz)], cs[col_out((size_t)c4.p[1], 1, cz)],
                                            cs[col_out((size_t)c4.p[2], 1, cz)], cs[col_out((size_t)c4.p[3], 1, cz)], sigma_HeI_at_ion_freq);
  const double cin_HeII = interp_column_fast(c4.s, cs[col_out((size_t)c4.p[0], 2, cz)], cs[col_out((size_t)c4.p[1], 2, cz)],
                                             cs[col_out((size_t)c4.p[2], 2, cz)], cs[col_out((size_t)c4.p[3], 2, cz)], sigma_HeII_at_ion_freq);
  const double path = c4.path * sc.dr1;
  if (sc.use_lls && in_mesh) {
    // Lyman-limit-system fog on the incoming HI column (evolve_point.F90:177-180)
    const double coldensh_LLS =
        A.lls_grid ? (double)A.lls_grid[(size_t)i + (size_t)g.n1 * ((size_t)j + (size_t)g.n2 * (size_t)k)] : sc.coldensh_lls;
    cin_HI = cin_HI + coldensh_LLS * path / sc.dr1;
  }
  // coldens (doric.f90:358-372): neufrac * ndens * path * abundance, from the left
  double cout_HI = cin_HI + u_HI * path * (1.0 - abu_he);
  double cout_HeI = cin_HeI + u_HeI * path * abu_he;
  double cout_HeII = cin_HeII + u_HeII * path * abu_he;
  if constexpr (ENTRY) {
    if (E->on && !in_mesh) {
      if constexpr (HALO) halo_columns(*E, g, i, j, k, cout_HI, cout_HeI, cout_HeII);
      else entry_columns(*E, g, i, j, k, cout_HI, cout_HeI, cout_HeII);
    }
  }
  store_columns(cs, p, cz, cin_HI, cin_HeI, cin_HeII, cout_HI, cout_HeI, cout_HeII);
}

// Which 256 cells of a shell of `cnt` cells a block takes (-1: none).  Blocks are dealt round-robin over the 8 XCDs,
// each with its own L2: with block b on cells [256 b, 256 b + 256) the two rows of the previous shell that a row of
// cells reads are fetched by two or three XCDs.  Instead the blocks of one XCD (equal b mod 8) take one contiguous
// eighth of the shell, so that a previous-shell line is fetched by one L2 (the host rounds launches of 64 blocks or
// more up to a multiple of 8; the surplus blocks leave at once).
__device__ __forceinline__ int sweep_block_cell(int cnt) {
  const int nblk_shell = (cnt + BLOCK - 1) / BLOCK;
  int vb = (int)blockIdx.x;
  if ((gridDim.x & 7u) == 0) {
    const int chunk = (int)gridDim.x >> 3;
    vb = ((int)blockIdx.x & 7) * chunk + ((int)blockIdx.x >> 3);
  }
  if (vb >= nblk_shell) return -1;
  const int t = vb * BLOCK + (int)threadIdx.x;
  return t < cnt ? t : -1;
}

// The same for a source of an open launch, whose shell is cut at its reach and has `cnt` cells of its own: the launch is
// sized for the largest cut shell among its sources (launch_shells), the eighths are those of the source's own blocks,
// and the blocks beyond them leave at once.
__device__ __forceinline__ int sweep_block_cell_open(int cnt) {
  const int nblk_shell = (cnt + BLOCK - 1) / BLOCK;
  int vb = (int)blockIdx.x;
  if (nblk_shell >= 64) {
    const int chunk = (nblk_shell + 7) >> 3;
    if (vb >= 8 * chunk) return -1;
    vb = (vb & 7) * chunk + (vb >> 3);
  }
  if (vb >= nblk_shell) return -1;
  const int t = vb * BLOCK + (int)threadIdx.x;
  return t < cnt ? t : -1;
}

// the cells of shell `shell` of source S (open boundaries: within its reach)
template <bool OPEN>
__device__ __forceinline__ int sweep_shell_cells(const SrcDev &S, int shell) {
  if constexpr (OPEN) return (int)(reach_cells(S.rl, S.rr, shell) - reach_cells(S.rl, S.rr, shell - 1));
  else return (int)shell_count(shell);
}

template <bool OPEN>
__global__ void __launch_bounds__(BLOCK, C2R_SWEEP_WAVES)
k_sweep_shell(SweepArgs A, const SrcDev *__restrict__ src, const int *__restrict__ active, int shell) {
  const SrcDev &S = src[active[blockIdx.y]];
  const int t = OPEN ? sweep_block_cell_open(sweep_shell_cells<OPEN>(S, shell)) : sweep_block_cell((int)shell_count(shell));
  if (t >= 0) sweep_cell<OPEN>(A, S, shell, t);
}

template <bool OPEN>
__global__ void __launch_bounds__(BLOCK, C2R_SWEEP_WAVES)
k_sweep_shell_fast(SweepArgs A, const SrcDev *__restrict__ src, const int *__restrict__ active, ShellGeom G) {
  const SrcDev &S = src[active[blockIdx.y]];
  const int t = OPEN ? sweep_block_cell_open(sweep_shell_cells<OPEN>(S, G.s)) : sweep_block_cell(24 * G.s * G.s + 2);
  if (t >= 0) sweep_cell_fast<OPEN>(A, S, G, t);
}

// The two sweep kernels of a batch that holds at least one source outside the mesh (c2r_set_sources_external): the open
// ones with the in-mesh test of sweep_cell's EXT.  Kernels of their own names, as k_rates_beam is beside k_rates: every
// batch without such a source launches the kernels it always launched, under the names they always had.
__global__ void __launch_bounds__(BLOCK, C2R_SWEEP_WAVES)
k_sweep_shell_ext(SweepArgs A, const SrcDev *__restrict__ src, const int *__restrict__ active, int shell) {
  const SrcDev &S = src[active[blockIdx.y]];
  const int t = sweep_block_cell_open(sweep_shell_cells<true>(S, shell));
  if (t >= 0) sweep_cell<true, true>(A, S, shell, t);
}

__global__ void __launch_bounds__(BLOCK, C2R_SWEEP_WAVES)
k_sweep_shell_fast_ext(SweepArgs A, const SrcDev *__restrict__ src, const int *__restrict__ active, ShellGeom G) {
  const SrcDev &S = src[active[blockIdx.y]];
  const int t = sweep_block_cell_open(sweep_shell_cells<true>(S, G.s));
  if (t >= 0) sweep_cell_fast<true, true>(A, S, G, t);
}

// ... and of a batch that holds a source with entry columns (c2r_set_source_face_entry): the two above with the ghost layer of
// sweep_cell's ENTRY.  ent: one record per source of the batch, beside src.  Launched for such a batch only.
__global__ void __launch_bounds__(BLOCK, C2R_SWEEP_WAVES)
k_sweep_shell_entry(SweepArgs A, const SrcDev *__restrict__ src, const int *__restrict__ active, int shell, const SrcEntry *__restrict__ ent) {
  const int b = active[blockIdx.y];
  const SrcDev &S = src[b];
  const int t = sweep_block_cell_open(sweep_shell_cells<true>(S, shell));
  if (t >= 0) sweep_cell<true, true, true>(A, S, shell, t, ent + b);
}

__global__ void __launch_bounds__(BLOCK, C2R_SWEEP_WAVES)
k_sweep_shell_fast_entry(SweepArgs A, const SrcDev *__restrict__ src, const int *__restrict__ active, ShellGeom G,
                         const SrcEntry *__restrict__ ent) {
  const int b = active[blockIdx.y];
  const SrcDev &S = src[b];
  const int t = sweep_block_cell_open(sweep_shell_cells<true>(S, G.s));
  if (t >= 0) sweep_cell_fast<true, true, true>(A, S, G, t, ent + b);
}

// ... and of a batch that holds a source whose halo has several faces (c2r_set_source_halo): the two above with sweep_cell's HALO.
// Twins, not a wider entry_columns: the entry kernels keep their registers and their occupancy, and a batch whose entries all
// have one face launches them as before.
__global__ void __launch_bounds__(BLOCK, C2R_SWEEP_WAVES)
k_sweep_shell_halo(SweepArgs A, const SrcDev *__restrict__ src, const int *__restrict__ active, int shell, const SrcEntry *__restrict__ ent) {
  const int b = active[blockIdx.y];
  const SrcDev &S = src[b];
  const int t = sweep_block_cell_open(sweep_shell_cells<true>(S, shell));
  if (t >= 0) sweep_cell<true, true, true, true>(A, S, shell, t, ent + b);
}

__global__ void __launch_bounds__(BLOCK, C2R_SWEEP_WAVES)
k_sweep_shell_fast_halo(SweepArgs A, const SrcDev *__restrict__ src, const int *__restrict__ active, ShellGeom G,
                        const SrcEntry *__restrict__ ent) {
  const int b = active[blockIdx.y];
  const SrcDev &S = src[b];
  const int t = sweep_block_cell_open(sweep_shell_cells<true>(S, G.s));
  if (t >= 0) sweep_cell_fast<true, true, true, true>(A, S, G, t, ent + b);
}

// Exit strips (c2r_select_source_face_exit): N_out of the cells in the layer of `face` from the shell-ordered blocks of the
// selected sources of a batch whose final boxes are in their records, one thread per face cell (blockIdx.x) and source
// (blockIdx.y).  pairs[2 y], pairs[2 y + 1]: the source's place in the batch and its strip among the face's strips (3 F
// doubles each, species slowest).  A periodic lateral axis maps the mesh index to the image within the reach (axis_offset);
// a layer cell outside the final box gets +0.0.
__global__ void __launch_bounds__(BLOCK)
k_source_face_exit(Grid g, const SrcDev *__restrict__ src, const int *__restrict__ pairs, int face, double *__restrict__ strips) {
  const SrcDev &S = src[pairs[2 * blockIdx.y]];
  const int axis = face >> 1, high = face & 1;
  const int na = axis == 0 ? g.n2 : g.n1, nb = axis == 2 ? g.n2 : g.n3, nc = axis == 0 ? g.n1 : (axis == 1 ? g.n2 : g.n3);
  const size_t F = (size_t)na * (size_t)nb, f = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (f >= F) return;
  // the layer cell of face cell f: the lower of the two other axes fastest
  const int xa = (int)(f % (size_t)na), xb = (int)(f / (size_t)na), xc = high ? nc - 1 : 0;
  const int i = axis == 0 ? xc : xa, j = axis == 0 ? xa : (axis == 1 ? xc : xb), k = axis == 2 ? xc : xb;
  const int di = axis_offset(i, S.i0, S.wn[0]), dj = axis_offset(j, S.j0, S.wn[1]), dk = axis_offset(k, S.k0, S.wn[2]);
  const bool inside = di >= S.lo[0] && di <= S.hi[0] && dj >= S.lo[1] && dj <= S.hi[1] && dk >= S.lo[2] && dk <= S.hi[2];
  // (only a cell of the box, which lies within the reach, has a position)
  const size_t p = inside ? reach_position(S.rl, S.rr, di, dj, dk) : 0;
  double *out = strips + (size_t)pairs[2 * blockIdx.y + 1] * 3 * F;
  const global_double *cs = (const global_double *)S.cols;
  for (int c = 0; c < 3; c++) out[(size_t)c * F + f] = inside ? cs[col_out(p, c, S.cz)] : 0.0;
}

// photon_loss_src_thread(tn) += ... (evolve_point.F90:312): sum the block partials of all shells of
// one sub-box round, per source (blockIdx.x).  Fixed shape (256 strided serial sums, then the
// block tree) => the same bits on every run.
__global__ void __launch_bounds__(BLOCK)
k_loss_finish(const double *__restrict__ loss_partial, int pitch, int count, double *__restrict__ loss_acc) {
  __shared__ double sh[BLOCK / 64];
  const double *p = loss_partial + (size_t)blockIdx.x * pitch;
  double a = 0.0;
  for (int i = threadIdx.x; i < count; i += BLOCK) a += p[i];
  const double tot = block_sum(a, sh);
  if (threadIdx.x == 0) loss_acc[blockIdx.x] = tot;
}

// A quick LOWER BOUND of that loss, to decide "this source goes on" without waiting for the full sum: of every
// `sample`-th block of the round's shells, 8 cells (every 32nd), each cell's bands spread over 32 lanes -- a thread
// evaluates one or two bands, so the launch lasts microseconds where a thread of k_loss walks all bands of
// its cell.  Every term is a non-negative photon count, so any subset, in any order, bounds the loss from below;
// a bound that clears the threshold of evolve_source.F90:136 with a factor 2 to spare is decisive, anything else
// is replaced by the full sum of k_loss.  No bit of any result depends on this kernel.
// The probes of several rounds of a batch in ONE launch (blockIdx.z counts the rounds): the rounds that were swept on
// trust are probed together, and two launches (this one and k_loss_finish_rounds) instead of two per round keep the
// probe's footprint on the device at a few microseconds.
struct ProbeRound {
  int s_lo, s_hi;   // shells of the round
  Box box;          // its sub-box
  int list_off;     // its active list in the batch's list buffer
  int nact;         // sources in that list
  int nblk;         // sampled blocks per source
  int partial_off;  // first partial sum of the round (nblk per source)
  int acc_off;      // first result of the round (one per source)
};
// (OPEN: a bound of the sum that decides -- the box of each source, the faces that can still move.)
template <bool OPEN>
__global__ void __launch_bounds__(BLOCK)
k_loss_probe_rounds(Grid g, const SrcDev *__restrict__ src, const int *__restrict__ lists, const ProbeRound *__restrict__ rounds,
                    int multi, StepScalars sc, const BandData *__restrict__ bd, SedSet ss, const int *__restrict__ block_base,
                    double *__restrict__ loss_partial, int sample) {
  __shared__ double sh[BLOCK / 64];
  const ProbeRound &R = rounds[blockIdx.z];
  if ((int)blockIdx.x >= R.nblk || (int)blockIdx.y >= R.nact) return; // uniform per block
  const SrcDev &S = src[lists[R.list_off + blockIdx.y]];
  Box cut_;
  if constexpr (OPEN) cut_ = source_box(R.box, S);
  const Box &box = OPEN ? cut_ : R.box; // (periodic: the launch's box itself)
  const int s_lo = R.s_lo, s_hi = R.s_hi;
  // every sample-th block counted from the END of the round (the surface of a box is mostly its outermost shell)
  const int B = block_base[s_hi + 1] - 1 - (int)blockIdx.x * sample;
  int lo = s_lo, hi = s_hi; // largest shell with block_base[shell] <= B
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (block_base[mid] <= B) lo = mid; else hi = mid - 1;
  }
  const int shell = lo;
  ReachShell RS{}; // (open boundaries: the shell cut at the source's reach; its blocks are the first of the uncut shell's)
  if constexpr (OPEN) RS = reach_shell(S.rl, S.rr, shell);
  const long long cnt = OPEN ? (long long)RS.cnt : shell_count(shell);
  const int slot = threadIdx.x & 31;
  const long long t = (long long)(B - block_base[shell]) * BLOCK + (threadIdx.x >> 5) * 32;
  double loss = 0.0;
  if (t < cnt) {
    int di, dj, dk;
    if constexpr (OPEN) reach_decode(RS, (int)t, di, dj, dk);
    else shell_decode(shell, (int)t, di, dj, dk);
    const bool inside = di >= box.lo[0] && di <= box.hi[0] && dj >= box.lo[1] && dj <= box.hi[1] && dk >= box.lo[2] &&
                        dk <= box.hi[2];
    const bool boundary = on_counted_face<OPEN>(box, S, di, dj, dk, 1);
    // (unlit cells of a beamed source are left out: terms are only ever left out, so this stays a lower bound)
    // (a curved source: the terms are those of its scaled fluxes, a lower bound of the loss k_loss will find)
    double cf;
    if (inside && boundary && source_flux(S, sc.dr1, sc.dr2, sc.dr3, di, dj, dk, cf)) {
      const size_t cz = S.cz;
      const size_t p = (OPEN ? (size_t)RS.off : (size_t)shell_offset(shell)) + (size_t)t;
      const global_double *cs = (const global_double *)S.cols;
      const double cin_HI = cs[col_in(p, 0, cz)], cin_HeI = cs[col_in(p, 1, cz)], cin_HeII = cs[col_in(p, 2, cz)];
      const double cout_HI = cs[col_out(p, 0, cz)], cout_HeI = cs[col_out(p, 1, cz)], cout_HeII = cs[col_out(p, 2, cz)];
      if (cin_HI < max_coldensh) {
        double vol_ph;
        if (shell == 0) {
          vol_ph = sc.dr1 * sc.dr2 * sc.dr3;
        } else {
          const double path = sc_path(di, dj, dk) * sc.dr1;
          const double xs = sc.dr1 * (double)di, ys = sc.dr2 * (double)dj, zs = sc.dr3 * (double)dk;
          vol_ph = 4.0 * pi * (xs * xs + ys * ys + zs * zs) * path;
        }
        const double nf[NSED] = {curve_scaled(S, S.nflux, cf), curve_scaled(S, S.nflux_sed[0], cf), curve_scaled(S, S.nflux_sed[1], cf)};
        double po = 0.0;
        for (int sd = 0; sd < (multi ? NSED : 1); sd++) {
          if (!(nf[sd] > 0.0)) continue;
          for (int b = ss.lo[sd] + slot; b < ss.hi[sd]; b += 32)
            po += photo_out_band(*bd, sd, ss.photo_thick[sd], ss.photo_thin[sd], b, cin_HI, cout_HI, cin_HeI, cout_HeI, cin_HeII,
                                 cout_HeII, nf[sd]);
        }
        loss = po * sc.vol / vol_ph;
      }
    }
  }
  const double bs = block_sum(loss, sh);
  if (threadIdx.x == 0) loss_partial[(size_t)R.partial_off + (size_t)blockIdx.y * R.nblk + blockIdx.x] = bs;
}
// the partial sums of (round blockIdx.y, source blockIdx.x) added up, fixed shape as k_loss_finish
__global__ void __launch_bounds__(BLOCK)
k_loss_finish_rounds(const ProbeRound *__restrict__ rounds, const double *__restrict__ loss_partial, double *__restrict__ loss_acc) {
  __shared__ double sh[BLOCK / 64];
  const ProbeRound &R = rounds[blockIdx.y];
  if ((int)blockIdx.x >= R.nact) return;
  const double *p = loss_partial + (size_t)R.partial_off + (size_t)blockIdx.x * R.nblk;
  double a = 0.0;
  for (int i = threadIdx.x; i < R.nblk; i += BLOCK) a += p[i];
  const double tot = block_sum(a, sh);
  if (threadIdx.x == 0) loss_acc[R.acc_off + blockIdx.x] = tot;
}

// columns of one slot from shell order back to mesh order (diagnostic download only)
template <bool OPEN>
__global__ void __launch_bounds__(BLOCK)
k_col_to_grid(Grid g, SrcDev S, const double *__restrict__ cs, double *__restrict__ out) {
  const size_t q = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (q >= g.ncell) return;
  const int i = (int)(q % g.n1), j = (int)((q / g.n1) % g.n2), k = (int)(q / ((size_t)g.n1 * g.n2));
  int di = i + 1 - S.i0, dj = j + 1 - S.j0, dk = k + 1 - S.k0;
  if constexpr (!OPEN) {
    di = wrap0(di + g.l1, g.n1) - g.l1;
    dj = wrap0(dj + g.l2, g.n2) - g.l2;
    dk = wrap0(dk + g.l3, g.n3) - g.l3;
  } else { // per axis: wrapped where the axis is periodic, as it is where it is open
    di = axis_offset(i, S.i0, S.wn[0]);
    dj = axis_offset(j, S.j0, S.wn[1]);
    dk = axis_offset(k, S.k0, S.wn[2]);
  }
  const bool inside = di >= S.lo[0] && di <= S.hi[0] && dj >= S.lo[1] && dj <= S.hi[1] && dk >= S.lo[2] && dk <= S.hi[2];
  // (open boundaries: only a cell of the box, which lies within the reach, has a position)
  size_t p = 0;
  if constexpr (OPEN) p = inside ? reach_position(S.rl, S.rr, di, dj, dk) : 0;
  else p = shell_position(di, dj, dk);
  for (int c = 0; c < 3; c++) out[q + c * g.ncell] = inside ? cs[col_out(p, c, S.cz)] : 0.0;
}

// ---------------------------------------------------------------------------------------------
// Rates of every cell from every source of the batch, accumulated in source order
// (evolve_point.F90:246-306 with photoion_rates, radiation_photoionrates.f90:108-277).
// rates layout: [phih | phihe0 | phihe1 | phiheat] each ncell.
#ifndef C2R_RATES_WAVES_ISO
#define C2R_RATES_WAVES_ISO 4
#endif
// Waves per SIMD the register allocation aims at.  The kernel is bound by instruction issue at any of these
// occupancies, so the setting only steers how many copies, spills and waits the compiler makes; measured per variant
// (isothermal: 20.1 / 19.8 / 19.8 ms at 5 / 4 / 3 waves -- 91 registers either way, so five waves still run;
// heating, one SED: 31.5 / 29.4 / 29.5 ms at 4 / 3 / 2 waves; heating, three SEDs: 443 / 466 / 425 ms in round 3, when
// the kernel still kept its per-SED results in scratch memory; round 4, without scratch and without the SED pair:
// 4 waves -- 128 registers, 4 of them spilled -- 358 against 372 ms at 2 waves, see photoion_rates_multi).
#ifndef C2R_RATES_WAVES_HEAT
#define C2R_RATES_WAVES_HEAT 3
#endif
#ifndef C2R_RATES_WAVES_HEAT_MULTI
#define C2R_RATES_WAVES_HEAT_MULTI 4
#endif
// OPEN (open and mixed boundaries): the offset of a cell from a source is what it is along an open axis, no modulo, and
// the image within the mesh's reach along a periodic one (axis_offset); the final sub-box and the surface
// test come from S.lo / S.hi as they always did.  Instantiations of their own: the periodic kernels have no issue slot
// to spare and stay the code they were.
// BEAM (beamed point sources, c2ray_beam.hpp): batches that hold at least one beamed source run k_rates_beam, a kernel of its
// own name with the same arguments, launch shape and source order; batches without one launch the k_rates they always
// launched.  The two share their text (c2ray_rates_body.inc).
#define C2R_RATES_BOUNDS __launch_bounds__(BLOCK, MULTI ? (HEAT ? C2R_RATES_WAVES_HEAT_MULTI : 4) : (HEAT ? C2R_RATES_WAVES_HEAT : C2R_RATES_WAVES_ISO))
template <bool HEAT, bool MULTI, bool OPEN = false>
__global__ void C2R_RATES_BOUNDS
k_rates(Grid g, const SrcDev *__restrict__ src, int nsrc, StepScalars sc, const double *__restrict__ ndens,
        const double *__restrict__ xh_av, const double *__restrict__ xhe_av,
        const BandDataByRow *__restrict__ bdr, SedSet ss, double *__restrict__ rates, const int *__restrict__ tiles,
        const int *__restrict__ tile_ptr, const int *__restrict__ tile_src, int tile_base, int fresh, RatesTables rt) {
  constexpr bool BEAM = false, CURVE = false;
#include "c2ray_rates_body.inc"
}
template <bool HEAT, bool MULTI, bool OPEN = false>
__global__ void C2R_RATES_BOUNDS
k_rates_beam(Grid g, const SrcDev *__restrict__ src, int nsrc, StepScalars sc, const double *__restrict__ ndens,
             const double *__restrict__ xh_av, const double *__restrict__ xhe_av,
             const BandDataByRow *__restrict__ bdr, SedSet ss, double *__restrict__ rates, const int *__restrict__ tiles,
             const int *__restrict__ tile_ptr, const int *__restrict__ tile_src, int tile_base, int fresh, RatesTables rt) {
  constexpr bool BEAM = true, CURVE = false;
#include "c2ray_rates_body.inc"
}
// CURVE (source light curves, c2ray_curve.hpp): batches that hold at least one curved source run k_rates_curve, the third
// kernel over the same text.  What it adds to k_rates_beam: the flux of a cell.source of a curved source is a value per lane,
// NormFlux times the factor of the cell's shell, where the two other kernels hold it in scalar registers; a source of the
// batch without a curve takes k_rates_beam's path, scalar flux included (a uniform branch on its record).
template <bool HEAT, bool MULTI, bool OPEN = false>
__global__ void C2R_RATES_BOUNDS
k_rates_curve(Grid g, const SrcDev *__restrict__ src, int nsrc, StepScalars sc, const double *__restrict__ ndens,
              const double *__restrict__ xh_av, const double *__restrict__ xhe_av,
              const BandDataByRow *__restrict__ bdr, SedSet ss, double *__restrict__ rates, const int *__restrict__ tiles,
              const int *__restrict__ tile_ptr, const int *__restrict__ tile_src, int tile_base, int fresh, RatesTables rt) {
  constexpr bool BEAM = true, CURVE = true;
#include "c2ray_rates_body.inc"
}
#undef C2R_RATES_BOUNDS

// ---------------------------------------------------------------------------------------------
// evolve0D_global + do_chemistry (files_for_3D/evolve_point.F90:325-440, :444-646), one cell per lane.
constexpr int CHEM_HIST = 24; // buckets of the histogram of thermal sub-steps per cell (powers of two)
// deferred cells that fit the device all at once, two waves per SIMD ("Heating global pass in tiers"); a context's own value:
// c2r_ctx::chem_resident
constexpr int CHEM_RESIDENT_CELLS = 131072;
// The counters of a pass -- cells not converged, the histogram, the two longest chains -- are one atomic per wave each,
// and atomics of device scope on ONE address are served one after the other, some 6 ns apiece: with the 262 144
// single-wave blocks of 256^3 every such counter cost 1.6 ms of a 5 ms heating launch (measured: 6.7 ms with three of
// them, 5.1 with two, 3.6 with none).  So the waves spread them over CHEM_CTL_COPIES copies, a page apart, chosen by
// block index; k_chem_ctl_reduce folds the copies into the counters the host reads when the pass is over.
constexpr int CHEM_CTL_COPIES = 64, CHEM_CTL_STRIDE = 1024;            // copies; ints between two of them
constexpr int CHEM_CTL_MAXWORK = CHEM_HIST, CHEM_CTL_MAXNIT = CHEM_HIST + 1, CHEM_CTL_NOTCONV = CHEM_HIST + 2, CHEM_CTL_SLOTS = CHEM_HIST + 3;
#ifndef C2R_CHEM_BLOCK
#define C2R_CHEM_BLOCK 64
#endif
#ifndef C2R_CHEM_WAVES
#define C2R_CHEM_WAVES 2
#endif
// LDSTAB (heating only): the five cooling curves (32 KB) and the log's table (2 KB) in LDS.  A thermal sub-step is one
// long chain of dependent operations, two of whose links are memory round trips -- the table of log10(T), then ten
// cooling-curve entries -- and with two waves per SIMD nothing hides them: from LDS they cost a sixth.  Filling 34 KB
// per block only pays for cells known to sub-cycle, so the first launch of a pass, where most cells are done after
// a handful of sub-steps, reads the tables from global memory and the repacked tiers after it use this variant;
// blocks are two waves there, so that eight waves per compute unit still fit beside 4 x 34 KB.
constexpr int CHEM_BLOCK_LDS = 128;
#if defined(C2R_CHEM_NIT_HIST)
__device__ unsigned long long c2r_chem_nit[64 * 136];
#endif
template <bool HEAT, bool LDSTAB = false>
__global__ void __launch_bounds__(LDSTAB ? CHEM_BLOCK_LDS : C2R_CHEM_BLOCK, C2R_CHEM_WAVES)
k_chemistry(Grid g, StepScalars sc, double dt, const double *__restrict__ ndens, const double *__restrict__ xh,
            const double *__restrict__ xhe, double *__restrict__ xh_av, double *__restrict__ xhe_av,
            double *__restrict__ xh_int, double *__restrict__ xhe_int, float *__restrict__ temperature,
            const double *__restrict__ rates, int *__restrict__ ctl, double *__restrict__ rc_last,
            const float *__restrict__ clumping_grid, size_t q_first, size_t q_end, const int *__restrict__ list,
            int budget, int *__restrict__ deferred, int *__restrict__ ndeferred, double *__restrict__ packed, int cubes) {
  // Cells are taken from the range [q_first, q_end) or, when `list` is given, from list[q_first .. q_end).
  // cubes != 0 (a range of whole k-planes, mesh sizes multiples of 4): a wave takes a 4 x 4 x 4 cube of the range
  // instead of 64 consecutive cells.  A wave lasts as long as its slowest lane, and the cells that need more
  // do_chemistry iterations than their neighbours lie on surfaces (ionisation fronts, the edges of sub-boxes): a row of
  // 64 cells crosses such a surface in one or two cells, a cube in sixteen -- an eighth as many waves are held up
  // (profiles/r04_chem_nit.json: the first iteration of a time step in ionised gas has a mean of 2.2 iterations per cell
  // and of 3.0 per row-shaped wave).  Cubes of one XCD are neighbours (runs of 64 blocks): the other three
  // quarters of every 128-byte line a cube touches belong to the next cubes along i.
  // Heating runs: budget > 0 drops a cell whose thermal sub-cycling passes `budget` steps -- nothing of it is
  // stored -- and appends it to `deferred`, to be redone from scratch by a launch that holds only such cells
  // (c2r_global_pass_finish).  ctl: the spread counters (see CHEM_CTL_COPIES), among them the cells per power of
  // two of sub-steps.
  const size_t nc = g.ncell;
  int *const my_ctl = ctl + (size_t)(blockIdx.x & (CHEM_CTL_COPIES - 1)) * CHEM_CTL_STRIDE;
  __shared__ double s_cool[LDSTAB ? 5 * NCOOL : 1];
  __shared__ double s_log[LDSTAB ? 256 : 1];
  if (LDSTAB) {
    for (int n = (int)threadIdx.x; n < 5 * NCOOL; n += CHEM_BLOCK_LDS) s_cool[n] = sc.cd.cool[n];
    for (int n = (int)threadIdx.x; n < 256; n += CHEM_BLOCK_LDS) s_log[n] = gm::log_table()[n];
    __syncthreads();
    sc.cd.cool = s_cool;
    sc.cd.logtab = s_log;
  } else {
    sc.cd.logtab = nullptr; // known at compile time: coolin's choice of table folds away
  }
  size_t idx = q_first + (size_t)blockIdx.x * (LDSTAB ? CHEM_BLOCK_LDS : C2R_CHEM_BLOCK) + threadIdx.x;
  size_t q_cube = 0;
  if (!LDSTAB && cubes) {
    constexpr int WPB = C2R_CHEM_BLOCK / 64; // waves per block
    int vb = (int)blockIdx.x;
    {
      constexpr int C = 64;
      const int full = (int)(gridDim.x / (8 * C)) * (8 * C);
      if (vb < full) {
        const int r = vb >> 3, xcd = vb & 7;
        vb = (r / C) * (8 * C) + xcd * C + (r % C);
      }
    }
    const int wv = vb * WPB + (int)(threadIdx.x >> 6), lane_ = (int)(threadIdx.x & 63);
    // cubes == 1: 4 x 4 x 4 cells; cubes == 2: 8 x 4 x 2 (rows of 64 bytes)
    const int si = cubes == 2 ? 3 : 2, sk = cubes == 2 ? 1 : 2; // log2 of the extent along i and k (along j: 4)
    const int ci_n = g.n1 >> si, cj_n = g.n2 >> 2;
    const int ci = wv % ci_n, cj = (wv / ci_n) % cj_n, ck = wv / (ci_n * cj_n);
    const size_t plane = (size_t)g.n1 * g.n2;
    const size_t k0 = q_first / plane;
    const size_t i = (size_t)((ci << si) + (lane_ & ((1 << si) - 1))), j = (size_t)(4 * cj + ((lane_ >> si) & 3)),
                 k = k0 + (size_t)((ck << sk) + (lane_ >> (si + 2)));
    q_cube = i + (size_t)g.n1 * (j + (size_t)g.n2 * k);
    idx = q_cube < q_end ? q_first : q_end; // in range (the launch covers whole cubes), or beyond it
  }
  int notconv = 0;
  int bucket = -1;
  int work_done = 0, nit_done = 0;
  bool dropped = false;
  int q_dropped = 0;
  if (idx < q_end) {
    const size_t q = list ? (size_t)list[idx] : ((!LDSTAB && cubes) ? q_cube : idx);
    int work = 0;
    // clumping_point for type_of_clumping = 5 (evolve_point.F90:483-484; REAL(4) grid)
    const double clumping = clumping_grid ? (double)clumping_grid[q] : sc.clumping;
    IonStates ion;
    ion.h[0] = dmax(epsilon, xh_int[q]);       ion.h[1] = dmax(epsilon, xh_int[q + nc]);
    ion.h_old[0] = dmax(epsilon, xh[q]);       ion.h_old[1] = dmax(epsilon, xh[q + nc]);
    const double yh0_av_old = xh_av[q];
    ion.h_av[0] = dmax(epsilon, yh0_av_old);   ion.h_av[1] = dmax(epsilon, xh_av[q + nc]);
    ion.he[0] = dmax(epsilon, xhe_int[q]);     ion.he[1] = dmax(epsilon, xhe_int[q + nc]);
    ion.he[2] = dmax(epsilon, xhe_int[q + 2 * nc]);
    ion.he_old[0] = dmax(epsilon, xhe[q]);     ion.he_old[1] = dmax(epsilon, xhe[q + nc]);
    ion.he_old[2] = dmax(epsilon, xhe[q + 2 * nc]);
    const double yhe0_av_old = xhe_av[q], yhe2_av_old = xhe_av[q + 2 * nc];
    ion.he_av[0] = dmax(epsilon, yhe0_av_old); ion.he_av[1] = dmax(epsilon, xhe_av[q + nc]);
    ion.he_av[2] = dmax(epsilon, yhe2_av_old);
    const double ndens_p = ndens[q];
    const double phi_HI = rates[q], phi_HeI = rates[q + nc], phi_HeII = rates[q + 2 * nc];
    const double heat = HEAT ? rates[q + 3 * nc] : 0.0;

    // get_temperature_point (mat_ini_test.F90:469-487)
    double avg_temper, temper1, temp_av_old;
    if (HEAT) {
      avg_temper = (double)temperature[q + nc];
      temper1 = (double)temperature[q + 2 * nc];
    } else {
      avg_temper = sc.temper_val;
      temper1 = sc.temper_val;
    }
    temp_av_old = avg_temper;
    const double temper0 = temper1;
    RecCoef rc = sc.rc;
    const double path = 1.0;
    int nit = 0;
    for (;;) {
      nit++;
      const double temper2 = temper1;
      const double h0_old = ion.h_av[0], he0_old = ion.he_av[0], he2_old = ion.he_av[2];
      double de = electrondens(ndens_p, ion.h_av, ion.he_av);
      if (HEAT) ini_rec_colion_factors(avg_temper, rc);

      double yfrac, zfrac, y2afrac, y2bfrac;
      prepare_doric_factors(coldens(path, ion.h[0], ndens_p, (1.0 - abu_he)), coldens(path, ion.he[0], ndens_p, abu_he),
                            coldens(path, ion.he[1], ndens_p, abu_he), yfrac, zfrac, y2afrac, y2bfrac);
      doric(dt, de, ion, phi_HI, phi_HeI, phi_HeII, yfrac, zfrac, y2afrac, y2bfrac, rc, clumping);
      de = electrondens(ndens_p, ion.h_av, ion.he_av);
      prepare_doric_factors(coldens(path, ion.h[0], ndens_p, (1.0 - abu_he)), coldens(path, ion.he[0], ndens_p, abu_he),
                            coldens(path, ion.he[1], ndens_p, abu_he), yfrac, zfrac, y2afrac, y2bfrac);
      const double ionh0old = ion.h[0], ionh1old = ion.h[1];
      const double ionhe0old = ion.he[0], ionhe1old = ion.he[1], ionhe2old = ion.he[2];
      const double oldhav = ion.h_av[0], oldhe0av = ion.he_av[0], oldhe1av = ion.he_av[1];
      doric(dt, de, ion, phi_HI, phi_HeI, phi_HeII, yfrac, zfrac, y2afrac, y2bfrac, rc, clumping);
      ion.h[0] = (ion.h[0] + ionh0old) / 2.0;
      ion.h[1] = (ion.h[1] + ionh1old) / 2.0;
      ion.he[0] = (ion.he[0] + ionhe0old) / 2.0;
      ion.he[1] = (ion.he[1] + ionhe1old) / 2.0;
      ion.he[2] = (ion.he[2] + ionhe2old) / 2.0;
      ion.h_av[0] = (ion.h_av[0] + oldhav) / 2.0;
      ion.he_av[0] = (ion.he_av[0] + oldhe0av) / 2.0;
      ion.he_av[1] = (ion.he_av[1] + oldhe1av) / 2.0;
      de = electrondens(ndens_p, ion.h_av, ion.he_av);
      temper1 = temper0;
      if (HEAT) {
        if (thermal(sc.cd, dt, temper1, avg_temper, de, ndens_p, ion, heat, &work, budget)) {
          dropped = true;
          break;
        }
      }

      const double mfc = minimum_fractional_change, mfa = minimum_fraction_of_atoms;
      if ((fabs((ion.h_av[0] - h0_old) / ion.h_av[0]) < mfc || ion.h_av[0] < mfa) &&
          (fabs((ion.he_av[0] - he0_old) / ion.he_av[0]) < mfc || ion.he_av[0] < mfa) &&
          (fabs((ion.he_av[2] - he2_old) / ion.he_av[2]) < mfc || ion.he_av[2] < mfa) &&
          fabs((temper1 - temper2) / temper1) < mfc)
        break;
      if (nit > 400) break;
    }
    if (dropped) {
      q_dropped = (int)q;
    } else {
    if (HEAT) bucket = work > 0 ? 32 - __clz(work) : 0;
    work_done = work;
    nit_done = nit;
    // The reference keeps the coefficients in module-global variables (cgsconstants.f90:106-133): after
    // the global pass they hold what the LAST cell (mesh,mesh,mesh) computed last, and
    // photonstatistics:total_rates then uses those for every cell.  Export them for the host.
    if (HEAT && q == nc - 1) {
      const double v12[12] = {rc.arech0, rc.brech0, rc.areche0, rc.breche0, rc.oreche0, rc.areche1,
                              rc.breche1, rc.treche1, rc.colli_HI, rc.colli_HeI, rc.colli_HeII, rc.v};
      for (int n = 0; n < 12; n++) rc_last[n] = v12[n];
    }
    double temp_av_new = temp_av_old;
    if (HEAT) { // set_temperature_point (mat_ini_test.F90:491-502): stored as REAL(4)
      const float t0 = (float)temper1, t1 = (float)avg_temper;
      temperature[q] = t0;
      temperature[q + nc] = t1;
      temp_av_new = (double)t1;
    }
    const double mfc = minimum_fractional_change, mfa = minimum_fraction_of_atoms;
    if ((fabs(ion.h_av[0] - yh0_av_old) > mfc && fabs((ion.h_av[0] - yh0_av_old) / ion.h_av[0]) > mfc &&
         ion.h_av[0] > mfa) ||
        (fabs(ion.he_av[0] - yhe0_av_old) > mfc && fabs((ion.he_av[0] - yhe0_av_old) / ion.he_av[0]) > mfc &&
         ion.he_av[0] > mfa) ||
        (fabs(ion.he_av[2] - yhe2_av_old) > mfc && fabs((ion.he_av[2] - yhe2_av_old) / ion.he_av[2]) > mfc &&
         ion.he_av[2] > mfa) ||
        (fabs((temp_av_old - temp_av_new) / temp_av_new) > 1.0e-1 && fabs(temp_av_new - temp_av_old) > 100.0))
      notconv = 1;
    xh_int[q] = ion.h[0];       xh_int[q + nc] = ion.h[1];
    xh_av[q] = ion.h_av[0];     xh_av[q + nc] = ion.h_av[1];
    xhe_int[q] = ion.he[0];     xhe_int[q + nc] = ion.he[1];     xhe_int[q + 2 * nc] = ion.he[2];
    xhe_av[q] = ion.he_av[0];   xhe_av[q + nc] = ion.he_av[1];   xhe_av[q + 2 * nc] = ion.he_av[2];
    // what the next pass's column sweep reads of this cell (k_pack_state): neufrac * ndens, fractions clamped at epsilon
    packed[q] = dmax(ion.h_av[0], epsilon) * ndens_p;
    packed[q + nc] = dmax(ion.he_av[0], epsilon) * ndens_p;
    packed[q + 2 * nc] = dmax(ion.he_av[1], epsilon) * ndens_p;
    } // not dropped
  }
  const int lane = threadIdx.x & 63;
  if (HEAT) {
    // the dropped cells of the wave take consecutive places in the list: one atomic per wave
    const unsigned long long dm = __ballot(dropped);
    if (dm) {
      const int leader = __ffsll((long long)dm) - 1;
      int base = 0;
      if (lane == leader) base = atomicAdd(ndeferred, (int)__popcll(dm));
      base = __shfl(base, leader, 64);
      if (dropped) deferred[base + (int)__popcll(dm & ((1ull << lane) - 1ull))] = q_dropped;
    }
    // the longest chain of the launch: most thermal sub-steps and most do_chemistry iterations of one cell
    // (diagnostics, C2R_CHEM_LOG).  A plain look at the copy first: it only ever grows, so a stale value costs one
    // atomic too many and never one too few.
    int wmax = bucket >= 0 ? work_done : 0, nmax = bucket >= 0 ? nit_done : 0;
    for (int off = 32; off > 0; off >>= 1) {
      wmax = max(wmax, __shfl_xor(wmax, off, 64));
      nmax = max(nmax, __shfl_xor(nmax, off, 64));
    }
    if (lane == 0) {
      if (wmax > *(volatile int *)&my_ctl[CHEM_CTL_MAXWORK]) atomicMax(&my_ctl[CHEM_CTL_MAXWORK], wmax);
      if (nmax > *(volatile int *)&my_ctl[CHEM_CTL_MAXNIT]) atomicMax(&my_ctl[CHEM_CTL_MAXNIT], nmax);
    }
    // the histogram: one atomic per wave and distinct bucket
    unsigned long long live = __ballot(bucket >= 0);
    while (live) {
      const int leader = __ffsll((long long)live) - 1;
      const int b = __shfl(bucket, leader, 64);
      const unsigned long long same = __ballot(bucket == b);
      if (lane == leader) atomicAdd(&my_ctl[b], (int)__popcll(same));
      live &= ~same;
    }
  }
  // conv_flag = conv_flag + 1 (evolve_point.F90:423): integer count, order-independent
  const unsigned long long m = __ballot(notconv);
  if (lane == 0 && m) atomicAdd(&my_ctl[CHEM_CTL_NOTCONV], (int)__popcll(m));
#if defined(C2R_CHEM_NIT_HIST)
  // diagnostic build (tools/chem_nit.py): do_chemistry iterations per cell [0..63], and per wave the largest of its
  // lanes [64..127] and the sum over its lanes [128] -- a wave lasts as long as its slowest lane
  {
    unsigned long long *hc = c2r_chem_nit + (blockIdx.x & 63) * 136;
    const int nb = nit_done < 63 ? nit_done : 63;
    int nmx = nit_done;
    long long nsum = nit_done;
    for (int off = 32; off > 0; off >>= 1) {
      nmx = max(nmx, __shfl_xor(nmx, off, 64));
      nsum += __shfl_xor(nsum, off, 64);
    }
    if (idx < q_end) atomicAdd(hc + nb, 1ull);
    if (lane == 0) {
      atomicAdd(hc + 64 + (nmx < 63 ? nmx : 63), 1ull);
      atomicAdd(hc + 128, (unsigned long long)nsum);
    }
  }
#endif
}

// The spread counters of k_chemistry, folded (and zeroed for the next pass): the cells not converged are added to
// conv_flag, the histogram and the two maxima to hist (heating; null otherwise).
__global__ void k_chem_ctl_reduce(int *__restrict__ ctl, int *__restrict__ conv_flag, int *__restrict__ hist) {
  const int t = threadIdx.x;
  if (t >= CHEM_CTL_SLOTS) return;
  const bool is_max = t == CHEM_CTL_MAXWORK || t == CHEM_CTL_MAXNIT;
  int acc = 0;
  for (int k = 0; k < CHEM_CTL_COPIES; k++) {
    int *p = ctl + (size_t)k * CHEM_CTL_STRIDE + t;
    const int v = *p;
    *p = 0;
    acc = is_max ? max(acc, v) : acc + v;
  }
  if (t == CHEM_CTL_NOTCONV) *conv_flag += acc;
  else if (hist) hist[t] = is_max ? max(hist[t], acc) : hist[t] + acc;
}

// ---------------------------------------------------------------------------------------------
// spec_integration (radiation_tables.f90:172-422) for one SED: every entry of the photo and heating
// tables is a 513-point Romberg-weighted sum over frequency of an integrand that holds one exp(-tau*s(nu)).
// One thread = one (tau, band, thick|thin): it walks the frequencies in order (Vector_Romberg is a serial
// sum, romberg.f90:180-186) and carries the photo sum and the up-to-three heating sums of the band.
// Per-frequency factors that do not depend on tau (SED shape, Planck denominator, h(nu - nu_ion)) come
// from the host, computed with the same bit-exact exp/pow (build_sed_vectors below).
// vec layout per band b, frequency x (index b*513 + x): csfd, A (numerator prefix), D (denominator),
// H0, H1, H2 (heating factors) -- six arrays of 47*513.  out: device table layout, pitch NTAUP.
constexpr int SEDV = NFREQ * 513;
__global__ void __launch_bounds__(BLOCK)
k_build_tables(const double *__restrict__ vec, const double *__restrict__ tau_tab, const double *__restrict__ romw,
               const double *__restrict__ delta_freq, int heat, double *__restrict__ photo_thick,
               double *__restrict__ photo_thin, double *__restrict__ heat_thick, double *__restrict__ heat_thin) {
  const int it = blockIdx.x * BLOCK + threadIdx.x;
  const int b = blockIdx.y >> 1, thin = blockIdx.y & 1; // band (0-based), table kind
  if (it > NTAU) return;
  const double tau = tau_tab[it], df = delta_freq[b];
  const double *csfd = vec + (size_t)b * 513, *A = csfd + SEDV, *D = A + SEDV;
  const double *H0 = D + SEDV, *H1 = H0 + SEDV, *H2 = H1 + SEDV;
  const int nh = b < NB1 ? 1 : (b < NB1 + NB2 ? 2 : 3);
  double itg = 0.0, h0 = 0.0, h1 = 0.0, h2 = 0.0;
  for (int x = 0; x <= 512; x++) {
    const double s_ = csfd[x];
    double f = 0.0;
    if (tau * s_ < 700.0) { // :471
      double t = A[x];
      if (thin) t = t * s_;
      t = t * C2R_MATH_EXP(-tau * s_);
      f = t / D[x];
    }
    const double w = romw[x];
    itg = itg + f * df * w;
    if (heat) {
      h0 = h0 + (H0[x] * f) * df * w;
      if (nh > 1) h1 = h1 + (H1[x] * f) * df * w;
      if (nh > 2) h2 = h2 + (H2[x] * f) * df * w;
    }
  }
  double *pt = (thin ? photo_thin : photo_thick) + (size_t)b * NTAUP;
  pt[it] = itg;
  if (it == NTAU) pt[NTAU + 1] = itg; // the duplicated last row (read_table)
  if (heat) {
    // heating columns of the band (radiation_tables.f90:300-310, 343-390), 0-based
    const int c0 = b < NB1 ? 0 : (b < NB1 + NB2 ? 2 * (b + 1) - NB1 - 2 : 3 * (b + 1) - NB2 - 2 * NB1 - 3);
    double *ht = (thin ? heat_thin : heat_thick) + (size_t)c0 * NTAUP;
    const double hv[3] = {h0, h1, h2};
    for (int k = 0; k < nh; k++) {
      ht[(size_t)k * NTAUP + it] = hv[k];
      if (it == NTAU) ht[(size_t)k * NTAUP + NTAU + 1] = hv[k];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// photonstatistics.f90: the grid sums of state_before/state_after (:117-144, :208-234) and of
// total_rates (:150-203).  Fixed launch shape (STAT_BLOCKS x 256, grid-stride, block tree, then one
// finishing block) => the same bits on every run; the order differs from the reference's serial
// loops, so the sums agree with it to rounding (~1e-14 relative), not bit for bit.
constexpr int STAT_BLOCKS = 1024;

template <int NV>
__device__ __forceinline__ void stat_block_reduce(double (&v)[NV], double *partial) {
  __shared__ double sh[NV][BLOCK / 64];
  for (int n = 0; n < NV; n++) {
    double x = v[n];
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if ((threadIdx.x & 63) == 0) sh[n][threadIdx.x >> 6] = x;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double r = 0.0;
    for (int i = 0; i < BLOCK / 64; i++) r += sh[threadIdx.x][i];
    partial[(size_t)blockIdx.x * NV + threadIdx.x] = r;
  }
}

__global__ void __launch_bounds__(BLOCK)
k_state_sums(size_t nc, const double *__restrict__ ndens, const double *__restrict__ xh,
             const double *__restrict__ xhe, double *__restrict__ partial) {
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (size_t q = (size_t)blockIdx.x * BLOCK + threadIdx.x; q < nc; q += (size_t)gridDim.x * BLOCK) {
    const double nd = ndens ? ndens[q] : 1.0; // ndens == nullptr: plain sums of the fractions
    v[0] += nd * xh[q];
    v[1] += nd * xh[q + nc];
    v[2] += nd * xhe[q];
    v[3] += nd * xhe[q + nc];
    v[4] += nd * xhe[q + 2 * nc];
  }
  stat_block_reduce<5>(v, partial);
}

__global__ void __launch_bounds__(BLOCK)
k_total_rates(size_t nc, RecCoef rc, double clumping_scalar, const float *__restrict__ clumping_grid,
              const double *__restrict__ ndens, const double *__restrict__ xh, const double *__restrict__ xhe,
              double *__restrict__ partial) {
  double v[3] = {0.0, 0.0, 0.0};
  for (size_t q = (size_t)blockIdx.x * BLOCK + threadIdx.x; q < nc; q += (size_t)gridDim.x * BLOCK) {
    const double clumping = clumping_grid ? (double)clumping_grid[q] : clumping_scalar; // photonstatistics.f90:175-177
    const double nd = ndens[q];
    const double yh[2] = {xh[q], xh[q + nc]};
    const double yhe[3] = {xhe[q], xhe[q + nc], xhe[q + 2 * nc]};
    const double de = electrondens(nd, yh, yhe);
    v[0] += nd * (yh[1] * rc.brech0 * (1.0 - abu_he) + yhe[1] * rc.breche0 * abu_he * 0.04) * de * clumping;
    v[1] += nd * de * (yh[0] * rc.colli_HI + yhe[0] * rc.colli_HeI + yhe[1] * rc.colli_HeII);
    v[2] += nd * abu_he * clumping * (yhe[2] * 1.121 * rc.breche1 + yhe[1] * rc.breche0 * 0.96) * abu_he * de;
  }
  stat_block_reduce<3>(v, partial);
}

// minval(xh_av(:,:,:,0)), minval(xhe_av(:,:,:,0)) of the log line at evolve.F90:463-466 (a minimum is exact in any order)
__global__ void __launch_bounds__(BLOCK)
k_state_min(size_t nc, const double *__restrict__ xh, const double *__restrict__ xhe, double *__restrict__ partial) {
  __shared__ double sh[2][BLOCK / 64];
  double a = (double)INFINITY, b = (double)INFINITY;
  for (size_t q = (size_t)blockIdx.x * BLOCK + threadIdx.x; q < nc; q += (size_t)gridDim.x * BLOCK) {
    a = dmin(a, xh[q]);
    b = dmin(b, xhe[q]);
  }
  for (int off = 32; off > 0; off >>= 1) {
    a = dmin(a, __shfl_down(a, off, 64));
    b = dmin(b, __shfl_down(b, off, 64));
  }
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = a; sh[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x < 2) {
    double r = sh[threadIdx.x][0];
    for (int i = 1; i < BLOCK / 64; i++) r = dmin(r, sh[threadIdx.x][i]);
    partial[(size_t)blockIdx.x * 2 + threadIdx.x] = r;
  }
}
__global__ void __launch_bounds__(BLOCK)
k_min_finish(const double *__restrict__ partial, int nblocks, double *__restrict__ out) {
  __shared__ double sh[2][BLOCK / 64];
  double a = (double)INFINITY, b = (double)INFINITY;
  for (int i = threadIdx.x; i < nblocks; i += BLOCK) {
    a = dmin(a, partial[(size_t)i * 2]);
    b = dmin(b, partial[(size_t)i * 2 + 1]);
  }
  for (int off = 32; off > 0; off >>= 1) {
    a = dmin(a, __shfl_down(a, off, 64));
    b = dmin(b, __shfl_down(b, off, 64));
  }
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = a; sh[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x < 2) {
    double r = sh[threadIdx.x][0];
    for (int i = 1; i < BLOCK / 64; i++) r = dmin(r, sh[threadIdx.x][i]);
    out[threadIdx.x] = r;
  }
}

template <int NV>
__global__ void __launch_bounds__(BLOCK)
k_stat_finish(const double *__restrict__ partial, int nblocks, double *__restrict__ out) {
  __shared__ double sh[NV][BLOCK / 64];
  for (int n = 0; n < NV; n++) {
    double x = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += BLOCK) x += partial[(size_t)i * NV + n];
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if ((threadIdx.x & 63) == 0) sh[n][threadIdx.x >> 6] = x;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double r = 0.0;
    for (int i = 0; i < BLOCK / 64; i++) r += sh[threadIdx.x][i];
    out[threadIdx.x] = r;
  }
}

// evolve0D for one cell and one source (c2r_evolve0d): the column part (sweep_cell) and the rates part (as k_rates
// for one source) in one thread, the loss through the cell if the caller says it lies on its sub-box's surface.
template <bool HEAT, bool MULTI, bool OPEN = false>
__global__ void __launch_bounds__(64)
k_evolve0d(SweepArgs A, SrcDev S, int di, int dj, int dk, const BandData *__restrict__ bd, SedSet ss, double *__restrict__ rates,
           double *__restrict__ loss_out) {
  if (threadIdx.x != 0) return;
  const Grid &g = A.g;
  const size_t nc = g.ncell;
  const int ia = di < 0 ? -di : di, ja = dj < 0 ? -dj : dj, ka = dk < 0 ? -dk : dk;
  const int shell = ia > ja ? (ia > ka ? ia : ka) : (ja > ka ? ja : ka);
  const size_t p = OPEN ? reach_position(S.rl, S.rr, di, dj, dk) : shell_position(di, dj, dk);
  sweep_cell<OPEN>(A, S, shell, (int)(p - (OPEN ? (size_t)reach_cells(S.rl, S.rr, shell - 1) : (size_t)shell_offset(shell))));
  __threadfence_block();
  const global_double *cs = (const global_double *)S.cols;
  const size_t cz = S.cz;
  const double cin_HI = cs[col_in(p, 0, cz)], cin_HeI = cs[col_in(p, 1, cz)], cin_HeII = cs[col_in(p, 2, cz)];
  const double cout_HI = cs[col_out(p, 0, cz)], cout_HeI = cs[col_out(p, 1, cz)], cout_HeII = cs[col_out(p, 2, cz)];
  const int i = mesh0<OPEN>(S.i0 - 1 + di, g.n1, S.wn[0]), j = mesh0<OPEN>(S.j0 - 1 + dj, g.n2, S.wn[1]),
            k = mesh0<OPEN>(S.k0 - 1 + dk, g.n3, S.wn[2]);
  const size_t q = (size_t)i + (size_t)g.n1 * ((size_t)j + (size_t)g.n2 * (size_t)k);
  const double nd = A.ndens[q];
  const double h0 = dmax(A.xh_av[q], epsilon), h1 = dmax(A.xh_av[q + nc], epsilon);
  const double he0 = dmax(A.xhe_av[q], epsilon), he1 = dmax(A.xhe_av[q + nc], epsilon);
  double vol_ph;
  if (shell == 0) {
    vol_ph = A.sc.dr1 * A.sc.dr2 * A.sc.dr3;
  } else {
    const double path = sc_path(di, dj, dk) * A.sc.dr1;
    const double xs = A.sc.dr1 * (double)di, ys = A.sc.dr2 * (double)dj, zs = A.sc.dr3 * (double)dk;
    const double dist2 = xs * xs + ys * ys + zs * zs;
    vol_ph = 4.0 * pi * dist2 * path;
  }
  double photo_out = 0.0;
  // (the columns above are the cell's whatever the beam: an unlit cell adds no rates and loses nothing)
  // (a curved source: the factor of the cell's shell scales its fluxes, and a shell of factor 0 is unlit)
  double cf;
  if (cin_HI < max_coldensh && source_flux(S, A.sc.dr1, A.sc.dr2, A.sc.dr3, di, dj, dk, cf)) {
    Ricotti ric = {};
    if (HEAT) ric = ricotti_parameters(h1);
    PhotoOut o;
    if (MULTI) {
      const double nf[NSED] = {curve_scaled(S, S.nflux, cf), curve_scaled(S, S.nflux_sed[0], cf), curve_scaled(S, S.nflux_sed[1], cf)};
      photoion_rates_multi<HEAT>(*bd, ss, cin_HI, cout_HI, cin_HeI, cout_HeI, cin_HeII, cout_HeII, vol_ph, nf, ric, o);
    } else {
      photoion_rates<HEAT>(*bd, ss.photo_thick[0], ss.photo_thin[0], ss.heat_thick[0], ss.heat_thin[0], cin_HI, cout_HI, cin_HeI,
                           cout_HeI, cin_HeII, cout_HeII, vol_ph, curve_scaled(S, S.nflux, cf), ric, o);
    }
    rates[q] = rates[q] + o.photo_HI / (h0 * nd * (1.0 - abu_he));
    rates[q + nc] = rates[q + nc] + o.photo_HeI / (he0 * nd * abu_he);
    rates[q + 2 * nc] = rates[q + 2 * nc] + o.photo_HeII / (he1 * nd * abu_he);
    if (HEAT) rates[q + 3 * nc] = rates[q + 3 * nc] + o.heat;
    photo_out = o.photo_out;
  }
  if (loss_out) *loss_out = photo_out * A.sc.vol / vol_ph;
}

// Everything the reference's loop reduces over the grid after a global pass, in one sweep of the arrays
// (c2r_iteration): v[0..4] = k_state_sums with ndens over (xh_intermed, xhe_intermed), v[5..9] = the same without
// ndens (the means), v[10..12] = k_total_rates over (xh_av, xhe_av), and the minima of xh_av(0), xhe_av(0).  Every sum
// runs over the cells in the order of the single-purpose kernels (same grid, same stride, same block tree), so the
// numbers are theirs bit for bit.  rc_dev: the coefficients the chemistry pass left behind (non-isothermal runs).
constexpr int ITER_NV = 13;
__global__ void __launch_bounds__(BLOCK)
k_iter_stats(size_t nc, RecCoef rc_host, const double *__restrict__ rc_dev, double clumping_scalar,
             const float *__restrict__ clumping_grid, const double *__restrict__ ndens, const double *__restrict__ xh_int,
             const double *__restrict__ xhe_int, const double *__restrict__ xh_av, const double *__restrict__ xhe_av,
             double *__restrict__ partial, double *__restrict__ partial_min) {
  RecCoef rc = rc_host;
  if (rc_dev) {
    rc.arech0 = rc_dev[0]; rc.brech0 = rc_dev[1]; rc.areche0 = rc_dev[2]; rc.breche0 = rc_dev[3]; rc.oreche0 = rc_dev[4];
    rc.areche1 = rc_dev[5]; rc.breche1 = rc_dev[6]; rc.treche1 = rc_dev[7]; rc.colli_HI = rc_dev[8]; rc.colli_HeI = rc_dev[9];
    rc.colli_HeII = rc_dev[10]; rc.v = rc_dev[11];
  }
  double v[ITER_NV];
  for (int n = 0; n < ITER_NV; n++) v[n] = 0.0;
  double a = (double)INFINITY, b = (double)INFINITY;
  for (size_t q = (size_t)blockIdx.x * BLOCK + threadIdx.x; q < nc; q += (size_t)gridDim.x * BLOCK) {
    const double nd = ndens[q];
    const double i0 = xh_int[q], i1 = xh_int[q + nc], j0 = xhe_int[q], j1 = xhe_int[q + nc], j2 = xhe_int[q + 2 * nc];
    v[0] += nd * i0; v[1] += nd * i1; v[2] += nd * j0; v[3] += nd * j1; v[4] += nd * j2;
    v[5] += 1.0 * i0; v[6] += 1.0 * i1; v[7] += 1.0 * j0; v[8] += 1.0 * j1; v[9] += 1.0 * j2;
    const double clumping = clumping_grid ? (double)clumping_grid[q] : clumping_scalar; // photonstatistics.f90:175-177
    const double yh[2] = {xh_av[q], xh_av[q + nc]};
    const double yhe[3] = {xhe_av[q], xhe_av[q + nc], xhe_av[q + 2 * nc]};
    const double de = electrondens(nd, yh, yhe);
    v[10] += nd * (yh[1] * rc.brech0 * (1.0 - abu_he) + yhe[1] * rc.breche0 * abu_he * 0.04) * de * clumping;
    v[11] += nd * de * (yh[0] * rc.colli_HI + yhe[0] * rc.colli_HeI + yhe[1] * rc.colli_HeII);
    v[12] += nd * abu_he * clumping * (yhe[2] * 1.121 * rc.breche1 + yhe[1] * rc.breche0 * 0.96) * abu_he * de;
    a = dmin(a, yh[0]);
    b = dmin(b, yhe[0]);
  }
  stat_block_reduce<ITER_NV>(v, partial);
  __shared__ double shm[2][BLOCK / 64];
  for (int off = 32; off > 0; off >>= 1) {
    a = dmin(a, __shfl_down(a, off, 64));
    b = dmin(b, __shfl_down(b, off, 64));
  }
  if ((threadIdx.x & 63) == 0) { shm[0][threadIdx.x >> 6] = a; shm[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x < 2) {
    double r = shm[threadIdx.x][0];
    for (int i = 1; i < BLOCK / 64; i++) r = dmin(r, shm[threadIdx.x][i]);
    partial_min[(size_t)blockIdx.x * 2 + threadIdx.x] = r;
  }
}
// out[0..12] the sums, out[13..14] the minima, out[15..26] the coefficients used
__global__ void __launch_bounds__(BLOCK)
k_iter_stats_finish(const double *__restrict__ partial, const double *__restrict__ partial_min, int nblocks, RecCoef rc_host,
                    const double *__restrict__ rc_dev, double *__restrict__ out) {
  __shared__ double sh[ITER_NV][BLOCK / 64];
  __shared__ double shm[2][BLOCK / 64];
  for (int n = 0; n < ITER_NV; n++) {
    double x = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += BLOCK) x += partial[(size_t)i * ITER_NV + n];
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if ((threadIdx.x & 63) == 0) sh[n][threadIdx.x >> 6] = x;
  }
  double a = (double)INFINITY, b = (double)INFINITY;
  for (int i = threadIdx.x; i < nblocks; i += BLOCK) {
    a = dmin(a, partial_min[(size_t)i * 2]);
    b = dmin(b, partial_min[(size_t)i * 2 + 1]);
  }
  for (int off = 32; off > 0; off >>= 1) {
    a = dmin(a, __shfl_down(a, off, 64));
    b = dmin(b, __shfl_down(b, off, 64));
  }
  if ((threadIdx.x & 63) == 0) { shm[0][threadIdx.x >> 6] = a; shm[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x < ITER_NV) {
    double r = 0.0;
    for (int i = 0; i < BLOCK / 64; i++) r += sh[threadIdx.x][i];
    out[threadIdx.x] = r;
  } else if (threadIdx.x < ITER_NV + 2) {
    const int m = threadIdx.x - ITER_NV;
    double r = shm[m][0];
    for (int i = 1; i < BLOCK / 64; i++) r = dmin(r, shm[m][i]);
    out[threadIdx.x] = r;
  } else if (threadIdx.x < ITER_NV + 2 + 12) {
    const int m = threadIdx.x - ITER_NV - 2;
    const double h[12] = {rc_host.arech0, rc_host.brech0, rc_host.areche0, rc_host.breche0, rc_host.oreche0, rc_host.areche1,
                          rc_host.breche1, rc_host.treche1, rc_host.colli_HI, rc_host.colli_HeI, rc_host.colli_HeII, rc_host.v};
    out[threadIdx.x] = rc_dev ? rc_dev[m] : h[m];
  }
}

// cosmo_evol's ndens(:,:,:) = ndens(:,:,:) / zfactor3 (cosmology.f90:193) on the device copy: one IEEE division per cell,
// correctly rounded on gfx950 as on the host (c2r_scale_ndens)
__global__ void __launch_bounds__(BLOCK) k_divide_by(double *__restrict__ a, size_t n, double d) {
  for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK) a[i] = a[i] / d;
}

// ---------------------------------------------------------------------------------------------
// Escape maps (c2r_enable_face_loss; the rule is c2ray_face.hpp): the terms of the kept loss of an
// open box, photo_out * vol / vol_ph of the cells on open mesh faces, kept per face cell instead of summed.
struct FaceLayout {
  int n[3];    // mesh
  int open[3]; // the axis is open
};

// A gather: lane f of block (x, face) owns face cell x * 256 + f of that face and walks the batch's sources in source
// order, as k_rates walks them for a mesh cell, map = map + term for every source whose final sub-box holds the cell and
// whose rule (face_of_cell) gives the cell to this face.  No atomics: the same bits every time and for every batch size.
// The term is k_loss<true, false>'s, from the same columns through the same functions -- the kernel runs on the sweep
// stream between the batch's last shell and the rates launch, which overwrites N_in(HI) of these cells with the term
// itself (SrcDev::loss_lo).  A wave sits on one face; the source record is uniform over the block (scalar loads); the face
// cells of a source's outermost shell are contiguous runs of its shell-ordered block, so a wave's loads coalesce.
// One lane per face cell leaves the device mostly idle (6 N^2 lanes) -- and costs 6/N of k_rates' cell.source pairs.
template <bool MULTI>
__global__ void __launch_bounds__(BLOCK)
k_face_loss(FaceLayout L, const SrcDev *__restrict__ src, int nsrc, StepScalars sc, const BandData *__restrict__ bd, SedSet ss,
            double *__restrict__ maps) {
  const int face = (int)blockIdx.y;
  const int axis = face >> 1;
  if (!face_pick(axis, L.open[0], L.open[1], L.open[2])) return;
  const int f = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
  if (f >= face_cells(L.n, axis)) return;
  int m[3];
  face_cell_decode(L.n, face, f, m);
  const double dr[3] = {sc.dr1, sc.dr2, sc.dr3};
  double *const slot = maps + face_map_offset(L.n, L.open, face) + f;
  double acc = *slot;
  bool touched = false;
  for (int e = 0; e < nsrc; e++) {
    const SrcDev &S = src[e];
    const int o[3] = {axis_offset(m[0], S.i0, S.wn[0]), axis_offset(m[1], S.j0, S.wn[1]), axis_offset(m[2], S.k0, S.wn[2])};
    const bool outside = o[0] < S.lo[0] || o[0] > S.hi[0] || o[1] < S.lo[1] || o[1] > S.hi[1] || o[2] < S.lo[2] || o[2] > S.hi[2];
    if (outside) continue;
    if (face_of_cell(L.n, L.open, m, o, dr) != face) continue;
    double cf; // (the factor of the cell's shell where the source has a curve)
    if (!source_flux(S, sc.dr1, sc.dr2, sc.dr3, o[0], o[1], o[2], cf)) continue; // the term of an unlit cell is 0.0: acc + 0.0 == acc
    const size_t cz = S.cz;
    const size_t p = reach_position(S.rl, S.rr, o[0], o[1], o[2]);
    const global_double *cs = (const global_double *)S.cols;
    const double cin_HI = cs[col_in(p, 0, cz)], cin_HeI = cs[col_in(p, 1, cz)], cin_HeII = cs[col_in(p, 2, cz)];
    const double cout_HI = cs[col_out(p, 0, cz)], cout_HeI = cs[col_out(p, 1, cz)], cout_HeII = cs[col_out(p, 2, cz)];
    if (!(cin_HI < max_coldensh)) continue;
    double vol_ph;
    if (o[0] == 0 && o[1] == 0 && o[2] == 0) {
      vol_ph = sc.dr1 * sc.dr2 * sc.dr3;
    } else {
      const double path = sc_path(o[0], o[1], o[2]) * sc.dr1;
      const double xs = sc.dr1 * (double)o[0], ys = sc.dr2 * (double)o[1], zs = sc.dr3 * (double)o[2];
      const double dist2 = xs * xs + ys * ys + zs * zs;
      vol_ph = 4.0 * pi * dist2 * path;
    }
    double po;
    if (MULTI) {
      const double nf[NSED] = {curve_scaled(S, S.nflux, cf), curve_scaled(S, S.nflux_sed[0], cf), curve_scaled(S, S.nflux_sed[1], cf)};
      po = photo_out_multi(*bd, ss, cin_HI, cout_HI, cin_HeI, cout_HeI, cin_HeII, cout_HeII, nf);
    } else {
      po = photo_out_only(*bd, ss.photo_thick[0], ss.photo_thin[0], cin_HI, cout_HI, cin_HeI, cout_HeI, cin_HeII, cout_HeII,
                          curve_scaled(S, S.nflux, cf));
    }
    acc = acc + po * sc.vol / vol_ph;
    touched = true;
  }
  if (touched) *slot = acc;
}

// Horizon loss (c2r_enable_horizon_loss; the rule is c2ray_rim.hpp): what crosses the photon horizon
// of the sources of a batch that have one (`list`: their places in the batch, one block row each).
// Lane <-> column: lane t = blockIdx.x * 256 + threadIdx.x of a row is entry t of that source's six sheets (rim_decode: the
// sheet, then the two transverse offsets from the extents of the source's final box, the lower axis fastest); it finds k*
// with the exact predicate, gathers the six columns of the column's cell at its shell position and forms po * w.
// The sum is order-fixed -- the block adds its 256 terms in block_sum's tree, k_loss_finish adds the block sums of a row in
// order, which is face_sum (c2ray_face.hpp) of the T terms -- so a source's loss has the same bits on every run and for every
// batch size; no float atomics.  The last row of the launch also stores its terms (c2r_download_horizon_rim).
// It runs on the sweep stream where k_face_loss runs: after the batch's last shell, the final boxes in the records, before
// the rates launch; it reads interior cells only, whose N_in(HI) slots the rates launch never overwrites.
// Cost: about 6 (2R+1)^2 lanes per source against k_rates' (2R+1)^3 cells -- 3/R of its cell.source pairs, each a
// photo-out band loop without the rates.  Most lanes of a sheet whose columns cross the sphere are busy (pi/4 of them for a
// sphere that fills its box); a wave sits on one sheet, and consecutive lanes read neighbouring cells of a shell face.
template <bool MULTI, bool OPEN>
__global__ void __launch_bounds__(BLOCK)
k_horizon_rim(const SrcDev *__restrict__ src, const int *__restrict__ list, StepScalars sc, const BandData *__restrict__ bd, SedSet ss,
              double *__restrict__ partial, int pitch, double *__restrict__ terms) {
  __shared__ double sh[BLOCK / 64];
  const SrcDev &S = src[list[blockIdx.y]];
  const long long t = (long long)blockIdx.x * BLOCK + (long long)threadIdx.x;
  double term = 0.0;
  int fc, oa, ob;
  if (rim_decode(S.lo, S.hi, t, fc, oa, ob)) {
    int k, o0, o1, o2;
    double w;
    // (a curved source: the face cell's own factor scales the fluxes of its po; a cell in a shell of factor 0 has no face)
    double cf = 1.0;
    bool face = rim_column(S.cut, S.bax, S.bay, S.baz, S.bK, S.hR2, sc.dr1, sc.dr2, sc.dr3, S.lo, S.hi, fc, oa, ob, k, o0, o1, o2, w);
    if (face && (S.cut & CUT_CURVE)) {
      cf = curve_factor_at(S.cR2, S.cfac, sc.dr1, sc.dr2, sc.dr3, o0, o1, o2);
      face = cf != 0.0;
    }
    if (face) {
      const size_t cz = S.cz;
      const size_t p = OPEN ? reach_position(S.rl, S.rr, o0, o1, o2) : shell_position(o0, o1, o2);
      if (p < cz) { // (an interior cell of the final box: the block holds its shell)
        const global_double *cs = (const global_double *)S.cols;
        const double cin_HI = cs[col_in(p, 0, cz)], cin_HeI = cs[col_in(p, 1, cz)], cin_HeII = cs[col_in(p, 2, cz)];
        const double cout_HI = cs[col_out(p, 0, cz)], cout_HeI = cs[col_out(p, 1, cz)], cout_HeII = cs[col_out(p, 2, cz)];
        if (cin_HI < max_coldensh) {
          double po;
          if (MULTI) {
            const double nf[NSED] = {curve_scaled(S, S.nflux, cf), curve_scaled(S, S.nflux_sed[0], cf), curve_scaled(S, S.nflux_sed[1], cf)};
            po = photo_out_multi(*bd, ss, cin_HI, cout_HI, cin_HeI, cout_HeI, cin_HeII, cout_HeII, nf);
          } else {
            po = photo_out_only(*bd, ss.photo_thick[0], ss.photo_thin[0], cin_HI, cout_HI, cin_HeI, cout_HeI, cin_HeII, cout_HeII,
                                curve_scaled(S, S.nflux, cf));
          }
          term = po * w;
        }
      }
    }
    if (blockIdx.y == gridDim.y - 1) terms[t] = term;
  }
  const double bs = block_sum(term, sh);
  if (threadIdx.x == 0) partial[(size_t)blockIdx.y * pitch + blockIdx.x] = bs;
}

} // namespace

// =============================================================================================
// host side
struct c2r_ctx {
  int device = 0;
  std::vector<c2r_ctx *> replicas; // further devices of a context made by c2r_create_multi (each a plain context)
  // sum over ranks (c2ray_comm.inc): kind 0 none, 1 RCCL, 2 in-process sum for replicas that share a device
  int comm_kind = 0, comm_rank = 0, comm_nranks = 1;
  void *comm = nullptr;            // ncclComm_t
  bool comm_broken = false;        // the communicator was aborted after an error inside a collective phase (c2ray_comm.inc)
  std::string comm_broken_why;
  long long slab_passes = 0;       // slab-wise passes this context has run (C2R_FAULT_INJECT counts them)
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_comm_a = nullptr, ev_comm_b = nullptr;
  std::vector<hipEvent_t> ev_sum;  // slab s of the rate grids is summed over the ranks
  // c2r_comm_selftest: per route {mismatches, lowest mismatching index} on the device, the pinned copy the host reads
  // (4 counters, then `got` of either route as doubles), and the timing events of the two routes
  unsigned long long *d_selftest = nullptr, *h_selftest = nullptr;
  hipEvent_t ev_selftest[4] = {nullptr, nullptr, nullptr, nullptr};
  // c2r_get_comm_timing: timing events recorded NEXT TO ev_slab / ev_sum while timing is on -- [0] every slab of rates
  // complete (rates stream), [1] first slab's sum released, [2] last slab's sum complete, [3] tail's sum released,
  // [4] tail's sum complete (comm stream)
  hipEvent_t ev_ct[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  bool ct_rates_recorded = false;
  c2r_comm_timing ctm{};
  hipStream_t stream = nullptr;
  Grid g{};
  mutable std::string err; // (mutable: a getter on a const context says why it refused)

  double *d_photo_thick = nullptr, *d_photo_thin = nullptr, *d_heat_thick = nullptr, *d_heat_thin = nullptr;
  // the heating tables as the kernels read them, interleaved by band (c2ray_device.hpp heat_interleave): [sed][thick, thin];
  // the column-wise copies above (and d_sed_tab[][2..3]) stay for c2r_download_tables and band_tau_zero
  double *d_heat_woven[3][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
  // what the rates kernels read instead of computing it (RatesTables): the pair copy of d_photo_thick, remade wherever that
  // table is written (refresh_tau_zero), and the shell volumes per offset, remade by the first pass after the cell sizes
  // changed (rates_tables); sv_key: the dr1, dr2, dr3, cellvol the table in hand was made from, compared bit by bit
  TablePair *d_photo_pairs = nullptr;
  ShellVol *d_shellvol = nullptr;
  int *d_shellvol_flag = nullptr;
  bool shellvol_valid = false;
  int shellvol_big = 0;
  double sv_key[4] = {0, 0, 0, 0};
  BandDataByRow *d_bands = nullptr;
  BandDataByRow h_bands{};         // host copy (tau_zero is refreshed whenever a table set changes); d_bands is its upload: the
                                   // other kernels take it as its base BandData, the three-SED heating kernel as what it is
  bool have_tables = false, have_heat_tables = false, have_bands = false, have_fvec = false;
  int bb_upper = 0;
  double *d_cool = nullptr;
  bool have_cool = false;
  double cool_mintemp = 1.0, cool_dtemp = 0.01;

  double *d_ndens = nullptr;
  StepScalars sc{};
  double zred = 0, H0 = 0, Omega0 = 0;
  int isothermal = 1;
  bool have_step = false;
  float *d_lls = nullptr, *d_clump = nullptr; // LLS_grid (type_of_LLS = 2), clumping_grid (type_of_clumping = 5)
  bool lls_on_grid = false, clumping_on_grid = false;

  int nsrc = 0;
  std::vector<int> srcpos;
  std::vector<double> normflux;
  double s_star = 0;
  // c2r_set_sources_external: the largest shell that a source OUTSIDE the mesh reaches, through the vacuum between it and
  // the far mesh faces (0: every source of the list stands inside).  The shell bookkeeping is made for it.
  int ext_smax = 0;
  // Point-source hand-over between stacked meshes (c2ray_handover.inc).
  // c2r_set_source_face_entry: per source (empty: no source has one) the face its entry columns come through (-1: none), the
  // rounds it is traced for and its strip on the device; the records of a batch in flight, per scratch set.
  // c2r_set_source_halo: the same record for up to three faces -- `face` is then the lowest of them, faces[d] the face of axis d
  // (-1: the source stands inside along d), and d_cols one allocation that holds the strips, the edge lines and the corner,
  // array a (c2ray_halo.hpp) at off[a] (HALO_ABSENT: none).  An entry of one face is the halo of one face.
  static constexpr size_t HALO_ABSENT = ~(size_t)0;
  struct FaceEntry {
    int face = -1, rounds = 0;
    double *d_cols = nullptr;
    int faces[3] = {-1, -1, -1};
    size_t off[HALO_ARRAYS] = {HALO_ABSENT, HALO_ABSENT, HALO_ABSENT, HALO_ABSENT, HALO_ABSENT, HALO_ABSENT, HALO_ABSENT};
    bool several() const { return (faces[0] >= 0) + (faces[1] >= 0) + (faces[2] >= 0) > 1; }
  };
  std::vector<FaceEntry> src_entry;
  // c2r_set_mesh_origin: where this mesh lies in the deep mesh it is a part of (0: it is the deep mesh, or begins at its cell 1)
  int origin[3] = {0, 0, 0};
  SrcEntry *d_ent[2] = {nullptr, nullptr}, *h_ent[2] = {nullptr, nullptr};
  // c2r_select_source_face_exit: per face the selected sources (1-based), their strips on the device (3 F doubles each), and
  // per strip nbox of the pass that filled it last, whether its final box met the layer, and that pass's stamp (0: none yet)
  struct FaceExit {
    std::vector<int> sources, rounds, reached;
    std::vector<long long> stamp;
    double *d_cols = nullptr;
  };
  FaceExit face_exit[6];
  // -DPL / -DQUASARS: power-law (0) and quasar-like (1) SEDs
  double *d_sed_tab[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};
  int sed_lo[2] = {0, 0}, sed_hi[2] = {0, 0}; // 0-based [lo, hi)
  bool have_sed[2] = {false, false}, have_sed_heat[2] = {false, false}, have_sed_limits[2] = {false, false};
  std::vector<double> normflux_sed[2];
  double s_star_sed[2] = {0, 0};
  // c2r_set_source_beams: one record per source as it was given, and beam_K of each (empty: no source is beamed)
  std::vector<c2r_source_beam> beams;
  std::vector<double> beam_k;
  // c2r_set_source_horizons: one radius per source as it was given, and horizon_R2 of each (empty: no source has a horizon)
  std::vector<double> horizons;
  std::vector<double> horizon_r2;
  // c2r_set_source_curves: one record per source as it was given, the entries behind its steps zeroed (empty: no source has
  // a curve)
  std::vector<c2r_source_curve> curves;

  double *d_xh = nullptr, *d_xhe = nullptr, *d_xh_av = nullptr, *d_xhe_av = nullptr, *d_xh_int = nullptr,
         *d_xhe_int = nullptr;
  float *d_temp = nullptr;
  bool have_state = false;

  double *d_rates = nullptr, *d_rates_own = nullptr;
  bool rates_zero_pending = false; // set_rates_to_zero has been asked for but not yet carried out (see flush_rates_zero)
  bool phiheat_dirty = false;      // a heating run has written phiheat since it was last zeroed
  size_t rates_count = 0;

  int batch = 256;                 // most sources per batch (c2r_set_batch); the scratch arena may allow fewer
  bool periodic = true;            // mesh boundaries (c2r_set_boundaries): periodic on all three axes as the reference, or not
  bool per[3] = {true, true, true}; // ... per axis (c2r_set_boundaries_axes): periodic == all of them.  All false is the open
                                   // mode, anything else the mixed one, which runs on the open kernels and host paths
  // Column scratch: per ping-pong set a list of segments; a source's block is cut from the current segment of
  // its set (shell-ordered arrays are prefixes of one another, so a block that turns out too small moves to a
  // deeper one by six copies).  A set that runs out of room gets another segment -- nothing that exists moves, no
  // sweep starts over.  Segments are zeroed when allocated and only ever hold finite columns afterwards.
  struct Segment {
    double *p = nullptr;
    size_t n = 0; // doubles
  };
  std::vector<Segment> segs[2];
  size_t seg_cur[2] = {0, 0}, seg_used[2] = {0, 0}; // bump allocation within a batch
  std::vector<Segment> vacated[2];                  // blocks whose source moved to a deeper one in this batch: reused first
  size_t arena_total = 0;                          // doubles in all segments
  std::vector<int> prev_nbox;      // per source: sub-boxes of the last pass (0: unknown), sizes the next block
  std::vector<int> prev_grow;      // per source: by how many sub-boxes its box grew from the pass before last to the last one
  int last_first = 0, last_stride = 0; // the share of the sources the last pass swept: first, first + stride, ... (arena_prepare plans the next step's scratch for it)
  bool arena_reserved = false;     // C2R_ARENA_RESERVE_GB has been looked at (first c2r_begin_step)
  bool in_pass = false;            // pass_list is running (arena statistics: allocations that land inside an iteration)
  long long arena_stats[5] = {0, 0, 0, 0, 0}; // segments allocated, of them inside a pass, doubles allocated, block moves, batch restarts
  SrcDev *d_src[2] = {nullptr, nullptr}, *h_src[2] = {nullptr, nullptr}; // source records of the two sets (h: pinned)
  int *d_list[2] = {nullptr, nullptr}, *h_list[2] = {nullptr, nullptr};  // active lists of a batch's rounds, one after another
  size_t list_cap = 0;             // ints per set
  double *d_loss_partial = nullptr, *d_loss_acc = nullptr;
  size_t loss_partial_cap = 0;     // doubles
  // the sampled losses of the rounds of a batch (one entry per round and active source), read back when the
  // sub-box loop needs them
  double *d_probe_partial = nullptr, *d_probe_acc = nullptr, *h_probe = nullptr;
  size_t probe_partial_cap = 0, probe_acc_cap = 0;
  void *d_probe_rounds = nullptr, *h_probe_rounds = nullptr; // ProbeRound[probe_rounds_cap], device and pinned host
  size_t probe_rounds_cap = 0;
  hipEvent_t ev_probe = nullptr;  // the probes launched last, and the copy of their results, are through
  hipEvent_t ev_round = nullptr;  // the shells those probes look at have been queued
  hipStream_t stream_probe = nullptr;           // probes run beside the next rounds' shells
  // losses the rates launch of a batch leaves behind (k_loss_stored), per ping-pong set
  double *d_final_partial[2] = {nullptr, nullptr}, *d_final_acc[2] = {nullptr, nullptr}, *h_final[2] = {nullptr, nullptr};
  size_t final_partial_cap[2] = {0, 0};
  // per batch of the open pass, in order: what photon_loss and sum_nbox get from each of its sources
  // (evolve_source.F90:233-236); a loss still on its way from the device is a slot of h_final[set]
  struct BatchTail {
    int set = 0;
    bool resolved = false;
    std::vector<double> loss;
    std::vector<int> slot; // -1: `loss` holds the value
    std::vector<int> nbox;
    std::vector<int> rim_ns;      // horizon loss: the batch's horizoned sources (1-based), entry j's sum is h_rim[set][j] ...
    std::vector<double> rim_loss; // ... until it is resolved into this
  };
  std::vector<BatchTail> tails;
  double *h_tail = nullptr;       // pinned: photon_loss(1:47), sum_nbox on their way to the reduction buffer
  // rates launches: listed tiles, and for each the sources that reach it (CSR), per set (h: pinned)
  int *d_tiles[2] = {nullptr, nullptr}, *h_tiles[2] = {nullptr, nullptr};
  int *d_tptr[2] = {nullptr, nullptr}, *h_tptr[2] = {nullptr, nullptr};
  int *d_tsrc[2] = {nullptr, nullptr}, *h_tsrc[2] = {nullptr, nullptr};
  size_t tsrc_cap[2] = {0, 0};
  size_t ntiles = 0;
  std::vector<int> tile_count;     // scratch of the CSR construction
  int *d_block_base = nullptr;     // device copy of block_base
  int blocks_total = 0;            // blocks of all shells 0..smax
  std::vector<int> block_base;     // first block of shell s in a partial-sum row
  std::vector<ShellGeom> shell_geom; // per-shell constants of k_sweep_shell_fast
  double *d_colgrid = nullptr;     // 3 ncell, diagnostic download
  double *d_stateT = nullptr;      // 6 ncell: k_pack_state's products in mesh order (3 ncell), then in (j,i,k) order
  bool packed_valid = false;       // the mesh-ordered half matches xh_av / xhe_av (a complete global pass wrote it)
  bool transposed_valid = false;   // ... and the (j,i,k)-ordered half too (that pass queued k_transpose_packed behind itself)
  size_t chem_cells = 0;           // cells the open global pass has been asked to do so far
  double *d_rc_last = nullptr;     // 12: coefficients left by the last cell of the chemistry pass
  double *d_stat = nullptr;        // STAT_BLOCKS*5 partials + 8 results
  double *h_stat = nullptr;        // pinned, 8
  double *d_iter = nullptr;        // k_iter_stats: STAT_BLOCKS*(ITER_NV+2) partials + 32 results
  double *h_iter = nullptr;        // pinned, 32
  int chem_first = 16;              // first rung of the next heating pass's ladder of sub-step ceilings (CHEM_FIRST_CEILING)
  long long chem_resident = CHEM_RESIDENT_CELLS; // the ladder ends once no more cells than this are left (C2R_CHEM_RESIDENT_CELLS)
  // c2r_evolve0d: the column block of the source being traced cell by cell, and which source that is
  double *d_point_cols = nullptr;
  int point_ns = 0, point_niter = 0;
  double *d_point_loss = nullptr, *h_point_loss = nullptr;
  bool want_iter_stats = false;    // the global pass being closed is followed by k_iter_stats (c2r_iteration)
  double *h_loss = nullptr; // pinned, BATCH_MAX
  int *d_conv = nullptr;
  int *h_conv = nullptr;    // pinned
  long long last_conv = -1;  // non-converged cells of the last global pass (-1: a step has just begun); shapes the next pass's waves
  int last_src = 0;
  double *last_cols = nullptr;      // column block of the last source swept (c2r_download_columns)
  size_t last_cz = 0;
  int last_lo[3] = {0, 0, 0}, last_hi[3] = {0, 0, 0};
  // c2r_get_source_trace: what the last pass that swept a source did for it, and when (a count of passes over all contexts
  // of the process, so that a multi-device context can tell which of its devices swept the source last)
  std::vector<c2r_source_trace> trace;
  std::vector<long long> trace_stamp;

  double photon_loss[C2R_NFREQ] = {0};
  int sum_nbox = 0;

  // plane-parallel sources (c2r_set_plane_sources): plane p (1-based) is "source nsrc + p" of every deal.  The buffers are
  // made by c2r_set_plane_sources and live until the planes are removed: never allocated inside a pass.
  // What one plane owns; removing the planes frees the buffers and makes every record a Plane{} again (free_plane_buffers).
  struct Plane {
    c2r_plane_source src = {};
    double tilt[2] = {0.0, 0.0};      // c2r_set_plane_tilt: tangents towards the two face axes ({0, 0}: normal incidence)
    double *d_entry = nullptr, *d_exit = nullptr; // 3 x face each: (HI, HeI, HeII) x face cells
    bool entry_set = false;           // entry columns were given (else zero)
    // flux maps (c2r_set_plane_flux_map): made by the call that sets the first map of the plane, never inside a pass
    double *d_fmap = nullptr, *d_fexit = nullptr; // 3 x face each: (SED 0, 1, 2) x face cells
    bool fmap_set = false;            // the plane has a map (it replaces normflux[])
    bool fmap_uses[2] = {false, false}; // some entry of SED 1 / SED 2 is non-zero (either: the three-SED routine)
    bool fexit_valid = false;         // the last pass that ran the plane ran it with a map: d_fexit holds its exit flux
    // c2r_set_plane_curve: the curve as it was given, the entries behind its steps zeroed (curve_set false: none, no path changes)
    c2r_plane_curve curve = {0, 0, 0.0, {}, {1.0}};
    bool curve_set = false;
    double loss = 0.0;                // the term the plane added to photon_loss(1) in the last pass that ran it
    long long stamp = 0;              // ... and which pass that was (as trace_stamp)
    // side entry (c2r_set_plane_side_entry): the ghost strips of side 0, side 1 and the corner line, na slots of 3 x L each
    // (L = fb, fa, 1); made by the call that sets a strip first, never inside a pass
    double *d_side_in[3] = {}, *d_side_inf[3] = {}; // columns, fluxes
    bool side_in_set[3] = {false, false, false}, side_inf_set[3] = {false, false, false};
    bool side_inf_uses[3][2] = {};    // some entry of SED 1 / SED 2 of that flux strip is non-zero
    // side exit (c2r_enable_plane_side_exit): the strips of side 0 and side 1 in the entry layout, made by the enabling call
    bool side_out_on = false;
    double *d_side_out[2] = {}, *d_side_outf[2] = {};
    bool side_out_valid = false;      // a pass has run the plane with the strips enabled ...
    bool side_out_live[2] = {false, false}; // ... with these sides live ...
    bool side_out_mapped = false;     // ... and with a map (the flux strips hold that pass's)
    // side loss (c2r_enable_plane_side_loss): what the plane added to photon_loss(1) through side 0 and side 1 in the last
    // pass that ran it; side_ran: the side was live in the pass in flight (its sum is on its way to h_side_loss)
    double side_loss[2] = {0.0, 0.0};
    bool side_ran[2] = {false, false};
  };
  int nplane = 0;
  Plane plane[PLANE_MAX];
  // shared by the planes, which run one after another
  double *d_plane_cin = nullptr;    // 3 ncell: the incoming columns of every cell, of the plane being run
  double *d_plane_layer[2] = {};    // 3 x the largest face each: the outgoing columns of a tilted plane's layers, used alternately
  double *d_pflux_layer[2] = {};    // 3 x the largest face each: the flux of a tilted plane's layers, used alternately
  double *d_pflux_cell = nullptr;   // 3 ncell: the flux of every cell of the tilted plane being run
  double *d_plane_partial = nullptr; // block sums of the exit loss
  double *d_plane_loss = nullptr, *h_plane_loss = nullptr; // PLANE_MAX each (h: pinned): the exit loss of the pass in flight
  std::vector<int> pass_planes;     // planes (0-based) of the pass in flight, in order
  // side loss of tilted planes (c2r_enable_plane_side_loss; the rule is c2ray_pside.hpp): made by the enabling call
  bool side_loss_on = false;
  double *d_side_partial = nullptr; // block sums of one side's terms (the largest mesh face)
  double *d_side_loss = nullptr, *h_side_loss = nullptr; // 2 PLANE_MAX each (h: pinned): [2 p + side] of the pass in flight

  // escape maps (c2r_enable_face_loss): the maps of the open faces one behind the other, in face order (face_map_offset,
  // c2ray_face.hpp); made by c2r_enable_face_loss and made anew by a change of boundary mode: never allocated inside a pass
  bool face_on = false;
  double *d_face_maps = nullptr;    // null while the feature is off or no axis is open
  size_t face_total = 0;            // doubles in it

  // horizon loss (c2r_enable_horizon_loss; the rule is c2ray_rim.hpp): everything below is made by c2r_enable_horizon_loss
  // except the block sums, which grow with the batches; nothing exists while the feature is off
  bool rim_on = false;
  std::vector<double> horizon_loss; // per source, the lifetime of photon_loss (a source without a finite horizon stays 0.0)
  double *d_rim_terms = nullptr;    // the terms of the horizoned source swept last: 2*(n1*n2 + n0*n2 + n0*n1) doubles
  size_t rim_terms_cap = 0;
  double *d_rim_partial[2] = {nullptr, nullptr}; // per ping-pong set: block sums, a row per horizoned source of the batch ...
  size_t rim_partial_cap[2] = {0, 0};
  double *d_rim_acc[2] = {nullptr, nullptr}, *h_rim[2] = {nullptr, nullptr}; // ... and their sums (h: pinned), BATCH_MAX each
  int *d_rim_list[2] = {nullptr, nullptr}, *h_rim_list[2] = {nullptr, nullptr}; // the batch's horizoned sources, BATCH_MAX each
  int rim_last_ns = 0, rim_last_ext[3] = {0, 0, 0}; // whose terms d_rim_terms holds, and the extents of its final box
  long long rim_last_stamp = 0;     // ... and the pass that wrote them (as trace_stamp)

  // second stream for the rates kernels: the (latency-bound) column sweep of batch n+1 runs beside
  // the (ALU-bound) rates kernel of batch n; two scratch sets ping-pong between them
  hipStream_t stream2 = nullptr;
  hipStream_t stream3 = nullptr;    // takes every other slab of a cut rates launch (kernel tails overlap)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_transposed = nullptr; // the (j,i,k)-ordered state copies of this pass are complete
  hipEvent_t ev_chem_done = nullptr;  // the launches of a global pass are through (its transposition waits for this)
  hipEvent_t ev_sweep_done[2] = {nullptr, nullptr}, ev_rates_done[2] = {nullptr, nullptr};
  bool set_busy[2] = {false, false};
  std::vector<hipEvent_t> ev_pool; // timing events, grown on demand
  size_t ev_used = 0;

  int chem_pieces = 0;              // pieces of the open global pass (c2r_global_pass_cells)
  double chem_dt = 0.0;
  int *d_defer[2] = {nullptr, nullptr}; // cells dropped by a tier of the heating global pass (ping-pong lists)
  int *d_chemspread = nullptr;      // the per-wave counters of k_chemistry, CHEM_CTL_COPIES copies (k_chem_ctl_reduce)
  int *d_chemctl = nullptr;         // {count of list 0, count of list 1, histogram[CHEM_HIST]}
  // slab-wise hand-over of the rate grids (c2r_pass_sources_begin / _wait_slab / _end)
  bool pass_open = false;
  int pass_slabs = 0;
  std::vector<int> slab_k;          // k-plane boundaries of the slabs
  std::vector<hipEvent_t> ev_slab;
  std::vector<hipEvent_t> pass_tev;

  bool timing = false;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  c2r_timing tm{};
};

static std::string g_create_error;

static int fail(c2r_ctx *c, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_create_error = buf;
  return 1;
}
#define HIPCHK(c, call)                                                                             \
  do {                                                                                              \
    hipError_t e_ = (call);                                                                         \
    if (e_ != hipSuccess) return fail(c, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// hipStreamSynchronize -- with a deadline where the stream may be waiting for OTHER RANKS (an RCCL communicator of more
// than one rank: the chemistry of a slab is queued behind the sum of that slab, the sum waits for every rank).  A rank
// that died, or returned from its pass with an error, never issues its share of the sum, and a plain synchronisation
// would then wait for ever.  C2R_COMM_TIMEOUT_S: seconds to wait (default 1800; 0: for ever).  The caller turns the
// error into an abort of the communicator (with_comm_abort), which is what ends the waiting kernels.
static int sync_stream(c2r_ctx *c, hipStream_t s, const char *what) {
  double limit = 0.0;
  if (c->comm_kind == 1 && c->comm_nranks > 1) {
    const char *e = getenv("C2R_COMM_TIMEOUT_S");
    limit = e ? atof(e) : 1800.0;
  }
  if (limit <= 0.0) {
    HIPCHK(c, hipStreamSynchronize(s));
    return 0;
  }
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spin = 0;; spin++) {
    const hipError_t e = hipStreamQuery(s);
    if (e == hipSuccess) return 0;
    if (e != hipErrorNotReady) return fail(c, "hipStreamQuery failed while waiting for %s: %s", what, hipGetErrorString(e));
    if (spin < 4096) std::this_thread::yield();
    else std::this_thread::sleep_for(std::chrono::microseconds(50));
    const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (waited > limit)
      return fail(c, "rank %d of %d waited %.0f s for %s: a peer rank has not issued its share of the sum over the ranks "
                  "(C2R_COMM_TIMEOUT_S)", c->comm_rank, c->comm_nranks, waited, what);
  }
}

// a context made by c2r_create_multi drives further devices through `replicas` (plain one-device contexts)
template <class F>
static int for_replicas(c2r_ctx *c, F f) {
  if (!c) return 0;
  for (c2r_ctx *r : c->replicas)
    if (int e = f(r)) {
      c->err = "device " + std::to_string(r->device) + ": " + r->err;
      return e;
    }
  return 0;
}

// A run-time flag as a compile-time one: f gets std::true_type or std::false_type, whose ::value picks a kernel's template
// argument.  Nested for two or three flags.
template <class F>
static void with_flag(bool flag, F f) {
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}

extern "C" const char *c2r_last_error(const c2r_ctx *c) { return c ? c->err.c_str() : "null context"; }
extern "C" const char *c2r_create_error(void) { return g_create_error.c_str(); }

// Zero a device range in pieces of at most 1 GiB.  (One hipMemset over more than 16 GiB -- a batch of 16
// scratch slots at 256^3, or any batch at 512^3 -- left the tail of the range untouched on ROCm 7.2;
// found because results then depended on the batch size.)
static hipError_t zero_device(void *ptr, size_t bytes, hipStream_t stream) {
  const size_t piece = (size_t)1 << 30;
  char *p = static_cast<char *>(ptr);
  for (size_t off = 0; off < bytes; off += piece) {
    hipError_t e = hipMemsetAsync(p + off, 0, std::min(piece, bytes - off), stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

static size_t block_doubles(int cap) { // doubles of a column block that holds shells 0..cap
  const size_t w = (size_t)(2 * cap + 1);
  return 6 * w * w * w;
}

// `n` doubles for a column block of set `set`, or nullptr when the device has no room for another segment (the
// caller then shrinks its batch).  Blocks are cut from the set's segments one after another; a new segment is at
// least half of what the set has so far (and 2 GB), so that their number stays small: hipMalloc costs ~25 ms
// per GB on this system, which is why nothing is allocated ahead of need.  `hint`: what the caller knows it will ask
// for in all (a new segment is made that large if the device has the room).
static double *arena_alloc(c2r_ctx *c, int set, size_t n, size_t hint = 0) {
  // a place some source of this batch has moved out of (its stream order protects it: whatever read or copied the old
  // block was queued on the sweep stream before anything the new owner will queue): the smallest that fits
  {
    std::vector<c2r_ctx::Segment> &v = c->vacated[set];
    size_t best = v.size();
    for (size_t i = 0; i < v.size(); i++)
      if (v[i].n >= n && (best == v.size() || v[i].n < v[best].n)) best = i;
    if (best < v.size()) {
      double *p = v[best].p;
      v.erase(v.begin() + (long)best);
      return p;
    }
  }
  for (;;) {
    if (c->seg_cur[set] < c->segs[set].size()) {
      c2r_ctx::Segment &sg = c->segs[set][c->seg_cur[set]];
      if (c->seg_used[set] + n <= sg.n) {
        double *p = sg.p + c->seg_used[set];
        c->seg_used[set] += n;
        return p;
      }
      c->seg_cur[set]++; // the rest of this segment stays unused in this batch
      c->seg_used[set] = 0;
      continue;
    }
    size_t have = 0;
    for (const c2r_ctx::Segment &sg : c->segs[set]) have += sg.n;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return nullptr;
    // a set may hold 45 % of what the device could give to column blocks: the two sets alternate, and a set that
    // took everything would leave the other with batches of a few sources
    size_t budget = (size_t)(0.45 * ((double)(free_b / sizeof(double)) + (double)c->arena_total));
    // C2R_ARENA_BUDGET_MB: a smaller budget per set, so that tests reach the release / shrink paths on small meshes
    if (const char *e = getenv("C2R_ARENA_BUDGET_MB")) budget = std::min(budget, (size_t)(atof(e) * 1.0e6 / sizeof(double)));
    if (have >= budget) return nullptr;
    const size_t room = std::min((size_t)(0.9 * (double)free_b) / sizeof(double), budget - have);
    if (n > room) return nullptr;
    // C2R_ARENA_MIN_SEGMENT_MB (tests): a smaller floor than 2 GB, so that small meshes reach the growth paths
    size_t floor_doubles = (size_t)1 << 28;
    if (const char *e = getenv("C2R_ARENA_MIN_SEGMENT_MB")) floor_doubles = std::max<size_t>(1024, (size_t)(atof(e) * 1.0e6 / sizeof(double)));
    // ... and a ceiling on the geometric growth: on this system a device allocation is free up to some tens of GB and
    // costs ~20 ms per GB beyond (0.97 s for a 45 GB segment, round 5), inside whatever iteration needs it
    size_t ceil_doubles = (size_t)2 << 30; // 16 GB
    if (const char *e = getenv("C2R_ARENA_MAX_SEGMENT_GB")) ceil_doubles = std::max<size_t>(floor_doubles, (size_t)(atof(e) * 1.0e9 / sizeof(double)));
    const size_t want = std::min(room, std::max(std::max(n, hint), std::max(std::min(have / 2, ceil_doubles), floor_doubles)));
    c2r_ctx::Segment sg;
    const auto t0 = std::chrono::steady_clock::now();
    if (hipMalloc(&sg.p, sizeof(double) * want) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    sg.n = want;
    // zeroed on the sweep stream: whatever uses the block is queued behind it there
    if (zero_device(sg.p, sizeof(double) * want, c->stream) != hipSuccess) { (void)hipFree(sg.p); return nullptr; }
    if (getenv("C2R_ARENA_LOG"))
      fprintf(stderr, "c2ray_hip: column scratch, set %d: segment %zu of %.2f GB (%.0f ms), %.2f GB in all\n", set,
              c->segs[set].size(), want * 8e-9, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(),
              (c->arena_total + want) * 8e-9);
    c->segs[set].push_back(sg);
    c->arena_total += want;
    c->arena_stats[0]++;
    if (c->in_pass) c->arena_stats[1]++;
    c->arena_stats[2] += (long long)want;
  }
}

// Give a set's segments back to the device.  Only when nothing in flight uses them: the caller has waited for the
// set's last rates launch and has not yet started a sweep on it.
static void arena_release(c2r_ctx *c, int set) {
  (void)hipStreamSynchronize(c->stream); // segments are zeroed on the sweep stream
  for (c2r_ctx::Segment &sg : c->segs[set]) {
    (void)hipFree(sg.p);
    c->arena_total -= sg.n;
    if (c->last_cols >= sg.p && c->last_cols < sg.p + sg.n) c->last_cols = nullptr;
  }
  c->segs[set].clear();
  c->vacated[set].clear();
  c->seg_cur[set] = c->seg_used[set] = 0;
  if (getenv("C2R_ARENA_LOG")) fprintf(stderr, "c2ray_hip: column scratch, set %d released, %.2f GB left in all\n", set, c->arena_total * 8e-9);
}

template <class T>
static int ensure_pair(c2r_ctx *c, T **d, T **h, size_t *cap, size_t need) {
  if (*cap >= need) return 0;
  if (*d) HIPCHK(c, hipFree(*d));
  if (h && *h) HIPCHK(c, hipHostFree(*h));
  *d = nullptr;
  if (h) *h = nullptr;
  const size_t want = need + need / 2 + 1024;
  HIPCHK(c, hipMalloc(d, sizeof(T) * want));
  if (h) HIPCHK(c, hipHostMalloc(h, sizeof(T) * want));
  *cap = want;
  return 0;
}

// What follows from the largest shell a source of this mesh can reach: mesh/2 with periodic boundaries
// (evolve_source.F90:105), mesh - 1 with open ones (a source in a corner, :107-108).  Host side only; the device copies
// are made by the caller.
// A source outside an open mesh (c2r_set_sources_external) reaches further, through the vacuum up to the far mesh face:
// c->ext_smax, which set_sources_one has checked against EXTERNAL_REACH_MAX.  Everything that is sized or indexed by shell
// number follows from smax here: block_base (and with it every row of loss partials, which are sized from block_base
// differences), shell_geom, the list buffers, the probe results (sweep_batch) and start_over's round limit.
static long long shell_blocks_upto(int smax) {
  long long n = 0;
  for (int s = 0; s <= smax; s++) n += (shell_count(s) + BLOCK - 1) / BLOCK;
  return n;
}
static void shell_bookkeeping(c2r_ctx *c) {
  Grid &g = c->g;
  g.smax = c->periodic ? std::max(g.l1, std::max(g.l2, g.l3))
                       : std::max(c->ext_smax, std::min(MAX_SUBBOX, std::max(g.n1, std::max(g.n2, g.n3)) - 1));
  g.colsize = (size_t)(2 * g.smax + 1) * (2 * g.smax + 1) * (2 * g.smax + 1);
  // block bookkeeping of the shells 0..smax
  c->block_base.assign(g.smax + 2, 0);
  for (int s = 0; s <= g.smax; s++)
    c->block_base[s + 1] = c->block_base[s] + (int)((shell_count(s) + BLOCK - 1) / BLOCK);
  c->blocks_total = c->block_base[g.smax + 1];
  c->shell_geom.clear();
  for (int s = 0; s <= g.smax; s++) c->shell_geom.push_back(shell_geometry(s));
  // active lists of all rounds of a batch, one after another (two per round at most, plus the final losses)
  // (per round: the active list, the undecided, and the probed ones where a source with entry columns is left out; behind
  // the rounds, the kept losses' lists and the pairs of the exit strips of up to six faces, c2ray_handover.inc)
  c->list_cap = (size_t)(3 * (g.smax / SUBBOXSIZE + 2) + 4 + 12) * BATCH_MAX;
}

extern "C" int c2r_create(c2r_ctx **out, int device, const int mesh[3]) {
  if (!out || !mesh) return fail(nullptr, "c2r_create: null argument");
  if (mesh[0] < 2 || mesh[1] < 2 || mesh[2] < 2 || mesh[0] > 4096 || mesh[1] > 4096 || mesh[2] > 4096)
    return fail(nullptr, "c2r_create: mesh %d x %d x %d out of range [2,4096]", mesh[0], mesh[1], mesh[2]);
  // cell numbers travel as 32-bit integers through the tile lists and the chemistry's lists of deferred cells
  if ((double)mesh[0] * mesh[1] * mesh[2] >= 2147483648.0)
    return fail(nullptr, "c2r_create: mesh %d x %d x %d has 2^31 cells or more (the largest cube is 1290^3)", mesh[0], mesh[1], mesh[2]);
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    return fail(nullptr, "c2r_create: no HIP device available (%s); this library has no CPU path",
                e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  if (device < 0 || device >= ndev) return fail(nullptr, "c2r_create: device %d not in [0,%d)", device, ndev);
  long long chem_resident = CHEM_RESIDENT_CELLS;
  if (const char *e = getenv("C2R_CHEM_RESIDENT_CELLS")) {
    char *end = nullptr;
    errno = 0;
    chem_resident = strtoll(e, &end, 10);
    if (end == e || *end != '\0' || errno != 0 || chem_resident < 0)
      return fail(nullptr, "c2r_create: C2R_CHEM_RESIDENT_CELLS=\"%s\" is not a cell count (a whole number, 0 or more)", e);
  }
  c2r_ctx *c = new c2r_ctx;
  c->chem_resident = chem_resident;
  c->device = device;
  c->g.n1 = mesh[0]; c->g.n2 = mesh[1]; c->g.n3 = mesh[2];
  c->g.l1 = mesh[0] / 2; c->g.l2 = mesh[1] / 2; c->g.l3 = mesh[2] / 2;
  c->g.ncell = (size_t)mesh[0] * mesh[1] * mesh[2];
  shell_bookkeeping(c);
  const size_t nc = c->g.ncell;
#define CR(call)                                                                                    \
  do {                                                                                              \
    hipError_t e_ = (call);                                                                         \
    if (e_ != hipSuccess) {                                                                         \
      fail(nullptr, "%s failed: %s", #call, hipGetErrorString(e_));                                 \
      c2r_destroy(c);                                                                               \
      return 1;                                                                                     \
    }                                                                                               \
  } while (0)
  CR(hipSetDevice(device));
  {
    int lo = 0, hi = 0; // numerically lower = higher priority
    CR(hipDeviceGetStreamPriorityRange(&lo, &hi));
    CR(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, hi));
    CR(hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, lo));
    CR(hipStreamCreateWithPriority(&c->stream3, hipStreamNonBlocking, lo));
    CR(hipStreamCreateWithPriority(&c->stream_probe, hipStreamNonBlocking, hi));
    CR(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    CR(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    CR(hipEventCreateWithFlags(&c->ev_transposed, hipEventDisableTiming));
    CR(hipEventCreateWithFlags(&c->ev_chem_done, hipEventDisableTiming));
  }
  for (int i = 0; i < 2; i++) {
    CR(hipEventCreateWithFlags(&c->ev_sweep_done[i], hipEventDisableTiming));
    CR(hipEventCreateWithFlags(&c->ev_rates_done[i], hipEventDisableTiming));
  }
  CR(hipMalloc(&c->d_ndens, sizeof(double) * nc));
  CR(hipMalloc(&c->d_xh, sizeof(double) * 2 * nc));
  CR(hipMalloc(&c->d_xhe, sizeof(double) * 3 * nc));
  CR(hipMalloc(&c->d_xh_av, sizeof(double) * 2 * nc));
  CR(hipMalloc(&c->d_xhe_av, sizeof(double) * 3 * nc));
  CR(hipMalloc(&c->d_xh_int, sizeof(double) * 2 * nc));
  CR(hipMalloc(&c->d_xhe_int, sizeof(double) * 3 * nc));
  CR(hipMalloc(&c->d_temp, sizeof(float) * 3 * nc));
  CR(hipMalloc(&c->d_stateT, sizeof(double) * 6 * nc));
  CR(hipMalloc(&c->d_rc_last, sizeof(double) * 12));
  CR(hipMemset(c->d_rc_last, 0, sizeof(double) * 12));
  CR(hipMalloc(&c->d_stat, sizeof(double) * (STAT_BLOCKS * 5 + 8)));
  CR(hipHostMalloc(&c->h_stat, sizeof(double) * 8));
  CR(hipMalloc(&c->d_iter, sizeof(double) * (STAT_BLOCKS * (ITER_NV + 2) + 32)));
  CR(hipHostMalloc(&c->h_iter, sizeof(double) * 32));
  c->rates_count = 4 * nc + C2R_NFREQ + 1;
  CR(hipMalloc(&c->d_rates_own, sizeof(double) * c->rates_count));
  c->d_rates = c->d_rates_own;
  CR(zero_device(c->d_rates, sizeof(double) * c->rates_count, nullptr));
  // the spread counters of the chemistry launches (CHEM_CTL_COPIES): here, not in the first global pass -- an allocation
  // is a device-wide synchronisation, and an outer iteration has exactly one, at its end
  CR(hipMalloc(&c->d_chemspread, sizeof(int) * (size_t)CHEM_CTL_COPIES * CHEM_CTL_STRIDE));
  CR(hipMemset(c->d_chemspread, 0, sizeof(int) * (size_t)CHEM_CTL_COPIES * CHEM_CTL_STRIDE)); // k_chem_ctl_reduce leaves it zeroed
  CR(hipDeviceSynchronize()); // phih_grid = 0 for initial output (evolve_data.F90:77,80)
  CR(hipMalloc(&c->d_block_base, sizeof(int) * c->block_base.size()));
  CR(hipMemcpy(c->d_block_base, c->block_base.data(), sizeof(int) * c->block_base.size(), hipMemcpyHostToDevice));
  c->ntiles = (size_t)((mesh[0] + 7) / 8) * ((mesh[1] + 7) / 8) * ((mesh[2] + 3) / 4);
  for (int k = 0; k < 2; k++) {
    CR(hipMalloc(&c->d_tiles[k], sizeof(int) * c->ntiles));
    CR(hipHostMalloc(&c->h_tiles[k], sizeof(int) * c->ntiles));
    CR(hipMalloc(&c->d_tptr[k], sizeof(int) * (c->ntiles + 1)));
    CR(hipHostMalloc(&c->h_tptr[k], sizeof(int) * (c->ntiles + 1)));
    CR(hipMalloc(&c->d_src[k], sizeof(SrcDev) * BATCH_MAX));
    CR(hipHostMalloc(&c->h_src[k], sizeof(SrcDev) * BATCH_MAX));
    CR(hipMalloc(&c->d_list[k], sizeof(int) * c->list_cap));
    CR(hipHostMalloc(&c->h_list[k], sizeof(int) * c->list_cap));
  }
  CR(hipMalloc(&c->d_loss_acc, sizeof(double) * BATCH_MAX));
  CR(hipHostMalloc(&c->h_loss, sizeof(double) * BATCH_MAX));
  CR(hipEventCreateWithFlags(&c->ev_probe, hipEventDisableTiming));
  CR(hipEventCreateWithFlags(&c->ev_round, hipEventDisableTiming));
  for (int k = 0; k < 2; k++) {
    CR(hipMalloc(&c->d_final_acc[k], sizeof(double) * BATCH_MAX));
    CR(hipHostMalloc(&c->h_final[k], sizeof(double) * BATCH_MAX));
  }
  CR(hipHostMalloc(&c->h_tail, sizeof(double) * (C2R_NFREQ + 1)));
  CR(hipMalloc(&c->d_conv, sizeof(int)));
  CR(hipHostMalloc(&c->h_conv, sizeof(int)));
  CR(hipMalloc(&c->d_bands, sizeof(BandDataByRow)));
  for (auto &ev : c->ev) CR(hipEventCreate(&ev));
#undef CR
  *out = c;
  return 0;
}

// the escape maps of one device (c2r_enable_face_loss, set_boundaries_one, c2r_destroy)
static void free_face_maps(c2r_ctx *c) {
  if (c->d_face_maps) (void)hipFree(c->d_face_maps);
  c->d_face_maps = nullptr;
  c->face_total = 0;
}

// ... made anew for the boundary mode in force, and zeroed (no buffer when no axis is open)
static int alloc_face_maps(c2r_ctx *c) {
  HIPCHK(c, hipSetDevice(c->device));
  if (c->d_face_maps) HIPCHK(c, hipStreamSynchronize(c->stream)); // nothing queued may still add to them
  free_face_maps(c);
  const int n[3] = {c->g.n1, c->g.n2, c->g.n3}, open[3] = {!c->per[0], !c->per[1], !c->per[2]};
  const size_t total = (size_t)face_map_offset(n, open, 6);
  if (total == 0) return 0;
  HIPCHK(c, hipMalloc(&c->d_face_maps, sizeof(double) * total));
  c->face_total = total;
  HIPCHK(c, zero_device(c->d_face_maps, sizeof(double) * total, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// the buffers of the horizon loss of one device (c2r_enable_horizon_loss, c2r_destroy)
static void free_horizon_loss(c2r_ctx *c) {
  if (c->d_rim_terms) (void)hipFree(c->d_rim_terms);
  c->d_rim_terms = nullptr;
  c->rim_terms_cap = 0;
  for (int k = 0; k < 2; k++) {
    if (c->d_rim_partial[k]) (void)hipFree(c->d_rim_partial[k]);
    if (c->d_rim_acc[k]) (void)hipFree(c->d_rim_acc[k]);
    if (c->h_rim[k]) (void)hipHostFree(c->h_rim[k]);
    if (c->d_rim_list[k]) (void)hipFree(c->d_rim_list[k]);
    if (c->h_rim_list[k]) (void)hipHostFree(c->h_rim_list[k]);
    c->d_rim_partial[k] = c->d_rim_acc[k] = c->h_rim[k] = nullptr;
    c->d_rim_list[k] = c->h_rim_list[k] = nullptr;
    c->rim_partial_cap[k] = 0;
  }
}

static void free_plane_buffers(c2r_ctx *c); // c2ray_planes.inc
static void free_side_loss(c2r_ctx *c);     // c2ray_planes.inc

extern "C" void c2r_destroy(c2r_ctx *c) {
  if (!c) return;
  (void)c2r_comm_destroy(c);
  for (c2r_ctx *r : c->replicas) c2r_destroy(r);
  c->replicas.clear();
  (void)hipSetDevice(c->device);
  if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
  if (c->ev_comm_a) (void)hipEventDestroy(c->ev_comm_a);
  if (c->ev_comm_b) (void)hipEventDestroy(c->ev_comm_b);
  for (auto &ev : c->ev_sum) (void)hipEventDestroy(ev);
  for (auto &ev : c->ev_selftest)
    if (ev) (void)hipEventDestroy(ev);
  for (auto &ev : c->ev_ct)
    if (ev) (void)hipEventDestroy(ev);
  if (c->d_selftest) (void)hipFree(c->d_selftest);
  if (c->h_selftest) (void)hipHostFree(c->h_selftest);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (auto &row : c->d_sed_tab)
    for (double *p : row)
      if (p) (void)hipFree(p);
  void *ptrs[] = {c->d_photo_pairs, c->d_shellvol, c->d_shellvol_flag, c->d_photo_thick, c->d_photo_thin, c->d_heat_thick, c->d_heat_thin, c->d_bands, c->d_cool,
                  c->d_ndens, c->d_xh, c->d_xhe, c->d_xh_av, c->d_xhe_av, c->d_xh_int, c->d_xhe_int, c->d_temp,
                  c->d_rates_own, c->d_stateT, c->d_loss_partial, c->d_loss_acc, c->d_conv, c->d_colgrid, c->d_rc_last, c->d_stat, c->d_lls, c->d_clump, c->d_block_base, c->d_defer[0], c->d_defer[1], c->d_chemctl, c->d_chemspread};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  for (auto &w : c->d_heat_woven)
    for (double *p : w)
      if (p) (void)hipFree(p);
  for (auto &list : c->segs)
    for (auto &sg : list)
      if (sg.p) (void)hipFree(sg.p);
  for (c2r_ctx::FaceEntry &e : c->src_entry)
    if (e.d_cols) (void)hipFree(e.d_cols);
  for (c2r_ctx::FaceExit &x : c->face_exit)
    if (x.d_cols) (void)hipFree(x.d_cols);
  for (int k = 0; k < 2; k++) {
    if (c->d_ent[k]) (void)hipFree(c->d_ent[k]);
    if (c->h_ent[k]) (void)hipHostFree(c->h_ent[k]);
  }
  if (c->h_loss) (void)hipHostFree(c->h_loss);
  if (c->h_probe) (void)hipHostFree(c->h_probe);
  if (c->h_tail) (void)hipHostFree(c->h_tail);
  if (c->d_probe_partial) (void)hipFree(c->d_probe_partial);
  if (c->d_probe_rounds) (void)hipFree(c->d_probe_rounds);
  if (c->h_probe_rounds) (void)hipHostFree(c->h_probe_rounds);
  if (c->ev_probe) (void)hipEventDestroy(c->ev_probe);
  if (c->ev_round) (void)hipEventDestroy(c->ev_round);
  for (int k = 0; k < 2; k++) {
    if (c->d_final_partial[k]) (void)hipFree(c->d_final_partial[k]);
    if (c->d_final_acc[k]) (void)hipFree(c->d_final_acc[k]);
    if (c->h_final[k]) (void)hipHostFree(c->h_final[k]);
  }
  if (c->d_probe_acc) (void)hipFree(c->d_probe_acc);
  for (int k = 0; k < 2; k++) {
    void *dev[] = {c->d_tiles[k], c->d_tptr[k], c->d_tsrc[k], c->d_src[k], c->d_list[k]};
    void *host[] = {c->h_tiles[k], c->h_tptr[k], c->h_tsrc[k], c->h_src[k], c->h_list[k]};
    for (void *q : dev)
      if (q) (void)hipFree(q);
    for (void *q : host)
      if (q) (void)hipHostFree(q);
  }
  free_plane_buffers(c);
  free_side_loss(c);
  free_face_maps(c);
  free_horizon_loss(c);
  if (c->h_conv) (void)hipHostFree(c->h_conv);
  if (c->h_stat) (void)hipHostFree(c->h_stat);
  if (c->h_iter) (void)hipHostFree(c->h_iter);
  if (c->h_point_loss) (void)hipHostFree(c->h_point_loss);
  if (c->d_point_loss) (void)hipFree(c->d_point_loss);
  if (c->d_point_cols) (void)hipFree(c->d_point_cols);
  if (c->d_iter) (void)hipFree(c->d_iter);
  for (auto &ev : c->ev)
    if (ev) (void)hipEventDestroy(ev);
  for (auto &ev : c->ev_pool) (void)hipEventDestroy(ev);
  for (auto &ev : c->ev_slab) (void)hipEventDestroy(ev);
  for (int i = 0; i < 2; i++) {
    if (c->ev_sweep_done[i]) (void)hipEventDestroy(c->ev_sweep_done[i]);
    if (c->ev_rates_done[i]) (void)hipEventDestroy(c->ev_rates_done[i]);
  }
  if (c->stream2) { (void)hipStreamSynchronize(c->stream2); (void)hipStreamDestroy(c->stream2); }
  if (c->stream3) { (void)hipStreamSynchronize(c->stream3); (void)hipStreamDestroy(c->stream3); }
  if (c->stream_probe) { (void)hipStreamSynchronize(c->stream_probe); (void)hipStreamDestroy(c->stream_probe); }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->ev_transposed) (void)hipEventDestroy(c->ev_transposed);
  if (c->ev_chem_done) (void)hipEventDestroy(c->ev_chem_done);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

// host (0:NumTau, ncol) -> device columns of pitch NTAUP with row 2001 = row 2000
static int upload_table(c2r_ctx *c, const double *src, int ncol, double **dst) {
  std::vector<double> tmp((size_t)ncol * NTAUP);
  for (int col = 0; col < ncol; col++) {
    const double *s = src + (size_t)col * (NTAU + 1);
    double *d = tmp.data() + (size_t)col * NTAUP;
    std::memcpy(d, s, sizeof(double) * (NTAU + 1));
    d[NTAU + 1] = s[NTAU];
  }
  if (!*dst) HIPCHK(c, hipMalloc(dst, sizeof(double) * tmp.size()));
  HIPCHK(c, hipMemcpy(*dst, tmp.data(), sizeof(double) * tmp.size(), hipMemcpyHostToDevice));
  return 0;
}

// BandData::tau_zero of SED `sed` (0 black body, 1 power law, 2 quasar) from the tables now on the device
// (uploaded or built there), and the band data to the device again.
static int refresh_tau_zero(c2r_ctx *c, int sed) {
  const double *tab[4] = {sed == 0 ? c->d_photo_thick : c->d_sed_tab[sed - 1][0], sed == 0 ? c->d_photo_thin : c->d_sed_tab[sed - 1][1],
                          sed == 0 ? c->d_heat_thick : c->d_sed_tab[sed - 1][2], sed == 0 ? c->d_heat_thin : c->d_sed_tab[sed - 1][3]};
  const bool have = sed == 0 ? c->have_tables : c->have_sed[sed - 1];
  const bool heat = sed == 0 ? c->have_heat_tables : c->have_sed_heat[sed - 1];
  for (int b = 0; b < NFREQ; b++) c->h_bands.tau_zero[sed][b] = (double)INFINITY;
  if (have) {
    std::vector<double> h[4];
    const int ncol[4] = {NFREQ, NFREQ, NHEAT, NHEAT};
    for (int t = 0; t < (heat ? 4 : 2); t++) {
      h[t].resize((size_t)ncol[t] * NTAUP);
      HIPCHK(c, hipMemcpy(h[t].data(), tab[t], sizeof(double) * h[t].size(), hipMemcpyDeviceToHost));
    }
    for (int b = 0; b < NFREQ; b++) {
      const double *cols[8];
      int n = 0;
      cols[n++] = &h[0][(size_t)b * NTAUP];
      cols[n++] = &h[1][(size_t)b * NTAUP];
      if (heat) {
        const int nh = b < NB1 ? 1 : (b < NB1 + NB2 ? 2 : 3);
        const int c0 = b < NB1 ? 0 : (b < NB1 + NB2 ? 2 * (b + 1) - NB1 - 2 : 3 * (b + 1) - NB2 - 2 * NB1 - 3);
        for (int k = 0; k < nh; k++) {
          cols[n++] = &h[2][(size_t)(c0 + k) * NTAUP];
          cols[n++] = &h[3][(size_t)(c0 + k) * NTAUP];
        }
      }
      c->h_bands.tau_zero[sed][b] = band_tau_zero(cols, n);
    }
    if (heat) { // the copies the kernels read (same numbers, woven by band)
      std::vector<double> woven((size_t)NHEAT * NTAUP);
      for (int t = 0; t < 2; t++) {
        heat_interleave(h[2 + t].data(), woven.data());
        if (!c->d_heat_woven[sed][t]) HIPCHK(c, hipMalloc(&c->d_heat_woven[sed][t], sizeof(double) * woven.size()));
        HIPCHK(c, hipMemcpy(c->d_heat_woven[sed][t], woven.data(), sizeof(double) * woven.size(), hipMemcpyHostToDevice));
      }
    }
  }
  if (sed == 0 && have) { // every writer of d_photo_thick ends here: its pair copy for the gathers-first readers
    if (!c->d_photo_pairs) HIPCHK(c, hipMalloc(&c->d_photo_pairs, sizeof(TablePair) * table_pair_index(NFREQ, 0)));
    hipLaunchKernelGGL(k_table_pairs, dim3((NTAUP + BLOCK - 1) / BLOCK, NFREQ), dim3(BLOCK), 0, c->stream, c->d_photo_thick, c->d_photo_pairs);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (c->have_bands) {
    band_rows_fill(c->h_bands);
    HIPCHK(c, hipMemcpy(c->d_bands, &c->h_bands, sizeof(BandDataByRow), hipMemcpyHostToDevice));
  }
  return 0;
}

static int set_tables_one(c2r_ctx *c, const double *photo_thick, const double *photo_thin,
                              const double *heat_thick, const double *heat_thin, const double *sigma_HI,
                              const double *sigma_HeI, const double *sigma_HeII, const double *const fvec[12],
                              int bb_upper) {
  if (!c) return 1;
  if (!sigma_HI || !sigma_HeI || !sigma_HeII) return fail(c, "c2r_set_tables: the cross sections are required");
  if ((photo_thick == nullptr) != (photo_thin == nullptr) || (heat_thick == nullptr) != (heat_thin == nullptr))
    return fail(c, "c2r_set_tables: thick and thin tables come in pairs");
  if (bb_upper < 1 || bb_upper > NFREQ) return fail(c, "c2r_set_tables: bb_upper %d not in [1,%d]", bb_upper, NFREQ);
  // The band loop of the rates kernels leaves out the terms of species that cannot absorb in a band and takes
  // the reciprocals of scale_int2/3 without operand scaling: both rest on the band layout of
  // radiation_sizes.f90:375-545 (sigma_HeI = 0 below the He I threshold, sigma_HeII = 0 below the He II
  // threshold, every other cross section an ordinary number), checked here once.
  for (int b = 0; b < NFREQ; b++) {
    const double lo = 0x1p-100, hi = 0x1p-30;
    const bool he1 = b >= NB1, he2 = b >= NB1 + NB2;
    const bool ok = sigma_HI[b] >= lo && sigma_HI[b] <= hi &&
                    (he1 ? (sigma_HeI[b] >= lo && sigma_HeI[b] <= hi) : sigma_HeI[b] == 0.0) &&
                    (he2 ? (sigma_HeII[b] >= lo && sigma_HeII[b] <= hi) : sigma_HeII[b] == 0.0);
    if (!ok)
      return fail(c, "c2r_set_tables: band %d has cross sections (%g, %g, %g): not the band layout of radiation_sizes.f90 "
                  "(He I / He II cross sections exactly 0 below their thresholds, all others within [2^-100, 2^-30])",
                  b + 1, sigma_HI[b], sigma_HeI[b], sigma_HeII[b]);
  }
  HIPCHK(c, hipSetDevice(c->device));
  // without tables this call only sets the band vectors; c2r_build_tables makes the tables on the device
  c->have_tables = false;
  if (photo_thick) {
    if (upload_table(c, photo_thick, NFREQ, &c->d_photo_thick)) return 1;
    if (upload_table(c, photo_thin, NFREQ, &c->d_photo_thin)) return 1;
    c->have_tables = true;
  }
  c->have_heat_tables = false;
  c->have_fvec = false;
  BandData bd;
  std::memset(&bd, 0, sizeof bd);
  std::memcpy(bd.sigma_HI, sigma_HI, sizeof bd.sigma_HI);
  std::memcpy(bd.sigma_HeI, sigma_HeI, sizeof bd.sigma_HeI);
  std::memcpy(bd.sigma_HeII, sigma_HeII, sizeof bd.sigma_HeII);
  bd.bb_upper = bb_upper;
  if (heat_thick && !fvec) return fail(c, "c2r_set_tables: heat tables given without the secondary-ionisation vectors");
  if (fvec) {
    for (int i = 0; i < 12; i++)
      if (!fvec[i]) return fail(c, "c2r_set_tables: fvec[%d] is NULL", i);
    if (heat_thick) {
      if (upload_table(c, heat_thick, NHEAT, &c->d_heat_thick)) return 1;
      if (upload_table(c, heat_thin, NHEAT, &c->d_heat_thin)) return 1;
    }
    double *dst[12] = {bd.f1ion_HI, bd.f1ion_HeI, bd.f1ion_HeII, bd.f2ion_HI, bd.f2ion_HeI, bd.f2ion_HeII,
                       bd.f1heat_HI, bd.f1heat_HeI, bd.f1heat_HeII, bd.f2heat_HI, bd.f2heat_HeI, bd.f2heat_HeII};
    for (int i = 0; i < 12; i++) std::memcpy(dst[i], fvec[i], sizeof(double) * (NFREQ - 1));
    c->have_fvec = true;
    c->have_heat_tables = heat_thick != nullptr;
  }
  for (int sd = 0; sd < 3; sd++) // the other SEDs keep theirs
    std::memcpy(bd.tau_zero[sd], c->h_bands.tau_zero[sd], sizeof bd.tau_zero[sd]);
  if (!c->have_bands)
    for (int sd = 0; sd < 3; sd++)
      for (int b = 0; b < NFREQ; b++) bd.tau_zero[sd][b] = (double)INFINITY;
  static_cast<BandData &>(c->h_bands) = bd;
  c->bb_upper = bb_upper;
  c->have_bands = true;
  return refresh_tau_zero(c, 0); // uploads the band data too
}

static int set_cooling_one(c2r_ctx *c, const double *cool, double mintemp, double dtemp) {
  if (!c) return 1;
  if (!cool || !(dtemp > 0.0)) return fail(c, "c2r_set_cooling: bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->d_cool) HIPCHK(c, hipMalloc(&c->d_cool, sizeof(double) * 5 * NCOOL));
  HIPCHK(c, hipMemcpy(c->d_cool, cool, sizeof(double) * 5 * NCOOL, hipMemcpyHostToDevice));
  c->cool_mintemp = mintemp;
  c->cool_dtemp = dtemp;
  c->have_cool = true;
  return 0;
}

// The lists of the heating tiers (cells dropped by a launch, redone by the next) and their counters: made when a step
// is declared non-isothermal (c2r_set_step), zeroed on the stream their first user follows.
static int alloc_heating_lists(c2r_ctx *c) {
  if (c->isothermal || (c->d_defer[0] && c->d_defer[1] && c->d_chemctl)) return 0;
  // all three or none: an allocation that fails half-way (out of memory) gives back what it got, so that the next
  // c2r_set_step tries again instead of finding "the lists exist" with a null pointer among them (round-4 ADVICE)
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && e == hipSuccess; k++)
    if (!c->d_defer[k]) e = hipMalloc(&c->d_defer[k], sizeof(int) * c->g.ncell);
  if (e == hipSuccess && !c->d_chemctl) e = hipMalloc(&c->d_chemctl, sizeof(int) * (4 + CHEM_HIST)); // two list counts, then the histogram
  if (e == hipSuccess) e = hipMemsetAsync(c->d_chemctl, 0, sizeof(int) * (4 + CHEM_HIST), c->stream);
  if (e != hipSuccess) {
    for (int k = 0; k < 2; k++) {
      if (c->d_defer[k]) (void)hipFree(c->d_defer[k]);
      c->d_defer[k] = nullptr;
    }
    if (c->d_chemctl) (void)hipFree(c->d_chemctl);
    c->d_chemctl = nullptr;
    (void)hipGetLastError();
    return fail(c, "c2r_set_step: the lists of the heating global pass could not be allocated: %s", hipGetErrorString(e));
  }
  return 0;
}

static int set_step_one(c2r_ctx *c, const double *ndens, const double dr[3], double vol, float clumping,
                            double zred, double H0, double Omega0, int isothermal, double temper_val,
                            const double reccoef[12]) {
  if (!c) return 1;
  if (!dr || !reccoef) return fail(c, "c2r_set_step: null argument");
  // ndens == nullptr (c2r_set_step_scalars): the density on the device stays as it is
  if (!ndens && !c->have_step) return fail(c, "c2r_set_step_scalars: no density on the device yet (c2r_set_step comes first)");
  HIPCHK(c, hipSetDevice(c->device));
  if (ndens) HIPCHK(c, hipMemcpyAsync(c->d_ndens, ndens, sizeof(double) * c->g.ncell, hipMemcpyHostToDevice, c->stream));
  c->isothermal = isothermal ? 1 : 0;
  if (alloc_heating_lists(c)) return 1; // a non-isothermal step: the tiers' lists exist before any pass starts
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->sc.dr1 = dr[0]; c->sc.dr2 = dr[1]; c->sc.dr3 = dr[2]; c->sc.vol = vol;
  c->sc.clumping = (double)clumping;
  c->sc.temper_val = temper_val;
  std::memcpy(&c->sc.rc, reccoef, sizeof(double) * 12);
  c->zred = zred; c->H0 = H0; c->Omega0 = Omega0;
  c->have_step = true;
  c->packed_valid = c->transposed_valid = false; // ndens may have changed
  return 0;
}

// horizon loss (c2r_enable_horizon_loss): other sources, other horizons or other boundaries -- the values start at 0.0 again,
// one per source of the list in force, and the terms of the source swept last are nobody's
static void forget_horizon_loss(c2r_ctx *c) {
  if (c->rim_on) c->horizon_loss.assign((size_t)c->nsrc, 0.0);
  c->rim_last_ns = 0;
  c->rim_last_stamp = 0;
}

// Point-source hand-over (c2ray_handover.inc): a new source list drops the entry columns and the exit selections, as it drops
// the beams.  The strips are read by launches of the sweep stream only.
static int forget_source_handover(c2r_ctx *c) {
  bool any = !c->src_entry.empty();
  for (const c2r_ctx::FaceExit &x : c->face_exit) any = any || !x.sources.empty();
  if (!any) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (c2r_ctx::FaceEntry &e : c->src_entry)
    if (e.d_cols) HIPCHK(c, hipFree(e.d_cols));
  c->src_entry.clear();
  for (c2r_ctx::FaceExit &x : c->face_exit) {
    if (x.d_cols) HIPCHK(c, hipFree(x.d_cols));
    x = c2r_ctx::FaceExit();
  }
  return 0;
}

// Sources outside the mesh (c2r_set_sources_external).  Does the position p stand outside along axis d?
static bool position_is_external(const Grid &g, const int *p, int d) {
  const int mesh[3] = {g.n1, g.n2, g.n3};
  return p[d] < 1 || p[d] > mesh[d];
}
static bool axis_is_external(const c2r_ctx *c, int ns, int d) { return position_is_external(c->g, &c->srcpos[3 * (size_t)(ns - 1)], d); }
static bool source_is_external(const c2r_ctx *c, int ns) {
  return axis_is_external(c, ns, 0) || axis_is_external(c, ns, 1) || axis_is_external(c, ns, 2);
}
// the largest shell within the reach of a source of the list that stands outside the mesh (0: there is none)
static int external_smax(const c2r_ctx *c, int nsrc, const int *srcpos) {
  const int mesh[3] = {c->g.n1, c->g.n2, c->g.n3};
  int m = 0;
  for (int s = 0; s < nsrc; s++) {
    const int *p = srcpos + 3 * (size_t)s;
    if (!(position_is_external(c->g, p, 0) || position_is_external(c->g, p, 1) || position_is_external(c->g, p, 2))) continue;
    for (int d = 0; d < 3; d++) {
      int l, r;
      axis_reach_external(mesh[d], p[d], c->per[d], MAX_SUBBOX, l, r);
      m = std::max(m, std::max(-l, r));
    }
  }
  return m;
}

// The shell bookkeeping for the boundaries and the source list in force, and the device buffers sized by it.  The caller has
// made sure that nothing queued still reads them.
static int remake_shell_buffers(c2r_ctx *c) {
  shell_bookkeeping(c);
  HIPCHK(c, hipFree(c->d_block_base));
  c->d_block_base = nullptr;
  HIPCHK(c, hipMalloc(&c->d_block_base, sizeof(int) * c->block_base.size()));
  HIPCHK(c, hipMemcpy(c->d_block_base, c->block_base.data(), sizeof(int) * c->block_base.size(), hipMemcpyHostToDevice));
  for (int k = 0; k < 2; k++) {
    HIPCHK(c, hipFree(c->d_list[k]));
    HIPCHK(c, hipHostFree(c->h_list[k]));
    c->d_list[k] = c->h_list[k] = nullptr;
    HIPCHK(c, hipMalloc(&c->d_list[k], sizeof(int) * c->list_cap));
    HIPCHK(c, hipHostMalloc(&c->h_list[k], sizeof(int) * c->list_cap));
  }
  return 0;
}

// external: c2r_set_sources_external -- a position may lie outside the mesh along axes that are open; everything is checked
// before anything is kept
static int set_sources_one(c2r_ctx *c, int nsrc, const int *srcpos, const double *normflux, double s_star, bool external = false) {
  if (!c) return 1;
  const char *who = external ? "c2r_set_sources_external" : "c2r_set_sources";
  if (nsrc < 0 || (nsrc > 0 && (!srcpos || !normflux))) return fail(c, "%s: bad arguments", who);
  const int mesh[3] = {c->g.n1, c->g.n2, c->g.n3};
  bool any_external = false;
  for (int s = 0; s < nsrc; s++) {
    const int *p = srcpos + 3 * s;
    const bool out[3] = {position_is_external(c->g, p, 0), position_is_external(c->g, p, 1), position_is_external(c->g, p, 2)};
    if (!(out[0] || out[1] || out[2])) continue;
    if (!external) return fail(c, "c2r_set_sources: source %d at (%d,%d,%d) outside the mesh", s + 1, p[0], p[1], p[2]);
    any_external = true;
    int l[3], r[3];
    for (int d = 0; d < 3; d++) {
      if (out[d] && c->per[d])
        return fail(c, "c2r_set_sources_external: source %d at (%d,%d,%d) stands outside the mesh along axis %d, which is periodic "
                    "(c2r_set_boundaries_axes opens an axis)", s + 1, p[0], p[1], p[2], d);
      axis_reach_external(mesh[d], p[d], c->per[d], MAX_SUBBOX, l[d], r[d]);
      // a reach clamped at max_subbox that ends before the mesh begins: no box of this source ever holds a mesh cell, and a
      // pass would sweep up to (max_subbox + 1)^3 cells of vacuum for nothing
      if (out[d] && (p[d] < 1 ? 1 - p[d] : p[d] - mesh[d]) > MAX_SUBBOX)
        return fail(c, "c2r_set_sources_external: source %d at (%d,%d,%d) stands more than max_subbox = %d cells from the mesh along "
                    "axis %d: its sub-boxes never reach a mesh cell", s + 1, p[0], p[1], p[2], MAX_SUBBOX, d);
    }
    const int refusal = external_reach_refusal(l, r);
    if (refusal == 1)
      return fail(c, "c2r_set_sources_external: source %d at (%d,%d,%d) reaches over (%d..%d, %d..%d, %d..%d), more than %d cells to "
                  "one side", s + 1, p[0], p[1], p[2], l[0], r[0], l[1], r[1], l[2], r[2], EXTERNAL_REACH_MAX);
    if (refusal == 2)
      return fail(c, "c2r_set_sources_external: source %d at (%d,%d,%d) reaches over (%d..%d, %d..%d, %d..%d), 2^31 cells or more",
                  s + 1, p[0], p[1], p[2], l[0], r[0], l[1], r[1], l[2], r[2]);
  }
  // What is indexed by mesh faces and mesh cells is not built for a source outside the mesh.
  if (any_external && c->face_on)
    return fail(c, "c2r_set_sources_external: the escape maps are on (c2r_enable_face_loss), which are not built for sources outside the mesh");
  if (any_external && c->rim_on)
    return fail(c, "c2r_set_sources_external: the horizon loss is on (c2r_enable_horizon_loss), which is not built for sources outside the mesh");
  const int ext_smax = external ? external_smax(c, nsrc, srcpos) : 0;
  if (ext_smax != c->ext_smax) {
    // the shell bookkeeping changes size: nothing queued may still read it, and no pass may be open
    if (c->pass_open)
      return fail(c, "%s: a pass opened by c2r_pass_sources_begin is still open (close it with c2r_pass_sources_end first)", who);
    if (shell_blocks_upto(std::max(ext_smax, c->g.smax)) > (long long)INT32_MAX)
      return fail(c, "internal: %s: the blocks of the shells 0..%d do not fit 32 bits", who, ext_smax);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream2));
    HIPCHK(c, hipStreamSynchronize(c->stream3));
    HIPCHK(c, hipStreamSynchronize(c->stream_probe));
    c->ext_smax = ext_smax;
    if (remake_shell_buffers(c)) return 1;
  } else if (external && c->pass_open) {
    return fail(c, "c2r_set_sources_external: a pass opened by c2r_pass_sources_begin is still open (close it with c2r_pass_sources_end first)");
  }
  // What the last pass learnt about each source -- how many sub-boxes it needed: the size of its column block and the
  // rounds that are swept without waiting for a loss probe -- stays valid across time steps as long as the source list
  // is the same (the reference's driver passes the same list at every evolve3D call of a redshift slice); a wrong
  // guess costs time, never a bit (tests/test_gpu_step_sequence.py holds it to that: gas that turns opaque or transparent
  // under learnt counts, a new source on a cell with a count).  Forgetting it made every evolve3D call after the first
  // regrow its column blocks and probe every round again: 2.7 ms per iteration over the 8-9 iterations of such a call
  // (round 3's dropin timing: 26.0 against 23.1 ms).
  const bool same_list = nsrc == c->nsrc && c->srcpos.size() == 3 * (size_t)nsrc &&
                         std::equal(srcpos, srcpos + 3 * (size_t)nsrc, c->srcpos.begin());
  if (!same_list) {
    // another list (the next redshift slice: sources appear, disappear, change places in the list): what is known about a
    // cell's source goes with the cell.  Sources that share a cell share the larger count.
    // (the key: three 21-bit fields, each position biased by 2^20 -- a source outside the mesh may stand at a position <= 0;
    // one beyond the fields, which no box of MAX_SUBBOX cells brings to the mesh, carries nothing over)
    constexpr long long KEY_BIAS = 1LL << 20, KEY_SPAN = 1LL << 21;
    auto key = [&](const int *p, long long &k) {
      k = 0;
      for (int d = 2; d >= 0; d--) {
        const long long v = (long long)p[d] + KEY_BIAS;
        if (v < 0 || v >= KEY_SPAN) return false;
        k = k * KEY_SPAN + v;
      }
      return true;
    };
    std::unordered_map<long long, int> known;
    if (c->prev_nbox.size() == (size_t)c->nsrc && c->srcpos.size() == 3 * (size_t)c->nsrc)
      for (int s = 0; s < c->nsrc; s++) {
        const int *p = &c->srcpos[3 * (size_t)s];
        long long k;
        if (!key(p, k)) continue;
        int &v = known[k];
        v = std::max(v, c->prev_nbox[(size_t)s]);
      }
    std::vector<int> carried((size_t)nsrc, 0);
    for (int s = 0; s < nsrc; s++) {
      const int *p = srcpos + 3 * (size_t)s;
      long long k;
      if (!key(p, k)) continue;
      const auto it = known.find(k);
      if (it != known.end()) carried[(size_t)s] = it->second;
    }
    c->prev_nbox.swap(carried);
    c->trace.clear(); // (c2r_get_source_trace: nothing has been swept of the new list)
    c->trace_stamp.clear();
  }
  c->nsrc = nsrc;
  if (c->prev_nbox.size() != (size_t)nsrc) c->prev_nbox.assign((size_t)nsrc, 0);
  c->srcpos.assign(srcpos, srcpos + 3 * (size_t)nsrc);
  c->normflux.assign(normflux, normflux + nsrc);
  c->s_star = s_star;
  c->normflux_sed[0].clear();
  c->normflux_sed[1].clear();
  c->beams.clear();
  c->beam_k.clear();
  c->horizons.clear();
  c->horizon_r2.clear();
  c->curves.clear();
  forget_horizon_loss(c);
  return forget_source_handover(c);
}

static int set_sed_tables_one(c2r_ctx *c, int sed, const double *photo_thick, const double *photo_thin,
                                  const double *heat_thick, const double *heat_thin, int lower, int upper) {
  if (!c) return 1;
  if (sed < 1 || sed > 2) return fail(c, "c2r_set_sed_tables: sed = %d, expected 1 (power law) or 2 (quasar)", sed);
  if (lower < 1 || upper > NFREQ || lower > upper)
    return fail(c, "c2r_set_sed_tables: band range %d..%d not inside 1..%d", lower, upper, NFREQ);
  HIPCHK(c, hipSetDevice(c->device));
  const int k = sed - 1;
  c->have_sed[k] = false;
  c->have_sed_heat[k] = false;
  c->sed_lo[k] = lower - 1;
  c->sed_hi[k] = upper;
  c->have_sed_limits[k] = true;
  if (!photo_thick && !photo_thin) return 0; // band range only: c2r_build_tables makes the tables
  if (!photo_thick || !photo_thin) return fail(c, "c2r_set_sed_tables: thick and thin tables come in pairs");
  if (upload_table(c, photo_thick, NFREQ, &c->d_sed_tab[k][0])) return 1;
  if (upload_table(c, photo_thin, NFREQ, &c->d_sed_tab[k][1])) return 1;
  if (heat_thick && heat_thin) {
    if (upload_table(c, heat_thick, NHEAT, &c->d_sed_tab[k][2])) return 1;
    if (upload_table(c, heat_thin, NHEAT, &c->d_sed_tab[k][3])) return 1;
    c->have_sed_heat[k] = true;
  }
  c->sed_lo[k] = lower - 1;
  c->sed_hi[k] = upper;
  c->have_sed[k] = true;
  return refresh_tau_zero(c, sed);
}

static int set_sources_sed_one(c2r_ctx *c, int sed, const double *normflux, double s_star) {
  if (!c) return 1;
  if (sed < 1 || sed > 2) return fail(c, "c2r_set_sources_sed: sed = %d, expected 1 or 2", sed);
  const int k = sed - 1;
  if (!normflux) { c->normflux_sed[k].clear(); return 0; }
  if (!c->have_sed[k]) return fail(c, "c2r_set_sources_sed: c2r_set_sed_tables(%d) has not been called", sed);
  c->normflux_sed[k].assign(normflux, normflux + c->nsrc);
  c->s_star_sed[k] = s_star;
  return 0;
}

// c2r_set_source_beams on one device: everything is checked before anything is kept
static int set_source_beams_one(c2r_ctx *c, int nsrc, const c2r_source_beam *beams) {
  if (!c) return 1;
  if (c->pass_open) return fail(c, "c2r_set_source_beams: a pass opened by c2r_pass_sources_begin is still open");
  if (nsrc != c->nsrc) return fail(c, "c2r_set_source_beams: nsrc = %d, but c2r_set_sources gave %d sources", nsrc, c->nsrc);
  if (!beams) {
    c->beams.clear();
    c->beam_k.clear();
    return 0;
  }
  std::vector<double> k((size_t)nsrc, 0.0);
  for (int s = 0; s < nsrc; s++) {
    const c2r_source_beam &b = beams[s];
    if (b.kind < BEAM_NONE || b.kind > BEAM_BICONE)
      return fail(c, "c2r_set_source_beams: source %d: kind = %d, expected 0 (none), 1 (cone) or 2 (bicone)", s + 1, b.kind);
    if (b.kind == BEAM_NONE) continue;
    if (!std::isfinite(b.axis[0]) || !std::isfinite(b.axis[1]) || !std::isfinite(b.axis[2]))
      return fail(c, "c2r_set_source_beams: source %d: axis (%g, %g, %g) is not finite", s + 1, b.axis[0], b.axis[1], b.axis[2]);
    const double a2 = (b.axis[0] * b.axis[0] + b.axis[1] * b.axis[1]) + b.axis[2] * b.axis[2];
    if (!std::isnormal(a2))
      return fail(c, "c2r_set_source_beams: source %d: the squared length %g of axis (%g, %g, %g) is zero or not a normal finite number",
                  s + 1, a2, b.axis[0], b.axis[1], b.axis[2]);
    if (!std::isfinite(b.cos_half) || b.cos_half < 0.0 || b.cos_half > 1.0)
      return fail(c, "c2r_set_source_beams: source %d: cos_half = %g is not in [0, 1]", s + 1, b.cos_half);
    k[(size_t)s] = beam_K(b.cos_half, b.axis[0], b.axis[1], b.axis[2]);
  }
  c->beams.assign(beams, beams + nsrc);
  c->beam_k.swap(k);
  return 0;
}

// c2r_set_source_horizons on one device: everything is checked before anything is kept
static int set_source_horizons_one(c2r_ctx *c, int nsrc, const double *radius) {
  if (!c) return 1;
  if (c->pass_open) return fail(c, "c2r_set_source_horizons: a pass opened by c2r_pass_sources_begin is still open");
  if (nsrc != c->nsrc) return fail(c, "c2r_set_source_horizons: nsrc = %d, but c2r_set_sources gave %d sources", nsrc, c->nsrc);
  if (!radius) {
    c->horizons.clear();
    c->horizon_r2.clear();
    forget_horizon_loss(c);
    return 0;
  }
  std::vector<double> r2((size_t)nsrc);
  for (int s = 0; s < nsrc; s++) {
    if (!(radius[s] >= 0.0)) // (a NaN fails every comparison)
      return fail(c, "c2r_set_source_horizons: source %d: radius = %g is negative or not a number", s + 1, radius[s]);
    r2[(size_t)s] = horizon_R2(radius[s]);
  }
  c->horizons.assign(radius, radius + nsrc);
  c->horizon_r2.swap(r2);
  forget_horizon_loss(c);
  return 0;
}

// a curve that leaves the source as it is: no step, factor 1.0
static bool curve_is_none(const c2r_source_curve &v) { return v.nstep == 0 && v.factor[0] == 1.0; }

// c2r_set_source_curves on one device: everything is checked before anything is kept
static int set_source_curves_one(c2r_ctx *c, int nsrc, const c2r_source_curve *curves) {
  if (!c) return 1;
  if (c->pass_open) return fail(c, "c2r_set_source_curves: a pass opened by c2r_pass_sources_begin is still open");
  if (nsrc != c->nsrc) return fail(c, "c2r_set_source_curves: nsrc = %d, but c2r_set_sources gave %d sources", nsrc, c->nsrc);
  if (!curves) {
    c->curves.clear();
    return 0;
  }
  std::vector<c2r_source_curve> kept((size_t)nsrc);
  for (int s = 0; s < nsrc; s++) {
    const c2r_source_curve &v = curves[s];
    if (v.nstep < 0 || v.nstep > C2R_CURVE_MAX_STEPS)
      return fail(c, "c2r_set_source_curves: source %d: nstep = %d not in [0,%d]", s + 1, v.nstep, C2R_CURVE_MAX_STEPS);
    for (int k = 0; k < v.nstep; k++) {
      if (!(v.radius[k] >= 0.0) || !std::isfinite(v.radius[k])) // (a NaN fails every comparison)
        return fail(c, "c2r_set_source_curves: source %d: radius[%d] = %g is negative or not finite", s + 1, k, v.radius[k]);
      if (k > 0 && !(v.radius[k] > v.radius[k - 1]))
        return fail(c, "c2r_set_source_curves: source %d: radius[%d] = %g is not above radius[%d] = %g", s + 1, k, v.radius[k], k - 1,
                    v.radius[k - 1]);
    }
    for (int k = 0; k <= v.nstep; k++)
      if (!(v.factor[k] >= 0.0) || !std::isfinite(v.factor[k]))
        return fail(c, "c2r_set_source_curves: source %d: factor[%d] = %g is negative or not finite", s + 1, k, v.factor[k]);
    // an all-zero record is a record nobody filled in, not a source that has gone dark (that is {1, {0.0}, {0.0, 0.0}})
    if (v.nstep == 0 && v.factor[0] == 0.0)
      return fail(c, "c2r_set_source_curves: source %d: nstep = 0 and factor[0] = 0 (a zeroed record); no curve is factor[0] = 1", s + 1);
    c2r_source_curve &o = kept[(size_t)s];
    o = c2r_source_curve{};
    o.nstep = v.nstep;
    for (int k = 0; k < v.nstep; k++) o.radius[k] = v.radius[k];
    for (int k = 0; k <= v.nstep; k++) o.factor[k] = v.factor[k];
  }
  c->curves.swap(kept);
  return 0;
}

// the beam, the horizon and the curve of source ns (1-based) in its device record
static void source_cut(const c2r_ctx *c, int ns, SrcDev &S) {
  S.cut = CUT_NONE;
  S.bax = S.bay = S.baz = S.bK = 0.0;
  S.hR2 = INFINITY;
  if (!c->beams.empty()) {
    const c2r_source_beam &b = c->beams[(size_t)ns - 1];
    if (b.kind != BEAM_NONE) {
      S.cut = b.kind;
      S.bax = b.axis[0]; S.bay = b.axis[1]; S.baz = b.axis[2];
      S.bK = c->beam_k[(size_t)ns - 1];
    }
  }
  // (+infinity as given: no horizon.  A finite radius whose square overflows keeps its flag: every cell is within, asked)
  if (!c->horizons.empty() && std::isfinite(c->horizons[(size_t)ns - 1])) {
    S.cut |= CUT_HORIZON;
    S.hR2 = c->horizon_r2[(size_t)ns - 1];
  }
  const c2r_source_curve none = {0, {}, {1.0}};
  const c2r_source_curve &v = c->curves.empty() ? none : c->curves[(size_t)ns - 1];
  curve_fill(v.nstep, v.radius, v.factor, S.cR2, S.cfac);
  if (!curve_is_none(v)) S.cut |= CUT_CURVE;
}

// The per-frequency vectors of k_build_tables, with the host versions of the bit-exact exp / pow:
// set_frequency_array, set_cross_section_freq_dependence and the tau-independent factors of
// fill_photo_integrands / fill_heating_integrands_* (radiation_tables.f90:432-783).
static void build_sed_vectors(const c2r_sed_setup &S, std::vector<double> &v) {
  v.assign((size_t)6 * SEDV, 0.0);
  double *csfd = v.data(), *A = csfd + SEDV, *D = A + SEDV, *H0 = D + SEDV, *H1 = H0 + SEDV, *H2 = H1 + SEDV;
  for (int b = 0; b < NFREQ; b++) {
    const double fmin = S.freq_min[b], df = S.delta_freq[b];
    for (int x = 0; x <= 512; x++) {
      const size_t q = (size_t)b * 513 + x;
      const double freq = fmin + df * (double)(float)x;
      csfd[q] = C2R_MATH_POW(freq / fmin, -S.xsec_index[b]);
      if (S.sed == 0) {
        if (freq * S.h_over_kT < 700.0) { // :474; otherwise the integrand is 0: A = 0, D = 1
          A[q] = 4.0 * S.pi * S.R_star2 * S.two_pi_over_c_square * freq * freq;
          D[q] = C2R_MATH_EXP(freq * S.h_over_kT) - 1.0;
        } else {
          A[q] = 0.0;
          D[q] = 1.0;
        }
      } else {
        A[q] = S.pl_scaling * C2R_MATH_POW(freq, -S.pl_index);
        D[q] = 1.0; // x / 1.0 == x
      }
      H0[q] = S.hplanck * (freq - S.ion_freq_HI);
      H1[q] = S.hplanck * (freq - S.ion_freq_HeI);
      H2[q] = S.hplanck * (freq - S.ion_freq_HeII);
    }
  }
}

static int build_tables_one(c2r_ctx *c, const c2r_sed_setup *S, int with_heat) {
  if (!c || !S) return 1;
  if (S->nfreq != 512) return fail(c, "c2r_build_tables: nfreq = %d, the band set-up is for NumFreq = 512", S->nfreq);
  if (S->sed < 0 || S->sed > 2) return fail(c, "c2r_build_tables: sed = %d, expected 0 (black body), 1 (power law), 2 (quasar)", S->sed);
  if (!S->freq_min || !S->delta_freq || !S->xsec_index || !S->tau || !S->romw) return fail(c, "c2r_build_tables: null vector");
  if (S->sed == 0 && !c->have_bands) return fail(c, "c2r_build_tables: c2r_set_tables (band vectors) has not been called");
  if (S->sed > 0 && !c->have_sed_limits[S->sed - 1]) return fail(c, "c2r_build_tables: c2r_set_sed_tables(%d) (band range) has not been called", S->sed);
  if (S->sed == 0 && with_heat && !c->have_fvec) return fail(c, "c2r_build_tables: heating tables need the secondary-ionisation vectors of c2r_set_tables");
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<double> v;
  build_sed_vectors(*S, v);
  struct DevBuf { // freed on every way out, the error returns included
    double *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
  } buf_v, buf_small;
  HIPCHK(c, hipMalloc(&buf_v.p, sizeof(double) * v.size()));
  HIPCHK(c, hipMalloc(&buf_small.p, sizeof(double) * (NTAU + 1 + 513 + NFREQ)));
  double *d_v = buf_v.p, *d_small = buf_small.p;
  HIPCHK(c, hipMemcpy(d_v, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(d_small, S->tau, sizeof(double) * (NTAU + 1), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(d_small + NTAU + 1, S->romw, sizeof(double) * 513, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(d_small + NTAU + 1 + 513, S->delta_freq, sizeof(double) * NFREQ, hipMemcpyHostToDevice));
  double **tab = S->sed == 0 ? nullptr : c->d_sed_tab[S->sed - 1];
  double **pt = S->sed == 0 ? &c->d_photo_thick : &tab[0], **pn = S->sed == 0 ? &c->d_photo_thin : &tab[1];
  double **ht = S->sed == 0 ? &c->d_heat_thick : &tab[2], **hn = S->sed == 0 ? &c->d_heat_thin : &tab[3];
  if (!*pt) HIPCHK(c, hipMalloc(pt, sizeof(double) * (size_t)NFREQ * NTAUP));
  if (!*pn) HIPCHK(c, hipMalloc(pn, sizeof(double) * (size_t)NFREQ * NTAUP));
  if (with_heat) {
    if (!*ht) HIPCHK(c, hipMalloc(ht, sizeof(double) * (size_t)NHEAT * NTAUP));
    if (!*hn) HIPCHK(c, hipMalloc(hn, sizeof(double) * (size_t)NHEAT * NTAUP));
  }
  hipLaunchKernelGGL(k_build_tables, dim3((NTAU + 1 + BLOCK - 1) / BLOCK, 2 * NFREQ), dim3(BLOCK), 0, c->stream, d_v,
                     d_small, d_small + NTAU + 1, d_small + NTAU + 1 + 513, with_heat ? 1 : 0, *pt, *pn,
                     with_heat ? *ht : nullptr, with_heat ? *hn : nullptr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (S->sed == 0) {
    c->have_tables = true;
    c->have_heat_tables = with_heat != 0;
  } else {
    c->have_sed[S->sed - 1] = true;
    c->have_sed_heat[S->sed - 1] = with_heat != 0;
  }
  return refresh_tau_zero(c, S->sed);
}

extern "C" int c2r_download_tables(c2r_ctx *c, int sed, double *photo_thick, double *photo_thin, double *heat_thick,
                                   double *heat_thin) {
  if (!c) return 1;
  if (sed < 0 || sed > 2) return fail(c, "c2r_download_tables: sed = %d", sed);
  HIPCHK(c, hipSetDevice(c->device));
  const bool have = sed == 0 ? c->have_tables : c->have_sed[sed - 1];
  const bool have_heat = sed == 0 ? c->have_heat_tables : c->have_sed_heat[sed - 1];
  if (!have) return fail(c, "c2r_download_tables: SED %d has no tables", sed);
  if ((heat_thick || heat_thin) && !have_heat) return fail(c, "c2r_download_tables: SED %d has no heating tables", sed);
  const double *src[4] = {sed == 0 ? c->d_photo_thick : c->d_sed_tab[sed - 1][0], sed == 0 ? c->d_photo_thin : c->d_sed_tab[sed - 1][1],
                          sed == 0 ? c->d_heat_thick : c->d_sed_tab[sed - 1][2], sed == 0 ? c->d_heat_thin : c->d_sed_tab[sed - 1][3]};
  double *dst[4] = {photo_thick, photo_thin, heat_thick, heat_thin};
  const int ncol[4] = {NFREQ, NFREQ, NHEAT, NHEAT};
  for (int t = 0; t < 4; t++) {
    if (!dst[t]) continue;
    std::vector<double> tmp((size_t)ncol[t] * NTAUP);
    HIPCHK(c, hipMemcpy(tmp.data(), src[t], sizeof(double) * tmp.size(), hipMemcpyDeviceToHost));
    for (int col = 0; col < ncol[t]; col++)
      std::memcpy(dst[t] + (size_t)col * (NTAU + 1), tmp.data() + (size_t)col * NTAUP, sizeof(double) * (NTAU + 1));
  }
  return 0;
}

static int set_lls_one(c2r_ctx *c, int use_lls, double coldensh_lls, const float *lls_grid) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  c->sc.use_lls = use_lls ? 1 : 0;
  c->sc.coldensh_lls = coldensh_lls;
  c->lls_on_grid = false;
  if (use_lls && lls_grid) {
    if (!c->d_lls) HIPCHK(c, hipMalloc(&c->d_lls, sizeof(float) * c->g.ncell));
    HIPCHK(c, hipMemcpyAsync(c->d_lls, lls_grid, sizeof(float) * c->g.ncell, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->lls_on_grid = true;
  }
  return 0;
}

static int set_clumping_grid_one(c2r_ctx *c, const float *clumping_grid) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  c->clumping_on_grid = false;
  if (clumping_grid) {
    if (!c->d_clump) HIPCHK(c, hipMalloc(&c->d_clump, sizeof(float) * c->g.ncell));
    HIPCHK(c, hipMemcpyAsync(c->d_clump, clumping_grid, sizeof(float) * c->g.ncell, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->clumping_on_grid = true;
  }
  return 0;
}

static int upload_state_one(c2r_ctx *c, const double *xh, const double *xhe, const float *temperature) {
  if (!c) return 1;
  if (!xh || !xhe) return fail(c, "c2r_upload_state: null argument");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nc = c->g.ncell;
  HIPCHK(c, hipMemcpyAsync(c->d_xh, xh, sizeof(double) * 2 * nc, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_xhe, xhe, sizeof(double) * 3 * nc, hipMemcpyHostToDevice, c->stream));
  if (temperature)
    HIPCHK(c, hipMemcpyAsync(c->d_temp, temperature, sizeof(float) * 3 * nc, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->have_state = true;
  return 0;
}

extern "C" int c2r_download_state(c2r_ctx *c, double *xh, double *xhe, float *temperature) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nc = c->g.ncell;
  if (xh) HIPCHK(c, hipMemcpyAsync(xh, c->d_xh, sizeof(double) * 2 * nc, hipMemcpyDeviceToHost, c->stream));
  if (xhe) HIPCHK(c, hipMemcpyAsync(xhe, c->d_xhe, sizeof(double) * 3 * nc, hipMemcpyDeviceToHost, c->stream));
  if (temperature)
    HIPCHK(c, hipMemcpyAsync(temperature, c->d_temp, sizeof(float) * 3 * nc, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

static int check_ready(c2r_ctx *c, const char *who) {
  if (!c->have_tables) return fail(c, "%s: c2r_set_tables has not been called", who);
  if (!c->have_step) return fail(c, "%s: c2r_set_step has not been called", who);
  if (!c->have_state) return fail(c, "%s: c2r_upload_state has not been called", who);
  if (!c->isothermal) {
    if (!c->have_heat_tables) return fail(c, "%s: non-isothermal run needs the heating tables", who);
    if (!c->have_cool) return fail(c, "%s: non-isothermal run needs c2r_set_cooling", who);
    for (int k = 0; k < 2; k++)
      if (c->have_sed[k] && !c->normflux_sed[k].empty() && !c->have_sed_heat[k])
        return fail(c, "%s: non-isothermal run needs the heating tables of SED %d", who, k + 1);
  }
  return 0;
}

static SedSet sedset(c2r_ctx *c, bool *multi) {
  SedSet ss;
  const BandData *unused = nullptr;
  (void)unused;
  ss.photo_thick[0] = c->d_photo_thick; ss.photo_thin[0] = c->d_photo_thin;
  // heating tables: the interleaved copies (made with tau_zero whenever a SED's tables are set or built)
  ss.heat_thick[0] = c->have_heat_tables ? c->d_heat_woven[0][0] : nullptr;
  ss.heat_thin[0] = c->have_heat_tables ? c->d_heat_woven[0][1] : nullptr;
  ss.lo[0] = 0; ss.hi[0] = c->bb_upper;
  *multi = false;
  for (int k = 0; k < 2; k++) {
    const bool on = c->have_sed[k] && !c->normflux_sed[k].empty();
    ss.photo_thick[k + 1] = on ? c->d_sed_tab[k][0] : nullptr;
    ss.photo_thin[k + 1] = on ? c->d_sed_tab[k][1] : nullptr;
    ss.heat_thick[k + 1] = on && c->have_sed_heat[k] ? c->d_heat_woven[k + 1][0] : nullptr;
    ss.heat_thin[k + 1] = on && c->have_sed_heat[k] ? c->d_heat_woven[k + 1][1] : nullptr;
    ss.lo[k + 1] = on ? c->sed_lo[k] : 0;
    ss.hi[k + 1] = on ? c->sed_hi[k] : 0;
    *multi = *multi || on;
  }
  return ss;
}

static StepScalars scalars(c2r_ctx *c) {
  StepScalars s = c->sc;
  s.cellvol = s.dr1 * s.dr2 * s.dr3;
  s.cd.cool = c->d_cool;
  s.cd.mintemp = c->cool_mintemp;
  s.cd.dtemp = c->cool_dtemp;
  s.cd.zred = c->zred;
  s.cd.H0 = c->H0;
  s.cd.Omega0 = c->Omega0;
  s.cd.logtab = nullptr;
  return s;
}

// RatesTables of a pass: the pair copy as it stands, and, on an all-periodic mesh, the shell volumes for the cell sizes of
// `sc` -- made here, on the main stream (which every rates launch of the pass waits for), when there are none yet or the
// sizes differ from those the table was made from.  Within a time step the sizes stay what they are, so its outer
// iterations, their passes and all sources share one table (16 bytes per offset: 2 bytes per mesh cell).
static int rates_tables(c2r_ctx *c, const StepScalars &sc, RatesTables &rt) {
  rt = RatesTables{c->d_photo_pairs, nullptr, 0, 0, 0};
  if (!c->periodic) return 0;
  const int e1 = shell_vol_extent(c->g.n1, c->g.l1), e2 = shell_vol_extent(c->g.n2, c->g.l2), e3 = shell_vol_extent(c->g.n3, c->g.l3);
  const size_t n = (size_t)e1 * e2 * e3;
  const double key[4] = {sc.dr1, sc.dr2, sc.dr3, sc.cellvol};
  if (!c->shellvol_valid || std::memcmp(key, c->sv_key, sizeof key) != 0) {
    c->shellvol_valid = false;
    if (!c->d_shellvol) {
      HIPCHK(c, hipMalloc(&c->d_shellvol, sizeof(ShellVol) * n));
      HIPCHK(c, hipMalloc(&c->d_shellvol_flag, sizeof(int)));
    }
    HIPCHK(c, hipMemsetAsync(c->d_shellvol_flag, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(k_shell_volumes, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, sc.dr1, sc.dr2, sc.dr3,
                       sc.cellvol, e1, e2, e3, c->d_shellvol, c->d_shellvol_flag);
    HIPCHK(c, hipGetLastError());
    int not_big = 1;
    HIPCHK(c, hipMemcpyAsync(&not_big, c->d_shellvol_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->shellvol_big = not_big ? 0 : 1;
    std::memcpy(c->sv_key, key, sizeof key);
    c->shellvol_valid = true;
  }
  rt.shellvol = c->d_shellvol;
  rt.e1 = e1;
  rt.e2 = e2;
  rt.big = c->shellvol_big;
  return 0;
}

// Column scratch for the passes of the step that begins, sized from what the LAST pass learnt about every source (sub-box
// counts carried from time step to time step, and with a source's cell from source list to source list): for each ping-pong set
// the blocks of its largest batch, in ONE segment.  A device allocation costs ~25 ms per GB here and synchronises the device;
// made now, it does not land inside an outer iteration (round-4 VERDICT: 0.3-0.8 s of such allocations, and a batch that
// started over, inside iterations 6 and 7 of profiles/r04_config4_call.json).  What cannot be known -- a first time step from a
// neutral start, a source that brightens -- still grows inside a pass, as before.
// Shells a source's column block is made for: the sub-boxes it needed in the last pass plus one round -- plus as many as its
// box grew by between the last two passes when it is growing faster than that (while the ionisation fronts of a first
// time step break out, boxes jump several rounds per iteration: a block sized for one more round then moved to one twice
// as deep in the middle of the sweep, its old place lay idle until the batch was over, and a batch that ran out of room
// that way started over); four rounds when nothing is known; never more than the mesh.
// extent of the mesh as seen from a source
struct Reach {
  int l[3], r[3];
};
// periodic_bc = .true. (evolve_source.F90:103-105): the same for every source
static Reach mesh_reach(const Grid &g) {
  const int mesh[3] = {g.n1, g.n2, g.n3};
  Reach R;
  for (int d = 0; d < 3; d++) {
    R.r[d] = std::min(MAX_SUBBOX, mesh[d] / 2 - 1 + mesh[d] % 2);
    R.l[d] = -std::min(MAX_SUBBOX, mesh[d] / 2);
  }
  return R;
}
// open boundaries, the else branch of evolve_source.F90:107-108 (dead code there: lastpos_r = min(srcpos + max_subbox,
// mesh), lastpos_l = max(srcpos - max_subbox, 1)): up to the mesh faces, per source -- along the axes that are open;
// along one that is periodic while another is open, the mesh's reach as above (axis_reach, c2ray_shell.hpp)
static Reach open_reach(const Grid &g, const bool *per, const int *srcpos) {
  const int mesh[3] = {g.n1, g.n2, g.n3};
  Reach R;
  // (axis_reach's numbers for a source inside the mesh; one outside along an open axis reaches through the vacuum)
  for (int d = 0; d < 3; d++) axis_reach_external(mesh[d], srcpos[d], per[d], MAX_SUBBOX, R.l[d], R.r[d]);
  return R;
}
static Reach source_reach(const c2r_ctx *c, int ns) {
  return c->periodic ? mesh_reach(c->g) : open_reach(c->g, c->per, &c->srcpos[3 * (size_t)(ns - 1)]);
}
// SrcDev::wn of a context that is not all-periodic
static void source_wrap(const c2r_ctx *c, int *wn) {
  const int mesh[3] = {c->g.n1, c->g.n2, c->g.n3};
  for (int d = 0; d < 3; d++) wn[d] = axis_wrap_extent(mesh[d], c->per[d]);
}
// the largest shell a source's column block ever has to hold
static int source_smax(const c2r_ctx *c, int ns) {
  if (c->periodic) return c->g.smax;
  const Reach R = source_reach(c, ns);
  int m = 0;
  for (int d = 0; d < 3; d++) m = std::max(m, std::max(R.r[d], -R.l[d]));
  return m;
}

// entries per column array of source ns's block for the shells 0..cap: the whole shells, or (open boundaries) their cells
// within the source's reach -- never more than the mesh has cells, unless the source stands outside it (its reach then runs
// through the vacuum between them: fewer than 2^31 cells, c2r_set_sources_external)
static size_t source_block_entries(const c2r_ctx *c, int ns, int cap) {
  if (c->periodic) return block_doubles(cap) / 6;
  const Reach R = source_reach(c, ns);
  return (size_t)reach_cells(R.l, R.r, cap);
}
static size_t source_block_doubles(const c2r_ctx *c, int ns, int cap) { return 6 * source_block_entries(c, ns, cap); }

static int predicted_shells(const c2r_ctx *c, int ns) {
  const int prev = c->prev_nbox[(size_t)ns - 1];
  const int grow = c->prev_grow.size() == c->prev_nbox.size() ? c->prev_grow[(size_t)ns - 1] : 0;
  const int smax = source_smax(c, ns);
  const int cap = std::min(smax, SUBBOXSIZE * (prev > 0 ? prev + std::max(1, 2 * grow) : 4));
  // within a fifth of the mesh limit: the limit (a block less than twice as large, and never a move)
  return 5 * cap >= 4 * smax ? smax : cap;
}

static int arena_prepare(c2r_ctx *c) {
  // C2R_ARENA_RESERVE_GB="a[,b]": column scratch of set 0 (and set 1) made when the FIRST step begins, for hosts that know
  // what their source lists will need.  A device allocation beyond the first tens of GB costs ~24 ms per GB on this system
  // and stalls every launch of the process while it lasts, whichever thread makes it (tools/micro/malloc_overlap.hip,
  // profiles/r05_malloc_overlap.txt: 0.97 s for 40 GB, the kernel stream of another thread idle for all of it): it can be
  // moved, not hidden -- this moves it in front of the first iteration.
  if (!c->arena_reserved) {
    c->arena_reserved = true;
    if (const char *e = getenv("C2R_ARENA_RESERVE_GB")) {
      double gb[2] = {0.0, 0.0};
      const int n = sscanf(e, "%lf,%lf", &gb[0], &gb[1]);
      for (int set = 0; set < 2 && set < std::max(n, 0); set++) {
        const size_t want = (size_t)(gb[set] * 1.0e9 / sizeof(double));
        size_t have = 0;
        for (const c2r_ctx::Segment &sg : c->segs[set]) have += sg.n;
        if (want > have) {
          c->seg_cur[set] = c->segs[set].size(); // a new segment, whatever the existing ones have free
          c->seg_used[set] = 0;
          (void)arena_alloc(c, set, want - have, want - have);
          c->seg_cur[set] = c->seg_used[set] = 0;
        }
      }
    }
  }
  if (c->last_stride < 1 || c->prev_nbox.size() != (size_t)c->nsrc) return 0;
  std::vector<int> mine; // this context's share, as the last pass had it (do_grid_static: first = 1 + rank, stride = ranks)
  for (int ns = c->last_first; ns <= c->nsrc; ns += c->last_stride) mine.push_back(ns);
  const int limit = std::min(c->batch, BATCH_MAX);
  size_t need[2] = {0, 0};
  int bi = 0;
  for (size_t b0 = 0; b0 < mine.size(); b0 += (size_t)limit, bi++) {
    size_t sum = 0, spare = 0;
    for (size_t b = b0; b < std::min(mine.size(), b0 + (size_t)limit); b++) {
      const int cap = predicted_shells(c, mine[b]); // pass_list's predicted_cap
      sum += source_block_doubles(c, mine[b], cap);
      // ... and room for ONE source of the batch to outgrow that (its block then moves to one twice as deep)
      const int smax = source_smax(c, mine[b]);
      if (cap < smax) spare = std::max(spare, source_block_doubles(c, mine[b], std::min(smax, 2 * cap)));
    }
    need[bi & 1] = std::max(need[bi & 1], sum + spare);
  }
  for (int set = 0; set < 2; set++) {
    if (need[set] == 0) continue;
    std::vector<c2r_ctx::Segment> &sg = c->segs[set];
    size_t largest = 0;
    for (size_t i = 1; i < sg.size(); i++)
      if (sg[i].n > sg[largest].n) largest = i;
    if (!sg.empty() && sg[largest].n >= need[set]) {
      std::swap(sg[0], sg[largest]); // blocks are cut from the segments in order: the one that holds a whole batch first
      continue;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream2)); // nothing of an earlier pass may still read the segments given back
    HIPCHK(c, hipStreamSynchronize(c->stream3));
    arena_release(c, set);
    c->seg_cur[set] = c->seg_used[set] = 0;
    (void)arena_alloc(c, set, need[set], need[set]); // no room for all of it: the pass will cut its batches, as before
    c->seg_cur[set] = c->seg_used[set] = 0;
  }
  return 0;
}

static int begin_step_one(c2r_ctx *c) {
  if (!c) return 1;
  if (!c->have_state) return fail(c, "c2r_begin_step: c2r_upload_state has not been called");
  HIPCHK(c, hipSetDevice(c->device));
  if (arena_prepare(c)) return 1;
  c->packed_valid = c->transposed_valid = false; // xh_av, xhe_av are overwritten below
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nc = c->g.ncell;
  HIPCHK(c, hipMemcpyAsync(c->d_xh_av, c->d_xh, sizeof(double) * 2 * nc, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_xh_int, c->d_xh, sizeof(double) * 2 * nc, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_xhe_av, c->d_xhe, sizeof(double) * 3 * nc, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_xhe_int, c->d_xhe, sizeof(double) * 3 * nc, hipMemcpyDeviceToDevice, c->stream));
  c->last_conv = -1;
  return 0;
}

static int end_step_one(c2r_ctx *c) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nc = c->g.ncell;
  HIPCHK(c, hipMemcpyAsync(c->d_xh, c->d_xh_int, sizeof(double) * 2 * nc, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_xhe, c->d_xhe_int, sizeof(double) * 3 * nc, hipMemcpyDeviceToDevice, c->stream));
  if (!c->isothermal) // set_final_temperature_point (mat_ini_test.F90:505-515)
    HIPCHK(c, hipMemcpyAsync(c->d_temp + 2 * nc, c->d_temp, sizeof(float) * nc, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

static int set_rates_to_zero_one(c2r_ctx *c) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  // Carried out lazily: when the pass that follows starts with a rates launch that covers every cell, that launch
  // writes the grids instead of adding to them and nothing has to be zeroed (flush_rates_zero otherwise).
  c->rates_zero_pending = true;
  std::memset(c->photon_loss, 0, sizeof c->photon_loss);
  c->sum_nbox = 0;
  std::fill(c->horizon_loss.begin(), c->horizon_loss.end(), 0.0); // (c2r_enable_horizon_loss)
  // the escape maps follow photon_loss (on the sweep stream, which every kernel that adds to them runs on)
  if (c->d_face_maps) HIPCHK(c, zero_device(c->d_face_maps, sizeof(double) * c->face_total, c->stream));
  return 0;
}

// the zeroing a c2r_set_rates_to_zero left pending, before anything reads or partly writes the rate grids
static int flush_rates_zero(c2r_ctx *c) {
  if (!c->rates_zero_pending) return 0;
  c->rates_zero_pending = false;
  c->phiheat_dirty = false;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, zero_device(c->d_rates, sizeof(double) * c->rates_count, c->stream));
  return 0;
}

static int set_batch_one(c2r_ctx *c, int nbatch) {
  if (!c) return 1;
  if (nbatch < 1 || nbatch > BATCH_MAX) return fail(c, "c2r_set_batch: %d not in [1,%d]", nbatch, BATCH_MAX);
  c->batch = nbatch;
  return 0;
}

// host-side sub-box bookkeeping of one source (do_source, evolve_source.F90:96-144, 233-236)
struct SrcRun {
  int ns;                 // 1-based source number
  int nbox = 0;
  double total_flux = 0, loss = 0;
  bool active = true;
  bool final_loss_due = false; // the last round ended for geometric reasons: its full loss is evaluated after the sweep
  int cap = 0;            // shells the column block can hold
  int smax_prev = -1;     // largest shell already swept
  Reach reach{};          // how far its box can go: the mesh's with periodic boundaries, its own with open ones
  int smax = 0;           // the largest shell within that reach
  long long sweep_threads = 0; // threads of the shell launches spent on it (c2r_get_source_trace)
  int entry_rounds = 0;   // > 0: the source has entry columns (c2r_set_source_face_entry) and is traced for that many rounds
                          // (fewer where its box cannot grow any more): no loss decides for it, and no probe looks at it
};

// the sub-box after `nbox` rounds (evolve_source.F90:141-144)
static Box round_box(const Reach &R, int nbox) {
  Box b;
  for (int d = 0; d < 3; d++) {
    b.hi[d] = std::min(SUBBOXSIZE * nbox, R.r[d]);
    b.lo[d] = std::max(-SUBBOXSIZE * nbox, R.l[d]);
  }
  return b;
}
static int box_smax(const Box &b) {
  int m = 0;
  for (int d = 0; d < 3; d++) m = std::max(m, std::max(b.hi[d], -b.lo[d]));
  return m;
}
static long long box_cells(const Box &b) {
  long long v = 1;
  for (int d = 0; d < 3; d++) v *= (b.hi[d] - b.lo[d] + 1);
  return v;
}
// the while-test of evolve_source.F90:136-139 can still pass after this box (z extent short of the mesh)
static bool box_can_grow(const Reach &R, const Box &b) { return b.hi[2] < R.r[2] && b.lo[2] > R.l[2]; }
// Open boundaries: that test looks at z only and at both sides at once, so a source on the plane k = 1 would never start
// its first round.  Instead: at least one of the six faces of the box is still short of the source's reach.
static bool box_can_grow_open(const Reach &R, const Box &b) {
  for (int d = 0; d < 3; d++)
    if (b.hi[d] < R.r[d] || b.lo[d] > R.l[d]) return true;
  return false;
}
static bool can_grow(const c2r_ctx *c, const Reach &R, const Box &b) { return c->periodic ? box_can_grow(R, b) : box_can_grow_open(R, b); }

static int pool_event(c2r_ctx *c, hipEvent_t *out) {
  if (c->ev_used == c->ev_pool.size()) {
    hipEvent_t e;
    HIPCHK(c, hipEventCreate(&e));
    c->ev_pool.push_back(e);
  }
  *out = c->ev_pool[c->ev_used++];
  return 0;
}


// A surface cell has one coordinate on a face of the box, so its shell is at least the nearest face's distance: the shells
// of [s_lo, s_hi] before that hold none.  Their blocks (this many) are not launched and their partial sums are set to zero.
static int blocks_before_surface(const c2r_ctx *c, const Box &box, int s_lo, int s_hi) {
  int s_first = 1 << 30;
  for (int d = 0; d < 3; d++) s_first = std::min(s_first, std::min(std::abs(box.lo[d]), std::abs(box.hi[d])));
  s_first = std::min(std::max(s_first, s_lo), s_hi);
  return c->block_base[s_first] - c->block_base[s_lo];
}

// Photon loss of the round's box for the sources h_list[set][list_off .. +n) (positions in the batch) into
// c->h_loss[0..n).  Synchronises the sweep stream.
// Open boundaries: `box` is the round's box before it is cut at each source's reach; deciding: the sum over the faces that
// can still move (the while-test), else the sum over the whole surface (the loss that is kept).
static int boundary_loss(c2r_ctx *c, int set, size_t list_off, int n, int s_lo, int s_hi, const Box &box,
                         const StepScalars &sc, const SedSet &ss, bool multi, bool deciding, const SrcEntry *ent = nullptr) {
  // ent: the kept loss of a batch that holds a source with entry columns (k_loss_entry; its records, one per source)
  const int nblk = c->block_base[s_hi + 1] - c->block_base[s_lo];
  const size_t need = (size_t)nblk * n;
  if (c->loss_partial_cap < need) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (ensure_pair<double>(c, &c->d_loss_partial, (double **)nullptr, &c->loss_partial_cap, need)) return 1;
  }
  // (open boundaries: a box cut at a mesh face has surface cells in every shell)
  const int first_block = c->periodic ? blocks_before_surface(c, box, s_lo, s_hi) : 0;
  if (first_block > 0) HIPCHK(c, zero_device(c->d_loss_partial, sizeof(double) * need, c->stream));
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(nblk - first_block, n), dim3(BLOCK), 0, c->stream, c->g, c->d_src[set], c->d_list[set] + list_off,
                       multi ? 1 : 0, s_lo, s_hi, box, sc, c->d_bands, ss, c->d_block_base, c->d_loss_partial, nblk,
                       1, first_block);
  };
  if (ent)
    hipLaunchKernelGGL(k_loss_entry, dim3(nblk - first_block, n), dim3(BLOCK), 0, c->stream, c->g, c->d_src[set], c->d_list[set] + list_off,
                       multi ? 1 : 0, s_lo, s_hi, box, sc, c->d_bands, ss, c->d_block_base, c->d_loss_partial, nblk, 1, first_block, ent);
  else if (c->periodic) go(k_loss<false, false>);
  else if (deciding) go(k_loss<true, true>);
  else go(k_loss<true, false>);
  hipLaunchKernelGGL(k_loss_finish, dim3(n), dim3(BLOCK), 0, c->stream, c->d_loss_partial, nblk, nblk, c->d_loss_acc);
  c->tm.sweep_launches += 2;
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->h_loss, c->d_loss_acc, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// shells below this one read the i-faces' state from the mesh-ordered grids (see pass_list)
constexpr int TRANSPOSED_FROM_SHELL = 32;

constexpr int PROBE_SAMPLE = 16; // the probe looks at 8 cells of every 16th block of the round's shells

// One round of a batch's sub-box loop, as the probes and the while-test see it.
struct RoundRec {
  int round = 0, nact = 0, s_lo = 0, s_hi = 0;
  size_t off = 0;     // its active list in h_list / d_list
  size_t acc_off = 0; // its results in d_probe_acc / h_probe
  Box box{};
};

// What the batches of one pass share.
struct PassCtx {
  c2r_ctx *c;
  StepScalars sc;
  SedSet ss;
  bool multi;
  Reach reach;
  bool generic_sweep;           // C2R_SWEEP_GENERIC=1 (diagnostic): every shell through the general per-cell code, one launch per shell
  bool arena_log;               // C2R_ARENA_LOG: say when a batch is cut or starts over
  bool packed_early = false;    // the mesh-ordered products need not wait for anything
  bool transposed_seen = false; // the sweep stream has waited for ev_transposed
  int nslab = 0;                // rate-grid slabs of the last batch (0: one rates launch)
  long long stamp = 0;          // this pass in the count of all passes of the process (c2r_get_source_trace)
  std::vector<hipEvent_t> tev;  // per batch: sweep start, sweep end, rates start, rates end
  RatesTables rt{};             // what the rates launches read instead of computing it (rates_tables)
};

// One batch: the sources mine[b0 .. b0 + nb) on scratch set `set`.
struct Batch {
  int set = 0, nb = 0;
  size_t b0 = 0;
  std::vector<int> known0; // what the last pass knew about the batch's sources (a batch that starts over raises prev_nbox)
  int restarts = 0;
  hipEvent_t ev[4] = {};   // timing: sweep start, sweep end, rates start, rates end
  // one attempt: a batch that starts over begins these anew
  std::vector<SrcRun> run;
  size_t list_used = 0;             // entries of h_list[set] / d_list[set] in use
  std::vector<RoundRec> recs;       // the rounds swept so far
  size_t settled = 0, launched = 0; // recs[0, settled): while-test applied; recs[settled, launched): probes in flight
  bool sweep_started = false;       // ev[0] goes in front of the first shell launch, behind the uploads of records and lists
  int ntiles = 0;                   // tiles in the rates launch's list h_tiles[set] (0: none, every tile of the mesh)
  bool beamed = false;              // some source of the batch has a beam or a finite horizon: its rates launch is k_rates_beam
  bool curved = false;              // some source of the batch has a curve: its rates launch is k_rates_curve
  bool external = false;            // some source of the batch stands outside the mesh: its shells are k_sweep_shell(_fast)_ext's,
                                    // and its kept losses are k_loss's (queue_kept_losses)
  bool entry = false;               // some source of the batch has entry columns (c2r_set_source_face_entry), or the mesh has an
                                    // origin (c2r_set_mesh_origin): the shells are
                                    // k_sweep_shell(_fast)_entry's, the kept losses k_loss_entry's; d_ent[set] holds the records
  bool halo = false;                // some source of the batch has a halo of several faces (c2r_set_source_halo): entry is set
                                    // too, and the shells are k_sweep_shell(_fast)_halo's
  std::vector<int> rim_ns;          // horizon loss: the sources (1-based) whose sums queue_horizon_rim has queued, in row order
};

// Queue the probes of the batch's rounds recs[launched ..) (lower bounds of their boundary losses, k_loss_probe_rounds) on
// the probe stream, behind everything queued on the sweep stream so far, and the copy of all their results to h_probe; ev_probe
// marks the end.  Does not wait.  One event on the sweep stream for all of them: the rounds of a batch whose
// sources are all expected to go on (prev_nbox) are probed together, late, and the sweep stream sees no probe
// kernel, no copy and no other event between its shells.  Whoever then changes what a probe reads -- the SrcDev
// entries, when a block moves -- waits for ev_probe first.
static int launch_probes(const PassCtx &P, Batch &B) {
  c2r_ctx *c = P.c;
  const std::vector<RoundRec> &recs = B.recs;
  const size_t from = B.launched, to = recs.size();
  if (from >= to) return 0;
  size_t need = 0;
  for (size_t i = from; i < to; i++) {
    const int count = c->block_base[recs[i].s_hi + 1] - c->block_base[recs[i].s_lo];
    need += (size_t)((count + PROBE_SAMPLE - 1) / PROBE_SAMPLE) * (size_t)recs[i].nact;
  }
  const size_t acc_need = recs[to - 1].acc_off + (size_t)recs[to - 1].nact;
  HIPCHK(c, hipEventSynchronize(c->ev_probe)); // the descriptors of an earlier launch have left the pinned buffer
  if (c->probe_acc_cap < acc_need) return fail(c, "internal: probe results of %zu rounds do not fit (%zu > %zu)", to, acc_need, c->probe_acc_cap);
  if (c->probe_partial_cap < need) {
    HIPCHK(c, hipStreamSynchronize(c->stream_probe)); // earlier probes may still use the old buffer
    if (ensure_pair<double>(c, &c->d_probe_partial, (double **)nullptr, &c->probe_partial_cap, need)) return 1;
  }
  hipStream_t st = c->stream_probe;
  HIPCHK(c, hipEventRecord(c->ev_round, c->stream));
  HIPCHK(c, hipStreamWaitEvent(st, c->ev_round, 0));
  // descriptors of the rounds, then one probe launch and one finishing launch for all of them
  const size_t nr = to - from;
  if (c->probe_rounds_cap < nr) {
    HIPCHK(c, hipStreamSynchronize(c->stream_probe));
    if (c->d_probe_rounds) HIPCHK(c, hipFree(c->d_probe_rounds));
    if (c->h_probe_rounds) HIPCHK(c, hipHostFree(c->h_probe_rounds));
    c->d_probe_rounds = c->h_probe_rounds = nullptr;
    const size_t want = nr + 64;
    HIPCHK(c, hipMalloc(&c->d_probe_rounds, sizeof(ProbeRound) * want));
    HIPCHK(c, hipHostMalloc(&c->h_probe_rounds, sizeof(ProbeRound) * want));
    c->probe_rounds_cap = want;
  }
  ProbeRound *hr = static_cast<ProbeRound *>(c->h_probe_rounds);
  size_t used = 0;
  int max_nblk = 0, max_nact = 0;
  for (size_t i = from; i < to; i++) {
    const RoundRec &R = recs[i];
    const int count = c->block_base[R.s_hi + 1] - c->block_base[R.s_lo];
    ProbeRound &P = hr[i - from];
    P.s_lo = R.s_lo; P.s_hi = R.s_hi; P.box = R.box;
    P.list_off = (int)R.off; P.nact = R.nact;
    P.nblk = (count + PROBE_SAMPLE - 1) / PROBE_SAMPLE;
    P.partial_off = (int)used; P.acc_off = (int)R.acc_off;
    used += (size_t)P.nblk * (size_t)R.nact;
    max_nblk = std::max(max_nblk, P.nblk);
    max_nact = std::max(max_nact, P.nact);
  }
  HIPCHK(c, hipMemcpyAsync(c->d_probe_rounds, hr, sizeof(ProbeRound) * nr, hipMemcpyHostToDevice, st));
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(max_nblk, max_nact, (unsigned)nr), dim3(BLOCK), 0, st, c->g, c->d_src[B.set], c->d_list[B.set],
                       static_cast<const ProbeRound *>(c->d_probe_rounds), P.multi ? 1 : 0, P.sc, c->d_bands, P.ss, c->d_block_base,
                       c->d_probe_partial, PROBE_SAMPLE);
  };
  if (c->periodic) go(k_loss_probe_rounds<false>); else go(k_loss_probe_rounds<true>);
  hipLaunchKernelGGL(k_loss_finish_rounds, dim3(max_nact, (unsigned)nr), dim3(BLOCK), 0, st,
                     static_cast<const ProbeRound *>(c->d_probe_rounds), c->d_probe_partial, c->d_probe_acc);
  c->tm.sweep_launches += 2;
  HIPCHK(c, hipGetLastError());
  const size_t a0 = recs[from].acc_off;
  HIPCHK(c, hipMemcpyAsync(c->h_probe + a0, c->d_probe_acc + a0, sizeof(double) * (acc_need - a0), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipEventRecord(c->ev_probe, st));
  B.launched = to;
  return 0;
}

// do_source (evolve_source.F90:66-238) for every source number in `mine`, up to c->batch at a time.
// Per batch: the column sweep (dependent shell launches, host test of the sub-box loop) on the
// high-priority stream, then ONE rates launch for the whole batch on the second stream; the next
// batch's sweep overlaps it (scratch sets ping-pong).  Rates launches are ordered on their stream,
// so the accumulation over sources keeps the reference's order.
static int pass_finish(c2r_ctx *c);

// the losses of set `set`'s batches that were still on their way from the device (the caller has waited for the
// set's last rates launch and what follows it)
static void resolve_tails(c2r_ctx *c, int set) {
  for (c2r_ctx::BatchTail &bt : c->tails) {
    if (bt.resolved || bt.set != set) continue;
    for (size_t b = 0; b < bt.loss.size(); b++)
      if (bt.slot[b] >= 0) bt.loss[b] = c->h_final[set][bt.slot[b]];
    for (size_t j = 0; j < bt.rim_ns.size(); j++) bt.rim_loss[j] = c->h_rim[set][j];
    bt.resolved = true;
  }
}

constexpr int START_OVER = 2; // sweep_batch: the batch has to start over (0: swept, 1: error)

// The products neufrac * ndens the sweep reads (k_pack_state; xh_av, xhe_av change every iteration), in mesh order and in
// (j,i,k) order: made on the third stream while the inner shells, which do without them, are already on their way.
static int queue_state_products(c2r_ctx *c) {
  const Grid &g = c->g;
  HIPCHK(c, hipStreamWaitEvent(c->stream3, c->ev_sweep_done[0], 0));
  // both valid: nothing to make, the global pass transposed its own products (ev_transposed is on record since then)
  const bool make = !(c->packed_valid && c->transposed_valid);
  if (make && c->packed_valid)
    hipLaunchKernelGGL(k_transpose_packed, dim3((g.n1 + 31) / 32, (g.n2 + 31) / 32, 3 * g.n3), dim3(BLOCK), 0, c->stream3, g,
                       c->d_stateT, c->d_stateT + 3 * g.ncell);
  else if (make)
    hipLaunchKernelGGL(k_pack_state, dim3((g.n1 + 31) / 32, (g.n2 + 31) / 32, g.n3), dim3(BLOCK), 0, c->stream3, g, c->d_ndens, c->d_xh_av,
                       c->d_xhe_av, c->d_stateT, c->d_stateT + 3 * g.ncell);
  HIPCHK(c, hipGetLastError());
  if (make) HIPCHK(c, hipEventRecord(c->ev_transposed, c->stream3));
  return 0;
}

// Column blocks of the batch (predicted_shells), their SrcDev entries and the sources' fluxes; B.nb becomes what fits.
// Segments are kept from batch to batch and pass to pass (allocation is slow), so what the set holds may be cut for other
// block sizes than this batch needs (many small segments of a pass with small boxes).  When the blocks do not fit although
// less than half of what the set holds is in use, its segments are given back and made anew in one piece; otherwise the
// batch is what did fit.
static int place_batch(const PassCtx &P, const std::vector<int> &mine, Batch &B) {
  c2r_ctx *c = P.c;
  const int set = B.set;
  SrcDev *hs = c->h_src[set];
  B.run.assign((size_t)B.nb, SrcRun());
  B.beamed = false;
  B.curved = false;
  B.external = false;
  B.entry = false;
  B.halo = false;
  for (bool released = false;;) {
    c->seg_cur[set] = 0;
    c->seg_used[set] = 0;
    c->vacated[set].clear();
    size_t total = 0;
    for (int b = 0; b < B.nb; b++) total += source_block_doubles(c, mine[B.b0 + b], predicted_shells(c, mine[B.b0 + b]));
    int placed = 0;
    size_t placed_doubles = 0;
    for (; placed < B.nb; placed++) {
      SrcRun &r = B.run[placed];
      r.ns = mine[B.b0 + placed];
      r.cap = predicted_shells(c, r.ns);
      hs[placed].cz = source_block_entries(c, r.ns, r.cap);
      hs[placed].cols = arena_alloc(c, set, 6 * hs[placed].cz, total);
      if (!hs[placed].cols) break;
      total -= 6 * hs[placed].cz;
      placed_doubles += 6 * hs[placed].cz;
    }
    if (placed == B.nb) break;
    size_t have = 0;
    for (const c2r_ctx::Segment &sg : c->segs[set]) have += sg.n;
    if (!released && have > 0 && placed_doubles < have / 2) {
      released = true;
      arena_release(c, set);
      continue;
    }
    if (placed == 0) return fail(c, "column scratch: one source of this mesh does not fit in device memory");
    // A batch cut to exactly what fits has no room for a source that outgrows its block (the deeper block is needed
    // while the old one is still in use) and starts over at the first such move -- at 512^3, where a block at the mesh
    // limit is 6.4 GB and a set holds some twenty, 615 times in six passes (round 5).  So the cut leaves room for a third
    // of the sources that can still grow to move once; sources at the mesh limit need none.
    int keep = placed;
    for (;;) {
      size_t used = 0, reserve = 0;
      for (int b = 0; b < keep; b++) {
        used += 6 * hs[b].cz;
        const int smax = source_smax(c, B.run[b].ns);
        if (B.run[b].cap < smax) reserve += source_block_doubles(c, B.run[b].ns, std::min(smax, 2 * B.run[b].cap));
      }
      if (keep <= 1 || used + reserve / 3 <= placed_doubles) break;
      keep--;
    }
    if (P.arena_log) fprintf(stderr, "c2ray_hip: column scratch, set %d: batch of %d cut to %d sources (%d fit)\n", set, B.nb, keep, placed);
    B.nb = keep; // the same calls place the same blocks again
    B.run.resize((size_t)B.nb);
  }
  for (int b = 0; b < B.nb; b++) {
    SrcRun &r = B.run[b];
    r.total_flux = c->normflux[r.ns - 1] * c->s_star; // evolve_source.F90:122-128
    for (int k = 0; k < 2; k++)
      if (P.multi && !c->normflux_sed[k].empty())
        r.total_flux = r.total_flux + c->normflux_sed[k][r.ns - 1] * c->s_star_sed[k];
    r.loss = r.total_flux;
    SrcDev &S = hs[b];
    const int *p = &c->srcpos[3 * (size_t)(r.ns - 1)];
    S.i0 = p[0]; S.j0 = p[1]; S.k0 = p[2];
    for (int d = 0; d < 3; d++) { S.lo[d] = 0; S.hi[d] = 0; }
    r.reach = source_reach(c, r.ns);
    r.smax = source_smax(c, r.ns);
    for (int d = 0; d < 3; d++) { S.rl[d] = r.reach.l[d]; S.rr[d] = r.reach.r[d]; }
    source_wrap(c, S.wn);
    S.nflux = c->normflux[r.ns - 1];
    for (int k = 0; k < 2; k++) S.nflux_sed[k] = c->normflux_sed[k].empty() ? 0.0 : c->normflux_sed[k][r.ns - 1];
    source_cut(c, r.ns, S);
    B.beamed = B.beamed || S.cut != CUT_NONE;
    B.curved = B.curved || (S.cut & CUT_CURVE) != 0;
    B.external = B.external || (c->ext_smax > 0 && source_is_external(c, r.ns));
    const bool placed_in_deep = c->origin[0] != 0 || c->origin[1] != 0 || c->origin[2] != 0;
    if (placed_in_deep || !c->src_entry.empty()) { // (either exists: the pinned records do too)
      const c2r_ctx::FaceEntry e = c->src_entry.empty() ? c2r_ctx::FaceEntry() : c->src_entry[(size_t)r.ns - 1];
      SrcEntry &E = c->h_ent[set][b];
      E = SrcEntry{e.face >= 0 ? 1 + e.face : 0, e.d_cols, {c->origin[0], c->origin[1], c->origin[2]}, {HALO_INSIDE, HALO_INSIDE, HALO_INSIDE}, {}};
      const int mesh[3] = {c->g.n1, c->g.n2, c->g.n3};
      for (int d = 0; d < 3; d++)
        if (e.faces[d] >= 0) E.ghost[d] = halo_ghost_index(p[d], mesh[d]);
      for (int a = 0; a < HALO_ARRAYS; a++) E.part[a] = e.off[a] == c2r_ctx::HALO_ABSENT ? nullptr : e.d_cols + e.off[a];
      r.entry_rounds = e.face >= 0 ? e.rounds : 0;
      B.halo = B.halo || e.several();
      // (a mesh with an origin: every batch through the kernels that move cinterp's coordinates, entry or not)
      B.entry = B.entry || e.face >= 0 || placed_in_deep;
    }
  }
  if (B.entry) HIPCHK(c, hipMemcpyAsync(c->d_ent[set], c->h_ent[set], sizeof(SrcEntry) * B.nb, hipMemcpyHostToDevice, c->stream));
  // coldensh_out = 0 for every new source (evolve_source.F90:94-95) serves two purposes in the
  // reference: the "already done" marker (replaced here by the shell order: every cell is visited
  // once) and finite values for corners whose interpolation weight is exactly 0.  The arena is
  // zeroed once at allocation and only ever holds finite columns afterwards, so 0*w stays 0.
  HIPCHK(c, hipMemcpyAsync(c->d_src[set], hs, sizeof(SrcDev) * B.nb, hipMemcpyHostToDevice, c->stream));
  return 0;
}

// Read the probes of all rounds not yet decided, replace what a probe leaves undecided by the full sum, apply the while-test
// round by round: sources that stop get active = false and that round as their last.
static int settle_rounds(const PassCtx &P, Batch &B) {
  c2r_ctx *c = P.c;
  if (B.settled == B.recs.size()) return 0;
  if (launch_probes(P, B)) return 1;
  HIPCHK(c, hipEventSynchronize(c->ev_probe));
  int *hl = c->h_list[B.set];
  for (; B.settled < B.recs.size(); B.settled++) {
    const RoundRec &R = B.recs[B.settled];
    const double *probe = c->h_probe + R.acc_off;
    const int *lst = hl + R.off;
    std::vector<int> undecided;
    for (int a = 0; a < R.nact; a++) {
      SrcRun &r = B.run[lst[a]];
      if (!r.active) continue; // stopped at an earlier round: swept this one on trust, to no effect
      r.loss = probe[a];
      if (!(r.loss > 2.0 * (C2R_F(1e-10) * r.total_flux))) undecided.push_back(lst[a]);
    }
    if (!undecided.empty()) {
      int *ul = hl + B.list_used;
      std::copy(undecided.begin(), undecided.end(), ul);
      HIPCHK(c, hipMemcpyAsync(c->d_list[B.set] + B.list_used, ul, sizeof(int) * undecided.size(), hipMemcpyHostToDevice, c->stream));
      if (boundary_loss(c, B.set, B.list_used, (int)undecided.size(), R.s_lo, R.s_hi, R.box, P.sc, P.ss, P.multi, true)) return 1;
      B.list_used += undecided.size();
      for (size_t j = 0; j < undecided.size(); j++) B.run[undecided[j]].loss = c->h_loss[j];
    }
    for (int a = 0; a < R.nact; a++) {
      SrcRun &r = B.run[lst[a]];
      if (!r.active) continue;
      if (!(r.loss > C2R_F(1e-10) * r.total_flux)) { // evolve_source.F90:136: the box does not grow any more
        r.active = false;
        r.nbox = R.round;
      }
    }
  }
  return 0;
}

// every source still active reached at least round `round` in the previous pass
static bool all_reached(const c2r_ctx *c, const Batch &B, int round) {
  for (const SrcRun &r : B.run)
    if (r.active && r.entry_rounds == 0 && c->prev_nbox[(size_t)r.ns - 1] < round) return false; // (entry columns: its rounds are given)
  return true;
}

// Source b's column block moves to `ncols`, made for shells 0..ncap (the shells stored so far are a prefix of each half).
static int move_block(const PassCtx &P, Batch &B, int b, int ncap, double *ncols) {
  c2r_ctx *c = P.c;
  SrcRun &r = B.run[b];
  // probes in flight read this source's SrcDev entry: they must be through before the entry changes
  if (B.launched > B.settled) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_probe, 0));
  SrcDev &S = c->h_src[B.set][b];
  const size_t ncz = source_block_entries(c, r.ns, ncap);
  const size_t have = r.smax_prev >= 0 ? source_block_entries(c, r.ns, r.smax_prev) : 0;
  // the shells stored so far are a prefix of each half, the incoming triples and the outgoing ones (col_in, col_out)
  for (int half = 0; half < 2 && have > 0; half++)
    HIPCHK(c, hipMemcpyAsync(ncols + 3 * half * ncz, S.cols + 3 * half * S.cz, sizeof(double) * 3 * have,
                             hipMemcpyDeviceToDevice, c->stream));
  if (S.cz > 0) c->vacated[B.set].push_back(c2r_ctx::Segment{S.cols, 6 * S.cz}); // free for the batch's later moves
  S.cols = ncols;
  S.cz = ncz;
  r.cap = ncap;
  c->arena_stats[3]++;
  HIPCHK(c, hipMemcpyAsync(c->d_src[B.set] + b, &S, sizeof(SrcDev), hipMemcpyHostToDevice, c->stream));
  return 0;
}

// No room left on the device in the middle of a sweep.  Nothing of this batch has reached the rate grids yet, so the
// batch starts over with what this attempt has taught (sources that have stopped get the block they needed, those still
// growing the mesh limit) and, since even that did not fit, with fewer sources.  Returns START_OVER or 1 (error).
static int start_over(const PassCtx &P, Batch &B, int round) {
  c2r_ctx *c = P.c;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream_probe));
  // (round 5: a source still growing when the room ran out is given the mesh limit, not two rounds more -- at 512^3
  // the fronts of a whole batch race there together, and "two more" made every batch start over twice)
  const int limit_rounds = (c->g.smax + SUBBOXSIZE - 1) / SUBBOXSIZE;
  for (const SrcRun &r : B.run) {
    int &pn = c->prev_nbox[(size_t)r.ns - 1];
    pn = std::max(pn, r.active ? limit_rounds : r.nbox);
  }
  if (B.nb == 1) return fail(c, "column scratch: one source of this mesh does not fit in device memory");
  if (P.arena_log) fprintf(stderr, "c2ray_hip: column scratch, set %d: no room to grow in round %d, batch of %d starts over\n", B.set, round, B.nb);
  // the first time with the same sources: blocks made for what is known now need no moves, and what a move leaves
  // behind is most of what filled the set; a batch that runs out of room again is halved
  if (B.restarts++ > 0) B.nb = (B.nb + 1) / 2;
  c->arena_stats[4]++;
  return START_OVER;
}

// the shells s_lo..s_hi of `box` for the nact sources of d_list[set][act_off ..), on the sweep stream
static int launch_shells(PassCtx &P, Batch &B, const Box &box, int s_lo, int s_hi, size_t act_off, int nact) {
  c2r_ctx *c = P.c;
  SweepArgs SA;
  SA.g = c->g; SA.box = box; SA.sc = P.sc;
  SA.ndens = c->d_ndens; SA.xh_av = c->d_xh_av; SA.xhe_av = c->d_xhe_av;
  SA.lls_grid = c->lls_on_grid ? c->d_lls : nullptr;
  const int *act = c->h_list[B.set] + act_off;
  if (c->timing && !B.sweep_started) {
    HIPCHK(c, hipEventRecord(B.ev[0], c->stream));
    B.sweep_started = true;
  }
  for (int s = s_lo; s <= s_hi; s++) {
    // (a large batch waits at once: its many small faces would pay more for strided reads than the wait costs)
    if ((s >= TRANSPOSED_FROM_SHELL || B.nb > 16) && !P.transposed_seen) {
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_transposed, 0));
      P.transposed_seen = true;
    }
    SA.packed = SA.packedT = nullptr;
    if (P.transposed_seen || P.packed_early) SA.packed = c->d_stateT;
    if (P.transposed_seen) SA.packedT = c->d_stateT + 3 * c->g.ncell;
    int nblk = c->block_base[s + 1] - c->block_base[s];
    if (!c->periodic) {
      // the largest shell s among the active sources, each cut at its own reach; blocks beyond a source's own leave at once
      long long most = 0;
      for (int a = 0; a < nact; a++) {
        const Reach &R = B.run[act[a]].reach;
        most = std::max(most, reach_cells(R.l, R.r, s) - reach_cells(R.l, R.r, s - 1));
      }
      nblk = (int)((most + BLOCK - 1) / BLOCK);
      if (nblk == 0) continue;
    }
    // from 64 blocks on: a multiple of 8 blocks, one contiguous eighth of the shell per XCD (see the kernel)
    const int nlaunch = nblk >= 64 ? ((nblk + 7) & ~7) : nblk;
    for (int a = 0; a < nact; a++)
      if (s <= B.run[act[a]].smax) B.run[act[a]].sweep_threads += (long long)nlaunch * BLOCK;
    // (open boundaries: positions are below the cells of the source's reach -- at most the mesh's for a source inside it, and
    // fewer than 2^31 for one outside, which c2r_set_sources_external refuses otherwise: 32 bits hold them in every shell)
    const bool fast = s >= 2 && (s <= SHELL_FAST_MAX || !c->periodic) && !P.generic_sweep;
    if (fast && c->periodic)
      hipLaunchKernelGGL(k_sweep_shell_fast<false>, dim3(nlaunch, nact), dim3(BLOCK), 0, c->stream, SA, c->d_src[B.set],
                         c->d_list[B.set] + act_off, c->shell_geom[(size_t)s]);
    else if (fast && B.halo) // (a source with a halo of several faces in the batch: the entry kernels' twins that know edges and corners)
      hipLaunchKernelGGL(k_sweep_shell_fast_halo, dim3(nlaunch, nact), dim3(BLOCK), 0, c->stream, SA, c->d_src[B.set],
                         c->d_list[B.set] + act_off, c->shell_geom[(size_t)s], c->d_ent[B.set]);
    else if (fast && B.entry) // (a source with entry columns in the batch: the kernels that know vacuum cells and the ghost layer)
      hipLaunchKernelGGL(k_sweep_shell_fast_entry, dim3(nlaunch, nact), dim3(BLOCK), 0, c->stream, SA, c->d_src[B.set],
                         c->d_list[B.set] + act_off, c->shell_geom[(size_t)s], c->d_ent[B.set]);
    else if (fast && B.external) // (a source outside the mesh in the batch: the kernels that know vacuum cells)
      hipLaunchKernelGGL(k_sweep_shell_fast_ext, dim3(nlaunch, nact), dim3(BLOCK), 0, c->stream, SA, c->d_src[B.set],
                         c->d_list[B.set] + act_off, c->shell_geom[(size_t)s]);
    else if (fast)
      hipLaunchKernelGGL(k_sweep_shell_fast<true>, dim3(nlaunch, nact), dim3(BLOCK), 0, c->stream, SA, c->d_src[B.set],
                         c->d_list[B.set] + act_off, c->shell_geom[(size_t)s]);
    else if (c->periodic)
      hipLaunchKernelGGL(k_sweep_shell<false>, dim3(nlaunch, nact), dim3(BLOCK), 0, c->stream, SA, c->d_src[B.set], c->d_list[B.set] + act_off, s);
    else if (B.halo)
      hipLaunchKernelGGL(k_sweep_shell_halo, dim3(nlaunch, nact), dim3(BLOCK), 0, c->stream, SA, c->d_src[B.set], c->d_list[B.set] + act_off, s,
                         c->d_ent[B.set]);
    else if (B.entry)
      hipLaunchKernelGGL(k_sweep_shell_entry, dim3(nlaunch, nact), dim3(BLOCK), 0, c->stream, SA, c->d_src[B.set], c->d_list[B.set] + act_off, s,
                         c->d_ent[B.set]);
    else if (B.external)
      hipLaunchKernelGGL(k_sweep_shell_ext, dim3(nlaunch, nact), dim3(BLOCK), 0, c->stream, SA, c->d_src[B.set], c->d_list[B.set] + act_off, s);
    else
      hipLaunchKernelGGL(k_sweep_shell<true>, dim3(nlaunch, nact), dim3(BLOCK), 0, c->stream, SA, c->d_src[B.set], c->d_list[B.set] + act_off, s);
    c->tm.sweep_launches++;
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}

// The sub-box loop (evolve_source.F90:136-144).  After the shells of round r the loss through the box surface decides who
// sweeps round r+1; a quick lower bound of it (k_loss_probe_rounds) nearly always does.  When every active source went
// beyond round r in the previous pass (prev_nbox), round r+1 is launched at once for all of them, on trust, and the probe of
// round r is not even queued yet: the probes of all such rounds go out together, on their own stream, when a decision is
// really needed -- before a round that some source did not reach last time, or before the round that is everybody's last
// for geometric reasons -- so that the sweep stream carries shells and nothing else (a probe per round cost it an event,
// and 13-24 us of gap at each of the 12 round boundaries of a 256^3 sweep).  A source that turns out to have stopped at r
// keeps round r as its last -- its shells of later rounds are never looked at (the rates launch only sees the final box),
// so a wrong guess costs time, never a bit.  Returns 0, 1 (error) or START_OVER.
static int sweep_batch(PassCtx &P, Batch &B) {
  c2r_ctx *c = P.c;
  const Reach &reach = P.reach;
  B.list_used = 0;
  B.recs.clear();
  B.settled = B.launched = 0;
  B.sweep_started = false;
  const size_t acc_need = (size_t)B.nb * (size_t)(c->g.smax / SUBBOXSIZE + 3);
  if (c->probe_acc_cap < acc_need) {
    HIPCHK(c, hipStreamSynchronize(c->stream_probe));
    if (ensure_pair<double>(c, &c->d_probe_acc, &c->h_probe, &c->probe_acc_cap, acc_need)) return 1;
  }
  int *hl = c->h_list[B.set];
  size_t cur_off = 0; // the active list of the last round launched
  int cur_nact = 0;
  size_t acc_used = 0;
  for (int round = 1;; round++) {
    // the round's box: with open boundaries before it is cut at each source's reach (the kernels do that, source_box)
    const Box box = round_box(reach, round);
    int s_hi = 0; // the largest shell any source sweeps in this round
    // may this round start before the losses of the rounds before it are known?
    const bool ahead = round > 1 && cur_nact > 0 && all_reached(c, B, round);
    if (!ahead && settle_rounds(P, B)) return 1;
    // who sweeps this round: the while-test of evolve_source.F90:136-139 (its loss part taken on trust when ahead)
    int nact = 0;
    int *act = hl + B.list_used;
    int s_lo = 1 << 30;
    for (int b = 0; b < B.nb; b++) {
      SrcRun &r = B.run[b];
      if (!r.active) continue;
      // (entry columns: exactly the rounds given, as far as the box can grow; r.loss stays the flux, no probe ever writes it)
      if (!can_grow(c, r.reach, round_box(r.reach, r.nbox)) || (r.entry_rounds > 0 && r.nbox >= r.entry_rounds) ||
          !(ahead || r.loss > C2R_F(1e-10) * r.total_flux)) {
        r.active = false;
        continue;
      }
      r.nbox = round;
      act[nact++] = b;
      s_lo = std::min(s_lo, r.smax_prev + 1);
      s_hi = std::max(s_hi, box_smax(round_box(r.reach, round)));
    }
    if (nact == 0) return settle_rounds(P, B);
    if (s_hi > c->g.smax) return fail(c, "internal: shell %d beyond smax %d", s_hi, c->g.smax);
    // blocks too small for this round move to larger ones
    for (int a = 0; a < nact; a++) {
      const int cap = B.run[act[a]].cap;
      // (open boundaries: shells beyond a source's own reach hold no cell of it)
      const int need = std::min(s_hi, B.run[act[a]].smax);
      if (cap >= need) continue;
      const int ncap = std::min(B.run[act[a]].smax, std::max(need, 2 * cap));
      double *ncols = arena_alloc(c, B.set, source_block_doubles(c, B.run[act[a]].ns, ncap));
      if (!ncols) return start_over(P, B, round);
      if (move_block(P, B, act[a], ncap, ncols)) return 1;
    }
    // the same sources as in the last round: the list is on the device already
    size_t act_off = B.list_used;
    if (cur_nact == nact && round > 1 && std::equal(act, act + nact, hl + cur_off)) {
      act_off = cur_off;
    } else {
      HIPCHK(c, hipMemcpyAsync(c->d_list[B.set] + B.list_used, act, sizeof(int) * nact, hipMemcpyHostToDevice, c->stream));
      B.list_used += (size_t)nact;
    }
    cur_off = act_off;
    cur_nact = nact;
    if (launch_shells(P, B, box, s_lo, s_hi, act_off, nact)) return 1;
    bool any_can_grow = false, any_can_grow_twice = false; // ... after this round, after the next one
    for (int a = 0; a < nact; a++) {
      SrcRun &r = B.run[hl[act_off + a]];
      r.smax_prev = std::min(s_hi, r.smax);
      // (a source with entry columns goes on while it has rounds left)
      const bool more = r.entry_rounds == 0 || round < r.entry_rounds, more2 = r.entry_rounds == 0 || round + 1 < r.entry_rounds;
      any_can_grow = any_can_grow || (more && can_grow(c, r.reach, round_box(r.reach, round)));
      any_can_grow_twice = any_can_grow_twice || (more2 && can_grow(c, r.reach, round_box(r.reach, round + 1)));
    }
    if (!any_can_grow) {
      // The while-test after this round fails whatever the loss: the round is every active source's last, and
      // its loss (the one that is kept, evolve_source.F90:233) is queued behind the rates launch (queue_kept_losses).
      // The rounds before it are decided now; their probes were queued before this round's shells.
      if (settle_rounds(P, B)) return 1;
      for (int a = 0; a < nact; a++) {
        SrcRun &r = B.run[hl[act_off + a]];
        if (!r.active) continue; // stopped a round earlier after all
        r.final_loss_due = true;
        r.active = false;
      }
      return 0;
    }
    // The loss of this round decides whether a source goes on.
    RoundRec R;
    R.round = round; R.nact = nact; R.s_lo = s_lo; R.s_hi = s_hi; R.off = act_off; R.acc_off = acc_used; R.box = box;
    if (B.entry) {
      // no loss decides for a source with entry columns, and no probe is launched for it: the round's record lists the others
      int *pl = hl + B.list_used, np = 0;
      for (int a = 0; a < nact; a++)
        if (B.run[hl[act_off + a]].entry_rounds == 0) pl[np++] = hl[act_off + a];
      if (np == 0) continue; // (nobody to decide about)
      if (np < nact) {
        HIPCHK(c, hipMemcpyAsync(c->d_list[B.set] + B.list_used, pl, sizeof(int) * np, hipMemcpyHostToDevice, c->stream));
        R.off = B.list_used;
        R.nact = np;
        B.list_used += (size_t)np;
      }
    }
    acc_used += (size_t)R.nact;
    B.recs.push_back(R);
    // Its probe goes out now if the next round needs the answer before it can start (somebody may stop here) or if
    // the next round is the last for geometric reasons (the probes then run beside its shells, and the answers
    // are there when the rates launch has to be put together); otherwise it waits for company.
    const bool next_is_last = !any_can_grow_twice;
    if ((!all_reached(c, B, round + 1) || next_is_last) && launch_probes(P, B)) return 1;
  }
}

static FaceLayout face_layout(const c2r_ctx *c) {
  FaceLayout L;
  L.n[0] = c->g.n1; L.n[1] = c->g.n2; L.n[2] = c->g.n3;
  for (int d = 0; d < 3; d++) L.open[d] = c->per[d] ? 0 : 1;
  return L;
}

// The escape-map terms of a batch whose SrcDev records, final boxes included, are on their way to the device on the sweep
// stream: one launch, a block row per face (the rows of periodic axes leave at once).
static int queue_face_loss(const PassCtx &P, const Batch &B) {
  c2r_ctx *c = P.c;
  const FaceLayout L = face_layout(c);
  int most = 0;
  for (int d = 0; d < 3; d++)
    if (L.open[d]) most = std::max(most, face_cells(L.n, d));
  const dim3 grid((unsigned)((most + BLOCK - 1) / BLOCK), 6);
  with_flag(P.multi, [&](auto multi) {
    hipLaunchKernelGGL(k_face_loss<decltype(multi)::value>, grid, dim3(BLOCK), 0, c->stream, L, c->d_src[B.set], B.nb, P.sc, c->d_bands, P.ss,
                       c->d_face_maps);
  });
  HIPCHK(c, hipGetLastError());
  c->tm.sweep_launches++;
  return 0;
}

// The horizon loss of a batch whose SrcDev records, final boxes included, are on their way to the device on the sweep
// stream: one launch with a block row per horizoned source that traced anything, one that adds each row's block sums, and
// the copy of the sums to the host, where resolve_tails finds them once the set's rates launch is through (it waits for
// this stream).  The last row's terms stay in d_rim_terms (c2r_download_horizon_rim).
static int queue_horizon_rim(const PassCtx &P, Batch &B) {
  c2r_ctx *c = P.c;
  const int set = B.set;
  int *hl = c->h_rim_list[set];
  int nh = 0;
  long long most = 0;
  for (int b = 0; b < B.nb; b++) {
    const SrcDev &S = c->h_src[set][b];
    if (!(S.cut & CUT_HORIZON) || B.run[b].nbox == 0) continue;
    const long long T = rim_total(rim_extent(S.lo[0], S.hi[0]), rim_extent(S.lo[1], S.hi[1]), rim_extent(S.lo[2], S.hi[2]));
    if (T > (long long)c->rim_terms_cap)
      return fail(c, "internal: the %lld sheet columns of source %d do not fit the %zu of the mesh", T, B.run[b].ns, c->rim_terms_cap);
    most = std::max(most, T);
    hl[nh++] = b;
    B.rim_ns.push_back(B.run[b].ns);
  }
  if (nh == 0) return 0;
  const int nblk = (int)((most + BLOCK - 1) / BLOCK);
  const size_t need = (size_t)nblk * (size_t)nh;
  if (c->rim_partial_cap[set] < need) {
    HIPCHK(c, hipStreamSynchronize(c->stream)); // an earlier batch's launches may still use the old buffer
    if (ensure_pair<double>(c, &c->d_rim_partial[set], (double **)nullptr, &c->rim_partial_cap[set], need)) return 1;
  }
  HIPCHK(c, hipMemcpyAsync(c->d_rim_list[set], hl, sizeof(int) * nh, hipMemcpyHostToDevice, c->stream));
  with_flag(P.multi, [&](auto multi) { with_flag(!c->periodic, [&](auto open) {
    const auto kernel = k_horizon_rim<decltype(multi)::value, decltype(open)::value>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)nblk, (unsigned)nh), dim3(BLOCK), 0, c->stream, c->d_src[set], c->d_rim_list[set], P.sc,
                       c->d_bands, P.ss, c->d_rim_partial[set], nblk, c->d_rim_terms);
  }); });
  hipLaunchKernelGGL(k_loss_finish, dim3(nh), dim3(BLOCK), 0, c->stream, c->d_rim_partial[set], nblk, nblk, c->d_rim_acc[set]);
  HIPCHK(c, hipGetLastError());
  c->tm.sweep_launches += 2;
  HIPCHK(c, hipMemcpyAsync(c->h_rim[set], c->d_rim_acc[set], sizeof(double) * nh, hipMemcpyDeviceToHost, c->stream));
  const SrcDev &L = c->h_src[set][hl[nh - 1]];
  c->rim_last_ns = B.rim_ns.back();
  for (int d = 0; d < 3; d++) c->rim_last_ext[d] = rim_extent(L.lo[d], L.hi[d]);
  c->rim_last_stamp = P.stamp;
  return 0;
}

// Exit strips (c2r_select_source_face_exit).  Does the batch hold a selected source?
static bool batch_has_face_exit(const c2r_ctx *c, const Batch &B) {
  for (const c2r_ctx::FaceExit &x : c->face_exit)
    for (int ns : x.sources)
      for (const SrcRun &r : B.run)
        if (r.ns == ns) return true;
  return false;
}
// The strips of the batch's selected sources, face by face: one gather launch per face (k_source_face_exit) on the sweep
// stream, behind the upload of the records with the final boxes; and what the host knows of each strip -- the rounds, whether
// the final box met the layer, the pass.
static int queue_source_face_exit(const PassCtx &P, Batch &B) {
  c2r_ctx *c = P.c;
  const int mesh[3] = {c->g.n1, c->g.n2, c->g.n3};
  for (int face = 0; face < 6; face++) {
    c2r_ctx::FaceExit &x = c->face_exit[face];
    if (x.sources.empty()) continue;
    const int axis = face >> 1, high = face & 1;
    int *pairs = c->h_list[B.set] + B.list_used, np = 0;
    for (size_t k = 0; k < x.sources.size(); k++)
      for (int b = 0; b < B.nb; b++) {
        const SrcRun &r = B.run[b];
        if (r.ns != x.sources[k]) continue;
        pairs[2 * np] = b;
        pairs[2 * np + 1] = (int)k;
        np++;
        // does the final box hold a cell of the layer?  Along the face's axis the layer's offset; across it any mesh cell
        const Box fb = round_box(r.reach, r.nbox);
        const int *p = &c->srcpos[3 * (size_t)(r.ns - 1)];
        bool met = r.nbox > 0;
        for (int d = 0; d < 3 && met; d++) {
          if (d == axis) {
            const int off = (high ? mesh[d] : 1) - p[d];
            met = off >= fb.lo[d] && off <= fb.hi[d];
          } else if (!c->per[d]) {
            met = std::max(fb.lo[d], 1 - p[d]) <= std::min(fb.hi[d], mesh[d] - p[d]);
          }
        }
        x.rounds[k] = r.nbox;
        x.reached[k] = met ? 1 : 0;
        x.stamp[k] = P.stamp;
      }
    if (np == 0) continue;
    HIPCHK(c, hipMemcpyAsync(c->d_list[B.set] + B.list_used, pairs, sizeof(int) * 2 * np, hipMemcpyHostToDevice, c->stream));
    const size_t F = (size_t)c->g.ncell / (size_t)mesh[axis];
    hipLaunchKernelGGL(k_source_face_exit, dim3((unsigned)((F + BLOCK - 1) / BLOCK), (unsigned)np), dim3(BLOCK), 0, c->stream, c->g,
                       c->d_src[B.set], c->d_list[B.set] + B.list_used, face, x.d_cols);
    HIPCHK(c, hipGetLastError());
    c->tm.sweep_launches++;
    B.list_used += (size_t)(2 * np);
  }
  return 0;
}

// Final sub-boxes for the rates launch, what the next pass learns from this one (prev_nbox, prev_grow), the upload of the
// SrcDev entries; then the rates stream takes the batch over.
static int close_boxes(PassCtx &P, Batch &B) {
  c2r_ctx *c = P.c;
  for (int b = 0; b < B.nb; b++) {
    SrcRun &r = B.run[b];
    SrcDev &S = c->h_src[B.set][b];
    const Box fb = round_box(r.reach, r.nbox);
    for (int d = 0; d < 3; d++) { S.lo[d] = fb.lo[d]; S.hi[d] = fb.hi[d]; }
    // Open boundaries: the loss that decided -- through the faces that could still move -- is not the one that is kept:
    // photon_loss takes what leaves through the WHOLE surface of the final box, mesh faces included, whichever way the
    // loop ended.  Every source that traced anything owes that sum.
    if (!c->periodic) r.final_loss_due = r.nbox > 0;
    // a source whose while-test failed before the first sub-box (a mesh only two cells deep) traced nothing:
    // an empty box, so that no cell passes the in-box test
    if (r.nbox == 0) { S.lo[0] = 1; S.hi[0] = 0; }
    // the terms of the kept loss of a round that was the last for geometric reasons come out of the rates launch: the
    // surface cells in the shells of that round (heating kernels do not keep photo_out, see k_rates)
    S.loss_lo = -1;
    // (a batch with a source outside the mesh: the surface of such a box has vacuum cells, which no rates launch visits --
    // the kept losses of the whole batch are evaluated by k_loss from the columns, as in a heating run, the same bits)
    if (r.final_loss_due && c->isothermal && !B.external)
      S.loss_lo = c->periodic && r.nbox > 1 ? box_smax(round_box(P.reach, r.nbox - 1)) + 1 : 0; // (open: every shell of the box)
    // (known0: what was known before this batch -- a batch that started over has raised prev_nbox meanwhile)
    const int known = B.known0[(size_t)b];
    c->prev_grow[(size_t)r.ns - 1] = known > 0 ? std::max(0, r.nbox - known) : 0;
    c->prev_nbox[(size_t)r.ns - 1] = r.nbox;
    c2r_source_trace &T = c->trace[(size_t)r.ns - 1];
    for (int d = 0; d < 3; d++) {
      T.reach_l[d] = r.reach.l[d]; T.reach_r[d] = r.reach.r[d];
      T.box_lo[d] = r.nbox > 0 ? fb.lo[d] : 0; T.box_hi[d] = r.nbox > 0 ? fb.hi[d] : 0;
    }
    T.nbox = r.nbox;
    T.block_shells = r.cap;
    T.block_cells = (long long)S.cz;
    T.swept_cells = r.nbox > 0 ? box_cells(fb) : 0;
    T.sweep_threads = r.sweep_threads;
    c->trace_stamp[(size_t)r.ns - 1] = P.stamp;
  }
  // Escape maps: the batch's terms, here -- the final boxes are known, the batch will not start over, and the N_in(HI)
  // slots still hold columns (the rates launch, which waits for the event below, overwrites them where SrcDev::loss_lo
  // asks it to).  The records go up first, and the kernel counts into the sweep's span.
  // Horizon loss: likewise, for the sources of the batch that have a finite horizon and traced anything.
  B.rim_ns.clear();
  bool rim = false;
  if (c->rim_on)
    for (int b = 0; b < B.nb && !rim; b++) rim = (c->h_src[B.set][b].cut & CUT_HORIZON) && B.run[b].nbox > 0;
  const bool maps = c->d_face_maps != nullptr;
  // Exit strips (c2r_select_source_face_exit): likewise, for the selected sources of the batch -- after their last round, with
  // the final boxes in the records, before the column blocks are given back.
  const bool exits = batch_has_face_exit(c, B);
  if (maps || rim || exits) {
    if (c->timing && !B.sweep_started) {
      HIPCHK(c, hipEventRecord(B.ev[0], c->stream));
      B.sweep_started = true;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_src[B.set], c->h_src[B.set], sizeof(SrcDev) * B.nb, hipMemcpyHostToDevice, c->stream));
    if (maps && queue_face_loss(P, B)) return 1;
    if (rim && queue_horizon_rim(P, B)) return 1;
    if (exits && queue_source_face_exit(P, B)) return 1;
  }
  if (c->timing) { // the sweep's span: from the first shell launch to the last, record uploads on either side left out
    if (!B.sweep_started) HIPCHK(c, hipEventRecord(B.ev[0], c->stream));
    HIPCHK(c, hipEventRecord(B.ev[1], c->stream));
  }
  if (!maps && !rim && !exits) HIPCHK(c, hipMemcpyAsync(c->d_src[B.set], c->h_src[B.set], sizeof(SrcDev) * B.nb, hipMemcpyHostToDevice, c->stream));
  if (!P.transposed_seen) {
    // small boxes only: nobody needed the copies, but whatever follows this sweep (the global pass rewrites the
    // state) has to come after the kernel that reads it
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_transposed, 0));
    P.transposed_seen = true;
  }
  HIPCHK(c, hipEventRecord(c->ev_sweep_done[B.set], c->stream));
  // rates of the whole batch, in source order, on the second stream
  HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_sweep_done[B.set], 0));
  if (c->timing) HIPCHK(c, hipEventRecord(B.ev[2], c->stream2));
  return 0;
}

// Tiles (8 x 8 x 4 cells) that intersect the final sub-box of some source of the batch, and per tile the sources that do,
// copied to the device on the rates stream; B.ntiles = 0 when every tile of the mesh walks every source of the batch.
static int build_tile_lists(const PassCtx &P, Batch &B) {
  c2r_ctx *c = P.c;
  const Grid &g = c->g;
  const int mesh[3] = {g.n1, g.n2, g.n3};
  const int nt1 = (g.n1 + 7) / 8, nt2 = (g.n2 + 7) / 8, nt3 = (g.n3 + 3) / 4;
  const int nblk = nt1 * nt2 * nt3;
  B.ntiles = 0;
  bool full = false;
  // The final box of a source as far as it lies in the mesh: along an open axis the box of a source outside the mesh runs
  // through vacuum, which has no tiles -- cut there at the mesh faces (for a source inside, the box lies in the mesh and the
  // cut does nothing); false: no cell of the box is a mesh cell
  auto mesh_box = [&](int b, Box &fb) {
    fb = round_box(B.run[b].reach, B.run[b].nbox);
    const int *p = &c->srcpos[3 * (size_t)(B.run[b].ns - 1)];
    for (int d = 0; d < 3; d++) {
      if (c->per[d]) continue;
      fb.lo[d] = std::max(fb.lo[d], 1 - p[d]);
      fb.hi[d] = std::min(fb.hi[d], mesh[d] - p[d]);
      if (fb.lo[d] > fb.hi[d]) return false;
    }
    return true;
  };
  for (int b = 0; b < B.nb && !full; b++) {
    Box fb;
    full = B.run[b].nbox > 0 && mesh_box(b, fb);
    for (int d = 0; d < 3; d++) full = full && (fb.hi[d] - fb.lo[d] + 1 >= mesh[d]);
  }
  // few sources one of which fills the mesh: every cell simply walks all of them
  if (full && B.nb <= 16) return 0;
  std::vector<int> &cnt = c->tile_count;
  cnt.assign((size_t)nblk, 0);
  std::vector<int> cov[3];
  const int tsz[3] = {8, 8, 4}, ntd[3] = {nt1, nt2, nt3};
  auto covered = [&](int b) {
    Box fb; // (an open axis: cut at the mesh faces, so the modulo below does nothing there)
    for (int d = 0; d < 3; d++) cov[d].clear();
    if (!mesh_box(b, fb)) return;
    const int *p = &c->srcpos[3 * (size_t)(B.run[b].ns - 1)];
    for (int d = 0; d < 3; d++) {
      int last = -1;
      std::vector<unsigned char> seen((size_t)ntd[d], 0);
      for (int o = fb.lo[d]; o <= fb.hi[d]; o++) {
        int x = (p[d] - 1 + o) % mesh[d];
        if (x < 0) x += mesh[d];
        const int t = x / tsz[d];
        if (t != last && !seen[t]) { seen[t] = 1; cov[d].push_back(t); }
        last = t;
      }
    }
  };
  size_t total = 0;
  for (int b = 0; b < B.nb; b++) {
    if (B.run[b].nbox == 0) continue;
    covered(b);
    for (int tk : cov[2])
      for (int tj_ : cov[1]) {
        int *row = &cnt[((size_t)tk * nt2 + tj_) * nt1];
        for (int ti_ : cov[0]) row[ti_]++;
      }
    total += cov[0].size() * cov[1].size() * cov[2].size();
  }
  const int set = B.set;
  if (ensure_pair<int>(c, &c->d_tsrc[set], &c->h_tsrc[set], &c->tsrc_cap[set], total + 1)) return 1;
  int *list = c->h_tiles[set], *tp = c->h_tptr[set], *tsrc = c->h_tsrc[set];
  int ntl = 0;
  size_t acc = 0;
  for (int t = 0; t < nblk; t++) {
    if (!cnt[t]) { cnt[t] = -1; continue; }
    list[ntl] = t;
    tp[ntl] = (int)acc;
    acc += (size_t)cnt[t];
    cnt[t] = ntl++; // from count to position in the list
  }
  if (ntl == 0) { list[0] = 0; tp[0] = 0; ntl = 1; }
  tp[ntl] = (int)acc;
  std::vector<int> fill(tp, tp + ntl);
  for (int b = 0; b < B.nb; b++) { // ascending b: every tile's sources end up in source order
    if (B.run[b].nbox == 0) continue;
    covered(b);
    for (int tk : cov[2])
      for (int tj_ : cov[1]) {
        const int *row = &cnt[((size_t)tk * nt2 + tj_) * nt1];
        for (int ti_ : cov[0]) tsrc[fill[row[ti_]]++] = b;
      }
  }
  HIPCHK(c, hipMemcpyAsync(c->d_tiles[set], list, sizeof(int) * (size_t)ntl, hipMemcpyHostToDevice, c->stream2));
  HIPCHK(c, hipMemcpyAsync(c->d_tptr[set], tp, sizeof(int) * (size_t)(ntl + 1), hipMemcpyHostToDevice, c->stream2));
  if (acc > 0) HIPCHK(c, hipMemcpyAsync(c->d_tsrc[set], tsrc, sizeof(int) * acc, hipMemcpyHostToDevice, c->stream2));
  B.ntiles = ntl;
  return 0;
}

// The rates of the batch on the rates stream: a pending zeroing of the rate grids first, then one launch, or for the last
// batch of a pass the caller takes slab by slab, one launch per slab with an event behind each.
static int launch_rates(const PassCtx &P, Batch &B, bool last_batch) {
  c2r_ctx *c = P.c;
  const bool lists = B.ntiles > 0;
  const size_t nc = c->g.ncell;
  // a pending set_rates_to_zero: this launch writes the grids if it covers every cell, else they are zeroed now
  // (on the rates stream, which this batch's launches follow)
  int fresh = 0;
  if (c->rates_zero_pending) {
    if (!lists) {
      fresh = 1;
      c->rates_zero_pending = false;
      if (c->isothermal && c->phiheat_dirty) { // phiheat of an earlier heating step: not written by this launch
        HIPCHK(c, zero_device(c->d_rates + 3 * nc, sizeof(double) * nc, c->stream2));
        c->phiheat_dirty = false;
      }
    } else {
      c->rates_zero_pending = false;
      c->phiheat_dirty = false;
      // (the four grids only: the tail of the buffer is written at the end of this pass, on the other stream)
      HIPCHK(c, zero_device(c->d_rates, sizeof(double) * 4 * nc, c->stream2));
    }
  }
  if (!c->isothermal) c->phiheat_dirty = true;
  const bool slabs = last_batch && P.nslab > 0;
  const int pieces = slabs ? P.nslab : 1;
  const int per_layer = ((c->g.n1 + 7) / 8) * ((c->g.n2 + 7) / 8), nt3 = (c->g.n3 + 3) / 4;
  // slabs alternate between two streams so that the thin tail of one launch overlaps the start of the
  // next; the third stream is forked from (and joined back into) the rates stream, which carries the
  // dependencies on the sweep, on earlier batches and on the tile-list copy
  if (pieces > 1) {
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream2));
    HIPCHK(c, hipStreamWaitEvent(c->stream3, c->ev_fork, 0));
  }
  for (int piece = 0; piece < pieces; piece++) {
    hipStream_t st = (pieces > 1 && (piece & 1)) ? c->stream3 : c->stream2;
    // tiles of the layers [l0, l1): a contiguous range of tile ids, hence of the (sorted) list too
    const int l0 = pieces == 1 ? 0 : c->slab_k[piece] / 4;
    const int l1 = pieces == 1 ? nt3 : (c->slab_k[piece + 1] + 3) / 4;
    int base, cnt;
    if (lists) {
      const int *list = c->h_tiles[B.set];
      base = (int)(std::lower_bound(list, list + B.ntiles, l0 * per_layer) - list);
      cnt = (int)(std::lower_bound(list, list + B.ntiles, l1 * per_layer) - list) - base;
    } else {
      base = l0 * per_layer;
      cnt = (l1 - l0) * per_layer;
    }
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(cnt), dim3(BLOCK), 0, st, c->g, c->d_src[B.set], B.nb, P.sc, c->d_ndens, c->d_xh_av, c->d_xhe_av,
                         c->d_bands, P.ss, c->d_rates, lists ? c->d_tiles[B.set] : nullptr, lists ? c->d_tptr[B.set] : nullptr,
                         lists ? c->d_tsrc[B.set] : nullptr, base, fresh, P.rt);
    };
    if (cnt > 0)
      with_flag(!c->isothermal, [&](auto heat) { with_flag(P.multi, [&](auto multi) { with_flag(!c->periodic, [&](auto open) {
        constexpr bool H = decltype(heat)::value, M = decltype(multi)::value, O = decltype(open)::value;
        // some source of the batch has a beam or a horizon: the kernel that asks (c2r_set_source_beams, _horizons)
        // ... or a curve: the kernel whose flux is a value per lane (c2r_set_source_curves)
        if (B.curved) go(k_rates_curve<H, M, O>);
        else if (B.beamed) go(k_rates_beam<H, M, O>);
        else go(k_rates<H, M, O>);
      }); }); });
    if (slabs) HIPCHK(c, hipEventRecord(c->ev_slab[piece], st));
  }
  if (pieces > 1) {
    HIPCHK(c, hipEventRecord(c->ev_join, c->stream3));
    HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_join, 0));
  }
  HIPCHK(c, hipGetLastError());
  c->tm.rates_launches++;
  if (c->timing) HIPCHK(c, hipEventRecord(B.ev[3], c->stream2));
  if (c->timing && slabs && c->ev_ct[0]) { // c2r_get_comm_timing: this device's last slab of rates is complete
    HIPCHK(c, hipEventRecord(c->ev_ct[0], c->stream2));
    c->ct_rates_recorded = true;
  }
  return 0;
}

// The losses that are kept but decided nothing (rounds that were a source's last for geometric reasons), one group of sources
// per such round (the same for every source of a mesh, so one group).  Isothermal: the rates launch has left their terms in
// the column blocks; they are added up behind it, on its stream, and the sums go to the host to be resolved later
// (resolve_tails).  Heating, and a batch with a source outside the mesh (close_boxes): boundary_loss evaluates them now.  The batch's losses and sub-box counts join c->tails.
static int queue_kept_losses(const PassCtx &P, Batch &B) {
  c2r_ctx *c = P.c;
  const int set = B.set;
  c2r_ctx::BatchTail bt;
  bt.set = set;
  bt.slot.assign((size_t)B.nb, -1);
  for (const SrcRun &r : B.run) {
    bt.loss.push_back(r.loss);
    bt.nbox.push_back(r.nbox);
  }
  int nslot = 0;
  for (;;) {
    int fr = -1;
    for (int b = 0; b < B.nb && fr < 0; b++)
      if (B.run[b].final_loss_due) fr = B.run[b].nbox;
    if (fr < 0) break;
    int *fl = c->h_list[set] + B.list_used;
    int nf = 0;
    for (int b = 0; b < B.nb; b++)
      if (B.run[b].final_loss_due && B.run[b].nbox == fr) {
        fl[nf++] = b;
        B.run[b].final_loss_due = false;
      }
    // (open boundaries: fb is cut at each source's reach by the kernels; the whole surface of the final box, all its shells)
    const Box fb = round_box(P.reach, fr);
    int f_lo = fr > 1 ? box_smax(round_box(P.reach, fr - 1)) + 1 : 0, f_hi = box_smax(fb);
    if (!c->periodic) {
      f_lo = f_hi = 0;
      for (int j = 0; j < nf; j++) f_hi = std::max(f_hi, box_smax(round_box(B.run[fl[j]].reach, fr)));
    }
    if (c->isothermal && !B.external) {
      HIPCHK(c, hipMemcpyAsync(c->d_list[set] + B.list_used, fl, sizeof(int) * nf, hipMemcpyHostToDevice, c->stream2));
      const int nblk = c->block_base[f_hi + 1] - c->block_base[f_lo];
      const size_t need = (size_t)nblk * (size_t)nf;
      if (c->final_partial_cap[set] < need) {
        HIPCHK(c, hipStreamSynchronize(c->stream2));
        if (ensure_pair<double>(c, &c->d_final_partial[set], (double **)nullptr, &c->final_partial_cap[set], need)) return 1;
      }
      const int first_block = c->periodic ? blocks_before_surface(c, fb, f_lo, f_hi) : 0;
      if (first_block > 0) HIPCHK(c, zero_device(c->d_final_partial[set], sizeof(double) * need, c->stream2));
      if (c->periodic)
        hipLaunchKernelGGL(k_loss_stored<false>, dim3(nblk - first_block, nf), dim3(BLOCK), 0, c->stream2, c->g, c->d_src[set],
                           c->d_list[set] + B.list_used, f_lo, f_hi, fb, c->d_block_base, c->d_final_partial[set], nblk, first_block);
      else
        hipLaunchKernelGGL(k_loss_stored<true>, dim3(nblk - first_block, nf), dim3(BLOCK), 0, c->stream2, c->g, c->d_src[set],
                           c->d_list[set] + B.list_used, f_lo, f_hi, fb, c->d_block_base, c->d_final_partial[set], nblk, first_block);
      hipLaunchKernelGGL(k_loss_finish, dim3(nf), dim3(BLOCK), 0, c->stream2, c->d_final_partial[set], nblk, nblk,
                         c->d_final_acc[set] + nslot);
      HIPCHK(c, hipGetLastError());
      for (int j = 0; j < nf; j++) bt.slot[(size_t)fl[j]] = nslot + j;
      nslot += nf;
    } else {
      HIPCHK(c, hipMemcpyAsync(c->d_list[set] + B.list_used, fl, sizeof(int) * nf, hipMemcpyHostToDevice, c->stream));
      if (boundary_loss(c, set, B.list_used, nf, f_lo, f_hi, fb, P.sc, P.ss, P.multi, false, B.entry ? c->d_ent[set] : nullptr)) return 1;
      for (int j = 0; j < nf; j++) bt.loss[(size_t)fl[j]] = c->h_loss[j];
    }
    B.list_used += (size_t)nf;
  }
  if (nslot > 0) HIPCHK(c, hipMemcpyAsync(c->h_final[set], c->d_final_acc[set], sizeof(double) * nslot, hipMemcpyDeviceToHost, c->stream2));
  bt.rim_ns = B.rim_ns; // (c2r_enable_horizon_loss: their sums are on their way to h_rim[set] on the sweep stream)
  bt.rim_loss.assign(bt.rim_ns.size(), 0.0);
  bt.resolved = nslot == 0 && bt.rim_ns.empty();
  c->tails.push_back(std::move(bt));
  return 0;
}

// The share of one caller in the static deal (do_grid_static): first, first + stride, ... over the point sources
// 1..NumSrc and, behind them, the planes NumSrc + 1 .. NumSrc + nplane.
static std::vector<int> dealt_share(const c2r_ctx *c, int first, int stride) {
  std::vector<int> mine;
  for (int ns = first; ns <= c->nsrc + c->nplane; ns += stride) mine.push_back(ns);
  return mine;
}

#include "c2ray_planes.inc" // the plane kernels, run_planes, the plane buffers and the c2r_*plane* entry points

// nslab > 0: the caller wants to consume the rate grids slab by slab (z ranges) while later slabs are
// still being computed: the rates launch of the LAST batch is cut into nslab launches, an event is
// recorded after each, and the final synchronisation is left to pass_finish.
// `dealt`: the caller's share of the deal -- point sources 1..NumSrc and planes NumSrc + 1 .. (dealt_share).  The planes
// are added first, in plane order, then the point sources as they always were.
static int pass_list(c2r_ctx *c, const std::vector<int> &dealt, int nslab = 0) {
  HIPCHK(c, hipSetDevice(c->device));
  if (c->pass_open) return fail(c, "previous c2r_pass_sources_begin was not closed by c2r_pass_sources_end");
  std::vector<int> mine, planes;
  for (int ns : dealt) {
    if (ns > c->nsrc) planes.push_back(ns - c->nsrc - 1);
    else mine.push_back(ns);
  }
  struct InPass {
    c2r_ctx *c;
    explicit InPass(c2r_ctx *c_) : c(c_) { c->in_pass = true; }
    ~InPass() { c->in_pass = false; }
  } in_pass_guard(c);
  static const bool generic_sweep = getenv("C2R_SWEEP_GENERIC") && atoi(getenv("C2R_SWEEP_GENERIC")) > 0;
  static const bool arena_log = getenv("C2R_ARENA_LOG") != nullptr;
  // (an open axis: the reach of a source in the far corner on either side -- what no source's box exceeds)
  Reach widest = mesh_reach(c->g);
  if (!c->periodic) {
    const int mesh[3] = {c->g.n1, c->g.n2, c->g.n3};
    for (int d = 0; d < 3; d++)
      // (... or of a source outside the mesh, through the vacuum: c->ext_smax)
      if (!c->per[d]) { widest.r[d] = std::max(c->ext_smax, std::min(MAX_SUBBOX, mesh[d] - 1)); widest.l[d] = -widest.r[d]; }
  }
  PassCtx P{c, scalars(c), SedSet(), false, widest, generic_sweep, arena_log};
  P.ss = sedset(c, &P.multi);
  if (rates_tables(c, P.sc, P.rt)) return 1;
  c->tm.sweep_ms = c->tm.rates_ms = 0.0;
  c->tm.sweep_launches = c->tm.rates_launches = 0;
  c->tm.cells_swept = 0;
  c->ev_used = 0;
  c->ct_rates_recorded = false;
  // every pass is closed by pass_finish, which adds the batches' kept losses into photon_loss / sum_nbox and empties
  // this list; entries still here belong to a pass that ended in an error and must not be added to this one
  c->tails.clear();
  if (c->prev_nbox.size() != (size_t)c->nsrc) c->prev_nbox.assign((size_t)c->nsrc, 0);
  if (c->rim_on && c->horizon_loss.size() != (size_t)c->nsrc) c->horizon_loss.assign((size_t)c->nsrc, 0.0);
  if (c->trace.size() != (size_t)c->nsrc) {
    c->trace.assign((size_t)c->nsrc, c2r_source_trace{});
    c->trace_stamp.assign((size_t)c->nsrc, 0);
  }
  static std::atomic<long long> passes{0};
  P.stamp = ++passes;
  // a rank without sources writes nothing: a pending zeroing of the rate grids has to happen for real
  if (mine.empty() && flush_rates_zero(c)) return 1;
  // planes add to the grids, so for them too; they are queued here, in front of the event the rates stream waits for:
  // the point sources' rates launches then accumulate on top of them, and a pass without point sources records its slab
  // events behind them
  c->pass_planes.clear();
  if (!planes.empty() && (flush_rates_zero(c) || run_planes(P, planes))) return 1;
  // everything queued earlier on the main stream (state upload, zeroing of the rates) must be
  // visible to the rates stream
  HIPCHK(c, hipEventRecord(c->ev_sweep_done[0], c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_sweep_done[0], 0));
  if (queue_state_products(c)) return 1;
  P.packed_early = c->packed_valid;
  // slabs: tile layers (4 planes each) [slab_k[s] / 4, slab_k[s + 1] / 4), and an event for each
  const int nt3_all = (c->g.n3 + 3) / 4;
  P.nslab = nslab > 0 ? std::min(nslab, nt3_all) : 0;
  c->slab_k.assign(1, 0);
  for (int sidx = 1; sidx <= P.nslab; sidx++) c->slab_k.push_back(std::min(c->g.n3, 4 * (int)((long long)nt3_all * sidx / P.nslab)));
  while (c->ev_slab.size() < (size_t)P.nslab) {
    hipEvent_t e;
    HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->ev_slab.push_back(e);
  }
  if (c->prev_grow.size() != (size_t)c->nsrc) c->prev_grow.assign((size_t)c->nsrc, 0);
  const int batch_limit = std::min(c->batch, BATCH_MAX);
  for (size_t b0 = 0, bi = 0; b0 < mine.size(); bi++) {
    Batch B;
    B.set = (int)(bi & 1);
    B.b0 = b0;
    B.nb = (int)std::min<size_t>((size_t)batch_limit, mine.size() - b0);
    // this set's scratch may still be read by the rates launch of two batches ago, and its pinned lists may
    // still feed copies queued then
    if (c->set_busy[B.set]) {
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_rates_done[B.set], 0));
      HIPCHK(c, hipEventSynchronize(c->ev_rates_done[B.set]));
      resolve_tails(c, B.set); // h_final[set] is about to be written again
    }
    for (int b = 0; b < B.nb; b++) B.known0.push_back(c->prev_nbox[(size_t)mine[b0 + b] - 1]);
    for (hipEvent_t &e : B.ev)
      if (c->timing && pool_event(c, &e)) return 1;
    for (;;) {
      if (place_batch(P, mine, B)) return 1;
      const int r = sweep_batch(P, B);
      if (r == 0) break;
      if (r != START_OVER) return 1;
    }
    if (close_boxes(P, B)) return 1;
    if (build_tile_lists(P, B) || launch_rates(P, B, b0 + B.nb >= mine.size()) || queue_kept_losses(P, B)) return 1;
    if (c->timing) P.tev.insert(P.tev.end(), B.ev, B.ev + 4);
    HIPCHK(c, hipEventRecord(c->ev_rates_done[B.set], c->stream2));
    c->set_busy[B.set] = true;
    for (const SrcRun &r : B.run) c->tm.cells_swept += r.nbox > 0 ? box_cells(round_box(r.reach, r.nbox)) : 0;
    const SrcDev &S = c->h_src[B.set][B.nb - 1];
    c->last_src = B.run[B.nb - 1].ns;
    c->last_cols = S.cols;
    c->last_cz = S.cz;
    for (int d = 0; d < 3; d++) { c->last_lo[d] = S.lo[d]; c->last_hi[d] = S.hi[d]; }
    b0 += (size_t)B.nb;
  }
  if (!P.transposed_seen) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_transposed, 0));
  // a rank without sources of its own still owes the caller its slab events
  if (mine.empty()) {
    for (int sidx = 0; sidx < P.nslab; sidx++) HIPCHK(c, hipEventRecord(c->ev_slab[sidx], c->stream2));
    if (c->timing && P.nslab > 0 && c->ev_ct[0]) {
      HIPCHK(c, hipEventRecord(c->ev_ct[0], c->stream2));
      c->ct_rates_recorded = true;
    }
  }
  c->pass_tev = P.tev;
  c->pass_open = true;
  c->pass_slabs = P.nslab;
  if (nslab > 0) return 0;
  return pass_finish(c);
}

static int pass_finish(c2r_ctx *c) {
  if (!c->pass_open) return 0;
  if (sync_stream(c, c->stream2, "the pass (rates stream)")) return 1;
  if (sync_stream(c, c->stream, "the pass")) return 1;
  c->set_busy[0] = c->set_busy[1] = false;
  // photon_loss(1) += photon_loss_src ; sum_nbox += nbox  (evolve_source.F90:233-236): batch by batch, source by
  // source, now that the losses the rates launches left behind have arrived
  resolve_tails(c, 0);
  resolve_tails(c, 1);
  for (int p : c->pass_planes) { // the planes came first
    c->plane[p].loss = c->h_plane_loss[p];
    c->photon_loss[0] = c->photon_loss[0] + c->plane[p].loss;
    if (c->side_loss_on) // behind the far loss: side 0, then side 1 (0.0 for a side that was not live)
      for (int s = 0; s < 2; s++) {
        c->plane[p].side_loss[s] = c->plane[p].side_ran[s] ? c->h_side_loss[2 * p + s] : 0.0;
        c->photon_loss[0] = c->photon_loss[0] + c->plane[p].side_loss[s];
      }
  }
  c->pass_planes.clear();
  for (const c2r_ctx::BatchTail &bt : c->tails)
    for (size_t b = 0; b < bt.loss.size(); b++) {
      c->photon_loss[0] = c->photon_loss[0] + bt.loss[b];
      c->sum_nbox += bt.nbox[b];
    }
  for (const c2r_ctx::BatchTail &bt : c->tails) // horizon loss: loss[ns] = loss[ns] + (this pass's sum)
    for (size_t j = 0; j < bt.rim_ns.size(); j++) {
      double &hl = c->horizon_loss[(size_t)bt.rim_ns[j] - 1];
      hl = hl + bt.rim_loss[j];
    }
  c->tails.clear();
  // tail of the reduction buffer: photon_loss(1:47), sum_nbox
  std::memcpy(c->h_tail, c->photon_loss, sizeof c->photon_loss);
  c->h_tail[C2R_NFREQ] = (double)c->sum_nbox;
  HIPCHK(c, hipMemcpyAsync(c->d_rates + 4 * c->g.ncell, c->h_tail, sizeof(double) * (C2R_NFREQ + 1), hipMemcpyHostToDevice, c->stream));
  if (sync_stream(c, c->stream, "the pass")) return 1;
  const std::vector<hipEvent_t> &tev = c->pass_tev;
  for (size_t i = 0; i + 3 < tev.size(); i += 4) {
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, tev[i], tev[i + 1]));
    c->tm.sweep_ms += ms;
    HIPCHK(c, hipEventElapsedTime(&ms, tev[i + 2], tev[i + 3]));
    c->tm.rates_ms += ms;
  }
  c->pass_open = false;
  return 0;
}

static int pass_sources_one(c2r_ctx *c, int first, int stride) {
  if (check_ready(c, "c2r_pass_sources")) return 1;
  if (first < 1 || stride < 1) return fail(c, "c2r_pass_sources: first=%d stride=%d", first, stride);
  c->last_first = first;
  c->last_stride = stride;
  return pass_list(c, dealt_share(c, first, stride));
}

extern "C" int c2r_pass_sources_begin(c2r_ctx *c, int first, int stride, int nslab) {
  if (!c) return 1;
  if (!c->replicas.empty()) return fail(c, "c2r_pass_sources_begin: not available on a multi-device context");
  if (check_ready(c, "c2r_pass_sources_begin")) return 1;
  if (first < 1 || stride < 1 || nslab < 1) return fail(c, "c2r_pass_sources_begin: first=%d stride=%d nslab=%d", first, stride, nslab);
  return pass_list(c, dealt_share(c, first, stride), nslab);
}

extern "C" int c2r_pass_slab_count(c2r_ctx *c) { return c && c->pass_open ? c->pass_slabs : 0; }

extern "C" int c2r_pass_wait_slab(c2r_ctx *c, int slab, size_t *first_cell, size_t *ncells) {
  if (!c) return 1;
  if (!c->pass_open || slab < 0 || slab >= c->pass_slabs) return fail(c, "c2r_pass_wait_slab: slab %d of %d (pass %s)", slab, c->pass_slabs, c->pass_open ? "open" : "not open");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(c->ev_slab[slab]));
  const size_t plane = (size_t)c->g.n1 * c->g.n2;
  if (first_cell) *first_cell = plane * (size_t)c->slab_k[slab];
  if (ncells) *ncells = plane * (size_t)(c->slab_k[slab + 1] - c->slab_k[slab]);
  return 0;
}

extern "C" int c2r_pass_sources_end(c2r_ctx *c) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  return pass_finish(c);
}

extern "C" int c2r_do_source(c2r_ctx *c, int ns) {
  if (!c) return 1;
  if (!c->replicas.empty()) return fail(c, "c2r_do_source: not available on a multi-device context");
  if (check_ready(c, "c2r_do_source")) return 1;
  // (NumSrc < ns <= NumSrc + nplane: plane ns - NumSrc)
  if (ns < 1 || ns > c->nsrc + c->nplane) return fail(c, "c2r_do_source: source %d not in [1,%d]", ns, c->nsrc + c->nplane);
  if (c->ext_smax > 0 && ns <= c->nsrc && source_is_external(c, ns))
    return fail(c, "c2r_do_source: source %d stands outside the mesh (c2r_set_sources_external), which the per-point route is not built for "
                "(c2r_pass_sources sweeps it)", ns);
  return pass_list(c, std::vector<int>{ns});
}

// The global pass over a range of cells, queued behind `after_event` (an event of another stream, e.g. the
// one on which the caller's sum over ranks of these cells completes; may be null).  A range starting at
// cell 0 opens a pass (zeroes the non-converged count); c2r_global_pass_finish closes it.
// Heating global pass in tiers.  The number of sub-steps thermal() takes for a cell spans four orders of magnitude
// (cells at an ionisation front sub-cycle the energy equation hundreds to thousands of times, over hundreds of
// do_chemistry iterations, next to neighbours that need two), a wave lasts as long as its slowest lane, and a sub-step
// is a chain of dependent operations some 2 700 cycles long (the log10 of coolin, ten cooling-curve look-ups, six
// divisions) with two waves per SIMD to hide it: a plain launch leaves nine tenths of the lane-time idle.  So every
// launch gives its cells a ceiling of sub-steps; a cell that needs more stores nothing, is put on a list and is redone
// from scratch, densely packed with its likes, by the next launch under a ceiling four times higher: 16, 64, 256,
// 1 024, then none -- and none earlier once the cells that are left fit the device all at once (two waves per SIMD:
// 131 072 cells): such a launch lasts as long as its longest chain whatever the others do.  The ladder starts at the
// lowest rung under which at least half of the PREVIOUS pass's cells finished (a smoothly ionised box whose cells all
// need some tens of sub-steps would otherwise do 16 of them in vain for every cell).  Within a tier the cells
// then differ by a factor of four at most, and what the dropped cells did in vain is a third of their useful work
// at worst.  (Rungs at 4 096 and 16 384 were measured too: 1-2 ms slower at 256^3, where they only add their own
// chains, and 0.5-1 s slower on 512^3 with 10^4 sources, where two thirds of the cells beyond 1 024 lie beyond 4 096
// as well and do 4 096 sub-steps in vain.)  (Rounds 1 and 2 chose ONE first ceiling from
// the previous pass's histogram, twice its 90th percentile, and went on in steps of eight: measured on the 128 faint
// sources of a configs[3] rank with heating, C2R_CHEM_LOG, that first launch took 90-100 ms of a 125 ms pass under a
// ceiling of 512 while two thirds of its cells needed fewer than 64 sub-steps.)  The last tier is the longest chain
// of the mesh -- some 14 000 sub-steps, 16 ms, however few cells are left -- and nothing on the device shortens that.
// Results do not depend on any of this: a dropped cell stores nothing and is recomputed from the same inputs.
// C2R_CHEM_RESIDENT_CELLS (environment, read by c2r_create; diagnostic): another residency cut than 131 072 cells, 0 for
// none, so that small meshes walk the whole ladder.  It changes launches, never results.
constexpr int CHEM_FIRST_CEILING = 16, CHEM_CEILING_STEP = 4, CHEM_LAST_CEILING = 1024, CHEM_TIERS = 6;

static int launch_chemistry(c2r_ctx *c, hipStream_t st, double dt, size_t first, size_t count, const int *list, int budget,
                            int *deferred, int *ndeferred) {
  if (count == 0) return 0;
  const Grid g = c->g;
  const StepScalars sc = scalars(c);
  const bool lds = !c->isothermal && list != nullptr; // the repacked tiers of a heating pass
  const int bs = lds ? CHEM_BLOCK_LDS : C2R_CHEM_BLOCK;
  const int nblk = (int)((count + bs - 1) / bs);
  // a range of whole k-planes on a mesh whose sizes are multiples of 4: waves take cubes (see the kernel)
  const size_t plane = (size_t)g.n1 * g.n2;
  // ... while the pass before left more than 1/64 of the cells unconverged (or a step has just begun): once nearly
  // every cell is done after one iteration there is nothing to gain, and rows of 64 cells read their 17 grids in
  // longer runs.  Same box, ms per pass over the 8 iterations of a time step in ionised gas, rows | 4x4x4 | 8x4x2 cells:
  // 2.80 2.53 2.28 1.80 1.54 1.44 1.17 1.02 | 2.04 1.92 1.84 1.62 1.53 1.37 1.19 1.15 | 2.04 1.87 1.80 1.55 1.45 1.29 1.08 1.06.
  // C2R_CHEM_CUBES=0 / 1 / 2 (environment): rows always / 4 x 4 x 4 always / 8 x 4 x 2 always; default: 8 x 4 x 2 by the rule.
  static const int cubes_env = getenv("C2R_CHEM_CUBES") ? atoi(getenv("C2R_CHEM_CUBES")) : -1;
  const bool busy = c->last_conv < 0 || c->last_conv * 64 > (long long)g.ncell;
  const int cubes_want = cubes_env >= 0 ? cubes_env : (busy ? 2 : 0);
  const int cubes = cubes_want && !list && g.n1 % 8 == 0 && g.n2 % 4 == 0 && first % plane == 0 && count % (4 * plane) == 0 ? cubes_want : 0;
  if (c->isothermal)
    hipLaunchKernelGGL(k_chemistry<false>, dim3(nblk), dim3(bs), 0, st, g, sc, dt, c->d_ndens, c->d_xh,
                       c->d_xhe, c->d_xh_av, c->d_xhe_av, c->d_xh_int, c->d_xhe_int, c->d_temp, c->d_rates, c->d_chemspread,
                       c->d_rc_last, c->clumping_on_grid ? c->d_clump : nullptr, first, first + count, list, 0,
                       (int *)nullptr, (int *)nullptr, c->d_stateT, cubes);
  else if (lds)
    hipLaunchKernelGGL((k_chemistry<true, true>), dim3(nblk), dim3(bs), 0, st, g, sc, dt, c->d_ndens, c->d_xh,
                       c->d_xhe, c->d_xh_av, c->d_xhe_av, c->d_xh_int, c->d_xhe_int, c->d_temp, c->d_rates, c->d_chemspread,
                       c->d_rc_last, c->clumping_on_grid ? c->d_clump : nullptr, first, first + count, list, budget, deferred,
                       ndeferred, c->d_stateT, 0);
  else
    hipLaunchKernelGGL(k_chemistry<true>, dim3(nblk), dim3(bs), 0, st, g, sc, dt, c->d_ndens, c->d_xh,
                       c->d_xhe, c->d_xh_av, c->d_xhe_av, c->d_xh_int, c->d_xhe_int, c->d_temp, c->d_rates, c->d_chemspread,
                       c->d_rc_last, c->clumping_on_grid ? c->d_clump : nullptr, first, first + count, list, budget, deferred,
                       ndeferred, c->d_stateT, cubes);
  HIPCHK(c, hipGetLastError());
  c->tm.chem_launches++;
  return 0;
}

// the spread counters of the launches so far, folded into d_conv and (heating) the histogram behind d_chemctl + 2
static int fold_chemistry_counters(c2r_ctx *c, hipStream_t st) {
  hipLaunchKernelGGL(k_chem_ctl_reduce, dim3(1), dim3(64), 0, st, c->d_chemspread, c->d_conv,
                     c->isothermal ? (int *)nullptr : c->d_chemctl + 2);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// Everything a global pass needs exists before it starts: the spread counters since c2r_create, the heating lists since
// the c2r_set_step that declared the step non-isothermal (round 3 allocated both here, inside the first pass).
static int ensure_chemistry_buffers(c2r_ctx *c) {
  if (!c->d_chemspread) return fail(c, "the chemistry counters are missing (c2r_create did not finish?)");
  if (!c->isothermal && !(c->d_defer[0] && c->d_defer[1] && c->d_chemctl))
    return fail(c, "a non-isothermal pass before c2r_set_step declared the step non-isothermal (or its lists could not be allocated)");
  return 0;
}

// evolve0D_global(dt,pos,conv_flag) (files_for_3D/evolve_point.F90:325-440) for ONE cell, as the reference's
// global_pass calls it (evolve.F90:477-484): applies the collected rates to the cell at 1-based mesh position
// pos and adds 1 to conv_flag if the cell has not converged.  A whole pass is c2r_global_pass; this entry point
// exists for hosts written against the per-cell interface (one launch and one synchronisation per call).
extern "C" int c2r_evolve0d_global(c2r_ctx *c, double dt, const int pos[3], int *conv_flag) {
  if (!c || !pos) return 1;
  if (check_ready(c, "c2r_evolve0d_global")) return 1;
  const Grid g = c->g;
  if (pos[0] < 1 || pos[0] > g.n1 || pos[1] < 1 || pos[1] > g.n2 || pos[2] < 1 || pos[2] > g.n3)
    return fail(c, "c2r_evolve0d_global: position (%d,%d,%d) outside the mesh", pos[0], pos[1], pos[2]);
  HIPCHK(c, hipSetDevice(c->device));
  if (flush_rates_zero(c)) return 1;
  if (ensure_chemistry_buffers(c)) return 1;
  const size_t q = (size_t)(pos[0] - 1) + (size_t)g.n1 * ((size_t)(pos[1] - 1) + (size_t)g.n2 * (size_t)(pos[2] - 1));
  HIPCHK(c, hipMemsetAsync(c->d_conv, 0, sizeof(int), c->stream));
  c->transposed_valid = false; // the launch keeps the mesh-ordered products of its cell up to date, not their (j,i,k) copy
  if (launch_chemistry(c, c->stream, dt, q, 1, nullptr, 0, c->d_defer[0], c->d_chemctl)) return 1;
  if (fold_chemistry_counters(c, c->stream)) return 1;
  HIPCHK(c, hipMemcpyAsync(c->h_conv, c->d_conv, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (conv_flag) *conv_flag += *c->h_conv;
  for (c2r_ctx *r : c->replicas) // the other devices of a multi-device context keep the same state
    if (c2r_evolve0d_global(r, dt, pos, nullptr)) { c->err = r->err; return 1; }
  return 0;
}

// evolve0D(dt,rtpos,ns,niter) for one cell (see the header): one small launch per call, in the caller's order
extern "C" int c2r_evolve0d(c2r_ctx *c, const int rtpos[3], int ns, int niter, int on_surface, double *loss) {
  if (!c || !rtpos) return 1;
  if (!c->replicas.empty()) return fail(c, "c2r_evolve0d: not available on a multi-device context");
  if (check_ready(c, "c2r_evolve0d")) return 1;
  if (ns < 1 || ns > c->nsrc) return fail(c, "c2r_evolve0d: source %d not in [1,%d]", ns, c->nsrc);
  if (c->pass_open) return fail(c, "c2r_evolve0d: a pass opened by c2r_pass_sources_begin is still open");
  if (c->ext_smax > 0 && source_is_external(c, ns))
    return fail(c, "c2r_evolve0d: source %d stands outside the mesh (c2r_set_sources_external), which the per-point route is not built for", ns);
  HIPCHK(c, hipSetDevice(c->device));
  const Grid g = c->g;
  const int *sp = &c->srcpos[3 * (size_t)(ns - 1)];
  const int di = rtpos[0] - sp[0], dj = rtpos[1] - sp[1], dk = rtpos[2] - sp[2];
  const Reach R = source_reach(c, ns);
  if (di < R.l[0] || di > R.r[0] || dj < R.l[1] || dj > R.r[1] || dk < R.l[2] || dk > R.r[2])
    return fail(c, "c2r_evolve0d: cell (%d,%d,%d) is beyond the reach of source %d at (%d,%d,%d)", rtpos[0], rtpos[1], rtpos[2], ns,
                sp[0], sp[1], sp[2]);
  if (flush_rates_zero(c)) return 1;
  // (open boundaries: the cells within a source's reach, in its own cut shell order, are never more than the mesh has)
  const size_t w = (size_t)(2 * g.smax + 1), cz = c->periodic ? w * w * w : g.ncell;
  if (!c->d_point_cols) {
    // a block that holds the whole mesh, zeroed once: only ever finite columns afterwards (see the arena)
    HIPCHK(c, hipMalloc(&c->d_point_cols, sizeof(double) * 6 * cz));
    HIPCHK(c, zero_device(c->d_point_cols, sizeof(double) * 6 * cz, c->stream));
    HIPCHK(c, hipMalloc(&c->d_point_loss, sizeof(double)));
    HIPCHK(c, hipHostMalloc(&c->h_point_loss, sizeof(double)));
  }
  c->point_ns = ns;
  c->point_niter = niter;
  const StepScalars sc = scalars(c);
  bool multi = false;
  const SedSet ss = sedset(c, &multi);
  SweepArgs SA;
  SA.g = g; SA.sc = sc;
  for (int d = 0; d < 3; d++) { SA.box.lo[d] = R.l[d]; SA.box.hi[d] = R.r[d]; }
  SA.ndens = c->d_ndens; SA.xh_av = c->d_xh_av; SA.xhe_av = c->d_xhe_av;
  SA.packed = SA.packedT = nullptr;
  SA.lls_grid = c->lls_on_grid ? c->d_lls : nullptr;
  SrcDev S{};
  S.i0 = sp[0]; S.j0 = sp[1]; S.k0 = sp[2];
  S.nflux = c->normflux[(size_t)ns - 1];
  for (int k = 0; k < 2; k++) S.nflux_sed[k] = c->normflux_sed[k].empty() ? 0.0 : c->normflux_sed[k][(size_t)ns - 1];
  S.cols = c->d_point_cols;
  S.cz = cz;
  S.loss_lo = -1;
  for (int d = 0; d < 3; d++) { S.rl[d] = R.l[d]; S.rr[d] = R.r[d]; }
  source_wrap(c, S.wn);
  source_cut(c, ns, S);
  double *dl = on_surface ? c->d_point_loss : nullptr;
  if (!c->isothermal) c->phiheat_dirty = true;
  with_flag(!c->isothermal, [&](auto heat) { with_flag(multi, [&](auto three) { with_flag(!c->periodic, [&](auto open) {
    const auto kernel = k_evolve0d<decltype(heat)::value, decltype(three)::value, decltype(open)::value>;
    hipLaunchKernelGGL(kernel, dim3(1), dim3(64), 0, c->stream, SA, S, di, dj, dk, c->d_bands, ss, c->d_rates, dl);
  }); }); });
  HIPCHK(c, hipGetLastError());
  if (on_surface) {
    HIPCHK(c, hipMemcpyAsync(c->h_point_loss, c->d_point_loss, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (loss) *loss = *c->h_point_loss;
  }
  return 0;
}

extern "C" int c2r_global_pass_cells(c2r_ctx *c, double dt, size_t first_cell, size_t ncells, void *after_event) {
  if (!c) return 1;
  if (check_ready(c, "c2r_global_pass_cells")) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (flush_rates_zero(c)) return 1;
  const Grid g = c->g;
  if (first_cell > g.ncell || ncells > g.ncell - first_cell) return fail(c, "c2r_global_pass_cells: range outside the mesh");
  const bool heat = !c->isothermal;
  if (ensure_chemistry_buffers(c)) return 1;
  if (first_cell == 0) {
    HIPCHK(c, hipMemsetAsync(c->d_conv, 0, sizeof(int), c->stream));
    if (heat) HIPCHK(c, hipMemsetAsync(c->d_chemctl, 0, sizeof(int) * (4 + CHEM_HIST), c->stream));
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
    // the second stream takes every other piece: it must see the zeroed counters (and everything before)
    HIPCHK(c, hipEventRecord(c->ev_sweep_done[0], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_sweep_done[0], 0));
    c->tm.chem_launches = 0;
    c->chem_pieces = 0;
    c->packed_valid = c->transposed_valid = false;
    c->chem_cells = 0;
    c->chem_dt = dt;
  }
  c->chem_cells += ncells;
  // Pieces alternate between the two streams: every launch ends in a long thin tail; on alternating streams
  // the next piece fills the chip while the previous one drains.
  hipStream_t st = (c->chem_pieces++ & 1) ? c->stream2 : c->stream;
  if (after_event) HIPCHK(c, hipStreamWaitEvent(st, static_cast<hipEvent_t>(after_event), 0));
  return launch_chemistry(c, st, dt, first_cell, ncells, nullptr, heat ? c->chem_first : 0, c->d_defer[0], c->d_chemctl);
}

extern "C" int c2r_global_pass_finish(c2r_ctx *c, int *conv_flag) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  // join the second stream
  HIPCHK(c, hipEventRecord(c->ev_rates_done[0], c->stream2));
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_rates_done[0], 0));
  if (!c->isothermal) {
    // later tiers: the cells dropped by the previous launch(es), densely packed
    // C2R_CHEM_LOG=1 (diagnostic): where the time of a heating pass goes, tier by tier, on stderr
    static const bool chem_log = getenv("C2R_CHEM_LOG") && atoi(getenv("C2R_CHEM_LOG")) > 0;
    auto t_tier = std::chrono::steady_clock::now();
    int cur = 0;
    long long ceiling = c->chem_first;
    for (int t = 1; t < CHEM_TIERS; t++) {
      int n = 0;
      HIPCHK(c, hipMemcpyAsync(&n, c->d_chemctl + cur, sizeof(int), hipMemcpyDeviceToHost, c->stream));
      if (sync_stream(c, c->stream, "a tier of the global pass")) return 1;
      if (chem_log) {
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "c2ray_hip: heating pass, tier %d (ceiling %lld sub-steps) done after %.1f ms: %d cells deferred\n", t - 1,
                ceiling, std::chrono::duration<double, std::milli>(now - t_tier).count(), n);
        t_tier = now;
      }
      if (n <= 0) break;
      const int nxt = cur ^ 1;
      ceiling *= CHEM_CEILING_STEP;
      HIPCHK(c, hipMemsetAsync(c->d_chemctl + nxt, 0, sizeof(int), c->stream));
      const bool last = t == CHEM_TIERS - 1 || n <= c->chem_resident || ceiling > CHEM_LAST_CEILING;
      if (launch_chemistry(c, c->stream, c->chem_dt, 0, (size_t)n, c->d_defer[cur], last ? 0 : (int)ceiling, c->d_defer[nxt],
                           c->d_chemctl + nxt))
        return 1;
      cur = nxt;
      if (last) break;
    }
    if (fold_chemistry_counters(c, c->stream)) return 1;
    // where the next pass starts its ladder: the lowest rung under which at least half of this pass's cells finished
    // (a pass whose cells all need some tens of sub-steps would otherwise do 16 of them in vain for every cell)
    int hist[CHEM_HIST + 2];
    HIPCHK(c, hipMemcpyAsync(hist, c->d_chemctl + 2, sizeof hist, hipMemcpyDeviceToHost, c->stream));
    if (sync_stream(c, c->stream, "the global pass")) return 1;
    {
      long long total = 0, acc = 0;
      for (int b = 0; b < CHEM_HIST; b++) total += hist[b];
      int first = CHEM_FIRST_CEILING, b = 0;
      for (long long rung = CHEM_FIRST_CEILING; rung <= CHEM_LAST_CEILING; rung *= CHEM_CEILING_STEP) {
        for (; b < CHEM_HIST && (1LL << b) <= rung; b++) acc += hist[b]; // bucket b holds [2^(b-1), 2^b)
        first = (int)rung;
        if (2 * acc >= total) break;
      }
      c->chem_first = total > 0 ? first : CHEM_FIRST_CEILING;
    }
    if (chem_log) {
      fprintf(stderr, "c2ray_hip: heating pass, last tier done after %.1f ms; longest chain: %d thermal sub-steps, %d do_chemistry iterations; cells per power of two of sub-steps:",
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_tier).count(), hist[CHEM_HIST], hist[CHEM_HIST + 1]);
      for (int b = 0; b < CHEM_HIST; b++) fprintf(stderr, " %d", hist[b]);
      fprintf(stderr, "\n");
    }
  }
  if (c->isothermal && fold_chemistry_counters(c, c->stream)) return 1;
  if (c->timing) HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  // every cell's products for the next column sweep are up to date if the pieces of this pass covered the mesh
  // (pieces that overlap or leave gaps, a caller's business, leave the flag down: the next pass then packs anew)
  const bool packed_now = c->chem_cells == c->g.ncell;
  if (packed_now) {
    // ... and their (j,i,k)-ordered copy is made right away, on the third stream, while the host reads this pass's
    // results: at the start of the next pass it would share the device with the sweep's innermost shells (measured: 9-14
    // us each beside it, 5-7 us alone)
    HIPCHK(c, hipEventRecord(c->ev_chem_done, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream3, c->ev_chem_done, 0));
    hipLaunchKernelGGL(k_transpose_packed, dim3((c->g.n1 + 31) / 32, (c->g.n2 + 31) / 32, 3 * c->g.n3), dim3(BLOCK), 0, c->stream3, c->g,
                       c->d_stateT, c->d_stateT + 3 * c->g.ncell);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_transposed, c->stream3));
  }
  if (c->want_iter_stats) {
    // c2r_iteration: the grid reductions the host loop wants after this pass, behind it in the same queue
    double *partial = c->d_iter, *partial_min = c->d_iter + (size_t)STAT_BLOCKS * ITER_NV, *res = partial_min + (size_t)STAT_BLOCKS * 2;
    const double *rc_dev = c->isothermal ? nullptr : c->d_rc_last;
    hipLaunchKernelGGL(k_iter_stats, dim3(STAT_BLOCKS), dim3(BLOCK), 0, c->stream, c->g.ncell, c->sc.rc, rc_dev, c->sc.clumping,
                       c->clumping_on_grid ? c->d_clump : nullptr, c->d_ndens, c->d_xh_int, c->d_xhe_int, c->d_xh_av, c->d_xhe_av,
                       partial, partial_min);
    hipLaunchKernelGGL(k_iter_stats_finish, dim3(1), dim3(BLOCK), 0, c->stream, partial, partial_min, STAT_BLOCKS, c->sc.rc, rc_dev, res);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_iter, res, sizeof(double) * (ITER_NV + 2 + 12), hipMemcpyDeviceToHost, c->stream));
    c->want_iter_stats = false;
  }
  HIPCHK(c, hipMemcpyAsync(c->h_conv, c->d_conv, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (sync_stream(c, c->stream, "the global pass")) return 1;
  if (c->timing) {
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[3], c->ev[4]));
    c->tm.chem_ms = ms;
  }
  if (conv_flag) *conv_flag = *c->h_conv;
  c->last_conv = *c->h_conv;
  c->packed_valid = c->transposed_valid = packed_now;
  return 0;
}

static int global_pass_one(c2r_ctx *c, double dt, int *conv_flag) {
  if (c2r_global_pass_cells(c, dt, 0, c->g.ncell, nullptr)) return 1;
  return c2r_global_pass_finish(c, conv_flag);
}

extern "C" int c2r_download_rates(c2r_ctx *c, double *phih, double *phihe, double *phiheat, double *photon_loss47,
                                  int *sum_nbox) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (flush_rates_zero(c)) return 1;
  const size_t nc = c->g.ncell;
  if (phih) HIPCHK(c, hipMemcpyAsync(phih, c->d_rates, sizeof(double) * nc, hipMemcpyDeviceToHost, c->stream));
  if (phihe) HIPCHK(c, hipMemcpyAsync(phihe, c->d_rates + nc, sizeof(double) * 2 * nc, hipMemcpyDeviceToHost, c->stream));
  if (phiheat) HIPCHK(c, hipMemcpyAsync(phiheat, c->d_rates + 3 * nc, sizeof(double) * nc, hipMemcpyDeviceToHost, c->stream));
  double tail[C2R_NFREQ + 1];
  HIPCHK(c, hipMemcpyAsync(tail, c->d_rates + 4 * nc, sizeof tail, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (photon_loss47) std::memcpy(photon_loss47, tail, sizeof(double) * C2R_NFREQ);
  if (sum_nbox) *sum_nbox = (int)(tail[C2R_NFREQ] + 0.5);
  return 0;
}

// the same for hosts that cannot pass a null pointer for an array (Fortran): bit 0 phih, bit 1 phihe, bit 2 phiheat
extern "C" int c2r_download_rates_sel(c2r_ctx *c, int which, double *phih, double *phihe, double *phiheat, double *photon_loss47,
                                      int *sum_nbox) {
  return c2r_download_rates(c, (which & 1) ? phih : nullptr, (which & 2) ? phihe : nullptr, (which & 4) ? phiheat : nullptr,
                            photon_loss47, sum_nbox);
}

extern "C" int c2r_get_loss(c2r_ctx *c, double *photon_loss47, int *sum_nbox) {
  if (!c) return 1;
  if (photon_loss47) std::memcpy(photon_loss47, c->photon_loss, sizeof c->photon_loss);
  if (sum_nbox) *sum_nbox = c->sum_nbox;
  return 0;
}

extern "C" int c2r_download_iter_state(c2r_ctx *c, double *xh_av, double *xhe_av, double *xh_intermed,
                                       double *xhe_intermed) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nc = c->g.ncell;
  if (xh_av) HIPCHK(c, hipMemcpyAsync(xh_av, c->d_xh_av, sizeof(double) * 2 * nc, hipMemcpyDeviceToHost, c->stream));
  if (xhe_av) HIPCHK(c, hipMemcpyAsync(xhe_av, c->d_xhe_av, sizeof(double) * 3 * nc, hipMemcpyDeviceToHost, c->stream));
  if (xh_intermed)
    HIPCHK(c, hipMemcpyAsync(xh_intermed, c->d_xh_int, sizeof(double) * 2 * nc, hipMemcpyDeviceToHost, c->stream));
  if (xhe_intermed)
    HIPCHK(c, hipMemcpyAsync(xhe_intermed, c->d_xhe_int, sizeof(double) * 3 * nc, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

static int upload_rates_one(c2r_ctx *c, const double *phih, const double *phihe, const double *phiheat) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (flush_rates_zero(c)) return 1;
  if (phiheat) c->phiheat_dirty = true;
  const size_t nc = c->g.ncell;
  if (phih) HIPCHK(c, hipMemcpyAsync(c->d_rates, phih, sizeof(double) * nc, hipMemcpyHostToDevice, c->stream));
  if (phihe) HIPCHK(c, hipMemcpyAsync(c->d_rates + nc, phihe, sizeof(double) * 2 * nc, hipMemcpyHostToDevice, c->stream));
  if (phiheat) HIPCHK(c, hipMemcpyAsync(c->d_rates + 3 * nc, phiheat, sizeof(double) * nc, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

static int upload_iter_state_one(c2r_ctx *c, const double *xh_av, const double *xhe_av, const double *xh_intermed,
                                     const double *xhe_intermed) {
  if (!c) return 1;
  c->packed_valid = c->transposed_valid = false;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nc = c->g.ncell;
  if (xh_av) HIPCHK(c, hipMemcpyAsync(c->d_xh_av, xh_av, sizeof(double) * 2 * nc, hipMemcpyHostToDevice, c->stream));
  if (xhe_av) HIPCHK(c, hipMemcpyAsync(c->d_xhe_av, xhe_av, sizeof(double) * 3 * nc, hipMemcpyHostToDevice, c->stream));
  if (xh_intermed)
    HIPCHK(c, hipMemcpyAsync(c->d_xh_int, xh_intermed, sizeof(double) * 2 * nc, hipMemcpyHostToDevice, c->stream));
  if (xhe_intermed)
    HIPCHK(c, hipMemcpyAsync(c->d_xhe_int, xhe_intermed, sizeof(double) * 3 * nc, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int c2r_download_columns(c2r_ctx *c, double *coldensh_out, double *coldenshe_out) {
  if (!c) return 1;
  if (!c->last_cols || c->last_src < 1) return fail(c, "c2r_download_columns: no source has been swept yet");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nc = c->g.ncell;
  if (!c->d_colgrid) HIPCHK(c, hipMalloc(&c->d_colgrid, sizeof(double) * 3 * nc));
  const int *p = &c->srcpos[3 * (size_t)(c->last_src - 1)];
  const int nblk = (int)((nc + BLOCK - 1) / BLOCK);
  SrcDev S{};
  S.i0 = p[0]; S.j0 = p[1]; S.k0 = p[2];
  for (int d = 0; d < 3; d++) { S.lo[d] = c->last_lo[d]; S.hi[d] = c->last_hi[d]; }
  S.cz = c->last_cz;
  const Reach R = source_reach(c, c->last_src);
  for (int d = 0; d < 3; d++) { S.rl[d] = R.l[d]; S.rr[d] = R.r[d]; }
  source_wrap(c, S.wn);
  if (c->periodic) hipLaunchKernelGGL(k_col_to_grid<false>, dim3(nblk), dim3(BLOCK), 0, c->stream, c->g, S, c->last_cols, c->d_colgrid);
  else hipLaunchKernelGGL(k_col_to_grid<true>, dim3(nblk), dim3(BLOCK), 0, c->stream, c->g, S, c->last_cols, c->d_colgrid);
  HIPCHK(c, hipGetLastError());
  if (coldensh_out) HIPCHK(c, hipMemcpyAsync(coldensh_out, c->d_colgrid, sizeof(double) * nc, hipMemcpyDeviceToHost, c->stream));
  if (coldenshe_out)
    HIPCHK(c, hipMemcpyAsync(coldenshe_out, c->d_colgrid + nc, sizeof(double) * 2 * nc, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int c2r_state_sums(c2r_ctx *c, int which, double out5[5]) {
  if (!c || !out5) return 1;
  if (!c->have_state || !c->have_step) return fail(c, "c2r_state_sums: state / step not set");
  if (which < 0 || which > 2) return fail(c, "c2r_state_sums: which = %d not in {0,1,2}", which);
  HIPCHK(c, hipSetDevice(c->device));
  const double *xh = which == 0 ? c->d_xh : (which == 1 ? c->d_xh_int : c->d_xh_av);
  const double *xhe = which == 0 ? c->d_xhe : (which == 1 ? c->d_xhe_int : c->d_xhe_av);
  hipLaunchKernelGGL(k_state_sums, dim3(STAT_BLOCKS), dim3(BLOCK), 0, c->stream, c->g.ncell, c->d_ndens, xh, xhe, c->d_stat);
  hipLaunchKernelGGL(k_stat_finish<5>, dim3(1), dim3(BLOCK), 0, c->stream, c->d_stat, STAT_BLOCKS, c->d_stat + STAT_BLOCKS * 5);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->h_stat, c->d_stat + STAT_BLOCKS * 5, sizeof(double) * 5, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // h0 = sum*vol*(1-abu_he) ... (photonstatistics.f90:139-143)
  out5[0] = c->h_stat[0] * c->sc.vol * (1.0 - abu_he);
  out5[1] = c->h_stat[1] * c->sc.vol * (1.0 - abu_he);
  out5[2] = c->h_stat[2] * c->sc.vol * abu_he;
  out5[3] = c->h_stat[3] * c->sc.vol * abu_he;
  out5[4] = c->h_stat[4] * c->sc.vol * abu_he;
  return 0;
}

extern "C" int c2r_fraction_means(c2r_ctx *c, int which, double out5[5]) {
  if (!c || !out5) return 1;
  if (!c->have_state) return fail(c, "c2r_fraction_means: state not set");
  if (which < 0 || which > 2) return fail(c, "c2r_fraction_means: which = %d not in {0,1,2}", which);
  HIPCHK(c, hipSetDevice(c->device));
  const double *xh = which == 0 ? c->d_xh : (which == 1 ? c->d_xh_int : c->d_xh_av);
  const double *xhe = which == 0 ? c->d_xhe : (which == 1 ? c->d_xhe_int : c->d_xhe_av);
  hipLaunchKernelGGL(k_state_sums, dim3(STAT_BLOCKS), dim3(BLOCK), 0, c->stream, c->g.ncell, (const double *)nullptr, xh, xhe,
                     c->d_stat);
  hipLaunchKernelGGL(k_stat_finish<5>, dim3(1), dim3(BLOCK), 0, c->stream, c->d_stat, STAT_BLOCKS, c->d_stat + STAT_BLOCKS * 5);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->h_stat, c->d_stat + STAT_BLOCKS * 5, sizeof(double) * 5, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int n = 0; n < 5; n++) out5[n] = c->h_stat[n] / (double)c->g.ncell;
  return 0;
}

extern "C" int c2r_fraction_minima(c2r_ctx *c, int which, double out2[2]) {
  if (!c || !out2) return 1;
  if (!c->have_state) return fail(c, "c2r_fraction_minima: state not set");
  if (which < 0 || which > 2) return fail(c, "c2r_fraction_minima: which = %d not in {0,1,2}", which);
  HIPCHK(c, hipSetDevice(c->device));
  const double *xh = which == 0 ? c->d_xh : (which == 1 ? c->d_xh_int : c->d_xh_av);
  const double *xhe = which == 0 ? c->d_xhe : (which == 1 ? c->d_xhe_int : c->d_xhe_av);
  hipLaunchKernelGGL(k_state_min, dim3(STAT_BLOCKS), dim3(BLOCK), 0, c->stream, c->g.ncell, xh, xhe, c->d_stat);
  hipLaunchKernelGGL(k_min_finish, dim3(1), dim3(BLOCK), 0, c->stream, c->d_stat, STAT_BLOCKS, c->d_stat + STAT_BLOCKS * 5);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->h_stat, c->d_stat + STAT_BLOCKS * 5, sizeof(double) * 2, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  out2[0] = c->h_stat[0];
  out2[1] = c->h_stat[1];
  return 0;
}

// The numerical and algorithmic parameters compiled into the device code, in the order of the header's list.
extern "C" int c2r_get_constants(double *out, int capacity) {
  const double v[] = {(double)SUBBOXSIZE, (double)MAX_SUBBOX, abu_he, abu_c, epsilon, convergence_fraction,
                      minimum_fractional_change, minimum_fraction_of_atoms, relative_denergy, minitemp,
                      (double)NTAU, minlogtau, 4.0 /* maxlogtau */, (double)NFREQ, (double)NHEAT};
  const int n = (int)(sizeof v / sizeof v[0]);
  for (int i = 0; i < n && i < capacity; i++) out[i] = v[i];
  return n;
}

extern "C" int c2r_total_rates(c2r_ctx *c, double dt, const double reccoef[12], double out3[3]) {
  if (!c || !reccoef || !out3) return 1;
  if (!c->have_state || !c->have_step) return fail(c, "c2r_total_rates: state / step not set");
  HIPCHK(c, hipSetDevice(c->device));
  RecCoef rc;
  std::memcpy(&rc, reccoef, sizeof rc);
  hipLaunchKernelGGL(k_total_rates, dim3(STAT_BLOCKS), dim3(BLOCK), 0, c->stream, c->g.ncell, rc, c->sc.clumping,
                     c->clumping_on_grid ? c->d_clump : nullptr, c->d_ndens, c->d_xh_av, c->d_xhe_av, c->d_stat);
  hipLaunchKernelGGL(k_stat_finish<3>, dim3(1), dim3(BLOCK), 0, c->stream, c->d_stat, STAT_BLOCKS, c->d_stat + STAT_BLOCKS * 5);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->h_stat, c->d_stat + STAT_BLOCKS * 5, sizeof(double) * 3, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int n = 0; n < 3; n++) out3[n] = c->h_stat[n] * c->sc.vol * dt; // photonstatistics.f90:199-201
  return 0;
}

extern "C" int c2r_get_reccoef(c2r_ctx *c, double out12[12]) {
  if (!c || !out12) return 1;
  if (c->isothermal) {
    std::memcpy(out12, &c->sc.rc, sizeof(double) * 12);
    return 0;
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(out12, c->d_rc_last, sizeof(double) * 12, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int c2r_arena_stats(const c2r_ctx *c, long long out[6]) {
  if (!c || !out) return 1;
  for (int i = 0; i < 5; i++) out[i] = c->arena_stats[i];
  out[5] = (long long)c->arena_total;
  return 0;
}
extern "C" int c2r_get_source_trace(c2r_ctx *c, int ns, c2r_source_trace *out) {
  if (!c || !out) return 1;
  if (ns < 1 || ns > c->nsrc) return fail(c, "c2r_get_source_trace: source %d not in [1,%d]", ns, c->nsrc);
  // the context itself or, of a multi-device context, the device that swept the source last
  const c2r_ctx *from = nullptr;
  long long stamp = 0;
  auto look = [&](const c2r_ctx *r) {
    if (r->trace_stamp.size() >= (size_t)ns && r->trace_stamp[(size_t)ns - 1] > stamp) {
      stamp = r->trace_stamp[(size_t)ns - 1];
      from = r;
    }
  };
  look(c);
  for (const c2r_ctx *r : c->replicas) look(r);
  if (from) {
    *out = from->trace[(size_t)ns - 1];
    return 0;
  }
  // not swept yet: its reach, and nothing else
  *out = c2r_source_trace{};
  const Reach R = source_reach(c, ns);
  for (int d = 0; d < 3; d++) { out->reach_l[d] = R.l[d]; out->reach_r[d] = R.r[d]; }
  return 0;
}
extern "C" size_t c2r_rates_count(const c2r_ctx *c) { return c ? c->rates_count : 0; }
extern "C" void *c2r_rates_device_ptr(c2r_ctx *c) {
  if (!c) return nullptr;
  (void)flush_rates_zero(c); // whoever asks for the address may read it
  return (void *)c->d_rates;
}
extern "C" int c2r_set_rates_buffer(c2r_ctx *c, void *device_ptr, size_t count) {
  if (!c) return 1;
  c->phiheat_dirty = true; // contents of the other buffer unknown
  if (!device_ptr) { c->d_rates = c->d_rates_own; return 0; }
  if (count < c->rates_count) return fail(c, "c2r_set_rates_buffer: %zu doubles given, %zu needed", count, c->rates_count);
  c->d_rates = (double *)device_ptr;
  return 0;
}
static int synchronize_one(c2r_ctx *c) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (flush_rates_zero(c)) return 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
static int enable_timing_one(c2r_ctx *c, int on) {
  if (!c) return 1;
  c->timing = on != 0;
  return 0;
}
extern "C" int c2r_get_timing(c2r_ctx *c, c2r_timing *out) {
  if (!c || !out) return 1;
  *out = c->tm;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// state-setting entry points: the same call on every device of a multi-device context
extern "C" int c2r_set_tables(c2r_ctx *c, const double *photo_thick, const double *photo_thin, const double *heat_thick, const double *heat_thin, const double *sigma_HI, const double *sigma_HeI, const double *sigma_HeII, const double *const fvec[12], int bb_upper) {
  if (int e_ = set_tables_one(c, photo_thick, photo_thin, heat_thick, heat_thin, sigma_HI, sigma_HeI, sigma_HeII, fvec, bb_upper)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_tables_one(r, photo_thick, photo_thin, heat_thick, heat_thin, sigma_HI, sigma_HeI, sigma_HeII, fvec, bb_upper); });
}

extern "C" int c2r_set_cooling(c2r_ctx *c, const double *cool, double mintemp, double dtemp) {
  if (int e_ = set_cooling_one(c, cool, mintemp, dtemp)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_cooling_one(r, cool, mintemp, dtemp); });
}

extern "C" int c2r_set_step(c2r_ctx *c, const double *ndens, const double dr[3], double vol, float clumping, double zred, double H0, double Omega0, int isothermal, double temper_val, const double reccoef[12]) {
  if (int e_ = set_step_one(c, ndens, dr, vol, clumping, zred, H0, Omega0, isothermal, temper_val, reccoef)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_step_one(r, ndens, dr, vol, clumping, zred, H0, Omega0, isothermal, temper_val, reccoef); });
}

extern "C" int c2r_set_step_scalars(c2r_ctx *c, const double dr[3], double vol, float clumping, double zred, double H0, double Omega0, int isothermal, double temper_val, const double reccoef[12]) {
  if (set_step_one(c, nullptr, dr, vol, clumping, zred, H0, Omega0, isothermal, temper_val, reccoef)) return 1;
  return for_replicas(c, [&](c2r_ctx *r) { return set_step_one(r, nullptr, dr, vol, clumping, zred, H0, Omega0, isothermal, temper_val, reccoef); });
}
static int scale_ndens_one(c2r_ctx *c, double divisor) {
  if (!c->have_step) return fail(c, "c2r_scale_ndens: no density on the device yet");
  if (!(divisor > 0.0) || !std::isfinite(divisor)) return fail(c, "c2r_scale_ndens: divisor %g", divisor);
  HIPCHK(c, hipSetDevice(c->device));
  const int nblk = (int)std::min<size_t>(65535, (c->g.ncell + BLOCK - 1) / BLOCK);
  hipLaunchKernelGGL(k_divide_by, dim3(nblk), dim3(BLOCK), 0, c->stream, c->d_ndens, c->g.ncell, divisor);
  HIPCHK(c, hipGetLastError());
  c->packed_valid = c->transposed_valid = false; // the products neufrac * ndens of the sweep are stale
  return 0;
}
extern "C" int c2r_scale_ndens(c2r_ctx *c, double divisor) {
  if (!c) return 1;
  if (scale_ndens_one(c, divisor)) return 1;
  return for_replicas(c, [&](c2r_ctx *r) { return scale_ndens_one(r, divisor); });
}
extern "C" int c2r_set_sources(c2r_ctx *c, int nsrc, const int *srcpos, const double *normflux, double s_star) {
  if (int e_ = set_sources_one(c, nsrc, srcpos, normflux, s_star)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_sources_one(r, nsrc, srcpos, normflux, s_star); });
}
extern "C" int c2r_set_sources_external(c2r_ctx *c, int nsrc, const int *srcpos, const double *normflux, double s_star) {
  if (int e_ = set_sources_one(c, nsrc, srcpos, normflux, s_star, true)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_sources_one(r, nsrc, srcpos, normflux, s_star, true); });
}

#include "c2ray_handover.inc" // exit strips and entry columns of point sources: the c2r_*source_face* entry points

// ---------------------------------------------------------------------------------------------
// escape maps
static int enable_face_loss_one(c2r_ctx *c, int on) {
  if (!c) return 1;
  if (c->pass_open) return fail(c, "c2r_enable_face_loss: a pass opened by c2r_pass_sources_begin is still open (close it with c2r_pass_sources_end first)");
  HIPCHK(c, hipSetDevice(c->device));
  if (!on) {
    if (c->d_face_maps) HIPCHK(c, hipStreamSynchronize(c->stream)); // nothing queued may still add to them
    free_face_maps(c);
    c->face_on = false;
    return 0;
  }
  if (c->face_on) return 0;
  if (c->ext_smax > 0)
    return fail(c, "c2r_enable_face_loss: a source of the list stands outside the mesh (c2r_set_sources_external), which the escape maps are not built for");
  if (alloc_face_maps(c)) return 1;
  c->face_on = true;
  return 0;
}

extern "C" int c2r_enable_face_loss(c2r_ctx *c, int on) {
  if (int e_ = enable_face_loss_one(c, on)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return enable_face_loss_one(r, on); });
}

extern "C" int c2r_get_face_loss_enabled(const c2r_ctx *c) { return c && c->face_on ? 1 : 0; }

// the map of one face, the devices of the context added in device order
static int face_map_to_host(c2r_ctx *c, const char *who, int face, std::vector<double> &map) {
  if (!c->face_on) return fail(c, "%s: the escape maps are off (c2r_enable_face_loss)", who);
  if (face < 0 || face > 5) return fail(c, "%s: face %d, expected 0..5 (2 * axis + high)", who, face);
  if (c->per[face >> 1]) return fail(c, "%s: face %d lies across axis %d, which is periodic: it has no map", who, face, face >> 1);
  if (c->pass_open) return fail(c, "%s: a pass opened by c2r_pass_sources_begin is still open", who);
  const FaceLayout L = face_layout(c);
  const size_t n = (size_t)face_cells(L.n, face >> 1), off = (size_t)face_map_offset(L.n, L.open, face);
  map.assign(n, 0.0);
  std::vector<double> one(n);
  std::vector<c2r_ctx *> dev(1, c);
  dev.insert(dev.end(), c->replicas.begin(), c->replicas.end());
  for (size_t k = 0; k < dev.size(); k++) {
    c2r_ctx *d = dev[k];
    if (!d->d_face_maps) return fail(c, "%s: internal: device %d has no maps", who, d->device);
    HIPCHK(c, hipSetDevice(d->device));
    HIPCHK(c, hipMemcpyAsync(k == 0 ? map.data() : one.data(), d->d_face_maps + off, sizeof(double) * n, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(c, hipStreamSynchronize(d->stream));
    if (k > 0)
      for (size_t i = 0; i < n; i++) map[i] = map[i] + one[i];
  }
  return 0;
}

extern "C" int c2r_download_face_loss(c2r_ctx *c, int face, double *map) {
  if (!c) return 1;
  if (!map) return fail(c, "c2r_download_face_loss: null argument");
  std::vector<double> m;
  if (face_map_to_host(c, "c2r_download_face_loss", face, m)) return 1;
  std::copy(m.begin(), m.end(), map);
  return 0;
}

extern "C" int c2r_get_face_loss(c2r_ctx *c, double out6[6]) {
  if (!c) return 1;
  if (!out6) return fail(c, "c2r_get_face_loss: null argument");
  if (!c->face_on) return fail(c, "c2r_get_face_loss: the escape maps are off (c2r_enable_face_loss)");
  std::vector<double> m;
  for (int face = 0; face < 6; face++) {
    out6[face] = 0.0;
    if (c->per[face >> 1]) continue;
    if (face_map_to_host(c, "c2r_get_face_loss", face, m)) return 1;
    out6[face] = face_sum(m.data(), m.size());
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
// horizon loss
static int enable_horizon_loss_one(c2r_ctx *c, int on) {
  if (!c) return 1;
  if (c->pass_open) return fail(c, "c2r_enable_horizon_loss: a pass opened by c2r_pass_sources_begin is still open (close it with c2r_pass_sources_end first)");
  HIPCHK(c, hipSetDevice(c->device));
  if (!on) {
    if (c->rim_on) HIPCHK(c, hipStreamSynchronize(c->stream)); // nothing queued may still write the buffers
    free_horizon_loss(c);
    c->rim_on = false;
    c->horizon_loss.clear();
    c->rim_last_ns = 0;
    c->rim_last_stamp = 0;
    return 0;
  }
  if (c->rim_on) return 0;
  if (c->ext_smax > 0)
    return fail(c, "c2r_enable_horizon_loss: a source of the list stands outside the mesh (c2r_set_sources_external), which the horizon loss is not built for");
  const size_t n0 = (size_t)c->g.n1, n1 = (size_t)c->g.n2, n2 = (size_t)c->g.n3;
  auto allocate = [&]() -> int {
    c->rim_terms_cap = 2 * (n1 * n2 + n0 * n2 + n0 * n1);
    HIPCHK(c, hipMalloc(&c->d_rim_terms, sizeof(double) * c->rim_terms_cap));
    for (int k = 0; k < 2; k++) {
      HIPCHK(c, hipMalloc(&c->d_rim_acc[k], sizeof(double) * BATCH_MAX));
      HIPCHK(c, hipHostMalloc(&c->h_rim[k], sizeof(double) * BATCH_MAX));
      HIPCHK(c, hipMalloc(&c->d_rim_list[k], sizeof(int) * BATCH_MAX));
      HIPCHK(c, hipHostMalloc(&c->h_rim_list[k], sizeof(int) * BATCH_MAX));
    }
    return 0;
  };
  if (allocate()) {
    free_horizon_loss(c); // (an allocation failed half way: nothing stays behind; the feature was off and stays off)
    return 1;
  }
  c->rim_on = true;
  forget_horizon_loss(c);
  return 0;
}

extern "C" int c2r_enable_horizon_loss(c2r_ctx *c, int on) {
  if (int e_ = enable_horizon_loss_one(c, on)) return e_; // (a refused call changes nothing)
  return for_replicas(c, [&](c2r_ctx *r) { return enable_horizon_loss_one(r, on); });
}

extern "C" int c2r_get_horizon_loss_enabled(const c2r_ctx *c) { return c && c->rim_on ? 1 : 0; }

// per source: the devices of the context added in device order (a source is swept by one device of a deal, the others hold 0.0)
extern "C" int c2r_get_horizon_loss(c2r_ctx *c, int nsrc, double *per_source, double *total) {
  if (!c) return 1;
  if (!c->rim_on) return fail(c, "c2r_get_horizon_loss: the horizon loss is off (c2r_enable_horizon_loss)");
  if (nsrc != c->nsrc) return fail(c, "c2r_get_horizon_loss: nsrc = %d, but c2r_set_sources gave %d sources", nsrc, c->nsrc);
  if (c->pass_open) return fail(c, "c2r_get_horizon_loss: a pass opened by c2r_pass_sources_begin is still open");
  double sum = 0.0;
  for (int s = 0; s < nsrc; s++) {
    double v = (size_t)s < c->horizon_loss.size() ? c->horizon_loss[(size_t)s] : 0.0;
    for (const c2r_ctx *r : c->replicas)
      if ((size_t)s < r->horizon_loss.size()) v = v + r->horizon_loss[(size_t)s];
    if (per_source) per_source[s] = v;
    sum = sum + v;
  }
  if (total) *total = sum;
  return 0;
}

extern "C" int c2r_download_horizon_rim(c2r_ctx *c, int *ns, int extent[3], double *terms, long long capacity) {
  if (!c) return 1;
  if (!ns || !extent || !terms) return fail(c, "c2r_download_horizon_rim: null argument");
  if (!c->rim_on) return fail(c, "c2r_download_horizon_rim: the horizon loss is off (c2r_enable_horizon_loss)");
  if (c->pass_open) return fail(c, "c2r_download_horizon_rim: a pass opened by c2r_pass_sources_begin is still open");
  // the context itself or, of a multi-device context, the device that swept a horizoned source last
  c2r_ctx *from = nullptr;
  long long stamp = 0;
  auto look = [&](c2r_ctx *r) {
    if (r->rim_last_ns > 0 && r->rim_last_stamp > stamp) { stamp = r->rim_last_stamp; from = r; }
  };
  look(c);
  for (c2r_ctx *r : c->replicas) look(r);
  if (!from) return fail(c, "c2r_download_horizon_rim: no source with a finite horizon has been swept yet");
  const long long T = rim_total(from->rim_last_ext[0], from->rim_last_ext[1], from->rim_last_ext[2]);
  *ns = from->rim_last_ns;
  for (int d = 0; d < 3; d++) extent[d] = from->rim_last_ext[d];
  if (capacity < T)
    return fail(c, "c2r_download_horizon_rim: capacity = %lld, but source %d has T = %lld terms (extents %d x %d x %d)", capacity, *ns, T,
                extent[0], extent[1], extent[2]);
  HIPCHK(c, hipSetDevice(from->device));
  HIPCHK(c, hipMemcpyAsync(terms, from->d_rim_terms, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, from->stream));
  HIPCHK(c, hipStreamSynchronize(from->stream));
  return 0;
}

extern "C" int c2r_set_sed_tables(c2r_ctx *c, int sed, const double *photo_thick, const double *photo_thin, const double *heat_thick, const double *heat_thin, int lower, int upper) {
  if (int e_ = set_sed_tables_one(c, sed, photo_thick, photo_thin, heat_thick, heat_thin, lower, upper)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_sed_tables_one(r, sed, photo_thick, photo_thin, heat_thick, heat_thin, lower, upper); });
}

extern "C" int c2r_set_sources_sed(c2r_ctx *c, int sed, const double *normflux, double s_star) {
  if (int e_ = set_sources_sed_one(c, sed, normflux, s_star)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_sources_sed_one(r, sed, normflux, s_star); });
}

extern "C" int c2r_set_source_beams(c2r_ctx *c, int nsrc, const c2r_source_beam *beams) {
  if (int e_ = set_source_beams_one(c, nsrc, beams)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_source_beams_one(r, nsrc, beams); });
}

extern "C" int c2r_get_source_beam(const c2r_ctx *c, int ns, c2r_source_beam *out) {
  if (!c || !out || ns < 1 || ns > c->nsrc) return 1;
  if (c->beams.empty()) *out = c2r_source_beam{};
  else *out = c->beams[(size_t)ns - 1];
  return 0;
}

extern "C" int c2r_set_source_horizons(c2r_ctx *c, int nsrc, const double *radius) {
  if (int e_ = set_source_horizons_one(c, nsrc, radius)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_source_horizons_one(r, nsrc, radius); });
}

extern "C" int c2r_get_source_horizon(const c2r_ctx *c, int ns, double *radius) {
  if (!c || !radius) return 1;
  if (ns < 1 || ns > c->nsrc) {
    c->err = "c2r_get_source_horizon: source " + std::to_string(ns) + " not in [1," + std::to_string(c->nsrc) + "]";
    return 1;
  }
  *radius = c->horizons.empty() ? (double)INFINITY : c->horizons[(size_t)ns - 1];
  return 0;
}

extern "C" int c2r_set_source_curves(c2r_ctx *c, int nsrc, const c2r_source_curve *curves) {
  if (int e_ = set_source_curves_one(c, nsrc, curves)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_source_curves_one(r, nsrc, curves); });
}

extern "C" int c2r_get_source_curve(const c2r_ctx *c, int ns, c2r_source_curve *out) {
  if (!c || !out) return 1;
  if (ns < 1 || ns > c->nsrc) {
    c->err = "c2r_get_source_curve: source " + std::to_string(ns) + " not in [1," + std::to_string(c->nsrc) + "]";
    return 1;
  }
  *out = c2r_source_curve{};
  out->factor[0] = 1.0;
  if (!c->curves.empty()) *out = c->curves[(size_t)ns - 1];
  return 0;
}

extern "C" int c2r_build_tables(c2r_ctx *c, const c2r_sed_setup *S, int with_heat) {
  if (int e_ = build_tables_one(c, S, with_heat)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return build_tables_one(r, S, with_heat); });
}

extern "C" int c2r_set_lls(c2r_ctx *c, int use_lls, double coldensh_lls, const float *lls_grid) {
  if (int e_ = set_lls_one(c, use_lls, coldensh_lls, lls_grid)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_lls_one(r, use_lls, coldensh_lls, lls_grid); });
}

extern "C" int c2r_set_clumping_grid(c2r_ctx *c, const float *clumping_grid) {
  if (int e_ = set_clumping_grid_one(c, clumping_grid)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_clumping_grid_one(r, clumping_grid); });
}

extern "C" int c2r_upload_state(c2r_ctx *c, const double *xh, const double *xhe, const float *temperature) {
  if (int e_ = upload_state_one(c, xh, xhe, temperature)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return upload_state_one(r, xh, xhe, temperature); });
}

extern "C" int c2r_begin_step(c2r_ctx *c) {
  if (int e_ = begin_step_one(c)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return begin_step_one(r); });
}

extern "C" int c2r_end_step(c2r_ctx *c) {
  if (int e_ = end_step_one(c)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return end_step_one(r); });
}

extern "C" int c2r_set_rates_to_zero(c2r_ctx *c) {
  if (int e_ = set_rates_to_zero_one(c)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_rates_to_zero_one(r); });
}

extern "C" int c2r_set_batch(c2r_ctx *c, int nbatch) {
  if (int e_ = set_batch_one(c, nbatch)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_batch_one(r, nbatch); });
}

// Switching forgets what earlier passes learnt about the sources (sub-box counts, hence predicted block sizes and the
// rounds swept on trust): none of it holds for the other geometry.  The column scratch stays; it only ever holds finite
// numbers, whoever wrote them.
static int set_boundaries_one(c2r_ctx *c, const int periodic[3]) {
  if (!c) return 1;
  if (c->pass_open) return fail(c, "c2r_set_boundaries: a pass opened by c2r_pass_sources_begin is still open (close it with c2r_pass_sources_end first)");
  const bool per[3] = {periodic[0] != 0, periodic[1] != 0, periodic[2] != 0};
  for (int p = 0; p < c->nplane; p++)
    if (per[c->plane[p].src.axis])
      return fail(c, "c2r_set_boundaries: plane source %d travels along axis %d, which has to stay open (remove the planes with "
                  "c2r_set_plane_sources(ctx, 0, NULL) first)", p + 1, c->plane[p].src.axis);
  for (int s = 0; s < c->nsrc; s++)
    for (int d = 0; d < 3; d++)
      if (per[d] && axis_is_external(c, s + 1, d))
        return fail(c, "c2r_set_boundaries: source %d at (%d,%d,%d) stands outside the mesh along axis %d, which has to stay open "
                    "(replace the source list first)", s + 1, c->srcpos[3 * (size_t)s], c->srcpos[3 * (size_t)s + 1],
                    c->srcpos[3 * (size_t)s + 2], d);
  for (int d = 0; d < 3; d++)
    if (per[d] && c->origin[d] != 0)
      return fail(c, "c2r_set_boundaries: the mesh has an origin along axis %d (c2r_set_mesh_origin), which has to stay open", d);
  for (int f = 0; f < 6; f++)
    if (per[f >> 1] && !c->face_exit[f].sources.empty())
      return fail(c, "c2r_set_boundaries: exit strips are selected through face %d of axis %d, which has to stay open (free them with "
                  "c2r_select_source_face_exit(ctx, %d, 0, NULL) first)", f, f >> 1, f);
  if (per[0] == c->per[0] && per[1] == c->per[1] && per[2] == c->per[2]) return 0;
  const bool want = per[0] && per[1] && per[2];
  HIPCHK(c, hipSetDevice(c->device));
  // nothing queued may still read the shell bookkeeping or the lists that are about to be replaced
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream2));
  HIPCHK(c, hipStreamSynchronize(c->stream3));
  HIPCHK(c, hipStreamSynchronize(c->stream_probe));
  c->periodic = want;
  for (int d = 0; d < 3; d++) c->per[d] = per[d];
  if (c->face_on && alloc_face_maps(c)) return 1; // other faces are open now: maps of the new sizes, zeroed
  // (an axis that opens shortens the reach of an external source along it from the periodic one to at most mesh - 1)
  c->ext_smax = external_smax(c, c->nsrc, c->srcpos.data());
  if (remake_shell_buffers(c)) return 1;
  if (c->d_point_cols) { // c2r_evolve0d's block holds the whole reach of a source: made anew at the next call
    HIPCHK(c, hipFree(c->d_point_cols));
    c->d_point_cols = nullptr;
    if (c->d_point_loss) HIPCHK(c, hipFree(c->d_point_loss));
    if (c->h_point_loss) HIPCHK(c, hipHostFree(c->h_point_loss));
    c->d_point_loss = c->h_point_loss = nullptr;
  }
  c->prev_nbox.assign((size_t)c->nsrc, 0);
  c->prev_grow.assign((size_t)c->nsrc, 0);
  c->trace.clear();
  c->trace_stamp.clear();
  c->last_src = 0;
  c->last_cols = nullptr;
  forget_horizon_loss(c);
  return 0;
}

extern "C" int c2r_set_boundaries_axes(c2r_ctx *c, const int periodic[3]) {
  if (!periodic) return c ? fail(c, "c2r_set_boundaries_axes: null argument") : 1;
  if (int e_ = set_boundaries_one(c, periodic)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_boundaries_one(r, periodic); });
}

extern "C" int c2r_set_boundaries(c2r_ctx *c, int periodic) {
  const int all[3] = {periodic, periodic, periodic};
  return c2r_set_boundaries_axes(c, all);
}

extern "C" int c2r_get_boundaries(const c2r_ctx *c) {
  if (!c || c->periodic) return 1;
  return c->per[0] || c->per[1] || c->per[2] ? 2 : 0;
}

extern "C" int c2r_get_boundaries_axes(const c2r_ctx *c, int out[3]) {
  if (!c || !out) return 1;
  for (int d = 0; d < 3; d++) out[d] = c->per[d] ? 1 : 0;
  return 0;
}

extern "C" int c2r_upload_rates(c2r_ctx *c, const double *phih, const double *phihe, const double *phiheat) {
  if (int e_ = upload_rates_one(c, phih, phihe, phiheat)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return upload_rates_one(r, phih, phihe, phiheat); });
}

extern "C" int c2r_upload_iter_state(c2r_ctx *c, const double *xh_av, const double *xhe_av, const double *xh_intermed, const double *xhe_intermed) {
  if (int e_ = upload_iter_state_one(c, xh_av, xhe_av, xh_intermed, xhe_intermed)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return upload_iter_state_one(r, xh_av, xhe_av, xh_intermed, xhe_intermed); });
}

extern "C" int c2r_enable_timing(c2r_ctx *c, int on) {
  if (int e_ = enable_timing_one(c, on)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return enable_timing_one(r, on); });
}

extern "C" int c2r_synchronize(c2r_ctx *c) {
  if (int e_ = synchronize_one(c)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return synchronize_one(r); });
}

#ifdef C2R_CHEM_NIT_HIST
// diagnostic build only: histogram of do_chemistry iterations (k_chemistry), read and optionally reset
extern "C" int c2r_debug_chem_nit(unsigned long long out[136], int reset) {
  static unsigned long long h[64 * 136];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(c2r_chem_nit), sizeof(h)) != hipSuccess) return 1;
  for (int k = 0; k < 136; k++) {
    out[k] = 0;
    for (int s = 0; s < 64; s++) out[k] += h[s * 136 + k];
  }
  if (reset) {
    memset(h, 0, sizeof(h));
    if (hipMemcpyToSymbol(HIP_SYMBOL(c2r_chem_nit), h, sizeof(h)) != hipSuccess) return 1;
  }
  return 0;
}
#endif
#ifdef C2R_RATES_COUNT
// diagnostic build only: see count_lanes (c2ray_device.hpp)
__device__ unsigned long long c2r::c2r_rates_cnt[64 * 24];
extern "C" int c2r_debug_rates_counters(unsigned long long out[24], int reset) {
  unsigned long long h[64 * 24];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(c2r::c2r_rates_cnt), sizeof(h)) != hipSuccess) return 1;
  for (int k = 0; k < 24; k++) {
    out[k] = 0;
    for (int s = 0; s < 64; s++) out[k] += h[s * 24 + k];
  }
  if (reset) {
    memset(h, 0, sizeof(h));
    if (hipMemcpyToSymbol(HIP_SYMBOL(c2r::c2r_rates_cnt), h, sizeof(h)) != hipSuccess) return 1;
  }
  return 0;
}
#endif
#include "c2ray_comm.inc"
