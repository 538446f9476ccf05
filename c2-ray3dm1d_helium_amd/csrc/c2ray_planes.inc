// Plane-parallel sources behind the C ABI (included by c2ray_hip.hip where the pass needs run_planes): the kernels, the
// queueing of a pass's planes, the plane buffers and the c2r_*plane* entry points.
//
// c2r_set_plane_sources; the per-cell rule is c2ray_plane.hpp, DESIGN.md section 3.1: a plane wave enters through an open
// face and travels along one axis, every line of cells a 1-D problem of its own.  Three stages per plane and pass, all on
// the sweep stream, one kernel each:
//   the march   k_plane_columns   one lane per line of cells, or for a tilted plane (c2r_set_plane_tilt)
//               k_plane_layer     one launch per layer; <true> carries the flux of a map along (c2r_set_plane_flux_map);
//               k_pside_layer     in its place where the plane reads the ghost strips of a neighbouring mesh or stores its edge
//                                 cells for the next one (c2r_set_plane_side_entry, c2r_enable_plane_side_exit)
//   the rates   k_plane_rates     no dependencies, one lane per cell; the flux uniform, by face cell or by cell (PlaneFlux)
//   the loss    k_plane_exit      what leaves through the far face; the flux of a map or uniform (MAPPED), the per-line
//                                 term also kept in the escape map of that face (KEEP, c2r_enable_face_loss)
//               k_pside_loss      what a tilted plane loses through its live open side faces (c2r_enable_plane_side_loss)
// A plane with a light curve (c2r_set_plane_curve, c2ray_pcurve.hpp) runs k_pcurve_rates and k_pcurve_exit for the last two.
namespace {

struct PlaneDev {
  double nf[NSED]; // NormFlux per cm^2 of face: black body, power law, quasar-like
};

// The march: lane f owns column f of the face and walks the mesh[axis] cells behind it in travel order, handing each
// cell's outgoing columns to the next as its incoming ones.  Writes the incoming columns of every cell (LLS fog applied),
// 3 doubles per cell in mesh order, and the outgoing columns of the last cell (species slowest).  Memory-bound and cheap
// next to the rates: 32 bytes read and 24 written per cell.  Along axis 0 the lanes of a wave are n1 doubles apart, but
// 16 consecutive steps of a lane stay within one 128-byte line of each grid, so the lines are fetched once.
__global__ void __launch_bounds__(BLOCK)
k_plane_columns(PlaneGeom G, StepScalars sc, double path, size_t nc, const double *__restrict__ ndens, const double *__restrict__ xh_av,
                const double *__restrict__ xhe_av, const float *__restrict__ lls_grid, const double *__restrict__ entry,
                double *__restrict__ cin_out, double *__restrict__ exit_cols) {
  const int face = G.fa * G.fb;
  const int f = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
  if (f >= face) return;
  double c_HI = 0.0, c_HeI = 0.0, c_HeII = 0.0;
  if (entry) { c_HI = entry[f]; c_HeI = entry[face + f]; c_HeII = entry[2 * face + f]; }
  long long q = (long long)plane_cell(G, f, 0);
  const long long step = G.from_high ? -(long long)G.sa : (long long)G.sa;
  for (int m = 0; m < G.na; m++, q += step) {
    const double lls = sc.use_lls ? (lls_grid ? (double)lls_grid[q] : sc.coldensh_lls) : 0.0;
    double o_HI, o_HeI, o_HeII;
    plane_cell_columns(ndens[q], xh_av[q], xhe_av[q], xhe_av[q + (long long)nc], path, sc.dr1, sc.use_lls, lls, c_HI, c_HeI, c_HeII,
                       o_HI, o_HeI, o_HeII);
    cin_out[3 * q] = c_HI; // (with the fog: what the rates and the exit loss see)
    cin_out[3 * q + 1] = c_HeI;
    cin_out[3 * q + 2] = c_HeII;
    c_HI = o_HI; c_HeI = o_HeI; c_HeII = o_HeII;
  }
  exit_cols[f] = c_HI;
  exit_cols[face + f] = c_HeI;
  exit_cols[2 * face + f] = c_HeII;
}

// One layer of the march of a tilted plane (c2r_set_plane_tilt, PlaneTilt): lane (u, v) owns face cell (u, v) of layer m
// (travel order), interpolates its incoming columns from four cells of the layer before (`prev`: that layer's outgoing
// columns, 3 x face, or the entry columns, or null = zero) and writes the fogged incoming columns into the cell's place of
// cin_out and the outgoing ones into `next`.  The layers depend on each other as the shells of a point source do, and are
// ordered the same way: one launch per layer on the sweep stream (DESIGN.md section 3.1).  prev and next are different
// buffers: every lane of the launch reads only what earlier launches wrote.
// A block is 64 x 4 face cells, a wave one row of 64 along f: its 12 loads of prev are unit-stride (shifted by at most one
// cell, and by whole rows), u and v come from the block and thread indices (no division), the wrap is a compare and an
// add.  The loads of the mesh grids are unit-stride for axis 1 and 2 and n1 doubles apart for axis 0, where 16
// consecutive layers share each 128-byte line.
// FLUX (a plane with a flux map, c2r_set_plane_flux_map): the three fluxes are carried along with the geometric weights
// (plane_layer_flux) -- 12 more loads of the layer before (`fprev`: 3 x face; the map in front of the first layer), the
// same shifted unit-stride rows as the loads of the columns, one store of 3 doubles at the cell (cell_flux, 3 per cell like
// cin_out) and one into the next flux layer (`fnext`; the last layer's is the exit flux).  All three SEDs are carried
// whether the plane uses them or not: the loads are issued together with those of the columns, and a test per SED would
// save none of the latency.  Without FLUX the three flux pointers are never read (null).
constexpr int PLANE_LAYER_BX = 64, PLANE_LAYER_BY = 4;
template <bool FLUX>
__global__ void __launch_bounds__(PLANE_LAYER_BX * PLANE_LAYER_BY)
k_plane_layer(PlaneGeom G, PlaneTilt T, StepScalars sc, int m, size_t nc, const double *__restrict__ ndens,
              const double *__restrict__ xh_av, const double *__restrict__ xhe_av, const float *__restrict__ lls_grid,
              const double *__restrict__ prev, double *__restrict__ cin_out, double *__restrict__ next,
              const double *__restrict__ fprev, double *__restrict__ cell_flux, double *__restrict__ fnext) {
  const int u = (int)blockIdx.x * PLANE_LAYER_BX + (int)threadIdx.x, v = (int)blockIdx.y * PLANE_LAYER_BY + (int)threadIdx.y;
  if (u >= G.fa || v >= G.fb) return;
  [[maybe_unused]] double nf[NSED];
  if constexpr (FLUX) plane_layer_flux(T, G.fa, G.fb, u, v, fprev, nf);
  const int face = G.fa * G.fb, f = u + G.fa * v;
  const int along = G.from_high ? G.na - 1 - m : m;
  const size_t q = (size_t)u * G.sf + (size_t)v * G.sg + (size_t)along * G.sa;
  double c_HI, c_HeI, c_HeII;
  plane_layer_in(T, G.fa, G.fb, u, v, prev, c_HI, c_HeI, c_HeII);
  const double lls = sc.use_lls ? (lls_grid ? (double)lls_grid[q] : sc.coldensh_lls) : 0.0;
  double o_HI, o_HeI, o_HeII;
  plane_cell_columns(ndens[q], xh_av[q], xhe_av[q], xhe_av[q + nc], T.path, sc.dr1, sc.use_lls, lls, c_HI, c_HeI, c_HeII, o_HI, o_HeI,
                     o_HeII);
  cin_out[3 * q] = c_HI;
  cin_out[3 * q + 1] = c_HeI;
  cin_out[3 * q + 2] = c_HeII;
  next[f] = o_HI;
  next[face + f] = o_HeI;
  next[2 * face + f] = o_HeII;
  if constexpr (FLUX)
    for (int k = 0; k < NSED; k++) {
      cell_flux[3 * q + k] = nf[k];
      fnext[k * face + f] = nf[k];
    }
}

// k_plane_layer for a plane that reads or writes side strips (side entry and side exit, c2r_set_plane_side_entry /
// c2r_enable_plane_side_exit): the same launch, the same statements, and two differences.  A corner outside an open side face
// reads the ghost strips of this layer's slot instead of 0.0 (the ghost-aware plane_layer_in / plane_layer_flux), and the lanes
// on the downstream edge of a live side store the corner c4 / F4 they have just loaded -- their own cell of the layer before --
// into the exit strips' slot m.  A kernel of its own, as the curved plane's are: a plane without strips runs k_plane_layer.
struct PlaneSideDev {
  PlaneGhost gc, gf;     // the ghost columns and ghost fluxes of slot m (null: 0.0)
  double *xc[2], *xf[2]; // the exit strips of side 0 / 1 at slot m: 3 x fb / 3 x fa columns, fluxes (null: not stored)
  int edge_f, edge_g;    // the downstream edge index of each side
};
template <bool FLUX>
__global__ void __launch_bounds__(PLANE_LAYER_BX * PLANE_LAYER_BY)
k_pside_layer(PlaneGeom G, PlaneTilt T, StepScalars sc, int m, size_t nc, const double *__restrict__ ndens,
              const double *__restrict__ xh_av, const double *__restrict__ xhe_av, const float *__restrict__ lls_grid,
              const double *__restrict__ prev, double *__restrict__ cin_out, double *__restrict__ next,
              const double *__restrict__ fprev, double *__restrict__ cell_flux, double *__restrict__ fnext, PlaneSideDev sd) {
  const int u = (int)blockIdx.x * PLANE_LAYER_BX + (int)threadIdx.x, v = (int)blockIdx.y * PLANE_LAYER_BY + (int)threadIdx.y;
  if (u >= G.fa || v >= G.fb) return;
  [[maybe_unused]] double nf[NSED];
  if constexpr (FLUX) plane_layer_flux(T, G.fa, G.fb, u, v, fprev, sd.gf, nf);
  const int face = G.fa * G.fb, f = u + G.fa * v;
  const int along = G.from_high ? G.na - 1 - m : m;
  const size_t q = (size_t)u * G.sf + (size_t)v * G.sg + (size_t)along * G.sa;
  double c_HI, c_HeI, c_HeII;
  plane_layer_in(T, G.fa, G.fb, u, v, prev, sd.gc, c_HI, c_HeI, c_HeII);
  for (int k = 0; k < 3; k++) { // the edge lanes hand on their own cell of the layer before
    if (u == sd.edge_f && sd.xc[0]) sd.xc[0][k * G.fb + v] = prev ? prev[k * face + f] : 0.0;
    if (v == sd.edge_g && sd.xc[1]) sd.xc[1][k * G.fa + u] = prev ? prev[k * face + f] : 0.0;
    if constexpr (FLUX) {
      if (u == sd.edge_f && sd.xf[0]) sd.xf[0][k * G.fb + v] = fprev[k * face + f];
      if (v == sd.edge_g && sd.xf[1]) sd.xf[1][k * G.fa + u] = fprev[k * face + f];
    }
  }
  const double lls = sc.use_lls ? (lls_grid ? (double)lls_grid[q] : sc.coldensh_lls) : 0.0;
  double o_HI, o_HeI, o_HeII;
  plane_cell_columns(ndens[q], xh_av[q], xhe_av[q], xhe_av[q + nc], T.path, sc.dr1, sc.use_lls, lls, c_HI, c_HeI, c_HeII, o_HI, o_HeI,
                     o_HeII);
  cin_out[3 * q] = c_HI;
  cin_out[3 * q + 1] = c_HeI;
  cin_out[3 * q + 2] = c_HeII;
  next[f] = o_HI;
  next[face + f] = o_HeI;
  next[2 * face + f] = o_HeII;
  if constexpr (FLUX)
    for (int k = 0; k < NSED; k++) {
      cell_flux[3 * q + k] = nf[k];
      fnext[k * face + f] = nf[k];
    }
}

// Where a cell's flux comes from: the plane's uniform normflux (PlaneDev::nf); the map at the cell's face cell, map[s][f]
// (a plane with a map at normal incidence); the three doubles k_plane_layer<true> left at the cell (a tilted one).
enum class PlaneFlux { uniform, by_face, by_cell };

// How a mesh cell (i, j, k) finds its face cell: f = i * fi + j * fj + k * fk, the coefficients from the plane's axis
// (run_planes forms them) -- no division beyond the tile decode.
struct PlaneFaceIndex {
  int fi, fj, fk;
};

// The rates of cell q from the flux nf, added to the rate grids.  The outgoing columns are formed again from the incoming
// ones (plane_cell_out, the expression the march used).
template <bool HEAT, bool MULTI>
__device__ __forceinline__ void plane_rates_cell(size_t q, size_t nc, double path, const double (&nf)[NSED], const double *__restrict__ ndens,
                                                 const double *__restrict__ xh_av, const double *__restrict__ xhe_av,
                                                 const BandDataByRow *__restrict__ bdr, const SedSet &ss, const double *__restrict__ cin,
                                                 double *__restrict__ rates, const gm::LogEntry *logtab, const gm::LogPins *pins) {
  const BandData *const bd = bdr;
  double u_HI, u_HeI, u_HeII;
  plane_cell_state(ndens[q], xh_av[q], xhe_av[q], xhe_av[q + nc], u_HI, u_HeI, u_HeII);
  const double cin_HI = cin[3 * q], cin_HeI = cin[3 * q + 1], cin_HeII = cin[3 * q + 2];
  double cout_HI, cout_HeI, cout_HeII;
  plane_cell_out(cin_HI, cin_HeI, cin_HeII, u_HI, u_HeI, u_HeII, path, cout_HI, cout_HeI, cout_HeII);
  const double h_av1 = HEAT ? xh_av[q + nc] : 0.0;
  double add[4];
  bool lit;
  if constexpr (HEAT && MULTI) // cross sections and factors band by band, as k_rates' three-SED heating kernel reads them
    lit = plane_cell_rates<HEAT, MULTI>(*bdr, ss, cin_HI, cout_HI, cin_HeI, cout_HeI, cin_HeII, cout_HeII, path, nf, h_av1, u_HI, u_HeI,
                                        u_HeII, add, logtab, pins);
  else
    lit = plane_cell_rates<HEAT, MULTI>(*bd, ss, cin_HI, cout_HI, cin_HeI, cout_HeI, cin_HeII, cout_HeII, path, nf, h_av1, u_HI, u_HeI,
                                        u_HeII, add, logtab, pins);
  if (!lit) return; // beyond max_coldensh: nothing is added
  rates[q] = rates[q] + add[0];
  rates[q + nc] = rates[q + nc] + add[1];
  rates[q + 2 * nc] = rates[q + 2 * nc] + add[2];
  if (HEAT) rates[q + 3 * nc] = rates[q + 3 * nc] + add[3];
}

// The rates of every cell from one plane, added to the rate grids: k_rates' shape -- a block is a tile of 8 x 8 x 4
// cells, a wave a 4 x 4 x 4 cube of it (neighbours see similar optical depths and take the same branches), the log's
// table in LDS -- with one source whose columns come in mesh order and whose vol_ph is dr[axis].  One lane per cell and
// not per line: the rates are some thousands of fp64 instructions per cell, and N^2 lanes would leave the device idle.
// FLUX says where the cell's flux comes from (`flux`: 3 x face with fx and face, or 3 per cell; not read for a uniform
// plane).  A dark cell of a map (plane_dark) leaves after the set-up the whole wave shares.
template <bool HEAT, bool MULTI, PlaneFlux FLUX>
__global__ void __launch_bounds__(BLOCK, MULTI ? (HEAT ? C2R_RATES_WAVES_HEAT_MULTI : 4) : (HEAT ? C2R_RATES_WAVES_HEAT : C2R_RATES_WAVES_ISO))
k_plane_rates(Grid g, double path, PlaneDev pl, PlaneFaceIndex fx, int face, const double *__restrict__ flux,
              const double *__restrict__ ndens, const double *__restrict__ xh_av, const double *__restrict__ xhe_av,
              const BandDataByRow *__restrict__ bdr, SedSet ss, const double *__restrict__ cin, double *__restrict__ rates) {
  const size_t nc = g.ncell;
  __shared__ gm::LogEntry s_logtab[256];
  s_logtab[threadIdx.x] = gm::make_log_entry((int)threadIdx.x);
  __syncthreads();
  gm::LogPins pins_ = {0.0, 0.0};
  const gm::LogPins *pins = nullptr;
  if (!HEAT) {
    pins_ = gm::pin_log_constants();
    pins = &pins_;
  }
  // the tile decode: the cell (i, j, k) of this lane
  const int ti = (g.n1 + 7) >> 3, tj = (g.n2 + 7) >> 3;
  const int tile = (int)blockIdx.x;
  const int bi = tile % ti, bj = (tile / ti) % tj, bk = tile / (ti * tj);
  const int lane = threadIdx.x & 63;
  const int w_ = threadIdx.x >> 6;
  const int i = bi * 8 + (w_ & 1) * 4 + (lane & 3), j = bj * 8 + (w_ >> 1) * 4 + ((lane >> 2) & 3), k = bk * 4 + (lane >> 4);
  if (!(i < g.n1 && j < g.n2 && k < g.n3)) return;
  const size_t q = (size_t)i + (size_t)g.n1 * ((size_t)j + (size_t)g.n2 * (size_t)k);
  if constexpr (FLUX == PlaneFlux::uniform) {
    plane_rates_cell<HEAT, MULTI>(q, nc, path, pl.nf, ndens, xh_av, xhe_av, bdr, ss, cin, rates, &s_logtab[0], pins);
  } else {
    double nf[NSED];
    if constexpr (FLUX == PlaneFlux::by_cell) {
      for (int s = 0; s < NSED; s++) nf[s] = flux[3 * q + s];
    } else {
      const int f = i * fx.fi + j * fx.fj + k * fx.fk;
      for (int s = 0; s < NSED; s++) nf[s] = flux[s * face + f];
    }
    if (plane_dark(nf)) return;
    plane_rates_cell<HEAT, MULTI>(q, nc, path, nf, ndens, xh_av, xhe_av, bdr, ss, cin, rates, &s_logtab[0], pins);
  }
}

// The loss term of line f with the flux of its last cell (`flux`: 3 x face -- the map at normal incidence, the exit flux
// of a tilted plane); 0.0 for a dark cell.
template <bool MULTI>
__device__ double pflux_exit_term(const PlaneGeom &G, const StepScalars &sc, double path, const BandData &bd, const SedSet &ss,
                                  const double *__restrict__ cin, const double *__restrict__ exit_cols, const double *__restrict__ flux,
                                  int f, int face) {
  const double nf[NSED] = {flux[f], flux[face + f], flux[2 * face + f]};
  if (plane_dark(nf)) return 0.0;
  const size_t q = plane_cell(G, f, G.na - 1);
  return plane_exit_term<MULTI>(bd, ss, cin[3 * q], exit_cols[f], cin[3 * q + 1], exit_cols[face + f], cin[3 * q + 2],
                                exit_cols[2 * face + f], nf, sc.vol, path);
}

// What the plane loses through the far face: lane f evaluates photo_out of the last cell of column f
// (plane_exit_term), the block adds its 256 terms in block_sum's fixed tree; k_loss_finish then adds the block sums in
// order.  No float atomics: the same bits every time.  MAPPED: the flux of line f from `flux` (pflux_exit_term) instead of
// the plane's uniform one.  KEEP (escape maps): the same terms, the same block sums, and map = map + term at the line's
// face cell of the plane's far face (`map`: that face's map; a plane's face cells are the map's, in its order).
template <bool MULTI, bool MAPPED, bool KEEP>
__global__ void __launch_bounds__(BLOCK)
k_plane_exit(PlaneGeom G, StepScalars sc, double path, PlaneDev pl, const double *__restrict__ flux, const BandData *__restrict__ bd,
             SedSet ss, const double *__restrict__ cin, const double *__restrict__ exit_cols, double *__restrict__ partial,
             double *__restrict__ map) {
  __shared__ double sh[BLOCK / 64];
  const int face = G.fa * G.fb;
  const int f = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
  double term = 0.0;
  if (f < face) {
    if constexpr (MAPPED) {
      term = pflux_exit_term<MULTI>(G, sc, path, *bd, ss, cin, exit_cols, flux, f, face);
    } else {
      const size_t q = plane_cell(G, f, G.na - 1);
      term = plane_exit_term<MULTI>(*bd, ss, cin[3 * q], exit_cols[f], cin[3 * q + 1], exit_cols[face + f], cin[3 * q + 2],
                                    exit_cols[2 * face + f], pl.nf, sc.vol, path);
    }
    if constexpr (KEEP) map[f] = map[f] + term;
  }
  const double bs = block_sum(term, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = bs;
}

// Plane light curves (c2r_set_plane_curve; the rule is c2ray_pcurve.hpp): a plane with a curve runs the two kernels below in
// the place of k_plane_rates and k_plane_exit, behind the same march.

// plane_rates_cell for the three-SED heating kernel of a curved plane: the same statements, the fluxes a PlaneCurveFlux
// (each product formed where the band loops use it, not kept in registers through them).
__device__ __forceinline__ void pcurve_rates_cell_heat3(size_t q, size_t nc, double path, const PlaneCurveFlux &nf, const double *__restrict__ ndens,
                                                        const double *__restrict__ xh_av, const double *__restrict__ xhe_av,
                                                        const BandDataByRow *__restrict__ bdr, const SedSet &ss, const double *__restrict__ cin,
                                                        double *__restrict__ rates, const gm::LogEntry *logtab) {
  double u_HI, u_HeI, u_HeII;
  plane_cell_state(ndens[q], xh_av[q], xhe_av[q], xhe_av[q + nc], u_HI, u_HeI, u_HeII);
  const double cin_HI = cin[3 * q], cin_HeI = cin[3 * q + 1], cin_HeII = cin[3 * q + 2];
  double cout_HI, cout_HeI, cout_HeII;
  plane_cell_out(cin_HI, cin_HeI, cin_HeII, u_HI, u_HeI, u_HeII, path, cout_HI, cout_HeI, cout_HeII);
  double add[4];
  if (!plane_cell_rates<true, true>(*bdr, ss, cin_HI, cout_HI, cin_HeI, cout_HeI, cin_HeII, cout_HeII, path, nf, xh_av[q + nc], u_HI, u_HeI,
                                    u_HeII, add, logtab, nullptr))
    return; // beyond max_coldensh: nothing is added
  rates[q] = rates[q] + add[0];
  rates[q + nc] = rates[q + nc] + add[1];
  rates[q + 2 * nc] = rates[q + 2 * nc] + add[2];
  rates[q + 3 * nc] = rates[q + 3 * nc] + add[3];
}

// k_plane_rates for a plane with a curve: the same tile, the same cube per wave, the same table in LDS.  A cube spans four
// layers whatever the axis, so the factor f -- and with it the fluxes -- is a value per lane: each lane finds its layer from
// its own (i, j, k) (PlaneLayerIndex), forms f by curve_factor's compares and selects on the record `cv` (a kernel argument:
// scalar registers, read at constant places) and leaves where its layer is unlit (f == 0.0) or its unscaled fluxes are dark.
// Then one rounded product per SED and plane_rates_cell, as ever.  The three-SED heating kernel forms each product where it
// is used instead (pcurve_rates_cell_heat3).
template <bool HEAT, bool MULTI, PlaneFlux FLUX>
__global__ void __launch_bounds__(BLOCK, MULTI ? (HEAT ? C2R_RATES_WAVES_HEAT_MULTI : 4) : (HEAT ? C2R_RATES_WAVES_HEAT : C2R_RATES_WAVES_ISO))
k_pcurve_rates(Grid g, double path, PlaneDev pl, PlaneFaceIndex fx, int face, const double *__restrict__ flux, PlaneCurveDev cv,
               PlaneLayerIndex lx, const double *__restrict__ ndens, const double *__restrict__ xh_av, const double *__restrict__ xhe_av,
               const BandDataByRow *__restrict__ bdr, SedSet ss, const double *__restrict__ cin, double *__restrict__ rates) {
  const size_t nc = g.ncell;
  __shared__ gm::LogEntry s_logtab[256];
  s_logtab[threadIdx.x] = gm::make_log_entry((int)threadIdx.x);
  __syncthreads();
  gm::LogPins pins_ = {0.0, 0.0};
  const gm::LogPins *pins = nullptr;
  if (!HEAT) {
    pins_ = gm::pin_log_constants();
    pins = &pins_;
  }
  // the tile decode: the cell (i, j, k) of this lane
  const int ti = (g.n1 + 7) >> 3, tj = (g.n2 + 7) >> 3;
  const int tile = (int)blockIdx.x;
  const int bi = tile % ti, bj = (tile / ti) % tj, bk = tile / (ti * tj);
  const int lane = threadIdx.x & 63;
  const int w_ = threadIdx.x >> 6;
  const int i = bi * 8 + (w_ & 1) * 4 + (lane & 3), j = bj * 8 + (w_ >> 1) * 4 + ((lane >> 2) & 3), k = bk * 4 + (lane >> 4);
  if (!(i < g.n1 && j < g.n2 && k < g.n3)) return;
  const double cf = pcurve_factor(cv, pcurve_layer(lx, i, j, k), path);
  if (cf == 0.0) return; // an unlit layer
  const size_t q = (size_t)i + (size_t)g.n1 * ((size_t)j + (size_t)g.n2 * (size_t)k);
  double nfu[NSED]; // the unscaled fluxes
  if constexpr (FLUX == PlaneFlux::uniform) {
    for (int s = 0; s < NSED; s++) nfu[s] = pl.nf[s];
  } else if constexpr (FLUX == PlaneFlux::by_cell) {
    for (int s = 0; s < NSED; s++) nfu[s] = flux[3 * q + s];
  } else {
    const int f = i * fx.fi + j * fx.fj + k * fx.fk;
    for (int s = 0; s < NSED; s++) nfu[s] = flux[s * face + f];
  }
  if (plane_dark(nfu)) return;
  if constexpr (HEAT && MULTI) {
    pcurve_rates_cell_heat3(q, nc, path, PlaneCurveFlux{nfu[0], nfu[1], nfu[2], cf}, ndens, xh_av, xhe_av, bdr, ss, cin, rates, &s_logtab[0]);
  } else {
    double nf[NSED];
    pcurve_fluxes(nfu, cf, nf);
    plane_rates_cell<HEAT, MULTI>(q, nc, path, nf, ndens, xh_av, xhe_av, bdr, ss, cin, rates, &s_logtab[0], pins);
  }
}

// k_plane_exit for a plane with a curve: `cf` is the factor of the last layer (the host forms it with the function the lanes of
// k_pcurve_rates use).  The same terms with nf*cf for nf, 0.0 for an unlit last layer or a dark line; the same block sums,
// the same k_loss_finish behind it, the same map = map + term.
template <bool MULTI, bool MAPPED, bool KEEP>
__global__ void __launch_bounds__(BLOCK)
k_pcurve_exit(PlaneGeom G, StepScalars sc, double path, PlaneDev pl, const double *__restrict__ flux, double cf,
              const BandData *__restrict__ bd, SedSet ss, const double *__restrict__ cin, const double *__restrict__ exit_cols,
              double *__restrict__ partial, double *__restrict__ map) {
  __shared__ double sh[BLOCK / 64];
  const int face = G.fa * G.fb;
  const int f = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
  double term = 0.0;
  if (f < face) {
    double nfu[NSED];
    for (int s = 0; s < NSED; s++) nfu[s] = MAPPED ? flux[s * face + f] : pl.nf[s];
    if (cf != 0.0 && !plane_dark(nfu)) {
      double nf[NSED];
      pcurve_fluxes(nfu, cf, nf);
      const size_t q = plane_cell(G, f, G.na - 1);
      term = plane_exit_term<MULTI>(*bd, ss, cin[3 * q], exit_cols[f], cin[3 * q + 1], exit_cols[face + f], cin[3 * q + 2],
                                    exit_cols[2 * face + f], nf, sc.vol, path);
    }
    if constexpr (KEEP) map[f] = map[f] + term;
  }
  const double bs = block_sum(term, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = bs;
}

// Side loss (c2r_enable_plane_side_loss; the rule is c2ray_pside.hpp): what a tilted plane loses through the open side face
// `side` leaves through.  One lane per cell of that mesh face, in the order of its escape map: the lane's mesh cell is the
// downstream edge cell behind the face cell, its layer m the cell's place along the plane's axis.  A cell of the layers
// m <= na - 2 gives plane_exit_term of its own columns (the incoming ones from cin, the outgoing ones formed again by
// plane_cell_out) and of the flux it used (uniform, or what the layers left per cell; times the curve factor of its layer),
// times the side's weight; the last layer gives 0.0 (its whole term is the far face's).  The sum as in k_plane_exit: the
// block's 256 terms in block_sum's tree, the block sums in order by k_loss_finish.  KEEP: map = map + term at the face cell.
template <bool MULTI, bool MAPPED, bool CURVED, bool KEEP>
__global__ void __launch_bounds__(BLOCK)
k_pside_loss(Grid g, PlaneGeom G, PlaneTilt T, StepScalars sc, int side, PlaneDev pl, const double *__restrict__ cell_flux,
             PlaneCurveDev cv, const double *__restrict__ ndens, const double *__restrict__ xh_av, const double *__restrict__ xhe_av,
             const BandData *__restrict__ bd, SedSet ss, const double *__restrict__ cin, double *__restrict__ partial,
             double *__restrict__ map) {
  __shared__ double sh[BLOCK / 64];
  const int n[3] = {g.n1, g.n2, g.n3};
  const int f_ax = face_axis_a(G.axis), g_ax = face_axis_b(G.axis);
  const int s_ax = side == 0 ? f_ax : g_ax;
  const int face = pside_face(s_ax, side == 0 ? T.e_f : T.e_g);
  const int sf = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
  double term = 0.0;
  if (sf < face_cells(n, s_ax)) {
    int mc[3];
    face_cell_decode(n, face, sf, mc);
    const int along = face_pick(G.axis, mc[0], mc[1], mc[2]);
    const int m = G.from_high ? G.na - 1 - along : along;
    if (m < G.na - 1) {
      const int u = face_pick(f_ax, mc[0], mc[1], mc[2]), v = face_pick(g_ax, mc[0], mc[1], mc[2]);
      const size_t q = (size_t)mc[0] + (size_t)g.n1 * ((size_t)mc[1] + (size_t)g.n2 * (size_t)mc[2]);
      double w0, w1;
      pside_weights(T, G.fa, G.fb, u, v, w0, w1);
      double nfu[NSED];
      for (int s = 0; s < NSED; s++) nfu[s] = MAPPED ? cell_flux[3 * q + s] : pl.nf[s];
      const double cf = CURVED ? pcurve_factor(cv, m, T.path) : 1.0;
      if (cf != 0.0 && !plane_dark(nfu)) {
        double nf[NSED];
        if constexpr (CURVED) pcurve_fluxes(nfu, cf, nf);
        else
          for (int s = 0; s < NSED; s++) nf[s] = nfu[s];
        double u_HI, u_HeI, u_HeII, o_HI, o_HeI, o_HeII;
        plane_cell_state(ndens[q], xh_av[q], xhe_av[q], xhe_av[q + g.ncell], u_HI, u_HeI, u_HeII);
        const double c_HI = cin[3 * q], c_HeI = cin[3 * q + 1], c_HeII = cin[3 * q + 2];
        plane_cell_out(c_HI, c_HeI, c_HeII, u_HI, u_HeI, u_HeII, T.path, o_HI, o_HeI, o_HeII);
        const double base = plane_exit_term<MULTI>(*bd, ss, c_HI, o_HI, c_HeI, o_HeI, c_HeII, o_HeII, nf, sc.vol, T.path);
        term = pside_term(base, side == 0 ? w0 : w1);
      }
    }
    if constexpr (KEEP) map[sf] = map[sf] + term;
  }
  const double bs = block_sum(term, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = bs;
}

} // namespace

// ---------------------------------------------------------------------------------------------
// host side
static int plane_face_cells(const c2r_ctx *c, int axis) {
  const PlaneGeom G = plane_geometry(c->g.n1, c->g.n2, c->g.n3, axis, 0);
  return G.fa * G.fb;
}

// The planes of a pass (0-based numbers, in order), queued on the sweep stream: the march, the rates, the exit loss of each,
// one plane after the other -- they share the column scratch, and every addition to a rate grid is grid = grid + term in
// plane order.  The rate grids must hold what they are to be added to (the caller has carried out a pending zeroing).
static int run_planes(PassCtx &P, const std::vector<int> &planes) {
  c2r_ctx *c = P.c;
  const Grid &g = c->g;
  SedSet ss = P.ss; // a plane's SEDs need the tables only, whatever the point sources use
  for (int k = 0; k < 2; k++) {
    const bool on = c->have_sed[k];
    ss.photo_thick[k + 1] = on ? c->d_sed_tab[k][0] : nullptr;
    ss.photo_thin[k + 1] = on ? c->d_sed_tab[k][1] : nullptr;
    ss.heat_thick[k + 1] = on && c->have_sed_heat[k] ? c->d_heat_woven[k + 1][0] : nullptr;
    ss.heat_thin[k + 1] = on && c->have_sed_heat[k] ? c->d_heat_woven[k + 1][1] : nullptr;
    ss.lo[k + 1] = on ? c->sed_lo[k] : 0;
    ss.hi[k + 1] = on ? c->sed_hi[k] : 0;
  }
  const int tiles = ((g.n1 + 7) / 8) * ((g.n2 + 7) / 8) * ((g.n3 + 3) / 4);
  // a tilted plane (c2r_set_plane_tilt): the weights and the path from the dr of this pass, the wrap from its boundaries;
  // refused before anything is queued where dr has changed so that the beam moves more than a cell sideways per layer
  PlaneTilt tilt_of[PLANE_MAX] = {};
  for (int p : planes) {
    const c2r_ctx::Plane &pn = c->plane[p];
    if (!plane_tilted(pn.tilt)) continue;
    const double dr[3] = {P.sc.dr1, P.sc.dr2, P.sc.dr3};
    const int per[3] = {c->per[0], c->per[1], c->per[2]};
    tilt_of[p] = PlaneTilt(pn.tilt, dr, pn.src.axis, per);
    if (!tilt_of[p].valid())
      return fail(c, "plane %d: with the cell sizes of this pass its tilt moves the beam %g and %g cells sideways per layer, more than 1 "
                  "(c2r_set_plane_tilt)", p + 1, tilt_of[p].a_f, tilt_of[p].a_g);
    if (!c->d_plane_layer[0] || !c->d_plane_layer[1]) return fail(c, "plane %d: tilted, but the layer buffers are missing", p + 1);
    if (pn.fmap_set && (!c->d_pflux_layer[0] || !c->d_pflux_layer[1] || !c->d_pflux_cell))
      return fail(c, "plane %d: tilted with a flux map, but the flux buffers are missing", p + 1);
  }
  for (int p : planes) {
    c2r_ctx::Plane &pn = c->plane[p];
    const c2r_plane_source &pl = pn.src;
    PlaneDev pd;
    for (int s = 0; s < NSED; s++) pd.nf[s] = pl.normflux[s];
    const bool mapped = pn.fmap_set; // a flux map replaces normflux[] (c2r_set_plane_flux_map)
    bool uses[2] = {mapped ? pn.fmap_uses[0] : pd.nf[1] != 0.0, mapped ? pn.fmap_uses[1] : pd.nf[2] != 0.0};
    if (mapped) // ... or a set side-entry flux strip has a flux of that SED (c2r_set_plane_side_entry)
      for (int s = 0; s < 3; s++)
        for (int k = 0; k < 2; k++) uses[k] = uses[k] || (pn.side_inf_set[s] && pn.side_inf_uses[s][k]);
    const bool multi = uses[0] || uses[1];
    for (int k = 0; k < 2; k++) {
      if (uses[k] && !c->have_sed[k]) return fail(c, "plane %d: flux of SED %d without c2r_set_sed_tables(%d)", p + 1, k + 1, k + 1);
      if (uses[k] && !c->isothermal && !c->have_sed_heat[k])
        return fail(c, "plane %d: non-isothermal run needs the heating tables of SED %d", p + 1, k + 1);
    }
    const PlaneGeom G = plane_geometry(g.n1, g.n2, g.n3, pl.axis, pl.from_high);
    const bool tilted = plane_tilted(pn.tilt);
    const PlaneTilt &T = tilt_of[p];
    const double path = tilted ? T.path : (pl.axis == 0 ? P.sc.dr1 : (pl.axis == 1 ? P.sc.dr2 : P.sc.dr3));
    const int face = G.fa * G.fb, fblk = (face + BLOCK - 1) / BLOCK;
    hipEvent_t ev[3] = {};
    for (hipEvent_t &e : ev)
      if (c->timing && pool_event(c, &e)) return 1;
    if (c->timing) HIPCHK(c, hipEventRecord(ev[0], c->stream));

    // the march: the incoming columns of every cell into d_plane_cin, the outgoing ones of the last layer into d_exit
    const float *lls = c->lls_on_grid ? c->d_lls : nullptr;
    const double *entry = pn.entry_set ? pn.d_entry : nullptr;
    const double *exit_flux = nullptr; // 3 x face: the flux of the last cell of every line of a plane with a map
    pn.side_out_valid = pn.side_out_on; // (c2r_download_plane_side_exit: no side is live at normal incidence)
    pn.side_out_live[0] = pn.side_out_live[1] = false;
    pn.side_out_mapped = mapped;
    if (tilted) { // one launch per layer, in travel order; with a map the flux is carried along, the last layer's is the exit flux
      const dim3 lgrid((unsigned)((G.fa + PLANE_LAYER_BX - 1) / PLANE_LAYER_BX), (unsigned)((G.fb + PLANE_LAYER_BY - 1) / PLANE_LAYER_BY));
      const double *prev = entry, *fprev = mapped ? pn.d_fmap : nullptr;
      // side entry and side exit: only a live side's strips are read or written; the corner line needs both sides live.  A plane
      // that uses neither runs the instances it always ran.
      const bool live[2] = {pside_live(pn.tilt[0], T.wrap_f), pside_live(pn.tilt[1], T.wrap_g)};
      const bool ghost_live[3] = {live[0], live[1], live[0] && live[1]};
      const size_t slot[3] = {3 * (size_t)G.fb, 3 * (size_t)G.fa, 3};
      bool sides = pn.side_out_on && (live[0] || live[1]);
      for (int s = 0; s < 3; s++) sides = sides || (ghost_live[s] && pn.side_in_set[s]);
      for (int m = 0; m < G.na; m++) {
        const bool last = m == G.na - 1;
        double *next = last ? pn.d_exit : c->d_plane_layer[m & 1];
        double *fnext = mapped ? (last ? pn.d_fexit : c->d_pflux_layer[m & 1]) : nullptr;
        PlaneSideDev sd = {};
        if (sides) {
          const double *gc[3], *gf[3];
          for (int s = 0; s < 3; s++) {
            gc[s] = ghost_live[s] && pn.side_in_set[s] ? pn.d_side_in[s] + (size_t)m * slot[s] : nullptr;
            gf[s] = mapped && ghost_live[s] && pn.side_inf_set[s] ? pn.d_side_inf[s] + (size_t)m * slot[s] : nullptr;
          }
          sd.gc = PlaneGhost{{gc[0], gc[1]}, gc[2]};
          sd.gf = PlaneGhost{{gf[0], gf[1]}, gf[2]};
          for (int s = 0; s < 2; s++) {
            sd.xc[s] = pn.side_out_on && live[s] ? pn.d_side_out[s] + (size_t)m * slot[s] : nullptr;
            sd.xf[s] = pn.side_out_on && live[s] && mapped ? pn.d_side_outf[s] + (size_t)m * slot[s] : nullptr;
          }
          sd.edge_f = pside_edge(T.e_f, G.fa);
          sd.edge_g = pside_edge(T.e_g, G.fb);
        }
        with_flag(mapped, [&](auto flux) {
          if (sides) {
            hipLaunchKernelGGL(k_pside_layer<decltype(flux)::value>, lgrid, dim3(PLANE_LAYER_BX, PLANE_LAYER_BY), 0, c->stream, G, T, P.sc, m,
                               g.ncell, c->d_ndens, c->d_xh_av, c->d_xhe_av, lls, prev, c->d_plane_cin, next, fprev,
                               mapped ? c->d_pflux_cell : nullptr, fnext, sd);
            return;
          }
          hipLaunchKernelGGL(k_plane_layer<decltype(flux)::value>, lgrid, dim3(PLANE_LAYER_BX, PLANE_LAYER_BY), 0, c->stream, G, T, P.sc, m,
                             g.ncell, c->d_ndens, c->d_xh_av, c->d_xhe_av, lls, prev, c->d_plane_cin, next, fprev,
                             mapped ? c->d_pflux_cell : nullptr, fnext);
        });
        prev = next;
        fprev = fnext;
      }
      pn.side_out_live[0] = pn.side_out_on && live[0];
      pn.side_out_live[1] = pn.side_out_on && live[1];
      c->tm.sweep_launches += G.na;
      if (mapped) exit_flux = pn.d_fexit;
    } else {
      hipLaunchKernelGGL(k_plane_columns, dim3(fblk), dim3(BLOCK), 0, c->stream, G, P.sc, path, g.ncell, c->d_ndens, c->d_xh_av, c->d_xhe_av,
                         lls, entry, c->d_plane_cin, pn.d_exit);
      c->tm.sweep_launches++;
      if (mapped) { // normal incidence: every cell of line f sees map[k][f], and so does the next slab
        exit_flux = pn.d_fmap;
        HIPCHK(c, hipMemcpyAsync(pn.d_fexit, pn.d_fmap, sizeof(double) * 3 * (size_t)face, hipMemcpyDeviceToDevice, c->stream));
      }
    }
    pn.fexit_valid = mapped;
    if (c->timing) HIPCHK(c, hipEventRecord(ev[1], c->stream));

    // the rates: the flux uniform, or of the cell's own -- the map by face cell, or what the layers left per cell
    const PlaneFaceIndex fx = {pl.axis == 0 ? 0 : 1, pl.axis == 0 ? 1 : (pl.axis == 1 ? 0 : g.n1), pl.axis == 2 ? 0 : (pl.axis == 0 ? g.n2 : g.n1)};
    // a plane with a curve (c2r_set_plane_curve): its record, and the factor of the last layer for the exit loss
    const bool curved = pn.curve_set;
    PlaneCurveDev cv = {};
    double cf_last = 1.0;
    if (curved) {
      pcurve_fill(pn.curve.nstep, pn.curve.depth, pn.curve.factor, pn.curve.layer0, pn.curve.depth0, cv);
      cf_last = pcurve_factor(cv, G.na - 1, path);
    }
    const PlaneLayerIndex lx = plane_layer_index(pl.axis, pl.from_high, G.na);
    auto rates = [&](auto flux, const double *field) {
      with_flag(!c->isothermal, [&](auto heat) { with_flag(multi, [&](auto three) {
        if (curved) {
          const auto kernel = k_pcurve_rates<decltype(heat)::value, decltype(three)::value, decltype(flux)::value>;
          hipLaunchKernelGGL(kernel, dim3(tiles), dim3(BLOCK), 0, c->stream, g, path, pd, fx, face, field, cv, lx, c->d_ndens, c->d_xh_av,
                             c->d_xhe_av, c->d_bands, ss, c->d_plane_cin, c->d_rates);
          return;
        }
        const auto kernel = k_plane_rates<decltype(heat)::value, decltype(three)::value, decltype(flux)::value>;
        hipLaunchKernelGGL(kernel, dim3(tiles), dim3(BLOCK), 0, c->stream, g, path, pd, fx, face, field, c->d_ndens, c->d_xh_av,
                           c->d_xhe_av, c->d_bands, ss, c->d_plane_cin, c->d_rates);
      }); });
    };
    if (!mapped) rates(std::integral_constant<PlaneFlux, PlaneFlux::uniform>{}, nullptr);
    else if (tilted) rates(std::integral_constant<PlaneFlux, PlaneFlux::by_cell>{}, c->d_pflux_cell);
    else rates(std::integral_constant<PlaneFlux, PlaneFlux::by_face>{}, pn.d_fmap);

    // the exit loss; with escape maps the same sum with every line's term kept, at the far face
    double *map = nullptr;
    if (c->d_face_maps) {
      const FaceLayout L = face_layout(c);
      map = c->d_face_maps + face_map_offset(L.n, L.open, 2 * pl.axis + (1 - pl.from_high));
    }
    with_flag(multi, [&](auto three) { with_flag(mapped, [&](auto from_map) { with_flag(map != nullptr, [&](auto keep) {
      if (curved) {
        const auto kernel = k_pcurve_exit<decltype(three)::value, decltype(from_map)::value, decltype(keep)::value>;
        hipLaunchKernelGGL(kernel, dim3(fblk), dim3(BLOCK), 0, c->stream, G, P.sc, path, pd, exit_flux, cf_last, c->d_bands, ss,
                           c->d_plane_cin, pn.d_exit, c->d_plane_partial, map);
        return;
      }
      const auto kernel = k_plane_exit<decltype(three)::value, decltype(from_map)::value, decltype(keep)::value>;
      hipLaunchKernelGGL(kernel, dim3(fblk), dim3(BLOCK), 0, c->stream, G, P.sc, path, pd, exit_flux, c->d_bands, ss, c->d_plane_cin,
                         pn.d_exit, c->d_plane_partial, map);
    }); }); });
    hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(BLOCK), 0, c->stream, c->d_plane_partial, fblk, fblk, c->d_plane_loss + p);
    // the side loss (c2r_enable_plane_side_loss): one sum per live side, side 0 first; with escape maps every term kept at the
    // side face the beam leaves through
    pn.side_ran[0] = pn.side_ran[1] = false;
    if (c->side_loss_on && tilted) {
      const int side_axis[2] = {face_axis_a(pl.axis), face_axis_b(pl.axis)};
      const int e[2] = {T.e_f, T.e_g}, wrap[2] = {T.wrap_f, T.wrap_g};
      const FaceLayout L = face_layout(c);
      for (int s = 0; s < 2; s++) {
        if (!pside_live(pn.tilt[s], wrap[s])) continue;
        const int cells = face_cells(L.n, side_axis[s]), sblk = (cells + BLOCK - 1) / BLOCK;
        double *smap = c->d_face_maps ? c->d_face_maps + face_map_offset(L.n, L.open, pside_face(side_axis[s], e[s])) : nullptr;
        with_flag(multi, [&](auto three) { with_flag(mapped, [&](auto from_map) { with_flag(curved, [&](auto with_curve) {
          with_flag(smap != nullptr, [&](auto keep) {
            const auto kernel = k_pside_loss<decltype(three)::value, decltype(from_map)::value, decltype(with_curve)::value, decltype(keep)::value>;
            hipLaunchKernelGGL(kernel, dim3(sblk), dim3(BLOCK), 0, c->stream, g, G, T, P.sc, s, pd, mapped ? c->d_pflux_cell : nullptr, cv,
                               c->d_ndens, c->d_xh_av, c->d_xhe_av, c->d_bands, ss, c->d_plane_cin, c->d_side_partial, smap);
          });
        }); }); });
        hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(BLOCK), 0, c->stream, c->d_side_partial, sblk, sblk, c->d_side_loss + 2 * p + s);
        HIPCHK(c, hipMemcpyAsync(c->h_side_loss + 2 * p + s, c->d_side_loss + 2 * p + s, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        pn.side_ran[s] = true;
        c->tm.rates_launches += 2;
      }
    }
    HIPCHK(c, hipGetLastError());
    c->tm.rates_launches += 3;
    if (c->timing) {
      HIPCHK(c, hipEventRecord(ev[2], c->stream));
      const hipEvent_t quad[4] = {ev[0], ev[1], ev[1], ev[2]}; // sweep start, sweep end, rates start, rates end (pass_finish)
      P.tev.insert(P.tev.end(), quad, quad + 4);
    }
    HIPCHK(c, hipMemcpyAsync(c->h_plane_loss + p, c->d_plane_loss + p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (!c->isothermal) c->phiheat_dirty = true;
    pn.stamp = P.stamp;
    c->pass_planes.push_back(p);
  }
  return 0;
}

// the device and pinned buffers of the plane sources (c2r_set_plane_sources makes them, removal and c2r_destroy free
// them), and every plane's record back to what a new context has
static void free_plane_buffers(c2r_ctx *c) {
  for (c2r_ctx::Plane &pn : c->plane) {
    for (double *b : {pn.d_entry, pn.d_exit, pn.d_fmap, pn.d_fexit, pn.d_side_in[0], pn.d_side_in[1], pn.d_side_in[2], pn.d_side_inf[0],
                      pn.d_side_inf[1], pn.d_side_inf[2], pn.d_side_out[0], pn.d_side_out[1], pn.d_side_outf[0], pn.d_side_outf[1]})
      if (b) (void)hipFree(b);
    pn = c2r_ctx::Plane{};
  }
  double **shared[] = {&c->d_plane_layer[0], &c->d_plane_layer[1], &c->d_pflux_layer[0], &c->d_pflux_layer[1], &c->d_pflux_cell,
                       &c->d_plane_cin, &c->d_plane_partial, &c->d_plane_loss};
  for (double **b : shared) {
    if (*b) (void)hipFree(*b);
    *b = nullptr;
  }
  if (c->h_plane_loss) (void)hipHostFree(c->h_plane_loss);
  c->h_plane_loss = nullptr;
}

static int set_plane_sources_one(c2r_ctx *c, int nplane, const c2r_plane_source *planes) {
  if (!c) return 1;
  if (c->pass_open) return fail(c, "c2r_set_plane_sources: a pass opened by c2r_pass_sources_begin is still open (close it with c2r_pass_sources_end first)");
  if (nplane < 0 || nplane > PLANE_MAX) return fail(c, "c2r_set_plane_sources: %d planes, expected 0..%d", nplane, PLANE_MAX);
  if (nplane > 0 && !planes) return fail(c, "c2r_set_plane_sources: null argument");
  for (int p = 0; p < nplane; p++) {
    const c2r_plane_source &pl = planes[p];
    if (pl.axis < 0 || pl.axis > 2) return fail(c, "c2r_set_plane_sources: plane %d: axis %d, expected 0, 1 or 2", p + 1, pl.axis);
    if (pl.from_high != 0 && pl.from_high != 1) return fail(c, "c2r_set_plane_sources: plane %d: from_high %d, expected 0 or 1", p + 1, pl.from_high);
    if (c->per[pl.axis])
      return fail(c, "c2r_set_plane_sources: plane %d travels along axis %d, which is periodic (open it with c2r_set_boundaries_axes first)",
                  p + 1, pl.axis);
    for (int k = 0; k < NSED; k++)
      if (!(pl.normflux[k] >= 0.0) || !std::isfinite(pl.normflux[k]))
        return fail(c, "c2r_set_plane_sources: plane %d: normflux[%d] = %g", p + 1, k, pl.normflux[k]);
    for (int k = 0; k < 2; k++)
      if (pl.normflux[k + 1] != 0.0 && !c->have_sed[k])
        return fail(c, "c2r_set_plane_sources: plane %d has a flux of SED %d, whose tables have not been set (c2r_set_sed_tables(%d))",
                    p + 1, k + 1, k + 1);
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream)); // nothing queued may still use the buffers that are about to go
  free_plane_buffers(c);
  c->nplane = 0;
  c->pass_planes.clear();
  if (nplane == 0) return 0;
  int face_max = 0;
  HIPCHK(c, hipMalloc(&c->d_plane_cin, sizeof(double) * 3 * c->g.ncell));
  for (int p = 0; p < nplane; p++) {
    c2r_ctx::Plane &pn = c->plane[p];
    const size_t n3 = 3 * (size_t)plane_face_cells(c, planes[p].axis);
    face_max = std::max(face_max, (int)(n3 / 3));
    HIPCHK(c, hipMalloc(&pn.d_entry, sizeof(double) * n3));
    HIPCHK(c, hipMalloc(&pn.d_exit, sizeof(double) * n3));
    HIPCHK(c, zero_device(pn.d_exit, sizeof(double) * n3, c->stream));
  }
  HIPCHK(c, hipMalloc(&c->d_plane_partial, sizeof(double) * (size_t)((face_max + BLOCK - 1) / BLOCK)));
  HIPCHK(c, hipMalloc(&c->d_plane_loss, sizeof(double) * PLANE_MAX));
  HIPCHK(c, hipHostMalloc(&c->h_plane_loss, sizeof(double) * PLANE_MAX));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int p = 0; p < nplane; p++) c->plane[p].src = planes[p];
  c->nplane = nplane;
  return 0;
}

extern "C" int c2r_set_plane_sources(c2r_ctx *c, int nplane, const c2r_plane_source *planes) {
  if (int e_ = set_plane_sources_one(c, nplane, planes)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_plane_sources_one(r, nplane, planes); });
}

extern "C" int c2r_get_plane_count(const c2r_ctx *c) { return c ? c->nplane : 0; }

static int set_plane_entry_columns_one(c2r_ctx *c, int plane, const double *cols3) {
  if (!c) return 1;
  if (plane < 1 || plane > c->nplane) return fail(c, "c2r_set_plane_entry_columns: plane %d not in [1,%d]", plane, c->nplane);
  if (c->pass_open) return fail(c, "c2r_set_plane_entry_columns: a pass opened by c2r_pass_sources_begin is still open");
  c2r_ctx::Plane &pn = c->plane[plane - 1];
  pn.entry_set = false;
  if (!cols3) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n3 = 3 * (size_t)plane_face_cells(c, pn.src.axis);
  HIPCHK(c, hipMemcpyAsync(pn.d_entry, cols3, sizeof(double) * n3, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  pn.entry_set = true;
  return 0;
}

extern "C" int c2r_set_plane_entry_columns(c2r_ctx *c, int plane, const double *cols3) {
  if (int e_ = set_plane_entry_columns_one(c, plane, cols3)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_plane_entry_columns_one(r, plane, cols3); });
}

// the largest face of the list of planes: what the layer buffers, shared by the planes, are made for
static size_t plane_face_max(const c2r_ctx *c) {
  size_t face_max = 0;
  for (int k = 0; k < c->nplane; k++) face_max = std::max(face_max, (size_t)plane_face_cells(c, c->plane[k].src.axis));
  return face_max;
}

// The buffers only a tilted plane with a flux map needs -- two flux layers for the largest face of the list and the flux
// of every cell -- made by whichever of c2r_set_plane_tilt and c2r_set_plane_flux_map completes the pair first.
static int ensure_pflux_buffers(c2r_ctx *c) {
  if (c->d_pflux_cell) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t face_max = plane_face_max(c);
  for (double *&b : c->d_pflux_layer)
    if (!b) HIPCHK(c, hipMalloc(&b, sizeof(double) * 3 * face_max));
  HIPCHK(c, hipMalloc(&c->d_pflux_cell, sizeof(double) * 3 * c->g.ncell));
  return 0;
}

static int set_plane_tilt_one(c2r_ctx *c, int plane, const double *tilt) {
  if (!c) return 1;
  if (plane < 1 || plane > c->nplane) return fail(c, "c2r_set_plane_tilt: plane %d not in [1,%d]", plane, c->nplane);
  if (c->pass_open) return fail(c, "c2r_set_plane_tilt: a pass opened by c2r_pass_sources_begin is still open");
  c2r_ctx::Plane &pn = c->plane[plane - 1];
  const double t[2] = {tilt ? tilt[0] : 0.0, tilt ? tilt[1] : 0.0};
  if (!std::isfinite(t[0]) || !std::isfinite(t[1])) return fail(c, "c2r_set_plane_tilt: plane %d: tilt (%g, %g) is not finite", plane, t[0], t[1]);
  if (plane_tilted(t)) {
    const double dr[3] = {c->sc.dr1, c->sc.dr2, c->sc.dr3};
    const int per[3] = {c->per[0], c->per[1], c->per[2]};
    if (!(dr[0] > 0.0 && dr[1] > 0.0 && dr[2] > 0.0))
      return fail(c, "c2r_set_plane_tilt: the cell sizes are not set yet (c2r_set_step first: the tilt is checked against them)");
    const PlaneTilt T(t, dr, pn.src.axis, per);
    if (!T.valid())
      return fail(c, "c2r_set_plane_tilt: plane %d: tilt (%g, %g) moves the beam %g and %g cells sideways per layer of axis %d; more than 1 "
                  "makes another axis the dominant one (send the plane along that axis instead)", plane, t[0], t[1], T.a_f, T.a_g,
                  pn.src.axis);
    if (!c->d_plane_layer[0]) { // first tilted plane of this list: the two layer buffers, for the largest face of the list
      HIPCHK(c, hipSetDevice(c->device));
      const size_t face_max = plane_face_max(c);
      for (double *&b : c->d_plane_layer) HIPCHK(c, hipMalloc(&b, sizeof(double) * 3 * face_max));
    }
    if (pn.fmap_set && ensure_pflux_buffers(c)) return 1;
  }
  pn.tilt[0] = t[0];
  pn.tilt[1] = t[1];
  return 0;
}

extern "C" int c2r_set_plane_tilt(c2r_ctx *c, int plane, const double tilt[2]) {
  if (int e_ = set_plane_tilt_one(c, plane, tilt)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_plane_tilt_one(r, plane, tilt); });
}

extern "C" int c2r_get_plane_tilt(const c2r_ctx *c, int plane, double tilt[2]) {
  if (!c || !tilt || plane < 1 || plane > c->nplane) return 1;
  tilt[0] = c->plane[plane - 1].tilt[0];
  tilt[1] = c->plane[plane - 1].tilt[1];
  return 0;
}

static int set_plane_flux_map_one(c2r_ctx *c, int plane, const double *flux3) {
  if (!c) return 1;
  if (plane < 1 || plane > c->nplane) return fail(c, "c2r_set_plane_flux_map: plane %d not in [1,%d]", plane, c->nplane);
  if (c->pass_open) return fail(c, "c2r_set_plane_flux_map: a pass opened by c2r_pass_sources_begin is still open");
  c2r_ctx::Plane &pn = c->plane[plane - 1];
  if (!flux3) { // the plane's uniform normflux again
    pn.fmap_set = pn.fmap_uses[0] = pn.fmap_uses[1] = false;
    return 0;
  }
  const size_t face = (size_t)plane_face_cells(c, pn.src.axis);
  bool uses[2] = {false, false};
  for (size_t i = 0; i < 3 * face; i++) {
    if (!(flux3[i] >= 0.0) || !std::isfinite(flux3[i]))
      return fail(c, "c2r_set_plane_flux_map: plane %d: entry %zu of SED %d is %g (a flux is finite and not negative)", plane, i % face,
                  (int)(i / face), flux3[i]);
    if (i >= face && flux3[i] != 0.0) uses[i / face - 1] = true;
  }
  for (int k = 0; k < 2; k++)
    if (uses[k] && !c->have_sed[k])
      return fail(c, "c2r_set_plane_flux_map: plane %d: the map has a flux of SED %d, whose tables have not been set (c2r_set_sed_tables(%d))",
                  plane, k + 1, k + 1);
  HIPCHK(c, hipSetDevice(c->device));
  if (!pn.d_fmap) HIPCHK(c, hipMalloc(&pn.d_fmap, sizeof(double) * 3 * face));
  if (!pn.d_fexit) HIPCHK(c, hipMalloc(&pn.d_fexit, sizeof(double) * 3 * face));
  if (plane_tilted(pn.tilt) && ensure_pflux_buffers(c)) return 1;
  pn.fmap_set = false;
  HIPCHK(c, hipMemcpyAsync(pn.d_fmap, flux3, sizeof(double) * 3 * face, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  pn.fmap_set = true;
  pn.fmap_uses[0] = uses[0];
  pn.fmap_uses[1] = uses[1];
  return 0;
}

extern "C" int c2r_set_plane_flux_map(c2r_ctx *c, int plane, const double *flux3) {
  if (int e_ = set_plane_flux_map_one(c, plane, flux3)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_plane_flux_map_one(r, plane, flux3); });
}

extern "C" int c2r_get_plane_flux_map_set(const c2r_ctx *c, int plane) {
  return c && plane >= 1 && plane <= c->nplane && c->plane[plane - 1].fmap_set ? 1 : 0;
}

// c2r_set_plane_curve on one device: everything is checked before anything is kept; nothing is allocated (the curve travels
// as a kernel argument)
static int set_plane_curve_one(c2r_ctx *c, int plane, const c2r_plane_curve *curve) {
  if (!c) return 1;
  if (plane < 1 || plane > c->nplane) return fail(c, "c2r_set_plane_curve: plane %d not in [1,%d]", plane, c->nplane);
  if (c->pass_open) return fail(c, "c2r_set_plane_curve: a pass opened by c2r_pass_sources_begin is still open");
  c2r_ctx::Plane &pn = c->plane[plane - 1];
  c2r_plane_curve kept = {0, 0, 0.0, {}, {1.0}};
  if (curve) {
    const c2r_plane_curve &v = *curve;
    if (v.nstep < 0 || v.nstep > C2R_PLANE_CURVE_MAX_STEPS)
      return fail(c, "c2r_set_plane_curve: plane %d: nstep = %d not in [0,%d]", plane, v.nstep, C2R_PLANE_CURVE_MAX_STEPS);
    if (v.layer0 < 0) return fail(c, "c2r_set_plane_curve: plane %d: layer0 = %d is negative", plane, v.layer0);
    if (!(v.depth0 >= 0.0) || !std::isfinite(v.depth0)) // (a NaN fails every comparison)
      return fail(c, "c2r_set_plane_curve: plane %d: depth0 = %g is negative or not finite", plane, v.depth0);
    for (int k = 0; k < v.nstep; k++) {
      if (!(v.depth[k] >= 0.0) || !std::isfinite(v.depth[k]))
        return fail(c, "c2r_set_plane_curve: plane %d: depth[%d] = %g is negative or not finite", plane, k, v.depth[k]);
      if (k > 0 && !(v.depth[k] > v.depth[k - 1]))
        return fail(c, "c2r_set_plane_curve: plane %d: depth[%d] = %g is not above depth[%d] = %g", plane, k, v.depth[k], k - 1,
                    v.depth[k - 1]);
    }
    for (int k = 0; k <= v.nstep; k++)
      if (!(v.factor[k] >= 0.0) || !std::isfinite(v.factor[k]))
        return fail(c, "c2r_set_plane_curve: plane %d: factor[%d] = %g is negative or not finite", plane, k, v.factor[k]);
    // an all-zero record is a record nobody filled in, not a plane that has gone dark (that is {1, .., {0.0}, {0.0, 0.0}})
    if (v.nstep == 0 && v.factor[0] == 0.0)
      return fail(c, "c2r_set_plane_curve: plane %d: nstep = 0 and factor[0] = 0 (a zeroed record); no curve is factor[0] = 1", plane);
    kept.nstep = v.nstep;
    kept.layer0 = v.layer0;
    kept.depth0 = v.depth0;
    for (int k = 0; k < v.nstep; k++) kept.depth[k] = v.depth[k];
    for (int k = 0; k <= v.nstep; k++) kept.factor[k] = v.factor[k];
  }
  pn.curve = kept;
  pn.curve_set = !(kept.nstep == 0 && kept.factor[0] == 1.0); // no step and factor 1.0: no curve, the uncurved kernels
  return 0;
}

extern "C" int c2r_set_plane_curve(c2r_ctx *c, int plane, const c2r_plane_curve *curve) {
  if (int e_ = set_plane_curve_one(c, plane, curve)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_plane_curve_one(r, plane, curve); });
}

extern "C" int c2r_get_plane_curve(const c2r_ctx *c, int plane, c2r_plane_curve *out) {
  if (!c || !out) return 1;
  if (plane < 1 || plane > c->nplane) {
    c->err = "c2r_get_plane_curve: plane " + std::to_string(plane) + " not in [1," + std::to_string(c->nplane) + "]";
    return 1;
  }
  *out = c->plane[plane - 1].curve;
  return 0;
}

// the device of the context that ran plane p (0-based) last: the deal gives a plane to one device per pass
static c2r_ctx *plane_owner(c2r_ctx *c, int p) {
  c2r_ctx *best = c;
  for (c2r_ctx *r : c->replicas)
    if (r->plane[p].stamp > best->plane[p].stamp) best = r;
  return best;
}

extern "C" int c2r_download_plane_exit_columns(c2r_ctx *c, int plane, double *cols3) {
  if (!c) return 1;
  if (plane < 1 || plane > c->nplane || !cols3) return fail(c, "c2r_download_plane_exit_columns: plane %d not in [1,%d], or null argument", plane, c->nplane);
  c2r_ctx *d = plane_owner(c, plane - 1);
  const c2r_ctx::Plane &pn = d->plane[plane - 1];
  HIPCHK(c, hipSetDevice(d->device));
  const size_t n3 = 3 * (size_t)plane_face_cells(d, pn.src.axis);
  HIPCHK(c, hipMemcpyAsync(cols3, pn.d_exit, sizeof(double) * n3, hipMemcpyDeviceToHost, d->stream));
  HIPCHK(c, hipStreamSynchronize(d->stream));
  return 0;
}

extern "C" int c2r_download_plane_exit_flux(c2r_ctx *c, int plane, double *flux3) {
  if (!c) return 1;
  if (plane < 1 || plane > c->nplane || !flux3) return fail(c, "c2r_download_plane_exit_flux: plane %d not in [1,%d], or null argument", plane, c->nplane);
  if (c->pass_open) return fail(c, "c2r_download_plane_exit_flux: a pass opened by c2r_pass_sources_begin is still open");
  c2r_ctx *d = plane_owner(c, plane - 1);
  const c2r_ctx::Plane &pn = d->plane[plane - 1];
  if (!pn.fexit_valid)
    return fail(c, "c2r_download_plane_exit_flux: no pass has run plane %d with a flux map yet (c2r_set_plane_flux_map, then a pass)", plane);
  HIPCHK(c, hipSetDevice(d->device));
  const size_t n3 = 3 * (size_t)plane_face_cells(d, pn.src.axis);
  HIPCHK(c, hipMemcpyAsync(flux3, pn.d_fexit, sizeof(double) * n3, hipMemcpyDeviceToHost, d->stream));
  HIPCHK(c, hipStreamSynchronize(d->stream));
  return 0;
}

extern "C" int c2r_get_plane_loss(c2r_ctx *c, int plane, double *loss) {
  if (!c) return 1;
  if (plane < 1 || plane > c->nplane || !loss) return fail(c, "c2r_get_plane_loss: plane %d not in [1,%d], or null argument", plane, c->nplane);
  if (c->pass_open) return fail(c, "c2r_get_plane_loss: a pass opened by c2r_pass_sources_begin is still open");
  *loss = plane_owner(c, plane - 1)->plane[plane - 1].loss;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// side faces of a tilted plane: side entry, side exit, side loss (include/c2ray_hip.h; the rule is c2ray_pside.hpp)

// cells along a line of `side` of a plane along `axis` (L_0 = fb, L_1 = fa, 1 for the corner line) and layers of the plane
static void plane_strip_shape(const c2r_ctx *c, int axis, int side, size_t &line, size_t &na) {
  const PlaneGeom G = plane_geometry(c->g.n1, c->g.n2, c->g.n3, axis, 0);
  line = side == 0 ? (size_t)G.fb : (side == 1 ? (size_t)G.fa : 1);
  na = (size_t)G.na;
}

// c2r_set_plane_side_entry on one device: everything is checked before anything changes
static int set_plane_side_entry_one(c2r_ctx *c, int plane, int side, const double *cols, const double *flux) {
  if (!c) return 1;
  if (plane < 1 || plane > c->nplane) return fail(c, "c2r_set_plane_side_entry: plane %d not in [1,%d]", plane, c->nplane);
  if (side < 0 || side > 2) return fail(c, "c2r_set_plane_side_entry: side %d, expected 0, 1 or 2 (the corner line)", side);
  if (c->pass_open) return fail(c, "c2r_set_plane_side_entry: a pass opened by c2r_pass_sources_begin is still open");
  if (!cols && flux) return fail(c, "c2r_set_plane_side_entry: plane %d, side %d: a flux strip without a column strip", plane, side);
  c2r_ctx::Plane &pn = c->plane[plane - 1];
  size_t line, na;
  plane_strip_shape(c, pn.src.axis, side, line, na);
  const size_t n = na * 3 * line;
  bool uses[2] = {false, false};
  if (flux)
    for (size_t i = 0; i < n; i++) {
      const int sed = (int)((i / line) % 3);
      if (!(flux[i] >= 0.0) || !std::isfinite(flux[i]))
        return fail(c, "c2r_set_plane_side_entry: plane %d, side %d: flux entry %zu of SED %d in slot %zu is %g (a flux is finite and not "
                    "negative)", plane, side, i % line, sed, i / (3 * line), flux[i]);
      if (sed > 0 && flux[i] != 0.0) uses[sed - 1] = true;
    }
  for (int k = 0; k < 2; k++)
    if (uses[k] && !c->have_sed[k])
      return fail(c, "c2r_set_plane_side_entry: plane %d, side %d: the strip has a flux of SED %d, whose tables have not been set "
                  "(c2r_set_sed_tables(%d))", plane, side, k + 1, k + 1);
  if (!cols) { // the side reads 0.0 again
    pn.side_in_set[side] = pn.side_inf_set[side] = pn.side_inf_uses[side][0] = pn.side_inf_uses[side][1] = false;
    return 0;
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (!pn.d_side_in[side]) HIPCHK(c, hipMalloc(&pn.d_side_in[side], sizeof(double) * n));
  if (flux && !pn.d_side_inf[side]) HIPCHK(c, hipMalloc(&pn.d_side_inf[side], sizeof(double) * n));
  pn.side_in_set[side] = pn.side_inf_set[side] = pn.side_inf_uses[side][0] = pn.side_inf_uses[side][1] = false;
  HIPCHK(c, hipMemcpyAsync(pn.d_side_in[side], cols, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  if (flux) HIPCHK(c, hipMemcpyAsync(pn.d_side_inf[side], flux, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  pn.side_in_set[side] = true;
  pn.side_inf_set[side] = flux != nullptr;
  pn.side_inf_uses[side][0] = uses[0];
  pn.side_inf_uses[side][1] = uses[1];
  return 0;
}

extern "C" int c2r_set_plane_side_entry(c2r_ctx *c, int plane, int side, const double *cols, const double *flux) {
  if (int e_ = set_plane_side_entry_one(c, plane, side, cols, flux)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_plane_side_entry_one(r, plane, side, cols, flux); });
}

static int enable_plane_side_exit_one(c2r_ctx *c, int plane, int on) {
  if (!c) return 1;
  if (plane < 1 || plane > c->nplane) return fail(c, "c2r_enable_plane_side_exit: plane %d not in [1,%d]", plane, c->nplane);
  if (c->pass_open) return fail(c, "c2r_enable_plane_side_exit: a pass opened by c2r_pass_sources_begin is still open");
  c2r_ctx::Plane &pn = c->plane[plane - 1];
  HIPCHK(c, hipSetDevice(c->device));
  if (!on) {
    HIPCHK(c, hipStreamSynchronize(c->stream)); // nothing queued may still write them
    for (int s = 0; s < 2; s++) {
      if (pn.d_side_out[s]) (void)hipFree(pn.d_side_out[s]);
      if (pn.d_side_outf[s]) (void)hipFree(pn.d_side_outf[s]);
      pn.d_side_out[s] = pn.d_side_outf[s] = nullptr;
      pn.side_out_live[s] = false;
    }
    pn.side_out_on = pn.side_out_valid = pn.side_out_mapped = false;
    return 0;
  }
  if (pn.side_out_on) return 0;
  for (int s = 0; s < 2; s++) {
    size_t line, na;
    plane_strip_shape(c, pn.src.axis, s, line, na);
    if (!pn.d_side_out[s]) HIPCHK(c, hipMalloc(&pn.d_side_out[s], sizeof(double) * na * 3 * line));
    if (!pn.d_side_outf[s]) HIPCHK(c, hipMalloc(&pn.d_side_outf[s], sizeof(double) * na * 3 * line));
  }
  pn.side_out_on = true;
  pn.side_out_valid = false;
  return 0;
}

extern "C" int c2r_enable_plane_side_exit(c2r_ctx *c, int plane, int on) {
  if (int e_ = enable_plane_side_exit_one(c, plane, on)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return enable_plane_side_exit_one(r, plane, on); });
}

extern "C" int c2r_download_plane_side_exit(c2r_ctx *c, int plane, int side, double *cols, double *flux) {
  if (!c) return 1;
  if (plane < 1 || plane > c->nplane || !cols)
    return fail(c, "c2r_download_plane_side_exit: plane %d not in [1,%d], or null argument", plane, c->nplane);
  if (side < 0 || side > 1) return fail(c, "c2r_download_plane_side_exit: side %d, expected 0 or 1", side);
  if (c->pass_open) return fail(c, "c2r_download_plane_side_exit: a pass opened by c2r_pass_sources_begin is still open");
  c2r_ctx *d = plane_owner(c, plane - 1);
  const c2r_ctx::Plane &pn = d->plane[plane - 1];
  if (!pn.side_out_on || !pn.side_out_valid)
    return fail(c, "c2r_download_plane_side_exit: no pass has run plane %d with the side exit enabled yet (c2r_enable_plane_side_exit, then "
                "a pass)", plane);
  if (!pn.side_out_live[side])
    return fail(c, "c2r_download_plane_side_exit: side %d of plane %d was not live in the last pass that ran it (its tilt component is "
                "zero or its axis periodic)", side, plane);
  if (flux && !pn.side_out_mapped)
    return fail(c, "c2r_download_plane_side_exit: plane %d ran without a flux map: it has no flux strips (pass flux = NULL)", plane);
  size_t line, na;
  plane_strip_shape(d, pn.src.axis, side, line, na);
  HIPCHK(c, hipSetDevice(d->device));
  HIPCHK(c, hipMemcpyAsync(cols, pn.d_side_out[side], sizeof(double) * na * 3 * line, hipMemcpyDeviceToHost, d->stream));
  if (flux) HIPCHK(c, hipMemcpyAsync(flux, pn.d_side_outf[side], sizeof(double) * na * 3 * line, hipMemcpyDeviceToHost, d->stream));
  HIPCHK(c, hipStreamSynchronize(d->stream));
  return 0;
}

// the buffers of the side loss of one device (c2r_enable_plane_side_loss, c2r_destroy)
static void free_side_loss(c2r_ctx *c) {
  if (c->d_side_partial) (void)hipFree(c->d_side_partial);
  if (c->d_side_loss) (void)hipFree(c->d_side_loss);
  if (c->h_side_loss) (void)hipHostFree(c->h_side_loss);
  c->d_side_partial = c->d_side_loss = c->h_side_loss = nullptr;
}

static int enable_plane_side_loss_one(c2r_ctx *c, int on) {
  if (!c) return 1;
  if (c->pass_open) return fail(c, "c2r_enable_plane_side_loss: a pass opened by c2r_pass_sources_begin is still open (close it with c2r_pass_sources_end first)");
  HIPCHK(c, hipSetDevice(c->device));
  if (!on) {
    if (c->side_loss_on) HIPCHK(c, hipStreamSynchronize(c->stream));
    free_side_loss(c);
    c->side_loss_on = false;
    return 0;
  }
  if (c->side_loss_on) return 0;
  const int n[3] = {c->g.n1, c->g.n2, c->g.n3};
  int most = 0;
  for (int d = 0; d < 3; d++) most = std::max(most, face_cells(n, d));
  HIPCHK(c, hipMalloc(&c->d_side_partial, sizeof(double) * (size_t)((most + BLOCK - 1) / BLOCK)));
  HIPCHK(c, hipMalloc(&c->d_side_loss, sizeof(double) * 2 * PLANE_MAX));
  HIPCHK(c, hipHostMalloc(&c->h_side_loss, sizeof(double) * 2 * PLANE_MAX));
  for (c2r_ctx::Plane &pn : c->plane) pn.side_loss[0] = pn.side_loss[1] = 0.0;
  c->side_loss_on = true;
  return 0;
}

extern "C" int c2r_enable_plane_side_loss(c2r_ctx *c, int on) {
  if (int e_ = enable_plane_side_loss_one(c, on)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return enable_plane_side_loss_one(r, on); });
}

extern "C" int c2r_get_plane_side_loss_enabled(const c2r_ctx *c) { return c && c->side_loss_on ? 1 : 0; }

extern "C" int c2r_get_plane_side_loss(c2r_ctx *c, int plane, double out2[2]) {
  if (!c) return 1;
  if (!c->side_loss_on) return fail(c, "c2r_get_plane_side_loss: the side loss is off (c2r_enable_plane_side_loss)");
  if (plane < 1 || plane > c->nplane || !out2) return fail(c, "c2r_get_plane_side_loss: plane %d not in [1,%d], or null argument", plane, c->nplane);
  if (c->pass_open) return fail(c, "c2r_get_plane_side_loss: a pass opened by c2r_pass_sources_begin is still open");
  const c2r_ctx::Plane &pn = plane_owner(c, plane - 1)->plane[plane - 1];
  out2[0] = pn.side_loss[0];
  out2[1] = pn.side_loss[1];
  return 0;
}
