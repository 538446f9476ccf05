// Plane-parallel sources behind the C ABI (included by c2ray_hip.hip where the pass needs run_planes): the kernels, the
// queueing of a pass's planes, the plane buffers and the c2r_*plane* entry points.
//
// c2r_set_plane_sources; the per-cell rule is c2ray_plane.hpp, DESIGN.md section 3.1: a plane wave enters through an open
// face and travels along one axis, every line of cells a 1-D problem of its own.  Three stages per plane and pass, all on
// the sweep stream, one kernel each:
//   the march   k_plane_columns   one lane per line of cells, or for a tilted plane (c2r_set_plane_tilt)
//               k_plane_layer     one launch per layer; <true> carries the flux of a map along (c2r_set_plane_flux_map)
//   the rates   k_plane_rates     no dependencies, one lane per cell; the flux uniform, by face cell or by cell (PlaneFlux)
//   the loss    k_plane_exit      what leaves through the far face; the flux of a map or uniform (MAPPED), the per-line
//                                 term also kept in the escape map of that face (KEEP, c2r_enable_face_loss)
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
    const bool uses[2] = {mapped ? pn.fmap_uses[0] : pd.nf[1] != 0.0, mapped ? pn.fmap_uses[1] : pd.nf[2] != 0.0};
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
    if (tilted) { // one launch per layer, in travel order; with a map the flux is carried along, the last layer's is the exit flux
      const dim3 lgrid((unsigned)((G.fa + PLANE_LAYER_BX - 1) / PLANE_LAYER_BX), (unsigned)((G.fb + PLANE_LAYER_BY - 1) / PLANE_LAYER_BY));
      const double *prev = entry, *fprev = mapped ? pn.d_fmap : nullptr;
      for (int m = 0; m < G.na; m++) {
        const bool last = m == G.na - 1;
        double *next = last ? pn.d_exit : c->d_plane_layer[m & 1];
        double *fnext = mapped ? (last ? pn.d_fexit : c->d_pflux_layer[m & 1]) : nullptr;
        with_flag(mapped, [&](auto flux) {
          hipLaunchKernelGGL(k_plane_layer<decltype(flux)::value>, lgrid, dim3(PLANE_LAYER_BX, PLANE_LAYER_BY), 0, c->stream, G, T, P.sc, m,
                             g.ncell, c->d_ndens, c->d_xh_av, c->d_xhe_av, lls, prev, c->d_plane_cin, next, fprev,
                             mapped ? c->d_pflux_cell : nullptr, fnext);
        });
        prev = next;
        fprev = fnext;
      }
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
    for (double *b : {pn.d_entry, pn.d_exit, pn.d_fmap, pn.d_fexit})
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
