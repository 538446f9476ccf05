// The body of k_rates, of k_rates_beam and of k_rates_curve (c2ray_hip.hip), included into each kernel after `constexpr bool
// BEAM, CURVE`: what the second kernel adds is compiled under `if constexpr (BEAM)`, what the third adds to the second under
// `if constexpr (CURVE)`, and k_rates stays the kernel it was before beams existed, k_rates_beam the one it was before curves
// did (register figures: profiles/source_beams_resources.json, profiles/source_curves_resources.json).  Not a function: a
// body that reaches the kernel through a call, even an inlined one, costs the isothermal kernel two vector registers.
  const size_t nc = g.ncell;
  // One block = a tile of 8 x 8 x 4 cells, one wave = a 4 x 4 x 4 cube of it.  Neighbouring cells see
  // similar optical depths: the lanes of a cube mostly take the same branch of the bit-exact log (its
  // near-1 path is 10 % of all arguments, so a wave of 64 unrelated cells nearly always runs both) and
  // gather from few table lines -- 31.2 -> 26.9 ms per launch at 256^3 x 8 sources against 64
  // consecutive i.  With sub-boxes much smaller than the mesh a cube also keeps ~(w/(w+3))^3 of its lanes
  // busy for a box of width w instead of w/(w+63).  Loads are 16 segments of 32 B; the kernel is ALU-bound.
  // `tiles`, when given, lists the tiles that intersect a sub-box of the batch (built on the host): the
  // launch then holds only blocks with work, which keeps enough heavy waves resident per SIMD.  With it come
  // `tile_ptr` / `tile_src`: for each listed tile the sources (positions in `src`, ascending = source order)
  // whose sub-box reaches into it, so that a batch of hundreds of faint sources costs a cell only the sources
  // near it.  Without lists every cell walks all nsrc sources of the batch (few sources, boxes that fill the mesh).
  // k_rates, isothermal, one SED (ISO1; its beam and curve twins stay the kernels they were): the exponent terms of
  // log10's tail are read from a table (gm::Log10Exp, 17 KB) that each block fills here with the multiplications the table
  // replaces -- per band six FP64-rate instructions less and two integer ones more -- and the four registers that the two
  // pairs need come from the cell's denominators, which wait in LDS (below)
  constexpr bool ISO1 = !HEAT && !MULTI && !BEAM;
  // ... and, with all axes periodic (FOLD), its log table holds the reciprocal with the power of two folded in as well
  // (gm::LogFold: the same pitch, no kshift) and its split hands down the exponent table's byte offset (gm::LogFoldExp).
  // By the same type it takes the near-1 test of a logarithm from the table entry (gm::LogFold::lim) and fetches a band's two
  // rows of the pair copy by index-scaled buffer loads (load_rows with a band offset, c2ray_device.hpp).
  // The open-boundary twin stays the kernel it was: the same route brings it from 92 to 94 registers, with or without the
  // select's constants pinned, past the budget of 93 (tests/test_rates_registers.py).
  constexpr bool FOLD = ISO1 && !OPEN;
  // the (invc, logc) table of the bit-exact log in LDS, with the log's power of two folded in (gm::LogEntry, 8 KB): two
  // gathers per band iteration that no longer queue behind the photo-table gathers in the vector memory path
  using LogTab = std::conditional_t<FOLD, gm::LogFold, gm::LogEntry>;
  __shared__ LogTab s_logtab[256];
  if constexpr (FOLD) s_logtab[threadIdx.x] = gm::make_log_fold((int)threadIdx.x);
  else s_logtab[threadIdx.x] = gm::make_log_entry((int)threadIdx.x);
  // (what every other kernel hands down)
  [[maybe_unused]] const gm::LogEntry *const logtab4 = [&]() -> const gm::LogEntry * {
    if constexpr (FOLD) return nullptr;
    else return &s_logtab[0];
  }();
  constexpr bool EXPT = ISO1;
  // ... and k_rates with one SED and all axes periodic reads the shell volume of a cell.source from a table (below)
  constexpr bool SHELLTAB = !MULTI && !BEAM && !OPEN;
  __shared__ gm::Log10Exp s_exptab[EXPT ? gm::LOG10_NEXP : 1];
  if constexpr (EXPT) {
    for (int e = (int)threadIdx.x; e < gm::LOG10_NEXP; e += BLOCK) s_exptab[e] = gm::make_log10_exp(gm::LOG10_KY_LO + e);
  }
  __syncthreads();
  // the two exponent fields of the split's select, in vector registers for the whole kernel (gm::FoldPins)
  [[maybe_unused]] gm::FoldPins fold_ = {0u, 0u};
  if constexpr (FOLD) fold_ = gm::pin_fold_constants();
  [[maybe_unused]] const auto logx = [&]() {
    if constexpr (FOLD) return gm::LogFoldExp{&s_logtab[0], &s_exptab[EXPT ? -gm::LOG10_KY_LO : 0], &fold_};
    else if constexpr (EXPT) return gm::LogEntryExp{&s_logtab[0], &s_exptab[0]};
    else return 0;
  }();
  // the band data as uploaded (a BandDataByRow: the plain arrays and, behind them, the same numbers band by band); a kernel
  // chooses its reading of them by the TYPE it hands down -- the base for the array form (an upcast, not a reinterpretation)
  const BandData *const bd = bdr;
  // two polynomial constants of the log held in vector registers for the whole kernel (gm::LogPins): -0.25 ms per
  // launch in the isothermal kernel; the heating kernels, which have no registers to spare, lose 2.7 ms with them
  gm::LogPins pins_ = {0.0, 0.0};
  const gm::LogPins *pins = nullptr;
  if (!HEAT) {
    pins_ = gm::pin_log_constants();
    pins = &pins_;
  }
  const int ti = (g.n1 + 7) >> 3, tj = (g.n2 + 7) >> 3;
  // Workgroups are dealt to the 8 XCDs round-robin, and each XCD has its own L2.  A cube reads its columns as 32-byte
  // rows of shell faces, so the other half of every cache line belongs to the neighbouring cube: give each XCD a
  // contiguous run of C = 128 tiles (a slab of the mesh), so that the neighbour's request finds the line in the same L2.
  int vb = (int)blockIdx.x;
  {
    constexpr int C = 128;
    const int full = (int)(gridDim.x / (8 * C)) * (8 * C);
    if (vb < full) {
      const int r = vb >> 3, xcd = vb & 7;
      vb = (r / C) * (8 * C) + xcd * C + (r % C);
    }
  }
  const int tile = tiles ? tiles[tile_base + vb] : tile_base + vb;
  const int bi = tile % ti, bj = (tile / ti) % tj, bk = tile / (ti * tj);
  const int lane = threadIdx.x & 63;
  const int w_ = threadIdx.x >> 6;
  const int i = bi * 8 + (w_ & 1) * 4 + (lane & 3), j = bj * 8 + (w_ >> 1) * 4 + ((lane >> 2) & 3), k = bk * 4 + (lane >> 4);
  if (i >= g.n1 || j >= g.n2 || k >= g.n3) return;
  // The cell's own quantities are needed once per source, after its band loops: only what those divisions use stays
  // in registers across the loops -- the three denominators h0 * nd * (1 - abu_he), ... (evaluated from the left, as
  // evolve_point.F90:288-296 does per source), not the four factors, and not the cell number, which is formed again
  // for the stores at the end.
  double den_HI, den_HeI, den_HeII, h1;
  double a_HI = 0.0, a_HeI = 0.0, a_HeII = 0.0, a_heat = 0.0;
  {
    const size_t q = (size_t)i + (size_t)g.n1 * ((size_t)j + (size_t)g.n2 * (size_t)k);
    const double nd = ndens[q];
    const double h0 = dmax(xh_av[q], epsilon);
    h1 = dmax(xh_av[q + nc], epsilon);
    const double he0 = dmax(xhe_av[q], epsilon), he1 = dmax(xhe_av[q + nc], epsilon);
    den_HI = h0 * nd * (1.0 - abu_he);
    den_HeI = he0 * nd * abu_he;
    den_HeII = he1 * nd * abu_he;
    // fresh: the first launch after set_rates_to_zero when the launch covers every cell -- the grids then need not
    // be zeroed first (4 x 8 bytes per cell written and read again: 1.3 ms per iteration at 256^3); 0 + x == x
    if (!fresh) {
      a_HI = rates[q];
      a_HeI = rates[q + nc];
      a_HeII = rates[q + 2 * nc];
      if (HEAT) a_heat = rates[q + 3 * nc];
    }
  }
  // secondary-ionisation parameters of this cell, i_state = h_av(1) (evolve_point.F90:255): once per cell,
  // not once per source
  Ricotti ric = {};
  if (HEAT) ric = ricotti_parameters(h1);
  // The three-SED heating kernel parks the cell's denominators and running sums, which the band loops do not touch, in
  // LDS, one column per lane, where the register allocation would otherwise spill them to scratch memory: it then fits
  // four waves per SIMD without a private segment.  (Parking the secondary-ionisation parameters as well costs more
  // than their registers: six LDS reads per heating band, 369 against 357 ms per pass on one box.)
  constexpr bool PARK = HEAT && MULTI;
  // the three denominators of the cell and its four running sums, touched once per source: [den_HI, den_HeI, den_HeII,
  // a_HI, a_HeI, a_HeII, a_heat] x BLOCK (each lane reads back only what it wrote itself: no barrier)
  // The isothermal one-SED k_rates parks its three denominators the same way (PARK_DEN): 93 -> 88 registers, which the
  // exponent table's two pairs bring to 92.  Its running sums stay in registers: parked as well they free nothing more (88
  // either way), and their 6 KB would not fit beside the tables.
  constexpr bool PARK_DEN = ISO1;
  __shared__ double s_den[PARK ? 7 * BLOCK : (PARK_DEN ? 3 * BLOCK : 1)];
  // five blocks of this kernel per compute unit (160 KB of LDS): at most 32 KB each
  static_assert(!ISO1 || sizeof(s_logtab) + sizeof(s_exptab) + sizeof(s_den) <= 32768, "k_rates: LDS for five blocks per compute unit");
  // k_rates_curve: and the flux factor of the cell for the source in hand, one per lane (likewise read back only by the lane
  // that wrote it)
  [[maybe_unused]] __shared__ double s_flux[PARK && CURVE ? BLOCK : 1];
  if (PARK) {
    s_den[threadIdx.x] = den_HI;
    s_den[BLOCK + threadIdx.x] = den_HeI;
    s_den[2 * BLOCK + threadIdx.x] = den_HeII;
    s_den[3 * BLOCK + threadIdx.x] = a_HI;
    s_den[4 * BLOCK + threadIdx.x] = a_HeI;
    s_den[5 * BLOCK + threadIdx.x] = a_HeII;
    s_den[6 * BLOCK + threadIdx.x] = a_heat;
  }
  if constexpr (PARK_DEN) {
    s_den[threadIdx.x] = den_HI;
    s_den[BLOCK + threadIdx.x] = den_HeI;
    s_den[2 * BLOCK + threadIdx.x] = den_HeII;
  }
  bool touched = false;
  const int slot = tile_base + vb;
  const int e0 = tile_ptr ? tile_ptr[slot] : 0, e1 = tile_ptr ? tile_ptr[slot + 1] : nsrc;
  for (int e = e0; e < e1; e++) {
    const SrcDev &S = src[tile_ptr ? tile_src[e] : e];
    // unwrapped offset rtpos - srcpos in [-mesh/2, mesh - mesh/2 - 1]
    int di = i + 1 - S.i0, dj = j + 1 - S.j0, dk = k + 1 - S.k0;
    if constexpr (!OPEN) {
      di = wrap0(di + g.l1, g.n1) - g.l1;
      dj = wrap0(dj + g.l2, g.n2) - g.l2;
      dk = wrap0(dk + g.l3, g.n3) - g.l3;
    } else { // per axis: wrapped where the axis is periodic (S.wn is uniform over the block), as it is where it is open
      di = axis_offset(i, S.i0, S.wn[0]);
      dj = axis_offset(j, S.j0, S.wn[1]);
      dk = axis_offset(k, S.k0, S.wn[2]);
    }
    // Cells outside the source's last sub-box were never traced (evolve_source.F90:136-144): no
    // contribution.  (The reference's own marker is coldensh_out == 0, evolve_point.F90:120; every cell
    // of the box is traced exactly once, so "inside the box" is the same set and needs no zeroing.)
    const bool outside = di < S.lo[0] || di > S.hi[0] || dj < S.lo[1] || dj > S.hi[1] || dk < S.lo[2] || dk > S.hi[2];
    C2R_COUNT_LANES(3, !outside);
    if (outside) continue;
    // A source with a beam or a horizon (S.cut: uniform over the block, a source with neither takes the path it always took):
    // the predicate (both, with d2 formed once: cut_lit, c2ray_horizon.hpp) joins the in-box test, before any column is loaded, and nothing of it outlives this statement -- an unlit
    // cell is a cell the source does not reach.  One thing remains to do for it: where the rates launch leaves the terms
    // of the kept loss behind (S.loss_lo >= 0), an unlit cell of the counted surface leaves its term, 0.0, in the N_in(HI)
    // slot that k_loss_stored will read.
    // A source with a curve (k_rates_curve; S.cut & CUT_CURVE, uniform): cut_flux asks the same and also finds cf, the factor
    // of the cell's shell, a value per lane that lives until the source's fluxes are formed below; a shell of factor 0 is unlit.
    [[maybe_unused]] double cf = 1.0;
    if constexpr (BEAM) { // (k_rates_beam and k_rates_curve only)
      bool unlit;
      if constexpr (CURVE)
        unlit = S.cut != CUT_NONE && !((S.cut & CUT_CURVE) ? cut_flux(S.cut, S.bax, S.bay, S.baz, S.bK, S.hR2, S.cR2, S.cfac, sc.dr1, sc.dr2, sc.dr3, di, dj, dk, cf)
                                                           : cut_lit(S.cut, S.bax, S.bay, S.baz, S.bK, S.hR2, sc.dr1, sc.dr2, sc.dr3, di, dj, dk));
      else
        unlit = S.cut != CUT_NONE && !cut_lit(S.cut, S.bax, S.bay, S.baz, S.bK, S.hR2, sc.dr1, sc.dr2, sc.dr3, di, dj, dk);
      if (unlit) {
        if (!HEAT && S.loss_lo >= 0) {
          const int ia = di < 0 ? -di : di, ja = dj < 0 ? -dj : dj, ka = dk < 0 ? -dk : dk;
          const int shell = ia > ja ? (ia > ka ? ia : ka) : (ja > ka ? ja : ka);
          if ((di == S.lo[0] || dj == S.lo[1] || dk == S.lo[2] || di == S.hi[0] || dj == S.hi[1] || dk == S.hi[2]) && shell >= S.loss_lo) {
            const size_t p = OPEN ? reach_position(S.rl, S.rr, di, dj, dk) : shell_position(di, dj, dk);
            ((global_double *)S.cols)[col_in(p, 0, S.cz)] = 0.0;
          }
        }
        continue;
      }
    }
    touched = true;
    const size_t cz = S.cz;
    const size_t p = OPEN ? reach_position(S.rl, S.rr, di, dj, dk) : shell_position(di, dj, dk);
    global_double *cs = (global_double *)S.cols;
    const double cout_HI = cs[col_out(p, 0, cz)];
    const double cin_HI = cs[col_in(p, 0, cz)], cin_HeI = cs[col_in(p, 1, cz)], cin_HeII = cs[col_in(p, 2, cz)];
    const double cout_HeI = cs[col_out(p, 1, cz)], cout_HeII = cs[col_out(p, 2, cz)];
    // The shell volume and its reciprocal.  SHELLTAB (k_rates, one SED, all axes periodic): read from the table per offset
    // (rt.shellvol, k_shell_volumes: these expressions and make_recip's, once per time step) -- one 16-byte load for a
    // division, a square root and a reciprocal per cell and source; rt.big, uniform, stands for Recip::ok_big of every entry.
    // The open and mixed-boundary kernels, whose offsets span the whole mesh, the beam and curve kernels and the three-SED
    // ones compute as they did.
    double vol_ph;
    [[maybe_unused]] Recip rvol_;
    const Recip *rvol = nullptr;
    if constexpr (SHELLTAB) {
      const int ia = di < 0 ? -di : di, ja = dj < 0 ? -dj : dj, ka = dk < 0 ? -dk : dk;
      const ShellVol v = rt.shellvol[shell_vol_index(ia, ja, ka, rt.e1, rt.e2)];
      vol_ph = v.vol;
      rvol_.b = v.vol;
      rvol_.y = v.rvol;
      rvol_.ok = rvol_.ok_big = rt.big != 0;
      rvol = &rvol_;
    } else if (di == 0 && dj == 0 && dk == 0) {
      vol_ph = sc.cellvol;
    } else {
      const double path = sc_path(di, dj, dk) * sc.dr1;
      const double xs = sc.dr1 * (double)di, ys = sc.dr2 * (double)dj, zs = sc.dr3 * (double)dk;
      const double dist2 = xs * xs + ys * ys + zs * zs;
      vol_ph = 4.0 * pi * dist2 * path;
    }
    // photoion_rates and the sums of this cell; with_loss: also return photo_out, which the kernel otherwise never
    // forms (one addition per band, registers that stay alive through the band loop, scalar registers short
    // enough already: 4 % of the launch when every wave pays it) -- two copies of the code, chosen per wave below
    // per_lane (k_rates_curve, a curved source): the fluxes are the source's times cf, one rounded product per SED held in
    // vector registers; otherwise they are the scalar registers they always were
    auto rates_of_flux = [&](auto with_loss, auto per_lane) -> double {
      constexpr bool LANE = CURVE && decltype(per_lane)::value;
      auto flux = [&](const double nflux) -> double {
        if constexpr (LANE) return nflux * cf;
        else return nflux;
      };
      double photo_out = 0.0;
      if (cin_HI < max_coldensh) {
        PhotoOut o;
        if (MULTI) {
          const double nf[NSED] = {flux(S.nflux), flux(S.nflux_sed[0]), flux(S.nflux_sed[1])};
          if constexpr (HEAT && LANE) {
            // The parked kernel has no six vector registers for three fluxes per lane: cf waits in LDS, and each flux is
            // formed where it is used -- the same rounded product every time (volatile: read there, not hoisted).
            struct LaneFlux {
              const SrcDev &S;
              volatile __attribute__((address_space(3))) double *cf;
              __device__ double operator[](int k) const { return (k == 0 ? S.nflux : (k == 1 ? S.nflux_sed[0] : S.nflux_sed[1])) * *cf; }
            };
            volatile __attribute__((address_space(3))) double *const pf = (volatile __attribute__((address_space(3))) double *)&s_flux[threadIdx.x];
            *pf = cf;
            photoion_rates_multi<HEAT>(*bdr, ss, cin_HI, cout_HI, cin_HeI, cout_HeI, cin_HeII, cout_HeII,
                                       vol_ph, LaneFlux{S, pf}, ric, o, logtab4, pins);
          } else if constexpr (HEAT) // this kernel reads cross sections and factors band by band (BandDataByRow)
            photoion_rates_multi<HEAT>(*bdr, ss, cin_HI, cout_HI, cin_HeI, cout_HeI, cin_HeII, cout_HeII,
                                       vol_ph, nf, ric, o, logtab4, pins);
          else
            photoion_rates_multi<HEAT>(*bd, ss, cin_HI, cout_HI, cin_HeI, cout_HeI, cin_HeII, cout_HeII, vol_ph, nf, ric, o, logtab4, pins);
        } else {
          // gathers first (band_positions_gathers_first) where the registers allow it: the isothermal kernel
          // (... which then read the table's pair copy, rt.pairs, in the table's place: band_positions_gathers_first)
          const double *const thick = !HEAT ? (const double *)rt.pairs : ss.photo_thick[0];
          if constexpr (EXPT)
            photoion_rates<HEAT, std::conditional_t<FOLD, gm::LogFoldExp, gm::LogEntryExp>, BandData, !HEAT>(*bd, thick, ss.photo_thin[0], ss.heat_thick[0], ss.heat_thin[0], cin_HI, cout_HI,
                                                                      cin_HeI, cout_HeI, cin_HeII, cout_HeII, vol_ph, flux(S.nflux), ric, o, &logx, pins, rvol);
          else
            photoion_rates<HEAT, gm::LogEntry, BandData, !HEAT>(*bd, thick, ss.photo_thin[0], ss.heat_thick[0], ss.heat_thin[0], cin_HI, cout_HI,
                                                                     cin_HeI, cout_HeI, cin_HeII, cout_HeII, vol_ph, flux(S.nflux), ric, o, logtab4, pins, rvol);
        }
        if (PARK) { // (volatile: read here, not hoisted back into registers)
          volatile __attribute__((address_space(3))) double *dn = (volatile __attribute__((address_space(3))) double *)&s_den[threadIdx.x];
          dn[3 * BLOCK] = dn[3 * BLOCK] + o.photo_HI / dn[0];
          dn[4 * BLOCK] = dn[4 * BLOCK] + o.photo_HeI / dn[BLOCK];
          dn[5 * BLOCK] = dn[5 * BLOCK] + o.photo_HeII / dn[2 * BLOCK];
          dn[6 * BLOCK] = dn[6 * BLOCK] + o.heat;
        } else if constexpr (PARK_DEN) { // (likewise)
          volatile __attribute__((address_space(3))) double *dn = (volatile __attribute__((address_space(3))) double *)&s_den[threadIdx.x];
          a_HI = a_HI + o.photo_HI / dn[0];
          a_HeI = a_HeI + o.photo_HeI / dn[BLOCK];
          a_HeII = a_HeII + o.photo_HeII / dn[2 * BLOCK];
        } else {
          a_HI = a_HI + o.photo_HI / den_HI;
          a_HeI = a_HeI + o.photo_HeI / den_HeI;
          a_HeII = a_HeII + o.photo_HeII / den_HeII;
          if (HEAT) a_heat = a_heat + o.heat;
        }
        if (decltype(with_loss)::value) photo_out = o.photo_out;
      } else {
        // rates are zero: x + 0.0 == x
      }
      return photo_out;
    };
    // (a uniform branch: a source without a curve in a curved batch takes k_rates_beam's code)
    auto rates_of_source = [&](auto with_loss) -> double {
      // (The three-SED heating kernel has no room for two copies of its band loops -- with both it needs a private segment,
      // 16 to 32 bytes -- so there every source of a curved batch takes the per-lane copy, an uncurved one with cf = 1.0:
      // x*1.0 == x, the same bits.)
      if constexpr (CURVE && HEAT && MULTI) return rates_of_flux(with_loss, std::true_type{});
      if constexpr (CURVE) {
        if (S.cut & CUT_CURVE) return rates_of_flux(with_loss, std::true_type{});
      }
      return rates_of_flux(with_loss, std::false_type{});
    };
    // evolve_point.F90:310-315: a cell on the surface of the (final) sub-box loses photo_out * vol / vol_ph photons
    // through it.  For a source whose last round ended for geometric reasons (SrcDev::loss_lo >= 0) that loss is
    // the one that is kept: leave it in the cell's N_in(HI) slot, which nobody reads any more, for k_loss_stored.
    // Only the shells of the final round count; the others were done -- and counted, for a loss that is not kept
    // -- in earlier rounds.
    // (Isothermal kernels only: the heating kernels, three times the code and short of registers as they are, lose
    // 10 % of their launch to the second copy -- 34.0 against 31.2 ms -- where the isothermal one gains; heating runs
    // evaluate the kept loss with k_loss beside the rates launch, as rounds 1 and 2 did.)
    bool surface = false;
    if (!HEAT && S.loss_lo >= 0) { // uniform
      const int ia = di < 0 ? -di : di, ja = dj < 0 ? -dj : dj, ka = dk < 0 ? -dk : dk;
      const int shell = ia > ja ? (ia > ka ? ia : ka) : (ja > ka ? ja : ka);
      surface = (di == S.lo[0] || dj == S.lo[1] || dk == S.lo[2] || di == S.hi[0] || dj == S.hi[1] || dk == S.hi[2]) &&
                shell >= S.loss_lo;
    }
    if (!HEAT && __any(surface ? 1 : 0)) {
      const double photo_out = rates_of_source(std::true_type{});
      if (surface) cs[col_in(p, 0, cz)] = photo_out * sc.vol / vol_ph;
    } else {
      (void)rates_of_source(std::false_type{});
    }
  }
  if (touched || fresh) {
    const size_t q = (size_t)i + (size_t)g.n1 * ((size_t)j + (size_t)g.n2 * (size_t)k);
    if (PARK) {
      a_HI = s_den[3 * BLOCK + threadIdx.x];
      a_HeI = s_den[4 * BLOCK + threadIdx.x];
      a_HeII = s_den[5 * BLOCK + threadIdx.x];
      a_heat = s_den[6 * BLOCK + threadIdx.x];
    }
    rates[q] = a_HI;
    rates[q + nc] = a_HeI;
    rates[q + 2 * nc] = a_HeII;
    if (HEAT) rates[q + 3 * nc] = a_heat;
  }
