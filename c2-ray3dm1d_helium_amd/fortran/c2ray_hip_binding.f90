!> iso_c_binding view of include/c2ray_hip.h -- the only place where the Fortran host meets C.
!! Every interface below binds one entry point of the C ABI; argument order and meaning are those
!! of the header.  Arrays are passed by address (assumed-size dummies), scalars by value.
module c2ray_hip

  use, intrinsic :: iso_c_binding

  implicit none

  public

  !> c2r_timing of include/c2ray_hip.h
  type, bind(C) :: c2r_timing
     real(c_double) :: sweep_ms, rates_ms, chem_ms
     integer(c_int) :: sweep_launches, rates_launches, chem_launches
     integer(c_long_long) :: cells_swept
  end type c2r_timing

  !> c2r_source_trace of include/c2ray_hip.h: what the last pass that swept a source did for it
  type, bind(C) :: c2r_source_trace
     integer(c_int) :: reach_l(3), reach_r(3)
     integer(c_int) :: nbox
     integer(c_int) :: box_lo(3), box_hi(3)
     integer(c_int) :: block_shells
     integer(c_long_long) :: block_cells
     integer(c_long_long) :: swept_cells
     integer(c_long_long) :: sweep_threads
  end type c2r_source_trace

  !> c2r_iteration_report of include/c2ray_hip.h: what evolve3D's loop reports about one outer iteration
  type, bind(C) :: c2r_iteration_report
     integer(c_int) :: conv_flag
     integer(c_int) :: sum_nbox
     real(c_double) :: photon_loss(47)
     real(c_double) :: means_intermed(5)
     real(c_double) :: sums_intermed(5)
     real(c_double) :: total_rates(3)
     real(c_double) :: minima_av(2)
     real(c_double) :: reccoef(12)
  end type c2r_iteration_report

  !> c2r_comm_selftest_report of include/c2ray_hip.h: what the self-test of the sum over ranks found
  type, bind(C) :: c2r_comm_selftest_report
     integer(c_int) :: ranks, kind, devices
     integer(c_long_long) :: elements(2)
     integer(c_long_long) :: mismatches(2)
     integer(c_int) :: bad_route, bad_rank
     integer(c_long_long) :: bad_index
     real(c_double) :: got, expected
     real(c_double) :: ms(2)
  end type c2r_comm_selftest_report

  !> c2r_comm_timing of include/c2ray_hip.h: the sum over ranks of the last fused iteration on one device
  type, bind(C) :: c2r_comm_timing
     integer(c_int) :: slabs
     real(c_double) :: allreduce_ms, allreduce_exposed_ms, tail_ms
  end type c2r_comm_timing

  !> c2r_plane_source of include/c2ray_hip.h: a plane wave entering through an open mesh face (axis is 0-based)
  type, bind(C) :: c2r_plane_source
     integer(c_int) :: axis, from_high
     real(c_double) :: normflux(3)
  end type c2r_plane_source

  !> c2r_source_beam of include/c2ray_hip.h: the emission cone (kind 1) or bicone (kind 2) of one point source; kind 0: none
  type, bind(C) :: c2r_source_beam
     integer(c_int) :: kind
     real(c_double) :: axis(3)
     real(c_double) :: cos_half
  end type c2r_source_beam

  !> c2r_source_curve of include/c2ray_hip.h: the light curve of one point source -- nstep ascending radii (physical lengths in
  !> the unit of dr) and the flux factor of each of the nstep + 1 distance shells; nstep = 0 and factor(1) = 1: no curve
  integer(c_int), parameter :: C2R_CURVE_MAX_STEPS = 8
  type, bind(C) :: c2r_source_curve
     integer(c_int) :: nstep
     real(c_double) :: radius(C2R_CURVE_MAX_STEPS)
     real(c_double) :: factor(C2R_CURVE_MAX_STEPS + 1)
  end type c2r_source_curve

  !> c2r_plane_curve of include/c2ray_hip.h: the light curve of one plane -- nstep ascending depths along its beam (lengths in
  !> the unit of dr) and the flux factor of each of the nstep + 1 depth shells; layer0 layers and the length depth0 lie in
  !> front of the mesh; nstep = 0 and factor(1) = 1: no curve
  integer(c_int), parameter :: C2R_PLANE_CURVE_MAX_STEPS = 8
  type, bind(C) :: c2r_plane_curve
     integer(c_int) :: nstep
     integer(c_int) :: layer0
     real(c_double) :: depth0
     real(c_double) :: depth(C2R_PLANE_CURVE_MAX_STEPS)
     real(c_double) :: factor(C2R_PLANE_CURVE_MAX_STEPS + 1)
  end type c2r_plane_curve

  !> c2r_sed_setup of include/c2ray_hip.h: what spec_integration starts from for one SED
  type, bind(C) :: c2r_sed_setup
     integer(c_int) :: nfreq, sed
     type(c_ptr) :: freq_min, delta_freq, xsec_index, tau, romw
     real(c_double) :: R_star2, h_over_kT, two_pi_over_c_square, hplanck, pi
     real(c_double) :: ion_freq_HI, ion_freq_HeI, ion_freq_HeII
     real(c_double) :: pl_scaling, pl_index
  end type c2r_sed_setup

  interface

     integer(c_int) function c2r_create(ctx, device, mesh) bind(C, name="c2r_create")
       import :: c_int, c_ptr
       type(c_ptr), intent(out) :: ctx
       integer(c_int), value :: device
       integer(c_int), intent(in) :: mesh(3)
     end function c2r_create

     subroutine c2r_destroy(ctx) bind(C, name="c2r_destroy")
       import :: c_ptr
       type(c_ptr), value :: ctx
     end subroutine c2r_destroy

     type(c_ptr) function c2r_last_error(ctx) bind(C, name="c2r_last_error")
       import :: c_ptr
       type(c_ptr), value :: ctx
     end function c2r_last_error

     type(c_ptr) function c2r_create_error() bind(C, name="c2r_create_error")
       import :: c_ptr
     end function c2r_create_error

     integer(c_int) function c2r_set_tables(ctx, photo_thick, photo_thin, heat_thick, heat_thin, &
          sigma_HI, sigma_HeI, sigma_HeII, fvec, bb_upper) bind(C, name="c2r_set_tables")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       type(c_ptr), value :: photo_thick, photo_thin ! c_loc of the tables, or c_null_ptr (c2r_build_tables)
       type(c_ptr), value :: heat_thick, heat_thin   ! c_loc of the tables, or c_null_ptr
       real(c_double), intent(in) :: sigma_HI(*), sigma_HeI(*), sigma_HeII(*)
       type(c_ptr), intent(in) :: fvec(12)           ! c_loc of the twelve f vectors
       integer(c_int), value :: bb_upper
     end function c2r_set_tables

     integer(c_int) function c2r_set_cooling(ctx, cool, mintemp, dtemp) bind(C, name="c2r_set_cooling")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: cool(*)
       real(c_double), value :: mintemp, dtemp
     end function c2r_set_cooling

     integer(c_int) function c2r_set_step(ctx, ndens, dr, vol, clumping, zred, H0, Omega0, &
          isothermal, temper_val, reccoef) bind(C, name="c2r_set_step")
       import :: c_int, c_ptr, c_double, c_float
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: ndens(*), dr(3)
       real(c_double), value :: vol
       real(c_float), value :: clumping
       real(c_double), value :: zred, H0, Omega0
       integer(c_int), value :: isothermal
       real(c_double), value :: temper_val
       real(c_double), intent(in) :: reccoef(12)
     end function c2r_set_step

     integer(c_int) function c2r_set_step_scalars(ctx, dr, vol, clumping, zred, H0, Omega0, &
          isothermal, temper_val, reccoef) bind(C, name="c2r_set_step_scalars")
       import :: c_int, c_ptr, c_double, c_float
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: dr(3)
       real(c_double), value :: vol
       real(c_float), value :: clumping
       real(c_double), value :: zred, H0, Omega0
       integer(c_int), value :: isothermal
       real(c_double), value :: temper_val
       real(c_double), intent(in) :: reccoef(12)
     end function c2r_set_step_scalars

     integer(c_int) function c2r_arena_stats(ctx, out) bind(C, name="c2r_arena_stats")
       import :: c_int, c_ptr, c_long_long
       type(c_ptr), value :: ctx
       integer(c_long_long), intent(out) :: out(6)
     end function c2r_arena_stats

     integer(c_int) function c2r_scale_ndens(ctx, divisor) bind(C, name="c2r_scale_ndens")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), value :: divisor
     end function c2r_scale_ndens

     integer(c_int) function c2r_set_sources(ctx, nsrc, srcpos, normflux, s_star) &
          bind(C, name="c2r_set_sources")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nsrc
       integer(c_int), intent(in) :: srcpos(*)
       real(c_double), intent(in) :: normflux(*)
       real(c_double), value :: s_star
     end function c2r_set_sources

     !> c2r_set_sources for a list in which a source may stand outside the mesh along open axes
     integer(c_int) function c2r_set_sources_external(ctx, nsrc, srcpos, normflux, s_star) &
          bind(C, name="c2r_set_sources_external")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nsrc
       integer(c_int), intent(in) :: srcpos(*)
       real(c_double), intent(in) :: normflux(*)
       real(c_double), value :: s_star
     end function c2r_set_sources_external

     !> point-source hand-over between meshes stacked along an open axis; face = 2 * axis + high.
     !> Keep the exit strips through `face` of the sources sources(1:nsel) (1-based); nsel = 0 frees them
     integer(c_int) function c2r_select_source_face_exit(ctx, face, nsel, sources) &
          bind(C, name="c2r_select_source_face_exit")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: face, nsel
       integer(c_int), intent(in) :: sources(*)
     end function c2r_select_source_face_exit

     !> the strip of source ns (3 x face cells, species slowest), nbox of the pass that filled it, and whether its
     !> final box held a cell of the face's layer
     integer(c_int) function c2r_download_source_face_exit(ctx, face, ns, cols3, rounds, reached) &
          bind(C, name="c2r_download_source_face_exit")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: face, ns
       real(c_double), intent(out) :: cols3(*)
       integer(c_int), intent(out) :: rounds, reached
     end function c2r_download_source_face_exit

     !> entry columns of source ns, which stands beyond `face` only: cols3 = c_loc of the upstream strip, or
     !> c_null_ptr to clear the entry; the source is traced for exactly `rounds` rounds
     integer(c_int) function c2r_set_source_face_entry(ctx, ns, face, cols3, rounds) &
          bind(C, name="c2r_set_source_face_entry")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx, cols3
       integer(c_int), value :: ns, face, rounds
     end function c2r_set_source_face_entry

     !> face = -1 while source ns has no entry
     integer(c_int) function c2r_get_source_face_entry(ctx, ns, face, rounds) &
          bind(C, name="c2r_get_source_face_entry")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: ns
       integer(c_int), intent(out) :: face, rounds
     end function c2r_get_source_face_entry

     !> the halo of source ns, which stands beyond one, two or three faces: c_loc of a c2r_source_halo, or c_null_ptr
     !> to clear it
     integer(c_int) function c2r_set_source_halo(ctx, ns, halo) bind(C, name="c2r_set_source_halo")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx, halo
       integer(c_int), value :: ns
     end function c2r_set_source_halo

     !> faces(d) = 2 (d - 1) + high, or -1 where source ns has no strip along axis d
     integer(c_int) function c2r_get_source_halo(ctx, ns, faces, rounds) bind(C, name="c2r_get_source_halo")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: ns
       integer(c_int), intent(out) :: faces(3), rounds
     end function c2r_get_source_halo

     !> this mesh's index + origin = the deep mesh's index, per axis: cinterp then forms its crossing points from
     !> the deep mesh's coordinates (non-zero along open axes only)
     integer(c_int) function c2r_set_mesh_origin(ctx, origin) bind(C, name="c2r_set_mesh_origin")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), intent(in) :: origin(3)
     end function c2r_set_mesh_origin

     integer(c_int) function c2r_get_mesh_origin(ctx, origin) bind(C, name="c2r_get_mesh_origin")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), intent(out) :: origin(3)
     end function c2r_get_mesh_origin

     integer(c_int) function c2r_set_sed_tables(ctx, sed, photo_thick, photo_thin, heat_thick, heat_thin, &
          lower, upper) bind(C, name="c2r_set_sed_tables")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: sed
       type(c_ptr), value :: photo_thick, photo_thin ! c_loc of the tables, or c_null_ptr (c2r_build_tables)
       type(c_ptr), value :: heat_thick, heat_thin
       integer(c_int), value :: lower, upper
     end function c2r_set_sed_tables

     integer(c_int) function c2r_set_sources_sed(ctx, sed, normflux, s_star) bind(C, name="c2r_set_sources_sed")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: sed
       real(c_double), intent(in) :: normflux(*)
       real(c_double), value :: s_star
     end function c2r_set_sources_sed

     !> beams: c_loc of NumSrc records of type(c2r_source_beam), or c_null_ptr: no source is beamed
     integer(c_int) function c2r_set_source_beams(ctx, nsrc, beams) bind(C, name="c2r_set_source_beams")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: nsrc
       type(c_ptr), value :: beams
     end function c2r_set_source_beams

     !> the beam of source ns (1-based) as it was set
     integer(c_int) function c2r_get_source_beam(ctx, ns, beam) bind(C, name="c2r_get_source_beam")
       import :: c_int, c_ptr, c2r_source_beam
       type(c_ptr), value :: ctx
       integer(c_int), value :: ns
       type(c2r_source_beam), intent(out) :: beam
     end function c2r_get_source_beam

     !> photon horizons: radius(NumSrc), a maximum ray length per source in the length unit of dr (ieee +infinity: none), or
     !> c_null_ptr: no source has a horizon
     integer(c_int) function c2r_set_source_horizons(ctx, nsrc, radius) bind(C, name="c2r_set_source_horizons")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: nsrc
       type(c_ptr), value :: radius
     end function c2r_set_source_horizons

     !> the horizon of source ns (1-based) as it was set; +infinity while it has none
     integer(c_int) function c2r_get_source_horizon(ctx, ns, radius) bind(C, name="c2r_get_source_horizon")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: ns
       real(c_double), intent(out) :: radius
     end function c2r_get_source_horizon

     !> light curves: c_loc of NumSrc records of type(c2r_source_curve), or c_null_ptr: no source has a curve
     integer(c_int) function c2r_set_source_curves(ctx, nsrc, curves) bind(C, name="c2r_set_source_curves")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: nsrc
       type(c_ptr), value :: curves
     end function c2r_set_source_curves

     !> the curve of source ns (1-based) as it was set; nstep = 0 and factor(1) = 1 while it has none
     integer(c_int) function c2r_get_source_curve(ctx, ns, curve) bind(C, name="c2r_get_source_curve")
       import :: c_int, c_ptr, c2r_source_curve
       type(c_ptr), value :: ctx
       integer(c_int), value :: ns
       type(c2r_source_curve), intent(out) :: curve
     end function c2r_get_source_curve

     integer(c_int) function c2r_build_tables(ctx, setup, with_heat) bind(C, name="c2r_build_tables")
       import :: c_int, c_ptr, c2r_sed_setup
       type(c_ptr), value :: ctx
       type(c2r_sed_setup), intent(in) :: setup
       integer(c_int), value :: with_heat
     end function c2r_build_tables

     integer(c_int) function c2r_download_tables(ctx, sed, photo_thick, photo_thin, heat_thick, heat_thin) &
          bind(C, name="c2r_download_tables")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: sed
       type(c_ptr), value :: photo_thick, photo_thin, heat_thick, heat_thin  ! (0:NumTau, ncol) or c_null_ptr
     end function c2r_download_tables

     integer(c_int) function c2r_set_lls(ctx, use_lls, coldensh_lls, lls_grid) bind(C, name="c2r_set_lls")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: use_lls
       real(c_double), value :: coldensh_lls
       type(c_ptr), value :: lls_grid            ! real(c_float) (mesh) or c_null_ptr
     end function c2r_set_lls

     integer(c_int) function c2r_set_clumping_grid(ctx, clumping_grid) bind(C, name="c2r_set_clumping_grid")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       type(c_ptr), value :: clumping_grid       ! real(c_float) (mesh) or c_null_ptr
     end function c2r_set_clumping_grid

     integer(c_int) function c2r_upload_state(ctx, xh, xhe, temperature) bind(C, name="c2r_upload_state")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: xh(*), xhe(*)
       type(c_ptr), value :: temperature            ! c_loc(temperature_grid) or c_null_ptr
     end function c2r_upload_state

     integer(c_int) function c2r_download_state(ctx, xh, xhe, temperature) bind(C, name="c2r_download_state")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: xh(*), xhe(*)
       type(c_ptr), value :: temperature
     end function c2r_download_state

     integer(c_int) function c2r_evolve3d(ctx, dt, niter, conv_flags, cap) bind(C, name="c2r_evolve3d")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), value :: dt
       integer(c_int), intent(out) :: niter
       integer(c_int), intent(out) :: conv_flags(*)
       integer(c_int), value :: cap
     end function c2r_evolve3d

     integer(c_int) function c2r_begin_step(ctx) bind(C, name="c2r_begin_step")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_begin_step

     integer(c_int) function c2r_set_rates_to_zero(ctx) bind(C, name="c2r_set_rates_to_zero")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_set_rates_to_zero

     integer(c_int) function c2r_pass_sources(ctx, first, stride) bind(C, name="c2r_pass_sources")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: first, stride
     end function c2r_pass_sources

     integer(c_int) function c2r_pass_sources_begin(ctx, first, stride, nslab) bind(C, name="c2r_pass_sources_begin")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: first, stride, nslab
     end function c2r_pass_sources_begin

     integer(c_int) function c2r_pass_slab_count(ctx) bind(C, name="c2r_pass_slab_count")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_pass_slab_count

     integer(c_int) function c2r_pass_wait_slab(ctx, slab, first_cell, ncells) bind(C, name="c2r_pass_wait_slab")
       import :: c_int, c_ptr, c_size_t
       type(c_ptr), value :: ctx
       integer(c_int), value :: slab
       integer(c_size_t), intent(out) :: first_cell, ncells
     end function c2r_pass_wait_slab

     integer(c_int) function c2r_pass_sources_end(ctx) bind(C, name="c2r_pass_sources_end")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_pass_sources_end

     integer(c_int) function c2r_do_source(ctx, ns) bind(C, name="c2r_do_source")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: ns
     end function c2r_do_source

     integer(c_int) function c2r_global_pass_cells(ctx, dt, first_cell, ncells, after_event) &
          bind(C, name="c2r_global_pass_cells")
       import :: c_int, c_ptr, c_double, c_size_t
       type(c_ptr), value :: ctx
       real(c_double), value :: dt
       integer(c_size_t), value :: first_cell, ncells
       type(c_ptr), value :: after_event          ! hipEvent_t or c_null_ptr
     end function c2r_global_pass_cells

     integer(c_int) function c2r_global_pass_finish(ctx, conv_flag) bind(C, name="c2r_global_pass_finish")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), intent(out) :: conv_flag
     end function c2r_global_pass_finish

     integer(c_int) function c2r_global_pass(ctx, dt, conv_flag) bind(C, name="c2r_global_pass")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), value :: dt
       integer(c_int), intent(out) :: conv_flag
     end function c2r_global_pass

     integer(c_int) function c2r_end_step(ctx) bind(C, name="c2r_end_step")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_end_step

     integer(c_int) function c2r_download_rates(ctx, phih, phihe, phiheat, photon_loss, sum_nbox) &
          bind(C, name="c2r_download_rates")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: phih(*), phihe(*), phiheat(*), photon_loss(*)
       integer(c_int), intent(out) :: sum_nbox
     end function c2r_download_rates

     integer(c_int) function c2r_download_rates_sel(ctx, which, phih, phihe, phiheat, photon_loss, sum_nbox) &
          bind(C, name="c2r_download_rates_sel")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: which
       real(c_double), intent(out) :: phih(*), phihe(*), phiheat(*), photon_loss(*)
       integer(c_int), intent(out) :: sum_nbox
     end function c2r_download_rates_sel

     integer(c_int) function c2r_get_loss(ctx, photon_loss, sum_nbox) bind(C, name="c2r_get_loss")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: photon_loss(*)
       integer(c_int), intent(out) :: sum_nbox
     end function c2r_get_loss

     integer(c_int) function c2r_download_iter_state(ctx, xh_av, xhe_av, xh_intermed, xhe_intermed) &
          bind(C, name="c2r_download_iter_state")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: xh_av(*), xhe_av(*), xh_intermed(*), xhe_intermed(*)
     end function c2r_download_iter_state

     integer(c_int) function c2r_upload_rates(ctx, phih, phihe, phiheat) bind(C, name="c2r_upload_rates")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: phih(*), phihe(*), phiheat(*)
     end function c2r_upload_rates

     integer(c_int) function c2r_upload_iter_state(ctx, xh_av, xhe_av, xh_intermed, xhe_intermed) &
          bind(C, name="c2r_upload_iter_state")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: xh_av(*), xhe_av(*), xh_intermed(*), xhe_intermed(*)
     end function c2r_upload_iter_state

     integer(c_int) function c2r_download_columns(ctx, coldensh_out, coldenshe_out) &
          bind(C, name="c2r_download_columns")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: coldensh_out(*), coldenshe_out(*)
     end function c2r_download_columns

     integer(c_int) function c2r_state_sums(ctx, which, out5) bind(C, name="c2r_state_sums")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: which
       real(c_double), intent(out) :: out5(5)
     end function c2r_state_sums

     integer(c_int) function c2r_fraction_means(ctx, which, out5) bind(C, name="c2r_fraction_means")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: which
       real(c_double), intent(out) :: out5(5)
     end function c2r_fraction_means

     integer(c_int) function c2r_evolve0d_global(ctx, dt, pos, conv_flag) bind(C, name="c2r_evolve0d_global")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), value :: dt
       integer(c_int), intent(in) :: pos(3)
       integer(c_int), intent(inout) :: conv_flag
     end function c2r_evolve0d_global

     integer(c_int) function c2r_fraction_minima(ctx, which, out2) bind(C, name="c2r_fraction_minima")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: which
       real(c_double), intent(out) :: out2(2)
     end function c2r_fraction_minima

     integer(c_int) function c2r_get_constants(out, capacity) bind(C, name="c2r_get_constants")
       import :: c_int, c_double
       real(c_double), intent(out) :: out(*)
       integer(c_int), value :: capacity
     end function c2r_get_constants

     ! ---- several GPUs: sources over ranks and the sum over ranks (RCCL inside the library) ----
     integer(c_int) function c2r_device_count() bind(C, name="c2r_device_count")
       import :: c_int
     end function c2r_device_count

     integer(c_int) function c2r_create_multi(ctx, ndev, devices, mesh) bind(C, name="c2r_create_multi")
       import :: c_int, c_ptr
       type(c_ptr), intent(out) :: ctx
       integer(c_int), value :: ndev
       integer(c_int), intent(in) :: devices(*)
       integer(c_int), intent(in) :: mesh(3)
     end function c2r_create_multi

     integer(c_int) function c2r_num_devices(ctx) bind(C, name="c2r_num_devices")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_num_devices

     integer(c_int) function c2r_comm_unique_id(id) bind(C, name="c2r_comm_unique_id")
       import :: c_int, c_char
       character(kind=c_char), intent(out) :: id(128)
     end function c2r_comm_unique_id

     integer(c_int) function c2r_comm_init(ctx, first_rank, nranks, id) bind(C, name="c2r_comm_init")
       import :: c_int, c_ptr, c_char
       type(c_ptr), value :: ctx
       integer(c_int), value :: first_rank, nranks
       character(kind=c_char), intent(in) :: id(128)
     end function c2r_comm_init

     integer(c_int) function c2r_comm_init_local(ctx) bind(C, name="c2r_comm_init_local")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_comm_init_local

     integer(c_int) function c2r_comm_destroy(ctx) bind(C, name="c2r_comm_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_comm_destroy

     integer(c_int) function c2r_comm_nranks(ctx) bind(C, name="c2r_comm_nranks")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_comm_nranks

     integer(c_int) function c2r_comm_available() bind(C, name="c2r_comm_available")
       import :: c_int
     end function c2r_comm_available

     integer(c_int) function c2r_comm_rank(ctx) bind(C, name="c2r_comm_rank")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_comm_rank

     integer(c_int) function c2r_comm_kind(ctx) bind(C, name="c2r_comm_kind")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_comm_kind

     integer(c_int) function c2r_comm_library(out, capacity) bind(C, name="c2r_comm_library")
       import :: c_int, c_char
       character(kind=c_char), dimension(*) :: out
       integer(c_int), value :: capacity
     end function c2r_comm_library

     integer(c_int) function c2r_allreduce_rates(ctx) bind(C, name="c2r_allreduce_rates")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_allreduce_rates

     integer(c_int) function c2r_pass_allreduce_chemistry(ctx, first, stride, nslab, dt, conv_flag) &
          bind(C, name="c2r_pass_allreduce_chemistry")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: first, stride, nslab
       real(c_double), value :: dt
       integer(c_int), intent(out) :: conv_flag
     end function c2r_pass_allreduce_chemistry

     integer(c_int) function c2r_evolve0d(ctx, rtpos, ns, niter, on_surface, loss) bind(C, name="c2r_evolve0d")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), intent(in) :: rtpos(3)
       integer(c_int), value :: ns, niter, on_surface
       real(c_double), intent(out) :: loss
     end function c2r_evolve0d

     integer(c_int) function c2r_iteration(ctx, first, stride, nslab, dt, report) bind(C, name="c2r_iteration")
       import :: c_int, c_ptr, c_double, c2r_iteration_report
       type(c_ptr), value :: ctx
       integer(c_int), value :: first, stride, nslab
       real(c_double), value :: dt
       type(c2r_iteration_report), intent(out) :: report
     end function c2r_iteration

     integer(c_int) function c2r_total_rates(ctx, dt, reccoef, out3) bind(C, name="c2r_total_rates")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), value :: dt
       real(c_double), intent(in) :: reccoef(12)
       real(c_double), intent(out) :: out3(3)
     end function c2r_total_rates

     integer(c_int) function c2r_get_reccoef(ctx, out12) bind(C, name="c2r_get_reccoef")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: out12(12)
     end function c2r_get_reccoef

     integer(c_size_t) function c2r_rates_count(ctx) bind(C, name="c2r_rates_count")
       import :: c_size_t, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_rates_count

     type(c_ptr) function c2r_rates_device_ptr(ctx) bind(C, name="c2r_rates_device_ptr")
       import :: c_ptr
       type(c_ptr), value :: ctx
     end function c2r_rates_device_ptr

     integer(c_int) function c2r_set_rates_buffer(ctx, device_ptr, count) bind(C, name="c2r_set_rates_buffer")
       import :: c_int, c_ptr, c_size_t
       type(c_ptr), value :: ctx, device_ptr
       integer(c_size_t), value :: count
     end function c2r_set_rates_buffer

     integer(c_int) function c2r_synchronize(ctx) bind(C, name="c2r_synchronize")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_synchronize

     integer(c_int) function c2r_set_batch(ctx, nbatch) bind(C, name="c2r_set_batch")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: nbatch
     end function c2r_set_batch

     !> mesh boundaries of the ray trace: periodic /= 0 (default) or 0, open (include/c2ray_hip.h)
     integer(c_int) function c2r_set_boundaries(ctx, periodic) bind(C, name="c2r_set_boundaries")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: periodic
     end function c2r_set_boundaries

     integer(c_int) function c2r_get_boundaries(ctx) bind(C, name="c2r_get_boundaries")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_get_boundaries

     !> per axis: periodic(d) /= 0, axis d wraps; 0, it is open (include/c2ray_hip.h)
     integer(c_int) function c2r_set_boundaries_axes(ctx, periodic) bind(C, name="c2r_set_boundaries_axes")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), intent(in) :: periodic(3)
     end function c2r_set_boundaries_axes

     integer(c_int) function c2r_get_boundaries_axes(ctx, periodic) bind(C, name="c2r_get_boundaries_axes")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), intent(out) :: periodic(3)
     end function c2r_get_boundaries_axes

     !> plane-parallel sources (include/c2ray_hip.h): plane p is "source NumSrc + p" of every deal; nplane = 0 removes them
     integer(c_int) function c2r_set_plane_sources(ctx, nplane, planes) bind(C, name="c2r_set_plane_sources")
       import :: c_int, c_ptr, c2r_plane_source
       type(c_ptr), value :: ctx
       integer(c_int), value :: nplane
       type(c2r_plane_source), intent(in) :: planes(*)
     end function c2r_set_plane_sources

     integer(c_int) function c2r_get_plane_count(ctx) bind(C, name="c2r_get_plane_count")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_get_plane_count

     !> cols3: (face cells, 3) -- HI, HeI, HeII; a c_null_ptr sets the entry columns to zero again
     integer(c_int) function c2r_set_plane_entry_columns(ctx, plane, cols3) bind(C, name="c2r_set_plane_entry_columns")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx, cols3
       integer(c_int), value :: plane
     end function c2r_set_plane_entry_columns

     integer(c_int) function c2r_download_plane_exit_columns(ctx, plane, cols3) bind(C, name="c2r_download_plane_exit_columns")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: plane
       real(c_double), intent(out) :: cols3(*)
     end function c2r_download_plane_exit_columns

     integer(c_int) function c2r_get_plane_loss(ctx, plane, loss) bind(C, name="c2r_get_plane_loss")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: plane
       real(c_double), intent(out) :: loss
     end function c2r_get_plane_loss

     !> oblique incidence of plane `plane`: tilt = the tangents towards the two face axes (the lower axis first);
     !> (0, 0) is normal incidence, as after c2r_set_plane_sources
     integer(c_int) function c2r_set_plane_tilt(ctx, plane, tilt) bind(C, name="c2r_set_plane_tilt")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: plane
       real(c_double), intent(in) :: tilt(2)
     end function c2r_set_plane_tilt

     integer(c_int) function c2r_get_plane_tilt(ctx, plane, tilt) bind(C, name="c2r_get_plane_tilt")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: plane
       real(c_double), intent(out) :: tilt(2)
     end function c2r_get_plane_tilt

     !> flux map of plane `plane`: 3 x face doubles, SED slowest, the face cells in the order of the entry columns; it
     !> replaces the plane's normflux while set; a c_null_ptr removes it
     integer(c_int) function c2r_set_plane_flux_map(ctx, plane, flux3) bind(C, name="c2r_set_plane_flux_map")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx, flux3
       integer(c_int), value :: plane
     end function c2r_set_plane_flux_map

     integer(c_int) function c2r_get_plane_flux_map_set(ctx, plane) bind(C, name="c2r_get_plane_flux_map_set")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: plane
     end function c2r_get_plane_flux_map_set

     !> the flux the cells of the last layer saw in the last pass that ran the plane with a map: the next slab's flux map
     integer(c_int) function c2r_download_plane_exit_flux(ctx, plane, flux3) bind(C, name="c2r_download_plane_exit_flux")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: plane
       real(c_double), intent(out) :: flux3(*)
     end function c2r_download_plane_exit_flux

     !> plane light curves: c_loc of one type(c2r_plane_curve), or c_null_ptr: the plane has no curve
     integer(c_int) function c2r_set_plane_curve(ctx, plane, curve) bind(C, name="c2r_set_plane_curve")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: plane
       type(c_ptr), value :: curve
     end function c2r_set_plane_curve

     !> side faces of a tilted plane (include/c2ray_hip.h): side entry -- the ghost strips a neighbouring mesh hands in;
     !> side = 0, 1, or 2 for the corner line; cols / flux: c_loc of na x 3 x L doubles, or c_null_ptr
     integer(c_int) function c2r_set_plane_side_entry(ctx, plane, side, cols, flux) bind(C, name="c2r_set_plane_side_entry")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: plane, side
       type(c_ptr), value :: cols, flux
     end function c2r_set_plane_side_entry

     integer(c_int) function c2r_enable_plane_side_exit(ctx, plane, on) bind(C, name="c2r_enable_plane_side_exit")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: plane, on
     end function c2r_enable_plane_side_exit

     !> cols / flux: c_loc of na x 3 x L doubles; flux = c_null_ptr for a plane without a map
     integer(c_int) function c2r_download_plane_side_exit(ctx, plane, side, cols, flux) bind(C, name="c2r_download_plane_side_exit")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: plane, side
       type(c_ptr), value :: cols, flux
     end function c2r_download_plane_side_exit

     !> side loss: what a tilted plane loses through its open side faces; off by default
     integer(c_int) function c2r_enable_plane_side_loss(ctx, on) bind(C, name="c2r_enable_plane_side_loss")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: on
     end function c2r_enable_plane_side_loss

     integer(c_int) function c2r_get_plane_side_loss_enabled(ctx) bind(C, name="c2r_get_plane_side_loss_enabled")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_get_plane_side_loss_enabled

     integer(c_int) function c2r_get_plane_side_loss(ctx, plane, out2) bind(C, name="c2r_get_plane_side_loss")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: plane
       real(c_double), intent(out) :: out2(2)
     end function c2r_get_plane_side_loss

     !> the curve of plane `plane` (1-based) as it was set; nstep = 0 and factor(1) = 1 while it has none
     integer(c_int) function c2r_get_plane_curve(ctx, plane, curve) bind(C, name="c2r_get_plane_curve")
       import :: c_int, c_ptr, c2r_plane_curve
       type(c_ptr), value :: ctx
       integer(c_int), value :: plane
       type(c2r_plane_curve), intent(out) :: curve
     end function c2r_get_plane_curve

     !> escape maps (include/c2ray_hip.h): the kept photon loss per cell of the open mesh face it leaves through;
     !> face = 2*axis + high, axis 0-based, high = 0 the face at index 1
     integer(c_int) function c2r_enable_face_loss(ctx, on) bind(C, name="c2r_enable_face_loss")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: on
     end function c2r_enable_face_loss

     integer(c_int) function c2r_get_face_loss_enabled(ctx) bind(C, name="c2r_get_face_loss_enabled")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_get_face_loss_enabled

     !> map: the face's cells in mesh order of the two remaining axes, the lower axis fastest
     integer(c_int) function c2r_download_face_loss(ctx, face, map) bind(C, name="c2r_download_face_loss")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: face
       real(c_double), intent(out) :: map(*)
     end function c2r_download_face_loss

     integer(c_int) function c2r_get_face_loss(ctx, out6) bind(C, name="c2r_get_face_loss")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: out6(6)
     end function c2r_get_face_loss

     !> horizon loss (include/c2ray_hip.h): what crosses each source's photon horizon, per source; off by default
     integer(c_int) function c2r_enable_horizon_loss(ctx, on) bind(C, name="c2r_enable_horizon_loss")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: on
     end function c2r_enable_horizon_loss

     integer(c_int) function c2r_get_horizon_loss_enabled(ctx) bind(C, name="c2r_get_horizon_loss_enabled")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2r_get_horizon_loss_enabled

     !> per_source(nsrc), nsrc = NumSrc; total: their sum in source order
     integer(c_int) function c2r_get_horizon_loss(ctx, nsrc, per_source, total) bind(C, name="c2r_get_horizon_loss")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       integer(c_int), value :: nsrc
       real(c_double), intent(out) :: per_source(*)
       real(c_double), intent(out) :: total
     end function c2r_get_horizon_loss

     !> diagnostic: the T = 2*(E1*E2 + E0*E2 + E0*E1) terms of the horizoned source swept last, its number and extents
     integer(c_int) function c2r_download_horizon_rim(ctx, ns, extent, terms, capacity) bind(C, name="c2r_download_horizon_rim")
       import :: c_int, c_ptr, c_double, c_long_long
       type(c_ptr), value :: ctx
       integer(c_int), intent(out) :: ns
       integer(c_int), intent(out) :: extent(3)
       real(c_double), intent(out) :: terms(*)
       integer(c_long_long), value :: capacity
     end function c2r_download_horizon_rim

     integer(c_int) function c2r_enable_timing(ctx, on) bind(C, name="c2r_enable_timing")
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
       integer(c_int), value :: on
     end function c2r_enable_timing

     integer(c_int) function c2r_get_timing_device(ctx, idev, tm) bind(C, name="c2r_get_timing_device")
       import :: c_int, c_ptr, c2r_timing
       type(c_ptr), value :: ctx
       integer(c_int), value :: idev
       type(c2r_timing), intent(out) :: tm
     end function c2r_get_timing_device

     !> ns is 1-based; host bookkeeping only, no device copy
     integer(c_int) function c2r_get_source_trace(ctx, ns, trace) bind(C, name="c2r_get_source_trace")
       import :: c_int, c_ptr, c2r_source_trace
       type(c_ptr), value :: ctx
       integer(c_int), value :: ns
       type(c2r_source_trace), intent(out) :: trace
     end function c2r_get_source_trace

     integer(c_int) function c2r_get_timing(ctx, tm) bind(C, name="c2r_get_timing")
       import :: c_int, c_ptr, c2r_timing
       type(c_ptr), value :: ctx
       type(c2r_timing), intent(out) :: tm
     end function c2r_get_timing

     !> collective: every rank of the communicator calls it (see the header for what a pass proves)
     integer(c_int) function c2r_comm_selftest(ctx, nslab, report) bind(C, name="c2r_comm_selftest")
       import :: c_int, c_ptr, c2r_comm_selftest_report
       type(c_ptr), value :: ctx
       integer(c_int), value :: nslab
       type(c2r_comm_selftest_report), intent(out) :: report
     end function c2r_comm_selftest

     integer(c_int) function c2r_get_comm_timing(ctx, idev, tm) bind(C, name="c2r_get_comm_timing")
       import :: c_int, c_ptr, c2r_comm_timing
       type(c_ptr), value :: ctx
       integer(c_int), value :: idev
       type(c2r_comm_timing), intent(out) :: tm
     end function c2r_get_comm_timing

  end interface

contains

  !> Text of the last error of a context (or of a failed c2r_create when ctx is null)
  function c2r_error_text(ctx) result(text)
    type(c_ptr), intent(in) :: ctx
    character(len=:), allocatable :: text
    type(c_ptr) :: p
    character(kind=c_char), pointer :: s(:)
    integer :: n

    if (c_associated(ctx)) then
       p = c2r_last_error(ctx)
    else
       p = c2r_create_error()
    endif
    text = ""
    if (.not. c_associated(p)) return
    call c_f_pointer(p, s, (/ 512 /))
    n = 0
    do while (n < 512)
       if (s(n+1) == c_null_char) exit
       n = n + 1
    enddo
    allocate(character(len=n) :: text)
    if (n > 0) text = transfer(s(1:n), text)
  end function c2r_error_text

end module c2ray_hip
