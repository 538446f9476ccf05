/* C ABI of the MI355X (gfx950) implementation of C2-Ray's evolve3D hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  Each entry
 * point names the reference interface it replaces (paths relative to the reference's
 * code/ directory).  Host arrays are caller-owned contiguous Fortran arrays, i fastest,
 * components slowest: xh(N1,N2,N3,0:1), xhe(N1,N2,N3,0:2), temperature_grid(N1,N2,N3,0:2) real(4).
 * The library owns device memory only.  All calls return 0 on success; on failure they return a
 * non-zero status and c2r_last_error() describes it (the reference has no error convention: its
 * Fortran shim logs the text to unit logf and stops).
 *
 * Threading: one host thread per context; one context per GPU (one rank per GPU).
 */
#ifndef C2RAY_HIP_H
#define C2RAY_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct c2r_ctx c2r_ctx;

#define C2R_NFREQ 47  /* radiation_sizes.f90:22 NumFreqBnd */
#define C2R_NHEAT 113 /* radiation_sizes.f90:23 NumheatBin */
#define C2R_NTAU 2000 /* radiation_sizes.f90:18 NumTau */
#define C2R_NCOOL 801 /* cooling_h.f90:25 temppoints */

/* evolve_ini (files_for_3D/evolve_data.F90:74-97): allocate the work arrays, here on `device`.
 * mesh = sizes.f90:31. */
int c2r_create(c2r_ctx **out, int device, const int mesh[3]);
void c2r_destroy(c2r_ctx *ctx);
const char *c2r_last_error(const c2r_ctx *ctx);
/* error text of a failed c2r_create (no context exists yet) */
const char *c2r_create_error(void);

/* What rad_ini leaves behind (radiation_tables.f90:141-168, radiation_sizes.f90:62-688):
 * bb_photo_thick/thin_table(0:NumTau,1:NumFreqBnd), bb_heat_thick/thin_table(0:NumTau,1:NumheatBin)
 * (tau index fastest; heat tables may be NULL for isothermal-only use), sigma_HI/HeI/HeII(1:47),
 * the twelve secondary-ionisation vectors f1ion_HI .. f2heat_HeII, each (2:47) = 46 doubles, in the
 * order f1ion_{HI,HeI,HeII}, f2ion_{..}, f1heat_{..}, f2heat_{..} (may be NULL with the heat tables),
 * and bb_FreqBnd_UpperLimit (radiation_tables.f90:193-199). */
/* photo_thick/photo_thin and heat_thick/heat_thin may be NULL: the call then only sets the band vectors and
 * c2r_build_tables makes the tables on the device. */
int c2r_set_tables(c2r_ctx *ctx, const double *photo_thick, const double *photo_thin,
                   const double *heat_thick, const double *heat_thin, const double *sigma_HI,
                   const double *sigma_HeI, const double *sigma_HeII, const double *const fvec[12],
                   int bb_upper);

/* What setup_cool leaves behind (cooling_h.f90:76-171): five linear cooling curves of 801 points
 * (H0, H1, He0, He1, He2), log10 T of the first row and the step. */
int c2r_set_cooling(c2r_ctx *ctx, const double *cool5x801, double mintemp, double dtemp);

/* Host state read at every evolve3D call because the driver rescales it each step
 * (cosmology.f90:159-202): material:ndens, grid:dr,vol, material:clumping (real(4)), cosmology:zred,
 * cosmology_parameters:H0,Omega0, material:isothermal,temper_val, and the twelve module-global
 * coefficients of cgsconstants.f90:106-133 in the order arech0, brech0, areche0, breche0, oreche0,
 * areche1, breche1, treche1, colli_HI, colli_HeI, colli_HeII, v (used as they stand when isothermal;
 * re-evaluated per cell from the temperature otherwise, evolve_point.F90:543). */
int c2r_set_step(c2r_ctx *ctx, const double *ndens, const double dr[3], double vol, float clumping,
                 double zred, double H0, double Omega0, int isothermal, double temper_val,
                 const double reccoef[12]);
/* The same without the density: material:ndens on the device stays as the last c2r_set_step (or c2r_scale_ndens) left it.
 * For hosts that know ndens has not changed since (a run without cosmological expansion), or has only been rescaled: */
int c2r_set_step_scalars(c2r_ctx *ctx, const double dr[3], double vol, float clumping, double zred, double H0, double Omega0,
                         int isothermal, double temper_val, const double reccoef[12]);
/* cosmo_evol's  ndens(:,:,:) = ndens(:,:,:) / zfactor3  (cosmology.f90:193) applied to the device copy: one correctly
 * rounded IEEE division per cell, the same bits as the host's.  The Fortran drop-in uses the two calls when
 * C2RAY_HIP_KEEP_STATE is set and a sample of the host array confirms that this is all that happened to it. */
int c2r_scale_ndens(c2r_ctx *ctx, double divisor);


/* Table construction on the device: spec_integration (radiation_tables.f90:172-422) for one SED from what
 * spectrum_parms, setup_scalingfactors (radiation_sizes.f90:62-688), romberg_initialisation(NumFreq)
 * (romberg.f90:24-92) and normalize_seds leave behind.  All of it is public module data of the reference:
 *   freq_min, delta_freq (47)          radiation_sizes
 *   xsec_index (47)                    cross_section_HI_powerlaw_index(1), ..HeI..(2:27), ..HeII..(28:47), the
 *                                      index spec_integration passes per band (radiation_tables.f90:278,315,349)
 *   tau (0:NumTau)                     radiation_tables:tau, romw = romberg:romw(0:NumFreq, 9)
 *   R_star2, h_over_kT                 radiation_sed_parameters (black body); pl_scaling/pl_index or
 *                                      qpl_scaling/qpl_index for sed = 1 / 2
 *   two_pi_over_c_square, hplanck (cgsconstants), pi (mathconstants), ion_freq_* (cgsphotoconstants)
 * The band vectors (c2r_set_tables with NULL tables) or the band range (c2r_set_sed_tables with NULL tables)
 * must have been given before.  Results are bit-identical to the reference's host-built tables.
 * c2r_download_tables returns tables in the reference's layout (0:NumTau, ncol); pointers may be NULL. */
typedef struct c2r_sed_setup {
  int nfreq;                /* NumFreq = 512 */
  int sed;                  /* 0 black body, 1 power law, 2 quasar-like power law */
  const double *freq_min, *delta_freq, *xsec_index, *tau, *romw;
  double R_star2, h_over_kT, two_pi_over_c_square, hplanck, pi;
  double ion_freq_HI, ion_freq_HeI, ion_freq_HeII;
  double pl_scaling, pl_index;
} c2r_sed_setup;
int c2r_build_tables(c2r_ctx *ctx, const c2r_sed_setup *setup, int with_heat);
int c2r_download_tables(c2r_ctx *ctx, int sed, double *photo_thick, double *photo_thin, double *heat_thick,
                        double *heat_thin);

/* Lyman-limit systems (c2ray_parameters.f90:72-78 use_LLS, type_of_LLS): a fog of unresolved absorbers added
 * to the incoming HI column of every cell but the source's, coldensh_in += coldensh_LLS*path/dr(1)
 * (evolve_point.F90:177-180).  use_lls = 0 switches it off (the reference's default); lls_grid == NULL is
 * type_of_LLS = 1 with material:coldensh_LLS as set by set_LLS each step (mat_ini_test.F90:640-662);
 * lls_grid != NULL is type_of_LLS = 2: material's REAL(4) LLS_grid(mesh) read per cell by LLS_point
 * (mat_ini_cubep3m.F90:859-870).  Stays in force until the next call.  LLS_loss stays 0 as in the
 * reference (it multiplies photo_in_HI, which photoion_rates never sets). */
int c2r_set_lls(c2r_ctx *ctx, int use_lls, double coldensh_lls, const float *lls_grid);

/* Position-dependent clumping, type_of_clumping = 5: material's REAL(4) clumping_grid(mesh), read per cell
 * by clumping_point in do_chemistry (evolve_point.F90:483-484) and in total_rates
 * (photonstatistics.f90:175-177).  NULL returns to the scalar material:clumping of c2r_set_step. */
int c2r_set_clumping_grid(c2r_ctx *ctx, const float *clumping_grid);

/* sourceprops: NumSrc, srcpos(3,NumSrc) (1-based mesh coordinates), NormFlux(1:NumSrc), and
 * radiation_sed_parameters:S_star (sourceprops_test.F90:38-40). */
int c2r_set_sources(c2r_ctx *ctx, int nsrc, const int *srcpos, const double *normflux, double s_star);

/* Point sources OUTSIDE the mesh: c2r_set_sources with one check replaced -- a position may lie outside the mesh
 * (srcpos_d < 1 or srcpos_d > mesh_d) along axes that are open (c2r_set_boundaries_axes): a quasar beside a slab, the
 * bright neighbour of a light-cone strip.  Diverging rays and 1/r^2 dilution, which no plane source can stand in for, and
 * none of the padding cells a wider mesh would pay for in every grid.  The reference has nothing of the kind.
 *   The mesh of such a source is the real one extended by vacuum up to the source: along an open axis its reach is
 * l = -min(max_subbox, max(srcpos - 1, 0)), r = min(max_subbox, max(mesh - srcpos, 0)).  A cell of its sub-box that lies
 * outside the mesh is a vacuum cell: neufrac * ndens = 0.0 exactly for HI, HeI and HeII, no LLS fog (scalar or grid),
 * N_out = N_in.  A mesh cell gets the arithmetic it always got, and rates are formed for mesh cells only.  photon_loss(1)
 * runs over the whole surface of the final sub-box, vacuum cells included -- photons that leave through a face of the
 * vacuum never meet the mesh --, so emitted = absorbed + lost keeps holding; the loss that decides whether a box grows and
 * sum_nbox are those of open boundaries.  Cost: the column scratch and the sweep follow the extended box, the rates the
 * mesh cells in it; c2r_get_source_trace counts the vacuum.
 *   A list whose sources all stand inside gives the bits, and launches the kernels, of c2r_set_sources, which keeps
 * refusing a position outside.  Everything is checked before anything is kept; refused, with a message that names the
 * source: a position outside along a periodic axis (so: any all-periodic context); a position more than max_subbox cells
 * from the mesh (no sub-box of it ever holds a mesh cell); a reach of more than 4096 cells to one side; a reach of 2^31
 * cells or more (a thin, long mesh: (2,2,1700) and a source 1149 cells beyond two faces); and a pass that is still open.  c2r_set_boundaries(_axes) refuses to make an axis
 * periodic while a source stands beyond it.  Beams, horizons, source curves, c2r_set_sources_sed, heating and LLS work
 * unchanged.  Not built, and refused while a source of the list stands outside: c2r_enable_face_loss,
 * c2r_enable_horizon_loss (and this call while either is on), and for such a source c2r_evolve0d and c2r_do_source. */
int c2r_set_sources_external(c2r_ctx *ctx, int nsrc, const int *srcpos, const double *normflux, double s_star);

/* Point-source HAND-OVER between meshes stacked along one open axis: a quasar or galaxy in the slab next door of a
 * light-cone strip.  The mesh that holds (or is nearer to) the source writes out the columns at its face, the next mesh takes
 * them in as a ghost layer and reproduces its part of one deep mesh.  (Planes have the same pair: c2r_download_plane_exit_columns
 * -> c2r_set_plane_entry_columns.)  The reference has nothing of the kind.
 *   Notation.  face = 2 * axis + high, as for the escape maps.  A face has F cells, in the order of
 * c2r_set_plane_entry_columns (the lower of the two remaining axes fastest); a STRIP is 3 F doubles, the species (HI, HeI, HeII)
 * slowest.  The LAYER of a face: the mesh cells with index 1 (high = 0) or mesh[axis] (high = 1) along the axis; its GHOST
 * LAYER: the cells one step outside, index 0 or mesh[axis] + 1.
 *
 * EXIT.  c2r_select_source_face_exit names the point sources (1-based) whose exit strip through `face` is kept: 3 F nsel
 * doubles per device; nsel = 0 frees everything of that face.  Every pass that sweeps a selected source -- c2r_pass_sources
 * and its slab-wise form, c2r_pass_allreduce_chemistry, c2r_iteration, c2r_evolve3d (its last iteration's pass), c2r_do_source
 * for a source inside the mesh -- fills the strip after the source's last round, before its column block is given back: N_out
 * of each layer cell (one more launch per face, k_source_face_exit; a periodic lateral axis maps the mesh index to the image
 * within the reach), +0.0 for a layer cell outside the source's final box.  It works for a source inside the mesh and for one
 * outside, with or without entry columns, so that a chain A -> B -> C passes the columns on.  Refused, with a message: a
 * face of a periodic axis, a face outside 0..5, a source number outside 1..NumSrc, a source named twice, a call between
 * c2r_pass_sources_begin and _end.  c2r_set_sources* drops the selection, as it drops beams; c2r_set_boundaries(_axes) refuses
 * to make the axis periodic while a selection exists.
 *   c2r_download_source_face_exit returns the strip, nbox of that pass for ns (rounds) and reached = 1 iff the final box held
 * at least one cell of the layer.  Refused before any pass swept ns with the selection in place, and while a slab-wise pass
 * is open; a multi-device context answers from the device that swept ns.
 *
 * ENTRY.  c2r_set_source_face_entry gives source ns, which must stand outside the mesh beyond `face` along that axis only
 * (its other two coordinates inside the mesh; a neighbour across an edge or a corner is refused by this call: HALO below), the strip cols3 of the mesh
 * upstream and the rounds that mesh traced; cols3 = NULL clears the entry.
 *   Ghost layer: the vacuum rule of c2r_set_sources_external changes in one place for this source -- a cell of its box in the
 * ghost layer of `face` stores N_out = cols3[species][face cell] instead of N_in.  Every other vacuum cell stays vacuum
 * (nobody downstream of the ghost layer reads one: every upstream corner of a mesh cell lies in the mesh or in the ghost
 * layer); no LLS fog is added in the ghost layer (the upstream mesh added its own); mesh cells get the arithmetic they always
 * got.
 *   Rounds: the source is traced for exactly `rounds` rounds (>= 1; fewer where no face of its reach can move any more).  No
 * deciding loss is formed for it and no probe is launched for it: the mesh that holds the source decides how far it is traced,
 * every mesh downstream covers the same cube cut at its own reach, so every ghost cell that is read was inside the upstream
 * box.  (A mesh upstream whose box ended at its own reach has decided nothing -- its trace says so, box == reach --: the host
 * then hands down at least the rounds the mesh downstream needs to run to its reach.)  sum_nbox counts the rounds traced.
 *   Kept loss: photon_loss(1) receives, for such a source, only the terms of the surface cells of the final box that are mesh
 * cells; what the vacuum surface "loses" is the upstream mesh's business.  (Upstream, the mesh's own photon_loss(1) still
 * counts what crosses the interface: the combined budget of a stack is not closed.)
 *   Kernels: a batch that holds a source with an entry runs k_sweep_shell_entry, k_sweep_shell_fast_entry and k_loss_entry;
 * every other batch launches what it always launched, with the same bits.
 *   Identities.  ZERO STRIP: an all-zero strip with `rounds` equal to the rounds the source takes without an entry gives the
 * rate grids of the run without an entry, bit for bit (vacuum columns are exactly 0).  HAND-OVER: let W be one mesh open along
 * the axis, A and B its two parts, the source in A, both traced as far as W traces it; with A's exit strip and W's rounds B has
 * W's incoming and outgoing columns and rate grids on its cells bit for bit where B keeps W's absolute indices (B begins at W's
 * index 1: the source beyond B's HIGH face), and to rounding where B's indices are shifted: cinterp forms its crossing points
 * from absolute coordinates.  The shift matters in the cells that lie on a face of their shell across another axis than the
 * stack's (their crossing points use the source's coordinate along the stack's axis); a part, or a strip, all of whose cells and
 * their ancestors lie further from the source along the stack's axis than across it has W's bits although it is shifted.
 *   c2r_set_mesh_origin removes the rounding for parts that lie anywhere in W: origin_d = W's index of the part's cell 1
 * along axis d, minus 1 (W's index = the part's + origin).  cinterp then forms its crossing points from W's coordinates -- every
 * source's position moved by the origin, in the sweep kernels only; cells, offsets, reaches and blocks stay the part's -- and
 * the part has W's bits: in a chain A -> B -> C = W's 25..36, 13..24, 1..12 with the origins 24, 12 and 0 along z, B and C
 * equal W bit for bit.  A context with a non-zero origin runs every batch through k_sweep_shell_entry and
 * k_sweep_shell_fast_entry, a source with an entry or not; with the origin 0 it launches what it always launched.  Refused: a
 * non-zero origin along a periodic axis, |origin_d| > 2^20, an open slab-wise pass; c2r_set_boundaries(_axes) refuses to make an
 * axis periodic while the origin along it is not 0.  The origin belongs to the mesh: source lists come and go, it stays.
 *   Refused, with a message and leaving everything unchanged: a bad ns or face, a source that does not stand beyond exactly
 * that face, rounds < 1, a negative or non-finite column, a call inside an open slab-wise pass.  c2r_set_sources* clears the
 * entries; c2r_set_boundaries*, beams, horizons and curves keep them.  The call acts on every device of a multi-device
 * context.  c2r_get_source_face_entry returns face = -1 (and rounds = 0) while none is set.  c2r_get_source_trace keeps
 * counting the vacuum.  Still refused for a source outside the mesh: the escape maps, the horizon loss, c2r_do_source and
 * c2r_evolve0d.
 *
 * HALO.  c2r_set_source_halo is the entry of a source that stands beyond two or three faces: the neighbour across an edge or a
 * corner of a mesh tiled in 2-D or 3-D.  The source ns stands outside the mesh along the axis set B, 1 <= |B| <= 3; for d in B
 * the side is h_d = 1 if srcpos_d > mesh_d, 0 if srcpos_d < 1, and the ghost index g_d = mesh_d + 1 for h_d = 1, 0 for h_d = 0
 * (1-based).  Take a cell of the source's box outside the mesh, at mesh index m, and let O be the axes along which m lies
 * outside 1..mesh.  The cell is a GHOST CELL iff O is a subset of B and m_d = g_d for every d in O; it stores N_out from the halo
 * instead of its N_in:
 *   |O| = 1, O = {d}: face[d], the strip of face 2d + h_d, at the cell's face cell -- the ghost layer and the layout of ENTRY;
 *   |O| = 2:          edge[e], the EDGE LINE along the remaining axis e, 3 mesh[e] doubles, species slowest, at entry m_e - 1;
 *   |O| = 3:          the CORNER, 3 doubles.
 * Every other vacuum cell stays vacuum, no LLS fog is added in a ghost cell, mesh cells get the arithmetic they always got.
 * The rule is complete: every upstream corner of a mesh cell lies at most one step outside the mesh per axis, and only along
 * axes of B (the upstream cells lie towards the source), so it lies in the mesh or is a ghost cell -- nobody downstream of a
 * ghost cell reads any other vacuum cell.  Rounds and kept loss are ENTRY's: exactly `rounds` rounds, no deciding loss, no
 * probe; photon_loss(1) receives only the terms of the surface cells of the final box that are mesh cells.
 *   A halo is whole: a strip for every d in B, an edge line along e for every e whose two other axes both lie in B, the corner
 * iff |B| = 3, and nothing else.  An edge line or the corner of a part of W is a cell of the diagonal neighbour's layer and is
 * read out of that neighbour's exit strip (either of the two strips that hold it); the exit side is unchanged.
 *   A halo of one face IS the entry of that face: the same bits, the same kernels, and c2r_get_source_face_entry reports it.
 * c2r_set_source_face_entry replaces a halo, and its cols3 = NULL clears either kind, as halo = NULL does here;
 * c2r_get_source_face_entry returns, for a halo of several faces, the lowest face number and the rounds.  c2r_get_source_halo
 * returns faces[d] = 2d + h_d, or -1 where the source has no strip along d; all -1 and rounds = 0 while none is set.
 *   Kernels: a batch that holds a source whose halo has several faces runs k_sweep_shell_halo and k_sweep_shell_fast_halo
 * (the entry kernels' twins with the ghost rule above) and k_loss_entry; every other batch launches what it always launched,
 * with the same bits.  ZERO STRIP holds for a halo whose arrays are all zero; HAND-OVER holds for a W tiled along two or
 * three axes, each part placed with c2r_set_mesh_origin: every part has W's bits on its cells.
 *   Everything is checked before anything is kept; refused, with a message that names the source and leaving everything
 * unchanged: a bad ns, an open slab-wise pass, rounds < 1, a source inside the mesh, a strip, line or corner that is missing,
 * one that is superfluous (given for an axis the source stands inside along, or for an edge whose two other axes are not both
 * in B), a negative or non-finite column (the message names the array and the entry).  -0.0 is stored as +0.0.  Lifetime as
 * for entries: c2r_set_sources* clears halos; boundaries, beams, horizons and curves keep them; the call acts on every device
 * of a multi-device context. */
typedef struct {
  int rounds;               /* >= 1, as for c2r_set_source_face_entry */
  const double *face[3];    /* face[d]: the strip of face 2d + h_d, or NULL where the source stands inside along d */
  const double *edge[3];    /* edge[e]: the line along axis e (3 * mesh[e]), needed iff the source stands outside along both other axes */
  const double *corner;     /* 3 doubles, needed iff the source stands outside along all three */
} c2r_source_halo;
int c2r_select_source_face_exit(c2r_ctx *ctx, int face, int nsel, const int *sources);
int c2r_download_source_face_exit(c2r_ctx *ctx, int face, int ns, double *cols3, int *rounds, int *reached);
int c2r_set_source_face_entry(c2r_ctx *ctx, int ns, int face, const double *cols3, int rounds);
int c2r_get_source_face_entry(c2r_ctx *ctx, int ns, int *face, int *rounds);
int c2r_set_source_halo(c2r_ctx *ctx, int ns, const c2r_source_halo *halo);   /* halo == NULL clears */
int c2r_get_source_halo(c2r_ctx *ctx, int ns, int faces[3], int *rounds);     /* faces[d] = 2d + h_d, or -1; all -1 and rounds 0 while none */
int c2r_set_mesh_origin(c2r_ctx *ctx, const int origin[3]);
int c2r_get_mesh_origin(c2r_ctx *ctx, int origin[3]);

/* The -DPL / -DQUASARS builds of the reference give every source up to two more SEDs
 * (radiation_photoionrates.f90:215-228, 256-271).  sed = 1: power law (pl_*), sed = 2: quasar-like (qpl_*).
 *   c2r_set_sed_tables   pl_/qpl_photo_thick/thin_table, pl_/qpl_heat_thick/thin_table (heat may be NULL
 *                        for isothermal-only use) and pl_/qpl_FreqBnd_LowerLimit..UpperLimit (1-based,
 *                        inclusive; radiation_tables.f90:207-256)
 *   c2r_set_sources_sed  NormFluxPL / NormFluxQPL(1:NumSrc) and pl_S_star / qpl_S_star; call after
 *                        c2r_set_sources (which clears them); NULL switches the SED off again */
int c2r_set_sed_tables(c2r_ctx *ctx, int sed, const double *photo_thick, const double *photo_thin,
                       const double *heat_thick, const double *heat_thin, int lower, int upper);
int c2r_set_sources_sed(c2r_ctx *ctx, int sed, const double *normflux, double s_star);

/* Beamed point sources: an emission cone or bicone per source -- a quasar that lights a cone, not a sphere.  The reference
 * has nothing of the kind; a source at infinity gets its direction from c2r_set_plane_tilt, a source inside the box here.
 *   kind      0 none (the source radiates isotropically, as every source of the reference), 1 cone, 2 bicone
 *   axis      the beam's axis in the physical directions x, y, z; it need not be normalised
 *   cos_half  the cosine of the half opening angle, 0 <= cos_half <= 1
 * The rule (csrc/c2ray_beam.hpp).  When the beams are set the host forms one double per source,
 *     K = (cos_half*cos_half) * ((a_x*a_x + a_y*a_y) + a_z*a_z).
 * For a cell at offset (di, dj, dk) from the source -- the offset exactly as the kernel in question already forms it: the
 * image within the reach on a periodic axis, the plain difference on an open one -- and the dr of the pass, every product
 * and sum rounded as written and evaluated from the left:
 *     xs = dr1*(double)di    ys = dr2*(double)dj    zs = dr3*(double)dk
 *     dot = (xs*a_x + ys*a_y) + zs*a_z
 *     d2  = (xs*xs + ys*ys) + zs*zs
 *     cone:    lit  iff  dot >= 0.0  &&  dot*dot >= K*d2
 *     bicone:  lit  iff  dot*dot >= K*d2
 * No square root and no division: a cell exactly on the cone is lit, and so is the source's own cell (0 >= 0).
 * An UNLIT cell behaves, for that source only, exactly like a cell with N_in(HI) >= max_coldensh: it adds nothing to phih,
 * phihe or phiheat, and its loss term photo_out*vol/vol_ph is 0.0 in the loss that decides whether the sub-box grows, in the
 * loss that is kept, in photon_loss(1) and in the escape maps.  A LIT cell gets the bits it gets without a beam.
 * What a beam does not do.  NormFlux stays the isotropic-equivalent flux: nothing is rescaled to conserve photons.  The
 * threshold 1e-10 * total_source_flux of the sub-box loop is unchanged (a beam can only end the loop earlier).  Columns are
 * swept as before, over the whole box, lit or not; sum_nbox counts rounds as before.  Planes are untouched.
 * Identities.
 *   Beams off: with no beams set, or every kind == 0, every grid, loss, map and sum_nbox has the bits it had before beams
 *     existed, from the same kernel launches.
 *   Full bicone: a bicone with cos_half = 0 lights every cell; the results are the unbeamed bits, through the beamed kernels.
 *   One beamed source, from zeroed grids: every rate grid equals the unbeamed source's grid where the cell is lit and +0.0
 *     elsewhere, provided both runs trace the same rounds.
 *   Several sources: grid = grid + where(lit_s, term_s, 0.0), folded in source order.
 * c2r_set_source_beams gives all NumSrc sources their beams at once (nsrc must equal the NumSrc of c2r_set_sources); beams =
 * NULL: no source is beamed.  c2r_set_sources clears the beams, as it clears the extra SEDs; c2r_set_boundaries* keep them.
 * The beams act on every device of a multi-device context, and every route that traces a point source honours them:
 * c2r_pass_sources and its slab-wise form, c2r_do_source, c2r_pass_allreduce_chemistry, c2r_iteration, c2r_evolve3d,
 * c2r_evolve0d (the loss of an unlit surface cell is 0.0) and the escape maps.
 * Refused, each with an error text: a call between c2r_pass_sources_begin and c2r_pass_sources_end; nsrc != NumSrc; a kind
 * outside 0..2; a non-finite axis component; an axis whose squared length is zero or not a normal finite double; a cos_half
 * outside [0, 1] or not finite.  (axis and cos_half of a source with kind == 0 mean nothing and are not looked at: a
 * zeroed record is "no beam".)  A refused call changes nothing.
 * c2r_get_source_beam returns the beam of source ns (1-based) as it was set; kind 0, axis {0, 0, 0}, cos_half 0 while none
 * is set. */
typedef struct {
  int kind;
  double axis[3];
  double cos_half;
} c2r_source_beam;
int c2r_set_source_beams(c2r_ctx *ctx, int nsrc, const c2r_source_beam *beams);
int c2r_get_source_beam(const c2r_ctx *ctx, int ns, c2r_source_beam *out);

/* Photon horizons: a maximum ray length per point source -- a mean free path set by unresolved absorbers, or the causal front
 * c*(t - t_on) of a source that has just switched on.  The reference's only cap is max_subbox, a compile-time cube in cells.
 *   radius    one double per source, in the length unit of dr: a PHYSICAL length, so a pass uses the dr of that pass (a host
 *             that wants a comoving horizon rescales it as it rescales dr); finite and >= 0, or +infinity: no horizon
 * The rule (csrc/c2ray_horizon.hpp).  When the horizons are set the host forms one double per source, R2 = radius*radius.
 * For a cell at offset (di, dj, dk) from the source -- the offset exactly as the kernel in question already forms it, as for
 * a beam -- and the dr of the pass, every product and sum rounded as written and evaluated from the left (the beam's own xs,
 * ys, zs, d2):
 *     xs = dr1*(double)di    ys = dr2*(double)dj    zs = dr3*(double)dk
 *     d2 = (xs*xs + ys*ys) + zs*zs
 *     within  iff  d2 <= R2
 * No square root and no division: a cell exactly on the sphere is within, and so is the source's own cell (0 <= R2); radius =
 * 0 lights the own cell only; a radius so large that R2 overflows to +infinity lights everything.
 * A cell that is NOT within is UNLIT for that source, in exactly the sense of c2r_set_source_beams: it adds nothing to phih,
 * phihe or phiheat, and its loss term photo_out*vol/vol_ph is 0.0 in the loss that decides whether the sub-box grows, in the
 * loss that is kept, in photon_loss(1) and in the escape maps.  A LIT cell gets the bits it gets without a horizon.  A source
 * with a beam and a horizon lights a cell iff both predicates hold.
 * What a horizon does not do.  Columns are swept as before, over the whole box (a cell within the sphere only interpolates
 * from cells nearer the source, which are within it too).  The threshold 1e-10 * total_source_flux of the sub-box loop and
 * the counting of sum_nbox are unchanged: the loop ends at the first sub-box that contains the sphere, because the deciding
 * loss becomes 0.0.  Reaches, column blocks and tile lists are untouched.  Planes are untouched.
 * THERE IS NO HORIZON LOSS unless c2r_enable_horizon_loss (below): photons cut off at the sphere appear in no loss and no
 * map, and with a horizon set photon_loss alone does not close the photon budget; the horizon loss does.
 * Identities.
 *   Horizons off: with none set, or every radius +infinity, every grid, loss, map and sum_nbox has the bits it had before
 *     horizons existed, from the same kernel launches.
 *   Infinite R2: a finite radius whose square overflows (1e200) lights every cell; the results are the unhorizoned bits,
 *     through the beamed kernels.
 * c2r_set_source_horizons gives all NumSrc sources their horizons at once (nsrc must equal the NumSrc of c2r_set_sources);
 * radius = NULL: no source has a horizon.  c2r_set_sources clears the horizons, as it clears beams and extra SEDs;
 * c2r_set_boundaries* and c2r_set_source_beams keep them.  The horizons act on every device of a multi-device context, and
 * every route that traces a point source honours them: c2r_pass_sources and its slab-wise form, c2r_do_source,
 * c2r_pass_allreduce_chemistry, c2r_iteration, c2r_evolve3d, c2r_evolve0d (the loss of an unlit surface cell is 0.0) and the
 * escape maps.
 * Refused, each with an error text: a call between c2r_pass_sources_begin and c2r_pass_sources_end; nsrc != NumSrc; a NaN or
 * negative radius.  A refused call changes nothing.
 * c2r_get_source_horizon returns the radius of source ns (1-based) as it was set, +infinity while none is set; an ns outside
 * 1..NumSrc is refused with an error text. */
int c2r_set_source_horizons(c2r_ctx *ctx, int nsrc, const double *radius);
int c2r_get_source_horizon(const c2r_ctx *ctx, int ns, double *radius);

/* Source light curves: a flux factor per shell of distance, per point source.  A cell at distance r sees a source at the
 * retarded time t - r/c, and the light-crossing time of a large box is many time steps: a host that knows a source's history
 * (a galaxy whose emissivity grows, a quasar that flickers or has switched off, a burst) hands it over as a piecewise-constant
 * curve, radius[k] = c*(t - t_k) and factor = L(t_k)/L(t).  A horizon is the crudest such curve: 1 within the sphere, 0 beyond.
 *   nstep     the number of steps, 0 .. C2R_CURVE_MAX_STEPS
 *   radius    radius[0..nstep-1]: physical lengths in the length unit of dr (a pass uses the dr of that pass, as for a
 *             horizon), finite, >= 0 and strictly ascending
 *   factor    factor[0..nstep]: finite and >= 0; factor[b] holds in distance shell b.  The shells are [0, r0], (r0, r1], ...,
 *             (r_{nstep-1}, infinity)
 * Entries behind nstep (radius) and nstep + 1 (factor) mean nothing and are not looked at.
 * The rule (csrc/c2ray_curve.hpp).  When the curves are set the host forms R2[k] = radius[k]*radius[k] for k < nstep.  For a
 * cell at offset (di, dj, dk) from the source -- the offset exactly as the kernel in question already forms it, as for a beam
 * -- and the dr of the pass, every product and sum rounded as written and evaluated from the left (the horizon's own xs, ys,
 * zs, d2):
 *     xs = dr1*(double)di    ys = dr2*(double)dj    zs = dr3*(double)dk
 *     d2 = (xs*xs + ys*ys) + zs*zs
 *     b  = the number of k < nstep with d2 > R2[k]
 *     f  = factor[b]
 * No square root and no division: a cell exactly on a radius belongs to the inner shell, and the source's own cell is always
 * shell 0.
 * A cell with f == 0.0 is UNLIT for that source, in exactly the sense of c2r_set_source_beams: it adds nothing to phih, phihe
 * or phiheat, and its loss term photo_out*vol/vol_ph is 0.0 in the loss that decides whether the sub-box grows, in the loss
 * that is kept, in photon_loss(1), in the escape maps and in the horizon rim (the po of a rim face is formed with the face
 * cell's scaled flux; a cell with f = 0 has no face).  Any other cell runs the per-cell routine the source always ran, with the
 * same columns and vol_ph, and NormFlux*f in the place of NormFlux -- in a three-SED run NormFluxPL*f and NormFluxQPL*f as
 * well: one rounded product per SED and nothing else, so f == 1.0 gives the uncurved bits.  A source with a beam, a horizon
 * and a curve lights a cell iff it is lit for each of them.
 * What a curve does not do.  Columns are swept as before.  The threshold 1e-10 * total_source_flux of the sub-box loop uses
 * the unscaled fluxes; sum_nbox, reaches, column blocks and tile lists are untouched.  Planes are untouched.  Nothing is
 * rescaled to conserve anything.
 * Identities.
 *   Curves off: with none set, or every source nstep = 0 and factor[0] = 1.0, every grid, loss, map and sum_nbox has the bits
 *     it had before curves existed, from the same kernel launches.
 *   All factors 1.0: the uncurved bits, through the curved kernel.
 *   Step to zero: {1, {R}, {1, 0}} is the horizon R bit for bit, rounds included.
 *   A factor 2^n scales phih, phihe, phiheat and the loss terms of its shell exactly.
 * c2r_set_source_curves gives all NumSrc sources their curves at once (nsrc must equal the NumSrc of c2r_set_sources); curves
 * = NULL: no source has a curve.  A source with nstep == 0 and factor[0] == 1.0 has no curve.  c2r_set_sources clears the
 * curves; c2r_set_boundaries*, c2r_set_source_beams and c2r_set_source_horizons keep them.  The curves act on every device of
 * a multi-device context, and every route that traces a point source honours them: c2r_pass_sources and its slab-wise form,
 * c2r_do_source, c2r_pass_allreduce_chemistry, c2r_iteration, c2r_evolve3d, c2r_evolve0d, the escape maps and the horizon
 * loss.
 * Refused, each with an error text: a call between c2r_pass_sources_begin and c2r_pass_sources_end; nsrc != NumSrc; an nstep
 * outside 0..C2R_CURVE_MAX_STEPS; a radius that is negative, not finite or not above its predecessor; a factor that is
 * negative or not finite; and a ZEROED RECORD (nstep == 0 and factor[0] == 0.0).  By the rule that record is a source that
 * lights nothing, which is not what a record nobody filled in should do, and reading it as "no curve" would make factor[0]
 * = 0 the one factor that does not scale: so it is refused, "no curve" is factor[0] = 1.0, and a source that has gone dark
 * is {1, {0.0}, {0.0, 0.0}}.  A refused call changes nothing.
 * c2r_get_source_curve returns the curve of source ns (1-based) as it was set, the entries behind its steps zeroed, and {0, {},
 * {1.0}} while none is set; an ns outside 1..NumSrc is refused with an error text. */
#define C2R_CURVE_MAX_STEPS 8
typedef struct {
  int nstep;
  double radius[C2R_CURVE_MAX_STEPS];
  double factor[C2R_CURVE_MAX_STEPS + 1];
} c2r_source_curve;
int c2r_set_source_curves(c2r_ctx *ctx, int nsrc, const c2r_source_curve *curves);
int c2r_get_source_curve(const c2r_ctx *ctx, int ns, c2r_source_curve *out);

/* Horizon loss: what crosses each source's photon horizon, per source.  The rule (csrc/c2ray_rim.hpp).  The cells within a
 * horizon are a closed staircase around the source whose boundary is made of cell faces; the solid angles of those faces add up
 * to 4 pi, so a weight per exposed face, taken at the face centre, tiles the sphere: summed over a box that contains the
 * sphere the weights give 1 to within 6.3e-4 at a radius of 5 cells and 4e-6 at 16.
 * For one point source with a finite horizon: R2, the dr of the pass and the final sub-box lo[3]..hi[3] (offsets).
 *   Sheets.  Six sheets, fc = 2*d + (s > 0 ? 1 : 0) for axis d and sign s = -1, +1 (the face numbering of the escape maps).
 *     Sheet fc has one entry per pair of transverse offsets (oa, ob), the two other axes a < b, a fastest, over the box's
 *     extents E_a = hi_a - lo_a + 1 and E_b: entry (oa - lo_a) + E_a*(ob - lo_b).  The six sheets lie one behind the other in
 *     face order, T = 2*(E1*E2 + E0*E2 + E0*E1) entries.
 *   The face of a sheet column.  Along the column cells have o_d = s*k, k = 0, 1, ...; the predicate above is monotone in k.
 *     If the k = 0 cell is not within, the column has no face.  Otherwise k* is the largest k whose cell is within and inside
 *     the box, and the column has a face iff that cell is not on the surface of the final box on any axis (lo_e < o_e < hi_e
 *     for all e: surface cells give their term to the kept loss), the cell at k* + 1 is not within, and the cell is lit (a
 *     beam-unlit cell has no face).  The two sheets of an axis both see the k = 0 cell; each owns its own face of it.
 *   Weight: the solid angle over 4 pi of that face at its centre, every product and sum rounded as written and evaluated from
 *     the left, no contraction (pi: the float-rounded constant of the kept loss):
 *         xa = dr_a*(double)oa     xb = dr_b*(double)ob     fd = dr_d*((double)k* + 0.5)
 *         f2 = (xa*xa + xb*xb) + fd*fd
 *         w  = ((dr_a*dr_b)*fd) / ((4.0*pi)*(f2*sqrt(f2)))
 *     The source's own cell (oa = ob = 0, k* = 0) takes w = 1.0/6.0 instead.
 *   Term: po * w, po the photo_out of the cell from its six stored columns, formed as the escape maps form it (0.0 where
 *     N_in(HI) >= max_coldensh); a column without a face has the term +0.0.
 *   The horizon loss of a source in a pass: its T terms added in the fixed order of c2r_get_face_loss (blocks of 256 by a
 *     tree, then the block sums in order).  No float atomics: the same bits on every run and for every c2r_set_batch.
 * Off by default; while it is off nothing is allocated, launched or waited for.  The values live as photon_loss lives:
 * c2r_set_rates_to_zero clears them, every pass that sweeps source ns does loss[ns] = loss[ns] + (that pass's sum), a source
 * without a finite horizon stays 0.0.  c2r_set_sources, c2r_set_source_horizons and a change of boundary mode zero them.
 * Routes that honour it: c2r_pass_sources and its slab-wise form (complete after c2r_pass_sources_end), c2r_do_source,
 * c2r_pass_allreduce_chemistry, c2r_iteration and c2r_evolve3d (the last iteration's pass).  c2r_evolve0d and planes do not
 * know it.  It is NOT part of the reduction buffer: c2r_rates_count and its layout are unchanged; a multi-device context
 * answers per source from the device that swept it (the devices' values added in device order), across processes a rank
 * reports its own sources and 0.0 for the others.  It changes no bit of any rate grid, photon_loss, escape map, sum_nbox,
 * sub-box decision or existing launch.
 * c2r_get_horizon_loss: per_source (may be NULL) takes nsrc doubles, nsrc must equal NumSrc; *total (may be NULL) their sum in
 * source order, added on the host.
 * c2r_download_horizon_rim (a diagnostic, like c2r_download_columns): the T terms of the point source with a finite horizon
 * that was swept last, its number *ns (1-based) and the extents extent[3] of its final box.  With capacity < T the call is
 * refused, its error text names T, and *ns and extent[] are set all the same (T follows from them).
 * Refused, each with an error text: enabling or disabling between c2r_pass_sources_begin and _end; nsrc != NumSrc; either
 * getter while the feature is off or while a slab-wise pass is open; a download before any horizoned source was swept; a
 * capacity < T. */
int c2r_enable_horizon_loss(c2r_ctx *ctx, int on);
int c2r_get_horizon_loss_enabled(const c2r_ctx *ctx);
int c2r_get_horizon_loss(c2r_ctx *ctx, int nsrc, double *per_source, double *total);
int c2r_download_horizon_rim(c2r_ctx *ctx, int *ns, int extent[3], double *terms, long long capacity);

/* material:xh, xhe, temperature_grid (temperature may be NULL when isothermal) */
int c2r_upload_state(c2r_ctx *ctx, const double *xh, const double *xhe, const float *temperature);
int c2r_download_state(c2r_ctx *ctx, double *xh, double *xhe, float *temperature);

/* evolve3D(time,dt,restart) with restart == 0 (files_for_3D/evolve.F90:78-229): the whole
 * convergence loop on the device.  niter_out: number of outer iterations; conv_flags_out (may be
 * NULL, capacity cap): non-converged count after each global pass (evolve.F90:488). */
int c2r_evolve3d(c2r_ctx *ctx, double dt, int *niter_out, int *conv_flags_out, int cap);

/* The pieces of evolve3D, for hosts that drive the loop themselves (multi-rank runs reduce the
 * rate grids between c2r_pass_sources and c2r_global_pass):
 *   c2r_begin_step      evolve.F90:131-136  xh_av = xh_intermed = xh, xhe_* likewise
 *   c2r_set_rates_to_zero evolve.F90:371-381 (carried out by the next pass's first rates launch, or by whoever reads
 *                       the grids first: nothing observable differs)
 *   c2r_pass_sources    do_grid_static (master_slave.F90:74-96): do_source for ns = first,
 *                       first+stride, ... <= NumSrc (1-based) -- evolve_source.F90:66-238
 *   c2r_global_pass     evolve.F90:435-501 loop: evolve0D_global for every cell
 *   c2r_end_step        evolve.F90:164-166  xh = xh_intermed, xhe = xhe_intermed,
 *                       set_final_temperature_point */
int c2r_begin_step(c2r_ctx *ctx);
int c2r_set_rates_to_zero(c2r_ctx *ctx);
int c2r_pass_sources(c2r_ctx *ctx, int first, int stride);
/* The same pass, handing the rate grids over in nslab slabs of k-planes while later slabs are still being
 * computed, so that a multi-rank host can start the sum over ranks (mpi_accumulate_grid_quantities,
 * evolve.F90:505-548) of slab s while the device works on slabs s+1..:
 *   c2r_pass_sources_begin  queues the whole pass and returns without waiting for the device
 *   c2r_pass_slab_count     slabs of the open pass (<= nslab: at least one 4-plane tile layer each)
 *   c2r_pass_wait_slab      blocks until phih/phihe/phiheat of slab `slab` hold this rank's final sums;
 *                           the slab is cells [first_cell, first_cell + ncells) of every component grid
 *   c2r_pass_sources_end    waits for the rest (photon_loss, sum_nbox, timing); must close every begin */
int c2r_pass_sources_begin(c2r_ctx *ctx, int first, int stride, int nslab);
int c2r_pass_slab_count(c2r_ctx *ctx);
int c2r_pass_wait_slab(c2r_ctx *ctx, int slab, size_t *first_cell, size_t *ncells);
int c2r_pass_sources_end(c2r_ctx *ctx);
/* do_source(dt,ns1,niter) (evolve_source.F90:66-238) for the single source ns1 (1-based): trace it
 * and add its contribution to the rate grids, photon_loss(1) and sum_nbox. */
int c2r_do_source(c2r_ctx *ctx, int ns);
int c2r_global_pass(c2r_ctx *ctx, double dt, int *conv_flag);
/* The same pass in pieces, for a multi-rank host that applies the rates of a slab of cells as soon as their
 * sum over ranks is complete: c2r_global_pass_cells queues evolve0D_global for cells [first_cell, first_cell +
 * ncells) on the library's stream, after `after_event` (a hipEvent_t recorded on the stream that finishes the
 * sum, or NULL); the piece starting at cell 0 opens a pass.  c2r_global_pass_finish waits for all pieces and
 * returns the non-converged count of the pass. */
int c2r_global_pass_cells(c2r_ctx *ctx, double dt, size_t first_cell, size_t ncells, void *after_event);
int c2r_global_pass_finish(c2r_ctx *ctx, int *conv_flag);
int c2r_end_step(c2r_ctx *ctx);

/* evolve_data: phih_grid, phihe_grid(:,:,:,0:1), phiheat; photonstatistics: photon_loss(1:47)
 * (as summed over this rank's sources, i.e. photon_loss_all before the division by mesh^3 of
 * evolve.F90:457); evolve_source: sum_nbox.  Any pointer may be NULL. */
int c2r_download_rates(c2r_ctx *ctx, double *phih, double *phihe, double *phiheat,
                       double *photon_loss47, int *sum_nbox);
/* The same with the grids chosen by a mask (bit 0 phih, bit 1 phihe, bit 2 phiheat) instead of by null pointers, for
 * hosts whose language cannot pass a null array: the Fortran drop-in leaves phiheat on the device in isothermal runs
 * (the grid is zero there and on the host, evolve_data.F90:80 -- 134 MB of PCIe per evolve3D call at 256^3). */
int c2r_download_rates_sel(c2r_ctx *ctx, int which, double *phih, double *phihe, double *phiheat,
                           double *photon_loss47, int *sum_nbox);
/* photon_loss(1:47) and sum_nbox of this rank's sources since the last c2r_set_rates_to_zero, from
 * the host-side bookkeeping (no device copy). */
int c2r_get_loss(c2r_ctx *ctx, double *photon_loss47, int *sum_nbox);
/* evolve_data: xh_av, xhe_av, xh_intermed, xhe_intermed -- the iteration-dump content
 * (write_iteration_dump, evolve.F90:233-275). */
int c2r_download_iter_state(c2r_ctx *ctx, double *xh_av, double *xhe_av, double *xh_intermed,
                            double *xhe_intermed);
/* start_from_dump (evolve.F90:279-367) reloads exactly these arrays before calling global_pass:
 * phih_grid, phihe_grid, [phiheat], xh_av, xhe_av, xh_intermed, xhe_intermed.  Any pointer may be
 * NULL (left as is). */
int c2r_upload_rates(c2r_ctx *ctx, const double *phih, const double *phihe, const double *phiheat);
int c2r_upload_iter_state(c2r_ctx *ctx, const double *xh_av, const double *xhe_av,
                          const double *xh_intermed, const double *xhe_intermed);
/* evolve_data: coldensh_out, coldenshe_out(:,:,:,0:1) of the source swept last (diagnostic). */
int c2r_download_columns(c2r_ctx *ctx, double *coldensh_out, double *coldenshe_out);

/* Photon statistics on the device (files_for_3D/photonstatistics.f90) -- the grid reductions the
 * reference runs on the host before and after every evolve3D call:
 *   c2r_state_sums   state_before (:117-144) / state_after (:208-234): number of H0, H+, He0, He+, He++
 *                    (sum of ndens*x times vol*(1-abu_he) or vol*abu_he) of which = 0: xh,xhe;
 *                    1: xh_intermed,xhe_intermed; 2: xh_av,xhe_av
 *   c2r_total_rates  total_rates (:150-203) on the time-averaged fractions xh_av,xhe_av with the given
 *                    twelve coefficients: out = totrec, totcollisions, recomions (already x vol x dt)
 *   c2r_get_reccoef  the module-global coefficients of cgsconstants.f90:106-133 as the reference's
 *                    global pass leaves them (isothermal: unchanged; otherwise what the last cell
 *                    (mesh,mesh,mesh) computed last, evolve_point.F90:543) -- total_rates uses these.
 * The sums are deterministic but associate differently from the reference's serial loops: they agree
 * with it to rounding, not bit for bit. */
int c2r_state_sums(c2r_ctx *ctx, int which, double out5[5]);
/* sum(x(:,:,:,n))/mesh^3 for the five fractions of `which` -- the "Intermediate result for mean
 * ... ionization fraction" lines of global_pass (evolve.F90:489-494) */
int c2r_fraction_means(c2r_ctx *ctx, int which, double out5[5]);
int c2r_total_rates(c2r_ctx *ctx, double dt, const double reccoef[12], double out3[3]);
int c2r_get_reccoef(c2r_ctx *ctx, double out12[12]);

/* The buffer that mpi_accumulate_grid_quantities (evolve.F90:505-548) sums over ranks, as ONE
 * contiguous device array of c2r_rates_count() doubles:
 *   [ phih_grid | phihe_grid(0) | phihe_grid(1) | phiheat | photon_loss(1:47) | sum_nbox ]
 * so that a single all-reduce(SUM, fp64) replaces the reference's four grid all-reduces and two
 * small ones.  c2r_rates_device_ptr returns its device address (after c2r_synchronize the data is
 * complete); c2r_set_rates_buffer makes the library use a caller-allocated device buffer instead
 * (e.g. a torch tensor that torch.distributed/RCCL reduces in place). */
size_t c2r_rates_count(const c2r_ctx *ctx);
void *c2r_rates_device_ptr(c2r_ctx *ctx);
int c2r_set_rates_buffer(c2r_ctx *ctx, void *device_ptr, size_t count);
int c2r_synchronize(c2r_ctx *ctx);

/* evolve0D_global(dt,pos,conv_flag) (files_for_3D/evolve_point.F90:325-440) for the ONE cell at 1-based mesh
 * position pos, as the reference's global_pass calls it cell by cell (evolve.F90:477-484): applies the
 * collected rates, adds 1 to *conv_flag when the cell has not converged.  c2r_global_pass is the whole pass. */
int c2r_evolve0d_global(c2r_ctx *ctx, double dt, const int pos[3], int *conv_flag);

/* minval(xh(:,:,:,0)), minval(xhe(:,:,:,0)) of the grids `which` selects as in c2r_fraction_means: the
 * "min xh_av / min xhe_av" log lines of global_pass (evolve.F90:463-466) want which = 2. */
int c2r_fraction_minima(c2r_ctx *ctx, int which, double out2[2]);

/* The numerical and algorithmic parameters that are COMPILED INTO the device code, for a host to compare with
 * the modules it was built with (c2ray_parameters.f90, abundances.f90, radiation_sizes.f90) before the first
 * step -- linking, say, c2ray_parameters_TEST4.f90 (subboxsize = mesh(1)) must stop the run, not silently
 * trace other sub-boxes.  out[0..]: subboxsize, max_subbox, abu_he, abu_c, epsilon, convergence_fraction,
 * minimum_fractional_change, minimum_fraction_of_atoms, relative_denergy, minitemp, NumTau, minlogtau,
 * maxlogtau, NumFreqBnd, NumheatBin.  Returns how many there are (15). */
int c2r_get_constants(double *out, int capacity);

/* Most sources swept by one batch of launches (1..4096; default 256).  Their column blocks come out of a
 * scratch arena (6 shell-ordered arrays per source, sized by the sub-boxes the source needed in the last
 * pass); a batch is cut short when the arena cannot hold it. */
int c2r_set_batch(c2r_ctx *ctx, int nbatch);

/* Mesh boundaries of the ray trace: periodic != 0 (the default; what the reference runs, evolve_data.F90:27-28
 * "has to be true for this version") or periodic == 0, OPEN: nothing wraps, photons that reach a mesh face leave the
 * box and are counted as lost.  Open boundaries follow the reference's own, dead, else branch of
 * evolve_source.F90:103-109: the reach of a source is per source and per axis, lastpos_l = max(srcpos - max_subbox, 1),
 * lastpos_r = min(srcpos + max_subbox, mesh); the box of round nbox (:143-144) is cut at that reach, so it differs from
 * source to source; a cell of a box lies at srcpos + offset, no modulo.  Everything per cell (cinterp, coldens,
 * photoion_rates, vol_ph, the LLS fog) is unchanged.
 * ONE DEPARTURE from that source text: the while-test of :136-139 looks at z only, and at both sides at once -- without
 * periodicity a source on the plane k = 1 would never start its first round, and a source three cells from a face
 * would be driven across the whole mesh by photons that leave through that face whatever its box does.  In open mode
 * there are therefore two sums over the surface cells of a box (evolve_point.F90:310-315) where the periodic code has
 * one:
 *   the loss that DECIDES: photo_out*vol/vol_ph over the surface cells on a face still short of the source's reach;
 *     the loop goes on while it exceeds 1e-10 * total_source_flux and at least one of the six faces can still move;
 *   the loss that is KEPT (photon_loss(1)): the same terms over the whole surface of the final box, mesh faces included.
 * With periodic boundaries every face can move until the limit, the two coincide, and nothing changes.
 * sum_nbox counts rounds as before.
 * Acts on every device of a multi-device context.  A switch forgets what earlier passes learnt about the sources
 * (sub-box counts, predicted column blocks, rounds swept without waiting for their loss).  Refused, with an error,
 * between c2r_pass_sources_begin and c2r_pass_sources_end.  c2r_pass_sources, c2r_pass_sources_begin, c2r_do_source,
 * c2r_evolve0d (whose cell must lie within the source's reach: inside the mesh), c2r_iteration, c2r_evolve3d,
 * c2r_pass_allreduce_chemistry and c2r_download_columns honour the mode.
 * Memory: the column block of a source holds the cells within its reach and nothing else, in a shell order cut at that
 * reach (csrc/c2ray_shell.hpp): prod_d(r_d - l_d + 1) <= N^3 cells of 48 bytes at the mesh limit wherever the source
 * sits -- 0.8 GB at N = 256, never more than a periodic block -- and a shell launch holds threads for the cells of the
 * cut shell only.  c2r_get_source_trace reports both per source. */
int c2r_set_boundaries(c2r_ctx *ctx, int periodic);
/* 1: periodic on all three axes, 0: open on all three, 2: mixed (c2r_set_boundaries_axes) */
int c2r_get_boundaries(const c2r_ctx *ctx);

/* Mesh boundaries per axis: periodic[d] != 0, axis d wraps; periodic[d] == 0, it is open.  All three non-zero is the
 * periodic mode above -- the same kernels, the same code path --, all three zero is the open mode, anything else is the
 * MIXED mode: a slab or a light-cone strip, periodic across the sky and open along the line of sight.
 * c2r_set_boundaries(ctx, p) means {p, p, p}.  The rules are those of c2r_set_boundaries: every device of a multi-device
 * context, refused between c2r_pass_sources_begin and c2r_pass_sources_end, a real change of mode forgets what earlier
 * passes learnt; the same entry points honour it (c2r_get_source_trace included), with heating and with three SEDs.
 * The mixed mode, per axis d of a source at srcpos:
 *   reach -- open axis, as in open mode: l = -min(max_subbox, srcpos - 1), r = min(max_subbox, mesh - srcpos);
 *     periodic axis, the then-branch of evolve_source.F90:103-109: l = -min(max_subbox, mesh/2),
 *     r = min(max_subbox, mesh/2 - 1 + mod(mesh,2)), the same for every source;
 *   a cell of a box lies at srcpos + offset, taken modulo the mesh on a periodic axis and as it is on an open one;
 *     cinterp works on the unwrapped offsets, as it always did;
 *   box growth and the two loss sums follow the OPEN mode's rule on all six faces, periodic axes included: the loss that
 *     decides runs over the surface cells on faces still short of their reach, the loop goes on while it exceeds
 *     1e-10 * total_source_flux and some face can still move, and the loss that is kept runs over the whole surface of the
 *     final box.
 * The reference's while-test, which looks at z only, and what follows from it -- a box whose z faces have arrived stops
 * growing along x and y too, and a mesh with (N/2 - 1) mod subboxsize == 0 stops one round short of its last -- belong to
 * the all-periodic path only.  A mixed run with z periodic therefore traces an open axis to its end where the all-periodic
 * code on a larger mesh would have stopped with z.
 * The column block of a source holds prod_d(r_d - l_d + 1) <= n1 n2 n3 cells, as in open mode. */
int c2r_set_boundaries_axes(c2r_ctx *ctx, const int periodic[3]);
/* out[d] = 1: axis d is periodic, 0: open */
int c2r_get_boundaries_axes(const c2r_ctx *ctx, int out[3]);

/* Plane-parallel sources: a plane wave that enters the mesh through an OPEN face and travels along one axis -- a slab lit
 * from outside, or slabs stacked along the line of sight that hand radiation to each other.  Axis-aligned incidence (a tilt:
 * c2r_set_plane_tilt below), one uniform flux per plane (a flux per face cell: c2r_set_plane_flux_map below).  A plane is not a many-source approximation: every line of cells along the axis is a 1-D
 * problem of its own, without cinterp (the incoming columns of a cell are the outgoing columns of the cell before it)
 * and without 1/r^2 dilution; everything per cell is what a point source gets (csrc/c2ray_plane.hpp).
 *   axis       0, 1 or 2: the axis the photons travel along; it must be open (c2r_set_boundaries_axes)
 *   from_high  0: they enter through the face at index 1 and travel towards index mesh[axis]; 1: the other way
 *   normflux   NormFlux of c2r_set_sources PER CM^2 OF FACE, one value per SED (black body, power law, quasar-like);
 *              S_star / pl_S_star / qpl_S_star stay those of c2r_set_sources / c2r_set_sources_sed.  A non-zero
 *              normflux[1] / [2] needs that SED's tables (c2r_set_sed_tables).
 * For every column (the two other indices fixed), in travel order, with q the cell, path = dr[axis]:
 *   N_in of the first cell = its entry column (0 unless set below), of every other cell N_out of the cell before;
 *   with LLS in force N_in(HI) = N_in(HI) + coldensh_LLS*path/dr(1), in every cell;
 *   N_out = N_in + max(x_av(q), epsilon)*ndens(q)*path*abundance (coldens, from the left);
 *   if N_in(HI) < max_coldensh: photoion_rates with these columns, vol_ph = dr[axis] (NormFlux*A photons per second are
 *   absorbed in the volume A*dr[axis]), the plane's flux and the cell's secondary-ionisation parameters, and
 *   phih += photo_HI / (x_av*ndens*(1-abu_he)), phihe likewise, phiheat += heat (evolve_point.F90:288-306);
 *   after the last cell the column adds photo_out*vol/dr[axis] to photon_loss(1) (0 beyond max_coldensh).  sum_nbox is
 *   not touched.  The sum over the columns has a fixed order: the same bits every time.
 * Plane p (1-based) is "source NumSrc + p" of the static deal: c2r_pass_sources(first, stride), its slab-wise form, the
 * per-device deal of a multi-device context, c2r_pass_allreduce_chemistry, c2r_iteration and c2r_evolve3d (whose
 * convergence criterion counts a plane as a source) give it to exactly one caller, and c2r_do_source(NumSrc + p) runs it.
 * The planes a caller owns are added before its point sources, in plane order.
 * Several planes: any mix of plain, tilted and mapped planes may share a list, and two planes may enter through the SAME face
 * (nothing refuses it): the rate grids and the far face's escape map receive each of them, in plane order, and every plane keeps
 * its own exit columns, exit flux and c2r_get_plane_loss.  The planes of a pass run one after another on scratch they share,
 * sized for the largest face of the list.  A tilt, a map and entry columns belong to the plane number they were set for.
 * c2r_set_plane_sources replaces the list (nplane = 0 removes it; at most 6) on every device of a multi-device context
 * and allocates what the planes need: 3 doubles per cell and two face buffers per plane.  It is refused for a plane
 * along a periodic axis, a bad axis, and between c2r_pass_sources_begin and c2r_pass_sources_end; c2r_set_boundaries*
 * refuses to make a plane's axis periodic while planes are set.  c2r_set_sources leaves the planes alone.
 * c2r_evolve0d and c2r_get_source_trace do not know planes. */
typedef struct {
  int axis;
  int from_high;
  double normflux[3];
} c2r_plane_source;
int c2r_set_plane_sources(c2r_ctx *ctx, int nplane, const c2r_plane_source *planes);
int c2r_get_plane_count(const c2r_ctx *ctx);
/* Entry columns of plane `plane` (1-based): (HI, HeI, HeII) x the face, the face cells in mesh order of the two remaining
 * axes (the lower axis fastest), species slowest -- what a slab upstream handed over.  NULL: zero again. */
int c2r_set_plane_entry_columns(c2r_ctx *ctx, int plane, const double *cols3);
/* The outgoing columns of the last cell of every column, same layout, from the last pass that ran the plane: the entry
 * columns of the next slab downstream. */
int c2r_download_plane_exit_columns(c2r_ctx *ctx, int plane, double *cols3);
/* What the plane added to photon_loss(1) in the last pass that ran it.  While no pass of this context has run the plane --
 * before the first pass, or because the deal gives it to another caller -- the loss is 0 and the exit columns are 0. */
int c2r_get_plane_loss(c2r_ctx *ctx, int plane, double *loss);

/* Oblique incidence: a tilt per plane, by short characteristics.  tilt[0] and tilt[1] are the tangents, in physical
 * lengths, of the beam's inclination towards the two face axes f < g (the two axes that are not the plane's axis):
 * travelling D along the axis in its travel direction (towards higher index for from_high = 0, towards lower index
 * otherwise) a photon moves tilt[0]*D along +f and tilt[1]*D along +g.  c2r_set_plane_sources sets every plane's tilt to
 * {0, 0}; tilt = NULL or {0, 0} returns plane `plane` (1-based) to normal incidence, which is the march above, unchanged
 * and with the same bits (the interpolation below is never used then: it would give c*w/w instead of c).  The tilt
 * applies to every device of a multi-device context.
 * Geometry of a tilted plane, host doubles formed once per pass from the dr of that pass:
 *   a_f = (|tilt[0]| * dr[axis]) / dr[f]       a_g = (|tilt[1]| * dr[axis]) / dr[g]     (cells moved sideways per layer)
 *   s_1 = a_f * a_g   s_2 = (1.0 - a_f) * a_g   s_3 = a_f * (1.0 - a_g)   s_4 = (1.0 - a_f) * (1.0 - a_g)
 *   path = dr[axis] * sqrt(1.0 + (tilt[0]*tilt[0] + tilt[1]*tilt[1]))
 *   e_f = +1 if tilt[0] > 0 else -1, e_g likewise                              (the upstream neighbour lies at index - e)
 * -- cinterp's weights s1..s4 (column_density.f90:116-122) for a source at infinity, where they are the same for every
 * cell: s_4 belongs to the cell straight behind, s_3 to the one displaced along f only, s_2 to the one displaced along g
 * only, s_1 to the diagonal one (the reference's corners c1..c4 with i -> f, j -> g).
 * The march.  For layer m = 0 .. mesh[axis]-1 in travel order and every face cell (u, v) of it (u along f, v along g):
 *   1. the four upstream cells c1..c4 are (u - e_f, v - e_g), (u, v - e_g), (u - e_f, v), (u, v): for m > 0 cells of
 *      layer m - 1 with that layer's outgoing columns, for m = 0 cells of the plane's entry columns (zero when not set);
 *   2. an index outside 1..mesh along a face axis wraps where that axis is periodic; where it is open that corner's three
 *      columns are 0 (the ray came in through the side of the mesh, and outside is empty) unless a side-entry strip of that
 *      side has been set (c2r_set_plane_side_entry below);
 *   3. per species, sig = sigma_HI / HeI / HeII at the species' threshold as weightf takes them for point sources:
 *        w_i = s_i * (1.0 / max(0.6, c_i*sig)),   N_in = (c1*w1 + c2*w2 + c3*w3 + c4*w4) / (w1 + w2 + w3 + w4),
 *      the sums from the left; no factor sqrt2 / sqrt3 (that belongs to cells adjacent to a source);
 *   4. from here on the normal plane's cell with this N_in, this path and vol_ph = path: the LLS fog
 *      coldensh_LLS*path/dr(1), N_out = N_in + max(x_av, epsilon)*ndens*path*abundance, the max_coldensh guard,
 *      photoion_rates.  A beam of normflux photons per cm^2 PERPENDICULAR TO ITSELF puts normflux*cos(theta)*A photons
 *      into a column of volume A*dr[axis], and dr[axis]/cos(theta) = path: normflux of a tilted plane is per cm^2
 *      perpendicular to the beam;
 *   5. the exit columns are the outgoing columns of the last layer; the loss term of a line is photo_out*vol/path of its
 *      last cell, added to photon_loss(1), to c2r_get_plane_loss and to the escape map of the far face at the line's face
 *      cell exactly as for the normal plane.  What crosses an open SIDE face, in or out, is in no loss and no map unless
 *      c2r_enable_plane_side_loss (below) is on; without it the loss identity of the escape maps holds for a tilted plane
 *      only when the tilted face axes are periodic.
 * Two slabs stacked along the axis with the same tilt, the upstream slab's exit columns given to the downstream slab as
 * entry columns, reproduce one mesh of the combined depth bit for bit.
 * Refused, each with an error text: a non-finite tilt; a_f > 1 or a_g > 1 with the current dr (the axis would no longer be
 * the dominant one, cinterp's own case split); a bad plane number; a call between c2r_pass_sources_begin and
 * c2r_pass_sources_end.  A pass refuses a tilted plane whose a has grown beyond 1 because dr changed since the tilt was
 * set.  c2r_set_boundaries* may change the face axes of a tilted plane at any time: the next pass takes the new wrap.
 * The first tilted plane allocates two buffers of 3 x face doubles; every layer is one kernel launch. */
int c2r_set_plane_tilt(c2r_ctx *ctx, int plane, const double tilt[2]);
int c2r_get_plane_tilt(const c2r_ctx *ctx, int plane, double tilt[2]);

/* Flux maps: the flux of a plane as a field over its face instead of one number per SED -- a finite beam, a patchy
 * background, or what the slab upstream let through.
 * flux3: 3 x face doubles, SED slowest (black body, power law, quasar-like), the face cells in the order of
 * c2r_set_plane_entry_columns.  While a map is set it REPLACES normflux[] of that plane: entry [k][f] is NormFlux per cm^2
 * for SED k at face cell f -- per cm^2 of face at normal incidence, per cm^2 perpendicular to the beam for a tilted plane,
 * as normflux is; S_star and its kin stay those of the point sources.  The map lives where the entry columns live, one
 * layer in front of the first.  flux3 = NULL: the plane's uniform normflux again.
 *   Normal incidence.  Every cell of line f uses nf[k] = map[k][f].  The plane takes the three-SED routine iff some entry
 *     of SED 1 or 2 of the map is non-zero (scanned when the map is set); every cell then gets its own triple through that
 *     routine, zeros included.
 *   Tilted plane.  The flux travels with the beam by the geometric weights of the tilt, without the optical-depth factor
 *     of the columns: for layer m and face cell (u, v), with the corners c1..c4 exactly as step 1 and 2 of the tilted
 *     march pick them,
 *        F[k] = F1[k]*s_1 + F2[k]*s_2 + F3[k]*s_3 + F4[k]*s_4,
 *     every product rounded, the sums from the left; Fi is the flux of that corner in the layer before, for m = 0 the map
 *     itself.  A corner outside an OPEN side face carries flux 0 (a map describes a finite beam: no flux enters through
 *     the side of the mesh) unless a side-entry flux strip of that side has been set; a periodic face axis wraps, and the face total is then conserved up to rounding (exactly,
 *     where the products are exact).  The cell (u, v) of layer m uses nf = F.
 *   Dark cells.  A cell whose three fluxes are all == 0.0 adds nothing to any rate grid, and its line's loss term is 0.0:
 *     it is skipped, no per-cell function is evaluated.  Everything else about a cell -- fog, columns, max_coldensh guard,
 *     denominators, vol_ph = path, loss term photo_out*vol/path, the escape map of the far face -- is the existing plane's
 *     cell with this nf.
 *   The exit flux (c2r_download_plane_exit_flux) is the flux the cells of the LAST layer saw in the last pass that ran the
 *     plane, in the map's layout: at normal incidence the map itself.  It is the flux map of the next slab downstream.
 * Identities.  At normal incidence a map whose every entry equals normflux[k] gives the uniform plane's bits in every grid,
 * exit column, loss and escape map.  For a tilted plane the same holds only to rounding: s_1 + s_2 + s_3 + s_4 is not
 * exactly 1.  Two slabs stacked along the axis with the same tilt reproduce one mesh of the combined depth bit for bit
 * when the upstream slab's exit columns AND its exit flux are handed downstream.
 * Refused, each with an error text: a bad plane number; a negative or non-finite entry; a non-zero entry of SED 1 or 2
 * without that SED's tables; a call between c2r_pass_sources_begin and c2r_pass_sources_end;
 * c2r_download_plane_exit_flux before any pass ran the plane with a map.  c2r_set_plane_sources replaces the list and drops
 * every map; c2r_set_boundaries* keep them, as they keep the tilts.  The calls act on every device of a multi-device
 * context, and every route that runs a plane honours the map.  A plane without a map runs the kernels it ran before maps
 * existed, with the same bits.  The first map of a plane allocates two buffers of 3 x face doubles; a plane with both a
 * tilt and a map needs two more and 3 doubles per cell, allocated by whichever of the two calls comes second. */
int c2r_set_plane_flux_map(c2r_ctx *ctx, int plane, const double *flux3);
int c2r_get_plane_flux_map_set(const c2r_ctx *ctx, int plane);          /* 1 / 0 */
int c2r_download_plane_exit_flux(c2r_ctx *ctx, int plane, double *flux3);

/* Plane light curves: a flux factor per shell of depth along a plane's beam, per plane.  What c2r_set_source_curves is to a
 * point source: a layer at depth d along the beam sees the plane at the retarded time t - d/c, and a stack of slabs that hand
 * their exit columns on models a light-cone strip many light-crossing times long.  A host that knows the history of what
 * shines through the face (a distant quasar that flickers, switches on or has switched off; a background that ramps up) hands
 * it over as a piecewise-constant curve, depth[k] = c*(t - t_k) and factor = F(t_k)/F(t).  A depth horizon is the crudest such
 * curve: {1, layer0, depth0, {D}, {1, 0}}.
 *   nstep     the number of steps, 0 .. C2R_PLANE_CURVE_MAX_STEPS
 *   layer0    >= 0: the layers of this plane's path the beam crossed before it entered this mesh (the layers of the slabs
 *             upstream, where they share the tilt and the cell size)
 *   depth0    finite, >= 0: a length the beam travelled before that, in the length unit of dr
 *   depth     depth[0..nstep-1]: lengths along the beam in the length unit of dr, finite, >= 0 and strictly ascending
 *   factor    factor[0..nstep]: finite and >= 0; factor[b] holds in depth shell b.  The shells are [0, depth[0]],
 *             (depth[0], depth[1]], ..., (depth[nstep-1], infinity)
 * Entries behind nstep (depth) and nstep + 1 (factor) mean nothing and are not looked at.
 * The rule (csrc/c2ray_pcurve.hpp).  For layer m = 0 .. mesh[axis]-1 in travel order and the per-layer path of the pass --
 * dr[axis] at normal incidence, dr[axis]*sqrt(1 + tilt[0]^2 + tilt[1]^2) as the tilted march forms it, from the dr of that
 * pass -- every operation rounded as written, no fused multiply-add:
 *     d = depth0 + ((double)(layer0 + m) + 0.5) * path
 *     b = the number of k < nstep with d > depth[k]
 *     f = factor[b]
 * No square root and no division: a layer whose centre lies exactly on a depth belongs to the nearer shell.  f is uniform
 * over a layer.
 * A cell of a layer with f == 0.0 is UNLIT: it adds nothing to phih, phihe or phiheat and no per-cell routine runs for it; if
 * it lies in the last layer its line's loss term is 0.0, in photon_loss(1), in c2r_get_plane_loss and in the far face's escape
 * map.  Any other cell is the plane's cell in every respect but one: nf[k]*f takes the place of nf[k], one rounded product per
 * SED, where nf is whatever the cell uses without a curve -- the plane's normflux, the map entry of its line, or the flux the
 * tilted march carried to the cell.  The exit term of a line uses the last layer's f in the same way.  A cell is skipped iff
 * its unscaled fluxes are dark (all three == 0.0) or f == 0.0; whether the plane takes the three-SED routine is decided from
 * the unscaled fluxes, as without a curve.
 * What a curve does not touch.  The march, the fog, the columns, the exit columns and the max_coldensh guard; vol_ph = path;
 * the flux a tilted plane with a map carries from layer to layer, and c2r_download_plane_exit_flux, which stays the UNSCALED
 * flux of the last layer (the slab downstream applies its own curve, with its own layer0 / depth0); sum_nbox and the deal of
 * planes to callers.  Nothing is rescaled to conserve anything.
 * Identities.
 *   Off: with no curve set every grid, loss, map and exit buffer has the bits it had before curves existed, from the same
 *     kernel launches.
 *   All factors 1.0: the same bits, through the curved kernels.
 *   Step to zero: {1, .., {D}, {1, 0}} is a depth horizon -- layers within D have the uncurved bits, layers beyond have rates
 *     of exactly zero, and the loss is exactly 0.0 when the last layer lies beyond D.
 *   A factor 2^n scales the rates and the loss terms of its layers exactly.
 *   Stacking: an upstream slab of n_a layers and a downstream slab with layer0 larger by n_a, the same tilt and the same
 *     path, the exit columns handed on (and the exit flux, where the plane has a map), reproduce one mesh of the combined
 *     depth bit for bit.
 * c2r_set_plane_curve gives plane `plane` (1-based) its curve; curve = NULL, or a record with nstep == 0 and factor[0] == 1.0:
 * the plane has no curve.  c2r_set_plane_sources drops every curve; c2r_set_plane_tilt, c2r_set_plane_flux_map,
 * c2r_set_plane_entry_columns, c2r_set_boundaries* and c2r_set_sources keep them.  The calls act on every device of a
 * multi-device context, and every route that runs a plane honours the curve: c2r_pass_sources and its slab-wise form,
 * c2r_do_source(NumSrc + p), c2r_pass_allreduce_chemistry, c2r_iteration, c2r_evolve3d.  Setting a curve allocates nothing.
 * Refused, each with an error text: a bad plane number; a call between c2r_pass_sources_begin and c2r_pass_sources_end; an
 * nstep outside 0..C2R_PLANE_CURVE_MAX_STEPS; a negative layer0; a negative or non-finite depth0; a depth that is negative,
 * not finite or not above its predecessor; a factor that is negative or not finite; and the ZEROED RECORD (nstep == 0 and
 * factor[0] == 0.0), for the reasons c2r_set_source_curves gives: a plane that has gone dark is {1, .., {0.0}, {0.0, 0.0}}.  A
 * refused call changes nothing.
 * c2r_get_plane_curve returns the curve of the plane as it was set, the entries behind its steps zeroed, and {0, 0, 0.0, {},
 * {1.0}} while none is set; a bad plane number is refused with an error text. */
#define C2R_PLANE_CURVE_MAX_STEPS 8
typedef struct {
  int nstep;
  int layer0;
  double depth0;
  double depth[C2R_PLANE_CURVE_MAX_STEPS];
  double factor[C2R_PLANE_CURVE_MAX_STEPS + 1];
} c2r_plane_curve;
int c2r_set_plane_curve(c2r_ctx *ctx, int plane, const c2r_plane_curve *curve);
int c2r_get_plane_curve(const c2r_ctx *ctx, int plane, c2r_plane_curve *out);

/* Side faces of a tilted plane: hand-over to the mesh that stands beside this one, and the loss through open side faces.
 * Notation: the plane travels along axis a; the face axes are f < g with extents fa, fb; na = mesh[a] layers m = 0 .. na-1 in
 * travel order; s_1..s_4, e_f, e_g and path are those of the tilted march above.  SIDE 0 is face axis f, SIDE 1 face axis g;
 * L_0 = fb and L_1 = fa are the lengths of a side's lines.  A side is LIVE in a pass iff its tilt component is non-zero and
 * its axis is open in that pass.  The upstream ghost index of a live side is -1 for e = +1 and n for e = -1 (where step 2
 * of the march finds a corner outside); its DOWNSTREAM EDGE is the cell index n-1 for e = +1 and 0 for e = -1.
 * All three parts are per plane; c2r_set_plane_sources drops them, c2r_set_plane_tilt, c2r_set_plane_flux_map,
 * c2r_set_plane_curve, c2r_set_plane_entry_columns, c2r_set_boundaries* and c2r_set_sources keep them; they are refused
 * between c2r_pass_sources_begin and c2r_pass_sources_end, act on every device of a multi-device context, and every route that
 * runs a plane honours them.  A plane that uses none of them runs the kernels it ran before, with the same bits.
 *
 * 1. Side entry: what a neighbouring mesh hands in.  side = 0, 1, or 2 for the corner line.  A strip has na SLOTS; slot m
 *    holds the ghost cells of the layer BEFORE layer m: for m = 0 the entry layer in front of the mesh (where the entry
 *    columns and the map live), for m >= 1 layer m-1.  Sides 0 and 1: cols[(m*3 + k)*L_s + t], k the species (HI, HeI, HeII),
 *    t the 0-based index along the OTHER face axis; flux has the same layout with k the SED.  The corner line (side 2):
 *    cols[m*3 + k] and flux[m*3 + k].  cols = NULL clears that side (flux must then be NULL too); flux = NULL with cols given
 *    is a ghost flux of 0.
 *    Steps 1-2 of the tilted march change in one place only: where a corner index falls outside an OPEN face axis on a LIVE
 *    side (an index that wraps still wraps).  Outside along f only: side 0's strip, slot m, at the corner's own index along g
 *    (after any wrap); outside along g only: side 1's strip, slot m, at the corner's own index along f; outside along both:
 *    the corner line, slot m; a strip that is not set: 0.0, as before.  The ghost values go through the weighted mean of step
 *    3 and the flux rule of c2r_set_plane_flux_map as in-mesh corners do.  The flux strips are read only while the plane has a
 *    map (a uniform plane's flux is normflux everywhere, ghost or not).  A strip of a side that is not live in a pass is kept
 *    and not read.  The plane takes the three-SED routine iff some entry of SED 1 or 2 of the map, or of a set side-entry flux
 *    strip, is non-zero.
 *    Refused, each with an error text and leaving everything unchanged: a bad plane or side; flux without cols; a negative or
 *    non-finite flux entry; a non-zero flux of SED 1 or 2 without that SED's tables.  Columns are taken as given.
 * 2. Side exit: what this mesh hands on.  c2r_enable_plane_side_exit allocates (on != 0) or frees the strips of a plane;
 *    c2r_download_plane_side_exit (side 0 or 1) fills the layout above from the last pass that ran the plane, for the
 *    downstream edge cells of a live side: slot m at t is the value of the layer before layer m at the edge cell whose other
 *    index is t -- slot 0 the plane's entry columns there (0 when none) and the map there, slot m >= 1 the outgoing columns
 *    of layer m-1 and the flux that cell saw (unscaled by any curve, as the exit flux is).  Each value is the corner c4 / F4
 *    the edge cell of layer m loads.  The last layer's edge is in no strip: it is in the exit columns and the exit flux, which
 *    a slab stacked downstream takes its slot 0 from.  flux must be NULL for a plane without a map.  The downstream corner
 *    cell is in both strips: a diagonal neighbour's corner line is read out of either.
 *    Refused: before any pass ran the plane with the strips enabled; a side that was not live in that pass; a non-NULL flux
 *    without a map.
 *    Hand-over identity.  Let mesh B be the downstream neighbour of mesh A along a face axis, with the same tilt, cell sizes
 *    and plane record (a curve shared with its layer0 and depth0).  With A's side exit given to B as side entry, and B's
 *    corner line taken from the diagonal neighbour's strip, B reproduces its part of one mesh of the combined width (open
 *    along that axis) bit for bit -- incoming columns, rate grids, exit columns, exit flux, per-line far-face terms -- and A
 *    reproduces its own part unaided, since the beam never comes back.
 * 3. Side loss: closing the photon budget.  Off by default; while off nothing is allocated, launched or added.  The rule
 *    (csrc/c2ray_pside.hpp) covers a tilted plane in a pass, every layer m = 0 .. na-2 and every cell (u, v) of it (the last
 *    layer gives its whole term to the far face).  The cell hands its outgoing beam to three displaced targets in layer m+1:
 *    (u+e_f, v+e_g) with weight s_1, (u, v+e_g) with s_2, (u+e_f, v) with s_3.  A target's index wraps on a periodic face
 *    axis; a target that then lies outside the mesh gives its weight to one side: outside along f only, side 0; outside along
 *    g only, side 1; outside along both, side 0 (the lowest axis, the escape maps' tie rule).  So w_0 = s_3 + s_1, and
 *    w_1 = s_2 + s_1, or s_2 alone on the line where side 0 takes the diagonal -- host doubles, one rounded sum each; only
 *    cells on a live side's downstream edge have a non-zero weight.  The term of a cell for side s is base * w_s, one rounded
 *    product, where base is photo_out*vol/path of that cell from its own incoming and outgoing columns and the flux it used
 *    (uniform, or the carried flux of a mapped plane, times the curve factor of layer m where the plane has a curve); base is
 *    0.0 for a dark cell, an unlit cell and where N_in(HI) >= max_coldensh.  A side's terms are added in the fixed order of
 *    the other loss sums (blocks of 256 by a tree, the block sums in order), the cells in the order of the side face's map.
 *    While enabled the sums go into photon_loss(1) (behind the plane's far loss: side 0, then side 1), into
 *    c2r_get_plane_side_loss (out2[0], out2[1]: the last pass that ran the plane) and, with c2r_enable_face_loss on, into the
 *    escape map of the side face the beam leaves through, 2*axis + (e > 0), at the edge cell's face cell, map = map + term, the
 *    planes in plane order.  c2r_get_plane_loss stays the far face's alone.  A plane at normal incidence, or with no live
 *    side, loses nothing through sides. */
int c2r_set_plane_side_entry(c2r_ctx *ctx, int plane, int side, const double *cols, const double *flux);
int c2r_enable_plane_side_exit(c2r_ctx *ctx, int plane, int on);
int c2r_download_plane_side_exit(c2r_ctx *ctx, int plane, int side, double *cols, double *flux);
int c2r_enable_plane_side_loss(c2r_ctx *ctx, int on);
int c2r_get_plane_side_loss_enabled(const c2r_ctx *ctx);                /* 1 / 0 */
int c2r_get_plane_side_loss(c2r_ctx *ctx, int plane, double out2[2]);

/* Escape maps: WHERE the photons that photon_loss(1) counts left an open box -- the kept loss per cell of the open mesh
 * face it leaves through.  Off by default; with it off nothing is allocated, launched or waited for.
 * Faces: face = 2*axis + high, axis 0, 1, 2; high = 0 is the face at mesh index 1, high = 1 the one at index mesh[axis].
 * Only faces of an OPEN axis have a map: one double per face cell, the face cells in mesh order of the two remaining
 * axes, the lower axis fastest (the layout of c2r_set_plane_entry_columns without the species index).
 * Point sources.  For every point source s a pass sweeps and every cell q of its FINAL sub-box, with o the cell's offset
 * from the source and m_d = srcpos_d + o_d its mesh index along an open axis d:
 *   the cell's candidate faces are (d, low) for every open d with m_d == 1 and (d, high) for every open d with
 *   m_d == mesh_d; a cell without candidate adds nothing;
 *   a cell with several candidates (mesh edges and corners) gives its whole term to exactly one: the candidate whose
 *   axis has the largest |o_d|*dr_d (compared as doubles, the product as written) -- the face the ray from the source
 *   leaves through --, on a tie the lowest axis, within one axis (a mesh one cell deep) low before high;
 *   the term is the one that enters the kept loss of open mode, photo_out*vol/vol_ph (vol_ph = 4 pi dist^2 path, the
 *   cell volume for the source's own cell), 0 where N_in(HI) >= max_coldensh: the same bits the pass adds into
 *   photon_loss(1) for that cell, from the same device functions (LLS fog, three SEDs and heating runs included).
 *   A cell of the final box on a mesh face of an open axis always lies on the box's surface.
 * Planes.  The per-line term of a plane (step 7 above) goes to the far face of its axis, high = 1 - from_high, at the
 * line's face cell.
 * Order.  Per face cell map = map + term in the order in which a pass adds to the rate grids: the planes the caller owns
 * first, in plane order, then its point sources in source order, across batches.  No float atomics: the same bits on
 * every run and for every c2r_set_batch.
 * Lifetime: that of photon_loss.  c2r_set_rates_to_zero clears the maps; every pass adds to them -- c2r_pass_sources, its
 * slab-wise form (complete after c2r_pass_sources_end), c2r_do_source, c2r_pass_allreduce_chemistry, c2r_iteration,
 * c2r_evolve3d (after which they hold the last iteration's pass).  c2r_evolve0d does not know them.
 * Several devices and ranks.  The maps are NOT part of the reduction buffer (c2r_rates_count and its layout are what
 * they were).  On a multi-device context a download returns the sum of the devices' maps, added in device order.  Across
 * processes the maps hold this rank's sources only; adding them over the ranks is the host's business.
 * Identities.  The sum of all maps is the part of the kept loss that comes from cells on open mesh faces, so it is
 * <= photon_loss(1) up to rounding; it equals photon_loss(1) to rounding when all axes are open and every source's final
 * box is its whole reach; in a mixed mode the faces of a periodic axis at +-N/2 count in photon_loss(1) and in no map.
 *
 * c2r_enable_face_loss allocates (on != 0) or frees the maps of the open faces on every device of the context; it is
 * refused between c2r_pass_sources_begin and c2r_pass_sources_end.  A later change of boundary mode re-sizes the maps and
 * zeroes them. */
int c2r_enable_face_loss(c2r_ctx *ctx, int on);
int c2r_get_face_loss_enabled(const c2r_ctx *ctx);
/* The map of `face`.  An error for a face of a periodic axis, for a face outside 0..5, while the feature is off, and
 * while a slab-wise pass is open. */
int c2r_download_face_loss(c2r_ctx *ctx, int face, double *map);
/* out6[face]: the sum of that face's map (0 for a face of a periodic axis) in a fixed order -- every 256 consecutive face
 * cells by a tree, then the block sums in order, the shape of the device's loss sums (face_sum, csrc/c2ray_face.hpp). */
int c2r_get_face_loss(c2r_ctx *ctx, double out6[6]);

/* ---- several GPUs: sources over ranks and the sum over ranks ----------------------------------------
 * The reference's MPI strategy (master_slave.F90:74-96 do_grid_static, evolve.F90:505-548
 * mpi_accumulate_grid_quantities): every rank holds the full grid, rank r sweeps sources r+1, r+1+npr, ...,
 * six MPI_ALLREDUCE calls sum phih_grid, phihe_grid, phiheat, photon_loss and sum_nbox, every rank runs the
 * global pass.  Here a rank is a GPU and the six sums are one fp64 ncclAllReduce (RCCL over xGMI) of the
 * contiguous buffer above, device to device.
 *
 * One process per GPU (an MPI rank, a torch.distributed.run rank): c2r_create, then c2r_comm_init with the
 * 128-byte id that ONE rank obtained from c2r_comm_unique_id and the launcher passed to the others (MPI_Bcast,
 * a file, ...).  One process for several GPUs (the reference's no_mpi build): c2r_create_multi returns a
 * context that applies every state-setting call to all its devices, runs passes on one host thread per device
 * and reads results from the first; c2r_comm_init_local gives it its communicators (ncclCommInitAll).  The two
 * compose: c2r_comm_init on a multi-device context makes its devices ranks first_rank, first_rank+1, ...
 * RCCL is loaded on first use; single-GPU runs never touch it. */
int c2r_device_count(void);
int c2r_create_multi(c2r_ctx **out, int ndev, const int *devices, const int mesh[3]);
int c2r_num_devices(const c2r_ctx *ctx);
/* 0 when librccl can be loaded and reports the major version this library was compiled against (what
 * c2r_comm_unique_id / c2r_comm_init need); otherwise non-zero with the reason in c2r_create_error().  Lets every
 * rank of a launcher agree BEFORE the collective ncclCommInitRank whether the communicator can be made at all. */
int c2r_comm_available(void);
int c2r_comm_unique_id(char id[128]);
int c2r_comm_init(c2r_ctx *ctx, int first_rank, int nranks, const char id[128]);
int c2r_comm_init_local(c2r_ctx *ctx);
int c2r_comm_destroy(c2r_ctx *ctx);
int c2r_comm_rank(const c2r_ctx *ctx);
int c2r_comm_nranks(const c2r_ctx *ctx);
/* What carries the sum over ranks (MPI_ALLREDUCE in evolve.F90:505-548): 0 nothing (one rank, no communicator),
 * 1 RCCL (ncclAllReduce), 2 the in-process sum of replicas that share a device (rehearsal mode of
 * c2r_comm_init_local).  A harness reports c2r_comm_nranks as "ranks RCCL saw" only when this is 1. */
int c2r_comm_kind(const c2r_ctx *ctx);
/* Path of the library whose ncclAllReduce carries the sums (librccl.so.1 of the loader's path, or the file named by
 * the environment variable C2R_RCCL_LIBRARY), "" when none could be loaded (non-zero return, reason in
 * c2r_create_error()).  A harness prints it next to its result: a sum carried by anything but RCCL is not an RCCL result. */
int c2r_comm_library(char *out, int capacity);
/* Errors while a communicator is in use (the reference has none: its ranks log, go on and meet again at the next
 * MPI_ALLREDUCE, evolve.F90:177-181,523-538; its drop-in host ends the job with MPI_ABORT).  c2r_allreduce_rates,
 * c2r_pass_allreduce_chemistry, c2r_iteration and c2r_evolve3d ABORT the context's RCCL communicators (ncclCommAbort)
 * before they return an error: nothing of this process is left waiting in a sum that cannot complete, every later
 * collective call on the context fails at once, and the host is expected to exit non-zero so that its launcher ends the
 * other ranks.  A rank whose peer never issues its share of a sum does not wait for ever either: after
 * C2R_COMM_TIMEOUT_S seconds (environment; default 1800, 0 = no limit) its wait ends with an error and the same abort. */
/* mpi_accumulate_grid_quantities (evolve.F90:505-548) after c2r_pass_sources: the whole buffer in one
 * all-reduce; afterwards c2r_get_loss / c2r_download_rates return the summed photon_loss and sum_nbox_all.
 * A no-op on a single rank without communicator.  On a multi-device context c2r_pass_sources(first, stride)
 * gives device i the sources first + i*stride, first + i*stride + stride*ndev, ... */
int c2r_allreduce_rates(c2r_ctx *ctx);
/* One outer iteration's pass_all_sources + mpi_accumulate_grid_quantities + global_pass
 * (evolve.F90:185-217) with all three overlapped: the rates launch of the last batch is cut into nslab slabs
 * of k-planes, slab s is summed over the ranks while slab s+1 is computed, and its chemistry runs as soon as
 * its sum is complete.  conv_flag: non-converged cells (evolve.F90:488). */
int c2r_pass_allreduce_chemistry(c2r_ctx *ctx, int first, int stride, int nslab, double dt, int *conv_flag);

/* Self-test of the sum over ranks: a collective call (every rank of the communicator makes it, like
 * c2r_allreduce_rates).  A known pattern is summed through the context's own reduction buffer (the one given to
 * c2r_set_rates_buffer, if any), communicators, comm streams and events, by the routines the production calls use,
 * over both routes a run takes:
 *   route 0, as c2r_allreduce_rates: the whole buffer (c2r_rates_count doubles) in one all-reduce;
 *   route 1, as c2r_pass_allreduce_chemistry: nslab slabs of k-planes (an even split; production boundaries depend
 *            on the sources), each slab's 3 or 4 component ranges in one grouped launch, then the 48-double tail.
 * The pattern, for position i of the buffer and rank r (0-based) of n:
 *   h = splitmix64(i)   (z = i + 0x9E3779B97F4A7C15; z = (z ^ z>>30) * 0xBF58476D1CE4E5B9;
 *                        z = (z ^ z>>27) * 0x94D049BB133111EB; h = z ^ z>>31)
 *   a(i) = (2^29 + (h mod 2^29)) | 1      e(i) = ((h >> 32) mod 121) - 60
 *   v(r, i) = (r + 1) a(i) 2^e(i)         expected(i) = n (n + 1) / 2 a(i) 2^e(i)
 * Every partial sum is an integer below 2^53 times one power of two, so the sum is exact in every association for
 * n <= 4095 (more ranks are refused) and the check is == on the value.  a(i) is odd with 30 significant bits: a
 * transport that reduces through fp32 cannot produce it; a rank left out, added twice or left un-reduced changes
 * the sum by a non-zero multiple of a(i); a and e vary with i, so a range that lands at a wrong offset is seen.
 * WHAT A PASS PROVES: the sums the transport returned for this buffer, these offsets, these message sizes and this
 * grouping were exact, on this process's devices, at the time of the call.  WHAT IT DOES NOT: performance, corruption
 * that happens later, or anything about a transport it was not run on.  The verdict is local to the process (a wrong
 * transport need not be wrong on every rank); agreeing about it is the launcher's business.
 * Allowed wherever c2r_set_rates_to_zero is allowed, and on a context fresh from c2r_create + c2r_comm_init*; it has
 * c2r_set_rates_to_zero's effect on the rate grids, photon_loss / sum_nbox of c2r_get_loss stay what they were.
 * One-device context without communicator: returns 0 with ranks = 1 and nothing checked.  A mismatch or a transport
 * error: non-zero return, the report is filled in all the same, the error text names route, rank, device, index, got,
 * expected, the mismatch count and c2r_comm_library's path, and -- as after any other error inside a collective phase
 * -- the RCCL communicators of the context are aborted.  Both routes always run to their end (unless the transport
 * itself returns an error), so that no peer waits for a rank that gave up half-way.
 * Environment: C2R_COMM_SELFTEST=1 makes c2r_comm_init and c2r_comm_init_local run it (nslab from
 * C2R_ALLREDUCE_SLABS, default 4) once the communicators exist: a failure fails the init call with the self-test's
 * text and leaves the context without communicator, a pass prints one "comm self-test ok" line on stderr. */
typedef struct {
  int ranks, kind, devices;      /* c2r_comm_nranks, c2r_comm_kind, devices of this context that were checked */
  long long elements[2];         /* doubles summed and compared per device: [0] whole-buffer route, [1] slab-wise route */
  long long mismatches[2];       /* over all devices of this context */
  int bad_route, bad_rank;       /* the first mismatch: lowest route, then lowest rank, then lowest index; -1: none */
  long long bad_index;           /* position in the reduction buffer */
  double got, expected;
  double ms[2];                  /* per route, event-timed on the first device: fill queued -> check complete */
} c2r_comm_selftest_report;
int c2r_comm_selftest(c2r_ctx *ctx, int nslab, c2r_comm_selftest_report *report);

/* Timings of the sum over ranks of the last c2r_pass_allreduce_chemistry on device idev (0 .. c2r_num_devices-1),
 * filled only while c2r_enable_timing(ctx, 1) is on (all zero otherwise, and for a context without communicator).
 * allreduce_exposed_ms is what the sum costs the iteration: after a device's last slab of rates nothing of its own is
 * left to hide the wire behind but the chemistry of earlier slabs. */
typedef struct {
  int slabs;                    /* slabs of the last slab-wise pass on this device; 0: none yet, or no communicator */
  double allreduce_ms;          /* comm stream: first slab's sum released -> tail's sum complete */
  double allreduce_exposed_ms;  /* this device's LAST slab of rates complete (or the first sum released, if that came
                                   later: until then the device waited for the host, not the wire) -> that slab's sum complete */
  double tail_ms;               /* the 48-double tail's sum alone */
} c2r_comm_timing;
int c2r_get_comm_timing(c2r_ctx *ctx, int idev, c2r_comm_timing *out);

/* evolve0D(dt,rtpos,ns,niter) (files_for_3D/evolve_point.F90:79-319) for ONE cell, for hosts that drive the sweep
 * themselves, cell by cell, as the reference's do_source does through evolve2D / evolve1D_axis / evolve2D_plane /
 * evolve3D_quadrant (files_for_3D/evolve_source.F90:244-608): the incoming columns of the cell at mesh position rtpos
 * (1-based, not wrapped: rtpos - srcpos(:,ns) is the offset from the source) by short characteristics from the cells
 * of source ns done before it, its own columns, its photo-ionisation (and heating) rates added to the rate grids.
 * The caller keeps the order of the reference's sweeps (a cell after the cells it interpolates from) and the
 * reference's "already done" test (coldensh_out(pos) == 0): every cell of a source is given once.  A new (ns, niter)
 * pair starts a new source.  on_surface != 0: the cell lies on the surface of the caller's current sub-box
 * (evolve_point.F90:310-315); *loss then receives phi%photo_out * vol / vol_ph, for which the call waits for the
 * device -- all other calls only queue work.  One launch per cell: an interface for the reference's own loops, tests
 * and small meshes; c2r_do_source / c2r_pass_sources trace a source as a whole. */
int c2r_evolve0d(c2r_ctx *ctx, const int rtpos[3], int ns, int niter, int on_surface, double *loss);

/* One outer iteration of evolve3D after set_rates_to_zero (files_for_3D/evolve.F90:185-217): pass_all_sources for the
 * sources first, first + stride, ... (:385-431), mpi_accumulate_grid_quantities (:505-548; a no-op without a
 * communicator) and global_pass (:435-501) -- c2r_pass_allreduce_chemistry -- followed, in the same queue and
 * with ONE host synchronisation for all of it, by every grid reduction the reference's loop prints or feeds to
 * calculate_photon_statistics after a global pass (:463-466, :487-499; photonstatistics.f90:117-234).  The numbers
 * are those of the single-purpose entry points (same kernels' summation order):
 *   means_intermed  = c2r_fraction_means(ctx, 1, .)      sums_intermed = c2r_state_sums(ctx, 1, .)
 *   total_rates     = c2r_total_rates(ctx, dt, reccoef, .) with reccoef = c2r_get_reccoef(ctx, .)
 *   minima_av       = c2r_fraction_minima(ctx, 2, .) as the NEXT iteration's log lines "min xh_av" / "min xhe_av"
 *                     will want them (xh_av does not change between a global pass and the next one)
 *   photon_loss, sum_nbox = c2r_get_loss (summed over the ranks).
 * A host driver that follows the reference's loop line by line makes six calls with six synchronisations for this;
 * the Fortran drop-in (fortran/evolve.F90) uses this one unless an iteration dump is due. */
typedef struct {
  int conv_flag;
  int sum_nbox;
  double photon_loss[C2R_NFREQ];
  double means_intermed[5];
  double sums_intermed[5];
  double total_rates[3];
  double minima_av[2];
  double reccoef[12];
} c2r_iteration_report;
int c2r_iteration(c2r_ctx *ctx, int first, int stride, int nslab, double dt, c2r_iteration_report *report);

/* Timing of the last c2r_pass_sources / c2r_global_pass on the context's stream, measured with
 * HIP events on that stream: milliseconds spent in the column sweep launches, the rates kernel
 * and the chemistry kernel, and the number of launches of each. */
typedef struct {
  double sweep_ms, rates_ms, chem_ms;
  int sweep_launches, rates_launches, chem_launches;
  long long cells_swept; /* cell x source pairs actually traced by the last c2r_pass_sources */
} c2r_timing;
int c2r_get_timing(c2r_ctx *ctx, c2r_timing *out);
/* The column scratch (the reference's coldensh_out / coldenshe_out per source in flight, evolve_source.F90:94-95) since the
 * context was made: out[0] device segments allocated, out[1] of them INSIDE a pass (the others by c2r_begin_step, which sizes
 * the scratch of a time step from the sub-box counts the step before ended with), out[2] doubles allocated in all, out[3]
 * column blocks moved to deeper ones in the middle of a sweep, out[4] batches that started over for lack of room,
 * out[5] doubles held now. */
int c2r_arena_stats(const c2r_ctx *ctx, long long out[6]);
/* the same for device `idev` (0 .. c2r_num_devices-1) of a context made by c2r_create_multi */
int c2r_get_timing_device(c2r_ctx *ctx, int idev, c2r_timing *out);
/* What the last pass that swept source ns (1-based) did for it, from the host's bookkeeping (no device copy, no
 * synchronisation; every boundary mode).  reach_l <= 0 <= reach_r: how far the source's box can go per axis (the mesh's
 * reach along a periodic axis, the source's own along an open one); nbox: its rounds (0, with everything below 0, while
 * it has not been swept since the source list or the boundary mode was set); box_lo / box_hi: its final sub-box as
 * offsets from the source; block_shells: the shells its column block could hold at the end; block_cells: entries per
 * column array of that block -- (2 block_shells + 1)^3 periodic, the cells of those shells within the reach open;
 * swept_cells: cells of the final sub-box; sweep_threads: threads the shell launches of that pass spent on it, the
 * launches' x-extent times the block size summed over its shells.  A multi-device context answers from the device that
 * swept ns last. */
typedef struct {
  int reach_l[3], reach_r[3];
  int nbox;
  int box_lo[3], box_hi[3];
  int block_shells;
  long long block_cells;
  long long swept_cells;
  long long sweep_threads;
} c2r_source_trace;
int c2r_get_source_trace(c2r_ctx *ctx, int ns, c2r_source_trace *out);
int c2r_enable_timing(c2r_ctx *ctx, int on);

#ifdef __cplusplus
}
#endif
#endif
