// Point-source hand-over between meshes stacked along an open axis (include/c2ray_hip.h): the entry points of the exit
// strips (c2r_select_source_face_exit, c2r_download_source_face_exit) and of the entry columns (c2r_set_source_face_entry,
// c2r_get_source_face_entry; through several faces, across edges and corners: c2r_set_source_halo, c2r_get_source_halo) and of the mesh's place in a deep mesh (c2r_set_mesh_origin).  Included by c2ray_hip.hip, which has the kernels (k_source_face_exit, k_sweep_shell_entry,
// k_sweep_shell_fast_entry, k_loss_entry) and the pass's side of both (place_batch, sweep_batch, queue_source_face_exit).

// cells of a face of axis `axis`
static size_t handover_face_cells(const c2r_ctx *c, int axis) {
  const int mesh[3] = {c->g.n1, c->g.n2, c->g.n3};
  return c->g.ncell / (size_t)mesh[axis];
}

// ---------------------------------------------------------------------------------------------
// exit
static int select_source_face_exit_one(c2r_ctx *c, int face, int nsel, const int *sources) {
  if (!c) return 1;
  if (face < 0 || face > 5) return fail(c, "c2r_select_source_face_exit: face %d, expected 0..5 (2 * axis + high)", face);
  if (nsel < 0 || (nsel > 0 && !sources)) return fail(c, "c2r_select_source_face_exit: bad arguments");
  if (c->pass_open) return fail(c, "c2r_select_source_face_exit: a pass opened by c2r_pass_sources_begin is still open (close it with c2r_pass_sources_end first)");
  if (nsel > 0 && c->per[face >> 1])
    return fail(c, "c2r_select_source_face_exit: face %d belongs to axis %d, which is periodic (c2r_set_boundaries_axes opens an axis)", face, face >> 1);
  for (int k = 0; k < nsel; k++) {
    if (sources[k] < 1 || sources[k] > c->nsrc)
      return fail(c, "c2r_select_source_face_exit: source %d not in [1,%d]", sources[k], c->nsrc);
    for (int j = 0; j < k; j++)
      if (sources[j] == sources[k]) return fail(c, "c2r_select_source_face_exit: source %d is named twice", sources[k]);
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream)); // (nothing queued may still write the strips that go)
  c2r_ctx::FaceExit &x = c->face_exit[face];
  if (x.d_cols) HIPCHK(c, hipFree(x.d_cols));
  x = c2r_ctx::FaceExit();
  if (nsel == 0) return 0;
  const size_t n = 3 * handover_face_cells(c, face >> 1) * (size_t)nsel;
  HIPCHK(c, hipMalloc(&x.d_cols, sizeof(double) * n));
  HIPCHK(c, zero_device(x.d_cols, sizeof(double) * n, c->stream));
  x.sources.assign(sources, sources + nsel);
  x.rounds.assign((size_t)nsel, 0);
  x.reached.assign((size_t)nsel, 0);
  x.stamp.assign((size_t)nsel, 0);
  return 0;
}
extern "C" int c2r_select_source_face_exit(c2r_ctx *c, int face, int nsel, const int *sources) {
  if (int e_ = select_source_face_exit_one(c, face, nsel, sources)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return select_source_face_exit_one(r, face, nsel, sources); });
}

extern "C" int c2r_download_source_face_exit(c2r_ctx *c, int face, int ns, double *cols3, int *rounds, int *reached) {
  if (!c) return 1;
  if (face < 0 || face > 5 || !cols3) return fail(c, "c2r_download_source_face_exit: face %d not in 0..5, or null argument", face);
  if (c->pass_open) return fail(c, "c2r_download_source_face_exit: a pass opened by c2r_pass_sources_begin is still open");
  // the context itself or, of a multi-device context, the device that swept the source last with the selection in place
  c2r_ctx *from = nullptr;
  size_t slot = 0;
  long long stamp = 0;
  bool selected = false;
  auto look = [&](c2r_ctx *r) {
    const c2r_ctx::FaceExit &x = r->face_exit[face];
    for (size_t k = 0; k < x.sources.size(); k++) {
      if (x.sources[k] != ns) continue;
      selected = true;
      if (x.stamp[k] > stamp) { stamp = x.stamp[k]; from = r; slot = k; }
    }
  };
  look(c);
  for (c2r_ctx *r : c->replicas) look(r);
  if (!selected)
    return fail(c, "c2r_download_source_face_exit: source %d is not selected for face %d (c2r_select_source_face_exit)", ns, face);
  if (!from) return fail(c, "c2r_download_source_face_exit: no pass has swept source %d since it was selected for face %d", ns, face);
  const c2r_ctx::FaceExit &x = from->face_exit[face];
  HIPCHK(c, hipSetDevice(from->device));
  const size_t n3 = 3 * handover_face_cells(from, face >> 1);
  HIPCHK(c, hipMemcpyAsync(cols3, x.d_cols + slot * n3, sizeof(double) * n3, hipMemcpyDeviceToHost, from->stream));
  HIPCHK(c, hipStreamSynchronize(from->stream));
  if (rounds) *rounds = x.rounds[slot];
  if (reached) *reached = x.reached[slot];
  return 0;
}

// ---------------------------------------------------------------------------------------------
// entry
// the records of a batch in flight (SrcEntry, one per source and scratch set), made at the first call that needs them
static int ensure_entry_records(c2r_ctx *c) {
  HIPCHK(c, hipSetDevice(c->device));
  for (int k = 0; k < 2; k++) {
    if (!c->d_ent[k]) HIPCHK(c, hipMalloc(&c->d_ent[k], sizeof(SrcEntry) * BATCH_MAX));
    if (!c->h_ent[k]) HIPCHK(c, hipHostMalloc(&c->h_ent[k], sizeof(SrcEntry) * BATCH_MAX));
  }
  return 0;
}
// drops the entry or halo of source ns, if it has one
static int clear_source_entry(c2r_ctx *c, int ns) {
  if (c->src_entry.empty() || c->src_entry[(size_t)ns - 1].face < 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c2r_ctx::FaceEntry &e = c->src_entry[(size_t)ns - 1];
  HIPCHK(c, hipFree(e.d_cols));
  e = c2r_ctx::FaceEntry();
  return 0;
}
// Keeps `fresh` (its faces, offsets and rounds; all arrays checked) as the entry or halo of source ns, with `packed` -- the
// arrays one behind the other -- as its one allocation; whatever the source had before goes.
static int keep_source_entry(c2r_ctx *c, int ns, c2r_ctx::FaceEntry fresh, std::vector<double> &packed) {
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream)); // (nothing queued may still read a strip that is replaced)
  if (ensure_entry_records(c)) return 1;
  double *d_new = nullptr;
  HIPCHK(c, hipMalloc(&d_new, sizeof(double) * packed.size()));
  // (-0.0 passes the callers' test: stored as +0.0, the vacuum's own column)
  for (double &v : packed) v = v + 0.0;
  HIPCHK(c, hipMemcpyAsync(d_new, packed.data(), sizeof(double) * packed.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->src_entry.size() != (size_t)c->nsrc) c->src_entry.assign((size_t)c->nsrc, c2r_ctx::FaceEntry());
  c2r_ctx::FaceEntry &e = c->src_entry[(size_t)ns - 1];
  if (e.d_cols) HIPCHK(c, hipFree(e.d_cols));
  e = fresh;
  e.d_cols = d_new;
  return 0;
}
static int set_source_face_entry_one(c2r_ctx *c, int ns, int face, const double *cols3, int rounds) {
  if (!c) return 1;
  if (ns < 1 || ns > c->nsrc) return fail(c, "c2r_set_source_face_entry: source %d not in [1,%d]", ns, c->nsrc);
  if (c->pass_open) return fail(c, "c2r_set_source_face_entry: a pass opened by c2r_pass_sources_begin is still open (close it with c2r_pass_sources_end first)");
  if (!cols3) return clear_source_entry(c, ns); // (an entry or a halo)
  if (face < 0 || face > 5) return fail(c, "c2r_set_source_face_entry: face %d, expected 0..5 (2 * axis + high)", face);
  const int axis = face >> 1, high = face & 1;
  const int mesh[3] = {c->g.n1, c->g.n2, c->g.n3};
  const int *p = &c->srcpos[3 * (size_t)(ns - 1)];
  for (int d = 0; d < 3; d++) {
    const bool ok = d != axis ? (p[d] >= 1 && p[d] <= mesh[d]) : (high ? p[d] > mesh[d] : p[d] < 1);
    if (!ok)
      return fail(c, "c2r_set_source_face_entry: source %d at (%d,%d,%d) does not stand outside the mesh beyond face %d and only beyond it "
                  "(a neighbour across an edge or a corner is not built)", ns, p[0], p[1], p[2], face);
  }
  if (rounds < 1) return fail(c, "c2r_set_source_face_entry: rounds = %d, expected at least 1", rounds);
  const size_t n3 = 3 * handover_face_cells(c, axis);
  for (size_t i = 0; i < n3; i++)
    if (!(cols3[i] >= 0.0) || !std::isfinite(cols3[i]))
      return fail(c, "c2r_set_source_face_entry: source %d: entry %zu of species %d is %g (a column is finite and not negative)", ns,
                  i % (n3 / 3), (int)(i / (n3 / 3)), cols3[i]);
  c2r_ctx::FaceEntry fresh;
  fresh.face = fresh.faces[axis] = face;
  fresh.rounds = rounds;
  fresh.off[axis] = 0;
  std::vector<double> packed(cols3, cols3 + n3);
  return keep_source_entry(c, ns, fresh, packed);
}
extern "C" int c2r_set_source_face_entry(c2r_ctx *c, int ns, int face, const double *cols3, int rounds) {
  if (int e_ = set_source_face_entry_one(c, ns, face, cols3, rounds)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_source_face_entry_one(r, ns, face, cols3, rounds); });
}

// c2r_set_mesh_origin: the deep mesh's coordinates for cinterp (entry_cinterp_position).  Numbers kept with the context;
// nothing on the device changes until the next batch is placed.
constexpr int MESH_ORIGIN_MAX = 1 << 20;
static int set_mesh_origin_one(c2r_ctx *c, const int origin[3]) {
  if (!c) return 1;
  const int o[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
  if (c->pass_open) return fail(c, "c2r_set_mesh_origin: a pass opened by c2r_pass_sources_begin is still open (close it with c2r_pass_sources_end first)");
  for (int d = 0; d < 3; d++) {
    if (o[d] < -MESH_ORIGIN_MAX || o[d] > MESH_ORIGIN_MAX)
      return fail(c, "c2r_set_mesh_origin: origin %d along axis %d not in [%d,%d]", o[d], d, -MESH_ORIGIN_MAX, MESH_ORIGIN_MAX);
    if (o[d] != 0 && c->per[d])
      return fail(c, "c2r_set_mesh_origin: origin %d along axis %d, which is periodic (a part of a deep mesh is open along the axes it is cut along)", o[d], d);
  }
  if (ensure_entry_records(c)) return 1;
  for (int d = 0; d < 3; d++) c->origin[d] = o[d];
  return 0;
}
extern "C" int c2r_set_mesh_origin(c2r_ctx *c, const int origin[3]) {
  if (int e_ = set_mesh_origin_one(c, origin)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_mesh_origin_one(r, origin); });
}
extern "C" int c2r_get_mesh_origin(c2r_ctx *c, int origin[3]) {
  if (!c || !origin) return 1;
  for (int d = 0; d < 3; d++) origin[d] = c->origin[d];
  return 0;
}

// ---------------------------------------------------------------------------------------------
// halo: entry columns through up to three faces, with the edge lines and the corner where their ghost layers meet
static int set_source_halo_one(c2r_ctx *c, int ns, const c2r_source_halo *halo) {
  if (!c) return 1;
  if (ns < 1 || ns > c->nsrc) return fail(c, "c2r_set_source_halo: source %d not in [1,%d]", ns, c->nsrc);
  if (c->pass_open)
    return fail(c, "c2r_set_source_halo: source %d: a pass opened by c2r_pass_sources_begin is still open (close it with c2r_pass_sources_end first)", ns);
  if (!halo) return clear_source_entry(c, ns);
  const int mesh[3] = {c->g.n1, c->g.n2, c->g.n3};
  const int *p = &c->srcpos[3 * (size_t)(ns - 1)];
  c2r_ctx::FaceEntry fresh;
  int nout = 0;
  for (int d = 2; d >= 0; d--) {
    if (p[d] >= 1 && p[d] <= mesh[d]) continue;
    fresh.faces[d] = 2 * d + (p[d] > mesh[d] ? 1 : 0);
    fresh.face = fresh.faces[d]; // (the lowest, in the end)
    nout++;
  }
  if (nout == 0)
    return fail(c, "c2r_set_source_halo: source %d at (%d,%d,%d) stands inside the mesh (a halo belongs to a source beyond one, two or three faces)",
                ns, p[0], p[1], p[2]);
  if (halo->rounds < 1) return fail(c, "c2r_set_source_halo: source %d: rounds = %d, expected at least 1", ns, halo->rounds);
  fresh.rounds = halo->rounds;
  // a whole halo and nothing else: array a of c2ray_halo.hpp, what it is called, whether the source needs it, its doubles per species
  const double *given[HALO_ARRAYS];
  char name[HALO_ARRAYS][16];
  size_t per[HALO_ARRAYS], total = 0;
  for (int d = 0; d < 3; d++) {
    const int a = (d + 1) % 3, b = (d + 2) % 3;
    given[d] = halo->face[d];
    given[3 + d] = halo->edge[d];
    snprintf(name[d], sizeof name[d], "face[%d]", d);
    snprintf(name[3 + d], sizeof name[3 + d], "edge[%d]", d);
    per[d] = handover_face_cells(c, d);
    per[3 + d] = (size_t)mesh[d];
    const bool need_face = fresh.faces[d] >= 0, need_edge = fresh.faces[a] >= 0 && fresh.faces[b] >= 0;
    if (need_face != (given[d] != nullptr))
      return fail(c, need_face ? "c2r_set_source_halo: source %d at (%d,%d,%d) stands outside the mesh along axis %d: %s is missing"
                               : "c2r_set_source_halo: source %d at (%d,%d,%d) stands inside the mesh along axis %d: %s is superfluous",
                  ns, p[0], p[1], p[2], d, name[d]);
    if (need_edge != (given[3 + d] != nullptr))
      return fail(c, need_edge ? "c2r_set_source_halo: source %d at (%d,%d,%d) stands outside the mesh along both axes other than %d: %s is missing"
                               : "c2r_set_source_halo: source %d at (%d,%d,%d) does not stand outside the mesh along both axes other than %d: %s is superfluous",
                  ns, p[0], p[1], p[2], d, name[3 + d]);
  }
  given[6] = halo->corner;
  snprintf(name[6], sizeof name[6], "corner");
  per[6] = 1;
  if ((nout == 3) != (given[6] != nullptr))
    return fail(c, nout == 3 ? "c2r_set_source_halo: source %d at (%d,%d,%d) stands outside the mesh along all three axes: the corner is missing"
                             : "c2r_set_source_halo: source %d at (%d,%d,%d) does not stand outside the mesh along all three axes: the corner is superfluous",
                ns, p[0], p[1], p[2]);
  for (int a = 0; a < HALO_ARRAYS; a++) {
    if (!given[a]) continue;
    for (size_t i = 0; i < 3 * per[a]; i++)
      if (!(given[a][i] >= 0.0) || !std::isfinite(given[a][i]))
        return fail(c, "c2r_set_source_halo: source %d: %s: entry %zu of species %d is %g (a column is finite and not negative)", ns, name[a],
                    i % per[a], (int)(i / per[a]), given[a][i]);
    fresh.off[a] = total;
    total += 3 * per[a];
  }
  std::vector<double> packed;
  packed.reserve(total);
  for (int a = 0; a < HALO_ARRAYS; a++)
    if (given[a]) packed.insert(packed.end(), given[a], given[a] + 3 * per[a]);
  return keep_source_entry(c, ns, fresh, packed);
}
extern "C" int c2r_set_source_halo(c2r_ctx *c, int ns, const c2r_source_halo *halo) {
  if (int e_ = set_source_halo_one(c, ns, halo)) return e_;
  return for_replicas(c, [&](c2r_ctx *r) { return set_source_halo_one(r, ns, halo); });
}
extern "C" int c2r_get_source_halo(c2r_ctx *c, int ns, int faces[3], int *rounds) {
  if (!c) return 1;
  if (ns < 1 || ns > c->nsrc) return fail(c, "c2r_get_source_halo: source %d not in [1,%d]", ns, c->nsrc);
  const bool set = !c->src_entry.empty() && c->src_entry[(size_t)ns - 1].face >= 0;
  if (faces)
    for (int d = 0; d < 3; d++) faces[d] = set ? c->src_entry[(size_t)ns - 1].faces[d] : -1;
  if (rounds) *rounds = set ? c->src_entry[(size_t)ns - 1].rounds : 0;
  return 0;
}

extern "C" int c2r_get_source_face_entry(c2r_ctx *c, int ns, int *face, int *rounds) {
  if (!c) return 1;
  if (ns < 1 || ns > c->nsrc) return fail(c, "c2r_get_source_face_entry: source %d not in [1,%d]", ns, c->nsrc);
  const bool set = !c->src_entry.empty() && c->src_entry[(size_t)ns - 1].face >= 0;
  if (face) *face = set ? c->src_entry[(size_t)ns - 1].face : -1;
  if (rounds) *rounds = set ? c->src_entry[(size_t)ns - 1].rounds : 0;
  return 0;
}
