"""Reference for several planes and point sources in one pass, shared by tests/test_mix_reference_host.py (CPU) and
tests/test_gpu_plane_mix.py (GPU).  Not a test module.

Nothing here computes a rate: it composes the references that exist, in the order include/c2ray_hip.h documents ("the planes
a caller owns are added before its point sources, in plane order").
  * Every plane's grids come from plane_reference.plane_pass, oblique_reference.oblique_pass or flux_reference.flux_pass,
    each from zeroed grids, so a grid holds the bare terms and the planes fold exactly: grid = grid + plane_k, elementwise,
    in plane order from 0.0 (a cell a plane skips adds +0.0).
  * The point sources go on top through the oracle itself: the folded grids are copied into the State of the periodic
    embedding (axis_boundary_cases.AxisCase; the padding keeps 0) and orc.do_source, which adds into phih / phihe / phiheat
    without zeroing (oracle/c2ray_oracle.c, evolve0D), runs for every point source in source order.
  * The escape maps fold every plane's per-line terms into the far face's map, 2*axis + (1 - from_high), in plane order,
    then face_loss_reference.expected's per-source maps in source order.
The cells are no cubes, dr = (d, 1.25 d, 0.75 d): the path, the fog's dr(1) and vol_ph each have to pick their own.

A plane is a dict: axis, from_high, normflux (a number or three), and optionally tilt (two tangents), fmap (3 x face) and
entry (3 x face).  The pass runs right after begin_step, so xh_av / xhe_av are the case's xh / xhe.
"""
import ctypes as C
import math

import numpy as np

import axis_boundary_cases as ab
import face_loss_reference as fl
import flux_reference as fr
import oblique_reference as obr
import open_boundary_cases as ob
import plane_reference as pr

DR_FACTORS = (1.0, 1.25, 0.75)
# mask -> (product mesh, embedding): the meshes of axis_boundary_cases; "xyz" is open_boundary_cases.case_one_round's box
MESHES = {"z": ((11, 11, 11), (11, 11, 24)), "xy": ((11, 11, 24), (24, 24, 24)), "xz": ((11, 24, 24), (24, 24, 48)),
          "xyz": ((11, 11, 11), (24, 24, 24))}


def make_case(pkg, mask, srcpos, flux, heat=False, pl=None, qpl=None, seed=None, mesh=None, kind="mixed"):
    """An AxisCase of kind "mixed" (or `kind`) on the meshes of `mask` (or mesh = (n, m)) whose cells are no cubes.  seed: other gas than
    AxisCase's own, region and padding (the gas does not depend on dr)."""
    n, m = MESHES[mask] if mesh is None else mesh
    srcpos = np.asarray(srcpos, dtype=np.int32).reshape(-1, 3)
    case = ab.AxisCase(pkg, n, mask, m, kind, srcpos, np.asarray(flux, dtype=np.float64), heat=heat, pl=pl, qpl=qpl)
    if seed is not None:
        case.region = ob.gas(pkg, ab.cells(n), np.random.default_rng(seed), kind, heat)
        case.big = case.embedding(pkg, m, seed + 1000, kind)
    d = float(case.dr[0])
    case.dr = tuple(k * d for k in DR_FACTORS)
    case.vol = case.dr[0] * case.dr[1] * case.dr[2]
    case.check_embedding(case.m)
    assert all(1 <= int(p[d]) <= n[d] for p in srcpos for d in range(3)), srcpos
    return case


def embed_lls(case, lls_grid, seed=99):
    """A REAL(4) fog grid of the region in the embedding mesh; the padding gets fog of the same kind."""
    pad = (10.0 ** np.random.default_rng(seed).uniform(15.5, 17, ab.cells(case.m))).astype(np.float32)
    return ab.embed3(np.asarray(lls_grid, dtype=np.float32), case.n, case.m, pad)


def plane_kind(plane):
    tilt = plane.get("tilt")
    tilted = tilt is not None and (float(tilt[0]) != 0.0 or float(tilt[1]) != 0.0)
    return tilted, plane.get("fmap") is not None


def plane_alone(orc, otables, case, plane, coldensh_lls=None, lls_grid=None):
    """One plane from zeroed grids by the matching reference: normal, tilted, mapped, or tilted and mapped."""
    ndens, xh, xhe, _ = case.region
    tilted, mapped = plane_kind(plane)
    kw = dict(heat=case.heat, coldensh_lls=coldensh_lls, lls_grid=lls_grid, entry=plane.get("entry"))
    args = (orc, otables, case.n, case.dr, case.vol, ndens, xh, xhe, plane["axis"], plane["from_high"])
    if mapped:
        return fr.flux_pass(*args, plane["fmap"], tilt=plane["tilt"] if tilted else None, periodic=case.periodic, **kw)
    if tilted:
        return obr.oblique_pass(*args, plane["normflux"], plane["tilt"], periodic=case.periodic, **kw)
    return pr.plane_pass(*args, plane["normflux"], **kw)


def share_of(nsrc, nplane, first=1, stride=1):
    """(point sources, planes) of the caller (first, stride) of the static deal, both 1-based and in order."""
    mine = list(range(first, nsrc + nplane + 1, stride))
    return [ns for ns in mine if ns <= nsrc], [ns - nsrc for ns in mine if ns > nsrc]


def fold_planes(case, refs, order):
    """grid = grid + plane_k from zero over the planes `order` (1-based numbers into refs)."""
    n = ab.cells(case.n)
    out = dict(phih_grid=np.zeros(n), phihe_grid=np.zeros(2 * n), phiheat=np.zeros(n))
    for p in order:
        for k in out:
            out[k] = out[k] + refs[p][k]
    return out


def point_sources_on_top(pkg, orc, otables, case, seed_grids, sources, coldensh_lls=None, lls_grid=None):
    """orc.do_source for the point sources `sources` (1-based, in that order) on the embedding, the rate grids seeded with
    `seed_grids` (region-sized; None: zero): region-sized grids, the oracle's nbox and its loss per source, and the (step, state)
    pair."""
    hp = pkg.hostphys
    nd, xh, xhe, temp = case.big
    kw = {}
    if case.pl is not None:
        kw = dict(normflux_pl=case.pl, normflux_qpl=case.qpl, pl_s_star=case.pl_s_star, qpl_s_star=case.qpl_s_star)
    st = orc.Step(case.m, case.dr, case.vol, ab.ZRED, hp.H0, hp.Omega0, not case.heat, 1.0e4, 1.0, case.srcpos, case.flux, case.s_star, nd,
                  case.reccoef, coldensh_lls=coldensh_lls, lls_grid=None if lls_grid is None else embed_lls(case, lls_grid), **kw)
    s = orc.State(st, xh, xhe, temp)
    orc.begin_step(s)
    if seed_grids is not None:
        for attr, k in (("phih", "phih_grid"), ("phihe", "phihe_grid"), ("phiheat", "phiheat")):
            getattr(s, attr)[:] = ab.embed3(seed_grids[k], case.n, case.m, np.zeros(getattr(s, attr).size))
    ran = [orc.do_source(otables, st, s, int(ns)) for ns in sources]
    nbox, loss = [r[0] for r in ran], [r[1] for r in ran]
    out = {k: ab.extract3(getattr(s, attr), case.n, case.m) for attr, k in (("phih", "phih_grid"), ("phihe", "phihe_grid"), ("phiheat", "phiheat"))}
    return out, nbox, loss, (st, s)


def point_maps_fog_grid(pkg, orc, otables, case, ns, lls_grid):
    """face_loss_reference.source_terms / maps_of_terms for point source ns (0-based) alone with the fog of a REAL(4) grid,
    which that module does not take: the same steps, the fog of evolve_point.F90:177-180 from the cell's own grid entry.
    Every fogged incoming HI column is held to the oracle's own outgoing column of that cell, N_out = N_in + coldens, bit for
    bit: the oracle fogged with ITS index into the grid, so an index slip here does not pass."""
    n, m, periodic = fl.geometry(case)
    _, _, _, (st, s) = point_sources_on_top(pkg, orc, otables, case, None, [ns + 1], lls_grid=lls_grid)
    consts = orc.constants()
    pi, abu_he, eps = float(consts[0]), float(consts[1]), float(consts[30])
    dr, vol = [float(x) for x in case.dr], float(case.vol)
    src = [int(x) for x in case.srcpos[ns]]
    nf = [float(case.flux[ns]), 0.0 if case.pl is None else float(case.pl[ns]), 0.0 if case.qpl is None else float(case.qpl[ns])]
    ncell_m = ab.cells(m)
    cH, cHe = s.coldensh_out, s.coldenshe_out
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    mesh_m, src_a = np.array(m, dtype=np.int32), np.array(src, dtype=np.int32)
    lls = np.asarray(lls_grid, dtype=np.float32).reshape(n[2], n[1], n[0])
    terms = []
    for k in range(1, n[2] + 1):
        for j in range(1, n[1] + 1):
            for i in range(1, n[0] + 1):
                m1 = (i, j, k)
                if not any((not periodic[d]) and (m1[d] == 1 or m1[d] == n[d]) for d in range(3)):
                    continue
                q = (i - 1) + m[0] * ((j - 1) + m[1] * (k - 1))
                if cH[q] == 0.0:
                    continue
                o = [(m1[d] - src[d] + n[d] // 2) % n[d] - n[d] // 2 if periodic[d] else m1[d] - src[d] for d in range(3)]
                if o == [0, 0, 0]:
                    cin, vol_ph = [0.0, 0.0, 0.0], dr[0] * dr[1] * dr[2]
                else:
                    pos = np.array([src[d] + o[d] for d in range(3)], dtype=np.int32)
                    a, b, c, p = C.c_double(), C.c_double(), C.c_double(), C.c_double()
                    orc.lib().orc_cinterp(mesh_m.ctypes.data_as(ip), cH.ctypes.data_as(dp), cHe.ctypes.data_as(dp), pos.ctypes.data_as(ip),
                                          src_a.ctypes.data_as(ip), C.byref(a), C.byref(b), C.byref(c), C.byref(p))
                    cin, path = [a.value, b.value, c.value], p.value * dr[0]
                    xs, ys, zs = dr[0] * float(o[0]), dr[1] * float(o[1]), dr[2] * float(o[2])
                    vol_ph = 4.0 * pi * (xs * xs + ys * ys + zs * zs) * path
                    cin[0] = cin[0] + float(lls[k - 1, j - 1, i - 1]) * path / dr[0]
                    own = max(float(s.xh_av[q]), eps) * float(st.ndens[q]) * path * (1.0 - abu_he)
                    assert cin[0] + own == float(cH[q]), (m1, cin[0] + own, float(cH[q]))
                term = 0.0
                if cin[0] < fl.MAX_COLDENSH:
                    cols6 = [cin[0], float(cH[q]), cin[1], float(cHe[q]), cin[2], float(cHe[q + ncell_m])]
                    term = pr._photoion(orc, otables, cols6, vol_ph, nf, case.pl is not None, max(float(s.xh_av[q + ncell_m]), eps), case.heat)[4]
                    term = term * vol / vol_ph
                terms.append((m1, tuple(o), term))
    maps = fl.maps_of_terms(case, terms)
    return {f: maps[f].reshape(fl.face_shape(n, f)) for f in maps}


def point_maps(pkg, orc, otables, case, key, sources, coldensh_lls=None, lls_grid=None):
    """The escape maps of each point source of `sources` (1-based) alone: a list of {face: [b, a]}."""
    if lls_grid is None:
        return fl.expected(pkg, orc, otables, case, key, sources=[ns - 1 for ns in sources], coldensh_lls=coldensh_lls)[1]
    return [point_maps_fog_grid(pkg, orc, otables, case, ns - 1, lls_grid) for ns in sources]


def has_loss_reference(case):
    """photon_loss(1) has a reference where every box face that loses photons is an open mesh face: all axes open and every
    offset within the first round, so that every source's final box is its whole reach (include/c2ray_hip.h, Identities)."""
    return not any(case.periodic) and all(nd - 1 <= ab.SUBBOXSIZE for nd in case.n)


def same_cells(case, sources, nbox):
    """Per point source of `sources` (1-based; nbox: the oracle's rounds for it): do the oracle on the embedding and the product
    on the open mesh trace the same cells of the region?  For gas of kind "mixed", the product in ONE round, yes where
      * the source's whole reach lies within subboxsize on every axis: the product's first box is its last (no face can still
        move), it holds every cell of the reach, and whatever further rounds the oracle runs on the larger mesh meet traced
        cells or padding only; or
      * the oracle stops after one round: its loss over the six faces of the +-subboxsize box is <= 1e-10 of the flux, and the
        product's deciding loss (include/c2ray_hip.h) runs over a subset of those surface cells, so it stops as well.
    Everywhere else the two may disagree about the rounds, and the case is not used.
    For gas of kind "ionised" (neutral fractions below 10^-3.5: the whole mesh is optically thin, every face of every box passes
    far more than 1e-10 of the flux) both run to their reach, as axis_boundary_cases' cases a to d do: yes where the oracle
    never stopped early, that is, ran the rounds its z faces need on the embedding.  The product's rounds are then
    case.expected_rounds(), which compose() reports as sum_nbox."""
    out = []
    if case.kind == "ionised":
        full = -(-(case.m[2] // 2 - 1 + case.m[2] % 2) // ab.SUBBOXSIZE)
        return [nb == full for nb in nbox]
    for ns, nb in zip(sources, nbox):
        l, r = case.reach(ns - 1)
        out.append(nb == 1 or max(max(-a for a in l), max(r)) <= ab.SUBBOXSIZE)
    return out


def compose(pkg, orc, otables, case, planes, key, first=1, stride=1, coldensh_lls=None, lls_grid=None, plane_order=None,
            planes_last=False, with_maps=True):
    """The pass of caller (first, stride) over the case's point sources and `planes`.
    plane_order: fold the caller's planes in this order instead of plane order; planes_last: add them after the point
    sources, elementwise -- both exist for the tests that show the order matters.
    Returns phih_grid, phihe_grid, phiheat, sum_nbox (the product's rounds where same_cells holds: one per point source in
    mixed gas, case.expected_rounds in ionised gas), nbox (the oracle's, per point source of the share), oracle_sum_nbox and
    oracle_loss (its sum_nbox and photon_loss(1) on the embedding: 0 + loss_1 + loss_2 ..., as orc_pass_all_sources adds them),
    same_cells (see there), sources and planes
    (the share, 1-based), plane (number -> that plane's reference alone), maps ({face: [b, a]}) and loss (the reference of
    photon_loss(1), or None where there is none)."""
    nsrc = len(case.flux)
    sources, mine = share_of(nsrc, len(planes), first, stride)
    lls = dict(coldensh_lls=coldensh_lls, lls_grid=lls_grid)
    refs = {p: plane_alone(orc, otables, case, planes[p - 1], **lls) for p in mine}
    order = list(mine if plane_order is None else plane_order)
    assert sorted(order) == sorted(mine)
    if planes_last:
        points, nbox, losses, _ = point_sources_on_top(pkg, orc, otables, case, None, sources, **lls)
        grids = {k: points[k].copy() for k in points}
        for p in order:
            for k in grids:
                grids[k] = grids[k] + refs[p][k]
    else:
        grids, nbox, losses, _ = point_sources_on_top(pkg, orc, otables, case, fold_planes(case, refs, order), sources, **lls)
    rounds = case.expected_rounds([ns - 1 for ns in sources]) if case.kind == "ionised" and sources else len(sources)
    oracle_loss = 0.0
    for one in losses:
        oracle_loss = oracle_loss + one
    out = dict(grids, sum_nbox=int(rounds), nbox=nbox, oracle_sum_nbox=int(sum(nbox)), oracle_loss=oracle_loss,
               same_cells=same_cells(case, sources, nbox), sources=sources, planes=mine, plane=refs, maps=None, loss=None)
    if not with_maps:
        return out
    n = tuple(int(x) for x in case.n)
    maps = {f: np.zeros(fl.face_shape(n, f)) for f in fl.open_faces(case.periodic)}
    for p in order:
        far = 2 * planes[p - 1]["axis"] + (1 - planes[p - 1]["from_high"])
        maps[far] = maps[far] + refs[p]["terms"].reshape(fl.face_shape(n, far))
    per_source = point_maps(pkg, orc, otables, case, key, sources, **lls) if sources else []
    for one in per_source:
        for f in maps:
            maps[f] = maps[f] + one[f]
    out["maps"] = maps
    if has_loss_reference(case):
        out["loss"] = math.fsum([refs[p]["loss"] for p in mine] + [fl.total_of(one) for one in per_source])
    return out


# -- cases both test files use ---------------------------------------------------------------------------------------------
FLUX = 3.0e-41          # per cm^2 of face, in units of S_star = 1e48 photons / s (tests/test_gpu_plane_sources.py)
FLUX_E = np.array([3.0e7, 8.0e6, 1.5e7, 2.0e7])     # axis_boundary_cases.case_e's isothermal fluxes
TILT = (0.35, -0.6)


def case_a(pkg, heat=False, **kw):
    """(11,11,11), z open, embedding (11,11,24), the four sources of axis_boundary_cases.E_SOURCES."""
    return make_case(pkg, "z", ab.E_SOURCES, FLUX_E, heat=heat, **kw)


PLANES_A = [dict(axis=2, from_high=0, normflux=FLUX), dict(axis=2, from_high=1, normflux=0.6 * FLUX)]
PLANES_D = [dict(axis=2, from_high=1, normflux=FLUX), dict(axis=2, from_high=1, normflux=0.6 * FLUX)]
# three planes on case a's mesh: the shortest list in which the order of the planes can change a bit
PLANES_A3 = PLANES_A + [dict(axis=2, from_high=1, normflux=1.7 * FLUX)]


def make_map(case, axis, seed, seds=1, scale=1.0):
    """A random flux map around FLUX with a block of dark cells and one dark line of the face: (3, face)."""
    a, b = pr.face_axes(axis)
    fa, fb = case.n[a], case.n[b]
    m = np.zeros((3, fb, fa))
    m[:seds] = scale * FLUX * np.random.default_rng(seed).uniform(0.3, 2.0, (seds, fb, fa))
    m[:, 2:5, 1:4] = 0.0
    m[:, fb - 2, :] = 0.0
    return m.reshape(3, -1)


def case_c(pkg, **kw):
    """(11,11,24), x and y open, embedding (24,24,24), axis_boundary_cases.case_c's source cells."""
    return make_case(pkg, "xy", [(1, 1, 1), (11, 11, 24), (6, 11, 12), (3, 5, 7)], ab.FLUX4, **kw)


def make_entry(case, axis, seed):
    """Entry columns as a slab upstream would hand them over: (HI, HeI, HeII) x face."""
    rng, face = np.random.default_rng(seed), pr.face_cells(case.n, axis)
    return np.concatenate([10.0 ** rng.uniform(15, 17, face), 10.0 ** rng.uniform(14, 16, face), 10.0 ** rng.uniform(12, 15, face)])


def planes_c(case, tilted=(2, 4), mapped=(3, 4), entry=(2, 3)):
    """Four planes through four different faces; `tilted` / `mapped` / `entry`: the 1-based numbers that get a tilt / a flux
    map / entry columns."""
    faces = [(0, 0), (1, 1), (0, 1), (1, 0)]
    out = []
    for p, (axis, from_high) in enumerate(faces, start=1):
        pl = dict(axis=axis, from_high=from_high, normflux=(0.5 + 0.25 * p) * FLUX)
        if p in tilted:
            pl["tilt"] = (TILT[0], TILT[1]) if axis == 0 else (TILT[1], TILT[0])
        if p in mapped:
            pl["fmap"] = make_map(case, axis, 40 + p, scale=0.5 + 0.1 * p)
        if p in entry:
            pl["entry"] = make_entry(case, axis, 60 + p)
        out.append(pl)
    return out


def case_j(pkg):
    """axis_boundary_cases.case_d with cells that are no cubes: (11,24,24), x and z open, ionised gas -- every point source runs
    to its reach, three rounds from a corner, so the planes meet point sources that need more than one round."""
    return make_case(pkg, "xz", [(1, 1, 1), (11, 24, 24), (6, 1, 12), (11, 13, 1)], ab.FLUX4, kind="ionised")


PLANES_J = [dict(axis=2, from_high=0, normflux=FLUX), dict(axis=0, from_high=1, normflux=0.8 * FLUX, tilt=TILT)]
