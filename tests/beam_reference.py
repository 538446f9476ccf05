"""Reference for beamed point sources (c2r_set_source_beams), shared by tests/test_source_beams_host.py (CPU) and
tests/test_gpu_source_beams.py (GPU).  Not a test module.

Nothing here computes a rate: it composes what exists.
  * Every point source alone, from zeroed grids, through orc.do_source -- on the mesh itself where every axis is periodic, on
    the periodic embedding of axis_boundary_cases.AxisCase where some axis is open (mix_reference.point_sources_on_top).  A
    grid then holds the bare terms of that source.
  * A NumPy restatement of the predicate of csrc/c2ray_beam.hpp (lit_offsets), on the offsets the kernels form: the image
    within the periodic reach [-(n/2), n/2 - 1 + n mod 2] on a periodic axis, the plain difference on an open one.
  * The fold in source order, grid = grid + where(lit_s, term_s, 0.0), from 0.0.
  * For the escape maps the per-source terms of face_loss_reference, the unlit ones set to 0.0, folded in source order.
A beam only switches a source's contribution to a cell on or off, so this is exact bit for bit wherever the product traces
the cells the oracle traces: the caller picks cases whose rounds are geometric, or asserts the rounds.

A beam is None (no beam) or a tuple (kind, axis, cos_half), kind 1 a cone and 2 a bicone, as HipEngine.set_source_beams takes it.
"""
import numpy as np

import axis_boundary_cases as ab
import face_loss_reference as fl
import mix_reference as mr

GRIDS = ("phih_grid", "phihe_grid", "phiheat")
CONE, BICONE = 1, 2


def beam_K(cos_half, axis):
    """The host's double: K = (cos_half*cos_half) * ((a_x*a_x + a_y*a_y) + a_z*a_z)."""
    c = np.float64(cos_half)
    a = [np.float64(x) for x in axis]
    return (c * c) * ((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def lit_offsets(beam, dr, di, dj, dk):
    """The predicate for integer offsets (arrays or scalars), every product and sum rounded as written, from the left."""
    di, dj, dk = (np.asarray(x, dtype=np.int64) for x in (di, dj, dk))
    if beam is None or int(beam[0]) == 0:
        return np.ones(np.broadcast(di, dj, dk).shape, dtype=bool)
    kind, axis, cos_half = beam
    ax, ay, az = (np.float64(x) for x in axis)
    K = beam_K(cos_half, axis)
    xs = np.float64(dr[0]) * di.astype(np.float64)
    ys = np.float64(dr[1]) * dj.astype(np.float64)
    zs = np.float64(dr[2]) * dk.astype(np.float64)
    dot = (xs * ax + ys * ay) + zs * az
    d2 = (xs * xs + ys * ys) + zs * zs
    wide = dot * dot >= K * d2
    return wide if int(kind) == BICONE else (dot >= 0.0) & wide


def offsets(n, src, periodic):
    """(di, dj, dk) of every cell of the mesh n from the 1-based source cell src, each of shape [n3, n2, n1]."""
    per_axis = []
    for d in range(3):
        m1 = np.arange(1, int(n[d]) + 1, dtype=np.int64)
        if periodic[d]:
            h = int(n[d]) // 2
            per_axis.append((m1 - int(src[d]) + h) % int(n[d]) - h)
        else:
            per_axis.append(m1 - int(src[d]))
    dk, dj, di = np.meshgrid(per_axis[2], per_axis[1], per_axis[0], indexing="ij")
    return di, dj, dk


def lit_cells(case, ns, beam):
    """Flat bool array over the cells of the product mesh (i fastest): is the cell lit by source ns (0-based)?"""
    di, dj, dk = offsets(case.n, case.srcpos[ns], case.periodic)
    return lit_offsets(beam, case.dr, di, dj, dk).reshape(-1)


def periodic_case(pkg, n, kind, srcpos, flux, heat=False, pl=None, qpl=None, cubic=True):
    """An all-periodic mesh as an AxisCase whose embedding is the mesh itself."""
    n = (int(n),) * 3 if np.isscalar(n) else tuple(int(x) for x in n)
    case = ab.AxisCase(pkg, n, "", n, kind, np.asarray(srcpos, dtype=np.int32).reshape(-1, 3), np.asarray(flux, dtype=np.float64),
                       heat=heat, pl=pl, qpl=qpl)
    if not cubic:
        d = float(case.dr[0])
        case.dr = tuple(k * d for k in mr.DR_FACTORS)
        case.vol = case.dr[0] * case.dr[1] * case.dr[2]
    return case


_alone = {}


def source_alone(pkg, orc, otables, case, key, ns):
    """Source ns (1-based) alone from zeroed grids: (region-sized grids, the oracle's nbox, its loss, (step, state)).  `key` names
    the case: computed once per session, never changed by a caller."""
    if (key, ns) not in _alone:
        _alone[(key, ns)] = mr.point_sources_on_top(pkg, orc, otables, case, None, [ns])
    grids, nbox, loss, pair = _alone[(key, ns)]
    return grids, nbox[0], loss[0], pair


def compose(pkg, orc, otables, case, key, beams, sources=None, inside=None):
    """grid = grid + where(lit_s, term_s, 0.0) over `sources` (1-based, default all, in that order) from 0.0.
    inside: {ns: flat bool array}, cells the product traces for source ns where that is less than the oracle traces.
    Returns the grids and nbox (the oracle's rounds per source, unbeamed)."""
    ncell = ab.cells(case.n)
    sources = list(range(1, len(case.flux) + 1)) if sources is None else list(sources)
    out = dict(phih_grid=np.zeros(ncell), phihe_grid=np.zeros(2 * ncell), phiheat=np.zeros(ncell))
    nbox = []
    for ns in sources:
        grids, nb, _, _ = source_alone(pkg, orc, otables, case, key, ns)
        nbox.append(nb)
        lit = lit_cells(case, ns - 1, beams[ns - 1])
        if inside is not None and ns in inside:
            lit = lit & inside[ns]
        for k in GRIDS:
            comp = out[k].size // ncell
            out[k] = out[k] + np.where(np.tile(lit, comp), grids[k], 0.0)
    out["nbox"] = nbox
    return out


def compose_maps(pkg, orc, otables, case, key, beams, sources=None):
    """The escape maps: face_loss_reference's per-source terms, the unlit ones 0.0, map = map + terms in source order.
    Returns ({face: [b, a]}, the per-source maps)."""
    n, _, periodic = fl.geometry(case)
    sources = list(range(1, len(case.flux) + 1)) if sources is None else list(sources)
    fl.expected(pkg, orc, otables, case, key, sources=[ns - 1 for ns in sources])
    total = {f: np.zeros(fl.face_shape(n, f)) for f in fl.open_faces(periodic)}
    per_source = []
    for ns in sources:
        terms = []
        for m1, o, term in fl.cached_terms(key, ns - 1):
            lit = bool(lit_offsets(beams[ns - 1], case.dr, o[0], o[1], o[2]))
            terms.append((m1, o, term if lit else 0.0))
        one = fl.maps_of_terms(case, terms)
        one = {f: one[f].reshape(fl.face_shape(n, f)) for f in one}
        per_source.append(one)
        for f in total:
            total[f] = total[f] + one[f]
    return total, per_source


# -- the wall in front of a cone ---------------------------------------------------------------------------------------------
WALL_N, WALL_SRC, WALL_FROM = 24, (12, 12, 12), 3
WALL_BEAM = (CONE, (1.0, 0.0, 0.0), float(np.cos(np.radians(35.0))))


def wall_case(pkg, heat=False):
    """Periodic 24^3 (two rounds: +-10, then the mesh), one source.  Thin, highly ionised gas except a neutral slab that fills
    the half space from WALL_FROM cells in front of the source along +x (offsets 3 .. 11, the periodic reach) whose hydrogen column
    per cell is 1e29 cm^-2: beyond max_coldensh = 2e29 after three cells."""
    case = periodic_case(pkg, WALL_N, "ionised", [WALL_SRC], [2.0e7], heat=heat)
    ndens, xh, xhe, temp = case.region
    ncell = ab.cells(case.n)
    di, _, _ = offsets(case.n, WALL_SRC, case.periodic)
    wall = (di >= WALL_FROM).reshape(-1)
    ndens = np.where(wall, 1.0e29 / float(case.dr[0]), ndens)      # (times 1 - abu_he: 0.93e29 of HI per cell)
    x = np.where(wall, 1.0e-6, xh[ncell:])
    xh = np.concatenate([1.0 - x, x])
    xhe = np.concatenate([1.0 - x, 0.8 * x, 0.2 * x])
    case.region = (ndens, xh, xhe, temp)
    case.big = [a for a in case.region]
    return case


def first_box(case, ns=0, size=ab.SUBBOXSIZE):
    """Flat bool array: the cells within +-size of source ns on every axis (the first sub-box)."""
    di, dj, dk = offsets(case.n, case.srcpos[ns], case.periodic)
    return ((np.abs(di) <= size) & (np.abs(dj) <= size) & (np.abs(dk) <= size)).reshape(-1)


def wall_incoming_columns(pkg, orc, otables, case, key):
    """The oracle's incoming HI column (orc_cinterp on its own outgoing columns) of every LIT cell on the surface of the first
    sub-box, for the wall case: [(offset, N_in(HI))]."""
    import ctypes as C
    _, _, _, (st, s) = source_alone(pkg, orc, otables, case, key, 1)
    n, src = case.n, [int(x) for x in case.srcpos[0]]
    di, dj, dk = offsets(n, src, case.periodic)
    surface = (np.maximum(np.maximum(np.abs(di), np.abs(dj)), np.abs(dk)) == ab.SUBBOXSIZE)
    lit = lit_offsets(WALL_BEAM, case.dr, di, dj, dk)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    mesh, src_a = np.array(n, dtype=np.int32), np.array(src, dtype=np.int32)
    out = []
    for o in zip(di[surface & lit], dj[surface & lit], dk[surface & lit]):
        pos = np.array([src[d] + int(o[d]) for d in range(3)], dtype=np.int32)
        a, b, c, p = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        orc.lib().orc_cinterp(mesh.ctypes.data_as(ip), s.coldensh_out.ctypes.data_as(dp), s.coldenshe_out.ctypes.data_as(dp),
                              pos.ctypes.data_as(ip), src_a.ctypes.data_as(ip), C.byref(a), C.byref(b), C.byref(c), C.byref(p))
        out.append((tuple(int(x) for x in o), a.value))
    return out
