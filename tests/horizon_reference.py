"""Reference for photon horizons (c2r_set_source_horizons), shared by tests/test_source_horizons_host.py (CPU) and
tests/test_gpu_source_horizons.py (GPU).  Not a test module.

Nothing here computes a rate: it composes what tests/beam_reference.py composes, with one more mask.
  * A NumPy restatement of the predicate of csrc/c2ray_horizon.hpp (within_offsets) on the offsets of beam_reference.offsets.
  * compose / compose_maps as in beam_reference, with lit = beam_lit & within & inside.
  * The loss terms of the cells on the surface of the first sub-box (box_surface_terms), by the steps of
    face_loss_reference.source_terms: the oracle's columns, orc_cinterp and the oracle's photoion_rates.
A horizon is None or inf (no horizon) or a radius in the length unit of dr, as HipEngine.set_source_horizons takes it.
"""
import ctypes as C

import numpy as np

import axis_boundary_cases as ab
import beam_reference as br
import face_loss_reference as fl

GRIDS = br.GRIDS


def horizon_R2(radius):
    """The host's double: R2 = radius*radius (+inf where it overflows)."""
    r = np.float64(radius)
    with np.errstate(over="ignore"):
        return r * r


def within_offsets(radius, dr, di, dj, dk):
    """The predicate for integer offsets (arrays or scalars), every product and sum rounded as written, from the left."""
    di, dj, dk = (np.asarray(x, dtype=np.int64) for x in (di, dj, dk))
    if radius is None or np.isposinf(radius):
        return np.ones(np.broadcast(di, dj, dk).shape, dtype=bool)
    xs = np.float64(dr[0]) * di.astype(np.float64)
    ys = np.float64(dr[1]) * dj.astype(np.float64)
    zs = np.float64(dr[2]) * dk.astype(np.float64)
    d2 = (xs * xs + ys * ys) + zs * zs
    return d2 <= horizon_R2(radius)


def lit_offsets(beam, radius, dr, di, dj, dk):
    """Both predicates: the cell is lit iff the beam lights it and it is within the horizon."""
    return br.lit_offsets(beam, dr, di, dj, dk) & within_offsets(radius, dr, di, dj, dk)


def within_cells(case, ns, radius):
    """Flat bool array over the cells of the product mesh (i fastest): is the cell within the horizon of source ns (0-based)?"""
    di, dj, dk = br.offsets(case.n, case.srcpos[ns], case.periodic)
    return within_offsets(radius, case.dr, di, dj, dk).reshape(-1)


def _beams(case, beams):
    return [None] * len(case.flux) if beams is None else list(beams)


def compose(pkg, orc, otables, case, key, horizons, beams=None, sources=None, inside=None):
    """beam_reference.compose with lit = beam_lit & within & inside."""
    masks = {}
    for ns in range(1, len(case.flux) + 1):
        masks[ns] = within_cells(case, ns - 1, horizons[ns - 1])
        if inside is not None and ns in inside:
            masks[ns] = masks[ns] & inside[ns]
    return br.compose(pkg, orc, otables, case, key, _beams(case, beams), sources=sources, inside=masks)


def compose_maps(pkg, orc, otables, case, key, horizons, beams=None, sources=None):
    """beam_reference.compose_maps with the horizon in the mask: ({face: [b, a]}, the per-source maps)."""
    beams = _beams(case, beams)
    n, _, periodic = fl.geometry(case)
    sources = list(range(1, len(case.flux) + 1)) if sources is None else list(sources)
    fl.expected(pkg, orc, otables, case, key, sources=[ns - 1 for ns in sources])
    total = {f: np.zeros(fl.face_shape(n, f)) for f in fl.open_faces(periodic)}
    per_source = []
    for ns in sources:
        terms = []
        for m1, o, term in fl.cached_terms(key, ns - 1):
            lit = bool(lit_offsets(beams[ns - 1], horizons[ns - 1], case.dr, o[0], o[1], o[2]))
            terms.append((m1, o, term if lit else 0.0))
        one = fl.maps_of_terms(case, terms)
        one = {f: one[f].reshape(fl.face_shape(n, f)) for f in one}
        per_source.append(one)
        for f in total:
            total[f] = total[f] + one[f]
    return total, per_source


def box_surface_terms(pkg, orc, otables, case, key, ns=1, size=ab.SUBBOXSIZE):
    """[(offset, term)]: photo_out*vol/vol_ph (evolve_point.F90:310-315) of every cell on the surface of the +-size box around
    source ns (1-based) of an all-periodic, isothermal, one-SED case whose reach exceeds `size`, from the oracle's columns of
    that source alone (every cell is traced once, so a later round leaves the columns of this surface as round 1 made them)."""
    assert all(case.periodic) and not case.heat and case.pl is None
    _, _, _, (st, s) = br.source_alone(pkg, orc, otables, case, key, ns)
    n, src = case.n, [int(x) for x in case.srcpos[ns - 1]]
    consts = orc.constants()
    pi, eps = float(consts[0]), float(consts[30])
    dr, vol, ncell = [float(x) for x in case.dr], float(case.vol), ab.cells(n)
    di, dj, dk = br.offsets(n, src, case.periodic)
    surface = np.maximum(np.maximum(np.abs(di), np.abs(dj)), np.abs(dk)) == size
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    mesh, src_a = np.array(n, dtype=np.int32), np.array(src, dtype=np.int32)
    cH, cHe = s.coldensh_out, s.coldenshe_out
    out = []
    for o in zip(di[surface], dj[surface], dk[surface]):
        o = tuple(int(x) for x in o)
        pos = np.array([src[d] + o[d] for d in range(3)], dtype=np.int32)
        m0 = [(src[d] + o[d] - 1) % n[d] for d in range(3)]
        q = m0[0] + n[0] * (m0[1] + n[1] * m0[2])
        a, b, c, p = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        orc.lib().orc_cinterp(mesh.ctypes.data_as(ip), cH.ctypes.data_as(dp), cHe.ctypes.data_as(dp), pos.ctypes.data_as(ip),
                              src_a.ctypes.data_as(ip), C.byref(a), C.byref(b), C.byref(c), C.byref(p))
        path = p.value * dr[0]
        xs, ys, zs = dr[0] * float(o[0]), dr[1] * float(o[1]), dr[2] * float(o[2])
        vol_ph = 4.0 * pi * (xs * xs + ys * ys + zs * zs) * path
        term = 0.0
        if a.value < fl.MAX_COLDENSH:
            cols6 = [a.value, float(cH[q]), b.value, float(cHe[q]), c.value, float(cHe[q + ncell])]
            i_state = max(float(s.xh_av[q + ncell]), eps)
            term = orc.photoion_rates(otables, cols6, vol_ph, float(case.flux[ns - 1]), i_state, True)[20] * vol / vol_ph
        out.append((o, term))
    return out
