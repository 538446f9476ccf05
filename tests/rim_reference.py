"""Reference for the horizon loss (c2r_enable_horizon_loss), shared by tests/test_horizon_loss_host.py (CPU) and
tests/test_gpu_horizon_loss.py (GPU).  Not a test module.

  * An independent restatement of the rule of csrc/c2ray_rim.hpp in plain Python floats (IEEE doubles, no contraction): the
    sheet columns of a box in order, k* by SCANNING the column with the predicate of tests/horizon_reference.py, the face
    flag, the weight as written.
  * face_sum: the fixed order of c2r_get_face_loss in NumPy.
  * The expected terms of a source: the rule composed with the oracle by the steps of horizon_reference.box_surface_terms /
    face_loss_reference.source_terms applied to the rim cells -- the oracle's columns of the source alone, orc_cinterp, then
    the oracle's photoion_rates(...)[20].
A beam is None or (kind, axis, cos_half) as in tests/beam_reference.py; a radius is a length in the unit of dr.
"""
import ctypes as C
import math

import numpy as np

import beam_reference as br
import face_loss_reference as fl
import horizon_reference as hr

PI = float(np.float32(3.141592654))          # the project's pi (csrc/c2ray_device.hpp), the one of the kept loss's vol_ph
BLOCK = 256


# -- the rule -------------------------------------------------------------------------------------------------------------------
def extents(lo, hi):
    return [max(0, int(hi[d]) - int(lo[d]) + 1) for d in range(3)]


def total(lo, hi):
    e = extents(lo, hi)
    return 2 * (e[1] * e[2] + e[0] * e[2] + e[0] * e[1])


def sheet_columns(lo, hi):
    """(fc, oa, ob) of every sheet column, in entry order: the six sheets in face order, a fastest."""
    out = []
    for fc in range(6):
        a, b = [d for d in range(3) if d != fc // 2]
        for ob in range(int(lo[b]), int(hi[b]) + 1):
            for oa in range(int(lo[a]), int(hi[a]) + 1):
                out.append((fc, oa, ob))
    return out


def cell_of(fc, oa, ob, k):
    d, s = fc // 2, (1 if fc & 1 else -1)
    a, b = [x for x in range(3) if x != d]
    o = [0, 0, 0]
    o[d], o[a], o[b] = s * k, oa, ob
    return tuple(o)


def within(radius, dr, o):
    """horizon_reference.within_offsets for one cell, in Python floats (the host test compares the two on a cube)."""
    xs, ys, zs = float(dr[0]) * float(o[0]), float(dr[1]) * float(o[1]), float(dr[2]) * float(o[2])
    d2 = (xs * xs + ys * ys) + zs * zs
    return d2 <= float(radius) * float(radius)


def weight(dr, fc, oa, ob, k):
    if oa == 0 and ob == 0 and k == 0:
        return 1.0 / 6.0
    d = fc // 2
    a, b = [x for x in range(3) if x != d]
    dra, drb, drd = float(dr[a]), float(dr[b]), float(dr[d])
    xa, xb, fd = dra * float(oa), drb * float(ob), drd * (float(k) + 0.5)
    f2 = (xa * xa + xb * xb) + fd * fd
    return ((dra * drb) * fd) / ((4.0 * PI) * (f2 * math.sqrt(f2)))


def column(radius, dr, lo, hi, fc, oa, ob, beam=None):
    """(k*, has a face, w, the column's cell): k* = -1 where the k = 0 cell is not within; w = 0.0 without a face."""
    d, s = fc // 2, (1 if fc & 1 else -1)
    inside = lambda o: all(int(lo[e]) <= o[e] <= int(hi[e]) for e in range(3))
    if not within(radius, dr, cell_of(fc, oa, ob, 0)):
        return -1, False, 0.0, (0, 0, 0)
    k = 0
    while inside(cell_of(fc, oa, ob, k + 1)) and within(radius, dr, cell_of(fc, oa, ob, k + 1)):
        k += 1
    o = cell_of(fc, oa, ob, k)
    interior = all(int(lo[e]) < o[e] < int(hi[e]) for e in range(3))
    if not interior or within(radius, dr, cell_of(fc, oa, ob, k + 1)):
        return k, False, 0.0, o
    if not bool(br.lit_offsets(beam, dr, o[0], o[1], o[2])):
        return k, False, 0.0, o
    return k, True, weight(dr, fc, oa, ob, k), o


def columns(radius, dr, lo, hi, beam=None):
    """The rule over every sheet column: dict of arrays kstar[T], face[T], w[T], cell[T, 3], col[T, 3]."""
    cols = sheet_columns(lo, hi)
    assert len(cols) == total(lo, hi)
    rows = [column(radius, dr, lo, hi, fc, oa, ob, beam) for fc, oa, ob in cols]
    return dict(kstar=np.array([r[0] for r in rows], dtype=np.int32), face=np.array([r[1] for r in rows], dtype=bool),
                w=np.array([r[2] for r in rows], dtype=np.float64), cell=np.array([r[3] for r in rows], dtype=np.int32).reshape(-1, 3),
                col=np.array(cols, dtype=np.int32).reshape(-1, 3))


# -- the fixed order ------------------------------------------------------------------------------------------------------------
def _block_tree(v):
    x = np.zeros(BLOCK)
    x[:len(v)] = v
    y = x.reshape(BLOCK // 64, 64).copy()
    off = 32
    while off > 0:
        y[:, :off] = y[:, :off] + y[:, off:2 * off]
        off >>= 1
    r = 0.0
    for wv in range(BLOCK // 64):
        r = r + float(y[wv, 0])
    return r


def face_sum(values):
    """csrc/c2ray_face.hpp face_sum: blocks of 256 by a tree, lane t of the last block adds the block sums t, t + 256, ..."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    lane = [0.0] * BLOCK
    for b in range((len(v) + BLOCK - 1) // BLOCK):
        lane[b % BLOCK] = lane[b % BLOCK] + _block_tree(v[b * BLOCK:(b + 1) * BLOCK])
    return _block_tree(np.array(lane))


# -- the rule composed with the oracle --------------------------------------------------------------------------------------------
def final_box(case, ns, nbox=1, size=10):
    """lo, hi of the final sub-box of source ns (0-based) after nbox rounds: +-size*nbox cut at the source's reach (the periodic
    reach [-(n/2), n/2 - 1 + n mod 2], the mesh itself on an open axis)."""
    n, _, periodic = fl.geometry(case)
    src = [int(x) for x in case.srcpos[ns]]
    lo, hi = [], []
    for d in range(3):
        l, r = (-(n[d] // 2), n[d] // 2 - 1 + n[d] % 2) if periodic[d] else (1 - src[d], n[d] - src[d])
        lo.append(max(-size * nbox, l))
        hi.append(min(size * nbox, r))
    return lo, hi


_runs = {}


def _oracle_columns(pkg, orc, otables, case, key, ns):
    if (key, ns) not in _runs:
        _runs[(key, ns)] = fl._oracle_run(pkg, orc, otables, case, ns, None)
    return _runs[(key, ns)]


def cell_photo_out(pkg, orc, otables, case, key, ns, o):
    """photo_out of the cell at offset o from source ns (0-based), the source alone: face_loss_reference.source_terms' steps."""
    return cell_photo_out_vol(pkg, orc, otables, case, key, ns, o)[0]


def cell_photo_out_vol(pkg, orc, otables, case, key, ns, o):
    """(photo_out, vol_ph) of that cell: its loss term is photo_out * vol / vol_ph (evolve_point.F90:310-315)."""
    n, m, periodic = fl.geometry(case)
    st, s, _ = _oracle_columns(pkg, orc, otables, case, key, ns)
    consts = orc.constants()
    pi, eps = float(consts[0]), float(consts[30])
    dr = [float(x) for x in case.dr]
    src = [int(x) for x in case.srcpos[ns]]
    nf = [float(case.flux[ns]), 0.0 if case.pl is None else float(case.pl[ns]), 0.0 if case.qpl is None else float(case.qpl[ns])]
    ncell_m = m[0] * m[1] * m[2]
    cH, cHe = s.coldensh_out, s.coldenshe_out
    m1 = [(src[d] + o[d] - 1) % n[d] + 1 if periodic[d] else src[d] + o[d] for d in range(3)]
    assert all(1 <= m1[d] <= n[d] for d in range(3)), (o, m1)
    q = (m1[0] - 1) + m[0] * ((m1[1] - 1) + m[1] * (m1[2] - 1))
    assert cH[q] != 0.0, "the oracle has not traced this cell"
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    if tuple(o) == (0, 0, 0):
        cin = [0.0, 0.0, 0.0]
        vol_ph = dr[0] * dr[1] * dr[2]
    else:
        mesh_m, src_a = np.array(m, dtype=np.int32), np.array(src, dtype=np.int32)
        pos = np.array([src[d] + o[d] for d in range(3)], dtype=np.int32)
        a, b, c, p = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        orc.lib().orc_cinterp(mesh_m.ctypes.data_as(ip), cH.ctypes.data_as(dp), cHe.ctypes.data_as(dp), pos.ctypes.data_as(ip),
                              src_a.ctypes.data_as(ip), C.byref(a), C.byref(b), C.byref(c), C.byref(p))
        cin = [a.value, b.value, c.value]
        path = p.value * dr[0]
        xs, ys, zs = dr[0] * float(o[0]), dr[1] * float(o[1]), dr[2] * float(o[2])
        vol_ph = 4.0 * pi * (xs * xs + ys * ys + zs * zs) * path
    if not cin[0] < fl.MAX_COLDENSH:
        return 0.0, vol_ph
    cols6 = [cin[0], float(cH[q]), cin[1], float(cHe[q]), cin[2], float(cHe[q + ncell_m])]
    i_state = max(float(s.xh_av[q + ncell_m]), eps)
    if case.pl is not None:
        r = orc.PhotRates()
        orc.lib().orc_photoion_rates3(C.byref(otables.c), *[C.c_double(x) for x in cols6], C.c_double(vol_ph), (C.c_double * 3)(*nf),
                                      C.c_double(i_state), C.c_int(0 if case.heat else 1), C.byref(r))
        return float(r.photo_out), vol_ph
    return float(orc.photoion_rates(otables, cols6, vol_ph, nf[0], i_state, not case.heat)[20]), vol_ph


def source_terms(pkg, orc, otables, case, key, ns, radius, lo, hi, beam=None):
    """The T expected terms of source ns (0-based) with the final box lo..hi: po * w per sheet column, +0.0 without a face; and
    the rule's arrays."""
    rule = columns(radius, case.dr, lo, hi, beam)
    terms = np.zeros(len(rule["w"]))
    po_of = {}
    for t in np.flatnonzero(rule["face"]):
        o = tuple(int(x) for x in rule["cell"][t])
        if o not in po_of:
            po_of[o] = cell_photo_out(pkg, orc, otables, case, key, ns, o)
        terms[t] = po_of[o] * float(rule["w"][t])
    return terms, rule
