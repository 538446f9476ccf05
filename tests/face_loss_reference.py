"""Reference for the escape maps (c2r_enable_face_loss), shared by tests/test_face_loss_host.py (CPU) and
tests/test_gpu_face_loss.py (GPU).  Not a test module.

The expected maps come from the oracle alone.  For each point source on its own: orc.do_source on the periodic embedding of
tests/open_boundary_cases.py / tests/axis_boundary_cases.py leaves coldensh_out / coldenshe_out of every cell it traced (the
cells of the product's final sub-box, by the argument of those files; coldensh_out != 0 is the reference's own marker);
for every such cell of the region on an open mesh face orc_cinterp gives the incoming columns and the path, the fog rule of
evolve_point.F90:177-180 is applied if LLS is on, orc_photoion_rates / orc_photoion_rates3 give photo_out, the term is
photo_out * vol / vol_ph (evolve_point.F90:310-315), and a NumPy restatement of the attribution rule of include/c2ray_hip.h
puts it into a face's map.  The sources are added in source order, map = map + terms (adding 0.0 changes no bit).
"""
import ctypes as C
import math

import numpy as np

MAX_COLDENSH = float(np.float32(2e29))


def geometry(case):
    """(n, m, periodic) as 3-tuples for an open_boundary_cases.Case or an axis_boundary_cases.AxisCase."""
    if isinstance(case.n, (int, np.integer)):
        return (int(case.n),) * 3, (int(case.m),) * 3, (False, False, False)
    return tuple(int(x) for x in case.n), tuple(int(x) for x in case.m), tuple(bool(p) for p in case.periodic)


def face_shape(n, face):
    """NumPy shape [b, a] of a face's map: a the lower of the two remaining axes (fastest)."""
    a, b = [d for d in range(3) if d != face // 2]
    return n[b], n[a]


def open_faces(periodic):
    return [f for f in range(6) if not periodic[f // 2]]


def attribute(n, periodic, m1, o, dr):
    """The rule: m1 the cell's 1-based mesh indices, o its offset from the source.  The face, or None."""
    cand = []
    for d in range(3):
        if periodic[d]:
            continue
        if m1[d] == 1:
            cand.append(2 * d)
        if m1[d] == n[d]:
            cand.append(2 * d + 1)
    if not cand:
        return None
    weight = lambda f: float(abs(int(o[f // 2]))) * float(dr[f // 2])
    # the largest |o_d| dr_d; on a tie the lowest axis, within one axis low before high: the lowest face number
    return min(cand, key=lambda f: (-weight(f), f))


def face_cell(n, face, m1):
    """Index of the cell with 1-based mesh indices m1 in the map of `face` (flat, the lower remaining axis fastest)."""
    a, b = [d for d in range(3) if d != face // 2]
    return (m1[a] - 1) + n[a] * (m1[b] - 1)


def _oracle_run(pkg, orc, otables, case, ns, coldensh_lls):
    """do_source of source ns (0-based) alone on the case's periodic embedding: (step, state, nbox)."""
    hp = pkg.hostphys
    _, m, _ = geometry(case)
    nd, xh, xhe, temp = case.big
    kw = {}
    if case.pl is not None:
        kw = dict(normflux_pl=case.pl[[ns]], normflux_qpl=case.qpl[[ns]], pl_s_star=case.pl_s_star, qpl_s_star=case.qpl_s_star)
    st = orc.Step(m, case.dr, case.vol, 9.0, hp.H0, hp.Omega0, not case.heat, 1.0e4, 1.0, case.srcpos[[ns]], case.flux[[ns]],
                  case.s_star, nd, case.reccoef, coldensh_lls=coldensh_lls, **kw)
    s = orc.State(st, xh, xhe, temp)
    orc.begin_step(s)
    nbox, _ = orc.do_source(otables, st, s, 1)
    return st, s, nbox


def source_terms(pkg, orc, otables, case, ns, coldensh_lls=None):
    """[(m1, o, term)] for every traced cell of the region on an open mesh face, source ns (0-based) alone."""
    n, m, periodic = geometry(case)
    st, s, _ = _oracle_run(pkg, orc, otables, case, ns, coldensh_lls)
    consts = orc.constants()
    pi, eps = float(consts[0]), float(consts[30])
    dr = [float(x) for x in case.dr]
    vol = float(case.vol)
    src = [int(x) for x in case.srcpos[ns]]
    nf = [float(case.flux[ns]), 0.0 if case.pl is None else float(case.pl[ns]), 0.0 if case.qpl is None else float(case.qpl[ns])]
    multi = case.pl is not None
    ncell_m = m[0] * m[1] * m[2]
    cH, cHe = s.coldensh_out, s.coldenshe_out
    ip = C.POINTER(C.c_int)
    dp = C.POINTER(C.c_double)
    mesh_m = np.array(m, dtype=np.int32)
    src_a = np.array(src, dtype=np.int32)
    lib = orc.lib()
    out = []
    for k in range(1, n[2] + 1):
        for j in range(1, n[1] + 1):
            for i in range(1, n[0] + 1):
                m1 = (i, j, k)
                if not any((not periodic[d]) and (m1[d] == 1 or m1[d] == n[d]) for d in range(3)):
                    continue
                q = (i - 1) + m[0] * ((j - 1) + m[1] * (k - 1))
                if cH[q] == 0.0:        # not traced: outside the source's final sub-box
                    continue
                o = []
                for d in range(3):
                    if periodic[d]:     # the image within the periodic reach [-(n/2), n/2 - 1 + n mod 2]
                        h = n[d] // 2
                        o.append((m1[d] - src[d] + h) % n[d] - h)
                    else:
                        o.append(m1[d] - src[d])
                if o == [0, 0, 0]:
                    cin = [0.0, 0.0, 0.0]
                    vol_ph = dr[0] * dr[1] * dr[2]
                else:
                    pos = np.array([src[d] + o[d] for d in range(3)], dtype=np.int32)
                    a, b, c, p = C.c_double(), C.c_double(), C.c_double(), C.c_double()
                    lib.orc_cinterp(mesh_m.ctypes.data_as(ip), cH.ctypes.data_as(dp), cHe.ctypes.data_as(dp), pos.ctypes.data_as(ip),
                                    src_a.ctypes.data_as(ip), C.byref(a), C.byref(b), C.byref(c), C.byref(p))
                    cin = [a.value, b.value, c.value]
                    path = p.value * dr[0]
                    xs, ys, zs = dr[0] * float(o[0]), dr[1] * float(o[1]), dr[2] * float(o[2])
                    dist2 = xs * xs + ys * ys + zs * zs
                    vol_ph = 4.0 * pi * dist2 * path
                    if coldensh_lls is not None:
                        cin[0] = cin[0] + float(coldensh_lls) * path / dr[0]
                term = 0.0
                if cin[0] < MAX_COLDENSH:
                    cols6 = [cin[0], float(cH[q]), cin[1], float(cHe[q]), cin[2], float(cHe[q + ncell_m])]
                    i_state = max(float(s.xh_av[q + ncell_m]), eps)
                    if multi:
                        r = orc.PhotRates()
                        lib.orc_photoion_rates3(C.byref(otables.c), *[C.c_double(x) for x in cols6], C.c_double(vol_ph), (C.c_double * 3)(*nf),
                                                C.c_double(i_state), C.c_int(0 if case.heat else 1), C.byref(r))
                        p_out = r.photo_out
                    else:
                        p_out = orc.photoion_rates(otables, cols6, vol_ph, nf[0], i_state, not case.heat)[20]
                    term = p_out * vol / vol_ph
                out.append((m1, tuple(o), term))
    return out


def maps_of_terms(case, terms):
    """The terms of one source put into the maps of the open faces by the rule: {face: flat array}."""
    n, _, periodic = geometry(case)
    maps = {f: np.zeros(face_shape(n, f)[0] * face_shape(n, f)[1]) for f in open_faces(periodic)}
    for m1, o, term in terms:
        f = attribute(n, periodic, m1, o, case.dr)
        assert f is not None
        maps[f][face_cell(n, f, m1)] = term      # a cell appears once per source
    return maps


_cache = {}


def expected(pkg, orc, otables, case, key, sources=None, coldensh_lls=None):
    """{face: map of shape [b, a]} for the sources `sources` (0-based, default all) added in that order, and the per-source
    maps.  `key` names the case (results are computed once per session and never changed by a caller: copies go out)."""
    n, _, periodic = geometry(case)
    idx = list(range(len(case.flux))) if sources is None else [int(x) for x in sources]
    per_source = []
    for ns in idx:
        k = (key, ns, coldensh_lls)
        if k not in _cache:
            terms = source_terms(pkg, orc, otables, case, ns, coldensh_lls)
            _cache[k] = (maps_of_terms(case, terms), terms)
        per_source.append(_cache[k][0])
    total = {f: np.zeros(face_shape(n, f)[0] * face_shape(n, f)[1]) for f in open_faces(periodic)}
    for one in per_source:
        for f in total:
            total[f] = total[f] + one[f]
    shaped = {f: total[f].reshape(face_shape(n, f)) for f in total}
    return shaped, [{f: one[f].reshape(face_shape(n, f)).copy() for f in one} for one in per_source]


def cached_terms(key, ns, coldensh_lls=None):
    """The (m1, o, term) list behind expected()'s maps of source ns: expected() must have been called for it."""
    return _cache[(key, ns, coldensh_lls)][1]


def total_of(maps):
    return math.fsum(float(x) for a in maps.values() for x in np.asarray(a).reshape(-1))
