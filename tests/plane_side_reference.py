"""Reference for the side faces of a tilted plane (c2r_set_plane_side_entry, c2r_enable_plane_side_exit,
c2r_enable_plane_side_loss), shared by tests/test_plane_side_host.py (CPU) and tests/test_gpu_plane_sides.py (GPU).  Not a
test module.

flux_reference.flux_pass / oblique_reference.oblique_pass (and plane_curve_reference.curve_pass' factor per layer) with ghost
strips in, strips out and the side terms per side-face cell, following the rule of include/c2ray_hip.h in plain Python floats:
  side entry  a corner outside an open face axis on a live side reads slot m of that side's strip (or of the corner line)
              instead of 0.0, columns and -- for a plane with a map -- fluxes;
  side exit   slot m of a live side holds, for its downstream edge cells, the columns and the flux of the layer before layer m;
  side loss   a cell of a layer m <= na-2 gives base * w_s to side s, base its photo_out*vol/path, w_0 = s3 + s1 and
              w_1 = s2 + s1, or s2 alone where side 0 takes the diagonal target.
Strips are arrays of shape (na, 3, L): L = fb for side 0, fa for side 1, 1 for the corner line (side 2).
"""
import math

import numpy as np

from oblique_reference import _interp, _upstream, geometry
from plane_curve_reference import layer_factor
from plane_reference import MAX_COLDENSH, _photoion, constants, face_axes


def live_sides(tilt, periodic, axis):
    """(side 0 live, side 1 live): the tilt component is non-zero and the face axis open."""
    f_ax, g_ax = face_axes(axis)
    return (float(tilt[0]) != 0.0 and not periodic[f_ax], float(tilt[1]) != 0.0 and not periodic[g_ax])


def downstream_edge(e, n):
    return n - 1 if e > 0 else 0


def side_face(axis, side, e):
    """The mesh face (2 * axis + high) the beam leaves through on `side` of a plane along `axis`."""
    return 2 * face_axes(axis)[side] + (1 if e > 0 else 0)


def side_of_target(fa, fb, wrap_f, wrap_g, tu, tv):
    """The side a displaced target gives its weight to: 0 outside along f (also when outside along g too), 1 outside along g
    only, -1 inside the mesh; an index on a periodic axis wraps and is never outside."""
    out_f = not wrap_f and not 0 <= tu < fa
    out_g = not wrap_g and not 0 <= tv < fb
    return 0 if out_f else (1 if out_g else -1)


def side_weights(s, e_f, e_g, fa, fb, wrap_f, wrap_g, u, v):
    """(w_0, w_1) of cell (u, v): the targets (u+e_f, v+e_g), (u, v+e_g), (u+e_f, v) carry s1, s2, s3."""
    diag = side_of_target(fa, fb, wrap_f, wrap_g, u + e_f, v + e_g)
    w0 = s[2] + s[0] if side_of_target(fa, fb, wrap_f, wrap_g, u + e_f, v) == 0 else 0.0
    w1 = 0.0
    if side_of_target(fa, fb, wrap_f, wrap_g, u, v + e_g) == 1:
        w1 = s[1] + s[0] if diag == 1 else s[1]
    return w0, w1


def _strip(ghost, kind, side, na, line):
    """The strip `side` of ghost[kind] as a (na, 3, line) array, or None."""
    a = None if ghost is None else (ghost.get(kind) or {}).get(side)
    return None if a is None else np.asarray(a, dtype=np.float64).reshape(na, 3, line)


def side_pass(orc, otables, mesh, dr, vol, ndens, xh_av, xhe_av, axis, from_high, tilt, flux_map=None, normflux=None,
              periodic=(False, False, False), heat=False, coldensh_lls=None, lls_grid=None, entry=None, ghost=None, curve=None, rates=True):
    """One tilted plane over the whole mesh, from zeroed rate grids.  flux_map (3 x face) or normflux (uniform); ghost: None or
    {"cols": {side: strip}, "flux": {side: strip}} with side 0, 1, 2; curve as plane_curve_reference.curve_pass takes it;
    rates=False marches the flux only (no oracle needed; orc, otables, ndens .. may be None).
    Returns flux_pass' dictionary plus live (2), side_cols / side_flux (per side: (na, 3, L), None for a side that is not live;
    side_flux None without a map), side_terms (per side: the terms in the order of the side face's map, None where not live),
    side_loss (their math.fsum, 0.0 where not live), weights (na-1 layers' (w_0, w_1) per face cell: (2, face)) and
    all_terms (na x face: photo_out*vol/path of every cell)."""
    mesh = [int(x) for x in mesh]
    n = mesh[0] * mesh[1] * mesh[2]
    f_ax, g_ax = face_axes(axis)
    fa, fb, na = mesh[f_ax], mesh[g_ax], mesh[axis]
    face = fa * fb
    mapped = flux_map is not None
    if mapped:
        fm = np.asarray(flux_map, dtype=np.float64).reshape(3, face)
    else:
        nf0 = [float(x) for x in np.atleast_1d(np.asarray(normflux, dtype=np.float64))]
        nf0 = (nf0 + [0.0, 0.0])[:3]
        fm = np.repeat(np.array(nf0)[:, None], face, axis=1)
    assert float(tilt[0]) != 0.0 or float(tilt[1]) != 0.0
    a_f, a_g, s, path, e_f, e_g = geometry(tilt, dr, axis)
    assert 0.0 <= a_f <= 1.0 and 0.0 <= a_g <= 1.0, (a_f, a_g)
    wrap_f, wrap_g = bool(periodic[f_ax]), bool(periodic[g_ax])
    live = live_sides(tilt, periodic, axis)
    ghost_live = (live[0], live[1], live[0] and live[1])
    lines = (fb, fa, 1)
    gcols = [_strip(ghost, "cols", k, na, lines[k]) if ghost_live[k] else None for k in range(3)]
    gflux = [_strip(ghost, "flux", k, na, lines[k]) if ghost_live[k] and mapped else None for k in range(3)]
    multi = bool(fm[1].any() or fm[2].any())
    if mapped:   # a SET flux strip counts, live or not
        for k in range(3):
            a = _strip(ghost, "flux", k, na, lines[k])
            multi = multi or (a is not None and bool(a[:, 1:].any()))
    edge = (downstream_edge(e_f, fa), downstream_edge(e_g, fb))
    factors = [layer_factor(curve, m, path) for m in range(na)]
    stride = [1, mesh[0], mesh[0] * mesh[1]]
    use_lls = coldensh_lls is not None or lls_grid is not None
    dr0, vol = float(dr[0]), float(vol)
    if rates:
        abu_he, eps = constants(orc)
        sig = [float(x) for x in orc.constants()[19:22]]
        nd, xh, xhe = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (ndens, xh_av, xhe_av))
    phih, phihe, phiheat = np.zeros(n), np.zeros(2 * n), np.zeros(n)
    terms, cin_grid, all_terms = np.zeros(face), np.zeros(n), np.zeros((na, face))
    zero = [0.0] * face
    prev = [zero, zero, zero] if entry is None else [[float(x) for x in np.asarray(entry)[k * face:(k + 1) * face]] for k in range(3)]
    fl = [[float(x) for x in fm[k]] for k in range(3)]
    layers = []
    side_cols = [np.zeros((na, 3, lines[k])) if live[k] else None for k in range(2)]
    side_flux = [np.zeros((na, 3, lines[k])) if live[k] and mapped else None for k in range(2)]
    # the side faces' maps: mesh order of the two axes that remain beside the side's axis, the lower fastest
    side_axes = (f_ax, g_ax)
    side_terms = [np.zeros(n // mesh[side_axes[k]]) if live[k] else None for k in range(2)]

    def corner(layer, strips, m, k, uu, vv):
        if uu >= 0 and vv >= 0:
            return layer[k][uu + fa * vv]
        if vv >= 0:
            return float(strips[0][m, k, vv]) if strips[0] is not None else 0.0
        if uu >= 0:
            return float(strips[1][m, k, uu]) if strips[1] is not None else 0.0
        return float(strips[2][m, k, 0]) if strips[2] is not None else 0.0

    weights = np.zeros((2, face))
    for v in range(fb):
        for u in range(fa):
            weights[:, u + fa * v] = side_weights(s, e_f, e_g, fa, fb, wrap_f, wrap_g, u, v)
    for m in range(na):
        along = na - 1 - m if from_high else m
        cf = factors[m]
        # side exit: the edge cells of the layer before, columns and flux, before anything of this layer is formed
        for k in range(3):
            if live[0]:
                side_cols[0][m, k] = [prev[k][edge[0] + fa * t] for t in range(fb)]
                if mapped:
                    side_flux[0][m, k] = [fl[k][edge[0] + fa * t] for t in range(fb)]
            if live[1]:
                side_cols[1][m, k] = [prev[k][t + fa * edge[1]] for t in range(fa)]
                if mapped:
                    side_flux[1][m, k] = [fl[k][t + fa * edge[1]] for t in range(fa)]
        if mapped:   # the flux of this layer from the layer before (the map in front of the first), ghosts included
            nfl = [[0.0] * face for _ in range(3)]
            for v in range(fb):
                vv = _upstream(v, e_g, fb, wrap_g)
                for u in range(fa):
                    uu = _upstream(u, e_f, fa, wrap_f)
                    for k in range(3):
                        F = [corner(fl, gflux, m, k, uu, vv), corner(fl, gflux, m, k, u, vv), corner(fl, gflux, m, k, uu, v), fl[k][u + fa * v]]
                        nfl[k][u + fa * v] = F[0] * s[0] + F[1] * s[1] + F[2] * s[2] + F[3] * s[3]
            fl = nfl
        layers.append(np.array(fl))
        if not rates:
            continue
        nxt = [[0.0] * face for _ in range(3)]
        for v in range(fb):
            vv = _upstream(v, e_g, fb, wrap_g)
            for u in range(fa):
                fc = u + fa * v
                uu = _upstream(u, e_f, fa, wrap_f)
                cin = [_interp(s, [corner(prev, gcols, m, k, uu, vv), corner(prev, gcols, m, k, u, vv), corner(prev, gcols, m, k, uu, v),
                                   prev[k][fc]], sig[k]) for k in range(3)]
                idx = [0, 0, 0]
                idx[f_ax], idx[g_ax], idx[axis] = u, v, along
                q = idx[0] * stride[0] + idx[1] * stride[1] + idx[2] * stride[2]
                ndq = float(nd[q])
                u_HI = max(float(xh[q]), eps) * ndq
                u_HeI = max(float(xhe[q]), eps) * ndq
                u_HeII = max(float(xhe[q + n]), eps) * ndq
                if use_lls:
                    lls = float(lls_grid[q]) if lls_grid is not None else float(coldensh_lls)
                    cin[0] = cin[0] + lls * path / dr0
                cout = [cin[0] + u_HI * path * (1.0 - abu_he), cin[1] + u_HeI * path * abu_he, cin[2] + u_HeII * path * abu_he]
                cin_grid[q] = cin[0]
                nfu = [fl[0][fc], fl[1][fc], fl[2][fc]]
                skip = (nfu[0] == 0.0 and nfu[1] == 0.0 and nfu[2] == 0.0) or cf == 0.0
                term = 0.0
                if not skip and cin[0] < MAX_COLDENSH:
                    nf = [nfu[0] * cf, nfu[1] * cf, nfu[2] * cf] if curve is not None else nfu
                    cols6 = [cin[0], cout[0], cin[1], cout[1], cin[2], cout[2]]
                    p_HI, p_HeI, p_HeII, h, p_out = _photoion(orc, otables, cols6, path, nf, multi, max(float(xh[q + n]), eps), heat)
                    phih[q] = phih[q] + p_HI / (u_HI * (1.0 - abu_he))
                    phihe[q] = phihe[q] + p_HeI / (u_HeI * abu_he)
                    phihe[q + n] = phihe[q + n] + p_HeII / (u_HeII * abu_he)
                    if heat:
                        phiheat[q] = phiheat[q] + h
                    term = p_out * vol / path
                for k in range(3):
                    nxt[k][fc] = cout[k]
                all_terms[m, fc] = term
                if m == na - 1:
                    terms[fc] = term
                else:        # the side terms, at the face cell behind which this edge cell lies
                    for side in range(2):
                        on_edge = (u == edge[0]) if side == 0 else (v == edge[1])
                        if live[side] and on_edge:
                            rest = [d for d in range(3) if d != side_axes[side]]
                            side_terms[side][idx[rest[0]] + mesh[rest[0]] * idx[rest[1]]] = term * weights[side, fc]
        prev = nxt
    exit3 = np.array(prev[0] + prev[1] + prev[2])
    return dict(phih_grid=phih, phihe_grid=phihe, phiheat=phiheat, exit=exit3, terms=terms, loss=math.fsum(terms), cin_HI=cin_grid,
                exit_flux=np.array(fl[0] + fl[1] + fl[2]), layer_flux=np.array(layers), factors=np.array(factors), live=live,
                side_cols=side_cols, side_flux=side_flux, side_terms=side_terms,
                side_loss=[math.fsum(t) if t is not None else 0.0 for t in side_terms], weights=weights, all_terms=all_terms)


# -- tiles: a mesh cut across its face axes, the pieces handing the beam to each other ------------------------------------------
def box_cells(mesh, lo, hi):
    """The 0-based cell numbers (i fastest) of the box lo <= index < hi of `mesh`, in the box's own mesh order."""
    i, j, k = (np.arange(lo[d], hi[d]) for d in range(3))
    return (i[None, None, :] + mesh[0] * (j[None, :, None] + mesh[1] * k[:, None, None])).reshape(-1)


def box_field(mesh, lo, hi, a):
    """The part of a field of c components (c x ncell, components slowest) that lies in the box, in the same layout."""
    n = int(np.prod(mesh))
    a = np.asarray(a)
    return np.ascontiguousarray(a.reshape(-1, n)[:, box_cells(mesh, lo, hi)]).reshape(-1)


def box_face(mesh, axis, lo, hi, a):
    """The part of a face field across `axis` (c x face, components slowest) that lies behind the box."""
    f_ax, g_ax = face_axes(axis)
    fa, fb = mesh[f_ax], mesh[g_ax]
    idx = (np.arange(lo[f_ax], hi[f_ax])[None, :] + fa * np.arange(lo[g_ax], hi[g_ax])[:, None]).reshape(-1)
    return np.ascontiguousarray(np.asarray(a).reshape(-1, fa * fb)[:, idx]).reshape(-1)


def tiled(mesh, axis, tilt, cut_f, cut_g, run):
    """Cut `mesh` across the face axes of a plane along `axis` at the 0-based indices cut_f, cut_g (None: no cut) and run the
    tiles from upstream to downstream: run(lo, hi, ghost) returns a dictionary with side_cols and side_flux (per side 0, 1:
    a (na, 3, L) strip or None), ghost is what set_plane_side_entry takes, {"cols": {side: strip}, "flux": {side: strip}},
    assembled from the upstream neighbours' strips and, for the corner line, from the diagonal neighbour's side 0 strip.
    Returns {(i_f, i_g): (lo, hi, result)}."""
    f_ax, g_ax = face_axes(axis)
    e = (1 if float(tilt[0]) > 0 else -1, 1 if float(tilt[1]) > 0 else -1)
    cuts = [[0, mesh[f_ax]] if cut_f is None else [0, cut_f, mesh[f_ax]], [0, mesh[g_ax]] if cut_g is None else [0, cut_g, mesh[g_ax]]]
    order = [list(range(len(c) - 1))[::e[k]] for k, c in enumerate(cuts)]
    out = {}
    for ig in order[1]:
        for i_f in order[0]:
            lo, hi = [0, 0, 0], list(mesh)
            lo[f_ax], hi[f_ax] = cuts[0][i_f], cuts[0][i_f + 1]
            lo[g_ax], hi[g_ax] = cuts[1][ig], cuts[1][ig + 1]
            nb_f, nb_g, nb_d = out.get((i_f - e[0], ig)), out.get((i_f, ig - e[1])), out.get((i_f - e[0], ig - e[1]))
            ghost = {"cols": {}, "flux": {}}
            for kind, key in (("cols", "side_cols"), ("flux", "side_flux")):
                if nb_f is not None and nb_f[2][key] is not None and nb_f[2][key][0] is not None:
                    ghost[kind][0] = nb_f[2][key][0]
                if nb_g is not None and nb_g[2][key] is not None and nb_g[2][key][1] is not None:
                    ghost[kind][1] = nb_g[2][key][1]
                if nb_d is not None and nb_d[2][key] is not None and nb_d[2][key][0] is not None:
                    strip = nb_d[2][key][0]                      # the diagonal tile's f edge, at its downstream edge along g
                    ghost[kind][2] = strip[:, :, (strip.shape[2] - 1 if e[1] > 0 else 0):][:, :, :1]
            out[(i_f, ig)] = (lo, hi, run(lo, hi, ghost))
    return out
