"""Reference for tilted plane-parallel sources (c2r_set_plane_tilt), shared by tests/test_oblique_reference_host.py (CPU) and
tests/test_gpu_oblique_planes.py (GPU).  Not a test module.

The rule of include/c2ray_hip.h in plain Python floats (IEEE doubles, every product and sum from the left, as written
there): the layers of the march in travel order, the incoming columns of a cell cinterp's weighted mean over four cells of
the layer before with the weights of a source at infinity, and behind that the normal plane's cell (tests/plane_reference.py)
with path = dr[axis] * sqrt(1 + tilt^2) -- per cell the oracle's photoion_rates / orc_photoion_rates3, called exactly as
the normal plane's reference calls them.  The sigmas of weightf are the oracle's own (oracle.constants()).
"""
import math

import numpy as np

from plane_reference import MAX_COLDENSH, _photoion, constants, face_axes


def geometry(tilt, dr, axis):
    """a_f, a_g, (s1, s2, s3, s4), path, e_f, e_g -- host doubles, as the header forms them."""
    f, g = face_axes(axis)
    t0, t1 = float(tilt[0]), float(tilt[1])
    a_f = (abs(t0) * float(dr[axis])) / float(dr[f])
    a_g = (abs(t1) * float(dr[axis])) / float(dr[g])
    s = (a_f * a_g, (1.0 - a_f) * a_g, a_f * (1.0 - a_g), (1.0 - a_f) * (1.0 - a_g))
    path = float(dr[axis]) * math.sqrt(1.0 + (t0 * t0 + t1 * t1))
    return a_f, a_g, s, path, (1 if t0 > 0 else -1), (1 if t1 > 0 else -1)


def _upstream(u, e, n, wrap):
    uu = u - e
    if 0 <= uu < n:
        return uu
    return uu % n if wrap else -1


def _interp(s, c, sig):
    w = [s[i] * (1.0 / max(0.6, c[i] * sig)) for i in range(4)]
    return (c[0] * w[0] + c[1] * w[1] + c[2] * w[2] + c[3] * w[3]) / (w[0] + w[1] + w[2] + w[3])


def oblique_pass(orc, otables, mesh, dr, vol, ndens, xh_av, xhe_av, axis, from_high, normflux, tilt, periodic=(False, False, False),
                 heat=False, coldensh_lls=None, lls_grid=None, entry=None):
    """One tilted plane over the whole mesh, from zeroed rate grids.  Arguments as plane_reference.plane_pass, plus tilt (two
    tangents, towards the two face axes, the lower axis first) and periodic (per mesh axis; the plane's own axis is open).
    Returns phih_grid, phihe_grid (2 ncell), phiheat, exit (3 x face), terms (face: each line's loss term), loss (their
    math.fsum) and cin_HI (ncell, the fogged incoming HI column of every cell)."""
    assert float(tilt[0]) != 0.0 or float(tilt[1]) != 0.0, "zero tilt is the normal plane: plane_reference.plane_pass"
    abu_he, eps = constants(orc)
    sig = [float(x) for x in orc.constants()[19:22]]
    mesh = [int(x) for x in mesh]
    n = mesh[0] * mesh[1] * mesh[2]
    nf = [float(x) for x in np.atleast_1d(np.asarray(normflux, dtype=np.float64))]
    nf = (nf + [0.0, 0.0])[:3]
    multi = nf[1] != 0.0 or nf[2] != 0.0
    use_lls = coldensh_lls is not None or lls_grid is not None
    f_ax, g_ax = face_axes(axis)
    fa, fb, na = mesh[f_ax], mesh[g_ax], mesh[axis]
    face = fa * fb
    stride = [1, mesh[0], mesh[0] * mesh[1]]
    a_f, a_g, s, path, e_f, e_g = geometry(tilt, dr, axis)
    assert 0.0 <= a_f <= 1.0 and 0.0 <= a_g <= 1.0, (a_f, a_g)
    wrap_f, wrap_g = bool(periodic[f_ax]), bool(periodic[g_ax])
    dr0, vol = float(dr[0]), float(vol)
    nd, xh, xhe = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (ndens, xh_av, xhe_av))
    phih, phihe, phiheat = np.zeros(n), np.zeros(2 * n), np.zeros(n)
    terms, cin_grid = np.zeros(face), np.zeros(n)
    zero = [0.0] * face
    prev = [zero, zero, zero] if entry is None else [[float(x) for x in np.asarray(entry)[k * face:(k + 1) * face]] for k in range(3)]
    for m in range(na):
        along = na - 1 - m if from_high else m
        nxt = [[0.0] * face for _ in range(3)]
        for v in range(fb):
            vv = _upstream(v, e_g, fb, wrap_g)
            for u in range(fa):
                uu = _upstream(u, e_f, fa, wrap_f)
                at = (uu + fa * vv if uu >= 0 and vv >= 0 else -1, u + fa * vv if vv >= 0 else -1, uu + fa * v if uu >= 0 else -1,
                      u + fa * v)                                                 # c1 .. c4
                cin = [_interp(s, [prev[k][i] if i >= 0 else 0.0 for i in at], sig[k]) for k in range(3)]
                q = u * stride[f_ax] + v * stride[g_ax] + along * stride[axis]
                ndq = float(nd[q])
                u_HI = max(float(xh[q]), eps) * ndq
                u_HeI = max(float(xhe[q]), eps) * ndq
                u_HeII = max(float(xhe[q + n]), eps) * ndq
                if use_lls:
                    lls = float(lls_grid[q]) if lls_grid is not None else float(coldensh_lls)
                    cin[0] = cin[0] + lls * path / dr0
                cout = [cin[0] + u_HI * path * (1.0 - abu_he), cin[1] + u_HeI * path * abu_he, cin[2] + u_HeII * path * abu_he]
                cin_grid[q] = cin[0]
                term = 0.0
                if cin[0] < MAX_COLDENSH:
                    cols6 = [cin[0], cout[0], cin[1], cout[1], cin[2], cout[2]]
                    p_HI, p_HeI, p_HeII, h, p_out = _photoion(orc, otables, cols6, path, nf, multi, max(float(xh[q + n]), eps), heat)
                    phih[q] = phih[q] + p_HI / (u_HI * (1.0 - abu_he))
                    phihe[q] = phihe[q] + p_HeI / (u_HeI * abu_he)
                    phihe[q + n] = phihe[q + n] + p_HeII / (u_HeII * abu_he)
                    if heat:
                        phiheat[q] = phiheat[q] + h
                    term = p_out * vol / path
                fc = u + fa * v
                for k in range(3):
                    nxt[k][fc] = cout[k]
                if m == na - 1:
                    terms[fc] = term
        prev = nxt
    exit3 = np.array(prev[0] + prev[1] + prev[2])
    return dict(phih_grid=phih, phihe_grid=phihe, phiheat=phiheat, exit=exit3, terms=terms, loss=math.fsum(terms), cin_HI=cin_grid)
