"""Reference for plane flux maps (c2r_set_plane_flux_map), shared by tests/test_flux_reference_host.py (CPU) and
tests/test_gpu_plane_flux_maps.py (GPU).  Not a test module.

plane_reference.plane_pass and oblique_reference.oblique_pass with one more argument, flux_map (3 x face, SED slowest, the
face cells in the order of the entry columns), following the rule of include/c2ray_hip.h in plain Python floats: at normal
incidence every cell of line f takes map[k][f]; on a tilted plane the flux of a cell is F1*s1 + F2*s2 + F3*s3 + F4*s4 over
the corners the columns use, every product rounded, the sums from the left, zero from outside an open side face; a cell
whose three fluxes are all == 0.0 is skipped.  Per cell the oracle's photoion_rates / orc_photoion_rates3, called exactly
as those two modules call them.  The three-SED routine is taken iff some entry of SED 1 or 2 of the MAP is non-zero.
"""
import math

import numpy as np

from oblique_reference import _interp, _upstream, geometry
from plane_reference import MAX_COLDENSH, _photoion, constants, face_axes


def advect(s, fa, fb, e_f, e_g, wrap_f, wrap_g, prev):
    """One layer of the flux march: prev and the result are three lists of face floats."""
    nxt = [[0.0] * (fa * fb) for _ in range(3)]
    for v in range(fb):
        vv = _upstream(v, e_g, fb, wrap_g)
        for u in range(fa):
            uu = _upstream(u, e_f, fa, wrap_f)
            at = (uu + fa * vv if uu >= 0 and vv >= 0 else -1, u + fa * vv if vv >= 0 else -1, uu + fa * v if uu >= 0 else -1, u + fa * v)
            for k in range(3):
                F = [prev[k][i] if i >= 0 else 0.0 for i in at]
                nxt[k][u + fa * v] = F[0] * s[0] + F[1] * s[1] + F[2] * s[2] + F[3] * s[3]
    return nxt


def flux_pass(orc, otables, mesh, dr, vol, ndens, xh_av, xhe_av, axis, from_high, flux_map, tilt=None, periodic=(False, False, False),
              heat=False, coldensh_lls=None, lls_grid=None, entry=None, rates=True):
    """One plane with a flux map over the whole mesh, from zeroed rate grids.  tilt None or (0, 0): normal incidence
    (plane_pass' march), else oblique_pass' layers.  rates=False marches the flux only (no oracle needed).
    Returns what those two return, plus exit_flux (3 x face) and layer_flux (mesh[axis] x 3 x face: the flux the cells of
    every layer saw, in travel order)."""
    mesh = [int(x) for x in mesh]
    n = mesh[0] * mesh[1] * mesh[2]
    f_ax, g_ax = face_axes(axis)
    fa, fb, na = mesh[f_ax], mesh[g_ax], mesh[axis]
    face = fa * fb
    fm = np.asarray(flux_map, dtype=np.float64).reshape(3, face)
    multi = bool(fm[1].any() or fm[2].any())
    tilted = tilt is not None and (float(tilt[0]) != 0.0 or float(tilt[1]) != 0.0)
    if tilted:
        a_f, a_g, s, path, e_f, e_g = geometry(tilt, dr, axis)
        assert 0.0 <= a_f <= 1.0 and 0.0 <= a_g <= 1.0, (a_f, a_g)
        wrap_f, wrap_g = bool(periodic[f_ax]), bool(periodic[g_ax])
    else:
        path = float(dr[axis])
    stride = [1, mesh[0], mesh[0] * mesh[1]]
    use_lls = coldensh_lls is not None or lls_grid is not None
    dr0, vol = float(dr[0]), float(vol)
    if rates:
        abu_he, eps = constants(orc)
        sig = [float(x) for x in orc.constants()[19:22]]
        nd, xh, xhe = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (ndens, xh_av, xhe_av))
    phih, phihe, phiheat = np.zeros(n), np.zeros(2 * n), np.zeros(n)
    terms, cin_grid = np.zeros(face), np.zeros(n)
    zero = [0.0] * face
    prev = [zero, zero, zero] if entry is None else [[float(x) for x in np.asarray(entry)[k * face:(k + 1) * face]] for k in range(3)]
    fl = [[float(x) for x in fm[k]] for k in range(3)]
    layers = []
    for m in range(na):
        along = na - 1 - m if from_high else m
        if tilted:
            fl = advect(s, fa, fb, e_f, e_g, wrap_f, wrap_g, fl)
        layers.append(np.array(fl))
        if not rates:
            continue
        nxt = [[0.0] * face for _ in range(3)]
        for v in range(fb):
            vv = _upstream(v, e_g, fb, wrap_g) if tilted else v
            for u in range(fa):
                fc = u + fa * v
                if tilted:
                    uu = _upstream(u, e_f, fa, wrap_f)
                    at = (uu + fa * vv if uu >= 0 and vv >= 0 else -1, u + fa * vv if vv >= 0 else -1, uu + fa * v if uu >= 0 else -1, fc)
                    cin = [_interp(s, [prev[k][i] if i >= 0 else 0.0 for i in at], sig[k]) for k in range(3)]
                else:
                    cin = [prev[k][fc] for k in range(3)]
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
                nf = [fl[0][fc], fl[1][fc], fl[2][fc]]
                dark = nf[0] == 0.0 and nf[1] == 0.0 and nf[2] == 0.0
                term = 0.0
                if not dark and cin[0] < MAX_COLDENSH:
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
                if m == na - 1:
                    terms[fc] = term
        prev = nxt
    exit3 = np.array(prev[0] + prev[1] + prev[2])
    return dict(phih_grid=phih, phihe_grid=phihe, phiheat=phiheat, exit=exit3, terms=terms, loss=math.fsum(terms), cin_HI=cin_grid,
                exit_flux=np.array(fl[0] + fl[1] + fl[2]), layer_flux=np.array(layers))
