"""Reference for plane light curves (c2r_set_plane_curve), shared by tests/test_plane_curve_host.py (CPU) and
tests/test_gpu_plane_curves.py (GPU).  Not a test module.

The march of flux_reference.flux_pass restated with the rule of include/c2ray_hip.h in plain Python floats: for layer m in
travel order
    d = depth0 + (float(layer0 + m) + 0.5) * path
    b = the number of k < nstep with d > depth[k]
    f = factor[b]
a cell of a layer with f == 0.0, or whose unscaled fluxes are all == 0.0, is skipped; any other cell gets nf[k]*f, one
rounded product per SED, where nf is the plane's uniform normflux, its map entry or the flux a tilted march carried to the
cell (the carried flux and the exit flux stay unscaled).  Per cell the oracle's photoion_rates / orc_photoion_rates3 through
plane_reference._photoion.  The three-SED routine is taken iff the UNSCALED normflux or map has a non-zero entry of SED 1 or 2.
"""
import math

import numpy as np

from flux_reference import advect
from oblique_reference import _interp, _upstream, geometry
from plane_reference import MAX_COLDENSH, _photoion, constants, face_axes

NO_CURVE = ((), (1.0,), 0, 0.0)


def unpack(curve):
    """(depths, factors, layer0, depth0) of a curve given as (depths, factors[, layer0[, depth0]]) or None."""
    if curve is None:
        return NO_CURVE
    depths, factors = [float(d) for d in curve[0]], [float(f) for f in curve[1]]
    assert len(factors) == len(depths) + 1
    return depths, factors, int(curve[2]) if len(curve) > 2 else 0, float(curve[3]) if len(curve) > 3 else 0.0


def layer_depth(depth0, layer0, m, path):
    return float(depth0) + (float(int(layer0) + int(m)) + 0.5) * float(path)


def layer_factor(curve, m, path):
    """f of layer m (travel order) for the per-layer path `path`."""
    depths, factors, layer0, depth0 = unpack(curve)
    d = layer_depth(depth0, layer0, m, path)
    return factors[sum(1 for x in depths if d > x)]


def plane_path(dr, axis, tilt=None):
    """The per-layer path of a pass, as the product's host forms it."""
    if tilt is not None and (float(tilt[0]) != 0.0 or float(tilt[1]) != 0.0):
        return geometry(tilt, dr, axis)[3]
    return float(dr[axis])


def curve_pass(orc, otables, mesh, dr, vol, ndens, xh_av, xhe_av, axis, from_high, normflux=None, flux_map=None, curve=None, tilt=None,
               periodic=(False, False, False), heat=False, coldensh_lls=None, lls_grid=None, entry=None):
    """One plane with a light curve over the whole mesh, from zeroed rate grids.  normflux (a number or three: uniform) or
    flux_map (3 x face); curve: (depths, factors[, layer0[, depth0]]) or None; everything else as flux_reference.flux_pass.
    Returns flux_pass' dictionary (exit_flux and layer_flux unscaled; for a uniform plane they repeat normflux) plus factors
    (mesh[axis]: f of every layer in travel order)."""
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
    multi = bool(fm[1].any() or fm[2].any())
    tilted = tilt is not None and (float(tilt[0]) != 0.0 or float(tilt[1]) != 0.0)
    if tilted:
        a_f, a_g, s, path, e_f, e_g = geometry(tilt, dr, axis)
        assert 0.0 <= a_f <= 1.0 and 0.0 <= a_g <= 1.0, (a_f, a_g)
        wrap_f, wrap_g = bool(periodic[f_ax]), bool(periodic[g_ax])
    else:
        path = float(dr[axis])
    factors = [layer_factor(curve, m, path) for m in range(na)]
    stride = [1, mesh[0], mesh[0] * mesh[1]]
    use_lls = coldensh_lls is not None or lls_grid is not None
    dr0, vol = float(dr[0]), float(vol)
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
        cf = factors[m]
        if tilted and mapped:                          # the carried flux is the unscaled one
            fl = advect(s, fa, fb, e_f, e_g, wrap_f, wrap_g, fl)
        layers.append(np.array(fl))
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
                nfu = [fl[0][fc], fl[1][fc], fl[2][fc]]
                skip = (nfu[0] == 0.0 and nfu[1] == 0.0 and nfu[2] == 0.0) or cf == 0.0
                term = 0.0
                if not skip and cin[0] < MAX_COLDENSH:
                    nf = [nfu[0] * cf, nfu[1] * cf, nfu[2] * cf]
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
                exit_flux=np.array(fl[0] + fl[1] + fl[2]), layer_flux=np.array(layers), factors=np.array(factors))
