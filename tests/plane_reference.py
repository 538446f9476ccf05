"""Reference for the plane-parallel sources (c2r_set_plane_sources), shared by tests/test_plane_reference_host.py (CPU) and
tests/test_gpu_plane_sources.py (GPU).  Not a test module.

The oracle has no such source, but a plane along an open axis is a 1-D march per line of cells in which everything per cell
is a routine the oracle does have: steps 1-7 of include/c2ray_hip.h in plain Python floats (IEEE doubles, every product
from the left, as written there), with oracle.photoion_rates (one SED) or orc_photoion_rates3 (three) per cell.  abu_he and
epsilon are the oracle's own (oracle.constants(), which tests/golden/consts.npz pins); max_coldensh is the REAL(4) literal
2e29 of evolve_point.F90:91.  The loss is summed with math.fsum.
"""
import ctypes as C
import math

import numpy as np

MAX_COLDENSH = float(np.float32(2e29))
RATES = ("phih_grid", "phihe_grid")


def constants(orc):
    """(abu_he, epsilon) as the oracle was compiled with them."""
    c = orc.constants()
    return float(c[1]), float(c[30])


def face_axes(axis):
    """The two remaining axes, the lower one first (it runs fastest over the face)."""
    return [d for d in range(3) if d != axis]


def face_cells(mesh, axis):
    a, b = face_axes(axis)
    return int(mesh[a]) * int(mesh[b])


def column_cells(mesh, axis, from_high):
    """cells[f, m]: 0-based mesh cell number (i fastest) of step m, in travel order, of face column f."""
    n = [int(x) for x in mesh]
    stride = [1, n[0], n[0] * n[1]]
    a, b = face_axes(axis)
    fa = np.arange(n[a])[None, :] * stride[a] + np.arange(n[b])[:, None] * stride[b]      # [b, a]: a fastest
    along = np.arange(n[axis])[::-1] if from_high else np.arange(n[axis])
    return fa.reshape(-1)[:, None] + along[None, :] * stride[axis]


def _photoion(orc, otables, cols6, vol_ph, nf, multi, i_state, heat):
    """photo_HI, photo_HeI, photo_HeII, heat, photo_out of one cell from the oracle."""
    if multi:
        out = orc.PhotRates()
        orc.lib().orc_photoion_rates3(C.byref(otables.c), *[C.c_double(x) for x in cols6], C.c_double(vol_ph), (C.c_double * 3)(*nf),
                                      C.c_double(i_state), C.c_int(0 if heat else 1), C.byref(out))
        r = out.as_array()
    else:
        r = orc.photoion_rates(otables, cols6, vol_ph, nf[0], i_state, not heat)
    return r[0], r[1], r[2], r[18], r[20]


def plane_pass(orc, otables, mesh, dr, vol, ndens, xh_av, xhe_av, axis, from_high, normflux, heat=False, coldensh_lls=None,
               lls_grid=None, entry=None):
    """One plane over the whole mesh, from zeroed rate grids.  ndens: ncell, xh_av: 2 ncell, xhe_av: 3 ncell (mesh order, i
    fastest, components slowest); normflux: a number (black body) or three; coldensh_lls / lls_grid: LLS in force with the
    scalar / the REAL(4) grid; entry: 3 x face entry columns or None.
    Returns phih_grid, phihe_grid (2 ncell), phiheat, exit (3 x face), terms (face: each column's loss term),
    loss (their math.fsum) and cin_HI (ncell, the fogged incoming HI column of every cell)."""
    abu_he, eps = constants(orc)
    n = int(np.prod(mesh))
    nf = [float(x) for x in np.atleast_1d(np.asarray(normflux, dtype=np.float64))]
    nf = (nf + [0.0, 0.0])[:3]
    multi = nf[1] != 0.0 or nf[2] != 0.0
    use_lls = coldensh_lls is not None or lls_grid is not None
    cells = column_cells(mesh, axis, from_high)
    face = cells.shape[0]
    path = float(dr[axis])
    dr0, vol = float(dr[0]), float(vol)
    nd, xh, xhe = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (ndens, xh_av, xhe_av))
    phih, phihe, phiheat = np.zeros(n), np.zeros(2 * n), np.zeros(n)
    exit3, terms, cin_grid = np.zeros(3 * face), np.zeros(face), np.zeros(n)
    for f in range(face):
        cin = [0.0, 0.0, 0.0] if entry is None else [float(entry[f]), float(entry[face + f]), float(entry[2 * face + f])]
        term = 0.0
        for q in cells[f]:
            q = int(q)
            ndq = float(nd[q])
            u_HI = max(float(xh[q]), eps) * ndq                                   # step 1
            u_HeI = max(float(xhe[q]), eps) * ndq
            u_HeII = max(float(xhe[q + n]), eps) * ndq
            if use_lls:                                                           # step 4
                lls = float(lls_grid[q]) if lls_grid is not None else float(coldensh_lls)
                cin[0] = cin[0] + lls * path / dr0
            cout = [cin[0] + u_HI * path * (1.0 - abu_he),                        # step 5
                    cin[1] + u_HeI * path * abu_he,
                    cin[2] + u_HeII * path * abu_he]
            cin_grid[q] = cin[0]
            term = 0.0
            if cin[0] < MAX_COLDENSH:                                             # step 6
                cols6 = [cin[0], cout[0], cin[1], cout[1], cin[2], cout[2]]
                p_HI, p_HeI, p_HeII, h, p_out = _photoion(orc, otables, cols6, path, nf, multi, max(float(xh[q + n]), eps), heat)
                phih[q] = phih[q] + p_HI / (u_HI * (1.0 - abu_he))
                phihe[q] = phihe[q] + p_HeI / (u_HeI * abu_he)
                phihe[q + n] = phihe[q + n] + p_HeII / (u_HeII * abu_he)
                if heat:
                    phiheat[q] = phiheat[q] + h
                term = p_out * vol / path                                         # step 7, kept for the last cell only
            cin = cout
        exit3[f], exit3[face + f], exit3[2 * face + f] = cin
        terms[f] = term
    return dict(phih_grid=phih, phihe_grid=phihe, phiheat=phiheat, exit=exit3, terms=terms, loss=math.fsum(terms), cin_HI=cin_grid)
