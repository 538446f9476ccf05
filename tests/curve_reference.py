"""Reference for source light curves (c2r_set_source_curves), shared by tests/test_source_curves_host.py (CPU) and
tests/test_gpu_source_curves.py (GPU).  Not a test module.

Nothing here computes a rate: it composes what tests/beam_reference.py and tests/horizon_reference.py compose, with the
source's flux scaled shell by shell.
  * A NumPy restatement of the rule of csrc/c2ray_curve.hpp (shell_offsets, factor_offsets) on the offsets of
    beam_reference.offsets: R2[k] = radius[k]*radius[k], d2 as the horizon forms it, b = the number of k with d2 > R2[k].
  * Per source and per shell b with factor[b] != 0 the oracle's do_source alone from zeroed grids (source_scaled), the source's
    flux -- and its PL / QPL fluxes -- replaced by np.float64(flux)*np.float64(factor[b]); the cells of shell b are taken from
    that run; the sources are folded in source order from 0.0.  A general factor scales the grids only to rounding (0.3: up to
    1.6e-13 relative), hence a run of its own per factor; a power of two scales them exactly
    (tests/test_source_curves_host.py keeps that premise).
  * The escape maps and the rim terms the same way: face_loss_reference.source_terms / rim_reference.source_terms on the case
    with the scaled flux, each cell from the run of its own shell's factor.
The composition is exact where product and oracle trace the same rounds: the caller picks such cases and asserts the rounds.

A curve is None (no curve) or (radii, factors) as HipEngine.set_source_curves takes it: up to 8 ascending radii in the length
unit of dr and one factor more.
"""
import copy

import numpy as np

import axis_boundary_cases as ab
import beam_reference as br
import face_loss_reference as fl
import horizon_reference as hr
import mix_reference as mr
import rim_reference as rr

GRIDS = br.GRIDS
MAX_STEPS = 8


def curve_R2(radius):
    """The host's double per step: R2 = radius*radius (+inf where it overflows)."""
    r = np.float64(radius)
    with np.errstate(over="ignore"):
        return r * r


def shell_offsets(curve, dr, di, dj, dk):
    """The shell index b for integer offsets (arrays or scalars), every product and sum rounded as written, from the left."""
    di, dj, dk = (np.asarray(x, dtype=np.int64) for x in (di, dj, dk))
    b = np.zeros(np.broadcast(di, dj, dk).shape, dtype=np.int64)
    if curve is None:
        return b
    xs = np.float64(dr[0]) * di.astype(np.float64)
    ys = np.float64(dr[1]) * dj.astype(np.float64)
    zs = np.float64(dr[2]) * dk.astype(np.float64)
    d2 = (xs * xs + ys * ys) + zs * zs
    for r in curve[0]:
        b = b + (d2 > curve_R2(r))
    return b


def factors_of(curve):
    return np.array([1.0] if curve is None else [float(f) for f in curve[1]], dtype=np.float64)


def factor_offsets(curve, dr, di, dj, dk):
    """f = factor[b] for integer offsets; 1.0 everywhere without a curve."""
    return factors_of(curve)[shell_offsets(curve, dr, di, dj, dk)]


def shell_cells(case, ns, curve):
    """Flat int array over the cells of the product mesh (i fastest): the shell of the cell for source ns (0-based)."""
    di, dj, dk = br.offsets(case.n, case.srcpos[ns], case.periodic)
    return shell_offsets(curve, case.dr, di, dj, dk).reshape(-1)


def factor_cells(case, ns, curve):
    return factors_of(curve)[shell_cells(case, ns, curve)]


def scaled_case(case, ns, f):
    """The case with the fluxes of source ns (1-based) replaced by the rounded products flux*f; everything else shared."""
    out = copy.copy(case)
    out.flux = case.flux.copy()
    out.flux[ns - 1] = np.float64(case.flux[ns - 1]) * np.float64(f)
    if case.pl is not None:
        out.pl, out.qpl = case.pl.copy(), case.qpl.copy()
        out.pl[ns - 1] = np.float64(case.pl[ns - 1]) * np.float64(f)
        out.qpl[ns - 1] = np.float64(case.qpl[ns - 1]) * np.float64(f)
    return out


_scaled = {}


def scaled_key(key, ns, f):
    return f"{key}|{ns}x{float(f).hex()}"


def source_scaled(pkg, orc, otables, case, key, ns, f):
    """Source ns (1-based) alone from zeroed grids with its fluxes times f: (region-sized grids, the oracle's nbox, its loss,
    (step, state)).  Computed once per session per (key, ns, f), never changed by a caller; f == 1.0 is beam_reference's run."""
    if float(f) == 1.0:
        return br.source_alone(pkg, orc, otables, case, key, ns)
    k = (key, ns, float(f))
    if k not in _scaled:
        _scaled[k] = mr.point_sources_on_top(pkg, orc, otables, scaled_case(case, ns, f), None, [ns])
    grids, nbox, loss, pair = _scaled[k]
    return grids, nbox[0], loss[0], pair


def lit_cells(case, ns, curve, horizon=None, beam=None):
    """Flat bool array: lit for every feature set -- the beam, the horizon, and a shell whose factor is not 0 (ns 0-based)."""
    return br.lit_cells(case, ns, beam) & hr.within_cells(case, ns, horizon) & (factor_cells(case, ns, curve) != 0.0)


def compose(pkg, orc, otables, case, key, curves, horizons=None, beams=None, sources=None, inside=None):
    """grid = grid + term_s over `sources` (1-based, default all, in that order) from 0.0; term_s holds, in every lit cell of
    shell b, the grid of the oracle's run of source s with its fluxes times factor[b], and 0.0 elsewhere.
    inside: {ns: flat bool array}, cells the product traces for source ns where that is less than the oracle traces.
    Returns the grids, nbox (the oracle's rounds per source, one entry per run, in shell order) and runs (the factors run)."""
    ncell = ab.cells(case.n)
    nsrc = len(case.flux)
    sources = list(range(1, nsrc + 1)) if sources is None else list(sources)
    horizons = [None] * nsrc if horizons is None else list(horizons)
    beams = [None] * nsrc if beams is None else list(beams)
    out = dict(phih_grid=np.zeros(ncell), phihe_grid=np.zeros(2 * ncell), phiheat=np.zeros(ncell))
    nbox, runs = [], []
    for ns in sources:
        curve = curves[ns - 1]
        lit = br.lit_cells(case, ns - 1, beams[ns - 1]) & hr.within_cells(case, ns - 1, horizons[ns - 1])
        if inside is not None and ns in inside:
            lit = lit & inside[ns]
        shell, fac = shell_cells(case, ns - 1, curve), factors_of(curve)
        term = {k: np.zeros(out[k].size) for k in GRIDS}
        rounds, ran = [], []
        for b in range(len(fac)):
            here = lit & (shell == b)
            if fac[b] == 0.0 or not here.any():
                continue
            grids, nb, _, _ = source_scaled(pkg, orc, otables, case, key, ns, fac[b])
            rounds.append(nb)
            ran.append(float(fac[b]))
            for k in GRIDS:
                m = np.tile(here, out[k].size // ncell)
                term[k][m] = grids[k][m]
        for k in GRIDS:
            out[k] = out[k] + term[k]
        nbox.append(rounds)
        runs.append(ran)
    out["nbox"], out["runs"] = nbox, runs
    return out


_terms = {}


def face_terms(pkg, orc, otables, case, key, ns, f):
    """face_loss_reference.source_terms of source ns (0-based) with its fluxes times f, once per session."""
    k = (key, ns, float(f))
    if k not in _terms:
        _terms[k] = fl.source_terms(pkg, orc, otables, scaled_case(case, ns + 1, f), ns)
    return _terms[k]


def compose_maps(pkg, orc, otables, case, key, curves, horizons=None, beams=None, sources=None):
    """The escape maps: per source the terms of face_loss_reference.source_terms, each cell from the run of its shell's factor,
    0.0 where unlit, map = map + terms in source order.  Returns ({face: [b, a]}, the per-source maps)."""
    n, _, periodic = fl.geometry(case)
    nsrc = len(case.flux)
    sources = list(range(1, nsrc + 1)) if sources is None else list(sources)
    horizons = [None] * nsrc if horizons is None else list(horizons)
    beams = [None] * nsrc if beams is None else list(beams)
    total = {f: np.zeros(fl.face_shape(n, f)) for f in fl.open_faces(periodic)}
    per_source = []
    for ns in sources:
        curve = curves[ns - 1]
        fac = factors_of(curve)
        by_cell = {}
        for b in range(len(fac)):
            if fac[b] == 0.0:
                continue
            for m1, o, term in face_terms(pkg, orc, otables, case, key, ns - 1, fac[b]):
                if int(shell_offsets(curve, case.dr, o[0], o[1], o[2])) == b:
                    by_cell[m1] = (o, term)
        terms = []
        for m1, o, _ in face_terms(pkg, orc, otables, case, key, ns - 1, 1.0):       # every traced face cell, lit or not
            lit = bool(hr.lit_offsets(beams[ns - 1], horizons[ns - 1], case.dr, o[0], o[1], o[2])) and m1 in by_cell
            terms.append((m1, o, by_cell[m1][1] if lit else 0.0))
        one = fl.maps_of_terms(case, terms)
        one = {f: one[f].reshape(fl.face_shape(n, f)) for f in one}
        per_source.append(one)
        for f in total:
            total[f] = total[f] + one[f]
    return total, per_source


def rim_terms(pkg, orc, otables, case, key, ns, curve, radius, lo, hi, beam=None):
    """The T expected rim terms of source ns (0-based): rim_reference.source_terms on the case with the fluxes times the factor
    of each face cell's own shell; a face cell in a shell of factor 0 has no face (+0.0).  Returns (terms, face flags)."""
    rule = rr.columns(radius, case.dr, lo, hi, beam)
    fac = factors_of(curve)
    cell = rule["cell"]
    shell = shell_offsets(curve, case.dr, cell[:, 0], cell[:, 1], cell[:, 2])
    terms = np.zeros(len(rule["w"]))
    face = rule["face"] & (fac[shell] != 0.0)
    for b in sorted(set(int(x) for x in shell[face])):
        one, _ = rr.source_terms(pkg, orc, otables, scaled_case(case, ns + 1, fac[b]), scaled_key(key, ns, fac[b]), ns, radius, lo, hi, beam)
        pick = face & (shell == b)
        terms[pick] = one[pick]
    return terms, face
