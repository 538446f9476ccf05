"""Seeded random cases for everything built on top of the reference's feature set -- open and per-axis boundaries, escape
maps, plane sources (normal, tilted, flux-mapped), beams, photon horizons, the horizon loss, source light curves and plane light
curves -- and the one composer that folds them in the documented order.  Shared by tests/test_extension_fuzz_host.py (CPU)
and tests/test_gpu_extension_fuzz.py (GPU).  Not a test module.

draw(rng) returns a plain dict, the spec, which is also the tag a failure prints; it knows nothing of the package (lengths
are in units of dr(1), a lattice radius is an offset and a nudge).  build(pkg, spec) makes the AxisCase and the settings.
The list is FIXED followed by draw(default_rng(SEED + i)) for i < NCASES; C2R_EXTFUZZ_CASES / C2R_EXTFUZZ_SEED widen or move it.
Behind it, and never moving it, comes the curved list: FIXED_CURVED followed by draw_curved(default_rng([SEED, 1, i])) for
i < NCURVED (C2R_EXTFUZZ_CURVED_CASES).  draw_curved is draw plus, from the same generator, a light curve per point source
("curves"), a light curve per plane ("curve" in the plane's dict) and the order in which the GPU test calls the setters
("set_order").  A spec without these keys means no curve anywhere.  Radii are horizons' radius dicts, depths are in units of the
plane's per-layer path (plane_curve_reference.plane_path) or name a layer centre and a nudge in ulps.

Tier A, one geometric round: every reach lies within subboxsize on every axis, so mix_reference.same_cells holds for any gas
and any feature, and every source's final box is its reach.
Tier B, several rounds, ionised gas on the meshes of axis_boundary_cases' cases A to D or a periodic 24^3: the rounds of a
beamed or horizoned source follow from the predicates alone (expected_trace) -- every lit surface cell of such gas passes far
more than 1e-10 of the flux, so the loop goes on exactly while some lit cell lies on a face that decides.

compose_all adds no physics: planes from their references folded in plane order from 0.0 (mix_reference.fold_planes), then
grid = grid + where(lit_s & within_s & inside_s, term_s, 0.0) per point source in source order, term_s the oracle's do_source of
that source alone (beam_reference.source_alone); the escape maps the same way from the planes' terms and
face_loss_reference's per-source terms; the horizon loss from rim_reference.source_terms and face_sum; the global pass from
the oracle's own on the product mesh, seeded with the composed grids (chemistry is cell-local).
With curves the composer composes what tests/curve_reference.py and tests/plane_curve_reference.py compose: term_s holds, in
each cell of shell b, the oracle's run of source s alone with its fluxes times factor[b] (curve_reference.source_scaled; for a
power of two the factor-1 term times the factor, which is exact), the mask gains factor != 0, expected_trace takes the same lit
predicate, escape maps and rim terms come per face cell from the run of that cell's shell, and a curved plane goes through
plane_curve_reference.curve_pass.
"""
import math
import os

import numpy as np

import axis_boundary_cases as ab
import beam_reference as br
import curve_reference as cr
import face_loss_reference as fl
import horizon_reference as hr
import mix_reference as mr
import oblique_reference as obr
import plane_curve_reference as pcr
import rim_reference as rr

DEFAULT_CASES, DEFAULT_SEED = 24, 20261031
NCASES = int(os.environ.get("C2R_EXTFUZZ_CASES", str(DEFAULT_CASES)))
SEED = int(os.environ.get("C2R_EXTFUZZ_SEED", str(DEFAULT_SEED)))
DEFAULT_CURVED = 10
NCURVED = int(os.environ.get("C2R_EXTFUZZ_CURVED_CASES", str(DEFAULT_CURVED)))

MASKS = ("", "x", "y", "z", "xy", "xz", "yz", "xyz")
OPEN_SIZES = (2, 3, 4, 5, 7, 8, 11)
PERIODIC_SIZES = (4, 5, 8, 9, 12, 16, 21)
OPEN_EXTENT = 24
# Tier B: name -> (mesh, open axes, embedding, another embedding)
TIER_B = {"A": ((24, 24, 24), "z", (24, 24, 48), (24, 24, 50)), "B": ((11, 24, 24), "x", (24, 24, 24), (26, 24, 24)),
          "C": ((11, 11, 24), "xy", (24, 24, 24), (26, 31, 24)), "D": ((11, 24, 24), "xz", (24, 24, 48), (31, 24, 50)),
          "P": ((24, 24, 24), "", (24, 24, 24), None)}
COS_HALF = {"0": 0.0, "1": 1.0, "sqrt_half": math.sqrt(0.5), "cos5": math.cos(math.radians(5.0)),
            "cos35": math.cos(math.radians(35.0)), "cos80": math.cos(math.radians(80.0))}
COS_CLASSES = tuple(COS_HALF) + ("uniform",)
AXIS_CLASSES = ("unit", "110", "111", "random")
RADIUS_CLASSES = ("none", "inf", "zero", "sub_cell", "huge", "uniform", "lattice_below", "lattice", "lattice_above")
ROUTES = ("plain", "slabs", "iteration", "do_source")
PLANE_KINDS = ("normal", "tilted", "mapped")
CURVE_CLASSES = ("none", "zero_one", "ones", "horizon", "gap", "eight", "general")
CURVE_RADIUS_CLASSES = ("uniform", "lattice_below", "lattice", "lattice_above", "sub_cell", "zero", "huge")
PLANE_CURVE_CLASSES = ("none", "uniform", "centre", "gap", "horizon")
FACTORS_A = (0.0, 0.25, 0.5, 1.0, 2.0, 3.0 / 7.0, 1.9)       # tests/test_gpu_source_curves.py's pool
FACTORS_B = (0.0, 0.25, 0.5, 1.0, 2.0, 4.0)                  # 0 and powers of two: they scale the oracle's term exactly
SETTERS = ("horizons", "beams", "curves", "plane_curves")
YEAR = 3.15576e7
GRIDS = br.GRIDS


# -- the generator ----------------------------------------------------------------------------------------------------------
def embedding_ok(n, m, periodic):
    """AxisCase.check_embedding as a predicate."""
    if not all(md == nd if per else md >= 2 * nd for nd, md, per in zip(n, m, periodic)):
        return False
    if (m[2] // 2 - 1) % ab.SUBBOXSIZE == 0:
        return False
    if periodic[2]:
        rounds = -(-(m[2] // 2) // ab.SUBBOXSIZE)
        return all(per or nd - 1 <= ab.SUBBOXSIZE * rounds for nd, per in zip(n, periodic))
    return True


def reach_of(n, periodic, pos):
    lr = [ab.axis_reach(int(nd), int(p), bool(per)) for nd, p, per in zip(n, pos, periodic)]
    return [a for a, _ in lr], [b for _, b in lr]


def _draw_mesh(rng, tier):
    if tier == "B":
        name = str(rng.choice(sorted(TIER_B)))
        n, mask, m, _ = TIER_B[name]
        return mask, n, m
    mask = MASKS[int(rng.integers(0, len(MASKS)))]
    low = int(rng.integers(0, 3))                           # this axis draws from the lower half of its list
    n = []
    for d, ax in enumerate("xyz"):
        sizes = OPEN_SIZES if ax in mask else PERIODIC_SIZES
        n.append(int(rng.choice(sizes[:3] if d == low else sizes)))
    m = tuple(OPEN_EXTENT if ax in mask else nd for ax, nd in zip("xyz", n))
    return mask, tuple(n), m


def _draw_beam(rng):
    kind = int(rng.integers(0, 3))
    cls = AXIS_CLASSES[int(rng.integers(0, len(AXIS_CLASSES)))]
    if cls == "unit":
        axis = [0.0, 0.0, 0.0]
        axis[int(rng.integers(0, 3))] = float(rng.choice([-1.0, 1.0]))
    elif cls == "110":
        axis = [1.0, 1.0, 0.0]
    elif cls == "111":
        axis = [1.0, 1.0, 1.0]
    else:
        v = rng.normal(0.0, 1.0, 3) * 10.0 ** rng.uniform(-3.0, 3.0)
        axis = [float(x) for x in v]
    name = COS_CLASSES[int(rng.integers(0, len(COS_CLASSES)))]
    cos_half = COS_HALF[name] if name in COS_HALF else float(rng.uniform(0.0, 1.0))
    return dict(kind=kind, axis=axis, axis_class=cls, cos_half=cos_half, cos_class=name)


def _draw_horizon(rng, lo, hi):
    """A radius class and what build() needs to form the radius: a factor of dr(1), or a lattice offset inside lo..hi."""
    name = str(rng.choice(["none", "inf", "zero", "sub_cell", "huge", "uniform", "lattice"]))
    out = dict(radius_class=name)
    if name == "uniform":
        out["cells"] = float(rng.uniform(0.5, 12.0))
    if name == "lattice":
        o = [0, 0, 0]
        while o == [0, 0, 0] and any(lo[d] != hi[d] for d in range(3)):
            o = [int(rng.integers(lo[d], hi[d] + 1)) for d in range(3)]
        nudge = int(rng.integers(-1, 2))
        out.update(offset=o, nudge=nudge, radius_class=("lattice_below", "lattice", "lattice_above")[nudge + 1])
    return out


def _tilt_fits(tilt, axis, cubic):
    k = (1.0, 1.0, 1.0) if cubic else mr.DR_FACTORS
    a_f, a_g = obr.geometry(tilt, k, axis)[:2]
    return a_f <= 1.0 and a_g <= 1.0 and (tilt[0] != 0.0 or tilt[1] != 0.0)


def _draw_plane(rng, mask, cubic, multi, rejected):
    axis = "xyz".index(str(rng.choice(list(mask))))
    kind = PLANE_KINDS[int(rng.integers(0, len(PLANE_KINDS)))]
    flux = [float(10.0 ** rng.uniform(-0.5, 0.5)), 0.0, 0.0]             # in units of mix_reference.FLUX
    if multi:
        flux[1:] = [float(rng.uniform(0.1, 1.0)) * float(rng.random() < 0.6) for _ in range(2)]
    out = dict(axis=axis, from_high=int(rng.integers(0, 2)), kind=kind, flux=flux)
    if kind == "tilted" or (kind == "mapped" and rng.random() < 0.3):
        while True:
            tilt = (float(rng.uniform(-0.8, 0.8)), float(rng.uniform(-0.8, 0.8)))
            if _tilt_fits(tilt, axis, cubic):
                break
            rejected.append("tilt beyond one cell per layer")
        out["tilt"] = tilt
    if kind == "mapped":
        out.update(map_seed=int(rng.integers(1 << 30)), map_scale=float(rng.uniform(0.5, 1.5)))
    if rng.random() < 0.3:
        out["entry_seed"] = int(rng.integers(1 << 30))
    return out


def draw(rng):
    """One well-posed case as a plain dict.  spec["rejected"] lists every draw that was thrown away on the way, with its
    reason: nothing is redrawn silently."""
    rejected = []
    while True:
        tier = "B" if rng.random() < 0.25 else "A"
        mask, n, m = _draw_mesh(rng, tier)
        periodic = tuple(ax not in mask for ax in "xyz")
        if embedding_ok(n, m, periodic):
            break
        rejected.append(f"embedding {n} in {m}")
    gas = "ionised" if tier == "B" else str(rng.choice(["mixed", "opaque"]))
    cubic, heat, multi = bool(rng.random() < 0.5), bool(rng.random() < 0.5), bool(rng.random() < 0.25)
    nsrc = int(rng.integers(1, 5))
    if tier == "B":
        nsrc = min(nsrc, 2)                                 # the oracle's runs on a 24 x 24 x 48 embedding are what a case costs
    srcpos = [[int(rng.integers(1, nd + 1)) for nd in n] for _ in range(nsrc)]
    if rng.random() < 0.3:                                  # a corner, or a cell on an open face
        if mask and rng.random() < 0.5:
            d = "xyz".index(str(rng.choice(list(mask))))
            srcpos[0][d] = (1, n[d])[int(rng.integers(0, 2))]
        else:
            srcpos[0] = [(1, nd)[int(rng.integers(0, 2))] for nd in n]
    if nsrc > 1 and rng.random() < 0.3:
        srcpos[1] = list(srcpos[0])                         # two sources in one cell
    flux = [float(x) for x in 10.0 ** rng.uniform(4.0, 7.5, nsrc)]
    pl = qpl = None
    if multi:
        pl = [float(x) for x in np.where(rng.random(nsrc) < 0.6, 10.0 ** rng.uniform(4.0, 7.0, nsrc), 0.0)]
        qpl = [float(x) for x in np.where(rng.random(nsrc) < 0.6, 10.0 ** rng.uniform(4.0, 7.0, nsrc), 0.0)]
        keep = rng.random(nsrc) < 0.8
        flux = [f if k or (a == 0.0 and b == 0.0) else 0.0 for f, k, a, b in zip(flux, keep, pl, qpl)]      # never all three zero
    beams, horizons = [], []
    for ns in range(nsrc):
        beams.append(_draw_beam(rng))
        horizons.append(_draw_horizon(rng, *reach_of(n, periodic, srcpos[ns])))
    finite = any(h["radius_class"] not in ("none", "inf") for h in horizons)
    planes = []
    if tier == "A" and mask:
        planes = [_draw_plane(rng, mask, cubic, multi, rejected) for _ in range(int(rng.integers(0, 3)))]
    route = ROUTES[int(rng.integers(0, len(ROUTES)))]
    return dict(tier=tier, mask=mask, n=list(n), m=list(m), gas=gas, gas_seed=int(rng.integers(1 << 30)), cubic=cubic, heat=heat, multi=multi,
                srcpos=srcpos, flux=flux, pl=pl, qpl=qpl, beams=beams, horizons=horizons,
                horizon_loss=bool(finite and rng.random() < 2.0 / 3.0), maps=bool(mask), planes=planes,
                batch=int(rng.integers(1, 9)), route=route, nslab=int(rng.integers(1, 5)),
                dt_years=float(10.0 ** rng.uniform(5.0, 7.3)), rejected=rejected)


# -- the curved list: draw() and, from the same generator, the light curves --------------------------------------------------------
def _rel_dr(cubic):
    return (1.0, 1.0, 1.0) if cubic else mr.DR_FACTORS


def _draw_radii(rng, nstep, lo, hi, cubic, rejected):
    """nstep radius dicts (as _draw_horizon makes them, minus "none" and "inf"), ascending and distinct for the case's cells."""
    got = []
    while len(got) < nstep:
        name = str(rng.choice(["uniform", "uniform", "uniform", "lattice", "lattice", "sub_cell", "zero", "huge"]))
        h = dict(radius_class=name)
        if name == "uniform":
            h["cells"] = float(rng.uniform(0.4, 12.0))
        if name == "lattice":
            o = [0, 0, 0]
            while o == [0, 0, 0] and any(lo[d] != hi[d] for d in range(3)):
                o = [int(rng.integers(lo[d], hi[d] + 1)) for d in range(3)]
            nudge = int(rng.integers(-1, 2))
            h.update(offset=o, nudge=nudge, radius_class=("lattice_below", "lattice", "lattice_above")[nudge + 1])
        r = radius_of(h, _rel_dr(cubic))
        if any(abs(r - x) <= 1e-9 * max(r, x) for x, _ in got):
            rejected.append(f"curve radius {name} twice")
            continue
        got.append((r, h))
    got.sort(key=lambda t: t[0])
    return [h for _, h in got]


def _draw_factors(rng, pool, n, lit=False):
    pool = [f for f in pool if f != 0.0] if lit else list(pool)
    return [float(pool[int(k)]) for k in rng.integers(0, len(pool), size=n)]


def _draw_curve(rng, pool, lo, hi, cubic, rejected):
    """None, or dict(cls, radii, factors): a source curve of one of CURVE_CLASSES."""
    cls = CURVE_CLASSES[int(rng.integers(0, len(CURVE_CLASSES)))]
    if cls == "none":
        return None
    if cls == "ones":
        nstep = int(rng.integers(1, 4))
        factors = [1.0] * (nstep + 1)
    elif cls == "horizon":
        nstep, factors = 1, [1.0, 0.0]
    elif cls == "gap":
        nstep = 2
        a, b = _draw_factors(rng, pool, 2, lit=True)
        factors = [a, 0.0, b]
    elif cls == "eight":
        nstep = 8
        factors = _draw_factors(rng, pool, 9)
    elif cls == "zero_one":
        nstep = int(rng.integers(1, 5))
        factors = _draw_factors(rng, (0.0, 1.0), nstep + 1)
    else:
        nstep = int(rng.integers(0, 5))
        factors = _draw_factors(rng, pool, nstep + 1, lit=nstep == 0)
    return dict(cls=cls, radii=_draw_radii(rng, nstep, lo, hi, cubic, rejected), factors=factors)


def _depth_key(d, layer0, depth0):
    """Where a depth dict lies, in paths, for sorting only."""
    if d["kind"] == "uniform":
        return d["paths"]
    return depth0 + layer0 + d["m"] + 0.5 + 1e-12 * d["nudge"]


def _draw_plane_curve(rng, na, rejected):
    """None, or dict(cls, depths, factors, layer0, depth0) for a plane that crosses na layers: depths in units of the per-layer
    path, dict(kind="uniform", paths) or dict(kind="centre", m, nudge) -- the centre of layer m, nudged by that many ulps."""
    cls = PLANE_CURVE_CLASSES[int(rng.integers(0, len(PLANE_CURVE_CLASSES)))]
    if cls == "none":
        return None
    layer0, depth0 = (int(rng.integers(1, 4)), float(rng.uniform(0.1, 2.0))) if rng.random() < 0.4 else (0, 0.0)
    base = depth0 + layer0
    if cls == "horizon":                                    # beyond the depth nothing: the last layer's centre lies beyond it
        depths = [dict(kind="uniform", paths=base + float(rng.uniform(0.2, na - 0.6)))]
        factors = _draw_factors(rng, FACTORS_A, 1, lit=True) + [0.0]
    elif cls == "gap":
        lo, hi = sorted(float(x) for x in rng.uniform(0.2, na - 0.3, 2))
        depths = [dict(kind="uniform", paths=base + lo), dict(kind="uniform", paths=base + hi)]
        a, b = _draw_factors(rng, FACTORS_A, 2, lit=True)
        factors = [a, 0.0, b]
    else:
        nstep = int(rng.integers(0, 9)) if cls == "uniform" else int(rng.integers(1, min(8, 2 * na) + 1))
        depths = []
        while len(depths) < nstep:
            if cls == "centre" and (not depths or rng.random() < 0.5):
                d = dict(kind="centre", m=int(rng.integers(0, na)), nudge=int(rng.integers(-1, 2)))
            else:
                d = dict(kind="uniform", paths=base + float(rng.uniform(0.0, na + 0.5)))
            k = _depth_key(d, layer0, depth0)
            if any(abs(k - _depth_key(x, layer0, depth0)) < 1e-13 for x in depths):
                rejected.append("plane curve depth twice")
                continue
            depths.append(d)
        factors = _draw_factors(rng, FACTORS_A, nstep + 1, lit=nstep == 0)
    depths.sort(key=lambda d: _depth_key(d, layer0, depth0))
    return dict(cls=cls, depths=depths, factors=factors, layer0=layer0, depth0=depth0)


def draw_curved(rng):
    """draw(rng), then from the same generator a curve per point source, a curve per plane and the order of the setters."""
    spec = draw(rng)
    n, periodic = spec["n"], tuple(ax not in spec["mask"] for ax in "xyz")
    pool = FACTORS_B if spec["tier"] == "B" else FACTORS_A
    spec["curves"] = [_draw_curve(rng, pool, *reach_of(n, periodic, pos), spec["cubic"], spec["rejected"]) for pos in spec["srcpos"]]
    spec["planes"] = [dict(p, curve=_draw_plane_curve(rng, n[p["axis"]], spec["rejected"])) for p in spec["planes"]]
    spec["set_order"] = [SETTERS[int(k)] for k in rng.permutation(len(SETTERS))]
    return spec


def _beam(kind, axis, cos_class, cos_half=None):
    return dict(kind=kind, axis=[float(x) for x in axis], axis_class="fixed", cos_class=cos_class,
                cos_half=COS_HALF[cos_class] if cos_half is None else cos_half)


# In front of the random cases: the corners of the space that a draw meets rarely, spelled out.
FIXED = [
    # every axis open and two or three cells long, two sources in one cell with different beams, a plane of each kind;
    # rim sheets far below one block (T = 2 * (6 + 6 + 4) = 32)
    dict(tier="A", mask="xyz", n=[2, 3, 2], m=[24, 24, 24], gas="mixed", gas_seed=11, cubic=False, heat=True, multi=False,
         srcpos=[[1, 2, 1], [1, 2, 1], [2, 3, 2]], flux=[3.0e7, 1.0e7, 5.0e6], pl=None, qpl=None,
         beams=[_beam(1, (0, 0, 1), "sqrt_half"), _beam(2, (1, 1, 0), "0"), _beam(0, (0, 0, 0), "0")],
         horizons=[dict(radius_class="lattice", offset=[1, 0, 1], nudge=0), dict(radius_class="sub_cell"), dict(radius_class="none")],
         horizon_loss=True, maps=True,
         planes=[dict(axis=1, from_high=0, kind="normal", flux=[1.0, 0.0, 0.0]),
                 dict(axis=0, from_high=1, kind="tilted", flux=[0.7, 0.0, 0.0], tilt=(0.35, -0.5)),
                 dict(axis=2, from_high=1, kind="mapped", flux=[1.2, 0.0, 0.0], map_seed=5, map_scale=1.0, entry_seed=6)],
         batch=2, route="plain", nslab=1, dt_years=1.0e6, rejected=[]),
    # x open with the source on the face x = 1 (its box is cut on one side only), y and z periodic; a cone of exactly
    # cos_half = 1 and a horizon one ulp below a lattice distance
    dict(tier="A", mask="x", n=[11, 5, 9], m=[24, 5, 9], gas="mixed", gas_seed=12, cubic=True, heat=False, multi=True,
         srcpos=[[1, 3, 4], [7, 1, 9]], flux=[2.0e7, 0.0], pl=[0.0, 3.0e6], qpl=[1.0e6, 0.0],
         beams=[_beam(1, (1, 0, 0), "1"), _beam(2, (1, 1, 1), "cos35")],
         horizons=[dict(radius_class="uniform", cells=6.5), dict(radius_class="lattice_below", offset=[3, -2, 4], nudge=-1)],
         horizon_loss=True, maps=True, planes=[dict(axis=0, from_high=0, kind="normal", flux=[1.0, 0.5, 0.0])],
         batch=1, route="do_source", nslab=1, dt_years=3.0e5, rejected=[]),
    # several rounds, two sources in one cell: a horizon inside the first box ends the loop after one round, a wide cone with
    # a horizon whose square overflows runs to the reach
    dict(tier="B", mask="xz", n=[11, 24, 24], m=[24, 24, 48], gas="ionised", gas_seed=13, cubic=False, heat=False, multi=False,
         srcpos=[[6, 13, 12], [6, 13, 12]], flux=[2.0e7, 1.0e7], pl=None, qpl=None,
         beams=[_beam(0, (0, 0, 0), "0"), _beam(1, (1, 1, -1), "cos80")],
         horizons=[dict(radius_class="uniform", cells=6.0), dict(radius_class="huge")],
         horizon_loss=True, maps=True, planes=[], batch=3, route="slabs", nslab=3, dt_years=2.0e6, rejected=[]),
    # every axis open, no beam and no finite horizon: the one kind of case in which photon_loss(1) has a reference
    # (mix_reference.has_loss_reference), with a plane that is tilted and mapped
    dict(tier="A", mask="xyz", n=[5, 2, 3], m=[24, 24, 24], gas="mixed", gas_seed=14, cubic=False, heat=True, multi=False,
         srcpos=[[5, 1, 3], [2, 2, 1]], flux=[1.5e7, 4.0e6], pl=None, qpl=None,
         beams=[_beam(0, (0, 0, 0), "0"), _beam(0, (0, 0, 0), "0")],
         horizons=[dict(radius_class="inf"), dict(radius_class="none")], horizon_loss=False, maps=True,
         planes=[dict(axis=0, from_high=0, kind="mapped", flux=[1.0, 0.0, 0.0], tilt=(-0.4, 0.3), map_seed=8, map_scale=0.8)],
         batch=8, route="iteration", nslab=2, dt_years=5.0e5, rejected=[]),
]


def _u(cells):
    return dict(radius_class="uniform", cells=cells)


def _d(paths):
    return dict(kind="uniform", paths=paths)


_NO_BEAM, _NO_HORIZON = _beam(0, (0, 0, 0), "0"), dict(radius_class="none")

# In front of the random curved cases: what a draw meets rarely, on the smallest meshes that still hold it.
FIXED_CURVED = [
    # k_rates_curve<isothermal, three SEDs, periodic>: a curved and an uncurved source in one batch, factors 3/7 and 1.9
    dict(tier="A", mask="", n=[5, 4, 8], m=[5, 4, 8], gas="mixed", gas_seed=21, cubic=False, heat=False, multi=True,
         srcpos=[[2, 3, 4], [5, 1, 7]], flux=[2.0e7, 6.0e6], pl=[3.0e6, 0.0], qpl=[1.0e6, 2.0e6],
         beams=[_NO_BEAM, _NO_BEAM], horizons=[_NO_HORIZON, _NO_HORIZON], horizon_loss=False, maps=False, planes=[],
         batch=4, route="slabs", nslab=2, dt_years=1.0e6, rejected=[],
         curves=[dict(cls="general", radii=[_u(1.3), _u(2.6)], factors=[3.0 / 7.0, 1.0, 1.9]), None],
         set_order=["curves", "beams", "plane_curves", "horizons"]),
    # k_rates_curve<isothermal, three SEDs, open>: every axis open and two or three cells long; a plane without a curve
    dict(tier="A", mask="xyz", n=[2, 3, 2], m=[24, 24, 24], gas="mixed", gas_seed=22, cubic=False, heat=False, multi=True,
         srcpos=[[1, 2, 1], [2, 3, 2]], flux=[1.0e7, 2.5e7], pl=[2.0e6, 4.0e6], qpl=[0.0, 1.5e6],
         beams=[_NO_BEAM, _NO_BEAM], horizons=[_NO_HORIZON, _NO_HORIZON], horizon_loss=False, maps=True,
         planes=[dict(axis=0, from_high=0, kind="normal", flux=[1.0, 0.5, 0.0], curve=None)],
         batch=2, route="do_source", nslab=1, dt_years=5.0e5, rejected=[],
         curves=[None, dict(cls="general", radii=[_u(0.9)], factors=[1.9, 0.5])],
         set_order=["beams", "curves", "horizons", "plane_curves"]),
    # k_rates_curve<heating, one SED, open>: z open, a lattice radius between two others
    dict(tier="A", mask="z", n=[4, 5, 3], m=[4, 5, 24], gas="mixed", gas_seed=23, cubic=True, heat=True, multi=False,
         srcpos=[[2, 2, 1], [4, 5, 3]], flux=[3.0e7, 8.0e6], pl=None, qpl=None,
         beams=[_NO_BEAM, _NO_BEAM], horizons=[_NO_HORIZON, _NO_HORIZON], horizon_loss=False, maps=True, planes=[],
         batch=8, route="iteration", nslab=2, dt_years=2.0e6, rejected=[],
         curves=[dict(cls="general", radii=[_u(1.2), dict(radius_class="lattice", offset=[1, 1, 1], nudge=0)], factors=[0.5, 3.0 / 7.0, 2.0]), None],
         set_order=["plane_curves", "curves", "horizons", "beams"]),
    # k_rates_curve<heating, three SEDs, open>: x open; every source of the batch takes the per-lane flux, one of them uncurved,
    # one with eight steps
    dict(tier="A", mask="x", n=[3, 5, 4], m=[24, 5, 4], gas="mixed", gas_seed=24, cubic=False, heat=True, multi=True,
         srcpos=[[3, 2, 2], [1, 5, 4], [2, 3, 1]], flux=[2.0e7, 0.0, 5.0e6], pl=[0.0, 3.0e6, 1.0e6], qpl=[2.0e6, 1.0e6, 0.0],
         beams=[_NO_BEAM] * 3, horizons=[_NO_HORIZON] * 3, horizon_loss=False, maps=True, planes=[],
         batch=3, route="plain", nslab=1, dt_years=1.0e6, rejected=[],
         curves=[None, dict(cls="general", radii=[_u(1.5)], factors=[1.9, 0.25]),
                 dict(cls="eight", radii=[_u(0.5 + 0.4 * k) for k in range(8)], factors=[1.0, 0.5, 3.0 / 7.0, 2.0, 0.0, 1.9, 0.25, 1.0, 0.5])],
         set_order=["horizons", "curves", "beams", "plane_curves"]),
    # cone + finite horizon + curve on both sources of one cell, the horizon loss on, heating with three SEDs: each curve's last
    # radius cuts through the rim, so rim cells beyond it lie in a shell of factor 0 and have no face
    dict(tier="A", mask="", n=[9, 9, 9], m=[9, 9, 9], gas="mixed", gas_seed=25, cubic=True, heat=True, multi=True,
         srcpos=[[5, 5, 5], [5, 5, 5]], flux=[2.0e7, 1.0e7], pl=[2.0e6, 0.0], qpl=[0.0, 3.0e6],
         beams=[_beam(1, (0, 0, 1), "sqrt_half"), _beam(2, (1, 1, 0), "cos35")], horizons=[_u(3.5), _u(3.0)],
         horizon_loss=True, maps=False, planes=[], batch=2, route="plain", nslab=1, dt_years=1.0e6, rejected=[],
         curves=[dict(cls="general", radii=[_u(1.5), _u(3.2)], factors=[1.0, 3.0 / 7.0, 0.0]),
                 dict(cls="general", radii=[_u(2.7)], factors=[2.0, 0.0])],
         set_order=["curves", "horizons", "plane_curves", "beams"]),
    # several rounds: a wide cone with a horizon whose square overflows runs to the reach in two rounds; the shell of factor 0
    # beyond 6 cells ends the loop after one
    dict(tier="B", mask="", n=[24, 24, 24], m=[24, 24, 24], gas="ionised", gas_seed=26, cubic=True, heat=False, multi=False,
         srcpos=[[12, 12, 12]], flux=[2.0e7], pl=None, qpl=None, beams=[_beam(1, (1, 1, -1), "cos80")], horizons=[dict(radius_class="huge")],
         horizon_loss=False, maps=False, planes=[], batch=1, route="slabs", nslab=3, dt_years=2.0e6, rejected=[],
         curves=[dict(cls="general", radii=[_u(6.0)], factors=[2.0, 0.0])],
         set_order=["beams", "horizons", "curves", "plane_curves"]),
    # a curved plane of each kind (the mapped one tilted) beside two curved point sources, escape maps on; no beam and no finite
    # horizon, every axis open: photon_loss(1) has its reference
    dict(tier="A", mask="xyz", n=[5, 3, 4], m=[24, 24, 24], gas="mixed", gas_seed=27, cubic=False, heat=False, multi=False,
         srcpos=[[2, 2, 2], [5, 1, 4]], flux=[1.5e7, 4.0e6], pl=None, qpl=None,
         beams=[_NO_BEAM, _NO_BEAM], horizons=[_NO_HORIZON, _NO_HORIZON], horizon_loss=False, maps=True,
         planes=[dict(axis=1, from_high=0, kind="normal", flux=[1.0, 0.0, 0.0],
                      curve=dict(cls="centre", depths=[dict(kind="centre", m=0, nudge=-1), dict(kind="centre", m=1, nudge=0), dict(kind="centre", m=2, nudge=1)],
                                 factors=[1.9, 0.5, 0.0, 2.0], layer0=0, depth0=0.0)),
                 dict(axis=0, from_high=1, kind="tilted", flux=[0.7, 0.0, 0.0], tilt=(0.35, -0.5),
                      curve=dict(cls="gap", depths=[_d(3.95), _d(5.35)], factors=[1.0, 0.0, 3.0 / 7.0], layer0=2, depth0=0.75)),
                 dict(axis=2, from_high=1, kind="mapped", flux=[1.2, 0.0, 0.0], tilt=(0.3, -0.4), map_seed=5, map_scale=1.0,
                      curve=dict(cls="horizon", depths=[_d(2.2)], factors=[0.25, 0.0], layer0=0, depth0=0.0))],
         batch=5, route="do_source", nslab=1, dt_years=5.0e5, rejected=[],
         curves=[dict(cls="gap", radii=[_u(1.2), _u(2.4)], factors=[1.9, 0.0, 0.5]), dict(cls="zero_one", radii=[_u(2.0)], factors=[1.0, 0.0])],
         set_order=["plane_curves", "beams", "curves", "horizons"]),
]


def case_list(ncases=None, seed=None):
    ncases, seed = NCASES if ncases is None else ncases, SEED if seed is None else seed
    return [dict(s) for s in FIXED] + [draw(np.random.default_rng(seed + i)) for i in range(ncases)]


def curved_list(ncurved=None, seed=None):
    ncurved, seed = NCURVED if ncurved is None else ncurved, SEED if seed is None else seed
    return [dict(s) for s in FIXED_CURVED] + [draw_curved(np.random.default_rng([seed, 1, i])) for i in range(ncurved)]


def full_list():
    """The default list with the curved list behind it: an old case keeps its number."""
    return case_list() + curved_list()


def source_curves(spec):
    """One entry per point source: None or the curve's dict."""
    return list(spec.get("curves") or [None] * len(spec["flux"]))


def has_curves(spec):
    return any(c is not None for c in source_curves(spec)) or any(p.get("curve") is not None for p in spec["planes"])


def tag(ic, spec):
    return f"case {ic}: {spec}"


# -- from a spec to a case and its settings ---------------------------------------------------------------------------------------
def d2_of(dr, o):
    """d2 as the predicate of csrc/c2ray_horizon.hpp forms it."""
    xs, ys, zs = (np.float64(dr[d]) * np.float64(o[d]) for d in range(3))
    return (xs * xs + ys * ys) + zs * zs


def radius_of(h, dr):
    name = h["radius_class"]
    if name == "none":
        return None
    if name == "inf":
        return float("inf")
    if name == "zero":
        return 0.0
    if name == "sub_cell":
        return 0.3 * min(float(x) for x in dr)
    if name == "huge":
        return 1e200
    if name == "uniform":
        return h["cells"] * float(dr[0])
    r = np.sqrt(d2_of(dr, h["offset"]))
    if h["nudge"]:
        r = np.nextafter(r, np.inf if h["nudge"] > 0 else 0.0)
    return float(r)


def is_finite(radius):
    return radius is not None and math.isfinite(radius)


def curve_of(c, dr):
    """(radii, factors) as HipEngine.set_source_curves takes them, or None."""
    if c is None:
        return None
    radii = [radius_of(h, dr) for h in c["radii"]]
    assert all(b > a for a, b in zip(radii, radii[1:])) and len(c["factors"]) == len(radii) + 1 <= cr.MAX_STEPS + 1, c
    return radii, [float(f) for f in c["factors"]]


def plane_curve_of(c, path):
    """(depths, factors, layer0, depth0) as HipEngine.set_plane_curve takes them, or None."""
    if c is None:
        return None
    layer0, depth0 = int(c["layer0"]), float(c["depth0"]) * float(path)
    depths = []
    for d in c["depths"]:
        if d["kind"] == "uniform":
            depths.append(float(d["paths"]) * float(path))
        else:
            x = pcr.layer_depth(depth0, layer0, d["m"], path)
            depths.append(float(np.nextafter(x, np.inf if d["nudge"] > 0 else 0.0)) if d["nudge"] else x)
    assert all(b > a for a, b in zip(depths, depths[1:])) and len(c["factors"]) == len(depths) + 1 <= 9, c
    return depths, [float(f) for f in c["factors"]], layer0, depth0


def is_pow2(f):
    return f > 0.0 and math.frexp(f)[0] == 0.5


def build(pkg, spec):
    """(AxisCase, settings): beams and horizons as HipEngine takes them, planes as mix_reference takes them, dt in seconds."""
    n, m = tuple(spec["n"]), tuple(spec["m"])
    kw = dict(heat=spec["heat"], pl=spec["pl"], qpl=spec["qpl"])
    if spec["mask"]:
        case = mr.make_case(pkg, spec["mask"], spec["srcpos"], spec["flux"], seed=spec["gas_seed"], mesh=(n, m), kind=spec["gas"], **kw)
        if spec["cubic"]:
            d = float(case.dr[0])
            case.dr, case.vol = (d, d, d), d * d * d
    else:
        import open_boundary_cases as ob
        case = br.periodic_case(pkg, n, spec["gas"], spec["srcpos"], spec["flux"], cubic=spec["cubic"], **kw)
        case.region = ob.gas(pkg, ab.cells(n), np.random.default_rng(spec["gas_seed"]), spec["gas"], spec["heat"])
        case.big = [a for a in case.region]
    case.check_embedding(case.m)
    assert embedding_ok(case.n, case.m, case.periodic)
    beams = [None if b["kind"] == 0 else (b["kind"], tuple(b["axis"]), b["cos_half"]) for b in spec["beams"]]
    horizons = [radius_of(h, case.dr) for h in spec["horizons"]]
    planes = []
    for p in spec["planes"]:
        flux = [f * mr.FLUX for f in p["flux"]]
        pl = dict(axis=p["axis"], from_high=p["from_high"], normflux=flux)
        assert not case.periodic[p["axis"]]
        if "tilt" in p:
            a_f, a_g = obr.geometry(p["tilt"], case.dr, p["axis"])[:2]
            assert 0.0 <= a_f <= 1.0 and 0.0 <= a_g <= 1.0 and a_f + a_g > 0.0, (a_f, a_g)
            pl["tilt"] = tuple(p["tilt"])
        if p["kind"] == "mapped":
            pl["fmap"] = mr.make_map(case, p["axis"], p["map_seed"], seds=3 if spec["multi"] else 1, scale=p["map_scale"])
        if "entry_seed" in p:
            pl["entry"] = mr.make_entry(case, p["axis"], p["entry_seed"])
        pl["curve"] = plane_curve_of(p.get("curve"), pcr.plane_path(case.dr, p["axis"], p.get("tilt")))
        planes.append(pl)
    curves = [curve_of(c, case.dr) for c in source_curves(spec)]
    settings = dict(beams=beams, horizons=horizons, planes=planes, curves=curves, dt=spec["dt_years"] * YEAR, maps=spec["maps"],
                    set_order=tuple(spec.get("set_order", SETTERS)),
                    horizon_loss=spec["horizon_loss"], batch=spec["batch"], route=spec["route"], nslab=spec["nslab"])
    return case, settings


def other_embedding(pkg, case, spec):
    """(m, big): the same region in a periodic mesh with another open extent and padding of another kind, or None where every
    axis is periodic."""
    if not spec["mask"]:
        return None
    if spec["tier"] == "B":
        m = [t for t in TIER_B.values() if t[0] == tuple(spec["n"]) and t[1] == spec["mask"]][0][3]
    else:
        m = tuple((26, 31, 31)[d] if ax in spec["mask"] else nd for d, (ax, nd) in enumerate(zip("xyz", spec["n"])))
    kind = "mixed" if spec["gas"] != "mixed" else "ionised"
    return m, case.embedding(pkg, m, ab.OTHER_PAD_SEED, kind)


def stripped(spec):
    """The spec without beams, horizons, planes and curves."""
    out = dict(spec)
    out["beams"] = [dict(b, kind=0) for b in spec["beams"]]
    out["horizons"] = [dict(radius_class="none") for _ in spec["horizons"]]
    out.update(planes=[], horizon_loss=False)
    if "curves" in spec:
        out["curves"] = [None] * len(spec["curves"])
    return out


def uncurved(spec):
    """The spec with every source and plane curve taken off; beams, horizons and planes kept."""
    out = dict(spec)
    out["curves"] = [None] * len(spec["flux"])
    out["planes"] = [dict(p, curve=None) for p in spec["planes"]]
    return out


# -- the rounds, from the predicates alone ----------------------------------------------------------------------------------------
def box_offsets(lo, hi):
    dk, dj, di = np.meshgrid(*(np.arange(lo[d], hi[d] + 1, dtype=np.int64) for d in (2, 1, 0)), indexing="ij")
    return di, dj, dk


def deciding_cells(case, ns, nbox):
    """(offsets, bool array) of the box of round nbox around source ns (0-based): the cells on the faces that decide whether the
    loop goes on after that round, by expected_trace's rule (all False where no face can still move)."""
    l, r = case.reach(ns)
    every = all(case.periodic)
    lo = [max(-ab.SUBBOXSIZE * nbox, l[d]) for d in range(3)]
    hi = [min(ab.SUBBOXSIZE * nbox, r[d]) for d in range(3)]
    short_lo, short_hi = [lo[d] > l[d] for d in range(3)], [hi[d] < r[d] for d in range(3)]
    o = box_offsets(lo, hi)
    decides = np.zeros(o[0].shape, dtype=bool)
    if (short_lo[2] and short_hi[2]) if every else (any(short_lo) or any(short_hi)):
        for d in range(3):
            if every or short_lo[d]:
                decides |= o[d] == lo[d]
            if every or short_hi[d]:
                decides |= o[d] == hi[d]
    return o, decides


def expected_trace(case, ns, beam, radius, curve=None):
    """(nbox, lo, hi) of source ns (0-based) where every lit cell of a surface that decides passes more than the threshold
    (ionised gas), and wherever one round is all there is.  The box of round nbox is +-subboxsize*nbox cut at the reach.  The
    loop goes on (include/c2ray_hip.h) while some face can still move -- all periodic: while both z faces are short of the
    reach, evolve_source.F90:136-139 -- and the loss that decides is not 0.0: the lit cells on the faces still short of the
    reach (all periodic: on the whole surface).  A cell in a shell of factor 0 of the source's curve is not lit."""
    l, r = case.reach(ns)
    every = all(case.periodic)
    nbox = 0
    while True:
        nbox += 1
        lo = [max(-ab.SUBBOXSIZE * nbox, l[d]) for d in range(3)]
        hi = [min(ab.SUBBOXSIZE * nbox, r[d]) for d in range(3)]
        short_lo, short_hi = [lo[d] > l[d] for d in range(3)], [hi[d] < r[d] for d in range(3)]
        if not ((short_lo[2] and short_hi[2]) if every else (any(short_lo) or any(short_hi))):
            return nbox, lo, hi
        o = box_offsets(lo, hi)
        decides = np.zeros(o[0].shape, dtype=bool)
        for d in range(3):
            if every or short_lo[d]:
                decides |= o[d] == lo[d]
            if every or short_hi[d]:
                decides |= o[d] == hi[d]
        if not (decides & hr.lit_offsets(beam, radius, case.dr, *o) & (cr.factor_offsets(curve, case.dr, *o) != 0.0)).any():
            return nbox, lo, hi


def inside_cells(case, ns, lo, hi):
    """Flat bool array over the product mesh: the cells of the box lo..hi around source ns (0-based)."""
    o = br.offsets(case.n, case.srcpos[ns], case.periodic)
    ok = np.ones(o[0].shape, dtype=bool)
    for d in range(3):
        ok &= (o[d] >= lo[d]) & (o[d] <= hi[d])
    return ok.reshape(-1)


# -- the composer -----------------------------------------------------------------------------------------------------------------
_composed = {}


def case_key(spec):
    """Names what the oracle's runs of a source alone depend on: mesh, gas, cells, sources -- no beam, horizon or plane."""
    return "extfuzz " + repr([spec[k] for k in ("mask", "n", "m", "gas", "gas_seed", "cubic", "heat", "srcpos", "flux", "pl", "qpl")])


def plane_reference(orc, otables, case, plane):
    """mix_reference.plane_alone, or plane_curve_reference.curve_pass where the plane has a curve (the host test holds the two
    to each other without one)."""
    if plane.get("curve") is None:
        return mr.plane_alone(orc, otables, case, plane)
    return curve_pass(orc, otables, case, plane, plane["curve"])


def curve_pass(orc, otables, case, plane, curve):
    ndens, xh, xhe, _ = case.region
    tilted, mapped = mr.plane_kind(plane)
    return pcr.curve_pass(orc, otables, case.n, case.dr, case.vol, ndens, xh, xhe, plane["axis"], plane["from_high"],
                          normflux=None if mapped else plane["normflux"], flux_map=plane["fmap"] if mapped else None, curve=curve,
                          tilt=plane["tilt"] if tilted else None, periodic=case.periodic, heat=case.heat, entry=plane.get("entry"))


def _scaled_run(pkg, orc, otables, case, key, ns, f):
    """curve_reference.source_scaled for a factor that is no power of two; rim_reference is handed the same run."""
    grids, nb, _, pair = cr.source_scaled(pkg, orc, otables, case, key, ns, f)
    rr._runs.setdefault((cr.scaled_key(key, ns - 1, f), ns - 1), (pair[0], pair[1], nb))
    return grids


def curved_term(pkg, orc, otables, case, key, ns, curve, base):
    """The term of source ns (1-based): in each cell of shell b the oracle's run with the fluxes times factor[b] -- base * factor
    for a power of two -- and 0.0 in a shell of factor 0."""
    ncell = ab.cells(case.n)
    shell, fac = cr.shell_cells(case, ns - 1, curve), cr.factors_of(curve)
    term = {k: np.zeros(base[k].size) for k in GRIDS}
    for b, f in enumerate(fac):
        here = shell == b
        if f == 0.0 or not here.any():
            continue
        grids = {k: f * base[k] for k in GRIDS} if is_pow2(f) else _scaled_run(pkg, orc, otables, case, key, ns, f)
        for k in GRIDS:
            m = np.tile(here, term[k].size // ncell)
            term[k][m] = grids[k][m]
    return term


def curved_face_terms(pkg, orc, otables, case, key, ns, curve, cached):
    """face_loss_reference's (m1, o, term) list of source ns (1-based) with each term from the run of its cell's shell, as
    curve_reference.compose_maps takes it."""
    fac = cr.factors_of(curve)
    out, scaled = [], {}
    for m1, o, term in cached:
        f = float(fac[int(cr.shell_offsets(curve, case.dr, o[0], o[1], o[2]))])
        if f == 0.0 or is_pow2(f):
            out.append((m1, o, f * term))
            continue
        if f not in scaled:
            scaled[f] = {a: t for a, _, t in cr.face_terms(pkg, orc, otables, case, key, ns - 1, f)}
        out.append((m1, o, scaled[f][m1]))
    return out


def curved_rim_terms(pkg, orc, otables, case, key, ns, curve, radius, lo, hi, beam, base, rule):
    """The rim terms of source ns (1-based) as curve_reference.rim_terms composes them: each face cell from the run of its own
    shell's factor (base * factor for a power of two), +0.0 in a shell of factor 0."""
    fac = cr.factors_of(curve)
    shell = cr.shell_offsets(curve, case.dr, rule["cell"][:, 0], rule["cell"][:, 1], rule["cell"][:, 2])
    face = rule["face"] & (fac[shell] != 0.0)
    terms = np.zeros(len(base))
    for b in sorted(set(int(x) for x in shell[face])):
        f = float(fac[b])
        if is_pow2(f):
            one = f * base
        else:
            _scaled_run(pkg, orc, otables, case, key, ns, f)
            one, _ = rr.source_terms(pkg, orc, otables, cr.scaled_case(case, ns, f), cr.scaled_key(key, ns - 1, f), ns - 1, radius, lo, hi, beam)
        pick = face & (shell == b)
        terms[pick] = one[pick]
    return terms


def compose_all(pkg, orc, otables, case, spec):
    """Everything the product is expected to report for the spec; computed once per session and never changed by a caller (the
    reference modules' caches are keyed by case_key).
    Returns phih_grid, phihe_grid, phiheat, sum_nbox, trace ([(nbox, lo, hi)] per source), oracle_nbox, maps ({face: [b, a]}),
    plane ({number: that plane's reference}), horizon_terms / horizon_rule ({ns (1-based): ...} for the sources with a
    finite radius, when the loss is on), horizon_loss (per source) and horizon_total, rim_source (the horizoned source swept
    last, or None), loss (the reference of photon_loss(1), or None), lit_fraction (per source), and conv, xh_av, xhe_av,
    xh_intermed, xhe_intermed, temperature after the oracle's global pass on the composed grids."""
    key = case_key(spec)
    if repr(spec) in _composed:
        return _composed[repr(spec)]
    _, cfg = build(pkg, spec)
    beams, horizons, planes, curves = cfg["beams"], cfg["horizons"], cfg["planes"], cfg["curves"]
    nsrc, ncell = len(case.flux), ab.cells(case.n)
    assert spec["tier"] == "A" or all(f == 0.0 or is_pow2(f) for c in curves if c is not None for f in c[1]), "tier B: 0 and powers of two"
    # the planes, in plane order from 0.0
    refs = {p: plane_reference(orc, otables, case, planes[p - 1]) for p in range(1, len(planes) + 1)}
    grids = mr.fold_planes(case, refs, list(range(1, len(planes) + 1)))
    # the point sources, in source order
    trace, oracle_nbox, lit_fraction, masks = [], [], [], []
    for ns in range(1, nsrc + 1):
        term, nb, _, pair = br.source_alone(pkg, orc, otables, case, key, ns)
        oracle_nbox.append(nb)
        rr._runs.setdefault((key, ns - 1), (pair[0], pair[1], nb))       # the run rim_reference would otherwise repeat
        tr = expected_trace(case, ns - 1, beams[ns - 1], horizons[ns - 1], curves[ns - 1])
        trace.append(tr)
        lit = br.lit_cells(case, ns - 1, beams[ns - 1])
        lit_fraction.append(float(lit.mean()))
        mask = lit & hr.within_cells(case, ns - 1, horizons[ns - 1]) & inside_cells(case, ns - 1, tr[1], tr[2])
        if curves[ns - 1] is not None:
            term = curved_term(pkg, orc, otables, case, key, ns, curves[ns - 1], term)
            mask = mask & (cr.factor_cells(case, ns - 1, curves[ns - 1]) != 0.0)
        masks.append(mask)
        for k in GRIDS:
            grids[k] = grids[k] + np.where(np.tile(mask, grids[k].size // ncell), term[k], 0.0)
    out = dict(grids, sum_nbox=sum(t[0] for t in trace), trace=trace, oracle_nbox=oracle_nbox, plane=refs, lit_fraction=lit_fraction,
               same_cells=mr.same_cells(case, range(1, nsrc + 1), oracle_nbox))
    # the escape maps: the planes' terms first, then the masked per-source terms
    n = tuple(int(x) for x in case.n)
    maps = {f: np.zeros(fl.face_shape(n, f)) for f in fl.open_faces(case.periodic)}
    per_source = []
    if maps:
        for p in range(1, len(planes) + 1):
            far = 2 * planes[p - 1]["axis"] + (1 - planes[p - 1]["from_high"])
            maps[far] = maps[far] + refs[p]["terms"].reshape(fl.face_shape(n, far))
        fl.expected(pkg, orc, otables, case, key)
        for ns in range(1, nsrc + 1):
            _, lo, hi = trace[ns - 1]
            cached = fl.cached_terms(key, ns - 1)
            o3 = np.array([o for _, o, _ in cached], dtype=np.int64).reshape(-1, 3)
            lit = hr.lit_offsets(beams[ns - 1], horizons[ns - 1], case.dr, o3[:, 0], o3[:, 1], o3[:, 2])
            for d in range(3):
                lit = lit & (o3[:, d] >= lo[d]) & (o3[:, d] <= hi[d])
            if curves[ns - 1] is not None:
                cached = curved_face_terms(pkg, orc, otables, case, key, ns, curves[ns - 1], cached)
            terms = [(m1, o, term if ok else 0.0) for (m1, o, term), ok in zip(cached, lit)]
            one = fl.maps_of_terms(case, terms)
            one = {f: one[f].reshape(fl.face_shape(n, f)) for f in one}
            per_source.append(one)
            for f in maps:
                maps[f] = maps[f] + one[f]
    out["maps"] = maps
    out["loss"] = None
    if mr.has_loss_reference(case) and all(b is None for b in beams) and all(h is None or h == float("inf") for h in horizons):
        out["loss"] = math.fsum([refs[p]["loss"] for p in refs] + [fl.total_of(one) for one in per_source])
    # the horizon loss
    out.update(horizon_terms={}, horizon_rule={}, horizon_loss=np.zeros(nsrc), horizon_total=0.0, rim_source=None)
    if cfg["horizon_loss"]:
        for ns in range(1, nsrc + 1):
            if not is_finite(horizons[ns - 1]):
                continue
            _, lo, hi = trace[ns - 1]
            terms, rule = rr.source_terms(pkg, orc, otables, case, key, ns - 1, horizons[ns - 1], lo, hi, beams[ns - 1])
            if curves[ns - 1] is not None:
                terms = curved_rim_terms(pkg, orc, otables, case, key, ns, curves[ns - 1], horizons[ns - 1], lo, hi, beams[ns - 1], terms, rule)
            out["horizon_terms"][ns], out["horizon_rule"][ns] = terms, rule
            out["horizon_loss"][ns - 1] = rr.face_sum(terms)
            out["rim_source"] = ns
        total = 0.0
        for x in out["horizon_loss"]:
            total = total + float(x)
        out["horizon_total"] = total
    # the global pass: the oracle's, on the product mesh, from the composed grids
    hp = pkg.hostphys
    ndens, xh, xhe, temp = case.region
    kw = {}
    if case.pl is not None:
        kw = dict(normflux_pl=case.pl, normflux_qpl=case.qpl, pl_s_star=case.pl_s_star, qpl_s_star=case.qpl_s_star)
    st = orc.Step(case.n, case.dr, case.vol, ab.ZRED, hp.H0, hp.Omega0, not case.heat, 1.0e4, 1.0, case.srcpos, case.flux, case.s_star,
                  ndens, case.reccoef, **kw)
    s = orc.State(st, xh, xhe, temp)
    orc.begin_step(s)
    s.phih[:], s.phihe[:], s.phiheat[:] = grids["phih_grid"], grids["phihe_grid"], grids["phiheat"]
    out["conv"] = int(orc.global_pass(otables, st, s, cfg["dt"]))
    for k in ab.ITER_STATE:
        out[k] = getattr(s, k).copy()
    out["temperature"] = None if s.temperature is None else s.temperature.copy()
    _composed[repr(spec)] = out
    return out
