"""Seeded sequences of time steps for ONE context, shared by tests/test_step_sequence_host.py (CPU) and
tests/test_gpu_step_sequence.py (GPU).  Not a test module; no GPU, no torch.

A sequence is a dict: name, why, mesh (fixed for the life of the context), multi (the extra SED tables are set at the start)
and 5 to 8 steps.  A step is a complete description of its inputs, made of plain Python values, never a difference against
the step before -- the oracle is built from the step alone (inputs()), apart from a state that is carried:

  excursion  None, or dict(periodic=[..3..], zred, aniso): before the step's own setters one pass and one global pass run with
             these boundaries and cell sizes (set_step_scalars), on whatever the context holds; nothing of it is asserted (the
             oracle is periodic), the boundaries then return to periodic.  Such a step uploads its gas.
  tables     dict(scale, how): the photo_thick table of the black body times `scale`; how it reaches the device: "keep" (no
             call: scale is what the step before had), "upload", "upload_noheat" (without heating tables, isothermal
             stretches only; `heat` says whether the device holds heating tables after the step) or "build" (built on the
             device from sed_setup.npz, scale 1.0 only).
  zred, aniso, dens, route
             cell sizes are hp.test_grid(24, zred) times (1, 1, 1) or ANISO; dens = dict(seed, z0, spread, divs): a log-normal
             field around hp.test_density(z0), divided by each of divs in turn.  route: "set_step" (the array is uploaded),
             "scale" (scale_ndens(divs[-1]) + set_step_scalars: dens is the step before's with one more divisor, the
             reference's cosmo_evol) or "scalars" (set_step_scalars alone: dens is the step before's).
  iso, clump, lls
             clump = dict(kind="scalar" | "grid", value, seed), lls = dict(kind="off" | "scalar" | "grid", value, seed).
             On the routes without set_step the LLS and clumping-grid calls are made only when the setting changed.
  src        dict(pos, flux, pl, qpl, change): the whole list; pl / qpl None means no set_sources_sed after set_sources.
  batch      set_batch.
  gas        dict(kind="ionised" | "opaque" | "mixed", seed) is uploaded; dict(kind="carried") means no upload_state: the step
             starts from what end_step left, in the oracle from the oracle's own end state of the step before.
  run        dict(kind="whole", dt) is evolve3d(dt); dict(kind="stepwise", dt, iters, slabs, cut) is begin_step, then `iters`
             times set_rates_to_zero, the pass (slabs 0: pass_sources, else pass_sources_begin/wait/end with that many
             slabs) and the global pass (cut None: global_pass, else global_pass_cells in two pieces and finish), end_step.
             mid = dict(how="scale" | "set_step", divisor), hand-written sequences only: between the two iterations the
             density is divided once more, by scale_ndens or by set_step with the divided array, and no begin_step follows --
             the one call order in which the second pass could sweep with the first global pass's neufrac * ndens products.
             `dens` is the density of the first iteration; the next step takes the route "set_step".

The list is FIXED + [draw(default_rng([SEED, i])) for i < NCASES]; C2R_SEQFUZZ_CASES / C2R_SEQFUZZ_SEED widen or move it.

Meshes.  The oracle's box loop ends on the z reach alone (evolve_source.F90:130: last_r(3) < lastpos_r(3)), so on a periodic
mesh of at most 24 cells along z no source ever runs more than two rounds of ten cells.  The cube of 24^3 is here, and one
mesh is longer along z than anything else in this module, "deep" = (12, 8, 44) with 4224 cells: its z reach is 21 / 22 cells,
three rounds in ionised gas, which is what "three rounds learnt, one needed" takes.  A whole evolve3d call converges only where
int(2.5e-4 * cells) >= 1, i.e. from 4000 cells on: the thin and tiny meshes run stepwise only.
"""
import copy
import os

import numpy as np

DEFAULT_CASES, DEFAULT_SEED = 6, 20261101
NCASES = int(os.environ.get("C2R_SEQFUZZ_CASES", str(DEFAULT_CASES)))
SEED = int(os.environ.get("C2R_SEQFUZZ_SEED", str(DEFAULT_SEED)))

YEAR = 3.15576e7
EXTRA_SEDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rad_tables_pl_qpl.npz")
MESHES = {"cube": (24, 24, 24), "ragged": (24, 16, 20), "deep": (12, 8, 44), "thin": (12, 5, 8), "two_deep": (24, 2, 2),
          "tiny": (9, 7, 5)}
ANISO = (1.0, 1.25, 0.75)
ZREDS = (9.0, 7.5, 6.0, 11.0)
S_STAR, PL_S_STAR, QPL_S_STAR = 1.0e48, 1.5e48, 0.7e48
TEMPER_VAL = 1.0e4
CONVERGENCE_FRACTION = float(np.float32(2.5e-4))
SOURCE_CHANGES = ("same", "fluxes", "permuted", "grown", "shrunk", "moved", "twin", "zero", "none")
# what a step is compared in, in the order a failure lists it
ITEMS = ("cells", "density", "table", "sources", "seds", "lls", "clump", "iso", "gas")


def whole_ok(mesh, nsrc):
    """A whole evolve3d call can converge: its criterion min(int(fraction * cells), nsrc) is at least 1."""
    return min(int(CONVERGENCE_FRACTION * mesh[0] * mesh[1] * mesh[2]), nsrc) >= 1


# -- a step's inputs as arrays ------------------------------------------------------------------------------------------------
def cell_sizes(hp, zred, aniso):
    d = hp.test_grid(24, zred)[0][0]
    dr = tuple(d * f for f in (ANISO if aniso else (1.0, 1.0, 1.0)))
    return dr, dr[0] * dr[1] * dr[2]


def density(hp, dens, ncell):
    nd = hp.test_density(dens["z0"]) * np.exp(np.random.default_rng(dens["seed"]).normal(0.0, dens["spread"], ncell))
    for d in dens["divs"]:
        nd = nd / d                                      # what k_divide_by does, one rounded division per cell
    return nd


def gas_state(gas, ncell, heat):
    """Ionised fractions of tests/open_boundary_cases.gas: 'ionised' runs every box to its reach, 'opaque' stops it after one
    round, 'mixed' lies between.  (xh, xhe, temperature or None)."""
    rng = np.random.default_rng(gas["seed"])
    if gas["kind"] == "mixed":
        x = 10.0 ** rng.uniform(-6, -0.3, ncell)
    elif gas["kind"] == "ionised":
        x = 1.0 - 10.0 ** rng.uniform(-4.5, -3.5, ncell)
    elif gas["kind"] == "opaque":
        x = 10.0 ** rng.uniform(-6, -5, ncell)
    else:
        raise ValueError(gas["kind"])
    xh = np.concatenate([1.0 - x, x])
    xhe = np.concatenate([1.0 - x, 0.8 * x, 0.2 * x])
    temp = np.tile((1e4 * np.exp(rng.normal(0, 0.2, ncell))).astype(np.float32), 3) if heat else None
    return xh, xhe, temp


def lls_arrays(lls, ncell):
    """(coldensh_lls or None, lls_grid or None)"""
    if lls["kind"] == "scalar":
        return float(lls["value"]), None
    if lls["kind"] == "grid":
        return None, (10.0 ** np.random.default_rng(lls["seed"]).uniform(15.0, 17.5, ncell)).astype(np.float32)
    return None, None


def clump_grid(clump, ncell):
    if clump["kind"] == "grid":
        return (1.0 + 5.0 * np.random.default_rng(clump["seed"]).random(ncell)).astype(np.float32)
    return None


def inputs(hp, seq, step):
    """Everything of a step but its gas, as arrays: a dict."""
    mesh = seq["mesh"]
    nc = mesh[0] * mesh[1] * mesh[2]
    dr, vol = cell_sizes(hp, step["zred"], step["aniso"])
    s = step["src"]
    coldensh_lls, lls_grid = lls_arrays(step["lls"], nc)
    return dict(mesh=mesh, ncell=nc, dr=dr, vol=vol, zred=step["zred"], ndens=density(hp, step["dens"], nc), iso=step["iso"],
                clumping=float(step["clump"]["value"]), clumping_grid=clump_grid(step["clump"], nc),
                coldensh_lls=coldensh_lls, lls_grid=lls_grid, reccoef=hp.reccoef(TEMPER_VAL),
                srcpos=np.asarray(s["pos"], dtype=np.int32).reshape(-1, 3), flux=np.asarray(s["flux"], dtype=np.float64),
                pl=None if s["pl"] is None else np.asarray(s["pl"], dtype=np.float64),
                qpl=None if s["qpl"] is None else np.asarray(s["qpl"], dtype=np.float64))


def changed_items(prev, step):
    """The items of ITEMS in which `step` differs from the step before it."""
    out = []
    if (prev["zred"], prev["aniso"]) != (step["zred"], step["aniso"]):
        out.append("cells")
    if prev["dens"] != step["dens"]:
        out.append("density")
    if prev["tables"]["scale"] != step["tables"]["scale"]:
        out.append("table")
    if (prev["src"]["pos"], prev["src"]["flux"]) != (step["src"]["pos"], step["src"]["flux"]):
        out.append("sources")
    if _seds_for(prev["src"], len(step["src"]["flux"])) != (step["src"]["pl"], step["src"]["qpl"]):
        out.append("seds")
    for k in ("lls", "clump", "iso"):
        if prev[k] != step[k]:
            out.append(k)
    if step["gas"]["kind"] != "carried":
        out.append("gas")
    return out


def _seds_for(src, nsrc):
    """The SED fluxes of another step's list, cut or zero-filled to nsrc sources: what a context that forgot to clear them holds."""
    return tuple(None if f is None or not nsrc else (list(f) + [0.0] * nsrc)[:nsrc] for f in (src["pl"], src["qpl"]))


def put_back(prev, step, item):
    """`step` with one item at the value it had the step before ("gas": see run_step's `start`)."""
    out = copy.deepcopy(step)
    if item == "cells":
        out["zred"], out["aniso"] = prev["zred"], prev["aniso"]
    elif item == "density":
        out["dens"] = copy.deepcopy(prev["dens"])
    elif item == "table":
        out["tables"]["scale"] = prev["tables"]["scale"]
    elif item == "sources":
        n = len(step["src"]["flux"])
        if len(prev["src"]["flux"]) == n:
            out["src"]["pos"], out["src"]["flux"] = copy.deepcopy(prev["src"]["pos"]), list(prev["src"]["flux"])
        else:                                            # another length: the old list, with the SED fluxes cut to fit
            out["src"] = copy.deepcopy(prev["src"])
            out["src"]["pl"], out["src"]["qpl"] = _seds_for(step["src"], len(prev["src"]["flux"]))
    elif item == "seds":
        out["src"]["pl"], out["src"]["qpl"] = _seds_for(prev["src"], len(step["src"]["flux"]))
    elif item in ("lls", "clump", "iso"):
        out[item] = copy.deepcopy(prev[item])
    elif item == "excursion":
        out["zred"], out["aniso"] = step["excursion"]["zred"], step["excursion"]["aniso"]
    elif item != "gas":
        raise ValueError(item)
    return out


# -- the oracle --------------------------------------------------------------------------------------------------------------
def run_step(orc, T, hp, seq, step, start):
    """One step in the oracle from the state `start` = (xh, xhe, temperature or None): a dict of everything that is compared.
    The pass is the loop over do_source (as tests/oracle_engine.py), which also gives the rounds per source; the host test
    holds it against orc.evolve3d for the whole calls."""
    a = inputs(hp, seq, step)
    nc = a["ncell"]
    st = orc.Step(a["mesh"], a["dr"], a["vol"], a["zred"], hp.H0, hp.Omega0, a["iso"], TEMPER_VAL, a["clumping"], a["srcpos"],
                  a["flux"], S_STAR, a["ndens"], a["reccoef"], normflux_pl=a["pl"], normflux_qpl=a["qpl"], pl_s_star=PL_S_STAR,
                  qpl_s_star=QPL_S_STAR, coldensh_lls=a["coldensh_lls"], lls_grid=a["lls_grid"], clumping_grid=a["clumping_grid"])
    xh, xhe, temp = start[:3]
    if not a["iso"] and temp is None:
        raise ValueError("a heating step needs a temperature: it cannot carry the state of an isothermal one")
    s = orc.State(st, xh, xhe, None if a["iso"] else temp)
    if len(start) > 3:                                   # no source: the columns stay what the last source of an earlier pass left
        s.coldensh_out[:], s.coldenshe_out[:] = start[3], start[4]
    run = step["run"]
    dt = run["dt"] * YEAR
    nsrc = len(step["src"]["flux"])
    whole = run["kind"] == "whole"
    criterion = min(int(CONVERGENCE_FRACTION * a["mesh"][0] * a["mesh"][1] * a["mesh"][2]), nsrc)
    orc.begin_step(s)
    niter, conv, flags, nbox, loss, rounds = 0, nc, [], [], 0.0, []
    while True:
        if whole and ((conv < criterion and niter > 1) or niter > 500):
            break
        if not whole and niter == run["iters"]:
            break
        niter += 1
        s.phih[:], s.phihe[:], s.phiheat[:] = 0.0, 0.0, 0.0
        nbox, loss = [], 0.0
        for ns in range(1, nsrc + 1):
            nb, ls = orc.do_source(T, st, s, ns)
            nbox.append(int(nb))
            loss += ls
        rounds.append(list(nbox))
        conv = int(orc.global_pass(T, st, s, dt))
        flags.append(conv)
        if niter == 1 and not whole and run.get("mid"):
            st.ndens[:] = st.ndens / run["mid"]["divisor"]
    s.xh[:], s.xhe[:] = s.xh_intermed, s.xhe_intermed      # end_step
    if s.temperature is not None:
        s.temperature[2 * nc:] = s.temperature[:nc]
    out = dict(sum_nbox=int(sum(nbox)), coldensh_out=s.coldensh_out.copy(), coldenshe_out=s.coldenshe_out.copy(),
               phih=s.phih.copy(), phihe=s.phihe.copy(), xh_av=s.xh_av.copy(), xhe_av=s.xhe_av.copy(),
               xh_intermed=s.xh_intermed.copy(), xhe_intermed=s.xhe_intermed.copy(), xh=s.xh.copy(), xhe=s.xhe.copy(),
               photon_loss=float(loss), nbox=list(nbox), rounds=rounds, step=st, state=s)
    if not a["iso"]:
        out.update(phiheat=s.phiheat.copy(), temperature=s.temperature.copy())
    if whole:
        out.update(niter=niter, conv_flags=flags)
    return out


COMPARED = ("coldensh_out", "coldenshe_out", "phih", "phihe", "phiheat", "xh_av", "xhe_av", "xh_intermed", "xhe_intermed", "xh",
            "xhe", "temperature")


COUNTS = ("sum_nbox", "niter", "conv_flags", "nbox")       # compared with ==; nbox: the rounds per source of the last pass
LOSS_BOUND = 1e-12                                       # photon_loss, as tests/test_gpu_fuzz.py: its sum order differs


def loss_err(got, exp):
    """conftest.rel_err for one number."""
    return abs(got - exp) / max(abs(exp), 1e-300)


def differs(a, b, flags=True):
    """Two results of run_step differ in something that the GPU test compares, by the comparison it makes (its _mismatches):
    the counts of COUNTS, photon_loss beyond LOSS_BOUND, the arrays of COMPARED bit for bit.  flags=False: one of the two is
    a whole call rerun stepwise, which has no niter and no conv_flags."""
    if any(a.get(k) != b.get(k) for k in COUNTS if flags or k not in ("niter", "conv_flags")):
        return True
    if not loss_err(a["photon_loss"], b["photon_loss"]) <= LOSS_BOUND:
        return True
    return any((k in a) != (k in b) or (k in a and not np.array_equal(a[k], b[k])) for k in COMPARED)


def start_state(seq, i, before):
    """What step i starts from: its own gas, or the end state of the step before (`before`: that step's result)."""
    step = seq["steps"][i]
    nc = seq["mesh"][0] * seq["mesh"][1] * seq["mesh"][2]
    if step["gas"]["kind"] == "carried":
        start = (before["xh"], before["xhe"], before.get("temperature"))
    else:
        start = gas_state(step["gas"], nc, not step["iso"])
    if not step["src"]["flux"] and before is not None:
        start = tuple(start) + (before["coldensh_out"], before["coldenshe_out"])
    return start


def make_tables_for(pkg, orc):
    """(scale, multi) -> the oracle's tables: the shipped ones, photo_thick times scale, with the two extra SEDs or without."""
    cache = {}

    def get(scale, multi):
        if (scale, multi) not in cache:
            with np.load(pkg.evolve.DEFAULT_TABLES) as z:
                d = {k: z[k] for k in z.files}
            if multi:
                with np.load(EXTRA_SEDS) as z:
                    d.update({k: z[k] for k in z.files})
            d["photo_thick"] = np.ascontiguousarray(d["photo_thick"] * scale)
            cache[(scale, multi)] = orc.Tables(d)
        return cache[(scale, multi)]
    return get


def run_oracle(orc, tables_for, seq, hp):
    """The expected results per step (run_step's dicts), each from the step's own description and, where the step carries its
    state, the end state of the step before.  tables_for(scale, multi) gives the oracle's tables."""
    out = []
    for i, step in enumerate(seq["steps"]):
        T = tables_for(step["tables"]["scale"], seq["multi"])
        out.append(run_step(orc, T, hp, seq, step, start_state(seq, i, out[-1] if out else None)))
    return out


def check(seq):
    """The rules a sequence keeps (the generator's and the hand-written ones alike); raises AssertionError."""
    mesh, steps = seq["mesh"], seq["steps"]
    assert 5 <= len(steps) <= 8, len(steps)
    heat_on_device = False
    for i, st in enumerate(steps):
        prev = steps[i - 1] if i else None
        tag = (seq["name"], i)
        t = st["tables"]
        assert t["how"] in ("keep", "upload", "upload_noheat", "build"), tag
        if i == 0:
            assert t["how"] != "keep" and st["route"] == "set_step" and st["gas"]["kind"] != "carried" and not st["excursion"], tag
            assert not seq["multi"] or t["how"] != "build", tag          # the extra SEDs' tables are uploaded once, at the start
        if t["how"] == "keep":
            assert t["scale"] == prev["tables"]["scale"], tag
        if st["excursion"]:
            assert prev["src"]["flux"] and len(st["excursion"]["periodic"]) == 3 and not all(st["excursion"]["periodic"]), tag
        if t["how"] == "build":
            assert t["scale"] == 1.0, tag
        if t["how"] == "upload_noheat":
            heat_on_device = False
        elif t["how"] != "keep":
            heat_on_device = True
        assert t["heat"] == heat_on_device, tag
        assert st["iso"] or heat_on_device, tag
        if st["route"] == "scalars":
            assert st["dens"] == prev["dens"], tag
        if st["route"] == "scale":
            assert st["dens"]["divs"][:-1] == prev["dens"]["divs"] and {k: v for k, v in st["dens"].items() if k != "divs"} == \
                {k: v for k, v in prev["dens"].items() if k != "divs"}, tag
            assert st["dens"]["divs"][-1] == ((1.0 + prev["zred"]) / (1.0 + st["zred"])) ** 3, tag
        if st["gas"]["kind"] == "carried":
            assert not st["excursion"] and (st["iso"] or not prev["iso"]), tag
        s = st["src"]
        n = len(s["flux"])
        assert n <= 6 and len(s["pos"]) == n and s["change"] in SOURCE_CHANGES, tag
        assert all(1 <= p[d] <= mesh[d] for p in s["pos"] for d in range(3)), tag
        assert all(f is None or (len(f) == n and seq["multi"]) for f in (s["pl"], s["qpl"])), tag
        assert n > 0 or (s["pl"] is None and s["qpl"] is None and not st["excursion"] and i > 0), tag
        if st["run"]["kind"] == "whole":
            assert whole_ok(mesh, n), tag
        else:
            assert st["run"]["iters"] in (1, 2), tag
            if st["run"]["mid"]:
                assert st["run"]["iters"] == 2 and st["run"]["mid"]["how"] in ("scale", "set_step"), tag
        if prev is not None and prev["run"].get("mid"):
            assert st["route"] == "set_step", tag
        assert st["batch"] >= 1, tag


# -- the generator -----------------------------------------------------------------------------------------------------------
def _fluxes(rng, n, gas_kind):
    lo, hi = (4.0, 5.0) if gas_kind == "opaque" else (6.3, 7.5)
    return [float(x) for x in 10.0 ** rng.uniform(lo, hi, n)]


def _cell(rng, mesh):
    return [int(rng.integers(1, nd + 1)) for nd in mesh]


def _draw_sources(rng, mesh, prev, gas_kind, first_corner):
    """The next source list and the name of the change."""
    if prev is None or not prev["flux"]:
        n = int(rng.integers(1, 5))
        pos = [_cell(rng, mesh) for _ in range(n)]
        if first_corner:
            pos[0] = [1, 1, 1]
        return dict(pos=pos, flux=_fluxes(rng, n, gas_kind), change="grown")
    pos, flux = copy.deepcopy(prev["pos"]), list(prev["flux"])
    n = len(flux)
    change = SOURCE_CHANGES[int(rng.integers(0, len(SOURCE_CHANGES)))]
    if change in ("permuted", "shrunk", "moved") and n < 2:
        change = "grown"
    if change == "grown" and n >= 6:
        change = "shrunk"
    if change == "zero" and sum(f > 0.0 for f in flux) < 2:   # some source stays lit: a dark list shows no change of anything
        change = "fluxes"
    if change == "fluxes":
        flux = _fluxes(rng, n, gas_kind)
    elif change == "permuted":
        order = [int(x) for x in rng.permutation(n)]
        while order == list(range(n)):
            order = [int(x) for x in rng.permutation(n)]
        pos, flux = [pos[o] for o in order], [flux[o] for o in order]
    elif change == "grown":
        for _ in range(int(rng.integers(1, min(2, 6 - n) + 1))):
            pos.append(_cell(rng, mesh))
            flux.append(_fluxes(rng, 1, gas_kind)[0])
    elif change == "shrunk":
        lit = [k for k in range(n) if flux[k] > 0.0]
        k = int(rng.choice([k for k in range(n) if lit != [k]]))
        del pos[k], flux[k]
    elif change == "moved":                               # j takes the cell k held, k goes somewhere new
        k = int(rng.integers(0, n))
        j = (k + 1 + int(rng.integers(0, n - 1))) % n
        pos[j] = list(pos[k])
        pos[k] = _cell(rng, mesh)
    elif change == "twin":
        if n < 2:
            pos.append(list(pos[0]))
            flux.append(_fluxes(rng, 1, gas_kind)[0])
        else:
            pos[1] = list(pos[0])
    elif change == "zero":
        flux[int(rng.choice([k for k in range(n) if flux[k] > 0.0]))] = 0.0
    elif change == "none":
        pos, flux = [], []
    return dict(pos=pos, flux=flux, change=change)


def _draw_seds(rng, src, multi, gas_kind):
    n = len(src["flux"])
    mode = int(rng.integers(0, 4)) if multi and n else 0      # neither, the power law, the quasar-like one, both
    lo, hi = (3.5, 4.5) if gas_kind == "opaque" else (5.5, 7.0)
    src["pl"] = [float(x) for x in 10.0 ** rng.uniform(lo, hi, n)] if mode in (1, 3) else None
    src["qpl"] = [float(x) for x in 10.0 ** rng.uniform(lo, hi, n)] if mode in (2, 3) else None


def _draw_run(rng, mesh, nsrc, ncell):
    dt = float(10.0 ** rng.uniform(4.5, 5.5))
    if whole_ok(mesh, nsrc) and rng.random() < 0.5:
        return dict(kind="whole", dt=dt)
    return dict(kind="stepwise", dt=dt, iters=int(rng.integers(1, 3)), slabs=int(rng.integers(1, 9)) if rng.random() < 0.4 else 0,
                cut=int(rng.integers(0, ncell + 1)) if rng.random() < 0.4 else None, mid=None)


def draw(rng):
    name = str(rng.choice(sorted(MESHES)))
    mesh = MESHES[name]
    nc = mesh[0] * mesh[1] * mesh[2]
    multi = bool(rng.random() < 0.5)
    nsteps = int(rng.integers(5, 9)) if nc < 8000 else int(rng.integers(5, 7))
    steps = []
    heat_on_device, scale = True, 1.0
    for i in range(nsteps):
        prev = steps[-1] if steps else None
        st = {}
        # 7: an excursion to other boundaries and cell sizes
        st["excursion"] = None
        if prev is not None and prev["src"]["flux"] and rng.random() < 0.25:
            per = [int(x) for x in rng.integers(0, 2, 3)]
            if all(per):
                per[int(rng.integers(0, 3))] = 0
            st["excursion"] = dict(periodic=per, zred=float(rng.choice([8.0, 5.0])), aniso=bool(rng.random() < 0.5))
        # 3: the mode
        iso = bool(rng.random() < 0.5) if prev is None else (not prev["iso"] if rng.random() < 0.35 else prev["iso"])
        st["iso"] = iso
        # 1: the gas
        may_carry = prev is not None and not st["excursion"] and (iso or not prev["iso"])
        if may_carry and rng.random() < 0.4:
            st["gas"] = dict(kind="carried")
            gas_kind = "ionised"
        else:
            gas_kind = str(rng.choice(["ionised", "ionised", "opaque", "mixed"]))
            st["gas"] = dict(kind=gas_kind, seed=int(rng.integers(1 << 30)))
        # 4, 5: sources and their SEDs
        src = _draw_sources(rng, mesh, prev["src"] if prev else None, gas_kind, name in ("cube", "deep"))
        if src["change"] == "none" and st["excursion"]:
            st["excursion"] = None
        _draw_seds(rng, src, multi, gas_kind)
        st["src"] = src
        n = len(src["flux"])
        # 6: the tables
        how = "upload" if prev is None else "keep"
        if prev is not None and n and gas_kind in ("opaque", "mixed") and st["gas"]["kind"] != "carried" and rng.random() < 0.6:
            # (another photo_thick shows only in cells that are not optically thin: not in uploaded "ionised" gas)
            if scale == 1.0:
                scale, how = float(rng.choice([0.5, 2.0])), ("upload_noheat" if iso and rng.random() < 0.5 else "upload")
            else:
                scale, how = 1.0, str(rng.choice(["upload", "build"]))
        if not iso and not heat_on_device and how in ("keep", "upload_noheat"):
            how = "upload"
        heat_on_device = how != "upload_noheat" and (heat_on_device or how != "keep")
        st["tables"] = dict(scale=scale, how=how, heat=heat_on_device)
        # 2: geometry and density
        zred = float(ZREDS[0]) if prev is None else prev["zred"]
        aniso = bool(rng.random() < 0.3) if prev is None else (not prev["aniso"] if rng.random() < 0.3 else prev["aniso"])
        route = "set_step"
        if prev is not None and not n:                        # no source: cell sizes, tables and LLS would change nothing
            aniso, route = prev["aniso"], str(rng.choice(["set_step", "scalars"]))
        elif prev is not None:
            if rng.random() < 0.6:
                zred = float(rng.choice([z for z in ZREDS if z != prev["zred"]]))
                route = str(rng.choice(["set_step", "scale", "scalars"]))
            else:
                route = str(rng.choice(["set_step", "scalars"]))
        if route == "set_step":
            dens = dict(seed=int(rng.integers(1 << 30)), z0=zred, spread=0.7, divs=[])
        elif route == "scale":
            dens = copy.deepcopy(prev["dens"])
            dens["divs"].append(((1.0 + prev["zred"]) / (1.0 + zred)) ** 3)
        else:
            dens = copy.deepcopy(prev["dens"])
        st.update(zred=zred, aniso=aniso, dens=dens, route=route)
        # clumping and LLS
        if prev is None or rng.random() < 0.35:
            kind = str(rng.choice(["scalar", "grid"]))
            st["clump"] = dict(kind=kind, value=float(rng.choice([1.0, 1.75, 2.5])), seed=int(rng.integers(1 << 30)) if kind == "grid" else 0)
        else:
            st["clump"] = copy.deepcopy(prev["clump"])
        if prev is None or (n and rng.random() < 0.35):
            kind = str(rng.choice(["off", "scalar", "grid"]))
            st["lls"] = dict(kind=kind, value=float(10.0 ** rng.uniform(15, 17)) if kind == "scalar" else 0.0,
                             seed=int(rng.integers(1 << 30)) if kind == "grid" else 0)
        else:
            st["lls"] = copy.deepcopy(prev["lls"])
        # 8: how it runs
        st["batch"] = int(rng.choice([1, max(1, n - 1), n + 2]))
        st["run"] = _draw_run(rng, mesh, n, nc)
        steps.append(st)
    return dict(name=f"draw-{name}", why="drawn", mesh=mesh, multi=multi, steps=steps)


# -- the hand-written sequences ---------------------------------------------------------------------------------------------
def _step(**kw):
    st = dict(excursion=None, tables=dict(scale=1.0, how="keep", heat=True), zred=9.0, aniso=False,
              dens=dict(seed=2424, z0=9.0, spread=0.7, divs=[]), route="scalars", iso=True, clump=dict(kind="scalar", value=1.0, seed=0),
              lls=dict(kind="off", value=0.0, seed=0), src=None, batch=1, gas=dict(kind="carried"),
              run=dict(kind="stepwise", dt=1.0e5, iters=2, slabs=0, cut=None, mid=None))
    st.update(copy.deepcopy(kw))
    st["run"].setdefault("mid", None)
    return st


def _src(pos, flux, change="same", pl=None, qpl=None):
    return dict(pos=[list(p) for p in pos], flux=list(flux), change=change, pl=pl, qpl=qpl)


def _opaque_and_back(batch):
    """Gas turns opaque under an unchanged source list -- three rounds learnt along z, one needed -- and ionised again:
    nothing of the rounds launched on trust may stay in the grids, and sum_nbox is the oracle's."""
    pos, flux = [(1, 1, 1), (12, 8, 44), (6, 4, 22)], [2.0e7, 1.0e7, 3.0e7]
    up = dict(scale=1.0, how="upload", heat=True)
    steps = [_step(tables=up, route="set_step", src=_src(pos, flux, "grown"), batch=batch, gas=dict(kind="ionised", seed=11)),
             _step(src=_src(pos, flux), batch=batch, gas=dict(kind="ionised", seed=12), run=dict(kind="whole", dt=1.0e5)),
             _step(src=_src(pos, flux), batch=batch, gas=dict(kind="opaque", seed=13)),
             _step(src=_src(pos, flux), batch=batch, run=dict(kind="stepwise", dt=1.0e5, iters=1, slabs=3, cut=1000)),
             _step(src=_src(pos, flux), batch=batch, gas=dict(kind="ionised", seed=14)),
             _step(src=_src(pos, [1.0e4, 1.0e4, 1.0e4], "fluxes"), batch=batch, gas=dict(kind="opaque", seed=15),
                   run=dict(kind="whole", dt=1.0e4)),
             _step(src=_src(pos, flux, "fluxes"), batch=batch, gas=dict(kind="ionised", seed=16), run=dict(kind="whole", dt=1.0e5))]
    return dict(name=f"opaque-and-back-batch{batch}", why=_opaque_and_back.__doc__.split(":")[0], mesh=MESHES["deep"], multi=False,
                steps=steps)


def _geometry_three_ways():
    """Geometry disturbed from three directions: another redshift through scale_ndens, an open excursion with other cell
    sizes, periodic again -- the step that would read a shell-volume table left from before."""
    pos, flux = [(1, 1, 1), (24, 16, 20), (12, 8, 10)], [2.0e7, 5.0e6, 3.0e7]
    d0 = dict(seed=77, z0=9.0, spread=0.7, divs=[])
    d1 = dict(d0, divs=[((1.0 + 9.0) / (1.0 + 6.0)) ** 3])
    d2 = dict(d0, divs=d1["divs"] + [((1.0 + 6.0) / (1.0 + 7.5)) ** 3])
    up = dict(scale=1.0, how="upload", heat=True)
    mixed = lambda seed: dict(kind="mixed", seed=seed)
    steps = [_step(tables=up, route="set_step", dens=d0, src=_src(pos, flux, "grown"), batch=2, gas=mixed(1)),
             _step(zred=6.0, route="scale", dens=d1, src=_src(pos, flux), batch=2, gas=mixed(2),
                   run=dict(kind="stepwise", dt=1.0e5, iters=2, slabs=0, cut=None, mid=dict(how="scale", divisor=1.5))),
             _step(zred=6.0, aniso=True, route="set_step", dens=d1, src=_src(pos, flux), batch=5, gas=mixed(3),
                   excursion=dict(periodic=[0, 0, 0], zred=8.0, aniso=False)),
             _step(zred=6.0, aniso=True, dens=d1, src=_src(pos, flux), batch=5, run=dict(kind="whole", dt=3.0e4)),
             _step(zred=7.5, aniso=True, route="scale", dens=d2, src=_src(pos, flux), batch=1, gas=mixed(4),
                   excursion=dict(periodic=[1, 0, 1], zred=7.5, aniso=False)),
             _step(zred=9.0, dens=d2, src=_src(pos, flux), batch=1, run=dict(kind="stepwise", dt=1.0e5, iters=1, slabs=4, cut=None))]
    return dict(name="geometry-three-ways", why=_geometry_three_ways.__doc__.split(":")[0], mesh=MESHES["ragged"], multi=False,
                steps=steps)


def _tables_around_seds():
    """Tables disturbed around a SED change: heating with three SEDs, a shorter list without set_sources_sed, isothermal with
    scaled tables uploaded without heating tables, heating again with the shipped tables built on the device."""
    pos, flux = [(3, 2, 5), (12, 5, 8), (7, 3, 1), (1, 1, 1)], [2.0e6, 1.0e6, 3.0e6, 5.0e5]
    pl, qpl = [1.0e6, 0.0, 2.0e6, 5.0e5], [0.0, 1.0e6, 3.0e6, 5.0e5]
    up = dict(scale=1.0, how="upload", heat=True)
    mixed = lambda seed: dict(kind="mixed", seed=seed)
    steps = [_step(tables=up, route="set_step", iso=False, src=_src(pos, flux, "grown", pl, qpl), batch=2, gas=mixed(21)),
             _step(iso=False, src=_src(pos[:3], flux[:3], "shrunk"), batch=2),
             _step(tables=dict(scale=0.5, how="upload_noheat", heat=False), src=_src(pos[:3], flux[:3]), batch=4, gas=mixed(22)),
             _step(tables=dict(scale=0.5, how="keep", heat=False), src=_src(pos[:3], flux[:3], "same", pl[:3], None), batch=4),
             _step(tables=dict(scale=1.0, how="build", heat=True), iso=False, src=_src(pos[:3], flux[:3], "same", None, qpl[:3]), batch=1,
                   gas=mixed(23)),
             _step(iso=False, src=_src(pos[:3], flux[:3]), batch=1)]
    return dict(name="tables-around-seds", why=_tables_around_seds.__doc__.split(":")[0], mesh=MESHES["thin"], multi=True, steps=steps)


def _lists_and_modes():
    """Source lists and modes shuffled on the cube: a source moves onto the cell another held and inherits its count, twins,
    a permuted list, a flux of 0, LLS and clumping through all their kinds, tables without heating tables and a first heating
    step late in the context's life, whole calls around stepwise ones."""
    a, b, c, d = (1, 1, 1), (24, 24, 24), (12, 1, 24), (7, 13, 12)
    flux = [2.0e7, 1.0e7, 1.5e7, 3.0e7]
    up = dict(scale=1.0, how="upload", heat=True)
    grid = lambda kind, seed: dict(kind=kind, value=0.0 if kind != "scalar" else 3.0e16, seed=seed if kind == "grid" else 0)
    cl = lambda kind, value, seed: dict(kind=kind, value=value, seed=seed if kind == "grid" else 0)
    noheat = dict(scale=2.0, how="upload_noheat", heat=False)
    steps = [_step(tables=up, route="set_step", src=_src([a, b, c, d], flux, "grown"), batch=2, gas=dict(kind="ionised", seed=31),
                   run=dict(kind="whole", dt=1.0e5)),
             _step(src=_src([(5, 20, 9), a, c, d], flux, "moved"), batch=2, lls=grid("grid", 5), run=dict(kind="whole", dt=1.0e5)),
             _step(tables=noheat, src=_src([(5, 20, 9), (5, 20, 9), c, d], [1.0e5, 2.0e5, 1.0e5, 3.0e5], "twin"), batch=6,
                   lls=grid("scalar", 0), clump=cl("grid", 1.0, 6), gas=dict(kind="opaque", seed=32),
                   run=dict(kind="stepwise", dt=1.0e5, iters=2, slabs=2, cut=None, mid=dict(how="set_step", divisor=0.75))),
             _step(tables=dict(noheat, how="keep"), route="set_step", src=_src([d, c, (5, 20, 9), (5, 20, 9)], [3.0e5, 1.0e5, 2.0e5, 1.0e5], "permuted"),
                   batch=3, lls=grid("grid", 7), clump=cl("scalar", 1.75, 0), run=dict(kind="whole", dt=1.0e5)),
             _step(tables=up, iso=False, src=_src([d, c, (5, 20, 9), (5, 20, 9)], [3.0e6, 0.0, 2.0e6, 1.0e6], "zero"), batch=3,
                   clump=cl("scalar", 1.75, 0), gas=dict(kind="mixed", seed=33),
                   run=dict(kind="stepwise", dt=1.0e5, iters=1, slabs=0, cut=5000)),
             _step(iso=False, src=_src([d, c, (5, 20, 9)], [3.0e6, 0.0, 2.0e6], "shrunk"), batch=1, clump=cl("scalar", 1.75, 0),
                   run=dict(kind="whole", dt=3.0e4))]
    return dict(name="lists-and-modes", why=_lists_and_modes.__doc__.split(":")[0], mesh=MESHES["cube"], multi=False, steps=steps)


FIXED = [_opaque_and_back(1), _opaque_and_back(3), _geometry_three_ways(), _tables_around_seds(), _lists_and_modes()]


def case_list():
    drawn = [draw(np.random.default_rng([SEED, i])) for i in range(NCASES)]
    return FIXED + [dict(d, name=f"draw{i}-{d['name'][5:]}") for i, d in enumerate(drawn)]
