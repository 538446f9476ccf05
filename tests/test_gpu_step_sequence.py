"""One context through a sequence of changing time steps, every step against the oracle, which keeps nothing between steps.

The sequences are tests/step_sequence_cases.py's (C2R_SEQFUZZ_CASES / C2R_SEQFUZZ_SEED widen or move the list; its premises are
tests/test_step_sequence_host.py): gas that turns opaque and back under learnt sub-box counts, redshifts that reach the device
three ways and once between two outer iterations, iso <-> heating, LLS and clumping kinds, source lists that grow, shrink,
permute and share cells, SED sets that come and go, tables scaled, without heating tables and built on the device,
excursions to open boundaries with other cell sizes, whole evolve3d calls and stepwise ones.  One test id per sequence, one
context per id.

After every step everything run_oracle yields is compared bit for bit (np.array_equal); photon_loss[0] at rel_err <= 1e-12,
tests/test_gpu_fuzz.py's bound (its sum order differs); the rounds per source of the step's last pass with source_trace,
after stepwise steps and after whole calls alike.  No cell, array or step is left out.  On a mismatch the failing step is run once more on a context that has seen nothing
else, and the message says whether that one agrees with the oracle: if it does, the context's history is the cause, if not
the kernels are wrong for these inputs.  In the passing path the last step of every sequence is run on a fresh context as well
and compared with the long-lived one: all results, rounds and final boxes per source (block sizes and shell counts may differ
with what a context has learnt, and are not compared).
"""
import numpy as np
import pytest

import step_sequence_cases as sq
from conftest import rel_err

pytestmark = pytest.mark.gpu
SEQS = sq.case_list()


@pytest.fixture(scope="module")
def tables_for(pkg, orc):
    return sq.make_tables_for(pkg, orc)


def _rad_tables(pkg, gold, seq, spec, fresh=False):
    """The product's tables for a step's `tables`; a fresh context gets what the long-lived one holds after the step."""
    how = spec["how"]
    if fresh and how == "keep":
        how = "upload" if spec["heat"] else "upload_noheat"
    t = pkg.RadiationTables.load()
    if how == "build" and not (fresh and seq["multi"]):   # (the extra SEDs' tables stay as they were uploaded at the start)
        t.setup, t.build_on_device = dict(gold("sed_setup.npz")), True
        return t
    t.photo_thick = np.ascontiguousarray(t.photo_thick * spec["scale"])
    if how == "upload_noheat":
        t.heat_thick = t.heat_thin = None
    if seq["multi"]:
        t.add_sed_file(sq.EXTRA_SEDS)
    return t


def _objects(pkg, seq, step, start):
    hp = pkg.hostphys
    a = sq.inputs(hp, seq, step)
    xh, xhe, temp = start[:3]
    mat = pkg.Material(a["ndens"], xh, xhe, None if a["iso"] else temp, a["iso"], sq.TEMPER_VAL, a["clumping"], a["reccoef"],
                       clumping_grid=a["clumping_grid"], use_LLS=step["lls"]["kind"] != "off", coldensh_LLS=a["coldensh_lls"] or 0.0,
                       LLS_grid=a["lls_grid"])
    grid = pkg.GridProps(a["mesh"], a["dr"], a["vol"])
    cosmo = pkg.Cosmology(a["zred"], hp.H0, hp.Omega0)
    src = pkg.SourceProps(a["srcpos"], a["flux"], sq.S_STAR, NormFluxPL=a["pl"], pl_S_star=sq.PL_S_STAR, NormFluxQPL=a["qpl"],
                          qpl_S_star=sq.QPL_S_STAR)
    return a, mat, grid, cosmo, src


def _excursion(pkg, e, seq, prev, exc):
    """One pass and one global pass under other boundaries and cell sizes, on what the context holds; periodic again."""
    hp = pkg.hostphys
    dr, vol = sq.cell_sizes(hp, exc["zred"], exc["aniso"])
    mat = pkg.Material(None, None, None, None, prev["iso"], sq.TEMPER_VAL, float(prev["clump"]["value"]), hp.reccoef(sq.TEMPER_VAL))
    e.set_boundaries([bool(p) for p in exc["periodic"]])
    e.set_step_scalars(mat, pkg.GridProps(seq["mesh"], dr, vol), pkg.Cosmology(exc["zred"], hp.H0, hp.Omega0))
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    e.global_pass(prev["run"]["dt"] * sq.YEAR)
    e.set_boundaries(True)


def _drive(pkg, gold, e, seq, i, start, fresh=False):
    """Step i of `seq` on engine e: the calls its description names (fresh: everything is set, the state uploaded) and what
    came of it, a dict with run_step's keys."""
    step = seq["steps"][i]
    prev = seq["steps"][i - 1] if i and not fresh else None
    if prev is not None and step["excursion"]:
        _excursion(pkg, e, seq, prev, step["excursion"])
    if fresh or step["tables"]["how"] != "keep":
        e.set_tables(_rad_tables(pkg, gold, seq, step["tables"], fresh))
    a, mat, grid, cosmo, src = _objects(pkg, seq, step, start)
    if fresh or step["route"] == "set_step":
        e.set_step(mat, grid, cosmo)
    else:
        if step["route"] == "scale":
            e.scale_ndens(step["dens"]["divs"][-1])
        e.set_step_scalars(mat, grid, cosmo)
        if prev["lls"] != step["lls"]:                    # (they stay in force until the next call)
            e.set_lls(mat)
        if prev["clump"] != step["clump"]:
            e.set_clumping_grid(mat)
    e.set_sources(src)
    if fresh or step["gas"]["kind"] != "carried":
        e.upload_state(mat)
    e.set_batch(step["batch"])
    run, nsrc, nc = step["run"], len(step["src"]["flux"]), a["ncell"]
    dt = run["dt"] * sq.YEAR
    out = {}
    if run["kind"] == "whole":
        out["niter"], out["conv_flags"] = e.evolve3d(dt)
    else:
        e.begin_step()
        for it in range(run["iters"]):
            if it == 1 and run["mid"]:                   # the density divided once more, and no begin_step
                if run["mid"]["how"] == "scale":
                    e.scale_ndens(run["mid"]["divisor"])
                else:
                    mat.ndens = a["ndens"] / run["mid"]["divisor"]
                    e.set_step(mat, grid, cosmo)
            e.set_rates_to_zero()
            if nsrc and run["slabs"]:
                for sl in range(e.pass_sources_begin(1, 1, run["slabs"])):
                    e.pass_wait_slab(sl)
                e.pass_sources_end()
            elif nsrc:
                e.pass_sources(1, 1)
            if run["cut"] is None:
                e.global_pass(dt)
            else:
                e.global_pass_cells(dt, 0, run["cut"])
                e.global_pass_cells(dt, run["cut"], nc - run["cut"])
                e.global_pass_finish()
        e.end_step()
    rates, it = e.download_rates(), e.download_iter_state()
    # (a context that has never swept a source has no columns: without sources they are what an earlier pass left)
    cols = e.download_columns() if nsrc or not fresh else dict(coldensh_out=start[3], coldenshe_out=start[4])
    m2 = pkg.Material(None, None, None, None if a["iso"] else np.empty(3 * nc, dtype=np.float32), a["iso"])
    e.download_state(m2)
    out.update(sum_nbox=int(rates["sum_nbox"]), coldensh_out=cols["coldensh_out"], coldenshe_out=cols["coldenshe_out"],
               phih=rates["phih_grid"], phihe=rates["phihe_grid"], photon_loss=float(rates["photon_loss"][0]), xh=m2.xh, xhe=m2.xhe, **it)
    if not a["iso"]:
        out.update(phiheat=rates["phiheat"], temperature=m2.temperature_grid)
    out["trace"] = [e.source_trace(ns) for ns in range(1, nsrc + 1)]
    out["nbox"] = [t["nbox"] for t in out["trace"]]      # of the last pass: a whole call's last iteration
    return out


def _mismatches(got, exp):
    """The names in which a device result differs from run_step's (everything it yields), with the count of differing cells.
    step_sequence_cases.differs is the same comparison between two oracle results: the host test's premise rests on it."""
    bad = []
    for k in sq.COUNTS:                                   # (the rounds per source on whole calls as well: more than asked)
        if k in exp and got.get(k) != exp[k]:
            bad.append(f"{k}: {got.get(k)} != {exp[k]}")
    for k in sq.COMPARED:
        if k in exp and not np.array_equal(got[k], exp[k]):
            bad.append(f"{k}: {int((got[k] != exp[k]).sum())} of {exp[k].size} differ")
    err = float(rel_err(got["photon_loss"], exp["photon_loss"]))
    if not err <= sq.LOSS_BOUND:
        bad.append(f"photon_loss: {got['photon_loss']!r} != {exp['photon_loss']!r} (rel_err {err:.3e})")
    return bad


def _fresh(pkg, gold, seq, i, start):
    e = pkg.HipEngine(seq["mesh"], 0)
    try:
        return _drive(pkg, gold, e, seq, i, start, fresh=True)
    finally:
        e.close()


@pytest.mark.parametrize("seq", SEQS, ids=[s["name"] for s in SEQS])
def test_one_context_through_the_sequence(pkg, orc, tables_for, gold, seq):
    expected = sq.run_oracle(orc, tables_for, seq, pkg.hostphys)
    e = pkg.HipEngine(seq["mesh"], 0)
    try:
        for i, (step, exp) in enumerate(zip(seq["steps"], expected)):
            start = sq.start_state(seq, i, expected[i - 1] if i else None)
            changed = ["first step"]
            if i:
                changed = sq.changed_items(seq["steps"][i - 1], step) + (["excursion"] if step["excursion"] else [])
            print(f"{seq['name']} step {i}: {step['run']['kind']}, changed {changed}")
            got = _drive(pkg, gold, e, seq, i, start)
            bad = _mismatches(got, exp)
            if bad:
                alone = _mismatches(_fresh(pkg, gold, seq, i, start), exp)
                verdict = ("a fresh context agrees with the oracle: the context's history is the cause" if not alone else
                           f"a fresh context differs from the oracle too: the kernels are wrong for these inputs ({alone})")
                raise AssertionError(f"{seq['name']} ({seq['why']}), step {i}, changed since the step before: {changed}\n  " +
                                     "\n  ".join(bad) + f"\n  {verdict}\n  step: {step}")
        # the last step on a context that has seen nothing else
        alone = _fresh(pkg, gold, seq, i, start)
        tag = (seq["name"], i, "long-lived context against a fresh one")
        for k, v in got.items():
            if k == "trace":
                for ns, (a, b) in enumerate(zip(v, alone[k]), 1):
                    for f in ("nbox", "reach_l", "reach_r", "box_lo", "box_hi"):
                        assert a[f] == b[f], (tag, ns, f, a, b)
            elif k == "photon_loss":                    # (its sum order follows the column blocks, which follow what was learnt)
                assert rel_err(v, alone[k]) <= 1e-12, (tag, k, v, alone[k])
            elif isinstance(v, np.ndarray):
                assert np.array_equal(v, alone[k]), (tag, k)
            else:
                assert v == alone[k], (tag, k, v, alone[k])
    finally:
        e.close()
