"""tests/step_sequence_cases.py held to account on the CPU with the oracle alone, so that a pass of
tests/test_gpu_step_sequence.py means something:

1. The list is seeded, plain and pinned (a SHA-256 over the default list's repr), and every sequence keeps the rules of
   step_sequence_cases.check.
2. Every change is visible: for every step and every item that changed against the step before -- cell sizes, density, table,
   source list or fluxes, SED set, LLS, clumping, iso / heating, gas, the cell sizes of an excursion, and the density divided
   between two outer iterations -- the oracle run once more with that one item put back to its earlier value differs from the
   expected result by the GPU test's own comparison (step_sequence_cases.differs: the same counts, rounds per source on
   every step, arrays bit for bit, photon_loss beyond its 1e-12).  There is no list of exemptions: a step on which a stale
   value would go unnoticed fails here, and the case is what changes.
5. The two opaque-and-back sequences themselves go three rounds, one, three.
3. Coverage is a condition: the tallies are printed and asserted over the default list.
4. Every whole evolve3d call converges within 40 iterations, and the do_source loop that run_step uses for it is
   orc.evolve3d: iterations, non-converged counts and end state, bit for bit.
"""
import collections
import copy
import hashlib

import numpy as np
import pytest

import step_sequence_cases as sq

SEQS = sq.case_list()
DIGEST = "4655fd4ac0525b344a55411d3ffc28a1369eccd3344be077c29ef73a4c1b1e6a"


@pytest.fixture(scope="module")
def tables_for(pkg, orc):
    return sq.make_tables_for(pkg, orc)


@pytest.fixture(scope="module")
def expected(pkg, orc, tables_for):
    return [sq.run_oracle(orc, tables_for, seq, pkg.hostphys) for seq in SEQS]


def test_the_list_is_seeded_plain_and_pinned():
    assert [repr(s) for s in sq.case_list()] == [repr(s) for s in SEQS]
    assert len(SEQS) == len(sq.FIXED) + sq.NCASES and len({s["name"] for s in SEQS}) == len(SEQS)

    def plain(x):
        if isinstance(x, (list, tuple)):
            return all(plain(y) for y in x)
        if isinstance(x, dict):
            return all(isinstance(k, str) and plain(v) for k, v in x.items())
        return x is None or type(x) in (bool, int, float, str)
    assert all(plain(s) for s in SEQS)
    for seq in SEQS:
        sq.check(seq)
        assert max(seq["mesh"][:2]) <= 24 and (seq["mesh"][2] <= 24 or seq["mesh"] == sq.MESHES["deep"]), seq["name"]
    assert all(s["why"] and s["why"] != "drawn" for s in sq.FIXED)
    if (sq.NCASES, sq.SEED) == (sq.DEFAULT_CASES, sq.DEFAULT_SEED):
        assert hashlib.sha256(repr(SEQS).encode()).hexdigest() == DIGEST


def _put_back_result(pkg, orc, tables_for, seq, i, exp, item):
    """The oracle's result of step i with `item` as the step before had it, and whether conv_flags can be compared."""
    hp = pkg.hostphys
    steps = seq["steps"]
    prev, step = steps[i - 1], steps[i]
    nc = int(np.prod(seq["mesh"]))
    alt = sq.put_back(prev, step, item)
    start = sq.start_state(seq, i, exp[i - 1])
    if item == "gas":                                    # the upload lost: what the step before left
        temp = exp[i - 1].get("temperature")
        start = (exp[i - 1]["xh"], exp[i - 1]["xhe"], temp if temp is not None else start[2]) + tuple(start[3:])
    if not alt["iso"] and start[2] is None:              # heating put back on an isothermal step: it needs some temperature
        temp = exp[i - 1].get("temperature")
        temp = temp if temp is not None else np.full(3 * nc, 1.0e4, dtype=np.float32)
        start = (start[0], start[1], temp) + tuple(start[3:])
    flags = True
    if alt["run"]["kind"] == "whole" and not sq.whole_ok(seq["mesh"], len(alt["src"]["flux"])):
        alt["run"] = dict(kind="stepwise", dt=alt["run"]["dt"], iters=exp[i]["niter"], slabs=0, cut=None)
        flags = False
    return sq.run_step(orc, tables_for(alt["tables"]["scale"], seq["multi"]), hp, seq, alt, start), flags


def test_every_change_is_visible(pkg, orc, tables_for, expected):
    holes, checked = [], collections.Counter()
    for seq, exp in zip(SEQS, expected):
        for i in range(1, len(seq["steps"])):
            items = sq.changed_items(seq["steps"][i - 1], seq["steps"][i])
            if seq["steps"][i]["excursion"]:
                items.append("excursion")
            for item in items:
                got, flags = _put_back_result(pkg, orc, tables_for, seq, i, exp, item)
                checked[item] += 1
                if not sq.differs(got, exp[i], flags):
                    holes.append((seq["name"], i, item))
            mid = seq["steps"][i]["run"].get("mid")
            if mid:                                      # the density divided between two iterations: without it, other results
                alt = copy.deepcopy(seq["steps"][i])
                alt["run"]["mid"] = None
                T = tables_for(alt["tables"]["scale"], seq["multi"])
                got = sq.run_step(orc, T, pkg.hostphys, seq, alt, sq.start_state(seq, i, exp[i - 1]))
                checked["mid " + mid["how"]] += 1
                if not sq.differs(got, exp[i]):
                    holes.append((seq["name"], i, "mid"))
    print("put-back runs per item:", dict(checked))
    assert not holes, holes
    assert all(checked[k] >= 2 for k in sq.ITEMS + ("excursion",)) and checked["mid scale"] and checked["mid set_step"], checked


def _learnt(prev_step, prev_result):
    """Per cell, what set_sources_one carries: the largest count of the sources that held it in the last pass."""
    known = {}
    for p, nb in zip(prev_step["src"]["pos"], prev_result["nbox"]):
        known[tuple(p)] = max(known.get(tuple(p), 0), nb)
    return known


def test_coverage(expected):
    t = collections.Counter()
    for seq, exp in zip(SEQS, expected):
        steps = seq["steps"]
        t["multi sequence"] += seq["multi"]
        kinds = [s["run"]["kind"] for s in steps]
        t["both kinds of run in one sequence"] += len(set(kinds)) == 2
        t["whole call before and after a stepwise step"] += any(kinds[a] == "whole" and kinds[b] == "stepwise" and kinds[c] == "whole"
                                                              for a in range(len(kinds)) for b in range(a + 1, len(kinds))
                                                              for c in range(b + 1, len(kinds)))
        for i, (st, r) in enumerate(zip(steps, exp)):
            n = len(st["src"]["flux"])
            run = st["run"]
            t["run " + run["kind"]] += 1
            if run["kind"] == "stepwise":
                t[f"stepwise {run['iters']} iterations"] += 1
                t["pass slab-wise"] += run["slabs"] > 0
                t["global pass in pieces"] += run["cut"] is not None
            t["batch 1"] += st["batch"] == 1 and n > 1
            t["batch < nsrc"] += 1 < st["batch"] < n
            t["batch > nsrc"] += st["batch"] > n > 0
            t["nbox >= 3"] += any(nb >= 3 for rd in r["rounds"] for nb in rd)
            t["aniso"] += st["aniso"]
            t["flux 0"] += any(f == 0.0 for f in st["src"]["flux"])
            t["two sources in one cell"] += len({tuple(p) for p in st["src"]["pos"]}) < n
            t["sed one"] += (st["src"]["pl"] is None) != (st["src"]["qpl"] is None)
            t["sed both"] += st["src"]["pl"] is not None and st["src"]["qpl"] is not None
            if i == 0:
                continue
            pv, pr = steps[i - 1], exp[i - 1]
            t["source change " + st["src"]["change"]] += 1
            t["excursion"] += bool(st["excursion"])
            t["gas carried"] += st["gas"]["kind"] == "carried"
            t["gas uploaded"] += st["gas"]["kind"] != "carried"
            t["gas to opaque"] += st["gas"]["kind"] == "opaque"
            t["gas to ionised"] += st["gas"]["kind"] == "ionised"
            t["carried into a whole call"] += st["gas"]["kind"] == "carried" and run["kind"] == "whole"
            t["iso -> heating"] += pv["iso"] and not st["iso"]
            t["heating -> iso"] += st["iso"] and not pv["iso"]
            t["first heating step late"] += not st["iso"] and all(s["iso"] for s in steps[:i])
            t["clump -> " + st["clump"]["kind"]] += pv["clump"]["kind"] != st["clump"]["kind"]
            t["lls -> " + st["lls"]["kind"]] += pv["lls"] != st["lls"]
            new_z = pv["zred"] != st["zred"]
            t["density by " + st["route"]] += new_z or st["route"] == "scale"
            t["redshift unchanged"] += not new_z
            t["aniso toggled"] += pv["aniso"] != st["aniso"]
            t["tables " + st["tables"]["how"]] += 1
            t["tables scaled"] += st["tables"]["scale"] != 1.0 and pv["tables"]["scale"] == 1.0
            t["tables back"] += st["tables"]["scale"] == 1.0 and pv["tables"]["scale"] != 1.0
            t["heating tables again"] += st["tables"]["heat"] and not pv["tables"]["heat"]
            t["seds omitted after being on"] += n > 0 and st["src"]["pl"] is None and st["src"]["qpl"] is None and \
                (pv["src"]["pl"] is not None or pv["src"]["qpl"] is not None)
            if not st["excursion"]:                      # (set_boundaries forgets the counts)
                known = _learnt(pv, pr)
                for p, nb in zip(st["src"]["pos"], r["rounds"][0] if r["rounds"] else []):
                    k = known.get(tuple(p), 0)
                    t["nbox below the learnt count"] += 0 < nb < k
                    t["nbox above the learnt count"] += nb > k > 0
                if st["src"]["change"] == "moved":
                    t["new source on a held cell"] += any(tuple(p) in known and (j >= len(pv["src"]["pos"]) or pv["src"]["pos"][j] != p)
                                                          for j, p in enumerate(st["src"]["pos"]))
    print("coverage:", dict(sorted(t.items())))
    if (sq.NCASES, sq.SEED) != (sq.DEFAULT_CASES, sq.DEFAULT_SEED):
        return
    twice = ["gas carried", "gas uploaded", "gas to opaque", "gas to ionised", "density by set_step", "density by scale",
             "density by scalars", "aniso toggled", "iso -> heating", "heating -> iso", "clump -> grid", "clump -> scalar",
             "lls -> off", "lls -> scalar", "lls -> grid", "batch 1", "batch < nsrc", "batch > nsrc", "multi sequence", "sed one",
             "sed both", "seds omitted after being on", "tables keep", "tables upload", "tables upload_noheat", "tables build",
             "tables scaled", "tables back", "heating tables again", "excursion", "run whole", "run stepwise",
             "stepwise 1 iterations", "stepwise 2 iterations", "pass slab-wise", "global pass in pieces",
             "both kinds of run in one sequence"] + ["source change " + c for c in sq.SOURCE_CHANGES]
    once = ["nbox below the learnt count", "nbox above the learnt count", "nbox >= 3", "new source on a held cell",
            "first heating step late", "carried into a whole call", "whole call before and after a stepwise step", "flux 0",
            "two sources in one cell", "aniso"]
    short = [k for k in twice if t[k] < 2] + [k for k in once if t[k] < 1]
    assert not short, short


def test_opaque_and_back_goes_three_one_three(expected):
    """What the two opaque-and-back sequences are for, held on themselves and not on the list's tallies: every source learns
    three rounds in ionised gas; in the first pass after the gas turned opaque every source needs fewer than it learnt and
    two of the three need one (the corner source runs a second); all need three again once the gas is back.  The carried step in between still runs below the learnt count."""
    seen = 0
    for seq, exp in zip(SEQS, expected):
        if not seq["name"].startswith("opaque-and-back"):
            continue
        seen += 1
        kinds = [st["gas"]["kind"] for st in seq["steps"]]
        assert kinds[:5] == ["ionised", "ionised", "opaque", "carried", "ionised"], (seq["name"], kinds)
        assert len({(tuple(map(tuple, st["src"]["pos"])), st["batch"]) for st in seq["steps"]}) == 1, seq["name"]
        rounds = [[list(rd) for rd in r["rounds"]] for r in exp]
        print(seq["name"], "rounds per step, iteration and source:", rounds)
        n = len(seq["steps"][0]["src"]["flux"])
        assert rounds[1][-1] == [3] * n, (seq["name"], "learnt", rounds[1])
        assert max(rounds[2][0]) < 3 and rounds[2][0].count(1) >= 2, (seq["name"], "needed", rounds[2])
        assert all(nb < 3 for rd in rounds[2] + rounds[3] for nb in rd), (seq["name"], "still opaque", rounds[2], rounds[3])
        assert rounds[4][0] == [3] * n, (seq["name"], "back", rounds[4])
        assert all(r["sum_nbox"] == sum(r["rounds"][-1]) for r in exp), seq["name"]
    assert seen == 2


def test_whole_calls_converge_and_the_loop_is_the_oracles(pkg, orc, tables_for, expected):
    hp = pkg.hostphys
    nwhole, worst = 0, 0
    for seq, exp in zip(SEQS, expected):
        for i, (st, r) in enumerate(zip(seq["steps"], exp)):
            if st["run"]["kind"] != "whole":
                continue
            nwhole += 1
            worst = max(worst, r["niter"])
            tag = (seq["name"], i, r["niter"], r["conv_flags"][-3:])
            criterion = min(int(sq.CONVERGENCE_FRACTION * np.prod(seq["mesh"])), len(st["src"]["flux"]))
            assert 2 <= r["niter"] <= 40 and r["conv_flags"][-1] < criterion, tag
            a = sq.inputs(hp, seq, st)
            step = orc.Step(a["mesh"], a["dr"], a["vol"], a["zred"], hp.H0, hp.Omega0, a["iso"], sq.TEMPER_VAL, a["clumping"], a["srcpos"],
                            a["flux"], sq.S_STAR, a["ndens"], a["reccoef"], normflux_pl=a["pl"], normflux_qpl=a["qpl"],
                            pl_s_star=sq.PL_S_STAR, qpl_s_star=sq.QPL_S_STAR, coldensh_lls=a["coldensh_lls"], lls_grid=a["lls_grid"],
                            clumping_grid=a["clumping_grid"])
            xh, xhe, temp = sq.start_state(seq, i, exp[i - 1] if i else None)[:3]
            s = orc.State(step, xh, xhe, None if a["iso"] else temp)
            T = tables_for(st["tables"]["scale"], seq["multi"])
            assert orc.evolve3d(T, step, s, st["run"]["dt"] * sq.YEAR) == r["niter"] and s.conv_flags == r["conv_flags"], tag
            assert int(s.c.sum_nbox) == r["sum_nbox"], tag
            for k in ("xh", "xhe", "phih", "phihe", "xh_av", "xhe_av", "coldensh_out", "coldenshe_out"):
                assert np.array_equal(getattr(s, k), r[k]), (k, tag)
            if not a["iso"]:
                assert np.array_equal(s.temperature, r["temperature"]) and np.array_equal(s.phiheat, r["phiheat"]), tag
    print(f"{nwhole} whole calls, at most {worst} iterations")
    assert nwhole >= 2 or sq.NCASES < sq.DEFAULT_CASES
