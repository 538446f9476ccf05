"""The ladder of sub-step ceilings of the heating global pass, as far as a CPU can see it (tests/test_gpu_chem_ladder.py is the
device's side):

  a. thermal()'s `work` / `budget` arguments (csrc/c2ray_device.hpp), which carry the whole scheme, compiled for the host:
     against the unbudgeted call and the oracle's count of trips through the loop;
  b. the shared cases (tests/chem_ladder_cases.py) cover what the GPU tests rely on, by the oracle's own counts -- conditions on
     the INPUTS, so that an edit of the cases cannot hollow the GPU tests out in silence;
  c. the model of the ladder (tests/chem_ladder_reference.py) against launches written down by hand.
"""
import ctypes as C

import numpy as np
import pytest

import chem_ladder_cases as cc
import chem_ladder_reference as lr

dp = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(dp)


# -- a. thermal()'s budget contract --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hh(harness, pkg):
    """The host build of the device functions with the shipped tables (as tests/test_device_functions_host.py sets them)."""
    t = pkg.RadiationTables.load()
    keep = [t.fvec[k] for k in pkg.evolve.FVEC_ORDER]
    fv = (dp * 12)(*[_p(a) for a in keep])
    harness.hh_set_tables(_p(t.photo_thick), _p(t.photo_thin), _p(t.heat_thick), _p(t.heat_thin), _p(t.sigma_HI),
                          _p(t.sigma_HeI), _p(t.sigma_HeII), fv, C.c_int(t.bb_upper), _p(t.cool),
                          C.c_double(t.cool_mintemp), C.c_double(t.cool_dtemp))
    harness._keep = (t, keep)
    return harness


def _directed_vectors(orc, otables, hp):
    """thermal() calls cut from the directed case: the calls its cells make in their first pass at either time step, with
    their arguments as do_chemistry passes them (orc.cell_thermal_calls).  Kept are calls that skip the sub-cycle, that are
    put back on the minitemp floor, that leave by the 10 000 cap, and ordinary ones: rows (dt, tend, de, nd, heat, ion15)."""
    case = cc.directed(hp, "ragged")
    picked = {"cold": [], "floor": [], "cap": [], "plain": []}
    for dt_years in cc.DTS:
        st, s = cc.oracle_objects(orc, hp, case)
        for q in range(case["ncell"]):
            rows, _ = orc.cell_thermal_calls(otables, st, s, dt_years * cc.YEAR, q, cap=8)
            for r in rows:
                kinds = [k for k, flag in zip(("floor", "cap", "cold"), r[21:24]) if flag] or ["plain"]   # (floor and cap may both hold)
                if any(len(picked[k]) < 5 for k in kinds):
                    row = (r[0], r[1], r[2], r[3], r[4], np.ascontiguousarray(r[5:20]))
                    for k in kinds:
                        picked[k].append(row)
    for kind, rows in picked.items():
        assert len(rows) >= 3, (kind, len(rows))         # the case does hold such calls
    return list({id(r): r for rows in picked.values() for r in rows}.values())


def test_thermal_budget_contract(hh, pkg, orc, otables, gold):
    """thermal(cd, dt, tend, tavg, de, nd, ion, heat, &work, budget) over the 200 reference vectors and over calls cut from the
    directed case (cold entry, floor, cap).  Budget 0: never gives up, outputs bit-equal to the call without the arguments, work
    grows by exactly the oracle's trips.  Budgets trips - 1, trips, trips + 1 with starting counts 0 and 7: gives up iff
    start + trips > budget (and the call has a sub-cycle at all); if not, outputs bit-equal to the unbudgeted call and work =
    start + trips; if so, work is one past the larger of budget and start (the count that passed the ceiling: budget + 1
    whenever the caller came in under its ceiling, as k_chemistry does).  A call that skips the sub-cycle leaves work alone and
    never gives up."""
    hp = pkg.hostphys
    c = gold("consts.npz")["consts"]
    vectors = [(row[0], row[1], row[2], row[3], row[4], np.ascontiguousarray(row[6:21]), row[5], c[42], c[43])
               for row in gold("funcvec.npz")["thermal"].reshape(-1, 25)]
    vectors += [r + (cc.ZRED, hp.H0, hp.Omega0) for r in _directed_vectors(orc, otables, hp)]

    def call(v, start=None, budget=0):
        dt, tend, de, nd, heat, ion, zred, H0, Om = v
        te, ta = C.c_double(tend), C.c_double(-1.0)
        args = [C.c_double(dt), C.byref(te), C.byref(ta), C.c_double(de), C.c_double(nd), _p(ion), C.c_double(heat),
                C.c_double(zred), C.c_double(H0), C.c_double(Om)]
        if start is None:
            hh.hh_thermal(*args)
            return te.value, ta.value
        work = C.c_int(start)
        flag = hh.hh_thermal_budget(*args, C.byref(work), C.c_int(budget))
        return bool(flag), te.value, ta.value, work.value

    seen = {"skip": 0, "gave_up": 0, "finished_under_budget": 0}
    for n, v in enumerate(vectors):
        plain = call(v)
        te, ta, trips, _ = orc.thermal_work(otables, v[0], v[1], -1.0, v[2], v[3], v[5], v[4], v[6], v[7], v[8])
        assert plain == (te, ta), n
        for start in (0, 7, 100000):
            assert call(v, start, 0) == (False,) + plain + (start + trips,), (n, start)
        budgets = (1, 5) if trips == 0 else [b for b in (trips - 1, trips, trips + 1) if b > 0]
        for budget in budgets:
            for start in (0, 7):
                flag, te_b, ta_b, work = call(v, start, budget)
                assert flag == (trips > 0 and start + trips > budget), (n, trips, start, budget)
                if flag:
                    assert work == max(start, budget) + 1, (n, trips, start, budget, work)
                    seen["gave_up"] += 1
                else:
                    assert (te_b, ta_b) == plain and work == start + trips, (n, trips, start, budget, work)
                    seen["skip" if trips == 0 else "finished_under_budget"] += 1
    assert all(seen.values()), seen


# -- b. the cases cover what they claim ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def directed_runs(pkg, orc, otables):
    hp = pkg.hostphys
    return {(name, dt): cc.run_directed(orc, otables, hp, cc.directed(hp, name), dt) for name in cc.MESHES for dt in cc.DTS}


@pytest.mark.parametrize("dt", cc.DTS)
@pytest.mark.parametrize("name", sorted(cc.MESHES))
def test_directed_case_walks_the_whole_ladder(directed_runs, name, dt):
    """With residency 0 every pass of the directed case makes all five launches (16, 64, 256, 1 024, none), each ceiling defers
    at least one cell and lets at least one finish; over the passes each of the four events occurs, the last cell of the mesh
    needs more than 1 024 sub-steps at least once, some cell needs none, and no cell passes MAX_CHAIN."""
    runs = directed_runs[(name, dt)]
    ncell = len(runs[0]["W"])
    events = {k: 0 for k in runs[0]["events"]}
    for p, ((launches, first), r) in enumerate(zip(lr.chain([r["W"] for r in runs], resident=0), runs)):
        print(f"{name} dt={dt:g} yr pass {p}: launches {launches}, longest chain {int(r['W'].max())}, events {r['events']}")
        assert first == 16 and [c for c, _ in launches] == [16, 64, 256, 1024, None], (p, first, launches)
        left = [ncell] + [n for _, n in launches]
        assert all(a > b for a, b in zip(left, left[1:])) and left[-1] == 0, (p, launches)   # some finish under each
        assert all(n > 0 for n in left[:5]), (p, launches)                                       # some are deferred by each
        assert int(r["W"].max()) <= cc.MAX_CHAIN, (p, int(r["W"].max()))
        for k in events:
            events[k] += r["events"][k]
    assert all(v > 0 for v in events.values()), events
    assert any(r["W"][-1] > 1024 for r in runs), [int(r["W"][-1]) for r in runs]
    assert any((r["W"] == 0).any() for r in runs)
    # with the default residency the same passes are "first launch, then one unbounded launch"
    for launches, first in lr.chain([r["W"] for r in runs]):
        assert [c for c, _ in launches] == [16, None], launches


def test_directed_case_with_clumping_stays_short(pkg, orc, otables):
    hp = pkg.hostphys
    r = cc.run_directed(orc, otables, hp, cc.directed(hp, "ragged", clump=True), cc.DTS[0], 1)[0]
    launches, _ = lr.ladder(r["W"], 16, 0)
    print(f"clumping: launches {launches}, longest chain {int(r['W'].max())}")
    assert len(launches) == 5 and int(r["W"].max()) <= cc.MAX_CHAIN


def test_raytraced_sequence_moves_the_first_ceiling(pkg, orc, otables):
    """Over its eight outer iterations the ray-traced case starts its ladder at 16, at 64 and at 256, each at least once."""
    hp = pkg.hostphys
    runs = cc.run_raytraced(orc, otables, hp, cc.raytraced(hp))
    chained = lr.chain([r["W"] for r in runs], resident=0)
    for p, ((launches, first), r) in enumerate(zip(chained, runs)):
        print(f"ray-traced pass {p}: first ceiling {first}, launches {launches}, longest chain {int(r['W'].max())}")
        assert int(r["W"].max()) <= cc.MAX_CHAIN
    assert {16, 64, 256} <= {first for _, first in chained}


# -- c. the model against hand-made counts -------------------------------------------------------------------------------------
def test_model_on_hand_made_counts():
    N = 10
    # nothing to do anywhere: one launch, nothing deferred, and (all cells in bucket 0) the ladder stays at 16
    assert lr.ladder([0] * N, 16, 0) == ([(16, 0)], 16)
    # exactly 16: finishes under the ceiling 16 (16 > 16 is false), one launch -- but counts in bucket 5, [16, 32), above
    # the rung 16, so the next pass starts at 64
    assert lr.bucket(15) == 4 and lr.bucket(16) == 5
    assert lr.ladder([16] * N, 16, 0) == ([(16, 0)], 64)
    # 17: deferred under 16, finishes under 64
    assert lr.ladder([17] * N, 16, 0) == ([(16, N), (64, 0)], 64)
    # 64: finishes under 64, counts in bucket 7, [64, 128): next first ceiling 256
    assert lr.ladder([64] * N, 16, 0) == ([(16, N), (64, 0)], 256)
    # 1 024: walks 16, 64, 256 and finishes under 1 024; bucket 11 lies above every rung, the next pass starts at the top one
    assert lr.ladder([1024] * N, 16, 0) == ([(16, N), (64, N), (256, N), (1024, 0)], 1024)
    # 1 025: deferred by all four ceilings, finishes in the unbounded launch
    assert lr.ladder([1025] * N, 16, 0) == ([(16, N), (64, N), (256, N), (1024, N), (None, 0)], 1024)
    # one cell above every rung among nine that need nothing: it alone walks the ladder, the next pass starts at 16
    assert lr.ladder([0] * 9 + [5000], 16, 0) == ([(16, 1), (64, 1), (256, 1), (1024, 1), (None, 0)], 16)
    # residency: ten deferred cells fit a device that holds ten -- the first follow-up launch is unbounded and the last ...
    assert lr.ladder([1025] * N, 16, N) == ([(16, N), (None, 0)], 1024)
    # ... but not one that holds nine
    assert lr.ladder([1025] * N, 16, N - 1) == ([(16, N), (64, N), (256, N), (1024, N), (None, 0)], 1024)
    # a pass that starts higher: from 256 the ceilings are 256, 1 024, none; from 1 024 the first follow-up is unbounded
    assert lr.ladder([17] * N, 256, 0) == ([(256, 0)], 64)
    assert lr.ladder([1025] * N, 256, 0) == ([(256, N), (1024, N), (None, 0)], 1024)
    assert lr.ladder([1025] * N, 1024, 0) == ([(1024, N), (None, 0)], 1024)
    # half of the cells below 16 is enough for the rung 16, one fewer is not
    assert lr.ladder([15] * 5 + [100] * 5, 16, 0)[1] == 16 and lr.ladder([15] * 4 + [100] * 6, 16, 0)[1] == 256
    # the chain hands each pass's next first ceiling to the pass after it
    assert [first for _, first in lr.chain([[16] * N, [64] * N, [0] * N, [0] * N], resident=0)] == [16, 64, 256, 16]
    assert lr.next_first([0] * lr.NBUCKETS) == 16
