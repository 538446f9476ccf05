"""The heating global pass walks its whole ladder of sub-step ceilings on small meshes, bit for bit against the oracle.

c2r_global_pass_finish ends the ladder as soon as the deferred cells fit the device (131 072), so on the meshes of the other
tests a heating pass is "first launch, then one unbounded launch".  C2R_CHEM_RESIDENT_CELLS=0 takes that cut away: here the
list-driven launches with a ceiling, re-deferral out of a list, the second deferred list and its counter, the rungs at 256
and 1 024 and the stop at the last ceiling all run, on 192 to 256 cells.

Every test runs once with C2R_CHEM_RESIDENT_CELLS=0 and once with it unset.  After every pass the four arrays of
download_iter_state, all three planes of the temperature grid and the non-converged count equal the oracle's (np.array_equal),
and timing().chem_launches equals the launch count of the model of the ladder (tests/chem_ladder_reference.py) for that
residency, fed with the oracle's sub-steps per cell and chained from pass to pass with its own next first ceiling, from 16 on
a fresh context.  The cases are tests/chem_ladder_cases.py's; that they reach every rung and stay short (no cell beyond 60 000
sub-steps in a pass) is tests/test_chem_ladder_host.py's business.
"""
import ctypes as C

import numpy as np
import pytest

import chem_ladder_cases as cc
import chem_ladder_reference as lr

pytestmark = pytest.mark.gpu
RESIDENCIES = (("0", 0), (None, lr.DEFAULT_RESIDENT))      # (the environment's value, what the model takes)
ITER = ("xh_av", "xhe_av", "xh_intermed", "xhe_intermed")
ABU_HE = float(np.float32(0.074))


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


@pytest.fixture(scope="module")
def oracle_runs(pkg, orc, otables):
    """The oracle's passes per case, computed once and left alone: get(name, dt, clump) for the directed case, get("ray")."""
    hp, cache = pkg.hostphys, {}

    def get(name, dt=None, clump=False, npass=cc.NPASS):
        key = (name, dt, clump, npass)
        if key not in cache:
            if name == "ray":
                case = cc.raytraced(hp)
                cache[key] = (case, cc.run_raytraced(orc, otables, hp, case))
            else:
                case = cc.directed(hp, name, clump=clump)
                cache[key] = (case, cc.run_directed(orc, otables, hp, case, dt, npass))
        return cache[key]
    return get


def _engine(pkg, tables, case, monkeypatch, env):
    """A fresh context under the residency setting `env`, the case's state uploaded, the step begun, its rates (if it brings
    any) in place."""
    if env is None:
        monkeypatch.delenv("C2R_CHEM_RESIDENT_CELLS", raising=False)
    else:
        monkeypatch.setenv("C2R_CHEM_RESIDENT_CELLS", env)
    hp = pkg.hostphys
    mat = pkg.Material(case["ndens"], case["xh"], case["xhe"], case["temp"], False, cc.TEMPER_VAL, case["clumping"], case["reccoef"],
                       clumping_grid=case["clumping_grid"])
    e = pkg.HipEngine(case["mesh"], 0)
    try:
        e.set_tables(tables)
        e.set_step(mat, pkg.GridProps(case["mesh"], case["dr"], case["vol"]), pkg.Cosmology(case["zred"], hp.H0, hp.Omega0))
        e.set_sources(pkg.SourceProps(case["srcpos"], case["flux"], case["s_star"]))
        e.upload_state(mat)
        e.begin_step()
        if "phih" in case:
            e.upload_rates(case["phih"], case["phihe"], case["phiheat"])
    except Exception:
        e.close()
        raise
    return e


def _temperature(pkg, e, ncell):
    m = pkg.Material(None, None, None, np.empty(3 * ncell, dtype=np.float32), False)
    e.download_state(m)
    return m.temperature_grid


def _check_pass(pkg, e, exp, conv, launches, extra, tag):
    """One pass's results against the oracle's `exp`, and its launches against the model's."""
    bad = []
    it = e.download_iter_state()
    for k in ITER:
        if not np.array_equal(it[k], exp[k]):
            bad.append(f"{k}: {int((it[k] != exp[k]).sum())} of {exp[k].size} differ, cells {np.nonzero(it[k] != exp[k])[0][:8] % len(exp['W'])}")
    temp = _temperature(pkg, e, len(exp["W"]))
    if not np.array_equal(temp, exp["temperature"]):
        bad.append(f"temperature: {int((temp != exp['temperature']).sum())} of {temp.size} differ")
    if conv != exp["conv"]:
        bad.append(f"non-converged count {conv} != {exp['conv']}")
    got = e.timing().chem_launches
    print(f"{tag}: launches {launches}, {got} on the device (+{extra} first-launch pieces), longest chain {int(exp['W'].max())}")
    if got != len(launches) + extra:
        bad.append(f"chem_launches {got} != {len(launches)} + {extra} (model: {launches})")
    assert not bad, f"{tag}: " + "; ".join(bad)
    return it


def _total_rates(case, it, rc, dt):
    """photonstatistics' total_rates on the averaged fractions, as tests/test_gpu_parity.py computes it on the host."""
    n, nd, vol, clump = case["ncell"], case["ndens"], case["vol"], case["clumping"]
    xh_av, xhe_av = it["xh_av"], it["xhe_av"]
    de = nd * (xh_av[n:] * (1 - ABU_HE) + float(np.float32(7.1e-7)) + ABU_HE * (xhe_av[n:2 * n] + 2.0 * xhe_av[2 * n:]))
    totrec = np.sum(nd * (xh_av[n:] * rc[1] * (1 - ABU_HE) + xhe_av[n:2 * n] * rc[3] * ABU_HE * 0.04) * de * clump) * vol * dt
    totcol = np.sum(nd * de * (xh_av[:n] * rc[8] + xhe_av[:n] * rc[9] + xhe_av[n:2 * n] * rc[10])) * vol * dt
    recom = np.sum(nd * ABU_HE * clump * (xhe_av[2 * n:] * 1.121 * rc[6] + xhe_av[n:2 * n] * rc[3] * 0.96) * ABU_HE * de) * vol * dt
    return np.array([totrec, totcol, recom])


def _run_directed(pkg, tables, monkeypatch, case, runs, dt, pieces=None):
    """The directed case's passes under both residency settings; per setting the coefficients and total_rates after each pass."""
    nc, seconds = case["ncell"], dt * cc.YEAR
    cuts = [0] + list(pieces or []) + [nc]
    left_behind = {}
    for env, resident in RESIDENCIES:
        e = _engine(pkg, tables, case, monkeypatch, env)
        try:
            chained = lr.chain([r["W"] for r in runs], resident=resident)
            after = []
            for p, (exp, (launches, first)) in enumerate(zip(runs, chained)):
                if pieces:
                    for a, b in zip(cuts, cuts[1:]):
                        e.global_pass_cells(seconds, a, b - a)
                    conv = e.global_pass_finish()
                else:
                    conv = e.global_pass(seconds)
                it = _check_pass(pkg, e, exp, conv, launches, len(cuts) - 2,
                                 f"{case['mesh']} dt={dt:g} yr residency={env} pass {p} (first ceiling {first})")
                rc = e.get_reccoef()
                tot = e.total_rates(seconds, rc)
                if case["clumping_grid"] is None:           # (the host formula above knows the scalar clumping only)
                    assert np.allclose(tot, _total_rates(case, it, rc, seconds), rtol=1e-12, atol=0), (env, p)
                after.append((rc, tot))
            left_behind[env] = after
        finally:
            e.close()
    (_, a), (_, b) = left_behind.items()
    for p, ((rc_a, tot_a), (rc_b, tot_b)) in enumerate(zip(a, b)):
        assert np.any(rc_a != 0.0) and np.array_equal(rc_a, rc_b), ("get_reccoef differs between the residency settings", p, rc_a, rc_b)
        assert np.array_equal(tot_a, tot_b), ("total_rates differs between the residency settings", p, tot_a, tot_b)


@pytest.mark.parametrize("dt", cc.DTS)
@pytest.mark.parametrize("name", sorted(cc.MESHES))
def test_directed_case(pkg, tables, oracle_runs, monkeypatch, name, dt):
    """Uploaded state, temperatures and rates, three global passes: on 8 x 4 x 6 (a partial last wave under the 64- and the
    128-thread block, rows only) and on 8 x 4 x 8 (8 x 4 x 2 bricks in the first launch, rows in the follow-ups).  With
    residency 0 every pass makes the five launches 16, 64, 256, 1 024, none.  The coefficients the last cell leaves behind
    (get_reccoef; that cell needs more than 1 024 sub-steps) and total_rates are the same under both settings."""
    case, runs = oracle_runs(name, dt)
    _run_directed(pkg, tables, monkeypatch, case, runs, dt)


def test_directed_case_in_pieces(pkg, tables, oracle_runs, monkeypatch):
    """global_pass_cells in four pieces cut at 1, 65 and 130 -- none a multiple of 64, alternating between two streams, all
    appending to one deferred list -- then global_pass_finish: launches = pieces + follow-ups."""
    case, runs = oracle_runs("ragged", cc.DTS[0])
    _run_directed(pkg, tables, monkeypatch, case, runs, cc.DTS[0], pieces=cc.PIECES)


def test_directed_case_with_a_clumping_grid(pkg, tables, oracle_runs, monkeypatch):
    """A REAL(4) clumping grid, 1 ... 6, read per cell through the deferred lists as well: one pass."""
    case, runs = oracle_runs("ragged", cc.DTS[0], clump=True, npass=1)
    _run_directed(pkg, tables, monkeypatch, case, runs, cc.DTS[0])


def test_raytraced_sequence(pkg, tables, oracle_runs, monkeypatch):
    """Eight outer iterations of the 8 x 4 x 4 two-source heating case: the first ceiling moves by itself (16, 64 and 256 all
    occur), and the launch counts follow the model through it.  What a late launch writes for the next sweep (`packed`, then
    its transposed copy) is what pass k + 1 reads: the columns and the rate grids of every pass equal the oracle's too."""
    case, runs = oracle_runs("ray")
    for env, resident in RESIDENCIES:
        chained = lr.chain([r["W"] for r in runs], resident=resident)
        e = _engine(pkg, tables, case, monkeypatch, env)
        try:
            for p, (exp, (launches, first)) in enumerate(zip(runs, chained)):
                e.set_rates_to_zero()
                e.pass_sources(1, 1)
                rates, cols = e.download_rates(), e.download_columns()
                for k, g in (("phih", rates["phih_grid"]), ("phihe", rates["phihe_grid"]), ("phiheat", rates["phiheat"]),
                             ("coldensh_out", cols["coldensh_out"]), ("coldenshe_out", cols["coldenshe_out"])):
                    assert np.array_equal(g, exp[k]), (env, p, k, int((g != exp[k]).sum()))
                assert rates["sum_nbox"] == exp["sum_nbox"], (env, p)
                conv = e.global_pass(cc.RAY_DT * cc.YEAR)
                _check_pass(pkg, e, exp, conv, launches, 0, f"ray-traced residency={env} pass {p} (first ceiling {first})")
        finally:
            e.close()


def test_one_long_cell_alone(pkg, tables, oracle_runs, monkeypatch):
    """c2r_evolve0d_global on a cell of the directed case that needs more than 1 024 sub-steps, on a fresh context: that
    cell's iteration state and temperature equal the oracle's, every other cell is untouched."""
    case, runs = oracle_runs("ragged", cc.DTS[0])
    exp, nc, mesh = runs[0], case["ncell"], case["mesh"]
    q = int(np.nonzero(exp["W"] > 1024)[0][0])
    pos = (C.c_int * 3)(q % mesh[0] + 1, (q // mesh[0]) % mesh[1] + 1, q // (mesh[0] * mesh[1]) + 1)
    for env, _ in RESIDENCIES:
        e = _engine(pkg, tables, case, monkeypatch, env)
        try:
            before, temp_before = e.download_iter_state(), _temperature(pkg, e, nc)
            conv = C.c_int(0)
            e._chk(e.lib.c2r_evolve0d_global(e.h, cc.DTS[0] * cc.YEAR, pos, C.byref(conv)))
            after, temp_after = e.download_iter_state(), _temperature(pkg, e, nc)
            for k in ITER:
                want = before[k].copy()
                want[q::nc] = exp[k][q::nc]
                assert np.array_equal(after[k], want), (env, k, q)
            want = temp_before.copy()
            want[q::nc] = exp["temperature"][q::nc]
            assert np.array_equal(temp_after, want), (env, q)
            assert not np.array_equal(after["xh_av"][q::nc], before["xh_av"][q::nc])     # the cell did move
        finally:
            e.close()


@pytest.mark.parametrize("value", ["-1", "many", "12cells", ""])
def test_residency_knob_rejects_what_is_no_cell_count(pkg, monkeypatch, value):
    monkeypatch.setenv("C2R_CHEM_RESIDENT_CELLS", value)
    with pytest.raises(pkg.C2RayHipError, match="C2R_CHEM_RESIDENT_CELLS"):
        pkg.HipEngine((8, 4, 6), 0).close()
