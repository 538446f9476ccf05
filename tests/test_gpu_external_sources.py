"""Point sources outside the mesh, c2r_set_sources_external, against the oracle.  python -m pytest tests -m gpu.

tests/external_source_cases.py has the two references: the oracle's periodic run on a vacuum-padded mesh for the grids (bit for
bit on the region), and the product's pinned open path on the virtual mesh -- the region extended by ndens = 0 cells up to the
sources -- for photon_loss(1), sum_nbox and the cells a source traces.  The oracle's own while-test counts what leaves through
the faces of its vacuum, so it never stops early; where the gas of a case may stop a box ("mixed", "opaque"), the rounds are
those of the virtual run and the grids are composed from the oracle's runs of each source alone, cut to the box of those
rounds (ExternalCase.compose).
"""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import axis_boundary_cases as ab
import beam_reference as br
import curve_reference as cr
import external_source_cases as xc
from conftest import rel_err

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
DT = 1.0e6 * 3.15576e7  # s
RATES, STATE = ("phih_grid", "phihe_grid"), ab.ITER_STATE


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


def one_pass(e):
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    return e.download_rates()


def oracle(case, pkg, orc, otables, **kw):
    with np.errstate(all="ignore"):       # (the oracle's vacuum cells hold 0/0; they are never compared)
        return case.oracle_pass(pkg, orc, otables, **kw)


def composed(case, pkg, orc, otables, tables, dt=None, lls_grid=None):
    """Rounds per source from the pinned open path on the source's virtual mesh, then the oracle's grids composed for them."""
    rounds = [virtual_alone(case, pkg, tables, ns, lls_grid)["sum_nbox"] for ns in range(len(case.flux))]
    ref = case.compose(pkg, orc, otables, rounds, lls_grid=lls_grid, dt=dt)
    ref.update(sum_nbox=sum(rounds), rounds=rounds)
    return ref


TRACE_KEYS = ("reach_l", "reach_r", "box_lo", "box_hi", "nbox", "block_cells", "swept_cells", "sweep_threads")


def virtual_alone(case, pkg, tables, ns, lls_grid=None):
    """Source ns (0-based) alone on ITS virtual mesh -- the bounding box of the region and that source: a mesh that also held
    the other sources would put vacuum beside this one, which its reach does not have --: the region's grids, photon_loss(1),
    sum_nbox, the trace, and the shift of the region."""
    ve, v = case.virtual_engine(pkg, tables, [ns], lls_grid=lls_grid)
    virt = one_pass(ve)
    out = {k: case.extract_virtual(virt[k], v, [ns]) for k in RATES}
    out.update(sum_nbox=virt["sum_nbox"], photon_loss=float(virt["photon_loss"][0]), trace=ve.source_trace(1), shift=case.virtual_shift([ns]))
    ve.close()
    return out


# A virtual mesh that shifts the region (a source beyond a LOW face) is no bit-exact reference: cinterp forms its crossing
# points from absolute coordinates, alam * d + x0 with |x0| < 2^7, so a shift moves each of the two weights of a cell by up to
# 2^-46 absolute, a column by some 2^-45 relative per shell, and the columns of the outermost of the <= 30 shells here by some
# 30 * 2^-45 = 1e-12; the rates of these thin ("ionised") cases follow the columns with factors of order one.  Ten times that,
# for the GRIDS of a shifted virtual run; unshifted, and for photon_loss(1) and the oracle's grids always, bit for bit.
SHIFTED_REL = 1.0e-11


def assert_grids_equal(got, ref, keys=RATES):
    for k in keys:
        assert np.array_equal(got[k], ref[k]), (k, float(np.max(rel_err(got[k], ref[k]))), int(np.count_nonzero(got[k] != ref[k])))


# -- 1. one round, every kind of position ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(xc.ONE_ROUND_SOURCES))
def test_one_round_every_kind_of_position(pkg, orc, otables, tables, which):
    """n = 11, "mixed" gas, M = 32: a source 1 and 4 cells beyond each of the six faces, beyond an edge, beyond a corner, and
    all of them together with two inside sources: rate grids equal to the oracle's, then the iteration state after one
    c2r_global_pass.  (A source 1 or 4 cells outside reaches 11 or 14 cells, more than the 10 of a first box: a second round
    where the light that arrives at the box's far face says so -- the rounds of the virtual run.)"""
    case = xc.case_one_round(pkg, which)
    ref = composed(case, pkg, orc, otables, tables, dt=DT)
    e = case.engine(pkg, tables)
    got = one_pass(e)
    print(which, "sum_nbox", got["sum_nbox"], "rounds", ref["rounds"])
    assert_grids_equal(got, ref)
    assert got["sum_nbox"] == ref["sum_nbox"]
    traced = np.zeros(ab.cells(case.n), dtype=bool)
    for ns in range(len(case.flux)):
        t = e.source_trace(ns + 1)
        l, r = case.reach(ns)
        assert t["reach_l"] == l and t["reach_r"] == r and t["nbox"] == ref["rounds"][ns]
        traced |= case.box_mask(ns, ref["rounds"][ns])
    assert np.count_nonzero(traced) >= 7 * 11 * 11 and np.array_equal(got["phih_grid"] > 0, traced)   # (4 cells outside: 7 planes)
    e.global_pass(DT)
    assert_grids_equal(e.download_iter_state(), ref, STATE)
    e.close()


# -- 2. several rounds ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def several_rounds(pkg, orc, otables, tables):
    """The case, the oracle's grids (M = 64), and each source alone on its virtual mesh."""
    case = xc.case_several_rounds(pkg)
    ref = oracle(case, pkg, orc, otables)
    alone = [virtual_alone(case, pkg, tables, ns) for ns in range(len(case.flux))]
    return case, ref, alone


@pytest.mark.parametrize("batch", [1, 256])
def test_several_rounds(pkg, tables, several_rounds, batch):
    """n = 24, "ionised" gas, a source 6 cells beyond the +z face, one 3 cells beyond the -x face and one inside.  Grids equal
    to the oracle's; sum_nbox, every source's trace (the same cells, the same block numbering) and photon_loss(1) -- the fold
    of the sources' losses in source order -- equal to the product's open runs on the virtual meshes; one source per batch or
    all in one; and again on a second pass with the learnt counts.
    photon_loss(1) bit for bit.  (The grids of the virtual runs: test_each_source_against_its_virtual_mesh.)"""
    case, ref, alone = several_rounds
    e = case.engine(pkg, tables)
    e.set_batch(batch)
    got = one_pass(e)
    want = 0.0
    for a in alone:
        want = want + a["photon_loss"]
    print("sum_nbox", got["sum_nbox"], "photon_loss", got["photon_loss"][0], want, "rel", rel_err(got["photon_loss"][0], want))
    assert_grids_equal(got, ref)
    assert np.all(got["phih_grid"] > 0)
    assert got["sum_nbox"] == sum(a["sum_nbox"] for a in alone) == case.expected_rounds() == 3 + 3 + 2
    assert got["photon_loss"][0] == want
    for ns, a in enumerate(alone):
        t = e.source_trace(ns + 1)
        # (sweep_threads: a launch is sized for the largest cut shell among the sources of its batch)
        assert all(t[k] == a["trace"][k] for k in TRACE_KEYS if batch == 1 or k != "sweep_threads"), (ns, t, a["trace"])
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    again = e.download_rates()
    assert_grids_equal(again, ref)
    assert again["sum_nbox"] == got["sum_nbox"] and again["photon_loss"][0] == got["photon_loss"][0]
    e.close()


@pytest.mark.parametrize("ns", [0, 1, 2], ids=["beyond+z", "beyond-x", "inside"])
def test_each_source_against_its_virtual_mesh(pkg, tables, several_rounds, ns):
    """Each source of the case alone, against the product's open run (c2r_set_sources) on the region extended by ndens = 0 cells
    up to it: sum_nbox, the trace and photon_loss(1) equal, the loss bit for bit; the grids on the region bit for bit where the
    virtual mesh does not shift the region (beyond +z, inside), within SHIFTED_REL where it does (beyond -x, three cells:
    measured 9.5e-13)."""
    case, _, alone = several_rounds
    a = alone[ns]
    e = case.engine(pkg, tables, [ns])
    got = one_pass(e)
    worst = max(float(np.max(rel_err(got[k], a[k]))) for k in RATES)
    print(ns, "shift", a["shift"], "loss", got["photon_loss"][0], a["photon_loss"], "rel", rel_err(got["photon_loss"][0], a["photon_loss"]), "grids", worst)
    assert got["sum_nbox"] == a["sum_nbox"]
    t = e.source_trace(1)
    assert all(t[k] == a["trace"][k] for k in TRACE_KEYS), (t, a["trace"])
    assert got["photon_loss"][0] == a["photon_loss"]
    if a["shift"] == [0, 0, 0]:
        assert_grids_equal(got, a)
    else:
        assert worst <= SHIFTED_REL
    e.close()


# -- 3. the general sweep kernel ------------------------------------------------------------------------------------------
_GENERIC_SNIPPET = r'''
import sys, numpy as np
sys.path.insert(0, "{root}"); sys.path.insert(0, "{root}/tests")
import __graft_entry__ as ge
import external_source_cases as xc
pkg = ge.load_package()
case = xc.case_several_rounds(pkg)
e = case.engine(pkg, pkg.RadiationTables.load())
e.begin_step(); e.set_rates_to_zero(); e.pass_sources(1, 1)
np.savez("{out}", **e.download_rates())
'''


def test_several_rounds_through_the_general_sweep_kernel(pkg, tables, several_rounds, tmp_path):
    """The same case with C2R_SWEEP_GENERIC=1 (read once per process, so in a process of its own): k_sweep_shell_ext for every
    shell instead of k_sweep_shell_fast_ext -- the same bits."""
    case, ref, alone = several_rounds
    e = case.engine(pkg, tables)
    fast = one_pass(e)
    e.close()
    out = tmp_path / "generic.npz"
    r = subprocess.run([sys.executable, "-c", _GENERIC_SNIPPET.format(root=str(ROOT), out=str(out))],
                       env={**os.environ, "C2R_SWEEP_GENERIC": "1"}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    assert_grids_equal(got, ref)
    assert int(got["sum_nbox"]) == fast["sum_nbox"] == 8 and got["photon_loss"][0] == fast["photon_loss"][0]


# -- 4. early stop --------------------------------------------------------------------------------------------------------
def test_early_stop(pkg, orc, otables, tables):
    """(24, 11, 11), "opaque" gas, a source 2 cells beyond the -x face: it stops after its first round.  Exact zeros outside the
    first box, as many as in the reference -- the product's open run on the virtual mesh (the oracle, whose while-test counts
    the vacuum faces, sweeps on) --, and the oracle's bits inside the first box."""
    case = xc.case_early_stop(pkg)
    a = virtual_alone(case, pkg, tables, 0)
    e = case.engine(pkg, tables)
    got = one_pass(e)
    print("sum_nbox", got["sum_nbox"], a["sum_nbox"], "zeros", int(np.count_nonzero(got["phih_grid"] == 0.0)), "loss rel",
          rel_err(got["photon_loss"][0], a["photon_loss"]))
    assert got["sum_nbox"] == a["sum_nbox"] == 1 and got["photon_loss"][0] == a["photon_loss"]
    t = e.source_trace(1)
    assert all(t[k] == a["trace"][k] for k in TRACE_KEYS), (t, a["trace"])
    assert t["reach_l"] == [0, -5, -5] and t["reach_r"] == [25, 5, 5] and t["box_hi"] == [10, 5, 5]
    # the first box reaches 10 cells from the source at i = -1: the mesh cells i = 1..9 of every row
    first = case.box_mask(0, 1)
    assert np.count_nonzero(first) == 9 * 11 * 11
    zeros = got["phih_grid"] == 0.0
    assert np.array_equal(zeros, ~first)
    assert 0 < np.count_nonzero(zeros) == np.count_nonzero(a["phih_grid"] == 0.0) == 15 * 11 * 11
    ref = oracle(case, pkg, orc, otables)
    assert ref["sum_nbox"] > 1                      # the oracle swept on
    for key in RATES:
        m = np.tile(first, ref[key].size // first.size)
        assert np.array_equal(got[key][m], ref[key][m]), key
        assert np.array_equal(got[key][~m], np.zeros(np.count_nonzero(~m))), key
    e.close()


# -- 5. heating -----------------------------------------------------------------------------------------------------------
def test_heating(pkg, orc, otables, tables):
    """The one-round case with isothermal = 0 and two external sources: phiheat as well."""
    case = xc.case_one_round(pkg, xc.TWO_EXTERNAL, heat=True)
    ref = composed(case, pkg, orc, otables, tables, dt=DT)
    e = case.engine(pkg, tables)
    got = one_pass(e)
    assert_grids_equal(got, ref, RATES + ("phiheat",))
    assert got["sum_nbox"] == ref["sum_nbox"] and np.count_nonzero(got["phiheat"] > 0) >= 9 * 11 * 11
    e.global_pass(DT)
    assert_grids_equal(e.download_iter_state(), ref, STATE)
    e.close()


def test_heating_three_seds(pkg, orc, gold):
    """Black-body, power-law and quasar-like SEDs on the two external sources, heating on."""
    if not (GOLD / "rad_tables_pl_qpl.npz").exists():
        pytest.skip("rad_tables_pl_qpl.npz not present")
    t = pkg.RadiationTables.load().add_sed_file(GOLD / "rad_tables_pl_qpl.npz")
    with np.load(pkg.evolve.DEFAULT_TABLES) as z:
        d = {k: z[k] for k in z.files}
    zz = gold("rad_tables_pl_qpl.npz")
    d.update({k: zz[k] for k in zz.files})
    case = xc.case_one_round(pkg, xc.TWO_EXTERNAL, heat=True, seds=True)
    ref = composed(case, pkg, orc, orc.Tables(d), t)
    e = case.engine(pkg, t)
    got = one_pass(e)
    assert_grids_equal(got, ref, RATES + ("phiheat",))
    assert got["sum_nbox"] == ref["sum_nbox"] and np.count_nonzero(got["phiheat"] > 0) >= 9 * 11 * 11
    e.close()


# -- 6. mixed boundaries --------------------------------------------------------------------------------------------------
def test_mixed_boundaries(pkg, orc, otables, tables):
    """Periodic in x and y, open in z, a source 3 cells beyond +z and one inside, on (24, 24, 11); the oracle on (24, 24, 32)."""
    case = xc.case_mixed_boundaries(pkg)
    ref = oracle(case, pkg, orc, otables, dt=DT)
    e = case.engine(pkg, tables)
    assert e.periodic_axes == (True, True, False)
    got = one_pass(e)
    assert_grids_equal(got, ref)
    assert np.all(got["phih_grid"] > 0)
    assert got["sum_nbox"] == case.expected_rounds() == 2 + 2
    assert e.source_trace(1)["reach_l"] == [-12, -12, -13] and e.source_trace(1)["reach_r"] == [11, 11, 0]
    e.global_pass(DT)
    assert_grids_equal(e.download_iter_state(), ref, STATE)
    e.close()


# -- 7. cuts --------------------------------------------------------------------------------------------------------------
def cuts_case(pkg):
    """n = 24, "ionised" gas: the source 6 cells beyond +z and the inside one."""
    return xc.case_several_rounds(pkg, [xc.SEVERAL_SOURCES[0], xc.SEVERAL_SOURCES[2]])


CONE_INTO_THE_MESH = (br.CONE, (0.1, -0.2, -1.0), float(np.cos(np.radians(40.0))))


@pytest.mark.parametrize("cut", ["cone", "horizon", "curve"])
def test_cuts(pkg, orc, otables, tables, cut):
    """A cone that points from the external source into the mesh; a horizon that ends inside the mesh (18 cells: 12 of them
    mesh); a two-step curve.  The reference is composed as tests/beam_reference.py, horizon_reference.py and curve_reference.py
    compose it, from the oracle's runs of each source alone on the vacuum-padded M = 64 mesh."""
    case = cuts_case(pkg)
    d = float(case.dr[0])
    beams = [CONE_INTO_THE_MESH, None] if cut == "cone" else None
    horizons = [18.0 * d, None] if cut == "horizon" else None
    curves = [((9.5 * d, 20.0 * d), (1.0, 0.25, 0.0)), None] if cut == "curve" else [None, None]
    with np.errstate(all="ignore"):
        ref = cr.compose(pkg, orc, otables, case, "external_cuts", curves, horizons, beams)
    e = case.engine(pkg, tables)
    if beams:
        e.set_source_beams(beams)
    if horizons:
        e.set_source_horizons(horizons)
    if cut == "curve":
        e.set_source_curves(curves)
    got = one_pass(e)
    assert_grids_equal(got, ref)
    lit = cr.lit_cells(case, 0, curves[0], None if horizons is None else horizons[0], None if beams is None else beams[0])
    assert 0 < np.count_nonzero(lit) < lit.size             # the cut goes through the mesh
    e.close()


# -- 8. LLS ---------------------------------------------------------------------------------------------------------------
def test_lls_grid(pkg, orc, otables, tables):
    """A REAL(4) lls_grid on the mesh; in the reference the same grid embedded with 0 outside: no fog in the vacuum."""
    case = xc.case_one_round(pkg, xc.TWO_EXTERNAL + [(3, 3, 3)])
    lls = (10.0 ** np.random.default_rng(88).uniform(15.5, 17, ab.cells(case.n))).astype(np.float32)
    ref = composed(case, pkg, orc, otables, tables, lls_grid=lls)
    e = case.engine(pkg, tables)
    plain = one_pass(e)
    mat = pkg.Material(case.region[0], case.region[1].copy(), case.region[2].copy(), None, True, 1.0e4, 1.0, case.reccoef)
    mat.use_LLS, mat.LLS_grid = True, lls
    e.set_lls(mat)
    got = one_pass(e)
    assert_grids_equal(got, ref)
    assert got["sum_nbox"] == ref["sum_nbox"]
    assert not np.array_equal(got["phih_grid"], plain["phih_grid"])        # the fog is there
    # the scalar fog: none in the vacuum either.  A scalar that REAL(4) holds exactly is the grid that has it in every mesh
    # cell -- and that grid, 0 outside, is held to the oracle first: the two passes agree bit for bit
    value = float(np.float32(1.0e16))
    flat = np.full(ab.cells(case.n), value, dtype=np.float32)
    assert float(flat[0]) == value
    ref_flat = composed(case, pkg, orc, otables, tables, lls_grid=flat)
    mat.LLS_grid = flat
    e.set_lls(mat)
    by_grid = one_pass(e)
    assert_grids_equal(by_grid, ref_flat)
    mat.LLS_grid, mat.coldensh_LLS = None, value
    e.set_lls(mat)
    scalar = one_pass(e)
    for k in RATES + ("photon_loss",):
        assert np.array_equal(scalar[k], by_grid[k]), k
    assert scalar["sum_nbox"] == by_grid["sum_nbox"] == ref_flat["sum_nbox"]
    assert not np.array_equal(scalar["phih_grid"], plain["phih_grid"])
    e.close()


# -- 9. the switch is clean -----------------------------------------------------------------------------------------------
def test_the_switch_is_clean(pkg, tables, several_rounds):
    """An all-inside list through the new call equals c2r_set_sources bit for bit (grids, loss, rounds, trace); going from an
    external list to a normal list on one context reproduces a fresh context."""
    case, _, _ = several_rounds
    inside = xc.ExternalCase(pkg, case.n, "xyz", case.m, "ionised", np.array([[1, 1, 1], [24, 12, 7], [7, 13, 12]], dtype=np.int32),
                             np.array([2.0e7, 1.5e7, 1.0e7]))
    keys = RATES + ("photon_loss",)
    fresh = inside._engine(pkg, tables, inside.n, inside.region, inside.periodic, inside._sources(None), external=False)
    ref = one_pass(fresh)
    ref_trace = [fresh.source_trace(ns) for ns in (1, 2, 3)]
    fresh.close()
    e = inside.engine(pkg, tables)                                      # c2r_set_sources_external, nobody outside
    got = one_pass(e)
    for k in keys:
        assert np.array_equal(got[k], ref[k]), k
    assert got["sum_nbox"] == ref["sum_nbox"] and [e.source_trace(ns) for ns in (1, 2, 3)] == ref_trace
    e.close()
    e = case.engine(pkg, tables)                                        # the external list ...
    ext = one_pass(e)
    assert not np.array_equal(ext["phih_grid"], ref["phih_grid"])
    e.set_sources(pkg.SourceProps(inside.srcpos, inside.flux, inside.s_star))   # ... then a normal one
    back = one_pass(e)
    for k in keys:
        assert np.array_equal(back[k], ref[k]), k
    assert back["sum_nbox"] == ref["sum_nbox"]
    for ns in (1, 2, 3):
        t = e.source_trace(ns)
        assert all(t[k] == ref_trace[ns - 1][k] for k in ("reach_l", "reach_r", "box_lo", "box_hi", "nbox", "swept_cells", "sweep_threads"))
    e.set_sources_external(pkg.SourceProps(case.srcpos, case.flux, case.s_star))  # ... and the external one again
    again = one_pass(e)
    for k in keys:
        assert np.array_equal(again[k], ext[k]), k
    e.close()


# -- 10. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(pkg, tables):
    """Each returns an error and a message that names the source; nothing is kept and nothing is launched: the pass after
    them gives the bits of the pass before them."""
    case = xc.case_one_round(pkg, xc.TWO_EXTERNAL + [(3, 3, 3)])
    e = case.engine(pkg, tables)
    ref = one_pass(e)
    launches = (int(e.timing().sweep_launches), int(e.timing().rates_launches))
    src = pkg.SourceProps(case.srcpos, case.flux, case.s_star)
    err = pkg.C2RayHipError
    with pytest.raises(err, match=r"c2r_set_sources: source 1 at \(4,5,13\) outside the mesh"):
        e.set_sources(src)
    # the four combinations that are not built
    with pytest.raises(err, match="c2r_enable_face_loss.*outside the mesh"):
        e.enable_face_loss(True)
    with pytest.raises(err, match="c2r_enable_horizon_loss.*outside the mesh"):
        e.enable_horizon_loss(True)
    loss = C.c_double(0.0)
    assert e.lib.c2r_evolve0d(e.h, (C.c_int * 3)(4, 5, 11), 1, 1, 0, C.byref(loss)) != 0
    assert "source 1 stands outside the mesh" in e.lib.c2r_last_error(e.h).decode()
    with pytest.raises(err, match="c2r_do_source: source 2 stands outside the mesh"):
        e.do_source(2)
    # boundaries under an external source: z (source 1) and x (source 2) have to stay open, y may close and open again
    with pytest.raises(err, match=r"c2r_set_boundaries: source 1 at \(4,5,13\).*axis 2"):
        e.set_boundaries((False, False, True))
    with pytest.raises(err, match=r"c2r_set_boundaries: source 2 at \(-1,6,3\).*axis 0"):
        e.set_boundaries((True, False, False))
    with pytest.raises(err, match="c2r_set_boundaries: source 1 "):
        e.set_boundaries(True)
    assert e.periodic is False
    assert (int(e.timing().sweep_launches), int(e.timing().rates_launches)) == launches     # nothing was launched
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    again = e.download_rates()
    for k in RATES + ("photon_loss",):
        assert np.array_equal(again[k], ref[k]), k
    # a pass that is still open
    e.set_rates_to_zero()
    e.pass_sources_begin(1, 1, 2)
    with pytest.raises(err, match="c2r_set_sources_external.*pass"):
        e.set_sources_external(src)
    e.pass_sources_end()
    # the escape maps or the horizon loss already on: the list is refused, the old one stays
    e.set_sources(pkg.SourceProps(case.srcpos[2:], case.flux[2:], case.s_star))
    e.enable_face_loss(True)
    with pytest.raises(err, match="c2r_set_sources_external.*escape maps"):
        e.set_sources_external(src)
    e.enable_face_loss(False)
    e.enable_horizon_loss(True)
    with pytest.raises(err, match="c2r_set_sources_external.*horizon loss"):
        e.set_sources_external(src)
    e.enable_horizon_loss(False)
    assert e.nsrc == 1
    # a position beyond a periodic axis; an all-periodic context
    e.set_boundaries((False, True, False))
    with pytest.raises(err, match=r"c2r_set_sources_external: source 1 at \(4,13,5\).*axis 1, which is periodic"):
        e.set_sources_external(pkg.SourceProps(np.array([[4, 13, 5]], dtype=np.int32), case.flux[:1], case.s_star))
    e.set_sources_external(pkg.SourceProps(np.array([[4, 5, 13]], dtype=np.int32), case.flux[:1], case.s_star))   # z is open
    e.set_sources(pkg.SourceProps(case.srcpos[2:], case.flux[2:], case.s_star))
    e.set_boundaries(True)
    with pytest.raises(err, match=r"c2r_set_sources_external: source 1 at \(4,5,13\).*periodic"):
        e.set_sources_external(pkg.SourceProps(np.array([[4, 5, 13]], dtype=np.int32), case.flux[:1], case.s_star))
    e.close()


def test_refusals_by_size(pkg, tables):
    """The 2^31-cell limit through the C ABI: a thin, long open mesh, (2, 2, 1700), and a source 1149 cells beyond two of its
    faces at half its length reach over 1151 x 1151 x 1700 = 2.25e9 cells.  Refused with a message that names the source and
    the limit; nothing is kept and nothing is launched: the pass after it gives the bits of the pass before it.  Likewise a
    source more than max_subbox = 1150 cells from the mesh, whose boxes never hold a mesh cell.
    (The 4096-cell limit cannot be reached through the ABI: the library clamps every reach at max_subbox = 1150.  It is held
    to the rule on the host, tests/test_external_reach_host.py, through the function the call uses.)"""
    hp = pkg.hostphys
    mesh = (2, 2, 1700)
    ndens, xh, xhe, _ = xc.gas(pkg, ab.cells(mesh), np.random.default_rng(1700), "ionised", False)
    dr, vol = hp.test_grid(24, ab.ZRED)
    mat = pkg.Material(ndens, xh.copy(), xhe.copy(), None, True, 1.0e4, 1.0, hp.reccoef(1.0e4))
    e = pkg.HipEngine(mesh, 0)
    e.set_boundaries(False)
    e.set_tables(tables)
    e.set_step(mat, pkg.GridProps(mesh, dr, vol), pkg.Cosmology(ab.ZRED, hp.H0, hp.Omega0))
    inside = pkg.SourceProps(np.array([[1, 2, 850]], dtype=np.int32), np.array([2.0e7]), 1.0e48)
    e.set_sources_external(inside)
    e.upload_state(mat)
    ref = one_pass(e)
    assert np.all(ref["phih_grid"] > 0)
    launches = (int(e.timing().sweep_launches), int(e.timing().rates_launches))
    err = pkg.C2RayHipError
    flux = np.array([2.0e7, 1.0e7])
    # source 2 of the list: l = (0, 0, -849), r = (1150, 1150, 850)
    with pytest.raises(err, match=r"c2r_set_sources_external: source 2 at \(-1148,-1148,850\).*2\^31 cells"):
        e.set_sources_external(pkg.SourceProps(np.array([[1, 2, 850], [-1148, -1148, 850]], dtype=np.int32), flux, 1.0e48))
    # one cell nearer along x, one cell further along z (l_z = -850, r_z = 849, both short of max_subbox): 1150 x 1151 x 1700
    with pytest.raises(err, match=r"source 1 at \(-1147,-1148,851\).*2\^31 cells"):
        e.set_sources_external(pkg.SourceProps(np.array([[-1147, -1148, 851]], dtype=np.int32), flux[:1], 1.0e48))
    with pytest.raises(err, match=r"source 2 at \(1,1,2851\) stands more than max_subbox = 1150 cells from the mesh along axis 2"):
        e.set_sources_external(pkg.SourceProps(np.array([[1, 2, 850], [1, 1, 2851]], dtype=np.int32), flux, 1.0e48))
    with pytest.raises(err, match=r"source 1 at \(-2000,-2000,-2000\) stands more than max_subbox"):
        e.set_sources_external(pkg.SourceProps(np.array([[-2000, -2000, -2000]], dtype=np.int32), flux[:1], 1.0e48))
    assert e.nsrc == 1 and e.source_trace(1)["reach_l"] == [0, -1, -849]
    assert (int(e.timing().sweep_launches), int(e.timing().rates_launches)) == launches          # nothing was launched
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    again = e.download_rates()
    for k in RATES + ("photon_loss",):
        assert np.array_equal(again[k], ref[k]), k
    # the farthest source that is accepted: 1150 cells beyond one face, a reach of 1151 x 2 x 1700 cells that ends on the face
    e.set_sources_external(pkg.SourceProps(np.array([[-1149, 1, 850]], dtype=np.int32), flux[:1], 1.0e48))
    assert e.source_trace(1)["reach_l"] == [0, 0, -849] and e.source_trace(1)["reach_r"] == [1150, 1, 850]
    e.close()
