"""Point-source hand-over between meshes stacked along z: exit strips (c2r_select_source_face_exit,
c2r_download_source_face_exit) and entry columns (c2r_set_source_face_entry).  python -m pytest tests -m gpu.

The reference throughout is W, one deep mesh run by the product's open path with the source inside (tests/source_handover_cases.py).
A, B, C are parts of W along z.  The mesh that holds the source hands its exit strip to the next one, which takes it in as a
ghost layer and has to reproduce its part of W.

ROUNDS.  A source with entry columns is traced for the rounds it is given, cut at its own reach.  In these thin ("ionised")
cases every box runs to its reach, so a part upstream stops for geometry alone (A of test 1: one round, its reach is 9 cells)
and has decided nothing; the rounds handed down are W's (three), which is what the part downstream needs, and the precondition
asserted is that W and the part upstream agree where they can: both ran to their reach, and their final boxes hold the same
cells of the part.

STRIPS.  cinterp forms its crossing points from absolute coordinates (SHIFTED_REL in tests/test_gpu_external_sources.py), so a
part whose indices are shifted against W's -- A = W's z = 21..36 is -- has W's columns to rounding only: in the cells that lie
on an x or y face of their shell, whose crossing points are formed from the absolute z of the source.  A layer that lies
further below the source than the mesh reaches to either side (here: 9 cells or more against 7) descends from cells on z faces
alone, whose crossing points are formed from x and y, which a stack along z does not shift: such a strip has W's bits, and the
tests assert that it has.  Anywhere else a part has W's bits once it is told where it lies in W (c2r_set_mesh_origin): cinterp
then takes W's coordinates.  Every bit-for-bit test still runs twice: with the strip that A (or B) hands over, as a stack
does, and with the strip cut from W's own columns in that layer (HipEngine.download_columns).
"""
import numpy as np
import pytest

import source_handover_cases as hc
from conftest import rel_err
from source_handover_cases import Z_HIGH, Z_LOW, one_pass
from test_gpu_external_sources import SHIFTED_REL, TRACE_KEYS, oracle

import external_source_cases as xc

pytestmark = pytest.mark.gpu
N = (14, 14, 36)
SRC = (7, 8, 30)
FLUX = 2.0e7
COLS = ("coldensh_out", "coldenshe_out")


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


@pytest.fixture(scope="module")
def deep(pkg, tables):
    """W of a kind, run once: get(open_axes, heat=False, src=SRC, kind="ionised") -> dict(stack, rates, cols, trace)."""
    cache = {}

    def get(open_axes, heat=False, src=SRC, kind="ionised"):
        key = (open_axes, heat, src, kind)
        if key not in cache:
            st = hc.Stack(pkg, N, open_axes, kind, [src], [FLUX], heat=heat)
            e = st.engine(pkg, tables)
            rates = one_pass(e)
            cache[key] = dict(stack=st, rates=rates, cols=e.download_columns(), trace=e.source_trace(1))
            e.close()
        return cache[key]
    return get


def worst(got, ref, keys):
    return max(float(np.max(rel_err(got[k], ref[k]))) for k in keys)


def assert_equal(got, ref, keys):
    for k in keys:
        assert np.array_equal(got[k], ref[k]), (k, float(np.max(rel_err(got[k], ref[k]))), int(np.count_nonzero(got[k] != ref[k])))


def ran_to_reach(trace):
    return trace["box_lo"] == trace["reach_l"] and trace["box_hi"] == trace["reach_r"]


def upstream(pkg, tables, st, z_lo, z_hi, face, batch=None, entry=None, placed=False):
    """The part z_lo..z_hi with source 1 selected for exit through `face` (and, entry = (face, strip, rounds), with entry
    columns; placed: told where it lies in W), after one pass: (engine, rates, strip, rounds, reached)."""
    e = st.engine(pkg, tables, z_lo, z_hi, batch=batch, placed=placed)
    assert e.mesh_origin == ((0, 0, z_lo - 1) if placed else (0, 0, 0))
    e.select_source_face_exit(face, [1])
    if entry is not None:
        e.set_source_face_entry(1, *entry)
    rates = one_pass(e)
    strip, rounds, reached = e.download_source_face_exit(face, 1)
    return e, rates, strip, rounds, reached


def downstream(pkg, tables, st, z_lo, z_hi, face, strip, rounds, batch=None, placed=False):
    e = st.engine(pkg, tables, z_lo, z_hi, batch=batch, placed=placed)
    e.set_source_face_entry(1, face, strip, rounds)
    rates = one_pass(e)
    rates.update(e.download_columns())
    rates["trace"] = e.source_trace(1)
    e.close()
    return rates


def reference(w, z_lo, z_hi, keys):
    st = w["stack"]
    return {k: st.part_of(w["cols"][k] if k in COLS else w["rates"][k], z_lo, z_hi) for k in keys}


# -- 1. unshifted ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strip_of", ["handed", "deep"])
@pytest.mark.parametrize("open_axes,heat,batch", [("xyz", False, 1), ("xyz", False, 256), ("z", False, 1), ("z", False, 256),
                                                    ("xyz", True, 256), ("z", True, 256)])
def test_unshifted_bit_for_bit(pkg, tables, deep, open_axes, heat, batch, strip_of):
    """W = (14, 14, 36), thin gas, the source at z = 30; A = W's z = 21..36, B = z = 1..20, whose source stands 10 cells beyond
    its +z face and 29 cells from z = 1: three rounds.  B's rate grids and outgoing columns equal W's [..., :20], sum_nbox the
    rounds.  strip_of = "deep": B is given W's own columns of the layer z = 21; "handed": the strip A hands over, which is W's
    layer bit for bit although A's indices are shifted by 20 (the module's text says why)."""
    w = deep(open_axes, heat)
    st = w["stack"]
    keys = ("phih_grid", "phihe_grid") + (("phiheat",) if heat else ()) + COLS
    a, _, strip_a, rounds_a, reached = upstream(pkg, tables, st, 21, 36, Z_LOW, batch)
    ta = a.source_trace(1)
    a.close()
    # precondition, never skipped: W and A ran to their reach, and A's final box is W's as far as A's cells go
    assert w["trace"]["nbox"] == 3 and ran_to_reach(w["trace"]) and ran_to_reach(ta) and rounds_a == ta["nbox"] and reached
    assert ta["box_lo"][:2] == w["trace"]["box_lo"][:2] and ta["box_hi"] == w["trace"]["box_hi"] and ta["box_lo"][2] == 21 - SRC[2]
    strip_w = st.layer_strip(w["cols"], 21)
    print("A's strip against W's layer z = 21: rel", float(np.max(rel_err(strip_a.reshape(-1), strip_w.reshape(-1)))))
    assert np.array_equal(strip_a, strip_w)
    b = downstream(pkg, tables, st, 1, 20, Z_HIGH, strip_a if strip_of == "handed" else strip_w, w["trace"]["nbox"], batch)
    ref = reference(w, 1, 20, keys)
    print(open_axes, heat, batch, strip_of, "worst rel", worst(b, ref, keys))
    assert b["sum_nbox"] == 3 and b["trace"]["nbox"] == 3
    assert_equal(b, ref, keys)


# -- 2. chain ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chains(pkg, tables, deep):
    """run(kind): A = 25..36 -> B = 13..24 -> C = 1..12 of W, run once per kind.  B takes A's strip and is selected for exit
    through its low face; C takes B's; the rounds are W's (B, whose reach is 17 cells, traces two of them).  Every part is
    told where it lies in W (c2r_set_mesh_origin: 24, 12, 0 along z), and cinterp forms its crossing points from W's coordinates.
    "deep": each part is given W's own columns of the layer above it instead; "unshifted": the strips handed over, no part told."""
    cache = {}

    def run(kind):
        if kind in cache:
            return cache[kind]
        w = deep("xyz")
        st = w["stack"]
        rounds = w["trace"]["nbox"]
        placed = kind != "unshifted"
        a, rates_a, strip_a, _, _ = upstream(pkg, tables, st, 25, 36, Z_LOW, placed=placed)
        a.close()
        to_b = st.layer_strip(w["cols"], 25) if kind == "deep" else strip_a
        b, rates_b, strip_b, rounds_b, reached_b = upstream(pkg, tables, st, 13, 24, Z_LOW, entry=(Z_HIGH, to_b, rounds), placed=placed)
        b.close()
        to_c = st.layer_strip(w["cols"], 13) if kind == "deep" else strip_b
        c = downstream(pkg, tables, st, 1, 12, Z_HIGH, to_c, rounds, placed=placed)
        cache[kind] = dict(w=w, kind=kind, rates_a=rates_a, strip_a=strip_a, rates_b=rates_b, strip_b=strip_b, rounds_b=rounds_b,
                           reached_b=reached_b, c=c)
        return cache[kind]
    return run


@pytest.mark.parametrize("strip_of", ["handed", "deep", "unshifted"])
def test_chain_last_part_bit_for_bit(chains, strip_of):
    """C, which keeps W's indices, equals W bit for bit where the parts are told where they lie: rate grids and outgoing columns.
    Untold ("unshifted"), A and B take their own indices for W's and agree with W within SHIFTED_REL, and so does C, which
    inherits their rounding through the strips (measured for B: 1.5e-13, in 16 and 28 cells: the cells with |dx| or |dy| = 7 >
    |dz| lie on x and y faces of their shell, whose crossing points use the z of the source, 18 in B and 30 in W)."""
    chain = chains(strip_of)
    w, st, keys = chain["w"], chain["w"]["stack"], ("phih_grid", "phihe_grid")
    ref_b, ref_c = reference(w, 13, 24, keys), reference(w, 1, 12, keys + COLS)
    print(chain["kind"], "B", worst(chain["rates_b"], ref_b, keys), "C", worst(chain["c"], ref_c, keys + COLS))
    assert chain["rounds_b"] == 2 and chain["reached_b"] and chain["c"]["sum_nbox"] == 3
    assert worst(chain["rates_b"], ref_b, keys) <= SHIFTED_REL and worst(chain["c"], ref_c, keys + COLS) <= SHIFTED_REL
    if strip_of != "unshifted":
        assert np.array_equal(chain["strip_a"], st.layer_strip(w["cols"], 25))
        assert np.array_equal(chain["strip_b"], st.layer_strip(w["cols"], 13))
        assert_equal(chain["rates_a"], reference(w, 25, 36, keys), keys)
        assert_equal(chain["c"], ref_c, keys + COLS)


@pytest.mark.parametrize("strip_of", ["handed", "deep"])
def test_chain_middle_part_bit_for_bit(chains, strip_of):
    """B = W's z = 13..24 equals W bit for bit.  The indices of A and B are shifted by 24 and 12 against W's, and cinterp forms
    its crossing points from absolute coordinates: they have W's bits because they are given W's coordinates
    (c2r_set_mesh_origin)."""
    chain = chains(strip_of)
    w, keys = chain["w"], ("phih_grid", "phihe_grid")
    ref_b = reference(w, 13, 24, keys)
    print(chain["kind"], "B against W: worst rel", worst(chain["rates_b"], ref_b, keys),
          "cells that differ", [int(np.count_nonzero(chain["rates_b"][k] != ref_b[k])) for k in keys])
    assert_equal(chain["rates_b"], ref_b, keys)


# -- 3. shifted --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", [False, True])
def test_shifted_within_rounding(pkg, tables, deep, placed):
    """The mirror image of test 1: the source at z = 7, A = W's z = 1..16, B = z = 17..36, whose indices are shifted by 16
    against W's.  Grids within SHIFTED_REL (thin gas, at most 30 shells: its derivation covers this case).  Measured: 0.0 -- B
    begins 10 cells above the source and reaches 7 to either side, so every cell of it lies on a z face of its shell.  placed:
    B is told where it lies in W (c2r_set_mesh_origin, 16 along z) and has W's bits by construction."""
    src = (SRC[0], SRC[1], 7)
    w = deep("xyz", src=src)
    st = w["stack"]
    keys = ("phih_grid", "phihe_grid")
    a, _, strip_a, _, reached = upstream(pkg, tables, st, 1, 16, Z_HIGH)
    ta = a.source_trace(1)
    a.close()
    assert w["trace"]["nbox"] == 3 and ran_to_reach(w["trace"]) and ran_to_reach(ta) and reached
    b = downstream(pkg, tables, st, 17, 36, Z_LOW, strip_a, w["trace"]["nbox"], placed=placed)
    ref = reference(w, 17, 36, keys)
    print("shifted: placed", placed, "worst rel", worst(b, ref, keys))
    assert b["sum_nbox"] == 3
    assert worst(b, ref, keys) <= SHIFTED_REL
    if placed:      # told where it lies in W, B has W's bits
        assert_equal(b, ref, keys)


# -- 4. zero strip -----------------------------------------------------------------------------------------------------------
def test_zero_strip_is_the_run_without_entry(pkg, tables):
    """"mixed" gas, B = z = 1..20 of W with the source 10 cells beyond +z: an all-zero strip with the rounds of the run
    without an entry gives that run's rate grids, bit for bit."""
    st = hc.Stack(pkg, N, "xyz", "mixed", [SRC], [FLUX])
    e = st.engine(pkg, tables, 1, 20)
    plain = one_pass(e)
    rounds = e.source_trace(1)["nbox"]
    assert rounds >= 1 and e.source_face_entry(1) == (-1, 0)
    e.set_source_face_entry(1, Z_HIGH, np.zeros((3, N[0] * N[1])), rounds)
    assert e.source_face_entry(1) == (Z_HIGH, rounds)
    zero = one_pass(e)
    assert zero["sum_nbox"] == rounds
    assert_equal(zero, plain, ("phih_grid", "phihe_grid"))
    e.set_source_face_entry(1)          # cleared: the run without an entry again, loss included
    assert e.source_face_entry(1) == (-1, 0)
    again = one_pass(e)
    assert_equal(again, plain, ("phih_grid", "phihe_grid"))
    assert again["photon_loss"][0] == plain["photon_loss"][0] and again["sum_nbox"] == plain["sum_nbox"]
    e.close()


# -- 5. two sources in one batch ---------------------------------------------------------------------------------------------
def test_entry_and_inside_source_in_one_batch(pkg, tables, deep):
    """B = z = 1..20 with the source of test 1 (entry columns) and a second source inside B, in one batch: the grids are the
    fold, in source order from 0.0, of the two single-source runs, and the inside source's trace is what it is alone."""
    w = deep("xyz")
    st2 = hc.Stack(pkg, N, "xyz", "ionised", [SRC, (5, 9, 6)], [FLUX, 1.2e7])
    strip, rounds = w["stack"].layer_strip(w["cols"], 21), w["trace"]["nbox"]
    runs = []
    for sources in ([0], [1], [0, 1]):
        e = st2.engine(pkg, tables, 1, 20, sources=sources, batch=256)
        if 0 in sources:
            e.set_source_face_entry(1, Z_HIGH, strip, rounds)
        r = one_pass(e)
        r["traces"] = [e.source_trace(k + 1) for k in range(len(sources))]
        runs.append(r)
        e.close()
    first, second, both = runs
    for k in ("phih_grid", "phihe_grid"):
        assert np.array_equal(both[k], first[k] + second[k]), k
    assert both["sum_nbox"] == first["sum_nbox"] + second["sum_nbox"]
    assert both["photon_loss"][0] == first["photon_loss"][0] + second["photon_loss"][0]
    assert all(both["traces"][1][k] == second["traces"][0][k] for k in TRACE_KEYS), (both["traces"][1], second["traces"][0])
    assert_equal(first, reference(w, 1, 20, ("phih_grid", "phihe_grid")), ("phih_grid", "phihe_grid"))


# -- 6. kept loss ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strip_of", ["handed", "deep"])
def test_kept_loss_is_the_mesh_surface(pkg, tables, strip_of):
    """W with every axis open, thin gas, its final box its whole reach, escape maps on: B's photon_loss(1) is W's z-low map plus
    the rows z <= 20 of W's four lateral maps, to 2 n 2^-53 relative -- two differently associated sums of n non-negative
    terms, n the number of map cells added."""
    st = hc.Stack(pkg, N, "xyz", "ionised", [SRC], [FLUX])
    e = st.engine(pkg, tables)
    e.enable_face_loss(True)
    one_pass(e)
    tw = e.source_trace(1)
    assert ran_to_reach(tw)
    maps = [e.face_loss_map(Z_LOW)] + [e.face_loss_map(f)[:20, :] for f in range(4)]
    cols = e.download_columns()
    e.close()
    n = sum(m.size for m in maps)
    expect = float(sum(float(np.sum(m)) for m in maps))
    if strip_of == "handed":
        a, _, strip, _, _ = upstream(pkg, tables, st, 21, 36, Z_LOW)
        a.close()
    else:
        strip = st.layer_strip(cols, 21)
    b = downstream(pkg, tables, st, 1, 20, Z_HIGH, strip, tw["nbox"])
    got = float(b["photon_loss"][0])
    tol = 2.0 * n * 2.0 ** -53
    print(strip_of, "kept loss", got, "maps", expect, "rel", abs(got - expect) / expect, "n", n, "tolerance", tol)
    assert n == N[0] * N[1] + 2 * 20 * (N[0] + N[1])
    assert abs(got - expect) <= tol * expect


# -- 7. refusals and lifetime ------------------------------------------------------------------------------------------------
def _refused(pkg, call, *a, match=None, **kw):
    with pytest.raises(pkg.C2RayHipError, match=match):
        call(*a, **kw)


def test_refusals_and_lifetime(pkg, tables, deep):
    w = deep("xyz")
    st2 = hc.Stack(pkg, N, "xyz", "ionised", [SRC, (5, 9, 6)], [FLUX, 1.2e7])
    F = N[0] * N[1]
    good = np.zeros((3, F))
    e = st2.engine(pkg, tables, 1, 20)         # source 1 beyond +z, source 2 inside
    # -- entry: every refusal leaves the getters as they were
    e.set_source_face_entry(1, Z_HIGH, good + 1.0, 3)
    before = [e.source_face_entry(1), e.source_face_entry(2)]
    assert before == [(Z_HIGH, 3), (-1, 0)]
    bad = good.copy(); bad[1, 5] = -1.0
    nan = good.copy(); nan[2, 7] = np.nan
    inf = good.copy(); inf[0, 0] = np.inf
    for args, match in (((0, Z_HIGH, good, 3), "not in"), ((3, Z_HIGH, good, 3), "not in"), ((1, 6, good, 3), "face"),
                        ((1, -1, good, 3), "face"), ((1, Z_LOW, good, 3), "beyond face"), ((1, 1, np.zeros((3, N[1] * 20)), 3), "beyond face"),
                        ((2, Z_HIGH, good, 3), "beyond face"), ((1, Z_HIGH, good, 0), "rounds"), ((1, Z_HIGH, bad, 3), "not negative"),
                        ((1, Z_HIGH, nan, 3), "finite"), ((1, Z_HIGH, inf, 3), "finite")):
        _refused(pkg, e.set_source_face_entry, *args, match=match)
        assert [e.source_face_entry(1), e.source_face_entry(2)] == before, args[:2]
    _refused(pkg, e.source_face_entry, 3, match="not in")
    # -- the mesh's origin: refused out of range, kept otherwise
    assert e.mesh_origin == (0, 0, 0)
    e.set_mesh_origin((0, 0, 5))
    for origin in ((0, 0, 2 ** 20 + 1), (-2 ** 20 - 1, 0, 0)):
        _refused(pkg, e.set_mesh_origin, origin, match="not in")
        assert e.mesh_origin == (0, 0, 5)
    _refused(pkg, e.do_source, 1, match="outside the mesh")
    # -- exit: refusals, and a download before any pass
    e.select_source_face_exit(Z_LOW, [2, 1])
    for args, match in (((6, [1]), "face"), ((-1, [1]), "face"), ((Z_LOW, [3]), "not in"), ((Z_LOW, [0]), "not in"), ((Z_LOW, [1, 2, 1]), "twice")):
        _refused(pkg, e.select_source_face_exit, *args, match=match)
    _refused(pkg, e.download_source_face_exit, Z_LOW, 1, match="no pass has swept")
    _refused(pkg, e.download_source_face_exit, Z_HIGH, 1, match="not selected")
    # -- inside an open slab-wise pass
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources_begin(1, 1, 2)
    _refused(pkg, e.set_source_face_entry, 1, Z_HIGH, good, 3, match="still open")
    _refused(pkg, e.set_mesh_origin, (0, 0, 2), match="still open")
    _refused(pkg, e.select_source_face_exit, Z_LOW, [1], match="still open")
    _refused(pkg, e.download_source_face_exit, Z_LOW, 1, match="still open")
    e.pass_sources_end()
    assert e.source_face_entry(1) == (Z_HIGH, 3)
    s1, r1, m1 = e.download_source_face_exit(Z_LOW, 1)     # the slab-wise pass filled the strips
    s2, r2, m2 = e.download_source_face_exit(Z_LOW, 2)
    assert (r1, m1) == (3, True) and m2 and s1.shape == (3, F) and np.all(s1 > 0.5) and np.all(s2 >= 0.0)
    # -- beams, horizons, curves and boundaries keep the entries; a new source list clears entries and selection
    e.set_source_beams([None, None])
    e.set_boundaries((False, False, False))
    assert e.source_face_entry(1) == (Z_HIGH, 3)
    src = pkg.SourceProps(st2.case.srcpos - np.array([0, 0, 0], dtype=np.int32), st2.case.flux, st2.case.s_star)
    e.set_sources_external(src)
    assert [e.source_face_entry(1), e.source_face_entry(2)] == [(-1, 0), (-1, 0)]
    assert e.mesh_origin == (0, 0, 5)       # (the origin belongs to the mesh: it stays)
    _refused(pkg, e.download_source_face_exit, Z_LOW, 1, match="not selected")
    e.close()
    # -- a face of a periodic axis
    stp = hc.Stack(pkg, N, "z", "ionised", [SRC], [FLUX])
    e = stp.engine(pkg, tables, 21, 36)
    _refused(pkg, e.select_source_face_exit, 0, [1], match="periodic")
    _refused(pkg, e.set_mesh_origin, (3, 0, 0), match="periodic")
    e.set_mesh_origin((0, 0, 20))
    _refused(pkg, e.set_boundaries, True, match="origin")
    e.set_mesh_origin()
    assert e.mesh_origin == (0, 0, 0)
    e.select_source_face_exit(Z_LOW, [1])
    _refused(pkg, e.set_boundaries, True, match="exit strips")       # (the axis of a selection has to stay open)
    assert e.periodic_axes == (True, True, False)
    e.select_source_face_exit(Z_LOW, [])
    _refused(pkg, e.download_source_face_exit, Z_LOW, 1, match="not selected")
    e.close()


def test_a_box_that_never_meets_the_face(pkg, tables):
    """Opaque gas, a source in the middle of 24^3: one round, a box of +-10 cells that ends a layer short of the z-low face.
    reached = 0 and an all-zero strip; do_source fills the strip of a source inside the mesh as a pass does."""
    st = hc.Stack(pkg, (24, 24, 24), "xyz", "opaque", [(12, 12, 12)], [1.0e4])
    e = st.engine(pkg, tables)
    e.select_source_face_exit(Z_LOW, [1])
    e.select_source_face_exit(Z_HIGH, [1])
    one_pass(e)
    assert e.source_trace(1)["nbox"] == 1
    strip, rounds, reached = e.download_source_face_exit(Z_LOW, 1)
    assert rounds == 1 and not reached and not strip.any() and not np.signbit(strip).any()
    strip, rounds, reached = e.download_source_face_exit(Z_HIGH, 1)
    assert rounds == 1 and not reached and not strip.any()
    e.close()
    st = hc.Stack(pkg, (24, 24, 24), "xyz", "opaque", [(12, 12, 3)], [1.0e4])
    e = st.engine(pkg, tables)
    e.select_source_face_exit(Z_LOW, [1])
    one_pass(e)
    by_pass = e.download_source_face_exit(Z_LOW, 1)
    cols = e.download_columns()
    e.begin_step()
    e.set_rates_to_zero()
    e.do_source(1)
    by_point = e.download_source_face_exit(Z_LOW, 1)
    assert by_pass[1:] == (1, True) and by_point[1:] == (1, True)
    assert np.array_equal(by_pass[0], by_point[0]) and np.array_equal(by_pass[0], st.layer_strip(cols, 1))
    assert np.count_nonzero(by_pass[0][0]) == 21 * 21        # (the box: +-10 cells across)
    e.close()


def test_contexts_without_hand_over_keep_their_bits(pkg, orc, otables, tables):
    """A context that never calls the new entry points: case_several_rounds of tests/external_source_cases.py -- two sources
    outside, one inside -- against the oracle's grids, bit for bit, as before."""
    case = xc.case_several_rounds(pkg)
    ref = oracle(case, pkg, orc, otables)
    e = case.engine(pkg, tables)
    got = one_pass(e)
    e.close()
    assert_equal(got, ref, ("phih_grid", "phihe_grid"))
