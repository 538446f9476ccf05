"""Source halos: point-source hand-over across mesh edges and corners (c2r_set_source_halo).  python -m pytest tests -m gpu.

The reference throughout is W, one mesh run by the product's open path (c2r_set_sources) with the source inside
(tests/source_halo_cases.py).  W is cut along two or three axes; every part is placed with c2r_set_mesh_origin and has to
reproduce its cells of W bit for bit.  The part diagonal to the source's part takes a halo: a strip per face the source stands
beyond, the edge lines and the corner where the ghost layers meet.

Every bit-for-bit test has two variants.  "deep": the halo is cut from W's own downloaded columns.  "handed": the halo is
assembled from the neighbours' exit strips as a tiling assembles it (source_halo_cases.run_tiling) -- the part that holds the
source first, then the parts beyond one face, two, three; edge lines and the corner come out of the diagonal neighbour's exit
strip through handover.edge_of_strip / corner_of_strip.

ROUNDS.  As in tests/test_gpu_source_handover.py: thin ("ionised") gas, every box runs to its reach, so the rounds handed down
are W's, and the precondition asserted (never skipped) is that W traced more than one round and ran to its reach.
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import source_halo_cases as sh
import source_handover_cases as hc
from conftest import rel_err
from source_halo_cases import COLS, X_HIGH, X_LOW, Y_HIGH, Y_LOW, Z_HIGH, Z_LOW, one_pass, ran_to_reach

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FLUX = 2.0e7
RATES = ("phih_grid", "phihe_grid")

# test 1: a 2 x 2 tiling in x and z
W1, SRC1, CUTS1 = (20, 10, 20), (15, 5, 16), {0: 10, 2: 10}
D1 = ((1, 1, 1), (10, 10, 10))
# test 2: a 2 x 2 x 2 tiling
W2, SRC2, CUTS2 = (16, 16, 16), (12, 11, 13), {0: 8, 1: 8, 2: 8}
D2 = ((1, 1, 1), (8, 8, 8))
# test 3: ghost cells in shells 0 and 1
W3, SRC3 = (12, 10, 12), (11, 5, 11)
D3 = ((1, 1, 1), (10, 10, 10))


@pytest.fixture(scope="module")
def tables(pkg):
    return pkg.RadiationTables.load()


@pytest.fixture(scope="module")
def deep(pkg, tables):
    """W of a kind, run once: get(n, src, open_axes="xyz", heat=False, kind="ionised") -> dict(tiling, rates, cols, trace)."""
    cache = {}

    def get(n, src, open_axes="xyz", heat=False, kind="ionised"):
        key = (n, src, open_axes, heat, kind)
        if key not in cache:
            t = sh.Tiling(pkg, n, open_axes, kind, [src], [FLUX], heat=heat)
            e = t.engine(pkg, tables)
            rates = one_pass(e)
            cache[key] = dict(tiling=t, rates=rates, cols=e.download_columns(), trace=e.source_trace(1))
            e.close()
        return cache[key]
    return get


@pytest.fixture(scope="module")
def handed(pkg, tables, deep):
    """The cascade of a tiling, run once per kind: get(n, src, cuts, open_axes, heat, batch) -> run_tiling's result."""
    cache = {}

    def get(n, src, cuts, open_axes="xyz", heat=False, batch=None):
        key = (n, src, tuple(sorted(cuts.items())), open_axes, heat, batch)
        if key not in cache:
            w = deep(n, src, open_axes, heat)
            cache[key] = sh.run_tiling(pkg, tables, w["tiling"], cuts, w["trace"]["nbox"], batch=batch)
        return cache[key]
    return get


def assert_equal(got, ref, keys):
    for k in keys:
        assert np.array_equal(got[k], ref[k]), (k, float(np.max(rel_err(got[k], ref[k]))), int(np.count_nonzero(got[k] != ref[k])))


def reference(w, lo, hi, keys):
    t = w["tiling"]
    return {k: t.part_of(w["cols"][k] if k in COLS else w["rates"][k], lo, hi) for k in keys}


def keys_of(heat):
    return RATES + (("phiheat",) if heat else ()) + COLS


def deep_part(pkg, tables, w, lo, hi, batch=None):
    """The part lo..hi with the halo cut from W's own columns, after one pass."""
    t = w["tiling"]
    e = t.engine(pkg, tables, lo, hi, batch=batch)
    halo = t.halo_of_deep(w["cols"], lo, hi)
    sh.set_halo(e, halo, w["trace"]["nbox"])
    faces = tuple(sorted(halo["faces"]))
    assert e.source_halo(1) == (faces, w["trace"]["nbox"]) and e.source_face_entry(1) == (faces[0], w["trace"]["nbox"])
    out = sh.collect(e)
    out["halo"] = halo
    e.close()
    return out


def check_part(w, part, lo, hi, heat, what, upstream=False):
    keys = keys_of(heat)
    ref = reference(w, lo, hi, keys)
    print(what, "part", lo, hi, "worst rel", max(float(np.max(rel_err(part[k], ref[k]))) for k in keys), "sum_nbox", part["sum_nbox"])
    if upstream:    # a part nearer the source: its own rounds (the part that holds it) or as many of W's as its reach needs
        assert part["sum_nbox"] == part["trace"]["nbox"] <= w["trace"]["nbox"] and ran_to_reach(part["trace"])
    else:
        assert part["sum_nbox"] == w["trace"]["nbox"] == part["trace"]["nbox"]
    assert_equal(part, ref, keys)


# -- 1. edge: a 2 x 2 tiling -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo_of", ["handed", "deep"])
@pytest.mark.parametrize("heat", [False, True])
@pytest.mark.parametrize("batch", [1, 256])
@pytest.mark.parametrize("open_axes", ["xyz", "xz"])
def test_edge_two_by_two_tiling(pkg, tables, deep, handed, open_axes, batch, heat, halo_of):
    """W = (20, 10, 20), the source at (15, 5, 16), cut at x = 10|11 and z = 10|11.  D = x 1..10, z 1..10 sees the source 5 cells
    beyond +x and 6 beyond +z: its ghost cells lie in shells >= 5, the fast sweep's.  D takes Bz's strip as face x-high, Bx's as
    face z-high and the edge line along y, which is A's cells x = 1, z = 1, out of either of A's strips.  D's rate grids and
    outgoing columns are W's, bit for bit; sum_nbox is W's rounds."""
    w = deep(W1, SRC1, open_axes, heat)
    t = w["tiling"]
    # precondition, never skipped: W traced more than one round and ran to its reach
    assert w["trace"]["nbox"] > 1 and ran_to_reach(w["trace"])
    assert t.beyond(*D1) == {0: 1, 2: 1}
    if halo_of == "deep":
        d = deep_part(pkg, tables, w, *D1, batch=batch)
        assert sorted(d["halo"]["faces"]) == [X_HIGH, Z_HIGH] and sorted(d["halo"]["edges"]) == [1] and d["halo"]["corner"] is None
    else:
        parts = handed(W1, SRC1, CUTS1, open_axes, heat, batch)
        a, bx, bz, d = parts[(1, 0, 1)], parts[(0, 0, 1)], parts[(1, 0, 0)], parts[(0, 0, 0)]
        assert (d["lo"], d["hi"]) == D1 and sorted(a["strips"]) == [X_LOW, Z_LOW] and sorted(bx["strips"]) == [Z_LOW] and sorted(bz["strips"]) == [X_LOW]
        assert bx["halo"]["faces"].keys() == {X_HIGH} and bz["halo"]["faces"].keys() == {Z_HIGH}
        assert d["halo"]["faces"][X_HIGH] is bz["strips"][X_LOW] and d["halo"]["faces"][Z_HIGH] is bx["strips"][Z_LOW]
        # the edge line: A's x-low strip at A's z = 1, and the same line out of A's z-low strip at x = 1
        line = pkg.handover.edge_of_strip(a["strips"][X_LOW], X_LOW, a["mesh"], Z_LOW)
        assert np.array_equal(d["halo"]["edges"][1], line) and line.shape == (3, 10)
        assert np.array_equal(line, pkg.handover.edge_of_strip(a["strips"][Z_LOW], Z_LOW, a["mesh"], X_LOW))
        # what was handed over is W's: the halo cut from W's own columns
        ref_halo = t.halo_of_deep(w["cols"], *D1)
        for f in (X_HIGH, Z_HIGH):
            assert np.array_equal(d["halo"]["faces"][f], ref_halo["faces"][f]), f
        assert np.array_equal(line, ref_halo["edges"][1])
        for p in (a, bx, bz):          # (the parts upstream of D: W's bits as well)
            check_part(w, p, p["lo"], p["hi"], heat, f"{open_axes} batch {batch} heat {heat} upstream", upstream=True)
    check_part(w, d, *D1, heat, f"{open_axes} batch {batch} heat {heat} {halo_of}")


# -- 2. corner: a 2 x 2 x 2 tiling -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo_of", ["handed", "deep"])
def test_corner_two_by_two_by_two_tiling(pkg, tables, deep, handed, halo_of):
    """W = (16, 16, 16), the source at (12, 11, 13), cut at 8|9 on all three axes.  The part (1..8)^3 takes three strips, three
    edge lines and the corner.  "handed" runs the whole cascade: A -> three one-face parts -> three two-face parts -> the corner
    part, eight contexts of 8^3, and every one of them has W's bits."""
    w = deep(W2, SRC2)
    t = w["tiling"]
    assert w["trace"]["nbox"] > 1 and ran_to_reach(w["trace"])
    assert t.beyond(*D2) == {0: 1, 1: 1, 2: 1}
    if halo_of == "deep":
        d = deep_part(pkg, tables, w, *D2)
    else:
        parts = handed(W2, SRC2, CUTS2)
        assert len(parts) == 8
        d = parts[(0, 0, 0)]
        ref_halo = t.halo_of_deep(w["cols"], *D2)
        for f in (X_HIGH, Y_HIGH, Z_HIGH):
            assert np.array_equal(d["halo"]["faces"][f], ref_halo["faces"][f]), f
        for ax in range(3):
            assert np.array_equal(d["halo"]["edges"][ax], ref_halo["edges"][ax]), ax
        assert np.array_equal(d["halo"]["corner"], ref_halo["corner"])
        for key, p in parts.items():
            if key != (0, 0, 0):
                check_part(w, p, p["lo"], p["hi"], False, f"cascade {key}", upstream=True)
    assert sorted(d["halo"]["faces"]) == [X_HIGH, Y_HIGH, Z_HIGH] and sorted(d["halo"]["edges"]) == [0, 1, 2] and d["halo"]["corner"].shape == (3,)
    check_part(w, d, *D2, False, f"corner {halo_of}")


# -- 3. near ghost cells: the general sweep ----------------------------------------------------------------------------------
def test_near_ghost_cells_through_sweep_cell(pkg, tables, deep):
    """W = (12, 10, 12), the source at (11, 5, 11); the part (10, 10, 10) sees it 1 cell beyond +x and 1 beyond +z: the ghost cells
    lie in shells 0 (the edge line's cell at the source's y: the source's own cell) and 1, which sweep_cell stores, not the
    fast sweep.  (W's reach is 10 cells: one round, to its reach.)"""
    w = deep(W3, SRC3)
    assert w["trace"]["nbox"] == 1 and ran_to_reach(w["trace"])
    assert w["tiling"].beyond(*D3) == {0: 1, 2: 1}
    d = deep_part(pkg, tables, w, *D3)
    check_part(w, d, *D3, False, "near")


_GENERIC_SNIPPET = r'''
import sys, numpy as np
sys.path.insert(0, "{root}"); sys.path.insert(0, "{root}/tests")
import __graft_entry__ as ge
import source_halo_cases as sh
pkg = ge.load_package()
z = np.load("{halo}")
t = sh.Tiling(pkg, {n}, "xyz", "ionised", [{src}], [{flux}])
e = t.engine(pkg, pkg.RadiationTables.load(), {lo}, {hi})
e.set_source_halo(1, faces={{1: z["x_high"], 5: z["z_high"]}}, edges={{1: z["edge_y"]}}, rounds=int(z["rounds"]))
out = sh.collect(e)
out.pop("trace")
np.savez("{out}", **out)
'''


def test_edge_through_the_general_sweep_kernel(pkg, tables, deep, tmp_path):
    """Test 1's deep case with C2R_SWEEP_GENERIC=1 (read once per process, so in a process of its own): k_sweep_shell_halo for
    every shell instead of k_sweep_shell_fast_halo -- the same bits."""
    w = deep(W1, SRC1)
    halo = w["tiling"].halo_of_deep(w["cols"], *D1)
    np.savez(tmp_path / "halo.npz", x_high=halo["faces"][X_HIGH], z_high=halo["faces"][Z_HIGH], edge_y=halo["edges"][1], rounds=w["trace"]["nbox"])
    out = tmp_path / "generic.npz"
    snippet = _GENERIC_SNIPPET.format(root=str(ROOT), halo=str(tmp_path / "halo.npz"), out=str(out), n=W1, src=SRC1, flux=FLUX, lo=D1[0], hi=D1[1])
    r = subprocess.run([sys.executable, "-c", snippet], env={**os.environ, "C2R_SWEEP_GENERIC": "1"}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    assert_equal(got, reference(w, *D1, keys_of(False)), keys_of(False))
    assert int(got["sum_nbox"]) == w["trace"]["nbox"]


# -- 4. zero halo ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part,n,src", [("edge", W1, SRC1), ("corner", W2, SRC2)])
def test_zero_halo_is_the_run_without_halo(pkg, tables, part, n, src):
    """"mixed" gas, the part diagonal to the source: all-zero strips, lines and corner with the rounds of the run without a halo
    give that run's rate grids, bit for bit (the header's ZERO STRIP for several faces); -0.0 is taken as +0.0; cleared, the run
    without a halo again, loss included."""
    t = sh.Tiling(pkg, n, "xyz", "mixed", [src], [FLUX])
    lo, hi = (D1 if part == "edge" else D2)
    e = t.engine(pkg, tables, lo, hi)
    plain = one_pass(e)
    rounds = e.source_trace(1)["nbox"]
    assert rounds >= 1 and e.source_halo(1) == ((), 0) and e.source_face_entry(1) == (-1, 0)
    zero_w = dict(coldensh_out=np.zeros(np.prod(n)), coldenshe_out=np.zeros(2 * np.prod(n)))
    halo = t.halo_of_deep(zero_w, lo, hi)
    for sign in (0.0, -0.0):
        signed = dict(faces={f: s + sign for f, s in halo["faces"].items()}, edges={a: s + sign for a, s in halo["edges"].items()},
                      corner=None if halo["corner"] is None else halo["corner"] + sign)
        sh.set_halo(e, signed, rounds)
        assert e.source_halo(1) == (tuple(sorted(halo["faces"])), rounds)
        zero = one_pass(e)
        assert zero["sum_nbox"] == rounds
        assert_equal(zero, plain, RATES)
    e.set_source_halo(1)
    assert e.source_halo(1) == ((), 0) and e.source_face_entry(1) == (-1, 0)
    again = one_pass(e)
    assert_equal(again, plain, RATES)
    assert again["photon_loss"][0] == plain["photon_loss"][0] and again["sum_nbox"] == plain["sum_nbox"]
    e.close()


# -- 5. one face through the new call ----------------------------------------------------------------------------------------
def test_one_face_halo_is_the_entry(pkg, tables):
    """The unshifted case of tests/test_gpu_source_handover.py, N = (14, 14, 36), the source at (7, 8, 30), B = z 1..20: a halo of
    one face gives the bits of c2r_set_source_face_entry, and both getters report it; the old call on a source that has a halo
    replaces it."""
    n, src = (14, 14, 36), (7, 8, 30)
    st = hc.Stack(pkg, n, "xyz", "ionised", [src], [FLUX])
    e = st.engine(pkg, tables)
    one_pass(e)
    strip, rounds = st.layer_strip(e.download_columns(), 21), e.source_trace(1)["nbox"]
    e.close()
    assert rounds == 3
    keys = RATES + COLS
    e = st.engine(pkg, tables, 1, 20)
    e.set_source_face_entry(1, Z_HIGH, strip, rounds)
    old = sh.collect(e)
    e.set_source_face_entry(1)
    e.set_source_halo(1, faces={Z_HIGH: strip}, rounds=rounds)
    assert e.source_face_entry(1) == (Z_HIGH, rounds) and e.source_halo(1) == ((Z_HIGH,), rounds)
    new = sh.collect(e)
    assert_equal(new, old, keys)
    assert new["sum_nbox"] == old["sum_nbox"] == rounds and new["photon_loss"][0] == old["photon_loss"][0]
    # the old call replaces the halo: another strip, other rounds
    other = np.zeros_like(strip)
    e.set_source_face_entry(1, Z_HIGH, other, 2)
    assert e.source_face_entry(1) == (Z_HIGH, 2) and e.source_halo(1) == ((Z_HIGH,), 2)
    replaced = sh.collect(e)
    e.set_source_halo(1, faces={Z_HIGH: other}, rounds=2)
    same = sh.collect(e)
    assert_equal(same, replaced, keys)
    assert replaced["sum_nbox"] == 2 and not np.array_equal(replaced["phih_grid"], old["phih_grid"])
    e.close()


# -- 6. mixed batch ----------------------------------------------------------------------------------------------------------
MIX_SOURCES = [SRC1, (4, 6, 14), (5, 4, 6)]        # beyond +x and +z of D, beyond +z only, inside D
MIX_FLUX = [FLUX, 1.2e7, 0.9e7]


def test_halo_entry_and_inside_source_in_one_batch(pkg, tables):
    """D of test 1 with three sources in one context: one with a halo, one with a one-face entry, one inside.  The grids of one
    pass are the fold, in source order from 0.0, of the three single-source passes; batch 1 and batch 256 agree."""
    t = sh.Tiling(pkg, W1, "xyz", "ionised", MIX_SOURCES, MIX_FLUX)
    given = []
    for ns in (0, 1):           # W with each outside source alone: its halo and its rounds
        e = t.engine(pkg, tables, sources=[ns])
        one_pass(e)
        tr = e.source_trace(1)
        assert ran_to_reach(tr)
        given.append((t.halo_of_deep(e.download_columns(), *D1, ns=ns), tr["nbox"]))
        e.close()
    assert sorted(given[0][0]["faces"]) == [X_HIGH, Z_HIGH] and sorted(given[1][0]["faces"]) == [Z_HIGH]

    def run(sources, batch):
        e = t.engine(pkg, tables, *D1, sources=sources, batch=batch)
        for at, ns in enumerate(sources):
            if ns == 0:
                sh.set_halo(e, given[0][0], given[0][1], ns=at + 1)
            elif ns == 1:
                e.set_source_face_entry(at + 1, Z_HIGH, given[1][0]["faces"][Z_HIGH], given[1][1])
        r = one_pass(e)
        e.close()
        return r

    singles = [run([ns], 256) for ns in range(3)]
    for batch, ref in ((256, None), (1, None)):
        both = run([0, 1, 2], batch)
        for k in RATES:
            assert np.array_equal(both[k], (singles[0][k] + singles[1][k]) + singles[2][k]), (k, batch)
        assert both["sum_nbox"] == sum(s["sum_nbox"] for s in singles) == given[0][1] + given[1][1] + singles[2]["sum_nbox"]
        assert both["photon_loss"][0] == (singles[0]["photon_loss"][0] + singles[1]["photon_loss"][0]) + singles[2]["photon_loss"][0]
    # another order in the list: the entry source first, the halo source last
    swapped = run([1, 2, 0], 256)
    for k in RATES:
        assert np.array_equal(swapped[k], (singles[1][k] + singles[2][k]) + singles[0][k]), k


# -- 7. kept loss ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo_of", ["handed", "deep"])
def test_kept_loss_is_the_mesh_surface(pkg, tables, deep, handed, halo_of):
    """W of test 1 with every axis open and the escape maps on: D's photon_loss(1) is the sum of W's map entries over the face
    cells of D's outer faces -- x-low, z-low and the two y faces, within D's range --, to 2 n 2^-53 relative: two differently
    associated sums of n non-negative terms, n the number of map cells added."""
    w = deep(W1, SRC1)
    e = w["tiling"].engine(pkg, tables)
    e.enable_face_loss(True)
    one_pass(e)
    assert ran_to_reach(e.source_trace(1))
    # face_loss_map: [b, a] by the two remaining axes, a the lower: x faces [z, y], y faces [z, x], z faces [y, x]
    maps = [e.face_loss_map(X_LOW)[:10, :], e.face_loss_map(Z_LOW)[:, :10], e.face_loss_map(Y_LOW)[:10, :10], e.face_loss_map(Y_HIGH)[:10, :10]]
    e.close()
    n = sum(m.size for m in maps)
    expect = float(sum(float(np.sum(m)) for m in maps))
    d = deep_part(pkg, tables, w, *D1) if halo_of == "deep" else handed(W1, SRC1, CUTS1)[(0, 0, 0)]
    got = float(d["photon_loss"][0])
    tol = 2.0 * n * 2.0 ** -53
    print(halo_of, "kept loss", got, "maps", expect, "rel", abs(got - expect) / expect, "n", n, "tolerance", tol)
    assert n == 10 * 10 + 10 * 10 + 2 * 10 * 10 and expect > 0.0
    assert abs(got - expect) <= tol * expect


# -- 8. refusals and lifetime ------------------------------------------------------------------------------------------------
def _refused(pkg, call, *a, match=None, **kw):
    with pytest.raises(pkg.C2RayHipError, match=match):
        call(*a, **kw)


def test_refusals_and_lifetime(pkg, tables):
    t = sh.Tiling(pkg, W1, "xyz", "ionised", [SRC1, (5, 4, 6)], [FLUX, 0.9e7])
    e = t.engine(pkg, tables, *D1)                  # source 1 beyond +x and +z, source 2 inside
    fx, fz, fy, ey = np.ones((3, 100)), np.ones((3, 100)) * 2.0, np.ones((3, 100)), np.ones((3, 10)) * 3.0
    good = dict(faces={X_HIGH: fx, Z_HIGH: fz}, edges={1: ey}, corner=None, rounds=2)
    e.set_source_halo(1, **good)

    def getters():
        return [e.source_halo(1), e.source_halo(2), e.source_face_entry(1), e.source_face_entry(2)]

    before = getters()
    assert before == [((X_HIGH, Z_HIGH), 2), ((), 0), (X_HIGH, 2), (-1, 0)]
    bits = one_pass(e)

    def with_(**kw):
        return {**good, **kw}

    neg = ey.copy(); neg[1, 3] = -1.0
    nan = fz.copy(); nan[2, 7] = np.nan
    inf = fx.copy(); inf[0, 0] = np.inf
    refusals = [
        (0, good, "source 0 not in"), (3, good, "source 3 not in"),
        (1, with_(rounds=0), "source 1.*rounds"),
        (1, with_(faces={X_HIGH: fx}), r"source 1.*face\[2\] is missing"),
        (1, with_(faces={Z_HIGH: fz}), r"source 1.*face\[0\] is missing"),
        (1, with_(edges={}), r"source 1.*edge\[1\] is missing"),
        (1, with_(faces={X_HIGH: fx, Z_HIGH: fz, Y_HIGH: fy}), r"source 1.*face\[1\] is superfluous"),
        (1, with_(faces={X_HIGH: fx, Z_HIGH: fz, Y_LOW: fy}), r"source 1.*face\[1\] is superfluous"),
        (1, with_(edges={1: ey, 0: np.ones((3, 10))}), r"source 1.*edge\[0\] is superfluous"),
        (1, with_(edges={1: ey, 2: np.ones((3, 10))}), r"source 1.*edge\[2\] is superfluous"),
        (1, with_(corner=np.ones(3)), "source 1.*corner is superfluous"),
        (2, good, "source 2.*inside the mesh"), (2, dict(faces={}, edges={}, corner=None, rounds=2), "source 2.*inside the mesh"),
        (1, with_(edges={1: neg}), r"source 1: edge\[1\]: entry 3 of species 1.*not negative"),
        (1, with_(faces={X_HIGH: fx, Z_HIGH: nan}), r"source 1: face\[2\]: entry 7 of species 2.*finite"),
        (1, with_(faces={X_HIGH: inf, Z_HIGH: fz}), r"source 1: face\[0\]: entry 0 of species 0.*finite"),
    ]
    for ns, kw, match in refusals:
        _refused(pkg, e.set_source_halo, ns, match=match, **kw)
        assert getters() == before, match
        assert_equal(one_pass(e), bits, RATES)
    _refused(pkg, e.source_halo, 3, match="not in")
    # the old call keeps refusing a source beyond two faces, and leaves its halo alone
    for face, strip in ((X_HIGH, fx), (Z_HIGH, fz)):
        _refused(pkg, e.set_source_face_entry, 1, face, strip, 2, match="beyond face")
        assert getters() == before
    assert_equal(one_pass(e), bits, RATES)
    # inside an open slab-wise pass: refused; the slab-wise pass with a halo has the bits of the plain pass
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources_begin(1, 1, 2)
    _refused(pkg, e.set_source_halo, 1, match="still open", **good)
    _refused(pkg, e.set_source_halo, 1, match="still open")
    e.pass_sources_end()
    assert getters() == before
    slabwise = e.download_rates()
    assert_equal(slabwise, bits, RATES)
    assert slabwise["sum_nbox"] == bits["sum_nbox"] and slabwise["photon_loss"][0] == bits["photon_loss"][0]
    # boundaries, beams, horizons keep the halo; a new source list clears it
    e.set_boundaries((False, False, False))
    e.set_source_beams([None, None])
    assert getters() == before
    assert_equal(one_pass(e), bits, RATES)
    src = pkg.SourceProps(t.shifted(D1[0]), t.case.flux, t.case.s_star)
    e.set_sources_external(src)
    assert getters() == [((), 0), ((), 0), (-1, 0), (-1, 0)]
    e.set_source_halo(1, **good)
    assert getters() == before
    e.set_source_halo(1)                    # cleared through the new call ...
    assert getters() == [((), 0), ((), 0), (-1, 0), (-1, 0)]
    e.set_source_halo(1, **good)
    e.set_source_face_entry(1)              # ... and through the old one
    assert getters() == [((), 0), ((), 0), (-1, 0), (-1, 0)]
    e.set_source_halo(1, **good)
    inside = pkg.SourceProps(np.array([[5, 4, 6]], dtype=np.int32), t.case.flux[1:], t.case.s_star)
    e.set_sources(inside)
    assert e.source_halo(1) == ((), 0)
    e.close()
    # a source beyond a corner: the corner is missing
    t3 = sh.Tiling(pkg, W2, "xyz", "ionised", [SRC2], [FLUX])
    e = t3.engine(pkg, tables, *D2)
    s, l = np.ones((3, 64)), np.ones((3, 8))
    whole = dict(faces={X_HIGH: s, Y_HIGH: s, Z_HIGH: s}, edges={0: l, 1: l, 2: l}, rounds=2)
    _refused(pkg, e.set_source_halo, 1, match="source 1.*corner is missing", **whole)
    _refused(pkg, e.set_source_halo, 1, match=r"source 1.*edge\[0\] is missing", **{**whole, "edges": {1: l, 2: l}, "corner": np.ones(3)})
    assert e.source_halo(1) == ((), 0)
    e.set_source_halo(1, corner=np.ones(3), **whole)
    assert e.source_halo(1) == ((X_HIGH, Y_HIGH, Z_HIGH), 2) and e.source_face_entry(1) == (X_HIGH, 2)
    e.close()


def two_device_pass(pkg, tables, devices):
    """D of test 1 with the inside source first and the halo source second, on two devices: device 0 sweeps source 1, device 1
    source 2, which needs the halo there; the summed grids are (0 + a) + (0 + b) of the two single-source passes."""
    t = sh.Tiling(pkg, W1, "xyz", "ionised", [(5, 4, 6), SRC1], [0.9e7, FLUX])
    e = t.engine(pkg, tables, sources=[1])
    one_pass(e)
    halo, rounds = t.halo_of_deep(e.download_columns(), *D1, ns=1), e.source_trace(1)["nbox"]
    e.close()
    singles = []
    for ns in (0, 1):
        e = t.engine(pkg, tables, *D1, sources=[ns])
        if ns == 1:
            sh.set_halo(e, halo, rounds)
        singles.append(one_pass(e))
        e.close()
    hp = pkg.hostphys
    lo, hi = D1
    mesh = tuple(h - l + 1 for l, h in zip(lo, hi))
    ndens, xh, xhe, _ = t.gas(lo, hi)
    mat = pkg.Material(ndens, xh.copy(), xhe.copy(), None, True, 1.0e4, 1.0, t.case.reccoef)
    e = pkg.HipEngine(mesh, devices)
    e.set_boundaries(t.case.periodic)
    e.set_tables(tables)
    e.set_step(mat, pkg.GridProps(mesh, t.case.dr, t.case.vol), pkg.Cosmology(sh.ab.ZRED, hp.H0, hp.Omega0))
    e.set_sources_external(pkg.SourceProps(t.shifted(lo), t.case.flux, t.case.s_star))
    e.upload_state(mat)
    e.comm_init_local()
    assert e.num_devices() == 2
    sh.set_halo(e, halo, rounds, ns=2)
    assert e.source_halo(2) == ((X_HIGH, Z_HIGH), rounds) and e.source_halo(1) == ((), 0)
    e.begin_step()
    e.set_rates_to_zero()
    e.pass_sources(1, 1)
    e.allreduce_rates()
    got = e.download_rates()
    e.close()
    for k in RATES:
        assert np.array_equal(got[k], (0.0 + singles[0][k]) + (0.0 + singles[1][k])), k
    assert got["sum_nbox"] == singles[0]["sum_nbox"] + singles[1]["sum_nbox"]


def test_two_replicas_on_one_device(pkg, tables):
    """c2r_create_multi([0, 0]): the halo reaches both replicas."""
    two_device_pass(pkg, tables, [0, 0])


def test_two_devices(pkg, tables):
    if int(pkg._lib.load().c2r_device_count()) < 2:
        pytest.skip("needs two HIP devices")
    two_device_pass(pkg, tables, [0, 1])
