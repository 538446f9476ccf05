"""Side faces of a tilted plane (c2r_set_plane_side_entry, c2r_enable_plane_side_exit, c2r_enable_plane_side_loss) on the CPU:
the reference of tests/plane_side_reference.py against the references it extends, its own tiling identity, the flux budget
that the side weights close, the attribution of the diagonal weight, and the product's weight rule (csrc/c2ray_pside.hpp)
compiled for the host against the reference's.  No GPU is needed.
"""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import flux_reference as fr
import oblique_reference as obr
import plane_side_reference as psr
from test_oblique_reference_host import make_slab

ROOT = Path(__file__).resolve().parent.parent
OPEN = (False, False, False)
SIGNS = [(1, 1), (1, -1), (-1, 1), (-1, -1)]
MESH = (7, 6, 4)
FLUX = 3.0e-41


@pytest.fixture(scope="module")
def slab(pkg):
    return make_slab(pkg, MESH, 4711, (1.0, 1.25, 0.8))


def make_map(mesh, axis, seed):
    f_ax, g_ax = psr.face_axes(axis)
    rng = np.random.default_rng(seed)
    m = np.zeros((3, mesh[g_ax], mesh[f_ax]))
    m[0] = FLUX * rng.uniform(0.3, 2.0, m[0].shape)
    m[:, 1, 2] = 0.0
    return m.reshape(3, -1)


def run_ref(orc, otables, slab, mesh, axis, from_high, tilt, fmap, **kw):
    (ndens, xh_av, xhe_av), dr, vol = slab
    return psr.side_pass(orc, otables, mesh, dr, vol, ndens, xh_av, xhe_av, axis, from_high, tilt, flux_map=fmap, **kw)


@pytest.mark.parametrize("axis,from_high,periodic", [(2, 0, OPEN), (0, 1, OPEN), (1, 0, (True, False, False))])
def test_without_strips_it_is_flux_pass(orc, otables, slab, axis, from_high, periodic):
    """No ghost strips: every output flux_pass has, bit for bit."""
    (ndens, xh_av, xhe_av), dr, vol = slab
    tilt = (0.35, -0.6)
    fmap = make_map(MESH, axis, 5)
    want = fr.flux_pass(orc, otables, MESH, dr, vol, ndens, xh_av, xhe_av, axis, from_high, fmap, tilt=tilt, periodic=periodic)
    got = run_ref(orc, otables, slab, MESH, axis, from_high, tilt, fmap, periodic=periodic)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert got["loss"] > 0


def test_uniform_without_strips_is_oblique_pass(orc, otables, slab):
    (ndens, xh_av, xhe_av), dr, vol = slab
    want = obr.oblique_pass(orc, otables, MESH, dr, vol, ndens, xh_av, xhe_av, 2, 0, FLUX, (0.35, -0.6))
    got = psr.side_pass(orc, otables, MESH, dr, vol, ndens, xh_av, xhe_av, 2, 0, (0.35, -0.6), normflux=FLUX)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert got["side_flux"] == [None, None] and got["side_cols"][0].shape == (4, 3, 6) and got["side_cols"][1].shape == (4, 3, 7)


@pytest.mark.parametrize("e_f,e_g", SIGNS)
def test_two_by_two_tiles_equal_one_mesh(orc, otables, slab, e_f, e_g):
    """The reference's own tiling identity: (7,6,4) along z cut at x = 3 and y = 4, the four tiles run from upstream to
    downstream with their neighbours' strips, against the one mesh -- rate grids, incoming columns, exit columns, exit flux,
    far-face terms, and the strips of the tiles on the combined mesh's downstream edges, all exactly."""
    (ndens, xh_av, xhe_av), dr, vol = slab
    tilt = (0.35 * e_f, 0.6 * e_g)
    fmap = make_map(MESH, 2, 7)
    whole = run_ref(orc, otables, slab, MESH, 2, 0, tilt, fmap)

    def run(lo, hi, ghost):
        sub = ((psr.box_field(MESH, lo, hi, ndens), psr.box_field(MESH, lo, hi, xh_av), psr.box_field(MESH, lo, hi, xhe_av)), dr, vol)
        mesh = tuple(hi[d] - lo[d] for d in range(3))
        return run_ref(orc, otables, sub, mesh, 2, 0, tilt, psr.box_face(MESH, 2, lo, hi, fmap), ghost=ghost)
    tiles = psr.tiled(MESH, 2, tilt, 3, 4, run)
    assert len(tiles) == 4
    for lo, hi, got in tiles.values():
        for k in ("phih_grid", "phihe_grid", "cin_HI"):
            assert np.array_equal(got[k], psr.box_field(MESH, lo, hi, whole[k])), (k, lo)
        for k in ("exit", "exit_flux", "terms"):
            assert np.array_equal(got[k], psr.box_face(MESH, 2, lo, hi, whole[k])), (k, lo)
    # the far tile's strips are the whole mesh's, cropped
    lo, hi, far = tiles[(1 if e_f > 0 else 0, 1 if e_g > 0 else 0)]
    assert np.array_equal(far["side_cols"][0], whole["side_cols"][0][:, :, lo[1]:hi[1]])
    assert np.array_equal(far["side_flux"][1], whole["side_flux"][1][:, :, lo[0]:hi[0]])
    assert np.array_equal(far["side_terms"][0].reshape(4, hi[1] - lo[1]), whole["side_terms"][0].reshape(4, 6)[:, lo[1]:hi[1]])


@pytest.mark.parametrize("periodic", [OPEN, (True, False, False), (False, True, False)])
@pytest.mark.parametrize("e_f,e_g", SIGNS)
def test_flux_budget(e_f, e_g, periodic):
    """rates=False: the last layer's flux, plus what the layers m <= na-2 give to the sides by the weights, is the flux of
    layer 0, to 8 na 2^-52 relative (every layer's redistribution is four rounded products and three sums, with weights that add
    to 1 within 2 ulp).  All sums by math.fsum."""
    mesh, na = (9, 7, 6), 6
    dr = (1.0, 1.25, 0.8)
    tilt = (0.35 * e_f, 0.6 * e_g)
    rng = np.random.default_rng(17)
    fmap = rng.uniform(0.3, 2.0, (3, 63))
    r = psr.side_pass(None, None, mesh, dr, 1.0, None, None, None, 2, 0, tilt, flux_map=fmap, periodic=periodic, rates=False)
    lay, w = r["layer_flux"], r["weights"]
    for k in range(3):
        lost = [float(w[s_, f]) * float(lay[m, k, f]) for m in range(na - 1) for s_ in range(2) for f in range(63)]
        total = math.fsum([float(x) for x in lay[na - 1, k]] + lost)
        first = math.fsum(float(x) for x in lay[0, k])
        print("SED", k, "budget", total, "layer 0", first, "rel", abs(total - first) / first)
        assert abs(total - first) <= 8 * na * 2.0 ** -52 * first
    assert (w[0].any(), w[1].any()) == (not periodic[0], not periodic[1])


@pytest.mark.parametrize("periodic", [OPEN, (True, False, False)])
@pytest.mark.parametrize("e_f,e_g", SIGNS)
def test_attribution_of_the_diagonal_weight(e_f, e_g, periodic):
    """On the corner cell of the two downstream edges side 0 takes s3 + s1 and side 1 keeps s2 alone; elsewhere on side 1's edge
    w_1 = s2 + s1; with the f axis periodic no target is outside along f, and side 1 has s2 + s1 on its whole edge."""
    fa, fb = 5, 4
    s = obr.geometry((0.35 * e_f, 0.6 * e_g), (1.0, 1.25, 0.8), 2)[2]
    wrap_f = bool(periodic[0])
    eu, ev = psr.downstream_edge(e_f, fa), psr.downstream_edge(e_g, fb)
    for v in range(fb):
        for u in range(fa):
            w0, w1 = psr.side_weights(s, e_f, e_g, fa, fb, wrap_f, False, u, v)
            want0 = s[2] + s[0] if u == eu and not wrap_f else 0.0
            want1 = 0.0 if v != ev else (s[1] if u == eu and not wrap_f else s[1] + s[0])
            assert (w0, w1) == (want0, want1), (u, v)
    # the displaced weights of the corner cell that leave the mesh (all three on an open mesh; s3 wraps where f is periodic):
    # nothing is counted twice, nothing dropped
    w0, w1 = psr.side_weights(s, e_f, e_g, fa, fb, wrap_f, False, eu, ev)
    assert abs((w0 + w1) - (s[0] + s[1] + (0.0 if wrap_f else s[2]))) <= 2.0 ** -52


@pytest.fixture(scope="module")
def ps(tmp_path_factory):
    """csrc/c2ray_pside.hpp compiled for the host."""
    d = tmp_path_factory.mktemp("pside")
    src = d / "pside_harness.cpp"
    src.write_text('#include "c2ray_pside.hpp"\n'
                   'extern "C" void ps_weights(const double *tilt, const double *dr, int axis, const int *per, int fa, int fb, int u, int v,\n'
                   '                           double *w, int *info) {\n'
                   '  const c2r::PlaneTilt T(tilt, dr, axis, per);\n'
                   '  c2r::pside_weights(T, fa, fb, u, v, w[0], w[1]);\n'
                   '  info[0] = c2r::pside_edge(T.e_f, fa); info[1] = c2r::pside_edge(T.e_g, fb);\n'
                   '  info[2] = c2r::pside_face(axis == 0 ? 1 : 0, T.e_f); info[3] = c2r::pside_face(axis == 2 ? 1 : 2, T.e_g);\n'
                   '  info[4] = c2r::pside_live(tilt[0], T.wrap_f); info[5] = c2r::pside_live(tilt[1], T.wrap_g);\n'
                   '}\n')
    so = d / "pside_harness.so"
    r = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-std=c++17", "-fPIC", "-shared", "-I", str(ROOT / "c2-ray3dm1d_helium_amd" / "csrc"),
                        "-o", str(so), str(src)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("csrc/c2ray_pside.hpp does not compile for the host:\n" + r.stderr[-2000:])
    return C.CDLL(str(so))


@pytest.mark.parametrize("axis,periodic", [(a, p) for a in range(3) for p in (OPEN, (True, False, False), (False, False, True)) if not p[a]])
@pytest.mark.parametrize("e_f,e_g", SIGNS)
def test_the_products_weights_are_the_references(ps, axis, periodic, e_f, e_g):
    """pside_weights, pside_edge, pside_face and pside_live of the product against the reference, every cell of a 5 x 4 face
    (the plane's own axis is open)."""
    fa, fb = 5, 4
    tilt, dr = (0.35 * e_f, 0.6 * e_g), (1.0, 1.25, 0.8)
    f_ax, g_ax = psr.face_axes(axis)
    s = obr.geometry(tilt, dr, axis)[2]
    w, info = (C.c_double * 2)(), (C.c_int * 6)()
    for v in range(fb):
        for u in range(fa):
            ps.ps_weights((C.c_double * 2)(*tilt), (C.c_double * 3)(*dr), axis, (C.c_int * 3)(*[int(b) for b in periodic]), fa, fb, u, v, w, info)
            assert (w[0], w[1]) == psr.side_weights(s, e_f, e_g, fa, fb, bool(periodic[f_ax]), bool(periodic[g_ax]), u, v), (u, v)
    assert (info[0], info[1]) == (psr.downstream_edge(e_f, fa), psr.downstream_edge(e_g, fb))
    assert (info[2], info[3]) == (psr.side_face(axis, 0, e_f), psr.side_face(axis, 1, e_g))
    assert (bool(info[4]), bool(info[5])) == psr.live_sides(tilt, periodic, axis)
