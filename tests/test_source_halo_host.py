"""Source halos (c2r_set_source_halo) on the CPU.

1. The ghost classification of csrc/c2ray_halo.hpp -- the function the halo sweep kernels run per lane -- compiled for the host
   (tests/halo_harness.cpp) against the NumPy restatement of tests/source_halo_cases.py, with == on every cell of a box that
   reaches 3 cells beyond a (4, 5, 6) mesh, for all 26 placements of the source: class, array and entry index.
2. handover.edge_of_strip / corner_of_strip against slicing a labelled W array.
3. The bindings, and the notes of the gfx950 code object against profiles/source_halo_resources.json.
"""
import ctypes as C
import itertools
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import source_halo_cases as sh
from code_object import READELF, kernel_notes

ROOT = Path(__file__).resolve().parent.parent
MESH, PAD = (4, 5, 6), 3


@pytest.fixture(scope="module")
def hh():
    so = ROOT / "tests" / "_halo_harness.so"
    src = ROOT / "tests" / "halo_harness.cpp"
    hdrs = list((ROOT / "c2-ray3dm1d_helium_amd" / "csrc").glob("*.hpp"))
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in [src] + hdrs):
        r = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(src)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            pytest.fail("tests/halo_harness.cpp does not compile against csrc/c2ray_halo.hpp:\n" + r.stderr[-2000:])
    lib = C.CDLL(str(so))
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    lib.hh_halo_inside.restype = C.c_int
    lib.hh_ghost_index.restype = C.c_int
    lib.hh_ghost_index.argtypes = [C.c_int, C.c_int]
    lib.hh_classify_box.restype = None
    lib.hh_classify_box.argtypes = [ip, ip, C.c_int, ip, ip, lp, lp]
    return lib


def box_indices():
    """0-based mesh indices (i, j, k) of every cell of the padded box, x fastest, as (z, y, x) arrays."""
    ax = [np.arange(-PAD, n + PAD, dtype=np.int64) for n in MESH]
    k, j, i = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return i, j, k


def header_box(hh, srcpos):
    shape = tuple(n + 2 * PAD for n in MESH)[::-1]
    cells = int(np.prod(shape))
    cls, arr = np.full(cells, -9, dtype=np.int32), np.full(cells, -9, dtype=np.int32)
    ent, strd = np.full(cells, -9, dtype=np.int64), np.full(cells, -9, dtype=np.int64)
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    hh.hh_classify_box((C.c_int * 3)(*MESH), (C.c_int * 3)(*srcpos), PAD, cls.ctypes.data_as(ip), arr.ctypes.data_as(ip),
                       ent.ctypes.data_as(lp), strd.ctypes.data_as(lp))
    return [a.reshape(shape) for a in (cls, arr, ent, strd)]


PLACEMENTS = [p for p in itertools.product((-1, 0, 1), repeat=3) if any(p)]


def position(placement, dist):
    """A source `dist` cells beyond the low (-1) or high (+1) face along each axis of the placement, inside (0) elsewhere."""
    inside = (2, 4, 3)
    return tuple(inside[d] if s == 0 else (MESH[d] + dist if s > 0 else 1 - dist) for d, s in enumerate(placement))


def test_there_are_26_placements():
    assert len(PLACEMENTS) == 26 and sorted(sum(1 for s in p if s) for p in PLACEMENTS).count(1) == 6
    assert sum(1 for p in PLACEMENTS if sum(1 for s in p if s) == 2) == 12 and sum(1 for p in PLACEMENTS if all(p)) == 8


@pytest.mark.parametrize("placement", PLACEMENTS, ids=lambda p: "".join("-0+"[s + 1] for s in p))
def test_ghost_classification_equals_the_restatement(hh, placement):
    i, j, k = box_indices()
    outside = (i < 0) | (i >= MESH[0]) | (j < 0) | (j >= MESH[1]) | (k < 0) | (k >= MESH[2])
    nb = sum(1 for s in placement if s)
    for dist in (1, 2, 7):
        srcpos = position(placement, dist)
        for d in range(3):
            want = hh.hh_halo_inside() if placement[d] == 0 else (MESH[d] if placement[d] > 0 else -1)
            assert hh.hh_ghost_index(srcpos[d], MESH[d]) == want
        cls, arr, ent, strd = header_box(hh, srcpos)
        assert np.all(cls[~outside] == -2)                         # (cells of the mesh: never asked)
        w_cls, w_arr, w_ent, w_strd = sh.classify(MESH, srcpos, i[outside], j[outside], k[outside])
        assert np.array_equal(cls[outside], w_cls)
        ghost = w_cls > 0
        for got, want in ((arr, w_arr), (ent, w_ent), (strd, w_strd)):
            assert np.array_equal(got[outside][ghost], want[ghost])
        # every array of a whole halo is covered exactly: each entry of each array by one ghost cell
        expect = {}
        for d in range(3):
            a, b = [c for c in range(3) if c != d]
            if placement[d]:
                expect[d] = MESH[a] * MESH[b]
            if placement[a] and placement[b]:
                expect[3 + d] = MESH[d]
        if nb == 3:
            expect[6] = 1
        seen = {int(a): np.sort(w_ent[ghost & (w_arr == a)]) for a in np.unique(w_arr[ghost])}
        assert sorted(seen) == sorted(expect)
        for a, count in expect.items():
            assert np.array_equal(seen[a], np.arange(count)), (a, count)
        assert int(ghost.sum()) == sum(expect.values())
        print(placement, dist, "ghost cells", int(ghost.sum()), "vacuum", int((~ghost).sum()), "arrays", sorted(expect))


# -- the helper module --------------------------------------------------------------------------------------------------------
def labelled(mesh):
    """(3, z, y, x): species s of cell (x, y, z) (1-based) holds s * 10^6 + x * 10^4 + y * 10^2 + z."""
    z, y, x = np.meshgrid(*[np.arange(1, n + 1) for n in mesh[::-1]], indexing="ij")
    return np.stack([s * 1.0e6 + x * 1.0e4 + y * 1.0e2 + z for s in range(3)])


def strip_of(w, face):
    axis, high = face >> 1, face & 1
    at = w.shape[3 - axis] - 1 if high else 0
    return np.take(w, at, axis=3 - axis).reshape(3, -1)            # (z, y, x) without the face's axis: the lower axis fastest


def test_edge_and_corner_of_a_labelled_strip(pkg):
    ho = pkg.handover
    mesh = (4, 5, 6)
    w = labelled(mesh)
    for face in range(6):
        axis = face >> 1
        strip = strip_of(w, face)
        at = {axis: mesh[axis] if face & 1 else 1}
        grid, (a, b) = ho.strip_grid(strip, face, mesh)
        assert (a, b) == tuple(d for d in range(3) if d != axis) and grid.shape == (3, mesh[b], mesh[a])
        for other in range(6):
            if other >> 1 == axis:
                with pytest.raises(ValueError):
                    ho.edge_of_strip(strip, face, mesh, other)
                continue
            oaxis = other >> 1
            at2 = dict(at)
            at2[oaxis] = mesh[oaxis] if other & 1 else 1
            e = 3 - axis - oaxis
            line = ho.edge_of_strip(strip, face, mesh, other)
            want = np.stack([s * 1.0e6 + sum(10.0 ** (4 - 2 * d) * (at2[d] if d in at2 else np.arange(1, mesh[e] + 1)) for d in range(3))
                             for s in range(3)])
            assert line.shape == (3, mesh[e]) and np.array_equal(line, want), (face, other)
            # the same line out of the other face's strip
            assert np.array_equal(line, ho.edge_of_strip(strip_of(w, other), other, mesh, face))
            for third in (2 * e, 2 * e + 1):
                at3 = dict(at2)
                at3[e] = mesh[e] if third & 1 else 1
                want = np.array([s * 1.0e6 + at3[0] * 1.0e4 + at3[1] * 1.0e2 + at3[2] for s in range(3)])
                assert np.array_equal(ho.corner_of_strip(strip, face, mesh, other, third), want)
                assert np.array_equal(ho.corner_of_strip(strip, face, mesh, third, other), want)
        with pytest.raises(ValueError):
            ho.corner_of_strip(strip, face, mesh, (face + 2) % 6, (face + 2) % 6 ^ 1)
        with pytest.raises(ValueError):
            ho.edge_of_strip(strip[:, 1:], face, mesh, (face + 2) % 6)


# -- the bindings and the code object ------------------------------------------------------------------------------------------
def test_bindings_have_the_two_calls(pkg):
    assert hasattr(pkg.HipEngine, "set_source_halo") and hasattr(pkg.HipEngine, "source_halo")
    assert "c2r_set_source_halo" in pkg._lib.SYMBOLS and "c2r_get_source_halo" in pkg._lib.SYMBOLS
    assert C.sizeof(pkg._lib.SourceHalo) == 8 + 7 * 8
    f = (ROOT / "c2-ray3dm1d_helium_amd" / "fortran" / "c2ray_hip_binding.f90").read_text()
    assert 'bind(C, name="c2r_set_source_halo")' in f and 'bind(C, name="c2r_get_source_halo")' in f
    h = (ROOT / "include" / "c2ray_hip.h").read_text()
    assert "int c2r_set_source_halo(c2r_ctx *ctx, int ns, const c2r_source_halo *halo);" in h
    assert "int c2r_get_source_halo(c2r_ctx *ctx, int ns, int faces[3], int *rounds);" in h


def test_sweep_and_loss_kernels_in_the_code_object(pkg):
    """profiles/source_halo_resources.json: the two halo kernels have no private segment and no more vector registers than
    their entry twins (the same occupancy class); the entry kernels keep the parent's vector registers, LDS and empty private
    segment; 'after' is what the library holds."""
    if not Path(READELF).exists():
        pytest.skip("llvm-readelf not present")
    notes = kernel_notes(pkg.build())
    rec = json.loads((ROOT / "profiles" / "source_halo_resources.json").read_text())
    keys = ("vgpr", "agpr", "sgpr", "private_segment", "lds")
    names = ("k_sweep_shell_entry", "k_sweep_shell_fast_entry", "k_loss_entry", "k_sweep_shell_halo", "k_sweep_shell_fast_halo")

    def find(table, name):
        hit = [v for v in table.values() if f"{len(name)}{name}E" in v["mangled"]]
        assert len(hit) == 1, (name, sorted(table))
        return hit[0]

    built = {n: find({m: dict(v, mangled=m) for m, v in notes.items()}, n) for n in names}
    for n in names:
        print(n, {k: built[n][k] for k in keys})
        assert built[n]["private_segment"] == 0, n
        assert {k: find(rec["after"], n)[k] for k in keys} == {k: built[n][k] for k in keys}, n
    for n in names[:3]:
        before = find(rec["before"], n)
        for k in ("vgpr", "agpr", "private_segment", "lds"):
            assert built[n][k] == before[k], (n, k)
    for halo, twin in (("k_sweep_shell_halo", "k_sweep_shell_entry"), ("k_sweep_shell_fast_halo", "k_sweep_shell_fast_entry")):
        assert built[halo]["vgpr"] + built[halo]["agpr"] <= built[twin]["vgpr"] + built[twin]["agpr"], (halo, built[halo], built[twin])
    assert not any("halo" in v["mangled"] for v in rec["before"].values())
