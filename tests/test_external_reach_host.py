"""Host checks of what c2r_set_sources_external adds to csrc/c2ray_shell.hpp (no GPU): the reach of a source that may stand
outside the mesh, the sweep's in-mesh predicate, the two size limits, and the cut shell order on such a reach.
tests/external_reach_harness.cpp compiles the header for the host."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
I3 = C.c_int * 3


@pytest.fixture(scope="module")
def xr():
    so, src = ROOT / "tests" / "_external_reach_harness.so", ROOT / "tests" / "external_reach_harness.cpp"
    hdrs = list((ROOT / "c2-ray3dm1d_helium_amd" / "csrc").glob("*.hpp"))
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(src)], check=True)
    lib = C.CDLL(str(so))
    lib.xr_reach_cells.restype = C.c_longlong
    lib.xr_reach_position.restype = C.c_longlong
    return lib


def reach(xr, fn, mesh, pos, periodic, max_subbox):
    lr = (C.c_int * 2)()
    getattr(xr, fn)(mesh, pos, periodic, max_subbox, lr)
    return lr[0], lr[1]


@pytest.mark.parametrize("max_subbox", [3, 1150])
def test_reach_of_every_position(xr, max_subbox):
    """Every mesh length <= 9, every position from -6 to mesh + 6: l <= 0 <= r; the rule of include/c2ray_hip.h; axis_reach's
    numbers for a position inside and on a periodic axis."""
    for mesh in range(1, 10):
        for pos in range(-6, mesh + 7):
            l, r = reach(xr, "xr_axis_reach_external", mesh, pos, 0, max_subbox)
            assert l <= 0 <= r
            assert (l, r) == (-min(max_subbox, max(pos - 1, 0)), min(max_subbox, max(mesh - pos, 0)))
            if 1 <= pos <= mesh:
                assert (l, r) == reach(xr, "xr_axis_reach", mesh, pos, 0, max_subbox)
                assert reach(xr, "xr_axis_reach_external", mesh, pos, 1, max_subbox) == reach(xr, "xr_axis_reach", mesh, pos, 1, max_subbox)
            else:   # the whole mesh lies on one side: the far face is pos - 1 or mesh - pos cells away
                assert l == 0 or r == 0
                assert max(-l, r) == min(max_subbox, pos - 1 if pos > mesh else mesh - pos)


@pytest.mark.parametrize("max_subbox", [3, 1150])
def test_in_mesh_predicate(xr, max_subbox):
    """The sweep's test -- wrap, then one unsigned compare -- against 1 <= pos + off <= mesh for every offset within the reach;
    a periodic axis never fails it."""
    for mesh in range(1, 10):
        for pos in range(-6, mesh + 7):
            l, r = reach(xr, "xr_axis_reach_external", mesh, pos, 0, max_subbox)
            inside = 0
            for off in range(l, r + 1):
                want = 1 <= pos + off <= mesh
                assert bool(xr.xr_in_mesh(mesh, pos, off, 0)) == want, (mesh, pos, off)
                inside += want
            if 1 <= pos <= mesh:
                assert inside == r - l + 1                       # a source inside has no vacuum cell
            elif max_subbox >= 15:
                assert inside == mesh                            # the reach ends at the far face: every mesh cell, once
        for pos in range(1, mesh + 1):
            l, r = reach(xr, "xr_axis_reach_external", mesh, pos, 1, max_subbox)
            assert all(xr.xr_in_mesh(mesh, pos, off, 1) for off in range(l, r + 1))


def test_size_limits(xr):
    """max(|l_d|, r_d) > 4096 -> 1; prod_d (r_d - l_d + 1) >= 2^31 -> 2; else 0.  (With max_subbox = 1150, the reference's
    value, the library clamps every reach at 1150 cells, so no list reaches the first limit through the C ABI: it is held to
    the rule here.  The second is reached on a thin, long mesh -- (2, 2, 1700) below -- and tests/test_gpu_external_sources.py
    meets it through the ABI as well.)"""
    assert xr.xr_refusal(I3(0, 0, 0), I3(4096, 0, 0)) == 0
    assert xr.xr_refusal(I3(0, 0, 0), I3(4097, 0, 0)) == 1
    assert xr.xr_refusal(I3(0, -4097, 0), I3(0, 0, 0)) == 1
    assert xr.xr_refusal(I3(-4096, -4096, -4096), I3(0, 0, 0)) == 2          # 4097^3 > 2^31
    assert xr.xr_refusal(I3(0, 0, 0), I3(2047, 1023, 1023)) == 2             # 2^31 exactly
    assert xr.xr_refusal(I3(0, 0, -1), I3(2047, 1023, 1021)) == 0            # 2^31 - 2^21
    assert xr.xr_refusal(I3(-1150, 0, 0), I3(0, 1150, 1150)) == 0            # 1151^3: outside along all three axes
    assert xr.xr_refusal(I3(0, 0, -849), I3(1150, 1150, 850)) == 2           # (2,2,1700), a source at (-1148,-1148,850)
    assert xr.xr_refusal(I3(0, 0, -849), I3(1150, 1, 850)) == 0              # ... at (-1149,1,850)


OUTSIDE = [  # (mesh, position): outside along one, two and three axes, low and high sides
    ((5, 4, 6), (8, 2, 3)), ((5, 4, 6), (3, -2, 3)), ((5, 4, 6), (0, 2, 9)), ((5, 4, 6), (7, 6, 1)),
    ((5, 4, 6), (-1, -3, 8)), ((4, 4, 4), (7, 7, 7)), ((3, 7, 2), (2, 4, -4)),
]


@pytest.mark.parametrize("mesh,pos", OUTSIDE)
def test_shell_order_is_a_bijection_on_the_virtual_reach(xr, mesh, pos):
    """reach_decode / reach_position on the reach of a source outside the mesh: the shells 0..smax list every cell of the box
    [l, r] exactly once, at consecutive positions from 0, and reach_position inverts the list."""
    lr = [reach(xr, "xr_axis_reach_external", m, p, 0, 1150) for m, p in zip(mesh, pos)]
    l, r = I3(*[a for a, _ in lr]), I3(*[b for _, b in lr])
    smax = max(max(-a, b) for a, b in lr)
    seen, at = {}, 0
    out = (C.c_int * 4)()
    for s in range(smax + 1):
        assert xr.xr_reach_cells(l, r, s - 1) == at
        cnt = xr.xr_reach_decode(l, r, s, -1, out)
        for t in range(cnt):
            xr.xr_reach_decode(l, r, s, t, out)
            cell = (out[0], out[1], out[2])
            assert max(abs(x) for x in cell) == s and all(a <= x <= b for x, (a, b) in zip(cell, lr))
            assert cell not in seen
            seen[cell] = at + t
            assert xr.xr_reach_position(l, r, *cell) == at + t
        at += cnt
    box = set(itertools.product(*[range(a, b + 1) for a, b in lr]))
    assert set(seen) == box and at == len(box) == xr.xr_reach_cells(l, r, smax)
    # the mesh cells of the box: those that pass the predicate on every axis, mesh_d of them per axis
    in_mesh = [c for c in box if all(xr.xr_in_mesh(m, p, o, 0) for m, p, o in zip(mesh, pos, c))]
    assert len(in_mesh) == mesh[0] * mesh[1] * mesh[2]
