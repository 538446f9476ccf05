"""The C-ABI library loads and exports every symbol include/c2ray_hip.h declares; without a GPU it
refuses to create a context (there is no CPU path)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from code_object import READELF, kernel_notes

ROOT = Path(__file__).resolve().parent.parent


def declared_symbols():
    text = (ROOT / "include" / "c2ray_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(c2r_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree(pkg):
    assert declared_symbols() == sorted(pkg._lib.SYMBOLS)


def test_fortran_binding_covers_the_header():
    """fortran/c2ray_hip_binding.f90 -- the iso_c_binding view a Fortran host compiles -- binds every entry point the
    header declares, and nothing else."""
    f = (ROOT / "c2-ray3dm1d_helium_amd" / "fortran" / "c2ray_hip_binding.f90").read_text()
    bound = sorted(set(re.findall(r'name="(c2r_[a-z0-9_]+)"', f)))
    assert bound == declared_symbols()


def test_library_exports_every_declared_symbol(pkg):
    lib = C.CDLL(str(pkg.build()))
    for name in declared_symbols():
        assert hasattr(lib, name), name


def test_no_device_fails_loudly(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.C2RayHipError, match="no HIP device|no CPU path"):
        pkg.HipEngine((16, 16, 16))


def test_product_does_not_touch_the_oracle():
    """Nothing under the package may import, link or name the oracle."""
    for p in (ROOT / "c2-ray3dm1d_helium_amd").rglob("*"):
        if p.suffix in {".py", ".hip", ".hpp", ".inc", ".h", ".F90", ".f90"}:
            t = p.read_text()
            assert "liboracle" not in t and "import oracle" not in t and "c2ray_oracle" not in t, p


def test_hot_kernels_keep_nothing_in_scratch_memory(pkg):
    """The gfx950 code object inside the built library: the kernels of the hot path have no private segment.  (Round 3
    found 12 bytes of it in the sweep kernel -- three offsets assigned through a pointer the compiler selected at run
    time -- that a register census reports as "0 spills" and that cost 5 % of the sweep.)"""
    if not Path(READELF).exists():
        pytest.skip("llvm-readelf not present")
    seg = {name: v["private_segment"] for name, v in kernel_notes(pkg.build()).items()}
    hot = [n for n in seg if re.search(r"k_sweep_shell|k_chemistry|k_loss|k_pack_state|k_transpose_packed|7k_ratesILb[01]ELb[01]E", n)]
    assert len(hot) >= 12, sorted(seg)
    assert {n: seg[n] for n in hot if seg[n]} == {}


def test_no_null_stream_fills_outside_context_creation():
    """hipMemset / hipMemcpy without a stream run on the null stream, which is ordered with nothing on the library's
    non-blocking streams: a fill issued lazily, next to launches, can land after them (round 3: the deferred-cell
    counters of the heating tiers).  Such calls may only appear where a device-wide synchronisation follows before
    any launch (c2r_create) or where the call itself blocks the host on data the host owns (hipMemcpy)."""
    src = (ROOT / "c2-ray3dm1d_helium_amd" / "csrc" / "c2ray_hip.hip").read_text()
    start = src.index('extern "C" int c2r_create(')
    end = src.index('extern "C" void c2r_destroy(')
    outside = src[:start] + src[end:]
    assert "hipMemset(" not in outside
    for inc in ("c2ray_comm.inc", "c2ray_planes.inc"):
        assert "hipMemset(" not in (ROOT / "c2-ray3dm1d_helium_amd" / "csrc" / inc).read_text()
    # inside c2r_create the fills are followed by a device synchronisation
    create = src[start:end]
    assert create.rindex("hipDeviceSynchronize()") > create.rindex("hipMemset(")


def test_no_allocation_inside_a_global_pass():
    """Round 3 allocated the chemistry counters and the heating tiers' lists inside the first global pass: a hipMalloc is a
    device-wide synchronisation in the middle of an iteration that has exactly one.  They now come from c2r_create and
    c2r_set_step; the check a pass makes must not allocate."""
    src = (ROOT / "c2-ray3dm1d_helium_amd" / "csrc" / "c2ray_hip.hip").read_text()
    start = src.index("static int ensure_chemistry_buffers(")
    body = src[start:src.index("\n}\n", start)]
    assert "hipMalloc" not in body and "hipMemset" not in body
    for fn in ("static int launch_chemistry(", 'extern "C" int c2r_global_pass_cells(', 'extern "C" int c2r_global_pass_finish('):
        a = src.index(fn)
        assert "hipMalloc" not in src[a:src.index("\n}\n", a)], fn
