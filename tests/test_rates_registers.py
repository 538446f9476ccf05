"""The register budget of the isothermal one-SED rates kernels.  Their band loop requests both table gathers of a band
ahead of the species split (band_positions_gathers_first); that the four table values fit rests on the order of a few
statements held in place by empty asm anchors, which another compiler may treat differently.  93 vector registers is
what the kernel had before and has now; from 97 on it loses its fifth wave per SIMD.  No GPU needed: the figures are
in the notes of the gfx950 code object inside the built library."""
import re
import struct
import subprocess
from pathlib import Path

import pytest

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def test_isothermal_one_sed_rates_kernels_stay_within_93_vgprs(pkg, tmp_path):
    if not Path(READELF).exists():
        pytest.skip("llvm-readelf not present")
    blob = Path(pkg.build()).read_bytes()
    at = blob.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert at >= 0, "no offload bundle in the library"
    (count,) = struct.unpack_from("<Q", blob, at + 24)
    pos, device = at + 32, None
    for _ in range(count):
        off, size, tl = struct.unpack_from("<QQQ", blob, pos)
        triple = blob[pos + 24: pos + 24 + tl].decode()
        pos += 24 + tl
        if "gfx950" in triple:
            device = blob[at + off: at + off + size]
    assert device, "no gfx950 code object in the library"
    co = tmp_path / "device.co"
    co.write_bytes(device)
    notes = subprocess.run([READELF, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    # within a kernel's map the keys are sorted: .name < .private_segment_fixed_size < .vgpr_count
    rows = re.findall(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)", notes, flags=re.S)
    iso = {name: (int(seg), int(vgpr)) for name, seg, vgpr in rows if re.search(r"7k_ratesILb0ELb0ELb[01]E", name)}
    assert len(iso) == 2, sorted(n for n, _, _ in rows)
    for name, (seg, vgpr) in iso.items():
        assert seg == 0 and vgpr <= 93, (name, seg, vgpr)
