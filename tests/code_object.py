"""The gfx950 code object inside the built library, for the tests that check what the compiler made of a kernel: no GPU
needed, the figures are in the code object's metadata notes (tools/kernel_resources.py prints the same table)."""
import re
import struct
import subprocess
import tempfile
from pathlib import Path

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def kernel_notes(lib):
    """{mangled kernel name: {vgpr, agpr, sgpr, private_segment, lds}} of every kernel in the library `lib`."""
    blob = Path(lib).read_bytes()
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
    with tempfile.TemporaryDirectory() as d:
        co = Path(d) / "device.co"
        co.write_bytes(device)
        notes = subprocess.run([READELF, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    out = {}
    for t in re.split(r"\n  - (?=\.agpr_count:)", notes)[1:]:
        g = lambda k: re.search(rf"\.{k}:\s+(\S+)", t).group(1)
        out[g("name")] = dict(vgpr=int(g("vgpr_count")), agpr=int(g("agpr_count")), sgpr=int(g("sgpr_count")),
                              private_segment=int(g("private_segment_fixed_size")), lds=int(g("group_segment_fixed_size")))
    return out
