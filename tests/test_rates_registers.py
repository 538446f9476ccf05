"""The register budget of the isothermal one-SED rates kernels.  Their band loop requests both table gathers of a band
ahead of the species split (band_positions_gathers_first); that the four table values fit rests on the order of a few
statements held in place by empty asm anchors, which another compiler may treat differently.  93 vector registers is
what the kernel had before and has now; from 97 on it loses its fifth wave per SIMD.  No GPU needed: the figures are
in the notes of the gfx950 code object inside the built library."""
import re
from pathlib import Path

import pytest

from code_object import READELF, kernel_notes


def test_isothermal_one_sed_rates_kernels_stay_within_93_vgprs(pkg):
    if not Path(READELF).exists():
        pytest.skip("llvm-readelf not present")
    notes = kernel_notes(pkg.build())
    iso = {name: (v["private_segment"], v["vgpr"]) for name, v in notes.items() if re.search(r"7k_ratesILb0ELb0ELb[01]E", name)}
    assert len(iso) == 2, sorted(notes)
    for name, (seg, vgpr) in iso.items():
        assert seg == 0 and vgpr <= 93, (name, seg, vgpr)
