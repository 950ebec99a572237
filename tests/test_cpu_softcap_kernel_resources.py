"""The soft-cap kernels (include/qattn_softcap.h) add 32 tanh evaluations per lane and chunk to the window sweep: none of their code
objects may use scratch memory or spill a register -- read, as tests/test_kernel_resources.py reads it for every unit, from the
code-object metadata of a -save-temps compile for gfx950 (hipcc cross-compiles without a GPU).  On top of that test: the three units hold
exactly the exact-sweep instances (BYTE = false) of every head dimension and format, they keep the window kernels' register budget, and
their SGPRs are not lane-spilled either -- which the first arrangement of the 32 evaluations did."""
import os
import sys

from tests.conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

UNITS = {"qattn_splitkv_softcap_fp8": "attn_splitkv_window_softcap_fp8_kernel",
         "qattn_paged_splitkv_softcap_fp8": "attn_paged_splitkv_window_softcap_fp8_kernel",
         "qattn_paged_varlen_splitkv_softcap_fp8": "attn_paged_varlen_splitkv_window_softcap_fp8_kernel"}


def test_the_softcap_kernels_use_no_scratch_and_spill_nothing():
    from quantumattention_amd import build as hip_build

    d = hip_build.build(save_temps=True)   # no-op when the objects and their .s files are current
    built = {name for _, _, name in hip_build.UNITS}
    for unit, kernel in UNITS.items():
        assert unit in built and unit + ".hip" in hip_build.SOURCES
        rows = [r for r in kernel_resources.parse(os.path.join(d, unit + "-hip-amdgcn-amd-amdhsa-gfx950.s")) if kernel in r["name"]]
        # D 64 / 128 / 256 x e4m3 / e5m2, BYTE = false only
        assert len(rows) == 6 and all("Lb0EEEv" in r["name"] and "Lb1EEEv" not in r["name"] for r in rows), unit
        for r in rows:
            assert r.get("private_segment_fixed_size", 0) == 0 and r.get("vgpr_spill_count", 0) == 0, r
            assert r.get("sgpr_spill_count", 0) == 0, r
            assert r["vgpr_count"] <= 256, r   # two waves per SIMD, as the window kernels
