"""CPU: the forecast kernels (phasetype_amd/csrc/pht_forecast.hip) in the built
library spill neither VGPRs nor SGPRs and use no scratch, their names carry
none of the substrings the other register tests count kernels by, and their
LDS stays within what DESIGN.md 5i's occupancy claim needs: two blocks a CU, at
most 80 KB each (tools/kernel_regs.py; no GPU).  The register count is printed,
not pinned."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

OTHERS = ("loglik", "llunif", "psis", "ppred", "estep", "quantile")


def test_fcast_kernels_do_not_spill(lib):
    import kernel_regs
    import phasetype_amd.build as B

    hits = {k: v for k, v in kernel_regs.kernels(B.LIB).items() if "fcast" in k}
    # totals-only and pointwise, each with 4 and with 16 state slots a unit
    assert len(hits) == 4, sorted(hits)
    for name, d in sorted(hits.items()):
        print(f"{name}: vgpr {d['vgpr']} waves_per_simd {d['waves_per_simd']} lds {d['lds_static']}")
        assert d["vgpr_spill"] == 0 and d["sgpr_spill"] == 0, (name, d)
        assert int(d["scratch"]) == 0, (name, d)
        assert int(d["lds_static"]) <= 80 * 1024, (name, d)
        for other in OTHERS:
            assert other not in name, name
    # a block of 512 lanes is two waves a SIMD: the totals-only kernels' registers allow the two
    # blocks a CU that the LDS allows (the pointwise ones with 16 slots are the tests' and hold one)
    for name, d in hits.items():
        if "Lb0E" in name:
            assert int(d["waves_per_simd"]) >= 4, (name, d)
