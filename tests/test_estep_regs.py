"""CPU: the E-step kernels (phasetype_amd/csrc/pht_estep.hip) in the built
library spill no VGPR and use no scratch, and the histogram kernel's LDS (the
table, 1 / k and the histogram at the cap K = 2047) leaves one block a CU
(160 KB) (tools/kernel_regs.py; no GPU).  Their occupancy is recorded in
DESIGN.md, and printed here, not pinned."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


def test_estep_kernels_do_not_spill(lib):
    import kernel_regs
    import phasetype_amd.build as B

    hits = {k: v for k, v in kernel_regs.kernels(B.LIB).items() if "estep" in k}
    # the histogram and the contraction kernel
    assert len(hits) == 2, sorted(hits)
    for name, d in sorted(hits.items()):
        print(f"{name}: vgpr {d['vgpr']} waves_per_simd {d['waves_per_simd']} lds {d['lds_static']}")
        assert d["vgpr_spill"] == 0, (name, "waves_per_simd", d["waves_per_simd"], d)
        assert int(d["scratch"]) == 0, (name, d)
        assert int(d["lds_static"]) <= 160 * 1024, (name, d)
        for other in ("loglik", "llunif", "psis", "ppred"):
            assert other not in name, name
