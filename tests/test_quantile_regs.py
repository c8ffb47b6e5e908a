"""CPU: the quantile kernel (phasetype_amd/csrc/pht_quantile.hip) in the built
library spills no VGPR and uses no scratch, and the LDS of its two builds
stays within what DESIGN.md 5h's occupancy claims need: the one-table pool two
blocks a CU (at most 80 KB each), the four-table pool one block a CU (160 KB)
(tools/kernel_regs.py; no GPU).  The register count is printed, not pinned."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


def test_quantile_kernels_do_not_spill(lib):
    import kernel_regs
    import phasetype_amd.build as B

    hits = {k: v for k, v in kernel_regs.kernels(B.LIB).items() if "quantile" in k}
    # the two LDS pools of quantile_kernel
    assert len(hits) == 2, sorted(hits)
    lds = []
    for name, d in sorted(hits.items()):
        print(f"{name}: vgpr {d['vgpr']} waves_per_simd {d['waves_per_simd']} lds {d['lds_static']}")
        assert d["vgpr_spill"] == 0 and d["sgpr_spill"] == 0, (name, d)
        assert int(d["scratch"]) == 0, (name, d)
        # a block of 256 lanes is one wave a SIMD: two blocks a CU need two
        assert int(d["waves_per_simd"]) >= 2, (name, d)
        lds.append(int(d["lds_static"]))
        for other in ("loglik", "llunif", "psis", "ppred", "estep"):
            assert other not in name, name
    assert min(lds) <= 80 * 1024 and max(lds) <= 160 * 1024, lds
