"""CPU: the uniformisation log-likelihood kernels
(phasetype_amd/csrc/pht_loglik_unif.hip) in the built library spill no VGPR
and use at most 64 KB of LDS (tools/kernel_regs.py; no GPU).  Their occupancy
is recorded in DESIGN.md, and printed here, not pinned."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


def test_llunif_kernels_do_not_spill(lib):
    import kernel_regs
    import phasetype_amd.build as B

    hits = {k: v for k, v in kernel_regs.kernels(B.LIB).items() if "llunif" in k}
    # the table kernel, and the evaluation kernel totals-only and pointwise
    assert len(hits) == 3, sorted(hits)
    assert sum("llunif_table_kernel" in k for k in hits) == 1
    for name, d in sorted(hits.items()):
        print(f"{name}: vgpr {d['vgpr']} waves_per_simd {d['waves_per_simd']} lds {d['lds_static']}")
        assert d["vgpr_spill"] == 0, (name, "waves_per_simd", d["waves_per_simd"], d)
        assert int(d["scratch"]) == 0, (name, d)
        assert int(d["lds_static"]) <= 64 * 1024, (name, "waves_per_simd", d["waves_per_simd"], d)
