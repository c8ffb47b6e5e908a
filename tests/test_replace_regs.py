"""CPU: the two replacement kernels (phasetype_amd/csrc/pht_replace.hip) in the
built library spill no VGPR and no SGPR and use no scratch, and the LDS of each
stays within what DESIGN.md 5l's occupancy statement needs: two blocks a CU, at
most 80 KB each (tools/kernel_regs.py; no GPU).  The register counts are
printed, not pinned."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


def test_replace_kernels_do_not_spill(lib):
    import kernel_regs
    import phasetype_amd.build as B

    hits = {k: v for k, v in kernel_regs.kernels(B.LIB).items() if "rp_curve_kernel" in k or "rp_policy_kernel" in k}
    assert len(hits) == 2, sorted(hits)
    for name, d in sorted(hits.items()):
        print(f"{name}: vgpr {d['vgpr']} sgpr {d.get('sgpr')} waves_per_simd {d['waves_per_simd']} "
              f"lds {d['lds_static']}")
        assert d["vgpr_spill"] == 0 and d["sgpr_spill"] == 0, (name, d)
        assert int(d["scratch"]) == 0, (name, d)
        # a block of 256 lanes is one wave a SIMD: two blocks a CU need two
        assert int(d["waves_per_simd"]) >= 2, (name, d)
        assert int(d["lds_static"]) <= 80 * 1024, (name, d)
        # the other kernels' register tests count theirs by these substrings
        for other in ("quantile", "loglik", "llunif", "psis", "ppred", "estep", "fcast", "cond", "spares"):
            assert other not in name, name
