"""CPU: the PSIS-LOO kernels (phasetype_amd/csrc/pht_psis.hip) in the built
library spill no VGPR, use no scratch and at most 64 KB of LDS
(tools/kernel_regs.py; no GPU).  Their occupancy is recorded in DESIGN.md, and
printed here, not pinned."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


def test_psis_kernels_do_not_spill(lib):
    import kernel_regs
    import phasetype_amd.build as B

    hits = {k: v for k, v in kernel_regs.kernels(B.LIB).items() if "psis" in k}
    # the transpose and the per-observation kernel
    assert len(hits) == 2, sorted(hits)
    for name, d in sorted(hits.items()):
        print(f"{name}: vgpr {d['vgpr']} waves_per_simd {d['waves_per_simd']} lds {d['lds_static']}")
        assert d["vgpr_spill"] == 0, (name, "waves_per_simd", d["waves_per_simd"], d)
        assert int(d["scratch"]) == 0, (name, d)
        assert int(d["lds_static"]) <= 64 * 1024, (name, "waves_per_simd", d["waves_per_simd"], d)
