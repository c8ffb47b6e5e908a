"""CPU: the spares kernels (phasetype_amd/csrc/pht_spares.hip) in the built
library.  The unit kernel's builds for a compile-time n (3, 5, 10, 15, 20;
totals-only and pointwise) spill neither VGPRs nor SGPRs and use no scratch:
v[n] lives in registers.  Their VGPR and LDS figures are pinned at what the
build shows (DESIGN.md 5k's table), the LDS under the 80 KB that two blocks a
CU need.  The runtime-n build (n up to 32) and the vectors kernel (row i of P*
and the 32 accumulators in registers) use no scratch either; their scalar
spills go to VGPR lanes and are printed, not pinned.  Their names carry none of
the substrings the other register tests count kernels by (tools/kernel_regs.py;
no GPU)."""
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

OTHERS = ("cond_", "fcast", "loglik", "llunif", "psis", "ppred", "estep", "quantile", "mhrs_search")
LDS = 75264
# n: (VGPRs totals-only, VGPRs pointwise)
PINNED = {3: (54, 58), 5: (54, 58), 10: (66, 72), 15: (86, 90), 20: (106, 110)}
VECTORS_VGPR = 162


def test_spares_kernels_do_not_spill(lib):
    import kernel_regs
    import phasetype_amd.build as B

    hits = {k: v for k, v in kernel_regs.kernels(B.LIB).items() if "spares_" in k}
    unit = {k: v for k, v in hits.items() if "spares_kernel" in k}
    # six values of n (0: runtime), totals-only and pointwise, and the vectors kernel
    assert len(unit) == 12 and len(hits) == 13, sorted(hits)
    for name, d in sorted(hits.items()):
        print(f"{name}: vgpr {d['vgpr']} sgpr_spill {d['sgpr_spill']} waves_per_simd {d['waves_per_simd']} "
              f"lds {d['lds_static']}")
        assert d["vgpr_spill"] == 0 and int(d["scratch"]) == 0, (name, d)
        for other in OTHERS:
            assert other not in name, name
    seen = set()
    for name, d in unit.items():
        m = re.search(r"ILi(\d+)ELb([01])E", name)
        n, pw = int(m.group(1)), int(m.group(2))
        seen.add((n, pw))
        # the block sums hold Delta and V at fixed places: the same LDS whatever n, two blocks a CU
        assert int(d["lds_static"]) == LDS and LDS <= 80 * 1024, (name, d)
        if n == 0:
            continue
        assert d["sgpr_spill"] == 0, (name, d)
        assert int(d["vgpr"]) == PINNED[n][pw], (name, d)
        # a block of 512 lanes is two waves a SIMD: the registers allow the two blocks a CU that the LDS allows
        assert int(d["waves_per_simd"]) >= 4, (name, d)
    assert seen == {(n, pw) for n in (0, 3, 5, 10, 15, 20) for pw in (0, 1)}
    vec = [d for k, d in hits.items() if "spares_vectors" in k]
    assert len(vec) == 1 and int(vec[0]["lds_static"]) == 0 and int(vec[0]["vgpr"]) == VECTORS_VGPR, vec
