"""CPU: the oracle's "ref" variant against the reference's own compiled C.

oracle/_ref/libpht_ref.so is the reference's unchanged C compiled where it
lies on an R-API stand-in (oracle/Makefile, target ref; oracle/rshim/;
oracle/ref_entry.c), with the R stream of rstream.c and the LAPACK the oracle
binds.  Bar, everywhere below: BIT FOR BIT, the reference is the truth, and
the cases are those of reference_pin.py (chain_matrix, sweep_matrix).

What that pins: the reference's C, given R's API, equals the ref variant draw
for draw.  What it does not: R's own nmath (rgamma above all) and R's bundled
BLAS/LAPACK, which remain stand-ins.

Every call of the reference and of the restatement runs in a child process
under a time limit (reference_pin.Side).  Left out of the live matrix, because
the reference itself does not return (reference_pin.LEFT_OUT holds the reason
read from its code; both are also run cut to the sweeps it does finish):

    fr3c-MHRS-own      MHRS, multipliers c > 1, the structure's own priors
    erlang3c-MHRS-own  the same

Where the reference's sources exist, a missing library is built by the
fixture and a failed build fails the tests; where neither exists (the GPU
machine) the live comparisons skip and the recorded fixture
tests/golden/r1_reference.npz, written from the reference binary by
tools/make_golden.py --from-reference, still runs.
"""
import ctypes as C
import os

import numpy as np
import pytest

import reference_pin as RP
import update_cases as UC
from reference_pin import DCS, ECS, MHRS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHAINS = RP.chain_matrix()
SWEEPS = RP.sweep_matrix()
LIVE = {"n": 0}


@pytest.fixture(scope="module")
def orc_side(orc):
    del orc  # builds the oracle's library where it is missing
    side = RP.Side("orc")
    yield side
    side.close()


@pytest.fixture(scope="module")
def ref_side():
    from oracle import oracle as O

    if os.path.isdir(O.ref_src()):
        if not os.path.exists(O.REF_SO):
            assert O.build_ref() and os.path.exists(O.REF_SO), "the reference build failed"
    elif not os.path.exists(O.REF_SO):
        pytest.skip("neither the reference's sources nor oracle/_ref/libpht_ref.so: recorded fixtures only")
    side = RP.Side("ref")
    yield side
    side.close()
    print(f"\nreference pin: {LIVE['n']} live comparisons in {side.calls} reference calls, each under "
          f"{RP.CALL_LIMIT:g} s; left out of the matrix ({len(RP.LEFT_OUT)} of "
          f"{len(CHAINS) + len(SWEEPS) - len(RP.SHORT) + len(RP.LEFT_OUT)}): {', '.join(RP.LEFT_OUT)}")


def both(ref_side, orc_side, job, keys):
    """the job on both sides; the fields that differ"""
    a, b = ref_side.call(job), orc_side.call(job)
    LIVE["n"] += 1
    return a, b, [k for k in keys if not RP.same(a[k], b[k])]


def test_matrix_leaves_out_at_most_one_in_ten():
    total = len(CHAINS) + len(SWEEPS) - len(RP.SHORT) + len(RP.LEFT_OUT)
    assert 10 * len(RP.LEFT_OUT) <= total, (len(RP.LEFT_OUT), total)
    assert not set(RP.LEFT_OUT) & {name for name, _ in CHAINS + SWEEPS}
    # the matrix the pin is stated on
    names = {name for name, _ in CHAINS}
    for n in RP.BD_N:
        for cen in (0, 30, 100):
            assert {f"bd{n}-ECS-c{cen}", f"bd{n}-DCS-c{cen}", f"bd{n}-MHRS-h1-c{cen}", f"bd{n}-MHRS-h5-c{cen}"} <= names
    for cname, method in UC.PAIRS:
        if method != UC.UNIF:
            for pri in ("own", "tight"):
                name = f"{cname}-{RP.NAMES[method]}-{pri}"
                assert name in names or name in RP.LEFT_OUT, name


# ------------------------------------------------------------ whole chains
@pytest.mark.parametrize("name,job", CHAINS, ids=[c[0] for c in CHAINS])
def test_chain_equals_reference(ref_side, orc_side, name, job):
    """LJMA_Gibbs against orc.gibbs(0, ...), same seed: every draw"""
    a, b, bad = both(ref_side, orc_side, job, ("res",))
    assert not bad, (name, a["res"], b["res"])
    assert np.isfinite(a["res"]).all() and (a["res"] > 0).all()


START_CASES = [("fr3c", ECS), ("fr3c", DCS), ("bd10t", ECS), ("bd10t", MHRS), ("full9c", MHRS)]


@pytest.mark.parametrize("cname,method", START_CASES, ids=[f"{c}-{RP.NAMES[m]}" for c, m in START_CASES])
def test_chain_from_a_given_start(ref_side, orc_side, cname, method):
    c = UC.CASES[cname]
    start = c.truth * np.linspace(0.8, 1.25, c.m)
    name, job = RP.case_chain(cname, method, True, start=start)
    a, b, bad = both(ref_side, orc_side, job, ("res",))
    assert not bad, (name, a["res"], b["res"])
    assert RP.same(a["res"][0], start)
    # start[0] < 0: the prior's mode where nu > 1 and no other element of start is read
    name, job = RP.case_chain(cname, method, True, start=np.concatenate([[-3.0], start[1:]]))
    a, b, bad = both(ref_side, orc_side, job, ("res",))
    assert not bad
    _, plain = RP.case_chain(cname, method, True)
    assert RP.same(a["res"], ref_side.call(plain)["res"])


def test_prior_draw_where_nu_is_at_most_one(ref_side, orc_side):
    """unused07's third parameter (nu = 0.7) starts from an rgamma draw, the
    others from their modes: the draw moves the stream before the first sweep"""
    name, job = RP.case_chain("unused07", ECS, False)
    a, b, bad = both(ref_side, orc_side, job, ("res",))
    assert not bad
    c = UC.CASES["unused07"]
    assert RP.same(a["res"][0, :2], (c.nu[:2] - 1.0) / c.zeta[:2]) and a["res"][0, 2] != (c.nu[2] - 1.0) / c.zeta[2]


@pytest.mark.parametrize("it", [1, 2, 3])
@pytest.mark.parametrize("method", [ECS, DCS, MHRS])
def test_short_chains(ref_side, orc_side, method, it):
    for name, job in (RP.bd_chain(5, method, 1, 0.3, it=it), RP.case_chain("fr3c", method, True, it=it)):
        a, b, bad = both(ref_side, orc_side, job, ("res",))
        assert not bad, (name, a["res"], b["res"])
        assert a["res"].shape[0] == it


@pytest.mark.parametrize("method", [ECS, DCS, MHRS])
def test_silent_changes_the_prints_only(ref_side, orc_side, method):
    _, quiet = RP.bd_chain(4, method, 1, 0.3, silent=1)
    name, loud = RP.bd_chain(4, method, 1, 0.3, silent=0)
    a, b, bad = both(ref_side, orc_side, quiet, ("res",))
    assert not bad
    v = ref_side.call(loud)
    assert RP.same(v["res"], a["res"]) and v["nword"] == a["nword"]
    # silent = 0 prints one progress line per sweep and not the one "silent processing" line
    assert v["prints"] == a["prints"] + (RP.CHAIN_IT - 1) - 1, (v["prints"], a["prints"])


@pytest.mark.parametrize("method", [0, 8, 16, 24, 1 << 20])
def test_unknown_method_code(ref_side, orc_side, method):
    """no sampler bit: the reference reports the method at every sweep and
    leaves the rows after the start as they were given; UNIF (8) is no method
    of the reference"""
    name, job = RP.bd_chain(4, method, 1, 0.3)
    a, b, bad = both(ref_side, orc_side, job, ("res",))
    assert not bad, (name, a["res"], b["res"])
    assert (a["res"][1:] == 0).all() and (a["res"][0] > 0).all() and a["nword"] == 0


# the reference's if / else if order: MHRS, then DCS, then ECS
TWO_BITS = [(3, MHRS), (5, MHRS), (6, DCS), (7, MHRS), (9, MHRS), (10, ECS), (12, DCS), (14, DCS)]


@pytest.mark.parametrize("word,runs", TWO_BITS)
def test_method_word_with_several_bits(ref_side, orc_side, word, runs):
    name, job = RP.bd_chain(4, word, 1, 0.3)
    a, b, bad = both(ref_side, orc_side, job, ("res",))
    assert not bad, (name, a["res"], b["res"])
    job["args"]["method"] = runs
    assert RP.same(a["res"], ref_side.call(job)["res"]), (word, runs)


# ------------------------------------------------------------------- power
def test_the_comparison_can_fail(ref_side, orc_side):
    """another seed, and one prior one ulp away, on the restatement's side"""
    for name, job in (RP.bd_chain(4, ECS, 1, 0.3), RP.case_chain("fr3c", MHRS, True), RP.bd_chain(10, DCS, 1, 0.0)):
        a = ref_side.call(job)
        other = dict(job, seed=job["seed"] + 1)
        assert not RP.same(a["res"], orc_side.call(other)["res"]), name
        args = dict(job["args"], zeta=job["args"]["zeta"].copy())
        args["zeta"][0] = np.nextafter(args["zeta"][0], np.inf)
        assert not RP.same(a["res"], orc_side.call(dict(job, args=args))["res"]), name
        assert RP.same(a["res"], orc_side.call(job)["res"]), name
        LIVE["n"] += 1


# --------------------------------------------------------- per observation
@pytest.mark.parametrize("name,job", SWEEPS, ids=[c[0] for c in SWEEPS])
def test_sweep_per_observation(ref_side, orc_side, name, job):
    """one step 1 at fixed (S, s): start state, z, N and the MT words of every
    observation, on simulated data with 30 % censored and on the F(y) = 0.01,
    0.5, 0.99, 0.9999 grid, exact and censored"""
    a, b, bad = both(ref_side, orc_side, job, ("B", "z", "N", "nword"))
    assert not bad, (name, bad)
    assert (a["nword"] > 0).all()
    y = job["args"]["y"]
    cen = job["args"]["cen"]
    if job["args"]["method"] != DCS:  # an exact observation's sojourns add up to y, a censored one's to more
        tot = a["z"].sum(1)
        assert np.allclose(tot[cen == 0], y[cen == 0], rtol=1e-12) and (tot[cen != 0] >= y[cen != 0]).all()


# ------------------------------------------- host functions of the product
def _eigen_inputs():
    import evaluator_cases as EC
    import test_host as TH

    out = [(f"perturbed-{n}-{seed}",) + tuple(TH._perturbed(n, 7 * n + 1000 * seed)) for n in (2, 3, 5, 10, 15, 20)
           for seed in range(8)]
    out += [(f"{fam}-10",) + tuple(EC.generator(fam, 10)) for fam in ("reversible", "neareq", "stiff")]
    return out


def test_eigen_equals_reference(ref_side, orc_side, lib):
    """LJMA_LAPACKspace + LJMA_eigen against the product's host eigen path
    (pht_build_params, as tests/test_host.py reaches it) and the oracle's:
    evals, Q and Q^-1 under the same LAPACK"""
    import test_host as TH

    for name, S, s in _eigen_inputs():
        n = S.shape[0]
        a, b, bad = both(ref_side, orc_side, RP.eigen_job(S), ("evals", "Q", "Qinv"))
        assert a["info"] == 0 and b["info"] == 0, name
        assert not bad, (name, bad)
        L, _, nbytes, nd = TH._layout(n)
        buf = np.zeros(nbytes, np.uint8)
        assert lib.pht_build_params(n, np.ascontiguousarray(S.reshape(-1, order="F")), s, 2,
                                    buf.ctypes.data_as(C.c_void_p), nbytes) == 0
        dv = buf[: nd * 8].view(np.float64)
        for field in ("evals", "Q", "Qinv"):
            o, size = L[field]
            assert RP.same(dv[o:o + size], a[field].reshape(-1, order="F")), (name, field)


@pytest.mark.parametrize("cname,method", [("fr3c", ECS), ("bd10t", ECS), ("bd10t", DCS), ("full9c", MHRS)])
def test_theta_to_S_is_the_generator_of_the_chain(ref_side, lib, cname, method):
    """A chain of two sweeps from a given start, and the generators it holds.
    Row 0: the numpy statement's generator of the start (diagonal by
    increasing column), handed to the reference's sampler (ref_sweep), then
    the update's Gamma draws on the same stream, give row 1 of LJMA_Gibbs bit
    for bit.  Row 1: the product's pht_theta_to_S (the diagonal order of the
    update, by decreasing column), after the chain so far on the same stream,
    gives row 2.  On full9c the two orders differ in the last bit of six
    diagonal entries."""
    import phasetype_amd as P

    del lib
    c = UC.CASES[cname]
    start = c.truth * np.linspace(0.8, 1.25, c.m)
    name, job = RP.case_chain(cname, method, False, it=3, start=start)
    chain = ref_side.call(job)["res"]
    a = job["args"]
    common = (a["y"], a["cen"], c.T, c.C, a["nu"], a["zeta"])
    S0, s0 = UC.assemble(start, c.T, c.C, True)
    got = ref_side.call(RP.first_update_job(job["seed"], method, 1, S0, s0, *common))
    assert RP.same(got["theta"], chain[1]), (name, got["theta"], chain[1])
    S1, s1 = P.theta_to_S(chain[1], c.T, c.C)
    want = UC.assemble(chain[1], c.T, c.C, False)
    assert RP.same(S1, want[0]) and RP.same(s1, want[1])
    got = ref_side.call(RP.first_update_job(job["seed"], method, 1, S1, s1, *common, prefix=dict(a, it=2)))
    assert RP.same(got["theta"], chain[2]), (name, got["theta"], chain[2])
    LIVE["n"] += 2
    if cname == "full9c":
        assert not RP.same(S0, P.theta_to_S(start, c.T, c.C)[0])


# --------------------------------- the committed golden files, regenerated
def test_golden_chains_from_reference(ref_side):
    """g1 and g2 (tools/make_golden.py) hold the restatement's chains: the
    reference binary reproduces them bit for bit"""
    d = np.load(os.path.join(GOLD, "g1_test_scripts.npz"))
    for tag in ("phtMCMC2", "phtMCMC"):
        T = d[f"{tag}_T"].reshape(4, 4, order="F")
        job = RP.gibbs_job(int(d[f"{tag}_seed"]), int(d[f"{tag}_it"]), int(d[f"{tag}_mhit"]), int(d[f"{tag}_method"]),
                           T, np.ones((4, 4)), d[f"{tag}_nu"], d[f"{tag}_zeta"], d["x"], np.zeros(20, np.int32))
        assert RP.same(ref_side.call(job)["res"], d[f"{tag}_res"]), tag
        LIVE["n"] += 1
    d = np.load(os.path.join(GOLD, "g2_cfg1.npz"))
    for method in (2, 1):
        job = RP.gibbs_job(int(d[f"m{method}_seed"]), int(d["it"]), 1, method, d["T"].reshape(4, 4, order="F"),
                           np.ones((4, 4)), d["nu"], d["zeta"], d["y"], np.zeros(len(d["y"]), np.int32))
        assert RP.same(ref_side.call(job)["res"], d[f"m{method}_res"]), method
        LIVE["n"] += 1


def test_golden_sweeps_from_reference(ref_side):
    """g3 / g4: per-observation sweeps and their MT word counts"""
    d = np.load(os.path.join(GOLD, "g3_sweeps.npz"))
    for n in (3, 4, 10):
        for method, mhit in ((1, 1), (1, 5), (2, 1), (4, 1)):
            k = f"n{n}_m{method}_h{mhit}"
            o = ref_side.call(RP.sweep_job(int(d[k + "_seed"]), method, mhit, d[f"n{n}_S"], d[f"n{n}_s"], d[f"n{n}_y"],
                                           d[f"n{n}_cen"]))
            assert RP.same(o["B"], d[k + "_B"]) and RP.same(o["z"], d[k + "_z"]), k
            assert RP.same(o["N"], d[k + "_N"].astype(np.int32)) and RP.same(o["nword"], d[k + "_nw"]), k
            LIVE["n"] += 1


# ------------------------------- recorded from the reference binary: runs everywhere
def _recorded():
    path = os.path.join(GOLD, "r1_reference.npz")
    return np.load(path) if os.path.exists(path) else None


def test_recorded_reference_fixture(orc_side):
    """tests/golden/r1_reference.npz holds inputs and outputs of a subset of
    the matrix as the reference binary gave them (tools/make_golden.py
    --from-reference): the ref variant reproduces every one bit for bit.
    Runs where the reference is absent too."""
    d = _recorded()
    assert d is not None, "tests/golden/r1_reference.npz is missing"
    cases = RP.unpack_all(d)
    names = [c[0] for c in cases]
    assert len(names) >= 40 and {"fr3c-ECS-own", "bd10t-DCS-tight", "full9c-MHRS-own", "sweep-bd10-MHRS-h5"} <= set(names)
    for name, job, want in cases:
        got = orc_side.call(job)
        bad = [k for k in want if not RP.same(got[k], want[k])]
        assert not bad, (name, bad)
    print(f"\nrecorded reference fixture: {len(names)} cases reproduced")
