"""The matrix on which the oracle's "ref" variant is pinned to the reference's
own compiled C, and the child processes both are called in.  Shared by
tests/test_reference_pin.py and tools/make_golden.py.

Two sides answer the same jobs: ``ref`` (oracle.RefLib: the reference's C on
the R-API stand-in, oracle/_ref/libpht_ref.so) and ``orc`` (oracle.OracleLib:
the restatement, variant "ref").  Every call of either runs in a child process
under a time limit (``Side.call``): a call that does not return is killed,
reported as ``Stalled`` and the child replaced, so nothing of the matrix can
hang the suite.  What the reference itself does not finish is listed in
``LEFT_OUT`` with the reason read from its code, and is not part of the live
matrix.

Run as a program, this module is the child: ``python reference_pin.py ref|orc``
answers pickled jobs on its standard input with pickled results.
"""
import os
import pickle
import select
import struct
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (REPO, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MHRS, ECS, DCS = 1, 2, 4
NAMES = {MHRS: "MHRS", ECS: "ECS", DCS: "DCS"}
CALL_LIMIT = 20.0  # seconds a single call of either side may take (the live cases take well under one)


# ------------------------------------------------------------- the children
class Stalled(Exception):
    """the call did not return within its time limit (the child was killed)"""


class Died(Exception):
    """the child ended during the call (abort, segmentation fault)"""


class Side:
    """A child process answering jobs for one side, each under a time limit."""

    def __init__(self, side):
        assert side in ("ref", "orc")
        self.side, self.proc, self.calls = side, None, 0

    def _start(self):
        self.proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), self.side], stdin=subprocess.PIPE,
                                     stdout=subprocess.PIPE, cwd=REPO)

    def _read(self, nbytes, deadline):
        buf = b""
        fd = self.proc.stdout.fileno()
        while len(buf) < nbytes:
            left = deadline - time.monotonic()
            if left <= 0 or not select.select([fd], [], [], left)[0]:
                raise Stalled(self.side)
            chunk = os.read(fd, nbytes - len(buf))
            if not chunk:
                raise Died(f"{self.side}: exit status {self.proc.wait()}")
            buf += chunk
        return buf

    def call(self, job, limit=CALL_LIMIT):
        if self.proc is None or self.proc.poll() is not None:
            self._start()
        blob = pickle.dumps(job)
        self.proc.stdin.write(struct.pack("<Q", len(blob)) + blob)
        self.proc.stdin.flush()
        self.calls += 1
        deadline = time.monotonic() + limit
        try:
            size, = struct.unpack("<Q", self._read(8, deadline))
            out = pickle.loads(self._read(size, deadline))
        except (Stalled, Died):
            self.close()
            raise
        if isinstance(out, dict) and "error" in out:
            raise RuntimeError(f"{self.side}: {out['error']}")
        return out

    def close(self):
        if self.proc is not None:
            self.proc.kill()
            self.proc.wait()
            for f in (self.proc.stdin, self.proc.stdout):
                try:
                    f.close()
                except OSError:
                    pass
            self.proc = None


def _serve(side):
    from oracle import oracle as O

    lib = O.RefLib() if side == "ref" else O.OracleLib()
    inp, out = sys.stdin.buffer, sys.stdout.buffer
    sys.stdout = sys.stderr  # nothing but answers on the pipe
    while True:
        head = inp.read(8)
        if len(head) < 8:
            return
        job = pickle.loads(inp.read(struct.unpack("<Q", head)[0]))
        try:
            res = _answer(side, lib, job)
        except Exception as e:  # noqa: BLE001  (reported to the parent, which raises)
            res = {"error": repr(e)}
        blob = pickle.dumps(res)
        out.write(struct.pack("<Q", len(blob)) + blob)
        out.flush()


def _answer(side, lib, job):
    op, seed, a = job["op"], job["seed"], job["args"]
    lib.set_seed(seed)
    if op == "gibbs":
        if side == "ref":
            p0, w0 = lib.print_count(), lib.nword()
            res = lib.gibbs(a["it"], a["mhit"], a["method"], a["n"], a["nu"], a["zeta"], a["T"], a["C"], a["y"],
                            a["cen"], a["start"], a["silent"])
            return {"res": res, "prints": lib.print_count() - p0, "nword": lib.nword() - w0}
        res = lib.gibbs(0, a["it"], a["mhit"], a["method"], a["n"], a["nu"], a["zeta"], a["T"], a["C"], a["y"],
                        a["cen"], a["start"])
        return {"res": res}
    if op == "sweep":
        if side == "ref":
            o = lib.sweep(a["method"], a["S"], a["s"], a["y"], a["cen"], mhit=a["mhit"])
        else:
            o = lib.ref_sweep(a["method"], a["S"], a["s"], a["y"], a["cen"], mhit=a["mhit"], per_obs=True)
        return {k: o[k] for k in ("B", "z", "N", "nword")}
    if op == "first_update":  # ref only: one step 1 at (S, s), then the update's Gamma draws on the same stream
        import update_cases as UC

        if a.get("prefix") is not None:  # the chain up to here, on the same stream
            q = a["prefix"]
            lib.gibbs(q["it"], q["mhit"], q["method"], q["n"], q["nu"], q["zeta"], q["T"], q["C"], q["y"], q["cen"],
                      q["start"], q["silent"])
        o = lib.sweep(a["method"], a["S"], a["s"], a["y"], a["cen"], mhit=a["mhit"])
        n, m = a["S"].shape[0], len(a["nu"])
        z = np.zeros(n)
        for row in o["z"]:  # one observation after the other, as the sampler accumulates them
            z = z + row
        N = o["N"].sum(0)
        walk = UC.cells(a["T"], a["C"])
        Nsum, zsum = [0] * m, [0.0] * m
        for i, j, k, c in walk:
            Nsum[k] += int(N[i, i] if j == n else N[i, j])
        for i, j, k, c in reversed(walk):
            zsum[k] = zsum[k] + float(z[i]) / c
        import ctypes

        lib.lib.rgamma.restype = ctypes.c_double
        lib.lib.rgamma.argtypes = [ctypes.c_double, ctypes.c_double]
        draws = [lib.lib.rgamma(float(a["nu"][k]) + Nsum[k], 1.0 / (float(a["zeta"][k]) + zsum[k])) for k in range(m)]
        return {"theta": np.array(draws), "z": z, "N": N}
    if op == "eigen":
        if side == "ref":
            info, ev, Q, Qi = lib.eigen(a["S"])
        else:
            n = a["S"].shape[0]
            sp, info = lib.sp(a["S"], -a["S"].sum(1), ECS)
            f = _sp_fields(lib, sp)
            ev, Q, Qi = f["evals"][:n].copy(), f["Q"][:n * n].reshape(n, n, order="F").copy(), \
                f["Qinv"][:n * n].reshape(n, n, order="F").copy()
        return {"info": info, "evals": ev, "Q": Q, "Qinv": Qi}
    raise ValueError(op)


def _sp_fields(orc, sp):
    """evals, Q, Qinv of the oracle's per-sweep block (oracle/pht_oracle.h:
    n, then S, s, pi, P, Pfull, Q, Qinv, evals as doubles at MAXN strides)"""
    M = orc.maxn
    d = np.frombuffer(sp.raw, np.float64, offset=8)  # int n, padded to 8
    off, out = 0, {}
    for name, size in (("S", M * M), ("s", M), ("pi", M), ("P", M * M), ("Pfull", M * (M + 1)), ("Q", M * M),
                       ("Qinv", M * M), ("evals", M)):
        out[name] = d[off:off + size]
        off += size
    return out


# ----------------------------------------------------------------- the jobs
def _flat(M, dtype):
    return np.ascontiguousarray(np.asarray(M).reshape(-1, order="F"), dtype)


def gibbs_job(seed, it, mhit, method, T, C, nu, zeta, y, cen, start=None, silent=1):
    T = np.asarray(T)
    return {"op": "gibbs", "seed": int(seed),
            "args": dict(it=int(it), mhit=int(mhit), method=int(method), n=T.shape[0] - 1,
                         nu=np.asarray(nu, np.float64), zeta=np.asarray(zeta, np.float64), T=_flat(T, np.int32),
                         C=_flat(C, np.float64), y=np.asarray(y, np.float64), cen=np.asarray(cen, np.int32),
                         start=np.array([-1.0]) if start is None else np.asarray(start, np.float64),
                         silent=int(silent))}


def sweep_job(seed, method, mhit, S, s, y, cen):
    return {"op": "sweep", "seed": int(seed),
            "args": dict(method=int(method), mhit=int(mhit), S=np.asarray(S, np.float64),
                         s=np.asarray(s, np.float64), y=np.asarray(y, np.float64), cen=np.asarray(cen, np.int32))}


def first_update_job(seed, method, mhit, S, s, y, cen, T, C, nu, zeta, prefix=None):
    """reference side only: (after the chain ``prefix``, a gibbs job's args,
    run on the same stream) one step 1 at (S, s) and the update's Gamma draws"""
    job = sweep_job(seed, method, mhit, S, s, y, cen)
    job["op"] = "first_update"
    job["args"].update(T=np.asarray(T, np.int32), C=np.asarray(C, np.float64), nu=np.asarray(nu, np.float64),
                       zeta=np.asarray(zeta, np.float64), prefix=prefix)
    return job


def eigen_job(S):
    return {"op": "eigen", "seed": 1, "args": dict(S=np.asarray(S, np.float64))}


# ------------------------------------------------------ the matrix of chains
BD_N = (3, 4, 5, 10, 15, 20)
CENS = (0.0, 0.3, 1.0)
CHAIN_OBS, CHAIN_IT = 40, 9  # 40 observations, 8 sweeps


def _seed(*parts):
    """a reproducible 31-bit seed from a case's name"""
    h = 2166136261
    for ch in "/".join(map(str, parts)).encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h & 0x7FFFFFFF


def bd_chain(n, method, mhit, frac, it=CHAIN_IT, N=CHAIN_OBS, **kw):
    from phasetype_amd.synth import bd_exit, bd_exit_structure, simulate_ph

    S, s = bd_exit(n)
    T, theta = bd_exit_structure(n)
    y, cen = simulate_ph(S, s, N, seed=0xB0D + n, censor_frac=min(frac, 1.0))
    if frac >= 1.0:
        cen = np.ones(N, np.int32)
    name = f"bd{n}-{NAMES.get(method, method)}" + (f"-h{mhit}" if method == MHRS else "") + f"-c{int(100 * frac)}"
    return name, gibbs_job(_seed(name), it, mhit, method, T, np.ones(T.shape), 1 + 50 * theta,
                           np.full(len(theta), 50.0), y, cen, **kw)


def case_chain(cname, method, tight, it=CHAIN_IT, N=CHAIN_OBS, **kw):
    import update_cases as UC

    c = UC.CASES[cname]
    y, cen = c.data(N, c.censor_frac(method))
    nu, zeta = c.tight_priors(y) if tight else (c.nu, c.zeta)
    name = f"{cname}-{NAMES[method]}-{'tight' if tight else 'own'}"
    return name, gibbs_job(_seed(name), it, 1, method, c.T, c.C, nu, zeta, y, cen, **kw)


def chain_matrix():
    """[(name, job)] of the whole-chain comparisons, LEFT_OUT excluded"""
    import update_cases as UC

    out = []
    for n in BD_N:
        for frac in CENS:
            for method, mhit in ((ECS, 1), (DCS, 1), (MHRS, 1), (MHRS, 5)):
                out.append(bd_chain(n, method, mhit, frac))
    for cname, method in UC.PAIRS:
        if method in NAMES:  # UNIF is not a reference method
            for tight in (False, True):
                out.append(case_chain(cname, method, tight))
    out = [(name, job) for name, job in out if name not in LEFT_OUT]
    for cname, method, tight, it in SHORT:
        name, job = case_chain(cname, method, tight, it=it)
        out.append((f"{name}-it{it}", job))
    return out


# Combinations the reference itself does not finish (the survey: every case of
# the matrix on both sides under a 5 s limit; these two stalled on both sides
# alike, every other returned within 0.25 s and equal), by name, with the
# reason read from the reference's code.  2 of 130; the bar is one in ten.
_MHRS_C = ("MHRS on exact data restarts a forward path until one outlives y (the loop at "
           "src/Simulate_AbsCTMC_gt_Bladt_MHRS.c:49).  The update divides z by c (src/PHT_MCMC_Aslett.c:352) "
           "where the model multiplies, so with multipliers c > 1 and the structure's own weak priors every "
           "sweep draws larger rates than the last ({}); the chance that a path outlives y falls "
           "geometrically and the loop stops returning at sweep {}.")
LEFT_OUT = {
    "fr3c-MHRS-own": _MHRS_C.format("F: 1.44, 2.59, 3.88; MT words per sweep: 23,818, then 696,718", 3),
    "erlang3c-MHRS-own": _MHRS_C.format("1.00, 2.80; 33,678 MT words in sweep 1", 2),
}
# ... and the same two, cut to the sweeps the reference does finish: (case, method, tight, it)
SHORT = [("fr3c", MHRS, False, 3), ("erlang3c", MHRS, False, 2)]


# ------------------------------------------------- per-observation sweeps
SWEEP_N = (3, 4, 10, 20)
SWEEP_SAMPLERS = ((ECS, 1), (DCS, 1), (MHRS, 1), (MHRS, 5))


def sweep_inputs(n):
    """bd_exit(n), 40 simulated observations with 30 % censored, then the
    F(y) = 0.01 / 0.5 / 0.99 / 0.9999 grid once exact and once censored"""
    import pathlaw_ref as PL
    from phasetype_amd.synth import bd_exit, simulate_ph

    S, s = bd_exit(n)
    y, cen = simulate_ph(S, s, 40, seed=0x5EE + n, censor_frac=0.3)
    g = np.asarray(PL.ygrid(S, s, (0.01, 0.5, 0.99, 0.9999)), np.float64)
    y = np.concatenate([y, g, g])
    cen = np.concatenate([cen, np.zeros(len(g), np.int32), np.ones(len(g), np.int32)]).astype(np.int32)
    return S, s, y, cen


def sweep_matrix():
    out = []
    for n in SWEEP_N:
        S, s, y, cen = sweep_inputs(n)
        for method, mhit in SWEEP_SAMPLERS:
            name = f"sweep-bd{n}-{NAMES[method]}-h{mhit}"
            if name not in LEFT_OUT:
                out.append((name, sweep_job(_seed(name), method, mhit, S, s, y, cen)))
    return out


# ------------------------------------------------------ the recorded fixture
RECORDED_OUT = {"gibbs": ("res",), "sweep": ("B", "z", "N", "nword")}


def recorded_subset():
    """the cases tests/golden/r1_reference.npz records: the chains of bd_exit
    at n = 3, 10, 20, every update_cases chain, the sweeps at n = 3 and 10"""
    keep = [(name, job) for name, job in chain_matrix() if not name.startswith(("bd4-", "bd5-", "bd15-"))]
    return keep + [(name, job) for name, job in sweep_matrix() if name.startswith(("sweep-bd3-", "sweep-bd10-"))]


def pack_all(cases):
    """[(name, job, result)] -> the arrays of the fixture.  Inputs that cases
    share (data, structures, priors) are stored once, in a pool; a case is a
    row of scalars, a row of pool indices and a slice of the outputs."""
    pool, where = [], {}

    def ref(v):
        v = np.ascontiguousarray(v)
        key = (v.dtype.str, v.shape, v.tobytes())
        if key not in where:
            where[key] = len(pool)
            pool.append(v)
        return where[key]

    def raw(v, dtype):
        return np.ascontiguousarray(v, dtype).view(np.uint8).reshape(-1)

    names, scal, idx, outs, cuts = [], [], [], [], [0]
    for name, job, res in cases:
        a = job["args"]
        names.append(name)
        if job["op"] == "gibbs":
            scal.append([0, job["seed"], a["it"], a["mhit"], a["method"], a["n"], a["silent"]])
            idx.append([ref(a[k]) for k in ("nu", "zeta", "T", "C", "y", "cen", "start")])
            mine = [raw(res["res"], np.float64)]
        else:
            scal.append([1, job["seed"], 0, a["mhit"], a["method"], a["S"].shape[0], 0])
            idx.append([ref(a[k]) for k in ("S", "s", "y", "cen")] + [-1, -1, -1])
            assert np.abs(res["N"]).max() < 2 ** 15
            mine = [raw(res["B"], np.int32), raw(res["z"], np.float64), raw(res["N"], np.int16),
                    raw(res["nword"], np.uint32)]
        outs += mine
        cuts.append(cuts[-1] + sum(len(o) for o in mine))
    d = {"names": np.array(names), "scalars": np.array(scal, np.int64), "inputs": np.array(idx, np.int32),
         "out_bytes": np.concatenate(outs), "out_cuts": np.array(cuts, np.int64)}
    for k, v in enumerate(pool):
        d[f"pool{k}"] = v
    return d


def unpack_all(d):
    """[(name, job, expected outputs)] of the fixture"""
    out = []
    for r, name in enumerate(d["names"]):
        op, seed, it, mhit, method, n, silent = (int(x) for x in d["scalars"][r])
        ins = [d[f"pool{k}"] if k >= 0 else None for k in d["inputs"][r]]
        raw = d["out_bytes"][d["out_cuts"][r]:d["out_cuts"][r + 1]]
        if op == 0:
            nu, zeta, T, C, y, cen, start = ins
            job = {"op": "gibbs", "seed": seed,
                   "args": dict(it=it, mhit=mhit, method=method, n=n, nu=nu, zeta=zeta, T=T, C=C, y=y, cen=cen,
                                start=start, silent=silent)}
            want = {"res": raw.view(np.float64).reshape(it, len(nu))}
        else:
            S, s, y, cen = ins[:4]
            l = len(y)
            job = {"op": "sweep", "seed": seed, "args": dict(method=method, mhit=mhit, S=S, s=s, y=y, cen=cen)}
            c0, c1, c2 = 4 * l, 4 * l + 8 * l * n, 4 * l + 8 * l * n + 2 * l * n * n
            want = {"B": raw[:c0].view(np.int32), "z": raw[c0:c1].view(np.float64).reshape(l, n),
                    "N": raw[c1:c2].view(np.int16).reshape(l, n, n).astype(np.int32), "nword": raw[c2:].view(np.uint32)}
        out.append((str(name), job, want))
    return out


def same(a, b):
    """bit-for-bit equality of two float or integer arrays (NaNs by pattern)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return a.tobytes() == b.tobytes()


if __name__ == "__main__":
    _serve(sys.argv[1])
