"""GPU: a context gives back everything it allocated.

Every device buffer, pinned buffer, stream and event of the host runtime is
held by an owning member of pht_ctx (phasetype_amd/csrc/host_hip.h); destroy
and pht_ctx_set_obs release them by letting the owners go.  Contexts of every
sampler are created, given observations twice, swept (plain and debug), asked
for log-likelihoods with pointwise output and accumulation, and destroyed,
twenty times over: free device memory must not shrink from round to round, and
the last round computes what the first did."""
import subprocess
import sys

import numpy as np
import pytest

import phasetype_amd as P
from phasetype_amd.synth import bd_exit, simulate_ph

pytestmark = pytest.mark.gpu

METHODS = {"MHRS": 1, "ECS": 2, "DCS": 4, "UNIF": 8}
ROUNDS = 20


def _round(S, s, obs_a, obs_b):
    """One life of a context per sampler: the sweeps' statistics, the debug
    sweeps' outputs and the log-likelihood words, as one list of arrays."""
    out = []
    for method in METHODS.values():
        sw = P.Sweeper(3, method, 1, device=0)
        sw.set_obs(*obs_a)
        sw.set_obs(*obs_b)  # another N: every observation-sized buffer goes and comes back
        out.append(sw.sweep(S, s, key=(7, 9), sweep=1))
        dbg = sw.sweep_debug(S, s, key=(7, 9), sweep=2)
        out += [dbg[k] for k in ("stats", "B", "pre", "flags", "ndraw", "zq", "N")]
        ll = sw.loglik([S, 1.25 * S], [s, 1.25 * s], batch=1, pointwise=True, accumulate=True)
        out += [ll[k] for k in ("H", "F", "nbad", "nobs")]
        out.append(ll["pointwise"].view(np.uint64))
        st = sw.waic_state()
        out += [st[k].view(np.uint64) if st[k].dtype == np.float64 else st[k] for k in sorted(st)]
        sw.close()
    return out


# Free device memory is read by torch in a child process of its own (the
# figure is device-wide, so the child sees what this process holds): torch
# cannot open the device in a process where the library already has.
_CHILD = """
import sys, torch
torch.cuda.init()
print("ready", flush=True)
for _ in sys.stdin:
    print(torch.cuda.mem_get_info(0)[0], flush=True)
"""


def test_contexts_leave_no_device_memory_behind(gpu):
    S, s = bd_exit(3)
    y, cens = simulate_ph(S, s, 200, seed=5, censor_frac=0.3)
    assert 0 < cens.sum() < 200
    obs_a, obs_b = (y, cens), (y[:150], cens[:150])
    child = subprocess.Popen([sys.executable, "-c", _CHILD], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def free_now():
        child.stdin.write("\n")
        child.stdin.flush()
        return int(child.stdout.readline())

    try:
        first = _round(S, s, obs_a, obs_b)
        last = _round(S, s, obs_a, obs_b)
        assert child.stdout.readline().strip() == "ready"
        free2 = free_now()
        for _ in range(2, ROUNDS):
            last = _round(S, s, obs_a, obs_b)
        free20 = free_now()
    finally:
        child.stdin.close()
        try:
            child.wait(timeout=30)
        except subprocess.TimeoutExpired:
            child.kill()
    print(f"free device memory after round 2: {free2}, after round {ROUNDS}: {free20}, drift {free2 - free20} bytes")
    assert free20 >= free2
    assert len(first) == len(last)
    for a, b in zip(first, last):
        assert np.array_equal(a, b)
