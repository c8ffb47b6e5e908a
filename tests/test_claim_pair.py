"""CPU: the persistent kernels' claim arithmetic (phasetype_amd/csrc/
pht_claim.h: the equal stripes and the weighted dealing between the two
blocks of a CU), checked by a stand-alone program (tests/host/claim_check.cpp)
built with the host compiler's address and undefined-behaviour sanitizers
where a sanitized program builds and runs, plain otherwise: every position
claimed exactly once for grids 1, 2, 4, 512 and 0 ... 30 grid + 7 chunks with
and without a ragged last chunk, positions increasing per block, chunk shares
P : Q."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "phasetype_amd", "csrc")
SRC = os.path.join(HERE, "host", "claim_check.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def _build(cxx, src, exe, extra):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", f"-I{CSRC}"] + extra + [src, "-o", exe]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def test_claim_arithmetic_standalone(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    if not cxx:
        pytest.fail("no host C++ compiler (c++ / g++)")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    pexe = str(tmp_path / "probe")
    sanitized = (_build(cxx, str(probe), pexe, SANITIZE).returncode == 0
                 and subprocess.run([pexe], capture_output=True, timeout=60).returncode == 0)
    exe = str(tmp_path / "claim_check")
    b = _build(cxx, SRC, exe, SANITIZE if sanitized else [])
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print("sanitized" if sanitized else "plain build (no sanitizer runtime)", r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "claim arithmetic: ok" in r.stdout
