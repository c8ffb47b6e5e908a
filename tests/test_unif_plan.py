"""CPU: the host arithmetic the uniformisation analyses share
(phasetype_amd/csrc/host_unif_plan.h: the draws' meta words, the table stride,
the batches, the layout of the input buffer), checked by a stand-alone program
(tests/host/) built with the host compiler's address and undefined-behaviour
sanitizers where a sanitized program builds and runs, plain otherwise."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "phasetype_amd", "csrc")
SRC = os.path.join(HERE, "host", "unif_plan_check.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def _build(cxx, src, exe, extra):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", f"-I{CSRC}"] + extra + [src, "-o", exe]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def test_unif_plan_standalone(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    if not cxx:
        pytest.fail("no host C++ compiler (c++ / g++)")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    pexe = str(tmp_path / "probe")
    sanitized = (_build(cxx, str(probe), pexe, SANITIZE).returncode == 0
                 and subprocess.run([pexe], capture_output=True, timeout=60).returncode == 0)
    exe = str(tmp_path / "unif_plan_check")
    b = _build(cxx, SRC, exe, SANITIZE if sanitized else [])
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print("sanitized" if sanitized else "plain build (no sanitizer runtime)", r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "unif plan: ok" in r.stdout
