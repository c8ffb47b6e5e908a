"""CPU: include/pht_replace.h's host function for one draw in a stand-alone C
program (tests/host/replace_draw_check.c) with every buffer at exactly its
documented size, built with the address and undefined-behaviour sanitizers
where their runtime links and runs (else plainly), and run once.  No GPU and no
Python in the checked process."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
SRC = os.path.join(HERE, "host", "replace_draw_check.c")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def _build(cc, src, exe, extra):
    cmd = [cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", f"-I{INCLUDE}"] + extra + \
        [src, "-o", exe, "-lm"]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def test_replace_draw_standalone(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if not cc:
        pytest.fail("no host C compiler (cc / gcc)")
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    pexe = str(tmp_path / "probe")
    sanitized = (_build(cc, str(probe), pexe, SANITIZE).returncode == 0
                 and subprocess.run([pexe], capture_output=True, timeout=60).returncode == 0)
    exe = str(tmp_path / "replace_draw_check")
    b = _build(cc, SRC, exe, SANITIZE if sanitized else [])
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print("sanitized" if sanitized else "plain build (no sanitizer runtime)", r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "replace draw: ok" in r.stdout
