"""The HIP-free lane plan of a batch with a population (csrc/rb_laneplan.hpp)
compiles as plain host C++ and passes the checks of tests/host_laneplan.cpp:
every present body exactly one lane, an environment's lanes consecutive in one
wave in body order, environments in order across waves, idle lanes -1, uniform
counts reproducing floor(64 / M) environments per wave, the edge cases.  Built
plain and with the address and undefined-behaviour sanitizers; both are
stand-alone programs.  No GPU."""
import os
import re
import subprocess

import pytest

from conftest import PKG, ROOT

CSRC = os.path.join(PKG, "csrc")


def makefile_hipcc():
    m = re.search(r"^HIPCC\s*\?=\s*(\S+)", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    return os.environ.get("HIPCC", m.group(1))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_host_laneplan(tmp_path, flags):
    out = str(tmp_path / "host_laneplan")
    subprocess.run([makefile_hipcc(), "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", out,
                    os.path.join(ROOT, "tests", "host_laneplan.cpp")], check=True)
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_laneplan: ok" in r.stdout
