"""The HIP-free launch plan of a sampled batch run (csrc/rb_sampleplan.hpp)
compiles as plain host C++ and passes the checks of tests/host_sampleplan.cpp:
every sampled step once and in order, no launch past 256 steps or the buffer,
the phase carried across launches, every step run.  Built plain and with the
address and undefined-behaviour sanitizers; both are stand-alone programs.
No GPU."""
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
def test_host_sampleplan(tmp_path, flags):
    out = str(tmp_path / "host_sampleplan")
    subprocess.run([makefile_hipcc(), "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", out,
                    os.path.join(ROOT, "tests", "host_sampleplan.cpp")], check=True)
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_sampleplan: ok" in r.stdout
