"""The two HIP-free host headers of the C-ABI implementation (rb_hostpool.hpp:
the thread pool of rb_set_state / rb_get_state; rb_period.hpp: the scoring of
the table layout's period split) compile as plain host C++ and pass the checks
of tests/host_units.cpp, with one pool thread and with four.  No GPU."""
import os
import re
import subprocess

import pytest

from conftest import PKG, ROOT

CSRC = os.path.join(PKG, "csrc")


def makefile_hipcc():
    m = re.search(r"^HIPCC\s*\?=\s*(\S+)", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    return os.environ.get("HIPCC", m.group(1))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_units") / "host_units")
    subprocess.run([makefile_hipcc(), "-x", "c++", "-std=c++17", "-O2", "-Wall", "-pthread", "-I", CSRC, "-o", out,
                    os.path.join(ROOT, "tests", "host_units.cpp")], check=True)
    return out


@pytest.mark.parametrize("threads", [1, 4])
def test_host_units(program, threads):
    env = dict(os.environ, RBHIP_HOST_THREADS=str(threads))
    r = subprocess.run([program], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
