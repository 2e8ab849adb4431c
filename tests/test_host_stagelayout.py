"""The HIP-free staging layout of the host-form queries (csrc/rb_stagelayout.hpp)
compiles as plain host C++ and passes the checks of tests/host_stagelayout.cpp:
the bytes per unit of rb_query_contacts, rb_batch_contacts and rb_batch_impulses
in their closed forms, fields back to back without overlap, reals 8-byte
aligned, absent fields empty, fit(limit) = limit / per, and consecutive ranges
tiling the caller's arrays.  Built plain and with the address and
undefined-behaviour sanitizers; both are stand-alone programs.  No GPU."""
import os
import subprocess

import pytest

from conftest import PKG, ROOT
from test_host_sampleplan import makefile_hipcc

CSRC = os.path.join(PKG, "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_host_stagelayout(tmp_path, flags):
    out = str(tmp_path / "host_stagelayout")
    subprocess.run([makefile_hipcc(), "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", out,
                    os.path.join(ROOT, "tests", "host_stagelayout.cpp")], check=True)
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_stagelayout: ok" in r.stdout
