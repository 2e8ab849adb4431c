"""The two-ball law in a batch and sampled runs (rb_batch_set_contact_law,
rb_batch_run_sampled): the entry points are exported and bound, and their
handle check runs before any device call (no GPU here)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG

NEW_FUNCS = ["rb_batch_set_contact_law", "rb_batch_run_sampled"]
EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    from rbhip import _lib
    return _lib.load(path)


def test_new_batch_entry_points_are_exported_and_bound(lib):
    from rbhip import _lib
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [f for f in NEW_FUNCS if f not in exported]
    assert not [f for f in NEW_FUNCS if f not in _lib.SIGNATURES]
    assert b"0.4" in lib.rb_version()
    import rbhip
    assert hasattr(rbhip.BatchWorld, "set_contact_law") and hasattr(rbhip.BatchWorld, "run_sampled")


def test_new_batch_entry_points_null_handle_is_einval(lib):
    a = np.zeros(16)
    p = a.ctypes.data_as(C.c_void_p)
    nf = C.c_int64()
    assert lib.rb_batch_set_contact_law(None, 1, 0.01) == EINVAL
    assert lib.rb_batch_set_contact_law(None, 0, 0.01) == EINVAL
    assert lib.rb_batch_run_sampled(None, 1, 1, 0.01, 0.5, 0.5, 0.0, p, p, C.byref(nf)) == EINVAL
    assert lib.rb_batch_run_sampled(None, 1, 1, 0.01, 0.5, 0.5, 0.0, p, None, None) == EINVAL
