"""Per-environment planes, gravity and applied forces of a batch
(rb_batch_set_planes / _gravity / _xfrc): the entry points are exported and
bound, a null handle is refused before any device call, and the step kernel
instances a batch without per-environment data launches compile to what they
compiled to before the per-environment instances existed (no GPU here)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG

NEW_FUNCS = ["rb_batch_set_planes", "rb_batch_set_gravity", "rb_batch_set_xfrc"]
EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    from rbhip import _lib
    return _lib.load(path)


def test_env_entry_points_are_exported_and_bound(lib):
    from rbhip import _lib
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [f for f in NEW_FUNCS if f not in exported]
    assert not [f for f in NEW_FUNCS if f not in _lib.SIGNATURES]
    assert b"0.4" in lib.rb_version()                      # additive: the version string stays
    import rbhip
    for m in ("set_planes", "set_gravity", "set_xfrc", "from_scenes"):
        assert callable(getattr(rbhip.BatchWorld, m))
    header = open(os.path.join(PKG, "..", "include", "rbhip.h")).read()
    for f in NEW_FUNCS:
        assert re.search(rf"\bint\s+{f}\s*\(rb_batch \*b, const double \*\w+\);", header), f


def test_env_entry_points_null_handle_is_einval(lib):
    a = np.zeros(48)
    p = a.ctypes.data_as(C.c_void_p)
    for f in NEW_FUNCS:
        assert getattr(lib, f)(None, p) == EINVAL
        assert b"null batch" in lib.rb_last_error()
        assert getattr(lib, f)(None, None) == EINVAL


# VGPRs, LDS bytes per block and scratch bytes per lane of the step kernel
# instances a batch without per-environment data launches, as `make -C csrc
# resource-usage` reported them on the parent of the commit that added the
# per-environment (ENVS) instances (there the kernels had no ENVS parameter:
# batch_step_kernel<T, BOX, REC>, batch_balls_kernel<T, REC>).  Keyed by
# (kernel, real type, flags before ENVS).
# The batch_step_kernel block is from that parent and has held since.  The
# batch_balls_kernel block is from the commit that moved the pair evaluation
# into ball_pair (rb_balls.hpp): the same expressions allocate fewer registers
# from there (that parent's 176 / 186 / 117 / 123 VGPRs; LDS and scratch as
# before), and an equality pin follows the build.
PARENT_RESOURCES = {
    ("batch_step_kernel", "d", (False, False)): (184, 4352, 0),
    ("batch_step_kernel", "d", (True, False)): (200, 4352, 0),
    ("batch_step_kernel", "f", (False, False)): (102, 2304, 0),
    ("batch_step_kernel", "f", (True, False)): (114, 2304, 0),
    ("batch_step_kernel", "d", (False, True)): (186, 4352, 0),     # the recording instances
    ("batch_step_kernel", "d", (True, True)): (202, 4352, 0),
    ("batch_step_kernel", "f", (False, True)): (104, 2304, 0),
    ("batch_step_kernel", "f", (True, True)): (116, 2304, 0),
    ("batch_balls_kernel", "d", (False,)): (168, 13056, 0),
    ("batch_balls_kernel", "d", (True,)): (180, 13056, 0),
    ("batch_balls_kernel", "f", (False,)): (116, 6656, 0),
    ("batch_balls_kernel", "f", (True,)): (122, 6656, 0),
}


def test_plain_instances_compile_as_before():
    """The ENVS = false instances are the code the pinned commits compiled
    (PARENT_RESOURCES says which): same VGPR count, LDS size and no scratch.
    The ENVS instances exist for every
    BOX x REC combination (and REC for the two-ball law), without scratch."""
    out = subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc"), "resource-usage"],
                         capture_output=True, text=True, check=True).stdout
    got = {}
    for m in re.finditer(r"Function Name: _ZN2rb\d+(batch_step_kernel|batch_balls_kernel)I([df])((?:Lb[01]E)+)E\S*\s+"
                         r"(?:.*\n)*?.*VGPRs: (\d+)(?:.*\n)*?.*ScratchSize \[bytes/lane\]: (\d+)(?:.*\n)*?"
                         r".*LDS Size \[bytes/block\]: (\d+)", out):
        flags = tuple(c == "1" for c in re.findall(r"Lb([01])E", m.group(3)))
        got[(m.group(1), m.group(2), flags)] = (int(m.group(4)), int(m.group(6)), int(m.group(5)))
    assert len(got) == 24, sorted(got)                     # 2 x 8 step and 2 x 4 two-ball instances
    for (kern, real, flags), want in PARENT_RESOURCES.items():
        assert got[(kern, real, flags + (False,))] == want, (kern, real, flags, got[(kern, real, flags + (False,))])
    envs = {k: v for k, v in got.items() if k[2][-1]}
    assert len(envs) == 12
    assert not [k for k, v in envs.items() if v[2] != 0], "an ENVS instance uses scratch"
    # the planes are dynamic LDS: the static size of an ENVS instance is the plain one's
    for k, v in envs.items():
        assert v[1] == got[(k[0], k[1], k[2][:-1] + (False,))][1]
