"""The HIP-free world plan (csrc/rb_worldplan.hpp) compiles as plain host C++ and
passes the checks of tests/host_worldplan.cpp: hand-computed plans taken from
the comments the code carries, properties of every plan over a sweep of scenes
(the table a power of two within its limits, the groups within a quarter of
it, the linear period's bits), the layout word's accessors, the byte counts in
their closed forms — and the rows of tests/golden/world_plan_parent.json,
recorded on the device before the plan was factored out of rb_world_create
(tests/test_gpu_world_plan.py), handed over as integers on stdin.  Built plain
and with the address and undefined-behaviour sanitizers; both are stand-alone
programs.  No GPU."""
import os
import subprocess

import pytest

from conftest import PKG, ROOT
from test_gpu_world_plan import recorded
from test_host_sampleplan import makefile_hipcc

CSRC = os.path.join(PKG, "csrc")


def plan_rows():
    """the creation-time rows (a row that stepped has grown its table since)"""
    rows = []
    for r in recorded().values():
        if r["steps"]:
            continue
        c, v, w = r["counts"], r["values"], r["world"]
        kept = r["env"].get("RBHIP_FIT_PERIOD") == "0"   # else rb_set_state has refitted the period's split
        nums = [c["n"], w.get("world_size", 1), w.get("rank", 0), int(c["n_spheres"] != c["n"]), c["n_spheres"],
                8 if r["dtype"] == "f64" else 4, w.get("max_partners", 16), c["n_planes"],
                v["buckets"], v["max_partners"], v["grid_layout"], v["hashed_form"], v["help_search"], v["table_epoch"],
                v["n_owned"], v["bytes_per_body_step"], int(kept)]
        env = [f"{k}={val}" for k, val in r["env"].items() if k != "RBHIP_FIT_PERIOD"]
        rows.append(" ".join(map(str, nums + env)))
    return rows


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_host_worldplan(tmp_path, flags):
    out = str(tmp_path / "host_worldplan")
    subprocess.run([makefile_hipcc(), "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", out,
                    os.path.join(ROOT, "tests", "host_worldplan.cpp")], check=True)
    rows = plan_rows()
    assert len(rows) >= 28
    r = subprocess.run([out, str(len(rows))], input="\n".join(rows) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_worldplan: ok" in r.stdout
