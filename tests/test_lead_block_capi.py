"""The step kernels' preloaded leads (csrc/rb_step.hpp Lead, DESIGN §4 "Kernel
arguments": LEAD_ARGS, and LEAD_EP_ARGS with the lead block's address for the
kernels of worlds with append epochs), read from the step units' device
assembly (kernel descriptors, code-object metadata) and resource listing.
No GPU needed: the units are cross-compiled for gfx950."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rigidbody-simulation_amd", "csrc")

# LEAD_ARGS: four pointers (snapshot, state, constants, kinds), two 64-bit row
# strides, n_local, lo.  LEAD_EP_ARGS: a fifth pointer (the lead block's
# generation word) and the strides as 32-bit counts.  14 dwords either way
LEAD_DWORDS = 4 * 2 + 2 * 2 + 2
LEAD_EP_DWORDS = 5 * 2 + 4
KERNARG_PTR_SGPRS = 2
# every kernel that takes a lead (the box, search and update kernels take the
# parameter block alone)
LEAD_KERNELS = ("step_kernel_wide_help", "step_kernel_wide", "step_kernel_coop_help", "step_kernel_coop",
                "step_kernel_one")
LEAD_EP_KERNELS = ("step_kernel_wide_help_ep", "step_kernel_wide_ep")
# instances per real type: wide_help MAXP x HALO x SHARE 8, wide MAXP x HALO 4, coop_help, coop, one MAXP 2 each;
# wide_help_ep MAXP x SHARE 4, wide_ep MAXP 2
LEAD_INSTANCES = 2 * (8 + 4 + 2 + 2 + 2)
LEAD_EP_INSTANCES = 2 * (4 + 2)


def _make(target):
    return subprocess.run(["make", "-s", "-C", CSRC, target], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def step_asm():
    """kernel name -> {preload, user_sgprs, vgprs, scratch} of the four step units"""
    out = _make("step-asm")
    kern = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\s+\.amdhsa_user_sgpr_count (\d+)\s+"
                         r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", out):
        kern[m.group(1)] = {"user_sgprs": int(m.group(2)), "preload": int(m.group(3))}
    for m in re.finditer(r"\.name:\s+(\S+)\s+\.private_segment_fixed_size:\s+(\d+)\s+\.vgpr_count:\s+(\d+)", out):
        kern[m.group(1)].update(scratch=int(m.group(2)), vgprs=int(m.group(3)))
    assert kern and all(len(v) == 4 for v in kern.values()), "descriptor and metadata of every kernel"
    return kern


def _is(name, kernels):
    return any(re.match(rf"_ZN2rb\d+{k}I[df]", name) for k in kernels)


def test_every_lead_kernel_preloads_its_whole_lead(step_asm):
    for kernels, count, dwords in ((LEAD_KERNELS, LEAD_INSTANCES, LEAD_DWORDS),
                                   (LEAD_EP_KERNELS, LEAD_EP_INSTANCES, LEAD_EP_DWORDS)):
        lead = {n: v for n, v in step_asm.items() if _is(n, kernels)}
        assert len(lead) == count, sorted(lead)
        for name, v in lead.items():
            assert v["preload"] == dwords == 14, (name, v)
            assert v["user_sgprs"] == KERNARG_PTR_SGPRS + dwords, (name, v)
    # ... and the kernels without a lead ask for no preload
    for name, v in step_asm.items():
        if not _is(name, LEAD_KERNELS + LEAD_EP_KERNELS):
            assert v["preload"] == 0, (name, v)


def test_no_kernel_has_scratch(step_asm):
    for name, v in step_asm.items():
        assert v["scratch"] == 0, (name, v)
    out = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage"], capture_output=True, text=True, check=True)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stdout + out.stderr)]
    assert len(scratch) > len(step_asm) and not any(scratch), scratch


def test_wide_help_fp64_fits_two_waves_per_simd(step_asm):
    """The wide + helper fp64 instances run two waves per SIMD: at most 256
    registers each.  The counts before the lead block, for the report:
    profiles/help_finish/resources_wide.txt (194-244), whose names carry the
    flags <MAXP, HALO, EP, SHARE>; the EP instances are the _ep kernels now.
    (The kernels' own parameters are still <MAXP, HALO, SHARE> and, for the
    _ep kernels, <MAXP, SHARE>; inside, a form type names them: rb_step.hpp
    WideHelp<MAXP, SHARE> and WideHelpEp<MAXP, SHARE>, HALO beside the form.)"""
    txt = open(os.path.join(ROOT, "profiles", "help_finish", "resources_wide.txt")).read()
    base = {}
    for m in re.finditer(r"Function Name: _ZN2rb21step_kernel_wide_helpIdLi(\d+)ELb([01])ELb([01])ELb([01])EE\S+\s+"
                         r"TotalSGPRs: \d+\s+VGPRs: (\d+)", txt):
        maxp, halo, ep, share = m.group(1), m.group(2), m.group(3), m.group(4)
        new = (f"_ZN2rb24step_kernel_wide_help_epIdLi{maxp}ELb{share}EEEv" if ep == "1"
               else f"_ZN2rb21step_kernel_wide_helpIdLi{maxp}ELb{halo}ELb{share}EEEv")
        base[new] = int(m.group(5))
    assert len(base) == 12, base
    for prefix, before in base.items():
        now = [v["vgprs"] for n, v in step_asm.items() if n.startswith(prefix)]
        assert len(now) == 1, prefix
        print(f"{prefix}: VGPRs {before} -> {now[0]}")
        assert now[0] <= 256, (prefix, before, now)
