"""dcn16t's two instances (plain, and with IDAUp's up-sample + add in the epilogue) keep the budget the kernel is written for:
three workgroups per CU = at most 168 VGPRs, at most 53 KB of LDS, and nothing in scratch.  Read from the metadata notes of the
built library's code objects; needs no GPU.  dcn16p and dcn16s, which share their set-up, blend and fallback code with dcn16t
(csrc/dcn_patch_common.h), are held to their two-workgroups-per-CU budget the same way."""
import os
import re
import shutil
import subprocess

import pytest

from centerpose_amd import hip


def _tool(name):
    return shutil.which(name) or os.path.join("/opt/rocm/lib/llvm/bin", name)


def test_dcn16t_instances_fit_three_workgroups_per_cu(tmp_path):
    objdump, readelf = _tool("llvm-objdump"), _tool("llvm-readelf")
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("llvm-objdump / llvm-readelf not available")
    so = tmp_path / "lib.so"
    shutil.copy(hip.LIB_PATH, so)
    subprocess.run([objdump, "--offloading", str(so)], cwd=tmp_path, check=True, capture_output=True)
    found = {}
    for o in sorted(p for p in tmp_path.iterdir() if "amdgcn" in p.name):
        notes = subprocess.run([readelf, "--notes", str(o)], check=True, capture_output=True, text=True).stdout
        # one metadata block per kernel: a list item that starts at `- .agpr_count` / `- .args` and holds `.name:`
        for block in re.split(r"\n\s+- \.", notes):
            m = re.search(r"\.?name:\s+(\S*dcn16t_kernel\S*)", block)
            if not m or ".kd" in m.group(1):
                continue
            get = lambda key: int(re.search(r"\.?%s:\s+(\d+)" % key, block).group(1))
            found[m.group(1)] = dict(vgpr=get("vgpr_count"), lds=get("group_segment_fixed_size"),
                                     scratch=get("private_segment_fixed_size"), spills=get("vgpr_spill_count"))
    assert len(found) == 2, sorted(found)   # dcn16t_kernel<2, false> and <2, true>
    for name, r in found.items():
        assert r["vgpr"] <= 168 and r["lds"] <= 53 * 1024 and r["scratch"] == 0 and r["spills"] == 0, (name, r)


def test_dcn16p_and_dcn16s_instances_fit_two_workgroups_per_cu(tmp_path):
    """dcn16p's two instances (64- and 128-wide N tile) and dcn16s keep the budget they are written for: two workgroups per CU = at
    most 256 VGPRs and 80 KB - 128 B of LDS, and no more scratch than the handful of spilled registers they are known to carry
    (0, 20 and 12 bytes).  Same mechanism as above."""
    objdump, readelf = _tool("llvm-objdump"), _tool("llvm-readelf")
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("llvm-objdump / llvm-readelf not available")
    so = tmp_path / "lib.so"
    shutil.copy(hip.LIB_PATH, so)
    subprocess.run([objdump, "--offloading", str(so)], cwd=tmp_path, check=True, capture_output=True)
    scratch_max = {"dcn16p_kernelILi2E": 0, "dcn16p_kernelILi4E": 20, "dcn16s_kernelILi2E": 12}  # mangled: <NT>
    found = {}
    for o in sorted(p for p in tmp_path.iterdir() if "amdgcn" in p.name):
        notes = subprocess.run([readelf, "--notes", str(o)], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n\s+- \.", notes):
            m = re.search(r"\.?name:\s+(\S*dcn16[ps]_kernel\S*)", block)
            if not m or ".kd" in m.group(1):
                continue
            get = lambda key: int(re.search(r"\.?%s:\s+(\d+)" % key, block).group(1))
            found[m.group(1)] = dict(vgpr=get("vgpr_count"), lds=get("group_segment_fixed_size"),
                                     scratch=get("private_segment_fixed_size"))
    assert len(found) == 3, sorted(found)
    for inst, scratch in scratch_max.items():
        (name, r), = [(n, r) for n, r in found.items() if inst in n]
        assert r["vgpr"] <= 256 and r["lds"] <= 80 * 1024 - 128 and r["scratch"] <= scratch, (name, r)
