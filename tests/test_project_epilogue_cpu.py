"""halo16's instances with the level entry's 1x1 projection in the epilogue (halo16_kernel<..., PJ = true>) keep the budget of the
plain instances they stand in for: the 128-wide tile two workgroups per CU (at most 256 VGPRs), the 64-wide tile three (at most
168), 51904 bytes of LDS, nothing in scratch, no spills.  Read from the metadata notes of the built library's code objects;
needs no GPU."""
import os
import re
import shutil
import subprocess

import pytest

from centerpose_amd import hip


def _tool(name):
    return shutil.which(name) or os.path.join("/opt/rocm/lib/llvm/bin", name)


def test_halo16_projection_instances_keep_their_budget(tmp_path):
    objdump, readelf = _tool("llvm-objdump"), _tool("llvm-readelf")
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("llvm-objdump / llvm-readelf not available")
    so = tmp_path / "lib.so"
    shutil.copy(hip.LIB_PATH, so)
    subprocess.run([objdump, "--offloading", str(so)], cwd=tmp_path, check=True, capture_output=True)
    found = {}
    for o in sorted(p for p in tmp_path.iterdir() if "amdgcn" in p.name):
        notes = subprocess.run([readelf, "--notes", str(o)], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n\s+- \.", notes):
            m = re.search(r"\.?name:\s+(\S*halo16_kernel\S*)", block)
            if not m or ".kd" in m.group(1):
                continue
            get = lambda key: int(re.search(r"\.?%s:\s+(\d+)" % key, block).group(1))
            found[m.group(1)] = dict(vgpr=get("vgpr_count"), lds=get("group_segment_fixed_size"),
                                     scratch=get("private_segment_fixed_size"), spills=get("vgpr_spill_count"))
    # mangled template arguments <MT, NT, WM, WN, BDIRECT, EPI, FT, PJ>
    budget = {"ILi2ELi2ELi2ELi2ELb1ELi0ELi0ELb1EE": 256, "ILi2ELi1ELi2ELi2ELb1ELi0ELi0ELb1EE": 168,
              "ILi2ELi2ELi2ELi2ELb1ELi0ELi0ELb0EE": 256, "ILi2ELi1ELi2ELi2ELb1ELi0ELi0ELb0EE": 168}
    for inst, vmax in budget.items():
        hit = [(n, r) for n, r in found.items() if inst in n]
        assert len(hit) == 1, (inst, sorted(found))
        name, r = hit[0]
        assert r["vgpr"] <= vmax and r["lds"] <= 51904 and r["scratch"] == 0 and r["spills"] == 0, (name, r)
    assert sum("ELb1EEEv10ConvParams" in n for n in found) == 2, sorted(found)  # PJ: those two instances only
