"""CPU tests (no GPU) of the pooled second output of pw16s_kernel (pw16.hip) and lowc1s_kernel (lowc.hip), read from the built
library: the POOL instances' resource use from the code objects' notes, and the plain instances' size from the disassembly."""
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as ge
from centerpose_amd import hip

LLVM = "/opt/rocm/lib/llvm/bin"

# instructions of the plain (POOL = false) instances in the commit before the pooled output existed, where they were the only
# instances: the template parameter must leave them as they were
PLAIN_INSTRUCTIONS = {"pw16s_kernelILi2ELb0E": 5979, "pw16s_kernelILi4ELb0E": 10633, "lowc1s_kernelILb0E": 1369}
POOLED = ("pw16s_kernelILi2ELb1E", "pw16s_kernelILi4ELb1E", "lowc1s_kernelILb1E")


def _tool(name):
    path = shutil.which(name) or os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.skip(name + " not available")
    return path


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    """(notes per kernel name, instruction count per function) over the code objects that hold the two kernels"""
    ge.build()
    objdump, readelf = _tool("llvm-objdump"), _tool("llvm-readelf")
    d = tmp_path_factory.mktemp("pooled_store")
    shutil.copy(hip.LIB_PATH, d / "lib.so")
    subprocess.run([objdump, "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
    notes, counts = {}, {}
    head = re.compile(r"^[0-9a-f]+ <(\S+)>:$")
    inst = re.compile(r"^\s+\S+.*//\s*[0-9A-Fa-f]+:")
    for o in sorted(p for p in d.iterdir() if "amdgcn" in p.name):
        text = subprocess.run([readelf, "--notes", str(o)], check=True, capture_output=True, text=True).stdout
        if "pw16s_kernel" not in text and "lowc1s_kernel" not in text:
            continue
        # one record per kernel: a YAML list item ("  - .agpr_count: ...") whose keys are sorted, .name among them
        for rec in re.split(r"\n\s+- (?=\.agpr_count|\.args)", text):
            name = re.search(r"\.name:\s+(_Z\S+)", rec)
            if name:
                notes[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", rec, flags=re.M)}
        fn = None
        for line in subprocess.run([objdump, "-d", "--no-show-raw-insn", str(o)], check=True, capture_output=True, text=True).stdout.splitlines():
            m = head.match(line)
            if m:
                fn = m.group(1)
                counts[fn] = 0
            elif fn and inst.match(line):
                counts[fn] += 1
    return notes, counts


def _one(table, key):
    hits = [k for k in table if key in k]
    assert len(hits) == 1, (key, hits)
    return table[hits[0]]


def test_pooled_instances_use_no_scratch_and_spill_nothing(code_objects):
    notes, _ = code_objects
    for key in POOLED:
        n = _one(notes, key)
        print(key, {k: n[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")})
        assert n["private_segment_fixed_size"] == 0 and n["vgpr_spill_count"] == 0 and n["sgpr_spill_count"] == 0, (key, n)


def test_pooled_64_wide_tile_keeps_three_waves_per_simd(code_objects):
    """512 vector registers per SIMD lane / 3 waves, in allocation granules of 8: 168"""
    notes, _ = code_objects
    n = _one(notes, "pw16s_kernelILi2ELb1E")
    assert n["vgpr_count"] + n.get("agpr_count", 0) <= 168, n


def test_plain_instances_are_the_instructions_they_were(code_objects):
    _, counts = code_objects
    for key, want in PLAIN_INSTRUCTIONS.items():
        assert _one(counts, key) == want, (key, _one(counts, key), want)
