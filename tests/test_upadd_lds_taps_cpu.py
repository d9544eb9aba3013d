"""dcn16t's up-sample + add epilogue reads its taps of t from LDS (dcn16t.hip, UPADD: the rectangle of t behind the workgroup's patch
is staged once, beside the weight table).  Read from the built library's gfx950 code object, no GPU:
  * the UPADD instance keeps the kernel's budget -- at most 168 VGPRs, nothing in scratch, no spills -- and no more LDS than the
    instance before the change (45684 bytes: three workgroups per CU);
  * the plain instance dcn16t_kernel<2, false> is, instruction for instruction, what it was before the change;
  * behind its last MFMA the UPADD instance issues fewer vector-memory loads than before the change (53: 32 taps of t per lane, 16
    of scale / shift, 4 of the table, 1 of the |max| commit).
What "before the change" was is recorded in tests/golden/dcn16t_upadd_lds_taps.json (instruction count and SHA-256 of the plain
instance's disassembly without addresses and encodings; LDS bytes and load count of the UPADD instance), taken from the parent
commit's library built with the same flags."""
import hashlib
import json
import os
import re
import shutil
import subprocess

import pytest

from centerpose_amd import hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dcn16t_upadd_lds_taps.json")
PLAIN, UPADD = "dcn16t_kernelILi2ELb0EE", "dcn16t_kernelILi2ELb1EE"  # mangled <NT, UPADD>


def _tool(name):
    return shutil.which(name) or os.path.join("/opt/rocm/lib/llvm/bin", name)


@pytest.fixture(scope="module")
def instances(tmp_path_factory):
    """{mangled name: metadata + `ins`, the instruction stream} of dcn16t's two instances"""
    objdump, readelf = _tool("llvm-objdump"), _tool("llvm-readelf")
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("llvm-objdump / llvm-readelf not available")
    tmp = tmp_path_factory.mktemp("dcn16t_isa")
    so = tmp / "lib.so"
    shutil.copy(hip.LIB_PATH, so)
    subprocess.run([objdump, "--offloading", str(so)], cwd=tmp, check=True, capture_output=True)
    found = {}
    for o in sorted(p for p in tmp.iterdir() if "amdgcn" in p.name):
        notes = subprocess.run([readelf, "--notes", str(o)], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n\s+- \.", notes):
            m = re.search(r"\.?name:\s+(\S*dcn16t_kernel\S*)", block)
            if not m or ".kd" in m.group(1):
                continue
            get = lambda key: int(re.search(r"\.?%s:\s+(\d+)" % key, block).group(1))
            found[m.group(1)] = dict(vgpr=get("vgpr_count"), lds=get("group_segment_fixed_size"),
                                     scratch=get("private_segment_fixed_size"), spills=get("vgpr_spill_count"), ins=[])
        if not found:
            continue
        dis = subprocess.run([objdump, "-d", "--no-show-raw-insn", "--no-leading-addr", str(o)],
                             check=True, capture_output=True, text=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^\S*\s*<(\S+)>:\s*$", line)
            if m:
                cur = found.get(m.group(1))
            elif cur is not None and line.strip():
                cur["ins"].append(re.sub(r"\s+", " ", line.split("//")[0].strip()))
    assert len(found) == 2 and all(r["ins"] for r in found.values()), sorted(found)
    return found


def _one(instances, inst):
    (name, r), = [(n, r) for n, r in instances.items() if inst in n]
    return r


def _vmem_loads_after_last_mfma(ins):
    last = max(i for i, s in enumerate(ins) if s.startswith("v_mfma"))
    return sum(1 for s in ins[last + 1:] if re.match(r"(buffer|global|flat)_load", s))


def test_upadd_instance_keeps_its_budget(instances):
    gold = json.load(open(GOLDEN))
    r = _one(instances, UPADD)
    print("UPADD instance: %d VGPRs, %d B LDS, %d B scratch, %d spills" % (r["vgpr"], r["lds"], r["scratch"], r["spills"]))
    assert r["vgpr"] <= 168 and r["scratch"] == 0 and r["spills"] == 0, r["vgpr"]
    assert r["lds"] <= gold["upadd_lds_bytes"] <= 53 * 1024, r["lds"]


def test_plain_instance_is_instruction_for_instruction_the_parents(instances):
    gold = json.load(open(GOLDEN))
    ins = _one(instances, PLAIN)["ins"]
    sha = hashlib.sha256("\n".join(ins).encode()).hexdigest()
    print("plain instance: %d instructions, sha256 %s" % (len(ins), sha))
    assert len(ins) == gold["plain_instructions"], (len(ins), gold["plain_instructions"])
    assert sha == gold["plain_sha256"]


def test_upadd_epilogue_issues_fewer_vector_memory_loads(instances):
    gold = json.load(open(GOLDEN))
    n = _vmem_loads_after_last_mfma(_one(instances, UPADD)["ins"])
    n_plain = _vmem_loads_after_last_mfma(_one(instances, PLAIN)["ins"])
    print("vector-memory loads behind the last MFMA: UPADD %d (parent %d), plain %d" % (n, gold["upadd_vmem_loads_after_last_mfma"], n_plain))
    assert n < gold["upadd_vmem_loads_after_last_mfma"]
    # what is left: the plain epilogue's loads, the table's four pieces and the region's four
    assert n == n_plain + 8
