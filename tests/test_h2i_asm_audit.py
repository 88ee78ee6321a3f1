"""The in-place split kernel (trunk_kernel_h2i, variant 25) as compiled for gfx950 (hipcc -S of a
translation unit of its own, CPU only): its inline-asm MFMA chains are hazard-free
(tests/kernel_asm_audit.py), every instantiation fits the 256 registers of a wave at two waves per
SIMD, and its private segment is what profiles/h2i_resources.txt records.

Registers: the code object's metadata counts the unified file in .vgpr_count (architectural VGPRs
rounded up to the allocation granule, plus the AGPRs of .agpr_count), so the two bounds are
.vgpr_count <= 256 and, from the assembler's own report, NumVgprs + NumAgprs <= 256."""
import os
import re
import shutil
import subprocess

import pytest

import kernel_asm_audit as kaa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NN = os.path.join(ROOT, "galvanise_zero_amd", "csrc", "nn")
HIPCC = "/opt/rocm/bin/hipcc"
PTNS = (2, 3, 4)

TU = "#include \"trunk_variants.h\"\nnamespace gznn {\n" + "".join(
    "template __global__ void trunk_kernel_h2i<128, %d, 3>(KParams);\n" % p for p in PTNS) + "}\n"


def recorded_resources():
    """{position tiles: {column: value}} from profiles/h2i_resources.txt's table."""
    rows, cols = {}, None
    for line in open(os.path.join(ROOT, "profiles", "h2i_resources.txt")):
        f = line.split()
        if line.startswith("# columns:"):
            cols = f[2:]
        elif f and f[0] == "h2i":
            rows[int(f[1])] = dict(zip(cols[2:], (int(v) for v in f[2:])))
    return rows


def compiled_resources(asm):
    """Per kernel symbol: the metadata's counts and the assembler's NumVgprs / NumAgprs."""
    out = {}
    for m in re.finditer(r"\.agpr_count:\s+(\d+)(.*?)\.vgpr_spill_count:\s+(\d+)", asm, re.S):
        body = m.group(2)
        name = re.search(r"\.name:\s+(\S+)", body).group(1)
        out[name] = {"agpr_count": int(m.group(1)), "vgpr_spill_count": int(m.group(3)),
                     "vgpr_count": int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1)),
                     "private_segment_fixed_size": int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))}
    for name, r in out.items():
        tail = asm[asm.index(name + ":"):]
        r["num_vgprs"] = int(re.search(r"; NumVgprs: (\d+)", tail).group(1))
        r["num_agprs"] = int(re.search(r"; NumAgprs: (\d+)", tail).group(1))
    return out


def conv_loop_scratch(asm, name):
    """(innermost loops running MFMAs, scratch accesses inside them) of one kernel."""
    body = asm[asm.index(name + ":"):]
    lines = body[:body.index(".Lfunc_end")].split("\n")
    labels = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"(\.LBB\d+_\d+):", l)] if m}
    spans = []
    for i, l in enumerate(lines):
        m = re.search(r"s_cbranch\w+\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i) < i:
            spans.append((labels[m.group(1)], i))
    inner = [s for s in spans if not any(t != s and s[0] <= t[0] and t[1] <= s[1] for t in spans)]
    loops = [lines[a:b] for a, b in inner if sum("v_mfma" in x for x in lines[a:b]) >= 9]
    return len(loops), sum("scratch_" in x for body_ in loops for x in body_)


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc absent")
def test_h2i_chains_registers_and_private_segment(tmp_path):
    src = tmp_path / "h2i_tu.hip"
    src.write_text(TU)
    out = tmp_path / "h2i_tu.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-parameter",
                           "-ffp-contract=on", "--cuda-device-only", "-S", "-I", NN, "-o", str(out), str(src)],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = out.read_text()
    res = kaa.audit(asm)
    assert len(res) == len(PTNS), sorted(res)
    for name, (n, bad) in res.items():
        assert n > 0
        assert bad == [], (name, bad[:5])
    got = compiled_resources(asm)
    rec = recorded_resources()
    assert sorted(rec) == list(PTNS)
    for ptn in PTNS:
        name, = [k for k in got if "trunk_kernel_h2iILi128ELi%dELi3E" % ptn in k]
        r = got[name]
        print("h2i<128, %d, 3>: %s" % (ptn, r))
        assert r["vgpr_count"] <= 256                      # the unified file: two waves per SIMD
        assert r["num_vgprs"] + r["num_agprs"] <= 256
        assert r["private_segment_fixed_size"] == rec[ptn]["private_segment_fixed_size"]
        loops, scratch = conv_loop_scratch(asm, name)
        assert loops >= 2                                  # the tower's two convs
        assert scratch == 0                                # no scratch or spill access inside a conv loop
