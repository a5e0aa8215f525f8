"""The small-channel conv kernels keep the registers, LDS and occupancy they were recorded with.

A refactor of shared device code can move a kernel's register allocation without changing one output bit: an accumulator array that goes
to scratch, or one VGPR more on a kernel that sits exactly at an occupancy step (convt_rows_kernel<3, 2, true, 4, false>: 128 VGPRs,
4 waves per SIMD), is invisible to every parity test.  hipcc cross-compiles without a GPU, so this compiles the five sources for gfx950
with the resource remarks on and compares them, kernel by kernel (mangled name), with tests/golden/smallc_resources.json."""
import json
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "collaborative-gan-sampling_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "smallc_resources.json")
SOURCES = ("convt_quad.hip", "conv_patch.hip", "convt_taps.hip", "convt_smalln.hip", "conv_smalln_f.hip")
# remark text -> fixture key.  TotalSGPRs is recorded and printed, not asserted: it does not bound occupancy on gfx950, and a renamed
# scalar can move it by one.
FIELDS = {"TotalSGPRs": "TotalSGPRs", "VGPRs": "VGPRs", "AGPRs": "AGPRs", "ScratchSize [bytes/lane]": "ScratchSize",
          "SGPRs Spill": "SGPRSpill", "VGPRs Spill": "VGPRSpill", "Occupancy [waves/SIMD]": "Occupancy", "LDS Size [bytes/block]": "LDSSize"}
ASSERTED = ("VGPRs", "AGPRs", "ScratchSize", "SGPRSpill", "VGPRSpill", "Occupancy", "LDSSize")
# zero everywhere: scratch and spilled vector registers.  SGPR spills go to VGPR lanes, not to memory, and seven of the recorded kernels have
# some (conv_smalln_f_kernel<4>: 32): they are held to their recorded count, not to zero.
ZERO = ("ScratchSize", "VGPRSpill")


def parse_remarks(text):
    """{mangled kernel name: {field: int}} from the stderr of -Rpass-analysis=kernel-resource-usage"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?): (\d+)\b", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return out


def compile_remarks(src):
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                          "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", os.path.join(CSRC, src), "-o", os.devnull],
                         capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-2000:]
    return parse_remarks(out.stderr)


def test_small_channel_kernels_keep_their_recorded_resources():
    with open(GOLDEN) as f:
        golden = json.load(f)
    with ThreadPoolExecutor(len(SOURCES)) as pool:       # (the compiles are child processes: the threads only wait)
        parsed = dict(zip(SOURCES, pool.map(compile_remarks, SOURCES)))
    assert sorted(parsed) == sorted(golden)
    bad = []
    for src in SOURCES:
        now, then = parsed[src], golden[src]
        assert sorted(now) == sorted(then), (src, sorted(set(now) ^ set(then)))
        for name in sorted(now):
            print(src, name, now[name], "recorded SGPRs", then[name].get("TotalSGPRs"))
            assert set(now[name]) == set(FIELDS.values()), (src, name, now[name])
            for k in ASSERTED:
                if now[name][k] != then[name][k]:
                    bad.append((src, name, k, then[name][k], now[name][k]))
            for k in ZERO:
                if now[name][k] != 0:
                    bad.append((src, name, k, 0, now[name][k]))
    assert not bad, "\n".join("%s: %s: %s recorded %d, now %d" % b for b in bad)
    assert sum(len(v) for v in parsed.values()) >= 58
