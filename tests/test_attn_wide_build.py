"""CPU test (no GPU): the compiler's resource figures of every attention kernel in csrc/dmc_attn.hip.

The 128-wide head-dim pad (head dims 72..128) puts the row-resident kernels next to two limits: 256 registers per lane
for a 512-thread block, and 160 KB of LDS. A kernel that goes over the first still compiles, with its excess spilled to
scratch memory (the bf16 resident dK/dV kernel with dropout did, before its tile body was split into per-chunk passes:
DESIGN.md section 3, "Head dims up to 128"). This compiles the file for gfx950 with the flags of build.py plus
-Rpass-analysis=kernel-resource-usage and holds every kernel to no scratch and an LDS size within the limit, and asks
for the 128-wide instantiations by name. It reads the remarks only, no instructions."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

HIPCC = "/opt/rocm/bin/hipcc"
LDS_LIMIT = 163840
FORMS = ("attn_fwd_kernel", "attn_dq_kernel", "attn_dkdv_kernel", "attn_fwd_res_kernel", "attn_dq_res_kernel",
         "attn_dkdv_res_kernel")


def parse_remarks(text):
    """-Rpass-analysis=kernel-resource-usage output -> {mangled name: {field: int}}."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        # "remark: file:line:col:     VGPRs: 98 [-R...]" or "file:line:col: remark:     VGPRs: 98 [-R...]"
        m = re.search(r"remark:(?: \S+:\d+:\d+:)?\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass-analysis", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def kernel_id(mangled):
    """(template name, 'fp32' | 'bf16', HDP, DROP or None) of an attention kernel's mangled name, None for anything
    else."""
    m = re.search(r"\d+(attn_\w+?_kernel)I(\w+?)Li(\d+)E(?:Lb([01])E)?", mangled)
    if not m:
        return None
    return m.group(1), "fp32" if m.group(2) == "f" else "bf16", int(m.group(3)), m.group(4) and int(m.group(4))


def test_parse_remarks():
    text = ("remark: a.hip:5:0: Function Name: _ZN12_GLOBAL__N_119attn_fwd_res_kernelItLi128ELb1EEEvNS_5AttnKEii "
            "[-Rpass-analysis=kernel-resource-usage]\n"
            "remark: a.hip:5:0:     VGPRs: 130 [-Rpass-analysis=kernel-resource-usage]\n"
            "a.hip:5:1: remark:     ScratchSize [bytes/lane]: 36 [-Rpass-analysis=kernel-resource-usage]\n"
            "remark: a.hip:5:0:     LDS Size [bytes/block]: 139264 [-Rpass-analysis=kernel-resource-usage]\n")
    r = parse_remarks(text)
    (name, f), = r.items()
    assert kernel_id(name) == ("attn_fwd_res_kernel", "bf16", 128, 1)
    assert f == {"VGPRs": 130, "ScratchSize": 36, "LDS Size": 139264}
    assert kernel_id("_ZN12_GLOBAL__N_115attn_fwd_kernelIfLi32EEEvNS_5AttnKE") == ("attn_fwd_kernel", "fp32", 32, None)
    assert kernel_id("_Z9something") is None


@pytest.mark.skipif(not Path(HIPCC).exists() and shutil.which("hipcc") is None, reason="hipcc not available")
def test_attention_kernels_fit_registers_and_lds(tmp_path):
    from diffusion_models_collection_amd import build as B
    src = B.CSRC / "dmc_attn.hip"
    common = ["--offload-arch=gfx950" if f.startswith("--offload-arch=") else f for f in B.COMMON]
    cmd = ([HIPCC if Path(HIPCC).exists() else "hipcc"] + common + B.EXTRA.get("dmc_attn.hip", [])
           + ["-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", str(tmp_path / "dmc_attn.o")])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = {kernel_id(n): f for n, f in parse_remarks(r.stderr).items() if kernel_id(n)}
    assert kernels, r.stderr[-2000:]
    for (name, dt, hdp, drop), f in sorted(kernels.items(), key=str):
        print(f"attn-resources {name} {dt} HDP {hdp} DROP {drop}: VGPRs {f.get('VGPRs')} AGPRs {f.get('AGPRs')} "
              f"scratch {f.get('ScratchSize')} LDS {f.get('LDS Size')} occupancy {f.get('Occupancy')}")
    have = {k[:3] for k in kernels}
    for dt in ("fp32", "bf16"):
        for hdp in (32, 64, 128):
            forms = FORMS[:3] if (dt == "fp32" and hdp > 64) else FORMS   # fp32 above 64 is staged only
            for name in forms:
                assert (name, dt, hdp) in have, f"no {name}<{dt}, {hdp}>"
    bad = [(k, f) for k, f in kernels.items()
           if f.get("ScratchSize", -1) != 0 or f.get("VGPRs Spill", -1) != 0 or not 0 <= f.get("LDS Size", -1) <= LDS_LIMIT]
    assert not bad, bad
