"""Run every case of the conv-plan table (tests/test_conv_plan_host.py CASES) once, in table order, through
kernels.conv with seeded random operands, and print one line per case with the sha256 of each output.

Two trees that dispatch the same way print the same lines, and under `rocprofv3 --kernel-trace -- python
scripts/conv_plan_sweep.py` give the same sequence of (kernel, grid, workgroup). With --trace CSV it instead
checks such a trace against the table's expected columns (main kernel, grid, block; then the split-K reduction
and the GroupNorm-partials pass where the case has them):
    python scripts/conv_plan_sweep.py [--only NAME]
    python scripts/conv_plan_sweep.py --trace kernel_trace.csv
"""
import argparse
import csv
import hashlib
import re
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from diffusion_models_collection_amd import _lib as L, kernels as K  # noqa: E402
from test_conv_plan_host import CASES, KERNEL, PASS, SPLITK, case_desc  # noqa: E402

CONV_KERNELS = re.compile(r"conv|gemm1x1|gn_part_kernel")
TYPE = {torch.bfloat16: "unsigned short", torch.float32: "float"}


def sha(t):
    if t is None:
        return "-"
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def run(only):
    gen = torch.Generator().manual_seed(1234)

    def alloc(name, shape, dtype):
        if name in ("y1", "y2", "y_pre", "part"):   # outputs: NaN-filled, so an unwritten element shows in the hash
            return torch.full(shape, float("nan"), dtype=dtype, device="cuda")
        amp = {"w": 0.05, "scale": 1.0, "shift": 0.1}.get(name, 1.0)
        t = torch.randn(shape, generator=gen) * amp + (1.0 if name == "scale" else 0.0)
        return t.to(dtype).to("cuda")

    for c in CASES:
        L.reset_options(False)
        for name, v in c["opts"].items():
            L.set_option(name, v)
        d, ops = case_desc(c, alloc)   # every case draws its operands, so --only does not shift the others' seeds
        if only and c["name"] != only:
            continue
        K.conv(d, ops["x1"], ops["x2"], ops["w"], ops["y1"], ops["y2"])
        torch.cuda.synchronize()
        print(f"{c['name']:20s} " + " ".join(f"{n} {sha(ops[o])}" for n, o in (("y1", "y1"), ("y2", "y2"), ("y_pre", "y_pre"),
                                                                              ("gn_part", "part"))), flush=True)
    L.reset_options(False)


def expected_launches(c):
    """(kernel, blocks, block) of every launch the table expects for a case."""
    ty = TYPE[c["dt"]]
    out = [(c["kernel"], c["grid"], c["block"])]
    if c["splits"] > 1:
        name = "conv_splitk_epi_gn_kernel" if c["gn_mode"] == SPLITK else "conv_splitk_epilogue_kernel"
        out.append((f"{name}<{ty}, {c['splits']}>", None, 256))
    if c["gn_mode"] == PASS:
        out.append((f"gn_part_kernel<{ty}>", None, 256))
    return out


def check_trace(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    got = []
    for r in rows:
        name = re.sub(r"\(anonymous namespace\)::", "", r["Kernel_Name"])
        name = re.sub(r"^void ", "", re.sub(r"\((?!\)).*$", "", name))
        if CONV_KERNELS.search(name) and not name.startswith("at::"):
            wg = int(r["Workgroup_Size_X"])
            got.append((name, tuple(int(r[f"Grid_Size_{a}"]) // (wg if a == "X" else 1) for a in "XYZ"), wg))
    want = [(c["name"],) + e for c in CASES for e in expected_launches(c)]
    bad = 0
    for i, w in enumerate(want):
        g = got[i] if i < len(got) else None
        ok = g is not None and g[0] == w[1] and (w[2] is None or g[1] == w[2]) and g[2] == w[3]
        bad += not ok
        print(f"{'ok      ' if ok else 'MISMATCH'} {w[0]:20s} want {w[1:]} got {g}")
    print(f"{len(want)} expected launches, {len(got)} traced, {bad} mismatches")
    return 1 if bad or len(got) != len(want) else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--trace", default=None)
    a = ap.parse_args()
    sys.exit(check_trace(a.trace) if a.trace else run(a.only))
