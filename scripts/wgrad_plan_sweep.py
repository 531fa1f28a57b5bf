"""Run every case of the weight-gradient plan table (tests/test_wgrad_plan_host.py CASES, then GROUPS) once, in table
order, with seeded random operands: a case through dmc_conv2d_wgrad_partial + dmc_wgrad_reduce_batch, a group through
dmc_conv2d_wgrad_group + dmc_wgrad_reduce_batch. Prints one line per case with the sha256 of dw and dbias, the fields
of the returned dmc_wgrad_job (pointers as offsets into the workspace) and the three host queries' answers.

Two trees that plan the same way print the same lines, and under `rocprofv3 --kernel-trace -- python
scripts/wgrad_plan_sweep.py` give the same sequence of (kernel, grid, workgroup). With --trace CSV it instead checks
such a trace against the table's expected columns (the partial-sum kernel's name, grid and block of every case):
    python scripts/wgrad_plan_sweep.py [--only NAME]
    python scripts/wgrad_plan_sweep.py --trace kernel_trace.csv
It needs nothing newer than the entry points the table was recorded from, so it runs on that commit as well.
"""
import argparse
import csv
import ctypes
import hashlib
import re
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from diffusion_models_collection_amd import _lib as L  # noqa: E402
from test_wgrad_plan_host import CASES, GROUPS, case_desc, group_items  # noqa: E402

WGRAD_KERNELS = re.compile(r"^(wgrad3x3_|wgrad1x1_|conv_wgrad_kernel)")
LIB = L.LIB


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def job_fields(j, ws):
    off = lambda p: "-" if not p else p - ws.data_ptr()   # noqa: E731
    return (f"splits {j.splits} KK {j.KK} Cpad {j.Cpad} Cout {j.Cout} Ctot {j.Ctot} ntaps {j.ntaps} Kc {j.Kc} "
            f"layout {j.layout} slab {off(j.slab)} bslab {off(j.bslab)}")


def make_alloc(gen):
    def alloc(name, shape, dtype):
        if name in ("dw", "dbias"):   # outputs: NaN-filled, so an unwritten element shows in the hash
            return torch.full(shape, float("nan"), dtype=dtype, device="cuda")
        return (torch.randn(shape, generator=gen) * (0.5 if name == "dy" else 1.0)).to(dtype).to("cuda")
    return alloc


def run(only):
    alloc = make_alloc(torch.Generator().manual_seed(4321))
    for c in CASES:
        L.reset_options(False)
        for name, v in c["opts"].items():
            L.set_option(name, v)
        d, ld_dy, ops = case_desc(c, alloc)   # every case draws its operands: --only does not shift the others' seeds
        if only and c["name"] != only:
            continue
        nbytes = LIB.dmc_conv2d_wgrad_workspace(ctypes.byref(d))
        group_ok = LIB.dmc_conv2d_wgrad_group_ok(ctypes.byref(d), ld_dy)
        ws = torch.zeros(max(nbytes, 256), dtype=torch.uint8, device="cuda")
        job = L.WgradJob()
        L.check(LIB.dmc_conv2d_wgrad_partial(ctypes.byref(d), L.ptr(ops["dy"]), ld_dy, L.ptr(ops["x1"]),
                                             L.ptr(ops["x2"]), L.ptr(ws), L.ptr(ops["dw"]), 0.5, ctypes.byref(job),
                                             L.stream()), "dmc_conv2d_wgrad_partial")
        L.check(LIB.dmc_wgrad_reduce_batch(ctypes.byref(job), 1, L.stream()), "dmc_wgrad_reduce_batch")
        torch.cuda.synchronize()
        print(f"{c['name']:18s} dw {sha(ops['dw'])} dbias {sha(ops['dbias'])} {job_fields(job, ws)} ws {nbytes} "
              f"group_ok {group_ok}", flush=True)
    for g, (opts, jobs, _) in GROUPS.items():
        L.reset_options(False)
        for name, v in opts.items():
            L.set_option(name, v)
        arr, descs, opss = group_items(jobs, alloc)
        if only and g != only:
            continue
        n = len(jobs)
        sizes = (ctypes.c_size_t * n)()
        total = LIB.dmc_conv2d_wgrad_group_workspace(arr, n, sizes)
        ws = torch.zeros(max(total, 256), dtype=torch.uint8, device="cuda")
        off = 0
        for i in range(n):
            arr[i].workspace = ws.data_ptr() + off
            off += sizes[i]
        out = (L.WgradJob * n)()
        L.check(LIB.dmc_conv2d_wgrad_group(arr, n, out, L.stream()), "dmc_conv2d_wgrad_group")
        L.check(LIB.dmc_wgrad_reduce_batch(out, n, L.stream()), "dmc_wgrad_reduce_batch")
        torch.cuda.synchronize()
        for i in range(n):
            print(f"{g + '.' + str(i):18s} dw {sha(opss[i]['dw'])} dbias {sha(opss[i]['dbias'])} "
                  f"{job_fields(out[i], ws)} bytes {sizes[i]}", flush=True)
    L.reset_options(False)


def check_trace(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    got = []
    for r in rows:
        name = re.sub(r"\(anonymous namespace\)::", "", r["Kernel_Name"])
        name = re.sub(r"^void ", "", re.sub(r"\((?!\)).*$", "", name))
        if WGRAD_KERNELS.search(name):
            wg = int(r["Workgroup_Size_X"])
            got.append((name, tuple(int(r[f"Grid_Size_{a}"]) // (wg if a == "X" else 1) for a in "XYZ"), wg))
    want = [(c["name"], c["kernel"], c["grid"], c["block"]) for c in CASES]
    bad = 0
    for i, w in enumerate(want):
        g = got[i] if i < len(got) else None
        ok = g is not None and g == w[1:]
        bad += not ok
        print(f"{'ok      ' if ok else 'MISMATCH'} {w[0]:18s} want {w[1:]} got {g}")
    for g in got[len(want):]:   # the grouped calls' launches: compared between two trees, not against the table
        print(f"group    {g}")
    print(f"{len(want)} table launches, {len(got)} traced, {bad} mismatches")
    return 1 if bad or len(got) < len(want) else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--trace", default=None)
    a = ap.parse_args()
    sys.exit(check_trace(a.trace) if a.trace else run(a.only))
