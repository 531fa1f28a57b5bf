"""Host equivalence sweep of the weight-gradient queries: a seeded generator of descriptors x option sets, and random
groups of 1..8 jobs, each answered by the three host-only queries every revision has (dmc_conv2d_wgrad_workspace,
dmc_conv2d_wgrad_group_ok, dmc_conv2d_wgrad_group_workspace with bytes[]). One line per question on stdout, a tally
by answer on stderr. Two builds that plan the same way print the same stdout:
    python scripts/wgrad_host_sweep.py --root TREE_A > a.txt; python scripts/wgrad_host_sweep.py --root TREE_B > b.txt
    cmp a.txt b.txt
--root is the checkout whose package (and libdmc.so) answers; default: this one. --table prints the host columns of
tests/test_wgrad_plan_host.py's table instead (what the table's ws / group / bytes[] columns were recorded with).
No GPU: the queries touch no device.
"""
import argparse
import collections
import ctypes
import random
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parents[1]
OPTS = {"DMC_NO_HALO": (0, 0, 0, 1), "DMC_WG_PIPE": (1, 1, 1, 0), "DMC_WG_IMG4": (1, 1, 0),
        "DMC_WG_HALO_TARGET": (256, 256, 2, 20, 44, 128, 1000), "DMC_WG_BLOCKS": (512, 512, 1, 64, 4096),
        "DMC_WG_MINPIX": (0, 0, 100, 512, 4096)}


def rand_job(rng):
    """(dtype, N, map, C1, C2, Cout, taps, stride, prologue, ld_dy slack): shapes around the dispatch's thresholds."""
    if rng.random() < 0.5:   # half the draws from the shapes the models run: the DMA kinds' neighbourhood
        S = rng.choice((1, 4, 8, 16, 32, 64))
        N = rng.choice((1, 2, 4, 6, 32, 128)) * (rng.choice((1, 64)) if S == 1 else 1)
        C1 = rng.choice((64, 128, 256))
        return (torch.bfloat16, N, S, C1, rng.choice((0, 0, 64, 128)) if C1 == 128 else 0,
                rng.choice((3, 64, 128, 192, 256, 512)), rng.choice("3331"), 1, False, rng.choice((0, 0, 8)))
    dt = torch.bfloat16 if rng.random() < 0.85 else torch.float32
    taps = rng.choice("33331d")
    S = rng.choice((1, 2, 4, 4, 8, 8, 16, 16, 32, 64))
    N = rng.choice((1, 2, 3, 4, 5, 8, 16, 32, 64, 128, 256))
    if S == 1:
        N *= rng.choice((1, 8, 64))
    C1 = rng.choice((3, 8, 16, 24, 32, 64, 64, 64, 128, 128, 192, 256, 512))
    C2 = rng.choice((0, 0, 0, 8, 64, 128)) if C1 % 8 == 0 else 0
    Cout = rng.choice((3, 8, 16, 24, 64, 64, 72, 128, 200, 256, 512, 1024))
    stride = 2 if taps == "3" and S >= 2 and rng.random() < 0.1 else 1
    pro = rng.random() < 0.08
    return dt, N, S, C1, C2, Cout, taps, stride, pro, rng.choice((0, 0, 0, 8, 4))


def desc_of(job, L, K):
    dt, N, S, C1, C2, Cout, taps, stride, pro, slack = job
    epc = L.chunk_for(dt)
    ld1 = (C1 + epc - 1) // epc * epc
    ld_dy = (Cout + epc - 1) // epc * epc + slack
    t = {"3": K.TAPS3, "d": K.TAPS3_DGRAD, "1": K.TAPS1}[taps]
    OS = S // stride
    d = K.make_desc(dt, N, S, S, C1, C2, ld1, C2, L.kc_for(C1 + C2, dt), OS, OS, Cout, t, stride=stride)
    if pro and C1 % epc == 0:
        K.set_prologue(d, L.PRO_SILU)
    return d, ld_dy


def sweep(L, K, n, seed):
    rng = random.Random(seed)
    tally = collections.Counter()
    for q in range(n):
        L.reset_options(False)
        opts = {k: rng.choice(v) for k, v in OPTS.items()}
        for k, v in opts.items():
            L.set_option(k, v)
        job = rand_job(rng)
        d, ld_dy = desc_of(job, L, K)
        ws = L.LIB.dmc_conv2d_wgrad_workspace(ctypes.byref(d))
        ok = L.LIB.dmc_conv2d_wgrad_group_ok(ctypes.byref(d), ld_dy)
        tally[f"group_ok {ok}"] += 1
        print(f"d {q} ws {ws} group_ok {ok}")
        if hasattr(K, "wgrad_plan"):   # a tree with the planner's export: the breakdown by kind (stderr only)
            p = L.WgradPlan()
            rc = L.LIB.dmc_conv2d_wgrad_plan(ctypes.byref(d), ld_dy, ctypes.byref(p))
            tally["kind " + ("rejected" if rc else L.WGRAD_KINDS[p.kind])] += 1
        # a group around this job: the same kind where it has one (other channels / batch), random jobs otherwise
        njobs = rng.randint(1, 8)
        arr, keep = (L.WgradGroupItem * njobs)(), []
        for i in range(njobs):
            if ok and i and rng.random() < 0.9:
                dt, N, S, C1, C2, Cout, taps, stride, pro, slack = job
                C1b = rng.choice((64, 128, 256, 512))
                jb = (dt, rng.choice((N, 2 * N)), S if ok != 1 else rng.choice((S, 8, 16)), C1b,
                      rng.choice((0, 0, 64 if ok != 1 else 8)) if C1b % 128 == 0 or ok != 1 else 0,
                      rng.choice((Cout, 64, 128, 256, 512)), taps, 1, False, slack)
            else:
                jb = job if i == 0 else rand_job(rng)
            di, ldi = desc_of(jb, L, K)
            keep.append(di)
            arr[i].d, arr[i].ld_dy = ctypes.pointer(di), ldi
        sizes = (ctypes.c_size_t * njobs)()
        total = L.LIB.dmc_conv2d_wgrad_group_workspace(arr, njobs, sizes)
        tally["group valid" if total else "group refused"] += 1
        print(f"g {q} n {njobs} total {total} bytes {list(sizes) if total else []}")
    L.reset_options(False)
    for k in sorted(tally):
        print(f"{k}: {tally[k]}", file=sys.stderr)


def table(L, K):
    sys.path.insert(0, str(HERE / "tests"))
    from test_wgrad_plan_host import CASES, GROUPS, case_desc, group_items
    for c in CASES:
        L.reset_options(False)
        for k, v in c["opts"].items():
            L.set_option(k, v)
        d, ld_dy, _ = case_desc(c)
        print(f"{c['name']:18s} ws {L.LIB.dmc_conv2d_wgrad_workspace(ctypes.byref(d))} "
              f"group_ok {L.LIB.dmc_conv2d_wgrad_group_ok(ctypes.byref(d), ld_dy)}")
    for g, (opts, jobs, _) in GROUPS.items():
        L.reset_options(False)
        for k, v in opts.items():
            L.set_option(k, v)
        arr, _, _ = group_items(jobs)
        sizes = (ctypes.c_size_t * len(jobs))()
        total = L.LIB.dmc_conv2d_wgrad_group_workspace(arr, len(jobs), sizes)
        print(f"{g:18s} total {total} bytes {list(sizes)}")
    L.reset_options(False)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=str(HERE))
    ap.add_argument("-n", type=int, default=6000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    from diffusion_models_collection_amd import _lib as L, kernels as K
    table(L, K) if a.table else sweep(L, K, a.n, a.seed)
