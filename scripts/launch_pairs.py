"""Pair the launches of two rocprofv3 kernel traces of the same graphed train step, position by position, and list
the positions whose kernel changed: per (old kernel, old grid, new kernel, new grid) the launches per step and the
mean time of each side. The step is the same work in the same order in both traces; a launch that exists on one
side only (a split-K reduction whose conv no longer splits) is charged to the launch before it.
usage: launch_pairs.py old_kernel_trace.csv new_kernel_trace.csv [N steps] [--all]"""
import collections
import csv
import re
import sys

FOLLOWERS = ("conv_splitk_epilogue_kernel", "conv_splitk_epi_gn_kernel")


def name_of(r):
    n = r["Kernel_Name"].replace("void ", "").replace("(anonymous namespace)::", "")
    m = re.match(r"[\w:]+(<[^()]*>)?", n)
    return m.group(0) if m else n[:40]


def blocks_of(r):
    def dim(prefix):
        if prefix + "_X" in r:
            return [int(r[prefix + s]) for s in ("_X", "_Y", "_Z")]
        return [int(r[prefix]), 1, 1]
    g, w = dim("Grid_Size"), dim("Workgroup_Size")
    n = 1
    for a, b in zip(g, w):
        n *= max(1, a // max(1, b))
    return n


def steps_of(path, nsteps):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    idx = [i for i, r in enumerate(rows) if "adamw" in r["Kernel_Name"]][-(nsteps + 1):]
    out = []
    for a, b in zip(idx[:-1], idx[1:]):
        seq = []
        for r in rows[a + 1: b + 1]:
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            n = name_of(r)
            if seq and n.split("<")[0] in FOLLOWERS:
                seq[-1][2] += us
                seq[-1][3] += "+" + n.split("<")[0]
            else:
                seq.append([n, blocks_of(r), us, ""])
        out.append(seq)
    return out


def main():
    nsteps = int(sys.argv[3]) if len(sys.argv) > 3 and sys.argv[3].isdigit() else 8
    old, new = steps_of(sys.argv[1], nsteps), steps_of(sys.argv[2], nsteps)
    agg = collections.defaultdict(lambda: [0, 0.0, 0.0])
    for so, sn in zip(old, new):
        if len(so) != len(sn):
            sys.exit(f"the steps differ in length after folding the reductions: {len(so)} vs {len(sn)}")
        for o, n in zip(so, sn):
            if o[0] != n[0] or o[1] != n[1] or "--all" in sys.argv:
                k = (o[0] + o[3], o[1], n[0] + n[3], n[1])
                agg[k][0] += 1
                agg[k][1] += o[2]
                agg[k][2] += n[2]
    print(f"{'launches/step':>13} {'old us':>8} {'new us':>8}  old kernel [blocks] -> new kernel [blocks]")
    to = tn = 0.0
    for k, v in sorted(agg.items(), key=lambda x: -x[1][1]):
        print(f"{v[0] / nsteps:13.1f} {v[1] / v[0]:8.2f} {v[2] / v[0]:8.2f}  {k[0]} [{k[1]}] -> {k[2]} [{k[3]}]")
        to += v[1] / nsteps
        tn += v[2] / nsteps
    print(f"sum over the listed launches: {to:.1f} -> {tn:.1f} us/step")


if __name__ == "__main__":
    main()
