"""Host test of the weight-gradient planner (include/dmc.h dmc_conv2d_wgrad_plan): a table of named descriptors, each
the smallest that still selects its form, and the plan each must get -- kind, grid, block, split count, slab layout --
plus, per case, that the workspace and the group queries report the same plan, and three grouped calls through
dmc_conv2d_wgrad_group_workspace's bytes[]. No GPU: the planner touches no device.

The expected columns were recorded from the commit BEFORE the planner existed (the dispatch inside wgrad_partial):
kernel, grid and block from a kernel trace of scripts/wgrad_plan_sweep.py over this table on the MI355X, splits and
layout from the dmc_wgrad_job its dmc_conv2d_wgrad_partial returned, the workspace bytes, the group kind and the
grouped bytes[] from its three host queries. They are not the planner's own output. `kernel` is the partial-sum
launch's name in that trace; the kind is read off its name (KIND_OF).

The issue that asked for this table expected `img4_off` (the whole-image case with DMC_WG_IMG4=0) to run the pipelined
kernel at width 4; at 16 channels the sources are not 64-aligned and the recorded dispatch is the generic kernel.
`img4_off_64` is the 64-channel descriptor that does fall to the pipelined kernel."""
import ctypes

import pytest
import torch

from conftest import ROOT

BF, F32 = torch.bfloat16, torch.float32

KIND_OF = {"wgrad3x3_img4_kernel": "img4", "wgrad3x3_pipe_kernel": "pipe", "wgrad3x3_halo2_kernel": "halo",
           "wgrad1x1_glds_kernel": "gemm1x1", "conv_wgrad_kernel": "generic"}
GENERIC_BF, GEMM1X1 = "conv_wgrad_kernel<unsigned short>", "wgrad1x1_glds_kernel<64, 2>"


def case(name, dt, N, S, C1, C2, Cout, taps, expect, ld_dy=None, stride=1, pro=None, opts=None):
    kernel, grid, block, splits, layout, ws, group = expect
    return dict(name=name, dt=dt, N=N, S=S, C1=C1, C2=C2, Cout=Cout, taps=taps, ld_dy=ld_dy, stride=stride, pro=pro,
                opts=opts or {}, kernel=kernel, grid=grid, block=block, splits=splits, layout=layout, ws=ws,
                group=group)


# name, dtype, N, square source map, C1, C2, Cout, taps ("3" forward 3x3, "d" flipped 3x3, "1" 1x1),
# (kernel, grid in blocks, block, splits, layout, dmc_conv2d_wgrad_workspace bytes, dmc_conv2d_wgrad_group_ok).
# Every case asks for the bias gradient. The dy pitch is Cout rounded up to a chunk unless given.
CASES = [
    # whole-image 4x4: one 512-pixel chunk; switched off; M not a whole chunk
    case("img4", BF, 32, 4, 16, 0, 16, "3", ("wgrad3x3_img4_kernel<true>", (1, 1, 1), 256, 0, 0, 1181696, 0)),
    case("img4_off", BF, 32, 4, 16, 0, 16, "3", (GENERIC_BF, (5, 1, 4), 256, 4, 0, 1181696, 0),
         opts={"DMC_WG_IMG4": 0}),
    case("img4_off_64", BF, 32, 4, 64, 0, 64, "3", ("wgrad3x3_pipe_kernel<4>", (8, 1, 1), 512, 8, 1, 2363392, 0),
         opts={"DMC_WG_IMG4": 0}),
    case("img4_part_chunk", BF, 4, 4, 64, 0, 64, "3", ("wgrad3x3_pipe_kernel<4>", (1, 1, 1), 512, 1, 1, 295424, 0)),
    # pipelined 3x3: widths 32 / 16 / 8, two sources, a narrow output in a pitch of 8, more than one tile per split
    case("pipe32", BF, 1, 32, 64, 0, 64, "3", ("wgrad3x3_pipe_kernel<32>", (8, 1, 1), 512, 8, 1, 2363392, 32)),
    case("pipe16", BF, 1, 16, 64, 0, 64, "3", ("wgrad3x3_pipe_kernel<16>", (2, 1, 1), 512, 2, 1, 590848, 16)),
    case("pipe8", BF, 2, 8, 64, 0, 64, "3", ("wgrad3x3_pipe_kernel<8>", (1, 1, 1), 512, 1, 1, 295424, 8)),
    case("pipe16_concat", BF, 1, 16, 64, 64, 64, "3", ("wgrad3x3_pipe_kernel<16>", (4, 1, 1), 512, 2, 1, 1180672, 16)),
    case("pipe16_narrow_out", BF, 1, 16, 64, 0, 3, "3", ("wgrad3x3_pipe_kernel<16>", (2, 1, 1), 512, 2, 1, 590848, 16)),
    case("pipe16_tps2", BF, 2, 16, 64, 0, 64, "3", ("wgrad3x3_pipe_kernel<16>", (2, 1, 1), 512, 2, 1, 1181696, 16),
         opts={"DMC_WG_HALO_TARGET": 2}),
    # round-4 halo: 64x64 at 7 pieces, 16x16 at 6 when the pipelined kind is off; flipped taps and a prologue pass
    case("halo64", BF, 1, 64, 64, 0, 64, "3", ("wgrad3x3_halo2_kernel<7>", (1, 1, 16), 256, 16, 0, 9453568, 0)),
    case("halo16_nopipe", BF, 1, 16, 64, 0, 64, "3", ("wgrad3x3_halo2_kernel<6>", (1, 1, 1), 256, 1, 0, 590848, 0),
         opts={"DMC_WG_PIPE": 0}),
    case("halo64_flipped", BF, 1, 64, 64, 0, 64, "d", ("wgrad3x3_halo2_kernel<7>", (1, 1, 16), 256, 16, 0, 9453568, 0)),
    case("halo16_silu", BF, 1, 16, 64, 0, 64, "3", ("wgrad3x3_halo2_kernel<6>", (1, 1, 1), 256, 1, 0, 590848, 0),
         pro="silu"),
    # 1x1 LDS-DMA: one stage, two sources, Linear shapes where the >= 256-pixel rule and the generic kernel's clamp bind
    case("g1x1_m64", BF, 1, 8, 8, 0, 8, "1", (GEMM1X1, (1, 1, 1), 256, 1, 1, 33280, 1)),
    case("g1x1_concat", BF, 1, 8, 128, 8, 64, "1", (GEMM1X1, (2, 1, 1), 256, 1, 1, 98816, 1)),
    case("linear256", BF, 256, 1, 64, 0, 64, "1", (GEMM1X1, (1, 1, 1), 256, 1, 1, 66560, 1)),
    case("linear1024_clamp", BF, 1024, 1, 64, 0, 64, "1", (GEMM1X1, (2, 1, 1), 256, 2, 1, 66560, 1),
         opts={"DMC_WG_MINPIX": 512}),
    # generic: fp32 on a 1x1 map, stride 2, a ragged first source, a 1x1 that is not a whole stage, DMC_NO_HALO
    case("generic_f32_1x1", F32, 1, 1, 32, 0, 32, "1", ("conv_wgrad_kernel<float>", (1, 1, 1), 256, 1, 0, 16896, 0)),
    case("generic_stride2", BF, 1, 16, 64, 0, 64, "3", (GENERIC_BF, (5, 1, 1), 256, 1, 0, 295424, 0),
         stride=2),
    case("generic_ragged_c1", BF, 1, 16, 3, 0, 64, "3", (GENERIC_BF, (5, 1, 2), 256, 2, 0, 590848, 0)),
    case("generic_1x1_m32", BF, 2, 4, 64, 0, 64, "1", (GENERIC_BF, (1, 1, 1), 256, 1, 0, 33280, 0)),
    case("generic_no_halo", BF, 1, 16, 64, 0, 64, "3", (GENERIC_BF, (5, 1, 2), 256, 2, 0, 590848, 0),
         opts={"DMC_NO_HALO": 1}),
]

# Grouped calls: name -> (options, jobs (N, square map, C1, C2, Cout, taps), bytes[] of
# dmc_conv2d_wgrad_group_workspace recorded from the parent commit)
GROUPS = {
    # two 3x3 jobs of one width in one launch
    "shared_launch": ({}, [(2, 16, 64, 0, 64, "3")] * 2, [591872, 591872]),
    # 16 + 32 + 16 output tiles fill the target / 4 = 64 cut: the fourth job runs alone, on its own plan (8 splits)
    "cut": ({}, [(4, 16, 256, 0, 256, "3"), (4, 16, 256, 0, 512, "3")] * 2, [9441280, 18882560, 9441280, 37765120]),
    # a 1x1 group of one: the single-layer split (4 x 256 pixels), also where the generic clamp binds (2, not 4)
    "one_1x1": ({}, [(4, 16, 64, 0, 192, "1")], [200704]),
    "one_1x1_clamp": ({"DMC_WG_MINPIX": 512}, [(1024, 1, 64, 0, 64, "1")], [33792]),
}


class HostOperand:
    """Stands in for a device tensor where only its address is taken (the planner never reads through it)."""

    def data_ptr(self):
        return 0x10000


def host_alloc(name, shape, dtype):
    return HostOperand()


def case_desc(c, alloc=host_alloc):
    """(descriptor, dy pitch, operands) of a table case. alloc(name, shape, dtype) provides each operand: HostOperand
    here, seeded device tensors in scripts/wgrad_plan_sweep.py."""
    from diffusion_models_collection_amd import _lib as L, kernels as K
    dt, N, S, C1, C2, Cout = c["dt"], c["N"], c["S"], c["C1"], c["C2"], c["Cout"]
    epc = L.chunk_for(dt)
    ld1 = (C1 + epc - 1) // epc * epc
    ld_dy = c.get("ld_dy") or (Cout + epc - 1) // epc * epc
    taps = {"3": K.TAPS3, "d": K.TAPS3_DGRAD, "1": K.TAPS1}[c["taps"]]
    OS = S // c.get("stride", 1)
    d = K.make_desc(dt, N, S, S, C1, C2, ld1, C2, L.kc_for(C1 + C2, dt), OS, OS, Cout, taps, stride=c.get("stride", 1))
    if c.get("pro") == "silu":
        K.set_prologue(d, L.PRO_SILU)
    ops = {"x1": alloc("x1", (N, S, S, ld1), dt), "x2": alloc("x2", (N, S, S, C2), dt) if C2 else None,
           "dy": alloc("dy", (N, OS, OS, ld_dy), dt), "dw": alloc("dw", (Cout, C1 + C2, len(taps)), F32),
           "dbias": alloc("dbias", (Cout,), F32)}
    d.wg_bias = ops["dbias"].data_ptr()
    return d, ld_dy, ops


def group_items(jobs, alloc=host_alloc):
    """(WgradGroupItem array without workspaces, descriptors, operands per job) of a GROUPS entry."""
    from diffusion_models_collection_amd import _lib as L
    arr, descs, opss = (L.WgradGroupItem * len(jobs))(), [], []
    for i, (N, S, C1, C2, Cout, taps) in enumerate(jobs):
        d, ld_dy, ops = case_desc(dict(dt=BF, N=N, S=S, C1=C1, C2=C2, Cout=Cout, taps=taps), alloc)
        arr[i].d = ctypes.pointer(d)
        arr[i].dy, arr[i].ld_dy = ops["dy"].data_ptr(), ld_dy
        arr[i].x1, arr[i].x2 = ops["x1"].data_ptr(), L.ptr(ops["x2"])
        arr[i].dw, arr[i].scale = ops["dw"].data_ptr(), 1.0
        descs.append(d)
        opss.append(ops)
    return arr, descs, opss


def per_split_bytes(d, layout):
    """Bytes one split's weight partials take in the slab of a dmc_wgrad_job of that layout."""
    cpad = (d.Cout + 127) // 128 * 128
    return 4 * (d.Cout * (d.C1 + d.C2) * d.ntaps if layout else d.ntaps * d.Kc * cpad)


def _lib():
    if not (ROOT / "diffusion_models_collection_amd" / "libdmc.so").exists():
        from diffusion_models_collection_amd.build import build
        build()
    from diffusion_models_collection_amd import _lib as L, kernels as K
    return L, K


def test_table_covers_every_kind():
    L, _ = _lib()
    assert {KIND_OF[c["kernel"].split("<")[0]] for c in CASES} == set(L.WGRAD_KINDS) - {""}
    assert len({c["name"] for c in CASES}) == len(CASES)
    assert len({c["kernel"] for c in CASES}) >= 10   # the sub-forms: distinct kernel instantiations in the table


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_plan_matches_recorded_dispatch(c, dmc_opt):
    L, K = _lib()
    for name, v in c["opts"].items():
        dmc_opt(name, v)
    d, ld_dy, _ = case_desc(c)
    p = K.wgrad_plan(d, ld_dy)
    got = (L.WGRAD_KINDS[p.kind], tuple(p.grid), p.block, p.splits, p.layout, p.ws_bytes, p.group_kind)
    assert got == (KIND_OF[c["kernel"].split("<")[0]], c["grid"], c["block"], c["splits"], c["layout"], c["ws"],
                   c["group"])
    # the queries are reads of the same plan, and the plan's slab fits the workspace the caller was told to bring
    assert p.ws_bytes == L.LIB.dmc_conv2d_wgrad_workspace(ctypes.byref(d))
    assert p.group_kind == L.LIB.dmc_conv2d_wgrad_group_ok(ctypes.byref(d), ld_dy)
    assert p.splits * (per_split_bytes(d, p.layout) + 4 * ((d.Cout + 127) // 128 * 128)) <= p.ws_bytes


@pytest.mark.parametrize("g", GROUPS, ids=list(GROUPS))
def test_group_bytes_match_recorded_plan(g, dmc_opt):
    L, K = _lib()
    opts, jobs, want = GROUPS[g]
    for name, v in opts.items():
        dmc_opt(name, v)
    arr, descs, _ = group_items(jobs)
    got = (ctypes.c_size_t * len(jobs))()
    total = L.LIB.dmc_conv2d_wgrad_group_workspace(arr, len(jobs), got)
    assert list(got) == want and total == sum(want)
    if len(jobs) == 1:   # a group of one is the single-layer plan: its split count, behind the grouped layout
        p = K.wgrad_plan(descs[0], arr[0].ld_dy)
        assert got[0] == p.splits * (per_split_bytes(descs[0], 1) + 4 * ((descs[0].Cout + 127) // 128 * 128))


def test_quirks_a_descriptor_can_show(dmc_opt):
    """DESIGN.md "Weight-gradient dispatch", quirks 1-5, each on the table's descriptor that shows it."""
    L, K = _lib()
    by = {c["name"]: c for c in CASES}

    def plan(name, **opts):
        for k, v in opts.items():
            dmc_opt(k, v)
        d, ld_dy, _ = case_desc(by[name])
        p = K.wgrad_plan(d, ld_dy)
        L.reset_options(False)
        return L.WGRAD_KINDS[p.kind], p, d

    # 1. the workspace query reports a slab for the whole-image kind, which uses none, and sizes a layout-1 plan's as
    #    layout 0
    kind, p, d = plan("img4")
    assert kind == "img4" and p.splits == 0 and p.ws_bytes > 0
    kind, p, d = plan("pipe16_narrow_out")
    assert p.layout == 1 and p.ws_bytes == p.splits * (per_split_bytes(d, 0) + 4 * 128)
    assert p.ws_bytes > p.splits * (per_split_bytes(d, 1) + 4 * 128)
    # 2. the halo kind takes flipped taps and a prologue; the pipelined kind refuses both
    assert plan("halo64_flipped")[0] == "halo" and plan("halo16_silu")[0] == "halo"
    d, ld_dy, _ = case_desc(dict(by["pipe16"], taps="d"))
    assert L.WGRAD_KINDS[K.wgrad_plan(d, ld_dy).kind] == "halo"
    # 3. DMC_NO_HALO turns off the halo and the pipelined kinds, DMC_WG_PIPE=0 the pipelined kind only
    assert plan("pipe16")[0] == "pipe"
    assert plan("pipe16", DMC_NO_HALO=1)[0] == "generic" and plan("pipe16", DMC_WG_PIPE=0)[0] == "halo"
    assert plan("halo64", DMC_NO_HALO=1)[0] == "generic"
    # 4. width 4 is a pipelined width for a single call and refused by the grouped entry
    kind, p, _ = plan("img4_part_chunk")
    assert kind == "pipe" and p.group_kind == 0
    # 5. the 1x1 kind's split count is clamped by the generic kernel's knobs
    assert plan("linear1024_clamp")[1].splits == 4
    assert plan("linear1024_clamp", DMC_WG_MINPIX=512)[1].splits == 2
    assert plan("linear1024_clamp", DMC_WG_BLOCKS=1)[1].splits == 1


def test_rejected_descriptor_and_pitch():
    L, K = _lib()
    d, ld_dy, _ = case_desc(CASES[0])
    with pytest.raises(L.DMCError, match="ld_dy"):
        K.wgrad_plan(d, ld_dy + 4)
    assert L.LIB.dmc_conv2d_wgrad_group_ok(ctypes.byref(d), ld_dy + 4) == 0
    d.ntaps = 0
    with pytest.raises(L.DMCError, match="ntaps"):
        K.wgrad_plan(d, ld_dy)
