"""Host test of the forward-conv planner (include/dmc.h dmc_conv2d_plan): a table of named descriptors, one per
kernel family and sub-form, and the plan each must get -- family, grid, block, split-K factor, who writes the
GroupNorm partials -- plus, per case, that the three legacy queries report the same plan. No GPU: the planner
touches no device.

The expected columns were recorded from a kernel trace of the commit BEFORE the planner existed (the five-place
dispatch), run over this table by scripts/conv_plan_sweep.py; they are not the planner's own output. `kernel` is
the main launch's name in that trace; the family is read off its name (FAMILY_OF)."""
import ctypes

import pytest
import torch

from conftest import ROOT

BF, F32 = torch.bfloat16, torch.float32
NONE, KERNEL, SPLITK, PASS = 0, 1, 2, 3   # include/dmc.h DMC_GN_PART_*

FAMILY_OF = {"conv3x3_nin_kernel": "nin_halo", "conv3x3_nout_kernel": "nout_halo", "conv_narrow_in_kernel": "narrow_in",
             "conv_narrow_out_kernel": "narrow_out", "conv3x3_img_kernel": "img", "gemm1x1_persist_kernel": "gemm1x1",
             "conv3x3_halo2_kernel": "halo", "conv_fwd_glds_kernel": "glds", "conv_fwd_kernel": "reg"}


def case(name, dt, N, S, C1, C2, Cout, taps, expect, pro=None, gn=False, addvec=False, resid=False, nchw=False,
         csplit=None, gelu=False, opts=None):
    kernel, grid, block, splits, gn_mode = expect
    return dict(name=name, dt=dt, N=N, S=S, C1=C1, C2=C2, Cout=Cout, taps=taps, pro=pro, gn=gn, addvec=addvec,
                resid=resid, nchw=nchw, csplit=csplit, gelu=gelu, opts=opts or {}, kernel=kernel, grid=grid, block=block,
                splits=splits, gn_mode=gn_mode)


# name, dtype, N, square map, C1, C2, Cout, taps ("3" forward 3x3, "d" its input gradient, "1" 1x1),
# (kernel, grid in blocks, block, splits, partials mode). Each is the smallest descriptor that still selects its form.
NOSK = {"DMC_NO_SPLITK": 1}
CASES = [
    # halo'd narrow-in (3 -> 128 at 16x16): epilogue from the accumulators, and the LDS-staged one
    case("nin_halo_reg", BF, 1, 16, 3, 0, 128, "3", ("conv3x3_nin_kernel<true>", (2, 1, 1), 256, 1, KERNEL), gn=True),
    case("nin_halo_lds", BF, 1, 16, 3, 0, 128, "d", ("conv3x3_nin_kernel<false>", (2, 1, 1), 256, 1, KERNEL), gn=True,
         opts={"DMC_REG_EPI": 0}),
    # halo'd narrow-out: 6 / 7 / 9 halo pieces per wave, one and two 64-channel planes
    case("nout_halo6_1", BF, 1, 16, 64, 0, 3, "3", ("conv3x3_nout_kernel<6, 1>", (2, 1, 1), 256, 1, NONE)),
    case("nout_halo6_2", BF, 1, 16, 64, 64, 3, "3", ("conv3x3_nout_kernel<6, 2>", (2, 1, 1), 256, 1, NONE), nchw=True),
    case("nout_halo7_2", BF, 1, 32, 128, 0, 3, "3", ("conv3x3_nout_kernel<7, 2>", (8, 1, 1), 256, 1, NONE), nchw=True),
    case("nout_halo7_1", BF, 2, 8, 64, 0, 3, "3", ("conv3x3_nout_kernel<7, 1>", (1, 1, 1), 256, 1, NONE)),
    case("nout_halo9_1", BF, 1, 64, 64, 0, 3, "3", ("conv3x3_nout_kernel<9, 1>", (32, 1, 1), 256, 1, NONE)),
    # generic narrow kernels (no halo geometry / too many channels), both dtypes
    case("narrow_in_bf16", BF, 1, 8, 3, 0, 32, "3", ("conv_narrow_in_kernel<unsigned short>", (1, 1, 1), 256, 1, NONE)),
    case("narrow_in_f32", F32, 5, 8, 3, 0, 48, "3", ("conv_narrow_in_kernel<float>", (2, 2, 1), 256, 1, NONE)),
    case("narrow_out_bf16", BF, 1, 8, 192, 0, 3, "3", ("conv_narrow_out_kernel<unsigned short>", (1, 1, 1), 256, 1, NONE)),
    case("narrow_out_f32", F32, 5, 8, 32, 0, 3, "3", ("conv_narrow_out_kernel<float>", (2, 1, 1), 256, 1, NONE)),
    # whole-image small-map kernel: 4x4 / 8x8, 16- / 32-channel tiles, forward / input gradient, GroupNorm prologue
    case("img4_bn16_fwd", BF, 8, 4, 64, 0, 64, "3", ("conv3x3_img_kernel<16, 32, 4, false>", (4, 1, 1), 256, 1, NONE)),
    case("img4_bn32_dgrad", BF, 128, 4, 64, 0, 512, "d", ("conv3x3_img_kernel<32, 32, 3, false>", (256, 1, 1), 256, 1, NONE)),
    case("img8_bn16_dgrad", BF, 4, 8, 64, 0, 64, "d", ("conv3x3_img_kernel<16, 64, 3, false>", (4, 1, 1), 256, 1, PASS),
         gn=True),
    case("img8_bn32_fwd", BF, 64, 8, 64, 0, 512, "3", ("conv3x3_img_kernel<32, 64, 2, false>", (256, 1, 1), 256, 1, KERNEL),
         gn=True, addvec=True, resid=True),
    case("img4_gn_silu", BF, 8, 4, 256, 0, 64, "3", ("conv3x3_img_kernel<16, 32, 4, true>", (4, 1, 1), 256, 1, NONE),
         pro="gn"),
    case("img8_gn_silu", BF, 64, 8, 256, 0, 512, "3", ("conv3x3_img_kernel<32, 64, 2, true>", (256, 1, 1), 256, 1, KERNEL),
         pro="gn", gn=True),
    # persistent 1x1 GEMM: one output and a split one
    case("gemm1x1", BF, 8, 16, 64, 0, 1024, "1", ("gemm1x1_persist_kernel<2>", (128, 1, 1), 256, 1, NONE)),
    case("gemm1x1_split", BF, 8, 16, 64, 0, 1024, "1", ("gemm1x1_persist_kernel<2>", (128, 1, 1), 256, 1, NONE), csplit=512),
    # a request for partials keeps a conv off the persistent GEMM ... unless both epilogue forms are switched off
    case("gemm1x1_gn_request", BF, 8, 16, 64, 0, 1024, "1", ("conv_fwd_glds_kernel<2, 2, true, 3>", (128, 1, 1), 256, 1, KERNEL),
         gn=True),
    case("gemm1x1_gn_quirk", BF, 8, 16, 64, 0, 1024, "1", ("gemm1x1_persist_kernel<2>", (128, 1, 1), 256, 1, PASS),
         gn=True, opts={"DMC_NO_EPI_STATS": 1, "DMC_NO_SKGN": 1}),
    # 128-pixel halo kernel at 6 / 7 / 9 pieces, without and with the GN-affine+SiLU prologue on the halo
    case("halo6", BF, 1, 16, 64, 0, 128, "3", ("conv3x3_halo2_kernel<6, 3, false>", (2, 1, 1), 256, 1, KERNEL), gn=True,
         opts=NOSK),
    case("halo7", BF, 1, 32, 64, 64, 128, "d", ("conv3x3_halo2_kernel<7, 3, false>", (8, 1, 1), 256, 1, NONE), opts=NOSK),
    case("halo9", BF, 1, 64, 64, 0, 256, "3", ("conv3x3_halo2_kernel<9, 2, false>", (64, 1, 1), 256, 1, NONE), resid=True,
         opts=NOSK),
    case("halo6_pro", BF, 1, 16, 64, 0, 128, "3", ("conv3x3_halo2_kernel<6, 3, true>", (2, 1, 1), 256, 1, KERNEL), pro="affine",
         gn=True, opts=NOSK),
    case("halo7_pro", BF, 1, 32, 64, 0, 128, "3", ("conv3x3_halo2_kernel<7, 3, true>", (8, 1, 1), 256, 1, NONE), pro="affine",
         opts=NOSK),
    case("halo9_pro", BF, 1, 64, 64, 0, 128, "3", ("conv3x3_halo2_kernel<9, 2, true>", (32, 1, 1), 256, 1, NONE), pro="affine",
         opts=NOSK),
    case("halo_no_xcd", BF, 1, 16, 64, 0, 256, "3", ("conv3x3_halo2_kernel<6, 3, false>", (2, 2, 1), 256, 1, NONE),
         opts={"DMC_NO_SPLITK": 1, "DMC_NO_XCD": 1}),
    # LDS-DMA implicit GEMM: split-K (plain and GroupNorm epilogue), 64-row tiles, 128-row tiles on the 3-stage and
    # on the 2-stage ring (more tiles than CUs; the 256x128-class plan), buffer (C1 = 64) and plain (C1 = 32) addressing
    case("glds_split_buf", BF, 1, 16, 64, 0, 128, "3", ("conv_fwd_glds_kernel<2, 2, true, 3>", (2, 1, 2), 256, 2, NONE)),
    case("glds_split_gn", BF, 1, 16, 64, 0, 128, "3", ("conv_fwd_glds_kernel<2, 2, true, 3>", (2, 1, 2), 256, 2, SPLITK),
         gn=True),
    case("glds_split_gn_pass", BF, 1, 16, 64, 0, 128, "3", ("conv_fwd_glds_kernel<2, 2, true, 3>", (2, 1, 2), 256, 2, PASS),
         gn=True, opts={"DMC_NO_SKGN": 1}),
    case("glds_split_plain", BF, 1, 16, 32, 0, 128, "3", ("conv_fwd_glds_kernel<2, 2, false, 3>", (2, 1, 2), 256, 2, NONE)),
    case("glds_64row_buf", BF, 1, 8, 64, 0, 128, "1", ("conv_fwd_glds_kernel<1, 2, true, 3>", (1, 1, 1), 128, 1, NONE)),
    case("glds_64row_plain", BF, 1, 8, 32, 0, 128, "1", ("conv_fwd_glds_kernel<1, 2, false, 3>", (1, 1, 1), 128, 1, NONE)),
    case("glds_nosplit_64row", BF, 1, 16, 32, 0, 128, "3", ("conv_fwd_glds_kernel<1, 2, false, 3>", (4, 1, 1), 128, 1, NONE),
         opts=NOSK),
    case("glds_3stage_buf", BF, 8, 16, 64, 0, 1024, "1", ("conv_fwd_glds_kernel<2, 2, true, 3>", (128, 1, 1), 256, 1, NONE),
         addvec=True),
    case("glds_3stage_gelu", BF, 8, 16, 64, 0, 1024, "1", ("conv_fwd_glds_kernel<2, 2, true, 3>", (128, 1, 1), 256, 1, NONE),
         gelu=True),
    case("glds_3stage_plain", BF, 8, 16, 32, 0, 1024, "1", ("conv_fwd_glds_kernel<2, 2, false, 3>", (128, 1, 1), 256, 1, NONE)),
    case("glds_2stage_buf", BF, 66, 8, 64, 0, 1024, "1", ("conv_fwd_glds_kernel<2, 2, true, 2>", (264, 1, 1), 256, 1, NONE),
         addvec=True),
    case("glds_2stage_plain", BF, 66, 8, 32, 0, 1024, "1", ("conv_fwd_glds_kernel<2, 2, false, 2>", (264, 1, 1), 256, 1, NONE)),
    case("glds_big", BF, 30, 16, 64, 0, 1024, "1", ("conv_fwd_glds_kernel<2, 2, true, 2>", (480, 1, 1), 256, 1, KERNEL),
         addvec=True, gn=True),
    # register-staged: 128x128 tiles, split-K, 64x64 tiles (fp32; bf16 with a prologue the halo kernel does not take)
    case("reg_big_f32", F32, 24, 16, 32, 0, 1024, "1", ("conv_fwd_kernel<float, 128, 128>", (48, 8, 1), 256, 1, NONE)),
    case("reg_splitk_f32", F32, 2, 1, 512, 0, 64, "1", ("conv_fwd_kernel<float, 64, 64>", (1, 1, 4), 256, 4, NONE)),
    case("reg_64_f32", F32, 1, 8, 32, 0, 64, "3", ("conv_fwd_kernel<float, 64, 64>", (1, 1, 1), 256, 1, PASS), gn=True),
    case("reg_64_bf16_silu", BF, 1, 8, 64, 0, 64, "3", ("conv_fwd_kernel<unsigned short, 64, 64>", (1, 1, 1), 256, 1, PASS),
         pro="silu", gn=True),
    case("reg_pro_small", BF, 1, 16, 64, 0, 128, "3", ("conv_fwd_kernel<unsigned short, 64, 64>", (4, 2, 1), 256, 1, NONE),
         pro="affine"),
]


class HostOperand:
    """Stands in for a device tensor where only its address is taken (the planner never reads through it)."""

    def data_ptr(self):
        return 0x10000


def host_alloc(name, shape, dtype):
    return HostOperand()


def case_desc(c, alloc=host_alloc):
    """(descriptor, operands) of a table case. alloc(name, shape, dtype) provides each operand: HostOperand here,
    seeded device tensors in scripts/conv_plan_sweep.py."""
    from diffusion_models_collection_amd import _lib as L, kernels as K
    dt, N, S, C1, C2, Cout = c["dt"], c["N"], c["S"], c["C1"], c["C2"], c["Cout"]
    epc = L.chunk_for(dt)
    ld1 = (C1 + epc - 1) // epc * epc
    taps = {"3": K.TAPS3, "d": K.TAPS3_DGRAD, "1": K.TAPS1}[c["taps"]]
    Kc, M, C = L.kc_for(C1 + C2, dt), N * S * S, C1 + C2
    d = K.make_desc(dt, N, S, S, C1, C2, ld1, C2, Kc, S, S, Cout, taps)
    ops = {"x1": alloc("x1", (N, S, S, ld1), dt), "x2": alloc("x2", (N, S, S, C2), dt) if C2 else None,
           "w": alloc("w", (Cout, len(taps), Kc), dt), "y2": None}
    if c["pro"] == "affine":
        K.set_prologue(d, L.PRO_AFFINE_SILU, alloc("scale", (N, C), F32), alloc("shift", (N, C), F32), C)
    elif c["pro"] == "gn":
        K.set_prologue(d, L.PRO_GN_SILU, alloc("scale", (C,), F32), alloc("shift", (C,), F32), C)
        d.pro_groups, d.pro_eps = 32, 1e-5
    elif c["pro"] == "silu":
        K.set_prologue(d, L.PRO_SILU)
    ops["part"] = alloc("part", (M // 64 * (Cout // 8) * 2,), F32) if c["gn"] else None
    epi = dict(bias=alloc("bias", (Cout,), F32), gn_part=ops["part"])
    if c["addvec"]:
        epi.update(addvec=alloc("addvec", (N, Cout), F32), ld_add=Cout)
    if c["resid"]:
        epi.update(resid=alloc("resid", (M, Cout), dt), ld_res=Cout)
    ops["y_pre"] = alloc("y_pre", (M, Cout), dt) if c["gelu"] else None
    if c["gelu"]:   # exact GELU last, the pre-activation stored too (the DiT MLP's fc1)
        epi.update(act=L.ACT_GELU, y_pre=ops["y_pre"], ld_pre=Cout)
    if c["nchw"]:
        ops["y1"] = alloc("y1", (N, Cout, S, S), F32)
        K.set_epilogue(d, out_f32=True, out_nchw=True, **epi)
    elif c["csplit"]:
        ops["y1"], ops["y2"] = alloc("y1", (M, c["csplit"]), dt), alloc("y2", (M, Cout - c["csplit"]), dt)
        K.set_epilogue(d, ldy1=c["csplit"], ldy2=Cout - c["csplit"], Csplit=c["csplit"], **epi)
    else:
        ops["y1"] = alloc("y1", (M, Cout), dt)
        K.set_epilogue(d, ldy1=Cout, **epi)
    return d, ops


def _lib():
    if not (ROOT / "diffusion_models_collection_amd" / "libdmc.so").exists():
        from diffusion_models_collection_amd.build import build
        build()
    from diffusion_models_collection_amd import _lib as L, kernels as K
    return L, K


def test_table_covers_every_family():
    L, _ = _lib()
    fams = {FAMILY_OF[c["kernel"].split("<")[0]] for c in CASES}
    assert fams == set(L.CONV_FAMILIES) - {"none"}
    assert len({c["name"] for c in CASES}) == len(CASES)
    assert len({c["kernel"] for c in CASES}) >= 30   # the sub-forms: distinct kernel instantiations in the table


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_plan_matches_recorded_dispatch(c, dmc_opt):
    L, K = _lib()
    for name, v in c["opts"].items():
        dmc_opt(name, v)
    d, _ = case_desc(c)
    p = K.conv_plan(d)
    got = (L.CONV_FAMILIES[p.family], tuple(p.grid), p.block, p.splits, p.gn_part)
    assert got == (FAMILY_OF[c["kernel"].split("<")[0]], c["grid"], c["block"], c["splits"], c["gn_mode"])
    # the legacy queries are reads of the same plan
    ws = L.LIB.dmc_conv2d_workspace(ctypes.byref(d))
    assert ws == p.ws_bytes and (p.splits > 1) <= (ws > 0)
    assert K.conv_halo_prologue(d) == bool(p.fused_prologue)
    # dmc_conv2d_fused_epilogue answers for the descriptor WITH the partials requested
    if not c["gn"] and c["S"] * c["S"] % 64 == 0 and c["Cout"] % 8 == 0 and not c["csplit"] and not c["nchw"]:
        d.gn_part = 0x10000
    if d.gn_part:
        assert K.conv_fused(d) == (L.FUSED_GN_STATS if K.conv_plan(d).gn_part == KERNEL else 0)
    # without a workspace nothing splits
    assert K.conv_plan(d, 0).splits == 1


def test_empty_problem_and_rejected_descriptor():
    L, K = _lib()
    d, _ = case_desc(dict(CASES[0], N=0))
    p = K.conv_plan(d)
    assert (L.CONV_FAMILIES[p.family], tuple(p.grid), p.ws_bytes) == ("none", (0, 0, 0), 0)
    # DMC_PRO_GN_SILU on a map the small-map kernel does not take: refused, as dmc_conv2d refuses it
    c = next(c for c in CASES if c["name"] == "img4_gn_silu")
    d, _ = case_desc(dict(c, S=16))
    assert not K.conv_halo_prologue(d)
    with pytest.raises(L.DMCError, match="DMC_PRO_GN_SILU"):
        K.conv_plan(d)
