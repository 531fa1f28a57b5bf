"""The whole-K form of the 1x1 GEMM (gemm1x1_wholek_kernel, DMC_GEMM1X1_WK) against the plans it replaces.

Per case the conv runs through K.conv with DMC_GEMM1X1_WK = 1 and = 0. The outputs -- and the GroupNorm partials
where requested -- must be BITWISE equal: every output element is accumulated k ascending through the same MFMA
steps (a split-K plan's runs summed in its order) and finished as (acc + bias) + residual, whichever kernel runs.
The plan with 1 must be the whole-K form at the tile the planner rule gives (a fallback would make the comparison
vacuous), the plan with 0 must not be. Both match an fp32 torch GEMM of the bf16 operands at the bf16 tolerance of
test_gpu_kernels.py::test_gemm1x1_persistent_bitwise.

The shapes are the smallest that reach each edge of the kernel and of the planner rule; every tile is reached."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
T64X128, T64 = 1, 2   # include/dmc.h DMC_WK_*


def case(name, N, S, C1, C2, Cout, tile, part=False, resid=None, csplit=None, runs=0):
    """runs: with the option at 0 the conv has a split-K plan of that many runs; the form then runs one wave per run"""
    return dict(name=name, N=N, S=S, C1=C1, C2=C2, Cout=Cout, tile=tile, part=part, resid=resid, csplit=csplit, runs=runs)


CASES = [
    case("two_stages_one_tile", 2, 8, 128, 0, 128, T64),
    case("k256", 2, 8, 256, 0, 256, T64),
    case("concat_k512_two_runs", 2, 8, 256, 256, 256, T64, runs=2),
    case("k768_slot_reuse_three_runs", 2, 8, 768, 0, 256, T64, runs=3),   # a run's 4 stages in its 3 slots
    case("k1024_four_runs", 2, 8, 1024, 0, 256, T64, runs=4),              # a run's 4 stages in its 2 slots
    case("k1536_six_runs_keep_splitk", 2, 8, 1536, 0, 256, 0),             # more runs than the form takes
    case("map4_wide_out", 8, 4, 256, 0, 768, T64),
    case("map4_one_block_per_cu", 128, 4, 256, 0, 256, T64),            # 128 blocks of 64 x 64
    case("attn_proj_partials_inplace", 128, 8, 256, 0, 256, T64X128, part=True, resid="inplace"),
    case("too_many_tiles", 128, 8, 256, 0, 768, 0),                     # 384 tiles: keeps the persistent GEMM
    case("resid_separate", 2, 8, 256, 0, 256, T64, resid="separate"),
    case("split_output", 2, 8, 256, 0, 512, T64, csplit=256),
    case("more_than_128_tiles", 128, 8, 256, 0, 512, 0),                # 256 tiles: keeps the persistent GEMM
    case("tile64x128_slot_reuse", 128, 8, 768, 0, 256, T64X128),        # 12 stages in 6 slots
    case("map4_k512_two_runs", 128, 4, 256, 256, 256, T64, runs=2),     # the up-path shortcut
]


def rel_err(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-12)).item()


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_wholek_bitwise_and_planned(c, dmc_opt):
    from diffusion_models_collection_amd import _lib as L, kernels as K
    N, S, C1, C2, Cout = c["N"], c["S"], c["C1"], c["C2"], c["Cout"]
    M, dt = N * S * S, torch.bfloat16
    gen = torch.Generator().manual_seed(N + S + C1 + C2 + Cout)
    x1 = torch.randn(N, S, S, C1, generator=gen).to(dt).to(DEV)
    x2 = torch.randn(N, S, S, C2, generator=gen).to(dt).to(DEV) if C2 else None
    w = (torch.randn(Cout, C1 + C2, 1, 1, generator=gen) * 0.05).to(DEV)
    b = torch.randn(Cout, generator=gen).to(DEV)
    r0 = torch.randn(N, S, S, Cout, generator=gen).to(dt).to(DEV) if c["resid"] else None
    Kc = L.kc_for(C1 + C2, dt)
    wp = K.pack_weight(L.PACK_FWD, dt, w, Kc)
    cs = c["csplit"] or Cout
    outs, plans = [], []
    for on in (1, 0):
        dmc_opt("DMC_GEMM1X1_WK", on)
        y1 = torch.full((N, S, S, cs), 7.0, device=DEV, dtype=dt)
        y2 = torch.full((N, S, S, Cout - cs), 7.0, device=DEV, dtype=dt) if c["csplit"] else None
        res = r0
        if c["resid"] == "inplace":
            y1 = r0.clone()
            res = y1
        part = torch.full((M // 64 * (Cout // 8) * 2,), -3.0, device=DEV) if c["part"] else None
        d = K.make_desc(dt, N, S, S, C1, C2, C1, C2, Kc, S, S, Cout, K.TAPS1)
        K.set_epilogue(d, bias=b, resid=res, ld_res=Cout if c["resid"] else 0, ldy1=cs, ldy2=Cout - cs, Csplit=cs,
                       gn_part=part)
        plans.append(K.conv_plan(d))
        K.conv(d, x1, x2, wp, y1, y2)
        outs.append((y1, y2, part))
    torch.cuda.synchronize()
    p1, p0 = plans
    assert p0.whole_k == 0
    assert p1.whole_k == c["tile"]
    if c["tile"]:
        bm, bn = {T64X128: (64, 128), T64: (64, 64)}[c["tile"]]
        assert (L.CONV_FAMILIES[p1.family], tuple(p1.grid), p1.block, p1.splits) == \
            ("gemm1x1", (M // bm * (Cout // bn), 1, 1), 64 * c["runs"] if c["runs"] else bm * bn // 64, 1)
        assert p1.gn_part == p0.gn_part
        assert p0.splits == max(1, c["runs"])
    assert torch.equal(outs[0][0], outs[1][0])
    if c["csplit"]:
        assert torch.equal(outs[0][1], outs[1][1])
    if c["part"]:
        assert p1.gn_part == L.GN_PART_KERNEL
        assert torch.equal(outs[0][2], outs[1][2]) and not (outs[0][2] == -3.0).any()
    xs = torch.cat([x1, x2], -1) if C2 else x1
    ref = xs.float().reshape(-1, C1 + C2) @ w.view(Cout, -1).to(dt).float().t() + b
    if c["resid"]:
        ref = ref + r0.float().reshape(-1, Cout)
    got = torch.cat([outs[0][0], outs[0][1]], -1) if c["csplit"] else outs[0][0]
    assert rel_err(got.float().reshape(-1, Cout), ref) < 1e-2


def test_every_tile_is_reached():
    assert {c["tile"] for c in CASES} == {0, T64X128, T64}
    assert {c["runs"] for c in CASES} == {0, 2, 3, 4}
