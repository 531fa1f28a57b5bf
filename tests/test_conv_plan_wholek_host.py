"""Host test of the planner rule of the whole-K 1x1 GEMM (DMC_GEMM1X1_WK; include/dmc.h dmc_conv_plan.whole_k).
No GPU: the planner touches no device.

With the option at 1 a descriptor the form takes is planned as family gemm1x1 with the tile, grid and block the
rule gives -- 64x64 where that needs at most 256 blocks, else 64x128 under the same bound; one wave per run of a
split-K plan -- with no split-K launch, and the GroupNorm partials written by whoever wrote them before. With the
option at 0 every descriptor gets the plan of the commit before the form existed: the `parent` columns were recorded from that commit's library over this
table, they are not this planner's output. Descriptors the form must refuse keep that plan under both settings."""
import pytest
import torch

from test_conv_plan_host import NONE, KERNEL, SPLITK, PASS, _lib, case, case_desc

BF = torch.bfloat16
T64X128, T64 = 1, 2   # include/dmc.h DMC_WK_*
TILE = {T64X128: (64, 128), T64: (64, 64)}
UNUSED = ("", (0, 0, 0), 0, 0, 0)


def row(name, N, S, C1, C2, Cout, tile, parent, **kw):
    return dict(case(name, BF, N, S, C1, C2, Cout, "1", UNUSED, **kw), tile=tile, parent=parent)


# name, N, map, C1, C2, Cout, tile with the option at 1 (0: refused), the parent commit's plan
# (family, grid, block, split-K factor, partials mode)
ROWS = [
    row("two_stages_one_tile", 2, 8, 128, 0, 128, T64, ("glds", (2, 1, 1), 128, 1, NONE)),
    row("k256", 2, 8, 256, 0, 256, T64, ("glds", (4, 1, 1), 128, 1, NONE)),
    row("concat_k512", 2, 8, 256, 256, 256, T64, ("glds", (1, 2, 2), 256, 2, NONE)),
    row("k768_slot_reuse", 2, 8, 768, 0, 256, T64, ("glds", (1, 2, 3), 256, 3, NONE)),
    row("map4_wide_out", 8, 4, 256, 0, 768, T64, ("glds", (12, 1, 1), 128, 1, NONE)),
    row("map4_one_block_per_cu", 128, 4, 256, 0, 256, T64, ("glds", (64, 1, 1), 128, 1, NONE)),
    row("attn_proj_partials", 128, 8, 256, 0, 256, T64X128, ("glds", (128, 1, 1), 256, 1, KERNEL), gn=True, resid=True),
    row("too_many_tiles", 128, 8, 256, 0, 768, 0, ("gemm1x1", (384, 1, 1), 256, 1, NONE)),
    row("resid_separate", 2, 8, 256, 0, 256, T64, ("glds", (4, 1, 1), 128, 1, NONE), resid=True),
    row("split_output", 2, 8, 256, 0, 512, T64, ("glds", (8, 1, 1), 128, 1, NONE), csplit=256),
    row("more_than_128_tiles", 128, 8, 256, 0, 512, 0, ("gemm1x1", (256, 1, 1), 256, 1, NONE)),
    row("k1024_four_runs", 2, 8, 1024, 0, 256, T64, ("glds", (1, 2, 4), 256, 4, NONE)),
    row("k1536_six_runs", 2, 8, 1536, 0, 256, 0, ("glds", (1, 2, 6), 256, 6, NONE)),
    row("tile64x128_slot_reuse", 128, 8, 768, 0, 256, T64X128, ("gemm1x1", (128, 1, 1), 256, 1, NONE)),
    row("map4_k512", 128, 4, 256, 256, 256, T64, ("glds", (16, 2, 2), 256, 2, NONE)),
    # partials the form cannot restate bit for bit keep their kernel: the 64-row tile's LDS-staged epilogue, the
    # split-K reduction's epilogue; a pass over the stored output follows either kernel
    row("partials_64row", 4, 8, 256, 0, 256, 0, ("glds", (8, 1, 1), 128, 1, KERNEL), gn=True),
    row("partials_splitk", 2, 8, 512, 0, 256, 0, ("glds", (1, 2, 2), 256, 2, SPLITK), gn=True),
    row("partials_pass", 2, 8, 256, 0, 256, T64, ("glds", (4, 1, 1), 128, 1, PASS), gn=True),
    # where the persistent GEMM applies the form takes the conv from K = 512 on
    row("persistent_k256", 128, 8, 256, 0, 256, 0, ("gemm1x1", (128, 1, 1), 256, 1, NONE)),
    row("persistent_k512", 128, 8, 512, 0, 256, T64X128, ("gemm1x1", (128, 1, 1), 256, 1, NONE)),
    # outside the predicates
    row("addvec", 128, 8, 256, 0, 256, 0, ("glds", (128, 1, 1), 256, 1, NONE), addvec=True),
    row("m_not_128", 3, 8, 256, 0, 256, 0, ("glds", (6, 1, 1), 128, 1, NONE)),
    row("kc64", 128, 8, 64, 0, 256, 0, ("gemm1x1", (128, 1, 1), 256, 1, NONE)),
]


def plan_of(c):
    L, K = _lib()
    d, _ = case_desc(c)
    p = K.conv_plan(d)
    return (L.CONV_FAMILIES[p.family], tuple(p.grid), p.block, p.splits, p.gn_part), p.whole_k


@pytest.mark.parametrize("c", ROWS, ids=[c["name"] for c in ROWS])
def test_option_off_is_the_parent_plan(c, dmc_opt):
    _lib()
    dmc_opt("DMC_GEMM1X1_WK", 0)
    assert plan_of(c) == (c["parent"], 0)


@pytest.mark.parametrize("c", ROWS, ids=[c["name"] for c in ROWS])
def test_option_on_plans_the_rule(c, dmc_opt):
    L, _ = _lib()
    assert L.get_option("DMC_GEMM1X1_WK") == 1   # the default
    plan, wk = plan_of(c)
    assert wk == c["tile"]
    if not c["tile"]:
        assert plan == c["parent"]
        return
    bm, bn = TILE[c["tile"]]
    M = c["N"] * c["S"] * c["S"]
    blocks = M // bm * (c["Cout"] // bn)
    runs = c["parent"][3]   # a split-K plan's runs: one wave each on the 64x64 tile
    assert plan == ("gemm1x1", (blocks, 1, 1), 64 * runs if runs > 1 else bm * bn // 64, 1, c["parent"][4])
    assert runs == 1 or (c["tile"] == T64 and runs <= 4)
    # the rule: at most 256 blocks, and the smaller tile would not have kept to that
    assert blocks <= 256
    assert c["tile"] == T64 or M // 64 * (c["Cout"] // 64) > 256


def test_per_tile_option_turns_the_form_off(dmc_opt):
    """DMC_GEMM1X1 = 0 is the per-tile LDS-DMA kernel for every 1x1 conv, the whole-K form included."""
    _lib()
    dmc_opt("DMC_GEMM1X1", 0)
    for c in ROWS:
        plan, wk = plan_of(c)
        assert wk == 0 and plan[0] == "glds", c["name"]


def test_rows_reach_every_tile():
    assert {c["tile"] for c in ROWS} == {0, T64X128, T64}
