"""The attention kernels of csrc/dmc_attn.hip at head dims 72..128 (the 128-wide pad), each output tensor on its own.

Same rule, references and launch harness as tests/test_gpu_attn_kernels.py, whose helpers are imported: for each of
o, lse, dq, dk, dv,  max|kernel - f64| <= k * max|yardstick - f64| + floor  with k = 4 for fp32 tensors and lse, k = 2
for bf16 tensors and the floors of attn_reference.floors; every check prints an `attn-ratio` line; every launch runs
inside NaN-sentinel buffers that must come back untouched outside the payload. Measured ratios: DESIGN.md section 4.

What is specific to the wide pad:
  * hd = 72 and 96 leave whole 16-byte chunks (and whole 16-wide output tiles) of the pad empty: the d guards of the
    loads, the staging and the stores are all that keeps them inside the row;
  * bf16 runs the row-resident kernels up to L = 256 (auto, hg1, hg2, hg4) and the staged ones above or when forced;
    the dK/dV tile body has a form of its own above 64 (per key chunk), so resident-equals-staged and
    head-group-equals-hg1 are asserted again here;
  * fp32 above 64 has no resident kernels: auto and every hgK must give the staged result bit for bit.
"""
import pytest
import torch

from test_gpu_attn_kernels import (BF16, DTYPES, F32, NAME, SENT, _lib, _refusal_buffers, accuracy, assert_same, bits,
                                   randn_case, run_case, same_bits, set_path)

pytestmark = pytest.mark.gpu

# L: 16 = a 4x4 map, a quarter of one key tile; 64; 80 = a ragged second tile; 256 = the resident limit; 272 = staged by
# length, ragged. hd 72 at every L, 96 and 128 where the launch plan or the tile count changes.
LS = {72: (16, 64, 80, 256, 272), 96: (16, 80, 256, 272), 128: (16, 80, 256, 272)}


def paths(Lq):
    """auto and staged everywhere; forced head groups where the padded length leaves room for them in 256 rows."""
    if Lq > 256:
        return ("auto", "staged")
    Lp = (Lq + 63) // 64 * 64
    return ("auto", "staged", "hg1") + tuple(f"hg{g}" for g in (2, 4) if g <= 256 // Lp)


SHAPES = [(L_, hd) for hd, ls in LS.items() for L_ in ls]
CASES = [pytest.param(dt, L_, hd, path, id=f"{NAME[dt]}-L{L_}-hd{hd}-{path}")
         for dt in DTYPES for (L_, hd) in SHAPES for path in paths(L_)]

_RESULTS = {}


def result(dmc_opt, dt, N, Lq, heads, hd, path):
    """One launch per (case, path), shared between the accuracy and the agreement tests: read-only."""
    key = (dt, N, Lq, heads, hd, path)
    if key not in _RESULTS:
        set_path(dmc_opt, path)
        _RESULTS[key] = run_case(dt, randn_case(dt, N, Lq, heads, hd))
    return _RESULTS[key]


@pytest.mark.parametrize("dt,Lq,hd,path", CASES)
def test_wide_shapes(dt, Lq, hd, path, dmc_opt):
    """N = 2, heads = 3, every launch path of the shape."""
    got = result(dmc_opt, dt, 2, Lq, 3, hd, path)
    accuracy(f"wide L{Lq} hd{hd} {path}", dt, got, randn_case(dt, 2, Lq, 3, hd))


@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("Lq,hd", [s for s in SHAPES if s[0] <= 256])
def test_wide_paths_agree(dt, Lq, hd, dmc_opt):
    """bf16: the resident and the staged kernels run the same tile bodies over the same keys in the same order, and
    within the resident kernels only the runtime HG differs, so every path gives the bits of `staged`. fp32 has no
    resident form above 64: auto and every forced head group must launch the staged kernels, hence the same bits."""
    stg = result(dmc_opt, dt, 2, Lq, 3, hd, "staged")
    for path in paths(Lq):
        if path != "staged":
            assert_same(result(dmc_opt, dt, 2, Lq, 3, hd, path), stg, f"{path} against staged")


@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("hg", [2, 4])
def test_wide_short_last_block(dt, hg, dmc_opt):
    """heads = 5 at L = 64: blocks of 2, 2, 1 and of 4, 1 heads (bf16; all 256 LDS rows in use with hg4)."""
    heads, Lq, hd = 5, 64, 72
    case = randn_case(dt, 2, Lq, heads, hd)
    got = result(dmc_opt, dt, 2, Lq, heads, hd, f"hg{hg}")
    accuracy(f"wide hg{hg} heads{heads} L{Lq} hd{hd}", dt, got, case)
    assert_same(got, result(dmc_opt, dt, 2, Lq, heads, hd, "hg1"), f"HG {hg} against HG 1")


@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("path", ["auto", "staged"])
def test_wide_padded_pitches_and_offset_bases(dt, path, dmc_opt):
    """hd = 72 under the 128-wide pad, ragged L, with qkv / out / dqkv as column slices of wider allocations (pitches
    3C + 8, C + 16, 3C + 8; bases 8 columns in). A chunk or an output tile past d = 72 that was not masked lands in
    the next head's columns or, for the last head, in the NaN padding: launch() checks the padding, the guard row and
    the elements behind lse, and the result must equal the dense run bit for bit."""
    heads, Lq, hd = 3, 80, 72
    case = randn_case(dt, 2, Lq, heads, hd)
    dense = result(dmc_opt, dt, 2, Lq, heads, hd, path)
    set_path(dmc_opt, path)
    padded = run_case(dt, case, pads=(8, 16, 8), offs=(8, 8, 8))
    accuracy(f"wide pitch {path} L{Lq} hd{hd}", dt, padded, case)
    assert_same(padded, dense, "padded pitches against dense")


DROP = (4242, 0.1)
DROP_CASES = [("hg2", 3, 64, 72), ("auto", 2, 100, 128), ("staged", 2, 272, 96)]


@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("path,heads,Lq,hd", DROP_CASES)
def test_wide_dropout(dt, path, heads, Lq, hd, dmc_opt):
    """p = 0.1 against the reference with the host-rebuilt keep mask (bf16 hg2 / auto: the resident DROP kernels, the
    dK/dV one being the kernel that spilled before its body was split). lse is that of the undropped softmax."""
    set_path(dmc_opt, path)
    case = randn_case(dt, 2, Lq, heads, hd, DROP)
    got = run_case(dt, case, drop=case["spec"])
    accuracy(f"wide drop {path} heads{heads} L{Lq} hd{hd}", dt, got, case)
    plain = run_case(dt, case, backward=False)
    assert same_bits(got["lse"], plain["lse"])
    assert not same_bits(got["o"], plain["o"])


@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("path,Lq,hd,drop", [("auto", 80, 72, None), ("staged", 272, 128, None), ("hg2", 64, 72, DROP)])
def test_wide_is_deterministic(dt, path, Lq, hd, drop, dmc_opt):
    """Two launches of one case, forward and backward, give the same bits."""
    set_path(dmc_opt, path)
    case = randn_case(dt, 2, Lq, 3, hd, drop)
    assert_same(run_case(dt, case, drop=case["spec"]), run_case(dt, case, drop=case["spec"]), "second launch")


@pytest.mark.parametrize("dt,hd", [(F32, 136), (BF16, 136), (F32, 132), (BF16, 132), (F32, 100), (BF16, 68)],
                         ids=lambda v: NAME.get(v, str(v)))
def test_wide_refused_head_dims(dt, hd):
    """Above 128, and above 64 anything that is not a multiple of 8, is refused before a launch with a text naming the
    head dim; the outputs keep their sentinel."""
    L, K = _lib()
    heads, N, Lq = 2, 1, 16
    C = heads * hd
    qkv, out, dout, dqkv, lse = _refusal_buffers(dt, N * Lq + 1, 3 * C + 8)
    with pytest.raises(L.DMCError, match=r"dmc_attn_fwd failed \([1-9]\d*\): .*attn: head dim"):
        K.attn_fwd(dt, qkv, 3 * C, N, Lq, heads, hd, out, C, lse)
    with pytest.raises(L.DMCError, match=r"dmc_attn_bwd failed \([1-9]\d*\): .*attn: head dim"):
        K.attn_bwd(dt, qkv, 3 * C, out, dout, C, lse, N, Lq, heads, hd, dqkv, 3 * C)
    torch.cuda.synchronize()
    for t in (out, dqkv, lse):
        assert bool((bits(t.cpu()) == SENT[t.dtype][1]).all())
