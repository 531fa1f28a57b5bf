"""The token-wise kernels of csrc/dmc_dit.hip, per tensor, against tests/token_reference.py in fp64, at the edges of
their launch plans: every channel-ownership pattern of a lane (C = 4 ... 2048), uneven and capped row splits, padded
pitches, dropout masks against the host restatement of the counter hash, and the grid-stride loops.

Bounds (per tensor; the measured figure is printed beside its yardstick):
  fp32 tensors   error relative to the tensor's absmax <= 4x the error of the same reference evaluated in fp32 on the
                 CPU, floor 1e-6 (the rule of test_gpu_mamba_kernels.py).
  bf16 tensors   the reference gets the bf16-rounded inputs; per element |got - ref| <= 2^-8 |ref| + the fp32 allowance
                 above (one round-to-nearest bf16 step, 2^-9, doubled for the fp32 -> bf16 double rounding).
  channel sums   dscale, dshift, dgate, dbias, dgamma, dbeta and batch_sum add rows in sequence where torch adds them
                 pairwise. They are held to the fp32 rule first; a tensor that misses it must meet, per channel, the
                 sequential-summation bound n * 2^-24 * sum |term| with the terms of the fp64 reference (n = L rows of an
                 image; L + B where the B images are added in sequence after that: dbias, dgamma, dbeta; the row count
                 for batch_sum). The printed line says which of the two a tensor needed.
  exact cases    small-integer inputs (|v| <= 8, dropout p = 0.5): x_out, dbr, dshift, dgate, dsum and dbias are exact
                 in fp32 and in bf16 and must equal the fp64 result."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import token_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
U = 2.0 ** -24
EPS = 1e-6
SENT = 7.5                      # pitch padding / unused columns (exact in bf16)
SEED, SEED_WORD = 1234, 77      # "split": seed 1234 + a device word 77; "host": their sum as the host seed


def _k():
    from diffusion_models_collection_amd import _lib as L_
    from diffusion_models_collection_amd import kernels as K
    return L_, K


def absmax(t):
    return t.detach().double().abs().max().item()


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-300)).item()


def rb(t, dt):
    """t (fp32) rounded to the storage dtype, back in fp32."""
    return t.to(dt).float()


def yard(ref32, ref64):
    return max(4 * rel(ref32, ref64), 1e-6)


def check(name, got, ref64, ref32, dt=F32, terms=None, n=None):
    """One tensor against its bound (module docstring). terms: sum |term| per output element (channel sums only)."""
    got = got.detach().double().cpu().reshape(ref64.shape)
    y = yard(ref32, ref64)
    err = (got - ref64).abs()
    if dt == BF16:
        excess = (err - 2.0 ** -8 * ref64.abs()).max().item() / (absmax(ref64) + 1e-300)
        print(f"  {name} bf16: worst |err| - 2^-8|ref| = {excess:.3e} of absmax, fp32 allowance {y:.3e}, "
              f"plain rel {rel(got, ref64):.3e}")
        assert excess <= y, (name, excess, y)
        return
    e = rel(got, ref64)
    if terms is None or e <= y:
        print(f"  {name} fp32: {e:.3e} of absmax, yardstick {y:.3e} (4x fp32-CPU {y / 4:.3e})")
        assert e <= y, (name, e, y)
        return
    ratio = (err / (n * U * terms + 1e-300)).max().item()
    print(f"  {name} fp32: {e:.3e} of absmax misses the 4x yardstick {y:.3e}; NEEDS THE SUMMATION BOUND: worst "
          f"err / (n 2^-24 sum|term|) = {ratio:.3e}, n = {n}")
    assert ratio <= 1.0, (name, ratio, e, y)


def drop_spec(mode, p, L_):
    """(spec for the wrappers, keep-alive tensor) for mode in (None, 'host', 'split')."""
    if mode is None:
        return None, None
    thresh = min(int(round(p * 4294967296.0)), 4294967295)
    if mode == "host":
        return (SEED + SEED_WORD, thresh, 1.0 / (1.0 - p)), None
    word = torch.tensor([SEED_WORD], dtype=torch.int32, device=DEV)
    return (SEED, thresh, 1.0 / (1.0 - p), word.data_ptr()), word


def keep_mask(rows, C, p):
    thresh = min(int(round(p * 4294967296.0)), 4294967295)
    return torch.from_numpy(R.drop_mask(rows, C, SEED, thresh, SEED_WORD))


def expected_splits(B, L):
    return max(1, min(-(-1024 // B), L // 16, 64))


def assert_splits(B, C, L, S):
    L_, _ = _k()
    assert expected_splits(B, L) == S
    assert L_.LIB.dmc_dit_rowsum_workspace(B, C, L) == (B * S * 2 * C * 4 if S > 1 else 0)


# ---- LayerNorm + modulation, gate: one case = inputs + fp64 / fp32 references ----------------------------------------
class Case:
    pass


@functools.lru_cache(maxsize=None)
def block_case(dt, B, L, C, drop, affine):
    """Inputs (fp32 CPU tensors holding the storage-rounded values) and the references in fp64 and fp32."""
    g = torch.Generator().manual_seed(1000 * C + 10 * L + B)
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    T = B * L
    c = Case()
    c.B, c.L, c.C, c.T, c.p = B, L, C, T, 0.25
    c.x, c.br, c.dh, c.dy, c.dx0 = rn(T, C), rb(rn(T, C), dt), rb(rn(T, C), dt), rn(T, C), rn(T, C)
    c.shift, c.scale, c.gate = 0.5 * rn(B, C), 0.5 * rn(B, C), 0.5 * rn(B, C)
    c.gamma = 1 + 0.3 * rn(C) if affine else None
    c.beta = 0.3 * rn(C) if affine else None
    c.mask = keep_mask(T, C, c.p) if drop else None
    sc = 1.0 / (1.0 - c.p)
    c.ref = {}
    for D in (F64, F32):
        lv = lambda t: t.to(D).clone().requires_grad_(True)   # noqa: E731
        x, br, sh, scm, gt = lv(c.x), lv(c.br), lv(c.shift), lv(c.scale), lv(c.gate)
        gm, bt = (lv(c.gamma), lv(c.beta)) if affine else (None, None)
        m = c.mask.to(D) if drop else None
        h, xn, mean, rstd = R.ln_mod(x, sh, scm, L, EPS, br, gt, m, sc, gm, bt)
        xn.retain_grad()
        (h * c.dh.to(D)).sum().backward()
        r = dict(h=h, x_out=xn, mean=mean, rstd=rstd, dx=c.dx0.to(D) + xn.grad, dshift=sh.grad, dscale=scm.grad)
        if affine:
            r.update(dgamma=gm.grad, dbeta=bt.grad)
        br2, gt2, bias = lv(c.br), lv(c.gate), torch.zeros(C, dtype=D, requires_grad=True)
        (R.gated_branch(br2, gt2, L, m, sc, bias) * c.dy.to(D)).sum().backward()
        r.update(dbr=br2.grad, dgate=gt2.grad, dbias=bias.grad)
        c.ref[D] = {k: v.detach() for k, v in r.items()}
    # sum |term| of every channel sum, from the fp64 reference
    r = c.ref[F64]
    d64 = lambda t: t.double()   # noqa: E731
    img = lambda t: t.view(B, L, C).sum(1)   # noqa: E731
    xhat = (r["x_out"] - r["mean"][:, None]) * r["rstd"][:, None]
    m = c.mask.double() * sc if drop else torch.ones(T, C, dtype=F64)
    dh = d64(c.dh).abs()
    s1 = R.per_row(1 + d64(c.scale), L).abs()
    aA, aH = img(dh * xhat.abs()), img(dh)
    c.terms = dict(dshift=aH, dgate=img((d64(c.dy) * m * d64(c.br)).abs()),
                   dbias=(d64(c.dy) * R.per_row(d64(c.gate), L) * m).abs().sum(0))
    if affine:
        c.terms.update(dscale=d64(c.gamma).abs() * aA + d64(c.beta).abs() * aH,
                       dgamma=(s1 * dh * xhat.abs()).sum(0), dbeta=(s1 * dh).sum(0))
    else:
        c.terms.update(dscale=aA)
    return c


def rows_buf(v, ld, dt):
    """[T, C] values in rows of pitch ld (padding = SENT) on the device, in the storage dtype."""
    T, C = v.shape
    b = torch.full((T, ld), SENT, dtype=dt, device=DEV)
    b[:, :C] = v.to(DEV).to(dt)
    return b


def out_buf(T, ld, dt):
    return torch.full((T, ld), SENT, dtype=dt, device=DEV)


def pad_intact(buf, C):
    return bool((buf[:, C:] == SENT).all())


def mod_layout(C, pad):
    """(row width, shift / scale / gate offsets) of the stacked modulation rows."""
    return (4 * C + 8, 4, C + 8, 2 * C + 12) if pad else (3 * C, 0, C, 2 * C)


def mod_buf(c, pad):
    W, o_sh, o_sc, o_g = mod_layout(c.C, pad)
    mod = torch.full((c.B, W), SENT, dtype=F32, device=DEV)
    for off, v in ((o_sh, c.shift), (o_sc, c.scale), (o_g, c.gate)):
        mod[:, off:off + c.C] = v.to(DEV)
    return mod


def cols_intact(buf, C, offs):
    keep = torch.ones(buf.shape[1], dtype=torch.bool, device=buf.device)
    for o in offs:
        keep[o:o + C] = False
    return bool((buf[:, keep] == SENT).all())


def gate_bwd_bias_raw(dt, dy, br, ld_br, mod, W, o_g, T, C, L, drop, dbr, ld_dbr, dmod, dsum, dbias):
    """dmc_gate_bwd_bias with the caller's dsum rows [B][W] (the wrapper keeps them to itself)."""
    L_, K = _k()
    seed, base, thresh, scale = K.drop_args(drop)
    ws = K._rowsum_ws(T, C, L, dy.device)
    L_.check(L_.LIB.dmc_gate_bwd_bias(L_.dtype_code(dt), dy.data_ptr(), br.data_ptr(), ld_br, mod.data_ptr() + 4 * o_g,
                                      W, T, C, L, seed, base, thresh, scale, dbr.data_ptr(), ld_dbr,
                                      dmod.data_ptr() + 4 * o_g, dsum.data_ptr(), dbias.data_ptr(), L_.ptr(ws),
                                      L_.stream()), "dmc_gate_bwd_bias")


def run_block(dt, c, mode, pad, affine=False):
    """The four kernels of one block over case c -> dict of outputs (device tensors, tight views)."""
    L_, K = _k()
    B, L, C, T = c.B, c.L, c.C, c.T
    ld = C + 8 if pad else C
    W, o_sh, o_sc, o_g = mod_layout(C, pad)
    drop, word = drop_spec(mode, c.p, L_)
    x, dy = c.x.to(DEV), c.dy.to(DEV)
    br, dh = rows_buf(c.br, ld, dt), rows_buf(c.dh, ld, dt)
    mod = mod_buf(c, pad)
    mod0 = mod.clone()
    h, dbr, dbr2 = out_buf(T, ld, dt), out_buf(T, ld, dt), out_buf(T, ld, dt)
    xo = torch.empty(T, C, device=DEV)
    mean, rstd = torch.empty(T, device=DEV), torch.empty(T, device=DEV)
    dx = c.dx0.to(DEV).clone()
    dmod, dmod2 = torch.full_like(mod, SENT), torch.full_like(mod, SENT)
    dbias = torch.empty(C, device=DEV)
    out = {}
    if affine:
        gm, bt = c.gamma.to(DEV), c.beta.to(DEV)
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        K.ln_affine_mod_fwd(dt, x, T, C, L, mod, W, o_sh, o_sc, EPS, gm, bt, h, ld, mean, rstd, br=br, ld_br=ld,
                            off_gate=o_g, drop=drop, x_out=xo)
        K.ln_affine_mod_bwd(dt, dh, ld, xo, mean, rstd, mod, W, o_sc, T, C, L, gm, bt, dx, dmod, o_sc, o_sh, dg, db)
        out.update(dgamma=dg, dbeta=db)
    else:
        K.ln_mod_fwd(dt, x, T, C, L, mod, W, o_sh, o_sc, EPS, h, ld, mean, rstd, br=br, ld_br=ld, off_gate=o_g,
                     drop=drop, x_out=xo)
        K.ln_mod_bwd(dt, dh, ld, xo, mean, rstd, mod, W, o_sc, T, C, L, dx, dmod, o_sc, o_sh)
    K.gate_bwd(dt, dy, br, ld, mod, W, o_g, T, C, L, dbr, ld, dmod, o_g, drop=drop)
    K.gate_bwd_bias(dt, dy, br, ld, mod, W, o_g, T, C, L, dbr2, ld, dmod2, o_g, dbias, drop=drop)
    torch.cuda.synchronize()
    # nothing outside the rows and columns a kernel owns may change
    assert torch.equal(mod, mod0) and torch.equal(x, c.x.to(DEV)) and torch.equal(dy, c.dy.to(DEV))
    for b_ in (br, dh, h, dbr, dbr2):
        assert pad_intact(b_, C)
    assert cols_intact(dmod, C, (o_sh, o_sc, o_g)) and cols_intact(dmod2, C, (o_g,))
    out.update(h=h[:, :C], x_out=xo, mean=mean, rstd=rstd, dx=dx, dshift=dmod[:, o_sh:o_sh + C],
               dscale=dmod[:, o_sc:o_sc + C], dbr=dbr[:, :C], dgate=dmod[:, o_g:o_g + C], dbias=dbias,
               dbr2=dbr2[:, :C], dgate2=dmod2[:, o_g:o_g + C])
    return out


def check_block(dt, B, L, C, mode="host", pad=False, affine=False):
    c = block_case(dt, B, L, C, mode is not None, affine)
    o = run_block(dt, c, mode, pad, affine)
    r64, r32 = c.ref[F64], c.ref[F32]
    print(f"ln/gate {dt} B={B} L={L} C={C} drop={mode} pad={pad} affine={affine}")
    for k in ("h", "dbr"):
        check(k, o[k], r64[k], r32[k], dt)
    for k in ("x_out", "mean", "rstd", "dx"):
        check(k, o[k], r64[k], r32[k])
    for k in ("dshift", "dscale", "dgate"):
        check(k, o[k], r64[k], r32[k], terms=c.terms[k], n=L)
    for k in ("dbias",) + (("dgamma", "dbeta") if affine else ()):
        check(k, o[k], r64[k], r32[k], terms=c.terms[k], n=L + B)
    # gate_bwd_bias restates gate_bwd: same rows, same sums
    assert torch.equal(o["dbr2"], o["dbr"]) and torch.equal(o["dgate2"], o["dgate"])
    return o


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("C", [4, 256, 260, 512, 516, 2048])
def test_ln_gate_every_channel_pattern(dt, C):
    """A lane owns channels (lane + 64 k) * 4, k < 8: C = 4 (one lane), 256 (k = 0 full), 260 (one lane into k = 1),
    512 (one LDS slice of the backward exactly), 516 (four channels into the second slice), 2048 (the maximum, four
    slices). B = 3, L = 37: two uneven row splits (18 + 19), so the slices also pass through the split workspace.
    Forward and backward with branch dropout. Channel sums (dshift, dscale, dgate, dbias): module docstring."""
    assert_splits(3, C, 37, 2)
    check_block(dt, 3, 37, C)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("C", [516, 2048])
def test_ln_affine_at_the_slice_edges(dt, C):
    """ln_affine_mod_fwd / bwd (gamma, beta; dgamma and dbeta are channel sums over L rows, then B images)."""
    check_block(dt, 3, 37, C, affine=True)


SPLIT_SHAPES = [(3, 1, 64, 1), (3, 196, 260, 12), (2, 49, 64, 3), (2, 1040, 260, 64), (600, 64, 64, 2)]


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("B,L,C,S", SPLIT_SHAPES)
def test_ln_gate_row_splits(dt, B, L, C, S):
    """T % 4 != 0 with one split; 12 uneven splits (DiT on 28 x 28, patch 2); 3 uneven splits; the 64 cap with 16.25
    rows per split; the ceil(1024 / B) term binding at S = 2. Channel sums (dshift, dscale, dgate, dbias): module
    docstring."""
    assert_splits(B, C, L, S)
    check_block(dt, B, L, C, mode=None if (B, L) == (2, 49) else "split")


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("B,L,C,S", SPLIT_SHAPES + [(3, 37, 516, 2)])
def test_row_coverage_is_exact_on_small_integers(dt, B, L, C, S):
    """Integer inputs in [-8, 8], integer gate, dropout p = 0.5 (scale 2): x_out, dbr, dshift = sum dh,
    dgate = sum dy drop(br), dsum = sum dy mask and dbias = sum_b gate dsum are exact in fp32 (every partial sum is an
    integer below 2^24) and in bf16 (|dbr| <= 128), so a dropped or doubled row shows whatever the tolerance."""
    L_, K = _k()
    assert_splits(B, C, L, S)
    g = torch.Generator().manual_seed(B * L + C)
    ri = lambda *s: torch.randint(-8, 9, s, generator=g).float()   # noqa: E731
    T = B * L
    c = Case()
    c.B, c.L, c.C, c.T, c.p = B, L, C, T, 0.5
    c.x, c.br, c.dh, c.dy = ri(T, C), ri(T, C), ri(T, C), ri(T, C)
    c.shift, c.scale, c.gate = ri(B, C), ri(B, C), ri(B, C)
    m2 = keep_mask(T, C, 0.5).double() * 2
    drop, word = drop_spec("split", 0.5, L_)
    W, o_sh, o_sc, o_g = mod_layout(C, False)
    mod = mod_buf(c, False)
    x, dy, br, dh = c.x.to(DEV), c.dy.to(DEV), c.br.to(DEV).to(dt), c.dh.to(DEV).to(dt)
    h, dbr, dbr2 = (torch.empty(T, C, dtype=dt, device=DEV) for _ in range(3))
    xo, dx = torch.empty(T, C, device=DEV), torch.zeros(T, C, device=DEV)
    mean, rstd = torch.empty(T, device=DEV), torch.empty(T, device=DEV)
    dmod, dmod2 = torch.zeros_like(mod), torch.zeros_like(mod)
    dsum = torch.full((B, W), SENT, device=DEV)
    dbias = torch.empty(C, device=DEV)
    K.ln_mod_fwd(dt, x, T, C, L, mod, W, o_sh, o_sc, EPS, h, C, mean, rstd, br=br, ld_br=C, off_gate=o_g, drop=drop,
                 x_out=xo)
    K.ln_mod_bwd(dt, dh, C, xo, mean, rstd, mod, W, o_sc, T, C, L, dx, dmod, o_sc, o_sh)
    K.gate_bwd(dt, dy, br, C, mod, W, o_g, T, C, L, dbr, C, dmod, o_g, drop=drop)
    gate_bwd_bias_raw(dt, dy, br, C, mod, W, o_g, T, C, L, drop, dbr2, C, dmod2, dsum, dbias)
    torch.cuda.synchronize()
    d = lambda t: t.double()   # noqa: E731
    img = lambda t: t.view(B, L, C).sum(1)   # noqa: E731
    gr = R.per_row(d(c.gate), L)
    want = {"x_out": d(c.x) + gr * m2 * d(c.br), "dbr": d(c.dy) * gr * m2, "dshift": img(d(c.dh)),
            "dgate": img(d(c.dy) * m2 * d(c.br)), "dsum": img(d(c.dy) * m2)}
    want["dbias"] = (d(c.gate) * want["dsum"]).sum(0)
    got = {"x_out": xo, "dbr": dbr, "dshift": dmod[:, o_sh:o_sh + C], "dgate": dmod[:, o_g:o_g + C],
           "dsum": dsum[:, :C], "dbias": dbias}
    assert max(absmax(v) for v in want.values()) < 2 ** 24
    for k, w in want.items():
        bad = int((got[k].double().cpu().reshape(w.shape) != w).sum())
        print(f"exact {dt} B={B} L={L} C={C} {k}: {bad} of {w.numel()} elements differ (absmax {absmax(w):.0f})")
    for k, w in want.items():
        assert torch.equal(got[k].double().cpu().reshape(w.shape), w), k
    assert torch.equal(dbr2, dbr) and torch.equal(dmod2[:, o_g:o_g + C], dmod[:, o_g:o_g + C])
    assert bool((dsum[:, C:] == SENT).all())


@pytest.mark.parametrize("dt", [F32, BF16])
def test_ln_gate_padded_pitches(dt):
    """ld_br, ld_h, ld_dh, ld_dbr = C + 8 and mod = [B][3C + 8 + C] with shift / scale / gate at columns 4, C + 8 and
    2C + 12; the padding and every unused column hold a sentinel that must come back bit-identical (run_block), and
    the outputs -- dropout mask included -- are bitwise those of the tight layout. Plain and affine kernels."""
    B, L, C = 3, 37, 260
    for affine in (False, True):
        c = block_case(dt, B, L, C, True, affine)
        tight = run_block(dt, c, "host", False, affine)
        o = check_block(dt, B, L, C, mode="host", pad=True, affine=affine)
        for k in o:
            assert torch.equal(o[k], tight[k]), k


# ---- dropout masks ---------------------------------------------------------------------------------------------------
def _nonzero(g, *s):
    """Values with 1 <= |v| <= 3 (exact in bf16 or not: never 0, GELU and its derivative never 0 either)."""
    return (1 + 2 * torch.rand(*s, generator=g)) * (torch.randint(0, 2, s, generator=g) * 2 - 1).float()


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("mode", [None, "host", "split"])
def test_dropout_zero_patterns_are_the_host_mask(dt, mode, pad):
    """With every operand nonzero (and x = 0, so that x_out = gate * drop(br) exactly) the zero pattern of the forward
    (ln_mod_fwd's x_out, gelu_fwd's a) and of the backward (gate_bwd and gate_bwd_bias's dbr; gelu_bwd and
    gelu_bwd_f32in's du) is the keep mask of drop_keep_np over row * C + c, bit for bit; without dropout nothing is 0.
    The seed is given on the host, or split over the host seed and a device word."""
    L_, K = _k()
    B, L, C, p = 3, 37, 260, 0.25
    T = B * L
    g = torch.Generator().manual_seed(11)
    c = Case()
    c.B, c.L, c.C, c.T, c.p = B, L, C, T, p
    c.x, c.br, c.dy = torch.zeros(T, C), _nonzero(g, T, C), _nonzero(g, T, C)
    c.shift, c.scale, c.gate = _nonzero(g, B, C), _nonzero(g, B, C), _nonzero(g, B, C)
    keep = keep_mask(T, C, p) if mode else torch.ones(T, C, dtype=torch.bool)
    assert mode is None or 0.7 < keep.float().mean().item() < 0.8
    drop, word = drop_spec(mode, p, L_)
    ld = C + 8 if pad else C
    W, o_sh, o_sc, o_g = mod_layout(C, pad)
    mod = mod_buf(c, pad)
    br = rows_buf(c.br, ld, dt)
    h, dbr, dbr2 = out_buf(T, ld, dt), out_buf(T, ld, dt), out_buf(T, ld, dt)
    xo = torch.empty(T, C, device=DEV)
    mean, rstd = torch.empty(T, device=DEV), torch.empty(T, device=DEV)
    dmod, dbias = torch.zeros_like(mod), torch.empty(C, device=DEV)
    K.ln_mod_fwd(dt, c.x.to(DEV), T, C, L, mod, W, o_sh, o_sc, EPS, h, ld, mean, rstd, br=br, ld_br=ld, off_gate=o_g,
                 drop=drop, x_out=xo)
    K.gate_bwd(dt, c.dy.to(DEV), br, ld, mod, W, o_g, T, C, L, dbr, ld, dmod, o_g, drop=drop)
    K.gate_bwd_bias(dt, c.dy.to(DEV), br, ld, mod, W, o_g, T, C, L, dbr2, ld, dmod, o_g, dbias, drop=drop)
    u, da = rows_buf(c.br, ld, dt), rows_buf(c.dy, ld, dt)
    da32 = rows_buf(c.dy, ld, F32)
    a, du, du32 = out_buf(T, ld, dt), out_buf(T, ld, dt), out_buf(T, ld, dt)
    K.gelu_fwd(dt, u, T, C, ld, a, drop=drop)
    K.gelu_bwd(dt, da, u, T, C, ld, du, drop=drop)
    K.gelu_bwd_f32in(dt, da32, u, T, C, ld, du32, drop=drop)
    torch.cuda.synchronize()
    outs = {"ln_mod_fwd x_out": xo, "gate_bwd dbr": dbr[:, :C], "gate_bwd_bias dbr": dbr2[:, :C],
            "gelu_fwd a": a[:, :C], "gelu_bwd du": du[:, :C], "gelu_bwd_f32in du": du32[:, :C]}
    for k, v in outs.items():
        diff = int(((v != 0).cpu() != keep).sum())
        print(f"mask {dt} mode={mode} pad={pad} {k}: {diff} elements off the host mask")
    for k, v in outs.items():
        assert torch.equal((v != 0).cpu(), keep), k
    for b_ in (h, dbr, dbr2, a, du, du32):
        assert pad_intact(b_, C)


# ---- GELU ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gelu_case(dt, rows, C, drop):
    g = torch.Generator().manual_seed(rows + C)
    c = Case()
    c.p = 0.1
    c.u = rb(torch.randn(rows, C, generator=g) * 3, dt)
    c.da32 = torch.randn(rows, C, generator=g)         # the unrounded gradient gelu_bwd_f32in reads
    c.da = rb(c.da32, dt)
    mask = keep_mask(rows, C, c.p) if drop else None
    c.ref = {}
    for D in (F64, F32):
        u = c.u.to(D).clone().requires_grad_(True)
        a = R.gelu(u, None if mask is None else mask.to(D), 1.0 / (1.0 - c.p))
        a.sum().backward()                              # the op is elementwise: du = da * (d a / d u)
        c.ref[D] = dict(a=a.detach(), du=c.da.to(D) * u.grad, du32=c.da32.to(D) * u.grad)
    return c


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("rows,C,mode,pad", [(777, 96, None, False), (777, 96, "host", False), (777, 96, "split", True),
                                            (333, 4, "host", False), (8200, 1028, "split", False)])
def test_gelu_matches_fp64_reference(dt, rows, C, mode, pad):
    """gelu_fwd, gelu_bwd and gelu_bwd_f32in (in bf16 its da stays fp32: the reference gets the unrounded da) with and
    without dropout; 8200 x 1028 is 2,107,400 float4 groups, past the 2,097,152 threads of the capped grid, so the
    grid-stride loop takes a second trip; C = 4 is one group per row; ld = C + 8 with sentinel padding."""
    L_, K = _k()
    assert (rows * C // 4 > 8192 * 256) == (rows == 8200)
    c = gelu_case(dt, rows, C, mode is not None)
    drop, word = drop_spec(mode, c.p, L_)
    ld = C + 8 if pad else C
    u, da, da32 = rows_buf(c.u, ld, dt), rows_buf(c.da, ld, dt), rows_buf(c.da32, ld, F32)
    a, du, du32 = out_buf(rows, ld, dt), out_buf(rows, ld, dt), out_buf(rows, ld, dt)
    K.gelu_fwd(dt, u, rows, C, ld, a, drop=drop)
    K.gelu_bwd(dt, da, u, rows, C, ld, du, drop=drop)
    K.gelu_bwd_f32in(dt, da32, u, rows, C, ld, du32, drop=drop)
    torch.cuda.synchronize()
    print(f"gelu {dt} {rows}x{C} drop={mode} pad={pad}")
    for k, v in (("a", a), ("du", du), ("du32", du32)):
        check(k, v[:, :C], c.ref[F64][k], c.ref[F32][k], dt)
        assert pad_intact(v, C)
    if dt == F32:
        assert torch.equal(du, du32)


# ---- embedding and layout helpers --------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_period", [10000.0, 100.0])
@pytest.mark.parametrize("dim", [2, 255, 256])
def test_timestep_embedding(dim, max_period):
    """1e-4 of the absmax (1): cos / sin of arguments t * f up to ~1000, where one ulp of the fp32 argument (the device
    exp of the frequencies against the host's) moves the result by ~6e-5. The odd dim's last column is 0."""
    _, K = _k()
    t = torch.tensor([0, 1, 999], dtype=torch.long)
    out = torch.full((3, dim), SENT, device=DEV)
    K.timestep_embedding(t.to(DEV), dim, out, max_period=max_period)
    ref = R.timestep_embedding(t, dim, max_period)
    ref32 = R.timestep_embedding(t, dim, max_period, dtype=F32)
    print(f"timestep_embedding dim={dim} period={max_period}: {rel(out, ref):.3e} (fp32-CPU {rel(ref32, ref):.3e}), "
          f"bound 1e-4")
    assert rel(out, ref) < 1e-4
    if dim % 2:
        assert torch.count_nonzero(out[:, -1]) == 0


@pytest.mark.parametrize("rows,n", [(2, 8192 * 256 + 259), (1, 1000), (7, 1000)])
def test_batch_sum(rows, n):
    """n past the 2,097,152 threads of the capped grid (a second grid-stride trip); one row (a copy, exact); the
    existing shape. A channel sum over `rows` terms added in sequence (module docstring)."""
    _, K = _k()
    x = torch.randn(rows, n, generator=torch.Generator().manual_seed(n))
    s = torch.full((n,), SENT, device=DEV)
    K.batch_sum(x.to(DEV), rows, n, s)
    print(f"batch_sum rows={rows} n={n}")
    check("sum", s, x.double().sum(0), x.sum(0), terms=x.double().abs().sum(0), n=rows)
    if rows == 1:
        assert torch.equal(s.cpu(), x[0])


@pytest.mark.parametrize("B,C,H,p,ht,wt,ld", [(1, 3, 4, 2, 420, 420, 8), (1, 3, 64, 2, 1, 1, 64), (2, 3, 64, 2, 4, 5, 64)])
def test_patch_dgrad(B, C, H, p, ht, wt, ld):
    """The patch embedding's input gradient against conv_transpose2d (stride = kernel = p) in fp64: 3 x 840 x 840 =
    2,116,800 outputs, past the capped grid, from token rows of pitch H + 4; one token row; the existing shape."""
    _, K = _k()
    g = torch.Generator().manual_seed(ht)
    assert (B * C * ht * p * wt * p > 8192 * 256) == (ht == 420)
    dtok = torch.randn(B, ht, wt, H, generator=g)
    w = torch.randn(H, C, p, p, generator=g)
    buf = torch.full((B, ht, wt, ld), 1e6, device=DEV)
    buf[..., :H] = dtok.to(DEV)
    dx = torch.full((B, C, ht * p, wt * p), SENT, device=DEV)
    K.patch_dgrad(buf, ld, w.to(DEV), B, ht, wt, p, C, H, dx)
    ref = F.conv_transpose2d(dtok.double().permute(0, 3, 1, 2), w.double(), stride=p)
    ref32 = F.conv_transpose2d(dtok.permute(0, 3, 1, 2), w, stride=p)
    print(f"patch_dgrad B={B} {ht}x{wt} H={H}")
    check("dx", dx, ref, ref32)


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_what_the_kernels_cannot_index():
    """C % 4 != 0, C = 2052 (> 2048), T % L != 0, a branch without its gate, and a pitch that is not a multiple of 4
    (the 8- and 16-byte vector accesses) -- forward and backward entry points alike, before any launch."""
    L_, K = _k()
    E = L_.DMCError
    t = torch.zeros(8, 4096, device=DEV)
    tb = torch.zeros(8, 4096, device=DEV, dtype=BF16)
    v = torch.zeros(8, device=DEV)
    g = torch.zeros(64, device=DEV)

    def fwd(C=64, T=8, L=4, ld_h=64, ld_br=64, ld_mod=256, br=t, aff=False):
        if aff:
            K.ln_affine_mod_fwd(F32, t, T, C, L, t, ld_mod, 0, C, EPS, g, g, t, ld_h, v, v, br=br, ld_br=ld_br,
                                off_gate=2 * C, x_out=None)
        else:
            K.ln_mod_fwd(F32, t, T, C, L, t, ld_mod, 0, C, EPS, t, ld_h, v, v, br=br, ld_br=ld_br, off_gate=2 * C)

    def bwd(C=64, T=8, L=4, ld_dh=64, ld_mod=256, aff=False):
        if aff:
            K.ln_affine_mod_bwd(F32, t, ld_dh, t, v, v, t, ld_mod, C, T, C, L, g, g, t, t, C, 0, g, g)
        else:
            K.ln_mod_bwd(F32, t, ld_dh, t, v, v, t, ld_mod, C, T, C, L, t, t, C, 0)

    def gate(C=64, T=8, L=4, ld_br=64, ld_dbr=64, ld_mod=256, bias=False):
        if bias:
            K.gate_bwd_bias(F32, t, t, ld_br, t, ld_mod, 2 * C, T, C, L, t, ld_dbr, t, 2 * C, g)
        else:
            K.gate_bwd(F32, t, t, ld_br, t, ld_mod, 2 * C, T, C, L, t, ld_dbr, t, 2 * C)

    for aff in (False, True):
        for kw in (dict(C=62), dict(C=2052, ld_h=2052, ld_br=2052, ld_mod=8192), dict(T=7), dict(ld_h=66),
                   dict(ld_br=66), dict(ld_mod=258)):
            with pytest.raises(E):
                fwd(aff=aff, **kw)
        for kw in (dict(C=62), dict(C=2052, ld_dh=2052, ld_mod=8192), dict(T=7), dict(ld_dh=66), dict(ld_mod=258)):
            with pytest.raises(E):
                bwd(aff=aff, **kw)
    for bias in (False, True):
        for kw in (dict(C=62), dict(C=2052, ld_br=2052, ld_dbr=2052, ld_mod=8192), dict(T=7), dict(ld_br=66),
                   dict(ld_dbr=66), dict(ld_mod=258)):
            with pytest.raises(E):
                gate(bias=bias, **kw)
    # a branch without a gate: the C entry point (the wrappers derive the gate from mod)
    with pytest.raises(E, match="gate"):
        L_.check(L_.LIB.dmc_ln_mod_fwd(L_.DMC_F32, t.data_ptr(), t.data_ptr(), 64, None, t.data_ptr(), t.data_ptr(),
                                       256, 8, 64, 4, EPS, 0, None, 0, 1.0, None, t.data_ptr(), 64, v.data_ptr(),
                                       v.data_ptr(), L_.stream()), "dmc_ln_mod_fwd")
    for dt, buf in ((F32, t), (BF16, tb)):
        for kw in (dict(C=62, ld=64), dict(C=64, ld=66)):
            with pytest.raises(E):
                K.gelu_fwd(dt, buf, 8, kw["C"], kw["ld"], buf)
            with pytest.raises(E):
                K.gelu_bwd(dt, buf, buf, 8, kw["C"], kw["ld"], buf)
            with pytest.raises(E):
                K.gelu_bwd_f32in(dt, t, buf, 8, kw["C"], kw["ld"], buf)
    torch.cuda.synchronize()
    assert torch.count_nonzero(t) == 0 and torch.count_nonzero(tb) == 0      # nothing was launched
