"""Numerics of the scan-order entry points of csrc/dmc_mamba.hip (dmc_selective_scan_fwd/bwd_ord,
dmc_causal_conv_silu_fwd/bwd_ord) against tests/scan_order_reference.py in fp64: "permute the tokens, run
tests/mamba_reference.py, un-permute".

Bounds are those of tests/test_gpu_mamba_kernels.py, with its input recipe (delta pre-activations -5 ... 25) and the
executor's layouts (z at column E of [T, 2E] rows, dBm | dCm rows with 8 pad columns that must come back zero):
  scan fp32   per tensor (y and every gradient), error relative to absmax <= max(4 x the error of the same reference
              evaluated in fp32 on the CPU, 1e-6); two runs bitwise equal.
  scan bf16   a bf16-stored tensor per element within 2^-8 |ref| + that allowance times the absmax; dA_log, dD fp32.
  conv fp32   u, dx elementwise rtol = atol = 2e-5; dw, dbias < 1e-5 of absmax; the backward twice, bitwise equal.
  conv bf16   u, dx per element within 2^-8 |ref| + the fp32 allowance times the absmax; dw, dbias the fp32 bound.
Token grids (h, w): (1, 1), (2, 2) L <= 4, the conv's whole window is boundary; (1, 33), (33, 1) one line, two chunks
with a 1-token tail (col and row each degenerate in one); (5, 7) L = 35, odd line count and length, so snake's last
line is a reversed one, 3-token tail; (6, 11) L = 66, three chunks; conv (5, 13) L = 65: with B = 3, E = 80 the
backward plan has 8 segments.
Order 0 through the _ord entry points is bitwise the plain entry points; an order in place is bitwise the plain entry
points on row-gathered inputs with the outputs scattered back (same arithmetic in the same order)."""
import functools

import pytest
import torch

from scan_order_reference import ORDERS, causal_conv_silu_ord, permutation, selective_scan_ord

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 16
F32, BF16 = torch.float32, torch.bfloat16
SENT = 7.5
NAMES = ("u", "z", "dpre", "Bm", "Cm", "A_log", "D", "bias")
STORED = ("y", "u", "z", "dpre", "Bm", "Cm")       # in the storage dtype
FEW = ("row_rev", "col", "snake_col_rev")
SMALL = [(1, 1), (2, 2), (1, 33), (33, 1)]
SCAN_CASES = ([(h, w, o) for h, w in ((5, 7), (6, 11)) for o in ORDERS] + [(h, w, o) for h, w in SMALL for o in FEW])


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-300)).item()


# ---- selective scan --------------------------------------------------------------------------------------------
def _scan_inputs(E, L, B, dt=F32):
    """The recipe of test_gpu_mamba_kernels._scan_inputs; in bf16 mode u, z and dy are bf16-representable."""
    g = torch.Generator().manual_seed(100 * E + L)
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    u, z = rn(B, L, E), rn(B, L, E)
    dpre = torch.rand(B, L, E, generator=g) * 30 - 5
    Bm, Cm = rn(B, L, N), rn(B, L, N)
    A_log = torch.log(torch.arange(1, N + 1, dtype=torch.float32)).repeat(E, 1) + 0.2 * rn(E, N)
    D = 1 + 0.2 * rn(E)
    bias = 0.3 * rn(E)
    dy = rn(B, L, E)
    if dt == BF16:
        u, z, dy = (t.bfloat16().float() for t in (u, z, dy))
    return dict(u=u, z=z, dpre=dpre, Bm=Bm, Cm=Cm, A_log=A_log, D=D, bias=bias), dy


@functools.lru_cache(maxsize=None)
def _scan_reference(E, h, w, order, B, dt):
    """{fp64, fp32: tensors by name ("y" and the gradient of every input)} of the order's reference."""
    inp, dy = _scan_inputs(E, h * w, B, dt)
    res = {}
    for D_ in (torch.float64, torch.float32):
        v = {k: t.to(D_).clone().requires_grad_(True) for k, t in inp.items()}
        y = selective_scan_ord(v["u"], v["z"], v["dpre"], v["Bm"], v["Cm"], v["A_log"], v["D"], v["bias"], order, h, w)
        (y * dy.to(D_)).sum().backward()
        r = {k: v[k].grad for k in NAMES}
        r["y"] = y.detach()
        res[D_] = r
    return res


def _run_scan(dt, E, h, w, B, order, gather=None):
    """Forward and backward in storage dtype dt -> {"y", gradients by input name} (device tensors, [T, .] rows).
    order: None = the plain entry points, else the _ord entry points with that order's code.
    gather: (perm, inv) = the plain entry points on the row-gathered inputs, the per-token outputs scattered back."""
    from diffusion_models_collection_amd import kernels as K
    L = h * w
    T = B * L
    inp, dy = _scan_inputs(E, L, B, dt)
    d = {k: t.to(DEV).contiguous() for k, t in inp.items()}
    rows = lambda t, c, D_: t.reshape(T, c).to(DEV).to(D_).contiguous()    # noqa: E731
    u, dyb = rows(inp["u"], E, dt), rows(dy, E, dt)
    dpre = rows(inp["dpre"], E, F32)
    bc = rows(torch.cat([inp["Bm"], inp["Cm"]], dim=-1), 2 * N, F32)
    xz = torch.full((T, 2 * E), SENT, dtype=dt, device=DEV)               # z at column E
    xz[:, E:] = rows(inp["z"], E, dt)
    if gather is not None:
        perm = gather[0].to(DEV)
        idx = (torch.arange(B, device=DEV)[:, None] * L + perm[None]).reshape(T)
        u, dyb, dpre, bc, xz = (t[idx].contiguous() for t in (u, dyb, dpre, bc, xz))
    y, du, ddp = (torch.full((T, E), SENT, dtype=dt, device=DEV) for _ in range(3))
    dxz = torch.full((T, 2 * E), SENT, dtype=dt, device=DEV)
    dbc = torch.full((T, 2 * N + 8), SENT, dtype=dt, device=DEV)          # 8 pad columns: must come back zero
    dA, dD = torch.empty(E, N, device=DEV), torch.empty(E, device=DEV)
    states = K.scan_states(B, L, E, N, DEV)
    if order is None:
        K.selective_scan_fwd(dt, u, E, xz, 2 * E, E, dpre, E, bc, 2 * N, 0, N, d["A_log"], d["D"], d["bias"], B, L, E, N,
                             states, y, E)
        K.selective_scan_bwd(dt, dyb, E, u, E, xz, 2 * E, E, dpre, E, bc, 2 * N, 0, N, d["A_log"], d["D"], d["bias"],
                             B, L, E, N, states, du, E, dxz, 2 * E, E, ddp, E, dbc, 2 * N + 8, 0, dA, dD)
    else:
        code = ORDERS.index(order)
        K.selective_scan_fwd_ord(dt, u, E, xz, 2 * E, E, dpre, E, bc, 2 * N, 0, N, d["A_log"], d["D"], d["bias"], B, h,
                                 w, code, E, N, states, y, E)
        K.selective_scan_bwd_ord(dt, dyb, E, u, E, xz, 2 * E, E, dpre, E, bc, 2 * N, 0, N, d["A_log"], d["D"],
                                 d["bias"], B, h, w, code, E, N, states, du, E, dxz, 2 * E, E, ddp, E, dbc, 2 * N + 8, 0,
                                 dA, dD)
    torch.cuda.synchronize()
    assert bool((dxz[:, :E] == SENT).all()) and torch.count_nonzero(dbc[:, 2 * N:]) == 0
    tok = {"y": y, "u": du, "z": dxz[:, E:], "dpre": ddp, "Bm": dbc[:, :N], "Cm": dbc[:, N:2 * N]}
    if gather is not None:
        back = torch.empty_like(idx)
        back[idx] = torch.arange(T, device=DEV)
        tok = {k: t[back] for k, t in tok.items()}
    got = {k: t.contiguous() for k, t in tok.items()}
    got.update(A_log=dA, D=dD)
    if dt == F32:
        got["bias"] = got["dpre"].sum(0)
    return got


def _scan_check(tag, dt, E, h, w, order, B, got):
    ref = _scan_reference(E, h, w, order, B, dt)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    fails = []
    for k, g in got.items():
        yard = max(4 * rel(r32[k], r64[k]), 1e-6)
        g = g.double().cpu().reshape(r64[k].shape)
        if dt == BF16 and k in STORED:
            e = (((g - r64[k]).abs() - 2.0 ** -8 * r64[k].abs()).max() / (r64[k].abs().max() + 1e-300)).item()
            print(f"{tag} {k} bf16: worst |err| - 2^-8|ref| = {e:.3e} of absmax, fp32 allowance {yard:.3e}")
        else:
            e = rel(g, r64[k])
            print(f"{tag} {k}: kernel {e:.3e}  yardstick {yard:.3e} (4x fp32-CPU)")
        if not e <= yard:
            fails.append((k, e, yard))
    assert not fails, fails


@pytest.mark.parametrize("h,w,order", SCAN_CASES)
@pytest.mark.parametrize("E", [16, 80])
def test_scan_order_fp32_matches_fp64_reference(E, h, w, order):
    got = _run_scan(F32, E, h, w, 2, order)
    _scan_check(f"scan {order} {h}x{w} E={E}", F32, E, h, w, order, 2, got)
    again = _run_scan(F32, E, h, w, 2, order)
    for k in got:
        assert torch.equal(got[k], again[k]), k


def test_scan_order_bf16_matches_fp64_reference():
    E, h, w, order = 136, 6, 11, "snake_col"
    got = _run_scan(BF16, E, h, w, 2, order)
    _scan_check(f"scan bf16 {order} {h}x{w} E={E}", BF16, E, h, w, order, 2, got)
    again = _run_scan(BF16, E, h, w, 2, order)
    for k in got:
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize("dt", [F32, BF16])
def test_scan_order_zero_is_the_plain_entry_points_bitwise(dt):
    plain = _run_scan(dt, 80, 6, 11, 2, None)
    ordered = _run_scan(dt, 80, 6, 11, 2, "row")
    for k in plain:
        assert torch.equal(plain[k], ordered[k]), k


@pytest.mark.parametrize("order", ["col_rev", "snake_row"])
def test_scan_order_in_place_equals_gathered_bitwise(order):
    """The _ord kernels on the rows as they lie = the plain kernels on the rows gathered into walking order, outputs
    scattered back: every per-token tensor, dA_log and dD bit for bit."""
    h, w, E = 6, 11, 80
    in_place = _run_scan(F32, E, h, w, 2, order)
    gathered = _run_scan(F32, E, h, w, 2, None, gather=permutation(order, h, w))
    for k in in_place:
        assert torch.equal(in_place[k], gathered[k]), (k, rel(in_place[k], gathered[k]))


def test_scan_order_refuses_bad_orders_and_grids():
    from diffusion_models_collection_amd import _lib as L_
    from diffusion_models_collection_amd import kernels as K
    t = torch.zeros(4, 32, device=DEV)
    for h, w, code, what in ((2, 2, 8, "scan order"), (2, 2, -1, "scan order"), (0, 4, 1, "token grid")):
        with pytest.raises(L_.DMCError, match=what):
            K.selective_scan_fwd_ord(F32, t, 32, t, 32, 0, t, 32, t, 32, 0, 16, t, t, t, 1, h, w, code, 32, 16, None, t,
                                     32)
        with pytest.raises(L_.DMCError, match=what):
            K.causal_conv_silu_fwd_ord(F32, t, 32, t, t, 1, h, w, code, 32, t, 32)


# ---- causal conv -----------------------------------------------------------------------------------------------
def _conv_case(dt, B, h, w, E, order, second_half=False, planted=True):
    """Forward and backward (twice: bitwise equal) of the ordered causal conv over x in columns [0, E) -- or,
    second_half, [E, 2E) -- of [T, 2E] rows whose other half holds 3e6; dx goes to the same columns of rows whose other
    half holds SENT and must keep it; u has pitch E + 8. planted: the first three and the last three physical token
    rows of images 0 and 2 (B = 3) hold 1e6. -> (got, ref64, ref32): u, dx, dw, dbias over all images."""
    from diffusion_models_collection_amd import kernels as K
    L = h * w
    code = ORDERS.index(order)
    # With 1e6 rows a pre-activation whose 1e6-sized terms nearly cancel carries their rounding (an ulp of 0.06) into a
    # small u, which no fp32 evaluation holds to 2e-5 relative: the seeds are ones at which the reference's own fp32
    # evaluation stays within half the bound (asserted below), so the bound tests the kernel and not the draw.
    g = torch.Generator().manual_seed(7 * L + E + B + 1000 * code + 31)
    q = (lambda t: t.bfloat16().float()) if dt == BF16 else (lambda t: t)
    x = torch.randn(B, L, E, generator=g)
    if planted:
        assert B == 3
        x[[0, 2], :3] = 1e6
        x[[0, 2], max(0, L - 3):] = 1e6
    x = q(x)
    wt, b = 0.5 * torch.randn(E, 1, 4, generator=g), 0.1 * torch.randn(E, generator=g)
    du = q(torch.randn(B, L, E, generator=g))
    refs = []
    for D_ in (torch.float64, torch.float32):
        xr, wr, br = (t.to(D_).clone().requires_grad_(True) for t in (x, wt, b))
        ur = causal_conv_silu_ord(xr, wr, br, order, h, w)
        (ur * du.to(D_)).sum().backward()
        refs.append({"u": ur.detach(), "dx": xr.grad, "dw": wr.grad, "dbias": br.grad})
    if planted and dt == F32:
        for k in ("u", "dx"):
            assert ((refs[1][k].double() - refs[0][k]).abs() / (2e-5 + 2e-5 * refs[0][k].abs())).max() <= 0.5, k
    T, col = B * L, E if second_half else 0
    xz = torch.full((T, 2 * E), 3e6, dtype=dt, device=DEV)
    xz[:, col:col + E] = x.reshape(T, E).to(DEV).to(dt)
    wd, bd = wt.to(DEV), b.to(DEV)
    u = torch.full((T, E + 8), SENT, dtype=dt, device=DEV)
    K.causal_conv_silu_fwd_ord(dt, xz, 2 * E, wd, bd, B, h, w, code, E, u, E + 8, x_col=col)
    torch.cuda.synchronize()
    assert bool((u[:, E:] == SENT).all())
    dud = du.reshape(T, E).to(DEV).to(dt).contiguous()
    outs = []
    for _ in range(2):
        dxz = torch.full((T, 2 * E), SENT, dtype=dt, device=DEV)
        dw, db = torch.empty(E, 1, 4, device=DEV), torch.empty(E, device=DEV)
        K.causal_conv_silu_bwd_ord(dt, dud, E, xz, 2 * E, wd, bd, B, h, w, code, E, dxz, 2 * E, dw, db, x_col=col,
                                   dx_col=col)
        outs.append((dxz, dw, db))
    torch.cuda.synchronize()
    assert all(torch.equal(p, q_) for p, q_ in zip(*outs))          # fixed-order reductions
    dxz, dw, db = outs[0]
    assert bool((dxz[:, E - col:2 * E - col] == SENT).all())
    got = {"u": u[:, :E], "dx": dxz[:, col:col + E], "dw": dw, "dbias": db}
    return got, refs[0], refs[1]


def _conv_check_fp32(tag, got, r64):
    for k in got:
        v = got[k].double().cpu().reshape(r64[k].shape)
        if k in ("u", "dx"):
            worst = ((v - r64[k]).abs() / (2e-5 + 2e-5 * r64[k].abs())).max().item()
            print(f"{tag} {k}: worst |err| / (2e-5 + 2e-5 |ref|) = {worst:.3e}")
            torch.testing.assert_close(v, r64[k], rtol=2e-5, atol=2e-5)
        else:
            print(f"{tag} {k}: {rel(v, r64[k]):.3e} of absmax, bound 1e-5")
            assert rel(v, r64[k]) < 1e-5, k


CONV_CASES = [(5, 13, o) for o in ORDERS] + [(h, w, o) for h, w in ((1, 1), (2, 2)) for o in FEW]


@pytest.mark.parametrize("h,w,order", CONV_CASES)
@pytest.mark.parametrize("E", [8, 80])
def test_conv_order_fp32_matches_fp64_reference(E, h, w, order):
    if (h, w, E) == (5, 13, 80):
        from diffusion_models_collection_amd import _lib as L_
        assert L_.LIB.dmc_causal_conv_workspace(3, h * w, E) == 3 * 8 * 5 * E * 4       # 8 segments per image
    got, r64, _ = _conv_case(F32, 3, h, w, E, order)
    _conv_check_fp32(f"conv {order} {h}x{w} E={E}", got, r64)


def test_conv_order_second_half_columns():
    """x_col = dx_col = E: the ordered conv over the second half of [T, 2E] rows; the first half of dx keeps its
    sentinel (_conv_case)."""
    got, r64, _ = _conv_case(F32, 3, 5, 13, 80, "snake_col_rev", second_half=True)
    _conv_check_fp32("conv snake_col_rev 5x13 E=80 second half", got, r64)


def test_conv_order_zero_is_the_plain_entry_points_bitwise():
    from diffusion_models_collection_amd import kernels as K
    B, h, w, E = 3, 5, 13, 80
    L, T = h * w, 3 * h * w
    g = torch.Generator().manual_seed(3)
    for dt in (F32, BF16):
        x, du = (torch.randn(T, E, generator=g).to(DEV).to(dt) for _ in range(2))
        wd, bd = (0.5 * torch.randn(E, 1, 4, generator=g)).to(DEV), (0.1 * torch.randn(E, generator=g)).to(DEV)
        res = []
        for ordered in (False, True):
            u, dx = torch.empty(T, E, dtype=dt, device=DEV), torch.empty(T, E, dtype=dt, device=DEV)
            dw, db = torch.empty(E, 1, 4, device=DEV), torch.empty(E, device=DEV)
            if ordered:
                K.causal_conv_silu_fwd_ord(dt, x, E, wd, bd, B, h, w, 0, E, u, E)
                K.causal_conv_silu_bwd_ord(dt, du, E, x, E, wd, bd, B, h, w, 0, E, dx, E, dw, db)
            else:
                K.causal_conv_silu_fwd(dt, x, E, wd, bd, B, L, E, u, E)
                K.causal_conv_silu_bwd(dt, du, E, x, E, wd, bd, B, L, E, dx, E, dw, db)
            res.append((u, dx, dw, db))
        assert all(torch.equal(p, q) for p, q in zip(*res)), dt


def test_conv_order_bf16():
    """x, du, u and dx in bf16, B = 2, E = 136 without planted rows (the absmax the fp32 allowance scales with would be
    1e6), the criteria of test_causal_conv_bwd_bf16: u and dx within 2^-8 |ref| + the allowance times the absmax, dw and
    dbias (fp32) under the fp32 bound."""
    got, r64, r32 = _conv_case(BF16, 2, 5, 13, 136, "snake_col", planted=False)
    fails = []
    for k in got:
        v = got[k].double().cpu().reshape(r64[k].shape)
        yard = max(4 * rel(r32[k], r64[k]), 1e-6)
        if k in ("u", "dx"):
            e = (((v - r64[k]).abs() - 2.0 ** -8 * r64[k].abs()).max() / r64[k].abs().max()).item()
            print(f"conv bf16 {k}: worst |err| - 2^-8|ref| = {e:.3e} of absmax, fp32 allowance {yard:.3e}")
        else:
            e = rel(v, r64[k])
            print(f"conv bf16 {k} fp32: {e:.3e} of absmax, yardstick {yard:.3e} (4x fp32-CPU)")
        if not e <= yard:
            fails.append((k, e, yard))
    assert not fails, fails
