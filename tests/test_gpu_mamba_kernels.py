"""Numerics of the DiM kernels: the selective scan and the causal conv (csrc/dmc_mamba.hip) against
tests/mamba_reference.py in fp64, and the affine LayerNorm + modulation (csrc/dmc_dit.hip) against the plain kernels
(bitwise at gamma = 1, beta = 0) and torch in fp64.

Scan bound, per tensor (forward and every gradient): the error relative to the tensor's absmax is at most 4x the
error of the same reference evaluated in fp32 on the CPU (a chunked scan reorders the products and the device exp
differs from libm's; nothing else separates the two), floor 1e-6. In bf16 mode (u, z, y, dy, du, dz, ddpre and
dBm | dCm stored in bf16; dpre, Bm, Cm, the states, dA_log and dD fp32) the reference gets the bf16-rounded inputs and a
bf16 tensor must hold, per element, |got - ref| <= 2^-8 |ref| + that fp32 allowance times the absmax (one
round-to-nearest bf16 step, 2^-9, doubled for the fp32 -> bf16 double rounding)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from mamba_reference import causal_conv_silu, selective_scan

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 16


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-300)).item()


def _chunk():
    from diffusion_models_collection_amd import kernels as K
    return K.scan_chunk()


def _scan_inputs(E, L, B=2):
    g = torch.Generator().manual_seed(100 * E + L)
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    u, z = rn(B, L, E), rn(B, L, E)
    # delta pre-activations (with the bias) from -5 to 25: both sides of the softplus threshold 20, and with
    # A down to about -20 decays exp(delta A) that underflow to 0
    dpre = torch.rand(B, L, E, generator=g) * 30 - 5
    Bm, Cm = rn(B, L, N), rn(B, L, N)
    A_log = torch.log(torch.arange(1, N + 1, dtype=torch.float32)).repeat(E, 1) + 0.2 * rn(E, N)
    D = 1 + 0.2 * rn(E)
    bias = 0.3 * rn(E)
    dy = rn(B, L, E)
    return dict(u=u, z=z, dpre=dpre, Bm=Bm, Cm=Cm, A_log=A_log, D=D, bias=bias), dy


NAMES = ("u", "z", "dpre", "Bm", "Cm", "A_log", "D", "bias")


@functools.lru_cache(maxsize=None)
def _scan_reference(E, L):
    """(y64, grads64, err32): the fp64 reference and the relative error of its fp32 evaluation, per tensor."""
    inp, dy = _scan_inputs(E, L)
    res = {}
    for dt in (torch.float64, torch.float32):
        v = {k: t.to(dt).clone().requires_grad_(True) for k, t in inp.items()}
        y = selective_scan(v["u"], v["z"], v["dpre"], v["Bm"], v["Cm"], v["A_log"], v["D"], v["bias"])
        (y * dy.to(dt)).sum().backward()
        res[dt] = (y.detach(), {k: v[k].grad for k in NAMES})
    y64, g64 = res[torch.float64]
    y32, g32 = res[torch.float32]
    err32 = {"y": rel(y32, y64)}
    err32.update({k: rel(g32[k], g64[k]) for k in NAMES})
    return y64, g64, err32


def _run_scan(E, L, backward=True, B=2):
    from diffusion_models_collection_amd import kernels as K
    inp, dy = _scan_inputs(E, L, B)
    f32 = torch.float32
    d = {k: t.to(DEV).contiguous() for k, t in inp.items()}
    T = B * L
    bc = torch.cat([d["Bm"], d["Cm"]], dim=-1).reshape(T, 2 * N).contiguous()
    xz = torch.cat([torch.zeros_like(d["z"]), d["z"]], dim=-1).reshape(T, 2 * E).contiguous()   # z at column E
    y = torch.empty(T, E, device=DEV)
    states = K.scan_states(B, L, E, N, DEV)
    K.selective_scan_fwd(f32, d["u"], E, xz, 2 * E, E, d["dpre"], E, bc, 2 * N, 0, N, d["A_log"], d["D"], d["bias"],
                         B, L, E, N, states, y, E)
    if not backward:
        return y.view(B, L, E), None
    du, ddp = torch.empty(T, E, device=DEV), torch.empty(T, E, device=DEV)
    dxz = torch.zeros(T, 2 * E, device=DEV)
    dbc = torch.full((T, 2 * N + 8), 7.0, device=DEV)       # 8 pad columns behind dBm | dCm: must come back zero
    dA, dD = torch.empty(E, N, device=DEV), torch.empty(E, device=DEV)
    K.selective_scan_bwd(f32, dy.to(DEV).contiguous(), E, d["u"], E, xz, 2 * E, E, d["dpre"], E, bc, 2 * N, 0, N,
                         d["A_log"], d["D"], d["bias"], B, L, E, N, states, du, E, dxz, 2 * E, E, ddp, E, dbc,
                         2 * N + 8, 0, dA, dD)
    assert torch.count_nonzero(dbc[:, 2 * N:]) == 0 and torch.count_nonzero(dxz[:, :E]) == 0
    grads = {"u": du.view(B, L, E), "z": dxz[:, E:].reshape(B, L, E), "dpre": ddp.view(B, L, E),
             "Bm": dbc[:, :N].reshape(B, L, N), "Cm": dbc[:, N:2 * N].reshape(B, L, N), "A_log": dA, "D": dD,
             "bias": ddp.view(T, E).sum(0)}
    return y.view(B, L, E), grads


def _scan_lengths():
    c = 32      # dmc_scan_chunk(); test_scan_chunk_is_what_the_lengths_assume pins it
    return [1, 3, 4, 5, c - 1, c, c + 1, 2 * c + 1, 300]


def test_scan_chunk_is_what_the_lengths_assume():
    assert _chunk() == 32


@pytest.mark.parametrize("L", _scan_lengths())
@pytest.mark.parametrize("E", [16, 80, 136])
def test_selective_scan_matches_fp64_reference(E, L):
    y64, g64, err32 = _scan_reference(E, L)
    y, grads = _run_scan(E, L)
    got = {"y": rel(y, y64)}
    got.update({k: rel(grads[k], g64[k]) for k in NAMES})
    for k, e in got.items():
        print(f"scan E={E} L={L} {k}: kernel {e:.3e}  fp32-CPU {err32[k]:.3e}")
    for k, e in got.items():
        assert e <= max(4 * err32[k], 1e-6), (k, e, err32[k])


def test_selective_scan_is_deterministic():
    for E, L in ((136, 300), (80, 33)):
        y1, g1 = _run_scan(E, L)
        y2, g2 = _run_scan(E, L)
        assert torch.equal(y1, y2)
        for k in g1:
            assert torch.equal(g1[k], g2[k]), k


def test_selective_scan_refuses_other_state_sizes():
    from diffusion_models_collection_amd import _lib as L_
    from diffusion_models_collection_amd import kernels as K
    t = torch.zeros(4, 32, device=DEV)
    with pytest.raises(L_.DMCError, match="16 only"):
        K.selective_scan_fwd(torch.float32, t, 32, t, 32, 0, t, 32, t, 32, 0, 8, t, t, t, 1, 4, 32, 8, None, t, 32)


# ---- the scan in bf16, at other channel counts and batches, in padded layouts, past the capped grid -----------------
BF16 = torch.bfloat16
SENT = 7.5                                     # pitch padding and foreign columns (exact in bf16)
STORED = ("y", "u", "z", "dpre", "Bm", "Cm")   # y and the per-token gradients: in the storage dtype


def _scan_inputs_dt(E, L, B, dt):
    inp, dy = _scan_inputs(E, L, B)
    if dt == BF16:
        inp = dict(inp, u=inp["u"].bfloat16().float(), z=inp["z"].bfloat16().float())
        dy = dy.bfloat16().float()
    return inp, dy


@functools.lru_cache(maxsize=None)
def _scan_reference_ex(E, L, B, dt):
    """{fp64 / fp32: tensors by name ("y" and the gradient of every input)} for the inputs as a kernel of storage dtype
    dt reads them. Channels run in slices of 16384: they are independent but for dBm / dCm, which add up."""
    inp, dy = _scan_inputs_dt(E, L, B, dt)
    per_token, per_channel = ("u", "z", "dpre"), ("A_log", "D", "bias")
    res = {}
    for D_ in (torch.float64, torch.float32):
        parts = {k: [] for k in ("y",) + per_token + per_channel}
        shared = {"Bm": 0, "Cm": 0}
        for e0 in range(0, E, 16384):
            sl = slice(e0, min(E, e0 + 16384))
            v = {k: (t[..., sl] if k in per_token else t[sl] if k in per_channel else t).to(D_).clone().requires_grad_(True)
                 for k, t in inp.items()}
            y = selective_scan(v["u"], v["z"], v["dpre"], v["Bm"], v["Cm"], v["A_log"], v["D"], v["bias"])
            (y * dy[..., sl].to(D_)).sum().backward()
            parts["y"].append(y.detach())
            for k in per_token + per_channel:
                parts[k].append(v[k].grad)
            for k in shared:
                shared[k] = shared[k] + v[k].grad
        r = {k: torch.cat(p, dim=0 if k in per_channel else -1) for k, p in parts.items()}
        r.update(shared)
        res[D_] = r
    return res


def _scan_check(tag, dt, E, L, B, got):
    ref = _scan_reference_ex(E, L, B, dt)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    fails = []
    for k, g in got.items():
        yard = max(4 * rel(r32[k], r64[k]), 1e-6)
        if dt == BF16 and k in STORED:
            err = (g.double().cpu().reshape(r64[k].shape) - r64[k]).abs()
            e = ((err - 2.0 ** -8 * r64[k].abs()).max() / (r64[k].abs().max() + 1e-300)).item()
            print(f"{tag} E={E} L={L} B={B} {k} bf16: worst |err| - 2^-8|ref| = {e:.3e} of absmax, fp32 allowance "
                  f"{yard:.3e}, plain rel {rel(g.reshape(r64[k].shape), r64[k]):.3e}")
        else:
            e = rel(g.reshape(r64[k].shape), r64[k])
            print(f"{tag} E={E} L={L} B={B} {k} fp32: kernel {e:.3e}  yardstick {yard:.3e} (4x fp32-CPU)")
        if not e <= yard:
            fails.append((k, e, yard))
    assert not fails, fails


def _run_scan_ex(dt, E, L, B, padded=False):
    """The scan forward and backward in storage dtype dt -> {"y", gradients by input name} (device tensors).
    tight:  the layout of _run_scan (Bm | Cm rows of pitch 2N, dbc of pitch 2N + 8 at column 0).
    padded: u, dpre, y, dy, du, ddpre in rows of pitch E + 8; Bm | Cm at columns 8 and 8 + N of rows of pitch 2N + 16 and
            dBm | dCm written the same way (bc_col = 8).
    Both: z at column E of [T, 2E] rows and dz written to column E. Everything a kernel does not own holds SENT
    before the call and must hold it afterwards; the dbc padding behind dBm | dCm must come back zero."""
    from diffusion_models_collection_amd import kernels as K
    inp, dy = _scan_inputs_dt(E, L, B, dt)
    f32 = torch.float32
    T = B * L
    pe = E + 8 if padded else E
    pbc, cb = (2 * N + 16, 8) if padded else (2 * N, 0)
    pdbc, cdbc = (2 * N + 16, 8) if padded else (2 * N + 8, 0)

    def rows(v, ld, d, col=0):
        buf = torch.full((T, ld), SENT, dtype=d, device=DEV)
        v = v.reshape(T, -1)
        buf[:, col:col + v.shape[1]] = v.to(DEV).to(d)
        return buf

    def blank(ld, d):
        return torch.full((T, ld), SENT, dtype=d, device=DEV)

    u, dpre, dyb = rows(inp["u"], pe, dt), rows(inp["dpre"], pe, f32), rows(dy, pe, dt)
    xz = rows(inp["z"], 2 * E, dt, col=E)
    bc = rows(torch.cat([inp["Bm"], inp["Cm"]], dim=-1), pbc, f32, col=cb)
    A_log, D, bias = (inp[k].to(DEV).contiguous() for k in ("A_log", "D", "bias"))
    ins = [t.clone() for t in (u, dpre, dyb, xz, bc)]
    y, du, ddp, dxz, dbc = blank(pe, dt), blank(pe, dt), blank(pe, dt), blank(2 * E, dt), blank(pdbc, dt)
    dA, dD = torch.empty(E, N, device=DEV), torch.empty(E, device=DEV)
    states = K.scan_states(B, L, E, N, DEV)
    K.selective_scan_fwd(dt, u, pe, xz, 2 * E, E, dpre, pe, bc, pbc, cb, cb + N, A_log, D, bias, B, L, E, N, states, y,
                         pe)
    K.selective_scan_bwd(dt, dyb, pe, u, pe, xz, 2 * E, E, dpre, pe, bc, pbc, cb, cb + N, A_log, D, bias, B, L, E, N,
                         states, du, pe, dxz, 2 * E, E, ddp, pe, dbc, pdbc, cdbc, dA, dD)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ins, (u, dpre, dyb, xz, bc)))
    for buf in (y, du, ddp):
        assert bool((buf[:, E:] == SENT).all())
    assert bool((dxz[:, :E] == SENT).all()) and bool((dbc[:, :cdbc] == SENT).all())
    assert torch.count_nonzero(dbc[:, cdbc + 2 * N:]) == 0
    got = {"y": y[:, :E], "u": du[:, :E], "z": dxz[:, E:], "dpre": ddp[:, :E], "Bm": dbc[:, cdbc:cdbc + N],
           "Cm": dbc[:, cdbc + N:cdbc + 2 * N], "A_log": dA, "D": dD}
    if dt == f32:
        got["bias"] = ddp[:, :E].sum(0)
    return got


@pytest.mark.parametrize("L", [1, 33, 300])
@pytest.mark.parametrize("E", [16, 136])
def test_selective_scan_bf16_matches_fp64_reference(E, L):
    """bf16 storage: y, du, dz, ddpre and dBm | dCm under the bf16 bound, dA_log and dD under the fp32 bound (module
    docstring); two runs bitwise equal."""
    got = _run_scan_ex(BF16, E, L, 2)
    _scan_check("scan bf16", BF16, E, L, 2, got)
    again = _run_scan_ex(BF16, E, L, 2)
    for k in got:
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("E", [8, 64])
def test_selective_scan_half_group_and_full_backward_block(E, B):
    """fp32, L = 65 (three chunks): E = 8 leaves half of the only 16-channel group invalid, E = 64 fills one backward
    block of four groups exactly; one image and five."""
    _scan_check("scan", torch.float32, E, 65, B, _run_scan_ex(torch.float32, E, 65, B))


@pytest.mark.parametrize("dt", [torch.float32, BF16])
def test_selective_scan_padded_layout(dt):
    """Bm | Cm at columns 8 and 8 + N of rows of pitch 2N + 16, dbc written at bc_col = 8 of the same pitch, z and dz at
    column E of 2E, every other row with pitch E + 8 (_run_scan_ex checks the sentinels): the results meet the bounds
    and are bitwise those of the tight layout. E = 40 is two and a half channel groups, L = 65 three chunks."""
    E, L, B = 40, 65, 2
    got = _run_scan_ex(dt, E, L, B, padded=True)
    _scan_check(f"scan padded {dt}", dt, E, L, B, got)
    tight = _run_scan_ex(dt, E, L, B)
    for k in got:
        assert torch.equal(got[k], tight[k]), k


def test_selective_scan_carry_past_the_capped_grid():
    """B E 16 = 2,097,408 (image, channel, state) carries, past the 2,097,152 threads of scan_carry_kernel's capped grid:
    the last 256 take the grid-stride loop's second trip, forward and reverse. L = 33 is two chunks."""
    E, L, B = 131088, 33, 1
    assert B * E * N > 8192 * 256
    _scan_check("scan carry", torch.float32, E, L, B, _run_scan_ex(torch.float32, E, L, B))


# ---- causal conv ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3, 4, 65])
def test_causal_conv_restarts_at_every_image(L):
    """B = 3 images in the flat [T, E] rows; the last rows of images 0 and 1 hold 1e6, so a read across an image
    boundary cannot hide. Forward and dx elementwise, dw / dbias relative to their absmax, against fp64."""
    from diffusion_models_collection_amd import kernels as K
    B, E = 3, 80
    g = torch.Generator().manual_seed(L)
    x = torch.randn(B, L, E, generator=g)
    x[:-1, max(0, L - 3):] = 1e6
    w = 0.5 * torch.randn(E, 1, 4, generator=g)
    b = 0.1 * torch.randn(E, generator=g)
    du = torch.randn(B, L, E, generator=g)
    xr, wr, br = (t.double().clone().requires_grad_(True) for t in (x, w, b))
    ur = causal_conv_silu(xr, wr, br)
    (ur * du.double()).sum().backward()
    T = B * L
    # x lives in the first E columns of [T, 2E] rows, as in the executor (xz)
    xz = torch.cat([x, torch.full_like(x, 3e6)], dim=-1).reshape(T, 2 * E).to(DEV).contiguous()
    wd, bd = w.to(DEV), b.to(DEV)
    u = torch.empty(T, E, device=DEV)
    K.causal_conv_silu_fwd(torch.float32, xz, 2 * E, wd, bd, B, L, E, u, E)
    torch.testing.assert_close(u.cpu().double().view(B, L, E), ur.detach(), rtol=2e-5, atol=2e-5)
    dxz = torch.zeros(T, 2 * E, device=DEV)
    dw, db = torch.empty(E, 1, 4, device=DEV), torch.empty(E, device=DEV)
    outs = []
    for _ in range(2):
        K.causal_conv_silu_bwd(torch.float32, du.reshape(T, E).to(DEV).contiguous(), E, xz, 2 * E, wd, bd, B, L, E,
                               dxz, 2 * E, dw, db)
        outs.append((dxz.clone(), dw.clone(), db.clone()))
    assert all(torch.equal(p, q) for p, q in zip(*outs))           # fixed-order reductions
    assert torch.count_nonzero(dxz[:, E:]) == 0
    torch.testing.assert_close(dxz[:, :E].cpu().double().view(B, L, E), xr.grad, rtol=2e-5, atol=2e-5)
    print(f"conv L={L}: dw {rel(dw, wr.grad):.3e} dbias {rel(db, br.grad):.3e}")
    assert rel(dw, wr.grad) < 1e-5 and rel(db, br.grad) < 1e-5


def test_causal_conv_bf16():
    from diffusion_models_collection_amd import kernels as K
    B, L, E = 2, 37, 136
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B * L, E, generator=g).to(DEV).bfloat16()
    w, b = 0.5 * torch.randn(E, 1, 4, generator=g), 0.1 * torch.randn(E, generator=g)
    u = torch.empty(B * L, E, device=DEV, dtype=torch.bfloat16)
    K.causal_conv_silu_fwd(torch.bfloat16, x, E, w.to(DEV), b.to(DEV), B, L, E, u, E)
    ur = causal_conv_silu(x.cpu().double().view(B, L, E), w.double(), b.double())
    assert rel(u.view(B, L, E), ur) < 1e-2


def _conv_splits(B, L, E):
    return max(1, min(-(-2048 // (B * -(-E // 64))), L // 8, 256))


def _conv_case(dt, B, L, E, second_half=False, backward=True, planted=True):
    """Forward (and backward, twice: bitwise equal) of the causal conv over x in columns [0, E) -- or, second_half,
    [E, 2E) -- of [T, 2E] rows whose other half holds 3e6; dx goes to the same columns of rows whose other half holds
    SENT and must keep it; u has pitch E + 8. planted: the last rows of every image but the last hold 1e6.
    -> (got, ref64, ref32): u, dx, dw, dbias."""
    from diffusion_models_collection_amd import kernels as K
    g = torch.Generator().manual_seed(7 * L + E + B)
    q = (lambda t: t.bfloat16().float()) if dt == BF16 else (lambda t: t)
    x = torch.randn(B, L, E, generator=g)
    if planted:
        assert B > 1
        x[:-1, max(0, L - 3):] = 1e6
    x = q(x)
    w, b = 0.5 * torch.randn(E, 1, 4, generator=g), 0.1 * torch.randn(E, generator=g)
    du = q(torch.randn(B, L, E, generator=g))
    refs = []
    for D_ in (torch.float64, torch.float32):
        xr, wr, br = (t.to(D_).clone().requires_grad_(True) for t in (x, w, b))
        ur = causal_conv_silu(xr, wr, br)
        r = {"u": ur.detach()}
        if backward:
            (ur * du.to(D_)).sum().backward()
            r.update(dx=xr.grad, dw=wr.grad, dbias=br.grad)
        refs.append(r)
    T, col = B * L, E if second_half else 0
    xz = torch.full((T, 2 * E), 3e6, dtype=dt, device=DEV)
    xz[:, col:col + E] = x.reshape(T, E).to(DEV).to(dt)
    wd, bd = w.to(DEV), b.to(DEV)
    u = torch.full((T, E + 8), SENT, dtype=dt, device=DEV)
    K.causal_conv_silu_fwd(dt, xz, 2 * E, wd, bd, B, L, E, u, E + 8, x_col=col)
    torch.cuda.synchronize()
    assert bool((u[:, E:] == SENT).all())
    got = {"u": u[:, :E]}
    if backward:
        dud = du.reshape(T, E).to(DEV).to(dt).contiguous()
        outs = []
        for _ in range(2):
            dxz = torch.full((T, 2 * E), SENT, dtype=dt, device=DEV)
            dw, db = torch.empty(E, 1, 4, device=DEV), torch.empty(E, device=DEV)
            K.causal_conv_silu_bwd(dt, dud, E, xz, 2 * E, wd, bd, B, L, E, dxz, 2 * E, dw, db, x_col=col, dx_col=col)
            outs.append((dxz, dw, db))
        torch.cuda.synchronize()
        assert all(torch.equal(p, q_) for p, q_ in zip(*outs))          # fixed-order reductions
        dxz, dw, db = outs[0]
        assert bool((dxz[:, E - col:2 * E - col] == SENT).all())
        got.update(dx=dxz[:, col:col + E], dw=dw, dbias=db)
    return got, refs[0], refs[1]


def _conv_check_fp32(tag, got, r64):
    """The bounds of test_causal_conv_restarts_at_every_image: u and dx per element, dw and dbias against their absmax."""
    for k in got:
        v = got[k].double().cpu().reshape(r64[k].shape)
        if k in ("u", "dx"):
            worst = ((v - r64[k]).abs() / (2e-5 + 2e-5 * r64[k].abs())).max().item()
            print(f"{tag} {k}: worst |err| / (2e-5 + 2e-5 |ref|) = {worst:.3e}")
            torch.testing.assert_close(v, r64[k], rtol=2e-5, atol=2e-5)
        else:
            print(f"{tag} {k}: {rel(v, r64[k]):.3e} of absmax, bound 1e-5")
            assert rel(v, r64[k]) < 1e-5, k


@pytest.mark.parametrize("B,L,E,second_half", [(3, 5, 80, True), (3, 65, 80, True), (3, 5, 8, False), (3, 65, 8, True)])
def test_causal_conv_second_half_columns_and_eight_channels(B, L, E, second_half):
    """x_col = dx_col = E: the conv over the second half of [T, 2E] rows (the first half of dx keeps its sentinel), and
    E = 8 (an eighth of the backward's 64-lane block), with the planted 1e6 rows."""
    got, r64, _ = _conv_case(torch.float32, B, L, E, second_half)
    _conv_check_fp32(f"conv B={B} L={L} E={E} second_half={second_half}", got, r64)


@pytest.mark.parametrize("B,L,E,S", [(2100, 9, 8, 1), (1, 2100, 8, 256)])
def test_causal_conv_split_plan_edges(B, L, E, S):
    """conv_splits: one segment per image because B ceil(E / 64) > 2048 already fills the chip, and the 256 cap
    (2100 tokens in segments of 8.2). The workspace size B S 5 E 4 pins the plan."""
    from diffusion_models_collection_amd import _lib as L_
    assert _conv_splits(B, L, E) == S
    assert L_.LIB.dmc_causal_conv_workspace(B, L, E) == B * S * 5 * E * 4
    got, r64, _ = _conv_case(torch.float32, B, L, E, planted=B > 1)
    _conv_check_fp32(f"conv B={B} L={L} E={E} S={S}", got, r64)


def test_causal_conv_forward_past_the_capped_grid():
    """B L E = 2,164,800 outputs, past the 2,097,152 threads of the capped grid: the grid-stride loop's second trip."""
    B, L, E = 2, 4100, 264
    assert B * L * E > 8192 * 256
    got, r64, _ = _conv_case(torch.float32, B, L, E, backward=False)
    _conv_check_fp32(f"conv fwd B={B} L={L} E={E}", got, r64)


def test_causal_conv_bwd_bf16():
    """x, du, u and dx in bf16: u and dx under the bf16 bound, dw and dbias (fp32) under the fp32 bound (module
    docstring), two runs bitwise equal (_conv_case). B = 2, L = 37, E = 136 without planted rows -- the absmax the fp32
    allowance scales with would be 1e6 -- and B = 3, L = 5 with them, u and dx then per element within
    2^-8 |ref| + 2e-5 (1 + |ref|), the fp32 test's elementwise bound in place of the absmax allowance."""
    got, r64, r32 = _conv_case(BF16, 2, 37, 136, planted=False)
    fails = []
    for k in got:
        v = got[k].double().cpu().reshape(r64[k].shape)
        yard = max(4 * rel(r32[k], r64[k]), 1e-6)
        if k in ("u", "dx"):
            e = (((v - r64[k]).abs() - 2.0 ** -8 * r64[k].abs()).max() / r64[k].abs().max()).item()
            print(f"conv bf16 {k}: worst |err| - 2^-8|ref| = {e:.3e} of absmax, fp32 allowance {yard:.3e}, plain rel "
                  f"{rel(v, r64[k]):.3e}")
        else:
            e = rel(v, r64[k])
            print(f"conv bf16 {k} fp32: {e:.3e} of absmax, yardstick {yard:.3e} (4x fp32-CPU)")
        if not e <= yard:
            fails.append((k, e, yard))
    assert not fails, fails
    got, r64, r32 = _conv_case(BF16, 3, 5, 80, second_half=True)
    for k in ("u", "dx"):
        v = got[k].double().cpu().reshape(r64[k].shape)
        worst = ((v - r64[k]).abs() / (2.0 ** -8 * r64[k].abs() + 2e-5 * (1 + r64[k].abs()))).max().item()
        print(f"conv bf16 planted {k}: worst |err| / (2^-8 |ref| + 2e-5 (1 + |ref|)) = {worst:.3e}")
        assert worst <= 1.0, k
    for k in ("dw", "dbias"):
        yard = max(4 * rel(r32[k], r64[k]), 1e-6)
        print(f"conv bf16 planted {k} fp32: {rel(got[k], r64[k].reshape(got[k].shape)):.3e}, yardstick {yard:.3e}")
        assert rel(got[k], r64[k].reshape(got[k].shape)) <= yard, k


# ---- affine LayerNorm + modulation -----------------------------------------------------------------------------
def _ln_case(C, dt, gen, B=3, L=48):
    T = B * L
    x = torch.randn(T, C, generator=gen).to(DEV)
    br = torch.randn(T, C, generator=gen).to(DEV).to(dt)
    mod = (torch.randn(B, 3 * C + 8, generator=gen) * 0.5).to(DEV)
    dh = torch.randn(T, C, generator=gen).to(DEV).to(dt)
    return B, L, T, x, br, mod, dh


def _ln_affine(K, dt, C, B, L, T, x, br, mod, dh, gamma, beta):
    ld = mod.shape[1]
    h = torch.empty(T, C, dtype=dt, device=DEV)
    mean, rstd, xo = torch.empty(T, device=DEV), torch.empty(T, device=DEV), torch.empty(T, C, device=DEV)
    K.ln_affine_mod_fwd(dt, x, T, C, L, mod, ld, 0, C, 1e-6, gamma, beta, h, C, mean, rstd, br=br, ld_br=C,
                        off_gate=2 * C, x_out=xo)
    dx = torch.zeros(T, C, device=DEV)
    dmod = torch.zeros_like(mod)
    dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    K.ln_affine_mod_bwd(dt, dh, C, xo, mean, rstd, mod, ld, C, T, C, L, gamma, beta, dx, dmod, C, 0, dg, db)
    return h, xo, mean, rstd, dx, dmod, dg, db


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [40, 64, 384, 768])
def test_ln_affine_identity_equals_plain_kernels_bitwise(dt, C):
    from diffusion_models_collection_amd import kernels as K
    gen = torch.Generator().manual_seed(C)
    B, L, T, x, br, mod, dh = _ln_case(C, dt, gen)
    ld = mod.shape[1]
    h, xo, mean, rstd, dx, dmod, dg, db = _ln_affine(K, dt, C, B, L, T, x, br, mod, dh, torch.ones(C, device=DEV),
                                                     torch.zeros(C, device=DEV))
    h0 = torch.empty(T, C, dtype=dt, device=DEV)
    mean0, rstd0, xo0 = torch.empty(T, device=DEV), torch.empty(T, device=DEV), torch.empty(T, C, device=DEV)
    K.ln_mod_fwd(dt, x, T, C, L, mod, ld, 0, C, 1e-6, h0, C, mean0, rstd0, br=br, ld_br=C, off_gate=2 * C, x_out=xo0)
    dx0 = torch.zeros(T, C, device=DEV)
    dmod0 = torch.zeros_like(mod)
    K.ln_mod_bwd(dt, dh, C, xo0, mean0, rstd0, mod, ld, C, T, C, L, dx0, dmod0, C, 0)
    for a, b in ((h, h0), (xo, xo0), (mean, mean0), (rstd, rstd0), (dx, dx0), (dmod, dmod0)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [40, 64, 384, 768])
def test_ln_affine_matches_torch_fp64(dt, C):
    from diffusion_models_collection_amd import kernels as K
    gen = torch.Generator().manual_seed(C + 1)
    B, L, T, x, br, mod, dh = _ln_case(C, dt, gen)
    gamma = (1 + 0.3 * torch.randn(C, generator=gen)).to(DEV)
    beta = (0.3 * torch.randn(C, generator=gen)).to(DEV)
    runs = [_ln_affine(K, dt, C, B, L, T, x, br, mod, dh, gamma, beta) for _ in range(2)]
    assert all(torch.equal(p, q) for p, q in zip(*runs))          # dgamma / dbeta: fixed-order sums
    h, xo, mean, rstd, dx, dmod, dg, db = runs[0]
    xr, brr, modr, gr, btr = (t.detach().double().cpu().clone().requires_grad_(True) for t in (x, br, mod, gamma, beta))
    sh, sc = modr[:, :C].repeat_interleave(L, 0), modr[:, C:2 * C].repeat_interleave(L, 0)
    xn = xr + modr[:, 2 * C:3 * C].repeat_interleave(L, 0) * brr
    xn.retain_grad()
    hr = F.layer_norm(xn, (C,), gr, btr, eps=1e-6) * (1 + sc) + sh
    (hr * dh.double().cpu()).sum().backward()
    lim_f, lim_b = (1e-5, 1e-4) if dt == torch.float32 else (1e-2, 2e-2)
    figs = {"h": rel(h, hr), "x_out": rel(xo, xn), "dx": rel(dx, xn.grad), "dshift": rel(dmod[:, :C], modr.grad[:, :C]),
            "dscale": rel(dmod[:, C:2 * C], modr.grad[:, C:2 * C]), "dgamma": rel(dg, gr.grad),
            "dbeta": rel(db, btr.grad)}
    print(f"ln_affine {dt} C={C}:", {k: f"{v:.2e}" for k, v in figs.items()})
    assert figs["h"] < lim_f and figs["x_out"] < 1e-6
    for k in ("dx", "dshift", "dscale", "dgamma", "dbeta"):
        assert figs[k] < lim_b, (k, figs[k])


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,drop", [(40, False), (768, True)])
def test_gate_bwd_bias(dt, C, drop):
    """dmc_gate_bwd_bias: dbr and dgate bitwise those of dmc_gate_bwd (dropout mask included); dbias = the fp32 sum of
    dy * gate * mask over all rows (against fp64, with the mask read back from dbr), two runs bitwise equal."""
    from diffusion_models_collection_amd import kernels as K
    gen = torch.Generator().manual_seed(C)
    B, L, T, x, br, mod, dh = _ln_case(C, dt, gen)
    ld = mod.shape[1]
    dy = x                                     # any fp32 rows
    d = (1234, min(int(round(0.25 * 4294967296.0)), 4294967295), 1.0 / 0.75) if drop else None
    dbr0 = torch.empty(T, C, dtype=dt, device=DEV)
    dmod0 = torch.zeros_like(mod)
    K.gate_bwd(dt, dy, br, C, mod, ld, 2 * C, T, C, L, dbr0, C, dmod0, 2 * C, drop=d)
    outs = []
    for _ in range(2):
        dbr = torch.empty(T, C, dtype=dt, device=DEV)
        dmod = torch.zeros_like(mod)
        db = torch.empty(C, device=DEV)
        K.gate_bwd_bias(dt, dy, br, C, mod, ld, 2 * C, T, C, L, dbr, C, dmod, 2 * C, db, drop=d)
        outs.append((dbr, dmod, db))
    assert all(torch.equal(p, q) for p, q in zip(*outs))
    dbr, dmod, db = outs[0]
    assert torch.equal(dbr, dbr0) and torch.equal(dmod, dmod0)
    gate = mod[:, 2 * C:3 * C].double().repeat_interleave(L, 0)
    mask = (dbr0 != 0).double() * (1.0 / 0.75 if drop else 1.0)      # dy and gate are nonzero almost surely
    ref = (dy.double() * gate * mask).sum(0)
    print(f"gate_bwd_bias {dt} C={C} drop={drop}: {rel(db, ref):.2e}")
    assert rel(db, ref) < 1e-5
