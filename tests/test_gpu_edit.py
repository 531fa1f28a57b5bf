"""img2img, inpaint and DDIM inversion on the GPU: dmc_known_blend bit for bit against an fp32 op-by-op restatement
(criterion 1 of test_gpu_elem_kernels: the kernel has no libm call and no fma), the entry points' semantics with an
elementwise denoiser, the loops against the float64 numpy loops of tests/edit_reference.py (criterion 2), against the
kernels composed by hand (bitwise), and graph replay against the eager loop.

Every input builder and reference runs on the CPU alone: cpu_selfcheck() calls them all without a GPU
(tests/test_edit_host.py runs it).
"""
import functools

import numpy as np
import pytest
import torch

import dpm_reference as R
import edit_reference as E
from test_gpu_dpm import GaussianDenoiser
from test_gpu_elem_kernels import DEV, F32, F64, NAN, dev, guard_ok, guarded, judge, rng, same_bits, tables

pytestmark = pytest.mark.gpu


def _lib():
    from diffusion_models_collection_amd import _lib as L, kernels as K
    return L, K


# ------------------------------------------------------------------------------------------------------------
# the blend kernel
# ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blend_table():
    """[100, 4] fp32 table of DDIM-50 on the linear T = 1000 schedule, from the float64 restatement rounded once
    (never modified). Even rows: rb = 0; rows 98, 99: kb = 0."""
    from diffusion_models_collection_amd.diffusion import _schedule
    ac = tables()["alphas_cumprod"].numpy()
    c = torch.from_numpy(E.ref_blend_coefficients(ac, _schedule.ddim_timesteps(1000, 50)).astype(np.float32))
    assert bool((c[:98, 1] != 0).all()) and bool((c[98:, 1] == 0).all())
    assert bool((c[0::2, 3] == 0).all()) and bool((c[1::2, 3] != 0).all())
    return c


ROWS = (10, 11, 98, 99, 51, 0, 97)     # the four kinds (kb = 0 or not) x (rb = 0 or not), then more of the common two


def blend_ref(dt, coef, row, x, x0, m, z, z2):
    """known_blend_kernel's ops one at a time in precision dt. z / z2 are not part of a row's result where its
    kb / rb is 0, whatever they hold."""
    N = x.shape[0]
    ka, kb, ra, rb = (coef.to(dt)[row][:, k].view((N,) + (1,) * (x.dim() - 1)) for k in range(4))
    known = ka * x0.to(dt)
    if z is not None:
        known = torch.where(kb != 0, known + kb * z.to(dt), known)
    else:
        assert bool((kb == 0).all())
    mm = m.to(dt)
    b = mm * known + (1 - mm) * x.to(dt)
    if z2 is not None:
        b = torch.where(rb != 0, ra * b + rb * z2.to(dt), b)
    else:
        assert bool((rb == 0).all())
    return b


def blend_shapes(N, per, mask_per):
    """(operand shape, mask shape): a full mask for mask_per == per, else one mask channel shared by per / mask_per."""
    if mask_per == per:
        return (N, per), (N, per)
    return (N, per // mask_per, mask_per), (N, 1, mask_per)


@functools.lru_cache(maxsize=None)
def blend_inputs(N, per, mask_per, soft, rot=0):
    g = rng(4100 + N + per + mask_per + soft)
    xs, ms = blend_shapes(N, per, mask_per)
    row = torch.tensor([ROWS[(n + rot) % len(ROWS)] for n in range(N)])
    x, x0, z, z2 = (torch.randn(xs, generator=g) for _ in range(4))
    m = torch.rand(ms, generator=g)
    if not soft:
        m = (m < 0.5).float()
    return x, x0, m, z, z2, row


BLEND_SHAPES = [(1, 1, 1), (5, 7, 7), (3, 3072, 1024), (3, 3072, 3072), (300, 48, 16), (6, 12, 3)]


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("N,per,mask_per", BLEND_SHAPES)
def test_known_blend(N, per, mask_per, soft):
    """(5, 7, 7): per % 4 != 0, the scalar path with misaligned rows; (3, 3072, ·) and (300, 48, 16): the 16-byte
    path with a shared and a full mask, the last with more samples than a block has threads; (6, 12, 3): per % 4 == 0
    but a mask pitch that forces the scalar path; (1, 1, 1) is run once per row kind. Written over NaN with guards
    intact, then with out aliasing x."""
    L, K = _lib()
    coef = blend_table()
    cd = dev(coef)
    for rot in range(4 if N < 4 else 1):
        x, x0, m, z, z2, row = blend_inputs(N, per, mask_per, soft, rot)
        if N >= 4:
            assert set(row.tolist()) >= {10, 11, 98, 99}
        ref = blend_ref(F32, coef, row, x, x0, m, z, z2)
        assert bool(ref.isfinite().all())
        out, buf = guarded(x.shape)
        r = K.known_blend(dev(x), dev(x0), dev(m), dev(row), cd, z=dev(z), z2=dev(z2), out=out)
        assert r is out
        what = f"known_blend rot={rot} soft={soft}"
        same_bits(what, out, ref)
        guard_ok(what, buf)
        xio, xbuf = guarded(x.shape)
        xio.copy_(x)
        K.known_blend(xio, dev(x0), dev(m), dev(row), cd, z=dev(z), z2=dev(z2), out=xio)
        same_bits(what + " in place", xio, ref)
        guard_ok(what + " in place", xbuf)
    # the restatement itself: the float64 version agrees to rounding
    x, x0, m, z, z2, row = blend_inputs(N, per, mask_per, soft, 0)
    r32, r64 = (blend_ref(dt, coef, row, x, x0, m, z, z2) for dt in (F32, F64))
    assert float((r32.double() - r64).abs().max()) < 1e-5


def poisoned(coef, row, z, z2):
    """z with NaN in every sample whose row has kb == 0, z2 with NaN where rb == 0."""
    pz, pz2 = z.clone(), z2.clone()
    no_z, no_z2 = coef[row][:, 1] == 0, coef[row][:, 3] == 0
    assert 0 < int(no_z.sum()) < len(row) and 0 < int(no_z2.sum()) < len(row)
    pz[no_z] = NAN
    pz2[no_z2] = NAN
    return pz, pz2


@pytest.mark.parametrize("N,per,mask_per", [(5, 7, 7), (300, 48, 16)])
def test_known_blend_never_reads_unused_noise(N, per, mask_per):
    """NaN in z / z2 for every sample whose row does not use them: finite outputs with the right bits. Then neither
    buffer at all: no z2 with even rows only, and no z with the last step's row."""
    L, K = _lib()
    coef = blend_table()
    x, x0, m, z, z2, row = blend_inputs(N, per, mask_per, True)
    pz, pz2 = poisoned(coef, row, z, z2)
    ref = blend_ref(F32, coef, row, x, x0, m, z, z2)
    out, buf = guarded(x.shape)
    K.known_blend(dev(x), dev(x0), dev(m), dev(row), dev(coef), z=dev(pz), z2=dev(pz2), out=out)
    assert bool(out.isfinite().all())
    same_bits("poisoned noise", out, ref)
    guard_ok("poisoned noise", buf)

    even = torch.tensor([2 * (n % 50) for n in range(N)])
    ref = blend_ref(F32, coef, even, x, x0, m, z, None)
    out, buf = guarded(x.shape)
    K.known_blend(dev(x), dev(x0), dev(m), dev(even), dev(coef), z=dev(z), z2=None, out=out)
    same_bits("no z2 buffer", out, ref)
    plain = coef[98:99].contiguous()                        # a table whose only row has kb == 0 and rb == 0
    first = torch.zeros(N, dtype=torch.long)
    ref = blend_ref(F32, plain, first, x, x0, m, None, None)
    out2, buf2 = guarded(x.shape)
    K.known_blend(dev(x), dev(x0), dev(m), dev(first), dev(plain), out=out2)
    same_bits("no noise buffers", out2, ref)
    guard_ok("no noise buffers", buf, buf2)


@pytest.mark.parametrize("which", ["x", "x0", "mask", "z", "z2", "out"])
def test_known_blend_misaligned_base(which):
    """per % 4 == 0 but one operand starts 4 bytes into its buffer: the element-wise path, the same bits."""
    L, K = _lib()
    N, per = 3, 64
    coef = blend_table()
    x, x0, m, z, z2, row = blend_inputs(N, per, per, True)
    ref = blend_ref(F32, coef, row, x, x0, m, z, z2)
    ops = {"x": dev(x), "x0": dev(x0), "mask": dev(m), "z": dev(z), "z2": dev(z2)}
    ops["out"], ob = guarded((N, per))
    shifted, sbuf = guarded((N * per + 1,))
    view = shifted[1:].view(N, per)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    if which != "out":
        view.copy_(ops[which])
    ops[which] = view
    K.known_blend(ops["x"], ops["x0"], ops["mask"], dev(row), dev(coef), z=ops["z"], z2=ops["z2"], out=ops["out"])
    same_bits(f"misaligned {which}", ops["out"], ref)
    guard_ok(f"misaligned {which}", ob, sbuf)
    assert bool(shifted[:1].isnan().all())                  # the element before the view is untouched


def test_known_blend_refusals():
    """A wrong operand is a DMCError before anything is launched: the NaN-filled output stays untouched."""
    L, K = _lib()
    N, per, mp = 3, 8, 4
    coef = dev(blend_table())
    x, x0, m, z, z2, row = (dev(v) for v in blend_inputs(N, per, mp, True))
    out, buf = guarded(x.shape)
    ok = dict(z=z, z2=z2, out=out)
    bad = [
        ("x0 shape", lambda: K.known_blend(x, x0[:, :1].contiguous(), m, row, coef, **ok)),
        ("z shape", lambda: K.known_blend(x, x0, m, row, coef, **{**ok, "z": z[:2].contiguous()})),
        ("z2 on the CPU", lambda: K.known_blend(x, x0, m, row, coef, **{**ok, "z2": z2.cpu()})),
        ("x0 float64", lambda: K.known_blend(x, x0.double(), m, row, coef, **ok)),
        ("x strided", lambda: K.known_blend(torch.zeros(N, per // mp, 2 * mp, device=DEV)[:, :, ::2], x0, m, row, coef,
                                            **ok)),
        ("mask strided", lambda: K.known_blend(x, x0, torch.zeros(N, 1, 2 * mp, device=DEV)[:, :, ::2], row, coef,
                                               **ok)),
        ("mask shape", lambda: K.known_blend(x, x0, m[:, :, :2].contiguous(), row, coef, **ok)),
        ("mask batch", lambda: K.known_blend(x, x0, m[:2].contiguous(), row, coef, **ok)),
        ("mask on the CPU", lambda: K.known_blend(x, x0, m.cpu(), row, coef, **ok)),
        ("mask float64", lambda: K.known_blend(x, x0, m.double(), row, coef, **ok)),
        ("row on the CPU", lambda: K.known_blend(x, x0, m, row.cpu(), coef, **ok)),
        ("row int32", lambda: K.known_blend(x, x0, m, row.int(), coef, **ok)),
        ("row length", lambda: K.known_blend(x, x0, m, row[:2].contiguous(), coef, **ok)),
        ("no row", lambda: K.known_blend(x, x0, m, None, coef, **ok)),
        ("coef [R, 5]", lambda: K.known_blend(x, x0, m, row, torch.zeros(4, 5, device=DEV), **ok)),
        ("coef flat", lambda: K.known_blend(x, x0, m, row, coef.flatten(), **ok)),
        ("coef strided", lambda: K.known_blend(x, x0, m, row, coef[::2], **ok)),
        ("coef float64", lambda: K.known_blend(x, x0, m, row, coef.double(), **ok)),
        ("coef on the CPU", lambda: K.known_blend(x, x0, m, row, coef.cpu(), **ok)),
    ]
    for what, call in bad:
        with pytest.raises(L.DMCError):
            call()
        torch.cuda.synchronize()
        assert bool(out.isnan().all()), what
    # the C entry point refuses empty extents, a mask pitch that does not divide, and a missing operand itself
    p = dict(x=x.data_ptr(), x0=x0.data_ptr(), mask=m.data_ptr(), row=row.data_ptr(), coef=coef.data_ptr(),
             out=out.data_ptr())

    def entry(R=100, n=N, per_=per, mp_=mp, **null):
        q = {**p, **null}
        return L.LIB.dmc_known_blend(q["x"], q["x0"], q["mask"], mp_, z.data_ptr(), z2.data_ptr(), q["row"], q["coef"],
                                     R, n, per_, q["out"], L.stream())

    assert entry(R=0) != 0 and b"known_blend" in L.LIB.dmc_last_error()
    for kw in (dict(n=0), dict(per_=0), dict(mp_=0), dict(mp_=-4), dict(mp_=3), dict(per_=-8),
               dict(x=None), dict(x0=None), dict(mask=None), dict(row=None), dict(coef=None), dict(out=None)):
        assert entry(**kw) != 0, kw
    torch.cuda.synchronize()
    assert bool(out.isnan().all())
    guard_ok("refusals", buf)


# ------------------------------------------------------------------------------------------------------------
# injected draws
# ------------------------------------------------------------------------------------------------------------
WHICH = ("start", "step", "known", "renoise")


class Draws:
    """noise=(j, which) for img2img / inpaint from fixed seeds: the same tensor for the device loop (__call__, which
    also logs what was asked for) and the numpy references (np)."""

    def __init__(self, shape, seed):
        self.shape, self.seed, self.asked = tuple(shape), seed, []

    def cpu(self, j, which):
        return torch.randn(self.shape, generator=rng(self.seed * 100003 + 4 * j + WHICH.index(which)))

    def np(self, j, which):
        return self.cpu(j, which).numpy()

    def __call__(self, j, which):
        self.asked.append((j, which))
        return dev(self.cpu(j, which))


# ------------------------------------------------------------------------------------------------------------
# semantics with the elementwise Gaussian denoiser
# ------------------------------------------------------------------------------------------------------------
SHAPE = (4, 3, 8, 8)


@functools.lru_cache(maxsize=None)
def gauss_inputs():
    """(x_T, image in [-1, 1], random binary [B, 1, H, W] mask, soft [B, C, H, W] mask); never modified."""
    g = rng(78)
    xT = torch.randn(SHAPE, generator=g)
    image = torch.rand(SHAPE, generator=g) * 2 - 1
    binary = (torch.rand((SHAPE[0], 1) + SHAPE[2:], generator=g) < 0.5).float()
    soft = torch.rand(SHAPE, generator=g)
    assert 0 < float(binary.mean()) < 1
    return xT, image, binary, soft


def make_sampler(kind, device):
    from diffusion_models_collection_amd.diffusion import DDIM, DDPM, DPMSolver
    if kind == "ddim":
        return DDIM(1000, 50, device=device)
    if kind == "ddpm":
        return DDPM(num_timesteps=12, device=device)
    return DPMSolver(1000, 20, device=device)


@pytest.mark.parametrize("kind", ["ddim", "ddpm", "dpm"])
def test_inpaint_semantics(kind):
    """resample = 1 and a denoiser that acts on each element alone: the unknown pixels are bitwise sample()'s from
    the same x_T (and step noise), the known pixels bitwise the image; an all-zero mask gives sample(), an all-one
    mask the image."""
    smp = make_sampler(kind, DEV)
    model = GaussianDenoiser(1.0)
    xT, image, binary, _ = gauss_inputs()
    draws = Draws(SHAPE, 5)
    if kind == "ddpm":
        plain = smp.sample(model, SHAPE, x_T=dev(xT), noise=lambda i: draws(i, "step"))
    else:
        plain = smp.sample(model, SHAPE, x_T=dev(xT))
    plain = plain.cpu()
    assert bool(plain.isfinite().all())
    keep = binary.expand(SHAPE) == 1
    got = smp.inpaint(model, dev(image), dev(binary), x_T=dev(xT), noise=draws).cpu()
    assert got.shape == SHAPE and got.dtype == F32
    assert torch.equal(got[keep], image[keep]) and torch.equal(got[~keep], plain[~keep])
    assert not torch.equal(got, plain) and not torch.equal(got, image)
    zeros = smp.inpaint(model, dev(image), torch.zeros(1, 1, 1, 1), x_T=dev(xT), noise=draws).cpu()
    assert torch.equal(zeros, plain)
    ones = smp.inpaint(model, dev(image), torch.ones(SHAPE), x_T=dev(xT), noise=draws).cpu()
    assert torch.equal(ones, image)


def test_draw_order():
    """Per walk entry: the step's z (DDPM draws one), the known region's z (not on the last step: kb = 0), the
    re-noise z2 (not on a step's last repetition); 'start' first when no x_T is given."""
    smp = make_sampler("ddpm", DEV)
    _, image, binary, _ = gauss_inputs()
    draws = Draws(SHAPE, 6)
    smp.inpaint(GaussianDenoiser(1.0), dev(image), dev(binary), resample=2, noise=draws)
    want = [(0, "start")]
    for j, (i, renoise) in enumerate(E.ref_walk(12, 0, 2)):
        want += [(j, "step")] + ([(j, "known")] if i < 11 else []) + ([(j, "renoise")] if renoise else [])
    assert draws.asked == want


# ------------------------------------------------------------------------------------------------------------
# the loops against the float64 numpy loops (criterion 2)
# ------------------------------------------------------------------------------------------------------------
LOOP_CASES = ("ddim_inpaint", "ddpm_inpaint", "ddim_img2img")


def loop_case(name):
    """-> (call(sampler on the device, model) -> device result, ref32, ref64): the sampler's own fp32 tables (built on
    the CPU: the same host arithmetic as on the device) through the numpy loops with the same injected draws."""
    from diffusion_models_collection_amd.diffusion import _schedule
    kind = name.split("_")[0]
    cpu = make_sampler(kind, "cpu")
    ac1000 = tables()["alphas_cumprod"].numpy()
    xT, image, binary, soft = gauss_inputs()
    draws = Draws(SHAPE, 7 + LOOP_CASES.index(name))
    if kind == "ddim":
        ts = cpu.inference_timesteps.numpy()
        tabs = {k: getattr(cpu, k).numpy() for k in ("alphas_cumprod", "sqrt_alphas_cumprod",
                                                     "sqrt_one_minus_alphas_cumprod")}
    else:
        ts = np.arange(11, -1, -1)
        tabs = _schedule.build_tables(12, 1e-4, 0.02, "linear")
        assert all(np.array_equal(tabs[k], getattr(cpu, k).numpy()) for k in E.DDPM_TABS)
    # GaussianDenoiser reads the T = 1000 table at the step's t, whatever the sampler's own schedule is
    eps = {dt: R.gaussian_eps_fn(dt, ac1000, ts, 1.0) for dt in (np.float32, np.float64)}
    if name == "ddim_img2img":
        def call(smp, model):
            return smp.img2img(model, dev(image), strength=0.5, noise=draws)
        refs = [E.img2img_loop(dt, kind, tabs, ts, 0.5, image.numpy(), eps[dt], draws.np)
                for dt in (np.float32, np.float64)]
    else:
        mask = soft if kind == "ddim" else binary
        coef = cpu._blend_table(ts, torch.device("cpu"))[0]

        def call(smp, model):
            return smp.inpaint(model, dev(image), dev(mask), resample=2, x_T=dev(xT), noise=draws)
        refs = [E.inpaint_loop(dt, kind, tabs, ts, coef, xT.numpy(), image.numpy(), mask.numpy(), 2, eps[dt],
                               draws.np) for dt in (np.float32, np.float64)]
    assert refs[0].dtype == np.float32 and refs[1].dtype == np.float64
    return call, torch.from_numpy(refs[0]), torch.from_numpy(refs[1])


@pytest.mark.parametrize("name", LOOP_CASES)
def test_loop_matches_float64(name):
    call, ref32, ref64 = loop_case(name)
    got = call(make_sampler(name.split("_")[0], DEV), GaussianDenoiser(1.0))
    assert got.shape == SHAPE and got.dtype == F32
    judge(name, got, ref32, ref64, rows=SHAPE[0])


# ------------------------------------------------------------------------------------------------------------
# the loops against the kernels composed by hand, on the tiny UNet
# ------------------------------------------------------------------------------------------------------------
def _unet(name):
    from diffusion_models_collection_amd.models import UNet
    from test_oracle import TINY
    torch.manual_seed(11)
    return UNet(**TINY[name]).to(DEV).eval()


USHAPE = (2, 3, 16, 16)


def unet_inputs(seed):
    g = rng(seed)
    image = torch.rand(USHAPE, generator=g) * 2 - 1
    mask = (torch.rand((USHAPE[0], 1) + USHAPE[2:], generator=g) < 0.5).float()
    return dev(torch.randn(USHAPE, generator=g)), dev(image), dev(mask)


def _full(v):
    return torch.full((USHAPE[0],), int(v), dtype=torch.long, device=DEV)


@pytest.mark.parametrize("pred", ["eps", "v"])
def test_inpaint_is_model_step_blend(pred, monkeypatch):
    """DDIM, 8 steps, resample = 2: inpaint == model + kernels.ddim_step + kernels.known_blend written out."""
    from diffusion_models_collection_amd.diffusion import DDIM, _edit
    L, K = _lib()
    monkeypatch.setenv("DMC_GRAPH", "0")
    m = _unet("unet_tiny_uncond")
    smp = DDIM(1000, 8, device=DEV, prediction_type=pred)
    xT, image, mask = unet_inputs(31)
    draws = Draws(USHAPE, 9)
    got = smp.inpaint(m, image, mask, resample=2, x_T=xT, noise=draws)
    ac = smp.alphas_cumprod
    ts = smp.inference_timesteps.tolist() + [-1]
    host = _edit.blend_coefficients(ac.cpu().numpy(), smp.inference_timesteps.cpu().numpy())
    coef = dev(torch.from_numpy(host))
    x = xT.clone()
    with torch.no_grad():
        for j, (i, renoise) in enumerate(_edit.edit_walk(8, 0, 2)):
            t, tn = _full(ts[i]), _full(ts[i + 1])
            eps, x0 = m(x, t[:1], None), None
            if pred == "v":
                eps, x0 = K.pred_convert("v", x, t, smp.sqrt_alphas_cumprod, smp.sqrt_one_minus_alphas_cumprod, eps)
            x = K.ddim_step(x, eps, t, tn, ac, eta=0.0, clip=True, x0=x0)
            r = 2 * i + renoise
            x = K.known_blend(x, image, mask, _full(r), coef, z=draws(j, "known") if host[r, 1] != 0 else None,
                              z2=draws(j, "renoise") if renoise else None)
    assert bool(got.isfinite().all()) and torch.equal(got, x)
    keep = mask.expand(USHAPE) == 1
    assert torch.equal(got[keep], image[keep])


def test_dpm_img2img_is_truncated_solver(monkeypatch):
    """DPMSolver.img2img(strength 0.5) == q_sample, then kernels.dpm_step over dpm_coefficients(ac, ts[i0:])."""
    from diffusion_models_collection_amd.diffusion import DPMSolver, _dpm, _edit
    L, K = _lib()
    monkeypatch.setenv("DMC_GRAPH", "0")
    m = _unet("unet_tiny_uncond")
    smp = DPMSolver(1000, 8, device=DEV)
    _, image, _ = unet_inputs(32)
    draws = Draws(USHAPE, 10)
    got = smp.img2img(m, image, strength=0.5, noise=draws)
    ts = smp.inference_timesteps.cpu().numpy()
    i0 = _edit.start_index(len(ts), 0.5)
    assert 0 < i0 < len(ts) - 1
    rows = _dpm.dpm_coefficients(smp.alphas_cumprod.cpu().numpy(), ts[i0:], 2, True)
    assert rows[0, 4] == 0 and smp.step_coefficients[i0, 4] != 0       # the first executed row is first order
    coef = dev(torch.from_numpy(rows))
    x = K.q_sample(image, draws(0, "start"), _full(ts[i0]), smp.sqrt_alphas_cumprod,
                   smp.sqrt_one_minus_alphas_cumprod)
    hist = None
    with torch.no_grad():
        for j in range(len(ts) - i0):
            t = _full(ts[i0 + j])
            x, hist = K.dpm_step(x, m(x, t[:1], None), _full(j), coef, clip=True, x0_prev=hist)
    assert bool(got.isfinite().all()) and torch.equal(got, x)
    assert smp._truncated_coefficients(i0, image.device) is smp._truncated_coefficients(i0, image.device)


def test_invert_is_p_sample_swapped(monkeypatch):
    """DDIM.invert == p_sample with (t, t_next) swapped over ascending timesteps, S - 1 model calls, unclipped.
    DDIM.sample's clip_denoised (there for the round trip) defaults to the clipped loop."""
    from diffusion_models_collection_amd.diffusion import DDIM
    monkeypatch.setenv("DMC_GRAPH", "0")
    m = _unet("unet_tiny_uncond")
    smp = DDIM(1000, 8, device=DEV)
    _, image, _ = unet_inputs(33)
    got = smp.invert(m, image)
    up = smp.inference_timesteps.flip(0).tolist()
    x = image.clone()
    with torch.no_grad():
        for k in range(len(up) - 1):
            t = _full(up[k])
            x = smp.p_sample(m, x, t, _full(up[k + 1]), clip_denoised=False, eps=m(x, t[:1], None))
    assert bool(got.isfinite().all()) and torch.equal(got, x) and not torch.equal(got, image)
    every = smp.invert(m, image, return_all_timesteps=True)
    assert every.shape == (len(up) - 1,) + USHAPE and torch.equal(every[-1], got.cpu())
    clipped = smp.sample(m, USHAPE, x_T=got)
    assert torch.equal(clipped, smp.sample(m, USHAPE, x_T=got, clip_denoised=True))
    assert float(clipped.abs().max()) <= 1.0
    assert bool(smp.sample(m, USHAPE, x_T=got, clip_denoised=False).isfinite().all())


# ------------------------------------------------------------------------------------------------------------
# graph replay against the eager loop
# ------------------------------------------------------------------------------------------------------------
def _graphs(smp):
    return [e[1] for e in smp.__dict__.get("_step_graphs", {}).values()]


def _graph_check(smp, m, calls, monkeypatch):
    """calls: two inpaint argument sets (different image, mask values, labels, x_T). DMC_GRAPH=0, =1 and the kept graph
    agree bitwise; one graph is kept; an in-place weight change recaptures."""
    def run(graph):
        monkeypatch.setenv("DMC_GRAPH", graph)
        return [smp.inpaint(m, *a, **kw) for a, kw in calls]

    eager = run("0")
    assert not _graphs(smp)
    graphed = run("1")
    kept = _graphs(smp)
    assert len(kept) == 1                                   # captured by the first call, replayed by the second
    again = run("1")
    assert _graphs(smp) == kept
    for a, b, c in zip(eager, graphed, again):
        assert bool(a.isfinite().all()) and torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(eager[0], eager[1])
    with torch.no_grad():
        next(m.parameters()).mul_(1.01)
    eager2, graphed2 = run("0"), run("1")
    assert len([g for g in _graphs(smp) if g not in kept]) == 1    # the new weights' graph, beside the old one
    for a, b in zip(eager2, graphed2):
        assert torch.equal(a, b)
    assert not torch.equal(eager[0], eager2[0])             # the model does drive the result


def _two_calls(resample, ya=None, yb=None, **kw):
    xa, ia, ma = unet_inputs(41)
    xb, ib, mb = unet_inputs(42)
    mb = mb * 0.75                                          # other mask values, the same layout
    da, db = Draws(USHAPE, 11), Draws(USHAPE, 12)
    return [((ia, ma), dict(y=ya, resample=resample, x_T=xa, noise=da, **kw)),
            ((ib, mb), dict(y=yb, resample=resample, x_T=xb, noise=db, **kw))]


def test_graph_equals_eager_inpaint(monkeypatch):
    from diffusion_models_collection_amd.diffusion import DDIM
    _graph_check(DDIM(1000, 8, device=DEV), _unet("unet_tiny_uncond"), _two_calls(2), monkeypatch)


@pytest.mark.parametrize("backbone", ["unet", "dit"])
def test_graph_equals_eager_inpaint_cfg(backbone, monkeypatch):
    from diffusion_models_collection_amd.diffusion import DDIM
    if backbone == "unet":
        m = _unet("unet_tiny_cond")
    else:
        import test_gpu_dit
        m, _ = test_gpu_dit.build("dit_tiny_cond")
        m.eval()
    ya, yb = torch.tensor([1, 2], device=DEV), torch.tensor([7, 5], device=DEV)
    _graph_check(DDIM(1000, 8, device=DEV), m, _two_calls(1, ya, yb, cfg_scale=3.0), monkeypatch)


# ------------------------------------------------------------------------------------------------------------
# entry points: refusals and return_all_timesteps
# ------------------------------------------------------------------------------------------------------------
def test_entry_point_refusals():
    from diffusion_models_collection_amd.diffusion import DDIM
    model = GaussianDenoiser(1.0)
    _, image, binary, _ = gauss_inputs()
    image, binary = dev(image), dev(binary)
    ddim, dpm = make_sampler("ddim", DEV), make_sampler("dpm", DEV)
    for smp in (ddim, make_sampler("ddpm", DEV), dpm):
        for strength in (0.0, -0.5, 1.5, float("nan")):
            with pytest.raises(ValueError):
                smp.img2img(model, image, strength=strength)
        for resample in (0, -1, 1.5):
            with pytest.raises(ValueError):
                smp.inpaint(model, image, binary, resample=resample)
        for bad in (binary * 1.5, binary - 0.25, torch.full_like(binary, NAN)):
            with pytest.raises(ValueError):
                smp.inpaint(model, image, bad)
        for shape in ((SHAPE[0], 2) + SHAPE[2:], (SHAPE[0] + 1, 1) + SHAPE[2:], (SHAPE[2] + 1, SHAPE[3])):
            with pytest.raises(ValueError):
                smp.inpaint(model, image, torch.zeros(shape))
        with pytest.raises(ValueError):
            smp.inpaint(model, image, binary, cfg_scale=3.0)            # CFG without labels
        with pytest.raises(ValueError):
            smp.img2img(model, image, cfg_scale=3.0)
        with pytest.raises(ValueError):
            smp.img2img(model, image, y=torch.zeros(SHAPE[0], dtype=torch.long), cfg_scale=3.0, p_threshold=1.0)
    with pytest.raises(ValueError):
        dpm.inpaint(model, image, binary, resample=2)
    with pytest.raises(NotImplementedError):
        dpm.invert(model, image)
    with pytest.raises(ValueError):
        DDIM(1000, 50, eta=0.5, device=DEV).invert(model, image)
    # a mask that broadcasts is taken: [H, W] and a scalar
    half = torch.zeros(SHAPE[2:])
    half[:, : SHAPE[3] // 2] = 1
    xT = dev(gauss_inputs()[0])
    a = ddim.inpaint(model, image, half, x_T=xT, noise=Draws(SHAPE, 13))
    b = ddim.inpaint(model, image, half.expand(SHAPE).contiguous(), x_T=xT, noise=Draws(SHAPE, 13))
    assert torch.equal(a, b) and torch.equal(a[..., : SHAPE[3] // 2], image[..., : SHAPE[3] // 2])


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_return_all_timesteps(kind):
    """One frame per walk entry (inpaint) or executed step (img2img); the last frame is the plain call's result."""
    from diffusion_models_collection_amd.diffusion import DDIM, DPMSolver, _edit
    m = _unet("unet_tiny_uncond")
    smp = DDIM(1000, 8, device=DEV) if kind == "ddim" else DPMSolver(1000, 8, device=DEV)
    xT, image, mask = unet_inputs(51)
    S = len(smp.inference_timesteps)
    U = 2 if kind == "ddim" else 1
    kw = dict(resample=U, x_T=xT)
    plain = smp.inpaint(m, image, mask, noise=Draws(USHAPE, 14), **kw)
    every = smp.inpaint(m, image, mask, noise=Draws(USHAPE, 14), return_all_timesteps=True, **kw)
    assert every.shape == (S * U,) + USHAPE
    assert torch.equal(every[-1], plain.cpu()) and not torch.equal(every[0], every[-1])
    plain = smp.img2img(m, image, strength=0.5, noise=Draws(USHAPE, 15))
    every = smp.img2img(m, image, strength=0.5, noise=Draws(USHAPE, 15), return_all_timesteps=True)
    assert every.shape == (S - _edit.start_index(S, 0.5),) + USHAPE
    assert torch.equal(every[-1], plain.cpu()) and not torch.equal(every[0], every[-1])


# ------------------------------------------------------------------------------------------------------------
# the references and input builders alone, on the CPU
# ------------------------------------------------------------------------------------------------------------
def cpu_selfcheck():
    """Runs every input builder and reference above without a GPU: every reference row is finite, the fp32 references
    pass their own criterion, and in every criterion-2 case the fp32 loop differs from the float64 one in every sample
    (4 x that difference is the margin: it must not be vacuous)."""
    n = 0
    coef = blend_table()
    assert coef.shape == (100, 4) and coef[98].tolist() == [1.0, 0.0, 1.0, 0.0]
    for N, per, mask_per in BLEND_SHAPES + [(3, 64, 64), (3, 8, 4)]:
        for soft in (False, True):
            for rot in range(4 if N < 4 else 1):
                x, x0, m, z, z2, row = blend_inputs(N, per, mask_per, soft, rot)
                xs, ms = blend_shapes(N, per, mask_per)
                assert x.shape == xs and m.shape == ms and m.numel() == N * mask_per
                assert bool(((m >= 0) & (m <= 1)).all()) and (soft or set(m.unique().tolist()) <= {0.0, 1.0})
                r32, r64 = (blend_ref(dt, coef, row, x, x0, m, z, z2) for dt in (F32, F64))
                assert bool(r32.isfinite().all()) and r32.dtype == F32 and r64.dtype == F64
                judge("selfcheck blend", r32, r32, r64, rows=N, quiet=True)
                n += 1
    for N, per, mask_per in ((5, 7, 7), (300, 48, 16)):
        x, x0, m, z, z2, row = blend_inputs(N, per, mask_per, True)
        pz, pz2 = poisoned(coef, row, z, z2)
        assert bool(pz.isnan().any()) and bool(pz2.isnan().any())
        n += 1
    xT, image, binary, soft = gauss_inputs()
    assert float(image.abs().max()) <= 1 and binary.shape == (SHAPE[0], 1) + SHAPE[2:] and soft.shape == SHAPE
    d = Draws(SHAPE, 3)
    assert torch.equal(d.cpu(2, "known"), d.cpu(2, "known")) and not torch.equal(d.cpu(2, "known"), d.cpu(2, "step"))
    for name in LOOP_CASES:
        _, ref32, ref64 = loop_case(name)
        assert bool(ref32.isfinite().all()) and bool(ref64.isfinite().all())
        differ = (ref32.double() - ref64).abs().reshape(SHAPE[0], -1).amax(1)
        assert bool((differ > 0).all()), (name, differ)
        judge("selfcheck " + name, ref32, ref32, ref64, rows=SHAPE[0], quiet=True)
        n += 1
    print(f"cpu_selfcheck ok: {n} reference cases")
    return n
