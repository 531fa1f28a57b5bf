"""Tensor-level wrappers over the C ABI (include/dmc.h).

Every function takes torch tensors that already live on the GPU, launches on torch's current stream
and returns without synchronising. Activations are NHWC tensors [N, H, W, ld] (ld = channel pitch).
No function here has a CPU or PyTorch-op fallback.
"""
import ctypes

import torch

from . import _lib as L
from ._lib import LIB, check, ptr

TAPS3 = [(kh - 1, kw - 1) for kh in range(3) for kw in range(3)]      # forward 3x3, pad 1
TAPS3_DGRAD = [(1 - kh, 1 - kw) for kh in range(3) for kw in range(3)]  # input-gradient of a 3x3 conv
TAPS1 = [(0, 0)]
TAPS_UPDGRAD = [(u - 1, v - 1) for u in range(4) for v in range(4)]    # folded nearest-x2 + 3x3 (4x4, s2)


class Scratch:
    """Grow-only device scratch (wgrad slabs, GN partials, ...), one buffer per HIP stream: kernels of one
    stream run in order and may share it; kernels on another stream (the executor's weight-gradient side
    stream) get their own. A buffer is allocated while its stream is current, so the caching allocator
    never hands it to another stream while its kernels are pending."""

    def __init__(self):
        self.bufs = {}

    def get(self, nbytes: int, device) -> torch.Tensor:
        nbytes = max(int(nbytes), 256)
        key = L.stream()   # stream handles are unique across devices
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)
            self.bufs[key] = buf
        return buf


SCRATCH = Scratch()


def make_desc(dtype, N, H, W, C1, C2, ld1, ld2, Kc, OH, OW, Cout, taps, mode=L.MODE_NORMAL, stride=1):
    d = L.ConvDesc()
    d.dtype = L.dtype_code(dtype)
    d.N, d.H, d.W = N, H, W
    d.C1, d.C2, d.ld1, d.ld2, d.Kc = C1, C2, ld1, ld2, Kc
    d.OH, d.OW, d.Cout = OH, OW, Cout
    d.ntaps, d.mode, d.stride = len(taps), mode, stride
    for i, (dy, dx) in enumerate(taps):
        d.tap_dy[i] = dy
        d.tap_dx[i] = dx
    d.Csplit = Cout
    d.drop_scale = 1.0
    return d


def drop_args(drop):
    """(seed, seed_base, thresh, scale) of a dropout spec (seed, thresh, scale[, seed_base]): seed_base is the
    device address of a uint32 added to seed in the kernels (a graph-captured step reads its seed there)."""
    if drop is None:
        return 0, None, 0, 1.0
    return drop[0], (drop[3] if len(drop) > 3 else None), drop[1], drop[2]


def set_prologue(d, kind=L.PRO_NONE, scale=None, shift=None, ld=0, drop=None, drop_ld=0):
    d.prologue = kind
    d._keep_pro = (scale, shift)   # the descriptor holds raw pointers: keep the tensors alive with it
    d.pro_scale = ptr(scale)
    d.pro_shift = ptr(shift)
    d.ld_pro = ld
    d.drop_seed, d.drop_seed_base, d.drop_thresh, d.drop_scale = drop_args(drop)
    d.drop_ld = drop_ld if drop is not None else 0


def set_epilogue(d, bias=None, addvec=None, ld_add=0, resid=None, ld_res=0, silu_pre=None, ld_silu=0,
                 ldy1=0, ldy2=0, Csplit=None, out_f32=False, out_nchw=False, act=L.ACT_NONE, y_pre=None, ld_pre=0,
                 gn_part=None):
    d._keep_epi = (bias, addvec, resid, silu_pre, y_pre, gn_part)   # keep what the raw pointers point at alive
    d.gn_part = ptr(gn_part)
    d.act = act
    d.y_pre = ptr(y_pre)
    d.ld_pre = ld_pre
    d.bias = ptr(bias)
    d.addvec = ptr(addvec)
    d.ld_add = ld_add
    d.resid = ptr(resid)
    d.ld_res = ld_res
    d.silu_pre = ptr(silu_pre)
    d.ld_silu = ld_silu
    d.ldy1, d.ldy2 = ldy1, ldy2
    d.Csplit = d.Cout if Csplit is None else Csplit
    d.out_f32 = int(out_f32)
    d.out_nchw = int(out_nchw)


class LayerProfile:
    """Opt-in (DMC_LAYER_PROF=1) per-call timing of the conv launches, keyed by kind and shape: HIP events on
    the launch stream around each call, read back by report(). Measurement tooling only."""

    def __init__(self):
        import os
        self.on = os.environ.get("DMC_LAYER_PROF", "0") not in ("", "0")
        self.pending = []

    def wrap(self, kind, d, fn):
        if not self.on:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        M = d.N * d.OH * d.OW
        key = (kind, d.dtype, d.N, d.H, d.W, d.C1 + d.C2, d.OH, d.OW, d.Cout, d.ntaps, d.mode)
        self.pending.append((key, 2.0 * M * d.Cout * d.ntaps * (d.C1 + d.C2), e0, e1))

    def report(self, steps=1):
        torch.cuda.synchronize()
        agg = {}
        for key, fl, e0, e1 in self.pending:
            a = agg.setdefault(key, [0, 0.0, 0.0])
            a[0] += 1
            a[1] += e0.elapsed_time(e1)
            a[2] += fl
        self.pending = []
        rows = sorted(agg.items(), key=lambda kv: -kv[1][1])
        tot = sum(v[1] for v in agg.values())
        lines = [f"conv launches: {tot / steps:.3f} ms/step"]
        for (kind, dt, N, H, W, Cin, OH, OW, Cout, nt, mode), (n, ms, fl) in rows:
            lines.append(f"{ms / steps * 1e3:8.1f} us/step  n/step {n / steps:4.1f}  avg {ms / n * 1e3:7.1f} us  "
                         f"{fl / (ms * 1e-3) / 1e12:7.1f} TF/s  {kind:5s} N{N} {H}x{W}x{Cin} -> {OH}x{OW}x{Cout} "
                         f"taps {nt} mode {mode}")
        return "\n".join(lines)


PROF = LayerProfile()


def conv(d, x1, x2, w, y1, y2=None):
    nbytes = LIB.dmc_conv2d_workspace(ctypes.byref(d))
    ws = SCRATCH.get(nbytes, y1.device) if nbytes else None
    PROF.wrap("conv", d, lambda: check(LIB.dmc_conv2d(ctypes.byref(d), ptr(x1), ptr(x2), ptr(w), ptr(y1), ptr(y2),
                                                      ptr(ws), nbytes, L.stream()), "dmc_conv2d"))


def conv_fused(d):
    """include/dmc.h dmc_conv2d_fused_epilogue: which optional outputs (L.FUSED_*) the kernel dmc_conv2d would run
    for `d` (with the workspace conv() passes) produces in its epilogue."""
    return LIB.dmc_conv2d_fused_epilogue(ctypes.byref(d), LIB.dmc_conv2d_workspace(ctypes.byref(d)))


def conv_plan(d, ws_bytes=None):
    """include/dmc.h dmc_conv2d_plan: the launch plan (L.ConvPlan) dmc_conv2d follows for `d` with a workspace of
    ws_bytes (default: what conv() passes). Host only."""
    if ws_bytes is None:
        ws_bytes = LIB.dmc_conv2d_workspace(ctypes.byref(d))
    p = L.ConvPlan()
    check(LIB.dmc_conv2d_plan(ctypes.byref(d), ws_bytes, ctypes.byref(p)), "dmc_conv2d_plan")
    return p


def conv_fold(d):
    """include/dmc.h dmc_conv_resample_fold: the output-parity fold (L.FOLD_*) dmc_conv2d can run the resampling conv
    `d` as (with the workspace conv() passes), 0 for none. The caller sets d.fold and passes the L.FOLD_PACK pack."""
    return LIB.dmc_conv_resample_fold(ctypes.byref(d), LIB.dmc_conv2d_workspace(ctypes.byref(d)))


def upsample2x(dtype, x, C):
    """Nearest x2 upsample of an NHWC [N, H, W, ld] activation's first C channels -> [N, 2H, 2W, C]."""
    N, H, W, ld = x.shape
    y = torch.empty(N, 2 * H, 2 * W, C, dtype=x.dtype, device=x.device)
    check(LIB.dmc_upsample2x_nhwc(L.dtype_code(dtype), ptr(x), N, H, W, C, ld, ptr(y), C, L.stream()),
          "dmc_upsample2x_nhwc")
    return y


def conv_halo_prologue(d):
    """True when dmc_conv2d applies d's GN-affine+SiLU prologue on the halo kernel's resident halo."""
    return bool(LIB.dmc_conv_halo_prologue(ctypes.byref(d)))


def _byte_span(t):
    """[first, past-the-last) device address a (possibly strided) tensor's elements occupy."""
    n = 1 + sum((sz - 1) * st for sz, st in zip(t.shape, t.stride())) if t.numel() else 0
    return t.data_ptr(), t.data_ptr() + n * t.element_size()


class WgradDefer:
    """Weight-gradient reductions deferred and batched (wgrad(defer=...) -> dmc_wgrad_reduce_batch).

    Each deferred call's fp32 partial sums get their own slice of a grow-only device arena and stay there until
    flush() reduces every pending job (<= 32 per launch) and recycles the arena. flush() runs every `every` jobs
    (DMC_WG_FLUSH_EVERY, default 3: the slabs are still in the 256 MB Infinity Cache when they are read back;
    3 measured best of 1-8 and of flushing only at the backward's segment ends: train 10,421 vs 10,365 img/s) and
    at every gradient-segment end (end_segment). When the pending jobs outgrow the arena they are flushed early
    and a larger arena is allocated; every arena ever allocated stays referenced (a captured HIP graph keeps
    using its addresses).

    The eligible 3x3 and 1x1 weight gradients are also collected into grouped launches (group_add -> wgrad_group,
    dmc_conv2d_wgrad_group), a queue per kind: `group` jobs (DMC_WG_DEFER = N, default 4; 3x3 alone at 1, 2, 3, 4, 6
    measured 11,637 / 11,906 / 11,926 / 11,930 / 11,678 img/s) share the block count of one conv's launch, so each
    conv's slab is up to N times smaller. end_segment() launches what is queued before it reduces."""

    def __init__(self):
        import os
        self.every = int(os.environ.get("DMC_WG_FLUSH_EVERY", "3"))
        # 3x3 weight gradients per grouped launch (dmc_conv2d_wgrad_group): the value of DMC_WG_DEFER, 1 = one launch
        # per conv
        self.group = max(1, min(int(os.environ.get("DMC_WG_DEFER", "4") or 1), L.WGRAD_GROUP_MAX))
        self.arenas = []
        self.buf = None
        self.off = 0
        self.jobs = []
        self.pending = []       # 3x3 group items not launched yet: (d, dy, ld_dy, x1, x2, dw, scale, dbias)
        self.pending_ow = 0
        self.pending1 = []      # the same for the 1x1 kind (any map size)

    def alloc(self, nbytes, device):
        nbytes = (max(int(nbytes), 256) + 255) // 256 * 256
        if self.buf is None or self.buf.device != device or self.off + nbytes > self.buf.numel():
            need = nbytes if self.buf is None or self.buf.device != device else self.off + nbytes
            self.flush()
            if self.buf is None or self.buf.device != device or need > self.buf.numel():
                self.buf = torch.empty(int(need * 1.25), dtype=torch.uint8, device=device)
                self.arenas.append(self.buf)
        ws = self.buf[self.off:self.off + nbytes]
        self.off += nbytes
        return ws

    def add(self, job):
        if job.splits == 0:
            return              # reduced inside the kernel (dmc_conv2d_wgrad_partial wrote dw directly)
        self.jobs.append(job)
        if self.every and len(self.jobs) >= self.every:
            self.flush()

    def flush(self):
        for k in range(0, len(self.jobs), 32):
            chunk = self.jobs[k:k + 32]
            arr = (L.WgradJob * len(chunk))(*chunk)
            check(LIB.dmc_wgrad_reduce_batch(arr, len(chunk), L.stream()), "dmc_wgrad_reduce_batch")
        self.jobs = []
        self.off = 0

    def group_add(self, item):
        """Queue a weight gradient for the next grouped launch if dmc_conv2d_wgrad_group takes it (returns False
        otherwise: the caller launches it alone). The queue holds the operand tensors, so the allocator cannot reuse
        them; the caller must not WRITE them before launch_pending() (see holds()). The group is launched when it
        reaches `group` jobs or a job of another map width arrives."""
        if self.group <= 1:
            return False
        ow = LIB.dmc_conv2d_wgrad_group_ok(ctypes.byref(item[0]), item[2])
        if not ow:
            return False
        if ow == 1:             # the 1x1 kind: a queue of its own
            self.pending1.append(item)
            if len(self.pending1) >= self.group:
                items, self.pending1 = self.pending1, []
                wgrad_group(items, defer=self)
            return True
        if self.pending and ow != self.pending_ow:
            self.launch_pending()
        self.pending.append(item)
        self.pending_ow = ow
        if len(self.pending) >= self.group:
            self.launch_pending()
        return True

    def holds(self, t):
        """True if the bytes tensor t spans overlap those of an operand of a queued, not yet launched weight gradient
        (views at any offset into an operand included)."""
        lo, hi = _byte_span(t)
        for it in self.pending + self.pending1:
            for o in (it[1], it[3], it[4]):
                if o is not None:
                    olo, ohi = _byte_span(o)
                    if lo < ohi and olo < hi:
                        return True
        return False

    def launch_pending(self):
        for items in (self.pending, self.pending1):
            if items:
                batch = items[:]
                del items[:]
                wgrad_group(batch, defer=self)

    def end_segment(self):
        self.launch_pending()
        self.flush()

    def reset(self):
        """Drop every pending job unreduced and recycle the arena. A backward starts with this: one that
        raised part-way (an OOM, a capture error the caller survived) leaves jobs holding raw slab / dw pointers that
        the next backward's first flush would otherwise replay onto reused buffers."""
        self.jobs = []
        self.pending = []
        self.pending1 = []
        self.off = 0


def wgrad_slab_bytes(reset=False):
    """Bytes of split partial sums the weight-gradient launches planned since the last reset (host-side counter)."""
    return LIB.dmc_wgrad_slab_bytes(int(reset))


def wgrad_plan(d, ld_dy):
    """include/dmc.h dmc_conv2d_wgrad_plan: the launch plan (L.WgradPlan) wgrad() follows for `d` and a dy pitch of
    ld_dy. Host only."""
    p = L.WgradPlan()
    check(LIB.dmc_conv2d_wgrad_plan(ctypes.byref(d), ld_dy, ctypes.byref(p)), "dmc_conv2d_wgrad_plan")
    return p


def wgrad_group(items, defer=None):
    """dmc_conv2d_wgrad_group: the partial-sum kernels of up to 8 eligible 3x3 weight gradients of one map width, or of
    up to 8 eligible 1x1 ones, in shared launches. items: (d, dy, ld_dy, x1, x2, dw, scale, dbias) each. With defer (a WgradDefer) the reductions
    join its batch, else they run at once in one dmc_wgrad_reduce_batch."""
    n = len(items)
    arr = (L.WgradGroupItem * n)()
    for i, (d, dy, ld_dy, x1, x2, dw, scale, dbias) in enumerate(items):
        d.wg_bias = ptr(dbias)
        d._keep_wgb = dbias
        arr[i].d = ctypes.pointer(d)
        arr[i].dy, arr[i].ld_dy, arr[i].x1, arr[i].x2 = ptr(dy), ld_dy, ptr(x1), ptr(x2)
        arr[i].dw, arr[i].scale = ptr(dw), scale
    sizes = (ctypes.c_size_t * n)()
    if not LIB.dmc_conv2d_wgrad_group_workspace(arr, n, sizes):
        raise L.DMCError("wgrad_group: the jobs are no valid group (bf16 stride-1 convs: 3x3 of one map width, or 1x1)")
    offs, total = [], 0
    for i in range(n):
        offs.append(total)
        total += (sizes[i] + 255) // 256 * 256
    dev = items[0][1].device
    ws = defer.alloc(total, dev) if defer is not None else SCRATCH.get(total, dev)
    for i in range(n):
        arr[i].workspace = ws.data_ptr() + offs[i]
    jobs = (L.WgradJob * n)()
    PROF.wrap("wgrad", items[0][0], lambda: check(LIB.dmc_conv2d_wgrad_group(arr, n, jobs, L.stream()),
                                                  "dmc_conv2d_wgrad_group"))
    if defer is not None:
        # all of the group's jobs first, then the flush check: a flush recycles the arena the group's slabs sit in
        defer.jobs.extend(L.WgradJob.from_buffer_copy(jobs[i]) for i in range(n))
        if defer.every and len(defer.jobs) >= defer.every:
            defer.flush()
        return
    check(LIB.dmc_wgrad_reduce_batch(jobs, n, L.stream()), "dmc_wgrad_reduce_batch")


def wgrad(d, dy, ld_dy, x1, x2, dw, scale=1.0, dbias=None, defer=None):
    """dmc_conv2d_wgrad: dw (and with dbias the bias gradient, the pixel sums of dy) from one pass over dy. With
    defer (a WgradDefer) only the partial-sum kernel runs now (dmc_conv2d_wgrad_partial); the reduction joins
    defer's batch."""
    d.wg_bias = ptr(dbias)
    d._keep_wgb = dbias
    if defer is not None and defer.group_add((d, dy, ld_dy, x1, x2, dw, scale, dbias)):
        return
    nbytes = LIB.dmc_conv2d_wgrad_workspace(ctypes.byref(d))
    if defer is not None:
        ws = defer.alloc(nbytes, dy.device)
        job = L.WgradJob()
        PROF.wrap("wgrad", d, lambda: check(LIB.dmc_conv2d_wgrad_partial(
            ctypes.byref(d), ptr(dy), ld_dy, ptr(x1), ptr(x2), ptr(ws), ptr(dw), scale, ctypes.byref(job), L.stream()),
            "dmc_conv2d_wgrad_partial"))
        defer.add(job)
        return
    ws = SCRATCH.get(nbytes, dy.device)
    PROF.wrap("wgrad", d, lambda: check(LIB.dmc_conv2d_wgrad(ctypes.byref(d), ptr(dy), ld_dy, ptr(x1), ptr(x2), ptr(ws),
                                                             ptr(dw), scale, L.stream()), "dmc_conv2d_wgrad"))


def pack_weight(mode, dtype, w, Kc, out=None):
    """fp32 [Cout][Cin][kh][kw] (or [Cout][Cin] Linear) -> packed kernel layout."""
    w = w.detach()
    if w.dim() == 2:
        Cout, Cin, kh, kw = w.shape[0], w.shape[1], 1, 1
    else:
        Cout, Cin, kh, kw = w.shape
    ntaps = 16 if mode in (L.PACK_UPDGRAD, L.PACK_UPFOLD) else kh * kw
    rows = Cout if mode in (L.PACK_FWD, L.PACK_UPFOLD) else Cin
    if out is None:
        out = torch.empty(rows * ntaps * Kc, dtype=dtype, device=w.device)
    check(LIB.dmc_pack_weight(mode, L.dtype_code(dtype), ptr(w.contiguous()), Cout, Cin, kh, kw, Kc, ptr(out),
                              L.stream()), "dmc_pack_weight")
    return out


class PackBatch:
    """Device arrays of dmc_pack_job + their tiles for one dmc_pack_weights launch.

    jobs: list of (w fp32 tensor, dst tensor, dst element offset, mode, Cout, Cin, kh, kw, Kc, koff)."""

    def __init__(self, jobs, device):
        arr = (L.PackJob * len(jobs))()
        self.keep = []
        tiles = []
        for i, (w, dst, off, mode, Cout, Cin, kh, kw, Kc, koff) in enumerate(jobs):
            w = w.detach()
            if not w.is_contiguous():
                raise L.DMCError("pack job: master weight must be contiguous")
            self.keep.append(w)
            j = arr[i]
            j.w = w.data_ptr()
            j.dst = dst.data_ptr() + off * dst.element_size()
            j.dtype = L.dtype_code(dst.dtype)
            j.mode, j.Cout, j.Cin, j.kh, j.kw, j.Kc, j.koff = mode, Cout, Cin, kh, kw, Kc, koff
            n = LIB.dmc_pack_tiles(ctypes.byref(j), i, None, 0)
            buf = (ctypes.c_int * (3 * n))()
            LIB.dmc_pack_tiles(ctypes.byref(j), i, buf, n)
            tiles.append(torch.frombuffer(bytearray(buf), dtype=torch.int32))
        self.count = len(jobs)
        t = torch.cat(tiles)
        self.ntiles = t.numel() // 3
        self.jobs = torch.frombuffer(bytearray(arr), dtype=torch.uint8).to(device)
        self.tiles = t.to(device)

    def launch(self):
        check(LIB.dmc_pack_weights(ptr(self.jobs), ptr(self.tiles), self.ntiles, L.stream()), "dmc_pack_weights")


def gn_stats(dtype, x1, x2, N, HW, C1, C2, ld1, ld2, G, eps, gamma, beta):
    C = C1 + C2
    dev = x1.device
    mr = torch.empty(N * G * 2, dtype=torch.float32, device=dev)
    sc = torch.empty(N * C, dtype=torch.float32, device=dev)
    sh = torch.empty(N * C, dtype=torch.float32, device=dev)
    ws = SCRATCH.get(LIB.dmc_gn_workspace(N, C, G, HW), dev)
    check(LIB.dmc_gn_stats(L.dtype_code(dtype), ptr(x1), ptr(x2), N, HW, C1, C2, ld1, ld2, G, eps, ptr(gamma),
                           ptr(beta), ptr(ws), ptr(mr), ptr(sc), ptr(sh), L.stream()), "dmc_gn_stats")
    return sc, sh, mr


def gn_finalize(p1, C1, p2, C2, N, HW, G, eps, gamma, beta, out=None):
    """GroupNorm (scale, shift, mean_rstd) from the producing convs' partials (dmc_conv_desc.gn_part); out: the
    three buffers to fill (allocated if None)."""
    dev = p1.device
    C = C1 + C2
    if out is None:
        out = (torch.empty(N * C, dtype=torch.float32, device=dev),
               torch.empty(N * C, dtype=torch.float32, device=dev),
               torch.empty(N * G * 2, dtype=torch.float32, device=dev))
    sc, sh, mr = out
    check(LIB.dmc_gn_finalize(ptr(p1), C1, ptr(p2), C2, N, HW, G, eps, ptr(gamma), ptr(beta), ptr(mr), ptr(sc),
                              ptr(sh), L.stream()), "dmc_gn_finalize")
    return sc, sh, mr


def gn_stats_apply_ok(dtype, N, HW, C1, C2, G):
    return bool(LIB.dmc_gn_stats_apply_ok(L.dtype_code(dtype), N, HW, C1, C2, G))


def gn_stats_apply(dtype, x1, x2, N, HW, C1, C2, ld1, ld2, G, eps, gamma, beta, silu=True, drop=None):
    """gn_stats + gn_apply in one launch (small samples, gn_stats_apply_ok): ((scale, shift, mean_rstd), a)."""
    C = C1 + C2
    dev = x1.device
    mr = torch.empty(N * G * 2, dtype=torch.float32, device=dev)
    sc = torch.empty(N * C, dtype=torch.float32, device=dev)
    sh = torch.empty(N * C, dtype=torch.float32, device=dev)
    out = torch.empty(N * HW * C, dtype=dtype, device=dev)
    seed, base, thresh, dscale = drop_args(drop)
    check(LIB.dmc_gn_stats_apply(L.dtype_code(dtype), ptr(x1), ptr(x2), N, HW, C1, C2, ld1, ld2, G, eps, ptr(gamma),
                                 ptr(beta), ptr(mr), ptr(sc), ptr(sh), int(silu), seed, base, thresh, dscale, ptr(out),
                                 C, L.stream()), "dmc_gn_stats_apply")
    return (sc, sh, mr), out


def gn_apply(dtype, x1, x2, N, HW, C1, C2, ld1, ld2, scale, shift, silu=True, drop=None, out=None):
    """a = dropout(silu(x*scale + shift)) materialised as [N*HW][C1+C2] (dtype)."""
    C = C1 + C2
    if out is None:
        out = torch.empty(N * HW * C, dtype=dtype, device=x1.device)
    seed, base, thresh, dscale = drop_args(drop)
    check(LIB.dmc_gn_apply(L.dtype_code(dtype), ptr(x1), ptr(x2), N, HW, C1, C2, ld1, ld2, ptr(scale), ptr(shift),
                           int(silu), seed, base, thresh, dscale, ptr(out), C, L.stream()), "dmc_gn_apply")
    return out


def gn_bwd(dtype, g, ld_g, x1, x2, N, HW, C1, C2, ld1, ld2, G, mr, gamma, beta, silu, drop, dx1, dx2, ld_dx1,
           ld_dx2, acc1, acc2, dgamma, dbeta, dx_sum_nc=None, ld_sum_nc=0, dx_sum_c=None, part=None, defer=None,
           add1=None, ld_add1=0):
    """GroupNorm(+SiLU+dropout) backward; optionally also the per-(n,c) / per-c pixel sums of dx (the bias and
    time-embedding gradients of the layer that produced x), fused into the dx pass. part: (sum dz, sum dz*xhat)
    partials from an earlier pass ([N*HW/64][C][2]), skipping the reduction. add1: a second operand added into dx1
    (single source, no pixel sums; folded into the one-pass kernel's dx pass on the deferred path)."""
    ws = SCRATCH.get(LIB.dmc_gn_workspace(N, C1 + C2, G, HW), g.device)
    seed, base, thresh, scale = drop_args(drop)
    if defer is not None:
        # the parameter column sums go to the caller's batch (colsum_batch) when the one-pass kernel takes the call
        C = C1 + C2
        a_keep = torch.empty(N * C * 2, dtype=torch.float32, device=g.device)
        s_keep = torch.empty(N * C, dtype=torch.float32, device=g.device) if dx_sum_c is not None else None
        flag = ctypes.c_int(0)
        check(LIB.dmc_gn_silu_bwd_deferred(
            L.dtype_code(dtype), ptr(g), ld_g, ptr(x1), ptr(x2), N, HW, C1, C2, ld1, ld2, G, ptr(mr), ptr(gamma),
            ptr(beta), int(silu), seed, base, thresh, scale, ptr(dx1), ptr(dx2), ld_dx1, ld_dx2, int(acc1), int(acc2),
            ptr(dgamma), ptr(dbeta), ptr(dx_sum_nc), ld_sum_nc, ptr(dx_sum_c), ptr(part), ptr(ws), ptr(a_keep),
            ptr(s_keep), ctypes.byref(flag), ptr(add1), int(ld_add1), L.stream()), "dmc_gn_silu_bwd_deferred")
        if flag.value:
            defer.append((a_keep, N, C, 2 * C, 2, dbeta, dgamma))
            if s_keep is not None:
                defer.append((s_keep, N, C, C, 1, dx_sum_c, None))
        return
    check(LIB.dmc_gn_silu_bwd(L.dtype_code(dtype), ptr(g), ld_g, ptr(x1), ptr(x2), N, HW, C1, C2, ld1, ld2, G, ptr(mr),
                              ptr(gamma), ptr(beta), int(silu), seed, base, thresh, scale, ptr(dx1), ptr(dx2), ld_dx1,
                              ld_dx2, int(acc1), int(acc2), ptr(dgamma), ptr(dbeta), ptr(dx_sum_nc), ld_sum_nc,
                              ptr(dx_sum_c), ptr(part), ptr(ws), L.stream()), "dmc_gn_silu_bwd")
    if add1 is not None:   # the immediate entry point has no extra operand: a separate add
        add_(dtype, dx1, add1)


def colsum_batch(jobs):
    """Launch the column sums gn_bwd(defer=jobs) left behind (dmc_colsum_batch, <= 56 per launch) and clear the
    list: out0[c] = sum_r in[r*ld + c*stride], out1 at +1 -- dgamma / dbeta / the bias sums."""
    for k in range(0, len(jobs), 56):
        chunk = jobs[k:k + 56]
        arr = (L.ColsumJob * len(chunk))()
        for j, (t, R, C, ld, stride, o0, o1) in enumerate(chunk):
            arr[j].in_, arr[j].R, arr[j].C, arr[j].ld, arr[j].stride = ptr(t), R, C, ld, stride
            arr[j].out0, arr[j].out1, arr[j].scale = ptr(o0), ptr(o1), 1.0
        check(LIB.dmc_colsum_batch(arr, len(chunk), L.stream()), "dmc_colsum_batch")
    jobs.clear()


def channel_sum(dtype, dy, N, HW, C, ld, out_nc=None, ld_out=0, out_c=None, scale=1.0):
    """Per-(n,c) and per-c pixel sums; wide tensors are processed in channel slices of <= 256 chunks."""
    step = 256 * L.chunk_for(dtype)
    esz = dy.element_size()
    for c0 in range(0, C, step):
        cs = min(step, C - c0)
        ws = SCRATCH.get(LIB.dmc_channel_sum_workspace(N, HW, cs), dy.device)
        onc = None if out_nc is None else out_nc.data_ptr() + 4 * c0
        oc = None if out_c is None else out_c.data_ptr() + 4 * c0
        check(LIB.dmc_channel_sum(L.dtype_code(dtype), dy.data_ptr() + esz * c0, N, HW, cs, ld, onc, ld_out, oc,
                                  scale, ptr(ws), L.stream()), "dmc_channel_sum")


def attn_fwd(dtype, qkv, ld_qkv, N, Lq, heads, hd, out, ld_out, lse, drop=None):
    """drop = (seed, thresh, scale[, seed_base]): attention-probability dropout (kernels.drop_args)."""
    seed, base, thresh, scale = drop_args(drop)
    check(LIB.dmc_attn_fwd(L.dtype_code(dtype), ptr(qkv), ld_qkv, N, Lq, heads, hd, ptr(out), ld_out, ptr(lse), seed,
                           base, thresh, scale, L.stream()), "dmc_attn_fwd")


def attn_bwd(dtype, qkv, ld_qkv, out, dout, ld_out, lse, N, Lq, heads, hd, dqkv, ld_dqkv, drop=None):
    ws = SCRATCH.get(LIB.dmc_attn_workspace(N, Lq, heads), qkv.device)
    seed, base, thresh, scale = drop_args(drop)
    check(LIB.dmc_attn_bwd(L.dtype_code(dtype), ptr(qkv), ld_qkv, ptr(out), ptr(dout), ld_out, ptr(lse), N, Lq, heads,
                           hd, ptr(dqkv), ld_dqkv, ptr(ws), seed, base, thresh, scale, L.stream()), "dmc_attn_bwd")


def time_embed(t, dim, out):
    check(LIB.dmc_time_embed(ptr(t), t.shape[0], dim, ptr(out), L.stream()), "dmc_time_embed")


def embed_fwd(y, table, out):
    check(LIB.dmc_embed_fwd(ptr(y), y.shape[0], table.shape[0], ptr(table), table.shape[1], ptr(out), L.stream()),
          "dmc_embed_fwd")


def embed_bwd(y, rows, dout, dtable):
    check(LIB.dmc_embed_bwd(ptr(y), y.shape[0], rows, ptr(dout), dout.shape[1], ptr(dtable), L.stream()),
          "dmc_embed_bwd")


def _same(ref, *ts, what):
    """Host-side operand validation before a launch: a shape the kernel does not expect is a Python error, never
    an out-of-bounds device access."""
    for t in ts:
        if t is not None and (t.shape != ref.shape or t.device != ref.device):
            raise L.DMCError(f"{what}: operand shape {tuple(t.shape)} on {t.device}, expected {tuple(ref.shape)} on "
                             f"{ref.device}")


def _steps(N, dev, *ts, what):
    for t in ts:
        if t is not None and (t.numel() != N or t.dtype != torch.long or t.device != dev or not t.is_contiguous()):
            raise L.DMCError(f"{what}: timesteps must be a contiguous int64 [{N}] tensor on {dev}, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")


def pack_input(dtype, x, ld, noise=None, t=None, a=None, b=None, out=None):
    N, C, H, W = x.shape
    _same(x, noise, what="dmc_pack_input")
    _steps(N, x.device, t, what="dmc_pack_input")
    if out is None:
        out = torch.empty(N, H, W, ld, dtype=dtype, device=x.device)
    check(LIB.dmc_pack_input(L.dtype_code(dtype), ptr(x), ptr(noise), ptr(t), ptr(a), ptr(b), N, C, H, W, ptr(out), ld,
                             L.stream()), "dmc_pack_input")
    return out


def unpack_output(dtype, src, ld, N, C, H, W, out=None):
    if out is None:
        out = torch.empty(N, C, H, W, dtype=torch.float32, device=src.device)
    check(LIB.dmc_unpack_output(L.dtype_code(dtype), ptr(src), ld, N, C, H, W, ptr(out), L.stream()),
          "dmc_unpack_output")
    return out


def add_(dtype, y, x):
    check(LIB.dmc_add(L.dtype_code(dtype), ptr(y), ptr(x), y.numel(), L.stream()), "dmc_add")


def silu_fwd(x, out=None):
    """y = x * sigmoid(x) of a contiguous fp32 tensor (dmc_silu_fwd)."""
    if out is None:
        out = torch.empty_like(x)
    _same(x, out, what="dmc_silu_fwd")
    check(LIB.dmc_silu_fwd(ptr(x), ptr(out), x.numel(), L.stream()), "dmc_silu_fwd")
    return out


def q_sample(x0, noise, t, a, b, out=None):
    x0 = x0.contiguous()
    noise = noise.contiguous()
    if out is None:
        out = torch.empty_like(x0, dtype=torch.float32)
    N = x0.shape[0]
    _same(x0, noise, out, what="dmc_q_sample")
    _steps(N, x0.device, t, what="dmc_q_sample")
    check(LIB.dmc_q_sample(ptr(x0), ptr(noise), ptr(t), ptr(a), ptr(b), N, x0.numel() // max(N, 1), ptr(out),
                           L.stream()), "dmc_q_sample")
    return out


def loss_fwd(loss_type, pred, target):
    _same(pred, target, what="dmc_loss_fwd")
    n = pred.numel()
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    ws = SCRATCH.get(4096 * 4, pred.device)
    check(LIB.dmc_loss_fwd(L.LOSS[loss_type], ptr(pred), ptr(target), n, ptr(loss), ptr(ws), L.stream()),
          "dmc_loss_fwd")
    return loss


def loss_bwd(loss_type, pred, target, dloss):
    dpred = torch.empty_like(pred)
    check(LIB.dmc_loss_bwd(L.LOSS[loss_type], ptr(pred), ptr(target), pred.numel(), ptr(dloss), ptr(dpred),
                           L.stream()), "dmc_loss_bwd")
    return dpred


def _fp32_contig(what, *ts):
    for t in ts:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise L.DMCError(f"{what}: operands must be contiguous fp32, got {t.dtype} strides {t.stride()}")


def _tables(what, dev, *tabs):
    """Length of the [T] fp32 device tables (all the same length; None entries are skipped)."""
    T = None
    for tab in tabs:
        if tab is None:
            continue
        if (tab.dim() != 1 or tab.numel() < 1 or tab.dtype != torch.float32 or tab.device != dev
                or not tab.is_contiguous() or (T is not None and tab.numel() != T)):
            raise L.DMCError(f"{what}: tables must be contiguous fp32 [T] tensors of one length on {dev}, got "
                             f"{tab.dtype} {tuple(tab.shape)} on {tab.device}")
        T = tab.numel()
    return T


def _pred_code(what, pred_type):
    if pred_type not in L.PRED:
        raise L.DMCError(f"{what}: unknown prediction type {pred_type!r}")
    return L.PRED[pred_type]


def objective(pred_type, loss_type, pred, x0, noise, t, sa, s1, w=None, dloss=None, grad=True, out=None):
    """Loss and its gradient in one pass (dmc_objective): target = noise ('eps') or sa[t]*noise - s1[t]*x0 ('v'), a
    per-sample weight w[t] (None: 1), mean over samples of the per-sample means. grad=False is the forward alone.
    Returns (loss, dpred or None); dloss: the upstream gradient, a device scalar; out: the dpred buffer to fill."""
    what = "dmc_objective"
    code, T, N, loss, dpred, ws = _objective_operands(what, pred_type, loss_type, pred, x0, noise, t, sa, s1, (w,), dloss,
                                                      grad, out)
    check(LIB.dmc_objective(code, L.LOSS[loss_type], ptr(pred), ptr(x0), ptr(noise), ptr(t), ptr(sa), ptr(s1), ptr(w),
                            T, N, pred.numel() // N, ptr(dloss) if grad else None, ptr(loss), ptr(dpred), ptr(ws),
                            L.stream()), what)
    return loss, dpred


def objective_is(pred_type, loss_type, pred, x0, noise, t, sa, s1, w=None, iw=None, dloss=None, grad=True, out=None,
                 row_loss=True):
    """objective under importance-sampled timesteps (dmc_objective_is): iw, the [T] importance weights of ts_sample
    (None: 1), is each sample's last factor in the loss and the gradient. Returns (loss, row_loss or None, dpred or
    None); row_loss [N] is each sample's own loss before iw, what ts_history_update takes."""
    what = "dmc_objective_is"
    code, T, N, loss, dpred, ws = _objective_operands(what, pred_type, loss_type, pred, x0, noise, t, sa, s1, (w, iw),
                                                      dloss, grad, out)
    row = torch.empty(N, dtype=torch.float32, device=pred.device) if row_loss else None
    check(LIB.dmc_objective_is(code, L.LOSS[loss_type], ptr(pred), ptr(x0), ptr(noise), ptr(t), ptr(sa), ptr(s1), ptr(w),
                               ptr(iw), T, N, pred.numel() // N, ptr(dloss) if grad else None, ptr(loss), ptr(row),
                               ptr(dpred), ptr(ws), L.stream()), what)
    return loss, row, dpred


def _objective_operands(what, pred_type, loss_type, pred, x0, noise, t, sa, s1, tabs, dloss, grad, out):
    """The operand checks and buffers objective and objective_is share: (prediction code, T, N, loss, dpred or None,
    workspace). tabs: the optional [T] tables beside sa and s1."""
    code = _pred_code(what, pred_type)
    if loss_type not in L.LOSS:
        raise L.DMCError(f"{what}: unknown loss type {loss_type!r}")
    if not pred.is_cuda or pred.dim() < 1 or pred.numel() < 1:
        raise L.DMCError(f"{what}: pred must be a non-empty device tensor, got {tuple(pred.shape)} on {pred.device}")
    N = pred.shape[0]
    _same(pred, x0, noise, what=what)
    _fp32_contig(what, pred, x0, noise)
    _steps(N, pred.device, t, what=what)
    T = _tables(what, pred.device, sa, s1, *tabs)
    if t is None or T is None or sa is None or s1 is None:
        raise L.DMCError(f"{what}: needs timesteps and the sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod tables")
    dpred = None
    if grad:
        if dloss is None or dloss.numel() != 1 or dloss.dtype != torch.float32 or dloss.device != pred.device:
            raise L.DMCError(f"{what}: dloss must be one fp32 value on {pred.device}")
        dpred = torch.empty_like(pred) if out is None else out
        _same(pred, dpred, what=what)
        _fp32_contig(what, dpred)
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    ws = SCRATCH.get(L.OBJECTIVE_MAX_BLOCKS * N * 4, pred.device)
    return code, T, N, loss, dpred, ws


def pred_convert(pred_type, x, t, sa, s1, pred, want_x0=True, out=None):
    """(eps, x0 or None) from a v-prediction model output (dmc_pred_convert). pred holds reps * N rows for x's N:
    row r*N + n pairs with x[n], t[n] (reps = 2: the batched cond / uncond forward of CFG). out: the buffers to fill."""
    what = "dmc_pred_convert"
    code = _pred_code(what, pred_type)
    if code == L.PRED["eps"]:
        raise L.DMCError(f"{what}: an eps prediction needs no conversion")
    if not x.is_cuda or x.dim() < 1 or x.numel() < 1:
        raise L.DMCError(f"{what}: x must be a non-empty device tensor, got {tuple(x.shape)} on {x.device}")
    N = x.shape[0]
    reps = pred.shape[0] // N if pred.dim() == x.dim() else 0
    if reps < 1 or pred.shape != (reps * N,) + tuple(x.shape[1:]) or pred.device != x.device:
        raise L.DMCError(f"{what}: pred {tuple(pred.shape)} on {pred.device} is not reps x {tuple(x.shape)} on "
                         f"{x.device}")
    eps, x0 = out if out is not None else (torch.empty_like(pred), torch.empty_like(pred) if want_x0 else None)
    _same(pred, eps, x0, what=what)
    _fp32_contig(what, x, pred, eps, x0)
    _steps(N, x.device, t, what=what)
    T = _tables(what, x.device, sa, s1)
    if t is None or T is None or sa is None or s1 is None:
        raise L.DMCError(f"{what}: needs timesteps and the sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod tables")
    check(LIB.dmc_pred_convert(code, ptr(x), ptr(t), ptr(sa), ptr(s1), T, ptr(pred), reps, N, x.numel() // N, ptr(eps),
                               ptr(x0), L.stream()), what)
    return eps, x0


def vlb_step(x0, x_t, pred, t, coef, clip=True, z_next=None, t_next=None, sa=None, s1=None, x_next=None, out=None):
    """One timestep of the variational bound (dmc_vlb_step): t[n] picks sample n's row {c_x, c_p, kprec, kvar, keps,
    isig} of the [T, 6] table (diffusion/_vlb.py). Returns (vb, xstart_mse, eps_mse, x0_sq), [N] fp32 each; out: the
    four buffers to fill. With x_next (a buffer of x0's shape), samples with t_next >= 0 get
    x_next = sa[t_next]*x0 + s1[t_next]*z_next in the same pass; the others are not written."""
    what = "dmc_vlb_step"
    if not x0.is_cuda or x0.dim() < 1 or x0.numel() < 1:
        raise L.DMCError(f"{what}: x0 must be a non-empty device tensor, got {tuple(x0.shape)} on {x0.device}")
    N = x0.shape[0]
    dev = x0.device
    _same(x0, x_t, pred, z_next, x_next, what=what)
    _fp32_contig(what, x0, x_t, pred, z_next, x_next)
    if t is None:
        raise L.DMCError(f"{what}: needs timesteps")
    _steps(N, dev, t, t_next, what=what)
    if (coef.dim() != 2 or coef.shape[1] != 6 or coef.shape[0] < 1 or coef.dtype != torch.float32
            or coef.device != dev or not coef.is_contiguous()):
        raise L.DMCError(f"{what}: coef must be a contiguous fp32 [T, 6] tensor on {dev}, got "
                         f"{coef.dtype} {tuple(coef.shape)} on {coef.device}")
    T = coef.shape[0]
    if x_next is not None:
        if z_next is None or t_next is None or _tables(what, dev, sa, s1) != T or sa is None or s1 is None:
            raise L.DMCError(f"{what}: x_next needs z_next, t_next and the [T = {T}] sqrt_alphas_cumprod / "
                             "sqrt_one_minus_alphas_cumprod tables")
    rows = out if out is not None else tuple(torch.empty(N, dtype=torch.float32, device=dev) for _ in range(4))
    if len(rows) != 4:
        raise L.DMCError(f"{what}: out must hold the four [N] buffers vb, xstart_mse, eps_mse, x0_sq")
    for r in rows:
        if r.shape != (N,) or r.device != dev:
            raise L.DMCError(f"{what}: an output row is {tuple(r.shape)} on {r.device}, expected ({N},) on {dev}")
    _fp32_contig(what, *rows)
    ws = SCRATCH.get(4 * L.VLB_MAX_BLOCKS * N * 4, dev)
    nxt = x_next is not None
    check(LIB.dmc_vlb_step(ptr(x0), ptr(x_t), ptr(pred), ptr(t), ptr(coef), T, int(bool(clip)),
                           ptr(z_next) if nxt else None, ptr(t_next) if nxt else None, ptr(sa) if nxt else None,
                           ptr(s1) if nxt else None, N, x0.numel() // N, ptr(x_next), ptr(rows[0]), ptr(rows[1]),
                           ptr(rows[2]), ptr(rows[3]), ptr(ws), L.stream()), what)
    return tuple(rows)


def _lvar_coef(what, coef, dev):
    if (coef is None or coef.dim() != 2 or coef.shape[1] != L.LVAR_COLS or coef.shape[0] < 1
            or coef.dtype != torch.float32 or coef.device != dev or not coef.is_contiguous()):
        raise L.DMCError(f"{what}: coef must be a contiguous fp32 [T, {L.LVAR_COLS}] tensor on {dev} "
                         "(diffusion/_vlb.py learned_coefficients)")
    return coef.shape[0]


def _halves(what, out, ref):
    """(prediction half, v half, row stride) of a model output [N, 2C, ...] for ref = [N, C, ...]: views, read in place."""
    if (out.dim() != ref.dim() or out.shape[0] != ref.shape[0] or out.shape[1] != 2 * ref.shape[1]
            or out.shape[2:] != ref.shape[2:] or out.device != ref.device):
        raise L.DMCError(f"{what}: the model output is {tuple(out.shape)} on {out.device}, expected twice the channels of "
                         f"{tuple(ref.shape)} on {ref.device}")
    _fp32_contig(what, out)
    C = ref.shape[1]
    return out[:, :C], out[:, C:], out.stride(0)


def hybrid_objective(pred_type, loss_type, out, x0, noise, t, sa, s1, coef, w=None, vlb_weight=0.001, dloss=None,
                     grad=True, dout=None):
    """L_simple + vlb_weight * mean_n vb_n and its gradient in one pass (dmc_hybrid_objective). out: the model output
    [N, 2C, ...], prediction half then v; x0, noise: [N, C, ...]; coef: the [T, 8] table of
    diffusion/_vlb.py learned_coefficients. Returns (loss[3] = {total, simple, vlb}, dout or None)."""
    what = "dmc_hybrid_objective"
    code, T, N, loss, dout, ws = _hybrid_operands(what, pred_type, loss_type, out, x0, noise, t, sa, s1, coef,
                                                  {"w": w}, dloss, grad, dout)
    check(LIB.dmc_hybrid_objective(code, L.LOSS[loss_type], ptr(out), ptr(x0), ptr(noise), ptr(t), ptr(sa), ptr(s1),
                                   ptr(w), ptr(coef), T, N, x0.numel() // N, float(vlb_weight),
                                   ptr(dloss) if grad else None, ptr(loss), ptr(dout), ptr(ws), L.stream()), what)
    return loss, dout


def hybrid_objective_is(pred_type, loss_type, out, x0, noise, t, sa, s1, coef, w=None, iw=None, vlb_weight=0.001,
                        dloss=None, grad=True, dout=None, row_loss=True):
    """hybrid_objective under importance-sampled timesteps (dmc_hybrid_objective_is), as objective_is. Returns
    (loss[3], row_loss or None, dout or None); row_loss[n] = simple_n + vlb_weight * vb_n, before iw."""
    what = "dmc_hybrid_objective_is"
    code, T, N, loss, dout, ws = _hybrid_operands(what, pred_type, loss_type, out, x0, noise, t, sa, s1, coef,
                                                  {"w": w, "iw": iw}, dloss, grad, dout)
    row = torch.empty(N, dtype=torch.float32, device=x0.device) if row_loss else None
    check(LIB.dmc_hybrid_objective_is(code, L.LOSS[loss_type], ptr(out), ptr(x0), ptr(noise), ptr(t), ptr(sa), ptr(s1),
                                      ptr(w), ptr(iw), ptr(coef), T, N, x0.numel() // N, float(vlb_weight),
                                      ptr(dloss) if grad else None, ptr(loss), ptr(row), ptr(dout), ptr(ws),
                                      L.stream()), what)
    return loss, row, dout


def _hybrid_operands(what, pred_type, loss_type, out, x0, noise, t, sa, s1, coef, tabs, dloss, grad, dout):
    """The operand checks and buffers hybrid_objective and hybrid_objective_is share: (prediction code, T, N, loss[3],
    dout or None, workspace). tabs: name -> the optional [T] tables beside sa and s1."""
    code = _pred_code(what, pred_type)
    if loss_type not in L.LOSS:
        raise L.DMCError(f"{what}: unknown loss type {loss_type!r}")
    if not x0.is_cuda or x0.dim() < 2 or x0.numel() < 1:
        raise L.DMCError(f"{what}: x0 must be a non-empty [N, C, ...] device tensor, got {tuple(x0.shape)} on "
                         f"{x0.device}")
    N, dev = x0.shape[0], x0.device
    _halves(what, out, x0)
    _same(x0, noise, what=what)
    _fp32_contig(what, x0, noise)
    if t is None:
        raise L.DMCError(f"{what}: needs timesteps")
    _steps(N, dev, t, what=what)
    T = _lvar_coef(what, coef, dev)
    if (_tables(what, dev, sa, s1, *tabs.values()) not in (None, T)
            or (code == L.PRED["v"] and (sa is None or s1 is None))):
        names = ", ".join(["sa", "s1"] + list(tabs)[:-1]) + " and " + list(tabs)[-1]
        raise L.DMCError(f"{what}: {names} must be [T = {T}] tables (sa and s1 are needed for v-prediction)")
    if grad:
        if dloss is None or dloss.numel() != 1 or dloss.dtype != torch.float32 or dloss.device != dev:
            raise L.DMCError(f"{what}: dloss must be one fp32 value on {dev}")
        dout = torch.empty_like(out) if dout is None else dout
        _same(out, dout, what=what)
        _fp32_contig(what, dout)
    else:
        dout = None
    loss = torch.empty(3, dtype=torch.float32, device=dev)
    ws = SCRATCH.get(2 * L.OBJECTIVE_MAX_BLOCKS * N * 4, dev)
    return code, T, N, loss, dout, ws


def _ts_state(what, hist, count):
    """(T, K) of the loss history: hist fp32 [T, K] and count int32 [T], contiguous, on one device."""
    if (not hist.is_cuda or hist.dim() != 2 or hist.numel() < 1 or hist.dtype != torch.float32
            or not hist.is_contiguous() or count.shape != (hist.shape[0],) or count.dtype != torch.int32
            or count.device != hist.device or not count.is_contiguous()):
        raise L.DMCError(f"{what}: the history must be a contiguous fp32 [T, K] device tensor with an int32 [T] count "
                         f"beside it, got {hist.dtype} {tuple(hist.shape)} on {hist.device} and {count.dtype} "
                         f"{tuple(count.shape)} on {count.device}")
    return hist.shape


def ts_history_update(t, loss, hist, count):
    """hist[tt][count[tt] % K] = loss[n]; ++count[tt] for n in index order, tt = t[n] clamped into [0, T)
    (dmc_ts_history_update): the last K losses per timestep, in place, exactly as the sequential loop leaves them."""
    what = "dmc_ts_history_update"
    T, K = _ts_state(what, hist, count)
    N = loss.numel()
    if N < 1 or loss.dim() != 1 or loss.device != hist.device:
        raise L.DMCError(f"{what}: loss must be a non-empty [N] tensor on {hist.device}, got {tuple(loss.shape)} on "
                         f"{loss.device}")
    _fp32_contig(what, loss)
    if t is None:
        raise L.DMCError(f"{what}: needs timesteps")
    _steps(N, hist.device, t, what=what)
    check(LIB.dmc_ts_history_update(ptr(t), ptr(loss), N, T, K, ptr(hist), ptr(count), L.stream()), what)


def ts_sample(hist, count, uniform_prob, u, out=None):
    """Loss-second-moment timestep draw in one launch (dmc_ts_sample): p ~ sqrt(mean_k hist^2) mixed with uniform_prob
    of the uniform distribution (uniform, iw = 1, until every count >= K), iw = 1/(T p), cdf, and t[n] = the smallest i
    with cdf[i] > u[n] for the caller's draws u in [0, 1). Returns (t int64 [N], p, iw, cdf: fp32 [T]); out: the three
    [T] buffers to fill."""
    what = "dmc_ts_sample"
    T, K = _ts_state(what, hist, count)
    dev = hist.device
    if u.dim() != 1 or u.numel() < 1 or u.device != dev:
        raise L.DMCError(f"{what}: u must be a non-empty [N] tensor on {dev}, got {tuple(u.shape)} on {u.device}")
    _fp32_contig(what, u)
    if not 0.0 <= float(uniform_prob) < 1.0:
        raise L.DMCError(f"{what}: uniform_prob {uniform_prob!r} is not in [0, 1)")
    p, iw, cdf = out if out is not None else (torch.empty(T, dtype=torch.float32, device=dev) for _ in range(3))
    if _tables(what, dev, p, iw, cdf) != T:
        raise L.DMCError(f"{what}: p, iw and cdf must be [T = {T}] tables")
    t = torch.empty(u.numel(), dtype=torch.long, device=dev)
    check(LIB.dmc_ts_sample(ptr(hist), ptr(count), T, K, float(uniform_prob), ptr(u), u.numel(), ptr(t), ptr(p), ptr(iw),
                            ptr(cdf), L.stream()), what)
    return t, p, iw, cdf


def vlb_step_learned(x0, x_t, out, t, coef, clip=True, z_next=None, t_next=None, sa=None, s1=None, x_next=None,
                     rows=None):
    """dmc_vlb_step with the learned variance (dmc_vlb_step_learned): out is the model output [N, 2C, ...], both halves
    read in place; coef the [T, 8] table of diffusion/_vlb.py learned_coefficients. Otherwise as vlb_step (rows: the
    four [N] buffers to fill)."""
    what = "dmc_vlb_step_learned"
    if not x0.is_cuda or x0.dim() < 2 or x0.numel() < 1:
        raise L.DMCError(f"{what}: x0 must be a non-empty [N, C, ...] device tensor, got {tuple(x0.shape)} on "
                         f"{x0.device}")
    N, dev = x0.shape[0], x0.device
    pred, v, ld = _halves(what, out, x0)
    _same(x0, x_t, z_next, x_next, what=what)
    _fp32_contig(what, x0, x_t, z_next, x_next)
    if t is None:
        raise L.DMCError(f"{what}: needs timesteps")
    _steps(N, dev, t, t_next, what=what)
    T = _lvar_coef(what, coef, dev)
    if x_next is not None:
        if z_next is None or t_next is None or _tables(what, dev, sa, s1) != T or sa is None or s1 is None:
            raise L.DMCError(f"{what}: x_next needs z_next, t_next and the [T = {T}] sqrt_alphas_cumprod / "
                             "sqrt_one_minus_alphas_cumprod tables")
    rows = rows if rows is not None else tuple(torch.empty(N, dtype=torch.float32, device=dev) for _ in range(4))
    if len(rows) != 4:
        raise L.DMCError(f"{what}: rows must hold the four [N] buffers vb, xstart_mse, eps_mse, x0_sq")
    for r in rows:
        if r.shape != (N,) or r.device != dev:
            raise L.DMCError(f"{what}: an output row is {tuple(r.shape)} on {r.device}, expected ({N},) on {dev}")
    _fp32_contig(what, *rows)
    ws = SCRATCH.get(4 * L.VLB_MAX_BLOCKS * N * 4, dev)
    nxt = x_next is not None
    check(LIB.dmc_vlb_step_learned(ptr(x0), ptr(x_t), ptr(pred), ld, ptr(v), ld, ptr(t), ptr(coef), T, int(bool(clip)),
                                   ptr(z_next) if nxt else None, ptr(t_next) if nxt else None,
                                   ptr(sa) if nxt else None, ptr(s1) if nxt else None, N, x0.numel() // N, ptr(x_next),
                                   ptr(rows[0]), ptr(rows[1]), ptr(rows[2]), ptr(rows[3]), ptr(ws), L.stream()), what)
    return tuple(rows)


def ddpm_step_learned(x, out, t, sra, srm1, c1, c2, coef, clip=True, eps=None, x0=None, z=None, res=None):
    """DDPM step with the learned variance (dmc_ddpm_step_learned). out: the model output [N, 2C, ...]; its v half is
    read in place, and so is its prediction half unless eps (a contiguous [N, C, ...] eps: the guided or converted one)
    is given; x0 (optional, with eps) replaces the x0 prediction. z None: the mean, with dmc_ddpm_step's bits."""
    what = "dmc_ddpm_step_learned"
    if not x.is_cuda or x.dim() < 2 or x.numel() < 1:
        raise L.DMCError(f"{what}: x must be a non-empty [N, C, ...] device tensor, got {tuple(x.shape)} on {x.device}")
    N, dev = x.shape[0], x.device
    per = x.numel() // N
    pred, v, ld = _halves(what, out, x)
    if x0 is not None and eps is None:
        raise L.DMCError(f"{what}: x0 comes with the eps it was formed from")
    res = torch.empty_like(x) if res is None else res
    _same(x, eps, x0, z, res, what=what)
    _fp32_contig(what, x, eps, x0, z, res)
    if t is None:
        raise L.DMCError(f"{what}: needs timesteps")
    _steps(N, dev, t, what=what)
    T = _lvar_coef(what, coef, dev)
    if _tables(what, dev, sra, srm1, c1, c2) != T or any(tab is None for tab in (sra, srm1, c1, c2)):
        raise L.DMCError(f"{what}: needs the four [T = {T}] sqrt_recip / posterior_mean_coef tables")
    e, eld = (pred, ld) if eps is None else (eps, per)
    check(LIB.dmc_ddpm_step_learned(ptr(x), ptr(e), eld, ptr(v), ld, ptr(x0), ptr(t), ptr(sra), ptr(srm1), ptr(c1),
                                    ptr(c2), ptr(coef), T, N, per, int(bool(clip)), ptr(z), ptr(res), L.stream()), what)
    return res


def ddim_step(x, eps, t, t_next, alphas_cumprod, eta=0.0, clip=True, x0=None, z=None, out=None):
    if out is None:
        out = torch.empty_like(x)
    N = x.shape[0]
    _same(x, eps, x0, z, out, what="dmc_ddim_step")
    _steps(N, x.device, t, t_next, what="dmc_ddim_step")
    check(LIB.dmc_ddim_step(ptr(x), ptr(eps), ptr(x0), ptr(t), ptr(t_next), ptr(alphas_cumprod), N, x.numel() // N,
                            float(eta), int(clip), ptr(z), ptr(out), L.stream()), "dmc_ddim_step")
    return out


def ddpm_step(x, eps, t, sra, srm1, c1, c2, logvar, clip=True, x0=None, z=None, out=None):
    if out is None:
        out = torch.empty_like(x)
    N = x.shape[0]
    _same(x, eps, x0, z, out, what="dmc_ddpm_step")
    _steps(N, x.device, t, what="dmc_ddpm_step")
    check(LIB.dmc_ddpm_step(ptr(x), ptr(eps), ptr(x0), ptr(t), ptr(sra), ptr(srm1), ptr(c1), ptr(c2), ptr(logvar), N,
                            x.numel() // N, int(clip), ptr(z), ptr(out), L.stream()), "dmc_ddpm_step")
    return out


def dpm_step(x, eps, step, coef, clip=True, x0=None, x0_prev=None, out=None, x0_out=None):
    """DPM-Solver++ update (dmc_dpm_step): step[n] picks sample n's row of the [S, 5] coefficient table
    (diffusion/_dpm.py). eps may be None when x0 is given; x0_out may be x0_prev. Returns (out, x0_out)."""
    if out is None:
        out = torch.empty_like(x)
    if x0_out is None:
        x0_out = torch.empty_like(x)
    N = x.shape[0]
    if eps is None and x0 is None:
        raise L.DMCError("dmc_dpm_step: eps may be None only when x0 is given")
    _same(x, eps, x0, x0_prev, out, x0_out, what="dmc_dpm_step")
    _steps(N, x.device, step, what="dmc_dpm_step")
    if step is None or N < 1 or x.numel() < 1:
        raise L.DMCError(f"dmc_dpm_step: needs a step index and a non-empty batch, got shape {tuple(x.shape)}")
    for t in (x, eps, x0, x0_prev, out, x0_out):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise L.DMCError(f"dmc_dpm_step: operands must be contiguous fp32, got {t.dtype} strides {t.stride()}")
    if (coef.dim() != 2 or coef.shape[1] != 5 or coef.shape[0] < 1 or coef.dtype != torch.float32
            or coef.device != x.device or not coef.is_contiguous()):
        raise L.DMCError(f"dmc_dpm_step: coef must be a contiguous fp32 [S, 5] tensor on {x.device}, got "
                         f"{coef.dtype} {tuple(coef.shape)} on {coef.device}")
    check(LIB.dmc_dpm_step(ptr(x), ptr(eps), ptr(x0), ptr(x0_prev), ptr(step), ptr(coef), coef.shape[0], N,
                           x.numel() // N, int(clip), ptr(out), ptr(x0_out), L.stream()), "dmc_dpm_step")
    return out, x0_out


def known_blend(x, x0, mask, row, coef, z=None, z2=None, out=None):
    """Known-region blend (dmc_known_blend): row[n] picks sample n's row {ka, kb, ra, rb} of the [R, 4] table
    (diffusion/_edit.py); out = ra * (mask * (ka*x0 + kb*z) + (1 - mask) * x) + rb*z2. mask: x's shape, or x's with
    one channel ([N, 1, ...]: shared by the channels). z / z2 may be None when no row has kb / rb != 0; out may be x."""
    what = "dmc_known_blend"
    if out is None:
        out = torch.empty_like(x)
    if not x.is_cuda or x.dim() < 1 or x.numel() < 1:
        raise L.DMCError(f"{what}: x must be a non-empty device tensor, got {tuple(x.shape)} on {x.device}")
    N = x.shape[0]
    per = x.numel() // N
    _same(x, x0, z, z2, out, what=what)
    if row is None:
        raise L.DMCError(f"{what}: needs a row index")
    _steps(N, x.device, row, what=what)
    shared = x.dim() >= 2 and tuple(mask.shape) == (N, 1) + tuple(x.shape[2:])
    if mask.device != x.device or not (mask.shape == x.shape or shared):
        raise L.DMCError(f"{what}: mask {tuple(mask.shape)} on {mask.device} is neither {tuple(x.shape)} nor that "
                         f"with one channel on {x.device}")
    _fp32_contig(what, x, x0, mask, z, z2, out)
    if (coef.dim() != 2 or coef.shape[1] != 4 or coef.shape[0] < 1 or coef.dtype != torch.float32
            or coef.device != x.device or not coef.is_contiguous()):
        raise L.DMCError(f"{what}: coef must be a contiguous fp32 [R, 4] tensor on {x.device}, got "
                         f"{coef.dtype} {tuple(coef.shape)} on {coef.device}")
    check(LIB.dmc_known_blend(ptr(x), ptr(x0), ptr(mask), mask.numel() // N, ptr(z), ptr(z2), ptr(row), ptr(coef),
                              coef.shape[0], N, per, ptr(out), L.stream()), what)
    return out


def cfg_x0(x, ec, eu, scale, t, ta, tb, mode, p_threshold, out=None):
    """(eps, x0) of the guided step; out: the two buffers to fill (allocated if None)."""
    N = x.shape[0]
    eps, x0 = out if out is not None else (torch.empty_like(x), torch.empty_like(x))
    _same(x, ec, eu, eps, x0, what="dmc_cfg_x0")
    _steps(N, x.device, t, what="dmc_cfg_x0")
    p = float(p_threshold) if p_threshold is not None else -1.0
    check(LIB.dmc_cfg_x0(ptr(x), ptr(ec), ptr(eu), float(scale), ptr(t), ptr(ta), ptr(tb), int(mode), N,
                         x.numel() // N, p, ptr(eps), ptr(x0), L.stream()), "dmc_cfg_x0")
    return eps, x0


def _row_stride(what, rows, ref):
    """Row stride, in floats, of rows: ref's shape on ref's device, fp32, every sample's elements contiguous and the
    samples a fixed, non-overlapping pitch apart (a contiguous tensor, or a view of some rows and the leading channels
    of a larger one, read in place)."""
    if rows is None or rows.shape != ref.shape or rows.device != ref.device or rows.dtype != torch.float32:
        got = "None" if rows is None else f"{rows.dtype} {tuple(rows.shape)} on {rows.device}"
        raise L.DMCError(f"{what}: a prediction is {got}, expected fp32 {tuple(ref.shape)} on {ref.device}")
    per = ref.numel() // ref.shape[0]
    ld = rows.stride(0) if rows.shape[0] > 1 else per
    if not rows[0].is_contiguous() or ld < per:
        raise L.DMCError(f"{what}: a prediction's samples must each be contiguous and at least {per} floats apart, got "
                         f"strides {rows.stride()}")
    return ld


def cfg_guide(pred_type, x, pc, pu, scale, rescale, t, sa, s1, p_threshold, want_eps=True, out=None):
    """(eps or None, x0) of the guided step from the model's own output (dmc_cfg_guide): guidance, the guidance rescale
    of arXiv:2305.08891 (rescale in [0, 1], 0: none), the conversion of either prediction type and the dynamic
    threshold. pc / pu: the conditional / unconditional predictions, x's shape, contiguous or row-strided views (the
    halves of the 2B-row model output, or of a learned_range output's prediction channels) read in place. out: the
    (eps, x0) buffers to fill; eps None or want_eps=False skips eps."""
    what = "dmc_cfg_guide"
    code = _pred_code(what, pred_type)
    if not x.is_cuda or x.dim() < 1 or x.numel() < 1:
        raise L.DMCError(f"{what}: x must be a non-empty device tensor, got {tuple(x.shape)} on {x.device}")
    N = x.shape[0]
    ldc, ldu = _row_stride(what, pc, x), _row_stride(what, pu, x)
    if out is not None:
        eps, x0 = out
    else:
        eps, x0 = (torch.empty_like(x) if want_eps else None), torch.empty_like(x)
    if x0 is None:
        raise L.DMCError(f"{what}: the x0 buffer is not optional")
    _same(x, eps, x0, what=what)
    _fp32_contig(what, x, eps, x0)
    _steps(N, x.device, t, what=what)
    T = _tables(what, x.device, sa, s1)
    if t is None or T is None or sa is None or s1 is None:
        raise L.DMCError(f"{what}: needs timesteps and the sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod tables")
    if not 0.0 <= float(rescale) <= 1.0:
        raise L.DMCError(f"{what}: rescale {rescale!r} is not in [0, 1]")
    p = float(p_threshold) if p_threshold is not None else -1.0
    check(LIB.dmc_cfg_guide(code, ptr(x), ptr(pc), ldc, ptr(pu), ldu, float(scale), float(rescale), ptr(t), ptr(sa),
                            ptr(s1), T, N, x.numel() // N, p, ptr(eps), ptr(x0), L.stream()), what)
    return eps, x0


def _flow_coef(what, coef, dev):
    if (coef is None or coef.dim() != 2 or coef.shape[1] != 4 or coef.shape[0] < 1 or coef.dtype != torch.float32
            or coef.device != dev or not coef.is_contiguous()):
        got = "None" if coef is None else f"{coef.dtype} {tuple(coef.shape)} on {coef.device}"
        raise L.DMCError(f"{what}: coef must be a contiguous fp32 [R, 4] tensor on {dev}, got {got}")
    return coef.shape[0]


def flow_step(x, pc, step, coef, pu=None, scale=1.0, xb=None, dprev=None, out=None, xb_out=None, d_out=None):
    """Rectified-flow ODE update (dmc_flow_step): step[n] picks sample n's row {sigma, h, hh, kind} of the [R, 4] table
    (diffusion/_flow.py). pc / pu: the conditional / unconditional velocities, x's shape, contiguous or row-strided views
    (the halves of the 2B-row model output) read in place; pu None: no guidance. xb / dprev: the Heun history a corrector
    row reads, xb_out / d_out: where a predictor row leaves it (either may be the tensor it replaces; None: not written).
    out may be x. Returns out."""
    what = "dmc_flow_step"
    if x is None or not x.is_cuda or x.dim() < 1 or x.numel() < 1:
        got = "None" if x is None else f"{tuple(x.shape)} on {x.device}"
        raise L.DMCError(f"{what}: x must be a non-empty device tensor, got {got}")
    N = x.shape[0]
    ldc = _row_stride(what, pc, x)
    ldu = _row_stride(what, pu, x) if pu is not None else 0
    if out is None:
        out = torch.empty_like(x)
    _same(x, xb, dprev, out, xb_out, d_out, what=what)
    _fp32_contig(what, x, xb, dprev, out, xb_out, d_out)
    if step is None:
        raise L.DMCError(f"{what}: needs a step index")
    _steps(N, x.device, step, what=what)
    R = _flow_coef(what, coef, x.device)
    check(LIB.dmc_flow_step(ptr(x), ptr(pc), ldc, ptr(pu), ldu, float(scale), ptr(xb), ptr(dprev), ptr(step), ptr(coef),
                            R, N, x.numel() // N, ptr(out), ptr(xb_out), ptr(d_out), L.stream()), what)
    return out


def flow_guide(x, pc, pu, scale, rescale, step, coef, threshold=False, p_threshold=None, out=None):
    """Guided velocity of a rectified flow (dmc_flow_guide) with the guidance rescale of arXiv:2305.08891 (rescale in
    [0, 1], 0: none) and, with threshold=True, the dynamic threshold on the data prediction x - sigma*g (p_threshold in
    (0, 1): quantile, None: clamp to +-1). pc / pu as flow_step; out must not be x. Returns out, flow_step's pc."""
    what = "dmc_flow_guide"
    if x is None or not x.is_cuda or x.dim() < 1 or x.numel() < 1:
        got = "None" if x is None else f"{tuple(x.shape)} on {x.device}"
        raise L.DMCError(f"{what}: x must be a non-empty device tensor, got {got}")
    N = x.shape[0]
    ldc, ldu = _row_stride(what, pc, x), _row_stride(what, pu, x)
    if out is None:
        out = torch.empty_like(x)
    _same(x, out, what=what)
    _fp32_contig(what, x, out)
    if out.data_ptr() == x.data_ptr():
        raise L.DMCError(f"{what}: out must not be x")
    if step is None:
        raise L.DMCError(f"{what}: needs a step index")
    _steps(N, x.device, step, what=what)
    R = _flow_coef(what, coef, x.device)
    if not 0.0 <= float(rescale) <= 1.0:
        raise L.DMCError(f"{what}: rescale {rescale!r} is not in [0, 1]")
    p = float(p_threshold) if p_threshold is not None else -1.0
    check(LIB.dmc_flow_guide(ptr(x), ptr(pc), ldc, ptr(pu), ldu, float(scale), float(rescale), ptr(step), ptr(coef), R,
                             N, x.numel() // N, int(bool(threshold)), p, ptr(out), L.stream()), what)
    return out


class TensorRefs:
    """Device array of dmc_tensor_ref {a, b, n} for the multi-tensor kernels (uploaded once per pointer set)."""

    def __init__(self, pairs, device):
        self.key = tuple((a.data_ptr(), b.data_ptr() if b is not None else 0, a.numel()) for a, b in pairs)
        arr = (L.TensorRef * len(pairs))()
        for i, (a, b) in enumerate(pairs):
            arr[i].a = a.data_ptr()
            arr[i].b = b.data_ptr() if b is not None else None
            arr[i].n = a.numel()
        host = torch.frombuffer(bytearray(arr), dtype=torch.uint8)
        self.dev = host.to(device)
        self.count = len(pairs)


def ema_update(refs: TensorRefs, decay):
    check(LIB.dmc_ema_update(ptr(refs.dev), refs.count, float(decay), L.stream()), "dmc_ema_update")


def clip_grad_norm(refs: TensorRefs, max_norm):
    total = torch.empty((), dtype=torch.float32, device=refs.dev.device)
    ws = SCRATCH.get((16 * refs.count + 16) * 4, refs.dev.device)
    check(LIB.dmc_clip_grad_norm(ptr(refs.dev), refs.count, float(max_norm), ptr(total), ptr(ws), L.stream()),
          "dmc_clip_grad_norm")
    return total


def grad_norm_flat(g, max_norm):
    """(total_norm, clip coef) of a flat fp32 gradient buffer, both device scalars; no host sync."""
    out = torch.empty(2, dtype=torch.float32, device=g.device)
    ws = SCRATCH.get(1024 * 4, g.device)   # one partial per dmc_grad_norm_flat block
    check(LIB.dmc_grad_norm_flat(ptr(g), g.numel(), float(max_norm), ptr(out), out.data_ptr() + 4, ptr(ws),
                                 L.stream()), "dmc_grad_norm_flat")
    return out[0], out[1:]


def adamw_flat(p, g, m, v, ema, coef, wd_mul, lerp_w, beta2, omb2, eps, neg_step, bc2_sqrt, ema_decay, ema_om):
    check(LIB.dmc_adamw_flat(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), p.numel(), ptr(coef), wd_mul, lerp_w, beta2,
                             omb2, eps, neg_step, bc2_sqrt, ema_decay, ema_om, L.stream()), "dmc_adamw_flat")


def adamw_flat_dev(p, g, m, v, ema, coef, hyper):
    """adamw_flat with the nine scalars (same order as adamw_flat's) read from the fp32 device tensor hyper."""
    check(LIB.dmc_adamw_flat_dev(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), p.numel(), ptr(coef), ptr(hyper),
                                 L.stream()), "dmc_adamw_flat_dev")


# ---- DiT token-wise kernels (csrc/dmc_dit.hip) ----------------------------------------------------------------
def _mod_ptr(mod, off):
    """Device address of column `off` of the stacked modulation rows [B][ld_mod] (fp32)."""
    return None if mod is None else mod.data_ptr() + 4 * off


def ln_mod_fwd(dtype, x, T, C, L_, mod, ld_mod, off_shift, off_scale, eps, h, ld_h, mean, rstd, br=None, ld_br=0,
               off_gate=0, drop=None, x_out=None):
    seed, seed_base, thresh, scale = drop_args(drop)
    check(LIB.dmc_ln_mod_fwd(L.dtype_code(dtype), ptr(x), ptr(br), ld_br, _mod_ptr(mod, off_gate) if br is not None
                             else None, _mod_ptr(mod, off_shift), _mod_ptr(mod, off_scale), ld_mod, T, C, L_,
                             float(eps), seed, seed_base, thresh, scale, ptr(x_out), ptr(h), ld_h, ptr(mean),
                             ptr(rstd), L.stream()), "dmc_ln_mod_fwd")


def _rowsum_ws(T, C, L_, dev):
    n = LIB.dmc_dit_rowsum_workspace(T // L_, C, L_)
    return SCRATCH.get(n, dev) if n else None


def ln_mod_bwd(dtype, dh, ld_dh, x, mean, rstd, mod, ld_mod, off_scale, T, C, L_, dx, dmod, off_dscale, off_dshift):
    ws = _rowsum_ws(T, C, L_, dx.device)
    check(LIB.dmc_ln_mod_bwd(L.dtype_code(dtype), ptr(dh), ld_dh, ptr(x), ptr(mean), ptr(rstd),
                             _mod_ptr(mod, off_scale), ld_mod, T, C, L_, ptr(dx), _mod_ptr(dmod, off_dscale),
                             _mod_ptr(dmod, off_dshift), ptr(ws), L.stream()), "dmc_ln_mod_bwd")


def gate_bwd(dtype, dy, br, ld_br, mod, ld_mod, off_gate, T, C, L_, dbr, ld_dbr, dmod, off_dgate, drop=None):
    seed, seed_base, thresh, scale = drop_args(drop)
    ws = _rowsum_ws(T, C, L_, dy.device)
    check(LIB.dmc_gate_bwd(L.dtype_code(dtype), ptr(dy), ptr(br), ld_br, _mod_ptr(mod, off_gate), ld_mod, T, C, L_,
                           seed, seed_base, thresh, scale, ptr(dbr), ld_dbr, _mod_ptr(dmod, off_dgate), ptr(ws),
                           L.stream()), "dmc_gate_bwd")


def gelu_fwd(dtype, u, rows, C, ld, a, drop=None):
    seed, seed_base, thresh, scale = drop_args(drop)
    check(LIB.dmc_gelu_fwd(L.dtype_code(dtype), ptr(u), rows, C, ld, seed, seed_base, thresh, scale, ptr(a),
                           L.stream()), "dmc_gelu_fwd")


def gelu_bwd(dtype, da, u, rows, C, ld, du, drop=None):
    seed, seed_base, thresh, scale = drop_args(drop)
    check(LIB.dmc_gelu_bwd(L.dtype_code(dtype), ptr(da), ptr(u), rows, C, ld, seed, seed_base, thresh, scale, ptr(du),
                           L.stream()), "dmc_gelu_bwd")


def timestep_embedding(t, dim, out, max_period=10000.0):
    _steps(t.shape[0], out.device, t, what="dmc_timestep_embedding")
    check(LIB.dmc_timestep_embedding(ptr(t), t.shape[0], dim, float(max_period), ptr(out), L.stream()),
          "dmc_timestep_embedding")


def unpatchify(src, ld_src, B, ht, wt, p, C, out):
    check(LIB.dmc_unpatchify(ptr(src), ld_src, B, ht, wt, p, C, ptr(out), L.stream()), "dmc_unpatchify")


def patchify_grad(dtype, dout, B, ht, wt, p, C, out, ld_out):
    check(LIB.dmc_patchify_grad(L.dtype_code(dtype), ptr(dout), B, ht, wt, p, C, ptr(out), ld_out, L.stream()),
          "dmc_patchify_grad")


def add_bcast(x, v, rows, n):
    check(LIB.dmc_add_bcast(ptr(x), ptr(v), rows, n, L.stream()), "dmc_add_bcast")


def batch_sum(x, rows, n, out):
    check(LIB.dmc_batch_sum(ptr(x), rows, n, ptr(out), L.stream()), "dmc_batch_sum")


def patch_dgrad(dtok, ld, w, B, ht, wt, p, C, H, dx):
    check(LIB.dmc_patch_dgrad(ptr(dtok), ld, ptr(w), B, ht, wt, p, C, H, ptr(dx), L.stream()), "dmc_patch_dgrad")


# ---- DiM: affine LayerNorm + modulation (csrc/dmc_dit.hip), the Mamba mixer (csrc/dmc_mamba.hip) ----------------
def ln_affine_mod_fwd(dtype, x, T, C, L_, mod, ld_mod, off_shift, off_scale, eps, gamma, beta, h, ld_h, mean, rstd,
                      br=None, ld_br=0, off_gate=0, drop=None, x_out=None):
    seed, seed_base, thresh, scale = drop_args(drop)
    check(LIB.dmc_ln_affine_mod_fwd(L.dtype_code(dtype), ptr(x), ptr(br), ld_br, _mod_ptr(mod, off_gate)
                                    if br is not None else None, _mod_ptr(mod, off_shift), _mod_ptr(mod, off_scale),
                                    ld_mod, T, C, L_, float(eps), ptr(gamma), ptr(beta), seed, seed_base, thresh, scale,
                                    ptr(x_out), ptr(h), ld_h, ptr(mean), ptr(rstd), L.stream()),
          "dmc_ln_affine_mod_fwd")


def ln_affine_mod_bwd(dtype, dh, ld_dh, x, mean, rstd, mod, ld_mod, off_scale, T, C, L_, gamma, beta, dx, dmod,
                      off_dscale, off_dshift, dgamma, dbeta):
    ws = _rowsum_ws(T, C, L_, dx.device)
    check(LIB.dmc_ln_affine_mod_bwd(L.dtype_code(dtype), ptr(dh), ld_dh, ptr(x), ptr(mean), ptr(rstd),
                                    _mod_ptr(mod, off_scale), ld_mod, T, C, L_, ptr(gamma), ptr(beta), ptr(dx),
                                    _mod_ptr(dmod, off_dscale), _mod_ptr(dmod, off_dshift), ptr(dgamma), ptr(dbeta),
                                    ptr(ws), L.stream()), "dmc_ln_affine_mod_bwd")


def gate_bwd_bias(dtype, dy, br, ld_br, mod, ld_mod, off_gate, T, C, L_, dbr, ld_dbr, dmod, off_dgate, dbias,
                  drop=None):
    """gate_bwd, plus the fp32 gradient dbias [C] of the bias of the branch's last Linear."""
    seed, seed_base, thresh, scale = drop_args(drop)
    ws = _rowsum_ws(T, C, L_, dy.device)
    dsum = torch.empty(T // L_, ld_mod, dtype=torch.float32, device=dy.device)
    check(LIB.dmc_gate_bwd_bias(L.dtype_code(dtype), ptr(dy), ptr(br), ld_br, _mod_ptr(mod, off_gate), ld_mod, T, C,
                                L_, seed, seed_base, thresh, scale, ptr(dbr), ld_dbr, _mod_ptr(dmod, off_dgate),
                                ptr(dsum), ptr(dbias), ptr(ws), L.stream()), "dmc_gate_bwd_bias")


def gelu_bwd_f32in(dtype, da, u, rows, C, ld, du, drop=None):
    """gelu_bwd with da as fp32 rows."""
    seed, seed_base, thresh, scale = drop_args(drop)
    check(LIB.dmc_gelu_bwd_f32in(L.dtype_code(dtype), ptr(da), ptr(u), rows, C, ld, seed, seed_base, thresh, scale,
                                 ptr(du), L.stream()), "dmc_gelu_bwd_f32in")


def _col_ptr(t, col):
    """Device address of column `col` of the rows t [.., ld]."""
    return t.data_ptr() + col * t.element_size()


def causal_conv_silu_fwd(dtype, x, ld_x, w, bias, B, L_, E, u, ld_u, x_col=0):
    check(LIB.dmc_causal_conv_silu_fwd(L.dtype_code(dtype), _col_ptr(x, x_col), ld_x, ptr(w), ptr(bias), B, L_, E,
                                       ptr(u), ld_u, L.stream()), "dmc_causal_conv_silu_fwd")


def causal_conv_silu_bwd(dtype, du, ld_du, x, ld_x, w, bias, B, L_, E, dx, ld_dx, dw, dbias, x_col=0, dx_col=0):
    ws = SCRATCH.get(LIB.dmc_causal_conv_workspace(B, L_, E), du.device)
    check(LIB.dmc_causal_conv_silu_bwd(L.dtype_code(dtype), ptr(du), ld_du, _col_ptr(x, x_col), ld_x, ptr(w), ptr(bias),
                                       B, L_, E, _col_ptr(dx, dx_col), ld_dx, ptr(dw), ptr(dbias), ptr(ws), L.stream()),
          "dmc_causal_conv_silu_bwd")


def scan_chunk():
    return LIB.dmc_scan_chunk()


def scan_states(B, L_, E, N, device):
    """The chunk-entry state buffer selective_scan_fwd fills and selective_scan_bwd reads (None for one chunk)."""
    K_ = (L_ + scan_chunk() - 1) // scan_chunk()
    return torch.empty(B, K_, E, N, dtype=torch.float32, device=device) if K_ > 1 else None


def selective_scan_fwd(dtype, u, ld_u, z, ld_z, z_col, dpre, ld_dp, bc, ld_bc, b_col, c_col, A_log, D, dt_bias, B, L_,
                       E, N, states, y, ld_y):
    ws = SCRATCH.get(LIB.dmc_selective_scan_workspace(B, L_, E, N, 0), u.device) if states is not None else None
    check(LIB.dmc_selective_scan_fwd(L.dtype_code(dtype), ptr(u), ld_u, _col_ptr(z, z_col), ld_z, ptr(dpre), ld_dp,
                                     _col_ptr(bc, b_col), _col_ptr(bc, c_col), ld_bc, ptr(A_log), ptr(D), ptr(dt_bias),
                                     B, L_, E, N, ptr(states), ptr(ws), ptr(y), ld_y, L.stream()),
          "dmc_selective_scan_fwd")


def selective_scan_bwd(dtype, dy, ld_dy, u, ld_u, z, ld_z, z_col, dpre, ld_dp, bc, ld_bc, b_col, c_col, A_log, D,
                       dt_bias, B, L_, E, N, states, du, ld_du, dz, ld_dz, dz_col, ddpre, ld_ddp, dbc, ld_dbc, bc_col,
                       dA_log, dD):
    ws = SCRATCH.get(LIB.dmc_selective_scan_workspace(B, L_, E, N, 1), u.device)
    check(LIB.dmc_selective_scan_bwd(L.dtype_code(dtype), ptr(dy), ld_dy, ptr(u), ld_u, _col_ptr(z, z_col), ld_z,
                                     ptr(dpre), ld_dp, _col_ptr(bc, b_col), _col_ptr(bc, c_col), ld_bc, ptr(A_log),
                                     ptr(D), ptr(dt_bias), B, L_, E, N, ptr(states), ptr(ws), ptr(du), ld_du,
                                     _col_ptr(dz, dz_col), ld_dz, ptr(ddpre), ld_ddp, ptr(dbc), ld_dbc, bc_col,
                                     ptr(dA_log), ptr(dD), L.stream()), "dmc_selective_scan_bwd")


# ---- scan orders: the same ops over the h x w token grid walked in order `order` (a 3-bit code, models/dim.py) ----
def scan_order_token(order, h, w, p):
    """The token (row index within an image) at logical position p of the walk `order` over the h x w grid."""
    t = LIB.dmc_scan_order_token(order, h, w, p)
    if t < 0:
        raise L.DMCError(f"dmc_scan_order_token: order {order}, grid {h} x {w}, position {p}")
    return t


def causal_conv_silu_fwd_ord(dtype, x, ld_x, w, bias, B, h, wt, order, E, u, ld_u, x_col=0):
    check(LIB.dmc_causal_conv_silu_fwd_ord(L.dtype_code(dtype), _col_ptr(x, x_col), ld_x, ptr(w), ptr(bias), B, h, wt,
                                           order, E, ptr(u), ld_u, L.stream()), "dmc_causal_conv_silu_fwd_ord")


def causal_conv_silu_bwd_ord(dtype, du, ld_du, x, ld_x, w, bias, B, h, wt, order, E, dx, ld_dx, dw, dbias, x_col=0,
                             dx_col=0):
    ws = SCRATCH.get(LIB.dmc_causal_conv_workspace(B, h * wt, E), du.device)
    check(LIB.dmc_causal_conv_silu_bwd_ord(L.dtype_code(dtype), ptr(du), ld_du, _col_ptr(x, x_col), ld_x, ptr(w),
                                           ptr(bias), B, h, wt, order, E, _col_ptr(dx, dx_col), ld_dx, ptr(dw),
                                           ptr(dbias), ptr(ws), L.stream()), "dmc_causal_conv_silu_bwd_ord")


def selective_scan_fwd_ord(dtype, u, ld_u, z, ld_z, z_col, dpre, ld_dp, bc, ld_bc, b_col, c_col, A_log, D, dt_bias, B,
                           h, wt, order, E, N, states, y, ld_y):
    ws = SCRATCH.get(LIB.dmc_selective_scan_workspace(B, h * wt, E, N, 0), u.device) if states is not None else None
    check(LIB.dmc_selective_scan_fwd_ord(L.dtype_code(dtype), ptr(u), ld_u, _col_ptr(z, z_col), ld_z, ptr(dpre), ld_dp,
                                         _col_ptr(bc, b_col), _col_ptr(bc, c_col), ld_bc, ptr(A_log), ptr(D),
                                         ptr(dt_bias), B, h, wt, order, E, N, ptr(states), ptr(ws), ptr(y), ld_y,
                                         L.stream()), "dmc_selective_scan_fwd_ord")


def selective_scan_bwd_ord(dtype, dy, ld_dy, u, ld_u, z, ld_z, z_col, dpre, ld_dp, bc, ld_bc, b_col, c_col, A_log, D,
                           dt_bias, B, h, wt, order, E, N, states, du, ld_du, dz, ld_dz, dz_col, ddpre, ld_ddp, dbc,
                           ld_dbc, bc_col, dA_log, dD):
    ws = SCRATCH.get(LIB.dmc_selective_scan_workspace(B, h * wt, E, N, 1), u.device)
    check(LIB.dmc_selective_scan_bwd_ord(L.dtype_code(dtype), ptr(dy), ld_dy, ptr(u), ld_u, _col_ptr(z, z_col), ld_z,
                                         ptr(dpre), ld_dp, _col_ptr(bc, b_col), _col_ptr(bc, c_col), ld_bc, ptr(A_log),
                                         ptr(D), ptr(dt_bias), B, h, wt, order, E, N, ptr(states), ptr(ws), ptr(du),
                                         ld_du, _col_ptr(dz, dz_col), ld_dz, ptr(ddpre), ld_ddp, ptr(dbc), ld_dbc,
                                         bc_col, ptr(dA_log), ptr(dD), L.stream()), "dmc_selective_scan_bwd_ord")
