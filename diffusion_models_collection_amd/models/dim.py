"""DiM (Diffusion Mamba) with the reference's API and parameter layout, executed by gfx950 HIP kernels.

Drop-in for models/dim.py of sunyzhi55/Diffusion_Models_Collection:
  * same classes (PatchEmbed :20, TimestepEmbedder :38, LabelEmbedder :66, MambaBlock :94, FeedForward :146,
    DiMBlock :176, FinalLayer :189, DiM :208), the same constructor arguments and nn.Module tree, built in the same
    order and re-initialised by the same initialize_weights (:276-298);
  * DiM.forward(x[B,C,H,W] f32, t[B] i64, y[B] i64 | None) -> [B,C,H,W] f32 (:314-346).

The reference chooses the token mixer of MambaBlock by whether `mamba_ssm` imports on the host (:11-17, :103-117):
mamba_ssm.Mamba(d_model, d_state, d_conv=4, expand=2), else nn.MultiheadAttention(hidden, 8 heads). The two have
different state_dicts, so here the choice is explicit: mixer="mamba" | "attention" (in a config: the key 'mixer' of
model_params); without it the constructor raises NotImplementedError and says how to choose.

  * mixer="attention": the reference's fallback exactly (checked against fixtures the reference itself produced).
  * mixer="mamba": `blocks.i.mamba_block.mamba` is a module with mamba_ssm.Mamba's parameters -- A_log, D,
    in_proj.weight, conv1d.{weight,bias}, x_proj.weight, dt_proj.{weight,bias}, out_proj.weight -- and the selective
    state-space recurrence of DESIGN.md §3c runs on the dmc_mamba.hip kernels. mamba_ssm is not a dependency: the key
    list, the RNG order of its own initialisation and parity with its fused kernels beyond that recurrence are
    unverified.

The modules are parameter containers; the arithmetic is `_dim_exec.DiMExecutor` on libdmc.so.
Extra (optional) constructor arguments: compute_dtype = "fp32" | "bf16" (as models/unet.py), mixer, scan.

scan (mixer="mamba" only, not in the reference): the order in which each block's causal conv and selective scan walk
the h x w patch grid. The reference walks every block in row-major order, so information only ever flows forward
along that one path; DiM (Teng et al., arXiv:2405.14224) and ZigMa (Hu et al., arXiv:2403.13802) change the order from
block to block instead, with no extra parameters. An order is a 3-bit code (bit 0 reverse, bit 1 column-major, bit 2
snake: every other line walked backwards, so consecutive tokens are always grid neighbours), named in SCAN_ORDERS;
scan is a pattern name of SCAN_PATTERNS, cycled over the blocks, or a sequence of `depth` order names. "row" (the
default) is the reference's behaviour, bit for bit. The kernels walk the order in place; the
state_dict does not change.
"""
import math
from typing import Tuple

import torch
import torch.nn as nn

from .dit import LabelEmbedder, PatchEmbed, TimestepEmbedder, _KernelOnly
from .unet import _resolve_dtype

_MIXERS = ("mamba", "attention")
# scan orders by name: the index is the code (bit 0 reverse, bit 1 column-major, bit 2 snake)
SCAN_ORDERS = ("row", "row_rev", "col", "col_rev", "snake_row", "snake_row_rev", "snake_col", "snake_col_rev")
SCAN_PATTERNS = {
    "row": ("row",),
    "bidir": ("row", "row_rev"),
    "cross": ("row", "row_rev", "col", "col_rev"),                                # DiM's four sweeps
    "zigzag": ("snake_row", "snake_col", "snake_row_rev", "snake_col_rev"),       # after ZigMa
}
_ATTN_HEADS = 8     # the reference's fallback: nn.MultiheadAttention(hidden, num_heads=8) (dim.py:112-117)


def DMCError(msg):
    from .._lib import DMCError as E    # _lib loads libdmc.so: only when there is something to report
    return E(msg)


class Mamba(_KernelOnly, nn.Module):
    """Parameter container with the state_dict of mamba_ssm.Mamba(d_model, d_state, d_conv=4, expand=2): E = 2 *
    d_model inner channels, dt_rank = ceil(d_model / 16). A_log = log(1..d_state) in every row, D = 1; conv1d keeps
    torch's default init; the Linears are re-initialised by DiM.initialize_weights (dt_proj.bias included)."""

    def __init__(self, d_model, d_state=16, d_conv=4, expand=2):
        super().__init__()
        self.d_model, self.d_state, self.d_conv, self.expand = d_model, d_state, d_conv, expand
        self.d_inner = expand * d_model
        self.dt_rank = math.ceil(d_model / 16)
        E = self.d_inner
        self.in_proj = nn.Linear(d_model, 2 * E, bias=False)
        self.conv1d = nn.Conv1d(E, E, d_conv, groups=E, padding=d_conv - 1, bias=True)
        self.x_proj = nn.Linear(E, self.dt_rank + 2 * d_state, bias=False)
        self.dt_proj = nn.Linear(self.dt_rank, E, bias=True)
        A = torch.arange(1, d_state + 1, dtype=torch.float32).repeat(E, 1)
        self.A_log = nn.Parameter(torch.log(A))
        self.D = nn.Parameter(torch.ones(E))
        self.out_proj = nn.Linear(E, d_model, bias=False)


class MambaBlock(_KernelOnly, nn.Module):
    """Affine LayerNorm + modulation -> token mixer -> gated residual (dim.py:94-143)."""

    def __init__(self, hidden_size, state_size=16, dropout=0.1, mixer="mamba"):
        super().__init__()
        self.norm = nn.LayerNorm(hidden_size, eps=1e-6)
        if mixer == "mamba":
            self.mamba = Mamba(d_model=hidden_size, d_state=state_size, d_conv=4, expand=2)
        else:
            self.mamba = nn.MultiheadAttention(hidden_size, num_heads=_ATTN_HEADS, dropout=dropout, batch_first=True)
        self.adaLN_modulation = nn.Sequential(
            nn.SiLU(),
            nn.Linear(hidden_size, 3 * hidden_size, bias=True)
        )


class FeedForward(_KernelOnly, nn.Module):
    """Affine LayerNorm + modulation -> MLP -> gated residual (dim.py:146-173)."""

    def __init__(self, hidden_size, mlp_ratio=4.0, dropout=0.1):
        super().__init__()
        self.norm = nn.LayerNorm(hidden_size, eps=1e-6)
        mlp_hidden_dim = int(hidden_size * mlp_ratio)
        self.mlp = nn.Sequential(
            nn.Linear(hidden_size, mlp_hidden_dim),
            nn.GELU(),
            nn.Dropout(dropout),
            nn.Linear(mlp_hidden_dim, hidden_size),
            nn.Dropout(dropout)
        )
        self.adaLN_modulation = nn.Sequential(
            nn.SiLU(),
            nn.Linear(hidden_size, 3 * hidden_size, bias=True)
        )


class DiMBlock(_KernelOnly, nn.Module):
    """MambaBlock then FeedForward (dim.py:176-186)."""

    def __init__(self, hidden_size, state_size=16, mlp_ratio=4.0, dropout=0.1, mixer="mamba"):
        super().__init__()
        self.mamba_block = MambaBlock(hidden_size, state_size, dropout, mixer)
        self.ff_block = FeedForward(hidden_size, mlp_ratio, dropout)


class FinalLayer(_KernelOnly, nn.Module):
    """Affine LayerNorm + modulation -> Linear(hidden, p*p*C) (dim.py:189-205)."""

    def __init__(self, hidden_size, patch_size, out_channels):
        super().__init__()
        self.norm_final = nn.LayerNorm(hidden_size, eps=1e-6)
        self.linear = nn.Linear(hidden_size, patch_size * patch_size * out_channels, bias=True)
        self.adaLN_modulation = nn.Sequential(
            nn.SiLU(),
            nn.Linear(hidden_size, 2 * hidden_size, bias=True)
        )


def _resolve_mixer(mixer):
    if mixer is None:
        raise NotImplementedError(
            "DiM: choose the token mixer. The reference builds MambaBlock with mamba_ssm.Mamba when `mamba_ssm` "
            "imports on the host and with nn.MultiheadAttention(hidden, 8 heads) when it does not; the two have "
            "different state_dicts, so this port does not guess. Pass mixer='mamba' or mixer='attention' (in a config: "
            "model_params['mixer']).")
    if mixer not in _MIXERS:
        raise DMCError(f"DiM: mixer {mixer!r} (one of {_MIXERS})")
    return mixer


def _order_code(order):
    if isinstance(order, str):
        if order not in SCAN_ORDERS:
            raise DMCError(f"DiM: scan order {order!r} (one of {SCAN_ORDERS})")
        return SCAN_ORDERS.index(order)
    if isinstance(order, bool) or not isinstance(order, int) or not 0 <= order < len(SCAN_ORDERS):
        raise DMCError(f"DiM: scan order {order!r} (a name of {SCAN_ORDERS} or its code 0..7)")
    return order


def scan_permutation(order, h, w):
    """LongTensor perm [h*w]: perm[p] = the token (row-major index i*w + j) at logical position p of the order (a name
    of SCAN_ORDERS or its code) over the h x w grid. x[:, perm] are the tokens in walking order; the C library's
    dmc_scan_order_token is the same mapping."""
    code = _order_code(order)
    if h < 1 or w < 1:
        raise DMCError(f"DiM: scan_permutation over a {h} x {w} grid")
    Lt = h * w
    p = torch.arange(Lt, dtype=torch.long)
    q = Lt - 1 - p if code & 1 else p
    inner = h if code & 2 else w
    a, b = q // inner, q % inner
    if code & 4:
        b = torch.where(a % 2 == 1, inner - 1 - b, b)
    i, j = (b, a) if code & 2 else (a, b)
    return i * w + j


def resolve_scan(scan, depth, mixer="mamba"):
    """scan (a pattern name of SCAN_PATTERNS or a sequence of `depth` order names) -> the tuple of per-block codes."""
    if isinstance(scan, str):
        if scan not in SCAN_PATTERNS:
            raise DMCError(f"DiM: scan {scan!r} (a pattern of {tuple(SCAN_PATTERNS)}, or a sequence of one order name "
                           f"of {SCAN_ORDERS} per block)")
        pat = SCAN_PATTERNS[scan]
        codes = tuple(SCAN_ORDERS.index(pat[i % len(pat)]) for i in range(depth))
    else:
        try:
            names = list(scan)
        except TypeError:
            raise DMCError(f"DiM: scan {scan!r} (a pattern of {tuple(SCAN_PATTERNS)}, or a sequence of one order "
                           "name per block)") from None
        if len(names) != depth:
            raise DMCError(f"DiM: scan gives {len(names)} orders for depth {depth} (one per block)")
        try:
            codes = tuple(_order_code(n) for n in names)
        except RuntimeError as e:
            raise DMCError(f"DiM: scan {names!r}: {e}") from None
    if mixer == "attention" and any(codes):
        raise DMCError(f"DiM(mixer='attention'): scan {scan!r}; attention has no token order to change (every token "
                       "attends to every other, and the position embedding is all that tells them apart): scan must "
                       "be 'row'")
    return codes


class DiM(nn.Module):
    """Diffusion Mamba (dim.py:208-346); the reference's arguments plus compute_dtype, mixer and scan."""

    def __init__(
        self,
        img_size: Tuple[int, int] = (32, 32),
        patch_size=2,
        in_channels=3,
        hidden_size=768,
        depth=12,
        state_size=16,
        mlp_ratio=4.0,
        num_classes=None,
        dropout=0.1,
        compute_dtype=None,
        mixer=None,
        learn_sigma=False,
        scan="row",
    ):
        mixer = _resolve_mixer(mixer)
        scan_orders = resolve_scan(scan, depth, mixer)
        dt = _resolve_dtype(compute_dtype)
        if isinstance(img_size, int):
            img_size = (img_size, img_size)
        if mixer == "attention":
            hd, mult = hidden_size // _ATTN_HEADS, 8 if dt == torch.bfloat16 else 4
            if hidden_size % _ATTN_HEADS or hd > 64 or hd % mult:
                raise DMCError(f"DiM(mixer='attention'): hidden_size {hidden_size} gives {_ATTN_HEADS} heads of dim "
                               f"{hidden_size / _ATTN_HEADS:g}; the attention kernels take a head dim of at most 64 "
                               f"that is a multiple of {mult} (4 for fp32, 8 for bf16)")
        else:
            if state_size != 16:
                raise DMCError(f"DiM(mixer='mamba'): state_size {state_size}; the selective-scan kernels hold one "
                               "state per lane of a 16-lane row and support state_size 16 only")
            if hidden_size % 8:
                raise DMCError(f"DiM(mixer='mamba'): hidden_size {hidden_size} must be a multiple of 8")
        super().__init__()
        self.img_size = tuple(img_size)
        self.patch_size = patch_size
        self.in_channels = in_channels
        # not in the reference: a variance head (the original DiT's learn_sigma) doubles the final projection; the
        # output is [B, 2C, H, W], the prediction then v (diffusion variance_type='learned_range')
        self.learn_sigma = bool(learn_sigma)
        self.out_channels = 2 * in_channels if self.learn_sigma else in_channels
        self.hidden_size = hidden_size
        self.state_size = state_size
        self.num_classes = num_classes
        self.dropout = dropout
        self.mlp_ratio = mlp_ratio
        self.mixer = mixer
        self.scan = scan if isinstance(scan, str) else tuple(SCAN_ORDERS[c] for c in scan_orders)
        self.scan_orders = scan_orders     # per block: the 3-bit code the mixer kernels get (0 = the reference's order)
        self.num_heads = _ATTN_HEADS
        self.compute_dtype = dt

        self.x_embedder = PatchEmbed(self.img_size, patch_size, in_channels, hidden_size)
        num_patches = self.x_embedder.num_patches
        self.h_tokens = self.x_embedder.h_tokens
        self.w_tokens = self.x_embedder.w_tokens
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches, hidden_size))
        self.t_embedder = TimestepEmbedder(hidden_size)
        if num_classes is not None:
            self.y_embedder = LabelEmbedder(num_classes, hidden_size, dropout_prob=0.0)
        else:
            self.y_embedder = None
        self.blocks = nn.ModuleList([
            DiMBlock(hidden_size, state_size, mlp_ratio, dropout, mixer)
            for _ in range(depth)
        ])
        self.final_layer = FinalLayer(hidden_size, patch_size, self.out_channels)
        self.initialize_weights()
        self._executor = None

    def initialize_weights(self):
        # the reference's order (dim.py:276-298): xavier on every nn.Linear of the tree (Mamba's projections and
        # dt_proj.bias included: the reference's init does not honour Mamba's _no_reinit), pos_embed ~ N(0, 0.02),
        # every adaLN projection and the final projection zeroed
        def _basic_init(module):
            if isinstance(module, nn.Linear):
                torch.nn.init.xavier_uniform_(module.weight)
                if module.bias is not None:
                    nn.init.constant_(module.bias, 0)
        self.apply(_basic_init)
        nn.init.normal_(self.pos_embed, std=0.02)
        for block in self.blocks:
            nn.init.constant_(block.mamba_block.adaLN_modulation[-1].weight, 0)
            nn.init.constant_(block.mamba_block.adaLN_modulation[-1].bias, 0)
            nn.init.constant_(block.ff_block.adaLN_modulation[-1].weight, 0)
            nn.init.constant_(block.ff_block.adaLN_modulation[-1].bias, 0)
        nn.init.constant_(self.final_layer.adaLN_modulation[-1].weight, 0)
        nn.init.constant_(self.final_layer.adaLN_modulation[-1].bias, 0)
        nn.init.constant_(self.final_layer.linear.weight, 0)
        nn.init.constant_(self.final_layer.linear.bias, 0)

    @property
    def executor(self):
        if self._executor is None:
            from ._dim_exec import DiMExecutor
            self._executor = DiMExecutor(self)
        return self._executor

    def set_compute_dtype(self, compute_dtype):
        dt = _resolve_dtype(compute_dtype)
        if self.mixer == "attention" and dt == torch.bfloat16 and (self.hidden_size // _ATTN_HEADS) % 8:
            raise DMCError(f"DiM(mixer='attention'): head dim {self.hidden_size // _ATTN_HEADS} must be a multiple of "
                           "8 for bf16")
        self.compute_dtype = dt
        self._executor = None

    def unpatchify(self, x):
        """(B, N, p*p*C) -> (B, C, H, W) (dim.py:300-312), on the device kernel."""
        from .. import kernels as K
        B = x.shape[0]
        p, h, w, C = self.patch_size, self.h_tokens, self.w_tokens, self.out_channels
        out = torch.empty(B, C, h * p, w * p, dtype=torch.float32, device=x.device)
        K.unpatchify(x.contiguous().float(), p * p * C, B, h, w, p, C, out)
        return out

    def forward(self, x, t, y=None):
        if not x.is_cuda:
            raise RuntimeError("DiM runs on the MI355X HIP kernels only: move the model and inputs to a cuda device")
        return self.executor.run(x, t, y if self.num_classes is not None else None)

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_executor"] = None
        return st
