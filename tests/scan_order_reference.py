"""Test reference -- never imported by the product path.

Scan orders of the DiM Mamba mixer as "permute the tokens, run the existing reference, un-permute": the semantics
the _ord kernels of csrc/dmc_mamba.hip and DiM(scan=...) are held to. The mapping is written out here from its
definition (a 3-bit code: bit 0 reverse, bit 1 column-major, bit 2 snake), independently of models/dim.py and of the C
library; tests/test_dim_scan_host.py holds the three equal.
"""
import torch

from dim_reference import DiMReference
from mamba_reference import causal_conv_silu, selective_scan

ORDERS = ("row", "row_rev", "col", "col_rev", "snake_row", "snake_row_rev", "snake_col", "snake_col_rev")
PATTERNS = {"row": ("row",), "bidir": ("row", "row_rev"), "cross": ("row", "row_rev", "col", "col_rev"),
            "zigzag": ("snake_row", "snake_col", "snake_row_rev", "snake_col_rev")}


def order_token(code, h, w, p):
    """The token (row-major index) at logical position p of order `code` over the h x w grid."""
    reverse, column, snake = code & 1, code & 2, code & 4
    q = h * w - 1 - p if reverse else p
    inner = h if column else w
    a, b = divmod(q, inner)
    if snake and a & 1:
        b = inner - 1 - b
    i, j = (b, a) if column else (a, b)
    return i * w + j


def permutation(order, h, w):
    """(perm, inv) LongTensors: x[:, perm] are the tokens in walking order, y[:, inv] puts them back."""
    code = ORDERS.index(order) if isinstance(order, str) else order
    perm = torch.tensor([order_token(code, h, w, p) for p in range(h * w)], dtype=torch.long)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(h * w)
    return perm, inv


def pattern_codes(scan, depth):
    if isinstance(scan, str):
        pat = PATTERNS[scan]
        return tuple(ORDERS.index(pat[i % len(pat)]) for i in range(depth))
    return tuple(ORDERS.index(n) for n in scan)


def causal_conv_silu_ord(x, w, b, order, h, wt):
    perm, inv = permutation(order, h, wt)
    return causal_conv_silu(x[:, perm], w, b)[:, inv]


def selective_scan_ord(u, z, dpre, Bm, Cm, A_log, D, dt_bias, order, h, w):
    perm, inv = permutation(order, h, w)
    return selective_scan(u[:, perm], z[:, perm], dpre[:, perm], Bm[:, perm], Cm[:, perm], A_log, D, dt_bias)[:, inv]


class DiMScanReference(DiMReference):
    """DiMReference with a scan order per block. Everything in a block but the mixer's conv and scan is per token, so
    permuting the block's input and un-permuting its output is the order's whole effect."""

    def __init__(self, sd, scan="row", **cfg):
        super().__init__(sd, **cfg)
        self.codes = pattern_codes(scan, self.depth)

    def block(self, i, x, c):
        perm, inv = permutation(self.codes[i], self.ht, self.wt)
        return super().block(i, x[:, perm], c)[:, inv]


def make_scan_reference(state_dict, cfg, dtype=torch.float32, requires_grad=False, **kw):
    sd = {k: v.detach().to(dtype).cpu().clone().requires_grad_(requires_grad) for k, v in state_dict.items()}
    cfg = {k: v for k, v in cfg.items() if k != "compute_dtype"}
    return DiMScanReference(sd, **cfg, **kw), sd
