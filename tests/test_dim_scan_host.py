"""CPU tests of the DiM scan orders: the mapping (C library = models/dim.py = tests/scan_order_reference.py, and its
properties), pattern resolution, the refused configurations, and that an order changes nothing about the parameters.
An out-of-range row index in the _ord kernels would be a wild store: these run before anything runs on a GPU."""
import copy
import pickle

import pytest
import torch

from scan_order_reference import ORDERS, PATTERNS, order_token, permutation

GRIDS = [(h, w) for h in range(1, 10) for w in range(1, 10)]


def _dim(**kw):
    from diffusion_models_collection_amd.models import DiM
    return DiM(**kw)


def _perm(order, h, w):
    from diffusion_models_collection_amd.models.dim import scan_permutation
    return scan_permutation(order, h, w)


def test_order_names_are_the_codes():
    from diffusion_models_collection_amd.models import dim
    assert dim.SCAN_ORDERS == ORDERS and dict(dim.SCAN_PATTERNS) == PATTERNS
    for code, name in enumerate(ORDERS):
        assert bool(code & 1) == name.endswith("_rev")
        assert bool(code & 2) == ("col" in name) and bool(code & 4) == name.startswith("snake")
        assert torch.equal(_perm(name, 3, 5), _perm(code, 3, 5))


def test_c_mapping_equals_scan_permutation():
    """dmc_scan_order_token = scan_permutation = the definition written out in scan_order_reference, all 8 orders,
    1 <= h, w <= 9; out-of-range arguments give -1 (the wrapper raises)."""
    from diffusion_models_collection_amd import _lib as L
    from diffusion_models_collection_amd import kernels as K
    for code in range(8):
        for h, w in GRIDS:
            py = _perm(code, h, w)
            assert py.dtype == torch.long and py.shape == (h * w,)
            c = [L.LIB.dmc_scan_order_token(code, h, w, p) for p in range(h * w)]
            assert c == py.tolist() == [order_token(code, h, w, p) for p in range(h * w)], (code, h, w)
    assert K.scan_order_token(3, 2, 3, 0) == 5
    for bad in ((8, 2, 2, 0), (-1, 2, 2, 0), (0, 0, 2, 0), (0, 2, 0, 0), (0, 2, 2, 4), (0, 2, 2, -1)):
        assert L.LIB.dmc_scan_order_token(*bad) == -1
        with pytest.raises(L.DMCError, match="dmc_scan_order_token"):
            K.scan_order_token(*bad)


def test_c_mapping_on_large_grids():
    """The library divides by a host-computed reciprocal ((q * mul) >> shift): exact up to h * w = 2^31 - 1, at line
    boundaries and at random positions, for line lengths that are and are not powers of two."""
    import random
    from diffusion_models_collection_amd import _lib as L
    rng = random.Random(1)
    grids = [(1, 2 ** 31 - 1), (2 ** 31 - 1, 1), (46340, 46340), (3, 715827882), (715827882, 3), (65536, 32767),
             (32767, 65536), (2, 2 ** 30 - 1), (1000, 1000), (48, 48)]
    for h, w in grids:
        Lt = h * w
        ps = {0, 1, Lt - 1, Lt - 2, Lt // 2} | {rng.randrange(Lt) for _ in range(100)}
        for inner in (h, w):
            for k in (1, 2, 3, Lt // inner // 2, Lt // inner - 1):
                ps |= {q for q in (k * inner - 1, k * inner, k * inner + 1) if 0 <= q < Lt}
        ps |= {Lt - 1 - q for q in ps}
        for code in range(8):
            for p in ps:
                assert L.LIB.dmc_scan_order_token(code, h, w, p) == order_token(code, h, w, p), (code, h, w, p)
    assert L.LIB.dmc_scan_order_token(0, 65536, 32768, 0) == -1          # h * w = 2^31: refused


def test_mapping_properties():
    for h, w in GRIDS:
        Lt = h * w
        ident = torch.arange(Lt)
        for name in ORDERS:
            assert sorted(_perm(name, h, w).tolist()) == list(range(Lt)), (name, h, w)      # a permutation
        assert torch.equal(_perm("row", h, w), ident)
        assert torch.equal(_perm("row_rev", h, w), ident.flip(0))
        assert torch.equal(_perm("col", h, w), ident.view(h, w).t().reshape(-1))            # the transpose order
        for name in ("row", "col", "snake_row", "snake_col"):
            assert torch.equal(_perm(name + "_rev", h, w), _perm(name, h, w).flip(0))
        for name in ORDERS[4:]:                                                             # snake: always a neighbour
            p = _perm(name, h, w)
            i, j = p // w, p % w
            d = (i[1:] - i[:-1]).abs() + (j[1:] - j[:-1]).abs()
            assert bool((d == 1).all()), (name, h, w)
    assert _perm("snake_row", 3, 4).tolist() == [0, 1, 2, 3, 7, 6, 5, 4, 8, 9, 10, 11]
    assert _perm("snake_col", 3, 4).tolist() == [0, 4, 8, 9, 5, 1, 2, 6, 10, 11, 7, 3]
    # the reference helper's inverse
    perm, inv = permutation("snake_col_rev", 5, 7)
    assert torch.equal(perm[inv], torch.arange(35)) and torch.equal(perm, _perm("snake_col_rev", 5, 7))


def _codes(*names):
    return tuple(ORDERS.index(n) for n in names)


@pytest.mark.parametrize("depth", [1, 4, 6])
def test_pattern_resolution(depth):
    kw = dict(img_size=(8, 8), hidden_size=16, depth=depth, mixer="mamba")
    assert _dim(**kw).scan_orders == (0,) * depth                    # the default is "row"
    for scan, pat in PATTERNS.items():
        m = _dim(**kw, scan=scan)
        assert m.scan_orders == tuple(ORDERS.index(pat[i % len(pat)]) for i in range(depth)), scan
        assert m.scan == scan and isinstance(m.scan_orders, tuple)
        assert all(isinstance(c, int) for c in m.scan_orders)
    assert _dim(**dict(kw, depth=6), scan="cross").scan_orders == (0, 1, 2, 3, 0, 1)
    assert _dim(**dict(kw, depth=6), scan="zigzag").scan_orders == _codes(
        "snake_row", "snake_col", "snake_row_rev", "snake_col_rev", "snake_row", "snake_col")
    seq = [ORDERS[(3 * i + 5) % 8] for i in range(depth)]
    for s in (seq, tuple(seq)):
        m = _dim(**kw, scan=s)
        assert m.scan_orders == _codes(*seq) and m.scan == tuple(seq)
    assert _dim(**kw, scan="row").executor.scan_orders == (0,) * depth
    assert _dim(**kw, scan=seq).executor.scan_orders == _codes(*seq)


def test_scan_errors():
    from diffusion_models_collection_amd._lib import DMCError
    kw = dict(img_size=(8, 8), hidden_size=64, depth=2)
    for bad in ("diagonal", ["row", "hilbert"], 3):
        with pytest.raises(DMCError, match="scan"):
            _dim(**kw, mixer="mamba", scan=bad)
    for bad in (["row"], ["row", "col", "row_rev"], ()):
        with pytest.raises(DMCError, match=r"scan.*depth 2"):
            _dim(**kw, mixer="mamba", scan=bad)
    for bad in ("cross", "bidir", ["row", "col"]):
        with pytest.raises(DMCError, match=r"attention.*scan.*no token order"):
            _dim(**kw, mixer="attention", scan=bad)
    assert _dim(**kw, mixer="attention", scan="row").scan_orders == (0, 0)
    assert _dim(**kw, mixer="attention", scan=["row", "row"]).scan_orders == (0, 0)


def test_scan_adds_no_parameters():
    """DiM(scan="cross") has the keys, shapes and seeded values of DiM() built from the same seed."""
    kw = dict(img_size=(8, 12), hidden_size=40, depth=4, num_classes=10, mixer="mamba")
    torch.manual_seed(77)
    a = _dim(**kw).state_dict()
    torch.manual_seed(77)
    b = _dim(**kw, scan="cross").state_dict()
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    m = _dim(**kw, scan="zigzag")
    m.load_state_dict(a)                                  # a checkpoint of the default order loads


def test_scan_orders_survive_pickle_and_deepcopy():
    m = _dim(img_size=(8, 8), hidden_size=16, depth=5, mixer="mamba", scan="zigzag")
    want = m.scan_orders
    assert want == (4, 6, 5, 7, 4)
    for c in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        assert c.scan_orders == want and c.scan == "zigzag" and c.executor.scan_orders == want
