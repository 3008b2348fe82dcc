"""GPU tests for the vectorised 2-byte pooling kernels (gemscore.hip).

The fast path must be bit-identical to the generic kernels, which the
bindings still reach through ``force_generic=True``; the generic kernels
are checked against PyTorch in tests/test_gpu.py. Stride-2 geometries
only take the fast path when W is a multiple of 16 (OW % 8 == 0), so each
listed shape is also run at twice its width for them.
"""

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

pytestmark = [gpu, requires_gpu]

DTYPES = [torch.bfloat16, torch.float16]
MAX_GEOMS = [(3, 1, 1), (3, 2, 1), (2, 2, 0)]

# (N, C, H, W): H shorter than a strip and one chunk holding both edges;
# ragged last strip with first/interior/last chunks; one full wave per
# row; a row spanning a wave boundary. Odd plane counts put plane
# boundaries inside a block's thread range.
SHAPES_S1 = [
    (1, 3, 1, 8), (1, 3, 2, 8), (1, 3, 3, 8),
    (2, 3, 5, 16), (1, 3, 9, 24),
    (2, 5, 16, 64),
    (1, 2, 16, 136),
]
_BASE_S2 = [
    (1, 3, 2, 8), (1, 3, 4, 8),
    (2, 3, 5, 16), (1, 3, 9, 24),
    (2, 5, 16, 64),
    (1, 2, 16, 136),
]
SHAPES_S2 = _BASE_S2 + [(n, c, h, 2 * w) for (n, c, h, w) in _BASE_S2]


def _shapes(s):
    return SHAPES_S1 if s == 1 else SHAPES_S2


def _ext():
    from mpi4dl_amd.ops import backend

    return backend.ext()


def _out_hw(h, w, k, s, p):
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def _max_both(x, go, k, s, p):
    """(y, idx, gi) from the fast path and from the generic kernels."""
    ge = _ext()
    h, w = x.shape[-2:]
    out = []
    for force in (False, True):
        y, idx = ge.maxpool_fwd(x, k, s, p, force_generic=force)
        gi = ge.maxpool_bwd(go, idx, h, w, k, s, p, force_generic=force)
        out.append((y, idx, gi))
    torch.cuda.synchronize()
    return out


MAX_CASES = [(g, sh) for g in MAX_GEOMS for sh in _shapes(g[1])]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("geom,shape", MAX_CASES, ids=lambda v: "x".join(map(str, v)))
def test_maxpool_fast_equals_generic(geom, shape, dtype):
    k, s, p = geom
    n, c, h, w = shape
    oh, ow = _out_hw(h, w, k, s, p)
    torch.manual_seed(0)
    x = torch.randn(n, c, h, w, device="cuda").to(dtype)
    go = torch.randn(n, c, oh, ow, device="cuda").to(dtype)
    (y, idx, gi), (yg, idxg, gig) = _max_both(x, go, k, s, p)
    assert torch.equal(y, yg)
    assert torch.equal(idx, idxg)
    assert torch.equal(gi, gig)


def _tie_input(kind, dtype):
    torch.manual_seed(1)
    shape = (2, 3, 9, 32)
    if kind == "constant":
        x = torch.full(shape, 1.5, device="cuda")
    elif kind == "ties":
        x = torch.randint(0, 3, shape, device="cuda").float()
    elif kind == "negative":
        x = -torch.rand(shape, device="cuda") - 0.5
    else:  # isolated -inf entries: no window is -inf throughout
        x = torch.randn(shape, device="cuda")
        x[..., ::3, ::3] = float("-inf")
    return x.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["constant", "ties", "negative", "neg_inf"])
@pytest.mark.parametrize("geom", MAX_GEOMS, ids=lambda v: "x".join(map(str, v)))
def test_maxpool_ties_and_padding(geom, kind, dtype):
    k, s, p = geom
    x = _tie_input(kind, dtype)
    oh, ow = _out_hw(x.shape[2], x.shape[3], k, s, p)
    # small integers: every gradient sum is exact in fp32 and in `dtype`,
    # so the order in which PyTorch accumulates cannot show
    go = torch.randint(-4, 5, (2, 3, oh, ow), device="cuda").to(dtype)
    (y, idx, gi), (yg, idxg, gig) = _max_both(x, go, k, s, p)
    assert torch.equal(y, yg)
    assert torch.equal(idx, idxg)
    assert torch.equal(gi, gig)
    xf = x.float().requires_grad_(True)
    yr = F.max_pool2d(xf, k, s, padding=p)
    (gr,) = torch.autograd.grad(yr, xf, go.float())
    assert torch.equal(y, yr.detach().to(dtype))
    assert torch.equal(gi, gr.to(dtype))


def _avg_geoms(h, w):
    # plain, and the tile as the bottom-right quarter of a 2H x 2W image
    # (p = 1): only the bottom and right borders are image borders
    return [(-1, -1, h, w), (h - 1, w - 1, 2 * h, 2 * w)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("include_pad", [True, False])
@pytest.mark.parametrize("shape", SHAPES_S1, ids=lambda v: "x".join(map(str, v)))
def test_avgpool_fast_equals_generic(shape, include_pad, dtype):
    ge = _ext()
    n, c, h, w = shape
    torch.manual_seed(2)
    x = torch.randn(n, c, h, w, device="cuda").to(dtype)
    go = torch.randn(n, c, h, w, device="cuda").to(dtype)
    for gr0, gc0, hg, wg in _avg_geoms(h, w):
        args = (3, 1, 1, gr0, gc0, hg, wg, include_pad)
        y = ge.avgpool_fwd(x, *args)
        yg = ge.avgpool_fwd(x, *args, force_generic=True)
        gi = ge.avgpool_bwd(go, h, w, *args)
        gig = ge.avgpool_bwd(go, h, w, *args, force_generic=True)
        torch.cuda.synchronize()
        assert torch.equal(y, yg), (gr0, gc0)
        assert torch.equal(gi, gig), (gr0, gc0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("include_pad", [True, False])
def test_avgpool_fast_matches_torch(include_pad, dtype):
    """One rounding of an fp32 sum: within half a spacing of `dtype`
    (2^-8 relative for bf16, 2^-11 for fp16) of the fp32 reference, plus
    the few fp32 ulps by which two summation orders can differ. The bound
    used is twice the half spacing."""
    ge = _ext()
    torch.manual_seed(3)
    x = torch.randn(2, 3, 9, 32, device="cuda").to(dtype)
    y = ge.avgpool_fwd(x, 3, 1, 1, -1, -1, 9, 32, include_pad)
    ref = F.avg_pool2d(x.float(), 3, 1, padding=1, count_include_pad=include_pad)
    rtol = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    assert torch.allclose(y.float(), ref, rtol=rtol, atol=1e-6)


@pytest.mark.parametrize(
    "shape,dtype",
    [((1, 2, 5, 12), torch.float32), ((2, 3, 8, 16), torch.float32)],
    ids=["ragged_fp32", "fastshape_fp32"],
)
def test_fallback_matches_torch(shape, dtype):
    """W % 8 != 0 and fp32 keep the generic kernels (tolerances of
    tests/test_gpu.py)."""
    from mpi4dl_amd.ops.native import native_avgpool, native_maxpool

    torch.manual_seed(4)
    for k, s, p in MAX_GEOMS:
        x = torch.randn(*shape, device="cuda", dtype=dtype, requires_grad=True)
        x2 = x.detach().clone().requires_grad_(True)
        y = native_maxpool(x, k, s, p)
        y_ref = F.max_pool2d(x2, k, s, padding=p)
        assert torch.allclose(y, y_ref, atol=1e-6)
        g = torch.randn_like(y)
        y.backward(g)
        y_ref.backward(g)
        assert torch.allclose(x.grad, x2.grad, atol=1e-5)
    for include_pad in (True, False):
        x = torch.randn(*shape, device="cuda", dtype=dtype, requires_grad=True)
        x2 = x.detach().clone().requires_grad_(True)
        y = native_avgpool(x, 3, 1, 1, include_pad=include_pad)
        y_ref = F.avg_pool2d(x2, 3, 1, padding=1, count_include_pad=include_pad)
        assert torch.allclose(y, y_ref, atol=1e-5)
        g = torch.randn_like(y)
        y.backward(g)
        y_ref.backward(g)
        assert torch.allclose(x.grad, x2.grad, atol=1e-5)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_fallback_ragged_two_byte(dtype):
    """A 2-byte input with W % 8 != 0 must fall back, not fault. Max is
    exact; the gradient uses small integers so its sums are exact too."""
    from mpi4dl_amd.ops.native import native_maxpool

    torch.manual_seed(5)
    for k, s, p in MAX_GEOMS:
        x = torch.randn(1, 2, 5, 12, device="cuda").to(dtype).requires_grad_(True)
        xf = x.detach().float().requires_grad_(True)
        y = native_maxpool(x, k, s, p)
        yr = F.max_pool2d(xf, k, s, padding=p)
        assert torch.equal(y.detach(), yr.detach().to(dtype))
        g = torch.randint(-4, 5, y.shape, device="cuda").to(dtype)
        (gi,) = torch.autograd.grad(y, x, g)
        (gr,) = torch.autograd.grad(yr, xf, g.float())
        assert torch.equal(gi, gr.to(dtype))


STRIDED_CASES = [
    ((2, 3, 8, 16), torch.bfloat16),   # fast path
    ((2, 3, 8, 32), torch.float16),    # fast path for the stride-2 pools too
    ((2, 3, 5, 12), torch.bfloat16),   # generic: ragged width
    ((2, 3, 8, 16), torch.float32),    # generic: fp32
]


@pytest.mark.parametrize(
    "shape,dtype", STRIDED_CASES,
    ids=["fast_bf16", "fast_fp16_w32", "ragged_bf16", "fp32"],
)
def test_strided_gradient(shape, dtype):
    """A channel slice of a wider gradient goes to the kernels as it is
    and gives what its repacked copy gives."""
    from mpi4dl_amd.ops.native import native_avgpool, native_maxpool

    ge = _ext()
    n, c, h, w = shape
    torch.manual_seed(6)
    for k, s, p in MAX_GEOMS:
        oh, ow = _out_hw(h, w, k, s, p)
        big = torch.randn(n, 9, oh, ow, device="cuda").to(dtype)
        go = big[:, 2:5]
        assert not go.is_contiguous()
        x = torch.randn(*shape, device="cuda").to(dtype).requires_grad_(True)
        y = native_maxpool(x, k, s, p)
        (g1,) = torch.autograd.grad(y, x, go, retain_graph=True)
        (g2,) = torch.autograd.grad(y, x, go.contiguous())
        assert torch.equal(g1, g2)
        # the bindings take the slice directly, on both paths
        _, idx = ge.maxpool_fwd(x.detach(), k, s, p)
        for force in (False, True):
            d1 = ge.maxpool_bwd(go, idx, h, w, k, s, p, force_generic=force)
            assert torch.equal(d1, g2)
    big = torch.randn(n, 9, h, w, device="cuda").to(dtype)
    go = big[:, 2:5]
    for include_pad in (True, False):
        x = torch.randn(*shape, device="cuda").to(dtype).requires_grad_(True)
        y = native_avgpool(x, 3, 1, 1, include_pad=include_pad)
        (g1,) = torch.autograd.grad(y, x, go, retain_graph=True)
        (g2,) = torch.autograd.grad(y, x, go.contiguous())
        assert torch.equal(g1, g2)
        for force in (False, True):
            d1 = ge.avgpool_bwd(go, h, w, 3, 1, 1, -1, -1, h, w, include_pad,
                                force_generic=force)
            assert torch.equal(d1, g2)


def test_kernel_size_check():
    ge = _ext()
    x = torch.randn(1, 1, 20, 20, device="cuda")
    with pytest.raises(RuntimeError):
        ge.maxpool_fwd(x, 17, 1, 8)
    idx = torch.zeros(1, 1, 20, 20, device="cuda", dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ge.maxpool_bwd(x, idx, 20, 20, 17, 1, 8)
