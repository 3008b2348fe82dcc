"""ge.tap_bwd_weight against float64 conv2d_weight: exact on dyadic inputs,
within the oracle's bound on random ones, and through autograd."""

import functools

import pytest
import torch

import conv_oracle
from mpi4dl_amd.ops import backend
from mpi4dl_amd.ops.conv_native import native_conv2d

pytestmark = pytest.mark.gpu

KERNELS = [(1, 7), (7, 1), (3, 3)]
# (N, C, K, H, W, pad mode); pixel tiles: 2x64 (1x7), 4x32 (7x1, 3x3)
SHAPES = [
    (2, 20, 24, 9, 17, "same"),     # C, K tails; odd W; patch > image
    (1, 72, 120, 10, 40, "same"),   # 2 C tiles, 2 K tiles, aligned, seams
    (3, 32, 16, 8, 8, "valid"),     # N = 3, OH or OW = 2
    (1, 40, 8, 12, 24, "full"),     # full padding
    (2, 16, 48, 21, 72, "same"),    # many pixel tiles: the run-length cases
]
IDS = ["n%dc%dk%d-%dx%d-%s" % s for s in SHAPES]
rs_id = lambda rs: "%dx%d" % rs


def _case(rs, s):
    (R, S), (N, C, K, H, W, mode) = rs, s
    m = {"same": 2, "valid": 0, "full": 4}[mode]   # pad = (size - 1) * m / 4
    ph, pw = (R - 1) * m // 4, (S - 1) * m // 4
    return conv_oracle.Case(f"tapw-{R}x{S}-" + IDS[SHAPES.index(s)], "autograd",
                            "tap+tap+tap_bwdw", C, K, H, W, R, S, ph=ph, pw=pw,
                            bias=True, N=N)


@functools.lru_cache(maxsize=None)
def _dyadic(c):
    """x, go: multiples of 1/4 in [-2, 2]; the float64 weight gradient. Every
    product is a multiple of 1/16 of at most 4 and N*OH*OW < 2^18, so every
    partial sum is exact in fp32 in any order."""
    assert c.N * c.OH * c.OW < 2 ** 18
    gen = torch.Generator().manual_seed(2)
    x = torch.randint(-8, 9, (c.N, c.C, c.H, c.W), generator=gen) / 4
    go = torch.randint(-8, 9, (c.N, c.K, c.OH, c.OW), generator=gen) / 4
    ref = torch.nn.grad.conv2d_weight(
        x.double(), (c.K, c.C, c.R, c.S), go.double(), padding=(c.ph, c.pw))
    return x.bfloat16().cuda(), go.bfloat16().cuda(), ref


@functools.lru_cache(maxsize=None)
def _random(c):
    inputs = conv_oracle.make_inputs(c)
    return inputs, conv_oracle.reference(c, *inputs)


def _bwdw(c, go, x, *extra):
    return backend.ext().tap_bwd_weight(go, x, c.R, c.S, c.ph, c.pw, *extra)


@pytest.mark.parametrize("s", SHAPES, ids=IDS)
@pytest.mark.parametrize("rs", KERNELS, ids=rs_id)
@pytest.mark.parametrize("prior", [False, True], ids=["fresh", "out"])
def test_exact_on_dyadic_inputs(rs, s, prior):
    """Fresh, or added into ``out`` pre-filled with dyadic values."""
    c = _case(rs, s)
    x, go, ref = _dyadic(c)
    gen = torch.Generator().manual_seed(3)
    g0 = torch.randint(-64, 65, ref.shape, generator=gen) / 16 * prior
    out = (g0.float().cuda(),) if prior else ()
    got = _bwdw(c, go, x, *out)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    assert not prior or got.data_ptr() == out[0].data_ptr()
    assert torch.equal(got.double().cpu(), g0.double() + ref)


@pytest.mark.parametrize("s", SHAPES, ids=IDS)
@pytest.mark.parametrize("rs", KERNELS, ids=rs_id)
def test_random_within_bound(rs, s):
    c = _case(rs, s)
    (x, w, b, go), ref = _random(c)
    got = _bwdw(c, go.cuda(), x.cuda())
    worst = conv_oracle.assert_within(
        got, *ref["gw"], conv_oracle.reduction_length(c, "gw"), False,
        what=c.name)
    print(f"err/bound {worst:.3f}")


@pytest.mark.parametrize("tpb", [1, 2, 5, 10 ** 6])
@pytest.mark.parametrize("rs", KERNELS, ids=rs_id)
def test_run_length(rs, tpb):
    c = _case(rs, SHAPES[4])
    x, go, ref = _dyadic(c)
    assert torch.equal(_bwdw(c, go, x, None, tpb).double().cpu(), ref)


@pytest.mark.parametrize("rs, s, sink", [
    (rs, s, False) for rs in KERNELS for s in SHAPES[:2]] + [
    ((1, 7), SHAPES[0], True)])
def test_autograd(rs, s, sink, monkeypatch):
    """Both switches. ``sink``: the weight sits behind the gradient sink with
    a prior g0, so w.grad is an fp32 sum, in some order, of g0 and the L
    products: the oracle's bound for L + 1 terms of magnitudes |g0| + A."""
    from mpi4dl_amd.ops.grad_sink import opt_in

    for name in ("MPI4DL_TAPCONV", "MPI4DL_TAPCONV_WGRAD", "MPI4DL_GRAD_SINK"):
        monkeypatch.setenv(name, "1")
    c = _case(rs, s)
    (x, w, b, go), ref = _random(c)
    xg, bg = x.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    wg = torch.nn.Parameter(w.cuda())
    g0 = torch.zeros_like(w)
    if sink:
        g0 = torch.randn(w.shape, generator=torch.Generator().manual_seed(4))
        wg.grad = g0.cuda()
        ptr = wg.grad.data_ptr()
        opt_in(wg)
    y = native_conv2d(xg, wg, bg, 1, (c.ph, c.pw))
    y.backward(go.cuda())
    ge = backend.ext()
    wb = w.bfloat16().cuda()
    assert torch.equal(y, ge.tap_fwd(x.cuda(), wb, b.cuda(), c.ph, c.pw))
    assert torch.equal(xg.grad, ge.tap_fwd(
        go.cuda(), wb, None, c.R - 1 - c.ph, c.S - 1 - c.pw, True))
    assert not sink or wg.grad.data_ptr() == ptr
    L = conv_oracle.reduction_length(c, "gw")
    r, A = ref["gw"]
    conv_oracle.assert_within(wg.grad, g0.double() + r, g0.double().abs() + A,
                              L + 1, False, what="gw")
    conv_oracle.assert_within(bg.grad, *ref["gb"], L, True, what="gb")


def test_unsupported_problems_are_errors():
    ge = backend.ext()
    x = torch.zeros(1, 8, 8, 8, device="cuda", dtype=torch.bfloat16)
    go = torch.zeros(1, 8, 8, 8, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="kernel size"):
        ge.tap_bwd_weight(go, x, 1, 5, 0, 2)
    with pytest.raises(RuntimeError, match="padding"):
        ge.tap_bwd_weight(go, x, 1, 7, 1, 3)
    with pytest.raises(RuntimeError, match="go is not the gradient"):
        ge.tap_bwd_weight(go, x, 1, 7, 0, 0)
