"""The tap-shift conv kernel (ge.tap_fwd) for 1x7, 7x1 and 3x3 against
float64 direct convolution: exactly on dyadic inputs, within the oracle's
bound on random ones, through autograd and the module, and run to run."""

import functools

import pytest
import torch
import torch.nn.functional as F

import conv_oracle
from mpi4dl_amd.ops import backend
from mpi4dl_amd.ops.conv_native import NativeConv2d, native_conv2d

pytestmark = pytest.mark.gpu

KERNELS = [(1, 7), (7, 1), (3, 3)]
# (N, C, K, H, W, pad mode, bias); tiles: 4x64 (1x7), 8x32 (7x1, 3x3)
SHAPES = [
    (2, 20, 24, 9, 17, "same", True),     # C, K tails; odd W; patch > image
    (1, 72, 120, 10, 40, "same", True),   # 3 chunks, 2 M tiles, aligned, seams
    (3, 32, 16, 8, 8, "valid", True),     # exact chunk, N = 3, OH or OW = 2
    (2, 104, 104, 20, 72, "same", False),  # MF = 7, 3.25 chunks, no bias
    (1, 40, 8, 12, 24, "full", True),     # full padding, MF = 2
    (2, 16, 48, 5, 64, "same", True),     # W = one 1x7 tile, 16-byte stores
]
IDS = ["n%dc%dk%d-%dx%d-%s" % s[:6] for s in SHAPES]
PADS = {"same": lambda R, S: (R // 2, S // 2), "valid": lambda R, S: (0, 0),
        "full": lambda R, S: (R - 1, S - 1)}


def _case(rs, s):
    (R, S), (N, C, K, H, W, mode, bias) = rs, s
    ph, pw = PADS[mode](R, S)
    return conv_oracle.Case(f"tap-{R}x{S}-" + IDS[SHAPES.index(s)], "autograd",
                            "tap+tap+conv_bwdw", C, K, H, W, R, S, ph=ph,
                            pw=pw, bias=bias, N=N)


def _run(c, transposed, x, w, b, go):
    """ge.tap_fwd on the GPU, the float64 reference of the same leg and the
    same operation on absolute values."""
    ge = backend.ext()
    wg = w.bfloat16().cuda()
    pad = (c.ph, c.pw)
    if transposed:
        got = ge.tap_fwd(go.bfloat16().cuda(), wg, None, c.R - 1 - c.ph,
                         c.S - 1 - c.pw, True)
        op = lambda x, w, b, go: torch.nn.grad.conv2d_input(
            [c.N, c.C, c.H, c.W], w, go, padding=pad)
    else:
        bg = None if b is None else b.cuda()
        got = ge.tap_fwd(x.bfloat16().cuda(), wg, bg, c.ph, c.pw)
        op = lambda x, w, b, go: F.conv2d(x, w, b, padding=pad)
    d = lambda t: None if t is None else t.double()
    a = lambda t: None if t is None else t.double().abs()
    return (got.cpu(), op(d(x), d(w), d(b), d(go)),
            op(a(x), a(w), a(b), a(go)))


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("s", SHAPES, ids=IDS)
@pytest.mark.parametrize("rs", KERNELS, ids=lambda rs: "%dx%d" % rs)
def test_exact_on_dyadic_inputs(rs, s, transposed):
    c = _case(rs, s)
    gen = torch.Generator().manual_seed(1)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=gen)
    x = ri(-8, 9, c.N, c.C, c.H, c.W) / 4
    w = ri(-8, 9, c.K, c.C, c.R, c.S) / 8
    b = ri(-16, 17, c.K) / 8 if c.bias else None
    go = ri(-8, 9, c.N, c.K, c.OH, c.OW) / 4
    got, ref, _ = _run(c, transposed, x, w, b, go)
    assert got.dtype == torch.bfloat16
    assert torch.equal(got, ref.bfloat16())


@functools.lru_cache(maxsize=None)
def _random_inputs(c):
    return conv_oracle.make_inputs(c)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("s", SHAPES, ids=IDS)
@pytest.mark.parametrize("rs", KERNELS, ids=lambda rs: "%dx%d" % rs)
def test_random_within_bound(rs, s, transposed):
    c = _case(rs, s)
    x, w, b, go = _random_inputs(c)
    got, ref, A = _run(c, transposed, x, w, b, go)
    L = c.K * c.R * c.S if transposed else c.C * c.R * c.S + int(c.bias)
    worst = conv_oracle.assert_within(
        got, ref, A, L, out_is_bf16=True, what=f"tap {c.name} T={transposed}")
    print(f"err/bound {worst:.3f}")


@pytest.mark.parametrize("s", SHAPES[:2], ids=IDS[:2])
@pytest.mark.parametrize("rs", KERNELS, ids=lambda rs: "%dx%d" % rs)
def test_autograd(rs, s, monkeypatch):
    monkeypatch.setenv("MPI4DL_TAPCONV", "1")
    c = _case(rs, s)
    x, w, b, go = _random_inputs(c)
    ge = backend.ext()
    xg = x.cuda().requires_grad_(True)
    wg = w.cuda().requires_grad_(True)
    bg = b.cuda().requires_grad_(True)
    y = native_conv2d(xg, wg, bg, 1, (c.ph, c.pw))
    y.backward(go.cuda())
    wb = w.bfloat16().cuda()
    assert torch.equal(y, ge.tap_fwd(x.cuda(), wb, b.cuda(), c.ph, c.pw))
    assert torch.equal(xg.grad, ge.tap_fwd(
        go.cuda(), wb, None, c.R - 1 - c.ph, c.S - 1 - c.pw, True))
    ref = conv_oracle.reference(c, x, w, b, go)
    for leg, got in (("gw", wg.grad), ("gb", bg.grad)):
        conv_oracle.assert_within(
            got, *ref[leg], conv_oracle.reduction_length(c, leg),
            conv_oracle.leg_is_bf16(leg), what=leg)


def test_module(monkeypatch):
    monkeypatch.setenv("MPI4DL_TAPCONV", "1")
    torch.manual_seed(0)
    conv = NativeConv2d(20, 24, (1, 7), padding=(0, 3))
    x = torch.randn(2, 20, 9, 17)
    assert torch.equal(conv(x),
                       F.conv2d(x, conv.weight, conv.bias, padding=(0, 3)))
    y = conv.cuda()(x.bfloat16().cuda())
    assert torch.equal(y, backend.ext().tap_fwd(
        x.bfloat16().cuda(), conv.weight.bfloat16(), conv.bias.float(), 0, 3))


@pytest.mark.parametrize("rs", KERNELS, ids=lambda rs: "%dx%d" % rs)
def test_deterministic(rs):
    c = _case(rs, SHAPES[1])
    inputs = _random_inputs(c)
    for transposed in (False, True):
        assert torch.equal(_run(c, transposed, *inputs)[0],
                           _run(c, transposed, *inputs)[0])


def test_unsupported_problems_are_errors():
    ge = backend.ext()
    x = torch.zeros(1, 8, 8, 8, device="cuda", dtype=torch.bfloat16)
    w = torch.zeros(8, 8, 1, 7, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="padding"):
        ge.tap_fwd(x, w, None, 1, 3)
    with pytest.raises(RuntimeError, match="kernel size"):
        ge.tap_fwd(x, w[:, :, :, :5].contiguous(), None, 0, 0)
    with pytest.raises(RuntimeError, match="channel mismatch"):
        ge.tap_fwd(x, w[:, :4].contiguous(), None, 0, 3)
