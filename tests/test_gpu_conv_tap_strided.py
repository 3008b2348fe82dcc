"""The strided tap-shift kernels (ge.tap_fwd_strided, ge.tap_bwd_data_strided)
for 1x7 at stride (1, 2), 7x1 at (2, 1) and 3x3 at (2, 2) against float64
direct convolution: exactly on dyadic inputs, within the oracle's bound on
random ones, through autograd and the module, and run to run."""

import functools

import pytest
import torch
import torch.nn.functional as F

import conv_oracle
from mpi4dl_amd.ops import backend
from mpi4dl_amd.ops.conv_native import NativeConv2d

pytestmark = pytest.mark.gpu

KERNELS = [(1, 7), (7, 1), (3, 3)]
# (N, C, K, H, W, pad mode, bias, x and go start 2 bytes off 16-byte alignment)
# tiles (output pixels, and go pixels of the data-grad): 4x64 (1x7), 8x32
# (7x1), 4x32 (3x3)
SHAPES = [
    (2, 20, 24, 9, 17, "same", True, False),     # C, K tails; odd W
    (1, 72, 120, 20, 136, "same", True, False),  # 3 chunks, 2 K tiles, seams
    (3, 32, 16, 10, 24, "valid", True, False),   # N = 3; last row/col unreached
    # MF = 7, no bias; OW = 72 for 1x7 and 3x3: go staged by 16-byte loads,
    # 4 chunks of K, column seams
    (2, 104, 104, 20, 144, "same", False, False),
    (1, 40, 8, 12, 25, "full", True, False),     # full padding, MF = 2
    (2, 16, 48, 7, 64, "valid", True, True),     # W % 8 == 0, unaligned base
]
IDS = ["n%dc%dk%d-%dx%d-%s" % s[:6] for s in SHAPES]
PADS = {"same": lambda R, S: (R // 2, S // 2), "valid": lambda R, S: (0, 0),
        "full": lambda R, S: (R - 1, S - 1)}


def _case(rs, s):
    (R, S), (N, C, K, H, W, mode, bias, _) = rs, s
    ph, pw = PADS[mode](R, S)
    return conv_oracle.Case(f"tap-s2-{R}x{S}-" + IDS[SHAPES.index(s)],
                            "autograd", "tap_s+tap_s+conv_bwdw", C, K, H, W, R,
                            S, sh=min(R, 2), sw=min(S, 2), ph=ph, pw=pw,
                            bias=bias, N=N)


def _gpu(t, off=False):
    """t as bf16 on the GPU; ``off``: starting 2 bytes past an aligned base."""
    if not off:
        return t.bfloat16().cuda()
    buf = torch.empty(t.numel() + 1, dtype=torch.bfloat16, device="cuda")
    return buf[1:].view(t.shape).copy_(t)


def _run(c, transposed, x, w, b, go, off=False):
    """The binding on the GPU, the float64 reference of the same leg and the
    same operation on absolute values."""
    ge = backend.ext()
    wg = w.bfloat16().cuda()
    st, pad = (c.sh, c.sw), (c.ph, c.pw)
    if transposed:
        got = ge.tap_bwd_data_strided(_gpu(go, off), wg, c.H, c.W, *st, *pad)
        op = lambda x, w, b, go: torch.nn.grad.conv2d_input(
            [c.N, c.C, c.H, c.W], w, go, stride=st, padding=pad)
    else:
        bg = None if b is None else b.cuda()
        got = ge.tap_fwd_strided(_gpu(x, off), wg, bg, *st, *pad)
        op = lambda x, w, b, go: F.conv2d(x, w, b, stride=st, padding=pad)
    d = lambda t: None if t is None else t.double()
    a = lambda t: None if t is None else t.double().abs()
    return (got.cpu(), op(d(x), d(w), d(b), d(go)),
            op(a(x), a(w), a(b), a(go)))


@functools.lru_cache(maxsize=None)
def _dyadic_inputs(c):
    """x, go: integers / 4; w, b: integers / 8. Every sum of products is a
    multiple of 1/32 far below 2^24 / 32: exact in fp32 in any order."""
    gen = torch.Generator().manual_seed(1)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=gen)
    x = ri(-8, 9, c.N, c.C, c.H, c.W) / 4
    w = ri(-8, 9, c.K, c.C, c.R, c.S) / 8
    b = ri(-16, 17, c.K) / 8 if c.bias else None
    go = ri(-8, 9, c.N, c.K, c.OH, c.OW) / 4
    return x, w, b, go


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("s", SHAPES, ids=IDS)
@pytest.mark.parametrize("rs", KERNELS, ids=lambda rs: "%dx%d" % rs)
def test_exact_on_dyadic_inputs(rs, s, transposed):
    c = _case(rs, s)
    got, ref, _ = _run(c, transposed, *_dyadic_inputs(c), s[7])
    # the fp32 sum is exact, so the one rounding to bf16 is the reference's
    assert torch.equal(ref.float().double(), ref)
    assert got.dtype == torch.bfloat16
    assert torch.equal(got, ref.bfloat16())
    if transposed and s[5] == "valid":
        # rows / columns past the last filter position (10x24: one of each
        # for every filter that strides that way): exact zeros
        hr = (c.OH - 1) * c.sh + c.R
        wr = (c.OW - 1) * c.sw + c.S
        assert not got[:, :, hr:].any() and not got[:, :, :, wr:].any()


@functools.lru_cache(maxsize=None)
def _random_inputs(c):
    return conv_oracle.make_inputs(c)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("s", SHAPES, ids=IDS)
@pytest.mark.parametrize("rs", KERNELS, ids=lambda rs: "%dx%d" % rs)
def test_random_within_bound(rs, s, transposed):
    c = _case(rs, s)
    x, w, b, go = _random_inputs(c)
    got, ref, A = _run(c, transposed, x, w, b, go, s[7])
    # data-grad: the most (k, tap) terms a phase sums
    L = (c.K * -(-c.R // c.sh) * -(-c.S // c.sw) if transposed
         else c.C * c.R * c.S + int(c.bias))
    worst = conv_oracle.assert_within(
        got, ref, A, L, out_is_bf16=True, what=f"{c.name} T={transposed}")
    print(f"err/bound {worst:.3f}")


@pytest.mark.parametrize("rs, sink", [(rs, False) for rs in KERNELS]
                         + [((3, 3), True)])
def test_module_autograd(rs, sink, monkeypatch):
    """NativeConv2d under both switches: y and x.grad are the bindings', and
    w.grad is what the same module gives with the second switch unset (with
    ``sink``: added into a prior gradient behind the gradient sink). On the
    dyadic inputs: conv_bwd_weight adds its (image, row) slices with atomicAdd
    in any order, and only exact sums are the same bits in every order."""
    from mpi4dl_amd.ops.grad_sink import opt_in

    for name in ("MPI4DL_TAPCONV", "MPI4DL_NATIVE_CONV", "MPI4DL_GRAD_SINK"):
        monkeypatch.setenv(name, "1")
    c = _case(rs, SHAPES[0])
    x, w, b, go = _dyadic_inputs(c)
    x, go = x.bfloat16(), go.bfloat16()
    ge = backend.ext()
    g0 = torch.randint(-64, 65, w.shape) / 8

    def step(strided):
        monkeypatch.setenv("MPI4DL_TAPCONV_STRIDED", "1" if strided else "0")
        conv = NativeConv2d(c.C, c.K, (c.R, c.S), stride=(c.sh, c.sw),
                            padding=(c.ph, c.pw)).cuda()
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(b)
        if sink:
            conv.weight.grad = g0.cuda()
            opt_in(conv.weight)
        xg = x.cuda().requires_grad_(True)
        y = conv(xg)
        y.backward(go.cuda())
        return y.detach(), xg.grad, conv.weight.grad

    y, gx, gw = step(True)
    wb = w.bfloat16().cuda()
    assert torch.equal(y, ge.tap_fwd_strided(
        x.cuda(), wb, b.cuda(), c.sh, c.sw, c.ph, c.pw))
    assert torch.equal(gx, ge.tap_bwd_data_strided(
        go.cuda(), wb, c.H, c.W, c.sh, c.sw, c.ph, c.pw))
    assert torch.equal(gw, step(False)[2])


@pytest.mark.parametrize("rs", KERNELS, ids=lambda rs: "%dx%d" % rs)
def test_deterministic(rs):
    c = _case(rs, SHAPES[3])
    inputs = _random_inputs(c)
    for transposed in (False, True):
        assert torch.equal(_run(c, transposed, *inputs)[0],
                           _run(c, transposed, *inputs)[0])


def test_unsupported_problems_are_errors():
    ge = backend.ext()
    x = torch.zeros(1, 8, 8, 8, device="cuda", dtype=torch.bfloat16)
    w = torch.zeros(8, 8, 1, 7, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="tap_fwd_strided: stride"):
        ge.tap_fwd_strided(x, w, None, 1, 1, 0, 3)
    with pytest.raises(RuntimeError, match="tap_fwd_strided: kernel size"):
        ge.tap_fwd_strided(x, x[:, :, :5, :5].contiguous(), None, 2, 2, 2, 2)
    with pytest.raises(RuntimeError, match="tap_bwd_data_strided: padding"):
        ge.tap_bwd_data_strided(x, w, 8, 16, 1, 2, 1, 3)
