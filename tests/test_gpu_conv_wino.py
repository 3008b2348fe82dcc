"""The fused Winograd F(2x2,3x3) kernel (ge.wino_fwd) against float64
direct convolution: exactly on dyadic inputs, within a derived bound on
random ones, through autograd, and run to run."""

import functools

import pytest
import torch
import torch.nn.functional as F

import conv_oracle
from conv_oracle import U_BF16
from mpi4dl_amd.ops import backend, winograd_ref
from mpi4dl_amd.ops.conv_native import NativeConv2d, native_conv2d

pytestmark = pytest.mark.gpu

# (N, C, K, H, W, ph, pw, bias)
SHAPES = [
    (2, 20, 24, 15, 17, 1, 1, True),    # C, K tails; odd OH, OW; wino<32>
    (1, 72, 72, 10, 40, 0, 2, True),    # 3 chunks, 2 K tiles, 2 column blocks
    (3, 32, 64, 8, 8, 2, 2, True),      # exact tiles, pad 2, N = 3
    (2, 136, 40, 9, 70, 1, 0, True),    # 5 chunks, 3 column and row blocks
    (1, 8, 8, 2, 2, 1, 1, True),        # smaller than one tile patch
    (2, 64, 136, 4, 64, 1, 1, False),   # no bias, 3 K tiles, aligned rows
    (1, 16, 16, 6, 16, 1, 1, True),     # wino<32> with 16-byte row stores
]
IDS = ["n%dc%dk%d-%dx%d-p%d%d" % s[:7] for s in SHAPES]


def _run(s, transposed, x, w, b, go):
    """ge.wino_fwd on the GPU and the float64 reference of the same leg."""
    N, C, K, H, W, ph, pw, _ = s
    ge = backend.ext()
    wg = w.bfloat16().cuda()
    if transposed:
        got = ge.wino_fwd(go.bfloat16().cuda(), wg, None, 2 - ph, 2 - pw, True)
        ref = torch.nn.grad.conv2d_input(
            [N, C, H, W], w.double(), go.double(), padding=(ph, pw))
    else:
        bg = None if b is None else b.cuda()
        got = ge.wino_fwd(x.bfloat16().cuda(), wg, bg, ph, pw)
        ref = F.conv2d(x.double(), w.double(),
                       None if b is None else b.double(), padding=(ph, pw))
    return got.cpu(), ref


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("s", SHAPES, ids=IDS)
def test_exact_on_dyadic_inputs(s, transposed):
    N, C, K, H, W, ph, pw, bias = s
    gen = torch.Generator().manual_seed(1)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=gen)
    x = ri(-8, 9, N, C, H, W) / 4
    w = ri(-8, 9, K, C, 3, 3) / 8
    b = ri(-16, 17, K) / 8 if bias else None
    go = ri(-8, 9, N, K, H + 2 * ph - 2, W + 2 * pw - 2) / 4
    got, ref = _run(s, transposed, x, w, b, go)
    assert got.dtype == torch.bfloat16
    assert torch.equal(got, ref.bfloat16())


def _winograd_magnitude(x, w, b, ph, pw):
    """Aw = |A^T| (sum_c |U| |V|) |A| + |b| in float64, U and V exact."""
    N, C, H, W = x.shape
    OH, OW = H + 2 * ph - 2, W + 2 * pw - 2
    TH, TW = (OH + 1) // 2, (OW + 1) // 2
    xin = F.pad(x.double(), (pw, 2 * TW + 2 - W - pw, ph, 2 * TH + 2 - H - ph))
    d = xin.unfold(2, 4, 2).unfold(3, 4, 2)
    bt, at = winograd_ref.BT.double(), winograd_ref.AT.double().abs()
    V = torch.einsum("ir,ncturs,js->nctuij", bt, d, bt).abs()
    G = winograd_ref.G.double()
    U = torch.einsum("ir,kcrs,js->kcij", G, w.double(), G).abs()
    M = torch.einsum("kcij,nctuij->nktuij", U, V)
    Y = torch.einsum("pi,nktuij,qj->nktupq", at, M, at)
    A = Y.permute(0, 1, 2, 4, 3, 5).reshape(N, -1, 2 * TH, 2 * TW)[:, :, :OH, :OW]
    return A if b is None else A + b.double().abs().view(1, -1, 1, 1)


@functools.lru_cache(maxsize=None)
def _random_inputs(s):
    N, C, K, H, W, ph, pw, bias = s
    case = conv_oracle.Case("wino-" + IDS[SHAPES.index(s)], "autograd",
                            "wino+wino+conv_bwdw", C, K, H, W, 3, 3,
                            ph=ph, pw=pw, bias=bias, N=N)
    return case, conv_oracle.make_inputs(case)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("s", SHAPES, ids=IDS)
def test_random_within_bound(s, transposed):
    N, C, K, H, W, ph, pw, _ = s
    _, (x, w, b, go) = _random_inputs(s)
    got, ref = _run(s, transposed, x, w, b, go)
    if transposed:
        Aw = _winograd_magnitude(go, w.transpose(0, 1).flip(2, 3), None,
                                 2 - ph, 2 - pw)
    else:
        Aw = _winograd_magnitude(x, w, b, ph, pw)
    worst = conv_oracle.assert_within(
        got, ref, Aw, L=(K if transposed else C) + 16, out_is_bf16=True,
        extra=(2 * U_BF16 + U_BF16 ** 2) * Aw, what=f"wino {s} T={transposed}")
    print(f"err/bound {worst:.3f}")


@pytest.mark.parametrize("s", SHAPES[:2], ids=IDS[:2])
def test_autograd(s, monkeypatch):
    monkeypatch.setenv("MPI4DL_WINOGRAD", "fused")
    N, C, K, H, W, ph, pw, _ = s
    case, (x, w, b, go) = _random_inputs(s)
    ge = backend.ext()
    xg = x.cuda().requires_grad_(True)
    wg = w.cuda().requires_grad_(True)
    bg = b.cuda().requires_grad_(True)
    y = native_conv2d(xg, wg, bg, 1, (ph, pw))
    y.backward(go.cuda())
    wb = w.bfloat16().cuda()
    assert torch.equal(y, ge.wino_fwd(x.cuda(), wb, b.cuda(), ph, pw))
    assert torch.equal(
        xg.grad, ge.wino_fwd(go.cuda(), wb, None, 2 - ph, 2 - pw, True))
    ref = conv_oracle.reference(case, x, w, b, go)
    for leg, got in (("gw", wg.grad), ("gb", bg.grad)):
        conv_oracle.assert_within(
            got, *ref[leg], conv_oracle.reduction_length(case, leg),
            conv_oracle.leg_is_bf16(leg), what=leg)


def test_module(monkeypatch):
    monkeypatch.setenv("MPI4DL_WINOGRAD", "fused")
    torch.manual_seed(0)
    conv = NativeConv2d(20, 24, 3, padding=1)
    x = torch.randn(2, 20, 15, 17)
    assert torch.equal(conv(x), F.conv2d(x, conv.weight, conv.bias, padding=1))
    y = conv.cuda()(x.bfloat16().cuda())
    assert torch.equal(y, backend.ext().wino_fwd(
        x.bfloat16().cuda(), conv.weight.bfloat16(), conv.bias.float(), 1, 1))


def test_deterministic():
    s = SHAPES[1]
    _, (x, w, b, go) = _random_inputs(s)
    for transposed in (False, True):
        assert torch.equal(_run(s, transposed, x, w, b, go)[0],
                           _run(s, transposed, x, w, b, go)[0])


def test_unsupported_problems_are_errors():
    ge = backend.ext()
    x = torch.zeros(1, 8, 8, 8, device="cuda", dtype=torch.bfloat16)
    w = torch.zeros(8, 8, 3, 3, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="padding"):
        ge.wino_fwd(x, w, None, 3, 1)
    with pytest.raises(RuntimeError, match="3x3"):
        ge.wino_fwd(x, torch.zeros_like(w[:, :, :, :1]).contiguous(), None, 0, 0)
    with pytest.raises(RuntimeError, match="channel mismatch"):
        ge.wino_fwd(x, w[:, :4].contiguous(), None, 1, 1)
