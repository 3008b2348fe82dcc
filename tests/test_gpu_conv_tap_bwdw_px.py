"""ge.tap_bwd_weight_px against float64 conv2d_weight, and through autograd."""

import functools

import pytest
import torch

import conv_oracle
from mpi4dl_amd.ops import backend
from mpi4dl_amd.ops.conv_native import native_conv2d

pytestmark = pytest.mark.gpu

KERNELS = [(1, 7), (7, 1), (3, 3)]
# (N, C, K, H, W, pad mode, x sliced off an unaligned base). A step is 2 rows of
# a band of 64 columns (1x7) or 4 rows of 32 (7x1, 3x3); a block owns 128 x 32
# channels. x is staged 16 bytes at a time where W % 8 == 0, the base is aligned
# and the pad is "same"; go where OW % 8 == 0.
SHAPES = [
    (2, 19, 20, 15, 17, "same", False),   # channel tails; odd H, W: by elements
    (1, 40, 130, 9, 72, "same", False),   # 2 k tiles, 2 c tiles, 2-3 bands; 16-byte
    (2, 33, 24, 23, 40, "same", False),   # 16-byte; N 2; rows not a multiple of a step
    (1, 20, 24, 12, 24, "same", True),    # W % 8 == 0 off an unaligned base
    (1, 40, 16, 10, 72, "valid", False),  # pad 0: x shifted under the patch
    (1, 20, 8, 12, 24, "full", False),    # the largest pads: the other shifts
    (3, 32, 33, 9, 22, "valid", False),   # 1x7: x by elements, go (OW 16) 16-byte
]
IDS = ["n%dc%dk%d-%dx%d-%s-%d" % s for s in SHAPES]
both = lambda f: pytest.mark.parametrize("s", SHAPES, ids=IDS)(
    pytest.mark.parametrize("rs", KERNELS, ids=lambda rs: "%dx%d" % rs)(f))


def _case(rs, s):
    (R, S), (N, C, K, H, W, mode, _) = rs, s
    m = {"same": 2, "valid": 0, "full": 4}[mode]   # pad = (size - 1) * m / 4
    return conv_oracle.Case(f"tappx-{R}x{S}-" + IDS[SHAPES.index(s)], "autograd",
                            "tap+tap+tap_bwdw", C, K, H, W, R, S,
                            ph=(R - 1) * m // 4, pw=(S - 1) * m // 4,
                            bias=True, N=N)


def _offset(t):
    """The same values, one element (2 bytes) into a larger buffer."""
    return torch.cat([t.new_zeros(1), t.flatten()])[1:].view(t.shape)


@functools.lru_cache(maxsize=None)
def _dyadic(c, unaligned=False):
    """x, go: multiples of 1/4 in [-2, 2], so with N*OH*OW < 2^18 every partial
    sum is exact in fp32 in any order; the float64 weight gradient."""
    assert c.N * c.OH * c.OW < 2 ** 18
    gen = torch.Generator().manual_seed(2)
    x = torch.randint(-8, 9, (c.N, c.C, c.H, c.W), generator=gen) / 4
    go = torch.randint(-8, 9, (c.N, c.K, c.OH, c.OW), generator=gen) / 4
    ref = torch.nn.grad.conv2d_weight(
        x.double(), (c.K, c.C, c.R, c.S), go.double(), padding=(c.ph, c.pw))
    x, go = x.bfloat16().cuda(), go.bfloat16().cuda()
    return (_offset(x), _offset(go), ref) if unaligned else (x, go, ref)


def _px(c, go, x, *extra):
    return backend.ext().tap_bwd_weight_px(go, x, c.R, c.S, c.ph, c.pw, *extra)


@both
@pytest.mark.parametrize("prior", [False, True], ids=["fresh", "out"])
def test_exact_on_dyadic_inputs(rs, s, prior):
    """Fresh, or added into a dyadic ``out``. The chooser's strip (0) is one
    step here; 23 rows also run as strips of 8 rows (4 or 2 steps, a short last
    strip) and as one strip of all steps, through both LDS buffers."""
    c = _case(rs, s)
    x, go, ref = _dyadic(c, s[6])
    assert (x.data_ptr() % 16 != 0) == s[6]
    gen = torch.Generator().manual_seed(3)
    g0 = torch.randint(-64, 65, ref.shape, generator=gen) / 16 * prior
    for rows in (0, 8, 10 ** 6) if s[3] == 23 else (0,):
        out = g0.float().cuda() if prior else None
        got = _px(c, go, x, out, rows)
        assert got.dtype == torch.float32 and got.shape == ref.shape
        assert not prior or got.data_ptr() == out.data_ptr()
        assert torch.equal(got.double().cpu(), g0.double() + ref), rows


@both
def test_random_within_bound(rs, s):
    c = _case(rs, s)
    x, w, b, go = conv_oracle.make_inputs(c)
    ref = conv_oracle.reference(c, x, w, b, go)
    worst = conv_oracle.assert_within(
        _px(c, go.cuda(), x.cuda()), *ref["gw"],
        conv_oracle.reduction_length(c, "gw"), False, what=c.name)
    print(f"err/bound {worst:.3f}")


@pytest.mark.parametrize("rs, s, sink", [
    (rs, SHAPES[0], False) for rs in KERNELS] + [((7, 1), SHAPES[2], True)])
def test_autograd(rs, s, sink, monkeypatch):
    """Both switches, dyadic inputs (the atomic sum is exact: bit for bit).
    ``sink``: the kernel adds into a w.grad that holds a dyadic g0."""
    from mpi4dl_amd.ops.grad_sink import opt_in
    for k, v in zip(("TAPCONV", "TAPCONV_WGRAD", "GRAD_SINK"), ("1", "px", "1")):
        monkeypatch.setenv("MPI4DL_" + k, v)
    c = _case(rs, s)
    x, go, ref = _dyadic(c)
    gen = torch.Generator().manual_seed(4)
    w = torch.randn(ref.shape, generator=gen) * 0.1
    b = torch.randn(c.K, generator=gen).cuda()
    xg, wg = x.clone().requires_grad_(True), torch.nn.Parameter(w.cuda())
    g0 = torch.zeros_like(w)
    if sink:
        g0 = torch.randint(-64, 65, w.shape, generator=gen) / 16
        wg.grad = g0.cuda()
        ptr = wg.grad.data_ptr()
        opt_in(wg)
    y = native_conv2d(xg, wg, b, 1, (c.ph, c.pw))
    y.backward(go)
    tap_fwd, wb = backend.ext().tap_fwd, w.bfloat16().cuda()
    assert torch.equal(y, tap_fwd(x, wb, b, c.ph, c.pw))
    assert torch.equal(xg.grad, tap_fwd(go, wb, None, c.R - 1 - c.ph,
                                        c.S - 1 - c.pw, True))
    assert not sink or wg.grad.data_ptr() == ptr
    assert torch.equal(wg.grad, _px(c, go, x, g0.cuda()))
    assert torch.equal(wg.grad.double().cpu(), g0.double() + ref)


@pytest.mark.parametrize("args, msg", [
    ((1, 5, 0, 2), "kernel size"), ((1, 7, 1, 3), "padding"),
    ((1, 7, 0, 0), "go is not the gradient")])
def test_unsupported_problems_are_errors(args, msg):
    x = torch.zeros(1, 8, 8, 8, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match=msg):
        backend.ext().tap_bwd_weight_px(x, x, *args)
