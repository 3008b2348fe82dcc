"""ge.tap_fwd with split != 0 against float64 direct convolution: bit-equal on
dyadic inputs, within the oracle's bound on random ones, chooser, autograd."""

import pytest
import torch
import torch.nn.functional as F

import conv_oracle
from mpi4dl_amd.ops import backend
from mpi4dl_amd.ops.conv_native import native_conv2d

pytestmark = pytest.mark.gpu

KERNELS = [(1, 7), (7, 1), (3, 3)]
# (H, W) for 1x7 and for 7x1 / 3x3 (tiles 4x64, 8x32); ragged: two tiles an axis
PLANES = {"ragged": ((9, 70), (17, 35)), "vec": ((8, 72), (16, 40)),
          "w23": ((5, 23), (9, 23))}
PADS = {"same": lambda R, S: (R // 2, S // 2), "valid": lambda R, S: (0, 0),
        "full": lambda R, S: (R - 1, S - 1)}
# (N, C reduced, K out, plane, pad, bias, split, x on an unaligned base)
SHAPES = [
    (2, 40, 20, "ragged", "same", True, 2, False),   # ragged 2nd chunk, K tail
    (1, 100, 130, "vec", "same", False, 3, False),   # 2/1/1, 16-byte paths
    (1, 100, 20, "ragged", "valid", True, 4, False),  # one chunk a slice
    (1, 40, 60, "vec", "full", True, 2, False),      # MF = 4: two store passes
    (1, 40, 20, "w23", "same", True, 2, True),       # element paths
    (1, 72, 130, "vec", "same", True, 3, True),      # W % 8 == 0, base is not
]
IDS = ["n%dc%dk%d-%s-%s-b%d-s%d-u%d" % s for s in SHAPES]


def _run(rs, s, transposed, x, w, b, split=None):
    """ge.tap_fwd(split), its float64 reference and that on absolute values."""
    (R, S), (mode, _, sc, unaligned) = rs, s[4:]
    ph, pw = PADS[mode](R, S)
    xg = x.bfloat16().cuda()
    if unaligned:  # 2 bytes past an aligned base
        xg = torch.cat([xg.new_zeros(1), xg.flatten()])[1:].view(x.shape)
    got = backend.ext().tap_fwd(
        xg, w.bfloat16().cuda(), None if b is None else b.cuda(), ph, pw,
        transposed, sc if split is None else split)
    if transposed:  # w is the forward weight [C reduced][K out]
        op = lambda *a: F.conv_transpose2d(*a, padding=(R - 1 - ph, S - 1 - pw))
    else:
        op = lambda *a: F.conv2d(*a, padding=(ph, pw))
    d = lambda t: None if t is None else t.double()
    a = lambda t: None if t is None else t.double().abs()
    return got.cpu(), op(d(x), d(w), d(b)), op(a(x), a(w), a(b))


def _inputs(rs, s, transposed, dyadic):
    N, C, K, plane, _, bias = s[:6]
    H, W = PLANES[plane][rs != (1, 7)]
    wshape = (C, K, *rs) if transposed else (K, C, *rs)
    gen = torch.Generator().manual_seed(3)
    if dyadic:
        ri = lambda lo, hi, *sh: torch.randint(lo, hi, sh, generator=gen)
        return (ri(-8, 9, N, C, H, W) / 4, ri(-8, 9, *wshape) / 8,
                ri(-16, 17, K) / 8 if bias else None)
    rn = lambda *sh: torch.randn(*sh, generator=gen)
    return (rn(N, C, H, W).bfloat16().float(),
            (0.1 * rn(*wshape)).bfloat16().float(), rn(K) if bias else None)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("s", SHAPES, ids=IDS)
@pytest.mark.parametrize("rs", KERNELS, ids=lambda rs: "%dx%d" % rs)
def test_exact_on_dyadic_inputs(rs, s, transposed):
    got, ref, _ = _run(rs, s, transposed, *_inputs(rs, s, transposed, True))
    assert got.dtype == torch.bfloat16 and torch.equal(got, ref.bfloat16())


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("s", SHAPES[:2], ids=IDS[:2])
@pytest.mark.parametrize("rs", KERNELS, ids=lambda rs: "%dx%d" % rs)
def test_random_within_bound_and_deterministic(rs, s, transposed):
    inputs = _inputs(rs, s, transposed, False)
    got, ref, A = _run(rs, s, transposed, *inputs)
    L = s[1] * rs[0] * rs[1] + int(s[5])   # the full C*R*S, not a slice's
    conv_oracle.assert_within(got, ref, A, L, out_is_bf16=True)
    assert torch.equal(got, _run(rs, s, transposed, *inputs)[0])


@pytest.mark.parametrize("rs", KERNELS, ids=lambda rs: "%dx%d" % rs)
def test_chooser_launch(rs):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ph, pw = PADS["same"](*rs)
    for s, splits in ((SHAPES[1], True), ((1, 20, 130) + SHAPES[1][3:], False)):
        inputs = _inputs(rs, s, False, True)
        _, sc = backend.ext().tap_split_kernel_name(
            *s[:3], *inputs[0].shape[2:], *rs, ph, pw, cus)
        got, ref, _ = _run(rs, s, False, *inputs, split=-1)
        assert (sc > 1) == splits and torch.equal(got, ref.bfloat16())
        unsplit = _run(rs, s, False, *inputs, split=0)[0]
        assert splits or torch.equal(got, unsplit)   # SC = 1: the same kernel


@pytest.mark.parametrize("rs", KERNELS, ids=lambda rs: "%dx%d" % rs)
def test_autograd(rs, monkeypatch):
    monkeypatch.setenv("MPI4DL_TAPCONV", "1")
    monkeypatch.setenv("MPI4DL_TAPCONV_SPLIT", "auto")
    ge = backend.ext()
    s = SHAPES[1][:5] + (True,)
    x, w, b = (t.cuda() for t in _inputs(rs, s, False, False))
    ph, pw = PADS["same"](*rs)
    xg = x.bfloat16().requires_grad_(True)
    y = native_conv2d(xg, w.clone().requires_grad_(True), b, 1, (ph, pw))
    go = torch.randn_like(y)
    y.backward(go)
    wb = w.bfloat16()
    assert torch.equal(y, ge.tap_fwd(xg.detach(), wb, b, ph, pw, split=-1))
    assert torch.equal(xg.grad, ge.tap_fwd(
        go, wb, None, rs[0] - 1 - ph, rs[1] - 1 - pw, True, split=-1))


def test_bad_slice_counts_are_errors():
    ge = backend.ext()
    z = lambda *sh: torch.zeros(*sh, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="only 2 chunks"):
        ge.tap_fwd(z(1, 40, 8, 8), z(8, 40, 1, 7), None, 0, 3, split=3)
    with pytest.raises(RuntimeError, match="at most 8"):
        ge.tap_fwd(z(1, 320, 8, 8), z(8, 320, 1, 7), None, 0, 3, split=9)
