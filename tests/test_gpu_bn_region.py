"""GPU (MI355X) tests of the BatchNorm kernels: region statistics,
TileBatchNorm2d with ``stat_margin`` and with planes whose H*W is no
multiple of 8, against references computed from the same, already
rounded inputs; and the bindings called directly on ragged, whole-slot
and misaligned tensors."""

import pytest
import torch

gpu = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

MARGINS = [(0, 0, 0, 0), (3, 0, 0, 3), (0, 3, 3, 0), (3, 3, 3, 3), (1, 1, 0, 0)]


def _crop(x, mg):
    t, b, l, r = mg
    H, W = x.shape[-2], x.shape[-1]
    return x[:, :, t : H - b, l : W - r]


def _ref_stats(x, mg):
    """[sum, sumsq] over the region: squared in fp32, summed in fp64."""
    c = _crop(x.float(), mg)
    return torch.cat([
        c.double().sum(dim=(0, 2, 3)), (c * c).double().sum(dim=(0, 2, 3))
    ])


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("margin", MARGINS)
def test_region_stats(dtype, margin):
    from mpi4dl_amd.ops import backend

    ge = backend.ext()
    torch.manual_seed(0)
    x = torch.randn(2, 5, 11, 13, device="cuda").to(dtype)
    buf = torch.zeros(10, device="cuda", dtype=torch.float64)
    got = ge.bn_stats64_region_acc(x, buf, list(margin)).clone()
    want = _ref_stats(x, margin)
    assert torch.allclose(got, want, rtol=1e-10, atol=0), (got - want).abs().max()
    # second call into the same buffer accumulates
    twice = ge.bn_stats64_region_acc(x, buf, list(margin))
    assert torch.allclose(twice, 2 * want, rtol=1e-10, atol=0)


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_region_stats_two_chunks(dtype):
    """HW = 4087 with C = 3: the stats grid has two chunks per channel."""
    from mpi4dl_amd.ops import backend

    ge = backend.ext()
    torch.manual_seed(1)
    x = torch.randn(1, 3, 67, 61, device="cuda").to(dtype)
    for margin in [(3, 3, 3, 3), (0, 0, 0, 0), (2, 1, 0, 0)]:
        buf = torch.zeros(6, device="cuda", dtype=torch.float64)
        got = ge.bn_stats64_region_acc(x, buf, list(margin))
        want = _ref_stats(x, margin)
        assert torch.allclose(got, want, rtol=1e-10, atol=0), (
            margin, (got - want).abs().max()
        )


@gpu
@requires_gpu
def test_region_stats_rejects_empty_region():
    from mpi4dl_amd.ops import backend

    x = torch.randn(1, 2, 6, 6, device="cuda")
    buf = torch.zeros(4, device="cuda", dtype=torch.float64)
    with pytest.raises(RuntimeError):
        backend.ext().bn_stats64_region_acc(x, buf, [3, 3, 0, 0])


def _run_pair(shape, margin, relu, dtype=torch.float32, seed=0):
    """Same module on cuda (native kernels) and on the CPU in fp32, train
    mode, group=None; returns both sides' results."""
    from mpi4dl_amd.ops.norm import TileBatchNorm2d

    torch.manual_seed(seed)
    C = shape[1]
    cpu = TileBatchNorm2d(C, relu=relu, stat_margin=margin)
    with torch.no_grad():
        cpu.weight.copy_(torch.rand(C) + 0.5)
        cpu.bias.copy_(torch.randn(C) * 0.3)
    dev = TileBatchNorm2d(C, relu=relu, stat_margin=margin).cuda()
    dev.load_state_dict(cpu.state_dict())
    x0 = torch.randn(*shape).to(dtype)
    g0 = torch.randn(*shape).to(dtype)
    xc = x0.float().clone().requires_grad_(True)
    yc = cpu(xc)
    yc.backward(g0.float())
    xd = x0.clone().cuda().requires_grad_(True)
    yd = dev(xd)
    yd.backward(g0.cuda())
    torch.cuda.synchronize()
    return cpu, dev, (xc, yc), (xd, yd)


FP32_CASES = [
    ((3, 9, 7, 9), (0, 0, 0, 0), False),  # ragged plane, no margin
    ((2, 4, 11, 13), (3, 0, 0, 3), False),
    ((2, 4, 11, 13), (3, 0, 0, 3), True),
    ((2, 4, 11, 13), (3, 3, 3, 3), False),
    ((2, 4, 11, 13), (3, 3, 3, 3), True),
]


@gpu
@requires_gpu
@pytest.mark.parametrize("shape,margin,relu", FP32_CASES)
def test_tile_bn_cuda_matches_cpu(shape, margin, relu):
    cpu, dev, (xc, yc), (xd, yd) = _run_pair(shape, margin, relu)
    assert yd.dtype == torch.float32 and yd.shape == yc.shape

    def err(a, b):
        return float((a.detach().cpu() - b.detach()).abs().max())

    assert err(yd, yc) <= 1e-5, err(yd, yc)
    assert err(xd.grad, xc.grad) <= 1e-4, err(xd.grad, xc.grad)
    assert err(dev.weight.grad, cpu.weight.grad) <= 1e-3
    assert err(dev.bias.grad, cpu.bias.grad) <= 1e-3
    assert err(dev.running_mean, cpu.running_mean) <= 1e-5
    assert err(dev.running_var, cpu.running_var) <= 1e-4
    assert int(dev.num_batches_tracked) == 1


def _bf16_ulp(v):
    """Spacing of bf16 (8 significand bits) at the magnitude of v."""
    mag = v.abs().float().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(mag)) - 7)


@gpu
@requires_gpu
def test_tile_bn_cuda_bf16_within_2ulp():
    cpu, dev, (xc, yc), (xd, yd) = _run_pair(
        (2, 4, 11, 13), (3, 0, 0, 3), True, dtype=torch.bfloat16
    )
    assert yd.dtype == torch.bfloat16 and xd.grad.dtype == torch.bfloat16
    for got, ref in ((yd, yc), (xd.grad, xc.grad)):
        ref16 = ref.detach().to(torch.bfloat16).float()
        diff = (got.detach().cpu().float() - ref16).abs()
        over = diff - 2 * _bf16_ulp(ref16)
        assert float(over.max()) <= 0, float(over.max())
    assert torch.allclose(dev.weight.grad.cpu(), cpu.weight.grad, atol=1e-3)
    assert torch.allclose(dev.bias.grad.cpu(), cpu.bias.grad, atol=1e-3)


@gpu
@requires_gpu
def test_ragged_plane_reaches_native_kernels(monkeypatch):
    """A plane whose H*W is no multiple of 8 runs the hand-written
    kernels, forward and backward (it took eager torch before)."""
    from mpi4dl_amd.ops import backend
    from mpi4dl_amd.ops.norm import TileBatchNorm2d

    ge = backend.ext()
    calls = []

    def spy(name):
        real = getattr(ge, name)

        def wrapped(*a, **k):
            calls.append(name)
            return real(*a, **k)

        monkeypatch.setattr(ge, name, wrapped)

    for name in ("bn_stats64_region_acc", "bn_finalize", "bn_apply",
                 "bn_bwd_stats", "bn_bwd_apply"):
        spy(name)
    bn = TileBatchNorm2d(9).cuda().train()
    x = torch.randn(3, 9, 7, 9, device="cuda", requires_grad=True)
    bn(x).sum().backward()
    torch.cuda.synchronize()
    assert calls == ["bn_stats64_region_acc", "bn_finalize", "bn_apply",
                     "bn_bwd_stats", "bn_bwd_apply"], calls


@gpu
@requires_gpu
def test_aligned_case_unchanged():
    """H*W % 8 == 0 and no margin: the module's results are bit-identical
    to the pre-existing bindings called directly."""
    from mpi4dl_amd.ops import backend
    from mpi4dl_amd.ops.norm import TileBatchNorm2d

    ge = backend.ext()
    torch.manual_seed(0)
    C = 9
    bn = TileBatchNorm2d(C).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C) + 0.5)
        bn.bias.copy_(torch.randn(C))
    x = torch.randn(3, C, 16, 24, device="cuda", requires_grad=True)
    go = torch.randn(3, C, 16, 24, device="cuda")
    y = bn(x)
    y.backward(go)

    xd = x.detach()
    n = float(3 * 16 * 24)
    buf = torch.zeros(2 * C, device="cuda", dtype=torch.float64)
    stats = ge.bn_stats64_acc(xd, buf)
    mv = ge.bn_finalize(stats, None, None, None, 0.1, n, bn.eps, rezero=True)
    mean, invstd = mv[:C].contiguous(), mv[C:].contiguous()
    w32 = bn.weight.detach().float().contiguous()
    b32 = bn.bias.detach().float().contiguous()
    y_old = ge.bn_apply(xd, mean, invstd, w32, b32, False)
    bst = ge.bn_bwd_stats(go, xd, y_old, mean, invstd, False).float()
    gi_old = ge.bn_bwd_apply(
        go, xd, y_old, mean, invstd, w32,
        bst[:C].contiguous(), bst[C:].contiguous(), n, False,
    )
    torch.cuda.synchronize()
    assert torch.equal(y.detach(), y_old)
    assert torch.equal(x.grad, gi_old)
    assert torch.equal(bn.bias.grad, bst[:C])
    assert torch.equal(bn.weight.grad, bst[C:])


# -- one kernel family for every plane shape: the bindings called directly --

def _bn_inputs(shape, dtype, seed):
    """Seeded x, go, y of ``shape`` plus the per-channel vectors and n, on
    cuda. x and go are offset from zero so that no per-channel sum comes
    out near zero (checked by _assert_no_cancellation)."""
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    t = {
        "x": (torch.randn(shape, generator=g) + 0.5).to(dtype),
        "go": (torch.randn(shape, generator=g) + 0.5).to(dtype),
        "y": torch.randn(shape, generator=g).to(dtype),
        "mean": torch.randn(C, generator=g) * 0.3,
        "invstd": torch.rand(C, generator=g) + 0.5,
        "w": torch.rand(C, generator=g) + 0.5,
        "b": torch.randn(C, generator=g) * 0.3,
        "gsum": torch.randn(C, generator=g),
        "gxsum": torch.randn(C, generator=g),
    }
    return {k: v.cuda() for k, v in t.items()}


def _ref_bwd_stats(go, x, y, mean, invstd, relu):
    """[gsum, gxsum]: products formed in fp32 as the kernel forms them,
    summed in fp64."""
    g = go.float()
    if relu:
        g = torch.where(y.float() <= 0, torch.zeros_like(g), g)
    xh = (x.float() - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
    return torch.cat([
        g.double().sum(dim=(0, 2, 3)), (g * xh).double().sum(dim=(0, 2, 3))
    ])


def _assert_no_cancellation(ref):
    """rtol=1e-10 with atol=0 only means something away from zero."""
    assert float(ref.abs().min()) >= 0.1, ref


def _close(a, b):
    return torch.allclose(a, b, rtol=1e-10, atol=0)


@gpu
@requires_gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_layout_independence(dtype, relu):
    """The same 7x9 planes as a ragged tensor (HW = 63: slots straddle the
    plane seams, the flat size 378 ends in a partial slot) and as the top
    rows of an 8x9 tensor (HW = 72: whole slots) give the same bits
    elementwise and the same sums."""
    from mpi4dl_amd.ops import backend

    ge = backend.ext()
    a = _bn_inputs((2, 3, 8, 9), dtype, seed=0)
    r = {k: v[:, :, :7].contiguous() if v.dim() == 4 else v
         for k, v in a.items()}
    vec = [a[k] for k in ("mean", "invstd", "w")]
    n = float(2 * 63)
    top = [0, 1, 0, 0]  # margin that leaves rows 0..6 of the 8x9 plane

    y_r = ge.bn_apply(r["x"], *vec, a["b"], relu)
    y_a = ge.bn_apply(a["x"], *vec, a["b"], relu)
    assert torch.equal(y_a[:, :, :7], y_r)

    gi_r = ge.bn_bwd_apply(r["go"], r["x"], r["y"], *vec, a["gsum"],
                           a["gxsum"], n, relu)
    gi_a = ge.bn_bwd_apply(a["go"], a["x"], a["y"], *vec, a["gsum"],
                           a["gxsum"], n, relu)
    gi_m = ge.bn_bwd_apply_region(a["go"], a["x"], a["y"], *vec, a["gsum"],
                                  a["gxsum"], n, relu, top)
    assert torch.equal(gi_a[:, :, :7], gi_r)
    assert torch.equal(gi_m[:, :, :7], gi_r)

    def zeros():
        return torch.zeros(6, device="cuda", dtype=torch.float64)

    want = _ref_stats(r["x"], (0, 0, 0, 0))
    _assert_no_cancellation(want)
    st_r = ge.bn_stats64_region_acc(r["x"], zeros(), [0, 0, 0, 0])
    st_m = ge.bn_stats64_region_acc(a["x"], zeros(), top)
    st_acc = ge.bn_stats64_acc(r["x"], zeros())
    for got in (st_r, st_m, st_acc):
        assert _close(got, want), (got - want).abs().max()
    assert _close(st_m, st_r) and _close(st_acc, st_r)

    want = _ref_bwd_stats(r["go"], r["x"], r["y"], a["mean"], a["invstd"], relu)
    _assert_no_cancellation(want)
    go_z = a["go"].clone()
    go_z[:, :, 7] = 0
    bs_r = ge.bn_bwd_stats(r["go"], r["x"], r["y"], a["mean"], a["invstd"], relu)
    bs_a = ge.bn_bwd_stats(go_z, a["x"], a["y"], a["mean"], a["invstd"], relu)
    assert _close(bs_r, want), (bs_r - want).abs().max()
    assert _close(bs_a, want), (bs_a - want).abs().max()
    assert _close(bs_a, bs_r)


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_whole_slot_planes_three_chunks(dtype):
    """HW = 4608 with C = 3: whole-slot planes, three chunks per channel,
    the last one partial."""
    from mpi4dl_amd.ops import backend

    ge = backend.ext()
    t = _bn_inputs((1, 3, 64, 72), dtype, seed=1)
    want = _ref_stats(t["x"], (0, 0, 0, 0))
    _assert_no_cancellation(want)
    got = ge.bn_stats64_acc(
        t["x"], torch.zeros(6, device="cuda", dtype=torch.float64))
    assert _close(got, want), (got - want).abs().max()
    for relu in (False, True):
        want = _ref_bwd_stats(t["go"], t["x"], t["y"], t["mean"], t["invstd"],
                              relu)
        _assert_no_cancellation(want)
        got = ge.bn_bwd_stats(t["go"], t["x"], t["y"], t["mean"], t["invstd"],
                              relu)
        assert _close(got, want), (relu, (got - want).abs().max())


@gpu
@requires_gpu
def test_misaligned_base():
    """Contiguous tensors whose data starts 2 bytes off the 16-byte grid
    give what their clones give."""
    from mpi4dl_amd.ops import backend

    ge = backend.ext()
    shape = (2, 3, 8, 8)
    t = _bn_inputs(shape, torch.bfloat16, seed=2)
    off = {}
    for k in ("x", "go", "y"):
        big = torch.empty(t[k].numel() + 8, device="cuda", dtype=torch.bfloat16)
        off[k] = big[1:1 + t[k].numel()].view(shape)
        off[k].copy_(t[k])
        assert off[k].is_contiguous() and off[k].data_ptr() % 16 == 2
    vec = [t[k] for k in ("mean", "invstd", "w")]
    n = float(2 * 64)
    cl = {k: v.clone() for k, v in off.items()}
    assert all(v.data_ptr() % 16 == 0 for v in cl.values())

    def both(fn):
        return fn(off), fn(cl)

    for relu in (False, True):
        def bwd(fn, *extra):
            return both(lambda s: fn(s["go"], s["x"], s["y"], *vec, t["gsum"],
                                     t["gxsum"], n, relu, *extra))

        got, want = both(lambda s: ge.bn_apply(s["x"], *vec, t["b"], relu))
        assert torch.equal(got, want)
        got, want = bwd(ge.bn_bwd_apply)
        assert torch.equal(got, want)
        got, want = bwd(ge.bn_bwd_apply_region, [1, 0, 2, 1])
        assert torch.equal(got, want)
        got, want = both(lambda s: ge.bn_bwd_stats(
            s["go"], s["x"], s["y"], t["mean"], t["invstd"], relu))
        assert _close(got, want)
    got, want = both(lambda s: ge.bn_stats64_acc(
        s["x"], torch.zeros(6, device="cuda", dtype=torch.float64)))
    assert _close(got, want)


@gpu
@requires_gpu
def test_bn_bindings_reject_bad_input():
    """Shapes, lengths and layouts are checked before any launch."""
    from mpi4dl_amd.ops import backend

    ge = backend.ext()
    t = _bn_inputs((2, 3, 8, 8), torch.bfloat16, seed=3)
    vec = [t[k] for k in ("mean", "invstd", "w")]
    with pytest.raises(RuntimeError):
        ge.bn_bwd_apply(t["go"][:, :, :4].contiguous(), t["x"], t["y"], *vec,
                        t["gsum"], t["gxsum"], 128.0, False)
    with pytest.raises(RuntimeError):
        ge.bn_apply(t["x"], torch.zeros(4, device="cuda"), t["invstd"],
                    t["w"], t["b"], False)
    go_nc = t["go"].transpose(2, 3)
    assert not go_nc.is_contiguous() and go_nc.shape == t["x"].shape
    with pytest.raises(RuntimeError):
        ge.bn_bwd_stats(go_nc, t["x"], t["y"], t["mean"], t["invstd"], False)
