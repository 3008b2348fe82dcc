"""GPU (MI355X) tests of the gradient sink: the backward kernels add the
weight gradients into ``param.grad`` in place. Every case runs twice from
the same seeds, with the sink and with ``MPI4DL_GRAD_SINK=0``, over two
micro-batches and a seeded nonzero prior gradient.

BatchNorm: the in-place add is a cast and one add per element, as the
returned-tensor path does them, so everything is ``torch.equal``.
Convolutions: both paths are fp32 sums of the same terms in another order,
bounded per element (see ``_conv_bound``)."""

import pytest
import torch

gpu = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

BF = torch.bfloat16


def _spy_backward(monkeypatch, fn_cls, log, params_of):
    """Log (parameters, returned gradients) of every fn_cls.backward call."""
    real = fn_cls.backward

    def wrapped(ctx, *gos):
        out = real(ctx, *gos)
        log.append((params_of(ctx), out))
        return out

    monkeypatch.setattr(fn_cls, "backward", staticmethod(wrapped))


def _spy_ext(monkeypatch, ge, name, log):
    real = getattr(ge, name)

    def wrapped(*a, **k):
        out = real(*a, **k)
        log.append((name, a, k, out))
        return out

    monkeypatch.setattr(ge, name, wrapped)


# ---------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------

def _bn_run(monkeypatch, sink, *args, **kw):
    with monkeypatch.context() as mp:  # the spies leave with the run
        return _bn_run_patched(mp, sink, *args, **kw)


def _bn_run_patched(monkeypatch, sink, shape, margin, relu, dtype,
                    mode="train"):
    """mode: train (two micro-batches), retain (one forward, two backwards
    over the retained graph), eval. Returns the results and the spy logs."""
    from mpi4dl_amd.ops import backend, native
    from mpi4dl_amd.ops.grad_sink import opt_in
    from mpi4dl_amd.ops.norm import TileBatchNorm2d

    monkeypatch.setenv("MPI4DL_GRAD_SINK", "1" if sink else "0")
    ge = backend.ext()
    C = shape[1]
    g = torch.Generator().manual_seed(11)
    bn = TileBatchNorm2d(C, relu=relu, stat_margin=margin).cuda()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g))
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.1 + 0.5)
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    if mode == "eval":
        bn.eval()
    grads = {}
    for name, p in (("weight", bn.weight), ("bias", bn.bias)):
        p.grad = (torch.randn(C, generator=g) * 3 + 1).cuda()  # nonzero prior
        opt_in(p)
        grads[name] = p.grad
    prior = {k: v.clone() for k, v in grads.items()}
    ptrs = {k: v.data_ptr() for k, v in grads.items()}

    fn_log, ext_log = [], []
    _spy_backward(monkeypatch, native.BatchNormFn, fn_log,
                  lambda ctx: ctx.params)
    for name in ("bn_finalize", "bn_bwd_stats"):
        _spy_ext(monkeypatch, ge, name, ext_log)

    def draw():
        return (torch.randn(shape, generator=g) + 0.5).to(dtype).cuda()

    gis = []
    if mode == "retain":
        x, go = draw().requires_grad_(True), draw()
        y = bn(x)
        y.backward(go, retain_graph=True)
        gis.append(x.grad)
        x.grad = None
        y.backward(go)
        gis.append(x.grad)
    else:
        for _ in range(2):
            x, go = draw().requires_grad_(True), draw()
            bn(x).backward(go)
            gis.append(x.grad)
    torch.cuda.synchronize()

    # .grad is still the tensor that was installed, whichever path added
    assert bn.weight.grad is grads["weight"] and bn.bias.grad is grads["bias"]
    assert {k: v.data_ptr() for k, v in grads.items()} == ptrs
    return dict(gi=gis, gw=bn.weight.grad.clone(), gb=bn.bias.grad.clone(),
                fn_log=fn_log, ext_log=ext_log, bn=bn, prior=prior)


def _bn_check_pair(monkeypatch, shape, margin, relu, dtype, mode="train"):
    on = _bn_run(monkeypatch, True, shape, margin, relu, dtype, mode)
    off = _bn_run(monkeypatch, False, shape, margin, relu, dtype, mode)
    assert len(on["fn_log"]) == len(off["fn_log"]) == 2
    # the sink run returns no parameter gradient: nothing for autograd to
    # cast or add; the other run returns both, fp32
    for (w, b), out in on["fn_log"]:
        assert w is on["bn"].weight and b is on["bn"].bias
        assert out[1] is None and out[2] is None
    for _, out in off["fn_log"]:
        assert out[1].dtype == out[2].dtype == torch.float32
    for a, b in zip(on["gi"], off["gi"]):
        assert torch.equal(a, b)
    assert torch.equal(on["gw"], off["gw"])
    assert torch.equal(on["gb"], off["gb"])
    # the gradients really moved off the prior
    assert not torch.equal(on["gw"], on["prior"]["weight"])
    assert not torch.equal(on["gb"], on["prior"]["bias"])
    return on, off


def _stats_buffers(run):
    """(zero2 handed to bn_finalize, out handed to bn_bwd_stats, its result)
    per call, in order."""
    fin = [k.get("zero2") for n, a, k, o in run["ext_log"] if n == "bn_finalize"]
    bwd = [(k.get("out"), o) for n, a, k, o in run["ext_log"]
           if n == "bn_bwd_stats"]
    return fin, bwd


# whole slots; ragged, HW = 63; more channels (600) than a block has threads,
# so block 0 walks the parameter gradients in several passes
BN_SHAPES = [(3, 9, 16, 24), (2, 5, 7, 9), (1, 600, 2, 2)]
BN_IDS = ["whole", "ragged", "tiny"]


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("margin", [(0, 0, 0, 0), (1, 0, 1, 0)],
                         ids=["full", "margin"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=BN_IDS)
def test_bn_sink_equals_returned_gradients(monkeypatch, shape, margin, relu,
                                           dtype):
    on, _ = _bn_check_pair(monkeypatch, shape, margin, relu, dtype)
    # no fp64 fill: each backward accumulated its statistics in the buffer
    # that its forward's bn_finalize had zeroed, and returned that buffer
    fin, bwd = _stats_buffers(on)
    assert len(fin) == len(bwd) == 2
    for z, (out, res) in zip(fin, bwd):
        assert z is not None and z.dtype == torch.float64
        assert out.data_ptr() == z.data_ptr() == res.data_ptr()


@gpu
@requires_gpu
@pytest.mark.parametrize("shape", BN_SHAPES, ids=BN_IDS)
def test_bn_second_backward_over_retained_graph(monkeypatch, shape):
    """The zeroed buffer serves the first backward only: the second fills
    its own and gives the same gi."""
    on, _ = _bn_check_pair(monkeypatch, shape, (0, 0, 0, 0), True, BF,
                           mode="retain")
    assert torch.equal(on["gi"][0], on["gi"][1])
    fin, bwd = _stats_buffers(on)
    assert len(fin) == 1 and len(bwd) == 2
    assert bwd[0][0].data_ptr() == fin[0].data_ptr()
    assert bwd[1][0] is None
    assert bwd[1][1].data_ptr() != fin[0].data_ptr()


@gpu
@requires_gpu
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
def test_bn_eval_mode(monkeypatch, relu):
    on, _ = _bn_check_pair(monkeypatch, (3, 9, 16, 24), (0, 0, 0, 0), relu,
                           BF, mode="eval")
    fin, bwd = _stats_buffers(on)
    assert fin == [] and all(out is None for out, _ in bwd)


# ---------------------------------------------------------------------------
# Convolution weight gradients
# ---------------------------------------------------------------------------

#        id                N  C    K    H    W    R  S  s  pad     gw route           label
CONV_CASES = [
    ("pw_bwdw128",        2, 24,  40,  8,   16,  1, 1, 1, (0, 0), "pw_bwdw",         "pw_bwdw128"),
    ("pw_bwdw128:slab",   1, 24,  40,  32,  32,  1, 1, 1, (0, 0), "pw_bwdw",         "pw_bwdw128:slab"),
    ("pw_bwdw256",        1, 256, 256, 128, 128, 1, 1, 1, (0, 0), "pw_bwdw",         "pw_bwdw256:slab"),
    ("pw_bwdw_sub",       2, 16,  24,  32,  32,  1, 1, 2, (0, 0), "pw_bwdw_sub",     "pw_bwdw128"),
    ("conv_bwdw-stem",    2, 3,   8,   16,  128, 3, 3, 2, (1, 1), "conv_bwd_weight", None),
    ("conv_bwdw-1x7",     2, 16,  16,  4,   384, 1, 7, 1, (0, 3), "conv_bwd_weight", None),
]
MICRO = 2


def _conv_data(case):
    _, N, C, K, H, W, R, S, s, (ph, pw), _, _ = case
    g = torch.Generator().manual_seed(23)
    OH = (H + 2 * ph - R) // s + 1
    OW = (W + 2 * pw - S) // s + 1
    w = torch.randn(K, C, R, S, generator=g) * 0.2
    g0 = torch.randn(K, C, R, S, generator=g) * 2 + 0.5  # nonzero prior grad
    xs = [torch.randn(N, C, H, W, generator=g).to(BF) for _ in range(MICRO)]
    gos = [torch.randn(N, K, OH, OW, generator=g).to(BF) for _ in range(MICRO)]
    return w, g0, xs, gos


def _conv_run(monkeypatch, case, data, sink):
    with monkeypatch.context() as mp:
        return _conv_run_patched(mp, case, data, sink)


def _conv_run_patched(monkeypatch, case, data, sink):
    from mpi4dl_amd.ops import conv_native
    from mpi4dl_amd.ops.grad_sink import opt_in

    _, N, C, K, H, W, R, S, s, pad, _, _ = case
    monkeypatch.setenv("MPI4DL_GRAD_SINK", "1" if sink else "0")
    w0, g0, xs, gos = data
    w = torch.nn.Parameter(w0.cuda())
    w.grad = g0.cuda().clone()
    grad_obj, ptr = w.grad, w.grad.data_ptr()
    opt_in(w)
    log = []
    _spy_backward(monkeypatch, conv_native.ConvFn, log, lambda ctx: ctx.wparam)
    gxs = []
    for x, go in zip(xs, gos):
        x = x.cuda().requires_grad_(True)
        y = conv_native.native_conv2d(x, w, None, (s, s), pad)
        y.backward(go.cuda())
        gxs.append(x.grad)
    torch.cuda.synchronize()
    assert w.grad is grad_obj and w.grad.data_ptr() == ptr
    assert len(log) == MICRO and all(p is w for p, _ in log)
    if sink:  # nothing came back for autograd to add
        assert all(out[1] is None for _, out in log)
    else:
        assert all(out[1].shape == w.shape for _, out in log)
    return w.grad.clone().cpu(), [t.cpu() for t in gxs]


def _conv_bound(case, data, label):
    """Per-element bound on |sink - returned|.

    Both are fp32 sums of the same m values in different orders: the prior
    gradient and one partial sum per block that adds into the element,
    ``blocks`` per micro-batch. A sum of m fp32 values in any order is
    within (m-1) * 2^-24 * sum|values| of the exact sum (first order), the
    two orders therefore within twice that of each other, and sum|values|
    <= |g0| + A with A = sum |go|*|x| over the element's reduction (fp64,
    here). blocks: pw_bwdw splits the pixels of an image into slabs (512
    pixels when the label says ':slab', for these power-of-two planes; the
    whole image otherwise), conv_bwdw has one block per output row."""
    _, N, C, K, H, W, R, S, s, (ph, pw), route, _ = case
    _, g0, xs, gos = data
    OH, OW = gos[0].shape[-2:]
    A = torch.zeros(K, C, R, S, dtype=torch.float64)
    for x, go in zip(xs, gos):
        xa, ga = x.double().abs(), go.double().abs()
        if R == 1 and S == 1:
            xa = xa[:, :, ::s, ::s].reshape(N, C, -1)
            A += torch.einsum("nkp,ncp->kc", ga.reshape(N, K, -1),
                              xa).view(K, C, 1, 1)
        else:
            A += torch.nn.grad.conv2d_weight(xa, (K, C, R, S), ga, stride=s,
                                             padding=(ph, pw))
    if route == "conv_bwd_weight":
        blocks = N * OH
    else:
        ohw = OH * OW
        blocks = N * (ohw // 512 if label.endswith(":slab") else 1)
    m = 1 + MICRO * blocks
    return 2 * (m - 1) * 2.0 ** -24 * (g0.double().abs() + A), m


@gpu
@requires_gpu
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_sink_within_reordering_bound(monkeypatch, case):
    from mpi4dl_amd.ops import backend
    from mpi4dl_amd.ops.conv_native import conv_plan

    _, N, C, K, H, W, R, S, s, (ph, pw), route, want_label = case
    ge = backend.ext()
    plan = conv_plan(N, C, K, H, W, R, S, s, s, ph, pw)
    assert plan.gw.route == route
    label = None
    if want_label is not None:
        label = ge.pw_bwdw_kernel_name(*plan.gw.problem)
        assert label == want_label
    data = _conv_data(case)
    gw_on, gx_on = _conv_run(monkeypatch, case, data, True)
    gw_off, gx_off = _conv_run(monkeypatch, case, data, False)
    for a, b in zip(gx_on, gx_off):
        assert torch.equal(a, b)
    bound, m = _conv_bound(case, data, label)
    diff = (gw_on.double() - gw_off.double()).abs()
    worst = float((diff / bound).max())
    print(f"{case[0]}: m={m} max|diff|={float(diff.max()):.3e} "
          f"max diff/bound={worst:.3f}")
    assert bool((diff <= bound).all()), worst
    # the returned-tensor run is autograd's own prior + both micro-batches;
    # the bound above ties the sink run to it. Neither left the prior alone.
    assert not torch.equal(gw_on, data[1])
    assert not torch.equal(gw_off, data[1])


@gpu
@requires_gpu
def test_autograd_grad_leaves_param_grad_alone(monkeypatch):
    """torch.autograd.grad w.r.t. the input only: the weight's gradient is
    not asked for, so nothing may be added into w.grad."""
    from mpi4dl_amd.ops import conv_native
    from mpi4dl_amd.ops.grad_sink import opt_in

    monkeypatch.setenv("MPI4DL_GRAD_SINK", "1")
    case = CONV_CASES[0]
    w0, g0, xs, gos = _conv_data(case)
    w = torch.nn.Parameter(w0.cuda())
    w.grad = g0.cuda().clone()
    opt_in(w)
    x = xs[0].cuda().requires_grad_(True)
    y = conv_native.native_conv2d(x, w, None, (1, 1), (0, 0))
    (gx,) = torch.autograd.grad(y, x, gos[0].cuda())
    torch.cuda.synchronize()
    assert gx.shape == x.shape
    assert torch.equal(w.grad.cpu(), g0)


# ---------------------------------------------------------------------------
# End to end: stem + two cells of AmoebaNet-D, FusedSGD's flat buffers
# ---------------------------------------------------------------------------

def _e2e_model():
    from mpi4dl_amd.models.amoebanet import amoebanetd
    from mpi4dl_amd.optim import FusedSGD

    torch.manual_seed(5)
    net = amoebanetd(num_classes=10, num_layers=3, num_filters=32)
    body = net[:3].cuda()  # stem and the two reduction cells: 64^2 -> 8^2
    opt = FusedSGD(body, lr=0.01)
    return body, opt


def _e2e_inputs():
    g = torch.Generator().manual_seed(6)
    return [torch.randn(2, 3, 64, 64, generator=g).cuda() for _ in range(2)]


def _e2e_step(body, opt, xs):
    """Two micro-batches into a zeroed flat gradient buffer."""
    opt.fg.zero_()
    for x in xs:
        with torch.autocast("cuda", dtype=BF):
            out = body(x)
        out = out[0] if isinstance(out, (tuple, list)) else out
        out.float().square().mean().backward()


def _bn_mask(body, opt):
    from mpi4dl_amd.ops.norm import TileBatchNorm2d

    bn_params = {id(p) for m in body.modules()
                 if isinstance(m, TileBatchNorm2d) for p in m.parameters()}
    mask = torch.zeros(opt.flat_g.numel(), dtype=torch.bool)
    off = 0
    for p in opt.fg.params:
        if id(p) in bn_params:
            mask[off:off + p.numel()] = True
        off += p.numel()
    assert mask.any()
    return mask.cuda()


def _e2e_eager(monkeypatch, sink):
    with monkeypatch.context() as mp:
        return _e2e_eager_patched(mp, sink)


def _e2e_eager_patched(monkeypatch, sink):
    from mpi4dl_amd.ops import conv_native, native

    monkeypatch.setenv("MPI4DL_GRAD_SINK", "1" if sink else "0")
    body, opt = _e2e_model()
    bn_log, conv_log = [], []
    _spy_backward(monkeypatch, native.BatchNormFn, bn_log,
                  lambda ctx: ctx.params)
    _spy_backward(monkeypatch, conv_native.ConvFn, conv_log,
                  lambda ctx: (ctx.wparam,))
    _e2e_step(body, opt, _e2e_inputs())
    torch.cuda.synchronize()
    return body, opt, bn_log, conv_log


@gpu
@requires_gpu
def test_end_to_end_sink_on_against_off(monkeypatch):
    body, opt, bn_log, conv_log = _e2e_eager(monkeypatch, True)
    flat_on = opt.flat_g.clone()
    mask = _bn_mask(body, opt)

    # every parameter the sink fed: no tensor went back to autograd for it,
    # and its .grad is still the view of the flat buffer, now nonzero
    lo = opt.flat_g.data_ptr()
    hi = lo + opt.flat_g.numel() * 4
    fed = {}
    for params, out in bn_log:
        for p, g in zip(params, out[1:3]):
            assert g is None
            fed[id(p)] = p
    n_bn = len(fed)
    for (p,), out in conv_log:
        if out[1] is None:
            fed[id(p)] = p
        else:  # a returned gradient is a tensor of its own
            assert not (lo <= out[1].data_ptr() < hi)
    assert n_bn > 0 and len(fed) > n_bn, (n_bn, len(fed))
    for p in fed.values():
        assert lo <= p.grad.data_ptr() < hi
        assert p.grad.is_contiguous() and p.grad.shape == p.shape
        assert float(p.grad.abs().sum()) > 0

    _, opt_off, bn_off, conv_off = _e2e_eager(monkeypatch, False)
    assert all(out[1] is not None and out[2] is not None for _, out in bn_off)
    assert all(out[1] is not None for _, out in conv_off)
    flat_off = opt_off.flat_g
    assert torch.equal(flat_on[mask], flat_off[mask])
    # (the conv entries differ in the order of their fp32 sums; their
    # bound is test_conv_sink_within_reordering_bound's)
    assert bool(torch.isfinite(flat_on).all())


@gpu
@requires_gpu
def test_end_to_end_under_hipgraph(monkeypatch):
    body, opt, _, _ = _e2e_eager(monkeypatch, True)
    mask = _bn_mask(body, opt)
    eager = opt.flat_g.clone()

    body2, opt2 = _e2e_model()
    xs = _e2e_inputs()
    monkeypatch.setenv("MPI4DL_GRAD_SINK", "1")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _e2e_step(body2, opt2, xs)  # first touch, allocator
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _e2e_step(body2, opt2, xs)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(opt2.flat_g[mask], eager[mask])
