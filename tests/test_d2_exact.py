"""AmoebaNet-D D2 (fused halo) is exact in TRAINING: BNs that run on a
surplus tile take their statistics from the nominal region only
(TileBatchNorm2d.stat_margin), so forward, parameter gradients and BN
running statistics equal the serial model's; plus the runner wiring of
``--model amoebanet --halo-d2``."""

import os
import sys

import pytest
import torch

from dist_util import run_distributed

NCLS = 10
EPS_REL = 1e-9  # fp64 parity bound, relative to the serial tensor's max


# ---------------------------------------------------------------------------
# stat_margin against a hand computation (single process, fp64)
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("margin", [(3, 0, 0, 3), (1, 1, 1, 1)])
def test_margin_bn_matches_hand_computation(margin, relu):
    from mpi4dl_amd.ops.norm import TileBatchNorm2d

    torch.manual_seed(0)
    t, b, l, r = margin
    x = torch.randn(2, 3, 9, 11, dtype=torch.float64)
    bn = TileBatchNorm2d(3, relu=relu, stat_margin=margin).double()
    with torch.no_grad():
        bn.weight.copy_(torch.tensor([0.5, 1.5, -2.0]))
        bn.bias.copy_(torch.tensor([0.1, -0.2, 0.3]))
    assert "stat_margin" not in bn.state_dict()
    ref = torch.nn.BatchNorm2d(3).double()
    crop = x[:, :, t : 9 - b, l : 11 - r]
    ref(crop)  # train mode: updates ref's running stats from the crop

    y = bn(x)
    mean = crop.mean(dim=(0, 2, 3)).view(1, -1, 1, 1)
    var = crop.var(dim=(0, 2, 3), unbiased=False).view(1, -1, 1, 1)
    want = (x - mean) / torch.sqrt(var + bn.eps)
    want = want * bn.weight.view(1, -1, 1, 1) + bn.bias.view(1, -1, 1, 1)
    if relu:
        want = torch.relu(want)
    assert y.shape == x.shape
    assert torch.allclose(y, want, rtol=0, atol=1e-12), (y - want).abs().max()
    assert torch.allclose(bn.running_mean, ref.running_mean, rtol=0, atol=1e-13)
    assert torch.allclose(bn.running_var, ref.running_var, rtol=0, atol=1e-13)
    assert int(bn.num_batches_tracked) == 1

    # eval ignores the margin
    bn.eval()
    ye = bn(x)
    rm = bn.running_mean.view(1, -1, 1, 1)
    rv = bn.running_var.view(1, -1, 1, 1)
    we = (x - rm) / torch.sqrt(rv + bn.eps) * bn.weight.view(1, -1, 1, 1)
    we = we + bn.bias.view(1, -1, 1, 1)
    if relu:
        we = torch.relu(we)
    assert torch.allclose(ye, we, rtol=0, atol=1e-12)
    bn.train()

    def fn(xi, w, bb):
        return torch.func.functional_call(bn, {"weight": w, "bias": bb}, (xi,))

    assert torch.autograd.gradcheck(
        fn,
        (
            x.clone().requires_grad_(True),
            bn.weight.detach().clone().requires_grad_(True),
            bn.bias.detach().clone().requires_grad_(True),
        ),
    )


def test_margin_bn_attribute_and_empty_region():
    from mpi4dl_amd.ops.norm import TileBatchNorm2d

    bn = TileBatchNorm2d(2).double()
    assert bn.stat_margin == (0, 0, 0, 0)
    x = torch.randn(2, 2, 6, 6, dtype=torch.float64)
    y0 = bn(x)
    bn.stat_margin = (1, 2, 0, 1)  # settable after construction
    y1 = bn(x)
    assert not torch.allclose(y0, y1)
    bn.stat_margin = (3, 3, 0, 0)
    with pytest.raises(ValueError):
        bn(x)
    bn.eval()
    bn(x)  # eval ignores the margin, even an impossible one


# ---------------------------------------------------------------------------
# train-mode parity with the serial model
# ---------------------------------------------------------------------------


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _d2_train_parity_body(rank, world, method, img):
    import torch.distributed as dist

    from mpi4dl_amd.comm import Communicator
    from mpi4dl_amd.models.amoebanet import amoebanetd
    from mpi4dl_amd.models.amoebanet_d2 import amoebanetd_d2
    from mpi4dl_amd.ops.halo import TileLayout
    from mpi4dl_amd.ops.plan import SpatialPlan

    comm = Communicator(
        split_size=1, ENABLE_SPATIAL=True, num_spatial_parts=world,
        spatial_size=1, backend="gloo",
    )
    torch.manual_seed(0)
    serial = amoebanetd(NCLS, 3, 32)
    plan = SpatialPlan(comm, [len(serial)], method)
    torch.manual_seed(0)
    d2 = amoebanetd_d2(NCLS, 3, 32, plan=plan)
    serial = torch.nn.Sequential(*list(serial)[:4]).double().train()
    d2 = torch.nn.Sequential(*list(d2)[:4]).double().train()
    torch.manual_seed(9)
    x = torch.randn(2, 3, img, img, dtype=torch.float64)
    layout = TileLayout(world, method)

    def tup(v):
        return v if isinstance(v, tuple) else (v,)

    ys = tup(serial(x))
    sum(y.square().sum() for y in ys).backward()
    yt = tup(d2(layout.slice_input(x, rank).contiguous()))
    sum(y.square().sum() for y in yt).backward()

    worst = {"fwd": 0.0, "grad": 0.0, "stat": 0.0}
    assert len(yt) == len(ys)
    for a, b in zip(yt, ys):
        a, b = a.detach(), b.detach()
        expect = layout.slice_input(b, rank)
        assert a.shape == expect.shape, (a.shape, expect.shape)
        worst["fwd"] = max(
            worst["fwd"], float((a - expect).abs().max() / b.abs().max())
        )

    ps, pt = list(serial.parameters()), list(d2.parameters())
    assert len(ps) == len(pt)
    checked = 0
    for a, b in zip(pt, ps):
        assert a.shape == b.shape
        g = a.grad.clone()
        dist.all_reduce(g)  # the whole world is the one tile group
        if b.grad.abs().max() < 1e-9:
            continue  # analytically zero (e.g. conv weights before a BN)
        checked += 1
        worst["grad"] = max(worst["grad"], _rel(g, b.grad))
    assert checked > len(ps) // 2, (checked, len(ps))

    bs, bt = list(serial.buffers()), list(d2.buffers())
    assert len(bs) == len(bt)
    for a, b in zip(bt, bs):
        if a.dtype == torch.long:
            assert int(a) == int(b)
            continue
        worst["stat"] = max(worst["stat"], _rel(a, b))
    print(f"rank {rank} {method} {img}: {worst}")
    assert worst["fwd"] <= EPS_REL, worst
    assert worst["stat"] <= EPS_REL, worst
    assert worst["grad"] <= EPS_REL, worst
    return worst


def test_amoebanet_d2_train_exact_vertical2():
    run_distributed(_d2_train_parity_body, 2, ("vertical", 64), timeout=300)


def test_amoebanet_d2_train_exact_square4():
    run_distributed(_d2_train_parity_body, 4, ("square", 128), timeout=300)


# ---------------------------------------------------------------------------
# runner wiring
# ---------------------------------------------------------------------------


def _bench_path():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "benchmarks"))


def test_runner_builds_amoebanet_d2():
    _bench_path()
    from runner import build_model

    from mpi4dl_amd.models.amoebanet_d2 import CellD2
    from mpi4dl_amd.parser import get_parser

    base = ["--model", "amoebanet", "--num-layers", "3", "--num-filters", "8",
            "--image-size", "32", "--num-classes", "10"]
    d2 = build_model(get_parser().parse_args(base + ["--halo-d2"]), None, 1)
    d1 = build_model(get_parser().parse_args(base), None, 1)
    assert any(isinstance(m, CellD2) for m in d2.modules())
    assert not any(isinstance(m, CellD2) for m in d1.modules())
    assert [p.shape for p in d1.parameters()] == [p.shape for p in d2.parameters()]


def _run_mode(rank, world, mode, model, extra):
    _bench_path()
    from runner import run_training

    from mpi4dl_amd.parser import get_parser

    argv = [
        "--model", model, "--batch-size", "4", "--parts", "2",
        "--image-size", "32", "--num-layers", "9", "--num-filters", "4",
        "--num-classes", "10", "--num-epochs", "1", "--num-steps", "2",
        "--backend", "gloo",
    ] + list(extra)
    args = get_parser().parse_args(argv)
    times = run_training(args, mode)
    return len(times)


def test_entry_sp_amoebanet_d2():
    # test_entry_sp_amoebanet's configuration with the D2 model
    got = run_distributed(
        _run_mode, 3,
        ("sp", "amoebanet",
         ("--split-size", "2", "--num-spatial-parts", "2",
          "--spatial-size", "1", "--slice-method", "vertical",
          "--num-layers", "6", "--num-filters", "8",
          "--image-size", "128", "--halo-d2")),
        timeout=300,
    )
    assert got[0] == 2
