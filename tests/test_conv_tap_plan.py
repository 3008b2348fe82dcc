"""conv_plan with the tap-shift switch: which problems take the tap_fwd
route, with which pads, and that nothing else moves."""

from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from mpi4dl_amd.ops.conv_native import (ConvPlan, Leg, _tap_dispatchable,
                                        _tap_ok, conv_plan)


@pytest.mark.parametrize("R, S, ph, pw, gx_problem", [
    (1, 7, 0, 3, (24, 20, 15, 17, 1, 7, 0, 3)),    # same
    (1, 7, 0, 0, (24, 20, 15, 11, 1, 7, 0, 6)),    # valid
    (1, 7, 0, 6, (24, 20, 15, 23, 1, 7, 0, 0)),    # full
    (7, 1, 3, 0, (24, 20, 15, 17, 7, 1, 3, 0)),
    (7, 1, 0, 0, (24, 20, 9, 17, 7, 1, 6, 0)),
    (7, 1, 6, 0, (24, 20, 21, 17, 7, 1, 0, 0)),
    (3, 3, 1, 1, (24, 20, 15, 17, 3, 3, 1, 1)),
])
def test_tap_routes(R, S, ph, pw, gx_problem):
    plan = conv_plan(2, 20, 24, 15, 17, R, S, 1, 1, ph, pw, winograd=False,
                     tap=True)
    assert plan == ConvPlan(
        Leg("tap_fwd", (20, 24, 15, 17, R, S, ph, pw)),
        Leg("tap_fwd", gx_problem),
        Leg("conv_bwd_weight", (20, 24, 15, 17, R, S, 1, 1, ph, pw)),
    )


@pytest.mark.parametrize("geom", [
    (2, 40, 48, 8, 16, 1, 1, 1, 1, 0, 0),    # 1x1
    (2, 26, 26, 16, 32, 1, 7, 1, 2, 0, 3),   # stride-2 1x7
    (2, 8, 16, 16, 16, 5, 5, 1, 1, 2, 2),    # 5x5
    (2, 16, 24, 16, 24, 3, 3, 1, 1, 3, 1),   # 3x3 with a pad the kernel lacks
])
def test_tap_leaves_other_problems(geom):
    assert (conv_plan(*geom, winograd=False, tap=True)
            == conv_plan(*geom, winograd=False, tap=False))


def test_module_predicate(monkeypatch):
    monkeypatch.setenv("MPI4DL_TAPCONV", "1")
    x = torch.empty(2, 8, 16, 16, dtype=torch.bfloat16)
    plain = nn.Conv2d(8, 8, (1, 7), padding=(0, 3))
    assert not _tap_dispatchable(x, plain)   # a CPU tensor never dispatches
    # what the predicate reads of a bf16 tensor on the GPU
    xg = SimpleNamespace(is_cuda=True, is_meta=False, dim=lambda: 4,
                         dtype=torch.bfloat16, shape=x.shape)
    assert _tap_dispatchable(xg, plain)
    assert not _tap_dispatchable(xg, nn.Conv2d(8, 8, 3, padding=2, dilation=2))
    assert not _tap_dispatchable(xg, nn.Conv2d(8, 8, 3, padding=1, groups=2))
    assert not _tap_dispatchable(xg, nn.Conv2d(8, 8, (1, 7), stride=(1, 2)))
    assert not _tap_ok(2, 16, 7, 1, 1, 1, 0, 0)   # no output pixel
    monkeypatch.delenv("MPI4DL_TAPCONV")
    assert not _tap_dispatchable(xg, plain)


@pytest.mark.parametrize("value", [None, "0", "fused"])
def test_default_plan_unchanged(monkeypatch, value):
    monkeypatch.delenv("MPI4DL_WINOGRAD", raising=False)
    if value is None:
        monkeypatch.delenv("MPI4DL_TAPCONV", raising=False)
    else:
        monkeypatch.setenv("MPI4DL_TAPCONV", value)
    fwd = (26, 26, 16, 24, 1, 7, 1, 1, 0, 3)
    assert conv_plan(2, *fwd) == ConvPlan(
        Leg("conv_fwd", fwd),
        Leg("conv_fwd", (26, 26, 16, 24, 1, 7, 1, 1, 0, 3)),
        Leg("conv_bwd_weight", fwd),
    )


def test_winograd_takes_precedence_on_3x3():
    geom = (2, 16, 24, 16, 24, 3, 3, 1, 1, 1, 1)
    assert (conv_plan(*geom, winograd=True, tap=True)
            == conv_plan(*geom, winograd=True, tap=False))
    assert conv_plan(*geom, winograd=True, tap=True).y.route == "wino_fwd"


@pytest.mark.parametrize("K, mf", [(16, 2), (52, 4), (104, 7), (120, 4),
                                   (416, 7)])
def test_kernel_name(K, mf):
    from mpi4dl_amd import _gemscore
    assert _gemscore.tap_kernel_name(20, K, 15, 17, 1, 7, 0, 3) == f"tap<1x7,{mf}>"
    assert _gemscore.tap_kernel_name(20, K, 15, 17, 7, 1, 3, 0) == f"tap<7x1,{mf}>"
    assert _gemscore.tap_kernel_name(20, K, 15, 17, 3, 3, 1, 1) == f"tap<3x3,{mf}>"


def test_env_switch(monkeypatch):
    monkeypatch.delenv("MPI4DL_WINOGRAD", raising=False)
    monkeypatch.setenv("MPI4DL_TAPCONV", "1")
    assert conv_plan(2, 16, 24, 16, 24, 7, 1, 1, 1, 3, 0).y == Leg(
        "tap_fwd", (16, 24, 16, 24, 7, 1, 3, 0))
