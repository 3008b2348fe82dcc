"""conv_plan with the fused-Winograd switch: which problems take the
wino_fwd route, with which pads, and that nothing else moves."""

import pytest

from mpi4dl_amd.ops.conv_native import ConvPlan, Leg, conv_plan


@pytest.mark.parametrize("ph, pw, gx_problem", [
    (1, 1, (24, 20, 15, 17, 1, 1)),
    (0, 0, (24, 20, 13, 15, 2, 2)),
    (0, 2, (24, 20, 13, 19, 2, 0)),
])
def test_winograd_routes(ph, pw, gx_problem):
    plan = conv_plan(2, 20, 24, 15, 17, 3, 3, 1, 1, ph, pw, winograd=True)
    assert plan == ConvPlan(
        Leg("wino_fwd", (20, 24, 15, 17, ph, pw)),
        Leg("wino_fwd", gx_problem),
        Leg("conv_bwd_weight", (20, 24, 15, 17, 3, 3, 1, 1, ph, pw)),
    )


@pytest.mark.parametrize("geom", [
    (2, 16, 24, 16, 24, 3, 3, 2, 2, 1, 1),   # 3x3 stride 2
    (2, 26, 26, 16, 24, 1, 7, 1, 1, 0, 3),   # 1x7
    (2, 40, 48, 8, 16, 1, 1, 1, 1, 0, 0),    # 1x1
    (2, 8, 16, 16, 16, 5, 5, 1, 1, 2, 2),    # 5x5
    (2, 16, 24, 16, 24, 3, 3, 1, 1, 3, 1),   # 3x3 with a pad the kernel lacks
])
def test_winograd_leaves_other_problems(geom):
    assert conv_plan(*geom, winograd=True) == conv_plan(*geom, winograd=False)


@pytest.mark.parametrize("value", [None, "0", "1"])
def test_default_plan_unchanged(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("MPI4DL_WINOGRAD", raising=False)
    else:
        monkeypatch.setenv("MPI4DL_WINOGRAD", value)
    fwd = (16, 24, 16, 24, 3, 3, 1, 1, 1, 1)
    assert conv_plan(2, *fwd) == ConvPlan(
        Leg("conv_fwd", fwd),
        Leg("conv_fwd", (24, 16, 16, 24, 3, 3, 1, 1, 1, 1)),
        Leg("conv_bwd_weight", fwd),
    )


@pytest.mark.parametrize("K, label", [
    (1, "wino<32>"), (32, "wino<32>"), (33, "wino<64>"), (136, "wino<64>")])
def test_kernel_name(K, label):
    from mpi4dl_amd import _gemscore
    assert _gemscore.wino_kernel_name(20, K, 15, 17, 1, 1) == label


def test_env_switch(monkeypatch):
    monkeypatch.setenv("MPI4DL_WINOGRAD", "fused")
    assert conv_plan(2, 16, 24, 16, 24, 3, 3, 1, 1, 1, 1).y == Leg(
        "wino_fwd", (16, 24, 16, 24, 1, 1))
