"""conv_plan with the tap weight-gradient switch, and its kernel's name."""

import pytest

from mpi4dl_amd.ops.conv_native import ConvPlan, Leg, conv_plan

GEOMS = [(1, 7, 0, 3), (7, 1, 3, 0), (3, 3, 1, 1)]


@pytest.mark.parametrize("R, S, ph, pw", GEOMS)
def test_routes(monkeypatch, R, S, ph, pw):
    monkeypatch.delenv("MPI4DL_TAPCONV_WGRAD", raising=False)
    geom = (2, 20, 24, 15, 17, R, S, 1, 1, ph, pw)
    legs = (Leg("tap_fwd", (20, 24, 15, 17, R, S, ph, pw)),
            Leg("tap_fwd", (24, 20, 15, 17, R, S, R - 1 - ph, S - 1 - pw)))
    # the first switch alone: today's plan
    assert conv_plan(*geom, winograd=False, tap=True) == ConvPlan(
        *legs, Leg("conv_bwd_weight", (20, 24, 15, 17, R, S, 1, 1, ph, pw)))
    assert conv_plan(*geom, winograd=False, tap=True, tap_wgrad=True) == (
        ConvPlan(*legs, Leg("tap_bwd_weight", (2, 20, 24, 15, 17, R, S, ph, pw))))


def test_switches_from_the_environment(monkeypatch):
    monkeypatch.delenv("MPI4DL_WINOGRAD", raising=False)
    monkeypatch.delenv("MPI4DL_TAPCONV", raising=False)
    geom = (2, 26, 26, 16, 24, 1, 7, 1, 1, 0, 3)
    default = conv_plan(*geom)
    assert default.gw == Leg("conv_bwd_weight", geom[1:])
    monkeypatch.setenv("MPI4DL_TAPCONV_WGRAD", "1")
    assert conv_plan(*geom) == default          # alone: nothing changes
    assert conv_plan(*geom, tap_wgrad=True) == default
    monkeypatch.setenv("MPI4DL_TAPCONV", "1")
    want = Leg("tap_bwd_weight", (2, 26, 26, 16, 24, 1, 7, 0, 3))
    assert conv_plan(*geom).gw == want
    # Winograd keeps its precedence on 3x3, weight-grad included
    wino = (2, 16, 24, 16, 24, 3, 3, 1, 1, 1, 1)
    assert (conv_plan(*wino, winograd=True)
            == conv_plan(*wino, winograd=True, tap=False))


@pytest.mark.parametrize("K, tpb", [(16, 4), (104, 8), (416, 29)])
def test_kernel_name(K, tpb):
    """1024 tiles of 2 x 64 or 4 x 32 pixels; 2 C tiles x 1, 2, 7 K tiles, so
    512 blocks are 256, 128, 36 runs of 4, 8, ceil(1024 / 36) = 29 tiles."""
    from mpi4dl_amd import _gemscore
    for (R, S, ph, pw) in GEOMS:
        assert (_gemscore.tap_bwdw_kernel_name(2, 104, K, 256, 256, R, S, ph, pw)
                == f"tap_bwdw<{R}x{S},64x64,tpb{tpb}>")
