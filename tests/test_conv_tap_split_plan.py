"""conv_plan with the split-channel switch: tap_fwd_split appears only with
both switches, on the tap kernel's problems; the chooser's answers at 256 CUs."""

import pytest

from mpi4dl_amd.ops.conv_native import Leg, _tap_ok, conv_plan

GEOMS = [
    (2, 20, 24, 15, 17, 1, 7, 1, 1, 0, 3),
    (2, 20, 24, 15, 17, 7, 1, 1, 1, 6, 0),   # full pad
    (2, 20, 24, 15, 17, 3, 3, 1, 1, 1, 1),
    (2, 26, 26, 16, 32, 1, 7, 1, 2, 0, 3),   # stride-2 1x7
    (2, 16, 24, 16, 24, 3, 3, 1, 1, 3, 1),   # 3x3 with a pad the kernel lacks
]


@pytest.mark.parametrize("geom", GEOMS)
def test_split_route_needs_both_switches(geom, monkeypatch):
    for v in ("MPI4DL_WINOGRAD", "MPI4DL_TAPCONV", "MPI4DL_TAPCONV_WGRAD"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("MPI4DL_TAPCONV_SPLIT", "auto")
    N, C, K, H, W, R, S, sh, sw, ph, pw = geom
    default = conv_plan(*geom, tap=False, tap_split=False)
    tap = conv_plan(*geom, tap=True, tap_split=False)
    assert conv_plan(*geom) == default == conv_plan(*geom, tap_split=True)
    both = conv_plan(*geom, tap=True)           # tap_split from the environment
    if not _tap_ok(H, W, R, S, sh, sw, ph, pw):
        assert both == tap == default
        return
    assert tap.y.route == tap.gx.route == "tap_fwd"
    assert both.y == Leg("tap_fwd_split", (N, C, K, H, W, R, S, ph, pw))
    assert both[1:] == (Leg("tap_fwd_split", (N,) + tap.gx.problem), tap.gw)
    monkeypatch.setenv("MPI4DL_TAPCONV_SPLIT", "1")   # only "auto" is on
    assert conv_plan(*geom, tap=True) == tap


@pytest.mark.parametrize("R, S", [(1, 7), (7, 1), (3, 3)])
def test_split_kernel_name(R, S):
    from mpi4dl_amd import _gemscore as ge
    ph, pw = R // 2, S // 2
    assert ge.tap_split_kernel_name(2, 416, 416, 64, 64, R, S, ph, pw, 256) \
        == (f"tap_split<{R}x{S},4>", 3)   # 7 k tiles x 32 x 3 >= 2 x 256
    assert ge.tap_split_kernel_name(2, 104, 104, 256, 256, R, S, ph, pw, 256) \
        == (ge.tap_kernel_name(104, 104, 256, 256, R, S, ph, pw), 1)
    # two chunks: never more than two slices, however small the grid
    assert ge.tap_split_kernel_name(1, 40, 16, 8, 8, R, S, ph, pw, 256)[1] == 2
    assert ge.tap_split_kernel_name(1, 512, 16, 8, 8, R, S, ph, pw, 256)[1] == 8
