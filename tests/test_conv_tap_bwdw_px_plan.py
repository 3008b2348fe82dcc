"""conv_plan with MPI4DL_TAPCONV_WGRAD=px, and the pixel-major kernel's name."""

import pytest

from mpi4dl_amd.ops.conv_native import Leg, conv_plan

GEOMS = [(1, 7, 0, 3), (7, 1, 3, 0), (3, 3, 1, 1)]


@pytest.mark.parametrize("R, S, ph, pw", GEOMS)
def test_routes(monkeypatch, R, S, ph, pw):
    monkeypatch.delenv("MPI4DL_WINOGRAD", raising=False)
    monkeypatch.delenv("MPI4DL_TAPCONV", raising=False)
    monkeypatch.delenv("MPI4DL_TAPCONV_WGRAD", raising=False)
    geom = (2, 20, 24, 15, 17, R, S, 1, 1, ph, pw)
    tapw = (2, 20, 24, 15, 17, R, S, ph, pw)
    px = conv_plan(*geom, tap=True, tap_wgrad="px")
    assert px == conv_plan(*geom, tap=True, tap_wgrad=False)._replace(
        gw=Leg("tap_bwd_weight_px", tapw))          # only the gw leg
    default = conv_plan(*geom)
    monkeypatch.setenv("MPI4DL_TAPCONV_WGRAD", "px")
    assert conv_plan(*geom) == default              # alone: nothing changes
    assert conv_plan(*geom, tap_wgrad="px") == default
    monkeypatch.setenv("MPI4DL_TAPCONV", "1")
    assert conv_plan(*geom) == px                   # the switch is the argument


@pytest.mark.parametrize("C, K, hw, rows17, rows", [
    (104, 104, 256, 16, 32), (208, 208, 128, 12, 24), (416, 416, 64, 12, 20),
    (52, 52, 512, 32, 64), (64, 64, 512, 32, 64), (512, 512, 64, 16, 32)])
def test_kernel_name(C, K, hw, rows17, rows):
    """N 2: a step is 2 rows of a band of 64 columns (1x7) or 4 rows of 32; a
    strip is floor(steps / ceil(512 / (k tiles * c tiles * bands))) steps. C104
    K104 at 256, 1x7: 1 * 4 tiles, 8 bands, ceil(512 / 32) = 16, 128 // 16 = 8
    steps. "Same" pads on W % 8 == 0 stage both operands 16 bytes at a time; pad
    0 moves x under the patch of the 1x7 and 3x3 (by elements) and makes OW
    W - 6 or W - 2 (go by elements); the 7x1 has no column taps to move."""
    from mpi4dl_amd import _gemscore
    name = _gemscore.tap_bwdw_px_kernel_name
    for (R, S, ph, pw) in GEOMS:
        r = rows17 if S == 7 else rows
        assert (name(2, C, K, hw, hw, R, S, ph, pw)
                == f"tap_bwdw_px<{R}x{S},128x32,rows{r},x16,go16>")
        staged = "x16,go16" if S == 1 else "xel,goel"
        assert name(2, C, K, hw, hw, R, S, ph, 0).endswith(staged + ">")
