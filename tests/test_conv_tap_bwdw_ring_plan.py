"""conv_plan with MPI4DL_TAPCONV_WGRAD=ring, and the ring kernel's name."""

import pytest

from mpi4dl_amd.ops.conv_native import Leg, conv_plan

GEOMS = [(1, 7, 0, 3), (7, 1, 3, 0), (3, 3, 1, 1)]


@pytest.mark.parametrize("R, S, ph, pw", GEOMS)
def test_routes(monkeypatch, R, S, ph, pw):
    monkeypatch.delenv("MPI4DL_WINOGRAD", raising=False)
    monkeypatch.delenv("MPI4DL_TAPCONV", raising=False)
    geom = (2, 20, 24, 15, 17, R, S, 1, 1, ph, pw)
    tapw = (2, 20, 24, 15, 17, R, S, ph, pw)
    first = conv_plan(*geom, tap=True, tap_wgrad=True)
    assert first.gw == Leg("tap_bwd_weight", tapw)   # True: the first kernel
    assert conv_plan(*geom, tap=True, tap_wgrad="ring") == first._replace(
        gw=Leg("tap_bwd_weight_ring", tapw))
    with pytest.raises(ValueError, match="tap_wgrad"):
        conv_plan(*geom, tap=True, tap_wgrad="rings")
    default = conv_plan(*geom)
    monkeypatch.setenv("MPI4DL_TAPCONV_WGRAD", "ring")
    assert conv_plan(*geom) == default          # alone: nothing changes
    assert conv_plan(*geom, tap_wgrad="ring") == default
    # Winograd keeps its precedence on 3x3, weight-grad included
    assert R != 3 or (conv_plan(*geom, winograd=True, tap=True)
                      == conv_plan(*geom, winograd=True, tap=False))
    monkeypatch.setenv("MPI4DL_TAPCONV", "1")
    assert conv_plan(*geom).gw == Leg("tap_bwd_weight_ring", tapw)
    monkeypatch.setenv("MPI4DL_TAPCONV_WGRAD", "1")
    assert conv_plan(*geom).gw == Leg("tap_bwd_weight", tapw)
    monkeypatch.setenv("MPI4DL_TAPCONV_WGRAD", "Ring")   # any other value
    assert conv_plan(*geom).gw == default.gw


@pytest.mark.parametrize("C, K, hw, tile, rows17, rows", [
    (104, 16, 256, "32x64", 4, 8), (104, 104, 256, "32x64", 16, 32),
    (104, 416, 256, "32x64", 50, 84), (52, 52, 512, "32x64", 16, 32),
    (104, 52, 512, "32x64", 32, 64), (20, 52, 512, "32x32", 16, 32),
    (84, 52, 512, "32x32", 46, 84)])
def test_kernel_name(C, K, hw, tile, rows17, rows):
    """N 2: hw / 2 steps a band, 2 hw / 64 (1x7) or 2 hw / 32 bands; a strip is
    floor(steps / ceil(1024 / (k tiles * c tiles * bands))) steps of 2 rows. C
    104 and 52 pad alike under both tiles (wide: 2, 1 c tiles); 20 and 84 pad to
    32 and 96, not 64 and 128 (narrow: 1, 3). K 16, 104, 416, 52: 1, 4, 13, 2 k
    tiles. K 416 at 256, 1x7: 13 * 2 * 8 = 208, ceil(1024 / 208) = 5, 128 // 5 = 25."""
    from mpi4dl_amd import _gemscore
    for (R, S, ph, pw) in GEOMS:
        assert (_gemscore.tap_bwdw_ring_kernel_name(2, C, K, hw, hw, R, S, ph, pw)
                == f"tap_bwdw_ring<{R}x{S},{tile},rows{rows17 if S == 7 else rows}>")
