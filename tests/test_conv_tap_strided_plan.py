"""conv_plan with the strided tap-shift switch: which problems take the
tap_fwd_strided / tap_bwd_data_strided routes, and that nothing else moves."""

from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from mpi4dl_amd.ops.conv_native import (ConvPlan, Leg, _tap_dispatchable,
                                        conv_plan)

# N = 2, C = 20, K = 24, 15 x 17: (R, S, sh, sw, ph, pw, OH, OW)
STRIDED = [(1, 7, 1, 2, 0, 3, 15, 9), (7, 1, 2, 1, 3, 0, 8, 17),
           (3, 3, 2, 2, 1, 1, 8, 9), (3, 3, 2, 2, 0, 2, 7, 10)]


@pytest.mark.parametrize("R, S, sh, sw, ph, pw, OH, OW", STRIDED)
def test_strided_routes(R, S, sh, sw, ph, pw, OH, OW):
    geom = (2, 20, 24, 15, 17, R, S, sh, sw, ph, pw)
    fwd = geom[1:]
    assert conv_plan(*geom, tap=True, tap_strided=True) == ConvPlan(
        Leg("tap_fwd_strided", fwd),
        Leg("tap_bwd_data_strided", (24, 20, OH, OW, 15, 17, R, S, sh, sw, ph, pw)),
        Leg("conv_bwd_weight", fwd),
    )
    # the second switch alone, or only the first: today's plan
    assert (conv_plan(*geom, tap=False, tap_strided=True)
            == conv_plan(*geom, tap=False, tap_strided=False)
            == conv_plan(*geom, tap=True, tap_strided=False))
    assert conv_plan(*geom, tap=True, tap_strided=False).gx.route == "conv_fwd_zs"


@pytest.mark.parametrize("geom", [
    (2, 20, 24, 15, 17, 1, 7, 1, 1, 0, 3),   # stride 1: stays on tap_fwd
    (2, 20, 24, 15, 17, 1, 7, 2, 2, 0, 3),   # 1x7 at (2, 2)
    (2, 20, 24, 15, 17, 3, 3, 2, 1, 1, 1),   # 3x3 at (2, 1)
    (2, 20, 24, 15, 17, 3, 3, 2, 2, 3, 1),   # a pad the kernel lacks
    (2, 8, 16, 16, 16, 5, 5, 2, 2, 2, 2),    # 5x5
    (2, 40, 48, 8, 16, 1, 1, 2, 2, 0, 0),    # strided 1x1
])
def test_strided_leaves_other_problems(geom):
    assert (conv_plan(*geom, winograd=False, tap=True, tap_strided=True)
            == conv_plan(*geom, winograd=False, tap=True, tap_strided=False))


def test_module_predicate_and_env(monkeypatch):
    xg = SimpleNamespace(is_cuda=True, is_meta=False, dim=lambda: 4,
                         dtype=torch.bfloat16, shape=(2, 8, 16, 16))
    strided = nn.Conv2d(8, 8, (1, 7), stride=(1, 2), padding=(0, 3))
    plain = nn.Conv2d(8, 8, (1, 7), padding=(0, 3))
    for tap, second, want in [("0", "0", (False, False)), ("0", "1", (False, False)),
                              ("1", "0", (False, True)), ("1", "1", (True, True))]:
        monkeypatch.setenv("MPI4DL_TAPCONV", tap)
        monkeypatch.setenv("MPI4DL_TAPCONV_STRIDED", second)
        assert (_tap_dispatchable(xg, strided), _tap_dispatchable(xg, plain)) == want
    # both set: conv_plan reads them
    assert conv_plan(2, 8, 8, 16, 16, 1, 7, 1, 2, 0, 3).y.route == "tap_fwd_strided"
    assert not _tap_dispatchable(
        xg, nn.Conv2d(8, 8, (1, 7), stride=(2, 2), padding=(0, 3)))


@pytest.mark.parametrize("K, mf", [(16, 2), (52, 4), (104, 7), (120, 4)])
def test_kernel_name(K, mf):
    from mpi4dl_amd import _gemscore
    name = _gemscore.tap_strided_kernel_name
    assert name(20, K, 15, 17, 1, 7, 1, 2, 0, 3) == f"tap_strided<1x7,{mf}>"
    assert name(20, K, 15, 17, 3, 3, 2, 2, 1, 1) == f"tap_strided<3x3,{mf}>"
    assert name(20, K, 15, 17, 7, 1, 2, 1, 3, 0, True) == f"tap_strided_bwd<7x1,{mf}>"
    # the 3x3 data gradient holds four accumulator sets: MF at most 4
    assert (name(20, K, 15, 17, 3, 3, 2, 2, 1, 1, True)
            == f"tap_strided_bwd<3x3,{min(mf, 4)}>")
