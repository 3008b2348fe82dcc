"""``conv_native.conv_plan``: the route of each leg at every measured
crossover, on both sides (CPU; needs neither GPU nor extension).

The expected routes are literals read off ``ConvFn`` as it stood before
the plan existed, not computed from the plan's own thresholds.
"""

import pytest

from mpi4dl_amd.ops.conv_native import conv_plan

NATIVE_PW = ("pw_fwd", "pw_fwd", "pw_bwdw")
GENERAL_S1 = ("conv_fwd", "conv_fwd", "conv_bwd_weight")
GENERAL_ZS = ("conv_fwd", "conv_fwd_zs", "conv_bwd_weight")


def _plan(C, K, H, W, R=1, S=1, sh=1, sw=1, ph=0, pw=0, N=2):
    return conv_plan(N, C, K, H, W, R, S, sh, sw, ph, pw)


def _routes(plan):
    return tuple(leg.route for leg in plan)


# (C, K, H, W), leg, route with MPI4DL_PW_BLASLT on; off, all are native
CROSSOVERS = [
    ((40, 64, 8, 16), "y", "pw_fwd"),
    ((40, 65, 8, 16), "y", "matmul"),
    ((64, 40, 8, 16), "gx", "pw_fwd"),
    ((65, 40, 8, 16), "gx", "matmul"),
    ((500, 700, 8, 16), "gw", "bmm"),         # C*K = 350 000
    ((499, 700, 8, 16), "gw", "pw_bwdw"),     # C*K = 349 300
    ((500, 700, 128, 256), "gw", "bmm"),      # OHW = 32 768
    ((500, 700, 257, 128), "gw", "pw_bwdw"),  # OHW = 32 896
]


@pytest.mark.parametrize("shape,leg,route", CROSSOVERS)
@pytest.mark.parametrize("switch", ["unset", "1", "0"])
def test_blaslt_crossovers(shape, leg, route, switch, monkeypatch):
    if switch == "unset":
        monkeypatch.delenv("MPI4DL_PW_BLASLT", raising=False)
    else:
        monkeypatch.setenv("MPI4DL_PW_BLASLT", switch)
    plan = _plan(*shape)
    if switch == "0":
        assert _routes(plan) == NATIVE_PW
    else:
        assert getattr(plan, leg).route == route
    # the explicit argument overrides the variable
    assert _routes(conv_plan(2, *shape, 1, 1, 1, 1, 0, 0, blaslt=False)) \
        == NATIVE_PW


def test_pw_problems():
    """What the 1x1 routes hand to their bindings; the mirror GEMM of gx
    swaps C and K."""
    C, K = 40, 24
    plan = conv_plan(3, C, K, 8, 16, 1, 1, 1, 1, 0, 0, blaslt=False)
    assert plan.y == ("pw_fwd", (C, K, 128, 1, 1))
    assert plan.gx == ("pw_fwd", (K, C, 128, 1, 1))
    assert plan.gw == ("pw_bwdw", (3, K, C, 128))
    plan = conv_plan(3, C, K, 16, 32, 1, 1, 2, 2, 0, 0)
    assert plan.y == ("pw_fwd", (C, K, 128, 2, 1))
    assert plan.gx == ("pw_bwd_data_strided", (K, C, 128, 1, 2))
    assert plan.gw == ("pw_bwdw_sub", (3, K, C, 128))


@pytest.mark.parametrize("kwargs,routes", [
    (dict(H=8, W=15), GENERAL_S1),                  # OHW % 128 != 0
    (dict(H=8, W=16, ph=1, pw=1), GENERAL_S1),      # 1x1 with pad 1
    (dict(H=16, W=32, sh=2, sw=2),
     ("pw_fwd", "pw_bwd_data_strided", "pw_bwdw_sub")),
    (dict(H=64, W=24, sh=2, sw=2), GENERAL_ZS),     # OHW = 384, OW = 12
    (dict(H=16, W=16, sh=2, sw=1), GENERAL_ZS),     # stride (2, 1)
])
def test_pw_geometry(kwargs, routes, monkeypatch):
    for switch in ("0", "1"):
        monkeypatch.setenv("MPI4DL_PW_BLASLT", switch)
        assert _routes(_plan(40, 72, **kwargs)) == routes


@pytest.mark.parametrize("kwargs,gx", [
    # stride 1: conv_fwd on (K -> C) with the transposed-conv pads
    (dict(H=16, W=24, R=3, S=3, ph=1, pw=1),
     ("conv_fwd", (24, 16, 16, 24, 3, 3, 1, 1, 1, 1))),
    (dict(H=16, W=38, R=1, S=7),
     ("conv_fwd", (24, 16, 16, 32, 1, 7, 1, 1, 0, 6))),
    # stride 2: the gradient zero-stuffed back to the input's extents
    (dict(H=34, W=34, R=3, S=3, sh=2, sw=2, ph=1, pw=1),
     ("conv_fwd_zs", (24, 16, 34, 34, 3, 3, 1, 1, 1, 1))),
    (dict(H=33, W=33, R=3, S=3, sh=2, sw=2, ph=1, pw=1),
     ("conv_fwd_zs", (24, 16, 33, 33, 3, 3, 1, 1, 1, 1))),
])
def test_general_conv(kwargs, gx):
    plan = _plan(16, 24, **kwargs)
    g = dict(dict(R=1, S=1, sh=1, sw=1, ph=0, pw=0), **kwargs)
    fwd = (16, 24, g["H"], g["W"], g["R"], g["S"], g["sh"], g["sw"],
           g["ph"], g["pw"])
    assert plan.y == ("conv_fwd", fwd)
    assert plan.gx == gx
    assert plan.gw == ("conv_bwd_weight", fwd)
