"""HaloExchanger's GPU path on one MI355X: the cached strip plan, the
flat staging buffers and the halo_pack / halo_unpack / halo_unpack_add
kernels, every tile of a grid on one device. Transport, oracles and the
case matrix: ``halo_loopback.py``; ``test_halo_loopback.py`` runs the
same matrix through the CPU packer.

Every case runs twice on the same exchangers with fresh data: the second
run takes the cached plan and reuses the staging buffers."""

import pytest
import torch

import halo_loopback as hl

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)
pytestmark = [gpu, requires_gpu]

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
dtypes = pytest.mark.parametrize(
    "dtype", DTYPES, ids=[str(d).split(".")[1] for d in DTYPES]
)


@pytest.fixture
def loop(monkeypatch):
    return hl.install(monkeypatch)


@dtypes
@pytest.mark.parametrize("case", hl.CASES, ids=hl.case_id)
def test_forward(case, dtype, loop):
    spec, h, d2 = case
    grid = hl.Grid(spec, loop)
    for seed in (0, 1):
        hl.check_forward(grid, h, d2, "cuda", dtype, seed)
    assert all(len(ex._plans) <= 1 for ex in grid.exs)


@dtypes
@pytest.mark.parametrize("case", hl.CASES, ids=hl.case_id)
def test_transposed(case, dtype, loop):
    spec, h, d2 = case
    grid = hl.Grid(spec, loop)
    for seed in (0, 1):
        hl.check_transposed(grid, h, d2, "cuda", dtype, seed)
    assert all(len(ex._plans) <= 1 for ex in grid.exs)


@dtypes
@pytest.mark.parametrize("d2", [False, True], ids=["sym", "d2"])
@pytest.mark.parametrize("h", [3, (2, 1)], ids=["h3", "h2x1"])
def test_autograd(h, d2, dtype, loop):
    """halo_pad and halo_pad_d2 hand h, off and nominal through to the
    exchanger, forward and backward (grad_mode='exact')."""
    hl.check_autograd(hl.Grid(("square", 4), loop), h, d2, "cuda", dtype)
