"""HaloExchanger's strip plan and begin/finish path, every tile of a
grid in one process (CPU, torch-slicing packer). Transport, oracles and
the case matrix: ``halo_loopback.py``."""

import pytest
import torch

import halo_loopback as hl


@pytest.fixture
def loop(monkeypatch):
    return hl.install(monkeypatch)


@pytest.mark.parametrize("case", hl.CASES, ids=hl.case_id)
def test_forward(case, loop):
    grid, h, d2 = case
    hl.check_forward(hl.Grid(grid, loop), h, d2, "cpu", torch.float32)


@pytest.mark.parametrize("case", hl.CASES, ids=hl.case_id)
def test_transposed(case, loop):
    grid, h, d2 = case
    hl.check_transposed(hl.Grid(grid, loop), h, d2, "cpu", torch.float32)


@pytest.mark.parametrize("d2", [False, True], ids=["sym", "d2"])
@pytest.mark.parametrize("h", [3, (2, 1)], ids=["h3", "h2x1"])
def test_autograd(h, d2, loop):
    hl.check_autograd(hl.Grid(("square", 4), loop), h, d2, "cpu", torch.float32)


def test_centre_tile_fills_all_strips(loop):
    """The centre of the 3x3 grid exchanges with 8 neighbours, MAX_STRIPS
    of halo_copy_kernel. The tags on the wire: a recv carries the index
    of the direction it arrives from, a send the index of the opposite
    direction (DIRS[7 - i] is the opposite of DIRS[i]), gradients 8 more."""
    from mpi4dl_amd.ops.halo import DIRS

    ex = hl.Grid(("square", 9), loop).exs[4]
    assert [d for d, _ in ex.neigh] == DIRS
    for grad, base in ((False, 0), (True, 8)):
        strips = ex._strips(hl.T, hl.T, (2, 1), None, grad)
        assert [s.peer for s in strips] == [0, 1, 2, 3, 5, 6, 7, 8]
        assert [s.recv_tag for s in strips] == [base + i for i in range(8)]
        assert [s.send_tag for s in strips] == [base + 7 - i for i in range(8)]


@pytest.mark.parametrize("entry", hl.ENTRY_POINTS)
@pytest.mark.parametrize("d2", [False, True], ids=["sym", "d2"])
def test_halo_larger_than_tile_asserts(entry, d2, loop):
    """A halo of 9 on an 8 x 8 tile cannot be served by the direct
    neighbours: every entry point refuses it before anything is sent."""
    grid = hl.Grid(("square", 4), loop)
    h = 9
    top, bottom, left, right = grid.pads(0, h, d2)
    xp = torch.zeros(hl.N, hl.C, hl.T + top + bottom, hl.T + left + right)
    loop.me = 0
    with pytest.raises(AssertionError, match="exceeds local tile"):
        getattr(grid.exs[0], entry)(xp, h, **grid.kwargs(0, h, d2))
    assert not loop.pending()
