"""The module tree, layout attributes and state-dict layout of the
AmoebaNet cells and models equal the recorded golden
(tests/amoebanet_layout.py): D1 and D2 cells without a plan and on three
tile positions with different surplus margins, and both whole models."""

import json

import pytest

import amoebanet_layout as L

CASES = sorted(L.cases())


def test_cases_are_the_golden_ones():
    assert len(CASES) == 18
    assert sorted(L.load_golden()) == CASES


@pytest.mark.parametrize("name", CASES)
def test_layout_matches_golden(name, tmp_path):
    desc = L.describe(L.cases()[name]())
    diff = L.first_difference(desc, L.load_golden()[name])
    if diff is not None:
        out = tmp_path / f"{name}.json"
        out.write_text(json.dumps(desc, indent=1, sort_keys=True))
        pytest.fail(f"{name}: first difference at {diff}; "
                    f"current description written to {out}")


def test_d2_margins_and_needs():
    """The figures of the surplus path, spelled out: square 4, tile 3 has
    neighbours above and to the left only."""
    from mpi4dl_amd.models.amoebanet_d2 import CellD2
    from mpi4dl_amd.ops.norm import TileBatchNorm2d

    ctx = L._ctx(L.CTXS["square4_tile3"])
    nor = CellD2(64, 64, 32, False, False, ctx=ctx, mknorm=TileBatchNorm2d)
    red = CellD2(64, 64, 32, True, False, ctx=ctx, mknorm=TileBatchNorm2d)
    assert nor.op_need == [0, 0, 0, 3, 0, 3, 0, 0, 0, 0]
    assert red.op_need == [0, 0, 0, 0, 3, 0, 0, 0, 0, 0]
    for pos in (3, 5):
        op = nor.operations[pos]
        assert [list(op[i].stat_margin) for i in (1, 4, 7)] == [
            [3, 0, 3, 0], [3, 0, 0, 0], [0, 0, 0, 0]]
