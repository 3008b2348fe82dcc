"""Every native pooling kernel against the fp64 oracle (MI355X).

One test per case of ``pool_oracle.CASES``: the forward and the backward
binding run once on the GPU, the results go to the CPU, and every
element must meet the requirement of ``pool_oracle``'s docstring. Each
case's label must be what the extension's chooser picks, and a recorder
around the extension asks the same chooser about the tensors of every
binding call that really happens. ``test_pool_oracle.py`` checks the
labels and the oracle itself without a GPU.

``test_halo_pool_on_one_gpu`` runs ``HaloPool2d``'s tiled branches, the
direct one and the overlap one, tile by tile on one device with a
stand-in exchanger that fills the ring from a global image.
"""

import pytest
import torch

import pool_oracle as po
from conv_oracle import assert_within

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)
pytestmark = [gpu, requires_gpu]


@pytest.mark.parametrize("cid", [c.id for c in po.CASES])
def test_pool_exact(cid):
    from mpi4dl_amd.ops import backend

    case = po.CASE_BY_ID[cid]
    assert po.expected_path(case, backend.ext()) == case.path
    kernels = []
    results = po.run_gpu(case, kernels)
    assert kernels == case.path.split("+"), (kernels, case.path)
    worst = po.check_case(case, results)
    for leg, kind in zip(("y", "gi"), case.path.split("+")):
        print(f"ORACLE {case.id} {leg} {kind} {worst[leg]:.3g}")


@pytest.mark.parametrize("cid", po.DETERMINISM_IDS)
def test_pool_bit_deterministic(cid):
    """No pool kernel uses atomics: two runs give identical bits."""
    case = po.CASE_BY_ID[cid]
    first, second = po.run_gpu(case), po.run_gpu(case)
    for leg in first:
        assert torch.equal(first[leg], second[leg]), (cid, leg)


# ---------------------------------------------------------------------------
# HaloPool2d, tiled, on one GPU
# ---------------------------------------------------------------------------

# (slice_method, parts, global image)
LAYOUTS = {
    "2x2": ("square", 4, (2, 3, 12, 32)),
    "1x3": ("vertical", 3, (2, 3, 8, 48)),
}
# (kind, stride, count_include_pad)
POOLS = [
    ("max", 1, True), ("max", 2, True),
    ("avg", 1, True), ("avg", 1, False),
    ("avg", 2, True), ("avg", 2, False),
]
HALO_CASES = [(lay, *pool, overlap)
              for lay in LAYOUTS for pool in POOLS for overlap in (False, True)
              if not overlap or pool[1] == 1]


def _run_tiles(layout_name, kind, s, include_pad, x, go, kernels):
    """HaloPool2d on every tile of the layout; per tile (y, x.grad)."""
    from mpi4dl_amd.ops.spatial_conv import HaloPool2d

    method, parts, _ = LAYOUTS[layout_name]
    out = []
    for t in range(parts):
        mod = HaloPool2d(kind, 3, s, padding=1, num_spatial_parts=parts,
                         slice_method=method, spatial_local_rank=t,
                         grad_mode="drop", count_include_pad=include_pad)
        mod.exchanger = po.GlobalImageExchanger(mod.layout, t, x)
        xt = mod.layout.slice_input(x, t).contiguous().requires_grad_(True)
        y = mod(xt)
        y.backward(mod.layout.slice_input(go, t))
        out.append((y.detach().cpu(), xt.grad.cpu()))
    torch.cuda.synchronize()
    assert kernels, "no native pool binding was called"
    return out


def _stitch(layout, tiles):
    rows = [torch.cat(tiles[r * layout.cols:(r + 1) * layout.cols], 3)
            for r in range(layout.rows)]
    return torch.cat(rows, 2)


@pytest.mark.parametrize(
    "layout_name,kind,s,include_pad,overlap", HALO_CASES,
    ids=lambda v: str(v))
def test_halo_pool_on_one_gpu(layout_name, kind, s, include_pad, overlap,
                              monkeypatch):
    """The tiles' outputs, stitched, meet the bound against the
    whole-image reference. Direct path: x.grad meets the bound against
    the centre crop of the reference d/dxp (grad_mode="drop"). Overlap
    path: interior pixels are bit-equal to the direct path's; the avg
    pixels whose divisor is not k*k round twice (the kernel's bf16
    average, then times k*k/div in fp32 to bf16) and carry one more
    eps*|ref|, named ``overlap-avg-border``; the max gradient, with
    integer go, is exact. The overlap avg gradient is the bf16 sum of up
    to four separately rounded pieces and is left to the band cases."""
    from mpi4dl_amd.ops import backend
    from mpi4dl_amd.ops.halo import TileLayout

    method, parts, shape = LAYOUTS[layout_name]
    layout = TileLayout(parts, method)
    N, C, Hg, Wg = shape
    Hl, Wl = Hg // layout.rows, Wg // layout.cols
    gen = torch.Generator().manual_seed(Hg * 100 + Wg + s)
    x = torch.randn(shape, generator=gen).bfloat16()
    oshape = (N, C, Hg // s, Wg // s)
    if kind == "max":
        go = torch.randint(-4, 5, oshape, generator=gen).bfloat16()
    else:
        go = torch.randn(oshape, generator=gen).bfloat16()
    eps = po.EPS["bf16"]
    plain = (-1, -1, Hg, Wg)

    rec = po.PoolRecorder(backend.ext())
    monkeypatch.setattr(backend, "ext", lambda: rec)
    monkeypatch.setenv("MPI4DL_NO_OVERLAP", "1")
    direct = _run_tiles(layout_name, kind, s, include_pad, x.cuda(), go.cuda(),
                        rec.kernels)
    tiles = direct
    label = "max" if kind == "max" else "avg"
    want = {f"{label}_fwd<3,{s}>", f"{label}_bwd<3,{s}>"}
    assert set(rec.kernels) == want, rec.kernels
    if overlap:
        monkeypatch.delenv("MPI4DL_NO_OVERLAP")
        del rec.kernels[:]
        tiles = _run_tiles(layout_name, kind, s, include_pad, x.cuda(),
                           go.cuda(), rec.kernels)
        assert set(rec.kernels) == want, rec.kernels
        # 1 interior + 4 bands forward, as many backward, per tile
        assert len(rec.kernels) == 10 * parts, len(rec.kernels)

    got = _stitch(layout, [y for y, _ in tiles])
    what = f"{layout_name} {kind} s{s} {'overlap' if overlap else 'direct'}"
    if kind == "max":
        yw, iw = po.max_fwd_ref(x, 3, s, 1)
        assert torch.equal(got, yw.bfloat16()), what
    else:
        yw, A = po.avg_fwd_ref(x, 3, s, 1, plain, include_pad)
        div = po.mask_divisor(Hg, Wg, 3, s, 1, plain, include_pad)
        extra = eps * yw.abs() * (div != 9) if overlap else None
        worst = assert_within(got, yw, A, 10, True, extra, what + " y")
        print(f"ORACLE halo {what} pad={include_pad} y {worst:.3g}")
        if overlap:
            # interior pixels: the direct path's bits
            same = _stitch(layout, [y for y, _ in direct])
            keep = (div == 9).expand_as(got)
            assert torch.equal(got[keep], same[keep]), what

    # gradients, tile by tile, against the centre crop of d/dxp
    for t, (_, gx) in enumerate(tiles):
        r, c = layout.pos(t)
        fill = float("-inf") if kind == "max" else 0.0
        xp, geom = po.tile_input(x, layout.rows, layout.cols, r, c, 1, fill)
        got_ = layout.slice_input(go, t)
        if kind == "max":
            _, idx = po.max_fwd_ref(xp, 3, s, 0)
            ref, A = po.max_bwd_ref(got_, idx, Hl + 2, Wl + 2, 3, s, 0)
            L = (-(-3 // s)) ** 2
        elif overlap:
            continue
        else:
            ref, A = po.avg_bwd_ref(got_, Hl + 2, Wl + 2, 3, s, 0, geom,
                                    include_pad)
            L = (-(-3 // s)) ** 2 + 2
        ref, A = ref[:, :, 1:-1, 1:-1], A[:, :, 1:-1, 1:-1]
        if kind == "max":
            assert torch.equal(gx, ref.bfloat16()), (what, t)
        else:
            assert_within(gx, ref, A, L, True, None, f"{what} tile {t} gx")
