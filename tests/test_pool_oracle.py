"""The pooling oracle checks itself (CPU, no GPU needed).

* the unfold / fold reference reproduces torch's own pooling in fp64;
* a correct kernel, emulated as sequential fp32 sums over shifted
  slices with one division and one rounding, stays within the derived
  bound on every leg of every case (the peak per leg is printed);
* kernels that are subtly wrong are rejected;
* the per-tile references of every grid, put side by side, are the
  whole-image reference, and ``HaloPool2d._avg_divisors`` is the mask
  divisor;
* every case's label is what the built extension's chooser picks, and
  the matrix reaches every pool kernel;
* the bindings reject impossible geometry before they touch a device;
* ``HaloPool2d`` with ``count_include_pad=False`` rounds interior pixels
  once on its CPU paths too.
"""

import pytest
import torch
import torch.nn.functional as F

import pool_oracle as po
from conv_oracle import assert_within

CASE_IDS = [c.id for c in po.CASES]


def _extension_or_skip():
    """Never skips for want of a GPU: only when the tree is not built."""
    try:
        from mpi4dl_amd import _gemscore
        return _gemscore
    except ImportError as e:
        pytest.skip("mpi4dl_amd._gemscore is not built: run `PYTORCH_ROCM_ARCH="
                    f"gfx950 python setup.py build_ext --inplace` ({e})")


# --- labels ------------------------------------------------------------------

@pytest.mark.parametrize("cid", CASE_IDS)
def test_pool_label_matches_dispatch(cid):
    ge = _extension_or_skip()
    case = po.CASE_BY_ID[cid]
    assert po.expected_path(case, ge) == case.path


def test_every_pool_path_is_covered():
    _extension_or_skip()
    reached = set()
    for case in po.CASES:
        reached.update(case.path.split("+"))
    assert len(set(po.ALL_POOL_PATHS)) == len(po.ALL_POOL_PATHS)
    assert reached == set(po.ALL_POOL_PATHS), (
        sorted(reached - set(po.ALL_POOL_PATHS)),
        sorted(set(po.ALL_POOL_PATHS) - reached))
    det = set()
    for cid in po.DETERMINISM_IDS:
        det.update(po.CASE_BY_ID[cid].path.split("+"))
    assert det == set(po.ALL_POOL_PATHS), sorted(set(po.ALL_POOL_PATHS) - det)


def test_pool_label_follows_alignment_and_go_stride():
    """The two arguments of the chooser that no case varies."""
    ge = _extension_or_skip()
    args = (2, 16, 64, 3, 1, 1)
    assert ge.pool_kernel_name("avg_bwd", *args) == "vec:avg3s1_bwd"
    assert ge.pool_kernel_name("avg_bwd", *args, False) == "avg_bwd<3,1>"
    assert ge.pool_kernel_name("avg_bwd", *args, True, 9 * 16 * 64) == \
        "vec:avg3s1_bwd"
    assert ge.pool_kernel_name("max_bwd", *args, True, 16 * 64 + 4) == \
        "max_bwd<3,1>"
    assert ge.pool_kernel_name("max_fwd", 4, 16, 64, 3, 1, 1) == "max_fwd<3,1>"
    with pytest.raises(RuntimeError, match="op must be"):
        ge.pool_kernel_name("min_fwd", *args)


# --- the reference against torch's pooling, fp64 -----------------------------

@pytest.mark.parametrize("k,s,p", [(3, 1, 1), (3, 2, 1), (2, 2, 0), (5, 1, 2)])
def test_reference_reproduces_torch(k, s, p):
    gen = torch.Generator().manual_seed(k * 100 + s * 10 + p)
    x = torch.randn(2, 3, 9, 14, generator=gen, dtype=torch.float64)
    y, idx = po.max_fwd_ref(x, k, s, p)
    go = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    xt = x.clone().requires_grad_(True)
    yt = F.max_pool2d(xt, k, s, padding=p)
    assert torch.equal(y, yt.detach())
    (gt,) = torch.autograd.grad(yt, xt, go)
    gi, _ = po.max_bwd_ref(go, idx, 9, 14, k, s, p)
    assert torch.allclose(gi, gt, rtol=0, atol=1e-14)
    for include_pad in (True, False):
        ya, _ = po.avg_fwd_ref(x, k, s, p, (-p, -p, 9, 14), include_pad)
        xt = x.clone().requires_grad_(True)
        yt = F.avg_pool2d(xt, k, s, padding=p, count_include_pad=include_pad)
        assert torch.allclose(ya, yt.detach(), rtol=0, atol=1e-14)
        (gt,) = torch.autograd.grad(yt, xt, go)
        ga, _ = po.avg_bwd_ref(go, 9, 14, k, s, p, (-p, -p, 9, 14),
                               include_pad)
        assert torch.allclose(ga, gt, rtol=0, atol=1e-14)


# --- emulation ---------------------------------------------------------------

_PEAK = {}


@pytest.mark.parametrize("cid", CASE_IDS)
def test_emulation_within_bound(cid):
    case = po.CASE_BY_ID[cid]
    (x, go), _ = po.case_data(case)
    worst = po.check_case(case, po.emulate(case, x, go))
    assert all(v <= 1.0 for v in worst.values()), worst
    for leg, v in worst.items():
        key = f"{case.op} {leg}"
        _PEAK[key] = max(_PEAK.get(key, 0.0), v)


def test_emulation_peak_report():
    """Prints the largest err/bound of the emulation per leg (run after
    the cases above; `-s` shows it)."""
    for key in sorted(_PEAK):
        print(f"EMULATION PEAK {key} {_PEAK[key]:.3g}")
    assert all(v <= 1.0 for v in _PEAK.values())


# --- mutants -----------------------------------------------------------------

def _truncate(t32, dtype):
    """Chop instead of round-to-nearest (bf16: drop 16 bits)."""
    assert dtype == "bf16"
    return (t32.float().contiguous().view(torch.int32) & -65536).view(
        torch.float32).bfloat16()


def _rejected(case, results, match="over the bound|differ"):
    with pytest.raises(AssertionError, match=match):
        po.check_case(case, results)


def _good(case):
    (x, go), _ = po.case_data(case)
    out = po.emulate(case, x, go)
    po.check_case(case, out)
    return x, go, out


AVG_BORDER_TILES = [
    "tile-avg-nopad-g2x2-t00-6x16-s1-bf16",
    "tile-avg-nopad-g2x2-t00-8x22-s2-bf16",
    "tile-avg-nopad-g1x3-t01-6x16-s1-bf16",
    "tile-avg-nopad-g3x3-t22-4x6-s1-bf16",
    "tile-avg-nopad-g2x2-t01-6x16-s1-fp32",
]


@pytest.mark.parametrize("cid", AVG_BORDER_TILES)
def test_avg_divisor_mutants_are_rejected(cid):
    case = po.CASE_BY_ID[cid]
    x, go, good = _good(case)
    div = po.clamp_divisor(case)
    assert bool((div != 9).any())
    # the divisor clipped against the tile instead of the global image
    tile_div = po.clamp_divisor(case, (0, 0, case.H, case.W))
    bad = po.emulate(case, x, go, div=tile_div)
    _rejected(case, {**good, "y": bad["y"]})
    _rejected(case, {**good, "gi": bad["gi"]})
    # k*k on one image border (the first one this tile has)
    one = div.clone()
    rows, cols, r, c = case.tile
    if r == 0:
        one[0, :] = 9.0
    elif r == rows - 1:
        one[-1, :] = 9.0
    elif c == 0:
        one[:, 0] = 9.0
    else:
        one[:, -1] = 9.0
    assert not torch.equal(one, div)
    bad = po.emulate(case, x, go, div=one)
    _rejected(case, {**good, "y": bad["y"]})
    _rejected(case, {**good, "gi": bad["gi"]})
    # the 1/9 shortcut applied to border windows too
    bad = po.emulate(case, x, go, shortcut=torch.ones_like(div, dtype=torch.bool))
    _rejected(case, {**good, "gi": bad["gi"]})


MUTANT_IDS = [
    "tile-avg-g2x2-t00-6x16-s1-bf16",
    "tile-avg-nopad-g2x2-t10-8x22-s2-bf16",
    "tile-max-g2x2-t01-6x16-s1-bf16",
    "tile-max-g2x2-t11-8x22-s2-bf16",
    "vec-avg311-nopad-q10-2x3x5x16-bf16",
    "vec-max311-2x3x5x16-bf16",
    "runtimek-avg-nopad-k5s1p2-bf16",
    "runtimek-max-k4s2p1-bf16",
]


@pytest.mark.parametrize("cid", MUTANT_IDS)
def test_mutants_are_rejected(cid):
    case = po.CASE_BY_ID[cid]
    x, go, good = _good(case)
    # a gradient routed one column off; an output one column off
    _rejected(case, {**good, "gi": good["gi"].roll(1, 3)})
    _rejected(case, {**good, "y": good["y"].roll(1, 3)})
    # one tap left out (the last one)
    bad = po.emulate(case, x, go, skip_tap=case.k * case.k - 1)
    _rejected(case, {**good, "y": bad["y"]})
    if case.op == "avg":
        _rejected(case, {**good, "gi": bad["gi"]})
    else:
        _rejected(case, {**bad, "y": good["y"]})   # its idx and gi
    # truncation instead of round-to-nearest
    bad = po.emulate(case, x, go, rounder=_truncate)
    _rejected(case, {**good, "gi": bad["gi"]})
    if case.op == "avg":
        _rejected(case, {**good, "y": bad["y"]})
    # one element replaced by its neighbour
    m = good["gi"].clone()
    m[1, 2, 2, 1] = m[1, 2, 2, 2] + 1
    _rejected(case, {**good, "gi": m})


@pytest.mark.parametrize("cid", [
    "tilemax-max-g2x2-t00-6x16-s1-bf16-ints",
    "tilemax-max-g2x2-t11-6x16-s2-bf16-ints",
    "tilemax-max-g2x2-t01-6x16-s1-bf16-const",
])
def test_last_maximum_is_rejected(cid):
    case = po.CASE_BY_ID[cid]
    x, go, good = _good(case)
    bad = po.emulate(case, x, go, last_max=True)
    assert torch.equal(bad["y"], good["y"])
    _rejected(case, {**good, "idx": bad["idx"]}, match="idx.*differ")
    _rejected(case, {**good, "gi": bad["gi"]})


def test_neg_inf_and_structural_zero():
    """-inf is never a legitimate max here; the -inf ring gets an exact
    zero gradient; the halo row and column a stride-2 pool leaves unused
    get an exact zero too."""
    case = po.CASE_BY_ID["tilemax-max-g2x2-t00-6x16-s1-bf16-neg"]
    x, go, good = _good(case)
    _, ref = po.case_data(case)
    assert bool((x[:, :, 0, :] == float("-inf")).all())
    assert bool((ref["gi"][1][:, :, 0, :] == 0).all())
    bad = good["y"].clone()
    bad[0, 1, 2, 3] = float("-inf")
    _rejected(case, {**good, "y": bad}, match=r"-inf.*\(0, 1, 2, 3\)")
    bad = good["gi"].clone()
    bad[1, 0, 0, 5] = 1e-30
    _rejected(case, {**good, "gi": bad}, match="err/bound inf")

    case = po.CASE_BY_ID["tile-avg-nopad-g2x2-t00-6x16-s2-bf16"]
    x, go, good = _good(case)
    _, ref = po.case_data(case)
    assert bool((ref["gi"][1][:, :, -1, :] == 0).all())
    assert bool((ref["gi"][1][:, :, :, -1] == 0).all())
    bad = good["gi"].clone()
    bad[0, 0, -1, 3] = 1e-30
    _rejected(case, {**good, "gi": bad}, match="err/bound inf")


def test_non_finite_is_rejected():
    case = po.CASE_BY_ID["tile-avg-g2x2-t00-6x16-s1-bf16"]
    x, go, good = _good(case)
    bad = good["y"].clone()
    bad[1, 2, 3, 4] = float("nan")
    _rejected(case, {**good, "y": bad}, match=r"non-finite.*\(1, 2, 3, 4\)")


# --- stitching ---------------------------------------------------------------

def _grid_images(rows, cols, Hl, Wl):
    gen = torch.Generator().manual_seed(rows * 1000 + cols * 100 + Hl)
    x = torch.randn(2, 3, rows * Hl, cols * Wl, generator=gen).bfloat16()
    return x, gen


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("size", po.TILE_SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("grid", [g[:2] for g in po.GRIDS],
                         ids=lambda v: f"{v[0]}x{v[1]}")
def test_tile_references_stitch_to_the_whole_image(grid, size, s):
    from mpi4dl_amd.ops.spatial_conv import HaloPool2d

    (rows, cols), (Hl, Wl) = grid, size
    x, gen = _grid_images(rows, cols, Hl, Wl)
    Hg, Wg = x.shape[-2:]
    plain = (-1, -1, Hg, Wg)
    OHl, OWl = Hl // s, Wl // s
    go = torch.randn(2, 3, Hg // s, Wg // s, generator=gen).bfloat16()

    def stitch(per_tile):
        return torch.cat([torch.cat([per_tile[r][c] for c in range(cols)], 3)
                          for r in range(rows)], 2)

    def scatter_add(per_tile):
        tot = torch.zeros(2, 3, Hg + 2, Wg + 2, dtype=torch.float64)
        for r in range(rows):
            for c in range(cols):
                tot[:, :, r * Hl:r * Hl + Hl + 2,
                    c * Wl:c * Wl + Wl + 2] += per_tile[r][c]
        return tot[:, :, 1:-1, 1:-1]

    def go_of(r, c):
        return go[:, :, r * OHl:(r + 1) * OHl, c * OWl:(c + 1) * OWl]

    # max
    yw, iw = po.max_fwd_ref(x, 3, s, 1)
    gw, _ = po.max_bwd_ref(go, iw, Hg, Wg, 3, s, 1)
    ys, gs = [], []
    for r in range(rows):
        ys.append([])
        gs.append([])
        for c in range(cols):
            xp, _ = po.tile_input(x, rows, cols, r, c, 1, float("-inf"))
            y, idx = po.max_fwd_ref(xp, 3, s, 0)
            assert y.shape[-2:] == (OHl, OWl)
            ys[r].append(y)
            gs[r].append(po.max_bwd_ref(go_of(r, c), idx, Hl + 2, Wl + 2,
                                        3, s, 0)[0])
    assert torch.equal(stitch(ys), yw)
    assert torch.allclose(scatter_add(gs), gw, rtol=0, atol=1e-13)

    # avg, both divisor conventions
    for include_pad in (True, False):
        yw, _ = po.avg_fwd_ref(x, 3, s, 1, plain, include_pad)
        gw, _ = po.avg_bwd_ref(go, Hg, Wg, 3, s, 1, plain, include_pad)
        ys, gs = [], []
        for r in range(rows):
            ys.append([])
            gs.append([])
            for c in range(cols):
                xp, geom = po.tile_input(x, rows, cols, r, c, 1, 0.0)
                ys[r].append(po.avg_fwd_ref(xp, 3, s, 0, geom, include_pad)[0])
                gs[r].append(po.avg_bwd_ref(go_of(r, c), Hl + 2, Wl + 2, 3, s,
                                            0, geom, include_pad)[0])
                if not include_pad:
                    method = ("vertical" if rows == 1 else
                              "horizontal" if cols == 1 else "square")
                    mod = HaloPool2d(
                        "avg", 3, s, padding=1, num_spatial_parts=rows * cols,
                        slice_method=method, spatial_local_rank=r * cols + c,
                        count_include_pad=False)
                    assert (mod.layout.rows, mod.layout.cols) == (rows, cols)
                    mine = mod._avg_divisors(OHl, OWl, Hl, Wl, "cpu")
                    assert torch.equal(
                        mine.double(),
                        po.mask_divisor(Hl + 2, Wl + 2, 3, s, 0, geom, False))
        assert torch.equal(stitch(ys), yw)
        assert torch.allclose(scatter_add(gs), gw, rtol=0, atol=1e-13)


# --- HaloPool2d's CPU paths: one rounding for interior pixels -----------------

@pytest.mark.parametrize("s,overlap", [(1, False), (2, False), (1, True)],
                         ids=["s1-direct", "s2-direct", "s1-overlap"])
def test_halo_avgpool_cpu_rounds_interior_once(s, overlap, monkeypatch):
    """count_include_pad=False on bf16 CPU tensors: the stitched tiles
    meet the single-rounding bound wherever the divisor is k*k and carry
    one more eps*|ref| on image-border pixels, which round twice
    (average to bf16, then times k*k/div to bf16)."""
    from mpi4dl_amd.ops.spatial_conv import HaloPool2d

    if overlap:
        monkeypatch.delenv("MPI4DL_NO_OVERLAP", raising=False)
    else:
        monkeypatch.setenv("MPI4DL_NO_OVERLAP", "1")
    x, _ = _grid_images(2, 2, 6, 16)
    ref, A = po.avg_fwd_ref(x, 3, s, 1, (-1, -1, 12, 32), False)
    div = po.mask_divisor(12, 32, 3, s, 1, (-1, -1, 12, 32), False)
    tiles = []
    for t in range(4):
        mod = HaloPool2d("avg", 3, s, padding=1, num_spatial_parts=4,
                         spatial_local_rank=t, grad_mode="drop",
                         count_include_pad=False)
        mod.exchanger = po.GlobalImageExchanger(mod.layout, t, x)
        tiles.append(mod(mod.layout.slice_input(x, t).contiguous()))
    got = torch.cat([torch.cat(tiles[0:2], 3), torch.cat(tiles[2:4], 3)], 2)
    assert got.dtype == torch.bfloat16
    extra = po.EPS["bf16"] * ref.abs() * (div != 9)
    assert_within(got, ref, A, 10, True, extra, "stitched avg")


# --- argument checks (CPU tensors: the checks come before the device one) -----

def test_bindings_reject_bad_geometry():
    ge = _extension_or_skip()
    x = torch.zeros(1, 1, 8, 8)
    idx = torch.zeros(1, 1, 8, 8, dtype=torch.uint8)
    plain = (-1, -1, 8, 8, True)

    def each(k, s, p, match, H=8, W=8):
        with pytest.raises(RuntimeError, match=match):
            ge.maxpool_fwd(x, k, s, p)
        with pytest.raises(RuntimeError, match=match):
            ge.avgpool_fwd(x, k, s, p, *plain)
        with pytest.raises(RuntimeError, match=match):
            ge.maxpool_bwd(x, idx, H, W, k, s, p)
        with pytest.raises(RuntimeError, match=match):
            ge.avgpool_bwd(x, H, W, k, s, p, *plain)
        with pytest.raises(RuntimeError, match=match):
            ge.pool_kernel_name("max_fwd", 2, H, W, k, s, p)

    each(0, 1, 0, "kernel size must be >= 1")
    each(3, 0, 1, "stride must be >= 1")
    each(3, -1, 1, "stride must be >= 1")
    each(3, 1, -1, "padding must be >= 0")
    each(3, 1, 2, "at most half the kernel")
    each(9, 1, 0, "kernel larger than the padded input")
    small = torch.zeros(1, 1, 2, 8)
    with pytest.raises(RuntimeError, match="kernel larger"):
        ge.maxpool_fwd(small, 5, 1, 1)
    with pytest.raises(RuntimeError, match="kernel larger"):
        ge.avgpool_fwd(small.transpose(2, 3).contiguous(), 5, 1, 1, *plain)
    with pytest.raises(RuntimeError, match="must be 4-D"):
        ge.maxpool_fwd(x[0], 3, 1, 1)
    with pytest.raises(RuntimeError, match="must be 4-D"):
        ge.avgpool_fwd(x[0], 3, 1, 1, *plain)


def test_bindings_reject_inconsistent_gradient_shape():
    ge = _extension_or_skip()
    go = torch.zeros(1, 1, 8, 8)
    idx = torch.zeros(1, 1, 8, 8, dtype=torch.uint8)
    plain = (-1, -1, 16, 16, True)
    # 16x16 at 3/2/1 gives 8x8; at 3/1/1 it gives 16x16
    with pytest.raises(RuntimeError, match="go is 8x8 but .* give 16x16"):
        ge.maxpool_bwd(go, idx, 16, 16, 3, 1, 1)
    with pytest.raises(RuntimeError, match="go is 8x8 but .* give 16x16"):
        ge.avgpool_bwd(go, 16, 16, 3, 1, 1, *plain)
    with pytest.raises(RuntimeError, match="go is 8x8 but .* give 9x8"):
        ge.avgpool_bwd(go, 18, 16, 3, 2, 1, *plain)
    with pytest.raises(RuntimeError, match="idx is 4x8 but .* give 8x8"):
        ge.maxpool_bwd(go, idx[:, :, :4].contiguous(), 16, 16, 3, 2, 1)
    with pytest.raises(RuntimeError, match="disagree on"):
        ge.maxpool_bwd(go, idx.expand(1, 2, 8, 8).contiguous(), 16, 16, 3, 2, 1)
    with pytest.raises(RuntimeError, match="must be 4-D"):
        ge.avgpool_bwd(go[0], 16, 16, 3, 2, 1, *plain)
    # consistent geometry on CPU tensors gets as far as the device check
    with pytest.raises(RuntimeError) as e:
        ge.avgpool_bwd(go, 16, 16, 3, 2, 1, *plain)
    assert "give" not in str(e.value)
