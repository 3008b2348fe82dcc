"""Per-element fp64 oracle for the native pooling kernels.

Shared by ``test_pool_oracle.py`` (CPU: the oracle checks itself) and
``test_gpu_pool_exact.py`` (MI355X: every kernel path against it).

* ``Case`` / ``CASES``: the case matrix, each case labelled by hand with
  the forward and backward kernel it must reach (``fwd+bwd``).
* ``expected_path``: what production code picks, asked of the built
  extension's ``pool_kernel_name``, which runs the chooser the bindings
  launch from. No GPU is needed, but the extension must be built.
* ``max_fwd_ref`` .. ``avg_bwd_ref``: float64 on the CPU from the
  dtype-rounded inputs, written with ``F.unfold`` / ``F.fold`` so that
  they share nothing with the kernels or with torch's own pooling.
* ``tile_input``: what ``halo_pad`` delivers for tile (r, c) of a grid.
* ``emulate``: what a correct kernel computes (sequential fp32 sums over
  shifted slices, one division, one rounding); a second, independent
  implementation that the CPU tests hold against the reference and turn
  into mutants.
* ``check_case``: the per-element requirement.

The bound. ``ref`` is the exact result and ``A`` the same operation on
absolute values. With ``eps`` the unit roundoff of the output format
(2^-8 bf16, 2^-11 fp16, 0 for fp32 and for fp64, whose kernels compute
in fp32) every leg but max ``y`` must satisfy

    |got - ref| <= eps * |ref| + 2 * L * 2^-24 * A

and is an exact zero where ``A == 0``. L counts the fp32 roundings:

* max ``gi``: an input lies in at most ceil(k/s)^2 windows; their
  gradients are added in fp32 (the first addition, to 0, is exact):
  L = ceil(k/s)^2.
* avg ``y``: k*k - 1 inexact additions and one division; the issue's
  L = k*k + 1 is kept, which also covers the fp64 inputs' conversion to
  fp32.
* avg ``gi``: each of the at most ceil(k/s)^2 terms is ``g / div`` (one
  rounding) or ``g * (1/9f)`` (the rounded reciprocal and the product:
  two), and fewer than ceil(k/s)^2 inexact additions follow:
  L = ceil(k/s)^2 + 2.

fp16 has a narrow exponent range: below its smallest normal number,
2^-14, the spacing is 2^-24 whatever the value, so the final rounding
of such a result costs up to 2^-25 and not eps * |ref|. fp16 legs carry
that absolute term where |ref| < 2^-14 (and A > 0; a structural zero
stays exact). bf16 shares fp32's exponent range and needs none.

max ``y`` is a maximum of representable values: it must equal the
reference bit for bit (for fp64 inputs: the reference rounded to fp32,
rounding being monotonic), may never be -inf, and ``idx`` must be the
first maximum in kh-major, kw-minor order.
"""

from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from conv_oracle import _Recorder, assert_within
from test_pool_fast import SHAPES_S1, SHAPES_S2

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16,
          "fp32": torch.float32, "fp64": torch.float64}
EPS = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 0.0, "fp64": 0.0}
ITEMSIZE = {"bf16": 2, "fp16": 2, "fp32": 4, "fp64": 8}

# Every kernel the four bindings can launch.
ALL_POOL_PATHS = [
    "vec:max3_fwd<1>", "vec:max3_fwd<2>", "vec:max2s2_fwd",
    "vec:max3s1_bwd", "vec:max3s2_bwd", "vec:max2s2_bwd",
    "vec:avg3s1_fwd", "vec:avg3s1_bwd",
    "max_fwd<3,1>", "max_fwd<3,2>", "max_fwd<2,2>", "max_fwd<0,0>",
    "max_bwd<3,1>", "max_bwd<3,2>", "max_bwd<2,2>", "max_bwd<0,0>",
    "avg_fwd<3,1>", "avg_fwd<3,2>", "avg_fwd<0,0>",
    "avg_bwd<3,1>", "avg_bwd<3,2>", "avg_bwd<0,0>",
]


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


# ---------------------------------------------------------------------------
# Reference: float64, unfold / fold
# ---------------------------------------------------------------------------

def _windows(x, k, s, p, fill):
    """(N, C, H, W) -> (N*C, k*k, OH*OW): every window as a column, taps
    in kh-major, kw-minor order; pad cells hold ``fill``."""
    N, C, H, W = x.shape
    xp = F.pad(x.reshape(N * C, 1, H, W), (p, p, p, p), value=fill)
    return F.unfold(xp, k, stride=s)


def _fold(cols, H, W, k, s, p):
    """Transpose of ``_windows``: sums (NC, k*k, L) back onto the padded
    plane and crops the pad. -> (NC, H, W)"""
    g = F.fold(cols, (H + 2 * p, W + 2 * p), k, stride=s)
    return g[:, 0, p:p + H, p:p + W]


def max_fwd_ref(x, k, s, p):
    """(y, idx) in float64 / uint8. argmax returns the first maximum,
    which is the kernels' rule (strict > while scanning kh, then kw)."""
    N, C, H, W = x.shape
    OH, OW = out_size(H, k, s, p), out_size(W, k, s, p)
    cols = _windows(x.double(), k, s, p, float("-inf"))
    idx = cols.argmax(1)
    y = cols.gather(1, idx[:, None, :])[:, 0]
    return (y.reshape(N, C, OH, OW),
            idx.to(torch.uint8).reshape(N, C, OH, OW))


def max_bwd_ref(go, idx, H, W, k, s, p):
    """(gi, A): go scattered to the winning tap of every window."""
    N, C, OH, OW = go.shape
    sel = idx.reshape(N * C, 1, OH * OW).long()

    def route(g):
        z = torch.zeros(N * C, k * k, OH * OW, dtype=torch.float64)
        z.scatter_(1, sel, g.reshape(N * C, 1, OH * OW))
        return _fold(z, H, W, k, s, p).reshape(N, C, H, W)
    g = go.double()
    return route(g), route(g.abs())


def mask_divisor(H, W, k, s, p, geom, include_pad):
    """(OH, OW) float64 divisor: the window sum of a 0/1 mask of "this
    cell of the padded input lies inside the global image". Cell (i, j)
    of the padded input is global (gr0 + i, gc0 + j)."""
    OH, OW = out_size(H, k, s, p), out_size(W, k, s, p)
    if include_pad:
        return torch.full((OH, OW), float(k * k), dtype=torch.float64)
    gr0, gc0, Hg, Wg = geom
    rows = torch.tensor([0 <= gr0 + i < Hg for i in range(H + 2 * p)])
    cols = torch.tensor([0 <= gc0 + j < Wg for j in range(W + 2 * p)])
    mask = (rows[:, None] & cols[None, :]).double()[None, None]
    div = F.unfold(mask, k, stride=s).sum(1).reshape(OH, OW)
    assert bool((div > 0).all()), "a window wholly outside the image"
    return div


def avg_fwd_ref(x, k, s, p, geom, include_pad):
    """(y, A)"""
    N, C, H, W = x.shape
    OH, OW = out_size(H, k, s, p), out_size(W, k, s, p)
    div = mask_divisor(H, W, k, s, p, geom, include_pad)

    def op(t):
        return _windows(t, k, s, p, 0.0).sum(1).reshape(N, C, OH, OW) / div
    xd = x.double()
    return op(xd), op(xd.abs())


def avg_bwd_ref(go, H, W, k, s, p, geom, include_pad):
    """(gi, A): go / div handed to every tap of its window."""
    N, C, OH, OW = go.shape
    div = mask_divisor(H, W, k, s, p, geom, include_pad)

    def op(g):
        gd = (g / div).reshape(N * C, 1, OH * OW).expand(-1, k * k, -1)
        return _fold(gd.contiguous(), H, W, k, s, p).reshape(N, C, H, W)
    g = go.double()
    return op(g), op(g.abs())


# ---------------------------------------------------------------------------
# Tiles
# ---------------------------------------------------------------------------

def tile_input(xg, rows, cols, r, c, h, fill):
    """What halo_pad delivers for tile (r, c) of a rows x cols grid over
    the global image ``xg``: the tile plus its ring of width h, neighbour
    pixels where there is a neighbour and ``fill`` outside the image.
    -> (xp, (gr0, gc0, Hg, Wg)) with (gr0, gc0) the global position of
    xp[0, 0]."""
    Hg, Wg = xg.shape[-2:]
    assert Hg % rows == 0 and Wg % cols == 0
    Hl, Wl = Hg // rows, Wg // cols
    gp = F.pad(xg, (h, h, h, h), value=fill)
    xp = gp[:, :, r * Hl:r * Hl + Hl + 2 * h, c * Wl:c * Wl + Wl + 2 * h]
    return xp.contiguous(), (r * Hl - h, c * Wl - h, Hg, Wg)


class GlobalImageExchanger:
    """Stands in for a HaloExchanger on one device: the ring of a padded
    tile is filled from a global image the test holds. No process group."""

    def __init__(self, layout, tile, image):
        self.neigh = layout.neighbours(tile)
        self._pos = layout.pos(tile)
        self._image = image

    def exchange_padded(self, xp, h, off=None, nominal=None):
        hh, hw = (h, h) if isinstance(h, int) else h
        Hg, Wg = self._image.shape[-2:]
        H, W = xp.shape[-2] - 2 * hh, xp.shape[-1] - 2 * hw
        r0, c0 = self._pos[0] * H - hh, self._pos[1] * W - hw
        rl, rh = max(r0, 0), min(r0 + H + 2 * hh, Hg)
        cl, ch = max(c0, 0), min(c0 + W + 2 * hw, Wg)
        xp[:, :, rl - r0:rh - r0, cl - c0:ch - c0].copy_(
            self._image[:, :, rl:rh, cl:ch])

    def exchange_padded_async(self, xp, h):
        self.exchange_padded(xp, h)
        return lambda: None


# ---------------------------------------------------------------------------
# The case matrix
# ---------------------------------------------------------------------------

@dataclass(frozen=True)
class Case:
    """One pool problem as the bindings get it: an (N, C, H, W) tensor,
    (k, s, p), and for avg the global geometry. ``tile`` = (rows, cols,
    r, c) says the tensor is tile (r, c) of a grid with its halo ring
    (then p == 0 and H, W include the ring). ``path`` is the hand-written
    ``fwd+bwd`` kernel label."""

    group: str
    name: str
    op: str
    path: str
    dtype: str
    k: int
    s: int
    p: int
    N: int
    C: int
    H: int
    W: int
    geom: Optional[Tuple[int, int, int, int]] = None
    include_pad: bool = True
    tile: Optional[Tuple[int, int, int, int]] = None
    xkind: str = "randn"     # randn | ints | const | neg
    gokind: str = "randn"    # randn | ints
    strided_go: bool = False  # go is channels 2:5 of a 9-channel tensor

    @property
    def id(self):
        return f"{self.group}-{self.name}"

    @property
    def OH(self):
        return out_size(self.H, self.k, self.s, self.p)

    @property
    def OW(self):
        return out_size(self.W, self.k, self.s, self.p)

    @property
    def geometry(self):
        """(gr0, gc0, Hg, Wg); a plain pool is its own global image."""
        return self.geom or (-self.p, -self.p, self.H, self.W)


def _gen(label, k, s):
    return f"{label}_fwd<{k},{s}>+{label}_bwd<{k},{s}>"


# Widths of SHAPES_S2 at which a stride-2 pool has OW % 8 == 0.
S2_VEC_WIDTHS = {16, 32, 48, 64, 128, 272}

# (H_loc, W_loc) -> xp 6x8 (one partial 8-chunk), 8x18 (two chunks and a
# 2-tail), 10x24 (OW 22: two chunks and a 6-tail)
TILE_SIZES = [(4, 6), (6, 16), (8, 22)]
# (rows, cols, tiles): 2x2 all; 1x3 and 3x1 all (the middle tile has no
# image border on two sides); 3x3 centre (every divisor 9) and a corner
GRIDS = [
    (2, 2, [(0, 0), (0, 1), (1, 0), (1, 1)]),
    (1, 3, [(0, 0), (0, 1), (0, 2)]),
    (3, 1, [(0, 0), (1, 0), (2, 0)]),
    (3, 3, [(1, 1), (2, 2)]),
]
AVG_PLACEMENTS = ["plain", "q00", "q01", "q10", "q11", "centre"]


def _placement(where, H, W):
    """Global geometry of an H x W tensor pooled at p = 1 as a quarter of
    a 2H x 2W image or the centre of a 3H x 3W one."""
    if where == "plain":
        return None
    if where == "centre":
        return (H - 1, W - 1, 3 * H, 3 * W)
    r, c = int(where[1]), int(where[2])
    return (r * H - 1, c * W - 1, 2 * H, 2 * W)


def _tile_case(group, op, dtype, s, grid, rc, size, **kw):
    rows, cols = grid
    (r, c), (Hl, Wl) = rc, size
    include_pad = kw.get("include_pad", True)
    label = "max" if op == "max" else "avg"
    name = (f"{op}{'' if include_pad else '-nopad'}-g{rows}x{cols}-t{r}{c}-"
            f"{Hl}x{Wl}-s{s}-{dtype}")
    if kw.get("xkind", "randn") != "randn":
        name += "-" + kw["xkind"]
    return Case(group, name, op, _gen(label, 3, s), dtype, 3, s, 0, 2, 3,
                Hl + 2, Wl + 2,
                geom=(r * Hl - 1, c * Wl - 1, rows * Hl, cols * Wl),
                tile=(rows, cols, r, c), **kw)


def _build_cases():
    cases = []
    ops = [("max", True), ("avg", True), ("avg", False)]

    # --- tile geometry: what HaloPool2d sends when it is tiled -----------
    for rows, cols, tiles in GRIDS:
        dts = ("bf16", "fp16", "fp32") if (rows, cols) == (2, 2) else ("bf16",)
        for rc in tiles:
            for size in TILE_SIZES:
                for s in (1, 2):
                    for op, ip in ops:
                        for dt in dts:
                            cases.append(_tile_case(
                                "tile", op, dt, s, (rows, cols), rc, size,
                                include_pad=ip))
    # --- tile max on inputs with ties, constants, negatives --------------
    for rc in GRIDS[0][2]:
        for s in (1, 2):
            for xkind in ("ints", "const", "neg"):
                cases.append(_tile_case(
                    "tilemax", "max", "bf16", s, (2, 2), rc, (6, 16),
                    xkind=xkind, gokind="ints"))
    # --- the slabs of the overlap path: OH = 1, and W = 3 with OW = 1 ----
    for H, W in ((3, 8), (3, 18), (6, 3), (16, 3)):
        for op in ("max", "avg"):
            cases.append(Case("band", f"{op}-{H}x{W}", op, _gen(op, 3, 1),
                              "bf16", 3, 1, 0, 2, 3, H, W))
    # --- plain, vectorised ------------------------------------------------
    for dt in ("bf16", "fp16"):
        for (n, c, h, w) in SHAPES_S1:
            cases.append(Case(
                "vec", f"max311-{n}x{c}x{h}x{w}-{dt}", "max",
                "vec:max3_fwd<1>+vec:max3s1_bwd", dt, 3, 1, 1, n, c, h, w))
            for ip in (True, False):
                for where in AVG_PLACEMENTS:
                    cases.append(Case(
                        "vec", f"avg311{'' if ip else '-nopad'}-{where}-"
                        f"{n}x{c}x{h}x{w}-{dt}", "avg",
                        "vec:avg3s1_fwd+vec:avg3s1_bwd", dt, 3, 1, 1, n, c,
                        h, w, geom=_placement(where, h, w), include_pad=ip))
        for (n, c, h, w) in SHAPES_S2:
            fast = w in S2_VEC_WIDTHS
            cases.append(Case(
                "vec", f"max321-{n}x{c}x{h}x{w}-{dt}", "max",
                "vec:max3_fwd<2>+vec:max3s2_bwd" if fast else _gen("max", 3, 2),
                dt, 3, 2, 1, n, c, h, w))
            cases.append(Case(
                "vec", f"max220-{n}x{c}x{h}x{w}-{dt}", "max",
                "vec:max2s2_fwd+vec:max2s2_bwd" if fast else _gen("max", 2, 2),
                dt, 2, 2, 0, n, c, h, w))
    # --- plain, generic kernels on 2-byte dtypes: W % 8 != 0, odd H ------
    for dt in ("bf16", "fp16"):
        for (n, c, h, w) in ((2, 3, 9, 12), (1, 3, 9, 20)):
            for k, s, p in ((3, 1, 1), (3, 2, 1), (2, 2, 0)):
                cases.append(Case(
                    "generic2b", f"max{k}{s}{p}-{n}x{c}x{h}x{w}-{dt}", "max",
                    _gen("max", k, s), dt, k, s, p, n, c, h, w))
            for s in (1, 2):
                for ip in (True, False):
                    cases.append(Case(
                        "generic2b", f"avg3{s}1{'' if ip else '-nopad'}-"
                        f"{n}x{c}x{h}x{w}-{dt}", "avg", _gen("avg", 3, s),
                        dt, 3, s, 1, n, c, h, w, include_pad=ip))
    # --- runtime (k, s): the <0,0> instantiations --------------------------
    for dt in ("bf16", "fp32"):
        for k, s, p in ((2, 1, 0), (5, 1, 2), (4, 2, 1), (3, 3, 0)):
            for op, ip in ops:
                cases.append(Case(
                    "runtimek", f"{op}{'' if ip else '-nopad'}-k{k}s{s}p{p}-"
                    f"{dt}", op, _gen(op, 0, 0), dt, k, s, p, 2, 3, 9, 20,
                    include_pad=ip))
    # --- go as a channel slice of a wider tensor, tile geometry ----------
    for s in (1, 2):
        for op, ip in (("max", True), ("avg", False)):
            cases.append(_tile_case(
                "stridedgo", op, "bf16", s, (2, 2), (0, 0), (6, 16),
                include_pad=ip, strided_go=True))
    # --- fp64 tensors: the kernels compute in fp32, so the results are
    # held to the fp32 bound (eps = 0), not to an fp64 one ----------------
    cases.append(Case("fp64", "max311", "max", _gen("max", 3, 1), "fp64",
                      3, 1, 1, 2, 3, 9, 20))
    cases.append(Case("fp64", "avg311-nopad", "avg", _gen("avg", 3, 1),
                      "fp64", 3, 1, 1, 2, 3, 9, 20, include_pad=False))
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids), "duplicate case id"
    return cases


CASES = _build_cases()
CASE_BY_ID = {c.id: c for c in CASES}

# one per kernel, run twice for bit-identical outputs (no atomics)
DETERMINISM_IDS = [
    "tile-max-g2x2-t00-8x22-s1-bf16",
    "tile-max-g2x2-t11-8x22-s2-bf16",
    "tile-avg-nopad-g2x2-t01-8x22-s1-bf16",
    "tile-avg-nopad-g2x2-t10-8x22-s2-bf16",
    "generic2b-max220-2x3x9x12-bf16",
    "runtimek-max-k5s1p2-bf16",
    "runtimek-avg-nopad-k4s2p1-bf16",
    "vec-max311-2x5x16x64-bf16",
    "vec-max321-2x5x16x64-bf16",
    "vec-max220-2x5x16x64-bf16",
    "vec-avg311-nopad-q11-2x5x16x64-bf16",
]


def expected_path(case, ge):
    """``fwd+bwd`` as the extension's chooser names them for this case."""
    go_bs = 9 * case.OH * case.OW if case.strided_go else 0
    args = (ITEMSIZE[case.dtype], case.H, case.W, case.k, case.s, case.p)
    return (ge.pool_kernel_name(case.op + "_fwd", *args) + "+" +
            ge.pool_kernel_name(case.op + "_bwd", *args, True, go_bs))


# ---------------------------------------------------------------------------
# Inputs, reference
# ---------------------------------------------------------------------------

def _values(kind, shape, gen):
    if kind == "randn":
        return torch.randn(shape, generator=gen, dtype=torch.float64)
    if kind == "ints":
        return torch.randint(0, 3, shape, generator=gen).double()
    if kind == "const":
        return torch.full(shape, 1.5, dtype=torch.float64)
    assert kind == "neg", kind
    return -torch.rand(shape, generator=gen, dtype=torch.float64) - 0.5


@functools.lru_cache(maxsize=None)
def global_image(N, C, Hg, Wg, dtype, xkind):
    """The image the tiles of a grid are cut from, shared by its tiles."""
    gen = torch.Generator().manual_seed(
        zlib.crc32(f"{N},{C},{Hg},{Wg},{dtype},{xkind}".encode()))
    return _values(xkind, (N, C, Hg, Wg), gen).to(DTYPES[dtype])


def make_inputs(case):
    """(x, go) in the case's dtype, fixed seed per case."""
    gen = torch.Generator().manual_seed(zlib.crc32(case.id.encode()))
    dt = DTYPES[case.dtype]
    if case.tile:
        rows, cols, r, c = case.tile
        _, _, Hg, Wg = case.geom
        img = global_image(case.N, case.C, Hg, Wg, case.dtype, case.xkind)
        fill = float("-inf") if case.op == "max" else 0.0
        x, geom = tile_input(img, rows, cols, r, c, 1, fill)
        assert geom == case.geom and x.shape[-2:] == (case.H, case.W)
    else:
        x = _values(case.xkind, (case.N, case.C, case.H, case.W), gen).to(dt)
    shape = (case.N, case.C, case.OH, case.OW)
    if case.gokind == "ints":
        go = torch.randint(-4, 5, shape, generator=gen).to(dt)
    else:
        go = torch.randn(shape, generator=gen, dtype=torch.float64).to(dt)
    return x, go


def reference(case, x, go):
    """{"y": (ref, A) or ref, "idx": ref, "gi": (ref, A)} in float64."""
    k, s, p = case.k, case.s, case.p
    if case.op == "max":
        y, idx = max_fwd_ref(x, k, s, p)
        return {"y": y, "idx": idx,
                "gi": max_bwd_ref(go, idx, case.H, case.W, k, s, p)}
    g = (case.geometry, case.include_pad)
    return {"y": avg_fwd_ref(x, k, s, p, *g),
            "gi": avg_bwd_ref(go, case.H, case.W, k, s, p, *g)}


@functools.lru_cache(maxsize=None)
def case_data(case):
    """(inputs, reference) of a case, computed once and shared."""
    inputs = make_inputs(case)
    return inputs, reference(case, *inputs)


def leg_length(case, leg):
    """L of the bound (module docstring)."""
    per_axis = -(-case.k // case.s)
    if case.op == "max":
        return per_axis ** 2
    return case.k * case.k + 1 if leg == "y" else per_axis ** 2 + 2


# ---------------------------------------------------------------------------
# Emulation: sequential fp32 over shifted slices
# ---------------------------------------------------------------------------

def clamp_divisor(case, geom=None):
    """(OH, OW) fp32 divisor by clamping the window against the global
    image: the kernels' formula, independent of ``mask_divisor``."""
    k, s = case.k, case.s
    if case.include_pad:
        return torch.full((case.OH, case.OW), float(k * k))
    gr0, gc0, Hg, Wg = geom or case.geometry
    r0 = gr0 + torch.arange(case.OH) * s
    c0 = gc0 + torch.arange(case.OW) * s
    rc = (r0 + k).clamp(max=Hg) - r0.clamp(min=0)
    cc = (c0 + k).clamp(max=Wg) - c0.clamp(min=0)
    return (rc[:, None] * cc[None, :]).clamp(min=1).float()


def _taps(case):
    """(t, row slice, col slice) of every tap on the padded input."""
    k, s = case.k, case.s
    for kh in range(k):
        for kw in range(k):
            yield (kh * k + kw,
                   slice(kh, kh + s * (case.OH - 1) + 1, s),
                   slice(kw, kw + s * (case.OW - 1) + 1, s))


def round_to(t32, dtype):
    return t32.to(DTYPES[dtype])


def emulate(case, x, go, div=None, shortcut=None, skip_tap=None,
            last_max=False, rounder=round_to):
    """What a correct kernel returns, {"y", "idx"?, "gi"} in the case's
    dtype. The keyword arguments turn it into the mutants of
    ``test_pool_oracle.py``: another divisor, the 1/(k*k) shortcut on
    chosen windows, one tap left out, the last maximum, another final
    rounding."""
    k, p = case.k, case.p
    pad = (p, p, p, p)
    shape = (case.N, case.C, case.H + 2 * p, case.W + 2 * p)
    gof = go.float()
    if case.op == "max":
        xp = F.pad(x.float(), pad, value=float("-inf"))
        best = torch.full(gof.shape, float("-inf"))
        bidx = torch.zeros(gof.shape, dtype=torch.uint8)
        for t, rs, cs in _taps(case):
            if t == skip_tap:
                continue
            v = xp[:, :, rs, cs]
            m = (v >= best) if last_max else (v > best)
            best = torch.where(m, v, best)
            bidx = torch.where(m, torch.tensor(t, dtype=torch.uint8), bidx)
        gp = torch.zeros(shape)
        for t, rs, cs in _taps(case):
            gp[:, :, rs, cs] += gof * (bidx == t)
        gi = gp[:, :, p:p + case.H, p:p + case.W]
        return {"y": rounder(best, case.dtype), "idx": bidx,
                "gi": rounder(gi, case.dtype)}
    if div is None:
        div = clamp_divisor(case)
    xp = F.pad(x.float(), pad)
    acc = torch.zeros(gof.shape)
    for t, rs, cs in _taps(case):
        if t != skip_tap:
            acc += xp[:, :, rs, cs]
    if shortcut is None:
        shortcut = div == float(k * k)
    inv_kk = torch.tensor(1.0) / float(k * k)
    gd = torch.where(shortcut, gof * inv_kk, gof / div)
    gp = torch.zeros(shape)
    for t, rs, cs in _taps(case):
        if t != skip_tap:
            gp[:, :, rs, cs] += gd
    gi = gp[:, :, p:p + case.H, p:p + case.W]
    return {"y": rounder(acc / div, case.dtype), "gi": rounder(gi, case.dtype)}


# ---------------------------------------------------------------------------
# The requirement
# ---------------------------------------------------------------------------

def _format_term(case, ref, A, extra):
    """``extra`` plus the fp16 underflow term (module docstring)."""
    if case.dtype != "fp16":
        return extra
    under = 2.0 ** -25 * ((ref.abs() < 2.0 ** -14) & (A > 0))
    return under if extra is None else extra + under


def _as_kernel_dtype(ref, dtype):
    """The exact reference as a correct kernel stores it: an fp64 tensor
    went through fp32 on the way."""
    return ref.float().double() if dtype == "fp64" else ref.to(DTYPES[dtype])


def _assert_equal(got, want, what):
    if got.shape != want.shape or not torch.equal(got, want):
        bad = (got != want).nonzero() if got.shape == want.shape else []
        first = tuple(bad[0].tolist()) if len(bad) else None
        raise AssertionError(
            f"{what}: {len(bad)} of {want.numel()} elements differ, first at "
            f"{first}" + (f": got {got[first]}, want {want[first]}"
                          if first else f" (shape {tuple(got.shape)})"))


def check_case(case, results, what="", extra=None):
    """Every leg of a case against the reference; {leg: worst err/bound}.
    ``extra`` maps a leg to a derived additional bound term."""
    _, ref = case_data(case)
    what = what or f"{case.id} [{case.path}]"
    eps = EPS[case.dtype]
    extra = extra or {}
    worst = {}
    if case.op == "max":
        y = results["y"].detach().cpu()
        ninf = (y == float("-inf")).nonzero()
        if len(ninf):
            raise AssertionError(f"{what} y: {len(ninf)} values are -inf, "
                                 f"first at {tuple(ninf[0].tolist())}")
        _assert_equal(y, _as_kernel_dtype(ref["y"], case.dtype), what + " y")
        _assert_equal(results["idx"].detach().cpu(), ref["idx"],
                      what + " idx")
        worst["y"] = 0.0
    else:
        r, A = ref["y"]
        worst["y"] = assert_within(
            results["y"], r, A, leg_length(case, "y"), False,
            _format_term(case, r, A, extra.get("y")), what + " y", eps=eps)
    r, A = ref["gi"]
    worst["gi"] = assert_within(
        results["gi"], r, A, leg_length(case, "gi"), False,
        _format_term(case, r, A, extra.get("gi")), what + " gi", eps=eps)
    if case.op == "max" and case.gokind == "ints":
        # small integers: every sum is exact in fp32 and in the dtype
        _assert_equal(results["gi"].detach().cpu(),
                      _as_kernel_dtype(r, case.dtype), what + " gi")
    return worst


# ---------------------------------------------------------------------------
# Running a case on the GPU
# ---------------------------------------------------------------------------

def _aligned(*tensors):
    return all(t.data_ptr() % 16 == 0 and t.numel() > 0 for t in tensors)


class PoolRecorder(_Recorder):
    """Notes, for every pool binding called, the kernel the extension
    names for that call's own tensors and integers."""

    def _name(self, op, t, H, W, k, s, p, aligned, go_bs=0):
        return self._ge.pool_kernel_name(op, t.element_size(), H, W, k, s, p,
                                         aligned, go_bs)

    def _label_maxpool_fwd(self, out, x, k, s, p):
        return self._name("max_fwd", x, x.shape[2], x.shape[3], k, s, p,
                          _aligned(x, *out))

    def _label_maxpool_bwd(self, gi, go, idx, H, W, k, s, p):
        return self._name("max_bwd", go, H, W, k, s, p,
                          _aligned(go, idx, gi),
                          0 if go.is_contiguous() else go.stride(0))

    def _label_avgpool_fwd(self, y, x, k, s, p, gr0, gc0, Hg, Wg, ip):
        return self._name("avg_fwd", x, x.shape[2], x.shape[3], k, s, p,
                          _aligned(x, y))

    def _label_avgpool_bwd(self, gi, go, H, W, k, s, p, gr0, gc0, Hg, Wg, ip):
        return self._name("avg_bwd", go, H, W, k, s, p, _aligned(go, gi),
                          0 if go.is_contiguous() else go.stride(0))


def run_gpu(case, kernels=None):
    """The case's forward and backward binding once each on the GPU;
    results as CPU tensors. ``kernels`` receives the recorder's labels."""
    from mpi4dl_amd.ops import backend

    ge = PoolRecorder(backend.ext())
    if kernels is not None:
        ge.kernels = kernels
    (x, go), _ = case_data(case)
    xg, gog = x.cuda(), go.cuda()
    if case.strided_go:
        big = torch.zeros(case.N, 9, case.OH, case.OW, dtype=go.dtype,
                          device="cuda")
        big[:, 2:5] = gog
        gog = big[:, 2:5]
        assert not gog.is_contiguous()
    geo = (case.H, case.W, case.k, case.s, case.p)
    if case.op == "max":
        y, idx = ge.maxpool_fwd(xg, case.k, case.s, case.p)
        out = {"y": y, "idx": idx, "gi": ge.maxpool_bwd(gog, idx, *geo)}
    else:
        g = (*case.geometry, case.include_pad)
        out = {"y": ge.avgpool_fwd(xg, case.k, case.s, case.p, *g),
               "gi": ge.avgpool_bwd(gog, *geo, *g)}
    torch.cuda.synchronize()
    return {leg: t.cpu() for leg, t in out.items()}
