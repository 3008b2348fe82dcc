"""Per-element fp64 oracle for the native convolution kernels.

Shared by ``test_conv_oracle.py`` (CPU: the oracle checks itself) and
``test_gpu_conv_exact.py`` (MI355X: every kernel path against it).

* ``Case`` / ``CASES``: the shape matrix, each case labelled with the
  kernels it must reach.
* ``expected_path``: what production code picks for a case, asked of
  ``conv_native.conv_plan`` and of the built extension's name functions;
  the labels in ``CASES`` are the hand-written expectation it is
  compared with. No GPU is needed, but the extension must be built.
* ``reference``: float64 on the CPU from the bf16-rounded inputs. It
  never touches MIOpen or hipBLASLt.
* ``bound`` / ``assert_within``: a derived per-element error bound.

The bound. ``ref`` is the exact result and ``A`` the same operation on
absolute values, so ``A`` bounds every partial sum. A kernel that
multiplies bf16 exactly, accumulates L terms in fp32 and rounds once to
bf16 (8 significant bits, round-to-nearest) is off by at most

    2^-8 * |ref|  +  2 * L * 2^-24 * A          (bf16 outputs)
                     2 * L * 2^-24 * A          (fp32 outputs)

The first term is the final rounding; ``L * 2^-24 * A`` is the fp32
accumulation in any order; the factor 2 absorbs the second-order terms
(rounding the already-perturbed sum, (1+u)^L - 1 - Lu). Where ``A`` is 0
the bound is 0: structural zeros must be exact zeros.
"""

from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass

import torch
import torch.nn.functional as F

U_BF16 = 2.0 ** -8   # unit roundoff of bf16 (8 significant bits)
U_FP32 = 2.0 ** -24  # unit roundoff of fp32

ENTRIES = (
    "conv_fwd", "conv_bwd_weight", "pw_fwd", "pw_bwd_data_strided",
    "pw_bwdw", "autograd",
)


@dataclass(frozen=True)
class Case:
    """One convolution problem and the entry point that runs it.

    (C, K) are always the FORWARD convolution's input and output
    channels, also for the gradient entry points. ``path`` names the
    kernel reached by each leg, joined with '+', in the order of
    ``legs(case)`` (the bias gradient is a torch reduction and has no
    label)."""

    name: str
    entry: str
    path: str
    C: int
    K: int
    H: int
    W: int
    R: int = 1
    S: int = 1
    sh: int = 1
    sw: int = 1
    ph: int = 0
    pw: int = 0
    bias: bool = False
    N: int = 2
    blaslt: bool = False       # MPI4DL_PW_BLASLT for this case
    x_fp32_strided: bool = False  # feed a non-contiguous fp32 x

    def __post_init__(self):
        assert self.entry in ENTRIES, self.entry

    @property
    def id(self):
        return f"{self.entry}-{self.name}"

    @property
    def OH(self):
        return (self.H + 2 * self.ph - self.R) // self.sh + 1

    @property
    def OW(self):
        return (self.W + 2 * self.pw - self.S) // self.sw + 1


def legs(case):
    return {
        "conv_fwd": ("y",),
        "pw_fwd": ("y",),
        "conv_bwd_weight": ("gw",),
        "pw_bwdw": ("gw",),
        "pw_bwd_data_strided": ("gx",),
        "autograd": ("y", "gx", "gw") + (("gb",) if case.bias else ()),
    }[case.entry]


def reduction_length(case, leg):
    if leg == "y":
        return case.C * case.R * case.S
    if leg == "gx":
        return case.K * case.R * case.S
    return case.N * case.OH * case.OW  # gw, gb


def leg_is_bf16(leg):
    return leg != "gw"


# ---------------------------------------------------------------------------
# What production code picks. Nothing of the dispatch is written here:
# ``conv_native.conv_plan`` says which route each leg takes and with which
# problem, and the extension's name functions, which call the choosers the
# launchers call, say which kernel a native route then launches. This
# file only spells the labels.
# ---------------------------------------------------------------------------

def _mfrag(K):
    """Spells the MFRAG of a label in ``_build_cases``; decides nothing."""
    return 1 if K <= 32 else 2 if K <= 64 else 4


def extension():
    """The built extension. It cross-compiles and imports without a GPU;
    ImportError if the tree is not built."""
    from mpi4dl_amd import _gemscore
    return _gemscore


def leg_label(which, leg, ge):
    """The label of one leg of a plan ('y', 'gx' or 'gw')."""
    route, problem = leg
    if route == "matmul":
        return {"y": "blaslt:fwd", "gx": "blaslt:gx"}[which]
    if route == "bmm":
        return "blaslt:gw_bmm"
    if route in ("pw_fwd", "pw_bwd_data_strided"):
        return ge.pw_kernel_name(*problem)
    if route == "pw_bwdw":
        return ge.pw_bwdw_kernel_name(*problem)
    if route == "pw_bwdw_sub":
        return "sub:" + ge.pw_bwdw_kernel_name(*problem)
    if route == "conv_fwd":
        return ge.conv_fwd_kernel_name(*problem)
    if route == "conv_fwd_zs":
        return "zs:" + ge.conv_fwd_kernel_name(*problem)
    assert route == "conv_bwd_weight", route
    return "conv_bwdw"


def expected_path(c, ge=None):
    """The kernels production code picks for a case: for a direct entry,
    its binding's name function on the arguments ``_run_gpu`` passes; for
    autograd, the three legs of ``conv_plan``."""
    ge = ge or extension()
    ohw = c.OH * c.OW
    if c.entry == "conv_fwd":
        return ge.conv_fwd_kernel_name(c.C, c.K, c.H, c.W, c.R, c.S, c.sh,
                                       c.sw, c.ph, c.pw)
    if c.entry == "conv_bwd_weight":
        return "conv_bwdw"
    if c.entry == "pw_fwd":
        return ge.pw_kernel_name(c.C, c.K, ohw, c.sw, 1)
    if c.entry == "pw_bwd_data_strided":
        return ge.pw_kernel_name(c.K, c.C, ohw, 1, c.sw)
    if c.entry == "pw_bwdw":
        return ge.pw_bwdw_kernel_name(c.N, c.K, c.C, ohw)
    assert c.entry == "autograd", c.entry
    from mpi4dl_amd.ops.conv_native import conv_plan
    plan = conv_plan(c.N, c.C, c.K, c.H, c.W, c.R, c.S, c.sh, c.sw, c.ph,
                     c.pw, blaslt=c.blaslt)
    return "+".join(leg_label(which, leg, ge)
                    for which, leg in zip(("y", "gx", "gw"), plan))


# Every kernel instantiation and wrapper branch the matrix reaches. The
# generic-S v2 instantiations (<0,*>) are gone: they returned wrong
# interior pixels and S not in {1,3,7} now runs the guarded v1 kernel.
ALL_PATHS = [
    "v1",
    "v2<3,1>", "v2<3,2>", "v2<3,4>",
    "v2<7,1>", "v2<7,2>", "v2<7,4>",
    "v2<1,1>", "v2<1,2>", "v2<1,4>",
    "zs:v1", "zs:v2<3,1>", "zs:v2<3,2>", "zs:v2<7,1>", "zs:v2<1,1>",
    "conv_bwdw",
    "pw<1,1>", "pw<2,1>", "pw<4,1>",
    "pw<1,2>", "pw<2,2>", "pw<4,2>",
    "pw<1,1>:scatter", "pw<2,1>:scatter", "pw<4,1>:scatter",
    "pw_fat", "pw_fat256",
    "pw_bwdw128", "pw_bwdw128:slab", "pw_bwdw256:slab", "sub:pw_bwdw128",
    "blaslt:fwd", "blaslt:gx", "blaslt:gw_bmm",
]


# ---------------------------------------------------------------------------
# The case matrix
# ---------------------------------------------------------------------------

def _conv_shapes():
    """(name, fwd path, autograd path, geometry) of every RxS shape; each
    runs through ge.conv_fwd directly and through native_conv2d autograd."""
    def g(C, K, H, W, R, S, sh=1, sw=1, ph=0, pw=0, N=2):
        return dict(C=C, K=K, H=H, W=W, R=R, S=S, sh=sh, sw=sw, ph=ph, pw=pw,
                    N=N)
    return [
        # --- v2 <3,*> ---------------------------------------------------
        ("3x3-c16k24", "v2<3,1>", "v2<3,1>+v2<3,1>+conv_bwdw",
         g(16, 24, 16, 24, 3, 3, ph=1, pw=1)),
        ("3x3-c12k40-cs36", "v2<3,2>", "v2<3,2>+v2<3,1>+conv_bwdw",
         g(12, 40, 8, 16, 3, 3, ph=1, pw=1)),
        ("3x3-c20k104", "v2<3,4>", "v2<3,4>+v2<3,1>+conv_bwdw",
         g(20, 104, 16, 40, 3, 3, ph=1, pw=1)),
        ("3x3-pad0-18x34", "v2<3,1>", "v2<3,1>+v1+conv_bwdw",
         g(16, 32, 18, 34, 3, 3)),
        ("3x3-pad0x2-d6", "v2<3,1>", "v2<3,1>+v1+conv_bwdw",
         g(16, 32, 18, 30, 3, 3, ph=0, pw=2)),
        # --- v2 <7,*> as 1x7 ---------------------------------------------
        ("1x7-c26k26", "v2<7,1>", "v2<7,1>+v2<7,1>+conv_bwdw",
         g(26, 26, 16, 24, 1, 7, pw=3)),
        ("1x7-c26k52", "v2<7,2>", "v2<7,2>+v2<7,1>+conv_bwdw",
         g(26, 52, 16, 24, 1, 7, pw=3)),
        ("1x7-c26k104", "v2<7,4>", "v2<7,4>+v2<7,1>+conv_bwdw",
         g(26, 104, 16, 24, 1, 7, pw=3)),
        ("1x7-pad0-16x38", "v2<7,1>", "v2<7,1>+v1+conv_bwdw",
         g(26, 26, 16, 38, 1, 7)),
        ("1x7-pad6-d2", "v2<7,1>", "v2<7,1>+v1+conv_bwdw",
         g(26, 26, 16, 26, 1, 7, pw=6)),
        ("7x7-c8k64", "v2<7,2>", "v2<7,2>+v2<7,1>+conv_bwdw",
         g(8, 64, 16, 16, 7, 7, ph=3, pw=3)),
        # --- v2 <1,*> as 7x1 ---------------------------------------------
        ("7x1-c52k24", "v2<1,1>", "v2<1,1>+v1+conv_bwdw",
         g(52, 24, 24, 16, 7, 1, ph=3)),
        ("7x1-c52k52", "v2<1,2>", "v2<1,2>+v2<1,2>+conv_bwdw",
         g(52, 52, 24, 16, 7, 1, ph=3)),
        ("7x1-c52k104", "v2<1,4>", "v2<1,4>+v2<1,2>+conv_bwdw",
         g(52, 104, 24, 16, 7, 1, ph=3)),
        ("7x1-pad0-22x32", "v2<1,1>", "v2<1,1>+v1+conv_bwdw",
         g(52, 24, 22, 32, 7, 1)),
        ("7x1-n1", "v2<1,2>", "v2<1,2>+v2<1,2>+conv_bwdw",
         g(52, 52, 24, 16, 7, 1, ph=3, N=1)),
        ("7x1-n3", "v2<1,1>", "v2<1,1>+v1+conv_bwdw",
         g(52, 24, 24, 16, 7, 1, ph=3, N=3)),
        # --- generic S (was v2 <0,*>, now v1) ----------------------------
        ("5x5-c8k16", "v1", "v1+v1+conv_bwdw",
         g(8, 16, 16, 16, 5, 5, ph=2, pw=2)),
        ("5x5-c8k48", "v1", "v1+v1+conv_bwdw",
         g(8, 48, 16, 16, 5, 5, ph=2, pw=2)),
        ("5x5-c8k72", "v1", "v1+v1+conv_bwdw",
         g(8, 72, 16, 16, 5, 5, ph=2, pw=2)),
        ("1x5-c8", "v1", "v1+v1+conv_bwdw",
         g(8, 16, 8, 16, 1, 5, pw=2)),
        ("2x2-c16-17x17", "v1", "v1+v1+conv_bwdw",
         g(16, 16, 17, 17, 2, 2)),
        # --- v1 ----------------------------------------------------------
        ("3x3s2-c3k40-34", "v1", "v1+zs:v1+conv_bwdw",
         g(3, 40, 34, 34, 3, 3, 2, 2, 1, 1)),
        ("3x3s2-c3k40-33", "v1", "v1+zs:v1+conv_bwdw",
         g(3, 40, 33, 33, 3, 3, 2, 2, 1, 1)),
        ("7x7s2-c3k16", "v1", "v1+zs:v2<7,1>+conv_bwdw",
         g(3, 16, 32, 32, 7, 7, 2, 2, 3, 3)),
        ("3x3s2-c8k136", "v1", "v1+zs:v2<3,1>+conv_bwdw",
         g(8, 136, 16, 16, 3, 3, 2, 2, 1, 1)),
        ("3x3-ow130", "v1", "v1+v1+conv_bwdw",
         g(4, 8, 3, 130, 3, 3, ph=1, pw=1)),
        ("3x3-15x15", "v1", "v1+v1+conv_bwdw",
         g(16, 24, 15, 15, 3, 3, ph=1, pw=1)),
        ("3x3-c3-cs9", "v1", "v1+v2<3,1>+conv_bwdw",
         g(3, 16, 16, 16, 3, 3, ph=1, pw=1)),
        ("1x7s1x2", "v1", "v1+zs:v2<7,1>+conv_bwdw",
         g(26, 26, 16, 32, 1, 7, 1, 2, 0, 3)),
        ("7x1s2x1", "v1", "v1+zs:v1+conv_bwdw",
         g(26, 26, 32, 16, 7, 1, 2, 1, 3, 0)),
        ("3x3s2-c40k48", "v1", "v1+zs:v2<3,2>+conv_bwdw",
         g(40, 48, 16, 16, 3, 3, 2, 2, 1, 1)),
        ("7x1s2x1-k40", "v1", "v1+zs:v2<1,1>+conv_bwdw",
         g(26, 40, 32, 16, 7, 1, 2, 1, 3, 0)),
    ]


def _build_cases():
    cases = []
    for name, fwd, auto, geom in _conv_shapes():
        cases.append(Case(name, "conv_fwd", fwd, bias=True, **geom))
        cases.append(Case(name, "autograd", auto, bias=True, **geom))
    # wrapper glue: non-contiguous fp32 x through ConvFn's .contiguous().to()
    cases.append(Case("3x3-c16k24-fp32-strided-x", "autograd",
                      "v2<3,1>+v2<3,1>+conv_bwdw", 16, 24, 16, 24, 3, 3,
                      ph=1, pw=1, bias=True, x_fp32_strided=True))
    # conv_bwdw directly: R != S, two M tiles (K > 64), CRS tail
    cases.append(Case("1x7-c26k72", "conv_bwd_weight", "conv_bwdw",
                      26, 72, 16, 24, 1, 7, pw=3))

    # --- pw_kernel<M,1>: the base grid, with and without bias -----------
    for C in (8, 36, 40, 64):
        for K in (24, 48, 104, 136):
            for bias in (False, True):
                cases.append(Case(
                    f"c{C}k{K}" + ("-bias" if bias else ""), "pw_fwd",
                    f"pw<{_mfrag(K)},1>", C, K, 8, 16, bias=bias))
    cases.append(Case("c40k48-n3", "pw_fwd", "pw<2,1>", 40, 48, 8, 16,
                      bias=True, N=3))
    cases.append(Case("c40k48-4x32", "pw_fwd", "pw<2,1>", 40, 48, 4, 32,
                      bias=True))
    cases.append(Case("c36k24-n1", "pw_fwd", "pw<1,1>", 36, 24, 8, 16,
                      bias=True, N=1))
    # the same family through autograd: gx is the mirror GEMM (C <-> K),
    # gw the unsplit 128-tile pw_bwdw at OHW = 128; (136, 136) gives it
    # two K tiles and two C tiles, both with tails
    for C, K in ((8, 24), (36, 48), (40, 104), (64, 136), (136, 136)):
        cases.append(Case(
            f"c{C}k{K}", "autograd",
            f"pw<{_mfrag(K)},1>+pw<{_mfrag(C)},1>+pw_bwdw128", C, K, 8, 16,
            bias=True))
    # --- pw_kernel<M,2> + scatter backward-data + subsampled gw ---------
    for K in (24, 48, 104):
        cases.append(Case(
            f"s2-c40k{K}", "autograd",
            f"pw<{_mfrag(K)},2>+pw<2,1>:scatter+sub:pw_bwdw128", 40, K,
            16, 32, sh=2, sw=2, bias=True))
    for C in (24, 40, 104):
        cases.append(Case(
            f"s2-c{C}k40", "pw_bwd_data_strided",
            f"pw<{_mfrag(C)},1>:scatter", C, 40, 16, 32, sh=2, sw=2))
    # --- pw_fat / pw_fat256 at their thresholds, with bias --------------
    for C, K, H, W, path in (
        (256, 128, 8, 16, "pw_fat"),
        (292, 133, 8, 16, "pw_fat"),
        (512, 256, 8, 16, "pw_fat"),      # OHW % 256 != 0 keeps it off fat256
        (512, 256, 16, 16, "pw_fat256"),
        (520, 264, 16, 16, "pw_fat256"),
    ):
        cases.append(Case(f"c{C}k{K}-{H}x{W}", "pw_fwd", path, C, K, H, W,
                          bias=True))
    # --- pw_bwdw ----------------------------------------------------------
    cases.append(Case("ohw128", "pw_bwdw", "pw_bwdw128", 40, 24, 8, 16))
    cases.append(Case("ohw2048-slab", "pw_bwdw", "pw_bwdw128:slab",
                      40, 24, 32, 64))
    cases.append(Case("ohw192", "pw_bwdw", "pw_bwdw128", 40, 24, 12, 16))
    cases.append(Case("c136k72-ohw192", "pw_bwdw", "pw_bwdw128",
                      136, 72, 12, 16))
    cases.append(Case("tile256", "pw_bwdw", "pw_bwdw256:slab",
                      260, 264, 128, 128, N=1))
    # --- hipBLASLt wrapper branches (MPI4DL_PW_BLASLT=1) ----------------
    cases.append(Case("blaslt-c104k136", "autograd",
                      "blaslt:fwd+blaslt:gx+pw_bwdw128", 104, 136, 8, 16,
                      bias=True, blaslt=True))
    cases.append(Case("blaslt-c640k560", "autograd",
                      "blaslt:fwd+blaslt:gx+blaslt:gw_bmm", 640, 560, 8, 16,
                      bias=True, blaslt=True))
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids), "duplicate case id"
    return cases


CASES = _build_cases()
CASE_BY_ID = {c.id: c for c in CASES}

# one per family, run twice for bit-identical y and gx
DETERMINISM_IDS = {
    "v1": "autograd-3x3s2-c3k40-34",
    "v2": "autograd-1x7-c26k52",
    "pw skinny": "autograd-c40k104",
    "pw stride 2": "autograd-s2-c40k48",
    "scatter": "pw_bwd_data_strided-s2-c104k40",
    "fat": "pw_fwd-c292k133-8x16",
    "fat256": "pw_fwd-c520k264-16x16",
}


# ---------------------------------------------------------------------------
# Inputs and reference
# ---------------------------------------------------------------------------

def make_inputs(case):
    """x, go: bf16 randn. w: 0.1*randn rounded to bf16, held in fp32.
    b: fp32 randn. Fixed seed per case."""
    gen = torch.Generator().manual_seed(zlib.crc32(case.id.encode()))
    x = torch.randn(case.N, case.C, case.H, case.W, generator=gen).bfloat16()
    w = (0.1 * torch.randn(case.K, case.C, case.R, case.S, generator=gen)
         ).bfloat16().float()
    b = torch.randn(case.K, generator=gen) if case.bias else None
    go = torch.randn(case.N, case.K, case.OH, case.OW,
                     generator=gen).bfloat16()
    return x, w, b, go


def _ops(case, x, w, b, go, want):
    """The operation of each leg in the dtype of its arguments."""
    st, pd = (case.sh, case.sw), (case.ph, case.pw)
    out = {}
    if "y" in want:
        out["y"] = F.conv2d(x, w, b, stride=st, padding=pd)
    if "gx" in want:
        out["gx"] = torch.nn.grad.conv2d_input(
            list(x.shape), w, go, stride=st, padding=pd)
    if "gw" in want:
        if (case.R, case.S, case.ph, case.pw) == (1, 1, 0, 0):
            # 1x1: conv2d_weight is this GEMM (on the strided pixels)
            xs = x[:, :, ::case.sh, ::case.sw]
            out["gw"] = torch.einsum(
                "nkp,ncp->kc", go.flatten(2), xs.flatten(2)
            ).reshape(w.shape)
        else:
            out["gw"] = torch.nn.grad.conv2d_weight(
                x, list(w.shape), go, stride=st, padding=pd)
    if "gb" in want:
        out["gb"] = go.sum(dim=(0, 2, 3))
    return out


def reference(case, x, w, b, go):
    """{leg: (ref, A)} in float64 on the CPU. A is the same operation on
    |x|, |w|, |b|, |go|."""
    d = lambda t: None if t is None else t.detach().cpu().double()
    a = lambda t: None if t is None else t.detach().cpu().double().abs()
    want = legs(case)
    ref = _ops(case, d(x), d(w), d(b), d(go), want)
    mag = _ops(case, a(x), a(w), a(b), a(go), want)
    return {leg: (ref[leg], mag[leg]) for leg in want}


def emulate(case, x, w, b, go):
    """What a correct kernel computes: the fp32 operation on the bf16
    inputs, rounded to bf16 where the leg is bf16. The two wrapper
    branches that round twice are emulated with both roundings."""
    f = lambda t: None if t is None else t.float()
    want = legs(case)
    out = _ops(case, f(x), f(w), f(b), f(go), want)
    kinds = dict(zip(want, case.path.split("+")))
    if kinds.get("y") == "blaslt:fwd" and b is not None:
        mm = _ops(case, f(x), f(w), None, f(go), ("y",))["y"].bfloat16()
        out["y"] = mm + b.bfloat16().view(1, -1, 1, 1)
    if kinds.get("gw") == "blaslt:gw_bmm":
        per_img = torch.einsum("nkp,ncp->nkc", f(go).flatten(2),
                               f(x).flatten(2)).bfloat16()
        out["gw"] = per_img.float().sum(0).reshape(w.shape)
    return {leg: (t.bfloat16() if leg_is_bf16(leg) else t).double()
            for leg, t in out.items()}


@functools.lru_cache(maxsize=None)
def case_data(case):
    """(inputs, reference) of a case, computed once and shared."""
    inputs = make_inputs(case)
    return inputs, reference(case, *inputs)


# ---------------------------------------------------------------------------
# Bound and assertion
# ---------------------------------------------------------------------------

def bound(ref, A, L, out_is_bf16, extra=None, eps=None):
    """Per-element error bound (module docstring). ``extra`` is the
    derived term of a branch that rounds more than once. ``eps`` is the
    unit roundoff of the output format where it is not told by
    ``out_is_bf16`` (the pool oracle's fp16 legs)."""
    if eps is None:
        eps = U_BF16 if out_is_bf16 else 0.0
    bd = 2.0 * L * U_FP32 * A
    if eps:
        bd = bd + eps * ref.abs()
    if extra is not None:
        bd = bd + extra
    return bd


def extra_term(case, leg, ref, A, b):
    """The two wrapper branches that round twice.

    blaslt:fwd with bias: matmul rounds to bf16 (2^-8 |ref - b|), the
    bias is rounded to bf16 (2^-8 |b|), and `y += bias` rounds the sum
    (the 2^-8 |ref| every bf16 leg already has).
    blaslt:gw_bmm: each image's partial gw is rounded to bf16 before the
    fp32 sum over images; the partials' magnitudes sum to at most A."""
    if case.entry != "autograd":
        return None
    kind = dict(zip(legs(case), case.path.split("+"))).get(leg)
    if kind == "blaslt:fwd" and b is not None:
        bb = b.detach().cpu().double().view(1, -1, 1, 1)
        return U_BF16 * ((ref - bb).abs() + bb.abs())
    if kind == "blaslt:gw_bmm":
        return U_BF16 * A
    return None


def assert_within(got, ref, A, L, out_is_bf16, extra=None, what="",
                  eps=None):
    """Fail unless every element of ``got`` is finite and within the
    bound of ``ref``. Reports the worst index, err/bound there and the
    number of elements over the bound. Returns the largest err/bound."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (
        f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}")
    finite = torch.isfinite(got)
    if not bool(finite.all()):
        bad = (~finite).nonzero()
        raise AssertionError(
            f"{what}: {bad.shape[0]} non-finite values, first at "
            f"{tuple(bad[0].tolist())}")
    bd = bound(ref, A, L, out_is_bf16, extra, eps)
    err = (got - ref).abs()
    over = err > bd
    # err/bound, with err > 0 at bound == 0 (a structural zero) as inf
    ratio = torch.where(
        bd > 0, err / bd.clamp_min(1e-300),
        torch.where(err > 0, torch.full_like(err, float("inf")),
                    torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if bool(over.any()):
        flat = int(ratio.argmax())
        idx = tuple(int(i) for i in torch.unravel_index(
            torch.tensor(flat), ratio.shape))
        raise AssertionError(
            f"{what}: {int(over.sum())} of {over.numel()} elements over the "
            f"bound; worst at {idx}: got {float(got[idx]):.9g}, ref "
            f"{float(ref[idx]):.9g}, err {float(err[idx]):.3g}, bound "
            f"{float(bd[idx]):.3g}, err/bound {worst:.3g}")
    return worst


def check_case(case, results, what=""):
    """assert_within on every leg of a case; {leg: worst err/bound}."""
    (x, w, b, go), ref = case_data(case)
    out = {}
    for leg in legs(case):
        r, A = ref[leg]
        out[leg] = assert_within(
            results[leg], r, A, reduction_length(case, leg),
            leg_is_bf16(leg), extra_term(case, leg, r, A, b),
            what=f"{what or case.id} {leg} [{case.path}]")
    return out


# ---------------------------------------------------------------------------
# Running a case on the GPU
# ---------------------------------------------------------------------------

class _Recorder:
    """Stands in for the extension module and notes, for every native
    convolution binding called, the kernel the extension names for the
    shapes of that call's own arguments and result: the name functions
    run the choosers the launch itself ran."""

    def __init__(self, ge):
        self._ge = ge
        self.kernels = []

    def __getattr__(self, name):
        fn = getattr(self._ge, name)
        label = getattr(self, "_label_" + name, None)
        if label is None:
            return fn

        def wrapped(*args):
            out = fn(*args)
            self.kernels.append(label(out, *args))
            return out
        return wrapped

    def _label_conv_fwd(self, y, x, w, bias, sh, sw, ph, pw):
        (_, C, H, W), (K, _, R, S) = x.shape, w.shape
        return self._ge.conv_fwd_kernel_name(C, K, H, W, R, S, sh, sw, ph, pw)

    def _label_conv_bwd_weight(self, gw, go, x, R, S, sh, sw, ph, pw):
        return "conv_bwdw"

    def _label_pw_fwd(self, y, x, w, bias, sh, sw):
        (_, K, OH, OW), C = y.shape, x.shape[1]
        return self._ge.pw_kernel_name(C, K, OH * OW, sw, 1)

    def _label_pw_bwd_data_strided(self, gx, go, wt, H, W, sh, sw):
        (_, Kred, OH, OW), Cout = go.shape, wt.shape[0]
        return self._ge.pw_kernel_name(Kred, Cout, OH * OW, 1, sw)

    def _label_pw_bwdw(self, gw, go, x):
        (N, K, OH, OW), C = go.shape, x.shape[1]
        return self._ge.pw_bwdw_kernel_name(N, K, C, OH * OW)


def run_gpu(case, kernels=None):
    """Run the case's entry point once on the GPU; {leg: CPU tensor}.
    The caller sets MPI4DL_PW_BLASLT from ``case.blaslt``. If ``kernels``
    is a list it receives, in call order, the kernel behind every native
    binding that the entry point called."""
    from mpi4dl_amd.ops import backend, conv_native
    from mpi4dl_amd.ops.conv_native import native_conv2d

    ge = _Recorder(backend.ext())
    if kernels is not None:
        ge.kernels = kernels
    if case.entry == "autograd":
        real_ext = conv_native.backend.ext
        conv_native.backend.ext = lambda: ge
        try:
            return _run_gpu(case, ge, native_conv2d)
        finally:
            conv_native.backend.ext = real_ext
    return _run_gpu(case, ge, native_conv2d)


def _run_gpu(case, ge, native_conv2d):
    (x, w, b, go), _ = case_data(case)
    dev = "cuda"
    xg, gog = x.to(dev), go.to(dev)
    wg = w.to(dev)
    bg = None if b is None else b.to(dev)
    st = (case.sh, case.sw, case.ph, case.pw)
    if case.entry == "conv_fwd":
        out = {"y": ge.conv_fwd(xg, wg.bfloat16(), bg, *st)}
    elif case.entry == "conv_bwd_weight":
        out = {"gw": ge.conv_bwd_weight(gog, xg, case.R, case.S, *st)}
    elif case.entry == "pw_fwd":
        out = {"y": ge.pw_fwd(xg, wg.bfloat16(), bg, case.sh, case.sw)}
    elif case.entry == "pw_bwd_data_strided":
        wt = wg.bfloat16().view(case.K, case.C).t().contiguous()
        out = {"gx": ge.pw_bwd_data_strided(gog, wt, case.H, case.W,
                                            case.sh, case.sw)}
    elif case.entry == "pw_bwdw":
        out = {"gw": ge.pw_bwdw(gog, xg).view(case.K, case.C, 1, 1)}
    else:
        if case.x_fp32_strided:
            # same values as x, fp32, every other column of a wider buffer
            wide = torch.zeros(case.N, case.C, case.H, 2 * case.W,
                               device=dev)
            wide[..., ::2] = xg.float()
            xin = wide[..., ::2]
            assert not xin.is_contiguous()
        else:
            xin = xg
        xin = xin.detach().requires_grad_(True)
        wg = wg.detach().requires_grad_(True)
        if bg is not None:
            bg = bg.detach().requires_grad_(True)
        y = native_conv2d(xin, wg, bg, (case.sh, case.sw),
                          (case.ph, case.pw))
        y.backward(gog)
        out = {"y": y.detach(), "gx": xin.grad, "gw": wg.grad}
        if bg is not None:
            out["gb"] = bg.grad
    torch.cuda.synchronize()
    return {leg: t.detach().cpu() for leg, t in out.items()}
