#!/usr/bin/env python3
"""Per-shape A/B of the gemscore implicit-GEMM MFMA conv vs MIOpen
(torch F.conv2d) on the shapes the flagship model actually runs.

Usage (GPU): python benchmarks/conv_microbench.py [--iters 20]
Writes a table to stdout; used to set the NativeConv2d dispatch policy.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

# (C, K, H, W, kh, kw, s, ph, pw) — amoebanet-D F416 @2048 + resnet shapes
SHAPES = [
    (3, 104, 2048, 2048, 3, 3, 2, 1, 1),     # stem
    (104, 208, 1024, 1024, 1, 1, 1, 0, 0),   # reduce 1x1 (big HW)
    (208, 52, 512, 512, 1, 7, 1, 0, 3),      # 1x7
    (208, 52, 512, 512, 7, 1, 1, 3, 0),      # 7x1
    (416, 104, 256, 256, 1, 7, 1, 0, 3),
    (416, 104, 256, 256, 3, 3, 1, 1, 1),     # conv_3x3 mid
    (64, 64, 512, 512, 3, 3, 1, 1, 1),       # resnet body
    (256, 256, 128, 128, 3, 3, 1, 1, 1),     # deeper
]


def timeit(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


# ResNet's stride-1 3x3 stack (C = K, H = W), all at pad 1
WINO_SHAPES = [(64, 512), (128, 256), (256, 128), (512, 64), (416, 256)]


def winograd_ab(args):
    """Stride-1 3x3: the fused F(2x2,3x3) kernel (ge.wino_fwd), the
    batched-GEMM staging, our direct v2<3,*> kernel (ge.conv_fwd) and
    MIOpen. All four are warmed up first; the timed rounds then alternate
    between them, and the median round of each is reported. Ratios are
    MIOpen's time over the variant's (above 1: the variant is faster)."""
    from mpi4dl_amd.ops import backend
    from mpi4dl_amd.ops.winograd_ref import filter_transform, winograd_bmm_conv2d

    ge = backend.ext()
    names = ("fused", "staging", "direct", "miopen")
    print(f"{'shape':<26}" + "".join(f"{n:>11}" for n in names)
          + "   fused/staging/direct vs miopen")
    for C, hw in WINO_SHAPES:
        x = torch.randn(args.batch, C, hw, hw, device="cuda", dtype=torch.bfloat16)
        w = torch.randn(C, C, 3, 3, device="cuda") * 0.05
        wb = w.to(torch.bfloat16)
        U = filter_transform(w)
        fns = {
            "fused": lambda: ge.wino_fwd(x, wb, None, 1, 1),
            "staging": lambda: winograd_bmm_conv2d(x, U, None, padding=1),
            "direct": lambda: ge.conv_fwd(x, wb, None, 1, 1, 1, 1),
            "miopen": lambda: torch.nn.functional.conv2d(x, wb, padding=1),
        }
        for fn in fns.values():
            timeit(fn, 2, warmup=3)
        rounds = {n: [] for n in names}
        for _ in range(5):
            for n in names:
                rounds[n].append(timeit(fns[n], max(args.iters // 5, 2), warmup=0))
        t = {n: sorted(v)[len(v) // 2] for n, v in rounds.items()}
        ref = torch.nn.functional.conv2d(x.float(), wb.float(), padding=1)
        rel = ((fns["fused"]().float() - ref).abs().max().item()
               / max(ref.abs().max().item(), 1e-3))
        tag = f"C{C}->K{C} {hw}x{hw} N{args.batch}"
        print(f"{tag:<26}" + "".join(f"{t[n]:9.3f}ms" for n in names)
              + "   " + " ".join(f"{t['miopen'] / t[n]:5.2f}x" for n in names[:3])
              + f"  [{ge.wino_kernel_name(C, C, hw, hw, 1, 1)}, "
              f"{ge.conv_fwd_kernel_name(C, C, hw, hw, 3, 3, 1, 1, 1, 1)}]"
              f"  fused relerr {rel:.3g}", flush=True)


# (C = K, H = W, R, S) at stride 1, "same" padding: AmoebaNet's
# conv_1x7_7x1 legs per plane, then ResNet's 3x3 stack
TAP_SHAPES = (
    [(c, hw, r, s) for c, hw in ((104, 256), (208, 128), (416, 64), (52, 512))
     for r, s in ((1, 7), (7, 1))]
    + [(c, hw, 3, 3) for c, hw in WINO_SHAPES[:4]]
)
# (C = K, H, W): the tiles a 4-way spatial split of the 128² and 64² planes
# hands one GPU; run at --batch and at N = 1, 1x7 and 7x1
TAP_TILES = ((208, 64, 64), (416, 32, 32), (416, 64, 16))


def tap_ab(args):
    """Stride-1 1x7 / 7x1 / 3x3, forward and data-grad legs: the tap-shift
    kernel (ge.tap_fwd, filter pre-pass included), the same with the channels
    split as its chooser says (split=-1: workspace allocation and reduce
    kernel included), our direct kernel (ge.conv_fwd; its data-grad includes
    the weight transpose and flip that ConvFn does) and MIOpen. All variants
    are warmed up first; the timed rounds then alternate between them, and
    the median round of each is reported. Ratios are MIOpen's time over the
    variant's."""
    import torch.nn.functional as F

    from mpi4dl_amd.ops import backend

    ge = backend.ext()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    names = ("tap", "split", "direct", "miopen")
    print(f"{'shape':<34}{'leg':<5}" + "".join(f"{n:>11}" for n in names)
          + "   tap/split/direct vs miopen  winner")
    shapes = [(c, hw, hw, r, s, args.batch) for c, hw, r, s in TAP_SHAPES]
    shapes += [(c, h, w, r, s, n) for n in sorted({args.batch, 1}, reverse=True)
               for c, h, w in TAP_TILES for r, s in ((1, 7), (7, 1))]
    for C, H, W, R, S, N in shapes:
        ph, pw = R // 2, S // 2
        x = torch.randn(N, C, H, W, device="cuda", dtype=torch.bfloat16)
        go = torch.randn(N, C, H, W, device="cuda", dtype=torch.bfloat16)
        wb = (torch.randn(C, C, R, S, device="cuda") * 0.05).to(torch.bfloat16)
        legs = {
            "fwd": {
                "tap": lambda: ge.tap_fwd(x, wb, None, ph, pw),
                "split": lambda: ge.tap_fwd(x, wb, None, ph, pw, split=-1),
                "direct": lambda: ge.conv_fwd(x, wb, None, 1, 1, ph, pw),
                "miopen": lambda: F.conv2d(x, wb, padding=(ph, pw)),
            },
            "gx": {
                "tap": lambda: ge.tap_fwd(go, wb, None, R - 1 - ph,
                                          S - 1 - pw, True),
                "split": lambda: ge.tap_fwd(go, wb, None, R - 1 - ph,
                                            S - 1 - pw, True, split=-1),
                "direct": lambda: ge.conv_fwd(
                    go, wb.transpose(0, 1).flip(2, 3).contiguous(), None,
                    1, 1, R - 1 - ph, S - 1 - pw),
                "miopen": lambda: torch.nn.grad.conv2d_input(
                    x.shape, wb, go, padding=(ph, pw)),
            },
        }
        for leg, fns in legs.items():
            for fn in fns.values():
                timeit(fn, 2, warmup=3)
            rounds = {n: [] for n in names}
            for _ in range(5):
                for n in names:
                    rounds[n].append(
                        timeit(fns[n], max(args.iters // 5, 2), warmup=0))
            t = {n: sorted(v)[len(v) // 2] for n, v in rounds.items()}
            ref = fns["miopen"]().float()
            rel = ((fns["tap"]().float() - ref).abs().max().item()
                   / max(ref.abs().max().item(), 1e-3))
            assert torch.equal(fns["split"](), fns["split"]())
            srel = ((fns["split"]().float() - ref).abs().max().item()
                    / max(ref.abs().max().item(), 1e-3))
            sname, sc = ge.tap_split_kernel_name(N, C, C, H, W, R, S, ph, pw,
                                                 cus)
            tag = f"C{C}->K{C} {H}x{W} k{R}x{S} N{N}"
            print(f"{tag:<34}{leg:<5}"
                  + "".join(f"{t[n]:9.3f}ms" for n in names) + "   "
                  + " ".join(f"{t['miopen'] / t[n]:5.2f}x" for n in names[:3])
                  + f"  {min(t, key=t.get):<7}"
                  f"[{ge.tap_kernel_name(C, C, H, W, R, S, ph, pw)}, "
                  f"{sname} sc{sc}, "
                  f"{ge.conv_fwd_kernel_name(C, C, H, W, R, S, 1, 1, ph, pw)}]"
                  f"  tap relerr {rel:.3g} split relerr {srel:.3g}",
                  flush=True)


# (C = K, H = W, R, S) at stride (min(R, 2), min(S, 2)), "same" padding:
# AmoebaNet's reduction-cell legs per plane, then the head of a ResNet stage
TAP_STRIDED_SHAPES = (
    [(c, hw, r, s) for c, hw in ((104, 256), (208, 128), (416, 64))
     for r, s in ((1, 7), (7, 1))]
    + [(c, hw, 3, 3) for c, hw in WINO_SHAPES[:3]]
)


def tap_strided_ab(args):
    """Strided 1x7 / 7x1 / 3x3, forward and data-grad legs: the strided
    tap-shift kernels (ge.tap_fwd_strided, ge.tap_bwd_data_strided, filter
    pre-pass included), the current native routes (ge.conv_fwd; for the
    data-grad conv_fwd_zs as ConvFn runs it: zero fill, scatter, weight
    transpose and flip, then the stride-1 kernel) and MIOpen. Same protocol as
    --tap: all variants warmed up, alternating rounds, median; ratios are
    MIOpen's time over the variant's."""
    import torch.nn.functional as F

    from mpi4dl_amd.ops import backend
    from mpi4dl_amd.ops.conv_native import conv_plan

    ge = backend.ext()
    names = ("tap", "native", "miopen")
    print(f"{'shape':<34}{'leg':<5}" + "".join(f"{n:>11}" for n in names)
          + "   tap/native vs miopen  winner")
    N = args.batch
    for C, hw, R, S in TAP_STRIDED_SHAPES:
        sh, sw, ph, pw = min(R, 2), min(S, 2), R // 2, S // 2
        plan = conv_plan(N, C, C, hw, hw, R, S, sh, sw, ph, pw, tap=False)
        _, _, hs, ws, _, _, _, _, tph, tpw = plan.gx.problem
        x = torch.randn(N, C, hw, hw, device="cuda", dtype=torch.bfloat16)
        wb = (torch.randn(C, C, R, S, device="cuda") * 0.05).to(torch.bfloat16)
        go = torch.randn_like(F.conv2d(x, wb, stride=(sh, sw), padding=(ph, pw)))

        def zero_stuffed():
            src = torch.zeros(N, C, hs, ws, device=go.device, dtype=go.dtype)
            src[:, :, ::sh, ::sw] = go
            wt = wb.transpose(0, 1).flip(2, 3).contiguous()
            return ge.conv_fwd(src, wt, None, 1, 1, tph, tpw)

        legs = {
            "fwd": {
                "tap": lambda: ge.tap_fwd_strided(x, wb, None, sh, sw, ph, pw),
                "native": lambda: ge.conv_fwd(x, wb, None, sh, sw, ph, pw),
                "miopen": lambda: F.conv2d(x, wb, stride=(sh, sw),
                                           padding=(ph, pw)),
            },
            "gx": {
                "tap": lambda: ge.tap_bwd_data_strided(go, wb, hw, hw, sh, sw,
                                                       ph, pw),
                "native": zero_stuffed,
                "miopen": lambda: torch.nn.grad.conv2d_input(
                    x.shape, wb, go, stride=(sh, sw), padding=(ph, pw)),
            },
        }
        for leg, fns in legs.items():
            for fn in fns.values():
                timeit(fn, 2, warmup=3)
            rounds = {n: [] for n in names}
            for _ in range(5):
                for n in names:
                    rounds[n].append(
                        timeit(fns[n], max(args.iters // 5, 2), warmup=0))
            t = {n: sorted(v)[len(v) // 2] for n, v in rounds.items()}
            ref = fns["miopen"]().float()
            rel = ((fns["tap"]().float() - ref).abs().max().item()
                   / max(ref.abs().max().item(), 1e-3))
            assert torch.equal(fns["tap"](), fns["tap"]())
            tag = f"C{C}->K{C} {hw}x{hw} k{R}x{S} s{sh}{sw} N{N}"
            kname = ge.tap_strided_kernel_name(C, C, hw, hw, R, S, sh, sw, ph,
                                               pw, leg == "gx")
            print(f"{tag:<34}{leg:<5}"
                  + "".join(f"{t[n]:9.3f}ms" for n in names) + "   "
                  + " ".join(f"{t['miopen'] / t[n]:5.2f}x" for n in names[:2])
                  + f"  {min(t, key=t.get):<7}[{kname}]  tap relerr {rel:.3g}",
                  flush=True)


def tap_bwdw_ab(args):
    """The shapes of --tap, weight-gradient leg only: the tap-shift kernel
    (ge.tap_bwd_weight), its rolling-window variant (ge.tap_bwd_weight_ring),
    its pixel-major variant (ge.tap_bwd_weight_px), our general kernel (ge.conv_bwd_weight) and MIOpen
    (torch.nn.grad.conv2d_weight on bf16 tensors). Same protocol as --tap:
    all variants warmed up, five alternating rounds, the median round.
    Ratios are MIOpen's time over the variant's; "px vs ring" is ring's time
    over px's."""
    from mpi4dl_amd.ops import backend

    ge = backend.ext()
    names = ("px", "ring", "tap", "bwdw", "miopen")
    print(f"{'shape':<34}" + "".join(f"{n:>11}" for n in names)
          + "   px/ring/tap/bwdw vs miopen  tap vs bwdw  ring vs tap"
          "  px vs ring  winner")
    for C, hw, R, S in TAP_SHAPES:
        ph, pw = R // 2, S // 2
        N = args.batch
        x = torch.randn(N, C, hw, hw, device="cuda", dtype=torch.bfloat16)
        go = torch.randn(N, C, hw, hw, device="cuda", dtype=torch.bfloat16)
        fns = {
            "px": lambda: ge.tap_bwd_weight_px(go, x, R, S, ph, pw),
            "ring": lambda: ge.tap_bwd_weight_ring(go, x, R, S, ph, pw),
            "tap": lambda: ge.tap_bwd_weight(go, x, R, S, ph, pw),
            "bwdw": lambda: ge.conv_bwd_weight(go, x, R, S, 1, 1, ph, pw),
            "miopen": lambda: torch.nn.grad.conv2d_weight(
                x, (C, C, R, S), go, padding=(ph, pw)),
        }
        for fn in fns.values():
            timeit(fn, 2, warmup=3)
        rounds = {n: [] for n in names}
        for _ in range(5):
            for n in names:
                rounds[n].append(
                    timeit(fns[n], max(args.iters // 5, 2), warmup=0))
        t = {n: sorted(v)[len(v) // 2] for n, v in rounds.items()}
        ref = fns["miopen"]().float()
        rel = {n: ((fns[n]() - ref).abs().max().item()
                   / max(ref.abs().max().item(), 1e-3)) for n in names[:3]}
        tag = f"C{C}->K{C} {hw}x{hw} k{R}x{S} N{N}"
        print(f"{tag:<34}"
              + "".join(f"{t[n]:9.3f}ms" for n in names) + "   "
              + " ".join(f"{t['miopen'] / t[n]:5.2f}x" for n in names[:4])
              + f"  {t['bwdw'] / t['tap']:5.2f}x  {t['tap'] / t['ring']:5.2f}x"
              f"  {t['ring'] / t['px']:5.2f}x  {min(t, key=t.get):<7}"
              f"[{ge.tap_bwdw_px_kernel_name(N, C, C, hw, hw, R, S, ph, pw)}, "
              f"{ge.tap_bwdw_ring_kernel_name(N, C, C, hw, hw, R, S, ph, pw)}, "
              f"{ge.tap_bwdw_kernel_name(N, C, C, hw, hw, R, S, ph, pw)}]"
              f"  px relerr {rel['px']:.3g} ring relerr {rel['ring']:.3g}"
              f" tap relerr {rel['tap']:.3g}",
              flush=True)


def model_pw_shapes(num_layers=18, num_filters=416, image=2048, mb=2):
    """Every distinct 1x1 conv shape the flagship model runs (meta pass)."""
    from mpi4dl_amd.models.amoebanet import amoebanetd
    from mpi4dl_amd.ops.conv_native import NativeConv2d

    shapes = {}
    orig = NativeConv2d.forward

    def probe(self, x):
        kh, kw = (
            (self.kernel_size, self.kernel_size)
            if isinstance(self.kernel_size, int)
            else self.kernel_size
        )
        if (kh, kw) == (1, 1):
            s = self.stride[0] if isinstance(self.stride, tuple) else self.stride
            key = (x.shape[1], self.out_channels, x.shape[2], x.shape[3], s)
            shapes[key] = shapes.get(key, 0) + 1
        return orig(self, x)

    NativeConv2d.forward = probe
    try:
        with torch.device("meta"):
            m = amoebanetd(1000, num_layers, num_filters)
            m(torch.zeros(mb, 3, image, image))
    finally:
        NativeConv2d.forward = orig
    return shapes


def pw_ab(args):
    """1x1 conv A/B: conv_pw streaming GEMM vs MIOpen, fwd + autograd,
    on the exact shapes of the flagship model."""
    from mpi4dl_amd.ops import backend
    from mpi4dl_amd.ops.conv_native import native_conv2d

    ge = backend.ext()
    shapes = model_pw_shapes(mb=args.batch)
    print(f"{'shape (xN uses)':<40} {'pw':>9} {'miopen':>9} {'ratio':>6}")
    tot_n = tot_m = 0.0
    for (C, K, H, W, s), uses in sorted(shapes.items()):
        x = torch.randn(args.batch, C, H, W, device="cuda", dtype=torch.bfloat16)
        w = torch.randn(K, C, 1, 1, device="cuda", dtype=torch.bfloat16) * 0.05
        tn = timeit(lambda: ge.pw_fwd(x, w, None, s, s), args.iters)
        tm = timeit(
            lambda: torch.nn.functional.conv2d(x, w, stride=s), args.iters
        )
        y = ge.pw_fwd(x, w, None, s, s).float()
        ref = torch.nn.functional.conv2d(x.float(), w.float(), stride=s)
        rel = (y - ref).abs().max().item() / max(ref.abs().max().item(), 1e-3)
        tag = f"C{C}->K{K} {H}x{W} s{s} (x{uses})"
        print(f"{tag:<40} {tn:8.3f}ms {tm:8.3f}ms {tm/tn:5.2f}x  relerr {rel:.3g}",
              flush=True)
        tot_n += tn * uses
        tot_m += tm * uses
        # autograd legs
        xg = x.clone().requires_grad_(True)
        wf = w.float().requires_grad_(True)
        g = torch.randn_like(ref).to(torch.bfloat16)

        def nat_step():
            yy = native_conv2d(xg, wf, None, (s, s), (0, 0))
            yy.backward(g)
            xg.grad = None
            wf.grad = None

        x2 = x.clone().requires_grad_(True)
        w2 = w.float().requires_grad_(True)

        def ref_step():
            yy = torch.nn.functional.conv2d(
                x2, w2.to(torch.bfloat16), stride=s
            )
            yy.backward(g)
            x2.grad = None
            w2.grad = None

        # grad correctness
        yy = native_conv2d(xg, wf, None, (s, s), (0, 0))
        yy.backward(g)
        ry = torch.nn.functional.conv2d(x2.float(), w2, stride=s)
        ry.backward(g.float())
        relx = (xg.grad.float() - x2.grad).abs().max().item() / max(
            x2.grad.abs().max().item(), 1e-3
        )
        relw = (wf.grad - w2.grad).abs().max().item() / max(
            w2.grad.abs().max().item(), 1e-3
        )
        xg.grad = wf.grad = x2.grad = w2.grad = None
        tn2 = timeit(nat_step, max(args.iters // 2, 3))
        tm2 = timeit(ref_step, max(args.iters // 2, 3))
        print(f"{'':<40} f+b {tn2:8.3f}ms {tm2:8.3f}ms {tm2/tn2:5.2f}x  "
              f"relgx {relx:.3g} relgw {relw:.3g}", flush=True)
    print(f"\nuse-weighted fwd total: pw {tot_n:.2f}ms vs miopen {tot_m:.2f}ms "
          f"({tot_m/max(tot_n,1e-9):.2f}x)")


def bwdw_ab(args):
    """pw_bwdw vs torch conv2d_weight on the flagship 1x1 shapes."""
    from mpi4dl_amd.ops import backend

    ge = backend.ext()
    shapes = model_pw_shapes(mb=args.batch)
    print(f"{'shape (xN uses)':<40} {'pw_bwdw':>9} {'torch':>9} {'ratio':>6}")
    tot_n = tot_m = 0.0
    for (C, K, H, W, s), uses in sorted(shapes.items()):
        if s != 1:
            continue
        x = torch.randn(args.batch, C, H, W, device="cuda", dtype=torch.bfloat16)
        go = torch.randn(args.batch, K, H, W, device="cuda", dtype=torch.bfloat16)
        tn = timeit(lambda: ge.pw_bwdw(go, x), args.iters)
        tm = timeit(
            lambda: torch.nn.grad.conv2d_weight(
                x, (K, C, 1, 1), go, stride=1, padding=0
            ),
            args.iters,
        )
        gw = ge.pw_bwdw(go, x)
        ref = torch.nn.grad.conv2d_weight(
            x.float(), (K, C, 1, 1), go.float(), stride=1, padding=0
        ).view(K, C)
        rel = (gw - ref).abs().max().item() / max(ref.abs().max().item(), 1e-3)
        tag = f"C{C}->K{K} {H}x{W} (x{uses})"
        print(f"{tag:<40} {tn:8.3f}ms {tm:8.3f}ms {tm/tn:5.2f}x  relerr {rel:.3g}",
              flush=True)
        tot_n += tn * uses
        tot_m += tm * uses
    print(f"\nuse-weighted bwdw total: pw {tot_n:.2f}ms vs torch {tot_m:.2f}ms "
          f"({tot_m/max(tot_n,1e-9):.2f}x)")


def matmul_ab(args):
    """Fat 1x1 shapes: pw kernels vs a plain hipBLASLt matmul view
    (w[K,C] @ x[N,C,HW]) — the 'plain library GEMM' alternative."""
    from mpi4dl_amd.ops import backend

    ge = backend.ext()
    shapes = model_pw_shapes(mb=args.batch)
    print(f"{'shape (xN uses)':<40} {'pw':>9} {'matmul':>9} {'ratio':>6}"
          f" | {'bwdw':>9} {'einsum':>9} {'ratio':>6}")
    for (C, K, H, W, s), uses in sorted(shapes.items()):
        if s != 1:
            continue
        x = torch.randn(args.batch, C, H, W, device="cuda", dtype=torch.bfloat16)
        w = torch.randn(K, C, device="cuda", dtype=torch.bfloat16) * 0.05
        w4 = w.view(K, C, 1, 1)
        xv = x.view(args.batch, C, H * W)
        tn = timeit(lambda: ge.pw_fwd(x, w4, None, 1, 1), args.iters)
        tm = timeit(lambda: torch.matmul(w, xv), args.iters)
        y = ge.pw_fwd(x, w4, None, 1, 1).float()
        ref = torch.matmul(w.float(), xv.float()).view(args.batch, K, H, W)
        rel = (y - ref).abs().max().item() / max(ref.abs().max().item(), 1e-3)
        # bwd-weight: native NT GEMM vs bmm+sum through hipBLASLt
        go = torch.randn(args.batch, K, H, W, device="cuda", dtype=torch.bfloat16)
        gv = go.view(args.batch, K, H * W)
        tb = timeit(lambda: ge.pw_bwdw(go, x), args.iters)
        te = timeit(
            lambda: torch.bmm(gv, xv.transpose(1, 2)).sum(dim=0), args.iters
        )
        tag = f"C{C}->K{K} {H}x{W} (x{uses})"
        print(f"{tag:<40} {tn:8.3f}ms {tm:8.3f}ms {tm/tn:5.2f}x"
              f" | {tb:8.3f}ms {te:8.3f}ms {te/tb:5.2f}x  relerr {rel:.3g}",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--winograd", action="store_true",
                    help="A/B the fused Winograd kernel, the bmm staging and "
                         "the direct kernel vs MIOpen on the 3x3 stride-1 "
                         "shapes")
    ap.add_argument("--tap", action="store_true",
                    help="A/B the tap-shift kernel and the direct kernel vs "
                         "MIOpen on the stride-1 1x7, 7x1 and 3x3 shapes, "
                         "forward and data-grad")
    ap.add_argument("--tap-strided", action="store_true",
                    help="A/B the strided tap-shift kernels vs the native "
                         "routes and MIOpen on the strided 1x7 / 7x1 / 3x3 "
                         "shapes, forward and data-grad")
    ap.add_argument("--tap-bwdw", action="store_true",
                    help="A/B the tap-shift weight-gradient kernels (rolling "
                         "window and first) and conv_bwd_weight vs MIOpen on "
                         "the shapes of --tap")
    ap.add_argument("--pw", action="store_true",
                    help="A/B the conv_pw 1x1 kernel vs MIOpen on the "
                         "flagship model's 1x1 shapes")
    ap.add_argument("--bwdw", action="store_true",
                    help="A/B pw_bwdw vs torch conv2d_weight")
    ap.add_argument("--matmul", action="store_true",
                    help="A/B pw fat kernels vs a plain hipBLASLt matmul")
    args = ap.parse_args()
    if args.matmul:
        return matmul_ab(args)
    if args.winograd:
        return winograd_ab(args)
    if args.tap:
        return tap_ab(args)
    if args.tap_strided:
        return tap_strided_ab(args)
    if args.tap_bwdw:
        return tap_bwdw_ab(args)
    if args.pw:
        return pw_ab(args)
    if args.bwdw:
        return bwdw_ab(args)
    from mpi4dl_amd.ops import backend

    ge = backend.ext()
    print(f"{'shape':<42} {'native':>9} {'miopen':>9} {'ratio':>6}")
    for C, K, H, W, kh, kw, s, ph, pw in SHAPES:
        x = torch.randn(args.batch, C, H, W, device="cuda", dtype=torch.bfloat16)
        w = torch.randn(K, C, kh, kw, device="cuda", dtype=torch.bfloat16) * 0.05
        tn = timeit(lambda: ge.conv_fwd(x, w, None, s, s, ph, pw), args.iters)
        tm = timeit(
            lambda: torch.nn.functional.conv2d(x, w, stride=s, padding=(ph, pw)),
            args.iters,
        )
        # correctness spot-check
        y = ge.conv_fwd(x, w, None, s, s, ph, pw).float()
        ref = torch.nn.functional.conv2d(x, w, stride=s, padding=(ph, pw)).float()
        rel = (y - ref).abs().max().item() / max(ref.abs().max().item(), 1e-3)
        tag = f"C{C}->K{K} {H}x{W} k{kh}x{kw} s{s}"
        print(f"{tag:<42} {tn:8.3f}ms {tm:8.3f}ms {tm/tn:5.2f}x  relerr {rel:.3g}")
        # full autograd step (fwd+bwd) A/B
        if True:
            from mpi4dl_amd.ops.conv_native import native_conv2d

            wf = w.float().requires_grad_(True)
            xg = x.clone().requires_grad_(True)
            g = torch.randn_like(ref).to(torch.bfloat16)

            def nat_step():
                y = native_conv2d(xg, wf, None, (s, s), (ph, pw))
                y.backward(g)
                xg.grad = None
                wf.grad = None

            x2 = x.clone().requires_grad_(True)
            w2 = w.float().requires_grad_(True)

            def ref_step():
                y = torch.nn.functional.conv2d(x2, w2.to(torch.bfloat16),
                                               stride=s, padding=(ph, pw))
                y.backward(g)
                x2.grad = None
                w2.grad = None

            tn2 = timeit(nat_step, max(args.iters // 2, 3))
            tm2 = timeit(ref_step, max(args.iters // 2, 3))
            print(f"{'':<42} fwd+bwd {tn2:8.3f}ms {tm2:8.3f}ms {tm2/tn2:5.2f}x")


if __name__ == "__main__":
    main()
