#!/usr/bin/env python3
"""Flagship benchmark: AmoebaNet-D training at 2048x2048 with SP+PP
(BASELINE.json metric: "img/sec AmoebaNet-D 2048x2048 SP+PP at 1/2/4/8
MI355X").

Launch (driver contract):
  python bench.py --gpus N --steps K --warmup W
  # N>1 via: python -m torch.distributed.run --nnodes=1 --nproc-per-node N
  #          --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints the result
line; nothing else is measured. --dump-outputs DIR additionally writes
what the last timed step computed as DIR/<name>.npy; that step then
starts from the seeded weights again, so with the same arguments its
inputs are identical from run to run and two builds can be compared
output for output (see SeededState). --full is
where secondary measurements belong; there are none today.

Topology per N (strong scaling, fixed global batch):
  N=1: whole model on one GPU (engine degenerates, same code path)
  N=2: 2 pipeline stages (PP)
  N=4: 2 spatial tiles on the first partition + 2 more LP stages (SP+PP)
  N=8: 4 spatial tiles + 4 more LP stages (SP+PP)

Synthetic data (no network for datasets), random-init weights,
loss/optimizer step included in the timed region. One JSON line on
rank 0. Default compute dtype is bf16 autocast; note the reference's
published numbers are fp32 on different (NVIDIA) hardware, so
vs_baseline is context, not a controlled same-precision A/B — run
--dtype fp32 for the like-for-like precision datum
(profiles/PERF_NOTES.md records both).
"""

from __future__ import annotations

import argparse
import collections
import json
import os
import sys
import time

# At >=4096^2 MIOpen's first-touch per-shape solution search takes minutes;
# FAST (immediate) mode avoids it. Kept off at the default 2048^2 config so
# steady-state algorithm choice is unaffected there.
if any(a.startswith("--image-size") for a in sys.argv):
    try:
        _i = [i for i, a in enumerate(sys.argv) if a.startswith("--image-size")][0]
        _v = sys.argv[_i].split("=")[1] if "=" in sys.argv[_i] else sys.argv[_i + 1]
        if int(_v) > 2048:
            os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    except (IndexError, ValueError):
        pass
# Multi-rank runs: 8 processes running the exhaustive find concurrently
# contend on the shared find-db file locks (serialized minutes-long finds
# can outlive the warmup). FAST keeps the multi-GPU warmup bounded; the
# N=1 headline still runs the full find.
if int(os.environ.get("WORLD_SIZE", "1")) > 1:
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")

# MIOpen's first-touch solution search also times its naive reference
# convolutions (30-140 ms per launch at these shapes, ~18 s of GPU time
# per cold-cache run). They never win a search here, so leaving them
# out shortens the first step of a run without changing which kernels
# the timed steps run. A convolution whose ONLY applicable solver is the
# naive one would now raise "no solution" instead of running slowly;
# the default configuration has no such shape (every convolution of a
# plain bf16 run, forward and backward, finds a solver with these
# switches off, and the run fails loudly otherwise). Export the three
# variables as 1 to bring the naive solvers back for unusual shapes.
for _d in ("FWD", "BWD", "WRW"):
    os.environ.setdefault(f"MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_{_d}", "0")

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# reference best published number on this metric/config:
# AmoebaNet-D 2048^2 SP-vert-D2 B=2 ~= 5.0 img/s
# NOTE: "metric" in the JSON is BASELINE.json's label for the benchmark
# FAMILY; the ACTUAL topology of a given run is config.parallelism
# ("single" at N=1 — no SP/PP runs on one GPU).
BASELINE_IMGS = 5.0


def topology(n: int):
    if n == 1:
        return dict(split_size=1, nsp=1, spatial_size=0)
    if n == 2:
        return dict(split_size=2, nsp=1, spatial_size=0)
    if n == 4:
        return dict(split_size=3, nsp=2, spatial_size=1)
    if n == 8:
        return dict(split_size=5, nsp=4, spatial_size=1)
    raise SystemExit(f"unsupported GPU count {n} (use 1/2/4/8)")


def make_balance(ncells: int, split: int, spatial_size: int):
    """Spatial partitions hold the early high-resolution cells (stem + 2
    reduction cells); remaining cells spread evenly over LP stages."""
    if split == 1:
        return [ncells]
    if spatial_size == 0:
        base, rem = divmod(ncells, split)
        return [base + (1 if i < rem else 0) for i in range(split)]
    sp_cells = 3  # stem + stem2 + stem3: the 1024^2..256^2 activations
    rest = ncells - sp_cells
    lp = split - spatial_size
    base, rem = divmod(rest, lp)
    return [sp_cells] + [base + (1 if i < rem else 0) for i in range(lp)]


MAX_DUMP_BYTES = 64 * 2**20
PARAM_SAMPLE = 1 << 18  # parameter elements written per optimizer


def _recording(criterion, sink):
    """Wrap a loss function so each call's (logits, loss) lands in `sink`.
    The detached tensors share storage with the live ones: under hipGraph
    capture that storage is static, so after a replay they hold that
    replay's values; no autograd state is kept alive."""

    def wrapped(logits, target):
        loss = criterion(logits, target)
        sink.append((logits.detach(), loss.detach()))
        return loss

    return wrapped


class SeededState:
    """The training state as seeding left it: a copy of the parameters,
    momentum zero. The weight-gradient kernels accumulate with fp32
    atomics, so parameters differ from run to run in their last bits
    after one update, and this model amplifies that ~1e4x per step: five
    steps in, two runs of one build disagree in the first digit. With
    --dump-outputs the last timed step therefore starts from this state
    again, which makes what it computes a function of the seeds alone,
    up to the order of the atomic adds within that one step (last bits
    of the updated parameters; nothing amplifies them before the dump).
    restore() is two stream-ordered device copies (in place, so a
    captured graph keeps reading the same addresses)."""

    def __init__(self, optimizers):
        self.optimizers = optimizers
        self.saved = [[p.detach().clone() for p in self._params(o)]
                      for o in optimizers]

    @staticmethod
    def _params(opt):
        if hasattr(opt, "flat_p"):  # FusedSGD: one flat buffer
            return [opt.flat_p]
        return [p for g in opt.param_groups for p in g["params"]]

    @torch.no_grad()
    def restore(self):
        for opt, saved in zip(self.optimizers, self.saved):
            torch._foreach_copy_(self._params(opt), saved)
            if hasattr(opt, "flat_m"):
                opt.flat_m.zero_()
            else:  # torch SGD: a zero buffer acts like a first step
                for st in opt.state.values():
                    if st.get("momentum_buffer") is not None:
                        st["momentum_buffer"].zero_()


def dump_outputs(dirname, rank, world, recorded, optimizers):
    """Write what the last timed step computed as float32 .npy files:
    what its loss function received and returned, `logits` [batch,
    classes] and `loss` [micro-batches], on ranks that hold the last
    stage; and on every rank `params_sample`, a fixed seeded sample of
    the parameters as the step's backward pass and optimizer update left
    them. Ranks of a multi-process run suffix their files with _rank<r>."""
    import numpy as np

    out = {}
    if recorded:
        out["loss"] = torch.stack([loss.reshape(()) for _, loss in recorded])
        out["logits"] = torch.cat([logits for logits, _ in recorded])
    gen = torch.Generator().manual_seed(0)
    picks = []
    for opt in optimizers:
        tensors = SeededState._params(opt)
        per = max(256, PARAM_SAMPLE // max(len(tensors), 1))
        for t in tensors:
            idx = torch.randint(t.numel(), (min(t.numel(), per),),
                                generator=gen)
            picks.append(t.detach().reshape(-1)[idx.to(t.device)].float())
    if picks:
        out["params_sample"] = torch.cat(picks)
    arrays = {k: v.float().cpu().numpy() for k, v in out.items()}
    assert sum(a.nbytes for a in arrays.values()) <= MAX_DUMP_BYTES
    os.makedirs(dirname, exist_ok=True)
    sfx = "" if world == 1 else f"_rank{rank}"
    for name, a in arrays.items():
        np.save(os.path.join(dirname, f"{name}{sfx}.npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--image-size", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=8, help="global batch per step")
    ap.add_argument("--parts", type=int, default=None,
                    help="pipeline micro-batches (default: 4 at N=1 — micro-batch 2\n"
                         "measured +12% over mb=1; 8 when pipelining)")
    ap.add_argument("--num-layers", type=int, default=18)
    ap.add_argument("--num-filters", type=int, default=416)
    ap.add_argument("--num-classes", type=int, default=1000)
    ap.add_argument("--slice-method", default="vertical")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--schedule", default="gpipe", choices=["gpipe", "1f1b"],
                    help="pipeline schedule (1f1b = PipeDream-flush memory profile)")
    ap.add_argument("--gems", action="store_true",
                    help="GEMS bidirectional pipelines on top of SP "
                         "(two mirrored engines per GPU, 2x batch/step)")
    ap.add_argument("--ref-quirks", action="store_true",
                    help="reproduce the reference model bitwise (its "
                         "max_pool_3x3 builder creates an AvgPool; see "
                         "models/amoebanet.py)")
    ap.add_argument("--act-ckpt", action="store_true",
                    help="recompute cell forwards in backward (fits larger "
                         "global batches in HBM at ~1 extra forward cost)")
    ap.add_argument("--grad-mode", default="drop", choices=["drop", "exact"],
                    help="halo backward: 'drop' = reference semantics + "
                         "halo/compute overlap (benchmark default); "
                         "'exact' = transposed-gradient exchange")
    ap.add_argument("--no-overlap-grads", action="store_true",
                    help="disable bucketed allreduce-during-backward on the "
                         "primary gradient group (overlap is the default)")
    ap.add_argument("--no-hipgraph", action="store_true",
                    help="disable hipGraph capture of the N=1 step")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed "
                         "step computed (logits and per-micro-batch loss on "
                         "the last stage, a seeded sample of the updated "
                         "parameters) as DIR/<name>.npy; that step starts "
                         "from the seeded weights again, and restoring "
                         "them (two device copies) falls inside the timed "
                         "region, so ms_per_step of such a run is not "
                         "exactly that of a plain run")
    ap.add_argument("--lr", type=float, default=0.01,
                    help="SGD learning rate")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements and checks; "
                         "this benchmark has none beyond the headline, so "
                         "the flag is accepted and changes nothing")
    args = ap.parse_args()

    # multi-rank: arm the P2P watchdog so an ordering bug produces a
    # diagnosis (pending peer set) instead of a silent driver timeout
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        os.environ.setdefault("MPI4DL_WAIT_TIMEOUT", "300")

    from mpi4dl_amd.comm import Communicator, GradReducer, init_distributed
    from mpi4dl_amd.models.amoebanet import amoebanetd
    from mpi4dl_amd.ops.plan import SpatialPlan
    from mpi4dl_amd.parallel.partition import model_generator
    from mpi4dl_amd.parallel.pipeline import train_model
    from mpi4dl_amd.parallel.spatial import train_model_spatial

    world = int(os.environ.get("WORLD_SIZE", "1"))
    n = args.gpus if args.gpus else world
    assert world in (1, n), f"WORLD_SIZE {world} != --gpus {n}"
    on_gpu = torch.cuda.is_available()
    device = None
    init_distributed()
    rank = dist.get_rank()
    if on_gpu:
        device = torch.device("cuda", torch.cuda.current_device())
    else:
        device = torch.device("cpu")

    topo = topology(n)
    S = args.image_size
    if args.parts is None:
        # N=1 has no pipeline: micro-batch 2 measured +12% over mb=1
        # (kernel efficiency); pipelined runs need parts >= stages
        args.parts = 4 if n == 1 else 8
    B, parts = args.batch, args.parts
    mb = B // parts
    autocast_dtype = torch.bfloat16 if (args.dtype == "bf16" and on_gpu) else None
    act_dtype = torch.bfloat16 if autocast_dtype else torch.float32

    spatial = topo["spatial_size"] > 0 and world > 1
    comm = Communicator(
        split_size=topo["split_size"],
        ENABLE_SPATIAL=spatial,
        num_spatial_parts=topo["nsp"],
        spatial_size=topo["spatial_size"] if spatial else 0,
        ENABLE_GEMS=args.gems,
    )

    # model (full, cells) — probe cell count cheaply on meta
    def build(plan=None):
        torch.manual_seed(0)
        return amoebanetd(args.num_classes, args.num_layers, args.num_filters,
                          plan, ref_quirks=args.ref_quirks)

    if spatial:
        with torch.device("meta"):
            ncells = len(build())
        planless = None
    else:
        # no plan to wait for: the probe is the model that trains
        planless = build()
        ncells = len(planless)
    balance = make_balance(ncells, topo["split_size"], topo["spatial_size"] if spatial else 0)

    use_gems = args.gems and spatial and world > 1

    def make_gen(plan, pos):
        model = planless if plan is None else build(plan)
        gen = model_generator(
            model, topo["split_size"], (mb, 3, S, S), balance=balance
        )
        gen.get_output_shapes()
        gen.ready_model(comm.get_split_rank(pos), device=device)
        return gen

    plan = (
        SpatialPlan(comm, balance, args.slice_method, grad_mode=args.grad_mode)
        if spatial
        else None
    )
    if use_gems:
        r = comm.rank % comm.mp_size
        plan2 = SpatialPlan(
            comm, balance, args.slice_method, grad_mode=args.grad_mode,
            gems_inverse=True,
        )
        gen = make_gen(plan, r)
        gen2 = make_gen(plan2, comm.mp_size - 1 - r)
    else:
        gen = make_gen(plan, comm.local_rank)

    if on_gpu:
        from mpi4dl_amd.optim import FusedSGD

        opt = FusedSGD(gen.models, lr=args.lr, momentum=0.9)
    else:
        opt = torch.optim.SGD(gen.models.parameters(), lr=args.lr, momentum=0.9)
    eng_kw = dict(
        optimizer=opt,
        device=device,
        autocast_dtype=autocast_dtype,
        act_dtype=act_dtype,
        schedule=args.schedule,
        act_ckpt=args.act_ckpt,
    )
    if use_gems:
        from mpi4dl_amd.parallel.gems import train_spatial_model_master

        if on_gpu:
            from mpi4dl_amd.optim import FusedSGD

            opt2 = FusedSGD(gen2.models, lr=args.lr, momentum=0.9)
        else:
            opt2 = torch.optim.SGD(gen2.models.parameters(), lr=args.lr, momentum=0.9)
        eng = train_spatial_model_master(
            gen, gen2, B, parts, comm, slice_method=args.slice_method,
            grad_mode=args.grad_mode, **eng_kw,
        )
        eng.train_model2.optimizer = opt2
    elif spatial:
        eng = train_model_spatial(
            gen, comm.local_rank, B, parts, comm,
            slice_method=args.slice_method, grad_mode=args.grad_mode, **eng_kw,
        )
    else:
        eng = train_model(gen, comm.local_rank, B, parts, comm, **eng_kw)
    reducer = GradReducer(comm)

    engines = ([eng.train_model1, eng.train_model2]
               if hasattr(eng, "train_model1") else [eng])
    recorded = seeded = None
    if args.dump_outputs:
        seeded = SeededState([opt, opt2] if use_gems else [opt])
        # one (logits, loss) pair per micro-batch of the latest step
        recorded = collections.deque(maxlen=parts * len(engines))
        for e in engines:
            e.criterion = _recording(e.criterion, recorded)

    # synthetic data of the benchmark shape
    torch.manual_seed(1234 + rank)
    B_step = 2 * B if use_gems else B  # GEMS runs two replicas per step
    x = torch.randn(B_step, 3, S, S, device=device, dtype=torch.float32)
    y = torch.randint(0, args.num_classes, (B_step,), device=device)

    if use_gems:
        def step():
            loss, _, _ = eng.run_step(x, y)
            eng.allreduce_and_update()
            return loss
    else:
        # bucketed allreduce-during-backward on the primary gradient
        # group (spatial tiles here), on by default — the reference gets
        # this from its DDP wrap (mp_pipeline.py:92-124)
        overlap = (
            reducer.setup_overlap(eng.models)
            if (spatial or comm.dp_size > 1) and not args.no_overlap_grads
            else None
        )

        def step():
            loss, _, _ = eng.run_step(x, y)
            if overlap is not None:
                reducer.finish_overlap(eng.models)
                reducer.apply_allreduce(eng.models, skip_group=overlap["group"])
            elif spatial or comm.dp_size > 1:
                reducer.apply_allreduce(eng.models)
            eng.update()
            return loss

    def fence():
        if world > 1:
            dist.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    # N=1: capture the whole step (fwd+bwd+optimizer) in one hipGraph —
    # replay removes the ~5-6k per-step host launches of the eager path
    # (grad-accumulate adds, BN stat zero-fills). Requires the step to
    # be sync-free: engine metrics off, fixed input tensors (they are).
    # One eager step (first-touch tuning, allocator warmup) precedes the
    # capture; the W warmup steps then run as replays, like the timed
    # ones, instead of as W further eager passes.
    if (
        on_gpu and world == 1 and not use_gems and not args.no_hipgraph
        and args.warmup > 0
    ):
        try:
            for e in ([eng.train_model1, eng.train_model2]
                      if hasattr(eng, "train_model1") else [eng]):
                e.metrics_enabled = False
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()  # first-touch + allocator warmup, metrics off
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            step = graph.replay  # noqa: F811
            if rank == 0:
                print("# hipGraph capture active", file=sys.stderr)
        except Exception as exc:  # pragma: no cover - fallback to eager
            if rank == 0:
                print(f"# hipGraph capture unavailable: {exc}",
                      file=sys.stderr)
    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    for i in range(args.steps):
        if seeded is not None and i == args.steps - 1:
            seeded.restore()
        step()
    fence()
    elapsed = time.perf_counter() - t0

    # MAX over ranks
    t = torch.tensor([elapsed], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t[0])

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, rank, world, recorded,
                     seeded.optimizers)

    imgs_per_s = B_step * args.steps / elapsed
    peak_gb = (
        round(torch.cuda.max_memory_allocated() / 2**30, 2) if on_gpu else None
    )
    if rank == 0:
        par = "single" if n == 1 else (
            f"pp{topo['split_size']}" if not spatial
            else (f"sp{topo['nsp']}+gems+pp{topo['split_size']}" if use_gems
                  else f"sp{topo['nsp']}+pp{topo['split_size']}")
        )
        print(
            json.dumps(
                {
                    "metric": "img/sec AmoebaNet-D 2048x2048 SP+PP",
                    "value": imgs_per_s,
                    "unit": "img/s",
                    "n_gpus": n,
                    "steps": args.steps,
                    "warmup": args.warmup,
                    "ms_per_step": elapsed / args.steps * 1e3,
                    "higher_is_better": True,
                    "scaling": "strong",
                    "vs_baseline": imgs_per_s / BASELINE_IMGS,
                    "dtype": args.dtype if on_gpu else "fp32",
                    "data": "synthetic",
                    "config": {
                        "model": f"amoebanet-d(L{args.num_layers},F{args.num_filters})",
                        "global_batch": B_step,
                        "parts": parts,
                        "seq_len": None,
                        "image_size": S,
                        "parallelism": par,
                        "slice_method": args.slice_method if spatial else None,
                        "peak_hbm_gb": peak_gb,
                        "act_ckpt": args.act_ckpt,
                    },
                }
            ),
            flush=True,
        )


if __name__ == "__main__":
    main()
