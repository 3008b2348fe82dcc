"""bench.py end-to-end at the driver's SCALE topologies, on gloo.

The round-end driver launches bench.py at N=1/2/4/8 (one rank per GPU
over RCCL). These tests run the SAME main() — same topology table, same
engine construction, same JSON contract — at world 2 (pp2), 4
(sp2+pp3) and 8 (sp4+pp5) on CPU, so a rendezvous/topology/balance bug
can't first appear on the 8-GPU box."""

import io
import json
import os
import sys

from dist_util import run_distributed


def _bench_body(rank, world, extra_argv):
    import bench

    argv = [
        "bench.py", "--gpus", str(world), "--steps", "1", "--warmup", "0",
        "--image-size", "64", "--batch", "8", "--num-layers", "6",
        "--num-filters", "16", "--num-classes", "10",
    ] + list(extra_argv)
    if "--image-size" in extra_argv:
        argv = [a for a in argv]  # extra_argv overrides the 64 default
        i = argv.index("--image-size")
        del argv[i:i + 2]
    old_argv, old_out = sys.argv, sys.stdout
    sys.argv = argv
    sys.stdout = cap = io.StringIO()
    try:
        bench.main()
    finally:
        sys.argv, sys.stdout = old_argv, old_out
    lines = [ln for ln in cap.getvalue().splitlines() if ln.startswith("{")]
    return json.loads(lines[-1]) if lines else None


def _check(out, world, parallelism):
    rank0 = out[0]
    assert rank0 is not None, "rank 0 printed no JSON"
    assert rank0["n_gpus"] == world
    assert rank0["config"]["parallelism"] == parallelism
    assert rank0["value"] > 0 and rank0["ms_per_step"] > 0
    for k in ("metric", "unit", "steps", "warmup", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data"):
        assert k in rank0, k
    # only rank 0 prints
    assert all(o is None for o in out[1:])


def test_bench_n1_dump_outputs(tmp_path):
    """--dump-outputs writes the last timed step's results as float32
    .npy; that step starts from the seeded weights, so two runs with
    the same arguments write identical files. --steps sets
    the number of timed steps and ms_per_step is per timed step."""
    import numpy as np

    outs = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        extra = ("--steps", "2", "--warmup", "1", "--full",
                 "--dump-outputs", d)
        res = run_distributed(_bench_body, 1, (extra,), timeout=300)
        _check(res, 1, "single")
        assert res[0]["steps"] == 2 and res[0]["warmup"] == 1
        # 8 images per step: value [img/s] and ms_per_step agree
        assert abs(res[0]["value"] * res[0]["ms_per_step"] / 8e3 - 1) < 1e-6
        outs.append({f: np.load(tmp_path / name / f)
                     for f in sorted(os.listdir(d))})
    a, b = outs
    assert sorted(a) == ["logits.npy", "loss.npy", "params_sample.npy"]
    assert a["logits.npy"].shape == (8, 10) and a["loss.npy"].shape == (4,)
    for f in a:
        assert a[f].dtype == np.float32 and np.isfinite(a[f]).all(), f
        assert np.array_equal(a[f], b[f]), f
    assert sum(v.nbytes for v in a.values()) <= 64 * 2**20
    # the dumped step restarts from the seeded weights: a run whose only
    # step is the first one computes the same arrays
    d = str(tmp_path / "c")
    run_distributed(_bench_body, 1, (("--dump-outputs", d),), timeout=300)
    for f in a:
        assert np.array_equal(a[f], np.load(tmp_path / "c" / f)), f
    # the parameter sample carries the step's backward pass and update:
    # another learning rate leaves the forward outputs alone and moves
    # the sampled parameters by exactly the ratio of the two rates
    d = str(tmp_path / "d")
    run_distributed(_bench_body, 1, (("--dump-outputs", d, "--lr", "0"),),
                    timeout=300)
    d = str(tmp_path / "e")
    run_distributed(_bench_body, 1, (("--dump-outputs", d, "--lr", "0.02"),),
                    timeout=300)
    p0, p2 = (np.load(tmp_path / n / "params_sample.npy") for n in "de")
    for n in "de":
        for f in ("logits.npy", "loss.npy"):
            assert np.array_equal(a[f], np.load(tmp_path / n / f)), (n, f)
    p1 = a["params_sample.npy"]
    moved = np.abs(p1 - p0)
    assert (moved > 0).mean() > 0.5  # the gradient reaches the sample
    assert np.allclose(p2 - p0, 2 * (p1 - p0), rtol=1e-4,
                       atol=1e-6 * float(np.abs(p0).max()))


def test_bench_n2_pp():
    out = run_distributed(_bench_body, 2, ((),), timeout=300)
    _check(out, 2, "pp2")


def test_bench_n4_sp_pp():
    out = run_distributed(_bench_body, 4, ((),), timeout=300)
    _check(out, 4, "sp2+pp3")


def test_bench_n8_sp_pp():
    # 128² so the deepest spatial cell's 4-way tile (W=4) still fits the
    # 1×7 halo of 3 — at 64² the tile is 2 wide and the loud halo-bounds
    # assertion fires (by design; the real config is 2048²)
    out = run_distributed(
        _bench_body, 8, (("--image-size", "128"),), timeout=600
    )
    _check(out, 8, "sp4+pp5")


def test_bench_n4_gems():
    out = run_distributed(_bench_body, 4, (("--gems",),), timeout=300)
    _check(out, 4, "sp2+gems+pp3")
    assert out[0]["config"]["global_batch"] == 16  # two replicas per step


def test_bench_n4_1f1b():
    out = run_distributed(_bench_body, 4, (("--schedule", "1f1b"),),
                          timeout=300)
    _check(out, 4, "sp2+pp3")


def test_bench_n8_gems():
    """Config-5 composition (SP+GEMS+PP on 8 ranks): the mp_size ==
    2*total_tiles boundary case of verify_spatial_master_config, two
    mirrored spatial engines, MASTER-OPT-capable pairing — the shape
    the driver would run as `bench.py --gpus 8 --gems`."""
    out = run_distributed(
        _bench_body, 8, (("--gems", "--image-size", "128"),), timeout=600
    )
    _check(out, 8, "sp4+gems+pp5")
    assert out[0]["config"]["global_batch"] == 16


def test_bench_n4_act_ckpt():
    out = run_distributed(_bench_body, 4, (("--act-ckpt",),), timeout=400)
    _check(out, 4, "sp2+pp3")
    assert out[0]["config"]["act_ckpt"] is True
