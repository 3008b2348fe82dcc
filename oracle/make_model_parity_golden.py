#!/usr/bin/env python3
"""Record the reference side of tests/test_model_parity.py.

    python oracle/make_model_parity_golden.py --reference <MPI4DL checkout>

Builds the reference models (its src/models package), gives them the
seeded values the tests load into ours, runs them once in eval mode on
CPU and writes tests/golden/model_parity.json (cell counts, parameter
counts and shapes) and tests/golden/model_parity_outputs.npz (every
output tensor, whole or as a seeded sample, see tests/parity_util.py). Only results are written; nothing of the
reference's code is copied.
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import parity_util as tmp  # noqa: E402


def _params(m):
    return sum(p.numel() for p in m.parameters())


def ref_resnet_v2_tensors(ref, ours):
    """Reference tensors in the order of tmp.resnet_v2_seeds(ours)."""
    import torch.nn as nn

    cr, co = list(ref), list(ours)
    assert len(cr) == len(co)
    st = cr[0]
    out = [st.conv1.weight, st.conv1.bias] + tmp.bn_tensors(st.batch_last)
    for r, o in zip(cr[1:-1], co[1:-1]):
        pre1 = not isinstance(o.pre1, nn.Identity)
        for layer, has_bn in ((r.r1, pre1), (r.r2, True), (r.r3, True)):
            out += [layer.conv1.weight, layer.conv1.bias]
            if has_bn:
                out += tmp.bn_tensors(layer.batch_first)
        assert hasattr(r, "r4") == (o.proj is not None)
        if hasattr(r, "r4"):
            out += [r.r4.conv1.weight, r.r4.conv1.bias]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True,
                    help="root of a checkout of the reference project")
    args = ap.parse_args()
    src = os.path.join(args.reference, "src")
    sys.path.insert(0, src)
    import models.amoebanet as ref_amoeba
    import models.resnet as ref_resnet

    sys.path.remove(src)
    import mpi4dl_amd.models.resnet as ours_r

    meta, outs = {"resnet": {}}, {}
    x = tmp.parity_input()

    for ver, n in ((1, 2), (2, 3)):
        depth = (6 if ver == 1 else 9) * n + 2
        m = getattr(ref_resnet, f"get_resnet_v{ver}")(
            (2, 3, 64, 64), depth, num_classes=10)
        meta["resnet"][f"v{ver}_n{n}"] = {"cells": len(m), "params": _params(m)}

    ref = ref_resnet.get_resnet_v2((2, 3, 64, 64), 29, num_classes=10)
    ours = ours_r.get_resnet_v2((2, 3, 64, 64), 10, n=3)
    seeds = tmp.resnet_v2_seeds(ours)
    tensors = ref_resnet_v2_tensors(ref, ours)
    assert len(seeds) == len(tensors)
    for (s, o), t in zip(seeds, tensors):
        assert o.shape == t.shape, (s, o.shape, t.shape)
        tmp.seeded_fill_(t, s)
    ref.eval()
    y = x
    with torch.no_grad():
        for c in list(ref)[:-1]:
            y = c(y)
    meta["resnet_v2_trunk"] = {
        "seeds": [s for s, _ in seeds],
        "shapes": [list(t.shape) for t in tensors],
        "out_shape": list(y.shape),
    }
    outs["resnet_v2_trunk"] = tmp.sample(y).numpy()

    ref = ref_amoeba.amoebanetd(num_classes=100, num_layers=6, num_filters=64)
    for s, p in tmp.amoebanet_seeds(ref):
        tmp.seeded_fill_(p, s)
    ref.eval()
    out_shapes = []
    y = x
    with torch.no_grad():
        for ci, c in enumerate(list(ref)):
            y = c(y)
            ts = y if isinstance(y, tuple) else (y,)
            out_shapes.append([list(t.shape) for t in ts])
            for ti, t in enumerate(ts):
                assert torch.isfinite(t).all()
                outs[f"amoebanet_cell{ci}_{ti}"] = tmp.sample(t).numpy()
    meta["amoebanet"] = {
        "cells": len(ref),
        "params": _params(ref),
        "param_shapes": [list(p.shape) for p in ref.parameters()],
        "out_shapes": out_shapes,
    }

    gold = os.path.join(ROOT, "tests", "golden")
    os.makedirs(gold, exist_ok=True)
    with open(os.path.join(gold, "model_parity.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    np.savez(os.path.join(gold, "model_parity_outputs.npz"), **outs)
    for k, v in outs.items():
        print(k, v.shape, float(np.abs(v).max()))


if __name__ == "__main__":
    main()
