"""Architecture parity with the reference models: cell counts, parameter
counts and eval-mode forward outputs of our builders must track the
reference's.

The reference side is recorded under tests/golden/ (model_parity.json,
model_parity_outputs.npz) by oracle/make_model_parity_golden.py, which
runs the reference models once. Both sides take their weights from
`seeded_fill_`, so no weights are stored: the recorded outputs are what
the reference computes from exactly the values these tests load into our
models.

The live comparison was bitwise because both models ran on the same
machine. A recorded output meets a different CPU, whose convolution
kernels may add the same products in another order, so the comparison
allows fp32 reassociation error. Unit roundoff 2^-24 ~ 6e-8, random-walk
growth over the longest reduction (256*9 = 2304 terms, sqrt ~ 48) and
over the <= 30 stacked convolutions gives ~ 48 * 6e-8 * 30 ~ 9e-5,
relative to the size of the summed terms. An element that is small by
cancellation still carries the error of terms of the tensor's typical
size, so each element is held to RTOL * (|recorded| + rms of the
recorded tensor) with RTOL = 1e-4. Tensors up to 8192 elements are
recorded whole, larger ones as 8192 seeded positions (a committed file
stays under 1 MiB).
"""

import json
import os

import numpy as np
import pytest
import torch

from parity_util import (amoebanet_seeds, parity_input, resnet_v2_seeds,
                         sample, seeded_fill_)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL = 1e-4


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "model_parity.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(GOLDEN, "model_parity_outputs.npz")) as z:
        outs = {k: z[k] for k in z.files}
    return meta, outs


def _params(m):
    return sum(p.numel() for p in m.parameters())


def _close(got, want, what):
    want = torch.from_numpy(want)
    rms = float(want.square().mean().sqrt())
    bound = RTOL * (want.abs() + rms)
    excess = ((got - want).abs() - bound).max()
    assert rms > 0 and float(excess) <= 0, (what, float(excess), rms)


def test_amoebanet_param_parity(golden):
    from mpi4dl_amd.models.amoebanet import amoebanetd

    ref = golden[0]["amoebanet"]
    ours = amoebanetd(100, 6, 64)
    assert ref["cells"] == len(ours)
    assert ref["params"] == _params(ours), (
        ref["params"], _params(ours))  # exact: same genotype, same widths


@pytest.mark.parametrize("ver,n", [(1, 2), (2, 3)])
def test_resnet_param_parity(golden, ver, n):
    import mpi4dl_amd.models.resnet as ours_r

    ref = golden[0]["resnet"][f"v{ver}_n{n}"]
    ours = getattr(ours_r, f"get_resnet_v{ver}")((2, 3, 64, 64), 10, n=n)
    assert ref["cells"] == len(ours)
    rp, op = ref["params"], _params(ours)
    # small residual diff: our GAP head vs the reference's flatten head
    assert abs(rp - op) / rp < 0.02, (rp, op)


def test_resnet_v2_forward_equivalence(golden):
    """Load the values the reference v2 model was given into ours
    (structure-aware: the reference's resnet_layer holds one USED and one
    dead BatchNorm) and compare trunk outputs with the recorded ones."""
    import mpi4dl_amd.models.resnet as ours_r

    meta, outs = golden
    torch.manual_seed(1)  # different init on purpose: the fill must win
    ours = ours_r.get_resnet_v2((2, 3, 64, 64), 10, n=3)
    seeds = resnet_v2_seeds(ours)
    assert [s for s, _ in seeds] == meta["resnet_v2_trunk"]["seeds"]
    assert [list(t.shape) for _, t in seeds] == meta["resnet_v2_trunk"]["shapes"]
    for s, t in seeds:
        seeded_fill_(t, s)
    ours.eval()
    yo = parity_input()
    with torch.no_grad():
        for c in list(ours)[:-1]:
            yo = c(yo)
    assert list(yo.shape) == meta["resnet_v2_trunk"]["out_shape"]
    _close(sample(yo), outs["resnet_v2_trunk"], "trunk")


def test_amoebanet_forward_equivalence_ref_quirks(golden):
    """With ref_quirks=True (reproducing the reference's
    max_pool_3x3-is-actually-AvgPool builder, amoebanet.py:108-125) and
    the reference's parameter values loaded in order, our AmoebaNet-D
    matches the reference model, cell by cell and through the head."""
    from mpi4dl_amd.models.amoebanet import amoebanetd

    meta, outs = golden
    torch.manual_seed(1)
    ours = amoebanetd(100, 6, 64, ref_quirks=True)
    seeds = amoebanet_seeds(ours)
    assert [list(p.shape) for _, p in seeds] == meta["amoebanet"]["param_shapes"]
    for s, p in seeds:
        seeded_fill_(p, s)
    ours.eval()
    yo = parity_input()
    cells = list(ours)
    assert len(cells) == meta["amoebanet"]["cells"]
    with torch.no_grad():
        for ci, co in enumerate(cells):
            yo = co(yo)
            tb = yo if isinstance(yo, tuple) else (yo,)
            assert [list(b.shape) for b in tb] == meta["amoebanet"]["out_shapes"][ci]
            for ti, b in enumerate(tb):
                _close(sample(b), outs[f"amoebanet_cell{ci}_{ti}"], (ci, ti))
