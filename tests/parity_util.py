"""Helpers shared by tests/test_model_parity.py and the script that
records its reference side (oracle/make_model_parity_golden.py): the
seeded weight fill, the probe input, the recorded view of an output
tensor, and the seed lists that pair our tensors with the reference's."""

import torch

SAMPLE = 8192  # elements recorded per output tensor (smaller ones whole)


def seeded_fill_(t, seed):
    """Overwrite `t` with values that are bit-identical on every machine:
    16-bit integers from a seeded generator, scaled by exactly rounded
    elementwise arithmetic (no transcendental functions). Matrices and
    filters get a unit-gain range, vectors (biases, norm scales and
    statistics) a positive one so they are valid variances too."""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 1 << 16, tuple(t.shape), generator=gen)
    u = q.to(torch.float32) / 65536.0  # [0, 1)
    if t.dim() > 1:
        bound = (3.0 / t[0].numel()) ** 0.5
        u = (u - 0.5) * (2.0 * bound)
    else:
        u = u + 0.5
    with torch.no_grad():
        t.copy_(u)
    return t


def sample(t):
    """The recorded view of an output tensor: all of it up to SAMPLE
    elements, else SAMPLE seeded positions."""
    flat = t.detach().reshape(-1)
    if flat.numel() <= SAMPLE:
        return flat.clone()
    gen = torch.Generator().manual_seed(7)
    idx = torch.randint(flat.numel(), (min(SAMPLE, flat.numel()),), generator=gen)
    return flat[idx]


def parity_input():
    gen = torch.Generator().manual_seed(5)
    q = torch.randint(0, 1 << 16, (2, 3, 64, 64), generator=gen)
    return (q.to(torch.float32) / 65536.0 - 0.5) * 4.0


def amoebanet_seeds(model):
    """(seed, parameter) in registration order, which the reference
    shares (asserted through the recorded shapes)."""
    return [(100 + i, p) for i, p in enumerate(model.parameters())]


# seeds of one conv(+norm) slot: weight, bias, norm weight/bias/mean/var
_CONV, _NORM = (0, 1), (2, 3, 4, 5)


def bn_tensors(bn):
    return [bn.weight, bn.bias, bn.running_mean, bn.running_var]


def resnet_v2_seeds(ours):
    """(seed, tensor) for every tensor of our ResNet-v2 trunk that has a
    used counterpart in the reference (its resnet_layer holds one USED
    and one dead BatchNorm). Seed = 100 * cell + 10 * layer + slot."""
    import torch.nn as nn

    cells = list(ours)
    stem = cells[0]
    out = list(zip(_CONV, [stem[0].weight, stem[0].bias]))
    out += list(zip(_NORM, bn_tensors(stem[1])))
    for ci, co in enumerate(cells[1:-1], start=1):
        pre1 = None if isinstance(co.pre1, nn.Identity) else co.pre1[0]
        layers = [(co.conv1, pre1), (co.conv2, co.pre2[0]),
                  (co.conv3, co.pre3[0]), (co.proj, None)]
        for li, (conv, bn) in enumerate(layers, start=1):
            if conv is None:
                continue
            base = 100 * ci + 10 * li
            out += [(base + s, t) for s, t in zip(_CONV, [conv.weight, conv.bias])]
            if bn is not None:
                out += [(base + s, t) for s, t in zip(_NORM, bn_tensors(bn))]
    return out
