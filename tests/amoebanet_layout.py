"""Structure of the AmoebaNet cells and models as plain data, and the
golden digests of it (tests/golden/amoebanet_layout.json).

``describe(module)`` lists what a refactor of models/amoebanet*.py must
not move: every submodule's path, class and layout attributes, the
state-dict keys and shapes in order, and a CellD2's halo needs.
``python tests/amoebanet_layout.py --write`` regenerates the golden.
"""

import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "amoebanet_layout.json")

ATTRS = (
    "stat_margin", "relu", "d2", "halo_len", "kind", "kernel_size", "stride",
    "padding", "count_include_pad", "op_need",
)

# hand-made plan ctx: rank_of_tile=None needs no process group
CTXS = {
    "plain": None,
    "vertical2_tile0": ("vertical", 2, 0),
    "horizontal2_tile1": ("horizontal", 2, 1),
    "square4_tile3": ("square", 4, 3),
}


def _plain(v):
    import torch.nn as nn

    if isinstance(v, nn.Module):
        return f"<{type(v).__name__}>"
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    assert v is None or isinstance(v, (bool, int, float, str)), v
    return v


def describe(module):
    modules = []
    for path, m in module.named_modules():
        attrs = {a: _plain(getattr(m, a)) for a in ATTRS if hasattr(m, a)}
        modules.append([path, type(m).__name__, attrs])
    state = [[k, list(v.shape)] for k, v in module.state_dict().items()]
    return {"modules": modules, "state_dict": state}


def _ctx(spec):
    if spec is None:
        return None
    method, parts, tile = spec
    return dict(
        num_spatial_parts=parts, slice_method=method, spatial_local_rank=tile,
        rank_of_tile=None, grad_mode="exact",
    )


def cases():
    """name -> zero-argument builder of the module to describe."""
    from mpi4dl_amd.models.amoebanet import Cell, amoebanetd
    from mpi4dl_amd.models.amoebanet_d2 import CellD2, amoebanetd_d2
    from mpi4dl_amd.ops.norm import TileBatchNorm2d

    out = {}
    for cls in (Cell, CellD2):
        for reduction in (False, True):
            for cname, spec in CTXS.items():
                kind = "reduction" if reduction else "normal"
                out[f"{cls.__name__}-{kind}-{cname}"] = (
                    lambda cls=cls, reduction=reduction, spec=spec: cls(
                        64, 64, 32, reduction, False, ctx=_ctx(spec),
                        mknorm=TileBatchNorm2d,
                    )
                )
    out["amoebanetd"] = lambda: amoebanetd(10, 3, 32)
    out["amoebanetd_d2"] = lambda: amoebanetd_d2(10, 3, 32)
    return out


def _sha(obj, n=None):
    text = json.dumps(obj, sort_keys=True, separators=(",", ":"))
    return hashlib.sha256(text.encode()).hexdigest()[:n]


def digest(desc):
    """One sha256 over the canonical JSON of a description; the short
    per-module digests only serve to name the first module that moved."""
    return {
        "sha256": _sha(desc),
        "modules": [_sha(m, 8) for m in desc["modules"]],
    }


def first_difference(desc, want):
    """Where ``desc`` first leaves the golden entry ``want`` (None: nowhere)."""
    got = digest(desc)
    if got["sha256"] == want["sha256"]:
        return None
    for i, (a, b) in enumerate(zip(got["modules"], want["modules"])):
        if a != b:
            return "module %d: %r" % (i, desc["modules"][i])
    if len(got["modules"]) != len(want["modules"]):
        return "%d modules, golden has %d" % (
            len(got["modules"]), len(want["modules"]))
    return "state_dict keys or shapes (all modules agree)"


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def main(argv):
    if argv != ["--write"]:
        raise SystemExit("usage: python tests/amoebanet_layout.py --write")
    sys.path.insert(0, ROOT)
    golden = {name: digest(describe(make())) for name, make in cases().items()}
    rows = [
        "%s: %s" % (json.dumps(name), json.dumps(golden[name], sort_keys=True))
        for name in sorted(golden)
    ]
    with open(GOLDEN, "w") as f:  # one case per line
        f.write("{\n" + ",\n".join(rows) + "\n}\n")
    print(f"wrote {len(golden)} cases to {GOLDEN}")


if __name__ == "__main__":
    main(sys.argv[1:])
