"""Every native convolution kernel path against the fp64 oracle (MI355X).

One test per case of ``conv_oracle.CASES``: the entry point runs once on
the GPU, the results go to the CPU, and every element of every leg must
lie within the derived bound of the float64 reference (``conv_oracle``'s
docstring has the bound). Each case's label must be what production code
picks (``conv_oracle.expected_path`` asks ``conv_plan`` and the
extension's kernel-name functions), and a recorder around the extension
asks the same name functions about every binding call that really
happens. ``test_conv_oracle.py`` checks the labels without a GPU.
"""

import pytest
import torch

import conv_oracle as co

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)


def _env(monkeypatch, case):
    monkeypatch.setenv("MPI4DL_PW_BLASLT", "1" if case.blaslt else "0")
    monkeypatch.delenv("MPI4DL_PW_FAT256", raising=False)


@gpu
@requires_gpu
@pytest.mark.parametrize("cid", [c.id for c in co.CASES])
def test_conv_exact(cid, monkeypatch):
    case = co.CASE_BY_ID[cid]
    _env(monkeypatch, case)
    assert co.expected_path(case) == case.path
    kernels = []
    results = co.run_gpu(case, kernels)
    # the bindings that ran, named by the extension from their own
    # arguments, are the ones the label names (ConvFn.backward computes
    # gw before gx; the hipBLASLt branches call no binding)
    y, gx, gw = (case.path.split("+") + ["", ""])[:3]
    order = [y, gw, gx] if case.entry == "autograd" else [y]
    named = [k.split(":", 1)[-1] if k[:3] in ("zs:", "sub") else k
             for k in order if k and not k.startswith("blaslt:")]
    assert kernels == named, (kernels, named)
    worst = co.check_case(case, results)
    for leg, kind in zip(co.legs(case), case.path.split("+") + ["sum"]):
        print(f"ORACLE {case.id} {leg} {kind} {worst[leg]:.3g}")


@gpu
@requires_gpu
@pytest.mark.parametrize("family", list(co.DETERMINISM_IDS))
def test_conv_bit_deterministic(family, monkeypatch):
    """Two runs of the same case give bit-identical y and gx (activation
    checkpointing recomputes the forward and relies on it). gw is
    accumulated with fp32 atomicAdd across blocks, so its summation
    order varies between runs: it is held to the bound by
    ``test_conv_exact`` and not asserted bit-equal here."""
    case = co.CASE_BY_ID[co.DETERMINISM_IDS[family]]
    _env(monkeypatch, case)
    first, second = co.run_gpu(case), co.run_gpu(case)
    compared = [leg for leg in ("y", "gx") if leg in first]
    assert compared
    for leg in compared:
        assert torch.equal(first[leg], second[leg]), (family, leg)
