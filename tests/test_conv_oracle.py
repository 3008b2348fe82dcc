"""The convolution oracle checks itself (CPU, no GPU needed).

* a correct kernel, emulated as the fp32 operation on the bf16 inputs
  rounded once (or, for the two double-rounding wrapper branches,
  twice), stays within the derived bound on every leg of every case;
* kernels that are subtly wrong are rejected;
* every case's label is what production code picks (``conv_plan`` and
  the built extension's kernel-name functions; the extension builds and
  imports without a GPU), and the matrix reaches every kernel path;
* ``conv_plan`` changes route at each measured crossover, on both sides
  (literal expectations, no extension needed).
"""

import pytest
import torch

import conv_oracle as co

CASE_IDS = [c.id for c in co.CASES]


def _extension_or_skip():
    """Never skips for want of a GPU: only when the tree is not built."""
    try:
        return co.extension()
    except ImportError as e:
        pytest.skip("mpi4dl_amd._gemscore is not built: run `PYTORCH_ROCM_ARCH="
                    f"gfx950 python setup.py build_ext --inplace` ({e})")


@pytest.mark.parametrize("cid", CASE_IDS)
def test_label_matches_dispatch(cid, monkeypatch):
    ge = _extension_or_skip()
    monkeypatch.delenv("MPI4DL_PW_FAT256", raising=False)
    case = co.CASE_BY_ID[cid]
    assert co.expected_path(case, ge) == case.path


def test_every_path_is_covered():
    reached = set()
    for case in co.CASES:
        reached.update(case.path.split("+"))
    assert len(set(co.ALL_PATHS)) == len(co.ALL_PATHS)
    assert reached == set(co.ALL_PATHS), (
        sorted(reached - set(co.ALL_PATHS)),
        sorted(set(co.ALL_PATHS) - reached))


def test_determinism_cases_exist():
    for cid in co.DETERMINISM_IDS.values():
        assert cid in co.CASE_BY_ID


@pytest.mark.parametrize("cid", CASE_IDS)
def test_emulation_within_bound(cid):
    case = co.CASE_BY_ID[cid]
    inputs, _ = co.case_data(case)
    worst = co.check_case(case, co.emulate(case, *inputs))
    assert all(v <= 1.0 for v in worst.values()), worst


# --- mutants -----------------------------------------------------------------

MUTANT_IDS = [
    "autograd-3x3-c16k24",
    "autograd-1x7-c26k104",
    "autograd-7x1-c52k52",
    "autograd-7x7-c8k64",
    "autograd-c64k136",
    "autograd-3x3s2-c40k48",
]


def _truncate_to_bf16(t):
    return (t.float().contiguous().view(torch.int32) & -65536).view(
        torch.float32)


def _rejects(case, leg, got):
    (x, w, b, go), ref = co.case_data(case)
    r, A = ref[leg]
    with pytest.raises(AssertionError, match="over the bound"):
        co.assert_within(got, r, A, co.reduction_length(case, leg),
                         co.leg_is_bf16(leg),
                         co.extra_term(case, leg, r, A, b), what=leg)


@pytest.mark.parametrize("cid", MUTANT_IDS)
def test_mutants_are_rejected(cid):
    case = co.CASE_BY_ID[cid]
    (x, w, b, go), _ = co.case_data(case)
    good = co.emulate(case, x, w, b, go)

    # one weight tap zeroed
    w2 = w.clone()
    w2[:, case.C - 1, case.R - 1, case.S - 1] = 0
    _rejects(case, "y", co.emulate(case, x, w2, b, go)["y"])
    _rejects(case, "gx", co.emulate(case, x, w2, b, go)["gx"])
    # bias omitted
    _rejects(case, "y", co.emulate(case, x, w, torch.zeros_like(b), go)["y"])
    # output rolled by one column
    _rejects(case, "y", good["y"].roll(1, 3))
    _rejects(case, "gx", good["gx"].roll(1, 3))
    # one output element replaced by its neighbour
    m = good["y"].clone()
    m[0, case.K - 1, case.OH - 1, case.OW - 1] = m[
        0, case.K - 1, case.OH - 1, case.OW - 2]
    _rejects(case, "y", m)
    # one input pixel omitted from gw (a pixel the strides do reach)
    x2 = x.clone()
    x2[case.N - 1, :, (case.OH - 1) * case.sh, (case.OW - 1) * case.sw] = 0
    _rejects(case, "gw", co.emulate(case, x2, w, b, go)["gw"])
    # bf16 truncation instead of round-to-nearest on the output
    f = lambda t: None if t is None else t.float()
    y32 = co._ops(case, f(x), f(w), f(b), f(go), ("y",))["y"]
    _rejects(case, "y", _truncate_to_bf16(y32))


def test_structural_zero_must_be_exact():
    """A == 0 gives bound 0: the odd pixels of a stride-2 1x1 data
    gradient must be exact zeros."""
    case = co.CASE_BY_ID["pw_bwd_data_strided-s2-c40k40"]
    (x, w, b, go), ref = co.case_data(case)
    r, A = ref["gx"]
    assert bool((A[:, :, 1::2, :] == 0).all())
    good = co.emulate(case, x, w, b, go)["gx"]
    co.assert_within(good, r, A, case.K, True)
    bad = good.clone()
    bad[0, 0, 1, 1] = 1e-30
    with pytest.raises(AssertionError, match="err/bound inf"):
        co.assert_within(bad, r, A, case.K, True)


def test_non_finite_is_rejected():
    case = co.CASE_BY_ID["pw_fwd-c8k24"]
    (x, w, b, go), ref = co.case_data(case)
    r, A = ref["y"]
    bad = co.emulate(case, x, w, b, go)["y"].clone()
    bad[1, 2, 3, 4] = float("nan")
    with pytest.raises(AssertionError, match=r"non-finite.*\(1, 2, 3, 4\)"):
        co.assert_within(bad, r, A, case.C, True)


def test_failure_reports_location():
    case = co.CASE_BY_ID["pw_fwd-c8k24"]
    (x, w, b, go), ref = co.case_data(case)
    r, A = ref["y"]
    bad = co.emulate(case, x, w, b, go)["y"].clone()
    bad[1, 5, 2, 7] += 1.0
    with pytest.raises(AssertionError,
                       match=r"1 of \d+ elements.*worst at \(1, 5, 2, 7\)"):
        co.assert_within(bad, r, A, case.C, True)
