"""Host checks of tests/nonfinite_ref.py: the plants land where their names say, the two rules reject what they must, and every
op-level case is non-vacuous -- its fp64 reference, run here on the CPU, has a non-finite element for every (operand, plant, kind)
and, unless the op spreads a poison over a BatchNorm channel or a scalar loss, a finite one too.  A case that fails is replaced in
nonfinite_ref.CASES, not skipped."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import nonfinite_ref as R  # noqa: E402


def test_plants_land_where_their_names_say():
    t = torch.zeros(3, 20, 9, 7)
    for name, idx in R.PLANTS["act"](tuple(t.shape)).items():
        p = R.plant(t, "nan", ("act", name))
        assert torch.isnan(p).sum() == 1 and math.isnan(p[idx].item()), name
        assert not torch.isnan(t).any()                                   # a copy: the operand is shared between cases
    pos = R.PLANTS["act"]((3, 20, 9, 7))
    assert pos["corner"] == (0, 0, 0, 0) and pos["last_channel"][1] == 19 and pos["last_row"][2] == 8 and pos["last_col"][3] == 6
    assert pos["last_tile"] == (2, 19, 8, 6) and 0 < pos["interior"][2] < 8 and 0 < pos["interior"][3] < 6
    assert R.PLANTS["weight"]((64, 32, 3, 3))["last_channel"] == (63, 31, 1, 1)      # centre tap
    assert R.PLANTS["weight"]((1, 8, 1, 1))["last_channel"] == (0, 7, 0, 0)
    assert R.plant(torch.zeros(4), "+inf", ("vec", "last_channel"))[3] == float("inf")
    assert R.plant(torch.zeros(4), "-inf", ("vec", "corner"))[0] == float("-inf")
    assert R.PLANTS["mat"]((3, 16, 512))["last_tile"] == (2, 15, 511)


def test_mask_rule():
    nan, inf = float("nan"), float("inf")
    ref = torch.tensor([1.0, nan, inf, -inf, 0.0], dtype=torch.float64)
    assert R.masks_agree(torch.tensor([2.0, nan, inf, -inf, 0.0]), ref)[0]
    assert R.masks_agree(torch.tensor([2.0, nan, nan, nan, 0.0]), ref)[0]             # an inf may turn into a NaN (the f16 split)
    assert not R.masks_agree(torch.tensor([2.0, 0.0, inf, -inf, 0.0]), ref)[0]        # a NaN dropped (fmaxf(NaN, 0) = 0)
    assert not R.masks_agree(torch.tensor([2.0, inf, inf, -inf, 0.0]), ref)[0]        # a NaN must stay a NaN
    assert not R.masks_agree(torch.tensor([2.0, nan, 7.0, -inf, 0.0]), ref)[0]        # an inf made finite
    assert not R.masks_agree(torch.tensor([nan, nan, inf, -inf, 0.0]), ref)[0]        # a poison that spread
    assert not R.masks_agree(torch.tensor([2.0, nan, inf, -inf]), ref)[0]             # shape
    ok, msg = R.masks_agree(torch.tensor([2.0, 0.0, inf, -inf, 0.0]), ref)
    assert "1 of 1 reference NaNs" in msg and "[1]" in msg


def test_clean_twin_rule():
    nan = float("nan")
    ref_c = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64)
    ref_p = torch.tensor([1.0, nan, 3.5, 4.0], dtype=torch.float64)                   # the plant reaches elements 1 and 2
    dev_c = torch.tensor([1.0, 2.0, 3.0, 4.0])
    assert R.untouched(ref_p, ref_c).tolist() == [True, False, False, True]
    assert R.clean_twin(torch.tensor([1.0, nan, 9.0, 4.0]), dev_c, ref_p, ref_c)[0]
    assert not R.clean_twin(torch.tensor([1.0, nan, 9.0, 4.0000005]), dev_c, ref_p, ref_c)[0]     # a neighbour moved by one ulp
    assert not R.clean_twin(torch.tensor([nan, nan, 9.0, 4.0]), dev_c, ref_p, ref_c)[0]
    assert R.clean_twin(torch.tensor([1.0, nan, 9.0, 4.0000005]), dev_c, ref_p, ref_c, tol=1e-6)[0]
    assert not R.clean_twin(torch.tensor([1.0, nan, 9.0, 4.1]), dev_c, ref_p, ref_c, tol=1e-6)[0]
    assert not R.clean_twin(torch.tensor([1.0, nan, 9.0, nan]), dev_c, ref_p, ref_c, tol=1e-6)[0]
    # -0.0 and 0.0 are different bit patterns, a NaN equals itself bit for bit
    assert not R.untouched(torch.tensor([0.0], dtype=torch.float64), torch.tensor([-0.0], dtype=torch.float64)).any()
    assert R.untouched(torch.tensor([nan], dtype=torch.float64), torch.tensor([nan], dtype=torch.float64)).all()


def test_torch_propagates_nan_where_the_kernels_must():
    """What the references rest on: torch's ReLU, max-pool, maximum, MaxPool3d fusion, clamp_min BCE and ReLU backward on a NaN."""
    nan = float("nan")
    x = torch.tensor([[[[nan, -1.0], [2.0, 3.0]]]], dtype=torch.float64)
    assert torch.isnan(torch.relu(x)[0, 0, 0, 0]) and torch.isnan(F.max_pool2d(x, 2, 2)).all()
    a, b = torch.tensor([nan, 1.0, nan]), torch.tensor([1.0, nan, nan])
    assert torch.isnan(torch.maximum(a, b)).all()
    z = F.max_pool3d(torch.stack((a, b), 0).view(1, 1, 2, 1, 3), (2, 1, 1))
    assert torch.isnan(z).all()
    assert torch.isnan(torch.clamp(torch.log(torch.tensor(nan)), min=-100.0))
    g = torch.ops.aten.threshold_backward(torch.tensor([5.0, 5.0, 5.0]), torch.tensor([nan, -1.0, 2.0]), 0.0)
    assert g.tolist() == [5.0, 0.0, 5.0]
    from oracle import egaze_oracle as O
    sd = {"fusion.weight": torch.zeros(1, 1, 1, 3, 3), "fusion.bias": torch.zeros(1), "bn.running_mean": torch.zeros(1),
          "bn.running_var": torch.ones(1), "bn.weight": torch.ones(1), "bn.bias": torch.zeros(1)}
    sd["fusion.weight"][0, 0, 0, 1, 1] = 1.0
    fs, ft = torch.tensor([nan, 1.0, 1.0, nan]).view(4, 1, 1, 1), torch.tensor([0.0, nan, 0.0, nan]).view(4, 1, 1, 1)
    fused = O.fusion_forward(sd, fs, ft, False).view(4)
    pooled = torch.relu(F.max_pool3d(torch.stack((fs, ft), dim=2), (2, 1, 1))).view(4)      # nn.MaxPool3d((2, 1, 1)), then BN (identity here) + ReLU
    assert torch.isnan(fused).tolist() == torch.isnan(pooled).tolist() == [True, True, False, True] and abs(float(fused[2]) - 1.0) < 1e-4


@pytest.mark.parametrize("name,op,where,kind", R.case_ids(), ids=["-".join((n, o, w[1], k)) for n, o, w, k in R.case_ids()])
def test_case_is_not_vacuous(name, op, where, kind):
    case = R.CASES_BY_NAME[name]
    clean = case.clean_ref()
    for k, v in clean.items():
        assert torch.isfinite(v).all(), f"the clean reference of {name}.{k} is not finite"
    ref = case.run_ref(R.poisoned_operands(case, op, where, kind))
    assert set(ref) == set(clean)
    nonfinite = sum(int((~torch.isfinite(v)).sum()) for v in ref.values())
    finite = sum(int(torch.isfinite(v).sum()) for v in ref.values())
    assert nonfinite > 0, f"{name}: the plant {op}/{where[1]}/{kind} reaches no output of the reference"
    if not case.spreads:
        assert finite > 0, f"{name}: the plant {op}/{where[1]}/{kind} floods every output"
    if kind == "nan":                            # the clean-twin rule has something to compare, or the case says why not
        reach = sum(int(R.untouched(ref[k], clean[k]).sum()) for k in ref)
        assert reach > 0 or case.spreads, f"{name}: no output element is untouched by {op}/{where[1]}"


def test_every_case_has_a_device_runner():
    import test_hip_nonfinite_ops as G
    assert set(G.RUN) == set(R.CASES_BY_NAME), set(G.RUN) ^ set(R.CASES_BY_NAME)


@pytest.mark.parametrize("name", R.SP_PLANTS)
def test_sp_step_plants_poison_the_oracle_loss(name):
    loss, sd = R.sp_oracle_poisoned(name)
    assert torch.isnan(loss), (name, loss)
    bad = [k for k, v in sd.items() if (k.endswith("running_mean") or k.endswith("running_var")) and not torch.isfinite(v).all()]
    assert bool(bad) == (name != "decoder_bias"), bad      # torch poisons the running statistics behind an encoder plant too


@pytest.mark.parametrize("T,B", [(1, 1), (3, 16)])
@pytest.mark.parametrize("name", sorted(R.AT_PLANTS))
def test_at_step_plants_poison_the_oracle_loss(name, T, B):
    assert torch.isfinite(R.at_oracle_loss(*R.at_inputs(T, B, 2)))
    assert torch.isnan(R.at_oracle_loss(*R.at_poisoned_inputs(T, B, 2, name)))


@pytest.mark.parametrize("name", sorted(R.LF_PLANTS))
def test_lf_step_plants_poison_the_oracle_loss(name):
    loss, _ = R.lf_oracle_poisoned(name)
    assert torch.isnan(loss), (name, loss)
