"""CPU-tier guard of the computed exp / SiLU / GELU forms of fast mode (csrc/activations.hpp), no GPU: the device FORMULAS evaluated in numpy fp32 -- every operation rounded to
fp32 as the kernels' (-ffp-contract=off), the exponential taken in float64 and rounded to fp32 -- over every finite fp16 argument, against the oracle's tables, under the same two
conditions tests/test_gpu_activations.py asserts on the device (activation_ref.py: within one fp16 ulp everywhere, at most 63 of 63 488 arguments different).  A formula that
cannot meet the contract with a correctly rounded exponential will not meet it with v_exp_f32 either; this keeps it honest on machines without a GPU.

It is also the one check of oracle/refcpu.c's tables that does not go through the oracle: an independent numpy evaluation of ggml's formulas (float64 tanh / exp rounded to fp32
standing in for libm's tanhf / expf)."""
import numpy as np
import pytest

import activation_ref as AR


def _table(which):
    import refcpu as R
    return R.table(which)


@pytest.mark.parametrize("which", [AR.GELU, AR.SILU, AR.EXP], ids=lambda w: AR.NAMES[w])
def test_device_formula_meets_the_contract_against_the_oracle_table(which):
    table = _table(which)
    AR.assert_table_sanity(which, table)
    dev = AR.assert_computed_contract(which, AR.evaluate(AR.DEVICE_MODEL[which]), table)
    AR.record("cpu_model_of_device_formula", AR.NAMES[which], dev)


@pytest.mark.parametrize("which", [AR.GELU, AR.SILU, AR.EXP], ids=lambda w: AR.NAMES[w])
def test_oracle_table_against_independent_evaluation_of_ggml_formula(which):
    """With a correctly rounded libm the tables equal this evaluation in every entry; another glibc's expf / tanhf need not be correctly rounded, hence the device contract's two
    conditions rather than equality."""
    table = _table(which)
    dev = AR.assert_computed_contract(which, AR.evaluate(AR.GGML_MODEL[which]), table)
    AR.record("oracle_table_vs_numpy_ggml_formula", AR.NAMES[which], dev)


def test_one_sided_gelu_fails_the_contract():
    """The check has teeth: tanh(u) = 1 - 2 / (exp(2 u) + 1) for either sign -- the form the vision GEMMs shipped with -- loses the low bits of a small exponential in
    exp(2 u) + 1 for u < 0, and 1 + th then cancels: hundreds of arguments in [-5.2, -0.35] off by up to 5 fp16 ulp.  Both conditions must reject it."""
    table = _table(AR.GELU)
    dev = AR.deviation(AR.evaluate(AR.device_gelu_one_sided), table)
    print("one-sided GELU:", dev["count"], "arguments differ, max", dev["max_ulp"], "ulp")
    AR.record("cpu_model_of_device_formula", "gelu_one_sided_before_the_fix", {k: dev[k] for k in ("count", "max_ulp", "nan_mismatches")})
    assert dev["max_ulp"] > AR.MAX_ULP and dev["count"] > AR.MAX_DIFFERENT
    with pytest.raises(AssertionError):
        AR.assert_computed_contract(AR.GELU, AR.evaluate(AR.device_gelu_one_sided), table)
    x = AR.ARGS[AR.FINITE & (AR.evaluate(AR.device_gelu_one_sided) != table)].astype(np.float32)
    assert x.max() < 0 and x.min() > -5.5                                       # the negative tail only
