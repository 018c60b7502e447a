"""The LoRA kernels (csrc/lora.hip) as the engine drives them at real shapes, through minigpt4_amd_test_lora_group: several K slabs under either form and every mode, joined
targets up to 192 rows of A, adapters of unequal width in one launch, up to four MFMA row tiles (one with nothing to do), rows mapped to conversation slots by a strided
table or slot0, the slots' factors, ldy > n_out and outputs that are ADDED to.  The cases, the float64 reference and the bound are tests/lora_ref.py's;
tests/test_cpu_lora_ref.py shows on the reference alone that a slab left out, targets confused or a slot, stride or factor misread moves these cases' outputs by more than
4 x the bound."""
import numpy as np
import pytest

import lora_ref as L

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("spec", L.SPECS, ids=L.IDS)
def test_group_against_float64(gpu_lib, spec):
    """Every output that receives a term within lora_ref.group_ref's bound of the float64 value; every other one -- rows whose slot has no adapter, targets the row's
    adapter lacks, the columns n_out .. ldy - 1 -- equal to what was there, bit for bit."""
    c = L.make_case(spec)
    want, bound, live = L.group_ref(c)
    got = gpu_lib.test_lora_group(c["x"], c["second"], c["n_out"], c["adapters"], c["slot_adapter"], c["slot_scale"], c["row_slot"], c["stride"], c["slot0"], c["y0"],
                                  c["mode"], c["form"])
    assert got.shape == c["y0"].shape and got.dtype == np.float32
    ratio = np.abs(got.astype(np.float64) - want)[live] / bound[live]
    worst = float(ratio.max(initial=0.0))
    print(f"lora group {spec['name']}: rows={c['rows']} n_in={c['n_in']} n_out={c['n_out']} live outputs={int(live.sum())} largest error / bound = {worst:.3g}")
    assert np.array_equal(got[~live].view(np.uint32), c["y0"][~live].view(np.uint32)), "an output without a term changed"
    assert worst <= 1.0, worst
