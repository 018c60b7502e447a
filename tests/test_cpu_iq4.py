"""IQ4_NL / IQ4_XS on the host: quants.py against the bit-field decoder of tests/test_gpu_iq4.py, the exact Q8_0 image, and the CPU oracle on such a twin."""
import os

import numpy as np
import pytest
from test_gpu_iq4 import NAMES, decode_iq4

both = pytest.mark.parametrize("t", sorted(NAMES), ids=lambda t: NAMES[t])


@both
@pytest.mark.parametrize("d_bits", [None, 5])
def test_quantiser_roundtrip_and_q8_0_image(t, d_bits):
    from minigpt4_cpp_amd import quants as Q
    x = (np.random.default_rng(t).standard_normal(16 * 1024) * 0.05).astype(np.float32)
    x[512:768] = 0.0                                               # an all-zero super-block: d = 0
    buf = Q.quantize(t, x, d_bits=d_bits)
    y = Q.dequantize(t, buf, x.size)
    assert np.array_equal(y, decode_iq4(t, buf, x.size))
    assert np.sqrt(np.mean((y - x) ** 2)) < 0.1 * x.std()         # a 4-bit code: ~8 % rms
    if d_bits == 5:                                                # d * (ls - 32): 5 + 6 bits, an fp16 number -> the image decodes to exactly the same values
        assert np.array_equal(Q.dequantize_q8_0(Q.iq4_to_q8_0(buf, t, x.size), x.size), y)


@both
def test_oracle_evaluates_the_q8_0_twin(tmp_path, t):
    import refcpu as R
    from minigpt4_cpp_amd import modelgen as G, quants as Q
    src, twin = os.path.join(tmp_path, "m.bin"), os.path.join(tmp_path, "m.q8_0.bin")
    G.write_llm_file(src, G.tiny_llm(wtype=NAMES[t], n_embd=256, n_layer=1, n_head=4, n_vocab=512), seed=1, std=0.05, d_bits=5, **G.TINY_CONDITIONED)
    G.write_q8_0_twin(src, twin)
    f, g = G.read_llm_file(src), G.read_llm_file(twin)
    assert (f.tensors["layers.0.attention.wq.weight"].gtype, g.tensors["layers.0.attention.wq.weight"].gtype) == (t, Q.GGML_Q8_0)
    for name in f.tensors:
        assert np.array_equal(f.f64(name), g.f64(name)), name
    logits = R.OracleLLM(g, n_ctx=16).eval_tokens([1, 5, 300])
    assert logits.shape == (512,) and np.isfinite(logits).all() and np.ptp(logits) > 0
