"""The kernel descriptors of the built library: how many dwords of leading plain kernel arguments the command processor preloads into SGPRs for the kernels of the decode
step (csrc/Makefile: PRELOAD; csrc/llm_kernels.hip, "Kernel arguments").  A struct passed by value in front of the head, or a build without the option, shows here as a
length of 0 -- the kernels would still be right, and every launch would again wait for its arguments.  Read from the code object inside libminigpt4.so with
tools/kres.py's reader; no compiler, no GPU."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mangled-name pattern -> dwords the head needs (the heads are written out above the kernels)
HEADS = [
    (r"^_ZN3mg411k_matvec_v2ILi1[2-4]ELi[1-3]ELi[12]ELi[123]ELi[01]ELb[01]EEEv", 8),     # k-quants, K <= 6144, every prologue, store / pair epilogue: row, second row, K, threads, groups, waves
    (r"^_ZN3mg416k_matvec_v2_freeILi1[2-4]ELi[1-7]E", 14),                               # planes of matrix 0, Q8_K plane, K, rows, groups, waves
    (r"^_ZN3mg412k_matvec_mixILi1[23]ELi14ELi[1-4]ELi1ELi0E", 10),                       # row, norm weight, K, threads, groups and waves of both sets
    (r"^_ZN3mg410k_attn_llmILi128ELb1ELb0ELi[124]EEEv", 13),                             # n_past, q, k, v, cos, sin, E
    (r"^_ZN3mg416k_silu_mul_quantE", 5),
    (r"^_ZN3mg410k_get_rowsE", 12),
    (r"^_ZN3mg413k_argmax_partE", 8),
    (r"^_ZN3mg414k_argmax_finalE", 6),
    (r"^_ZN3mg49k_advanceE", 8),
]


def _lengths():
    spec = importlib.util.spec_from_file_location("mg4_kres", os.path.join(ROOT, "tools", "kres.py"))
    kres = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kres)
    so = os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4.so")
    if not os.path.exists(so):
        pytest.skip("libminigpt4.so is not built")
    try:
        pre = kres.preload_lengths(so)
    except Exception as e:      # a bundle layout this reader does not know
        pytest.skip(f"the code object cannot be read: {e}")
    if not pre:
        pytest.skip("no gfx950 code object found in libminigpt4.so")
    return pre


@pytest.mark.parametrize("pattern,dwords", HEADS, ids=[re.sub(r"\W+", "_", p)[:40] for p, _ in HEADS])
def test_decode_kernels_preload_their_argument_heads(pattern, dwords):
    pre = _lengths()
    hit = {n: v for n, v in pre.items() if re.search(pattern, n)}
    assert hit, pattern
    short = {n: v for n, v in hit.items() if v < dwords}
    assert not short, (dwords, sorted(short.items())[:4])
