"""k_attn_prefill_s (csrc/attn_stream.hip), the streaming prompt attention kernel, alone against the float64 reference of tests/attn_ref.py.

The bound is attn_ref.attn_bound, unchanged.  Why the two-sweep scheme stays inside it: the scores are the family's (fp16 operands, fp32 MFMA accumulation, one multiply
by the scale) and sweep 2 repeats sweep 1's chain bit for bit, so the exponentials e_j = exp_h(s_j - m) see the arguments the bound's fragile-key term F already covers.
What differs from the contract is the normalisation: the kernel accumulates sum_j e_j v_jd in fp32 and multiplies once by fp32(1 / tot), i.e. it uses p'_j = e_j / tot
where the reference uses p_j = fp16(fp32(e_j) fp32(1 / tot)).  For a normal fp16 p_j that is half an fp16 ulp, |p'_j - p_j| <= 2^-11 p_j; for a subnormal one
|p'_j - p_j| <= 2^-25, over T keys at most T 2^-25 |v| -- 2^-13 |v| at 4096 keys, where sum_j p_j = 1 makes the bound's first term about 2^-10 |v|.  The inverse and the
final multiply add 2 x 2^-24 relative.  Together under 2^-11 + 2^-13 + 2^-23 < 2^-10 of scale_d, the bound's probability term, for every context up to 8192 keys; the fp32
accumulation term is the family's.  A numpy float32 / float16 emulation of the scheme with random accumulation orders stayed below 0.49 of the bound on these cases.
Largest |got - ref| / bound observed on an MI355X: see the README row of the kernel."""
import numpy as np
import pytest

import attn_ref as A

pytestmark = pytest.mark.gpu

H = A.N_HEAD
# the kernel's query tile is 64 rows, 16 per wave: N at its edges (65 is in the list already) and three tiles
TILE_EDGE_CASES = [(hd, pos0, N) for hd in A.HDS for pos0 in (0, 100) for N in (63, 64)] + [(hd, 1, 129) for hd in A.HDS]
# (hd, n_ctx, pos0, N): the last key just past what the LDS-row forms serve (1984 / 2240 / 2368 keys)
PAST_LIMIT_CASES = [(128, 2112, 1990, 33), (64, 2368, 2250, 33), (32, 2496, 2380, 33)]


@pytest.mark.parametrize("key", A.PROMPT_CASES + TILE_EDGE_CASES, ids=lambda k: f"hd{k[0]}-p{k[1]}-N{k[2]}")
def test_streaming_form_within_bound(gpu_lib, key):
    """Form 5 on the prompt kernels' cases: N at the edges of the query tiles, first positions at the 64-key tile edge, a needle at pos0 + N that no query may see."""
    case, ref = A.prompt_case_of(*key), A.expected_of(A.prompt_case_of, *key)
    hd, pos0, N = key
    out_seg, out_ref, one = gpu_lib.amd_test_attn_prefill_seg(case["kc"], case["vc"], H, [(0, N, pos0)], case["q"], 5)
    assert not one                                               # there is no segmented streaming launch: both sides ran k_attn_prefill_s per segment
    for got in (out_ref, out_seg):
        r = A.ratio(got, ref["out"], ref["bound"])
        print(f"k_attn_prefill_s {key}: {r:.4f}")
        assert r <= 1.0, (key, r)


@pytest.mark.parametrize("hd,n_ctx,pos0,N", PAST_LIMIT_CASES, ids=lambda v: str(v))
def test_launcher_serves_a_chunk_past_the_lds_row_forms(gpu_lib, hd, n_ctx, pos0, N):
    """Form 0, the launcher's own choice: the chunk is served (the hook's rc is 0, not 4) and lies within the bound.  The needles' gain grows with the logarithm of
    the key count, as attn_ref.split_case's does."""
    gain = 4.0 + float(np.log((pos0 + N) / 1024.0))
    case = A.prompt_case(hd, H, n_ctx, pos0, N, 600000 + hd, gain=gain)
    ref = A.expected(case)
    out_seg, out_ref, _ = gpu_lib.amd_test_attn_prefill_seg(case["kc"], case["vc"], H, [(0, N, pos0)], case["q"], 0)
    for got in (out_ref, out_seg):
        r = A.ratio(got, ref["out"], ref["bound"])
        print(f"launcher past the limit hd{hd} p{pos0} N{N}: {r:.4f}")
        assert r <= 1.0, (hd, r)
