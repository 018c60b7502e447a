"""What the engine asks before it fuses a row preparation into a decode mat-vec launch (matvec_prologue_supported, matvec_silu_pair_supported, matvec_rows_prologue_ok)
against the kernel family's ranges written out here, independently of the library's dispatch table: a predicate that says yes for a shape the launcher has no kernel for
makes Engine::mul_mat_set throw in the middle of a decode step.  tests/test_gpu_matvec_dispatch.py launches the same list."""
import pytest

# type -> (elements per 16-byte unit, instantiated units per lane, K must be a multiple of)
KQ, Q32 = ("q4_k", "q5_k", "q6_k"), ("q4_0", "q4_1", "q5_0", "q5_1")
FAMILY = {**{t: (32, (1, 2, 3, 4, 5, 6, 7), 32) for t in Q32}, **{t: (32, (1, 2, 3, 4, 5, 6, 7), 256) for t in KQ}, "q8_0": (16, (1, 4, 5, 11), 32), "f16": (8, (1, 2, 8, 10), 8)}
NO_KERNEL = ("f32", "q2_k", "q3_k")                       # types the pipelined decode kernel is not built for at all


def cases(wtype):
    """The largest K of each instantiated unit count, the first K beyond the last one, a K that breaks the type's divisibility rule (marked)."""
    if wtype in NO_KERNEL:
        return [(256, True), (4096, True), (5120, True)]
    epu, units, mult = FAMILY[wtype]
    ks = [(n * 64 * epu, True) for n in units]
    ks.append((units[-1] * 64 * epu + mult, True))
    ks.append((units[1] * 64 * epu - mult // 2, False))   # inside the unit range, off the rule: 32-weight types -16, k-quants -128 (still a multiple of 32), F16 -4
    return ks


def expected(wtype, K):
    """(single-row prologue, SiLU pair epilogue, multi-row prologue)"""
    if wtype in NO_KERNEL:
        return False, False, False
    epu, units, mult = FAMILY[wtype]
    pro = K % mult == 0 and K <= units[-1] * 64 * epu
    pair = pro and wtype not in ("q8_0", "f16") and K <= 3 * 64 * 32              # pair epilogue: 1..3 units per lane
    rows = pro and wtype in ("q4_0",) + KQ and K <= 3 * 64 * 32                   # multi-row prologue: 1..3 units per lane, Q4_0 and the k-quants
    return pro, pair, rows


ALL = [(t, K) for t in list(FAMILY) + list(NO_KERNEL) for K, _ in cases(t)]


@pytest.mark.parametrize("wtype,K", ALL)
def test_prologue_predicates_state_the_instantiated_ranges(lib, wtype, K):
    from minigpt4_cpp_amd import quants as Q
    assert lib.amd_test_matvec_predicates(Q.NAME_TO_TYPE[wtype], K) == expected(wtype, K), (wtype, K)
