"""The value-column split of the decode attention (csrc/llm_kernels.hip: VS workgroups per (head, row), each with its own hd / VS output dims; MINIGPT4_ATTN_VS).
Every fp32 chain is the one of the plain launch, so the claim is identity: `out` and both caches of a launch with VS = 2 / 4 equal those of VS = 1 bit for bit, for
the one-row, the batched and the verify form, with table and computed exponentials; only split 0 appends; and a decode run gives the same ids and logits whatever VS."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_HEAD, N_CTX = 3, 1024                                 # an odd head count catches head indexing
# cached keys: only the own key / one cached key / the partition boundary P = 32 (hd 128) / the end of the NPRE x P = 512-key prefetch and the first steady round /
# a ragged steady round.  hd 64 (P = 64) and hd 32 (P = 128) prefetch 1024 / 2048 keys: they take the steady loop at none of these, hd 128 at the last four
# (tests/test_gpu_attn_kernels.py takes every head size through its own steady loop, VS = 1, against a float64 reference: contexts of 1664 / 3200 rows).
N_PAST = (0, 1, 31, 32, 33, 511, 512, 513, 777)
HD_VS = [(128, 2), (128, 4), (64, 2), (64, 4), (32, 2), (32, 4)]   # hd 32, VS 4: one 8-dim chunk per workgroup
_INPUTS, _REF = {}, {}


def _inputs(hd, rows, n_slot):
    """Random fp32 q / k / v rows and fp16 caches (as bit patterns) from a fixed seed; made once, read-only."""
    key = (hd, rows, n_slot)
    if key not in _INPUTS:
        E = N_HEAD * hd
        rng = np.random.default_rng(7000 + 10 * hd + rows)
        arrs = [rng.standard_normal((rows, E)).astype(np.float32) for _ in range(3)]
        arrs += [rng.standard_normal((n_slot, N_CTX, E)).astype(np.float16).view(np.uint16) for _ in range(2)]
        for a in arrs:
            a.setflags(write=False)
        _INPUTS[key] = tuple(arrs)
    return _INPUTS[key]


def _launch(lib, form, vs, hd, row_slot, n_past, computed):
    """(out, kc, vc) of one launch; the VS = 1 result of a case is computed once and shared."""
    key = (form, vs, hd, tuple(row_slot), tuple(n_past), computed)
    if vs != 1 or key not in _REF:
        q, k, v, kc, vc = _inputs(hd, len(row_slot), len(n_past))
        res = lib.amd_test_attn_vsplit(form, vs, q, k, v, kc, vc, N_HEAD, row_slot, n_past, computed_exp=bool(computed))
        if vs != 1:
            return res
        for a in res:
            a.setflags(write=False)
        _REF[key] = res
    return _REF[key]


def _check(lib, form, vs, hd, row_slot, n_past, computed, written):
    """written: [(slot, first row, rows)] -- the cache rows the launch appends."""
    tag = (form, vs, hd, tuple(row_slot), tuple(n_past), computed)
    ref = _launch(lib, form, 1, hd, row_slot, n_past, computed)
    got = _launch(lib, form, vs, hd, row_slot, n_past, computed)
    assert np.isfinite(ref[0]).all() and np.abs(ref[0]).max() > 0, tag
    assert np.array_equal(got[0], ref[0]), (tag, float(np.abs(got[0] - ref[0]).max()))
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), tag
    # the append: the appended rows changed in every head, nothing else did
    _, _, _, kc, vc = _inputs(hd, len(row_slot), len(n_past))
    for new, old in ((got[1], kc), (got[2], vc)):
        untouched = np.ones(old.shape[:2], bool)
        for slot, r0, n in written:
            untouched[slot, r0:r0 + n] = False
            per_head = (new[slot, r0:r0 + n] != old[slot, r0:r0 + n]).reshape(n, N_HEAD, hd).any(axis=2)
            assert per_head.all(), (tag, slot, r0)
        assert np.array_equal(new[untouched], old[untouched]), tag


@pytest.mark.parametrize("computed", [0, 1])
@pytest.mark.parametrize("hd,vs", HD_VS)
def test_one_row_launch_is_bit_identical_to_the_unsplit_launch(gpu_lib, hd, vs, computed):
    for n_past in N_PAST:
        _check(gpu_lib, 0, vs, hd, [0], [n_past], computed, [(0, n_past, 1)])


@pytest.mark.parametrize("computed", [0, 1])
@pytest.mark.parametrize("hd,vs", HD_VS)
def test_batched_launch_is_bit_identical_to_the_unsplit_launch(gpu_lib, hd, vs, computed):
    """3 rows in 3 slots at positions 0, 33 and 513 (row r is conversation row_slot[r])."""
    row_slot, n_past = [2, 0, 1], [33, 513, 0]
    _check(gpu_lib, 1, vs, hd, row_slot, n_past, computed, [(s, n_past[s], 1) for s in row_slot])


@pytest.mark.parametrize("computed", [0, 1])
@pytest.mark.parametrize("hd,vs", HD_VS)
def test_verify_launch_is_bit_identical_to_the_unsplit_launch(gpu_lib, hd, vs, computed):
    """R = 8 rows from p0: the keys taken from LDS lie before (0, 27), across (505) and behind (512) the 512 keys hd 128 prefetches."""
    for p0 in (0, 27, 505, 512):
        _check(gpu_lib, 2, vs, hd, [1] * 8, [0, p0], computed, [(1, p0, 8)])


def test_unsupported_splits_are_refused_before_a_device_is_touched(gpu_lib):
    q, k, v, kc, vc = _inputs(64, 1, 1)
    for vs in (0, 3, 8):
        with pytest.raises(RuntimeError, match="rc=1"):
            gpu_lib.amd_test_attn_vsplit(0, vs, q, k, v, kc, vc, N_HEAD, [0], [5])


def test_decode_run_is_bit_identical_for_every_split(gpu_lib, tmpdir_models):
    """A tiny Q5_K_M model, a 30-row prompt, 40 greedy steps with MINIGPT4_ATTN_VS = 1, 2 and 4 (read per engine): the same ids and the same logits at every step."""
    from minigpt4_cpp_amd import modelgen as G
    vp, lp = os.path.join(tmpdir_models, "vision_tiny_vsplit.bin"), os.path.join(tmpdir_models, "llm_vsplit_q5km.bin")
    G.write_vision_file(vp, G.tiny_vision(n_embd_llm=4096), seed=3, std=0.05)
    G.write_llm_file(lp, G.tiny_llm(wtype="q5_k", n_embd=256, n_layer=2, n_head=4, n_vocab=512, mix="q5_k_m"), seed=1, std=0.05)
    toks = [1] + [int(t) for t in np.random.default_rng(31).integers(3, 512, 29)]
    runs = {}
    for vs in ("1", "2", "4"):
        os.environ["MINIGPT4_ATTN_VS"] = vs
        try:
            ctx = gpu_lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=128, n_batch=32)
        finally:
            os.environ.pop("MINIGPT4_ATTN_VS", None)
        try:
            gpu_lib.amd_eval_tokens(ctx, toks)
            got = gpu_lib.amd_logits(ctx).copy()
            ids, lg = [], [got]
            for _ in range(40):
                ids.append(int(got.argmax()))
                gpu_lib.amd_eval_tokens(ctx, [ids[-1]])
                got = gpu_lib.amd_logits(ctx).copy()
                lg.append(got)
            runs[vs] = (ids, np.stack(lg))
        finally:
            gpu_lib.minigpt4_free(ctx)
    assert np.isfinite(runs["1"][1]).all()
    for vs in ("2", "4"):
        assert runs[vs][0] == runs["1"][0], vs
        assert np.array_equal(runs[vs][1], runs["1"][1]), (vs, float(np.abs(runs[vs][1] - runs["1"][1]).max()))
