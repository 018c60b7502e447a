"""Conversation snapshots on the GPU (include/minigpt4_amd.h: the format and the rules).
1. kernels alone, through minigpt4_amd_test_kv_pack / _unpack: the packed block is the NumPy slice bit for bit (random fp16 bit patterns, NaN patterns included), the
   checksum is NumPy's uint32 view summed in uint64, unpack touches only its rows; the real row width; the launchers' refusals;
2. engine: a saved conversation, restored into the same slot, another slot, a fresh context (file pair) and in parity mode, continues with the SAME logits rows and ids as
   the uninterrupted one (np.array_equal); penalties and bias come back; a restored and an untouched conversation step together; every refusal leaves the conversation
   untouched; a corrupted block is the one failure that resets it; a context that never uses the feature counts nothing."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK_ROWS = 16                              # tiny models: 2 layers x 256 -> 2048 bytes per row; 45 rows = blocks of 16, 16, 13
ROW_BYTES = 4 * 2 * 256


# ------------------------------------------------------------------------------------------------ kernels alone
def _caches(seed, L, C, E):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1 << 16, size=(L, C, E), dtype=np.uint16)
    v = rng.integers(0, 1 << 16, size=(L, C, E), dtype=np.uint16)
    for a in (k, v):                         # NaN and infinity patterns in every row range the tests take: the copy is bitwise
        a[:, :, 0] = 0x7E00
        a[:, :, 1] = 0xFFFF
        a[:, :, 2] = 0xFC00
        a[:, :, 3] = 0x7C01
    return k, v


def _sum32(block):
    return int(np.ascontiguousarray(block).view(np.uint32).astype(np.uint64).sum(dtype=np.uint64))


@pytest.fixture(scope="module")
def small_caches():
    return _caches(11, 3, 40, 64)


@pytest.mark.parametrize("r0,n", [(0, 1), (0, 7), (5, 8), (3, 9), (0, 40), (39, 1)])
def test_pack_is_the_slice_and_unpack_touches_only_its_rows(gpu_lib, small_caches, r0, n):
    k, v = small_caches
    want = np.stack([k[:, r0:r0 + n, :], v[:, r0:r0 + n, :]])                  # [tensor][layer][row][E]
    blk, s, _ = gpu_lib.amd_test_kv_pack(k, v, r0, n)
    assert blk.shape == want.shape and np.array_equal(blk, want)
    assert s == _sum32(want)
    zk, zv, s2, _ = gpu_lib.amd_test_kv_unpack(want, np.zeros_like(k), np.zeros_like(v), r0)
    assert s2 == s
    ek, ev = np.zeros_like(k), np.zeros_like(v)
    ek[:, r0:r0 + n, :] = k[:, r0:r0 + n, :]
    ev[:, r0:r0 + n, :] = v[:, r0:r0 + n, :]
    assert np.array_equal(zk, ek) and np.array_equal(zv, ev)
    # into a cache that holds other data: every other row keeps its bits
    ok, ov = _caches(12, *k.shape)
    gk, gv, _, _ = gpu_lib.amd_test_kv_unpack(want, ok, ov, r0)
    ok[:, r0:r0 + n, :] = k[:, r0:r0 + n, :]
    ov[:, r0:r0 + n, :] = v[:, r0:r0 + n, :]
    assert np.array_equal(gk, ok) and np.array_equal(gv, ov)


def test_pack_unpack_at_the_real_row_width(gpu_lib):
    k, v = _caches(13, 2, 5, 5120)                                             # 13B rows: 640 pieces each, 3 rows x 2 layers x 2 tensors = 7680 pieces, 8 workgroups
    want = np.stack([k[:, 1:4, :], v[:, 1:4, :]])
    blk, s, _ = gpu_lib.amd_test_kv_pack(k, v, 1, 3)
    assert np.array_equal(blk, want) and s == _sum32(want)
    zk, zv, s2, _ = gpu_lib.amd_test_kv_unpack(want, np.zeros_like(k), np.zeros_like(v), 1)
    assert s2 == s and np.array_equal(zk[:, 1:4], k[:, 1:4]) and not zk[:, 0].any() and not zk[:, 4].any() and np.array_equal(zv[:, 1:4], v[:, 1:4]) and not zv[:, 4].any()


def test_kernel_launchers_refuse_bad_shapes(gpu_lib, small_caches):
    k, v = small_caches
    with pytest.raises(RuntimeError, match="launch_kv_pack: rows outside the cache"):
        gpu_lib.amd_test_kv_pack(k, v, 35, 6)
    with pytest.raises(RuntimeError, match="launch_kv_pack"):
        gpu_lib.amd_test_kv_pack(k, v, -1, 2)
    with pytest.raises(RuntimeError, match="launch_kv_unpack: rows outside the cache"):
        gpu_lib.amd_test_kv_unpack(np.zeros((2, 3, 2, 64), np.uint16), k, v, 39)
    with pytest.raises(RuntimeError, match="launch_kv_pack: bad shape"):
        gpu_lib.amd_test_kv_pack(k[:, :, :12], v[:, :, :12], 0, 2)             # E % 8
    blk, s, _ = gpu_lib.amd_test_kv_pack(k, v, 4, 0)                           # no row: nothing launched, the word is zeroed
    assert blk.size == 0 and s == 0


# ------------------------------------------------------------------------------------------------ engine
def _load(lib, tiny_files, wtype, n_ctx=256, n_conv=1):
    vp, llm = tiny_files
    old = os.environ.get("MINIGPT4_STATE_BLOCK_BYTES")
    os.environ["MINIGPT4_STATE_BLOCK_BYTES"] = str(BLOCK_ROWS * ROW_BYTES)     # read by the load
    try:
        ctx = lib.minigpt4_model_load(vp, llm(wtype), verbosity=0, n_ctx=n_ctx, n_batch=64)
    finally:
        if old is None:
            del os.environ["MINIGPT4_STATE_BLOCK_BYTES"]
        else:
            os.environ["MINIGPT4_STATE_BLOCK_BYTES"] = old
    if n_conv > 1:
        lib.amd_set_conversations(ctx, n_conv)
    return ctx


def _converse(lib, ctx, question="what is the text in the picture?", seed=7):
    """system prompt, 32 embedding rows, a question -- through the queue, like minigpt4_begin_chat_image; never a whole number of blocks"""
    lib.minigpt4_reset_chat(ctx)
    lib.minigpt4_system_prompt(ctx)
    lib.amd_eval_tokens(ctx, lib.amd_tokenize(ctx, b"Human: <Img>"))
    emb = (0.05 * np.random.default_rng(seed).standard_normal((32, lib.library.minigpt4_amd_n_embd(ctx.ptr)))).astype(np.float32)
    lib.amd_eval_embd(ctx, emb)
    lib.amd_eval_tokens(ctx, lib.amd_tokenize(ctx, b"</Img> "))
    lib.amd_eval_tokens(ctx, lib.amd_tokenize(ctx, question.encode()))
    lib.amd_eval_tokens(ctx, lib.amd_tokenize(ctx, b"### Assistant:"))
    if lib.library.minigpt4_amd_n_past(ctx.ptr) % BLOCK_ROWS == 0:
        lib.amd_eval_tokens(ctx, [5])
    assert lib.library.minigpt4_amd_n_past(ctx.ptr) >= 45


def _steps(lib, ctx, n=6):
    """n greedy minigpt4_end_chat steps: the logits row before every pick, the pieces, the ids (the history's tail)"""
    rows, pieces = [], []
    for _ in range(n):
        rows.append(lib.amd_logits(ctx).copy())
        pieces.append(lib.minigpt4_end_chat(ctx, temp=0.0))
    return rows, pieces, lib.amd_token_history(ctx)[-n:].tolist()


def _snapshot_of_now(lib, ctx, slot=0):
    """what must come back right after a load"""
    return dict(n_past=lib.library.minigpt4_amd_n_past(ctx.ptr), hist=lib.amd_token_history(ctx).copy(), logits=lib.amd_logits(ctx).copy(), top=lib.amd_top_logprobs(ctx, [slot], top_n=5))


def _assert_same_now(lib, ctx, want, slot=0):
    got = _snapshot_of_now(lib, ctx, slot)
    assert got["n_past"] == want["n_past"] and np.array_equal(got["hist"], want["hist"]) and np.array_equal(got["logits"], want["logits"])
    for key in ("top_ids", "top_logprobs"):
        assert np.array_equal(got["top"][key], want["top"][key]), key


def _assert_same_run(a, b):
    assert len(a[0]) == len(b[0]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
    assert a[1] == b[1] and a[2] == b[2]


def _kv_offset(peek, has_logits=True, n_bias=0):
    off = 64 + 4 * peek["n_rows"] + (4 * peek["n_vocab"] if has_logits else 0) + 20 + 8 * n_bias
    off = (off + 7) // 8 * 8 + 8 * -(-peek["n_rows"] // peek["block_rows"])
    return (off + 15) // 16 * 16


@pytest.mark.parametrize("wtype", ["q4_0", "q5_k"])
def test_round_trip_same_slot_other_slot_fresh_context_and_parity(gpu_lib, tiny_files, tmp_path, wtype):
    lib = gpu_lib
    ctx = _load(lib, tiny_files, wtype)
    fresh = None
    try:
        for parity in (False, True):
            lib.amd_set_parity(ctx, parity)
            _converse(lib, ctx)
            before = lib.amd_state_info(ctx)
            assert lib.amd_state_size(ctx, 0) > 0
            blob = lib.amd_state_save(ctx, 0)
            peek = lib.amd_state_peek(blob)
            n_blocks = -(-peek["n_rows"] // BLOCK_ROWS)
            assert peek["block_rows"] == BLOCK_ROWS and n_blocks >= 3 and peek["n_rows"] % BLOCK_ROWS != 0      # several blocks, the last one short
            assert peek["n_rows"] == lib.library.minigpt4_amd_n_past(ctx.ptr) and peek["flags"] == (3 if parity else 1) and len(blob) == peek["total_bytes"] == lib.amd_state_size(ctx, 0)
            assert peek["arena_hash"] == lib.amd_arena_plan(ctx)["llm_hash"]
            info = lib.amd_state_info(ctx)
            assert info["saves"] == before["saves"] + 1 and info["pack_launches"] == before["pack_launches"] + n_blocks and info["staging_bytes"] >= 4 * BLOCK_ROWS * ROW_BYTES
            at_save = _snapshot_of_now(lib, ctx)
            path = str(tmp_path / f"chat_{wtype}_{int(parity)}.mg4s")
            lib.amd_state_save_file(ctx, 0, path)
            assert open(path, "rb").read() == blob and not os.path.exists(path + ".tmp")
            want = _steps(lib, ctx)
            # the same slot
            lib.minigpt4_reset_chat(ctx)
            lib.amd_state_load(ctx, 0, blob)
            assert lib.amd_state_info(ctx)["unpack_launches"] == before["unpack_launches"] + n_blocks
            _assert_same_now(lib, ctx, at_save)
            _assert_same_run(_steps(lib, ctx), want)
            if parity:
                continue
            # a fresh context of the same files, through the file: it has never used the feature
            fresh = _load(lib, tiny_files, wtype)
            lib.minigpt4_system_prompt(fresh)
            lib.minigpt4_end_chat(fresh, temp=0.0)
            assert set(lib.amd_state_info(fresh).values()) == {0}                  # a chat alone counts and allocates nothing
            lib.amd_state_load_file(fresh, 0, path)
            _assert_same_now(lib, fresh, at_save)
            _assert_same_run(_steps(lib, fresh), want)
            lib.minigpt4_free(fresh)
            fresh = None
            # another slot, after set_conversations (the staging survives it)
            held = lib.amd_state_info(ctx)["staging_bytes"]
            lib.amd_set_conversations(ctx, 3)
            assert lib.amd_state_info(ctx)["staging_bytes"] == held
            lib.amd_state_load(ctx, 2, blob)
            lib.amd_select_conversation(ctx, 2)
            _assert_same_now(lib, ctx, at_save, slot=2)
            _assert_same_run(_steps(lib, ctx), want)
            lib.amd_select_conversation(ctx, 0)
            assert lib.library.minigpt4_amd_n_past(ctx.ptr) == 0                                      # the other conversations were not touched
            lib.amd_set_conversations(ctx, 1)
    finally:
        if fresh is not None:
            lib.minigpt4_free(fresh)
        lib.minigpt4_free(ctx)


def test_penalties_and_bias_come_back_and_a_restored_conversation_steps_in_a_batch(gpu_lib, tiny_files):
    lib = gpu_lib
    ctx = _load(lib, tiny_files, "q4_0", n_conv=3)
    try:
        # ---- restored parameters: the pick under a bias and a repetition penalty
        lib.amd_set_penalties(ctx, True)
        lib.amd_select_conversation(ctx, 0)
        _converse(lib, ctx)
        raw = int(np.argmax(lib.amd_logits(ctx)))
        lib.amd_conversation_penalties(ctx, 0, repeat_last_n=64, repeat_penalty=1.3)
        lib.amd_set_logit_bias(ctx, {raw: -np.inf, (raw + 1) % 512: 0.75})
        blob = lib.amd_state_save(ctx, 0)
        want_pick = lib.amd_end_chat_batch(ctx, [0], temp=0.0)[0]
        want_id = int(lib.amd_token_history(ctx)[-1])
        assert want_id != raw
        lib.amd_state_load(ctx, 1, blob)                                         # slot 1 held neutral parameters and no bias
        assert lib.amd_end_chat_batch(ctx, [1], temp=0.0)[0] == want_pick
        lib.amd_select_conversation(ctx, 1)
        assert int(lib.amd_token_history(ctx)[-1]) == want_id
        lib.amd_set_penalties(ctx, False)
        for slot in (0, 1):
            lib.amd_select_conversation(ctx, slot)
            lib.amd_conversation_penalties(ctx, slot)
            lib.amd_set_logit_bias(ctx, None)

        # ---- batched step: a restored conversation next to an untouched one
        def pair():
            lib.amd_select_conversation(ctx, 0)
            _converse(lib, ctx, "what is the text in the picture?", seed=7)
            lib.amd_select_conversation(ctx, 1)
            _converse(lib, ctx, "describe the colours", seed=8)

        def batch_steps():
            out = []
            for _ in range(3):
                pieces = lib.amd_end_chat_batch(ctx, [0, 1], temp=0.0)
                for slot in (0, 1):
                    lib.amd_select_conversation(ctx, slot)
                    out.append((slot, pieces[slot], lib.amd_logits(ctx).copy()))
            return out
        pair()
        want = batch_steps()
        pair()
        blob = lib.amd_state_save(ctx, 0)
        lib.amd_select_conversation(ctx, 0)
        lib.minigpt4_reset_chat(ctx)
        lib.amd_state_load(ctx, 0, blob)
        got = batch_steps()
        assert len(got) == len(want)
        for (s1, p1, l1), (s2, p2, l2) in zip(got, want):
            assert s1 == s2 and p1 == p2 and np.array_equal(l1, l2)
    finally:
        lib.minigpt4_free(ctx)


def test_refusals_leave_the_conversation_untouched_and_a_bad_block_resets_it(gpu_lib, tiny_files):
    lib = gpu_lib
    ctx = _load(lib, tiny_files, "q4_0")
    other = small = None
    try:
        _converse(lib, ctx)
        blob = lib.amd_state_save(ctx, 0)
        lib.minigpt4_end_chat(ctx, temp=0.0)                                     # the conversation has moved on: a load that did anything would show
        now = (lib.library.minigpt4_amd_n_past(ctx.ptr), lib.amd_logits(ctx).copy())

        def untouched():
            assert lib.library.minigpt4_amd_n_past(ctx.ptr) == now[0] and np.array_equal(lib.amd_logits(ctx), now[1])
        size = lib.amd_state_size(ctx, 0)
        with pytest.raises(RuntimeError, match="state_save: the buffer holds") as e:
            lib.amd_state_save(ctx, 0, cap=size - 1)
        assert e.value.needed == size
        untouched()
        with pytest.raises(RuntimeError, match="state_load: total size"):
            lib.amd_state_load(ctx, 0, blob[:-7])
        untouched()
        flipped = bytearray(blob)
        flipped[20] ^= 0x10                                                      # n_embd
        with pytest.raises(RuntimeError, match="state_load: "):
            lib.amd_state_load(ctx, 0, bytes(flipped))
        untouched()
        flipped = bytearray(blob)
        flipped[0] ^= 0x01
        with pytest.raises(RuntimeError, match="state_load: wrong magic"):
            lib.amd_state_load(ctx, 0, bytes(flipped))
        untouched()
        for slot in (-1, 1, 64):
            with pytest.raises(RuntimeError, match="state_load: conversation index out of range"):
                lib.amd_state_load(ctx, slot, blob)
            with pytest.raises(RuntimeError, match="state_save: conversation index out of range"):
                lib.amd_state_save(ctx, slot, cap=len(blob))
        untouched()
        # the q5_k file's snapshot offered to the q4_0 context: same shape, another arena layout
        other = _load(lib, tiny_files, "q5_k")
        _converse(lib, other)
        with pytest.raises(RuntimeError, match="state_load: .*arena hash"):
            lib.amd_state_load(ctx, 0, lib.amd_state_save(other, 0))
        untouched()
        lib.minigpt4_free(other)
        other = None
        # 200 rows offered to a context of 128
        lib.minigpt4_reset_chat(ctx)
        lib.amd_eval_tokens(ctx, [1] + [3 + (i * 7) % 500 for i in range(199)])
        long_blob = lib.amd_state_save(ctx, 0)
        assert lib.amd_state_peek(long_blob)["n_rows"] == 200
        small = _load(lib, tiny_files, "q4_0", n_ctx=128)
        lib.minigpt4_system_prompt(small)
        lib.minigpt4_end_chat(small, temp=0.0)
        s_now = (lib.library.minigpt4_amd_n_past(small.ptr), lib.amd_logits(small).copy())
        with pytest.raises(RuntimeError, match="state_load: n_rows 200 exceeds n_ctx 128"):
            lib.amd_state_load(small, 0, long_blob)
        assert lib.library.minigpt4_amd_n_past(small.ptr) == s_now[0] and np.array_equal(lib.amd_logits(small), s_now[1])
        assert set(lib.amd_state_info(small).values()) == {0}                    # refused before anything was allocated
        # ---- a byte flipped inside the second KV block: the one failure that is not "nothing changed"
        peek = lib.amd_state_peek(blob)
        bad = bytearray(blob)
        bad[_kv_offset(peek) + BLOCK_ROWS * ROW_BYTES + 3] ^= 0x40
        lib.amd_state_load(ctx, 0, blob)                                         # something to lose
        assert lib.library.minigpt4_amd_n_past(ctx.ptr) == peek["n_rows"]
        with pytest.raises(RuntimeError, match="state_load: block 1 checksum"):
            lib.amd_state_load(ctx, 0, bytes(bad))
        assert lib.library.minigpt4_amd_n_past(ctx.ptr) == 0
        assert (lib.amd_top_logprobs(ctx, [0], top_n=3)["top_ids"] == -1).all()  # no logits: as minigpt4_reset_chat leaves it
        assert lib.amd_state_info(ctx)["checksum_failures"] == 1
        lib.amd_state_load(ctx, 0, blob)                                         # and the slot is usable again
        assert lib.library.minigpt4_amd_n_past(ctx.ptr) == peek["n_rows"]
    finally:
        for c in (other, small):
            if c is not None:
                lib.minigpt4_free(c)
        lib.minigpt4_free(ctx)
