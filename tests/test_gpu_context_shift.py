"""Context shift (include/minigpt4_amd.h: minigpt4_amd_shift_context / minigpt4_amd_set_context_shift): a conversation outlives n_ctx the way llama.cpp's do.
Rows [n_keep, n_keep + n_discard) are dropped, the rows above slide down in place and their cached keys are re-rotated by -n_discard positions.

1. the kernel (launch_kv_shift through minigpt4_amd_test_kv_shift) against numpy on random fp16 caches, every overlap case;
2. whole model against tests/f64ref.LlamaF64 with the same rows dropped and the kept keys rotated, fast and parity mode, tolerance calibrated on the same model's unshifted
   run, and a negative control (rows dropped WITHOUT the re-rotation) that must miss by >= 10 x that tolerance;
3. a shift that takes a long conversation back below the key-split attention threshold (the decode graph is re-captured);
4. a shift inside a batch of conversations (the others bit-identical to an untouched twin context);
5. / 6. the automatic policy through the reference ABI, and the default (off) behaviour and argument checks.

The whole-model tests use the tiny conditioned model with qk_scale (modelgen.write_llm_file): sharper attention, so that the positions of the cached keys decide the
logits.  With TINY_CONDITIONED alone the token embeddings dominate the residual stream -- dropping the rows without re-rotating the keys moves the f64 logits by only
~5e-3 of their range, less than the Q5_K model's own GPU-vs-f64 noise, and the negative control would show nothing.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHIFT_MODEL = dict(resid_scale=0.5, tok_std=1.0, output_tie=0.4, qk_scale=3.0)


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def shift_model(tmpdir_models):
    from minigpt4_cpp_amd import modelgen as G
    made = {}

    def get(wtype):
        if wtype not in made:
            p = os.path.join(tmpdir_models, f"llm_shift_{wtype}.bin")
            G.write_llm_file(p, G.tiny_llm(wtype=wtype, n_embd=256, n_layer=2, n_head=4, n_vocab=512), seed=1, std=0.05, **SHIFT_MODEL)
            made[wtype] = p
        return made[wtype]
    return get


# ------------------------------------------------------------------------------------------------ 1. the kernel
def rope_row_f32(hd, pos):
    """cos / sin of table row `pos` as the engine builds it: ggml's iterative fp32 theta (theta = pos; theta *= theta_scale per pair), cosf / sinf / powf of the C
    library the engine's host code calls (numpy's own float32 cos can differ from it by an ulp, which moves a rotated key whose two terms cancel by more than
    an fp16 ulp)."""
    import ctypes
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    for fn in (libm.cosf, libm.sinf):
        fn.argtypes, fn.restype = [ctypes.c_float], ctypes.c_float
    libm.powf.argtypes, libm.powf.restype = [ctypes.c_float, ctypes.c_float], ctypes.c_float
    theta_scale = np.float32(libm.powf(10000.0, float(np.float32(-2.0) / np.float32(hd))))
    c, s = np.empty(hd // 2, np.float32), np.empty(hd // 2, np.float32)
    theta = np.float32(pos)
    for i in range(hd // 2):
        c[i], s[i] = libm.cosf(float(theta)), libm.sinf(float(theta))
        theta = np.float32(theta * theta_scale)
    return c, s


def check_shift(lib, k, v, n_head, n_rows, keep, d):
    L, C, E = k.shape
    hd = E // n_head
    gk, gv, _ = lib.amd_test_kv_shift(k, v, n_head, n_rows, keep, d)
    ku, kv_, gku, gvu = k.view(np.uint16), v.view(np.uint16), gk.view(np.uint16), gv.view(np.uint16)
    m = max(n_rows - keep - d, 0) if d > 0 else 0            # rows that move
    assert np.array_equal(gku[:, :keep], ku[:, :keep]) and np.array_equal(gvu[:, :keep], kv_[:, :keep])   # below n_keep: untouched
    top = keep + m if m else 0
    hi = max(top, n_rows if m else 0)
    if not m:                                                # nothing moves: nothing is written
        assert np.array_equal(gku, ku) and np.array_equal(gvu, kv_)
        return
    assert np.array_equal(gku[:, hi:], ku[:, hi:]) and np.array_equal(gvu[:, hi:], kv_[:, hi:])          # at or above n_rows: never written
    assert np.array_equal(gvu[:, keep:keep + m], kv_[:, keep + d:keep + d + m])                            # V: bit for bit
    c, s = rope_row_f32(hd, d)
    c = np.tile(c.astype(np.float64), n_head)
    s = np.tile(s.astype(np.float64), n_head)
    for il in range(L):                                      # per layer: bounded host memory at the 40-layer shapes
        src = k[il, keep + d:keep + d + m].astype(np.float64).reshape(m, E // 2, 2)
        want = np.empty_like(src)
        want[..., 0] = src[..., 0] * c + src[..., 1] * s
        want[..., 1] = -src[..., 0] * s + src[..., 1] * c
        want = want.reshape(m, E)
        got = gk[il, keep:keep + m].astype(np.float64)
        ulp = np.spacing(np.abs(want).astype(np.float16)).astype(np.float64)
        bad = np.abs(got - want) > ulp
        assert not bad.any(), (il, int(bad.sum()), np.argwhere(bad)[:4])


@pytest.mark.parametrize("E,H", [(256, 4), (4096, 32), (5120, 40)])
@pytest.mark.parametrize("L,C", [(2, 2048), (40, 256)])
def test_kv_shift_kernel_matches_numpy(gpu_lib, E, H, L, C):
    rng = np.random.default_rng(E + L)
    k = rng.standard_normal((L, C, E), dtype=np.float32).astype(np.float16)
    v = rng.standard_normal((L, C, E), dtype=np.float32).astype(np.float16)
    n_rows = C - 3                                           # rows at and above n_rows must stay as they are
    for keep in (0, 1, 45):
        span = n_rows - keep
        cases = [1, 3, 8, 9, 100,
                 (2 * span) // 3,                            # the tail that moves is shorter than the discard
                 span,                                       # discard everything after keep: nothing moves
                 0]
        for d in cases:
            check_shift(gpu_lib, k, v, H, n_rows, keep, d)


# ------------------------------------------------------------------------------------------------ 2. whole model against float64
def rot_f64(x, d, n_head):
    """RoPE rotation of cached keys [T, E] by -d positions (float64, exact angles)."""
    T, E = x.shape
    hd = E // n_head
    y = x.reshape(T, n_head, hd // 2, 2).copy()
    ang = -d * 10000.0 ** (-2.0 * np.arange(hd // 2) / hd)
    c, s = np.cos(ang), np.sin(ang)
    x0, x1 = y[..., 0].copy(), y[..., 1].copy()
    y[..., 0] = x0 * c - x1 * s
    y[..., 1] = x0 * s + x1 * c
    return y.reshape(T, E)


def shift_f64(m, keep, d, rotate=True):
    for il in range(m.L):
        kept = m.k[il][keep + d:]
        m.k[il] = np.concatenate([m.k[il][:keep], rot_f64(kept, d, m.H) if rotate else kept])
        m.v[il] = np.concatenate([m.v[il][:keep], m.v[il][keep + d:]])


def f64_run(f, prefix, chunk, singles, shift=None, rotate=True):
    import f64ref as F
    m = F.LlamaF64(f)
    m.eval(tokens=prefix)
    if shift:
        shift_f64(m, *shift, rotate=rotate)
    out = [m.eval(tokens=chunk)[-1]] if len(chunk) else []
    out += [m.eval(tokens=[t])[-1] for t in singles]
    return np.array(out)


def gpu_run(lib, ctx, prefix, chunk, singles, shift=None):
    lib.minigpt4_reset_chat(ctx)
    lib.amd_eval_tokens(ctx, prefix)
    if shift:
        lib.amd_shift_context(ctx, *shift)
        assert lib.library.minigpt4_amd_n_past(ctx.ptr) == len(prefix) - shift[1]
    out = []
    if len(chunk):
        lib.amd_eval_tokens(ctx, chunk)
        out.append(lib.amd_logits(ctx))
    for t in singles:                                        # one row at a time: the captured decode step
        lib.amd_eval_tokens(ctx, [t])
        out.append(lib.amd_logits(ctx))
    return np.array(out)


def step_err(a, b):
    return max(_rel(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("parity", [False, True])
@pytest.mark.parametrize("wtype", ["f16", "q5_k"])
def test_shifted_conversation_matches_f64(gpu_lib, shift_model, vision_file, wtype, parity):
    from minigpt4_cpp_amd import modelgen as G
    lp = shift_model(wtype)
    f = G.read_llm_file(lp)
    toks = [int(t) for t in np.random.default_rng(7).integers(3, 512, 60 + 7 + 16)]
    prefix, chunk, singles = toks[:60], toks[60:67], toks[67:]
    ctx = gpu_lib.minigpt4_model_load(vision_file, lp, verbosity=0, n_ctx=256, n_batch=32)
    try:
        gpu_lib.amd_set_parity(ctx, parity)
        base = gpu_run(gpu_lib, ctx, prefix, chunk, singles)
        got = gpu_run(gpu_lib, ctx, prefix, chunk, singles, shift=(5, 20))
    finally:
        gpu_lib.minigpt4_free(ctx)
    err0 = step_err(base, f64_run(f, prefix, chunk, singles))
    tol = max(2.0 * err0, 2e-3)
    err = step_err(got, f64_run(f, prefix, chunk, singles, shift=(5, 20)))
    miss = step_err(got, f64_run(f, prefix, chunk, singles, shift=(5, 20), rotate=False))
    assert err <= tol, (err, err0, tol)
    assert miss >= 10.0 * tol, (miss, tol)                   # the check can tell a missing re-rotation


@pytest.fixture(scope="module")
def vision_file(tmpdir_models):
    from minigpt4_cpp_amd import modelgen as G
    vp = os.path.join(tmpdir_models, "vision_tiny.bin")
    if not os.path.exists(vp):
        G.write_vision_file(vp, G.tiny_vision(n_embd_llm=4096), seed=3, std=0.05)
    return vp


# ------------------------------------------------------------------------------------------------ 3. back below the key-split threshold
def test_shift_below_the_key_split_threshold_recaptures(gpu_lib, shift_model, vision_file):
    """900 rows + 3 decode steps run on the key-split attention (captured in the decode graph); a shift of 600 rows takes the conversation back below the threshold
    (768 keys): the step must be re-captured with the one-workgroup-per-head attention, and the 8 steps after the shift must match f64."""
    from minigpt4_cpp_amd import modelgen as G
    lp = shift_model("f16")
    f = G.read_llm_file(lp)
    toks = [int(t) for t in np.random.default_rng(11).integers(3, 512, 900 + 3 + 8)]
    prefix, pre_steps, post_steps = toks[:900], toks[900:903], toks[903:]
    ctx = gpu_lib.minigpt4_model_load(vision_file, lp, verbosity=0, n_ctx=1024, n_batch=512)
    try:
        base = gpu_run(gpu_lib, ctx, prefix, [], pre_steps + post_steps)[3:]
        gpu_lib.minigpt4_reset_chat(ctx)
        gpu_run(gpu_lib, ctx, prefix, [], pre_steps)
        gpu_lib.amd_shift_context(ctx, 5, 600)
        assert gpu_lib.library.minigpt4_amd_n_past(ctx.ptr) == 303
        got = np.array([(gpu_lib.amd_eval_tokens(ctx, [t]), gpu_lib.amd_logits(ctx))[1] for t in post_steps])
    finally:
        gpu_lib.minigpt4_free(ctx)
    import f64ref as F
    m = F.LlamaF64(f)
    m.eval(tokens=prefix)
    for t in pre_steps:
        m.eval(tokens=[t])
    want0 = np.array([m.eval(tokens=[t])[-1] for t in post_steps])
    m = F.LlamaF64(f)
    m.eval(tokens=prefix)
    for t in pre_steps:
        m.eval(tokens=[t])
    shift_f64(m, 5, 600)
    want = np.array([m.eval(tokens=[t])[-1] for t in post_steps])
    tol = max(2.0 * step_err(base, want0), 2e-3)
    assert step_err(got, want) <= tol, (step_err(got, want), tol)


# ------------------------------------------------------------------------------------------------ 4. one conversation of a batch
def test_shift_inside_a_batch(gpu_lib, shift_model, vision_file):
    from minigpt4_cpp_amd import modelgen as G
    lp = shift_model("f16")
    f = G.read_llm_file(lp)
    rng = np.random.default_rng(5)
    toks = [[int(t) for t in rng.integers(3, 512, 60 + 8)] for _ in range(3)]
    a = gpu_lib.minigpt4_model_load(vision_file, lp, verbosity=0, n_ctx=256, n_batch=32)
    b = gpu_lib.minigpt4_model_load(vision_file, lp, verbosity=0, n_ctx=256, n_batch=32)
    got = {c: [[] for _ in range(3)] for c in ("a", "b")}
    try:
        for ctx in (a, b):
            gpu_lib.amd_set_conversations(ctx, 3)
            for s in range(3):
                gpu_lib.amd_select_conversation(ctx, s)
                gpu_lib.amd_eval_tokens(ctx, toks[s][:60])
        gpu_lib.amd_select_conversation(a, 1)
        gpu_lib.amd_shift_context(a, 5, 20)
        for step in range(8):
            forced = [toks[s][60 + step] for s in range(3)]
            for name, ctx in (("a", a), ("b", b)):
                gpu_lib.amd_eval_batch(ctx, [0, 1, 2], forced)
                for s in range(3):
                    gpu_lib.amd_select_conversation(ctx, s)
                    got[name][s].append(gpu_lib.amd_logits(ctx))
        gpu_lib.amd_select_conversation(a, 1)
        assert gpu_lib.library.minigpt4_amd_n_past(a.ptr) == 60 - 20 + 8
    finally:
        gpu_lib.minigpt4_free(a)
        gpu_lib.minigpt4_free(b)
    for s in (0, 2):                                         # the other conversations: bit for bit what an untouched twin computes
        for step in range(8):
            assert np.array_equal(got["a"][s][step], got["b"][s][step]), (s, step)
    want0 = f64_run(f, toks[1][:60], [], toks[1][60:])
    want = f64_run(f, toks[1][:60], [], toks[1][60:], shift=(5, 20))
    tol = max(2.0 * step_err(got["b"][1], want0), 2e-3)
    assert step_err(got["a"][1], want) <= tol, (step_err(got["a"][1], want), tol)


# ------------------------------------------------------------------------------------------------ 5. / 6. the policy, the default and the arguments
def n_past(lib, ctx):
    return lib.library.minigpt4_amd_n_past(ctx.ptr)


def test_automatic_policy_through_the_reference_abi(gpu_lib, shift_model, vision_file):
    n_ctx = 128
    ctx = gpu_lib.minigpt4_model_load(vision_file, shift_model("q5_k"), verbosity=0, n_ctx=n_ctx, n_batch=64)
    try:
        gpu_lib.minigpt4_system_prompt(ctx)
        keep = n_past(gpu_lib, ctx)
        assert 0 < keep < n_ctx - 32
        gpu_lib.amd_set_context_shift(ctx, keep)
        gpu_lib.minigpt4_begin_chat(ctx, "hello")
        shifts = 0
        for _ in range(300):
            p = n_past(gpu_lib, ctx)
            gpu_lib.minigpt4_end_chat(ctx, temp=0.0)
            q = n_past(gpu_lib, ctx)
            if p + 1 > n_ctx:
                assert q == p + 1 - max(p + 1 - n_ctx, (p - keep) // 2), (p, q)
                shifts += 1
            else:
                assert q == p + 1
            assert q <= n_ctx
        assert shifts > 0
        # an add longer than n_ctx - n_keep cannot be made room for: it fails as without the policy, and nothing moves
        p = n_past(gpu_lib, ctx)
        with pytest.raises(RuntimeError):
            gpu_lib.amd_eval_tokens(ctx, [5] * (n_ctx - keep + 1))
        assert n_past(gpu_lib, ctx) == p
        # a batched step advances a full conversation
        gpu_lib.minigpt4_reset_chat(ctx)
        gpu_lib.amd_eval_tokens(ctx, [1] + [5] * (n_ctx - 1))
        gpu_lib.amd_set_context_shift(ctx, 10)
        gpu_lib.amd_end_chat_batch(ctx, [0], temp=0.0)
        assert n_past(gpu_lib, ctx) == n_ctx - (n_ctx - 10) // 2 + 1
    finally:
        gpu_lib.minigpt4_free(ctx)


def test_policy_off_by_default_and_bad_arguments(gpu_lib, shift_model, vision_file):
    n_ctx = 128
    lp = shift_model("q5_k")
    ctx = gpu_lib.minigpt4_model_load(vision_file, lp, verbosity=0, n_ctx=n_ctx, n_batch=64)
    twin = gpu_lib.minigpt4_model_load(vision_file, lp, verbosity=0, n_ctx=n_ctx, n_batch=64)
    try:
        gpu_lib.minigpt4_system_prompt(ctx)
        gpu_lib.minigpt4_begin_chat(ctx, "hello")
        for _ in range(n_ctx):
            gpu_lib.minigpt4_end_chat(ctx, temp=0.0)
            assert n_past(gpu_lib, ctx) <= n_ctx
        assert n_past(gpu_lib, ctx) == n_ctx                 # stops at a full context, as the reference does
        assert gpu_lib.library.minigpt4_begin_chat(ctx.ptr, b"hello", 0) == 8   # FailedToAddString
        assert n_past(gpu_lib, ctx) == n_ctx
        # bad arguments: 1, and nothing changes -- the next step's logits equal an untouched twin's bit for bit
        toks = [int(t) for t in np.random.default_rng(3).integers(3, 512, 50)]
        for c in (ctx, twin):
            gpu_lib.minigpt4_reset_chat(c)
            gpu_lib.amd_eval_tokens(c, toks)
        for keep, d in ((-1, 1), (0, -1), (40, 11), (51, 0)):
            assert gpu_lib.library.minigpt4_amd_shift_context(ctx.ptr, keep, d) == 1, (keep, d)
            assert gpu_lib.library.minigpt4_amd_last_error()
            assert n_past(gpu_lib, ctx) == 50
        assert gpu_lib.library.minigpt4_amd_shift_context(ctx.ptr, 50, 0) == 0          # n_discard = 0: a no-op
        assert n_past(gpu_lib, ctx) == 50
        for c in (ctx, twin):
            gpu_lib.amd_eval_tokens(c, [7])
        assert np.array_equal(gpu_lib.amd_logits(ctx), gpu_lib.amd_logits(twin))
    finally:
        gpu_lib.minigpt4_free(ctx)
        gpu_lib.minigpt4_free(twin)
