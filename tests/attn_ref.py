"""float64 references, error bounds, inputs and deliberately wrong variants for the language model's attention and RoPE / append kernels (csrc/llm_kernels.hip,
csrc/attn_llm_body.hpp), shared by tests/test_cpu_attn_ref.py (no GPU: the references, the bounds and the inputs checked against each other) and
tests/test_gpu_attn_kernels.py (each kernel alone against them).  numpy only.

The contract, from the comments above the kernels and csrc/activations.hpp:
  RoPE       ggml mode 0, interleaved pairs; theta_0 = pos, theta *= powf(10000, -2 / hd) per pair in fp32, cosf / sinf of that (rope_tables); the rotation
             x0 c - x1 s, x0 s + x1 c in fp32.  The rotated q stays fp32 in k_rope_kv* and is rounded to fp16 inside every attention kernel; the rotated k and the raw v go
             to the caches as fp16, round to nearest.
  attention  per (head, query row at position pos): keys 0 .. pos; s_j = (sum_i k_ji q_i) / sqrt(hd), operands fp16 values, accumulation fp32; m = max s_j;
             e_j = fp16(exp(fp16(s_j - m))) (ggml's table; computed exponentials are within one fp16 ulp of the entry); tot = sum e_j exact in double;
             p_j = fp16(fp32(e_j) * fp32(1 / tot)); out_d = sum_j p_j v_jd, fp32 in a kernel-specific order.

  rope_thetas_ref / rope_tables_ref / rope_angles_exact / rope_dtheta   the table, restated, and what the fp32 iteration may move an angle
  rope_ref / rope_bound / rope_f32                                      the rotation in float64, its bound, and the kernels' fp32 statements (what the attention operands are)
  attn_ref / attn_bound / attn_f32_emulated                             one (head, query): reference, bound, and an fp32 emulation in a chosen accumulation order
  expected                                                              a whole launch: out, bound, the rotated q and the appended cache rows -- or a MUTANT of them
  needle_case / pass_case / prompt_case / rope_case                     the inputs
  decode_case / verify_case / split_case / plain_case / prompt_case_of  the launch forms' assemblies: expected(...) of one gives that launch's out and appended rows.
                                                                        Fused one-row, batched (its slots), verify (row t: cache rows [0, p0), then the pass's rows
                                                                        0 .. t), key-split stepped L times and rope_kv + the plain form are all "pass" cases -- the
                                                                        same numbers by contract; the prompt kernels' q arrives rotated and every key is cached
  DECODE_CASES, VERIFY_CASES, SPLIT_CASES, PLAIN_CASES, PROMPT_CASES, ROPE_CASES   the case lists both test files use
"""
import functools

import numpy as np

F = np.float32
D = np.float64


def f16(x):
    """round to nearest fp16 (numpy converts float64 -> float16 in one rounding)"""
    return np.asarray(x).astype(np.float16)


def ulp16(x):
    """the spacing of fp16 at |x|, float64"""
    return np.spacing(np.abs(f16(x))).astype(D)


# ---- RoPE -------------------------------------------------------------------------------------------------------------------------------------------------------------
def rope_thetas_ref(n_ctx, hd):
    """ggml's iteration, restated: theta = pos; theta *= theta_scale per pair, in fp32 -> [n_ctx][hd / 2] fp32"""
    scale = F(10000.0 ** (-2.0 / hd))
    th = np.empty((n_ctx, hd // 2), F)
    theta = np.arange(n_ctx, dtype=F)
    for i in range(hd // 2):
        th[:, i] = theta
        theta = theta * scale
        assert theta.dtype == F
    return th


def rope_tables_ref(n_ctx, hd):
    """(cos, sin) [n_ctx][hd / 2] fp32: evaluated in float64 on the fp32 theta, rounded to fp32 (a correctly rounded cosf / sinf)"""
    th = rope_thetas_ref(n_ctx, hd).astype(D)
    return np.cos(th).astype(F), np.sin(th).astype(F)


def rope_angles_exact(n_ctx, hd):
    """pos * 10000 ** (-2 i / hd) in float64"""
    return np.arange(n_ctx, dtype=D)[:, None] * 10000.0 ** (-2.0 * np.arange(hd // 2) / hd)[None, :]


def rope_dtheta(pos, hd):
    """What the fp32 iteration may move the angle of pair i at position pos: theta_scale is rounded once and every multiplication rounds once, so after i steps theta is
    within i x 2^-23 relative of pos scale^i; one more 2^-23 for a cosf / sinf that is one ulp off at an angle whose derivative is at most 1.  -> [len(pos)][hd / 2]"""
    i = np.arange(hd // 2, dtype=D)
    return np.asarray(pos, D).reshape(-1, 1) * (10000.0 ** (-2.0 * i / hd) * (i + 1.0) * 2.0 ** -23)[None, :]


def _pairs(x, n_head, half_split):
    """x [N][E] -> (x0, x1) [N][n_head][hd / 2]: the interleaved pairs (2 i, 2 i + 1); half_split: (i, i + hd / 2) -- a MUTANT (the NeoX layout)"""
    N, E = x.shape
    hd = E // n_head
    if half_split:
        xr = x.reshape(N, n_head, 2, hd // 2)
        return xr[:, :, 0, :], xr[:, :, 1, :]
    xr = x.reshape(N, n_head, hd // 2, 2)
    return xr[..., 0], xr[..., 1]


def _unpairs(y0, y1, half_split):
    N, H, h2 = y0.shape
    return (np.stack([y0, y1], axis=2) if half_split else np.stack([y0, y1], axis=3)).reshape(N, H * 2 * h2)


def rope_ref(x, pos, n_head, tables, sin_sign=1.0, half_split=False):
    """The rotation in float64 on fp32 inputs: x [N][E] fp32, row t at position pos[t]; tables = rope_tables_ref(...).  -> [N][E] float64.
    sin_sign = -1 and half_split are MUTANTS."""
    c, s = (t[np.asarray(pos)].astype(D)[:, None, :] for t in tables)
    s = s * sin_sign
    x0, x1 = _pairs(np.asarray(x, F).astype(D), n_head, half_split)
    return _unpairs(x0 * c - x1 * s, x0 * s + x1 * c, half_split)


def rope_f32(x, pos, n_head, tables, sin_sign=1.0, half_split=False):
    """The kernels' statements in np.float32: x0 * c - x1 * s, x0 * s + x1 * c, every product and sum rounded (the library is built without contraction).  -> fp32"""
    c, s = (t[np.asarray(pos)][:, None, :] for t in tables)
    s = s * F(sin_sign)
    x0, x1 = _pairs(np.asarray(x, F), n_head, half_split)
    y = _unpairs(x0 * c - x1 * s, x0 * s + x1 * c, half_split)
    assert y.dtype == F
    return y


def rope_bound(x, pos, hd, cache=False, tables=None):
    """Per element of a rotated row: |(x0, x1)| * (dtheta + 2^-22).  dtheta: rope_dtheta; 2^-22 covers the three fp32 roundings of a rotated element (at most
    (1 + sqrt 2) 2^-24 |(x0, x1)|) and the table entries' own rounding.  cache: plus half an fp16 ulp of the value (taken at |reference| + the bound in front, so that a
    value pushed over a power of two is covered).  x [N][E] fp32 -> [N][E] float64"""
    x = np.asarray(x, F).astype(D)
    N, E = x.shape
    n_head = E // hd
    x0, x1 = _pairs(x, n_head, False)
    b = np.hypot(x0, x1) * (rope_dtheta(pos, hd)[:, None, :] + 2.0 ** -22)
    b = _unpairs(b, b, False)
    if cache:
        ref = rope_ref(x, pos, n_head, tables)
        b = b + 0.5 * ulp16(np.abs(ref) + b)
    return b


def rope_unrotate(y, pos, n_head, hd):
    """fp32 rows whose rotation at pos[t] is y[t] up to fp32 rounding (the inputs' builder: a raw projection for a wanted rotated row)"""
    th = rope_thetas_ref(int(np.max(pos)) + 1, hd).astype(D)[np.asarray(pos)][:, None, :]
    c, s = np.cos(th), np.sin(th)
    y0, y1 = _pairs(np.asarray(y, D), n_head, False)
    return _unpairs(y0 * c + y1 * s, -y0 * s + y1 * c, False).astype(F)


# ---- one (head, query row) --------------------------------------------------------------------------------------------------------------------------------------------
def attn_scale(hd):
    """the kernels' 1.0f / sqrtf((float)hd)"""
    return float(F(1.0) / np.sqrt(F(hd)))


def _softmax_contract(s, m, fp16_points, count=None):
    x = s - m
    if not fp16_points:
        e = np.exp(x)
        return x, e / e.sum()
    e = f16(np.exp(f16(x).astype(D)))                                  # e_j = fp16(exp(fp16(s_j - m)))
    tot = (e.astype(D) * (1.0 if count is None else count)).sum()      # exact: a few thousand fp16 values in a double
    inv = F(1.0 / tot)                                                 # (float)(1.0 / tot)
    return x, f16(e.astype(F) * inv).astype(D)                         # p_j = fp16(fp32(e_j) * inv)


def attn_ref(qh, K, V, hd, fp16_points=True, scale_hd=None, n_max=None, count=None):
    """One head, one query, float64: qh [hd], K / V [T][hd] hold fp16 VALUES (any float type).  -> (out [hd], p [T], scale_d [hd] = sum_j p_j |v_jd|).
    fp16_points = False: no rounding point at all (the plain softmax(q K^T / sqrt(hd)) V).  MUTANTS: scale_hd -- the scale of another head size; n_max -- the softmax
    maximum taken over the first n_max keys only; count [T] -- how often key j is taken (0: left out, 2: counted twice), in the maximum, the sum and the output."""
    qh, K, V = (np.asarray(a, D) for a in (qh, K, V))
    s = (K @ qh) * (attn_scale(scale_hd or hd) if fp16_points else 1.0 / np.sqrt(scale_hd or hd))
    if count is not None:
        s = np.where(count > 0, s, -np.inf)                            # exp(-inf) = 0: the key is in neither the maximum nor the sum
    m = s.max() if n_max is None else s[:n_max].max()
    _, p = _softmax_contract(s, m, fp16_points, count)
    if count is not None:
        p = p * count
    return p @ V, p, p @ np.abs(V)


def attn_bound(qh, K, V, hd):
    """Per output dim, against attn_ref:   (2^-10 + 2 F) scale_d + hd 2^-24 scale_d,   scale_d = sum_j p_j |v_jd|.
      2^-10      every probability may be one fp16 ulp (2^-10 relative at most) off -- the computed-exp contract, and what a differently rounded 1 / tot can do to
                 p_j = fp16(e_j * inv); the same term for the table arm, not tightened;
      F          = sum over FRAGILE keys of p_j ulp16(s_j - m).  An fp32 chain of hd fma and one multiply, in any order, is within
                 eps_j = (hd + 2) 2^-24 scale sum_i |k_ji q_i| of the exact score, so x = s_j - m is within 2 eps (the maximum is such a score too).  Key j is fragile when
                 fp16(x - 2 eps) != fp16(x + 2 eps): its exponential may be taken one fp16 step of x away, a relative change of ulp16(x); once in p_j and once more through
                 the sum -- the 2;
      hd 2^-24   the fp32 accumulation of out_d."""
    qh, K, V = (np.asarray(a, D) for a in (qh, K, V))
    scale = attn_scale(hd)
    s = (K @ qh) * scale
    x, p = _softmax_contract(s, s.max(), True)
    eps = (hd + 2) * 2.0 ** -24 * scale * (np.abs(K) @ np.abs(qh))
    fragile = f16(x - 2 * eps) != f16(x + 2 * eps)
    Fr = float((p[fragile] * ulp16(x[fragile])).sum())
    scale_d = p @ np.abs(V)
    return (2.0 ** -10 + 2.0 * Fr) * scale_d + hd * 2.0 ** -24 * scale_d


ORDERS = ("sequential", "reversed", "partitioned")


def _fma32(a, b, c):
    """fmaf on fp16-valued a, b and an fp32 c: the product is exact in float64, the sum is rounded to float64 and then to fp32"""
    return (a.astype(D) * b.astype(D) + c.astype(D)).astype(F)


def attn_f32_emulated(qh, K, V, hd, order, P=None):
    """The contract with fp32 arithmetic where the kernels have it, for one query and ALL heads at once: qh [H][hd], K / V [T][H][hd] -> out [H][hd] fp32.  order (ORDERS)
    names how BOTH fp32 sums are taken:
      scores  sequential / reversed: one fma chain over the head dim, up or down; partitioned: the body's dot16 -- 8-dim fma chains, added pairwise across the lanes;
      P.V     sequential / reversed: one fma chain over the keys, up or down; partitioned: key j in chain j mod P, the P chains added in order (the body's order)."""
    qf, Kf, Vf = (f16(a).astype(F) for a in (qh, K, V))
    T, H = Kf.shape[:2]
    P = P or 512 // (hd // 8)
    if order == "partitioned":
        parts = np.zeros((T, H, hd // 8), F)
        for e in range(8):
            parts = _fma32(Kf.reshape(T, H, hd // 8, 8)[..., e], qf.reshape(H, hd // 8, 8)[None, ..., e], parts)
        while parts.shape[-1] > 1:                                     # the DPP adds: lane pairs, then pairs of pairs
            parts = parts[..., 0::2] + parts[..., 1::2]
        s = parts[..., 0]
    else:
        s = np.zeros((T, H), F)
        for i in (range(hd) if order == "sequential" else range(hd - 1, -1, -1)):
            s = _fma32(Kf[..., i], qf[None, :, i], s)
    s = s * F(attn_scale(hd))
    assert s.dtype == F
    x = s - s.max(0, keepdims=True)                                    # fp32, as the kernels subtract
    e = f16(np.exp(f16(x).astype(D)))
    inv = (1.0 / e.astype(D).sum(0, keepdims=True)).astype(F)
    p = f16(e.astype(F) * inv).astype(F)                               # [T][H]
    if order == "partitioned":
        rounds = -(-T // P)
        pp = np.zeros((rounds * P, H), F); pp[:T] = p
        vv = np.zeros((rounds * P, H, hd), F); vv[:T] = Vf
        o = np.zeros((P, H, hd), F)
        for r in range(rounds):
            o = _fma32(vv[r * P:(r + 1) * P], pp[r * P:(r + 1) * P, :, None], o)
        out = np.zeros((H, hd), F)
        for q_ in range(P):
            out = out + o[q_]
    else:
        out = np.zeros((H, hd), F)
        for j in (range(T) if order == "sequential" else range(T - 1, -1, -1)):
            out = _fma32(Vf[j], p[j][:, None], out)
    assert out.dtype == F
    return out


# ---- a whole launch ------------------------------------------------------------------------------------------------------------------------------------------------------
# A case (dict, arrays read-only):
#   kind     "pass": rows of raw projections q, k, v; row t belongs to conversation slot[t] at position pos[t] and sees the cache rows [0, p0) of its conversation (p0 = the
#            lowest position of the pass in that conversation), then the pass's rows of that conversation up to its own.  This is every fused form (one row; batched: one
#            row per conversation; verify: R rows of one), the key-split form stepped L times, and launch_rope_kv + the plain form.
#            "prompt": q is already rotated, every key comes from the cache: row t sees the cache rows [0, pos[t]].
#   hd, n_head, n_ctx, kc / vc [n_slot][n_ctx][E] float16, q / k / v [R][E] float32, slot [R], pos [R], probes (the needle positions, per conversation)
MUTANTS = ("drop_key", "last_cached_twice", "own_key_left_out", "own_key_unrotated", "q_at_pos_minus_1", "q_at_pos_plus_1", "sin_sign", "half_split_pairs",
           "scale_of_other_head_size", "max_over_cached_only", "values_of_next_head", "causal_one_too_long", "causal_one_too_short", "verify_reads_stale_cache_row")


def mutants_of(case):
    """[(name, arg)]: every mutant that APPLIES to the case -- that changes the mathematics of at least one of its rows (why each condition: at the branches)."""
    multi = max(np.bincount(case["slot"])) > 1
    p0 = _p0(case)
    out = []
    if case.get("own_lead"):
        # the maximum over the cached keys only is, in exact arithmetic, the same softmax: it shows when the own key leads by more than fp16's exp can hold (e^11.09);
        # these cases are built for that, their own key holds nearly all the weight and hides every other key -- only what concerns the own key applies
        return [("max_over_cached_only", None), ("own_key_left_out", None), ("own_key_unrotated", None)]
    for s in range(case["kc"].shape[0]):
        rows = np.flatnonzero(case["slot"] == s)
        T_last = case["pos"][rows].max() + (1 if case["kind"] == "prompt" else 0)
        out += [("drop_key", (s, j)) for j in case["probes"][s] if j < (T_last if case["kind"] == "prompt" else p0[s])]
    if (p0 >= 1).any() or case["kind"] == "prompt":
        out.append(("last_cached_twice", None))
    out.append(("values_of_next_head", None))
    if case["pos"].max() >= 1:                                           # a lone key's probability is 1 at every scale
        out.append(("scale_of_other_head_size", None))
    if case["kind"] == "pass":
        if case["pos"].max() >= 1:
            # a row at position 0 has no key but its own (without it there is no softmax) and is not rotated (the angle is 0 for every pairing and either sign)
            out += [("own_key_left_out", None), ("own_key_unrotated", None), ("q_at_pos_minus_1", None), ("sin_sign", None), ("half_split_pairs", None)]
        if (p0 >= 1).any():                                           # a pass from an empty cache: q and the pass's keys would turn together
            out.append(("q_at_pos_plus_1", None))
    if multi or case["kind"] == "prompt":
        out += [("causal_one_too_long", None), ("causal_one_too_short", None)]
    if multi and case["kind"] == "pass":
        out.append(("verify_reads_stale_cache_row", None))
    return out


def _p0(case):
    p0 = np.zeros(case["kc"].shape[0], np.int64)
    for s in range(len(p0)):
        rows = case["pos"][case["slot"] == s]
        p0[s] = rows.min() if len(rows) else 0
    return p0


@functools.lru_cache(maxsize=8)
def _tables(n, hd):
    return rope_tables_ref(n, hd)


_CACHES64 = {}


def _caches64(case):
    """the case's caches as float64 (fp16 -> float64 is numpy's slowest conversion; the mutants of one case ask for it dozens of times): the last two cases are kept"""
    key = id(case["kc"])
    if key not in _CACHES64:
        if len(_CACHES64) >= 2:
            _CACHES64.clear()
        _CACHES64[key] = (case["kc"].astype(D), case["vc"].astype(D), case["kc"])      # the array itself is held, so its id is not reused
    return _CACHES64[key][:2]


def expected(case, mutant=None, emulate=None, P=None, rows=None):
    """-> dict(out [R][E] float64, bound [R][E], q_rot [R][E] float64 or None, k_rows [R][E] float64 / v_rows [R][E] float16: the appended cache rows (pass cases)).
    mutant = (name, arg) of mutants_of(case): the same with ONE line changed (marked MUTANT below); its bound is not computed.
    emulate = one of ORDERS: out is attn_f32_emulated's on the same operands (P: its partition count) -- what fp32 arithmetic in that order gives; no bound either.
    rows: only these rows of out / bound are computed (the others stay zero)."""
    name, arg = mutant or (None, None)
    hd, H, n_ctx, kind = case["hd"], case["n_head"], case["n_ctx"], case["kind"]
    E, R = H * hd, len(case["pos"])
    pos, slot, p0 = case["pos"], case["slot"], _p0(case)
    tabs = _tables(n_ctx + 1, hd)
    kc64, vc64 = _caches64(case)
    res = dict(out=np.zeros((R, E)), bound=None if name or emulate else np.zeros((R, E)), q_rot=None, k_rows=None, v_rows=None)
    if kind == "pass":
        rope_kw = dict(sin_sign=-1.0 if name == "sin_sign" else 1.0, half_split=name == "half_split_pairs")                     # MUTANTS
        qpos = pos - 1 if name == "q_at_pos_minus_1" else pos + 1 if name == "q_at_pos_plus_1" else pos                        # MUTANTS
        qh = f16(rope_f32(case["q"], np.maximum(qpos, 0), H, tabs, **rope_kw)).astype(D)
        kp = f16(rope_f32(case["k"], pos, H, tabs, **rope_kw)).astype(D)
        vp = f16(case["v"]).astype(D)
        if not name:
            res["q_rot"], res["k_rows"], res["v_rows"] = rope_ref(case["q"], pos, H, tabs), rope_ref(case["k"], pos, H, tabs), f16(case["v"])
    else:
        qh = f16(case["q"]).astype(D)
    ka, va = kc64, vc64
    if kind == "pass":                                                 # the caches as the pass leaves them: a row's keys are then the rows [0, pos]
        ka, va = kc64.copy(), vc64.copy()
        ka[slot, pos], va[slot, pos] = kp, vp
    for t in (range(R) if rows is None else rows):
        s, T = slot[t], int(pos[t]) + 1
        n_cached = int(p0[s]) if kind == "pass" else T
        if name == "causal_one_too_long" and T < n_ctx:                                                                         # MUTANT: the pass's next row, or what lies behind it
            T += 1
        K, V = ka[s, :T], va[s, :T]
        w = np.ones(T)                                                 # how often each key counts: 1
        if name == "verify_reads_stale_cache_row":                                                                              # MUTANT
            K, V = K.copy(), V.copy()
            K[n_cached:pos[t]], V[n_cached:pos[t]] = kc64[s, n_cached:pos[t]], vc64[s, n_cached:pos[t]]
        if name == "own_key_unrotated":                                                                                         # MUTANT
            K = K.copy(); K[pos[t]] = f16(case["k"][t]).astype(D)
        if name in ("own_key_left_out", "causal_one_too_short") and pos[t] >= 1:                                                # MUTANTS
            w[pos[t]] = 0.0
        if name == "drop_key" and arg[0] == s and arg[1] < T and T > 1:                                                         # MUTANT
            w[arg[1]] = 0.0
        if name == "last_cached_twice" and n_cached >= 1:                                                                       # MUTANT: a clamped load taken as live
            w[min(n_cached, T) - 1] = 2.0
        K, V = K.reshape(len(K), H, hd), V.reshape(len(V), H, hd)
        if emulate:
            res["out"][t] = attn_f32_emulated(qh[t].reshape(H, hd), K, V, hd, emulate, P).reshape(E)
            continue
        for h in range(H):
            hv = (h + 1) % H if name == "values_of_next_head" else h                                                             # MUTANT
            kw = dict(count=w) if name else {}
            if name == "scale_of_other_head_size":                                                                              # MUTANT
                kw["scale_hd"] = 64 if hd == 128 else 2 * hd
            if name == "max_over_cached_only" and kind == "pass" and p0[s] >= 1:                                                # MUTANT
                kw["n_max"] = int(p0[s])
            q1 = qh[t, h * hd:(h + 1) * hd]
            with np.errstate(over="ignore", invalid="ignore"):
                res["out"][t, h * hd:(h + 1) * hd] = attn_ref(q1, K[:, h], V[:, hv], hd, **kw)[0]
            if not name:
                res["bound"][t, h * hd:(h + 1) * hd] = attn_bound(q1, K[:, h], V[:, h], hd)
    return res


def ratio(got, want, bound):
    """max over the elements of |got - want| / bound (0 / 0 = 0; anything that is not finite counts as infinitely far)"""
    got, want = np.asarray(got, D), np.asarray(want, D)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    r = np.where(np.isfinite(got), r, np.inf)
    return float(r.max())


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------------------------------
def _frozen(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _unit_dirs(rng, H, hd):
    """one direction per head with |u|^2 = hd exactly (a unit-normal vector's expected length): a needle's score is then its gain, whatever the draw"""
    u = rng.standard_normal((H, hd))
    return u * (np.sqrt(hd) / np.linalg.norm(u, axis=1, keepdims=True))


def pass_case(hd, n_head, n_ctx, convs, probes_fn, seed, row_order=None, gain=4.0, own_lead=False):
    """Needle inputs for a "pass" launch.  convs = [(p0, R)]: conversation s has p0 cached rows and R rows of this pass at p0 .. p0 + R - 1; the launch's rows are the
    conversations' rows in order, permuted by row_order.  Caches and v rows: unit normals (fp16 / fp32).  Per conversation and head a direction u, |u|^2 = hd:
      - every pass row's q is built so that its ROTATED q is u + 0.25 noise, every pass row's k so that its rotated k is a needle (below);
      - the cache key at each probe position (probes_fn(hd, p0) plus key 0 and the last cached key) is the needle u * gain / sqrt(hd) + 0.25 noise: its score is about
        `gain` where an ordinary key's is a unit normal, so each needle holds a visible share of the softmax;
      - the cache rows p0 .. p0 + R - 1 the pass overwrites hold ordinary rows (what a stale read would get), row p0 + R, the first behind the pass, is a needle again
        (what a causal range one key too long would add).
    own_lead: the pass keys' gain is 5 x gain -- the own key's score leads every cached key's by more than 11.09, where fp16(exp(.)) overflows."""
    rng = np.random.default_rng(seed)
    E, S = n_head * hd, len(convs)
    kc, vc = f16(rng.standard_normal((S, n_ctx, E))), f16(rng.standard_normal((S, n_ctx, E)))
    g = gain / np.sqrt(hd)
    q, k, v, slot, pos, probes = [], [], [], [], [], []
    for s, (p0, R) in enumerate(convs):
        assert 0 <= p0 and R >= 1 and p0 + R <= n_ctx
        u = _unit_dirs(rng, n_head, hd)
        pr = sorted({j for j in list(probes_fn(hd, p0)) + [0, p0 - 1] if 0 <= j < p0})
        behind = [p0 + R] if p0 + R < n_ctx else []
        for j in pr + behind:
            kc[s, j] = f16((u * g + 0.25 * rng.standard_normal((n_head, hd))).reshape(E))
        pp = p0 + np.arange(R)
        q.append(rope_unrotate((u[None] + 0.25 * rng.standard_normal((R, n_head, hd))).reshape(R, E), pp, n_head, hd))
        k.append(rope_unrotate((u[None] * g * (5.0 if own_lead else 1.0) + 0.25 * rng.standard_normal((R, n_head, hd))).reshape(R, E), pp, n_head, hd))
        v.append(rng.standard_normal((R, E)).astype(F))
        slot += [s] * R; pos += list(pp); probes.append(pr)
    order = np.arange(len(slot)) if row_order is None else np.asarray(row_order)
    return _frozen(dict(kind="pass", hd=hd, n_head=n_head, n_ctx=n_ctx, kc=kc, vc=vc, q=np.concatenate(q)[order], k=np.concatenate(k)[order], v=np.concatenate(v)[order],
                        slot=np.asarray(slot)[order], pos=np.asarray(pos)[order], probes=probes, own_lead=own_lead))


def needle_case(hd, n_head, T, probes, seed, rows=1, n_ctx=None, **kw):
    """One conversation with T cached keys and `rows` rows of this pass behind them; probes: the needle positions (key 0 and the last cached key are added)."""
    return pass_case(hd, n_head, n_ctx or T + rows + 1, [(T, rows)], lambda hd_, p0: probes, seed, **kw)


def prompt_case(hd, n_head, n_ctx, pos0, N, seed, gain=4.0):
    """Needle inputs for the prompt kernels: q [N][E] is the ROTATED q (u + 0.25 noise per row), the cache holds needles at key 0, around the 64-key tile edges, at every
    row's own key (positions pos0 .. pos0 + N - 1) and at position pos0 + N -- the first row behind the prompt, which no query may see; further rows are ordinary."""
    rng = np.random.default_rng(seed)
    E = n_head * hd
    kc, vc = f16(rng.standard_normal((1, n_ctx, E))), f16(rng.standard_normal((1, n_ctx, E)))
    u = _unit_dirs(rng, n_head, hd)
    T = pos0 + N
    assert T < n_ctx
    edges = [0, 15, 16, 31, 32, 63, 64, 65, 127, 128, pos0 - 1, pos0, T - 1]
    pr = sorted({j for j in edges + list(range(pos0, T)) if 0 <= j < T})
    for j in pr + [T]:
        kc[0, j] = f16((u * (gain / np.sqrt(hd)) + 0.25 * rng.standard_normal((n_head, hd))).reshape(E))
    q = (u[None] + 0.25 * rng.standard_normal((N, n_head, hd))).reshape(N, E).astype(F)
    return _frozen(dict(kind="prompt", hd=hd, n_head=n_head, n_ctx=n_ctx, kc=kc, vc=vc, q=q, k=None, v=None, slot=np.zeros(N, np.int64), pos=pos0 + np.arange(N),
                        probes=[sorted({j for j in edges if 0 <= j < T})]))          # the keys the drop mutants take: the edges, not every row's own key


def rope_case(hd, n_head, segs, seed):
    """q, k, v [N][E] fp32 unit normals for the packed rows of segs = [(slot, rows, pos0)]; -> (q, k, v, slot [N], pos [N])"""
    rng = np.random.default_rng(seed)
    N = sum(r for _, r, _ in segs)
    q, k, v = (rng.standard_normal((N, n_head * hd)).astype(F) for _ in range(3))
    slot = np.concatenate([[s] * r for s, r, _ in segs])
    pos = np.concatenate([p + np.arange(r) for _, r, p in segs])
    return q, k, v, slot, pos


# ---- the case lists (tests/test_cpu_attn_ref.py checks reference, bound and mutants on exactly these; tests/test_gpu_attn_kernels.py runs the kernels on them) ------------
N_HEAD = 3                                                              # an odd head count, so that head indexing shows
HDS = (128, 64, 32)


def body_P(hd):
    """key partitions of the decode body (attn_llm_body.hpp: AT_THREADS / (hd / 8)); it prefetches 16 P keys and then takes 8 P per round"""
    return 512 // (hd // 8)


def split_P(hd):
    """key partitions of the key-split kernels (AS_THREADS / (hd / 8)); 16 keys per lane group in flight"""
    return 256 // (hd // 8)


BODY_CTX = {128: 1024, 64: 1664, 32: 3200}                              # holds 16 P + 8 P + 3 cached keys and the pass's rows, for every form


def body_positions(hd):
    P = body_P(hd)
    return (0, 1, P - 1, P, P + 1, 16 * P - 1, 16 * P, 16 * P + 1, 16 * P + 8 * P + 3)


def body_probes(hd, T):
    """where the body changes behaviour: partition boundary, end of the 16 P prefetch, the rounds of the steady loop (8 P each) and its ragged tail"""
    P = body_P(hd)
    return [j for b in (1, P, 16 * P, 24 * P) for j in (b - 1, b, b + 1)] + [T - 2]


def split_per(T, S, P):
    return -(-(-(-T // S)) // P) * P


def split_probes_for(S):
    def probes(hd, T):
        """first / last key of every split's range, for the score launch (T keys) and the P.V launch (T + 1), and the end of a split's first round of 16 P keys"""
        P = split_P(hd)
        out = [1, P - 1, P, T - 2]
        for per in {split_per(T, S, P), split_per(T + 1, S, P)}:
            for sp in range(1, S):
                out += [sp * per - 1, sp * per]
            out += [16 * P - 1, 16 * P, per + 16 * P - 1, per + 16 * P]
        return out
    return probes


def split_positions(hd, S):
    """first positions of the L = 3 steps of a key-split case (n_ctx - 2: the two steps that fit)"""
    P = split_P(hd)
    steady = (16 * P * S - 1, 16 * P * S, (S - 1) * 17 * P + 16 * P + 1)     # the last split's range ends at 16 P - 1, 16 P, 16 P + 1 keys
    return (0, 1, P - 1, P, S * P - 1, S * P, S * P + 1) + steady + (split_ctx(hd, S) - 2,)


def split_ctx(hd, S):
    P = split_P(hd)
    return ((S - 1) * 17 * P + 16 * P + 1 + 3 + 8 + 7) // 8 * 8


# (form, hd, positions): form 0 one row, form 1 three rows in three slots (row r = conversation row_slot[r])
DECODE_CASES = [("one", hd, (n_past,)) for hd in HDS for n_past in body_positions(hd)] + \
               [("batched", hd, body_positions(hd)[3 * g:3 * g + 3]) for hd in HDS for g in range(3)] + \
               [("one_own_lead", hd, (body_P(hd) + 1,)) for hd in HDS]
BATCHED_ROW_SLOT = (2, 0, 1)
# (hd, p0, R): the pass's rows straddle a partition boundary and the end of the prefetch
VERIFY_CASES = [(hd, 16 * body_P(hd) - 3, R) for hd in HDS for R in (1, 2, 8)] + [(hd, 0, 8) for hd in HDS] + [(hd, 24 * body_P(hd) + 3 - 8, 8) for hd in HDS]
SPLITS = (2, 6, 16)
SPLIT_CASES = [(hd, S, n_past) for hd in HDS for S in SPLITS for n_past in split_positions(hd, S)]
SPLIT_WIDE = (128, 6, 777, 40, 1024)                                    # split_case(hd, S, position, heads, n_ctx): the 13B grid, 240 workgroups across the XCDs
PLAIN_CASES = [(hd, n_past, N) for hd in HDS for n_past in (0, 16 * body_P(hd) - 2) for N in (1, 5)]
PROMPT_FORMS = (1, 2, 3, 4)
PROMPT_CASES = [(hd, pos0, N) for hd in HDS for pos0 in (0, 1, 63, 64, 100) for N in (2, 15, 16, 17, 33, 65)]
PROMPT_CTX = 176                                                       # 100 + 65 keys and ordinary rows behind them
ROPE_CTX = 2048
ROPE_SEGS = [(0, 3, 0), (2, 2, 1), (1, 5, 2043), (2, 17, 600)]          # (slot, rows, first position): positions 0, 1 and n_ctx - 1 = 2047 among them; slot 2 twice
ROPE_CASES = [(hd, ks) for hd in HDS for ks in (1, 3)]


@functools.lru_cache(maxsize=None)
def decode_case(form, hd, positions):
    n_ctx = BODY_CTX[hd]
    seed = 100000 + 1000 * hd + 7 * positions[0] + len(positions)
    if form == "batched":
        return pass_case(hd, N_HEAD, n_ctx, [(p, 1) for p in positions], body_probes, seed, row_order=BATCHED_ROW_SLOT)
    return pass_case(hd, N_HEAD, n_ctx, [(positions[0], 1)], body_probes, seed, own_lead=form == "one_own_lead")


@functools.lru_cache(maxsize=None)
def verify_case(hd, p0, R):
    return pass_case(hd, N_HEAD, BODY_CTX[hd], [(p0, R)], body_probes, 200000 + 1000 * hd + 10 * p0 + R)


@functools.lru_cache(maxsize=None)
def split_case(hd, S, n_past, n_head=N_HEAD, n_ctx=None):
    """The needles' gain grows with the logarithm of the key count beyond 1024 keys: the ordinary keys' exponentials add up to about 1.65 per key, so a needle of fixed
    gain would hold an ever smaller share among the 17 000 keys the steady loop of 16 splits needs at head size 32."""
    n_ctx = n_ctx or split_ctx(hd, S)
    gain = 4.0 + max(0.0, float(np.log((n_past + 1) / 1024.0)))
    return pass_case(hd, n_head, n_ctx, [(n_past, min(3, n_ctx - n_past))], split_probes_for(S), 300000 + 1000 * hd + 37 * S + n_past, gain=gain)


@functools.lru_cache(maxsize=None)
def plain_case(hd, n_past, N):
    return pass_case(hd, N_HEAD, BODY_CTX[hd], [(n_past, N)], body_probes, 400000 + 1000 * hd + 10 * n_past + N)


@functools.lru_cache(maxsize=None)
def prompt_case_of(hd, pos0, N):
    return prompt_case(hd, N_HEAD, PROMPT_CTX, pos0, N, 500000 + 1000 * hd + 100 * pos0 + N)


@functools.lru_cache(maxsize=None)
def expected_of(maker, *key):
    """expected(case) of a listed case, computed once per process and shared"""
    res = expected(maker(*key))
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res
