"""Quantised mat-mul / mat-vec / embedding-gather kernels on ARBITRARY block bytes, against float64.  No GPU in here; tests/test_cpu_quant_blocks.py checks this module
against the oracle, tests/test_gpu_quant_blocks.py runs the kernels on exactly the same inputs.

Why: every other quantised test decodes only what quants.quantize emits from Gaussian values, and compares at 2e-5 of the ROW MAXIMUM because activation quantisation noise
forbids more.  Here the block bytes are arbitrary (uniform random, or constant extreme patterns) and the activation rows are integers that quantise EXACTLY:
  * Q8_K is exact with d = 1 for integers in [-128, 127] when -128 is present in every non-zero 256-block;
  * Q8_0 / Q8_1 are exact with d = 1 for integers in [-127, 127] when +-127 is present in every non-zero 32-block;
  * the fp16 / fp32 activation paths hold those integers exactly.
So the mathematically exact output is the float64 product of the rows with the float64-decoded blocks, and the only error a correct kernel has left is fp32 summation.

THE BOUND of one output (derived, not measured):  (n_blocks_along_K + 4) * 2^-24 * sum_k |x_k| * a_k,  a = the weight's UNCANCELLED magnitude (below).  Any order of fp32
additions of the per-block terms fits: n terms added in any order err by at most (n - 1) * 2^-24 * sum |term| to first order, each per-block term carries at most a few
roundings of its own (d_w * d_a * float(isum), the fp32 conversion of an integer above 2^24), and each term's magnitude is at most its block's share of sum |x| a -- `a` counts
the parts that a kernel forms separately (scale part and min part; code part and offset part) without their cancellation.  A residual adds one fp32 addition: 2^-24 of the
result.  Where the bound is zero (an all-zero row, d = dmin = 0) the output must be exactly zero.

Inf and NaN fields are out of scope: every fp16 d / dmin / m field is finite (generators overwrite them), fp16 / fp32 weights are finite.

The float64 decoders are written from the bit fields (ggml's block layouts), NOT on quants.dequantize_*; the oracle's dequantize_row is the second opinion (CPU test).
"""
import functools

import numpy as np

F32, F16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0 = 0, 1, 2, 3, 6, 7, 8
Q2_K, Q3_K, Q4_K, Q5_K, Q6_K = 10, 11, 12, 13, 14
NAMES = {F32: "f32", F16: "f16", Q4_0: "q4_0", Q4_1: "q4_1", Q5_0: "q5_0", Q5_1: "q5_1", Q8_0: "q8_0", Q2_K: "q2_k", Q3_K: "q3_k", Q4_K: "q4_k", Q5_K: "q5_k", Q6_K: "q6_k"}
TYPE = {v: k for k, v in NAMES.items()}
BLOCK = {F32: (1, 4), F16: (1, 2), Q4_0: (32, 18), Q4_1: (32, 20), Q5_0: (32, 22), Q5_1: (32, 24), Q8_0: (32, 34), Q2_K: (256, 84), Q3_K: (256, 110), Q4_K: (256, 144),
         Q5_K: (256, 176), Q6_K: (256, 210)}
ALL_TYPES = [Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K, F16, F32]
K_TYPES = (Q2_K, Q3_K, Q4_K, Q5_K, Q6_K)                       # Q8_K activations (256-element blocks); everything else: 32-element rows
TWO_TERM = (Q4_1, Q5_1, Q2_K, Q4_K, Q5_K)                       # w = scale part - min part: one fp32 rounding when a decoder forms it; the others decode exactly
U = 2.0 ** -24
# byte offsets of the fp16 fields of a block
F16_FIELDS = {Q4_0: (0,), Q4_1: (0, 2), Q5_0: (0,), Q5_1: (0, 2), Q8_0: (0,), Q2_K: (80, 82), Q3_K: (108,), Q4_K: (0, 2), Q5_K: (0, 2), Q6_K: (208,)}
# what the generators put into those fields: +-0, +- the smallest subnormal, +-1e-3, +-0.37, +-2.0 (fp16 roundings of them)
FIELD_VALUES = np.array([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 1e-3, -1e-3, 0.37, -0.37, 2.0, -2.0], np.float16)


def n_blocks(t, K):
    return K // BLOCK[t][0]


def row_bytes(t, K):
    return K // BLOCK[t][0] * BLOCK[t][1]


def _h(b, off):
    """fp16 field at byte offset off of blocks b [nb][bytes] -> float64 [nb]"""
    return np.ascontiguousarray(b[:, off:off + 2]).view(np.float16)[:, 0].astype(np.float64)


def _k4_scales(s, mutant):
    """the 6-bit scale / min pairs of Q4_K / Q5_K: s [nb][12] -> sc, mn [nb][8] ints"""
    s = s.astype(np.int64)
    sc, mn = np.empty((s.shape[0], 8), np.int64), np.empty((s.shape[0], 8), np.int64)
    for j in range(8):
        if j < 4:
            sc[:, j], mn[:, j] = s[:, j] & 63, s[:, j + 4] & 63
        elif mutant == "k4_high_bits_ignored":                                       # MUTANT: sub-blocks 4..7 lose their two high bits
            sc[:, j], mn[:, j] = s[:, j + 4] & 0xF, s[:, j + 4] >> 4
        else:
            sc[:, j], mn[:, j] = (s[:, j + 4] & 0xF) | ((s[:, j - 4] >> 6) << 4), (s[:, j + 4] >> 4) | ((s[:, j] >> 6) << 4)
    return sc, mn


def _parts(t, raw, n, mutant=None):
    """The decoded parts of n weights, each float64 [n]: (p, off, mpart) with w = p - off - mpart where
       p     = the scale part d * sc * code (one-term types without offset: the value),
       off   = d * sc * offset of the offset forms (Q4_0 8, Q5_0 16, Q6_K 32, Q3_K through its Q6_K image: 32), else 0,
       mpart = dmin * m of Q2_K / Q4_K / Q5_K, -m of Q4_1 / Q5_1, else 0.
    mutant: one decoding step done wrongly (MUTANTS)."""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    z = np.zeros(n)
    if t == F32:
        return raw[:4 * n].view(np.float32).astype(np.float64), z, z
    if t == F16:
        return raw[:2 * n].view(np.float16).astype(np.float64), z, z
    be, bb = BLOCK[t]
    nb = n // be
    b = raw[:nb * bb].reshape(nb, bb)
    e = np.arange(be)
    fix = (lambda d: np.abs(d)) if mutant == "d_sign_dropped" else (lambda d: d)   # MUTANT: |d|
    swap = mutant == "nibbles_swapped"                                              # MUTANT: low and high nibble halves exchanged
    if t in (Q4_0, Q4_1, Q5_0, Q5_1):
        qo = {Q4_0: 2, Q4_1: 4, Q5_0: 6, Q5_1: 8}[t]
        qs = b[:, qo:qo + 16].astype(np.int64)
        lo, hi = (qs >> 4, qs & 15) if swap else (qs & 15, qs >> 4)
        q = np.concatenate([lo, hi], axis=1)                                         # element j < 16: low nibble of byte j; j >= 16: high nibble of byte j - 16
        if t in (Q5_0, Q5_1):
            qh = np.ascontiguousarray(b[:, qo - 4:qo]).view(np.uint32)[:, 0].astype(np.int64)
            bit = (e + 1) & 31 if mutant == "q5_high_bit_neighbour" else e           # MUTANT: the neighbouring bit
            q = q | (((qh[:, None] >> bit[None, :]) & 1) << 4)
        d = fix(_h(b, 0))[:, None]
        p = d * q
        if t in (Q4_1, Q5_1):
            return p.reshape(-1), z, -np.repeat(_h(b, 2), 32)
        return p.reshape(-1), np.broadcast_to(d * (8 if t == Q4_0 else 16), p.shape).reshape(-1), z
    if t == Q8_0:
        return (fix(_h(b, 0))[:, None] * b[:, 2:34].view(np.int8).astype(np.float64)).reshape(-1), z, z
    s, l = e >> 5, e & 31                                                            # 32-weight sub-block and position in it
    if t in (Q4_K, Q5_K):
        d, dm = fix(_h(b, 0)), _h(b, 2)
        if mutant == "dmin_read_as_d":                                               # MUTANT
            dm = d
        sc, mn = _k4_scales(b[:, 4:16], mutant)
        qs = b[:, (16 if t == Q4_K else 48):][:, (s >> 1) * 32 + l].astype(np.int64)
        q = np.where(((s & 1) == 1) != swap, qs >> 4, qs & 15)
        if t == Q5_K:
            sh = (s + 1) & 7 if mutant == "q5_high_bit_neighbour" else s
            q = q + 16 * ((b[:, 16:48][:, l].astype(np.int64) >> sh[None, :]) & 1)
        return ((d[:, None] * sc[:, s]) * q).reshape(-1), z, (dm[:, None] * mn[:, s]).reshape(-1)
    if t == Q2_K:
        d, dm = fix(_h(b, 80)), _h(b, 82)
        if mutant == "dmin_read_as_d":
            dm = d
        scb = b[:, 0:16][:, e >> 4].astype(np.int64)
        sc, mn = (scb >> 4, scb & 15) if swap else (scb & 15, scb >> 4)
        q = (b[:, 16:80][:, 32 * (e >> 7) + l].astype(np.int64) >> (2 * ((e >> 5) & 3))[None, :]) & 3
        return ((d[:, None] * sc) * q).reshape(-1), z, (dm[:, None] * mn).reshape(-1)
    if t == Q6_K:
        d = fix(_h(b, 208))
        n7, a4 = e >> 7, (e >> 5) & 3
        qlb = b[:, 0:128][:, 64 * n7 + 32 * (a4 & 1) + l].astype(np.int64)
        lo = np.where(((a4 & 2) == 2) != swap, qlb >> 4, qlb & 15)
        pair = (a4 + 1) & 3 if mutant == "q6_high_bits_shifted" else a4              # MUTANT: the high two bits of the next pair
        hi = (b[:, 128:192][:, 32 * n7 + l].astype(np.int64) >> (2 * pair)[None, :]) & 3
        scb = b[:, 192:208][:, 8 * n7 + 2 * a4 + (l >> 4)]
        sc = scb.astype(np.int64) if mutant == "q6_scales_unsigned" else scb.view(np.int8).astype(np.int64)   # MUTANT: int8 scales read as unsigned
        ds = d[:, None] * sc
        return (ds * (lo | (hi << 4))).reshape(-1), (ds * 32).reshape(-1), z
    if t == Q3_K:                                                                    # 110 bytes: hmask[32], qs[64], scales[12] (sixteen 6-bit), d
        d = fix(_h(b, 108))
        sb = b[:, 96:108].astype(np.int64)
        sc16 = np.empty((nb, 16), np.int64)
        for j in range(4):
            hi = sb[:, 8 + j]
            sc16[:, j] = (sb[:, j] & 15) | ((hi & 3) << 4)
            sc16[:, 4 + j] = (sb[:, 4 + j] & 15) | (((hi >> 2) & 3) << 4)
            sc16[:, 8 + j] = (sb[:, j] >> 4) | (((hi >> 4) & 3) << 4)
            sc16[:, 12 + j] = (sb[:, 4 + j] >> 4) | (((hi >> 6) & 3) << 4)
        n7, j4 = e >> 7, (e >> 5) & 3
        v = ((b[:, 32:96][:, 32 * n7 + l].astype(np.int64) >> (2 * j4)[None, :]) & 3) - 4 * (1 - ((b[:, 0:32][:, l].astype(np.int64) >> (4 * n7 + j4)[None, :]) & 1))
        ds = d[:, None] * (sc16[:, e >> 4] - 32)
        # the kernels see the value-identical Q6_K image of the load path: code = v + 32 against the offset 32
        return (ds * (v + 32)).reshape(-1), (ds * 32).reshape(-1), z
    raise ValueError(t)


def decode(t, raw, n, mutant=None):
    """-> (w, a) float64 [n]: the value and its uncancelled magnitude (a >= |w|):
         Q4_K, Q5_K, Q2_K   w = d sc q - dmin m        a = |d sc q| + |dmin m|
         Q4_1, Q5_1         w = d q + m                a = |d q| + |m|
         Q6_K, Q5_0, Q4_0   w = d sc (code - off)      a = |d sc| (code + off)      (the kernels form the code part and the offset part separately; Q3_K: as its Q6_K image)
         Q8_0, F16, F32     w                          a = |w|"""
    p, off, m = _parts(t, raw, n, mutant)
    return p - off - m, np.abs(p) + np.abs(off) + np.abs(m)


def _seed(*key):
    h = 2166136261
    for v in key:
        for c in str(v).encode():
            h = ((h ^ c) * 16777619) & 0xFFFFFFFF
    return h


def _set_fields(t, b, values_for):
    """overwrite every fp16 field of blocks b [rows][nb][bytes]: values_for(field index) -> fp16 [rows][nb]"""
    for i, off in enumerate(F16_FIELDS[t]):
        b[:, :, off:off + 2] = np.ascontiguousarray(values_for(i).astype(np.float16))[..., None].view(np.uint8)


def random_blocks(t, n_rows, K, seed):
    """raw bytes [n_rows][row_bytes] of uniformly random blocks: every byte uniform in 0..255, then every fp16 d / dmin / m field drawn from FIELD_VALUES (finite: Inf and NaN
    are out of scope).  F16 / F32 weights: a FIELD_VALUES entry times a random integer in [-15, 15] (rounded to the type)."""
    rng = np.random.default_rng(_seed("random", t, n_rows, K, seed))
    if t in (F16, F32):
        v = FIELD_VALUES[rng.integers(0, len(FIELD_VALUES), (n_rows, K))].astype(np.float64) * rng.integers(-15, 16, (n_rows, K))
        return np.ascontiguousarray(v.astype(np.float16 if t == F16 else np.float32)).view(np.uint8).reshape(n_rows, -1)
    nb, bb = n_blocks(t, K), BLOCK[t][1]
    b = rng.integers(0, 256, (n_rows, nb, bb), dtype=np.uint8)
    _set_fields(t, b, lambda i: FIELD_VALUES[rng.integers(0, len(FIELD_VALUES), (n_rows, nb))])
    return b.reshape(n_rows, nb * bb)


# the byte ranges of a block that hold sub-block scales (the rest, apart from the fp16 fields, are quants)
SCALE_BYTES = {Q2_K: (0, 16), Q3_K: (96, 108), Q4_K: (4, 16), Q5_K: (4, 16), Q6_K: (192, 208)}
FILLS = (0xFF, 0x00, 0x80, 0x7F)
EXTREME_D = (2.0, 0.37, 1e-3, 2.0 ** -24)


def extreme_patterns(t):
    """(scale byte, quant byte) per constant row pattern: every pair of FILLS for the types with sub-block scales -- all-ones, all-zero, 0x80 and 0x7F bytes are the
    pairs (x, x); Q6_K's int8 scales at +127 (0x7F), -128 (0x80), -1, 0; the 6-bit scale / min pairs at 63 / 63 (0xFF); quants at each end -- and FILLS alone elsewhere."""
    return [(s, q) for s in FILLS for q in FILLS] if t in SCALE_BYTES else [(q, q) for q in FILLS]


def extreme_blocks(t, n_rows, K, seed):
    """raw bytes [n_rows][row_bytes]: row r is ONE constant pattern -- extreme_patterns(t)[r % P] in every block, |d| = EXTREME_D[(r // P) % 4] with the sign of d
    alternating from block to block (starting sign alternates with r), dmin / m of the same set (shifted by one), its sign alternating every two blocks.  The LAST row has one
    block (chosen by seed, never the first when there are several) of another pattern and another d among constant neighbours, so that a block-index error shows.
    F16 / F32: constant rows of +-30, +-0.37, +-1e-3, +- the smallest fp16 subnormal and 0, sign alternating every 32 weights on every other cycle."""
    rng = np.random.default_rng(_seed("extreme", t, n_rows, K, seed))
    if t in (F16, F32):
        vals = [30.0, -30.0, 0.37, -1e-3, 2.0 ** -24, -2.0 ** -24, 0.0]
        v = np.empty((n_rows, K))
        alt = np.where((np.arange(K) >> 5) & 1, -1.0, 1.0)
        for r in range(n_rows):
            v[r] = vals[r % len(vals)] * (alt if (r // len(vals)) & 1 else 1.0)
        if K >= 64:
            k0 = 32 * int(rng.integers(1, K // 32))
            v[n_rows - 1] = 0.37
            v[n_rows - 1, k0:k0 + 32] = -30.0
        return np.ascontiguousarray(v.astype(np.float16 if t == F16 else np.float32)).view(np.uint8).reshape(n_rows, -1)
    nb, bb = n_blocks(t, K), BLOCK[t][1]
    pats = extreme_patterns(t)
    P = len(pats)
    b = np.empty((n_rows, nb, bb), np.uint8)
    blk = np.arange(nb)
    dv = np.empty((2, n_rows, nb))
    for r in range(n_rows):
        sbyte, qbyte = pats[r % P]
        b[r] = qbyte
        if t in SCALE_BYTES:
            b[r, :, SCALE_BYTES[t][0]:SCALE_BYTES[t][1]] = sbyte
        c = r // P
        dv[0, r] = EXTREME_D[c % 4] * np.where((blk + r) & 1, -1.0, 1.0)
        dv[1, r] = EXTREME_D[(c + 1) % 4] * np.where(((blk >> 1) + c) & 1, -1.0, 1.0)
    r = n_rows - 1
    odd = int(rng.integers(1, nb)) if nb > 1 else 0
    b[r] = 0xFF
    dv[0, r], dv[1, r] = 0.37, 1e-3
    b[r, odd] = 0x00
    if t in SCALE_BYTES:
        b[r, odd, SCALE_BYTES[t][0]:SCALE_BYTES[t][1]] = 0x7F
    dv[0, r, odd], dv[1, r, odd] = -2.0, -2.0
    _set_fields(t, b, lambda i: dv[i])
    return b.reshape(n_rows, nb * bb)


GENERATORS = {"random": random_blocks, "extreme": extreme_blocks}
N_ACT = 9                                                       # rows of activation_rows


def activation_rows(t, K):
    """[N_ACT][K] float32 integer rows that the activation format of weight type t holds exactly.  k-quants (Q8_K, blocks of 256):
         0  all -128 (every 16-sum -2048, every 32-sum -4096)            1  integers in [-127, 127], -128 planted at a random place of every block
         2  alternating +127, -128                                       3  all +127 except the planted -128
         4  as 1 with an all-zero block in the middle                    5  zero except in its first block
         6..8  as 1, other draws
    32-element types, F16, F32 (Q8_0 / Q8_1, blocks of 32): the same rows with -127 for -128 and +-127 planted in every 32-block."""
    return _activation_rows(256 if t in K_TYPES else 32, K)


@functools.lru_cache(maxsize=None)
def _activation_rows(B, K):
    rng = np.random.default_rng(_seed("act", B, K))
    lo = -128 if B == 256 else -127
    nb = K // B

    def planted():
        x = rng.integers(-127, 128, K)
        at = np.arange(nb) * B + rng.integers(0, B, nb)
        x[at] = lo if B == 256 else np.where(rng.integers(0, 2, nb) == 1, 127, -127)
        return x
    x = np.empty((N_ACT, K), np.int64)
    x[0] = lo
    x[1] = planted()
    x[2] = np.where(np.arange(K) & 1, lo, 127)
    x[3] = 127
    x[3, np.arange(nb) * B + rng.integers(0, B, nb)] = lo
    x[4] = planted()
    x[4, (nb // 2) * B:(nb // 2 + 1) * B] = 0
    x[5] = 0
    x[5, :B] = planted()[:B]
    for i in range(6, N_ACT):
        x[i] = planted()
    out = x.astype(np.float32)
    out.setflags(write=False)
    return out


def act_rows(t, K, N, first=0):
    """N rows for a launch: activation_rows(t, K)[(first + i) % N_ACT]"""
    return np.ascontiguousarray(activation_rows(t, K)[(first + np.arange(N)) % N_ACT])


@functools.lru_cache(maxsize=None)
def blocks(gen, t, n_rows, K):
    """the generator's raw bytes for (type, rows, K) -- one draw per key, shared by the CPU and the GPU tests; read-only"""
    raw = GENERATORS[gen](t, n_rows, K, 0)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def reference(gen, t, n_rows, K):
    """-> (exact [N_ACT][n_rows], mag [N_ACT][n_rows]) float64 for activation_rows(t, K) against blocks(gen, t, n_rows, K): x . w and |x| . a.  Computed once, read-only."""
    w, a = decode(t, blocks(gen, t, n_rows, K), n_rows * K)
    x = activation_rows(t, K).astype(np.float64)
    exact, mag = x @ w.reshape(n_rows, K).T, np.abs(x) @ a.reshape(n_rows, K).T
    exact.setflags(write=False), mag.setflags(write=False)
    return exact, mag


def bound(mag, nb):
    return (nb + 4) * U * mag


def ratio_of(got, exact, mag, nb, residual=None):
    """max |got - exact| / bound over the outputs; inf where the bound is zero and got is not exactly zero (residual given: not exactly the residual).  residual: added by the
    kernel in one more fp32 addition -> 2^-24 of the result on top."""
    got = np.asarray(got, np.float64)
    bd = bound(mag, nb)
    want = exact
    if residual is not None:
        want = exact + residual
        bd = np.where(bd > 0, bd + U * (np.abs(want) + bd), 0.0)
    err = np.abs(got - want)
    if not np.isfinite(got).all():
        return float("inf")
    r = np.where(bd > 0, err / np.where(bd > 0, bd, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(r.max())


def ratio(got, x, w, a, nb, residual=None):
    """got [N][R] against rows x [N][K], decoded weights w / a [R][K] (float64), nb blocks along K"""
    x = np.asarray(x, np.float64)
    return ratio_of(got, x @ w.T, np.abs(x) @ a.T, nb, residual)


def rows_index(N, first=0):
    return (first + np.arange(N)) % N_ACT


# ---- mutants: one decoding step done wrongly; tests/test_cpu_quant_blocks.py requires the inputs to push every one of them past the bound --------------------------------
MUTANTS = {
    "k4_high_bits_ignored": (Q4_K, Q5_K),                       # the 6-bit scale / min unpack drops the high bits of sub-blocks 4..7
    "q5_high_bit_neighbour": (Q5_0, Q5_1, Q5_K),                # the fifth bit taken from the neighbouring bit position
    "q6_high_bits_shifted": (Q6_K,),                            # Q6_K's high two bits taken one pair further
    "d_sign_dropped": (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K),
    "q6_scales_unsigned": (Q6_K,),                              # the int8 scales read as unsigned
    "dmin_read_as_d": (Q2_K, Q4_K, Q5_K),
    "nibbles_swapped": (Q4_0, Q4_1, Q5_0, Q5_1, Q2_K, Q4_K, Q5_K, Q6_K),   # Q2_K: the scale and the min nibble of a scale byte
    "bsum32_high_digit_clamped": (Q4_K, Q5_K),                  # the min term on bsum32 = 128 hi + lo with hi kept to +-31: wrong exactly where a 32-sum is below -3968 (-4096)
}


def mutants_of(t):
    return [m for m, types in MUTANTS.items() if t in types]


def mutant_product(mutant, gen, t, n_rows, K):
    """[N_ACT][n_rows] float64: what a kernel with that one step wrong would compute (exact arithmetic otherwise)"""
    raw = blocks(gen, t, n_rows, K)
    x = activation_rows(t, K).astype(np.float64)
    if mutant == "bsum32_high_digit_clamped":
        p, off, m = _parts(t, raw, n_rows * K)
        bs = x.reshape(N_ACT, K // 32, 32).sum(axis=2).astype(np.int64)
        hi, lo = np.clip(bs >> 7, -31, 31), bs & 127                                  # MUTANT: the digit split's high digit cannot hold -32
        m32 = m.reshape(n_rows, K // 32, 32)[:, :, 0]                                 # dmin * m is constant over a sub-block
        return x @ (p - off).reshape(n_rows, K).T - (128 * hi + lo).astype(np.float64) @ m32.T
    w, _ = decode(t, raw, n_rows * K, mutant)
    return x @ w.reshape(n_rows, K).T


# ---- the cases: tests/test_gpu_quant_blocks.py runs them on the device, tests/test_cpu_quant_blocks.py holds the oracle (and the mutants) to the same inputs ------------------
Q32_TYPES = [Q4_0, Q4_1, Q5_0, Q5_1, Q8_0]
MUL_MAT_CASES = ([(t, 3, 512, 96) for t in ALL_TYPES] + [(t, 33, 1024, 70) for t in ALL_TYPES]             # (type, N, K, n_out); N >= 16: the MFMA route
                 + [(t, 5, 352, 100) for t in Q32_TYPES])                                                   # the ViT's row length: 11 blocks of 32
MMQ2_TYPES = [Q4_K, Q5_K, Q6_K, Q4_0]
MMQ2_SHAPES = [(31, 256, 32, 1, 0, False), (33, 1024, 130, 2, 0, False), (40, 2048, 64, 1, 2, True)]        # N, K, n_out, n_mat, ks, residual
MATVEC_TYPES = [Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q4_K, Q5_K, Q6_K, F16]                                        # the types of test_gpu_parity.MATVEC_CASES
MATVEC_SHAPES = [(t, K, 130) for t in MATVEC_TYPES for K in (512, 5120)] + [(Q5_K, 13824, 64), (Q6_K, 13824, 64)]   # type, K, rows per matrix
MATVEC_MIX_SHAPES = [(ta, K, 130) for ta in (Q4_K, Q5_K) for K in (512, 5120)]                              # two of ta + one Q6_K in one launch
ROWS_TYPES = [Q4_0, Q4_1, Q5_0, Q5_1, Q4_K, Q5_K, Q6_K]                                                     # what k_matvec_tn is built for
ROWS_SHAPES = [(t, K, 130) for t in ROWS_TYPES for K in (512, 5120)]
RI_TYPES = [Q4_K, Q5_K, Q6_K]
# rows 128 = two 64-row groups; K = 5120 with so few groups makes the launcher split K over workgroups (ri_ksplit: fewer groups than half the CUs, at least 16 super-blocks);
# (4096, 64) is the smallest such shape: one group, 16 super-blocks -> 2 parts of 8; K = 512 cannot split.  The mixed launch never splits.
RI_SHAPES = [(t, K, rows) for t in RI_TYPES for (K, rows) in ((512, 128), (5120, 128), (4096, 64))]
RI_MIX_SHAPES = [(ta, K, 128) for ta in (Q4_K, Q5_K) for K in (512, 5120)]
GET_ROWS_CASES = [(t, K) for t in ALL_TYPES for K in (256, 1280)]
GET_ROWS_TABLE, GET_ROWS_TOKENS = 7, [6, 0, -1, 3, 3]


def weight_sets():
    """every (type, rows, K) that a mat-mul / mat-vec case multiplies (matrices of one launch back to back), without repeats, in a fixed order"""
    out = []

    def add(t, rows, K):
        if (t, rows, K) not in out:
            out.append((t, rows, K))
    for t, N, K, R in MUL_MAT_CASES:
        add(t, R, K)
    for t in MMQ2_TYPES:
        for N, K, R, n_mat, ks, res in MMQ2_SHAPES:
            add(t, n_mat * R, K)
    for t, K, R in MATVEC_SHAPES + ROWS_SHAPES:
        add(t, 3 * R, K)                                        # the three-matrix launch; the one-matrix launch takes its first R rows
    for ta, K, R in MATVEC_MIX_SHAPES:
        add(ta, 3 * R, K), add(Q6_K, 3 * R, K)                  # two matrices of ta (the first 2 R rows of the set) + one of Q6_K (its first R rows)
    for t, K, R in RI_SHAPES:
        add(t, 3 * R, K)
    for ta, K, R in RI_MIX_SHAPES:
        add(ta, 3 * R, K), add(Q6_K, 3 * R, K)
    return out
