"""The activation preparation of the language model, stated from the rule (numpy, no GPU): what launch_rms_quant / launch_silu_mul_quant and the consumers of a deferred
split-K combine must write into each of an ActQ's thirteen planes, and the inputs that reach the rule's decision points.

The rule (ggml's quantize_row_q8_K / q8_0 / q8_1 and rms_norm, as csrc/row_prep.hpp and csrc/common.hpp state them):
  Q8_K   per 256: the FIRST element of largest magnitude, sign included, is `max`; iscale = -128 / max (fp32); q = min(127, round-half-even(iscale * x)); d = 1 / iscale;
         sums per 16 (bsk); an all-zero block: d = 0, q = 0.  Per-32 sums s as two digits: lo = s mod 128 in 0 .. 127, hi = floor(s / 128) (bsq int8, bs16 fp16).
         q16: the int8 values as fp16 in the fragment order documented at ActQ.
  Q8_0/1 per 32: d = amax / 127, id = 1 / d or 0, q = round-half-even(x * id); d0 = d through fp16, d1 = d, s1 = d * (float)sum, sum0 = sum.
  xh = round-to-nearest-even fp16, xf = the values.
  values (x * scale) * w, scale = 1 / sqrtf((float)(S / K) + 1e-6f), S = the sum of the fp32-rounded squares -- computed EXACTLY here (math.fsum); or table[fp16(a)] * b.
  slabs  ((slab_0 + slab_1) + ... + slab_{ks-1}) + residual, every addition rounded to fp32.
Every function takes `wrong`: the name of ONE deliberately wrong rule (WRONG_RULES), for tests/test_cpu_act_ref.py's proof that the inputs reach the edge that rule governs."""
import functools
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24
ACT_Q8K, ACT_Q80, ACT_F16, ACT_F32 = 1, 2, 4, 8
PLANE_BSQ, PLANE_BS16, PLANE_Q16 = 1, 2, 4
PLANES = ("q8k", "dk", "bsk", "bsq", "bs16", "q16", "q80", "d0", "d1", "s1", "sum0", "xh", "xf")
# wrong rule -> the planes in which it must show
WRONG_RULES = {"last_max_wins": ("q8k", "dk"), "sign_from_abs_max": ("q8k", "dk"), "no_clamp": ("q8k", "bsk"), "round_half_away": ("q8k", "q80"), "hi_trunc": ("bsq", "bs16"),
               "lo_from_abs": ("bsq", "bs16"), "d0_unrounded": ("d0",), "s1_unrounded_sum": ("s1",), "slab_reverse": ("sum",), "residual_first": ("sum",)}


# ---------------------------------------------------------------------------------------------------------------- quantisers
def _round(p, wrong):
    """fp32 products -> integers: half to even (rintf); the wrong rule rounds half away from zero"""
    if wrong == "round_half_away":
        p64 = p.astype(np.float64)
        return (np.sign(p64) * np.floor(np.abs(p64) + 0.5)).astype(np.int64)
    return np.rint(p).astype(np.int64)


def _q16_order():
    """chunk c = 8 p + 4 uu + d of a super-block holds elements 64 p + 16 uu + 4 d + {0, 2, 1, 3} and the same + 32 (ActQ in csrc/common.hpp)"""
    idx = np.empty((32, 8), np.int64)
    for c in range(32):
        e0 = 64 * (c >> 3) + 16 * ((c >> 2) & 1) + 4 * (c & 3)
        idx[c] = [e0, e0 + 2, e0 + 1, e0 + 3, e0 + 32, e0 + 34, e0 + 33, e0 + 35]
    return idx.reshape(-1)


Q16_ORDER = _q16_order()


def q8k_planes(v, wrong=None):
    """v [N][K] fp32, K % 256 == 0 -> {q8k, dk, bsk, bsq, bs16, q16} of N rows"""
    N, K = v.shape
    x = np.ascontiguousarray(v, F32).reshape(-1, 256)
    nb = x.shape[0]
    ax = np.abs(x)
    amax = ax.max(axis=1)
    first = np.argmax(ax == amax[:, None], axis=1)
    if wrong == "last_max_wins":
        first = 255 - np.argmax((ax == amax[:, None])[:, ::-1], axis=1)
    mx = x[np.arange(nb), first]
    if wrong == "sign_from_abs_max":
        mx = np.abs(mx)
    live = amax != 0
    iscale = (F32(-128.0) / np.where(live, mx, F32(1.0))).astype(F32)
    r = _round((iscale[:, None] * x).astype(F32), wrong)
    q = r if wrong == "no_clamp" else np.minimum(r, 127)
    q = np.where(live[:, None], q, 0)
    d = np.where(live, (F32(1.0) / iscale).astype(F32), F32(0.0)).astype(F32)
    s32 = q.reshape(nb, 8, 32).sum(axis=2)
    lo, hi = np.mod(s32, 128), np.floor_divide(s32, 128)
    if wrong == "hi_trunc":
        hi = np.trunc(s32 / 128.0).astype(np.int64)
    if wrong == "lo_from_abs":
        lo = np.abs(s32) & 127
    digits = np.concatenate([lo, hi], axis=1)
    return {"q8k": q.astype(np.int8).reshape(N, K), "dk": d.reshape(N, K // 256), "bsk": q.reshape(nb, 16, 16).sum(axis=2).astype(np.int16).reshape(N, K // 16),
            "bsq": digits.astype(np.int8).reshape(N, K // 256, 16), "bs16": digits.astype(np.float16).view(np.uint16).reshape(N, K // 256, 16),
            "q16": q[:, Q16_ORDER].astype(np.float16).view(np.uint16).reshape(N, K)}


def q80_planes(v, wrong=None):
    """v [N][K] fp32, K % 32 == 0 -> {q80, d0, d1, s1, sum0} of N rows"""
    N, K = v.shape
    x = np.ascontiguousarray(v, F32).reshape(-1, 32)
    d = (np.abs(x).max(axis=1) / F32(127.0)).astype(F32)
    inv = np.where(d != 0, F32(1.0) / np.where(d != 0, d, F32(1.0)), F32(0.0)).astype(F32)
    p = (x * inv[:, None]).astype(F32)
    q = _round(p, wrong)
    s = q.sum(axis=1)
    sf = s.astype(F32)
    if wrong == "s1_unrounded_sum":
        sf = p.astype(np.float64).sum(axis=1).astype(F32)
    d0 = d if wrong == "d0_unrounded" else d.astype(np.float16).astype(F32)
    nb = K // 32
    return {"q80": q.astype(np.int8).reshape(N, K), "d0": d0.reshape(N, nb), "d1": d.reshape(N, nb), "s1": (d * sf).astype(F32).reshape(N, nb), "sum0": s.astype(np.int32).reshape(N, nb)}


def planes(v, mask, optional=PLANE_BSQ | PLANE_BS16 | PLANE_Q16, wrong=None):
    """every plane a launch with `mask` and the optional planes `optional` writes for the prepared values v [N][K]: name -> N rows (fp16 planes as uint16 bit patterns)"""
    v = np.ascontiguousarray(v, F32)
    out = {}
    if mask & ACT_Q8K:
        k = q8k_planes(v, wrong)
        if not optional & PLANE_BSQ:
            del k["bsq"], k["bs16"]                                   # bs16 is written next to bsq only
        elif not optional & PLANE_BS16:
            del k["bs16"]
        if not optional & PLANE_Q16:
            del k["q16"]
        out.update(k)
    if mask & ACT_Q80:
        out.update(q80_planes(v, wrong))
    if mask & ACT_F16:
        with np.errstate(over="ignore"):
            out["xh"] = v.astype(np.float16).view(np.uint16)
    if mask & ACT_F32:
        out["xf"] = v
    return out


# ---------------------------------------------------------------------------------------------------------------- prepared values
def sum_squares(row):
    """S: the exact sum of the fp32-rounded squares (a double holds an fp32 square exactly)"""
    r = np.ascontiguousarray(row, F32)
    return math.fsum((r * r).astype(np.float64).tolist())


def rms_mean(row):
    """((float)(S / K), ambiguous): ambiguous when S (1 +- K 2^-52) / K lands on two different floats -- a parallel double sum and the sequential one may then differ"""
    K = row.shape[0]
    S = sum_squares(row)
    e = K * 2.0 ** -52
    return F32(S / K), F32(S * (1.0 - e) / K) != F32(S * (1.0 + e) / K)


def rms_scale(row):
    return F32(1.0) / np.sqrt(F32(rms_mean(row)[0] + F32(1e-6)))


def rms_values(x, w):
    """(x * scale) * w, every product rounded to fp32; w None: the rows as they are"""
    x = np.ascontiguousarray(x, F32)
    if w is None:
        return x
    scale = np.array([rms_scale(r) for r in x], F32)
    return ((x * scale[:, None]).astype(F32) * np.ascontiguousarray(w, F32)[None, :]).astype(F32)


def silu_values(a, b, table):
    """table[fp16(a)] * b with table = 65536 fp16 bit patterns; b None: the rows as they are"""
    a = np.ascontiguousarray(a, F32)
    if b is None:
        return a
    with np.errstate(over="ignore"):
        bits = a.astype(np.float16).view(np.uint16)
        return (np.ascontiguousarray(table).view(np.float16)[bits].astype(F32) * np.ascontiguousarray(b, F32)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- slab sums
def slab_sum32(slabs, residual=None, wrong=None):
    """slabs [ks][...] fp32 -> ((slab_0 + slab_1) + ... ) + residual, every addition rounded to fp32"""
    s = np.ascontiguousarray(slabs, F32)
    order = list(range(s.shape[0]))[::-1] if wrong == "slab_reverse" else list(range(s.shape[0]))
    terms = [s[z] for z in order]
    if residual is not None:
        r = np.ascontiguousarray(residual, F32).reshape(s.shape[1:])
        terms = [r] + terms if wrong == "residual_first" else terms + [r]
    acc = terms[0]
    for t in terms[1:]:
        acc = (acc + t).astype(F32)
    return acc


def slab_sum64(slabs, residual=None):
    """(the float64 sum, the bound (ks + 1) * 2^-24 * sum |terms| on what an fp32 sum in any order may differ from it)"""
    s = np.ascontiguousarray(slabs, F32).astype(np.float64)
    tot, mag = s.sum(axis=0), np.abs(s).sum(axis=0)
    if residual is not None:
        r = np.ascontiguousarray(residual, F32).astype(np.float64).reshape(tot.shape)
        tot, mag = tot + r, mag + np.abs(r)
    return tot, (s.shape[0] + 1) * U * mag


def bound_ratio(got, slabs, residual=None):
    """largest |got - float64 sum| / bound; a zero bound admits only the exact value"""
    tot, bound = slab_sum64(slabs, residual)
    err = np.abs(np.asarray(got, np.float64).reshape(tot.shape) - tot)
    if not np.isfinite(err).all() or (err[bound == 0] != 0).any():
        return float("inf")
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


# ---------------------------------------------------------------------------------------------------------------- inputs
K_Q8K = (256, 1024, 4096, 4352, 5120, 11008, 13824)
K_32 = K_Q8K + (32, 352, 1408)
NS = (1, 3, 5)
MASKS = (ACT_Q8K, ACT_Q80, ACT_F16, ACT_F32, ACT_Q8K | ACT_Q80, 15)
OPTIONALS = (0, PLANE_BSQ, PLANE_BSQ | PLANE_BS16 | PLANE_Q16)
SUMS_A = (-4096, -129, -128, -127, -1, 0, 1, 127)
SUMS_B = (128, 4064, -129, 0, 1, -1, 127, -128)
FAMILIES = ("gauss", "zero", "negzero", "negmax", "tie_pn", "tie_np", "tie_thread_pn", "tie_thread_np", "tie_lane0_63_pn", "tie_lane0_63_np", "tie_last_elem", "half_k",
            "half_80", "int_a", "int_b", "tiny", "big", "last_only")
ROW_ZERO, ROW_LAST = -1, -2                                      # layout codes of the two row-level families: an all-zero row, a single non-zero at element K - 1


def _sub32(rng, total):
    """32 integers in [-128, 127] whose sum is `total`"""
    if total == -4096:
        return np.full(32, -128, np.int64)
    if total == 4064:
        return np.full(32, 127, np.int64)
    x = rng.integers(-3, 4, 32)
    x[:3] = 0
    lead = {-129: (-128, -1), 128: (127, 1), -128: (-128, 0), 127: (127, 0), -127: (-127, 0)}.get(total, (total, 0))
    x[0], x[1] = lead
    x[2] = total - x.sum()
    assert x.sum() == total and np.abs(x).max() <= 128 and x.max() <= 127
    return rng.permutation(x) if total not in (-129, -128) else x    # (the -128 stays in front: the block's first maximum)


def _block(name, rng):
    """one 256-block of family `name` (fp32)"""
    m = F32(rng.uniform(0.5, 3.0))
    base = np.clip(rng.standard_normal(256) * 0.3 * m, -0.9 * m, 0.9 * m).astype(F32)

    def tie(i, vi, j, vj):
        x = base.copy()
        x[i], x[j] = vi, vj
        return x
    if name == "gauss":
        return (rng.standard_normal(256) * 0.7).astype(F32)
    if name == "zero":
        return np.zeros(256, F32)
    if name == "negzero":
        return np.full(256, -0.0, F32)
    if name == "negmax":
        return tie(int(rng.integers(0, 256)), -m, int(rng.integers(0, 256)), -m)
    if name in ("tie_pn", "tie_np"):                             # two lanes, the first wins; the second then lands on +128 and is clamped to 127
        i, j = int(rng.integers(0, 120)), int(rng.integers(128, 256))
        return tie(i, m if name == "tie_pn" else -m, j, -m if name == "tie_pn" else m)
    if name in ("tie_thread_pn", "tie_thread_np"):               # inside one thread's four elements
        t = int(rng.integers(0, 64))
        return tie(4 * t + 1, m if name == "tie_thread_pn" else -m, 4 * t + 3, -m if name == "tie_thread_pn" else m)
    if name in ("tie_lane0_63_pn", "tie_lane0_63_np"):
        return tie(2, m if name == "tie_lane0_63_pn" else -m, 253, -m if name == "tie_lane0_63_pn" else m)
    if name == "tie_last_elem":                                  # the partner of the tie is the last element of the last 32-block
        return tie(100, -m, 255, m)
    if name == "half_k":                                         # -128 makes iscale 1: the values k + 0.5 ARE the products; 127.5 rounds to 128 and is clamped
        k = rng.integers(-128, 128, 256).astype(np.float64) + 0.5
        k[rng.permutation(256)[:8]] = [127.5, -127.5, 126.5, 0.5, -0.5, 1.5, 2.5, -2.5]
        k[int(rng.integers(1, 256))] = -128.0
        return k.astype(F32)
    if name == "half_80":                                        # per 32: amax = 127 makes id 1
        k = rng.integers(-127, 127, 256).astype(np.float64) + 0.5
        k[np.arange(8) * 32 + rng.integers(0, 32, 8)] = np.where(rng.integers(0, 2, 8) == 1, 127.0, -127.0)
        return k.astype(F32)
    if name in ("int_a", "int_b"):                               # integers with -128 as the first maximum: iscale 1, the per-32 sums are SUMS_A / SUMS_B
        return np.concatenate([_sub32(rng, s) for s in (SUMS_A if name == "int_a" else SUMS_B)]).astype(F32)
    if name == "tiny":                                           # amax / 127 stays a normal fp32; d0 underflows to 0 in fp16
        return (np.where(rng.integers(0, 2, 256) == 1, 1.0, -1.0) * rng.uniform(0.25, 1.0, 256) * 1e-30).astype(F32)
    if name == "big":
        x = rng.uniform(-3e4, 3e4, 256)
        x[int(rng.integers(0, 256))] = -3e4
        return x.astype(F32)
    if name == "last_only":
        x = np.zeros(256, F32)
        x[255] = m
        return x
    raise KeyError(name)


def _shift(K, r):
    return 3 * K_32.index(K) + (0, 5, 10, 3, 8, 13, 16, 1)[r]


@functools.lru_cache(maxsize=None)
def _pool_row(K, r):
    """row r of K's pool: 256-blocks whose families step through FAMILIES from a (K, r)-dependent start (so neighbours in FAMILIES -- tiny | big -- are neighbouring blocks);
    a K that is no multiple of 256 takes the first K elements"""
    rng = np.random.default_rng([20240607, K, r])
    nb = (K + 255) // 256
    fam = (np.arange(nb) + _shift(K, r)) % len(FAMILIES)
    x = np.concatenate([_block(FAMILIES[f], rng) for f in fam])[:K]
    x.setflags(write=False)
    return x, tuple(int(f) for f in fam)


@functools.lru_cache(maxsize=None)
def rows(K, N):
    """(x [N][K] fp32, layout [N] of per-block family indices or ROW_ZERO / ROW_LAST).  N = 3 and 5 carry the row-level families between live rows."""
    plan = {1: (0,), 3: (1, ROW_ZERO, 2), 5: (3, ROW_LAST, 4, ROW_ZERO, 5)}[N]
    x, layout = np.zeros((N, K), F32), []
    for i, r in enumerate(plan):
        if r == ROW_LAST:
            x[i, K - 1] = F32(-1.75)
        elif r != ROW_ZERO:
            x[i] = _pool_row(K, r)[0]
        layout.append(r if r < 0 else _pool_row(K, r)[1])
    x.setflags(write=False)
    return x, tuple(layout)


@functools.lru_cache(maxsize=None)
def norm_weight(K):
    w = (1.0 + 0.25 * np.random.default_rng([20240608, K]).standard_normal(K)).astype(F32)
    w.setflags(write=False)
    return w


FINITE_BITS = np.array([b for b in range(65536) if (b & 0x7C00) != 0x7C00], np.uint16)


@functools.lru_cache(maxsize=None)
def silu_operands(K, N):
    """(a, b) [N][K]: a = fp16-exact values drawn from the finite bit patterns, with fp32 values ON an fp16 rounding boundary (the midpoint of two neighbouring finite fp16
    values: a tie) or one fp32 step to either side of it among them -- every 5th element, or, once N * K exceeds 63 488, the elements behind one copy of every pattern.
    b Gaussian around 1."""
    rng = np.random.default_rng([20240609, K, N])
    n = N * K
    bits = np.resize(rng.permutation(FINITE_BITS), n)
    a = bits.view(np.float16).astype(F32)
    at = np.arange(2, n, 5) if n <= FINITE_BITS.size else np.arange(FINITE_BITS.size, n)                 # (when there is room behind all 63 488 patterns, they all stay)
    h = rng.permutation(FINITE_BITS[(FINITE_BITS & 0x7FFF) < 0x7BFF])
    h = np.resize(h, at.size)
    mid = ((h.view(np.float16).astype(np.float64) + (h + np.uint16(1)).view(np.float16).astype(np.float64)) / 2).astype(F32)
    side = rng.integers(0, 3, at.size)
    mid = np.where(side == 1, np.nextafter(mid, F32(np.inf)), np.where(side == 2, np.nextafter(mid, F32(-np.inf)), mid)).astype(F32)
    a[at] = mid
    b = (1.0 + 0.2 * rng.standard_normal(n)).astype(F32)
    a, b = a.reshape(N, K), b.reshape(N, K)
    a.setflags(write=False), b.setflags(write=False)
    return a, b


KS = (2, 3, 8)
MIXED_KS = ((2, 2, 1), (3, 3, 2), (2, 2, 2))
SLAB_SHAPES = ((1, 256), (3, 4352), (5, 5120))                   # (N, K) of the slab consumers' cases: one block; ragged against 4096 and 1024; the second loop pass


def slab_stride(n):
    """a slab of n values and 64 floats of padding (NaN) behind them"""
    return n + 64


@functools.lru_cache(maxsize=None)
def slab_case(ks, n, stride, tag=0):
    """(slabs [ks][stride], residual [n]): the first ks - 1 slabs hold terms of +-1e4, the last one their negated sum plus an O(1) value -- the sums are O(1) and another
    order of the additions changes their bits; NaN in the padding behind n"""
    rng = np.random.default_rng([20240610, ks, n, stride, tag])
    s = np.empty((ks, stride), F32)
    s[:ks - 1, :n] = (rng.uniform(0.2, 1.0, (ks - 1, n)) * 1e4 * np.where(rng.integers(0, 2, (ks - 1, n)) == 1, 1.0, -1.0)).astype(F32)
    s[ks - 1, :n] = (rng.standard_normal(n) * 0.7 - s[:ks - 1, :n].astype(np.float64).sum(axis=0)).astype(F32)
    s[:, n:] = np.nan
    res = (rng.standard_normal(n) * 0.7).astype(F32)
    s.setflags(write=False), res.setflags(write=False)
    return s, res
