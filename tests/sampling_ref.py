"""Reference of the device-side sampling rule (include/minigpt4_amd.h), independent of the library: Philox4x32-10 restated in NumPy, the transformed row (bias, penalties,
constraint) in NumPy fp32 -- single fp32 operations, so the bits match the kernel's --, the candidate order by lexsort, and the rule's steps 1 to 4 in float64."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
PEN_REP, PEN_ALPHA, PEN_KEEP_NL, PEN_NL = 1, 2, 4, 13
EOS = 2
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (anything that converts to uint64 arrays of 32-bit words) -> uint32 [..., 4]"""
    c = [np.asarray(counter, np.uint64)[..., i] & MASK for i in range(4)]
    k = [np.asarray(key, np.uint64)[..., i] & MASK for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, -1).astype(np.uint32)


def draw_word(seed, draws):
    """output word 0 for (seed, draws), Python integers below 2^64"""
    return int(philox4x32_10([draws & MASK, draws >> 32, 0, 0], [seed & MASK, seed >> 32])[0])


def pen_row(flags=0, repeat_penalty=1.0, alpha_frequency=0.0, alpha_presence=0.0):
    return dict(flags=flags, repeat_penalty=np.float32(repeat_penalty), alpha_frequency=np.float32(alpha_frequency), alpha_presence=np.float32(alpha_presence))


def transformed(row, table, pen):
    """steps 1 to 5 of the penalties on a copy of `row` (fp32): table = [(id, count, bias, has_bias)], pen = pen_row(...)"""
    out = np.array(row, np.float32)
    for tid, count, bias, has_bias in table:
        l = np.float32(row[tid])
        if has_bias:
            l = np.float32(l + np.float32(bias))
        if count > 0 and not ((pen["flags"] & PEN_KEEP_NL) and tid == PEN_NL):
            if pen["flags"] & PEN_REP:
                l = np.float32(l * pen["repeat_penalty"]) if l <= 0 else np.float32(l / pen["repeat_penalty"])
            if pen["flags"] & PEN_ALPHA:
                t = np.float32(np.float32(count) * pen["alpha_frequency"])
                t = np.float32(t + pen["alpha_presence"])
                l = np.float32(l - t)
        out[tid] = l
    return out


def bitmap_ids(bitmap, n_vocab):
    b = np.asarray(bitmap, np.uint32)
    i = np.arange(n_vocab)
    return np.nonzero((b[i >> 5] >> (i & 31).astype(np.uint32)) & np.uint32(1))[0]


def make_bitmap(n_vocab, ids):
    w = ((n_vocab + 31) // 32 + 3) // 4 * 4
    b = np.zeros(w, np.uint32)
    for i in ids:
        b[i >> 5] |= np.uint32(1 << (i & 31))
    return b


def candidates(trow, top_k, allowed_ids=None):
    """(ids, values) of the first min(top_k, participating ids): value descending, equal values by ascending id"""
    ids = np.arange(len(trow)) if allowed_ids is None else np.asarray(allowed_ids, np.int64)
    vals = trow[ids]
    with np.errstate(invalid="ignore"):
        order = np.lexsort((ids, -vals))[:top_k]
    return ids[order].astype(np.int32), vals[order].astype(np.float32)


def rule64(v, temp, top_p, word, kept=None):
    """steps 1 to 4 in float64 on the fp32 candidate values (temp / top_p as the fp32 values the library takes).  dict(kept, c: the cumulative q of step 1 (None when
    top_p >= 1), p [kept], cum: S_j / S, u, pick); kept given: step 1 is skipped and that value used."""
    v = np.asarray(v, np.float64)
    temp, top_p = float(np.float32(temp)), float(np.float32(top_p))
    n_c, c = len(v), None
    with np.errstate(invalid="ignore"):
        if top_p < 1.0:
            a = np.exp(v - v[0])
            c = np.cumsum(a / a.sum())
            hit = np.nonzero(c >= top_p)[0]
            k1 = int(hit[0]) + 1 if len(hit) else n_c
        else:
            k1 = n_c
        kept = k1 if kept is None else kept
        w = v[:kept] / temp
        b = np.exp(w - w[0])
    S = np.cumsum(b)
    u = float(word >> 8) * 2.0 ** -24
    above = np.nonzero(S > u * S[-1])[0]
    return dict(kept=k1, c=c, p=b / S[-1], cum=S / S[-1], u=u, pick=int(above[0]) if len(above) else kept - 1)
