"""Reference of the extended device-side sampling rule (include/minigpt4_amd.h: tail-free -> typical -> top-p -> min-p -> temperature -> softmax -> draw over the live
list, or mirostat v2 behind top-k), independent of the library: float64 throughout, on the fp32 candidate values, with the parameters as the fp32 values the library takes.
Every stage returns what it compared with its threshold -- the cumulative sums, the typicality scores, the surprises -- so a test can see how close a decision was, and
takes the decision from outside (`force`) so the rule can be continued from the library's outcome where the reference says it was too close to call."""
import numpy as np


def f32(x):
    return float(np.float32(x))


def softmax64(v):
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.exp(np.asarray(v, np.float64) - float(v[0]))
    return a / a.sum()


def tail_free64(v, z, cut=None):
    """dict(ran, s: the sum of |second differences|, c: the cumulative normalised ones (c[i] is compared with z at i >= 1), cut: the new length)"""
    m = len(v)
    if not (z < 1.0 and m > 2):
        return dict(ran=False, s=None, c=None, cut=m)
    q = softmax64(v)
    d2 = np.abs(np.diff(np.diff(q)))                                # |d1_i - d1_{i+1}|, d1_i = q_i - q_{i+1}
    s = float(d2.sum())
    d2 = d2 / s if s > 1e-6 else np.full(m - 2, 1.0 / (m - 2))
    c = np.cumsum(d2)
    hit = [i for i in range(1, m - 2) if c[i] > z]
    return dict(ran=True, s=s, c=c, cut=(hit[0] if hit else m) if cut is None else cut)


def typical64(v, p, order=None, t=None):
    """dict(ran, H, sh: the typicality scores, order: positions by score ascending (stable), c: the cumulative q in that order, t: how many are kept, keep: their
    positions back in value order)"""
    m = len(v)
    if not p < 1.0:
        return dict(ran=False, keep=np.arange(m), t=m)
    q = softmax64(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        lq = np.where(q > 0, np.log(np.where(q > 0, q, 1.0)), -np.inf)
        H = float(np.sum(np.where(q > 0, -q * lq, 0.0)))
        sh = np.where(q > 0, np.abs(-lq - H), np.inf)
    order = np.argsort(sh, kind="stable") if order is None else np.asarray(order)
    c = np.cumsum(q[order])
    hit = np.nonzero(c > p)[0]
    t = (int(hit[0]) + 1 if len(hit) else m) if t is None else t
    return dict(ran=True, H=H, q=q, sh=sh, order=order, c=c, t=t, keep=np.sort(order[:t]))


def top_p64(v, top_p, kept=None):
    m = len(v)
    if not top_p < 1.0:
        return dict(ran=False, c=None, kept=m)
    c = np.cumsum(softmax64(v))
    hit = np.nonzero(c >= top_p)[0]
    return dict(ran=True, c=c, kept=(int(hit[0]) + 1 if len(hit) else m) if kept is None else kept)


def min_p64(v, min_p, kept=None):
    """dict(ran, ratio: q_j / q_first (compared with min_p), kept)"""
    m = len(v)
    if not min_p > 0.0:
        return dict(ran=False, ratio=None, kept=m)
    q = softmax64(v)
    with np.errstate(invalid="ignore"):
        ratio = q / q[0]
    below = np.nonzero(~(ratio >= min_p))[0]
    below = below[below >= 1]
    return dict(ran=True, ratio=ratio, kept=(int(below[0]) if len(below) else m) if kept is None else kept)


def draw64(b, word):
    """the draw over the unnormalised b: dict(p, cum: S_j / S, u, at: the first position whose running sum exceeds u * S, the last if none)"""
    S = np.cumsum(b)
    u = float(word >> 8) * 2.0 ** -24
    above = np.nonzero(S > u * S[-1])[0]
    return dict(p=b / S[-1], cum=S / S[-1], u=u, at=int(above[0]) if len(above) else len(b) - 1)


# ---- how close is too close.  The p_j bound of tests/test_gpu_device_sampling.py, REL = 2e-4 relative, stands on an estimated error E = 4e-5 of an fp32 softmax entry
# (argument of expf, the 64-term sum, expf itself); its own margin for a cumulative sum of such entries against top_p is MARGIN = 1e-4 > E * 1 + 4e-6.  From the same E:
#   cumulative q against top_p / typical_p           MARGIN, unchanged: the sums are of the same kind
#   tail-free: d2_i = |q_i - 2 q_{i+1} + q_{i+2}| is off by at most 4 E max(q) each, their cumulative sum and s by at most 4 E sum(q) = 4 E; the normalised cumulative
#     sum c = (partial sum) / s therefore by at most (4 E + c 4 E) / s <= 8 E / s = 3.2e-4 / s -- it scales with 1 / s, so the tests choose peaked rows (s >= 0.3)
#   typicality scores sh_j = |-log q_j - H|: log q_j is off by E, H = sum -q log q by at most E (H + 1) <= 5.2 E (H <= log 64), so a score by 6.2 E and the
#     difference of two scores by 12.4 E: two scores closer than SH_MARGIN = 5e-4 may come out in either order
#   min-p: q_j / q_first is off by 2 E relative, the product min_p * q_first by one rounding: relative MINP_REL = 1e-4
#   mirostat: s_j = -log2 p_j is off by E / ln 2 = 5.8e-5 plus log2f's own few ulp of a value below 128 (about 3e-5): S_MARGIN = 1e-4
# A decision is too close when moving its threshold by the margin either way (or swapping two such scores) changes its outcome; every outcome reached that way is
# admissible, and the reference continues from each of them, so a close call early in the chain is followed through the later filters.
REL, E, MARGIN, SH_MARGIN, MINP_REL, S_MARGIN = 2e-4, 4e-5, 1e-4, 5e-4, 1e-4, 1e-4


def _first(c, thr, strict, start=0):
    for i in range(start, len(c)):
        if (c[i] > thr) if strict else (c[i] >= thr):
            return i
    return None


def admissible_lists(v, top_p, tfs_z=1.0, typical_p=1.0, min_p=0.0):
    """every live list (tuple of candidate indices) the filters may end with, given the margins above; one entry: no decision was close"""
    v = np.asarray(v, np.float64)
    top_p, tfs_z, typical_p, min_p = f32(top_p), f32(tfs_z), f32(typical_p), f32(min_p)
    lists = {tuple(range(len(v)))}

    def step(lists, alts):
        return {tuple(L[i] for i in keep) for L in lists for keep in alts(v[list(L)])}

    def tfs_alts(x):
        r = tail_free64(x, tfs_z)
        if not r["ran"]:
            return [range(len(x))]
        mg = 8 * E / r["s"] if r["s"] > 1e-6 else MARGIN
        cuts = {_first(r["c"], tfs_z + d, True, 1) for d in (-mg, 0.0, mg)}
        return [range(len(x) if c is None else c) for c in cuts]

    def typ_alts(x):
        r = typical64(x, typical_p)
        if not r["ran"]:
            return [range(len(x))]
        orders, o = [r["order"]], r["order"]
        for i in range(len(o) - 1):
            a, b = r["sh"][o[i]], r["sh"][o[i + 1]]
            if np.isfinite(a) and np.isfinite(b) and b - a < SH_MARGIN:
                s = o.copy()
                s[i], s[i + 1] = o[i + 1], o[i]
                orders.append(s)
        out = []
        for o in orders:
            c = np.cumsum(r["q"][o])
            for d in (-MARGIN, 0.0, MARGIN):
                t = _first(c, typical_p + d, True)
                out.append(tuple(sorted(int(j) for j in o[:len(x) if t is None else t + 1])))
        return set(out)

    def top_p_alts(x):
        r = top_p64(x, top_p)
        if not r["ran"]:
            return [range(len(x))]
        ks = {_first(r["c"], top_p + d, False) for d in (-MARGIN, 0.0, MARGIN)}
        return [range(len(x) if k is None else k + 1) for k in ks]

    def min_p_alts(x):
        r = min_p64(x, min_p)
        if not r["ran"]:
            return [range(len(x))]
        out = []
        for d in (-MINP_REL, 0.0, MINP_REL):
            below = [j for j in range(1, len(x)) if not r["ratio"][j] >= min_p * (1.0 + d)]
            out.append(range(below[0] if below else len(x)))
        return out

    for alts in (tfs_alts, typ_alts, top_p_alts, min_p_alts):
        lists = step(lists, alts)
    return lists


def mask_of(L):
    return sum(1 << int(j) for j in L)


def judge_chain(got, v, temp, top_p, word, tfs_z=1.0, typical_p=1.0, min_p=0.0):
    """Holds one decision of the library (dict(pick: candidate index, kept, p [n_c], mask)) against the float64 rule; asserts.  Returns (row_excluded, draw_excluded):
    whether the reference found a filter decision / the draw too close to call -- the outcome must then still be an admissible one."""
    v = np.asarray(v, np.float64)
    n_c = len(v)
    lists = admissible_lists(v, top_p, tfs_z, typical_p, min_p)
    masks = {mask_of(L): L for L in lists}
    want = chain64(v, temp, top_p, word, tfs_z, typical_p, min_p)["mask"]
    assert want in masks
    gm = int(got["mask"])
    assert gm in masks, (hex(gm), sorted(hex(m) for m in masks), tfs_z, typical_p, top_p, min_p)
    if len(masks) == 1:
        assert gm == want
    L = [j for j in range(n_c) if gm >> j & 1]
    assert got["kept"] == len(L) >= 1
    last = last_step64(v, L, temp, word)
    p = np.asarray(got["p"], np.float64)[:n_c]
    assert np.all(np.abs(p - last["p"]) <= REL * last["p"]), (p, last["p"])
    assert np.all(p[[j for j in range(n_c) if j not in L]] == 0)
    assert int(got["pick"]) in L
    near_u = bool(len(L) > 1 and np.abs(last["cum"][:-1] - last["u"]).min() < MARGIN)   # the boundaries between two picks: the last sum, 1, is none
    if not near_u:
        assert int(got["pick"]) == last["pick"], (got["pick"], last["pick"], word)
    else:
        assert abs(L.index(int(got["pick"])) - L.index(last["pick"])) <= 1
    return len(masks) > 1, near_u


def judge_mirostat(got, v, temp, word, tau, eta, mu):
    """The same for one mirostat v2 decision (got: pick, kept, p, mask, mu, observed; mu: the value the decision started from, None: unset).  mu' is held against the
    float64 value for the library's own cut and pick within MU_BOUND: observed = -log2 p_pick with p_pick within REL relative, so observed is off by at most REL / ln 2,
    plus log2f's and the subtraction's roundings (4 ulp of |observed| + tau); times eta; plus the rounding of eta * e and of the final subtraction (2 ulp of |mu| + |mu'|)."""
    v = np.asarray(v, np.float64)
    n_c = len(v)
    ref = mirostat64(v, temp, word, tau, eta, mu)
    ns = set()
    for d in (-S_MARGIN, 0.0, S_MARGIN):
        over = np.nonzero(ref["s"] > ref["mu_in"] + d)[0]
        ns.add(max(int(over[0]), 1) if len(over) else n_c)
    n = int(got["kept"])
    assert n in ns and int(got["mask"]) == (1 << n) - 1, (n, ns)
    if len(ns) == 1:
        assert n == ref["n"]
    cut = mirostat64(v, temp, word, tau, eta, mu, n=n)
    p = np.asarray(got["p"], np.float64)[:n_c]
    assert np.all(np.abs(p - cut["p"]) <= REL * cut["p"]) and np.all(p[n:] == 0)
    pick = int(got["pick"])
    assert 0 <= pick < n
    near_u = bool(n > 1 and np.abs(cut["cum"][:-1] - cut["u"]).min() < MARGIN)
    if not near_u:
        assert pick == cut["pick"], (pick, cut["pick"], word)
    else:
        assert abs(pick - cut["pick"]) <= 1
    forced = mirostat64(v, temp, word, tau, eta, mu, n=n, at=pick)
    ulp = 2.0 ** -24
    bound_obs = REL / np.log(2.0) + 4 * ulp * (abs(forced["observed"]) + f32(tau))
    assert abs(float(got["observed"]) - forced["observed"]) <= bound_obs, (got["observed"], forced["observed"])
    bound_mu = f32(eta) * bound_obs + 2 * ulp * (abs(forced["mu_in"]) + abs(forced["mu"]) + f32(eta) * abs(forced["observed"] - f32(tau)))
    assert abs(float(got["mu"]) - forced["mu"]) <= bound_mu, (got["mu"], forced["mu"], bound_mu)
    return len(ns) > 1, near_u


def chain64(v, temp, top_p, word, tfs_z=1.0, typical_p=1.0, min_p=0.0, force=None):
    """mirostat == 0.  force: dict with any of tfs (the cut length), typ_order / typ (the order and the kept count), top_p, min_p (kept counts).  dict(tfs, typ, top_p,
    min_p: the stages' own dicts; L: the live list (candidate indices); p [n_c]; cum, u; pick: the candidate index; mask)"""
    force = force or {}
    v = np.asarray(v, np.float64)
    temp, top_p, tfs_z, typical_p, min_p = f32(temp), f32(top_p), f32(tfs_z), f32(typical_p), f32(min_p)
    L = np.arange(len(v))
    tf = tail_free64(v[L], tfs_z, force.get("tfs"))
    L = L[:tf["cut"]]
    ty = typical64(v[L], typical_p, force.get("typ_order"), force.get("typ"))
    L = L[ty["keep"]]
    tp = top_p64(v[L], top_p, force.get("top_p"))
    L = L[:tp["kept"]]
    mp = min_p64(v[L], min_p, force.get("min_p"))
    L = L[:mp["kept"]]
    w = v[L] / temp
    with np.errstate(invalid="ignore"):
        d = draw64(np.exp(w - w[0]), word)
    p = np.zeros(len(v))
    p[L] = d["p"]
    return dict(tfs=tf, typ=ty, top_p=tp, min_p=mp, L=L, p=p, cum=d["cum"], u=d["u"], pick=int(L[d["at"]]), mask=sum(1 << int(j) for j in L))


def last_step64(v, L, temp, word):
    """step 5 alone over a given live list: dict(p [n_c], cum, u, pick)"""
    v, L = np.asarray(v, np.float64), np.asarray(L)
    w = v[L] / f32(temp)
    with np.errstate(invalid="ignore"):
        d = draw64(np.exp(w - w[0]), word)
    p = np.zeros(len(v))
    p[L] = d["p"]
    return dict(p=p, cum=d["cum"], u=d["u"], pick=int(L[d["at"]]))


def mirostat64(v, temp, word, tau, eta, mu=None, n=None, at=None):
    """mirostat v2 over the candidates.  mu None: unset (2 * tau).  dict(mu_in, s: the surprises -log2 p_j over all candidates, n: how many stay, p [n_c], cum, u,
    at = pick: the candidate index, observed, mu: mu'); n / at given: the cut / the pick are taken from outside."""
    v = np.asarray(v, np.float64)
    temp, tau, eta = f32(temp), f32(tau), f32(eta)
    mu_in = 2.0 * tau if mu is None or np.isnan(mu) else float(mu)
    w = v / temp
    with np.errstate(invalid="ignore", divide="ignore"):
        b = np.exp(w - w[0])
        s = -np.log2(b / b.sum())
    over = np.nonzero(s > mu_in)[0]
    n0 = max(int(over[0]), 1) if len(over) else len(v)
    n = n0 if n is None else n
    d = draw64(b[:n], word)
    at = d["at"] if at is None else at
    p = np.zeros(len(v))
    p[:n] = d["p"]
    observed = float(-np.log2(d["p"][at]))
    return dict(mu_in=mu_in, s=s, n=n, p=p, cum=d["cum"], u=d["u"], pick=at, observed=observed, mu=mu_in - eta * (observed - tau), mask=(1 << n) - 1)
