"""float64 reference of one LoRA site group (csrc/lora.hip: launch_lora_down + launch_lora_up once, what minigpt4_amd_test_lora_group drives), its error bound, the
mutants that tests/test_cpu_lora_ref.py shows the cases to discriminate, and the case list that tests/test_gpu_lora_group.py runs on the kernels.

A case `c` is a dict with the hook's arguments: rows, n_in, n_out, ldy, mode (0 plain, 1 RMS, 2 SiLU), form (1 vector, 2 MFMA), n_targets, x [rows][n_in] f32, second
(None | g [n_in] | h3 [rows][n_in]) f32, adapters = [dict(rank, alpha_r, mask, A={m: [rank][n_in] f16}, B={m: [n_out][rank] f16})], slot_adapter, slot_scale, row_slot
([rows * stride] or None), stride, slot0, y0 [n_targets][rows][ldy] f32."""
import zlib

import numpy as np

U = 2.0 ** -24
SLAB = {1: 512, 2: 2048}          # K elements per slab of the down kernel's forms (kernels.hpp: LORA_SLAB_VEC, LORA_SLAB_MFMA)
N_TARGETS_MAX = 3
MUTANTS = ("t_slab", "ssq_slab", "swap_b", "aoff0", "scale1", "slot_row", "stride1", "store")


def lora_bound(form, n_in, r, terms):
    """Bound on |kernel - float64| of one output y_n = s sum_j B[n][j] t_j, t_j = sum_k A[j][k] f_k, with terms = S_n = |s| sum_j |B[n][j]| sum_k |A[j][k] f_k| (the sum of
    the absolute values of every product that enters y_n) and u = 2^-24:
      vector: f(x) is formed in fp32 (at most x * g, or expf / add / divide / multiply: <= 8 u relative), the RMS factor from an fp32 sum of n_in squares, a divide, a
              square root and a divide (<= (n_in + 8) u relative, applied to t with one more rounding), every t_j from an fp32 sum of n_in products in some order plus the
              slab sums (<= (n_in + 8) u T_j), y_n from an fp32 sum of r products and the scale (<= (r + 8) u):  (2 n_in + r + 32) u S_n
      MFMA:   additionally f(x) and t are rounded to fp16 before they enter the matrix cores, 2^-11 S_n each (second order: a factor 1 + 2^-10)."""
    b = (2 * n_in + r + 32) * 2.0 ** -24 * terms
    return b + (2 * 2.0 ** -11 * (1 + 2.0 ** -10) * terms if form == 2 else 0.0)


def n_slabs(n_in, form):
    return -(-n_in // SLAB[form])


def rank_padded(r):
    return (r + 15) // 16 * 16


def concat_layout(mask, rp):
    """(aoff per target, -1: absent; rcat): the present targets' rp rows follow one another in target order (kernels.hpp: lora_concat)."""
    aoff, rcat = [], 0
    for m in range(N_TARGETS_MAX):
        aoff.append(rcat if mask >> m & 1 else -1)
        rcat += rp if mask >> m & 1 else 0
    return aoff, rcat


def f_raw(mode, x, second):
    """f(x) before the RMS factor, float64 [rows][n_in]."""
    x = x.astype(np.float64)
    if mode == 1:
        return x * second.astype(np.float64)[None, :]
    if mode == 2:
        return x / (1.0 + np.exp(-x)) * second.astype(np.float64)
    return x


def row_slots(c, mutant=None):
    rows = c["rows"]
    if mutant == "slot_row":
        return np.arange(rows) % len(c["slot_adapter"])
    if c["row_slot"] is None:
        return np.full(rows, c["slot0"])
    return np.asarray(c["row_slot"])[np.arange(rows) * (1 if mutant == "stride1" else c["stride"])]


def group_ref(c, mutant=None, which=0):
    """(want, bound, live), each [n_targets][rows][ldy]: the float64 outputs, the bound on |kernel - want| (lora_bound of the term + 2^-24 (|y0| + |term|) for the one fp32
    add onto y), and which outputs receive a term at all -- every other output must equal y0 bit for bit.
    mutant: the same operation with one mistake of the kind a kernel can make -- "t_slab" / "ssq_slab": K slab `which` (at the slab size of the case's form) left out of t /
    of the RMS sum of squares; "swap_b": each target takes the B of the adapter's next present target; "aoff0": every target reads the rows of A from row 0; "scale1": the
    slots' factors taken as 1; "slot_row": the slot taken as the row index; "stride1": row_slot read with stride 1; "store": the result stored, not added."""
    rows, n_in, n_out, ldy, mode, form, T = (c[k] for k in ("rows", "n_in", "n_out", "ldy", "mode", "form", "n_targets"))
    x64 = c["x"].astype(np.float64)
    f = f_raw(mode, c["x"], c["second"])
    k = np.arange(n_in) // SLAB[form]
    if mode == 1:
        sq = x64 * x64 * (k != which if mutant == "ssq_slab" else np.ones(n_in, bool))[None, :]
        f = f / np.sqrt(sq.sum(axis=1, keepdims=True) / n_in + 1e-6)
    ft = f * (k != which)[None, :] if mutant == "t_slab" else f
    slot = row_slots(c, mutant)
    adapter = np.asarray(c["slot_adapter"])[slot]
    scale = np.ones(rows) if mutant == "scale1" else np.asarray(c["slot_scale"], np.float64)[slot]
    y0 = c["y0"].astype(np.float64)
    want, bound, live = y0.copy(), U * np.abs(y0), np.zeros(y0.shape, bool)
    for a, ad in enumerate(c["adapters"]):
        ra = np.flatnonzero(adapter == a)
        present = [m for m in range(T) if ad["mask"] >> m & 1]
        if not len(ra) or not present:
            continue
        r, rp = ad["rank"], rank_padded(ad["rank"])
        aoff, rcat = concat_layout(ad["mask"], rp)
        acat = np.zeros((rcat, n_in))
        for m in present:
            acat[aoff[m]:aoff[m] + r] = np.asarray(ad["A"][m], np.float64)
        s = ad["alpha_r"] * scale[ra]
        for i, m in enumerate(present):
            b = np.zeros((n_out, rp))
            b[:, :r] = np.asarray(ad["B"][present[(i + 1) % len(present)] if mutant == "swap_b" else m], np.float64)
            off = 0 if mutant == "aoff0" else aoff[m]
            am = acat[off:off + rp]
            term = s[:, None] * ((ft[ra] @ am.T) @ b.T)
            terms = np.abs(s)[:, None] * ((np.abs(f[ra]) @ np.abs(am).T) @ np.abs(b).T)
            want[m, ra, :n_out] = term if mutant == "store" else y0[m, ra, :n_out] + term
            bound[m, ra, :n_out] = lora_bound(form, n_in, r, terms) + U * (np.abs(y0[m, ra, :n_out]) + np.abs(term))
            live[m, ra, :n_out] = True
    return want, bound, live


def one_target(c, m):
    """The case restricted to target m: what a launch for that target alone would be given."""
    d = dict(c, n_targets=1, y0=c["y0"][m:m + 1])
    d["adapters"] = [dict(ad, mask=ad["mask"] >> m & 1, A={0: ad["A"][m]} if ad["mask"] >> m & 1 else {}, B={0: ad["B"][m]} if ad["mask"] >> m & 1 else {}) for ad in c["adapters"]]
    return d


# ------------------------------------------------------------------------------------------------ the cases
# Inputs are COHERENT: column k of f(x) has one sign s_k in every row, A[j][k] = e_j s_k |a|, B[n][j] = d_n e_j |b| with random signs e, d of their own per adapter and
# target.  Every product that enters an output then has the output's sign, so |term| = terms: a mistake that loses, misplaces or rescales a share p of the products moves
# the output by p x terms, against a bound of ~1.5e-3 x terms (MFMA) or ~1e-4 x terms (vector).  With independent zero-mean inputs the sum of n_in x r products is only
# ~sqrt(n_in r) of them large, and at n_in = 4104 the whole term would sit inside 4 x the MFMA bound.  Magnitudes: |x| = 0.25 + |N(0, 1)|, times 3 in one K slab and
# times 32 in a ragged last slab (8 elements in every case here), so that every slab holds >= 2 % of every sum; in SiLU mode the factors go to h3.  |a| ~ 2 / n_in
# (fp16 normal), |b| such that |B t| ~ 1; alpha_r from (2, 0.5, 1), the slots' scales from (1, -0.5, 2.5, 0); y0 = +-(0.5 + |N(0, 1)|), padding columns included.
ALPHA_R = (2.0, 0.5, 1.0)
SCALES = (1.0, -0.5, 2.5, 0.0)


def _spec(name, rows, n_in, n_out, mode, form, adapters, slots, rowmap="cycle", n_targets=None, pad=0, stride=1):
    n_targets = n_targets or max(m.bit_length() for _, m in adapters)
    return dict(name=f"{name}-{('plain', 'rms', 'silu')[mode]}-{('', 'vector', 'mfma')[form]}", rows=rows, n_in=n_in, n_out=n_out, mode=mode, form=form, adapters=adapters, slots=slots,
                rowmap=rowmap, n_targets=n_targets, pad=pad, stride=stride)


def _specs():
    out = []
    # K slabs: an exact slab, a slab + an 8-element tail, three slabs + a tail (vector 512; MFMA 2048; 72 = one K step of 64 + 8), every mode; two targets, two adapters
    # of rank 16 on both and rank 64 on the second alone (aoff 16 / 0), four slots (the third without an adapter).  Then each width once under the other form.
    two = [(16, 0b11), (64, 0b10)]
    slots4 = [(0, 1.0), (1, -0.5), (-1, 1.0), (0, 2.5)]
    sizes = [(1, 512), (1, 520), (1, 1032), (2, 72), (2, 2048), (2, 2056), (2, 4104)]
    for form, n_in in sizes:
        for mode in (0, 1, 2):
            out.append(_spec(f"slab{n_in}", 3 if form == 1 else 33, n_in, 100, mode, form, two, slots4))
    for i, (form, n_in) in enumerate(sizes):
        out.append(_spec(f"slab{n_in}", 3 if form == 2 else 33, n_in, 100, i % 3, 3 - form, two, slots4))
    # joined targets (n_in 264: four K steps + 8; ldy = n_out + 24)
    slots5 = [(0, 1.0), (1, -0.5), (2, 2.5), (-1, 1.0), (1, 0.0)]
    slots3 = [(0, 2.5), (1, -0.5), (-1, 1.0)]
    for form in (1, 2):
        rows = 5 if form == 1 else 40
        out.append(_spec("rcat192", rows, 264, 100, 1, form, [(64, 0b111)] * 3, slots5, pad=24))                       # grid.z = 3 of k_lora_down, u = 1 of k_lora_down_mfma
        out.append(_spec("ranks24_8_64", rows, 264, 100, 0, form, [(24, 0b111), (8, 0b111), (64, 0b111)], slots5, pad=24))   # rp 32 / 16 / 64, rcat 96 / 48 / 192 in one launch
        out.append(_spec("middle_absent", rows, 264, 100, 2, form, [(64, 0b101)], [(0, 1.0), (0, -0.5), (-1, 1.0)], pad=24))
        out.append(_spec("two_adapters", rows, 264, 100, 1, form, [(8, 0b101), (64, 0b111)], slots3, pad=24))
        out.append(_spec("unused_index", rows, 264, 100, 0, form, [(8, 0), (16, 0b11)], [(1, 2.5), (0, 1.0), (1, -0.5)], pad=24))   # adapter 0 has nothing at this site
    # row tiles (n_in 136, n_out 260: three 128-column blocks of the MFMA up kernel, two 256-column blocks of the vector one, both ragged)
    for rows, mode in ((32, 0), (64, 1), (65, 2)):
        out.append(_spec(f"rows{rows}", rows, 136, 260, mode, 2, two, slots4))
    out.append(_spec("rows100_empty_tile", 100, 136, 260, 1, 2, two, slots4, rowmap="tile"))
    out.append(_spec("rows100_empty_tile", 100, 136, 260, 1, 1, two, slots4, rowmap="tile"))
    out.append(_spec("rows1", 1, 136, 260, 1, 1, two, [(1, 2.5)]))
    out.append(_spec("rows3", 3, 136, 260, 2, 1, two, slots4))
    # row plumbing (ldy = n_out + 24)
    for form in (1, 2):
        rows = 7 if form == 1 else 40
        out.append(_spec("grouped", rows, 264, 100, 0, form, two, slots4, rowmap="group", pad=24))
        out.append(_spec("stride2", rows, 264, 100, 1, form, two, slots4, rowmap="group", pad=24, stride=2))
        out.append(_spec("slot0", rows, 264, 100, 2, form, two, slots4, rowmap=("slot0", 3), pad=24))
    out.append(_spec("slot0_none", 40, 264, 100, 0, 2, two, slots4, rowmap=("slot0", 2), pad=24))
    return out


SPECS = _specs()
IDS = [s["name"] for s in SPECS]
assert len(set(IDS)) == len(IDS)


def _rowmap(spec):
    rows, n = spec["rows"], len(spec["slots"])
    r = np.arange(rows)
    if spec["rowmap"] == "cycle":
        return r % n
    if spec["rowmap"] == "group":                                   # three rows to a slot
        return r // 3 % n
    if spec["rowmap"] == "tile":                                    # rows 32..63: the slot without an adapter -- a tile with nothing to do between live ones
        none = [i for i, (a, _) in enumerate(spec["slots"]) if a < 0][0]
        return np.where((r >= 32) & (r < 64), none, r % n)
    raise ValueError(spec["rowmap"])


def make_case(spec):
    rng = np.random.default_rng(zlib.crc32(spec["name"].encode()))
    rows, n_in, n_out, mode, form, T = (spec[k] for k in ("rows", "n_in", "n_out", "mode", "form", "n_targets"))
    ldy = n_out + spec["pad"]
    ks, k = n_slabs(n_in, form), np.arange(n_in) // SLAB[form]
    fac = np.ones(ks)
    if ks > 1:
        fac[1 if n_in >= 2 * SLAB[form] else 0] = 3.0
        if n_in % SLAB[form]:
            fac[-1] = 32.0
    mag = lambda *shape: 0.25 + np.abs(rng.standard_normal(shape))
    sign = lambda *shape: rng.integers(0, 2, shape) * 2.0 - 1.0
    sx, s2 = sign(n_in), sign(n_in)
    x = mag(rows, n_in) * sx
    if mode == 0:
        x, second, sf = x * fac[k], None, sx
    elif mode == 1:
        x, second, sf = x * fac[k], 0.5 + rng.random(n_in), sx
    else:
        second, sf = mag(rows, n_in) * s2 * fac[k], sx * s2
    x = x.astype(np.float32)
    second = None if second is None else second.astype(np.float32)
    f = np.abs(f_raw(mode, x, second))
    if mode == 1:
        f = f / np.sqrt((x.astype(np.float64) ** 2).mean(axis=1, keepdims=True) + 1e-6)
    tbar = 2.0 / n_in * f.sum(axis=1).mean()                         # the size of a t entry
    adapters = []
    for a, (rank, mask) in enumerate(spec["adapters"]):
        A, B = {}, {}
        for m in range(T):
            if mask >> m & 1:
                e, d = sign(rank), sign(n_out)
                A[m] = (e[:, None] * sf[None, :] * (0.5 + rng.random((rank, n_in))) * 2.0 / n_in).astype(np.float16)
                B[m] = (d[:, None] * e[None, :] * (0.5 + rng.random((n_out, rank))) / (rank * tbar)).astype(np.float16)
        adapters.append(dict(rank=rank, alpha_r=ALPHA_R[a % 3], mask=mask, A=A, B=B))
    c = dict(name=spec["name"], rows=rows, n_in=n_in, n_out=n_out, ldy=ldy, mode=mode, form=form, n_targets=T, x=x, second=second, adapters=adapters,
             slot_adapter=np.array([a for a, _ in spec["slots"]], np.int32), slot_scale=np.array([s for _, s in spec["slots"]], np.float32), row_slot=None, stride=1, slot0=0)
    if isinstance(spec["rowmap"], tuple):
        c["slot0"] = spec["rowmap"][1]
    else:
        st, own = spec["stride"], _rowmap(spec)
        rs = np.empty(rows * st, np.int32)
        for i in range(st):                                         # the entries a stride skips: valid slots, but the next one on
            rs[i::st] = (own + i) % len(spec["slots"])
        c["row_slot"], c["stride"] = rs, st
    c["y0"] = (sign(T, rows, ldy) * (0.5 + np.abs(rng.standard_normal((T, rows, ldy))))).astype(np.float32)
    return c
