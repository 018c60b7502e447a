"""The greedy step epilogues in numpy (csrc/llm_kernels.hip: launch_argmax, k_batch_finish, k_seg_finish, k_draft_argmax / k_draft_finish), and the rows they are
tried on.  numpy only.

THE RULE ("first maximum wins", include/minigpt4_amd_test.h states it for the kernels): first_max(row) is the lowest index i with row[i] equal to the maximum over the
row's non-NaN entries, when that maximum is above -inf; otherwise (every entry NaN or -inf) it is 0.  -0.0 and +0.0 are equal: the lower index wins.

Where an element lives decides which compare it meets, so the planted ties are described by PLACE:
  launch_argmax           element i: workgroup (i // 256) % 64, wave (i % 256) // 64, lane i % 64, trip i // 16384 (64 workgroups x 256 threads, stride 16384)
  batch_finish_row, n % 4 == 0 (16-byte loads): float4 j = i // 4, thread j % 1024 (wave thread // 64), trip j // 1024 (stride 4096 elements), float4 lane i % 4
  batch_finish_row, n % 4 != 0 (scalar loop over the whole row): thread i % 1024, trip i // 1024
A thread meets its own elements in ascending order (`>` keeps the first); between threads argmax_combine decides (equal values: the lower index), once with each side
as the one already held -- so every pair class comes in both orders: the lower index in the lower-numbered wave / workgroup, and in the higher-numbered one (possible
from the second trip on)."""
import numpy as np

LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 4097, 16383, 16384, 16385, 32000, 32001]
PEAK = np.float32(9.0)       # the planted maximum
CAP = np.float32(4.0)        # every unplanted element is at most this
FILL32 = np.uint32(0xFFFFFFFF)


def first_max(row) -> int:
    x = np.asarray(row, np.float32).reshape(-1)
    ok = ~np.isnan(x)
    if not ok.any():
        return 0
    m = x[ok].max()
    if not m > -np.inf:
        return 0
    return int(np.flatnonzero(x == m)[0])             # NaN == m is false; -0.0 == +0.0 is true


# ---- places ---------------------------------------------------------------------------------------------------------------------------------------------------------
def argmax_place(i: int) -> dict:
    return dict(group=(i // 256) % 64, wave=(i % 256) // 64, lane=i % 64, trip=i // 16384, unit=(i // 256) % 64 * 256 + i % 256)


def finish_place(i: int, n: int) -> dict:
    if n % 4 == 0:
        j = i // 4
        return dict(group=0, wave=(j % 1024) // 64, lane=j % 64, trip=j // 1024, unit=j % 1024, f4=i % 4)
    return dict(group=0, wave=(i % 1024) // 64, lane=i % 64, trip=i // 1024, unit=i % 1024, f4=0)


def pair_classes(lo: int, hi: int, n: int, kernel: str) -> set:
    """Which compares the tie (lo, hi), lo < hi < n, goes through in `kernel` ("argmax" or "finish")."""
    a, b = (argmax_place(lo), argmax_place(hi)) if kernel == "argmax" else (finish_place(lo, n), finish_place(hi, n))
    c = set()
    if a["unit"] == b["unit"]:
        c.add("f4" if a["trip"] == b["trip"] else "trips")          # one thread: two lanes of its float4, or two of its trips
    elif a["group"] != b["group"]:
        c.add("groups" if a["group"] < b["group"] else "groups_rev")
    elif a["wave"] != b["wave"]:
        c.add("waves" if a["wave"] < b["wave"] else "waves_rev")
    else:
        c.add("lanes" if a["lane"] < b["lane"] else "lanes_rev")
    if lo == 0 and hi == n - 1:
        c.add("ends")
    return c


def classes_possible(n: int, kernel: str) -> set:
    """Every class some pair lo < hi < n can have in `kernel` -- from the geometry above, not from tie_pairs."""
    c = set()
    if n >= 2:
        c.add("ends")
    if kernel == "argmax":
        if n >= 2: c.add("lanes")
        if n > 64: c.add("waves")
        if n > 256: c.add("groups")
        if n > 16384: c |= {"trips", "lanes_rev", "waves_rev", "groups_rev"}
    elif n % 4 == 0:
        if n >= 4: c.add("f4")
        if n >= 8: c.add("lanes")
        if n > 256: c.add("waves")
        if n > 4096: c |= {"trips", "lanes_rev", "waves_rev"}
    else:
        if n >= 2: c.add("lanes")
        if n > 64: c.add("waves")
        if n > 1024: c |= {"trips", "lanes_rev", "waves_rev"}
    return c


_CANDIDATES = [
    # launch_argmax: lanes, waves, workgroups; then the second trip against the first
    (0, 1), (0, 63), (62, 63), (0, 64), (63, 64), (63, 255), (64, 192), (0, 256), (255, 256), (0, 16383), (1287, 10243),
    (0, 16384), (5, 16389), (1, 16384), (64, 16384), (255, 16385), (256, 16384), (16383, 16384), (300, 16394), (15615, 31999),
    # batch_finish_row, 16-byte loads: lanes of a float4, threads of a wave, waves; then the second trip against the first
    (1, 3), (2, 3), (0, 4), (3, 252), (1, 6), (0, 4095), (1792, 3072), (0, 4096), (5, 4101), (4, 4096), (256, 4096), (4095, 4096), (300, 4100), (27904, 32000 - 1),
    # batch_finish_row, scalar loop: lanes, waves; then the second trip against the first
    (0, 1023), (448, 768), (0, 1024), (7, 1031), (1, 1024), (64, 1024), (1023, 1024), (100, 1030), (30976, 32000),
]


def tie_pairs(n: int) -> list:
    """The index pairs (lo, hi), lo < hi < n, at which a row of length n gets two equal maxima -- the same list for every kernel: a pair planted for one kernel's
    geometry is a tie in the others too.  Always holds (0, n - 1), (n - 2, n - 1) and the last element against its own earlier trips."""
    p = set(c for c in _CANDIDATES if c[1] < n)
    if n >= 2:
        p |= {(0, n - 1), (n - 2, n - 1)}
    for d in (1024, 4096, 16384):
        if n - 1 - d >= 0:
            p.add((n - 1 - d, n - 1))
    return sorted(p)


# ---- rows -----------------------------------------------------------------------------------------------------------------------------------------------------------
def base_row(n: int, seed: int) -> np.ndarray:
    """Seeded normals capped at CAP: no element reaches PEAK, none is NaN or infinite."""
    return np.minimum(np.random.default_rng([n, seed]).standard_normal(n).astype(np.float32), CAP)


def planted_row(n: int, seed: int, ids, value=PEAK) -> np.ndarray:
    x = base_row(n, seed)
    x[list(ids)] = value
    return x


def tie_rows(n: int) -> list:
    """[(label, row, expected id)]: one row per pair of tie_pairs(n) with PEAK at both places; the lower index is expected."""
    return [(f"tie{lo}+{hi}", planted_row(n, 1000 + k, (lo, hi)), lo) for k, (lo, hi) in enumerate(tie_pairs(n))]


def nan_with_payload(n: int) -> np.ndarray:
    """n distinct quiet-NaN bit patterns, both signs."""
    w = np.uint32(0x7FC00001) + np.arange(n, dtype=np.uint32) % np.uint32(0x3FFFFE)
    w[1::2] |= np.uint32(0x80000000)
    return w.view(np.float32)


def special_rows(n: int) -> list:
    """[(label, row, expected id)]: the rows that are not "a seeded draw with a planted tie"."""
    out = []
    for k, i in enumerate(sorted({0, n // 2, n - 1})):
        out.append((f"single{i}", planted_row(n, 2000 + k, (i,)), i))                         # n = 32001: index 32000 lies in no 16-byte load, only in the last scalar trip
    out.append(("all_equal", np.full(n, np.float32(1.5)), 0))
    out.append(("all_neg_equal", np.full(n, np.float32(-3.0e38)), 0))
    out.append(("all_-inf", np.full(n, -np.inf, np.float32), 0))
    out.append(("all_nan", nan_with_payload(n), 0))
    if n >= 2:
        z = -np.abs(base_row(n, 2100)) - np.float32(1.0)                                       # everything else below zero
        for lo, hi in sorted({(0, n - 1), (n // 3, n // 3 + 1), (n // 2, n - 1)} - {(0, 0)}):
            if lo < hi:
                a = z.copy(); a[lo] = np.float32(-0.0); a[hi] = np.float32(0.0)
                b = z.copy(); b[lo] = np.float32(0.0); b[hi] = np.float32(-0.0)
                out += [(f"-0+0@{lo},{hi}", a, lo), (f"+0-0@{lo},{hi}", b, lo)]
        m = np.full(n, -np.inf, np.float32); m[n - 1] = np.float32(-3.0e38)
        out.append(("-inf_but_last", m, n - 1))
        q = nan_with_payload(n).copy(); q[n - 1] = -np.inf                                     # NaN and -inf only: nothing above -inf
        out.append(("nan_and_-inf", q, 0))
        q = nan_with_payload(n).copy(); q[n - 1] = np.float32(-7.0)
        out.append(("nan_but_last", q, n - 1))
    if n >= 5:
        p = n // 2
        x = planted_row(n, 2200, (p,)); x[[0, p - 1, p + 1]] = nan_with_payload(3)              # NaN at index 0 and at the peak's neighbours
        out.append(("nan_round_peak", x, p))
        x = planted_row(n, 2201, (p, n - 1)); x[0] = np.nan; x[::7] = np.nan; x[[p, n - 1]] = PEAK  # NaN sprinkled, and a tie
        out.append(("nan_sprinkled_tie", x, p))
        x = planted_row(n, 2202, (1,)); x[0] = np.nan                                          # NaN first: the first comparison a thread makes
        out.append(("nan_first", x, 1))
    return out


def all_rows(n: int) -> list:
    return tie_rows(n) + special_rows(n)


def agrees_everywhere(row) -> bool:
    """The rows on which the whole family must give one number: NaN-free, maximum above -inf (k_logprob_rows makes no promise elsewhere)."""
    x = np.asarray(row, np.float32)
    return not np.isnan(x).any() and bool(x.max() > -np.inf)


# ---- state ----------------------------------------------------------------------------------------------------------------------------------------------------------
def start_state(n_slot: int, n_vocab: int, seed: int) -> dict:
    """n_past / argmax / feed [n_slot + 1]: distinct non-trivial words; slot_logits [n_slot + 1][n_vocab]: distinct finite rows.  The last word / row is the guard."""
    rng = np.random.default_rng([n_slot, n_vocab, seed])
    w = rng.permutation(np.arange(1000, 1000 + 16 * (n_slot + 1), dtype=np.int32))[:3 * (n_slot + 1)].reshape(3, -1)
    keep = (rng.standard_normal((n_slot + 1, n_vocab)) * 3 + 20).astype(np.float32)
    return dict(n_past=w[0].copy(), argmax=(w[1] + 100000).copy(), feed=(w[2] + 200000).copy(), slot_logits=keep)


def slot_maps(rows: int, n_slot: int, seed: int) -> dict:
    """Row-to-slot maps that are not the identity: the reversal (onto the top slots) and a seeded permutation with gaps."""
    rng = np.random.default_rng([rows, n_slot, seed])
    perm = rng.permutation(n_slot)[:rows].astype(np.int32)
    if rows > 1 and (perm == np.arange(rows)).all():
        perm = perm[::-1].copy()
    return dict(reversal=np.arange(n_slot - 1, n_slot - 1 - rows, -1, dtype=np.int32), permutation=perm)


def finish_ref(form: int, logits, slots_or_fin, state: dict) -> dict:
    """launch_batch_finish (form 0: row_slot [rows]) / launch_seg_finish (form 1: fin [rows][2] = slot, new position): the state arrays after the launch."""
    lg = np.asarray(logits, np.float32)
    d = np.asarray(slots_or_fin, np.int32).reshape(len(lg), -1)
    out = {k: np.array(v, copy=True) for k, v in state.items()}
    for r in range(len(lg)):
        s, i = int(d[r, 0]), first_max(lg[r])
        out["argmax"][s] = i
        out["feed"][s] = i
        out["n_past"][s] = state["n_past"][s] + 1 if form == 0 else d[r, 1]
        out["slot_logits"][s] = lg[r]
    return out


def draft_finish_ref(logits, tok, slot: int, state: dict) -> dict:
    """launch_draft_finish: ids[r] = first_max(row r); m = the number of LEADING draft tokens the rows chose (tok[i + 1] == ids[i] for every i < m, m <= R - 1: a match
    behind the first mismatch does not count); row m becomes the slot's logits row, ids[m] its greedy and feed token, its position advances by 1 + m.
    dict(m, res [10]: m, the ids, -1 behind R, the guard word -1; the state arrays)."""
    lg = np.asarray(logits, np.float32)
    R = len(lg)
    ids = [first_max(lg[r]) for r in range(R)]
    m = 0
    while m < R - 1 and int(tok[m + 1]) == ids[m]:
        m += 1
    out = {k: np.array(v, copy=True) for k, v in state.items()}
    out["slot_logits"][slot] = lg[m]
    out["argmax"][slot] = ids[m]
    out["feed"][slot] = ids[m]
    out["n_past"][slot] = state["n_past"][slot] + 1 + m
    res = np.full(10, -1, np.int32)
    res[0] = m
    res[1:1 + R] = ids
    out.update(m=m, res=res, ids=ids)
    return out


def draft_toks(ids, m: int, later_match: bool = False) -> np.ndarray:
    """Row tokens for which the reference's count is m: tok[0] is the conversation's own token (never compared), tok[i + 1] = ids[i] for i < m, then a mismatch, then
    (later_match) the rows' own choices again -- matches that must not count -- or further mismatches."""
    R = len(ids)
    tok = np.zeros(R, np.int32)
    tok[0] = ids[0] + 5
    for i in range(R - 1):
        if i < m or (later_match and i > m):
            tok[i + 1] = ids[i]
        else:
            tok[i + 1] = ids[i] + 1                      # never the row's choice
    return tok


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
