"""numpy reference of the epilogue of the verify pass over several conversations (llm_kernels.hip: launch_mdraft_begin + launch_draft_finish_batch), and the builders of
its test inputs.  The rule per row is tests/greedy_ref.py's first_max; per group it is draft_finish_ref's, with the group found from the slot and position arrays alone:
a group starts at row 0 and wherever the slot differs from the row before."""
import numpy as np

import greedy_ref as G

ROWS = 64                       # the result block: m [ROWS] | row_greedy [ROWS] | one guard word


def groups_of(row_slot) -> list:
    """[(t0, R)] of the packed rows: maximal runs of one slot."""
    rs = [int(s) for s in row_slot]
    out, t = [], 0
    while t < len(rs):
        R = 1
        while t + R < len(rs) and rs[t + R] == rs[t]:
            R += 1
        out.append((t, R))
        t += R
    return out


def pack(groups) -> tuple:
    """groups [(slot, p0, R)] -> (row_slot [N], row_pos [N]) in list order."""
    rs = [s for s, _, R in groups for _ in range(R)]
    rp = [p0 + r for _, p0, R in groups for r in range(R)]
    return np.array(rs, np.int32), np.array(rp, np.int32)


def finish_batch_ref(logits, tok, row_slot, row_pos, state: dict) -> dict:
    """The state arrays and the result block after launch_mdraft_begin + launch_draft_finish_batch.  Per group (t0, R, slot): n_past[slot] = row_pos[t0] first; ids[t] =
    first_max(row t); m = the number of LEADING draft tokens the rows chose (tok[t0 + i + 1] == ids[t0 + i] for every i < m, m <= R - 1: a match behind the first
    mismatch, or with another row's choice, does not count); row t0 + m becomes the slot's logits row, ids[t0 + m] its greedy and feed token, n_past[slot] = row_pos[t0] +
    1 + m.  Slots not in the pass keep everything.  res [129]: m per group at its first row and -1 at its other rows, -1 behind N; the rows' ids, -1 behind N; the guard -1."""
    lg = np.asarray(logits, np.float32)
    N = len(lg)
    ids = [G.first_max(lg[t]) for t in range(N)]
    out = {k: np.array(v, copy=True) for k, v in state.items()}
    res = np.full(2 * ROWS + 1, -1, np.int32)
    res[ROWS:ROWS + N] = ids
    ms = {}
    for t0, R in groups_of(row_slot):
        slot = int(row_slot[t0])
        m = 0
        while m < R - 1 and int(tok[t0 + m + 1]) == ids[t0 + m]:
            m += 1
        out["slot_logits"][slot] = lg[t0 + m]
        out["argmax"][slot] = ids[t0 + m]
        out["feed"][slot] = ids[t0 + m]
        out["n_past"][slot] = int(row_pos[t0]) + 1 + m
        res[t0] = m
        ms[slot] = m
    out.update(res=res, ids=ids, m_of_slot=ms)
    return out


def toks_for(ids, groups_m) -> np.ndarray:
    """Row tokens for which group (t0, R) has the count m: groups_m [(t0, R, m, later_match)] -- greedy_ref.draft_toks per group."""
    tok = np.zeros(len(ids), np.int32)
    for t0, R, m, later in groups_m:
        tok[t0:t0 + R] = G.draft_toks(list(ids[t0:t0 + R]), m, later)
    return tok
