#!/usr/bin/env python3
"""Draft verification for SEVERAL conversations in one weight pass (minigpt4_amd_verify_draft_batch / minigpt4_amd_decode_lookup_batch): what a pass of n groups of R rows
costs next to the batched step of n rows, and what that means for lookup decoding of a wave.  Files: --vision / --llm, or bench.py's synthetic files (--config 13b | 7b |
tiny), n_ctx 2048.  One JSON line per measurement; medians of --reps (>= 5) alternated runs, every run and max - min printed.  Times are host wall-clock per call
through the public entry points (both sides wait once per step for their token ids).
  a  the verify pass in ms for n = 2 / 4 / 8 conversations x R = 1 / 2 / 4 / 8 rows each (N = n R <= 64; R - 1 wrong draft tokens: the pass costs the same whatever it
     accepts; R = 1 is the call without drafts, i.e. the plain batched step through this entry point) against minigpt4_amd_end_chat_batch(temp = 0) at B = n in the
     same process, at about 150 cached keys, with the break-even per cell: kept draft tokens per conversation per pass from which the pass beats plain steps,
     pass_ms(N) / step_ms(n) - 1, and that as a fraction of the R - 1 sent.  ("launches" is minigpt4_amd_batch_path: the launch kinds of the pass that was last BUILT
     in the context -- a replayed graph does not update it -- so it need not be this cell's.)
  b  minigpt4_amd_decode_lookup_batch at n = 4 over --tokens tokens per conversation; each corpus = that conversation's own greedy continuation with a fraction
     f = 0, 0.25, 0.5, 1 of its tokens replaced by wrong ids, against the plain batched loop; with the check that every conversation's tokens equal the plain loop's.
     A SYNTHETIC MODEL REPEATS NOTHING ON ITS OWN, so this leg sweeps the acceptance rate by construction; IT SAYS NOTHING ABOUT REAL TEXT.
  c  the new attention launch (k_attn_llm_mdraft) and the new epilogue (k_draft_argmax + k_draft_finish_batch) alone against the existing ones at the same row count
     (one k_attn_llm_draft launch per group; k_draft_argmax + k_draft_finish for one group), through the test library's hooks at this model's head shape.  THIS LEG
     TIMES NOTHING ITSELF: the hooks upload and download around their launches and return no device time, so it only ISSUES the launches, --c-iters times each, for a
     kernel trace of the run (`rocprofv3 --kernel-trace --stats -- python tools/lookup_batch_decode.py --legs c`) to read the kernels' own durations from.  It prints
     which launches it issued and no figure.
    python tools/lookup_batch_decode.py [--config 13b] [--legs a,b,c] [--reps 5] [--tokens 128]   GPU only."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkg  # noqa: E402

PASSES = 16


def med(x):
    return round(float(np.median(x)), 4)


def spread(x):
    return round(float(max(x) - min(x)), 4)


def runs(x):
    return [round(float(v), 4) for v in x]


def alternate(reps, arms):
    """arms: {name: fn() -> ms}; every arm once as warm-up (captures its graph), then `reps` rounds in turn."""
    for fn in arms.values():
        fn()
    out = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            out[k].append(fn())
    return out


def fixed_ids(n, n_vocab, seed):
    return [int(v) for v in np.random.default_rng(seed).integers(3, n_vocab, n)]


def prompts_for(n, keys, n_vocab):
    return [[1] + fixed_ids(keys - 1, n_vocab, seed=1000 * keys + s) for s in range(n)]


def setup(lib, ctx, prompts):
    for s, p in enumerate(prompts):
        lib.amd_select_conversation(ctx, s)
        lib.minigpt4_reset_chat(ctx)
        lib.amd_eval_tokens(ctx, p)
        lib.amd_logits(ctx)
    lib.library.minigpt4_amd_sync(ctx.ptr)


def leg_pass(lib, ctx, n_vocab, reps, llm_path, keys, ns, rows):
    sync = lambda: lib.library.minigpt4_amd_sync(ctx.ptr)  # noqa: E731
    wrong = fixed_ids(PASSES * 8 * max(ns), n_vocab, seed=3)
    for n in ns:
        prompts, slots = prompts_for(n, keys, n_vocab), list(range(n))

        def plain():
            setup(lib, ctx, prompts)
            t0 = time.perf_counter()
            for _ in range(PASSES):
                lib.amd_end_chat_batch(ctx, slots, temp=0.0)
            sync()
            return (time.perf_counter() - t0) * 1e3 / PASSES

        def verify(R):
            def fn():
                setup(lib, ctx, prompts)
                kept = 0
                t0 = time.perf_counter()
                for i in range(PASSES):
                    base = 8 * n * i
                    kept += sum(len(x) for x in lib.amd_verify_draft_batch(ctx, slots, [wrong[base + 8 * s:base + 8 * s + R - 1] for s in slots])["ids"])
                ms = (time.perf_counter() - t0) * 1e3 / PASSES
                fn.kept = kept / PASSES / n
                fn.path = lib.amd_batch_path(ctx)
                return ms
            return fn
        arms = {"step": plain}
        for R in rows:
            if n * R <= 64:
                arms["R%d" % R] = verify(R)
        r = alternate(reps, arms)
        t_step = med(r["step"])
        table = []
        for R in rows:
            if "R%d" % R not in arms:
                continue
            t = med(r["R%d" % R])
            even = t / t_step - 1.0
            table.append({"R": R, "N": n * R, "pass_ms": t, "max_minus_min_ms": spread(r["R%d" % R]), "pass_over_step": round(t / t_step, 3),
                          "break_even_kept_per_conversation_per_pass": round(even, 3), "break_even_fraction_of_sent": round(even / (R - 1), 3) if R > 1 else None,
                          "tok_s_all_accepted": round(1e3 * n * R / t, 1), "tok_s_none_accepted": round(1e3 * n / t, 1),
                          "tokens_kept_per_conversation_per_pass_in_this_run": round(arms["R%d" % R].kept, 2), "launches": arms["R%d" % R].path})
        print(json.dumps({"leg": "a", "llm": llm_path, "cached_keys": keys, "conversations": n, "step_ms": t_step, "step_max_minus_min_ms": spread(r["step"]),
                          "step_tok_s": round(1e3 * n / t_step, 1), "rows": table, "runs_ms": {k: runs(v) for k, v in r.items()}}), flush=True)


def leg_lookup(lib, ctx, n_vocab, reps, llm_path, n, n_tokens, n_draft):
    sync = lambda: lib.library.minigpt4_amd_sync(ctx.ptr)  # noqa: E731
    prompts, slots = prompts_for(n, 150, n_vocab), list(range(n))
    setup(lib, ctx, prompts)
    own = [[int(v) for v in r["tokens"]] for r in lib.amd_decode_lookup_batch(ctx, slots, [[]] * n, n_tokens, n_draft=n_draft)]   # no corpus: what each conversation emits
    rng = np.random.default_rng(11)
    state = {}

    def plain():
        setup(lib, ctx, prompts)
        t0 = time.perf_counter()
        for _ in range(n_tokens):
            lib.amd_end_chat_batch(ctx, slots, temp=0.0)
        sync()
        return (time.perf_counter() - t0) * 1e3

    def lookup(f):
        corpora = [[((t + 1) % n_vocab if (f >= 1 or (f > 0 and rng.random() < f)) else t) for t in o] for o in own]

        def fn():
            setup(lib, ctx, prompts)
            t0 = time.perf_counter()
            r = lib.amd_decode_lookup_batch(ctx, slots, corpora, n_tokens, ngram_max=3, ngram_min=1, n_draft=n_draft)
            ms = (time.perf_counter() - t0) * 1e3
            state[f] = r
            return ms
        return fn
    fs = (0.0, 0.25, 0.5, 1.0)
    arms = {"plain": plain}
    for f in fs:
        arms["f%g" % f] = lookup(f)
    r = alternate(reps, arms)
    t_plain = med(r["plain"])
    print(json.dumps({"leg": "b", "llm": llm_path, "conversations": n, "tokens_per_conversation": n_tokens, "n_draft": n_draft, "plain_ms": t_plain,
                      "plain_max_minus_min_ms": spread(r["plain"]), "plain_tok_s": round(1e3 * n * n_tokens / t_plain, 1), "runs_ms": runs(r["plain"]),
                      "note": "synthetic model: each corpus is the conversation's own continuation with a fraction f of wrong ids -- an acceptance sweep, not a statement about real text"}),
          flush=True)
    for f in fs:
        s, t = state[f], med(r["f%g" % f])
        total = sum(len(x["tokens"]) for x in s)
        sent, acc = sum(x["sent"] for x in s), sum(x["accepted"] for x in s)
        print(json.dumps({"leg": "b", "wrong_fraction": f, "ms": t, "max_minus_min_ms": spread(r["f%g" % f]), "tok_s": round(1e3 * total / t, 1), "speedup_over_plain": round(t_plain / t, 3),
                          "passes_with_a_draft": [x["passes"] for x in s], "passes_without": [x["steps"] for x in s], "draft_sent": sent, "draft_accepted": acc,
                          "acceptance": round(acc / max(sent, 1), 3), "tokens_equal_plain_greedy": [[int(v) for v in x["tokens"]] == o for x, o in zip(s, own)],
                          "counters": lib.amd_speculation_batch_info(ctx), "runs_ms": runs(r["f%g" % f])}), flush=True)


def leg_kernels(lib, n_head, hd, n_vocab, iters):
    """Issues the launches; their durations are for a kernel trace to read (the docstring's leg c)."""
    n_ctx, E = 1040, n_head * hd
    rng = np.random.default_rng(5)
    for n, R in ((4, 4), (8, 2), (8, 8)):
        N, n_slot = n * R, n + 1
        groups = [(s, 1000, R) for s in range(n)]
        q, k, v = (rng.standard_normal((N, E)).astype(np.float32) for _ in range(3))
        kc = rng.standard_normal((n_slot, n_ctx, E)).astype(np.float16).view(np.uint16)
        lg = rng.standard_normal((N, n_vocab)).astype(np.float32)
        rs, rp = np.repeat(np.arange(n, dtype=np.int32), R), np.tile(np.arange(R, dtype=np.int32), n) + 1000
        st = dict(n_past=np.zeros(n_slot + 1, np.int32), argmax=np.zeros(n_slot + 1, np.int32), feed=np.zeros(n_slot + 1, np.int32),
                  slot_logits=np.zeros((n_slot + 1, n_vocab), np.float32))           # the hooks' state arrays: one guard word / row behind the last slot
        for name, fn in (("attn_mdraft_one_launch", lambda: lib.amd_test_attn_draft_batch(0, q, k, v, kc, kc, n_head, groups)),
                         ("attn_draft_one_launch_per_group", lambda: lib.amd_test_attn_draft_batch(1, q, k, v, kc, kc, n_head, groups)),
                         ("finish_batch", lambda: lib.amd_test_draft_finish_batch(lg, np.zeros(N, np.int32), rs, rp, st["n_past"], st["argmax"], st["feed"], st["slot_logits"])),
                         ("finish_one_group", lambda: lib.amd_test_draft_finish(lg[:R], np.zeros(R, np.int32), 0, st["n_past"], st["argmax"], st["feed"], st["slot_logits"]))):
            for _ in range(iters + 1):
                fn()
        print(json.dumps({"leg": "c", "conversations": n, "rows_each": R, "n_head": n_head, "head_size": hd, "cached_keys": 1000, "n_vocab": n_vocab, "iterations": iters + 1,
                          "issued": ["k_attn_llm_mdraft (one launch)", "k_attn_llm_draft (one launch per group)", "k_draft_argmax + k_draft_finish_batch",
                                     "k_draft_argmax + k_draft_finish (one group)"], "note": "nothing is timed here: kernel durations come from a kernel trace of this run"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="13b", help="bench.py's synthetic files (ignored with --vision / --llm)")
    ap.add_argument("--vision")
    ap.add_argument("--llm")
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--n-ctx", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--n-draft", type=int, default=4)
    ap.add_argument("--c-iters", type=int, default=20)
    args = ap.parse_args()
    _pkg.load_package()
    from minigpt4_cpp_amd import minigpt4_library as ML
    lib = ML.load_library()
    if lib.amd_device_count() <= 0:
        raise SystemExit("lookup_batch_decode.py: no HIP device visible")
    if bool(args.vision) != bool(args.llm):
        raise SystemExit("lookup_batch_decode.py: --vision and --llm go together")
    legs = set(args.legs.split(","))
    reps = max(5, args.reps)
    import bench
    vp, lp = (args.vision, args.llm) if args.llm else bench.make_models(args.config, 0, 1, lambda: None)[:2]
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=args.n_ctx, n_batch=512)
    try:
        n_vocab = lib.library.minigpt4_amd_n_vocab(ctx.ptr)
        lib.amd_set_conversations(ctx, 8)
        lib.amd_set_speculation(ctx, 7)
        if "a" in legs:
            leg_pass(lib, ctx, n_vocab, reps, lp, 150, (2, 4, 8), (1, 2, 4, 8))
        if "b" in legs:
            leg_lookup(lib, ctx, n_vocab, reps, lp, 4, args.tokens, args.n_draft)
        if "c" in legs:
            n_embd = lib.library.minigpt4_amd_n_embd(ctx.ptr)
            hd = 128 if n_embd % 128 == 0 and n_embd >= 1024 else 64               # LLaMA's head size (the tiny files: 64)
            leg_kernels(lib, n_embd // hd, hd, n_vocab, args.c_iters)
    finally:
        lib.minigpt4_free(ctx)


if __name__ == "__main__":
    main()
