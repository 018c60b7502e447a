#!/usr/bin/env python3
"""Draft verification and greedy lookup decoding (minigpt4_amd_verify_draft / minigpt4_amd_decode_lookup): what a verify pass of R rows costs next to the plain decode
step, and what that means for one conversation's tokens per second.  Files: --vision / --llm, or bench.py's synthetic files (--config 13b | 7b | tiny), n_ctx 2048.
One JSON line per measurement; medians of --reps (>= 5) alternated runs, every run printed.  Times are host wall-clock per call through the public entry points
(both sides wait once per step for their token ids).
  a  the verify pass in ms for R = 1 .. 8 (R - 1 wrong draft tokens: the pass costs the same whatever it accepts) against minigpt4_end_chat(temp = 0) in the same
     process, at about 150 and about 1 024 cached keys; R = 3 and 4 again once the context has the row-interleaved MFMA image (set_conversations(2) then (1)).
  b  the single-conversation tok/s this gives with every draft token accepted (R / pass) and with none accepted (1 / pass).
  c  per R the break-even: accepted draft tokens per pass, and the fraction of the R - 1 sent, from which a pass beats plain steps (pass / plain - 1).
  d  minigpt4_amd_decode_lookup over --tokens tokens; corpus = the model's own greedy continuation with a fraction f = 0, 0.25, 0.5, 1 of its tokens replaced by wrong
     ids.  A SYNTHETIC MODEL REPEATS NOTHING ON ITS OWN, so this leg sweeps the acceptance rate by construction; IT SAYS NOTHING ABOUT REAL TEXT.
    python tools/lookup_decode.py [--config 13b] [--legs a,d] [--reps 5] [--tokens 256]   GPU only."""
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


def leg_pass(lib, ctx, n_vocab, reps, llm_path, keys, rows, image):
    sync = lambda: lib.library.minigpt4_amd_sync(ctx.ptr)  # noqa: E731
    prompt = [1] + fixed_ids(keys - 1, n_vocab, seed=keys)
    wrong = fixed_ids(PASSES * 8, n_vocab, seed=3)

    def setup():
        lib.minigpt4_reset_chat(ctx)
        lib.amd_eval_tokens(ctx, prompt)
        lib.amd_logits(ctx)
        sync()

    def plain():
        setup()
        t0 = time.perf_counter()
        for _ in range(PASSES):
            lib.minigpt4_end_chat(ctx, temp=0.0)
        sync()
        return (time.perf_counter() - t0) * 1e3 / PASSES

    def verify(R):
        def fn():
            setup()
            kept = 0
            t0 = time.perf_counter()
            for i in range(PASSES):
                kept += len(lib.amd_verify_draft(ctx, wrong[8 * i:8 * i + R - 1])["ids"])
            ms = (time.perf_counter() - t0) * 1e3 / PASSES
            fn.kept = kept / PASSES
            return ms
        return fn
    arms = {"plain": plain}
    for R in rows:
        arms["R%d" % R] = verify(R)
    r = alternate(reps, arms)
    t_plain = med(r["plain"])
    table = []
    for R in rows:
        t = med(r["R%d" % R])
        even = t / t_plain - 1.0
        table.append({"R": R, "pass_ms": t, "pass_over_plain": round(t / t_plain, 3), "tok_s_all_accepted": round(1e3 * R / t, 1), "tok_s_none_accepted": round(1e3 / t, 1),
                      "break_even_accepted_per_pass": round(even, 3), "break_even_fraction_of_sent": round(even / (R - 1), 3) if R > 1 else None,
                      "tokens_kept_per_pass_in_this_run": round(arms["R%d" % R].kept, 2)})
    print(json.dumps({"leg": "a", "llm": llm_path, "cached_keys": keys, "mfma_image": image, "plain_step_ms": t_plain, "plain_tok_s": round(1e3 / t_plain, 1), "rows": table,
                      "launches_of_the_last_pass": lib.amd_batch_path(ctx), "runs_ms": {k: runs(v) for k, v in r.items()}}), flush=True)


def leg_lookup(lib, ctx, n_vocab, reps, llm_path, n_tokens, n_draft):
    sync = lambda: lib.library.minigpt4_amd_sync(ctx.ptr)  # noqa: E731
    prompt = [1] + fixed_ids(149, n_vocab, seed=150)

    def setup():
        lib.minigpt4_reset_chat(ctx)
        lib.amd_eval_tokens(ctx, prompt)
        lib.amd_logits(ctx)
        sync()
    setup()
    own = [int(v) for v in lib.amd_decode_lookup(ctx, [], n_tokens, n_draft=n_draft)["tokens"]]        # no corpus, nothing repeats: plain steps only
    rng = np.random.default_rng(11)
    state = {}

    def plain():
        setup()
        t0 = time.perf_counter()
        for _ in range(n_tokens):
            lib.minigpt4_end_chat(ctx, temp=0.0)
        sync()
        return (time.perf_counter() - t0) * 1e3

    def lookup(f):
        corpus = [((t + 1) % n_vocab if rng.random() < f else t) for t in own] if 0 < f < 1 else ([(t + 1) % n_vocab for t in own] if f >= 1 else list(own))

        def fn():
            setup()
            t0 = time.perf_counter()
            r = lib.amd_decode_lookup(ctx, corpus, n_tokens, ngram_max=3, ngram_min=1, n_draft=n_draft)
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
    print(json.dumps({"leg": "d", "llm": llm_path, "tokens": n_tokens, "n_draft": n_draft, "plain_ms": t_plain, "plain_tok_s": round(1e3 * n_tokens / t_plain, 1),
                      "note": "synthetic model: the corpus is its own continuation with a fraction f of wrong ids -- an acceptance sweep, not a statement about real text"}), flush=True)
    for f in fs:
        s, t = state[f], med(r["f%g" % f])
        print(json.dumps({"leg": "d", "wrong_fraction": f, "ms": t, "tok_s": round(1e3 * len(s["tokens"]) / t, 1), "speedup_over_plain": round(t_plain / t, 3), "passes": s["passes"],
                          "plain_steps": s["steps"], "draft_sent": s["sent"], "draft_accepted": s["accepted"], "acceptance": round(s["accepted"] / max(s["sent"], 1), 3),
                          "tokens_equal_plain_greedy": [int(v) for v in s["tokens"]] == own, "runs_ms": runs(r["f%g" % f])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="13b", help="bench.py's synthetic files (ignored with --vision / --llm)")
    ap.add_argument("--vision")
    ap.add_argument("--llm")
    ap.add_argument("--legs", default="a,d")
    ap.add_argument("--n-ctx", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--n-draft", type=int, default=4)
    args = ap.parse_args()
    _pkg.load_package()
    from minigpt4_cpp_amd import minigpt4_library as ML
    lib = ML.load_library()
    if lib.amd_device_count() <= 0:
        raise SystemExit("lookup_decode.py: no HIP device visible")
    if bool(args.vision) != bool(args.llm):
        raise SystemExit("lookup_decode.py: --vision and --llm go together")
    legs = set(args.legs.split(","))
    reps = max(5, args.reps)
    import bench
    vp, lp = (args.vision, args.llm) if args.llm else bench.make_models(args.config, 0, 1, lambda: None)[:2]
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=args.n_ctx, n_batch=512)
    try:
        n_vocab = lib.library.minigpt4_amd_n_vocab(ctx.ptr)
        lib.amd_set_speculation(ctx, 7)
        if "a" in legs:
            for keys in (150, 1024):
                leg_pass(lib, ctx, n_vocab, reps, lp, keys, list(range(1, 9)), image=False)
        if "d" in legs:
            leg_lookup(lib, ctx, n_vocab, reps, lp, args.tokens, args.n_draft)
        if "a" in legs:
            lib.amd_set_conversations(ctx, 2)            # builds the row-interleaved image of the k-quant weights (twice their memory); it stays with the context
            lib.amd_set_conversations(ctx, 1)
            for keys in (150, 1024):
                leg_pass(lib, ctx, n_vocab, reps, lp, keys, [3, 4], image=True)
    finally:
        lib.minigpt4_free(ctx)


if __name__ == "__main__":
    main()
