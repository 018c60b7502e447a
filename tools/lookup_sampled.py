#!/usr/bin/env python3
"""Draft verification under sampling (minigpt4_amd_verify_draft_sampled / minigpt4_amd_decode_lookup_sampled; kernels k_sample_rows + k_draft_sample_finish): what the
sampled verify pass costs next to the greedy one and next to a plain sampled step, and what that means for one conversation's tokens per second at temp 0.8, top-k 40,
top-p 0.9 (the reference's defaults).  Files: --vision / --llm, or bench.py's synthetic files (--config 13b | 7b | tiny), n_ctx 2048.  One JSON line per measurement;
medians of --reps (>= 5) alternated runs with max - min, every run printed.  Times are host wall-clock per call through the public entry points.
  a  the sampled verify pass in ms for R = 1 .. 8 (R - 1 wrong draft tokens: the pass costs the same whatever it accepts) against the greedy verify pass at the same R and
     against one minigpt4_amd_end_chat_batch_sampled step at B = 1, in the same process, at about 150 cached keys.
  b  per R the break-even that follows from a: accepted draft tokens per pass, and the fraction of the R - 1 sent, from which a sampled pass beats plain sampled steps
     (pass / step - 1).
  c  minigpt4_amd_decode_lookup_sampled over --tokens tokens against a plain minigpt4_amd_end_chat_batch_sampled loop from the same (seed, draws); corpus = the plain
     loop's own text with a fraction f = 0, 0.25, 0.5, 1 of its tokens replaced by wrong ids.  A SYNTHETIC MODEL REPEATS NOTHING ON ITS OWN, so this leg sweeps the
     acceptance rate by construction; IT SAYS NOTHING ABOUT REAL TEXT.
  d  the epilogue alone on bare rows at the model's vocabulary: k_sample_rows over R rows and k_draft_sample_finish, hipEvent times of the test library's hooks.
    python tools/lookup_sampled.py [--config 13b] [--legs a,c,d] [--reps 5] [--tokens 128]   GPU only."""
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
TEMP, TOP_K, TOP_P = 0.8, 40, 0.9
SEED = 4242


def med(x):
    return round(float(np.median(x)), 4)


def spread(x):
    return round(float(np.max(x) - np.min(x)), 4)


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


def make_setup(lib, ctx, n_vocab, keys=150):
    prompt = [1] + fixed_ids(keys - 1, n_vocab, seed=keys)

    def setup():
        lib.minigpt4_reset_chat(ctx)
        lib.amd_eval_tokens(ctx, prompt)
        lib.amd_logits(ctx)
        lib.amd_conversation_seed(ctx, 0, SEED, 0)
        lib.library.minigpt4_amd_sync(ctx.ptr)
    return setup


def leg_pass(lib, ctx, n_vocab, reps, llm_path):
    setup = make_setup(lib, ctx, n_vocab)
    wrong = fixed_ids(PASSES * 8, n_vocab, seed=3)

    def timed(step):
        def fn():
            setup()
            t0 = time.perf_counter()
            for i in range(PASSES):
                step(i)
            lib.library.minigpt4_amd_sync(ctx.ptr)
            return (time.perf_counter() - t0) * 1e3 / PASSES
        return fn
    arms = {"step": timed(lambda i: lib.amd_end_chat_batch_sampled(ctx, [0], TEMP, TOP_K, TOP_P))}
    for R in range(1, 9):
        arms["greedy_R%d" % R] = timed(lambda i, R=R: lib.amd_verify_draft(ctx, wrong[8 * i:8 * i + R - 1]))
        arms["sampled_R%d" % R] = timed(lambda i, R=R: lib.amd_verify_draft_sampled(ctx, wrong[8 * i:8 * i + R - 1], TEMP, TOP_K, TOP_P))
    r = alternate(reps, arms)
    t_step = med(r["step"])
    table = []
    for R in range(1, 9):
        g, s = med(r["greedy_R%d" % R]), med(r["sampled_R%d" % R])
        even = s / t_step - 1.0
        table.append({"R": R, "sampled_pass_ms": s, "sampled_spread_ms": spread(r["sampled_R%d" % R]), "greedy_pass_ms": g, "greedy_spread_ms": spread(r["greedy_R%d" % R]),
                      "sampled_minus_greedy_us": round(1e3 * (s - g), 1), "sampled_over_step": round(s / t_step, 3),
                      "break_even_accepted_per_pass": round(even, 3), "break_even_fraction_of_sent": round(even / (R - 1), 3) if R > 1 else None})
    print(json.dumps({"leg": "a+b", "llm": llm_path, "cached_keys": 150, "sampled_step_ms": t_step, "sampled_step_spread_ms": spread(r["step"]),
                      "sampled_step_tok_s": round(1e3 / t_step, 1), "rows": table, "speculation_info": lib.amd_speculation_info(ctx),
                      "runs_ms": {k: runs(v) for k, v in r.items()}}), flush=True)


def leg_lookup(lib, ctx, n_vocab, reps, llm_path, n_tokens, n_draft):
    setup = make_setup(lib, ctx, n_vocab)
    setup()
    own = [int(lib.amd_end_chat_batch_sampled(ctx, [0], TEMP, TOP_K, TOP_P, with_ids=True)[1][0]) for _ in range(n_tokens)]
    rng = np.random.default_rng(11)
    state = {}

    def plain():
        setup()
        t0 = time.perf_counter()
        for _ in range(n_tokens):
            lib.amd_end_chat_batch_sampled(ctx, [0], TEMP, TOP_K, TOP_P)
        lib.library.minigpt4_amd_sync(ctx.ptr)
        return (time.perf_counter() - t0) * 1e3

    def lookup(f):
        corpus = [((t + 1) % n_vocab if rng.random() < f else t) for t in own] if 0 < f < 1 else ([(t + 1) % n_vocab for t in own] if f >= 1 else list(own))

        def fn():
            setup()
            t0 = time.perf_counter()
            r = lib.amd_decode_lookup_sampled(ctx, corpus, n_tokens, ngram_max=3, ngram_min=1, n_draft=n_draft, temp=TEMP, top_k=TOP_K, top_p=TOP_P)
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
    print(json.dumps({"leg": "c", "llm": llm_path, "tokens": n_tokens, "n_draft": n_draft, "plain_ms": t_plain, "plain_spread_ms": spread(r["plain"]),
                      "plain_tok_s": round(1e3 * n_tokens / t_plain, 1), "runs_ms": runs(r["plain"]),
                      "note": "synthetic model: the corpus is the plain loop's own text with a fraction f of wrong ids -- an acceptance sweep, not a statement about real text"}), flush=True)
    for f in fs:
        s, t = state[f], med(r["f%g" % f])
        toks = [int(v) for v in s["tokens"]]
        print(json.dumps({"leg": "c", "wrong_fraction": f, "ms": t, "spread_ms": spread(r["f%g" % f]), "tok_s": round(1e3 * len(toks) / t, 1),
                          "speedup_over_plain": round(t_plain * len(toks) / n_tokens / t, 3), "tokens": len(toks), "passes": s["passes"], "plain_steps": s["steps"], "draft_sent": s["sent"],
                          "draft_accepted": s["accepted"], "accepted_per_pass": round(s["accepted"] / max(s["passes"], 1), 3),
                          "tokens_equal_the_plain_loop": toks == own[:len(toks)], "runs_ms": runs(r["f%g" % f])}), flush=True)


def leg_epilogue(lib, n_vocab, reps):
    rng = np.random.default_rng(5)
    out = []
    for R in (1, 2, 4, 8):
        buf = (3.0 * rng.standard_normal((R, n_vocab))).astype(np.float32)
        rows = np.array([(r, 0, 0, 0, 0, 0, 0, 0) for r in range(R)], np.int32)
        sd = np.array([(SEED, 1 + r) for r in range(R)], np.uint64)
        args = (buf, n_vocab, rows, np.zeros((0, 4), np.int32), [(TEMP, TOP_P)] * R, [TOP_K] * R, sd)
        fin, smp = [], []
        for _ in range(reps + 1):
            fin.append(lib.amd_test_draft_sample(*args, [-1] * R, 0, np.zeros((2, 3), np.int32), np.zeros((2, n_vocab), np.float32))["ms"] * 1e3)
            smp.append(lib.amd_test_sample_rows(*args)["ms"] * 1e3)
        out.append({"R": R, "k_sample_rows_us": med(smp[1:]), "k_sample_rows_spread_us": spread(smp[1:]), "k_draft_sample_finish_us": med(fin[1:]),
                    "k_draft_sample_finish_spread_us": spread(fin[1:])})
    print(json.dumps({"leg": "d", "n_vocab": n_vocab, "rows": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="13b", help="bench.py's synthetic files (ignored with --vision / --llm)")
    ap.add_argument("--vision")
    ap.add_argument("--llm")
    ap.add_argument("--legs", default="a,c,d")
    ap.add_argument("--n-ctx", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--n-draft", type=int, default=4)
    args = ap.parse_args()
    _pkg.load_package()
    from minigpt4_cpp_amd import minigpt4_library as ML
    lib = ML.load_library()
    if lib.amd_device_count() <= 0:
        raise SystemExit("lookup_sampled.py: no HIP device visible")
    if bool(args.vision) != bool(args.llm):
        raise SystemExit("lookup_sampled.py: --vision and --llm go together")
    legs = set(args.legs.split(","))
    reps = max(5, args.reps)
    import bench
    vp, lp = (args.vision, args.llm) if args.llm else bench.make_models(args.config, 0, 1, lambda: None)[:2]
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=args.n_ctx, n_batch=512)
    try:
        n_vocab = lib.library.minigpt4_amd_n_vocab(ctx.ptr)
        lib.amd_set_speculation(ctx, 7)
        if "a" in legs or "b" in legs:
            leg_pass(lib, ctx, n_vocab, reps, lp)
        if "c" in legs:
            leg_lookup(lib, ctx, n_vocab, reps, lp, args.tokens, args.n_draft)
        if "d" in legs:
            leg_epilogue(lib, n_vocab, reps)
    finally:
        lib.minigpt4_free(ctx)


if __name__ == "__main__":
    main()
