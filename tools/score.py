#!/usr/bin/env python3
"""Scoring given tokens (minigpt4_amd_score_tokens / minigpt4_amd_score_batch): what the model thought of every token of a prompt, from the prompt pass itself.
Files: --vision / --llm, or bench.py's synthetic files (--config 13b | 7b | tiny ...), n_batch 512.  One JSON line per leg.
  a  perplexity, exp(-mean logprob) over entries 1 .. n - 1 of every window, of a token sequence in windows of n_ctx tokens (each window from a reset conversation, as
     llama.cpp's perplexity tool evaluates them).  The sequence: --tokens FILE (whitespace-separated ids, or a .npy array), or --text FILE tokenized by the model's own
     vocabulary, or (default) a fixed pseudo-random id sequence -- which says nothing about a synthetic file's quality, only that two files can be compared on it.
  b  multiple choice: one image head + question on conversation 0, fork to k conversations, ONE amd_score_batch of the k candidate answers; the summed log-probability
     per candidate and the winner.  --question / --candidates a|b|c.
  c  timing.  A score pass of 142 and of 512 rows against the same rows through amd_eval_tokens + amd_logits (medians of --reps alternated runs, with the runs);
     B = 4 candidates of 8 tokens through amd_score_batch against four amd_score_tokens calls.  The expected extra cost of scoring is ceil(rows / 64) passes over the
     output matrix plus the kernel.  The plain arm also copies the last logits row to the host (amd_logits, 128 KB), which the score arm does not: the difference
     understates the cost of scoring by that copy (a few microseconds).
  k  the kernel alone: k_logprob_rows on 64 and 1 rows of n_vocab logits through the test library's hook (hipEvent time of the one launch; median and runs).
    python tools/score.py [--config 13b] [--legs a,b,c,k] [--n-ctx 2048] [--reps 5]   GPU only."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkg  # noqa: E402


def med(x):
    return round(float(np.median(x)), 3)


def runs(x):
    return [round(float(v), 3) for v in x]


def alternate(reps, arms):
    """arms: {name: fn() -> ms}; every arm once as warm-up, then `reps` rounds in turn."""
    for fn in arms.values():
        fn()
    out = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            out[k].append(fn())
    return out


def fixed_ids(n, n_vocab, seed=20240):
    return [int(v) for v in np.random.default_rng(seed).integers(3, n_vocab, n)]


def read_sequence(lib, ctx, args, n_vocab):
    if args.tokens:
        ids = np.load(args.tokens).reshape(-1) if args.tokens.endswith(".npy") else np.array(open(args.tokens).read().split(), np.int64)
        return [int(v) for v in ids], args.tokens
    if args.text:
        return lib.amd_tokenize(ctx, open(args.text, "rb").read()), args.text
    return [1] + fixed_ids(args.n_tokens - 1, n_vocab), "fixed pseudo-random ids"


def leg_perplexity(lib, ctx, args, n_vocab, n_ctx, llm_path):
    ids, source = read_sequence(lib, ctx, args, n_vocab)
    total, count, per_window = 0.0, 0, []
    t0 = time.perf_counter()
    for at in range(0, len(ids), n_ctx):
        win = ids[at:at + n_ctx]
        if len(win) < 2:
            break
        lib.minigpt4_reset_chat(ctx)
        lp = lib.amd_score_tokens(ctx, win)["logprob"][1:].astype(np.float64)   # entry 0 of a reset conversation is the no-logits case: skipped, like llama.cpp's first token
        total += float(lp.sum())
        count += len(lp)
        per_window.append(round(float(np.exp(-lp.mean())), 4))
    ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"leg": "a", "llm": llm_path, "sequence": source, "tokens": len(ids), "n_ctx": n_ctx, "scored": count, "perplexity": round(float(np.exp(-total / max(count, 1))), 4),
                      "mean_logprob": round(total / max(count, 1), 5), "per_window": per_window, "ms": round(ms, 1), "rows_per_s": round(len(ids) / ms * 1e3, 1)}), flush=True)


def image_head(lib, ctx, rows, question):
    tok = lambda s: lib.amd_tokenize(ctx, s.encode())  # noqa: E731
    lib.minigpt4_reset_chat(ctx)
    lib.minigpt4_system_prompt(ctx)
    lib.amd_eval_tokens(ctx, tok("Human: <Img>"))
    lib.amd_eval_embd(ctx, rows)
    lib.amd_eval_tokens(ctx, tok("</Img> "))
    lib.amd_eval_tokens(ctx, tok(question))
    lib.amd_eval_tokens(ctx, tok("### Assistant:"))


def leg_multiple_choice(lib, ML, G, ctx, args):
    cands = args.candidates.split("|")
    k = len(cands)
    lib.amd_set_conversations(ctx, k + 1)
    emb = lib.minigpt4_encode_image(ctx, ML.array_to_image_struct(G.synth_image(args.image_seed)))
    rows = np.ctypeslib.as_array(emb.data, shape=(32 * lib.library.minigpt4_amd_n_embd(ctx.ptr),)).copy()
    lib.minigpt4_free_embedding(emb)
    toks = [lib.amd_tokenize(ctx, (" " + c).encode(), add_bos=False) for c in cands]
    slots = list(range(1, k + 1))
    t0 = time.perf_counter()
    lib.amd_select_conversation(ctx, 0)
    image_head(lib, ctx, rows, args.question)
    lib.amd_fork_conversation(ctx, 0, slots)                                # the whole state: every candidate's first token is scored by the head's logits
    res = lib.amd_score_batch(ctx, slots, toks)
    ms = (time.perf_counter() - t0) * 1e3
    sums = [float(r["logprob"].astype(np.float64).sum()) for r in res]
    print(json.dumps({"leg": "b", "question": args.question, "candidates": cands, "tokens_each": [len(t) for t in toks], "sum_logprob": [round(s, 4) for s in sums],
                      "mean_logprob": [round(s / len(t), 4) for s, t in zip(sums, toks)], "chosen": cands[int(np.argmax(sums))], "ms_head_fork_score": round(ms, 2)}), flush=True)
    lib.amd_select_conversation(ctx, 0)


def leg_timing(lib, ctx, n_vocab, reps, llm_path):
    sync = lambda: lib.library.minigpt4_amd_sync(ctx.ptr)  # noqa: E731
    lib.amd_select_conversation(ctx, 0)
    for rows in (142, 512):
        ids = [1] + fixed_ids(rows - 1, n_vocab, seed=rows)

        def score():
            lib.minigpt4_reset_chat(ctx)
            sync()
            t0 = time.perf_counter()
            lib.amd_score_tokens(ctx, ids)
            sync()
            return (time.perf_counter() - t0) * 1e3

        def plain():
            lib.minigpt4_reset_chat(ctx)
            sync()
            t0 = time.perf_counter()
            lib.amd_eval_tokens(ctx, ids)
            lib.amd_logits(ctx)
            sync()
            return (time.perf_counter() - t0) * 1e3
        r = alternate(reps, {"score": score, "plain": plain})
        print(json.dumps({"leg": "c", "llm": llm_path, "rows": rows, "score_ms": med(r["score"]), "eval_tokens_logits_ms": med(r["plain"]),
                          "extra_ms": round(med(r["score"]) - med(r["plain"]), 3), "output_tiles": -(-(rows - 1) // 64), "score_rows_per_s": round(rows / med(r["score"]) * 1e3, 1),
                          "score_runs": runs(r["score"]), "eval_tokens_logits_runs": runs(r["plain"])}), flush=True)
    # B = 4 candidates of 8 tokens behind a shared 142-row head
    lib.amd_set_conversations(ctx, 5)
    head = [1] + fixed_ids(141, n_vocab, seed=7)
    cands = [fixed_ids(8, n_vocab, seed=100 + i) for i in range(4)]
    slots = [1, 2, 3, 4]

    def fork():
        lib.amd_select_conversation(ctx, 0)
        lib.minigpt4_reset_chat(ctx)
        lib.amd_eval_tokens(ctx, head)
        lib.amd_fork_conversation(ctx, 0, slots)
        sync()

    def batch():
        fork()
        t0 = time.perf_counter()
        lib.amd_score_batch(ctx, slots, cands)
        sync()
        return (time.perf_counter() - t0) * 1e3

    def single():
        fork()
        t0 = time.perf_counter()
        for s, c in zip(slots, cands):
            lib.amd_select_conversation(ctx, s)
            lib.amd_score_tokens(ctx, c)
        sync()
        return (time.perf_counter() - t0) * 1e3
    r = alternate(reps, {"batch": batch, "single": single})
    print(json.dumps({"leg": "c", "llm": llm_path, "candidates": 4, "tokens_each": 8, "head_rows": len(head), "score_batch_ms": med(r["batch"]), "four_score_tokens_ms": med(r["single"]),
                      "speedup": round(med(r["single"]) / med(r["batch"]), 3), "score_batch_runs": runs(r["batch"]), "four_score_tokens_runs": runs(r["single"])}), flush=True)
    lib.amd_select_conversation(ctx, 0)


def leg_kernel(lib, n_vocab, reps):
    rng = np.random.default_rng(5)
    for rows in (64, 1):
        x = (3.0 * rng.standard_normal((rows, n_vocab))).astype(np.float32)
        t = rng.integers(0, n_vocab, rows).astype(np.int32)
        lib.amd_test_logprob_rows(x, t)                                     # warm-up (the first launch loads the code object)
        us = [lib.amd_test_logprob_rows(x, t)[3] * 1e3 for _ in range(reps)]
        print(json.dumps({"leg": "k", "kernel": "k_logprob_rows", "rows": rows, "n_vocab": n_vocab, "us": round(float(np.median(us)), 2), "runs_us": [round(float(v), 2) for v in us],
                          "GBps_two_sweeps": round(2 * rows * n_vocab * 4 / np.median(us) / 1e3, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="13b", help="bench.py's synthetic files (ignored with --vision / --llm)")
    ap.add_argument("--vision")
    ap.add_argument("--llm")
    ap.add_argument("--legs", default="a,b,c,k")
    ap.add_argument("--n-ctx", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tokens")
    ap.add_argument("--text")
    ap.add_argument("--n-tokens", type=int, default=4096, help="length of the default sequence of leg a")
    ap.add_argument("--question", default="what is in the picture?")
    ap.add_argument("--candidates", default="a cat|a dog on a lawn|a page of printed text|nothing at all")
    ap.add_argument("--image-seed", type=int, default=7)
    args = ap.parse_args()
    _pkg.load_package()
    import bench
    from minigpt4_cpp_amd import minigpt4_library as ML, modelgen as G
    lib = ML.load_library()
    if lib.amd_device_count() <= 0:
        raise SystemExit("score.py: no HIP device visible")
    if bool(args.vision) != bool(args.llm):
        raise SystemExit("score.py: --vision and --llm go together")
    vp, lp = (args.vision, args.llm) if args.llm else bench.make_models(args.config, 0, 1, lambda: None)[:2]
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=args.n_ctx, n_batch=512)
    try:
        n_vocab = lib.library.minigpt4_amd_n_vocab(ctx.ptr)
        legs = set(args.legs.split(","))
        if "a" in legs:
            leg_perplexity(lib, ctx, args, n_vocab, args.n_ctx, lp)
        if "b" in legs:
            leg_multiple_choice(lib, ML, G, ctx, args)
        if "c" in legs:
            leg_timing(lib, ctx, n_vocab, max(5, args.reps), lp)
        if "k" in legs:
            leg_kernel(lib, n_vocab, max(5, args.reps))
    finally:
        lib.minigpt4_free(ctx)


if __name__ == "__main__":
    main()
