#!/usr/bin/env python3
"""Top-N alternatives with log-probabilities (k_topn_rows; minigpt4_amd_score_tokens_top / _end_chat_batch_top): what they cost next to the unchanged paths they sit
on.  Files: --vision / --llm, or bench.py's synthetic files (--config 13b | 7b | tiny), n_batch 512.  One JSON line per measurement; medians of --reps alternated
runs, every run printed.
  k  the kernel alone through the test library's hook (hipEvent time of the one launch): 1, 64 and 65 rows of 32000 and 32001 logits, top_n 1 / 5 / 20 / 64, on
     3 N(0, 1) data and on all-equal rows, next to k_logprob_rows on the same rows.
  s  a 142-row and a 512-row score pass with top_n 5 and 20 against the plain score pass (amd_score_tokens) of the same tokens.
  d  amd_end_chat_batch_top(top_n = 5) against amd_end_chat_batch at B = 1, 4, 32, greedy and at the reference's default sampling (temp 0.8, top-k 40, top-p 0.9):
     milliseconds per step over --steps steps from the same prompt.
    python tools/top_logprobs.py [--config 13b] [--legs k,s,d] [--reps 5] [--steps 32]   GPU only."""
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


def leg_kernel(lib, reps):
    rng = np.random.default_rng(5)
    for n_vocab in (32000, 32001):
        for rows in (1, 64, 65):
            for data in ("normal", "all_equal"):
                x = (3.0 * rng.standard_normal((rows, n_vocab))).astype(np.float32) if data == "normal" else np.full((rows, n_vocab), 1.25, np.float32)
                t = rng.integers(0, n_vocab, rows).astype(np.int32)
                arms = {"logprob_rows": lambda: lib.amd_test_logprob_rows(x, t)[3] * 1e3}
                for top_n in (1, 5, 20, 64):
                    arms["top%d" % top_n] = (lambda k: lambda: lib.amd_test_topn_rows(x, k, t)[4] * 1e3)(top_n)
                r = alternate(reps, arms)
                print(json.dumps({"leg": "k", "rows": rows, "n_vocab": n_vocab, "data": data, "us": {k: med(v) for k, v in r.items()}, "runs_us": {k: runs(v) for k, v in r.items()}}),
                      flush=True)


def leg_score(lib, ctx, n_vocab, reps, llm_path):
    sync = lambda: lib.library.minigpt4_amd_sync(ctx.ptr)  # noqa: E731
    lib.amd_select_conversation(ctx, 0)
    for rows in (142, 512):
        ids = [1] + fixed_ids(rows - 1, n_vocab, seed=rows)

        def arm(top_n):
            def fn():
                lib.minigpt4_reset_chat(ctx)
                sync()
                t0 = time.perf_counter()
                lib.amd_score_tokens(ctx, ids, top_n=top_n)
                sync()
                return (time.perf_counter() - t0) * 1e3
            return fn
        r = alternate(reps, {"plain": arm(0), "top5": arm(5), "top20": arm(20)})
        print(json.dumps({"leg": "s", "llm": llm_path, "rows": rows, "score_ms": med(r["plain"]), "score_top5_ms": med(r["top5"]), "score_top20_ms": med(r["top20"]),
                          "extra_top5_ms": round(med(r["top5"]) - med(r["plain"]), 3), "extra_top20_ms": round(med(r["top20"]) - med(r["plain"]), 3),
                          "runs": {k: runs(v) for k, v in r.items()}}), flush=True)


def leg_decode(lib, ctx, n_vocab, reps, steps, llm_path):
    sync = lambda: lib.library.minigpt4_amd_sync(ctx.ptr)  # noqa: E731
    for B in (1, 4, 32):
        lib.amd_set_conversations(ctx, B)
        slots = list(range(B))
        heads = [[1] + fixed_ids(23, n_vocab, seed=50 + s) for s in slots]
        for name, kw in (("greedy", dict(temp=0.0)), ("temp0.8_top40_p0.9", dict(temp=0.8, top_k=40, top_p=0.9))):
            def arm(top):
                def fn():
                    for s in slots:
                        lib.amd_select_conversation(ctx, s)
                        lib.minigpt4_reset_chat(ctx)
                        lib.amd_eval_tokens(ctx, heads[s])
                    lib.amd_prefill_batch(ctx, slots)
                    sync()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        if top:
                            lib.amd_end_chat_batch_top(ctx, slots, top_n=5, **kw)
                        else:
                            lib.amd_end_chat_batch(ctx, slots, **kw)
                    sync()
                    return (time.perf_counter() - t0) * 1e3 / steps
                return fn
            r = alternate(reps, {"plain": arm(False), "top5": arm(True)})
            print(json.dumps({"leg": "d", "llm": llm_path, "B": B, "sampling": name, "steps": steps, "end_chat_batch_ms_per_step": med(r["plain"]),
                              "end_chat_batch_top5_ms_per_step": med(r["top5"]), "extra_ms_per_step": round(med(r["top5"]) - med(r["plain"]), 4),
                              "runs": {k: runs(v) for k, v in r.items()}}), flush=True)
    lib.amd_select_conversation(ctx, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="13b", help="bench.py's synthetic files (ignored with --vision / --llm)")
    ap.add_argument("--vision")
    ap.add_argument("--llm")
    ap.add_argument("--legs", default="k,s,d")
    ap.add_argument("--n-ctx", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=32)
    args = ap.parse_args()
    _pkg.load_package()
    from minigpt4_cpp_amd import minigpt4_library as ML
    lib = ML.load_library()
    if lib.amd_device_count() <= 0:
        raise SystemExit("top_logprobs.py: no HIP device visible")
    if bool(args.vision) != bool(args.llm):
        raise SystemExit("top_logprobs.py: --vision and --llm go together")
    legs = set(args.legs.split(","))
    reps = max(5, args.reps)
    if "k" in legs:
        leg_kernel(lib, reps)
    if not legs & {"s", "d"}:
        return
    import bench
    vp, lp = (args.vision, args.llm) if args.llm else bench.make_models(args.config, 0, 1, lambda: None)[:2]
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=args.n_ctx, n_batch=512)
    try:
        n_vocab = lib.library.minigpt4_amd_n_vocab(ctx.ptr)
        if "s" in legs:
            leg_score(lib, ctx, n_vocab, reps, lp)
        if "d" in legs:
            leg_decode(lib, ctx, n_vocab, reps, args.steps, lp)
    finally:
        lib.minigpt4_free(ctx)


if __name__ == "__main__":
    main()
