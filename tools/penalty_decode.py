#!/usr/bin/env python3
"""What the repetition penalty costs a greedy decode step (minigpt4_amd_set_penalties; kernel k_pen_pick).  Files: --vision / --llm, or bench.py's synthetic files
(--config 13b | 7b | tiny), n_ctx 2048.  One JSON line per measurement: medians of --reps (>= 5) alternated runs with max - min next to them, every run printed.
Times are host wall-clock per step through the public entry points (every arm waits once per step for its token ids).
  a  one conversation, minigpt4_end_chat(temp = 0): the mode off against the mode on with repeat_penalty 1.1 and a window of 64 (one k_pen_pick launch, one table
     upload and one 4-byte copy back per step), tok/s.
  b  the same through minigpt4_amd_end_chat_batch at B = 4 and B = 32 conversations (one launch per step for all of them), aggregate tok/s.
  c  the kernel alone (the test library's hook: hipEvent time of one launch) for 1, 4 and 32 rows of the file's vocabulary with tables of 64 and 1280 entries.
    python tools/penalty_decode.py [--config 13b] [--legs a,b,c] [--reps 5] [--steps 64]   GPU only."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkg  # noqa: E402

PEN = dict(repeat_last_n=64, repeat_penalty=1.1, alpha_presence=0.0, alpha_frequency=0.0, penalize_nl=1)


def stat(x):
    return dict(median=round(float(np.median(x)), 2), spread=round(float(max(x) - min(x)), 2), runs=[round(float(v), 2) for v in x])


def alternate(reps, arms):
    """arms: {name: fn() -> tok/s}; every arm once as warm-up (captures its graphs, allocates the feature's buffers), then `reps` rounds in turn."""
    for fn in arms.values():
        fn()
    out = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            out[k].append(fn())
    return out


def prompt_ids(n_vocab, seed, n=100):
    return [1] + [int(v) for v in np.random.default_rng(seed).integers(3, n_vocab, n - 1)]


def leg_single(lib, ctx, n_vocab, reps, steps):
    def arm(on):
        def run():
            lib.amd_set_penalties(ctx, on)
            lib.minigpt4_reset_chat(ctx)
            lib.amd_eval_tokens(ctx, prompt_ids(n_vocab, 1))
            lib.amd_logits(ctx)
            t0 = time.perf_counter()
            for _ in range(steps):
                lib.minigpt4_end_chat(ctx, temp=0.0, **PEN)
            lib.library.minigpt4_amd_sync(ctx.ptr)
            return steps / (time.perf_counter() - t0)
        return run
    before = lib.amd_penalty_info(ctx)["launches"]
    r = alternate(reps, {"off": arm(False), "on": arm(True)})
    print(json.dumps({"leg": "a", "what": "minigpt4_end_chat(temp 0), one conversation, tok/s", "steps": steps, "mode_off": stat(r["off"]), "repeat_penalty_1.1_window_64": stat(r["on"]),
                      "k_pen_pick_launches": lib.amd_penalty_info(ctx)["launches"] - before}), flush=True)
    lib.amd_set_penalties(ctx, False)


def leg_batch(lib, ctx, n_vocab, reps, steps, B):
    lib.amd_set_conversations(ctx, B)
    slots = list(range(B))

    def arm(on):
        def run():
            lib.amd_set_penalties(ctx, on)
            for k in slots:
                lib.amd_select_conversation(ctx, k)
                lib.minigpt4_reset_chat(ctx)
                lib.amd_conversation_penalties(ctx, k, **PEN)
                lib.amd_eval_tokens(ctx, prompt_ids(n_vocab, 10 + k))
            lib.amd_prefill_batch(ctx, slots)
            lib.library.minigpt4_amd_sync(ctx.ptr)
            t0 = time.perf_counter()
            for _ in range(steps):
                lib.amd_end_chat_batch(ctx, slots, temp=0.0)
            lib.library.minigpt4_amd_sync(ctx.ptr)
            return B * steps / (time.perf_counter() - t0)
        return run
    before = lib.amd_penalty_info(ctx)["launches"]
    r = alternate(reps, {"off": arm(False), "on": arm(True)})
    info = lib.amd_penalty_info(ctx)
    print(json.dumps({"leg": "b", "what": "minigpt4_amd_end_chat_batch(temp 0), aggregate tok/s", "B": B, "steps": steps, "mode_off": stat(r["off"]),
                      "repeat_penalty_1.1_window_64": stat(r["on"]), "k_pen_pick_launches": info["launches"] - before, "table_entries_last_launch": info["last_entries"]}), flush=True)
    lib.amd_set_penalties(ctx, False)


def leg_kernel(lib, n_vocab, reps):
    rng = np.random.default_rng(5)
    one = np.float32(1.1).view(np.int32)
    for rows in (1, 4, 32):
        logits = (rng.standard_normal((rows, n_vocab)) * 4).astype(np.float32)
        for entries in (64, 1280):
            if entries > n_vocab:
                continue
            table = np.zeros((rows * entries, 4), np.int32)
            words = np.zeros((rows, 8), np.int32)
            for r in range(rows):
                table[r * entries:(r + 1) * entries, 0] = rng.choice(n_vocab, entries, replace=False)
                table[r * entries:(r + 1) * entries, 1] = 1
                words[r] = (r, r * entries, entries, 1, one, 0, 0, 0)
            ms = [lib.amd_test_pen_pick(logits, n_vocab, words, table)[2] for _ in range(reps + 1)][1:]
            print(json.dumps({"leg": "c", "what": "k_pen_pick alone, one launch, us", "rows": rows, "n_vocab": n_vocab, "table_entries_per_row": entries,
                              "us": stat([1e3 * v for v in ms])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="13b", help="bench.py's synthetic files (ignored with --vision / --llm)")
    ap.add_argument("--vision")
    ap.add_argument("--llm")
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--n-ctx", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    args = ap.parse_args()
    _pkg.load_package()
    from minigpt4_cpp_amd import minigpt4_library as ML
    lib = ML.load_library()
    if lib.amd_device_count() <= 0:
        raise SystemExit("penalty_decode.py: no HIP device visible")
    if bool(args.vision) != bool(args.llm):
        raise SystemExit("penalty_decode.py: --vision and --llm go together")
    legs = set(args.legs.split(","))
    reps = max(5, args.reps)
    import bench
    vp, lp = (args.vision, args.llm) if args.llm else bench.make_models(args.config, 0, 1, lambda: None)[:2]
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=args.n_ctx, n_batch=512)
    try:
        n_vocab = lib.library.minigpt4_amd_n_vocab(ctx.ptr)
        print(json.dumps({"config": args.config, "llm": os.path.basename(lp), "n_vocab": n_vocab, "reps": reps}), flush=True)
        if "a" in legs:
            leg_single(lib, ctx, n_vocab, reps, args.steps)
        if "b" in legs:
            for B in (4, 32):
                leg_batch(lib, ctx, n_vocab, reps, args.steps, B)
        if "c" in legs:
            leg_kernel(lib, n_vocab, reps)
    finally:
        lib.minigpt4_free(ctx)


if __name__ == "__main__":
    main()
