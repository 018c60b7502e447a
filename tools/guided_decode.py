#!/usr/bin/env python3
"""What guided decoding costs per step (minigpt4_amd_end_chat_guided; kernel k_guide_rows).  Files: --vision / --llm, or bench.py's synthetic files (--config 13b | 7b |
tiny).  One JSON line per measurement: medians of --reps (>= 5) alternated runs with max - min next to them, every run printed.
  a  n = 1, 2, 4, 16 pairs (2 n conversations), host wall-clock ms per greedy step over --steps steps of
       guided     minigpt4_amd_end_chat_guided(scale 1.5, temp 0): k_guide_rows, the pick handed to the pass on the device, the batched pass at 2 n rows;
       batch      minigpt4_amd_end_chat_batch(temp 0) at B = 2 n: the same pass without the decision -- the feature's cost is guided - batch;
       host       what a caller had to do before: two minigpt4_amd_get_logits per pair, the mix in NumPy (float32 log-softmax), minigpt4_amd_eval_batch with the token.
  b  k_guide_rows alone (the test library's hook: hipEvent time of one launch) for 1, 2, 4, 16, 32 pairs of 32 001-float rows, with and without the mixed rows written.
    python tools/guided_decode.py [--config 13b] [--legs a,b] [--reps 5] [--steps 32]   GPU only."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkg  # noqa: E402

SCALE = 1.5


def stat(x, nd=3):
    return dict(median=round(float(np.median(x)), nd), spread=round(float(max(x) - min(x)), nd), runs=[round(float(v), nd) for v in x])


def prompt_ids(n_vocab, seed, n=64):
    return [1] + [int(v) for v in np.random.default_rng(seed).integers(3, n_vocab, n - 1)]


def log_softmax32(x):
    x = x - x.max()
    return x - np.log(np.exp(x).sum(dtype=np.float32))


def leg_steps(lib, ctx, n_vocab, reps, steps, n):
    lib.amd_set_conversations(ctx, 2 * n)
    slots = list(range(2 * n))
    pos, neg = slots[0::2], slots[1::2]

    def prompts():
        for k in slots:
            lib.amd_select_conversation(ctx, k)
            lib.minigpt4_reset_chat(ctx)
            lib.amd_eval_tokens(ctx, prompt_ids(n_vocab, 10 + k))
        lib.amd_select_conversation(ctx, 0)
        lib.amd_prefill_batch(ctx, slots)
        lib.library.minigpt4_amd_sync(ctx.ptr)

    def timed(step):
        prompts()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        lib.library.minigpt4_amd_sync(ctx.ptr)
        return 1e3 * (time.perf_counter() - t0) / steps

    def host_step():
        ids = []
        for p, g in zip(pos, neg):
            lib.amd_select_conversation(ctx, p)
            lb = log_softmax32(lib.amd_logits(ctx))
            lib.amd_select_conversation(ctx, g)
            lg = log_softmax32(lib.amd_logits(ctx))
            t = int(np.argmax(lg + np.float32(SCALE) * (lb - lg)))
            ids += [t, t]
        lib.amd_eval_batch(ctx, slots, ids)

    arms = {"guided": lambda: lib.amd_end_chat_guided(ctx, pos, neg, SCALE, temp=0.0), "batch": lambda: lib.amd_end_chat_batch(ctx, slots, temp=0.0), "host": host_step}
    out = {k: [] for k in arms}
    for f in arms.values():                                       # warm-up: the graph captured, the feature's buffers allocated
        timed(f)
    before = lib.amd_guidance_info(ctx)
    for _ in range(reps):
        for k, f in arms.items():
            out[k].append(timed(f))
    after = lib.amd_guidance_info(ctx)
    handed = (after["handed"] - before["handed"]) / max(after["launches"] - before["launches"], 1)
    print(json.dumps({"leg": "a", "what": "ms per greedy step, host wall-clock", "pairs": n, "rows_per_pass": 2 * n, "steps": steps, "end_chat_guided": stat(out["guided"]),
                      "end_chat_batch_B=2n": stat(out["batch"]), "host_emulation": stat(out["host"]),
                      "guided_minus_batch_ms": round(float(np.median(out["guided"]) - np.median(out["batch"])), 3), "pairs_handed_on_device_per_launch": handed}), flush=True)


def leg_kernel(lib, reps, V=32001):
    rng = np.random.default_rng(1)
    for n in (1, 2, 4, 16, 32):
        buf = (3.0 * rng.standard_normal((2 * n, V))).astype(np.float32)
        pairs = [(2 * i, 2 * i + 1) for i in range(n)]
        for rows in (False, True):
            ms = [lib.amd_test_guide_rows(buf, pairs, [SCALE] * n, with_rows=rows)["ms"] for _ in range(reps + 1)][1:]
            print(json.dumps({"leg": "b", "what": "k_guide_rows alone, one launch", "pairs": n, "n_vocab": V, "mixed_rows_written": rows, "us": stat([1e3 * v for v in ms], 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="13b", help="bench.py's synthetic files (ignored with --vision / --llm)")
    ap.add_argument("--vision")
    ap.add_argument("--llm")
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--n-ctx", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=32)
    args = ap.parse_args()
    _pkg.load_package()
    from minigpt4_cpp_amd import minigpt4_library as ML
    lib = ML.load_library()
    if lib.amd_device_count() <= 0:
        raise SystemExit("guided_decode.py: no HIP device visible")
    if bool(args.vision) != bool(args.llm):
        raise SystemExit("guided_decode.py: --vision and --llm go together")
    legs = set(args.legs.split(","))
    reps = max(5, args.reps)
    if "a" in legs:
        import bench
        vp, lp = (args.vision, args.llm) if args.llm else bench.make_models(args.config, 0, 1, lambda: None)[:2]
        ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=args.n_ctx, n_batch=512)
        try:
            n_vocab = lib.library.minigpt4_amd_n_vocab(ctx.ptr)
            print(json.dumps({"config": args.config, "llm": os.path.basename(lp), "n_vocab": n_vocab, "n_ctx": args.n_ctx, "reps": reps, "scale": SCALE}), flush=True)
            for n in (1, 2, 4, 16):
                leg_steps(lib, ctx, n_vocab, reps, args.steps, n)
        finally:
            lib.minigpt4_free(ctx)
    if "b" in legs:
        leg_kernel(lib, reps)


if __name__ == "__main__":
    main()
