#!/usr/bin/env python3
"""What a sampled batched decode step costs (minigpt4_amd_end_chat_batch_sampled; kernel k_sample_rows).  Files: --vision / --llm, or bench.py's synthetic files (--config
13b | 7b | tiny).  Sampling parameters: temp 0.8, top-k 40, top-p 0.9 (the reference's defaults).  One JSON line per measurement: medians of --reps (>= 5) alternated runs
with max - min next to them, every run printed.
  a  B = 1, 4, 32 conversations, host wall-clock ms per step and tokens per second over --steps steps of
       greedy     minigpt4_amd_end_chat_batch(temp 0): the pass alone, the decision taken by the pass's own argmax;
       host       minigpt4_amd_end_chat_batch(temp 0.8): per conversation one logits row to the host, one synchronise, one partial sort -- the arm to beat;
       device     minigpt4_amd_end_chat_batch_sampled: one k_sample_rows launch, the picks handed to the pass on the device.
  b  k_sample_rows alone (the test library's hook: hipEvent time of one launch) beside k_topn_rows (top_n = 40) for 1, 4, 32 rows of 32 001 floats, without and with a
     64-entry penalty table per row.
    python tools/sampled_batch_decode.py [--config 13b] [--legs a,b] [--reps 5] [--steps 32]   GPU only."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkg  # noqa: E402

TEMP, TOP_K, TOP_P = 0.8, 40, 0.9


def stat(x, nd=3):
    return dict(median=round(float(np.median(x)), nd), spread=round(float(max(x) - min(x)), nd), runs=[round(float(v), nd) for v in x])


def prompt_ids(n_vocab, seed, n=64):
    return [1] + [int(v) for v in np.random.default_rng(seed).integers(3, n_vocab, n - 1)]


def f32_word(v):
    return int(np.array([v], np.float32).view(np.int32)[0])


def leg_steps(lib, ctx, n_vocab, reps, steps, B):
    lib.amd_set_conversations(ctx, B)
    slots = list(range(B))

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

    arms = {"greedy": lambda: lib.amd_end_chat_batch(ctx, slots, temp=0.0),
            "host": lambda: lib.amd_end_chat_batch(ctx, slots, temp=TEMP, top_k=TOP_K, top_p=TOP_P),
            "device": lambda: lib.amd_end_chat_batch_sampled(ctx, slots, temp=TEMP, top_k=TOP_K, top_p=TOP_P)}
    out = {k: [] for k in arms}
    for f in arms.values():                                       # warm-up: the graph captured, the feature's buffers allocated
        timed(f)
    before = lib.amd_sampling_info(ctx, 0)
    for _ in range(reps):
        for k, f in arms.items():
            out[k].append(timed(f))
    after = lib.amd_sampling_info(ctx, 0)
    handed = (after["handed"] - before["handed"]) / max(after["launches"] - before["launches"], 1)
    med = {k: float(np.median(v)) for k, v in out.items()}
    print(json.dumps({"leg": "a", "what": "ms per step, host wall-clock", "B": B, "steps": steps, "greedy_end_chat_batch": stat(out["greedy"]),
                      "host_chain_end_chat_batch": stat(out["host"]), "end_chat_batch_sampled": stat(out["device"]),
                      "tok_per_s": {k: round(1e3 * B / v, 1) for k, v in med.items()}, "device_minus_greedy_ms": round(med["device"] - med["greedy"], 3),
                      "host_minus_device_ms": round(med["host"] - med["device"], 3), "picks_handed_on_device_per_launch": handed}), flush=True)


def leg_kernel(lib, reps, V=32001):
    rng = np.random.default_rng(1)
    for n in (1, 4, 32):
        buf = (3.0 * rng.standard_normal((n, V))).astype(np.float32)
        for entries in (0, 64):
            rows = np.zeros((n, 8), np.int32)
            table = np.zeros((n * entries, 4), np.int32)
            for r in range(n):
                rows[r] = (r, r * entries, entries, 3 if entries else 0, f32_word(1.3), f32_word(0.25), f32_word(0.5), 0)
                for k, t in enumerate(rng.permutation(V)[:entries]):
                    table[r * entries + k] = (int(t), 1 + k % 3, 0, 0)
            sd = np.array([(1000 + r, 0) for r in range(n)], np.uint64)
            ms = [lib.amd_test_sample_rows(buf, V, rows, table, [(TEMP, TOP_P)] * n, [TOP_K] * n, sd)["ms"] for _ in range(reps + 1)][1:]
            line = {"leg": "b", "what": "one launch, hipEvent time", "rows": n, "n_vocab": V, "table_entries_per_row": entries, "k_sample_rows_us": stat([1e3 * v for v in ms], 1)}
            if not entries:
                tn = [lib.amd_test_topn_rows(buf, TOP_K, [-1] * n)[4] for _ in range(reps + 1)][1:]
                line["k_topn_rows_us"] = stat([1e3 * v for v in tn], 1)
            print(json.dumps(line), flush=True)


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
        raise SystemExit("sampled_batch_decode.py: no HIP device visible")
    if bool(args.vision) != bool(args.llm):
        raise SystemExit("sampled_batch_decode.py: --vision and --llm go together")
    legs = set(args.legs.split(","))
    reps = max(5, args.reps)
    if "a" in legs:
        import bench
        vp, lp = (args.vision, args.llm) if args.llm else bench.make_models(args.config, 0, 1, lambda: None)[:2]
        ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=args.n_ctx, n_batch=512)
        try:
            n_vocab = lib.library.minigpt4_amd_n_vocab(ctx.ptr)
            print(json.dumps({"config": args.config, "llm": os.path.basename(lp), "n_vocab": n_vocab, "n_ctx": args.n_ctx, "reps": reps, "temp": TEMP, "top_k": TOP_K,
                              "top_p": TOP_P}), flush=True)
            for B in (1, 4, 32):
                leg_steps(lib, ctx, n_vocab, reps, args.steps, B)
        finally:
            lib.minigpt4_free(ctx)
    if "b" in legs:
        leg_kernel(lib, reps)


if __name__ == "__main__":
    main()
