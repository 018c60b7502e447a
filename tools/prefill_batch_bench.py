#!/usr/bin/env python3
"""Prompt passes of B conversations: B separate evaluations (one flush per conversation, what the first batched decode step does today) against one
minigpt4_amd_prefill_batch (the conversations' rows packed into chunks of <= n_batch rows, one weight pass per chunk).  Every conversation queues the system prompt
and an image turn (~142 rows, modelgen.synth_image).  Files: the 13B Q5_K_M headline file and the 7B Q4_0 file (bench.py's synthetic files), n_ctx 2048,
n_batch 512.  Both arms are warmed up, then timed alternately with minigpt4_amd_sync around them; one JSON line per (file, B): median ms of each arm, ms per
conversation, rows per second.
    python tools/prefill_batch_bench.py [--configs 13b,7b] [--batches 1,2,4,8,16,32] [--reps 3]   GPU only."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="13b,7b")
    ap.add_argument("--batches", default="1,2,4,8,16,32")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    _pkg.load_package()
    import bench
    from minigpt4_cpp_amd import minigpt4_library as ML, modelgen as G
    lib = ML.load_library()
    if lib.amd_device_count() <= 0:
        raise SystemExit("prefill_batch_bench.py: no HIP device visible")
    batches = [int(b) for b in args.batches.split(",")]
    for config in args.configs.split(","):
        vp, lp, _, _ = bench.make_models(config, 0, 1, lambda: None)
        ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=2048, n_batch=512)
        lib.amd_set_conversations(ctx, max(batches))
        embs = [lib.minigpt4_encode_image(ctx, ML.array_to_image_struct(G.synth_image(7 + i))) for i in range(8)]
        sync = lambda: lib.library.minigpt4_amd_sync(ctx.ptr)  # noqa: E731

        def queue(B):
            rows = 0
            for s in range(B):
                lib.amd_select_conversation(ctx, s)
                lib.minigpt4_reset_chat(ctx)
                lib.minigpt4_system_prompt(ctx)
                lib.minigpt4_begin_chat_image(ctx, embs[s % len(embs)], "what is in the picture?")
                rows += lib.library.minigpt4_amd_n_past(ctx.ptr)
            lib.amd_select_conversation(ctx, 0)
            return rows

        def separate(B):
            for s in range(B):
                lib.amd_select_conversation(ctx, s)
                sync()                                           # the conversation's own flush(), then a stream synchronise
            lib.amd_select_conversation(ctx, 0)

        def batched(B):
            lib.amd_prefill_batch(ctx, list(range(B)))
            sync()

        def timed(B, fn):
            queue(B)                                             # host-side queues only: nothing is launched before t0
            t0 = time.perf_counter()
            fn(B)
            return (time.perf_counter() - t0) * 1e3

        for B in batches:
            rows = queue(B)
            for fn in (separate, batched):                        # warm-up: code objects, LDS opt-in, first touch
                timed(B, fn)
            sep, bat = [], []
            for _ in range(args.reps):
                sep.append(timed(B, separate))
                bat.append(timed(B, batched))
            ms_s, ms_b = float(np.median(sep)), float(np.median(bat))
            print(json.dumps({"config": config, "B": B, "rows": rows, "rows_per_conversation": rows // B, "separate_ms": round(ms_s, 3), "batched_ms": round(ms_b, 3),
                              "separate_ms_per_conversation": round(ms_s / B, 3), "batched_ms_per_conversation": round(ms_b / B, 3), "speedup": round(ms_s / ms_b, 3),
                              "separate_rows_per_s": round(rows / ms_s * 1e3), "batched_rows_per_s": round(rows / ms_b * 1e3),
                              "separate_runs": [round(x, 3) for x in sep], "batched_runs": [round(x, 3) for x in bat]}), flush=True)
        for e in embs:
            lib.minigpt4_free_embedding(e)
        lib.minigpt4_free(ctx)


if __name__ == "__main__":
    main()
