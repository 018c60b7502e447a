#!/usr/bin/env python3
"""What beam search costs per step (minigpt4_amd_beam_search; kernels k_beam_select, k_kv_permute).  Files: --vision / --llm, or bench.py's synthetic files
(--config 13b | 7b | tiny), n_ctx 2048.  One JSON line per measurement: medians of --reps (>= 5) alternated runs with max - min next to them, every run printed.
  a  W = 2, 4, 8 beams: host wall-clock ms per step of one minigpt4_amd_beam_search call of --steps steps (k_topn_rows + k_beam_select + k_kv_permute + the batched pass
     at W rows + the result block's read-back) against ms per step of minigpt4_amd_end_chat_batch(temp 0) at B = W -- the same pass without the search; next to them the
     call's statistics: permute launches that were not the identity, cache rows moved per step.
  b  k_kv_permute alone (the test library's hook: hipEvent time of one launch) at the 13B (40 layers x 5120) and 7B (32 x 4096) cache shapes: W conversations, a full
     cycle (every conversation takes another one's rows), --rows rows; GB/s counts every byte read and written.
    python tools/beam_decode.py [--config 13b] [--legs a,b] [--reps 5] [--steps 32] [--rows 64]   GPU only."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkg  # noqa: E402


def stat(x, nd=3):
    return dict(median=round(float(np.median(x)), nd), spread=round(float(max(x) - min(x)), nd), runs=[round(float(v), nd) for v in x])


def prompt_ids(n_vocab, seed, n=100):
    return [1] + [int(v) for v in np.random.default_rng(seed).integers(3, n_vocab, n - 1)]


def leg_search(lib, ctx, n_vocab, reps, steps, W):
    lib.amd_set_conversations(ctx, W)
    slots = list(range(W))
    last = {}

    def prompt(k, seed):
        lib.amd_select_conversation(ctx, k)
        lib.minigpt4_reset_chat(ctx)
        lib.amd_eval_tokens(ctx, prompt_ids(n_vocab, seed))

    def beam():
        prompt(0, 1)
        lib.amd_logits(ctx)
        t0 = time.perf_counter()
        _, st = lib.amd_beam_search(ctx, slots, steps, 1.0, with_stats=True)
        dt = time.perf_counter() - t0
        last.update(st)
        return 1e3 * dt / max(st["passes"], 1)

    def batch():
        for k in slots:
            prompt(k, 10 + k)
        lib.amd_prefill_batch(ctx, slots)
        lib.library.minigpt4_amd_sync(ctx.ptr)
        t0 = time.perf_counter()
        for _ in range(steps):
            lib.amd_end_chat_batch(ctx, slots, temp=0.0)
        lib.library.minigpt4_amd_sync(ctx.ptr)
        return 1e3 * (time.perf_counter() - t0) / steps

    out = {"beam": [], "batch": []}
    beam(), batch()                                               # warm-up: graphs captured, the feature's buffers allocated
    for _ in range(reps):
        out["beam"].append(beam())
        out["batch"].append(batch())
    print(json.dumps({"leg": "a", "what": "ms per step, host wall-clock", "W": W, "steps": steps, "beam_search": stat(out["beam"]), "end_chat_batch_B=W": stat(out["batch"]),
                      "passes": last.get("passes"), "permute_launches_not_identity": last.get("permutes"),
                      "rows_moved_per_step": round(last.get("rows_moved", 0) / max(last.get("passes", 1), 1), 2), "finished_by_eos": last.get("finished")}), flush=True)


def leg_kernel(lib, reps, rows, n_ctx=256):
    for name, n_layer, E in (("13b", 40, 5120), ("7b", 32, 4096)):
        for W in (2, 4, 8):
            cycle = [(i + 1) % W for i in range(W)]
            ms = [lib.amd_test_kv_permute_ms(W, n_layer, n_ctx, E, list(range(W)), cycle, 0, rows) for _ in range(reps + 1)][1:]
            moved = 2.0 * W * 2 * n_layer * rows * E * 2         # read + write, W conversations, keys + values, fp16
            print(json.dumps({"leg": "b", "what": "k_kv_permute alone, one launch, full cycle", "shape": name, "W": W, "rows": rows, "MB_read_and_written": round(moved / 1e6, 1),
                              "us": stat([1e3 * v for v in ms], 1), "GB_per_s": stat([moved / (v * 1e-3) / 1e9 for v in ms], 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="13b", help="bench.py's synthetic files (ignored with --vision / --llm)")
    ap.add_argument("--vision")
    ap.add_argument("--llm")
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--n-ctx", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rows", type=int, default=64)
    args = ap.parse_args()
    _pkg.load_package()
    from minigpt4_cpp_amd import minigpt4_library as ML
    lib = ML.load_library()
    if lib.amd_device_count() <= 0:
        raise SystemExit("beam_decode.py: no HIP device visible")
    if bool(args.vision) != bool(args.llm):
        raise SystemExit("beam_decode.py: --vision and --llm go together")
    legs = set(args.legs.split(","))
    reps = max(5, args.reps)
    if "a" in legs:
        import bench
        vp, lp = (args.vision, args.llm) if args.llm else bench.make_models(args.config, 0, 1, lambda: None)[:2]
        ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=args.n_ctx, n_batch=512)
        try:
            n_vocab = lib.library.minigpt4_amd_n_vocab(ctx.ptr)
            print(json.dumps({"config": args.config, "llm": os.path.basename(lp), "n_vocab": n_vocab, "reps": reps}), flush=True)
            for W in (2, 4, 8):
                leg_search(lib, ctx, n_vocab, reps, args.steps, W)
        finally:
            lib.minigpt4_free(ctx)
    if "b" in legs:
        leg_kernel(lib, reps, args.rows)


if __name__ == "__main__":
    main()
