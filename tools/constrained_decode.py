#!/usr/bin/env python3
"""What constrained decoding costs (minigpt4_amd_constraint_compile / _set_constraint; kernels k_constrain_index, k_constrain_pick).  Files: --vision / --llm, or bench.py's
synthetic files (--config 13b | 7b | tiny).  One JSON line per measurement: medians of --reps (>= 5) alternated runs with max - min next to them, every run printed.
  a  the index build against S: minigpt4_amd_constraint_compile (host compile + upload + k_constrain_index + synchronise, wall-clock ms) for patterns of 2 .. 1024
       states on the loaded vocabulary, and k_constrain_index alone (the test library's hook, hipEvent time) on the 32 001-piece synthetic vocabulary.
  b  k_constrain_pick alone against k_pen_pick alone (hooks, hipEvent time of one launch) on the same 1, 4, 32 rows of 32 001 floats, with the same penalty tables.
  c  greedy tokens per second, unconstrained against constrained ([ -~]* : printable ASCII, so the constraint never ends the text): one conversation through
       minigpt4_end_chat, and minigpt4_amd_end_chat_batch at B = 4 and B = 32.
    python tools/constrained_decode.py [--config 13b] [--legs a,b,c] [--reps 5] [--steps 32]   GPU only."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkg  # noqa: E402

FREE_TEXT = "[ -~]*"
BY_STATES = [("", 2), ("(yes|no)", 6), ("[0-9]{30}", 32), ("[a-z]{126}", 128), ("a{255}b{255}", 512), ("a{255}b{255}c{255}d{255}e{2}", 1024)]


def stat(x, nd=3):
    return dict(median=round(float(np.median(x)), nd), spread=round(float(max(x) - min(x)), nd), runs=[round(float(v), nd) for v in x])


def prompt_ids(n_vocab, seed, n=64):
    return [1] + [int(v) for v in np.random.default_rng(seed).integers(3, n_vocab, n - 1)]


def leg_index(lib, ctx, reps):
    from minigpt4_cpp_amd import modelgen as G
    pieces = [p for p, _ in G.synth_vocab(32001)]
    for pattern, states in BY_STATES:
        trans, acc, S = lib.amd_test_constraint_compile(pattern)
        assert S == states, (pattern, S)
        t0 = time.perf_counter()
        for _ in range(20):
            lib.amd_test_constraint_compile(pattern)
        host_ms = 1e3 * (time.perf_counter() - t0) / 20
        kernel = [lib.amd_test_constrain_index(pieces, trans, acc)[1] for _ in range(reps + 1)][1:]
        whole = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            h = lib.amd_constraint_compile(ctx, pattern)
            whole.append(1e3 * (time.perf_counter() - t0))
            lib.amd_constraint_free(ctx, h)
        print(json.dumps({"leg": "a", "what": "index build", "states": S, "pattern": pattern, "host_compile_ms": round(host_ms, 3),
                          "k_constrain_index_us_V32001": stat([1e3 * v for v in kernel], 1), "constraint_compile_ms": stat(whole[1:])}), flush=True)


def leg_kernels(lib, reps, V=32001):
    rng = np.random.default_rng(1)
    f32 = lambda v: int(np.float32(v).view(np.int32))                        # noqa: E731
    for n in (1, 4, 32):
        buf = (3.0 * rng.standard_normal((n, V))).astype(np.float32)
        rows, table = [], []
        for r in range(n):                                                   # 64 window ids per row, repeat_penalty 1.3
            ids = sorted(int(i) for i in rng.choice(V, 64, replace=False))
            rows.append([r, len(table), 64, 1, f32(1.3), f32(0.0), f32(0.0), 0])
            table += [[i, 1, 0, 0] for i in ids]
        allowed = (rng.random((n, ((V + 31) // 32 + 3) // 4 * 4 * 32)) < 0.5)
        allowed[:, V:] = False
        bitmaps = np.packbits(allowed, axis=1, bitorder="little").view(np.uint32)
        out = {"pen": [], "con": []}
        for _ in range(reps + 1):
            out["pen"].append(lib.amd_test_pen_pick(buf, V, np.array(rows, np.int32), np.array(table, np.int32))[2])
            out["con"].append(lib.amd_test_constrain_pick(buf, V, np.array(rows, np.int32), np.array(table, np.int32), bitmaps, list(range(n)))[2])
        print(json.dumps({"leg": "b", "what": "one launch, hipEvent time", "rows": n, "n_vocab": V, "table_entries_per_row": 64,
                          "k_pen_pick_us": stat([1e3 * v for v in out["pen"][1:]], 1), "k_constrain_pick_us": stat([1e3 * v for v in out["con"][1:]], 1)}), flush=True)


def leg_decode(lib, ctx, n_vocab, reps, steps):
    handle = lib.amd_constraint_compile(ctx, FREE_TEXT)
    for B in (1, 4, 32):
        lib.amd_set_conversations(ctx, B)
        slots = list(range(B))

        def timed(constrained):
            for k in slots:
                lib.amd_select_conversation(ctx, k)
                lib.minigpt4_reset_chat(ctx)
                lib.amd_set_constraint(ctx, k, handle if constrained else 0)
                lib.amd_eval_tokens(ctx, prompt_ids(n_vocab, 10 + k))
            lib.amd_select_conversation(ctx, 0)
            if B > 1:
                lib.amd_prefill_batch(ctx, slots)
            lib.library.minigpt4_amd_sync(ctx.ptr)
            t0 = time.perf_counter()
            for _ in range(steps):
                if B == 1:
                    lib.minigpt4_end_chat(ctx, temp=0.0)
                else:
                    lib.amd_end_chat_batch(ctx, slots, temp=0.0)
            lib.library.minigpt4_amd_sync(ctx.ptr)
            return B * steps / (time.perf_counter() - t0)

        out = {False: [], True: []}
        for c in (False, True):                                              # warm-up: the graph captured
            timed(c)
        before = lib.amd_constraint_info(ctx)
        for _ in range(reps):
            for c in (False, True):
                out[c].append(timed(c))
        after = lib.amd_constraint_info(ctx)
        print(json.dumps({"leg": "c", "what": "greedy tok/s, host wall-clock", "conversations": B, "steps": steps,
                          "call": "minigpt4_end_chat" if B == 1 else "minigpt4_amd_end_chat_batch", "unconstrained": stat(out[False], 2), "constrained": stat(out[True], 2),
                          "ms_per_step_added": round(1e3 * B * (1 / np.median(out[True]) - 1 / np.median(out[False])), 4),
                          "pick_launches_per_constrained_step": (after["pick_launches"] - before["pick_launches"]) / (reps * steps), "stuck": after["stuck"]}), flush=True)
    for k in range(32):
        lib.amd_set_constraint(ctx, k, 0)
    lib.amd_constraint_free(ctx, handle)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="13b", help="bench.py's synthetic files (ignored with --vision / --llm)")
    ap.add_argument("--vision")
    ap.add_argument("--llm")
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--n-ctx", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=32)
    args = ap.parse_args()
    _pkg.load_package()
    from minigpt4_cpp_amd import minigpt4_library as ML
    lib = ML.load_library()
    if lib.amd_device_count() <= 0:
        raise SystemExit("constrained_decode.py: no HIP device visible")
    if bool(args.vision) != bool(args.llm):
        raise SystemExit("constrained_decode.py: --vision and --llm go together")
    legs = set(args.legs.split(","))
    reps = max(5, args.reps)
    if "b" in legs:
        leg_kernels(lib, reps)
    if legs & {"a", "c"}:
        import bench
        vp, lp = (args.vision, args.llm) if args.llm else bench.make_models(args.config, 0, 1, lambda: None)[:2]
        ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=args.n_ctx, n_batch=512)
        try:
            n_vocab = lib.library.minigpt4_amd_n_vocab(ctx.ptr)
            print(json.dumps({"config": args.config, "llm": os.path.basename(lp), "n_vocab": n_vocab, "n_ctx": args.n_ctx, "reps": reps}), flush=True)
            if "a" in legs:
                leg_index(lib, ctx, reps)
            if "c" in legs:
                leg_decode(lib, ctx, n_vocab, reps, args.steps)
        finally:
            lib.minigpt4_free(ctx)


if __name__ == "__main__":
    main()
