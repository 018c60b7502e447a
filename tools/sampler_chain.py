#!/usr/bin/env python3
"""What the extended sampling rule costs on the device (minigpt4_amd_end_chat_batch_sampled_ex; kernel k_sample_rows_ex: tail-free, typical, top-p, min-p, mirostat v2 with
one mu per conversation).  Files: --vision / --llm, or bench.py's synthetic files (--config 13b | 7b | tiny).  temp 0.8, top-k 40, top-p 0.9 (the reference's defaults).
One JSON line per measurement: medians of --reps (>= 5) alternated runs with max - min next to them, every run printed.
  a  the kernel alone (the test library's hooks: hipEvent time of one launch) at 1, 4, 32 rows of 32 001 floats: k_sample_rows, and k_sample_rows_ex with neutral values,
     with each filter on, with all of them and with mirostat v2.
  b  B = 1, 4, 32 conversations, host wall-clock ms per step over --steps steps, per parameter set:
       plain      minigpt4_amd_end_chat_batch_sampled (neutral values only: the path that existed before);
       device     minigpt4_amd_end_chat_batch_sampled_ex with the set;
       host       minigpt4_amd_end_chat_batch with the same parameters (the host chain: one logits row, one synchronise and one sort per conversation; it has no min_p,
                  so that set has no host arm) -- the arm to beat.
     The mirostat set is the device's mirostat v2 over 40 candidates against the host chain's over the whole vocabulary.
    python tools/sampler_chain.py [--config 13b] [--legs a,b] [--reps 5] [--steps 32]   GPU only."""
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
SETS = [("neutral", {}), ("tail_free", dict(tfs_z=0.95)), ("typical", dict(typical_p=0.9)), ("min_p", dict(min_p=0.05)),
        ("all_four", dict(tfs_z=0.95, typical_p=0.9, min_p=0.05)), ("mirostat_v2", dict(mirostat=2, mirostat_tau=5.0, mirostat_eta=0.1))]


def stat(x, nd=3):
    return dict(median=round(float(np.median(x)), nd), spread=round(float(max(x) - min(x)), nd), runs=[round(float(v), nd) for v in x])


def prompt_ids(n_vocab, seed, n=64):
    return [1] + [int(v) for v in np.random.default_rng(seed).integers(3, n_vocab, n - 1)]


def chain_row(kw):
    return [kw.get("tfs_z", 1.0), kw.get("typical_p", 1.0), kw.get("min_p", 0.0), kw.get("mirostat", 0), kw.get("mirostat_tau", 5.0), kw.get("mirostat_eta", 0.1), float("nan")]


def leg_kernel(lib, reps, V=32001):
    rng = np.random.default_rng(1)
    for n in (1, 4, 32):
        buf = (3.0 * rng.standard_normal((n, V))).astype(np.float32)
        rows = np.zeros((n, 8), np.int32)
        rows[:, 0] = np.arange(n)
        table = np.zeros((0, 4), np.int32)
        sd = np.array([(1000 + r, 0) for r in range(n)], np.uint64)
        args = (buf, V, rows, table, [(TEMP, TOP_P)] * n, [TOP_K] * n, sd)
        runs = {"k_sample_rows": []}
        runs.update({"k_sample_rows_ex " + name: [] for name, _ in SETS})
        for _ in range(reps + 1):                                    # alternated; the first round is the warm-up
            runs["k_sample_rows"].append(lib.amd_test_sample_rows(*args)["ms"])
            for name, kw in SETS:
                runs["k_sample_rows_ex " + name].append(lib.amd_test_sample_rows_ex(*args, [chain_row(kw)] * n)["ms"])
        print(json.dumps({"leg": "a", "what": "one launch, hipEvent time, us", "rows": n, "n_vocab": V, **{k: stat([1e3 * v for v in ms[1:]], 1) for k, ms in runs.items()}}),
              flush=True)


def leg_steps(lib, ctx, n_vocab, reps, steps, B):
    lib.amd_set_conversations(ctx, B)
    slots = list(range(B))

    def prompts():
        for k in slots:
            lib.amd_select_conversation(ctx, k)
            lib.minigpt4_reset_chat(ctx)
            lib.amd_eval_tokens(ctx, prompt_ids(n_vocab, 10 + k))
            lib.amd_conversation_mirostat(ctx, k, None)
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

    base = dict(temp=TEMP, top_k=TOP_K, top_p=TOP_P)
    for name, kw in SETS:
        arms = {"device": lambda: lib.amd_end_chat_batch_sampled(ctx, slots, _extended=True, **base, **kw)}
        if not kw:
            arms["plain"] = lambda: lib.amd_end_chat_batch_sampled(ctx, slots, **base)
        if "min_p" not in kw:
            arms["host"] = lambda: lib.amd_end_chat_batch(ctx, slots, **base, **kw)
        out = {k: [] for k in arms}
        for f in arms.values():                                       # warm-up: the graph captured, the buffers allocated
            timed(f)
        for _ in range(reps):
            for k, f in arms.items():
                out[k].append(timed(f))
        med = {k: float(np.median(v)) for k, v in out.items()}
        line = {"leg": "b", "what": "ms per step, host wall-clock", "set": name, "B": B, "steps": steps, **{k: stat(v) for k, v in out.items()},
                "tok_per_s": {k: round(1e3 * B / v, 1) for k, v in med.items()}}
        if "host" in med:
            line["host_minus_device_ms"] = round(med["host"] - med["device"], 3)
        if "plain" in med:
            line["device_minus_plain_ms"] = round(med["device"] - med["plain"], 3)
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
        raise SystemExit("sampler_chain.py: no HIP device visible")
    if bool(args.vision) != bool(args.llm):
        raise SystemExit("sampler_chain.py: --vision and --llm go together")
    legs = set(args.legs.split(","))
    reps = max(5, args.reps)
    if "a" in legs:
        leg_kernel(lib, reps)
    if "b" in legs:
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


if __name__ == "__main__":
    main()
