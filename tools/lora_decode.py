#!/usr/bin/env python3
"""What a run-time LoRA adapter costs: the decode step, the image turn's prompt pass and batched steps with no adapter loaded, a q,v rank-64 adapter and an all-seven
rank-16 adapter, every variant in its own process, the variants alternated, medians over the runs.
usage: tools/lora_decode.py [--config 13b] [--runs 5] [--steps 64] [--only decode|batch]
Expectation stated before measuring: 2 launches per adapted site group per layer at about 5 us each (the project's dependent-launch figure), i.e. +80 launches per token
for a q,v adapter on 13B (+0.4 ms), +320 for all seven targets (4 site groups).  The kernels alone: the "lora" rows of the eager per-site table (one k_lora_down + one
k_lora_up per row)."""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ADAPTERS = {"none": None, "qv_r64": (64, ("attn_q", "attn_v")), "all7_r16": (16, ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_down", "ffn_up"))}


def child(config, what, B, n_adapters, steps):
    import _pkg
    _pkg.load_package()
    import bench
    from minigpt4_cpp_amd import minigpt4_library as ML, modelgen as G
    lib = ML.load_library()
    vp, lp, vcfg, lcfg = bench.make_models(config, 0, 1, lambda: None)
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, seed=1337, n_ctx=2048, n_batch=512)
    handles = []
    if ADAPTERS[what]:
        rank, targets = ADAPTERS[what]
        for a in range(max(n_adapters, 1)):
            ap = os.path.join(os.path.dirname(lp), f"lora_{config}_{what}_{a}.gguf")
            if not os.path.exists(ap):
                G.write_lora_gguf(ap, lcfg, rank=rank, alpha=float(rank), targets=targets, seed=50 + a, std_a=0.01, std_b=0.01)
            handles.append(lib.amd_adapter_load(ctx, ap))
    emb = lib.minigpt4_encode_image(ctx, ML.array_to_image_struct(G.synth_image(42)))
    lib.amd_set_conversations(ctx, B)
    prefill = []
    for sl in range(B):
        lib.amd_select_conversation(ctx, sl)
        if handles and n_adapters:
            lib.amd_set_adapter(ctx, sl, handles[sl % n_adapters])
        lib.minigpt4_system_prompt(ctx)
        lib.library.minigpt4_amd_sync(ctx.ptr)
        t0 = time.perf_counter()
        lib.minigpt4_begin_chat_image(ctx, emb, bench.PROMPT)
        lib.library.minigpt4_amd_sync(ctx.ptr)
        prefill.append((time.perf_counter() - t0) * 1e3)
    lib.amd_select_conversation(ctx, 0)
    step = (lambda: lib.minigpt4_end_chat_image(ctx, temp=0.0)) if B == 1 else (lambda: lib.amd_end_chat_batch(ctx, list(range(B)), temp=0.0))
    for _ in range(8):
        step()
    lib.library.minigpt4_amd_sync(ctx.ptr)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    lib.library.minigpt4_amd_sync(ctx.ptr)
    dt = time.perf_counter() - t0
    out = {"ms_step": dt * 1e3 / steps, "tok_s": B * steps / dt, "prompt_ms": min(prefill)}
    if B == 1 and handles:
        rows = [s for s in lib.amd_profile_sites(ctx, 8)["sites"] if s["site"] == "lora"]
        calls = sum(s["calls_per_step"] for s in rows)
        out.update(lora_pairs_per_step=calls, lora_pair_us=sum(s["avg_us"] * s["calls_per_step"] for s in rows) / max(calls, 1e-9))
    print(json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1], args[2], int(args[3]), int(args[4]), int(args[5]))
    config, runs, steps, only = "13b", 5, 64, None
    while args:
        if args[0] == "--config": config = args[1]
        elif args[0] == "--runs": runs = int(args[1])
        elif args[0] == "--steps": steps = int(args[1])
        elif args[0] == "--only": only = args[1]
        args = args[2:]
    variants = []
    if only in (None, "decode"):
        variants += [(f"decode {w}", w, 1, 1) for w in ADAPTERS]
    if only in (None, "batch"):
        variants += [(f"batch B={B} on {n} adapters", "qv_r64" if n else "none", B, n) for B in (4, 32) for n in (0, 1, 2)]
    got = {v[0]: [] for v in variants}
    for _ in range(runs):                                                      # alternated: every variant once per round
        for name, what, B, n in variants:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config, what, str(B), str(n), str(steps)], capture_output=True, text=True, timeout=600)
            line = [l for l in p.stdout.splitlines() if l.startswith("{")]
            if not line:
                print(f"{name}: FAILED rc={p.returncode} {p.stderr[-400:]}", flush=True)
                return 1
            got[name].append(json.loads(line[-1]))
            print(f"{name:32s} {line[-1]}", flush=True)
    print(f"\nmedians of {runs} alternated runs, {config}, {steps} steps")
    for name, rs in got.items():
        print(f"| {name} | " + " | ".join(f"{k} {statistics.median(r[k] for r in rs):.3f}" for k in rs[0]) + " |")


if __name__ == "__main__":
    sys.exit(main())
