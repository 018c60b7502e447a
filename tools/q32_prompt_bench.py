#!/usr/bin/env python3
"""What a prompt pass and a batched step cost on a 7B file whose 2-D weights are Q8_0, Q5_0, Q5_1 or Q4_1 (k_mmq2_q32, csrc/mmq2_q32.hip) Q2_K (--formats q2_k:
k_mmq2_q2k, csrc/mmq2_q2k.hip) or Q3_K (--formats q3_k: the native 3.4-bit planes and k_mmq2_q3k, csrc/mmq2_q3k.hip; before them a Q6_K image of the file); before the
other kernels: k_mul_mat<T, 2, 4>, one pass over the weights per four rows.
One JSON line per format: medians of --reps (>= 5) alternated runs with max - min behind them, every run printed.
  p142 / p512   wall clock in ms of amd_eval_tokens + amd_logits around minigpt4_amd_sync for a 142-row (the image turn's size) and a 512-row prompt on an empty conversation
  b4 / b8       ms per step of 16 greedy amd_end_chat_batch steps of 4 / 8 conversations (short prompts evaluated beforehand)
  dec           ms per step of 64 greedy one-conversation decode steps (amd_decode_loop) behind a 16-token prompt
  mem           MiB of device memory the process holds after minigpt4_model_load (hipMemGetInfo before / after)
The files are synthetic (modelgen.headline_llm's conditioning, every 2-D tensor in the format); every run is a child process that loads the file, warms each measurement
up once and measures it once.  With --parent-lib (a libminigpt4.so built from the parent commit) the runs alternate, parent first in each pair.
    python tools/q32_prompt_bench.py [--formats q8_0,q5_0,q5_1,q4_1 | q2_k | q3_k] [--reps 5] [--parent-lib PATH]        GPU only."""
import argparse
import ctypes
import dataclasses
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkg  # noqa: E402

FTYPE = {"q8_0": 7, "q5_0": 8, "q5_1": 9, "q4_1": 3, "q2_k": 10, "q3_k": 11}
MEASURES = ("p142", "p512", "b4", "b8", "dec", "mem")
B, STEPS, DEC_STEPS = 8, 16, 64


def stat(x):
    return [round(float(np.median(x)), 3), round(float(max(x) - min(x)), 3)]


def files(fmt):
    """(vision file, 7B LLM file of the format) in bench.py's model directory, written once"""
    import bench
    from minigpt4_cpp_amd import modelgen as G
    vp = os.path.join(bench.model_dir(), "vision_7b.bin")
    if not os.path.exists(vp + ".ok"):
        G.write_vision_file(vp, G.vision_7b(), seed=4321, std=0.02, unique_blocks=1, fast=True)
        open(vp + ".ok", "w").write("ok")
    cfg, kw = G.headline_llm("7b_q8_0")
    lp = os.path.join(bench.model_dir(), f"llm_7b_{fmt}_q32bench.bin")
    if not os.path.exists(lp + ".ok"):
        G.write_llm_file(lp, dataclasses.replace(cfg, wtype=fmt, ftype=FTYPE[fmt]), **kw)
        open(lp + ".ok", "w").write("ok")
    return vp, lp


def measure_once(lib, fmt):
    """-> {measure: ms} of this process's library"""
    vp, lp = files(fmt)
    rng = np.random.default_rng(3)
    toks = [1] + rng.integers(3, 30000, 511).tolist()
    hip = ctypes.CDLL("libamdhip64.so")

    def free_mib():
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value / 2 ** 20
    before = free_mib()
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=1024, n_batch=512)
    sync = lambda: lib.library.minigpt4_amd_sync(ctx.ptr)   # noqa: E731
    out = {"mem": before - free_mib()}
    try:
        for rows in (142, 512):
            for rep in range(2):                                         # the first round is the warm-up
                lib.minigpt4_reset_chat(ctx)
                sync()
                t0 = time.perf_counter()
                lib.amd_eval_tokens(ctx, toks[:rows])
                lib.amd_logits(ctx)
                sync()
                out[f"p{rows}"] = (time.perf_counter() - t0) * 1e3
        for rep in range(2):
            lib.minigpt4_reset_chat(ctx)
            lib.amd_eval_tokens(ctx, toks[:16])
            lib.amd_decode_loop(ctx, 8)
            sync()
            t0 = time.perf_counter()
            lib.amd_decode_loop(ctx, DEC_STEPS)
            sync()
            out["dec"] = (time.perf_counter() - t0) * 1e3 / DEC_STEPS
        lib.amd_set_conversations(ctx, B)
        for nb in (4, B):
            for rep in range(2):
                for s in range(nb):
                    lib.amd_select_conversation(ctx, s)
                    lib.minigpt4_reset_chat(ctx)
                    lib.amd_eval_tokens(ctx, toks[:4 + s])
                    lib.amd_logits(ctx)
                lib.amd_select_conversation(ctx, 0)
                lib.amd_end_chat_batch(ctx, list(range(nb)), temp=0.0)   # the first step of a round builds what the later ones replay
                sync()
                t0 = time.perf_counter()
                for _ in range(STEPS):
                    lib.amd_end_chat_batch(ctx, list(range(nb)), temp=0.0)
                sync()
                out[f"b{nb}"] = (time.perf_counter() - t0) * 1e3 / STEPS
    finally:
        lib.minigpt4_free(ctx)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", default="q8_0,q5_0,q5_1,q4_1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)   # one run per measure of one format, as JSON
    args = ap.parse_args()
    _pkg.load_package()
    from minigpt4_cpp_amd import minigpt4_library as ML
    lib = ML.load_library()
    if lib.amd_device_count() <= 0:
        raise SystemExit("q32_prompt_bench.py: no HIP device visible")
    if args.child:
        print("CHILD " + json.dumps(measure_once(lib, args.child)), flush=True)
        return
    for fmt in args.formats.split(","):
        files(fmt)
        arms = ([("parent", os.path.abspath(args.parent_lib))] if args.parent_lib else []) + [("this", None)]
        runs = {a: {k: [] for k in MEASURES} for a, _ in arms}
        for _ in range(args.reps):
            for arm, path in arms:
                env = dict(os.environ)
                if path:
                    env["MINIGPT4_LIBRARY"] = path
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", fmt], env=env, capture_output=True, text=True, timeout=600)
                if r.returncode:
                    raise SystemExit(f"q32_prompt_bench.py: the {arm} run on {fmt} ended with {r.returncode}:\n{r.stderr[-2000:]}")
                got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])
                for k in MEASURES:
                    runs[arm][k].append(got[k])
        print(json.dumps({"format": fmt, "unit": "ms (b4, b8, dec: per step; mem: MiB)", "median_spread": {a: {k: stat(v) for k, v in r.items()} for a, r in runs.items()},
                          "runs": {a: {k: [round(x, 2) for x in v] for k, v in r.items()} for a, r in runs.items()}}), flush=True)


if __name__ == "__main__":
    main()
