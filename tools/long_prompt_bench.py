#!/usr/bin/env python3
"""What a prompt chunk past the LDS-row attention kernels' range costs (k_attn_prefill_s, csrc/attn_stream.hip).  One JSON line per measurement: medians of --reps
(>= 5) alternated runs with max - min behind them, every run printed.
  kernel   the attention launch alone on a synthetic cache (minigpt4_amd_bench_attn_prefill, 40 heads x 128, 512 rows, hipEvent time per launch): the streaming form
           (form 5) against k_attn_prefill_h8 (form 1) with the last key at 1536, where both serve, and the streaming form alone with the last key at 2048 and 4096
  chunk    bench.py's synthetic 13B Q5_K_M / 7B Q4_0 file: the 512-row chunk whose last key is at 2048 (n_ctx 2048) and at 4096 (n_ctx 4096), wall clock of
           amd_eval_tokens + amd_logits around minigpt4_amd_sync; the conversation is rebuilt before every run.  With --parent-lib (a libminigpt4.so built from the
           parent commit, where such a chunk runs one k_attn_llm workgroup per row and head) every run is a child process per library, alternated.
    python tools/long_prompt_bench.py [--config 13b,7b] [--reps 5] [--parent-lib PATH] [--skip-kernel] [--skip-chunk]        GPU only."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkg  # noqa: E402

LAST_KEYS = (2048, 4096)
ROWS = 512


def stat(x):
    return [round(float(np.median(x)), 3), round(float(max(x) - min(x)), 3)]


def kernel_arms(lib, reps):
    L = lib.library
    L.minigpt4_amd_bench_attn_prefill.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_float)]

    def arm(form, last):
        def run():
            os.environ["MINIGPT4_ATTN_PREFILL_FORM"] = str(form)
            us = ctypes.c_float()
            rc = L.minigpt4_amd_bench_attn_prefill(40, 128, ROWS, last - ROWS, 50, ctypes.byref(us))
            if rc:
                raise RuntimeError(f"bench_attn_prefill rc={rc}")
            return us.value
        return run
    arms = {"h8_1536": arm(1, 1536), "stream_1536": arm(5, 1536), "stream_2048": arm(5, 2048), "stream_4096": arm(5, 4096)}
    for fn in arms.values():
        fn()
    runs = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            runs[k].append(fn())
    os.environ.pop("MINIGPT4_ATTN_PREFILL_FORM", None)
    print(json.dumps({"measure": "kernel", "unit": "us per launch", "heads": 40, "hd": 128, "rows": ROWS, "median_spread": {k: stat(v) for k, v in runs.items()},
                      "runs": {k: [round(x, 2) for x in v] for k, v in runs.items()}}), flush=True)


def chunk_once(lib, config, reps):
    """-> {last key: [ms per run]} of this process's library"""
    import bench
    vp, lp, _, _ = bench.make_models(config, 0, 1, lambda: None)
    rng = np.random.default_rng(3)
    out = {}
    for last in LAST_KEYS:
        ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=last, n_batch=ROWS)
        try:
            toks = [1] + rng.integers(3, 30000, last - 1).tolist()
            ms = []
            for rep in range(reps + 1):                                  # the first round is the warm-up
                lib.minigpt4_reset_chat(ctx)
                for i in range(0, last - ROWS, ROWS):
                    lib.amd_eval_tokens(ctx, toks[i:i + ROWS])
                lib.amd_logits(ctx)
                lib.library.minigpt4_amd_sync(ctx.ptr)
                t0 = time.perf_counter()
                lib.amd_eval_tokens(ctx, toks[last - ROWS:])
                lib.amd_logits(ctx)
                lib.library.minigpt4_amd_sync(ctx.ptr)
                if rep:
                    ms.append((time.perf_counter() - t0) * 1e3)
            out[last] = ms
        finally:
            lib.minigpt4_free(ctx)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="13b,7b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-chunk", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)   # one run per last key of one config, as JSON
    args = ap.parse_args()
    _pkg.load_package()
    from minigpt4_cpp_amd import minigpt4_library as ML
    lib = ML.load_library()
    if lib.amd_device_count() <= 0:
        raise SystemExit("long_prompt_bench.py: no HIP device visible")
    if args.child:
        print("CHILD " + json.dumps({str(k): v[0] for k, v in chunk_once(lib, args.child, 1).items()}), flush=True)
        return
    if not args.skip_kernel:
        kernel_arms(lib, args.reps)
    for config in [] if args.skip_chunk else args.config.split(","):
        if not args.parent_lib:
            runs = {"this": chunk_once(lib, config, args.reps)}
        else:
            runs = {"parent": {k: [] for k in LAST_KEYS}, "this": {k: [] for k in LAST_KEYS}}
            for _ in range(args.reps):
                for arm, path in (("parent", args.parent_lib), ("this", None)):
                    env = dict(os.environ)
                    if path:
                        env["MINIGPT4_LIBRARY"] = os.path.abspath(path)
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config], env=env, capture_output=True, text=True, check=True, timeout=600)
                    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])
                    for k in LAST_KEYS:
                        runs[arm][k].append(got[str(k)])
        for last in LAST_KEYS:
            print(json.dumps({"measure": "chunk", "unit": "ms", "config": config, "rows": ROWS, "last_key": last, "median_spread": {a: stat(r[last]) for a, r in runs.items()},
                              "runs": {a: [round(x, 2) for x in r[last]] for a, r in runs.items()}}), flush=True)


if __name__ == "__main__":
    main()
