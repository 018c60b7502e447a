#!/usr/bin/env python3
"""What reusing cached K / V rows buys (minigpt4_amd_set_prefix_cache, minigpt4_amd_fork_conversation).  Files: the 13B Q5_K_M headline file and the 7B Q4_0 file
(bench.py's synthetic files), n_ctx 2048, n_batch 512.  Both arms of every leg are warmed up, then timed alternately in one process with minigpt4_amd_sync around
them; one JSON line per leg with the median and the runs of each arm.
  a  image-turn prompt pass (system prompt + image turn, ~142 rows), one conversation: prefix cache off against on (after the capture)
  b  the same through minigpt4_amd_prefill_batch at B = 4 and 8
  c  k = 4 questions about one image: four full image turns against one image head + fork to three conversations + four question-only passes
  d  the copy kernel alone (minigpt4_amd_test_kv_copy on device buffers, hipEvent time) in the engine's layouts at the 13B / 7B widths -- conversations with 2048 rows
     per layer, the store with 256; from a conversation (fork) and from the store (hit); 45 and 142 rows, 1 and 4 destinations: ms, GB/s (bytes read + written), share of
     the 6.29 TB/s device copy peak -- alternated with 2 x n_dst hipMemcpy2DAsync calls doing the same copy (the baseline the kernel has to beat)
    python tools/prefix_cache_bench.py [--configs 13b,7b] [--legs a,b,c,d] [--reps 5]   GPU only."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkg  # noqa: E402

COPY_PEAK = 6.29e12
QUESTIONS = ["what is in the picture?", "describe the colours", "is there any text?", "how many objects are there?"]


def med(x):
    return round(float(np.median(x)), 3)


def runs(x):
    return [round(float(v), 3) for v in x]


def alternate(reps, arms):
    """arms: {name: fn() -> ms}; every arm once as warm-up, then `reps` rounds in turn."""
    for fn in arms.values():
        fn()
    out = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            out[k].append(fn())
    return out


def engine_legs(lib, ML, G, bench, config, legs, reps):
    vp, lp, _, _ = bench.make_models(config, 0, 1, lambda: None)
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=2048, n_batch=512)
    lib.amd_set_conversations(ctx, 8)
    embs = [lib.minigpt4_encode_image(ctx, ML.array_to_image_struct(G.synth_image(7 + i))) for i in range(8)]
    sync = lambda: lib.library.minigpt4_amd_sync(ctx.ptr)  # noqa: E731
    n_embd = lib.library.minigpt4_amd_n_embd(ctx.ptr)

    def queue(B):
        for s in range(B):
            lib.amd_select_conversation(ctx, s)
            lib.minigpt4_reset_chat(ctx)
            lib.minigpt4_system_prompt(ctx)
            lib.minigpt4_begin_chat_image(ctx, embs[s], QUESTIONS[s % 4])
        lib.amd_select_conversation(ctx, 0)

    def pass_ms(B, cache, batched):
        lib.amd_set_prefix_cache(ctx, 256 if cache else 0)
        if cache:                                               # the capture: not part of the timed pass
            queue(1)
            sync()
        queue(B)                                                # host-side queues only: nothing is launched before t0
        t0 = time.perf_counter()
        if batched:
            lib.amd_prefill_batch(ctx, list(range(B)))
        sync()
        ms = (time.perf_counter() - t0) * 1e3
        pass_ms.info = lib.amd_prefix_cache_info(ctx)
        return ms

    for leg, B, batched in (("a", 1, False), ("b", 4, True), ("b", 8, True)):
        if leg not in legs:
            continue
        r = alternate(reps, {"off": lambda: pass_ms(B, False, batched), "on": lambda: pass_ms(B, True, batched)})
        pass_ms(B, True, batched)
        lib.amd_select_conversation(ctx, 0)
        print(json.dumps({"leg": leg, "config": config, "B": B, "rows_per_conversation": lib.library.minigpt4_amd_n_past(ctx.ptr), "cache_off_ms": med(r["off"]),
                          "cache_on_ms": med(r["on"]), "delta_ms": round(med(r["on"]) - med(r["off"]), 3), "rows_reused_by_last_pass": pass_ms.info["rows_reused_by_last_pass"],
                          "cache_off_runs": runs(r["off"]), "cache_on_runs": runs(r["on"])}), flush=True)

    if "c" in legs:
        lib.amd_set_prefix_cache(ctx, 0)
        tok = lambda s: lib.amd_tokenize(ctx, s.encode())  # noqa: E731
        rows = np.ctypeslib.as_array(embs[0].data, shape=(32 * n_embd,))

        def head():
            lib.minigpt4_reset_chat(ctx)
            lib.minigpt4_system_prompt(ctx)
            lib.amd_eval_tokens(ctx, tok("Human: <Img>"))
            lib.amd_eval_embd(ctx, rows)
            lib.amd_eval_tokens(ctx, tok("</Img> "))

        def question(q):
            lib.amd_eval_tokens(ctx, tok(q))
            lib.amd_eval_tokens(ctx, tok("### Assistant:"))

        def full():
            t0 = time.perf_counter()
            for s in range(4):
                lib.amd_select_conversation(ctx, s)
                head()
                question(QUESTIONS[s])
                sync()
            return (time.perf_counter() - t0) * 1e3

        def forked():
            t0 = time.perf_counter()
            lib.amd_select_conversation(ctx, 0)
            head()
            lib.amd_fork_conversation(ctx, 0, [1, 2, 3])
            for s in range(4):
                lib.amd_select_conversation(ctx, s)
                question(QUESTIONS[s])
                sync()
            return (time.perf_counter() - t0) * 1e3
        r = alternate(reps, {"full": full, "fork": forked})
        print(json.dumps({"leg": "c", "config": config, "questions": 4, "four_full_turns_ms": med(r["full"]), "one_turn_fork_four_questions_ms": med(r["fork"]),
                          "speedup": round(med(r["full"]) / med(r["fork"]), 3), "full_runs": runs(r["full"]), "fork_runs": runs(r["fork"])}), flush=True)
    for e in embs:
        lib.minigpt4_free_embedding(e)
    lib.minigpt4_free(ctx)


class Hip:
    """The few runtime calls the hipMemcpy2DAsync baseline of leg d needs."""
    def __init__(self):
        self.h = ctypes.CDLL("libamdhip64.so")
        self.h.hipMemcpy2DAsync.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        self.h.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.h.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        self.h.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        self.h.hipFree.argtypes = [ctypes.c_void_p]

    def ok(self, rc):
        if rc:
            raise RuntimeError(f"HIP call failed: {rc}")

    def malloc(self, n):
        p = ctypes.c_void_p()
        self.ok(self.h.hipMalloc(ctypes.byref(p), ctypes.c_size_t(n)))
        self.ok(self.h.hipMemset(p, 1, n))
        return p

    def copy2d_ms(self, pairs, width, height):
        """pairs: [(dst address, dst pitch, src address, src pitch)], one hipMemcpy2DAsync each (device to device) between one event pair"""
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        self.ok(self.h.hipEventCreate(ctypes.byref(a)))
        self.ok(self.h.hipEventCreate(ctypes.byref(b)))
        self.ok(self.h.hipEventRecord(a, None))
        for dst, dpitch, src, spitch in pairs:
            self.ok(self.h.hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, 3, None))   # 3 = device to device
        self.ok(self.h.hipEventRecord(b, None))
        self.ok(self.h.hipDeviceSynchronize())
        ms = ctypes.c_float()
        self.ok(self.h.hipEventElapsedTime(ctypes.byref(ms), a, b))
        self.h.hipEventDestroy(a)
        self.h.hipEventDestroy(b)
        return float(ms.value)


def kernel_leg(lib, config, reps):
    """The engine's own layouts at n_ctx = 2048: every conversation's layers are 2048 rows apart, the store's 256 (max_rows), so a prefix is n_layer separate runs per tensor.
    source "conversation" = a fork, source "store" = a cache hit.  Device buffers only (minigpt4_amd_test_kv_copy without host caches)."""
    L, E = (40, 5120) if config == "13b" else (32, 4096)
    S, C, STORE = 5, 2048, 256
    hip = Hip()
    slot_bytes, conv_pitch, store_pitch = L * C * E * 2, C * E * 2, STORE * E * 2
    kv = [hip.malloc(S * slot_bytes), hip.malloc(S * slot_bytes)]
    store = [hip.malloc(L * store_pitch), hip.malloc(L * store_pitch)]
    for source, src_rows in (("conversation", 0), ("store", STORE)):
        for n_rows in (45, 142):
            for dsts in ([1], [0, 1, 2, 3]):
                if source == "store":
                    pairs = [(kv[t].value + d * slot_bytes, conv_pitch, store[t].value, store_pitch) for t in range(2) for d in dsts]
                else:
                    pairs = [(kv[t].value + d * slot_bytes, conv_pitch, kv[t].value + 4 * slot_bytes, conv_pitch) for t in range(2) for d in dsts]
                r = alternate(reps, {"kernel": lambda: lib.amd_test_kv_copy_ms(S, L, C, E, 4, dsts, n_rows, src_rows),
                                     "memcpy2d": lambda: hip.copy2d_ms(pairs, n_rows * E * 2, L)})
                moved = 2 * L * n_rows * E * 2 * (1 + len(dsts))
                km, mm = float(np.median(r["kernel"])), float(np.median(r["memcpy2d"]))
                print(json.dumps({"leg": "d", "config": config, "source": source, "layer_stride_rows": {"src": src_rows or C, "dst": C}, "n_rows": n_rows, "n_dst": len(dsts),
                                  "bytes_read_plus_written": moved, "kernel_ms": round(km, 4), "kernel_GBps": round(moved / km / 1e6, 1),
                                  "kernel_share_of_copy_peak": round(moved / (km * 1e-3) / COPY_PEAK, 3), "memcpy2d_calls": len(pairs), "memcpy2d_ms": round(mm, 4),
                                  "memcpy2d_GBps": round(moved / mm / 1e6, 1), "kernel_runs": [round(x, 4) for x in r["kernel"]],
                                  "memcpy2d_runs": [round(x, 4) for x in r["memcpy2d"]]}), flush=True)
    for p in kv + store:
        hip.h.hipFree(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="13b,7b")
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    _pkg.load_package()
    import bench
    from minigpt4_cpp_amd import minigpt4_library as ML, modelgen as G
    lib = ML.load_library()
    if lib.amd_device_count() <= 0:
        raise SystemExit("prefix_cache_bench.py: no HIP device visible")
    legs = set(args.legs.split(","))
    for config in args.configs.split(","):
        if legs & {"a", "b", "c"}:
            engine_legs(lib, ML, G, bench, config, legs, max(5, args.reps))
        if "d" in legs:
            kernel_leg(lib, config, max(5, args.reps))


if __name__ == "__main__":
    main()
