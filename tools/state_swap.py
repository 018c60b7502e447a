#!/usr/bin/env python3
"""What parking a conversation costs (minigpt4_amd_state_save / _state_load).  Files: bench.py's synthetic 13B Q5_K_M or 7B Q4_0 file, n_ctx 2048, n_batch 512; one
conversation of 64 / 512 / 2040 rows.  Per row count one JSON line; every entry is the median of --reps alternated runs, with max - min behind it:
  save / load   through the library (raw C calls into a preallocated buffer, minigpt4_amd_sync before, wall clock around): milliseconds, GB/s of snapshot bytes
  pack / unpack the kernels alone (minigpt4_amd_test_kv_pack / _unpack on device buffers of the engine's shape, ONE launch over all rows; hipEvent time of the launcher's
                8-byte memset of the checksum word + the kernel): ms and GB/s read + written
  baseline      what a loop of runtime copies would be: 2 * n_layer hipMemcpy2DAsync calls, device cache -> one pinned block (hipEvent time), followed by k_checksum over
                that pinned block (minigpt4_amd_test_checksum, hipEvent time; its value is checked); the two times and their sum
    python tools/state_swap.py --config 13b|7b [--rows 64,512,2040] [--reps 5]        GPU only."""
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


def stat(x):
    return [round(float(np.median(x)), 4), round(float(max(x) - min(x)), 4)]


def alternate(reps, arms):
    for fn in arms.values():
        fn()
    out = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            out[k].append(fn())
    return out


class Hip:
    def __init__(self):
        self.h = ctypes.CDLL("libamdhip64.so")
        self.h.hipMemcpy2DAsync.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        self.h.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.h.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        self.h.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        self.h.hipFree.argtypes = [ctypes.c_void_p]
        self.h.hipHostFree.argtypes = [ctypes.c_void_p]
        self.h.hipHostMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]

    def ok(self, rc):
        if rc:
            raise RuntimeError(f"HIP call failed: {rc}")

    def malloc(self, n):
        p = ctypes.c_void_p()
        self.ok(self.h.hipMalloc(ctypes.byref(p), ctypes.c_size_t(n)))
        self.ok(self.h.hipMemset(p, 1, n))
        return p

    def pinned(self, n):
        p = ctypes.c_void_p()
        self.ok(self.h.hipHostMalloc(ctypes.byref(p), n, 0))
        ctypes.memset(p, 0, n)
        return p

    def copy2d_ms(self, pairs, width, height):
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        self.ok(self.h.hipEventCreate(ctypes.byref(a)))
        self.ok(self.h.hipEventCreate(ctypes.byref(b)))
        self.ok(self.h.hipEventRecord(a, None))
        for dst, dpitch, src, spitch in pairs:
            self.ok(self.h.hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, 2, None))   # 2 = device to host
        self.ok(self.h.hipEventRecord(b, None))
        self.ok(self.h.hipDeviceSynchronize())
        ms = ctypes.c_float()
        self.ok(self.h.hipEventElapsedTime(ctypes.byref(ms), a, b))
        self.h.hipEventDestroy(a)
        self.h.hipEventDestroy(b)
        return float(ms.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="13b", choices=["13b", "7b"])
    ap.add_argument("--rows", default="64,512,2040")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    _pkg.load_package()
    import bench
    from minigpt4_cpp_amd import minigpt4_library as ML
    lib = ML.load_library()
    if lib.amd_device_count() <= 0:
        raise SystemExit("state_swap.py: no HIP device visible")
    L, E = (40, 5120) if args.config == "13b" else (32, 4096)
    C = 2048
    vp, lp, _, _ = bench.make_models(args.config, 0, 1, lambda: None)
    ctx = lib.minigpt4_model_load(vp, lp, verbosity=0, n_ctx=C, n_batch=512)
    raw, sync = lib.library, lambda: lib.library.minigpt4_amd_sync(ctx.ptr)  # noqa: E731
    hip = Hip()
    rng = np.random.default_rng(1)
    for n_rows in [int(r) for r in args.rows.split(",")]:
        lib.minigpt4_reset_chat(ctx)
        lib.amd_eval_tokens(ctx, [1] + rng.integers(3, 30000, n_rows - 1).tolist())
        size = lib.amd_state_size(ctx, 0)
        buf = (ctypes.c_uint8 * size)()
        written = ctypes.c_size_t()

        def save():
            sync()
            t0 = time.perf_counter()
            if raw.minigpt4_amd_state_save(ctx.ptr, 0, buf, size, ctypes.byref(written)):
                raise RuntimeError(lib._err())
            return (time.perf_counter() - t0) * 1e3

        def load():
            sync()
            t0 = time.perf_counter()
            if raw.minigpt4_amd_state_load(ctx.ptr, 0, buf, size):
                raise RuntimeError(lib._err())
            return (time.perf_counter() - t0) * 1e3
        save()
        r = alternate(args.reps, {"save": save, "load": load})
        info = lib.amd_state_info(ctx)
        kv_bytes = 4 * L * E * n_rows
        kv = [hip.malloc(L * C * E * 2), hip.malloc(L * C * E * 2)]
        host = hip.pinned(kv_bytes)
        pairs = [(host.value + (t * L + layer) * n_rows * E * 2, n_rows * E * 2, kv[t].value + layer * C * E * 2, n_rows * E * 2) for t in range(2) for layer in range(L)]
        want_sum = (kv_bytes // 4) * 0x01010101 % (1 << 64)                  # every byte of the caches is 1

        def checksum_ms():
            s_, ms_ = lib.amd_test_checksum(host.value, kv_bytes)
            if s_ != want_sum:
                raise RuntimeError(f"baseline checksum {s_:#x} != {want_sum:#x}")
            return ms_
        k = alternate(args.reps, {"pack": lambda: lib.amd_test_kv_block_ms(L, C, E, 0, n_rows), "unpack": lambda: lib.amd_test_kv_block_ms(L, C, E, 0, n_rows, unpack=True),
                                  "memcpy2d": lambda: hip.copy2d_ms(pairs, n_rows * E * 2, 1), "checksum": checksum_ms})
        for p in kv:
            hip.h.hipFree(p)
        hip.h.hipHostFree(host)
        gbps = lambda nbytes, ms: round(nbytes / ms / 1e6, 1)  # noqa: E731
        print(json.dumps({"config": args.config, "n_rows": n_rows, "snapshot_bytes": size, "kv_bytes": kv_bytes,
                          "save_ms": stat(r["save"]), "load_ms": stat(r["load"]), "save_GBps": gbps(size, np.median(r["save"])), "load_GBps": gbps(size, np.median(r["load"])),
                          "pack_ms": stat(k["pack"]), "unpack_ms": stat(k["unpack"]), "pack_GBps_read_plus_written": gbps(2 * kv_bytes, np.median(k["pack"])),
                          "unpack_GBps_read_plus_written": gbps(2 * kv_bytes, np.median(k["unpack"])), "memcpy2d_calls": len(pairs), "memcpy2d_to_pinned_ms": stat(k["memcpy2d"]),
                          "memcpy2d_GBps": gbps(kv_bytes, np.median(k["memcpy2d"])), "checksum_of_pinned_ms": stat(k["checksum"]),
                          "baseline_ms": round(float(np.median(k["memcpy2d"]) + np.median(k["checksum"])), 4), "staging_bytes": info["staging_bytes"], "pack_launches_total": info["pack_launches"]}), flush=True)
    lib.minigpt4_free(ctx)


if __name__ == "__main__":
    main()
