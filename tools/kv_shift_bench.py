#!/usr/bin/env python3
"""Kernel time of the context shift (launch_kv_shift through minigpt4_amd_test_kv_shift) at the 13B and 7B cache shapes: a full 2048-row context, keep 45, discard 1001.
One JSON line per shape: ms (hipEvent time of the launch, after a warm-up launch), algorithmic bytes (moved K and V rows, read + written), GB/s and the fraction of the
6.29 TB/s device-to-device copy peak.   python tools/kv_shift_bench.py   GPU only."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkg  # noqa: E402

_pkg.load_package()
from minigpt4_cpp_amd import minigpt4_library as ML  # noqa: E402

COPY_PEAK = 6.29e12
lib = ML.load_library()
for name, L, E, H in (("13B", 40, 5120, 40), ("7B", 32, 4096, 32)):
    C, keep, discard = 2048, 45, 1001
    rng = np.random.default_rng(0)
    k = rng.standard_normal((L, C, E), dtype=np.float32).astype(np.float16)
    v = k.copy()
    lib.amd_test_kv_shift(k, v, H, C, keep, discard)                       # warm-up (code object load, first-touch of the device buffers' pages)
    runs = [lib.amd_test_kv_shift(k, v, H, C, keep, discard)[2] for _ in range(3)]
    ms = float(np.median(runs))
    moved = C - keep - discard
    nbytes = L * moved * E * 2 * 2 * 2                                     # fp16, K + V, read + write
    gbs = nbytes / (ms * 1e-3) / 1e9
    print(json.dumps({"shape": name, "n_layer": L, "n_embd": E, "n_head": H, "n_ctx": C, "n_keep": keep, "n_discard": discard, "ms": round(ms, 4),
                      "ms_runs": [round(r, 4) for r in runs], "bytes": nbytes, "GBps": round(gbs, 1), "frac_copy_peak": round(gbs * 1e9 / COPY_PEAK, 3)}), flush=True)
