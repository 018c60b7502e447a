"""Conversation snapshots on the CPU (no GPU): the format of include/minigpt4_amd.h, pinned by a snapshot assembled HERE from the documented layout and read back through
minigpt4_amd_state_peek; the reasons the parser gives for what it refuses; the parser as a stand-alone program under AddressSanitizer + UBSan (tests/c/state_parse_main.c)."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_LAYER, N_EMBD, N_HEAD, N_VOCAB, N_ROWS, BLOCK_ROWS = 2, 64, 4, 41, 5, 2      # three blocks, the last one short; 41 logits: both paddings are not empty
ARENA_HASH = 0xC0FFEE1234567890
HIST = [1, 17, -1, -1, 39]
BIAS = [(3, -1.5), (21, 0.25)]


def build_snapshot(n_rows=N_ROWS, block_rows=BLOCK_ROWS, has_logits=True, parity=True, version=1, magic=b"MG4S", hist=None, bias=BIAS, seed=5):
    """A version-1 snapshot written from the header's description alone (little-endian): header, history, logits, penalties, bias, pad 8, block table, pad 16, KV blocks."""
    rng = np.random.default_rng(seed)
    hist = list(HIST[:n_rows]) if hist is None else list(hist)
    row_bytes = 4 * N_LAYER * N_EMBD
    n_blocks = (n_rows + block_rows - 1) // block_rows
    body = b"".join(struct.pack("<i", t) for t in hist)
    logits = rng.standard_normal(N_VOCAB).astype("<f4")
    if has_logits:
        body += logits.tobytes()
    body += struct.pack("<ifffi", 32, 1.25, 0.5, 0.125, 0)
    body += b"".join(struct.pack("<if", i, b) for i, b in bias)
    body += b"\0" * (-(64 + len(body)) % 8)
    blocks = []
    for c in range(n_blocks):
        rows = min(block_rows, n_rows - c * block_rows)
        blocks.append(rng.integers(0, 1 << 16, size=(2, N_LAYER, rows, N_EMBD), dtype=np.uint16).astype("<u2"))      # [tensor][layer][row][E]
    sums = [int(b.view("<u4").astype(np.uint64).sum(dtype=np.uint64)) for b in blocks]
    body += b"".join(struct.pack("<Q", s) for s in sums)
    body += b"\0" * (-(64 + len(body)) % 16)
    assert sum(b.nbytes for b in blocks) == n_rows * row_bytes
    body += b"".join(b.tobytes() for b in blocks)
    flags = (1 if has_logits else 0) | (2 if parity else 0)
    head = magic + struct.pack("<IQIIIIQIIIiiI", version, 64 + len(body), N_LAYER, N_EMBD, N_HEAD, N_VOCAB, ARENA_HASH, n_rows, block_rows, flags, 7, 9, len(bias))
    assert len(head) == 64
    return head + body


def test_python_built_snapshot_is_accepted_and_every_field_comes_back(lib):
    blob = build_snapshot()
    assert len(blob) == 64 + 20 + 164 + 20 + 16 + 4 + 24 + 8 + N_ROWS * 512      # header, history, logits, penalties, bias, pad, table, pad, 512 bytes per row
    got = lib.amd_state_peek(blob)
    assert got == dict(version=1, total_bytes=len(blob), n_layer=N_LAYER, n_embd=N_EMBD, n_head=N_HEAD, n_vocab=N_VOCAB, arena_hash=ARENA_HASH, n_rows=N_ROWS,
                       block_rows=BLOCK_ROWS, flags=3, greedy=7, feed=9)
    # without a logits row the section is absent, not zero-filled
    short = build_snapshot(has_logits=False, parity=False)
    assert len(short) == 64 + 20 + 20 + 16 + 24 + N_ROWS * 512 and lib.amd_state_peek(short)["flags"] == 0      # (both paddings empty here)
    # one block when block_rows covers every row; an empty conversation has no block at all
    assert lib.amd_state_peek(build_snapshot(block_rows=1000))["block_rows"] == 1000
    empty = build_snapshot(n_rows=0, has_logits=False)
    assert lib.amd_state_peek(empty)["n_rows"] == 0 and len(empty) == 64 + 20 + 16 + 4 + 8


def _patched_total(blob, n):
    return blob[:8] + struct.pack("<Q", n) + blob[16:n]


@pytest.mark.parametrize("name,make,reason", [
    ("magic", lambda b: b"MG4T" + b[4:], "magic"),
    ("version", lambda b: b[:4] + struct.pack("<I", 2) + b[8:], "version 2"),
    ("total", lambda b: b + b"\0" * 16, "total size"),
    ("total_short", lambda b: b[:-1], "total size"),
    ("history", lambda b: _patched_total(b, 64 + 4 * N_ROWS - 4), "token history truncated"),
    ("table", lambda b: _patched_total(b, 64 + 20 + 164 + 20 + 16 + 4 + 16), "block table truncated"),
    ("empty", lambda b: b"", "empty buffer"),
    ("history_id", lambda b: b[:64] + struct.pack("<i", N_VOCAB) + b[68:], "token history id out of range at row 0"),
    ("history_id_low", lambda b: b[:68] + struct.pack("<i", -2) + b[72:], "token history id out of range at row 1"),
    ("embd", lambda b: b[:20] + struct.pack("<I", 60) + b[24:], "model shape"),
    ("block_rows_0", lambda b: b[:44] + struct.pack("<I", 0) + b[48:], "block_rows"),
    ("kv_size", lambda b: b[:40] + struct.pack("<I", N_ROWS - 1) + b[44:], "KV blocks"),
])
def test_peek_refuses_with_its_reason(lib, name, make, reason):
    bad = make(build_snapshot())
    with pytest.raises(RuntimeError, match="state_peek: .*" + re.escape(reason)):
        lib.amd_state_peek(bad)


def test_new_symbols_are_declared_and_exported(lib):
    txt = open(os.path.join(ROOT, "include", "minigpt4_amd.h")).read()
    declared = set(re.findall(r"MINIGPT4_API[^;]*?\b(minigpt4_\w+)\s*\(", txt))
    want = {"minigpt4_amd_state_" + s for s in ("size", "save", "load", "save_file", "load_file", "peek", "info")}
    assert want <= declared
    for s in want:
        assert hasattr(lib.library, s)
    for text in ("MG4S", "MINIGPT4_STATE_BLOCK_BYTES", "mirostat", "constraint handle", "prefix store", "queued rows", "block c checksum"):      # the format, the omissions, the one failure
        assert text in txt, text


def _sanitizer_toolchains():
    """(C compiler, C++ compiler, extra link flags) to try: the ROCm installation's clang (the compiler the library is built with), then the system's gcc.  Either way the
    sanitizer runtime is linked INTO the program (clang's default; gcc: -static-libasan), so nothing has to be preloaded or come first among the shared objects."""
    out = []
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
    if os.path.exists(os.path.join(llvm, "clang++")):
        out.append((os.path.join(llvm, "clang"), os.path.join(llvm, "clang++"), []))
    if shutil.which("gcc") and shutil.which("g++"):
        out.append(("gcc", "g++", ["-static-libasan", "-static-libubsan"]))
    return out


def test_parser_program_under_sanitizers_exits_0(tmp_path):
    """tests/c/state_parse_main.c + csrc/state.cpp, both compiled with -fsanitize=address,undefined for the host and linked into one program with its own main: a valid
    snapshot, every truncation, single-byte corruptions.  Nothing is preloaded; a sanitizer report ends the program with a non-zero status (-fno-sanitize-recover)."""
    src_c = os.path.join(ROOT, "tests", "c", "state_parse_main.c")
    src_cpp = os.path.join(ROOT, "minigpt4.cpp_amd", "csrc", "state.cpp")
    san = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    exe, log = str(tmp_path / "state_parse"), []
    for cc, cxx, link in _sanitizer_toolchains():
        steps = [[cc, "-std=c99", "-Wall", "-Werror", *san, "-c", src_c, "-o", str(tmp_path / "main.o")],
                 [cxx, "-std=c++17", "-Wall", *san, "-I", os.path.dirname(src_cpp), "-c", src_cpp, "-o", str(tmp_path / "state.o")],
                 [cxx, *san, *link, str(tmp_path / "main.o"), str(tmp_path / "state.o"), "-o", exe]]
        runs = [subprocess.run(s, capture_output=True, text=True) for s in steps]
        if all(r.returncode == 0 for r in runs):
            break
        log.append((cc, [r.stderr[-2000:] for r in runs if r.returncode]))
    else:
        pytest.fail(f"no toolchain built the sanitizer program: {log}")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "state_parse ok" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stdout + run.stderr
