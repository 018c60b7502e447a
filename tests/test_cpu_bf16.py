"""BF16 (GGUF tensor type 30) on the host: quants.quantize rounds to nearest even exactly as torch's bfloat16 does, dequantize is the exact widening, and a tiny
all-BF16 GGUF file is read with its types, shapes and bytes (a GGJT file that claims the type is refused)."""
import ctypes

import numpy as np
import torch

BF16 = 30


def test_quantize_is_rne_and_dequantize_the_exact_widening():
    from minigpt4_cpp_amd import quants as Q
    assert Q.GGML_BF16 == BF16 and Q.TYPE_NAMES[BF16] == "bf16" and Q.BLOCK[BF16] == (1, 2)
    bits = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,       # exact ties: down to even, up to even, both signs
                     0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0xFF7FFFFF,       # just above / below a tie; the largest finite float (rounds to inf)
                     0x00000001, 0x00008000, 0x00018000, 0x807FFFFF,       # subnormals, two of them ties
                     0x00000000, 0x80000000, 0x7F800000, 0xFF800000], np.uint32)
    x = np.concatenate([bits.view(np.float32), np.random.default_rng(3).standard_normal(4096).astype(np.float32)])
    got = Q.quantize(BF16, x).view(np.uint16)
    want = torch.tensor(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    wide = Q.dequantize(BF16, got.view(np.uint8), got.size)
    assert wide.dtype == np.float64 and np.array_equal(wide.astype(np.float32).view(np.uint32), got.astype(np.uint32) << 16)


def test_tiny_bf16_gguf_is_read_and_a_ggjt_file_with_the_type_is_refused(lib, tiny_files, tmp_path):
    from minigpt4_cpp_amd import modelgen as G
    _, llm = tiny_files
    src, dst = llm("bf16"), str(tmp_path / "bf16.gguf")
    G.ggjt_to_gguf(src, dst)
    f = G.read_llm_file(src)
    assert all(t.gtype == (0 if len(t.ne) == 1 else BF16) for t in f.tensors.values())
    L = lib.library
    L.minigpt4_amd_llm_file_digest.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    digest = ctypes.c_uint64()
    assert L.minigpt4_amd_llm_file_digest(src.encode(), ctypes.byref(digest), 1) != 0            # GGJT v3 cannot carry the type
    assert L.minigpt4_amd_llm_file_digest(dst.encode(), ctypes.byref(digest), 1) == 0, L.minigpt4_amd_last_error()
    raw = bytearray(open(dst, "rb").read())                                                     # one byte of one BF16 tensor changes the loader's view of the file
    at = bytes(raw).find(bytes(f.raw("layers.0.attention.wq.weight")[:64]))
    raw[at + 1] ^= 0x01
    open(str(tmp_path / "twin.gguf"), "wb").write(bytes(raw))
    twin = ctypes.c_uint64()
    assert at > 0 and L.minigpt4_amd_llm_file_digest(str(tmp_path / "twin.gguf").encode(), ctypes.byref(twin), 1) == 0 and twin.value != digest.value
    n_tensors, wb = ctypes.c_int(), ctypes.c_int64()
    assert L.minigpt4_amd_inspect_files(None, dst.encode(), None, ctypes.byref(n_tensors), ctypes.byref(wb)) == 0 and n_tensors.value == len(f.tensors)
    # every matrix at 2 bytes per weight, the norm vectors as F32, one row of the embedding table
    assert wb.value == sum(2 * 256 if n == "tok_embeddings.weight" else int(np.prod(t.ne)) * (4 if len(t.ne) == 1 else 2) for n, t in f.tensors.items())
