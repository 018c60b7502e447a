"""Host-side mirror of the reference's Python binding for the MI355X build of libminigpt4.so.

Same class and method names, argument meaning and error behaviour as the reference's
`minigpt4/minigpt4_library.py` (MiniGPT4SharedLibrary :74-523, load_library :525-566, MiniGPT4ChatBot :568-689),
so code and tests written against the reference binding read the same here.  The reference's *unmodified* binding
also works against this library; this mirror exists so the repo is self-contained, adds correct
ctypes prototypes (`size_t` / `bool` instead of int32) and exposes the additive `minigpt4_amd_*` entry points.

There is no CPU fallback: loading a model without a usable gfx950 device raises.
"""
from __future__ import annotations

import ctypes
import enum
import os
from typing import Iterator, List, Optional, Sequence

import numpy as np


class DataType(enum.IntEnum):
    F16 = 0; F32 = 1; I32 = 2; L64 = 3; Q4_0 = 4; Q4_1 = 5; Q5_0 = 6; Q5_1 = 7; Q8_0 = 8; Q8_1 = 9   # noqa: E702
    Q2_K = 10; Q3_K = 11; Q4_K = 12; Q5_K = 13; Q6_K = 14; Q8_K = 15                                   # noqa: E702

    def __str__(self):
        return str(self.name)


class Verbosity(enum.IntEnum):
    SILENT = 0; ERR = 1; INFO = 2; DEBUG = 3   # noqa: E702


class ImageFormat(enum.IntEnum):
    UNKNOWN = 0; F32 = 1; U8 = 2   # noqa: E702


I32, F32, SIZE_T, VOID_PTR = ctypes.c_int32, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
CHAR_PTR = ctypes.c_char_p
FLOAT_PTR = ctypes.POINTER(ctypes.c_float)
INT_PTR = ctypes.POINTER(ctypes.c_int32)


class MiniGPT4Context:
    def __init__(self, ptr):
        self.ptr = ptr


class MiniGPT4Image(ctypes.Structure):
    _fields_ = [("data", VOID_PTR), ("width", I32), ("height", I32), ("channels", I32), ("format", I32)]


class MiniGPT4Embedding(ctypes.Structure):
    _fields_ = [("data", FLOAT_PTR), ("n_embeddings", SIZE_T)]   # 2nd field is `elements` in the C header


class MiniGPT4Images(ctypes.Structure):
    _fields_ = [("images", ctypes.POINTER(MiniGPT4Image)), ("n_images", SIZE_T)]


class MiniGPT4Embeddings(ctypes.Structure):
    _fields_ = [("embeddings", ctypes.POINTER(MiniGPT4Embedding)), ("n_embeddings", SIZE_T)]


_CHAT_ARGS = [SIZE_T, F32, I32, F32, F32, F32, I32, F32, F32, F32, I32, F32, F32, I32]

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


_REGEX_SPECIAL = frozenset(b"\\.[](){}|*+?^$-")


def regex_escape(text) -> str:
    """`text` (str, or bytes of UTF-8) as a pattern of the constraint language that matches exactly it: the characters with a meaning there get a backslash, a control byte
    becomes \\xHH; everything else, UTF-8 included, stands for itself.  Python's `re` reads the result the same way."""
    data = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    out = bytearray()
    for b in data:
        if b in _REGEX_SPECIAL:
            out += b"\\" + bytes([b])
        elif b < 0x20 or b == 0x7F:
            out += b"\\x%02X" % b
        else:
            out.append(b)
    return out.decode("utf-8")


def choice_pattern(options) -> str:
    """The pattern that matches exactly one of `options` (str each): (?:a|b|c) with every option escaped."""
    options = list(options)
    if not options:
        raise ValueError("choice_pattern: at least one option is required")
    return "(?:" + "|".join(regex_escape(o) for o in options) + ")"


def _test_hook_names() -> frozenset:
    """The names include/minigpt4_amd_test.h declares: the ONLY symbols that may be served by libminigpt4_test.so."""
    import re
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "minigpt4_amd_test.h")
    try:
        with open(hdr) as f:
            return frozenset(re.findall(r"\b(minigpt4_amd_[a-z0-9_]+)\s*\(", f.read()))
    except OSError:
        return frozenset()


class _Symbols:
    """Attribute access to the product library's symbols.  A name that include/minigpt4_amd_test.h declares (kernel-level test hooks, micro-benchmarks, probes, host-only test
    helpers) is served by libminigpt4_test.so, which is loaded -- and has its prototypes declared -- on first use; only tests/ and tools/ ever get there.  Any other
    name the product does not export is an AttributeError (a typo must not load a second copy of the engine).  The two libraries are separate copies of the engine's
    state (tuning knobs, last error): contexts are never passed from one to the other except by `minigpt4_amd_copy_arenas`, and both must report the same build."""

    def __init__(self, product, test_path: str, declare_test):
        self.__dict__.update(_product=product, _test_path=test_path, _declare_test=declare_test, _test=None, _hook_names=_test_hook_names())

    def _hooks(self):
        if self._test is None:
            if hasattr(self._product, "minigpt4_amd_test_mul_mat"):      # MINIGPT4_LIBRARY names a test-hook build itself: ONE copy of the engine serves everything
                self.__dict__["_test"] = self._product                     # (what the in-kernel timeline tools need: the stamps live in the library that ran the kernel)
                self._declare_test(self._product)
                return self._test
            if not os.path.exists(self._test_path):
                raise AttributeError(f"{self._test_path} not found (the test-hook build of the library: `make -C minigpt4.cpp_amd/csrc`)")
            test = ctypes.cdll.LoadLibrary(self._test_path)
            for lib_ in (test, self._product):
                lib_.minigpt4_amd_build_info.restype = CHAR_PTR
            a, b = self._product.minigpt4_amd_build_info(), test.minigpt4_amd_build_info()
            if a != b:
                raise RuntimeError(f"libminigpt4.so and {os.path.basename(self._test_path)} come from different builds ({a!r} vs {b!r}): rebuild both (`make -C minigpt4.cpp_amd/csrc`)")
            self.__dict__["_test"] = test
            self._declare_test(test)
        return self._test

    @property
    def test_hooks(self):
        """libminigpt4_test.so itself (explicit handle)."""
        return self._hooks()

    def _last_error(self):
        """thread-local error text of the product library and, once it is loaded, of the test-hook library (each has its own copy of the engine's state)."""
        a = self._product.minigpt4_amd_last_error() or b""
        b = (self._test.minigpt4_amd_last_error() or b"") if self._test is not None else b""
        return a + (b" | " if a and b else b"") + b

    def __getattr__(self, name):
        if name == "minigpt4_amd_last_error":
            return self._last_error
        if name in self._hook_names:
            return getattr(self._hooks(), name)
        return getattr(self._product, name)


class MiniGPT4SharedLibrary:
    """ctypes wrapper around libminigpt4.so (reference class of the same name)."""

    def __init__(self, shared_library_path: str, test_library_path: Optional[str] = None):
        product = ctypes.cdll.LoadLibrary(shared_library_path)
        if test_library_path is None:
            test_library_path = os.environ.get("MINIGPT4_TEST_LIBRARY", shared_library_path[:-3] + "_test.so" if shared_library_path.endswith(".so") else shared_library_path + "_test")
        self.library = _Symbols(product, test_library_path, self._declare_test_hooks)
        L = product
        P = ctypes.POINTER
        L.minigpt4_model_load.argtypes = [CHAR_PTR, CHAR_PTR, I32, I32, I32, I32, ctypes.c_bool]
        L.minigpt4_model_load.restype = VOID_PTR
        L.minigpt4_image_load_from_file.argtypes = [VOID_PTR, CHAR_PTR, P(MiniGPT4Image), I32]
        L.minigpt4_preprocess_image.argtypes = [VOID_PTR, P(MiniGPT4Image), P(MiniGPT4Image), I32]
        L.minigpt4_encode_image.argtypes = [VOID_PTR, P(MiniGPT4Image), P(MiniGPT4Embedding), SIZE_T]
        L.minigpt4_begin_chat_image.argtypes = [VOID_PTR, P(MiniGPT4Embedding), CHAR_PTR, SIZE_T]
        L.minigpt4_end_chat_image.argtypes = [VOID_PTR, P(ctypes.c_char_p)] + _CHAT_ARGS
        L.minigpt4_system_prompt.argtypes = [VOID_PTR, SIZE_T]
        L.minigpt4_begin_chat.argtypes = [VOID_PTR, CHAR_PTR, SIZE_T]
        L.minigpt4_end_chat.argtypes = [VOID_PTR, P(ctypes.c_char_p)] + _CHAT_ARGS
        L.minigpt4_reset_chat.argtypes = [VOID_PTR]
        L.minigpt4_contains_eos_token.argtypes = [CHAR_PTR]
        L.minigpt4_is_eos.argtypes = [CHAR_PTR]
        L.minigpt4_free.argtypes = [VOID_PTR]
        L.minigpt4_free_image.argtypes = [P(MiniGPT4Image)]
        L.minigpt4_free_embedding.argtypes = [P(MiniGPT4Embedding)]
        L.minigpt4_error_code_to_string.argtypes = [I32]
        L.minigpt4_error_code_to_string.restype = CHAR_PTR
        L.minigpt4_quantize_model.argtypes = [CHAR_PTR, CHAR_PTR, I32]
        L.minigpt4_set_verbosity.argtypes = [I32]
        L.minigpt4_set_verbosity.restype = None
        for name in ("image_load_from_file", "preprocess_image", "encode_image", "begin_chat_image", "end_chat_image", "system_prompt",
                     "begin_chat", "end_chat", "reset_chat", "contains_eos_token", "is_eos", "free", "free_image", "free_embedding", "quantize_model"):
            getattr(L, "minigpt4_" + name).restype = I32
        # additive API (include/minigpt4_amd.h)
        L.minigpt4_amd_device_count.restype = I32
        L.minigpt4_amd_last_error.restype = CHAR_PTR
        L.minigpt4_amd_build_info.restype = CHAR_PTR
        L.minigpt4_amd_decode_image.argtypes = [CHAR_PTR, SIZE_T, P(MiniGPT4Image)]
        L.minigpt4_amd_decode_image.restype = I32
        for name in ("n_vocab", "n_embd", "n_past", "sync"):
            getattr(L, "minigpt4_amd_" + name).argtypes = [VOID_PTR]
            getattr(L, "minigpt4_amd_" + name).restype = I32
        L.minigpt4_amd_eval_tokens.argtypes = [VOID_PTR, INT_PTR, I32]
        L.minigpt4_amd_eval_embd.argtypes = [VOID_PTR, FLOAT_PTR, I32]
        L.minigpt4_amd_get_logits.argtypes = [VOID_PTR, FLOAT_PTR, SIZE_T]
        L.minigpt4_amd_tokenize.argtypes = [VOID_PTR, CHAR_PTR, I32, INT_PTR, I32]
        L.minigpt4_amd_sample.argtypes = [VOID_PTR, INT_PTR, F32, I32, F32, F32, F32, I32, F32, F32]
        L.minigpt4_amd_decode_loop.argtypes = [VOID_PTR, I32, INT_PTR, FLOAT_PTR]
        L.minigpt4_amd_profile_sites.argtypes = [VOID_PTR, I32, ctypes.c_char_p, SIZE_T]
        L.minigpt4_amd_weight_bytes_per_token.argtypes = [VOID_PTR]
        L.minigpt4_amd_weight_bytes_per_token.restype = ctypes.c_double
        L.minigpt4_amd_last_encode_ms.argtypes = [VOID_PTR]
        L.minigpt4_amd_last_encode_ms.restype = F32
        for name in ("minigpt4_amd_encode_images", "minigpt4_encode_images"):        # the second = deprecated alias (include/minigpt4_amd.h)
            getattr(L, name).argtypes = [VOID_PTR, P(MiniGPT4Images), P(MiniGPT4Embeddings), SIZE_T]
        for name in ("minigpt4_amd_free_embeddings", "minigpt4_free_embeddings"):
            getattr(L, name).argtypes = [P(MiniGPT4Embeddings)]
        L.minigpt4_amd_weight_arena.argtypes = [VOID_PTR, I32, P(VOID_PTR), P(SIZE_T)]
        U64P, SZP = P(ctypes.c_uint64), P(ctypes.c_size_t)
        L.minigpt4_amd_plan_arenas.argtypes = [CHAR_PTR, CHAR_PTR, SZP, SZP, U64P, U64P]
        L.minigpt4_amd_arena_plan.argtypes = [VOID_PTR, SZP, SZP, U64P, U64P]
        L.minigpt4_amd_load_mode.argtypes = [VOID_PTR]
        L.minigpt4_amd_weights_received.argtypes = [VOID_PTR]
        L.minigpt4_amd_arena_checksum.argtypes = [VOID_PTR, I32, U64P]
        L.minigpt4_amd_set_parity.argtypes = [VOID_PTR, I32]
        L.minigpt4_amd_dist_info.argtypes = [VOID_PTR, P(I32), P(I32), P(F32)]
        L.minigpt4_amd_dist_info.restype = I32
        L.minigpt4_amd_parity.argtypes = [VOID_PTR]
        L.minigpt4_amd_set_conversations.argtypes = [VOID_PTR, I32]
        L.minigpt4_amd_select_conversation.argtypes = [VOID_PTR, I32]
        L.minigpt4_amd_n_conversations.argtypes = [VOID_PTR]
        L.minigpt4_amd_end_chat_batch.argtypes = [VOID_PTR, INT_PTR, I32, P(ctypes.c_char_p), F32, I32, F32, F32, F32, I32, F32, F32]
        L.minigpt4_amd_eval_batch.argtypes = [VOID_PTR, INT_PTR, I32, INT_PTR, INT_PTR]
        L.minigpt4_amd_prefill_batch.argtypes = [VOID_PTR, INT_PTR, I32]
        L.minigpt4_amd_batch_path.argtypes = [VOID_PTR, INT_PTR]
        L.minigpt4_amd_shift_context.argtypes = [VOID_PTR, I32, I32]
        L.minigpt4_amd_set_context_shift.argtypes = [VOID_PTR, I32]
        L.minigpt4_amd_fork_conversation.argtypes = [VOID_PTR, I32, INT_PTR, I32, I32]
        L.minigpt4_amd_set_prefix_cache.argtypes = [VOID_PTR, I32]
        L.minigpt4_amd_prefix_cache_info.argtypes = [VOID_PTR, INT_PTR]
        L.minigpt4_amd_score_tokens.argtypes = [VOID_PTR, INT_PTR, I32, FLOAT_PTR, INT_PTR, FLOAT_PTR, FLOAT_PTR]
        L.minigpt4_amd_score_batch.argtypes = [VOID_PTR, INT_PTR, I32, INT_PTR, INT_PTR, FLOAT_PTR, INT_PTR, FLOAT_PTR]
        L.minigpt4_amd_token_piece.argtypes = [VOID_PTR, I32]
        L.minigpt4_amd_token_piece.restype = ctypes.c_char_p
        L.minigpt4_amd_top_logprobs.argtypes = [VOID_PTR, INT_PTR, I32, I32, INT_PTR, INT_PTR, FLOAT_PTR, FLOAT_PTR, INT_PTR]
        L.minigpt4_amd_end_chat_batch_top.argtypes = [VOID_PTR, INT_PTR, I32, P(ctypes.c_char_p), F32, I32, F32, F32, F32, I32, F32, F32, I32, INT_PTR, FLOAT_PTR, INT_PTR, INT_PTR,
                                                      FLOAT_PTR]
        L.minigpt4_amd_score_tokens_top.argtypes = [VOID_PTR, INT_PTR, I32, I32, FLOAT_PTR, INT_PTR, INT_PTR, FLOAT_PTR]
        L.minigpt4_amd_set_speculation.argtypes = [VOID_PTR, I32]
        L.minigpt4_amd_verify_draft.argtypes = [VOID_PTR, INT_PTR, I32, INT_PTR, INT_PTR, INT_PTR]
        L.minigpt4_amd_decode_lookup.argtypes = [VOID_PTR, INT_PTR, I32, I32, I32, I32, I32, INT_PTR, INT_PTR, INT_PTR]
        L.minigpt4_amd_set_penalties.argtypes = [VOID_PTR, I32]
        L.minigpt4_amd_conversation_penalties.argtypes = [VOID_PTR, I32, I32, F32, F32, F32, I32]
        L.minigpt4_amd_set_logit_bias.argtypes = [VOID_PTR, INT_PTR, FLOAT_PTR, I32]
        L.minigpt4_amd_token_history.argtypes = [VOID_PTR, INT_PTR, I32]
        L.minigpt4_amd_penalty_info.argtypes = [VOID_PTR, INT_PTR]
        L.minigpt4_amd_beam_search.argtypes = [VOID_PTR, INT_PTR, I32, I32, F32, I32, INT_PTR, INT_PTR, FLOAT_PTR, INT_PTR, INT_PTR]
        L.minigpt4_amd_end_chat_guided.argtypes = [VOID_PTR, INT_PTR, INT_PTR, I32, F32, ctypes.POINTER(ctypes.c_char_p), F32, I32, F32, F32, F32, I32, F32, F32, INT_PTR]
        L.minigpt4_amd_guided_logits.argtypes = [VOID_PTR, INT_PTR, INT_PTR, I32, F32, FLOAT_PTR, INT_PTR]
        L.minigpt4_amd_guidance_info.argtypes = [VOID_PTR, INT_PTR]
        L.minigpt4_amd_constraint_compile.argtypes = [VOID_PTR, CHAR_PTR, I32, INT_PTR]
        L.minigpt4_amd_constraint_free.argtypes = [VOID_PTR, I32]
        L.minigpt4_amd_set_constraint.argtypes = [VOID_PTR, I32, I32]
        L.minigpt4_amd_constraint_advance.argtypes = [VOID_PTR, I32, INT_PTR, I32]
        L.minigpt4_amd_constraint_info.argtypes = [VOID_PTR, I32, INT_PTR]
        L.minigpt4_amd_constraint_mask.argtypes = [VOID_PTR, I32, I32, P(ctypes.c_uint32), I32]
        L.minigpt4_amd_end_chat_batch_sampled.argtypes = [VOID_PTR, INT_PTR, I32, P(ctypes.c_char_p), F32, I32, F32, INT_PTR]
        L.minigpt4_amd_sampled_candidates.argtypes = [VOID_PTR, INT_PTR, I32, F32, I32, F32, INT_PTR, FLOAT_PTR, INT_PTR, INT_PTR]
        L.minigpt4_amd_conversation_seed.argtypes = [VOID_PTR, I32, ctypes.c_uint64, ctypes.c_uint64]
        L.minigpt4_amd_sampling_info.argtypes = [VOID_PTR, I32, U64P]
        L.minigpt4_amd_end_chat_batch_sampled_ex.argtypes = [VOID_PTR, INT_PTR, I32, P(ctypes.c_char_p), F32, I32, F32, F32, F32, F32, I32, F32, F32, INT_PTR]
        L.minigpt4_amd_sampled_candidates_ex.argtypes = [VOID_PTR, INT_PTR, I32, F32, I32, F32, F32, F32, F32, I32, F32, F32, INT_PTR, FLOAT_PTR, INT_PTR, U64P]
        L.minigpt4_amd_conversation_mirostat.argtypes = [VOID_PTR, I32, F32]
        L.minigpt4_amd_mirostat_info.argtypes = [VOID_PTR, I32, FLOAT_PTR]
        I64P = P(ctypes.c_int64)
        L.minigpt4_amd_state_size.argtypes = [VOID_PTR, I32]
        L.minigpt4_amd_state_size.restype = SIZE_T
        L.minigpt4_amd_state_save.argtypes = [VOID_PTR, I32, VOID_PTR, SIZE_T, P(ctypes.c_size_t)]
        L.minigpt4_amd_state_load.argtypes = [VOID_PTR, I32, VOID_PTR, SIZE_T]
        L.minigpt4_amd_state_save_file.argtypes = [VOID_PTR, I32, CHAR_PTR]
        L.minigpt4_amd_state_load_file.argtypes = [VOID_PTR, I32, CHAR_PTR]
        L.minigpt4_amd_state_peek.argtypes = [VOID_PTR, SIZE_T, I64P]
        L.minigpt4_amd_state_info.argtypes = [VOID_PTR, I64P]
        L.minigpt4_amd_verify_draft_sampled.argtypes = [VOID_PTR, INT_PTR, I32, F32, I32, F32, INT_PTR, INT_PTR, INT_PTR, INT_PTR, FLOAT_PTR]
        L.minigpt4_amd_decode_lookup_sampled.argtypes = [VOID_PTR, INT_PTR, I32, I32, I32, I32, I32, F32, I32, F32, INT_PTR, INT_PTR, INT_PTR]
        L.minigpt4_amd_speculation_info.argtypes = [VOID_PTR, I64P]
        L.minigpt4_amd_verify_draft_batch.argtypes = [VOID_PTR, INT_PTR, I32, INT_PTR, INT_PTR, INT_PTR, INT_PTR, INT_PTR]
        L.minigpt4_amd_decode_lookup_batch.argtypes = [VOID_PTR, INT_PTR, I32, INT_PTR, INT_PTR, I32, I32, I32, I32, INT_PTR, INT_PTR, INT_PTR]
        L.minigpt4_amd_speculation_batch_info.argtypes = [VOID_PTR, I64P]
        L.minigpt4_amd_verify_draft_sampled_ex.argtypes = [VOID_PTR, INT_PTR, I32, F32, I32, F32, F32, F32, F32, INT_PTR, INT_PTR, INT_PTR, INT_PTR, FLOAT_PTR]
        L.minigpt4_amd_decode_lookup_sampled_ex.argtypes = [VOID_PTR, INT_PTR, I32, I32, I32, I32, I32, F32, I32, F32, F32, F32, F32, INT_PTR, INT_PTR, INT_PTR]

    @staticmethod
    def _declare_test_hooks(L):
        """Prototypes of libminigpt4_test.so's extra symbols (include/minigpt4_amd_test.h)."""
        P = ctypes.POINTER
        U64P = P(ctypes.c_uint64)
        L.minigpt4_amd_convert_q3k_q6k.argtypes = [VOID_PTR, VOID_PTR, ctypes.c_int64]
        L.minigpt4_amd_test_mul_mat.argtypes = [I32, VOID_PTR, ctypes.c_int64, ctypes.c_int64, FLOAT_PTR, ctypes.c_int64, FLOAT_PTR]
        L.minigpt4_amd_test_mul_mat_ref.argtypes = L.minigpt4_amd_test_mul_mat.argtypes
        L.minigpt4_amd_test_mmq2.argtypes = [I32, VOID_PTR, I32, ctypes.c_int64, ctypes.c_int64, FLOAT_PTR, ctypes.c_int64, FLOAT_PTR, I32, I32, FLOAT_PTR]
        L.minigpt4_amd_test_matvec.argtypes = [I32, VOID_PTR, I32, I32, VOID_PTR, I32, ctypes.c_int64, ctypes.c_int64, FLOAT_PTR, FLOAT_PTR, I32, I32, I32, FLOAT_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_matvec_rows.argtypes = [I32, VOID_PTR, I32, ctypes.c_int64, ctypes.c_int64, FLOAT_PTR, I32, FLOAT_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_matvec_issue.argtypes = L.minigpt4_amd_test_matvec.argtypes[:11] + [I32, FLOAT_PTR, I32, I32, FLOAT_PTR]
        L.minigpt4_amd_test_matvec_waves.argtypes = []
        L.minigpt4_amd_test_quantize.argtypes = [FLOAT_PTR, FLOAT_PTR, ctypes.c_int64, ctypes.c_int64, VOID_PTR, VOID_PTR, VOID_PTR, VOID_PTR, VOID_PTR]
        planes13 = [VOID_PTR] * 13
        L.minigpt4_amd_test_prepare.argtypes = [I32, FLOAT_PTR, FLOAT_PTR, ctypes.c_int64, ctypes.c_int64, I32, I32, I32, VOID_PTR] + planes13
        L.minigpt4_amd_test_prepare_slabs.argtypes = [I32, FLOAT_PTR, I32, ctypes.c_int64, FLOAT_PTR, I32, FLOAT_PTR, ctypes.c_int64, ctypes.c_int64, I32, I32, VOID_PTR, FLOAT_PTR] + planes13
        L.minigpt4_amd_test_slab_flush.argtypes = [I32, I32, INT_PTR, FLOAT_PTR, ctypes.c_int64, FLOAT_PTR, I32, FLOAT_PTR]
        L.minigpt4_amd_test_rope_kv_slabs.argtypes = [I32, I32, I32, I32, I32, INT_PTR, FLOAT_PTR, ctypes.c_int64, FLOAT_PTR, FLOAT_PTR, VOID_PTR, VOID_PTR]
        L.minigpt4_amd_test_gemm_f16.argtypes = [FLOAT_PTR, FLOAT_PTR, FLOAT_PTR, I32, I32, I32, I32, FLOAT_PTR]
        L.minigpt4_amd_test_gemm_f16_skinny.argtypes = L.minigpt4_amd_test_gemm_f16.argtypes
        L.minigpt4_amd_test_gemm_f16_ex.argtypes = [FLOAT_PTR, FLOAT_PTR, FLOAT_PTR, I32, I32, I32, I32, I32, VOID_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_matvec_ex.argtypes = L.minigpt4_amd_test_matvec.argtypes[:-1] + [VOID_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_f16_silu_pair.argtypes = [FLOAT_PTR, VOID_PTR, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, VOID_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_f16_silu_pair_ex.argtypes = [FLOAT_PTR, VOID_PTR, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, VOID_PTR, VOID_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_layernorm.argtypes = [FLOAT_PTR, FLOAT_PTR, FLOAT_PTR, I32, I32, I32, FLOAT_PTR, VOID_PTR]
        L.minigpt4_amd_test_splitk_reduce_ln.argtypes = [FLOAT_PTR, I32, ctypes.c_int64, FLOAT_PTR, FLOAT_PTR, I32, I32, I32, FLOAT_PTR, FLOAT_PTR, FLOAT_PTR, FLOAT_PTR, VOID_PTR]
        L.minigpt4_amd_test_gemm_f16_splitk.argtypes = [FLOAT_PTR, FLOAT_PTR, I32, I32, I32, I32, I32, FLOAT_PTR, INT_PTR]
        L.minigpt4_amd_test_gemm_f16_head_major.argtypes = [FLOAT_PTR, FLOAT_PTR, FLOAT_PTR, I32, I32, I32, I32, FLOAT_PTR]
        L.minigpt4_amd_test_im2col.argtypes = [FLOAT_PTR, I32, I32, VOID_PTR]
        L.minigpt4_amd_test_assemble.argtypes = [FLOAT_PTR, FLOAT_PTR, FLOAT_PTR, I32, I32, FLOAT_PTR]
        L.minigpt4_amd_test_lin_epilogue.argtypes = [FLOAT_PTR, FLOAT_PTR, FLOAT_PTR, VOID_PTR, I32, I32, FLOAT_PTR, VOID_PTR]
        L.minigpt4_amd_test_set_gemm_arm.argtypes = [I32, I32]
        L.minigpt4_amd_test_set_gemm_arm.restype = None
        L.minigpt4_amd_test_set_splitk_xcd.argtypes = [I32]
        L.minigpt4_amd_test_set_splitk_xcd.restype = None
        L.minigpt4_amd_test_activation.argtypes = [I32, VOID_PTR, VOID_PTR]
        L.minigpt4_amd_test_attn_f32.argtypes = [FLOAT_PTR, FLOAT_PTR, FLOAT_PTR, I32, I32, I32, I32, I32, F32, F32, I32, I32, VOID_PTR, FLOAT_PTR, VOID_PTR]
        L.minigpt4_amd_test_kv_shift.argtypes = [I32, I32, I32, I32, I32, I32, I32, VOID_PTR, VOID_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_kv_copy.argtypes = [I32, I32, I32, I32, I32, INT_PTR, I32, I32, I32, VOID_PTR, VOID_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_checksum.argtypes = [VOID_PTR, SIZE_T, U64P, FLOAT_PTR]
        L.minigpt4_amd_test_kv_pack.argtypes = [I32, I32, I32, I32, I32, VOID_PTR, VOID_PTR, VOID_PTR, U64P, FLOAT_PTR]
        L.minigpt4_amd_test_kv_unpack.argtypes = [I32, I32, I32, I32, I32, VOID_PTR, VOID_PTR, VOID_PTR, U64P, FLOAT_PTR]
        L.minigpt4_amd_test_logprob_rows.argtypes = [FLOAT_PTR, I32, I32, I32, INT_PTR, FLOAT_PTR, INT_PTR, FLOAT_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_topn_rows.argtypes = [FLOAT_PTR, I32, I32, I32, INT_PTR, I32, I32, INT_PTR, INT_PTR, FLOAT_PTR, INT_PTR, FLOAT_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_penalise_host.argtypes = [FLOAT_PTR, I32, INT_PTR, I32, I32, I32, F32, F32, F32, I32, INT_PTR, FLOAT_PTR, I32, INT_PTR, I32, INT_PTR]
        L.minigpt4_amd_test_beam_select_host.argtypes = [I32, I32, INT_PTR, FLOAT_PTR, FLOAT_PTR, ctypes.c_uint32, I32, I32, F32, I32, INT_PTR, INT_PTR, INT_PTR, FLOAT_PTR, INT_PTR, INT_PTR]
        L.minigpt4_amd_test_beam_select.argtypes = [I32, INT_PTR, FLOAT_PTR, FLOAT_PTR, ctypes.c_uint32, I32, I32, INT_PTR, INT_PTR]
        L.minigpt4_amd_test_kv_permute.argtypes = [I32, I32, I32, I32, INT_PTR, I32, INT_PTR, I32, I32, VOID_PTR, VOID_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_pen_pick.argtypes = [FLOAT_PTR, I32, I32, I32, INT_PTR, I32, INT_PTR, I32, INT_PTR, FLOAT_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_guide_rows.argtypes = [FLOAT_PTR, I32, I32, I32, INT_PTR, FLOAT_PTR, INT_PTR, I32, FLOAT_PTR, INT_PTR, FLOAT_PTR, INT_PTR, FLOAT_PTR]
        U16P, U32P = P(ctypes.c_uint16), P(ctypes.c_uint32)
        L.minigpt4_amd_test_constraint_compile.argtypes = [CHAR_PTR, I32, U16P, U32P, I32, INT_PTR, ctypes.c_char_p, SIZE_T]
        L.minigpt4_amd_test_constrain_index.argtypes = [P(ctypes.c_uint8), INT_PTR, I32, U16P, U32P, I32, U32P, FLOAT_PTR]
        L.minigpt4_amd_test_constrain_pick.argtypes = [FLOAT_PTR, I32, I32, I32, INT_PTR, I32, INT_PTR, I32, U32P, I32, INT_PTR, INT_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_philox.argtypes = [U32P, U32P, U32P]
        L.minigpt4_amd_test_sample_rule.argtypes = [FLOAT_PTR, I32, F32, F32, ctypes.c_uint32, FLOAT_PTR, INT_PTR]
        L.minigpt4_amd_test_sample_rows.argtypes = [FLOAT_PTR, I32, I32, I32, INT_PTR, I32, INT_PTR, I32, U32P, I32, INT_PTR, FLOAT_PTR, INT_PTR, U64P, INT_PTR, INT_PTR, INT_PTR,
                                                    FLOAT_PTR]
        L.minigpt4_amd_test_sample_chain.argtypes = [FLOAT_PTR, I32, F32, F32, F32, F32, F32, I32, F32, F32, F32, ctypes.c_uint32, FLOAT_PTR, INT_PTR, U64P, FLOAT_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_sample_rows_ex.argtypes = [FLOAT_PTR, I32, I32, I32, INT_PTR, I32, INT_PTR, I32, U32P, I32, INT_PTR, FLOAT_PTR, INT_PTR, U64P, INT_PTR, FLOAT_PTR, INT_PTR,
                                                       INT_PTR, INT_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_draft_sample.argtypes = [FLOAT_PTR, I32, I32, I32, INT_PTR, INT_PTR, I32, U32P, I32, INT_PTR, FLOAT_PTR, INT_PTR, U64P, INT_PTR, I32, INT_PTR, FLOAT_PTR,
                                                     INT_PTR, INT_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_draft_tables.argtypes = [INT_PTR, I32, I32, INT_PTR, I32, I32, F32, F32, F32, I32, INT_PTR, FLOAT_PTR, I32, I32, I32, U16P, U32P, I32, I32, P(ctypes.c_uint8),
                                                     INT_PTR, INT_PTR, INT_PTR, INT_PTR, INT_PTR, I32, INT_PTR, INT_PTR]
        L.minigpt4_amd_test_attn_draft.argtypes = [I32, I32, I32, I32, I32, I32, I32, I32, I32, FLOAT_PTR, FLOAT_PTR, FLOAT_PTR, VOID_PTR, VOID_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_attn_vsplit.argtypes = [I32, I32, I32, I32, I32, I32, I32, INT_PTR, INT_PTR, I32, FLOAT_PTR, FLOAT_PTR, FLOAT_PTR, VOID_PTR, VOID_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_ngram_draft.argtypes = [INT_PTR, I32, I32, I32, I32, INT_PTR]
        L.minigpt4_amd_test_attn_draft_batch.argtypes = [I32, I32, I32, I32, I32, I32, I32, INT_PTR, I32, FLOAT_PTR, FLOAT_PTR, FLOAT_PTR, VOID_PTR, VOID_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_draft_finish_batch.argtypes = [FLOAT_PTR, I32, I32, INT_PTR, INT_PTR, INT_PTR, I32, INT_PTR, INT_PTR, INT_PTR, FLOAT_PTR, INT_PTR]
        L.minigpt4_amd_test_argmax.argtypes = [FLOAT_PTR, I32, INT_PTR, FLOAT_PTR, INT_PTR]
        L.minigpt4_amd_test_step_finish.argtypes = [I32, FLOAT_PTR, I32, I32, I32, INT_PTR, INT_PTR, INT_PTR, INT_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_draft_finish.argtypes = [FLOAT_PTR, I32, I32, INT_PTR, I32, I32, INT_PTR, INT_PTR, INT_PTR, FLOAT_PTR, INT_PTR]
        L.minigpt4_amd_test_step_words.argtypes = [I32, I32, I32, INT_PTR, INT_PTR, I32, INT_PTR, INT_PTR, INT_PTR]
        L.minigpt4_amd_test_gather_rows.argtypes = [FLOAT_PTR, I32, INT_PTR, I32, I32, FLOAT_PTR]
        L.minigpt4_amd_test_attn_rows.argtypes = [I32, I32, I32, I32, I32, I32, I32, I32, FLOAT_PTR, FLOAT_PTR, FLOAT_PTR, VOID_PTR, VOID_PTR, FLOAT_PTR, FLOAT_PTR]
        L.minigpt4_amd_test_attn_prefill_seg.argtypes = [I32, I32, I32, I32, VOID_PTR, VOID_PTR, I32, INT_PTR, FLOAT_PTR, I32, FLOAT_PTR, FLOAT_PTR, INT_PTR, VOID_PTR, VOID_PTR, INT_PTR]
        L.minigpt4_amd_test_rope_kv_seg.argtypes = [I32, I32, I32, I32, I32, INT_PTR, FLOAT_PTR, FLOAT_PTR, FLOAT_PTR, I32, FLOAT_PTR, VOID_PTR, VOID_PTR, FLOAT_PTR, VOID_PTR, VOID_PTR]
        L.minigpt4_amd_last_error.restype = CHAR_PTR
        L.minigpt4_amd_vocab_load.argtypes = [CHAR_PTR]
        L.minigpt4_amd_vocab_load.restype = VOID_PTR
        L.minigpt4_amd_vocab_free.argtypes = [VOID_PTR]
        L.minigpt4_amd_vocab_free.restype = None
        L.minigpt4_amd_vocab_size.argtypes = [VOID_PTR]
        L.minigpt4_amd_vocab_piece.argtypes = [VOID_PTR, I32, INT_PTR]
        L.minigpt4_amd_vocab_piece.restype = VOID_PTR
        L.minigpt4_amd_vocab_tokenize.argtypes = [VOID_PTR, CHAR_PTR, I32, INT_PTR, I32]
        L.minigpt4_amd_inspect_files.argtypes = [CHAR_PTR, CHAR_PTR, INT_PTR, INT_PTR, P(ctypes.c_int64)]
        L.minigpt4_amd_sample_logits.argtypes = [FLOAT_PTR, I32, I32, F32, I32, F32, F32, F32, I32, F32, F32]
        L.minigpt4_amd_resample_coeffs.argtypes = [I32, I32, INT_PTR, INT_PTR, INT_PTR, INT_PTR, SIZE_T]
        L.minigpt4_amd_copy_arenas.argtypes = [VOID_PTR, VOID_PTR]
        L.minigpt4_amd_llm_file_digest.argtypes = [CHAR_PTR, U64P, I32]
        L.minigpt4_amd_quantize_chunk.argtypes = [I32, FLOAT_PTR, VOID_PTR, ctypes.c_int64]
        L.minigpt4_amd_quantize_chunk.restype = ctypes.c_int64
        L.minigpt4_amd_probe_valu.restype = F32
        L.minigpt4_amd_probe_grid_barrier.restype = F32

    # ---------------------------------------------------------------- reference surface
    def panic_if_error(self, error_code: int) -> None:
        if error_code != 0:
            raise RuntimeError(self.library.minigpt4_error_code_to_string(I32(error_code)))

    def minigpt4_model_load(self, model_path: str, llm_model_path: str, verbosity: int = 1, seed: int = 1337, n_ctx: int = 2048,
                            n_batch: int = 512, numa: int = 0) -> MiniGPT4Context:
        ptr = self.library.minigpt4_model_load(model_path.encode(), llm_model_path.encode(), int(verbosity), seed, n_ctx, n_batch, bool(numa))
        if not ptr:
            raise RuntimeError("minigpt4_model_load failed: " + (self.library.minigpt4_amd_last_error() or b"").decode(errors="replace"))
        return MiniGPT4Context(ptr)

    def minigpt4_image_load_from_file(self, ctx: MiniGPT4Context, path: str, flags: int = 0) -> MiniGPT4Image:
        image = MiniGPT4Image()
        self.panic_if_error(self.library.minigpt4_image_load_from_file(ctx.ptr, path.encode(), ctypes.pointer(image), flags))
        return image

    def minigpt4_preprocess_image(self, ctx: MiniGPT4Context, image: MiniGPT4Image, flags: int = 0) -> MiniGPT4Image:
        out = MiniGPT4Image()
        self.panic_if_error(self.library.minigpt4_preprocess_image(ctx.ptr, ctypes.pointer(image), ctypes.pointer(out), flags))
        return out

    def minigpt4_encode_image(self, ctx: MiniGPT4Context, image: MiniGPT4Image, n_threads: int = 0) -> MiniGPT4Embedding:
        embedding = MiniGPT4Embedding()
        self.panic_if_error(self.library.minigpt4_encode_image(ctx.ptr, ctypes.pointer(image), ctypes.pointer(embedding), n_threads))
        return embedding

    def minigpt4_begin_chat_image(self, ctx: MiniGPT4Context, image_embedding: MiniGPT4Embedding, s: str, n_threads: int = 0):
        self.panic_if_error(self.library.minigpt4_begin_chat_image(ctx.ptr, ctypes.pointer(image_embedding), s.encode(), n_threads))

    def _end(self, fn, ctx, n_threads, temp, top_k, top_p, tfs_z, typical_p, repeat_last_n, repeat_penalty, alpha_presence, alpha_frequency,
             mirostat, mirostat_tau, mirostat_eta, penalize_nl) -> str:
        token = ctypes.c_char_p()
        self.panic_if_error(fn(ctx.ptr, ctypes.byref(token), n_threads, temp, top_k, top_p, tfs_z, typical_p, repeat_last_n, repeat_penalty,
                               alpha_presence, alpha_frequency, mirostat, mirostat_tau, mirostat_eta, penalize_nl))
        return (token.value or b"").decode("utf-8", errors="replace")

    def minigpt4_end_chat_image(self, ctx, n_threads=0, temp=0.8, top_k=40, top_p=0.9, tfs_z=1.0, typical_p=1.0, repeat_last_n=64,
                                repeat_penalty=1.1, alpha_presence=1.0, alpha_frequency=1.0, mirostat=0, mirostat_tau=5.0, mirostat_eta=1.0,
                                penalize_nl=1) -> str:
        return self._end(self.library.minigpt4_end_chat_image, ctx, n_threads, temp, top_k, top_p, tfs_z, typical_p, repeat_last_n, repeat_penalty,
                         alpha_presence, alpha_frequency, mirostat, mirostat_tau, mirostat_eta, penalize_nl)

    def minigpt4_system_prompt(self, ctx: MiniGPT4Context, n_threads: int = 0):
        self.panic_if_error(self.library.minigpt4_system_prompt(ctx.ptr, n_threads))

    def minigpt4_begin_chat(self, ctx: MiniGPT4Context, s: str, n_threads: int = 0):
        self.panic_if_error(self.library.minigpt4_begin_chat(ctx.ptr, s.encode(), n_threads))

    def minigpt4_end_chat(self, ctx, n_threads=0, temp=0.8, top_k=40, top_p=0.9, tfs_z=1.0, typical_p=1.0, repeat_last_n=64, repeat_penalty=1.1,
                          alpha_presence=1.0, alpha_frequency=1.0, mirostat=0, mirostat_tau=5.0, mirostat_eta=1.0, penalize_nl=1) -> str:
        return self._end(self.library.minigpt4_end_chat, ctx, n_threads, temp, top_k, top_p, tfs_z, typical_p, repeat_last_n, repeat_penalty,
                         alpha_presence, alpha_frequency, mirostat, mirostat_tau, mirostat_eta, penalize_nl)

    def minigpt4_reset_chat(self, ctx: MiniGPT4Context):
        self.panic_if_error(self.library.minigpt4_reset_chat(ctx.ptr))

    def minigpt4_contains_eos_token(self, s: str) -> bool:
        return bool(self.library.minigpt4_contains_eos_token(s.encode()))

    def minigpt4_is_eos(self, s: str) -> bool:
        return bool(self.library.minigpt4_is_eos(s.encode()))

    def minigpt4_free(self, ctx: MiniGPT4Context) -> None:
        self.panic_if_error(self.library.minigpt4_free(ctx.ptr))
        ctx.ptr = None

    def minigpt4_free_image(self, image: MiniGPT4Image) -> None:
        self.panic_if_error(self.library.minigpt4_free_image(ctypes.pointer(image)))

    def minigpt4_free_embedding(self, embedding: MiniGPT4Embedding) -> None:
        self.panic_if_error(self.library.minigpt4_free_embedding(ctypes.pointer(embedding)))

    def minigpt4_error_code_to_string(self, error_code: int) -> str:
        return self.library.minigpt4_error_code_to_string(error_code).decode()

    def minigpt4_quantize_model(self, in_path: str, out_path: str, data_type: DataType):
        self.panic_if_error(self.library.minigpt4_quantize_model(in_path.encode(), out_path.encode(), int(data_type)))

    def minigpt4_set_verbosity(self, verbosity: Verbosity):
        self.library.minigpt4_set_verbosity(int(verbosity))

    # ---------------------------------------------------------------- additive surface (numpy in / out)
    def amd_device_count(self) -> int:
        return int(self.library.minigpt4_amd_device_count())

    # multi-GPU load (include/minigpt4_amd.h)
    def amd_plan_arenas(self, vision_path: str, llm_path: str) -> dict:
        """Arena layout the two files produce, computed on the host (no GPU): {"llm_bytes", "vision_bytes", "llm_hash", "vision_hash"}."""
        lb, vb, lh, vh = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint64(), ctypes.c_uint64()
        rc = self.library.minigpt4_amd_plan_arenas(vision_path.encode(), llm_path.encode(), ctypes.byref(lb), ctypes.byref(vb), ctypes.byref(lh), ctypes.byref(vh))
        if rc:
            raise RuntimeError(f"plan_arenas failed ({rc}): " + self.library.minigpt4_amd_last_error().decode())
        return {"llm_bytes": lb.value, "vision_bytes": vb.value, "llm_hash": lh.value, "vision_hash": vh.value}

    def amd_arena_plan(self, ctx) -> dict:
        lb, vb, lh, vh = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint64(), ctypes.c_uint64()
        assert self.library.minigpt4_amd_arena_plan(ctx.ptr, ctypes.byref(lb), ctypes.byref(vb), ctypes.byref(lh), ctypes.byref(vh)) == 0
        return {"llm_bytes": lb.value, "vision_bytes": vb.value, "llm_hash": lh.value, "vision_hash": vh.value}

    def amd_arena_checksum(self, ctx, which: int) -> int:
        v = ctypes.c_uint64()
        assert self.library.minigpt4_amd_arena_checksum(ctx.ptr, which, ctypes.byref(v)) == 0
        return int(v.value)

    # several conversations per context (include/minigpt4_amd.h): the reference calls act on the selected one
    def amd_dist_info(self, ctx) -> dict:
        """what the native (in-library RCCL) weight broadcast of this context's load did: world size, rank, milliseconds (0.0 for an ordinary load)"""
        w, r, ms = I32(), I32(), F32()
        assert self.library.minigpt4_amd_dist_info(ctx.ptr, ctypes.byref(w), ctypes.byref(r), ctypes.byref(ms)) == 0
        return {"world": w.value, "rank": r.value, "bcast_ms": ms.value}

    def amd_set_parity(self, ctx, on: bool):
        """Parity mode (MINIGPT4_PARITY): the language path adds its fp32 terms in the CPU oracle's order -- bit-identical logits, slow."""
        if self.library.minigpt4_amd_set_parity(ctx.ptr, 1 if on else 0):
            raise RuntimeError("minigpt4_amd_set_parity failed")

    def amd_set_conversations(self, ctx, n: int):
        if self.library.minigpt4_amd_set_conversations(ctx.ptr, n):
            raise RuntimeError("set_conversations failed: " + self.library.minigpt4_amd_last_error().decode())

    def amd_select_conversation(self, ctx, slot: int):
        if self.library.minigpt4_amd_select_conversation(ctx.ptr, slot):
            raise RuntimeError("select_conversation: index out of range")

    def amd_end_chat_batch(self, ctx, slots: Sequence[int], temp=0.8, top_k=40, top_p=0.9, tfs_z=1.0, typical_p=1.0, mirostat=0, mirostat_tau=5.0,
                           mirostat_eta=1.0) -> List[str]:
        """One minigpt4_end_chat step for several conversations in one pass over the weights; returns one piece per conversation."""
        sl = np.ascontiguousarray(slots, np.int32)
        toks = (ctypes.c_char_p * len(sl))()
        rc = self.library.minigpt4_amd_end_chat_batch(ctx.ptr, sl.ctypes.data_as(INT_PTR), len(sl), toks, temp, top_k, top_p, tfs_z, typical_p, mirostat, mirostat_tau, mirostat_eta)
        if rc:
            raise RuntimeError("end_chat_batch failed: " + self.library.minigpt4_amd_last_error().decode())
        return [(t or b"").decode("utf-8", errors="replace") for t in toks]

    def amd_prefill_batch(self, ctx, slots: Sequence[int]):
        """Evaluate the queued prompt rows of several conversations, packed into chunks of <= n_batch rows (one pass over the weights per chunk)."""
        sl = np.ascontiguousarray(slots, np.int32)
        rc = self.library.minigpt4_amd_prefill_batch(ctx.ptr, sl.ctypes.data_as(INT_PTR), len(sl))
        if rc:
            raise RuntimeError("prefill_batch failed: " + self.library.minigpt4_amd_last_error().decode())

    def amd_eval_batch(self, ctx, slots: Sequence[int], tokens: Sequence[int]) -> List[int]:
        """One batched decode step with GIVEN next tokens (teacher forcing); returns every conversation's own greedy choice."""
        n = len(slots)
        assert len(tokens) == n
        sl, tk, out = (ctypes.c_int32 * n)(*slots), (ctypes.c_int32 * n)(*[int(t) for t in tokens]), (ctypes.c_int32 * n)()
        if self.library.minigpt4_amd_eval_batch(ctx.ptr, sl, n, tk, out):
            raise RuntimeError("minigpt4_amd_eval_batch failed: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return [int(x) for x in out]

    def amd_shift_context(self, ctx, n_keep: int, n_discard: int):
        """Context shift of the selected conversation: drop rows [n_keep, n_keep + n_discard), slide the rest down, re-rotate their keys (include/minigpt4_amd.h)."""
        if self.library.minigpt4_amd_shift_context(ctx.ptr, int(n_keep), int(n_discard)):
            raise RuntimeError("shift_context failed: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))

    def amd_set_context_shift(self, ctx, n_keep: int):
        """Automatic context shift of this context when an add would overflow, keeping the first n_keep rows; n_keep < 0 = off (the default)."""
        if self.library.minigpt4_amd_set_context_shift(ctx.ptr, int(n_keep)):
            raise RuntimeError("set_context_shift failed: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))

    PREFIX_INFO_FIELDS = ("max_rows", "stored_rows", "hits", "rows_reused_total", "captures", "rows_reused_by_last_pass", "hit_launches")

    def amd_fork_conversation(self, ctx, src: int, dsts: Sequence[int], n_rows: int = -1):
        """Copy conversation `src` into the conversations `dsts` (one launch): n_rows = -1 the whole state (rows, logits, greedy token: sample at once), otherwise the
        first n_rows rows only (no logits: add rows before sampling).  include/minigpt4_amd.h"""
        d = np.ascontiguousarray(dsts, np.int32)
        if self.library.minigpt4_amd_fork_conversation(ctx.ptr, int(src), d.ctypes.data_as(INT_PTR), len(d), int(n_rows)):
            raise RuntimeError("fork_conversation failed: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))

    def amd_set_prefix_cache(self, ctx, max_rows: int):
        """Prefix cache of this context: 0 = off (the default); > 0 = one stored prefix of up to max_rows rows, emptied (and its counters zeroed) by every call."""
        if self.library.minigpt4_amd_set_prefix_cache(ctx.ptr, int(max_rows)):
            raise RuntimeError("set_prefix_cache failed: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))

    def amd_prefix_cache_info(self, ctx) -> dict:
        out = (ctypes.c_int32 * len(self.PREFIX_INFO_FIELDS))()
        if self.library.minigpt4_amd_prefix_cache_info(ctx.ptr, out):
            raise RuntimeError("prefix_cache_info failed: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return dict(zip(self.PREFIX_INFO_FIELDS, (int(x) for x in out)))

    def amd_score_tokens(self, ctx, tokens: Sequence[int], want_logits: bool = False, top_n: int = 0) -> dict:
        """Append `tokens` to the selected conversation and evaluate them like amd_eval_tokens + amd_logits (same state afterwards), reporting per token the
        log-probability the model gave it.  Entry i describes the distribution tokens[i] is drawn from (entry 0: the conversation's logits from before the call; none:
        logprob 0, greedy -1).  dict(logprob [n] f32, greedy [n] i32, greedy_logprob [n] f32[, logits [n][n_vocab] f32]).  top_n > 0 (minigpt4_amd_score_tokens_top;
        not together with want_logits) adds rank [n] i32 (how many tokens the model preferred to tokens[i]; -1 without a distribution), top_ids [n][top_n] i32 and
        top_logprobs [n][top_n] f32 (logit descending, equal logits by ascending id); greedy / greedy_logprob are then column 0.  include/minigpt4_amd.h"""
        t = np.ascontiguousarray(tokens, np.int32)
        n = len(t)
        if top_n:
            if want_logits:
                raise ValueError("amd_score_tokens: top_n > 0 and want_logits=True exclude each other")
            lp, rk = np.zeros(n, np.float32), np.zeros(n, np.int32)
            ti, tl = np.zeros((n, max(int(top_n), 1)), np.int32), np.zeros((n, max(int(top_n), 1)), np.float32)
            if self.library.minigpt4_amd_score_tokens_top(ctx.ptr, t.ctypes.data_as(INT_PTR), n, int(top_n), lp.ctypes.data_as(FLOAT_PTR), rk.ctypes.data_as(INT_PTR),
                                                          ti.ctypes.data_as(INT_PTR), tl.ctypes.data_as(FLOAT_PTR)):
                raise RuntimeError("score_tokens_top failed: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
            return dict(logprob=lp, greedy=ti[:, 0].copy(), greedy_logprob=tl[:, 0].copy(), rank=rk, top_ids=ti, top_logprobs=tl)
        lp, gr, glp = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        lg = np.zeros((n, self.library.minigpt4_amd_n_vocab(ctx.ptr)), np.float32) if want_logits else None
        if self.library.minigpt4_amd_score_tokens(ctx.ptr, t.ctypes.data_as(INT_PTR), n, lp.ctypes.data_as(FLOAT_PTR), gr.ctypes.data_as(INT_PTR), glp.ctypes.data_as(FLOAT_PTR),
                                                  lg.ctypes.data_as(FLOAT_PTR) if want_logits else None):
            raise RuntimeError("score_tokens failed: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        out = dict(logprob=lp, greedy=gr, greedy_logprob=glp)
        if want_logits:
            out["logits"] = lg
        return out

    def amd_set_speculation(self, ctx, max_draft: int) -> None:
        """Draft verification for this context: max_draft 1 .. 7 allocates what amd_verify_draft / amd_decode_lookup need, 0 (the default) frees it.  include/minigpt4_amd.h"""
        if self.library.minigpt4_amd_set_speculation(ctx.ptr, int(max_draft)):
            raise RuntimeError("set_speculation failed: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))

    def amd_verify_draft(self, ctx, draft: Sequence[int]) -> dict:
        """One weight pass over the selected conversation's greedy token and the guessed tokens behind it; keeps the guesses the pass's own logits confirm.
        dict(ids [1 + m] i32: the tokens plain greedy decoding would have emitted, row_greedy [1 + len(draft)] i32: the first argmax of every evaluated row, -1 for a
        row not evaluated).  include/minigpt4_amd.h"""
        d = np.ascontiguousarray(draft, np.int32)
        n = len(d)
        ids, rg, n_out = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32), np.zeros(1, np.int32)
        if self.library.minigpt4_amd_verify_draft(ctx.ptr, d.ctypes.data_as(INT_PTR) if n else None, n, ids.ctypes.data_as(INT_PTR), n_out.ctypes.data_as(INT_PTR),
                                                  rg.ctypes.data_as(INT_PTR)):
            raise RuntimeError("verify_draft failed: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return dict(ids=ids[:int(n_out[0])].copy(), row_greedy=rg)

    def amd_decode_lookup(self, ctx, corpus: Sequence[int], max_tokens: int, ngram_max: int = 3, ngram_min: int = 1, n_draft: int = 4) -> dict:
        """Greedy generation of up to max_tokens tokens with drafts looked up in corpus + the tokens emitted so far (n-gram lookup decoding).
        dict(tokens [n] i32, passes, steps, sent, accepted): verify passes, plain decode steps, draft tokens sent and accepted.  include/minigpt4_amd.h"""
        c = np.ascontiguousarray(corpus, np.int32)
        out, n, st = np.zeros(max(int(max_tokens), 1), np.int32), np.zeros(1, np.int32), np.zeros(4, np.int32)
        if self.library.minigpt4_amd_decode_lookup(ctx.ptr, c.ctypes.data_as(INT_PTR) if len(c) else None, len(c), int(max_tokens), int(ngram_max), int(ngram_min), int(n_draft),
                                                   out.ctypes.data_as(INT_PTR), n.ctypes.data_as(INT_PTR), st.ctypes.data_as(INT_PTR)):
            raise RuntimeError("decode_lookup failed: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return dict(tokens=out[:int(n[0])].copy(), passes=int(st[0]), steps=int(st[1]), sent=int(st[2]), accepted=int(st[3]))

    SPECULATION_INFO_FIELDS = ("passes", "rows", "sent", "accepted", "launches", "stuck", "cut")

    def amd_verify_draft_sampled(self, ctx, draft: Sequence[int], temp=0.8, top_k=40, top_p=0.9, want_rows: bool = False, want_logits: bool = False, tfs_z=1.0, typical_p=1.0,
                                 min_p=0.0) -> dict:
        """amd_verify_draft under sampling: every row of the pass is sampled with the draw plain sampled decoding (amd_end_chat_batch_sampled) would use at its position; a
        draft token is kept exactly when the sample of the row before it equals it.  dict(ids [1 + m] i32: the emitted tokens; next: the sample of row m, which the next
        decision recomputes (draft behind it); want_rows: row_sampled [1 + len(draft)] i32, -1 for a row not evaluated; want_logits: row_logits [1 + len(draft)][n_vocab]
        f32, NaN rows where not evaluated).  include/minigpt4_amd.h states the rule.  A non-neutral tfs_z, typical_p or min_p sends the call to
        minigpt4_amd_verify_draft_sampled_ex: every row is decided by the extended rule (no mirostat there)."""
        ex = self._chain_args("verify_draft_sampled", tfs_z, typical_p, min_p, 0, 5.0, 0.1)
        d = np.ascontiguousarray(draft, np.int32).reshape(-1)
        n = len(d)
        ids, n_out, nxt = np.zeros(n + 1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
        rs = np.zeros(n + 1, np.int32) if want_rows else None
        rl = np.full((n + 1, int(self.library.minigpt4_amd_n_vocab(ctx.ptr))), np.nan, np.float32) if want_logits and ctx is not None else None
        head = (ctx.ptr if ctx is not None else None, d.ctypes.data_as(INT_PTR) if n else None, n, float(temp), int(top_k), float(top_p))
        tail = (ids.ctypes.data_as(INT_PTR), n_out.ctypes.data_as(INT_PTR), nxt.ctypes.data_as(INT_PTR), rs.ctypes.data_as(INT_PTR) if rs is not None else None,
                rl.ctypes.data_as(FLOAT_PTR) if rl is not None else None)
        if ex:
            rc = self.library.minigpt4_amd_verify_draft_sampled_ex(*head, float(tfs_z), float(typical_p), float(min_p), *tail)
        else:
            rc = self.library.minigpt4_amd_verify_draft_sampled(*head, *tail)
        if rc:
            raise RuntimeError("verify_draft_sampled failed: " + self._err())
        out = dict(ids=ids[:int(n_out[0])].copy(), next=int(nxt[0]))
        if rs is not None:
            out["row_sampled"] = rs
        if rl is not None:
            out["row_logits"] = rl
        return out

    def amd_decode_lookup_sampled(self, ctx, corpus: Sequence[int], max_tokens: int, ngram_max: int = 3, ngram_min: int = 1, n_draft: int = 4, temp=0.8, top_k=40,
                                  top_p=0.9, tfs_z=1.0, typical_p=1.0, min_p=0.0) -> dict:
        """amd_decode_lookup under sampling (amd_verify_draft_sampled per step; no match: its n_draft = 0 form).  dict(tokens [n] i32, passes, steps, sent, accepted).
        A non-neutral tfs_z, typical_p or min_p: minigpt4_amd_decode_lookup_sampled_ex, the extended rule on every row."""
        ex = self._chain_args("decode_lookup_sampled", tfs_z, typical_p, min_p, 0, 5.0, 0.1)
        c = np.ascontiguousarray(corpus, np.int32).reshape(-1)
        out, n, st = np.zeros(max(int(max_tokens), 1), np.int32), np.zeros(1, np.int32), np.zeros(4, np.int32)
        head = (ctx.ptr if ctx is not None else None, c.ctypes.data_as(INT_PTR) if len(c) else None, len(c), int(max_tokens), int(ngram_max), int(ngram_min), int(n_draft),
                float(temp), int(top_k), float(top_p))
        tail = (out.ctypes.data_as(INT_PTR), n.ctypes.data_as(INT_PTR), st.ctypes.data_as(INT_PTR))
        if ex:
            rc = self.library.minigpt4_amd_decode_lookup_sampled_ex(*head, float(tfs_z), float(typical_p), float(min_p), *tail)
        else:
            rc = self.library.minigpt4_amd_decode_lookup_sampled(*head, *tail)
        if rc:
            raise RuntimeError("decode_lookup_sampled failed: " + self._err())
        return dict(tokens=out[:int(n[0])].copy(), passes=int(st[0]), steps=int(st[1]), sent=int(st[2]), accepted=int(st[3]))

    def amd_speculation_info(self, ctx) -> dict:
        """dict(passes: sampled verify passes, rows: rows they evaluated, sent / accepted: draft tokens, launches: sampling launches made by these calls, stuck: picks
        without a participating id, cut: draft tokens cut by a constraint) -- of the context so far."""
        out = (ctypes.c_int64 * 8)()
        if self.library.minigpt4_amd_speculation_info(ctx.ptr if ctx is not None else None, out):
            raise RuntimeError("speculation_info failed: " + self._err())
        return dict(zip(self.SPECULATION_INFO_FIELDS, (int(x) for x in out)))

    SPECULATION_BATCH_INFO_FIELDS = ("passes", "rows", "groups", "sent", "accepted", "plain_steps", "cut")

    def amd_verify_draft_batch(self, ctx, slots: Sequence[int], drafts: Sequence[Sequence[int]]) -> dict:
        """amd_verify_draft for several conversations in ONE weight pass: conversation slots[i] brings its raw greedy token and the guesses drafts[i] (may be empty).
        dict(ids: list of [1 + m_i] i32 arrays -- the tokens plain greedy decoding would have emitted, empty for a conversation left out (context full);
        row_greedy [n][8] i32: the first argmax of every evaluated row, -1 behind them).  include/minigpt4_amd.h states the rule."""
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        n = len(sl)
        if len(drafts) != n:
            raise ValueError("amd_verify_draft_batch: one draft (possibly empty) per conversation")
        cnt = np.array([len(d) for d in drafts], np.int32)
        flat = np.ascontiguousarray([t for d in drafts for t in d], np.int32).reshape(-1)
        ids, n_out, rg = np.zeros((max(n, 1), 8), np.int32), np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 8), np.int32)
        if self.library.minigpt4_amd_verify_draft_batch(ctx.ptr if ctx is not None else None, sl.ctypes.data_as(INT_PTR) if n else None, n,
                                                        flat.ctypes.data_as(INT_PTR) if flat.size else None, cnt.ctypes.data_as(INT_PTR) if n else None,
                                                        ids.ctypes.data_as(INT_PTR), n_out.ctypes.data_as(INT_PTR), rg.ctypes.data_as(INT_PTR)):
            raise RuntimeError("verify_draft_batch failed: " + self._err())
        return dict(ids=[ids[i, :int(n_out[i])].copy() for i in range(n)], row_greedy=rg[:n])

    def amd_decode_lookup_batch(self, ctx, slots: Sequence[int], corpora: Sequence[Sequence[int]], max_tokens: int, ngram_max: int = 3, ngram_min: int = 1,
                                n_draft: int = 4) -> list:
        """amd_decode_lookup for several conversations: each its own corpus (may be empty), drafter, budget and end; every iteration is one amd_verify_draft_batch over the
        conversations still running.  A list of dict(tokens [n_i] i32, passes, steps, sent, accepted), one per conversation."""
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        n = len(sl)
        if len(corpora) != n:
            raise ValueError("amd_decode_lookup_batch: one corpus (possibly empty) per conversation")
        cnt = np.array([len(c) for c in corpora], np.int32)
        flat = np.ascontiguousarray([t for c in corpora for t in c], np.int32).reshape(-1)
        mt = max(int(max_tokens), 1)
        out, nt, st = np.zeros((max(n, 1), mt), np.int32), np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 4), np.int32)
        if self.library.minigpt4_amd_decode_lookup_batch(ctx.ptr if ctx is not None else None, sl.ctypes.data_as(INT_PTR) if n else None, n,
                                                         flat.ctypes.data_as(INT_PTR) if flat.size else None, cnt.ctypes.data_as(INT_PTR) if n else None, int(max_tokens),
                                                         int(ngram_max), int(ngram_min), int(n_draft), out.ctypes.data_as(INT_PTR), nt.ctypes.data_as(INT_PTR),
                                                         st.ctypes.data_as(INT_PTR)):
            raise RuntimeError("decode_lookup_batch failed: " + self._err())
        return [dict(tokens=out[i, :int(nt[i])].copy(), passes=int(st[i, 0]), steps=int(st[i, 1]), sent=int(st[i, 2]), accepted=int(st[i, 3])) for i in range(n)]

    def amd_speculation_batch_info(self, ctx) -> dict:
        """dict(passes, rows, groups, sent, accepted: of the verify passes over several conversations; plain_steps: calls without a draft that took the plain batched step;
        cut: draft tokens cut for room) -- of the context so far."""
        out = (ctypes.c_int64 * 8)()
        if self.library.minigpt4_amd_speculation_batch_info(ctx.ptr if ctx is not None else None, out):
            raise RuntimeError("speculation_batch_info failed: " + self._err())
        return dict(zip(self.SPECULATION_BATCH_INFO_FIELDS, (int(x) for x in out)))

    def amd_test_attn_draft_batch(self, mode: int, q: np.ndarray, k: np.ndarray, v: np.ndarray, kc: np.ndarray, vc: np.ndarray, n_head: int, groups, computed_exp: bool = True,
                                  vs: int = 1):
        """The attention of the verify pass over several conversations (mode 0: launch_mdraft_begin + ONE launch_attn_llm_draft_batched; mode 1: one launch_attn_llm_draft
        per group) for the packed rows q, k, v [N][E]; groups [n][3] = (slot, p0, R) in row order; fp16 caches [n_slot][n_ctx][E] as uint16 patterns.  Returns
        (out [N][E], kc, vc) -- copies.  ValueError: arguments the hook refuses before it looks for a device."""
        q, k, v = (np.ascontiguousarray(x, np.float32) for x in (q, k, v))
        kc, vc = np.array(kc, np.uint16, order="C"), np.array(vc, np.uint16, order="C")
        g = np.ascontiguousarray(groups, np.int32).reshape(-1, 3)
        N, E = q.shape
        S, C, _ = kc.shape
        if int(g[:, 2].sum()) != N or k.shape != q.shape or v.shape != q.shape or vc.shape != kc.shape or kc.shape[2] != E:
            raise ValueError("amd_test_attn_draft_batch: q, k, v [sum R][E], caches [n_slot][n_ctx][E]")
        out = np.zeros_like(q)
        self._step_rc("test_attn_draft_batch", self.library.minigpt4_amd_test_attn_draft_batch(
            int(mode), int(vs), n_head, E // n_head, C, S, len(g), g.ctypes.data_as(INT_PTR), int(computed_exp), q.ctypes.data_as(FLOAT_PTR), k.ctypes.data_as(FLOAT_PTR),
            v.ctypes.data_as(FLOAT_PTR), kc.ctypes.data_as(VOID_PTR), vc.ctypes.data_as(VOID_PTR), out.ctypes.data_as(FLOAT_PTR)))
        return out, kc, vc

    def amd_test_draft_finish_batch(self, logits: np.ndarray, tok: Sequence[int], row_slot: Sequence[int], row_pos: Sequence[int], n_past, argmax, feed, slot_logits) -> dict:
        """launch_mdraft_begin + ONE launch_draft_finish_batch on logits [N][n_vocab] with the pass's row tokens, conversations and positions.  dict(m [N] i32: a group's
        first row holds its m, every other row -1; row_greedy [N] i32; res [129]: the whole block and its guard word; n_past, argmax, feed, slot_logits after the launches)."""
        lg = np.ascontiguousarray(logits, np.float32)
        if lg.ndim != 2:
            raise ValueError("amd_test_draft_finish_batch: logits [N][n_vocab]")
        N = lg.shape[0]
        tk, rs, rp = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (tok, row_slot, row_pos))
        if not (tk.size == rs.size == rp.size == N):
            raise ValueError("amd_test_draft_finish_batch: one token, slot and position per row")
        st, keep = self._step_state(n_past, argmax, feed, slot_logits, lg.shape[1])
        res = np.zeros(129, np.int32)
        self._step_rc("test_draft_finish_batch", self.library.minigpt4_amd_test_draft_finish_batch(
            lg.ctypes.data_as(FLOAT_PTR) if lg.size else None, N, lg.shape[1], tk.ctypes.data_as(INT_PTR) if N else None, rs.ctypes.data_as(INT_PTR) if N else None,
            rp.ctypes.data_as(INT_PTR) if N else None, len(st[0]) - 1, st[0].ctypes.data_as(INT_PTR), st[1].ctypes.data_as(INT_PTR), st[2].ctypes.data_as(INT_PTR),
            keep.ctypes.data_as(FLOAT_PTR), res.ctypes.data_as(INT_PTR)))
        return dict(m=res[:N].copy(), row_greedy=res[64:64 + N].copy(), res=res, n_past=st[0], argmax=st[1], feed=st[2], slot_logits=keep)

    def amd_test_draft_sample(self, logits: np.ndarray, n_vocab: int, rows: np.ndarray, table: np.ndarray, params, top_k, seed_draws, row_tok: Sequence[int], slot: int,
                              state: np.ndarray, slot_logits: np.ndarray, bitmaps=None, bitmap_of_row=None) -> dict:
        """The sampled verify pass's epilogue alone (include/minigpt4_amd_test.h): k_sample_rows over the R rows of host logits [R][ld] (descriptors as
        amd_test_sample_rows, descriptor r on row r), then k_draft_sample_finish with the pass's row tokens on a two-slot state [2][3] (n_past, argmax, feed) and the
        slots' logits rows [2][n_vocab].  dict(m, picks [R], stuck [R], res [17]; pick, stuck, word, n_cand, kept, ids, p as amd_test_sample_rows; state [2][3],
        slot_logits [2][n_vocab] afterwards; ms: k_draft_sample_finish alone)."""
        lg = np.ascontiguousarray(logits, np.float32)
        assert lg.ndim == 2
        R = lg.shape[0]
        rw = np.ascontiguousarray(rows, np.int32).reshape(-1, 8)
        tb = np.ascontiguousarray(table, np.int32).reshape(-1, 4)
        pr = np.ascontiguousarray(params, np.float32).reshape(-1, 2)
        tk = np.ascontiguousarray(top_k, np.int32).reshape(-1)
        sd = np.ascontiguousarray(seed_draws, np.uint64).reshape(-1, 2)
        W = ((int(n_vocab) + 31) // 32 + 3) // 4 * 4
        bm = np.zeros((0, W), np.uint32) if bitmaps is None else np.ascontiguousarray(bitmaps, np.uint32)
        assert bm.ndim == 2 and bm.shape[1] == W
        br = np.full(R, -1, np.int32) if bitmap_of_row is None else np.ascontiguousarray(bitmap_of_row, np.int32).reshape(-1)
        rt = np.ascontiguousarray(row_tok, np.int32).reshape(-1)
        st = np.ascontiguousarray(state, np.int32).copy()
        keep = np.ascontiguousarray(slot_logits, np.float32).copy()
        assert len(rw) == R and len(pr) == R and len(tk) == R and len(sd) == R and len(br) == R and len(rt) == R and st.shape == (2, 3) and keep.shape == (2, int(n_vocab))
        out, res, ms = np.zeros((max(R, 1), 5 + 128), np.int32), np.zeros(17, np.int32), ctypes.c_float()
        U32P = ctypes.POINTER(ctypes.c_uint32)
        rc = self.library.minigpt4_amd_test_draft_sample(lg.ctypes.data_as(FLOAT_PTR), R, int(n_vocab), lg.shape[1], rw.ctypes.data_as(INT_PTR),
                                                         tb.ctypes.data_as(INT_PTR) if len(tb) else None, len(tb), bm.ctypes.data_as(U32P) if len(bm) else None, len(bm),
                                                         br.ctypes.data_as(INT_PTR), pr.ctypes.data_as(FLOAT_PTR), tk.ctypes.data_as(INT_PTR),
                                                         sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), rt.ctypes.data_as(INT_PTR), int(slot), st.ctypes.data_as(INT_PTR),
                                                         keep.ctypes.data_as(FLOAT_PTR), res.ctypes.data_as(INT_PTR), out.ctypes.data_as(INT_PTR), ctypes.byref(ms))
        if rc:
            raise RuntimeError(f"test_draft_sample rc={rc}: " + self._err())
        return dict(m=int(res[0]), picks=res[1:1 + R].copy(), stuck_flags=res[9:9 + R].copy(), res=res, pick=out[:, 0].copy(), stuck=out[:, 1].copy(),
                    word=out[:, 2].copy().view(np.uint32), n_cand=out[:, 3].copy(), kept=out[:, 4].copy(), ids=out[:, 5:69].copy(),
                    p=np.ascontiguousarray(out[:, 69:133]).view(np.float32), state=st, slot_logits=keep, ms=float(ms.value))

    # ---- the greedy step epilogues alone (include/minigpt4_amd_test.h states the rule: the first maximum over the non-NaN entries, 0 when there is none above -inf).
    # State arrays are [n_slot + 1] words / [n_slot + 1][n_vocab] floats, the last word / row a guard; the wrappers copy them and return the copies after the launch.
    # ValueError: arguments the hook refuses before it looks for a device.
    def _step_rc(self, name: str, rc: int) -> None:
        if rc == 1:
            raise ValueError(f"amd_{name}: bad arguments")
        if rc:
            raise RuntimeError(f"{name} rc={rc}: " + self._err())

    @staticmethod
    def _step_state(n_past, argmax, feed, slot_logits=None, n_vocab: int = 0):
        st = [np.ascontiguousarray(a, np.int32).reshape(-1).copy() for a in (n_past, argmax, feed)]
        if not (len(st[0]) == len(st[1]) == len(st[2]) and len(st[0]) >= 2):
            raise ValueError("state arrays: n_slot + 1 words each")
        keep = None
        if slot_logits is not None:
            keep = np.ascontiguousarray(slot_logits, np.float32).copy()
            if keep.shape != (len(st[0]), int(n_vocab)):
                raise ValueError("slot_logits: [n_slot + 1][n_vocab]")
        return st, keep

    def amd_test_argmax(self, logits: np.ndarray, n: Optional[int] = None):
        """ONE launch_argmax on logits[n]: (id, partial_values [64] f32, partial_ids [64] i32) -- the partials are what the 64 workgroups of the first launch left."""
        lg = np.ascontiguousarray(logits, np.float32).reshape(-1)
        n = lg.size if n is None else int(n)
        if n > lg.size:
            raise ValueError("amd_test_argmax: n beyond the row")
        out, pv, pi = ctypes.c_int32(-2), np.zeros(64, np.float32), np.zeros(64, np.int32)
        self._step_rc("test_argmax", self.library.minigpt4_amd_test_argmax(lg.ctypes.data_as(FLOAT_PTR) if lg.size else None, n, ctypes.byref(out), pv.ctypes.data_as(FLOAT_PTR),
                                                                            pi.ctypes.data_as(INT_PTR)))
        return int(out.value), pv, pi

    def amd_test_step_finish(self, form: int, logits: np.ndarray, slots_or_fin, n_past, argmax, feed, slot_logits) -> dict:
        """form 0: ONE launch_batch_finish, slots_or_fin = row_slot [rows]; form 1: ONE launch_seg_finish, slots_or_fin = fin [rows][2] (slot, new position), on logits
        [rows][n_vocab].  dict(n_past, argmax, feed [n_slot + 1], slot_logits [n_slot + 1][n_vocab]) after the launch."""
        lg = np.ascontiguousarray(logits, np.float32)
        if lg.ndim != 2:
            raise ValueError("amd_test_step_finish: logits [rows][n_vocab]")
        rows, nv = lg.shape
        d = np.ascontiguousarray(slots_or_fin, np.int32).reshape(-1)
        if d.size != rows * (2 if form == 1 else 1):
            raise ValueError("amd_test_step_finish: one slot (form 1: one pair) per row")
        st, keep = self._step_state(n_past, argmax, feed, slot_logits, nv)
        self._step_rc("test_step_finish", self.library.minigpt4_amd_test_step_finish(int(form), lg.ctypes.data_as(FLOAT_PTR) if lg.size else None, rows, nv, len(st[0]) - 1,
                                                                                      d.ctypes.data_as(INT_PTR) if d.size else None, st[0].ctypes.data_as(INT_PTR),
                                                                                      st[1].ctypes.data_as(INT_PTR), st[2].ctypes.data_as(INT_PTR), keep.ctypes.data_as(FLOAT_PTR)))
        return dict(n_past=st[0], argmax=st[1], feed=st[2], slot_logits=keep)

    def amd_test_draft_finish(self, logits: np.ndarray, tok: Sequence[int], slot: int, n_past, argmax, feed, slot_logits, R: Optional[int] = None) -> dict:
        """ONE launch_draft_finish on logits [R][n_vocab] with the pass's row tokens tok[R] for conversation `slot`.  dict(m, res [10]: m, 8 ids (0xFF fill behind R), a
        guard word; n_past, argmax, feed, slot_logits after the launch).  R: the row count handed to the hook (default: the rows of `logits`)."""
        lg = np.ascontiguousarray(logits, np.float32)
        if lg.ndim != 2:
            raise ValueError("amd_test_draft_finish: logits [R][n_vocab]")
        R = lg.shape[0] if R is None else int(R)
        tk = np.ascontiguousarray(tok, np.int32).reshape(-1)
        if 1 <= R <= 8 and (lg.shape[0] != R or tk.size != R):
            raise ValueError("amd_test_draft_finish: R rows and R tokens")
        st, keep = self._step_state(n_past, argmax, feed, slot_logits, lg.shape[1])
        res = np.zeros(10, np.int32)
        self._step_rc("test_draft_finish", self.library.minigpt4_amd_test_draft_finish(lg.ctypes.data_as(FLOAT_PTR) if lg.size else None, R, lg.shape[1],
                                                                                        tk.ctypes.data_as(INT_PTR) if tk.size else None, len(st[0]) - 1, int(slot),
                                                                                        st[0].ctypes.data_as(INT_PTR), st[1].ctypes.data_as(INT_PTR), st[2].ctypes.data_as(INT_PTR),
                                                                                        keep.ctypes.data_as(FLOAT_PTR), res.ctypes.data_as(INT_PTR)))
        return dict(m=int(res[0]), res=res, n_past=st[0], argmax=st[1], feed=st[2], slot_logits=keep)

    def amd_test_step_words(self, form: int, row_slot, n_past, argmax, feed, row_pos=None, n: Optional[int] = None, with_tok0: bool = True) -> dict:
        """The bookkeeping launches on state words.  form 0: launch_advance by n on slot row_slot[0] (with_tok0: feed[slot] <- argmax[slot]); form 1: launch_batch_begin,
        n_past[row_slot[r]] = row_pos[r] for r < n (default: every row given); form 2: launch_draft_begin, n_past[row_slot[0]] = row_pos[0].  dict(n_past, argmax, feed)."""
        sl = np.ascontiguousarray(row_slot, np.int32).reshape(-1)
        ps = None if row_pos is None else np.ascontiguousarray(row_pos, np.int32).reshape(-1)
        if form == 1 and n is None:
            n = sl.size
        if ps is not None and ps.size != sl.size:
            raise ValueError("amd_test_step_words: one position per slot")
        if form == 1 and 1 <= n <= 64 and n > sl.size:
            raise ValueError("amd_test_step_words: n beyond the rows given")
        st, _ = self._step_state(n_past, argmax, feed)
        self._step_rc("test_step_words", self.library.minigpt4_amd_test_step_words(int(form), len(st[0]) - 1, int(n or 0), sl.ctypes.data_as(INT_PTR) if sl.size else None,
                                                                                    ps.ctypes.data_as(INT_PTR) if ps is not None and ps.size else None, int(bool(with_tok0)),
                                                                                    st[0].ctypes.data_as(INT_PTR), st[1].ctypes.data_as(INT_PTR), st[2].ctypes.data_as(INT_PTR)))
        return dict(n_past=st[0], argmax=st[1], feed=st[2])

    def amd_test_gather_rows(self, src: np.ndarray, idx: Sequence[int]) -> np.ndarray:
        """ONE launch_gather_rows: dst[r] = src[idx[r]] on src [n_src][E]; returns [n + 1][E] fp32 -- row n is the guard row and keeps its 0xFF fill."""
        s = np.ascontiguousarray(src, np.float32)
        if s.ndim != 2:
            raise ValueError("amd_test_gather_rows: src [n_src][E]")
        ix = np.ascontiguousarray(idx, np.int32).reshape(-1)
        out = np.zeros((ix.size + 1, s.shape[1]), np.float32)
        self._step_rc("test_gather_rows", self.library.minigpt4_amd_test_gather_rows(s.ctypes.data_as(FLOAT_PTR) if s.size else None, s.shape[0],
                                                                                      ix.ctypes.data_as(INT_PTR) if ix.size else None, ix.size, s.shape[1],
                                                                                      out.ctypes.data_as(FLOAT_PTR)))
        return out

    def amd_test_draft_tables(self, history: Sequence[int], x0: int, draft: Sequence[int], n_ctx: int, n_vocab: int, repeat_last_n: int = 64, repeat_penalty: float = 1.0,
                              alpha_presence: float = 0.0, alpha_frequency: float = 0.0, penalize_nl: int = 1, bias=None, trans=None, accept=None, state: int = 0,
                              pieces: Optional[Sequence[bytes]] = None) -> dict:
        """The host staging of a sampled verify pass alone (no GPU; csrc/draft_host.hpp): dict(n_rows, cut, rows [R][8] i32 PenRow words, tables: a list of R arrays
        [n][4] i32 (id, count, bias bits, has_bias), states [R]).  trans [S][256] u16 + accept bitmap + pieces (bytes per token id): the constraint; None: none."""
        h = np.ascontiguousarray(history, np.int32).reshape(-1)
        d = np.ascontiguousarray(draft, np.int32).reshape(-1)
        pairs = list(bias.items()) if isinstance(bias, dict) else list(bias or [])
        bi = np.ascontiguousarray([p[0] for p in pairs], np.int32)
        bv = np.ascontiguousarray([p[1] for p in pairs], np.float32)
        U8P, U16P, U32P = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint32)
        tr = ac = vb = of = None
        n_states = 0
        if trans is not None:
            tr = np.ascontiguousarray(trans, np.uint16).reshape(-1, 256)
            n_states = len(tr)
            ac = np.zeros((n_states + 31) // 32 + 1, np.uint32)
            a = np.ascontiguousarray(accept, np.uint32).reshape(-1)
            ac[:len(a)] = a
            assert pieces is not None and len(pieces) == int(n_vocab)
            of = np.zeros(int(n_vocab) + 1, np.int32)
            of[1:] = np.cumsum([len(p) for p in pieces])
            vb = np.frombuffer(b"".join(pieces) + b"\0", np.uint8).copy()
        cap = 8 * 1281
        n_rows, cut, n_tab = I32(0), I32(0), I32(0)
        rows, tab, states = np.zeros((8, 8), np.int32), np.zeros((cap, 4), np.int32), np.zeros(8, np.int32)
        rc = self.library.minigpt4_amd_test_draft_tables(h.ctypes.data_as(INT_PTR) if len(h) else None, len(h), int(x0), d.ctypes.data_as(INT_PTR) if len(d) else None, len(d),
                                                         int(repeat_last_n), float(repeat_penalty), float(alpha_presence), float(alpha_frequency), int(penalize_nl),
                                                         bi.ctypes.data_as(INT_PTR) if len(pairs) else None, bv.ctypes.data_as(FLOAT_PTR) if len(pairs) else None, len(pairs),
                                                         int(n_ctx), int(n_vocab), tr.ctypes.data_as(U16P) if tr is not None else None,
                                                         ac.ctypes.data_as(U32P) if ac is not None else None, n_states, int(state),
                                                         vb.ctypes.data_as(U8P) if vb is not None else None, of.ctypes.data_as(INT_PTR) if of is not None else None,
                                                         ctypes.byref(n_rows), ctypes.byref(cut), rows.ctypes.data_as(INT_PTR), tab.ctypes.data_as(INT_PTR), cap, ctypes.byref(n_tab),
                                                         states.ctypes.data_as(INT_PTR))
        if rc:
            raise RuntimeError(f"test_draft_tables rc={rc}")
        R = int(n_rows.value)
        rows = rows[:R].copy()
        return dict(n_rows=R, cut=int(cut.value), rows=rows, tables=[tab[rows[r, 1]:rows[r, 1] + rows[r, 2]].copy() for r in range(R)], states=states[:R].copy())

    # ---- beam search (include/minigpt4_amd.h)
    def amd_beam_search(self, ctx, slots: Sequence[int], max_tokens: int, length_penalty: float = 1.0, n_best: Optional[int] = None, with_stats: bool = False):
        """Beam search with len(slots) beams: slots[0] is the source conversation (left exactly as it was), the others are scratch.  Returns the hypotheses, best first, as a
        list of (ids i32 array, score); a finished hypothesis ends in id 2.  with_stats: (that list, dict(passes, permutes, rows_moved, finished)).  Continue the chat with
        amd_eval_tokens(ctx, best ids).  include/minigpt4_amd.h states the rule."""
        sl = np.ascontiguousarray(slots, np.int32)
        W = len(sl)
        nb = W if n_best is None else int(n_best)
        if W < 2 or W > 8:
            raise ValueError("beam_search: 2 .. 8 beams (slots)")
        if nb < 1 or nb > W:
            raise ValueError("beam_search: n_best outside 1 .. len(slots)")
        if int(max_tokens) < 1:
            raise ValueError("beam_search: max_tokens must be at least 1")
        if not np.isfinite(length_penalty):
            raise ValueError("beam_search: length_penalty must be finite")
        stride = int(max_tokens) + 1
        tok, ln, sc = np.full((nb, stride), -1, np.int32), np.zeros(nb, np.int32), np.zeros(nb, np.float32)
        n, st = np.zeros(1, np.int32), np.zeros(4, np.int32)
        if self.library.minigpt4_amd_beam_search(ctx.ptr if ctx is not None else None, sl.ctypes.data_as(INT_PTR), W, int(max_tokens), float(length_penalty), nb,
                                                 tok.ctypes.data_as(INT_PTR), ln.ctypes.data_as(INT_PTR), sc.ctypes.data_as(FLOAT_PTR), n.ctypes.data_as(INT_PTR),
                                                 st.ctypes.data_as(INT_PTR)):
            raise RuntimeError("beam_search failed: " + self._err())
        hyps = [(tok[i, :int(ln[i])].copy(), float(sc[i])) for i in range(int(n[0]))]
        if with_stats:
            return hyps, dict(passes=int(st[0]), permutes=int(st[1]), rows_moved=int(st[2]), finished=int(st[3]))
        return hyps

    # ---- guided decoding (include/minigpt4_amd.h)
    @staticmethod
    def _guided_args(name: str, slots: Sequence[int], neg_slots: Sequence[int], scale: float):
        """The two slot lists as int32 arrays; ValueError before the library is touched."""
        sl, ng = np.ascontiguousarray(slots, np.int32).reshape(-1), np.ascontiguousarray(neg_slots, np.int32).reshape(-1)
        if len(sl) != len(ng):
            raise ValueError(f"{name}: slots and neg_slots must have the same length")
        if len(sl) < 1 or len(sl) > 32:
            raise ValueError(f"{name}: 1 .. 32 pairs")
        both = np.concatenate([sl, ng])
        if len(np.unique(both)) != len(both):
            raise ValueError(f"{name}: a conversation may be named once, in one of the two lists")
        if both.min() < 0:
            raise ValueError(f"{name}: conversation index out of range")
        if not np.isfinite(ctypes.c_float(float(scale)).value):     # as the fp32 the library takes
            raise ValueError(f"{name}: scale must be finite")
        return sl, ng

    def amd_end_chat_guided(self, ctx, slots: Sequence[int], neg_slots: Sequence[int], scale: float, temp=0.8, top_k=40, top_p=0.9, tfs_z=1.0, typical_p=1.0, mirostat=0,
                            mirostat_tau=5.0, mirostat_eta=1.0, with_ids: bool = False):
        """One guided decode step: pair i decides ONE token from the logits of conversation slots[i] contrasted with those of neg_slots[i] (scale 1 = no guidance) and both
        advance by it in one pass over the weights.  Returns one piece per pair; with_ids: (pieces, ids i32 array).  include/minigpt4_amd.h states the rule."""
        sl, ng = self._guided_args("end_chat_guided", slots, neg_slots, scale)
        toks, ids = (ctypes.c_char_p * len(sl))(), np.zeros(len(sl), np.int32)
        rc = self.library.minigpt4_amd_end_chat_guided(ctx.ptr if ctx is not None else None, sl.ctypes.data_as(INT_PTR), ng.ctypes.data_as(INT_PTR), len(sl), float(scale), toks,
                                                       temp, top_k, top_p, tfs_z, typical_p, mirostat, mirostat_tau, mirostat_eta, ids.ctypes.data_as(INT_PTR))
        if rc:
            raise RuntimeError("end_chat_guided failed: " + self._err())
        pieces = [(t or b"").decode("utf-8", errors="replace") for t in toks]
        return (pieces, ids) if with_ids else pieces

    def amd_guided_logits(self, ctx, slots: Sequence[int], neg_slots: Sequence[int], scale: float, with_rows: bool = True) -> dict:
        """The guided rows of the listed pairs BEFORE bias and penalties, and their first maxima; nothing advances.  dict(mixed f32 [n][n_vocab] (None without with_rows),
        pick i32 [n])."""
        sl, ng = self._guided_args("guided_logits", slots, neg_slots, scale)
        n = len(sl)
        pick = np.zeros(n, np.int32)
        mixed = np.zeros((n, self.library.minigpt4_amd_n_vocab(ctx.ptr)), np.float32) if with_rows and ctx is not None else None
        rc = self.library.minigpt4_amd_guided_logits(ctx.ptr if ctx is not None else None, sl.ctypes.data_as(INT_PTR), ng.ctypes.data_as(INT_PTR), n, float(scale),
                                                     None if mixed is None else mixed.ctypes.data_as(FLOAT_PTR), pick.ctypes.data_as(INT_PTR))
        if rc:
            raise RuntimeError("guided_logits failed: " + self._err())
        return dict(mixed=mixed, pick=pick)

    def amd_guidance_info(self, ctx) -> dict:
        """dict(launches: k_guide_rows launches so far, handed: pairs whose token went to the pass on the device, pen_picked: pairs picked through k_pen_pick, sampled: pairs
        sampled on the host)."""
        o = np.zeros(4, np.int32)
        if self.library.minigpt4_amd_guidance_info(ctx.ptr if ctx is not None else None, o.ctypes.data_as(INT_PTR)):
            raise RuntimeError("guidance_info failed: " + self._err())
        return dict(launches=int(o[0]), handed=int(o[1]), pen_picked=int(o[2]), sampled=int(o[3]))

    def amd_test_guide_rows(self, logits: np.ndarray, pairs, scales: Sequence[float], n_vocab: Optional[int] = None, row_tok_index=None, row_tok: Optional[Sequence[int]] = None,
                            with_rows: bool = True) -> dict:
        """k_guide_rows, one launch, on logits [rows][ld] (include/minigpt4_amd_test.h): pairs [n][2] buffer rows (guided, guidance), scales [n], row_tok_index [n][2] indices
        into a 64-entry row-token array (-1 / None: none), row_tok its contents before the launch (default: all -7).  dict(mixed [n][n_vocab] or None, pick, value, row_tok
        [64], ms)."""
        lg = np.ascontiguousarray(logits, np.float32)
        if lg.ndim != 2:
            raise ValueError("test_guide_rows: logits must be [rows][ld]")
        nv = lg.shape[1] if n_vocab is None else int(n_vocab)
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = len(pr)
        sc = np.ascontiguousarray(scales, np.float32).reshape(-1)
        ti = np.full((n, 2), -1, np.int32) if row_tok_index is None else np.ascontiguousarray(row_tok_index, np.int32).reshape(-1, 2)
        if len(sc) != n or len(ti) != n:
            raise ValueError("test_guide_rows: pairs, scales and row_tok_index must name the same number of pairs")
        rt = np.full(64, -7, np.int32) if row_tok is None else np.ascontiguousarray(row_tok, np.int32).copy()
        if rt.shape != (64,):
            raise ValueError("test_guide_rows: row_tok must hold 64 entries")
        mixed = np.zeros((n, max(nv, 1)), np.float32) if with_rows else None
        pick, val, ms = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float32), ctypes.c_float(0)
        rc = self.library.minigpt4_amd_test_guide_rows(lg.ctypes.data_as(FLOAT_PTR), lg.shape[0], nv, lg.shape[1], pr.ctypes.data_as(INT_PTR), sc.ctypes.data_as(FLOAT_PTR),
                                                       ti.ctypes.data_as(INT_PTR), n, None if mixed is None else mixed.ctypes.data_as(FLOAT_PTR), pick.ctypes.data_as(INT_PTR),
                                                       val.ctypes.data_as(FLOAT_PTR), rt.ctypes.data_as(INT_PTR), ctypes.byref(ms))
        if rc:
            raise RuntimeError(f"test_guide_rows rc={rc}: " + self._err())
        return dict(mixed=mixed, pick=pick[:n], value=val[:n], row_tok=rt, ms=float(ms.value))

    def amd_test_beam_select_host(self, ids: np.ndarray, logprobs: np.ndarray, length_penalty: float = 1.0, n_best: Optional[int] = None, position: int = 0,
                                  scores0: Optional[Sequence[float]] = None, live0: int = 0, eos: int = 2) -> dict:
        """The search rule on the CPU over GIVEN candidates ids / logprobs [n_steps][W][2 W] (include/minigpt4_amd_test.h).  dict(steps [steps run][44] i32 words,
        hyps [(ids, score f32)], stats [4])."""
        ids = np.ascontiguousarray(ids, np.int32)
        lp = np.ascontiguousarray(logprobs, np.float32)
        T, W, C = ids.shape
        if lp.shape != ids.shape or C != 2 * W:
            raise ValueError("test_beam_select_host: ids / logprobs must both be [n_steps][W][2 W]")
        nb = W if n_best is None else int(n_best)
        steps = np.zeros((T, 44), np.int32)
        tok, ln, sc = np.full((max(nb, 1), T + 1), -1, np.int32), np.zeros(max(nb, 1), np.int32), np.zeros(max(nb, 1), np.float32)
        n, st = np.zeros(1, np.int32), np.zeros(4, np.int32)
        s0 = None if scores0 is None else np.ascontiguousarray(scores0, np.float32)
        rc = self.library.minigpt4_amd_test_beam_select_host(W, T, ids.ctypes.data_as(INT_PTR), lp.ctypes.data_as(FLOAT_PTR), None if s0 is None else s0.ctypes.data_as(FLOAT_PTR),
                                                             int(live0), int(eos), int(position), float(length_penalty), nb, steps.ctypes.data_as(INT_PTR),
                                                             tok.ctypes.data_as(INT_PTR), ln.ctypes.data_as(INT_PTR), sc.ctypes.data_as(FLOAT_PTR), n.ctypes.data_as(INT_PTR),
                                                             st.ctypes.data_as(INT_PTR))
        if rc:
            raise RuntimeError(f"test_beam_select_host rc={rc}")
        return dict(steps=steps[:int(st[0])].copy(), hyps=[(tok[i, :int(ln[i])].copy(), np.float32(sc[i])) for i in range(int(n[0]))], stats=st)

    def amd_test_beam_select(self, ids: np.ndarray, logprobs: np.ndarray, scores: Sequence[float], live: int, n_vocab: int, eos: int = 2) -> dict:
        """k_beam_select on one step's candidates ids / logprobs [W][2 W]: dict(step [44] i32 words, row_tok [W], scores [W] f32: the next step's)."""
        ids = np.ascontiguousarray(ids, np.int32)
        lp = np.ascontiguousarray(logprobs, np.float32)
        W = ids.shape[0]
        s = np.ascontiguousarray(scores, np.float32).copy()
        step, rt = np.zeros(44, np.int32), np.zeros(W, np.int32)
        rc = self.library.minigpt4_amd_test_beam_select(W, ids.ctypes.data_as(INT_PTR), lp.ctypes.data_as(FLOAT_PTR), s.ctypes.data_as(FLOAT_PTR), int(live), int(eos), int(n_vocab),
                                                        step.ctypes.data_as(INT_PTR), rt.ctypes.data_as(INT_PTR))
        if rc:
            raise RuntimeError(f"test_beam_select rc={rc}: " + self._err())
        return dict(step=step, row_tok=rt, scores=s)

    def amd_test_kv_permute(self, k: np.ndarray, v: np.ndarray, slots: Sequence[int], parent: Sequence[int], r0: int, r1: int):
        """k_kv_permute on fp16 caches k / v = [n_slot][n_layer][n_ctx][n_embd] (uint16 bit patterns): returns the caches after listed slot i took rows [r0, r1) of listed
        slot parent[i]."""
        k, v = np.ascontiguousarray(k, np.uint16).copy(), np.ascontiguousarray(v, np.uint16).copy()
        sl, pa = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(parent, np.int32)
        rc = self.library.minigpt4_amd_test_kv_permute(k.shape[0], k.shape[1], k.shape[2], k.shape[3], sl.ctypes.data_as(INT_PTR), len(sl), pa.ctypes.data_as(INT_PTR), int(r0),
                                                       int(r1), k.ctypes.data_as(VOID_PTR), v.ctypes.data_as(VOID_PTR), None)
        if rc:
            raise RuntimeError(f"test_kv_permute rc={rc}: " + self._err())
        return k, v

    def amd_test_kv_permute_ms(self, n_slot: int, n_layer: int, n_ctx: int, n_embd: int, slots: Sequence[int], parent: Sequence[int], r0: int, r1: int) -> float:
        """hipEvent time of one k_kv_permute launch on device caches of that shape."""
        sl, pa = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(parent, np.int32)
        ms = ctypes.c_float(0)
        rc = self.library.minigpt4_amd_test_kv_permute(n_slot, n_layer, n_ctx, n_embd, sl.ctypes.data_as(INT_PTR), len(sl), pa.ctypes.data_as(INT_PTR), int(r0), int(r1), None, None,
                                                       ctypes.byref(ms))
        if rc:
            raise RuntimeError(f"test_kv_permute rc={rc}: " + self._err())
        return float(ms.value)

    # ---- repetition / frequency / presence penalties, logit bias (include/minigpt4_amd.h)
    def _err(self) -> str:
        return (self.library.minigpt4_amd_last_error() or b"").decode("utf-8", errors="replace")

    def amd_set_penalties(self, ctx, on: bool) -> None:
        """Off (the default, the reference's behaviour): minigpt4_end_chat(_image) ignores its five penalty arguments.  On: it stores them as the selected
        conversation's parameters and samples with them; the batched calls and amd_sample use each conversation's stored parameters.  NEUTRAL values are
        repeat_penalty 1.0, alpha_presence 0.0, alpha_frequency 0.0 -- the wrappers' defaults for the alphas (the reference binding's) are 1.0."""
        if self.library.minigpt4_amd_set_penalties(ctx.ptr, int(bool(on))):
            raise RuntimeError("set_penalties failed: " + self._err())

    def amd_conversation_penalties(self, ctx, slot: int, repeat_last_n: int = 64, repeat_penalty: float = 1.0, alpha_presence: float = 0.0,
                                   alpha_frequency: float = 0.0, penalize_nl: int = 1) -> None:
        """A conversation's penalty parameters (the defaults are the neutral ones); they take effect only while amd_set_penalties is on."""
        if self.library.minigpt4_amd_conversation_penalties(ctx.ptr, int(slot), int(repeat_last_n), float(repeat_penalty), float(alpha_presence), float(alpha_frequency),
                                                            int(penalize_nl)):
            raise RuntimeError("conversation_penalties failed: " + self._err())

    def amd_set_logit_bias(self, ctx, bias) -> None:
        """The selected conversation's logit bias: a dict {id: bias} or a sequence of (id, bias) pairs, at most 256; empty / None clears it.  Active whatever the
        penalties mode; -inf bans a token."""
        pairs = list(bias.items()) if isinstance(bias, dict) else list(bias or [])
        ids = np.ascontiguousarray([p[0] for p in pairs], np.int32)
        val = np.ascontiguousarray([p[1] for p in pairs], np.float32)
        if self.library.minigpt4_amd_set_logit_bias(ctx.ptr, ids.ctypes.data_as(INT_PTR) if len(pairs) else None, val.ctypes.data_as(FLOAT_PTR) if len(pairs) else None,
                                                    len(pairs)):
            raise RuntimeError("set_logit_bias failed: " + self._err())

    # ---- snapshots (include/minigpt4_amd.h: the format and the rules)
    STATE_PEEK_FIELDS = ("version", "total_bytes", "n_layer", "n_embd", "n_head", "n_vocab", "arena_hash", "n_rows", "block_rows", "flags", "greedy", "feed")
    STATE_INFO_FIELDS = ("saves", "loads", "rows_saved", "rows_loaded", "pack_launches", "unpack_launches", "checksum_failures", "staging_bytes")

    def amd_state_size(self, ctx, slot: int) -> int:
        """The bytes amd_state_save(ctx, slot) would return now, queued rows counted."""
        n = int(self.library.minigpt4_amd_state_size(ctx.ptr, int(slot)))
        if n == 0:
            raise RuntimeError("state_size failed: " + self._err())
        return n

    def amd_state_save(self, ctx, slot: int, cap: Optional[int] = None) -> bytes:
        """Conversation `slot` as one checksummed blob (queued rows are evaluated first).  cap: the buffer size to offer (default: what amd_state_size says); too small
        raises with the size needed in the text and in the exception's `needed` attribute."""
        n = self.amd_state_size(ctx, slot) if cap is None else int(cap)
        buf = (ctypes.c_uint8 * max(n, 1))()
        written = ctypes.c_size_t()
        if self.library.minigpt4_amd_state_save(ctx.ptr, int(slot), buf, n, ctypes.byref(written)):
            e = RuntimeError("state_save failed: " + self._err())
            e.needed = int(written.value)
            raise e
        return bytes(memoryview(buf)[:written.value])

    def amd_state_load(self, ctx, slot: int, blob) -> None:
        """Restore conversation `slot` from a blob of amd_state_save (any slot of any context of the same language-model file)."""
        data = bytes(blob)
        if self.library.minigpt4_amd_state_load(ctx.ptr, int(slot), ctypes.c_char_p(data) if data else None, len(data)):
            raise RuntimeError("state_load failed: " + self._err())

    def amd_state_save_file(self, ctx, slot: int, path: str) -> None:
        if self.library.minigpt4_amd_state_save_file(ctx.ptr, int(slot), os.fsencode(path)):
            raise RuntimeError("state_save_file failed: " + self._err())

    def amd_state_load_file(self, ctx, slot: int, path: str) -> None:
        if self.library.minigpt4_amd_state_load_file(ctx.ptr, int(slot), os.fsencode(path)):
            raise RuntimeError("state_load_file failed: " + self._err())

    def amd_state_peek(self, blob) -> dict:
        """The header fields of a snapshot after every check that needs no context (no GPU either)."""
        data = bytes(blob)
        out = (ctypes.c_int64 * len(self.STATE_PEEK_FIELDS))()
        if self.library.minigpt4_amd_state_peek(ctypes.c_char_p(data) if data else None, len(data), out):
            raise RuntimeError("state_peek failed: " + self._err())
        d = dict(zip(self.STATE_PEEK_FIELDS, (int(x) for x in out)))
        d["arena_hash"] &= (1 << 64) - 1
        return d

    def amd_state_info(self, ctx) -> dict:
        out = (ctypes.c_int64 * len(self.STATE_INFO_FIELDS))()
        if self.library.minigpt4_amd_state_info(ctx.ptr, out):
            raise RuntimeError("state_info failed: " + self._err())
        return dict(zip(self.STATE_INFO_FIELDS, (int(x) for x in out)))

    def amd_token_history(self, ctx) -> np.ndarray:
        """The selected conversation's row-aligned token history (queued rows are evaluated first): the token id of every cache row, -1 for an embedding row."""
        n = self.library.minigpt4_amd_token_history(ctx.ptr, None, 0)
        if n < 0:
            raise RuntimeError("token_history failed: " + self._err())
        out = np.zeros(max(n, 1), np.int32)
        self.library.minigpt4_amd_token_history(ctx.ptr, out.ctypes.data_as(INT_PTR), n)
        return out[:n]

    def amd_penalty_info(self, ctx) -> dict:
        """dict(mode, launches: k_pen_pick launches so far, host_rows: rows penalised on the host so far, last_entries: table entries the last launch uploaded)."""
        o = np.zeros(4, np.int32)
        if self.library.minigpt4_amd_penalty_info(ctx.ptr, o.ctypes.data_as(INT_PTR)):
            raise RuntimeError("penalty_info failed: " + self._err())
        return dict(mode=int(o[0]), launches=int(o[1]), host_rows=int(o[2]), last_entries=int(o[3]))

    def amd_test_penalise_host(self, row: np.ndarray, history: Sequence[int], n_ctx: int, repeat_last_n: int = 64, repeat_penalty: float = 1.0,
                               alpha_presence: float = 0.0, alpha_frequency: float = 0.0, penalize_nl: int = 1, bias=None):
        """The host function on one row (no GPU): returns (row', table [n][4] i32 = id, count, bias bits, has_bias, flags)."""
        r = np.ascontiguousarray(row, np.float32).copy()
        h = np.ascontiguousarray(history, np.int32)
        pairs = list(bias.items()) if isinstance(bias, dict) else list(bias or [])
        ids = np.ascontiguousarray([p[0] for p in pairs], np.int32)
        val = np.ascontiguousarray([p[1] for p in pairs], np.float32)
        tab, fl = np.zeros((1281, 4), np.int32), np.zeros(1, np.int32)
        n = self.library.minigpt4_amd_test_penalise_host(r.ctypes.data_as(FLOAT_PTR), len(r), h.ctypes.data_as(INT_PTR) if len(h) else None, len(h), int(n_ctx),
                                                         int(repeat_last_n), float(repeat_penalty), float(alpha_presence), float(alpha_frequency), int(penalize_nl),
                                                         ids.ctypes.data_as(INT_PTR) if len(pairs) else None, val.ctypes.data_as(FLOAT_PTR) if len(pairs) else None,
                                                         len(pairs), tab.ctypes.data_as(INT_PTR), len(tab), fl.ctypes.data_as(INT_PTR))
        if n < 0:
            raise RuntimeError("test_penalise_host: bad arguments")
        return r, tab[:n].copy(), int(fl[0])

    def amd_test_pen_pick(self, logits: np.ndarray, n_vocab: int, rows: np.ndarray, table: np.ndarray):
        """launch_pen_pick on host logits [buf_rows][ld] (n_vocab <= ld columns are read).  rows [n][8] i32 words (buffer row, first entry, entries, flags, the bit
        patterns of repeat_penalty / alpha_frequency / alpha_presence, 0), table [m][4] i32 words: returns (picked [n] i32, adjusted [m] f32, ms)."""
        lg = np.ascontiguousarray(logits, np.float32)
        assert lg.ndim == 2
        rw = np.ascontiguousarray(rows, np.int32).reshape(-1, 8)
        tb = np.ascontiguousarray(table, np.int32).reshape(-1, 4)
        picked, adj, ms = np.zeros(len(rw), np.int32), np.zeros(max(len(tb), 1), np.float32), ctypes.c_float()
        rc = self.library.minigpt4_amd_test_pen_pick(lg.ctypes.data_as(FLOAT_PTR), lg.shape[0], int(n_vocab), lg.shape[1], rw.ctypes.data_as(INT_PTR), len(rw),
                                                     tb.ctypes.data_as(INT_PTR) if len(tb) else None, len(tb), picked.ctypes.data_as(INT_PTR), adj.ctypes.data_as(FLOAT_PTR),
                                                     ctypes.byref(ms))
        if rc:
            raise RuntimeError(f"test_pen_pick rc={rc}: " + self._err())
        return picked, adj[:len(tb)], float(ms.value)

    # ---- constrained decoding: a regular expression per conversation (include/minigpt4_amd.h)
    CONSTRAINT_INFO_FIELDS = ("handle", "state", "accepting", "n_states", "pick_launches", "host_rows", "stuck", "index_launches")

    @staticmethod
    def _pattern_bytes(pattern) -> bytes:
        return pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern)

    def amd_constraint_compile(self, ctx, pattern) -> int:
        """Compile a pattern (str: its UTF-8 bytes; or bytes) for this context: the DFA, its upload and the index of allowed tokens per state.  Returns the handle (1 .. 8).
        RuntimeError carries the compiler's refusal ("... at byte N", "too many states ...", "matches nothing")."""
        pat, h = self._pattern_bytes(pattern), I32(0)
        if self.library.minigpt4_amd_constraint_compile(ctx.ptr, pat, len(pat), ctypes.byref(h)):
            raise RuntimeError("constraint_compile failed: " + self._err())
        return int(h.value)

    def amd_constraint_free(self, ctx, handle: int) -> None:
        if self.library.minigpt4_amd_constraint_free(ctx.ptr, int(handle)):
            raise RuntimeError("constraint_free failed: " + self._err())

    def amd_set_constraint(self, ctx, slot: int, handle: int) -> None:
        """Conversation `slot` generates inside the compiled pattern `handle` from now on (0: no constraint); its state goes to the start."""
        if self.library.minigpt4_amd_set_constraint(ctx.ptr, int(slot), int(handle)):
            raise RuntimeError("set_constraint failed: " + self._err())

    def amd_constraint_advance(self, ctx, slot: int, tokens: Sequence[int]) -> None:
        """Walk the conversation's state over token ids the caller fed itself; a token that leaves the pattern refuses the whole call."""
        tk = np.ascontiguousarray(tokens, np.int32)
        if self.library.minigpt4_amd_constraint_advance(ctx.ptr, int(slot), tk.ctypes.data_as(INT_PTR) if len(tk) else None, len(tk)):
            raise RuntimeError("constraint_advance failed: " + self._err())

    def amd_constraint_info(self, ctx, slot: int = 0) -> dict:
        """dict(handle, state, accepting, n_states of the conversation's constraint; pick_launches: k_constrain_pick launches, host_rows: rows masked for the host chain,
        stuck: picks without an allowed id, index_launches: k_constrain_index launches -- of the context so far)."""
        o = np.zeros(8, np.int32)
        if self.library.minigpt4_amd_constraint_info(ctx.ptr, int(slot), o.ctypes.data_as(INT_PTR)):
            raise RuntimeError("constraint_info failed: " + self._err())
        return dict(zip(self.CONSTRAINT_INFO_FIELDS, (int(v) for v in o)))

    def amd_constraint_mask(self, ctx, handle: int, state: int, n_words: Optional[int] = None) -> np.ndarray:
        """The device index row of (handle, state): uint32 words, bit i of word i // 32 = token i is allowed."""
        nv = self.library.minigpt4_amd_n_vocab(ctx.ptr)
        w = ((nv + 31) // 32 + 3) // 4 * 4 if n_words is None else int(n_words)
        out = np.zeros(max(w, 1), np.uint32)
        if self.library.minigpt4_amd_constraint_mask(ctx.ptr, int(handle), int(state), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), w):
            raise RuntimeError("constraint_mask failed: " + self._err())
        return out[:w]

    def amd_test_constraint_compile(self, pattern):
        """The compiler alone, no GPU (include/minigpt4_amd_test.h): (trans [S][256] uint16, accept [(S + 31) // 32] uint32, S).  ValueError carries a refusal's text."""
        pat = self._pattern_bytes(pattern)
        trans, acc, n, err = np.zeros((1024, 256), np.uint16), np.zeros(32, np.uint32), I32(0), ctypes.create_string_buffer(256)
        rc = self.library.minigpt4_amd_test_constraint_compile(pat, len(pat), trans.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)),
                                                               acc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 1024, ctypes.byref(n), err, len(err))
        if rc == 1:
            raise ValueError(err.value.decode("utf-8", errors="replace"))
        if rc:
            raise RuntimeError(f"test_constraint_compile rc={rc}")
        S = int(n.value)
        return trans[:S].copy(), acc[:(S + 31) // 32].copy(), S

    def amd_test_constrain_index(self, pieces: Sequence[bytes], trans: np.ndarray, accept: np.ndarray):
        """k_constrain_index alone on a given vocabulary (a list of byte strings) and table: (index [S][W] uint32, ms)."""
        off = np.zeros(len(pieces) + 1, np.int32)
        off[1:] = np.cumsum([len(p) for p in pieces])
        blob = np.frombuffer(b"".join(bytes(p) for p in pieces) + b"\0", np.uint8).copy()
        tr = np.ascontiguousarray(trans, np.uint16)
        ac = np.ascontiguousarray(accept, np.uint32)
        S, V = len(tr), len(pieces)
        out, ms = np.zeros((S, ((V + 31) // 32 + 3) // 4 * 4), np.uint32), ctypes.c_float()
        U32P = ctypes.POINTER(ctypes.c_uint32)
        rc = self.library.minigpt4_amd_test_constrain_index(blob.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), off.ctypes.data_as(INT_PTR), V,
                                                            tr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), ac.ctypes.data_as(U32P), S, out.ctypes.data_as(U32P), ctypes.byref(ms))
        if rc:
            raise RuntimeError(f"test_constrain_index rc={rc}: " + self._err())
        return out, float(ms.value)

    def amd_test_constrain_pick(self, logits: np.ndarray, n_vocab: int, rows: np.ndarray, table: np.ndarray, bitmaps: np.ndarray, bitmap_of_row: Sequence[int]):
        """k_constrain_pick alone on host logits [buf_rows][ld]; rows / table as amd_test_pen_pick, bitmaps [k][W] uint32, bitmap_of_row [n]: returns (ids [n], stuck [n]
        bool, ms)."""
        lg = np.ascontiguousarray(logits, np.float32)
        assert lg.ndim == 2
        rw = np.ascontiguousarray(rows, np.int32).reshape(-1, 8)
        tb = np.ascontiguousarray(table, np.int32).reshape(-1, 4)
        bm = np.ascontiguousarray(bitmaps, np.uint32)
        assert bm.ndim == 2 and bm.shape[1] == ((int(n_vocab) + 31) // 32 + 3) // 4 * 4
        br = np.ascontiguousarray(bitmap_of_row, np.int32)
        assert len(br) == len(rw)
        out, ms = np.zeros(len(rw), np.int32), ctypes.c_float()
        rc = self.library.minigpt4_amd_test_constrain_pick(lg.ctypes.data_as(FLOAT_PTR), lg.shape[0], int(n_vocab), lg.shape[1], rw.ctypes.data_as(INT_PTR), len(rw),
                                                           tb.ctypes.data_as(INT_PTR) if len(tb) else None, len(tb), bm.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(bm),
                                                           br.ctypes.data_as(INT_PTR), out.ctypes.data_as(INT_PTR), ctypes.byref(ms))
        if rc:
            raise RuntimeError(f"test_constrain_pick rc={rc}: " + self._err())
        return out & ~(1 << 30), (out & (1 << 30)) != 0, float(ms.value)

    # ---- sampled batched steps decided on the device (include/minigpt4_amd.h)
    SAMPLE_MAX = 64

    @staticmethod
    def _sampled_args(name: str, slots: Sequence[int], temp, top_k, top_p) -> np.ndarray:
        """The slot list as an int32 array; ValueError before the library is touched."""
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        if len(sl) < 1 or len(sl) > 64:
            raise ValueError(f"{name}: 1 .. 64 conversations")
        if len(np.unique(sl)) != len(sl) or sl.min() < 0:
            raise ValueError(f"{name}: conversations must be distinct and in range")
        t, p = ctypes.c_float(float(temp)).value, ctypes.c_float(float(top_p)).value      # as the fp32 the library takes
        if not (np.isfinite(t) and t > 0):
            raise ValueError(f"{name}: temp must be finite and > 0")
        if int(top_k) != top_k or not 1 <= int(top_k) <= 64:
            raise ValueError(f"{name}: top_k outside 1 .. 64")
        if not (0 < p <= 1):
            raise ValueError(f"{name}: top_p outside (0, 1]")
        return sl

    @staticmethod
    def _chain_args(name: str, tfs_z, typical_p, min_p, mirostat, mirostat_tau, mirostat_eta) -> bool:
        """True when any parameter of the extended rule is not neutral (the call then goes to the _ex entry point); ValueError before the library is touched."""
        f = lambda x: ctypes.c_float(float(x)).value                                      # as the fp32 the library takes
        z, ty, mp, tau, eta = f(tfs_z), f(typical_p), f(min_p), f(mirostat_tau), f(mirostat_eta)
        if not (0 < z <= 1):
            raise ValueError(f"{name}: tfs_z outside (0, 1]")
        if not (0 < ty <= 1):
            raise ValueError(f"{name}: typical_p outside (0, 1]")
        if not (0 <= mp <= 1):
            raise ValueError(f"{name}: min_p outside [0, 1]")
        if int(mirostat) != mirostat or int(mirostat) not in (0, 1, 2):
            raise ValueError(f"{name}: mirostat must be 0 or 2")
        if int(mirostat) == 1:
            raise ValueError(f"{name}: mirostat v1 is not built")
        if not (np.isfinite(tau) and tau > 0):
            raise ValueError(f"{name}: mirostat_tau must be finite and > 0")
        if not (np.isfinite(eta) and eta >= 0):
            raise ValueError(f"{name}: mirostat_eta must be finite and >= 0")
        return z < 1 or ty < 1 or mp > 0 or int(mirostat) != 0

    def amd_end_chat_batch_sampled(self, ctx, slots: Sequence[int], temp=0.8, top_k=40, top_p=0.9, with_ids: bool = False, tfs_z=1.0, typical_p=1.0, min_p=0.0, mirostat=0,
                                   mirostat_tau=5.0, mirostat_eta=0.1, _extended: Optional[bool] = None):
        """One minigpt4_amd_end_chat_batch step whose tokens are sampled ON THE DEVICE, every conversation from its own (seed, draws) stream, and handed to the weight pass
        without a host visit.  Returns one piece per conversation; with_ids: (pieces, ids i32 array).  include/minigpt4_amd.h states the rule.  A non-neutral tfs_z,
        typical_p, min_p or mirostat sends the call to minigpt4_amd_end_chat_batch_sampled_ex, the extended rule; mirostat's mu is the conversation's.  _extended (a test and
        measurement aid): True sends neutral values there too."""
        sl = self._sampled_args("end_chat_batch_sampled", slots, temp, top_k, top_p)
        ex = self._chain_args("end_chat_batch_sampled", tfs_z, typical_p, min_p, mirostat, mirostat_tau, mirostat_eta)
        toks, ids = (ctypes.c_char_p * len(sl))(), np.zeros(len(sl), np.int32)
        cp = ctx.ptr if ctx is not None else None
        if ex if _extended is None else _extended:
            rc = self.library.minigpt4_amd_end_chat_batch_sampled_ex(cp, sl.ctypes.data_as(INT_PTR), len(sl), toks, float(temp), int(top_k), float(top_p), float(tfs_z),
                                                                     float(typical_p), float(min_p), int(mirostat), float(mirostat_tau), float(mirostat_eta),
                                                                     ids.ctypes.data_as(INT_PTR))
        else:
            rc = self.library.minigpt4_amd_end_chat_batch_sampled(cp, sl.ctypes.data_as(INT_PTR), len(sl), toks, float(temp), int(top_k), float(top_p), ids.ctypes.data_as(INT_PTR))
        if rc:
            raise RuntimeError("end_chat_batch_sampled failed: " + self._err())
        pieces = [(t or b"").decode("utf-8", errors="replace") for t in toks]
        return (pieces, ids) if with_ids else pieces

    def amd_sampled_candidates(self, ctx, slots: Sequence[int], temp=0.8, top_k=40, top_p=0.9, tfs_z=1.0, typical_p=1.0, min_p=0.0, mirostat=0, mirostat_tau=5.0,
                               mirostat_eta=0.1, _extended: Optional[bool] = None) -> dict:
        """The distribution the next sampled step would draw from; nothing advances, no draw is counted.  dict(ids i32 [n][64] (-1 behind n_cand), probs f32 [n][64] (0 behind
        kept), n_cand i32 [n], kept i32 [n]).  A non-neutral tfs_z, typical_p, min_p or mirostat (_extended=True, a test aid: neutral values too): minigpt4_amd_sampled_candidates_ex, probs 0 for a
        candidate outside the live list, and kept_mask uint64 [n] (bit j: candidate j is in it; kept = its population count); mu does not move."""
        sl = self._sampled_args("sampled_candidates", slots, temp, top_k, top_p)
        ex = self._chain_args("sampled_candidates", tfs_z, typical_p, min_p, mirostat, mirostat_tau, mirostat_eta)
        n = len(sl)
        ids, probs, nc, kept = np.zeros((n, 64), np.int32), np.zeros((n, 64), np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        cp = ctx.ptr if ctx is not None else None
        if ex if _extended is None else _extended:
            mask = np.zeros(n, np.uint64)
            rc = self.library.minigpt4_amd_sampled_candidates_ex(cp, sl.ctypes.data_as(INT_PTR), n, float(temp), int(top_k), float(top_p), float(tfs_z), float(typical_p),
                                                                 float(min_p), int(mirostat), float(mirostat_tau), float(mirostat_eta), ids.ctypes.data_as(INT_PTR),
                                                                 probs.ctypes.data_as(FLOAT_PTR), nc.ctypes.data_as(INT_PTR), mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
            if rc:
                raise RuntimeError("sampled_candidates failed: " + self._err())
            kept = np.array([bin(int(m)).count("1") for m in mask], np.int32)
            return dict(ids=ids, probs=probs, n_cand=nc, kept=kept, kept_mask=mask)
        rc = self.library.minigpt4_amd_sampled_candidates(cp, sl.ctypes.data_as(INT_PTR), n, float(temp), int(top_k), float(top_p),
                                                          ids.ctypes.data_as(INT_PTR), probs.ctypes.data_as(FLOAT_PTR), nc.ctypes.data_as(INT_PTR), kept.ctypes.data_as(INT_PTR))
        if rc:
            raise RuntimeError("sampled_candidates failed: " + self._err())
        return dict(ids=ids, probs=probs, n_cand=nc, kept=kept)

    def amd_conversation_mirostat(self, ctx, slot: int, mu: Optional[float]) -> None:
        """Set a conversation's mirostat mu (a finite value), or unset it (None / NaN): the next mirostat decision then starts from 2 * tau."""
        m = float("nan") if mu is None else ctypes.c_float(float(mu)).value
        if np.isinf(m):
            raise ValueError("conversation_mirostat: mu must be finite (None unsets it)")
        if self.library.minigpt4_amd_conversation_mirostat(ctx.ptr if ctx is not None else None, int(slot), m):
            raise RuntimeError("conversation_mirostat failed: " + self._err())

    def amd_mirostat_info(self, ctx, slot: int = 0) -> dict:
        """dict(set: bool, mu: f32 (None when unset), observed: the last observed surprise, tau: the tau it was measured against) of one conversation."""
        o = np.zeros(4, np.float32)
        if self.library.minigpt4_amd_mirostat_info(ctx.ptr if ctx is not None else None, int(slot), o.ctypes.data_as(FLOAT_PTR)):
            raise RuntimeError("mirostat_info failed: " + self._err())
        return dict(set=bool(o[0]), mu=o[1] if o[0] else None, observed=o[2], tau=o[3])

    def amd_conversation_seed(self, ctx, slot: int, seed: int, draws: int = 0) -> None:
        """Set a conversation's 64-bit seed and its count of draws (the next draw's Philox counter)."""
        if not (0 <= int(seed) < 1 << 64 and 0 <= int(draws) < 1 << 64):
            raise ValueError("conversation_seed: seed and draws are unsigned 64-bit integers")
        if self.library.minigpt4_amd_conversation_seed(ctx.ptr if ctx is not None else None, int(slot), int(seed), int(draws)):
            raise RuntimeError("conversation_seed failed: " + self._err())

    def amd_sampling_info(self, ctx, slot: int = 0) -> dict:
        """dict(seed, draws of the conversation; launches: k_sample_rows launches, handed: picks handed to a pass on the device, stuck: picks without a participating id,
        rows: rows sampled on the device -- of the context so far)."""
        o = np.zeros(6, np.uint64)
        if self.library.minigpt4_amd_sampling_info(ctx.ptr if ctx is not None else None, int(slot), o.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))):
            raise RuntimeError("sampling_info failed: " + self._err())
        return dict(zip(("seed", "draws", "launches", "handed", "stuck", "rows"), (int(v) for v in o)))

    def amd_test_philox(self, counter: Sequence[int], key: Sequence[int]) -> np.ndarray:
        """Philox4x32-10 of counter[4] under key[2] (host hook, no GPU): uint32 [4]."""
        c, k, o = np.ascontiguousarray(counter, np.uint32), np.ascontiguousarray(key, np.uint32), np.zeros(4, np.uint32)
        if c.shape != (4,) or k.shape != (2,):
            raise ValueError("test_philox: counter[4], key[2]")
        U32P = ctypes.POINTER(ctypes.c_uint32)
        if self.library.minigpt4_amd_test_philox(c.ctypes.data_as(U32P), k.ctypes.data_as(U32P), o.ctypes.data_as(U32P)):
            raise RuntimeError("test_philox failed")
        return o

    def amd_test_sample_rule(self, values, temp: float, top_p: float, word: int) -> dict:
        """The rule's steps 1 to 4 on the candidate values (in order) with the given Philox word (host hook, no GPU): dict(pick index, kept, p f32 [n])."""
        v = np.ascontiguousarray(values, np.float32).reshape(-1)
        p, kept = np.zeros(max(len(v), 1), np.float32), I32(0)
        pick = self.library.minigpt4_amd_test_sample_rule(v.ctypes.data_as(FLOAT_PTR), len(v), float(temp), float(top_p), int(word) & 0xFFFFFFFF, p.ctypes.data_as(FLOAT_PTR),
                                                          ctypes.byref(kept))
        if pick < 0:
            raise ValueError("test_sample_rule: bad arguments")
        return dict(pick=int(pick), kept=int(kept.value), p=p[:len(v)])

    def amd_test_sample_rows(self, logits: np.ndarray, n_vocab: int, rows: np.ndarray, table: np.ndarray, params, top_k, seed_draws, bitmaps=None, bitmap_of_row=None,
                             tok_index=None, row_tok: Optional[Sequence[int]] = None) -> dict:
        """k_sample_rows alone on host logits [buf_rows][ld] (include/minigpt4_amd_test.h): rows / table as amd_test_pen_pick, params [n][2] (temp, top_p), top_k [n],
        seed_draws [n][2] uint64, bitmaps [k][W] uint32 + bitmap_of_row [n] (-1 / None: no constraint), tok_index [n] into a 64-entry row-token array (-1 / None: none),
        row_tok its contents before the launch (default: all -7).  dict(pick, stuck, word, n_cand, kept [n]; ids [n][64]; p [n][64]; row_tok [64]; ms)."""
        lg = np.ascontiguousarray(logits, np.float32)
        assert lg.ndim == 2
        rw = np.ascontiguousarray(rows, np.int32).reshape(-1, 8)
        n = len(rw)
        tb = np.ascontiguousarray(table, np.int32).reshape(-1, 4)
        pr = np.ascontiguousarray(params, np.float32).reshape(-1, 2)
        tk = np.ascontiguousarray(top_k, np.int32).reshape(-1)
        sd = np.ascontiguousarray(seed_draws, np.uint64).reshape(-1, 2)
        W = ((int(n_vocab) + 31) // 32 + 3) // 4 * 4
        bm = np.zeros((0, W), np.uint32) if bitmaps is None else np.ascontiguousarray(bitmaps, np.uint32)
        assert bm.ndim == 2 and bm.shape[1] == W
        br = np.full(n, -1, np.int32) if bitmap_of_row is None else np.ascontiguousarray(bitmap_of_row, np.int32).reshape(-1)
        ti = np.full(n, -1, np.int32) if tok_index is None else np.ascontiguousarray(tok_index, np.int32).reshape(-1)
        assert len(pr) == n and len(tk) == n and len(sd) == n and len(br) == n and len(ti) == n
        rt = np.full(64, -7, np.int32) if row_tok is None else np.ascontiguousarray(row_tok, np.int32).copy()
        assert rt.shape == (64,)
        out, ms = np.zeros((max(n, 1), 5 + 128), np.int32), ctypes.c_float()
        U32P = ctypes.POINTER(ctypes.c_uint32)
        rc = self.library.minigpt4_amd_test_sample_rows(lg.ctypes.data_as(FLOAT_PTR), lg.shape[0], int(n_vocab), lg.shape[1], rw.ctypes.data_as(INT_PTR), n,
                                                        tb.ctypes.data_as(INT_PTR) if len(tb) else None, len(tb), bm.ctypes.data_as(U32P) if len(bm) else None, len(bm),
                                                        br.ctypes.data_as(INT_PTR), pr.ctypes.data_as(FLOAT_PTR), tk.ctypes.data_as(INT_PTR),
                                                        sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ti.ctypes.data_as(INT_PTR), rt.ctypes.data_as(INT_PTR),
                                                        out.ctypes.data_as(INT_PTR), ctypes.byref(ms))
        if rc:
            raise RuntimeError(f"test_sample_rows rc={rc}: " + self._err())
        out = out[:n]
        return dict(pick=out[:, 0].copy(), stuck=out[:, 1].copy(), word=out[:, 2].copy().view(np.uint32), n_cand=out[:, 3].copy(), kept=out[:, 4].copy(),
                    ids=out[:, 5:69].copy(), p=np.ascontiguousarray(out[:, 69:133]).view(np.float32), row_tok=rt, ms=float(ms.value))

    def amd_test_sample_chain(self, values, temp: float, top_p: float, word: int, tfs_z=1.0, typical_p=1.0, min_p=0.0, mirostat=0, mirostat_tau=5.0, mirostat_eta=0.1,
                              mu=None) -> dict:
        """The extended rule's host side on the candidate values (in order) with the given Philox word (host hook, no GPU); mu None: unset.  dict(pick index, kept = the
        live list's length, p f32 [n], mask: bit j = candidate j is in the live list, mu: mu' (mirostat 0: as given), observed)."""
        v = np.ascontiguousarray(values, np.float32).reshape(-1)
        p, kept, mask, mu_o, obs = np.zeros(max(len(v), 1), np.float32), I32(0), ctypes.c_uint64(0), ctypes.c_float(), ctypes.c_float()
        pick = self.library.minigpt4_amd_test_sample_chain(v.ctypes.data_as(FLOAT_PTR), len(v), float(temp), float(top_p), float(tfs_z), float(typical_p), float(min_p), int(mirostat),
                                                           float(mirostat_tau), float(mirostat_eta), float("nan") if mu is None else float(mu), int(word) & 0xFFFFFFFF,
                                                           p.ctypes.data_as(FLOAT_PTR), ctypes.byref(kept), ctypes.byref(mask), ctypes.byref(mu_o), ctypes.byref(obs))
        if pick < 0:
            raise ValueError("test_sample_chain: bad arguments")
        return dict(pick=int(pick), kept=int(kept.value), p=p[:len(v)], mask=int(mask.value), mu=np.float32(mu_o.value), observed=np.float32(obs.value))

    def amd_test_sample_rows_ex(self, logits: np.ndarray, n_vocab: int, rows: np.ndarray, table: np.ndarray, params, top_k, seed_draws, chain, bitmaps=None, bitmap_of_row=None,
                                tok_index=None, row_tok: Optional[Sequence[int]] = None) -> dict:
        """k_sample_rows_ex alone on host logits [buf_rows][ld] (include/minigpt4_amd_test.h): the arguments of amd_test_sample_rows and chain [n][7] = (tfs_z, typical_p,
        min_p, mirostat, tau, eta, mu; mu NaN: unset).  The dict of amd_test_sample_rows (kept = the live list's length) and mask uint64 [n], mu f32 [n], observed f32 [n]."""
        lg = np.ascontiguousarray(logits, np.float32)
        assert lg.ndim == 2
        rw = np.ascontiguousarray(rows, np.int32).reshape(-1, 8)
        n = len(rw)
        tb = np.ascontiguousarray(table, np.int32).reshape(-1, 4)
        pr = np.ascontiguousarray(params, np.float32).reshape(-1, 2)
        tk = np.ascontiguousarray(top_k, np.int32).reshape(-1)
        sd = np.ascontiguousarray(seed_draws, np.uint64).reshape(-1, 2)
        ch = np.asarray(chain, np.float64).reshape(-1, 7)
        cf, mi = np.ascontiguousarray(ch[:, [0, 1, 2, 4, 5, 6]], np.float32), np.ascontiguousarray(ch[:, 3], np.int32)
        W = ((int(n_vocab) + 31) // 32 + 3) // 4 * 4
        bm = np.zeros((0, W), np.uint32) if bitmaps is None else np.ascontiguousarray(bitmaps, np.uint32)
        assert bm.ndim == 2 and bm.shape[1] == W
        br = np.full(n, -1, np.int32) if bitmap_of_row is None else np.ascontiguousarray(bitmap_of_row, np.int32).reshape(-1)
        ti = np.full(n, -1, np.int32) if tok_index is None else np.ascontiguousarray(tok_index, np.int32).reshape(-1)
        assert len(pr) == n and len(tk) == n and len(sd) == n and len(br) == n and len(ti) == n and len(cf) == n
        rt = np.full(64, -7, np.int32) if row_tok is None else np.ascontiguousarray(row_tok, np.int32).copy()
        assert rt.shape == (64,)
        out, ms = np.zeros((max(n, 1), 9 + 128), np.int32), ctypes.c_float()
        U32P = ctypes.POINTER(ctypes.c_uint32)
        rc = self.library.minigpt4_amd_test_sample_rows_ex(lg.ctypes.data_as(FLOAT_PTR), lg.shape[0], int(n_vocab), lg.shape[1], rw.ctypes.data_as(INT_PTR), n,
                                                           tb.ctypes.data_as(INT_PTR) if len(tb) else None, len(tb), bm.ctypes.data_as(U32P) if len(bm) else None, len(bm),
                                                           br.ctypes.data_as(INT_PTR), pr.ctypes.data_as(FLOAT_PTR), tk.ctypes.data_as(INT_PTR),
                                                           sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ti.ctypes.data_as(INT_PTR), cf.ctypes.data_as(FLOAT_PTR),
                                                           mi.ctypes.data_as(INT_PTR), rt.ctypes.data_as(INT_PTR), out.ctypes.data_as(INT_PTR), ctypes.byref(ms))
        if rc:
            raise RuntimeError(f"test_sample_rows_ex rc={rc}: " + self._err())
        out = out[:n]
        mask = out[:, 133].copy().view(np.uint32).astype(np.uint64) | out[:, 134].copy().view(np.uint32).astype(np.uint64) << np.uint64(32)
        return dict(pick=out[:, 0].copy(), stuck=out[:, 1].copy(), word=out[:, 2].copy().view(np.uint32), n_cand=out[:, 3].copy(), kept=out[:, 4].copy(),
                    ids=out[:, 5:69].copy(), p=np.ascontiguousarray(out[:, 69:133]).view(np.float32), mask=mask, mu=out[:, 135].copy().view(np.float32),
                    observed=out[:, 136].copy().view(np.float32), row_tok=rt, ms=float(ms.value))

    def amd_token_piece(self, ctx, token_id: int) -> Optional[str]:
        """The text of one token id, as minigpt4_end_chat returns it ("</s>" for id 2); None for an id outside the vocabulary."""
        p = self.library.minigpt4_amd_token_piece(ctx.ptr, int(token_id))
        return None if p is None else p.decode("utf-8", errors="replace")

    def amd_top_logprobs(self, ctx, slots: Sequence[int], top_n: int = 5, targets: Optional[Sequence[int]] = None) -> dict:
        """What each listed (distinct) conversation would say next, without advancing anything: queued rows are evaluated first (as amd_prefill_batch does), then
        dict(top_ids [n][top_n] i32, top_logprobs [n][top_n] f32, logprob [n] f32, rank [n] i32) -- the last two describe targets[i] (None / -1: logprob 0, rank -1).
        A conversation without current logits gets ids -1, log-probabilities 0, rank -1.  include/minigpt4_amd.h"""
        sl = np.ascontiguousarray(slots, np.int32)
        n, k = len(sl), max(int(top_n), 1)
        tg = None if targets is None else np.ascontiguousarray(targets, np.int32)
        if tg is not None and tg.shape != (n,):
            raise RuntimeError("top_logprobs failed: top_logprobs: one target per slot is required")
        ti, tl, lp, rk = np.zeros((max(n, 1), k), np.int32), np.zeros((max(n, 1), k), np.float32), np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.int32)
        if self.library.minigpt4_amd_top_logprobs(ctx.ptr, sl.ctypes.data_as(INT_PTR), n, int(top_n), None if tg is None else tg.ctypes.data_as(INT_PTR),
                                                  ti.ctypes.data_as(INT_PTR), tl.ctypes.data_as(FLOAT_PTR), lp.ctypes.data_as(FLOAT_PTR), rk.ctypes.data_as(INT_PTR)):
            raise RuntimeError("top_logprobs failed: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return dict(top_ids=ti[:n], top_logprobs=tl[:n], logprob=lp[:n], rank=rk[:n])

    def amd_end_chat_batch_top(self, ctx, slots: Sequence[int], top_n: int = 5, temp=0.8, top_k=40, top_p=0.9, tfs_z=1.0, typical_p=1.0, mirostat=0, mirostat_tau=5.0,
                               mirostat_eta=1.0) -> dict:
        """amd_end_chat_batch that also reports what it drew from: dict(pieces [n] str, ids [n] i32, logprob [n] f32, rank [n] i32, top_ids [n][top_n] i32,
        top_logprobs [n][top_n] f32).  Log-probabilities are those of the raw logits, whatever the sampling parameters.  include/minigpt4_amd.h"""
        sl = np.ascontiguousarray(slots, np.int32)
        n, k = len(sl), max(int(top_n), 1)
        toks = (ctypes.c_char_p * max(n, 1))()
        ids, lp, rk = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.int32)
        ti, tl = np.zeros((max(n, 1), k), np.int32), np.zeros((max(n, 1), k), np.float32)
        if self.library.minigpt4_amd_end_chat_batch_top(ctx.ptr, sl.ctypes.data_as(INT_PTR), n, toks, temp, top_k, top_p, tfs_z, typical_p, mirostat, mirostat_tau, mirostat_eta,
                                                        int(top_n), ids.ctypes.data_as(INT_PTR), lp.ctypes.data_as(FLOAT_PTR), rk.ctypes.data_as(INT_PTR),
                                                        ti.ctypes.data_as(INT_PTR), tl.ctypes.data_as(FLOAT_PTR)):
            raise RuntimeError("end_chat_batch_top failed: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return dict(pieces=[(t or b"").decode("utf-8", errors="replace") for t in toks[:n]], ids=ids[:n], logprob=lp[:n], rank=rk[:n], top_ids=ti[:n], top_logprobs=tl[:n])

    def amd_score_batch(self, ctx, slots: Sequence[int], token_lists: Sequence[Sequence[int]]) -> List[dict]:
        """amd_score_tokens for several distinct conversations in packed passes (as amd_prefill_batch evaluates them): one dict(logprob, greedy, greedy_logprob) per
        conversation, in slot-list order.  include/minigpt4_amd.h"""
        sl = np.ascontiguousarray(slots, np.int32)
        lists = [np.ascontiguousarray(t, np.int32).reshape(-1) for t in token_lists]
        cnt = np.ascontiguousarray([len(t) for t in lists], np.int32)
        tk = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0), np.int32)
        n = max(int(tk.size), 1)
        lp, gr, glp = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        if len(lists) != len(sl):
            raise RuntimeError("score_batch failed: score_batch: one token list per slot is required")
        if self.library.minigpt4_amd_score_batch(ctx.ptr, sl.ctypes.data_as(INT_PTR), len(sl), tk.ctypes.data_as(INT_PTR), cnt.ctypes.data_as(INT_PTR),
                                                 lp.ctypes.data_as(FLOAT_PTR), gr.ctypes.data_as(INT_PTR), glp.ctypes.data_as(FLOAT_PTR)):
            raise RuntimeError("score_batch failed: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        ends = np.cumsum(cnt)
        return [dict(logprob=lp[e - c:e].copy(), greedy=gr[e - c:e].copy(), greedy_logprob=glp[e - c:e].copy()) for e, c in zip(ends, cnt)]

    def amd_test_logprob_rows(self, logits: np.ndarray, targets: Sequence[int], n_vocab: Optional[int] = None):
        """launch_logprob_rows on host logits [rows][ld] (n_vocab <= ld columns are read): returns (logprob, greedy, greedy_logprob, ms) -- per row the log-softmax of
        targets[r] (-1: none), the first argmax, its log-softmax, and the launch's hipEvent time."""
        lg = np.ascontiguousarray(logits, np.float32)
        assert lg.ndim == 2
        rows, ld = lg.shape
        nv = ld if n_vocab is None else int(n_vocab)
        tg = np.ascontiguousarray(targets, np.int32)
        assert tg.shape == (rows,)
        lp, gr, glp, ms = np.zeros(rows, np.float32), np.zeros(rows, np.int32), np.zeros(rows, np.float32), ctypes.c_float()
        rc = self.library.minigpt4_amd_test_logprob_rows(lg.ctypes.data_as(FLOAT_PTR), rows, nv, ld, tg.ctypes.data_as(INT_PTR), lp.ctypes.data_as(FLOAT_PTR),
                                                         gr.ctypes.data_as(INT_PTR), glp.ctypes.data_as(FLOAT_PTR), ctypes.byref(ms))
        if rc:
            raise RuntimeError(f"test_logprob_rows rc={rc}: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return lp, gr, glp, float(ms.value)

    def amd_test_topn_rows(self, logits: np.ndarray, top_n: int, targets: Sequence[int], n_vocab: Optional[int] = None, row_index: Optional[Sequence[int]] = None):
        """launch_topn_rows on host logits [buf_rows][ld] (n_vocab <= ld columns are read; row r = buffer row row_index[r], or r): returns (ids [rows][top_n],
        logprobs [rows][top_n], rank [rows], target_logprob [rows], ms) -- logit descending, equal logits by ascending id; rank / target_logprob describe targets[r]
        (-1: none)."""
        lg = np.ascontiguousarray(logits, np.float32)
        assert lg.ndim == 2
        buf_rows, ld = lg.shape
        nv = ld if n_vocab is None else int(n_vocab)
        tg = np.ascontiguousarray(targets, np.int32)
        ri = None if row_index is None else np.ascontiguousarray(row_index, np.int32)
        rows = int(tg.shape[0])
        assert tg.ndim == 1 and (ri is None or ri.shape == (rows,))
        k = max(int(top_n), 1)
        ids, lps = np.zeros((max(rows, 1), k), np.int32), np.zeros((max(rows, 1), k), np.float32)
        rk, tlp, ms = np.zeros(max(rows, 1), np.int32), np.zeros(max(rows, 1), np.float32), ctypes.c_float()
        rc = self.library.minigpt4_amd_test_topn_rows(lg.ctypes.data_as(FLOAT_PTR), buf_rows, nv, ld, None if ri is None else ri.ctypes.data_as(INT_PTR), rows, int(top_n),
                                                      tg.ctypes.data_as(INT_PTR), ids.ctypes.data_as(INT_PTR), lps.ctypes.data_as(FLOAT_PTR), rk.ctypes.data_as(INT_PTR),
                                                      tlp.ctypes.data_as(FLOAT_PTR), ctypes.byref(ms))
        if rc:
            raise RuntimeError(f"test_topn_rows rc={rc}: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return ids[:rows], lps[:rows], rk[:rows], tlp[:rows], float(ms.value)

    def amd_test_kv_copy(self, k: np.ndarray, v: np.ndarray, src: int, dsts: Sequence[int], n_rows: int, src_rows: int = 0):
        """launch_kv_copy on fp16 caches [n_slot][n_layer][rows][n_embd]: rows [0, n_rows) of slot `src` (src_rows > 0: of a compact [n_layer][src_rows][n_embd] copy of its
        first rows) to the slots `dsts`; returns (k, v, ms) -- changed copies and the launch's hipEvent time."""
        k = np.ascontiguousarray(k, np.float16).copy()
        v = np.ascontiguousarray(v, np.float16).copy()
        assert k.ndim == 4 and k.shape == v.shape
        d = np.ascontiguousarray(dsts, np.int32)
        ms = ctypes.c_float()
        rc = self.library.minigpt4_amd_test_kv_copy(k.shape[0], k.shape[1], k.shape[2], k.shape[3], int(src), d.ctypes.data_as(INT_PTR), len(d), int(n_rows), int(src_rows),
                                                    k.ctypes.data_as(VOID_PTR), v.ctypes.data_as(VOID_PTR), ctypes.byref(ms))
        if rc:
            raise RuntimeError(f"test_kv_copy rc={rc}: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return k, v, float(ms.value)

    def amd_test_kv_pack(self, k: np.ndarray, v: np.ndarray, r0: int, n: int):
        """launch_kv_pack alone on uint16 caches [n_layer][n_ctx][n_embd] of one conversation: (block [2][n_layer][n][n_embd] uint16, checksum, ms)."""
        k = np.ascontiguousarray(k, np.uint16)
        v = np.ascontiguousarray(v, np.uint16)
        assert k.ndim == 3 and k.shape == v.shape
        blk = np.zeros((2, k.shape[0], max(int(n), 0), k.shape[2]), np.uint16)
        s, ms = ctypes.c_uint64(), ctypes.c_float()
        rc = self.library.minigpt4_amd_test_kv_pack(k.shape[0], k.shape[1], k.shape[2], int(r0), int(n), k.ctypes.data_as(VOID_PTR), v.ctypes.data_as(VOID_PTR),
                                                    blk.ctypes.data_as(VOID_PTR), ctypes.byref(s), ctypes.byref(ms))
        if rc:
            raise RuntimeError(f"test_kv_pack rc={rc}: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return blk, int(s.value), float(ms.value)

    def amd_test_checksum(self, device_ptr: int, n_bytes: int):
        """k_checksum over a device-accessible range (an address, e.g. of a hipMalloc / hipHostMalloc block): (sum of its 32-bit words mod 2^64, hipEvent ms)."""
        s, ms = ctypes.c_uint64(), ctypes.c_float()
        rc = self.library.minigpt4_amd_test_checksum(ctypes.c_void_p(device_ptr), int(n_bytes), ctypes.byref(s), ctypes.byref(ms))
        if rc:
            raise RuntimeError(f"test_checksum rc={rc}: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return int(s.value), float(ms.value)

    def amd_test_kv_block_ms(self, n_layer: int, n_ctx: int, n_embd: int, r0: int, n: int, unpack: bool = False) -> float:
        """launch_kv_pack (unpack: launch_kv_unpack) on device-only buffers of the given shape (nothing crosses the host): its hipEvent time in ms."""
        s, ms = ctypes.c_uint64(), ctypes.c_float()
        fn = self.library.minigpt4_amd_test_kv_unpack if unpack else self.library.minigpt4_amd_test_kv_pack
        rc = fn(int(n_layer), int(n_ctx), int(n_embd), int(r0), int(n), None, None, None, ctypes.byref(s), ctypes.byref(ms))
        if rc:
            raise RuntimeError(f"test_kv_block rc={rc}: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return float(ms.value)

    def amd_test_kv_unpack(self, block: np.ndarray, k: np.ndarray, v: np.ndarray, r0: int):
        """launch_kv_unpack alone: block [2][n_layer][n][n_embd] uint16 into rows [r0, r0 + n) of copies of the uint16 caches [n_layer][n_ctx][n_embd]:
        (k, v, checksum of what the launch read, ms)."""
        block = np.ascontiguousarray(block, np.uint16)
        k = np.ascontiguousarray(k, np.uint16).copy()
        v = np.ascontiguousarray(v, np.uint16).copy()
        assert k.ndim == 3 and k.shape == v.shape and block.ndim == 4 and block.shape[:2] == (2, k.shape[0]) and block.shape[3] == k.shape[2]
        s, ms = ctypes.c_uint64(), ctypes.c_float()
        rc = self.library.minigpt4_amd_test_kv_unpack(k.shape[0], k.shape[1], k.shape[2], int(r0), block.shape[2], block.ctypes.data_as(VOID_PTR), k.ctypes.data_as(VOID_PTR),
                                                      v.ctypes.data_as(VOID_PTR), ctypes.byref(s), ctypes.byref(ms))
        if rc:
            raise RuntimeError(f"test_kv_unpack rc={rc}: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return k, v, int(s.value), float(ms.value)

    def amd_test_kv_copy_ms(self, n_slot: int, n_layer: int, rows: int, n_embd: int, src: int, dsts: Sequence[int], n_rows: int, src_rows: int = 0) -> float:
        """The same launch on device-only caches of the given shape (nothing crosses the host): its hipEvent time in ms."""
        d = np.ascontiguousarray(dsts, np.int32)
        ms = ctypes.c_float()
        rc = self.library.minigpt4_amd_test_kv_copy(n_slot, n_layer, rows, n_embd, int(src), d.ctypes.data_as(INT_PTR), len(d), int(n_rows), int(src_rows), None, None, ctypes.byref(ms))
        if rc:
            raise RuntimeError(f"test_kv_copy rc={rc}: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return float(ms.value)

    def amd_test_kv_shift(self, k: np.ndarray, v: np.ndarray, n_head: int, n_rows: int, n_keep: int, n_discard: int):
        """launch_kv_shift on fp16 caches [n_layer][n_ctx][n_embd]; returns (k, v, ms) -- shifted copies and the launch's hipEvent time."""
        k = np.ascontiguousarray(k, np.float16).copy()
        v = np.ascontiguousarray(v, np.float16).copy()
        assert k.ndim == 3 and k.shape == v.shape
        ms = ctypes.c_float()
        rc = self.library.minigpt4_amd_test_kv_shift(k.shape[0], k.shape[1], k.shape[2], n_head, n_rows, n_keep, n_discard, k.ctypes.data_as(VOID_PTR),
                                                     v.ctypes.data_as(VOID_PTR), ctypes.byref(ms))
        if rc:
            raise RuntimeError(f"test_kv_shift rc={rc}: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return k, v, float(ms.value)

    def amd_test_attn_prefill_seg(self, kc: np.ndarray, vc: np.ndarray, n_head: int, segs, q: np.ndarray, form: int = 0, fp16_rows: bool = False):
        """Segmented prompt attention (one launch) and one launch_attn_prefill per segment on fp16 caches [n_slots][n_ctx][E]; segs = [(slot, rows, pos0)], q = packed
        [N][E] fp32.  form: 0 auto, 1 h8, 2 h QS 2, 3 h QS 1, 4 exact f32.  Returns (out_seg, out_ref, seg_launched); fp16_rows: the launchers may store fp16 rows instead
        (the F16 wo's input), returns (out_seg, out_ref, seg_launched, h_seg, h_ref, (seg wrote fp16, every per-segment launch wrote fp16))."""
        kc, vc = np.ascontiguousarray(kc, np.float16), np.ascontiguousarray(vc, np.float16)
        assert kc.ndim == 3 and kc.shape == vc.shape
        S, C, E = kc.shape
        sg = np.ascontiguousarray(segs, np.int32).reshape(-1, 3)
        q = np.ascontiguousarray(q, np.float32)
        a, b, one = np.zeros_like(q), np.zeros_like(q), ctypes.c_int32()
        ha, hb, wrote = (np.zeros(q.shape, np.uint16), np.zeros(q.shape, np.uint16), (ctypes.c_int32 * 2)()) if fp16_rows else (None, None, None)
        hp = [x.ctypes.data_as(VOID_PTR) if x is not None else None for x in (ha, hb)]
        rc = self.library.minigpt4_amd_test_attn_prefill_seg(n_head, E // n_head, C, S, kc.ctypes.data_as(VOID_PTR), vc.ctypes.data_as(VOID_PTR), len(sg), sg.ctypes.data_as(INT_PTR),
                                                             q.ctypes.data_as(FLOAT_PTR), form, a.ctypes.data_as(FLOAT_PTR), b.ctypes.data_as(FLOAT_PTR), ctypes.byref(one),
                                                             hp[0], hp[1], wrote)
        if rc:
            raise RuntimeError(f"test_attn_prefill_seg rc={rc}: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        if fp16_rows:
            return a, b, bool(one.value), ha, hb, (bool(wrote[0]), bool(wrote[1]))
        return a, b, bool(one.value)

    def amd_test_rope_kv_seg(self, n_head: int, n_ctx: int, n_slots: int, segs, q: np.ndarray, k: np.ndarray, v: np.ndarray, ks: int = 1):
        """RoPE + cache append of packed rows (k_rope_kv_seg, ks > 1: the slab form) and per segment (k_rope_kv / _slabs).  Returns ((q, kc, vc) seg, (q, kc, vc) ref);
        caches [n_slots][n_ctx][E] fp16."""
        q, k, v = (np.ascontiguousarray(x, np.float32) for x in (q, k, v))
        N, E = q.shape
        sg = np.ascontiguousarray(segs, np.int32).reshape(-1, 3)
        out = [np.zeros_like(q), np.zeros((n_slots, n_ctx, E), np.float16), np.zeros((n_slots, n_ctx, E), np.float16),
               np.zeros_like(q), np.zeros((n_slots, n_ctx, E), np.float16), np.zeros((n_slots, n_ctx, E), np.float16)]
        ptr = [o.ctypes.data_as(FLOAT_PTR) if o.dtype == np.float32 else o.ctypes.data_as(VOID_PTR) for o in out]
        rc = self.library.minigpt4_amd_test_rope_kv_seg(n_head, E // n_head, n_ctx, n_slots, len(sg), sg.ctypes.data_as(INT_PTR), q.ctypes.data_as(FLOAT_PTR), k.ctypes.data_as(FLOAT_PTR),
                                                        v.ctypes.data_as(FLOAT_PTR), ks, *ptr)
        if rc:
            raise RuntimeError(f"test_rope_kv_seg rc={rc}: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return tuple(out[:3]), tuple(out[3:])

    def amd_test_attn_draft(self, mode: int, q: np.ndarray, k: np.ndarray, v: np.ndarray, kc: np.ndarray, vc: np.ndarray, n_head: int, slot: int, n_past: int,
                            computed_exp: bool = True):
        """The verify pass's attention (mode 0: one k_attn_llm_draft launch; mode 1: one launch of the batched decode kernel per row) for the rows q, k, v [R][E] of
        conversation `slot` at positions n_past ..., on fp16 caches [n_slot][n_ctx][E] given as uint16 patterns.  Returns (out [R][E], kc, vc) -- copies."""
        q, k, v = (np.ascontiguousarray(x, np.float32) for x in (q, k, v))
        kc, vc = np.array(kc, np.uint16, order="C"), np.array(vc, np.uint16, order="C")
        R, E = q.shape
        S, C, _ = kc.shape
        out = np.zeros_like(q)
        rc = self.library.minigpt4_amd_test_attn_draft(int(mode), n_head, E // n_head, C, S, slot, n_past, R, int(computed_exp), q.ctypes.data_as(FLOAT_PTR), k.ctypes.data_as(FLOAT_PTR),
                                                       v.ctypes.data_as(FLOAT_PTR), kc.ctypes.data_as(VOID_PTR), vc.ctypes.data_as(VOID_PTR), out.ctypes.data_as(FLOAT_PTR))
        if rc:
            raise RuntimeError(f"test_attn_draft rc={rc}: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return out, kc, vc

    def amd_test_attn_vsplit(self, form: int, vs: int, q: np.ndarray, k: np.ndarray, v: np.ndarray, kc: np.ndarray, vc: np.ndarray, n_head: int, row_slot: Sequence[int],
                             n_past: Sequence[int], computed_exp: bool = True):
        """One launch of the decode attention with `vs` workgroups per (head, row), each on its own share of the value columns (vs 1: the plain launch).  form 0: the
        one-row fused kernel, 1: the batched kernel (row r = conversation row_slot[r]), 2: the verify kernel (all rows in row_slot[0], consecutive positions).  q, k, v
        [rows][E]; fp16 caches [n_slot][n_ctx][E] as uint16 patterns; n_past [n_slot].  Returns (out [rows][E], kc, vc) -- copies."""
        q, k, v = (np.ascontiguousarray(x, np.float32) for x in (q, k, v))
        kc, vc = np.array(kc, np.uint16, order="C"), np.array(vc, np.uint16, order="C")
        R, E = q.shape
        S, C, _ = kc.shape
        rs, npast = np.ascontiguousarray(row_slot, np.int32), np.ascontiguousarray(n_past, np.int32)
        if len(rs) != R or len(npast) != S:
            raise ValueError("test_attn_vsplit: one slot per row and one position per slot")
        out = np.zeros_like(q)
        rc = self.library.minigpt4_amd_test_attn_vsplit(int(form), int(vs), n_head, E // n_head, C, S, R, rs.ctypes.data_as(INT_PTR), npast.ctypes.data_as(INT_PTR), int(computed_exp),
                                                        q.ctypes.data_as(FLOAT_PTR), k.ctypes.data_as(FLOAT_PTR), v.ctypes.data_as(FLOAT_PTR), kc.ctypes.data_as(VOID_PTR),
                                                        vc.ctypes.data_as(VOID_PTR), out.ctypes.data_as(FLOAT_PTR))
        if rc:
            raise RuntimeError(f"test_attn_vsplit rc={rc}: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return out, kc, vc

    def amd_test_attn_rows(self, mode: int, q: np.ndarray, k: np.ndarray, v: np.ndarray, kc: np.ndarray, vc: np.ndarray, n_head: int, n_past: int, splits: int = 0,
                           computed_exp: bool = True):
        """mode 0: q.shape[0] successive decode steps of the key-split attention (`splits` workgroups per head) on one workspace; mode 1: launch_rope_kv + the plain form
        of the decode attention for the rows at n_past ...  q, k, v [rows][E]; fp16 caches [n_ctx][E] as uint16 patterns.  Returns (out [rows + 1][E] -- the last row is
        the hook's 0xFF guard row --, q_rot [rows][E] (mode 1, else None), kc, vc) -- copies."""
        q, k, v = (np.ascontiguousarray(x, np.float32) for x in (q, k, v))
        kc, vc = np.array(kc, np.uint16, order="C"), np.array(vc, np.uint16, order="C")
        R, E = q.shape
        C, _ = kc.shape
        out = np.zeros((R + 1, E), np.float32)
        q_rot = np.zeros_like(q) if mode == 1 else None
        rc = self.library.minigpt4_amd_test_attn_rows(int(mode), n_head, E // n_head, C, int(n_past), R, int(splits), int(computed_exp), q.ctypes.data_as(FLOAT_PTR),
                                                      k.ctypes.data_as(FLOAT_PTR), v.ctypes.data_as(FLOAT_PTR), kc.ctypes.data_as(VOID_PTR), vc.ctypes.data_as(VOID_PTR),
                                                      q_rot.ctypes.data_as(FLOAT_PTR) if q_rot is not None else None, out.ctypes.data_as(FLOAT_PTR))
        if rc:
            raise RuntimeError(f"test_attn_rows rc={rc}: " + self.library.minigpt4_amd_last_error().decode("utf-8", errors="replace"))
        return out, q_rot, kc, vc

    def amd_test_ngram_draft(self, history: Sequence[int], ngram_max: int, ngram_min: int, n_draft: int) -> List[int]:
        """The draft minigpt4_amd_decode_lookup's host drafter proposes for `history` (its last token = the one about to be evaluated)."""
        h = np.ascontiguousarray(history, np.int32)
        out = np.zeros(max(int(n_draft), 1), np.int32)
        n = self.library.minigpt4_amd_test_ngram_draft(h.ctypes.data_as(INT_PTR) if len(h) else None, len(h), int(ngram_max), int(ngram_min), int(n_draft), out.ctypes.data_as(INT_PTR))
        if n < 0:
            raise ValueError("test_ngram_draft: bad arguments")
        return [int(x) for x in out[:n]]

    def amd_batch_path(self, ctx) -> dict:
        """Launch kinds of the batched step as last built (include/minigpt4_amd.h: minigpt4_amd_batch_path)."""
        out = (ctypes.c_int32 * 8)()
        if self.library.minigpt4_amd_batch_path(ctx.ptr, out):
            raise RuntimeError("minigpt4_amd_batch_path failed")
        return dict(zip(("rows", "ri", "ri_mix", "ri_ksplit", "dot4", "dot4_mix", "mul_mat", "sets"), [int(x) for x in out]))

    def amd_encode_images(self, ctx, images: Sequence[np.ndarray]) -> List[np.ndarray]:
        """minigpt4_amd_encode_images: the images (f32 CHW [3,224,224] arrays) in passes of up to 8 over the vision weights; one [32, n_embd] array per image."""
        arrs = [np.ascontiguousarray(i, dtype=np.float32) for i in images]
        structs = (MiniGPT4Image * len(arrs))(*[array_to_image_struct(a) for a in arrs])
        batch, out = MiniGPT4Images(structs, len(arrs)), MiniGPT4Embeddings()
        self.panic_if_error(self.library.minigpt4_amd_encode_images(ctx.ptr, ctypes.byref(batch), ctypes.byref(out), 0))
        try:
            return [np.ctypeslib.as_array(out.embeddings[i].data, shape=(out.embeddings[i].n_embeddings,)).copy().reshape(32, -1) for i in range(out.n_embeddings)]
        finally:
            self.library.minigpt4_amd_free_embeddings(ctypes.byref(out))

    def amd_decode_image(self, data: bytes) -> MiniGPT4Image:
        image = MiniGPT4Image()
        self.panic_if_error(self.library.minigpt4_amd_decode_image(data, len(data), ctypes.pointer(image)))
        return image

    def amd_eval_tokens(self, ctx, tokens: Sequence[int]):
        t = np.ascontiguousarray(tokens, np.int32)
        self.panic_if_error(self.library.minigpt4_amd_eval_tokens(ctx.ptr, t.ctypes.data_as(INT_PTR), len(t)))

    def amd_eval_embd(self, ctx, embd: np.ndarray):
        e = np.ascontiguousarray(embd, np.float32)
        n_embd = self.library.minigpt4_amd_n_embd(ctx.ptr)
        self.panic_if_error(self.library.minigpt4_amd_eval_embd(ctx.ptr, e.ctypes.data_as(FLOAT_PTR), e.size // n_embd))

    def amd_logits(self, ctx) -> np.ndarray:
        out = np.empty(self.library.minigpt4_amd_n_vocab(ctx.ptr), np.float32)
        assert self.library.minigpt4_amd_get_logits(ctx.ptr, out.ctypes.data_as(FLOAT_PTR), out.size) == 0
        return out

    def amd_tokenize(self, ctx, text: bytes, add_bos: bool = True) -> List[int]:
        cap = len(text) + 8
        out = (ctypes.c_int32 * cap)()
        n = self.library.minigpt4_amd_tokenize(ctx.ptr, text, int(add_bos), out, cap)
        return list(out[:n])

    def amd_decode_loop(self, ctx, steps: int):
        toks = np.zeros(steps, np.int32)
        ms = ctypes.c_float()
        rc = self.library.minigpt4_amd_decode_loop(ctx.ptr, steps, toks.ctypes.data_as(INT_PTR), ctypes.byref(ms))
        if rc:
            raise RuntimeError("decode_loop failed: " + self.library.minigpt4_amd_last_error().decode())
        return toks, float(ms.value)

    def amd_profile_sites(self, ctx, steps: int) -> dict:
        """Per-launch-site table of `steps` eager decode steps (the launch set of the captured graph): {"steps", "eager_ms_per_step", "sites": [{site, kernel, calls_per_step, avg_us, bytes_per_call}]}"""
        import json as _json
        buf = ctypes.create_string_buffer(1 << 16)
        rc = self.library.minigpt4_amd_profile_sites(ctx.ptr, steps, buf, len(buf))
        if rc:
            raise RuntimeError("profile_sites failed")
        return _json.loads(buf.value.decode())

    def amd_test_mul_mat(self, ggml_type: int, raw_w: np.ndarray, n_in: int, n_out: int, x: np.ndarray, ref: bool = False) -> np.ndarray:
        """ref: the parity-mode kernel (oracle accumulation order) instead of the engine's fast dispatch."""
        x = np.ascontiguousarray(x, np.float32).reshape(-1, n_in)
        raw_w = np.ascontiguousarray(raw_w)
        y = np.empty((x.shape[0], n_out), np.float32)
        fn = self.library.minigpt4_amd_test_mul_mat_ref if ref else self.library.minigpt4_amd_test_mul_mat
        rc = fn(ggml_type, raw_w.ctypes.data_as(VOID_PTR), n_in, n_out, x.ctypes.data_as(FLOAT_PTR), x.shape[0],
                                                    y.ctypes.data_as(FLOAT_PTR))
        if rc:
            raise RuntimeError(f"test_mul_mat rc={rc}: " + self.library.minigpt4_amd_last_error().decode())
        return y

    def amd_test_mmq2(self, ggml_type: int, raw_w: np.ndarray, n_mat: int, n_in: int, n_out: int, x: np.ndarray, residual: Optional[np.ndarray] = None, ks: int = 0,
                      generation: int = 2) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32).reshape(-1, n_in)
        raw_w = np.ascontiguousarray(raw_w)
        N = x.shape[0]
        y = np.empty((n_mat, N, n_out), np.float32)
        r = np.ascontiguousarray(residual, np.float32) if residual is not None else None
        rc = self.library.minigpt4_amd_test_mmq2(ggml_type, raw_w.ctypes.data_as(VOID_PTR), n_mat, n_in, n_out, x.ctypes.data_as(FLOAT_PTR), N,
                                                 r.ctypes.data_as(FLOAT_PTR) if r is not None else None, ks, generation, y.ctypes.data_as(FLOAT_PTR))
        if rc:
            raise RuntimeError(f"amd_test_mmq2 failed ({rc}): " + self.library.minigpt4_amd_last_error().decode())
        return y

    def amd_test_matvec(self, type1: int, raw1: np.ndarray, n1: int, n_in: int, n_out: int, x: np.ndarray, x2: Optional[np.ndarray] = None, prep: int = 2,
                        fuse: bool = False, epi: int = 0, residual: Optional[np.ndarray] = None, type2: int = 0, raw2: Optional[np.ndarray] = None,
                        silu_table: Optional[np.ndarray] = None, computed: bool = False) -> np.ndarray:
        """Decode mat-vec launches exactly as the engine issues them (see include/minigpt4_amd_test.h).  silu_table: the fp16 SiLU table (uint16[65536]) that prep 3 / epi 1
        gather from; computed: no table, the kernels compute its values (the decode step's fast-mode arm); neither: the hook's own host-libm table."""
        x = np.ascontiguousarray(x, np.float32).reshape(n_in)
        x2c = None if x2 is None else np.ascontiguousarray(x2, np.float32).reshape(n_in)
        raw1 = np.ascontiguousarray(raw1)
        n2 = 0 if raw2 is None else 1
        raw2c = None if raw2 is None else np.ascontiguousarray(raw2)
        res = None if residual is None else np.ascontiguousarray(residual, np.float32).reshape(-1)
        y = np.empty(((1 if epi == 1 else n1 + n2), n_out), np.float32)      # epi 1: the SiLU pair epilogue writes one row; 2: the CPU oracle's fp32 order (k-quants)
        args = [type1, raw1.ctypes.data_as(VOID_PTR), n1, type2, None if raw2c is None else raw2c.ctypes.data_as(VOID_PTR), n2,
                n_in, n_out, x.ctypes.data_as(FLOAT_PTR), None if x2c is None else x2c.ctypes.data_as(FLOAT_PTR), prep, int(fuse), epi,
                None if res is None else res.ctypes.data_as(FLOAT_PTR)]
        if computed or silu_table is not None:
            tab = None if computed else self._table_arg(silu_table)
            rc = self.library.minigpt4_amd_test_matvec_ex(*args, None if tab is None else tab.ctypes.data_as(VOID_PTR), y.ctypes.data_as(FLOAT_PTR))
        else:
            rc = self.library.minigpt4_amd_test_matvec(*args, y.ctypes.data_as(FLOAT_PTR))
        if rc:
            raise RuntimeError(f"test_matvec rc={rc}: " + self.library.minigpt4_amd_last_error().decode())
        return y

    def amd_test_matvec_issue(self, type1: int, raw1: np.ndarray, n1: int, n_in: int, n_out: int, x: np.ndarray, x2: Optional[np.ndarray] = None, prep: int = 1, epi: int = 0,
                              residual: Optional[np.ndarray] = None, type2: int = 0, raw2: Optional[np.ndarray] = None, issue_barrier: bool = False, guard: int = 0):
        """ONE prologue launch of the decode mat-vec (preparation `prep` fused) with or without the issue barrier (csrc/llm_kernels.hip: IB).  Returns (y, guard):
        y as amd_test_matvec, guard = the `guard` floats behind the outputs as uint32 bit patterns (0xFFFFFFFF where the launch left them alone)."""
        x = np.ascontiguousarray(x, np.float32).reshape(n_in)
        x2c = None if x2 is None else np.ascontiguousarray(x2, np.float32).reshape(n_in)
        raw1 = np.ascontiguousarray(raw1)
        n2 = 0 if raw2 is None else 1
        raw2c = None if raw2 is None else np.ascontiguousarray(raw2)
        res = None if residual is None else np.ascontiguousarray(residual, np.float32).reshape(-1)
        rows = 1 if epi == 1 else n1 + n2
        buf = np.empty(rows * n_out + guard, np.float32)
        rc = self.library.minigpt4_amd_test_matvec_issue(type1, raw1.ctypes.data_as(VOID_PTR), n1, type2, None if raw2c is None else raw2c.ctypes.data_as(VOID_PTR), n2, n_in, n_out,
                                                         x.ctypes.data_as(FLOAT_PTR), None if x2c is None else x2c.ctypes.data_as(FLOAT_PTR), prep, epi,
                                                         None if res is None else res.ctypes.data_as(FLOAT_PTR), int(issue_barrier), int(guard), buf.ctypes.data_as(FLOAT_PTR))
        if rc:
            raise RuntimeError(f"test_matvec_issue rc={rc}: " + self.library.minigpt4_amd_last_error().decode())
        return buf[:rows * n_out].reshape(rows, n_out).copy(), buf[rows * n_out:].view(np.uint32).copy()

    def amd_test_matvec_waves(self) -> int:
        """Waves of a prologue mat-vec launch that fills the device: wave w owns row groups w, w + waves, ..."""
        return int(self.library.minigpt4_amd_test_matvec_waves())

    def amd_test_matvec_predicates(self, ggml_type: int, n_in: int):
        """(single-row prologue, SiLU pair epilogue, multi-row prologue): which in-launch preparations the decode mat-vec offers for (type, n_in).  Needs no GPU."""
        f = self.library.minigpt4_amd_test_matvec_predicates
        f.argtypes = [I32, ctypes.c_int64]
        bits = int(f(ggml_type, n_in))
        if bits < 0:
            raise ValueError("amd_test_matvec_predicates: bad arguments")
        return bool(bits & 1), bool(bits & 2), bool(bits & 4)

    def amd_test_matvec_rows(self, ggml_type: int, raw_w: np.ndarray, n_mat: int, n_in: int, n_out: int, x: np.ndarray, residual: Optional[np.ndarray] = None,
                             rms_w: Optional[np.ndarray] = None, prepare: bool = False) -> np.ndarray:
        """The batched-decode mat-vec: x [N][n_in] (N <= 4) against n_mat matrices in one weight pass -> [n_mat][N][n_out].  prepare: the rows are prepared inside the
        launch (rms_w: rms_norm(x_t) * rms_w, else as they are); otherwise by a launch of their own in front."""
        x = np.ascontiguousarray(x, np.float32).reshape(-1, n_in)
        raw_w = np.ascontiguousarray(raw_w)
        res = None if residual is None else np.ascontiguousarray(residual, np.float32)
        y = np.empty((n_mat, x.shape[0], n_out), np.float32)
        if rms_w is not None or prepare:
            f = self.library.minigpt4_amd_test_matvec_rows_prep
            f.argtypes = [I32, VOID_PTR, I32, ctypes.c_int64, ctypes.c_int64, FLOAT_PTR, I32, FLOAT_PTR, FLOAT_PTR, I32, FLOAT_PTR]
            w = None if rms_w is None else np.ascontiguousarray(rms_w, np.float32).reshape(n_in)
            rc = f(ggml_type, raw_w.ctypes.data_as(VOID_PTR), n_mat, n_in, n_out, x.ctypes.data_as(FLOAT_PTR), x.shape[0], None if res is None else res.ctypes.data_as(FLOAT_PTR),
                   None if w is None else w.ctypes.data_as(FLOAT_PTR), int(bool(prepare)), y.ctypes.data_as(FLOAT_PTR))
        else:
            rc = self.library.minigpt4_amd_test_matvec_rows(ggml_type, raw_w.ctypes.data_as(VOID_PTR), n_mat, n_in, n_out, x.ctypes.data_as(FLOAT_PTR), x.shape[0],
                                                            None if res is None else res.ctypes.data_as(FLOAT_PTR), y.ctypes.data_as(FLOAT_PTR))
        if rc:
            raise RuntimeError(f"test_matvec_rows rc={rc}: " + self.library.minigpt4_amd_last_error().decode())
        return y

    def amd_test_matvec_rows_mixed(self, type_a: int, raw_a: np.ndarray, n_a: int, type_b: int, raw_b: np.ndarray, n_b: int, n_in: int, n_out: int, x: np.ndarray):
        """The batched decode's two-type launch (k_matvec_tn_mix): x [N][n_in] (N <= 4) -> (y [n_a + n_b][N][n_out], guard: the n_out floats behind them as uint32 bit
        patterns, 0xFFFFFFFF where the launch left them alone)."""
        x = np.ascontiguousarray(x, np.float32).reshape(-1, n_in)
        raw_a, raw_b = np.ascontiguousarray(raw_a), np.ascontiguousarray(raw_b)
        n, N = n_a + n_b, x.shape[0]
        buf = np.empty((n * N + 1, n_out), np.float32)
        f = self.library.minigpt4_amd_test_matvec_rows_mixed
        f.argtypes = [I32, VOID_PTR, I32, I32, VOID_PTR, I32, ctypes.c_int64, ctypes.c_int64, FLOAT_PTR, I32, FLOAT_PTR]
        rc = f(type_a, raw_a.ctypes.data_as(VOID_PTR), n_a, type_b, raw_b.ctypes.data_as(VOID_PTR), n_b, n_in, n_out, x.ctypes.data_as(FLOAT_PTR), N, buf.ctypes.data_as(FLOAT_PTR))
        if rc:
            raise RuntimeError(f"test_matvec_rows_mixed rc={rc}: " + self.library.minigpt4_amd_last_error().decode())
        return buf[:n * N].reshape(n, N, n_out).copy(), buf[n * N].view(np.uint32).copy()

    def amd_test_matvec_ri(self, ggml_type: int, raw_w: np.ndarray, n_mat: int, n_in: int, n_out: int, x: np.ndarray, residual: Optional[np.ndarray] = None,
                           rms_w: Optional[np.ndarray] = None) -> np.ndarray:
        """The batched decode's MFMA launch over the row-interleaved image (csrc/ri_kernels.hip): x [N][n_in] (N <= 4) -> [n_mat][N][n_out]."""
        x = np.ascontiguousarray(x, np.float32).reshape(-1, n_in)
        raw_w = np.ascontiguousarray(raw_w)
        res = None if residual is None else np.ascontiguousarray(residual, np.float32)
        y = np.empty((n_mat, x.shape[0], n_out), np.float32)
        f = self.library.minigpt4_amd_test_matvec_ri
        f.argtypes = [I32, VOID_PTR, I32, ctypes.c_int64, ctypes.c_int64, FLOAT_PTR, I32, FLOAT_PTR, FLOAT_PTR, FLOAT_PTR]
        w = None if rms_w is None else np.ascontiguousarray(rms_w, np.float32)
        rc = f(ggml_type, raw_w.ctypes.data_as(VOID_PTR), n_mat, n_in, n_out, x.ctypes.data_as(FLOAT_PTR), x.shape[0], None if res is None else res.ctypes.data_as(FLOAT_PTR),
               None if w is None else w.ctypes.data_as(FLOAT_PTR), y.ctypes.data_as(FLOAT_PTR))
        if rc:
            raise RuntimeError(f"test_matvec_ri rc={rc}: " + self.library.minigpt4_amd_last_error().decode())
        return y

    def amd_test_matvec_ri_mixed(self, type_a: int, raw_a: np.ndarray, n_a: int, type_b: int, raw_b: np.ndarray, n_b: int, n_in: int, n_out: int, x: np.ndarray) -> np.ndarray:
        """The mixed-type MFMA launch of a "more bits" layer (wq | wk of Q4_K / Q5_K + a Q6_K wv): x [N][n_in] (N <= 4) -> [n_a + n_b][N][n_out]."""
        x = np.ascontiguousarray(x, np.float32).reshape(-1, n_in)
        raw_a, raw_b = np.ascontiguousarray(raw_a), np.ascontiguousarray(raw_b)
        y = np.empty((n_a + n_b, x.shape[0], n_out), np.float32)
        f = self.library.minigpt4_amd_test_matvec_ri_mixed
        f.argtypes = [I32, VOID_PTR, I32, I32, VOID_PTR, I32, ctypes.c_int64, ctypes.c_int64, FLOAT_PTR, I32, FLOAT_PTR]
        rc = f(type_a, raw_a.ctypes.data_as(VOID_PTR), n_a, type_b, raw_b.ctypes.data_as(VOID_PTR), n_b, n_in, n_out, x.ctypes.data_as(FLOAT_PTR), x.shape[0], y.ctypes.data_as(FLOAT_PTR))
        if rc:
            raise RuntimeError(f"test_matvec_ri_mixed rc={rc}: " + self.library.minigpt4_amd_last_error().decode())
        return y

    def amd_test_quantize(self, x: np.ndarray, rms_w: Optional[np.ndarray] = None):
        x = np.ascontiguousarray(x, np.float32)
        N, K = x.shape
        q8k, dk, bs = np.empty((N, K), np.int8), np.empty((N, K // 256), np.float32), np.empty((N, K // 16), np.int16)
        q80, d0 = np.empty((N, K), np.int8), np.empty((N, K // 32), np.float32)
        w = None if rms_w is None else np.ascontiguousarray(rms_w, np.float32)
        rc = self.library.minigpt4_amd_test_quantize(x.ctypes.data_as(FLOAT_PTR), None if w is None else w.ctypes.data_as(FLOAT_PTR), N, K,
                                                     q8k.ctypes.data_as(VOID_PTR), dk.ctypes.data_as(VOID_PTR), bs.ctypes.data_as(VOID_PTR),
                                                     q80.ctypes.data_as(VOID_PTR), d0.ctypes.data_as(VOID_PTR))
        if rc:
            raise RuntimeError(f"test_quantize rc={rc}")
        return q8k, dk, bs, q80, d0

    def amd_test_get_rows(self, ggml_type: int, raw_table: np.ndarray, n_rows: int, K: int, tokens) -> np.ndarray:
        """The embedding gather alone (one launch_get_rows over a raw table [n_rows][K]): returns [N + 1][K] fp32 -- row N is the guard row, a row whose token is -1 and
        the guard row keep their 0xFF fill.  ValueError for arguments the hook refuses before it touches a device."""
        raw = np.ascontiguousarray(raw_table)
        tok = np.ascontiguousarray(tokens, np.int32).reshape(-1)
        out = np.zeros((tok.size + 1, K), np.float32)
        f = self.library.minigpt4_amd_test_get_rows
        f.argtypes = [I32, VOID_PTR, I32, ctypes.c_int64, VOID_PTR, I32, FLOAT_PTR]
        rc = f(ggml_type, raw.ctypes.data_as(VOID_PTR), n_rows, K, tok.ctypes.data_as(VOID_PTR), tok.size, out.ctypes.data_as(FLOAT_PTR))
        if rc == 1:
            raise ValueError("amd_test_get_rows: bad arguments")
        if rc:
            raise RuntimeError(f"test_get_rows rc={rc}: " + self.library.minigpt4_amd_last_error().decode())
        return out

    @staticmethod
    def _table_arg(table: np.ndarray) -> np.ndarray:
        t = np.ascontiguousarray(table).view(np.uint16).reshape(-1)
        if t.size != 65536:
            raise ValueError("an fp16 table has 65536 entries")
        return t

    def amd_test_activation(self, which: int, table: Optional[np.ndarray] = None) -> np.ndarray:
        """GELU (0) / SiLU (1) / exp (2) of csrc/activations.hpp on all 65536 fp16 bit patterns -> uint16[65536]; table: gathered from it, None: the computed form."""
        out = np.zeros(65536, np.uint16)
        tab = None if table is None else self._table_arg(table)
        rc = self.library.minigpt4_amd_test_activation(which, None if tab is None else tab.ctypes.data_as(VOID_PTR), out.ctypes.data_as(VOID_PTR))
        if rc:
            raise RuntimeError(f"test_activation rc={rc}: " + self.library.minigpt4_amd_last_error().decode())
        return out

    def amd_test_f16_silu_pair(self, x: np.ndarray, w: np.ndarray, silu_table: Optional[np.ndarray] = None, computed: bool = False):
        """The F16 w1 | w3 pair launch: x [N][n_in] fp32, w [2 * n_out][n_in] fp16 (w1 then w3) -> (fp16 bits [N][n_out], fp32 [N][n_out]).  Table arms as amd_test_matvec."""
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(w, np.float16)
        N, n_in = x.shape
        n_out = w.shape[0] // 2
        oh, of = np.zeros((N, n_out), np.uint16), np.zeros((N, n_out), np.float32)
        if computed or silu_table is not None:
            tab = None if computed else self._table_arg(silu_table)
            rc = self.library.minigpt4_amd_test_f16_silu_pair_ex(x.ctypes.data_as(FLOAT_PTR), w.ctypes.data_as(VOID_PTR), N, n_in, n_out,
                                                                 None if tab is None else tab.ctypes.data_as(VOID_PTR), oh.ctypes.data_as(VOID_PTR), of.ctypes.data_as(FLOAT_PTR))
        else:
            rc = self.library.minigpt4_amd_test_f16_silu_pair(x.ctypes.data_as(FLOAT_PTR), w.ctypes.data_as(VOID_PTR), N, n_in, n_out, oh.ctypes.data_as(VOID_PTR), of.ctypes.data_as(FLOAT_PTR))
        if rc:
            raise RuntimeError(f"test_f16_silu_pair rc={rc}: " + self.library.minigpt4_amd_last_error().decode())
        return oh, of

    def amd_test_attn_f32(self, q: np.ndarray, k: np.ndarray, v: np.ndarray, heads: int, hd: int, nq: int, nk: int, batch: int = 1, q_prescale: float = 0.0,
                          score_div: float = 0.0, head_major: bool = False, qt: int = 0, exp_table: Optional[np.ndarray] = None):
        """The ViT / Q-Former attention kernel on q [batch * nq][heads * hd], k / v [batch * nk][heads * hd] -> (fp32 [batch * nq][heads * hd], the same as fp16 bits).
        exp_table None: computed exponentials (fast mode's arm)."""
        D = heads * hd
        q = np.ascontiguousarray(q, np.float32).reshape(batch * nq, D)
        k = np.ascontiguousarray(k, np.float32).reshape(batch * nk, D)
        v = np.ascontiguousarray(v, np.float32).reshape(batch * nk, D)
        out, out_h = np.zeros((batch * nq, D), np.float32), np.zeros((batch * nq, D), np.uint16)
        tab = None if exp_table is None else self._table_arg(exp_table)
        rc = self.library.minigpt4_amd_test_attn_f32(q.ctypes.data_as(FLOAT_PTR), k.ctypes.data_as(FLOAT_PTR), v.ctypes.data_as(FLOAT_PTR), heads, hd, nq, nk, batch,
                                                     q_prescale, score_div, int(head_major), qt, None if tab is None else tab.ctypes.data_as(VOID_PTR),
                                                     out.ctypes.data_as(FLOAT_PTR), out_h.ctypes.data_as(VOID_PTR))
        if rc:
            raise RuntimeError(f"test_attn_f32 rc={rc}: " + self.library.minigpt4_amd_last_error().decode())
        return out, out_h

    def amd_test_gemm_f16(self, A: np.ndarray, W: np.ndarray, bias: Optional[np.ndarray] = None, gelu: bool = False, skinny: bool = False,
                          gelu_table: Optional[np.ndarray] = None, computed: bool = False) -> np.ndarray:
        """gelu_table: the fp16 GELU table (uint16[65536]) the epilogue gathers from; computed: no table, the epilogue computes (fast mode's arm); neither: the hook's host-libm table."""
        A = np.ascontiguousarray(A, np.float32)
        W = np.ascontiguousarray(W, np.float32)
        M, K = A.shape
        N = W.shape[0]
        C = np.empty((M, N), np.float32)
        b = None if bias is None else np.ascontiguousarray(bias, np.float32)
        if computed or gelu_table is not None:
            tab = None if computed else self._table_arg(gelu_table)
            rc = self.library.minigpt4_amd_test_gemm_f16_ex(A.ctypes.data_as(FLOAT_PTR), W.ctypes.data_as(FLOAT_PTR), None if b is None else b.ctypes.data_as(FLOAT_PTR), M, N, K,
                                                            int(gelu), int(skinny), None if tab is None else tab.ctypes.data_as(VOID_PTR), C.ctypes.data_as(FLOAT_PTR))
        else:
            fn = self.library.minigpt4_amd_test_gemm_f16_skinny if skinny else self.library.minigpt4_amd_test_gemm_f16
            rc = fn(A.ctypes.data_as(FLOAT_PTR), W.ctypes.data_as(FLOAT_PTR), None if b is None else b.ctypes.data_as(FLOAT_PTR), M, N, K, int(gelu), C.ctypes.data_as(FLOAT_PTR))
        if rc:
            raise RuntimeError(f"test_gemm_f16 rc={rc}")
        return C

    # ---- the image encoder's kernels between its GEMMs (include/minigpt4_amd_test.h).  These wrappers RETURN the hook's code first instead of raising (the tests assert the
    # refusals too); every output array is created filled with HOOK_FILL bytes, so an output the hook did not copy back is recognisable, and keeps the hook's guard row.
    HOOK_FILL = 0xA5

    @classmethod
    def _hook_out(cls, shape, dtype) -> np.ndarray:
        a = np.empty(shape, dtype)
        a.view(np.uint8).fill(cls.HOOK_FILL)
        return a

    @staticmethod
    def _f32p(a: Optional[np.ndarray]):
        return None if a is None else a.ctypes.data_as(FLOAT_PTR)

    @staticmethod
    def _vp(a: Optional[np.ndarray]):
        return None if a is None else a.ctypes.data_as(VOID_PTR)

    @staticmethod
    def _f32(a, shape=None) -> Optional[np.ndarray]:
        if a is None:
            return None
        a = np.ascontiguousarray(a, np.float32)
        return a if shape is None else a.reshape(shape)

    def amd_test_layernorm(self, x: np.ndarray, w: np.ndarray, b: Optional[np.ndarray] = None, sequential: bool = False, want_out: bool = True, want_out_h: bool = True):
        """One launch_layernorm on x [rows][n] -> (rc, out fp32 [rows + 1][n] or None, out_h uint16 [rows + 1][n] or None); the last row is the hook's guard row."""
        x = self._f32(x)
        rows, n = x.shape
        w, b = self._f32(w, (n,)), self._f32(b, (n,))
        out = self._hook_out((rows + 1, n), np.float32) if want_out else None
        out_h = self._hook_out((rows + 1, n), np.uint16) if want_out_h else None
        rc = self.library.minigpt4_amd_test_layernorm(self._f32p(x), self._f32p(w), self._f32p(b), rows, n, int(sequential), self._f32p(out), self._vp(out_h))
        return rc, out, out_h

    def amd_test_splitk_reduce_ln(self, slabs: np.ndarray, rows: int, n: int, bias: Optional[np.ndarray] = None, residual: Optional[np.ndarray] = None, in_place: bool = False,
                                  ln_w: Optional[np.ndarray] = None, ln_b: Optional[np.ndarray] = None, want_x: bool = True, want_ln: bool = True, want_ln_h: bool = True):
        """One launch_splitk_reduce_ln.  slabs [n_slabs][slab_stride] fp32 (slab_stride >= rows * n, padding included) -> (rc, x_out, ln_out, ln_out_h), each [rows + 1][n]
        (guard row last) or None; without ln_w only x_out is produced."""
        slabs = self._f32(slabs)
        n_slabs, stride = slabs.shape
        bias, residual, ln_w, ln_b = self._f32(bias, (n,)), self._f32(residual, (rows, n)), self._f32(ln_w, (n,)), self._f32(ln_b, (n,))
        x_out = self._hook_out((rows + 1, n), np.float32) if want_x else None
        ln_out = self._hook_out((rows + 1, n), np.float32) if want_ln and ln_w is not None else None
        ln_out_h = self._hook_out((rows + 1, n), np.uint16) if want_ln_h and ln_w is not None else None
        rc = self.library.minigpt4_amd_test_splitk_reduce_ln(self._f32p(slabs), n_slabs, stride, self._f32p(bias), self._f32p(residual), int(in_place), rows, n, self._f32p(ln_w),
                                                             self._f32p(ln_b), self._f32p(x_out), self._f32p(ln_out), self._vp(ln_out_h))
        return rc, x_out, ln_out, ln_out_h

    def amd_test_gemm_f16_splitk(self, A: np.ndarray, W: np.ndarray, slices: int, skinny: bool = False):
        """The split-K GEMM forms -> (rc, slabs fp32 [slices wanted][M][N], slices used); rc 0: slabs[:used] are the raw partial products, otherwise nothing was written."""
        A, W = self._f32(A), self._f32(W)
        (M, K), N = A.shape, W.shape[0]
        slabs = self._hook_out((max(1, slices), M, N), np.float32)
        used = ctypes.c_int32(-1)
        rc = self.library.minigpt4_amd_test_gemm_f16_splitk(self._f32p(A), self._f32p(W), M, N, K, slices, int(skinny), self._f32p(slabs), ctypes.byref(used))
        return rc, slabs, used.value

    def amd_test_gemm_f16_head_major(self, A: np.ndarray, W: np.ndarray, bias: Optional[np.ndarray], D: int, hd: int):
        """launch_gemm_f16_head_major, W [3 * D][K] -> (rc, fp32 [(M + 2) * 3 * D]: 3 * D guard floats, [3][D / hd][M][hd], 3 * D guard floats)."""
        A, W = self._f32(A), self._f32(W)
        M, K = A.shape
        assert W.shape == (3 * D, K)
        bias = self._f32(bias, (3 * D,))
        out = self._hook_out(((M + 2) * 3 * D,), np.float32)
        rc = self.library.minigpt4_amd_test_gemm_f16_head_major(self._f32p(A), self._f32p(W), self._f32p(bias), M, D, hd, K, self._f32p(out))
        return rc, out

    def amd_test_im2col(self, image: np.ndarray, ldp: int = 592):
        """launch_im2col on image [B][3][224][224] -> (rc, uint16 [B * 256 + 1][ldp] fp16 bit patterns, guard row last)."""
        image = self._f32(image)
        B = image.shape[0]
        assert image.shape == (B, 3, 224, 224)
        out = self._hook_out((B * 256 + 1, ldp), np.uint16)
        return self.library.minigpt4_amd_test_im2col(self._f32p(image), B, ldp, self._vp(out)), out

    def amd_test_assemble(self, cls_token: np.ndarray, pe: np.ndarray, pos: np.ndarray):
        """launch_assemble_embeddings: cls [D], pe [B * 256][D], pos [257][D] -> (rc, fp32 [B * 257 + 1][D], guard row last)."""
        pe = self._f32(pe)
        D = pe.shape[1]
        B = pe.shape[0] // 256
        assert pe.shape[0] == B * 256
        cls_token, pos = self._f32(cls_token, (D,)), self._f32(pos, (257, D))
        out = self._hook_out((B * 257 + 1, D), np.float32)
        return self.library.minigpt4_amd_test_assemble(self._f32p(cls_token), self._f32p(pe), self._f32p(pos), B, D, self._f32p(out)), out

    def amd_test_lin_epilogue(self, y: np.ndarray, bias: Optional[np.ndarray] = None, residual: Optional[np.ndarray] = None, gelu_table: Optional[np.ndarray] = None,
                              want_out: bool = True, want_out_h: bool = True):
        """launch_lin_epilogue on y [rows][n] -> (rc, out fp32 [rows + 1][n] or None, out_h uint16 [rows + 1][n] or None); gelu_table given = with the GELU step."""
        y = self._f32(y)
        rows, n = y.shape
        bias, residual = self._f32(bias, (n,)), self._f32(residual, (rows, n))
        tab = None if gelu_table is None else self._table_arg(gelu_table)
        out = self._hook_out((rows + 1, n), np.float32) if want_out else None
        out_h = self._hook_out((rows + 1, n), np.uint16) if want_out_h else None
        rc = self.library.minigpt4_amd_test_lin_epilogue(self._f32p(y), self._f32p(bias), self._f32p(residual), self._vp(tab), rows, n, self._f32p(out), self._vp(out_h))
        return rc, out, out_h

    # ---- the activation-preparation kernels and the consumers of a deferred split-K combine (include/minigpt4_amd_test.h).  Same form as the image encoder's hooks above: the
    # hook's code comes back first, every output is created filled with HOOK_FILL bytes and keeps the hook's guard row.
    ACT_Q8K, ACT_Q80, ACT_F16, ACT_F32 = 1, 2, 4, 8
    PLANE_BSQ, PLANE_BS16, PLANE_Q16 = 1, 2, 4
    ACT_PLANES = ("q8k", "dk", "bsk", "bsq", "bs16", "q16", "q80", "d0", "d1", "s1", "sum0", "xh", "xf")

    @staticmethod
    def act_plane_shapes(N: int, K: int) -> dict:
        """name -> (shape of N + 1 rows, dtype) of an ActQ's thirteen planes as the hooks return them (fp16 planes as uint16 bit patterns)."""
        return {"q8k": ((N + 1, K), np.int8), "dk": ((N + 1, K // 256), np.float32), "bsk": ((N + 1, K // 16), np.int16), "bsq": ((N + 1, K // 256, 16), np.int8),
                "bs16": ((N + 1, K // 256, 16), np.uint16), "q16": ((N + 1, K), np.uint16), "q80": ((N + 1, K), np.int8), "d0": ((N + 1, K // 32), np.float32),
                "d1": ((N + 1, K // 32), np.float32), "s1": ((N + 1, K // 32), np.float32), "sum0": ((N + 1, K // 32), np.int32), "xh": ((N + 1, K), np.uint16),
                "xf": ((N + 1, K), np.float32)}

    def _act_outs(self, N: int, K: int):
        outs = {name: self._hook_out(shape, dtype) for name, (shape, dtype) in self.act_plane_shapes(N, K).items()}
        return outs, [self._vp(outs[name]) for name in self.ACT_PLANES]

    def amd_test_prepare(self, launcher: int, x: np.ndarray, second: Optional[np.ndarray] = None, mask: int = 1, planes: int = 0, sequential_sum: bool = False,
                         silu_table: Optional[np.ndarray] = None):
        """One launch_rms_quant (launcher 0, second = the norm weight [K]) or launch_silu_mul_quant (launcher 1, second = b [N][K]) on x [N][K] -> (rc, {plane: N + 1 rows})."""
        x = self._f32(x)
        N, K = x.shape
        second = self._f32(second, (K,) if launcher == 0 else (N, K))
        tab = None if silu_table is None else self._table_arg(silu_table)
        outs, ptrs = self._act_outs(N, K)
        rc = self.library.minigpt4_amd_test_prepare(launcher, self._f32p(x), self._f32p(second), N, K, mask, planes, int(sequential_sum), self._vp(tab), *ptrs)
        return rc, outs

    def amd_test_prepare_slabs(self, launcher: int, slabs: np.ndarray, N: int, K: int, residual: Optional[np.ndarray] = None, in_place: bool = False,
                               w: Optional[np.ndarray] = None, mask: int = 1, planes: int = 0, silu_table: Optional[np.ndarray] = None):
        """One launch_rms_quant_slabs (launcher 0: slabs [ks][stride]) or launch_silu_mul_quant_slabs (launcher 1: slabs [2][ks][stride]) -> (rc, x_out [N + 1][K] or None,
        {plane: N + 1 rows})."""
        slabs = self._f32(slabs)
        ks, stride = slabs.shape[-2:]
        assert slabs.shape == ((ks, stride) if launcher == 0 else (2, ks, stride))
        residual, w = self._f32(residual, (N, K)), self._f32(w, (K,))
        tab = None if silu_table is None else self._table_arg(silu_table)
        x_out = self._hook_out((N + 1, K), np.float32) if launcher == 0 else None
        outs, ptrs = self._act_outs(N, K)
        rc = self.library.minigpt4_amd_test_prepare_slabs(launcher, self._f32p(slabs), ks, stride, self._f32p(residual), int(in_place), self._f32p(w), N, K, mask, planes,
                                                          self._vp(tab), self._f32p(x_out), *ptrs)
        return rc, x_out, outs

    def amd_test_slab_flush(self, mks: Sequence[int], slabs: np.ndarray, stride: int, mixed: bool = False, residual: Optional[np.ndarray] = None, residual_mask: int = 0,
                            in_place: Optional[dict] = None):
        """One launch_slab_flush: slabs [sum of the counts above 1][stride], residual [n][stride]; in_place {matrix: its contents [stride]} for the matrices whose count is 1
        -> (rc, y [n + 1][stride], guard row last)."""
        m = np.ascontiguousarray(mks, np.int32)
        n = m.size
        slabs, residual = self._f32(slabs), self._f32(residual, (n, stride))
        y = self._hook_out((n + 1, stride), np.float32)
        for i, rows in (in_place or {}).items():
            y[i] = rows
        rc = self.library.minigpt4_amd_test_slab_flush(n, int(mixed), m.ctypes.data_as(INT_PTR), self._f32p(slabs), stride, self._f32p(residual), residual_mask, self._f32p(y))
        return rc, y

    def amd_test_rope_kv_slabs(self, n_head: int, hd: int, n_ctx: int, N: int, pos0: int, mks: Sequence[int], slabs: np.ndarray, stride: int,
                               v_in_place: Optional[np.ndarray] = None):
        """One launch_rope_kv_slabs with a slab count per matrix -> (rc, q [N + 1][E] with its guard row, kc [n_ctx][E] fp16, vc [n_ctx][E] fp16)."""
        m = np.ascontiguousarray(mks, np.int32)
        E = n_head * hd
        slabs, v_in_place = self._f32(slabs), self._f32(v_in_place, (N, E))
        q = self._hook_out((N + 1, E), np.float32)
        kc, vc = self._hook_out((n_ctx, E), np.float16), self._hook_out((n_ctx, E), np.float16)
        rc = self.library.minigpt4_amd_test_rope_kv_slabs(n_head, hd, n_ctx, N, pos0, m.ctypes.data_as(INT_PTR), self._f32p(slabs), stride, self._f32p(v_in_place), self._f32p(q),
                                                          self._vp(kc), self._vp(vc))
        return rc, q, kc, vc

    def amd_sample_logits(self, logits: np.ndarray, seed: int, temp=0.8, top_k=40, top_p=0.9, tfs_z=1.0, typical_p=1.0, mirostat=0, mirostat_tau=5.0,
                          mirostat_eta=1.0) -> int:
        lg = np.ascontiguousarray(logits, np.float32)
        return int(self.library.minigpt4_amd_sample_logits(lg.ctypes.data_as(FLOAT_PTR), lg.size, seed, temp, top_k, top_p, tfs_z, typical_p, mirostat,
                                                           mirostat_tau, mirostat_eta))


def default_library_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libminigpt4.so")


def load_library() -> MiniGPT4SharedLibrary:
    """Reference `load_library` (:525-566) searches a few relative paths for libminigpt4.so; here the in-tree build is used."""
    path = os.environ.get("MINIGPT4_LIBRARY", default_library_path())
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    return MiniGPT4SharedLibrary(path)


def image_to_array(image, size: int = 224) -> np.ndarray:
    """Preprocessing of the reference's ChatBot (:589-600, 682-687) without torchvision: RGB, bicubic resize to 224x224, /255,
    CLIP mean/std, HWC -> CHW float32."""
    from PIL import Image
    if not isinstance(image, Image.Image):
        image = Image.open(image)
    image = image.convert("RGB").resize((size, size), Image.BICUBIC)
    a = np.asarray(image, np.float32) / 255.0
    a = (a - np.asarray(CLIP_MEAN, np.float32)) / np.asarray(CLIP_STD, np.float32)
    return np.ascontiguousarray(a.transpose(2, 0, 1))


def array_to_image_struct(chw: np.ndarray) -> MiniGPT4Image:
    chw = np.ascontiguousarray(chw, np.float32)
    assert chw.shape == (3, 224, 224)
    img = MiniGPT4Image(chw.ctypes.data_as(VOID_PTR), 224, 224, 3, int(ImageFormat.F32))
    img._keepalive = chw
    return img


class MiniGPT4ChatBot:
    """Reference class of the same name (:568-689): upload_image / generate / reset_chat."""

    def __init__(self, model_path: str, llm_model_path: str, verbosity: Verbosity = Verbosity.SILENT, n_threads: int = 0, library: Optional[MiniGPT4SharedLibrary] = None,
                 n_ctx: int = 2048, n_batch: int = 512, seed: int = 1337):
        self.library = library or load_library()
        self.ctx = self.library.minigpt4_model_load(model_path, llm_model_path, int(verbosity), seed=seed, n_ctx=n_ctx, n_batch=n_batch)
        self.n_threads = n_threads
        self.embedding: Optional[MiniGPT4Embedding] = None
        self.is_image_uploaded = False

    def free(self):
        if self.ctx is not None and self.ctx.ptr:
            self.library.minigpt4_free(self.ctx)

    def generate(self, message: str, limit: int = 1024, temp: float = 0.8, top_k: int = 40, top_p: float = 0.9, tfs_z: float = 1.0, typical_p: float = 1.0,
                 repeat_last_n: int = 64, repeat_penalty: float = 1.1, alpha_presence: float = 1.0, alpha_frequency: float = 1.0, mirostat: int = 0,
                 mirostat_tau: float = 5.0, mirostat_eta: float = 1.0, penalize_nl: int = 1, ignore_eos: bool = False) -> Iterator[str]:
        if self.is_image_uploaded:
            self.library.minigpt4_begin_chat_image(self.ctx, self.embedding, message, self.n_threads)
            self.is_image_uploaded = False
        else:
            self.library.minigpt4_begin_chat(self.ctx, message, self.n_threads)
        chat = ""
        for _ in range(limit):
            token = self.library.minigpt4_end_chat_image(self.ctx, self.n_threads, temp, top_k, top_p, tfs_z, typical_p, repeat_last_n, repeat_penalty,
                                                          alpha_presence, alpha_frequency, mirostat, mirostat_tau, mirostat_eta, penalize_nl)
            chat += token
            if not ignore_eos:
                if self.library.minigpt4_contains_eos_token(token):
                    continue
                if self.library.minigpt4_is_eos(chat):
                    break
            yield token

    def reset_chat(self):
        self.is_image_uploaded = False
        if self.embedding is not None:
            self.library.minigpt4_free_embedding(self.embedding)
            self.embedding = None
        self.library.minigpt4_reset_chat(self.ctx)
        self.library.minigpt4_system_prompt(self.ctx, self.n_threads)

    def upload_image(self, image):
        """image: a preprocessed f32 [3][224][224] array, a file path / encoded bytes (decoded and preprocessed by the library itself:
        minigpt4_image_load_from_file + minigpt4_preprocess_image, the reference's `test_native_image_implementation` path, minigpt4_library.py:722-724),
        or a PIL image (the reference's torchvision-style path, via Pillow)."""
        self.reset_chat()
        if isinstance(image, (str, bytes, bytearray)):
            raw = self.library.amd_decode_image(bytes(image)) if not isinstance(image, str) else self.library.minigpt4_image_load_from_file(self.ctx, image)
            pre = None
            try:
                pre = self.library.minigpt4_preprocess_image(self.ctx, raw)
                self.embedding = self.library.minigpt4_encode_image(self.ctx, pre, self.n_threads)
            finally:
                self.library.minigpt4_free_image(raw)
                if pre is not None:
                    self.library.minigpt4_free_image(pre)
        else:
            chw = image if isinstance(image, np.ndarray) else image_to_array(image)
            self.embedding = self.library.minigpt4_encode_image(self.ctx, array_to_image_struct(chw), self.n_threads)
        self.is_image_uploaded = True
