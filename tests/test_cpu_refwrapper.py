"""Boundary, CPU side (round-1 verdict item 8): the reference's UNMODIFIED ctypes declarations against libminigpt4.so, as far as a box without a GPU
gets (every declaration binds, the model-load call the reference's MiniGPT4ChatBot makes is marshalled and fails where the reference would fail on a
missing model), and the honesty check of the restated ABI table the GPU-side test binds through.  What the reference's binding declares is recorded in
tests/golden/reference_binding.json (ctypes type names; tests/golden/make_reference_binding.py regenerates it from a reference checkout)."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "minigpt4.cpp_amd", "libminigpt4.so")
REF = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_binding.json")))


def _name(t):
    return None if t is None else t.__name__


def test_restated_abi_table_equals_the_reference_declarations(lib):
    import ref_abi
    decl = REF["declarations"]
    assert sorted(decl) == sorted(ref_abi.ABI)
    bound = ref_abi.bind(SO)
    for name, (args, res) in ref_abi.ABI.items():
        fn = getattr(bound, name)
        assert [_name(a) for a in fn.argtypes] == decl[name]["argtypes"], name
        assert _name(fn.restype) == decl[name]["restype"], name
    for s in (ref_abi.MiniGPT4Image, ref_abi.MiniGPT4Embedding):
        want = REF["structs"][s.__name__]
        assert ctypes.sizeof(s) == want["size"]
        assert [[f[0], _name(f[1])] for f in s._fields_] == want["fields"]
    assert ctypes.sizeof(ref_abi.MiniGPT4Image) == 24 and ctypes.sizeof(ref_abi.MiniGPT4Embedding) == 16


def test_reference_chatbot_constructor_marshals_model_load(lib, tiny_files):
    """`MiniGPT4ChatBot(model, llm)` of the reference: minigpt4_model_load through ITS argtypes, with the verbosity the constructor passes and the defaults of
    its wrapper (seed, n_ctx, n_batch, numa -- in the wrapper's argument order).  Without a GPU the engine refuses to load (no CPU fallback) and returns NULL
    exactly like the reference on a load failure, which the reference's wrapper turns into its own AssertionError."""
    if lib.amd_device_count() > 0:
        pytest.skip("a GPU is visible: the GPU suite runs the whole flow")
    import ref_abi
    w = ref_abi.bind(SO)
    vp, llm = tiny_files
    d = REF["model_load_defaults"]
    assert REF["chatbot_defaults"]["verbosity"] == REF["verbosity"]["SILENT"]
    args = [ref_abi.cstr(vp), ref_abi.cstr(llm("q4_0"))] + [ref_abi.I32(v) for v in (REF["chatbot_defaults"]["verbosity"], d["seed"], d["n_ctx"], d["n_batch"], d["numa"])]
    assert w.minigpt4_model_load(*args) is None
    # the calls that need no context, through the reference's declarations
    assert w.minigpt4_contains_eos_token(ref_abi.cstr("##")) and not w.minigpt4_contains_eos_token(ref_abi.cstr("#"))
    assert w.minigpt4_is_eos(ref_abi.cstr("xyz###")) and not w.minigpt4_is_eos(ref_abi.cstr("xyz##"))
    w.minigpt4_set_verbosity(ref_abi.I32(REF["verbosity"]["ERR"]))
    assert w.minigpt4_model_load(ref_abi.cstr("/nonexistent/a.bin"), ref_abi.cstr("/nonexistent/b.bin"),
                                 *[ref_abi.I32(d[k]) for k in ("verbosity", "seed", "n_ctx", "n_batch", "numa")]) is None
