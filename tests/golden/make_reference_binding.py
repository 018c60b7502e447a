#!/usr/bin/env python3
"""Generates tests/golden/reference_binding.json: what the reference's unmodified Python binding (`minigpt4/minigpt4_library.py` of a
minigpt4.cpp checkout) declares -- the ctypes argtypes / restype of every symbol it binds, the layout of its two structures, and the
defaults of `MiniGPT4SharedLibrary.minigpt4_model_load` / `MiniGPT4ChatBot.__init__` -- as ctypes type NAMES, so that the tests of the
drop-in boundary (tests/test_cpu_refwrapper.py, tests/test_cpu_host.py) run without a reference checkout.  Interface data only.

    python tests/golden/make_reference_binding.py <checkout>/minigpt4/minigpt4_library.py      (after build())
"""
import importlib.util
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "..", "..", "minigpt4.cpp_amd", "libminigpt4.so")


def tname(t):
    return None if t is None else t.__name__


def main(ref_path: str) -> None:
    spec = importlib.util.spec_from_file_location("ref_minigpt4_library", ref_path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = mod.MiniGPT4SharedLibrary(SO).library
    decl = {}
    for name, fn in sorted(vars(lib).items()):              # the symbols the wrapper's constructor looked up and declared
        if name.startswith("minigpt4_") and hasattr(fn, "argtypes"):
            decl[name] = {"argtypes": [tname(a) for a in (fn.argtypes or [])], "restype": tname(fn.restype)}
    structs = {s.__name__: {"size": __import__("ctypes").sizeof(s), "fields": [[f[0], tname(f[1])] for f in s._fields_]}
               for s in (mod.MiniGPT4Image, mod.MiniGPT4Embedding)}

    def defaults(f):
        return {k: (int(v.default) if isinstance(v.default, int) else v.default) for k, v in inspect.signature(f).parameters.items()
                if v.default is not inspect.Parameter.empty}
    out = {"source": "minigpt4/minigpt4_library.py of the reference checkout (unmodified)", "declarations": decl, "structs": structs,
           "model_load_defaults": defaults(mod.MiniGPT4SharedLibrary.minigpt4_model_load),
           "chatbot_defaults": defaults(mod.MiniGPT4ChatBot.__init__),
           "verbosity": {v.name: int(v) for v in mod.Verbosity}}
    dst = os.path.join(HERE, "reference_binding.json")
    json.dump(out, open(dst, "w"), indent=1, sort_keys=True)
    open(dst, "a").write("\n")
    print(f"wrote {dst}: {len(decl)} declarations")


if __name__ == "__main__":
    main(sys.argv[1])
