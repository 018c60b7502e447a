"""Shared by tests/test_cpu_activations.py and tests/test_gpu_activations.py: the contract of the COMPUTED exp / SiLU / GELU forms (csrc/activations.hpp) against ggml's fp16
tables, fp16 distances in ordered-integer form, numpy models of the device formulas and of ggml's table formulas, and the observation record.

The contract (the project's own statement of the deviation): on every finite fp16 argument the computed value is within ONE fp16 ulp of the table's entry; at most
SHARE_CAP = 1e-3 of the finite arguments (63 of 63 488) differ at all; +-0, +-inf and NaN come out as the table has them."""
import numpy as np

GELU, SILU, EXP = 0, 1, 2                     # oracle/refcpu.c orc_table numbering = minigpt4_amd_test_activation's `which`
NAMES = {GELU: "gelu", SILU: "silu", EXP: "exp"}
BITS = np.arange(65536, dtype=np.uint32).astype(np.uint16)
ARGS = BITS.view(np.float16)
FINITE = (BITS & 0x7C00) != 0x7C00            # exponent field not all ones
NAN = ((BITS & 0x7C00) == 0x7C00) & ((BITS & 0x03FF) != 0)
N_FINITE = int(FINITE.sum())
assert N_FINITE == 63488
MAX_ULP = 1
SHARE_CAP = 1e-3
MAX_DIFFERENT = int(SHARE_CAP * N_FINITE)      # 63
P_INF, N_INF, N_MAX = 0x7C00, 0xFC00, 0xFBFF   # +inf, -inf, -65504


def is_nan(bits):
    bits = np.asarray(bits, np.uint16)
    return ((bits & 0x7C00) == 0x7C00) & ((bits & 0x03FF) != 0)


def ordered(bits):
    """fp16 bit patterns -> integers whose differences count representable values in between (+0 and -0 both 0, subnormals one step apart)."""
    b = np.asarray(bits, np.uint16).astype(np.int32)
    m = b & 0x7FFF
    return np.where(b & 0x8000, -m, m)


def deviation(got, table):
    """{count, max_ulp, patterns} of the finite arguments whose result is not the table's entry (patterns: argument bit patterns, hex)."""
    got, table = np.asarray(got, np.uint16), np.asarray(table, np.uint16)
    diff = FINITE & (got != table)
    nan_mismatch = diff & (is_nan(got) | is_nan(table))
    d = np.abs(ordered(got) - ordered(table))
    return {"count": int(diff.sum()), "max_ulp": int(d[diff & ~nan_mismatch].max()) if (diff & ~nan_mismatch).any() else 0, "nan_mismatches": int(nan_mismatch.sum()),
            "patterns": ["0x%04x" % int(b) for b in BITS[diff]]}


def assert_table_sanity(which, table):
    """What the issue states about the tables themselves (a wrong table would make every comparison below meaningless)."""
    t = np.asarray(table, np.uint16)
    assert t[P_INF] == P_INF, hex(int(t[P_INF]))
    if which == EXP:
        assert t[N_INF] == 0x0000
        assert (t[(ARGS.astype(np.float32) >= 11.1) & FINITE] == P_INF).all()     # fp16(expf(x)) overflows from x = 11.09 upwards
    else:
        assert is_nan(t[N_INF])
        assert t[N_MAX] == 0x8000                                                 # -65504 * 0 = -0
    assert is_nan(t[NAN]).all()


def assert_computed_contract(which, got, table):
    """The hard bound, the zero signs, the infinities, the NaNs and the share cap; returns deviation(got, table)."""
    got, table = np.asarray(got, np.uint16), np.asarray(table, np.uint16)
    name = NAMES[which]
    dev = deviation(got, table)
    print(f"{name}: {dev['count']} of {N_FINITE} finite arguments differ from the table, max {dev['max_ulp']} fp16 ulp, {dev['nan_mismatches']} NaN mismatches; {dev['patterns'][:24]}")
    assert dev["nan_mismatches"] == 0, (name, dev)                               # a finite argument gives NaN exactly where the table does (nowhere)
    assert dev["max_ulp"] <= MAX_ULP, (name, dev["count"], dev["max_ulp"], dev["patterns"][:32])
    zz = FINITE & ((got & 0x7FFF) == 0) & ((table & 0x7FFF) == 0)
    assert np.array_equal(got[zz], table[zz]), (name, "sign of a zero result", ["0x%04x" % int(b) for b in BITS[zz][got[zz] != table[zz]]][:16])
    assert got[0x0000] == table[0x0000] and got[0x8000] == table[0x8000], (name, "f(+-0)", hex(int(got[0])), hex(int(got[0x8000])))
    for arg in (P_INF, N_INF):
        assert (is_nan(got[arg]) and is_nan(table[arg])) or got[arg] == table[arg], (name, hex(arg), hex(int(got[arg])), hex(int(table[arg])))
    assert got[P_INF] == P_INF, (name, hex(int(got[P_INF])))
    if which == EXP:
        assert got[N_INF] == 0x0000, hex(int(got[N_INF]))
    else:
        assert is_nan(got[N_INF]), (name, hex(int(got[N_INF])))
        assert got[N_MAX] == 0x8000, (name, hex(int(got[N_MAX])))
    assert is_nan(got[NAN]).all(), (name, "NaN arguments", int((~is_nan(got[NAN])).sum()))
    assert dev["count"] <= MAX_DIFFERENT, (name, dev["count"], MAX_DIFFERENT)
    return dev


# ---- numpy models: fp32 arithmetic step by step (the kernels are built with -ffp-contract=off), the exponential / tanh taken in float64 and rounded to fp32
F = np.float32
_C = F(0.79788456080286535587989211986876)


def _exp32(x):
    return np.exp(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def _h(y):
    return np.asarray(y, np.float32).astype(np.float16).view(np.uint16)


def device_exp(x):
    return _h(_exp32(x))


def device_silu(x):
    return _h(x / (F(1) + _exp32(-x)))


def _u(x):
    return _C * x * (F(1) + F(0.044715) * x * x)


def device_gelu(x):
    u = _u(x)
    th = np.copysign(F(1) - F(2) / (_exp32(F(2) * np.abs(u)) + F(1)), u)
    return _h(F(0.5) * x * (F(1) + th))


def device_gelu_one_sided(x):
    """The form shipped before this check existed: tanh(u) = 1 - 2 / (exp(2 u) + 1) for either sign of u."""
    th = F(1) - F(2) / (_exp32(F(2) * _u(x)) + F(1))
    return _h(F(0.5) * x * (F(1) + th))


def ggml_exp(x):
    return _h(_exp32(x))


def ggml_silu(x):
    return _h(x / (F(1) + _exp32(-x)))


def ggml_gelu(x):
    th = np.tanh(_u(x).astype(np.float64)).astype(np.float32)
    return _h(F(0.5) * x * (F(1) + th))


DEVICE_MODEL = {GELU: device_gelu, SILU: device_silu, EXP: device_exp}
GGML_MODEL = {GELU: ggml_gelu, SILU: ggml_silu, EXP: ggml_exp}


def evaluate(fn):
    with np.errstate(all="ignore"):
        return fn(ARGS.astype(np.float32))


_OBSERVED = {}


def record(section, name, dev):
    """What this run measured, kept where the other observation records go and by the same writer (test_gpu_headline._dump: parity_observed_activation_deviation.json, the
    whole record rewritten at every call); tests/golden/activation_deviation_observed.json is one GPU box's committed copy."""
    from test_gpu_headline import _dump
    _OBSERVED.setdefault(section, {})[name] = dev
    _dump("activation_deviation", _OBSERVED)
