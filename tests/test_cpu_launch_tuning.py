"""launch_tuning_from_env (csrc/engine.cpp): the launch tuning a context gets at load -- the defaults of struct LaunchTuning (csrc/kernels.hpp), the CU count it is
handed and the five environment switches, each normalised in LaunchTuning::normalised().  Host only: no device is touched."""
import ctypes

import pytest

FIELDS = ("cus", "mv_waves_per_cu", "mmq", "mmqh", "mmq_ks", "mmq3_waves", "attn_prefill_w8", "attn_prefill_f16", "attn_prefill_form", "gemm_arm", "gemm_sk_arm",
          "f16_ks", "splitk_xcd", "attn_vit_qt")                    # the order include/minigpt4_amd_test.h documents
DEFAULTS = dict(cus=256, mv_waves_per_cu=0, mmq=2, mmqh=0, mmq_ks=0, mmq3_waves=8, attn_prefill_w8=1, attn_prefill_f16=1, attn_prefill_form=0, gemm_arm=0, gemm_sk_arm=0,
                f16_ks=0, splitk_xcd=1, attn_vit_qt=0)
SWITCHES = {"MINIGPT4_ATTN_PREFILL_W8": "attn_prefill_w8", "MINIGPT4_MMQH": "mmqh", "MINIGPT4_ATTN_QT": "attn_vit_qt", "MINIGPT4_SPLITK_XCD": "splitk_xcd",
            "MINIGPT4_F16_KS": "f16_ks"}


def tuning_from_env(lib, cus=256):
    f = lib.library.minigpt4_amd_test_tuning_from_env
    f.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    f.restype = ctypes.c_int
    out = (ctypes.c_int * len(FIELDS))()
    assert f(cus, out, len(FIELDS)) == len(FIELDS)
    return dict(zip(FIELDS, out))


@pytest.fixture
def clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_defaults_with_the_five_switches_unset(lib, clean_env):
    assert tuning_from_env(lib) == DEFAULTS
    assert set(DEFAULTS) == set(FIELDS)


def test_cus_is_passed_through(lib, clean_env):
    for cus in (1, 104, 256, 304):
        assert tuning_from_env(lib, cus) == dict(DEFAULTS, cus=cus)


@pytest.mark.parametrize("var,value,want", [("MINIGPT4_ATTN_PREFILL_W8", "0", 0), ("MINIGPT4_MMQH", "1", 1), ("MINIGPT4_ATTN_QT", "2", 2), ("MINIGPT4_SPLITK_XCD", "0", 0),
                                            ("MINIGPT4_F16_KS", "3", 3)])
def test_each_switch_alone_changes_only_its_own_field(lib, clean_env, var, value, want):
    clean_env.setenv(var, value)
    assert tuning_from_env(lib) == dict(DEFAULTS, **{SWITCHES[var]: want})
    clean_env.delenv(var)
    assert tuning_from_env(lib) == DEFAULTS                       # nothing sticks: read again, the default is back


@pytest.mark.parametrize("var,value,want", [("MINIGPT4_F16_KS", "99", 8), ("MINIGPT4_F16_KS", "-3", 0), ("MINIGPT4_F16_KS", "8", 8), ("MINIGPT4_ATTN_QT", "-1", 0),
                                            ("MINIGPT4_SPLITK_XCD", "7", 1), ("MINIGPT4_SPLITK_XCD", "-1", 1), ("MINIGPT4_ATTN_PREFILL_W8", "5", 1),
                                            ("MINIGPT4_MMQH", "-2", 1), ("MINIGPT4_MMQH", "0", 0)])
def test_clamps(lib, clean_env, var, value, want):
    clean_env.setenv(var, value)
    assert tuning_from_env(lib) == dict(DEFAULTS, **{SWITCHES[var]: want})


def test_all_five_together_and_a_short_buffer(lib, clean_env):
    for var, value in (("MINIGPT4_ATTN_PREFILL_W8", "0"), ("MINIGPT4_SPLITK_XCD", "0"), ("MINIGPT4_ATTN_QT", "2"), ("MINIGPT4_F16_KS", "2"), ("MINIGPT4_MMQH", "1")):
        clean_env.setenv(var, value)
    assert tuning_from_env(lib, 64) == dict(DEFAULTS, cus=64, attn_prefill_w8=0, splitk_xcd=0, attn_vit_qt=2, f16_ks=2, mmqh=1)
    f = lib.library.minigpt4_amd_test_tuning_from_env
    out = (ctypes.c_int * 4)(-7, -7, -7, -7)
    assert f(64, out, 3) == 3 and list(out) == [64, 0, 2, -7]      # writes no more than it is given room for
    assert f(64, None, 3) == -1
