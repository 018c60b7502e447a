"""The case list of tests/test_gpu_lora_group.py discriminates, shown on the float64 reference alone (tests/lora_ref.py): every mistake of the kinds lora_ref.MUTANTS
names that changes a case's result at all moves at least half of the outputs it changes by more than 4 x the bound the GPU test holds the kernels to.  No GPU."""
import functools

import numpy as np
import pytest

import lora_ref as L


def _variants(c, mutant):
    if mutant in ("t_slab", "ssq_slab"):
        return range(L.n_slabs(c["n_in"], c["form"]))
    return (0,)


@functools.lru_cache(maxsize=None)
def _applied(name):
    """The mutants that change the case's result, each checked against the bound; computed once per case for both tests that need it."""
    spec = L.SPECS[L.IDS.index(name)]
    c = L.make_case(spec)
    want, bound, live = L.group_ref(c)
    y0 = c["y0"].astype(np.float64)
    assert np.array_equal(want[~live], y0[~live]) and not live[:, :, c["n_out"]:].any()
    assert live.any() or name.startswith("slot0_none")
    # the inputs are coherent (lora_ref.py): the term IS the sum of the absolute values of its products, so the bound is a small fraction of the term, and |y0| >= 0.5 outweighs it
    assert float((4 * bound[live]).max(initial=0.0)) < 0.5 <= float(np.abs(y0).min())
    applied = []
    for mutant in L.MUTANTS:
        for which in _variants(c, mutant):
            got, _, _ = L.group_ref(c, mutant, which)
            diff = np.abs(got - want)
            changed = diff > 1e-12 * np.maximum(1.0, np.abs(want))
            if mutant in ("t_slab", "store"):                       # these two change every output that holds a non-zero term / every live output
                assert np.array_equal(changed, (want != y0) if mutant == "t_slab" else live), (name, mutant, which)
            if not changed.any():
                continue
            outside = float((diff[changed] > 4 * bound[changed]).mean())
            assert outside >= 0.5, (name, mutant, which, outside)
            applied.append(mutant)
    return frozenset(applied)


@pytest.mark.parametrize("name", L.IDS)
def test_mutants_leave_the_bound(name):
    _applied(name)


@pytest.mark.parametrize("spec", [s for s in L.SPECS if s["n_targets"] > 1 and s["form"] == 2 and s["n_in"] <= 264], ids=lambda s: s["name"])
def test_one_target_at_a_time_agrees_with_the_joined_call(spec):
    c = L.make_case(spec)
    want, bound, live = L.group_ref(c)
    for m in range(c["n_targets"]):
        w1, b1, l1 = L.group_ref(L.one_target(c, m))
        assert np.array_equal(l1[0], live[m])
        np.testing.assert_allclose(w1[0], want[m], rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(b1[0], bound[m], rtol=1e-12)


def test_the_list_reaches_the_named_paths():
    """What the kernels' code branches on, counted over the list: slabs per form and mode, joined widths, adapters of unequal width, row tiles, plumbing, output widths."""
    S = L.SPECS
    ks = lambda s: L.n_slabs(s["n_in"], s["form"])
    rcat = lambda s: max(L.concat_layout(m, L.rank_padded(r))[1] for r, m in s["adapters"])
    for form in (1, 2):
        for mode in (0, 1, 2):
            assert {ks(s) for s in S if s["form"] == form and s["mode"] == mode} >= {1, 2, 3}, (form, mode)
        assert any(rcat(s) == 192 for s in S if s["form"] == form)                                        # blockIdx.z = 2 of k_lora_down, u = 1 of k_lora_down_mfma
        assert any(len({L.rank_padded(r) for r, m in s["adapters"] if m}) == 3 for s in S if s["form"] == form)
        assert any(m == 0b101 for s in S if s["form"] == form for _, m in s["adapters"])
        assert any(s["stride"] == 2 for s in S if s["form"] == form) and any(isinstance(s["rowmap"], tuple) for s in S if s["form"] == form)
        assert any(s["rowmap"] == "group" for s in S if s["form"] == form) and any(s["pad"] == 24 for s in S if s["form"] == form)
        assert {s["n_out"] for s in S if s["form"] == form} == {100, 260}
    assert {s["n_in"] for s in S if s["form"] == 1} >= {512, 520, 1032} and {s["n_in"] for s in S if s["form"] == 2} >= {72, 2048, 2056, 4104}
    assert {s["rows"] for s in S if s["form"] == 2} >= {32, 64, 65, 100} and {s["rows"] for s in S if s["form"] == 1} >= {1, 3}
    assert any(s["rowmap"] == "tile" and s["rows"] == 100 for s in S if s["form"] == 2)
    assert 45 <= len(S) <= 60


@pytest.mark.parametrize("what", ["n_in", "ldy", "rank", "no_target", "mask", "slot_adapter", "skipped_row_slot", "stride", "slot0", "rows", "second", "form"])
def test_the_hook_refuses_bad_arguments(lib, what):
    """minigpt4_amd_test_lora_group answers 1 before it looks for a device: nothing out of range reaches a kernel (a skipped row_slot entry included)."""
    c = L.make_case(L.SPECS[L.IDS.index("stride2-rms-vector")])
    if what == "n_in":
        c["x"] = c["x"][:, :12]
    elif what == "ldy":
        c["y0"] = c["y0"][:, :, :c["n_out"] - 1]
    elif what == "rank":
        c["adapters"] = [dict(c["adapters"][0], rank=65, A={m: np.zeros((65, c["n_in"]), np.float16) for m in (0, 1)}, B={m: np.zeros((c["n_out"], 65), np.float16) for m in (0, 1)})]
    elif what == "no_target":
        c["adapters"] = [dict(c["adapters"][0], mask=0)]
    elif what == "mask":
        c["adapters"] = [dict(c["adapters"][0], mask=0b111, A={m: c["adapters"][0]["A"][0] for m in range(3)}, B={m: c["adapters"][0]["B"][0] for m in range(3)})]
    elif what == "slot_adapter":
        c["slot_adapter"] = np.array([0, 2, -1, 0], np.int32)
    elif what == "skipped_row_slot":
        c["row_slot"] = c["row_slot"].copy()
        c["row_slot"][1] = 4
    elif what == "stride":
        c["stride"], c["row_slot"] = 0, c["row_slot"][:0]
    elif what == "slot0":
        c["row_slot"], c["slot0"] = None, 4
    elif what == "rows":
        c["x"], c["y0"], c["row_slot"] = np.zeros((513, c["n_in"]), np.float32), np.zeros((2, 513, c["ldy"]), np.float32), np.zeros(1026, np.int32)
    elif what == "second":
        c["second"] = None
    with pytest.raises(RuntimeError, match="rc=1"):
        lib.test_lora_group(c["x"], c["second"], c["n_out"], c["adapters"], c["slot_adapter"], c["slot_scale"], c["row_slot"], c["stride"], c["slot0"], c["y0"], c["mode"],
                            3 if what == "form" else c["form"])


def test_every_mutant_applies_somewhere():
    """Each kind of mistake changes the result of some case under either form, and a dropped slab that of every multi-slab case."""
    for mutant in L.MUTANTS:
        names = [n for n in L.IDS if mutant in _applied(n)]
        assert any(n.endswith("vector") for n in names) and any(n.endswith("mfma") for n in names), (mutant, names)
