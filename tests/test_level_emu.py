"""Evaluation below the data level on the emulator (the shared kernel bodies behind the real host driver, range check on): the
context of a level, key sets derived on the device, and every op at the level against the oracle of the shortened chain; see
level_common.  The GPU suite makes the same calls in tests/test_gpu_level.py, where a shape is sent only after it passed here."""
import pytest

import level_common as lc
import parity_common as pc

# the lowest level at which rotate + multiply_plain + add on the switched product of the keyless flow still has noise budget,
# N = 4096 over 4 x 50 bits, t = 65537.  Computed on the CPU with the short-chain oracle: budget per level {3: 76, 2: 53, 1: 4}
KEYLESS_LEVEL_N4096 = 1
# ... and where that level is not the last one: N = 1024 over 20 + 50 + 50 (+ 50) bits, a 20-bit q_0 holds no result under t = 65537.
# Computed the same way: budget per level {3: 50, 2: 26, 1: 0}
KEYLESS_LEVEL_20_50_50 = 2


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


def parent(orc, api, lib, chain):
    S = lc.parent_setup(orc, chain)
    return api.Context(S.logn, S.q, S.t, lib=lib), S


@pytest.mark.parametrize("chain,l", lc.EMU_CASES)
def test_level_context_constants(orc, api, emu_lib, chain, l):
    X, S = parent(orc, api, emu_lib, chain)
    lc.check_context(X, S, orc, api, l)


def test_level_context_refusals(orc, api, emu_lib):
    X, S = parent(orc, api, emu_lib, "n1024_4x50")
    lc.check_context_refusals(X, api)


@pytest.mark.parametrize("chain", list(lc.CHAINS))
def test_derivation_of_uploaded_keys(orc, api, emu_lib, chain):
    X, S = parent(orc, api, emu_lib, chain)
    lc.check_derivation_uploaded(X, S, orc, api, lc.CHAINS[chain][2])


@pytest.mark.parametrize("chain,l", [("n1024_4x50", 2), ("n1024_4x50", 1), ("n1024_mixed", 3)])
def test_derivation_refusals(orc, api, emu_lib, chain, l):
    X, S = parent(orc, api, emu_lib, chain)
    lc.check_derivation_refusals(X, S, orc, api, l)


def test_derivation_and_kept_keystreams(orc, api, emu_lib, mem):
    X, S = parent(orc, api, emu_lib, "n1024_10x50")
    lc.check_derivation_keeps_keystreams(X, S, orc, api, mem, 8)


@pytest.mark.parametrize("chain", ["n1024_4x50", "n4096_4x60"])
def test_derivation_of_generated_keys(orc, api, emu_lib, mem, chain):
    X, S = parent(orc, api, emu_lib, chain)
    lc.check_derivation_generated(X, S, orc, api, mem, lc.CHAINS[chain][2])


@pytest.mark.parametrize("chain,l", [("n1024_4x50", 2), ("n1024_4x50", 1), ("n1024_mixed", 2), ("n4096_4x60", 1)])
def test_key_switch_of_a_derived_key_against_the_definition(orc, api, emu_lib, mem, chain, l):
    X, S = parent(orc, api, emu_lib, chain)
    lc.check_definition(X, S, orc, mem, l)


@pytest.mark.parametrize("chain,l", lc.EMU_CASES)
def test_evaluation_at_the_level(orc, api, emu_lib, mem, chain, l):
    X, S = parent(orc, api, emu_lib, chain)
    lc.check_eval(X, S, orc, api, mem, l, lc.CHAINS[chain][3][l], lc.CHAINS[chain][4][l])


@pytest.mark.parametrize("chain,l", [("n1024_4x50", 1), ("n4096_4x60", 2), ("n4096_4x60", 1), ("n1024_mixed", 2)])
def test_fc_variants_and_chain_at_the_level(orc, api, emu_lib, mem, monkeypatch, chain, l):
    X, S = parent(orc, api, emu_lib, chain)
    Sl = lc.level_setup(orc, api, S, l)
    pc.check_fc_variants(lambda: X.at_level(l), Sl, orc, mem, monkeypatch, n_in=9)
    Xl = X.at_level(l)
    Sl.load_keys(Xl)
    pc.check_two_layer_chain(Xl, Sl, mem, n_in=8)


@pytest.mark.parametrize("l", [9, 8])
def test_noise_budget_forms_from_a_level_context(orc, api, emu_lib, mem, l):
    X, S = parent(orc, api, emu_lib, "n1024_10x50")
    lc.check_noise_form(X, S, orc, api, mem, l)


def test_keyless_flow_at_a_level(orc, api, emu_lib, mem):
    q = orc.coeff_modulus_create(4096, [50] * 4)
    X, O = api.Context(12, q, lc.T16, lib=emu_lib), orc.Oracle(12, q, lc.T16)
    lc.check_keyless_level(X, O, orc, api, mem, KEYLESS_LEVEL_N4096)


def keyless_small_q0(orc, api, lib):
    q = orc.coeff_modulus_create(1024, [20, 50, 50, 50])
    return api.Context(10, q, lc.T16, lib=lib), orc.Oracle(10, q, lc.T16)


def test_keyless_flow_at_a_level_above_the_last(orc, api, emu_lib, mem):
    X, O = keyless_small_q0(orc, api, emu_lib)
    lc.check_keyless_level(X, O, orc, api, mem, KEYLESS_LEVEL_20_50_50)
