"""Modulus switching, level-aware decryption and the level-aware wire entries on the emulator (the shared kernel bodies behind the real
host driver); see mod_switch_common for the definition every word is compared with.  The GPU suite makes the same calls in
tests/test_gpu_mod_switch.py."""
import pytest

import mod_switch_common as ms
import parity_common as pc

# the lowest level at which the product of the keyless flow still has noise budget, N = 4096 over 4 x 50 bits.  Computed on the CPU:
# budget per level {3: 96, 2: 77, 1: 27}
KEYLESS_LEVEL_N4096 = 1


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


def make(orc, api, lib, name, t=ms.T16):
    logn, q = ms.shape_primes(orc, api, lib, name)
    return api.Context(logn, q, t, lib=lib), (orc.Oracle(logn, q, t) if len(q) <= 32 else ms.Shape(logn, q, t))


@pytest.mark.parametrize("shape", ms.WORD_SHAPES)
def test_words_against_definition(orc, api, emu_lib, mem, shape):
    X, O = make(orc, api, emu_lib, shape)
    ms.check_words(X, O, mem, sizes=ms.sizes_of(shape))


@pytest.mark.parametrize("shape", ["n1024_mixed", "n1024_10x50"])
def test_composition(orc, api, emu_lib, mem, shape):
    X, O = make(orc, api, emu_lib, shape)
    ms.check_composition(X, O, mem)


def test_refusals(orc, api, emu_lib, mem):
    X, O = make(orc, api, emu_lib, "n1024_3x50")
    ms.check_refusals(X, O, mem, api)


@pytest.mark.parametrize("case", list(ms.MEANING))
def test_meaning(orc, api, emu_lib, mem, case):
    logn, bits, t, levels = ms.MEANING[case]
    q = orc.coeff_modulus_create(1 << logn, bits)
    X, O = api.Context(logn, q, t, lib=emu_lib), orc.Oracle(logn, q, t)
    ms.check_meaning(X, O, orc, mem, levels)


def test_keyless_flow(orc, api, emu_lib, mem):
    q = orc.coeff_modulus_create(4096, [50] * 4)
    X, O = api.Context(12, q, ms.T16, lib=emu_lib), orc.Oracle(12, q, ms.T16)
    ms.check_keyless_flow(X, O, orc, mem, KEYLESS_LEVEL_N4096)


# ... and where the lowest level with budget is not the last one: N = 1024 over 20 + 50 + 50 (+ 50) bits, a 20-bit q_0 holds no result
# under t = 65537.  Computed on the CPU: budget per level {3: 69, 2: 48, 1: 0}
KEYLESS_LEVEL_20_50_50 = 2


def keyless_small_q0(orc, api, lib):
    q = orc.coeff_modulus_create(1024, [20, 50, 50, 50])
    return api.Context(10, q, ms.T16, lib=lib), orc.Oracle(10, q, ms.T16)


def test_keyless_flow_stops_above_the_last_level(orc, api, emu_lib, mem):
    X, O = keyless_small_q0(orc, api, emu_lib)
    ms.check_keyless_flow(X, O, orc, mem, KEYLESS_LEVEL_20_50_50)


def test_wire(orc, api, emu_lib, mem):
    X, O = make(orc, api, emu_lib, "n1024_mixed")
    ms.check_wire(X, O, mem, api)
