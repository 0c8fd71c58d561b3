"""Modulus switching, level-aware decryption and the level-aware wire entries on the gfx950 kernels: the calls of
tests/test_mod_switch_emu.py through mod_switch_common, and the deployed parameters (BFVDefault(16384), L = 8)."""
import pytest

import mod_switch_common as ms
import parity_common as pc
from test_mod_switch_emu import KEYLESS_LEVEL_20_50_50, keyless_small_q0, make

# the lowest level at which the product of the keyless flow still has noise budget at BFVDefault(16384), t = 65537.  Computed on the
# CPU (the same flow on the tests-only emulator; the keys and ciphertexts come from the same seeds, word for word): budget per level
# {8: 332, 7: 316, 6: 267, 5: 218, 4: 169, 3: 120, 2: 72, 1: 24}
KEYLESS_LEVEL_N16384 = 1


@pytest.fixture(scope="module")
def mem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pc.TorchMem("cuda:0")


@pytest.fixture(scope="module")
def lib(api):
    lib = api.load_library()
    assert lib.hhe_backend() == b"hip-gfx950"
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ms.WORD_SHAPES)
def test_gpu_words_against_definition(orc, api, lib, mem, shape):
    X, O = make(orc, api, lib, shape)
    ms.check_words(X, O, mem, sizes=ms.sizes_of(shape))


@pytest.mark.gpu
def test_gpu_words_against_definition_deployed(orc, api, lib, mem):
    X, O = make(orc, api, lib, "n16384_default")
    ms.check_words(X, O, mem, B=2)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["n1024_mixed", "n1024_10x50"])
def test_gpu_composition(orc, api, lib, mem, shape):
    X, O = make(orc, api, lib, shape)
    ms.check_composition(X, O, mem)


@pytest.mark.gpu
def test_gpu_refusals(orc, api, lib, mem):
    X, O = make(orc, api, lib, "n1024_3x50")
    ms.check_refusals(X, O, mem, api)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(ms.MEANING))
def test_gpu_meaning(orc, api, lib, mem, case):
    logn, bits, t, levels = ms.MEANING[case]
    q = orc.coeff_modulus_create(1 << logn, bits)
    X, O = api.Context(logn, q, t, lib=lib), orc.Oracle(logn, q, t)
    ms.check_meaning(X, O, orc, mem, levels)


@pytest.mark.gpu
def test_gpu_meaning_deployed(orc, api, lib, mem):
    X, O = make(orc, api, lib, "n16384_default")
    ms.check_meaning(X, O, orc, mem, (1,), nb=1)


@pytest.mark.gpu
def test_gpu_keyless_flow_deployed(orc, api, lib, mem):
    X, O = make(orc, api, lib, "n16384_default")
    ms.check_keyless_flow(X, O, orc, mem, KEYLESS_LEVEL_N16384)


@pytest.mark.gpu
def test_gpu_keyless_flow_stops_above_the_last_level(orc, api, lib, mem):
    X, O = keyless_small_q0(orc, api, lib)
    ms.check_keyless_flow(X, O, orc, mem, KEYLESS_LEVEL_20_50_50)


@pytest.mark.gpu
def test_gpu_wire(orc, api, lib, mem):
    X, O = make(orc, api, lib, "n1024_mixed")
    ms.check_wire(X, O, mem, api)
