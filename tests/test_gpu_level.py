"""Evaluation below the data level on the gfx950 kernels: the calls of tests/test_level_emu.py through level_common (a shape is
listed here once its emulator twin passed), and the shapes only the GPU runs: BFVDefault(4096) at level 1 (the separate-kernel path
with K = 2), the deployed BFVDefault(16384) at levels 4 and 1, and N = 2^15 over 4 x 60 bits at level 1."""
import pytest

import level_common as lc
import parity_common as pc
from test_level_emu import KEYLESS_LEVEL_20_50_50, KEYLESS_LEVEL_N4096, keyless_small_q0, parent

# the lowest level at which the keyless flow at a level still has noise budget at BFVDefault(16384), t = 65537.  Computed on the CPU
# (the same flow on the tests-only emulator with the short-chain oracle; keys and ciphertexts come from the same seeds, word for word):
# budget per level {8: 311, 7: 291, 6: 242, 5: 193, 4: 144, 3: 96, 2: 48, 1: 1}
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
@pytest.mark.parametrize("chain,l", lc.EMU_CASES)
def test_gpu_level_context_constants(orc, api, lib, chain, l):
    X, S = parent(orc, api, lib, chain)
    lc.check_context(X, S, orc, api, l)


@pytest.mark.gpu
def test_gpu_level_context_refusals(orc, api, lib):
    X, S = parent(orc, api, lib, "n1024_4x50")
    lc.check_context_refusals(X, api)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", list(lc.CHAINS))
def test_gpu_derivation_of_uploaded_keys(orc, api, lib, chain):
    X, S = parent(orc, api, lib, chain)
    lc.check_derivation_uploaded(X, S, orc, api, lc.CHAINS[chain][2])


@pytest.mark.gpu
@pytest.mark.parametrize("chain,l", [("n1024_4x50", 2), ("n1024_4x50", 1), ("n1024_mixed", 3)])
def test_gpu_derivation_refusals(orc, api, lib, chain, l):
    X, S = parent(orc, api, lib, chain)
    lc.check_derivation_refusals(X, S, orc, api, l)


@pytest.mark.gpu
def test_gpu_derivation_and_kept_keystreams(orc, api, lib, mem):
    X, S = parent(orc, api, lib, "n1024_10x50")
    lc.check_derivation_keeps_keystreams(X, S, orc, api, mem, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", ["n1024_4x50", "n4096_4x60"])
def test_gpu_derivation_of_generated_keys(orc, api, lib, mem, chain):
    X, S = parent(orc, api, lib, chain)
    lc.check_derivation_generated(X, S, orc, api, mem, lc.CHAINS[chain][2])


@pytest.mark.gpu
@pytest.mark.parametrize("chain,l", [("n1024_4x50", 2), ("n1024_4x50", 1), ("n1024_mixed", 2), ("n4096_4x60", 1)])
def test_gpu_key_switch_of_a_derived_key_against_the_definition(orc, api, lib, mem, chain, l):
    X, S = parent(orc, api, lib, chain)
    lc.check_definition(X, S, orc, mem, l)


@pytest.mark.gpu
@pytest.mark.parametrize("chain,l", lc.EMU_CASES)
def test_gpu_evaluation_at_the_level(orc, api, lib, mem, chain, l):
    X, S = parent(orc, api, lib, chain)
    lc.check_eval(X, S, orc, api, mem, l, lc.CHAINS[chain][3][l], lc.CHAINS[chain][4][l])


@pytest.mark.gpu
@pytest.mark.parametrize("chain,l", [("n1024_4x50", 1), ("n4096_4x60", 2), ("n4096_4x60", 1), ("n1024_mixed", 2)])
def test_gpu_fc_variants_and_chain_at_the_level(orc, api, lib, mem, monkeypatch, chain, l):
    X, S = parent(orc, api, lib, chain)
    Sl = lc.level_setup(orc, api, S, l)
    pc.check_fc_variants(lambda: X.at_level(l), Sl, orc, mem, monkeypatch, n_in=9)
    Xl = X.at_level(l)
    Sl.load_keys(Xl)
    pc.check_two_layer_chain(Xl, Sl, mem, n_in=8)


@pytest.mark.gpu
@pytest.mark.parametrize("l", [9, 8])
def test_gpu_noise_budget_forms_from_a_level_context(orc, api, lib, mem, l):
    X, S = parent(orc, api, lib, "n1024_10x50")
    lc.check_noise_form(X, S, orc, api, mem, l)


@pytest.mark.gpu
def test_gpu_keyless_flow_at_a_level(orc, api, lib, mem):
    q = orc.coeff_modulus_create(4096, [50] * 4)
    X, O = api.Context(12, q, lc.T16, lib=lib), orc.Oracle(12, q, lc.T16)
    lc.check_keyless_level(X, O, orc, api, mem, KEYLESS_LEVEL_N4096)


@pytest.mark.gpu
def test_gpu_keyless_flow_at_a_level_above_the_last(orc, api, lib, mem):
    X, O = keyless_small_q0(orc, api, lib)
    lc.check_keyless_level(X, O, orc, api, mem, KEYLESS_LEVEL_20_50_50)


# ---- the shapes only the GPU runs ----
@pytest.mark.gpu
def test_gpu_bfv_default_4096_at_level_1(orc, api, lib, mem):
    """36 + 36 + 37 bits: no pseudo-Mersenne form, the separate-kernel key switch at K = 2"""
    S = lc.parent_setup(orc, "bfv_default_4096", 12, api.bfv_default_coeff_modulus(4096, lib))
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    assert X.query("row_kernel") == 0
    lc.check_eval(X, S, orc, api, mem, 1, 0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("l", [4, 1])
def test_gpu_deployed_parameters_at_a_level(orc, api, lib, mem, l):
    """BFVDefault(16384), L = 8, at levels 4 and 1: an FC row of 37 inputs and an affine layer of dim 16 among the ops"""
    S = lc.parent_setup(orc, "bfv_default_16384", 14, pc.BFV_DEFAULT_16384)
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    assert X.query("row_kernel") == 1
    lc.check_eval(X, S, orc, api, mem, l, 1, 0, n_in=37, dim=16, every_key=False)


@pytest.mark.gpu
def test_gpu_keyless_flow_at_a_level_deployed(orc, api, lib, mem):
    q = pc.BFV_DEFAULT_16384
    X, O = api.Context(14, q, lc.T16, lib=lib), orc.Oracle(14, q, lc.T16)
    lc.check_keyless_level(X, O, orc, api, mem, KEYLESS_LEVEL_N16384)


@pytest.mark.gpu
def test_gpu_n32768_at_level_1(orc, api, lib, mem):
    """the benchmark's parameters, N = 2^15 over 4 x 60 bits, at level 1: one rotation and one relinearization with real keys"""
    S = lc.parent_setup(orc, "n32768_4x60", 15, orc.coeff_modulus_create(32768, [60] * 4), all_galois=False)
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    lc.check_rotation_and_relin(X, S, orc, api, mem, 1, 1)
