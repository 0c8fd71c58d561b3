"""The plain side at the reference's three plain moduli (65537, 8088322049, 1096486890805657601) on the GPU: the checks of
plain_modulus_common.py that test_plain_moduli.py runs on the emulator, at N = 4096 where the degree is free, and the reference's
own N = 32768 options end to end.  Every comparison is exact equality.  Run on an MI355X: python -m pytest tests -m gpu."""
import pytest

import parity_common as pc
import plain_modulus_common as pm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pc.TorchMem("cuda:0")


@pytest.fixture(scope="module")
def lib(api):
    lib = api.load_library()  # fails loudly if the HIP library is missing
    assert lib.hhe_backend() == b"hip-gfx950"
    return lib


@pytest.mark.parametrize("name", list(pm.LIFT_CASES))
def test_lift_words_equal_integer_product(orc, api, lib, mem, name):
    """a. hhe_multiply_plain (per item and broadcast) and the oracle's multiply_plain equal lift_j followed by a schoolbook
    negacyclic product in Python integers, on every limb, at N = 1024 and L = 2: t below q_j, between q_j and 2 q_j, above 2 q_j."""
    pm.check_lift_words(lambda logn, q, t: api.Context(logn, q, t, lib=lib), orc, api, lib, mem, name)


@pytest.fixture(scope="module")
def meaning(orc, api, lib):
    S = pm.meaning_setup(orc)
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    S.load_keys(X)
    yield X, S
    X.close()


def test_meaning_plain_product(meaning, mem):
    """b. T60 over 15 primes of 55 bits at N = 1024 (t > 2 q_j): decode(decrypt(multiply_plain(Enc(a), Encode(b)))) = a o b mod t"""
    pm.check_meaning_product(*meaning, mem)


def test_meaning_mask(meaning, mem):
    pm.check_meaning_mask(*meaning, mem)


@pytest.mark.parametrize("bsgs", [None, pm.MEANING_BSGS], ids=["diagonal", "bsgs4x4"])
def test_meaning_packed_affine(meaning, mem, bsgs):
    pm.check_meaning_affine(*meaning, mem, bsgs)


def test_meaning_fc_row(meaning, mem):
    pm.check_meaning_fc_row(*meaning, mem)


def test_meaning_ragged_transciphering(orc, meaning, mem):
    """15 is the smallest count of 55-bit primes at which the oracle keeps more than 10 bits of noise budget after one PASTA-3
    transciphering at T60: 23 bits on the full block and 24 on the 44-word one (0 with 14 primes).  The guard asserts it."""
    X, S = meaning
    pm.check_meaning_transcipher(X, S, orc, mem)


@pytest.mark.parametrize("name", list(pm.HOT_CASES))
def test_hot_path_words_n4096(orc, api, lib, mem, monkeypatch, name):
    """c. check_hot_path with the FC variants, BSGS transciphering, both affine methods, the adversarial matmul loop and the batched
    decryption at T33 and T60, on the row kernels (3 x 60 bits; 3 x 55 bits with T60, t above the primes) and on the fallback
    (BFVDefault(4096); 4 x 40 bits with T60)"""
    S, make_ctx = pm.hot_setup(orc, api, lib, name)
    pm.check_hot_words(make_ctx, S, orc, mem, monkeypatch, seed=len(name))


@pytest.mark.parametrize("name", list(pm.EDGE_CASES))
def test_plain_side_edges_n4096(orc, api, lib, mem, name):
    """d. encode with 1, N/2, N/2 + 1, N - 1 and N values and a row of t - 1; decrypt on all-(q_j - 1), alternating and uniform
    words and along six multiply_plain that run the noise budget to 0; hhe_add with size 3 on a product"""
    S = pm.edge_setup(orc, name, 12)
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    pm.check_plain_edges(X, S, mem)
    X.close()


@pytest.mark.parametrize("t,regime", [(pm.T60, "slow"), (pm.T33, "fast")], ids=["t60", "t33"])
def test_reference_option_n32768(orc, api, lib, mem, t, regime):
    """The reference's options at N = 32768 (configs/config.cpp:19-26) over CoeffModulus::BFVDefault(32768), 55- and 56-bit primes: T60
    sits above every one of them, T33 below.  Two items, encode -> add_plain / multiply_plain / hhe_mask -> hhe_decrypt, every slot
    against Python integers mod t."""
    q = api.bfv_default_coeff_modulus(32768, lib)
    assert pm.regime_of(t, q[:-1]) == regime, q
    S = pm.LightSetup(orc, 15, q, t)
    X = api.Context(15, q, t, lib=lib)
    pm.check_reference_option(X, S, mem)
    X.close()
