"""Keys and ciphertexts from a seed on the gfx950 kernels: the calls of tests/test_keygen_emu.py through keygen_common, at the smallest
shapes that take each path, and one case at the benchmark's parameters."""
import numpy as np
import pytest

import keygen_common as kg
import parity_common as pc
import plain_modulus_common as pm
from test_keygen_emu import SHAPES, T, low_half_prime, make


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


def ctx(orc, api, lib, shape, t=T):
    logn, bits = SHAPES[shape]
    X, O = make(orc, api, lib, logn, orc.coeff_modulus_create(1 << logn, bits), t)
    assert X.query("row_kernel") == (1 if logn >= 12 else 0)
    return X, O


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gpu_sampler(orc, api, lib, mem, shape):
    X, O = ctx(orc, api, lib, shape)
    kg.check_sampler(X, O, mem)
    kg.check_sampler(X, O, mem, seed=kg.SEED2)


@pytest.mark.gpu
def test_gpu_sampler_second_rejection_branch(orc, api, lib, mem):
    n = 1024
    q = [low_half_prime(orc, n, 50)] + orc.coeff_modulus_create(n, [50, 50])
    X, O = make(orc, api, lib, 10, q)
    assert kg.check_sampler(X, O, mem, min_words=129) > 128


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gpu_keys_word_for_word(orc, api, lib, mem, shape):
    X, O = ctx(orc, api, lib, shape)
    kg.check_keys_words(X, O, mem)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gpu_generated_keys_behave(orc, api, lib, mem, shape):
    X, O = ctx(orc, api, lib, shape)
    kg.check_keys_behave(X, O, orc, mem)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gpu_life_cycle(orc, api, lib, mem, shape):
    X, O = ctx(orc, api, lib, shape)
    kg.check_life_cycle(X, api.Context(O.logn, O.q, T, lib=lib), O, orc, mem, api)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gpu_regeneration_drops_kept_keystreams(orc, api, lib, mem, shape, monkeypatch):
    monkeypatch.setenv("HHE_KS_CACHE", "1")
    X, O = ctx(orc, api, lib, shape)
    assert X.query("ks_cache") == 1
    kg.check_regeneration_drops_keystreams(X, O, orc, mem)


@pytest.mark.gpu
@pytest.mark.parametrize("t", [pm.T16, pm.T33, pm.T60])
def test_gpu_encrypt_n1024(orc, api, lib, mem, t):
    q = pm.primes_near(orc, 1024, [60] * 3 if t == pm.T60 else [50] * 3)
    X, O = make(orc, api, lib, 10, q, t)
    kg.check_encrypt(X, O, mem)


@pytest.mark.gpu
def test_gpu_encrypt_n4096(orc, api, lib, mem):
    X, O = ctx(orc, api, lib, "n4096_3x60")
    kg.check_encrypt(X, O, mem)


@pytest.mark.gpu
def test_gpu_keys_on_bfv_default_4096(orc, api, lib, mem):
    """36 + 36 + 37 bits: no pseudo-Mersenne form, the separate-kernel key switch"""
    X, O = make(orc, api, lib, 12, api.bfv_default_coeff_modulus(4096, lib))
    assert X.query("row_kernel") == 0
    kg.check_keys_words(X, O, mem)
    kg.check_keys_behave(X, O, orc, mem)


@pytest.mark.gpu
def test_gpu_no_oracle_key_anywhere(orc, api, lib, mem):
    X, O = make(orc, api, lib, 10, orc.coeff_modulus_create(1024, [50] * 9))
    kg.check_full_flow(X, O, orc, mem)


@pytest.mark.gpu
def test_gpu_benchmarked_parameters(orc, api, lib, mem):
    """N = 2^15, 4 x 60 bits: all default Galois keys; k1 of every key and digit is pure sampler output; one element in full; the
    oracle's rotate_rows with that key read back; two encrypted items"""
    logn = 15
    X, O = make(orc, api, lib, logn, orc.coeff_modulus_create(1 << logn, [60] * 4))
    assert X.query("row_kernel") == 1
    D = kg.DeviceKeys(X, O, mem, kg.SEED)
    ks = X.keyset()
    ks.generate_galois(D.d_sk, kg.SEED2)
    elts = list(dict.fromkeys(int(e) for e in O.galois_elts_all()))
    assert len(elts) == 2 * (logn - 1)  # get_elts_all lists 2 (logn - 1) + 1 elements and repeats 3^(N/4)
    one = O.galois_elt(1)
    assert one in elts
    full = None
    for e in elts:
        assert ks.has_galois(e)
        got = ks.get_galois(e)
        ref, _ = kg.expected_enc_zero(O, None, kg.SEED2, kg.GALOIS, e, O.L, only_k1=True)
        assert (got[:, 1] == ref[:, 1]).all(), e
        if e == one:
            full = got
    _, sk = kg.expected_secret(O, kg.SEED)
    assert (D.sk == sk).all()
    nk = kg.new_key_galois(O, sk, one)
    ref, noise = kg.expected_enc_zero(O, sk, kg.SEED2, kg.GALOIS, one, O.L, nk)
    assert (full == ref).all()
    vals = np.arange(O.n, dtype=np.uint64) % np.uint64(1000)
    plain = np.stack([O.encode(vals), O.encode(vals[::-1].copy())])
    d_ct, d_out = mem.empty((2,) + O.ct_shape), mem.empty((2,) + O.ct_shape)
    X.encrypt(D.d_pk, mem.to_dev(plain), kg.SEED2, 2, d_ct)
    cts = mem.to_host(d_ct)
    for b in range(2):
        assert (cts[b] == kg.expected_encrypt(O, D.pk, plain[b], kg.SEED2, b)).all(), b
    X.rotate_rows(d_ct, 1, d_out, 2, gk=ks)
    got = mem.to_host(d_out)
    rot, nks = O.rotate_rows(cts[0], 1, orc.GaloisKeys([one], full[None]))
    assert nks == 1 and (got[0] == rot).all()
    assert (kg.slots_of(O, D.sk, got[0]) == kg.rot_rows(vals, 1)).all()
    ks.close()
