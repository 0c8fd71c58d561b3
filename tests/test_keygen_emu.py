"""Keys and ciphertexts from a seed on the emulator (the shared kernel bodies behind the real host driver); see keygen_common for
what every check compares.  The GPU suite makes the same calls in tests/test_gpu_keygen.py."""
import numpy as np
import pytest

import keygen_common as kg
import parity_common as pc
import plain_modulus_common as pm

T = 65537


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


def make(orc, api, lib, logn, q, t=T):
    return api.Context(logn, q, t, lib=lib), orc.Oracle(logn, q, t)


def low_half_prime(orc, n, bits):
    """the first prime = 1 mod 2n from 2^(bits-1) upward: a uniform word passes its mask and fails the comparison about half the time"""
    p = (1 << (bits - 1)) + 1
    while not orc.lib().orc_is_prime(p):
        p += 2 * n
    assert p.bit_length() == bits and p < (1 << (bits - 1)) + (1 << (bits - 4))
    return p


SHAPES = {"n1024_3x50": (10, [50] * 3), "n4096_3x60": (12, [60] * 3)}


def test_restatement_sanity():
    r = kg.sanity()
    assert all(abs(f - 1 / 3) < 0.01 for f in r["freq"]), r
    assert abs(r["var"] - 10.5) < 0.5 and abs(r["mean"]) < 0.1, r
    assert -21 <= r["lo"] and r["hi"] <= 21, r


@pytest.mark.parametrize("shape", list(SHAPES))
def test_sampler(orc, api, emu_lib, mem, shape):
    logn, bits = SHAPES[shape]
    X, O = make(orc, api, emu_lib, logn, orc.coeff_modulus_create(1 << logn, bits))
    kg.check_sampler(X, O, mem)
    kg.check_sampler(X, O, mem, seed=kg.SEED2)


def test_sampler_second_rejection_branch(orc, api, emu_lib, mem):
    n = 1024
    q = [low_half_prime(orc, n, 50)] + orc.coeff_modulus_create(n, [50, 50])
    X, O = make(orc, api, emu_lib, 10, q)
    assert kg.check_sampler(X, O, mem, min_words=129) > 128  # some chunk squeezed past 128 words: several blocks more than its neighbours


@pytest.mark.parametrize("shape", list(SHAPES))
def test_keys_word_for_word(orc, api, emu_lib, mem, shape):
    logn, bits = SHAPES[shape]
    X, O = make(orc, api, emu_lib, logn, orc.coeff_modulus_create(1 << logn, bits))
    kg.check_keys_words(X, O, mem)


@pytest.mark.parametrize("logn,bits,row", [(11, [50] * 3, 0), (12, [50] * 3, 1)])
def test_generated_keys_behave(orc, api, emu_lib, mem, logn, bits, row):
    X, O = make(orc, api, emu_lib, logn, orc.coeff_modulus_create(1 << logn, bits))
    assert X.query("row_kernel") == row
    kg.check_keys_behave(X, O, orc, mem)


@pytest.mark.parametrize("logn,row", [(10, 0), (12, 1)])
def test_life_cycle(orc, api, emu_lib, mem, logn, row):
    q = orc.coeff_modulus_create(1 << logn, [50] * 3)
    X, O = make(orc, api, emu_lib, logn, q)
    assert X.query("row_kernel") == row
    kg.check_life_cycle(X, api.Context(logn, q, T, lib=emu_lib), O, orc, mem, api)


def test_regeneration_drops_kept_keystreams(orc, api, emu_lib, mem, monkeypatch):
    monkeypatch.setenv("HHE_KS_CACHE", "1")
    X, O = make(orc, api, emu_lib, 10, orc.coeff_modulus_create(1024, [50] * 3))
    assert X.query("ks_cache") == 1
    kg.check_regeneration_drops_keystreams(X, O, orc, mem)


@pytest.mark.parametrize("t", [pm.T16, pm.T33, pm.T60])
def test_encrypt(orc, api, emu_lib, mem, t):
    q = pm.primes_near(orc, 1024, [60] * 3 if t == pm.T60 else [50] * 3)
    X, O = make(orc, api, emu_lib, 10, q, t)
    kg.check_encrypt(X, O, mem)


def test_no_oracle_key_anywhere(orc, api, emu_lib, mem):
    X, O = make(orc, api, emu_lib, 10, orc.coeff_modulus_create(1024, [50] * 9))
    kg.check_full_flow(X, O, orc, mem)
