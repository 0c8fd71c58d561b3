"""One keystream per key (HHE_KS_CACHE, DESIGN.md "one keystream per key"): what tests/test_ks_cache.py (emulator) and
tests/test_gpu_ks_cache.py share.  Every check is exact equality of ciphertext words: a context that keeps keystreams across calls
against a fresh context created under HHE_KS_CACHE=0 (which evaluates every call in full, launch for launch what the library did before
it kept anything), named items against the oracle's transcipher_block, and the evaluations / hits the context reports."""
import numpy as np

import dedup_common as dc

words = dc.words


def ctx_on(api, lib, S, monkeypatch, load=True, **env):
    X = _ctx(api, lib, S, monkeypatch, load, HHE_KS_CACHE=1, **env)
    assert X.query("ks_cache") == 1 and X.query("ks_cache_entries") == 0
    return X


def ctx_off(api, lib, S, monkeypatch, load=True, **env):
    X = _ctx(api, lib, S, monkeypatch, load, HHE_KS_CACHE=0, **env)
    assert X.query("ks_cache") == 0
    return X


def _ctx(api, lib, S, monkeypatch, load, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    for k in env:
        monkeypatch.delenv(k)
    if load:
        S.load_keys(X)
    return X


def load_default(X, rk, gk):
    X.set_relin_key(rk)
    for i, e in enumerate(gk.elts):
        X.set_galois_key(int(e), gk.keys[i])


def load_set(X, rk, gk):
    ks = X.keyset()
    ks.set_relin(rk)
    for i, e in enumerate(gk.elts):
        ks.set_galois(int(e), gk.keys[i])
    return ks


def run(X, S, mem, cw, ncw, ids, key=None, use_bsgs=False, rk=None, gk=None):
    """key: a device buffer that holds the key ciphertext (default: a new one with S.enc_key)"""
    out = mem.empty((len(ids),) + S.O.ct_shape)
    X.transcipher(mem.to_dev(S.enc_key) if key is None else key, cw, ncw, ids, out, use_bsgs=use_bsgs, rk=rk, gk=gk)
    return mem.to_host(out)


def counts(X):
    """(keystream chains the last call ran, counters it found a kept keystream for)"""
    return X.query("transcipher_evaluated"), X.query("ks_cache_hits")


def ct_bytes(S):
    return int(np.prod(S.O.ct_shape)) * 8


def other_keys(S, seed):
    """(relin key, Galois keys for the elements of S.gk) from another run of the key generator: same secret key, other randomness"""
    return S.O.keygen_relin(S.sk, seed), S.O.keygen_galois(S.sk, [int(e) for e in S.gk.elts], seed + 1)


def other_enc_key(S, k):
    """the BFV encryption of another PASTA key"""
    return S.O.encrypt(S.pk, S.O.pasta_pack_key((S.key * (k + 2) + k) % S.t), 100 + k)
