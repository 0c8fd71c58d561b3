"""One keystream per block counter (HHE_DEDUP, DESIGN.md "one keystream per counter"): what tests/test_dedup.py (emulator) and
tests/test_gpu_dedup.py share.  Every check is exact equality of ciphertext words: knob 1 (a call evaluates each distinct counter
once and finishes every item against its counter's keystream) against knob 0 (every item evaluates its own), the named items against
the oracle's transcipher_block, and the number of keystream evaluations the context reports."""
import numpy as np


def make_ctx(api, lib, S, monkeypatch, **env):
    """a context created under the given knobs (they are read at creation), keys loaded"""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    for k in env:
        monkeypatch.delenv(k)
    S.load_keys(X)
    return X


def words(S, B, seed):
    """[B][128] symmetric ciphertext words, a different row per item; a row is full, so the words past an item's count are the
    stale ones the call must not read"""
    return np.random.default_rng(seed).integers(0, S.t, size=(B, 128), dtype=np.uint64)


def run(X, S, mem, cw, ncw, ids, enc_key=None, use_bsgs=False):
    out = mem.empty((len(ids),) + S.O.ct_shape)
    X.transcipher(mem.to_dev(S.enc_key if enc_key is None else enc_key), cw, ncw, ids, out, use_bsgs=use_bsgs)
    return mem.to_host(out)


def oracle_block(S, cw, ncw, ids, b, enc_key=None, use_bsgs=False):
    return S.O.transcipher_block(S.enc_key if enc_key is None else enc_key, S.rk, S.gk, cw[b, :ncw[b]], ids[b], use_bsgs=use_bsgs)


def check_dedup(api, lib, S, orc, mem, monkeypatch, cw, ncw, ids, unique, oracle_items, use_bsgs=False, **env):
    """knob 1 == knob 0 word for word, the chosen items == the oracle, and the evaluations counted: `unique` under knob 1 (the item
    count when no counter repeats), the item count under knob 0"""
    X1 = make_ctx(api, lib, S, monkeypatch, HHE_DEDUP=1, **env)
    X0 = make_ctx(api, lib, S, monkeypatch, HHE_DEDUP=0, **env)
    assert X1.query("dedup") == 1 and X0.query("dedup") == 0
    r1 = run(X1, S, mem, cw, ncw, ids, use_bsgs=use_bsgs)
    r0 = run(X0, S, mem, cw, ncw, ids, use_bsgs=use_bsgs)
    assert (r1 == r0).all()
    for b in oracle_items:
        assert (r1[b] == oracle_block(S, cw, ncw, ids, b, use_bsgs=use_bsgs)).all(), f"item {b} differs from the oracle"
    assert X1.query("transcipher_unique") == unique and X0.query("transcipher_unique") == len(ids)
    return X1, X0, r1
