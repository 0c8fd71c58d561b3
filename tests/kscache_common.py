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


# ---- the bodies of tests/test_ks_cache.py that tests/test_stream_order_emu.py runs again under the lazy order of the emulator

def check_enc_key_overwritten_in_place(orc, api, lib, mem, S, monkeypatch):
    """the caller's buffer is identified by its words: refilled with another key ciphertext it misses, refilled with the first one it
    hits the older snapshot; a fifth key ciphertext drops the least recently used snapshot with its keystreams"""
    S, ids, ncw = S, [0, 0], [128, 40]
    cw = words(S, 2, 7)
    encs = [S.enc_key] + [other_enc_key(S, k) for k in range(4)]
    X = ctx_on(api, lib, S, monkeypatch)
    buf = mem.to_dev(encs[0])
    ra = run(X, S, mem, cw, ncw, ids, key=buf)
    assert counts(X) == (1, 0)
    buf[...] = encs[1]
    rb = run(X, S, mem, cw, ncw, ids, key=buf)
    assert counts(X) == (1, 0) and X.query("ks_cache_entries") == 2
    fresh = run(ctx_off(api, lib, S, monkeypatch), S, mem, cw, ncw, ids, key=mem.to_dev(encs[1]))
    assert (rb == fresh).all() and not (rb == ra).all()
    assert (rb[1] == dc.oracle_block(S, cw, ncw, ids, 1, enc_key=encs[1])).all()
    buf[...] = encs[0]
    assert (run(X, S, mem, cw, ncw, ids, key=buf) == ra).all() and counts(X) == (0, 1)
    # snapshots now, least recently used first: encs[1], encs[0]; three more fill the four, the last of them drops encs[1]
    for k in (2, 3):
        buf[...] = encs[k]
        run(X, S, mem, cw, ncw, ids, key=buf)
        assert counts(X) == (1, 0)
    assert X.query("ks_cache_entries") == 4
    buf[...] = encs[4]
    r4 = run(X, S, mem, cw, ncw, ids, key=buf)
    assert counts(X) == (1, 0) and X.query("ks_cache_entries") == 4
    assert (r4[1] == dc.oracle_block(S, cw, ncw, ids, 1, enc_key=encs[4])).all()
    buf[...] = encs[0]
    assert (run(X, S, mem, cw, ncw, ids, key=buf) == ra).all() and counts(X) == (0, 1)
    buf[...] = encs[1]  # the dropped one: evaluated again, the same words
    assert (run(X, S, mem, cw, ncw, ids, key=buf) == rb).all() and counts(X) == (1, 0)


def check_key_replaced_or_added(orc, api, lib, mem, S, monkeypatch):
    """a key of the default set replaced (Galois key of step -1, then the relinearization key) or added: the set is another object"""
    S, O, ids, ncw = S, S.O, [2, 2], [128, 50]
    cw = words(S, 2, 8)
    rk2, gk2 = other_keys(S, 41)
    e1 = int(O.galois_elt(-1))
    i1 = [int(e) for e in S.gk.elts].index(e1)
    X = ctx_on(api, lib, S, monkeypatch)
    ra = run(X, S, mem, cw, ncw, ids)
    assert counts(X) == (1, 0)

    def fresh(rk, g1):
        Y = ctx_off(api, lib, S, monkeypatch)
        Y.set_relin_key(rk)
        Y.set_galois_key(e1, g1)
        return run(Y, S, mem, cw, ncw, ids)

    X.set_galois_key(e1, gk2.keys[i1])
    rb = run(X, S, mem, cw, ncw, ids)
    assert counts(X) == (1, 0) and X.query("ks_cache_entries") == 1  # what was kept under the replaced key is gone
    assert (rb == fresh(S.rk, gk2.keys[i1])).all() and not (rb == ra).all()
    X.set_relin_key(rk2)
    rc = run(X, S, mem, cw, ncw, ids)
    assert counts(X) == (1, 0)
    assert (rc == fresh(rk2, gk2.keys[i1])).all() and not (rc == rb).all()
    assert (run(X, S, mem, cw, ncw, ids) == rc).all() and counts(X) == (0, 1)
    e5 = int(O.galois_elt(5))  # a key no transciphering uses: the serial is the set's
    X.set_galois_key(e5, O.keygen_galois(S.sk, [e5], 43).keys[0])
    assert (run(X, S, mem, cw, ncw, ids) == rc).all() and counts(X) == (1, 0)


def check_two_key_sets_and_a_destroyed_one(orc, api, lib, mem, S, monkeypatch):
    S, ids, ncw = S, [1, 1], [128, 3]
    cw = words(S, 2, 9)
    rk2, gk2 = other_keys(S, 51)
    X = ctx_on(api, lib, S, monkeypatch, load=False)
    A, B = load_set(X, S.rk, S.gk), load_set(X, rk2, gk2)
    ra = run(X, S, mem, cw, ncw, ids, rk=A, gk=A)
    rb = run(X, S, mem, cw, ncw, ids, rk=B, gk=B)
    assert counts(X) == (1, 0) and X.query("ks_cache_entries") == 2
    assert (run(X, S, mem, cw, ncw, ids, rk=A, gk=A) == ra).all() and counts(X) == (0, 1)
    assert (run(X, S, mem, cw, ncw, ids, rk=B, gk=B) == rb).all() and counts(X) == (0, 1)
    rab = run(X, S, mem, cw, ncw, ids, rk=A, gk=B)  # the pair is the identity, not either set
    assert counts(X) == (1, 0) and X.query("ks_cache_entries") == 3
    Y = ctx_off(api, lib, S, monkeypatch, load=False)
    load_default(Y, rk2, gk2)
    assert (ra == run(ctx_off(api, lib, S, monkeypatch), S, mem, cw, ncw, ids)).all()
    assert (rb == run(Y, S, mem, cw, ncw, ids)).all() and not (ra == rb).all() and not (rab == ra).all() and not (rab == rb).all()
    assert (rb[1] == S.O.transcipher_block(S.enc_key, rk2, gk2, cw[1, :3], 1)).all()
    # a destroyed set takes its keystreams with it, and a new set (here: at the keys of B) never finds the old one's
    A.close()
    assert X.query("ks_cache_entries") == 1
    Cs = load_set(X, rk2, gk2)
    assert (run(X, S, mem, cw, ncw, ids, rk=Cs, gk=Cs) == rb).all() and counts(X) == (1, 0)
    assert (run(X, S, mem, cw, ncw, ids, rk=B, gk=B) == rb).all() and counts(X) == (0, 1)


def check_budget_of_two_entries(orc, api, lib, mem, S, monkeypatch):
    S, cw = S, words(S, 1, 11)
    X = ctx_on(api, lib, S, monkeypatch, HHE_KS_CACHE_MB=2 * ct_bytes(S) / 2**20)
    r = [run(X, S, mem, cw, [128], [ctr]) for ctr in (0, 1, 2)]
    assert X.query("ks_cache_entries") == 2 and X.query("ks_cache_bytes") == 2 * ct_bytes(S) and X.query("block_cache_entries") == 3
    assert (run(X, S, mem, cw, [128], [2]) == r[2]).all() and counts(X) == (0, 1)
    assert (run(X, S, mem, cw, [128], [0]) == r[0]).all() and counts(X) == (1, 0)  # the least recently used one had gone
    assert (run(X, S, mem, cw, [128], [2]) == r[2]).all() and counts(X) == (0, 1)  # ... and now counter 1 has
    assert (run(X, S, mem, cw, [128], [1]) == r[1]).all() and counts(X) == (1, 0)
    assert X.query("ks_cache_entries") == 2
    assert (r[0][0] == dc.oracle_block(S, cw, [128], [0], 0)).all()


def check_goes_with_the_block_tables_and_clearing(orc, api, lib, mem, S, monkeypatch):
    S, cw = S, words(S, 2, 12)
    X = ctx_on(api, lib, S, monkeypatch)
    ra = run(X, S, mem, cw[:1], [128], [0])
    rb = run(X, S, mem, cw[1:], [60], [1])
    assert X.query("ks_cache_entries") == 2 and X.query("block_cache_entries") == 2
    limit = X.query("block_cache_bytes")
    X.set_block_cache_limit(limit - 1)  # the tables of counter 0 (least recently used) go, and its keystream with them
    assert X.query("block_cache_entries") == 1 and X.query("ks_cache_entries") == 1 and X.query("ks_cache_bytes") == ct_bytes(S)
    X.set_block_cache_limit(limit)
    r = run(X, S, mem, cw, [128, 60], [0, 1])
    assert counts(X) == (1, 1) and (r[0] == ra[0]).all() and (r[1] == rb[0]).all()
    assert X.query("ks_cache_entries") == 2
    X.clear_keystream_cache()
    assert X.query("ks_cache_entries") == 0 and X.query("ks_cache_bytes") == 0 and X.query("block_cache_entries") == 2
    assert (run(X, S, mem, cw, [128, 60], [0, 1]) == r).all() and counts(X) == (2, 0)
    X.clear_block_cache()
    assert X.query("ks_cache_entries") == 0 and X.query("block_cache_entries") == 0
    assert (run(X, S, mem, cw, [128, 60], [0, 1]) == r).all() and counts(X) == (2, 0)
    assert (run(X, S, mem, cw, [128, 60], [0, 1]) == r).all() and counts(X) == (0, 2)
    X.close()  # with entries and a snapshot resident
