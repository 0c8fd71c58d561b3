"""One keystream per key on the emulator (the shared kernel bodies behind the real host driver): a context keeps the keystream
ciphertext of every block counter it has evaluated, and a later call under the same key ciphertext, key sets and use_bsgs evaluates
only the counters it finds none for.  See kscache_common for what every check compares."""
import numpy as np
import pytest

from conftest import Setup
import dedup_common as dc
import kscache_common as kc
import parity_common as pc
import plain_modulus_common as pm


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


@pytest.fixture(scope="module")
def row_setup(orc):
    return Setup(orc, 12, [50, 50, 50])  # the smallest context that takes the fused key-switch row kernel


def test_repeat(orc, api, emu_lib, mem, small, monkeypatch):
    S, ids, ncw = small, [0, 0, 3, 0, 3], [128, 17, 128, 1, 60]
    cw = kc.words(S, 5, 1)
    X, X0 = kc.ctx_on(api, emu_lib, S, monkeypatch), kc.ctx_off(api, emu_lib, S, monkeypatch)
    r1 = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (2, 0) and X.query("transcipher_unique") == 2
    assert X.query("ks_cache_entries") == 2 and X.query("ks_cache_bytes") == 2 * kc.ct_bytes(S)
    r2 = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (0, 2) and X.query("transcipher_unique") == 2 and X.query("ks_cache_entries") == 2
    r0 = kc.run(X0, S, mem, cw, ncw, ids)
    assert kc.counts(X0) == (2, 0)
    kc.run(X0, S, mem, cw, ncw, ids)
    assert kc.counts(X0) == (2, 0) and X0.query("ks_cache_entries") == 0  # the second implementation keeps nothing
    assert (r1 == r0).all() and (r2 == r0).all()
    assert (r2[4] == dc.oracle_block(S, cw, ncw, ids, 4)).all()


def test_new_words_same_counters(orc, api, emu_lib, mem, small, monkeypatch):
    """the finishing pass uses the call's own words and lengths, not the ones the keystream was first used with"""
    S, ids = small, [5, 1, 5]
    X, X0 = kc.ctx_on(api, emu_lib, S, monkeypatch), kc.ctx_off(api, emu_lib, S, monkeypatch)
    kc.run(X, S, mem, kc.words(S, 3, 2), [128, 128, 128], ids)
    cw, ncw = kc.words(S, 3, 3), [9, 128, 77]
    r = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (0, 2)
    assert (r == kc.run(X0, S, mem, cw, ncw, ids)).all()
    assert (r[0] == dc.oracle_block(S, cw, ncw, ids, 0)).all()


@pytest.mark.parametrize("env", [dict(HHE_STREAMS=2, HHE_CHUNK=2), dict(HHE_STREAMS=0)])
def test_partial_hits(orc, api, emu_lib, mem, small, monkeypatch, env):
    """counters [0, 1], then [1, 2, 0, 2]: one evaluation, in the slot before the two kept ones"""
    S = small
    X, X0 = kc.ctx_on(api, emu_lib, S, monkeypatch, **env), kc.ctx_off(api, emu_lib, S, monkeypatch, **env)
    kc.run(X, S, mem, kc.words(S, 2, 4), [128, 128], [0, 1])
    assert kc.counts(X) == (2, 0)
    cw, ncw, ids = kc.words(S, 4, 5), [128, 30, 128, 128], [1, 2, 0, 2]
    r = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (1, 2) and X.query("transcipher_unique") == 3 and X.query("ks_cache_entries") == 3
    assert (r == kc.run(X0, S, mem, cw, ncw, ids)).all()
    for b in (0, 1):
        assert (r[b] == dc.oracle_block(S, cw, ncw, ids, b)).all(), b


def test_all_distinct_call(orc, api, emu_lib, mem, small, monkeypatch):
    """U == B: one record of distinct counters is the service's real call and takes the two-phase shape too"""
    S, ids, ncw = small, [0, 1, 2], [128, 128, 9]
    cw = kc.words(S, 3, 6)
    X, X0 = kc.ctx_on(api, emu_lib, S, monkeypatch), kc.ctx_off(api, emu_lib, S, monkeypatch)
    r1 = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (3, 0)
    r2 = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (0, 3) and X.query("transcipher_unique") == 3
    r0 = kc.run(X0, S, mem, cw, ncw, ids)
    assert (r1 == r0).all() and (r2 == r0).all()
    assert (r2[2] == dc.oracle_block(S, cw, ncw, ids, 2)).all()


def test_enc_key_overwritten_in_place(orc, api, emu_lib, mem, small, monkeypatch):
    """the caller's buffer is identified by its words: refilled with another key ciphertext it misses, refilled with the first one it
    hits the older snapshot; a fifth key ciphertext drops the least recently used snapshot with its keystreams"""
    S, ids, ncw = small, [0, 0], [128, 40]
    cw = kc.words(S, 2, 7)
    encs = [S.enc_key] + [kc.other_enc_key(S, k) for k in range(4)]
    X = kc.ctx_on(api, emu_lib, S, monkeypatch)
    buf = mem.to_dev(encs[0])
    ra = kc.run(X, S, mem, cw, ncw, ids, key=buf)
    assert kc.counts(X) == (1, 0)
    buf[...] = encs[1]
    rb = kc.run(X, S, mem, cw, ncw, ids, key=buf)
    assert kc.counts(X) == (1, 0) and X.query("ks_cache_entries") == 2
    fresh = kc.run(kc.ctx_off(api, emu_lib, S, monkeypatch), S, mem, cw, ncw, ids, key=mem.to_dev(encs[1]))
    assert (rb == fresh).all() and not (rb == ra).all()
    assert (rb[1] == dc.oracle_block(S, cw, ncw, ids, 1, enc_key=encs[1])).all()
    buf[...] = encs[0]
    assert (kc.run(X, S, mem, cw, ncw, ids, key=buf) == ra).all() and kc.counts(X) == (0, 1)
    # snapshots now, least recently used first: encs[1], encs[0]; three more fill the four, the last of them drops encs[1]
    for k in (2, 3):
        buf[...] = encs[k]
        kc.run(X, S, mem, cw, ncw, ids, key=buf)
        assert kc.counts(X) == (1, 0)
    assert X.query("ks_cache_entries") == 4
    buf[...] = encs[4]
    r4 = kc.run(X, S, mem, cw, ncw, ids, key=buf)
    assert kc.counts(X) == (1, 0) and X.query("ks_cache_entries") == 4
    assert (r4[1] == dc.oracle_block(S, cw, ncw, ids, 1, enc_key=encs[4])).all()
    buf[...] = encs[0]
    assert (kc.run(X, S, mem, cw, ncw, ids, key=buf) == ra).all() and kc.counts(X) == (0, 1)
    buf[...] = encs[1]  # the dropped one: evaluated again, the same words
    assert (kc.run(X, S, mem, cw, ncw, ids, key=buf) == rb).all() and kc.counts(X) == (1, 0)


def test_key_replaced_or_added(orc, api, emu_lib, mem, small, monkeypatch):
    """a key of the default set replaced (Galois key of step -1, then the relinearization key) or added: the set is another object"""
    S, O, ids, ncw = small, small.O, [2, 2], [128, 50]
    cw = kc.words(S, 2, 8)
    rk2, gk2 = kc.other_keys(S, 41)
    e1 = int(O.galois_elt(-1))
    i1 = [int(e) for e in S.gk.elts].index(e1)
    X = kc.ctx_on(api, emu_lib, S, monkeypatch)
    ra = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (1, 0)

    def fresh(rk, g1):
        Y = kc.ctx_off(api, emu_lib, S, monkeypatch)
        Y.set_relin_key(rk)
        Y.set_galois_key(e1, g1)
        return kc.run(Y, S, mem, cw, ncw, ids)

    X.set_galois_key(e1, gk2.keys[i1])
    rb = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (1, 0) and X.query("ks_cache_entries") == 1  # what was kept under the replaced key is gone
    assert (rb == fresh(S.rk, gk2.keys[i1])).all() and not (rb == ra).all()
    X.set_relin_key(rk2)
    rc = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (1, 0)
    assert (rc == fresh(rk2, gk2.keys[i1])).all() and not (rc == rb).all()
    assert (kc.run(X, S, mem, cw, ncw, ids) == rc).all() and kc.counts(X) == (0, 1)
    e5 = int(O.galois_elt(5))  # a key no transciphering uses: the serial is the set's
    X.set_galois_key(e5, O.keygen_galois(S.sk, [e5], 43).keys[0])
    assert (kc.run(X, S, mem, cw, ncw, ids) == rc).all() and kc.counts(X) == (1, 0)


def test_two_key_sets_and_a_destroyed_one(orc, api, emu_lib, mem, small, monkeypatch):
    S, ids, ncw = small, [1, 1], [128, 3]
    cw = kc.words(S, 2, 9)
    rk2, gk2 = kc.other_keys(S, 51)
    X = kc.ctx_on(api, emu_lib, S, monkeypatch, load=False)
    A, B = kc.load_set(X, S.rk, S.gk), kc.load_set(X, rk2, gk2)
    ra = kc.run(X, S, mem, cw, ncw, ids, rk=A, gk=A)
    rb = kc.run(X, S, mem, cw, ncw, ids, rk=B, gk=B)
    assert kc.counts(X) == (1, 0) and X.query("ks_cache_entries") == 2
    assert (kc.run(X, S, mem, cw, ncw, ids, rk=A, gk=A) == ra).all() and kc.counts(X) == (0, 1)
    assert (kc.run(X, S, mem, cw, ncw, ids, rk=B, gk=B) == rb).all() and kc.counts(X) == (0, 1)
    rab = kc.run(X, S, mem, cw, ncw, ids, rk=A, gk=B)  # the pair is the identity, not either set
    assert kc.counts(X) == (1, 0) and X.query("ks_cache_entries") == 3
    Y = kc.ctx_off(api, emu_lib, S, monkeypatch, load=False)
    kc.load_default(Y, rk2, gk2)
    assert (ra == kc.run(kc.ctx_off(api, emu_lib, S, monkeypatch), S, mem, cw, ncw, ids)).all()
    assert (rb == kc.run(Y, S, mem, cw, ncw, ids)).all() and not (ra == rb).all() and not (rab == ra).all() and not (rab == rb).all()
    assert (rb[1] == S.O.transcipher_block(S.enc_key, rk2, gk2, cw[1, :3], 1)).all()
    # a destroyed set takes its keystreams with it, and a new set (here: at the keys of B) never finds the old one's
    A.close()
    assert X.query("ks_cache_entries") == 1
    Cs = kc.load_set(X, rk2, gk2)
    assert (kc.run(X, S, mem, cw, ncw, ids, rk=Cs, gk=Cs) == rb).all() and kc.counts(X) == (1, 0)
    assert (kc.run(X, S, mem, cw, ncw, ids, rk=B, gk=B) == rb).all() and kc.counts(X) == (0, 1)


def test_bsgs_and_diagonal_do_not_share(orc, api, emu_lib, mem, monkeypatch):
    S, _ = pm.hot_setup(orc, api, emu_lib, "t33_60x3")
    ids, ncw = [0, 1, 0], [128, 128, 12]
    cw = kc.words(S, 3, 10)
    X, X0 = kc.ctx_on(api, emu_lib, S, monkeypatch), kc.ctx_off(api, emu_lib, S, monkeypatch)
    res = {}
    for rnd, want in ((0, (2, 0)), (1, (0, 2))):
        for bsgs in (True, False):
            res[rnd, bsgs] = kc.run(X, S, mem, cw, ncw, ids, use_bsgs=bsgs)
            assert kc.counts(X) == want, (rnd, bsgs)
    assert X.query("ks_cache_entries") == 4
    for bsgs in (True, False):
        r0 = kc.run(X0, S, mem, cw, ncw, ids, use_bsgs=bsgs)
        assert (res[0, bsgs] == r0).all() and (res[1, bsgs] == r0).all()
    assert not (res[1, True] == res[1, False]).all()
    assert (res[1, True][2] == dc.oracle_block(S, cw, ncw, ids, 2, use_bsgs=True)).all()


def test_budget_of_two_entries(orc, api, emu_lib, mem, small, monkeypatch):
    S, cw = small, kc.words(small, 1, 11)
    X = kc.ctx_on(api, emu_lib, S, monkeypatch, HHE_KS_CACHE_MB=2 * kc.ct_bytes(S) / 2**20)
    r = [kc.run(X, S, mem, cw, [128], [ctr]) for ctr in (0, 1, 2)]
    assert X.query("ks_cache_entries") == 2 and X.query("ks_cache_bytes") == 2 * kc.ct_bytes(S) and X.query("block_cache_entries") == 3
    assert (kc.run(X, S, mem, cw, [128], [2]) == r[2]).all() and kc.counts(X) == (0, 1)
    assert (kc.run(X, S, mem, cw, [128], [0]) == r[0]).all() and kc.counts(X) == (1, 0)  # the least recently used one had gone
    assert (kc.run(X, S, mem, cw, [128], [2]) == r[2]).all() and kc.counts(X) == (0, 1)  # ... and now counter 1 has
    assert (kc.run(X, S, mem, cw, [128], [1]) == r[1]).all() and kc.counts(X) == (1, 0)
    assert X.query("ks_cache_entries") == 2
    assert (r[0][0] == dc.oracle_block(S, cw, [128], [0], 0)).all()


def test_goes_with_the_block_tables_and_clearing(orc, api, emu_lib, mem, small, monkeypatch):
    S, cw = small, kc.words(small, 2, 12)
    X = kc.ctx_on(api, emu_lib, S, monkeypatch)
    ra = kc.run(X, S, mem, cw[:1], [128], [0])
    rb = kc.run(X, S, mem, cw[1:], [60], [1])
    assert X.query("ks_cache_entries") == 2 and X.query("block_cache_entries") == 2
    limit = X.query("block_cache_bytes")
    X.set_block_cache_limit(limit - 1)  # the tables of counter 0 (least recently used) go, and its keystream with them
    assert X.query("block_cache_entries") == 1 and X.query("ks_cache_entries") == 1 and X.query("ks_cache_bytes") == kc.ct_bytes(S)
    X.set_block_cache_limit(limit)
    r = kc.run(X, S, mem, cw, [128, 60], [0, 1])
    assert kc.counts(X) == (1, 1) and (r[0] == ra[0]).all() and (r[1] == rb[0]).all()
    assert X.query("ks_cache_entries") == 2
    X.clear_keystream_cache()
    assert X.query("ks_cache_entries") == 0 and X.query("ks_cache_bytes") == 0 and X.query("block_cache_entries") == 2
    assert (kc.run(X, S, mem, cw, [128, 60], [0, 1]) == r).all() and kc.counts(X) == (2, 0)
    X.clear_block_cache()
    assert X.query("ks_cache_entries") == 0 and X.query("block_cache_entries") == 0
    assert (kc.run(X, S, mem, cw, [128, 60], [0, 1]) == r).all() and kc.counts(X) == (2, 0)
    assert (kc.run(X, S, mem, cw, [128, 60], [0, 1]) == r).all() and kc.counts(X) == (0, 2)
    X.close()  # with entries and a snapshot resident


def test_decompose_two_records_in_two_calls(orc, api, emu_lib, mem, monkeypatch):
    S = Setup(orc, 10, [50] * 9, extra_steps=(-128, -256))
    O = S.O
    pts = [np.array([(7 * i + 3 + 11 * s) % 256 for i in range(300)], dtype=np.uint64) for s in range(2)]
    recs = [orc.pasta_encrypt(S.t, S.key, p).reshape(1, -1) for p in pts]
    X, X0 = kc.ctx_on(api, emu_lib, S, monkeypatch), kc.ctx_off(api, emu_lib, S, monkeypatch)
    key, res = mem.to_dev(S.enc_key), {}
    for Y in (X, X0):
        for s in range(2):
            out = mem.empty((1,) + O.ct_shape)
            Y.decompose(key, recs[s], out, mask_last=True)
            res[Y is X, s] = mem.to_host(out)
            assert kc.counts(Y) == ((0, 3) if (Y is X and s) else (3, 0)) and Y.query("transcipher_unique") == 3
    assert (res[True, 0] == res[False, 0]).all() and (res[True, 1] == res[False, 1]).all()
    cw, ncw = S.sym_blocks(orc, pts[1])
    blocks = [O.transcipher_block(S.enc_key, S.rk, S.gk, cw[b, :ncw[b]], b) for b in range(3)]
    blocks[2] = O.mask(blocks[2], np.ones(44, np.uint64))
    assert (res[True, 1][0] == O.flatten(np.stack(blocks), S.gk)).all()


def test_profiled_calls_bypass(orc, api, emu_lib, mem, row_setup, monkeypatch):
    """a profiled call exists to time the chain: it neither looks a keystream up nor keeps one"""
    S, ids, ncw = row_setup, [3, 3], [128, 40]
    cw = kc.words(S, 2, 13)
    X = kc.ctx_on(api, emu_lib, S, monkeypatch)
    assert X.query("row_kernel") == 1
    X.profile(True)
    r1 = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (1, 0)
    r2 = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (1, 0) and X.query("ks_cache_entries") == 0
    X.profile(False)
    r3 = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (1, 0) and X.query("ks_cache_entries") == 1
    X.profile(True)
    r4 = kc.run(X, S, mem, cw, ncw, ids)  # nor does it use what an unprofiled call kept
    assert kc.counts(X) == (1, 0)
    X.profile(False)
    r5 = kc.run(X, S, mem, cw, ncw, ids)
    assert kc.counts(X) == (0, 1)
    r0 = kc.run(kc.ctx_off(api, emu_lib, S, monkeypatch), S, mem, cw, ncw, ids)
    for r in (r1, r2, r3, r4, r5):
        assert (r == r0).all()
    assert (r5[1] == dc.oracle_block(S, cw, ncw, ids, 1)).all()


def test_per_item_evaluation_keeps_nothing(orc, api, emu_lib, mem, small, monkeypatch):
    """HHE_DEDUP=0: every item evaluates its own keystream, on every call"""
    S, ids, ncw = small, [4, 4], [128, 128]
    cw = kc.words(S, 2, 14)
    X = kc.ctx_on(api, emu_lib, S, monkeypatch, HHE_DEDUP=0)
    for _ in range(2):
        r = kc.run(X, S, mem, cw, ncw, ids)
        assert kc.counts(X) == (2, 0) and X.query("transcipher_unique") == 2 and X.query("ks_cache_entries") == 0
    assert (r == kc.run(kc.ctx_on(api, emu_lib, S, monkeypatch), S, mem, cw, ncw, ids)).all()
