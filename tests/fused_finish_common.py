"""The fused finishing pass of a transciphering call (HHE_FIN_FUSED, DESIGN.md "Fused finishing pass"): what tests/test_fused_finish.py
(emulator) and tests/test_gpu_fused_finish.py share.  Every check is exact equality of ciphertext words between a context created under
HHE_FIN_FUSED=1 (res = Enc(c_b) - KS in two kernels: the first inverse pass mod t gathers its tile from the words, the last one ends in
the add_plain epilogue), one created under HHE_FIN_FUSED=0 (clear, scatter, transform, add_plain: launch for launch what the library did
before) and, for named items, the oracle's transcipher_block."""
import numpy as np

import dedup_common as dc
import kscache_common as kc

BSGS_STEPS = tuple(-16 * k for k in range(1, 8))
CHUNKED = dict(HHE_STREAMS=2, HHE_CHUNK=2)  # seven items finish in four chunks on two lanes: offsets into words, table and out
SEVEN = [1, 2, 0, 2, 3, 4, 1]
SEVEN_NCW = [128, 30, 128, 128, 1, 128, 64]


def pair(api, lib, S, monkeypatch, **env):
    """(fused context, unfused context) under the same further knobs, keys loaded; each has asserted what it runs"""
    X1 = dc.make_ctx(api, lib, S, monkeypatch, HHE_FIN_FUSED=1, **env)
    X0 = dc.make_ctx(api, lib, S, monkeypatch, HHE_FIN_FUSED=0, **env)
    assert X1.query("fin_fused") == 1 and X0.query("fin_fused") == 0
    return X1, X0


def same(S, mem, X1, X0, cw, ncw, ids, oracle_items=(), use_bsgs=False):
    r1 = kc.run(X1, S, mem, cw, ncw, ids, use_bsgs=use_bsgs)
    r0 = kc.run(X0, S, mem, cw, ncw, ids, use_bsgs=use_bsgs)
    assert (r1 == r0).all(), ("items that differ from the unfused pass:", np.argwhere((r1 != r0).reshape(len(ids), -1).any(axis=1)).ravel())
    for b in oracle_items:
        assert (r1[b] == dc.oracle_block(S, cw, ncw, ids, b, use_bsgs=use_bsgs)).all(), f"item {b} differs from the oracle"
    return r1


def check_lengths(api, lib, S, mem, monkeypatch):
    """block lengths 0, 1, 127 and 128 within one call; the rows are full, so the words past a count are stale ones"""
    X1, X0 = pair(api, lib, S, monkeypatch)
    same(S, mem, X1, X0, kc.words(S, 4, 71), [0, 1, 127, 128], [0, 0, 1, 0], oracle_items=(1, 2))
    X1.close(), X0.close()


def check_word_range(api, lib, S, mem, monkeypatch):
    """every slot at t - 1, against the oracle; words of t, t + 5 and 2^64 - 1 against the unfused pass, which reduces them mod t"""
    X1, X0 = pair(api, lib, S, monkeypatch)
    cw = np.full((2, 128), S.t - 1, np.uint64)
    same(S, mem, X1, X0, cw, [128, 128], [0, 3], oracle_items=(0,))
    cw = kc.words(S, 3, 72)
    cw[0, ::3], cw[0, 1::3], cw[0, 127] = S.t, S.t + 5, 2**64 - 1
    cw[1, :] = 2**64 - 1
    cw[2, 5] = S.t
    r = same(S, mem, X1, X0, cw, [128, 128, 6], [0, 0, 0])
    red = cw.copy()
    red[0], red[1], red[2, 5] = cw[0] % np.uint64(S.t), cw[1] % np.uint64(S.t), 0
    assert (r == kc.run(X1, S, mem, red, [128, 128, 6], [0, 0, 0])).all()  # ... and so does the fused one
    X1.close(), X0.close()


def check_chunks_and_hits(api, lib, S, mem, monkeypatch):
    """seven items over five counters in four chunks on two lanes: cold, with two of the counters kept, with all of them kept"""
    cw = kc.words(S, 7, 73)
    X1, X0 = pair(api, lib, S, monkeypatch, **CHUNKED)
    r_cold = same(S, mem, X1, X0, cw, SEVEN_NCW, SEVEN, oracle_items=(4, 6))
    assert kc.counts(X1) == (5, 0) and kc.counts(X0) == (5, 0)
    X2 = dc.make_ctx(api, lib, S, monkeypatch, HHE_FIN_FUSED=1, **CHUNKED)
    kc.run(X2, S, mem, kc.words(S, 2, 74), [128, 128], [0, 1])
    assert kc.counts(X2) == (2, 0)
    r_part = kc.run(X2, S, mem, cw, SEVEN_NCW, SEVEN)
    assert kc.counts(X2) == (3, 2) and X2.query("transcipher_unique") == 5
    r_all = kc.run(X2, S, mem, cw, SEVEN_NCW, SEVEN)
    assert kc.counts(X2) == (0, 5)
    assert (r_part == r_cold).all() and (r_all == r_cold).all()
    assert (kc.run(X0, S, mem, cw, SEVEN_NCW, SEVEN) == r_cold).all() and kc.counts(X0) == (0, 5)
    for X in (X1, X0, X2):
        X.close()


def check_grow_and_shrink(api, lib, S, mem, monkeypatch):
    """B = 1, then 9, then 2 on one context: the staging grows, and the last call's short blocks lie where the second had full ones"""
    X1, X0 = pair(api, lib, S, monkeypatch)
    cw = kc.words(S, 9, 75)
    same(S, mem, X1, X0, cw[:1], [128], [0])
    same(S, mem, X1, X0, cw, [128] * 9, [0, 1, 0, 1, 0, 1, 0, 1, 0])
    same(S, mem, X1, X0, kc.words(S, 2, 76), [3, 0], [1, 0], oracle_items=(0,))
    X1.close(), X0.close()


def check_chunk_tail(api, lib, S, mem, monkeypatch, oracle=True):
    """the path without a keystream table (transcipher_chunk's own tail): HHE_KS_CACHE=0 with distinct counters, HHE_DEDUP=0, a profiled call"""
    cw, ncw = kc.words(S, 3, 77), [128, 9, 0]
    for env, ids in ((dict(HHE_KS_CACHE=0), [0, 1, 2]), (dict(HHE_DEDUP=0), [0, 0, 1])):
        X1, X0 = pair(api, lib, S, monkeypatch, **env)
        same(S, mem, X1, X0, cw, ncw, ids, oracle_items=(1,) if oracle and "HHE_DEDUP" in env else ())
        assert kc.counts(X1) == (3, 0) and X1.query("ks_cache_entries") == 0
        X1.close(), X0.close()
    X1, X0 = pair(api, lib, S, monkeypatch)
    X1.profile(True), X0.profile(True)
    same(S, mem, X1, X0, cw, ncw, [0, 1, 2])
    assert X1.query("ks_cache_entries") == 0
    X1.close(), X0.close()


def check_bsgs(api, lib, S, mem, monkeypatch):
    X1, X0 = pair(api, lib, S, monkeypatch)
    same(S, mem, X1, X0, kc.words(S, 2, 78), [128, 40], [0, 0], oracle_items=(1,), use_bsgs=True)
    X1.close(), X0.close()


def check_one_call(api, lib, S, mem, monkeypatch, oracle_items=(1,), seed=79):
    """one transciphering of three items over two counters, then the same against the kept keystreams"""
    X1, X0 = pair(api, lib, S, monkeypatch)
    cw, ncw, ids = kc.words(S, 3, seed), [128, 17, 128], [0, 0, 2]
    r = same(S, mem, X1, X0, cw, ncw, ids, oracle_items=oracle_items)
    assert (kc.run(X1, S, mem, cw, ncw, ids) == r).all() and kc.counts(X1) == (0, 2)
    X1.close(), X0.close()


def check_prediction(api, lib, S, mem, monkeypatch, in_place=False):
    """key A twice, key B over the same counters, A again, under HHE_FIN_ITEM=1 (set by the caller): the second call is enqueued on the
    prediction and confirmed (one launch), the third is enqueued on the prediction of A, refuted and finished again (two launches), the
    fourth predicts B -- the key used last -- and is refuted too; every result is the oracle's for its key and the counts are what they
    are without the item kernel.  in_place (numpy-backed memory only): every call reads the key ciphertext from ONE buffer, overwritten
    between the calls -- what the key comparison sees is what the buffer holds when the comparison runs"""
    X = dc.make_ctx(api, lib, S, monkeypatch)
    X0 = dc.make_ctx(api, lib, S, monkeypatch, HHE_FIN_ITEM=0)
    assert X.query("fin_item") == 1 and X0.query("fin_item") == 0
    cw, ncw, ids = kc.words(S, 3, 81), [128, 9, 128], [0, 2, 0]
    enc_b = kc.other_enc_key(S, 0)
    key_a, key_b = mem.to_dev(S.enc_key), mem.to_dev(enc_b)
    buf = mem.to_dev(S.enc_key) if in_place else None

    def held(key):
        if not in_place:
            return key
        buf[...] = key
        return buf

    launches, results = [], []
    for key, want in ((key_a, (2, 0)), (key_a, (0, 2)), (key_b, (2, 0)), (key_a, (0, 2))):
        before = X.query("fin_item_launches")
        results.append(kc.run(X, S, mem, cw, ncw, ids, key=held(key)))
        launches.append(X.query("fin_item_launches") - before)
        assert kc.counts(X) == want
        assert (kc.run(X0, S, mem, cw, ncw, ids, key=held(key)) == results[-1]).all() and kc.counts(X0) == want
        assert X.query("ks_cache_entries") == X0.query("ks_cache_entries")
    assert launches == [1, 1, 2, 2] and X0.query("fin_item_launches") == 0
    assert (results[0] == results[1]).all() and (results[0] == results[3]).all() and (results[0] != results[2]).any()
    assert (results[1][1] == dc.oracle_block(S, cw, ncw, ids, 1)).all()
    assert (results[2][1] == dc.oracle_block(S, cw, ncw, ids, 1, enc_key=enc_b)).all()
    # the snapshot used last is now A's again: a call with A is confirmed
    before = X.query("fin_item_launches")
    assert (kc.run(X, S, mem, cw, ncw, ids, key=held(key_a)) == results[0]).all() and X.query("fin_item_launches") == before + 1
    X.close(), X0.close()
