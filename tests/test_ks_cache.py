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
    kc.check_enc_key_overwritten_in_place(orc, api, emu_lib, mem, small, monkeypatch)


def test_key_replaced_or_added(orc, api, emu_lib, mem, small, monkeypatch):
    kc.check_key_replaced_or_added(orc, api, emu_lib, mem, small, monkeypatch)


def test_two_key_sets_and_a_destroyed_one(orc, api, emu_lib, mem, small, monkeypatch):
    kc.check_two_key_sets_and_a_destroyed_one(orc, api, emu_lib, mem, small, monkeypatch)


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
    kc.check_budget_of_two_entries(orc, api, emu_lib, mem, small, monkeypatch)


def test_goes_with_the_block_tables_and_clearing(orc, api, emu_lib, mem, small, monkeypatch):
    kc.check_goes_with_the_block_tables_and_clearing(orc, api, emu_lib, mem, small, monkeypatch)


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
