"""PASTA under a caller's nonce: what tests/test_nonce_emu.py (emulator) and tests/test_gpu_nonce.py share.

The truth of the homomorphic side is written once, here: PASTA_SEAL::decomposition (pasta_3_seal.cpp:106-172, with `diagonal`
:370-413 and `babystep_giantstep` :267-366) restated in Python over the oracle's encode, rotate_rows, rotate_columns, multiply_plain,
add, add_plain, negate, multiply and relinearize, with the matrices of orc.pasta_block_randomness(t, block, nonce) -- as
tests/affine_common.py restates packed_matMul.  The restatement is held to orc.transcipher_block at nonce 123456789, word for word
(check_restatement), and is then the truth at other nonces.  Every comparison is exact equality of all ciphertext words.  One
keystream ciphertext is composed per distinct (setup, pair, method) and every item is finished from it; nothing writes to it.

The plain side is held to the reference itself through tests/golden/pasta_plain_nonce.json (tests/golden/make_pasta_nonce_golden.py)."""
import hashlib
import json
import os

import numpy as np

import dedup_common as dc

HERE = os.path.dirname(os.path.abspath(__file__))
T = 128
FIXED = 123456789
NA, NB = 0x0102030405060708, 2**64 - 1  # distinct bytes catch a byte order; all ones the end of the range
# (nonce, counter) of the items of the transciphering checks: a pair twice, one nonce under two counters, a counter past 32 bits
ITEMS = [(NA, 0), (NB, 0), (NA, 0), (NA, 1), (NB, 2**32 + 5)]
ITEMS_NCW = [128, 7, 40, 1, 100]
MODULI = (65537, 8088322049, 1096486890805657601)


def golden():
    return json.load(open(os.path.join(HERE, "golden", "pasta_plain_nonce.json")))["randomness"]


def demo_key(t):
    return np.array([(i * 2654435761 + 12345) % t for i in range(256)], dtype=np.uint64)


# ---------------------------------------------------------------- the restatement
def _diagonals(m1, m2, i):
    j = np.arange(T)
    return m1[j, (j + T - i) % T], m2[j, (j + T - i) % T]


def _diagonal(S, state, m1, m2):
    """PASTA_SEAL::diagonal (pasta_3_seal.cpp:370-413)"""
    O, half = S.O, S.n // 2
    if half != T:
        state = O.add(state, O.rotate_rows(state, T, S.gk)[0])
    total = None
    for i in range(T):
        vec = np.zeros(half + T, np.uint64)
        vec[:T], vec[half:half + T] = _diagonals(m1, m2, i)
        if i:
            state = O.rotate_rows(state, -1, S.gk)[0]
        prod = O.multiply_plain(state, O.encode(vec))
        total = prod if total is None else O.add(total, prod)
    return total


def _bsgs(S, state, m1, m2, n1=16, n2=8):
    """PASTA_SEAL::babystep_giantstep (pasta_3_seal.cpp:267-366)"""
    O, n, half = S.O, S.n, S.n // 2
    plains = []
    for i in range(T):
        k = i // n1
        d1, d2 = _diagonals(m1, m2, i)
        a, b = np.zeros(n, np.uint64), np.zeros(half, np.uint64)
        a[:T], b[:T] = np.roll(d1, -k * n1), np.roll(d2, -k * n1)  # std::rotate(begin, begin + k*N1, end) (:297-301)
        if half != T:  # :304-317
            for m in range(k * n1):
                a[half - 1 - m], a[T - 1 - m] = a[T - 1 - m], 0
                b[half - 1 - m], b[T - 1 - m] = b[T - 1 - m], 0
        a[half:] = b
        plains.append(O.encode(a))
    if half != T:
        state = O.add(state, O.rotate_rows(state, T, S.gk)[0])
    rot = [state]
    for j in range(1, n1):
        rot.append(O.rotate_rows(rot[j - 1], -1, S.gk)[0])
    outer = None
    for k in range(n2):
        inner = O.multiply_plain(rot[0], plains[k * n1])
        for j in range(1, n1):
            inner = O.add(inner, O.multiply_plain(rot[j], plains[k * n1 + j]))
        outer = inner if k == 0 else O.add(outer, O.rotate_rows(inner, -k * n1, S.gk)[0])
    return outer


_keystreams = {}


def keystream(orc, S, nonce, block, use_bsgs=False):
    """the state of PASTA_SEAL::decomposition (pasta_3_seal.cpp:123-159) in front of its `add cipher`, under (nonce, block)"""
    key = (id(S), nonce, block, bool(use_bsgs))
    if key in _keystreams:
        return _keystreams[key][1]
    O, half = S.O, S.n // 2
    mats, rcs = orc.pasta_block_randomness(S.t, block, nonce)
    state = S.enc_key
    for r in range(4):
        state = (_bsgs if use_bsgs else _diagonal)(S, state, mats[r, 0], mats[r, 1])  # matmul (:251-263)
        vec = np.zeros(half + T, np.uint64)
        vec[:T], vec[half:half + T] = rcs[r, 0], rcs[r, 1]
        state = O.add_plain(state, O.encode(vec))  # add_rc (:205-211)
        tmp = O.add(O.rotate_columns(state, S.gk), state)  # mix (:417-423)
        state = O.add(state, tmp)
        if r == 3:
            break
        if r == 2:  # sbox_cube (:215-218)
            sq = O.relinearize(O.multiply(state, state), S.rk)
            state = O.relinearize(O.multiply(sq, state), S.rk)
        else:  # sbox_feistel (:222-247)
            vec = np.zeros(half + T, np.uint64)
            vec[1:T], vec[half + 1:half + T] = 1, 1
            tmp = O.multiply_plain(O.rotate_rows(state, -1, S.gk)[0], O.encode(vec))
            state = O.add(state, O.relinearize(O.multiply(tmp, tmp), S.rk))
    state.setflags(write=False)
    _keystreams[key] = (S, state)  # S kept alive: its id is the key
    return state


def item_truth(orc, S, cw_row, count, nonce, block, use_bsgs=False):
    """`add cipher` (:161-169): Enc(c_b) - KS"""
    O = S.O
    return O.add_plain(O.negate(keystream(orc, S, nonce, block, use_bsgs)), O.encode(cw_row[:count]))


def check_restatement(orc, S):
    """the restatement equals orc.transcipher_block at the reference's nonce, both methods"""
    cw = dc.words(S, 2, 5)
    for bsgs, (blk, cnt) in ((False, (1, 128)), (True, (1, 9))):
        want = S.O.transcipher_block(S.enc_key, S.rk, S.gk, cw[0, :cnt], blk, use_bsgs=bsgs)
        assert (item_truth(orc, S, cw[0], cnt, FIXED, blk, bsgs) == want).all(), ("restatement differs from the oracle", bsgs)


# ---------------------------------------------------------------- contexts and calls
def light_ctx(orc, api, lib, t, logn=10):
    """a context at N = 1024 under plain modulus t, as tests/plain_modulus_common.py builds them (no keys)"""
    import plain_modulus_common as pm
    q = pm.primes_near(orc, 1 << logn, [50] * 3)
    return api.Context(logn, q, t, lib=lib)


def run(X, S, mem, cw, ncw, pairs, use_bsgs=False, key=None):
    out = mem.empty((len(pairs),) + S.O.ct_shape)
    X.transcipher(mem.to_dev(S.enc_key) if key is None else key, cw, ncw, [p[1] for p in pairs], out, use_bsgs=use_bsgs,
                  nonces=[p[0] for p in pairs])
    return mem.to_host(out)


def run_old(X, S, mem, cw, ncw, ids, use_bsgs=False):
    out = mem.empty((len(ids),) + S.O.ct_shape)
    X.transcipher(mem.to_dev(S.enc_key), cw, ncw, ids, out, use_bsgs=use_bsgs)
    return mem.to_host(out)


# ---------------------------------------------------------------- 1. device randomness
def check_device_randomness(orc, api, lib, mem, t):
    """hhe_pasta3_block_randomness_dev for 1, 64 and 65 pairs in one call (the XOF workgroup is 64 lanes): every pair equals the
    oracle, the golden pairs among them equal the reference, and another order gives the same words per pair"""
    gold = [c for c in golden() if c["t"] == t]
    assert len(gold) == 16
    pairs = [(c["nonce"], c["block"]) for c in gold]
    rng = np.random.default_rng(t % 1000)
    while len(pairs) < 65:
        pairs.append((int(rng.integers(0, 2**63)) * 2 + 1, int(rng.integers(0, 2**63))))
    want = {p: orc.pasta_block_randomness(t, p[1], p[0]) for p in pairs}
    X = light_ctx(orc, api, lib, t)
    got = {}
    for sel in (pairs[:1], pairs[:64], pairs, pairs[::-1]):
        mats, rcs = mem.empty((len(sel), 4, 2, T, T)), mem.empty((len(sel), 4, 2, T))
        X.block_randomness_dev([p[0] for p in sel], [p[1] for p in sel], mats, rcs)
        hm, hr = mem.to_host(mats), mem.to_host(rcs)
        for i, p in enumerate(sel):
            assert (hm[i] == want[p][0]).all() and (hr[i] == want[p][1]).all(), ("device randomness differs from the oracle", len(sel), i, p)
        got = {p: (hm[i], hr[i]) for i, p in enumerate(sel)}
    for c in gold:
        m, r = got[(c["nonce"], c["block"])]
        assert hashlib.sha256(np.ascontiguousarray(m).tobytes()).hexdigest() == c["mats_sha256"]
        assert hashlib.sha256(np.ascontiguousarray(r).tobytes()).hexdigest() == c["rcs_sha256"]
    X.close()


def check_oracle_against_golden(orc, api, lib):
    """the oracle and the product's host generator with nonce arguments against the reference's recorded words"""
    for c in golden():
        t, nonce, blk = c["t"], c["nonce"], c["block"]
        mats, rcs = orc.pasta_block_randomness(t, blk, nonce)
        assert hashlib.sha256(mats.tobytes()).hexdigest() == c["mats_sha256"] and hashlib.sha256(rcs.tobytes()).hexdigest() == c["rcs_sha256"]
        ks = orc.pasta_keystream(t, demo_key(t), blk, nonce)
        assert hashlib.sha256(ks.tobytes()).hexdigest() == c["keystream_sha256"]
        pm, pr = api.block_randomness(t, blk, lib=lib, nonce=nonce)
        assert (pm == mats).all() and (pr == rcs).all()


# ---------------------------------------------------------------- 2. client end
def check_client(orc, api, lib, mem, t):
    gold = [c for c in golden() if c["t"] == t]
    key = demo_key(t)
    X = light_ctx(orc, api, lib, t)
    for c in gold:
        ks = mem.empty((1, T))
        X.plain_keystream(key, c["block"], 1, ks, nonce=c["nonce"])
        assert hashlib.sha256(np.ascontiguousarray(mem.to_host(ks)[0]).tobytes()).hexdigest() == c["keystream_sha256"], (t, c["nonce"], c["block"])
    # a run of counters under one nonce, across 2^32
    ks = mem.empty((3, T))
    X.plain_keystream(key, 2**32 - 1, 3, ks, nonce=NA)
    for i, row in enumerate(mem.to_host(ks)):
        assert (row == orc.pasta_keystream(t, key, 2**32 - 1 + i, NA)).all()
    # the default nonce gives the words of the old calls
    a, b = mem.empty((2, T)), mem.empty((2, T))
    X.plain_keystream(key, 5, 2, a)
    X.plain_keystream(key, 5, 2, b, nonce=FIXED)
    assert (mem.to_host(a) == mem.to_host(b)).all()
    # records: two records under two nonces differ, decrypt inverts encrypt, the default nonce repeats the old call
    nwords = 200
    pt = np.random.default_rng(3).integers(0, t, size=(3, nwords), dtype=np.uint64)
    pt[1] = pt[0]
    d_pt, ct, back, old = mem.to_dev(pt), mem.empty(pt.shape), mem.empty(pt.shape), mem.empty(pt.shape)
    nonces = [NA, NB, 7]
    X.plain_crypt(key, d_pt, 3, nwords, ct, nonces=nonces)
    h = mem.to_host(ct)
    tt = np.uint64(t)
    for s in range(3):
        ksr = np.concatenate([orc.pasta_keystream(t, key, b, nonces[s]) for b in range(2)])[:nwords]
        assert (h[s] == (pt[s] % tt + ksr) % tt).all(), ("record", s)  # both below t < 2^60: the sum fits
    assert not (h[0] == h[1]).all()
    X.plain_crypt(key, ct, 3, nwords, back, decrypt=True, nonces=nonces)
    assert (mem.to_host(back) == pt).all()
    X.plain_crypt(key, d_pt, 3, nwords, old)
    X.plain_crypt(key, d_pt, 3, nwords, ct, nonces=[FIXED] * 3)
    assert (mem.to_host(ct) == mem.to_host(old)).all()
    X.close()


# ---------------------------------------------------------------- 3. transciphering words
def check_words(orc, api, lib, mem, S, monkeypatch, use_bsgs, row_kernel, variants=True, **env):
    """every item equals the restatement; four distinct pairs; HHE_DEDUP=0 and both HHE_PUBLIC_DEVICE settings give the same words"""
    cw = dc.words(S, len(ITEMS), 21)
    truth = [item_truth(orc, S, cw[b], ITEMS_NCW[b], *ITEMS[b], use_bsgs) for b in range(len(ITEMS))]
    X = dc.make_ctx(api, lib, S, monkeypatch, HHE_PUBLIC_DEVICE=1, **env)
    assert X.query("row_kernel") == row_kernel and X.query("public_device") == 1
    r = run(X, S, mem, cw, ITEMS_NCW, ITEMS, use_bsgs)
    for b in range(len(ITEMS)):
        assert (r[b] == truth[b]).all(), f"item {b} differs from the restatement"
    assert X.query("transcipher_unique") == 4 and X.query("public_device_built") == 4 and X.query("transcipher_groups") == 1
    X.close()
    if not variants:
        return r
    X0 = dc.make_ctx(api, lib, S, monkeypatch, HHE_PUBLIC_DEVICE=0, **env)
    assert X0.query("public_device") == 0
    assert (run(X0, S, mem, cw, ITEMS_NCW, ITEMS, use_bsgs) == r).all()
    assert X0.query("transcipher_unique") == 4 and X0.query("public_device_built") == 0
    X0.close()
    Xd = dc.make_ctx(api, lib, S, monkeypatch, HHE_DEDUP=0, **env)
    assert (run(Xd, S, mem, cw, ITEMS_NCW, ITEMS, use_bsgs) == r).all() and Xd.query("transcipher_unique") == len(ITEMS)
    Xd.close()
    return r


# ---------------------------------------------------------------- 4. one cache
def check_one_cache(orc, api, lib, mem, S, monkeypatch, **env):
    """an old-entry call on counters [0, 1], then a new-entry call on (123456789, 0), (123456789, 1): the same entries"""
    cw, ncw = dc.words(S, 2, 22), [128, 50]
    X = dc.make_ctx(api, lib, S, monkeypatch, **env)
    r_old = run_old(X, S, mem, cw, ncw, [0, 1])
    entries, kept = X.query("block_cache_entries"), X.query("ks_cache_entries")
    assert entries == 2 and kept == 2
    r_new = run(X, S, mem, cw, ncw, [(FIXED, 0), (FIXED, 1)])
    assert (r_new == r_old).all()
    assert X.query("ks_cache_hits") == 2 and X.query("transcipher_evaluated") == 0 and X.query("block_cache_entries") == entries
    assert (r_old[1] == dc.oracle_block(S, cw, ncw, [0, 1], 1)).all()
    r_other = run(X, S, mem, cw[:1], ncw[:1], [(NA, 0)])  # a different nonce on counter 0 misses
    assert X.query("ks_cache_hits") == 0 and X.query("transcipher_evaluated") == 1 and X.query("block_cache_entries") == entries + 1
    assert not (r_other[0] == r_old[0]).all()
    assert (r_other[0] == item_truth(orc, S, cw[0], ncw[0], NA, 0)).all()
    r_back = run_old(X, S, mem, cw, ncw, [0, 1])  # ... and the other way round
    assert (r_back == r_old).all() and X.query("ks_cache_hits") == 2
    X.close()


# ---------------------------------------------------------------- 5. groups
GROUP_ITEMS = [(NA, 0), (NA, 1), (NA, 0), (NB, 0), (NA, 1), (NB, 2**32 + 5), (FIXED, 3)]  # 7 items, 5 distinct pairs
GROUP_NCW = [128, 30, 128, 128, 1, 100, 64]


def check_groups(orc, api, lib, mem, S, monkeypatch, **env):
    """a limit that two pairs fit: [(NA,0) (NA,1) (NA,0)] [(NB,0) (NA,1)] [(NB,2^32+5) (FIXED,3)] -- three groups, the words of the
    single-item calls, the cache within its limit; the old entry with counters under the fixed nonce stays one call"""
    cw = dc.words(S, len(GROUP_ITEMS), 23)
    X1 = dc.make_ctx(api, lib, S, monkeypatch, **env)
    single = []
    for b, p in enumerate(GROUP_ITEMS):
        single.append(run(X1, S, mem, cw[b:b + 1], GROUP_NCW[b:b + 1], [p])[0])
        assert X1.query("transcipher_groups") == 1
    per = X1.query("block_cache_bytes") // X1.query("block_cache_entries")
    X1.close()
    X = dc.make_ctx(api, lib, S, monkeypatch, **env)
    limit = 2 * per + per // 2
    X.set_block_cache_limit(limit)
    r = run(X, S, mem, cw, GROUP_NCW, GROUP_ITEMS)
    assert X.query("transcipher_groups") == 3
    for b in range(len(GROUP_ITEMS)):
        assert (r[b] == single[b]).all(), f"item {b} differs from its single-item call"
    assert 0 < X.query("block_cache_bytes") <= limit and X.query("block_cache_entries") == 2
    assert X.query("transcipher_unique") == 6  # summed over the groups: (NA,0) (NA,1) | (NB,0) (NA,1) | two more
    assert (r[5] == item_truth(orc, S, cw[5], GROUP_NCW[5], *GROUP_ITEMS[5])).all()
    # the old entry: one call whatever it needs, served over the limit, as before
    ids = [0, 1, 0, 2, 1, 3, 4]
    r_old = run_old(X, S, mem, cw, GROUP_NCW, ids)
    assert X.query("transcipher_groups") == 1 and X.query("transcipher_unique") == 5 and X.query("block_cache_entries") == 5
    assert X.query("block_cache_bytes") == 5 * per
    assert (r_old[6] == dc.oracle_block(S, cw, GROUP_NCW, ids, 6)).all()
    X.close()


# ---------------------------------------------------------------- 6. decompose
def check_decompose(orc, api, lib, mem, S, monkeypatch, **env):
    """three records under three nonces, a ragged last block: restatement + mask + flatten of the oracle"""
    nwords, nonces = 128 + 37, [NA, NB, 5]
    rec = np.random.default_rng(24).integers(0, S.t, size=(3, nwords), dtype=np.uint64)
    X = dc.make_ctx(api, lib, S, monkeypatch, **env)
    out = mem.empty((3,) + S.O.ct_shape)
    X.decompose(mem.to_dev(S.enc_key), rec, out, nonces=nonces)
    got = mem.to_host(out)
    for s in range(3):
        b0 = item_truth(orc, S, rec[s, :128], 128, nonces[s], 0)
        b1 = S.O.mask(item_truth(orc, S, rec[s, 128:], 37, nonces[s], 1), np.ones(37, np.uint64))
        assert (got[s] == S.O.flatten(np.stack([b0, b1]), S.gk)).all(), f"record {s}"
    assert X.query("transcipher_unique") == 6
    X.close()


# ---------------------------------------------------------------- 7. refusals
def check_refusals(orc, api, lib, mem, S, monkeypatch):
    """null nonce array, B = 0 and a missing Galois key: the codes of the old entries, the prefilled output untouched"""
    import ctypes as C
    X = dc.make_ctx(api, lib, S, monkeypatch)
    cw, ncw = dc.words(S, 1, 25), np.array([128], np.uint32)
    bi, nn = np.zeros(1, np.uint64), np.array([NA], np.uint64)
    fill = np.full((1,) + S.O.ct_shape, 0x5a5a, np.uint64)
    out, key = mem.to_dev(fill), mem.to_dev(S.enc_key)
    P = api._ptr

    def new(nonce, B, h=None):
        return lib.hhe_pasta3_transcipher_nonce_ks(h or X.h, None, None, P(key), P(cw), P(ncw), P(nonce), P(bi), C.c_size_t(B), 0, P(out))

    def old(index, B, h=None):
        return lib.hhe_pasta3_transcipher_ks(h or X.h, None, None, P(key), P(cw), P(ncw), P(index), C.c_size_t(B), 0, P(out))
    assert new(None, 1) == old(None, 1) == api.ERR_INVALID
    assert new(nn, 0) == old(bi, 0) == api.ERR_INVALID
    Y = api.Context(S.logn, S.q, S.t, lib=lib)
    Y.set_relin_key(S.rk)  # no Galois key at all
    assert new(nn, 1, Y.h) == old(bi, 1, Y.h) == api.ERR_NO_GALOIS_KEY
    assert lib.hhe_decompose_nonce_ks(X.h, None, None, None, P(key), P(cw), P(None), C.c_size_t(1), C.c_size_t(128), 1, P(out)) == api.ERR_INVALID
    assert lib.hhe_pasta3_prepare_tables(X.h, P(None), P(bi), C.c_size_t(1), 0, None) == api.ERR_INVALID
    assert (mem.to_host(out) == fill).all()
    assert X.query("block_cache_entries") == 0
    X.close(), Y.close()


def check_prepare_tables(orc, api, lib, mem, S, monkeypatch, **env):
    """hhe_pasta3_prepare_tables builds what a call would and reports it; the call then finds every table"""
    cw = dc.words(S, 2, 26)
    X = dc.make_ctx(api, lib, S, monkeypatch, HHE_PUBLIC_DEVICE=1, **env)
    pairs = [(NA, 0), (NA, 1), (NA, 0)]
    assert X.prepare_tables([p[0] for p in pairs], [p[1] for p in pairs]) == 2 and X.query("public_device_built") == 2
    assert X.query("block_cache_entries") == 2
    assert X.prepare_tables([NA], [1]) == 0
    r = run(X, S, mem, cw, [128, 5], [(NA, 1), (NA, 0)])
    assert X.query("public_device_built") == 0 and X.query("block_cache_entries") == 2
    assert (r[1] == item_truth(orc, S, cw[1], 5, NA, 0)).all()
    X.close()
