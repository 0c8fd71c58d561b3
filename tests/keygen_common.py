"""Key generation and encryption from a seed: what tests/test_keygen_emu.py (emulator, numpy memory) and tests/test_gpu_keygen.py
(gfx950, torch memory) share.

The sampler is restated here from its prose definition with hashlib.shake_128 and struct only; expected key and
ciphertext words are composed from that restatement with the oracle's ntt_fwd / ntt_inv and Python integers.  Nothing here shares code
with the product.  Every comparison is exact word equality unless it says otherwise.

    SHAKE128( seed[32] || u8 purpose || LE32 elt || LE32 index || u8 kind || LE32 limb || LE32 chunk ), little-endian 64-bit words;
    one chunk = 64 consecutive coefficients
    noise    one word per coefficient: popcount(w & 0x1fffff) - popcount((w >> 21) & 0x1fffff)
    ternary  the 32 two-bit fields of a word, low to high; 3 is rejected; value = field - 1; first 64 accepted
    uniform  w & (2^bitlen(q) - 1), accepted below q; first 64 accepted
"""
import hashlib
import struct

import numpy as np
import pytest

SECRET, PUBLIC, RELIN, GALOIS, ENCRYPT = 1, 2, 3, 4, 5
TERNARY, NOISE, UNIFORM = 1, 2, 3
SEED = bytes(range(32))
SEED2 = bytes((7 * i + 3) % 256 for i in range(32))


# ---- the restatement ----
def _words(seed, purpose, elt, index, kind, limb, nchunks, nwords):
    pre = bytes(seed) + struct.pack("<BIIBI", purpose, elt, index, kind, limb)
    assert len(pre) == 46
    buf = b"".join(hashlib.shake_128(pre + struct.pack("<I", c)).digest(8 * nwords) for c in range(nchunks))
    return np.frombuffer(buf, dtype="<u8").reshape(nchunks, nwords)


def _first64(draw, nwords):
    """draw(nwords) -> (values [chunks][m], accepted [chunks][m], candidates per word); the first 64 accepted values of every chunk and
    the number of words the chunk consumed.  The squeeze is unbounded: the request doubles until every chunk has its 64."""
    while True:
        vals, ok, per_word = draw(nwords)
        cs = np.cumsum(ok, axis=1)
        if (cs[:, -1] >= 64).all():
            out = vals[ok & (cs <= 64)].reshape(vals.shape[0], 64)
            used = (np.argmax(cs >= 64, axis=1) // per_word) + 1
            return out, used
        nwords *= 2


def small_poly(seed, purpose, elt, index, kind, n, limb=0):
    """one ternary or noise polynomial as signed integers [n]"""
    assert kind in (TERNARY, NOISE) and n % 64 == 0
    if kind == NOISE:
        w = _words(seed, purpose, elt, index, kind, limb, n // 64, 64)
        lo, hi = w & np.uint64(0x1FFFFF), (w >> np.uint64(21)) & np.uint64(0x1FFFFF)
        pop = lambda v: np.unpackbits(v.astype("<u8").view(np.uint8).reshape(v.shape + (8,)), axis=-1).sum(axis=-1).astype(np.int64)
        return (pop(lo) - pop(hi)).reshape(n)

    def draw(nwords):
        w = _words(seed, purpose, elt, index, kind, limb, n // 64, nwords)
        f = ((w[:, :, None] >> (2 * np.arange(32, dtype=np.uint64))) & np.uint64(3)).reshape(n // 64, nwords * 32).astype(np.int64)
        return f - 1, f != 3, 32
    return _first64(draw, 8)[0].reshape(n)


def uniform_poly(seed, purpose, elt, index, limb, q, n, with_used=False):
    """one uniform polynomial below q as uint64 [n] (and the words every chunk consumed)"""
    mask = np.uint64((1 << int(q).bit_length()) - 1)

    def draw(nwords):
        v = _words(seed, purpose, elt, index, UNIFORM, limb, n // 64, nwords) & mask
        return v, v < np.uint64(q), 1
    out, used = _first64(draw, 84)
    return (out.reshape(n), used) if with_used else out.reshape(n)


def residues(small, q):
    return np.array([int(v) % int(q) for v in small], dtype=np.uint64)


def centred(v, q):
    return np.array([int(x) - int(q) if int(x) > int(q) // 2 else int(x) for x in v], dtype=np.int64)


def sanity():
    """seed-independent checks of the restatement itself (CPU, once): bytes(range(32)), purposes 1 and 2, 32768 coefficients each"""
    n = 32768
    tern = small_poly(SEED, SECRET, 0, 0, TERNARY, n)
    freq = [float((tern == v).mean()) for v in (-1, 0, 1)]
    noise = small_poly(SEED, PUBLIC, 0, 0, NOISE, n)
    return dict(freq=freq, var=float(noise.var()), mean=float(noise.mean()), lo=int(noise.min()), hi=int(noise.max()))


# ---- composing expected words (Python integers in object arrays + the oracle's transforms) ----
def _obj(a):
    return np.array([int(v) for v in np.asarray(a).reshape(-1)], dtype=object).reshape(np.asarray(a).shape)


def _u64(a):
    return np.array([int(v) for v in a], dtype=np.uint64)


def galois_coeff(a, elt, q, logn):
    """GaloisTool::apply_galois on coefficients: out[i * elt mod N] = +-a[i], the sign flips where i * elt mod 2N >= N"""
    n = 1 << logn
    i = np.arange(n, dtype=np.int64)
    raw = i * int(elt)
    neg = ((raw >> logn) & 1).astype(bool)
    v = _obj(a)
    v[neg] = (int(q) - v[neg]) % int(q)
    out = np.zeros(n, dtype=object)
    out[raw & (n - 1)] = v
    return _u64(out)


def expected_secret(O, seed):
    s = small_poly(seed, SECRET, 0, 0, TERNARY, O.n)
    return s, np.stack([O.ntt_fwd(j, residues(s, O.q[j])) for j in range(O.K)])


def new_key_relin(O, sk):
    return np.stack([_u64(_obj(sk[j]) * _obj(sk[j]) % O.q[j]) for j in range(O.K)])


def new_key_galois(O, sk, elt):
    return np.stack([O.ntt_fwd(j, galois_coeff(O.ntt_inv(j, sk[j]), elt, O.q[j], O.logn)) for j in range(O.K)])


def expected_enc_zero(O, sk, seed, purpose, elt, D, new_key=None, only_k1=False):
    """[D][2][K][N]: (-(a s + e) (+ (q_sp mod q_I) new_key[I] on limb I), a) per digit; also the noise polynomials [D][N]"""
    n, K = O.n, O.K
    out = np.zeros((D, 2, K, n), np.uint64)
    noise = []
    for I in range(D):
        e = None if only_k1 else small_poly(seed, purpose, elt, I, NOISE, n)
        noise.append(e)
        for j in range(K):
            q = O.q[j]
            a = uniform_poly(seed, purpose, elt, I, j, q, n)
            out[I, 1, j] = a
            if only_k1:
                continue
            ehat = O.ntt_fwd(j, residues(e, q))
            c0 = (-(_obj(a) * _obj(sk[j]) + _obj(ehat))) % q
            if new_key is not None and j == I:
                c0 = (c0 + (O.q[K - 1] % q) * _obj(new_key[I])) % q
            out[I, 0, j] = _u64(c0)
    return out, noise


def check_structure(O, sk, key, new_key, noise):
    """k0 + k1 s - [j = I] (q_sp mod q_I) new_key, inverse-transformed and centred, is the same small polynomial on every limb: -e"""
    K = O.K
    for I in range(key.shape[0]):
        for j in range(K):
            q = O.q[j]
            v = _obj(key[I, 0, j]) + _obj(key[I, 1, j]) * _obj(sk[j])
            if new_key is not None and j == I:
                v = v - (O.q[K - 1] % q) * _obj(new_key[I])
            small = centred(O.ntt_inv(j, _u64(v % q)), q)
            assert (small == -noise[I]).all(), (I, j)


def expected_encrypt(O, pk, plain, seed, b):
    n, L = O.n, O.L
    u = small_poly(seed, ENCRYPT, 0, b, TERNARY, n)
    ct = np.zeros((2, L, n), np.uint64)
    for k in range(2):
        e = small_poly(seed, ENCRYPT, 0, b, NOISE, n, limb=k)
        for j in range(L):
            q = O.q[j]
            prod = O.ntt_inv(j, _u64(_obj(O.ntt_fwd(j, residues(u, q))) * _obj(pk[k, j]) % q))
            ct[k, j] = _u64((_obj(prod) + _obj(residues(e, q))) % q)
    return O.add_plain(ct, plain)


# ---- checks against a context (X: api.Context on the emulator or the gfx950 library; mem: HostMem / TorchMem) ----
def check_sampler(X, O, mem, seed=SEED, min_words=0):
    """hhe_sample_poly for the three kinds under the key-level primes, and a uniform draw at a modulus offset; returns the most words a
    uniform chunk consumed"""
    n, K = O.n, O.K
    out = mem.empty((K, n))
    for kind, purpose, elt, index in ((TERNARY, SECRET, 0, 0), (NOISE, RELIN, 0, 2), (NOISE, GALOIS, 2 * n - 1, 1), (TERNARY, ENCRYPT, 0, 70000)):
        X.sample_poly(seed, purpose, elt, index, kind, 0, K, out)
        s = small_poly(seed, purpose, elt, index, kind, n)
        got = mem.to_host(out)
        for j in range(K):
            assert (got[j] == residues(s, O.q[j])).all(), (kind, purpose, j)
    most = 0
    X.sample_poly(seed, GALOIS, 3, 1, UNIFORM, 0, K, out)
    got = mem.to_host(out)
    for j in range(K):
        ref, used = uniform_poly(seed, GALOIS, 3, 1, j, O.q[j], n, with_used=True)
        most = max(most, int(used.max()))
        assert (got[j] == ref).all(), j
    if K > 1:  # the limb of a uniform draw is the modulus index, whatever the offset of the request
        X.sample_poly(seed, PUBLIC, 0, 0, UNIFORM, 1, K - 1, out)
        got = mem.to_host(out)
        for j in range(1, K):
            assert (got[j - 1] == uniform_poly(seed, PUBLIC, 0, 0, j, O.q[j], n)).all(), j
    assert most >= min_words, most
    return most


class DeviceKeys:
    """secret and public key of a context made on the device, and their host copies"""

    def __init__(self, X, O, mem, seed=SEED):
        self.X, self.O, self.mem, self.seed = X, O, mem, seed
        self.d_sk, self.d_pk = mem.empty((O.K, O.n)), mem.empty((2, O.K, O.n))
        X.keygen_secret(seed, self.d_sk)
        X.keygen_public(self.d_sk, seed, self.d_pk)
        self.sk, self.pk = mem.to_host(self.d_sk), mem.to_host(self.d_pk)

    def keyset(self, elts, seed=None, relin=True):
        ks = self.X.keyset()
        if relin:
            ks.generate_relin(self.d_sk, seed or self.seed)
        ks.generate_galois(self.d_sk, seed or self.seed, elts)
        return ks


def oracle_gk(orc, ks, elts):
    return orc.GaloisKeys(list(elts), np.stack([ks.get_galois(int(e)) for e in elts]))


def third_element(O):
    return O.galois_elt(-1)


def check_keys_words(X, O, mem, seed=SEED, full_elts=None):
    """secret, public, relinearization and Galois keys word for word, and the structural form of what is read back"""
    elts = [3, 2 * O.n - 1, third_element(O)] if full_elts is None else list(full_elts)
    D = DeviceKeys(X, O, mem, seed)
    s, sk = expected_secret(O, seed)
    assert (D.sk == sk).all()
    pk, pk_noise = expected_enc_zero(O, sk, seed, PUBLIC, 0, 1)
    assert (D.pk == pk[0]).all()
    check_structure(O, sk, D.pk[None], None, pk_noise)
    ks = D.keyset(elts)
    assert ks.has_relin() and all(ks.has_galois(e) for e in elts)
    nk = new_key_relin(O, sk)
    ref, noise = expected_enc_zero(O, sk, seed, RELIN, 0, O.L, nk)
    got = ks.get_relin()
    assert (got == ref).all()
    check_structure(O, sk, got, nk, noise)
    for e in elts:
        nk = new_key_galois(O, sk, e)
        ref, noise = expected_enc_zero(O, sk, seed, GALOIS, e, O.L, nk)
        got = ks.get_galois(e)
        assert (got == ref).all(), e
        check_structure(O, sk, got, nk, noise)
    ks.close()
    return D


def slots_of(O, sk, ct):
    return O.decode(O.decrypt(sk, ct))


def rot_rows(vals, step):
    h = len(vals) // 2
    return np.concatenate([np.roll(vals[:h], -step), np.roll(vals[h:], -step)])


def check_keys_behave(X, O, orc, mem, seed=SEED):
    """the named-set calls with generated keys equal the oracle called with the words read back, and decrypt to the rotated or
    multiplied slots"""
    D = DeviceKeys(X, O, mem, seed)
    key_step, other_step = 1, 3          # step 3 has no key: NAF chain over the keys of the set
    elts = [O.galois_elt(key_step), O.galois_elt(-1), O.galois_elt(4), O.galois_elt(0)]
    ks = D.keyset(elts)
    gk, rk = oracle_gk(orc, ks, elts), ks.get_relin()
    rng = np.random.default_rng(5)
    vals = rng.integers(0, 256, O.n).astype(np.uint64)
    ct = O.encrypt(D.pk, O.encode(vals), 21)
    assert (slots_of(O, D.sk, ct) == vals).all()
    d_ct, d_out = mem.to_dev(ct[None]), mem.empty((1,) + O.ct_shape)
    for step in (key_step, other_step):
        X.rotate_rows(d_ct, step, d_out, 1, gk=ks)
        got = mem.to_host(d_out)[0]
        ref, nks = O.rotate_rows(ct, step, gk)
        assert nks == (1 if step == key_step else 2), (step, nks)
        assert (got == ref).all(), step
        assert (slots_of(O, D.sk, got) == rot_rows(vals, step)).all(), step
    X.rotate_columns(d_ct, d_out, 1, gk=ks)
    got = mem.to_host(d_out)[0]
    assert (got == O.rotate_columns(ct, gk)).all()
    h = O.n // 2
    assert (slots_of(O, D.sk, got) == np.concatenate([vals[h:], vals[:h]])).all()
    small = rng.integers(0, 16, O.n).astype(np.uint64)
    ct2 = O.encrypt(D.pk, O.encode(small), 22)
    d3, d_ct2 = mem.empty((1, 3, O.L, O.n)), mem.to_dev(ct2[None])
    X.multiply(d_ct, d_ct2, d3, 1)
    X.relinearize(d3, d_out, 1, rk=ks)
    got = mem.to_host(d_out)[0]
    assert (got == O.relinearize(O.multiply(ct, ct2), rk)).all()
    assert (slots_of(O, D.sk, got) == (vals * small) % np.uint64(O.t)).all()
    ks.close()


def check_life_cycle(X, X_other, O, orc, mem, api, S=None):
    """regeneration replaces the key and what was derived from it; failed lists leave the set as it was; get / set round trips"""
    D = DeviceKeys(X, O, mem, SEED)
    e1, em = O.galois_elt(1), O.galois_elt(-1)
    ks = D.keyset([e1, em])
    vals = np.arange(O.n, dtype=np.uint64) % np.uint64(251)
    ct = O.encrypt(D.pk, O.encode(vals), 23)
    d_ct, d_out = mem.to_dev(ct[None]), mem.empty((1,) + O.ct_shape)
    X.rotate_rows(d_ct, 1, d_out, 1, gk=ks)     # builds whatever the context derives from the key (Shoup quotients on the row kernel)
    first = mem.to_host(d_out)[0]
    old = {e: ks.get_galois(e) for e in (e1, em)}
    old_rk = ks.get_relin()
    assert (first == O.rotate_rows(ct, 1, orc.GaloisKeys([e1], old[e1][None]))[0]).all()
    # a list with an even element, or one >= 2N: nothing changes
    for bad in ([e1, 4], [em, 2 * O.n + 1], [2 * O.n]):
        with pytest.raises(api.HheError) as ei:
            ks.generate_galois(D.d_sk, SEED2, bad)
        assert ei.value.code == api.ERR_INVALID
        for e in (e1, em):
            assert (ks.get_galois(e) == old[e]).all()
        assert not ks.has_galois(4) and (ks.get_relin() == old_rk).all()
    X.rotate_rows(d_ct, 1, d_out, 1, gk=ks)
    assert (mem.to_host(d_out)[0] == first).all()
    # another seed: the rotation's words are those of the new key
    ks.generate_galois(D.d_sk, SEED2, [e1])
    new = ks.get_galois(e1)
    assert (new != old[e1]).any() and (ks.get_galois(em) == old[em]).all()
    X.rotate_rows(d_ct, 1, d_out, 1, gk=ks)
    got = mem.to_host(d_out)[0]
    assert (got == O.rotate_rows(ct, 1, orc.GaloisKeys([e1], new[None]))[0]).all()
    assert (got != first).any() and (slots_of(O, D.sk, got) == rot_rows(vals, 1)).all()
    # absent keys
    for call, code in ((lambda: ks.get_galois(O.galois_elt(4)), api.ERR_NO_GALOIS_KEY), (lambda: X.keyset().get_relin(), api.ERR_NO_RELIN_KEY)):
        with pytest.raises(api.HheError) as ei:
            call()
        assert ei.value.code == code
    # set then get
    ks2 = X.keyset()
    ks2.set_galois(e1, old[e1]).set_relin(old_rk)
    assert (ks2.get_galois(e1) == old[e1]).all() and (ks2.get_relin() == old_rk).all()
    # a set of another context is refused
    with pytest.raises(api.HheError) as ei:
        X_other.rotate_rows(d_ct, 1, d_out, 1, gk=ks)
    assert ei.value.code == api.ERR_INVALID
    ks.close(), ks2.close()


def check_regeneration_drops_keystreams(X, O, orc, mem):
    """a transciphering call after a regeneration into one of its sets evaluates its keystream again (needs N/2 >= 128 slots per row and
    a chain that decrypts is not required: only the counters are read)"""
    D = DeviceKeys(X, O, mem, SEED)
    elts = [O.galois_elt(s) for s in ([-1, 0] + ([128] if O.n // 2 != 128 else []))]
    ks = D.keyset(elts)
    key = np.array([(i * 2654435761 + 12345) % O.t for i in range(256)], dtype=np.uint64)
    d_plain, d_key = mem.to_dev(O.pasta_pack_key(key)[None]), mem.empty((1,) + O.ct_shape)
    X.encrypt(D.d_pk, d_plain, SEED, 1, d_key)
    cw = orc.pasta_encrypt(O.t, key, np.arange(128, dtype=np.uint64)).reshape(1, 128)
    out = mem.empty((1,) + O.ct_shape)
    counts = lambda: (X.query("transcipher_evaluated"), X.query("ks_cache_hits"))
    X.transcipher(d_key, cw, [128], [0], out, rk=ks, gk=ks)
    assert counts() == (1, 0)
    X.transcipher(d_key, cw, [128], [0], out, rk=ks, gk=ks)
    assert counts() == (0, 1)
    ks.generate_galois(D.d_sk, SEED2, [elts[0]])
    X.transcipher(d_key, cw, [128], [0], out, rk=ks, gk=ks)
    assert counts() == (1, 0)
    X.transcipher(d_key, cw, [128], [0], out, rk=ks, gk=ks)
    assert counts() == (0, 1)
    ks.generate_relin(D.d_sk, SEED2)
    X.transcipher(d_key, cw, [128], [0], out, rk=ks, gk=ks)
    assert counts() == (1, 0)
    got = mem.to_host(out)[0]
    ref = O.transcipher_block(mem.to_host(d_key)[0], ks.get_relin(), oracle_gk(orc, ks, elts), cw[0], 0)
    assert (got == ref).all()
    ks.close()


def check_encrypt(X, O, mem, seed=SEED, B=3, budget=True):
    """hhe_encrypt per item and broadcast against the composed expectation; items differ; hhe_decrypt returns the slots; the noise
    budget is positive and at most 3 bits below the oracle's own encryption of the same plaintext under the same public key"""
    D = DeviceKeys(X, O, mem, seed)
    rng = np.random.default_rng(9)
    vals = rng.integers(0, min(O.t, 1 << 62), (B, O.n), dtype=np.uint64)
    plain = np.stack([O.encode(v) for v in vals])
    d_plain, d_out, d_vals = mem.to_dev(plain), mem.empty((B,) + O.ct_shape), mem.empty((B, O.n))
    X.encrypt(D.d_pk, d_plain, SEED2, B, d_out)
    got = mem.to_host(d_out)
    for b in range(B):
        assert (got[b] == expected_encrypt(O, D.pk, plain[b], SEED2, b)).all(), b
    X.decrypt(D.sk, d_out, B, d_vals)
    assert (mem.to_host(d_vals) == vals).all()
    if budget:
        for b in range(B):
            mine, theirs = O.noise_budget(D.sk, got[b]), O.noise_budget(D.sk, O.encrypt(D.pk, plain[b], 31 + b))
            assert mine > 0 and mine >= theirs - 3, f"budget of the device ciphertext {mine} bits, of the oracle's {theirs} bits"
    X.encrypt(D.d_pk, mem.to_dev(plain[1:2]), SEED2, B, d_out, bcast=True)
    bc = mem.to_host(d_out)
    for b in range(B):
        assert (bc[b] == expected_encrypt(O, D.pk, plain[1], SEED2, b)).all(), b
    assert (bc[1] == got[1]).all()
    for a in range(B):
        for b in range(a + 1, B):
            assert (bc[a] != bc[b]).any()
    X.decrypt(D.sk, d_out, B, d_vals)
    assert (mem.to_host(d_vals) == vals[1]).all()


def check_full_flow(X, O, orc, mem, use_bsgs=False):
    """no oracle key anywhere: device keys, device encryption of the packed PASTA key, the plain cipher, transciphering with the
    generated sets, decryption -- and the ciphertext words equal the oracle's transcipher_block given the words read back"""
    D = DeviceKeys(X, O, mem, SEED)
    elts = [O.galois_elt(s) for s in ([-1, 0] + ([128] if O.n // 2 != 128 else []))]
    ks = D.keyset(elts, SEED2)
    key = np.array([(i * 2654435761 + 12345) % O.t for i in range(256)], dtype=np.uint64)
    d_enc_key = mem.empty((1,) + O.ct_shape)
    X.encrypt(D.d_pk, mem.to_dev(O.pasta_pack_key(key)[None]), SEED2, 1, d_enc_key)
    pt = np.array([(7 * i + 3) % 256 for i in range(128)], dtype=np.uint64)
    d_sym = mem.empty((1, 128))
    X.plain_crypt(key, mem.to_dev(pt[None]), 1, 128, d_sym)
    cw = mem.to_host(d_sym)
    assert (cw[0] == orc.pasta_encrypt(O.t, key, pt)).all()
    out, d_vals = mem.empty((1,) + O.ct_shape), mem.empty((1, O.n))
    X.transcipher(d_enc_key, cw, [128], [0], out, use_bsgs=use_bsgs, rk=ks, gk=ks)
    got = mem.to_host(out)[0]
    ref = O.transcipher_block(mem.to_host(d_enc_key)[0], ks.get_relin(), oracle_gk(orc, ks, elts), cw[0], 0, use_bsgs)
    assert (got == ref).all()
    X.decrypt(D.sk, out, 1, d_vals)
    assert (mem.to_host(d_vals)[0, :128] == pt).all()
    ks.close()
