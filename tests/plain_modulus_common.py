"""Checks of the plain side at every plain modulus the reference lists (configs/config.cpp:19-26): 65537, 8088322049 (T33) and
1096486890805657601 (T60), shared by the emulator suite (numpy memory) and the GPU suite (torch memory).

The plaintext lift of multiply_plain (SEAL's multiply_plain_normal) maps a coefficient x in [0, t) to the residue of
its centred representative:  x mod q_j below (t + 1) / 2,  (x - t) mod q_j from there on.  For t below q_j that is x + (q_j - t)
without a reduction (the fast branch); for t above q_j the sum x + (Q - t) is decomposed per prime.  The oracle restates the
product's rule, so parity with it cannot tell whether the rule is right.  This module carries a second truth that shares no code
with either: lift_j and an O(N^2) negacyclic product in Python integers at the word level, and plain integers mod t behind a
decryption at the level of meaning.  Every comparison is exact equality."""
import numpy as np

import affine_common as ac
import parity_common as pc

T16, T33, T60 = 65537, 8088322049, 1096486890805657601


# ---- a. the lift, word level ----
def lift_j(x, t, q):
    """the lifted residue of a plaintext coefficient x in [0, t) modulo the coefficient prime q, in Python integers"""
    x, t, q = int(x), int(t), int(q)
    assert 0 <= x < t
    return (x - t) % q if x >= (t + 1) // 2 else x % q


def negacyclic_product(a, b, q):
    """a * b in Z_q[X] / (X^N + 1), schoolbook, Python integers in object arrays: c_k = sum_{i+j=k} a_i b_j - sum_{i+j=k+N} a_i b_j"""
    n = len(a)
    a = np.array([int(v) for v in a], dtype=object)
    b = np.array([int(v) for v in b], dtype=object)
    c = np.zeros(n, dtype=object)
    for i in range(n):
        if a[i]:
            c[i:] += a[i] * b[:n - i]
            c[:i] -= a[i] * b[n - i:]
    return np.array([int(v) % q for v in c], dtype=np.uint64)


def regime_of(t, q_data):
    """'fast' (t below every data prime), 'mid' (every q_j < t < 2 q_j) or 'slow' (t > 2 q_j for every j); None if the set is mixed"""
    if all(t < q for q in q_data):
        return "fast"
    if all(q < t < 2 * q for q in q_data):
        return "mid"
    if all(t > 2 * q for q in q_data):
        return "slow"
    return None


# name: (t, prime bit sizes or "default4096" = CoeffModulus::BFVDefault(4096), the regime the case is there for)
LIFT_CASES = {
    "t16_over_50": (T16, [50] * 3, "fast"),
    "t60_over_60": (T60, [60] * 3, "fast"),
    "t33_over_32": (T33, [32] * 3, "mid"),
    "t60_over_55": (T60, [55] * 3, "slow"),
    "t60_over_36_36_37": (T60, "default4096", "slow"),
    "t33_over_30": (T33, [30] * 3, "slow"),
}


def primes_near(orc, n, bits):
    """coeff_modulus_create(n, bits); where a size has too few primes = 1 mod 2n, the nearest size that has them"""
    for d in (0, 1, -1, 2, -2):
        try:
            return orc.coeff_modulus_create(n, [b + d for b in bits])
        except AssertionError:
            continue
    raise AssertionError(("no NTT primes near", bits, n))


def case_primes(orc, api, lib, n, spec):
    return api.bfv_default_coeff_modulus(4096, lib) if spec == "default4096" else primes_near(orc, n, spec)


def edge_values(t):
    return [0, 1, (t - 1) // 2, (t + 1) // 2, (t + 1) // 2 + 1, t - 2, t - 1]


def lift_plaintexts(t, n, seed=0):
    """[3][n] plaintext POLYNOMIALS (coefficients, not slots): drawn from the edges of the lift, all t - 1, all (t + 1) / 2"""
    rng = np.random.default_rng(seed)
    ev = np.array(edge_values(t), dtype=np.uint64)
    p0 = ev[rng.integers(0, len(ev), n)]
    p0[:len(ev)] = ev   # every edge value is there whatever the draw
    return np.stack([p0, np.full(n, t - 1, np.uint64), np.full(n, (t + 1) // 2, np.uint64)])


class LightSetup:
    """oracle, secret and public key only (seeds as conftest.Setup): enough for everything that needs no key switch"""

    def __init__(self, orc, logn, q, t):
        self.t, self.logn, self.n, self.q = int(t), logn, 1 << logn, [int(v) for v in q]
        self.O = orc.Oracle(logn, self.q, self.t)
        self.sk = self.O.keygen_secret(1)
        self.pk = self.O.keygen_public(self.sk, 2)


def check_lift_words(make_ctx, orc, api, lib, mem, name, logn=10):
    """hhe_multiply_plain, per item and broadcast, and the oracle's multiply_plain against lift_j + the schoolbook product, limb by
    limb, on one ciphertext.  The regime is asserted on the primes actually chosen."""
    t, spec, regime = LIFT_CASES[name]
    n = 1 << logn
    q = case_primes(orc, api, lib, n, spec)
    assert len(q) == 3   # L = 2
    assert regime_of(t, q[:-1]) == regime, (name, q)
    S = LightSetup(orc, logn, q, t)
    O = S.O
    rng = np.random.default_rng(5)
    ct = O.encrypt(S.pk, O.encode(rng.integers(0, t, n, dtype=np.uint64)), 10)
    plains = lift_plaintexts(t, n)
    P = len(plains)
    truth = np.zeros((P,) + O.ct_shape, np.uint64)
    for p in range(P):
        for j in range(O.L):
            lifted = [lift_j(x, t, q[j]) for x in plains[p]]
            for k in range(2):
                truth[p, k, j] = negacyclic_product(ct[k, j], lifted, q[j])
    for p in range(P):
        ref = O.multiply_plain(ct, plains[p])
        bad = [(k, j) for k in range(2) for j in range(O.L) if not (ref[k, j] == truth[p, k, j]).all()]
        assert not bad, (name, "oracle multiply_plain differs from the integer product; plaintext, (poly, limb):", p, bad)
    X = make_ctx(logn, q, t)
    d_cts = mem.to_dev(np.stack([ct] * P))
    out = mem.empty((P,) + O.ct_shape)
    X.multiply_plain(d_cts, mem.to_dev(plains), out, P)
    got = mem.to_host(out)
    for p in range(P):
        bad = [(k, j) for k in range(2) for j in range(O.L) if not (got[p, k, j] == truth[p, k, j]).all()]
        assert not bad, (name, "hhe_multiply_plain differs from the integer product; plaintext, (poly, limb):", p, bad)
    for p in range(P):
        X.multiply_plain(d_cts, mem.to_dev(plains[p:p + 1]), out, P, bcast=True)
        got = mem.to_host(out)
        for b in range(P):
            assert (got[b] == truth[p]).all(), (name, "broadcast hhe_multiply_plain differs from the integer product", p, b)
    X.close()


# ---- b. meaning, through decryption, at t > q_j ----
MEANING_T = T60
MEANING_BITS = 55
# the smallest count of 55-bit primes that leaves the oracle more than 10 bits after one transciphering: 23 and 24 bits on the two
# blocks of ragged_plaintext with 15 primes (14 data primes), 0 with 14
MEANING_PRIMES = 15
MEANING_DIM, MEANING_BSGS = 16, (4, 4)
_meaning = {}


def meaning_setup(orc, count=MEANING_PRIMES, logn=10):
    """T60 over `count` 55-bit primes at N = 1024, every default Galois key plus the steps of BSGS transciphering and of the affine
    layers; made once and shared (nothing writes to it)"""
    if (count, logn) not in _meaning:
        n = 1 << logn
        q = orc.coeff_modulus_create(n, [MEANING_BITS] * count)
        assert regime_of(MEANING_T, q) == "slow", q
        steps = sorted(set(ac.hand_steps(n, MEANING_DIM, *MEANING_BSGS)) | {-16 * k for k in range(1, 8)} | {-128, -256})
        _meaning[(count, logn)] = pc.setup_from_primes(orc, logn, q, MEANING_T, all_galois=True, extra_steps=steps)
    return _meaning[(count, logn)]


def decrypt_slots(S, words):
    return [int(v) for v in S.O.decode(S.O.decrypt(S.sk, words))]


def guard(S, ref):
    """the oracle's ciphertext still has noise budget: only then does a decryption mean anything"""
    budget = S.O.noise_budget(S.sk, ref)
    assert budget > 0, ("the oracle's ciphertext has no noise budget left", budget)
    return budget


def meaning_transcipher_ref(S, orc, pt):
    cw, ncw = S.sym_blocks(orc, pt)
    return cw, ncw, [S.O.transcipher_block(S.enc_key, S.rk, S.gk, cw[b, :ncw[b]], b) for b in range(len(ncw))]


def ragged_plaintext(t):
    """172 words = 128 + 44, spread over [0, t)"""
    return np.random.default_rng(60).integers(0, t, 172, dtype=np.uint64)


def check_meaning_product(X, S, mem):
    O, t, n = S.O, S.t, S.n
    rng = np.random.default_rng(61)
    a, b = rng.integers(0, t, n, dtype=np.uint64), rng.integers(0, t, n, dtype=np.uint64)
    b[:7] = edge_values(t)
    ct, pl = O.encrypt(S.pk, O.encode(a), 71), O.encode(b)
    guard(S, O.multiply_plain(ct, pl))
    out = mem.empty((1,) + O.ct_shape)
    X.multiply_plain(mem.to_dev(ct[None]), mem.to_dev(pl[None]), out, 1)
    assert decrypt_slots(S, mem.to_host(out)[0]) == [int(x) * int(y) % t for x, y in zip(a, b)]


def check_meaning_mask(X, S, mem, count=44):
    O, t, n = S.O, S.t, S.n
    rng = np.random.default_rng(62)
    a, mv = rng.integers(0, t, n, dtype=np.uint64), rng.integers(0, t, count, dtype=np.uint64)
    mv[:7] = edge_values(t)
    ct = O.encrypt(S.pk, O.encode(a), 72)
    guard(S, O.mask(ct, mv))
    out = mem.empty((1,) + O.ct_shape)
    X.mask(mem.to_dev(ct[None]), mv, out, 1)
    assert decrypt_slots(S, mem.to_host(out)[0]) == [int(a[i]) * int(mv[i]) % t if i < count else 0 for i in range(n)]


def check_meaning_affine(X, S, mem, bsgs):
    O, t, dim = S.O, S.t, MEANING_DIM
    M, bias = ac.seeded_matrix(t, dim, 63)
    cts, xs = ac.inputs(S, dim, 2, seed=3)
    refs = [ac.packed_affine_ref(O, S.gk, M, cts[b], bias, bsgs) for b in range(2)]
    for r in refs:
        guard(S, r)
    mat = X.matrix(M, bias=bias, bsgs=bsgs)
    out = mem.empty((2,) + O.ct_shape)
    X.packed_affine(mem.to_dev(cts), mat, out, 2)
    got = mem.to_host(out)
    mat.close()
    for b in range(2):
        assert decrypt_slots(S, got[b])[:dim] == ac.plain_affine(M, xs[b], bias, t), (bsgs, b)


def check_meaning_fc_row(X, S, mem, n_in=9):
    O, t = S.O, S.t
    rng = np.random.default_rng(64)
    v, w = rng.integers(0, 4, n_in), rng.integers(-8, 9, n_in)
    vi, wc = O.encrypt(S.pk, O.encode(v), 73), O.encrypt(S.pk, O.encode(w % t), 74)
    guard(S, O.fc_row(vi, wc, S.rk, S.gk, n_in)[0])
    out = mem.empty((1,) + O.ct_shape)
    X.fc_row(mem.to_dev(vi[None]), mem.to_dev(wc[None]), 1, n_in, out, 1, relin_slot=0, default_galois_only=False)
    assert decrypt_slots(S, mem.to_host(out)[0])[n_in - 1] == sum(int(x) * int(y) for x, y in zip(v, w)) % t


def check_meaning_transcipher(X, S, orc, mem):
    pt = ragged_plaintext(S.t)
    cw, ncw, refs = meaning_transcipher_ref(S, orc, pt)
    assert list(ncw) == [128, 44]
    for r in refs:
        assert guard(S, r) > 10
    out = mem.empty((2,) + S.O.ct_shape)
    X.transcipher(mem.to_dev(S.enc_key), cw, ncw, [0, 1], out)
    got = mem.to_host(out)
    for b in range(2):
        assert decrypt_slots(S, got[b])[:ncw[b]] == [int(v) for v in pt[128 * b:128 * b + ncw[b]]], b


# ---- c. word parity of the whole hot path at the other moduli ----
# name: (t, prime bit sizes or "default4096", expected row_kernel, expected regime of the lift)
HOT_CASES = {
    "t33_60x3": (T33, [60] * 3, 1, "fast"),
    "t33_default4096": (T33, "default4096", 0, "fast"),
    "t60_60x3": (T60, [60] * 3, 1, "fast"),
    "t60_55x3": (T60, [55] * 3, 1, "slow"),
    "t60_default4096": (T60, "default4096", 0, "slow"),
    "t60_40x4": (T60, [40] * 4, 0, "slow"),
}
HOT_DIM, HOT_BSGS = 16, (4, 4)


def hot_setup(orc, api, lib, name, logn=12):
    """(Setup, context factory that asserts the dispatch) of a HOT_CASES entry: every default Galois key plus the steps of decompose,
    of BSGS transciphering and of the two affine methods"""
    t, spec, row_kernel, regime = HOT_CASES[name]
    n = 1 << logn
    q = case_primes(orc, api, lib, n, spec)
    assert regime_of(t, q[:-1]) == regime, (name, q)
    steps = sorted(set(ac.hand_steps(n, HOT_DIM, *HOT_BSGS)) | {-16 * k for k in range(1, 8)} | {-128, -256})
    S = pc.setup_from_primes(orc, logn, q, t, all_galois=True, extra_steps=steps)

    def make_ctx():
        X = api.Context(logn, q, t, lib=lib)
        pc.assert_dispatch(X, q, row_kernel)
        return X
    return S, make_ctx


def check_bsgs_transcipher(X, S, orc, mem):
    pt = np.array([(13 * i + 2) % 256 for i in range(140)], dtype=np.uint64)
    cw, ncw = S.sym_blocks(orc, pt)
    out = mem.empty((2,) + S.O.ct_shape)
    X.transcipher(mem.to_dev(S.enc_key), cw, ncw, [0, 1], out, use_bsgs=True)
    res = mem.to_host(out)
    for b in range(2):
        assert (res[b] == S.O.transcipher_block(S.enc_key, S.rk, S.gk, cw[b, :ncw[b]], b, use_bsgs=True)).all(), b


def check_hot_words(make_ctx, S, orc, mem, monkeypatch, fc_variants=True, n_in=9, seed=0):
    """check_hot_path (with the FC's execution variants), a BSGS transciphering, both affine methods, the matmul loop on worst-case
    residues and the batched decryption, word for word against the oracle"""
    X = make_ctx()
    S.load_keys(X)
    pc.check_hot_path(X, S, orc, mem, make_ctx if fc_variants else None, monkeypatch, n_in=n_in, seed=seed)
    check_bsgs_transcipher(X, S, orc, mem)
    M, bias = ac.seeded_matrix(S.t, HOT_DIM, 31)
    for bsgs in (None, HOT_BSGS):
        ac.check_affine(X, S, mem, M, bias, bsgs, B=2, seed=1)
    for pattern in ("max", "alt", "max_keys"):
        pc.check_matmul_adversarial(X, S, orc, mem, pattern)
    pc.check_decrypt(X, S, mem, B=2)
    X.close()


# ---- d. plain-side edges ----
# name: (t, prime bit sizes): the three moduli with the fast lift, and T60 over primes below it
EDGE_CASES = {
    "t16_50x3": (T16, [50] * 3),
    "t33_50x3": (T33, [50] * 3),
    "t60_60x3": (T60, [60] * 3),
    "t60_55x3": (T60, [55] * 3),
}
_edge = {}


def edge_setup(orc, name, logn):
    if (name, logn) not in _edge:
        t, bits = EDGE_CASES[name]
        _edge[(name, logn)] = LightSetup(orc, logn, orc.coeff_modulus_create(1 << logn, bits), t)
    return _edge[(name, logn)]


def check_encode_edges(X, S, mem):
    """BatchEncoder::encode with 1, N/2, N/2 + 1, N - 1 and N values per row; row 0 is all t - 1"""
    O, t, n = S.O, S.t, S.n
    rng = np.random.default_rng(65)
    for count in (1, n // 2, n // 2 + 1, n - 1, n):
        vals = rng.integers(0, t, (2, count), dtype=np.uint64)
        vals[0, :] = t - 1
        d_pl = mem.empty((2, n))
        X.encode(mem.to_dev(vals), 2, count, d_pl)
        pl = mem.to_host(d_pl)
        for b in range(2):
            assert (pl[b] == O.encode(vals[b])).all(), (count, b)
            assert [int(v) for v in O.decode(pl[b])] == [int(v) for v in vals[b]] + [0] * (n - count), (count, b)


def check_decrypt_edges(X, S, mem):
    """hhe_decrypt on words that are no encryption of anything: all q_j - 1, alternating with 0, uniform below q_j"""
    O = S.O
    rng = np.random.default_rng(66)
    uni = np.zeros(O.ct_shape, np.uint64)
    for j in range(O.L):
        uni[:, j] = rng.integers(0, S.q[j], (2, O.n), dtype=np.uint64)
    cts = np.stack([pc.adversarial_words(S, 2, "max"), pc.adversarial_words(S, 2, "alt"), uni])
    out = mem.empty((3, O.n))
    X.decrypt(S.sk, mem.to_dev(cts), 3, out)
    got = mem.to_host(out)
    for b in range(3):
        assert (got[b] == O.decode(O.decrypt(S.sk, cts[b]))).all(), b


def check_decrypt_exhausted_chain(X, S, mem, steps=6):
    """six multiply_plain by dense plaintexts: the words stay the oracle's and hhe_decrypt returns what the oracle decrypts, at every
    step, while the noise budget runs from above 0 to 0.  As long as budget is left, the decryption is the product of the slots."""
    O, t, n = S.O, S.t, S.n
    rng = np.random.default_rng(67)
    prod = [int(v) for v in rng.integers(0, t, n, dtype=np.uint64)]
    ref = O.encrypt(S.pk, O.encode(np.array(prod, dtype=np.uint64)), 75)
    budgets = [O.noise_budget(S.sk, ref)]
    assert budgets[0] > 0
    d, d_next = mem.to_dev(ref[None]), mem.empty((1,) + O.ct_shape)
    out = mem.empty((1, n))
    for s in range(steps):
        b = rng.integers(0, t, n, dtype=np.uint64)
        pl = O.encode(b)
        ref = O.multiply_plain(ref, pl)
        prod = [x * int(y) % t for x, y in zip(prod, b)]
        X.multiply_plain(d, mem.to_dev(pl[None]), d_next, 1)
        d, d_next = d_next, d
        assert (mem.to_host(d)[0] == ref).all(), s
        X.decrypt(S.sk, d, 1, out)
        got = mem.to_host(out)[0]
        assert (got == O.decode(O.decrypt(S.sk, ref))).all(), s
        budgets.append(O.noise_budget(S.sk, ref))
        if budgets[-1] > 0:
            assert [int(v) for v in got] == prod, s
    assert budgets[-1] == 0, budgets


def check_add_size3(X, S, mem):
    """hhe_add on the three polynomials of an unrelinearized product"""
    O = S.O
    rng = np.random.default_rng(68)
    cts = np.stack([O.encrypt(S.pk, O.encode(rng.integers(0, S.t, S.n, dtype=np.uint64)), 76 + b) for b in range(2)])
    d = mem.to_dev(cts)
    o3, s3 = mem.empty((2, 3, O.L, O.n)), mem.empty((2, 3, O.L, O.n))
    X.multiply(d, mem.to_dev(cts[::-1].copy()), o3, 2)
    h3 = mem.to_host(o3)
    for b in range(2):
        assert (h3[b] == O.multiply(cts[b], cts[1 - b])).all(), b
    X.add(o3, mem.to_dev(h3[::-1].copy()), s3, 2, size=3)
    got = mem.to_host(s3)
    for b in range(2):
        assert (got[b] == O.add(h3[b], h3[1 - b])).all(), b


def check_plain_edges(X, S, mem):
    check_encode_edges(X, S, mem)
    check_decrypt_edges(X, S, mem)
    check_decrypt_exhausted_chain(X, S, mem)
    check_add_size3(X, S, mem)


# ---- the reference's own N = 32768 options (GPU suite) ----
def check_reference_option(X, S, mem, B=2):
    """encode -> add_plain / multiply_plain / hhe_mask -> hhe_decrypt on B items, every slot against Python integers mod t; secret
    and public key only"""
    O, t, n = S.O, S.t, S.n
    rng = np.random.default_rng(69)
    a = rng.integers(0, t, (B, n), dtype=np.uint64)
    b = rng.integers(0, t, (B, n), dtype=np.uint64)
    b[:, :7] = edge_values(t)
    count = 300
    mv = rng.integers(0, t, count, dtype=np.uint64)
    mv[:7] = edge_values(t)
    cts = np.stack([O.encrypt(S.pk, O.encode(a[i]), 77 + i) for i in range(B)])
    d_pl = mem.empty((B, n))
    X.encode(mem.to_dev(b), B, n, d_pl)
    pl = mem.to_host(d_pl)
    for i in range(B):
        assert (pl[i] == O.encode(b[i])).all(), i
    guard(S, O.add_plain(cts[0], pl[0]))
    guard(S, O.multiply_plain(cts[0], pl[0]))
    guard(S, O.mask(cts[0], mv))
    d_cts = mem.to_dev(cts)
    o_add, o_mul, o_mask = (mem.empty((B,) + O.ct_shape) for _ in range(3))
    X.add_plain(d_cts, d_pl, o_add, B)
    X.multiply_plain(d_cts, d_pl, o_mul, B)
    X.mask(d_cts, mv, o_mask, B)
    dec = mem.empty((B, n))
    want = {
        "add_plain": lambda i: [(int(x) + int(y)) % t for x, y in zip(a[i], b[i])],
        "multiply_plain": lambda i: [int(x) * int(y) % t for x, y in zip(a[i], b[i])],
        "mask": lambda i: [int(a[i, k]) * int(mv[k]) % t if k < count else 0 for k in range(n)],
    }
    for what, d_out in (("add_plain", o_add), ("multiply_plain", o_mul), ("mask", o_mask)):
        X.decrypt(S.sk, d_out, B, dec)
        got = mem.to_host(dec)
        for i in range(B):
            assert [int(v) for v in got[i]] == want[what](i), (what, i)
