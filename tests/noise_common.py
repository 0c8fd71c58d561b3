"""The invariant noise budget on the device (hhe_noise_budget): what tests/test_noise_emu.py (emulator, numpy memory) and
tests/test_gpu_noise.py (gfx950, torch memory) share.

The truth is written once, here, in Python integers (Decryptor::invariant_noise_budget, seal/decryptor.h:103), and shares no code with
the product or with the oracle's sampled estimate.  For a ciphertext of `size` polynomials under Q = q_0 ... q_{limbs-1}:

    v_j[i] = t * (c0 + c1 s + c2 s^2)_j[i] mod q_j          x[i] = the CRT representative of the column v_.[i] in [0, Q)
    m[i]   = Q - x[i] if x[i] >= (Q+1)/2 else x[i]          norm_bits = bit_length(max_i m[i])  (0 for an all-zero noise polynomial)
    budget = max(0, bit_length(Q) - norm_bits - 1)

Every comparison is exact equality of norm_bits and of budget, per item.
"""
import ctypes as C

import numpy as np
import pytest

import mod_switch_common as ms
from plain_modulus_common import T60

T16, T33 = ms.T16, ms.T33


# ---- the definition ----
def product(q):
    Q = 1
    for v in q:
        Q *= int(v)
    return Q


def centred(x, Q):
    return Q - x if x >= (Q + 1) // 2 else x


def budget_of(bits, Q):
    return max(0, Q.bit_length() - bits - 1)


def define(phase, q, t):
    """phase [B][l][n]: the words of c0 + c1 s (+ c2 s^2) under q[:l] -> (budget [B], norm_bits [B]) by the definition, full vector"""
    phase = np.asarray(phase)
    l = phase.shape[1]
    q = [int(v) for v in q[:l]]
    Q = product(q)
    v = np.empty(phase.shape, dtype=object)
    for j in range(l):
        v[:, j] = ms._obj(phase[:, j]) * int(t) % q[j]
    x = ms.crt(v, q)
    bits = [max(centred(int(c), Q) for c in item).bit_length() for item in x]
    return np.array([budget_of(b, Q) for b in bits], np.int32), np.array(bits, np.uint32)


def call(X, mem, sk, words, size, limbs):
    """hhe_noise_budget on host words [B][size][limbs][N]"""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    assert words.shape[1:] == (size, limbs, X.n)
    return X.noise_budget(sk, mem.to_dev(words), words.shape[0], size, limbs, with_bits=True)


def same(got, want, what):
    (gb, gn), (wb, wn) = got, want
    assert gb.dtype == np.int32 and gn.dtype == np.uint32
    assert gn.tolist() == wn.tolist(), (what, "norm_bits", gn.tolist(), wn.tolist())
    assert gb.tolist() == wb.tolist(), (what, "budget", gb.tolist(), wb.tolist())


# ---- 1. crafted magnitudes: c1 = 0, so the phase is c0 whatever the key, and c0 = v t^-1 mod Q puts v into a coefficient ----
CRAFTED = {  # name -> (shape of mod_switch_common, plain modulus)
    "n1024_3x50": ("n1024_3x50", T16),
    "n4096_3x60": ("n4096_3x60", T16),
    "n1024_mixed": ("n1024_mixed", T16),
    "n1024_9x50": ("n1024_9x50", T16),       # 8 data primes: the last register form
    "n1024_10x50": ("n1024_10x50", T16),     # 9 data primes: the first LDS form
    "n1024_chain65536": ("n1024_chain65536", T16),
    "n1024_33x50": ("n1024_33x50", T16),
    "n1024_3x50_t33": ("n1024_3x50", T33),
    "n1024_4x55_t60": ("n1024_4x55", T60),   # t above every prime
}
NOISE_REGS = 8


def crafted_primes(orc, api, lib, name):
    shape, t = CRAFTED[name]
    if shape == "n1024_4x55":
        return 10, orc.coeff_modulus_create(1024, [55] * 4), t
    logn, q = ms.shape_primes(orc, api, lib, shape)
    return logn, q, t


def crafted_values(q):
    """the magnitudes of the issue's list that are below Q, in order, without repeats"""
    Q = product(q)
    ks = [63, 64, 65, 127, 128, Q.bit_length() - 2]
    vals = [0, 1]
    for k in ks:
        vals += [2 ** k - 1, 2 ** k, 2 ** k + 1]
    vals += [q[0] - 1, q[0]]
    if len(q) > 1:
        vals.append(q[0] * q[1])
    vals += [(Q - 1) // 2, (Q + 1) // 2, (Q + 1) // 2 + 1, Q - 1]
    for k in ks:
        vals += [Q - 2 ** k, Q - 2 ** k - 1]
    out = []
    for v in vals:
        if 0 <= v < Q and v not in out:
            out.append(v)
    return out


def residues_of(v, q, t):
    """v t^-1 mod Q, residue-wise"""
    return [v % qj * pow(int(t) % qj, -1, qj) % qj for qj in q]


def crafted_levels(L):
    return list(range(1, L + 1)) if L <= 9 else [L, L // 2 + 1, NOISE_REGS + 1]


def check_crafted(X, q, t, mem, levels=None):
    """every value alone in an otherwise all-zero item (the first one, 0, is the whole item), at a coefficient that moves with the item"""
    n, L = X.n, X.L
    rng = np.random.default_rng(7)
    sk = np.stack([rng.integers(0, int(qj), n, dtype=np.uint64) for qj in q])   # c1 = 0: any key
    for l in levels or crafted_levels(L):
        ql = [int(v) for v in q[:l]]
        Q = product(ql)
        vals = crafted_values(ql)
        w = np.zeros((len(vals), 2, l, n), np.uint64)
        for b, v in enumerate(vals):
            w[b, 0, :, (37 * b + 5) % n] = residues_of(v, ql, t)
        bits = [centred(v, Q).bit_length() for v in vals]
        want = np.array([budget_of(b, Q) for b in bits], np.int32), np.array(bits, np.uint32)
        same(call(X, mem, sk, w, 2, l), want, ("crafted", l))
        assert X.query("noise_form") == (l if l <= NOISE_REGS else 0), l


# ---- 2. the reduction over an item ----
def check_reduction(X, q, t, mem):
    n, L = X.n, X.L
    q = [int(v) for v in q[:L]]
    Q = product(q)
    sk = np.zeros((len(q) + 1, n), np.uint64)
    at = [0, 63, 64, 255, 256, n - 1]
    top = Q.bit_length() - 2

    def run(vals, what):
        w = np.zeros((len(vals), 2, L, n), np.uint64)
        for b, (i, v) in enumerate(vals):
            if v:
                w[b, 0, :, i] = residues_of(v, q, t)
        bits = [centred(v, Q).bit_length() for _, v in vals]
        want = np.array([budget_of(b, Q) for b in bits], np.int32), np.array(bits, np.uint32)
        same(call(X, mem, sk, w, 2, L), want, what)

    first = [(i, 2 ** (top - 3 * k) + k) for k, i in enumerate(at)] + [(0, 0)]     # six items of one coefficient each, one all-zero item
    run(first, "reduction, first call")
    run([(i, 2 ** (5 + k)) for k, i in enumerate(at)] + [(0, 0)], "reduction, smaller values on the same context")   # no maximum of the call before
    run([(n - 1, 3)], "reduction, one item")
    # several coefficients in an item, the largest in the middle of a wave and in another workgroup than the others
    w = np.zeros((2, 2, L, n), np.uint64)
    for i, v in ((0, 5), (300, 2 ** 40), (301, 2 ** 41 - 1), (n - 1, 9)):
        w[0, 0, :, i] = residues_of(v, q, t)
    w[1, 0, :, 77] = residues_of(Q - 2 ** 20, q, t)
    same(call(X, mem, sk, w, 2, L), (np.array([budget_of(41, Q), budget_of(21, Q)], np.int32), np.array([41, 21], np.uint32)), "several")


# ---- 3. real ciphertexts: the residues from the oracle's phase, the rest from the definition ----
REAL = {"n1024_4x50": (10, [50] * 4), "n4096_3x60": (12, [60] * 3)}


def check_real(X, O, orc, mem):
    n, L, t = O.n, O.L, O.t
    sk, rng = O.keygen_secret(1), np.random.default_rng(93)
    pk, rk = O.keygen_public(sk, 2), O.keygen_relin(sk, 3)
    a, b = (O.encode(rng.integers(0, t, n, dtype=np.uint64)) for _ in range(2))
    ct, ct2 = O.encrypt(pk, a, 21), O.encrypt(pk, b, 22)
    m3 = O.multiply(ct, ct2)
    cases = {"fresh": ct, "multiply_plain": O.multiply_plain(ct, b), "multiply": m3, "relinearize": O.relinearize(m3, rk)}
    for what, c in cases.items():
        size = c.shape[0]
        want = define(O.phase(sk, c)[None], O.q, t)
        got = call(X, mem, sk, c[None], size, L)
        same(got, want, what)
        secondary(O, sk, c, got, what)
    both = np.stack([cases["fresh"], cases["relinearize"]])     # a batch, and every level of it
    for l in range(L, 0, -1):
        low = mem.to_host(ms.switch(X, mem, mem.to_dev(both), 2, 2, L, l))
        O2, sk2 = ms.short_oracle(orc, O, sk, l)
        want = define(np.stack([O2.phase(sk2, low[i]) for i in range(2)]), O2.q, t)
        got = call(X, mem, sk, low, 2, l)
        same(got, want, ("level", l))
        for i in range(2):
            secondary(O2, sk2, low[i], (got[0][i:i + 1], got[1][i:i + 1]), ("level", l, i))


def secondary(O, sk, c, got, what):
    """the oracle's own formula over every coefficient is this budget or one less"""
    if got[1][0] == 0:
        return
    b_o = O.noise_budget(sk, c, sample=O.n)
    assert int(got[0][0]) in (b_o, b_o + 1), (what, int(got[0][0]), b_o)


# ---- 4. the keyless flow, the level chosen by the device's budget ----
def check_keyless_flow(X, O, mem, level, seed=bytes(range(32)), seed2=bytes((5 * i + 1) % 256 for i in range(32))):
    """mod_switch_common.check_keyless_flow with hhe_noise_budget in the oracle's place: device keys, device encryption of two items,
    multiply, relinearize; `level` is the lowest level from which every level upward has budget, and decryption there gives the
    slot-wise product mod t"""
    n, L, t = O.n, O.L, O.t
    d_sk, d_pk = mem.empty((O.K, n)), mem.empty((2, O.K, n))
    X.keygen_secret(seed, d_sk)
    X.keygen_public(d_sk, seed, d_pk)
    ks = X.keyset()
    ks.generate_relin(d_sk, seed2)
    rng = np.random.default_rng(92)
    a, b = rng.integers(0, t, (2, n), dtype=np.uint64), rng.integers(0, t, (2, n), dtype=np.uint64)
    d_pa, d_pb = mem.empty((2, n)), mem.empty((2, n))
    X.encode(mem.to_dev(a), 2, n, d_pa)
    X.encode(mem.to_dev(b), 2, n, d_pb)
    d_a, d_b = mem.empty((2,) + O.ct_shape), mem.empty((2,) + O.ct_shape)
    X.encrypt(d_pk, d_pa, seed, 2, d_a)
    X.encrypt(d_pk, d_pb, seed2, 2, d_b)
    d_3, d_r = mem.empty((2, 3, L, n)), mem.empty((2,) + O.ct_shape)
    X.reserve(2)
    X.multiply(d_a, d_b, d_3, 2)
    X.relinearize(d_3, d_r, 2, rk=ks)
    X.sync()
    sk = mem.to_host(d_sk)
    budgets = {l: int(X.noise_budget(sk, ms.switch(X, mem, d_r, 2, 2, L, l), 2, 2, l).min()) for l in range(L, 0, -1)}
    print("keyless flow: device noise budget per level", budgets)
    lowest = min(l for l in budgets if all(budgets[k] > 0 for k in range(l, L + 1)))
    assert lowest == level, budgets
    want = np.array([[int(x) * int(y) % t for x, y in zip(a[i], b[i])] for i in range(2)], dtype=np.uint64)
    d_vals = mem.empty((2, n))
    X.decrypt_level(sk, ms.switch(X, mem, d_r, 2, 2, L, level), level, 2, d_vals)
    assert (mem.to_host(d_vals) == want).all()
    ks.close()
    return budgets


# ---- 5. refusals: HHE_ERR_INVALID, both outputs untouched ----
def check_refusals(X, mem, api):
    n, L, B = X.n, X.L, 2
    sk = np.zeros((L + 1, n), np.uint64)
    d_ct = mem.to_dev(np.zeros((B, 3, L, n), np.uint64))
    budget, bits = np.full(B, -77, np.int32), np.full(B, 0xABCDEF01, np.uint32)
    p = api._ptr

    def raw(sk_, ct_, size, limbs, nb, budget_, bits_):
        return X.lib.hhe_noise_budget(X.h, p(sk_), p(ct_), C.c_int(size), C.c_int(limbs), C.c_size_t(nb), p(budget_), p(bits_))

    assert raw(sk, d_ct, 2, L, B, budget, bits) == 0 and (budget != -77).all() and (bits == 0).all()    # the arguments the refusals vary
    budget[:], bits[:] = -77, 0xABCDEF01
    for args in ((None, d_ct, 2, L, B, budget, bits), (sk, None, 2, L, B, budget, bits), (sk, d_ct, 2, L, B, None, bits),
                 (sk, d_ct, 2, L, 0, budget, bits), (sk, d_ct, 1, L, B, budget, bits), (sk, d_ct, 4, L, B, budget, bits),
                 (sk, d_ct, 0, L, B, budget, bits), (sk, d_ct, 2, 0, B, budget, bits), (sk, d_ct, 2, L + 1, B, budget, bits),
                 (sk, d_ct, 2, -1, B, budget, bits)):
        assert raw(*args) == api.ERR_INVALID, args[2:5]
        assert (budget == -77).all() and (bits == 0xABCDEF01).all(), args[2:5]
    assert X.lib.hhe_noise_budget(None, p(sk), p(d_ct), C.c_int(2), C.c_int(L), C.c_size_t(B), p(budget), p(bits)) == api.ERR_INVALID
    assert (budget == -77).all() and (bits == 0xABCDEF01).all()
    with pytest.raises(api.HheError) as e:
        X.noise_budget(sk, d_ct, B, 4)
    assert e.value.code == api.ERR_INVALID
    assert raw(sk, d_ct, 3, L, B, budget, None) == 0 and (budget != -77).all()     # norm_bits may be null
    assert X.noise_budget(sk, d_ct, B, 3).dtype == np.int32
