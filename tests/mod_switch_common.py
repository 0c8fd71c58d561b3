"""BFV modulus switching: what tests/test_mod_switch_emu.py (emulator, numpy memory) and tests/test_gpu_mod_switch.py (gfx950, torch
memory) share.

The truth is written once, here, in Python integers, and shares no code with the product or the oracle.  For a polynomial whose CRT
representative under q_0 .. q_m is x in [0, Q_m+1), one step of Evaluator::mod_switch_to_next gives the words

    floor((x + floor(q_m / 2)) / q_m)  mod q_j        for j < m

(the quotient can equal the product of the remaining primes, so the `mod q_j` is part of the definition), and a switch over several
levels is that step repeated: every dropped prime rounds on its own.  Every comparison is exact word equality.
"""
import numpy as np
import pytest

import seal_writer as sw

T16, T33 = 65537, 8088322049
B = 3


# ---- the definition ----
def _obj(a):
    a = np.asarray(a)
    return np.array([int(v) for v in a.reshape(-1)], dtype=object).reshape(a.shape)


def crt(res, q):
    """res [..., l, n] words under q[:l] -> representatives in [0, Q) as Python integers [..., n]"""
    Q = 1
    for v in q:
        Q *= int(v)
    x = 0
    for j, qj in enumerate(q):
        Mj = Q // int(qj)
        x = x + _obj(res[..., j, :]) * (Mj * pow(Mj, -1, int(qj)) % Q)
    return x % Q


def chain(words, q):
    """words [P][l][n] under q[:l] -> {level: words [P][level][n]} for every level 1 .. l, by the definition"""
    l = words.shape[1]
    q = [int(v) for v in q[:l]]
    x = crt(words, q)
    out = {l: words.copy()}
    for m in range(l - 1, 0, -1):
        Qn = 1
        for v in q[:m]:
            Qn *= v
        x = ((x + q[m] // 2) // q[m]) % Qn
        out[m] = np.stack([(x % q[j]).astype(np.uint64) for j in range(m)], axis=1)
    return out


# ---- shapes: name -> (logn, primes of the context, the special prime last) ----
def shape_primes(orc, api, lib, name):
    if name == "n1024_3x50":
        return 10, orc.coeff_modulus_create(1024, [50] * 3)
    if name == "n4096_3x60":
        return 12, orc.coeff_modulus_create(4096, [60] * 3)
    if name == "n1024_mixed":  # small above large and large above small
        return 10, orc.coeff_modulus_create(1024, [18, 60, 30, 59, 20, 45, 60])
    if name == "n1024_9x50":   # 8 data primes: the last register form
        return 10, orc.coeff_modulus_create(1024, [50] * 9)
    if name == "n1024_10x50":  # 9 data primes: the first limb count past a register form
        return 10, orc.coeff_modulus_create(1024, [50] * 10)
    if name == "n1024_chain65536":  # L = 28; the primes are 1 mod 2^17, so they serve any smaller N
        q = api.bfv_default_coeff_modulus(65536, lib)
        assert len(q) == 29
        return 10, q
    if name == "n1024_33x50":  # L = 32 = HHE_MAXL: the largest column the LDS form takes (64 KiB per workgroup)
        return 10, orc.coeff_modulus_create(1024, [50] * 33)
    if name == "n16384_default":
        return 14, api.bfv_default_coeff_modulus(16384, lib)
    raise KeyError(name)


WORD_SHAPES = ["n1024_3x50", "n4096_3x60", "n1024_mixed", "n1024_9x50", "n1024_10x50", "n1024_chain65536", "n1024_33x50"]


def sizes_of(name):
    """ciphertext sizes a shape is run at: 2 and 3, but the 33-prime shape is there for its LDS block alone"""
    return (2,) if name == "n1024_33x50" else (2, 3)


class Shape:
    """the parameters of a context the oracle cannot make (it stops at 32 primes): what the word checks read of an Oracle"""

    def __init__(self, logn, q, t):
        self.logn, self.n, self.q, self.t = logn, 1 << logn, [int(v) for v in q], int(t)
        self.K, self.L = len(q), len(q) - 1


def crafted_columns(q):
    """columns [C][l] of residues under the data primes q: the edges of one step's arithmetic"""
    l = len(q)
    rng = np.random.default_rng(90)
    rnd = lambda: [int(rng.integers(0, v)) for v in q]
    cols = [[v - 1 for v in q],    # every word q_j - 1, which is also x = Q - 1
            [0] * l]
    for m in range(l):             # the two sides of the wrap of r = (x_m + floor(q_m/2)) mod q_m
        for d in (1, 0):
            c = rnd()
            c[m] = q[m] - q[m] // 2 - d
            cols.append(c)
    for m in range(1, l):          # x_j = 0 with r mod q_j != 0
        c = [0] * l
        c[m] = 1
        assert all((1 + q[m] // 2) % q[j] != 0 for j in range(m))
        cols.append(c)
    return np.array(cols, dtype=np.uint64)


def make_inputs(O, size, seed, wg=256, B=B):
    """[B][size][L][N]: oracle encryptions (a third polynomial from another encryption's c1), with the crafted columns at the first
    coefficients, at the last coefficients and across a workgroup boundary of the first polynomial and of the last one"""
    n, L, q = O.n, O.L, O.q[:O.L]
    rng = np.random.default_rng(seed)
    w = np.zeros((B, size, L, n), np.uint64)
    if isinstance(O, Shape):   # a chain longer than the oracle takes: uniform words below the primes
        for j in range(L):
            w[:, :, j] = rng.integers(0, q[j], (B, size, n), dtype=np.uint64)
    else:
        sk = O.keygen_secret(1)
        pk = O.keygen_public(sk, 2)
    for b in range(B if not isinstance(O, Shape) else 0):
        ct = O.encrypt(pk, O.encode(rng.integers(0, O.t, n, dtype=np.uint64)), seed + b)
        w[b, :2] = ct
        if size == 3:
            w[b, 2] = O.encrypt(pk, O.encode(rng.integers(0, O.t, n, dtype=np.uint64)), seed + 100 + b)[1]
    cols = crafted_columns(q).T  # [L][C]
    C = cols.shape[1]
    assert 2 * C + C <= n and wg - C // 2 >= C
    for (b, p) in ((0, 0), (B - 1, size - 1)):
        w[b, p, :, :C] = cols
        w[b, p, :, n - C:] = cols
        w[b, p, :, wg - C // 2: wg - C // 2 + C] = cols
    return w


def switch(X, mem, d_in, size, nb, lin, lout):
    out = mem.empty((nb, size, lout, X.n))
    X.mod_switch(d_in, size, nb, lin, lout, out)
    return out


def check_words(X, O, mem, sizes=(2, 3), targets=None, B=B):
    """hhe_mod_switch from the data level to every limbs_out against the definition, on the full vector"""
    L = O.L
    for size in sizes:
        w = make_inputs(O, size, 40 + size, B=B)
        truth = chain(w.reshape(B * size, L, O.n), O.q)
        d_in = mem.to_dev(w)
        for lout in (targets or range(1, L + 1)):
            got = mem.to_host(switch(X, mem, d_in, size, B, L, lout)).reshape(B * size, lout, O.n)
            bad = np.argwhere(got != truth[lout])
            assert bad.size == 0, (size, lout, bad[:4].tolist())
    check_wrap_at_every_prime(X, O, mem)


def check_wrap_at_every_prime(X, O, mem):
    """A switch from L meets the crafted values of x_m only at the first dropped prime; below it the earlier steps have changed the
    residues.  So the first limbs_in limbs of the crafted input enter as an input of their own, for every limbs_in below L: the
    column made for m = limbs_in - 1 then has its x_m on the two sides of the wrap of r at the step that drops q_m.  One step, and
    the switch to the last level, against the definition."""
    L, n = O.L, O.n
    w = make_inputs(O, 2, 45, B=1)
    C = len(crafted_columns(O.q[:L]))
    at = np.r_[0:C, 256 - C // 2:256 - C // 2 + C, n - C:n]   # where make_inputs put the columns (the full vector is check_words' part)
    for lin in range(2, L):
        part = np.ascontiguousarray(w[:, :, :lin])
        truth = chain(part.reshape(2, lin, n)[:, :, at], O.q)
        d_in = mem.to_dev(part)
        for lout in sorted({lin - 1, 1}):
            got = mem.to_host(switch(X, mem, d_in, 2, 1, lin, lout)).reshape(2, lout, n)[:, :, at]
            bad = np.argwhere(got != truth[lout])
            assert bad.size == 0, (lin, lout, bad[:4].tolist())


def check_composition(X, O, mem):
    """L -> l equals the chain of single steps word for word; inputs below L work; limbs_out == limbs_in copies; one launch per call"""
    L = O.L
    w = make_inputs(O, 2, 50)
    d_top = mem.to_dev(w)
    n0 = X.query("mod_switch_launches")
    d_step, calls = d_top, 0
    for l in range(L - 1, 0, -1):
        d_step = switch(X, mem, d_step, 2, B, l + 1, l)   # limbs_in < L from the second step on
        direct = switch(X, mem, d_top, 2, B, L, l)
        calls += 2
        assert (mem.to_host(d_step) == mem.to_host(direct)).all(), l
        assert X.query("mod_switch_launches") == n0 + calls
    for l in (L, max(1, L - 1)):
        src = d_top if l == L else switch(X, mem, d_top, 2, B, L, l)
        n1 = X.query("mod_switch_launches")
        same = switch(X, mem, src, 2, B, l, l)
        assert X.query("mod_switch_launches") == n1 + 1
        assert (mem.to_host(same) == mem.to_host(src)).all(), l


def check_refusals(X, O, mem, api):
    L, n = O.L, O.n
    big = mem.to_dev(np.arange(B * 3 * (L + 1) * n, dtype=np.uint64))
    mark = 0xABCDEF0123456789
    out = mem.to_dev(np.full(B * 3 * (L + 1) * n, mark, dtype=np.uint64))
    n0 = X.query("mod_switch_launches")
    for size, lin, lout in ((2, L, 0), (2, L, L + 1), (2, max(1, L - 1), L), (2, L + 1, L), (2, L + 1, 1), (1, L, 1), (4, L, 1), (2, L, -1)):
        with pytest.raises(api.HheError) as e:
            X.mod_switch(big, size, B, lin, lout, out)
        assert e.value.code == api.ERR_INVALID, (size, lin, lout)
    assert (mem.to_host(out) == np.uint64(mark)).all()
    # overlapping buffers: in place, and the output starting inside the input's last item
    buf = mem.to_dev(np.arange(2 * B * 2 * L * n, dtype=np.uint64))
    before = mem.to_host(buf).copy()
    words_in = B * 2 * L * n
    base = buf.data_ptr() if hasattr(buf, "data_ptr") else buf.ctypes.data
    words_out = B * 2 * 1 * n
    for src, dst in ((0, 0), (0, words_in - 1), (words_out - 1, 0)):   # in place; out begins in ct's last word; out ends in ct's first
        with pytest.raises(api.HheError) as e:
            X.mod_switch(base + 8 * src, 2, B, L, 1, base + 8 * dst)
        assert e.value.code == api.ERR_INVALID, (src, dst)
    assert (mem.to_host(buf) == before).all()
    assert X.query("mod_switch_launches") == n0


# ---- meaning ----
MEANING = {  # name -> (logn, bit sizes with the special prime last, plain modulus, levels that decrypt)
    "n1024_4x50_t16": (10, [50] * 4, T16, (2, 1)),
    "n1024_3x30_t16": (10, [30] * 3, T16, (1,)),
    "n1024_4x55_t33": (10, [55] * 4, T33, (2, 1)),
}


def short_oracle(orc, O, sk, l):
    """the oracle of the context whose data primes are q_0 .. q_{l-1} (the same special prime), and the secret key's matching rows"""
    K = O.K
    return orc.Oracle(O.logn, O.q[:l] + [O.q[K - 1]], O.t), np.ascontiguousarray(np.concatenate([sk[:l], sk[K - 1:K]]))


def check_meaning(X, O, orc, mem, levels, nb=2):
    """hhe_decrypt_level of the switched ciphertext gives the encoded slot values; the short-chain oracle agrees and reports budget"""
    n, L, t = O.n, O.L, O.t
    sk = O.keygen_secret(1)
    pk = O.keygen_public(sk, 2)
    rng = np.random.default_rng(91)
    vals = rng.integers(0, t, (nb, n), dtype=np.uint64)
    vals[0, :4] = [0, 1, t - 1, t // 2]
    cts = np.stack([O.encrypt(pk, O.encode(vals[b]), 60 + b) for b in range(nb)])
    d_ct, d_vals = mem.to_dev(cts), mem.empty((nb, n))
    X.decrypt(sk, d_ct, nb, d_vals)
    full = mem.to_host(d_vals).copy()
    assert (full == vals).all()
    X.decrypt_level(sk, d_ct, L, nb, d_vals)
    assert (mem.to_host(d_vals) == full).all()
    budgets = {}
    for l in levels:
        d_low = switch(X, mem, d_ct, 2, nb, L, l)
        X.decrypt_level(sk, d_low, l, nb, d_vals)
        got, low = mem.to_host(d_vals), mem.to_host(d_low)
        O2, sk2 = short_oracle(orc, O, sk, l)
        for b in range(nb):
            budgets[(l, b)] = O2.noise_budget(sk2, low[b])
            assert budgets[(l, b)] > 0, ("no noise budget at this level", l, b, budgets)
            assert (O2.decode(O2.decrypt(sk2, low[b])) == vals[b]).all(), (l, b)
            assert (got[b] == vals[b]).all(), (l, b)
    return budgets


def check_keyless_flow(X, O, orc, mem, level, seed=bytes(range(32)), seed2=bytes((5 * i + 1) % 256 for i in range(32))):
    """no oracle key anywhere: device keys, device encryption of two items, multiply, relinearize, switch to `level`, decrypt: the
    slot-wise product mod t.  The oracle only reports the budget at every level, given the device's key: `level` is the lowest one from
    which every level upward has budget, and where a level exists below it, that one is asserted to have none."""
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
    want = np.array([[int(x) * int(y) % t for x, y in zip(a[i], b[i])] for i in range(2)], dtype=np.uint64)
    d_vals = mem.empty((2, n))
    budgets = {}
    for l in range(L, 0, -1):
        low = mem.to_host(switch(X, mem, d_r, 2, 2, L, l))
        O2, sk2 = short_oracle(orc, O, sk, l)
        budgets[l] = min(O2.noise_budget(sk2, low[i]) for i in range(2))
    print("keyless flow: noise budget per level", budgets)
    lowest = min(l for l in budgets if all(budgets[k] > 0 for k in range(l, L + 1)))
    assert lowest == level, budgets
    assert level == 1 or budgets[level - 1] <= 0, budgets
    d_low = switch(X, mem, d_r, 2, 2, L, level)
    X.decrypt_level(sk, d_low, level, 2, d_vals)
    assert (mem.to_host(d_vals) == want).all()
    ks.close()
    return budgets


# ---- wire ----
def check_wire(X, O, mem, api):
    n, L = O.n, O.L
    w = make_inputs(O, 3, 70)
    d_top = mem.to_dev(w)
    for size in (2, 3):
        for l in range(1, L + 1):
            pid = bytes((l * 16 + i) % 256 for i in range(32))   # carried through, not computed: the target level's id
            d_full = switch(X, mem, d_top, 3, B, L, l)
            words = mem.to_host(d_full)[1, :size]
            d_ct = mem.to_dev(words)
            blob = X.seal_save_ciphertext_level(d_ct, size, l, pid)
            assert blob == sw.obj(sw.ct_members(pid, words, size, n, l))   # `written` = the writer's size arithmetic, and the bytes
            assert sw.parse_ciphertext(blob)[1:4] == (size, n, l)
            out = mem.empty((3, L, n))
            stream = blob + b"tail"
            got_size, got_l, got_pid, used = X.seal_load_ciphertext_level(stream, out)
            assert (got_size, got_l, got_pid, used) == (size, l, pid, len(blob))
            assert (mem.to_host(out).reshape(-1)[:size * l * n].reshape(size, l, n) == words).all()
            if l < L:   # the data-level loader still refuses a lower-level stream, target untouched
                mark = mem.to_dev(np.full((3, L, n), 7, dtype=np.uint64))
                with pytest.raises(api.HheError, match="not at the data level"):
                    X.seal_load_ciphertext(blob, mark)
                assert (mem.to_host(mark) == 7).all()
            else:       # and at the data level the two pairs write and read the same stream
                assert blob == X.seal_save_ciphertext(d_ct, size, pid)
                assert X.seal_load_ciphertext(blob, out)[0] == size
            # a word at its prime, in the last limb of the last polynomial: refused, target untouched
            bad = words.copy()
            bad[size - 1, l - 1, n - 1] = O.q[l - 1]
            mark = mem.to_dev(np.full((3, L, n), 7, dtype=np.uint64))
            with pytest.raises(api.HheError, match="not reduced"):
                X.seal_load_ciphertext_level(sw.obj(sw.ct_members(pid, bad, size, n, l)), mark)
            assert (mem.to_host(mark) == 7).all()
    # limb counts outside 1 .. L
    over = np.zeros((2, L + 1, n), np.uint64)
    with pytest.raises(api.HheError, match="not at a level"):
        X.seal_load_ciphertext_level(sw.obj(sw.ct_members(pid, over, 2, n, L + 1)), mem.empty((3, L + 1, n)))
    with pytest.raises(api.HheError):
        X.seal_save_ciphertext_level(d_ct, 2, L + 1, pid)
    with pytest.raises(api.HheError):
        X.seal_save_ciphertext_level(d_ct, 2, 0, pid)
