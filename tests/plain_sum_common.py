"""Checker of the plain-weights sum of rotations (hhe_rotate_plain_sum_ks) and of the open FC layer under plain weights built on it
(hhe_fc_open_plain_ks).  Shared by the emulator suite (numpy memory) and the GPU suite (torch memory).  Every comparison is exact
equality.

Truth 1 is the DEFINITION of include/hhe_gfx950.h in Python integers.  It takes the CRT-free key objects and the coefficient-domain
Galois map of definition_common (SparseKey / LiftedKey, galois_limbs, mod_down's formula) and shares nothing with the oracle's or the
product's key switch.  With sparse plaintexts -- a few monomials with centred coefficients -- the product m~ * X costs a few shifted
copies and the full vector is checked; their slot vectors are the oracle's decode of the polynomial (encode is its inverse).  With
DENSE plaintexts (dense_truth) every child's X is made once as an integer polynomial -- per prime through the oracle's transforms,
which definition_common.check_ntt holds to the definition, then a CRT in Python integers -- and m~ * X at a coefficient is one integer
dot product of length N.
Truth 2: n = 1 with the all-ones plaintext is the oracle's rotate_rows, word for word.
Truth 3: plain integers mod t behind a decryption, after the oracle's noise budget is seen positive."""
import random

import numpy as np

import definition_common as dc
import fc_packed_common as fp
import mlp_common as mc
import parity_common as pc

T = fp.T


# ---- truth 1: the definition ----
def centred(t, x):
    """the lift: x below (t + 1) / 2 stays, x - t from there on"""
    x, t = int(x), int(t)
    return x if x < (t + 1) // 2 else x - t


class SparsePlain:
    """a plaintext polynomial of a few monomials [(coefficient in [0, t), exponent)]; slots: what the handle is given"""

    def __init__(self, E, terms):
        self.terms = [(int(c) % E.t, int(e)) for c, e in terms]
        poly = np.zeros(E.n, np.uint64)
        for c, e in self.terms:
            assert poly[e] == 0
            poly[e] = c
        self.poly = poly
        self.slots = E.O.decode(poly)
        assert (E.O.encode(self.slots) == poly).all()
        self.lift = [(centred(E.t, c), e) for c, e in self.terms]

    def times(self, a):
        """m~ * a in Z[X]/(X^N + 1) on an object array"""
        acc = np.zeros(len(a), dtype=object)
        for c, e in self.lift:
            acc = acc + dc.negacyclic_shift(a * c, e)
        return acc

    def times_at(self, get, n, l):
        """coefficient l of m~ * a, a read through get(index)"""
        s = 0
        for c, e in self.lift:
            s += c * (get(l - e) if l >= e else -get(l - e + n))
        return s

    def needs(self, n, idx):
        return sorted({(l - e) % n for l in idx for _, e in self.lift})


def ones_plain(E):
    return SparsePlain(E, [(1, 0)])


def random_sparse_plains(E, count, seed):
    """three monomials each: coefficient 1, t - 1 and a seeded one (both sides of the lift's threshold over the set), at exponent 0, N - 1
    and a seeded one"""
    rnd = random.Random(seed)
    out = []
    for k in range(count):
        cs = [1, E.t - 1, rnd.randrange(2, E.t - 1)]
        es = [0, E.n - 1, rnd.randrange(1, E.n - 1)]
        out.append(SparsePlain(E, [(cs[(r + k) % 3], es[r]) for r in range(3)]))
    return out


class ChosenKey:
    """key[0][i] = the polynomial whose coefficient l IS X_i[l] for an input whose digits are (1, 0, .., 0) (definition_common.DenseKey with
    the values given by the caller): Xs two lists of N integers in [0, Q p)"""

    def __init__(self, E, Xs):
        self.Xs = [np.array([int(v) for v in X], dtype=object) for X in Xs]
        self.words = np.zeros(E.O.ksk_shape, np.uint64)
        for k in range(2):
            for J in range(E.K):
                self.words[0, k, J] = E.O.ntt_fwd(J, (self.Xs[k] % E.q[J]).astype(np.uint64))

    def X(self, E, d, idx=None):
        unit = np.zeros((E.L, E.n), np.uint64)
        unit[0, 0] = 1
        assert (d == unit).all(), "a chosen key needs the digits (1, 0, ..., 0)"
        return self.Xs


def plain_sum_truth(E, pairs, ct, idx=None):
    """the definition's output [2][L][N] for pairs = [(step, SparsePlain, key or None for step 0)]; idx: only those coefficients are
    filled in (the keys are then asked for X at the coefficients the plaintexts' monomials reach)"""
    n, L = E.n, E.L
    full = idx is None
    where = list(range(n)) if full else list(idx)
    base = [[np.zeros(n, dtype=object) for _ in range(L)] for _ in range(2)]
    Xacc = [np.zeros(n, dtype=object) for _ in range(2)]
    for step, pl, key in pairs:
        elt = pc.galois_elt_py(n, step) if step else 1
        g0 = dc.galois_limbs(E, ct[0], elt) if step else ct[0]
        for j in range(L):
            a = g0[j].astype(object)
            if full:
                base[0][j] = base[0][j] + pl.times(a)
            else:
                for l in where:
                    base[0][j][l] += pl.times_at(lambda i: int(a[i]), n, l)
        if not step:
            for j in range(L):
                a = ct[1][j].astype(object)
                if full:
                    base[1][j] = base[1][j] + pl.times(a)
                else:
                    for l in where:
                        base[1][j][l] += pl.times_at(lambda i: int(a[i]), n, l)
            continue
        d = dc.galois_limbs(E, ct[1], elt)
        if full:
            Xs = key.X(E, d)
            for i in range(2):
                Xacc[i] = Xacc[i] + pl.times(Xs[i])
        else:
            Xs = key.X(E, d, pl.needs(n, where))
            for i in range(2):
                for l in where:
                    Xacc[i][l] += pl.times_at(lambda m: int(Xs[i][m]), n, l)
    out = np.zeros((2, L, n), np.uint64)
    for i in range(2):
        for l in where:
            y = (int(Xacc[i][l]) % E.QP + E.h) // E.p
            for j in range(L):
                out[i, j, l] = (int(base[i][j][l]) + y) % E.q[j]
    return out


# ---- truth 1 for DENSE plaintexts ----
def mulmod_u64(a, b, q):
    """a * b mod q on uint64 arrays, q < 2^61: the quotient from an 80-bit floating product (within 2 of the true one), the remainder in
    wrapping 64-bit arithmetic, corrected; the first words are compared with Python integers on every call"""
    q = int(q)
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    assert np.finfo(np.longdouble).nmant >= 63 and q < (1 << 61)
    quo = np.floor(a.astype(np.longdouble) * b.astype(np.longdouble) / np.longdouble(q)).astype(np.uint64)
    r = (a * b - quo * np.uint64(q)).view(np.int64)
    r = np.where(r < 0, r + q, r)
    r = np.where(r < 0, r + q, r)
    r = np.where(r >= q, r - q, r)
    r = np.where(r >= q, r - q, r).astype(np.uint64)
    for i in range(min(4, len(r))):
        assert int(r[i]) == int(a[i]) * int(b[i]) % q
    return r


class DensePlain:
    """a plaintext given by its slot values (or by its polynomial): slots as the handle takes them, lift = the centred coefficients"""

    def __init__(self, E, slots=None, poly=None):
        if poly is None:
            full = np.zeros(E.n, np.uint64)
            full[:len(slots)] = slots
            poly = E.O.encode(full)
            self.slots = np.asarray(slots, np.uint64)
        else:
            poly = np.asarray(poly, np.uint64)
            self.slots = E.O.decode(poly)
            assert (E.O.encode(self.slots) == poly).all()
        self.poly = poly
        self.lift = np.array([centred(E.t, c) for c in poly], dtype=object)


def switch_sums(E, d, words):
    """[X_0, X_1], each the integer polynomial in [0, Q p) congruent to sum_I d[I] * key[I][i] modulo every prime of q u {p}, for a key
    given by its NTT-form words [L][2][K][N] (any words): per prime the cyclic-free product through the oracle's transforms (held to the
    definition by definition_common.check_ntt) and mulmod_u64, then the CRT in Python integers.  d: the digits [L][N] as residues in [0, q_I)"""
    coef = [(E.QP // qJ) * pow(E.QP // qJ, -1, qJ) % E.QP for qJ in E.q]
    out = []
    for i in range(2):
        acc = np.zeros(E.n, dtype=object)
        for J, qJ in enumerate(E.q):
            sJ = np.zeros(E.n, np.uint64)
            for I in range(E.L):
                dJ = E.O.ntt_fwd(J, d[I] % np.uint64(qJ))
                sJ = (sJ + mulmod_u64(dJ, words[I, i, J], qJ)) % np.uint64(qJ)
            acc = acc + E.O.ntt_inv(J, sJ).astype(object) * coef[J]
        out.append(acc % E.QP)
    return out


def dense_truth(E, pairs, ct, idx=None):
    """the definition's output [2][L][N] at the coefficients idx (None: all) for pairs = [(step, DensePlain, key words or None for step
    0)]: X of every child as an integer polynomial (switch_sums), the products with m~ as integer dot products"""
    n, L = E.n, E.L
    where = list(range(n)) if idx is None else list(idx)
    base = np.zeros((2, L, n), dtype=object)
    Xacc = np.zeros((2, n), dtype=object)
    for step, pl, words in pairs:
        elt = pc.galois_elt_py(n, step) if step else 1
        g0 = dc.galois_limbs(E, ct[0], elt) if step else ct[0]
        for j in range(L):
            a = g0[j].astype(object)
            for l in where:
                base[0, j, l] += dc.negacyclic_at(pl.lift, a, l)
        if not step:
            for j in range(L):
                a = ct[1][j].astype(object)
                for l in where:
                    base[1, j, l] += dc.negacyclic_at(pl.lift, a, l)
            continue
        Xs = switch_sums(E, dc.galois_limbs(E, ct[1], elt), words)
        for i in range(2):
            for l in where:
                Xacc[i, l] += dc.negacyclic_at(pl.lift, Xs[i], l)
    out = np.zeros((2, L, n), np.uint64)
    for i in range(2):
        for l in where:
            y = (int(Xacc[i, l]) % E.QP + E.h) // E.p
            for j in range(L):
                out[i, j, l] = (int(base[i, j, l]) + y) % E.q[j]
    return out


# ---- running the product ----
def run_plain_sum(X, mem, cts, slot_rows, steps, gk=None, in_place=False, n=None):
    B = len(cts)
    rows = X.plain_rows(np.stack(slot_rows))
    try:
        d_in = mem.to_dev(cts)
        out = d_in if in_place else mem.empty(tuple(cts.shape))
        X.rotate_plain_sum(d_in, rows, steps if n is None else steps[:n], out, B, gk=gk)
        return mem.to_host(out)
    finally:
        rows.destroy()


def expect_counters(X):
    want = 1 if X.query("row_kernel") == 1 and X.query("rot_hoist") != 0 else 0
    assert X.query("plain_sum_launches") == want, (X.query("plain_sum_launches"), want)
    assert X.query("plain_sum_mod_downs") == 1


def keyset_of(X, E, steps, keys):
    ks = X.keyset()
    for s, key in zip(steps, keys):
        if s:
            ks.set_galois(pc.galois_elt_py(E.n, s), key.words)
    return ks


def check_definition_sparse(make_ctx, E, mem, steps=(1, -1, 0, 3), seed=0):
    """truth 1, full vector: three-monomial keys, three-monomial plaintexts, three distinct items in one call, step 0 among the steps"""
    X = make_ctx()
    steps = list(steps)
    first = {s: i for i, s in reversed(list(enumerate(steps)))}   # a set holds one key per element: equal steps share theirs
    keys = [E.stored(("sparse", seed + 20 + first[s]), lambda i=first[s]: dc.SparseKey(E, seed + 20 + i)) if s else None for s in steps]
    plains = random_sparse_plains(E, len(steps), seed + 40)
    ks = keyset_of(X, E, steps, keys)
    cts = dc.switch_inputs(E, ("rows", 1), 3, seed + 5)
    got = run_plain_sum(X, mem, cts, [p.slots for p in plains], steps, gk=ks)
    expect_counters(X)
    pairs = list(zip(steps, plains, keys))
    for b in range(len(cts)):
        dc.assert_switch("rotate_plain_sum, item %d" % b, tuple(steps), got[b], plain_sum_truth(E, pairs, cts[b]))
    ks.close()
    X.close()


def check_definition_boundary(make_ctx, E, mem, seed=0):
    """truth 1, the rounding: two children whose X values cross m p - floor(p / 2) only as a SUM.  Child A holds m p - h - 3 (and m p - h - 1)
    at coefficient l, child B holds 5 (and 1): each alone rounds to m - 1 + 0, the sum to m.  A form that took a mod-down per child would
    be one short there.  Plaintexts: the constant 1; digits (1, 0, .., 0)"""
    X = make_ctx()
    rnd = random.Random(seed)
    p, h, Q, n = E.p, E.h, E.Q, E.n
    ms = [1, 2, Q - 1, Q // 2]
    A = [[rnd.randrange(E.QP) for _ in range(n)] for _ in range(2)]
    Bv = [[rnd.randrange(E.QP) for _ in range(n)] for _ in range(2)]
    crossing = []
    for i in range(2):
        for r, m in enumerate(ms):
            for s, (da, db) in enumerate(((3, 5), (1, 1), (1, 0))):   # (1, 0): the sum stays one below the boundary
                l = (3 * r + s) if i == 0 else n - 1 - (3 * r + s)
                A[i][l], Bv[i][l] = m * p - h - da, db
                if da <= db:
                    crossing.append((i, l, m))
    for i, l, m in crossing:
        assert (A[i][l] + h) // p == m - 1 and (Bv[i][l] + h) // p == 0 and (A[i][l] + Bv[i][l] + h) // p == m
    steps = [1, -2]
    keys = [ChosenKey(E, A), ChosenKey(E, Bv)]
    one = ones_plain(E)
    assert (one.slots == 1).all()
    ks = keyset_of(X, E, steps, keys)
    ct = dc.unit_input(E, ("rows", 1), np.random.default_rng(seed))
    got = run_plain_sum(X, mem, ct[None], [one.slots, one.slots], steps, gk=ks)
    want = plain_sum_truth(E, [(steps[0], one, keys[0]), (steps[1], one, keys[1])], ct)
    dc.assert_switch("rotate_plain_sum, rounding boundary", tuple(steps), got[0], want)
    # ... and the sum of the two rotations taken one at a time is NOT that (the definition is no composition): one short at the crossings
    for i, l, m in crossing[:2]:
        separate = ((A[i][l] + h) // p + (Bv[i][l] + h) // p) % E.q[0]
        assert separate != m % E.q[0]
    ks.close()
    X.close()


def check_definition_real_keys(make_ctx, S, E, mem, steps=(1, -3, 0), samples=6, seed=0):
    """truth 1 at sampled coefficients under the oracle's real keys (S: a setup on E's parameters holding the steps' keys)"""
    X = make_ctx()
    steps = list(steps)
    elt = {int(e): k for e, k in zip(S.gk.elts, S.gk.keys)}
    keys = [E.stored(("lifted", s), lambda s=s: dc.LiftedKey(E, elt[pc.galois_elt_py(E.n, s)])) if s else None for s in steps]
    plains = random_sparse_plains(E, len(steps), seed + 60)
    ks = keyset_of(X, E, steps, keys)
    cts = np.stack([S.O.encrypt(S.pk, np.random.default_rng(seed).integers(0, S.t, S.n, dtype=np.uint64), 700 + seed)])
    got = run_plain_sum(X, mem, cts, [p.slots for p in plains], steps, gk=ks)
    idx = dc.sample_indices(E.n, samples, seed + 1)
    want = plain_sum_truth(E, list(zip(steps, plains, keys)), cts[0], idx)
    dc.assert_switch("rotate_plain_sum, real keys", tuple(steps), got[0], want, idx)
    ks.close()
    X.close()


def check_definition_dense(make_ctx, S, E, mem, steps=(1, -3, 0, 2, -1), samples=12, seed=0, idx="sampled"):
    """truth 1 with DENSE plaintexts (uniform slot values: every coefficient of m~ is non-zero) under the oracle's real keys, on an
    encryption and on uniform words: `samples` + 4 coefficients, or with idx None the full vector"""
    X = make_ctx()
    steps = list(steps)
    elt = {int(e): k for e, k in zip(S.gk.elts, S.gk.keys)}
    words = [elt[pc.galois_elt_py(E.n, s)] if s else None for s in steps]
    rng = np.random.default_rng(seed + 70)
    plains = [DensePlain(E, slots=rng.integers(0, E.t, E.n, dtype=np.uint64)) for _ in steps]
    assert all((p.lift != 0).sum() > E.n // 2 for p in plains)
    ks = X.keyset()
    for s, w in zip(steps, words):
        if s:
            ks.set_galois(pc.galois_elt_py(E.n, s), w)
    cts = np.stack([S.O.encrypt(S.pk, rng.integers(0, S.t, S.n, dtype=np.uint64), 710 + seed), E.uniform(rng, 2)])
    cts[1][cts[1] == 0] = 1
    got = run_plain_sum(X, mem, cts, [p.slots for p in plains], steps, gk=ks)
    assert X.query("plain_sum_fallbacks") == 0
    expect_counters(X)
    where = None if idx is None else dc.sample_indices(E.n, samples, seed + 1)
    for b in range(len(cts)):
        want = dense_truth(E, list(zip(steps, plains, words)), cts[b], where)
        dc.assert_switch("rotate_plain_sum, dense plaintexts, item %d" % b, tuple(steps), got[b], want, where)
    ks.close()
    X.close()


def check_bounds(make_ctx, E, mem, pattern, step_pool, counts=None, samples=4):
    """'max': c0, c1, every key word and every lifted plaintext word at q_j - 1 (the plaintext -1: every NTT word is q_j - 1).  'alt': c0, c1
    and the key words alternate q_j - 1 with 0, and the plaintext's coefficients alternate -1 with 0 (no single plaintext has prescribed NTT
    words under all K primes at once; this one has every lifted coefficient at a bound).  'uniform': uniform words and a plaintext of
    uniform slot values, dense with effectively uniform lifted words.  `counts` children (default: plain_sum_fold + 1 and 17), the last
    one step 0, against the definition at sampled coefficients with the key taken as the integers its words stand for.  No zero residue
    in c1: this is about the lazy sums of the shared form, which must not take the fallback"""
    rng = np.random.default_rng(5)
    words = np.zeros(E.O.ksk_shape, np.uint64)
    for J in range(E.K):
        if pattern == "uniform":
            words[:, :, J] = rng.integers(0, E.q[J], words[:, :, J].shape, dtype=np.uint64)
        else:
            words[:, :, J, ::2 if pattern == "alt" else 1] = E.q[J] - 1
    poly = np.zeros(E.n, np.uint64)
    if pattern == "max":
        poly[0] = E.t - 1
        plain = DensePlain(E, poly=poly)
        assert (plain.slots == E.t - 1).all()
    elif pattern == "alt":
        poly[::2] = E.t - 1
        plain = DensePlain(E, poly=poly)
    else:
        plain = DensePlain(E, slots=rng.integers(0, E.t, E.n, dtype=np.uint64))
    ct = E.uniform(rng, 2) if pattern == "uniform" else E.maxed(2, alternate=pattern == "alt")
    ct[1][ct[1] == 0] = 1
    X = make_ctx()
    counts = (X.query("plain_sum_fold") + 1, 17) if counts is None else counts
    steps = [s for s in step_pool if s][:max(counts) - 1] + [0]
    ks = X.keyset()
    for s in steps:
        if s:
            ks.set_galois(pc.galois_elt_py(E.n, s), words)
    idx = dc.sample_indices(E.n, samples, 9)
    for n in counts:
        st = steps[-n:]
        got = run_plain_sum(X, mem, ct[None], [plain.slots] * n, st, gk=ks)
        assert X.query("plain_sum_fallbacks") == 0
        expect_counters(X)
        want = dense_truth(E, [(s, plain, words if s else None) for s in st], ct, idx)
        dc.assert_switch("rotate_plain_sum at the bounds", (pattern, n), got[0], want, idx)
    ks.close()
    X.close()


# ---- truth 2: one child, the plaintext 1 ----
def check_one_child_is_rotate_rows(X, S, mem, steps, B=2, seed=100):
    O = S.O
    ones = np.ones((1, S.n), np.uint64)
    cts = encryptions(S, B, seed)
    for s in steps:
        got = run_plain_sum(X, mem, cts, ones, [s])
        for b in range(B):
            want = cts[b] if s == 0 else O.rotate_rows(cts[b], s, S.gk)[0]
            assert (got[b] == want).all(), ("n = 1 with the all-ones plaintext differs from the oracle's rotate_rows", s, b)
        expect_counters(X)


# ---- truth 3: plain integers ----
def encryptions(S, B, seed=100):
    """(every slot of both rows random)"""
    O = S.O
    rng = np.random.default_rng(seed)
    return np.stack([O.encrypt(S.pk, O.encode(rng.integers(0, S.t, S.n, dtype=np.uint64)), seed + b) for b in range(B)])


def rotate_slots(v, step, n):
    """the slots of rotate_rows(v, step): both rows cyclically left by step"""
    h = n // 2
    return np.concatenate([np.roll(v[:h], -step), np.roll(v[h:], -step)])


def slot_sum(S, x_slots, slot_rows, steps):
    acc = np.zeros(S.n, dtype=object)
    for row, s in zip(slot_rows, steps):
        full = np.zeros(S.n, np.uint64)
        full[:len(row)] = row
        acc = acc + full.astype(object) * rotate_slots(x_slots, s, S.n).astype(object)
    return [int(v) % S.t for v in acc]


def check_slots(S, mem, got, cts, slot_rows, steps, O=None, sk=None, what=""):
    O, sk = O or S.O, S.sk if sk is None else sk
    budgets = []
    for b in range(len(cts)):
        budget = O.noise_budget(sk, got[b])
        assert budget > 0, ("no noise budget left", what, b)
        x = O.decode(O.decrypt(sk, cts[b]))
        dec = O.decode(O.decrypt(sk, got[b]))
        assert [int(v) for v in dec] == slot_sum(S, x, slot_rows, steps), ("slots differ from sum_k plain_k[s] x[rot_k(s)] mod t", what, b)
        budgets.append(budget)
    return budgets


def random_rows(S, n, count, seed):
    return np.random.default_rng(seed).integers(0, S.t, size=(n, count), dtype=np.uint64)


def check_primitive(X, S, mem, steps, B=2, seed=0, count=None, cts=None, gk=None, in_place=False, O=None, sk=None):
    """random dense plaintexts: the slots behind a decryption.  Returns (words, inputs, slot rows)"""
    rows = random_rows(S, len(steps), S.n if count is None else count, 900 + seed)
    cts = encryptions(S, B, 100 + 16 * seed) if cts is None else cts
    got = run_plain_sum(X, mem, cts, rows, steps, gk=gk, in_place=in_place)
    expect_counters(X)
    check_slots(S, mem, got, cts, rows, steps, O=O, sk=sk, what=tuple(steps))
    return got, cts, rows


# ---- the layer ----
def plain_affine(M, bias, x, t):
    rows, cols = M.shape
    return [(sum(int(M[i][j]) * int(x[j]) for j in range(cols)) + (int(bias[i]) if bias is not None else 0)) % t for i in range(rows)]


def layer_setup(orc, logn, q, rows, cols, t=T):
    """exactly the keys hhe_fc_open_galois_steps lists (by hand: mlp_common.hand_open_steps)"""
    return pc.setup_from_primes(orc, logn, q, t, extra_steps=mc.hand_open_steps(1 << logn, rows, cols), base_steps=())


def seeded_bias(t, rows, seed):
    return np.random.default_rng(seed).integers(0, t, size=rows, dtype=np.uint64)


def composed_layer(X, S, mem, M, bias, d_in, B):
    """the same layer from the public calls: hhe_rotate_rows_many_ks, hhe_multiply_plain per diagonal, hhe_add_many, the tail, hhe_add_plain"""
    rows, cols = M.shape
    r, c = mc.hand_open_shape(S.n, rows, cols)
    D = mc.hand_open_diagonals(M)
    O = S.O
    shape = (B,) + tuple(O.ct_shape)
    rot = mem.empty((r,) + shape)
    X.rotate_rows_many(d_in, [-e for e in range(r)], rot, B)
    for e in range(r):
        plain = mem.to_dev(O.encode(fp.slot_vector(S.n, D[e]))[None])
        X.multiply_plain(rot[e], plain, rot[e], B, bcast=True)
    y = mem.empty(shape)
    X.add_many(rot, r, y, B)
    tmp = mem.empty(shape)
    s = r
    while s < c:
        X.rotate_rows(y, s, tmp, B)
        X.add(y, tmp, y, B)
        s *= 2
    if bias is not None:
        X.add_plain(y, mem.to_dev(O.encode(fp.slot_vector(S.n, bias))[None]), y, B, bcast=True)
    X.sync()
    return mem.to_host(y)


def check_layer(X, S, mem, M, bias=None, B=2, seed=0, in_place=False, data=None, O=None, sk=None, gk=None, budget_beside=False):
    """slots [0, rows) of row 0 against (M x + b) mod t behind a decryption; the input carries a random value in every slot of both rows.
    Returns (words, data)"""
    rows, cols = M.shape
    O, sk = O or S.O, S.sk if sk is None else sk
    cts, xs, _ = mc.full_inputs(S, cols, B, 40 + seed) if data is None else data
    mat = X.plain_fc_open(M, bias)
    try:
        assert mat.bytes == 2 * mc.hand_open_shape(S.n, rows, cols)[0] * X.K * X.n * 8 + (X.n * 8 if bias is not None else 0)
        d_in = mem.to_dev(cts)
        out = d_in if in_place else mem.empty((B,) + tuple(cts.shape[1:]))
        got = mem.to_host(mat.apply(d_in, B, gk=gk, out=out))
    finally:
        mat.destroy()
    expect_counters(X)
    for b in range(B):
        budget = O.noise_budget(sk, got[b])
        assert budget > 0, ("no noise budget left", rows, cols, b)
        dec = O.decode(O.decrypt(sk, got[b]))
        assert [int(v) for v in dec[:rows]] == plain_affine(M, bias, xs[b], S.t), ("slots [0, rows) differ from (M x + b) mod t", rows, cols, b)
        if budget_beside and b == 0:
            comp = composed_layer(X, S, mem, M, bias, mem.to_dev(cts[:1]), 1)
            dec2 = O.decode(O.decrypt(sk, comp[0]))
            assert [int(v) for v in dec2[:rows]] == plain_affine(M, bias, xs[0], S.t)
            print("noise budget %dx%d: one mod-down %d bits, composed from the public calls %d bits" % (rows, cols, budget, O.noise_budget(sk, comp[0])))
    return got, (cts, xs, None)


# ---- refusals ----
def check_refusals(X, Y, S, mem, api):
    """every refusal of the primitive and of the layer, with `out` prefilled and untouched.  S holds keys of 1, -1, 4, 8 and the steps of the
    3 x 5 layer, none of 12; X, Y: two contexts of S with its keys in their default sets"""
    import ctypes as C

    import pytest
    O = S.O
    cts = encryptions(S, 1, seed=900)
    d_in = mem.to_dev(cts)
    rows = X.plain_rows(random_rows(S, 2, 8, 1))
    yrows = Y.plain_rows(random_rows(S, 2, 8, 1))

    def refused(code, call):
        out = mem.to_dev(np.full((1,) + tuple(O.ct_shape), 12345, np.uint64))
        with pytest.raises(api.HheError) as e:
            call(out)
        assert e.value.code == code, (code, str(e.value))
        assert (mem.to_host(out) == 12345).all()

    assert not X.has_galois_key(pc.galois_elt_py(S.n, 12)) and all(X.has_galois_key(pc.galois_elt_py(S.n, s)) for s in (4, 8))
    refused(api.ERR_NO_GALOIS_KEY, lambda out: X.rotate_plain_sum(d_in, rows, [1, 12], out, 1))      # 12 = 4 + 8 has no key of its own: no NAF chain
    refused(api.ERR_INVALID, lambda out: X.rotate_plain_sum(d_in, rows, [1, S.n // 2], out, 1))
    refused(api.ERR_INVALID, lambda out: X.rotate_plain_sum(d_in, rows, [-(S.n // 2)], out, 1))
    refused(api.ERR_INVALID, lambda out: X.rotate_plain_sum(d_in, rows, [], out, 1))
    refused(api.ERR_INVALID, lambda out: X.rotate_plain_sum(d_in, rows, [1, -1, 1], out, 1))          # more pairs than plaintexts
    refused(api.ERR_INVALID, lambda out: X.rotate_plain_sum(d_in, rows, [1], out, 0))
    refused(api.ERR_INVALID, lambda out: X.rotate_plain_sum(d_in, yrows, [1], out, 1))                # a handle of another context
    refused(api.ERR_INVALID, lambda out: X.rotate_plain_sum(d_in, None, [1], out, 1))
    refused(api.ERR_INVALID, lambda out: X.rotate_plain_sum(None, rows, [1], out, 1))
    with pytest.raises(api.HheError) as e:
        X.rotate_plain_sum(d_in, rows, [1], None, 1)
    assert e.value.code == api.ERR_INVALID
    refused(api.ERR_INVALID, lambda out: X._chk(X.lib.hhe_rotate_plain_sum_ks(X.h, None, rows.h, None, C.c_size_t(1), api._ptr(d_in), api._ptr(out),
                                                                            C.c_size_t(1))))   # null steps_hptr: the C ABI directly
    yks = Y.keyset()
    refused(api.ERR_INVALID, lambda out: X.rotate_plain_sum(d_in, rows, [1], out, 1, gk=yks))
    yks.close()
    empty = X.keyset()
    refused(api.ERR_NO_GALOIS_KEY, lambda out: X.rotate_plain_sum(d_in, rows, [1], out, 1, gk=empty))
    # step 0 alone needs no key at all
    out = mem.empty((1,) + tuple(O.ct_shape))
    X.rotate_plain_sum(d_in, rows, [0], out, 1, gk=empty)
    # handle creation
    for bad in (np.full((1, 4), S.t, np.uint64), np.zeros((1, S.n + 1), np.uint64), np.zeros((0, 4), np.uint64), np.zeros(((1 << 20) + 1, 1), np.uint64)):
        with pytest.raises(api.HheError) as e:
            X.plain_rows(bad)
        assert e.value.code == api.ERR_INVALID
    # the layer
    M = fp.seeded_matrix(S.t, 3, 5, 3)
    mat, ymat = X.plain_fc_open(M), Y.plain_fc_open(M)
    refused(api.ERR_INVALID, lambda out: X._chk(X.lib.hhe_fc_open_plain_ks(X.h, None, ymat.h, api._ptr(d_in), api._ptr(out), 1)))   # a handle of another context
    refused(api.ERR_INVALID, lambda out: X._chk(X.lib.hhe_fc_open_plain_ks(X.h, None, None, api._ptr(d_in), api._ptr(out), 1)))
    refused(api.ERR_INVALID, lambda out: mat.apply(d_in, 0, out=out))
    refused(api.ERR_NO_GALOIS_KEY, lambda out: mat.apply(d_in, 1, gk=empty, out=out))
    elt = {int(e): k for e, k in zip(S.gk.elts, S.gk.keys)}
    need = mc.hand_open_steps(S.n, 3, 5)
    for missing in need:   # every step of hhe_fc_open_galois_steps is needed, each as a key of its own
        ks = X.keyset()
        for s in need:
            if s != missing:
                ks.set_galois(pc.galois_elt_py(S.n, s), elt[pc.galois_elt_py(S.n, s)])
        refused(api.ERR_NO_GALOIS_KEY, lambda out: mat.apply(d_in, 1, gk=ks, out=out))
        ks.close()
    empty.close()
    for rws, cls, bias, code in ((0, 5, None, api.ERR_INVALID), (3, 0, None, api.ERR_INVALID), (3, S.n // 2, None, api.ERR_TOO_FEW_SLOTS)):
        with pytest.raises(api.HheError) as e:
            X.plain_fc_open(np.zeros((rws, cls), np.uint64), bias)
        assert e.value.code == code
    with pytest.raises(api.HheError) as e:
        X.plain_fc_open(M, np.full(3, S.t, np.uint64))
    assert e.value.code == api.ERR_INVALID
    with pytest.raises(api.HheError) as e:
        X.plain_fc_open(np.full((3, 5), S.t, np.uint64))
    assert e.value.code == api.ERR_INVALID
    for h in (mat, ymat, rows, yrows):
        h.destroy()
