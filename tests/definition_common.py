"""Integer definitions of the ciphertext side, shared by the emulator suite (numpy memory) and the GPU suite (torch memory).

Every other test of the negacyclic NTT, the Galois map, the generic key switch, add_plain and BEHZ multiply asserts product ==
oracle, and the oracle's RNS code was written from the same reading of SEAL as the product's.  This module states each operation
once more, in Python integers, with no transform and no RNS trick, and holds the oracle, the emulator and the kernels to it:

  a. the minimal primitive 2N-th root of every modulus a context transforms;
  b. NTT_m(x)[bitrev(k)] = sum_i x[i] psi^((2k+1) i) mod m;
  c. the coefficient-domain Galois map;
  d. the key switch (SURVEY A.4 with its RNS taken away): X_k = the integer in [0, Q p) congruent to sum_I d[I] * key[I][k] modulo
     every coefficient prime, output limb j = running[k][j] + floor((X_k + floor(p / 2)) / p) mod q_j;
  e. add_plain / sub_plain: c0[j] +- floor((m Q + (t + 1) / 2) / t) mod q_j;
  f. BEHZ multiply as a distance: |centred(CRT(out) - floor((2 t d + Q) / (2 Q)))| <= L + 1.

The plaintext boundary continues the list in codec_common.py, on the Env, the tables and the roots of this file: g. the slots
(hhe_encode and the decode half of hhe_decrypt as evaluations at psi_t^(e_i)) and h. decrypt (the scale-and-round of hhe_decrypt and
hhe_decrypt_level with its RNS removed).

No expected value here comes from a transform, a CRT or a key switch of the oracle or of the product, with two exceptions that come
after b has held the oracle's transforms to the definition: a dense key of chosen COEFFICIENTS is brought to the NTT form the ABI
takes (DenseKey), and the oracle's real keys are brought back to coefficients (lift_key).  The oracle's and the product's
relinearize / apply_galois / rotate_rows / rotate_columns and transforms appear below only as the parties under test."""
import random

import numpy as np

import parity_common as pc
import plain_modulus_common as pm

T16, T33, T60 = pm.T16, pm.T33, pm.T60


# ---- a. roots ----
def minimal_primitive_root(m, n):
    """the smallest primitive 2n-th root of unity modulo the prime m: g^((m-1)/2n) for the first g that gives a primitive one, then
    the minimum over its odd powers (the primitive 2n-th roots are exactly those)"""
    m, n = int(m), int(n)
    assert (m - 1) % (2 * n) == 0, (m, n)
    g = 2
    while True:
        r = pow(g, (m - 1) // (2 * n), m)
        if pow(r, n, m) == m - 1:
            break
        g += 1
    best, cur, r2 = r, r, r * r % m
    for _ in range(n):
        best = min(best, cur)
        cur = cur * r2 % m
    return best


def bitrev_table(logn):
    k = np.arange(1 << logn, dtype=np.int64)
    br = np.zeros(1 << logn, np.int64)
    for b in range(logn):
        br |= ((k >> b) & 1) << (logn - 1 - b)
    return br


class Env:
    """One parameter set: the oracle, the moduli a context transforms (K coefficient primes, L + 1 BEHZ primes, t) and, per modulus,
    this file's own root and the table of its 2N powers.  Made once per parameter set and shared; nothing writes to it."""

    def __init__(self, orc, logn, q, t):
        self.orc, self.logn, self.n, self.q, self.t = orc, logn, 1 << logn, [int(v) for v in q], int(t)
        self.O = orc.Oracle(logn, self.q, self.t)
        self.K, self.L = len(self.q), len(self.q) - 1
        self.Q = 1
        for v in self.q[:self.L]:
            self.Q *= v
        self.p = self.q[-1]
        self.QP, self.h = self.Q * self.p, self.p // 2
        self.br = bitrev_table(logn)
        self.bsk = [self.O.query("bsk", i) for i in range(self.L + 1)]
        assert (self.t - 1) % (2 * self.n) == 0, "t does not batch at this degree: the context transforms nothing modulo t"
        self.mods = self.q + self.bsk + [self.t]
        self._tab, self._keys, self.store = {}, None, {}

    def orc_index(self, mi):
        return mi if mi < 2 * self.K else -1

    def table(self, mi):
        """(psi, [psi^i for i < 2N] as Python integers, the same as uint64)"""
        if mi not in self._tab:
            m = self.mods[mi]
            psi = minimal_primitive_root(m, self.n)
            P = [1] * (2 * self.n)
            for i in range(1, 2 * self.n):
                P[i] = P[i - 1] * psi % m
            assert P[self.n] == m - 1
            self._tab[mi] = (psi, P, np.array(P, dtype=np.uint64))
        return self._tab[mi]

    def keypair(self):
        if self._keys is None:
            sk = self.O.keygen_secret(1)
            self._keys = (sk, self.O.keygen_public(sk, 2))
        return self._keys

    def stored(self, key, make):
        if key not in self.store:
            self.store[key] = make()
        return self.store[key]

    def encryption(self, seed):
        rng = np.random.default_rng(seed)
        return self.O.encrypt(self.keypair()[1], rng.integers(0, self.t, self.n, dtype=np.uint64), 500 + seed)

    def uniform(self, rng, size):
        a = np.zeros((size, self.L, self.n), np.uint64)
        for j in range(self.L):
            a[:, j] = rng.integers(0, self.q[j], (size, self.n), dtype=np.uint64)
        return a

    def maxed(self, size, alternate=False):
        a = np.zeros((size, self.L, self.n), np.uint64)
        for j in range(self.L):
            a[:, j, ::2 if alternate else 1] = self.q[j] - 1
        return a

    def half(self, size, negative=False):
        """every coefficient the residues of (Q - 1) / 2, the largest centred value; negative: of (Q + 1) / 2, which is -(Q - 1) / 2"""
        v = (self.Q + 1) // 2 if negative else (self.Q - 1) // 2
        a = np.zeros((size, self.L, self.n), np.uint64)
        for j in range(self.L):
            a[:, j] = v % self.q[j]
        return a


_envs = {}


def env(orc, logn, q, t):
    key = (logn, tuple(int(v) for v in q), int(t))
    if key not in _envs:
        _envs[key] = Env(orc, logn, q, t)
    return _envs[key]


def case(orc, api, lib, name):
    """(logn, primes, t, expected row_kernel, expected digit_reduce or None).  n1024 / n2048: ragged tiles; rowNN: 3 x 60 bits on the
    row kernel (n2 = 6, 7, 7, 8, 8 with n1 = 6, 6, 7, 7, 8 at logn = 12 .. 16); nttNN: CoeffModulus::Create of 3 + 1 primes of 60 bits;
    bench15: the benchmark's parameters; a single letter: parity_common.dispatch_case.  65537 does not batch at N = 65536, so the
    contexts of that degree take 8088322049 as the reference does."""
    cm = orc.coeff_modulus_create
    if name in ("n1024", "n2048"):
        logn = 10 if name == "n1024" else 11
        return logn, cm(1 << logn, [50] * 3), T16, 0, None
    if name[:3] in ("row", "ntt"):
        logn = int(name[3:])
        return logn, cm(1 << logn, [60] * (3 if name[:3] == "row" else 4)), T33 if logn == 16 else T16, int(logn >= 12), None
    if name == "bench15":
        return 15, cm(32768, [60] * 4), T16, 1, None
    return pc.dispatch_case(orc, api, lib, name)


def setup(orc, api, lib, name):
    """(Env, factory of contexts that have asserted their dispatch) of a case"""
    logn, q, t, row_kernel, digit_reduce = case(orc, api, lib, name)

    def make_ctx():
        X = api.Context(logn, q, t, lib=lib)
        pc.assert_dispatch(X, q, row_kernel, digit_reduce)
        return X
    return env(orc, logn, q, t), make_ctx


def check_roots(make_ctx, E):
    """a. this file's minimal root equals the product's and the oracle's for every coefficient prime; the BEHZ primes and t have no
    query and are pinned through b, which transforms with this file's roots"""
    X = make_ctx()
    for i in range(E.K):
        psi = E.table(i)[0]
        assert pow(psi, E.n, E.q[i]) == E.q[i] - 1
        assert E.O.query("root", i) == psi, ("oracle root", i)
        assert X.query("root", i) == psi, ("product root", i)
        assert E.orc.minimal_primitive_root(2 * E.n, E.q[i]) == psi
    for i in range(E.L + 1):
        assert X.query("bsk", i) == E.bsk[i]
    X.close()


# ---- b. NTT ----
def monomial_image(E, mi, terms):
    """NTT_m(sum_r c_r X^(e_r)), full vector: word bitrev(k) is sum_r c_r psi^((2k+1) e_r mod 2N), the powers read from the table.
    A coefficient other than 1 and m - 1 costs one scaled copy of the table, 2N multiplications."""
    m, n = E.mods[mi], E.n
    _, P, Pu = E.table(mi)
    odd = 2 * np.arange(n, dtype=np.int64) + 1
    acc = np.zeros(n, np.uint64)
    for c, e in terms:
        c = int(c) % m
        if e == 0:
            term = np.full(n, c, np.uint64)
        else:
            tab = Pu if c == 1 else np.uint64(m) - Pu if c == m - 1 else np.array([c * x % m for x in P], dtype=np.uint64)
            term = tab[(odd * e) % (2 * n)]
        acc = (acc + term) % np.uint64(m)   # two residues below 2^61: no wrap
    out = np.zeros(n, np.uint64)
    out[E.br] = acc
    return out


def ntt_point(E, mi, x_list, k):
    """word bitrev(k) of NTT_m(x) by Horner: sum_i x[i] w^i with w = psi^(2k+1)"""
    m = E.mods[mi]
    w = E.table(mi)[1][(2 * k + 1) % (2 * E.n)]
    acc = 0
    for v in reversed(x_list):
        acc = (acc * w + v) % m
    return acc


def sample_indices(n, count, seed):
    """0, 1, N/2, N - 1 and `count` seeded ones"""
    rng = np.random.default_rng(seed)
    return [0, 1, n // 2, n - 1] + [int(v) for v in rng.integers(2, n - 1, count)]


def sparse_polys(E, seed):
    """per modulus three monomials: coefficients 1, m - 1 and a random one over the exponents 0, N - 1 and a random one, the pairing
    rotating with the modulus; (polynomials [nm][N], their term lists)"""
    rng = np.random.default_rng(seed)
    n, nm = E.n, len(E.mods)
    polys, terms = np.zeros((nm, n), np.uint64), []
    for mi, m in enumerate(E.mods):
        cs = [1, m - 1, int(rng.integers(2, m - 1))]
        es = [0, n - 1, int(rng.integers(1, n - 1))]
        tl = [(cs[(r + mi) % 3], es[r]) for r in range(3)]
        for c, e in tl:
            polys[mi, e] = c
        terms.append(tl)
    return polys, terms


def dense_polys(E, kind, seed):
    rng = np.random.default_rng(seed)
    a = np.zeros((len(E.mods), E.n), np.uint64)
    for mi, m in enumerate(E.mods):
        if kind == "uniform":
            a[mi] = rng.integers(0, m, E.n, dtype=np.uint64)
        else:
            a[mi, ::2 if kind == "alt" else 1] = m - 1
    return a


def check_ntt(make_ctx, E, mem, samples=12, seed=0):
    """b. hhe_ntt and the oracle's ntt_fwd against the definition over every modulus of the context: the full vector on three
    monomials, `samples` + 4 output words by Horner on uniform residues, on every word at m - 1 and on m - 1 alternating with 0.
    The inverse: inverse(forward(x)) == x on all of them, and the inverse of the closed-form image returns the monomials."""
    X, O, nm = make_ctx(), E.O, len(E.mods)

    def product(a, inverse):
        d = mem.to_dev(a)
        X.ntt(d, nm, 0, nm, inverse)
        return mem.to_host(d)

    def oracle(a, inverse):
        f = O.ntt_inv if inverse else O.ntt_fwd
        return np.stack([f(E.orc_index(mi), a[mi]) for mi in range(nm)])

    polys, terms = sparse_polys(E, seed)
    image = np.stack([monomial_image(E, mi, terms[mi]) for mi in range(nm)])
    for who, f in (("oracle", oracle), ("product", product)):
        got = f(polys, False)
        bad = [mi for mi in range(nm) if not (got[mi] == image[mi]).all()]
        assert not bad, (who, "forward transform of three monomials differs from the definition; modulus indices:", bad)
        got = f(image, True)
        bad = [mi for mi in range(nm) if not (got[mi] == polys[mi]).all()]
        assert not bad, (who, "inverse transform of the closed-form image does not return the monomials; modulus indices:", bad)
    idx = sample_indices(E.n, samples, seed + 1)
    for kind in ("uniform", "max", "alt"):
        a = dense_polys(E, kind, seed + 2)
        want = [[ntt_point(E, mi, a[mi].tolist(), k) for k in idx] for mi in range(nm)]
        for who, f in (("oracle", oracle), ("product", product)):
            got = f(a, False)
            bad = [(mi, k) for mi in range(nm) for s, k in enumerate(idx) if int(got[mi, E.br[k]]) != want[mi][s]]
            assert not bad, (who, kind, "forward transform differs from the definition at (modulus index, k):", bad)
            assert (f(got, True) == a).all(), (who, kind, "inverse(forward(x)) != x")
    X.close()


# ---- c. Galois map ----
_gmaps = {}


def galois_map(n, elt):
    """SURVEY A.3 as a loop: coefficient i goes to i elt mod N, negated when bit log N of i elt is set"""
    if (n, elt) not in _gmaps:
        idx, neg = [0] * n, [False] * n
        for i in range(n):
            raw = i * elt
            idx[i], neg[i] = raw % n, bool((raw // n) & 1)
        _gmaps[(n, elt)] = (np.array(idx), np.array(neg))
    return _gmaps[(n, elt)]


def galois_limbs(E, a, elt):
    """the map on [L][N] residues"""
    idx, neg = galois_map(E.n, elt)
    out = np.zeros_like(a)
    for j in range(E.L):
        qj = np.uint64(E.q[j])
        out[j, idx] = np.where(neg, (qj - a[j]) % qj, a[j])
    return out


def check_galois_map(E, seed=0):
    """the oracle's coefficient-domain map against the loop, for the column swap, 3 and a seeded odd element"""
    rng = np.random.default_rng(seed)
    a = E.uniform(rng, 1)[0]
    a[:, 0] = 0   # the negation of 0 stays 0
    for elt in (2 * E.n - 1, 3, 2 * int(rng.integers(2, E.n - 1)) + 1):
        want = galois_limbs(E, a, elt)
        for j in range(E.L):
            assert (E.O.galois_poly(j, elt, a[j]) == want[j]).all(), (elt, j)


def naf(v):
    """non-adjacent form, least significant term first (util::naf)"""
    sign, v, out, i = (-1 if v < 0 else 1), abs(v), [], 0
    while v:
        z = 2 - (v & 3) if v & 1 else 0
        v = (v - z) >> 1
        if z:
            out.append(sign * z * (1 << i))
        i += 1
    return out


# ---- d. key switch ----
def mod_down(E, X):
    """[L][N] words floor((X + h) / p) mod q_j of an object array of integers X"""
    y = (X + E.h) // E.p
    return np.stack([(y % qj).astype(np.uint64) for qj in E.q[:E.L]])


def switch_operands(E, entry, ct):
    """(d [L][N], running [2][L][N]) of an entry point: relinearize takes d = c2 and keeps (c0, c1); the rotations take
    d = galois(c1) and keep (galois(c0), 0)"""
    if entry[0] == "relin":
        return ct[2], ct[:2]
    elt = entry_elt(E, entry)
    return galois_limbs(E, ct[1], elt), np.stack([galois_limbs(E, ct[0], elt), np.zeros_like(ct[0])])


def entry_elt(E, entry):
    return {"galois": lambda: entry[1], "rows": lambda: pc.galois_elt_py(E.n, entry[1]), "cols": lambda: 2 * E.n - 1}[entry[0]]()


def add_running(E, running, low):
    out = np.zeros_like(running)
    for j in range(E.L):
        out[:, j] = (running[:, j] + low[:, j]) % np.uint64(E.q[j])
    return out


def negacyclic_shift(a, e):
    """a X^e in Z[X] / (X^N + 1) on an object array"""
    if e == 0:
        return a
    out = np.empty(len(a), dtype=object)
    out[e:] = a[:len(a) - e]
    out[:e] = -a[len(a) - e:]
    return out


class SparseKey:
    """key[I][k] = three monomials with coefficients that are integers mod Q p, at the exponents 0, N - 1 and a seeded one;
    key[0][0] has Q p - 1 at exponent 0.  words: its NTT form [L][2][K][N], limb by limb from the power tables."""

    def __init__(self, E, seed):
        rnd = random.Random(seed)
        self.terms = [[[(E.QP - 1 if (I, k) == (0, 0) else rnd.randrange(E.QP), 0), (rnd.randrange(E.QP), E.n - 1),
                        (rnd.randrange(E.QP), rnd.randrange(1, E.n - 1))] for k in range(2)] for I in range(E.L)]
        self.words = np.zeros(E.O.ksk_shape, np.uint64)
        for I in range(E.L):
            for k in range(2):
                for J in range(E.K):
                    self.words[I, k, J] = monomial_image(E, J, self.terms[I][k])

    def X(self, E, d, idx=None):
        """[X_0, X_1]: 3 L shifted, signed, scaled copies of the digits, reduced into [0, Q p)"""
        dO = [d[I].astype(object) for I in range(E.L)]
        out = []
        for k in range(2):
            acc = np.zeros(E.n, dtype=object)
            for I in range(E.L):
                for c, e in self.terms[I][k]:
                    acc = acc + negacyclic_shift(dO[I] * c, e)
            out.append(acc % E.QP)
        return out


def boundary_values(E):
    p, h, Q = E.p, E.h, E.Q
    vals = [m * p - h + s for m in (0, 1, 2, Q - 1, Q) for s in (-1, 0, 1)] + [0, h, E.QP - 1]
    return [v for v in vals if 0 <= v < E.QP]


class DenseKey:
    """key[0][k] = a dense polynomial whose coefficient l IS the wanted X_k[l] (the digits are the constant polynomial 1 in limb 0
    and 0 elsewhere): the values around every multiple of p that matters, placed at the front of X_0 and at the back of X_1, seeded
    values elsewhere.  Brought to NTT form with the oracle's ntt_fwd, which check_ntt holds to the definition."""

    def __init__(self, E, seed):
        rnd = random.Random(seed)
        edge = boundary_values(E)
        self.Xs = []
        for k in range(2):
            v = [rnd.randrange(E.QP) for _ in range(E.n)]
            if k == 0:
                v[:len(edge)] = edge
            else:
                v[E.n - len(edge):] = edge
            self.Xs.append(np.array(v, dtype=object))
        self.words = np.zeros(E.O.ksk_shape, np.uint64)
        for k in range(2):
            for J in range(E.K):
                self.words[0, k, J] = E.O.ntt_fwd(J, (self.Xs[k] % E.q[J]).astype(np.uint64))

    def X(self, E, d, idx=None):
        unit = np.zeros((E.L, E.n), np.uint64)
        unit[0, 0] = 1
        assert (d == unit).all(), "the rounding-boundary key needs the digits (1, 0, ..., 0)"
        return self.Xs


def unit_input(E, entry, rng):
    """an input whose digits are (1, 0, ..., 0): the switched polynomial is the constant 1 in limb 0 (the Galois map fixes it)"""
    ct = E.uniform(rng, 3 if entry[0] == "relin" else 2)
    ct[-1] = 0
    ct[-1, 0, 0] = 1
    return ct


def lift_key(E, ksk):
    """a key in NTT form [L][2][K][N] -> object array [L][2][N] of its coefficients as integers in [0, Q p): the oracle's ntt_inv
    per limb (held to the definition by check_ntt), then a CRT lift per coefficient in Python integers"""
    coef = [(E.QP // qJ) * pow(E.QP // qJ, -1, qJ) % E.QP for qJ in E.q]
    out = np.empty((E.L, 2, E.n), dtype=object)
    for I in range(E.L):
        for k in range(2):
            acc = np.zeros(E.n, dtype=object)
            for J in range(E.K):
                acc = acc + E.O.ntt_inv(J, ksk[I, k, J]).astype(object) * coef[J]
            out[I, k] = acc % E.QP
    return out


def negacyclic_at(a, b, l):
    """coefficient l of a * b in Z[X] / (X^N + 1), object arrays"""
    n = len(a)
    rev = b[(l - np.arange(n)) % n]
    s = int(np.dot(a[:l + 1], rev[:l + 1]))
    return s - int(np.dot(a[l + 1:], rev[l + 1:])) if l + 1 < n else s


class LiftedKey:
    """a real key of the oracle: X_k at chosen coefficients only, N L big-integer products each"""

    def __init__(self, E, ksk):
        self.words, self.coeffs = ksk, lift_key(E, ksk)

    def X(self, E, d, idx):
        dO = [d[I].astype(object) for I in range(E.L)]
        return [{l: sum(negacyclic_at(dO[I], self.coeffs[I, k], l) for I in range(E.L)) % E.QP for l in idx} for k in range(2)]


def switch_truth(E, entry, key, ct, idx=None):
    """the definition's output [2][L][N] (idx: only those coefficients are filled in)"""
    d, running = switch_operands(E, entry, ct)
    Xs = key.X(E, d, idx)
    if idx is None:
        return add_running(E, running, np.stack([mod_down(E, Xs[k]) for k in range(2)]))
    out = np.zeros((2, E.L, E.n), np.uint64)
    for k in range(2):
        for l in idx:
            y = (Xs[k][l] + E.h) // E.p
            for j in range(E.L):
                out[k, j, l] = (int(running[k, j, l]) + y) % E.q[j]
    return out


def run_product(X, E, mem, entry, words, cts, in_place=False):
    """one call of the entry point on the batch cts with the key `words` in a key set of its own"""
    ks = X.keyset()
    B = len(cts)
    d_in = mem.to_dev(cts)
    out = d_in if in_place else mem.empty((B, 2, E.L, E.n))
    if entry[0] == "relin":
        ks.set_relin(words)
        X.relinearize(d_in, out, B, rk=ks)
    else:
        ks.set_galois(entry_elt(E, entry), words)
        if entry[0] == "galois":
            X.apply_galois(d_in, entry[1], out, B, gk=ks)
        elif entry[0] == "rows":
            X.rotate_rows(d_in, entry[1], out, B, gk=ks)
        else:
            X.rotate_columns(d_in, out, B, gk=ks)
    got = mem.to_host(out)
    ks.close()
    return got


def run_oracle(E, entry, words, ct):
    O = E.O
    if entry[0] == "relin":
        return O.relinearize(ct, words)
    if entry[0] == "galois":
        return O.apply_galois(ct, entry[1], words)
    gk = E.orc.GaloisKeys([entry_elt(E, entry)], words[None])
    return O.rotate_rows(ct, entry[1], gk)[0] if entry[0] == "rows" else O.rotate_columns(ct, gk)


def assert_switch(who, entry, got, want, idx=None):
    if idx is not None:
        got, want = got[..., idx], want[..., idx]
    bad = [(k, j, int(np.argmax(got[k, j] != want[k, j]))) for k in range(2) for j in range(got.shape[1]) if not (got[k, j] == want[k, j]).all()]
    assert not bad, (who, entry, "differs from the integer definition at (component, limb, first position):", bad)


def entries(E):
    """the four entry points; the step and the element are arbitrary, every key here is made for the element the call names"""
    return [("relin",), ("galois", 3), ("rows", -1), ("cols",)]


def switch_inputs(E, entry, count, seed):
    """`count` distinct items: from an encryption (for relinearize the oracle's product of two), uniform words, every word at q_j - 1"""
    rng = np.random.default_rng(seed)
    size = 3 if entry[0] == "relin" else 2
    enc = E.encryption(seed)
    first = E.O.multiply(enc, E.encryption(seed + 1)) if size == 3 else enc
    return np.stack([first, E.uniform(rng, size), E.maxed(size)][:count])


def check_switch_sparse(make_ctx, E, mem, B=3, in_place=True, seed=0):
    """d, sparse keys: every entry point, product and oracle, full output vector, B distinct items in one call; one call in place"""
    X = make_ctx()
    key = E.stored(("sparse", seed), lambda: SparseKey(E, seed))
    for e_i, entry in enumerate(entries(E)):
        cts = switch_inputs(E, entry, B, seed + 10 * e_i)
        want = [switch_truth(E, entry, key, ct) for ct in cts]
        for b in range(B):
            assert_switch("oracle, item %d" % b, entry, run_oracle(E, entry, key.words, cts[b]), want[b])
        got = run_product(X, E, mem, entry, key.words, cts)
        for b in range(B):
            assert_switch("product, item %d" % b, entry, got[b], want[b])
        if in_place and entry[0] == "rows":
            got = run_product(X, E, mem, entry, key.words, cts, in_place=True)
            for b in range(B):
                assert_switch("product in place, item %d" % b, entry, got[b], want[b])
    X.close()


def check_switch_boundary(make_ctx, E, mem, seed=0):
    """d, rounding boundary: X_k chosen coefficient by coefficient around the multiples of p, full output vector"""
    X = make_ctx()
    key = E.stored(("dense", seed), lambda: DenseKey(E, seed))
    assert len(boundary_values(E)) >= 14
    rng = np.random.default_rng(seed)
    for entry in entries(E):
        ct = unit_input(E, entry, rng)
        want = switch_truth(E, entry, key, ct)
        assert_switch("oracle", entry, run_oracle(E, entry, key.words, ct), want)
        assert_switch("product", entry, run_product(X, E, mem, entry, key.words, ct[None])[0], want)
    X.close()


def real_keys(E):
    """the oracle's relin key and Galois keys of the elements entries() names, lifted once per parameter set"""
    if "real" not in E.store:
        sk = E.keypair()[0]
        elts = [entry_elt(E, e) for e in entries(E)[1:]]
        gk = E.O.keygen_galois(sk, elts, 7)
        keys = {("relin",): LiftedKey(E, E.O.keygen_relin(sk, 3))}
        for e, w in zip(entries(E)[1:], gk.keys):
            keys[e] = LiftedKey(E, w)
        E.store["real"] = keys
    return E.store["real"]


def check_switch_real(make_ctx, E, mem, samples=12, seed=0, which=None):
    """d, real keys, sampled: X_k at 0, 1, N/2, N - 1 and `samples` seeded coefficients; d from an encryption and, for relinearize,
    once more from words all at q_j - 1"""
    X = make_ctx()
    keys = real_keys(E)
    idx = sample_indices(E.n, samples, seed + 3)
    for e_i, entry in enumerate(which or entries(E)):
        cts = switch_inputs(E, entry, 3, seed + 10 * e_i)[[0, 2] if entry[0] == "relin" else [0]]
        want = [switch_truth(E, entry, keys[entry], ct, idx) for ct in cts]
        for b, ct in enumerate(cts):
            assert_switch("oracle, item %d" % b, entry, run_oracle(E, entry, keys[entry].words, ct), want[b], idx)
        got = run_product(X, E, mem, entry, keys[entry].words, cts)
        for b in range(len(cts)):
            assert_switch("product, item %d" % b, entry, got[b], want[b], idx)
    X.close()


def check_switch_naf(make_ctx, E, mem, step=3, seed=0):
    """d, a rotate_rows whose step has no key: served through its NAF terms in vector order (3 = -1 + 4), each term one sparse-key
    switch; the truth is the composition of the definition, term by term"""
    X = make_ctx()
    terms = [s for s in naf(step) if abs(s) != E.n // 2]
    assert len(terms) > 1 and terms == E.orc.naf(step)
    keys = {s: E.stored(("sparse", seed + 1 + i), lambda i=i: SparseKey(E, seed + 1 + i)) for i, s in enumerate(terms)}
    ct = switch_inputs(E, ("rows", step), 1, seed + 77)[0]
    want = ct
    for s in terms:
        want = switch_truth(E, ("rows", s), keys[s], want)
    elts = [pc.galois_elt_py(E.n, s) for s in terms]
    assert pc.galois_elt_py(E.n, step) not in elts
    ref, nks = E.O.rotate_rows(ct, step, E.orc.GaloisKeys(elts, np.stack([keys[s].words for s in terms])))
    assert nks == len(terms)
    assert_switch("oracle", ("rows", step), ref, want)
    ks = X.keyset()
    for s, e in zip(terms, elts):
        ks.set_galois(e, keys[s].words)
    out = mem.empty((1, 2, E.L, E.n))
    X.rotate_rows(mem.to_dev(ct[None]), step, out, 1, gk=ks)
    assert_switch("product", ("rows", step), mem.to_host(out)[0], want)
    ks.close()
    X.close()


# ---- e. add_plain / sub_plain ----
def scaled_plain(E, plain):
    """[L][N] words floor((m Q + (t + 1) / 2) / t) mod q_j, the one integer expression"""
    y = (plain.astype(object) * E.Q + (E.t + 1) // 2) // E.t
    return np.stack([(y % qj).astype(np.uint64) for qj in E.q[:E.L]])


def plain_case(orc, api, lib, name):
    """(Env, context factory) of an add_plain case: the two contexts at 65537 and 8088322049, and 1096486890805657601 over the 15
    primes of 55 bits of plain_modulus_common.meaning_setup, where t > 2 q_j"""
    where, t = name.split("-")
    if t == "t60":
        q = orc.coeff_modulus_create(1024, [pm.MEANING_BITS] * pm.MEANING_PRIMES)
        assert pm.regime_of(T60, q) == "slow"
        return env(orc, 10, q, T60), lambda: api.Context(10, q, T60, lib=lib)
    logn, q, _, row_kernel, _ = case(orc, api, lib, where)
    t = {"t16": T16, "t33": T33}[t]

    def make_ctx():
        X = api.Context(logn, q, t, lib=lib)
        pc.assert_dispatch(X, q, row_kernel)
        return X
    return env(orc, logn, q, t), make_ctx


def check_add_plain(make_ctx, E, mem, B=3, seed=0):
    """e. hhe_add_plain per item, broadcast and subtracting, and the oracle's add_plain / sub_plain: only c0 changes, by the scaled
    plaintext; full vector"""
    X, O, t, n = make_ctx(), E.O, E.t, E.n
    rng = np.random.default_rng(seed)
    # the two coefficients at the rounding boundary: m Q mod t = (t - 1) / 2 is the smallest remainder that rounds up, (t - 3) / 2 the
    # largest that does not (a random m sits there with probability 1 / t)
    rho_inv = pow(E.Q % t, -1, t)
    edge = np.array([0, 1, (t - 1) // 2, (t + 1) // 2, t - 1, (t - 1) // 2 * rho_inv % t, (t - 3) // 2 * rho_inv % t], dtype=np.uint64)
    assert (int(edge[5]) * E.Q + (t + 1) // 2) % t == 0 and (int(edge[6]) * E.Q + (t + 1) // 2) % t == t - 1
    plains = rng.integers(0, t, (B, n), dtype=np.uint64)
    plains[0, :len(edge)], plains[1, n - len(edge):] = edge, edge
    plains[B - 1] = edge[rng.integers(0, len(edge), n)]
    cts = np.stack([E.encryption(seed + 20), E.uniform(rng, 2), E.maxed(2)][:B])
    want = {}
    for sub in (False, True):
        for b in range(B):
            for p in range(B):
                w = cts[b].copy()
                s = scaled_plain(E, plains[p])
                for j in range(E.L):
                    qj = np.uint64(E.q[j])
                    w[0, j] = (w[0, j] + (qj - s[j]) % qj) % qj if sub else (w[0, j] + s[j]) % qj
                want[(sub, b, p)] = w
    for b in range(B):
        assert (O.add_plain(cts[b], plains[b]) == want[(False, b, b)]).all(), ("oracle add_plain", b)
        assert (O.sub_plain(cts[b], plains[b]) == want[(True, b, b)]).all(), ("oracle sub_plain", b)
    d_cts, out = mem.to_dev(cts), mem.empty(cts.shape)
    for sub in (False, True):
        X.add_plain(d_cts, mem.to_dev(plains), out, B, subtract=sub)
        got = mem.to_host(out)
        for b in range(B):
            assert (got[b] == want[(sub, b, b)]).all(), ("product, per item, subtract =", sub, b)
        for p in range(B):
            X.add_plain(d_cts, mem.to_dev(plains[p:p + 1]), out, B, bcast=True, subtract=sub)
            got = mem.to_host(out)
            for b in range(B):
                assert (got[b] == want[(sub, b, p)]).all(), ("product, broadcast, subtract =", sub, b, p)
    X.close()


# ---- f. BEHZ multiply ----
def centred_lift(E, a):
    """[L][N] residues -> object array of the centred representatives mod Q"""
    coef = [(E.Q // qj) * pow(E.Q // qj, -1, qj) % E.Q for qj in E.q[:E.L]]
    acc = np.zeros(E.n, dtype=object)
    for j in range(E.L):
        acc = acc + a[j].astype(object) * coef[j]
    return np.array([v - E.Q if v > E.Q // 2 else v for v in (acc % E.Q)], dtype=object)


def behz_pairs(E, seed):
    """two encryptions; every word at q_j - 1 squared; q_j - 1 alternating with 0 against all q_j - 1; two pairs of uniform words;
    'half': every coefficient (Q - 1) / 2, squared -- the centred values of largest magnitude, where 'max' is the integer -1"""
    rng = np.random.default_rng(seed)
    return [(E.encryption(seed + 30), E.encryption(seed + 31)), (E.maxed(2), E.maxed(2)), (E.maxed(2, True), E.maxed(2)),
            (E.uniform(rng, 2), E.uniform(rng, 2)), (E.uniform(rng, 2), E.uniform(rng, 2)), (E.half(2), E.half(2))]


def behz_distance(E, a, b, out3, idx):
    """max over the three output polynomials and the coefficients idx of |centred(CRT(out) - floor((2 t d + Q) / (2 Q)) mod Q)|"""
    Q, t = E.Q, E.t
    al, bl = [centred_lift(E, a[k]) for k in range(2)], [centred_lift(E, b[k]) for k in range(2)]
    coef = [(Q // qj) * pow(Q // qj, -1, qj) % Q for qj in E.q[:E.L]]
    worst = 0
    for l in idx:
        d = [negacyclic_at(al[0], bl[0], l), negacyclic_at(al[0], bl[1], l) + negacyclic_at(al[1], bl[0], l), negacyclic_at(al[1], bl[1], l)]
        for k in range(3):
            x = sum(int(out3[k, j, l]) * coef[j] for j in range(E.L)) % Q
            e = (x - (2 * t * d[k] + Q) // (2 * Q)) % Q
            worst = max(worst, min(e, Q - e))
    return worst


def check_behz(make_ctx, E, mem, samples=28, seed=0):
    """f. hhe_multiply and the oracle's multiply within L + 1 of the rounded integer tensor product at 4 + `samples` coefficients.
    A defect of the kind this looks for moves the distance by about Q over a prime, so L + 1 is a condition and no tolerance.
    Returns the largest distance seen (oracle, product)."""
    X = make_ctx()
    pairs = behz_pairs(E, seed)
    idx = sample_indices(E.n, samples, seed + 4)
    worst = [0, 0]
    for s in range(0, len(pairs), 3):
        part = pairs[s:s + 3]
        o3 = mem.empty((len(part), 3, E.L, E.n))
        X.multiply(mem.to_dev(np.stack([a for a, _ in part])), mem.to_dev(np.stack([b for _, b in part])), o3, len(part))
        got = mem.to_host(o3)
        for i, (a, b) in enumerate(part):
            for w, (who, out3) in enumerate((("oracle", E.O.multiply(a, b)), ("product", got[i]))):
                dist = behz_distance(E, a, b, out3, idx)
                print("BEHZ distance, N = %d, L = %d, t = %d, pair %d, %s: %d" % (E.n, E.L, E.t, s + i, who, dist))
                worst[w] = max(worst[w], dist)
                assert dist <= E.L + 1, (who, "pair", s + i, "is", dist, "from the rounded integer product; the cap is L + 1 =", E.L + 1)
    X.close()
    return tuple(worst)
