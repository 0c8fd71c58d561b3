"""Integer definitions of the plaintext boundary, shared by the emulator suite (test_codec_emu.py, numpy memory) and the GPU suite
(test_gpu_codec.py, torch memory): definitions g and h of the list that definition_common.py begins.

hhe_encode, the decode half of hhe_decrypt and the scale-and-round of hhe_decrypt / hhe_decrypt_level were compared with the oracle's
encode, decode and decrypt only, on phases that an encryption produces.  This module states them once more in Python integers:

  g. Slots.  psi_t = the minimal primitive 2N-th root of unity modulo t;  e_i = 3^i mod 2N for i < N/2,  e_{N/2+i} = 2N - e_i.
       decode(p)[i] = p(psi_t^(e_i)) mod t
       encode(v, count) = the one p of degree < N with p(psi_t^(e_i)) = v[i] for i < count and 0 at every other slot.
     A one-hot value v at slot i0 encodes to p_k = v N^-1 zeta^-k mod t with zeta = psi_t^(e_i0): the N evaluation points are the
     roots of X^N + 1, two of them differ by an N-th root of unity, so sum_k (zeta' / zeta)^k is N at zeta' = zeta and 0 elsewhere.

  h. decrypt (RNSTool::decrypt_scale_and_round with its RNS removed).  For a coefficient whose phase has the CRT representative x in
     [0, Q), Q = q_0 ... q_{l-1} for the limb count l of the call, gamma = the second-largest prime of 61 bits that is 1 mod 2N:
       v_j = x t gamma (Q / q_j)^-1 mod q_j
       alpha = floor(sum_j v_j (Q / q_j) / Q)        the overshoot of the fast base conversion, 0 <= alpha < l;
                                                      sum_j v_j (Q / q_j) == (t gamma x mod Q) + alpha Q is asserted
       w = floor(t gamma x / Q) - alpha
       m = floor((2 w + gamma) / (2 gamma)) mod t    the nearest integer to w / gamma; gamma is odd, there is no tie
     m is the exact floor((2 t x + Q) / (2 Q)) mod t unless 0 <= (t x mod Q) - Q / 2 < l Q / gamma (asserted for every coefficient a
     check uses, before any product runs).  Outside that one-sided window decryption is exact rounding; inside it the library follows
     SEAL, alpha and all.

No expected value comes from a transform, a CRT, a rounding, an encode, a decode or a decrypt of the oracle or of the product.  Phases
are CHOSEN: the secret key is this file's s = X^a - X^b + X^c, its NTT words closed-form from the tables of powers, c1 is uniform and
c0 = target - c1 * s by shifts, so a coefficient sits exactly where the walk puts it -- on both sides of every rounding boundary, on
both sides of the window, and on the two values of w mod gamma that decide `vg > (gamma >> 1)`.  The oracle and the product are both
parties under test; an assertion names the one that differs.

hhe_encode takes slot values below t (include/hhe_gfx950.h states no behaviour for larger words), so no word >= t is encoded here."""
import random

import numpy as np

import definition_common as dc
from mod_switch_common import crt

MARK = 0xABCDEF0123456789   # what an output buffer holds before a call: every word of it has to be written


# ---- gamma ----
def is_prime(v):
    """Miller-Rabin with the first twelve primes as bases: exact below 3.3 * 10^24"""
    if v < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in small:
        if v % p == 0:
            return v == p
    d, r = v - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in small:
        y = pow(a, d, v)
        if y in (1, v - 1):
            continue
        for _ in range(r - 1):
            y = y * y % v
            if y == v - 1:
                break
        else:
            return False
    return True


def gamma_of(n):
    """the second prime below 2^61 that is 1 mod 2N, counted from the top (the first is the BEHZ m_sk)"""
    v, found = (1 << 61) - 2 * n + 1, 0
    while True:
        if is_prime(v):
            found += 1
            if found == 2:
                return v
        v -= 2 * n


# ---- g. slots ----
def slot_exponents(n):
    e, pos = [0] * n, 1
    for i in range(n // 2):
        e[i], e[n // 2 + i] = pos, 2 * n - pos
        pos = pos * 3 % (2 * n)
    return e


def t_table(E):
    """(psi_t, its 2N powers as Python integers, the same as uint64)"""
    return E.table(len(E.mods) - 1)


def horner(coeffs, z, t):
    """sum_k coeffs[k] z^k mod t"""
    acc = 0
    for v in reversed(coeffs):
        acc = (acc * z + v) % t
    return acc


def slot_values(E, coeffs, slots):
    """decode(coeffs) at the given slots, by Horner at psi_t^(e_i)"""
    P, e = t_table(E)[1], slot_exponents(E.n)
    c = [int(v) for v in coeffs]
    return [horner(c, P[e[i]], E.t) for i in slots]


def sample_slots(n, count, seed):
    """0, 1, N/2 - 1, N/2, N - 1 and `count` seeded ones"""
    rng = np.random.default_rng(seed)
    return [0, 1, n // 2 - 1, n // 2, n - 1] + [int(v) for v in rng.integers(2, n - 1, count)]


def one_hot_plain(E, hot):
    """encode of the slot vector that is v at slot s for (s, v) in hot and 0 elsewhere, full vector: sum v N^-1 zeta_s^-k"""
    n, t = E.n, E.t
    P, e, ninv = t_table(E)[1], slot_exponents(n), pow(n, -1, t)
    out = [0] * n
    for s, v in hot:
        c = v * ninv % t
        for k in range(n):
            out[k] = (out[k] + c * P[(-e[s] * k) % (2 * n)]) % t
    return np.array(out, dtype=np.uint64)


def monomial_slots(E, terms):
    """decode(sum_r c_r X^(d_r)), all N slots: sum_r c_r psi_t^(e_i d_r mod 2N), the powers read from the table"""
    n, t = E.n, E.t
    _, P, Pu = t_table(E)
    e = np.array(slot_exponents(n), dtype=np.int64)
    acc = np.zeros(n, np.uint64)
    for c, d in terms:
        c = int(c) % t
        tab = Pu if c == 1 else np.uint64(t) - Pu if c == t - 1 else np.array([c * x % t for x in P], dtype=np.uint64)
        acc = (acc + tab[(e * d) % (2 * n)]) % np.uint64(t)   # two residues below 2^61: no wrap
    return acc


def marked(mem, shape):
    return mem.to_dev(np.full(shape, MARK, dtype=np.uint64))


def check_encode(make_ctx, E, mem, seed=0):
    """1. hhe_encode and the oracle's encode against g with 1, N/2, N/2 + 1 and N values per item, three items per call.  Item 0: up
    to three one-hot slots (0, N/2 - 1 and one of the second row: those below count) with the values t - 1, 1 and (t + 1) / 2, the
    full coefficient vector against the closed form.  Items 1 and 2: uniform values, row 0 of item 1 all t - 1; the party's
    coefficients evaluated by Horner at the slots 0, 1, N/2 - 1, N/2, N - 1, count - 1, count (the first slot that must be 0) and 12
    seeded ones."""
    X, O, n, t = make_ctx(), E.O, E.n, E.t
    for count in (1, n // 2, n // 2 + 1, n):
        rng = np.random.default_rng(seed + count)
        vals = rng.integers(0, t, (3, count), dtype=np.uint64)
        second = n // 2 if count == n // 2 + 1 else n // 2 + 37
        hot = [(s, v) for s, v in ((0, t - 1), (n // 2 - 1, 1), (second, (t + 1) // 2)) if s < count]
        assert len(hot) == {1: 1, n // 2: 2}.get(count, 3)
        vals[0] = 0
        for s, v in hot:
            vals[0, s] = v
        vals[1, :min(count, n // 2)] = t - 1
        want0 = one_hot_plain(E, hot)
        slots = sorted(set(sample_slots(n, 12, seed + 1) + [count - 1] + ([count] if count < n else [])))
        want = [[int(vals[b, i]) if i < count else 0 for i in slots] for b in range(3)]
        d_pl = marked(mem, (3, n))
        X.encode(mem.to_dev(vals), 3, count, d_pl)
        for who, got in (("oracle", np.stack([O.encode(vals[b]) for b in range(3)])), ("product", mem.to_host(d_pl))):
            assert (got < np.uint64(t)).all(), (who, "count", count, "a coefficient is not below t")
            bad = np.flatnonzero(got[0] != want0)
            assert bad.size == 0, (who, "count", count, "one-hot slots", hot, "differ from v N^-1 zeta^-k at coefficients", bad[:4].tolist())
            for b in (1, 2):
                have = slot_values(E, got[b], slots)
                bad = [(i, h, w) for i, h, w in zip(slots, have, want[b]) if h != w]
                assert not bad, (who, "count", count, "item", b, "p(psi^(e_i)) != v[i] at (slot, p(..), v):", bad[:4])
    X.close()


# ---- the test's own key and chosen phases ----
class SparseSecret:
    """s = X^a - X^b + X^c with b = N - 1 and seeded a < c: words() is its NTT form under every prime of E, limb by limb from the power
    tables (definition b); times() multiplies residues by it with three signed shifts"""

    def __init__(self, n, seed):
        rnd = random.Random(seed)
        self.a, self.c = sorted(rnd.sample(range(1, n - 1), 2))
        self.b = n - 1

    def words(self, E):
        return np.stack([dc.monomial_image(E, J, [(1, self.a), (E.q[J] - 1, self.b), (1, self.c)]) for J in range(E.K)])

    def times(self, c1, q):
        """c1 [.., l, N] under q[:l] -> c1 * s in Z_q[X] / (X^N + 1), the same shape"""
        out = np.zeros_like(c1)
        for j in range(c1.shape[-2]):
            qj = np.uint64(q[j])
            acc = shift_mod(c1[..., j, :], self.a, qj)
            acc = (acc + (qj - shift_mod(c1[..., j, :], self.b, qj)) % qj) % qj
            out[..., j, :] = (acc + shift_mod(c1[..., j, :], self.c, qj)) % qj
        return out


def shift_mod(a, e, qj):
    """a X^e in Z_q[X] / (X^N + 1) on residues [.., N]: the top e coefficients come round negated"""
    n = a.shape[-1]
    out = np.empty_like(a)
    out[..., e:] = a[..., :n - e]
    out[..., :e] = (qj - a[..., n - e:]) % qj
    return out


def residues(x, q):
    """object array [.., N] of integers -> words [.., l, N] under q"""
    return np.stack([(x % int(qj)).astype(np.uint64) for qj in q], axis=-2)


def ciphertexts(E, key, target, seed):
    """[B][2][l][N]: uniform c1 and c0 = target - c1 * s, so that the phase c0 + c1 s IS target [B][l][N], whatever c1 is"""
    rng = np.random.default_rng(seed)
    q = E.q[:E.L]
    c1 = np.stack([rng.integers(0, qj, (target.shape[0], E.n), dtype=np.uint64) for qj in q], axis=1)
    c1s = key.times(c1, q)
    c0 = np.zeros_like(c1)
    for j, qj in enumerate(q):
        c0[:, j] = (target[:, j] + (np.uint64(qj) - c1s[:, j]) % np.uint64(qj)) % np.uint64(qj)
    ct = np.stack([c0, c1], axis=1)
    x = crt(ct[:, 0], q) + crt(c1s, q)      # the construction, read back: c0 + c1 s is the target as an integer mod Q
    assert (x % E.Q == crt(target, q)).all()
    return ct


def decryptions(E, sk, mem, cts, products):
    """[(who, coefficients [B][N] or None, slots [B][N])]: the oracle's decrypt and decode of every item, and each product call
    (name, f(ct_dev, B, vals_dev)) on the batch, its output buffer marked beforehand"""
    B = cts.shape[0]
    coeffs = np.stack([E.O.decrypt(sk, cts[b]) for b in range(B)])
    out = [("oracle", coeffs, np.stack([E.O.decode(coeffs[b]) for b in range(B)]))]
    for who, f in products:
        d_vals = marked(mem, (B, E.n))
        f(mem.to_dev(cts), B, d_vals)
        out.append((who, None, mem.to_host(d_vals)))
    return out


def plain_monomials(E, b, seed):
    """item b's plaintext: the coefficients 1, t - 1 and a seeded one at the exponents 0, N - 1 and a seeded one, the pairing
    rotating with the item"""
    rnd = random.Random(1000 * seed + b)
    cs, ds = [1, E.t - 1, rnd.randrange(2, E.t - 1)], [0, E.n - 1, rnd.randrange(1, E.n - 1)]
    return [(cs[(r + b) % 3], ds[r]) for r in range(3)]


def slots_body(E, key, sk, mem, products, B, seed):
    """2. on one limb set: phase = floor((m Q + (t + 1) / 2) / t) of three monomials m, different per item; every party's N slots
    against m(psi_t^(e_i)), and the oracle's coefficients against m"""
    n, t, Q = E.n, E.t, E.Q
    terms = [plain_monomials(E, b, seed) for b in range(B)]
    m = np.zeros((B, n), dtype=object)
    for b in range(B):
        for c, d in terms[b]:
            m[b, d] = c
    want = np.stack([monomial_slots(E, terms[b]) for b in range(B)])
    cts = ciphertexts(E, key, residues((m * Q + (t + 1) // 2) // t, E.q[:E.L]), seed + 1)
    for who, coeffs, slots in decryptions(E, sk, mem, cts, products):
        for b in range(B):
            if coeffs is not None:
                bad = [i for i in range(n) if int(coeffs[b, i]) != m[b, i]]
                assert not bad, (who, "limbs", E.L, "item", b, "the scaled plaintext does not decrypt to itself at coefficients", bad[:4])
            bad = np.flatnonzero(slots[b] != want[b])
            assert bad.size == 0, (who, "limbs", E.L, "item", b, "slot i is not m(psi^(e_i)); first slots:", bad[:4].tolist())


# ---- h. decrypt ----
class Scale:
    """definition h over the data primes q: Python integers only"""

    def __init__(self, q, t, gamma):
        self.q, self.t, self.gamma, self.l = [int(v) for v in q], int(t), int(gamma), len(q)
        self.Q = 1
        for v in self.q:
            self.Q *= v
        self.tg = self.t * self.gamma
        self.punct = [self.Q // v for v in self.q]
        self.cj = [self.tg * pow(M, -1, v) % v for M, v in zip(self.punct, self.q)]

    def w(self, x):
        s = sum((x % qj) * cj % qj * M for qj, cj, M in zip(self.q, self.cj, self.punct))
        alpha, rest = divmod(s - self.tg * x % self.Q, self.Q)
        assert rest == 0 and 0 <= alpha < self.l, "the fast base conversion is t gamma x mod Q plus alpha Q with 0 <= alpha < l"
        return self.tg * x // self.Q - alpha

    def m(self, x):
        return (2 * self.w(x) + self.gamma) // (2 * self.gamma) % self.t

    def exact(self, x):
        return (2 * self.t * x + self.Q) // (2 * self.Q) % self.t

    def in_window(self, x):
        """0 <= (t x mod Q) - Q / 2 < l Q / gamma, in integers"""
        d = 2 * (self.t * x % self.Q) - self.Q
        return 0 <= d and d * self.gamma < 2 * self.l * self.Q

    def has_window(self):
        return self.l * self.Q >= self.t * self.gamma     # l Q / gamma >= t: the window holds an x for every m

    def fine(self):
        return self.Q > 2 * self.tg                       # floor(t gamma x / Q) takes every integer as x runs

    def with_residue(self, rho, k):
        """an x with w mod gamma == rho exactly: floor(t gamma x / Q) = k gamma + rho + a for the a that alpha then takes back, tried
        from the likeliest a (alpha is about a sum of l uniform fractions) over the x that share that floor"""
        assert self.fine()
        per = self.Q // self.tg      # that many consecutive x share a floor, or one more
        for a in sorted(range(self.l), key=lambda a: abs(2 * a + 1 - self.l)):
            first = -(-(k * self.gamma + rho + a) * self.Q // self.tg)
            for x in range(first, first + min(per, 64)):
                if self.w(x) % self.gamma == rho:
                    return x
        raise AssertionError("no x with w mod gamma == %d near m = %d" % (rho, k))


def walk_of(S, seed, limit=None):
    """the x of the walk: 0, 1, Q - 1, floor(Q / 2), floor(Q / 2) + 1; for m in {0, 1, 2, floor(t / 2), t - 2, t - 1} the first x that
    exact rounding takes to m + 1, c = ceil((m + 1/2) Q / t), with the offsets -2 .. 2 and +-W, +-W/2, +-W/3 for W = floor((l + 2) Q /
    (gamma t)) + 2, a little more than the window; where Q > 2 t gamma two x whose w mod gamma is exactly (gamma - 1) / 2 and
    (gamma + 1) / 2.  limit: the two searched x and a seeded choice of the others, `limit` in all."""
    Q, t, g, l = S.Q, S.t, S.gamma, S.l
    pts = [0, 1, Q - 1, Q // 2, Q // 2 + 1]
    cs = [-(-(2 * m + 1) * Q // (2 * t)) for m in (0, 1, 2, t // 2, t - 2, t - 1)]
    for c in cs:
        pts += [(c + o) % Q for o in (-2, -1, 0, 1, 2)]
    W = (l + 2) * Q // (g * t) + 2
    for c in cs:
        pts += [(c + o) % Q for o in (W, -W, W // 2, -(W // 2), W // 3, -(W // 3))]
    searched = [S.with_residue(rho, t // 3 + i) for i, rho in enumerate(((g - 1) // 2, (g + 1) // 2))] if S.fine() else []
    if limit is not None:
        pts = random.Random(seed).sample(pts, limit - len(searched))
    return pts + searched


def rounding_inputs(S, n, B, seed, limit=None):
    """x [B][N] as integers: item 0 the walk -- dense at the front, or, with `limit`, that many of its points at seeded coefficients
    -- among seeded uniform x; further items uniform"""
    rnd = random.Random(seed)
    x = np.array([[rnd.randrange(S.Q) for _ in range(n)] for _ in range(B)], dtype=object)
    walk = walk_of(S, seed, limit)
    at = range(len(walk)) if limit is None else sorted(rnd.sample(range(n), len(walk)))
    for i, v in zip(at, walk):
        x[0, i] = v
    return x, list(at)


def rounding_body(E, key, sk, mem, products, gamma, B, seed, samples=16, limit=None):
    """3. on one limb set: every party's decryption of chosen x against h -- the oracle's coefficients all of them, everybody's slots
    at 5 + `samples` places, each of which is a linear form with invertible weights in every coefficient.  Returns (coefficients of
    item 0 inside the window, coefficients of item 0 where h differs from exact rounding)."""
    n = E.n
    S = Scale(E.q[:E.L], E.t, gamma)
    assert S.Q == E.Q
    x, at = rounding_inputs(S, n, B, seed, limit)
    want = np.array([[S.m(int(v)) for v in item] for item in x], dtype=object)
    # properties of the definition, before anybody is called
    inside = [{i for i in range(n) if S.in_window(int(item[i]))} for item in x]
    for b in range(B):
        off = [i for i in range(n) if i not in inside[b] and want[b, i] != S.exact(int(x[b, i]))]
        assert not off, ("definition h leaves exact rounding outside its window, item", b, "coefficients", off[:4])
    differs = [i for i in sorted(inside[0]) if want[0, i] != S.exact(int(x[0, i]))]
    print("decrypt walk: N = %d, l = %d, t = %d: %d coefficients in the window, %d off exact rounding"
          % (n, S.l, S.t, len(inside[0]), len(differs)))
    if S.has_window():
        assert len(inside[0] & set(at)) >= 12, ("the walk has too few x inside the window", len(inside[0]))
    if S.fine():
        assert differs, "no coefficient of the walk tells h from exact rounding"
        have = {S.w(int(x[0, i])) % gamma for i in at}
        assert {(gamma - 1) // 2, (gamma + 1) // 2} <= have, "the two sides of vg > (gamma >> 1) are not in the walk"
    slots = sample_slots(n, samples, seed + 2)
    want_slots = [slot_values(E, want[b], slots) for b in range(B)]
    cts = ciphertexts(E, key, residues(x, E.q[:E.L]), seed + 3)
    for who, coeffs, vals in decryptions(E, sk, mem, cts, products):
        for b in range(B):
            if coeffs is not None:
                bad = [i for i in range(n) if int(coeffs[b, i]) != want[b, i]]
                assert not bad, (who, "limbs", S.l, "item", b, "differs from definition h at coefficients", bad[:6],
                                 "of them in the window:", [i for i in bad if i in inside[b]][:6])
            bad = [(i, int(vals[b, i]), w) for i, w in zip(slots, want_slots[b]) if int(vals[b, i]) != w]
            assert not bad, (who, "limbs", S.l, "item", b, "slots differ from definition h evaluated by g at (slot, got, want):", bad[:3])
    return len(inside[0]), len(differs)


def gamma_checked(E, X):
    g = gamma_of(E.n)
    assert g not in E.q and g % (2 * E.n) == 1
    assert E.O.query("gamma") == g, ("oracle", "gamma is not the second 61-bit prime that is 1 mod 2N")
    assert X.query("gamma") == g, ("product", "gamma is not the second 61-bit prime that is 1 mod 2N")
    return g


def check_decrypt_slots(make_ctx, E, mem, B=3, seed=0):
    """2. hhe_decrypt and the oracle's decrypt + decode on B chosen phases under this file's key: the slot order, the c1 s path and
    both item strides, with values the test chose"""
    X = make_ctx()
    key = SparseSecret(E.n, seed)
    sk = key.words(E)
    slots_body(E, key, sk, mem, [("product", lambda d, nb, o: X.decrypt(sk, d, nb, o))], B, seed)
    X.close()


def check_decrypt_rounding(make_ctx, E, mem, B=2, seed=0, samples=16, limit=None):
    """3. hhe_decrypt and the oracle's decrypt on the walk of x (item 0) and on uniform x (item 1)"""
    X = make_ctx()
    key = SparseSecret(E.n, seed)
    sk = key.words(E)
    got = rounding_body(E, key, sk, mem, [("product", lambda d, nb, o: X.decrypt(sk, d, nb, o))], gamma_checked(E, X), B, seed, samples, limit)
    X.close()
    return got


def check_decrypt_levels(make_ctx, E, orc, mem, seed=0):
    """4. checks 2 and 3 at every limb count l = 1 .. L of one context: through hhe_decrypt_level with the context's key [K][N], and
    through hhe_decrypt on the context hhe_ctx_create_level makes for l, with the rows {0 .. l-1, K-1} of that key.  The definition is
    the one of Q = q_0 ... q_{l-1}; the oracle is the one of the context over q_0 .. q_{l-1} and the special prime.  Returns the
    window counts of check 3 per level."""
    X = make_ctx()
    key = SparseSecret(E.n, seed)
    sk = key.words(E)
    gamma = gamma_checked(E, X)
    counts = {}
    for l in range(1, E.L + 1):
        El = E if l == E.L else dc.env(orc, E.logn, E.q[:l] + [E.q[-1]], E.t)
        skl = np.ascontiguousarray(sk[list(range(l)) + [E.K - 1]])
        Xl = X.at_level(l)
        assert (Xl.L, Xl.query("gamma"), El.O.query("gamma")) == (l, gamma, gamma)
        products = [("product, hhe_decrypt_level", lambda d, nb, o, l=l: X.decrypt_level(sk, d, l, nb, o)),
                    ("product, hhe_decrypt on the level context", lambda d, nb, o, Xl=Xl, skl=skl: Xl.decrypt(skl, d, nb, o))]
        slots_body(El, key, skl, mem, products, 3, seed + l)
        counts[l] = rounding_body(El, key, skl, mem, products, gamma, 2, seed + l)
        Xl.close()
    X.close()
    return counts
