"""Checker of hhe_multiply_sum and hhe_fc_packed_sum_ks, shared by the emulator suite (numpy memory) and the GPU suite (torch memory).

hhe_multiply_sum is no composition of the oracle's operations, so its truth is stated here: the BEHZ steps of SURVEY A.7 once more, in
Python integers, with the tensor step replaced by a sum (`restate`).  It shares no code with the product or with the oracle's multiply;
of the oracle it uses the forward and inverse transforms alone (held to their definition by definition_common.check_ntt), the point
products are Python integers.  test_mult_sum_emu holds the restatement to the oracle's multiply at K = 1 before it is used for K > 1.
A second truth that knows nothing of RNS: the distance of definition_common.behz_distance with the sum of the K integer products.
Every comparison of ciphertexts is exact equality of words."""
import numpy as np

import definition_common as dc
import fc_packed_common as fp

MT = 1 << 32
SAT = (1 << 63) - 1


def _prod(vs):
    p = 1
    for v in vs:
        p *= int(v)
    return p


# ---- the cap of include/hhe_gfx950.h ----
def sum_cap(n, q_data, bsk, t):
    """the largest K <= 2^63 - 1 with K N t Q (1 + rho)^2 / 2 + L < B (floor(m_sk / 2) - L), rho = (2L + 1) / 2^32, fractions cleared"""
    L = len(q_data)
    Q, B, msk = _prod(q_data), _prod(bsk[:L]), int(bsk[L])
    rhs = (1 << 65) * B * (msk // 2 - L)
    slack = (1 << 65) * L
    unit = int(n) * int(t) * Q * (MT + 2 * L + 1) ** 2
    if rhs <= slack:
        return 0
    return min((rhs - slack - 1) // unit, SAT)


def check_cap(X, E):
    want = sum_cap(E.n, E.q[:E.L], E.bsk, E.t)
    assert X.query("behz_sum_cap") == want, (X.query("behz_sum_cap"), want)
    return want


def hand_fold(primes):
    bits = max(int(p).bit_length() for p in primes)
    f = min(128, 1 << (127 - 2 * bits))
    assert 2 * f * (2 ** bits - 1) ** 2 + 2 ** bits < 1 << 128   # a residue and f addends of two products stay below 2^128
    return f


# ---- the restatement ----
class Restate:
    """constants of one parameter set, all Python integers"""

    def __init__(self, E):
        self.E = E
        self.qd = [int(v) for v in E.q[:E.L]]
        self.bsk = [int(v) for v in E.bsk]
        self.Q, self.B, self.msk = _prod(self.qd), _prod(self.bsk[:E.L]), self.bsk[E.L]
        self.Qhat = [self.Q // v for v in self.qd]
        self.Qhat_inv = [pow(h, -1, v) for h, v in zip(self.Qhat, self.qd)]
        self.Bhat = [self.B // v for v in self.bsk[:E.L]]
        self.Bhat_inv = [pow(h, -1, v) for h, v in zip(self.Bhat, self.bsk[:E.L])]
        # (modulus, index of the oracle's transform) of q u B_sk
        self.mods = [(v, j) for j, v in enumerate(self.qd)] + [(v, E.K + i) for i, v in enumerate(self.bsk)]

    def fastconv_q(self, xq, targets):
        """FastConv_{q -> targets}: xq [L] object arrays of residues"""
        w = [xq[l] * self.Qhat_inv[l] % self.qd[l] for l in range(len(self.qd))]
        return [sum(w[l] * (self.Qhat[l] % p) for l in range(len(self.qd))) % p for p in targets]

    def extend(self, x):
        """one polynomial [L][N] under q -> its residues under q u B_sk (fastbconv_m_tilde + sm_mrq), object arrays"""
        xq = [x[l].astype(object) for l in range(len(self.qd))]
        y = self.fastconv_q([xq[l] * MT % self.qd[l] for l in range(len(self.qd))], self.bsk + [MT])
        r = (-y[-1] * pow(self.Q, -1, MT)) % MT
        r = np.array([v - MT if v >= MT // 2 else v for v in r], dtype=object)
        return xq + [(y[i] + self.Q * r) * pow(MT, -1, p) % p for i, p in enumerate(self.bsk)]

    def representative(self, x):
        """one polynomial [L][N] -> object array of the integers sm_mrq leaves for it: the CRT over q u B_sk of extend(x), centred.
        It is congruent to x modulo Q and within (Q / 2)(1 + rho), rho = (2L + 1) / 2^32 -- the premise of the cap, asserted here --
        and it is the centred lift except where x is within L Q / 2^32 of -Q / 2, where it is the lift + Q"""
        L, mods = len(self.qd), self.qd + self.bsk
        M = self.Q * self.B * self.msk
        acc = np.zeros(self.E.n, dtype=object)
        for res, p in zip(self.extend(x), mods):
            acc = acc + res * ((M // p) * pow(M // p, -1, p) % M)
        rep = np.array([v - M if v > M // 2 else v for v in (acc % M)], dtype=object)
        assert all(abs(int(v)) * (1 << 33) <= self.Q * (MT + 2 * L + 1) for v in rep), "an operand leaves sm_mrq outside (Q / 2)(1 + rho)"
        return rep

    def transformed(self, ct):
        """a ciphertext [2][L][N] -> [2][2L + 1] transforms of its extended polynomials, object arrays"""
        O = self.E.O
        return [[O.ntt_fwd(mi, np.array(res, dtype=np.uint64)).astype(object) for res, (_, mi) in zip(self.extend(ct[k]), self.mods)]
                for k in range(2)]

    def floor_sk(self, d):
        """d [2L + 1] object arrays, the residues of t * (summed tensor polynomial) under q u B_sk -> [L][N] uint64"""
        L = len(self.qd)
        conv = self.fastconv_q(d[:L], self.bsk)
        f = [(d[L + i] - conv[i]) * pow(self.Q, -1, p) % p for i, p in enumerate(self.bsk)]
        u = [f[l] * self.Bhat_inv[l] % self.bsk[l] for l in range(L)]
        alpha = (sum(u[l] * (self.Bhat[l] % self.msk) for l in range(L)) - f[L]) * pow(self.B, -1, self.msk) % self.msk
        out = np.zeros((L, len(alpha)), np.uint64)
        for j, qj in enumerate(self.qd):
            v = sum(u[l] * (self.Bhat[l] % qj) for l in range(L))
            corr = np.array([-int(a) * self.B if a <= self.msk // 2 else (self.msk - int(a)) * self.B for a in alpha], dtype=object)
            out[j] = ((v + corr) % qj).astype(np.uint64)
        return out

    def multiply_sum(self, a, b):
        """a, b [K][2][L][N] -> [3][L][N]: the words hhe_multiply_sum must give for one item"""
        O, t = self.E.O, self.E.t
        ta, tb = self.cached(a), self.cached(b)
        out = np.zeros((3, len(self.qd), self.E.n), np.uint64)
        d = [[None] * len(self.mods) for _ in range(3)]
        for i, (p, mi) in enumerate(self.mods):
            s = [0, 0, 0]
            for x, y in zip(ta, tb):
                s[0] = s[0] + x[0][i] * y[0][i]
                s[1] = s[1] + x[0][i] * y[1][i] + x[1][i] * y[0][i]
                s[2] = s[2] + x[1][i] * y[1][i]
            for k in range(3):
                d[k][i] = O.ntt_inv(mi, np.array(s[k] % p, dtype=np.uint64)).astype(object) * t % p
        for k in range(3):
            out[k] = self.floor_sk(d[k])
        return out

    def multiply_sum_at(self, a, b, idx):
        """the same at the coefficients idx only, the negacyclic products by schoolbook (no transform): -> [3][L][len(idx)]"""
        t = self.E.t
        pairs = distinct_pairs(a, b, lambda ct: [self.extend(ct[k]) for k in range(2)])
        d = [[None] * len(self.mods) for _ in range(3)]
        for i, (p, _) in enumerate(self.mods):
            s = [[0] * len(idx) for _ in range(3)]
            for x, y, count in pairs:
                for c, l in enumerate(idx):
                    s[0][c] += count * dc.negacyclic_at(x[0][i], y[0][i], l)
                    s[1][c] += count * (dc.negacyclic_at(x[0][i], y[1][i], l) + dc.negacyclic_at(x[1][i], y[0][i], l))
                    s[2][c] += count * dc.negacyclic_at(x[1][i], y[1][i], l)
            for k in range(3):
                d[k][i] = np.array([v * t % p for v in s[k]], dtype=object)
        return np.stack([self.floor_sk(d[k]) for k in range(3)])

    def cached(self, cts):
        """the transforms of every ciphertext of cts, computed once per distinct buffer content"""
        memo, res = {}, []
        for ct in cts:
            key = ct.tobytes()
            if key not in memo:
                memo[key] = self.transformed(ct)
            res.append(memo[key])
        return res


def distinct_pairs(a, b, image):
    """[(image(a_k), image(b_k), how often the pair occurs)]: equal pairs of a sum are computed once, image once per distinct operand"""
    memo, count = {}, {}
    for x, y in zip(a, b):
        kx, ky = x.tobytes(), y.tobytes()
        for key, ct in ((kx, x), (ky, y)):
            if key not in memo:
                memo[key] = image(ct)
        count[(kx, ky)] = count.get((kx, ky), 0) + 1
    return [(memo[kx], memo[ky], c) for (kx, ky), c in count.items()]


def restate(E):
    return E.stored("mult_sum_restate", lambda: Restate(E))


def sum_distance(E, a, b, out3, idx, lift=None):
    """behz_distance for a sum: max over the three polynomials and the coefficients idx of the centred distance between CRT(out) and
    floor((2 t sum_k d_k + Q) / (2 Q)), d_k the integer tensor product of the centred lifts of pair k.  lift: another integer
    representative of a polynomial [L][N] than its centred lift (Restate.representative)"""
    Q, t = E.Q, E.t
    lift = lift or (lambda x: dc.centred_lift(E, x))
    pairs = distinct_pairs(a, b, lambda ct: [lift(ct[k]) for k in range(2)])
    coef = [(Q // qj) * pow(Q // qj, -1, qj) % Q for qj in E.q[:E.L]]
    worst = 0
    for l in idx:
        d = [0, 0, 0]
        for al, bl, count in pairs:
            d[0] += count * dc.negacyclic_at(al[0], bl[0], l)
            d[1] += count * (dc.negacyclic_at(al[0], bl[1], l) + dc.negacyclic_at(al[1], bl[0], l))
            d[2] += count * dc.negacyclic_at(al[1], bl[1], l)
        for k in range(3):
            x = sum(int(out3[k, j, l]) * coef[j] for j in range(E.L)) % Q
            e = (x - (2 * t * d[k] + Q) // (2 * Q)) % Q
            worst = max(worst, min(e, Q - e))
    return worst


# ---- inputs ----
def operands(E, K, B, pattern, seed):
    """(a, b) [K][B][2][L][N]: 'enc' real encryptions, 'max' every word q_j - 1, 'alt' q_j - 1 alternating with 0 against all q_j - 1,
    'rand' uniform words; 'half' every coefficient of every operand (Q - 1) / 2, the centred value of largest magnitude, 'half_neg' the
    same against (Q + 1) / 2 = -(Q - 1) / 2, 'half_mixed' K - 1 'half' pairs and a last pair of uniform words"""
    if pattern in ("half", "half_neg", "half_mixed"):
        h = E.half(2)
        a = np.broadcast_to(h, (K, B) + h.shape).copy()
        b_ = np.broadcast_to(E.half(2, True) if pattern == "half_neg" else h, (K, B) + h.shape).copy()
        if pattern == "half_mixed":
            rng = np.random.default_rng(seed)
            for item in range(B):
                a[K - 1, item], b_[K - 1, item] = E.uniform(rng, 2), E.uniform(rng, 2)
        return a, b_
    if pattern == "enc":
        pool = [E.encryption(seed + i) for i in range(4)]
        a = np.stack([np.stack([pool[(k + b) % 4] for b in range(B)]) for k in range(K)])
        b_ = np.stack([np.stack([pool[(k + 2 * b + 1) % 4] for b in range(B)]) for k in range(K)])
        return a, b_
    if pattern == "max":
        m = E.maxed(2)
        return np.broadcast_to(m, (K, B) + m.shape).copy(), np.broadcast_to(m, (K, B) + m.shape).copy()
    if pattern == "alt":
        m, alt = E.maxed(2), E.maxed(2, True)
        return np.broadcast_to(alt, (K, B) + m.shape).copy(), np.broadcast_to(m, (K, B) + m.shape).copy()
    rng = np.random.default_rng(seed)
    pool = [E.uniform(rng, 2) for _ in range(6)]
    a = np.stack([np.stack([pool[(k + b) % 6] for b in range(B)]) for k in range(K)])
    b_ = np.stack([np.stack([pool[(2 * k + b + 3) % 6] for b in range(B)]) for k in range(K)])
    return a, b_


def run(X, mem, a, b, bcast=False):
    """hhe_multiply_sum on a [K][B][..], b [K][B or 1][..]; asserts one launch per modulus set"""
    K, B = a.shape[:2]
    out = mem.empty((B, 3) + a.shape[3:])
    before = X.query("multiply_sum_launches")
    X.multiply_sum(mem.to_dev(a), mem.to_dev(b), K, out, B, b_bcast=bcast)
    X.sync()
    assert X.query("multiply_sum_launches") == before + 2, "one launch of the sum kernel per modulus set"
    return mem.to_host(out)


def check_words(X, E, mem, K, B, pattern, seed=0, samples=6):
    """the device's words against the restatement (every word) and the distance at sampled coefficients; returns the worst distance"""
    a, b = operands(E, K, B, pattern, seed)
    got = run(X, mem, a, b)
    R = restate(E)
    idx = dc.sample_indices(E.n, samples, seed + 4)
    worst = 0
    for item in range(B):
        want = R.multiply_sum(a[:, item], b[:, item])
        assert (got[item] == want).all(), ("hhe_multiply_sum differs from the restatement", K, B, pattern, item)
        dist = sum_distance(E, a[:, item], b[:, item], got[item], idx)
        print("summed BEHZ distance, N = %d, L = %d, K = %d, %s, item %d: %d" % (E.n, E.L, K, pattern, item, dist))
        assert dist <= E.L + 1, ("the sum of", K, "products is", dist, "from the rounded integer sum; the cap is L + 1 =", E.L + 1)
        worst = max(worst, dist)
    return worst


# ---- the layer ----
def fc_packed_sum_ref(X, mem, O, rk, gk, W, x, rows, cols, hoisted):
    """the layer on one ciphertext: the oracle's rotate_rows, add and relinearize around the public hhe_multiply_sum of X"""
    n = O.n
    r, c = fp.hand_shape(n, rows, cols)
    x = np.array(x, dtype=np.uint64, copy=True)
    if 2 * c != n:
        x = O.add(x, O.rotate_rows(x, -c, gk)[0])
    rot = [x]
    for i in range(1, r):
        rot.append(O.rotate_rows(x if hoisted else rot[i - 1], i if hoisted else 1, gk)[0])
    out3 = mem.empty((1, 3) + tuple(O.ct_shape[1:]))
    X.multiply_sum(mem.to_dev(np.stack(rot)[:, None]), mem.to_dev(np.asarray(W)[:, None]), r, out3, 1)
    X.sync()
    y = O.relinearize(mem.to_host(out3)[0], rk)
    s = r
    while s < c:
        y = O.add(y, O.rotate_rows(y, s, gk)[0])
        s *= 2
    return y


def check_sum_layer(X, S, mem, M, hoisted, B=2, seed=0, in_place=False, rk=None, gk=None, refs=None, O=None, keys=None, data=None, XR=None):
    """hhe_fc_packed_sum_ks against the composition around hhe_multiply_sum and against (M x) mod t; the counters; the per-product
    forms on the same handle before and after.  data: (W, cts, xs) already at the context's level; XR: the context the reference's
    hhe_multiply_sum runs on (default X).  Returns (device words, references)"""
    rows, cols = M.shape
    O = O or S.O
    ork, ogk = keys or (S.rk, S.gk)
    if data is None:
        rng = np.random.default_rng(2000 + seed)
        xs = [rng.integers(0, S.t, size=cols, dtype=np.uint64) for _ in range(B)]
        W = fp.encrypt_diagonals(S, M, seed=300 + 16 * seed)
        cts = fp.encrypt_inputs(S, xs, seed=100 + 16 * seed)
    else:
        W, cts, xs = data
    r, _ = fp.hand_shape(S.n, rows, cols)
    shape = (B,) + tuple(O.ct_shape)
    mat = X.enc_matrix(mem.to_dev(W), rows, cols)
    try:
        d_in = mem.to_dev(cts)
        forms = (mat.apply_hoisted, mat.apply) if hoisted else (mat.apply, mat.apply_hoisted)
        before = [mem.to_host(f(d_in, B, rk=rk, gk=gk, out=mem.empty(shape))) for f in forms]
        assert X.query("fc_packed_floors") == 3 * r
        adds = X.query("add_many_launches")
        d_work = mem.to_dev(cts) if in_place else d_in
        d_out = d_work if in_place else mem.empty(shape)
        got = mem.to_host(mat.apply_sum(d_work, B, rk=rk, gk=gk, out=None if in_place else d_out, hoisted=hoisted))
        assert X.query("fc_packed_floors") == 3
        assert X.query("add_many_launches") == adds, "the sum kernel of hhe_add_many ran"
        after = [mem.to_host(f(d_in, B, rk=rk, gk=gk, out=mem.empty(shape))) for f in forms]
        for x, y in zip(before, after):
            assert (x == y).all(), "a per-product form changed its words after a sum call on the same handle"
    finally:
        mat.destroy()
    if refs is None:
        refs = [fc_packed_sum_ref(XR or X, mem, O, ork, ogk, W, cts[b], rows, cols, hoisted) for b in range(B)]
    for b in range(B):
        assert (got[b] == refs[b]).all(), ("fc_packed_sum differs from the composition around hhe_multiply_sum", b, rows, cols, hoisted)
    return got, refs, xs


def check_sum_slots(S, got, M, xs):
    for b in range(len(xs)):
        fp.check_slots(S, got[b], M, xs[b], what=(M.shape, b))
