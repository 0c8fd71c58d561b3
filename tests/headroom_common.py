"""hhe_multiply_sum AT its cap, and the contexts whose cap is 0.  Shared by the emulator suite (numpy memory) and the GPU suite (torch
memory).

behz_sum_cap is a proved limit (include/hhe_gfx950.h).  Every other context of the suites has a cap far above any
K they run, and no other operand pattern puts centred values near +-Q / 2, so neither the formula nor the kernels at the cap are held
to anything there.  Here t = 1096486890805657601 over primes chosen so that the cap is small, and the operands are 'half': every
coefficient of both polynomials of every operand is (Q - 1) / 2.  With them the bound is tight: at K = cap the restatement of
mult_sum_common is within L + 1 of the rounded integer sum, at K = cap + 1 it is about Q over a prime away (check_tightness).

Two distances are taken at K = cap.  The one of mult_sum_common.sum_distance, with the centred lifts of the operands, for 'half' and
'half_mixed'.  And, for every pattern, the one DESIGN.md section 4 proves: with the representatives sm_mrq leaves
(Restate.representative).  The two lifts agree except on a coefficient within L Q / 2^32 of -Q / 2, and 'half_neg' (the second operand
(Q + 1) / 2 = -(Q - 1) / 2) is made of such coefficients: where sm_mrq leaves (Q + 1) / 2 itself, the result differs from the one of the
centred lifts by a multiple of t -- the same ciphertext, K N t away as an integer (measured: 8192 t + 1 at 3 x 55 bits), and that is
what the oracle's multiply gives too.  So 'half_neg' is held to the words of the restatement and to the distance with the
representatives, and its distance with the centred lifts is printed, not asserted.
Every comparison of ciphertexts is exact equality of words; L + 1 is the project's condition and no tolerance."""
import numpy as np
import pytest

import definition_common as dc
import fc_packed_common as fp
import mlp_common as mc
import mult_sum_common as ms
import plain_modulus_common as pm
import rot_many_common as rmc

T60 = pm.T60
# name: (logn, bit sizes of the primes (the last one is the special prime), behz_sum_cap)
CONTEXTS = {
    "50x2": (10, [50, 50], 4),
    "55x3": (10, [55] * 3, 8),
    "57x4": (10, [57] * 4, 8),
    "58x5": (10, [58] * 5, 8),
    "54x3": (10, [54] * 3, 33),       # cap == multiply_sum_fold_bsk + 1: K = cap crosses a fold of the 128-bit sums
    "53_54_54": (10, [53, 54, 54], 67),
    "n4096_55x3": (12, [55] * 3, 2),
}
AT_THE_CAP = ("half", "half_neg", "half_mixed")
# bit sizes of the contexts at N = 1024 whose cap is 0
ZERO = {"60x2": [60] * 2, "60x5": [60] * 5}
SEED = 7


def context(orc, name):
    """(Env, the cap the issue pins) of a context; primes_near gave the sizes asked for"""
    logn, bits, cap = CONTEXTS[name]
    q = pm.primes_near(orc, 1 << logn, bits)
    assert [int(p).bit_length() for p in q] == bits, (name, q)
    return dc.env(orc, logn, q, T60), cap


def coefficients(n, seed=SEED):
    """0, 1, N / 2, N - 2, N - 1 and four seeded ones"""
    return [0, 1, n // 2, n - 2, n - 1] + [int(v) for v in np.random.default_rng(seed).integers(2, n - 2, 4)]


def check_cap(X, E, cap):
    """the context's query, the header's condition in Python integers and the literal are one number"""
    assert X.query("behz_sum_cap") == ms.sum_cap(E.n, E.q[:E.L], E.bsk, E.t) == cap, (X.query("behz_sum_cap"), cap)


def truth(E, K, pattern):
    """(a, b [K][2][L][N], the restatement's words [3][L][N]) of one item, computed once per context"""
    def make():
        a, b = ms.operands(E, K, 1, pattern, SEED)
        return a[:, 0], b[:, 0], ms.restate(E).multiply_sum(a[:, 0], b[:, 0])
    return E.stored(("headroom", K, pattern), make)


def check_item(E, a, b, got, want, what, centred=True):
    """one item's words against the restatement, its distances at coefficients(); returns the larger distance asserted"""
    assert (got == want).all(), ("hhe_multiply_sum differs from the restatement at the cap", what)
    idx = coefficients(E.n)
    dist = ms.sum_distance(E, a, b, got, idx, lift=ms.restate(E).representative)
    print("summed BEHZ distance at the cap, N = %d, L = %d, K = %d, %s: %d with the representatives of sm_mrq" % (E.n, E.L, len(a), what, dist))
    assert dist <= E.L + 1, (what, "is", dist, "from the rounded integer sum of the representatives; the cap is L + 1 =", E.L + 1)
    lifted = ms.sum_distance(E, a, b, got, idx)
    print("    %d with the centred lifts" % lifted)
    if centred:
        assert lifted <= E.L + 1, (what, "is", lifted, "from the rounded integer sum; the cap is L + 1 =", E.L + 1)
        dist = max(dist, lifted)
    return dist


def check_at_the_cap(X, E, mem, cap, pattern):
    """K = cap, B = 1: every word, both distances"""
    a, b, want = truth(E, cap, pattern)
    got = ms.run(X, mem, a[:, None], b[:, None])
    return check_item(E, a, b, got[0], want, pattern, centred=pattern != "half_neg")


def check_three_items_and_broadcast(X, E, mem, cap):
    """K = cap, B = 3 with the items 'half', 'half_neg' and 'rand' in one call; then the broadcast form with the 'half' second operand
    against the stacked form and against the restatement"""
    items = [truth(E, cap, p) for p in ("half", "half_neg", "rand")]
    a3 = np.stack([a for a, _, _ in items], axis=1)
    got = ms.run(X, mem, a3, np.stack([b for _, b, _ in items], axis=1))
    worst = 0
    for i, (p, (a, b, want)) in enumerate(zip(("half", "half_neg", "rand"), items)):
        worst = max(worst, check_item(E, a, b, got[i], want, "item %d of 3, %s" % (i, p), centred=p != "half_neg"))
    half_b = items[0][1]
    cast = ms.run(X, mem, a3, half_b[:, None], bcast=True)
    assert (cast == ms.run(X, mem, a3, np.broadcast_to(half_b[:, None], a3.shape).copy())).all(), "broadcast differs from stacked"
    assert (cast[0] == items[0][2]).all() and (cast[1] == items[0][2]).all(), "broadcast 'half' differs from the restatement"
    assert (cast[2] == ms.restate(E).multiply_sum(items[2][0], half_b)).all(), "uniform words against broadcast 'half' differ from the restatement"
    return worst


def check_refused_above_the_cap(X, E, mem, api, cap):
    a, b = ms.operands(E, cap + 1, 1, "half", SEED)
    out = mem.to_dev(np.full((1, 3, E.L, E.n), 12345, np.uint64))
    with pytest.raises(api.HheError) as e:
        X.multiply_sum(mem.to_dev(a), mem.to_dev(b), cap + 1, out, 1)
    assert e.value.code == api.ERR_INVALID and "behz_sum_cap" in str(e.value)
    assert (mem.to_host(out) == 12345).all()


def check_tightness(E, cap):
    """no device and no emulator: the restatement at K = cap + 1 on 'half'.  Returns its distance"""
    a, b, words = truth(E, cap + 1, "half")
    return ms.sum_distance(E, a, b, words, coefficients(E.n))


def check_multiply_and_square(X, E, mem):
    """hhe_square(a) == hhe_multiply(a, a) == the oracle's multiply(a, a) on 'half' (mlp_common.check_square), within L + 1 of the
    rounded integer product.  Returns the distance"""
    got = mc.check_square(X, E, mem, 1, "half")
    a = E.half(2)
    dist = dc.behz_distance(E, a, a, got[0], coefficients(E.n))
    print("BEHZ distance of hhe_multiply on 'half', N = %d, L = %d: %d" % (E.n, E.L, dist))
    assert dist <= E.L + 1, ("hhe_multiply is", dist, "from the rounded integer product; the cap is L + 1 =", E.L + 1)
    return dist


# ---- cap == 0 ----
_zero = {}


def zero_setup(orc, name):
    """(Setup with every default Galois key, Env) of a ZERO context"""
    if name not in _zero:
        q = orc.coeff_modulus_create(1024, ZERO[name])
        assert [int(p).bit_length() for p in q] == ZERO[name]
        _zero[name] = (fp.make_setup(orc, 10, q, t=T60), dc.env(orc, 10, q, T60))
    return _zero[name]


def check_zero_multiply(X, E, mem):
    """the pin: at cap == 0 hhe_multiply on 'half' gives the oracle's words, and both are MORE than L + 1 from the rounded integer
    product.  Returns the distance"""
    assert X.query("behz_sum_cap") == ms.sum_cap(E.n, E.q[:E.L], E.bsk, E.t) == 0
    a = E.half(2)
    out = mem.empty((1, 3, E.L, E.n))
    X.multiply(mem.to_dev(a[None]), mem.to_dev(a[None]), out, 1)
    got, ref = mem.to_host(out)[0], E.O.multiply(a, a)
    assert (got == ref).all(), "hhe_multiply differs from the oracle's multiply on 'half'"
    idx = coefficients(E.n)
    dist = {who: dc.behz_distance(E, a, a, words, idx) for who, words in (("oracle", ref), ("product", got))}
    print("BEHZ distance at behz_sum_cap == 0, L = %d: %s" % (E.L, dist))
    for who, d in dist.items():
        assert d > E.L + 1, (who, "is within L + 1 of the rounded integer product where behz_sum_cap is 0: the operands no longer sit at the bound")
    return dist["product"]


def check_zero_layers(X, S, mem, orc, seed):
    """the per-product layers on real encryptions, 3 x 5: the words of the oracle's composition, its budget positive, (M x) mod t.
    Over ONE 60-bit data prime Q / t is below 2 and a fresh encryption has no noise budget, on the oracle as in SEAL: nothing decrypts
    there whatever the layer does.  That is asserted, and the layers are held to the oracle's words alone."""
    O = S.O
    M = fp.seeded_matrix(S.t, 3, 5, seed)
    if O.L > 1:
        fp.check_layer(X, S, mem, M, B=2, seed=seed)
        rmc.check_hoisted_layer(X, S, mem, orc, M, B=2, seed=seed)
        return
    assert int(S.q[0]) < 2 * S.t and O.noise_budget(S.sk, fp.encrypt_inputs(S, [np.arange(5, dtype=np.uint64)], seed=seed)[0]) == 0
    xs = [np.random.default_rng(2000 + seed).integers(0, S.t, size=5, dtype=np.uint64) for _ in range(2)]
    W, cts = fp.encrypt_diagonals(S, M, seed=300 + seed), fp.encrypt_inputs(S, xs, seed=100 + seed)
    mat = X.enc_matrix(mem.to_dev(W), 3, 5)
    try:
        shape = (2,) + tuple(O.ct_shape)
        for form, ref in ((mat.apply, fp.fc_packed_ref), (mat.apply_hoisted, rmc.fc_packed_hoisted_ref)):
            got = mem.to_host(form(mem.to_dev(cts), 2, out=mem.empty(shape)))
            for b in range(2):
                assert (got[b] == ref(O, S.rk, S.gk, W, cts[b], 3, 5)).all(), ("differs from the oracle's composition", ref.__name__, b)
    finally:
        mat.destroy()


def check_zero_refusals(X, S, mem, api):
    """the sum forms refuse with `out` untouched"""
    shape = (1,) + tuple(S.O.ct_shape)
    M, M1 = fp.seeded_matrix(S.t, 3, 5, 92), fp.seeded_matrix(S.t, 2, 3, 93)
    cyc = X.enc_matrix(mem.to_dev(fp.encrypt_diagonals(S, M, seed=810)), 3, 5)
    first = X.enc_matrix_open(mem.to_dev(mc.encrypt_open_diagonals(S, M, seed=820)), 3, 5)
    second = X.enc_matrix_open(mem.to_dev(mc.encrypt_open_diagonals(S, M1, seed=830)), 2, 3)
    d_in = mem.to_dev(mc.full_inputs(S, 5, 1, 94)[0])
    calls = [lambda o: cyc.apply_sum(d_in, 1, out=o, hoisted=False), lambda o: cyc.apply_sum(d_in, 1, out=o, hoisted=True),
             lambda o: first.apply_open(d_in, 1, out=o), lambda o: X.mlp([first, second], d_in, o, 1)]
    try:
        for i, call in enumerate(calls):
            out = mem.to_dev(np.full(shape, 12345, np.uint64))
            with pytest.raises(api.HheError) as e:
                call(out)
            assert e.value.code == api.ERR_INVALID and "behz_sum_cap" in str(e.value), (i, str(e.value))
            assert (mem.to_host(out) == 12345).all(), i
    finally:
        for m in (cyc, first, second):
            m.destroy()
