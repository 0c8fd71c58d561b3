"""Evaluation below the data level: what tests/test_level_emu.py (emulator, numpy memory) and tests/test_gpu_level.py (gfx950, torch
memory) share.

A level with l data primes is the BFV context over {q_0 .. q_{l-1}, q_sp} (hhe_ctx_create_level); its key-switch keys are digits
I < l and limbs {0 .. l-1, special} of the parent's (hhe_keyset_derive_level).  The truth of every comparison is the oracle of the
shortened chain (mod_switch_common.short_oracle's context) called with key words projected in numpy.  The projection itself is held
to two statements that share nothing with it: the structural key relation of keygen_common on a device-generated parent key, and
the Python-integer definition of the key switch of definition_common with the digits I < l.  Every comparison is exact word equality.
"""
import ctypes as C

import numpy as np
import pytest

import affine_common as ac
import definition_common as dc
import keygen_common as kg
import mod_switch_common as ms
import parity_common as pc

T16, T33 = 65537, 8088322049

# name -> (logn, bit sizes with the special prime last, levels, row_kernel per level, digit_reduce per level)
# n1024_4x50: ragged tiles; level 1 is K = 2, one digit, a BEHZ base of two primes.
# n4096_4x60: the row kernels at L = 2 and 1.
# n1024_mixed: mod_switch_common's chain.  Every level from 2 up holds the 18-bit q_0 and the 60-bit q_1: digits are reduced, as on
#   the parent.  Level 1 has the 18-bit prime alone as data: nothing to reduce, unlike the parent.  pm_ok holds for the primes of 33
#   bits and more only, so the set of lazy primes changes with the level as well; assert_dispatch compares prime by prime.
# n1024_10x50: level 9 (the same chain, a second context) and level 8: the two sides of the noise kernel's register / LDS boundary.
CHAINS = {
    "n1024_4x50": (10, [50] * 4, (2, 1), {2: 0, 1: 0}, {2: 0, 1: 0}),
    "n4096_4x60": (12, [60] * 4, (2, 1), {2: 1, 1: 1}, {2: 0, 1: 0}),
    "n1024_mixed": (10, [18, 60, 30, 59, 20, 45, 60], (4, 3, 2, 1), {4: 0, 3: 0, 2: 0, 1: 0}, {4: 1, 3: 1, 2: 1, 1: 0}),
    "n1024_10x50": (10, [50] * 10, (9, 8), {9: 0, 8: 0}, {9: 0, 8: 0}),
}
EMU_CASES = [(c, l) for c in CHAINS for l in CHAINS[c][2]]


def rows(l, K):
    return list(range(l)) + [K - 1]


def project(key, l):
    """[L][2][K][N] -> [l][2][l+1][N]: digits I < l, limbs {0 .. l-1, K-1}"""
    key = np.asarray(key)
    K = key.shape[2]
    return np.ascontiguousarray(key[:l][:, :, rows(l, K)])


_setups = {}


def parent_setup(orc, chain, logn=None, q=None, all_galois=True):
    """conftest.Setup of a chain with every default Galois key (steps +-2^k and the column swap) and the relin key, made once.
    chain: a name of CHAINS, or any name with logn and the primes q given (all_galois = False: the keys of steps -1, 0, 128 only)"""
    if chain not in _setups:
        if q is None:
            logn, bits = CHAINS[chain][:2]
            q = orc.coeff_modulus_create(1 << logn, bits)
        _setups[chain] = pc.setup_from_primes(orc, logn, q, T16, all_galois=all_galois)
    return _setups[chain]


def level_setup(orc, api, S, l):
    """S_l: the Setup of the level with l data primes, every key a projection of S's -- nothing is generated"""
    if ("level", id(S), l) in _setups:
        return _setups[("level", id(S), l)]
    from conftest import Setup
    K = len(S.q)
    Sl = Setup.__new__(Setup)
    Sl.t, Sl.logn, Sl.n = S.t, S.logn, S.n
    Sl.q = [S.q[j] for j in rows(l, K)]
    Sl.O = orc.Oracle(S.logn, Sl.q, S.t)
    Sl.sk, Sl.pk = api.level_rows(S.sk, l), api.level_rows(S.pk, l)
    O2, sk2 = ms.short_oracle(orc, S.O, S.sk, l)
    assert O2.q == Sl.q and (sk2 == Sl.sk).all() and Sl.pk.shape == (2, l + 1, S.n)
    Sl.rk = project(S.rk, l)
    Sl.gk = orc.GaloisKeys(S.gk.elts, np.stack([project(k, l) for k in S.gk.keys]))
    Sl.key = S.key
    Sl.enc_key = Sl.O.encrypt(Sl.pk, Sl.O.pasta_pack_key(S.key), 11)
    _setups[("level", id(S), l)] = Sl
    return Sl


def top_set(X, S):
    ks = X.keyset()
    ks.set_relin(S.rk)
    for e, k in zip(S.gk.elts, S.gk.keys):
        ks.set_galois(int(e), k)
    return ks


def switched(X, S, mem, cts, l, size=2):
    """oracle ciphertexts of the top [B][size][L][N] -> (device, host) words at level l, by hhe_mod_switch on the parent"""
    B = len(cts)
    d = ms.switch(X, mem, mem.to_dev(cts), size, B, S.O.L, l)
    return d, mem.to_host(d)


# ---- 1. the context of a level ----
def check_context(X, S, orc, api, l):
    O = S.O
    Xl = X.at_level(l)
    Ol, _ = ms.short_oracle(orc, O, S.sk, l)
    assert (Xl.L, Xl.K, Xl.n, Xl.t, Xl.q) == (l, l + 1, O.n, O.t, Ol.q)
    pc.check_context_constants(Xl, Ol)
    for i in range(O.n):
        assert Xl.query("slot_map", i) == X.query("slot_map", i)
    # the BEHZ base is a prefix of the parent's, with its m_sk and gamma
    assert [Xl.query("bsk", i) for i in range(l)] == [X.query("bsk", i) for i in range(l)]
    assert Xl.query("bsk", l) == X.query("bsk", O.L) and Xl.query("gamma") == X.query("gamma")
    # a level of a level is the level of the parent
    for m in sorted({1, max(1, l - 1), l}):
        Xm = Xl.at_level(m)
        Om, _ = ms.short_oracle(orc, O, S.sk, m)
        assert Xm.q == Om.q
        pc.check_context_constants(Xm, Om)
        Xm.close()
    Xl.close()


def check_context_refusals(X, api):
    for limbs in (0, X.L + 1, -1):
        with pytest.raises(api.HheError) as e:
            X.at_level(limbs)
        assert e.value.code == api.ERR_INVALID, limbs
    h = C.c_void_p()
    assert X.lib.hhe_ctx_create_level(C.c_void_p(0), C.c_int(1), C.byref(h)) == api.ERR_INVALID and not h.value
    assert X.lib.hhe_ctx_create_level(X.h, C.c_int(1), C.c_void_p(0)) == api.ERR_INVALID
    assert X.lib.hhe_keyset_derive_level(C.c_void_p(0), C.c_void_p(0)) == api.ERR_INVALID


# ---- 2. derivation ----
def assert_set_is(ks, rk, gk, l, what):
    """the set holds exactly the projection of (rk, gk) to level l (rk None: no relin key)"""
    assert ks.has_relin() == (rk is not None), what
    if rk is not None:
        got = ks.get_relin()
        assert got.shape == (l, 2, l + 1, got.shape[3]) and (got == project(rk, l)).all(), (what, "relin")
    for e, k in zip(gk.elts, gk.keys):
        assert ks.has_galois(int(e)), (what, int(e))
        assert (ks.get_galois(int(e)) == project(k, l)).all(), (what, int(e))


def check_derivation_uploaded(X, S, orc, api, levels):
    """uploaded oracle keys: get == numpy projection for relin and every Galois key; one launch per key; level -> lower level ==
    direct derivation; a level of a level; equal chains copy; former keys of dst are gone"""
    O, L = S.O, S.O.L
    top = top_set(X, S)
    nkeys = 1 + len(S.gk.elts)
    for l in levels:
        Xl = X.at_level(l)
        dl = Xl.keyset()
        # dst holds a key of an element src does not have, and a relin key of its own: both go
        stale = int(O.galois_elt(-5))
        assert not top.has_galois(stale)
        junk = np.zeros((l, 2, l + 1, O.n), np.uint64)
        dl.set_galois(stale, junk)
        dl.set_relin(junk)
        n0 = Xl.query("key_proj_launches")
        assert dl.derive_from(top) is dl
        assert Xl.query("key_proj_launches") == n0 + nkeys
        assert not dl.has_galois(stale)
        assert_set_is(dl, S.rk, S.gk, l, ("direct", l))
        for m in sorted({1, max(1, l - 1)}):
            Xm, Xlm = X.at_level(m), Xl.at_level(m)
            for Xd, src, what in ((Xm, dl, "level -> lower level"), (Xm, top, "direct"), (Xlm, dl, "into a level of a level")):
                dm = Xd.keyset()
                n1 = Xd.query("key_proj_launches")
                dm.derive_from(src)
                assert Xd.query("key_proj_launches") == n1 + nkeys
                assert_set_is(dm, S.rk, S.gk, m, (what, l, m))
            Xm.close(); Xlm.close()
        # src without a relin key: dst loses its own
        only_gk = X.keyset()
        only_gk.set_galois(int(S.gk.elts[0]), S.gk.keys[0])
        dl.derive_from(only_gk)
        assert not dl.has_relin() and dl.has_galois(int(S.gk.elts[0])) and not dl.has_galois(int(S.gk.elts[1]))
        assert (dl.get_galois(int(S.gk.elts[0])) == project(S.gk.keys[0], l)).all()
        only_gk.close()
        Xl.close()
    # equal chains copy, in both directions, also within one context
    X2 = X.at_level(L)
    for Xd in (X2, X):
        c = Xd.keyset()
        c.derive_from(top)
        assert_set_is(c, S.rk, S.gk, L, "equal chains")
        back = X.keyset()
        back.derive_from(c)
        assert_set_is(back, S.rk, S.gk, L, "equal chains, back")
    X2.close()
    top.close()


def check_derivation_refusals(X, S, orc, api, l):
    """upward, foreign chain, other special prime, other t, other N, dst == src: HHE_ERR_INVALID, dst's words as they were, no launch"""
    O, n, logn = S.O, S.O.n, S.O.logn
    Xl = X.at_level(l)
    top = top_set(X, S)
    dl = Xl.keyset().derive_from(top)
    cm = orc.coeff_modulus_create
    other_sp = [v for v in cm(n, [49] * 2) if v not in S.q][0]
    foreign = {
        "foreign chain": api.Context(logn, cm(n, [49] * (O.K)), S.t, lib=X.lib),
        "other special prime": api.Context(logn, S.q[:O.L] + [other_sp], S.t, lib=X.lib),
        "not a prefix": api.Context(logn, S.q[1:], S.t, lib=X.lib) if O.L > 1 else None,
        "other t": api.Context(logn, S.q, T33, lib=X.lib),
        "other N": api.Context(logn + 1, cm(2 * n, [50] * O.K), S.t, lib=X.lib),
    }
    before_rk, e0 = dl.get_relin(), int(S.gk.elts[0])
    before_gk = dl.get_galois(e0)
    n0 = Xl.query("key_proj_launches")

    def refused(dst, src, what):
        with pytest.raises(api.HheError) as e:
            dst.derive_from(src)
        assert e.value.code == api.ERR_INVALID, what

    for what, Xf in foreign.items():
        if Xf is None:
            continue
        src = Xf.keyset()
        src.set_relin(np.zeros((Xf.L, 2, Xf.K, Xf.n), np.uint64))
        refused(dl, src, what)
        mine = Xf.keyset()
        refused(mine, top, what + ", the other way")
        assert not mine.has_relin()
        Xf.close()
    refused(dl, dl, "dst == src")
    up = X.keyset()
    up.set_galois(e0, S.gk.keys[1])   # something to keep
    refused(up, dl, "upward")
    assert (up.get_galois(e0) == S.gk.keys[1]).all() and not up.has_relin()
    if l > 1:
        X1 = X.at_level(1)
        low = X1.keyset().derive_from(top)
        refused(dl, low, "upward from a lower level")
        X1.close()
    assert (dl.get_relin() == before_rk).all() and (dl.get_galois(e0) == before_gk).all()
    assert sorted(int(e) for e in S.gk.elts if dl.has_galois(int(e))) == sorted(int(e) for e in S.gk.elts)
    assert Xl.query("key_proj_launches") == n0 and X.query("key_proj_launches") == 0
    Xl.close()
    top.close()


def check_derivation_keeps_keystreams(X, S, orc, api, mem, l):
    """serial-dependent behaviour: a keystream kept under the level's derived sets survives a refused derivation and is gone after a
    successful one; the level context transciphers to the words of the short oracle"""
    Sl = level_setup(orc, api, S, l)
    Xl = X.at_level(l)
    top = top_set(X, S)
    dl = Xl.keyset().derive_from(top)
    pt = np.array([(7 * i + 3) % 256 for i in range(128)], dtype=np.uint64)
    cw, ncw = Sl.sym_blocks(orc, pt)
    want = Sl.O.transcipher_block(Sl.enc_key, Sl.rk, Sl.gk, cw[0, :ncw[0]], 0)
    key = mem.to_dev(Sl.enc_key)

    def run():
        out = mem.empty((1,) + Sl.O.ct_shape)
        Xl.transcipher(key, cw, ncw, [0], out, rk=dl, gk=dl)
        assert (mem.to_host(out)[0] == want).all()
        return Xl.query("transcipher_evaluated"), Xl.query("ks_cache_hits")

    assert run() == (1, 0)
    assert run() == (0, 1)
    Xf = api.Context(S.logn, orc.coeff_modulus_create(S.n, [49] * 3), S.t, lib=X.lib)
    with pytest.raises(api.HheError):
        dl.derive_from(Xf.keyset())
    Xf.close()
    assert run() == (0, 1), "a refused derivation dropped the kept keystream"
    dl.derive_from(top)
    assert run() == (1, 0), "a keystream kept under the replaced keys was served"
    Xl.close()
    top.close()


def check_derivation_generated(X, S, orc, api, mem, levels, seed=kg.SEED, seed2=bytes((5 * i + 1) % 256 for i in range(32))):
    """keys generated on the device: get == projection; the projected words satisfy the structural key relation on every kept limb;
    re-derivation after the parent regenerated a key changes the level's words and its rotations"""
    O = S.O
    D = kg.DeviceKeys(X, O, mem, seed)
    e1 = int(O.galois_elt(1))
    elts = [e1, int(O.galois_elt(0))]
    ks = D.keyset(elts)
    rk, gk = ks.get_relin(), kg.oracle_gk(orc, ks, elts)
    vals = np.random.default_rng(5).integers(0, 256, O.n).astype(np.uint64)
    ct = O.encrypt(D.pk, O.encode(vals), 21)
    for l in levels:
        Ol, sk_l = ms.short_oracle(orc, O, D.sk, l)
        assert (sk_l == api.level_rows(D.sk, l)).all()
        Xl = X.at_level(l)
        dl = Xl.keyset().derive_from(ks)
        assert_set_is(dl, rk, gk, l, ("generated", l))
        # k0 + k1 s - [j == I] (q_sp mod q_I) new_key = -e, small, the same polynomial on every kept limb
        noise = lambda purpose, elt: [kg.small_poly(seed, purpose, elt, I, kg.NOISE, O.n) for I in range(l)]
        kg.check_structure(Ol, sk_l, dl.get_relin(), kg.new_key_relin(Ol, sk_l), noise(kg.RELIN, 0))
        for e in elts:
            kg.check_structure(Ol, sk_l, dl.get_galois(e), kg.new_key_galois(Ol, sk_l, e), noise(kg.GALOIS, e))
        # the parent regenerates one key: the level's copy is the old one until it is derived again
        d_low, low = switched(X, S, mem, ct[None], l)
        out = mem.empty((1,) + Ol.ct_shape)
        Xl.rotate_rows(d_low, 1, out, 1, gk=dl)
        first = mem.to_host(out)[0].copy()
        assert (first == Ol.rotate_rows(low[0], 1, orc.GaloisKeys(elts, np.stack([project(k, l) for k in gk.keys])))[0]).all()
        ks.generate_galois(D.d_sk, seed2, [e1])
        new_words = ks.get_galois(e1)
        assert (new_words != gk.keys[0]).any()
        Xl.rotate_rows(d_low, 1, out, 1, gk=dl)
        assert (mem.to_host(out)[0] == first).all()
        dl.derive_from(ks)
        assert (dl.get_galois(e1) == project(new_words, l)).all()
        Xl.rotate_rows(d_low, 1, out, 1, gk=dl)
        second = mem.to_host(out)[0]
        assert (second != first).any()
        assert (second == Ol.apply_galois(low[0], e1, project(new_words, l))).all()
        if Ol.noise_budget(sk_l, second) > 0:
            assert (kg.slots_of(Ol, sk_l, second) == kg.rot_rows(vals, 1)).all()
        ks.generate_galois(D.d_sk, seed, [e1])   # as it was, for the next level
        assert (ks.get_galois(e1) == gk.keys[0]).all()
        Xl.close()
    ks.close()


# ---- the key switch of a derived key against the integer definition, digits I < l ----
class ProjectedSparseKey:
    """definition_common.SparseKey of the parent seen from the level: the monomials of the digits I < l, their coefficients
    (integers mod Q p of the parent) reduced mod Q_l p.  Nothing of the words is used: X() is SparseKey's sum over these terms."""

    def __init__(self, E_l, parent_key):
        self.terms = [[[(c % E_l.QP, e) for c, e in parent_key.terms[I][k]] for k in range(2)] for I in range(E_l.L)]

    X = dc.SparseKey.X


def check_definition(X, S, orc, mem, l, seed=0):
    """running + floor((X_k + floor(p / 2)) / p) mod q_j with X_k = sum over I < l of d_I key[I][k] in Python integers, for a sparse
    key uploaded at the top and derived on the device; every entry point, full output vector"""
    O = S.O
    E = dc.env(orc, O.logn, S.q, S.t)
    El = dc.env(orc, O.logn, [S.q[j] for j in rows(l, O.K)], S.t)
    parent_key = E.stored(("sparse", seed), lambda: dc.SparseKey(E, seed))
    key = ProjectedSparseKey(El, parent_key)
    Xl = X.at_level(l)
    for e_i, entry in enumerate(dc.entries(El)):
        top, dl = X.keyset(), Xl.keyset()
        if entry[0] == "relin":
            top.set_relin(parent_key.words)
        else:
            top.set_galois(dc.entry_elt(El, entry), parent_key.words)
        dl.derive_from(top)
        cts = dc.switch_inputs(El, entry, 3, seed + 10 * e_i)
        want = [dc.switch_truth(El, entry, key, ct) for ct in cts]
        d_in, out = mem.to_dev(cts), mem.empty((3, 2, l, O.n))
        if entry[0] == "relin":
            Xl.relinearize(d_in, out, 3, rk=dl)
        elif entry[0] == "galois":
            Xl.apply_galois(d_in, entry[1], out, 3, gk=dl)
        elif entry[0] == "rows":
            Xl.rotate_rows(d_in, entry[1], out, 3, gk=dl)
        else:
            Xl.rotate_columns(d_in, out, 3, gk=dl)
        got = mem.to_host(out)
        for b in range(3):
            dc.assert_switch("level %d, item %d" % (l, b), entry, got[b], want[b])
        top.close(); dl.close()
    Xl.close()


# ---- 3. evaluation at the level ----
def check_eval(X, S, orc, api, mem, l, row_kernel, digit_reduce, B=2, n_in=9, dim=16, every_key=True):
    """every op at the level against the short oracle with projected keys: parity_common's checks on S_l with the keys uploaded into
    the level's default set (every_key: check_ops, which rotates by every key of the set), then inputs encrypted at the top and
    switched, evaluated under the DERIVED set.  row_kernel / digit_reduce: what the level context must report (CHAINS)"""
    O = S.O
    Sl = level_setup(orc, api, S, l)
    Ol = Sl.O
    Xl = X.at_level(l)
    pc.assert_dispatch(Xl, Sl.q, row_kernel, digit_reduce)
    Sl.load_keys(Xl)
    pc.check_context_constants(Xl, Ol)
    if every_key:
        pc.check_ops(Xl, Sl, mem, B=B, seed=l)
    fresh = Ol.encrypt(Sl.pk, Ol.encode(np.arange(8, dtype=np.uint64)), 5)
    if Ol.noise_budget(Sl.sk, fresh, O.n) > 0:
        pc.check_decrypt(Xl, Sl, mem, B=B, seed=l)
    else:   # a data modulus too small to hold a plaintext mod t (the 18-bit q_0 alone): the words of the decryption, not their meaning
        d_out = mem.empty((1, O.n))
        Xl.decrypt(Sl.sk, mem.to_dev(fresh[None]), 1, d_out)
        assert (mem.to_host(d_out)[0] == Ol.decode(Ol.decrypt(Sl.sk, fresh))).all()
    if l == 1 and O.n <= 4096:
        # a ragged two-block transciphering at one data prime: the fused matmul loop's scratch is L + 2 polynomials per item there, more
        # than a ciphertext's 2 L (lane_reserve); the diagonal affine layer below runs the same loop.  Words only: 128 rotations and
        # three multiplications leave no budget under one prime
        pc.check_transcipher(Xl, Sl, orc, mem, [(7 * i + 3) % 256 for i in range(128 + 44)], check_decrypt=False)
    top = top_set(X, S)
    dl = Xl.keyset().derive_from(top)
    rng = np.random.default_rng(100 + l)
    n, t = O.n, O.t
    vals = rng.integers(0, t, (B, n), dtype=np.uint64)
    cts = np.stack([O.encrypt(S.pk, O.encode(vals[b]), 300 + b) for b in range(B)])
    d_low, low = switched(X, S, mem, cts, l)
    out = mem.empty((B,) + Ol.ct_shape)
    # rotate_rows with a key, through NAF terms (3 = -1 + 4), rotate_columns
    for step, nks in ((-1, 1), (3, 2)):
        Xl.rotate_rows(d_low, step, out, B, gk=dl)
        got = mem.to_host(out)
        for b in range(B):
            ref, k = Ol.rotate_rows(low[b], step, Sl.gk)
            assert k == nks and (got[b] == ref).all(), ("rotate_rows", step, b)
    Xl.rotate_columns(d_low, out, B, gk=dl)
    got = mem.to_host(out)
    for b in range(B):
        assert (got[b] == Ol.rotate_columns(low[b], Sl.gk)).all(), ("rotate_columns", b)
    # multiply -> relinearize at the level
    o3 = mem.empty((B, 3, l, n))
    Xl.multiply(d_low, mem.to_dev(low[::-1].copy()), o3, B)
    h3 = mem.to_host(o3)
    Xl.relinearize(o3, out, B, rk=dl)
    got = mem.to_host(out)
    for b in range(B):
        assert (h3[b] == Ol.multiply(low[b], low[B - 1 - b])).all(), ("multiply", b)
        assert (got[b] == Ol.relinearize(h3[b], Sl.rk)).all(), ("relinearize", b)
    # entering at size 3: multiply at the top, switch the product, relinearize at the level
    t3 = mem.empty((B, 3, O.L, n))
    X.multiply(mem.to_dev(cts), mem.to_dev(cts[::-1].copy()), t3, B)
    d3 = ms.switch(X, mem, t3, 3, B, O.L, l)
    low3 = mem.to_host(d3)
    for b in range(B):
        assert (low3[b] == ms.chain(O.multiply(cts[b], cts[B - 1 - b]), O.q)[l]).all(), ("size 3 switch", b)
    Xl.relinearize(d3, out, B, rk=dl)
    got = mem.to_host(out)
    for b in range(B):
        assert (got[b] == Ol.relinearize(low3[b], Sl.rk)).all(), ("relinearize of a switched product", b)
    # mask, flatten of two blocks (step -128 through the derived set)
    mv = rng.integers(0, 2, 44).astype(np.uint64)
    Xl.mask(d_low, mv, out, B)
    got = mem.to_host(out)
    for b in range(B):
        assert (got[b] == Ol.mask(low[b], mv)).all(), ("mask", b)
    fo = mem.empty((1,) + Ol.ct_shape)
    Xl.flatten(d_low, 2, fo, 1, gk=dl)
    assert (mem.to_host(fo)[0] == Ol.flatten(low[:2], Sl.gk)).all(), "flatten"
    # an FC row and its weight row, switched once
    v, w = rng.integers(0, 4, (B, n_in)), rng.integers(-8, 9, n_in)
    vi = np.stack([O.encrypt(S.pk, O.encode(v[b]), 320 + b) for b in range(B)])
    wc = O.encrypt(S.pk, O.encode(w % t), 330)
    d_vi, low_vi = switched(X, S, mem, vi, l)
    d_w, low_w = switched(X, S, mem, wc[None], l)
    Xl.fc_row(d_vi, d_w, 1, n_in, out, B, rk=dl, gk=dl)
    got = mem.to_host(out)
    for b in range(B):
        assert (got[b] == Ol.fc_row(low_vi[b], low_w[0], Sl.rk, Sl.gk, n_in)[0]).all(), ("fc_row", b)
    assert Xl.query("fc_fallbacks") == 0
    # a packed affine layer, diagonal and babystep-giantstep, the matrix handle made on the level context
    M, bias = ac.seeded_matrix(t, dim, 77 + l)
    xs = rng.integers(0, t, (B, dim), dtype=np.uint64)
    a_cts = np.stack([O.encrypt(S.pk, O.encode(xs[b]), 340 + b) for b in range(B)])
    d_a, low_a = switched(X, S, mem, a_cts, l)
    for bsgs in (None, (4, 4)):
        mat = Xl.matrix(M, bias=bias, bsgs=bsgs)
        Xl.packed_affine(d_a, mat, out, B, gk=dl)
        got = mem.to_host(out)
        for b in range(B):
            assert (got[b] == ac.packed_affine_ref(Ol, Sl.gk, M, low_a[b], bias, bsgs)).all(), ("packed_affine", bsgs, b)
        mat.close()
    Xl.close()
    top.close()
    return Sl


def check_rotation_and_relin(X, S, orc, api, mem, l, row_kernel, B=2):
    """one rotation and one relinearization at the level with real keys, derived on the device from the uploaded parent set"""
    O = S.O
    Sl = level_setup(orc, api, S, l)
    Ol = Sl.O
    Xl = X.at_level(l)
    pc.assert_dispatch(Xl, Sl.q, row_kernel)
    top = top_set(X, S)
    dl = Xl.keyset().derive_from(top)
    assert_set_is(dl, S.rk, S.gk, l, "derived")
    rng = np.random.default_rng(200 + l)
    vals = rng.integers(0, O.t, (B, O.n), dtype=np.uint64)
    cts = np.stack([O.encrypt(S.pk, O.encode(vals[b]), 300 + b) for b in range(B)])
    d_low, low = switched(X, S, mem, cts, l)
    out, o3 = mem.empty((B,) + Ol.ct_shape), mem.empty((B, 3, l, O.n))
    Xl.rotate_rows(d_low, -1, out, B, gk=dl)
    got = mem.to_host(out)
    for b in range(B):
        assert (got[b] == Ol.rotate_rows(low[b], -1, Sl.gk)[0]).all(), ("rotate_rows", b)
    assert (kg.slots_of(Ol, Sl.sk, got[0]) == kg.rot_rows(vals[0], -1)).all()
    Xl.multiply(d_low, d_low, o3, B)
    Xl.relinearize(o3, out, B, rk=dl)
    h3, got = mem.to_host(o3), mem.to_host(out)
    for b in range(B):
        assert (h3[b] == Ol.multiply(low[b], low[b])).all(), ("multiply", b)
        assert (got[b] == Ol.relinearize(h3[b], Sl.rk)).all(), ("relinearize", b)
    Xl.close()
    top.close()


def check_noise_form(X, S, orc, api, mem, l, B=2):
    """hhe_noise_budget on the level context: the form the launch takes is the level's, the figures are those of the parent at
    `limbs` = l (pinned to the definition by the noise tests) and the short oracle's to one bit"""
    O = S.O
    Sl = level_setup(orc, api, S, l)
    Xl = X.at_level(l)
    rng = np.random.default_rng(7)
    cts = np.stack([O.encrypt(S.pk, O.encode(rng.integers(0, O.t, O.n, dtype=np.uint64)), 400 + b) for b in range(B)])
    d_low, low = switched(X, S, mem, cts, l)
    got = Xl.noise_budget(Sl.sk, d_low, B, with_bits=True)
    assert Xl.query("noise_form") == (l if l <= 8 else 0)
    want = X.noise_budget(S.sk, d_low, B, limbs=l, with_bits=True)
    assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist()
    for b in range(B):
        assert got[0][b] > 0 and 0 <= got[0][b] - Sl.O.noise_budget(Sl.sk, low[b], O.n) <= 1
    Xl.close()


# ---- 4. meaning, without an oracle key ----
def check_keyless_level(X, O, orc, api, mem, level, seed=kg.SEED, seed2=bytes((5 * i + 1) % 256 for i in range(32))):
    """device keys, device encryption, a product at the top, switched to `level`; keys derived; rotate + multiply_plain + add at the
    level; decrypted on the level context with level_rows(sk): the slots in Python integers mod t.  The device's own noise budget at
    the level is positive.  The oracle only reports, given the device's key, the budget of the same flow at every level: `level` is
    the lowest one from which every level upward has budget."""
    n, L, t = O.n, O.L, O.t
    d_sk, d_pk = mem.empty((O.K, n)), mem.empty((2, O.K, n))
    X.keygen_secret(seed, d_sk)
    X.keygen_public(d_sk, seed, d_pk)
    ks = X.keyset()
    ks.generate_relin(d_sk, seed2)
    ks.generate_galois(d_sk, seed2, [int(O.galois_elt(1))])
    rng = np.random.default_rng(92)
    a, b, c = (rng.integers(0, t, (2, n), dtype=np.uint64) for _ in range(3))
    d_pa, d_pb, d_pc = mem.empty((2, n)), mem.empty((2, n)), mem.empty((2, n))
    for v, d in ((a, d_pa), (b, d_pb), (c, d_pc)):
        X.encode(mem.to_dev(v), 2, n, d)
    d_a, d_b = mem.empty((2,) + O.ct_shape), mem.empty((2,) + O.ct_shape)
    X.encrypt(d_pk, d_pa, seed, 2, d_a)
    X.encrypt(d_pk, d_pb, seed2, 2, d_b)
    d_3, d_r = mem.empty((2, 3, L, n)), mem.empty((2,) + O.ct_shape)
    X.reserve(2)
    X.multiply(d_a, d_b, d_3, 2)
    X.relinearize(d_3, d_r, 2, rk=ks)
    X.sync()
    sk = mem.to_host(d_sk)
    prod = [[int(x) * int(y) % t for x, y in zip(a[i], b[i])] for i in range(2)]
    want = np.array([[(int(r) * int(z) + p) % t for r, z, p in zip(kg.rot_rows(np.array(prod[i], dtype=object), 1), c[i], prod[i])]
                     for i in range(2)], dtype=np.uint64)

    def at(l):
        Xl = X.at_level(l)
        dl = Xl.keyset().derive_from(ks)
        d_low = ms.switch(X, mem, d_r, 2, 2, L, l)
        d_rot, d_mul, d_sum, d_vals = mem.empty((2, 2, l, n)), mem.empty((2, 2, l, n)), mem.empty((2, 2, l, n)), mem.empty((2, n))
        Xl.reserve(2)
        Xl.rotate_rows(d_low, 1, d_rot, 2, gk=dl)
        Xl.multiply_plain(d_rot, d_pc, d_mul, 2)
        Xl.add(d_mul, d_low, d_sum, 2)
        Xl.sync()
        sk_l = api.level_rows(sk, l)
        mine = Xl.noise_budget(sk_l, d_sum, 2)
        Xl.decrypt(sk_l, d_sum, 2, d_vals)
        Ol, sk2 = ms.short_oracle(orc, O, sk, l)
        theirs = min(Ol.noise_budget(sk2, ct, n) for ct in mem.to_host(d_sum))
        res = (int(min(mine)), theirs, mem.to_host(d_vals).copy())
        Xl.close()
        return res

    res = {l: at(l) for l in range(L, 0, -1)}
    budgets = {l: res[l][1] for l in res}
    print("keyless flow at a level: the oracle's noise budget per level", budgets, "the device's", {l: res[l][0] for l in res})
    lowest = min(l for l in budgets if all(budgets[k] > 0 for k in range(l, L + 1)))
    assert lowest == level, budgets
    assert level == 1 or budgets[level - 1] <= 0, budgets
    assert res[level][0] > 0, res[level][0]
    assert 0 <= res[level][0] - res[level][1] <= 1
    assert (res[level][2] == want).all()
    ks.close()
    return budgets
