"""Parity checks shared by the CPU-emulator suite (numpy memory) and the GPU suite
(torch cuda memory).  Every check compares the C-ABI library with the oracle bit for bit."""
import numpy as np


class HostMem:
    """numpy-backed 'device' memory for the tests-only emulator."""

    def to_dev(self, a):
        return np.ascontiguousarray(a, dtype=np.uint64).copy()

    def empty(self, shape):
        return np.zeros(shape, np.uint64)

    def to_host(self, b):
        return np.array(b, copy=True)


class TorchMem:
    """torch cuda tensors (int64 storage viewed as uint64 words)."""

    def __init__(self, device="cuda:0"):
        import torch
        self.torch, self.device = torch, device

    def to_dev(self, a):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        return self.torch.from_numpy(a.view(np.int64)).to(self.device)

    def empty(self, shape):
        return self.torch.zeros(shape, dtype=self.torch.int64, device=self.device)

    def to_host(self, b):
        self.torch.cuda.synchronize()
        return b.cpu().numpy().view(np.uint64)


def setup_from_primes(orc, logn, q, t, all_galois=False, extra_steps=(), base_steps=(-1, 0, 128)):
    """conftest.Setup for an explicit list of coefficient primes (the last one is the special prime) instead of SEAL's
    CoeffModulus::Create(bit sizes): same seeds, same keys, same PASTA key.  base_steps: the rotation steps that always get
    a key (the PASTA matmul needs -1, 128 and the column swap)."""
    from conftest import Setup
    S = Setup.__new__(Setup)
    S.t, S.logn, S.n = int(t), logn, 1 << logn
    S.q = [int(v) for v in q]
    S.O = O = orc.Oracle(logn, S.q, S.t)
    S.sk = O.keygen_secret(1)
    S.pk = O.keygen_public(S.sk, 2)
    S.rk = O.keygen_relin(S.sk, 3)
    steps = [s for s in base_steps if not (s == 128 and S.n // 2 == 128)] + list(extra_steps)
    elts = [int(e) for e in O.galois_elts_all()] if all_galois else []
    elts = list(dict.fromkeys(elts + [int(O.galois_elt(s)) for s in steps]))
    S.gk = O.keygen_galois(S.sk, elts, 7)
    S.key = np.array([(i * 2654435761 + 12345) % S.t for i in range(256)], dtype=np.uint64)
    S.enc_key = O.encrypt(S.pk, O.pasta_pack_key(S.key), 11)
    return S


def pm_ok(q):
    """The predicate of the product's fill_mod (csrc/hhe_context.cpp), restated: q = 2^b - c with 33 <= b <= 60, c < 2^32 and
    2^b + 2^(64-b) c <= 2q.  Python integers, so nothing here can overflow."""
    q = int(q)
    b = q.bit_length()
    c = (1 << b) - q
    return int(33 <= b <= 60 and c < (1 << 32) and c * ((1 << (64 - b)) + 2) <= (1 << b))


def assert_dispatch(X, q, row_kernel, digit_reduce=None):
    """The context reports, prime by prime, the form this file computes for it, and takes the path the test means to run."""
    logn = X.logn
    for i, qi in enumerate(q):
        assert X.query("pm_ok", i) == pm_ok(qi), (i, qi)
    n2 = logn - logn // 2
    supported = logn >= 12 and 6 <= n2 <= 8
    assert X.query("row_kernel") == int(supported and all(pm_ok(v) for v in q))
    assert X.query("row_kernel") == row_kernel, [pm_ok(v) for v in q]
    qmax, qmin = max(q[:-1]), min(q)
    assert X.query("digit_reduce") == int(qmax // 4 >= qmin)
    if digit_reduce is not None:
        assert X.query("digit_reduce") == digit_reduce


def check_context_constants(X, O):
    for i in range(O.K):
        assert X.query("root", i) == O.query("root", i)
    for i in range(O.L + 1):
        assert X.query("bsk", i) == O.query("bsk", i)
    assert X.query("gamma") == O.query("gamma")
    for s in (-1, 1, 128, -128, 0):
        assert X.query("galois_elt", s) == O.galois_elt(s)
    for j in range(O.L):
        assert X.query("delta", j) == O.query("delta", j)


def check_ntt(X, O, mem, seed=0):
    rng = np.random.default_rng(seed)
    nm = 2 * O.K  # coeff primes + Bsk primes
    polys = np.stack([rng.integers(0, 1 << 40, O.n, dtype=np.uint64) for _ in range(nm + 1)])
    polys[nm] %= O.t
    for i in range(nm):   # residues: a no-op for primes above 2^40, needed for the 33..40-bit primes of the dispatch cases
        polys[i] %= np.uint64(O.q[i] if i < O.K else O.query("bsk", i - O.K))
    ref = np.stack([O.ntt_fwd(i, polys[i]) for i in range(nm)] + [O.ntt_fwd(-1, polys[nm])])
    d = mem.to_dev(polys)
    X.ntt(d, nm + 1, 0, nm + 1, False)
    assert (mem.to_host(d) == ref).all()
    X.ntt(d, nm + 1, 0, nm + 1, True)
    assert (mem.to_host(d) == polys).all()
    # extreme residues: the lazily reduced butterflies (values allowed to grow to 16q between folds) must not wrap 64 bits
    mods = [O.q[i] if i < O.K else O.query("bsk", i - O.K) for i in range(nm)] + [O.t]
    for pattern in ("max", "alt", "one_hot"):
        ext = np.zeros((nm + 1, O.n), np.uint64)
        for i, qi in enumerate(mods):
            if pattern == "max":
                ext[i, :] = qi - 1
            elif pattern == "alt":
                ext[i, ::2] = qi - 1
            else:
                ext[i, O.n - 1] = qi - 1
        ref = np.stack([O.ntt_fwd(i, ext[i]) for i in range(nm)] + [O.ntt_fwd(-1, ext[nm])])
        d = mem.to_dev(ext)
        X.ntt(d, nm + 1, 0, nm + 1, False)
        assert (mem.to_host(d) == ref).all(), pattern
        X.ntt(d, nm + 1, 0, nm + 1, True)
        assert (mem.to_host(d) == ext).all(), pattern


def check_ops(X, S, mem, B=3, seed=0):
    """S: conftest.Setup with keys loaded into X."""
    O = S.O
    n, t = O.n, O.t
    rng = np.random.default_rng(seed)
    cts = np.stack([O.encrypt(S.pk, O.encode(rng.integers(0, t, n)), 10 + b) for b in range(B)])
    d_cts = mem.to_dev(cts)
    out = mem.empty(cts.shape)
    # encode (ragged count)
    vals = np.stack([rng.integers(0, t, 100, dtype=np.uint64) for _ in range(B)])
    d_pl = mem.empty((B, n))
    X.encode(mem.to_dev(vals), B, 100, d_pl)
    pl = mem.to_host(d_pl)
    for b in range(B):
        assert (pl[b] == O.encode(vals[b])).all()
    # add / negate
    rev = cts[::-1].copy()
    X.add(d_cts, mem.to_dev(rev), out, B)
    h = mem.to_host(out)
    for b in range(B):
        assert (h[b] == O.add(cts[b], rev[b])).all()
    X.negate(d_cts, out, B)
    assert (mem.to_host(out)[0] == O.negate(cts[0])).all()
    # add_plain / sub_plain / broadcast
    X.add_plain(d_cts, d_pl, out, B)
    h = mem.to_host(out)
    for b in range(B):
        assert (h[b] == O.add_plain(cts[b], pl[b])).all()
    X.add_plain(d_cts, d_pl, out, B, subtract=True)
    assert (mem.to_host(out)[1] == O.sub_plain(cts[1], pl[1])).all()
    X.add_plain(d_cts, mem.to_dev(pl[0:1]), out, B, bcast=True)
    assert (mem.to_host(out)[B - 1] == O.add_plain(cts[B - 1], pl[0])).all()
    # multiply_plain
    X.multiply_plain(d_cts, d_pl, out, B)
    h = mem.to_host(out)
    for b in range(B):
        assert (h[b] == O.multiply_plain(cts[b], pl[b])).all()
    X.multiply_plain(d_cts, mem.to_dev(pl[1:2]), out, B, bcast=True)
    assert (mem.to_host(out)[B - 1] == O.multiply_plain(cts[B - 1], pl[1])).all()
    # galois / rotations (incl. in place)
    for e, k in zip(S.gk.elts, S.gk.keys):
        X.apply_galois(d_cts, int(e), out, B)
        h = mem.to_host(out)
        for b in range(B):
            assert (h[b] == O.apply_galois(cts[b], int(e), k)).all(), int(e)
    x = mem.to_dev(cts)
    X.rotate_rows(x, -1, x, B)
    assert (mem.to_host(x)[1] == O.rotate_rows(cts[1], -1, S.gk)[0]).all()
    X.rotate_columns(d_cts, out, B)
    assert (mem.to_host(out)[0] == O.rotate_columns(cts[0], S.gk)).all()
    # BEHZ multiply / square / relinearize
    o3 = mem.empty((B, 3, O.L, n))
    X.multiply(d_cts, mem.to_dev(rev), o3, B)
    h3 = mem.to_host(o3)
    for b in range(B):
        assert (h3[b] == O.multiply(cts[b], rev[b])).all()
    X.multiply(d_cts, d_cts, o3, B)
    h3 = mem.to_host(o3)
    assert (h3[1] == O.multiply(cts[1], cts[1])).all()
    X.relinearize(o3, out, B)
    assert (mem.to_host(out)[1] == O.relinearize(h3[1], S.rk)).all()


def check_transcipher(X, S, orc, mem, pt, block_ids=None, check_decrypt=True, oracle_items=None):
    """transcipher the PASTA encryption of pt; compare chosen items with the oracle bit for bit."""
    O = S.O
    cw, ncw = S.sym_blocks(orc, pt)
    nb = cw.shape[0]
    block_ids = list(range(nb)) if block_ids is None else block_ids
    out = mem.empty((nb,) + O.ct_shape)
    X.transcipher(mem.to_dev(S.enc_key), cw, ncw, block_ids, out)
    res = mem.to_host(out)
    for b in (range(nb) if oracle_items is None else oracle_items):
        ref = O.transcipher_block(S.enc_key, S.rk, S.gk, cw[b, :ncw[b]], block_ids[b])
        assert (res[b] == ref).all(), f"block {b} differs from oracle"
        if check_decrypt:
            dec = O.decode(O.decrypt(S.sk, res[b]))[:ncw[b]]
            assert (dec == np.asarray(pt[b * 128:b * 128 + ncw[b]], dtype=np.uint64)).all()
    return res


def check_batched_calls_regrow(make_ctx, S, orc, mem, n_in=37, dim=16, bsgs=(4, 4)):
    """The three batched entry points on ONE context whose internal streams have been used, every grow-only workspace reallocated
    in between: hhe_pasta3_transcipher (use_bsgs = 1), hhe_packed_affine_ks (BSGS handle) and hhe_fc_row_ks (W = 1) with 1 item,
    then 5 (with 2 items per chunk: three chunks on two lanes, the last one ragged), then 1 again.  Every output word equals the
    same call on a fresh context that saw that batch size first; item 0 of every first call equals the oracle.  make_ctx() returns
    a fresh context created under the knobs the caller set (HHE_STREAMS, HHE_CHUNK, HHE_FC_CHUNK); S holds every default Galois
    key plus steps -16k (k = 1..7) and the affine layer's (affine_common.hand_steps)."""
    import affine_common as ac
    O = S.O
    small, large = 1, 5
    pt = np.array([(11 * i + 5) % 256 for i in range(128 * large)], dtype=np.uint64)
    cw, ncw = S.sym_blocks(orc, pt[:128 * large - 30])   # the last block is short
    M, bias = ac.seeded_matrix(S.t, dim, 77)
    cts, _ = ac.inputs(S, dim, large, 7)
    rng = np.random.default_rng(21)
    v, w = rng.integers(0, 4, (large, n_in)), rng.integers(-8, 9, n_in)
    vi = np.stack([O.encrypt(S.pk, O.encode(v[b]), 141 + b) for b in range(large)])
    wc = O.encrypt(S.pk, O.encode(w % S.t), 143)

    def open_ctx():
        X = make_ctx()
        S.load_keys(X)
        ks = X.keyset()   # hhe_fc_row_ks names its key objects
        ks.set_relin(S.rk)
        for e, k in zip(S.gk.elts, S.gk.keys):
            ks.set_galois(int(e), k)
        return X, ks, X.matrix(M, bias=bias, bsgs=bsgs)

    def calls(ctx, B):
        X, ks, mat = ctx
        o_t, o_a, o_f = (mem.empty((B,) + O.ct_shape) for _ in range(3))
        X.transcipher(mem.to_dev(S.enc_key), cw[:B], ncw[:B], list(range(B)), o_t, use_bsgs=True)
        X.packed_affine(mem.to_dev(cts[:B]), mat, o_a, B)
        X.fc_row(mem.to_dev(vi[:B]), mem.to_dev(wc[None]), 1, n_in, o_f, B, rk=ks, gk=ks)
        return [mem.to_host(o) for o in (o_t, o_a, o_f)]

    def close(ctx):
        X, ks, mat = ctx
        mat.close(); ks.close(); X.close()

    fresh = {}
    for B in (small, large):
        ctx = open_ctx()
        fresh[B] = calls(ctx, B)
        close(ctx)
    ctx = open_ctx()
    for B in (small, large, small):
        got = calls(ctx, B)
        for name, g, f in zip(("transcipher", "packed_affine", "fc_row"), got, fresh[B]):
            assert g.shape == f.shape and (g == f).all(), (name, B, "differs from a fresh context", np.argwhere((g != f).reshape(B, -1).any(axis=1)).ravel())
    assert ctx[0].query("fc_fallbacks") == 0
    close(ctx)
    ref_t = O.transcipher_block(S.enc_key, S.rk, S.gk, cw[0, :ncw[0]], 0, use_bsgs=True)
    ref_a = ac.packed_affine_ref(O, S.gk, M, cts[0], bias, bsgs)
    ref_f = O.fc_row(vi[0], wc, S.rk, S.gk, n_in)[0]
    for B in (small, large):
        for name, g, ref in zip(("transcipher", "packed_affine", "fc_row"), fresh[B], (ref_t, ref_a, ref_f)):
            assert (g[0] == ref).all(), (name, B, "item 0 differs from the oracle")


def golden_key(t):
    return np.array([(i * 2654435761 + 12345) % t for i in range(256)], dtype=np.uint64)


def check_plain_cipher_golden(X, orc, mem, golden):
    """Client-side plain PASTA-3 on the device vs the vectors the reference's own pasta_3_plain.cpp produced
    (tests/golden/pasta_plain.json) and vs the oracle for block counters the fixture does not hold."""
    t = X.t
    key = golden_key(t)
    hit = 0
    for c in golden["randomness"]:
        if c["t"] != t:
            continue
        ks = mem.empty((1, 128))
        X.plain_keystream(key, c["block"], 1, ks)
        assert [int(v) for v in mem.to_host(ks)[0]] == c["keystream"]
        hit += 1
    assert hit, "no golden keystream for this modulus"
    # a run of consecutive counters in one launch, each block against the oracle
    nb = 5
    ks = mem.empty((nb, 128))
    X.plain_keystream(key, 3, nb, ks)
    got = mem.to_host(ks)
    for b in range(nb):
        assert (got[b] == orc.pasta_keystream(t, key, 3 + b)).all()
    for e in golden["encrypt"]:
        if e["t"] != t:
            continue
        n = e["n"]
        S = 3  # every record restarts at counter 0: identical ciphertext rows for identical plaintext rows
        pt = np.tile(np.array([(7 * i + 3) % 256 for i in range(n)], dtype=np.uint64), (S, 1))
        d_in, d_out = mem.to_dev(pt), mem.empty((S, n))
        X.plain_crypt(key, d_in, S, n, d_out)
        ct = mem.to_host(d_out)
        for s in range(S):
            assert [int(v) for v in ct[s]] == e["ct"]
        X.plain_crypt(key, d_out, S, n, d_out, decrypt=True)  # in place
        assert (mem.to_host(d_out) == pt).all()


def check_decrypt(X, S, mem, B=3, seed=0):
    """Batched Decryptor::decrypt + BatchEncoder::decode vs the oracle, on fresh and on evaluated ciphertexts."""
    O = S.O
    rng = np.random.default_rng(seed)
    vals = rng.integers(0, O.t, (B, O.n), dtype=np.uint64)
    cts = np.stack([O.encrypt(S.pk, O.encode(vals[b]), 30 + b) for b in range(B)])
    # one evaluated ciphertext (rotation: key-switch noise) so that the rounding path is not trivial
    cts[B - 1] = O.rotate_rows(cts[B - 1], -1, S.gk)[0]
    out = mem.empty((B, O.n))
    X.decrypt(S.sk, mem.to_dev(cts), B, out)
    got = mem.to_host(out)
    for b in range(B):
        assert (got[b] == O.decode(O.decrypt(S.sk, cts[b]))).all()
    assert (got[0] == vals[0]).all()


def check_fc_variants(make_ctx, S, orc, mem, monkeypatch, n_in=37):
    """hhe_fc_row execution variants (per-child digit transforms, shared digits, forced exact fallback, with and without
    leaf sums) all return the oracle's words."""
    O = S.O
    rng = np.random.default_rng(8)
    v, w = rng.integers(0, 4, n_in), rng.integers(-8, 9, n_in)
    wc = O.encrypt(S.pk, O.encode(w), 43)
    B = 3
    vi = np.stack([O.encrypt(S.pk, O.encode(v), 41 + b) for b in range(B)])
    refs = [O.fc_row(vi[b], wc, S.rk, S.gk, n_in)[0] for b in range(B)]
    # (shared digits, leaf sums, items per chunk): chunk 1 -> three chunks round-robin over the internal streams
    # fourth column: leaf key switches per launch (leaves of any nodes whose digit transforms are resident; 1 = one leaf at a time)
    for shared, leafsum, chunk, group in (("1", "1", "40", "4"), ("0", "1", "40", "4"), ("2", "1", "40", "4"), ("1", "0", "40", "4"),
                                          ("0", "0", "40", "4"), ("1", "1", "1", "4"), ("2", "1", "1", "4"), ("0", "1", "2", "4"),
                                          ("1", "1", "40", "1"), ("1", "1", "2", "2"), ("1", "1", "40", "3")):
        monkeypatch.setenv("HHE_FC_LEAFGROUP", group)
        monkeypatch.setenv("HHE_FC_SHARED", shared)
        monkeypatch.setenv("HHE_FC_LEAFSUM", leafsum)
        monkeypatch.setenv("HHE_FC_CHUNK", chunk)
        X = make_ctx()
        S.load_keys(X)
        out = mem.empty((B,) + O.ct_shape)
        X.fc_row(mem.to_dev(vi), mem.to_dev(wc[None]), 1, n_in, out, B, relin_slot=0, default_galois_only=False)
        got = mem.to_host(out)
        for b in range(B):
            assert (got[b] == refs[b]).all(), (shared, leafsum, chunk, group, b)
        assert X.query("fc_fallbacks") == ((B + int(chunk) - 1) // int(chunk) if shared == "2" else 0)
        X.close()


def check_two_layer_chain(X, S, mem, n_in=24, seed=3, w1_vals=None, x_vals=None):
    """BASELINE config 4 shape (FC -> packed_square -> FC, SEAL_Cipher.cpp:547-552 between two sealhelper FC rows):
    ciphertext parity of the whole chain against the oracle's op sequence.  w1_vals / x_vals: first-layer weights (signed
    integers, encoded mod t as the analyst does) and inputs; defaults are small seeded values."""
    O = S.O
    rng = np.random.default_rng(seed)
    x = np.asarray(x_vals if x_vals is not None else rng.integers(0, 4, n_in), dtype=np.int64)
    w1i = np.asarray(w1_vals if w1_vals is not None else rng.integers(0, 4, n_in), dtype=np.int64)
    assert len(x) == n_in and len(w1i) == n_in
    vi = O.encrypt(S.pk, O.encode(x % S.t), 61)
    w1 = O.encrypt(S.pk, O.encode(w1i % S.t), 62)
    w2 = O.encrypt(S.pk, O.encode(rng.integers(0, 4, n_in)), 63)
    ref1, _ = O.fc_row(vi, w1, S.rk, S.gk, n_in)
    ref_sq = O.relinearize(O.multiply(ref1, ref1), S.rk)
    ref2, _ = O.fc_row(ref_sq, w2, S.rk, S.gk, n_in)
    d1, d3, dsq, d2 = mem.empty((1,) + O.ct_shape), mem.empty((1, 3, O.L, O.n)), mem.empty((1,) + O.ct_shape), mem.empty((1,) + O.ct_shape)
    X.fc_row(mem.to_dev(vi[None]), mem.to_dev(w1[None]), 1, n_in, d1, 1, relin_slot=0, default_galois_only=False)
    X.multiply(d1, d1, d3, 1)
    X.relinearize(d3, dsq, 1)
    X.fc_row(dsq, mem.to_dev(w2[None]), 1, n_in, d2, 1, relin_slot=0, default_galois_only=False)
    assert (mem.to_host(d1)[0] == ref1).all()
    assert (mem.to_host(dsq)[0] == ref_sq).all()
    assert (mem.to_host(d2)[0] == ref2).all()
    if O.noise_budget(S.sk, ref1, 8) > 0:  # the first layer decrypts to the plain integer dot product (FC == matMul, hhe_pktnn_examples.cpp:692-699)
        got = int(O.decode(O.decrypt(S.sk, mem.to_host(d1)[0]))[n_in - 1])
        assert got == int(np.dot(x, w1i)) % S.t


def check_key_sets(X, S, orc, mem, threads=True):
    """Key objects with identity (CSP.cpp:238-242, 271-278, 306, 312-316; Analyst.cpp:62-94): two GaloisKeys objects and two
    RelinKeys objects under ONE secret key, made with different randomness.  A = every default element (what
    create_galois_keys() without arguments makes), B = {0, -1, 128, -128, -256, -384}.  Every call must produce the words the
    oracle produces WITH THE SET THE CALL NAMES: rotate_rows(-384) NAF-decomposes over A and is one key switch with B; flatten
    differs between A and B; the FC uses (rk2, A); nothing uploaded into one set is seen through another."""
    O = S.O
    n = O.n
    eltsA = list(dict.fromkeys(int(e) for e in O.galois_elts_all()))
    stepsB = [0, -1, 128, -128, -256, -384]
    eltsB = list(dict.fromkeys(int(O.galois_elt(s)) for s in stepsB))
    gkA = O.keygen_galois(S.sk, eltsA, 101)
    gkB = O.keygen_galois(S.sk, eltsB, 202)   # same elements where they overlap, different randomness: different words
    rk2 = O.keygen_relin(S.sk, 303)
    A, Bs, R2 = X.keyset(), X.keyset(), X.keyset()
    for e, k in zip(gkA.elts, gkA.keys):
        A.set_galois(int(e), k)
    for e, k in zip(gkB.elts, gkB.keys):
        Bs.set_galois(int(e), k)
    R2.set_relin(rk2)
    A.set_relin(S.rk)  # a set may hold both kinds
    assert A.has_galois(O.galois_elt(-128)) and Bs.has_galois(O.galois_elt(-384)) and not A.has_galois(O.galois_elt(-384))
    assert R2.has_relin() and not Bs.has_relin()
    rng = np.random.default_rng(77)
    cts = np.stack([O.encrypt(S.pk, O.encode(rng.integers(0, O.t, n)), 70 + b) for b in range(2)])
    d, out = mem.to_dev(cts), mem.empty(cts.shape)
    # rotate_rows(-384): NAF over A ({128, -512} at N = 2^15; the +-N/2 term is skipped when it is a whole row), direct with B
    refA = [O.rotate_rows(cts[b], -384, gkA) for b in range(2)]
    refB = [O.rotate_rows(cts[b], -384, gkB) for b in range(2)]
    assert n >= 2048 and refB[0][1] == 1 and refA[0][1] == 2   # (at N = 1024 a row has 512 slots and -384 is the element of +128)
    X.rotate_rows(d, -384, out, 2, gk=A)
    hA = mem.to_host(out)
    X.rotate_rows(d, -384, out, 2, gk=Bs)
    hB = mem.to_host(out)
    for b in range(2):
        assert (hA[b] == refA[b][0]).all() and (hB[b] == refB[b][0]).all()
    assert not (hA[0] == hB[0]).all()
    # an element both sets hold: same rotation, different key words -> different ciphertext words, each equal to its oracle
    for ks, gk in ((A, gkA), (Bs, gkB)):
        X.rotate_rows(d, -128, out, 2, gk=ks)
        assert (mem.to_host(out)[1] == O.rotate_rows(cts[1], -128, gk)[0]).all()
        X.rotate_columns(d, out, 2, gk=ks)
        assert (mem.to_host(out)[0] == O.rotate_columns(cts[0], gk)).all()
    # the default set is empty: the un-named call fails, and a step neither direct nor NAF-reachable in B fails with B
    for kw in ({}, {"gk": Bs}):
        try:
            X.rotate_rows(d, -5, out, 2, **kw)
            raise AssertionError("rotation without its key must fail")
        except RuntimeError as e:
            assert "Galois key not present" in str(e)
    # flatten(in, out, galois_keys): 3 blocks, steps -128, -256 -- direct in B, direct in A as well but with A's words
    blocks = np.stack([O.encrypt(S.pk, O.encode(rng.integers(0, O.t, 128)), 80 + i) for i in range(3)])
    fo = mem.empty((1,) + O.ct_shape)
    X.flatten(mem.to_dev(blocks[None]), 3, fo, 1, gk=A)
    fA = mem.to_host(fo)[0]
    X.flatten(mem.to_dev(blocks[None]), 3, fo, 1, gk=Bs)
    fB = mem.to_host(fo)[0]
    assert (fA == O.flatten(blocks, gkA)).all() and (fB == O.flatten(blocks, gkB)).all() and not (fA == fB).all()
    # relinearize / FC with the objects the CSP names: csp rk (R2) and the analyst's default Galois keys (A)
    o3 = mem.empty((2, 3) + O.ct_shape[1:])
    X.multiply(d, d, o3, 2)
    X.relinearize(o3, out, 2, rk=R2)
    assert (mem.to_host(out)[0] == O.relinearize(O.multiply(cts[0], cts[0]), rk2)).all()
    X.relinearize(o3, out, 2, rk=A)
    assert (mem.to_host(out)[0] == O.relinearize(O.multiply(cts[0], cts[0]), S.rk)).all()
    n_in = 45
    v, w = rng.integers(0, 4, n_in), rng.integers(-8, 9, n_in)
    vi, wc = O.encrypt(S.pk, O.encode(v), 91), O.encrypt(S.pk, O.encode(w % O.t), 92)
    X.fc_row(mem.to_dev(vi[None]), mem.to_dev(wc[None]), 1, n_in, fo, 1, rk=R2, gk=A)
    ref_fc, _ = O.fc_row(vi, wc, rk2, gkA, n_in)
    assert (mem.to_host(fo)[0] == ref_fc).all()
    if not threads:
        return
    # two request handlers at once (CSPRPC.cpp:201-203), each naming its own set on the shared context
    import threading
    res, errs = {}, []

    def work(name, ks, step):
        try:
            o = mem.empty(cts.shape)
            for _ in range(3):
                X.rotate_rows(mem.to_dev(cts), step, o, 2, gk=ks)
            res[name] = mem.to_host(o)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=work, args=("A", A, -128)), threading.Thread(target=work, args=("B", Bs, -128))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert (res["A"][0] == O.rotate_rows(cts[0], -128, gkA)[0]).all() and (res["B"][0] == O.rotate_rows(cts[0], -128, gkB)[0]).all()
    for ks in (A, Bs, R2):
        ks.close()


def check_hot_path(X, S, orc, mem, make_ctx=None, monkeypatch=None, n_in=9, B=2, seed=0, ntt=True):
    """Everything the hot path is made of, on ONE parameter set, word for word against the oracle: context constants, the
    transforms (random and extreme residues), every evaluator op (rotations by every key of S, BEHZ multiply, relinearize),
    a ragged two-block transciphering (blocks 0 and 2 of a 300-word record: 128 and 44 words), BaseCSP::decompose of that
    record (3 transcipherings + mask + flatten; S must hold the keys of steps -128 and -256) and, with make_ctx, the FC's
    execution variants.  S: keys already loaded into X.  Noise budgets may be exhausted at the moduli this is used with:
    words are compared, never decryptions."""
    O = S.O
    check_context_constants(X, O)
    if ntt:
        check_ntt(X, O, mem, seed=seed)
    check_ops(X, S, mem, B=B, seed=seed)
    pt = np.array([(7 * i + 3 + seed) % 256 for i in range(300)], dtype=np.uint64)
    cw, ncw = S.sym_blocks(orc, pt)
    assert list(ncw) == [128, 128, 44]
    blocks = [O.transcipher_block(S.enc_key, S.rk, S.gk, cw[b, :ncw[b]], b) for b in range(3)]
    out = mem.empty((2,) + O.ct_shape)
    X.transcipher(mem.to_dev(S.enc_key), cw[[0, 2]], ncw[[0, 2]], [0, 2], out)
    res = mem.to_host(out)
    assert (res[0] == blocks[0]).all(), "block 0 differs from the oracle"
    assert (res[1] == blocks[2]).all(), "ragged block 2 differs from the oracle"
    rec = orc.pasta_encrypt(S.t, S.key, pt)
    flat = mem.empty((1,) + O.ct_shape)
    X.decompose(mem.to_dev(S.enc_key), rec[None], flat, mask_last=True)
    masked = list(blocks)
    masked[2] = O.mask(blocks[2], np.ones(44, np.uint64))
    assert (mem.to_host(flat)[0] == O.flatten(np.stack(masked), S.gk)).all(), "decompose differs from the oracle"
    if make_ctx is not None:
        check_fc_variants(make_ctx, S, orc, mem, monkeypatch, n_in=n_in)


def adversarial_words(S, size, pattern):
    """a size-`size` 'ciphertext' with every word at q_j - 1 ('alt': alternating with 0)"""
    a = np.zeros((size, S.O.L, S.O.n), np.uint64)
    for j in range(S.O.L):
        if pattern == "alt":
            a[:, j, ::2] = S.q[j] - 1
        else:
            a[:, j, :] = S.q[j] - 1
    return a


def adversarial_keys(S, orc, pattern):
    """(relin key, Galois keys) of S, or -- 'max_keys' -- keys whose every word is q_j - 1"""
    if pattern != "max_keys":
        return S.rk, S.gk
    rk = np.zeros_like(S.rk)
    for j in range(S.O.K):
        rk[:, :, j, :] = S.q[j] - 1
    return rk, orc.GaloisKeys(S.gk.elts, np.stack([rk] * len(S.gk.elts)))


def check_keyswitch_adversarial(X, S, orc, mem, pattern, n_in=11):
    """The generic key switch (rotations: both sums inverse-transformed, mod-down in the store of the last pass), BEHZ multiply,
    relinearize and -- pattern 'max' -- one FC row (shared digits, leaf sums) on worst-case residues: a size-2 and a size-3
    'ciphertext' with every word at q_j - 1 (or alternating with 0) and, for 'max_keys', every key word at q_j - 1.  Nothing here
    is a valid encryption; the oracle's exact 128-bit arithmetic defines the expected words, as in check_matmul_adversarial.
    S needs the keys of steps -1, 0 and, for the FC, every default Galois element."""
    O = S.O
    ct2, ct3 = adversarial_words(S, 2, pattern), adversarial_words(S, 3, pattern)
    rk, gk = adversarial_keys(S, orc, pattern)
    ks = X.keyset()
    ks.set_relin(rk)
    for e, k in zip(gk.elts, gk.keys):
        ks.set_galois(int(e), k)
    d2, out = mem.to_dev(ct2[None]), mem.empty((1,) + O.ct_shape)
    X.rotate_rows(d2, -1, out, 1, gk=ks)
    ref, nks = O.rotate_rows(ct2, -1, gk)
    assert nks == 1 and (mem.to_host(out)[0] == ref).all(), (pattern, "rotate_rows")
    X.rotate_columns(d2, out, 1, gk=ks)
    assert (mem.to_host(out)[0] == O.rotate_columns(ct2, gk)).all(), (pattern, "rotate_columns")
    o3 = mem.empty((1, 3, O.L, O.n))
    X.multiply(d2, d2, o3, 1)
    assert (mem.to_host(o3)[0] == O.multiply(ct2, ct2)).all(), (pattern, "multiply")
    X.relinearize(mem.to_dev(ct3[None]), out, 1, rk=ks)
    assert (mem.to_host(out)[0] == O.relinearize(ct3, rk)).all(), (pattern, "relinearize")
    if pattern == "max":
        X.fc_row(d2, d2, 1, n_in, out, 1, rk=ks, gk=ks)
        assert (mem.to_host(out)[0] == O.fc_row(ct2, ct2, rk, gk, n_in)[0]).all(), (pattern, "fc_row")
    ks.close()


T16 = 65537
T33 = 8088322049   # the reference's plain modulus at N = 65536 (65537 cannot batch there)
NEAR_3_2_58 = [864691128455086081, 864691128454914049, 864691128454594561, 864691128454438913]  # 60-bit primes = 1 mod 8192, none pm_ok


def dispatch_case(orc, api, lib, name):
    """Parameter sets chosen for the kernels they select (dispatch matrix):
    (logn, coefficient primes, t, expected row_kernel, expected digit_reduce).  A-G lack the pseudo-Mersenne form on at least one
    prime and take the separate-kernel path at full tiles; H and I have the LARGEST c = 2^b - q (with q = 1 mod 2N) that pm_fold's
    guarantee still admits, where its bound is tightest."""
    cm = orc.coeff_modulus_create
    if name == "A":   # BFVDefault(4096): what SEALZpCipher::create_context(4096) picks, 36 + 36 + 37 bits
        return 12, api.bfv_default_coeff_modulus(4096, lib), T16, 0, 0
    if name == "B":   # 40-bit primes at N = 8192, L = 5: all non-pm
        return 13, cm(8192, [40] * 6), T16, 0, 0
    if name == "C":   # 256-point rows without the row kernel
        return 15, cm(32768, [36] * 4), T16, 0, 0
    if name == "D":
        return 16, cm(65536, [40] * 3), T33, 0, 0
    if name == "E":   # caller-supplied 60-bit primes that do not hug a power of two
        return 12, NEAR_3_2_58, T16, 0, 0
    if name == "F":   # pm data primes, non-pm special prime.  Digits come from the DATA primes only (50 bits, below 4 q_J for
        return 12, cm(4096, [50, 50]) + NEAR_3_2_58[:1], T16, 0, 0   # every J): no digit reduction is needed or done
    if name == "F2":  # the same mix with the 60-bit non-pm prime among the data primes: its digits are reduced for the 50-bit primes
        return 12, [cm(4096, [50])[0], NEAR_3_2_58[0], NEAR_3_2_58[1]], T16, 0, 1
    if name == "G":   # one non-pm data prime, and q_I >= 4 q_J
        return 12, cm(4096, [36, 50, 50, 50]), T16, 0, 1
    if name == "H":
        return 12, [(1 << 42) - c for c in (802815, 974847, 999423)] + [(1 << 43) - 4186111], T16, 1, 0
    if name == "I":
        return 15, [(1 << 44) - c for c in (13041663, 13631487, 14352383)] + [(1 << 45) - 65798143], T16, 1, 0
    raise KeyError(name)


def dispatch_setup(orc, api, lib, name, all_galois=True, extra_steps=(-128, -256)):
    """(Setup, context factory) of a dispatch case; every context the factory returns has asserted its path"""
    logn, q, t, row_kernel, digit_reduce = dispatch_case(orc, api, lib, name)
    S = setup_from_primes(orc, logn, q, t, all_galois=all_galois, extra_steps=extra_steps)

    def make_ctx():
        X = api.Context(logn, q, t, lib=lib)
        assert_dispatch(X, q, row_kernel, digit_reduce)
        return X
    return S, make_ctx


def check_matmul_adversarial(X, S, orc, mem, pattern):
    """The matmul loop on worst-case residues (the lazy ranges are tightest at 60-bit primes, 16q ~ 2^64): the 'ciphertext' the
    loop starts from, the symmetric words and -- for 'max_keys' -- every key-switch key word sit at q_j - 1 (or alternate with
    0).  Nothing here is a valid encryption; the oracle's exact arithmetic defines the expected words all the same."""
    O = S.O
    enc = np.zeros(O.ct_shape, np.uint64)
    for j in range(O.L):
        if pattern == "alt":
            enc[:, j, ::2] = S.q[j] - 1
        else:
            enc[:, j, :] = S.q[j] - 1
    rk, gk = S.rk, S.gk
    if pattern == "max_keys":
        rk = np.zeros_like(S.rk)
        for j in range(O.K):
            rk[:, :, j, :] = S.q[j] - 1
        gk = orc.GaloisKeys(S.gk.elts, np.stack([rk] * len(S.gk.elts)))
    ks = X.keyset()
    ks.set_relin(rk)
    for e, k in zip(gk.elts, gk.keys):
        ks.set_galois(int(e), k)
    cw = np.full((1, 128), S.t - 1, np.uint64)
    out = mem.empty((1,) + O.ct_shape)
    X.transcipher(mem.to_dev(enc), cw, [128], [0], out, rk=ks, gk=ks)
    assert (mem.to_host(out)[0] == O.transcipher_block(enc, rk, gk, cw[0], 0)).all(), pattern
    ks.close()


# ---- the FC row at the shapes where it is used (tests/test_fc_shapes.py, tests/golden/make_fc784.py) ----
BFV_DEFAULT_16384 = [281474976546817, 281474976317441, 281474975662081, 562949952798721, 562949952700417,
                     562949952274433, 562949951979521, 562949951881217, 562949951619073]  # CoeffModulus::BFVDefault(16384), SURVEY A.10

CSUM_MAX = 2000   # FcWalk::CSUM_MAX (csrc/hhe_api.cpp)


def galois_elt_py(n, step):
    """GaloisTool::get_elt_from_step (seal/util/galois.cpp), restated: 3^step mod 2N for a left rotation by `step` of a row of
    N/2 slots, a right rotation by s being the left rotation by N/2 - s; step 0 is the column swap 2N - 1."""
    m, row = 2 * n, n // 2
    if step == 0:
        return m - 1
    assert abs(step) < row
    return pow(3, step if step > 0 else row - (-step), m)


def default_galois_elts_py(n):
    """what GaloisKeys created without arguments hold (GaloisTool::get_elts_all): 3^(2^k), their inverses and the column swap"""
    m, elts, g, gi = 2 * n, [2 * n - 1], 3, pow(3, -1, 2 * n)
    for _ in range(n.bit_length() - 2):
        elts += [g, gi]
        g, gi = g * g % m, gi * gi % m
    return list(dict.fromkeys(elts))


class FcTrie:
    """Model of the rotation trie of one hhe_fc_row chunk, built by the rule of fc_build_trie (csrc/hhe_api.cpp) and nothing else of
    the library: for i = 1 .. n_in-1, step -i is ONE term [-i] if the key set holds its element and (i is a power of two, or the
    call sees the whole set: hhe_fc_row_ks, or default_galois_only = 0); otherwise its terms are naf(-i) without those equal to
    +-N/2.  Node 0 is the root (the relinearized product); term[k] / parent[k] / kids[k] / mult[k] describe node k, mult = how many
    steps end there.  A leaf is a node without children that ends exactly one step."""

    def __init__(self, orc, n, n_in, key_elts, whole_set):
        self.n, self.n_in = n, n_in
        keys = set(int(e) for e in key_elts)
        self.term, self.parent, self.kids, self.mult, self.depth = [0], [-1], [[]], [0], [0]
        for i in range(1, n_in):
            if galois_elt_py(n, -i) in keys and (i & (i - 1) == 0 or whole_set):
                terms = [-i]
            else:
                terms = [t for t in orc.naf(-i) if abs(t) != n // 2]
            node = 0
            for t in terms:
                assert galois_elt_py(n, t) in keys, ("Galois key not present", i, t)
                nxt = next((k for k in self.kids[node] if self.term[k] == t), -1)
                if nxt < 0:
                    nxt = len(self.term)
                    self.term.append(t); self.parent.append(node); self.kids.append([]); self.mult.append(0)
                    self.depth.append(self.depth[node] + 1)
                    self.kids[node].append(nxt)
                node = nxt
            self.mult[node] += 1
        assert self.mult[0] == 0 and max(self.mult) <= 1   # distinct steps have distinct term sequences
        self.nodes = len(self.term) - 1                     # key switches of the trie: every node but the root
        self.leaf = [k > 0 and not self.kids[k] and self.mult[k] == 1 for k in range(len(self.term))]
        self.leaves = sum(self.leaf)
        self.elt = [0] + [galois_elt_py(n, t) for t in self.term[1:]]
        # leaves per Galois element of their last term.  Two different terms can name one element: step -(N/2 - 2^k) and step +2^k
        self.leaves_per_elt = {}
        for k in range(1, len(self.term)):
            if self.leaf[k]:
                self.leaves_per_elt[self.elt[k]] = self.leaves_per_elt.get(self.elt[k], 0) + 1
        self.closes, self.closed_sums = self._closes()

    def _closes(self):
        """c1 sums closed in one chunk, by the rule of FcWalk::csum_leaf / fc_dfs_shared: the walk visits a node's leaf children
        first (in the order they were created), then descends into the others; a leaf joins the sum of its element, which is closed
        BEFORE the leaf is added once it holds CSUM_MAX terms, and every sum that holds any term is closed once at the end.
        The wrap byte: a term is below q < 2^60, so CSUM_MAX = 2000 < 2^11 terms stay below 2^71 and wrap the 64-bit word at most
        2000 q / 2^64 < 125 times (about half that with random residues): a byte holds it.  No open sum may exceed CSUM_MAX terms."""
        count, closed = {}, []
        stack = [0]
        while stack:
            node = stack.pop()
            for k in self.kids[node]:
                if self.leaf[k]:
                    e = self.elt[k]
                    if count.get(e, 0) >= CSUM_MAX:
                        closed.append((e, count[e]))
                        count[e] = 0
                    count[e] = count.get(e, 0) + 1
                    assert count[e] <= CSUM_MAX
            stack.extend(k for k in reversed(self.kids[node]) if not self.leaf[k])
        closed += [(e, c) for e, c in count.items() if c]
        return len(closed), closed

    def leaves_per_step(self, steps):
        """{step: leaves whose last term has the element of `step`}, and nothing left over"""
        got = {s: self.leaves_per_elt.get(galois_elt_py(self.n, s), 0) for s in steps}
        assert sum(got.values()) == self.leaves, (got, self.leaves_per_elt)
        return got


FC_SHAPES = {
    # the benchmarked shape (bench.py MnistFlow: N = 2^15, 4 x 60 bits, 784 inputs): 5 items over 2 weight rows
    "fc784_n32768": dict(logn=15, bits=[60] * 4, n_in=784, B=5, W=2, seed=784),
    # the deployed shape: the only parameter set the reference ships, and the only one of the three that decrypts
    "fc784_n16384": dict(logn=14, primes=BFV_DEFAULT_16384, n_in=784, B=2, W=1, seed=785),
    # the widest row the ABI admits at N = 2^14: one element collects 2731 leaves, more than CSUM_MAX
    "fc8192_n16384": dict(logn=14, bits=[60] * 3, n_in=8192, B=1, W=1, seed=8192),
}


def fc_shape_setup(orc, name):
    """keys of an FC_SHAPES case: Setup seeds (sk 1, pk 2, rk 3, gk 7), Galois keys = exactly what create_galois_keys() without
    arguments makes (steps -1, 0 and 128 are among them)"""
    p = FC_SHAPES[name]
    if "primes" in p:
        S = setup_from_primes(orc, p["logn"], p["primes"], T16, all_galois=True)
    else:
        from conftest import Setup
        S = Setup(orc, p["logn"], p["bits"], all_galois=True)
    assert sorted(int(e) for e in S.gk.elts) == sorted(int(e) for e in set(S.O.galois_elts_all()))
    assert sorted(int(e) for e in S.gk.elts) == sorted(default_galois_elts_py(S.n))
    return S


def fc_shape_inputs(S, name, items=None):
    """(v [B][n_in] in [0,4), w [W][n_in] in [-8,9), their encryptions): default_rng(seed), encrypt seeds 100 + b and 200 + r.
    items: encrypt these items only (the others stay zero words and must not be used)."""
    p = FC_SHAPES[name]
    O = S.O
    rng = np.random.default_rng(p["seed"])
    v = rng.integers(0, 4, (p["B"], p["n_in"]))
    w = rng.integers(-8, 9, (p["W"], p["n_in"]))
    vi = np.zeros((p["B"],) + O.ct_shape, np.uint64)
    for b in (range(p["B"]) if items is None else items):
        vi[b] = O.encrypt(S.pk, O.encode(v[b]), 100 + b)
    wc = np.stack([O.encrypt(S.pk, O.encode(w[r] % S.t), 200 + r) for r in range(p["W"])])
    return v, w, vi, wc


def limb_hashes(ct):
    """SHA-256 per (polynomial, limb) of a ciphertext's words: a mismatch names the limb"""
    import hashlib
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    return [[hashlib.sha256(ct[p, j].tobytes()).hexdigest() for j in range(ct.shape[1])] for p in range(ct.shape[0])]


def assert_limb_hashes(got, want, what):
    h = limb_hashes(got)
    bad = [(p, j) for p in range(len(want)) for j in range(len(want[p])) if h[p][j] != want[p][j]]
    assert len(h) == len(want) and len(h[0]) == len(want[0]) and not bad, (what, "(polynomial, limb) that differ from the oracle:", bad)


# ---- real zero coefficients: the exactness fallback of the shared digits (csrc/hhe_api.cpp, "shared digits") ----
# (logn, prime bit sizes, n_in, B, expected digit_reduce, what the case reaches).  Primes this small make zero coefficients
# of c1 a matter of course (N L nodes / q per item is of order one); none of these contexts runs the fused row kernels.
ZERO_CASES = {
    "n1024_18x4": (10, [18] * 4, 60, 8, 0, "single-tile transform"),
    "n1024_17_20_20": (10, [17, 20, 20], 60, 8, 1, "digit_reduce == 1"),
    "n1024_19x6": (10, [19] * 6, 60, 8, 0, "L = 5: no leaf groups, no c1 sums"),
    "n4096_19x3": (12, [19] * 3, 30, 10, 0, "two-pass transform, row_kernel == 0"),
    "n8192_20x3": (13, [20] * 3, 20, 8, 0, "the same with larger tiles"),
}
_zero_cache = {}


def zero_case(orc, name):
    """(Setup, n_in, vi [B], wc, oracle rows [B], zeros) of a ZERO_CASES entry; inputs as in check_fc_variants (default_rng(8), v in
    [0,4), w in [-8,9) mod t, encrypt seeds 41 + b and 43).  zeros is the PREDICTION, made from the oracle alone: a list of (item,
    depth, limb) for every limb of c1 that holds a 0 in a trie node WITH children (the root, depth 0, included) -- the nodes whose
    digit transforms the children share, where a flipped 0 stays 0 instead of becoming q_I.  Every node is computed with
    O.apply_galois from O.relinearize(O.multiply(vi, w), rk) along the model's trie."""
    if name in _zero_cache:
        return _zero_cache[name]
    from conftest import Setup
    logn, bits, n_in, B, _, _ = ZERO_CASES[name]
    S = Setup(orc, logn, bits, all_galois=True)
    O = S.O
    rng = np.random.default_rng(8)
    v, w = rng.integers(0, 4, n_in), rng.integers(-8, 9, n_in)
    wc = O.encrypt(S.pk, O.encode(w), 43)
    vi = np.stack([O.encrypt(S.pk, O.encode(v), 41 + b) for b in range(B)])
    refs = [O.fc_row(vi[b], wc, S.rk, S.gk, n_in)[0] for b in range(B)]
    trie = FcTrie(orc, S.n, n_in, S.gk.elts, whole_set=True)
    key = {int(e): S.gk.keys[i] for i, e in enumerate(S.gk.elts)}
    zeros = []
    for b in range(B):
        cts = {0: O.relinearize(O.multiply(vi[b], wc), S.rk)}
        for k in range(len(trie.term)):   # a node's index is larger than its parent's
            if not trie.kids[k]:
                continue
            if k:
                cts[k] = O.apply_galois(cts[trie.parent[k]], trie.elt[k], key[trie.elt[k]])
            zeros += [(b, trie.depth[k], j) for j in range(O.L) if (cts[k][1, j] == 0).any()]
    _zero_cache[name] = (S, n_in, vi, wc, refs, zeros)
    return _zero_cache[name]


def assert_zero_cases_valid(orc, name):
    """The conditions under which these cases test anything, asserted on the prediction before the library is looked at: the case
    has an item that must fall back and one that must not; over all cases there is a zero below the root and one outside limb 0."""
    allz = {c: zero_case(orc, c)[5] for c in ZERO_CASES}
    assert any(d > 0 for z in allz.values() for _, d, _ in z), "no zero in a node below the root: choose other seeds or primes"
    assert any(j > 0 for z in allz.values() for _, _, j in z), "no zero outside limb 0: choose other seeds or primes"
    items = sorted(set(b for b, _, _ in allz[name]))
    assert 0 < len(items) < ZERO_CASES[name][3], (name, items)
    return items


def check_fc_real_zeros(make_ctx, orc, mem, monkeypatch, name):
    """A zero coefficient of c1 in a node whose digits are shared is DETECTED -- for exactly the items the oracle-side walk predicts,
    in whatever limb and node -- and the recomputed chunk returns the oracle's words.  fc_fallbacks counts recomputed chunks: with one
    item per chunk it equals the number of predicted items exactly (a spurious fallback is a performance bug the counter exists to
    show), with two per chunk the number of chunks that hold one, and without shared digits it is 0.
    make_ctx(q, t, digit_reduce) returns a fresh context that has asserted its dispatch; the knobs are read at creation."""
    items = assert_zero_cases_valid(orc, name)
    S, n_in, vi, wc, refs, zeros = zero_case(orc, name)
    logn, bits, _, B, digit_reduce, _ = ZERO_CASES[name]
    O = S.O

    def run(expect, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        X = make_ctx(logn, S.q, S.t, digit_reduce)
        for k in env:
            monkeypatch.delenv(k)
        S.load_keys(X)
        out = mem.empty((B,) + O.ct_shape)
        X.fc_row(mem.to_dev(vi), mem.to_dev(wc[None]), 1, n_in, out, B, relin_slot=0, default_galois_only=False)
        got = mem.to_host(out)
        for b in range(B):
            assert (got[b] == refs[b]).all(), (name, env, "item", b, "predicted to fall back:", items, "zeros (item, depth, limb):", zeros)
        assert X.query("fc_fallbacks") == expect, (name, env, X.query("fc_fallbacks"), expect, items)
        X.close()

    # the c1-sum path negates an integer sum, where a flipped 0 matters in the same way: every leaf scheme on the same inputs
    for csum in (1, 0):
        for leafsum in (1, 0):
            for group in (4, 1):
                run(len(items), HHE_FC_CHUNK=1, HHE_FC_CSUM=csum, HHE_FC_LEAFSUM=leafsum, HHE_FC_LEAFGROUP=group)
    run(len(set(b // 2 for b in items)), HHE_FC_CHUNK=2)
    run(0, HHE_FC_CHUNK=1, HHE_FC_SHARED=0)


def check_fc_transparent_row_kernel(make_ctx, orc, mem, monkeypatch):
    """Zero detection on the path of the fused row kernels (ks_perm_row_kernel, c0hat, the digit load of the strided first pass):
    N = 4096, 3 x 60-bit primes, n_in = 9, three items over three weight rows in one chunk, item 0 the product of two TRANSPARENT
    ciphertexts (c1 = 0 in vi[0] and in w[0], c0 uniform words below their primes): its c1 is 0 in every node of the trie.
    This pins that the digit loads of that path raise the flag at all, and that the recomputed chunk is right for the ordinary items
    as well.  It does not pin a single isolated zero there: those kernels need pseudo-Mersenne primes of 33 bits and more, where a
    zero coefficient of a real ciphertext has probability below 10^-4 per row, and a ciphertext cannot be crafted to have one zero
    coefficient in c1 after BEHZ multiply and relinearize without inverting them."""
    from conftest import Setup
    S = Setup(orc, 12, [60] * 3, all_galois=True)
    O = S.O
    n_in, B = 9, 3
    rng = np.random.default_rng(9)
    v, w = rng.integers(0, 4, (B, n_in)), rng.integers(-8, 9, (B, n_in))
    vi = np.stack([O.encrypt(S.pk, O.encode(v[b]), 41 + b) for b in range(B)])
    wc = np.stack([O.encrypt(S.pk, O.encode(w[b]), 51 + b) for b in range(B)])
    for ct in (vi, wc):
        ct[0, 1] = 0
        for j in range(O.L):
            ct[0, 0, j] = rng.integers(0, S.q[j], O.n, dtype=np.uint64)
    refs = [O.fc_row(vi[b], wc[b], S.rk, S.gk, n_in)[0] for b in range(B)]
    # on the oracle, not assumed: item 0's c1 is 0 in the root and in every node with children, its c0 is not
    trie = FcTrie(orc, S.n, n_in, S.gk.elts, whole_set=True)
    key = {int(e): S.gk.keys[i] for i, e in enumerate(S.gk.elts)}
    cts = {0: O.relinearize(O.multiply(vi[0], wc[0]), S.rk)}
    assert any(trie.kids[k] for k in range(1, len(trie.term))), "the trie has no inner node below the root"
    for k in range(len(trie.term)):
        if k:
            cts[k] = O.apply_galois(cts[trie.parent[k]], trie.elt[k], key[trie.elt[k]])
        assert not cts[k][1].any() and cts[k][0].any(), k
    for b in (1, 2):
        assert (O.relinearize(O.multiply(vi[b], wc[b]), S.rk)[1] != 0).all()
    monkeypatch.setenv("HHE_FC_CHUNK", "1")   # rounded up to the three weight rows: one chunk
    X = make_ctx(12, S.q, S.t, 0)
    monkeypatch.delenv("HHE_FC_CHUNK")
    assert X.query("row_kernel") == 1
    S.load_keys(X)
    out = mem.empty((B,) + O.ct_shape)
    X.fc_row(mem.to_dev(vi), mem.to_dev(wc), B, n_in, out, B, relin_slot=0, default_galois_only=False)
    got = mem.to_host(out)
    for b in range(B):
        assert (got[b] == refs[b]).all(), b
    assert X.query("fc_fallbacks") == 1
    X.close()
