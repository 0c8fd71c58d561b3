"""Checker of the packed encrypted FC layer (hhe_enc_matrix_create / hhe_fc_packed_ks): the definition of include/hhe_gfx950.h composed
from the oracle's encode, encrypt, rotate_rows, multiply, add and relinearize alone, and a second truth in plain Python integers.
Shared by the emulator suite (numpy memory) and the GPU suite (torch memory): every comparison of ciphertexts is exact equality of
words, every comparison of slots exact equality of integers."""
import numpy as np

import parity_common as pc

T = 65537

# rows, cols, (r, c), Galois key switches per item at N = 1024
SHAPES = [
    (3, 5, (4, 8), 5),       # base case
    (1, 8, (1, 8), 4),       # r = 1: no chain, the tail sum alone
    (4, 4, (4, 4), 4),       # r == c: no tail
    (2, 512, (2, 512), 9),   # 2c == N: no preparation
    (5, 256, (8, 256), 13),  # 4c == N: the largest c that needs the preparation
    (8, 3, (8, 8), 8),       # rows > cols
]


def pow2_ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def hand_shape(n, rows, cols):
    """(r, c): powers of two, c >= r; the slot rule of SEAL_Cipher.cpp:192-193 with c for the dimension"""
    r = pow2_ceil(rows)
    c = max(pow2_ceil(cols), r)
    if 2 * c != n and 4 * c > n:
        raise RuntimeError("too little slots for matmul implementation!")
    return r, c


def hand_steps(n, rows, cols):
    """-c unless the row is full, +1 when r > 1, then r, 2r, .. below c"""
    r, c = hand_shape(n, rows, cols)
    steps = ([] if 2 * c == n else [-c]) + ([1] if r > 1 else [])
    s = r
    while s < c:
        steps.append(s)
        s *= 2
    return steps


def hand_key_switches(n, rows, cols):
    r, c = hand_shape(n, rows, cols)
    return (0 if 2 * c == n else 1) + (r - 1) + (c // r).bit_length() - 1


def hand_diagonals(M, rows, cols):
    """d_i[j] = M[j mod r][(j + i) mod c] of the matrix zero-padded to r x c, i < r, j < c"""
    r = pow2_ceil(rows)
    c = max(pow2_ceil(cols), r)
    P = [[int(M[i][j]) if i < rows and j < cols else 0 for j in range(c)] for i in range(r)]
    return [[P[j % r][(j + i) % c] for j in range(c)] for i in range(r)]


def seeded_matrix(t, rows, cols, seed):
    """entries in [0, t) from a fixed seed"""
    return np.random.default_rng(seed).integers(0, t, size=(rows, cols), dtype=np.uint64)


def make_setup(orc, logn, q, t=T, steps=None):
    """relin key and Galois keys: every default key (create_galois_keys() without arguments) when steps is None, else exactly the
    keys of `steps`"""
    if steps is None:
        return pc.setup_from_primes(orc, logn, q, t, all_galois=True, base_steps=())
    return pc.setup_from_primes(orc, logn, q, t, extra_steps=steps, base_steps=())


def slot_vector(n, row0, row1=None):
    """the slot values BatchEncoder::encode receives: row0 at slots [0, len), row1 (optional) at [N/2, N/2 + len)"""
    v = np.zeros(n if row1 is not None else max(len(row0), 1), np.uint64)
    v[:len(row0)] = row0
    if row1 is not None:
        v[n // 2:n // 2 + len(row1)] = row1
    return v


def encrypt_diagonals(S, M, both_rows=False, seed=300):
    """W_0 .. W_{r-1}: the analyst's encryptions of the generalized diagonals (in both rows of the batching if asked)"""
    rows, cols = M.shape
    d = hand_diagonals(M, rows, cols)
    O = S.O
    return np.stack([O.encrypt(S.pk, O.encode(slot_vector(S.n, di, di if both_rows else None)), seed + i) for i, di in enumerate(d)])


def encrypt_inputs(S, xs, xs1=None, seed=100):
    """one ciphertext per input vector (row 0), with a second vector in row 1 when xs1 is given"""
    O = S.O
    return np.stack([O.encrypt(S.pk, O.encode(slot_vector(S.n, x, None if xs1 is None else xs1[b])), seed + b) for b, x in enumerate(xs)])


def fc_packed_ref(O, rk, gk, W, x, rows, cols):
    """the layer on one ciphertext, in the oracle's operations -- the definition, step for step"""
    n = O.n
    r, c = hand_shape(n, rows, cols)
    x = np.array(x, dtype=np.uint64, copy=True)
    if 2 * c != n:
        x = O.add(x, O.rotate_rows(x, -c, gk)[0])
    rot = [x]
    for i in range(1, r):
        rot.append(O.rotate_rows(rot[i - 1], 1, gk)[0])
    acc = O.multiply(rot[0], W[0])
    for i in range(1, r):
        acc = O.add(acc, O.multiply(rot[i], W[i]))
    y = O.relinearize(acc, rk)
    s = r
    while s < c:
        y = O.add(y, O.rotate_rows(y, s, gk)[0])
        s *= 2
    return y


def plain_product(M, x, t):
    """(M x) mod t in Python integers; x may be longer than cols (the padded columns of the diagonals are zero)"""
    rows, cols = M.shape
    return [sum(int(M[i][j]) * int(x[j]) for j in range(cols)) % t for i in range(rows)]


def check_slots(S, ct, M, x, x1=None, what=""):
    """the oracle's noise budget is positive, then slots [0, rows) of row 0 (and of row 1) are (M x) mod t"""
    O = S.O
    assert O.noise_budget(S.sk, ct) > 0, ("no noise budget left", what)
    dec = O.decode(O.decrypt(S.sk, ct))
    rows = M.shape[0]
    assert [int(v) for v in dec[:rows]] == plain_product(M, x, S.t), ("row 0 differs from (M x) mod t", what)
    if x1 is not None:
        assert [int(v) for v in dec[S.n // 2:S.n // 2 + rows]] == plain_product(M, x1, S.t), ("row 1 differs from (M x) mod t", what)


def check_layer(X, S, mem, M, B=2, seed=0, in_place=False, rk=None, gk=None, xs=None, xs1=None, both_rows=False, refs=None, words_items=None):
    """hhe_fc_packed_ks against both truths.  words_items: the items compared word for word with the oracle's composition (None: all).
    Returns (device words, reference words per compared item)"""
    rows, cols = M.shape
    O = S.O
    rng = np.random.default_rng(2000 + seed)
    if xs is None:
        xs = [rng.integers(0, S.t, size=cols, dtype=np.uint64) for _ in range(B)]
    W = encrypt_diagonals(S, M, both_rows=both_rows, seed=300 + 16 * seed)
    cts = encrypt_inputs(S, xs, xs1, seed=100 + 16 * seed)
    mat = X.enc_matrix(mem.to_dev(W), rows, cols)
    try:
        r, c = hand_shape(S.n, rows, cols)
        assert mat.bytes == r * 2 * (2 * O.L + 1) * O.n * 8
        d_in = mem.to_dev(cts)
        d_out = d_in if in_place else mem.empty((B,) + O.ct_shape)
        got = mem.to_host(mat.apply(d_in, B, rk=rk, gk=gk, out=None if in_place else d_out))
        assert X.query("fc_packed_key_switches") == hand_key_switches(S.n, rows, cols)
    finally:
        mat.destroy()
    items = range(B) if words_items is None else words_items
    if refs is None:
        refs = {b: fc_packed_ref(O, S.rk, S.gk, W, cts[b], rows, cols) for b in items}
    for b in items:
        assert (got[b] == refs[b]).all(), ("fc_packed differs from the oracle's composition", b, rows, cols)
    for b in range(B):
        check_slots(S, got[b], M, xs[b], None if xs1 is None else xs1[b], what=(rows, cols, b))
    return got, refs


def add_many_words(q, K, B, size, n, pattern):
    """[K][B][size][L][N] words: 'max' = q_j - 1 everywhere, 'alt' = q_j - 1 and 0 alternating along the terms and the coefficients,
    'rand' = uniform below q_j"""
    L = len(q)
    w = np.zeros((K, B, size, L, n), np.uint64)
    rng = np.random.default_rng(K * 131 + size)
    for j, qj in enumerate(q):
        if pattern == "max":
            w[:, :, :, j, :] = qj - 1
        elif pattern == "alt":
            on = (np.arange(K)[:, None] + np.arange(n)[None, :]) % 2 == 0
            w[:, :, :, j, :] = np.where(on, np.uint64(qj - 1), np.uint64(0))[:, None, None, :]
        else:
            w[:, :, :, j, :] = rng.integers(0, qj, size=(K, B, size, n), dtype=np.uint64)
    return w


def check_add_many(X, mem, q, K, B, size, pattern):
    """hhe_add_many against Python integers: every word of the sum, one launch"""
    L, n = len(q), X.n
    w = add_many_words(q, K, B, size, n, pattern)
    out = mem.empty((B, size, L, n))
    before = X.query("add_many_launches")
    X.add_many(mem.to_dev(w), K, out, B, size)
    X.sync()
    assert X.query("add_many_launches") == before + 1
    got = mem.to_host(out)
    for j, qj in enumerate(q):
        want = (w[:, :, :, j, :].astype(object).sum(axis=0) % int(qj)).astype(np.uint64)   # Python integers: no word to wrap
        assert (got[:, :, j, :] == want).all(), ("add_many differs from the integer sum", K, size, pattern, j)


# ---- chunking, lifecycle, refusals: the same checks on the emulator and on the device (N = 1024, every default Galois key) ----
def check_chunking(make_ctx, S, mem, monkeypatch):
    """B = 5: the unchunked words, under HHE_CHUNK=2 HHE_STREAMS=2 (one item per chunk, two lanes) and under HHE_CHUNK=8 HHE_STREAMS=0
    (r = 4: two items per chunk, 2 + 2 + 1, on the caller's stream)"""
    M = seeded_matrix(S.t, 3, 5, 61)
    X = make_ctx()
    got, refs = check_layer(X, S, mem, M, B=5, seed=7)
    X.close()
    for chunk, streams in (("2", "2"), ("8", "0")):
        monkeypatch.setenv("HHE_CHUNK", chunk)
        monkeypatch.setenv("HHE_STREAMS", streams)
        Y = make_ctx()
        g2, _ = check_layer(Y, S, mem, M, B=5, seed=7, refs=refs)
        assert (g2 == got).all(), (chunk, streams)
        Y.close()


def check_handles(X, S, mem):
    """two handles on one context used alternately; a handle from two threads with the other one beside it; destroy, then create again;
    a forgotten handle goes with its context"""
    import threading
    O = S.O
    shapes = [(3, 5), (4, 4)]
    Ms = [seeded_matrix(S.t, r, c, 70 + i) for i, (r, c) in enumerate(shapes)]
    Ws = [encrypt_diagonals(S, M, seed=400 + 32 * i) for i, M in enumerate(Ms)]
    xs = [np.random.default_rng(71).integers(0, S.t, size=4, dtype=np.uint64) for _ in range(2)]
    cts = encrypt_inputs(S, xs, seed=500)
    refs = [np.stack([fc_packed_ref(O, S.rk, S.gk, Ws[i], cts[b], *shapes[i]) for b in range(2)]) for i in range(2)]
    mats = [X.enc_matrix(mem.to_dev(Ws[i]), *shapes[i]) for i in range(2)]
    d_in = mem.to_dev(cts)
    for i in (0, 1, 0, 1):
        out = mem.empty((2,) + O.ct_shape)
        mats[i].apply(d_in, 2, out=out)
        assert (mem.to_host(out) == refs[i]).all(), i
    errors = []

    def work(i):
        try:
            for _ in range(2):
                o = mem.empty((2,) + O.ct_shape)
                mats[i].apply(mem.to_dev(cts), 2, out=o)
                assert (mem.to_host(o) == refs[i]).all(), i
        except BaseException as e:  # noqa: BLE001 -- reported by the asserting thread below
            errors.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in (0, 0, 1)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    mats[0].destroy()
    again = X.enc_matrix(mem.to_dev(Ws[0]), *shapes[0])
    out = mem.empty((2,) + O.ct_shape)
    again.apply(d_in, 2, out=out)
    assert (mem.to_host(out) == refs[0]).all()
    again.destroy()
    mats[1].destroy()
    X.enc_matrix(mem.to_dev(Ws[1]), *shapes[1]).h = None   # never destroyed: hhe_ctx_destroy releases it


def check_refusals(X, Y, S, mem, api):
    """every refusal of hhe_fc_packed_ks and hhe_enc_matrix_create, with `out` prefilled and untouched.  X, Y: two contexts of S"""
    import ctypes as C

    import pytest
    O = S.O
    rows, cols = 3, 5   # steps -8, +1, 4
    M = seeded_matrix(S.t, rows, cols, 91)
    d_W = mem.to_dev(encrypt_diagonals(S, M, seed=800))
    d_in = mem.to_dev(encrypt_inputs(S, [np.arange(cols, dtype=np.uint64)], seed=900))
    mat = X.enc_matrix(d_W, rows, cols)
    elt = {int(e): k for e, k in zip(S.gk.elts, S.gk.keys)}

    def refused(code, text, B=1, **kw):
        out = mem.to_dev(np.full((1,) + O.ct_shape, 12345, np.uint64))
        with pytest.raises(api.HheError) as e:
            mat.apply(d_in, B, out=out, **kw)
        assert e.value.code == code and text in str(e.value), (code, str(e.value))
        assert (mem.to_host(out) == 12345).all()

    full = X.keyset().set_relin(S.rk)
    for s in (-8, 1, 4):
        full.set_galois(int(O.galois_elt(s)), elt[int(O.galois_elt(s))])
    out = mem.empty((1,) + O.ct_shape)
    mat.apply(d_in, 1, rk=full, gk=full, out=out)   # exactly the three keys serve the layer
    check_slots(S, mem.to_host(out)[0], M, np.arange(cols))
    for missing in (-8, 1, 4):                      # ... and each kind of step is missed: -c, +1, a tail step
        ks = X.keyset().set_relin(S.rk)
        for s in (-8, 1, 4):
            if s != missing:
                ks.set_galois(int(O.galois_elt(s)), elt[int(O.galois_elt(s))])
        refused(api.ERR_NO_GALOIS_KEY, "Galois key not present", rk=ks, gk=ks)
        ks.close()
    norelin = X.keyset()
    refused(api.ERR_NO_RELIN_KEY, "relinearization key not set", rk=norelin, gk=full)
    norelin.close()
    full.close()
    refused(api.ERR_INVALID, "empty batch", B=0)
    yks = Y.keyset().set_relin(S.rk)
    refused(api.ERR_INVALID, "another context", rk=yks)
    yks.close()
    other = Y.enc_matrix(d_W, rows, cols)
    out = mem.to_dev(np.full((1,) + O.ct_shape, 12345, np.uint64))   # Y's handle in a call on X (the binding's object names its own context)
    assert X.lib.hhe_fc_packed_ks(X.h, None, None, other.h, api._ptr(d_in), api._ptr(out), C.c_size_t(1)) == api.ERR_INVALID
    assert b"another context" in X.lib.hhe_last_error() and (mem.to_host(out) == 12345).all()
    other.destroy()
    # creation: 2c != N with 4c > N, and an empty dimension
    for r_, c_, code in ((3, 513, api.ERR_TOO_FEW_SLOTS), (600, 5, api.ERR_TOO_FEW_SLOTS), (0, 5, api.ERR_INVALID), (3, 0, api.ERR_INVALID)):
        with pytest.raises(api.HheError) as e:
            X.enc_matrix(d_W, r_, c_)
        assert e.value.code == code, (r_, c_)
    mat.destroy()
