"""Checker of the chainable packed FC (hhe_enc_matrix_create_open / hhe_fc_open_ks), of hhe_square and of the FC-square-FC network
call (hhe_mlp_ks).  Shared by the emulator suite (numpy memory) and the GPU suite (torch memory), as fc_packed_common is.

Four truths, none of which shares code with the library:
  1. hhe_square: the oracle's multiply(a, a), word for word;
  2. the open layer, words: the oracle's rotate_rows, add and relinearize composed around the public hhe_multiply_sum (which has its
     own truth in mult_sum_common);
  3. the open layer and the network, slots: plain Python integers, M x mod t and M_2 (M_1 x)^2 mod t and so on, after the oracle's
     noise budget is seen positive.  THE INPUT CIPHERTEXTS CARRY A RANDOM VALUE IN EVERY SLOT OF BOTH ROWS outside [0, cols): the point
     of the open layout is that nothing is asked of those slots;
  4. hhe_mlp_ks: hhe_fc_open_ks, hhe_square and hhe_relinearize_ks composed on the same context, word for word.
Every comparison of ciphertexts is exact equality of words, every comparison of slots exact equality of integers."""
import numpy as np

import fc_packed_common as fp
import rot_many_common as rmc

T = fp.T

# rows, cols, (r, c), Galois key switches per item when the set holds a key for each of -1 .. -(r-1)
OPEN_SHAPES = [
    (3, 5, (4, 8), 4),        # base case
    (1, 8, (1, 8), 3),        # r = 1: no rotation, the tail alone
    (4, 4, (4, 8), 4),        # the cyclic form has no tail here; the open one has one step
    (2, 511, (2, 512), 9),    # c == N/2: the tail reaches the row's end
    (5, 250, (8, 512), 13),
    (8, 3, (8, 16), 8),       # rows > cols
]

# chain name -> (logn, bit sizes, [(rows, cols), ..]); the oracle's budgets after input / layer / square / layer .. are in the issue:
# 124 / 97 / 72 / 46, 124 / 94 / 70 / 45, 174 / 147 / 122 / 96 / 71 / 44 and 154 / 120 / 95 / 66
NETWORKS = {
    "6x20_3x6": (10, [50] * 4, [(6, 20), (3, 6)]),
    "5x250_3x5": (10, [50] * 4, [(5, 250), (3, 5)]),
    "three_layers": (10, [50] * 5, [(6, 20), (4, 6), (3, 4)]),
    "16x784_10x16": (12, [60] * 4, [(16, 784), (10, 16)]),
}


# ---- the layout, by hand ----
def hand_open_shape(n, rows, cols):
    """(r, c): r = the smallest power of two >= rows, c = the smallest power of two >= cols + r - 1; c <= N/2 is the only slot rule"""
    r = fp.pow2_ceil(rows)
    c = fp.pow2_ceil(cols + r - 1)
    if 2 * c > n:
        raise RuntimeError("too little slots for matmul implementation!")
    return r, c


def hand_open_steps(n, rows, cols):
    """-1 .. -(r-1), then r, 2r, .. below c"""
    r, c = hand_open_shape(n, rows, cols)
    steps = [-e for e in range(1, r)]
    s = r
    while s < c:
        steps.append(s)
        s *= 2
    return steps


def hand_open_diagonals(M):
    """D_e[j] = M[j mod r][j - e] if j mod r < rows and 0 <= j - e < cols, else 0; e < r, j < c -- no index wraps"""
    rows, cols = M.shape
    r = fp.pow2_ceil(rows)
    c = fp.pow2_ceil(cols + r - 1)
    return [[int(M[j % r][j - e]) if j % r < rows and 0 <= j - e < cols else 0 for j in range(c)] for e in range(r)]


def hand_open_key_switches(orc, n, rows, cols, key_elts):
    """the nodes of the trie over -1 .. -(r-1) (the model of rot_many_common) + the tail's log2(c / r)"""
    r, c = hand_open_shape(n, rows, cols)
    nodes = rmc.RotTrie(orc, n, [-e for e in range(1, r)], key_elts).nodes if r > 1 else 0
    return nodes + (c // r).bit_length() - 1


def all_steps(n, shapes):
    out = []
    for rows, cols in shapes:
        out += hand_open_steps(n, rows, cols)
    return sorted(set(out))


# ---- inputs ----
def encrypt_open_diagonals(S, M, seed=300):
    """W_0 .. W_{r-1}: the open diagonals in slots [0, c) of BOTH rows of the batching, encrypted"""
    O = S.O
    return np.stack([O.encrypt(S.pk, O.encode(fp.slot_vector(S.n, d, d)), seed + e) for e, d in enumerate(hand_open_diagonals(M))])


def full_inputs(S, cols, B, seed):
    """(cts, xs, xs1): B ciphertexts whose slots are ALL random -- xs[b] is what row 0 holds at [0, cols), xs1[b] what row 1 holds there;
    every other slot of both rows holds a random value too"""
    O = S.O
    rng = np.random.default_rng(seed)
    cts, xs, xs1 = [], [], []
    for b in range(B):
        v = rng.integers(0, S.t, size=S.n, dtype=np.uint64)
        assert (v[cols:S.n // 2] != 0).any() or cols == S.n // 2
        xs.append(v[:cols].copy())
        xs1.append(v[S.n // 2:S.n // 2 + cols].copy())
        cts.append(O.encrypt(S.pk, O.encode(v), 5000 + 16 * seed + b))
    return np.stack(cts), xs, xs1


# ---- truth 2: the layer's words ----
def fc_open_ref(X, mem, O, rk, gk, W, x, rows, cols):
    """the open layer on one ciphertext: the oracle's rotate_rows, add and relinearize around the public hhe_multiply_sum of X"""
    r, c = hand_open_shape(O.n, rows, cols)
    x = np.array(x, dtype=np.uint64, copy=True)
    rot = [x] + [O.rotate_rows(x, -e, gk)[0] for e in range(1, r)]
    out3 = mem.empty((1, 3) + tuple(O.ct_shape[1:]))
    X.multiply_sum(mem.to_dev(np.stack(rot)[:, None]), mem.to_dev(np.asarray(W)[:, None]), r, out3, 1)
    X.sync()
    y = O.relinearize(mem.to_host(out3)[0], rk)
    s = r
    while s < c:
        y = O.add(y, O.rotate_rows(y, s, gk)[0])
        s *= 2
    return y


# ---- truth 3: plain integers ----
def plain_mlp(Ms, x, t):
    """M_k ( .. (M_1 x)^2 .. )^2 mod t in Python integers: a square between layers, none after the last"""
    v = [int(a) for a in x]
    for k, M in enumerate(Ms):
        rows, cols = M.shape
        assert len(v) >= cols
        v = [sum(int(M[i][j]) * v[j] for j in range(cols)) % t for i in range(rows)]
        if k + 1 < len(Ms):
            v = [a * a % t for a in v]
    return v


def check_slots(S, ct, Ms, x, x1, what="", O=None, sk=None):
    """the oracle's noise budget is positive, then slots [0, rows) of row 0 and of row 1 are the plain integers"""
    O, sk = O or S.O, S.sk if sk is None else sk
    budget = O.noise_budget(sk, ct)
    assert budget > 0, ("no noise budget left", what)
    dec = O.decode(O.decrypt(sk, ct))
    rows = Ms[-1].shape[0]
    assert [int(v) for v in dec[:rows]] == plain_mlp(Ms, x, S.t), ("row 0 differs from the plain integers", what)
    assert [int(v) for v in dec[S.n // 2:S.n // 2 + rows]] == plain_mlp(Ms, x1, S.t), ("row 1 differs from the plain integers", what)
    return budget


# ---- the checks ----
def check_open_layer(X, S, mem, orc, M, B=2, seed=0, in_place=False, rk=None, gk=None, refs=None, O=None, keys=None, data=None,
                     words_items=None, key_elts=None):
    """hhe_fc_open_ks against truths 2 and 3, and its counters.  data: (W, cts, xs, xs1) already at the context's level.
    Returns (device words, references, xs, xs1)"""
    rows, cols = M.shape
    O = O or S.O
    ork, ogk = keys or (S.rk, S.gk)
    if data is None:
        W = encrypt_open_diagonals(S, M, seed=300 + 16 * seed)
        cts, xs, xs1 = full_inputs(S, cols, B, seed)
    else:
        W, cts, xs, xs1 = data
    r, c = hand_open_shape(S.n, rows, cols)
    shape = (B,) + tuple(O.ct_shape)
    mat = X.enc_matrix_open(mem.to_dev(W), rows, cols)
    try:
        assert mat.bytes == r * 2 * (2 * O.L + 1) * O.n * 8
        d_in = mem.to_dev(cts)
        adds = X.query("add_many_launches")
        got = mem.to_host(mat.apply_open(d_in, B, rk=rk, gk=gk, out=None if in_place else mem.empty(shape)))
        want = hand_open_key_switches(orc, S.n, rows, cols, ogk.elts if key_elts is None else key_elts)
        assert X.query("fc_packed_key_switches") == want, (X.query("fc_packed_key_switches"), want)
        assert X.query("fc_packed_floors") == 3
        assert X.query("add_many_launches") == adds, "the sum kernel of hhe_add_many ran"
    finally:
        mat.destroy()
    items = range(B) if words_items is None else words_items
    if refs is None:
        refs = {b: fc_open_ref(X, mem, O, ork, ogk, W, cts[b], rows, cols) for b in items}
    for b in items:
        assert (got[b] == refs[b]).all(), ("fc_open differs from the composition around hhe_multiply_sum", b, rows, cols)
    return got, refs, xs, xs1


def check_open_slots(S, got, M, xs, xs1, O=None, sk=None):
    for b in range(len(xs)):
        check_slots(S, got[b], [M], xs[b], xs1[b], what=(M.shape, b), O=O, sk=sk)


def network_setup(orc, name):
    """the Setup of a chain of NETWORKS: the relin key, every default Galois key and a key for every step of every layer"""
    logn, bits, shapes = NETWORKS[name]
    return rmc.setup_with_steps(orc, logn, orc.coeff_modulus_create(1 << logn, bits), all_steps(1 << logn, shapes), all_default=True)


def network_data(S, shapes, B, seed):
    """(Ms, Ws, cts, xs, xs1): seeded weights, their encrypted open diagonals, and inputs with every slot random"""
    Ms = [fp.seeded_matrix(S.t, r, c, 40 * seed + k) for k, (r, c) in enumerate(shapes)]
    Ws = [encrypt_open_diagonals(S, M, seed=7000 + 64 * k + seed) for k, M in enumerate(Ms)]
    cts, xs, xs1 = full_inputs(S, shapes[0][1], B, 90 + seed)
    return Ms, Ws, cts, xs, xs1


def composed(X, mem, mats, d_in, B, ct_shape, rk=None, gk=None):
    """truth 4: the network from the public calls hhe_fc_open_ks, hhe_square and hhe_relinearize_ks, with their host waits"""
    shape = (B,) + tuple(ct_shape)
    x = d_in
    for k, m in enumerate(mats):
        y = m.apply_open(x, B, rk=rk, gk=gk, out=mem.empty(shape))
        if k + 1 == len(mats):
            return y
        s3 = mem.empty((B, 3) + tuple(ct_shape[1:]))
        X.square(y, s3, B)
        x = mem.empty(shape)
        X.relinearize(s3, x, B, rk=rk)
        X.sync()


def check_network(X, S, mem, shapes, B=2, seed=0, in_place=False, data=None, slots=True):
    """hhe_mlp_ks against truth 4 (every word of every item) and truth 3 (both rows); the counters.  Returns (words, data)"""
    O = S.O
    data = data or network_data(S, shapes, B, seed)
    Ms, Ws, cts, xs, xs1 = data
    mats = [X.enc_matrix_open(mem.to_dev(W), *M.shape) for W, M in zip(Ws, Ms)]
    try:
        d_in = mem.to_dev(cts)
        want = mem.to_host(composed(X, mem, mats, d_in, B, O.ct_shape))
        ks = 0
        for m in mats:   # the layers one by one leave their counters behind
            m.apply_open(d_in, B, out=mem.empty((B,) + tuple(O.ct_shape)))
            ks += X.query("fc_packed_key_switches")
        d_work = mem.to_dev(cts) if in_place else d_in
        out = d_work if in_place else mem.to_dev(np.full((B,) + tuple(O.ct_shape), 12345, np.uint64))
        got = mem.to_host(X.mlp(mats, d_work, out, B))
        assert X.query("mlp_layers") == len(mats)
        assert X.query("mlp_key_switches") == ks, (X.query("mlp_key_switches"), ks)
        assert X.query("fc_packed_floors") == 3
    finally:
        for m in mats:
            m.destroy()
    for b in range(B):
        assert (got[b] == want[b]).all(), ("hhe_mlp_ks differs from the composed public calls", b, shapes)
    if slots:
        for b in range(B):
            budget = check_slots(S, got[b], Ms, xs[b], xs1[b], what=(shapes, b))
            print("oracle noise budget after %s, item %d: %d bits" % (shapes, b, budget))
    return got, data


def square_operands(E, B, pattern, seed):
    """[B][2][L][N]: 'enc' encryptions, 'max' every word q_j - 1, 'alt' q_j - 1 alternating with 0, 'rand' uniform words, 'half' every
    coefficient (Q - 1) / 2"""
    import mult_sum_common as ms
    return ms.operands(E, 1, B, pattern, seed)[0][0]


def check_square(X, E, mem, B, pattern, seed=0, oracle_items=None):
    """hhe_square against the oracle's multiply(a, a), and against hhe_multiply(a, a) on the same context, whose words and launches
    (one launch of the one-product tensor kernel per modulus set, none of the squaring or the summed kernel) a square before it does
    not change"""
    a = square_operands(E, B, pattern, seed)
    d_a = mem.to_dev(a)
    shape3 = (B, 3) + a.shape[2:]
    def counters():
        return [X.query(k) for k in ("tensor_launches", "square_launches", "multiply_sum_launches")]
    mul0 = mem.empty(shape3)
    c0 = counters()
    X.multiply(d_a, d_a, mul0, B)
    X.sync()
    c1 = counters()
    assert [b - a for a, b in zip(c0, c1)] == [2, 0, 0], "hhe_multiply(a, a): one one-product tensor launch per modulus set"
    got = mem.to_dev(np.full(shape3, 12345, np.uint64))
    X.square(d_a, got, B)
    c2 = counters()
    assert [b - a for a, b in zip(c1, c2)] == [0, 2, 0], "hhe_square: one launch of the squaring kernel per modulus set"
    mul1 = mem.empty(shape3)
    X.multiply(d_a, d_a, mul1, B)
    X.sync()
    assert [b - a for a, b in zip(c2, counters())] == [2, 0, 0], "hhe_multiply(a, a) after a square launches what it launched"
    got, mul0, mul1 = mem.to_host(got), mem.to_host(mul0), mem.to_host(mul1)
    assert (mul0 == mul1).all(), "hhe_multiply(a, a) changed its words after a square"
    assert (got == mul0).all(), ("hhe_square differs from hhe_multiply(a, a)", pattern, B)
    for b in (range(B) if oracle_items is None else oracle_items):
        assert (got[b] == E.O.multiply(a[b], a[b])).all(), ("hhe_square differs from the oracle's multiply(a, a)", pattern, b)
    return got


# ---- chunking, fallback, lifecycle, refusals: the same checks on the emulator and on the device.  make_ctx() gives a context of S with
# S's keys loaded; NET is network_setup(orc, "6x20_3x6") ----
SHAPES_NET = NETWORKS["6x20_3x6"][2]


def check_one_layer_network(X, S, mem):
    Ms, Ws, cts, xs, xs1 = network_data(S, [(6, 20)], 2, 4)
    mat = X.enc_matrix_open(mem.to_dev(Ws[0]), 6, 20)
    shape = (2,) + tuple(S.O.ct_shape)
    a = mem.to_host(mat.apply_open(mem.to_dev(cts), 2, out=mem.empty(shape)))
    b = mem.to_host(X.mlp([mat], mem.to_dev(cts), mem.empty(shape), 2))
    assert (a == b).all()
    assert X.query("mlp_layers") == 1 and X.query("mlp_key_switches") == X.query("fc_packed_key_switches")
    mat.destroy()


def check_chunking(make_ctx, S, mem, monkeypatch):
    """B = 5: the unchunked words, under HHE_CHUNK=2 HHE_STREAMS=2 and under HHE_CHUNK=8 HHE_STREAMS=0 (max r = 8: one item per chunk)"""
    X = make_ctx()
    got, data = check_network(X, S, mem, SHAPES_NET, B=5, seed=7)
    X.close()
    for chunk, streams in (("2", "2"), ("8", "0")):
        monkeypatch.setenv("HHE_CHUNK", chunk)
        monkeypatch.setenv("HHE_STREAMS", streams)
        Y = make_ctx()
        g2, _ = check_network(Y, S, mem, SHAPES_NET, B=5, data=data, slots=False)
        assert (g2 == got).all(), (chunk, streams)
        Y.close()


def check_fallback(make_ctx, S, mem, monkeypatch):
    """HHE_ROT_HOIST=2 (every chunk recomputed whole, from vi; in place the results are parked) and =0, against the default's words"""
    X = make_ctx()
    got, data = check_network(X, S, mem, SHAPES_NET, B=3, seed=9)
    X.close()
    monkeypatch.setenv("HHE_ROT_HOIST", "2")
    Y = make_ctx()
    assert Y.query("rot_hoist") == 2
    before = Y.query("rot_many_fallbacks")
    g2, _ = check_network(Y, S, mem, SHAPES_NET, B=3, data=data, slots=False)
    assert Y.query("rot_many_fallbacks") > before
    assert (g2 == got).all()
    g3, _ = check_network(Y, S, mem, SHAPES_NET, B=3, data=data, slots=False, in_place=True)
    assert (g3 == got).all()
    Y.close()
    monkeypatch.setenv("HHE_ROT_HOIST", "0")
    Z = make_ctx()
    assert Z.query("rot_hoist") == 0
    g4, _ = check_network(Z, S, mem, SHAPES_NET, B=3, data=data, slots=False)
    assert (g4 == got).all()
    Z.close()


def check_lifecycle(X, S, mem):
    """two handles used alternately, destroy, create again; a forgotten handle goes with its context"""
    Ms, Ws, cts, xs, xs1 = network_data(S, SHAPES_NET, 2, 5)
    shape = (2,) + tuple(S.O.ct_shape)
    mats = [X.enc_matrix_open(mem.to_dev(W), *M.shape) for W, M in zip(Ws, Ms)]
    d_in = mem.to_dev(cts)
    first = [mem.to_host(m.apply_open(d_in, 2, out=mem.empty(shape))) for m in mats]
    net = mem.to_host(X.mlp(mats, d_in, mem.empty(shape), 2))
    for i in (1, 0, 1, 0):
        assert (mem.to_host(mats[i].apply_open(d_in, 2, out=mem.empty(shape))) == first[i]).all(), i
    mats[0].destroy()
    again = X.enc_matrix_open(mem.to_dev(Ws[0]), *Ms[0].shape)
    assert (mem.to_host(again.apply_open(d_in, 2, out=mem.empty(shape))) == first[0]).all()
    assert (mem.to_host(X.mlp([again, mats[1]], d_in, mem.empty(shape), 2)) == net).all()
    again.destroy()
    mats[1].destroy()
    X.enc_matrix_open(mem.to_dev(Ws[1]), *Ms[1].shape).h = None   # never destroyed: hhe_ctx_destroy releases it


def check_level(orc, api, lib, mem):
    """N = 1024, 4 x 50 bits, level 2, derived key sets; the truth is the oracle of the short chain under the projected keys"""
    import level_common as lc
    S = lc.parent_setup(orc, "n1024_4x50")
    l, rows, cols = 2, 3, 5
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    top = lc.top_set(X, S)
    Xl = X.at_level(l)
    ks = Xl.keyset().derive_from(top)
    Sl = lc.level_setup(orc, api, S, l)
    M = fp.seeded_matrix(S.t, rows, cols, 81)
    cts, xs, xs1 = full_inputs(S, cols, 2, 82)
    _, W = lc.switched(X, S, mem, encrypt_open_diagonals(S, M, seed=600), l)
    _, cts = lc.switched(X, S, mem, cts, l)
    got, _, _, _ = check_open_layer(Xl, Sl, mem, orc, M, B=2, rk=ks, gk=ks, O=Sl.O, keys=(Sl.rk, Sl.gk), data=(W, cts, xs, xs1))
    check_open_slots(Sl, got, M, xs, xs1)
    ks.close()
    top.close()
    Xl.close()
    X.close()


def check_refusals(X, Y, S, mem, api):
    """every refusal of hhe_fc_open_ks, hhe_mlp_ks and hhe_enc_matrix_create_open, and the two kinds of handle handed to the other kind's
    calls, with `out` prefilled and untouched.  X, Y: two contexts of S = network_setup(orc, "6x20_3x6")"""
    import ctypes as C

    import pytest
    O = S.O
    shapes = NETWORKS["6x20_3x6"][2]   # r = 8, c = 32 and r = 4, c = 16
    Ms, Ws, cts, _, _ = network_data(S, shapes, 1, 6)
    d_in = mem.to_dev(cts)
    mats = [X.enc_matrix_open(mem.to_dev(W), *M.shape) for W, M in zip(Ws, Ms)]
    cyclic = X.enc_matrix(mem.to_dev(Ws[0]), 6, 20)
    other = Y.enc_matrix_open(mem.to_dev(Ws[0]), 6, 20)
    elt = {int(e): k for e, k in zip(S.gk.elts, S.gk.keys)}

    def prefilled():
        return mem.to_dev(np.full((1,) + tuple(O.ct_shape), 12345, np.uint64))

    def refused(call, code, text):
        out = prefilled()
        with pytest.raises(api.HheError) as e:
            call(out)
        assert e.value.code == code and text in str(e.value), (code, str(e.value))
        assert (mem.to_host(out) == 12345).all()

    def raw_mlp(handles, out, B=1, vi=d_in):
        arr = (C.c_void_p * max(len(handles), 1))(*handles)
        return X.lib.hhe_mlp_ks(X.h, None, None, arr, C.c_size_t(len(handles)), api._ptr(vi), api._ptr(out), C.c_size_t(B))

    # the two kinds of handle do not cross
    for hoisted in (False, True):
        refused(lambda o: mats[0].apply_sum(d_in, 1, out=o, hoisted=hoisted), api.ERR_INVALID, "open handle")
    refused(lambda o: mats[0].apply(d_in, 1, out=o), api.ERR_INVALID, "open handle")
    refused(lambda o: mats[0].apply_hoisted(d_in, 1, out=o), api.ERR_INVALID, "open handle")
    refused(lambda o: cyclic.apply_open(d_in, 1, out=o), api.ERR_INVALID, "cyclic handle")
    refused(lambda o: X.mlp([mats[0], cyclic], d_in, o, 1), api.ERR_INVALID, "cyclic handle")
    # the network's own
    refused(lambda o: X.mlp([], d_in, o, 1), api.ERR_INVALID, "no layer")
    refused(lambda o: X.mlp([mats[0], None], d_in, o, 1), api.ERR_INVALID, "null handle")
    refused(lambda o: X.mlp([mats[0], other], d_in, o, 1), api.ERR_INVALID, "another context")
    refused(lambda o: X.mlp([mats[1], mats[0]], d_in, o, 1), api.ERR_INVALID, "rows of a layer")
    refused(lambda o: X.mlp(mats, d_in, o, 0), api.ERR_INVALID, "empty batch")
    refused(lambda o: mats[0].apply_open(d_in, 0, out=o), api.ERR_INVALID, "empty batch")
    out = prefilled()
    assert raw_mlp([m.h for m in mats], out, vi=None) == api.ERR_INVALID and (mem.to_host(out) == 12345).all()
    assert X.lib.hhe_mlp_ks(X.h, None, None, None, C.c_size_t(2), api._ptr(d_in), api._ptr(out), C.c_size_t(1)) == api.ERR_INVALID
    assert X.lib.hhe_fc_open_ks(X.h, None, None, None, api._ptr(d_in), api._ptr(out), C.c_size_t(1)) == api.ERR_INVALID
    assert (mem.to_host(out) == 12345).all()
    yks = Y.keyset().set_relin(S.rk)
    refused(lambda o: X.mlp(mats, d_in, o, 1, rk=yks), api.ERR_INVALID, "another context")
    yks.close()
    # keys: a tail step of either layer, a rotation term of either layer, the relinearization key
    need = all_steps(S.n, shapes)

    def keyset(missing=None, relin=True):
        ks = X.keyset()
        if relin:
            ks.set_relin(S.rk)
        for s in need:
            if s != missing:
                ks.set_galois(int(O.galois_elt(s)), elt[int(O.galois_elt(s))])
        return ks
    full = keyset()
    out = mem.empty((1,) + tuple(O.ct_shape))
    X.mlp(mats, d_in, out, 1, rk=full, gk=full)   # exactly these keys serve the network
    for missing in (16, 8, 4, -1, -4):            # layer 1's tail; both tails; layer 2's tail; terms of every rotation
        ks = keyset(missing)
        refused(lambda o: X.mlp(mats, d_in, o, 1, rk=ks, gk=ks), api.ERR_NO_GALOIS_KEY, "Galois key not present")
        ks.close()
    ks = keyset(4)                                 # layer 1 alone is served without the step 4 ...
    mats[0].apply_open(d_in, 1, rk=ks, gk=ks, out=mem.empty((1,) + tuple(O.ct_shape)))
    refused(lambda o: mats[1].apply_open(d_in, 1, rk=ks, gk=ks, out=o), api.ERR_NO_GALOIS_KEY, "Galois key not present")
    ks.close()
    norelin = keyset(relin=False)
    refused(lambda o: X.mlp(mats, d_in, o, 1, rk=norelin, gk=full), api.ERR_NO_RELIN_KEY, "relinearization key not set")
    refused(lambda o: mats[0].apply_open(d_in, 1, rk=norelin, gk=full, out=o), api.ERR_NO_RELIN_KEY, "relinearization key not set")
    norelin.close()
    full.close()
    # creation
    for r_, c_, code in ((2, 512, api.ERR_TOO_FEW_SLOTS), (600, 5, api.ERR_TOO_FEW_SLOTS), (0, 5, api.ERR_INVALID), (3, 0, api.ERR_INVALID)):
        with pytest.raises(api.HheError) as e:
            X.enc_matrix_open(mem.to_dev(Ws[0]), r_, c_)
        assert e.value.code == code, (r_, c_)
    for m in mats + [cyclic]:
        m.destroy()
    other.destroy()


def check_cap_refusal(orc, api, lib, mem):
    """N = 1024, one 60-bit data prime, t of 60 bits: the floored sum of two products no longer fits B_sk; r = 1 is served"""
    import pytest

    import definition_common as dc
    q = orc.coeff_modulus_create(1024, [60] * 2)
    S = fp.make_setup(orc, 10, q, t=dc.T60)
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    S.load_keys(X)
    assert X.query("behz_sum_cap") < 2
    M = fp.seeded_matrix(S.t, 3, 5, 92)
    M1 = fp.seeded_matrix(S.t, 1, 3, 93)
    mat = X.enc_matrix_open(mem.to_dev(encrypt_open_diagonals(S, M, seed=810)), 3, 5)
    one = X.enc_matrix_open(mem.to_dev(encrypt_open_diagonals(S, M1, seed=820)), 1, 3)
    cts, _, _ = full_inputs(S, 5, 1, 93)
    for call in (lambda o: mat.apply_open(mem.to_dev(cts), 1, out=o), lambda o: X.mlp([mat, one], mem.to_dev(cts), o, 1)):
        out = mem.to_dev(np.full((1,) + tuple(S.O.ct_shape), 12345, np.uint64))
        with pytest.raises(api.HheError) as e:
            call(out)
        assert e.value.code == api.ERR_INVALID and "behz_sum_cap" in str(e.value)
        assert (mem.to_host(out) == 12345).all()
    one.apply_open(mem.to_dev(cts), 1, out=mem.empty((1,) + tuple(S.O.ct_shape)))
    mat.destroy()
    one.destroy()
    X.close()
