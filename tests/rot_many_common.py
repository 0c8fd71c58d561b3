"""Checker of the hoisted rotations (hhe_rotate_rows_many_ks) and of the packed encrypted FC with a hoisted chain
(hhe_fc_packed_hoisted_ks).  Shared by the emulator suite (numpy memory) and the GPU suite (torch memory), as fc_packed_common is.

Three things live here: the MODEL of the trie the host driver walks, built from oracle.naf and the key set's elements and from nothing
of the library (node count, children per inner node, depth, the expected queries); the reference COMPOSITION of the layer from the
oracle's operations; and the checks both suites run.  Every comparison of ciphertexts is exact equality of words."""
import numpy as np

import definition_common as dc
import fc_packed_common as fp
import parity_common as pc

T = fp.T


# ---- the trie model ----
class RotTrie:
    """Evaluator::rotate_rows serves a step from its own key when the set holds one, else term by term along naf(step) with the terms
    equal to +-N/2 skipped.  The term sequences of a list of steps form a trie; node 0 is the input (step 0 ends there), every other
    node is one key switch.  kids[k] / parent[k] / depth[k] / term[k] describe node k; ends[k] lists the steps (indices) that end there."""

    def __init__(self, orc, n, steps, key_elts):
        keys = set(int(e) for e in key_elts)
        self.n, self.steps = n, list(steps)
        self.term, self.parent, self.kids, self.depth, self.ends = [0], [-1], [[]], [0], [[]]
        for idx, s in enumerate(self.steps):
            assert abs(s) < n // 2
            if s == 0:
                terms = []
            elif pc.galois_elt_py(n, s) in keys:
                terms = [s]
            else:
                terms = [t for t in orc.naf(s) if abs(t) != n // 2]
            node = 0
            for t in terms:
                if pc.galois_elt_py(n, t) not in keys:
                    raise KeyError(("Galois key not present", s, t))
                # children are told apart by their element: -1 and N/2 - 1 name the same key switch
                nxt = next((k for k in self.kids[node] if pc.galois_elt_py(n, self.term[k]) == pc.galois_elt_py(n, t)), -1)
                if nxt < 0:
                    nxt = len(self.term)
                    self.term.append(t); self.parent.append(node); self.kids.append([]); self.ends.append([])
                    self.depth.append(self.depth[node] + 1)
                    self.kids[node].append(nxt)
                node = nxt
            self.ends[node].append(idx)
        self.nodes = len(self.term) - 1
        self.max_depth = max(self.depth)
        self.kid_counts = sorted((len(k) for k in self.kids if k), reverse=True)

    def launches(self, group):
        return sum(-(-c // group) for c in self.kid_counts)


def expect_queries(X, trie):
    """the queries about the last call: the trie's nodes, and the multi-child launches per chunk where the row kernels run"""
    group = X.query("rot_many_group")
    assert group >= 16
    assert X.query("rot_many_key_switches") == trie.nodes, (X.query("rot_many_key_switches"), trie.nodes)
    want = trie.launches(group) if X.query("row_kernel") == 1 and X.query("rot_hoist") != 0 else 0
    assert X.query("rot_many_launches") == want, (X.query("rot_many_launches"), want)


# ---- key sets ----
def setup_with_steps(orc, logn, q, steps, all_default=False, t=T):
    """Setup whose Galois keys are exactly those of `steps` (plus every default key with all_default)"""
    return pc.setup_from_primes(orc, logn, q, t, all_galois=all_default, extra_steps=steps, base_steps=())


def load_ctx(api, lib, S):
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    S.load_keys(X)
    return X


def encryptions(S, B, seed=100):
    O = S.O
    rng = np.random.default_rng(seed)
    return np.stack([O.encrypt(S.pk, O.encode(rng.integers(0, S.t, 8, dtype=np.uint64)), seed + b) for b in range(B)])


# ---- truth (a): the oracle's rotate_rows per step ----
def oracle_rotations(S, cts, steps, gk=None):
    """[n_steps][B][2][L][N]; equal steps are computed once"""
    O, gk = S.O, gk or S.gk
    memo = {}
    out = np.zeros((len(steps), len(cts)) + O.ct_shape, np.uint64)
    for k, s in enumerate(steps):
        for b, ct in enumerate(cts):
            if (s, b) not in memo:
                memo[(s, b)] = np.array(ct, copy=True) if s == 0 else O.rotate_rows(ct, s, gk)[0]
            out[k, b] = memo[(s, b)]
    return out


def run_rot_many(X, mem, cts, steps, gk=None):
    B = len(cts)
    out = mem.empty((len(steps), B) + tuple(cts.shape[1:]))
    X.rotate_rows_many(mem.to_dev(cts), steps, out, B, gk=gk)
    return mem.to_host(out)


def check_rot_many(X, S, mem, orc, steps, B=3, cts=None, refs=None, seed=100):
    """every word of every step against the oracle, and the queries against the model.  Returns (words, reference)"""
    cts = encryptions(S, B, seed) if cts is None else cts
    got = run_rot_many(X, mem, cts, steps)
    refs = oracle_rotations(S, cts, steps) if refs is None else refs
    bad = [(k, b) for k in range(len(steps)) for b in range(len(cts)) if not (got[k, b] == refs[k, b]).all()]
    assert not bad, ("rotate_rows_many differs from the oracle's rotate_rows at (step index, item):", bad, steps)
    expect_queries(X, RotTrie(orc, S.n, steps, S.gk.elts))
    return got, refs


def check_refusals(X, Y, S, mem, api):
    """every refusal, with `out` prefilled and untouched.  S holds the default keys only; X, Y: two contexts of S"""
    import ctypes as C

    import pytest
    O = S.O
    cts = encryptions(S, 1, seed=900)
    d_in = mem.to_dev(cts)

    def refused(code, steps, B=1, gk=None, ct=d_in):
        out = mem.to_dev(np.full((max(len(steps), 1), 1) + O.ct_shape, 12345, np.uint64))
        with pytest.raises(api.HheError) as e:
            X.rotate_rows_many(ct, steps, out, B, gk=gk)
        assert e.value.code == code, (code, str(e.value))
        assert (mem.to_host(out) == 12345).all()

    only = X.keyset()   # the keys of 1 and 4 alone: 3 = -1 + 4 needs the key of -1
    elt = {int(e): k for e, k in zip(S.gk.elts, S.gk.keys)}
    for s in (1, 4):
        only.set_galois(int(O.galois_elt(s)), elt[int(O.galois_elt(s))])
    refused(api.ERR_NO_GALOIS_KEY, [1, 4, 3, 5], gk=only)
    only.close()
    refused(api.ERR_INVALID, [1, S.n // 2])
    refused(api.ERR_INVALID, [1, -(S.n // 2)])
    refused(api.ERR_INVALID, [])
    refused(api.ERR_INVALID, [1], B=0)
    yks = Y.keyset()
    refused(api.ERR_INVALID, [1], gk=yks)
    yks.close()
    # overlap: out begins inside ct, and ct begins inside out
    buf = mem.to_dev(np.concatenate([cts, cts, cts]))
    before = mem.to_host(buf).copy()
    ctw = int(np.prod(O.ct_shape))
    base = api._ptr(buf).value
    steps = (C.c_int * 2)(1, 2)
    for ct_off, out_off in ((0, 0), (2, 0), (1, 0)):
        rc = X.lib.hhe_rotate_rows_many_ks(X.h, None, C.c_void_p(base + ct_off * ctw * 8), steps, C.c_size_t(2), C.c_void_p(base + out_off * ctw * 8),
                                           C.c_size_t(1))
        if ct_off == 2:   # ct behind the two output ciphertexts: no overlap, served
            assert rc == 0
            X.sync()
            after = mem.to_host(buf)
            assert (after[2] == before[2]).all() and (after[0] == O.rotate_rows(cts[0], 1, S.gk)[0]).all()
            buf = mem.to_dev(before)
            base = api._ptr(buf).value
        else:
            assert rc == api.ERR_INVALID and b"overlaps" in X.lib.hhe_last_error()
            assert (mem.to_host(buf) == before).all()


# ---- truth (b): the Python-integer key switch, through one node with three children ----
def check_against_integers(make_ctx, E, mem, seed=0):
    """three sparse keys and the rounding-boundary key of definition_common as the children of ONE node (the input), full vector"""
    X = make_ctx()
    steps = [1, -1, 3]
    keys = [E.stored(("sparse", seed + 20 + i), lambda i=i: dc.SparseKey(E, seed + 20 + i)) for i in range(3)]
    ks = X.keyset()
    for s, key in zip(steps, keys):
        ks.set_galois(pc.galois_elt_py(E.n, s), key.words)
    cts = dc.switch_inputs(E, ("rows", 1), 3, seed + 5)
    got = run_rot_many(X, mem, cts, steps, gk=ks)
    assert X.query("rot_many_key_switches") == 3
    for k, (s, key) in enumerate(zip(steps, keys)):
        for b in range(len(cts)):
            dc.assert_switch("rotate_rows_many, item %d" % b, ("rows", s), got[k, b], dc.switch_truth(E, ("rows", s), key, cts[b]))
    # the rounding boundary: one dense key under all three elements, digits (1, 0, .., 0)
    dense = E.stored(("dense", seed), lambda: dc.DenseKey(E, seed))
    for s in steps:
        ks.set_galois(pc.galois_elt_py(E.n, s), dense.words)
    ct = dc.unit_input(E, ("rows", 1), np.random.default_rng(seed))
    got = run_rot_many(X, mem, ct[None], steps, gk=ks)
    for k, s in enumerate(steps):
        dc.assert_switch("rotate_rows_many, boundary", ("rows", s), got[k, 0], dc.switch_truth(E, ("rows", s), dense, ct))
    ks.close()
    X.close()


# ---- the layer: truth (c) ----
def hand_hoisted_steps(n, rows, cols):
    """-c unless the row is full, 1 .. r-1, then r, 2r, .. below c"""
    r, c = fp.hand_shape(n, rows, cols)
    steps = ([] if 2 * c == n else [-c]) + list(range(1, r))
    s = r
    while s < c:
        steps.append(s)
        s *= 2
    return steps


def hand_hoisted_key_switches(orc, n, rows, cols, key_elts):
    r, c = fp.hand_shape(n, rows, cols)
    return (0 if 2 * c == n else 1) + RotTrie(orc, n, list(range(1, r)), key_elts).nodes + (c // r).bit_length() - 1


def fc_packed_hoisted_ref(O, rk, gk, W, x, rows, cols):
    """the layer with step 2 hoisted, in the oracle's operations: rot_i = rotate_rows(x, i, gk)"""
    n = O.n
    r, c = fp.hand_shape(n, rows, cols)
    x = np.array(x, dtype=np.uint64, copy=True)
    if 2 * c != n:
        x = O.add(x, O.rotate_rows(x, -c, gk)[0])
    rot = [x] + [O.rotate_rows(x, i, gk)[0] for i in range(1, r)]
    acc = O.multiply(rot[0], W[0])
    for i in range(1, r):
        acc = O.add(acc, O.multiply(rot[i], W[i]))
    y = O.relinearize(acc, rk)
    s = r
    while s < c:
        y = O.add(y, O.rotate_rows(y, s, gk)[0])
        s *= 2
    return y


def check_hoisted_layer(X, S, mem, orc, M, B=2, seed=0, in_place=False, rk=None, gk=None, refs=None, words_items=None, chain=True):
    """hhe_fc_packed_hoisted_ks against the composition and against plain integers; with `chain` the SAME handle also serves
    hhe_fc_packed_ks, whose words are those of its own composition.  Returns (device words, references, inputs)"""
    rows, cols = M.shape
    O = S.O
    rng = np.random.default_rng(2000 + seed)
    xs = [rng.integers(0, S.t, size=cols, dtype=np.uint64) for _ in range(B)]
    W = fp.encrypt_diagonals(S, M, seed=300 + 16 * seed)
    cts = fp.encrypt_inputs(S, xs, seed=100 + 16 * seed)
    mat = X.enc_matrix(mem.to_dev(W), rows, cols)
    try:
        d_in = mem.to_dev(cts)
        d_out = d_in if in_place else mem.empty((B,) + O.ct_shape)
        got = mem.to_host(X.fc_packed_hoisted(d_in, mat, d_out, B, rk=rk, gk=gk))
        r, _ = fp.hand_shape(S.n, rows, cols)
        assert X.query("fc_packed_key_switches") == hand_hoisted_key_switches(orc, S.n, rows, cols, S.gk.elts)
        if r > 1:
            expect_queries(X, RotTrie(orc, S.n, list(range(1, r)), S.gk.elts))
        if chain and 1 in [int(s) for s in fp.hand_steps(S.n, rows, cols)] and pc.galois_elt_py(S.n, 1) in set(int(e) for e in S.gk.elts):
            one = mem.to_host(mat.apply(mem.to_dev(cts[:1]), 1, rk=rk, gk=gk, out=mem.empty((1,) + O.ct_shape)))
            assert (one[0] == fp.fc_packed_ref(O, S.rk, S.gk, W, cts[0], rows, cols)).all(), "hhe_fc_packed_ks changed its words"
            assert X.query("fc_packed_key_switches") == fp.hand_key_switches(S.n, rows, cols)
    finally:
        mat.destroy()
    items = range(B) if words_items is None else words_items
    if refs is None:
        refs = {b: fc_packed_hoisted_ref(O, S.rk, S.gk, W, cts[b], rows, cols) for b in items}
    for b in items:
        assert (got[b] == refs[b]).all(), ("fc_packed_hoisted differs from the oracle's composition", b, rows, cols)
    for b in range(B):
        fp.check_slots(S, got[b], M, xs[b], what=(rows, cols, b))
    return got, refs, (W, cts, xs)
