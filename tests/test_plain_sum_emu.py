"""The plain-weights sum of rotations (hhe_rotate_plain_sum_ks) and the open FC layer under plain weights (hhe_fc_open_plain_ks) on the
tests-only emulator (built with -DHHE_RANGE_CHECK): the host driver, the child loop of the key-switch row kernel's body with its outer
lazy sums, and the separate-launch path.  Truths (plain_sum_common): the definition in Python integers; the oracle's rotate_rows for one
child with the plaintext 1; plain integers mod t behind a decryption.  Every comparison is exact equality."""
import threading

import numpy as np
import pytest

import definition_common as dc
import fc_packed_common as fp
import level_common as lc
import mlp_common as mc
import parity_common as pc
import plain_sum_common as ps
import rot_many_common as rm

T = ps.T
STEPS17 = [1, -1, 0, 2, 3, -3, 1, 4, -4, 5, 6, 7, -7, 8, 0, 9, 10]   # step 0 twice, 1 twice, +k with -k


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


def _own_keys(orc, logn, bits, extra=(), t=T):
    steps = sorted(set(s for s in STEPS17 if s) | set(extra))
    return pc.setup_from_primes(orc, logn, orc.coeff_modulus_create(1 << logn, bits), t, extra_steps=steps, base_steps=())


@pytest.fixture(scope="module")
def S10(orc):
    """N = 1024, 3 x 50 bits (no row kernel): a key for every step of STEPS17 and of the 3 x 5 layer"""
    return _own_keys(orc, 10, [50] * 3, mc.hand_open_steps(1024, 3, 5))


@pytest.fixture(scope="module")
def S12(orc):
    """N = 4096, 3 x 60 bits (row kernel, 64-point row pass)"""
    return _own_keys(orc, 12, [60] * 3, mc.hand_open_steps(4096, 3, 5))


def _ctx(api, lib, S, row_kernel=None):
    X = rm.load_ctx(api, lib, S)
    if row_kernel is not None:
        assert X.query("row_kernel") == row_kernel
    return X


def _pair(request, name):
    return request.getfixturevalue("S10" if name == "n1024" else "S12"), 0 if name == "n1024" else 1


# ---- 1. the definition ----
@pytest.mark.parametrize("name", ["n1024", "row12"])
def test_definition_sparse_keys_and_plaintexts(orc, api, emu_lib, mem, name):
    E, make_ctx = dc.setup(orc, api, emu_lib, name)
    ps.check_definition_sparse(make_ctx, E, mem)
    ps.check_definition_sparse(make_ctx, E, mem, steps=(2, 2, -2, 0, 0, 5), seed=3)   # repeated steps, +k with -k, step 0 twice


@pytest.mark.parametrize("name", ["n1024", "row12"])
def test_definition_rounding_boundary_of_the_sum(orc, api, emu_lib, mem, name):
    E, make_ctx = dc.setup(orc, api, emu_lib, name)
    ps.check_definition_boundary(make_ctx, E, mem)


@pytest.mark.parametrize("name", ["n1024", "row12"])
def test_definition_real_keys_sampled(orc, api, emu_lib, mem, request, name):
    S, _ = _pair(request, name)
    E, make_ctx = dc.setup(orc, api, emu_lib, name)
    assert E.q == S.q
    ps.check_definition_real_keys(make_ctx, S, E, mem)


@pytest.mark.parametrize("name", ["n1024", "row12"])
def test_definition_dense_plaintexts(orc, api, emu_lib, mem, request, name):
    """uniform slot values, every coefficient of the plaintext non-zero: 16 coefficients on both paths, and at N = 1024 the full vector"""
    S, _ = _pair(request, name)
    E, make_ctx = dc.setup(orc, api, emu_lib, name)
    ps.check_definition_dense(make_ctx, S, E, mem)
    if name == "n1024":
        ps.check_definition_dense(make_ctx, S, E, mem, steps=(2, 0, -7), seed=4, idx=None)


def test_definition_t_above_every_prime(orc, api, emu_lib, mem):
    """T60 over 4 x 55 bits: the second branch of the lift under every prime, the special one included"""
    q = orc.coeff_modulus_create(1024, [55] * 4)
    assert all(dc.T60 > v for v in q)
    E = dc.env(orc, 10, q, dc.T60)
    make_ctx = lambda: api.Context(10, q, dc.T60, lib=emu_lib)
    ps.check_definition_sparse(make_ctx, E, mem)
    S = pc.setup_from_primes(orc, 10, q, dc.T60, extra_steps=[1, -3], base_steps=())
    ps.check_definition_real_keys(make_ctx, S, E, mem)
    ps.check_definition_dense(make_ctx, S, E, mem, steps=(1, 0, -3), samples=4)


# ---- 2. one child with the plaintext 1 is rotate_rows ----
@pytest.mark.parametrize("name", ["n1024", "row12"])
def test_one_child_all_ones_is_the_oracles_rotate_rows(orc, api, emu_lib, mem, request, name):
    S, rowk = _pair(request, name)
    X = _ctx(api, emu_lib, S, row_kernel=rowk)
    ps.check_one_child_is_rotate_rows(X, S, mem, [1, -3, 0, 7])
    assert X.query("plain_sum_fallbacks") == 0
    X.close()


# ---- 3. child counts and batch sizes: the slots behind a decryption ----
@pytest.mark.parametrize("name", ["n1024", "row12"])
@pytest.mark.parametrize("B", [1, 3])
def test_child_counts(orc, api, emu_lib, mem, request, name, B):
    S, rowk = _pair(request, name)
    X = _ctx(api, emu_lib, S, row_kernel=rowk)
    fold = X.query("plain_sum_fold")
    assert fold == 3
    cts = ps.encryptions(S, B, 300)
    for n in (1, 2, fold + 1, 17):
        ps.check_primitive(X, S, mem, STEPS17[:n], cts=cts, seed=n)
    ps.check_primitive(X, S, mem, [0, 0], cts=cts, seed=50)         # no rotation at all
    ps.check_primitive(X, S, mem, [3, -3], cts=cts, seed=51, count=8)   # short slot vectors
    assert X.query("plain_sum_fallbacks") == 0
    X.close()


def test_fewer_pairs_than_the_handle_holds(orc, api, emu_lib, mem, S12):
    X = _ctx(api, emu_lib, S12, row_kernel=1)
    rows = ps.random_rows(S12, 5, S12.n, 77)
    cts = ps.encryptions(S12, 1, 310)
    got = ps.run_plain_sum(X, mem, cts, rows, STEPS17[:5], n=3)
    ps.check_slots(S12, mem, got, cts, rows[:3], STEPS17[:3])
    X.close()


# ---- 4. every word at its bound, under the range check ----
@pytest.mark.parametrize("name", ["n1024", "row12"])
@pytest.mark.parametrize("pattern", ["max", "alt", "uniform"])
def test_words_at_their_bounds(orc, api, emu_lib, mem, name, pattern):
    """c0, c1, key words and lifted plaintext words at q_j - 1 (the plaintext -1: every NTT word is q_j - 1); alternating with 0 (the
    plaintext's coefficients alternate -1 with 0); uniform words under a dense plaintext of uniform slot values; fold + 1 children and
    17.  The definition at sampled coefficients (plain_sum_common.dense_truth)."""
    E, make_ctx = dc.setup(orc, api, emu_lib, name)
    ps.check_bounds(make_ctx, E, mem, pattern, STEPS17)


# ---- 5. the fallback ----
def test_one_zero_residue_over_small_primes(orc, api, emu_lib, mem, monkeypatch):
    """N = 1024, 4 x 18 bits: one residue of c1 set to 0 -- the shared digits are not exact, the chunk is recomputed from each child's own
    digits; without the zero it is not.  Both against the definition-backed n = 1 truth and the decrypted slots"""
    logn, bits = pc.ZERO_CASES["n1024_18x4"][:2]
    q = orc.coeff_modulus_create(1 << logn, bits)
    steps = [1, 2, 3]
    S = rm.setup_with_steps(orc, logn, q, steps)
    cts = None
    for seed in range(180, 200):
        c = rm.encryptions(S, 3, seed=seed)
        if (c[:, 1] != 0).all():
            cts = c
            break
    assert cts is not None
    X = _ctx(api, emu_lib, S, row_kernel=0)
    ones = np.ones((1, S.n), np.uint64)
    assert (ps.run_plain_sum(X, mem, cts, ones, [2])[2] == S.O.rotate_rows(cts[2], 2, S.gk)[0]).all()
    assert X.query("plain_sum_fallbacks") == 0
    cts[2, 1, 1, 517] = 0
    assert (ps.run_plain_sum(X, mem, cts, ones, [2])[2] == S.O.rotate_rows(cts[2], 2, S.gk)[0]).all()
    assert X.query("plain_sum_fallbacks") == 1
    # n = 3 with small plaintexts (18-bit primes leave little budget): the flagged call gives the words of the exact form
    rows = np.random.default_rng(3).integers(0, 2, size=(3, S.n), dtype=np.uint64)
    got = ps.run_plain_sum(X, mem, cts, rows, steps)
    assert X.query("plain_sum_fallbacks") == 2
    X.close()
    monkeypatch.setenv("HHE_ROT_HOIST", "0")
    Y = _ctx(api, emu_lib, S, row_kernel=0)
    monkeypatch.delenv("HHE_ROT_HOIST")
    assert (ps.run_plain_sum(Y, mem, cts, rows, steps) == got).all() and Y.query("plain_sum_fallbacks") == 0
    Y.close()


def test_transparent_item_on_the_row_kernels(orc, api, emu_lib, mem, monkeypatch, S12):
    """one transparent item (c1 = 0) among ordinary ones in one chunk at N = 4096: the flag, the recomputation, every item right"""
    S, O = S12, S12.O
    rng = np.random.default_rng(9)
    cts = ps.encryptions(S, 3, 170)
    cts[1, 1] = 0
    for j in range(O.L):
        cts[1, 0, j] = rng.integers(0, S.q[j], O.n, dtype=np.uint64)
    X = _ctx(api, emu_lib, S, row_kernel=1)
    steps = STEPS17[:5]
    rows = ps.random_rows(S, len(steps), S.n, 12)
    got = ps.run_plain_sum(X, mem, cts, rows, steps)
    assert X.query("plain_sum_fallbacks") == 1
    ps.check_slots(S, mem, got[[0, 2]], cts[[0, 2]], rows, steps)
    g2 = ps.run_plain_sum(X, mem, cts[[0, 2]], rows, steps)
    assert X.query("plain_sum_fallbacks") == 1 and (g2 == got[[0, 2]]).all()
    X.close()
    # the transparent item has no budget to decrypt with: its words are those of the form that takes every child's own digits
    monkeypatch.setenv("HHE_ROT_HOIST", "0")
    Y = _ctx(api, emu_lib, S, row_kernel=1)
    monkeypatch.delenv("HHE_ROT_HOIST")
    assert (ps.run_plain_sum(Y, mem, cts, rows, steps) == got).all()
    Y.close()


@pytest.mark.parametrize("name", ["n1024", "row12"])
def test_knob_values_give_the_default_words(orc, api, emu_lib, mem, monkeypatch, request, name):
    S, rowk = _pair(request, name)
    steps = STEPS17[:6]
    cts = ps.encryptions(S, 3, 210)
    X = _ctx(api, emu_lib, S, row_kernel=rowk)
    got, _, rows = ps.check_primitive(X, S, mem, steps, cts=cts, seed=4)
    X.close()
    for knob, fallbacks, launches in (("2", 1, rowk), ("0", 0, 0)):
        monkeypatch.setenv("HHE_ROT_HOIST", knob)
        Y = _ctx(api, emu_lib, S, row_kernel=rowk)
        monkeypatch.delenv("HHE_ROT_HOIST")
        assert Y.query("rot_hoist") == int(knob)
        g2 = ps.run_plain_sum(Y, mem, cts, rows, steps)
        assert (g2 == got).all() and Y.query("plain_sum_fallbacks") == fallbacks
        assert Y.query("plain_sum_launches") == launches and Y.query("plain_sum_mod_downs") == 1
        Y.close()


# ---- 6. chunks, streams, in place ----
@pytest.mark.parametrize("name", ["n1024", "row12"])
def test_chunks_streams_and_in_place(orc, api, emu_lib, mem, monkeypatch, request, name):
    S, rowk = _pair(request, name)
    steps = STEPS17[:5]
    cts = ps.encryptions(S, 5, 220)
    X = _ctx(api, emu_lib, S, row_kernel=rowk)
    got, _, rows = ps.check_primitive(X, S, mem, steps, cts=cts, seed=6)
    assert (ps.run_plain_sum(X, mem, cts, rows, steps, in_place=True) == got).all()
    X.close()
    for chunk, streams, hoist in (("2", "2", None), ("8", "0", None), ("4", "2", "2")):
        monkeypatch.setenv("HHE_CHUNK", chunk)
        monkeypatch.setenv("HHE_STREAMS", streams)
        if hoist:
            monkeypatch.setenv("HHE_ROT_HOIST", hoist)   # in place under the forced fallback: a recomputed chunk must not read its own result
        Y = _ctx(api, emu_lib, S, row_kernel=rowk)
        monkeypatch.delenv("HHE_ROT_HOIST", raising=False)
        assert (ps.run_plain_sum(Y, mem, cts, rows, steps, in_place=bool(hoist)) == got).all(), (chunk, streams, hoist)
        if hoist:
            assert Y.query("plain_sum_fallbacks") == -(-5 // max(1, int(chunk) // 2))
        Y.close()


# ---- 7. a level ----
def test_at_a_level(orc, api, emu_lib, mem):
    """N = 1024, 4 x 50 bits, level 2, a handle made on the level context and a derived key set"""
    S = lc.parent_setup(orc, "n1024_4x50")
    l = 2
    X = api.Context(S.logn, S.q, S.t, lib=emu_lib)
    top = lc.top_set(X, S)
    Xl = X.at_level(l)
    ks = Xl.keyset().derive_from(top)
    Sl = lc.level_setup(orc, api, S, l)
    d_x, cts = lc.switched(X, S, mem, ps.encryptions(S, 2, 240), l)
    steps = [1, -2, 0, 4, -1]
    ones = np.ones((1, S.n), np.uint64)
    got = ps.run_plain_sum(Xl, mem, cts, ones, [4], gk=ks)
    assert (got[0] == Sl.O.rotate_rows(cts[0], 4, Sl.gk)[0]).all()
    rows = ps.random_rows(S, len(steps), S.n, 13)
    got = ps.run_plain_sum(Xl, mem, cts, rows, steps, gk=ks)
    ps.check_slots(Sl, mem, got, cts, rows, steps)
    M = fp.seeded_matrix(S.t, 2, 3, 8)   # r = 2, c = 4: steps -1, 2 are default keys
    mat = Xl.plain_fc_open(M, ps.seeded_bias(S.t, 2, 1))
    out = mem.to_host(mat.apply(d_x, 2, gk=ks, out=mem.empty((2, 2, l, S.n))))
    for b in range(2):
        x = Sl.O.decode(Sl.O.decrypt(Sl.sk, cts[b]))
        assert Sl.O.noise_budget(Sl.sk, out[b]) > 0
        assert [int(v) for v in Sl.O.decode(Sl.O.decrypt(Sl.sk, out[b]))[:2]] == ps.plain_affine(M, ps.seeded_bias(S.t, 2, 1), x, S.t)
    mat.destroy()
    ks.close()
    top.close()
    Xl.close()
    X.close()


# ---- 8. the layer ----
LAYER_SHAPES = [(3, 5), (1, 8), (4, 4), (2, 511), (5, 250), (8, 3)]


@pytest.mark.parametrize("rows,cols", LAYER_SHAPES)
@pytest.mark.parametrize("with_bias", [False, True])
def test_layer_shapes(orc, api, emu_lib, mem, rows, cols, with_bias):
    S = ps.layer_setup(orc, 10, orc.coeff_modulus_create(1024, [50] * 3), rows, cols)
    assert api.fc_open_galois_steps(1024, rows, cols, lib=emu_lib) == mc.hand_open_steps(1024, rows, cols)
    X = _ctx(api, emu_lib, S, row_kernel=0)
    M = fp.seeded_matrix(T, rows, cols, 7 * rows + cols)
    ps.check_layer(X, S, mem, M, ps.seeded_bias(T, rows, rows) if with_bias else None, B=2, seed=rows, budget_beside=with_bias and rows == 3)
    assert X.query("plain_sum_fallbacks") == 0
    X.close()


def test_layer_bias_is_add_plain_of_the_layer_without(orc, api, emu_lib, mem, S10):
    """with a bias the words are hhe_add_plain(encode(bias)) of the words without"""
    X = _ctx(api, emu_lib, S10, row_kernel=0)
    M, bias = fp.seeded_matrix(T, 3, 5, 5), ps.seeded_bias(T, 3, 9)
    got, data = ps.check_layer(X, S10, mem, M, None, B=2, seed=3)
    gb, _ = ps.check_layer(X, S10, mem, M, bias, B=2, seed=3, data=data)
    out = mem.empty(got.shape)
    X.add_plain(mem.to_dev(got), mem.to_dev(S10.O.encode(fp.slot_vector(S10.n, bias))[None]), out, 2, bcast=True)
    X.sync()
    assert (mem.to_host(out) == gb).all()
    for b in range(2):
        assert (gb[b] == S10.O.add_plain(got[b], S10.O.encode(fp.slot_vector(S10.n, bias)))).all()
    X.close()


def test_layer_in_place_chunks_and_the_forced_fallback(orc, api, emu_lib, mem, monkeypatch, S10):
    M, bias = fp.seeded_matrix(T, 3, 5, 62), ps.seeded_bias(T, 3, 4)
    X = _ctx(api, emu_lib, S10)
    got, data = ps.check_layer(X, S10, mem, M, bias, B=5, seed=8)
    g2, _ = ps.check_layer(X, S10, mem, M, bias, B=5, seed=8, in_place=True, data=data)
    assert (g2 == got).all()
    X.close()
    for knob in ("2", "0"):
        monkeypatch.setenv("HHE_ROT_HOIST", knob)
        monkeypatch.setenv("HHE_CHUNK", "4")
        monkeypatch.setenv("HHE_STREAMS", "2")
        Y = _ctx(api, emu_lib, S10)
        g3, _ = ps.check_layer(Y, S10, mem, M, bias, B=5, seed=8, in_place=True, data=data)
        assert (g3 == got).all() and Y.query("plain_sum_fallbacks") == (3 if knob == "2" else 0)
        Y.close()


def test_layer_mnist_shape_on_the_row_kernels(orc, api, emu_lib, mem):
    """N = 4096, 3 x 60 bits, 10 x 784: r = 16 children in one launch, one mod-down, then the six tail rotations"""
    S = ps.layer_setup(orc, 12, orc.coeff_modulus_create(4096, [60] * 3), 10, 784)
    X = _ctx(api, emu_lib, S, row_kernel=1)
    ps.check_layer(X, S, mem, fp.seeded_matrix(T, 10, 784, 5), ps.seeded_bias(T, 10, 6), B=1, seed=6)
    assert X.query("plain_sum_launches") == 1 and X.query("plain_sum_mod_downs") == 1 and X.query("plain_sum_fallbacks") == 0
    X.close()


# ---- 9. refusals and handles ----
@pytest.mark.parametrize("name", ["n1024", "row12"])
def test_refusals_leave_out_untouched(api, emu_lib, mem, request, name):
    S, _ = _pair(request, name)
    X, Y = _ctx(api, emu_lib, S), _ctx(api, emu_lib, S)
    ps.check_refusals(X, Y, S, mem, api)
    Y.close()
    X.close()


def test_handle_lifecycle(orc, api, emu_lib, mem, S10):
    """two handles side by side, two threads on one context, destroy and create again, a forgotten handle released by the context"""
    S = S10
    X = _ctx(api, emu_lib, S)
    cts = ps.encryptions(S, 2, 400)
    steps = [1, -1, 0]
    ra, rb = ps.random_rows(S, 3, S.n, 1), ps.random_rows(S, 3, S.n, 2)
    ha, hb = X.plain_rows(ra), X.plain_rows(rb)
    assert ha.bytes == hb.bytes == 2 * 3 * X.K * X.n * 8
    d_in = mem.to_dev(cts)

    def run(h):
        out = mem.empty(cts.shape)
        X.rotate_plain_sum(d_in, h, steps, out, 2)
        return mem.to_host(out)
    ga, gb = run(ha), run(hb)
    ps.check_slots(S, mem, ga, cts, ra, steps)
    ps.check_slots(S, mem, gb, cts, rb, steps)
    res = {}
    th = [threading.Thread(target=lambda k=k, h=h: res.__setitem__(k, run(h))) for k, h in (("a", ha), ("b", hb))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert (res["a"] == ga).all() and (res["b"] == gb).all()
    ha.destroy()
    assert (run(hb) == gb).all()
    ha = X.plain_rows(ra)
    assert (run(ha) == ga).all()
    forgotten = X.plain_rows(rb)
    fc = X.plain_fc_open(fp.seeded_matrix(T, 3, 5, 1))
    forgotten.h, fc.h = None, None   # never destroyed by the caller: hhe_ctx_destroy releases them
    ha.destroy()
    hb.destroy()
    X.close()


# ---- 10. nothing existing changes ----
def test_existing_calls_keep_their_launch_counts(orc, api, emu_lib, mem, S12):
    """hhe_rotate_rows_many_ks and hhe_fc_open_ks on one context, before and after calls of the new entry points: the same words and counters"""
    S = S12
    X = _ctx(api, emu_lib, S, row_kernel=1)
    cts = ps.encryptions(S, 2, 500)
    steps = [1, 2, 3, -3]

    def existing():
        rot = rm.run_rot_many(X, mem, cts, steps)
        q1 = [X.query(w) for w in ("rot_many_launches", "rot_many_key_switches", "rot_many_fallbacks")]
        M = fp.seeded_matrix(T, 3, 5, 2)
        mat = X.enc_matrix_open(mem.to_dev(mc.encrypt_open_diagonals(S, M)), 3, 5)
        y = mem.to_host(mat.apply_open(mem.to_dev(cts), 2, out=mem.empty(cts.shape)))
        mat.destroy()
        q2 = [X.query(w) for w in ("rot_many_launches", "fc_packed_key_switches", "fc_packed_floors", "multiply_sum_launches", "add_many_launches",
                                   "tensor_launches", "rot_many_fallbacks")]
        return rot, y, q1, q2
    r0, y0, a0, b0 = existing()
    ps.check_primitive(X, S, mem, STEPS17[:5], cts=cts, seed=1)
    ps.check_layer(X, S, mem, fp.seeded_matrix(T, 3, 5, 9), ps.seeded_bias(T, 3, 1), B=2)
    r1, y1, a1, b1 = existing()
    assert (r0 == r1).all() and (y0 == y1).all() and a0 == a1
    assert b1[:3] == b0[:3] and b1[3] - b0[3] == b0[3] and b1[4:] == b0[4:]   # multiply_sum_launches counts up by the same amount
    X.close()
