"""Hoisted rotations (hhe_rotate_rows_many_ks) and the packed encrypted FC with a hoisted chain (hhe_fc_packed_hoisted_ks) on the
tests-only emulator (built with -DHHE_RANGE_CHECK): the host driver's walk over the trie, the multi-child form of the key-switch row
kernel's body and the separate-kernel path, word for word against the oracle's rotate_rows per step, against the Python-integer key
switch of definition_common, and -- the layer -- against the oracle's composition and (M x) mod t in plain integers."""
import ctypes as C

import numpy as np
import pytest

import definition_common as dc
import fc_packed_common as fp
import level_common as lc
import parity_common as pc
import rot_many_common as rm

T = rm.T
MIXED = [1, -1, 3, 5, -5, 7, 100, -100, 511, -511, 0]


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


@pytest.fixture(scope="module")
def S10(orc):
    """N = 1024, 3 x 50 bits (no row kernel): every default Galois key"""
    return rm.setup_with_steps(orc, 10, orc.coeff_modulus_create(1024, [50] * 3), (), all_default=True)


@pytest.fixture(scope="module")
def S10own(orc):
    """... and a key for each of 1 .. 15"""
    return rm.setup_with_steps(orc, 10, orc.coeff_modulus_create(1024, [50] * 3), list(range(1, 16)), all_default=True)


@pytest.fixture(scope="module")
def S10three(orc):
    """... the default keys and a key for step 3"""
    return rm.setup_with_steps(orc, 10, orc.coeff_modulus_create(1024, [50] * 3), [3], all_default=True)


@pytest.fixture(scope="module")
def S12(orc):
    """N = 4096, 3 x 60 bits (row kernels): every default key and a key for each of 1 .. 17"""
    return rm.setup_with_steps(orc, 12, orc.coeff_modulus_create(4096, [60] * 3), list(range(1, 18)), all_default=True)


@pytest.fixture(scope="module")
def S12default(orc):
    return rm.setup_with_steps(orc, 12, orc.coeff_modulus_create(4096, [60] * 3), (), all_default=True)


def _ctx(api, lib, S, row_kernel=None):
    X = rm.load_ctx(api, lib, S)
    if row_kernel is not None:
        assert X.query("row_kernel") == row_kernel
    return X


# ---- 1. pins of the model ----
def test_trie_model_pins(orc):
    d10, d12 = pc.default_galois_elts_py(1024), pc.default_galois_elts_py(4096)
    own = [pc.galois_elt_py(4096, s) for s in range(1, 16)]
    t = rm.RotTrie(orc, 4096, range(1, 16), d12)
    assert (t.nodes, t.kid_counts, t.max_depth) == (20, [7, 4, 3, 2, 1, 1, 1, 1], 3)
    t = rm.RotTrie(orc, 4096, range(1, 16), d12 + own)
    assert (t.nodes, t.kid_counts, t.max_depth) == (15, [15], 1)
    assert rm.RotTrie(orc, 1024, range(1, 8), d10).nodes == 9
    assert rm.RotTrie(orc, 1024, MIXED, d10 + [pc.galois_elt_py(1024, 3)]).nodes == 12
    assert t.launches(16) == 1 and rm.RotTrie(orc, 4096, range(1, 18), d12 + own + [pc.galois_elt_py(4096, s) for s in (16, 17)]).launches(16) == 2
    with pytest.raises(KeyError):
        rm.RotTrie(orc, 1024, [3], [pc.galois_elt_py(1024, 4)])


# ---- 2. N = 1024: the separate-kernel path ----
@pytest.mark.parametrize("case", ["1..15 default", "1..15 own", "1..7 default", "mixed, a key for 3"])
def test_n1024_steps_against_the_oracle(orc, api, emu_lib, mem, S10, S10own, S10three, case):
    S, steps = {"1..15 default": (S10, list(range(1, 16))), "1..15 own": (S10own, list(range(1, 16))),
                "1..7 default": (S10, list(range(1, 8))), "mixed, a key for 3": (S10three, MIXED)}[case]
    X = _ctx(api, emu_lib, S, row_kernel=0)
    rm.check_rot_many(X, S, mem, orc, steps, B=3)
    assert X.query("rot_many_launches") == 0 and X.query("rot_many_fallbacks") == 0
    X.close()


def test_repeated_steps_and_step_zero_copy(orc, api, emu_lib, mem, S10three):
    X = _ctx(api, emu_lib, S10three)
    steps = [0, 3, 5, 3, 0, 5, 5]
    cts = rm.encryptions(S10three, 2, seed=140)
    got, _ = rm.check_rot_many(X, S10three, mem, orc, steps, cts=cts)
    assert (got[0] == cts).all() and (got[4] == cts).all()
    assert (got[1] == got[3]).all() and (got[2] == got[5]).all() and (got[2] == got[6]).all()
    assert X.query("rot_many_key_switches") == 3   # 3 by its key; 5 = 1 + 4
    X.close()


# ---- 3. N = 4096: the multi-child launch of the row kernel ----
@pytest.mark.parametrize("B", [1, 3])
def test_row_kernel_one_node_fifteen_children(orc, api, emu_lib, mem, S12, B):
    X = _ctx(api, emu_lib, S12, row_kernel=1)
    rm.check_rot_many(X, S12, mem, orc, list(range(1, 16)), B=B)
    assert X.query("rot_many_launches") == 1 and X.query("rot_many_key_switches") == 15 and X.query("rot_many_fallbacks") == 0
    X.close()


def test_row_kernel_group_and_one_more(orc, api, emu_lib, mem, S12):
    """1 .. group is one launch, 1 .. group + 1 the second launch of the node"""
    X = _ctx(api, emu_lib, S12, row_kernel=1)
    group = X.query("rot_many_group")
    assert 16 <= group and group + 1 <= 17, "the fixture holds keys for 1 .. 17"
    cts = rm.encryptions(S12, 1, seed=150)
    refs = rm.oracle_rotations(S12, cts, list(range(1, group + 2)))
    rm.check_rot_many(X, S12, mem, orc, list(range(1, group + 1)), cts=cts, refs=refs[:group])
    assert X.query("rot_many_launches") == 1
    rm.check_rot_many(X, S12, mem, orc, list(range(1, group + 2)), cts=cts, refs=refs)
    assert X.query("rot_many_launches") == 2
    X.close()


def test_row_kernel_one_child_and_opposite_steps(orc, api, emu_lib, mem, S12):
    X = _ctx(api, emu_lib, S12, row_kernel=1)
    rm.check_rot_many(X, S12, mem, orc, [7], B=2)
    assert X.query("rot_many_launches") == 1
    rm.check_rot_many(X, S12, mem, orc, [4, -4, 1, -1, 64, -64], B=2)
    X.close()


def test_row_kernel_default_keys_depth_three(orc, api, emu_lib, mem, S12default):
    """intermediate nodes that are no outputs (8 on the way to 7 = -1 + 8, 16 on the way to 15): 20 nodes, 8 inner ones"""
    X = _ctx(api, emu_lib, S12default, row_kernel=1)
    steps = list(range(1, 16))
    trie = rm.RotTrie(orc, 4096, steps, S12default.gk.elts)
    assert trie.max_depth == 3 and any(not e and k for k, e in enumerate(trie.ends))
    rm.check_rot_many(X, S12default, mem, orc, steps, B=2)
    assert X.query("rot_many_launches") == sum(-(-c // X.query("rot_many_group")) for c in trie.kid_counts) == 8
    X.close()


def test_row_kernel_every_word_at_q_minus_one(orc, api, emu_lib, mem, S12):
    """c0 and c1 at q_j - 1 everywhere, uniform random keys below their primes: the lazy sums of the multi-child body at their bound,
    under the emulator's range check"""
    S, O = S12, S12.O
    steps = list(range(1, 16))
    rng = np.random.default_rng(160)
    elts = [pc.galois_elt_py(S.n, s) for s in steps]
    keys = np.zeros((len(elts),) + O.ksk_shape, np.uint64)
    for J in range(O.K):
        keys[:, :, :, J, :] = rng.integers(0, S.q[J], keys[:, :, :, J, :].shape, dtype=np.uint64)
    gk = orc.GaloisKeys(elts, keys)
    X = api.Context(S.logn, S.q, S.t, lib=emu_lib)
    assert X.query("row_kernel") == 1
    ks = X.keyset()
    for e, k in zip(elts, keys):
        ks.set_galois(int(e), k)
    cts = np.stack([pc.adversarial_words(S, 2, "max"), pc.adversarial_words(S, 2, "alt")])
    cts[1][cts[1] == 0] = 1   # a zero residue would (rightly) take the fallback; this case is about the hoisted body
    got = rm.run_rot_many(X, mem, cts, steps, gk=ks)
    assert X.query("rot_many_fallbacks") == 0 and X.query("rot_many_launches") == 1
    for k, s in enumerate(steps):
        for b in range(2):
            assert (got[k, b] == O.rotate_rows(cts[b], s, gk)[0]).all(), (s, b)
    ks.close()
    X.close()


# ---- 4. against the Python-integer key switch ----
@pytest.mark.parametrize("name", ["n1024", "row12"])
def test_against_the_integer_definition(orc, api, emu_lib, mem, name):
    E, make_ctx = dc.setup(orc, api, emu_lib, name)
    rm.check_against_integers(make_ctx, E, mem)


# ---- 5. the exactness fallback ----
def test_transparent_item_takes_the_fallback_on_the_row_kernels(orc, api, emu_lib, mem, S12):
    """one transparent item (c1 = 0, c0 uniform) among ordinary ones in one chunk: the digit loads raise the flag, the chunk is recomputed
    step by step, and every item is right"""
    S, O = S12, S12.O
    rng = np.random.default_rng(9)
    cts = rm.encryptions(S, 3, seed=170)
    cts[1, 1] = 0
    for j in range(O.L):
        cts[1, 0, j] = rng.integers(0, S.q[j], O.n, dtype=np.uint64)
    assert (cts[0, 1] != 0).all() and (cts[2, 1] != 0).all()
    X = _ctx(api, emu_lib, S, row_kernel=1)
    rm.check_rot_many(X, S, mem, orc, [1, 2, 3, -5], cts=cts)
    assert X.query("rot_many_fallbacks") == 1
    rm.check_rot_many(X, S, mem, orc, [1, 2, 3, -5], cts=cts[[0, 2]])
    assert X.query("rot_many_fallbacks") == 1
    X.close()


def test_one_zero_residue_over_small_primes(orc, api, emu_lib, mem):
    """N = 1024, 4 x 18 bits (the primes of test_fc_shapes' zero cases): one residue of c1 set to 0 in one limb of one item.  A flipped 0
    stays 0 instead of becoming q_I, so the shared transforms are not exact: the chunk falls back; without the zero it does not"""
    logn, bits = pc.ZERO_CASES["n1024_18x4"][:2]
    q = orc.coeff_modulus_create(1 << logn, bits)
    steps = [1, 2, 3]
    S = rm.setup_with_steps(orc, logn, q, steps)   # own keys: the input is the only node with children
    cts = None
    for seed in range(180, 200):   # an encryption whose c1 has no zero residue (they are common at 18 bits)
        c = rm.encryptions(S, 3, seed=seed)
        if (c[:, 1] != 0).all():
            cts = c
            break
    assert cts is not None
    X = _ctx(api, emu_lib, S, row_kernel=0)
    rm.check_rot_many(X, S, mem, orc, steps, cts=cts)
    assert X.query("rot_many_fallbacks") == 0
    cts[2, 1, 1, 517] = 0
    rm.check_rot_many(X, S, mem, orc, steps, cts=cts)
    assert X.query("rot_many_fallbacks") == 1
    X.close()


@pytest.mark.parametrize("fixture,row_kernel", [("S10three", 0), ("S12", 1)])
def test_knob_values_give_the_default_words(orc, api, emu_lib, mem, monkeypatch, request, fixture, row_kernel):
    S = request.getfixturevalue(fixture)
    steps = MIXED if row_kernel == 0 else [1, 2, 3, -5, 0, 16]
    cts = rm.encryptions(S, 3, seed=210)
    X = _ctx(api, emu_lib, S, row_kernel=row_kernel)
    assert X.query("rot_hoist") == 1
    got, refs = rm.check_rot_many(X, S, mem, orc, steps, cts=cts)
    X.close()
    for knob, fallbacks in (("2", 1), ("0", 0)):
        monkeypatch.setenv("HHE_ROT_HOIST", knob)
        Y = _ctx(api, emu_lib, S, row_kernel=row_kernel)
        monkeypatch.delenv("HHE_ROT_HOIST")
        assert Y.query("rot_hoist") == int(knob)
        g2, _ = rm.check_rot_many(Y, S, mem, orc, steps, cts=cts, refs=refs)
        assert (g2 == got).all() and Y.query("rot_many_fallbacks") == fallbacks
        Y.close()


# ---- 6. chunking ----
def test_chunks_and_streams_do_not_change_the_words(orc, api, emu_lib, mem, S10three, monkeypatch):
    cts = rm.encryptions(S10three, 5, seed=220)
    X = _ctx(api, emu_lib, S10three)
    got, refs = rm.check_rot_many(X, S10three, mem, orc, MIXED, cts=cts)
    X.close()
    for chunk, streams in (("2", "2"), ("8", "0")):
        monkeypatch.setenv("HHE_CHUNK", chunk)
        monkeypatch.setenv("HHE_STREAMS", streams)
        Y = _ctx(api, emu_lib, S10three)
        g2, _ = rm.check_rot_many(Y, S10three, mem, orc, MIXED, cts=cts, refs=refs)
        assert (g2 == got).all(), (chunk, streams)
        Y.close()


def test_chunks_on_the_row_kernels(orc, api, emu_lib, mem, S12, monkeypatch):
    """three children, HHE_CHUNK=6: chunks of 2 + 1 items on two lanes, each one launch over 3 x items virtual items"""
    cts = rm.encryptions(S12, 3, seed=230)
    monkeypatch.setenv("HHE_CHUNK", "6")
    monkeypatch.setenv("HHE_STREAMS", "2")
    X = _ctx(api, emu_lib, S12, row_kernel=1)
    rm.check_rot_many(X, S12, mem, orc, [1, 2, -5, 3], cts=cts)
    X.close()


# ---- 7. a level ----
def test_at_a_level(orc, api, emu_lib, mem):
    """N = 1024, 4 x 50 bits, level 2 with a derived key set: the truth is the oracle of the short chain under the projected keys"""
    S = lc.parent_setup(orc, "n1024_4x50")
    l = 2
    X = api.Context(S.logn, S.q, S.t, lib=emu_lib)
    top = lc.top_set(X, S)
    Xl = X.at_level(l)
    ks = Xl.keyset().derive_from(top)
    Sl = lc.level_setup(orc, api, S, l)
    d_x, cts = lc.switched(X, S, mem, rm.encryptions(S, 2, seed=240), l)
    steps = [1, 3, -6, 0, 7]
    out = mem.empty((len(steps), 2, 2, l, S.n))
    Xl.rotate_rows_many(d_x, steps, out, 2, gk=ks)
    got = mem.to_host(out)
    assert (got == rm.oracle_rotations(Sl, cts, steps)).all()
    rm.expect_queries(Xl, rm.RotTrie(orc, S.n, steps, Sl.gk.elts))
    ks.close()
    top.close()
    Xl.close()
    X.close()


# ---- 8. refusals ----
def test_refusals_leave_out_untouched(api, emu_lib, mem, S10):
    X, Y = _ctx(api, emu_lib, S10), _ctx(api, emu_lib, S10)
    rm.check_refusals(X, Y, S10, mem, api)
    Y.close()
    X.close()


# ---- 9. the layer ----
def _layer_setup(orc, logn, q, rows, cols, own):
    steps = rm.hand_hoisted_steps(1 << logn, rows, cols) if own else ()
    return rm.setup_with_steps(orc, logn, q, steps, all_default=True)


@pytest.mark.parametrize("rows,cols,rc,ks", fp.SHAPES)
def test_layer_own_keys(orc, api, emu_lib, mem, rows, cols, rc, ks):
    """a key for each of 1 .. r-1: one node, as many key switches as the chain's"""
    S = _layer_setup(orc, 10, orc.coeff_modulus_create(1024, [50] * 3), rows, cols, own=True)
    X = _ctx(api, emu_lib, S, row_kernel=0)
    rm.check_hoisted_layer(X, S, mem, orc, fp.seeded_matrix(T, rows, cols, 7 * rows + cols), B=2, seed=rows)
    assert rm.hand_hoisted_key_switches(orc, 1024, rows, cols, S.gk.elts) == ks
    X.close()


def test_layer_default_keys_only(orc, api, emu_lib, mem, S10):
    """5 x 256, r = 8: steps 1 .. 7 through the NAF trie over the power-of-two keys, 9 nodes for 7 rotations"""
    X = _ctx(api, emu_lib, S10, row_kernel=0)
    rm.check_hoisted_layer(X, S10, mem, orc, fp.seeded_matrix(T, 5, 256, 291), B=2, seed=5)
    assert rm.hand_hoisted_key_switches(orc, 1024, 5, 256, S10.gk.elts) == 1 + 9 + 5   # check_hoisted_layer held the query to it
    X.close()


def test_layer_in_place_and_under_the_fallback(orc, api, emu_lib, mem, monkeypatch):
    S = _layer_setup(orc, 10, orc.coeff_modulus_create(1024, [50] * 3), 3, 5, own=True)
    M = fp.seeded_matrix(T, 3, 5, 62)
    X = _ctx(api, emu_lib, S)
    got, refs, _ = rm.check_hoisted_layer(X, S, mem, orc, M, B=3, seed=8)
    g2, _, _ = rm.check_hoisted_layer(X, S, mem, orc, M, B=3, seed=8, in_place=True, refs=refs)
    assert (g2 == got).all()
    X.close()
    for knob in ("2", "0"):   # in place, a recomputed chunk must not read its own result
        monkeypatch.setenv("HHE_ROT_HOIST", knob)
        monkeypatch.setenv("HHE_CHUNK", "8")   # r = 4: two items per chunk
        Y = _ctx(api, emu_lib, S)
        g3, _, _ = rm.check_hoisted_layer(Y, S, mem, orc, M, B=3, seed=8, in_place=True, refs=refs, chain=False)
        assert (g3 == got).all() and Y.query("rot_many_fallbacks") == (2 if knob == "2" else 0)
        Y.close()


def test_layer_refuses_a_step_without_its_key(orc, api, emu_lib, mem):
    """3 x 5 at N = 1024: -8 and 4 need their own keys; 1 .. 3 may come through 1, 2, 4, -1 -- but not through nothing"""
    S = _layer_setup(orc, 10, orc.coeff_modulus_create(1024, [50] * 3), 3, 5, own=False)
    X = _ctx(api, emu_lib, S)
    O = S.O
    M = fp.seeded_matrix(T, 3, 5, 91)
    mat = X.enc_matrix(mem.to_dev(fp.encrypt_diagonals(S, M, seed=800)), 3, 5)
    d_in = mem.to_dev(fp.encrypt_inputs(S, [np.arange(5, dtype=np.uint64)], seed=900))
    elt = {int(e): k for e, k in zip(S.gk.elts, S.gk.keys)}
    need = (-8, 1, 2, -1, 4)
    for missing in need:
        ks = X.keyset().set_relin(S.rk)
        for s in need:
            if s != missing:
                ks.set_galois(int(O.galois_elt(s)), elt[int(O.galois_elt(s))])
        out = mem.to_dev(np.full((1,) + O.ct_shape, 12345, np.uint64))
        with pytest.raises(api.HheError) as e:
            X.fc_packed_hoisted(d_in, mat, out, 1, rk=ks, gk=ks)
        assert e.value.code == api.ERR_NO_GALOIS_KEY and (mem.to_host(out) == 12345).all(), missing
        ks.close()
    mat.destroy()
    X.close()


def test_layer_mnist_shape_on_the_row_kernels(orc, api, emu_lib, mem):
    """N = 4096, 3 x 60 bits, 10 x 784: r = 16, the 15 rotations are the children of one node, one launch"""
    q = orc.coeff_modulus_create(4096, [60] * 3)
    S = rm.setup_with_steps(orc, 12, q, rm.hand_hoisted_steps(4096, 10, 784) + [1])
    X = _ctx(api, emu_lib, S, row_kernel=1)
    rm.check_hoisted_layer(X, S, mem, orc, fp.seeded_matrix(T, 10, 784, 5), B=1, seed=6, chain=False)
    assert X.query("fc_packed_key_switches") == 1 + 15 + 6 and X.query("rot_many_launches") == 1
    X.close()


def test_layer_step_lists(api, emu_lib):
    f = lambda *a: api.fc_packed_hoisted_galois_steps(*a, lib=emu_lib)
    assert f(1024, 3, 5) == [-8, 1, 2, 3, 4]
    assert f(1024, 1, 8) == [-8, 1, 2, 4]                              # r == 1: no rotation of x at all; the tail starts at 1
    assert f(1024, 2, 512) == [1] + [2 << k for k in range(8)]         # 2c == N: no -c
    assert f(4096, 10, 784) == [-1024] + list(range(1, 16)) + [16, 32, 64, 128, 256, 512]
    for n, rows, cols in ((1024, 3, 5), (1024, 8, 3), (4096, 10, 784), (1024, 5, 256)):
        assert f(n, rows, cols) == rm.hand_hoisted_steps(n, rows, cols)
    out, cnt = (C.c_int * 2)(), C.c_size_t(2)
    assert emu_lib.hhe_fc_packed_hoisted_galois_steps(C.c_size_t(1024), C.c_size_t(3), C.c_size_t(5), out, C.byref(cnt)) == api.ERR_CAPACITY
    assert cnt.value == 5
    with pytest.raises(api.HheError) as e:
        f(1024, 3, 513)
    assert e.value.code == api.ERR_TOO_FEW_SLOTS
