"""The chainable packed FC (hhe_fc_open_ks), hhe_square and the network call hhe_mlp_ks on the tests-only emulator (built with
-DHHE_RANGE_CHECK, so a 128-bit sum of a tensor kernel that wraps aborts the run).  The truths are in mlp_common: the oracle's
multiply(a, a), the oracle's composition around the public hhe_multiply_sum, plain Python integers with a random value in every
unused input slot, and the public calls composed on the same context."""
import ctypes as C

import numpy as np
import pytest

import definition_common as dc
import fc_packed_common as fp
import mlp_common as mc
import parity_common as pc
import rot_many_common as rmc

T = fp.T
PARAMS = {"n1024": (10, [50] * 3), "n4096": (12, [60] * 3)}


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


def _lctx(api, lib, S):
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    S.load_keys(X)
    return X


# ---- 1. the host helpers ----
@pytest.mark.parametrize("rows,cols,rc,ks", mc.OPEN_SHAPES)
def test_shapes_diagonals_and_steps(api, emu_lib, rows, cols, rc, ks):
    assert mc.hand_open_shape(1024, rows, cols) == rc
    assert api.fc_open_shape(1024, rows, cols, lib=emu_lib) == rc
    M = fp.seeded_matrix(T, rows, cols, 3 * rows + cols)
    want = mc.hand_open_diagonals(M)
    got = api.fc_open_diagonals(T, M, lib=emu_lib)
    assert got.shape == rc and got.tolist() == want
    # the formula once more, entry by entry, and the coverage: row m meets every column exactly once over the r diagonals and c slots
    r, c = rc
    for m in range(rows):
        met = sorted(j - e for e in range(r) for j in range(c) if j % r == m and 0 <= j - e < cols)
        assert met == list(range(cols))
    steps = api.fc_open_galois_steps(1024, rows, cols, lib=emu_lib)
    assert steps == mc.hand_open_steps(1024, rows, cols)
    assert len(steps) == ks == (r - 1) + (c // r).bit_length() - 1


def test_helper_refusals(api, emu_lib):
    for n, rows, cols, code in ((1024, 2, 512, api.ERR_TOO_FEW_SLOTS), (1024, 600, 5, api.ERR_TOO_FEW_SLOTS), (1024, 0, 5, api.ERR_INVALID),
                                (1024, 3, 0, api.ERR_INVALID), (1000, 3, 5, api.ERR_INVALID), (0, 3, 5, api.ERR_INVALID)):
        with pytest.raises(api.HheError) as e:
            api.fc_open_shape(n, rows, cols, lib=emu_lib)
        assert e.value.code == code, (n, rows, cols)
    assert api.fc_open_shape(1024, 2, 511, lib=emu_lib) == (2, 512)
    M = fp.seeded_matrix(T, 3, 5, 1)
    M[1, 2] = T
    with pytest.raises(api.HheError) as e:
        api.fc_open_diagonals(T, M, lib=emu_lib)
    assert e.value.code == api.ERR_INVALID and "plain modulus" in str(e.value)
    # the capacity convention of the step lists: the count comes back, nothing is written
    buf = (C.c_int * 4)(7, 7, 7, 7)
    cnt = C.c_size_t(3)
    assert emu_lib.hhe_fc_open_galois_steps(C.c_size_t(1024), C.c_size_t(3), C.c_size_t(5), buf, C.byref(cnt)) == api.ERR_CAPACITY
    assert cnt.value == 4 and list(buf) == [7, 7, 7, 7]
    assert emu_lib.hhe_fc_open_galois_steps(C.c_size_t(1024), C.c_size_t(3), C.c_size_t(5), buf, C.byref(cnt)) == 0
    assert list(buf) == [-1, -2, -3, 4]
    cnt = C.c_size_t(0)
    assert emu_lib.hhe_fc_open_galois_steps(C.c_size_t(1024), C.c_size_t(3), C.c_size_t(5), None, C.byref(cnt)) == api.ERR_CAPACITY
    assert cnt.value == 4


# ---- 2. the square ----
@pytest.mark.parametrize("pattern", ["enc", "max", "alt", "rand", "half"])
@pytest.mark.parametrize("name", list(PARAMS))
def test_square_is_the_oracles_multiply(orc, api, emu_lib, mem, name, pattern):
    logn, bits = PARAMS[name]
    E = dc.env(orc, logn, orc.coeff_modulus_create(1 << logn, bits), T)
    X = api.Context(E.logn, E.q, E.t, lib=emu_lib)
    for B in (1, 3):
        mc.check_square(X, E, mem, B, pattern, seed=11 + B)
    X.close()


# ---- 3. one open layer ----
@pytest.fixture(scope="module")
def S3(orc):
    """N = 1024, 3 x 50 bits: every default Galois key and a key for each of -1 .. -7"""
    return rmc.setup_with_steps(orc, 10, orc.coeff_modulus_create(1024, [50] * 3), [-e for e in range(1, 8)], all_default=True)


@pytest.fixture(scope="module")
def S3d(orc):
    """the same with the default (power-of-two) keys only"""
    return fp.make_setup(orc, 10, orc.coeff_modulus_create(1024, [50] * 3))


@pytest.mark.parametrize("rows,cols,rc,ks", mc.OPEN_SHAPES)
def test_layer_words_slots_and_counters(orc, api, emu_lib, mem, S3, rows, cols, rc, ks):
    X = _lctx(api, emu_lib, S3)
    M = fp.seeded_matrix(T, rows, cols, 7 * rows + cols)
    got, _, xs, xs1 = mc.check_open_layer(X, S3, mem, orc, M, B=2, seed=rows)
    assert X.query("fc_packed_key_switches") == ks
    mc.check_open_slots(S3, got, M, xs, xs1)
    X.close()


def test_layer_over_the_naf_trie(orc, api, emu_lib, mem, S3d):
    """5 x 250 with the default keys only: -3, -5, -6, -7 go through their NAF terms; the node count against the model"""
    X = _lctx(api, emu_lib, S3d)
    M = fp.seeded_matrix(T, 5, 250, 17)
    trie = rmc.RotTrie(orc, 1024, [-e for e in range(1, 8)], S3d.gk.elts)
    assert trie.nodes > 7 and trie.max_depth > 1
    got, _, xs, xs1 = mc.check_open_layer(X, S3d, mem, orc, M, B=2, seed=21)
    assert X.query("fc_packed_key_switches") == trie.nodes + 6
    rmc.expect_queries(X, trie)
    mc.check_open_slots(S3d, got, M, xs, xs1)
    X.close()


def test_mnist_shape_on_the_row_kernels(orc, api, emu_lib, mem):
    """N = 4096, 3 x 60 bits, 10 x 784: r = 16, c = 1024"""
    assert mc.hand_open_shape(4096, 10, 784) == (16, 1024) == fp.hand_shape(4096, 10, 784)
    S = fp.make_setup(orc, 12, orc.coeff_modulus_create(4096, [60] * 3), steps=mc.hand_open_steps(4096, 10, 784))
    X = _lctx(api, emu_lib, S)
    assert X.query("row_kernel") == 1
    M = fp.seeded_matrix(T, 10, 784, 5)
    got, _, xs, xs1 = mc.check_open_layer(X, S, mem, orc, M, B=1, seed=6)
    assert X.query("fc_packed_key_switches") == 15 + 6
    mc.check_open_slots(S, got, M, xs, xs1)
    X.close()


def test_layer_at_a_level(orc, api, emu_lib, mem):
    mc.check_level(orc, api, emu_lib, mem)


# ---- 4. networks ----
@pytest.fixture(scope="module")
def NET(orc):
    return mc.network_setup(orc, "6x20_3x6")


@pytest.mark.parametrize("name", list(mc.NETWORKS))
def test_network_words_and_slots(orc, api, emu_lib, mem, name):
    S = mc.network_setup(orc, name)
    X = _lctx(api, emu_lib, S)
    if S.n >= 4096:
        assert X.query("row_kernel") == 1
    mc.check_network(X, S, mem, mc.NETWORKS[name][2], B=1 if S.n >= 4096 else 2, seed=3)
    X.close()


def test_one_layer_network_is_the_open_layer(api, emu_lib, mem, NET):
    X = _lctx(api, emu_lib, NET)
    mc.check_one_layer_network(X, NET, mem)
    X.close()


def test_chunks_and_streams_do_not_change_the_words(api, emu_lib, mem, NET, monkeypatch):
    mc.check_chunking(lambda: _lctx(api, emu_lib, NET), NET, mem, monkeypatch)


def test_in_place(api, emu_lib, mem, NET):
    X = _lctx(api, emu_lib, NET)
    mc.check_network(X, NET, mem, mc.NETWORKS["6x20_3x6"][2], B=3, seed=8, in_place=True)
    X.close()


def test_forced_fallback_and_no_hoisting(api, emu_lib, mem, NET, monkeypatch):
    mc.check_fallback(lambda: _lctx(api, emu_lib, NET), NET, mem, monkeypatch)


def test_lifecycle(api, emu_lib, mem, NET):
    X = _lctx(api, emu_lib, NET)
    mc.check_lifecycle(X, NET, mem)
    X.close()


# ---- 5. refusals: `out` prefilled and untouched ----
def test_refusals_leave_out_untouched(api, emu_lib, mem, NET):
    X, Y = _lctx(api, emu_lib, NET), _lctx(api, emu_lib, NET)
    mc.check_refusals(X, Y, NET, mem, api)
    Y.close()
    X.close()


def test_refused_above_the_cap(orc, api, emu_lib, mem):
    mc.check_cap_refusal(orc, api, emu_lib, mem)
