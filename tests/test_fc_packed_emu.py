"""Packed encrypted FC layer (hhe_fc_packed_shape / _diagonals / _galois_steps, hhe_enc_matrix_create, hhe_fc_packed_ks) and
hhe_add_many on the tests-only emulator (built with -DHHE_RANGE_CHECK): the host driver's schedule and the index arithmetic of the
kernel bodies, word for word against the oracle's composition of the definition (fc_packed_common.fc_packed_ref) and slot for slot
against (M x) mod t in Python integers."""
import ctypes as C

import numpy as np
import pytest

import fc_packed_common as fp
import level_common as lc
import parity_common as pc

T = fp.T

SHAPES = fp.SHAPES


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


@pytest.fixture(scope="module")
def S3(orc):
    """N = 1024, 3 x 50 bits, every default Galois key"""
    return fp.make_setup(orc, 10, orc.coeff_modulus_create(1024, [50] * 3))


def _ctx(api, lib, S):
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    S.load_keys(X)
    return X


# ---- 1. the helpers ----
@pytest.mark.parametrize("rows,cols,rc,ks", SHAPES)
def test_shape_and_steps(api, emu_lib, rows, cols, rc, ks):
    n = 1024
    assert fp.hand_shape(n, rows, cols) == rc
    assert api.fc_packed_shape(n, rows, cols, lib=emu_lib) == rc
    r, c = rc
    tail = [r << k for k in range(20) if (r << k) < c]
    want = ([] if 2 * c == n else [-c]) + ([1] if r > 1 else []) + tail
    assert fp.hand_steps(n, rows, cols) == want
    assert api.fc_packed_galois_steps(n, rows, cols, lib=emu_lib) == want
    assert fp.hand_key_switches(n, rows, cols) == ks == (2 * c != n) + (r - 1) + len(tail)


def test_step_lists_at_the_edges(api, emu_lib):
    assert api.fc_packed_galois_steps(1024, 1, 8, lib=emu_lib) == [-8, 1, 2, 4]          # r == 1: no +1 chain; the tail starts at 1
    assert api.fc_packed_galois_steps(1024, 8, 8, lib=emu_lib) == [-8, 1]                # r == c: no tail
    assert api.fc_packed_galois_steps(1024, 2, 512, lib=emu_lib) == [1] + [2 << k for k in range(8)]   # 2c == N: no -c
    assert api.fc_packed_galois_steps(4096, 10, 784, lib=emu_lib) == [-1024, 1, 16, 32, 64, 128, 256, 512]
    assert api.fc_packed_galois_steps(1024, 1, 1, lib=emu_lib) == [-1]


def test_shape_refusals(api, emu_lib):
    assert api.fc_packed_shape(1024, 3, 300, lib=emu_lib) == (4, 512)     # c = N / 2 is admitted
    assert api.fc_packed_shape(1024, 3, 256, lib=emu_lib) == (4, 256)     # ... and c = N / 4
    for n, rows, cols, code in ((1024, 3, 513, api.ERR_TOO_FEW_SLOTS),    # c = 1024 > N / 2
                                (1024, 600, 4, api.ERR_TOO_FEW_SLOTS),    # r = 1024 raises c
                                (1024, 0, 4, api.ERR_INVALID), (1024, 4, 0, api.ERR_INVALID), (1000, 4, 4, api.ERR_INVALID)):
        for fn in (api.fc_packed_shape, api.fc_packed_galois_steps):
            with pytest.raises(api.HheError) as e:
                fn(n, rows, cols, lib=emu_lib)
            assert e.value.code == code, (n, rows, cols)
    # the capacity convention of hhe_affine_galois_steps
    out, cnt = (C.c_int * 2)(), C.c_size_t(2)
    assert emu_lib.hhe_fc_packed_galois_steps(C.c_size_t(1024), C.c_size_t(3), C.c_size_t(5), out, C.byref(cnt)) == api.ERR_CAPACITY
    assert cnt.value == 3


@pytest.mark.parametrize("rows,cols", [(3, 5), (1, 8), (4, 4), (8, 3), (10, 100), (5, 256)])
def test_diagonals_against_the_formula(api, emu_lib, rows, cols):
    M = fp.seeded_matrix(T, rows, cols, rows * 1000 + cols)
    got = api.fc_packed_diagonals(T, M, lib=emu_lib)
    want = np.array(fp.hand_diagonals(M, rows, cols), dtype=np.uint64)
    assert got.shape == want.shape and (got == want).all()
    # every entry of M sits in exactly one (diagonal, slot): the r diagonals tile the padded matrix
    assert int(got.astype(object).sum()) == int(M.astype(object).sum())


def test_diagonals_refuse_entries_not_below_t(api, emu_lib):
    M = fp.seeded_matrix(T, 3, 5, 1)
    M[2, 4] = T
    with pytest.raises(api.HheError) as e:
        api.fc_packed_diagonals(T, M, lib=emu_lib)
    assert e.value.code == api.ERR_INVALID


# ---- 2. the shapes at N = 1024, words and integers ----
@pytest.mark.parametrize("rows,cols,rc,ks", SHAPES)
def test_word_parity_and_integers(api, emu_lib, mem, S3, rows, cols, rc, ks):
    X = _ctx(api, emu_lib, S3)
    fp.check_layer(X, S3, mem, fp.seeded_matrix(T, rows, cols, 7 * rows + cols), B=2, seed=rows)
    assert X.query("fc_packed_key_switches") == ks
    X.close()


# ---- 3. a wider chain ----
def test_10_by_100_four_primes(orc, api, emu_lib, mem):
    S = fp.make_setup(orc, 10, orc.coeff_modulus_create(1024, [50] * 4))
    X = _ctx(api, emu_lib, S)
    assert fp.hand_shape(1024, 10, 100) == (16, 128)
    fp.check_layer(X, S, mem, fp.seeded_matrix(T, 10, 100, 3), B=2, seed=3)
    X.close()


# ---- 4. what the padded slots and the second row may hold ----
def test_padded_input_slots_may_hold_anything(api, emu_lib, mem, S3):
    """non-zero values in input slots [cols, c): the padded columns of the diagonals are zero, the integers stay (M x) mod t"""
    X = _ctx(api, emu_lib, S3)
    rng = np.random.default_rng(41)
    xs = [rng.integers(1, T, size=8, dtype=np.uint64) for _ in range(2)]   # c = 8 > cols = 5
    fp.check_layer(X, S3, mem, fp.seeded_matrix(T, 3, 5, 42), B=2, seed=4, xs=xs)
    X.close()


def test_both_rows_carry_an_input(api, emu_lib, mem, S3):
    """the diagonals encoded into both rows of the batching: two products per ciphertext"""
    X = _ctx(api, emu_lib, S3)
    rng = np.random.default_rng(43)
    xs = [rng.integers(0, T, size=5, dtype=np.uint64) for _ in range(2)]
    xs1 = [rng.integers(0, T, size=5, dtype=np.uint64) for _ in range(2)]
    fp.check_layer(X, S3, mem, fp.seeded_matrix(T, 3, 5, 44), B=2, seed=5, xs=xs, xs1=xs1, both_rows=True)
    X.close()


# ---- 5. the row kernels ----
def test_mnist_shape_on_the_row_kernels(orc, api, emu_lib, mem):
    """N = 4096, 3 x 60 bits, 10 x 784: r = 16, c = 1024 = N / 4, 22 key switches"""
    S = fp.make_setup(orc, 12, orc.coeff_modulus_create(4096, [60] * 3), steps=fp.hand_steps(4096, 10, 784))
    X = _ctx(api, emu_lib, S)
    assert X.query("row_kernel") == 1
    fp.check_layer(X, S, mem, fp.seeded_matrix(T, 10, 784, 5), B=1, seed=6)
    assert X.query("fc_packed_key_switches") == 22
    X.close()


# ---- 6. chunking and lifecycle ----
def test_chunks_and_streams_do_not_change_the_words(api, emu_lib, mem, S3, monkeypatch):
    fp.check_chunking(lambda: _ctx(api, emu_lib, S3), S3, mem, monkeypatch)


def test_in_place(api, emu_lib, mem, S3):
    X = _ctx(api, emu_lib, S3)
    fp.check_layer(X, S3, mem, fp.seeded_matrix(T, 3, 5, 62), B=3, seed=8, in_place=True)
    X.close()


def test_handles_two_on_a_context_two_threads_and_again(api, emu_lib, mem, S3):
    X = _ctx(api, emu_lib, S3)
    fp.check_handles(X, S3, mem)
    X.close()


# ---- 7. a level ----
def test_at_a_level(orc, api, emu_lib, mem):
    """N = 1024, 4 x 50 bits, level 2: input and diagonals switched with hhe_mod_switch, the key sets derived, the handle made on the
    level context; the truth is the oracle of the short chain under the projected keys"""
    S = lc.parent_setup(orc, "n1024_4x50")
    l, rows, cols = 2, 3, 5
    X = api.Context(S.logn, S.q, S.t, lib=emu_lib)
    top = lc.top_set(X, S)
    Xl = X.at_level(l)
    ks = Xl.keyset().derive_from(top)
    Sl = lc.level_setup(orc, api, S, l)
    M = fp.seeded_matrix(T, rows, cols, 81)
    xs = [np.random.default_rng(82).integers(0, T, size=cols, dtype=np.uint64) for _ in range(2)]
    d_W, W = lc.switched(X, S, mem, fp.encrypt_diagonals(S, M, seed=600), l)
    d_x, cts = lc.switched(X, S, mem, fp.encrypt_inputs(S, xs, seed=700), l)
    mat = Xl.enc_matrix(d_W, rows, cols)
    assert mat.bytes == 4 * 2 * (2 * l + 1) * S.n * 8
    got = mem.to_host(mat.apply(d_x, 2, rk=ks, gk=ks, out=mem.empty((2, 2, l, S.n))))
    for b in range(2):
        assert (got[b] == fp.fc_packed_ref(Sl.O, Sl.rk, Sl.gk, W, cts[b], rows, cols)).all(), b
        fp.check_slots(Sl, got[b], M, xs[b], what=("level", l, b))
    mat.destroy()
    ks.close()
    top.close()
    Xl.close()
    X.close()


# ---- 8. refusals: `out` prefilled and untouched ----
def test_refusals_leave_out_untouched(api, emu_lib, mem, S3):
    X, Y = _ctx(api, emu_lib, S3), _ctx(api, emu_lib, S3)
    fp.check_refusals(X, Y, S3, mem, api)
    Y.close()
    X.close()


# ---- 9. the sum of many ----
@pytest.mark.parametrize("size", [2, 3])
@pytest.mark.parametrize("K", [1, 2, 17, 512])
def test_add_many_against_integers(orc, api, emu_lib, mem, K, size):
    """60-bit primes, every word q_j - 1 (K = N / 2 of them: 2^69, far past a 64-bit running sum), alternating with 0, and random"""
    q = orc.coeff_modulus_create(1024, [60] * 3)
    assert all(int(v).bit_length() == 60 for v in q)
    X = api.Context(10, q, T, lib=emu_lib)
    for pattern in ("max", "alt", "rand"):
        fp.check_add_many(X, mem, q[:-1], K, 2 if K <= 17 else 1, size, pattern)
    X.close()


def test_add_many_refusals_and_in_place(orc, api, emu_lib, mem):
    q = orc.coeff_modulus_create(1024, [60] * 3)
    X = api.Context(10, q, T, lib=emu_lib)
    w = fp.add_many_words(q[:-1], 3, 2, 2, 1024, "rand")
    d = mem.to_dev(w)
    for K, B, size in ((0, 2, 2), (3, 0, 2), (3, 2, 1), (3, 2, 4)):
        with pytest.raises(api.HheError) as e:
            X.add_many(d, K, mem.empty((2, 2, 2, 1024)), B, size)
        assert e.value.code == api.ERR_INVALID
    X.add_many(d, 3, d, 2, 2)   # out = the first operand
    X.sync()
    got = mem.to_host(d)[0]
    for j, qj in enumerate(q[:-1]):
        assert (got[:, :, j, :] == (w[:, :, :, j, :].astype(object).sum(axis=0) % int(qj)).astype(np.uint64)).all()
    X.close()
