"""hhe_multiply_sum and hhe_fc_packed_sum_ks on the tests-only emulator (built with -DHHE_RANGE_CHECK, so a 128-bit sum of the kernel
that wraps aborts the run): the words against the restatement of mult_sum_common (held to the oracle's multiply at K = 1 first), the
distance to the rounded integer sum, the cap against Python integers, and the layer word for word against the oracle's composition
around the public hhe_multiply_sum and slot for slot against (M x) mod t."""
import ctypes as C

import numpy as np
import pytest

import definition_common as dc
import fc_packed_common as fp
import level_common as lc
import mult_sum_common as ms
import parity_common as pc
import rot_many_common as rmc

T = fp.T
PARAMS = {"n1024": (10, [50] * 3), "n4096": (12, [60] * 3)}


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


def _env(orc, name):
    logn, bits = PARAMS[name]
    return dc.env(orc, logn, orc.coeff_modulus_create(1 << logn, bits), T)


def _ctx(api, lib, E):
    return api.Context(E.logn, E.q, E.t, lib=lib)


# ---- 1. the restatement against the oracle, before it is trusted ----
@pytest.mark.parametrize("name", list(PARAMS))
def test_restatement_is_the_oracles_multiply_at_k1(orc, name):
    E = _env(orc, name)
    R = ms.restate(E)
    for i, (a, b) in enumerate(dc.behz_pairs(E, 5)):
        assert (R.multiply_sum(a[None], b[None]) == E.O.multiply(a, b)).all(), ("pair", i)


def test_sampled_restatement_is_the_full_one(orc):
    """the schoolbook form the GPU suite uses at N = 2^15, against the transform form, with a repeated pair"""
    E = _env(orc, "n1024")
    R = ms.restate(E)
    a, b = ms.operands(E, 3, 1, "rand", 6)
    a, b = np.concatenate([a, a[:1]])[:, 0], np.concatenate([b, b[:1]])[:, 0]
    idx = [0, E.n - 1] + list(dc.sample_indices(E.n, 3, 7))
    assert (R.multiply_sum_at(a, b, idx) == R.multiply_sum(a, b)[:, :, idx]).all()


# ---- 2. the cap and the intervals ----
@pytest.mark.parametrize("name", list(PARAMS))
def test_cap_and_intervals_against_python(orc, api, emu_lib, name):
    E = _env(orc, name)
    X = _ctx(api, emu_lib, E)
    cap = ms.check_cap(X, E)
    assert cap > E.n // 2
    assert X.query("multiply_sum_fold_q") == ms.hand_fold(E.q[:E.L])
    assert X.query("multiply_sum_fold_bsk") == ms.hand_fold(E.bsk) == 32   # 61-bit primes
    X.close()


# ---- 3. K = 1 is hhe_multiply ----
@pytest.mark.parametrize("name", list(PARAMS))
def test_k1_gives_the_words_of_multiply(orc, api, emu_lib, mem, name):
    E = _env(orc, name)
    X = _ctx(api, emu_lib, E)
    for pattern in ("enc", "max", "alt", "rand", "half"):
        a, b = ms.operands(E, 1, 3, pattern, 11)
        want = mem.empty((3, 3, E.L, E.n))
        X.multiply(mem.to_dev(a[0]), mem.to_dev(b[0]), want, 3)
        assert (ms.run(X, mem, a, b) == mem.to_host(want)).all(), pattern
    X.close()


# ---- 4. sums: every word against the restatement, the distance against integers ----
def _ks(orc, name):
    """2, 3, 16 and one above each reduction interval of the kernel"""
    E = _env(orc, name)
    return [2, 3, 16, ms.hand_fold(E.bsk) + 1, ms.hand_fold(E.q[:E.L]) + 1]


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("name", list(PARAMS))
def test_sums_against_the_restatement(orc, api, emu_lib, mem, name, which):
    E = _env(orc, name)
    K = _ks(orc, name)[which]
    X = _ctx(api, emu_lib, E)
    assert K <= ms.check_cap(X, E)
    if which >= 3:
        assert K == (X.query("multiply_sum_fold_bsk"), X.query("multiply_sum_fold_q"))[which - 3] + 1
    worst = 0
    for pattern in ("enc", "max", "alt", "rand", "half"):
        for B in ((1, 3) if K <= 3 else (1,)):
            worst = max(worst, ms.check_words(X, E, mem, K, B, pattern, seed=20 + which))
    print("worst summed BEHZ distance, %s, K = %d: %d (cap L + 1 = %d)" % (name, K, worst, E.L + 1))
    X.close()


@pytest.mark.parametrize("name", list(PARAMS))
def test_broadcast_equals_stacked(orc, api, emu_lib, mem, name):
    E = _env(orc, name)
    X = _ctx(api, emu_lib, E)
    a, b = ms.operands(E, 3, 3, "rand", 31)
    b1 = b[:, :1]
    stacked = np.broadcast_to(b1, b.shape).copy()
    assert (ms.run(X, mem, a, b1, bcast=True) == ms.run(X, mem, a, stacked)).all()
    X.close()


@pytest.mark.parametrize("name", list(PARAMS))
def test_order_of_the_pairs_does_not_matter(orc, api, emu_lib, mem, name):
    E = _env(orc, name)
    X = _ctx(api, emu_lib, E)
    a, b = ms.operands(E, 16, 1, "rand", 32)
    perm = np.random.default_rng(33).permutation(16)
    assert (perm != np.arange(16)).any()
    assert (ms.run(X, mem, a, b) == ms.run(X, mem, a[perm], b[perm])).all()
    X.close()


# ---- 5. the context that admits no sum ----
def test_refusal_context(orc, api, emu_lib, mem):
    """N = 1024, one 60-bit data prime and a special prime, t of 60 bits: the floored sum of two products no longer fits B_sk"""
    q = orc.coeff_modulus_create(1024, [60] * 2)
    E = dc.env(orc, 10, q, dc.T60)
    assert E.t == 1096486890805657601
    X = _ctx(api, emu_lib, E)
    assert ms.check_cap(X, E) < 2
    a, b = ms.operands(E, 2, 1, "enc", 41)
    out = mem.to_dev(np.full((1, 3, E.L, E.n), 12345, np.uint64))
    with pytest.raises(api.HheError) as e:
        X.multiply_sum(mem.to_dev(a), mem.to_dev(b), 2, out, 1)
    assert e.value.code == api.ERR_INVALID and "behz_sum_cap" in str(e.value)
    assert (mem.to_host(out) == 12345).all()
    want = mem.empty((1, 3, E.L, E.n))
    X.multiply(mem.to_dev(a[0]), mem.to_dev(b[0]), want, 1)
    assert (ms.run(X, mem, a[:1], b[:1]) == mem.to_host(want)).all()   # K = 1 is served, with hhe_multiply's words
    X.close()


def test_other_refusals(orc, api, emu_lib, mem):
    E = _env(orc, "n1024")
    X = _ctx(api, emu_lib, E)
    a, b = ms.operands(E, 2, 1, "rand", 42)
    d_a, d_b = mem.to_dev(a), mem.to_dev(b)

    def refused(aa, bb, K, B, out=None):
        out = mem.to_dev(np.full((1, 3, E.L, E.n), 12345, np.uint64)) if out is None else out
        keep = mem.to_host(out)
        with pytest.raises(api.HheError) as e:
            X.multiply_sum(aa, bb, K, out, B)
        assert e.value.code == api.ERR_INVALID
        assert (mem.to_host(out) == keep).all()
    refused(None, d_b, 2, 1)
    refused(d_a, None, 2, 1)
    refused(d_a, d_b, 0, 1)
    refused(d_a, d_b, 2, 0)
    with pytest.raises(api.HheError):
        X.multiply_sum(d_a, d_b, 2, None, 1)
    # out3 inside an operand: a [4][1][2][L][N] holds 8 L N words, out3 [1][3][L][N] laid over its tail
    big = mem.to_dev(np.concatenate([a, a]))
    flat = big.reshape(-1)
    tail = flat[flat.size - 3 * E.L * E.n:]
    refused(big, mem.to_dev(np.concatenate([b, b])), 4, 1, out=tail)
    refused(mem.to_dev(np.concatenate([b, b])), big, 4, 1, out=tail)
    X.close()


# ---- 6. the layer ----
@pytest.fixture(scope="module")
def S3(orc):
    """N = 1024, 3 x 50 bits, every default Galois key"""
    return fp.make_setup(orc, 10, orc.coeff_modulus_create(1024, [50] * 3))


def _lctx(api, lib, S):
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    S.load_keys(X)
    return X


@pytest.mark.parametrize("hoisted", [0, 1])
@pytest.mark.parametrize("rows,cols,rc,ks", fp.SHAPES)
def test_layer_words_slots_and_counters(api, emu_lib, mem, S3, rows, cols, rc, ks, hoisted):
    X = _lctx(api, emu_lib, S3)
    M = fp.seeded_matrix(T, rows, cols, 7 * rows + cols)
    got, _, xs = ms.check_sum_layer(X, S3, mem, M, hoisted, B=2, seed=rows)
    ms.check_sum_slots(S3, got, M, xs)
    X.close()


@pytest.mark.parametrize("hoisted", [0, 1])
def test_mnist_shape_on_the_row_kernels(orc, api, emu_lib, mem, hoisted):
    """N = 4096, 3 x 60 bits, 10 x 784: r = 16, c = 1024"""
    steps = sorted(set(fp.hand_steps(4096, 10, 784)) | set(rmc.hand_hoisted_steps(4096, 10, 784)))
    S = fp.make_setup(orc, 12, orc.coeff_modulus_create(4096, [60] * 3), steps=steps)
    X = _lctx(api, emu_lib, S)
    assert X.query("row_kernel") == 1
    M = fp.seeded_matrix(T, 10, 784, 5)
    got, _, xs = ms.check_sum_layer(X, S, mem, M, hoisted, B=1, seed=6)
    ms.check_sum_slots(S, got, M, xs)
    X.close()


@pytest.mark.parametrize("hoisted", [0, 1])
def test_chunks_and_streams_do_not_change_the_words(api, emu_lib, mem, S3, monkeypatch, hoisted):
    M = fp.seeded_matrix(T, 3, 5, 61)
    X = _lctx(api, emu_lib, S3)
    got, refs, xs = ms.check_sum_layer(X, S3, mem, M, hoisted, B=5, seed=7)
    ms.check_sum_slots(S3, got, M, xs)
    X.close()
    for chunk, streams in (("2", "2"), ("8", "0")):
        monkeypatch.setenv("HHE_CHUNK", chunk)
        monkeypatch.setenv("HHE_STREAMS", streams)
        Y = _lctx(api, emu_lib, S3)
        g2, _, _ = ms.check_sum_layer(Y, S3, mem, M, hoisted, B=5, seed=7, refs=refs)
        assert (g2 == got).all(), (chunk, streams)
        Y.close()


@pytest.mark.parametrize("hoisted", [0, 1])
def test_in_place(api, emu_lib, mem, S3, hoisted):
    X = _lctx(api, emu_lib, S3)
    M = fp.seeded_matrix(T, 3, 5, 62)
    got, _, xs = ms.check_sum_layer(X, S3, mem, M, hoisted, B=3, seed=8, in_place=True)
    ms.check_sum_slots(S3, got, M, xs)
    X.close()


def test_forced_fallback_of_the_hoisted_rotation(api, emu_lib, mem, S3, monkeypatch):
    M = fp.seeded_matrix(T, 3, 5, 63)
    X = _lctx(api, emu_lib, S3)
    got, refs, _ = ms.check_sum_layer(X, S3, mem, M, 1, B=3, seed=9)
    X.close()
    monkeypatch.setenv("HHE_ROT_HOIST", "2")
    Y = _lctx(api, emu_lib, S3)
    assert Y.query("rot_hoist") == 2
    before = Y.query("rot_many_fallbacks")
    g2, _, _ = ms.check_sum_layer(Y, S3, mem, M, 1, B=3, seed=9, refs=refs)
    assert Y.query("rot_many_fallbacks") > before
    assert (g2 == got).all()
    Y.close()


@pytest.mark.parametrize("hoisted", [0, 1])
def test_at_a_level(orc, api, emu_lib, mem, hoisted):
    """N = 1024, 4 x 50 bits, level 2, derived key sets; the truth is the oracle of the short chain under the projected keys"""
    S = lc.parent_setup(orc, "n1024_4x50")
    l, rows, cols = 2, 3, 5
    X = api.Context(S.logn, S.q, S.t, lib=emu_lib)
    top = lc.top_set(X, S)
    Xl = X.at_level(l)
    ks = Xl.keyset().derive_from(top)
    Sl = lc.level_setup(orc, api, S, l)
    ms.check_cap(Xl, dc.env(orc, Sl.logn, Sl.q, Sl.t))
    M = fp.seeded_matrix(T, rows, cols, 81)
    xs = [np.random.default_rng(82).integers(0, T, size=cols, dtype=np.uint64) for _ in range(2)]
    _, W = lc.switched(X, S, mem, fp.encrypt_diagonals(S, M, seed=600), l)
    _, cts = lc.switched(X, S, mem, fp.encrypt_inputs(S, xs, seed=700), l)
    got, _, _ = ms.check_sum_layer(Xl, Sl, mem, M, hoisted, B=2, rk=ks, gk=ks, O=Sl.O, keys=(Sl.rk, Sl.gk), data=(W, cts, xs))
    ms.check_sum_slots(Sl, got, M, xs)
    ks.close()
    top.close()
    Xl.close()
    X.close()


@pytest.mark.parametrize("hoisted", [0, 1])
def test_layer_refusals_leave_out_untouched(api, emu_lib, mem, S3, hoisted):
    """the refusals of hhe_fc_packed_ks, through the new entry"""
    X, Y = _lctx(api, emu_lib, S3), _lctx(api, emu_lib, S3)
    O = S3.O
    rows, cols = 3, 5   # steps -8, +1 (or 1 .. 3), 4
    M = fp.seeded_matrix(T, rows, cols, 91)
    d_W = mem.to_dev(fp.encrypt_diagonals(S3, M, seed=800))
    d_in = mem.to_dev(fp.encrypt_inputs(S3, [np.arange(cols, dtype=np.uint64)], seed=900))
    mat = X.enc_matrix(d_W, rows, cols)
    elt = {int(e): k for e, k in zip(S3.gk.elts, S3.gk.keys)}

    def refused(code, text, B=1, **kw):
        out = mem.to_dev(np.full((1,) + O.ct_shape, 12345, np.uint64))
        with pytest.raises(api.HheError) as e:
            mat.apply_sum(d_in, B, out=out, hoisted=hoisted, **kw)
        assert e.value.code == code and text in str(e.value), (code, str(e.value))
        assert (mem.to_host(out) == 12345).all()

    own = (-8, 4)   # the steps both forms need a key of their own for
    for missing in own:
        ks = X.keyset().set_relin(S3.rk)
        for s in (-8, 1, 2, 4):
            if s != missing:
                ks.set_galois(int(O.galois_elt(s)), elt[int(O.galois_elt(s))])
        refused(api.ERR_NO_GALOIS_KEY, "Galois key not present", rk=ks, gk=ks)
        ks.close()
    full = X.keyset().set_relin(S3.rk)
    for s in (-8, 1, 2, 4):
        full.set_galois(int(O.galois_elt(s)), elt[int(O.galois_elt(s))])
    norelin = X.keyset()
    refused(api.ERR_NO_RELIN_KEY, "relinearization key not set", rk=norelin, gk=full)
    norelin.close()
    full.close()
    refused(api.ERR_INVALID, "empty batch", B=0)
    yks = Y.keyset().set_relin(S3.rk)
    refused(api.ERR_INVALID, "another context", rk=yks)
    yks.close()
    other = Y.enc_matrix(d_W, rows, cols)
    out = mem.to_dev(np.full((1,) + O.ct_shape, 12345, np.uint64))
    assert X.lib.hhe_fc_packed_sum_ks(X.h, None, None, other.h, api._ptr(d_in), api._ptr(out), C.c_size_t(1), C.c_int(hoisted)) == api.ERR_INVALID
    assert b"another context" in X.lib.hhe_last_error() and (mem.to_host(out) == 12345).all()
    assert X.lib.hhe_fc_packed_sum_ks(X.h, None, None, mat.h, None, api._ptr(out), C.c_size_t(1), C.c_int(hoisted)) == api.ERR_INVALID
    other.destroy()
    mat.destroy()
    Y.close()
    X.close()


def test_layer_refused_above_the_cap(orc, api, emu_lib, mem):
    """the refusal context: r = 4 diagonals above a cap below 2; r = 1 is served"""
    q = orc.coeff_modulus_create(1024, [60] * 2)
    S = fp.make_setup(orc, 10, q, t=dc.T60)
    X = _lctx(api, emu_lib, S)
    assert X.query("behz_sum_cap") < 2
    M = fp.seeded_matrix(S.t, 3, 5, 92)
    mat = X.enc_matrix(mem.to_dev(fp.encrypt_diagonals(S, M, seed=810)), 3, 5)
    d_in = mem.to_dev(fp.encrypt_inputs(S, [np.arange(5, dtype=np.uint64)], seed=910))
    for hoisted in (False, True):
        out = mem.to_dev(np.full((1,) + S.O.ct_shape, 12345, np.uint64))
        with pytest.raises(api.HheError) as e:
            mat.apply_sum(d_in, 1, out=out, hoisted=hoisted)
        assert e.value.code == api.ERR_INVALID and "behz_sum_cap" in str(e.value)
        assert (mem.to_host(out) == 12345).all()
    mat.destroy()
    M1 = fp.seeded_matrix(S.t, 1, 8, 93)
    one = X.enc_matrix(mem.to_dev(fp.encrypt_diagonals(S, M1, seed=820)), 1, 8)
    cts = fp.encrypt_inputs(S, [np.arange(8, dtype=np.uint64)], seed=920)
    a = mem.to_host(one.apply(mem.to_dev(cts), 1, out=mem.empty((1,) + S.O.ct_shape)))
    b = mem.to_host(one.apply_sum(mem.to_dev(cts), 1, out=mem.empty((1,) + S.O.ct_shape)))
    assert (a == b).all()   # r = 1: one product, the words of hhe_fc_packed_ks
    one.destroy()
    X.close()
