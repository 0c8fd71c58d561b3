"""hhe_multiply_sum and hhe_fc_packed_sum_ks on the device: the cases of the emulator suite (tests/test_mult_sum_emu.py) on the kernels,
the summed product at the benchmarked degree N = 2^15, BFVDefault(4096), and the deployed parameter set BFVDefault(16384) with the
10 x 784 MNIST layer -- words against the restatement of tests/mult_sum_common.py and the composition around the public
hhe_multiply_sum, slots against plain integers and against hhe_fc_packed_ks.  Run on an MI355X: python -m pytest tests -m gpu."""
import json
import os

import numpy as np
import pytest

import definition_common as dc
import fc_packed_common as fp
import level_common as lc
import mult_sum_common as ms
import parity_common as pc
import rot_many_common as rmc

pytestmark = pytest.mark.gpu
T = fp.T
HERE = os.path.dirname(os.path.abspath(__file__))
PARAMS = {"n1024": (10, [50] * 3), "n4096": (12, [60] * 3)}


@pytest.fixture(scope="module")
def mem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pc.TorchMem("cuda:0")


@pytest.fixture(scope="module")
def lib(api):
    lib = api.load_library()  # fails loudly if the HIP library is missing
    assert lib.hhe_backend() == b"hip-gfx950"
    return lib


@pytest.fixture(scope="module")
def S3(orc):
    """N = 1024, 3 x 50 bits, every default Galois key"""
    return fp.make_setup(orc, 10, orc.coeff_modulus_create(1024, [50] * 3))


@pytest.fixture(scope="module")
def S16(orc, api, lib):
    """BFVDefault(16384), every default Galois key: the parameter set that decrypts"""
    return fp.make_setup(orc, 14, api.bfv_default_coeff_modulus(1 << 14, lib))


def _env(orc, name):
    logn, bits = PARAMS[name]
    return dc.env(orc, logn, orc.coeff_modulus_create(1 << logn, bits), T)


def _lctx(api, lib, S, row_kernel=None):
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    if row_kernel is not None:
        assert X.query("row_kernel") == row_kernel
    S.load_keys(X)
    return X


# ---- hhe_multiply_sum at N = 1024 and N = 4096 ----
@pytest.mark.parametrize("name", list(PARAMS))
def test_k1_cap_and_intervals(orc, api, lib, mem, name):
    E = _env(orc, name)
    X = api.Context(E.logn, E.q, E.t, lib=lib)
    assert ms.check_cap(X, E) > E.n // 2
    assert X.query("multiply_sum_fold_q") == ms.hand_fold(E.q[:E.L]) and X.query("multiply_sum_fold_bsk") == ms.hand_fold(E.bsk)
    for pattern in ("enc", "max", "alt", "rand", "half"):
        a, b = ms.operands(E, 1, 3, pattern, 11)
        want = mem.empty((3, 3, E.L, E.n))
        X.multiply(mem.to_dev(a[0]), mem.to_dev(b[0]), want, 3)
        assert (ms.run(X, mem, a, b) == mem.to_host(want)).all(), pattern
    X.close()


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("name", list(PARAMS))
def test_sums_against_the_restatement(orc, api, lib, mem, name, which):
    """K = 2, 3, 16 and one above each reduction interval; encryptions, q_j - 1 everywhere, alternating with 0, uniform,
    (Q - 1) / 2 everywhere; B = 1 and 3"""
    E = _env(orc, name)
    K = [2, 3, 16, ms.hand_fold(E.bsk) + 1, ms.hand_fold(E.q[:E.L]) + 1][which]
    X = api.Context(E.logn, E.q, E.t, lib=lib)
    worst = 0
    for pattern in ("enc", "max", "alt", "rand", "half"):
        for B in ((1, 3) if K <= 3 else (1,)):
            worst = max(worst, ms.check_words(X, E, mem, K, B, pattern, seed=20 + which))
    print("worst summed BEHZ distance, %s, K = %d: %d (cap L + 1 = %d)" % (name, K, worst, E.L + 1))
    X.close()


@pytest.mark.parametrize("name", list(PARAMS))
def test_broadcast_and_order(orc, api, lib, mem, name):
    E = _env(orc, name)
    X = api.Context(E.logn, E.q, E.t, lib=lib)
    a, b = ms.operands(E, 3, 3, "rand", 31)
    b1 = b[:, :1]
    assert (ms.run(X, mem, a, b1, bcast=True) == ms.run(X, mem, a, np.broadcast_to(b1, b.shape).copy())).all()
    a, b = ms.operands(E, 16, 1, "rand", 32)
    perm = np.random.default_rng(33).permutation(16)
    assert (ms.run(X, mem, a, b) == ms.run(X, mem, a[perm], b[perm])).all()
    X.close()


def test_refusal_context(orc, api, lib, mem):
    q = orc.coeff_modulus_create(1024, [60] * 2)
    E = dc.env(orc, 10, q, dc.T60)
    X = api.Context(E.logn, E.q, E.t, lib=lib)
    assert ms.check_cap(X, E) < 2
    a, b = ms.operands(E, 2, 1, "enc", 41)
    out = mem.to_dev(np.full((1, 3, E.L, E.n), 12345, np.uint64))
    with pytest.raises(api.HheError) as e:
        X.multiply_sum(mem.to_dev(a), mem.to_dev(b), 2, out, 1)
    assert e.value.code == api.ERR_INVALID and (mem.to_host(out) == 12345).all()
    for args in ((None, mem.to_dev(b), 2, out, 1), (mem.to_dev(a), mem.to_dev(b), 0, out, 1), (mem.to_dev(a), mem.to_dev(b), 2, out, 0)):
        with pytest.raises(api.HheError):
            X.multiply_sum(*args)
    assert (mem.to_host(out) == 12345).all()
    want = mem.empty((1, 3, E.L, E.n))
    X.multiply(mem.to_dev(a[0]), mem.to_dev(b[0]), want, 1)
    assert (ms.run(X, mem, a[:1], b[:1]) == mem.to_host(want)).all()
    X.close()


# ---- the benchmarked degree ----
@pytest.mark.parametrize("which", [0, 1, 2])
def test_benchmarked_degree_worst_case(orc, api, lib, mem, which):
    """N = 2^15 over 4 x 60 bits, every word q_j - 1: K = 16 and one above each interval; the distance and the restatement's words at
    sampled coefficients (schoolbook products: no transform on the truth's side)"""
    q = orc.coeff_modulus_create(1 << 15, [60] * 4)
    E = dc.env(orc, 15, q, T)
    X = api.Context(15, q, T, lib=lib)
    K = [16, X.query("multiply_sum_fold_bsk") + 1, X.query("multiply_sum_fold_q") + 1][which]
    assert K == [16, 33, 129][which] and K <= ms.check_cap(X, E)
    a, b = ms.operands(E, K, 1, "max", 0)
    got = ms.run(X, mem, a, b)[0]
    idx = [0, E.n - 1] + list(dc.sample_indices(E.n, 2, 50 + which))
    want = ms.restate(E).multiply_sum_at(a[:, 0], b[:, 0], idx)
    assert (got[:, :, idx] == want).all()
    dist = ms.sum_distance(E, a[:, 0], b[:, 0], got, idx)
    print("summed BEHZ distance, N = 32768, L = 3, K = %d, max: %d" % (K, dist))
    assert dist <= E.L + 1
    X.close()


# ---- the layer ----
@pytest.mark.parametrize("hoisted", [0, 1])
@pytest.mark.parametrize("rows,cols,rc,ks", fp.SHAPES)
def test_layer_words_slots_and_counters(api, lib, mem, S3, rows, cols, rc, ks, hoisted):
    X = _lctx(api, lib, S3, 0)
    M = fp.seeded_matrix(T, rows, cols, 7 * rows + cols)
    got, _, xs = ms.check_sum_layer(X, S3, mem, M, hoisted, B=2, seed=rows)
    ms.check_sum_slots(S3, got, M, xs)
    X.close()


@pytest.mark.parametrize("hoisted", [0, 1])
def test_mnist_shape_on_the_row_kernels(orc, api, lib, mem, hoisted):
    steps = sorted(set(fp.hand_steps(4096, 10, 784)) | set(rmc.hand_hoisted_steps(4096, 10, 784)))
    S = fp.make_setup(orc, 12, orc.coeff_modulus_create(4096, [60] * 3), steps=steps)
    X = _lctx(api, lib, S, 1)
    M = fp.seeded_matrix(T, 10, 784, 5)
    got, _, xs = ms.check_sum_layer(X, S, mem, M, hoisted, B=1, seed=6)
    ms.check_sum_slots(S, got, M, xs)
    X.close()


@pytest.mark.parametrize("hoisted", [0, 1])
def test_chunks_streams_and_in_place(api, lib, mem, S3, monkeypatch, hoisted):
    M = fp.seeded_matrix(T, 3, 5, 61)
    X = _lctx(api, lib, S3)
    got, refs, xs = ms.check_sum_layer(X, S3, mem, M, hoisted, B=5, seed=7)
    ms.check_sum_slots(S3, got, M, xs)
    g1, _, _ = ms.check_sum_layer(X, S3, mem, M, hoisted, B=5, seed=7, refs=refs, in_place=True)
    assert (g1 == got).all()
    X.close()
    for chunk, streams in (("2", "2"), ("8", "0")):
        monkeypatch.setenv("HHE_CHUNK", chunk)
        monkeypatch.setenv("HHE_STREAMS", streams)
        Y = _lctx(api, lib, S3)
        g2, _, _ = ms.check_sum_layer(Y, S3, mem, M, hoisted, B=5, seed=7, refs=refs)
        assert (g2 == got).all(), (chunk, streams)
        Y.close()


def test_forced_fallback_of_the_hoisted_rotation(api, lib, mem, S3, monkeypatch):
    M = fp.seeded_matrix(T, 3, 5, 63)
    X = _lctx(api, lib, S3)
    got, refs, _ = ms.check_sum_layer(X, S3, mem, M, 1, B=3, seed=9)
    X.close()
    monkeypatch.setenv("HHE_ROT_HOIST", "2")
    Y = _lctx(api, lib, S3)
    before = Y.query("rot_many_fallbacks")
    g2, _, _ = ms.check_sum_layer(Y, S3, mem, M, 1, B=3, seed=9, refs=refs)
    assert Y.query("rot_many_fallbacks") > before and (g2 == got).all()
    Y.close()


@pytest.mark.parametrize("hoisted", [0, 1])
def test_at_a_level(orc, api, lib, mem, hoisted):
    S = lc.parent_setup(orc, "n1024_4x50")
    l, rows, cols = 2, 3, 5
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    top = lc.top_set(X, S)
    Xl = X.at_level(l)
    ks = Xl.keyset().derive_from(top)
    Sl = lc.level_setup(orc, api, S, l)
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
def test_bfv_default_4096(orc, api, lib, mem, hoisted):
    """BFVDefault(4096), 36 + 36 + 37 bits, 3 x 5: the separate-kernel path at full tiles"""
    steps = sorted(set(fp.hand_steps(4096, 3, 5)) | set(rmc.hand_hoisted_steps(4096, 3, 5)))
    S = fp.make_setup(orc, 12, api.bfv_default_coeff_modulus(4096, lib), steps=steps)
    X = _lctx(api, lib, S, 0)
    M = fp.seeded_matrix(T, 3, 5, 9)
    got, _, xs = ms.check_sum_layer(X, S, mem, M, hoisted, B=2, seed=1)
    ms.check_sum_slots(S, got, M, xs)
    X.close()


# ---- the deployed parameter set ----
def _mnist(count):
    """(M [10][784] mod t, pixels [count][784], plain logits [count][10]) of the fixtures"""
    fx = json.load(open(os.path.join(HERE, "golden", "mnist_64.json")))
    W = np.array(json.load(open(os.path.join(HERE, "golden", "mnist_1fc.json")))["weights_rows"], dtype=np.int64)
    packed = np.array([list(bytes.fromhex(h)) for h in fx["pixels_2bit_hex"][:count]], dtype=np.uint8)
    pix = ((packed[:, :, None] >> (2 * np.arange(4))) & 3).reshape(count, 784).astype(np.int64)
    assert (pix @ W.T == np.array(fx["plain_logits"][:count])).all()
    return (W % T).astype(np.uint64), pix.astype(np.uint64), np.array(fx["plain_logits"][:count])


def test_deployed_parameters_mnist(api, lib, mem, S16):
    """BFVDefault(16384), four MNIST images, both forms: the ten logits against plain integers mod t and against the slots of
    hhe_fc_packed_ks; the device's noise budget is positive"""
    S, O = S16, S16.O
    NS = 4
    M, pix, plain = _mnist(NS)
    X = _lctx(api, lib, S, 1)
    assert X.query("behz_sum_cap") > S.n // 2
    d_x = mem.to_dev(fp.encrypt_inputs(S, list(pix), seed=1100))
    mat = X.enc_matrix(mem.to_dev(fp.encrypt_diagonals(S, M, seed=1200)), 10, 784)

    def logits(ct):
        vals = mem.empty((NS, O.n))
        X.decrypt(S.sk, ct, NS, vals)
        return mem.to_host(vals)[:, :10].astype(np.int64)
    ref = logits(mat.apply(d_x, NS, out=mem.empty((NS,) + O.ct_shape)))
    assert X.query("fc_packed_floors") == 48
    for hoisted in (False, True):
        out = mat.apply_sum(d_x, NS, out=mem.empty((NS,) + O.ct_shape), hoisted=hoisted)
        assert X.query("fc_packed_floors") == 3
        budget = X.noise_budget(S.sk, out, NS)
        print("noise budget of hhe_fc_packed_sum_ks, hoisted = %d: %s" % (hoisted, [int(v) for v in budget]))
        assert (budget > 0).all()
        got = logits(out)
        assert (got == plain % T).all() and (got == ref).all(), hoisted
    mat.destroy()
    X.close()
