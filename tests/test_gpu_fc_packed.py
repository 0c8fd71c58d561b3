"""Packed encrypted FC layer and hhe_add_many on the device: the shapes, chunking, lifecycle and refusals of the emulator suite on
the separate-kernel path, the row kernels at N = 4096, BFVDefault(4096), and the deployed parameter set BFVDefault(16384) with the
10 x 784 MNIST layer -- word for word against the oracle's composition of the definition (tests/fc_packed_common.py), slot for slot
against plain integers, and against hhe_fc_row_ks on the same inputs.  Run on an MI355X: python -m pytest tests -m gpu."""
import json
import os

import numpy as np
import pytest

import fc_packed_common as fp
import level_common as lc
import parity_common as pc

pytestmark = pytest.mark.gpu
T = fp.T
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = fp.SHAPES


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


def _ctx(api, lib, S, row_kernel=None):
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    if row_kernel is not None:
        assert X.query("row_kernel") == row_kernel
    S.load_keys(X)
    return X


def _mnist(count):
    """(M [10][784] mod t, pixels [count][784], plain logits [count][10]) of the fixtures"""
    fx = json.load(open(os.path.join(HERE, "golden", "mnist_64.json")))
    W = np.array(json.load(open(os.path.join(HERE, "golden", "mnist_1fc.json")))["weights_rows"], dtype=np.int64)
    packed = np.array([list(bytes.fromhex(h)) for h in fx["pixels_2bit_hex"][:count]], dtype=np.uint8)
    pix = ((packed[:, :, None] >> (2 * np.arange(4))) & 3).reshape(count, 784).astype(np.int64)
    assert (pix @ W.T == np.array(fx["plain_logits"][:count])).all()
    return (W % T).astype(np.uint64), pix.astype(np.uint64), np.array(fx["plain_logits"][:count])


# ---- the shapes at N = 1024 (separate kernels), words and integers ----
@pytest.mark.parametrize("rows,cols,rc,ks", SHAPES)
def test_word_parity_and_integers(api, lib, mem, S3, rows, cols, rc, ks):
    X = _ctx(api, lib, S3, 0)
    fp.check_layer(X, S3, mem, fp.seeded_matrix(T, rows, cols, 7 * rows + cols), B=2, seed=rows)
    assert X.query("fc_packed_key_switches") == ks
    X.close()


def test_padded_slots_and_both_rows(api, lib, mem, S3):
    X = _ctx(api, lib, S3)
    rng = np.random.default_rng(41)
    xs = [rng.integers(1, T, size=8, dtype=np.uint64) for _ in range(2)]   # c = 8 > cols = 5: slots [cols, c) hold anything
    fp.check_layer(X, S3, mem, fp.seeded_matrix(T, 3, 5, 42), B=2, seed=4, xs=xs)
    xs = [rng.integers(0, T, size=5, dtype=np.uint64) for _ in range(2)]
    xs1 = [rng.integers(0, T, size=5, dtype=np.uint64) for _ in range(2)]
    fp.check_layer(X, S3, mem, fp.seeded_matrix(T, 3, 5, 44), B=2, seed=5, xs=xs, xs1=xs1, both_rows=True)
    X.close()


def test_chunks_and_streams_do_not_change_the_words(api, lib, mem, S3, monkeypatch):
    fp.check_chunking(lambda: _ctx(api, lib, S3), S3, mem, monkeypatch)


def test_in_place_and_handles(api, lib, mem, S3):
    X = _ctx(api, lib, S3)
    fp.check_layer(X, S3, mem, fp.seeded_matrix(T, 3, 5, 62), B=3, seed=8, in_place=True)
    fp.check_handles(X, S3, mem)
    X.close()


def test_refusals_leave_out_untouched(api, lib, mem, S3):
    X, Y = _ctx(api, lib, S3), _ctx(api, lib, S3)
    fp.check_refusals(X, Y, S3, mem, api)
    Y.close()
    X.close()


# ---- the row kernels, and the separate kernels at full tiles ----
def test_mnist_shape_on_the_row_kernels(orc, api, lib, mem):
    """N = 4096, 3 x 60 bits, 10 x 784: r = 16, c = 1024 = N / 4, 22 key switches"""
    S = fp.make_setup(orc, 12, orc.coeff_modulus_create(4096, [60] * 3), steps=fp.hand_steps(4096, 10, 784))
    X = _ctx(api, lib, S, 1)
    fp.check_layer(X, S, mem, fp.seeded_matrix(T, 10, 784, 5), B=1, seed=6)
    assert X.query("fc_packed_key_switches") == 22
    X.close()


def test_bfv_default_4096(orc, api, lib, mem):
    """BFVDefault(4096), 36 + 36 + 37 bits: no pseudo-Mersenne form, the separate-kernel path at full tiles (17 bits of budget left)"""
    S = fp.make_setup(orc, 12, api.bfv_default_coeff_modulus(4096, lib), steps=fp.hand_steps(4096, 3, 5))
    X = _ctx(api, lib, S, 0)
    fp.check_layer(X, S, mem, fp.seeded_matrix(T, 3, 5, 9), B=2, seed=1)
    X.close()


# ---- the deployed parameter set ----
def test_deployed_parameters_words(api, lib, mem, S16):
    """BFVDefault(16384), 10 x 784, one item word for word against the oracle"""
    X = _ctx(api, lib, S16, 1)
    M, pix, _ = _mnist(1)
    fp.check_layer(X, S16, mem, M, B=1, seed=11, xs=[pix[0]])
    assert X.query("fc_packed_key_switches") == 22
    X.close()


def test_deployed_parameters_mnist_against_integers_and_fc_row(api, lib, mem, S16):
    """four MNIST images under the fixture's weights: the ten logits of every image against plain integers mod t and against slot
    n - 1 of hhe_fc_row_ks on the same inputs; the device's noise budget is positive"""
    S, O = S16, S16.O
    NS, n_in = 4, 784
    M, pix, plain = _mnist(NS)
    X = _ctx(api, lib, S, 1)
    d_x = mem.to_dev(fp.encrypt_inputs(S, list(pix), seed=1100))
    mat = X.enc_matrix(mem.to_dev(fp.encrypt_diagonals(S, M, seed=1200)), 10, n_in)
    assert mat.bytes == 16 * 2 * 17 * (1 << 14) * 8
    out = mat.apply(d_x, NS, out=mem.empty((NS,) + O.ct_shape))
    assert (X.noise_budget(S.sk, out, NS) > 0).all()
    vals = mem.empty((NS, O.n))
    X.decrypt(S.sk, out, NS, vals)
    logits = mem.to_host(vals)[:, :10].astype(np.int64)
    assert (logits == plain % T).all()
    # the same layer row by row: item = (sample, neuron)
    wcs = mem.to_dev(np.stack([O.encrypt(S.pk, O.encode(M[r]), 1300 + r) for r in range(10)]))
    vi = d_x.repeat_interleave(10, dim=0).contiguous()
    rows_out = mem.empty((NS * 10,) + O.ct_shape)
    X.fc_row(vi, wcs, 10, n_in, rows_out, NS * 10)   # the context's default set: the same key objects
    rvals = mem.empty((NS * 10, O.n))
    X.decrypt(S.sk, rows_out, NS * 10, rvals)
    assert (mem.to_host(rvals)[:, n_in - 1].astype(np.int64).reshape(NS, 10) == logits).all()
    mat.destroy()
    X.close()


def test_deployed_parameters_at_level_4(orc, api, lib, mem, S16):
    """BFVDefault(16384) at level 4: input and diagonals switched on the parent, key sets derived, the handle made on the level's
    context; the truth is the oracle of the short chain under the projected keys"""
    S, l, rows, cols = S16, 4, 10, 784
    M, pix, plain = _mnist(1)
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    top = lc.top_set(X, S)
    Xl = X.at_level(l)
    assert Xl.query("row_kernel") == 1
    ks = Xl.keyset().derive_from(top)
    Sl = lc.level_setup(orc, api, S, l)
    d_W, W = lc.switched(X, S, mem, fp.encrypt_diagonals(S, M, seed=1400), l)
    d_x, cts = lc.switched(X, S, mem, fp.encrypt_inputs(S, [pix[0]], seed=1500), l)
    mat = Xl.enc_matrix(d_W, rows, cols)
    got = mem.to_host(mat.apply(d_x, 1, rk=ks, gk=ks, out=mem.empty((1, 2, l, S.n))))
    assert (got[0] == fp.fc_packed_ref(Sl.O, Sl.rk, Sl.gk, W, cts[0], rows, cols)).all()
    fp.check_slots(Sl, got[0], M, pix[0], what=("level", l))
    mat.destroy()
    ks.close()
    top.close()
    Xl.close()
    X.close()


# ---- the sum of many ----
@pytest.mark.parametrize("size", [2, 3])
@pytest.mark.parametrize("K", [1, 2, 17, 512])
def test_add_many_against_integers(orc, api, lib, mem, K, size):
    """N = 1024, 60-bit primes: every word q_j - 1, alternating with 0, and random; one launch per call"""
    q = orc.coeff_modulus_create(1024, [60] * 3)
    X = api.Context(10, q, T, lib=lib)
    for pattern in ("max", "alt", "rand"):
        fp.check_add_many(X, mem, q[:-1], K, 2 if K <= 17 else 1, size, pattern)
    X.close()


def test_add_many_benchmarked_degree_worst_case(orc, api, lib, mem):
    """N = 2^15 over 4 x 60 bits, K = 16: more than one workgroup per polynomial, every word at q_j - 1"""
    q = orc.coeff_modulus_create(1 << 15, [60] * 4)
    X = api.Context(15, q, T, lib=lib)
    fp.check_add_many(X, mem, q[:-1], 16, 1, 3, "max")
    fp.check_add_many(X, mem, q[:-1], 16, 1, 2, "alt")
    X.close()
