"""Packed plain-matrix affine layers on the device (hhe_matrix_create / hhe_packed_affine_ks): the benchmarked and the deployed
parameter sets, the fallback path, the full-packed row and a dimension that is not a power of two, word for word against the Python
restatement of SEALZpCipher::packed_matMul / packed_affine (tests/affine_common.py), plus the reference's own kind of end-to-end
check: the decryption equals (M x + b) mod t for real inputs.  Run on an MI355X: python -m pytest tests -m gpu."""
import json
import os

import numpy as np
import pytest

import affine_common as ac
import parity_common as pc

pytestmark = pytest.mark.gpu
T = 65537
HERE = os.path.dirname(os.path.abspath(__file__))


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


def _both_methods(orc, api, lib, mem, logn, q, dim, bsgs, row_kernel, B=3, vals=None, seed=0):
    """diagonal and BSGS with bias on one context; returns (Setup, context, inputs' slot values, outputs per method)"""
    n = 1 << logn
    S = ac.make_setup(orc, logn, q, T, ac.hand_steps(n, dim, *bsgs))
    X = api.Context(logn, q, T, lib=lib)
    assert X.query("row_kernel") == row_kernel
    S.load_keys(X)
    M, b = ac.seeded_matrix(T, dim, 100 + seed)
    cts, xs = ac.inputs(S, dim, B, seed, vals=vals)
    outs = {}
    for method in (None, bsgs):
        outs[method], _ = ac.check_affine(X, S, mem, M, b, method, B=B, cts=cts, in_place=method is not None)
    return S, X, M, b, xs, outs


def test_benchmarked_parameters_two_chunks(orc, api, lib, mem, monkeypatch):
    """N = 2^15, 4 x 60 bits, dim = 128, three items over two chunks: the row-kernel loop and BSGS 16 x 8, both with bias"""
    monkeypatch.setenv("HHE_CHUNK", "2")
    q = orc.coeff_modulus_create(1 << 15, [60] * 4)
    S, X, *_ = _both_methods(orc, api, lib, mem, 15, q, 128, (16, 8), 1, seed=1)
    X.profile(True)
    M, b = ac.seeded_matrix(T, 128, 101)
    mat = X.matrix(M, bias=b)
    assert mat.nbytes == (2 * 128 * 3 + 1) * (1 << 15) * 8   # 201 MB of multipliers and quotients + the bias
    d = mem.to_dev(ac.inputs(S, 128, 3, 1)[0])
    X.packed_affine(d, mat, d, 3)
    _, launches, _, items = X.profile_read()
    assert launches == 2 * 127 and items == 3 * 127   # ks_row_kernel: dim - 1 launches per chunk
    mat.close()
    X.close()


def test_deployed_parameters_words_and_decryption(orc, api, lib, mem):
    """N = 2^14, BFVDefault(16384), L = 8: word parity, and hhe_decrypt(out)[0:dim] == (M x + b) mod t for the first 128 pixels of three
    MNIST images (tests/golden/mnist_64.json)"""
    fx = json.load(open(os.path.join(HERE, "golden", "mnist_64.json")))
    packed = np.array([list(bytes.fromhex(h)) for h in fx["pixels_2bit_hex"][:3]], dtype=np.uint8)
    pix = ((packed[:, :, None] >> (2 * np.arange(4))) & 3).reshape(3, 784)[:, :128].astype(np.uint64)
    q = api.bfv_default_coeff_modulus(1 << 14, lib)
    assert len(q) == 9
    S, X, M, b, xs, outs = _both_methods(orc, api, lib, mem, 14, q, 128, (16, 8), 1, vals=pix, seed=2)
    for method, got in outs.items():
        vals = mem.empty((3, S.n))
        X.decrypt(S.sk, mem.to_dev(got), 3, vals)
        dec = mem.to_host(vals)
        for k in range(3):
            assert [int(v) for v in dec[k, :128]] == ac.plain_affine(M, xs[k], b, T), (method, k)
    X.close()


def test_fallback_path_bfv_default_4096(orc, api, lib, mem):
    """BFVDefault(4096): no pseudo-Mersenne form, the separate-kernel step at full tiles"""
    q = api.bfv_default_coeff_modulus(4096, lib)
    _, X, *_ = _both_methods(orc, api, lib, mem, 12, q, 64, (8, 8), 0, seed=3)
    X.close()


def test_full_packed_row(orc, api, lib, mem):
    """dim = N / 2 = 512: no preparation rotation; 511 chain steps, and BSGS 32 x 16"""
    q = orc.coeff_modulus_create(1024, [50] * 3)
    _, X, *_ = _both_methods(orc, api, lib, mem, 10, q, 512, (32, 16), 0, B=2, seed=4)
    X.close()


def test_dim_100_bsgs_10_by_10(orc, api, lib, mem):
    """not a power of two; n2 = 10 takes the inner-sum kernel's second group of giant steps"""
    q = orc.coeff_modulus_create(4096, [50] * 3)
    _, X, *_ = _both_methods(orc, api, lib, mem, 12, q, 100, (10, 10), 1, seed=5)
    X.close()
