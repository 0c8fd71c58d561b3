"""PASTA under a caller's nonce on the gfx950 kernels: the checks of nonce_common (whose docstring says what the truth is) on the
device, and one flow end to end without an oracle key at BFVDefault(16384).  Shapes: N = 1024 over 3 x 50 bits (ragged tiles) and
N = 4096 over 3 x 60 bits (the fused key-switch row kernel)."""
import numpy as np
import pytest

import fused_finish_common as ff
import keygen_common as kg
import nonce_common as nc
import parity_common as pc
from conftest import Setup


@pytest.fixture(scope="module")
def mem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pc.TorchMem("cuda:0")


@pytest.fixture(scope="module")
def lib(api):
    lib = api.load_library()
    assert lib.hhe_backend() == b"hip-gfx950"
    return lib


@pytest.fixture(scope="module")
def ragged(orc):
    return Setup(orc, 10, [50] * 3, extra_steps=ff.BSGS_STEPS + (-128,))


@pytest.fixture(scope="module")
def row(orc):
    return Setup(orc, 12, [60] * 3, extra_steps=ff.BSGS_STEPS)


@pytest.mark.gpu
@pytest.mark.parametrize("t", nc.MODULI)
def test_gpu_device_randomness(orc, api, lib, mem, t):
    nc.check_device_randomness(orc, api, lib, mem, t)


@pytest.mark.gpu
@pytest.mark.parametrize("t", nc.MODULI)
def test_gpu_client_end(orc, api, lib, mem, t):
    nc.check_client(orc, api, lib, mem, t)


@pytest.mark.gpu
@pytest.mark.parametrize("use_bsgs", [False, True], ids=["diagonal", "bsgs"])
def test_gpu_words_ragged(orc, api, lib, mem, ragged, monkeypatch, use_bsgs):
    nc.check_words(orc, api, lib, mem, ragged, monkeypatch, use_bsgs, row_kernel=0)


@pytest.mark.gpu
@pytest.mark.parametrize("use_bsgs", [False, True], ids=["diagonal", "bsgs"])
def test_gpu_words_row_kernel(orc, api, lib, mem, row, monkeypatch, use_bsgs):
    nc.check_words(orc, api, lib, mem, row, monkeypatch, use_bsgs, row_kernel=1)


@pytest.mark.gpu
def test_gpu_words_unfused_matmul(orc, api, lib, mem, ragged, monkeypatch):
    nc.check_words(orc, api, lib, mem, ragged, monkeypatch, False, row_kernel=0, variants=False, HHE_MATMUL=0)


@pytest.mark.gpu
def test_gpu_one_cache(orc, api, lib, mem, ragged, monkeypatch):
    nc.check_one_cache(orc, api, lib, mem, ragged, monkeypatch)


@pytest.mark.gpu
def test_gpu_groups(orc, api, lib, mem, ragged, monkeypatch):
    nc.check_groups(orc, api, lib, mem, ragged, monkeypatch)
    nc.check_groups(orc, api, lib, mem, ragged, monkeypatch, HHE_PUBLIC_DEVICE=1)


@pytest.mark.gpu
def test_gpu_decompose(orc, api, lib, mem, ragged, monkeypatch):
    nc.check_decompose(orc, api, lib, mem, ragged, monkeypatch)


@pytest.mark.gpu
def test_gpu_refusals(orc, api, lib, mem, ragged, monkeypatch):
    nc.check_refusals(orc, api, lib, mem, ragged, monkeypatch)


@pytest.mark.gpu
def test_gpu_prepare_tables(orc, api, lib, mem, ragged, monkeypatch):
    nc.check_prepare_tables(orc, api, lib, mem, ragged, monkeypatch)


@pytest.mark.gpu
def test_gpu_end_to_end_without_an_oracle_key(orc, api, lib, mem, monkeypatch):
    """BFVDefault(16384): keys from a seed on the device (steps -1, +128 and the columns element), a 200-word record encrypted on the
    device under a nonce, transciphered under that nonce with the public randomness drawn on the device: positive noise budget,
    decrypts to the record; under another nonce it decrypts to something else"""
    logn, t = 14, 65537
    q = api.bfv_default_coeff_modulus(1 << logn, lib)
    monkeypatch.setenv("HHE_PUBLIC_DEVICE", "1")
    X = api.Context(logn, q, t, lib=lib)
    monkeypatch.delenv("HHE_PUBLIC_DEVICE")
    O = orc.Oracle(logn, q, t)
    D = kg.DeviceKeys(X, O, mem, kg.SEED)
    ks = D.keyset([O.galois_elt(s) for s in (-1, 128, 0)], kg.SEED2)
    key = nc.demo_key(t)
    d_enc_key = mem.empty((1,) + O.ct_shape)
    X.encrypt(D.d_pk, mem.to_dev(O.pasta_pack_key(key)[None]), kg.SEED2, 1, d_enc_key)
    record = np.random.default_rng(9).integers(0, t, size=(1, 200), dtype=np.uint64)
    d_sym = mem.empty((1, 200))
    X.plain_crypt(key, mem.to_dev(record), 1, 200, d_sym, nonces=[nc.NA])
    sym = mem.to_host(d_sym)[0]
    cw = np.zeros((2, 128), np.uint64)
    cw[0], cw[1, :72] = sym[:128], sym[128:]
    out, vals = mem.empty((2,) + O.ct_shape), mem.empty((2, O.n))
    X.transcipher(d_enc_key, cw, [128, 72], [0, 1], out, rk=ks, gk=ks, nonces=[nc.NA, nc.NA])
    assert X.query("public_device_built") == 2 and X.query("transcipher_unique") == 2
    assert (X.noise_budget(D.sk, out, 2) > 0).all()
    X.decrypt(D.sk, out, 2, vals)
    got = mem.to_host(vals)
    assert (got[0, :128] == record[0, :128]).all() and (got[1, :72] == record[0, 128:]).all()
    X.transcipher(d_enc_key, cw, [128, 72], [0, 1], out, rk=ks, gk=ks, nonces=[nc.NB, nc.NB])
    assert (X.noise_budget(D.sk, out, 2) > 0).all()
    X.decrypt(D.sk, out, 2, vals)
    other = mem.to_host(vals)
    assert not (other[0, :128] == record[0, :128]).all() and not (other[1, :72] == record[0, 128:]).all()
    ks.close(), X.close()
