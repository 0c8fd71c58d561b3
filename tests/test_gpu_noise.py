"""The invariant noise budget (hhe_noise_budget) on the gfx950 kernels: the calls of tests/test_noise_emu.py through noise_common, and
the deployed parameters (BFVDefault(16384), L = 8) against the full-vector definition."""
import numpy as np
import pytest

import mod_switch_common as ms
import noise_common as nc
import parity_common as pc
from test_mod_switch_emu import KEYLESS_LEVEL_20_50_50, KEYLESS_LEVEL_N4096, keyless_small_q0
from test_noise_emu import crafted


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


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(nc.CRAFTED))
def test_gpu_crafted_magnitudes(orc, api, lib, mem, name):
    X, q, t = crafted(orc, api, lib, name)
    nc.check_crafted(X, q, t, mem)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n1024_3x50", "n1024_10x50"])
def test_gpu_reduction(orc, api, lib, mem, name):
    X, q, t = crafted(orc, api, lib, name)
    nc.check_reduction(X, q, t, mem)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(nc.REAL))
def test_gpu_real_ciphertexts(orc, api, lib, mem, case):
    logn, bits = nc.REAL[case]
    q = orc.coeff_modulus_create(1 << logn, bits)
    nc.check_real(api.Context(logn, q, nc.T16, lib=lib), orc.Oracle(logn, q, nc.T16), orc, mem)


@pytest.mark.gpu
def test_gpu_keyless_flow(orc, api, lib, mem):
    q = orc.coeff_modulus_create(4096, [50] * 4)
    nc.check_keyless_flow(api.Context(12, q, nc.T16, lib=lib), orc.Oracle(12, q, nc.T16), mem, KEYLESS_LEVEL_N4096)


@pytest.mark.gpu
def test_gpu_keyless_flow_stops_above_the_last_level(orc, api, lib, mem):
    X, O = keyless_small_q0(orc, api, lib)
    nc.check_keyless_flow(X, O, mem, KEYLESS_LEVEL_20_50_50)


@pytest.mark.gpu
def test_gpu_refusals(orc, api, lib, mem):
    X, q, t = crafted(orc, api, lib, "n1024_3x50")
    nc.check_refusals(X, mem, api)


@pytest.mark.gpu
def test_gpu_deployed(orc, api, lib, mem):
    """BFVDefault(16384), L = 8: two fresh encryptions, and their switch to 4 limbs and to 1, every coefficient by the definition"""
    logn, q = ms.shape_primes(orc, api, lib, "n16384_default")
    X, O = api.Context(logn, q, nc.T16, lib=lib), orc.Oracle(logn, q, nc.T16)
    sk, rng = O.keygen_secret(1), np.random.default_rng(94)
    pk = O.keygen_public(sk, 2)
    cts = np.stack([O.encrypt(pk, O.encode(rng.integers(0, O.t, O.n, dtype=np.uint64)), 31 + i) for i in range(2)])
    d_ct = mem.to_dev(cts)
    for l in (O.L, 4, 1):
        low = mem.to_host(ms.switch(X, mem, d_ct, 2, 2, O.L, l))
        O2, sk2 = ms.short_oracle(orc, O, sk, l)
        want = nc.define(np.stack([O2.phase(sk2, low[i]) for i in range(2)]), O2.q, O.t)
        nc.same(nc.call(X, mem, sk, low, 2, l), want, ("deployed", l))
        assert X.query("noise_form") == l
