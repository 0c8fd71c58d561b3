"""The fused finishing pass on the gfx950 kernels (see fused_finish_common and test_fused_finish): every pass length its two kernels
are instantiated for and launched at -- ragged 2^5 / 2^5 (N = 1024), full tiles 2^6 / 2^6 (N = 4096), 2^7 row / 2^6 strided (N = 8192)
and the benchmark's 2^8 / 2^7 (N = 32768).  N = 65536 (a strided pass of 2^8) takes the separate launches: fin_fused reads 0 there."""
import pytest

import fused_finish_common as ff
import kscache_common as kc
import parity_common as pc
import plain_modulus_common as pm
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
    return Setup(orc, 10, [50] * 3, extra_steps=ff.BSGS_STEPS)


@pytest.fixture(scope="module")
def full(orc):
    return Setup(orc, 12, [50] * 3)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["ragged", "full"])
def test_gpu_lengths_and_word_range(orc, api, lib, mem, monkeypatch, request, shape):
    S = request.getfixturevalue(shape)
    ff.check_lengths(api, lib, S, mem, monkeypatch)
    ff.check_word_range(api, lib, S, mem, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["ragged", "full"])
def test_gpu_chunks_and_hits(orc, api, lib, mem, monkeypatch, request, shape):
    ff.check_chunks_and_hits(api, lib, request.getfixturevalue(shape), mem, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["ragged", "full"])
def test_gpu_grow_and_shrink(orc, api, lib, mem, monkeypatch, request, shape):
    ff.check_grow_and_shrink(api, lib, request.getfixturevalue(shape), mem, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["ragged", "full"])
def test_gpu_chunk_tail(orc, api, lib, mem, monkeypatch, request, shape):
    ff.check_chunk_tail(api, lib, request.getfixturevalue(shape), mem, monkeypatch, oracle=shape == "ragged")


@pytest.mark.gpu
def test_gpu_bsgs(orc, api, lib, mem, ragged, monkeypatch):
    ff.check_bsgs(api, lib, ragged, mem, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["t33_60x3", "t60_55x3"])
def test_gpu_plain_moduli(orc, api, lib, mem, monkeypatch, name):
    S, _ = pm.hot_setup(orc, api, lib, name)
    ff.check_one_call(api, lib, S, mem, monkeypatch)


@pytest.mark.gpu
def test_gpu_n8192(orc, api, lib, mem, monkeypatch):
    """row pass of 2^7, strided pass of 2^6"""
    ff.check_one_call(api, lib, Setup(orc, 13, [50] * 3), mem, monkeypatch)


@pytest.mark.gpu
def test_gpu_bench_parameters(orc, api, lib, mem, monkeypatch):
    """N = 2^15, 4 x 60 bits, B = 4: passes of 2^8 / 2^7; two calls with different words, the second against the kept keystreams"""
    S, ids = Setup(orc, 15, [60] * 4), [0, 0, 6, 0]
    X1, X0 = ff.pair(api, lib, S, monkeypatch)
    ff.same(S, mem, X1, X0, kc.words(S, 4, 38), [128, 128, 16, 5], ids)
    assert kc.counts(X1) == (2, 0)
    ff.same(S, mem, X1, X0, kc.words(S, 4, 39), [128, 3, 16, 128], ids)
    assert kc.counts(X1) == (0, 2) and kc.counts(X0) == (0, 2)
    X1.close(), X0.close()


@pytest.mark.gpu
def test_gpu_n65536_takes_the_separate_launches(orc, api, lib):
    """no test runs the fused kernels at a strided pass of 2^8, so no context takes them there"""
    q = orc.coeff_modulus_create(65536, [40] * 3)
    X = api.Context(16, q, pc.T33, lib=lib)
    assert X.query("fin_fused") == 0
    X.close()
