"""The finishing pass of a transciphering call with one workgroup per item (fin_item_kernel, DESIGN.md "Finishing pass in one
workgroup") on the gfx950 kernels.  Every check is exact equality of ciphertext words between a context created under HHE_FIN_ITEM=1
(the kernel runs for every batch size), one created under HHE_FIN_FUSED=0 (clear, scatter, transform, add_plain: the separate
launches) and, for named items, the oracle's transcipher_block; fin_item_launches tells which path a call took.  The cases are those
of fused_finish_common, run through its helpers with the knob set, at every number of register rounds the kernel has: N = 2^10
(3 + a round of one stage), 2^12 (4), 2^13 (4 + one stage), 2^14 (4 + two stages), 2^15 (5: the benchmark's parameters)."""
import pytest

import dedup_common as dc
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
    return Setup(orc, 10, [50] * 3)


@pytest.fixture(scope="module")
def full(orc):
    return Setup(orc, 12, [50] * 3)


@pytest.fixture
def item(monkeypatch):
    """every context of the test is created under HHE_FIN_ITEM=1, and every comparison of ff.same checks which path its contexts took"""
    monkeypatch.setenv("HHE_FIN_ITEM", "1")
    plain_same = ff.same

    def same(S, mem, X1, X0, *args, **kw):
        assert X1.query("fin_item") == 1 and X0.query("fin_item") == 0
        before = X1.query("fin_item_launches")
        r = plain_same(S, mem, X1, X0, *args, **kw)
        assert X1.query("fin_item_launches") > before and X0.query("fin_item_launches") == 0
        return r

    monkeypatch.setattr(ff, "same", same)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["ragged", "full"])
def test_gpu_lengths_and_word_range(orc, api, lib, mem, monkeypatch, request, item, shape):
    S = request.getfixturevalue(shape)
    ff.check_lengths(api, lib, S, mem, monkeypatch)
    ff.check_word_range(api, lib, S, mem, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["ragged", "full"])
def test_gpu_seven_items_cold_partly_kept_all_kept(orc, api, lib, mem, monkeypatch, request, item, shape):
    ff.check_chunks_and_hits(api, lib, request.getfixturevalue(shape), mem, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["ragged", "full"])
def test_gpu_grow_and_shrink(orc, api, lib, mem, monkeypatch, request, item, shape):
    ff.check_grow_and_shrink(api, lib, request.getfixturevalue(shape), mem, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["ragged", "full"])
def test_gpu_prediction(orc, api, lib, mem, monkeypatch, request, item, shape):
    """key A twice, key B over the same counters, A again: the second call is enqueued on the prediction and confirmed (one launch), the
    third is enqueued on the prediction of A, refuted and finished again (two launches), the fourth predicts B -- the key used last --
    and is refuted too; every result is the oracle's for its key and the counts are what they are without the item kernel"""
    ff.check_prediction(api, lib, request.getfixturevalue(shape), mem, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [13, 14])
def test_gpu_larger_degrees(orc, api, lib, mem, monkeypatch, item, logn):
    ff.check_one_call(api, lib, Setup(orc, logn, [50] * 3), mem, monkeypatch, oracle_items=())


@pytest.mark.gpu
def test_gpu_bench_parameters(orc, api, lib, mem, monkeypatch, item):
    """N = 2^15, 4 x 60 bits, B = 4: 128 KiB of LDS per workgroup; the second call runs on the prediction"""
    S, ids = Setup(orc, 15, [60] * 4), [0, 0, 6, 0]
    X1, X0 = ff.pair(api, lib, S, monkeypatch)
    ff.same(S, mem, X1, X0, kc.words(S, 4, 38), [128, 128, 16, 5], ids)
    assert kc.counts(X1) == (2, 0)
    ff.same(S, mem, X1, X0, kc.words(S, 4, 39), [128, 3, 16, 128], ids)
    assert kc.counts(X1) == (0, 2) and kc.counts(X0) == (0, 2) and X1.query("fin_item_launches") == 2
    X1.close(), X0.close()


@pytest.mark.gpu
def test_gpu_default_threshold(orc, api, lib, mem, full, monkeypatch):
    """without the knob a small call takes the two-pass kernels: fin_item reads 1, nothing is launched"""
    X = dc.make_ctx(api, lib, full, monkeypatch)
    assert X.query("fin_item") == 1 and X.query("fin_item_min") > 3
    kc.run(X, full, mem, kc.words(full, 3, 82), [128, 1, 0], [0, 0, 1])
    assert X.query("fin_item_launches") == 0
    X.close()


@pytest.mark.gpu
def test_gpu_ineligible_contexts(orc, api, lib, mem, full, monkeypatch):
    """a plain modulus of 33 bits, and the knob at 0: fin_item reads 0, the kernel is never launched, the words are the separate launches'"""
    monkeypatch.setenv("HHE_FIN_ITEM", "1")
    S33, _ = pm.hot_setup(orc, api, lib, "t33_60x3")
    for S, env in ((S33, {}), (full, dict(HHE_FIN_ITEM=0))):
        X1, X0 = ff.pair(api, lib, S, monkeypatch, **env)
        assert X1.query("fin_item") == 0 and X1.query("fin_fused") == 1
        cw, ncw, ids = kc.words(S, 3, 83), [128, 17, 128], [0, 0, 2]
        r = ff.same(S, mem, X1, X0, cw, ncw, ids)
        assert (kc.run(X1, S, mem, cw, ncw, ids) == r).all() and kc.counts(X1) == (0, 2)
        assert X1.query("fin_item_launches") == 0
        X1.close(), X0.close()
