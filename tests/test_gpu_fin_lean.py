"""The item kernel's 32-bit instantiation with one lazy reduction per c0 word, the keystream pointer read once per workgroup and
32-bit offsets from uniform bases (fin_item32_kernel, fin_word32, fin_at; DESIGN.md "32-bit scaling") on the gfx950 kernels, over the
limb counts at which its store phase takes another path: L = 1, 2, 3 (limbs fetched ahead, fewer than or all of FIN_PRE) and 4 (one
limb past them).  Every context is created under HHE_FIN_ITEM=1, so the kernel runs for every batch size.  Every check is exact
equality of ciphertext words against a context created under HHE_FIN_FUSED=0 (clear, scatter, transform, add_plain with the shared
128-bit definition) and against one under HHE_FIN_SCALE32=0 (the item kernel's 64-bit instantiation), and for one item of each small
shape against the oracle; fin_scale32 and fin_item_launches tell which instantiation a context takes and that it ran."""
import numpy as np
import pytest

import dedup_common as dc
import kscache_common as kc
import parity_common as pc
from conftest import Setup

T30 = 1073479681  # prime, = 1 mod 2^16, just below 2^30: the largest plain modulus the item kernel takes


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


@pytest.fixture
def item(monkeypatch):
    monkeypatch.setenv("HHE_FIN_ITEM", "1")


def three_ways(api, lib, S, mem, monkeypatch, cw, ncw, ids, limbs, oracle_items=()):
    """the words of the 32-bit instantiation, equal to those of the unfused pass and of the 64-bit instantiation; each path asserted"""
    assert len(S.q) - 1 == limbs
    Xn = dc.make_ctx(api, lib, S, monkeypatch, HHE_FIN_FUSED=1, HHE_FIN_SCALE32=1)
    Xu = dc.make_ctx(api, lib, S, monkeypatch, HHE_FIN_FUSED=0)
    Xo = dc.make_ctx(api, lib, S, monkeypatch, HHE_FIN_FUSED=1, HHE_FIN_SCALE32=0)
    assert Xn.query("fin_item") == 1 and Xn.query("fin_scale32") == 1
    assert Xu.query("fin_item") == 0 and Xu.query("fin_scale32") == 0
    assert Xo.query("fin_item") == 1 and Xo.query("fin_scale32") == 0
    rn, ru, ro = (kc.run(X, S, mem, cw, ncw, ids) for X in (Xn, Xu, Xo))
    assert Xn.query("fin_item_launches") == 1 and Xu.query("fin_item_launches") == 0 and Xo.query("fin_item_launches") == 1
    assert rn.shape[2] == limbs
    for what, r in (("the unfused pass", ru), ("the 64-bit instantiation", ro)):
        assert (rn == r).all(), ("items that differ from " + what, np.argwhere((rn != r).reshape(len(ids), -1).any(axis=1)).ravel())
    for b in oracle_items:
        assert (rn[b] == dc.oracle_block(S, cw, ncw, ids, b)).all(), f"item {b} differs from the oracle"
    # the same call against the kept keystreams: the steady step, one launch more
    assert (kc.run(Xn, S, mem, cw, ncw, ids) == rn).all() and Xn.query("fin_item_launches") == 2
    for X in (Xn, Xu, Xo):
        X.close()


@pytest.mark.gpu
@pytest.mark.parametrize("primes,t", [(2, 65537), (3, 65537), (4, 65537), (5, 65537), (4, T30)],
                         ids=["L1", "L2", "L3", "L4", "L3-t30"])
def test_gpu_limb_counts(orc, api, lib, mem, monkeypatch, item, primes, t):
    """N = 2^10, B = 3 items of 128, 17 and 0 words over the counters 0, 0, 2; the item of 17 words against the oracle"""
    S = Setup(orc, 10, [50] * primes, t=t)
    three_ways(api, lib, S, mem, monkeypatch, kc.words(S, 3, 95), [128, 17, 0], [0, 0, 2], primes - 1, oracle_items=(1,))


@pytest.mark.gpu
def test_gpu_slices_cut_a_limb(orc, api, lib, mem, monkeypatch, item):
    """N = 2^13, L = 3: four rounds and one stage, so seven c1 slices over three limbs -- slice boundaries inside a limb"""
    S = Setup(orc, 13, [50] * 4)
    three_ways(api, lib, S, mem, monkeypatch, kc.words(S, 3, 96), [128, 17, 0], [0, 0, 2], 3)


@pytest.mark.gpu
def test_gpu_flagship_instantiation(orc, api, lib, mem, monkeypatch, item):
    """N = 2^15, 4 x 60 bits (L = 3), B = 4: the instantiation the benchmark's steady step runs, 128 KiB of LDS"""
    S = Setup(orc, 15, [60] * 4)
    three_ways(api, lib, S, mem, monkeypatch, kc.words(S, 4, 97), [128, 128, 16, 5], [0, 0, 6, 0], 3)
