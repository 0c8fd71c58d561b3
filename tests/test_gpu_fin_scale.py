"""The item kernel's 32-bit plaintext scaling with -c1 written early (fin_item32_kernel, HHE_FIN_SCALE32; DESIGN.md "32-bit scaling") on
the gfx950 kernels.  Every context is created under HHE_FIN_ITEM=1, so the kernel runs for every batch size.  Every check is exact
equality of ciphertext words against a context created under HHE_FIN_FUSED=0 (clear, scatter, transform, add_plain with the shared
128-bit plain_fix / plain_scaled), against a context under HHE_FIN_SCALE32=0 (the item kernel's earlier instantiation), against
Python integers for the scaled coefficient itself, and for named items against the oracle; fin_scale32 and fin_item_launches tell
which instantiation a context takes and that it ran."""
import numpy as np
import pytest

import dedup_common as dc
import fused_finish_common as ff
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


@pytest.fixture(scope="module")
def small_t(orc):
    return Setup(orc, 10, [50] * 3)


@pytest.fixture(scope="module")
def large_t(orc):
    return Setup(orc, 10, [50] * 3, t=T30)


@pytest.fixture
def item(monkeypatch):
    monkeypatch.setenv("HHE_FIN_ITEM", "1")


PLAIN_SAME = ff.same  # ff.same itself: a test below puts same_counted in its place for the helpers of fused_finish_common


def same_counted(S, mem, X1, X0, cw, ncw, ids, scale32=1, **kw):
    """ff.same with the paths asserted: X1 runs the item kernel (the 32-bit instantiation iff scale32), X0 never does"""
    assert X1.query("fin_item") == 1 and X1.query("fin_scale32") == scale32 and X0.query("fin_item") == 0 and X0.query("fin_scale32") == 0
    before = X1.query("fin_item_launches")
    r = PLAIN_SAME(S, mem, X1, X0, cw, ncw, ids, **kw)
    assert X1.query("fin_item_launches") > before and X0.query("fin_item_launches") == 0
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["small_t", "large_t"])
def test_gpu_boundary_coefficients(orc, api, lib, mem, monkeypatch, request, item, shape):
    """one word per item, chosen so that coefficient 0 of the item's plaintext is m*: 1, t - 1, the two coefficients at the rounding
    boundary of the fix (m* (Q mod t) mod t = (t - 1) / 2 rounds up, (t - 3) / 2 does not), (t +- 1) / 2; the last item has no word"""
    S = request.getfixturevalue(shape)
    t, n, q = S.t, S.n, [int(x) for x in S.q[:-1]]
    Q = int(np.prod(np.array(q, dtype=object)))
    qi = pow(Q % t, -1, t)
    ms = [1, t - 1, (t - 1) // 2 * qi % t, (t - 3) // 2 * qi % t, (t - 1) // 2, (t + 1) // 2]
    assert ms[2] * (Q % t) % t == (t - 1) // 2 and ms[3] * (Q % t) % t == (t - 3) // 2
    B = len(ms) + 1
    cw = kc.words(S, B, 91)  # the words past the first are stale
    cw[:len(ms), 0] = [m * n % t for m in ms]
    ncw, ids = [1] * len(ms) + [0], [0] * B
    X1, X0 = ff.pair(api, lib, S, monkeypatch)
    r = same_counted(S, mem, X1, X0, cw, ncw, ids, oracle_items=(0, 2))
    assert r.shape[2] == len(q)
    for b, m in enumerate(ms):
        for j, qj in enumerate(q):
            got = (int(r[b, 0, j, 0]) - int(r[B - 1, 0, j, 0])) % qj
            assert got == (m * Q + (t + 1) // 2) // t % qj, (b, j)
    X1.close(), X0.close()


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [10, 12])
def test_gpu_random_words_large_t(orc, api, lib, mem, monkeypatch, request, item, logn):
    S = request.getfixturevalue("large_t") if logn == 10 else Setup(orc, logn, [50] * 3, t=T30)
    monkeypatch.setattr(ff, "same", same_counted)  # undone by the fixture; same_counted calls PLAIN_SAME, not ff.same
    ff.check_one_call(api, lib, S, mem, monkeypatch)


@pytest.mark.gpu
def test_gpu_fallbacks(orc, api, lib, mem, monkeypatch, item, small_t):
    """a data prime below t, and the knob at 0: fin_scale32 reads 0, the item kernel still runs, the words are the unfused context's"""
    S28 = Setup(orc, 10, [28, 50, 50], t=T30)
    assert min(int(x) for x in S28.q[:-1]) < T30
    for S, env in ((S28, {}), (small_t, dict(HHE_FIN_SCALE32=0))):
        X1, X0 = ff.pair(api, lib, S, monkeypatch, **env)
        cw, ncw, ids = kc.words(S, 3, 92), [128, 17, 0], [0, 0, 2]
        r = same_counted(S, mem, X1, X0, cw, ncw, ids, scale32=0, oracle_items=(1,))
        assert (kc.run(X1, S, mem, cw, ncw, ids) == r).all() and kc.counts(X1) == (0, 2)
        X1.close(), X0.close()


def new_and_old(api, lib, S, mem, monkeypatch, cw, ncw, ids):
    Xn = dc.make_ctx(api, lib, S, monkeypatch, HHE_FIN_SCALE32=1)
    Xo = dc.make_ctx(api, lib, S, monkeypatch, HHE_FIN_SCALE32=0)
    assert Xn.query("fin_scale32") == 1 and Xo.query("fin_scale32") == 0 and Xn.query("fin_item") == 1 and Xo.query("fin_item") == 1
    rn, ro = kc.run(Xn, S, mem, cw, ncw, ids), kc.run(Xo, S, mem, cw, ncw, ids)
    assert Xn.query("fin_item_launches") == 1 and Xo.query("fin_item_launches") == 1
    assert (rn == ro).all(), ("items that differ:", np.argwhere((rn != ro).reshape(len(ids), -1).any(axis=1)).ravel())
    Xn.close(), Xo.close()


@pytest.mark.gpu
@pytest.mark.parametrize("logn", [13, 14])
def test_gpu_round_counts_new_against_old(orc, api, lib, mem, monkeypatch, item, logn):
    """4 rounds + one stage and 4 + two stages (N = 2^10 and 2^12 above: 3 + one stage, 4): the slices of -c1 follow the round count"""
    S = Setup(orc, logn, [50] * 3)
    new_and_old(api, lib, S, mem, monkeypatch, kc.words(S, 3, 93), [128, 17, 128], [0, 0, 2])


@pytest.mark.gpu
def test_gpu_bench_parameters_new_against_old(orc, api, lib, mem, monkeypatch, item):
    """N = 2^15, 4 x 60 bits (one limb past the prefetched three), B = 4: five rounds, 128 KiB of LDS"""
    S = Setup(orc, 15, [60] * 4)
    new_and_old(api, lib, S, mem, monkeypatch, kc.words(S, 4, 94), [128, 128, 16, 5], [0, 0, 6, 0])
