"""hhe_multiply_sum at behz_sum_cap, and the contexts whose cap is 0, on the device: the cases of tests/test_headroom_emu.py on the
kernels -- the B_sk sums of tensor_sum_kernel, the floor and the centred comparison against m_sk / 2 with the floored sum at the limit
fastbconv_sk recovers.  One to three items at N = 1024 or 4096 per call; the restatement of an item is computed once per context
(headroom_common.truth).  Run on an MI355X: python -m pytest tests -m gpu."""
import pytest

import headroom_common as hc
import parity_common as pc

pytestmark = pytest.mark.gpu
NAMES = list(hc.CONTEXTS)


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


def _ctx(api, lib, E):
    return api.Context(E.logn, E.q, E.t, lib=lib)


@pytest.mark.parametrize("name", NAMES)
def test_at_the_cap(orc, api, lib, mem, name):
    """the cap against Python integers and the pinned literal; K = cap on 'half', 'half_neg' and 'half_mixed' with B = 1, on three
    items in one call and broadcast: every word the restatement's, the distance at most L + 1.  The operands sit at the bound:
    test_headroom_emu.test_one_above_the_cap_leaves_the_bound.  Largest distance on the device: 1, 2, 3, 3, 2, 2 at N = 1024 and 2 at
    N = 4096 (the uniform item of the three-item call included); on 'half' alone 1, 1, 2, 3, 2, 2 and 1, the emulator's figures."""
    E, cap = hc.context(orc, name)
    X = _ctx(api, lib, E)
    hc.check_cap(X, E, cap)
    if name == "54x3":
        assert cap == X.query("multiply_sum_fold_bsk") + 1
    worst = max([hc.check_at_the_cap(X, E, mem, cap, pattern) for pattern in hc.AT_THE_CAP] + [hc.check_three_items_and_broadcast(X, E, mem, cap)])
    print("largest distance at K = cap = %d, %s: %d (L + 1 = %d)" % (cap, name, worst, E.L + 1))
    X.close()


@pytest.mark.parametrize("name", NAMES)
def test_one_above_the_cap_is_refused(orc, api, lib, mem, name):
    E, cap = hc.context(orc, name)
    X = _ctx(api, lib, E)
    hc.check_refused_above_the_cap(X, E, mem, api, cap)
    X.close()


@pytest.mark.parametrize("name", NAMES)
def test_multiply_and_square_on_half(orc, api, lib, mem, name):
    E, _ = hc.context(orc, name)
    X = _ctx(api, lib, E)
    hc.check_multiply_and_square(X, E, mem)
    X.close()


@pytest.mark.parametrize("name", list(hc.ZERO))
def test_cap_zero(orc, api, lib, mem, name):
    """behz_sum_cap == 0 (T60 over 60-bit primes at N = 1024): hhe_multiply on 'half' is the oracle's, word for word, and both are
    more than L + 1 from the rounded integer product -- BEHZ's own limit, no defect: one product of arbitrary words is outside the
    proved bound there, and SEAL serves it all the same.  The per-product layers are served (and decrypt over 5 x 60 bits; over
    2 x 60 bits a fresh encryption has no budget); the sum forms refuse and leave `out` untouched."""
    S, E = hc.zero_setup(orc, name)
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    S.load_keys(X)
    hc.check_zero_multiply(X, E, mem)
    hc.check_zero_layers(X, S, mem, orc, seed=5)
    hc.check_zero_refusals(X, S, mem, api)
    X.close()
