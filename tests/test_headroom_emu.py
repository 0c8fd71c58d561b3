"""hhe_multiply_sum at behz_sum_cap, and the contexts whose cap is 0, on the tests-only emulator (built with -DHHE_RANGE_CHECK, so a
128-bit sum of a tensor kernel that wraps aborts the run).  The contexts, the operands and the truths are in headroom_common; the test
that needs neither device nor emulator, and shows that the operands sit at the bound, is here."""
import pytest

import headroom_common as hc
import parity_common as pc

NAMES = list(hc.CONTEXTS)


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


def _ctx(api, lib, E):
    return api.Context(E.logn, E.q, E.t, lib=lib)


# ---- the operands sit at the bound: no device, no emulator ----
@pytest.mark.parametrize("name", NAMES)
def test_one_above_the_cap_leaves_the_bound(orc, name):
    """The restatement (Python integers; of the oracle its transforms alone) at K = cap + 1 on 'half' is MORE than L + 1 from the rounded
    integer sum, in every context: about 2^47, 2^109, 2^164, 2^226, 2^103, 2^105 at N = 1024 and 2^105 at N = 4096, where K = cap gives
    1, 1, 2, 3, 2, 2 and 1.  This is what shows that 'half' puts the floored sum at the limit of fastbconv_sk and that the cap is not one
    too small.  If it ever stops holding, the tests at K = cap prove nothing about the cap."""
    E, cap = hc.context(orc, name)
    dist = hc.check_tightness(E, cap)
    print("restatement at K = cap + 1 = %d, %s: 2^%d from the rounded integer sum" % (cap + 1, name, dist.bit_length() - 1))
    assert dist > E.L + 1


# ---- the cap ----
@pytest.mark.parametrize("name", NAMES)
def test_cap_is_the_pinned_one(orc, api, emu_lib, name):
    E, cap = hc.context(orc, name)
    X = _ctx(api, emu_lib, E)
    hc.check_cap(X, E, cap)
    if name == "54x3":
        assert cap == X.query("multiply_sum_fold_bsk") + 1
    X.close()


# ---- K = cap ----
@pytest.mark.parametrize("pattern", hc.AT_THE_CAP)
@pytest.mark.parametrize("name", NAMES)
def test_words_and_distance_at_the_cap(orc, api, emu_lib, mem, name, pattern):
    """largest distance seen, over the three patterns and both lifts: 1, 2, 2, 3, 2, 2 at N = 1024 and 2 at N = 4096 ('half' alone:
    1, 1, 2, 3, 2, 2 and 1)"""
    E, cap = hc.context(orc, name)
    X = _ctx(api, emu_lib, E)
    hc.check_at_the_cap(X, E, mem, cap, pattern)
    X.close()


@pytest.mark.parametrize("name", NAMES)
def test_three_items_and_broadcast_at_the_cap(orc, api, emu_lib, mem, name):
    E, cap = hc.context(orc, name)
    X = _ctx(api, emu_lib, E)
    hc.check_three_items_and_broadcast(X, E, mem, cap)
    X.close()


# ---- K = cap + 1 ----
@pytest.mark.parametrize("name", NAMES)
def test_one_above_the_cap_is_refused(orc, api, emu_lib, mem, name):
    E, cap = hc.context(orc, name)
    X = _ctx(api, emu_lib, E)
    hc.check_refused_above_the_cap(X, E, mem, api, cap)
    X.close()


# ---- one product ----
@pytest.mark.parametrize("name", NAMES)
def test_multiply_and_square_on_half(orc, api, emu_lib, mem, name):
    """distance 1, 2, 3, 3, 2, 2 at N = 1024 and 2 at N = 4096"""
    E, _ = hc.context(orc, name)
    X = _ctx(api, emu_lib, E)
    hc.check_multiply_and_square(X, E, mem)
    X.close()


# ---- cap == 0 ----
def _zctx(api, lib, S):
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    S.load_keys(X)
    return X


@pytest.mark.parametrize("name", list(hc.ZERO))
def test_cap_zero_multiply_is_the_oracles_and_outside_the_bound(orc, api, emu_lib, mem, name):
    """behz_sum_cap == 0: even one product of arbitrary words is outside the proved bound.  hhe_multiply still serves, as SEAL does, and
    on 'half' it is about 2^39 (one data prime) and 2^225 (four) from the rounded integer product -- word for word what the oracle
    gives.  That is the limit of BEHZ at these parameters and no defect of the product; the pin is that the product does not differ
    from the oracle there, and that the cap says 0 where one worst-case product already fails."""
    S, E = hc.zero_setup(orc, name)
    X = _zctx(api, emu_lib, S)
    hc.check_zero_multiply(X, E, mem)
    X.close()


@pytest.mark.parametrize("name", list(hc.ZERO))
def test_cap_zero_per_product_layers_decrypt(orc, api, emu_lib, mem, name):
    """hhe_fc_packed_ks and hhe_fc_packed_hoisted_ks are served at cap == 0: over 5 x 60 bits they decrypt to (M x) mod t with the
    oracle's budget positive; over 2 x 60 bits a fresh encryption already has budget 0, so there they are held to the oracle's words"""
    S, _ = hc.zero_setup(orc, name)
    X = _zctx(api, emu_lib, S)
    hc.check_zero_layers(X, S, mem, orc, seed=5)
    X.close()


@pytest.mark.parametrize("name", list(hc.ZERO))
def test_cap_zero_sum_forms_refuse(orc, api, emu_lib, mem, name):
    S, _ = hc.zero_setup(orc, name)
    X = _zctx(api, emu_lib, S)
    hc.check_zero_refusals(X, S, mem, api)
    X.close()
