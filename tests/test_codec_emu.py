"""The plaintext boundary against its definitions in Python integers (codec_common.py: g. slots, h. decrypt), on the oracle and on
the tests-only emulator: hhe_encode as the interpolation at psi_t^(e_i), hhe_decrypt on phases the test chose under its own sparse
key (the slot order, the c1 s path, both item strides), the scale-and-round on a walk of x across every rounding boundary, the
gamma-correction window and the two sides of `vg > (gamma >> 1)`, and all of it again at every limb count through hhe_decrypt_level
and through the level contexts.  A failure names who is wrong: the oracle and the product are held to the same truth in the same
test.  The checks run unchanged on the GPU (test_gpu_codec.py).

N = 1024 at the three plain moduli: 65537 and 8088322049 over 2 data primes of 50 bits, 1096486890805657601 over 14 of 55 bits."""
import pytest

import codec_common as cc
import definition_common as dc
import parity_common as pc

SETS = ["n1024-t16", "n1024-t33", "n1024-t60"]


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


def level_case(orc, api, lib):
    """N = 1024, four primes of 50 bits: L = 3"""
    q = orc.coeff_modulus_create(1024, [50] * 4)
    return dc.env(orc, 10, q, dc.T16), lambda: api.Context(10, q, dc.T16, lib=lib)


@pytest.mark.parametrize("name", SETS)
def test_encode_is_the_interpolation_at_the_slots(orc, api, emu_lib, mem, name):
    """g. 1, N/2, N/2 + 1 and N values per item: one-hot slots on the full vector, uniform values at 19 slots by Horner"""
    E, make_ctx = dc.plain_case(orc, api, emu_lib, name)
    cc.check_encode(make_ctx, E, mem)


@pytest.mark.parametrize("name", SETS)
def test_decrypt_returns_the_chosen_slots(orc, api, emu_lib, mem, name):
    """g. three items, each the scaled plaintext of three monomials under s = X^a - X^b + X^c with uniform c1: all N slots"""
    E, make_ctx = dc.plain_case(orc, api, emu_lib, name)
    cc.check_decrypt_slots(make_ctx, E, mem)


@pytest.mark.parametrize("name", SETS)
def test_decrypt_rounds_as_defined(orc, api, emu_lib, mem, name):
    """h. the walk and a uniform item.  Coefficients of item 0 inside the window / where h differs from exact rounding, on the oracle
    and on the emulator alike: 27 / 20 at t = 65537 and 26 / 20 at t = 8088322049 (l = 2), 33 / 26 at t = 1096486890805657601 (l = 14)."""
    E, make_ctx = dc.plain_case(orc, api, emu_lib, name)
    inside, differs = cc.check_decrypt_rounding(make_ctx, E, mem)
    assert inside >= 12 and differs >= 1


def test_decrypt_at_every_level(orc, api, emu_lib, mem):
    """g, h. checks 2 and 3 through hhe_decrypt_level and through hhe_decrypt on the level context, l = 1, 2, 3 of four 50-bit primes.
    l = 1: Q has 50 bits, below t gamma, so there is no window and nothing to search (0 / 0); l = 2 and 3 have both (27 / 20, 33 / 21)."""
    E, make_ctx = level_case(orc, api, emu_lib)
    counts = cc.check_decrypt_levels(make_ctx, E, orc, mem)
    assert counts[1][1] == 0 and all(counts[l][0] >= 12 and counts[l][1] >= 1 for l in (2, 3)), counts
