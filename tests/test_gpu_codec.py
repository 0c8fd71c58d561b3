"""The plaintext boundary against its definitions in Python integers (codec_common.py: g. slots, h. decrypt) on the GPU: the checks
test_codec_emu.py runs on the emulator, and the parameter sets where the kernels take another path -- N = 4096 over 60-bit primes
(full tiles, pm_fold transforms) and over BFVDefault(4096) (Harvey butterflies; Q has 72 bits, so the window is empty and every
coefficient rounds exactly), every limb count of the 60-bit chain, and once the benchmark's parameters.  Two or three items per call:
the device time is milliseconds, what a test costs is the integer work on the host.  Run on an MI355X: python -m pytest tests -m gpu."""
import pytest

import codec_common as cc
import definition_common as dc
import parity_common as pc

pytestmark = pytest.mark.gpu

SETS = ["n1024-t16", "n1024-t33", "n1024-t60", "row12-t16", "row12-t33", "A-t16", "A-t33"]


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


@pytest.mark.parametrize("name", SETS)
def test_encode_is_the_interpolation_at_the_slots(orc, api, lib, mem, name):
    """g. 1, N/2, N/2 + 1 and N values per item: one-hot slots on the full vector, uniform values at 19 slots by Horner"""
    E, make_ctx = dc.plain_case(orc, api, lib, name)
    cc.check_encode(make_ctx, E, mem)


@pytest.mark.parametrize("name", SETS)
def test_decrypt_returns_the_chosen_slots(orc, api, lib, mem, name):
    """g. three items, each the scaled plaintext of three monomials under s = X^a - X^b + X^c with uniform c1: all N slots"""
    E, make_ctx = dc.plain_case(orc, api, lib, name)
    cc.check_decrypt_slots(make_ctx, E, mem)


@pytest.mark.parametrize("name", SETS)
def test_decrypt_rounds_as_defined(orc, api, lib, mem, name):
    """h. the walk and a uniform item.  Coefficients of item 0 inside the window / where h differs from exact rounding, oracle and
    kernels alike: 27 / 20, 26 / 20 and 33 / 26 at N = 1024 (as on the emulator), 27 / 20 and 27 / 21 at N = 4096 over 2 x 60 bits; on
    BFVDefault(4096) Q has 72 bits, below t gamma, the window is empty and every coefficient rounds exactly (0 / 0)."""
    E, make_ctx = dc.plain_case(orc, api, lib, name)
    inside, differs = cc.check_decrypt_rounding(make_ctx, E, mem)
    assert (inside, differs) == (0, 0) if name[0] == "A" else (inside >= 12 and differs >= 1)


def test_decrypt_at_every_level(orc, api, lib, mem):
    """g, h. checks 2 and 3 through hhe_decrypt_level and through hhe_decrypt on the level context, l = 1, 2 of N = 4096, 3 x 60 bits"""
    E, make_ctx = dc.setup(orc, api, lib, "row12")
    counts = cc.check_decrypt_levels(make_ctx, E, orc, mem)
    assert counts[1][1] == 0 and counts[2][0] >= 12 and counts[2][1] >= 1, counts


def test_decrypt_at_the_benchmark_parameters(orc, api, lib, mem):
    """g, h. N = 32768, 4 x 60 bits: one item each, 8 slots, 64 points of the walk at seeded coefficients among uniform x (30 of
    them in the window, 20 off exact rounding)"""
    E, make_ctx = dc.setup(orc, api, lib, "bench15")
    cc.check_decrypt_slots(make_ctx, E, mem, B=1)
    inside, differs = cc.check_decrypt_rounding(make_ctx, E, mem, B=1, samples=3, limit=64)
    assert inside >= 12 and differs >= 1
