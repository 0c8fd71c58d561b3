"""The invariant noise budget (hhe_noise_budget) on the emulator, built with its range check: the shared kernel bodies behind the real
host driver; see noise_common for the definition every count is compared with.  The GPU suite makes the same calls in
tests/test_gpu_noise.py."""
import pytest

import noise_common as nc
import parity_common as pc
from test_mod_switch_emu import KEYLESS_LEVEL_20_50_50, KEYLESS_LEVEL_N4096, keyless_small_q0


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


def crafted(orc, api, lib, name):
    logn, q, t = nc.crafted_primes(orc, api, lib, name)
    return api.Context(logn, q, t, lib=lib), q, t


@pytest.mark.parametrize("name", list(nc.CRAFTED))
def test_crafted_magnitudes(orc, api, emu_lib, mem, name):
    X, q, t = crafted(orc, api, emu_lib, name)
    nc.check_crafted(X, q, t, mem)


@pytest.mark.parametrize("name", ["n1024_3x50", "n1024_10x50"])
def test_reduction(orc, api, emu_lib, mem, name):
    X, q, t = crafted(orc, api, emu_lib, name)
    nc.check_reduction(X, q, t, mem)


@pytest.mark.parametrize("case", list(nc.REAL))
def test_real_ciphertexts(orc, api, emu_lib, mem, case):
    logn, bits = nc.REAL[case]
    q = orc.coeff_modulus_create(1 << logn, bits)
    nc.check_real(api.Context(logn, q, nc.T16, lib=emu_lib), orc.Oracle(logn, q, nc.T16), orc, mem)


def test_keyless_flow(orc, api, emu_lib, mem):
    q = orc.coeff_modulus_create(4096, [50] * 4)
    nc.check_keyless_flow(api.Context(12, q, nc.T16, lib=emu_lib), orc.Oracle(12, q, nc.T16), mem, KEYLESS_LEVEL_N4096)


def test_keyless_flow_stops_above_the_last_level(orc, api, emu_lib, mem):
    X, O = keyless_small_q0(orc, api, emu_lib)
    nc.check_keyless_flow(X, O, mem, KEYLESS_LEVEL_20_50_50)


def test_refusals(orc, api, emu_lib, mem):
    X, q, t = crafted(orc, api, emu_lib, "n1024_3x50")
    nc.check_refusals(X, mem, api)
