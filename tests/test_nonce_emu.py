"""PASTA under a caller's nonce on the tests-only emulator (real host driver, kernel bodies on the CPU): the checks of nonce_common,
whose docstring says what the truth is.  Shapes: N = 1024 over 3 x 50 bits (ragged tiles; the knob variants run here) and N = 4096
over 3 x 60 bits (the host takes the fused key-switch row kernel's path)."""
import pytest

import fused_finish_common as ff
import nonce_common as nc
import parity_common as pc
from conftest import Setup
from test_stream_order_emu import KeptMem, lazy_order


@pytest.fixture
def mem():
    return pc.HostMem()


@pytest.fixture(scope="module")
def ragged(orc):
    """N = 1024, L = 2, with the keys of the babystep-giantstep variant and of flatten"""
    return Setup(orc, 10, [50] * 3, extra_steps=ff.BSGS_STEPS + (-128,))


@pytest.fixture(scope="module")
def row(orc):
    return Setup(orc, 12, [60] * 3, extra_steps=ff.BSGS_STEPS)


def test_oracle_and_host_generator_equal_the_reference_at_other_nonces(orc, api, emu_lib):
    nc.check_oracle_against_golden(orc, api, emu_lib)


def test_restatement_equals_the_oracle_at_the_fixed_nonce(orc, ragged):
    nc.check_restatement(orc, ragged)


@pytest.mark.parametrize("t", nc.MODULI)
def test_device_randomness(orc, api, emu_lib, mem, t):
    nc.check_device_randomness(orc, api, emu_lib, mem, t)


@pytest.mark.parametrize("t", nc.MODULI)
def test_client_end(orc, api, emu_lib, mem, t):
    nc.check_client(orc, api, emu_lib, mem, t)


@pytest.mark.parametrize("use_bsgs", [False, True], ids=["diagonal", "bsgs"])
def test_words_ragged(orc, api, emu_lib, mem, ragged, monkeypatch, use_bsgs):
    nc.check_words(orc, api, emu_lib, mem, ragged, monkeypatch, use_bsgs, row_kernel=0)


@pytest.mark.parametrize("use_bsgs", [False, True], ids=["diagonal", "bsgs"])
def test_words_row_kernel(orc, api, emu_lib, mem, row, monkeypatch, use_bsgs):
    nc.check_words(orc, api, emu_lib, mem, row, monkeypatch, use_bsgs, row_kernel=1, variants=False)


def test_words_unfused_matmul(orc, api, emu_lib, mem, ragged, monkeypatch):
    """HHE_MATMUL=0 reads `diag`, not `pdiag`: the other table the device matrices feed"""
    nc.check_words(orc, api, emu_lib, mem, ragged, monkeypatch, False, row_kernel=0, variants=False, HHE_MATMUL=0)


def test_one_cache(orc, api, emu_lib, mem, ragged, monkeypatch):
    nc.check_one_cache(orc, api, emu_lib, mem, ragged, monkeypatch)


def test_groups(orc, api, emu_lib, mem, ragged, monkeypatch):
    nc.check_groups(orc, api, emu_lib, mem, ragged, monkeypatch)


def test_decompose(orc, api, emu_lib, mem, ragged, monkeypatch):
    nc.check_decompose(orc, api, emu_lib, mem, ragged, monkeypatch)


def test_refusals(orc, api, emu_lib, mem, ragged, monkeypatch):
    nc.check_refusals(orc, api, emu_lib, mem, ragged, monkeypatch)


def test_prepare_tables(orc, api, emu_lib, mem, ragged, monkeypatch):
    nc.check_prepare_tables(orc, api, emu_lib, mem, ragged, monkeypatch)


def test_lazy_order(orc, api, emu_lib, ragged, monkeypatch):
    """the checks of the words (device randomness, both methods) and of the groups under the emulator's lazy stream order: the XOF and
    expansion launches have no host wait between them or in front of the table pipeline, so a missing edge shows here"""
    mem = KeptMem()
    with lazy_order(emu_lib, monkeypatch):
        nc.check_words(orc, api, emu_lib, mem, ragged, monkeypatch, False, row_kernel=0, variants=False)
        nc.check_words(orc, api, emu_lib, mem, ragged, monkeypatch, True, row_kernel=0, variants=False)
        nc.check_groups(orc, api, emu_lib, mem, ragged, monkeypatch, HHE_PUBLIC_DEVICE=1)
