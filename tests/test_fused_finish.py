"""The fused finishing pass on the emulator (the shared kernel bodies behind the real host driver): the two new ops of the transform
bodies -- the tile gathered from the words (LOAD_ENCODE) and the add_plain epilogue (STORE_ADD_PLAIN) -- and the host's order of a
call, at the two smallest shapes that reach the ragged and the full-tile instantiations.  See fused_finish_common for what every check
compares."""
import pytest

import fused_finish_common as ff
import parity_common as pc
import plain_modulus_common as pm
from conftest import Setup


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


@pytest.fixture(scope="module")
def ragged(orc):
    """N = 1024: ragged tiles, passes of 2^5 / 2^5 (t = 65537 over 50-bit primes: EDGE_CASES t16_50x3)"""
    return Setup(orc, 10, [50] * 3, extra_steps=ff.BSGS_STEPS)


@pytest.fixture(scope="module")
def full(orc):
    """N = 4096: full tiles, passes of 2^6 / 2^6, the fused key-switch row kernel"""
    return Setup(orc, 12, [50] * 3)


def test_lengths(orc, api, emu_lib, mem, ragged, monkeypatch):
    ff.check_lengths(api, emu_lib, ragged, mem, monkeypatch)


def test_word_range(orc, api, emu_lib, mem, ragged, monkeypatch):
    ff.check_word_range(api, emu_lib, ragged, mem, monkeypatch)


def test_chunks_and_hits(orc, api, emu_lib, mem, ragged, monkeypatch):
    ff.check_chunks_and_hits(api, emu_lib, ragged, mem, monkeypatch)


def test_grow_and_shrink(orc, api, emu_lib, mem, ragged, monkeypatch):
    ff.check_grow_and_shrink(api, emu_lib, ragged, mem, monkeypatch)


def test_chunk_tail(orc, api, emu_lib, mem, ragged, monkeypatch):
    ff.check_chunk_tail(api, emu_lib, ragged, mem, monkeypatch)


def test_bsgs(orc, api, emu_lib, mem, ragged, monkeypatch):
    ff.check_bsgs(api, emu_lib, ragged, mem, monkeypatch)


def test_full_tiles_lengths(orc, api, emu_lib, mem, full, monkeypatch):
    assert full.logn == 12
    ff.check_lengths(api, emu_lib, full, mem, monkeypatch)


def test_full_tiles_word_range(orc, api, emu_lib, mem, full, monkeypatch):
    ff.check_word_range(api, emu_lib, full, mem, monkeypatch)


def test_full_tiles_chunks_and_hits(orc, api, emu_lib, mem, full, monkeypatch):
    ff.check_chunks_and_hits(api, emu_lib, full, mem, monkeypatch)


def test_full_tiles_grow_and_shrink(orc, api, emu_lib, mem, full, monkeypatch):
    ff.check_grow_and_shrink(api, emu_lib, full, mem, monkeypatch)


def test_full_tiles_chunk_tail(orc, api, emu_lib, mem, full, monkeypatch):
    ff.check_chunk_tail(api, emu_lib, full, mem, monkeypatch, oracle=False)


@pytest.mark.parametrize("name", ["t33_60x3", "t60_55x3"])
def test_plain_moduli(orc, api, emu_lib, mem, monkeypatch, name):
    """the scaling variant's one definition at the 33- and the 60-bit plain modulus (t above every prime at t60_55x3)"""
    S, _ = pm.hot_setup(orc, api, emu_lib, name)
    ff.check_one_call(api, emu_lib, S, mem, monkeypatch)
