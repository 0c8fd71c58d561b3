"""The steady transciphering step on the emulator (steady_step_common): each checker eagerly, and under the lazy order of
tests/emu/emu_order.cpp, where the item kernel enqueued in front of the key comparison reads the staged words and the device's table
only when the call's final wait forces the stream -- staging rewritten too early, or a skipped upload the device did not hold, changes
ciphertext words.

The emulator's staging is always page-locked (it defines rt_host_malloc), so the malloc fallback of HostStage -- where the words are
still uploaded -- cannot be taken here without changing the emulator, and no test runs it; the upload it keeps is the one the
two-pass kernels take in every call of these tests (fin_word_uploads of the HHE_FIN_ITEM=0 contexts).

Shapes: N = 1024 and N = 4096 over 3 x 50 bits, the set-ups of tests/test_gpu_fin_item.py."""
import pytest

import steady_step_common as ss
from conftest import Setup

ORDERS = {"eager": ss.eager_order, "lazy": ss.lazy_order}


@pytest.fixture
def mem():
    return ss.KeptMem()


@pytest.fixture(scope="module")
def ragged(orc):
    return Setup(orc, 10, [50] * 3)


@pytest.fixture(scope="module")
def full(orc):
    return Setup(orc, 12, [50] * 3)


def run(name, order, api, emu_lib, mem, S, monkeypatch, **kw):
    with ORDERS[order](emu_lib, monkeypatch):
        getattr(ss, name)(api, emu_lib, S, mem, monkeypatch, **kw)


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("shape", ["ragged", "full"])
def test_same_table_new_words(orc, api, emu_lib, mem, monkeypatch, request, shape, order):
    run("check_same_table_new_words", order, api, emu_lib, mem, request.getfixturevalue(shape), monkeypatch)


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("name", ["check_table_changes", "check_both_paths", "check_growth", "check_cache_cleared"])
def test_steady_step(orc, api, emu_lib, mem, ragged, monkeypatch, name, order):
    run(name, order, api, emu_lib, mem, ragged, monkeypatch)


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("in_place", [False, True])
def test_keys(orc, api, emu_lib, mem, ragged, monkeypatch, in_place, order):
    run("check_keys", order, api, emu_lib, mem, ragged, monkeypatch, in_place=in_place)


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("name", ["check_same_table_new_words", "check_keys"])
def test_no_internal_lane(orc, api, emu_lib, mem, ragged, monkeypatch, name, order):
    run(name, order, api, emu_lib, mem, ragged, monkeypatch, HHE_STREAMS=0)
