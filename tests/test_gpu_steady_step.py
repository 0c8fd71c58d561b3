"""The steady transciphering step on the gfx950 kernels (steady_step_common): the item kernel launched in front of the key comparison,
reading the items' words out of the host's page-locked staging, with a pointer table that goes up only when it changed.  Every check is
exact equality of ciphertext words with a context under HHE_FIN_ITEM=0 and, for named items, the oracle's transcipher_block; the
uploads and launches each call enqueued are read from the context.

Shapes: N = 1024 and N = 4096 over 3 x 50 bits (tests/test_gpu_fin_item.py's), three to seven items under HHE_FIN_ITEM=1; 64 items at
N = 1024 where the default threshold between the two paths is the subject."""
import pytest

import parity_common as pc
import steady_step_common as ss
from conftest import Setup


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
def ragged(orc):
    return Setup(orc, 10, [50] * 3)


@pytest.fixture(scope="module")
def full(orc):
    return Setup(orc, 12, [50] * 3)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["ragged", "full"])
@pytest.mark.parametrize("name", ["check_same_table_new_words", "check_table_changes", "check_growth", "check_keys", "check_cache_cleared"])
def test_gpu_steady_step(orc, api, lib, mem, monkeypatch, request, name, shape):
    getattr(ss, name)(api, lib, request.getfixturevalue(shape), mem, monkeypatch)


@pytest.mark.gpu
def test_gpu_both_paths_on_one_context(orc, api, lib, mem, ragged, monkeypatch):
    ss.check_both_paths(api, lib, ragged, mem, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["check_same_table_new_words", "check_keys"])
def test_gpu_no_internal_lane(orc, api, lib, mem, ragged, monkeypatch, name):
    getattr(ss, name)(api, lib, ragged, mem, monkeypatch, HHE_STREAMS=0)
