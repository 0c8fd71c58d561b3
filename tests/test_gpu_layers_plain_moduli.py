"""The packed encrypted layers and the FC-square-FC call at the plain moduli 8088322049 and 1096486890805657601 on the device: the cases
of tests/test_layers_plain_moduli_emu.py on the kernels, and the one degree at which 65537 does not batch -- N = 65536 over 4 x 60
bits, one item, with exactly the Galois keys of its steps.  One or two items per call; what a test costs is the oracle's work on the
host.  Run on an MI355X: python -m pytest tests -m gpu."""
import pytest

import layer_moduli_common as lm
import parity_common as pc

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("t", [lm.T16, lm.T33, lm.T60])
def test_diagonals_functions(api, lib, t):
    lm.check_diagonals(api, lib, t)


@pytest.mark.parametrize("name,which", lm.layer_cases())
def test_five_forms_of_a_layer(orc, api, lib, mem, name, which):
    S, rows, cols, B, row_kernel = lm.layer_setup(orc, name, which)
    X = lm.load_ctx(api, lib, S, row_kernel)
    lm.check_five_forms(X, S, mem, orc, rows, cols, B, seed=11 + which)
    X.close()


@pytest.mark.parametrize("name", list(lm.NETS))
def test_network_words_slots_and_budget(orc, api, lib, mem, name):
    S, shapes = lm.net_setup(orc, name)
    X = lm.load_ctx(api, lib, S, 0)
    lm.check_net(X, S, mem, shapes)
    X.close()
