"""The packed encrypted layers and the FC-square-FC call at the plain moduli 8088322049 and 1096486890805657601 on the tests-only
emulator (built with -DHHE_RANGE_CHECK): the cases of layer_moduli_common up to N = 4096 -- the five forms of a layer word for word
against their references and slot for slot against (M x) mod t, hhe_mlp_ks against the composed public calls and plain integers -- and
the two diagonals functions at all three moduli.  N = 65536 runs in the GPU suite only."""
import pytest

import layer_moduli_common as lm
import parity_common as pc


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


@pytest.mark.parametrize("t", [lm.T16, lm.T33, lm.T60])
def test_diagonals_functions(api, emu_lib, t):
    lm.check_diagonals(api, emu_lib, t)


@pytest.mark.parametrize("name,which", lm.layer_cases(max_logn=12))
def test_five_forms_of_a_layer(orc, api, emu_lib, mem, name, which):
    S, rows, cols, B, row_kernel = lm.layer_setup(orc, name, which)
    X = lm.load_ctx(api, emu_lib, S, row_kernel)
    lm.check_five_forms(X, S, mem, orc, rows, cols, B, seed=11 + which)
    X.close()


@pytest.mark.parametrize("name", list(lm.NETS))
def test_network_words_slots_and_budget(orc, api, emu_lib, mem, name):
    S, shapes = lm.net_setup(orc, name)
    X = lm.load_ctx(api, emu_lib, S)
    lm.check_net(X, S, mem, shapes)
    X.close()
