"""The ciphertext side against its definitions in Python integers (definition_common.py) on the GPU: the checks test_definitions.py
runs on the emulator, at the degrees and prime sets where the kernels take another path.  The negacyclic NTT at N = 2^10 .. 2^16 over
CoeffModulus::Create primes of 60 bits (pm_fold butterflies) and over BFVDefault(4096) (Harvey butterflies); the key switch with
sparse keys and on the rounding boundary, full vector, at every tiling of the row kernel (N = 2^12 .. 2^16), on the separate-kernel
and digit-reducing contexts at N = 4096 and on the ragged tiles below; real keys at sampled coefficients, once at the benchmark's
parameters; add_plain at the three plain moduli; BEHZ multiply as a distance.  One item or one batch of three per call: the device
time is milliseconds, what a test costs is the integer work on the host.  Run on an MI355X: python -m pytest tests -m gpu."""
import pytest

import definition_common as dc
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


# sampled output words beside 0, 1, N/2, N - 1: 12, 16 from N = 2^15 on; 8 at N = 2^16, where the 27 Horner evaluations of one word cost 0.2 s
NTT_SAMPLES = {15: 16, 16: 8}


@pytest.mark.parametrize("name", ["ntt%d" % logn for logn in range(10, 17)] + ["A"])
def test_ntt_is_the_negacyclic_evaluation(orc, api, lib, mem, name):
    """a, b. roots, then hhe_ntt and the oracle's transforms over the 4 coefficient primes, the 4 BEHZ primes and t"""
    E, make_ctx = dc.setup(orc, api, lib, name)
    dc.check_roots(make_ctx, E)
    dc.check_ntt(make_ctx, E, mem, samples=NTT_SAMPLES.get(E.logn, 12))


ROW = ["row%d" % logn for logn in range(12, 17)]
OTHER = ["A", "E", "F2", "G", "H", "n1024", "n2048"]


@pytest.mark.parametrize("name", ROW + OTHER)
def test_key_switch_sparse_keys(orc, api, lib, mem, name):
    """d. three-monomial keys, full vector, through relinearize, apply_galois, rotate_rows (once in place) and rotate_columns; three
    distinct items per call up to N = 4096, one item above"""
    E, make_ctx = dc.setup(orc, api, lib, name)
    dc.check_switch_sparse(make_ctx, E, mem, B=3 if E.logn <= 12 else 1)


@pytest.mark.parametrize("name", ROW + OTHER)
def test_key_switch_rounding_boundary(orc, api, lib, mem, name):
    """d. X_k walks m p - h - 1, m p - h, m p - h + 1 for m in {0, 1, 2, Q - 1, Q}, and 0, h, Q p - 1: the half of the mod-down"""
    E, make_ctx = dc.setup(orc, api, lib, name)
    dc.check_switch_boundary(make_ctx, E, mem)


@pytest.mark.parametrize("name", ["row12", "A", "n1024", "n2048"])
def test_rotation_through_naf_terms(orc, api, lib, mem, name):
    """d. rotate_rows(3) without its key is the switch of step -1 followed by the switch of step 4"""
    E, make_ctx = dc.setup(orc, api, lib, name)
    dc.check_switch_naf(make_ctx, E, mem)


@pytest.mark.parametrize("name", ["row12", "A", "bench15"])
def test_key_switch_real_keys_sampled(orc, api, lib, mem, name):
    """d. the oracle's relin and Galois keys, CRT-lifted per coefficient, at 16 output coefficients; at N = 32768 with 4 x 60 bits
    (the benchmark's parameters) relinearize and rotate_rows only"""
    E, make_ctx = dc.setup(orc, api, lib, name)
    dc.check_switch_real(make_ctx, E, mem, which=[("relin",), ("rows", -1)] if name == "bench15" else None)


@pytest.mark.parametrize("name", ["n1024-t16", "n1024-t33", "n1024-t60", "row12-t16", "row12-t33", "A-t16", "A-t33"])
def test_add_plain_is_the_rounded_scaling(orc, api, lib, mem, name):
    """e. c0 += floor((m Q + (t + 1) / 2) / t) mod q_j, per item, broadcast and subtracting"""
    E, make_ctx = dc.plain_case(orc, api, lib, name)
    dc.check_add_plain(make_ctx, E, mem)


@pytest.mark.parametrize("name", ["n1024", "row12", "A"])
def test_behz_multiply_distance(orc, api, lib, mem, name):
    """f. at most L + 1 = 3 from the rounded integer tensor product at 32 coefficients, six input pairs (the last: every coefficient (Q - 1) / 2, squared).  Largest distance observed on
    the oracle: 2 at N = 1024 (3 x 50 bits), 2 at N = 4096 (3 x 60 bits) and 2 on BFVDefault(4096)."""
    E, make_ctx = dc.setup(orc, api, lib, name)
    dc.check_behz(make_ctx, E, mem)
