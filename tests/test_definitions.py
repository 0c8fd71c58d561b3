"""The ciphertext side against its definitions in Python integers (definition_common.py), on the oracle and on the tests-only
emulator: roots, the negacyclic NTT over every modulus of a context, the Galois map, the generic key switch through its four entry
points (sparse keys and the rounding boundary on the full vector, real keys at sampled coefficients, a step served through its NAF
terms), add_plain / sub_plain at the three plain moduli and BEHZ multiply as a distance.  A failure names who is wrong: the oracle
and the product are held to the same truth in the same test.  The checks run unchanged on the GPU (test_gpu_definitions.py).

Contexts, chosen for the code they select: N = 1024 with 3 x 50 bits (ragged tiles), N = 4096 with 3 x 60 bits (row kernel), and for
the key switch the dispatch cases A (BFVDefault(4096), separate kernels), G (digit reduction) and H (largest admitted c)."""
import pytest

import definition_common as dc
import parity_common as pc

BOTH = ["n1024", "row12"]
SWITCH = BOTH + ["A", "G", "H"]


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


@pytest.mark.parametrize("name", BOTH)
def test_roots_and_galois_map(orc, api, emu_lib, name):
    """a, c. the minimal primitive 2N-th roots found in Python are the product's and the oracle's; the oracle's coefficient-domain
    Galois map is SURVEY A.3's loop"""
    E, make_ctx = dc.setup(orc, api, emu_lib, name)
    dc.check_roots(make_ctx, E)
    dc.check_galois_map(E)


@pytest.mark.parametrize("name", BOTH)
def test_ntt_is_the_negacyclic_evaluation(orc, api, emu_lib, mem, name):
    """b. hhe_ntt and the oracle's transforms over the K coefficient primes, the L + 1 BEHZ primes and t"""
    E, make_ctx = dc.setup(orc, api, emu_lib, name)
    dc.check_ntt(make_ctx, E, mem)


@pytest.mark.parametrize("name", SWITCH)
def test_key_switch_sparse_keys(orc, api, emu_lib, mem, name):
    """d. three-monomial keys, full vector, three distinct items per call, one call in place"""
    E, make_ctx = dc.setup(orc, api, emu_lib, name)
    dc.check_switch_sparse(make_ctx, E, mem)


@pytest.mark.parametrize("name", SWITCH)
def test_key_switch_rounding_boundary(orc, api, emu_lib, mem, name):
    """d. X_k walks m p - h - 1, m p - h, m p - h + 1 for m in {0, 1, 2, Q - 1, Q}, and 0, h, Q p - 1: the half of the mod-down"""
    E, make_ctx = dc.setup(orc, api, emu_lib, name)
    dc.check_switch_boundary(make_ctx, E, mem)


@pytest.mark.parametrize("name", SWITCH)
def test_key_switch_real_keys_sampled(orc, api, emu_lib, mem, name):
    """d. the oracle's relin and Galois keys, CRT-lifted per coefficient, at 16 output coefficients"""
    E, make_ctx = dc.setup(orc, api, emu_lib, name)
    dc.check_switch_real(make_ctx, E, mem)


@pytest.mark.parametrize("name", SWITCH)
def test_rotation_through_naf_terms(orc, api, emu_lib, mem, name):
    """d. rotate_rows(3) without its key is the switch of step -1 followed by the switch of step 4"""
    E, make_ctx = dc.setup(orc, api, emu_lib, name)
    dc.check_switch_naf(make_ctx, E, mem)


PLAIN = ["n1024-t16", "n1024-t33", "n1024-t60", "row12-t16", "row12-t33"]


@pytest.mark.parametrize("name", PLAIN)
def test_add_plain_is_the_rounded_scaling(orc, api, emu_lib, mem, name):
    """e. c0 += floor((m Q + (t + 1) / 2) / t) mod q_j at 0, 1, (t - 1) / 2, (t + 1) / 2, t - 1 and seeded coefficients"""
    E, make_ctx = dc.plain_case(orc, api, emu_lib, name)
    dc.check_add_plain(make_ctx, E, mem)


@pytest.mark.parametrize("name", BOTH)
def test_behz_multiply_distance(orc, api, emu_lib, mem, name):
    """f. at most L + 1 = 3 from the rounded integer tensor product at 32 coefficients, six input pairs.  Largest distance observed,
    on the oracle and on the emulator alike: 2 at N = 1024 (3 x 50 bits) and 2 at N = 4096 (3 x 60 bits); per pair 2, 1, 1, 2, 2, 2 at
    both (two encryptions; all q_j - 1 squared; alternating against all q_j - 1; two uniform pairs; all (Q - 1) / 2 squared)."""
    E, make_ctx = dc.setup(orc, api, emu_lib, name)
    dc.check_behz(make_ctx, E, mem)
