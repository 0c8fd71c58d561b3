"""The packed encrypted layers at the plain moduli of the reference other than 65537 (configs/config.cpp:19-26): 8088322049 (T33), the
one that batches at N = 65536, and 1096486890805657601 (T60).  The case table and the steps of a case, shared by the emulator suite
(numpy memory) and the GPU suite (torch memory).  t enters these layers through the diagonals functions, encode, the factor t of the
floor in the tensor kernels, behz_sum_cap and with it whether the sum forms serve; the checkers are the ones the layers have at 65537
(fc_packed_common, rot_many_common, mult_sum_common, mlp_common), with their Setup built at t: the words of every form against its
reference, the slots against Python integers mod t.  Matrix entries and inputs are drawn over the whole of [0, t)."""
import numpy as np
import pytest

import fc_packed_common as fp
import mlp_common as mc
import mult_sum_common as ms
import plain_modulus_common as pm
import rot_many_common as rmc

T16, T33, T60 = pm.T16, pm.T33, pm.T60

# name: (t, logn, prime bit sizes, [(rows, cols, B)], expected row_kernel); the oracle's budgets, input -> layer: 107 -> 64, 280 -> 209,
# 76 -> 32 (3 x 5) and 76 -> 26 (10 x 784), 135 -> 85
LAYERS = {
    "t33_1024": (T33, 10, [50] * 4, [(3, 5, 2)], 0),
    "t60_slow": (T60, 10, [50] * 8, [(3, 5, 2)], 0),           # t > 2 q_j: the slow lift
    "t33_row": (T33, 12, [60] * 3, [(3, 5, 2), (10, 784, 1)], 1),
    "t33_65536": (T33, 16, [60] * 4, [(3, 5, 1)], 1),         # 65537 does not batch at this degree; GPU suite only
}
# name: (t, logn, prime bit sizes, [(rows, cols), ..]); budgets input -> layer -> square -> layer: 207 -> 163 -> 121 -> 78 and
# 280 -> 208 -> 139 -> 69
NETS = {
    "net_t33": (T33, 10, [50] * 6, [(6, 20), (3, 6)]),
    "net_t60": (T60, 10, [50] * 8, [(6, 20), (3, 6)]),
}
_setups = {}


def layer_cases(max_logn=16):
    return [(name, i) for name, case in LAYERS.items() if case[1] <= max_logn for i in range(len(case[3]))]


def layer_setup(orc, name, which):
    """(Setup with exactly the Galois keys of the five forms of the shape, rows, cols, B, expected row_kernel)"""
    t, logn, bits, shapes, row_kernel = LAYERS[name]
    rows, cols, B = shapes[which]
    if (name, which) not in _setups:
        n = 1 << logn
        q = pm.primes_near(orc, n, bits)
        if name == "t60_slow":
            assert pm.regime_of(t, q[:-1]) == "slow"
        steps = sorted(set(fp.hand_steps(n, rows, cols)) | set(rmc.hand_hoisted_steps(n, rows, cols)) | set(mc.hand_open_steps(n, rows, cols)))
        _setups[(name, which)] = fp.make_setup(orc, logn, q, t=t, steps=steps)
    return _setups[(name, which)], rows, cols, B, row_kernel


def net_setup(orc, name):
    t, logn, bits, shapes = NETS[name]
    if name not in _setups:
        n = 1 << logn
        _setups[name] = rmc.setup_with_steps(orc, logn, pm.primes_near(orc, n, bits), mc.all_steps(n, shapes), all_default=True, t=t)
    return _setups[name], shapes


def load_ctx(api, lib, S, row_kernel=None):
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    if row_kernel is not None:
        assert X.query("row_kernel") == row_kernel
    S.load_keys(X)
    return X


def check_five_forms(X, S, mem, orc, rows, cols, B, seed):
    """hhe_fc_packed_ks, hhe_fc_packed_hoisted_ks, hhe_fc_packed_sum_ks (hoisted 0 and 1) and hhe_fc_open_ks on one matrix over [0, t)"""
    M = fp.seeded_matrix(S.t, rows, cols, seed)
    assert int(M.max()) > S.t // 2 > T16, "the entries do not reach the upper half of [0, t)"
    ms.check_cap(X, _Primes(X, S))
    fp.check_layer(X, S, mem, M, B=B, seed=seed)
    rmc.check_hoisted_layer(X, S, mem, orc, M, B=B, seed=seed)
    for hoisted in (0, 1):
        got, _, xs = ms.check_sum_layer(X, S, mem, M, hoisted, B=B, seed=seed)
        ms.check_sum_slots(S, got, M, xs)
    got, _, xs, xs1 = mc.check_open_layer(X, S, mem, orc, M, B=B, seed=seed)
    mc.check_open_slots(S, got, M, xs, xs1)


class _Primes:
    """what mult_sum_common.check_cap reads of an Env"""

    def __init__(self, X, S):
        self.n, self.q, self.t, self.L = S.n, S.q, S.t, len(S.q) - 1
        self.bsk = [X.query("bsk", i) for i in range(self.L + 1)]
        assert self.bsk == [S.O.query("bsk", i) for i in range(self.L + 1)]


def check_net(X, S, mem, shapes, B=2, seed=3):
    """hhe_mlp_ks == the composed public calls, == plain integers mod t, and the device's noise budget is positive"""
    got, _ = mc.check_network(X, S, mem, shapes, B=B, seed=seed)
    budget = X.noise_budget(S.sk, mem.to_dev(got), B)
    print("device noise budget after %s at t = %d: %s" % (shapes, S.t, [int(v) for v in budget]))
    assert (budget > 0).all()


# ---- the diagonals functions ----
def check_diagonals(api, lib, t):
    """hhe_fc_packed_diagonals and hhe_fc_open_diagonals at t: seeded entries over [0, t) and every entry t - 1 against the formulas by
    hand; an entry equal to t is refused"""
    for rows, cols in ((3, 5), (5, 250), (8, 3)):
        for M in (fp.seeded_matrix(t, rows, cols, 3 * rows + cols), np.full((rows, cols), t - 1, np.uint64)):
            assert api.fc_packed_diagonals(t, M, lib=lib).tolist() == fp.hand_diagonals(M, rows, cols), (t, rows, cols)
            assert api.fc_open_diagonals(t, M, lib=lib).tolist() == mc.hand_open_diagonals(M), (t, rows, cols)
    M = np.full((3, 5), t - 1, np.uint64)
    M[1, 2] = t
    for f in (api.fc_packed_diagonals, api.fc_open_diagonals):
        with pytest.raises(api.HheError) as e:
            f(t, M, lib=lib)
        assert e.value.code == api.ERR_INVALID and "plain modulus" in str(e.value), (t, f.__name__)
