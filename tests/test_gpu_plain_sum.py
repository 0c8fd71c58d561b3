"""The plain-weights sum of rotations (hhe_rotate_plain_sum_ks) and the open FC layer under plain weights (hhe_fc_open_plain_ks) on the
device: the cases of the emulator suite (tests/test_plain_sum_emu.py) on the kernels, one case per row-pass size of
ks_plain_sum_row_kernel, BFVDefault(4096), and the deployed parameter set BFVDefault(16384) with keys generated on the device.
Run on an MI355X: python -m pytest tests -m gpu."""
import json
import os

import numpy as np
import pytest

import definition_common as dc
import fc_packed_common as fp
import keygen_common as kg
import mlp_common as mc
import parity_common as pc
import plain_sum_common as ps

pytestmark = pytest.mark.gpu
T = ps.T
HERE = os.path.dirname(os.path.abspath(__file__))
STEPS17 = [1, -1, 0, 2, 3, -3, 1, 4, -4, 5, 6, 7, -7, 8, 0, 9, 10]
CASES = {"n1024": (10, [50] * 3, 0), "row12": (12, [60] * 3, 1)}


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


_setups = {}


def _setup(orc, name):
    """a key for every step of STEPS17 and of the 3 x 5 layer"""
    if name not in _setups:
        logn, bits, _ = CASES[name]
        steps = sorted(set(s for s in STEPS17 if s) | set(mc.hand_open_steps(1 << logn, 3, 5)))
        _setups[name] = pc.setup_from_primes(orc, logn, orc.coeff_modulus_create(1 << logn, bits), T, extra_steps=steps, base_steps=())
    return _setups[name]


def _lctx(api, lib, S, row_kernel=None):
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    if row_kernel is not None:
        assert X.query("row_kernel") == row_kernel
    S.load_keys(X)
    return X


# ---- the cases of the emulator suite ----
@pytest.mark.parametrize("name", list(CASES))
def test_definition(orc, api, lib, mem, name):
    """truth 1: sparse keys and plaintexts (full vector), the rounding boundary of the sum, real keys at sampled coefficients"""
    E, make_ctx = dc.setup(orc, api, lib, name)
    ps.check_definition_sparse(make_ctx, E, mem)
    ps.check_definition_sparse(make_ctx, E, mem, steps=(2, 2, -2, 0, 0, 5), seed=3)
    ps.check_definition_boundary(make_ctx, E, mem)
    S = _setup(orc, name)
    assert S.q == E.q
    ps.check_definition_real_keys(make_ctx, S, E, mem)
    ps.check_definition_dense(make_ctx, S, E, mem)


def test_definition_t_above_every_prime(orc, api, lib, mem):
    q = orc.coeff_modulus_create(1024, [55] * 4)
    E = dc.env(orc, 10, q, dc.T60)
    ps.check_definition_sparse(lambda: api.Context(10, q, dc.T60, lib=lib), E, mem)


@pytest.mark.parametrize("name", list(CASES))
def test_one_child_and_child_counts(orc, api, lib, mem, name):
    """truth 2 (n = 1, the plaintext 1: the oracle's rotate_rows), then n = 1, 2, fold + 1, 17 on B = 1 and 3 behind a decryption"""
    S = _setup(orc, name)
    X = _lctx(api, lib, S, CASES[name][2])
    ps.check_one_child_is_rotate_rows(X, S, mem, [1, -3, 0, 7])
    fold = X.query("plain_sum_fold")
    for B in (1, 3):
        cts = ps.encryptions(S, B, 300)
        for n in (1, 2, fold + 1, 17):
            ps.check_primitive(X, S, mem, STEPS17[:n], cts=cts, seed=n)
    ps.check_primitive(X, S, mem, [0, 0], B=1, seed=50)
    assert X.query("plain_sum_fallbacks") == 0
    X.close()


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("pattern", ["max", "alt", "uniform"])
def test_words_at_their_bounds(orc, api, lib, mem, name, pattern):
    E, make_ctx = dc.setup(orc, api, lib, name)
    ps.check_bounds(make_ctx, E, mem, pattern, STEPS17)


@pytest.mark.parametrize("logn", [12, 13, 15])
def test_every_row_pass_size(orc, api, lib, mem, logn):
    """row passes of 2^6, 2^7, 2^8 points (N = 2^12, 2^13, 2^15) over 4 x 60 bits, four children, every word q_j - 1"""
    q = orc.coeff_modulus_create(1 << logn, [60] * 4)
    E = dc.env(orc, logn, q, T)

    def make_ctx():
        X = api.Context(logn, q, T, lib=lib)
        assert X.query("row_kernel") == 1
        return X
    ps.check_bounds(make_ctx, E, mem, "max", STEPS17, counts=(4,), samples=2)


@pytest.mark.parametrize("name", list(CASES))
def test_fallback_knobs_chunks_and_in_place(orc, api, lib, mem, monkeypatch, name):
    S, rowk = _setup(orc, name), CASES[name][2]
    steps = STEPS17[:5]
    cts = ps.encryptions(S, 5, 220)
    X = _lctx(api, lib, S, rowk)
    got, _, rows = ps.check_primitive(X, S, mem, steps, cts=cts, seed=6)
    assert (ps.run_plain_sum(X, mem, cts, rows, steps, in_place=True) == got).all()
    # one transparent item among ordinary ones: the flag, the recomputation, the same words for the others
    c2 = cts.copy()
    c2[1, 1] = 0
    g2 = ps.run_plain_sum(X, mem, c2, rows, steps)
    assert X.query("plain_sum_fallbacks") == 1 and (g2[[0, 2, 3, 4]] == got[[0, 2, 3, 4]]).all()
    X.close()
    for chunk, streams, hoist in (("2", "2", "1"), ("8", "0", "1"), ("4", "2", "2"), ("128", "1", "0")):
        monkeypatch.setenv("HHE_CHUNK", chunk)
        monkeypatch.setenv("HHE_STREAMS", streams)
        monkeypatch.setenv("HHE_ROT_HOIST", hoist)
        Y = _lctx(api, lib, S, rowk)
        assert (ps.run_plain_sum(Y, mem, cts, rows, steps, in_place=hoist == "2") == got).all(), (chunk, streams, hoist)
        assert Y.query("plain_sum_fallbacks") == (3 if hoist == "2" else 0)
        assert Y.query("plain_sum_launches") == (rowk if hoist != "0" else 0) and Y.query("plain_sum_mod_downs") == 1
        assert (ps.run_plain_sum(Y, mem, c2, rows, steps) == g2).all()
        Y.close()


def test_one_zero_residue_over_small_primes(orc, api, lib, mem):
    import rot_many_common as rm
    logn, bits = pc.ZERO_CASES["n1024_18x4"][:2]
    S = rm.setup_with_steps(orc, logn, orc.coeff_modulus_create(1 << logn, bits), [1, 2, 3])
    cts = next(c for c in (rm.encryptions(S, 3, seed=s) for s in range(180, 200)) if (c[:, 1] != 0).all())
    X = _lctx(api, lib, S, 0)
    ones = np.ones((1, S.n), np.uint64)
    assert (ps.run_plain_sum(X, mem, cts, ones, [2])[2] == S.O.rotate_rows(cts[2], 2, S.gk)[0]).all()
    assert X.query("plain_sum_fallbacks") == 0
    cts[2, 1, 1, 517] = 0
    assert (ps.run_plain_sum(X, mem, cts, ones, [2])[2] == S.O.rotate_rows(cts[2], 2, S.gk)[0]).all()
    assert X.query("plain_sum_fallbacks") == 1
    X.close()


@pytest.mark.parametrize("rows,cols", [(3, 5), (1, 8), (4, 4), (2, 511), (5, 250), (8, 3)])
def test_layer_shapes(orc, api, lib, mem, rows, cols):
    S = ps.layer_setup(orc, 10, orc.coeff_modulus_create(1024, [50] * 3), rows, cols)
    X = _lctx(api, lib, S, 0)
    M = fp.seeded_matrix(T, rows, cols, 7 * rows + cols)
    ps.check_layer(X, S, mem, M, None, B=2, seed=rows)
    ps.check_layer(X, S, mem, M, ps.seeded_bias(T, rows, rows), B=2, seed=rows, in_place=True, budget_beside=rows == 3)
    X.close()


def test_layer_mnist_shape_on_the_row_kernels(orc, api, lib, mem):
    S = ps.layer_setup(orc, 12, orc.coeff_modulus_create(4096, [60] * 3), 10, 784)
    X = _lctx(api, lib, S, 1)
    ps.check_layer(X, S, mem, fp.seeded_matrix(T, 10, 784, 5), ps.seeded_bias(T, 10, 6), B=1, seed=6)
    assert X.query("plain_sum_launches") == 1 and X.query("plain_sum_mod_downs") == 1 and X.query("plain_sum_fallbacks") == 0
    X.close()


def test_bfv_default_4096(orc, api, lib, mem):
    """BFVDefault(4096), 36 + 36 + 37 bits, 3 x 5: the separate-launch path at full tiles"""
    S = ps.layer_setup(orc, 12, api.bfv_default_coeff_modulus(4096, lib), 3, 5)
    X = _lctx(api, lib, S, 0)
    ps.check_layer(X, S, mem, fp.seeded_matrix(T, 3, 5, 9), ps.seeded_bias(T, 3, 2), B=2, seed=1)
    assert X.query("plain_sum_launches") == 0
    X.close()


@pytest.mark.parametrize("name", list(CASES))
def test_refusals_leave_out_untouched(orc, api, lib, mem, name):
    S = _setup(orc, name)
    X, Y = _lctx(api, lib, S), _lctx(api, lib, S)
    ps.check_refusals(X, Y, S, mem, api)
    Y.close()
    X.close()


# ---- the deployed parameter set, keys generated on the device ----
class Deployed:
    """BFVDefault(16384): secret, public and relinearization key and the Galois keys of `steps`, all made on the device; their host
    copies in the oracle's form serve the truths"""

    def __init__(self, orc, api, lib, mem, steps):
        self.logn, self.n, self.t = 14, 1 << 14, T
        self.q = api.bfv_default_coeff_modulus(self.n, lib)
        self.O = orc.Oracle(self.logn, self.q, T)
        self.X = api.Context(self.logn, self.q, T, lib=lib)
        assert self.X.query("row_kernel") == 1
        D = kg.DeviceKeys(self.X, self.O, mem, kg.SEED)
        self.sk, self.pk = D.sk, D.pk
        self.elts = list(dict.fromkeys(int(self.O.galois_elt(s)) for s in steps))
        self.ks = D.keyset(self.elts)
        self.gk = kg.oracle_gk(orc, self.ks, self.elts)

    def close(self):
        self.ks.close()
        self.X.close()


@pytest.fixture(scope="module")
def D16(orc, api, lib, mem):
    S = Deployed(orc, api, lib, mem, mc.hand_open_steps(1 << 14, 10, 784))
    yield S
    S.close()


def _encrypt(S, mem, slot_rows, seed):
    k = len(slot_rows)
    plain, ct = mem.empty((k, S.n)), mem.empty((k,) + tuple(S.O.ct_shape))
    S.X.encode(mem.to_dev(slot_rows), k, slot_rows.shape[1], plain)
    S.X.encrypt(mem.to_dev(S.pk), plain, bytes((seed + i) % 256 for i in range(32)), k, ct)
    return ct


def _mnist(count):
    """(M [10][784] mod t, pixels [count][784], plain logits [count][10]) of the fixtures"""
    fx = json.load(open(os.path.join(HERE, "golden", "mnist_64.json")))
    W = np.array(json.load(open(os.path.join(HERE, "golden", "mnist_1fc.json")))["weights_rows"], dtype=np.int64)
    packed = np.array([list(bytes.fromhex(h)) for h in fx["pixels_2bit_hex"][:count]], dtype=np.uint8)
    pix = ((packed[:, :, None] >> (2 * np.arange(4))) & 3).reshape(count, 784).astype(np.int64)
    assert (pix @ W.T == np.array(fx["plain_logits"][:count])).all()
    return (W % T).astype(np.uint64), pix.astype(np.uint64), np.array(fx["plain_logits"][:count])


def test_deployed_parameters_words(orc, api, lib, mem, D16):
    """one item of 10 x 784 at BFVDefault(16384), word for word, under keys made on the device.  The 16 open diagonals of the fixture's
    weights are DENSE plaintexts: the primitive over (-e, D_e) against the definition at sampled coefficients (every child's X once as an
    integer polynomial, then integer dot products: plain_sum_common.dense_truth), and the layer's words against the oracle's rotate_rows,
    add and add_plain applied to the primitive's words -- the tail and the bias are compositions of SEAL's operations"""
    S, X, O = D16, D16.X, D16.O
    E = dc.env(orc, S.logn, S.q, T)
    M, _, _ = _mnist(1)
    bias = ps.seeded_bias(T, 10, 4)
    r, c = mc.hand_open_shape(S.n, 10, 784)
    assert (r, c) == (16, 1024)
    diag = np.array(mc.hand_open_diagonals(M), dtype=np.uint64)
    steps = [-e for e in range(r)]
    elt = {int(e): k for e, k in zip(S.gk.elts, S.gk.keys)}
    words = [elt[pc.galois_elt_py(S.n, s)] if s else None for s in steps]
    plains = [ps.DensePlain(E, slots=d) for d in diag]
    assert all((p.lift != 0).sum() > S.n // 2 for p in plains[:10])
    vals = np.random.default_rng(3).integers(0, T, size=(1, S.n), dtype=np.uint64)
    ct = mem.to_host(_encrypt(S, mem, vals, 1))
    got = ps.run_plain_sum(X, mem, ct, diag, steps, gk=S.ks)
    ps.expect_counters(X)
    assert X.query("plain_sum_fallbacks") == 0
    idx = [0, S.n - 1, 5003]
    dc.assert_switch("rotate_plain_sum, 10 x 784 at BFVDefault(16384)", (10, 784), got[0], ps.dense_truth(E, list(zip(steps, plains, words)), ct[0], idx), idx)
    y = got[0]
    s = r
    while s < c:
        y = O.add(y, O.rotate_rows(y, s, S.gk)[0])
        s *= 2
    y = O.add_plain(y, O.encode(fp.slot_vector(S.n, bias)))
    mat = X.plain_fc_open(M, bias)
    layer = mem.to_host(mat.apply(mem.to_dev(ct), 1, gk=S.ks, out=mem.empty(ct.shape)))
    mat.destroy()
    assert (layer[0] == y).all(), "hhe_fc_open_plain_ks differs from the primitive's words under the oracle's tail and add_plain"
    # truth 2 under a device-made key
    ones = np.ones((1, S.n), np.uint64)
    assert (ps.run_plain_sum(X, mem, ct, ones, [-7], gk=S.ks)[0] == O.rotate_rows(ct[0], -7, S.gk)[0]).all()


def test_deployed_parameters_mnist(orc, api, lib, mem, D16):
    """four MNIST images under the fixture's weights and a seeded bias: the ten logits against plain integers mod t and against the slots
    of hhe_fc_open_ks (encrypted weights) on the same inputs; the device's noise budget positive.  The images sit in slots [0, 784) of
    row 0; every other slot of both rows holds a random value"""
    S, X, O, NS = D16, D16.X, D16.O, 4
    M, pix, plain = _mnist(NS)
    bias = ps.seeded_bias(T, 10, 4)
    vals = np.random.default_rng(77).integers(0, T, size=(NS, S.n), dtype=np.uint64)
    vals[:, :784] = pix
    d_x = _encrypt(S, mem, vals, 1)
    shape = (NS,) + tuple(O.ct_shape)

    def logits(ct):
        dec = mem.empty((NS, S.n))
        X.decrypt(S.sk, ct, NS, dec)
        return mem.to_host(dec)[:, :10].astype(np.int64)
    mat = X.plain_fc_open(M, bias)
    print("plain-weights handle of 10 x 784 at BFVDefault(16384): %d bytes" % mat.bytes)
    out = mat.apply(d_x, NS, gk=S.ks, out=mem.empty(shape))
    ps.expect_counters(X)
    assert X.query("plain_sum_fallbacks") == 0
    budget = X.noise_budget(S.sk, out, NS)
    assert (budget > 0).all()
    got = logits(out)
    assert (got == (plain + bias.astype(np.int64)) % T).all()
    mat.destroy()
    nobias = X.plain_fc_open(M)
    out0 = nobias.apply(d_x, NS, gk=S.ks, out=mem.empty(shape))
    nobias.destroy()
    d = np.array(mc.hand_open_diagonals(M), dtype=np.uint64)
    full = np.zeros((len(d), S.n), np.uint64)
    full[:, :d.shape[1]] = d
    enc = X.enc_matrix_open(_encrypt(S, mem, full, 2), 10, 784)
    ref = enc.apply_open(d_x, NS, rk=S.ks, gk=S.ks, out=mem.empty(shape))
    b_enc = X.noise_budget(S.sk, ref, NS)
    enc.destroy()
    assert (logits(out0) == logits(ref)).all() and (logits(ref) == plain % T).all()
    print("noise budget of the 10 x 784 layer at BFVDefault(16384): plain weights %s, encrypted weights %s" % ([int(v) for v in budget], [int(v) for v in b_enc]))
