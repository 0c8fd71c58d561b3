"""The chainable packed FC (hhe_fc_open_ks), hhe_square and the network call hhe_mlp_ks on the device: the cases of the emulator suite
(tests/test_mlp_emu.py) on the kernels, the square at the benchmarked degree N = 2^15, BFVDefault(4096), and the deployed parameter
set BFVDefault(16384) with keys generated on the device -- one 10 x 784 open layer word for word, and a (16 x 784, 10 x 16) network on
four MNIST images against plain integers and against the composed public calls.  Run on an MI355X: python -m pytest tests -m gpu."""
import json
import os

import numpy as np
import pytest

import definition_common as dc
import fc_packed_common as fp
import keygen_common as kg
import mlp_common as mc
import parity_common as pc
import rot_many_common as rmc

pytestmark = pytest.mark.gpu
T = fp.T
HERE = os.path.dirname(os.path.abspath(__file__))
PARAMS = {"n1024": (10, [50] * 3), "n4096": (12, [60] * 3)}


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


@pytest.fixture(scope="module")
def S3(orc):
    """N = 1024, 3 x 50 bits: every default Galois key and a key for each of -1 .. -7"""
    return rmc.setup_with_steps(orc, 10, orc.coeff_modulus_create(1024, [50] * 3), [-e for e in range(1, 8)], all_default=True)


@pytest.fixture(scope="module")
def NET(orc):
    return mc.network_setup(orc, "6x20_3x6")


def _lctx(api, lib, S, row_kernel=None):
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    if row_kernel is not None:
        assert X.query("row_kernel") == row_kernel
    S.load_keys(X)
    return X


# ---- the square ----
@pytest.mark.parametrize("name", list(PARAMS))
def test_square_is_the_oracles_multiply(orc, api, lib, mem, name):
    logn, bits = PARAMS[name]
    E = dc.env(orc, logn, orc.coeff_modulus_create(1 << logn, bits), T)
    X = api.Context(E.logn, E.q, E.t, lib=lib)
    for pattern in ("enc", "max", "alt", "rand", "half"):
        for B in (1, 3):
            mc.check_square(X, E, mem, B, pattern, seed=11 + B)
    X.close()


def test_square_at_the_benchmarked_degree(orc, api, lib, mem):
    """N = 2^15 over 4 x 60 bits, every word q_j - 1: hhe_multiply(a, a) on the device for every item, the oracle on one"""
    q = orc.coeff_modulus_create(1 << 15, [60] * 4)
    E = dc.env(orc, 15, q, T)
    X = api.Context(15, q, T, lib=lib)
    mc.check_square(X, E, mem, 2, "max", oracle_items=[0])
    X.close()


# ---- one open layer ----
@pytest.mark.parametrize("rows,cols,rc,ks", mc.OPEN_SHAPES)
def test_layer_words_slots_and_counters(orc, api, lib, mem, S3, rows, cols, rc, ks):
    X = _lctx(api, lib, S3, 0)
    M = fp.seeded_matrix(T, rows, cols, 7 * rows + cols)
    got, _, xs, xs1 = mc.check_open_layer(X, S3, mem, orc, M, B=2, seed=rows)
    assert X.query("fc_packed_key_switches") == ks
    mc.check_open_slots(S3, got, M, xs, xs1)
    X.close()


def test_layer_over_the_naf_trie(orc, api, lib, mem):
    S = fp.make_setup(orc, 10, orc.coeff_modulus_create(1024, [50] * 3))
    X = _lctx(api, lib, S, 0)
    M = fp.seeded_matrix(T, 5, 250, 17)
    trie = rmc.RotTrie(orc, 1024, [-e for e in range(1, 8)], S.gk.elts)
    got, _, xs, xs1 = mc.check_open_layer(X, S, mem, orc, M, B=2, seed=21)
    assert X.query("fc_packed_key_switches") == trie.nodes + 6
    rmc.expect_queries(X, trie)
    mc.check_open_slots(S, got, M, xs, xs1)
    X.close()


def test_mnist_shape_on_the_row_kernels(orc, api, lib, mem):
    S = fp.make_setup(orc, 12, orc.coeff_modulus_create(4096, [60] * 3), steps=mc.hand_open_steps(4096, 10, 784))
    X = _lctx(api, lib, S, 1)
    M = fp.seeded_matrix(T, 10, 784, 5)
    got, _, xs, xs1 = mc.check_open_layer(X, S, mem, orc, M, B=1, seed=6)
    assert X.query("fc_packed_key_switches") == 15 + 6
    mc.check_open_slots(S, got, M, xs, xs1)
    X.close()


def test_layer_at_a_level(orc, api, lib, mem):
    mc.check_level(orc, api, lib, mem)


def test_bfv_default_4096(orc, api, lib, mem):
    """BFVDefault(4096), 36 + 36 + 37 bits, 3 x 5: the separate-kernel path at full tiles"""
    S = fp.make_setup(orc, 12, api.bfv_default_coeff_modulus(4096, lib), steps=mc.hand_open_steps(4096, 3, 5))
    X = _lctx(api, lib, S, 0)
    M = fp.seeded_matrix(T, 3, 5, 9)
    got, _, xs, xs1 = mc.check_open_layer(X, S, mem, orc, M, B=2, seed=1)
    mc.check_open_slots(S, got, M, xs, xs1)
    X.close()


# ---- networks ----
@pytest.mark.parametrize("name", list(mc.NETWORKS))
def test_network_words_and_slots(orc, api, lib, mem, name):
    S = mc.network_setup(orc, name)
    X = _lctx(api, lib, S, 1 if S.n >= 4096 else 0)
    mc.check_network(X, S, mem, mc.NETWORKS[name][2], B=1 if S.n >= 4096 else 2, seed=3)
    X.close()


def test_one_layer_network_is_the_open_layer(api, lib, mem, NET):
    X = _lctx(api, lib, NET)
    mc.check_one_layer_network(X, NET, mem)
    X.close()


def test_chunks_and_streams_do_not_change_the_words(api, lib, mem, NET, monkeypatch):
    mc.check_chunking(lambda: _lctx(api, lib, NET), NET, mem, monkeypatch)


def test_in_place(api, lib, mem, NET):
    X = _lctx(api, lib, NET)
    mc.check_network(X, NET, mem, mc.SHAPES_NET, B=3, seed=8, in_place=True)
    X.close()


def test_forced_fallback_and_no_hoisting(api, lib, mem, NET, monkeypatch):
    mc.check_fallback(lambda: _lctx(api, lib, NET), NET, mem, monkeypatch)


def test_lifecycle(api, lib, mem, NET):
    X = _lctx(api, lib, NET)
    mc.check_lifecycle(X, NET, mem)
    X.close()


def test_refusals_leave_out_untouched(api, lib, mem, NET):
    X, Y = _lctx(api, lib, NET), _lctx(api, lib, NET)
    mc.check_refusals(X, Y, NET, mem, api)
    Y.close()
    X.close()


def test_refused_above_the_cap(orc, api, lib, mem):
    mc.check_cap_refusal(orc, api, lib, mem)


# ---- the deployed parameter set, keys generated on the device ----
class Deployed:
    """BFVDefault(16384): secret, public and relinearization key and the Galois keys of `steps`, all made on the device; their host
    copies in the oracle's form serve truth 2"""

    def __init__(self, orc, api, lib, mem, steps):
        self.logn, self.n, self.t = 14, 1 << 14, T
        self.q = api.bfv_default_coeff_modulus(self.n, lib)
        self.O = orc.Oracle(self.logn, self.q, T)
        self.X = api.Context(self.logn, self.q, T, lib=lib)
        assert self.X.query("row_kernel") == 1
        D = kg.DeviceKeys(self.X, self.O, mem, kg.SEED)
        self.sk, self.pk = D.sk, D.pk
        elts = list(dict.fromkeys(int(self.O.galois_elt(s)) for s in steps))
        self.ks = D.keyset(elts)
        self.rk = self.ks.get_relin()
        self.gk = kg.oracle_gk(orc, self.ks, elts)

    def close(self):
        self.ks.close()
        self.X.close()


def test_deployed_parameters_one_layer_words(orc, api, lib, mem):
    """one item of 10 x 784 open, word for word against the oracle's composition around hhe_multiply_sum, and its slots"""
    S = Deployed(orc, api, lib, mem, mc.hand_open_steps(1 << 14, 10, 784))
    M = fp.seeded_matrix(T, 10, 784, 5)
    got, _, xs, xs1 = mc.check_open_layer(S.X, S, mem, orc, M, B=1, seed=6, rk=S.ks, gk=S.ks)
    mc.check_open_slots(S, got, M, xs, xs1)
    S.close()


def _mnist_pixels(count):
    fx = json.load(open(os.path.join(HERE, "golden", "mnist_64.json")))
    packed = np.array([list(bytes.fromhex(h)) for h in fx["pixels_2bit_hex"][:count]], dtype=np.uint8)
    return ((packed[:, :, None] >> (2 * np.arange(4))) & 3).reshape(count, 784).astype(np.uint64)


def test_deployed_parameters_mnist_network(orc, api, lib, mem):
    """(16 x 784, 10 x 16) on four MNIST images under seeded random weights: M_2 (M_1 x)^2 mod t in plain integers, the device's noise
    budget positive, and hhe_mlp_ks == the composed public calls.  The images sit in slots [0, 784) of row 0; every other slot of
    both rows holds a random value"""
    shapes = [(16, 784), (10, 16)]
    S = Deployed(orc, api, lib, mem, mc.all_steps(1 << 14, shapes))
    X, O, NS = S.X, S.O, 4
    Ms = [fp.seeded_matrix(T, r, c, 50 + k) for k, (r, c) in enumerate(shapes)]
    pix = _mnist_pixels(NS)
    vals = np.random.default_rng(77).integers(0, T, size=(NS, S.n), dtype=np.uint64)
    vals[:, :784] = pix

    def encrypt(slot_rows, seed):
        k = len(slot_rows)
        plain, ct = mem.empty((k, S.n)), mem.empty((k,) + tuple(O.ct_shape))
        X.encode(mem.to_dev(slot_rows), k, S.n, plain)
        X.encrypt(mem.to_dev(S.pk), plain, bytes((seed + i) % 256 for i in range(32)), k, ct)
        return ct

    def diag_rows(M):
        d = np.array(mc.hand_open_diagonals(M), dtype=np.uint64)
        full = np.zeros((len(d), S.n), np.uint64)
        full[:, :d.shape[1]] = d
        full[:, S.n // 2:S.n // 2 + d.shape[1]] = d
        return full
    d_x = encrypt(vals, 1)
    mats = [X.enc_matrix_open(encrypt(diag_rows(M), 2 + k), *M.shape) for k, M in enumerate(Ms)]
    shape = (NS,) + tuple(O.ct_shape)
    out = X.mlp(mats, d_x, mem.empty(shape), NS, rk=S.ks, gk=S.ks)
    assert X.query("mlp_layers") == 2
    budget = X.noise_budget(S.sk, out, NS)
    print("noise budget of hhe_mlp_ks (16 x 784, 10 x 16) at BFVDefault(16384): %s" % [int(v) for v in budget])
    assert (budget > 0).all()
    dec = mem.empty((NS, S.n))
    X.decrypt(S.sk, out, NS, dec)
    dec = mem.to_host(dec)
    for b in range(NS):
        assert [int(v) for v in dec[b, :10]] == mc.plain_mlp(Ms, pix[b], T), ("row 0", b)
        assert [int(v) for v in dec[b, S.n // 2:S.n // 2 + 10]] == mc.plain_mlp(Ms, vals[b, S.n // 2:S.n // 2 + 784], T), ("row 1", b)
    want = mc.composed(X, mem, mats, d_x, NS, O.ct_shape, rk=S.ks, gk=S.ks)
    assert (mem.to_host(out) == mem.to_host(want)).all(), "hhe_mlp_ks differs from the composed public calls"
    for m in mats:
        m.destroy()
    S.close()
