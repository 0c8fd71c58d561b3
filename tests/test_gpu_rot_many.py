"""Hoisted rotations (hhe_rotate_rows_many_ks) and the packed encrypted FC with a hoisted chain (hhe_fc_packed_hoisted_ks) on the
device: the cases of the emulator suite on the separate-kernel path (N = 1024) and on the multi-child launch of the key-switch row
kernel (N = 4096), one case per row-pass size the row kernel is instantiated for, BFVDefault(4096), and the deployed parameter set
BFVDefault(16384) with keys for 1 .. 15 generated on the device -- word for word against the oracle (tests/rot_many_common.py), slot
for slot against plain integers.  Run on an MI355X: python -m pytest tests -m gpu."""
import json
import os

import numpy as np
import pytest

import definition_common as dc
import fc_packed_common as fp
import parity_common as pc
import rot_many_common as rm

pytestmark = pytest.mark.gpu
T = rm.T
HERE = os.path.dirname(os.path.abspath(__file__))
MIXED = [1, -1, 3, 5, -5, 7, 100, -100, 511, -511, 0]


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
def S10(orc):
    """N = 1024, 3 x 50 bits: every default Galois key and a key for 3"""
    return rm.setup_with_steps(orc, 10, orc.coeff_modulus_create(1024, [50] * 3), [3], all_default=True)


@pytest.fixture(scope="module")
def S12(orc):
    """N = 4096, 3 x 60 bits (row kernels): every default key and a key for each of 1 .. 17"""
    return rm.setup_with_steps(orc, 12, orc.coeff_modulus_create(4096, [60] * 3), list(range(1, 18)), all_default=True)


def _ctx(api, lib, S, row_kernel=None):
    X = rm.load_ctx(api, lib, S)
    if row_kernel is not None:
        assert X.query("row_kernel") == row_kernel
    return X


def _default_only(orc, S):
    """the Setup of S with the default keys alone (same key words)"""
    from conftest import Setup
    D = Setup.__new__(Setup)
    D.__dict__.update(S.__dict__)
    keep = set(pc.default_galois_elts_py(S.n))
    idx = [i for i, e in enumerate(S.gk.elts) if int(e) in keep]
    D.gk = orc.GaloisKeys([int(S.gk.elts[i]) for i in idx], np.stack([S.gk.keys[i] for i in idx]))
    return D


# ---- N = 1024: the separate kernels ----
def test_n1024_mixed_steps_copies_and_chunks(orc, api, lib, mem, S10, monkeypatch):
    X = _ctx(api, lib, S10, 0)
    cts = rm.encryptions(S10, 5, seed=220)
    got, refs = rm.check_rot_many(X, S10, mem, orc, MIXED, cts=cts)
    assert X.query("rot_many_key_switches") == 12 and X.query("rot_many_launches") == 0 and X.query("rot_many_fallbacks") == 0
    assert (got[10] == cts).all()
    X.close()
    for chunk, streams in (("2", "2"), ("8", "0")):
        monkeypatch.setenv("HHE_CHUNK", chunk)
        monkeypatch.setenv("HHE_STREAMS", streams)
        Y = _ctx(api, lib, S10)
        g2, _ = rm.check_rot_many(Y, S10, mem, orc, MIXED, cts=cts, refs=refs)
        assert (g2 == got).all(), (chunk, streams)
        Y.close()


def test_n1024_default_keys_one_to_fifteen(orc, api, lib, mem, S10):
    D = _default_only(orc, S10)
    X = _ctx(api, lib, D, 0)
    rm.check_rot_many(X, D, mem, orc, list(range(1, 16)), B=3)
    assert X.query("rot_many_key_switches") == 20
    X.close()


def test_n1024_knobs_refusals_and_a_real_zero(orc, api, lib, mem, S10, monkeypatch):
    cts = rm.encryptions(S10, 3, seed=210)
    X, Y = _ctx(api, lib, S10), _ctx(api, lib, S10)
    got, refs = rm.check_rot_many(X, S10, mem, orc, MIXED, cts=cts)
    rm.check_refusals(X, Y, _default_only(orc, S10), mem, api)
    Y.close()
    X.close()
    for knob, fallbacks in (("2", 1), ("0", 0)):
        monkeypatch.setenv("HHE_ROT_HOIST", knob)
        Z = _ctx(api, lib, S10)
        monkeypatch.delenv("HHE_ROT_HOIST")
        g2, _ = rm.check_rot_many(Z, S10, mem, orc, MIXED, cts=cts, refs=refs)
        assert (g2 == got).all() and Z.query("rot_many_fallbacks") == fallbacks
        Z.close()
    # one residue of c1 at 0 in one limb, over 18-bit primes
    logn, bits = pc.ZERO_CASES["n1024_18x4"][:2]
    S = rm.setup_with_steps(orc, logn, orc.coeff_modulus_create(1 << logn, bits), [1, 2, 3])
    cts = next(c for c in (rm.encryptions(S, 3, seed=s) for s in range(180, 200)) if (c[:, 1] != 0).all())
    Z = _ctx(api, lib, S, 0)
    rm.check_rot_many(Z, S, mem, orc, [1, 2, 3], cts=cts)
    assert Z.query("rot_many_fallbacks") == 0
    cts[2, 1, 1, 517] = 0
    rm.check_rot_many(Z, S, mem, orc, [1, 2, 3], cts=cts)
    assert Z.query("rot_many_fallbacks") == 1
    Z.close()


# ---- N = 4096: the multi-child launch ----
def test_row_kernel_children_of_one_node(orc, api, lib, mem, S12):
    """15 children in one launch (B = 1 and 3), group and group + 1 children, one child, +k with -k"""
    X = _ctx(api, lib, S12, 1)
    group = X.query("rot_many_group")
    assert 16 <= group <= 16, "the fixture holds keys for 1 .. 17"
    cts = rm.encryptions(S12, 3, seed=150)
    refs = rm.oracle_rotations(S12, cts, list(range(1, group + 2)))
    rm.check_rot_many(X, S12, mem, orc, list(range(1, 16)), cts=cts, refs=refs[:15])
    assert X.query("rot_many_launches") == 1 and X.query("rot_many_key_switches") == 15
    rm.check_rot_many(X, S12, mem, orc, list(range(1, 16)), cts=cts[:1], refs=refs[:15, :1])
    rm.check_rot_many(X, S12, mem, orc, list(range(1, group + 1)), cts=cts[:1], refs=refs[:group, :1])
    assert X.query("rot_many_launches") == 1
    rm.check_rot_many(X, S12, mem, orc, list(range(1, group + 2)), cts=cts[:1], refs=refs[:, :1])
    assert X.query("rot_many_launches") == 2
    rm.check_rot_many(X, S12, mem, orc, [7], cts=cts[:2], refs=refs[6:7, :2])
    rm.check_rot_many(X, S12, mem, orc, [4, -4, 1, -1, 64, -64], cts=cts[:2])
    assert X.query("rot_many_fallbacks") == 0
    X.close()


def test_row_kernel_default_keys_depth_three(orc, api, lib, mem, S12):
    D = _default_only(orc, S12)
    X = _ctx(api, lib, D, 1)
    rm.check_rot_many(X, D, mem, orc, list(range(1, 16)), B=2)
    assert X.query("rot_many_launches") == 8 and X.query("rot_many_key_switches") == 20
    X.close()


def test_row_kernel_every_word_at_q_minus_one(orc, api, lib, mem, S12):
    S, O = S12, S12.O
    steps = list(range(1, 16))
    rng = np.random.default_rng(160)
    elts = [pc.galois_elt_py(S.n, s) for s in steps]
    keys = np.zeros((len(elts),) + O.ksk_shape, np.uint64)
    for J in range(O.K):
        keys[:, :, :, J, :] = rng.integers(0, S.q[J], keys[:, :, :, J, :].shape, dtype=np.uint64)
    gk = orc.GaloisKeys(elts, keys)
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    ks = X.keyset()
    for e, k in zip(elts, keys):
        ks.set_galois(int(e), k)
    cts = np.stack([pc.adversarial_words(S, 2, "max"), pc.adversarial_words(S, 2, "alt")])
    cts[1][cts[1] == 0] = 1
    got = rm.run_rot_many(X, mem, cts, steps, gk=ks)
    assert X.query("rot_many_fallbacks") == 0 and X.query("rot_many_launches") == 1
    for k, s in enumerate(steps):
        for b in range(2):
            assert (got[k, b] == O.rotate_rows(cts[b], s, gk)[0]).all(), (s, b)
    ks.close()
    X.close()


def test_row_kernel_transparent_item_knobs_and_chunks(orc, api, lib, mem, S12, monkeypatch):
    S, O = S12, S12.O
    rng = np.random.default_rng(9)
    cts = rm.encryptions(S, 3, seed=170)
    steps = [1, 2, 3, -5, 0, 16]
    X = _ctx(api, lib, S, 1)
    got, refs = rm.check_rot_many(X, S, mem, orc, steps, cts=cts)
    assert X.query("rot_many_fallbacks") == 0
    tr = cts.copy()
    tr[1, 1] = 0
    for j in range(O.L):
        tr[1, 0, j] = rng.integers(0, S.q[j], O.n, dtype=np.uint64)
    rm.check_rot_many(X, S, mem, orc, steps, cts=tr)
    assert X.query("rot_many_fallbacks") == 1
    X.close()
    for env in ({"HHE_ROT_HOIST": "2"}, {"HHE_ROT_HOIST": "0"}, {"HHE_CHUNK": "6", "HHE_STREAMS": "2"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        Y = _ctx(api, lib, S, 1)
        for k in env:
            monkeypatch.delenv(k)
        g2, _ = rm.check_rot_many(Y, S, mem, orc, steps, cts=cts, refs=refs)
        assert (g2 == got).all(), env
        Y.close()


@pytest.mark.parametrize("name", ["n1024", "row12"])
def test_against_the_integer_definition(orc, api, lib, mem, name):
    E, make_ctx = dc.setup(orc, api, lib, name)
    rm.check_against_integers(make_ctx, E, mem)


# ---- one case per row-pass size of the row kernel ----
@pytest.mark.parametrize("logn,limbs,row_pass", [(12, 3, 6), (13, 3, 7), (15, 4, 8)])
def test_every_row_pass_size(orc, api, lib, mem, logn, limbs, row_pass):
    """CoeffModulus::Create primes of 60 bits; steps [1, 2, 3, -5], own keys for 1 .. 3, -5 through its NAF terms"""
    n = 1 << logn
    assert logn - logn // 2 == row_pass   # ntt_split (csrc/hhe_launch.h): the row pass takes the larger half of logn
    S = rm.setup_with_steps(orc, logn, orc.coeff_modulus_create(n, [60] * limbs), [1, 2, 3, -1, -4])
    X = _ctx(api, lib, S, 1)
    rm.check_rot_many(X, S, mem, orc, [1, 2, 3, -5], B=2)
    assert X.query("rot_many_key_switches") == 5 and X.query("rot_many_launches") == 2
    X.close()


# ---- the layer ----
@pytest.mark.parametrize("rows,cols,rc,ks", fp.SHAPES)
def test_layer_own_keys(orc, api, lib, mem, rows, cols, rc, ks):
    S = rm.setup_with_steps(orc, 10, orc.coeff_modulus_create(1024, [50] * 3), rm.hand_hoisted_steps(1024, rows, cols), all_default=True)
    X = _ctx(api, lib, S, 0)
    rm.check_hoisted_layer(X, S, mem, orc, fp.seeded_matrix(T, rows, cols, 7 * rows + cols), B=2, seed=rows)
    X.close()


def test_layer_default_keys_in_place_and_fallback(orc, api, lib, mem, S10, monkeypatch):
    D = _default_only(orc, S10)
    X = _ctx(api, lib, D, 0)
    M = fp.seeded_matrix(T, 5, 256, 291)
    got, refs, _ = rm.check_hoisted_layer(X, D, mem, orc, M, B=3, seed=5)
    g2, _, _ = rm.check_hoisted_layer(X, D, mem, orc, M, B=3, seed=5, in_place=True, refs=refs, chain=False)
    assert (g2 == got).all()
    X.close()
    monkeypatch.setenv("HHE_ROT_HOIST", "2")
    monkeypatch.setenv("HHE_CHUNK", "16")   # r = 8: two items per chunk
    Y = _ctx(api, lib, D, 0)
    g3, _, _ = rm.check_hoisted_layer(Y, D, mem, orc, M, B=3, seed=5, in_place=True, refs=refs, chain=False)
    assert (g3 == got).all() and Y.query("rot_many_fallbacks") == 2
    Y.close()


def test_layer_mnist_shape_on_the_row_kernels(orc, api, lib, mem):
    S = rm.setup_with_steps(orc, 12, orc.coeff_modulus_create(4096, [60] * 3), rm.hand_hoisted_steps(4096, 10, 784))
    X = _ctx(api, lib, S, 1)
    rm.check_hoisted_layer(X, S, mem, orc, fp.seeded_matrix(T, 10, 784, 5), B=1, seed=6)
    X.close()


def test_layer_bfv_default_4096(orc, api, lib, mem):
    """BFVDefault(4096): the separate-kernel path at full tiles, 3 x 5 hoisted"""
    S = rm.setup_with_steps(orc, 12, api.bfv_default_coeff_modulus(4096, lib), rm.hand_hoisted_steps(4096, 3, 5))
    X = _ctx(api, lib, S, 0)
    rm.check_hoisted_layer(X, S, mem, orc, fp.seeded_matrix(T, 3, 5, 9), B=2, seed=1)
    X.close()


# ---- the deployed parameter set, keys for 1 .. 15 generated on the device ----
def _mnist(count):
    fx = json.load(open(os.path.join(HERE, "golden", "mnist_64.json")))
    W = np.array(json.load(open(os.path.join(HERE, "golden", "mnist_1fc.json")))["weights_rows"], dtype=np.int64)
    packed = np.array([list(bytes.fromhex(h)) for h in fx["pixels_2bit_hex"][:count]], dtype=np.uint8)
    pix = ((packed[:, :, None] >> (2 * np.arange(4))) & 3).reshape(count, 784).astype(np.int64)
    assert (pix @ W.T == np.array(fx["plain_logits"][:count])).all()
    return (W % T).astype(np.uint64), pix.astype(np.uint64), np.array(fx["plain_logits"][:count])


def test_deployed_parameters_device_keys(orc, api, lib, mem):
    """BFVDefault(16384), 10 x 784: one item word for word against the composition under the keys read back from the device; four MNIST
    images against plain integers and against the slots of hhe_fc_packed_ks; the device's noise budget is positive"""
    S = rm.setup_with_steps(orc, 14, api.bfv_default_coeff_modulus(1 << 14, lib), [-1024, 1, 16, 32, 64, 128, 256, 512])
    O = S.O
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    assert X.query("row_kernel") == 1
    ks = X.keyset().set_relin(S.rk)
    for e, k in zip(S.gk.elts, S.gk.keys):
        ks.set_galois(int(e), k)
    have = set(int(e) for e in S.gk.elts)
    new = [pc.galois_elt_py(S.n, s) for s in range(2, 16)]
    assert not have & set(new)
    ks.generate_galois(mem.to_dev(S.sk), bytes(range(32)), elts=new)
    S.gk = orc.GaloisKeys(list(S.gk.elts) + new, np.concatenate([S.gk.keys, np.stack([ks.get_galois(e) for e in new])]))
    NS = 4
    M, pix, plain = _mnist(NS)
    W = fp.encrypt_diagonals(S, M, seed=1200)
    cts = fp.encrypt_inputs(S, list(pix), seed=1100)
    mat = X.enc_matrix(mem.to_dev(W), 10, 784)
    d_x = mem.to_dev(cts)
    out = X.fc_packed_hoisted(d_x, mat, mem.empty((NS,) + O.ct_shape), NS, rk=ks, gk=ks)
    assert X.query("fc_packed_key_switches") == 22 and X.query("rot_many_launches") == 1 and X.query("rot_many_fallbacks") == 0
    assert (X.noise_budget(S.sk, out, NS) > 0).all()
    got = mem.to_host(out)
    assert (got[0] == rm.fc_packed_hoisted_ref(O, S.rk, S.gk, W, cts[0], 10, 784)).all()
    fp.check_slots(S, got[0], M, pix[0])
    vals = mem.empty((NS, O.n))
    X.decrypt(S.sk, out, NS, vals)
    logits = mem.to_host(vals)[:, :10].astype(np.int64)
    assert (logits == plain % T).all()
    chain = mat.apply(d_x, NS, rk=ks, gk=ks, out=mem.empty((NS,) + O.ct_shape))
    assert (X.noise_budget(S.sk, chain, NS) > 0).all()
    X.decrypt(S.sk, chain, NS, vals)
    assert (mem.to_host(vals)[:, :10].astype(np.int64) == logits).all()
    assert not (mem.to_host(chain) == got).all()   # other words: the noise differs
    mat.destroy()
    ks.close()
    X.close()
