"""GPU parity on the paths that the prime sets of the other GPU tests never select, and on the folds of the row kernels at
their bounds.  Which kernels a context runs is decided by the form of its coefficient primes (hhe_ctx_query "row_kernel",
"pm_ok", "digit_reduce"; DESIGN.md section 2, dispatch matrix): every test here asserts the path it means to run before it
compares words, and every comparison is exact equality with the CPU oracle.  Run on an MI355X: python -m pytest tests -m gpu."""
import numpy as np
import pytest

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


def test_row_kernel_query_coincides_with_row_kernel_launches(orc, api, lib, mem):
    """hhe_ctx_query("row_kernel") is the dispatch itself, not a restatement of it: with 1 the matmul loop launches
    ks_row_kernel (counted by hhe_ctx_profile_read), with 0 -- BFVDefault(4096), same degree -- it launches none"""
    for name, launched in (("H", True), ("A", False)):
        S, make_ctx = pc.dispatch_setup(orc, api, lib, name, all_galois=False, extra_steps=())
        X = make_ctx()
        S.load_keys(X)
        X.profile(True)
        cw = np.full((1, 128), 5, np.uint64)
        out = mem.empty((1,) + S.O.ct_shape)
        X.transcipher(mem.to_dev(S.enc_key), cw, [128], [0], out)
        kname, launches, _, items = X.profile_read()
        assert (launches > 0) == launched and X.query("row_kernel") == int(launched), (name, kname, launches, items)
        assert (mem.to_host(out)[0] == S.O.transcipher_block(S.enc_key, S.rk, S.gk, cw[0], 0)).all()
        X.close()


@pytest.mark.parametrize("name,n_in", [("A", 21), ("B", 9), ("C", 5), ("E", 21), ("F", 9), ("F2", 9), ("G", 21)])
def test_fallback_path_at_full_tiles(orc, api, lib, mem, monkeypatch, name, n_in):
    """N >= 4096 WITHOUT the fused row kernel (a coefficient prime lacks the pseudo-Mersenne form): step_separate in the matmul
    loop, k_ntt / ks_mac / ks_finish in every generic key switch, galois_kernel in rotations, the ks_mac branch of the FC -- on
    the full-tile geometry, with Harvey's butterflies on the coefficient primes.  Case A is the reference's own N = 4096
    parameter set."""
    S, make_ctx = pc.dispatch_setup(orc, api, lib, name)
    X = make_ctx()
    S.load_keys(X)
    pc.check_hot_path(X, S, orc, mem, make_ctx, monkeypatch, n_in=n_in, seed=ord(name[0]))
    X.close()


def test_reference_flow_at_bfv_default_4096(orc, api, lib, mem):
    """the reference-shaped flow at SEALZpCipher::create_context(4096)'s parameters: client PASTA encryption on the device,
    BaseCSP::decompose for two records (blocks -> mask -> flatten), every word against the oracle's op sequence.  109 bits of
    modulus leave no noise budget for PASTA-3: words are compared, not decryptions."""
    S, make_ctx = pc.dispatch_setup(orc, api, lib, "A", all_galois=False)
    O = S.O
    X = make_ctx()
    S.load_keys(X)
    pts = np.stack([np.array([(7 * i + 3 + s) % 256 for i in range(300)], dtype=np.uint64) for s in range(2)])
    d_sym = mem.empty((2, 300))
    X.plain_crypt(S.key, mem.to_dev(pts), 2, 300, d_sym)
    recs = mem.to_host(d_sym)
    out = mem.empty((2,) + O.ct_shape)
    X.decompose(mem.to_dev(S.enc_key), recs, out, mask_last=True)
    res = mem.to_host(out)
    for s in range(2):
        assert (recs[s] == orc.pasta_encrypt(S.t, S.key, pts[s])).all()
        cw, ncw = S.sym_blocks(orc, pts[s])
        blocks = [O.transcipher_block(S.enc_key, S.rk, S.gk, cw[b, :ncw[b]], b) for b in range(3)]
        blocks[2] = O.mask(blocks[2], np.ones(44, np.uint64))
        assert (res[s] == O.flatten(np.stack(blocks), S.gk)).all()


def test_fallback_path_n65536(orc, api, lib, mem):
    """case D: N = 2^16, 3 x 40-bit primes (none pm_ok), t = 8088322049 -- transforms, every op, and a chain of four
    rotate_rows(-1) in place through galois_kernel + the separate key-switch kernels"""
    S, make_ctx = pc.dispatch_setup(orc, api, lib, "D", all_galois=False, extra_steps=())
    O = S.O
    X = make_ctx()
    S.load_keys(X)
    pc.check_context_constants(X, O)
    pc.check_ntt(X, O, mem, seed=16)
    pc.check_ops(X, S, mem, B=2, seed=16)
    rng = np.random.default_rng(16)
    ct = O.encrypt(S.pk, O.encode(rng.integers(0, 1 << 30, O.n)), 40)
    d, ref = mem.to_dev(ct[None]), ct
    for _ in range(4):
        X.rotate_rows(d, -1, d, 1)
        ref = O.rotate_rows(ref, -1, S.gk)[0]
    assert (mem.to_host(d)[0] == ref).all()


@pytest.mark.parametrize("name,n_in", [("H", 21), ("I", 5)])
def test_row_kernel_at_the_largest_admitted_c(orc, api, lib, mem, monkeypatch, name, n_in):
    """pm_fold leaves any 64-bit value below 2q as long as 2^b + 2^(64-b) c <= 2q: the bound is tightest for the largest c.
    Primes with the largest c = 2^b - q the predicate admits (and q = 1 mod 2N) through the whole hot path on the row kernels,
    then worst-case residues through the matmul loop and the generic key switches."""
    S, make_ctx = pc.dispatch_setup(orc, api, lib, name)
    X = make_ctx()
    S.load_keys(X)
    pc.check_hot_path(X, S, orc, mem, make_ctx, monkeypatch, n_in=n_in, seed=ord(name))
    for pattern in ("max", "alt", "max_keys"):
        pc.check_matmul_adversarial(X, S, orc, mem, pattern)
        pc.check_keyswitch_adversarial(X, S, orc, mem, pattern)
    X.close()


@pytest.mark.parametrize("pattern", ["max", "alt", "max_keys"])
@pytest.mark.parametrize("logn,K", [(12, 5), (12, 8), (15, 5)])
def test_row_kernel_folds_at_60_bits(orc, api, lib, mem, logn, K, pattern):
    """The lazy sums of ks_row_kernel / ks_perm_row_kernel are folded after every third digit (hhe_kernel_bodies.h,
    ks_row_mac_phase / ks_row_mac_gather); at 60-bit primes 14q is just under 2^64.  L = 4: one fold, then one more digit;
    L = 7: two folds and a last digit that the flush folds; N = 2^15: the same on 256-point rows.  Every ciphertext, plaintext
    and -- 'max_keys' -- key word at q_j - 1, through the matmul loop, rotations, multiply, relinearize and one FC row.
    What these cases can and cannot tell: up to L = 7 a fold after every FOURTH digit would be just as safe (four products below
    4q: under 16q < 2^64; then 2q + 3 x 4q = 14q), so they pin the words and the absence of wraps on the fold code, not its period."""
    from conftest import Setup
    S = Setup(orc, logn, [60] * K, all_galois=True)
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    pc.assert_dispatch(X, S.q, 1, 0)
    pc.check_matmul_adversarial(X, S, orc, mem, pattern)
    pc.check_keyswitch_adversarial(X, S, orc, mem, pattern)
    X.close()


def test_reference_n65536_chain_key_switches(orc, api, lib, mem):
    """the reference's hard-coded N = 65536 chain (hhe_bfv_default_coeff_modulus(65536): 29 primes, L = 28, t = 8088322049),
    B = 1: rotate_rows(-1), multiply and relinearize against the oracle -- nine folds per lazy sum of the row kernel, the deepest
    BEHZ conversions.  One Galois key and the relinearization key only (0.85 GB each, plus their Shoup tables on the device)."""
    q = api.bfv_default_coeff_modulus(65536, lib)
    assert len(q) == 29
    S = pc.setup_from_primes(orc, 16, q, pc.T33, base_steps=(-1,))
    O = S.O
    X = api.Context(16, q, pc.T33, lib=lib)
    pc.assert_dispatch(X, q, 1)
    S.load_keys(X)
    rng = np.random.default_rng(65536)
    ct = O.encrypt(S.pk, O.encode(rng.integers(0, 1 << 30, O.n)), 40)
    d, out = mem.to_dev(ct[None]), mem.empty((1,) + O.ct_shape)
    X.rotate_rows(d, -1, out, 1)
    rot = O.rotate_rows(ct, -1, S.gk)[0]
    assert (mem.to_host(out)[0] == rot).all()
    o3 = mem.empty((1, 3, O.L, O.n))
    X.multiply(out, d, o3, 1)
    ref3 = O.multiply(rot, ct)
    assert (mem.to_host(o3)[0] == ref3).all()
    X.relinearize(o3, out, 1)
    assert (mem.to_host(out)[0] == O.relinearize(ref3, S.rk)).all()
    X.close()
