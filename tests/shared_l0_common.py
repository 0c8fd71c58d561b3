"""The shared first layer of the fused diagonal matmul (HHE_SHARED_L0, DESIGN.md "Fused diagonal matmul"): what
tests/test_shared_first_layer.py (emulator and GPU) and tests/test_stream_order_emu.py share.  Every check is exact equality of
ciphertext words: knob 1 (the rotation chain of layer 0 runs once per call) against knob 0 (per item), and named items against the
oracle's transcipher_block."""
import numpy as np


def make_ctx(api, lib, S, monkeypatch, **env):
    """a context created under the given knobs (they are read at creation), keys loaded"""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    X = api.Context(S.logn, S.q, S.t, lib=lib)
    for k in env:
        monkeypatch.delenv(k)
    S.load_keys(X)
    return X


def run(X, S, mem, cw, ncw, ids, enc_key=None):
    out = mem.empty((len(ids),) + S.O.ct_shape)
    X.transcipher(mem.to_dev(S.enc_key if enc_key is None else enc_key), cw, ncw, ids, out)
    return mem.to_host(out)


def oracle_blocks(S, cw, ncw, ids, items=None, enc_key=None):
    enc_key = S.enc_key if enc_key is None else enc_key
    return {b: S.O.transcipher_block(enc_key, S.rk, S.gk, cw[b, :ncw[b]], ids[b]) for b in (range(len(ids)) if items is None else items)}


def blocks_of(S, orc, nwords, seed=3):
    pt = np.array([(seed * i + 1) % 256 for i in range(nwords)], dtype=np.uint64)
    return S.sym_blocks(orc, pt)


def check_knob(api, lib, S, orc, mem, monkeypatch, cw, ncw, ids, oracle_items=None, **env):
    """knob 1 == knob 0 word for word, and the chosen items == the oracle"""
    X1 = make_ctx(api, lib, S, monkeypatch, HHE_SHARED_L0=1, **env)
    X0 = make_ctx(api, lib, S, monkeypatch, HHE_SHARED_L0=0, **env)
    assert X1.query("shared_l0") == 1 and X0.query("shared_l0") == 0
    r1, r0 = run(X1, S, mem, cw, ncw, ids), run(X0, S, mem, cw, ncw, ids)
    assert X0.query("shared_l0_steps") == 0  # the per-item path never builds the operand table
    assert (r1 == r0).all()
    for b, ref in oracle_blocks(S, cw, ncw, ids, oracle_items).items():
        assert (r1[b] == ref).all(), f"item {b} differs from the oracle"
    return X1, X0, r1
