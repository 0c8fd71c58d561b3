"""One keystream per block counter on the emulator (the shared kernel bodies behind the real host driver): a transciphering call
in which counters repeat evaluates each distinct counter once (phase 1, into the keystream table) and finishes every item with one
encode + add_plain that reads its counter's slot (phase 2, AddPlainArgs::ct_map).  See dedup_common for what every check asserts."""
import numpy as np
import pytest

from conftest import Setup
import dedup_common as dc
import parity_common as pc
import plain_modulus_common as pm


@pytest.fixture(scope="module")
def mem():
    return pc.HostMem()


def test_mixed_duplicates_ragged_lengths(orc, api, emu_lib, mem, small, monkeypatch):
    """non-adjacent duplicates, and different lengths inside one group: the keystream is common, the encoded words are not"""
    ids, ncw = [0, 0, 3, 0, 3], [128, 17, 128, 1, 60]
    dc.check_dedup(api, emu_lib, small, orc, mem, monkeypatch, dc.words(small, 5, 1), ncw, ids, unique=2, oracle_items=[1, 3, 4])


def test_one_group_with_the_shared_first_layer(orc, api, emu_lib, mem, small, monkeypatch):
    """HHE_SHARED_L0 counts evaluations: its chain runs for the one counter and leaves the sums in the keystream table (`out`
    belongs to the finishing pass)"""
    X1, X0, _ = dc.check_dedup(api, emu_lib, small, orc, mem, monkeypatch, dc.words(small, 3, 2), [128, 40, 128], [5, 5, 5],
                               unique=1, oracle_items=[1], HHE_SHARED_L0=1)
    assert X1.query("shared_l0_steps") == 128 and X0.query("shared_l0_steps") == 128


@pytest.mark.parametrize("streams", [2, 0])
def test_both_phases_chunked(orc, api, emu_lib, mem, small, monkeypatch, streams):
    """3 evaluations in 2 chunks, 7 items in 4: the last item reads a slot that another lane wrote.  streams = 0: everything on the
    caller's stream, one chunk per phase"""
    ids, ncw = [0, 1, 0, 2, 1, 2, 0], [128, 128, 3, 128, 77, 128, 128]
    dc.check_dedup(api, emu_lib, small, orc, mem, monkeypatch, dc.words(small, 7, 3), ncw, ids, unique=3, oracle_items=[4, 6],
                   HHE_STREAMS=streams, HHE_CHUNK=2)


def test_all_distinct_runs_per_item(orc, api, emu_lib, mem, small, monkeypatch):
    dc.check_dedup(api, emu_lib, small, orc, mem, monkeypatch, dc.words(small, 3, 4), [128, 128, 9], [0, 1, 2], unique=3, oracle_items=[2])


def test_bsgs(orc, api, emu_lib, mem, monkeypatch):
    S, _ = pm.hot_setup(orc, api, emu_lib, "t33_60x3")
    dc.check_dedup(api, emu_lib, S, orc, mem, monkeypatch, dc.words(S, 3, 5), [128, 128, 12], [0, 1, 0], unique=2, oracle_items=[2],
                   use_bsgs=True)


def test_context_with_the_row_kernel(orc, api, emu_lib, mem, monkeypatch):
    S = Setup(orc, 12, [50, 50, 50])
    X1, _, _ = dc.check_dedup(api, emu_lib, S, orc, mem, monkeypatch, dc.words(S, 2, 6), [128, 40], [3, 3], unique=1, oracle_items=[1])
    assert X1.query("row_kernel") == 1


def test_decompose_of_three_records(orc, api, emu_lib, mem, monkeypatch):
    """hhe_decompose numbers the blocks of every record from 0: 9 items, 3 counters"""
    S = Setup(orc, 10, [50] * 9, extra_steps=(-128, -256))
    O = S.O
    pts = [np.array([(7 * i + 3 + 11 * s) % 256 for i in range(300)], dtype=np.uint64) for s in range(3)]
    recs = np.stack([orc.pasta_encrypt(S.t, S.key, p) for p in pts])
    res = {}
    for knob in (1, 0):
        X = dc.make_ctx(api, emu_lib, S, monkeypatch, HHE_DEDUP=knob)
        out = mem.empty((3,) + O.ct_shape)
        X.decompose(mem.to_dev(S.enc_key), recs, out, mask_last=True)
        res[knob] = mem.to_host(out)
        assert X.query("transcipher_unique") == (3 if knob else 9)
    assert (res[1] == res[0]).all()
    cw, ncw = S.sym_blocks(orc, pts[1])
    blocks = [O.transcipher_block(S.enc_key, S.rk, S.gk, cw[b, :ncw[b]], b) for b in range(3)]
    blocks[2] = O.mask(blocks[2], np.ones(44, np.uint64))
    assert (res[1][1] == O.flatten(np.stack(blocks), S.gk)).all()
    assert (O.decode(O.decrypt(S.sk, res[1][1]))[:300] == pts[1]).all()


def test_key_change_between_calls_reuses_nothing(orc, api, emu_lib, mem, small, monkeypatch):
    """the keystream table is a workspace of one call: the same counters under another key ciphertext give what a fresh context gives"""
    O = small.O
    enc2 = O.encrypt(small.pk, O.pasta_pack_key((small.key * 3 + 1) % small.t), 12)
    cw, ncw, ids = dc.words(small, 3, 7), [128, 128, 50], [0, 0, 1]
    X = dc.make_ctx(api, emu_lib, small, monkeypatch)
    assert X.query("dedup") == 1  # the default
    ra = dc.run(X, small, mem, cw, ncw, ids)
    rb = dc.run(X, small, mem, cw, ncw, ids, enc_key=enc2)
    assert X.query("transcipher_unique") == 2
    fresh = dc.run(dc.make_ctx(api, emu_lib, small, monkeypatch), small, mem, cw, ncw, ids, enc_key=enc2)
    assert (rb == fresh).all() and not (ra == rb).all()
    assert (rb[1] == dc.oracle_block(small, cw, ncw, ids, 1, enc_key=enc2)).all()
    assert (ra[1] == dc.oracle_block(small, cw, ncw, ids, 1)).all()
