"""The host driver's stream schedule under the lazy order of the emulator (tests/emu/emu_order.cpp, HHE_EMU_ORDER=lazy): enqueued work
runs only when something forces its stream, and a force runs nothing the schedule did not order before it.  A missing event wait, a
chunk on the wrong lane, staging rewritten before its copy ran or a result read before the final wait then changes ciphertext words,
deterministically, without a GPU.  tests/test_cpp_stream_order.py pins the model itself.

Every test here re-runs checkers the suite already has -- the shared *_common helpers, or the body of an emulator test -- with every
context created and driven under the lazy order.  The comparisons are theirs: exact equality of ciphertext words with the oracle, and
with a second context that takes another path.  Memory is numpy's (kept alive to the end of the test); its `to_host` does not wait for anything, so a synchronous
entry point whose result is not there on return fails, and `SyncedMem` waits for the whole device where a checker reads the result of
the asynchronous generic ops (as TorchMem does on the GPU).  Each test ends by asserting that work really was deferred and forced:
a run in which the lazy order did not engage has tested nothing.

Shapes: N = 1024 over 3 x 50 bits (L = 2) and N = 2048 over 4 x 60 bits (L = 3), what the emulator suites use; N = 4096 over 3 x 60
bits once, for the row kernels of the hoisted rotations, and N = 1024 over 4 x 18 bits once, where a residue of c1 can be set to 0."""
import contextlib
import ctypes

import numpy as np
import pytest

import affine_common as ac
import dedup_common as dc
import fc_packed_common as fp
import fused_finish_common as ff
import keygen_common as kg
import kscache_common as kc
import mlp_common as mc
import mod_switch_common as ms
import mult_sum_common as msc
import parity_common as pc
import rot_many_common as rm
import shared_l0_common as tsl
from conftest import Setup


def order_stats(lib):
    """(operations deferred, operations run at force points, most pending at once since the last emu_order_window, forces)"""
    out = (ctypes.c_uint64 * 4)()
    lib.emu_order_stats.argtypes, lib.emu_order_stats.restype = [ctypes.POINTER(ctypes.c_uint64)], None
    lib.emu_order_stats(out)
    return tuple(int(v) for v in out)


def device_sync(lib):
    lib.emu_device_sync.argtypes, lib.emu_device_sync.restype = [], None
    lib.emu_device_sync()


class KeptMem(pc.HostMem):
    """numpy memory that keeps every buffer it handed out alive.  Under the lazy order work that a broken schedule left pending runs
    after its call has returned -- at the next free, or when the context goes; it must then find the call's buffers, so that what the
    test sees is its own failed comparison of words and not a read of released memory"""

    def __init__(self):
        self.kept = []

    def to_dev(self, a):
        self.kept.append(super().to_dev(a))
        return self.kept[-1]

    def empty(self, shape):
        self.kept.append(super().empty(shape))
        return self.kept[-1]


class SyncedMem(KeptMem):
    """... whose read-back waits for the whole device first, like TorchMem.to_host: for checkers that read what the asynchronous
    generic ops (rotate, multiply, encrypt ...) wrote"""

    def __init__(self, lib):
        super().__init__()
        self.lib = lib

    def to_host(self, b):
        device_sync(self.lib)
        return super().to_host(b)


@contextlib.contextmanager
def lazy_order(lib, monkeypatch, min_pending=8):
    """everything inside runs under HHE_EMU_ORDER=lazy; on the way out: work was deferred, forced, and at least min_pending operations
    were pending at once (a schedule that synchronised after every launch would hide what these tests look for)"""
    device_sync(lib)  # nothing pending: the order is read at the next operation
    lib.emu_order_window.argtypes, lib.emu_order_window.restype = [], None
    lib.emu_order_window()  # the largest number pending at once is this block's own
    s0 = order_stats(lib)
    monkeypatch.setenv("HHE_EMU_ORDER", "lazy")
    try:
        yield
    finally:
        device_sync(lib)
        monkeypatch.delenv("HHE_EMU_ORDER")
    s1 = order_stats(lib)
    assert s1[0] > s0[0] and s1[3] > s0[3], "nothing was deferred: the lazy order did not engage"
    assert s1[1] - s0[1] == s1[0] - s0[0], "deferred operations that never ran"
    assert s1[2] >= min_pending


@pytest.fixture
def mem():
    return KeptMem()


@pytest.fixture(scope="module")
def ragged(orc):
    """N = 1024, L = 2 (fused_finish_common's smallest shape), with the keys of the babystep-giantstep variant"""
    return Setup(orc, 10, [50] * 3, extra_steps=ff.BSGS_STEPS)


@pytest.fixture(scope="module")
def n2048(orc):
    """N = 2048, L = 3: the set-up of tests/test_scheduler.py"""
    return Setup(orc, 11, [60] * 4, all_galois=True, extra_steps=[-16 * k for k in range(1, 8)] + ac.hand_steps(2048, 16, 4, 4))


def test_eager_is_the_default_and_defers_nothing(orc, api, emu_lib, mem, ragged, monkeypatch):
    monkeypatch.delenv("HHE_EMU_ORDER", raising=False)
    device_sync(emu_lib)
    s0 = order_stats(emu_lib)
    X = dc.make_ctx(api, emu_lib, ragged, monkeypatch)
    kc.run(X, ragged, mem, kc.words(ragged, 1, 1), [5], [0])
    X.close()
    assert order_stats(emu_lib) == s0


def test_lazy_context_equals_eager_context_and_both_orders_share_one_library(orc, api, emu_lib, mem, ragged, monkeypatch):
    S, cw, ncw, ids = ragged, kc.words(ragged, 3, 2), [128, 7, 0], [0, 1, 0]
    Xe = dc.make_ctx(api, emu_lib, S, monkeypatch, **ff.CHUNKED)
    r_eager = kc.run(Xe, S, mem, cw, ncw, ids)
    with lazy_order(emu_lib, monkeypatch):
        Xl = dc.make_ctx(api, emu_lib, S, monkeypatch, **ff.CHUNKED)
        r_lazy = kc.run(Xl, S, mem, cw, ncw, ids)
        r_kept = kc.run(Xl, S, mem, cw, ncw, ids)
        assert kc.counts(Xl) == (0, 2)
        Xl.close()
    assert (r_lazy == r_eager).all() and (r_kept == r_eager).all()
    assert (r_lazy[1] == dc.oracle_block(S, cw, ncw, ids, 1)).all()
    assert (kc.run(Xe, S, mem, cw, ncw, ids) == r_eager).all()  # the eager context goes on as before
    Xe.close()


def test_chunk_scheduler_small_large_small(orc, api, emu_lib, mem, n2048, monkeypatch):
    """transciphering (BSGS), the packed affine layer and the FC row on two lanes, two items per chunk, every workspace regrown after
    the lanes were used: the fork, the per-lane joins and the waits in front of every regrowth"""
    for k in ("HHE_STREAMS", "HHE_CHUNK", "HHE_FC_CHUNK"):
        monkeypatch.setenv(k, "2")
    S = n2048
    with lazy_order(emu_lib, monkeypatch):
        pc.check_batched_calls_regrow(lambda: api.Context(S.logn, S.q, S.t, lib=emu_lib), S, orc, mem)


def test_packed_affine_diagonal_method(orc, api, emu_lib, mem, n2048, monkeypatch):
    """the diagonal method of the affine layer (check_batched_calls_regrow runs the babystep-giantstep handle), chunked on two lanes"""
    S, O, dim, B = n2048, n2048.O, 16, 5
    M, bias = ac.seeded_matrix(S.t, dim, 78)
    cts, _ = ac.inputs(S, dim, B, 8)
    for k in ("HHE_STREAMS", "HHE_CHUNK"):
        monkeypatch.setenv(k, "2")
    with lazy_order(emu_lib, monkeypatch):
        X = api.Context(S.logn, S.q, S.t, lib=emu_lib)
        S.load_keys(X)
        mat = X.matrix(M, bias=bias)
        out = mem.empty((B,) + O.ct_shape)
        X.packed_affine(mem.to_dev(cts), mat, out, B)
        got = mem.to_host(out)
        mat.close(), X.close()
    for b in (0, B - 1):
        assert (got[b] == ac.packed_affine_ref(O, S.gk, M, cts[b], bias, None)).all(), b


def item_kernel(monkeypatch, asserted):
    """HHE_FIN_ITEM=1 for every context of the test; asserted: every comparison of ff.same checks which path its contexts took"""
    monkeypatch.setenv("HHE_FIN_ITEM", "1")
    if not asserted:
        return
    plain_same = ff.same

    def same(S, mem, X1, X0, *args, **kw):
        assert X1.query("fin_item") == 1 and X0.query("fin_item") == 0
        before = X1.query("fin_item_launches")
        r = plain_same(S, mem, X1, X0, *args, **kw)
        assert X1.query("fin_item_launches") > before and X0.query("fin_item_launches") == 0
        return r

    monkeypatch.setattr(ff, "same", same)


FINISH_CHECKS = ["check_chunks_and_hits", "check_grow_and_shrink", "check_chunk_tail", "check_bsgs"]


def _finish(name, api, emu_lib, mem, S, monkeypatch):
    for k, v in ff.CHUNKED.items():  # for the checkers that do not set them themselves; make_ctx removes what it was given
        monkeypatch.setenv(k, str(v))
    with lazy_order(emu_lib, monkeypatch):
        getattr(ff, name)(api, emu_lib, S, mem, monkeypatch)


@pytest.mark.parametrize("name", FINISH_CHECKS)
def test_fused_finish_chunked(orc, api, emu_lib, mem, ragged, monkeypatch, name):
    _finish(name, api, emu_lib, mem, ragged, monkeypatch)


@pytest.mark.parametrize("name", FINISH_CHECKS)
def test_fused_finish_chunked_item_kernel(orc, api, emu_lib, mem, ragged, monkeypatch, name):
    item_kernel(monkeypatch, asserted=name != "check_chunk_tail")  # the calls without a keystream table never take the item kernel
    _finish(name, api, emu_lib, mem, ragged, monkeypatch)


@pytest.mark.parametrize("in_place", [False, True])
def test_prediction_sequence(orc, api, emu_lib, mem, ragged, monkeypatch, in_place):
    """key A twice, B, A again with the item kernel enqueued on a prediction before the comparison's event is waited for
    (tests/test_gpu_fin_item.py::test_gpu_prediction); in_place: enc_key overwritten in the same buffer between the calls"""
    monkeypatch.setenv("HHE_FIN_ITEM", "1")
    with lazy_order(emu_lib, monkeypatch):
        ff.check_prediction(api, emu_lib, ragged, mem, monkeypatch, in_place=in_place)


@pytest.mark.parametrize("name", ["check_budget_of_two_entries", "check_goes_with_the_block_tables_and_clearing", "check_key_replaced_or_added",
                                  "check_two_key_sets_and_a_destroyed_one", "check_enc_key_overwritten_in_place"])
def test_keystream_cache(orc, api, emu_lib, mem, ragged, monkeypatch, name):
    """the checkers behind tests/test_ks_cache.py (kscache_common) at L = 2: eviction by HHE_KS_CACHE_MB, by the block-table limit and by the snapshot limit,
    a key of the default set and of a named set replaced between calls, hhe_pasta3_clear_keystream_cache between calls"""
    with lazy_order(emu_lib, monkeypatch):
        getattr(kc, name)(orc, api, emu_lib, mem, ragged, monkeypatch)


def test_block_tables_evicted_while_a_call_runs(orc, api, emu_lib, mem, ragged, monkeypatch):
    """a block-table limit of one counter's tables: every call of a new counter evicts inside ensure_block, behind sync_ctx, while the
    kept keystream of the evicted counter goes with it; three counters in one call are served above the limit"""
    S, cw = ragged, kc.words(ragged, 3, 21)
    with lazy_order(emu_lib, monkeypatch):
        X = kc.ctx_on(api, emu_lib, S, monkeypatch)
        r0 = kc.run(X, S, mem, cw[:1], [128], [0])
        X.set_block_cache_limit(X.query("block_cache_bytes"))
        r1 = kc.run(X, S, mem, cw[1:2], [77], [1])
        assert X.query("block_cache_entries") == 1 and X.query("ks_cache_entries") == 1
        assert (kc.run(X, S, mem, cw[:1], [128], [0]) == r0).all() and kc.counts(X) == (1, 0)
        r3 = kc.run(X, S, mem, cw, [128, 77, 3], [0, 1, 2])
        assert X.query("block_cache_entries") == 3 and kc.counts(X) == (2, 1)
        X.close()
    assert (r3[0] == r0[0]).all() and (r3[1] == r1[0]).all()
    for b in (1, 2):
        assert (r3[b] == dc.oracle_block(S, cw, [128, 77, 3], [0, 1, 2], b)).all(), b


def test_shared_first_layer(orc, api, emu_lib, mem, ragged, monkeypatch):
    """tests/test_shared_first_layer.py's checker: the chain once on lane 0 before the chunks fork, several lanes reading its table,
    and the chain in blocks of two steps (the smallest operand table)"""
    S = ragged
    with lazy_order(emu_lib, monkeypatch):
        cw, ncw = tsl.blocks_of(S, orc, 5 * 128 - 3, seed=7)
        tsl.check_knob(api, emu_lib, S, orc, mem, monkeypatch, cw, ncw, [0, 1, 2, 3, 4], oracle_items=[2, 4], HHE_STREAMS=2, HHE_CHUNK=2)
        cw, ncw = tsl.blocks_of(S, orc, 2 * 128 + 5, seed=11)
        X1, _, _ = tsl.check_knob(api, emu_lib, S, orc, mem, monkeypatch, cw, ncw, [0, 1, 2], oracle_items=[2], HHE_SHARED_L0_MB=0.0)
        assert X1.query("shared_l0_steps") == 2
        tsl.check_knob(api, emu_lib, S, orc, mem, monkeypatch, cw[:2], ncw[:2], [0, 1], oracle_items=[1], HHE_STREAMS=0)


def test_decompose_with_masking(orc, api, emu_lib, mem, monkeypatch):
    """hhe_decompose of two records of three blocks, the last one masked, twice on one context, against the oracle's op sequence.  The
    mask values are staged in a pageable host vector, whose bytes the upload takes at the call: the wait in stage_begin is not what
    this test pins ("Stream order": the edge table says why nothing can)"""
    S = Setup(orc, 10, [50] * 3, extra_steps=(-128, -256))
    O, nwords = S.O, 300
    pts = [np.array([(7 * i + 3 + s) % 256 for i in range(nwords)], dtype=np.uint64) for s in range(2)]
    recs = np.stack([orc.pasta_encrypt(S.t, S.key, pt) for pt in pts])
    with lazy_order(emu_lib, monkeypatch):
        X = dc.make_ctx(api, emu_lib, S, monkeypatch)
        out = mem.empty((2,) + O.ct_shape)
        X.decompose(mem.to_dev(S.enc_key), recs, out, mask_last=True)
        first = mem.to_host(out)
        X.decompose(mem.to_dev(S.enc_key), recs[::-1].copy(), out, mask_last=True)  # the lane's staging is written a second time
        second = mem.to_host(out)
        X.close()
    assert (first == second[::-1]).all()
    for s in range(2):
        cw, ncw = S.sym_blocks(orc, pts[s])
        blocks = [O.transcipher_block(S.enc_key, S.rk, S.gk, cw[b, :ncw[b]], b) for b in range(3)]
        blocks[2] = O.mask(blocks[2], np.ones(nwords - 256, np.uint64))
        assert (first[s] == O.flatten(np.stack(blocks), S.gk)).all(), s


def test_mask_twice_without_a_wait_in_between(orc, api, emu_lib, ragged, monkeypatch):
    """hhe_mask only enqueues: two calls with different values and no wait in between, read after one hhe_ctx_sync, give the oracle's
    two products -- each upload took the bytes of the lane's (pageable) staging vector at its call, and the kernels ran in stream
    order at the sync"""
    S, O = ragged, ragged.O
    ct = O.encrypt(S.pk, O.encode(np.arange(S.n, dtype=np.uint64) % S.t), 31)
    m1, m2 = np.ones(40, np.uint64), np.array([(3 * i + 2) % S.t for i in range(90)], dtype=np.uint64)
    mem = KeptMem()
    with lazy_order(emu_lib, monkeypatch, min_pending=4):
        X = dc.make_ctx(api, emu_lib, S, monkeypatch)
        d_ct, o1, o2 = mem.to_dev(ct[None]), mem.empty((1,) + O.ct_shape), mem.empty((1,) + O.ct_shape)
        X.mask(d_ct, m1, o1, 1)
        X.mask(d_ct, m2, o2, 1)
        X.sync()
        r1, r2 = mem.to_host(o1), mem.to_host(o2)
        X.close()
    assert (r1[0] == O.mask(ct, m1)).all() and (r2[0] == O.mask(ct, m2)).all()


def test_mod_switch_then_decrypt_level(orc, api, emu_lib, monkeypatch):
    logn, bits, t, levels = ms.MEANING["n1024_4x50_t16"]
    q = orc.coeff_modulus_create(1 << logn, bits)
    with lazy_order(emu_lib, monkeypatch, min_pending=1):
        X, O = api.Context(logn, q, t, lib=emu_lib), orc.Oracle(logn, q, t)
        ms.check_meaning(X, O, orc, SyncedMem(emu_lib), levels)
        X.close()


def test_generated_keys_then_calls_under_them(orc, api, emu_lib, monkeypatch):
    """device key generation, then rotations, a multiplication and a transciphering under the generated sets (keygen_common)"""
    monkeypatch.setenv("HHE_KS_CACHE", "1")
    with lazy_order(emu_lib, monkeypatch):
        q = orc.coeff_modulus_create(2048, [50] * 3)
        X, O = api.Context(11, q, 65537, lib=emu_lib), orc.Oracle(11, q, 65537)
        kg.check_keys_behave(X, O, orc, SyncedMem(emu_lib))
        X.close()
        q = orc.coeff_modulus_create(1024, [50] * 3)
        X, O = api.Context(10, q, 65537, lib=emu_lib), orc.Oracle(10, q, 65537)
        kg.check_regeneration_drops_keystreams(X, O, orc, SyncedMem(emu_lib))
        X.close()


# ---- the calls that run their chunks optimistically, read one flag per chunk back and recompute the flagged ones on the main lane ----
ROT_MIXED = [1, -1, 3, 5, -5, 7, 100, -100, 511, -511, 0]   # tests/test_rot_many_emu.py's MIXED


def _q1024(orc):
    return orc.coeff_modulus_create(1024, [50] * 3)


@pytest.fixture(scope="module")
def rot10(orc):
    """N = 1024, L = 2: every default Galois key and a key for step 3 (tests/test_rot_many_emu.py's S10three)"""
    return rm.setup_with_steps(orc, 10, _q1024(orc), [3], all_default=True)


@pytest.fixture(scope="module")
def rot12(orc):
    """N = 4096, 3 x 60 bits (the row kernels): every default key and a key for each of 1 .. 17"""
    return rm.setup_with_steps(orc, 12, orc.coeff_modulus_create(4096, [60] * 3), list(range(1, 18)), all_default=True)


@pytest.fixture(scope="module")
def layer10(orc):
    """N = 1024, L = 2, every default Galois key: the set-up of the packed encrypted layers' emulator suites"""
    return fp.make_setup(orc, 10, _q1024(orc))


@pytest.fixture(scope="module")
def net10(orc):
    return mc.network_setup(orc, "6x20_3x6")


def _loaded(api, lib, S):
    return lambda: rm.load_ctx(api, lib, S)


@pytest.mark.parametrize("knob", [None, "2"])
def test_rotate_rows_many_chunked(orc, api, emu_lib, mem, rot10, monkeypatch, knob):
    """tests/test_rot_many_emu.py::test_chunks_and_streams_do_not_change_the_words with two items per chunk: B = 5 in chunks of 2, 2, 1
    on two lanes (no chunk covers the stride: the arena and the copies); knob 2: every chunk is recomputed step by step on the main
    lane after the join"""
    S = rot10
    cts = rm.encryptions(S, 5, seed=220)
    X = rm.load_ctx(api, emu_lib, S)
    got, refs = rm.check_rot_many(X, S, mem, orc, ROT_MIXED, cts=cts)
    group = min(rm.RotTrie(orc, S.n, ROT_MIXED, S.gk.elts).kid_counts[0], X.query("rot_many_group"))
    X.close()
    monkeypatch.setenv("HHE_CHUNK", str(2 * group))   # a chunk keeps the sums of `group` children of its items at once
    monkeypatch.setenv("HHE_STREAMS", "2")
    if knob:
        monkeypatch.setenv("HHE_ROT_HOIST", knob)
    with lazy_order(emu_lib, monkeypatch):
        Y = rm.load_ctx(api, emu_lib, S)
        before = Y.query("rot_many_fallbacks")
        g2, _ = rm.check_rot_many(Y, S, mem, orc, ROT_MIXED, cts=cts, refs=refs)
        fallbacks = Y.query("rot_many_fallbacks") - before
        Y.close()
    assert (g2 == got).all()
    assert fallbacks == (3 if knob else 0)


def test_rotate_rows_many_chunks_on_the_row_kernels(orc, api, emu_lib, mem, rot12, monkeypatch):
    """tests/test_rot_many_emu.py::test_chunks_on_the_row_kernels: three children, chunks of 2 + 1 items on two lanes"""
    cts = rm.encryptions(rot12, 3, seed=230)
    monkeypatch.setenv("HHE_CHUNK", "6")
    monkeypatch.setenv("HHE_STREAMS", "2")
    with lazy_order(emu_lib, monkeypatch):
        X = rm.load_ctx(api, emu_lib, rot12)
        assert X.query("row_kernel") == 1
        rm.check_rot_many(X, rot12, mem, orc, [1, 2, -5, 3], cts=cts)
        X.close()


def test_rotate_rows_many_raised_flag_is_read_after_the_chunks(orc, api, emu_lib, mem, monkeypatch):
    """tests/test_rot_many_emu.py::test_one_zero_residue_over_small_primes with one item per chunk on two lanes: the one flag that a
    chunk raises on its lane is on the host when the call decides what to recompute -- exactly that chunk, and its words are the oracle's"""
    logn, bits = pc.ZERO_CASES["n1024_18x4"][:2]
    steps = [1, 2, 3]
    S = rm.setup_with_steps(orc, logn, orc.coeff_modulus_create(1 << logn, bits), steps)
    cts = None
    for seed in range(180, 200):   # an encryption whose c1 has no zero residue (they are common at 18 bits)
        c = rm.encryptions(S, 3, seed=seed)
        if (c[:, 1] != 0).all():
            cts = c
            break
    assert cts is not None
    monkeypatch.setenv("HHE_CHUNK", "3")   # three children at once: one item per chunk
    monkeypatch.setenv("HHE_STREAMS", "2")
    with lazy_order(emu_lib, monkeypatch):
        X = rm.load_ctx(api, emu_lib, S)
        rm.check_rot_many(X, S, mem, orc, steps, cts=cts)
        assert X.query("rot_many_fallbacks") == 0
        cts[1, 1, 1, 517] = 0
        rm.check_rot_many(X, S, mem, orc, steps, cts=cts)
        assert X.query("rot_many_fallbacks") == 1
        X.close()


def test_fc_packed_chunked(api, emu_lib, mem, layer10, monkeypatch):
    """hhe_fc_packed_ks: fc_packed_common.check_chunking (B = 5, one item per chunk on two lanes; two per chunk on the caller's stream)"""
    with lazy_order(emu_lib, monkeypatch):
        fp.check_chunking(_loaded(api, emu_lib, layer10), layer10, mem, monkeypatch)


@pytest.mark.parametrize("hoisted", [0, 1])
def test_fc_packed_sum_and_hoisted_chunked(api, emu_lib, mem, layer10, monkeypatch, hoisted):
    """tests/test_mult_sum_emu.py::test_chunks_and_streams_do_not_change_the_words: every call of check_sum_layer runs hhe_fc_packed_ks,
    hhe_fc_packed_hoisted_ks and hhe_fc_packed_sum_ks on one handle"""
    S, M = layer10, fp.seeded_matrix(fp.T, 3, 5, 61)
    X = rm.load_ctx(api, emu_lib, S)
    got, refs, _ = msc.check_sum_layer(X, S, mem, M, hoisted, B=5, seed=7)
    X.close()
    with lazy_order(emu_lib, monkeypatch):
        for chunk, streams in (("2", "2"), ("8", "0")):
            monkeypatch.setenv("HHE_CHUNK", chunk)
            monkeypatch.setenv("HHE_STREAMS", streams)
            Y = rm.load_ctx(api, emu_lib, S)
            g2, _, _ = msc.check_sum_layer(Y, S, mem, M, hoisted, B=5, seed=7, refs=refs)
            assert (g2 == got).all(), (chunk, streams)
            Y.close()


def test_fc_packed_hoisted_in_place_under_the_fallback(orc, api, emu_lib, mem, monkeypatch):
    """tests/test_rot_many_emu.py::test_layer_in_place_and_under_the_fallback on two lanes: in place every chunk's result waits in
    the context's buffer, the chunks are recomputed from the untouched input and the results copied out after them"""
    S = rm.setup_with_steps(orc, 10, _q1024(orc), rm.hand_hoisted_steps(1024, 3, 5), all_default=True)
    M = fp.seeded_matrix(fp.T, 3, 5, 62)
    X = rm.load_ctx(api, emu_lib, S)
    got, refs, _ = rm.check_hoisted_layer(X, S, mem, orc, M, B=3, seed=8)
    X.close()
    monkeypatch.setenv("HHE_CHUNK", "8")   # r = 4: two items per chunk
    monkeypatch.setenv("HHE_STREAMS", "2")
    with lazy_order(emu_lib, monkeypatch):
        for knob in ("1", "2"):
            monkeypatch.setenv("HHE_ROT_HOIST", knob)
            Y = rm.load_ctx(api, emu_lib, S)
            g3, _, _ = rm.check_hoisted_layer(Y, S, mem, orc, M, B=3, seed=8, in_place=True, refs=refs, chain=False)
            assert (g3 == got).all() and Y.query("rot_many_fallbacks") == (2 if knob == "2" else 0)
            Y.close()


def test_fc_packed_sum_in_place_under_the_fallback(api, emu_lib, mem, layer10, monkeypatch):
    """hhe_fc_packed_sum_ks with hoisted = 1 in place, every chunk recomputed (tests/test_mult_sum_emu.py's test_in_place and
    test_forced_fallback_of_the_hoisted_rotation in one)"""
    S, M = layer10, fp.seeded_matrix(fp.T, 3, 5, 63)
    X = rm.load_ctx(api, emu_lib, S)
    got, refs, _ = msc.check_sum_layer(X, S, mem, M, 1, B=3, seed=9)
    X.close()
    monkeypatch.setenv("HHE_CHUNK", "8")
    monkeypatch.setenv("HHE_STREAMS", "2")
    monkeypatch.setenv("HHE_ROT_HOIST", "2")
    with lazy_order(emu_lib, monkeypatch):
        Y = rm.load_ctx(api, emu_lib, S)
        before = Y.query("rot_many_fallbacks")
        g2, _, _ = msc.check_sum_layer(Y, S, mem, M, 1, B=3, seed=9, in_place=True, refs=refs)
        assert Y.query("rot_many_fallbacks") > before
        Y.close()
    assert (g2 == got).all()


def test_mlp_chunked(api, emu_lib, mem, net10, monkeypatch):
    """hhe_mlp_ks and hhe_fc_open_ks (the layers one by one inside check_network): mlp_common.check_chunking"""
    with lazy_order(emu_lib, monkeypatch):
        mc.check_chunking(_loaded(api, emu_lib, net10), net10, mem, monkeypatch)


def test_mlp_fallback_on_two_lanes(api, emu_lib, mem, net10, monkeypatch):
    """mlp_common.check_fallback with one item per chunk on two lanes: every chunk recomputed whole from vi on the main lane, and in
    place under the fallback"""
    monkeypatch.setenv("HHE_CHUNK", "8")   # max r = 8
    monkeypatch.setenv("HHE_STREAMS", "2")
    with lazy_order(emu_lib, monkeypatch):
        mc.check_fallback(_loaded(api, emu_lib, net10), net10, mem, monkeypatch)


@pytest.fixture(scope="module")
def fc10(orc):
    """N = 1024, L = 2, every default Galois key"""
    return Setup(orc, 10, [50] * 3, all_galois=True)


@pytest.mark.parametrize("shared", ["2", "1"])
def test_fc_row_chunks_on_two_lanes(orc, api, emu_lib, mem, fc10, monkeypatch, shared):
    """hhe_fc_row, B = 3 with one item per chunk on two lanes, against the oracle's row as tests/test_host_emu.py compares it
    (parity_common.check_fc_variants' inputs); shared 2: every chunk recomputed with per-child transforms on the main lane"""
    S, O, n_in, B = fc10, fc10.O, 21, 3
    rng = np.random.default_rng(8)
    v, w = rng.integers(0, 4, n_in), rng.integers(-8, 9, n_in)
    wc = O.encrypt(S.pk, O.encode(w), 43)
    vi = np.stack([O.encrypt(S.pk, O.encode(v), 41 + b) for b in range(B)])
    refs = [O.fc_row(vi[b], wc, S.rk, S.gk, n_in)[0] for b in range(B)]
    monkeypatch.setenv("HHE_FC_CHUNK", "1")
    monkeypatch.setenv("HHE_STREAMS", "2")
    monkeypatch.setenv("HHE_FC_SHARED", shared)
    with lazy_order(emu_lib, monkeypatch):
        X = api.Context(S.logn, S.q, S.t, lib=emu_lib)
        S.load_keys(X)
        before = X.query("fc_fallbacks")
        out = mem.empty((B,) + O.ct_shape)
        X.fc_row(mem.to_dev(vi), mem.to_dev(wc[None]), 1, n_in, out, B, relin_slot=0, default_galois_only=False)
        got = mem.to_host(out)
        fallbacks = X.query("fc_fallbacks") - before
        X.close()
    for b in range(B):
        assert (got[b] == refs[b]).all(), (shared, b)
    assert fallbacks == (B if shared == "2" else 0)
