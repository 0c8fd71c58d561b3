"""The steady transciphering step (DESIGN.md "Steady step: the item kernel first"): what tests/test_steady_step_emu.py (emulator, eager
and under the lazy order) and tests/test_gpu_steady_step.py share.  A call whose counters all have a kept keystream launches the item
kernel on a prediction IN FRONT of the key comparison, the kernel reads the items' words where the host staged them (page-locked
staging), and a pointer table the device already holds is not uploaded again.

Every comparison is exact equality of ciphertext words with a context created under HHE_FIN_ITEM=0 (the two-pass kernels, which take
no prediction and upload their words) and, for named items, with the oracle's transcipher_block.  What a call sent is read from the
context: fin_tab_uploads and fin_word_uploads count the uploads that were enqueued, fin_item_launches the launches.

Why the FIRST steady call of a sequence uploads a table although its counters are those of the cold call before it: the cold call's
table points at the keystreams where they were evaluated (ks_tab), a steady call's at the copies the cache keeps.  The bytes differ,
so that one upload is owed; from the second steady call on nothing is."""
import contextlib
import ctypes

import dedup_common as dc
import fused_finish_common as ff
import kscache_common as kc
import parity_common as pc

IDS = [0, 2, 0]


# ---- the lazy order of the emulator (tests/emu/emu_order.cpp), as tests/test_stream_order_emu.py drives it

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
    """numpy memory that keeps every buffer it handed out alive: work a broken schedule left pending runs after its call has returned
    and must find the call's buffers, so that the test fails on its comparison of words and not on a read of released memory"""

    def __init__(self):
        self.kept = []

    def to_dev(self, a):
        self.kept.append(super().to_dev(a))
        return self.kept[-1]

    def empty(self, shape):
        self.kept.append(super().empty(shape))
        return self.kept[-1]


@contextlib.contextmanager
def lazy_order(lib, monkeypatch, min_pending=4):
    """everything inside runs under HHE_EMU_ORDER=lazy; on the way out: work was deferred, forced, and at least min_pending operations
    were pending at once"""
    device_sync(lib)
    lib.emu_order_window.argtypes, lib.emu_order_window.restype = [], None
    lib.emu_order_window()
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


@contextlib.contextmanager
def eager_order(lib, monkeypatch):
    monkeypatch.delenv("HHE_EMU_ORDER", raising=False)
    yield


# ---- the checkers

def sent(X):
    """(table uploads, word uploads, item-kernel launches) of the context so far"""
    return X.query("fin_tab_uploads"), X.query("fin_word_uploads"), X.query("fin_item_launches")


def item_pair(api, lib, S, monkeypatch, **env):
    """(context under HHE_FIN_ITEM=1, context under HHE_FIN_ITEM=0) with the same further knobs"""
    X = dc.make_ctx(api, lib, S, monkeypatch, HHE_FIN_ITEM=1, **env)
    X0 = dc.make_ctx(api, lib, S, monkeypatch, HHE_FIN_ITEM=0, **env)
    assert X.query("fin_item") == 1 and X0.query("fin_item") == 0
    return X, X0


def call(S, mem, X, X0, cw, ncw, ids, tab, launches=1, words=0, oracle_items=()):
    """one call on both contexts: the same words, named items the oracle's; X enqueued `tab` table uploads, `words` uploads of the
    words and `launches` item kernels"""
    before = sent(X)
    r = ff.same(S, mem, X, X0, cw, ncw, ids, oracle_items=oracle_items)
    after = sent(X)
    assert tuple(a - b for a, b in zip(after, before)) == (tab, words, launches), (before, after)
    return r


def check_same_table_new_words(api, lib, S, mem, monkeypatch, **env):
    """a cold call, then three steady ones with the same key and counters and other words and lengths (0 and 128 among them): the
    first steady call uploads the table of kept keystreams, the next two nothing; no call uploads words; one launch each; every
    result is its own call's words"""
    X, X0 = item_pair(api, lib, S, monkeypatch, **env)
    call(S, mem, X, X0, kc.words(S, 3, 91), [128, 9, 128], IDS, tab=1)
    assert kc.counts(X) == (2, 0)
    results = []
    for k, (ncw, tab) in enumerate((([128, 0, 9], 1), ([0, 128, 128], 0), ([77, 1, 0], 0))):
        results.append(call(S, mem, X, X0, kc.words(S, 3, 92 + k), ncw, IDS, tab=tab, oracle_items=(k,)))
        assert kc.counts(X) == (0, 2) and kc.counts(X0) == (0, 2)
    assert (results[0] != results[1]).any() and (results[1] != results[2]).any()
    assert X.query("fin_word_uploads") == 0 and X0.query("fin_word_uploads") == 4 and X0.query("fin_item_launches") == 0
    X.close(), X0.close()


def check_table_changes(api, lib, S, mem, monkeypatch, **env):
    """other counters at the same item count, more items with the same leading counters, the first item count again: every change
    uploads, an identical repeat does not, and the words are right each time"""
    X, X0 = item_pair(api, lib, S, monkeypatch, **env)
    cw = kc.words(S, 5, 95)
    ncw = [128, 30, 1, 0, 64]
    call(S, mem, X, X0, cw[:3], ncw[:3], IDS, tab=1)  # cold
    for ids in (IDS, [2, 0, 0], [2, 0, 0, 2, 0], [2, 0, 0]):
        B = len(ids)
        first = call(S, mem, X, X0, cw[:B], ncw[:B], ids, tab=1, oracle_items=(1,))
        again = call(S, mem, X, X0, cw[:B], ncw[:B], ids, tab=0)
        assert (first == again).all() and kc.counts(X) == (0, 2)
    X.close(), X0.close()


def check_both_paths(api, lib, S, mem, monkeypatch, **env):
    """the default knob: 64 items take the item kernel, 3 items the two-pass kernels, whose map and words go where the table of the
    64 was; the 64 again upload their table again and give the words they gave before"""
    X = dc.make_ctx(api, lib, S, monkeypatch, **env)
    X0 = dc.make_ctx(api, lib, S, monkeypatch, HHE_FIN_ITEM=0, **env)
    assert X.query("fin_item") == 1 and 3 < X.query("fin_item_min") <= 64 and X0.query("fin_item") == 0
    cw, ncw, ids = kc.words(S, 64, 96), [128 - (b % 5) * 31 for b in range(64)], [0] * 64
    call(S, mem, X, X0, cw, ncw, ids, tab=1)  # cold
    first = call(S, mem, X, X0, cw, ncw, ids, tab=1, oracle_items=(63,))
    assert (kc.run(X, S, mem, cw, ncw, ids) == first).all() and sent(X) == (2, 0, 3)
    small = call(S, mem, X, X0, cw[:3], ncw[:3], ids[:3], tab=1, words=1, launches=0)
    assert (small == first[:3]).all()
    assert (call(S, mem, X, X0, cw, ncw, ids, tab=1) == first).all()
    assert (call(S, mem, X, X0, cw, ncw, ids, tab=0) == first).all()
    X.close(), X0.close()


def check_growth(api, lib, S, mem, monkeypatch, **env):
    """steady calls of three items, a call of seven (fin_dev grows), the three again; then hhe_ctx_reserve grows fin_dev between two
    identical calls: the new block holds no table, so the table goes up again"""
    X, X0 = item_pair(api, lib, S, monkeypatch, **env)
    cw, ncw = kc.words(S, 7, 97), ff.SEVEN_NCW
    call(S, mem, X, X0, cw[:3], ncw[:3], IDS, tab=1)
    three = call(S, mem, X, X0, cw[:3], ncw[:3], IDS, tab=1)
    call(S, mem, X, X0, cw[:3], ncw[:3], IDS, tab=0)
    call(S, mem, X, X0, cw, ncw, [0, 2, 0, 2, 2, 0, 0], tab=1, oracle_items=(6,))
    assert kc.counts(X) == (0, 2)
    assert (call(S, mem, X, X0, cw[:3], ncw[:3], IDS, tab=1) == three).all()
    assert (call(S, mem, X, X0, cw[:3], ncw[:3], IDS, tab=0) == three).all()
    X.reserve(40)
    assert (call(S, mem, X, X0, cw[:3], ncw[:3], IDS, tab=1, oracle_items=(1,)) == three).all()
    assert (call(S, mem, X, X0, cw[:3], ncw[:3], IDS, tab=0) == three).all()
    X.close(), X0.close()


def check_keys(api, lib, S, mem, monkeypatch, in_place=False, **env):
    """fused_finish_common.check_prediction (keys A, A, B, A, then A confirmed with one launch), the knob set as it wants it; then the
    same sequence with what each call sent: a refuted call finds the predicted table on the device where the call before left it, or
    uploads it, and uploads the table it finishes with"""
    for k, v in dict(HHE_FIN_ITEM=1, **env).items():  # check_prediction creates its contexts under the caller's environment
        monkeypatch.setenv(k, str(v))
    ff.check_prediction(api, lib, S, mem, monkeypatch, in_place=in_place)
    for k in dict(HHE_FIN_ITEM=1, **env):
        monkeypatch.delenv(k, raising=False)
    X, X0 = item_pair(api, lib, S, monkeypatch, **env)
    cw, ncw = kc.words(S, 3, 98), [128, 9, 128]
    enc_b = kc.other_enc_key(S, 1)
    key_a, key_b = mem.to_dev(S.enc_key), mem.to_dev(enc_b)
    results = []
    # cold | confirmed, table of A's kept keystreams | predicts A with the table the device holds, refuted, finishes out of ks_tab |
    # predicts B and uploads B's table, refuted, uploads A's | predicts A: confirmed, nothing to upload
    for key, want, tab, launches in ((key_a, (2, 0), 1, 1), (key_a, (0, 2), 1, 1), (key_b, (2, 0), 1, 2), (key_a, (0, 2), 2, 2), (key_a, (0, 2), 0, 1)):
        before = sent(X)
        results.append(kc.run(X, S, mem, cw, ncw, IDS, key=key))
        assert tuple(a - b for a, b in zip(sent(X), before)) == (tab, 0, launches) and kc.counts(X) == want
        assert (kc.run(X0, S, mem, cw, ncw, IDS, key=key) == results[-1]).all()
    assert all((results[0] == results[k]).all() for k in (1, 3, 4)) and (results[0] != results[2]).any()
    assert (results[4][1] == dc.oracle_block(S, cw, ncw, IDS, 1)).all()
    assert (results[2][1] == dc.oracle_block(S, cw, ncw, IDS, 1, enc_key=enc_b)).all()
    X.close(), X0.close()


def check_cache_cleared(api, lib, S, mem, monkeypatch, **env):
    """hhe_pasta3_clear_keystream_cache between two steady calls: the same call evaluates its two counters again, the next one hits;
    the words are the same throughout"""
    X, X0 = item_pair(api, lib, S, monkeypatch, **env)
    cw, ncw = kc.words(S, 3, 99), [5, 128, 0]
    call(S, mem, X, X0, cw, ncw, IDS, tab=1)
    r = call(S, mem, X, X0, cw, ncw, IDS, tab=1, oracle_items=(0,))
    call(S, mem, X, X0, cw, ncw, IDS, tab=0)
    X.clear_keystream_cache()
    assert X.query("ks_cache_entries") == 0
    before = sent(X)
    assert (kc.run(X, S, mem, cw, ncw, IDS) == r).all() and kc.counts(X) == (2, 0)
    assert sent(X)[1:] == (before[1], before[2] + 1)
    assert (kc.run(X, S, mem, cw, ncw, IDS) == r).all() and kc.counts(X) == (0, 2)
    assert (kc.run(X, S, mem, cw, ncw, IDS) == r).all() and kc.counts(X) == (0, 2)
    assert sent(X)[1:] == (before[1], before[2] + 3)
    X.close(), X0.close()
