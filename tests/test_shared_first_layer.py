"""The first affine layer of the fused matmul on shared operands (HHE_SHARED_L0, DESIGN.md "shared first layer"): every
item of a transciphering call starts from the same key ciphertext, so the layer's 127 key switches run once per call and an
item only multiplies its own diagonals into the shared rotated states (diag_sum_body behind k_perm).  Everything here is exact
equality of ciphertext words: knob 1 (every call shares) against knob 0 (the per-item chain) and against the oracle's
transcipher_block.  The knob's value is the smallest batch that shares; the default (12) keeps one-record calls on the per-item
chain, where a few items cost what the one shared ciphertext costs.

The N / 2 = 128 branch of the layer (no rotate_rows(128) + add in front of the chain) is NOT covered: N = 256 is below the
smallest pass either backend builds."""
import numpy as np
import pytest

from conftest import Setup
import parity_common as pc
from shared_l0_common import blocks_of, check_knob, make_ctx, oracle_blocks, run  # noqa: F401


@pytest.fixture(scope="module")
def hostmem():
    return pc.HostMem()


# ------------------------------------------------------------------ CPU: the emulator runs the shared kernel bodies and the real host driver

def test_single_item(orc, api, emu_lib, hostmem, small, monkeypatch):
    cw, ncw = blocks_of(small, orc, 128)
    X1, _, _ = check_knob(api, emu_lib, small, orc, hostmem, monkeypatch, cw, ncw, [0])
    assert X1.query("shared_l0_steps") == 128  # the whole chain in one block of steps


def test_five_items_distinct_counters_ragged_last_block(orc, api, emu_lib, hostmem, small, monkeypatch):
    cw, ncw = blocks_of(small, orc, 4 * 128 + 17)
    assert list(ncw) == [128] * 4 + [17]
    check_knob(api, emu_lib, small, orc, hostmem, monkeypatch, cw, ncw, [0, 1, 2, 3, 9], oracle_items=[0, 3, 4])


def test_context_with_the_row_kernel(orc, api, emu_lib, hostmem, monkeypatch):
    """N = 4096, pseudo-Mersenne primes: layers 1-3 run ks_row_kernel, the shared chain of layer 0 the separate-kernel step"""
    S = Setup(orc, 12, [50, 50, 50])
    cw, ncw = blocks_of(S, orc, 128 + 40, seed=13)
    X1, _, _ = check_knob(api, emu_lib, S, orc, hostmem, monkeypatch, cw, ncw, [3, 4], oracle_items=[1])
    assert X1.query("row_kernel") == 1


def test_context_without_the_row_kernel(orc, api, emu_lib, hostmem, small, monkeypatch):
    cw, ncw = blocks_of(small, orc, 2 * 128, seed=5)
    X1, _, _ = check_knob(api, emu_lib, small, orc, hostmem, monkeypatch, cw, ncw, [7, 8], oracle_items=[0])
    assert X1.query("row_kernel") == 0


def test_several_lanes_read_one_table(orc, api, emu_lib, hostmem, small, monkeypatch):
    cw, ncw = blocks_of(small, orc, 5 * 128 - 3, seed=7)
    check_knob(api, emu_lib, small, orc, hostmem, monkeypatch, cw, ncw, [0, 1, 2, 3, 4], oracle_items=[2, 4], HHE_STREAMS=2, HHE_CHUNK=2)


def test_caller_stream_only(orc, api, emu_lib, hostmem, small, monkeypatch):
    cw, ncw = blocks_of(small, orc, 2 * 128, seed=9)
    check_knob(api, emu_lib, small, orc, hostmem, monkeypatch, cw, ncw, [0, 1], oracle_items=[1], HHE_STREAMS=0)


@pytest.mark.parametrize("mb,steps", [(0.6, 3), (0.0, 2), (7.5, 40)])
def test_budget_forces_blocks_of_steps(orc, api, emu_lib, hostmem, small, monkeypatch, mb, steps):
    """N = 1024, L = 8: one state takes 3 * 8 * 1024 words = 192 KiB of the table.  3 states per block: 43 blocks with a ragged last
    one (128 = 42 * 3 + 2); 2: the smallest table (a step reads one slot and writes the next); 40: the fold of the lazy sums (every
    32 products) inside a block that is carried"""
    cw, ncw = blocks_of(small, orc, 2 * 128 + 5, seed=11)
    X1, _, _ = check_knob(api, emu_lib, small, orc, hostmem, monkeypatch, cw, ncw, [0, 1, 2], oracle_items=[2], HHE_SHARED_L0_MB=mb)
    assert X1.query("shared_l0_steps") == steps


def test_two_calls_with_different_keys_reuse_nothing(orc, api, emu_lib, hostmem, small, monkeypatch):
    O = small.O
    key2 = (small.key * 3 + 1) % small.t
    enc2 = O.encrypt(small.pk, O.pasta_pack_key(key2), 12)
    cw, ncw = blocks_of(small, orc, 128 + 60, seed=15)
    X = make_ctx(api, emu_lib, small, monkeypatch, HHE_SHARED_L0=1)
    ra = run(X, small, hostmem, cw, ncw, [0, 1])
    rb = run(X, small, hostmem, cw, ncw, [0, 1], enc_key=enc2)
    rc = run(X, small, hostmem, cw, ncw, [0, 1])
    assert (ra == rc).all() and not (ra == rb).all()
    assert (ra[1] == oracle_blocks(small, cw, ncw, [0, 1], [1])[1]).all()
    assert (rb[1] == oracle_blocks(small, cw, ncw, [0, 1], [1], enc_key=enc2)[1]).all()


def test_decompose_of_a_multi_block_record(orc, api, emu_lib, hostmem, monkeypatch):
    S = Setup(orc, 10, [50] * 9, extra_steps=(-128, -256))
    O = S.O
    pt = np.array([(7 * i + 3) % 256 for i in range(300)], dtype=np.uint64)
    rec = orc.pasta_encrypt(S.t, S.key, pt)[None]
    res = []
    for knob in (1, 0):
        X = make_ctx(api, emu_lib, S, monkeypatch, HHE_SHARED_L0=knob)
        out = hostmem.empty((1,) + O.ct_shape)
        X.decompose(hostmem.to_dev(S.enc_key), rec, out, mask_last=True)
        res.append(hostmem.to_host(out))
    assert (res[0] == res[1]).all()
    cw, ncw = S.sym_blocks(orc, pt)
    blocks = [O.transcipher_block(S.enc_key, S.rk, S.gk, cw[b, :ncw[b]], b) for b in range(3)]
    blocks[2] = O.mask(blocks[2], np.ones(44, np.uint64))
    assert (res[0][0] == O.flatten(np.stack(blocks), S.gk)).all()
    assert (O.decode(O.decrypt(S.sk, res[0][0]))[:300] == pt).all()


def test_default_threshold_keeps_small_calls_on_the_per_item_chain(orc, api, emu_lib, hostmem, small, monkeypatch):
    cw, ncw = blocks_of(small, orc, 128, seed=19)
    X = make_ctx(api, emu_lib, small, monkeypatch)
    assert X.query("shared_l0") == 12
    r = run(X, small, hostmem, cw, ncw, [2])
    assert X.query("shared_l0_steps") == 0
    X1 = make_ctx(api, emu_lib, small, monkeypatch, HHE_SHARED_L0=1)
    assert (r == run(X1, small, hostmem, cw, ncw, [2])).all() and X1.query("shared_l0_steps") == 128


def test_block_cache_accounting_is_untouched(orc, api, emu_lib, hostmem, small, monkeypatch):
    """the operand table is a workspace, not a block table"""
    cw, ncw = blocks_of(small, orc, 2 * 128)
    stats = []
    for knob in (1, 0):
        X = make_ctx(api, emu_lib, small, monkeypatch, HHE_SHARED_L0=knob)
        run(X, small, hostmem, cw, ncw, [0, 1])
        stats.append((X.query("block_cache_bytes"), X.query("block_cache_entries")))
    assert stats[0] == stats[1] and stats[0][1] == 2


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def gpumem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pc.TorchMem("cuda:0")


@pytest.fixture(scope="module")
def lib(api):
    lib = api.load_library()
    assert lib.hhe_backend() == b"hip-gfx950"
    return lib


def gpu_case(S, orc):
    """B = 3, counters 0, 1, 6, 16 words in the last block"""
    cw, ncw = blocks_of(S, orc, 2 * 128 + 16, seed=17)
    assert list(ncw) == [128, 128, 16]
    return cw, ncw, [0, 1, 6]


@pytest.mark.gpu
def test_gpu_bench_shape(orc, api, lib, gpumem, monkeypatch):
    S = Setup(orc, 15, [60] * 4)
    cw, ncw, ids = gpu_case(S, orc)
    X1, _, _ = check_knob(api, lib, S, orc, gpumem, monkeypatch, cw, ncw, ids, oracle_items=[0])
    assert X1.query("row_kernel") == 1 and X1.query("shared_l0_steps") == 128


@pytest.mark.gpu
def test_gpu_bench_shape_in_blocks_of_steps(orc, api, lib, gpumem, monkeypatch):
    """the same with a 96 MB budget: 2.25 MiB per state, 42 states per block, accumulators carried through `out`"""
    S = Setup(orc, 15, [60] * 4)
    cw, ncw, ids = gpu_case(S, orc)
    X1 = make_ctx(api, lib, S, monkeypatch, HHE_SHARED_L0=1, HHE_SHARED_L0_MB=96)
    X0 = make_ctx(api, lib, S, monkeypatch, HHE_SHARED_L0=0)
    assert (run(X1, S, gpumem, cw, ncw, ids) == run(X0, S, gpumem, cw, ncw, ids)).all()
    assert X1.query("shared_l0_steps") == 42


@pytest.mark.gpu
def test_gpu_without_the_row_kernel(orc, api, lib, gpumem, monkeypatch):
    S, _ = pc.dispatch_setup(orc, api, lib, "A", all_galois=False, extra_steps=())
    cw, ncw, ids = gpu_case(S, orc)
    X1, _, _ = check_knob(api, lib, S, orc, gpumem, monkeypatch, cw, ncw, ids, oracle_items=[0])
    assert X1.query("row_kernel") == 0


@pytest.mark.gpu
def test_gpu_profile_counts_batch_launches_only(orc, api, lib, gpumem, monkeypatch):
    """hhe_ctx_profile brackets the batch launches of ks_row_kernel: items / launches is the chunk's item count, with the shared
    chain (one ciphertext, separate kernels) outside; and a quarter of the per-item path's launches are gone"""
    S, _ = pc.dispatch_setup(orc, api, lib, "H", all_galois=False, extra_steps=())
    cw, ncw, ids = gpu_case(S, orc)
    launches = {}
    for knob in (1, 0):
        X = make_ctx(api, lib, S, monkeypatch, HHE_SHARED_L0=knob)
        assert X.query("row_kernel") == 1
        X.profile(True)
        run(X, S, gpumem, cw, ncw, ids)
        _, n, _, items = X.profile_read()
        assert n > 0 and items == 3 * n, (knob, n, items)
        launches[knob] = n
        X.close()
    assert launches[0] - launches[1] == 127
