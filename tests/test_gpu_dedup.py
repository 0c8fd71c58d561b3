"""One keystream per block counter on the gfx950 kernels (see dedup_common and test_dedup): the benchmark's parameters with and
without the fused row kernel, and the two-chunk batch path of the row kernel, which a call of one counter no longer takes by
default."""
import numpy as np
import pytest

from conftest import Setup
import dedup_common as dc
import parity_common as pc

IDS, NCW = [0, 0, 6, 0], [128, 128, 16, 5]  # non-adjacent duplicates, ragged lengths inside the group of counter 0


@pytest.fixture(scope="module")
def mem():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pc.TorchMem("cuda:0")


@pytest.fixture(scope="module")
def lib(api):
    lib = api.load_library()
    assert lib.hhe_backend() == b"hip-gfx950"
    return lib


@pytest.fixture(scope="module")
def bench_setup(orc):
    return Setup(orc, 15, [60] * 4)


@pytest.mark.gpu
def test_gpu_bench_parameters(orc, api, lib, mem, bench_setup, monkeypatch):
    S = bench_setup
    X1, X0, _ = dc.check_dedup(api, lib, S, orc, mem, monkeypatch, dc.words(S, 4, 21), NCW, IDS, unique=2, oracle_items=[1])
    assert X1.query("row_kernel") == 1
    X1.close(), X0.close()


@pytest.mark.gpu
def test_gpu_without_the_row_kernel(orc, api, lib, mem, monkeypatch):
    S, _ = pc.dispatch_setup(orc, api, lib, "A", all_galois=False, extra_steps=())
    X1, X0, _ = dc.check_dedup(api, lib, S, orc, mem, monkeypatch, dc.words(S, 4, 22), NCW, IDS, unique=2, oracle_items=[1])
    assert X1.query("row_kernel") == 0
    X1.close(), X0.close()


@pytest.mark.gpu
def test_gpu_two_chunk_batch_of_one_counter(orc, api, lib, mem, bench_setup, monkeypatch):
    """130 items of counter 0: per item they are two chunks of 65 on the row kernel's batch path; grouped they are one evaluation
    (every bracketed ks_row_kernel launch covers one ciphertext) and a finishing pass of two chunks"""
    S, B = bench_setup, 130
    cw, ncw, ids = dc.words(S, B, 23), [128] * (B - 1) + [7], [0] * B
    X1 = dc.make_ctx(api, lib, S, monkeypatch, HHE_DEDUP=1)
    X1.profile(True)
    r1 = dc.run(X1, S, mem, cw, ncw, ids)
    _, launches, _, items = X1.profile_read()
    assert X1.query("transcipher_unique") == 1 and launches > 0 and items == launches, (launches, items)
    X1.close()
    X0 = dc.make_ctx(api, lib, S, monkeypatch, HHE_DEDUP=0)
    r0 = dc.run(X0, S, mem, cw, ncw, ids)
    assert X0.query("transcipher_unique") == B
    X0.close()
    assert (r1 == r0).all()
