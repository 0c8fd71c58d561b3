"""The chunk scheduler and the grow-only workspaces of the host driver (csrc/hhe_api.cpp: ChunkPlan / run_chunks, GrowBuf):
hhe_pasta3_transcipher, hhe_packed_affine_ks and hhe_fc_row_ks on one context with two internal streams and two items per chunk,
each first with a small batch, then with a larger one (several chunks, a ragged last one, every workspace reallocated after the
lanes have been used), then with the small one again -- word for word against fresh contexts and the oracle
(parity_common.check_batched_calls_regrow).  At N = 2048 on the emulator and, marked gpu, on real streams of an MI355X
(python -m pytest tests -m gpu)."""
import pytest

import affine_common as ac
import parity_common as pc
from conftest import Setup


def _run(orc, api, lib, mem, monkeypatch):
    for k in ("HHE_STREAMS", "HHE_CHUNK", "HHE_FC_CHUNK"):
        monkeypatch.setenv(k, "2")
    S = Setup(orc, 11, [60] * 4, all_galois=True, extra_steps=[-16 * k for k in range(1, 8)] + ac.hand_steps(2048, 16, 4, 4))
    pc.check_batched_calls_regrow(lambda: api.Context(S.logn, S.q, S.t, lib=lib), S, orc, mem)


def test_batched_calls_small_large_small_on_emulator(orc, api, emu_lib, monkeypatch):
    _run(orc, api, emu_lib, pc.HostMem(), monkeypatch)


@pytest.mark.gpu
def test_batched_calls_small_large_small_on_gfx950(orc, api, monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    lib = api.load_library()  # fails loudly if the HIP library is missing
    assert lib.hhe_backend() == b"hip-gfx950"
    _run(orc, api, lib, pc.TorchMem("cuda:0"), monkeypatch)
