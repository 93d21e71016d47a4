"""The quantising KV append of an fp8-KV engine (epilogue<EPI_QKV_ROPE>, csrc/gemv_device.h), bit for bit.

One-layer `random_init` models: layer 0's K and V depend on the embedding only, so the cache of a bf16-KV engine run over the same
tokens and positions is the exact input of the quantiser, and the e4m3 cache must hold
(bf16_cache / scale).clamp(-448, 448).to(float8_e4m3fn) on the written positions and zero bytes everywhere else. Every route that
owns an append: the GEMV (1 and 5 tokens), a 40-token and a 100-token pass of the multi-token kernels, and a 300-token prompt
through epilogue_rows_kernel of both prefill backends (its K / V taken from the bf16 engine's prompt on the same backend)."""

import pytest
import torch

import attention_cases as A
from specdec_hip.engine import HipModel
from test_hip_attention_geometry_gpu import _weights
from test_hip_prefill_rows_fp64_gpu import _backend

pytestmark = pytest.mark.gpu

ROUTES = [(md, M, "passes") for md in (A.MHA, A.G3) for M in (1, 5, 40, 100)] + [(A.G3, 300, b) for b in ("native", "rocblas")]
WHERE = [(0, (1.0, 1.0)), (37, (0.25, 2.0))]   # start position, (k_scale, v_scale)


@pytest.mark.parametrize("start,scales", WHERE, ids=["pos0-unit", "pos37-scaled"])
@pytest.mark.parametrize("md,M,backend", ROUTES, ids=[f"{md.name}-{M}-{b}" for md, M, b in ROUTES])
def test_append_is_the_quantised_bf16_cache(md, M, backend, start, scales):
    if backend != "passes":
        _backend(backend)
    mw = _weights(md)
    tok = torch.randint(4, md.vocab, (1, M), generator=torch.Generator(device="cuda").manual_seed(M + start), device="cuda", dtype=torch.int32)
    pos = torch.tensor([start], dtype=torch.int32, device="cuda")
    caches = {}
    for kvd in ("bf16", "fp8"):
        eng = HipModel(mw, batch=2, l_max=512, prefill_backend=backend, kv_dtype=kvd, kv_scales=scales)   # row0 = 1 of a 2-row bind
        eng.forward(tok, pos, row0=1, skip_head=True)
        assert eng.engine_status() == 0
        caches[kvd] = eng.kv_view()
    for name, ref, got, s in zip("KV", caches["bf16"], caches["fp8"], scales):
        want = (ref.float() / s).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        written = torch.zeros_like(want, dtype=torch.bool)
        (written[0, 1, :, start:start + M] if name == "K" else written[0, 1, :, :, start:start + M]).fill_(True)
        assert bool((ref != 0)[written].any()) and not bool((ref != 0)[~written].any())       # the bf16 engine wrote these and only these
        g = got.view(torch.uint8)
        assert torch.equal(g[written], want[written]), f"{name}: {int((g != want)[written].sum())} of {int(written.sum())} written bytes differ"
        assert not bool(g[~written].any()), f"{name}: a byte outside the written positions is not zero"
