"""attention_mfma_kv8_kernel (csrc/attention_kv8.hip: 64-key blocks over an e4m3 cache) against fp64, by the cases of
tests/attention_cases.py.

Every dense case whose model an fp8-KV engine can bind (head_dim 64 or 128; the D = 32 models of the table are refused at bind),
plus one launch whose rows hold 1, 63, 64, 65 and 129 cached keys: the edges of the new block. The table already has launches of
more than one 16-row tile (tile-edge-M9 / -M17, g3-d128, cap-1b) and split launches whose rows use different s_eff (ragged,
cap-1b). The written prefix carries the case's sentinel layout, quantised through kv_view; after one forward q and the attention
rows are read with debug_rows and the cache — new positions included — with kv_view, and every element is held to
stage_ref.attention_stage over the DEQUANTISED cache and its derived bound. Each case runs with and without the split and issues
its forward twice (bit-identical).

On the bound. attention_stage's terms hold for this kernel as they stand: e4m3 -> bf16 is exact, so the operands of both
contractions are the dequantised values divided by a power of two; the scores chain D / 32 MFMA steps and the PV sums one step per
32 keys, as counted; a 64-key block halves the running-max rescalings the bound allows per 32 keys. The one assumption e4m3
scales could break is that `scale` is a single fp32 constant: k_scale * (1 / sqrt(D)) and v_scale / den are further fp32
roundings for general scales. The cases use powers of two (k_scale 1/2, v_scale >= 1 chosen so that the largest sentinel is
representable: amplitude / 256), for which both products are exact and no term changes."""

import pytest
import torch

import attention_cases as A
import stage_ref as R
from specdec_hip.engine import HipModel
from test_hip_attention_geometry_gpu import _tokens, _weights

pytestmark = pytest.mark.gpu

BLOCK_EDGES = A.Case("kv8-block-edges", A.EDGE, (1, 63, 64, 65, 129), 5, 512)
CASES = [c for c in A.CASES if None in c.pages and c.model.D in (64, 128)] + [BLOCK_EDGES]
K_SCALE = 0.5


@pytest.mark.parametrize("split", [True, False], ids=["split", "nosplit"])
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_fp8_kv_attention_against_fp64(case, split, monkeypatch):
    if not split:
        monkeypatch.setenv("SPECDEC_NO_ATTN_SPLIT", "1")
    md, M, T = case.model, case.M, case.B * case.M
    v_scale = max(1.0, A.amplitude(max(case.lens) + M) / 256)
    eng = HipModel(_weights(md), batch=case.bound_batch, l_max=case.l_max, kv_dtype="fp8", kv_scales=(K_SCALE, v_scale))
    assert eng.l_max == case.l_max and not eng.persist_active(1) and T <= eng.pass_tokens
    k8, v8 = (t.view(torch.uint8) for t in eng.kv_view())
    for i in range(case.B):
        kk, vv = (t.to("cuda").float() for t in A.cache_row(case, i))          # [Hkv][n][D]
        n, row = kk.shape[1], case.row0 + i
        k8[0, row, :, :n] = (kk / K_SCALE).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        v8[0, row, :, :, :n] = (vv / v_scale).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).transpose(1, 2)
    tok = _tokens(case, len(case.id) + M)
    pos = torch.tensor(case.lens, dtype=torch.int32, device="cuda")
    _, logits = eng.forward(tok, pos, want_logits=True, row0=case.row0)
    q, attn = eng.debug_rows(HipModel.DEBUG_Q, T), eng.debug_rows(HipModel.DEBUG_ATTN, T).clone()
    _, logits2 = eng.forward(tok, pos, want_logits=True, row0=case.row0)
    assert torch.equal(attn, eng.debug_rows(HipModel.DEBUG_ATTN, T)) and torch.equal(logits, logits2), "a repeated forward differs"
    k, v = eng.kv_view()
    worst = 0.0
    for i, p0 in enumerate(case.lens):
        S, row = p0 + M, case.row0 + i
        kd = (k[0, row, :, :S].to(R.F64) * K_SCALE).expand(M, -1, -1, -1)
        vd = (v[0, row, :, :, :S].to(R.F64) * v_scale).transpose(1, 2).expand(M, -1, -1, -1)
        q_pos = torch.arange(p0, p0 + M, device="cuda")
        ref = R.attention_stage(q[i * M:(i + 1) * M], kd, vd, q_pos, md.hkv, md.D)
        worst = max(worst, R.check(attn[i * M:(i + 1) * M], ref, f"{case.id} row {i} ({p0} cached keys)"))
    assert eng.engine_status() == 0
    print(f"[kv8/attention] {case.id} {'split' if split else 'no split'}: k_scale {K_SCALE} v_scale {v_scale} worst / bound {worst:.3f}")
