"""A forward over an evicted cache (HipModel.evict_row, csrc/kv_evict.hip) against the fp32 oracle over ITS cache rolled the same
way (tests/rolling_ref.py, the bf16 rounding of the moved K included): 64 tokens forwarded, evict_row(keep 4, drop 24, n_pos 64),
one token at pos_base = 40 with logits. Undamped two-layer weights (random_init at std 0.1 and 0.2): with the default std 0.02 a
key that is moved but not rotated changes the logits by about 1 % and the test would show nothing.

The bound is the suite's one-row logits bound at toy shapes (tests/test_hip_prefill_gemm_gpu.py, test_hip_prefill_native_gpu.py:
max error < 3 % and RMS error < 1.5 % of ONE scale of the row), unchanged, with the row's max |logit| as that scale — never larger
than the logit range those tests use: max |got - want| < 3 % of the row's max |logit|, RMS(got - want) < 1.5 % of it. The planted
defect "moved, not rotated" is computed on the oracle and asserted, on the CPU side, to sit at least 10 x that bound away from the
right logits, in the maximum and in the RMS.

Not the bound of tests/test_hip_fullshape_parity_gpu.py, whose RMS clause is relative to RMS(want) and whose reference is the bf16
oracle: against the fp32 oracle no bf16 forward meets that clause on these undamped weights, evicted or not. Measured on the MI355X,
RMS(got - want) / RMS(want), in the order D=32 plain 0.1 / 0.2, D=32 llama3 0.1 / 0.2, D=128 plain 0.1 / 0.2, D=128 llama3 0.1 / 0.2:
    device        0.0149  0.0175  0.0132  0.0133  0.0219  0.0269  0.0174  0.0161
    bf16 oracle   0.0164  0.0198  0.0133  0.0127  0.0242  0.0264  0.0174  0.0211      (OracleLM(bf16) over its own rolled cache, CPU)
In the scale of this test the device's RMS error is 0.004 - 0.009 of the row's max |logit| and its max error 0.011 - 0.027; the
defect's RMS is 0.29 - 0.49 of it. Both ratios are printed by every case."""

import pytest
import torch

import rolling_ref as RR
from oracle.model_ref import OracleLM
from specdec_hip import weights as W

pytestmark = pytest.mark.gpu

LLAMA3 = {"factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 64, "rope_type": "llama3"}
N, KEEP, DROP = 64, 4, 24


def _cfg(D, scaling):
    return W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=2, d_model=4 * D, n_heads=4, n_kv_heads=2, head_dim=D, d_ff=8 * D, vocab=512,
                         max_pos=512, rope_theta=500000.0, rope_scaling=scaling, tie_embeddings=False, name=f"roll-{D}")


@pytest.mark.parametrize("std", [0.1, 0.2])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "llama3"])
@pytest.mark.parametrize("D", [32, 128])
def test_forward_after_eviction_matches_the_oracle_over_its_rolled_cache(D, scaled, std):
    from specdec_hip.engine import HipModel

    cfg = _cfg(D, LLAMA3 if scaled else None)
    mw = W.random_init(cfg, seed=1, std=std)
    lm = OracleLM(mw, "fp32")
    toks = torch.randint(4, cfg.vocab, (1, N + 1), generator=torch.Generator().manual_seed(5))
    _, past = lm.forward(toks[:, :N], need_logits=False)
    cos, sin = mw.rope_cos[DROP], mw.rope_sin[DROP]
    want = lm.forward(toks[:, N:], RR.roll_past(past, KEEP, DROP, cos, sin))[0][0, 0]
    defect = lm.forward(toks[:, N:], RR.roll_past(past, KEEP, DROP, cos, sin, rotate=False))[0][0, 0]
    top, rms = want.abs().max().item(), want.double().pow(2).mean().sqrt().item()
    d_max, d_rms = (defect - want).abs().max().item(), (defect - want).double().pow(2).mean().sqrt().item()
    print(f"[rolling forward] D={D} {'llama3' if scaled else 'plain'} std={std}: rms(logits) {rms:.3f} max|logit| {top:.3f}; "
          f"moved-not-rotated: max {d_max:.3f} rms {d_rms:.3f}")
    assert d_max >= 10 * 0.03 * top and d_rms >= 10 * 0.015 * top, (d_max, d_rms, top)    # the test can see the defect

    hm = HipModel(mw.to("cuda"), batch=2, l_max=96)
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    hm.forward(toks[:, :N].to(torch.int32).cuda(), zero, 0, skip_head=True, row0=1)
    hm.evict_row(1, KEEP, DROP, N)
    _, logits = hm.forward(toks[:, N:].to(torch.int32).cuda(), torch.tensor([N - DROP], dtype=torch.int32, device="cuda"), 0,
                           want_logits=True, row0=1)
    got = logits.float().cpu()[0, 0]
    assert torch.isfinite(got).all()
    err_rms = (got - want).double().pow(2).mean().sqrt().item()
    e_max, e_rms = (got - want).abs().max().item() / top, err_rms / top
    print(f"[rolling forward]   device: max err {e_max:.4f} and rms err {e_rms:.4f} of max|logit| (rms err {err_rms / rms:.4f} of rms(logits))")
    assert e_max < 0.03 and e_rms < 0.015, (D, scaled, std, e_max, e_rms)
