"""sliding_window through the public interface: a greedy generate_batch of a synthetic pair (head_dim 64) under a 64-key window, prompts
longer than the window and enough new tokens to cross several key blocks, repeats token for token and equals the target's own greedy
decoding on a windowed HipLM; both engines stay off the persistent forward; context_window is refused by name."""

import pytest
import torch

from specdec_hip import weights as W

pytestmark = pytest.mark.gpu

TARGET = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=3, d_model=128, n_heads=2, n_kv_heads=1, head_dim=64, d_ff=256, vocab=1000, max_pos=512,
                       rope_theta=500000.0, tie_embeddings=False, name="window-target")
DRAFT = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=2, d_model=64, n_heads=1, n_kv_heads=1, head_dim=64, d_ff=128, vocab=1000, max_pos=512,
                      rope_theta=500000.0, tie_embeddings=False, name="window-draft")
PROMPTS = [torch.randint(4, 1000, (n,), generator=torch.Generator().manual_seed(n)).tolist() for n in (70, 130)]


def test_greedy_generate_batch_repeats_and_equals_the_targets_own_decoding():
    from src.specdec import HipLM, SpeculativePipeline

    tgt = W.synthetic_llama(TARGET, seed=0, device="cpu", layer_gain=0.05)
    drf = W.synthetic_llama(DRAFT, seed=1, device="cpu", layer_gain=0.05, embed_from=tgt, flip_fraction=0.25)
    pair = HipLM(tgt.to("cuda"), sliding_window=64), HipLM(drf.to("cuda"), sliding_window=64)
    pipe = SpeculativePipeline(base_lm=pair[0], draft_lm=pair[1], controller="fixed", controller_params={"k": 4}, seed=1234)
    got = pipe.generate_batch(PROMPTS, max_tokens=80, do_sample=False)
    again = pipe.generate_batch(PROMPTS, max_tokens=80, do_sample=False)
    engines = [e for rt in pipe._runtimes.values() for e in (rt["target"], rt["draft"])]
    assert engines and all(e.sliding_window == 64 and not e.persist_active(1) and e.persist_tokens == 0 for e in engines)
    alone = HipLM(pair[0].weights, sliding_window=64)
    for p, g, a in zip(PROMPTS, got, again):
        assert g["generated_tokens"] == a["generated_tokens"] and len(g["generated_tokens"]) >= 72
        want, _ = alone.generate_tokens(torch.tensor([p]), len(g["generated_tokens"]), do_sample=False)
        assert g["generated_tokens"] == want[0].tolist()
    with pytest.raises(NotImplementedError, match="sliding_window"):
        pipe.generate_batch(PROMPTS[:1], max_tokens=8, do_sample=False, context_window=256)
