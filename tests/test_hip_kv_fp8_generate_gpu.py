"""kv_cache_dtype="fp8" through the public interface: a greedy generate_batch of a synthetic pair (head_dim 64) over e4m3 caches
repeats token for token and equals the target's own greedy decoding on an fp8-KV HipLM (token ids identical, the comparison of
tests/test_hip_pipeline_gpu.py); both engines stay off the persistent forward; and what an e4m3 cache does not serve is refused
with a message that names the KV dtype."""

import pytest
import torch

import attention_cases as A
from specdec_hip import weights as W
from specdec_hip.engine import HipModel
from test_hip_attention_geometry_gpu import _weights

pytestmark = pytest.mark.gpu

TARGET = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=3, d_model=128, n_heads=2, n_kv_heads=1, head_dim=64, d_ff=256, vocab=1000, max_pos=512,
                       rope_theta=500000.0, tie_embeddings=False, name="kv8-target")
DRAFT = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=2, d_model=64, n_heads=1, n_kv_heads=1, head_dim=64, d_ff=128, vocab=1000, max_pos=512,
                      rope_theta=500000.0, tie_embeddings=False, name="kv8-draft")


@pytest.fixture(scope="module")
def pair():
    from src.specdec import HipLM

    tgt = W.synthetic_llama(TARGET, seed=0, device="cpu", layer_gain=0.05)
    drf = W.synthetic_llama(DRAFT, seed=1, device="cpu", layer_gain=0.05, embed_from=tgt, flip_fraction=0.25)
    return HipLM(tgt.to("cuda")), HipLM(drf.to("cuda"))


def _pipe(pair, **kw):
    from src.specdec import SpeculativePipeline

    return SpeculativePipeline(base_lm=pair[0], draft_lm=pair[1], controller="fixed", controller_params={"k": 4}, seed=1234,
                               kv_cache_dtype="fp8", **kw)


PROMPTS = [torch.randint(4, 1000, (n,), generator=torch.Generator().manual_seed(n)).tolist() for n in (40, 130)]


def test_greedy_generate_batch_repeats_and_equals_the_targets_own_decoding(pair):
    from src.specdec import HipLM

    pipe, prompts = _pipe(pair), PROMPTS
    assert pair[0].kv_cache_dtype == pair[1].kv_cache_dtype == "fp8"
    got = pipe.generate_batch(prompts, max_tokens=48, do_sample=False)
    again = pipe.generate_batch(prompts, max_tokens=48, do_sample=False)
    engines = [e for rt in pipe._runtimes.values() for e in (rt["target"], rt["draft"])]
    assert engines and all(e.kv_dtype == "fp8" and not e.persist_active(1) and e.persist_tokens == 0 for e in engines)
    alone = HipLM(pair[0].weights, kv_dtype="fp8")
    for p, g, a in zip(prompts, got, again):
        assert g["generated_tokens"] == a["generated_tokens"] and len(g["generated_tokens"]) >= 40
        want, _ = alone.generate_tokens(torch.tensor([p]), len(g["generated_tokens"]), do_sample=False)
        assert g["generated_tokens"] == want[0].tolist()
    kv = alone.get_kv_cache()
    assert kv.dtype == torch.bfloat16 and kv.past_key_values[0][0].dtype == torch.bfloat16 and bool(kv.past_key_values[0][0].any())


def test_refusals_name_the_kv_dtype(pair):
    pipe, prompts = _pipe(pair), PROMPTS
    with pytest.raises(RuntimeError, match="kv_cache_dtype fp8"):
        pipe.generate_batch([prompts[0], prompts[0]], max_tokens=8, do_sample=False, share_prefix=True)
    with pytest.raises(NotImplementedError, match="kv_cache_dtype fp8"):
        pipe.generate_batch(prompts[:1], max_tokens=8, do_sample=False, context_window=256)
    mw = _weights(A.EDGE)
    with pytest.raises(ValueError, match="kv_cache_dtype fp8"):
        HipModel(mw, batch=1, l_max=128, kv_dtype="fp8", page_len=32)
    eng = HipModel(mw, batch=2, l_max=128, kv_dtype="fp8")
    for call in (lambda: eng.fork_row(0, [1], 8), lambda: eng.evict_row(0, 4, 8, 64), lambda: eng.set_kv_dtype("bf16")):
        with pytest.raises(RuntimeError, match="(?i)kv.?(cache.?)?dtype"):
            call()
    with pytest.raises(RuntimeError, match="kv dtype.*head_dim"):
        HipModel(_weights(A.MAXS), batch=1, l_max=128, kv_dtype="fp8")     # head_dim 32
