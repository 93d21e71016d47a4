"""cascade_attention=True through the public interface, on a tiny synthetic pair with cascade_min_shared lowered to one key block.

Greedy ties on synthetic weights may flip between the cascade merge order and the plain one, so token equality with the un-cascaded
run is not asserted: every emitted token must be within the target's own top-2 at its position, under a plain (cascade off)
score_logits of the finished sequence."""

import pytest
import torch

from specdec_hip import weights as W
from specdec_hip.engine import HipModel

pytestmark = pytest.mark.gpu

TARGET = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=3, d_model=128, n_heads=2, n_kv_heads=1, head_dim=64, d_ff=256, vocab=1000, max_pos=512,
                       rope_theta=500000.0, tie_embeddings=False, name="cascade-target")
DRAFT = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=2, d_model=64, n_heads=1, n_kv_heads=1, head_dim=64, d_ff=128, vocab=1000, max_pos=512,
                      rope_theta=500000.0, tie_embeddings=False, name="cascade-draft")


@pytest.fixture(scope="module")
def pair():
    from src.specdec import HipLM

    tgt = W.synthetic_llama(TARGET, seed=0, device="cpu", layer_gain=0.05)
    drf = W.synthetic_llama(DRAFT, seed=1, device="cpu", layer_gain=0.05, embed_from=tgt, flip_fraction=0.25)
    return HipLM(tgt.to("cuda")), HipLM(drf.to("cuda"))


def _pipe(pair):
    from src.specdec import SpeculativePipeline

    pipe = SpeculativePipeline(base_lm=pair[0], draft_lm=pair[1], controller="fixed", controller_params={"k": 4}, seed=1234)
    pipe.config["cascade_min_shared"] = 32
    return pipe


def _ids(n, seed):
    return torch.randint(4, 1000, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


def _within_top2(pair, results, prompts):
    plain = pair[0].new_engine(1, 512, cascade=False)
    for r, p in zip(results, prompts):
        seq, n0 = r["sequence"], len(p)
        assert seq[:n0] == list(p) and seq[n0:] == r["generated_tokens"] and len(seq) > n0 + 8
        logits, _ = plain.score_logits(seq)
        top2 = logits[n0 - 1:len(seq) - 1].float().topk(2, dim=-1).indices.tolist()
        assert all(t in two for t, two in zip(seq[n0:], top2)), "an emitted token is outside the target's top-2"


def _cascade_targets(pipe):
    engines = [rt["target"] for key, rt in pipe._runtimes.items() if "cascade" in key]
    assert engines and all(e.cascade and not e.persist_active(1) and e.engine_status() == 0 for e in engines)
    return engines


def test_generate_batch_n4_forms_a_group(pair):
    pipe, prompt = _pipe(pair), _ids(200, 3)
    rs = pipe.generate_batch([prompt], max_tokens=24, do_sample=False, n=4, share_prefix=True, cascade_attention=True)
    bm = rs[0]["batch_metrics"]
    assert bm["forked_rows"] == 3 and bm["cascade_rows"] == 3 and bm["cascade_positions"] == 3 * 192      # floor32(199) each
    _cascade_targets(pipe)
    _within_top2(pair, rs, [prompt] * 4)
    off = pipe.generate_batch([prompt], max_tokens=8, do_sample=False, n=2)                               # the mode is per call
    assert off[0]["batch_metrics"]["cascade_rows"] == 0


def test_generate_many_hands_a_roots_slot_to_a_new_prompt(pair):
    """3 slots, 6 prompts behind one 160-token system prompt: slot 0 leads the first group; when the first rows end, slot 0 is
    the first to be re-admitted, while the table still names it the leader of slots 1 and 2 — the group passes to slot 1 before
    slot 0's cache is rewritten, and the later admissions form a new group behind slot 0's new prompt."""
    pipe, system = _pipe(pair), _ids(160, 5)
    prompts = [system + _ids(8 + i, 20 + i) for i in range(6)]
    rs = pipe.generate_many(prompts, max_tokens=16, batch_size=3, do_sample=False, share_prefix=True, cascade_attention=True)
    bm = rs[0]["batch_metrics"]
    assert bm["cascade_rows"] >= 4 and bm["cascade_positions"] == 160 * bm["cascade_rows"], bm
    _cascade_targets(pipe)
    _within_top2(pair, rs, prompts)


def test_refusals_on_engines_and_sessions(pair):
    pipe, prompt = _pipe(pair), _ids(64, 7)
    with pytest.raises(ValueError, match="share_prefix"):
        pipe.generate_batch([prompt], max_tokens=4, cascade_attention=True)
    with pytest.raises(NotImplementedError, match="context_window"):
        pipe.generate_batch([prompt], max_tokens=4, n=2, cascade_attention=True, context_window=256)
    with pytest.raises(NotImplementedError, match="generate\\(\\)"):
        pipe.generate(prompt, max_tokens=4, cascade_attention=True)
    with pytest.raises(ValueError, match="share_prefix"):
        pipe.start_session([prompt, prompt], 4, 1, cascade_attention=True)
    eng = HipModel(pair[0].weights, batch=2, l_max=128, cascade=True)
    with pytest.raises(RuntimeError, match="cascade"):
        eng.evict_row(0, 4, 8, 64)
    for args, word in (((1, 0, 48), "multiple of 32"), ((1, 2, 32), "outside"), ((1, 0, 0), "own leader")):
        with pytest.raises(RuntimeError, match=word):
            eng.set_shared_prefix(*args)
    eng.set_shared_prefix(1, 0, 64)
    with pytest.raises(RuntimeError, match="still names"):
        eng.set_shared_prefix(0, 0, 0)            # a row that members name stays a root
    with pytest.raises(RuntimeError, match="cascade=True"):
        HipModel(pair[0].weights, batch=1, l_max=128).set_shared_prefix(0, 0, 0)
