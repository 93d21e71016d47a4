"""The captured speculative step (csrc/spec_loop.hip) audited against fp64 on one-layer `random_init` models, not damped.

The kernels of a forward are checked pass by pass elsewhere (tests/test_hip_stage_fp64_gpu.py and its family). This file
checks the PROTOCOL the step builds out of those passes — both forms of draft forward 0 and who picks one, the positions of
forwards 1..K-1, the verify pass and the K + 1 cache rows it writes, the stale rows above the new length, the draft-cache hole
after a fully accepted step, set_row after a host cut — with tests/step_audit.py: it follows the device's own records and
audits the state they imply (items 1-5 there), every error as a fraction of a bound of tests/stage_ref.py with R.chain_hip.
It never compares tokens with an oracle's, so an argmax near-tie cannot fail it.

Target: TOY (TOY128 in one case) of the stage tests, seed 7, drawn on the host. Draft: the same weights with a seeded 30 % of
the lm_head rows rolled among themselves (ROLL_SEED per K), or unmodified (every step fully accepted). The loop's draft
stores its stage rows (SPECDEC_PERSIST_TAPS at its creation) but in the one case that says otherwise. Run with -s for the
[stage/bound] lines of every step; profiles/step_fp64_audit.md tabulates them."""

import random

import pytest
import torch

import stage_ref as R
import step_audit as A
from specdec_hip import weights as W
from specdec_hip.engine import HipModel, HipSpecDec
from test_hip_stage_fp64_gpu import TOY, TOY128

pytestmark = pytest.mark.gpu

FRACTION = 0.30
ROLL_SEED = {1: 5, 2: 5, 3: 5, 4: 6, 8: 5}      # per K: under it the two greedy cases of that K visit every accept length 0..K
LENGTHS = [2, 30, 31, 33]                        # ragged starts: the steps cross the 32-key block edge inside the replayed graph
KS = [1, 2, 3, 4, 8]

_PAIRS = {}
_DONE = {}


def _pair(cfg, fraction, seed):
    """(draft weights, target weights) on the device, one copy per (config, fraction, seed)"""
    if cfg.name not in _PAIRS:
        _PAIRS[cfg.name] = W.random_init(cfg, seed=7, device="cpu").to("cuda")
    key = (cfg.name, fraction, seed)
    if key not in _PAIRS:
        _PAIRS[key] = A.rolled_draft(_PAIRS[cfg.name], fraction, seed)
    return _PAIRS[key], _PAIRS[cfg.name]


def _prompts(lengths, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(4, vocab, (n,), generator=g).tolist() for n in lengths]


def _lengths(B, K):
    i = KS.index(K) if K in KS else 0
    return [LENGTHS[(i + j + (1 if B == 1 else 0)) % 4] for j in range(B)]


def _audit(monkeypatch, name, B, K, steps, lengths, cfg=TOY, fraction=FRACTION, l_max=256, page_len=None, backend="auto",
           draft_launch=False, taps=True, mode=None, step_kw=None, script=None):
    """one case: engines, loop, `steps` audited steps (script: {step index: lambda audit}, run before that step) -> the audit,
    with the paths the step took"""
    dw, tw = _pair(cfg, fraction, ROLL_SEED.get(K, 5))
    if taps:
        monkeypatch.setenv("SPECDEC_PERSIST_TAPS", "1")
    else:
        monkeypatch.delenv("SPECDEC_PERSIST_TAPS", raising=False)
    target = HipModel(tw, batch=B, l_max=l_max, page_len=page_len, prefill_backend=backend)
    draft = HipModel(dw, batch=B, l_max=l_max, page_len=page_len, prefill_backend=backend)
    if page_len is not None:            # pages handed out in a scrambled order, differently for the two models
        random.Random(B * 100 + K).shuffle(target._free)
        random.Random(B * 100 + K + 1).shuffle(draft._free)
    if draft_launch:
        draft.set_persist_tokens(0)
    loop = HipSpecDec(draft, target, B, K, HipSpecDec.EMIT_BONUS)
    if mode == "logprobs":
        loop.set_logprobs(0)
    elif mode == "processors":
        loop.set_logit_processors(True)
    persistent = draft.persist_active(1) and draft.persist_active(2) and B == 1
    select = persistent
    stored = mode is not None
    tail = not stored and B * (K + 1) <= target.pass_tokens
    audit = A.StepAudit(loop, draft, target, dw, tw, chain=R.chain_hip, what=name, fwd0_select=select, stored=stored,
                        draft_taps=taps or not persistent)
    audit.paths = dict(draft="persistent" if persistent else "launch", select=select,
                       verify="persistent" if (B == 1 and target.persist_active(K + 1)) else "launch",
                       tail="tail" if tail else "three launches", taps=audit.draft_taps,
                       n_split=max(1, target.l_max // 512))     # launch_attention: one split per 512 keys of the cache

    audit.start(_prompts(lengths, cfg.vocab, 100 * K + B), reach=steps * (K + 1) + 2)
    for s in range(steps):
        if script and s in script:
            script[s](audit)
        audit.step(**(step_kw or {}))
    assert all(r <= 1.0 for r in audit.worst.values()), audit.worst
    print(f"[audit] {name}: paths {audit.paths}, accept lengths {dict(sorted(audit.accept_hist.items()))}, hole fills {audit.hole_fills}, "
          f"forward-0 forms {dict(audit.forms)}, worst " + " ".join(f"{A.ITEMS[i]} {r:.3f}" for i, r in audit.worst.items()))
    loop.close()
    return audit


def _greedy(monkeypatch, K, B):
    """the greedy case (K, B) under the captured graph, run once per session: the coverage test reads what it left"""
    if (K, B) not in _DONE:
        _DONE[(K, B)] = _audit(monkeypatch, f"greedy K={K} B={B}", B, K, 16 if K == 8 else 14, _lengths(B, K))
    return _DONE[(K, B)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", KS)
def test_greedy_step(K, B, monkeypatch):
    a = _greedy(monkeypatch, K, B)
    assert a.paths["tail"] == "tail"
    if B == 1:          # the persistent draft and the device-selected forward 0: both forms are to be taken
        assert a.paths["draft"] == "persistent" and a.paths["select"], a.paths
        assert a.forms[1] >= 1 and a.forms[2] >= 1, a.forms
    else:
        assert a.paths["draft"] == "launch" and a.forms[1] == 0


@pytest.mark.parametrize("K", KS)
def test_accept_lengths_cover_every_value(K, monkeypatch):
    """what keeps the audit from hiding a failure: over the two greedy cases of one K every accept length 0..K occurs, and the
    a == K -> next-step check of item 4 (the hole filled) ran at least twice"""
    hist, fills = {}, 0
    for B in (1, 3):
        a = _greedy(monkeypatch, K, B)
        fills += a.hole_fills
        for k, v in a.accept_hist.items():
            hist[k] = hist.get(k, 0) + v
    print(f"[audit] K={K} roll seed {ROLL_SEED[K]}: accept lengths {dict(sorted(hist.items()))}, hole fills {fills}")
    assert sorted(hist) == list(range(K + 1)), f"K={K}: accept lengths {sorted(hist)} visited, want every one of 0..{K} (change ROLL_SEED[{K}])"
    assert fills >= 2, fills


def test_greedy_step_without_graph(monkeypatch):
    _audit(monkeypatch, "greedy K=4 B=3 eager", 3, 4, 12, [33, 2, 30], step_kw=dict(use_graph=False))


def test_greedy_step_on_one_stream(monkeypatch):
    _audit(monkeypatch, "greedy K=4 B=1 one stream", 1, 4, 12, [31], step_kw=dict(two_streams=False))


def test_draft_without_stage_row_stores(monkeypatch):
    """the draft's persistent instantiation WITHOUT the stage-row stores, as a loop outside this file runs it (item 5 needs the
    taps: items 1-4 only)"""
    a = _audit(monkeypatch, "greedy K=4 B=1 draft taps off", 1, 4, 12, [33], taps=False)
    assert a.paths["draft"] == "persistent" and not a.paths["taps"] and a.hole_fills >= 2


def test_draft_on_the_launch_path(monkeypatch):
    a = _audit(monkeypatch, "greedy K=4 B=1 draft on launches", 1, 4, 12, [30], draft_launch=True)
    assert a.paths["draft"] == "launch" and not a.paths["select"] and a.forms[1] == 0


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("mode", ["logprobs", "processors"])
def test_stored_logits(mode, B, monkeypatch):
    """set_logprobs(0): the three launches, rows stored; identity logit processors: HAND_NEXT, rows processed in place. The
    stored rows against the head stage, target_ids the first argmax of the stored row"""
    a = _audit(monkeypatch, f"{mode} K=4 B={B}", B, 4, 12, _lengths(B, 4), mode=mode)
    assert a.paths["tail"] == "three launches"


@pytest.mark.parametrize("page_len", [None, 32], ids=["dense", "page32"])
def test_split_threshold(page_len, monkeypatch):
    """rows at 505 and 509 keys in caches of 1088: the attention launch carries two splits, and a row's second one starts
    to count inside the captured replay as the row passes 512 keys; paged: pages of 32 from a shuffled free list, page edges
    crossed at 512 and 544"""
    a = _audit(monkeypatch, f"split K=4 B=2 {'dense' if page_len is None else 'paged'}", 2, 4, 12, [505, 509], l_max=1088,
               page_len=page_len, backend="native")
    assert min(a.pos_last) > 520


@pytest.mark.parametrize("K", [4, 8])
def test_identity_draft(K, monkeypatch):
    """the unmodified copy: every step is fully accepted (but for a near-tie between two kernels' sums), so the hole and the
    2-token forward 0 are audited on every step"""
    a = _audit(monkeypatch, f"identity K={K} B=1", 1, K, 12, [31], fraction=0.0)
    assert a.paths["select"] and a.hole_fills >= 2, (a.paths, a.hole_fills)


def test_host_cut_and_inactive_row(monkeypatch):
    """after step 6 the host commits three tokens fewer of row 1 than the device emitted (set_row): the stale rows above the
    cut are never visible (item 3: attention from the positions <= the query's own) and are overwritten (items 2, 4: every
    slot holds what the protocol last put there); after step 9 row 2 goes inactive: its committed rows and cur_len stay"""
    seen = {}

    def cut(audit):
        seen["cut"] = audit.pos_last[1]
        audit.cut(1, 3)

    def stop(audit):
        seen["stop"] = audit.pos_last[2]
        audit.deactivate(2)

    a = _audit(monkeypatch, "host cut K=4 B=3", 3, 4, 14, [30, 31, 33], script={6: cut, 9: stop})
    assert a.pos_last[2] == seen["stop"]
    assert a.pos_last[1] > seen["cut"], "row 1 is to pass its old length again: every stale row overwritten"


def test_head_dim_128(monkeypatch):
    _audit(monkeypatch, "toy-d128 K=4 B=1", 1, 4, 12, [30], cfg=TOY128)
