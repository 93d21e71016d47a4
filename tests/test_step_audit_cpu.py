"""The step audit of tests/step_audit.py has the power it claims: on a pure-torch stand-in for the two engines and the loop it
passes a correct step, and each of five planted protocol defects fails at least one audit item within the case's steps.

The stand-in restates the one-layer forward of oracle/model_ref.py (OracleLM, precision "bf16": fp32 arithmetic, bf16 at the
points where the kernels round) over a slot-addressed cache with the engine's layout ([1][B][Hkv][Lmax][D] keys, values
transposed), and the step protocol of csrc/spec_loop.hip in bonus emit mode: draft forward 0 in its two forms, forwards
1..K-1, one verify pass over (last, d_1..d_K), accept scan, state advance, set_row. Its products are torch's fp32 matmuls, so
the audit runs with step_audit.chain_fp32 (an fp32 sum in any order) in place of chain_hip; nothing else differs from the
device audit and no tolerance is fitted. The norm statistic is taken in fp64 (inside the 2^-20 the bounds allow a kernel).
Sequences stay below 64 positions, where stage_ref's allowance for the PV sum (S / 32 + 64) covers an fp32 sum in any order."""

import math
import types

import numpy as np
import pytest
import torch

import step_audit as A
from specdec_hip import weights as W
from specdec_hip.engine import HipModel

CFG = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=1, d_model=256, n_heads=4, n_kv_heads=2, head_dim=64, d_ff=512, vocab=512,
                    max_pos=4096, rope_theta=500000.0, rope_scaling=None, tie_embeddings=False, name="toy-d64")

DEFECTS = {
    "draft_row_late": "a draft K/V row written one position late",
    "one_token_fwd0_after_full_accept": "the 1-token form of forward 0 taken after a == K",
    "stale_key_visible": "one stale key visible to query m = 0",
    "rejected_row_kept": "a rejected verify row kept instead of overwritten",
    "set_row_keeps_length": "set_row not lowering the visible length",
}


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


class TorchEngine:
    """one-layer Llama forward over a slot-addressed cache, with the reading surface stage_check asks of an engine"""

    def __init__(self, mw, batch, l_max):
        c = self.cfg = mw.config
        self.weights, self.device, self.page_len = mw, torch.device("cpu"), None
        self.k = torch.zeros(1, batch, c.n_kv_heads, l_max, c.head_dim, dtype=torch.bfloat16)
        self.v = torch.zeros(1, batch, c.n_kv_heads, c.head_dim, l_max, dtype=torch.bfloat16)
        self.high = [0] * batch          # one past the highest slot written per row (rejected_row_kept)
        self.taps = {}

    def kv_view(self):
        return self.k, self.v

    def reserve(self, row, length, stream=None):
        pass

    def hidden_rows(self, n):
        return self.taps[HipModel.DEBUG_X][:n]

    def debug_rows(self, which, n):
        return self.taps[which][:n]

    def _rms(self, x, w):
        rs = 1.0 / torch.sqrt(x.double().pow(2).mean(-1, keepdim=True) + self.cfg.norm_eps)
        return _bf((x.double() * rs).to(torch.bfloat16).float() * w.float())

    def forward(self, tokens, pos_base, pos_off=0, skip_head=False, row0=0, slot_shift=0, see_next=False, keep_written=False):
        """tokens [B][M] at positions pos_base[b] + pos_off + m of rows row0 + b -> bf16 logits [B][M][V]. The defects:
        slot_shift — K / V stored that many slots late; see_next — query m = 0 also sees the key one past its own;
        keep_written — a slot that already holds a row is not overwritten"""
        c, mw = self.cfg, self.weights
        lw = mw.layers[0]
        Hq, Hkv, D = c.n_heads, c.n_kv_heads, c.head_dim
        B, M = tokens.shape
        pos = (pos_base.long().view(B, 1) + pos_off + torch.arange(M).view(1, M))          # [B][M]
        x0 = mw.tok_emb[tokens.long()].float()
        qkv = self._rms(x0, lw.attn_norm_w) @ lw.wqkv.float().t()
        cos, sin = mw.rope_cos[pos].unsqueeze(2), mw.rope_sin[pos].unsqueeze(2)            # [B][M][1][D/2]

        def rope(t):
            a, b = t[..., : D // 2], t[..., D // 2:]
            return torch.cat([a * cos - b * sin, b * cos + a * sin], -1)

        q = _bf(rope(qkv[..., : Hq * D].view(B, M, Hq, D)))
        k = _bf(rope(qkv[..., Hq * D:(Hq + Hkv) * D].view(B, M, Hkv, D)))
        v = _bf(qkv[..., (Hq + Hkv) * D:].view(B, M, Hkv, D))
        o = torch.zeros(B, M, Hq * D)
        for b in range(B):
            r = row0 + b
            for m in range(M):
                s = int(pos[b, m]) + slot_shift
                if keep_written and s < self.high[r]:
                    continue
                self.k[0, r, :, s] = k[b, m].to(torch.bfloat16)
                self.v[0, r, :, :, s] = v[b, m].to(torch.bfloat16)
            self.high[r] = max(self.high[r], int(pos[b, -1]) + slot_shift + 1)
            S = int(pos[b, -1]) + 2
            kk, vv = self.k[0, r, :, :S].float(), self.v[0, r, :, :, :S].float().transpose(1, 2)      # [Hkv][S][D]
            qh = q[b].view(M, Hkv, Hq // Hkv, D)
            att = torch.einsum("mhgd,hsd->mhgs", qh, kk) / math.sqrt(D)
            vis = torch.arange(S).view(1, S) <= pos[b].view(M, 1)
            if see_next:
                vis[0, int(pos[b, 0]) + 1] = True
            att = torch.softmax(att.masked_fill(~vis.view(M, 1, 1, S), float("-inf")), -1)
            o[b] = _bf(torch.einsum("mhgs,hsd->mhgd", att, vv).reshape(M, Hq * D))
        x1 = _bf(x0 + o @ lw.wo.float().t())
        up = self._rms(x1, lw.mlp_norm_w) @ lw.w_up.float().t()
        g, u = up[..., : c.d_ff], up[..., c.d_ff:]
        act = _bf(g / (1.0 + torch.exp(-g)) * u)
        x2 = _bf(x1 + act @ lw.w_down.float().t())
        self.taps = {HipModel.DEBUG_Q: q.reshape(B * M, -1).bfloat16(), HipModel.DEBUG_ATTN: o.reshape(B * M, -1).bfloat16(),
                     HipModel.DEBUG_ACT: act.reshape(B * M, -1).bfloat16(), HipModel.DEBUG_X: x2.reshape(B * M, -1).bfloat16()}
        if skip_head:
            return None, None
        return None, (self._rms(x2, mw.final_norm_w) @ mw.lm_head.float().t()).to(torch.bfloat16)


class TorchSpecDec:
    """the step protocol over two TorchEngines; `defect`: one of DEFECTS, or None"""

    def __init__(self, draft, target, B, K, defect=None):
        assert defect is None or defect in DEFECTS
        self.draft, self.target, self.B, self.K, self.defect = draft, target, B, K, defect
        self.cur = torch.zeros(B, dtype=torch.int32)
        self.tok2 = torch.zeros(B, 2, dtype=torch.int32)
        self.active = [True] * B
        self.two = True                  # B == 1: the device-selected form of the next forward 0; B > 1: always the 2-token form
        self.step_logits = None
        self.rec = None

    def join_current_stream(self):
        pass

    def set_row(self, b, seq_len, prev_tok, last_tok, active=True):
        keep = self.defect == "set_row_keeps_length" and seq_len - 1 < int(self.cur[b])
        if not keep:
            self.cur[b] = seq_len - 1
        self.tok2[b, 0], self.tok2[b, 1] = prev_tok, last_tok
        self.active[b] = bool(active)
        self.two = True

    def step(self, use_graph=True, two_streams=True):
        B, K = self.B, self.K
        d = torch.zeros(B, K, dtype=torch.int32)
        if self.two or B > 1:
            _, lg = self.draft.forward(self.tok2, self.cur, -1)
        else:
            _, lg = self.draft.forward(self.tok2[:, 1:], self.cur, 0)
        d[:, 0] = A._first_argmax(lg[:, -1])
        for i in range(1, K):
            _, lg = self.draft.forward(d[:, i - 1:i], self.cur, i, slot_shift=1 if self.defect == "draft_row_late" else 0)
            d[:, i] = A._first_argmax(lg[:, -1])
        vt = torch.cat([self.tok2[:, 1:], d], 1)
        _, lg = self.target.forward(vt, self.cur, 0, see_next=self.defect == "stale_key_visible",
                                    keep_written=self.defect == "rejected_row_kept")
        self.step_logits = lg
        t = A._first_argmax(lg).to(torch.int32)                                              # [B][K+1]
        rec = types.SimpleNamespace(accept_len=np.zeros(B, np.int32), n_new=np.zeros(B, np.int32), cur_len=np.zeros(B, np.int32),
                                    new_tokens=np.full((B, K + 1), -1, np.int32), draft_tokens=d.numpy().copy(),
                                    target_ids=t.numpy().copy(), engine_status=0)
        for b in range(B):
            a = next((i for i in range(K) if int(t[b, i]) != int(d[b, i])), K)
            rec.accept_len[b], rec.n_new[b] = a, a + 1
            rec.new_tokens[b, :a + 1] = t[b, :a + 1].numpy()
            if self.active[b]:
                self.tok2[b, 0] = t[b, a - 1] if a >= 1 else self.tok2[b, 1]
                self.tok2[b, 1] = t[b, a]
                self.cur[b] += a + 1
            if b == 0:
                self.two = (not self.active[b]) or (a >= K and self.defect != "one_token_fwd0_after_full_accept")
            rec.cur_len[b] = int(self.cur[b])
        self.rec = rec

    def sync(self):
        return self.rec


_W = {}


def _pair(fraction):
    if "t" not in _W:
        _W["t"] = W.random_init(CFG, seed=7, device="cpu")
    if fraction not in _W:
        _W[fraction] = A.rolled_draft(_W["t"], fraction, seed=5)
    return _W[fraction], _W["t"]


def _run(B, K, fraction, defect, stored, steps=8, lengths=(16, 2, 9), script=None):
    """`steps` audited steps of a stand-in loop; script: {step index: lambda audit} run before that step. -> the audit"""
    dw, tw = _pair(fraction)
    draft, target = TorchEngine(dw, B, 128), TorchEngine(tw, B, 128)
    loop = TorchSpecDec(draft, target, B, K, defect)
    audit = A.StepAudit(loop, draft, target, dw, tw, chain=A.chain_fp32, what=f"stand-in B={B} K={K} {defect or 'correct'}",
                        fwd0_select=B == 1, stored=stored)
    g = torch.Generator().manual_seed(11)
    audit.start([torch.randint(4, CFG.vocab, (n,), generator=g).tolist() for n in lengths[:B]], reach=steps * (K + 1) + 2)
    for s in range(steps):
        if script and s in script:
            script[s](audit)
        audit.step()
    assert max(audit.pos_last) + K + 1 <= 64, "keep the stand-in's sequences below 64 positions (see the module docstring)"
    return audit


def _host_script(audit):
    audit.cut(1, 3)


SCRIPT = {3: _host_script, 5: lambda audit: audit.deactivate(2)}


@pytest.mark.parametrize("B,K,fraction,stored", [(1, 4, 0.3, False), (1, 1, 0.3, True), (1, 3, 0.0, True), (3, 4, 0.3, True), (3, 2, 0.0, False)])
def test_audit_passes_a_correct_step(B, K, fraction, stored):
    audit = _run(B, K, fraction, None, stored, script=SCRIPT if B == 3 else None)
    assert audit.steps == 8 and all(r <= 1.0 for r in audit.worst.values()), audit.worst
    if fraction == 0.0:
        assert set(audit.accept_hist) == {K} and audit.hole_fills >= 7 * (B - (1 if B == 3 else 0)) - 1
        assert B > 1 or audit.forms[2] == 8
    elif B == 1 and K == 4:
        assert audit.forms[1] >= 1 and audit.forms[2] >= 1, "both forms of forward 0 are to be taken"
    print(f"[audit] B={B} K={K} roll {fraction}: accept lengths {dict(sorted(audit.accept_hist.items()))}, hole fills {audit.hole_fills}, "
          f"forms {dict(audit.forms)}, worst " + " ".join(f"{i}:{r:.3f}" for i, r in audit.worst.items()))


# (B, K, rolled fraction, host script) under which each defect acts within 8 steps, and the items that may catch it
PLANTED = {
    "draft_row_late": (1, 4, 0.3, None, {4, 5}),
    "one_token_fwd0_after_full_accept": (1, 3, 0.0, None, {4}),
    "stale_key_visible": (1, 4, 0.3, None, {3}),
    "rejected_row_kept": (1, 4, 0.3, None, {2, 3}),
    "set_row_keeps_length": (3, 4, 0.3, SCRIPT, {1}),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_each_planted_defect_fails_the_audit(defect):
    B, K, fraction, script, items = PLANTED[defect]
    caught = None
    try:
        _run(B, K, fraction, defect, True, script=script)
    except A.AuditFailure as e:
        caught = e
    assert caught is not None, f"planted defect passed the audit unnoticed: {DEFECTS[defect]}"
    assert caught.item in items, f"planted defect ({DEFECTS[defect]}) was caught by item {caught.item}, expected one of {sorted(items)}: {caught}"
    print(f"[audit] planted: {DEFECTS[defect]} -> {str(caught)[:240]}")
