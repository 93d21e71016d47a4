"""Audit of the draft-then-verify step (csrc/spec_loop.hip) against fp64, on one-layer `random_init` models (test
infrastructure: no conftest; tests/test_hip_step_fp64_gpu.py runs it on the device, tests/test_step_audit_cpu.py shows on a
pure-torch stand-in that it passes a correct step and fails five planted protocol defects).

The audit never compares the device's tokens with an oracle's: it follows the device's own choices (the step record) and
checks the state they imply. With ONE layer the K / V row of a position is a function of the token there and the position
alone (R.embed, then R.qkv_stage), so every cache row can be recomputed in fp64 from a token sequence, and every bound is
that of tests/stage_ref.py. After every synchronised step:

 1. record consistency   cur_len = previous cur_len + n_new (unchanged for an inactive row); accept_len = the longest prefix
                         with target_ids[i] == draft_tokens[i]; n_new = accept_len + 1; new_tokens = target_ids[:accept_len + 1];
                         engine_status 0.
 2. target cache         EVERY slot the protocol has written so far holds the fp64 K / V of the token the protocol put there,
                         at every step (a late overwrite shows): the prompt, the committed tokens, and above them the stale
                         rows of rejected drafts until a later pass overwrites them. Positions [0, pos_last) are those of the
                         committed sequence (asserted on the host, from the model of the slots).
 3. verify pass          the stage checks (stage_check.check_pass: q, new K / V rows, attention from the DEVICE's cache at the
                         positions <= the query's own and no others, activation, residual) over the B (K + 1) rows of the pass:
                         tokens (last, d_1..d_K) at pos_last + m. Stored rows (step_logits): the logits too, and target_ids is
                         the first argmax of the stored row. Not stored (the fused tail): target_ids by R.check_head_argmax from
                         the residual tap — no other logit can have been the larger one within the bound (a tie cannot fail it;
                         the tail exposes no value, so the value clause is given the reference itself).
 4. draft cache          as 2, for the slots the draft forwards wrote: (prev,) last, d_1..d_{K-1} at pos_last (- 1) + i. Every
                         position below the new `prev` is that of its committed token; the new `prev` itself see
                         prev_in_draft_cache.
 5. last draft forward   the stage checks over the draft's taps: forward K - 1 (one token d_{K-1} per row at pos_last + K - 1),
                         or forward 0 when K = 1 (the 2-token form over (prev, last), or the 1-token form over last); d_K by
                         R.check_head_argmax from its residual tap (the draft's rows do not survive a step: where they are
                         stored at all, the verify pass overwrites them).

Positions: `pos_last` is the device's cur_len, the position of `last` (sequence length - 1); its K / V are not in a cache
until the next step writes them."""

from __future__ import annotations

import collections
import dataclasses
from typing import Dict, List, Optional, Sequence

import torch

import stage_ref as R
from stage_check import cache_rows, check_pass, matrices

ITEMS = {1: "record consistency", 2: "target cache", 3: "verify pass", 4: "draft cache", 5: "last draft forward"}


def chain_fp32(K: int) -> float:
    """term 2 of stage_ref for a product summed in fp32 in ANY order (the stand-in's torch matmul): K - 1 additions, each within
    2^-24 of its partial sum, bound the error by K 2^-24 |A| @ |B| whatever the order; + 64 as chain_hip allows for the rest"""
    return K + 64


class AuditFailure(AssertionError):
    def __init__(self, item: int, msg: str):
        super().__init__(f"audit item {item} ({ITEMS[item]}): {msg}")
        self.item = item


def prev_in_draft_cache(a: int, k: int) -> bool:
    """The draft-cache hole, stated once, from accept_row's comment on fwd0_w (csrc/misc.hip), bonus emit mode: the new `prev`
    sits at old pos_last + a. It is d_a (a >= 1), an input of draft forward a, which ran iff a < k — or the old `last` (a == 0),
    an input of forward 0. So its K / V are in the draft cache exactly when a < k; after a == k the slot is a hole, and the NEXT
    step's forward 0 must be the 2-token form over (prev, last), which fills it: after that step it is valid in every case."""
    return a < k


def rolled_draft(mw, fraction: float, seed: int):
    """a copy of the one-layer target whose lm_head has a seeded `fraction` of its rows rolled among themselves: it proposes
    the target's argmax except where that falls in the rolled set. Shares every other tensor; its own packed copy."""
    V = mw.config.vocab
    idx = torch.randperm(V, generator=torch.Generator().manual_seed(seed))[: int(round(fraction * V))].to(mw.lm_head.device)
    h = mw.lm_head.clone()
    if idx.numel():
        h[idx] = mw.lm_head[idx.roll(1)]
    return dataclasses.replace(mw, lm_head=h, meta={})


def _first_argmax(rows: torch.Tensor) -> torch.Tensor:
    V = rows.shape[-1]
    top = rows.float().amax(-1, keepdim=True)
    ar = torch.arange(V, device=rows.device).expand_as(rows)
    return torch.where(rows.float() == top, ar, torch.full_like(ar, V)).amin(-1)


class StepAudit:
    """Follows one HipSpecDec loop (bonus emit mode) over its steps. `loop`: B, K, step(), sync(), set_row(),
    join_current_stream(), step_logits; the engines: stage_check's reading surface plus forward() / reserve() for the prompts."""

    def __init__(self, loop, draft, target, draft_w, target_w, chain=R.chain_hip, what: str = "", fwd0_select: bool = False,
                 stored: bool = False, draft_taps: bool = True, weight_dtype: str = "bf16"):
        self.loop, self.draft, self.target = loop, draft, target
        self.dw, self.tw = draft_w, target_w
        self.dm, self.tm = matrices(draft_w, weight_dtype), matrices(target_w, weight_dtype)
        self.chain, self.what = chain, what
        self.B, self.K = int(loop.B), int(loop.K)
        self.fwd0_select, self.stored, self.draft_taps = bool(fwd0_select), bool(stored), bool(draft_taps)
        self.seq: List[List[int]] = [[] for _ in range(self.B)]
        self.pos_last = [0] * self.B
        self.active = [True] * self.B
        self.two_next = [True] * self.B          # the form of the next forward 0 (rows of a loop that does not select: always 2)
        self.prev_a: List[Optional[int]] = [None] * self.B
        self.ever_cut = [False] * self.B
        self.tslot: List[Dict[int, int]] = [dict() for _ in range(self.B)]   # position -> the token whose K / V the slot holds
        self.dslot: List[Dict[int, int]] = [dict() for _ in range(self.B)]
        self.frozen: Dict[int, tuple] = {}       # inactive row -> (pos_last, bits of its committed target / draft rows)
        self.steps = 0
        self.accept_hist = collections.Counter()
        self.hole_fills = 0                      # steps of an active row that followed a == K: item 4 saw the hole filled
        self.forms = collections.Counter()
        self.worst = {i: 0.0 for i in ITEMS}

    # ---- the host's side ---------------------------------------------------------------------------------------------------
    def start(self, prompts: Sequence[Sequence[int]], reach: int) -> None:
        """prompts (>= 2 tokens each) into both caches but for their last token, rows set; `reach`: positions past the prompt the
        steps can touch (paged engines get their pages now: the captured step reserves nothing)"""
        for b, p in enumerate(prompts):
            p = [int(t) for t in p]
            assert len(p) >= 2
            for eng in (self.draft, self.target):
                eng.reserve(b, len(p) + reach)
                tok = torch.tensor([p[:-1]], dtype=torch.int32, device=eng.device)
                eng.forward(tok, torch.zeros(1, dtype=torch.int32, device=eng.device), 0, skip_head=True, row0=b)
            self.seq[b] = p
            self.pos_last[b] = len(p) - 1
            for slots in (self.tslot[b], self.dslot[b]):
                slots.update({i: t for i, t in enumerate(p[:-1])})
            self.loop.set_row(b, len(p), p[-2], p[-1], True)
        self.loop.join_current_stream()

    def cut(self, b: int, n_back: int) -> None:
        """the host commits n_back tokens fewer than the device emitted (an EOS cut, a budget): set_row to the shorter sequence.
        The rows above the cut stay in both caches, stale, until later passes overwrite them."""
        self.seq[b] = self.seq[b][: len(self.seq[b]) - n_back]
        s = self.seq[b]
        self.pos_last[b] = len(s) - 1
        self.two_next[b] = True
        self.prev_a[b] = None
        self.ever_cut[b] = True
        self.loop.set_row(b, len(s), s[-2], s[-1], True)

    def deactivate(self, b: int) -> None:
        """the row stops advancing; from now on its committed cache rows and its cur_len must not move"""
        s, c = self.seq[b], self.pos_last[b]
        self.active[b] = False
        self.two_next[b] = True
        self.loop.set_row(b, len(s), s[-2], s[-1], False)
        tk, tv = cache_rows(self.target, b, torch.arange(c))
        dk, dv = cache_rows(self.draft, b, torch.arange(c - 1))
        self.frozen[b] = (c, tk.clone(), tv.clone(), dk.clone(), dv.clone())

    # ---- one step ------------------------------------------------------------------------------------------------------------
    def step(self, **kw):
        self.loop.step(**kw)
        rec = self.loop.sync()
        self.audit(rec)
        return rec

    def _fail(self, item: int, msg: str):
        raise AuditFailure(item, f"{self.what} step {self.steps}: {msg}")

    def _item(self, item: int, fn):
        """run a check of `item`; a bound it misses is that item's failure"""
        try:
            r = fn()
        except AuditFailure:
            raise
        except AssertionError as e:
            self._fail(item, str(e))
        r = max(r.values()) if isinstance(r, dict) else float(r)
        self.worst[item] = max(self.worst[item], r)
        return r

    def _check_cache(self, eng, mw, mats, slots: List[Dict[int, int]], name: str) -> float:
        """every modelled slot of every row against the fp64 K / V of its token at its position -> worst error / bound"""
        c = mw.config
        Hq, Hkv, D = c.n_heads, c.n_kv_heads, c.head_dim
        dev = eng.device
        pos = [sorted(s) for s in slots]
        tokens = torch.tensor([s[p] for s, ps in zip(slots, pos) for p in ps], dtype=torch.long, device=dev)
        positions = torch.tensor([p for ps in pos for p in ps], dtype=torch.long, device=dev)
        x0, x0d = R.embed(c, mw, tokens, positions)
        ref, bnd = R.qkv_stage(c, mw.layers[0], mats["wqkv"], x0, x0d, positions, mw.rope_cos, mw.rope_sin, self.chain)
        got_k, got_v = [], []
        for b, ps in enumerate(pos):
            k, v = cache_rows(eng, b, torch.tensor(ps, dtype=torch.long))
            got_k.append(k.transpose(0, 1).reshape(len(ps), Hkv * D))
            got_v.append(v.transpose(0, 1).reshape(len(ps), Hkv * D))
        where = [(b, p) for b, ps in enumerate(pos) for p in ps]
        out = 0.0
        for nm, got, lo, hi in (("K", got_k, Hq * D, (Hq + Hkv) * D), ("V", got_v, (Hq + Hkv) * D, (Hq + 2 * Hkv) * D)):
            got = torch.cat(got)
            try:
                out = max(out, R.check(got, (ref[:, lo:hi], bnd[:, lo:hi]), f"{name} cache {nm}"))
            except AssertionError as e:
                ratio = ((got.to(R.F64) - ref[:, lo:hi]).abs() / bnd[:, lo:hi]).amax(-1)
                bad = [(b, p, slots[b][p]) for (b, p), r in zip(where, ratio.tolist()) if r > 1][:8]
                raise AssertionError(f"{e}; (row, position, token the protocol put there) of the first bad slots: {bad}")
        return out

    def audit(self, rec) -> None:
        B, K = self.B, self.K
        what = f"{self.what} step {self.steps}"
        old = list(self.pos_last)
        # ---- 1. the record, and the protocol's model of the slots ------------------------------------------------------------
        if int(getattr(rec, "engine_status", 0)) != 0:
            self._fail(1, f"engine_status {rec.engine_status:#x}")
        verify_tok, last_fwd = [], []
        for b in range(B):
            c, s = old[b], self.seq[b]
            d = [int(t) for t in rec.draft_tokens[b][:K]]
            t = [int(x) for x in rec.target_ids[b][:K + 1]]
            a, n_new = int(rec.accept_len[b]), int(rec.n_new[b])
            want_a = next((i for i in range(K) if t[i] != d[i]), K)
            if a != want_a:
                self._fail(1, f"row {b}: accept_len {a}, but target_ids {t} and draft_tokens {d} agree on a prefix of {want_a}")
            if n_new != a + 1 or [int(x) for x in rec.new_tokens[b][:n_new]] != t[:a + 1]:
                self._fail(1, f"row {b}: n_new {n_new}, new_tokens {rec.new_tokens[b].tolist()}; want target_ids[:{a + 1}] = {t[:a + 1]}")
            want_len = c + n_new if self.active[b] else c
            if int(rec.cur_len[b]) != want_len:
                self._fail(1, f"row {b}: cur_len {int(rec.cur_len[b])}, want {c} + {n_new if self.active[b] else 0} = {want_len}")
            prev, last = s[-2], s[-1]
            verify_tok.append([last] + d)
            two = self.two_next[b] or not self.fwd0_select
            self.forms[2 if two else 1] += 1
            # what the step's passes wrote: the draft (prev,) last, d_1..d_{K-1}; the target last, d_1..d_K
            if two:
                self.dslot[b][c - 1] = prev
            self.dslot[b][c] = last
            for i in range(1, K):
                self.dslot[b][c + i] = d[i - 1]
            for m in range(K + 1):
                self.tslot[b][c + m] = verify_tok[b][m]
            last_fwd.append((([prev, last], c - 1) if two else ([last], c)) if K == 1 else ([d[K - 2]], c + K - 1))
            if not self.active[b]:
                continue
            filled = self.prev_a[b] == K
            self.accept_hist[a] += 1
            s.extend(t[:a + 1])
            self.pos_last[b] = c + n_new
            self.prev_a[b] = a
            self.two_next[b] = a >= K
            # the committed sequence is what the slots hold: the target's below pos_last, the draft's below the new prev
            c1 = self.pos_last[b]
            bad = [p for p in range(c1) if self.tslot[b].get(p) != s[p]]
            if bad:
                self._fail(2, f"row {b}: the protocol leaves positions {bad[:8]} of the target cache without their committed token")
            bad = [p for p in range(c1 - 1) if self.dslot[b].get(p) != s[p]]
            if bad:
                self._fail(4, f"row {b}: the protocol leaves positions {bad[:8]} of the draft cache (below the new prev at {c1 - 1}) "
                              f"without their committed token — after a == K the next forward 0 must be the 2-token form")
            has = self.dslot[b].get(c1 - 1) == s[c1 - 1]
            if has != prev_in_draft_cache(a, K) and not (has and self.ever_cut[b]):   # (a cut row regenerates what its stale rows hold)
                self._fail(4, f"row {b}: a = {a} of K = {K}, but the draft cache {'holds' if has else 'lacks'} the new prev at {c1 - 1}")
            self.hole_fills += int(filled)
        # ---- 2. target cache, 4. draft cache: every slot the protocol has written ---------------------------------------------
        r2 = self._item(2, lambda: self._check_cache(self.target, self.tw, self.tm, self.tslot, "target"))
        r4 = self._item(4, lambda: self._check_cache(self.draft, self.dw, self.dm, self.dslot, "draft"))
        print(f"[stage/bound] {what}: target cache {r2:.3f} ({sum(map(len, self.tslot))} slots) draft cache {r4:.3f} "
              f"({sum(map(len, self.dslot))} slots) accept {[int(x) for x in rec.accept_len]}")
        for b, (c, tk, tv, dk, dv) in self.frozen.items():
            k, v = cache_rows(self.target, b, torch.arange(c))
            if not (torch.equal(k, tk) and torch.equal(v, tv)):
                self._fail(2, f"inactive row {b}: its committed target rows [0, {c}) moved")
            k, v = cache_rows(self.draft, b, torch.arange(c - 1))
            if not (torch.equal(k, dk) and torch.equal(v, dv)):
                self._fail(4, f"inactive row {b}: its committed draft rows [0, {c - 1}) moved")
        # ---- 3. the verify pass ----------------------------------------------------------------------------------------------
        dev = self.target.device
        T = B * (K + 1)
        tokens = torch.tensor(verify_tok, dtype=torch.long, device=dev).reshape(-1)
        positions = torch.tensor([old[b] + m for b in range(B) for m in range(K + 1)], dtype=torch.long, device=dev)
        rows = torch.tensor([b for b in range(B) for _ in range(K + 1)], dtype=torch.long)
        ids = torch.tensor([[int(x) for x in rec.target_ids[b][:K + 1]] for b in range(B)], dtype=torch.long, device=dev).reshape(T, 1)
        logits = self.loop.step_logits.reshape(T, -1) if self.stored else None
        self._item(3, lambda: check_pass(self.target, self.tw, self.tm, tokens, positions, rows, logits, self.chain, f"{what} verify"))
        self._item(3, lambda: self._check_ids(self.target, self.tw, self.tm, ids, logits, T, list(range(T)), f"{what} target_ids"))
        # ---- 5. the draft's last forward ---------------------------------------------------------------------------------------
        if self.draft_taps:
            M = len(last_fwd[0][0])
            tokens = torch.tensor([tk for tk, _ in last_fwd], dtype=torch.long, device=dev).reshape(-1)
            positions = torch.tensor([p0 + m for _, p0 in last_fwd for m in range(M)], dtype=torch.long, device=dev)
            rows = torch.tensor([b for b in range(B) for _ in range(M)], dtype=torch.long)
            ids = torch.tensor([int(rec.draft_tokens[b][K - 1]) for b in range(B)], dtype=torch.long, device=dev).reshape(B, 1)
            self._item(5, lambda: check_pass(self.draft, self.dw, self.dm, tokens, positions, rows, None, self.chain,
                                             f"{what} draft forward {K - 1} ({M} token{'s' if M > 1 else ''})"))
            self._item(5, lambda: self._check_ids(self.draft, self.dw, self.dm, ids, None, B * M, [b * M + M - 1 for b in range(B)],
                                                  f"{what} d_{K}"))
        self.steps += 1

    def _check_ids(self, eng, mw, mats, ids, stored, T, sel, what) -> float:
        """ids [n][1] of the tap rows `sel` of a pass of T rows: the first argmax of the stored row where there is one, else
        R.check_head_argmax from the residual tap"""
        if stored is not None:
            want = _first_argmax(stored[sel])
            if not torch.equal(want, ids[:, 0]):
                i = int((want != ids[:, 0]).nonzero()[0])
                raise AssertionError(f"{what}: row {i}: id {int(ids[i, 0])}, but the first argmax of the stored row is {int(want[i])}")
            vals = stored[sel].float().gather(1, ids)
        x = eng.hidden_rows(T)[sel]
        ref, bnd = R.head_stage(mw.config, mw, mats["head"], x, self.chain)
        if stored is None:
            vals = ref.gather(1, ids)
        return R.check_head_argmax(ids, vals, (ref[None], bnd[None]), what)
