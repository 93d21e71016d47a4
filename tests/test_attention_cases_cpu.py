"""The attention geometry cases (tests/attention_cases.py) on a machine without a GPU: the plan, and the proof that the checks
can fail.

1. `sd_attention_plan` (the function launch_attention consults) against the Python restatement, for every case and over a sweep
   of head counts, batches, token counts and cache lengths; every case in the regime it is listed for.
2. For every case and every row of it, the fp64 reference and bound of stage_ref.attention_stage over the case's cache
   contents, then every planted defect applied to the REFERENCE COMPUTATION: some element must move by at least 4 x its bound,
   or a kernel with that defect would pass the GPU test of the case. The 4 x is a condition on the inputs (the sentinel
   layout), not a tolerance of the kernel.

   (a) one (split, wave) class of blocks left out — every class, of the split launch and of the unsplit one
   (b) one class counted twice
   (c) the outputs of two query tiles exchanged (cases with >= 2 tiles)
   (d) two batch rows' caches exchanged (cases with >= 2 rows)
   (e) query m also sees key pos0 + m + 1 (`stale` cases)
   (f) the keys of the last block beyond n_keys are visible
   (g) two pages of the row exchanged (paged cases)

   Where a defect cannot be seen, by the arithmetic and not by the layout, it is not asked:
   - (b) on a row whose keys all belong to one class: every term of numerator and denominator doubles, the output is the same
     bits in exact arithmetic (the defect is harmless there).
   - (a) / (b) under the `peaked` adversary: a softmax concentrated on one key is blind to every class but that key's, by
     construction. There (a) is asked of the classes that hold the heaviest key of some query — leaving such a class out must
     show — and (b) is not asked (doubling the class that holds all the weight changes nothing).
   - (g) exchanges the first page with the page of the last key: two pages wholly visible to every query commute under the
     softmax sum, so only an exchange across the visibility edge can show; rows of one page are skipped.

The least defect / bound of every kind is printed per case (run with -s; profiles/attention_geometry_fp64.md)."""

import math

import pytest
import torch

import attention_cases as A
import stage_ref as R
from specdec_hip.ops import attention_plan

F64 = torch.float64
NEED = 4.0


# ---- the plan ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A.CASES + A.HANDOVER, ids=[c.id for c in A.CASES + A.HANDOVER])
def test_case_reaches_its_regime(case, monkeypatch):
    md = case.model
    for page in case.pages:
        got = attention_plan(md.hq, md.hkv, md.D, case.B, case.M, case.l_max, page or 0)
        want = A.case_plan(case)
        assert (got.tiles, got.n_split) == (want["tiles"], want["n_split"]) == (case.tiles, case.n_split), (got, want)
        assert got.grid == (md.hkv, case.B, case.tiles * case.n_split)
    assert want["cap"] == case.cap, want
    assert tuple(sorted({r[2] for r in want["rows"]})) == case.s_eff, want["rows"]
    assert case.row0 + case.B <= case.bound_batch
    assert all(n + case.M <= case.l_max for n in case.lens) and A.written(case, 0) <= case.l_max <= md.max_pos
    monkeypatch.setenv("SPECDEC_NO_ATTN_SPLIT", "1")
    got = attention_plan(md.hq, md.hkv, md.D, case.B, case.M, case.l_max)
    assert (got.tiles, got.n_split, got.grid) == (case.tiles, 1, (md.hkv, case.B, case.tiles))


def test_listed_regimes():
    """what the case table promises beyond the numbers asserted per case"""
    c = A.BY_ID
    assert [c[f"tile-edge-M{m}"].model.G * m for m in (8, 9, 17)] == [16, 18, 34]
    assert A.query_row(2, 9, 1, 6) == (0, 15) and A.query_row(2, 9, 1, 7) == (1, 0)        # the tile edge inside head 1
    assert (2 * 9) % 16 == 2 and (2 * 17) % 16 == 2                                      # a 2-row last tile
    assert c["ragged"].row0 > 0 and c["ragged"].lens[:8] == (0, 511, 512, 513, 1023, 1025, 2047, 2049)
    for name in ("cap-512", "cap-1b"):
        p = A.case_plan(c[name])
        assert p["base"] == 128 and c[name].l_max // 512 == 9 and p["n_split"] == 4
        assert max(r[1] for r in p["rows"]) / p["n_split"] > 16                          # a workgroup walks more than 16 blocks
    p = A.case_plan(c["past-max"])
    assert p["rows"][0][1] / 32 > 32 and p["rows"][0][0] > 32768
    assert A.case_plan(c["max-split"])["rows"][0][0] > 16384
    assert (c["cap-1b"].model.hq, c["cap-1b"].model.hkv, c["cap-1b"].model.D) == (32, 8, 64)


def test_restatement_agrees_with_the_plan_over_a_sweep():
    """tiles and n_split for every combination; and with the present constants the workspace cap (1024 // base) never binds
    below the chip cap (512 // base): it is the looser of the two for every base, so n_split is never held by it alone"""
    l_maxes = [8, 256, 504, 512, 1016, 1024, 1536, 2048, 4608, 8192, 16384, 16512, 20480, 33024, 40960]
    n = 0
    for hkv in (1, 2, 8):
        for G, D in ((1, 64), (2, 32), (3, 128), (4, 64)):
            for B in (1, 2, 8, 16, 64):
                for M in (1, 2, 5, 9, 17, 128):
                    for l_max in l_maxes:
                        got = attention_plan(hkv * G, hkv, D, B, M, l_max)
                        want = A.plan(hkv * G, hkv, B, M, l_max)
                        assert (got.tiles, got.n_split) == (want["tiles"], want["n_split"]), (hkv, G, B, M, l_max, got, want)
                        assert A.SLOTS // want["base"] >= A.CHIP // want["base"]
                        assert want["cap"] != ("slots",)
                        assert want["n_split"] * want["base"] <= A.SLOTS or want["n_split"] == 1
                        n += 1
    assert n == 3 * 4 * 5 * 6 * len(l_maxes)


def test_query_refuses_in_the_launch_words():
    for args, word in (((4, 2, 48, 1, 5, 1024), "head_dim 48"), ((5, 2, 64, 1, 5, 1024), "Hq % Hkv"), ((4, 2, 64, 0, 5, 1024), "empty batch"),
                       ((4, 2, 64, 1, 5, 1020), "multiple of 8"), ((4, 2, 64, 1, 5, 1024, 48), "paged cache"),
                       ((4, 2, 64, 1, 5, 1056, 64), "paged cache"), ((4, 2, 64, 1, 300, 1024), "attention_plan")):
        with pytest.raises(RuntimeError, match=word):
            attention_plan(*args)
    assert attention_plan(4, 2, 64, 1, 5, 1024, 64).n_split == 2


# ---- the planted defects -------------------------------------------------------------------------------------------------------
def _queries(case, i):
    md = case.model
    gen = torch.Generator().manual_seed(77 + 13 * A.CASES.index(case) + i)
    return torch.randn(case.M, md.hq * md.D, generator=gen).bfloat16()


def _softmax(q, k, v, vis, md):
    """q f64 [M][Hkv][G][D], k / v f64 [Hkv][S][D], vis bool [M][S] -> (p [M][Hkv][G][S] relative to the row maximum over the
    visible keys, num [M][Hkv][G][D], den [M][Hkv][G])"""
    sc = torch.einsum("mhgd,hsd->mhgs", q, k) / math.sqrt(md.D)
    sc = torch.where(vis[:, None, None, :], sc, torch.full_like(sc, -math.inf))
    p = torch.exp(sc - sc.amax(-1, keepdim=True))
    return p, torch.einsum("mhgs,hsd->mhgd", p, v), p.sum(-1)


def _out(num, den):
    return torch.where(den[..., None] > 0, num / den.clamp_min(1e-300)[..., None], torch.zeros_like(num))   # (the kernel writes 0 for an empty row)


class _Row:
    """one row of a case: its reference, its bound and the pieces the defects are built from"""

    def __init__(self, case, i):
        md, self.pos0, self.M = case.model, case.lens[i], case.M
        self.case, self.md = case, md
        self.k16, self.v16 = A.cache_row(case, i)
        self.q16 = _queries(case, i)
        self.n_keys = self.pos0 + self.M
        S = self.n_keys
        q_pos = torch.arange(self.pos0, self.pos0 + self.M)
        kk = self.k16[:, :S].unsqueeze(0).expand(self.M, -1, -1, -1)
        vv = self.v16[:, :S].unsqueeze(0).expand(self.M, -1, -1, -1)
        ref, bound = R.attention_stage(self.q16, kk, vv, q_pos, md.hkv, md.D)
        self.ref = ref.view(self.M, md.hkv, md.G, md.D)
        self.bound = bound.view(self.M, md.hkv, md.G, md.D)
        self.q = self.q16.to(F64).view(self.M, md.hkv, md.G, md.D)
        self.k, self.v = self.k16.to(F64), self.v16.to(F64)
        self.vis = torch.arange(self.k.shape[1])[None, :] <= q_pos[:, None]
        self.p, self.num, self.den = _softmax(self.q, self.k, self.v, self.vis, md)
        assert float(((_out(self.num, self.den) - self.ref).abs() / self.bound).max()) < 1e-6     # the same computation

    def moved(self, out):
        """the largest change of any element, in units of its bound"""
        return float(((out - self.ref).abs() / self.bound).max())

    def with_cache(self, k, v, vis=None):
        n = min(k.shape[1], self.vis.shape[1])
        _, num, den = _softmax(self.q, k[:, :n], v[:, :n], (self.vis if vis is None else vis)[:, :n], self.md)
        return _out(num, den)

    def classes(self, s_eff):
        """{class: (moved when left out, moved when counted twice)} from per-class partial sums"""
        cls = A.key_classes(self.k.shape[1], s_eff)
        res = {}
        for c in sorted(set(cls[:self.n_keys].tolist())):
            idx = (cls == c).nonzero().flatten()
            pc = self.p[..., idx]
            num_c, den_c = torch.einsum("mhgs,hsd->mhgd", pc, self.v[:, idx]), pc.sum(-1)
            res[c] = (self.moved(_out(self.num - num_c, (self.den - den_c).clamp_min(0.0))), self.moved(_out(self.num + num_c, self.den + den_c)))
        return res


def _least(table, kind, value):
    table[kind] = min(table.get(kind, math.inf), value)


@pytest.mark.parametrize("case", A.CASES, ids=[c.id for c in A.CASES])
def test_planted_defects_move_the_reference(case):
    md, M = case.model, case.M
    rows = [_Row(case, i) for i in range(case.B)]
    least = {}
    for i, r in enumerate(rows):
        what = f"{case.id} row {i} ({r.pos0} keys)"
        # (a), (b): the classes of the split launch and of the unsplit one
        for split in (True, False):
            s_eff = A.row_plan(A.case_plan(case, split)["n_split"], r.pos0, M, case.l_max)[2]
            res = r.classes(s_eff)
            if case.adversary == "peaked":
                cls = A.key_classes(r.k.shape[1], s_eff)
                heavy = sorted(set(cls[r.p.argmax(-1).flatten()].tolist()))
                assert heavy
                for c in heavy:
                    _least(least, "a", res[c][0])
                    assert res[c][0] >= NEED, f"{what}: class {divmod(c, 4)} of s_eff {s_eff} left out moves {res[c][0]:.2f} x the bound"
                continue
            for c, (out, twice) in res.items():
                _least(least, "a", out)
                assert out >= NEED, f"{what}: class {divmod(c, 4)} of s_eff {s_eff} left out moves {out:.2f} x the bound"
                if len(res) > 1:
                    _least(least, "b", twice)
                    assert twice >= NEED, f"{what}: class {divmod(c, 4)} of s_eff {s_eff} counted twice moves {twice:.2f} x the bound"
        # (c) the outputs of tile t and t + 1 exchanged, row by row
        if case.tiles >= 2:
            flat = r.ref.permute(1, 2, 0, 3).reshape(md.hkv, md.G * M, md.D)         # [Hkv][gh * M + m][D]: the kernel's row order
            for t in range(case.tiles - 1):
                n = min(A.ROWS, md.G * M - (t + 1) * A.ROWS)
                sw = flat.clone()
                sw[:, t * 16:t * 16 + n], sw[:, (t + 1) * 16:(t + 1) * 16 + n] = flat[:, (t + 1) * 16:(t + 1) * 16 + n], flat[:, t * 16:t * 16 + n]
                mv = r.moved(sw.view(md.hkv, md.G, M, md.D).permute(2, 0, 1, 3))
                _least(least, "c", mv)
                assert mv >= NEED, f"{what}: tiles {t} and {t + 1} exchanged move {mv:.2f} x the bound"
        # (d) the next row's cache
        if case.B >= 2:
            o = rows[(i + 1) % case.B]
            n = r.k.shape[1]
            k2, v2 = torch.zeros_like(r.k), torch.zeros_like(r.v)                     # (beyond what the other row wrote: a fresh cache's zeros)
            m = min(n, o.k.shape[1])
            k2[:, :m], v2[:, :m] = o.k[:, :m], o.v[:, :m]
            mv = r.moved(r.with_cache(k2, v2))
            _least(least, "d", mv)
            assert mv >= NEED, f"{what}: the cache of row {(i + 1) % case.B} moves {mv:.2f} x the bound"
        # (e) one key of the future
        if case.adversary == "stale":
            mv = r.moved(r.with_cache(r.k, r.v, torch.arange(r.k.shape[1])[None, :] <= (r.pos0 + 1 + torch.arange(M))[:, None]))
            _least(least, "e", mv)
            assert mv >= NEED, f"{what}: key pos0 + m + 1 visible moves {mv:.2f} x the bound"
        # (f) the last block's keys beyond n_keys
        end = -(-r.n_keys // A.BLOCK) * A.BLOCK
        assert r.n_keys < end <= r.k.shape[1], "every row of the table ends inside a block"
        beyond = (torch.arange(r.k.shape[1]) >= r.n_keys) & (torch.arange(r.k.shape[1]) < end)
        mv = r.moved(r.with_cache(r.k, r.v, r.vis | beyond[None, :]))
        _least(least, "f", mv)
        assert mv >= NEED, f"{what}: keys {r.n_keys}..{end - 1} visible move {mv:.2f} x the bound"
        # (g) the first page and the page of the last key exchanged
        for P in case.pages:
            if P is None or (r.n_keys - 1) // P == 0:
                continue
            a0 = (r.n_keys - 1) // P * P
            pad = a0 + P - r.k.shape[1]                                              # (the unwritten end of the last page: zeros)
            k2, v2 = (torch.cat([t, t.new_zeros(md.hkv, max(pad, 0), md.D)], 1) for t in (r.k, r.v))
            for t in (k2, v2):
                first = t[:, :P].clone()
                t[:, :P] = t[:, a0:a0 + P]
                t[:, a0:a0 + P] = first
            mv = r.moved(r.with_cache(k2, v2))
            _least(least, "g", mv)
            assert mv >= NEED, f"{what}: pages 0 and {a0 // P} (of {P}) exchanged move {mv:.2f} x the bound"
    if any(P is not None for P in case.pages):
        assert "g" in least, "no row of a paged case spans two pages"
    print(f"[defect/bound] {case.id}: " + " ".join(f"({k}) {v:.1f}" for k, v in sorted(least.items())))
