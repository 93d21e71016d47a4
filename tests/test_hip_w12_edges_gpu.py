"""W12 / W12S on the device where random weights never put them: the format's edges through the device packer, and wide blocks
PLANTED at chosen places of the GEMV's work split (tests/w12_cases.py; the builders are checked in tests/test_w12_cases_cpu.py).

a. The device packer (w12_classify_kernel / w12_number_kernel / w12_fill_kernel, csrc/pack.hip) decides narrow or wide by widening
   on the device (w12_widen / w12s_widen, csrc/gemv_device.h) and comparing, so its table, main stream and overflow against
   specdec_hip/w12.py, byte for byte, on every edge case is an exact test of the device widening on every bit pattern — inf, nan
   and huge values included (nothing is multiplied in that part).
b. Forwards with every matrix class on the form under test against the same forwards under SPECDEC_NO_W12, bit for bit (every
   stage tap, ids, bf16 logits, both caches), on a background that is narrow everywhere with wide blocks planted: none at all; one
   per batch at every batch position (stairs); whole first and last batches (runs); the first and the last step of every slice
   (edges); short last tiles and the last workgroup (tail) — on the one-layer 1B / 3B / 8B cuts and on three heads with the
   production lm_head's work split at small K (251 pairs per workgroup in 32 tiles over two rounds; 26 tiles where the table
   stride is not the round-up to 32; 13 of 16). The native table must name exactly the planted blocks.
c. The same weights against the fp64 stage reference (tests/stage_ref.py) with its derived bounds, so that the two routes cannot
   be wrong together.

Parts a and b are exact: no tolerance appears in them."""

import re

import numpy as np
import pytest
import torch

import gemv_cases
import test_hip_stage_fp64_gpu as stage
import w12_cases as C
from specdec_hip import w12
from specdec_hip import weights as W
from specdec_hip.ops import gemv_instance

pytestmark = pytest.mark.gpu

CTX = 7                     # positions in the cache before the compared passes
FORMS = {"w12": w12.W12_CODES, "w12s": w12.W12_SPLIT}
CLASS_ENV = {"w12": "SPECDEC_W12_CLASSES", "w12s": "SPECDEC_W12S_CLASSES"}


def _config(name, dims, **kw):
    return W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=1, max_pos=256, rope_theta=500000.0, tie_embeddings=True, name=name, **dims, **kw)


def _env(monkeypatch, form):
    monkeypatch.setenv("SPECDEC_NO_PERSIST", "1")        # the launch path at 1 and 2 tokens too
    monkeypatch.setenv("SPECDEC_W12", "1")
    monkeypatch.delenv("SPECDEC_W12_CLASSES", raising=False)
    monkeypatch.delenv("SPECDEC_W12S_CLASSES", raising=False)
    monkeypatch.setenv(CLASS_ENV[form], "0x1f")          # every matrix class on the form under test
    monkeypatch.delenv("SPECDEC_NO_W12", raising=False)
    monkeypatch.delenv("SPECDEC_GEMV_GENERIC", raising=False)


def _matrices(w):
    """the five matrices in packing order (one layer; the lm_head is the tied embedding)"""
    l = w.layers[0]
    return [l.wqkv, l.wo, l.w_up, l.w_down, w.lm_head]


def _set_bits(t, bits):
    t.copy_(torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).to(t.device))


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _copy_parts(buf, info, entries):
    """(main, overflow, table) of a matrix of a W12 buffer (a host array), at the offsets sd_w12_matrix gives"""
    o = info["offset"]
    main = buf[o:o + info["main_bytes"]]
    ovf = buf[o + info["main_bytes"]:o + info["main_bytes"] + info["ovf_bytes"]]
    t0 = o + info["main_bytes"] + info["ovf_bytes"]
    return main, ovf, buf[t0:t0 + 4 * entries].view(np.uint32)


# ---- a. the device packer on the format's edges ------------------------------------------------------------------------------------
# wo of the first model is [64][512]: one pair per tile, the shape of the CPU format tests' block cases; the second model has
# the toy-b dimensions (8 and 5 pairs per tile, K = 2048 in 16 slices)
EDGE_MODELS = {
    "1 pair per tile": dict(d_model=64, n_heads=8, n_kv_heads=8, head_dim=64, d_ff=256, vocab=1001),
    "toy-b": dict(d_model=256, n_heads=4, n_kv_heads=2, head_dim=64, d_ff=2048, vocab=2560),
}
EDGE_NAMES = list(C.edge_cases())


@pytest.mark.parametrize("first", range(len(EDGE_NAMES)), ids=[n.replace(" ", "-") for n in EDGE_NAMES])
def test_device_packer_on_the_edge_cases(first, monkeypatch):
    """edge case `first` in wo and the next four in the other matrices, in both models and both forms"""
    from specdec_hip.engine import HipModel, build_w12, w12_matrix_info

    _env(monkeypatch, "w12")
    monkeypatch.setenv("SPECDEC_W12", "0")               # the copies are built below, one per form, over the same packed weights
    cases = C.edge_cases()
    checked = left_out = 0
    for model, dims in EDGE_MODELS.items():
        cfg = _config(f"w12-edges-{model}", dims)
        w = W.random_init(cfg, seed=1, device="cuda")
        shapes = C.model_matrices(**dims)
        want_bits = {}
        for j, which in enumerate((1, 0, 2, 3, 4)):      # wo takes the case under test
            N, K, epi, hd = shapes[which]
            want_bits[which] = cases[EDGE_NAMES[(first + j) % len(EDGE_NAMES)]](N, K, epi, hd)
            _set_bits(_matrices(w)[which], want_bits[which])
        hm = HipModel(w, batch=1, l_max=32)
        assert hm._w12 is None and hm._w12s is None
        packed = hm._packed.cpu().numpy()
        for form in FORMS.values():
            buf, n_wide = build_w12(hm.lib, hm._mc, hm.device, 0x1F, form)
            buf = buf.cpu().numpy()
            off_bf16 = 0
            for which, (N, K, epi, hd) in enumerate(shapes):
                n_pairs = C.n_pairs_of(N, epi)
                info = w12_matrix_info(hm.lib, hm._mc, n_wide, which, form=form)
                want_stream = w12.pack_bf16(want_bits[which], n_pairs, epi, hd)
                assert np.array_equal(packed[off_bf16:off_bf16 + want_stream.nbytes].view(np.uint16), want_stream), (model, which)
                off_bf16 += info["bf16_bytes"]
                ref = w12.w12_pack(want_stream, n_pairs, K, form)
                what = (model, EDGE_NAMES[(first + (1, 0, 2, 3, 4).index(which)) % len(EDGE_NAMES)], which, form)
                assert info["n_wide"] == ref.n_wide and info["blocks"] == ref.table.size, what      # also for a matrix left out
                assert info["taken"] == (C.covered(n_pairs, K) and C.taken(n_pairs, K, ref.n_wide)), what
                if not info["taken"]:
                    left_out += 1
                    continue
                main, ovf, table = _copy_parts(buf, info, ref.table.size)
                assert np.array_equal(table, ref.table), what
                assert np.array_equal(main[:ref.main.nbytes], ref.main) and np.array_equal(ovf[:ref.ovf.nbytes], ref.ovf), what
                native = w12.W12Matrix(main[:ref.main.nbytes], ovf[:ref.ovf.nbytes], table, ref.n_blocks, ref.n_wide)
                assert np.array_equal(w12.w12_unpack(native, n_pairs, K, form), want_stream), what   # decodes to the input bits
                checked += 1
    assert checked >= 8, (checked, left_out)


# ---- b. GEMVs on planted patterns, bit for bit against the bf16 route ----------------------------------------------------------------
def _background(N, K, gen):
    """w12_cases.narrow_background on the device: +-(1 + u) * 2^e, e uniform in -9 .. -4"""
    u = torch.rand(N, K, generator=gen, device="cuda")
    e = torch.randint(-9, -3, (N, K), generator=gen, device="cuda")
    sign = torch.randint(0, 2, (N, K), generator=gen, device="cuda") * 2 - 1
    return ((1.0 + u) * torch.exp2(e.float()) * sign).bfloat16()


def _build(model, pattern):
    """-> (weights, {matrix: planted table indices in table order}, {matrix: (kind, thinning)}): built on the device, the
    planted elements from the host-side coordinates"""
    dims = C.GPU_MODELS[model]
    cfg = _config(f"w12-edges-{model}", dims)
    w = W.random_init(cfg, seed=3, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(17)
    planted = {}
    for which, (N, K, epi, hd) in enumerate(C.model_matrices(**dims)):
        mat = _matrices(w)[which]
        assert tuple(mat.shape) == (N, K)
        n_pairs = C.n_pairs_of(N, epi)
        if which not in C.UNDER_TEST[model]:
            mat.copy_(_background(N, K, gen))
            continue
        if pattern == "window":
            bits, index, top = C.window_background(N, K, epi, hd, 23 + which)
            _set_bits(mat, bits)
            planted[which] = (np.zeros(0, dtype=np.int64), 1, (index, top))
            continue
        mat.copy_(_background(N, K, gen))
        m = C.thinning(n_pairs, K, pattern)
        rows, cols, idx = C.plant_coords(n_pairs, K, epi, hd, C.pattern(pattern, m))
        assert rows.size == 0 or (rows.max() < N and cols.max() < K)
        if idx.size:
            mat[torch.from_numpy(rows).cuda(), torch.from_numpy(cols).cuda()] = 0.0
        planted[which] = (idx, m, None)
    return w, planted


def _instances(hm, T, form):
    out = []
    for which in range(5):
        _, K, n_pairs, epi, pro = hm.matrix_shape(which)
        out.append(gemv_instance(T, n_pairs, K, False, pro, epi, w12=form))
    return out


def _run(w, form, no_w12, monkeypatch, batch=1, tokens=C.TOKENS):
    """every observable of the passes: stage rows, logits, ids, then the whole K and V caches"""
    from specdec_hip.engine import HipModel

    _env(monkeypatch, form)
    hm = HipModel(w, batch=batch, l_max=64)              # built WITH the copy on both sides: the switch is the library's
    assert (hm._w12 is not None) == (form == "w12") and (hm._w12s is not None) == (form == "w12s")
    if no_w12:
        monkeypatch.setenv("SPECDEC_NO_W12", "1")
    g = torch.Generator().manual_seed(12)
    toks = torch.randint(0, w.config.vocab, (batch, CTX + sum(tokens)), generator=g).to(torch.int32).cuda()
    seen, names = [], {}
    pos = 0
    for M in (CTX,) + tuple(tokens):
        T = batch * M
        if T <= 9:                                       # (the two-row context pass, 14 tokens, is not a GEMV launch)
            names[T] = _instances(hm, T, FORMS[form])
        ids, logits = hm.forward(toks[:, pos:pos + M].contiguous(), torch.full((batch,), pos, dtype=torch.int32, device="cuda"), 0,
                                 want_logits=True, logits_dtype=torch.bfloat16, skip_head=(pos == 0))
        for which in (hm.DEBUG_X, hm.DEBUG_Q, hm.DEBUG_ATTN, hm.DEBUG_ACT):
            seen.append((f"T={T} stage {which}", hm.debug_rows(which, T).cpu()))
        if ids is not None:
            seen.append((f"T={T} ids", ids.cpu()))
            seen.append((f"T={T} logits", logits.cpu()))
        pos += M
    torch.cuda.synchronize()
    seen.append(("k cache", hm.k_cache.cpu()))
    seen.append(("v cache", hm.v_cache.cpu()))
    return seen, names, hm


def _longest_run(flags):
    best = run = 0
    for f in flags.tolist():
        run = run + 1 if f else 0
        best = max(best, run)
    return best


def _check_copy(model, pattern, form, hm, planted, names):
    """the conditions of a case, all asserted: taken, the native table's wide blocks are the planted ones, the instance names"""
    from specdec_hip.engine import w12_matrix_info

    buf, n_wide = hm._w12 if form == "w12" else hm._w12s
    report = []
    for which in C.UNDER_TEST[model]:
        idx, m, window = planted[which]
        _, K, n_pairs, epi, _ = hm.matrix_shape(which)
        info = w12_matrix_info(hm.lib, hm._mc, n_wide, which, form=FORMS[form])
        what = (model, pattern, form, which)
        assert info["taken"], what
        g = C.grid(n_pairs, K)
        assert g.q.kw * g.q.ksplit == K and info["blocks"] == g.q.grid * g.ntf * g.nst
        t0 = info["offset"] + info["main_bytes"] + info["ovf_bytes"]
        table = buf[t0:t0 + 4 * info["blocks"]].cpu().numpy().view(np.uint32)
        wide = np.nonzero(table >> 31)[0]
        assert info["n_wide"] == idx.size and np.array_equal(wide, idx), (what, info["n_wide"], idx.size)
        assert np.array_equal(table[wide] & 0x7FFFFF, np.arange(idx.size))              # numbered once each, in stream order
        if pattern in C.UNTHINNED:
            assert m == 1 or g.q.tile_pairs < 4, what
        if pattern == "none":
            assert info["n_wide"] == 0 and info["ovf_bytes"] == 0, what
        elif pattern != "window":
            assert idx.size > 0, what
        if window is not None:                                                            # every base from the block's largest exponent
            index, top = window
            assert info["n_wide"] == 0 and np.array_equal((table[index] >> 23) & 0xFF, w12.block_base(top, FORMS[form])), what
        depths = set()
        for T, five in names.items():
            n = five[which]
            assert form + "," in n or n.endswith(form + ">"), (what, T, n)                # "w12" or "w12s", not the other
            if model in ("1b", "3b", "8b") and which < 4:
                assert n.startswith("fixed<") == (T == 5), (what, T, n)                   # twins of the fixed instances: token bound 5
            depths.add(int(re.search(r"kb(\d+)", n).group(1)))
        if pattern.startswith("runs"):                    # a slice with kb consecutive wide steps (all of it where it is shorter)
            flags = (table >> 31).reshape(-1, g.S)                                       # one row per (tile, slice)
            assert max(_longest_run(f) for f in flags[flags.any(axis=1)][:64]) >= min(max(depths), g.S), what
        report.append(f"{which}:{idx.size}/{info['n_wide']}(m={m})")
    return report


def _compare(model, pattern, got, want):
    assert len(got) == len(want)
    for (what, a), (_, b) in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a, b.view(torch.int16) if b.dtype == torch.bfloat16 else b), (model, pattern, what)
    for what, t in got:
        if "stage" in what or "cache" in what or "logits" in what:
            assert torch.isfinite(t.float()).all() and t.float().abs().sum() > 0, (model, pattern, what)


@pytest.mark.parametrize("model,pattern", C.GPU_CASES, ids=[f"{m}-{p.replace(':', '')}" for m, p in C.GPU_CASES])
def test_forwards_on_planted_patterns_are_equal_bit_for_bit(model, pattern, monkeypatch):
    w, planted = _build(model, pattern)
    for form in FORMS:
        want, names_off, _ = _run(w, form, True, monkeypatch)
        got, names_on, hm = _run(w, form, False, monkeypatch)
        assert all("w12" not in n for names in names_off.values() for n in names)
        report = _check_copy(model, pattern, form, hm, planted, names_on)
        print(f"[w12 edges] {model} {pattern} {form}: planted/native wide per matrix {' '.join(report)}; "
              f"instances {sorted({n for five in names_on.values() for i, n in enumerate(five) if i in C.UNDER_TEST[model]})}")
        _compare(model, pattern, got, want)


def test_two_rows_of_four_tokens_on_the_1b_cut(monkeypatch):
    """batch = 2, M = 4: an 8-token pass (token bound 9), the t -> (row, position) map of the QKV and head epilogues"""
    w, planted = _build("1b", "stairs:6")
    for form in FORMS:
        want, _, _ = _run(w, form, True, monkeypatch, batch=2, tokens=(4,))
        got, names_on, hm = _run(w, form, False, monkeypatch, batch=2, tokens=(4,))
        assert set(names_on) == {8}
        _check_copy("1b", "stairs:6", form, hm, planted, names_on)
        _compare("1b", "stairs:6 B=2", got, want)


def _w12_depths(names):
    return {m.group(0) for n in names if "w12" in n for m in [re.search(r"kb\d+", n)]}


def test_the_cases_run_every_batch_depth_of_the_production_launches():
    """the instance names asserted per case above, over the whole list, against the W12 launches of the production shapes"""
    for form in FORMS.values():
        want = set()
        for cfg in gemv_cases.G.PRODUCTION:
            _, _, shapes = gemv_cases.G.model_facts(cfg, "bf16")
            want |= _w12_depths(gemv_instance(T, n_pairs, K, False, pro, epi, w12=form) for T in range(1, 10) for (_, K, n_pairs, epi, pro) in shapes)
        got = set()
        for model, dims in C.GPU_MODELS.items():
            _, _, shapes = gemv_cases.G.model_facts(_config(f"w12-edges-{model}", dims), "bf16")
            for which in C.UNDER_TEST[model]:
                _, K, n_pairs, epi, pro = shapes[which]
                got |= _w12_depths(gemv_instance(T, n_pairs, K, False, pro, epi, w12=form) for T in C.TOKENS)
        assert want and got >= want, (form, want, got)


# ---- c. the fp64 anchor --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,pattern", [(m, p) for m in C.WINDOW_MODELS for p in ("stairs:6", "window")],
                         ids=[f"{m}-{p.replace(':', '')}" for m in C.WINDOW_MODELS for p in ("stairs:6", "window")])
def test_planted_weights_against_the_fp64_stages(model, pattern, monkeypatch):
    """W12S, M = 5: every stage within the derived bounds of tests/stage_ref.py (unchanged); the worst stage / bound ratios are
    printed (run with -s)"""
    from specdec_hip.engine import HipModel

    M, pos0 = 5, CTX
    w, planted = _build(model, pattern)
    _env(monkeypatch, "w12s")
    eng = HipModel(w, batch=1, l_max=pos0 + M + 64)
    eng.set_persist_tokens(0)
    assert eng._w12s is not None and not eng.persist_active(M)
    names = {M: _instances(eng, M, w12.W12_SPLIT)}
    _check_copy(model, pattern, "w12s", eng, planted, names)
    gen = torch.Generator(device="cuda").manual_seed(pos0 + M)
    stage._write_prefix(eng, 0, pos0, gen, spikes=(pos0 - 1, 3))
    tok = torch.randint(4, w.config.vocab, (1, M), generator=gen, device="cuda", dtype=torch.int32)
    _, logits = eng.forward(tok, torch.tensor([pos0], dtype=torch.int32, device="cuda"), want_logits=True)
    positions = torch.arange(pos0, pos0 + M, device="cuda")
    stage._check_pass(eng, w, stage._matrices(w, "bf16"), tok[0].long(), positions, torch.zeros(M, dtype=torch.long), logits[0],
                      stage.R.chain_hip, f"w12s {model} {pattern} M={M}")
