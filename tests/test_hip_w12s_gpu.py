"""W12S, the split-byte form of the lossless 12-bit weight copy (csrc/gemv_device.h, csrc/pack.hip, csrc/gemv.hip), on the GPU.

Exact properties only (no tolerance appears in this file):
  * the native packer's W12S streams, overflow and table are the ones specdec_hip/w12.py builds (w12s_pack), byte for byte,
    and they decode to the packed bf16 stream;
  * a forward with every matrix class on its W12S copy gives the bits of the same forward under SPECDEC_NO_W12 (read at every
    launch: both routes in one process), and the instance names say which kernel ran;
  * a greedy speculative run gives the same tokens and counters with and without the copy.

Shapes: the toy models and the one-layer, vocab-1024 cuts of the 1B / 3B / 8B dimensions (every class of the fixed-geometry
table between them), at 1, 2, 3, 5 and 9 tokens: every token bound of the generic kernel and the fixed twins' bound, 5. Row 0
of every matrix has an exact zero in every other 32-k step, so the blocks of its tile alternate wide, narrow, wide, ..."""

import dataclasses

import numpy as np
import pytest
import torch

from specdec_hip import w12
from specdec_hip import weights as W
from specdec_hip.ops import gemv_instance

pytestmark = pytest.mark.gpu

TOKENS = (1, 2, 3, 5, 9)
CTX = 7                     # positions in the cache before the compared passes


def _toy(**kw):
    return W.ModelConfig(arch=W.ARCH_LLAMA, max_pos=256, rope_theta=500000.0, tie_embeddings=True, **kw)


def _one_layer(base):
    return dataclasses.replace(base, n_layers=1, vocab=1024, max_pos=256, tie_embeddings=True)


MODELS = {
    "toy-a": _toy(n_layers=2, d_model=64, n_heads=2, n_kv_heads=2, head_dim=32, d_ff=256, vocab=1001, name="w12s-toy-a"),
    "toy-b": _toy(n_layers=2, d_model=256, n_heads=4, n_kv_heads=2, head_dim=64, d_ff=2048, vocab=2560, name="w12s-toy-b"),
    "1b": _one_layer(W.LLAMA_3_2_1B),
    "3b": _one_layer(W.LLAMA_3_2_3B),
    "8b": _one_layer(W.LLAMA_3_8B),
}
_weights = {}


def _model_weights(name):
    if name not in _weights:
        cfg = MODELS[name]
        w = W.random_init(cfg, seed=cfg.d_model + 2, device="cuda")
        for l in w.layers:                       # alternate wide and narrow blocks along row 0 of every matrix
            for m in (l.wqkv, l.wo, l.w_up, l.w_down):
                m[0, 0::64] = 0.0
        w.lm_head[0, 0::64] = 0.0
        _weights[name] = w
    return _weights[name]


def _env(monkeypatch):
    monkeypatch.setenv("SPECDEC_NO_PERSIST", "1")        # the launch path at 1 and 2 tokens too
    monkeypatch.setenv("SPECDEC_W12", "1")
    monkeypatch.delenv("SPECDEC_W12_CLASSES", raising=False)
    monkeypatch.setenv("SPECDEC_W12S_CLASSES", "0x1f")   # every matrix class on the split-byte form
    monkeypatch.delenv("SPECDEC_NO_W12", raising=False)


def _model(name, **kw):
    from specdec_hip.engine import HipModel

    return HipModel(_model_weights(name), batch=1, l_max=64, **kw)


def _matrices(w):
    """(index, HF matrix, epilogue, head_dim) in packing order"""
    c = w.config
    out = []
    for i, l in enumerate(w.layers):
        out += [(4 * i, l.wqkv, w12.EPI_QKV_ROPE, c.head_dim), (4 * i + 1, l.wo, w12.EPI_RESID, 0),
                (4 * i + 2, l.w_up, w12.EPI_SWIGLU, 0), (4 * i + 3, l.w_down, w12.EPI_RESID, 0)]
    out.append((4 * c.n_layers, w.lm_head, w12.EPI_ARGMAX, 0))
    return out


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("name", ["toy-a", "toy-b"])
def test_native_w12s_streams_are_the_reference_streams_and_decode_to_the_input(name, monkeypatch):
    from specdec_hip.engine import W12_SPLIT, w12_matrix_info

    _env(monkeypatch)
    hm = _model(name)
    assert hm._w12 is None and hm._w12s is not None
    buf, n_wide = hm._w12s
    buf, packed = buf.cpu().numpy(), hm._packed.cpu().numpy()
    off_bf16 = 0
    n_taken = 0
    for index, mat, epi, hd in _matrices(hm.weights):
        N, K = mat.shape
        n_pairs = (N + 1) // 2 if epi != w12.EPI_SWIGLU else N // 2
        info = w12_matrix_info(hm.lib, hm._mc, n_wide, index, form=W12_SPLIT)
        assert info["form"] == W12_SPLIT
        want_stream = w12.pack_bf16(_bits(mat), n_pairs, epi, hd)
        got_stream = packed[off_bf16:off_bf16 + want_stream.nbytes].view(np.uint16)
        assert np.array_equal(got_stream, want_stream), (name, index)
        off_bf16 += info["bf16_bytes"]
        ref = w12.w12s_pack(want_stream, n_pairs, K)
        assert info["n_wide"] == ref.n_wide and info["blocks"] == ref.table.size, (name, index)
        assert info["taken"] == (w12.w12_bytes(n_pairs, K, ref.n_wide) <= 0.85 * info["bf16_bytes"])
        if not info["taken"]:
            continue
        n_taken += 1
        o = info["offset"]
        main = buf[o:o + ref.main.nbytes]
        ovf = buf[o + info["main_bytes"]:o + info["main_bytes"] + ref.ovf.nbytes]
        table = buf[o + info["main_bytes"] + info["ovf_bytes"]:o + info["main_bytes"] + info["ovf_bytes"] + ref.table.nbytes].view(np.uint32)
        assert np.array_equal(table, ref.table), (name, index)
        assert np.array_equal(main, ref.main) and np.array_equal(ovf, ref.ovf), (name, index)
        native = w12.W12Matrix(main, ovf, table, ref.n_blocks, ref.n_wide)
        assert np.array_equal(w12.w12s_unpack(native, n_pairs, K), want_stream), (name, index)   # decodes to the input bits
        flags = table[:K // 32] >> 31                     # row 0 sits in tile 0 of workgroup 0
        assert (flags[0::2] == 1).all() and (flags[1::2] == 0).sum() >= 1, (name, index, flags)
        assert 0 < ref.n_wide < ref.n_blocks
        # the two forms are different bytes: the code form's stream of the same matrix is not this one
        assert not np.array_equal(main, w12.w12_pack(want_stream, n_pairs, K).main)
    assert n_taken >= 3


def _instances(hm, T, form):
    out = []
    for which in range(5):
        _, K, n_pairs, epi, pro = hm.matrix_shape(which)
        out.append(gemv_instance(T, n_pairs, K, False, pro, epi, w12=form))
    return out


def _run(name, no_w12, monkeypatch):
    """every observable of the passes: stage rows, logits, ids, then the whole K and V caches"""
    from specdec_hip.engine import W12_SPLIT

    _env(monkeypatch)
    hm = _model(name)                                    # built WITH the copy on both sides: the switch is the library's
    assert hm._w12s is not None and hm._w12 is None
    if no_w12:
        monkeypatch.setenv("SPECDEC_NO_W12", "1")
    cfg = MODELS[name]
    g = torch.Generator().manual_seed(12)
    toks = torch.randint(0, cfg.vocab, (1, CTX + sum(TOKENS)), generator=g).to(torch.int32).cuda()
    seen, names = [], {}
    pos = 0
    for T in (CTX,) + TOKENS:
        names[T] = _instances(hm, T, W12_SPLIT)
        ids, logits = hm.forward(toks[:, pos:pos + T].contiguous(), torch.tensor([pos], dtype=torch.int32, device="cuda"), 0,
                                 want_logits=True, logits_dtype=torch.bfloat16, skip_head=(pos == 0))
        for which in (hm.DEBUG_X, hm.DEBUG_Q, hm.DEBUG_ATTN, hm.DEBUG_ACT):
            seen.append((f"T={T} stage {which}", hm.debug_rows(which, T).cpu()))
        if ids is not None:
            seen.append((f"T={T} ids", ids.cpu()))
            seen.append((f"T={T} logits", logits.cpu()))
        pos += T
    torch.cuda.synchronize()
    seen.append(("k cache", hm.k_cache.cpu()))
    seen.append(("v cache", hm.v_cache.cpu()))
    return seen, names, hm


@pytest.mark.parametrize("name", list(MODELS))
def test_forwards_on_w12s_and_on_bf16_are_equal_bit_for_bit(name, monkeypatch):
    from specdec_hip.engine import W12_SPLIT, w12_matrix_info

    want, names_off, _ = _run(name, True, monkeypatch)
    got, names_on, hm = _run(name, False, monkeypatch)
    taken = [w12_matrix_info(hm.lib, hm._mc, hm._w12s[1], i, form=W12_SPLIT)["taken"] for i in (0, 1, 2, 3, 4 * hm.cfg.n_layers)]
    # (the 8B down-projection, K = 14336, is a MASK shape: bf16; a toy matrix of a few KB can miss the 15 % rule and stays bf16)
    covered = [True, True, True, name != "8b", True] if name in ("1b", "3b", "8b") else taken
    assert taken == covered and sum(taken) >= 3, (name, taken)
    for T, names in names_on.items():
        for which, n in enumerate(names):
            assert ("w12s" in n) == covered[which], (name, T, names)
            if name in ("1b", "3b", "8b") and which < 4 and covered[which]:
                assert n.startswith("fixed<") == (T == 5), (name, T, n)      # W12S twins of the fixed instances: token bound 5
    assert all("w12" not in n for names in names_off.values() for n in names)
    assert len(got) == len(want)
    for (what, a), (_, b) in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a, b.view(torch.int16) if b.dtype == torch.bfloat16 else b), (name, what)
    assert all(t.float().abs().sum() > 0 for what, t in got if "stage" in what or "cache" in what)


def test_a_greedy_pipeline_run_gives_the_same_tokens_and_counts(monkeypatch):
    from helpers import synthetic_prompts
    from src.specdec import HipLM, SpeculativePipeline

    tcfg = _toy(n_layers=2, d_model=256, n_heads=4, n_kv_heads=2, head_dim=64, d_ff=512, vocab=2048, name="w12s-target")
    dcfg = _toy(n_layers=1, d_model=128, n_heads=2, n_kv_heads=1, head_dim=64, d_ff=256, vocab=2048, name="w12s-draft")
    tcfg, dcfg = dataclasses.replace(tcfg, tie_embeddings=False), dataclasses.replace(dcfg, tie_embeddings=False)
    tgt = W.synthetic_llama(tcfg, seed=3).to("cuda")
    drf = W.synthetic_llama(dcfg, seed=4, embed_from=tgt, flip_fraction=0.25).to("cuda")
    prompts = synthetic_prompts(1, 12, 2048, seed=5).tolist()
    _env(monkeypatch)
    runs = []
    for no_w12 in (True, False):
        monkeypatch.setenv("SPECDEC_W12", "0" if no_w12 else "1")
        pipe = SpeculativePipeline(base_lm=HipLM(tgt), draft_lm=HipLM(drf), controller="fixed", controller_params={"k": 4}, seed=1234)
        r = pipe.generate_batch(prompts, max_tokens=8 * 5, do_sample=False)[0]     # >= 8 steps of K = 4
        runs.append((r["generated_tokens"], r["proposed"], r["accepted"]))
    assert runs[0] == runs[1]
    assert runs[1][1] >= 8 * 4 and 0 < runs[1][2] < runs[1][1]
