"""KV eviction on the device (csrc/kv_evict.hip through HipModel.evict_row / sd_model_kv_evict): in one cache row, positions
[keep + drop, n_pos) become positions [keep, n_pos - drop) in place. V moves bit for bit; K is rotated by -drop positions and is
compared with the fp64 rotation of the stored values by the model's own fp32 table row, within the bound of
tests/rolling_ref.py (one bf16 rounding, two fp32 products, one fp32 addition); everything outside the destination range —
positions [0, keep), positions >= n_pos - drop, rows 0 and 2 — keeps its bits. The models are those of
tests/test_hip_kv_fork_gpu.py: 2 layers, batch 3, row 1 evicted.

The kernel walks a lane in chunks of 128 destination positions (kEvictChunk): (keep 4, drop 8, n_pos 500) moves 488 positions,
so every lane crosses three chunk boundaries while the move overlaps itself 60-fold."""

import itertools

import pytest
import torch

import rolling_ref as RR
from specdec_hip import _abi
from specdec_hip import weights as W

pytestmark = pytest.mark.gpu

GEOMETRIES = [(1, 32), (2, 32), (2, 64), (1, 128), (2, 128)]
KEEPS, DROPS = (0, 4, 8, 13), (8, 16, 40)
CHUNK = 128
ROW, BATCH = 1, 3


def _moved(drop):
    return sorted({0, 1, 7, 8, 9, drop - 1, drop, drop + 1, 2 * drop + 3})


def _cases(l_max):
    """(keep, drop, n_pos) that fit the cache, and on the larger cache the long overlapping move"""
    out = [(keep, drop, keep + drop + m) for keep, drop in itertools.product(KEEPS, DROPS) for m in _moved(drop) if keep + drop + m <= l_max]
    if l_max >= 512:
        out.append((4, 8, 500))
        assert (500 - 4 - 8) > 3 * CHUNK
    return out


def _cfg(hkv, d):
    return W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=2, d_model=2 * hkv * d, n_heads=2 * hkv, n_kv_heads=hkv, head_dim=d, d_ff=4 * hkv * d,
                         vocab=1000, max_pos=512, rope_theta=500000.0, rope_scaling=None, tie_embeddings=False, name=f"fork-{hkv}-{d}")


_weights = {}


def _model(hkv=2, d=32, l_max=96, **kw):
    from specdec_hip.engine import HipModel

    key = (hkv, d)
    if key not in _weights:
        _weights[key] = W.synthetic_llama(_cfg(hkv, d), seed=3, device="cpu", layer_gain=0.05).to("cuda")
    return HipModel(_weights[key], batch=BATCH, l_max=l_max, **kw)


def _fill_bits(m, seed):
    """distinct random bf16 bit patterns in every element of both caches (test_hip_kv_fork_gpu._fill, drawn on the device)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    for t in m.kv_view():
        t.view(torch.int16).copy_(torch.randint(-32768, 32768, tuple(t.shape), generator=g, dtype=torch.int32, device="cuda").to(torch.int16))
    torch.cuda.synchronize()


def _bits(m):
    return tuple(t.view(torch.int16).clone() for t in m.kv_view())


@pytest.mark.parametrize("l_max", [96, 512])
@pytest.mark.parametrize("hkv,d", GEOMETRIES)
def test_v_moves_bit_for_bit_and_nothing_else_changes(hkv, d, l_max):
    m = _model(hkv, d, l_max)
    assert m.l_max == l_max
    _fill_bits(m, 100 + l_max)
    for keep, drop, n_pos in _cases(l_max):
        k0, v0 = _bits(m)                                # (the previous case's result is this case's random content)
        m.evict_row(ROW, keep, drop, n_pos)
        torch.cuda.synchronize()
        k, v = _bits(m)
        end = n_pos - drop
        want_v = v0.clone()
        want_v[:, ROW, :, :, keep:end] = v0[:, ROW, :, :, keep + drop:n_pos]
        assert torch.equal(v, want_v), (keep, drop, n_pos)
        want_k = k0.clone()
        want_k[:, ROW, :, keep:end] = k[:, ROW, :, keep:end]     # K's destination range: test_k_is_rotated_within_the_derived_bound
        assert torch.equal(k, want_k), (keep, drop, n_pos)
    # K with arbitrary bit patterns: NaN and infinity go through the rotation without touching a neighbour (asserted above)


@pytest.mark.parametrize("l_max", [96, 512])
@pytest.mark.parametrize("hkv,d", GEOMETRIES)
def test_k_is_rotated_within_the_derived_bound(hkv, d, l_max):
    m = _model(hkv, d, l_max)
    cos, sin = _weights[(hkv, d)].rope_cos, _weights[(hkv, d)].rope_sin
    g = torch.Generator(device="cuda").manual_seed(7 + l_max)
    worst = 0.0
    for keep, drop, n_pos in _cases(l_max):
        k, v = m.kv_view()
        k.copy_(torch.randn(tuple(k.shape), generator=g, device="cuda").to(torch.bfloat16))     # finite normal values
        v.copy_(torch.randn(tuple(v.shape), generator=g, device="cuda").to(torch.bfloat16))
        torch.cuda.synchronize()
        want_k, bound, want_v = RR.evicted_cache(k, v, ROW, keep, drop, n_pos, cos[drop], sin[drop])
        m.evict_row(ROW, keep, drop, n_pos)
        torch.cuda.synchronize()
        err = (m.kv_view()[0].to(torch.float64) - want_k).abs()
        bad = err > bound                                  # bound 0 outside [keep, n_pos - drop) of row 1: unchanged there
        assert not bool(bad.any()), (keep, drop, n_pos, bad.nonzero()[:4].tolist(), float(err[bad].max()))
        assert torch.equal(m.kv_view()[1].view(torch.int16), want_v), (keep, drop, n_pos)
        if n_pos - keep - drop > 0:
            worst = max(worst, float((err / bound.clamp_min(1e-300))[bound > 0].max()))
    print(f"[kv_evict] hkv={hkv} D={d} l_max={l_max}: worst |got - want| / bound over {len(_cases(l_max))} cases {worst:.3f}")
    assert worst > 0.0     # (the rotation happened: a bit-exact K would mean nothing was rounded)


def test_refusals_change_nothing_and_the_empty_move_succeeds():
    lib = _abi.load()
    dense = _model(1, 32, 96)
    paged = _model(1, 32, 96, page_len=32, n_pages=9)
    g2 = W.ModelConfig(arch=W.ARCH_GPT2, n_layers=1, d_model=128, n_heads=2, n_kv_heads=2, head_dim=64, d_ff=512, vocab=512,
                       max_pos=256, tie_embeddings=True, name="gpt2-toy")
    from specdec_hip.engine import HipModel

    gpt2 = HipModel(W.synthetic_gpt2(g2, seed=1).to("cuda"), batch=BATCH, l_max=96)
    for mdl in (dense, paged, gpt2):
        _fill_bits(mdl, 5)
    before = [_bits(mdl) for mdl in (dense, paged, gpt2)]
    ev = lambda mdl, *a: lib.sd_model_kv_evict(mdl.handle, *a, None)
    # (row, keep, drop, n_pos) -> a piece of the message; max_pos of the dense model is 512, Lmax 96
    for args, msg in (((3, 4, 8, 40), "row 3 outside"), ((-1, 4, 8, 40), "row -1"), ((1, -1, 8, 40), "keep=-1"), ((1, 4, 0, 40), "drop=0"),
                      ((1, 4, -8, 40), "drop=-8"), ((1, 4, 12, 40), "drop=12"), ((1, 4, 512, 600), "rope positions"),
                      ((1, 4, 40, 43), "exceed n_pos=43"), ((1, 4, 8, 97), "exceeds Lmax=96")):
        assert ev(dense, *args) != 0 and msg in _abi.last_error() and _abi.last_error().startswith("kv_evict:"), (args, _abi.last_error())
    assert ev(paged, 1, 4, 8, 40) != 0 and "paged cache" in _abi.last_error()
    assert ev(gpt2, 1, 4, 8, 40) != 0 and "GPT-2" in _abi.last_error()
    with pytest.raises(_abi.HipLibraryError, match="paged cache"):
        paged.evict_row(1, 4, 8, 40)
    assert lib.sd_model_kv_evict(None, 1, 4, 8, 40, None) != 0 and "NULL model" in _abi.last_error()
    # nothing to move: succeeds, launches nothing
    assert ev(dense, 1, 4, 8, 12) == 0 and ev(dense, 1, 0, 96, 96) == 0
    torch.cuda.synchronize()
    for mdl, was in zip((dense, paged, gpt2), before):
        now = _bits(mdl)
        assert torch.equal(now[0], was[0]) and torch.equal(now[1], was[1])


def test_eviction_is_capturable_and_replays():
    """graph-capturable: no allocation, no synchronisation — captured once, replayed twice on fresh contents"""
    m = _model(2, 64, 512)
    keep, drop, n_pos = 4, 16, 300
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    _fill_bits(m, 9)
    with torch.cuda.stream(s):
        m.evict_row(ROW, keep, drop, n_pos, stream=s)     # (loads the code object before the capture)
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            m.evict_row(ROW, keep, drop, n_pos, stream=s)
    for seed in (10, 11):
        _fill_bits(m, seed)
        _, v0 = _bits(m)
        graph.replay()
        torch.cuda.synchronize()
        want = v0.clone()
        want[:, ROW, :, :, keep:n_pos - drop] = v0[:, ROW, :, :, keep + drop:n_pos]
        assert torch.equal(_bits(m)[1], want)
