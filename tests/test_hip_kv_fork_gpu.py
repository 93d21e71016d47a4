"""KV fork on the device (csrc/kv_fork.hip through HipModel.fork_row / sd_model_kv_fork / sd_model_kv_copy_pages): bitwise copies
of the first n positions of a cache row (dense) or of pages (paged) into other rows, nothing else touched; and a fork followed by
the same forward gives the same cache as the row that computed the prefix itself."""

import ctypes

import pytest
import torch

from specdec_hip import _abi
from specdec_hip import weights as W

pytestmark = pytest.mark.gpu

N_POS = [0, 1, 7, 8, 9, 33, 95, 96]
LENGTHS = [1, 2, 31, 32, 33, 34, 64, 65, 66]


def _cfg(hkv=2, d=32, layers=2):
    return W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=layers, d_model=2 * hkv * d, n_heads=2 * hkv, n_kv_heads=hkv, head_dim=d, d_ff=4 * hkv * d,
                         vocab=1000, max_pos=512, rope_theta=500000.0, rope_scaling=None, tie_embeddings=False, name=f"fork-{hkv}-{d}")


_weights = {}


def _model(hkv=2, d=32, batch=4, l_max=96, **kw):
    from specdec_hip.engine import HipModel

    key = (hkv, d)
    if key not in _weights:
        _weights[key] = W.synthetic_llama(_cfg(hkv, d), seed=3, device="cpu", layer_gain=0.05).to("cuda")
    return HipModel(_weights[key], batch=batch, l_max=l_max, **kw)


def _fill(m, seed):
    """distinct random bf16 bit patterns in every element of both caches; -> int16 copies of them"""
    g = torch.Generator().manual_seed(seed)
    k, v = m.kv_view()
    for t in (k, v):
        bits = torch.randint(-32768, 32768, tuple(t.shape), generator=g, dtype=torch.int32).to(torch.int16)
        t.view(torch.int16).copy_(bits.cuda())
    torch.cuda.synchronize()
    return k.view(torch.int16).clone(), v.view(torch.int16).clone()


def _i32(xs):
    return (ctypes.c_int32 * max(len(xs), 1))(*xs)


@pytest.mark.parametrize("hkv,d", [(1, 32), (2, 32), (1, 128), (2, 128)])
def test_dense_fork_is_a_bitwise_copy_of_the_first_positions_only(hkv, d):
    m = _model(hkv, d)
    assert m.l_max == 96
    for n in N_POS:
        k0, v0 = _fill(m, 100 + n)
        m.fork_row(1, [0, 3], n)
        torch.cuda.synchronize()
        k, v = (t.view(torch.int16) for t in m.kv_view())
        want_k, want_v = k0.clone(), v0.clone()
        for dst in (0, 3):
            want_k[:, dst, :, :n] = k0[:, 1, :, :n]
            want_v[:, dst, :, :, :n] = v0[:, 1, :, :, :n]
        # the destinations' first n positions equal the source; positions >= n, row 2 and the source row are unchanged
        assert torch.equal(k, want_k), n
        assert torch.equal(v, want_v), n


@pytest.mark.parametrize("dsts", [[2], [3, 0, 2]])
def test_dense_fork_one_and_three_destinations(dsts):
    m = _model(2, 32)
    k0, v0 = _fill(m, 7)
    m.fork_row(1, dsts, 41)
    torch.cuda.synchronize()
    k, v = (t.view(torch.int16) for t in m.kv_view())
    want_k, want_v = k0.clone(), v0.clone()
    for dst in dsts:
        want_k[:, dst, :, :41] = k0[:, 1, :, :41]
        want_v[:, dst, :, :, :41] = v0[:, 1, :, :, :41]
    assert torch.equal(k, want_k) and torch.equal(v, want_v)


def test_geometry_refusals_on_bound_models_change_nothing():
    """The refusals that need a bound geometry (the argument-only ones: tests/test_kv_fork_abi.py)."""
    lib = _abi.load()
    dense, paged = _model(1, 32), _model(1, 32, page_len=32, n_pages=6)
    k0, v0 = _fill(dense, 1)
    fork = lambda src, dsts, n: lib.sd_model_kv_fork(dense.handle, src, _i32(dsts), len(dsts), n, None)
    for args, msg in (((4, [0], 4), "src_row 4 outside"), ((1, [0, 4], 4), "destination row 4 outside"), ((1, [0, 2, 0], 4), "listed twice"),
                      ((1, [0], 97), "exceeds Lmax=96")):
        assert fork(*args) != 0 and msg in _abi.last_error(), _abi.last_error()
    assert lib.sd_model_kv_copy_pages(dense.handle, _i32([0]), _i32([1]), 1, 4, None) != 0 and "dense cache" in _abi.last_error()
    torch.cuda.synchronize()
    k, v = (t.view(torch.int16) for t in dense.kv_view())
    assert torch.equal(k, k0) and torch.equal(v, v0)
    pk0, pv0 = _fill(paged, 2)
    copy = lambda s, d_, n: lib.sd_model_kv_copy_pages(paged.handle, _i32(s), _i32(d_), len(s), n, None)
    for args, msg in ((([0], [6], 4), "outside the pool of 6"), (([6], [0], 4), "outside the pool of 6"), (([0], [1], 33), "exceeds page_len=32"),
                      (([0, 2], [1, 1], 4), "listed twice"), (([0, 1], [1, 2], 4), "also a source")):
        assert copy(*args) != 0 and msg in _abi.last_error(), _abi.last_error()
    assert lib.sd_model_kv_fork(paged.handle, 0, _i32([1]), 1, 4, None) != 0 and "paged cache" in _abi.last_error()
    torch.cuda.synchronize()
    k, v = (t.view(torch.int16) for t in paged.kv_view())
    assert torch.equal(k, pk0) and torch.equal(v, pv0)
    # nothing to do: succeeds, launches nothing
    assert fork(1, [0], 0) == 0 and fork(1, [], 5) == 0 and copy([], [], 5) == 0 and copy([0], [1], 0) == 0


def test_page_pairs_beyond_the_per_launch_cap():
    """69 pairs (more than the 64 list entries one launch carries): page 0 and page 1 alternately into pages 2..70."""
    m = _model(2, 32, batch=2, l_max=64, page_len=32, n_pages=72)
    k0, v0 = _fill(m, 11)
    dst = list(range(2, 71))
    src = [i & 1 for i in range(len(dst))]
    _abi.check(m.lib.sd_model_kv_copy_pages(m.handle, _i32(src), _i32(dst), len(dst), 19, None), "sd_model_kv_copy_pages")
    torch.cuda.synchronize()
    k, v = (t.view(torch.int16) for t in m.kv_view())
    want_k, want_v = k0.clone(), v0.clone()
    for s, d_ in zip(src, dst):
        want_k[:, d_, :, :19] = k0[:, s, :, :19]
        want_v[:, d_, :, :, :19] = v0[:, s, :, :, :19]
    assert torch.equal(k, want_k) and torch.equal(v, want_v)      # page 71 and positions >= 19 untouched


def _gather(m, row, n):
    """positions [0, n) of a paged row through its block table -> (K int16 [layers][Hkv][n][D], V int16 [layers][Hkv][D][n])"""
    k, v = (t.view(torch.int16) for t in m.kv_view())
    table = m.block_table[row].cpu().tolist()
    P = m.page_len
    ks = [k[:, table[p // P], :, p % P] for p in range(n)]
    vs = [v[:, table[p // P], :, :, p % P] for p in range(n)]
    if not ks:
        return k[:, 0, :, :0].clone(), v[:, 0, :, :, :0].clone()
    return torch.stack(ks, dim=2), torch.stack(vs, dim=3)


@pytest.mark.parametrize("length", LENGTHS)
def test_paged_fork_shares_and_copies(length):
    m = _model(2, 32, batch=3, l_max=128, page_len=32, n_pages=16)
    V = m.cfg.vocab
    m.reserve(2, 1)
    m.reserve(1, length)
    k0, v0 = _fill(m, 200 + length)                     # the whole pool, the source's pages included
    src_pages = list(m._owned[1])
    want_k, want_v = _gather(m, 1, length)
    m.fork_row(1, [0], length)
    torch.cuda.synchronize()
    got_k, got_v = _gather(m, 0, length)
    assert torch.equal(got_k, want_k) and torch.equal(got_v, want_v)
    k, v = (t.view(torch.int16) for t in m.kv_view())
    for p in src_pages:                                  # the source's physical pages: unchanged
        assert torch.equal(k[:, p], k0[:, p]) and torch.equal(v[:, p], v0[:, p])
    n_share = max(length - 2, 0) // 32
    assert m._owned[0][:n_share] == src_pages[:n_share] and not set(m._owned[0][n_share:]) & set(src_pages)
    assert m.pages_in_use() == 1 + len(src_pages) + (len(src_pages) - n_share)
    # a forward of a few tokens on the destination at pos_base = length leaves the source's positions [0, length) alone
    toks = torch.randint(4, V, (1, 3), dtype=torch.int32, device="cuda")
    m.forward(toks, torch.tensor([length], dtype=torch.int32, device="cuda"), 0, skip_head=True, row0=0)
    torch.cuda.synchronize()
    again_k, again_v = _gather(m, 1, length)
    assert torch.equal(again_k, want_k) and torch.equal(again_v, want_v)
    got_k, got_v = _gather(m, 0, length)                 # ... and the destination's own forked positions too
    assert torch.equal(got_k, want_k) and torch.equal(got_v, want_v)
    for r in range(3):
        m.release(r)
    assert m.pages_in_use() == 0


@pytest.mark.parametrize("paged", [False, True])
def test_fork_then_forward_equals_forward_then_forward(paged):
    """Row A: forward(prefix), forward(suffix, pos_base=c). Row B: c positions forked from A after the prefix, then the same
    forward(suffix, pos_base=c). Their caches are bitwise equal over [0, c + len(suffix))."""
    c, s = 45, 21
    m = _model(2, 32, batch=2, l_max=96, **({"page_len": 32} if paged else {}))
    V = m.cfg.vocab
    g = torch.Generator().manual_seed(5)
    prefix = torch.randint(4, V, (1, c), generator=g, dtype=torch.int64).to(torch.int32).cuda()
    suffix = torch.randint(4, V, (1, s), generator=g, dtype=torch.int64).to(torch.int32).cuda()
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    at_c = torch.tensor([c], dtype=torch.int32, device="cuda")
    m.forward(prefix, zero, 0, skip_head=True, row0=0)
    m.fork_row(0, [1], c)
    m.forward(suffix, at_c, 0, skip_head=True, row0=0)
    m.forward(suffix, at_c, 0, skip_head=True, row0=1)
    torch.cuda.synchronize()
    n = c + s
    if paged:
        (ka, va), (kb, vb) = _gather(m, 0, n), _gather(m, 1, n)
    else:
        k, v = (t.view(torch.int16) for t in m.kv_view())
        (ka, va), (kb, vb) = (k[:, 0, :, :n], v[:, 0, :, :, :n]), (k[:, 1, :, :n], v[:, 1, :, :, :n])
    assert torch.equal(ka, kb) and torch.equal(va, vb)
    assert bool((ka != 0).any()) and bool((va != 0).any())
