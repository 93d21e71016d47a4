"""Tensor-level wrappers over the C-ABI ops (device memory + stream plumbing only).

These are the functions the kernel registry registers for device "cuda" (the
native device string of PyTorch-ROCm). Argument meaning and assertion behaviour
follow the reference contract in src/kernels/reference.py:13-159; the work is done
by the HIP kernels in csrc/. CPU tensors are rejected: there is no CPU fallback.
"""

from __future__ import annotations

import ctypes
import weakref
from typing import Dict, NamedTuple, Optional, Tuple

import torch

from . import _abi

_TORCH_TO_SD = {
    torch.float32: _abi.SD_F32,
    torch.float16: _abi.SD_F16,
    torch.bfloat16: _abi.SD_BF16,
    torch.int32: _abi.SD_I32,
    torch.int64: _abi.SD_I64,
    torch.uint8: _abi.SD_U8,
}


def sd_dtype(t: torch.dtype) -> int:
    try:
        return _TORCH_TO_SD[t]
    except KeyError:
        raise TypeError(f"dtype {t} is not supported by the HIP path") from None


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _require_device(name: str, *tensors: torch.Tensor) -> torch.device:
    dev = tensors[0].device
    for t in tensors:
        if t.device.type != "cuda":
            raise RuntimeError(
                f"{name}: the HIP path needs device tensors (got {t.device}); "
                "there is no CPU fallback in this build"
            )
        if t.device != dev:
            raise RuntimeError(f"{name}: tensors on different devices ({dev} vs {t.device})")
    return dev


# --------------------------------------------------------------------------- verify
def verify_prefix_workspace(B: int, K: int, V: int, device) -> torch.Tensor:
    """Scratch for verify_prefix_hip(..., workspace=): allocate once, reuse for every call of that shape or smaller."""
    return torch.empty(max(_abi.load().sd_verify_prefix_workspace(B, K, V), 1), dtype=torch.uint8, device=device)


def verify_prefix_hip(
    logits: torch.Tensor, draft_ids: torch.Tensor, return_pred: bool = False,
    out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, workspace: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, ...]:
    """accept_len[B] int32, accepted_mask[B,K] uint8 (reference.py:13-56) on gfx950.

    With return_pred=True also returns the argmax ids [B,K] int32. `out` = (accept_len, mask) and `workspace`
    (verify_prefix_workspace) make the call allocation-free, which is what a captured graph needs.
    """
    assert logits.dim() == 3, "logits must be 3D tensor [B][K][V]"
    assert draft_ids.dim() == 2, "draft_ids must be 2D tensor [B][K]"
    assert logits.size(0) == draft_ids.size(0), "Batch size mismatch"
    assert logits.size(1) == draft_ids.size(1), "K dimension mismatch"
    dev = _require_device("verify_prefix", logits, draft_ids)
    if logits.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"verify_prefix: logits dtype {logits.dtype} not supported (f32/f16/bf16)")
    if draft_ids.dtype not in (torch.int32, torch.int64):
        if draft_ids.dtype.is_floating_point or draft_ids.dtype == torch.bool:
            raise TypeError(f"verify_prefix: draft_ids dtype {draft_ids.dtype} is not an integer type")
        draft_ids = draft_ids.to(torch.int64)
    B, K, V = logits.shape
    if V > 0 and logits.stride(2) != 1:
        logits = logits.contiguous()
    ids = draft_ids.contiguous()
    if out is not None:
        accept_len, mask = out
        assert accept_len.dtype == torch.int32 and accept_len.shape == (B,) and accept_len.is_contiguous() and accept_len.device == dev
        assert mask.dtype == torch.uint8 and mask.shape == (B, K) and mask.is_contiguous() and mask.device == dev
    else:
        accept_len = torch.empty(B, dtype=torch.int32, device=dev)
        mask = torch.empty((B, K), dtype=torch.uint8, device=dev)
    pred = torch.empty((B, K), dtype=torch.int32, device=dev) if return_pred else None
    if B == 0:
        return (accept_len, mask, pred) if return_pred else (accept_len, mask)
    lib = _abi.load()
    ws_bytes = lib.sd_verify_prefix_workspace(B, K, V)
    ws = workspace if workspace is not None else torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    assert ws.device == dev and ws.numel() >= ws_bytes, "verify_prefix: workspace too small"
    with torch.cuda.device(dev):
        rc = lib.sd_verify_prefix(
            logits.data_ptr(), sd_dtype(logits.dtype), ids.data_ptr(), sd_dtype(ids.dtype),
            accept_len.data_ptr(), mask.data_ptr(), pred.data_ptr() if pred is not None else None,
            B, K, V, logits.stride(0), logits.stride(1),
            ws.data_ptr(), ws.numel(), _stream_ptr(dev),
        )
    _abi.check(rc, "sd_verify_prefix")
    return (accept_len, mask, pred) if return_pred else (accept_len, mask)


# ------------------------------------------------------------------------ kv append
class _Arena:
    """A [B,H,cap,D] pair of buffers that kv_append_hip grows in place.

    It lives exactly as long as the newest view handed out of it: each hand-out
    bumps `gen` and arms a finalizer on the returned K view that retires the arena
    if no newer view has replaced it.
    """

    __slots__ = ("k", "v", "frontier", "gen")

    def __init__(self, k: torch.Tensor, v: torch.Tensor, frontier: int):
        self.k, self.v, self.frontier, self.gen = k, v, frontier, 0


# storage pointer of an arena's K buffer -> arena
_arenas: Dict[int, _Arena] = {}


def _retire(key: int, gen: int) -> None:
    ar = _arenas.get(key)
    if ar is not None and ar.gen == gen:
        del _arenas[key]


def _hand_out(key: int, ar: _Arena, rows: int) -> Tuple[torch.Tensor, torch.Tensor]:
    ar.frontier = rows
    ar.gen += 1
    vk, vv = ar.k[:, :, :rows], ar.v[:, :, :rows]
    weakref.finalize(vk, _retire, key, ar.gen)
    return vk, vv


def _find_arena(base_k: torch.Tensor, base_v: torch.Tensor) -> Optional[_Arena]:
    ar = _arenas.get(base_k.untyped_storage().data_ptr())
    if ar is None:
        return None
    B, H, L, D = base_k.shape
    cap = ar.k.shape[2]
    ok = (
        ar.k.dtype == base_k.dtype
        and ar.k.shape[0] == B and ar.k.shape[1] == H and ar.k.shape[3] == D
        and base_k.data_ptr() == ar.k.data_ptr() and base_v.data_ptr() == ar.v.data_ptr()
        and base_k.stride() == ar.k.stride() and base_v.stride() == ar.v.stride()
        and L == ar.frontier and L <= cap
    )
    return ar if ok else None


def _check_kv_shapes(base_k, base_v, new_k, new_v):
    assert base_k.dim() == 4, "base_k must be 4D tensor [B][H][L][D]"
    assert base_v.dim() == 4, "base_v must be 4D tensor [B][H][L][D]"
    assert new_k.dim() == 4, "new_k must be 4D tensor [B][H][K][D]"
    assert new_v.dim() == 4, "new_v must be 4D tensor [B][H][K][D]"
    assert base_k.shape[0] == new_k.shape[0], "Batch size mismatch"
    assert base_k.shape[1] == new_k.shape[1], "Num heads mismatch"
    assert base_k.shape[3] == new_k.shape[3], "Head dim mismatch"


def _row_major(t: torch.Tensor) -> torch.Tensor:
    """Rows of D contiguous elements at stride D (strided b/h allowed)."""
    if t.shape[3] == 0 or t.shape[2] == 0:
        return t
    if t.stride(3) == 1 and (t.stride(2) == t.shape[3] or t.shape[2] == 1):
        return t
    return t.contiguous()


def kv_append_hip(
    base_k: torch.Tensor, base_v: torch.Tensor, new_k: torch.Tensor, new_v: torch.Tensor
) -> Tuple[torch.Tensor, torch.Tensor]:
    """[B,H,L,D] + [B,H,K,D] -> [B,H,L+K,D] (reference.py:59-93) on gfx950.

    The result is a view of a runtime-owned [B,H,cap,D] arena. When `base_*` is
    the result of the previous call and has not been appended to since, the K new
    rows are written in place behind it (sd_kv_append: 2*B*H*K*D elements moved,
    not the reference's re-copy of all L rows) and a longer view is returned; the
    rows [0,L) that `base_*` views are never modified. Any other base is copied
    once into a fresh arena (sd_kv_concat).
    """
    _check_kv_shapes(base_k, base_v, new_k, new_v)
    dev = _require_device("kv_append", base_k, base_v, new_k, new_v)
    if not (base_k.dtype == base_v.dtype == new_k.dtype == new_v.dtype):
        raise TypeError("kv_append: base/new dtypes differ")
    esize = base_k.element_size()
    if esize not in (2, 4):
        raise TypeError(f"kv_append: element size {esize} not supported")
    assert base_v.shape == base_k.shape and new_v.shape == new_k.shape, "K/V shape mismatch"
    B, H, L, D = base_k.shape
    K = new_k.shape[2]
    lib = _abi.load()
    new_k = new_k.contiguous()
    new_v = new_v.contiguous()

    ar = _find_arena(base_k, base_v)
    if ar is not None and L + K <= ar.k.shape[2]:
        with torch.cuda.device(dev):
            rc = lib.sd_kv_append(
                ar.k.data_ptr(), ar.v.data_ptr(), new_k.data_ptr(), new_v.data_ptr(),
                None, L, esize, B, H, ar.k.shape[2], K, D, _stream_ptr(dev),
            )
        _abi.check(rc, "sd_kv_append")
        return _hand_out(ar.k.untyped_storage().data_ptr(), ar, L + K)

    # fresh arena with head-room: amortised O(K) per later append
    cap = max(L + K, 1)
    cap = max(cap + max(64, cap // 2), 2 * K)
    buf_k = torch.empty((B, H, cap, D), dtype=base_k.dtype, device=dev)
    buf_v = torch.empty((B, H, cap, D), dtype=base_k.dtype, device=dev)
    bk, bv = _row_major(base_k), _row_major(base_v)
    if bv.stride()[:2] != bk.stride()[:2]:
        bk, bv = bk.contiguous(), bv.contiguous()
    if B * H * D > 0 and L + K > 0:
        with torch.cuda.device(dev):
            rc = lib.sd_kv_concat(
                buf_k.data_ptr(), buf_v.data_ptr(), bk.data_ptr(), bv.data_ptr(),
                new_k.data_ptr(), new_v.data_ptr(), esize, B, H, L, K, D, cap,
                bk.stride(0) if L else 0, bk.stride(1) if L else 0, _stream_ptr(dev),
            )
        _abi.check(rc, "sd_kv_concat")
    ar = _Arena(buf_k, buf_v, L + K)
    key = buf_k.untyped_storage().data_ptr()
    _arenas[key] = ar
    return _hand_out(key, ar, L + K)


def kv_concat_hip(base_k, base_v, new_k, new_v):
    """Plain out-of-place form: fresh contiguous [B,H,L+K,D] tensors (sd_kv_concat)."""
    _check_kv_shapes(base_k, base_v, new_k, new_v)
    dev = _require_device("kv_concat", base_k, base_v, new_k, new_v)
    esize = base_k.element_size()
    B, H, L, D = base_k.shape
    K = new_k.shape[2]
    bk, bv = _row_major(base_k), _row_major(base_v)
    if bv.stride()[:2] != bk.stride()[:2]:
        bk, bv = bk.contiguous(), bv.contiguous()
    new_k, new_v = new_k.contiguous(), new_v.contiguous()
    out_k = torch.empty((B, H, L + K, D), dtype=base_k.dtype, device=dev)
    out_v = torch.empty((B, H, L + K, D), dtype=base_k.dtype, device=dev)
    with torch.cuda.device(dev):
        rc = _abi.load().sd_kv_concat(
            out_k.data_ptr(), out_v.data_ptr(), bk.data_ptr(), bv.data_ptr(),
            new_k.data_ptr(), new_v.data_ptr(), esize, B, H, L, K, D, L + K,
            bk.stride(0) if L else 0, bk.stride(1) if L else 0, _stream_ptr(dev),
        )
    _abi.check(rc, "sd_kv_concat")
    return out_k, out_v


def kv_append_inplace_hip(
    cache_k: torch.Tensor, cache_v: torch.Tensor, new_k: torch.Tensor, new_v: torch.Tensor,
    row_len: Optional[torch.Tensor] = None, L: int = 0,
) -> None:
    """Write new[b,h,:,:] into cache[b,h,row_len[b]:row_len[b]+K,:] (sd_kv_append)."""
    dev = _require_device("kv_append_inplace", cache_k, cache_v, new_k, new_v)
    assert cache_k.is_contiguous() and cache_v.is_contiguous(), "cache must be contiguous"
    B, H, Lmax, D = cache_k.shape
    K = new_k.shape[2]
    assert new_k.shape == (B, H, K, D) and new_v.shape == (B, H, K, D), "new_k/new_v shape mismatch"
    if row_len is not None:
        assert row_len.dtype == torch.int32 and row_len.shape == (B,) and row_len.device == dev
    new_k, new_v = new_k.contiguous(), new_v.contiguous()
    with torch.cuda.device(dev):
        rc = _abi.load().sd_kv_append(
            cache_k.data_ptr(), cache_v.data_ptr(), new_k.data_ptr(), new_v.data_ptr(),
            row_len.data_ptr() if row_len is not None else None, L,
            cache_k.element_size(), B, H, Lmax, K, D, _stream_ptr(dev),
        )
    _abi.check(rc, "sd_kv_append")


def kv_append_with_mask_hip(
    base_k: torch.Tensor, base_v: torch.Tensor, draft_k: torch.Tensor, draft_v: torch.Tensor,
    accepted_mask: torch.Tensor, accept_len: torch.Tensor, offset: int = 0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Compacting append (reference.py:96-159) on gfx950; `offset` is unused there too."""
    assert base_k.dim() == 4, "base_k must be 4D tensor [B][H][L][D]"
    assert base_v.dim() == 4, "base_v must be 4D tensor [B][H][L][D]"
    assert draft_k.dim() == 4, "draft_k must be 4D tensor [B][H][K][D]"
    assert draft_v.dim() == 4, "draft_v must be 4D tensor [B][H][K][D]"
    assert accepted_mask.dim() == 2, "accepted_mask must be 2D tensor [B][K]"
    assert accept_len.dim() == 1, "accept_len must be 1D tensor [B]"
    dev = _require_device("kv_append_with_mask", base_k, base_v, draft_k, draft_v, accepted_mask, accept_len)
    B, H, L, D = base_k.shape
    K = draft_k.shape[2]
    esize = base_k.element_size()
    bk, bv = _row_major(base_k), _row_major(base_v)
    if bv.stride()[:2] != bk.stride()[:2]:
        bk, bv = bk.contiguous(), bv.contiguous()
    draft_k, draft_v = draft_k.contiguous(), draft_v.contiguous()
    mask = (accepted_mask != 0).to(torch.uint8).contiguous()
    alen = accept_len.to(torch.int32).contiguous()
    out_k = torch.empty((B, H, L + K, D), dtype=base_k.dtype, device=dev)
    out_v = torch.empty((B, H, L + K, D), dtype=base_v.dtype, device=dev)
    with torch.cuda.device(dev):
        rc = _abi.load().sd_kv_append_masked(
            out_k.data_ptr(), out_v.data_ptr(), bk.data_ptr(), bv.data_ptr(),
            draft_k.data_ptr(), draft_v.data_ptr(), mask.data_ptr(), alen.data_ptr(),
            esize, B, H, L, K, D, bk.stride(0) if L else 0, bk.stride(1) if L else 0,
            _stream_ptr(dev),
        )
    _abi.check(rc, "sd_kv_append_masked")
    return out_k, out_v


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return t.data_ptr() if t is not None else None


def _check_entry_vectors(name: str, B: int, dev, **tensors: Optional[torch.Tensor]) -> None:
    """The optional per-entry vectors of an op (pos, draw_counters, stream_ids, active, ...), by argument name."""
    for arg, t in tensors.items():
        if t is not None and (t.device != dev or t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous()):
            raise ValueError(f"{name}: {arg} must be a contiguous int32 [{B}] tensor on {dev}")


def _entry_rows(name: str, logits: torch.Tensor, rows_per_entry: int):
    """The [rows, V] logits of a draw op, unit stride along V -> (logits, device, entries, V)."""
    if logits.dim() == 1:
        logits = logits.unsqueeze(0)
    if logits.dim() != 2:
        raise ValueError(f"{name}: logits must be [rows, V], got {tuple(logits.shape)}")
    dev = _require_device(name, logits)
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    rows, V = logits.shape
    if rows % rows_per_entry:
        raise ValueError(f"{name}: {rows} rows is not a multiple of rows_per_entry={rows_per_entry}")
    return logits, dev, rows // rows_per_entry, V


def _sample_token(name: str, logits, draw, pos, rows_per_entry, draw_counters, stream_ids, active, scalars=None, table=None) -> torch.Tensor:
    """sample_token_hip (`scalars`: temperature, top_k, top_p, seed as the library takes them) / sample_token_rows_hip (`table`)."""
    lib = _abi.load()
    logits, dev, B, V = _entry_rows(name, logits, rows_per_entry)
    _check_entry_vectors(name, B, dev, pos=pos, draw_counters=draw_counters, stream_ids=stream_ids, active=active)
    if table is not None:
        table = _row_table(name, table, B, dev)
    out = torch.empty(B, dtype=torch.int32, device=dev)
    head = (logits.data_ptr(), sd_dtype(logits.dtype), logits.stride(0), B, V, _ptr(pos), int(rows_per_entry), _ptr(active))
    tail = (_ptr(draw_counters), int(draw) & 0xFFFFFFFF, _ptr(stream_ids), out.data_ptr(), _stream_ptr(dev))
    with torch.cuda.device(dev):
        if table is None:
            _abi.check(lib.sd_sample_token(*head, *scalars, *tail), "sd_sample_token")
        else:
            _abi.check(lib.sd_sample_token_rows(*head, table.data_ptr(), *tail), "sd_sample_token_rows")
    return out


def sample_token_hip(logits: torch.Tensor, temperature: float, top_k: Optional[int] = None, top_p: Optional[float] = None,
                     seed: int = 0, draw: int = 0, pos: Optional[torch.Tensor] = None, rows_per_entry: int = 1,
                     draw_counters: Optional[torch.Tensor] = None, stream_ids: Optional[torch.Tensor] = None,
                     active: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sampled token per entry (sd_sample_token): the device form of the reference's
    `sample_bonus_token_from_logits(..., do_sample=True)` (src/specdec/core/pipeline.py:48-147).

    logits: [rows, V] (or [V]) f32/bf16/f16 on the GPU, unit stride along V. Entry b reads row
    b*rows_per_entry + pos[b]. Returns int32 [entries]. `draw` (or the int32 `draw_counters`, read
    and incremented on the device) and `stream_ids` select the Philox value; see include/specdec_hip.h."""
    scalars = (float(temperature), int(top_k) if top_k else 0, 1.0 if top_p is None else float(top_p), int(seed) & (2 ** 64 - 1))
    return _sample_token("sample_token", logits, draw, pos, rows_per_entry, draw_counters, stream_ids, active, scalars=scalars)


def _spec_triple(name: str, draft_logits: torch.Tensor, target_logits: torch.Tensor, draft_ids: torch.Tensor):
    """(draft_logits [B,K,V], target_logits [B,K+1,V], draft_ids [B,K]) of a speculative-sampling op, made contiguous
    -> (draft_logits, target_logits, draft_ids, device, B, K, V)."""
    dev = _require_device(name, draft_logits, target_logits, draft_ids)
    if draft_logits.dim() != 3 or target_logits.dim() != 3 or draft_ids.dim() != 2:
        raise ValueError(f"{name}: need draft_logits [B,K,V], target_logits [B,K+1,V], draft_ids [B,K]")
    B, K, V = draft_logits.shape
    if tuple(target_logits.shape) != (B, K + 1, V) or tuple(draft_ids.shape) != (B, K):
        raise ValueError(f"{name}: shapes {tuple(draft_logits.shape)} / {tuple(target_logits.shape)} / {tuple(draft_ids.shape)}")
    if draft_logits.dtype != torch.bfloat16 or target_logits.dtype != torch.bfloat16 or draft_ids.dtype != torch.int32:
        raise TypeError(f"{name}: logits must be bfloat16 and draft_ids int32")
    return draft_logits.contiguous(), target_logits.contiguous(), draft_ids.contiguous(), dev, B, K, V


def _spec_sample_accept(name: str, draft_logits, target_logits, draft_ids, draw, draw_counters, stream_ids, active, return_ratios,
                        symbol: str = "sd_spec_sample_accept_rows", scalars: tuple = (), table=None):
    """spec_sample_accept_hip (`symbol`: the shaped or the unshaped entry point, `scalars`: what it takes between V and the draw
    counters) / spec_sample_accept_rows_hip (`table` in their place)."""
    lib = _abi.load()
    draft_logits, target_logits, draft_ids, dev, B, K, V = _spec_triple(name, draft_logits, target_logits, draft_ids)
    _check_entry_vectors(name, B, dev, draw_counters=draw_counters, stream_ids=stream_ids, active=active)
    params = scalars if table is None else (_row_table(name, table, B, dev).data_ptr(),)
    accept = torch.zeros(B, dtype=torch.int32, device=dev)
    nxt = torch.full((B,), -1, dtype=torch.int32, device=dev)
    ratios = torch.full((B, K), float("nan"), dtype=torch.float64, device=dev) if return_ratios else None
    ws = torch.empty(max(lib.sd_spec_sample_workspace(B, K), 4), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _abi.check(getattr(lib, symbol)(
            draft_logits.data_ptr(), target_logits.data_ptr(), draft_ids.data_ptr(), B, K, V, *params, _ptr(draw_counters),
            int(draw) & 0xFFFFFFFF, _ptr(stream_ids), _ptr(active), accept.data_ptr(), nxt.data_ptr(), _ptr(ratios), ws.data_ptr(),
            ws.numel(), _stream_ptr(dev)), symbol)
    return (accept, nxt, ratios) if return_ratios else (accept, nxt)


def spec_sample_accept_hip(draft_logits: torch.Tensor, target_logits: torch.Tensor, draft_ids: torch.Tensor, temperature: float,
                           seed: int = 0, draw: int = 0, draw_counters: Optional[torch.Tensor] = None,
                           stream_ids: Optional[torch.Tensor] = None, active: Optional[torch.Tensor] = None,
                           return_ratios: bool = False, top_k: Optional[int] = None, top_p: Optional[float] = None):
    """Acceptance and next token of speculative sampling (sd_spec_sample_accept) on caller tensors. With `top_k` (1..1024),
    optionally `top_p` < 1, both distributions are shaped as sd_sample_token shapes them (sd_spec_sample_accept_shaped: the
    draft ids are then draws of sample_token_hip(q_i, top_k, top_p), the next token an inversion draw); `top_p` without
    `top_k` is refused by the library.

    draft_logits bf16 [B, K, V] (q_i), target_logits bf16 [B, K+1, V] (p_i), draft_ids int32 [B, K] (the tokens drawn from
    q_i). Returns (accept_len int32 [B], next_tok int32 [B]) and, with return_ratios, the float64 [B, K] ratios
    p_i(d)/q_i(d). Row b's draws use counter `draw` (or the int32 `draw_counters`, advanced by K + 1 on the device) and
    Philox stream stream_ids[b] (default b); see include/specdec_hip.h for the schedule."""
    seed = int(seed) & (2 ** 64 - 1)
    if top_k or (top_p is not None and float(top_p) < 1.0):
        symbol = "sd_spec_sample_accept_shaped"
        scalars = (float(temperature), int(top_k) if top_k else 0, 1.0 if top_p is None else float(top_p), seed)
    else:
        symbol, scalars = "sd_spec_sample_accept", (float(temperature), seed)
    return _spec_sample_accept("spec_sample_accept", draft_logits, target_logits, draft_ids, draw, draw_counters, stream_ids, active,
                               return_ratios, symbol, scalars)


def typical_accept_workspace(B: int, K: int, V: int, device) -> torch.Tensor:
    """Scratch for typical_accept(..., workspace=): allocate once, reuse for every call of that shape or smaller."""
    return torch.empty(max(_abi.load().sd_typical_accept_workspace(B, K, V), 4), dtype=torch.uint8, device=device)


def typical_accept(target_logits: torch.Tensor, draft_ids: torch.Tensor, rule: str = "typical", temperature: float = 1.0,
                   epsilon: float = 0.09, delta: Optional[float] = 0.3, agree_k: int = 1, return_stats: bool = False,
                   out: Optional[torch.Tensor] = None, stats_out: Optional[torch.Tensor] = None,
                   workspace: Optional[torch.Tensor] = None):
    """Accept lengths of a lossy acceptance rule on the verify pass's logits (sd_typical_accept).

    target_logits: [B, K+1, V] f32 / bf16 / f16 on the GPU, unit stride along V, rows at one stride (a view whose rows are
    further apart than V is taken as it is); draft_ids int32 [B, K]. rule "typical": position i is kept iff
    p_i(d) >= min(epsilon, delta * exp(-H(p_i))) at `temperature` (delta None: the fixed threshold epsilon); rule "topk_agree":
    iff d is among the row's `agree_k` largest logits (ties to the lower index). Returns accept_len int32 [B] — the leading
    kept positions — and with return_stats the float32 [B, K, 4] records (p_d, H, threshold, rank_d). `out`, `stats_out` and
    `workspace` (typical_accept_workspace) make the call allocation-free, which is what a captured graph needs."""
    lib = _abi.load()
    dev = _require_device("typical_accept", target_logits, draft_ids)
    if rule not in _abi.ACCEPT_RULES:
        raise ValueError(f"typical_accept: rule {rule!r} (one of {sorted(_abi.ACCEPT_RULES)})")
    if target_logits.dim() != 3 or draft_ids.dim() != 2:
        raise ValueError("typical_accept: need target_logits [B,K+1,V] and draft_ids [B,K]")
    B, K1, V = target_logits.shape
    K = K1 - 1
    if tuple(draft_ids.shape) != (B, K):
        raise ValueError(f"typical_accept: shapes {tuple(target_logits.shape)} / {tuple(draft_ids.shape)}")
    if draft_ids.dtype != torch.int32:
        raise TypeError("typical_accept: draft_ids must be int32")
    if target_logits.stride(2) != 1 or target_logits.stride(0) != K1 * target_logits.stride(1):
        target_logits = target_logits.contiguous()
    draft_ids = draft_ids.contiguous()
    if out is None:
        out = torch.zeros(B, dtype=torch.int32, device=dev)
    elif out.dtype != torch.int32 or tuple(out.shape) != (B,) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"typical_accept: out must be a contiguous int32 [{B}] tensor on {dev}")
    stats = stats_out
    if stats is None and return_stats:
        stats = torch.full((B, max(K, 0), 4), float("nan"), dtype=torch.float32, device=dev)
    if stats is not None and (stats.dtype != torch.float32 or tuple(stats.shape) != (B, K, 4) or not stats.is_contiguous() or stats.device != dev):
        raise ValueError(f"typical_accept: stats_out must be a contiguous float32 [{B}][{K}][4] tensor on {dev}")
    ws = workspace if workspace is not None else typical_accept_workspace(B, K, V, dev)
    with torch.cuda.device(dev):
        _abi.check(lib.sd_typical_accept(target_logits.data_ptr(), sd_dtype(target_logits.dtype), target_logits.stride(1),
                                         draft_ids.data_ptr(), B, K, V, _abi.ACCEPT_RULES[rule], float(temperature), float(epsilon),
                                         float("inf") if delta is None else float(delta), int(agree_k), out.data_ptr(),
                                         stats.data_ptr() if stats is not None else None, ws.data_ptr(), ws.numel(),
                                         _stream_ptr(dev)), "sd_typical_accept")
    return (out, stats) if (return_stats or stats_out is not None) else out


def draft_confidence(logits: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The confidence of every row of `logits` (sd_draft_confidence): 1 / sum_v exp(x_v - max x), the temperature-1 softmax
    probability of the row's largest stored value — what the confidence-gated step (HipSpecDec.set_draft_confidence) judges a
    draft forward by.

    logits: [B, V] f32 / bf16 / f16 on the GPU, unit stride along V; a view whose rows are further apart than V, or start off a
    16-byte boundary, is taken as it is. Returns float32 [B]; NaN for a row with a NaN, a +inf, or nothing above -inf. `out`
    (contiguous float32 [B]) makes the call allocation-free."""
    lib = _abi.load()
    dev = _require_device("draft_confidence", logits)
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError("draft_confidence: need logits [B, V]")
    if logits.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"draft_confidence: logits must be float32, float16 or bfloat16, got {logits.dtype}")
    B, V = logits.shape
    if logits.stride(1) != 1 or (B > 1 and logits.stride(0) < V):
        logits = logits.contiguous()
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B,) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"draft_confidence: out must be a contiguous float32 [{B}] tensor on {dev}")
    with torch.cuda.device(dev):
        _abi.check(lib.sd_draft_confidence(logits.data_ptr(), sd_dtype(logits.dtype), logits.stride(0) if B > 1 else V, B, V,
                                           out.data_ptr(), _stream_ptr(dev)), "sd_draft_confidence")
    return out


class TokenLogprobs(NamedTuple):
    logprob: torch.Tensor        # float32 [R]
    rank: torch.Tensor           # int32 [R]
    top_ids: torch.Tensor        # int32 [R][N]
    top_logprobs: torch.Tensor   # float32 [R][N]


def token_logprobs(logits: torch.Tensor, token_ids, top_n: int = 0, out: Optional[TokenLogprobs] = None) -> TokenLogprobs:
    """Log-prob, rank and the top-N alternatives of one token per logits row (sd_token_logprobs), at temperature 1 over the
    stored values: logprob = (x_t - max) - log sum exp(x - max), rank = the entries that beat x_t under the argmax kernels' ties
    (0: the row's argmax), the N = min(top_n, V) largest entries (value descending, index ascending) as ids and log-probs.

    logits: [R, V] f32 / bf16 / f16 on the GPU, unit stride along V; a view whose rows are further apart than V, or start off a
    16-byte boundary, is taken as it is. token_ids: R ids, a host sequence (checked against [0, V) here) or an int32 tensor [R]
    on the device (an id outside the vocabulary then yields the NaN / -1 record). top_n in 0..20. A token at -inf has logprob
    -inf; a row with nothing above -inf gives logprob NaN, rank -1 and top ids -1. `out` (contiguous tensors of the result's
    shapes) makes the call allocation-free."""
    lib = _abi.load()
    dev = _require_device("token_logprobs", logits)
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError("token_logprobs: need logits [R, V]")
    if logits.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"token_logprobs: logits must be float32, float16 or bfloat16, got {logits.dtype}")
    R, V = logits.shape
    top_n = int(top_n)
    if not 0 <= top_n <= 20:
        raise ValueError(f"token_logprobs: top_n {top_n} outside 0..20")
    if isinstance(token_ids, torch.Tensor) and token_ids.is_cuda:
        if token_ids.dtype != torch.int32 or tuple(token_ids.shape) != (R,) or token_ids.device != dev:
            raise ValueError(f"token_logprobs: token_ids must be int32 [{R}] on {dev}")
        ids = token_ids.contiguous()
    else:
        host = [int(t) for t in (token_ids.tolist() if isinstance(token_ids, torch.Tensor) else token_ids)]
        if len(host) != R:
            raise ValueError(f"token_logprobs: {len(host)} token ids for {R} rows")
        bad = [t for t in host if not 0 <= t < V]
        if bad:
            raise ValueError(f"token_logprobs: token id {bad[0]} outside [0, {V})")
        ids = torch.tensor(host, dtype=torch.int32, device=dev)
    if logits.stride(1) != 1 or (R > 1 and logits.stride(0) < V):
        logits = logits.contiguous()
    N = min(top_n, V)
    if out is None:
        out = TokenLogprobs(torch.empty(R, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.int32, device=dev),
                            torch.empty((R, N), dtype=torch.int32, device=dev), torch.empty((R, N), dtype=torch.float32, device=dev))
    else:
        want = ((R,), torch.float32), ((R,), torch.int32), ((R, N), torch.int32), ((R, N), torch.float32)
        for t, (shape, dt) in zip(out, want):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"token_logprobs: out must hold contiguous tensors {want} on {dev}")
    with torch.cuda.device(dev):
        _abi.check(lib.sd_token_logprobs(logits.data_ptr(), sd_dtype(logits.dtype), logits.stride(0) if R > 1 else V, R, V, ids.data_ptr(),
                                         top_n, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr() if N else None,
                                         out[3].data_ptr() if N else None, _stream_ptr(dev)), "sd_token_logprobs")
    return out


def _row_table(name: str, table, B: int, dev) -> torch.Tensor:
    """The device table of a _rows op: a list of SamplingParams is packed, a tensor (sampling_params.pack: uint8 [B][32]) is
    taken as it is."""
    from .sampling_params import ROW_BYTES, pack

    if not isinstance(table, torch.Tensor):
        table = pack(list(table), dev)
    if table.dtype != torch.uint8 or table.device != dev or not table.is_contiguous() or table.numel() != B * ROW_BYTES:
        raise ValueError(f"{name}: the table must be a contiguous uint8 [{B}][{ROW_BYTES}] tensor on {dev} (sampling_params.pack)")
    return table


def sample_token_rows_hip(logits: torch.Tensor, table, draw: int = 0, pos: Optional[torch.Tensor] = None, rows_per_entry: int = 1,
                          draw_counters: Optional[torch.Tensor] = None, stream_ids: Optional[torch.Tensor] = None,
                          active: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sample_token_hip with every entry's own temperature, top_k, top_p and seed (sd_sample_token_rows): `table` is a list of
    SamplingParams, one per entry, or their packed tensor. Entry b's result is that of sample_token_hip on its row alone with
    its normalised parameters, the same draw and the same stream id."""
    return _sample_token("sample_token_rows", logits, draw, pos, rows_per_entry, draw_counters, stream_ids, active, table=table)


def spec_sample_accept_rows_hip(draft_logits: torch.Tensor, target_logits: torch.Tensor, draft_ids: torch.Tensor, table, draw: int = 0,
                                draw_counters: Optional[torch.Tensor] = None, stream_ids: Optional[torch.Tensor] = None,
                                active: Optional[torch.Tensor] = None, return_ratios: bool = False):
    """spec_sample_accept_hip with every row's own temperature, top_k, top_p and seed (sd_spec_sample_accept_rows): a row
    without top_k and top_p runs the unshaped statistics, any other row the shaped ones; a row the speculative-sampling
    kernels cannot honour (temperature 0, top_p without top_k, ...) is a greedy row. Shapes and results as
    spec_sample_accept_hip."""
    return _spec_sample_accept("spec_sample_accept_rows", draft_logits, target_logits, draft_ids, draw, draw_counters, stream_ids, active,
                               return_ratios, table=table)


def logit_counts(B: int, V: int, device) -> torch.Tensor:
    """A zeroed counts table for the logit processors: int16 [B][V] holding the uint16 words of sd_logit_process (bit 15: the
    token is in the row's prompt, i.e. a negative int16; bits 0..14: times generated, saturating at 32767)."""
    return torch.zeros((int(B), int(V)), dtype=torch.int16, device=device)


def _check_counts(name: str, counts: torch.Tensor, dev) -> Tuple[int, int]:
    if counts.dim() != 2 or counts.dtype != torch.int16 or counts.device != dev or not counts.is_contiguous():
        raise ValueError(f"{name}: counts must be a contiguous int16 [B][V] tensor on {dev} (logit_counts)")
    return int(counts.shape[0]), int(counts.shape[1])


def _check_fsm(name: str, nxt: torch.Tensor, allow: torch.Tensor, fsm_state: torch.Tensor, B: int, V: int, dev) -> int:
    """The automaton tables (fsm_tables) and the rows' states of a grammar over V tokens -> S."""
    S, Vn = _check_fsm_table(name, nxt, dev)
    if Vn != V or allow.dtype != torch.int32 or tuple(allow.shape) != (S, (V + 31) // 32) or not allow.is_contiguous():
        raise ValueError(f"{name}: tables {tuple(nxt.shape)} / {tuple(allow.shape)} for V={V} (fsm_tables)")
    if fsm_state.dtype != torch.int32 or fsm_state.numel() != B or not fsm_state.is_contiguous():
        raise ValueError(f"{name}: fsm_state must be a contiguous int32 [{B}] tensor")
    return S


def _logit_process(name: str, rows, counts, bias, tokens, n_tokens, active, return_ids, penalties=None, table=None, fsm=None):
    """logit_process / logit_process_fsm (`penalties`: the three scalars) and logit_process_rows_hip (`table`); fsm: (nxt, allow,
    fsm_state, eos_id) or None."""
    lib = _abi.load()
    dev = _require_device(name, rows, counts, *(fsm[:3] if fsm else ()))
    if rows.dim() != 3 or rows.dtype != torch.bfloat16:
        raise ValueError(f"{name}: rows must be bfloat16 [B][R][V]")
    B, R, V = (int(x) for x in rows.shape)
    if _check_counts(name, counts, dev) != (B, V):
        raise ValueError(f"{name}: counts {tuple(counts.shape)} for rows {tuple(rows.shape)}")
    S = _check_fsm(name, *fsm[:3], B, V, dev) if fsm else 0
    stride = int(rows.stride(1)) if R > 1 else (int(rows.stride(0)) if B > 1 else V)
    if rows.stride(2) != 1 or stride < V or (B > 1 and rows.stride(0) != R * stride):
        raise ValueError(f"{name}: rows must have a unit inner stride and one constant stride >= V between consecutive rows (in place: no copy is made)")
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (B, V) or bias.device != dev or not bias.is_contiguous()):
        raise ValueError(f"{name}: bias must be a contiguous float32 [{B}][{V}] tensor on {dev}")
    n_tok = -1 if n_tokens is None else int(n_tokens)
    tok_stride = 0
    if tokens is not None:
        if tokens.dim() != 2 or tokens.dtype != torch.int32 or tokens.shape[0] != B or tokens.device != dev or not tokens.is_contiguous():
            raise ValueError(f"{name}: tokens must be a contiguous int32 [{B}][n] tensor on {dev}")
        tok_stride = int(tokens.shape[1])
    _check_entry_vectors(name, B, dev, active=active)
    if table is not None:
        table = _row_table(name, table, B, dev)
    ids = torch.empty((B, R), dtype=torch.int32, device=dev) if return_ids else None
    ws = torch.empty(max(lib.sd_logit_process_workspace(B, R, V), 16), dtype=torch.uint8, device=dev) if return_ids else None
    head = (rows.data_ptr(), stride, B, R, V, counts.data_ptr(), _ptr(bias), _ptr(tokens), tok_stride, n_tok, _ptr(active))
    out = (_ptr(ids), R, _ptr(ws), ws.numel() if ws is not None else 0)
    with torch.cuda.device(dev):
        if table is not None:
            nxt, allow, fsm_state, eos_id = fsm or (None, None, None, 0)
            _abi.check(lib.sd_logit_process_rows(*head, table.data_ptr(), *out, _ptr(nxt), _ptr(allow), S, _ptr(fsm_state), int(eos_id),
                                                 _stream_ptr(dev)), "sd_logit_process_rows")
        elif fsm:
            nxt, allow, fsm_state, eos_id = fsm
            _abi.check(lib.sd_logit_process_fsm(*head, *penalties, *out, nxt.data_ptr(), allow.data_ptr(), S, fsm_state.data_ptr(),
                                                int(eos_id), _stream_ptr(dev)), "sd_logit_process_fsm")
        else:
            _abi.check(lib.sd_logit_process(*head, *penalties, *out, _stream_ptr(dev)), "sd_logit_process")
    return ids


def logit_process(rows: torch.Tensor, counts: torch.Tensor, repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
                  frequency_penalty: float = 0.0, bias: Optional[torch.Tensor] = None, tokens: Optional[torch.Tensor] = None,
                  n_tokens: Optional[int] = None, active: Optional[torch.Tensor] = None, return_ids: bool = False):
    """The logit processors on caller tensors, IN PLACE (sd_logit_process, csrc/logit_proc.hip; the formula is in
    include/specdec_hip.h and restated in tests/logit_proc_ref.py).

    rows: bf16 [B][R][V], unit inner stride, rows a constant stride apart (a view of a wider buffer is not copied); counts:
    logit_counts(B, V); bias: optional float32 [B][V]; tokens: optional int32 [B][n], row b's in-step tokens; n_tokens: None =
    row (b, r) is conditioned on the first r tokens (the verify pass), else every row on the first n_tokens; active: optional
    int32 [B], rows with 0 are not written. Returns None, or with return_ids the int32 [B][R] argmax of each processed row."""
    return _logit_process("logit_process", rows, counts, bias, tokens, n_tokens, active, return_ids,
                          penalties=(float(repetition_penalty), float(presence_penalty), float(frequency_penalty)))


def logit_counts_set(counts: torch.Tensor, b: int, prompt_ids: Optional[torch.Tensor] = None,
                     generated_ids: Optional[torch.Tensor] = None) -> None:
    """Row b of `counts` <- cleared, the prompt bit of every id in prompt_ids, one count per occurrence in generated_ids (int32
    device vectors; sd_logit_counts_set). Asynchronous on the current stream."""
    dev = _require_device("logit_counts_set", counts)
    B, V = _check_counts("logit_counts_set", counts, dev)
    for name, t in (("prompt_ids", prompt_ids), ("generated_ids", generated_ids)):
        if t is not None and (t.dim() != 1 or t.dtype != torch.int32 or t.device != dev or not t.is_contiguous()):
            raise ValueError(f"logit_counts_set: {name} must be a contiguous int32 vector on {dev}")
    n_p = int(prompt_ids.numel()) if prompt_ids is not None else 0
    n_g = int(generated_ids.numel()) if generated_ids is not None else 0
    with torch.cuda.device(dev):
        _abi.check(_abi.load().sd_logit_counts_set(counts.data_ptr(), B, V, int(b), prompt_ids.data_ptr() if n_p else None, n_p,
                                                   generated_ids.data_ptr() if n_g else None, n_g, _stream_ptr(dev)), "sd_logit_counts_set")


def logit_counts_add(counts: torch.Tensor, tokens: torch.Tensor, n_new: torch.Tensor, active: Optional[torch.Tensor] = None) -> None:
    """Every active row's first n_new[b] tokens of tokens[b] (int32 [B][n]; ids outside the vocabulary, such as a -1 padding,
    are ignored) enter its counts, saturating; a token listed twice counts twice (sd_logit_counts_add)."""
    dev = _require_device("logit_counts_add", counts, tokens, n_new)
    B, V = _check_counts("logit_counts_add", counts, dev)
    if tokens.dim() != 2 or tokens.dtype != torch.int32 or tokens.shape[0] != B or not tokens.is_contiguous():
        raise ValueError(f"logit_counts_add: tokens must be a contiguous int32 [{B}][n] tensor")
    _check_entry_vectors("logit_counts_add", B, dev, n_new=n_new, active=active)
    n = int(tokens.shape[1])
    with torch.cuda.device(dev):
        _abi.check(_abi.load().sd_logit_counts_add(counts.data_ptr(), B, V, tokens.data_ptr(), n, n_new.data_ptr(), n,
                                                   _ptr(active), _stream_ptr(dev)), "sd_logit_counts_add")


def _check_fsm_table(name: str, nxt: torch.Tensor, dev) -> Tuple[int, int]:
    if nxt.dim() != 2 or nxt.dtype != torch.int16 or nxt.device != dev or not nxt.is_contiguous():
        raise ValueError(f"{name}: next must be a contiguous int16 [S][V] tensor on {dev} holding the automaton's uint16 words (fsm_tables)")
    return int(nxt.shape[0]), int(nxt.shape[1])


def fsm_build_masks(nxt: torch.Tensor) -> torch.Tensor:
    """The mask table of a token automaton, built on the device from its transition table (sd_fsm_build_masks, csrc/grammar.hip).
    nxt: int16 [S][V] holding the uint16 words (0xFFFF = not allowed) -> int32 [S][ceil(V / 32)]: bit v % 32 of word v / 32 is
    set where nxt[s][v] != 0xFFFF, pad bits 0."""
    lib = _abi.load()
    dev = _require_device("fsm_build_masks", nxt)
    S, V = _check_fsm_table("fsm_build_masks", nxt, dev)
    W = (V + 31) // 32
    nbytes = int(lib.sd_fsm_mask_bytes(S, V))
    buf = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _abi.check(lib.sd_fsm_build_masks(nxt.data_ptr(), S, V, buf.data_ptr(), nbytes, _stream_ptr(dev)), "sd_fsm_build_masks")
    return buf[:S * W].view(S, W)


def fsm_tables(fsm, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """A specdec_hip.grammar.TokenFSM on the device: (next int16 [S][V], allow int32 [S][ceil(V / 32)])."""
    import numpy as np

    nxt = torch.from_numpy(np.ascontiguousarray(fsm.next).view(np.int16)).to(device)
    return nxt, fsm_build_masks(nxt)


def logit_process_fsm(rows: torch.Tensor, counts: torch.Tensor, nxt: torch.Tensor, allow: torch.Tensor, fsm_state: torch.Tensor,
                      eos_id: int, repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                      bias: Optional[torch.Tensor] = None, tokens: Optional[torch.Tensor] = None, n_tokens: Optional[int] = None,
                      active: Optional[torch.Tensor] = None, return_ids: bool = False):
    """logit_process with the grammar line (sd_logit_process_fsm): row (b, r) is masked by the state its automaton reaches from
    fsm_state[b] (int32 [B]; -1 = unconstrained) over the row's in-step tokens; a disallowed element is stored as -inf. nxt /
    allow: fsm_tables. Everything else as logit_process."""
    return _logit_process("logit_process_fsm", rows, counts, bias, tokens, n_tokens, active, return_ids,
                          penalties=(float(repetition_penalty), float(presence_penalty), float(frequency_penalty)),
                          fsm=(nxt, allow, fsm_state, eos_id))


def logit_process_rows_hip(rows: torch.Tensor, counts: torch.Tensor, table, bias: Optional[torch.Tensor] = None,
                           tokens: Optional[torch.Tensor] = None, n_tokens: Optional[int] = None, active: Optional[torch.Tensor] = None,
                           return_ids: bool = False, nxt: Optional[torch.Tensor] = None, allow: Optional[torch.Tensor] = None,
                           fsm_state: Optional[torch.Tensor] = None, eos_id: int = 0):
    """logit_process / logit_process_fsm with every batch row's own penalties (sd_logit_process_rows): `table` is a list of
    SamplingParams, one per batch row, or their packed tensor; a row whose penalties the scalar op would refuse is processed
    with the identity. nxt / allow / fsm_state: the grammar of logit_process_fsm, all None for none."""
    grammar = nxt is not None or allow is not None or fsm_state is not None
    if grammar and (nxt is None or allow is None or fsm_state is None):
        raise ValueError("logit_process_rows: a grammar needs nxt, allow and fsm_state")
    return _logit_process("logit_process_rows", rows, counts, bias, tokens, n_tokens, active, return_ids, table=table,
                          fsm=(nxt, allow, fsm_state, eos_id) if grammar else None)


def fsm_advance(nxt: torch.Tensor, fsm_state: torch.Tensor, tokens: torch.Tensor, n_new: torch.Tensor,
                active: Optional[torch.Tensor] = None) -> None:
    """Every active row with a state >= 0 walks its first n_new[b] tokens of tokens[b] (int32 [B][n]), in place in fsm_state
    (int32 [B]); a token the state does not allow, or an id outside the vocabulary, leads to DEAD = 0xFFFF (sd_fsm_advance)."""
    dev = _require_device("fsm_advance", nxt, fsm_state, tokens, n_new)
    S, V = _check_fsm_table("fsm_advance", nxt, dev)
    B = int(fsm_state.numel())
    if fsm_state.dtype != torch.int32 or not fsm_state.is_contiguous():
        raise ValueError("fsm_advance: fsm_state must be a contiguous int32 [B] tensor")
    if tokens.dim() != 2 or tokens.dtype != torch.int32 or tokens.shape[0] != B or not tokens.is_contiguous():
        raise ValueError(f"fsm_advance: tokens must be a contiguous int32 [{B}][n] tensor")
    _check_entry_vectors("fsm_advance", B, dev, n_new=n_new, active=active)
    n = int(tokens.shape[1])
    with torch.cuda.device(dev):
        _abi.check(_abi.load().sd_fsm_advance(nxt.data_ptr(), S, V, fsm_state.data_ptr(), B, tokens.data_ptr(), n, n_new.data_ptr(), n,
                                              _ptr(active), _stream_ptr(dev)), "sd_fsm_advance")


def spec_agreement(draft_logits: torch.Tensor, target_logits: torch.Tensor, temperature: float = 1.0):
    """Draft-target agreement per position (sd_spec_agreement, csrc/spec_agree.hip): how much of softmax(target / T) the draft's
    softmax(draft / T) reproduces, in float64 over the stored bf16 logits.

    draft_logits, target_logits: bf16 device tensors of equal shape [n, V] or [B, K, V] with unit inner stride (row strides are
    passed on; rows taken as views of a wider buffer are not copied). Returns, shaped like the leading dimensions,
    (alpha float64: the acceptance probability sum_v min(p, q) = 1 - TV(p, q); kl float64: KL(p || q); agree bool: equal argmax;
    p_arg, q_arg int32: the target's and the draft's argmax id). A position whose rows hold a NaN or have a non-finite maximum
    gives alpha = kl = NaN. Bit-identical run to run; a position's outputs do not depend on the other positions."""
    lib = _abi.load()
    dev = _require_device("spec_agreement", draft_logits, target_logits)
    if draft_logits.dim() not in (2, 3) or draft_logits.shape != target_logits.shape:
        raise ValueError(f"spec_agreement: need two [n,V] or [B,K,V] tensors of one shape, got {tuple(draft_logits.shape)} / "
                         f"{tuple(target_logits.shape)}")
    if draft_logits.dtype != torch.bfloat16 or target_logits.dtype != torch.bfloat16:
        raise TypeError("spec_agreement: logits must be bfloat16")
    lead, V = tuple(draft_logits.shape[:-1]), int(draft_logits.shape[-1])
    n = 1
    for d in lead:
        n *= int(d)
    if n < 1 or V < 1:
        raise ValueError(f"spec_agreement: empty logits {tuple(draft_logits.shape)}")

    def rows(t):   # -> ([n, V] view when the leading dimensions collapse (else a copy), elements between its rows)
        t = t.reshape(n, V)
        if t.stride(1) != 1 or (n > 1 and t.stride(0) < V):
            t = t.contiguous()
        return t, (int(t.stride(0)) if n > 1 else V)

    (q, ld_q), (p, ld_p) = rows(draft_logits), rows(target_logits)
    alpha = torch.empty(n, dtype=torch.float64, device=dev)
    kl = torch.empty(n, dtype=torch.float64, device=dev)
    ints = torch.empty((3, n), dtype=torch.int32, device=dev)
    ws = torch.empty(max(lib.sd_spec_agreement_workspace(n, V), 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _abi.check(lib.sd_spec_agreement(q.data_ptr(), ld_q, p.data_ptr(), ld_p, n, V, float(temperature), alpha.data_ptr(),
                                         kl.data_ptr(), ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), ws.data_ptr(),
                                         ws.numel(), _stream_ptr(dev)), "sd_spec_agreement")
    return alpha.view(lead), kl.view(lead), ints[0].view(lead) != 0, ints[1].view(lead), ints[2].view(lead)


def quantize_fp8_rows_hip(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(q float8_e4m3fn [N][K], scales float32 [N]) of a bf16 matrix: the per-output-row quantiser of the
    engine's fp8 weight storage (sd_quantize_fp8_rows)."""
    lib = _abi.load()
    dev = _require_device("quantize_fp8_rows", w)
    if w.dtype != torch.bfloat16 or w.dim() != 2:
        raise TypeError(f"quantize_fp8_rows: need a bf16 matrix, got {w.dtype} {tuple(w.shape)}")
    w = w.contiguous()
    N, K = w.shape
    q = torch.empty((N, K), dtype=torch.uint8, device=dev)
    sc = torch.empty(N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _abi.check(lib.sd_quantize_fp8_rows(w.data_ptr(), N, K, q.data_ptr(), sc.data_ptr(), _stream_ptr(dev)), "sd_quantize_fp8_rows")
    return q.view(torch.float8_e4m3fn), sc


def eagle_extrapolate(x: torch.Tensor, prev: torch.Tensor, has_prev: torch.Tensor, norm_w: torch.Tensor,
                      norm_b: Optional[torch.Tensor], eps: float, alpha: float, K: int, rms: bool = True) -> torch.Tensor:
    """The extrapolation launch of the EAGLE step (sd_eagle_extrapolate) on the caller's buffers: x bf16 [B][d] residual rows;
    prev bf16 [B][d] and has_prev int32 [B], the per-row state, are read and then OVERWRITTEN (prev <- h_K, has_prev <- 1).
    -> H bf16 [B][K][d]: h_1 .. h_K of every row."""
    lib = _abi.load()
    dev = _require_device("eagle_extrapolate", x, prev, has_prev, norm_w)
    if x.dim() != 2 or x.dtype != torch.bfloat16 or prev.dtype != torch.bfloat16 or prev.shape != x.shape or norm_w.dtype != torch.bfloat16:
        raise TypeError("eagle_extrapolate: x and prev must be bf16 [B][d], norm_w bf16 [d]")
    B, d = (int(v) for v in x.shape)
    if has_prev.dtype != torch.int32 or has_prev.shape != (B,) or norm_w.shape != (d,):
        raise TypeError("eagle_extrapolate: has_prev must be int32 [B], norm_w [d]")
    if not rms and (norm_b is None or norm_b.dtype != torch.bfloat16 or norm_b.shape != (d,) or norm_b.device != dev):
        raise TypeError("eagle_extrapolate: LayerNorm needs a bf16 bias [d]")
    if not (x.is_contiguous() and prev.is_contiguous() and has_prev.is_contiguous() and norm_w.is_contiguous()
            and (norm_b is None or norm_b.is_contiguous())):
        raise ValueError("eagle_extrapolate: tensors must be contiguous")
    H = torch.empty((B, int(K), d), dtype=torch.bfloat16, device=dev)
    with torch.cuda.device(dev):
        _abi.check(lib.sd_eagle_extrapolate(x.data_ptr(), H.data_ptr(), prev.data_ptr(), has_prev.data_ptr(), norm_w.data_ptr(),
                                            norm_b.data_ptr() if norm_b is not None else None, float(eps), float(alpha), d, B, int(K),
                                            1 if rms else 0, _stream_ptr(dev)), "sd_eagle_extrapolate")
    return H


PRO_NONE, PRO_RMSNORM, PRO_LAYERNORM = range(3)                              # enum GemvPrologue (csrc/kernels.h)
EPI_QKV_ROPE, EPI_RESID, EPI_SWIGLU, EPI_GELU, EPI_ARGMAX = range(5)         # enum GemvEpilogue
PLAN_NO_DIRECT, PLAN_NO_PIPE = 1, 2                                          # sd_gemm_plan flags


def gemm_plan(T: int, n_pairs: int, K: int, w8: bool = False, prologue: int = PRO_NONE, epi: int = EPI_RESID, flags: int = 0) -> str:
    """Name of the kernel instantiation one matrix launch of T tokens runs (sd_gemm_plan): "pipe<swiglu,tg2,bf16,sc4>",
    "chunked<qkv,tg6,fp8,nb1>", "slice<tg3>", "direct<tg1>", "gemv" (T <= 9) or "none" (not covered). Host-only: needs no GPU."""
    buf = ctypes.create_string_buffer(64)
    _abi.check(_abi.load().sd_gemm_plan(int(T), int(n_pairs), int(K), 1 if w8 else 0, int(prologue), int(epi), int(flags), buf, len(buf)),
               "sd_gemm_plan")
    return buf.value.decode()


def gemv_variant(T: int, n_pairs: int, K: int, w8: bool = False, prologue: int = PRO_NONE, epi: int = EPI_RESID, w12: int = 0) -> str:
    """Name of the csrc/gemv.hip instance a layer-matrix launch of T <= 9 tokens runs (sd_gemv_variant): "generic" or
    "fixed<qkv,ks8,tp5,rmsnorm,tt5,kb6>". w12: the (bf16) matrix has a W12 copy — "fixed<...,w12>" at 5 tokens, "generic" at other
    counts; SPECDEC_NO_W12 turns it off. w12 is the form of the copy: True / W12_CODES (1) the code form, W12_SPLIT (2) the
    split-byte form, whose names say "w12s". Follows SPECDEC_GEMV_GENERIC in the environment, as a launch does. Host-only."""
    buf = ctypes.create_string_buffer(64)
    _abi.check(_abi.load().sd_gemv_variant(int(T), int(n_pairs), int(K), 1 if w8 else 1 + int(w12) if w12 else 0, int(prologue), int(epi), buf, len(buf)),
               "sd_gemv_variant")
    return buf.value.decode()


def gemv_instance(T: int, n_pairs: int, K: int, w8: bool = False, prologue: int = PRO_NONE, epi: int = EPI_RESID, w12: int = 0) -> str:
    """Name of the kernel a layer-matrix launch of T <= 9 tokens really runs (sd_gemv_instance): "fixed<...>" as gemv_variant,
    "generic<resid,mask,tt9,bf16,kb12>" (the generic kernel's template key) or "skinny:direct<tg1>" (rows too long to stage:
    the csrc/gemm_skinny.hip body that takes the launch). w12: as for gemv_variant ("generic<...,w12s,kb12>"). Raises where the launcher would refuse. Follows SPECDEC_GEMV_GENERIC
    in the environment, as a launch does. Host-only."""
    buf = ctypes.create_string_buffer(64)
    _abi.check(_abi.load().sd_gemv_instance(int(T), int(n_pairs), int(K), 1 if w8 else 1 + int(w12) if w12 else 0, int(prologue), int(epi), buf, len(buf)),
               "sd_gemv_instance")
    return buf.value.decode()


class AttentionPlan(NamedTuple):
    tiles: int                    # 16-row query tiles per (row, kv head)
    n_split: int                  # workgroups per tile (1: no split-KV); a row uses min(n_split, ceil(key blocks / 16)) of them
    grid: Tuple[int, int, int]    # (Hkv, B, tiles * n_split)


def attention_plan(n_q_heads: int, n_kv_heads: int, head_dim: int, B: int, M: int, l_max: int, paged: int = 0) -> AttentionPlan:
    """The geometry of one K-token attention launch (csrc/attention.hip) of B rows x M tokens over a cache of l_max positions
    per row (sd_attention_plan), from the function the launch itself consults. paged: 0 = dense rows, else the page length.
    Follows SPECDEC_NO_ATTN_SPLIT in the environment, as a launch does; raises where the launch would refuse. Host-only."""
    out = [ctypes.c_int(0) for _ in range(5)]
    _abi.check(_abi.load().sd_attention_plan(int(n_q_heads), int(n_kv_heads), int(head_dim), int(B), int(M), int(l_max), int(paged or 0),
                                             *(ctypes.byref(o) for o in out)), "sd_attention_plan")
    t, ns, gx, gy, gz = (int(o.value) for o in out)
    return AttentionPlan(t, ns, (gx, gy, gz))


class PersistPlan(NamedTuple):
    eligible: bool       # the model passes every static rule of the persistent forward
    max_tokens: int      # tokens one persistent pass can hold (0 when not eligible)
    name: str            # "persist<64,1>" ... "persist<128,2>" for an eligible T, else "none"
    ring_bytes: int      # weight ring the LDS carve of one row of T tokens leaves (0 with "none")
    reason: str          # "" for an eligible T, else the rule that refused


def persist_plan(arch: int, n_layers: int, d_model: int, n_heads: int, n_kv_heads: int, head_dim: int, d_ff: int, vocab: int,
                 T: int = 1, packed: bool = True, weight_dtype: str = "bf16", has_bias: bool = False) -> PersistPlan:
    """What the persistent forward (csrc/persist.hip) decides for a model of these dimensions and a pass of T tokens
    (sd_persist_plan): the bind's eligibility rules, the token limit and the launch's instantiation, from the functions the
    engine itself asks. Host-only: needs no GPU (256 CUs are assumed)."""
    el, mt, ring = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    name, reason = ctypes.create_string_buffer(32), ctypes.create_string_buffer(96)
    wd = {"bf16": _abi.SD_BF16, "fp8": _abi.SD_FP8_E4M3}[weight_dtype]
    _abi.check(_abi.load().sd_persist_plan(int(arch), int(n_layers), int(d_model), int(n_heads), int(n_kv_heads), int(head_dim), int(d_ff),
                                           int(vocab), 1 if packed else 0, wd, 1 if has_bias else 0, int(T), ctypes.byref(el),
                                           ctypes.byref(mt), ctypes.byref(ring), name, len(name), reason, len(reason)), "sd_persist_plan")
    return PersistPlan(bool(el.value), int(mt.value), name.value.decode(), int(ring.value), reason.value.decode())


class PrefillPlan(NamedTuple):
    eligible: bool        # the native backend serves a model of these dimensions
    name: str             # "mfma<rf4,bf16>", "mfma<rf2,fp8>", ... or "none"
    row_blocks: int       # workgroups along the packed rows (128 rows each for rf4, 64 for rf2: whole tiles, so some hold fewer)
    token_blocks: int     # workgroups along the chunk's positions (128 each)
    grid: int             # row_blocks * token_blocks
    swizzled: bool        # the grid is a multiple of 8: workgroups are dealt to blocks XCD by XCD
    last_rows: int        # rows of the last token block (1 .. 128)
    min_block_rows: int   # fewest packed rows in any row block
    k_stages: int         # 64-k stages of the main loop
    reason: str           # "" or the rule that refused the model
    blocks: Tuple[Tuple[int, int], ...]   # (first row pair, packed rows) of every row block
    wg_block: Tuple[int, ...]             # workgroup -> linear block index row_block * token_blocks + token_block

    @property
    def rb(self) -> int:
        """block height of the instantiation: 128 (rf4) or 64 (rf2)"""
        return 128 if "rf4" in self.name else 64


def prefill_plan(arch: int, d_model: int, n_heads: int, n_kv_heads: int, head_dim: int, d_ff: int, which: int, T: int,
                 w8: bool = False, packed: bool = True) -> PrefillPlan:
    """What the native prompt-prefill GEMM (csrc/prefill_mfma.hip) decides for layer product `which` (0 qkv, 1 out, 2 gate / up,
    3 down) of a model of these dimensions over one chunk of T <= 512 positions (sd_prefill_plan, sd_prefill_plan_tables): the
    launcher's own block-height choice, row-block tables and workgroup mapping; for a model the backend refuses, the reason sd_model_set_prefill_backend gives. Host-only: needs no GPU."""
    lib = _abi.load()
    v = [ctypes.c_int(0) for _ in range(8)]
    name, reason = ctypes.create_string_buffer(32), ctypes.create_string_buffer(96)
    dims = (int(arch), int(d_model), int(n_heads), int(n_kv_heads), int(head_dim), int(d_ff), int(which), int(T))
    _abi.check(lib.sd_prefill_plan(*dims, 1 if w8 else 0, 1 if packed else 0, *[ctypes.byref(x) for x in v], name, len(name), reason, len(reason)),
               "sd_prefill_plan")
    el, nb, ntb, grid, swz, last, minrows, ks = (int(x.value) for x in v)
    blocks, wg = (), ()
    if el:
        b, g = (ctypes.c_int * (2 * nb))(), (ctypes.c_int * grid)()
        _abi.check(lib.sd_prefill_plan_tables(*dims, b, nb, g, grid), "sd_prefill_plan_tables")
        blocks, wg = tuple((b[2 * i], b[2 * i + 1]) for i in range(nb)), tuple(g)
    return PrefillPlan(bool(el), name.value.decode(), nb, ntb, grid, bool(swz), last, minrows, ks, reason.value.decode(), blocks, wg)
