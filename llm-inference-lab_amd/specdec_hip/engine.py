"""Python face of the decoder-forward / step-loop entry points of the C-ABI.

Plumbing only: ctypes structs mirroring include/specdec_hip.h, torch tensors as the
owners of device memory (weights, KV caches, workspaces), torch streams as the HIP
streams. All arithmetic happens in csrc/.
"""

from __future__ import annotations

import ctypes
import os
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi
from .pages import PagePool
from .weights import ARCH_LLAMA, ModelConfig, ModelWeights

_vp = ctypes.c_void_p


class _LayerWeights(ctypes.Structure):
    _fields_ = [(n, _vp) for n in (
        "attn_norm_w", "attn_norm_b", "wqkv", "bqkv", "wo", "bo",
        "mlp_norm_w", "mlp_norm_b", "w_up", "b_up", "w_down", "b_down")]


class _ModelConfig(ctypes.Structure):
    _fields_ = [
        ("arch", ctypes.c_int),
        ("n_layers", ctypes.c_int), ("d_model", ctypes.c_int), ("n_heads", ctypes.c_int),
        ("n_kv_heads", ctypes.c_int), ("head_dim", ctypes.c_int), ("d_ff", ctypes.c_int),
        ("vocab", ctypes.c_int), ("max_pos", ctypes.c_int),
        ("norm_eps", ctypes.c_float),
        ("weight_dtype", ctypes.c_int),
        ("tok_emb", _vp), ("pos_emb", _vp), ("final_norm_w", _vp), ("final_norm_b", _vp),
        ("lm_head", _vp), ("rope_cos", _vp), ("rope_sin", _vp),
        ("layers", ctypes.POINTER(_LayerWeights)),
        ("packed", _vp),
    ]


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream(stream: Optional[torch.cuda.Stream], device) -> int:
    return (stream or torch.cuda.current_stream(device)).cuda_stream


W12_DEFAULT = True   # bf16 models get the W12 copy (profiles/w12_verify.md)
W12_CLASSES = 0x10   # matrix classes that stream it (SD_W12_DEFAULT_CLASSES: the lm_head); SPECDEC_W12_CLASSES=0x1f: all five
W12S_CLASSES = 0x14  # classes that stream the split-byte form instead: gate / up and the lm_head (SD_W12S_DEFAULT_CLASSES; profiles/w12_split.md)
W12_CODES, W12_SPLIT = 1, 2   # enum W12Form


def w12_class_masks(env=None) -> Tuple[int, int]:
    """(code-form classes, split-byte classes) of a new model, disjoint. SPECDEC_W12_CLASSES and SPECDEC_W12S_CLASSES override the
    defaults; a class in both masks takes W12S, except that a class NAMED in an explicitly set SPECDEC_W12_CLASSES is not
    moved to W12S by the mere default of the other mask (the code form stays reachable exactly as it was)."""
    env = os.environ if env is None else env
    codes_set, split_set = env.get("SPECDEC_W12_CLASSES"), env.get("SPECDEC_W12S_CLASSES")
    codes = (int(codes_set, 0) if codes_set is not None else W12_CLASSES) & 0x1F
    split = (int(split_set, 0) & 0x1F) if split_set is not None else (W12S_CLASSES & ~codes if codes_set is not None else W12S_CLASSES)
    return codes & ~split, split


def build_w12(lib, mc: "_ModelConfig", dev, classes: int = 0x1F, form: int = W12_CODES) -> Tuple[torch.Tensor, np.ndarray]:
    """The W12 copy, in the given form, of a config's packed bf16 matrices of the given classes (bit 0 qkv .. bit 4 lm_head):
    (device buffer, host uint32 wide-block counts per matrix, SD_W12_SKIP = 0xFFFFFFFF for a matrix that is left out)."""
    n_wide = np.zeros(4 * mc.n_layers + 1, dtype=np.uint32)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        scratch = torch.empty(lib.sd_w12_scratch_bytes(ctypes.byref(mc)), dtype=torch.uint8, device=dev)
        _abi.check(lib.sd_w12_measure_form(ctypes.byref(mc), form, scratch.data_ptr(), scratch.numel(), n_wide.ctypes.data, st), "sd_w12_measure_form")
        for i in range(n_wide.size):
            if not (classes >> (4 if i == 4 * mc.n_layers else i & 3)) & 1:
                n_wide[i] = 0xFFFFFFFF
        nbytes = lib.sd_w12_bytes(ctypes.byref(mc), n_wide.ctypes.data)
        buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        _abi.check(lib.sd_w12_pack_form(ctypes.byref(mc), form, scratch.data_ptr(), n_wide.ctypes.data, buf.data_ptr(), buf.numel(), st), "sd_w12_pack_form")
        torch.cuda.current_stream(dev).synchronize()   # scratch is read by the pack
    return buf, n_wide


def w12_matrix_info(lib, mc: "_ModelConfig", n_wide: np.ndarray, index: int, form: int = W12_CODES) -> dict:
    """sd_w12_matrix as a dict: taken, offset, main_bytes, ovf_bytes, table_bytes, blocks, bf16_bytes, n_wide, and the form
    (W12_CODES / W12_SPLIT) of the copy the counts belong to, as the caller names it."""
    taken = ctypes.c_int()
    v = [ctypes.c_size_t() for _ in range(6)]
    _abi.check(lib.sd_w12_matrix(ctypes.byref(mc), n_wide.ctypes.data, index, ctypes.byref(taken), *[ctypes.byref(x) for x in v]),
               "sd_w12_matrix")
    keys = ("offset", "main_bytes", "ovf_bytes", "table_bytes", "blocks", "bf16_bytes")
    return {"taken": bool(taken.value), "n_wide": int(n_wide[index]), "form": int(form), **{k: int(x.value) for k, x in zip(keys, v)}}


class EngineGaveUp(_abi.HipLibraryError):
    """A persistent forward hit one of its bounded waits (another kernel held CUs it needs, or a workgroup never ran) and left.
    Nothing hangs and nothing is silently wrong: the health word says so, the caller repeats the work on the launch path."""

    def __init__(self, msg: str, status: int = 0):
        super().__init__(msg)
        self.status = status


_PREFILL_NAMES = {v: k for k, v in _abi.PREFILL_BACKENDS.items()}


def _prefill_backend_id(name: str) -> int:
    """enum sd_prefill_backend of a backend name; raises before any device work"""
    if name not in _abi.PREFILL_BACKENDS:
        raise ValueError(f"prefill_backend={name!r} (one of {', '.join(_abi.PREFILL_BACKENDS)})")
    return _abi.PREFILL_BACKENDS[name]


def prefill_backends_available() -> List[str]:
    """names of the prefill backends this process can use"""
    lib = _abi.load()
    return [name for name, v in _abi.PREFILL_BACKENDS.items() if lib.sd_prefill_backend_available(v)]


class HipModel:
    """A decoder (Llama or GPT-2 shaped) bound to its KV cache on one GPU."""

    def __init__(self, weights: ModelWeights, batch: int, l_max: int, device: Optional[torch.device] = None,
                 weight_dtype: str = "bf16", page_len: Optional[int] = None, n_pages: Optional[int] = None,
                 prefill_backend: str = "auto"):
        """weight_dtype "fp8": the engine streams an OCP e4m3 copy of the Linear weights (per-output-row
        scales, quantised on the device at load); activations and the KV cache stay bf16.
        page_len (a power of two >= 32): paged KV — the rows share a pool of `n_pages` pages (default: enough for every
        row to reach l_max) through a block table; `reserve(row, length)` / `release(row)` manage a row's pages.
        prefill_backend: how prompts (>= 96 positions per row) are absorbed — "auto" (rocBLAS where it serves the model, else
        the passes), "passes", "rocblas" or "native" (this library's GEMM over the packed weights); see set_prefill_backend."""
        if weight_dtype not in ("bf16", "fp8"):
            raise ValueError(f"weight_dtype={weight_dtype!r} (bf16 or fp8)")
        _prefill_backend_id(prefill_backend)
        self.weight_dtype = weight_dtype
        self.lib = _abi.load()
        self.cfg: ModelConfig = weights.config
        dev = torch.device(device) if device is not None else weights.tok_emb.device
        if dev.type == "cuda" and dev.index is None:
            dev = weights.tok_emb.device if weights.tok_emb.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise RuntimeError("HipModel needs weights on a GPU (PyTorch-ROCm device 'cuda'); there is no CPU path")
        self.device = dev
        self.weights = weights  # keeps the tensors (borrowed pointers) alive
        for name, t in weights.tensors():
            if t.device != dev:
                raise RuntimeError(f"weight {name} is on {t.device}, expected {dev}")
            want = torch.float32 if name.startswith("rope_") else torch.bfloat16
            if t.dtype != want or not t.is_contiguous():
                raise TypeError(f"weight {name}: need contiguous {want}, got {t.dtype} contiguous={t.is_contiguous()}")
        c = self.cfg
        if not (1 <= c.n_kv_heads <= c.n_heads <= 255 and c.head_dim in (32, 64, 128)):
            # (the kernels' argument blocks carry these in 8-bit fields)
            raise ValueError(f"unsupported attention geometry: {c.n_heads} heads / {c.n_kv_heads} kv heads / head_dim {c.head_dim}")
        self._layers = (_LayerWeights * c.n_layers)()
        for i, l in enumerate(weights.layers):
            for f, _ in _LayerWeights._fields_:
                setattr(self._layers[i], f, _ptr(getattr(l, f)))
        mc = _ModelConfig(
            arch=c.arch, n_layers=c.n_layers, d_model=c.d_model, n_heads=c.n_heads, n_kv_heads=c.n_kv_heads,
            head_dim=c.head_dim, d_ff=c.d_ff, vocab=c.vocab, max_pos=c.max_pos, norm_eps=c.norm_eps,
            weight_dtype=_abi.SD_FP8_E4M3 if weight_dtype == "fp8" else _abi.SD_BF16,
            tok_emb=_ptr(weights.tok_emb), pos_emb=_ptr(weights.pos_emb),
            final_norm_w=_ptr(weights.final_norm_w), final_norm_b=_ptr(weights.final_norm_b),
            lm_head=_ptr(weights.lm_head), rope_cos=_ptr(weights.rope_cos), rope_sin=_ptr(weights.rope_sin),
            layers=self._layers,
        )
        # the engine's packed copy of the Linear weights (one per ModelWeights, shared by every
        # engine instance built over it)
        key = "_packed" if weight_dtype == "bf16" else "_packed_fp8"
        packed = weights.meta.get(key)
        if packed is None and (weight_dtype == "fp8" or not os.environ.get("SPECDEC_NO_PACK")):
            nbytes = self.lib.sd_packed_bytes(ctypes.byref(mc))
            with torch.cuda.device(dev):
                packed = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                _abi.check(self.lib.sd_pack_weights(ctypes.byref(mc), packed.data_ptr(), nbytes,
                                                    torch.cuda.current_stream(dev).cuda_stream), "sd_pack_weights")
            weights.meta[key] = packed
        self._packed = packed
        mc.packed = _ptr(packed)
        handle = _vp()
        _abi.check(self.lib.sd_model_create(ctypes.byref(mc), ctypes.byref(handle)), "sd_model_create")
        self.handle = handle
        # W12: a lossless 12-bit copy of the packed bf16 matrices for the launches of 1..9 tokens (csrc/pack.hip), one per
        # ModelWeights like the packed copy. W12_DEFAULT / W12_CLASSES: what profiles/w12_verify.md measured; SPECDEC_W12=1 / 0 and
        # SPECDEC_W12_CLASSES (bit mask: 1 qkv, 2 out, 4 gate / up, 8 down, 16 lm_head) override them, and
        # SPECDEC_NO_W12 (the library's per-launch switch) also skips building the copy. A copy is built per (classes, form):
        # _w12 the code form, _w12s the split-byte form (W12S_CLASSES / SPECDEC_W12S_CLASSES; w12_class_masks).
        self._w12 = None
        self._w12s = None
        self._mc = mc
        want_w12 = os.environ.get("SPECDEC_W12", "1" if W12_DEFAULT else "0") not in ("", "0")
        if weight_dtype == "bf16" and packed is not None and want_w12 and not os.environ.get("SPECDEC_NO_W12"):
            for attr, classes, form in zip(("_w12", "_w12s"), w12_class_masks(), (W12_CODES, W12_SPLIT)):
                if not classes:
                    continue
                key = f"{attr}_{classes:02x}"
                copy = weights.meta.get(key)
                if copy is None:
                    copy = weights.meta[key] = build_w12(self.lib, mc, dev, classes, form)
                setattr(self, attr, copy)
                _abi.check(self.lib.sd_model_set_w12_form(self.handle, _ptr(copy[0]), copy[1].ctypes.data, classes, form), "sd_model_set_w12_form")
        self.batch, self.l_max = int(batch), (int(l_max) + 31) // 32 * 32  # whole 32-key blocks
        self.page_len = None
        if page_len is not None or os.environ.get("SPECDEC_PAGED_KV"):
            self._bind_paged(int(page_len or os.environ["SPECDEC_PAGED_KV"]), n_pages)
        else:
            self._bind_dense()
        if prefill_backend != "auto":
            self.set_prefill_backend(prefill_backend)

    def _bind_dense(self) -> None:
        dev = self.device
        kv_bytes = self.lib.sd_model_kv_bytes(self.handle, self.batch, self.l_max)
        with torch.cuda.device(dev):
            # [n_layers][B][Hkv][Lmax][D] bf16 — sized for 288 GB of HBM: no paging, no realign copies
            self.k_cache = torch.zeros(kv_bytes // 2, dtype=torch.bfloat16, device=dev)
            self.v_cache = torch.zeros(kv_bytes // 2, dtype=torch.bfloat16, device=dev)
            self.workspace = torch.empty(self.lib.sd_model_workspace_bytes(self.handle), dtype=torch.uint8, device=dev)
            _abi.check(self.lib.sd_model_bind(self.handle, self.k_cache.data_ptr(), self.v_cache.data_ptr(),
                                              self.batch, self.l_max, self.workspace.data_ptr(),
                                              self.workspace.numel()), "sd_model_bind")

    # ---- paged KV -----------------------------------------------------------------------------------------------
    def _bind_paged(self, page_len: int, n_pages: Optional[int]) -> None:
        P = int(page_len)
        if P < 32 or P & (P - 1):
            raise ValueError(f"page_len={P}: a power of two >= 32")
        self.page_len = P
        self.max_pages = (self.l_max + P - 1) // P
        self.l_max = self.max_pages * P
        self.n_pages = int(n_pages) if n_pages is not None else self.batch * self.max_pages
        dev = self.device
        pool = self.lib.sd_model_kv_pool_bytes(self.handle, self.n_pages, P)
        with torch.cuda.device(dev):
            self.k_cache = torch.zeros(pool // 2, dtype=torch.bfloat16, device=dev)
            self.v_cache = torch.zeros(pool // 2, dtype=torch.bfloat16, device=dev)
            # every entry names a valid page at all times (unreached entries are never read, but a clamped load may touch them)
            self.block_table = torch.zeros(self.batch, self.max_pages, dtype=torch.int32, device=dev)
            self.workspace = torch.empty(self.lib.sd_model_workspace_bytes(self.handle), dtype=torch.uint8, device=dev)
            _abi.check(self.lib.sd_model_bind_paged(self.handle, self.k_cache.data_ptr(), self.v_cache.data_ptr(), self.n_pages, P,
                                                    self.block_table.data_ptr(), self.max_pages, self.batch,
                                                    self.workspace.data_ptr(), self.workspace.numel()), "sd_model_bind_paged")
        # host bookkeeping (pages.PagePool): free stack, pages per row in position order, owners per page
        self._pool = PagePool(self.n_pages, self.batch, P)
        self._free = self._pool.free
        self._owned: List[List[int]] = self._pool.owned

    def reserve(self, row: int, length: int, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Make positions [0, length) of `row` addressable (paged engines; a no-op on dense ones). New table entries are
        written on `stream` (default: the current stream) — the forward that uses them must be ordered after it."""
        if self.page_len is None:
            return
        need = (min(int(length), self.l_max) + self.page_len - 1) // self.page_len
        first, new = self._pool.reserve(row, need)
        if new:
            self._write_table(row, first, new, stream)

    def _write_table(self, row: int, first: int, pages: Sequence[int], stream: Optional[torch.cuda.Stream]) -> None:
        new = torch.tensor(list(pages), dtype=torch.int32)
        with torch.cuda.device(self.device), torch.cuda.stream(stream or torch.cuda.current_stream(self.device)):
            self.block_table[row, first:first + len(pages)].copy_(new.to(self.device, non_blocking=False))

    def release(self, row: int) -> None:
        """Return the row's pages to the pool (its sequence is finished; the next reserve() starts from nothing). A page that
        other rows share (fork_row) stays theirs."""
        if self.page_len is None:
            return
        self._pool.release(row)

    def pages_in_use(self) -> int:
        """Physical pages with an owner (a page shared by several rows counts once)."""
        return 0 if self.page_len is None else self._pool.pages_in_use()

    def unshare(self, row: int) -> None:
        """Before a row's cache is rebuilt from position 0: a row that shares pages with others gives all its pages up, so
        that the rebuild writes fresh ones (shared pages are never written). Rows that share nothing keep their pages."""
        if self.page_len is not None and self._pool.shares(row):
            self._pool.release(row)

    def fork_row(self, src: int, dsts: Sequence[int], length: int, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Give the rows `dsts` the first `length` cached positions of row `src`, asynchronously on `stream` (default: the
        current stream; the work that wrote the source must be ordered before it, what reads the destinations after it).
        Dense caches: one sd_model_kv_fork copies them. Paged caches: every destination releases what it owns, then SHARES
        the source's pages that no later write can touch (pages.shared_pages: those wholly below position length - 2) and
        gets fresh pages for the rest, filled by sd_model_kv_copy_pages (whole pages, and length % page_len positions of a
        partial last one); the table entries are written on `stream`, as reserve() does. Shared pages are immutable — rows
        only append or roll back to >= their accepted length — so there is no copy-on-write. A pool that cannot serve the
        fork raises before any table entry or ownership list has changed."""
        dsts = [int(d) for d in dsts]
        length = int(length)
        st = _stream(stream, self.device)
        if self.page_len is None:
            arr = (ctypes.c_int32 * max(len(dsts), 1))(*dsts)
            with torch.cuda.device(self.device):
                _abi.check(self.lib.sd_model_kv_fork(self.handle, int(src), arr, len(dsts), length, st), "sd_model_kv_fork")
            return
        if not 0 <= length <= self.l_max:
            raise ValueError(f"fork_row: length {length} outside [0, {self.l_max}]")
        plan = self._pool.fork(int(src), dsts, length)
        for d, pages in zip(dsts, plan.tables):
            if pages:
                self._write_table(d, 0, pages, stream)
        by_n: dict = {}
        for s, d, n in plan.copies:       # one call per distinct position count: whole pages, and the partial last page
            by_n.setdefault(n, []).append((s, d))
        with torch.cuda.device(self.device):
            for n, pairs in by_n.items():
                sp = (ctypes.c_int32 * len(pairs))(*[p[0] for p in pairs])
                dp = (ctypes.c_int32 * len(pairs))(*[p[1] for p in pairs])
                _abi.check(self.lib.sd_model_kv_copy_pages(self.handle, sp, dp, len(pairs), n, st), "sd_model_kv_copy_pages")

    def evict_row(self, row: int, keep: int, drop: int, n_pos: int, stream: Optional[torch.cuda.Stream] = None) -> None:
        """The rolling context window's device step (csrc/kv_evict.hip), asynchronously on `stream`: in cache row `row`, positions
        [keep + drop, n_pos) become positions [keep, n_pos - drop) in every layer and KV head — V bit for bit, K rotated by
        -drop positions with the model's own RoPE tables (one more bf16 rounding of the moved keys). The first `keep` positions,
        positions >= n_pos - drop and the other rows keep their bits; the row's length afterwards is the caller's to lower by
        `drop`. Dense Llama caches only, drop a positive multiple of 8 below max_pos: anything else raises before device work."""
        with torch.cuda.device(self.device):
            _abi.check(self.lib.sd_model_kv_evict(self.handle, int(row), int(keep), int(drop), int(n_pos), _stream(stream, self.device)),
                       "sd_model_kv_evict")

    def kv_view(self):
        c = self.cfg
        if self.page_len is not None:
            return (self.k_cache.view(c.n_layers, self.n_pages, c.n_kv_heads, self.page_len, c.head_dim),
                    self.v_cache.view(c.n_layers, self.n_pages, c.n_kv_heads, c.head_dim, self.page_len))
        k_shape = (c.n_layers, self.batch, c.n_kv_heads, self.l_max, c.head_dim)
        v_shape = (c.n_layers, self.batch, c.n_kv_heads, c.head_dim, self.l_max)  # V is kept transposed
        return self.k_cache.view(k_shape), self.v_cache.view(v_shape)

    def forward(self, tokens: torch.Tensor, pos_base: torch.Tensor, pos_off: int = 0,
                want_ids: bool = True, want_logits: bool = False, logits_dtype=torch.float32,
                skip_head: bool = False, stream: Optional[torch.cuda.Stream] = None, row0: int = 0):
        """tokens int32 [B][M] on the device, pos_base int32 [B] for rows [row0, row0+B) of the
        bound batch. Appends to the cache in place."""
        assert tokens.dtype == torch.int32 and tokens.dim() == 2 and tokens.device == self.device
        assert pos_base.dtype == torch.int32 and pos_base.shape == (tokens.shape[0],) and pos_base.device == self.device
        B, M = tokens.shape
        tokens = tokens.contiguous()
        if self.health():                 # an earlier persistent pass gave up: do not pile more work on invalid rows
            self.check_health("sd_model_forward")
        if self.page_len is not None:     # paged KV: the positions this pass writes must have pages (host-known here at the cost
            for i, p0 in enumerate(pos_base.tolist()):   # of one read-back; the captured step loop reserves ahead instead)
                self.reserve(row0 + i, p0 + int(pos_off) + M, stream=stream)
        ids = torch.empty((B, M), dtype=torch.int32, device=self.device) if (want_ids and not skip_head) else None
        logits = None
        if want_logits and not skip_head:
            logits = torch.empty((B, M, self.cfg.vocab), dtype=logits_dtype, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.sd_model_forward(
                self.handle, tokens.data_ptr(), M, pos_base.data_ptr(), int(pos_off), int(row0), B, M,
                _ptr(ids), M, _ptr(logits),
                _abi.SD_F32 if logits_dtype == torch.float32 else _abi.SD_BF16,
                1 if skip_head else 0, _stream(stream, self.device))
        _abi.check(rc, "sd_model_forward")
        return ids, logits

    def score(self, tokens, row: int = 0, pos0: int = 0, stream: Optional[torch.cuda.Stream] = None):
        """Log-likelihood of `tokens` (n >= 2 ids) appended to cache row `row` at positions pos0 .. pos0+n-1 (sd_model_score).
        -> (logprob fp32 [n-1]: log p(tokens[i+1] | ...), greedy int32 [n]: the argmax id after position i), device tensors.
        Leaves the cache as forward(skip_head=True) over the same tokens does; the [n][V] logits are never written."""
        t = torch.as_tensor(tokens).reshape(-1).to(self.device, torch.int32).contiguous()
        n = int(t.numel())
        if self.health():
            self.check_health("sd_model_score")
        if self.page_len is not None and n >= 2 and 0 <= row < self.batch and pos0 >= 0:
            self.reserve(int(row), int(pos0) + n, stream=stream)
        logprob = torch.empty((max(n - 1, 0),), dtype=torch.float32, device=self.device)
        greedy = torch.empty((n,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.sd_model_score(self.handle, t.data_ptr() if n else None, n, int(row), int(pos0), _ptr(logprob), _ptr(greedy),
                                         _stream(stream, self.device))
        _abi.check(rc, "sd_model_score")
        return logprob, greedy

    def score_logits(self, tokens, row: int = 0, pos0: int = 0, out: Optional[torch.Tensor] = None,
                     stream: Optional[torch.cuda.Stream] = None):
        """score() with the head storing each position's logits instead of reducing them (sd_model_score_logits): `tokens`
        (n >= 1 ids) appended to cache row `row` at positions pos0 .. pos0+n-1 -> (logits bf16 [n][V], greedy int32 [n]).
        Route, chunking, cache effect and prefill counters are score()'s. `out`: a contiguous bf16 buffer of at least n x V
        elements to store into (its first n rows are returned)."""
        t = torch.as_tensor(tokens).reshape(-1).to(self.device, torch.int32).contiguous()
        n, V = int(t.numel()), self.cfg.vocab
        if self.health():
            self.check_health("sd_model_score_logits")
        if self.page_len is not None and n >= 1 and 0 <= row < self.batch and pos0 >= 0:
            self.reserve(int(row), int(pos0) + n, stream=stream)
        if out is None:
            logits = torch.empty((n, V), dtype=torch.bfloat16, device=self.device)
        else:
            if out.dtype != torch.bfloat16 or out.device != self.device or not out.is_contiguous() or out.numel() < n * V:
                raise ValueError(f"score_logits: out must be a contiguous bf16 buffer of >= {n} x {V} elements on {self.device}")
            logits = out.view(-1)[: n * V].view(n, V)
        greedy = torch.empty((n,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.sd_model_score_logits(self.handle, t.data_ptr() if n else None, n, int(row), int(pos0), logits.data_ptr(),
                                                _ptr(greedy), _stream(stream, self.device))
        _abi.check(rc, "sd_model_score_logits")
        return logits, greedy

    def hidden_rows(self, n: int, row0: int = 0, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
        """bf16 [n][d_model]: the residual-stream rows (before the final norm) of the last forward pass (sd_model_hidden_rows)."""
        out = torch.empty((n, self.cfg.d_model), dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.sd_model_hidden_rows(self.handle, int(row0), int(n), out.data_ptr(), _stream(stream, self.device)),
                       "sd_model_hidden_rows")
        return out

    @property
    def pass_tokens(self) -> int:
        """Tokens per forward pass (64 with the multi-token kernel, else 9)."""
        return int(self.lib.sd_model_pass_tokens(self.handle))

    PROBE_O, PROBE_GATE_UP, PROBE_DOWN, PROBE_LM_HEAD = 1, 2, 3, 4

    def probe_gemv(self, which: int, T: int, iters: int = 200, stream: Optional[torch.cuda.Stream] = None):
        """(average launch duration in microseconds, algorithmic bytes per launch) of one of the
        forward's GEMVs, timed with HIP events on the launch stream (sd_model_probe_gemv)."""
        usec, nbytes = ctypes.c_float(0), ctypes.c_double(0)
        with torch.cuda.device(self.device):
            rc = self.lib.sd_model_probe_gemv(self.handle, int(which), int(T), int(iters), _stream(stream, self.device),
                                              ctypes.byref(usec), ctypes.byref(nbytes))
        _abi.check(rc, "sd_model_probe_gemv")
        return float(usec.value), float(nbytes.value)

    @property
    def persist_tokens(self) -> int:
        """Tokens per pass that run as ONE persistent launch (sd_model_persist_tokens); 0 = launch-per-operator only."""
        return int(self.lib.sd_model_persist_tokens(self.handle))

    def persist_active(self, tokens: int = 1) -> bool:
        """Would a pass of `tokens` tokens of one row run as the persistent launch right now (token limit, length hint, paging)?"""
        return bool(self.lib.sd_model_persist_active(self.handle, int(tokens)))

    # ---- prompt prefill -------------------------------------------------------------------------------------------
    def set_prefill_backend(self, name: str) -> None:
        """"auto", "passes", "rocblas" or "native". Raises (ValueError) for an unknown name and (RuntimeError, with the
        library's reason) for a backend that cannot serve this model: rocBLAS missing, or asked for fp8 / paged / GPT-2;
        native asked for GPT-2 or a model without packed weights. A choice is never replaced by another GEMM."""
        _abi.check(self.lib.sd_model_set_prefill_backend(self.handle, _prefill_backend_id(name)), "sd_model_set_prefill_backend")

    @property
    def prefill_backend(self) -> str:
        return _PREFILL_NAMES[self.lib.sd_model_prefill_backend(self.handle)]

    def prefill_counts(self) -> dict:
        """Prompt rows absorbed per backend since the bind (one per row of a forward of >= 96 positions per row)."""
        return {name: int(self.lib.sd_model_prefill_count(self.handle, _abi.PREFILL_BACKENDS[name])) for name in ("passes", "rocblas", "native")}

    def set_persist_tokens(self, max_tokens: int) -> None:
        """Tokens per pass the persistent launch takes from now on (0: launch path only; sd_model_set_persist_tokens). Loops that
        captured a step over this model must be invalidated (HipSpecDec.invalidate)."""
        _abi.check(self.lib.sd_model_set_persist_tokens(self.handle, int(max_tokens)), "sd_model_set_persist_tokens")

    def set_persist_taps(self, enable: bool) -> None:
        """Whether persistent passes also store the stage rows (the default) or run the instantiation without those stores, as the
        draft of a loop does (sd_model_set_persist_taps). A pass with skip_head keeps its stores; while off, debug_rows and
        hidden_rows are stale after a persistent pass."""
        _abi.check(self.lib.sd_model_set_persist_taps(self.handle, 1 if enable else 0), "sd_model_set_persist_taps")

    def persist_plan(self, T: int = 1):
        """ops.persist_plan of this model's dimensions, storage and biases for a pass of T tokens: eligibility, token limit,
        instantiation name, ring bytes, reason. The model's own state (token limit set, length hint, paging, cache size) is
        persist_active's question."""
        from .ops import persist_plan
        c = self.cfg
        has_bias = any(getattr(l, f) is not None for l in self.weights.layers for f in ("bqkv", "bo", "b_up", "b_down"))
        return persist_plan(c.arch, c.n_layers, c.d_model, c.n_heads, c.n_kv_heads, c.head_dim, c.d_ff, c.vocab, T,
                            packed=self._packed is not None, weight_dtype=self.weight_dtype, has_bias=has_bias)

    def set_length_hint(self, max_len: Optional[int]) -> None:
        """The caller's bound on the current length of the rows the coming passes touch (None: the cache size). The persistent
        launch serves rows of up to 1280 positions (sd_model_set_length_hint)."""
        _abi.check(self.lib.sd_model_set_length_hint(self.handle, int(max_len or 0)), "sd_model_set_length_hint")

    def health(self) -> int:
        """The persistent launches' health word as the pinned host copy holds it — no copy, no synchronisation: valid for every
        pass the caller has already synchronised with (it has read the pass's ids / logits). 0 = all completed."""
        w = getattr(self, "_status_word", None)
        if w is None:
            ptr = self.lib.sd_model_status_word(self.handle)
            if not ptr:
                return 0
            w = self._status_word = np.ctypeslib.as_array(ptr, shape=(1,))
        return int(w[0])

    def check_health(self, what: str = "forward", sync: bool = False, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Raise EngineGaveUp when a persistent launch of this model gave up (its outputs, and those of every pass after it, are
        invalid). sync: drain `stream` first (for a caller that has not yet read anything of its last pass)."""
        if sync:
            (stream or torch.cuda.current_stream(self.device)).synchronize()
        st = self.health()
        if st:
            raise EngineGaveUp(f"{what}: a persistent forward gave up (status {st:#x}: see sd_model_engine_status); the outputs since "
                               "then are invalid — HipModel.recover() clears the word and continues on the launch path", st)

    def recover(self, stream: Optional[torch.cuda.Stream] = None) -> int:
        """After a give-up: drain the stream, clear the health word (device and host), move the launch counter past the failed
        launch, and switch this model to the launch path (persistent passes stay off until the model is bound again or
        set_persist_tokens re-enables them). The passes since the failure must be repeated. Returns the status that was cleared."""
        st = self.engine_status(stream)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.sd_model_engine_status_clear(self.handle, _stream(stream, self.device)), "sd_model_engine_status_clear")
        self.set_persist_tokens(0)
        return st

    def clear_engine_status(self, stream: Optional[torch.cuda.Stream] = None) -> None:
        """sd_model_engine_status_clear alone: the persistent path stays on (tests of the give-up path)."""
        with torch.cuda.device(self.device):
            _abi.check(self.lib.sd_model_engine_status_clear(self.handle, _stream(stream, self.device)), "sd_model_engine_status_clear")

    def engine_status(self, stream: Optional[torch.cuda.Stream] = None) -> int:
        """0 = every persistent launch of this model completed (sd_model_engine_status; synchronises the stream)."""
        st = ctypes.c_uint32(0)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.sd_model_engine_status(self.handle, ctypes.byref(st), _stream(stream, self.device)), "sd_model_engine_status")
        return int(st.value)

    DEBUG_X, DEBUG_Q, DEBUG_ATTN, DEBUG_ACT = 0, 1, 2, 3

    def debug_rows(self, which: int, n: int, row0: int = 0, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
        """bf16 [n][width]: rows of a workspace buffer of the last pass, last layer (sd_model_debug_rows)."""
        c = self.cfg
        width = {0: c.d_model, 1: c.n_heads * c.head_dim, 2: c.n_heads * c.head_dim, 3: c.d_ff}[int(which)]
        out = torch.empty((n, width), dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.sd_model_debug_rows(self.handle, int(which), int(row0), int(n), out.data_ptr(), _stream(stream, self.device)),
                       "sd_model_debug_rows")
        return out

    def prefill_rows(self, which: int, row0: int, n: int, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
        """bf16 [n][width]: rows [row0, row0 + n) of the last chunk of the last GEMM-prefilled prompt, in position order, for
        every position of the chunk (sd_model_prefill_rows; `which` as for debug_rows). Raises when the model's last forward was
        not such a chunk."""
        c = self.cfg
        width = {0: c.d_model, 1: c.n_heads * c.head_dim, 2: c.n_heads * c.head_dim, 3: c.d_ff}[int(which)]
        out = torch.empty((max(int(n), 0), width), dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.sd_model_prefill_rows(self.handle, int(which), int(row0), int(n), out.data_ptr(), _stream(stream, self.device)),
                       "sd_model_prefill_rows")
        return out

    def prefill_plan(self, which: int, T: int):
        """ops.prefill_plan of this model's dimensions and storage for layer product `which` over a chunk of T positions."""
        from .ops import prefill_plan
        c = self.cfg
        return prefill_plan(c.arch, c.d_model, c.n_heads, c.n_kv_heads, c.head_dim, c.d_ff, which, T, self.weight_dtype == "fp8",
                            packed=self._packed is not None)

    def matrix_shape(self, which: int):
        """(N, K, n_pairs, epi, prologue) of matrix kind `which` (0 qkv, 1 out, 2 gate / up, 3 down, 4 lm_head) as the forward
        launches it (sd_model_matrix_shape)."""
        v = [ctypes.c_int(0) for _ in range(5)]
        _abi.check(self.lib.sd_model_matrix_shape(self.handle, int(which), *[ctypes.byref(x) for x in v]), "sd_model_matrix_shape")
        return tuple(int(x.value) for x in v)

    def pass_plan(self, T: int, flags: int = 0) -> List[str]:
        """The five kernel instantiations (ops.gemm_plan) a launch-path pass of T tokens runs for qkv, out, gate / up, down and
        lm_head (every layer runs the same four)."""
        from .ops import gemm_plan
        out = []
        for which in range(5):
            _, K, n_pairs, epi, prologue = self.matrix_shape(which)
            out.append(gemm_plan(T, n_pairs, K, self.weight_dtype == "fp8", prologue, epi, flags))
        return out

    def small_pass_instances(self, T: int) -> List[str]:
        """The five kernels (ops.gemv_instance) a launch-path pass of T <= 9 tokens runs for qkv, out, gate / up, down and
        lm_head, by analogy with pass_plan."""
        from .ops import gemv_instance
        out = []
        for which in range(5):
            _, K, n_pairs, epi, prologue = self.matrix_shape(which)
            out.append(gemv_instance(T, n_pairs, K, self.weight_dtype == "fp8", prologue, epi))
        return out

    def probe_forward(self, M: int = 1, iters: int = 50, skip_head: bool = False, timeline: bool = False,
                      stream: Optional[torch.cuda.Stream] = None, pos0: int = 0):
        """(average microseconds per forward of M tokens, bytes of weights per forward, timeline or None): sd_model_probe_forward.
        timeline: uint64 [256][12 * n_ops + 4] stamps (100 MHz) of one persistent forward — per op: gather start, input staged,
        op done, attention done, third consumer start, its MFMA end, leader MFMA end, loader done issuing; then (realtime,
        shader clock) at start and end."""
        usec, nbytes = ctypes.c_float(0), ctypes.c_double(0)
        n_ops = 4 * self.cfg.n_layers + (0 if skip_head else 1)
        tl = np.zeros(256 * (12 * n_ops + 4), dtype=np.uint64) if timeline else None
        with torch.cuda.device(self.device):
            rc = self.lib.sd_model_probe_forward(self.handle, int(M), int(pos0), int(iters), 1 if skip_head else 0, _stream(stream, self.device),
                                                 ctypes.byref(usec), ctypes.byref(nbytes),
                                                 tl.ctypes.data if tl is not None else None, tl.size if tl is not None else 0)
        _abi.check(rc, "sd_model_probe_forward")
        return float(usec.value), float(nbytes.value), tl

    def head_argmax(self, x: torch.Tensor, heads: "PackedHeads", rows: Optional[torch.Tensor] = None, per_head: bool = False,
                    normalised: bool = False, stream: Optional[torch.cuda.Stream] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The head evaluation of the Medusa / EAGLE steps on the caller's rows (sd_model_head_argmax): x bf16 [n][d_model];
        rows: int32 device indices into x (None: every row of x in order); heads: pack_heads of [n_heads][vocab][d_model].
        -> (ids int32 [B][n_heads], values float32 [B][n_heads]: the bf16-rounded logit the kernels attached to each id).
        per_head: one launch per head; normalised: x holds final-norm outputs (no norm in front of the product).
        `self.head_launches` then holds what the call enqueued: (matrix launches, rows gathered first)."""
        if x.dim() != 2 or x.dtype != torch.bfloat16 or x.device != self.device or x.shape[1] != self.cfg.d_model or not x.is_contiguous():
            raise ValueError(f"head_argmax: x must be contiguous bf16 [n][{self.cfg.d_model}] on {self.device}")
        if (heads.vocab, heads.d_model) != (self.cfg.vocab, self.cfg.d_model) or heads.buffer.device != self.device:
            raise ValueError(f"head_argmax: heads are [{heads.vocab}][{heads.d_model}], the model's head is [{self.cfg.vocab}][{self.cfg.d_model}]")
        if rows is not None:
            if rows.dtype != torch.int32 or rows.device != self.device or rows.dim() != 1 or not rows.is_contiguous():
                raise ValueError("head_argmax: rows must be a contiguous int32 vector on the model's device")
        B = int(x.shape[0]) if rows is None else int(rows.numel())
        n = len(heads.ptrs)
        ids = torch.empty((B, n), dtype=torch.int32, device=self.device)
        vals = torch.empty((B, n), dtype=torch.float32, device=self.device)
        arr = (ctypes.c_void_p * n)(*heads.ptrs)
        flags = (1 if per_head else 0) | (2 if normalised else 0)      # SD_HEADS_PER_HEAD | SD_HEADS_NORMALISED
        with torch.cuda.device(self.device):
            info = (ctypes.c_int * 2)(0, 0)
            _abi.check(self.lib.sd_model_head_argmax(self.handle, x.data_ptr(), int(x.shape[0]), _ptr(rows), B, n, arr, heads.wd, flags,
                                                     ids.data_ptr(), vals.data_ptr(), info, _stream(stream, self.device)), "sd_model_head_argmax")
        self.head_launches = (int(info[0]), bool(info[1]))
        return ids, vals

    def close(self):
        if getattr(self, "handle", None):
            self.lib.sd_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PackedHeads(NamedTuple):
    """Vocabulary-sized matrices packed by sd_pack_head into one device buffer (pack_heads)."""
    buffer: torch.Tensor     # uint8, owns the storage
    ptrs: List[int]          # device address of each head
    wd: int                  # _abi.SD_BF16 | _abi.SD_FP8_E4M3
    vocab: int
    d_model: int


def pack_heads(heads: torch.Tensor, weight_dtype: str = "bf16", uneven: bool = False) -> PackedHeads:
    """heads bf16 [n][V][d] on a GPU -> each packed (and quantised for fp8) like an lm_head (sd_pack_head), at a constant
    256-byte aligned stride in ONE buffer; uneven: one more 256 bytes in front of the last head (n >= 3), so that the
    stride is not constant and the engine takes one launch per head."""
    if heads.dim() != 3 or heads.dtype != torch.bfloat16 or not heads.is_cuda:
        raise ValueError("pack_heads: need bf16 [n][V][d] on a GPU")
    lib = _abi.load()
    n, V, d = (int(v) for v in heads.shape)
    wd = {"bf16": _abi.SD_BF16, "fp8": _abi.SD_FP8_E4M3}[weight_dtype]
    nbytes = lib.sd_packed_head_bytes(V, d, wd)
    stride = (nbytes + 255) // 256 * 256
    offs = [i * stride + (256 if uneven and i == n - 1 else 0) for i in range(n)]
    with torch.cuda.device(heads.device):
        st = torch.cuda.current_stream(heads.device)
        buf = torch.zeros(offs[-1] + stride + 256, dtype=torch.uint8, device=heads.device)
        base = (buf.data_ptr() + 255) // 256 * 256
        for i in range(n):
            _abi.check(lib.sd_pack_head(heads[i].contiguous().data_ptr(), V, d, wd, base + offs[i], nbytes, st.cuda_stream), "sd_pack_head")
        st.synchronize()
    return PackedHeads(buf, [base + o for o in offs], wd, V, d)


class StepRecord:
    """Host view of one completed step (pinned memory written by the device)."""

    __slots__ = ("accept_len", "n_new", "cur_len", "new_tokens", "draft_tokens", "target_ids", "k_row", "engine_status",
                 "logprob", "rank", "top_ids", "top_logprobs")

    def __init__(self, arr: np.ndarray, K: int, lp: Optional[np.ndarray] = None):
        """arr: the record's slot [B][rec_ints]; lp: the same launch's slot of log-prob words [B][K+1][2 + 2N] (set_logprobs), or
        None while that mode is off."""
        self.accept_len = arr[:, 0].copy()
        self.n_new = arr[:, 1].copy()
        self.cur_len = arr[:, 2].copy()
        self.new_tokens = arr[:, 3:4 + K].copy()
        self.draft_tokens = arr[:, 4 + K:4 + 2 * K].copy()
        self.target_ids = arr[:, 4 + 2 * K:5 + 3 * K].copy()
        # per-token log-probs (HipSpecDec.set_logprobs): entry (b, i) describes new_tokens[b][i]; NaN / -1 where nothing was emitted
        self.logprob = self.rank = self.top_ids = self.top_logprobs = None
        if lp is not None:
            n = (lp.shape[2] - 2) // 2
            w = lp.copy()
            self.logprob = w[:, :, 0].view(np.float32)
            self.rank = w[:, :, 1]
            self.top_ids = w[:, :, 2:2 + n]
            self.top_logprobs = w[:, :, 2 + n:2 + 2 * n].view(np.float32)
        self.k_row = arr[:, 5 + 3 * K].copy()      # proposals that counted per row (per-row adaptive K, confidence gating), else K
        # health word of the models' persistent launches (sd_model_engine_status): a launch that gave up leaves garbage
        self.engine_status = int(arr[0, 6 + 3 * K]) if arr.shape[1] > 6 + 3 * K else 0
        if self.engine_status:
            raise EngineGaveUp(f"a persistent forward gave up (status {self.engine_status:#x}: see sd_model_engine_status); "
                               "the step's outputs are invalid", self.engine_status)


class HipSpecDec:
    """The draft-then-verify step loop on the device (sd_specdec_*)."""

    EMIT_BONUS, EMIT_DRAFT = 0, 1

    def __init__(self, draft: Optional[HipModel], target: HipModel, batch: int, k: int, emit_mode: int = 0):
        """draft=None: self-draft mode (Medusa-lite with heads tied to the lm_head, see sd_specdec_create)."""
        assert draft is None or draft.device == target.device
        self.lib = _abi.load()
        self.draft, self.target = draft, target
        self.device = target.device
        self.B, self.K = int(batch), int(k)
        handle = _vp()
        with torch.cuda.device(self.device):
            _abi.check(self.lib.sd_specdec_create(draft.handle if draft is not None else None, target.handle, self.B, self.K, int(emit_mode),
                                                  ctypes.byref(handle)), "sd_specdec_create")
        self.handle = handle
        # hipGraph capture is not allowed on the legacy default stream: the loop owns two
        # non-default streams (verify/target and draft), ordered by events inside the step
        with torch.cuda.device(self.device):
            self.stream_t = torch.cuda.Stream(self.device)
            self.stream_d = torch.cuda.Stream(self.device)
        # sampling modes (set_sampling / set_spec_sampling): off; their buffers are allocated at first use and kept
        self.sampling = self.spec_sampling = False
        self.acceptance = None     # the lossy acceptance rule of set_acceptance ("typical" / "topk_agree"), None = exact match
        self.spec_shape = None     # (top_k, top_p) of the speculative-sampling mode, None = the whole vocabulary
        self.draft_confidence = None   # (tau, min_k) of set_draft_confidence, None = every row proposes K
        self._conf_logits = self.draft_conf = None
        self.logprobs = None           # top_n of set_logprobs, None = off
        self._lp_words = None          # the pinned words [2][B][K+1][2 + 2N] while the mode is on
        self._logits = self._draft_logits = self._draw = self._stream_ids = None
        # per-row parameters (set_row_sampling): none; the table is allocated at first use and kept (rewritten in place)
        self.row_table = None          # uint8 [B][32] on the device: sd_row_sampling[B], or None while the scalars rule
        self.row_params = None         # the host's view of it: List[SamplingParams]
        self._row_table_buf = None
        # logit processors (set_logit_processors): off; counts / bias tables are allocated at first use and kept
        self.logit_processors = False
        self.logit_counts = self.logit_bias = self._lp_ws = None
        # grammar (set_grammar): none; a TokenFSM's device tables are uploaded once per object and kept
        self.grammar = None
        self.grammar_state = None      # int32 [B] on the device: -1 unconstrained, 0..S-1, 0xFFFF dead
        self._grammar_tables = {}      # id(fsm) -> (fsm, next, allow)
        # kept for the sessions that use the loop one after another (a loop outlives them): the models' paths (persistent /
        # launch) the captured step was recorded on, and the parameters set_adaptive was last enabled with
        self.captured_paths = None
        self.adaptive_params = None
        self.rec_ints = self.lib.sd_specdec_record_ints(self.handle)
        ptr = self.lib.sd_specdec_record(self.handle)
        self._record = np.ctypeslib.as_array(ptr, shape=(2, self.B, self.rec_ints))   # slot = launch index & 1

    def join_current_stream(self):
        """Order the loop's streams after work already enqueued on torch's current
        stream (prefill, weight uploads)."""
        self.stream_t.wait_stream(torch.cuda.current_stream(self.device))

    def set_row(self, b: int, seq_len: int, prev_tok: int, last_tok: int, active: bool = True):
        with torch.cuda.device(self.device):
            _abi.check(self.lib.sd_specdec_set_row(self.handle, b, int(seq_len), int(prev_tok), int(last_tok),
                                                   1 if active else 0, self.stream_t.cuda_stream), "sd_specdec_set_row")

    def set_adaptive(self, enable: bool, initial_k: int = 4, min_k: int = 1, max_k: Optional[int] = None, step_size: int = 1,
                     target_acceptance_rate: float = 0.7):
        """Per-row adaptive K inside the captured step (sd_specdec_set_adaptive): the loop's K is the shape (max_k),
        the device moves every row's own k by the reference's controller rule after each accept scan."""
        max_k = self.K if max_k is None else int(max_k)
        with torch.cuda.device(self.device):
            _abi.check(self.lib.sd_specdec_set_adaptive(self.handle, 1 if enable else 0, int(initial_k), int(min_k), max_k, int(step_size),
                                                        float(target_acceptance_rate), self.stream_t.cuda_stream), "sd_specdec_set_adaptive")
        self.adaptive = bool(enable)

    def set_adaptive_row(self, b: int, k: int, accepted: int = 0, proposed: int = 0, history: Optional[Sequence[float]] = None):
        """Row b's controller state (new sequence: defaults; repair: the host mirror's counters and last <= 4 rates)."""
        hist = None
        n = 1
        if history is not None:
            h = [float(x) for x in history][-4:]
            n = len(h)
            hist = (ctypes.c_double * 4)(*(h + [0.0] * (4 - n)))
        with torch.cuda.device(self.device):
            _abi.check(self.lib.sd_specdec_set_adaptive_row(self.handle, int(b), int(k), int(accepted), int(proposed), n, hist,
                                                            self.stream_t.cuda_stream), "sd_specdec_set_adaptive_row")

    def set_medusa(self, heads: torch.Tensor, weight_dtype: str = "bf16"):
        """Persistent Medusa heads for a loop created with draft=None (sd_specdec_set_medusa). heads: bf16 [K][V][d];
        each is packed (and quantised for fp8) once, like the lm_head."""
        K, V, d = heads.shape
        if K != self.K or heads.dtype != torch.bfloat16 or heads.device != self.device:
            raise ValueError(f"medusa heads must be bf16 [{self.K}][V][d] on {self.device}")
        with torch.cuda.device(self.device):
            self._heads_packed = pack_heads(heads, weight_dtype)      # one buffer, constant stride: the engine evaluates them in one launch
            arr = (ctypes.c_void_p * K)(*self._heads_packed.ptrs)
            _abi.check(self.lib.sd_specdec_set_medusa(self.handle, K, arr, self._heads_packed.wd), "sd_specdec_set_medusa")

    def set_eagle(self, alpha: float = 0.7, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """EAGLE-lite drafting for a loop created with draft=None (sd_specdec_set_eagle): K extrapolated hidden rows
        per step, scored by one lm_head launch. `workspace` (uint8, shared between loops of different K so that the
        per-row state survives a change of K) is allocated for K = 8 when not given; returns it."""
        d = self.target.cfg.d_model
        if workspace is None:
            workspace = torch.zeros(int(self.lib.sd_specdec_eagle_bytes(self.B, 8, d)), dtype=torch.uint8, device=self.device)
        self._eagle_ws = workspace
        _abi.check(self.lib.sd_specdec_set_eagle(self.handle, ctypes.c_float(alpha), workspace.data_ptr(), workspace.numel()),
                   "sd_specdec_set_eagle")
        return workspace

    def reset_eagle(self):
        """Forget the extrapolation state of every row (start of new sequences); ordered on the loop's target stream."""
        _abi.check(self.lib.sd_specdec_reset_eagle(self.handle, self.stream_t.cuda_stream), "sd_specdec_reset_eagle")

    @property
    def _vocab(self) -> int:
        return self.target.weights.config.vocab

    def _step_logits(self) -> torch.Tensor:
        """The step's [B][K+1][V] bf16 logits, allocated at first use: every mode that stores the verify rows shares them."""
        if self._logits is None:
            self._logits = torch.empty((self.B, self.K + 1, self._vocab), dtype=torch.bfloat16, device=self.device)
        return self._logits

    def _upload_draws(self, draw_counts: Optional[Sequence[int]], stream_ids: Optional[Sequence[int]]) -> None:
        """Draw counters (default 0: a new run) and Philox stream ids (default: the row's index), on the current stream."""
        draws = list(draw_counts) if draw_counts is not None else [0] * self.B
        sid = list(stream_ids) if stream_ids is not None else list(range(self.B))
        self._draw = torch.tensor(draws, dtype=torch.int32, device=self.device)
        self._stream_ids = torch.tensor(sid, dtype=torch.int32, device=self.device)

    def set_sampling(self, enable: bool, temperature: float = 1.0, top_k: Optional[int] = None,
                     top_p: Optional[float] = None, seed: int = 0, stream_ids: Optional[Sequence[int]] = None,
                     draw_counts: Optional[Sequence[int]] = None):
        """Sampled bonus token inside the step (sd_specdec_set_sampling). Draw counters start at
        `draw_counts` (default 0: a new run)."""
        with torch.cuda.device(self.device):
            if not enable:
                _abi.check(self.lib.sd_specdec_set_sampling(self.handle, 0, 1.0, 0, 1.0, 0, None, 0, None, None),
                           "sd_specdec_set_sampling")
                self.sampling = False
                return
            logits = self._step_logits()
            self._upload_draws(draw_counts, stream_ids)
            torch.cuda.current_stream(self.device).synchronize()
            _abi.check(self.lib.sd_specdec_set_sampling(
                self.handle, 1, float(temperature), int(top_k) if top_k else 0, 1.0 if top_p is None else float(top_p),
                int(seed) & (2 ** 64 - 1), logits.data_ptr(), logits.numel() * 2, self._draw.data_ptr(),
                self._stream_ids.data_ptr()), "sd_specdec_set_sampling")
            self.sampling = True

    def set_spec_sampling(self, enable: bool, temperature: float = 1.0, seed: int = 0, stream_ids: Optional[Sequence[int]] = None,
                          draw_counts: Optional[Sequence[int]] = None, top_k: Optional[int] = None, top_p: Optional[float] = None):
        """Speculative sampling inside the step (sd_specdec_set_spec_sampling): draft tokens drawn from the draft's
        distribution, accepted with probability min(1, p/q), the first rejection redrawn from the residual — the output is
        distributed as the target's own sampling at `temperature`. The loop owns the two logits buffers (`spec_draft_logits`
        [B][K][V], `step_logits` [B][K+1][V]) and the draw counters (K + 1 per row and step; start at `draw_counts`).
        `top_k` (1..1024), optionally with `top_p` < 1, shapes BOTH distributions as sd_sample_token does
        (sd_specdec_set_spec_shaping): the output is then distributed as the target's own top-k / top-p sampling. Without
        them the mode samples the whole vocabulary; `top_p` without `top_k` is refused."""
        with torch.cuda.device(self.device):
            if not enable:
                _abi.check(self.lib.sd_specdec_set_spec_sampling(self.handle, 0, 1.0, 0, None, 0, None, 0, None, None),
                           "sd_specdec_set_spec_sampling")
                self.spec_sampling = False
                return
            _abi.check(self.lib.sd_specdec_set_spec_shaping(self.handle, int(top_k) if top_k else 0, 1.0 if top_p is None else float(top_p)),
                       "sd_specdec_set_spec_shaping")
            self.spec_shape = (int(top_k), 1.0 if top_p is None else float(top_p)) if top_k else None
            logits = self._step_logits()
            if self._draft_logits is None:
                self._draft_logits = torch.empty((self.B, self.K, self._vocab), dtype=torch.bfloat16, device=self.device)
            self._upload_draws(draw_counts, stream_ids)
            torch.cuda.current_stream(self.device).synchronize()
            _abi.check(self.lib.sd_specdec_set_spec_sampling(
                self.handle, 1, float(temperature), int(seed) & (2 ** 64 - 1), self._draft_logits.data_ptr(),
                self._draft_logits.numel() * 2, logits.data_ptr(), logits.numel() * 2, self._draw.data_ptr(),
                self._stream_ids.data_ptr()), "sd_specdec_set_spec_sampling")
            self.spec_sampling = True

    def set_logit_processors(self, enable: bool, repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
                             frequency_penalty: float = 0.0, bias: bool = False) -> None:
        """Logit processors inside the step (sd_specdec_set_logit_processors): every logits row the step consumes is stored,
        processed in place (penalties from `logit_counts`, then `logit_bias`), then consumed — greedy, sampled-bonus and
        speculative sampling alike. The loop owns the buffers: `logit_counts` (int16 [B][V] holding the uint16 words: bit 15
        prompt, bits 0..14 times generated; zeroed at first use, rows are the caller's to initialise with set_logit_counts_row),
        `logit_bias` (float32 [B][V] of zeros, only with bias=True; -inf bans a token) and the logits [B][K+1][V] (shared with
        the sampling modes: `step_logits`). The values are per loop, the tables per row."""
        with torch.cuda.device(self.device):
            if not enable:
                _abi.check(self.lib.sd_specdec_set_logit_processors(self.handle, 0, 1.0, 0.0, 0.0, None, 0, None, 0, None, 0, None, 0),
                           "sd_specdec_set_logit_processors")
                self.logit_processors = False
                self.grammar = None        # the grammar is a line of this stage: the library unbinds it too
                return
            V = self._vocab
            logits = self._step_logits()
            if self.logit_counts is None:
                self.logit_counts = torch.zeros((self.B, V), dtype=torch.int16, device=self.device)
                self._lp_ws = torch.empty(max(int(self.lib.sd_logit_process_workspace(self.B, self.K + 1, V)), 16), dtype=torch.uint8,
                                          device=self.device)
            if bias and self.logit_bias is None:
                self.logit_bias = torch.zeros((self.B, V), dtype=torch.float32, device=self.device)
            b = self.logit_bias if bias else None
            torch.cuda.current_stream(self.device).synchronize()
            _abi.check(self.lib.sd_specdec_set_logit_processors(
                self.handle, 1, float(repetition_penalty), float(presence_penalty), float(frequency_penalty),
                self.logit_counts.data_ptr(), self.logit_counts.numel() * 2, b.data_ptr() if b is not None else None,
                b.numel() * 4 if b is not None else 0, logits.data_ptr(), logits.numel() * 2, self._lp_ws.data_ptr(),
                self._lp_ws.numel()), "sd_specdec_set_logit_processors")
            self.logit_processors = True

    def set_acceptance(self, rule: Optional[str], temperature: float = 1.0, epsilon: float = 0.09, delta: Optional[float] = 0.3,
                       agree_k: int = 1) -> None:
        """A lossy acceptance rule inside the step (sd_specdec_set_acceptance; None switches it off): "typical" keeps d_{i+1}
        iff p_i(d) >= min(epsilon, delta * exp(-H(p_i))) at `temperature` (delta None: the fixed threshold), "topk_agree" iff
        d is among the `agree_k` largest logits of row i — p_i being the target's distribution after d_1..d_i, the rows of the
        verify forward (`step_logits`, after the logit-processor stage when that is on). The step emits the draft's ids while
        the rule keeps them, then the target's argmax of the next position, or its draw when set_sampling is on."""
        with torch.cuda.device(self.device):
            if rule is None:
                _abi.check(self.lib.sd_specdec_set_acceptance(self.handle, _abi.SD_ACCEPT_OFF, 1.0, 1.0, 1.0, 1, None, 0),
                           "sd_specdec_set_acceptance")
                self.acceptance = None
                return
            if rule not in _abi.ACCEPT_RULES:
                raise ValueError(f"set_acceptance: rule {rule!r} (one of {sorted(_abi.ACCEPT_RULES)})")
            fresh = self._logits is None
            logits = self._step_logits()
            if fresh:
                torch.cuda.current_stream(self.device).synchronize()
            _abi.check(self.lib.sd_specdec_set_acceptance(
                self.handle, _abi.ACCEPT_RULES[rule], float(temperature), float(epsilon), float("inf") if delta is None else float(delta),
                int(agree_k), logits.data_ptr(), logits.numel() * 2), "sd_specdec_set_acceptance")
            self.acceptance = rule

    def set_draft_confidence(self, tau: Optional[float], min_k: int = 1) -> None:
        """Confidence-gated draft length inside the step (sd_specdec_set_draft_confidence; None switches it off): a row stops
        drafting after the first forward i + 1 >= min_k whose confidence — the softmax probability of the draft's own token,
        ops.draft_confidence of the row — is below `tau`; only its first k proposals count (StepRecord.k_row), and a draft
        forward no row needs returns at entry. The device decides alone and starts every step at K: there is no per-row state
        to set or repair. The loop owns the draft's row buffer and `draft_conf` (float32 [B][K]: the last step's confidences of
        the judged forwards that ran, NaN elsewhere). The caller has drained the loop."""
        with torch.cuda.device(self.device):
            if tau is None:
                _abi.check(self.lib.sd_specdec_set_draft_confidence(self.handle, 0, 1.0, 1, None, 0, None), "sd_specdec_set_draft_confidence")
                self.draft_confidence = None
                return
            if self._conf_logits is None:
                n = int(self.lib.sd_specdec_draft_confidence_bytes(self.B, self._vocab))
                self._conf_logits = torch.empty(n // 2, dtype=torch.bfloat16, device=self.device)
                self.draft_conf = torch.full((self.B, self.K), float("nan"), dtype=torch.float32, device=self.device)
                torch.cuda.current_stream(self.device).synchronize()
            _abi.check(self.lib.sd_specdec_set_draft_confidence(
                self.handle, 1, float(tau), int(min_k), self._conf_logits.data_ptr(), self._conf_logits.numel() * 2,
                self.draft_conf.data_ptr()), "sd_specdec_set_draft_confidence")
            self.draft_confidence = (float(tau), int(min_k))

    def set_logprobs(self, top_n: Optional[int]) -> None:
        """Per-token log-probs inside the step (sd_specdec_set_logprobs; None switches it off): every emitted token is described
        by the verify row it was checked against or drawn from — log-prob and rank at temperature 1 over the stored (processed)
        values, and the `top_n` (0..20) largest entries of the row. The numbers arrive with the step record (StepRecord.logprob,
        rank, top_ids, top_logprobs: [B][K+1], entry i for new_tokens[b][i]). The rows are `step_logits`, shared with every mode
        that stores them; a plain greedy step stores them too while this is on. The caller has drained the loop."""
        with torch.cuda.device(self.device):
            if top_n is None:
                _abi.check(self.lib.sd_specdec_set_logprobs(self.handle, 0, 0, None, 0), "sd_specdec_set_logprobs")
                self.logprobs = self._lp_words = None
                return
            fresh = self._logits is None
            logits = self._step_logits()
            if fresh:
                torch.cuda.current_stream(self.device).synchronize()
            _abi.check(self.lib.sd_specdec_set_logprobs(self.handle, 1, int(top_n), logits.data_ptr(), logits.numel() * 2),
                       "sd_specdec_set_logprobs")
            self.logprobs = int(top_n)
            words = int(self.lib.sd_specdec_logprob_words(self.handle))
            self._lp_words = np.ctypeslib.as_array(self.lib.sd_specdec_logprobs(self.handle), shape=(2, self.B, self.K + 1, words))

    def _record_of(self, index: int) -> StepRecord:
        slot = index & 1   # the record of launch i and its log-prob words share slot i & 1
        return StepRecord(self._record[slot], self.K, self._lp_words[slot] if self._lp_words is not None else None)

    def set_logit_counts_row(self, b: int, prompt_ids: Sequence[int], generated_ids: Sequence[int] = ()) -> None:
        """Row b's counts for a new sequence in its slot: the prompt bit of every prompt id, one count per generated id
        (sd_logit_counts_set on the loop's target stream)."""
        from .ops import logit_counts_set
        dev = self.device
        with torch.cuda.device(dev), torch.cuda.stream(self.stream_t):   # the lists are uploaded on the stream that reads them
            p = torch.tensor([int(x) for x in prompt_ids], dtype=torch.int32, device=dev) if len(prompt_ids) else None
            g = torch.tensor([int(x) for x in generated_ids], dtype=torch.int32, device=dev) if len(generated_ids) else None
            logit_counts_set(self.logit_counts, int(b), p, g)

    def set_grammar(self, fsm, eos_id: Optional[int] = None) -> None:
        """A token automaton inside the step (sd_specdec_set_grammar; specdec_hip.grammar.TokenFSM, None unbinds): every
        process launch of the logit-processor stage also masks its row by the state the row's automaton reaches over the step's
        own draft tokens, and the accept stage advances `grammar_state` (int32 [B]) over the emitted tokens. The stage must be
        on (set_logit_processors; identity penalties will do). Binding leaves every row unconstrained (-1) unless the same
        automaton is bound again; set_grammar_state gives a row its start state. The tables are uploaded once per TokenFSM."""
        with torch.cuda.device(self.device):
            if fsm is None:
                _abi.check(self.lib.sd_specdec_set_grammar(self.handle, 0, None, None, 0, None, 0), "sd_specdec_set_grammar")
                self.grammar = None
                return
            V = self._vocab
            if fsm.V != V:
                raise ValueError(f"set_grammar: the automaton is over {fsm.V} tokens, the models' vocabulary has {V}")
            if id(fsm) not in self._grammar_tables:
                from .ops import fsm_tables
                self._grammar_tables[id(fsm)] = (fsm,) + fsm_tables(fsm, self.device)
                torch.cuda.current_stream(self.device).synchronize()
            _, nxt, allow = self._grammar_tables[id(fsm)]
            if self.grammar_state is None:
                self.grammar_state = torch.full((self.B,), -1, dtype=torch.int32, device=self.device)
                torch.cuda.current_stream(self.device).synchronize()
            elif self.grammar is not fsm:
                with torch.cuda.stream(self.stream_t):
                    self.grammar_state.fill_(-1)
            _abi.check(self.lib.sd_specdec_set_grammar(self.handle, 1, nxt.data_ptr(), allow.data_ptr(), fsm.S, self.grammar_state.data_ptr(),
                                                       int(fsm.eos_id if eos_id is None else eos_id)), "sd_specdec_set_grammar")
            self.grammar = fsm

    def set_grammar_state(self, b: int, state: int) -> None:
        """Row b's automaton state (-1: unconstrained), written on the loop's target stream: a new sequence's start state, or
        the host's in-order view after steps that were launched ahead turned out void for the row."""
        if self.grammar_state is None:
            raise RuntimeError("set_grammar_state: no grammar is bound (set_grammar)")
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream_t):
            self.grammar_state[int(b):int(b) + 1].fill_(int(state))

    def set_row_sampling(self, params) -> None:
        """Per-row sampling parameters inside the step (sd_specdec_set_row_sampling): `params` is one SamplingParams per batch
        row (seeds resolved), or None to return to the loop's scalars. With a table the draws, the speculative-sampling
        statistics and the logit-processor launches read row b's temperature, top_k, top_p, seed and penalties from the table
        at run time; the mode and the buffers stay what set_sampling / set_spec_sampling / set_logit_processors configured.
        Either call drops the captured step; set_row_params then rewrites a slot and keeps it."""
        from .sampling_params import ROW_BYTES, pack

        with torch.cuda.device(self.device):
            if params is None:
                _abi.check(self.lib.sd_specdec_set_row_sampling(self.handle, None), "sd_specdec_set_row_sampling")
                self.row_table = self.row_params = None
                return
            params = list(params)
            if len(params) != self.B:
                raise ValueError(f"set_row_sampling: {len(params)} entries for {self.B} rows")
            if self._row_table_buf is None:
                self._row_table_buf = torch.zeros((self.B, ROW_BYTES), dtype=torch.uint8, device=self.device)
            with torch.cuda.stream(self.stream_t):
                self._row_table_buf.copy_(pack(params, self.device))
            _abi.check(self.lib.sd_specdec_set_row_sampling(self.handle, self._row_table_buf.data_ptr()), "sd_specdec_set_row_sampling")
            self.row_table = self._row_table_buf
            self.row_params = params

    def set_row_params(self, b: int, params, stream_id: Optional[int] = None, draw_count: Optional[int] = None) -> None:
        """Slot b's entry of the bound table <- `params` (a SamplingParams, seed resolved), written on the loop's target stream:
        a new request in the slot. stream_id / draw_count: the slot's Philox stream and draw counter, rewritten the same way.
        The captured step is kept — its kernels read all three at run time."""
        from .sampling_params import pack

        if self.row_table is None:
            raise RuntimeError("set_row_params: no table is bound (set_row_sampling)")
        b = int(b)
        if not 0 <= b < self.B:
            raise ValueError(f"set_row_params: row {b} of {self.B}")
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream_t):
            self.row_table[b:b + 1].copy_(pack([params], self.device))
            if stream_id is not None:
                self._stream_ids[b:b + 1].fill_(int(stream_id))
            if draw_count is not None:
                self._draw[b:b + 1].copy_(torch.tensor([int(draw_count) & 0xFFFFFFFF], dtype=torch.int64).to(torch.int32).to(self.device))
        self.row_params[b] = params

    @property
    def stream_ids(self) -> List[int]:
        """The rows' Philox stream ids on the device (synchronises)."""
        return [int(x) for x in self._stream_ids.cpu().tolist()]

    def set_draw_counts(self, draw_counts: Sequence[int]) -> None:
        """Rewrite the rows' draw counters (sampling modes) on the loop's target stream: the host's in-order view after steps
        that were launched ahead turned out void for a row. The captured step is kept."""
        host = torch.tensor([int(x) & 0xFFFFFFFF for x in draw_counts], dtype=torch.int64).to(torch.int32)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream_t):
            self._draw.copy_(host.to(self.device))

    @property
    def draw_counts(self) -> List[int]:
        """The device's draw counters (synchronises)."""
        return [int(x) & 0xFFFFFFFF for x in self._draw.cpu().tolist()]

    @property
    def spec_draft_logits(self) -> torch.Tensor:
        """[B][K][V] bf16: row (b, i) = the logits d_{i+1} was drawn from in the last step (speculative sampling only)."""
        return self._draft_logits

    @property
    def step_logits(self) -> torch.Tensor:
        """[B][K+1][V] bf16 logits of the last verify forward (sampling modes only)."""
        return self._logits

    def step(self, use_graph: bool = True, two_streams: bool = True):
        if os.environ.get("SPECDEC_ONE_STREAM"):   # experiment knob: draft and verify on one stream (no fork/join events)
            two_streams = False
        with torch.cuda.device(self.device):
            sd = self.stream_d.cuda_stream if two_streams else None
            _abi.check(self.lib.sd_specdec_step(self.handle, self.stream_t.cuda_stream, sd,
                                                1 if use_graph else 0), "sd_specdec_step")

    def sync(self) -> StepRecord:
        """Drain the loop's stream; the record of the LAST launched step."""
        with torch.cuda.device(self.device):
            _abi.check(self.lib.sd_specdec_sync(self.handle, self.stream_t.cuda_stream), "sd_specdec_sync")
        last = max(int(self.lib.sd_specdec_launches(self.handle)) - 1, 0)
        return self._record_of(last)

    @property
    def launches(self) -> int:
        return int(self.lib.sd_specdec_launches(self.handle))

    @property
    def graph_nodes(self) -> int:
        """Nodes of the captured step's graph (0: no step is captured) — sd_specdec_graph_nodes."""
        return int(self.lib.sd_specdec_graph_nodes(self.handle))

    def invalidate(self) -> None:
        """Drop the captured step (a model's path changed: set_persist_tokens / set_length_hint / a re-bind). The caller has
        drained the loop; the next step runs eagerly, the one after it captures again (sd_specdec_invalidate)."""
        _abi.check(self.lib.sd_specdec_invalidate(self.handle), "sd_specdec_invalidate")

    def drain(self) -> None:
        """Wait for everything launched, without reading a record (recovery path: the records may be invalid)."""
        with torch.cuda.device(self.device):
            _abi.check(self.lib.sd_specdec_sync(self.handle, self.stream_t.cuda_stream), "sd_specdec_sync")
            _abi.check(self.lib.sd_specdec_sync(self.handle, self.stream_d.cuda_stream), "sd_specdec_sync")

    def wait(self, launch_index: int) -> StepRecord:
        """Wait for one of the last two launched steps (the other may still be running) and return its record."""
        with torch.cuda.device(self.device):
            _abi.check(self.lib.sd_specdec_wait(self.handle, int(launch_index)), "sd_specdec_wait")
        return self._record_of(launch_index)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.sd_specdec_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
