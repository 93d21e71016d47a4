"""Per-request sampling parameters: the host side of sd_row_sampling (include/specdec_hip.h).

A `SamplingParams` is one request's temperature, top_k, top_p, seed and penalties. `pack` turns a list of them into the
table the _rows kernels read (one 32-byte record per batch row). The kernels normalise whatever a record holds — a value
they cannot honour becomes a greedy row or identity penalties — so the dataclass refuses such values here, with the
messages the scalar paths use, instead of letting a request silently decode greedily.

This module imports neither torch nor the library at import time: validation, packing to bytes and the JSON form work
without a GPU.
"""

from __future__ import annotations

import ctypes
import json
import math
from dataclasses import dataclass, fields
from typing import Any, List, Optional, Sequence

MAX_TOP_K = 1024   # kSampleMaxK (csrc/sample_device.h)


class RowSampling(ctypes.Structure):
    """sd_row_sampling, field for field."""

    _fields_ = [("temperature", ctypes.c_float), ("top_k", ctypes.c_int32), ("top_p", ctypes.c_float),
                ("seed_lo", ctypes.c_uint32), ("seed_hi", ctypes.c_uint32),
                ("repetition_penalty", ctypes.c_float), ("presence_penalty", ctypes.c_float), ("frequency_penalty", ctypes.c_float)]


ROW_BYTES = ctypes.sizeof(RowSampling)


def check_penalties(rp: float, pres: float, freq: float) -> None:
    """What a repetition / presence / frequency penalty may be, for a request's own and for a call's."""
    if not rp > 0.0:
        raise ValueError(f"repetition_penalty={rp} (must be > 0)")
    if not (math.isfinite(pres) and math.isfinite(freq)):
        raise ValueError(f"presence_penalty={pres} / frequency_penalty={freq} must be finite")


@dataclass(frozen=True)
class SamplingParams:
    """One request's sampling parameters. temperature 0 asks for greedy decoding; top_k None / 0 = no top-k (else 1..1024);
    top_p None / >= 1 = no nucleus cut; seed None = the call's seed; the penalties as the call-level arguments define them
    (src/specdec/core/step_options.py)."""

    temperature: float = 1.0
    top_k: Optional[int] = None
    top_p: Optional[float] = None
    seed: Optional[int] = None
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0

    def __post_init__(self):
        t = float(self.temperature)
        if math.isnan(t) or t < 0.0 or math.isinf(t):
            raise ValueError(f"temperature={self.temperature} (must be a finite value >= 0; 0 is greedy)")
        if self.top_k is not None and int(self.top_k) != self.top_k:
            raise ValueError(f"top_k={self.top_k} (an integer)")
        if self.top_k is not None and int(self.top_k) < 0:
            raise ValueError(f"top_k={self.top_k} (must be >= 0; 0 or None: no top-k)")
        if self.top_p is not None and not float(self.top_p) > 0.0:
            raise ValueError(f"top_p={self.top_p} (must be > 0)")
        check_penalties(float(self.repetition_penalty), float(self.presence_penalty), float(self.frequency_penalty))
        if self.seed is not None and int(self.seed) != self.seed:
            raise ValueError(f"seed={self.seed} (an integer)")

    # ---- what the request asks for
    @property
    def greedy(self) -> bool:
        return float(self.temperature) == 0.0

    @property
    def has_penalties(self) -> bool:
        return not (float(self.repetition_penalty) == 1.0 and float(self.presence_penalty) == 0.0 and float(self.frequency_penalty) == 0.0)

    def check(self, vocab: int, spec: bool = False) -> None:
        """Refuse what the device would only turn into a greedy row: top_k above 1024 after the clamp to the vocabulary and, for
        speculative sampling (`spec`), the full-vocabulary nucleus."""
        k = int(self.top_k) if self.top_k else 0
        if k and min(k, int(vocab)) > MAX_TOP_K:
            if spec:
                raise NotImplementedError(f"policy='rejection' (backend='device'): top_k={k} is outside 1..1024")
            raise NotImplementedError(f"do_sample=True: top_k={k} > 1024 is not on the HIP path")
        if spec and not self.greedy and not k and self.top_p is not None and float(self.top_p) < 1.0:
            raise NotImplementedError("policy='rejection' (backend='device'): top_p without top_k (the full-vocabulary nucleus) is not "
                                      "supported; give a top_k in 1..1024")

    def scalars(self, spec: bool = False, vocab: Optional[int] = None) -> dict:
        """The entry as the kernels normalise it (normalise_row_sampling): the arguments of the scalar op that gives this row's
        result — temperature, top_k (None: no top-k), top_p (None: no cut), seed."""
        k = int(self.top_k) if self.top_k else 0
        p = 1.0 if self.top_p is None or float(self.top_p) >= 1.0 else float(self.top_p)
        t = float(self.temperature)
        greedy = not t > 0.0 or (k and vocab is not None and min(k, int(vocab)) > MAX_TOP_K) or (spec and not k and p < 1.0)
        if greedy:
            t, k, p = 1.0, 1, 1.0
        return {"temperature": t, "top_k": k or None, "top_p": None if p >= 1.0 else p, "seed": int(self.seed or 0)}

    def record(self, default_seed: int = 0) -> RowSampling:
        seed = int(default_seed if self.seed is None else self.seed) & (2 ** 64 - 1)
        return RowSampling(float(self.temperature), int(self.top_k) if self.top_k else 0, 1.0 if self.top_p is None else float(self.top_p),
                           seed & 0xFFFFFFFF, seed >> 32, float(self.repetition_penalty), float(self.presence_penalty),
                           float(self.frequency_penalty))

    def with_seed(self, default_seed: int) -> "SamplingParams":
        """The same request with its seed resolved (its own, else `default_seed`)."""
        if self.seed is not None:
            return self
        return SamplingParams(**{**{f.name: getattr(self, f.name) for f in fields(self)}, "seed": int(default_seed)})

    @classmethod
    def from_dict(cls, d: Any) -> "SamplingParams":
        if not isinstance(d, dict):
            raise ValueError(f"sampling parameters: expected an object, got {type(d).__name__}")
        names = {f.name for f in fields(cls)}
        unknown = set(d) - names
        if unknown:
            raise ValueError(f"sampling parameters: unknown key(s) {sorted(unknown)} (known: {sorted(names)})")
        return cls(**d)


def pack_bytes(params: Sequence[SamplingParams], default_seed: int = 0) -> bytes:
    """The table of `params` as bytes: len(params) records of 32 bytes."""
    arr = (RowSampling * len(params))(*[p.record(default_seed) for p in params])
    return bytes(arr)


def pack(params: Sequence[SamplingParams], device, default_seed: int = 0):
    """The table of `params` on `device`: a uint8 [B][32] tensor (torch allocations are 16-byte aligned, as the kernels need)."""
    import torch

    if not params:
        raise ValueError("pack: an empty list of sampling parameters")
    host = torch.frombuffer(bytearray(pack_bytes(params, default_seed)), dtype=torch.uint8).view(len(params), ROW_BYTES)
    return host.to(device)


def unpack(table) -> List[RowSampling]:
    """The records of a table tensor (synchronises)."""
    raw = bytes(table.detach().cpu().contiguous().view(-1).tolist())
    return list((RowSampling * (len(raw) // ROW_BYTES)).from_buffer_copy(raw))


def load_for_cli(path: Optional[str], n_prompts: int, clashes: dict) -> Optional[List[SamplingParams]]:
    """--sampling-params of a command line: None without the option, else load_file — refused next to the options in `clashes`
    ({option: its value}; those given, i.e. neither None nor False, carry a parameter the file's entries carry already, or
    select a mode the entries are not read in)."""
    if path is None:
        return None
    given = sorted(k for k, v in clashes.items() if v is not None and v is not False)
    if given:
        raise ValueError(f"--sampling-params cannot be combined with {', '.join(given)}")
    return load_file(path, n_prompts)


def load_file(path: str, n_prompts: int) -> List[SamplingParams]:
    """--sampling-params FILE of the command lines: a JSON list with one object per prompt."""
    with open(path) as f:
        try:
            data = json.load(f)
        except json.JSONDecodeError as e:
            raise ValueError(f"{path}: not JSON ({e})") from e
    if not isinstance(data, list):
        raise ValueError(f"{path}: expected a JSON list with one object per prompt")
    if len(data) != n_prompts:
        raise ValueError(f"{path}: {len(data)} entries for {n_prompts} prompt(s)")
    return [SamplingParams.from_dict(d) for d in data]
