"""Perplexity of a text under a HIP model, scored on the device (HipLM.score: sd_model_score).

The counterpart of the reference's `PerplexityEvaluator` (same constructor, `calculate_perplexity` and `compare_texts`, same result
keys). The model is what `create_hip_lm` builds from `model_name`: a local checkpoint directory, "synthetic:<preset>" or a hub name
of the reference's configs (synthetic weights of that shape when no local copy exists). Nothing is downloaded.
"""

from __future__ import annotations

import logging
import math
from typing import Any, Dict, List, Optional

logger = logging.getLogger(__name__)


class PerplexityEvaluator:
    """Evaluates text quality using perplexity scores: exp of the mean negative log-likelihood of tokens 1..n-1 (the
    `labels=input_ids` loss of a HF causal LM), over at most `max_length` tokens of the text."""

    def __init__(self, model_name: str, device: str = "cuda", model: Any = None, max_length: int = 512):
        """`model`: anything with `encode(text) -> ids` and `score(ids) -> (logprob [n-1], greedy [n])` (default: create_hip_lm)."""
        self.model_name = model_name
        self.device = device
        self.max_length = int(max_length)
        self.logger = logging.getLogger(__name__)
        if model is None:
            from src.specdec.models.hip_lm import create_hip_lm

            self.logger.info("Loading evaluation model: %s", model_name)
            model = create_hip_lm(model_name, device=device, max_len=max(self.max_length + 64, 1024))
        self.model = model

    def _ids(self, text: str) -> List[int]:
        ids = self.model.encode(text)
        ids = ids.reshape(-1).tolist() if hasattr(ids, "reshape") else list(ids)
        return [int(i) for i in ids[: self.max_length]]   # truncation=True, max_length

    def calculate_perplexity(self, text: str) -> Dict[str, Any]:
        """{perplexity, loss, text_length, token_count, model, device}; on failure perplexity = loss = inf plus `error`."""
        token_count = 0
        try:
            ids = self._ids(text)
            token_count = len(ids)
            if token_count < 2:
                raise ValueError(f"{token_count} token(s): perplexity needs at least 2")
            logprob, _ = self.model.score(ids)
            lp = [float(v) for v in (logprob.double().cpu().tolist() if hasattr(logprob, "cpu") else logprob)]
            loss = -math.fsum(lp) / len(lp)
            if not math.isfinite(loss):
                raise FloatingPointError(f"non-finite loss {loss}")
            return {
                "perplexity": math.exp(loss),
                "loss": loss,
                "text_length": len(text),
                "token_count": token_count,
                "model": self.model_name,
                "device": self.device,
            }
        except Exception as e:
            self.logger.error("Perplexity calculation failed: %s", e)
            return {
                "perplexity": float("inf"),
                "loss": float("inf"),
                "text_length": len(text),
                "token_count": 0,
                "model": self.model_name,
                "device": self.device,
                "error": str(e),
            }

    def compare_texts(self, texts: List[str], labels: Optional[List[str]] = None) -> Dict[str, Any]:
        """Per-text results (with `label`) and the mean / min / max perplexity over the texts that scored (`count` of them)."""
        if labels is None:
            labels = [f"text_{i}" for i in range(len(texts))]
        results = []
        for text, label in zip(texts, labels):
            r = self.calculate_perplexity(text)
            r["label"] = label
            results.append(r)
        ppl = [r["perplexity"] for r in results if r["perplexity"] != float("inf")]
        inf = float("inf")
        return {
            "results": results,
            "statistics": {
                "avg_perplexity": sum(ppl) / len(ppl) if ppl else inf,
                "min_perplexity": min(ppl) if ppl else inf,
                "max_perplexity": max(ppl) if ppl else inf,
                "count": len(ppl),
            },
            "model": self.model_name,
            "device": self.device,
        }
