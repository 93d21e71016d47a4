"""Perplexity of a text under a HIP model, scored on the device (HipLM.score: sd_model_score), and the agreement of a draft model
with a target on a text (AgreementEvaluator: SpeculativePipeline.draft_agreement, sd_spec_agreement).

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


class AgreementEvaluator:
    """Evaluates how well a draft model fits a target on given texts, without generating: per-position acceptance probability
    of speculative sampling, KL(target || draft) and greedy agreement, over at most `max_length` tokens of a text
    (SpeculativePipeline.draft_agreement, reduced on the device)."""

    def __init__(self, base_model: str, draft_model: str, device: str = "cuda", pipeline: Any = None, max_length: int = 512,
                 temperature: float = 1.0, chunk: int = 256):
        """`pipeline`: anything with `draft_agreement(ids, temperature, chunk) -> dict` and `_encode(text) -> ids` (default: a
        SpeculativePipeline over create_hip_lm's models)."""
        self.base_model, self.draft_model = base_model, draft_model
        self.device = device
        self.max_length = int(max_length)
        self.temperature = float(temperature)
        self.chunk = int(chunk)
        self.logger = logging.getLogger(__name__)
        if pipeline is None:
            from src.specdec.core.pipeline import SpeculativePipeline

            self.logger.info("Loading models: %s / %s", base_model, draft_model)
            pipeline = SpeculativePipeline(base_model=base_model, draft_model=draft_model, device=device)
        self.pipeline = pipeline

    def calculate_agreement(self, text: Any) -> Dict[str, Any]:
        """{mean_alpha, mean_kl, greedy_agreement, expected_tokens_per_step, token_count, temperature, base_model, draft_model,
        device}; on failure the three means are NaN plus `error`."""
        try:
            ids = [int(i) for i in self.pipeline._encode(text)][: self.max_length]
            r = self.pipeline.draft_agreement(ids, temperature=self.temperature, chunk=self.chunk)
            return {"mean_alpha": r["mean_alpha"], "mean_kl": r["mean_kl"], "greedy_agreement": r["greedy_agreement"],
                    "expected_tokens_per_step": r["expected_tokens_per_step"], "token_count": len(ids),
                    "temperature": self.temperature, "base_model": self.base_model, "draft_model": self.draft_model,
                    "device": self.device}
        except Exception as e:
            self.logger.error("Agreement calculation failed: %s", e)
            nan = float("nan")
            return {"mean_alpha": nan, "mean_kl": nan, "greedy_agreement": nan, "expected_tokens_per_step": None, "token_count": 0,
                    "temperature": self.temperature, "base_model": self.base_model, "draft_model": self.draft_model,
                    "device": self.device, "error": str(e)}

    def compare_texts(self, texts: List[Any], labels: Optional[List[str]] = None) -> Dict[str, Any]:
        """Per-text results (with `label`) and the mean acceptance probability / greedy agreement over the texts that scored."""
        if labels is None:
            labels = [f"text_{i}" for i in range(len(texts))]
        results = []
        for text, label in zip(texts, labels):
            r = self.calculate_agreement(text)
            r["label"] = label
            results.append(r)
        ok = [r for r in results if "error" not in r]
        nan = float("nan")
        return {"results": results,
                "statistics": {"avg_alpha": sum(r["mean_alpha"] for r in ok) / len(ok) if ok else nan,
                               "avg_greedy_agreement": sum(r["greedy_agreement"] for r in ok) / len(ok) if ok else nan,
                               "count": len(ok)},
                "base_model": self.base_model, "draft_model": self.draft_model, "device": self.device}
