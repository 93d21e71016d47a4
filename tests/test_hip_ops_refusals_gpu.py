"""The argument checks the sampling-side wrappers of specdec_hip.ops share: every wrapper refuses each kind of malformed
argument with the full text its own copy of the check had before the copies became one, the op's name in front. The texts are
literals here, not taken from ops.py. Every refusal is raised in Python before the library is called: no kernel runs."""

import pytest
import torch

from specdec_hip import ops
from specdec_hip.sampling_params import ROW_BYTES

pytestmark = pytest.mark.gpu

B, K, V, S = 2, 2, 64, 3
DEV = "cuda:0"


def _i32(*shape):
    return torch.zeros(shape, dtype=torch.int32, device=DEV)


def _bf16(*shape):
    return torch.zeros(shape, dtype=torch.bfloat16, device=DEV)


def _good():
    """One well-formed value of every argument the ten wrappers take."""
    return dict(logits=_bf16(B, V), q=_bf16(B, K, V), p=_bf16(B, K + 1, V), ids=_i32(B, K), rows=_bf16(B, K + 1, V),
                counts=ops.logit_counts(B, V, DEV), table=torch.zeros((B, ROW_BYTES), dtype=torch.uint8, device=DEV),
                nxt=torch.zeros((S, V), dtype=torch.int16, device=DEV), allow=_i32(S, V // 32), state=_i32(B), tokens=_i32(B, K),
                n_new=_i32(B))


# op -> (name in the messages, call(g, **overrides of optional arguments))
OPS = {
    "sample_token_hip": ("sample_token", lambda g, **kw: ops.sample_token_hip(g["logits"], 1.0, **kw)),
    "sample_token_rows_hip": ("sample_token_rows", lambda g, **kw: ops.sample_token_rows_hip(g["logits"], g["table"], **kw)),
    "spec_sample_accept_hip": ("spec_sample_accept", lambda g, **kw: ops.spec_sample_accept_hip(g["q"], g["p"], g["ids"], 1.0, **kw)),
    "spec_sample_accept_rows_hip": ("spec_sample_accept_rows",
                                    lambda g, **kw: ops.spec_sample_accept_rows_hip(g["q"], g["p"], g["ids"], g["table"], **kw)),
    "logit_process": ("logit_process", lambda g, **kw: ops.logit_process(g["rows"], g["counts"], **kw)),
    "logit_process_fsm": ("logit_process_fsm",
                          lambda g, **kw: ops.logit_process_fsm(g["rows"], g["counts"], g["nxt"], g["allow"], g["state"], 0, **kw)),
    "logit_process_rows_hip": ("logit_process_rows", lambda g, **kw: ops.logit_process_rows_hip(g["rows"], g["counts"], g["table"], **kw)),
    "logit_counts_add": ("logit_counts_add", lambda g, **kw: ops.logit_counts_add(g["counts"], g["tokens"], g["n_new"], **kw)),
    "fsm_advance": ("fsm_advance", lambda g, **kw: ops.fsm_advance(g["nxt"], g["state"], g["tokens"], g["n_new"], **kw)),
    "logit_counts_set": ("logit_counts_set", lambda g, **kw: ops.logit_counts_set(g["counts"], 0, **kw)),
}
DRAWS = ["sample_token_hip", "sample_token_rows_hip", "spec_sample_accept_hip", "spec_sample_accept_rows_hip"]
PROCESS = ["logit_process", "logit_process_fsm", "logit_process_rows_hip"]


def _refused(op, text, g=None, **kw):
    with pytest.raises(ValueError) as e:
        OPS[op][1](g or _good(), **kw)
    assert str(e.value) == text


@pytest.mark.parametrize("op", DRAWS + PROCESS + ["logit_counts_add", "fsm_advance"])
def test_wrong_dtype_active(op):
    _refused(op, f"{OPS[op][0]}: active must be a contiguous int32 [2] tensor on cuda:0", active=torch.zeros(B, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("op", DRAWS)
def test_non_contiguous_stream_ids(op):
    _refused(op, f"{OPS[op][0]}: stream_ids must be a contiguous int32 [2] tensor on cuda:0", stream_ids=_i32(2 * B)[::2])


@pytest.mark.parametrize("op", PROCESS)
def test_counts_of_another_vocabulary(op):
    g = _good()
    g["counts"] = ops.logit_counts(B, V // 2, DEV)
    _refused(op, f"{OPS[op][0]}: counts (2, 32) for rows (2, 3, 64)", g)


@pytest.mark.parametrize("op", PROCESS + ["logit_counts_add", "logit_counts_set"])
def test_counts_of_the_wrong_shape(op):
    g = _good()
    g["counts"] = torch.zeros((B, 1, V), dtype=torch.int16, device=DEV)
    _refused(op, f"{OPS[op][0]}: counts must be a contiguous int16 [B][V] tensor on cuda:0 (logit_counts)", g)


@pytest.mark.parametrize("op", PROCESS)
def test_rows_with_a_non_unit_inner_stride(op):
    g = _good()
    g["rows"] = _bf16(B, K + 1, 2 * V)[:, :, ::2]
    _refused(op, f"{OPS[op][0]}: rows must have a unit inner stride and one constant stride >= V between consecutive rows "
                 "(in place: no copy is made)", g)


@pytest.mark.parametrize("op", PROCESS)
def test_bias_of_the_wrong_shape(op):
    _refused(op, f"{OPS[op][0]}: bias must be a contiguous float32 [2][64] tensor on cuda:0",
             bias=torch.zeros((B, V + 1), dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("op", PROCESS)
def test_in_step_tokens_on_the_wrong_row_count(op):
    _refused(op, f"{OPS[op][0]}: tokens must be a contiguous int32 [2][n] tensor on cuda:0", tokens=_i32(B + 1, K))


@pytest.mark.parametrize("op", ["logit_counts_add", "fsm_advance"])
def test_new_tokens_on_the_wrong_row_count(op):
    g = _good()
    g["tokens"] = _i32(B + 1, K)
    _refused(op, f"{OPS[op][0]}: tokens must be a contiguous int32 [2][n] tensor", g)


def test_allow_table_of_the_wrong_width():
    g = _good()
    g["allow"] = _i32(S, V // 32 + 1)
    _refused("logit_process_fsm", "logit_process_fsm: tables (3, 64) / (3, 3) for V=64 (fsm_tables)", g)
    with pytest.raises(ValueError) as e:
        ops.logit_process_rows_hip(g["rows"], g["counts"], g["table"], nxt=g["nxt"], allow=g["allow"], fsm_state=g["state"])
    assert str(e.value) == "logit_process_rows: tables (3, 64) / (3, 3) for V=64 (fsm_tables)"


def test_logits_that_do_not_divide_into_entries():
    for op in ("sample_token_hip", "sample_token_rows_hip"):
        _refused(op, f"{OPS[op][0]}: 2 rows is not a multiple of rows_per_entry=3", rows_per_entry=3)


@pytest.mark.parametrize("op", ["spec_sample_accept_hip", "spec_sample_accept_rows_hip"])
def test_target_logits_without_the_bonus_row(op):
    g = _good()
    g["p"] = _bf16(B, K, V)
    _refused(op, f"{OPS[op][0]}: shapes (2, 2, 64) / (2, 2, 64) / (2, 2)", g)
