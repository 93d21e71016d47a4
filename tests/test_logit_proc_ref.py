"""The CPU restatement of the logit processors (tests/logit_proc_ref.py) against transformers' RepetitionPenaltyLogitsProcessor
on float32 rows (where transformers imports; the formula otherwise), hand-made cases for the in-step count and for the prompt
bit without a generated count, the identity, the argmax rule and the two count updates; and the new flags of the two CLIs."""

import numpy as np
import pytest
import torch

import logit_proc_ref as L


def _bits(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _row(V, seed):
    rng = np.random.default_rng(seed)
    bits = _bits(rng.normal(0, 3.0, V))
    bits[:3] = _bits([0.0, -0.0, 2.5])
    return bits


def test_bf16_rounding_is_torchs():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.normal(0, 5, 4096).astype(np.float32),
                        np.array([0.0, -0.0, np.inf, -np.inf, 1.00390625, 1.01171875, 3.3895314e38, -3.3895314e38, 1e-30], dtype=np.float32)])
    assert np.array_equal(L.f32_to_bf16(x), _bits(x))           # round to nearest even, ties included, overflow to inf
    assert L.f32_to_bf16(np.float32(np.nan)) == L.NAN_BF16
    assert np.array_equal(L.bf16_to_f32(_bits(x)), torch.as_tensor(x).to(torch.bfloat16).float().numpy())


@pytest.mark.parametrize("rp", [1.3, 0.8, 2.0])
def test_repetition_penalty_is_hfs(rp):
    V = 4099
    bits = _row(V, 1)
    seen = [0, 1, 2, 17, 900, 4098]     # x == 0 and -0 among them: they take the division
    x = L.bf16_to_f32(bits)
    try:
        from transformers import RepetitionPenaltyLogitsProcessor
        want = RepetitionPenaltyLogitsProcessor(rp)(torch.tensor([seen]), torch.from_numpy(x.copy())[None])[0].numpy()
    except ImportError:
        want = x.copy()
        want[seen] = np.where(x[seen] < 0, x[seen] * np.float32(rp), x[seen] / np.float32(rp))
    want_bits = _bits(want)
    # the same ids as prompt tokens, as generated tokens (no other penalty) and as in-step tokens: one transform
    as_prompt = L.process_row(bits, L.counts_set(V, seen), rp=rp)
    as_generated = L.process_row(bits, L.counts_set(V, [], seen), rp=rp)
    as_in_step = L.process_row(bits, np.zeros(V, np.uint16), in_step=seen, rp=rp)
    for got in (as_prompt, as_generated, as_in_step):
        assert np.array_equal(got, want_bits)
    assert np.array_equal(as_prompt[[5, 6, 7]], bits[[5, 6, 7]])     # unseen tokens keep their bits


def test_in_step_count_prompt_bit_and_order_of_operations():
    V = 16
    x = np.array([4.0, -4.0, 4.0, 4.0, 4.0, 4.0] + [1.0] * 10, dtype=np.float32)
    bits = _bits(x)
    counts = np.zeros(V, np.uint16)
    counts[0] = L.PROMPT_BIT            # prompt only: repetition penalty, no presence / frequency
    counts[1] = 2                       # generated twice
    counts[2] = L.PROMPT_BIT | 1        # prompt and generated once
    counts[3] = L.COUNT_MASK            # saturated count
    # token 4: twice in step (t_1 == t_2); token 0: in step AND prompt bit -> now counts as generated once; token 5 untouched
    got = L.bf16_to_f32(L.process_row(bits, counts, in_step=[4, 4, 0], rp=2.0, presence=0.5, frequency=0.25))
    f = np.float32
    assert got[1] == f(f(f(-4.0) * f(2.0)) - f(0.5)) - f(f(0.25) * f(2.0))          # -8 - 0.5 - 0.5
    assert got[2] == f(f(f(4.0) / f(2.0)) - f(0.5)) - f(0.25)                       # 2 - 0.5 - 0.25
    assert got[4] == f(f(2.0) - f(0.5)) - f(0.5)                                     # c = 2 from the step alone
    assert got[0] == f(f(2.0) - f(0.5)) - f(0.25)                                    # prompt bit + one in-step occurrence
    assert got[5] == 4.0 and got[6] == 1.0
    want3 = L.bf16_to_f32(L.f32_to_bf16(f(f(2.0) - f(0.5)) - f(f(0.25) * f(32767.0))))
    assert got[3] == want3
    # prompt bit without a generated count, presence / frequency only: untouched
    assert np.array_equal(L.process_row(bits, counts, rp=1.0, presence=0.5, frequency=0.25)[0], bits[0])
    # positions of a verify pass: row r sees the first r in-step tokens
    rows = np.stack([bits, bits, bits])[None]
    out, ids = L.process_rows(rows, np.zeros((1, V), np.uint16), tokens=[[4, 4]], presence=1.0)
    assert L.bf16_to_f32(out[0, :, 4]).tolist() == [4.0, 3.0, 3.0]
    assert ids[0].tolist() == [0, 0, 0]
    # bias: -inf bans, the ban of every larger value moves the argmax; +inf + -inf is NaN and NaN wins the argmax
    bias = np.zeros((1, V), np.float32)
    bias[0, [0, 2, 3, 4, 5]] = -np.inf
    out, ids = L.process_rows(rows[:, :1], np.zeros((1, V), np.uint16), bias=bias)
    assert ids[0, 0] == 6 and np.isneginf(L.bf16_to_f32(out[0, 0, 0]))
    r2 = bits.copy()
    r2[9] = _bits([np.inf])[0]
    bias[0, 9] = -np.inf
    out, ids = L.process_rows(r2[None, None], np.zeros((1, V), np.uint16), bias=bias)
    assert out[0, 0, 9] == L.NAN_BF16 and ids[0, 0] == 9


def test_identity_returns_the_row_unchanged():
    V = 50257
    bits = _row(V, 2)
    bits[100] = _bits([np.inf])[0]
    bits[101] = _bits([-np.inf])[0]
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 4, V).astype(np.uint16) | (rng.integers(0, 2, V).astype(np.uint16) << 15)
    got = L.process_row(bits, counts, in_step=[5, 5, 9], rp=1.0, presence=0.0, frequency=0.0)
    assert np.array_equal(got, bits)
    bits[7] = 0x7FC1                     # a NaN keeps being a NaN (its payload is not kept)
    assert L.process_row(bits, counts)[7] == L.NAN_BF16
    rows = bits[None, None]
    out, ids = L.process_rows(rows, counts[None], rp=3.0, presence=1.0, frequency=1.0, active=[0])
    assert np.array_equal(out, rows) and ids[0, 0] == 7     # inactive: untouched, argmax of the row as it is (NaN first)


def test_argmax_rule():
    assert L.argmax_bits(_bits([1.0, 3.0, 3.0, 2.0])) == 1                 # ties: lowest index
    assert L.argmax_bits(_bits([1.0, np.nan, np.inf, np.nan])) == 1        # NaN beats +inf, the first NaN wins
    assert L.argmax_bits(_bits([-np.inf, -np.inf])) == 0
    assert L.argmax_bits(_bits([-0.0, 0.0])) == 0                          # -0 == 0


def test_count_updates():
    V = 10
    row = L.counts_set(V, [1, 2, 2, 11, -1], [2, 3, 3, 3, 12])
    assert row.tolist() == [0, 0x8000, 0x8001, 3, 0, 0, 0, 0, 0, 0]
    counts = np.stack([row, row, row])
    counts[0, 4] = L.COUNT_MASK
    counts[0, 5] = L.PROMPT_BIT | (L.COUNT_MASK - 1)
    got = L.counts_add(counts, [[4, 5, 5, 7], [7, 7, -1, -1], [1, 1, 1, 1]], [4, 3, 4], active=[1, 1, 0])
    assert got[0, 4] == L.COUNT_MASK and got[0, 5] == (L.PROMPT_BIT | L.COUNT_MASK) and got[0, 7] == 1    # saturation keeps the prompt bit
    assert got[1, 7] == 2 and np.array_equal(np.delete(got[1], 7), np.delete(row, 7))                       # emitted twice: counted twice
    assert np.array_equal(got[2], row)                                                                       # inactive: unchanged
    assert np.array_equal(L.counts_add(counts, [[4], [4], [4]], [0, 0, 0]), counts)


def test_cli_flags_parse():
    """--repetition-penalty / --presence-penalty / --frequency-penalty / --ban-token ID (repeatable) on both command lines"""
    from src.specdec.run_specdec import parse_args
    from src.specdec_cli.main import build_parser

    flags = ["--repetition-penalty", "1.3", "--presence-penalty", "0.5", "--frequency-penalty", "0.2", "--ban-token", "7", "--ban-token", "9"]
    for a in (parse_args(["--prompt", "1 2 3"] + flags), build_parser().parse_args(["run", "1 2 3"] + flags)):
        assert (a.repetition_penalty, a.presence_penalty, a.frequency_penalty, a.ban_token) == (1.3, 0.5, 0.2, [7, 9])
    a = parse_args(["--prompt", "1 2 3"])
    assert a.repetition_penalty is None and a.presence_penalty is None and a.frequency_penalty is None and a.ban_token is None
