"""Token automata on the device (csrc/grammar.hip and the grammar line of csrc/logit_proc.hip) against their CPU restatement
(tests/grammar_ref.py): the mask builder, the stand-alone op, the advance, and the refusals of the C level.

Everything compared here is an integer or a bf16 word and must be EQUAL: the mask is a bit test on top of a fixed sequence of
correctly rounded float32 operations, so there is no tolerance to derive."""

import numpy as np
import pytest
import torch

import grammar_ref as G
import logit_proc_ref as L
from helpers import synthetic_prompts, tiny_pair
from test_hip_logit_proc_gpu import _bf16_tensor, _bits_of, _counts_tensor
from test_hip_spec_sample_gpu import _pipe

pytestmark = pytest.mark.gpu


def _table(S, V, seed, p_allow=0.4):
    rng = np.random.default_rng(seed)
    nxt = rng.integers(0, S, (S, V)).astype(np.uint16)
    nxt[rng.random((S, V)) >= p_allow] = G.NONE
    return nxt


def _dev_table(nxt):
    return torch.from_numpy(np.ascontiguousarray(nxt).view(np.int16)).cuda()


@pytest.mark.parametrize("V", [31, 1000, 1003, 8200])
@pytest.mark.parametrize("S", [1, 3, 70])
def test_build_masks_equals_restatement(S, V):
    from specdec_hip.ops import fsm_build_masks

    nxt = _table(S, V, 7 * S + V)
    nxt[S - 1, V - 1] = 0                      # the last entry of the table is allowed: the bit next to the pad bits
    nxt[0, 0] = G.NONE
    got = fsm_build_masks(_dev_table(nxt)).cpu().numpy().view(np.uint32)
    want = G.build_masks(nxt)
    assert got.shape == want.shape == (S, (V + 31) // 32)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    if V % 32:
        assert (got[:, -1] >> np.uint32(V % 32) == 0).all(), "pad bits"
    assert 0 < int(np.unpackbits(got.view(np.uint8)).sum()) == int((nxt != G.NONE).sum())


def _fsm_case(V, K, seed):
    """B = 3 rows of R = K + 1 positions over a 6-state automaton. Row 0 follows allowed tokens from state 2; row 1 is
    unconstrained (-1); row 2 starts in state 4 and its first in-step token is not allowed there, so its rows r >= 1 are DEAD.
    Row (0, 0) holds a NaN at an allowed and at a disallowed id, and -inf under a +inf bias at another disallowed id."""
    B, R, S = 3, K + 1, 6
    rng = np.random.default_rng(seed)
    nxt = _table(S, V, seed + 1)
    eos = V - 2
    nxt[:, eos] = G.NONE
    nxt[1, eos] = 5
    state = np.array([2, -1, 4], dtype=np.int32)
    toks = np.zeros((B, max(K, 1)), dtype=np.int32)
    s = 2
    for j in range(K):
        toks[0, j] = rng.choice(np.flatnonzero(nxt[s] != G.NONE))
        s = int(nxt[s, toks[0, j]])
    toks[1] = rng.integers(0, V, K)
    toks[2] = rng.integers(0, V, K)
    toks[2, 0] = np.flatnonzero(nxt[4] == G.NONE)[0]
    x = rng.normal(0, 3.0, (B, R, V)).astype(np.float32)
    ok0, no0 = np.flatnonzero(nxt[2] != G.NONE), np.flatnonzero(nxt[2] == G.NONE)
    nan_ok, nan_no, inf_no = int(ok0[3]), int(no0[3]), int(no0[5])
    x[0, 0, nan_ok] = np.nan
    x[0, 0, nan_no] = np.nan
    x[0, 0, inf_no] = -np.inf
    x[1, R - 1, 500] = np.nan                  # the unconstrained row keeps its NaN
    bits = _bits_of(torch.from_numpy(x).to(torch.bfloat16))
    counts = np.zeros((B, V), np.uint16)
    idx = rng.permutation(V)
    counts[:, idx[:200]] = L.PROMPT_BIT
    counts[:, idx[200:400]] = 1
    counts[:, idx[400:450]] = L.PROMPT_BIT | 3
    bias = rng.normal(0, 1.0, (B, V)).astype(np.float32)
    bias[:, idx[500:560]] = -np.inf
    bias[:, eos] = 0.5                         # (eos keeps a finite value in the DEAD rows)
    bias[0, inf_no] = np.inf                   # -inf + +inf = NaN before the mask; -inf after it
    return nxt, eos, state, toks, bits, counts, bias, (nan_ok, nan_no, inf_no)


@pytest.mark.parametrize("V", [1000, 1003, 8200])
@pytest.mark.parametrize("K", [1, 4])
def test_process_fsm_is_bit_equal_to_restatement(V, K):
    from specdec_hip.ops import fsm_build_masks, logit_process, logit_process_fsm

    nxt, eos, state, toks, bits, counts, bias, (nan_ok, nan_no, inf_no) = _fsm_case(V, K, 10 * K + (V & 7))
    d_nxt = _dev_table(nxt)
    d_allow = fsm_build_masks(d_nxt)
    d_state = torch.from_numpy(state).cuda()
    d_toks = torch.from_numpy(toks).cuda()
    rp, pres, freq = 1.3, 0.5, 0.2
    for use_bias in (False, True):
        b_np = bias if use_bias else None
        d_bias = torch.from_numpy(bias).cuda() if use_bias else None
        want, want_ids = G.process_rows_fsm(bits, counts, nxt, state, eos, toks, None, rp, pres, freq, b_np)
        rows = _bf16_tensor(bits).cuda()
        ids = logit_process_fsm(rows, _counts_tensor(counts), d_nxt, d_allow, d_state, eos, rp, pres, freq, bias=d_bias, tokens=d_toks,
                                return_ids=True)
        got = _bits_of(rows)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (V, K, use_bias, bad[:5], [hex(got[tuple(i)]) for i in bad[:5]], [hex(want[tuple(i)]) for i in bad[:5]])
        assert ids.cpu().tolist() == want_ids.tolist(), (V, K, use_bias)
        # the row at -1 is what sd_logit_process makes of it
        plain = _bf16_tensor(bits).cuda()
        plain_ids = logit_process(plain, _counts_tensor(counts), rp, pres, freq, bias=d_bias, tokens=d_toks, return_ids=True)
        assert np.array_equal(got[1], _bits_of(plain)[1]) and ids[1].tolist() == plain_ids[1].tolist()
        # the cases the issue names are really in the data
        assert want[0, 0, nan_ok] == L.NAN_BF16 and want[0, 0, nan_no] == G.NEG_INF_BF16 and want_ids[0, 0] == nan_ok
        assert want[0, 0, inf_no] == G.NEG_INF_BF16
        if use_bias:
            assert np.isnan(L.bf16_to_f32(_bits_of(plain))[0, 0, inf_no]), "without the mask the +inf bias gives a NaN there"
        assert G.walk(nxt, state[0], toks[0][:K]) < nxt.shape[0] and G.walk(nxt, state[2], toks[2][:1]) == G.DEAD
        dead = want[2, 1:]
        assert (np.delete(dead, eos, axis=1) == G.NEG_INF_BF16).all() and (dead[:, eos] != G.NEG_INF_BF16).all()
        assert want_ids[2, 1:].tolist() == [eos] * K
        # the fixed-n_tokens form on a strided view: row 1 of a [B][2][V] buffer, every row conditioned on the first n tokens
        n = min(2, K)
        buf = torch.stack([_bf16_tensor(bits[:, 0]), _bf16_tensor(bits[:, K])], 1).cuda()
        before = _bits_of(buf)
        ids1 = logit_process_fsm(buf[:, 1:2, :], _counts_tensor(counts), d_nxt, d_allow, d_state, eos, rp, pres, freq, bias=d_bias,
                                 tokens=d_toks, n_tokens=n, return_ids=True)
        want1, want_ids1 = G.process_rows_fsm(before[:, 1:2], counts, nxt, state, eos, toks, n, rp, pres, freq, b_np)
        after = _bits_of(buf)
        assert np.array_equal(after[:, 0], before[:, 0]), "the rows between the processed ones were written"
        assert np.array_equal(after[:, 1:2], want1) and ids1.cpu().tolist() == want_ids1.tolist()


def test_process_fsm_inactive_rows_and_states_beyond_the_table():
    """an inactive row is not written; a state >= S (and 0xFFFF) reads as DEAD; identity parameters mask and nothing else"""
    from specdec_hip.ops import fsm_build_masks, logit_counts, logit_process_fsm

    V, K = 1003, 2
    nxt, eos, _, toks, bits, counts, _, _ = _fsm_case(V, K, 99)
    state = np.array([6, 0xFFFF, 3], dtype=np.int32)
    active = [1, 1, 0]
    d_nxt = _dev_table(nxt)
    rows = _bf16_tensor(bits).cuda()
    ids = logit_process_fsm(rows, logit_counts(3, V, "cuda"), d_nxt, fsm_build_masks(d_nxt), torch.from_numpy(state).cuda(), eos,
                            tokens=torch.from_numpy(toks).cuda(), active=torch.tensor(active, dtype=torch.int32, device="cuda"),
                            return_ids=True)
    want, want_ids = G.process_rows_fsm(bits, np.zeros((3, V), np.uint16), nxt, state, eos, toks, None, active=active)
    got = _bits_of(rows)
    assert np.array_equal(got, want) and ids.cpu().tolist() == want_ids.tolist()
    assert np.array_equal(got[2], bits[2]) and want_ids[0].tolist() == [eos] * 3 and want_ids[1].tolist() == [eos] * 3


def test_advance_equals_restatement():
    from specdec_hip.ops import fsm_advance

    S, V = 6, 1003
    nxt = _table(S, V, 21)
    ok = lambda s: int(np.flatnonzero(nxt[s] != G.NONE)[2])  # noqa: E731
    no = lambda s: int(np.flatnonzero(nxt[s] == G.NONE)[2])  # noqa: E731
    t0 = [ok(0)]
    t0.append(ok(int(nxt[0, t0[0]])))
    state = np.array([0, 1, 2, -1, 3, 0xFFFF, 4, 5, 70], dtype=np.int32)
    toks = np.full((len(state), 3), -1, dtype=np.int32)
    toks[0, :2] = t0                           # two allowed tokens
    toks[1] = [ok(1), ok(1), ok(1)]            # n_new = 0: untouched
    toks[2] = [ok(2), ok(2), ok(2)]            # an inactive row
    toks[3] = [5, 6, 7]                        # an unconstrained row
    toks[4] = [V + 3, ok(3), ok(3)]            # an id outside the vocabulary -> DEAD
    toks[5] = [ok(0), ok(0), ok(0)]            # DEAD stays DEAD
    toks[6] = [no(4), ok(4), ok(4)]            # a token the state does not allow -> DEAD, and stays
    toks[7] = [ok(5), -1, -1]                  # a -1 padding inside n_new -> DEAD
    toks[8] = [ok(0), ok(0), ok(0)]            # a state beyond the table is DEAD
    n_new = [2, 0, 3, 3, 3, 3, 3, 2, 1]
    active = [1, 1, 0, 1, 1, 1, 1, 1, 1]
    dev = torch.from_numpy(state.copy()).cuda()
    fsm_advance(_dev_table(nxt), dev, torch.from_numpy(toks).cuda(), torch.tensor(n_new, dtype=torch.int32, device="cuda"),
                torch.tensor(active, dtype=torch.int32, device="cuda"))
    want = G.advance(nxt, state, toks, n_new, active)
    assert dev.cpu().tolist() == want.tolist()
    assert want.tolist()[1:] == [1, 2, -1, G.DEAD, G.DEAD, G.DEAD, G.DEAD, G.DEAD] and 0 <= want[0] < S
    dev2 = torch.from_numpy(state.copy()).cuda()
    fsm_advance(_dev_table(nxt), dev2, torch.from_numpy(toks).cuda(), torch.tensor(n_new, dtype=torch.int32, device="cuda"))
    assert dev2.cpu().tolist() == G.advance(nxt, state, toks, n_new).tolist()


def test_refusals_at_the_c_level():
    from specdec_hip import _abi
    from specdec_hip.engine import HipSpecDec
    from specdec_hip.ops import fsm_build_masks, logit_counts

    lib = _abi.load()
    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(2, 12, tgt.config.vocab).tolist()
    pipe = _pipe(drf, tgt)
    sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
    loop = sess.loop
    loop.sync()
    V, B, K = loop.target.cfg.vocab, loop.B, loop.K
    S = 3
    nxt = _dev_table(_table(S, V, 1))
    allow = fsm_build_masks(nxt)
    state = torch.full((B,), -1, dtype=torch.int32, device="cuda")

    def bind(handle=None, n=nxt.data_ptr(), a=allow.data_ptr(), s=S, st=state.data_ptr(), eos=V - 1):
        return lib.sd_specdec_set_grammar(loop.handle if handle is None else handle, 1, n, a, s, st, eos)

    assert bind() != 0 and "stage is off" in _abi.last_error()
    loop.set_logit_processors(True)
    for kw, word in (({"s": 0}, "states"), ({"s": 65535}, "states"), ({"eos": V}, "eos_id"), ({"eos": -1}, "eos_id"), ({"n": None}, "NULL"),
                     ({"a": None}, "NULL"), ({"st": None}, "NULL"), ({"n": nxt.data_ptr() + 2}, "aligned"),
                     ({"a": allow.data_ptr() + 4}, "aligned")):
        assert bind(**kw) != 0, kw
        assert word in _abi.last_error(), (kw, _abi.last_error())
    assert bind() == 0
    with pytest.raises(_abi.HipLibraryError, match="keep a fixed K"):
        loop.set_adaptive(True, initial_k=2, min_k=1, max_k=K)
    assert lib.sd_specdec_set_grammar(loop.handle, 0, None, None, 0, None, 0) == 0
    loop.set_logit_processors(False)
    loop.set_adaptive(True, initial_k=2, min_k=1, max_k=K)
    assert bind() != 0 and "adaptive K" in _abi.last_error()
    loop.set_adaptive(False)
    sess.finish()
    selfd = HipSpecDec(None, loop.target, B, K)                      # self-draft (and with it Medusa heads and EAGLE)
    assert bind(handle=selfd.handle) != 0 and "draft model" in _abi.last_error()
    selfd.close()
    # the ops
    rows = torch.zeros((1, 1, V), dtype=torch.bfloat16, device="cuda")
    c1 = logit_counts(1, V, "cuda")
    st1 = torch.zeros(1, dtype=torch.int32, device="cuda")

    def op(n=nxt.data_ptr(), a=allow.data_ptr(), s=S, st=st1.data_ptr(), eos=0):
        return lib.sd_logit_process_fsm(rows.data_ptr(), V, 1, 1, V, c1.data_ptr(), None, None, 0, 0, None, 1.0, 0.0, 0.0, None, 0, None, 0,
                                        n, a, s, st, eos, None)

    for kw, word in (({"s": 0}, "states"), ({"s": 65535}, "states"), ({"eos": V}, "eos_id"), ({"n": None}, "NULL"), ({"st": None}, "NULL"),
                     ({"a": allow.data_ptr() + 8}, "aligned")):
        assert op(**kw) != 0, kw
        assert word in _abi.last_error(), (kw, _abi.last_error())
    assert op() == 0
    torch.cuda.synchronize()
    need = lib.sd_fsm_mask_bytes(S, V)
    assert need == (S * ((V + 31) // 32) * 4 + 15) // 16 * 16
    for args, word in (((nxt.data_ptr(), S, V, allow.data_ptr(), need - 16), "mask table"), ((nxt.data_ptr(), 0, V, allow.data_ptr(), need), "S="),
                       ((None, S, V, allow.data_ptr(), need), "NULL"), ((nxt.data_ptr() + 2, S, V, allow.data_ptr(), need), "aligned")):
        assert lib.sd_fsm_build_masks(*args, None) != 0, args
        assert word in _abi.last_error(), (args, _abi.last_error())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fsm_build_masks(nxt.cpu())
