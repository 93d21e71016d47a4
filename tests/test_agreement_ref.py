"""The draft-target agreement definition on the CPU (tests/agreement_ref.py, the restatement of csrc/spec_agree.hip): its
properties, its link to the speculative-sampling step merged before it (tests/spec_sample_ref.py), the windowed
expected-tokens formula, and the refusals of the C entry that need no device."""

import ctypes
import math

import numpy as np
import pytest
import torch

import agreement_ref as A
import spec_sample_ref as R


def _bf16(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def _pairs():
    """random and adversarial finite row pairs (p, q, T)"""
    rng = np.random.default_rng(7)
    out = []
    for V, T in ((1, 1.0), (2, 0.7), (40, 1.0), (257, 2.5), (4099, 0.7)):
        p = _bf16(rng.normal(0, 3.0, V))
        out.append((p, _bf16(p + rng.normal(0, 0.5, V)), T))
        out.append((p, _bf16(rng.normal(0, 3.0, V)), T))
    p = _bf16(np.linspace(-60, 60, 300))                      # wide dynamic range: most probabilities underflow next to the top
    out.append((p, p[::-1].copy(), 1.0))
    out.append((_bf16(np.zeros(64)), _bf16(np.r_[30.0, np.zeros(63)]), 1.0))      # uniform against a spike
    out.append((_bf16(np.r_[5.0, 5.0, np.zeros(30)]), _bf16(np.r_[5.0, 5.0, np.zeros(30)] * 0.5), 0.7))   # tied maxima
    p = _bf16(rng.normal(0, 3.0, 50))
    p[::3] = -np.inf                                           # -inf entries on the target's side only: kl stays finite
    out.append((p, _bf16(rng.normal(0, 3.0, 50)), 1.0))
    return out


def test_alpha_is_a_probability_symmetric_and_one_minus_tv():
    for p, q, T in _pairs():
        r, s = A.agreement_row(p, q, T), A.agreement_row(q, p, T)
        b_alpha, _ = A.bounds(p, q, T)
        assert 0.0 <= r.alpha <= 1.0 + b_alpha
        assert r.alpha == s.alpha                              # min is symmetric term by term: the same sum
        assert abs(r.alpha - A.tv_alpha(p, q, T)) <= b_alpha
        assert (r.p_arg, r.q_arg) == (s.q_arg, s.p_arg) and r.agree == (r.p_arg == r.q_arg)


def test_kl_is_nonnegative_and_zero_on_equal_rows():
    for p, q, T in _pairs():
        b_alpha, b_kl = A.bounds(p, q, T)
        assert A.agreement_row(p, q, T).kl >= -b_kl
        same = A.agreement_row(p, p.copy(), T)
        assert same.kl == 0.0
        assert abs(same.alpha - 1.0) <= A.bounds(p, p, T)[0] and same.agree


def test_disjoint_supports_and_the_non_finite_rules():
    inf = np.inf
    p = _bf16(np.r_[1.0, 2.0, -inf, -inf])
    q = _bf16(np.r_[-inf, -inf, 0.5, 3.0])
    r = A.agreement_row(p, q, 1.0)
    assert r.alpha == 0.0 and r.kl == inf and (r.p_arg, r.q_arg, r.agree) == (1, 3, False)
    # -inf entries in q only, overlapping supports: alpha counts the overlap, kl is +inf
    r = A.agreement_row(_bf16(np.r_[0.0, 0.0]), _bf16(np.r_[0.0, -inf]), 1.0)
    assert r.alpha == 0.5 and r.kl == inf and r.agree
    # a NaN, +inf on top, all -inf: alpha = kl = NaN; the argmax follows NaN first, then value, then index
    fin = _bf16(np.r_[0.0, 1.0, 0.5])
    for bad, arg in ((np.r_[0.0, np.nan, 5.0], 1), (np.r_[0.0, inf, inf], 1), (np.r_[-inf, -inf, -inf], 0)):
        for r, pa, qa in ((A.agreement_row(_bf16(bad), fin, 1.0), arg, 1), (A.agreement_row(fin, _bf16(bad), 0.7), 1, arg)):
            assert math.isnan(r.alpha) and math.isnan(r.kl) and (r.p_arg, r.q_arg) == (pa, qa) and r.agree == (pa == qa)
    # tied maxima: the lower index; rows whose argmaxes differ by index only do not agree
    r = A.agreement_row(_bf16(np.r_[1.0, 3.0, 3.0]), _bf16(np.r_[1.0, 2.0, 3.0]), 1.0)
    assert (r.p_arg, r.q_arg, r.agree) == (1, 2, False)


def _pair_for(alpha_target):
    """a fixed V = 40 pair whose alpha is near the target"""
    seed, noise = {0.2: (21, 9.0), 0.6: (12, 1.1), 0.95: (13, 0.12)}[alpha_target]
    rng = np.random.default_rng(seed)
    p = _bf16(rng.normal(0, 2.0, 40))
    return p, _bf16(p + rng.normal(0, noise, 40))


@pytest.mark.parametrize("alpha_target", [0.2, 0.6, 0.95])
def test_alpha_is_the_accept_frequency_of_the_restated_sampling_step(alpha_target):
    """The link to csrc/spec_sample.hip: at K = 1 the restated unshaped step (the draft draws d from q, the target accepts it
    with probability min(1, p(d)/q(d))) accepts with probability sum_v q(v) min(1, p(v)/q(v)) = sum_v min(p(v), q(v)) = alpha.
    Over N seeded Philox counters the accept frequency must lie within 5 binomial standard deviations of alpha."""
    p, q = _pair_for(alpha_target)
    T, N, seed = 1.0, 1200, 20240611
    alpha = A.agreement_row(p, q, T).alpha
    assert abs(alpha - alpha_target) < 0.08, alpha             # the pair is what the case says it is
    p_rows, q_rows = np.stack([p, p]), q[None]
    accepted = 0
    for i in range(N):                                         # a step at K = 1 consumes counters c and c + 1
        _, res, _, _ = R.spec_step_ref(q_rows, p_rows, T, seed, 2 * i, 0)
        accepted += res.accept_len
    sigma = math.sqrt(alpha * (1.0 - alpha) / N)
    print(f"alpha {alpha:.4f} accept frequency {accepted / N:.4f} ({(accepted / N - alpha) / sigma:+.2f} sigma, N = {N})")
    assert abs(accepted / N - alpha) <= 5.0 * sigma


def test_expected_tokens_per_step_against_a_direct_loop():
    from src.specdec.core.pipeline import expected_tokens_per_step

    rng = np.random.default_rng(3)
    for n in (1, 3, 8, 25):
        alpha = rng.uniform(0, 1, n).tolist()
        got = expected_tokens_per_step(alpha)
        assert sorted(got) == list(range(1, 9))
        for K in range(1, 9):
            want = A.expected_tokens_loop(alpha, K)
            assert (got[K] is None and want is None) if n < K else got[K] == pytest.approx(want, rel=1e-12)
    assert expected_tokens_per_step([1.0] * 10)[4] == 5.0 and expected_tokens_per_step([0.0] * 10)[4] == 1.0
    assert expected_tokens_per_step([True, False, True], k_max=2) == {1: pytest.approx(1 + 2 / 3), 2: pytest.approx(1 + 0.5 + 0.0)}


def test_entry_points_are_bound_and_refuse_without_a_device():
    from specdec_hip import _abi

    lib = _abi.load()
    for name in ("sd_spec_agreement", "sd_spec_agreement_workspace", "sd_model_score_logits"):
        assert name in _abi.SIGNATURES and hasattr(lib, name)
    assert lib.sd_spec_agreement_workspace(0, 100) == 0 and lib.sd_spec_agreement_workspace(4, 0) == 0
    one = lib.sd_spec_agreement_workspace(1, 128256)
    assert one >= 32 * 16 and lib.sd_spec_agreement_workspace(7, 128256) == 7 * one       # slices depend on V only
    assert lib.sd_spec_agreement_workspace(1, 100) < lib.sd_spec_agreement_workspace(1, 4099)
    buf = ctypes.c_void_p(64)
    call = lambda q=buf, ld_q=100, p=buf, ld_p=100, n=2, V=100, T=1.0, ws=buf, ws_bytes=1 << 20: lib.sd_spec_agreement(  # noqa: E731
        q, ld_q, p, ld_p, n, V, T, None, None, None, None, None, ws, ws_bytes, None)
    for kwargs, word in (({"q": None}, "NULL"), ({"p": None}, "NULL"), ({"n": 0}, "n=0"), ({"V": 0}, "V=0"), ({"ld_q": 99}, "stride"),
                         ({"ld_p": 1}, "stride"), ({"T": 0.0}, "temperature"), ({"T": -1.0}, "temperature"),
                         ({"T": float("nan")}, "temperature"), ({"ws_bytes": 8}, "workspace"), ({"ws": None}, "workspace")):
        assert call(**kwargs) != 0 and word in _abi.last_error(), (kwargs, _abi.last_error())
    assert lib.sd_model_score_logits(None, buf, 4, 0, 0, buf, None, None) != 0 and "NULL model" in _abi.last_error()
    assert lib.sd_model_score_logits(None, buf, 4, 0, 0, None, None, None) != 0 and "NULL logits" in _abi.last_error()


def test_python_surface_refuses_before_device_work():
    from specdec_hip import ops
    from src.specdec.run_specdec import parse_args

    with pytest.raises(RuntimeError, match="device tensors"):
        ops.spec_agreement(torch.zeros(2, 8, dtype=torch.bfloat16), torch.zeros(2, 8, dtype=torch.bfloat16))
    assert parse_args(["--prompt", "1 2", "--eval-agreement"]).eval_agreement
    assert not parse_args(["--prompt", "1 2"]).eval_agreement
    import src.kernels as sk

    assert "spec_agreement" in sk.get_kernel_info()
