"""The lossy acceptance op (csrc/typical_accept.hip, specdec_hip.ops.typical_accept) against its float64 restatement
(tests/typical_ref.py): accept lengths EQUAL on every planted case (all sit >= 1e-2 from their threshold, asserted on the CPU
by tests/test_typical_ref.py) and on every random row none of whose positions is within 1e-4 of its threshold; the float
records (p_d, H, threshold) within the bound derived from the kernel's summation shape (typical_ref.bounds);
bit-identical across runs and under graph replay; every refusal."""

import math

import numpy as np
import pytest
import torch

import typical_ref as R

pytestmark = pytest.mark.gpu

MARGIN, CAP = 1e-4, 0.02


def _dev(lg, dtype):
    return torch.from_numpy(np.asarray(lg, dtype=np.float32)).to(dtype).cuda()


def _stored(t):
    """what the device tensor holds, as float64"""
    return t.cpu().to(torch.float64).numpy()


def _run(lg_dev, ids, rule, par, **kw):
    from specdec_hip.ops import typical_accept

    acc, stats = typical_accept(lg_dev, torch.as_tensor(np.asarray(ids, dtype=np.int32)).cuda(), rule, temperature=par.get("T", 1.0),
                                epsilon=par.get("eps", 0.09), delta=par.get("delta", None), agree_k=par.get("k", 1), return_stats=True, **kw)
    return acc.cpu().numpy(), stats.cpu().numpy().astype(np.float64)


def _check_stats(got, lg64, ids, rule, par, width, worst):
    """records against float64 within typical_ref.bounds; `worst` collects measured / bound ratios"""
    B, K = np.asarray(ids).shape
    V = lg64.shape[-1]
    T = par.get("T", 1.0)
    for b in range(B):
        for i in range(K):
            d = int(ids[b][i])
            pd, H, rank, (logS, M1, M2) = R.row_stats(lg64[b, i], d, T)
            assert got[b, i, 3] == rank, (b, i)
            if rule != "typical":
                assert got[b, i, 2] == par["k"]
                continue
            if not math.isfinite(H):
                continue
            xd = lg64[b, i, d]
            t_d = (xd - lg64[b, i][lg64[b, i] > -np.inf].max()) / T if xd > -np.inf else 0.0
            _, e_p, e_H, e_thr = R.bounds(V, width, logS, M1, M2, t_d, H)
            thr = R.threshold(H, par.get("eps", 0.09), par.get("delta"))
            # the records are fp32: one more rounding of the stored value
            if pd < 1e-30:      # below what fp32 holds with full precision: the device may flush it to 0
                assert 0.0 <= got[b, i, 0] <= 2e-30, (b, i, got[b, i, 0])
                err_p = 0.0
            else:
                err_p = abs(got[b, i, 0] - pd) / pd
            err_H = abs(got[b, i, 1] - H)
            err_t = abs(got[b, i, 2] - thr) / thr
            worst["p"] = max(worst["p"], err_p / (e_p + R.U))
            worst["H"] = max(worst["H"], err_H / (e_H + R.U * abs(H)))
            worst["thr"] = max(worst["thr"], err_t / (e_thr + R.U))
            worst["abs_p"], worst["abs_H"] = max(worst["abs_p"], err_p), max(worst["abs_H"], err_H)
            assert err_p <= e_p + R.U, (b, i, err_p, e_p)
            assert err_H <= e_H + R.U * abs(H), (b, i, err_H, e_H)
            assert err_t <= e_thr + R.U, (b, i, err_t, e_thr)


def _width(V, dtype):
    """elements per load of the row walker (sample_device.h) on an aligned row: bf16 8, f32 4 when V allows it; f16 is always scalar"""
    if dtype == torch.float32:
        return 4 if V % 4 == 0 else 1
    return 8 if (dtype == torch.bfloat16 and V % 8 == 0) else 1


SHAPES = [(50, 4, torch.bfloat16), (1000, 8, torch.bfloat16), (8200, 4, torch.bfloat16), (8195, 1, torch.bfloat16),
          (8200, 8, torch.float32), (1000, 1, torch.float32), (128256, 4, torch.bfloat16)]


@pytest.mark.parametrize("V,K,dtype", SHAPES, ids=lambda x: str(x).replace("torch.", ""))
def test_planted_cases(V, K, dtype):
    worst = {"p": 0.0, "H": 0.0, "thr": 0.0, "abs_p": 0.0, "abs_H": 0.0}
    cases = R.planted_cases(V, K)
    assert len(cases) >= K + 8
    # B = 3 in one launch where the vocabulary is small: three cases stacked; the real vocabulary runs at B = 1
    group = 1 if V > 10000 else 3
    by_key = {}
    for c in cases:
        by_key.setdefault((c[1], tuple(sorted(c[2].items(), key=str))), []).append(c)
    for (rule, _), cs in by_key.items():
        par = cs[0][2]
        for g in range(0, len(cs), group):
            part = cs[g:g + group]
            lg = np.concatenate([c[3] for c in part])
            ids = np.concatenate([np.asarray(c[4]) for c in part])
            dev = _dev(lg, dtype)
            lg64 = _stored(dev)
            want, _, margins = R.accept(lg64, ids, rule, **par)
            assert want.tolist() == [c[5] for c in part], [c[0] for c in part]
            assert margins.min() >= 1e-2
            acc, stats = _run(dev, ids, rule, par)
            assert acc.tolist() == want.tolist(), [c[0] for c in part]
            _check_stats(stats, lg64, ids, rule, par, _width(V, dtype), worst)
    print(f"[typical op] planted V={V} K={K} {dtype}: measured / bound  p {worst['p']:.3f}  H {worst['H']:.3f}  thr {worst['thr']:.3f}; "
          f"worst rel p {worst['abs_p']:.3e}  worst abs H {worst['abs_H']:.3e}")


@pytest.mark.parametrize("B,K,V,dtype", [(3, 8, 1000, torch.bfloat16), (3, 4, 8200, torch.bfloat16), (1, 8, 8195, torch.bfloat16),
                                         (3, 4, 50, torch.float32), (3, 1, 8200, torch.float16)], ids=lambda x: str(x).replace("torch.", ""))
def test_random_rows(B, K, V, dtype):
    worst = {"p": 0.0, "H": 0.0, "thr": 0.0, "abs_p": 0.0, "abs_H": 0.0}
    lg, ids = R.random_case(B, K, V, seed=B * 1000 + K)
    dev = _dev(lg, dtype)
    lg64 = _stored(dev)
    under = total = 0
    for rule, par in (("typical", {"T": 0.7, "eps": 0.09, "delta": 0.3}), ("typical", {"T": 1.0, "eps": 0.2, "delta": None}),
                      ("topk_agree", {"k": 1}), ("topk_agree", {"k": 3})):
        want, _, margins = R.accept(lg64, ids, rule, **par)
        acc, stats = _run(dev, ids, rule, par)
        under += int((margins < MARGIN).sum())        # positions within 1e-4 of their threshold: their rows are not compared
        total += margins.size
        for b in range(B):
            if margins[b].min() >= MARGIN:
                assert acc[b] == want[b], (rule, par, b)
        _check_stats(stats, lg64, ids, rule, par, _width(V, dtype), worst)
    assert under <= CAP * total, (under, total)
    print(f"[typical op] random B={B} K={K} V={V} {dtype}: positions under the margin {under}/{total}; measured / bound  p {worst['p']:.3f}  H {worst['H']:.3f}  "
          f"thr {worst['thr']:.3f}; worst rel p {worst['abs_p']:.3e}  worst abs H {worst['abs_H']:.3e}")


def test_misaligned_row_stride_takes_the_scalar_path():
    """rows 8200 apart would be aligned; a view into rows 8203 elements apart starts every other row off 16 bytes"""
    B, K, V, pad = 3, 4, 8200, 3
    lg, ids = R.random_case(B, K, V, seed=5)
    wide = torch.zeros((B, K + 1, V + pad), dtype=torch.bfloat16, device="cuda")
    wide[:, :, :V] = _dev(lg, torch.bfloat16)
    view = wide[:, :, :V]
    assert view.stride(1) == V + pad and view.stride(0) == (K + 1) * (V + pad)
    par = {"T": 0.7, "eps": 0.09, "delta": 0.3}
    a_view, s_view = _run(view, ids, "typical", par)
    a_ref, s_ref = _run(view.contiguous(), ids, "typical", par)
    want, _, margins = R.accept(_stored(view), ids, "typical", **par)
    keep = margins.min(axis=1) >= MARGIN
    assert (a_view[keep] == want[keep]).all() and (a_ref[keep] == want[keep]).all()
    worst = {"p": 0.0, "H": 0.0, "thr": 0.0, "abs_p": 0.0, "abs_H": 0.0}
    _check_stats(s_view, _stored(view), ids, "typical", par, 8, worst)       # (rows that happen to be aligned take the 16-byte walk: the larger bound)
    assert (s_view[..., 3] == s_ref[..., 3]).all()


def test_bit_identical_across_runs_and_under_graph_replay():
    from specdec_hip.ops import typical_accept, typical_accept_workspace

    B, K, V = 3, 4, 8200
    lg, ids = R.random_case(B, K, V, seed=9)
    dev, ids_d = _dev(lg, torch.bfloat16), torch.from_numpy(ids).cuda()
    kw = dict(rule="typical", temperature=0.7, epsilon=0.09, delta=0.3)
    a1, s1 = typical_accept(dev, ids_d, return_stats=True, **kw)
    a2, s2 = typical_accept(dev, ids_d, return_stats=True, **kw)
    assert torch.equal(a1, a2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    out = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    stats = torch.zeros((B, K, 4), dtype=torch.float32, device="cuda")
    ws = typical_accept_workspace(B, K, V, "cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        typical_accept(dev, ids_d, out=out, stats_out=stats, workspace=ws, **kw)      # warm-up outside the capture
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    out.fill_(-7)
    with torch.cuda.graph(g, stream=st):
        typical_accept(dev, ids_d, out=out, stats_out=stats, workspace=ws, **kw)
    for _ in range(2):
        out.fill_(-7)
        stats.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a1) and torch.equal(stats.view(torch.int32), s1.view(torch.int32))


def test_every_refusal_fires():
    from specdec_hip import _abi
    from specdec_hip.ops import typical_accept

    B, K, V = 2, 3, 64
    lg = torch.zeros((B, K + 1, V), dtype=torch.bfloat16, device="cuda")
    ids = torch.zeros((B, K), dtype=torch.int32, device="cuda")
    lib = _abi.load()
    ws = torch.empty(lib.sd_typical_accept_workspace(B, K, V), dtype=torch.uint8, device="cuda")
    out = torch.zeros(B, dtype=torch.int32, device="cuda")

    def raw(logits=lg.data_ptr(), dt=_abi.SD_BF16, stride=V, d=ids.data_ptr(), K_=K, V_=V, rule=1, T=1.0, eps=0.09, delta=0.3, k=1,
            acc=out.data_ptr(), ws_p=ws.data_ptr(), ws_n=ws.numel()):
        rc = lib.sd_typical_accept(logits, dt, stride, d, B, K_, V_, rule, T, eps, delta, k, acc, None, ws_p, ws_n, None)
        return rc, _abi.last_error()

    assert raw()[0] == 0
    for kw, word in (({"rule": 0}, "rule"), ({"rule": 3}, "rule"), ({"T": 0.0}, "temperature"), ({"T": -1.0}, "temperature"),
                     ({"T": float("nan")}, "temperature"), ({"eps": 0.0}, "epsilon"), ({"eps": 1.5}, "epsilon"), ({"eps": float("nan")}, "epsilon"),
                     ({"delta": 0.0}, "delta"), ({"delta": -2.0}, "delta"), ({"delta": float("nan")}, "delta"),
                     ({"rule": 2, "k": 0}, "agree_k"), ({"rule": 2, "k": V + 1}, "agree_k"), ({"K_": 0}, "K="), ({"K_": 64}, "K="),
                     ({"logits": None}, "NULL"), ({"d": None}, "NULL"), ({"acc": None}, "NULL"), ({"ws_p": None}, "NULL"),
                     ({"ws_n": 8}, "workspace"), ({"stride": V - 1}, "row_stride"), ({"dt": _abi.SD_I32}, "dtype")):
        rc, msg = raw(**kw)
        assert rc != 0 and word in msg, (kw, msg)
    assert raw(delta=float("inf"))[0] == 0 and raw(eps=1.0)[0] == 0 and raw(rule=2, k=V)[0] == 0
    with pytest.raises(ValueError, match="rule"):
        typical_accept(lg, ids, "conf_threshold")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        typical_accept(lg.cpu(), ids.cpu())
    torch.cuda.synchronize()
