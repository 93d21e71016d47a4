"""The log-prob op (csrc/token_logprobs.hip, specdec_hip.ops.token_logprobs) against its float64 restatement
(tests/logprobs_ref.py): rank and the top ids EQUAL in every case (both order the same stored values: no margin, nothing skipped),
log-probs within the bound derived from the kernel's summation shape (logprobs_ref.bounds); planted rows for every edge the op
defines; bit-identical across runs and under graph replay; every refusal."""

import functools

import numpy as np
import pytest
import torch

import logprobs_ref as R

pytestmark = pytest.mark.gpu

NEG = float("-inf")
BF16_MAX = 3.3895313892515355e38   # 0x7f7f


def _width(V, dtype, aligned=True):
    """elements per load of the row walker (sample_device.h): bf16 8, f32 4 on a 16-byte aligned row when V allows it, else 1"""
    if not aligned:
        return 1
    if dtype == torch.float32:
        return 4 if V % 4 == 0 else 1
    return 8 if (dtype == torch.bfloat16 and V % 8 == 0) else 1


def _stored(t):
    return t.cpu().to(torch.float64).numpy()


def _run(dev, ids, top_n, **kw):
    from specdec_hip.ops import token_logprobs

    out = token_logprobs(dev, ids, top_n, **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _check(dev, ids, top_n, width, worst):
    lp, rank, tid, tlp = _run(dev, ids, top_n)
    x = _stored(dev)
    N = min(top_n, x.shape[1])
    assert tid.shape == (x.shape[0], N) and tlp.shape == (x.shape[0], N)
    for r in range(x.shape[0]):
        R.check_row(x[r], int(ids[r]), top_n, width, (lp[r], rank[r], tid[r], tlp[r]), worst)


@functools.lru_cache(maxsize=None)
def _random_rows(Rn, V, dtype):
    """seeded rows (normal * 3, one in a hundred at -inf) on the device, and a token per row: the argmax, index 0, V - 1, then random"""
    rng = np.random.default_rng(1000 * Rn + V)
    lg = rng.standard_normal((Rn, V)).astype(np.float32) * 3.0
    lg[rng.random((Rn, V)) < 0.01] = NEG
    dev = torch.from_numpy(lg).to(dtype).cuda()
    x = _stored(dev)
    ids = [int(rng.integers(0, V)) for _ in range(Rn)]
    ids[0] = int(np.argmax(x[0]))
    if Rn > 2:
        ids[1], ids[2] = 0, V - 1
    return dev, ids


SHAPES = [(1, 17, torch.bfloat16), (5, 50, torch.bfloat16), (9, 1000, torch.bfloat16), (5, 8195, torch.bfloat16),
          (27, 8200, torch.bfloat16), (5, 8200, torch.float32), (5, 128256, torch.bfloat16)]


@pytest.mark.parametrize("top_n", [0, 1, 5, 20])
@pytest.mark.parametrize("Rn,V,dtype", SHAPES, ids=lambda x: str(x).replace("torch.", ""))
def test_random_rows(Rn, V, dtype, top_n):
    dev, ids = _random_rows(Rn, V, dtype)
    worst = {}
    _check(dev, ids, top_n, _width(V, dtype), worst)
    print(f"[logprobs op] R={Rn} V={V} {dtype} top_n={top_n}: measured / bound {worst.get('ratio', 0.0):.3f}  "
          f"worst abs error {worst.get('abs', 0.0):.3e}")


def _planted(V, N):
    """[(name, row float64 [V], token)] — every edge the op defines; values are exact in bf16"""
    rng = np.random.default_rng(V)
    base = np.round(rng.standard_normal(V) * 2.0 * 8) / 8        # multiples of 1/8 in about +-8: exact in bf16
    rows = []
    x = base.copy(); x[V // 3] = 12.0
    rows.append(("token is the argmax", x, V // 3))
    x = base.copy(); x[5] = NEG
    rows.append(("token at -inf", x, 5))
    x = np.full(V, NEG); x[V - 2] = 1.5
    rows.append(("all but one at -inf", x, V - 2))
    rows.append(("all but one at -inf, token at -inf", x.copy(), 3))
    rows.append(("whole row equal", np.full(V, -0.75), V // 2))
    rows.append(("whole row -inf", np.full(V, NEG), 1))
    x = np.full(V, -4.0); x[[2, 9, 11, 20][:N - 1]] = [9.0, 8.0, 7.0, 6.0][:N - 1]; x[[30, 31, 40]] = 5.0   # places N, N+1, N+2 share a value
    rows.append(("tie straddling place N", x, 31))
    x = np.full(V, -3.0); x[[1, 24, 25, 26, V - 1]] = 2.0; x[0] = 5.0
    rows.append(("token tied with lower and higher indices", x, 25))
    x = base.copy(); x[3] = BF16_MAX; x[7] = -BF16_MAX
    rows.append(("bf16 max-finite, token ordinary", x, 10))
    rows.append(("bf16 max-finite, token the minimum", x.copy(), 7))
    rows.append(("bf16 max-finite, token the maximum", x.copy(), 3))
    rows.append(("token at index 0", base.copy(), 0))
    rows.append(("token at index V - 1", base.copy(), V - 1))
    return rows


@pytest.mark.parametrize("V", [50, 8200])
def test_planted_rows(V):
    N = 5
    rows = _planted(V, N)
    lg = np.stack([r[1] for r in rows])
    ids = [r[2] for r in rows]
    dev = torch.from_numpy(lg.astype(np.float32)).to(torch.bfloat16).cuda()
    assert (_stored(dev) == lg).all()                     # the planted values are what the device holds
    worst = {}
    _check(dev, ids, N, _width(V, torch.bfloat16), worst)
    # the definitions, stated once more on the device's own numbers
    lp, rank, tid, tlp = _run(dev, ids, N)
    by = {r[0]: k for k, r in enumerate(rows)}
    k = by["token is the argmax"]
    assert rank[k] == 0 and tid[k, 0] == ids[k] and tlp[k, 0] == lp[k]
    assert lp[by["token at -inf"]] == NEG
    k = by["all but one at -inf"]
    assert lp[k] == 0.0 and rank[k] == 0 and tid[k].tolist() == [V - 2, 0, 1, 2, 3] and tlp[k].tolist() == [0.0] + [NEG] * 4
    k = by["whole row equal"]
    assert rank[k] == V // 2 and tid[k].tolist() == list(range(N))
    k = by["whole row -inf"]
    assert R.none_record((lp[k], rank[k], tid[k], tlp[k]))
    assert tid[by["tie straddling place N"]].tolist() == [2, 9, 11, 20, 30]
    assert rank[by["tie straddling place N"]] == 5
    assert rank[by["token tied with lower and higher indices"]] == 3
    assert lp[by["bf16 max-finite, token the minimum"]] == NEG and lp[by["bf16 max-finite, token the maximum"]] == 0.0
    print(f"[logprobs op] planted V={V}: measured / bound {worst.get('ratio', 0.0):.3f}  worst abs error {worst.get('abs', 0.0):.3e}")


@pytest.mark.parametrize("V,dtype", [(8200, torch.bfloat16), (1000, torch.float32)], ids=lambda x: str(x).replace("torch.", ""))
def test_row_base_misaligned_by_one_element(V, dtype):
    """a view that starts one element into its storage (2 bytes for bf16): the walkers' scalar path, same answers as the aligned copy"""
    Rn = 3
    dev, ids = _random_rows(Rn, V, dtype)
    buf = torch.empty(Rn * V + 8, dtype=dtype, device="cuda")
    view = buf[1:1 + Rn * V].view(Rn, V)
    view.copy_(dev)
    assert view.data_ptr() % 16 == dev.element_size() and view.stride(0) == V
    worst = {}
    _check(view, ids, 5, 1, worst)
    a, b = _run(view, ids, 5), _run(dev, ids, 5)
    assert (a[1] == b[1]).all() and (a[2] == b[2]).all()


def test_device_ids_outside_the_vocabulary_give_no_record():
    dev, _ = _random_rows(5, 50, torch.bfloat16)
    ids = torch.tensor([0, -1, 50, 49, 1 << 30], dtype=torch.int32, device="cuda")
    lp, rank, tid, tlp = _run(dev, ids, 3)
    for r in (1, 2, 4):
        assert R.none_record((lp[r], rank[r], tid[r], tlp[r]))
    for r in (0, 3):
        R.check_row(_stored(dev)[r], int(ids[r]), 3, 1, (lp[r], rank[r], tid[r], tlp[r]))


def test_bit_identical_across_runs_and_under_graph_replay():
    from specdec_hip.ops import TokenLogprobs, token_logprobs

    Rn, V, N = 27, 8200, 20
    dev, ids = _random_rows(Rn, V, torch.bfloat16)
    ids_d = torch.tensor(ids, dtype=torch.int32, device="cuda")
    a = token_logprobs(dev, ids_d, N)
    b = token_logprobs(dev, ids_d, N)
    bits = lambda t: t.view(torch.int32)                  # noqa: E731
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
    out = TokenLogprobs(torch.zeros(Rn, dtype=torch.float32, device="cuda"), torch.zeros(Rn, dtype=torch.int32, device="cuda"),
                        torch.zeros((Rn, N), dtype=torch.int32, device="cuda"), torch.zeros((Rn, N), dtype=torch.float32, device="cuda"))
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        token_logprobs(dev, ids_d, N, out=out)            # warm-up outside the capture
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        token_logprobs(dev, ids_d, N, out=out)
    for _ in range(2):
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(out, a))


def test_every_refusal_fires():
    from specdec_hip import _abi
    from specdec_hip.ops import token_logprobs

    lg = torch.zeros((2, 64), dtype=torch.bfloat16, device="cuda")
    for ids in ([0, 64], [-1, 0]):
        with pytest.raises(ValueError, match="outside"):
            token_logprobs(lg, ids, 1)
    for n in (-1, 21):
        with pytest.raises(ValueError, match="top_n"):
            token_logprobs(lg, [0, 0], n)
    with pytest.raises(ValueError, match="token ids for"):
        token_logprobs(lg, [0], 1)
    with pytest.raises(TypeError):
        token_logprobs(lg.to(torch.int32), [0, 0], 1)
    with pytest.raises(ValueError, match="logits"):
        token_logprobs(lg[0], [0], 1)
    with pytest.raises(ValueError, match="out must"):
        token_logprobs(lg, [0, 0], 1, out=tuple(torch.zeros(2, device="cuda") for _ in range(4)))
    lib = _abi.load()
    ids = torch.zeros(2, dtype=torch.int32, device="cuda")
    o = [torch.zeros(8, dtype=torch.int32, device="cuda") for _ in range(4)]
    ptr = [t.data_ptr() for t in o]

    def call(logits=lg.data_ptr(), dtype=_abi.SD_BF16, stride=64, Rn=2, V=64, tok=ids.data_ptr(), n=2, lp=ptr[0], rank=ptr[1], tid=ptr[2],
             tlp=ptr[3]):
        return lib.sd_token_logprobs(logits, dtype, stride, Rn, V, tok, n, lp, rank, tid, tlp, None)

    for kw, word in (({"logits": None}, "NULL"), ({"tok": None}, "NULL"), ({"lp": None}, "NULL"), ({"rank": None}, "NULL"),
                     ({"tid": None}, "NULL"), ({"tlp": None}, "NULL"), ({"V": 0}, "V="), ({"Rn": 0}, "R="), ({"n": -1}, "top_n"),
                     ({"n": 21}, "top_n"), ({"dtype": 99}, "dtype"), ({"stride": 63}, "row_stride"), ({"lp": ptr[0] + 2}, "misaligned")):
        assert call(**kw) != 0, kw
        assert word in _abi.last_error(), (kw, _abi.last_error())
    assert call() == 0
    torch.cuda.synchronize()
