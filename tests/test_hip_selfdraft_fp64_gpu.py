"""The kernels that PROPOSE in the two self-drafting modes against fp64, on weights without successor structure.

Speculative decoding is lossless: a wrong draft token never changes the text, it only lowers `accepted`, so the
token-equality tests of the pipeline (engineered margins: the right logit ~ d, every other ~ sqrt(d)) cannot see a head
kernel that lost a K slice or read another head's scales. Here the step's own head evaluation (sd_model_head_argmax: one
function with the Medusa and EAGLE steps, csrc/spec_loop.hip enqueue_head_argmax) and the EAGLE extrapolation launch
(sd_eagle_extrapolate) run on N(0, 0.02) heads and random rows, and are checked with tests/stage_ref.py:

  heads   for every (head, row): the value the kernel attached to its id is that id's fp64 logit within the derived bound, and
          no other logit can have been larger (check_head_argmax); exact ties go to the lowest index wherever the work split
          puts the tied rows (check_ties);
  EAGLE   the norm row within the fp64 norm's possible flips, everything after it bit for bit (eagle_protocol);
  wiring  a captured step proposes exactly what the entries return from the same bits.

The worst error / bound of every case is printed (run with -s); profiles/selfdraft_fp64_coverage.md keeps a run."""

import pytest
import torch

import stage_ref as R
from selfdraft_cases import eagle_inputs, eagle_protocol, hidden_rows, random_heads
from specdec_hip import _abi
from specdec_hip import weights as W
from specdec_hip.engine import HipModel, HipSpecDec, PackedHeads, pack_heads
from specdec_hip.ops import eagle_extrapolate, quantize_fp8_rows_hip

pytestmark = pytest.mark.gpu


def _llama(name, d, hq, hkv, D, ff, vocab):
    return W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=1, d_model=d, n_heads=hq, n_kv_heads=hkv, head_dim=D, d_ff=ff, vocab=vocab,
                         max_pos=512, rope_theta=500000.0, tie_embeddings=False, name=name)


# (vocabulary, d_model) by the work split of the head (csrc/pack.hip gemv_geometry; tests/test_selfdraft_bounds.py checks the
# numbers): fewer workgroups than CUs with one pair each and 2 K slices; an odd vocabulary (the last pair has no second row)
# over 228 workgroups of 9 pairs in 2 tiles of 5, 8 K slices; 16 tiles per workgroup and whole-K waves, the small stand-in
# for a full vocabulary; a full vocabulary; the LayerNorm prologue at GPT-2's width
V200 = _llama("v200-d128", 128, 4, 2, 32, 256, 200)
V4099 = _llama("v4099-d2048", 2048, 32, 8, 64, 8192, 4099)
V33001 = _llama("v33001-d256", 256, 4, 2, 64, 512, 33001)
VFULL = _llama("v128256-d2048", 2048, 32, 8, 64, 8192, 128256)
GPT2 = W.ModelConfig(arch=W.ARCH_GPT2, n_layers=1, d_model=768, n_heads=12, n_kv_heads=12, head_dim=64, d_ff=3072, vocab=512,
                     max_pos=512, tie_embeddings=False, name="gpt2-d768")
TOY = _llama("toy-d256", 256, 4, 2, 64, 512, 512)

_STATE = {}


def _shape(cfg, wd, n_heads):
    """(weights, engine, heads bf16 [n][V][d], packed, the fp64 matrices the device multiplies by) of one shape: built once and
    shared by the cases (one shape at a time: the large ones hold GiBs)"""
    key = (cfg.name, wd, n_heads)
    if _STATE.get("key") != key:
        _STATE.clear()
        torch.cuda.empty_cache()
        mw = W.random_init(cfg, seed=7, device="cuda")
        eng = HipModel(mw, batch=1, l_max=64)
        heads = random_heads(n_heads, cfg.vocab, cfg.d_model, 11, device="cuda")
        packed = pack_heads(heads, wd)
        mats = []
        for h in heads:
            if wd == "fp8":          # the device quantiser's output, dequantised
                q, s = quantize_fp8_rows_hip(h)
                mats.append(q.to(torch.float64) * s.to(torch.float64)[:, None])
            else:
                mats.append(h)
        _STATE.update(key=key, val=(mw, eng, heads, packed, mats))
    return _STATE["val"]


def _first(packed, n):
    return PackedHeads(packed.buffer, packed.ptrs[:n], packed.wd, packed.vocab, packed.d_model)


@pytest.fixture(scope="module", autouse=True)
def _release_shapes():
    """the last shape's model, heads and fp64 matrices leave the device with this file"""
    yield
    _STATE.clear()
    torch.cuda.empty_cache()


def _launch(eng, n, expect=None):
    """which launches the call just made took, from what the engine reports (HipModel.head_launches); `expect` asserts it"""
    launches, gathered = eng.head_launches
    assert launches in (1, n)
    name = "gathered" if gathered else ("one-launch" if launches == 1 and n >= 2 else "per-head")
    assert not gathered or launches == n
    assert expect is None or name == expect, (name, expect, eng.head_launches)
    return name


def _check(cfg, wd, n, x, rows, per_head=False, normalised=False, n_max=None, expect=None):
    mw, eng, heads, packed, mats = _shape(cfg, wd, n_max or n)
    ids, vals = eng.head_argmax(x, _first(packed, n), rows, per_head=per_head, normalised=normalised)
    xs = x if rows is None else x[rows.long()]
    out = [R.head_stage_normed(xs, m, R.chain_hip) if normalised else R.head_stage(cfg, mw, m, xs, R.chain_hip) for m in mats[:n]]
    ref = torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])
    B = xs.shape[0]
    if expect is None:
        expect = "per-head" if per_head or n == 1 else "one-launch"
    what = f"{cfg.name} {wd} heads={n} B={B} {_launch(eng, n, expect)}{' normalised' if normalised else ''}"
    worst = R.check_head_argmax(ids, vals, ref, what)
    return worst, what, ids, vals


def _rows(B, n_rows, seed):
    """B distinct rows of n_rows in a scrambled order"""
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(n_rows, generator=g)[:B].to(torch.int32).cuda()


SHAPES = [(V200, "bf16", 4), (V200, "fp8", 4), (V4099, "bf16", 4), (V4099, "fp8", 4), (V33001, "bf16", 4), (V33001, "fp8", 4),
          (VFULL, "bf16", 2), (VFULL, "fp8", 2), (GPT2, "bf16", 4)]


@pytest.mark.parametrize("cfg,wd,n", SHAPES, ids=[f"{c.name}-{wd}" for c, wd, n in SHAPES])
def test_head_shapes(cfg, wd, n):
    """every work split: 5 gathered rows through the one launch and the per-head loop (norm prologue), and the same rows as
    already-normalised ones"""
    x = hidden_rows(10, cfg.d_model, 3, device="cuda")
    rows = _rows(5, 10, 1)
    res = []
    for per_head in (False, True):
        worst, what, ids, vals = _check(cfg, wd, n, x, rows, per_head=per_head)
        res.append((worst, ids, vals))
        print(f"[head/bound] {what}: {worst:.3f}")
    # the two launch shapes run the same tiles over the same rows: the same bits
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    worst, what, _, _ = _check(cfg, wd, n, x[:5].contiguous(), None, normalised=True)
    print(f"[head/bound] {what}: {worst:.3f}")


@pytest.mark.parametrize("wd,per_head", [("bf16", False), ("bf16", True), ("fp8", False), ("fp8", True)],
                         ids=["bf16-one-launch", "bf16-per-head", "fp8-one-launch", "fp8-per-head"])
def test_head_sweep_4099(wd, per_head):
    """head counts x row counts of the one-launch path (every token-count instantiation of gemv.hip: 1, 2, 3-5 -> 5, 9)"""
    x = hidden_rows(10, 2048, 5, device="cuda")
    worst_all = 0.0
    for n in (1, 2, 4, 8):
        for B in (1, 2, 5, 9):
            worst, what, _, _ = _check(V4099, wd, n, x, _rows(B, 10, 10 * n + B), per_head=per_head, n_max=8)
            worst_all = max(worst_all, worst)
    print(f"[head/bound] v4099-d2048 {wd} heads 1,2,4,8 x B 1,2,5,9 {'per-head' if per_head else 'one-launch (per-head at 1 head)'}: {worst_all:.3f}")


@pytest.mark.parametrize("wd", ["bf16", "fp8"])
def test_head_gathered_4099(wd):
    """more rows than a GEMV pass: gathered, then the multi-token kernel, one launch per head"""
    mw, eng, *_ = _shape(V4099, wd, 8)
    x = hidden_rows(24, 2048, 6, device="cuda")
    for B in (10, 11):
        assert B <= eng.pass_tokens
        worst, what, _, _ = _check(V4099, wd, 4, x, _rows(B, 24, B), n_max=8, expect="gathered")
        print(f"[head/bound] {what}: {worst:.3f}")


def test_head_row_indices_and_strides():
    """row indices that are a non-monotone permutation with repeats; heads at an uneven stride take one launch each and give
    the same bits; what the entry refuses"""
    mw, eng, heads, packed, mats = _shape(V4099, "bf16", 8)
    x = hidden_rows(10, 2048, 8, device="cuda")
    rows = torch.tensor([7, 0, 7, 3], dtype=torch.int32, device="cuda")
    worst, what, ids, vals = _check(V4099, "bf16", 4, x, rows, n_max=8)
    print(f"[head/bound] {what} rows [7, 0, 7, 3]: {worst:.3f}")
    assert torch.equal(ids[0], ids[2]) and torch.equal(vals[0], vals[2])
    uneven = pack_heads(heads[:4], "bf16", uneven=True)
    assert uneven.ptrs[3] - uneven.ptrs[2] != uneven.ptrs[1] - uneven.ptrs[0]
    ids_u, vals_u = eng.head_argmax(x, uneven, rows)
    assert _launch(eng, 4) == "per-head"
    assert torch.equal(ids_u, ids) and torch.equal(vals_u, vals)
    with pytest.raises(_abi.HipLibraryError, match="row_idx\\[1\\] = 10 outside"):
        eng.head_argmax(x, _first(packed, 2), torch.tensor([0, 10], dtype=torch.int32, device="cuda"))
    with pytest.raises(_abi.HipLibraryError, match="row_idx\\[0\\] = -1 outside"):
        eng.head_argmax(x, _first(packed, 2), torch.tensor([-1], dtype=torch.int32, device="cuda"))
    with pytest.raises(_abi.HipLibraryError, match="not 256-byte aligned"):
        eng.head_argmax(x, PackedHeads(packed.buffer, [packed.ptrs[0] + 64], packed.wd, packed.vocab, packed.d_model))
    with pytest.raises(_abi.HipLibraryError, match="exceeds one pass"):
        eng.head_argmax(hidden_rows(eng.pass_tokens + 1, 2048, 9, device="cuda"), _first(packed, 1))
    with pytest.raises(ValueError, match="the model's head is"):
        eng.head_argmax(x, pack_heads(heads[:1, :512].contiguous(), "bf16"))


@pytest.mark.parametrize("cfg,wd", [(V4099, "bf16"), (V4099, "fp8"), (V33001, "bf16"), (V33001, "fp8")],
                         ids=lambda v: getattr(v, "name", v))
def test_ties_go_to_the_lowest_index(cfg, wd):
    """the fp64 winner of a row, doubled and copied to both slots of one pair, a second pair of its tile, another tile, other
    workgroups (one of them in the same lane of the finalize's fold) and the last two rows of the odd vocabulary
    (stage_ref.tie_copies): the fused argmax (pair slots, tiles, the workgroup's fold) and the finalize over workgroups must
    return the lowest copy; each copy alone returns the same value bits, so the ties were exact"""
    mw = W.random_init(cfg, seed=7, device="cuda")
    eng = HipModel(mw, batch=1, l_max=64)
    V, d = cfg.vocab, cfg.d_model
    base = random_heads(1, V, d, 21, device="cuda")[0]
    x = hidden_rows(3, d, 22, device="cuda")

    def mat(h):
        if wd == "fp8":
            q, s = quantize_fp8_rows_hip(h)
            return q.to(torch.float64) * s.to(torch.float64)[:, None]
        return h

    winners = R.head_stage(cfg, mw, mat(base), x, R.chain_hip)[0].argmax(-1).tolist()
    between = 0
    for b, r in enumerate(winners):
        copies = R.tie_copies(V, d, r)
        between += copies[0] < r < copies[-1]
        heads = torch.stack([R.plant_ties(base, r, copies)] + [R.plant_ties(base, r, [p]) for p in copies])
        out = [R.head_stage(cfg, mw, mat(h), x, R.chain_hip) for h in heads]
        ref = torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])
        for per_head in (False, True):
            ids, vals = eng.head_argmax(x, pack_heads(heads, wd), per_head=per_head)
            _launch(eng, len(heads), "per-head" if per_head else "one-launch")
            R.check_ties(ids[b], vals[b], copies, ref, b, f"{cfg.name} {wd} row {b} winner {r} per_head={per_head}")
    assert between >= 1      # at least one row's winner has copies below and above it


# ---- EAGLE extrapolation ----------------------------------------------------------------------------------------------------------
def _dev_eagle(x, prev, has, w, b, eps, alpha, K, rms):
    p, h = prev.clone(), has.clone()
    H = eagle_extrapolate(x, p, h, w, b, eps, alpha, K, rms)
    return H, p, h


EAGLE_D = [(64, True), (136, True), (768, False), (2048, True), (3072, True), (4096, True)]


@pytest.mark.parametrize("form", ["plain", "spikes", "offset"])
@pytest.mark.parametrize("d,rms", EAGLE_D, ids=[f"d{d}-{'rms' if r else 'layernorm'}" for d, r in EAGLE_D])
def test_eagle_extrapolation(d, rms, form):
    """B x K x alpha x (state of earlier calls | random state rows), has_prev mixed per row. The offset form (8 standard
    deviations common to all channels) is a choice: nobody has measured what the residual rows of real checkpoints carry."""
    eps = 1e-5
    flips = n = 0
    worst = 0.0
    for B in (1, 3, 9):
        x, prev, w, b = eagle_inputs(B, d, 100 * B + d, form, device="cuda")
        nb = None if rms else b
        has = (torch.arange(B, device="cuda") % 3 != 1).to(torch.int32)           # rows 1, 4, 7 start without a state
        for K in (1, 2, 4, 8):
            for alpha in (0.0, 0.7, 1.5):
                # the state two earlier calls leave behind (another x, then this x's neighbour): h_K of a real recurrence
                x1, p1, _, _ = eagle_inputs(B, d, 7 * K + B, form, device="cuda")
                _, st, hs = _dev_eagle(x1, p1, torch.zeros(B, dtype=torch.int32, device="cuda"), w, nb, eps, alpha, K, rms)
                _, st, hs = _dev_eagle(p1, st, hs, w, nb, eps, alpha, K, rms)
                for state in (st, prev):
                    f, r = eagle_protocol(_dev_eagle, x, state, has, w, nb, eps, alpha, K, rms, f"d={d} {form} B={B} K={K} alpha={alpha}")
                    flips, n, worst = flips + f, n + B * d, max(worst, r)
    print(f"[eagle/bound] d={d} {'rms' if rms else 'layernorm'} {form}: {flips} of {n} norm elements on the other neighbour, "
          f"needing at most {worst:.3f} of the allowed statistic error; recurrence and state bit-exact")


def test_eagle_rows_are_independent():
    """a change of one row's state changes that row alone: the other rows' H and state keep their bits"""
    B, d, K = 3, 768, 4
    x, prev, w, b = eagle_inputs(B, d, 5, device="cuda")
    has = torch.ones(B, dtype=torch.int32, device="cuda")
    H0, e0, _ = _dev_eagle(x, prev, has, w, b, 1e-5, 0.7, K, False)
    prev2, has2 = prev.clone(), has.clone()
    prev2[1] = (prev[1].float() * 2 + 1).bfloat16()
    H1, e1, _ = _dev_eagle(x, prev2, has, w, b, 1e-5, 0.7, K, False)
    has2[1] = 0
    H2, e2, _ = _dev_eagle(x, prev, has2, w, b, 1e-5, 0.7, K, False)
    for H, e in ((H1, e1), (H2, e2)):
        assert torch.equal(H[[0, 2]], H0[[0, 2]]) and torch.equal(e[[0, 2]], e0[[0, 2]])
        assert not torch.equal(H[1], H0[1]) and not torch.equal(e[1], e0[1])


# ---- step wiring ------------------------------------------------------------------------------------------------------------------
def _loop(B, K, seed):
    mw = W.random_init(TOY, seed=seed, device="cuda")
    eng = HipModel(mw, batch=B, l_max=256)
    loop = HipSpecDec(None, eng, B, K, HipSpecDec.EMIT_BONUS)
    return mw, eng, loop


def _start(eng, loop, B, seed):
    g = torch.Generator().manual_seed(seed)
    prompts = torch.randint(4, TOY.vocab, (B, 9), generator=g).to(torch.int32)
    eng.forward(prompts[:, :-1].contiguous().cuda(), torch.zeros(B, dtype=torch.int32, device="cuda"), 0, skip_head=True)
    for b in range(B):
        loop.set_row(b, 9, int(prompts[b, -2]), int(prompts[b, -1]), True)
    loop.join_current_stream()


def test_medusa_step_proposes_what_the_entry_returns():
    """random heads, B = 3, K = 4: after step s the entry, fed the verify pass's hidden rows and the record's accept lengths,
    returns exactly the draft tokens step s + 1 records — eager step, capture, and replays of the captured graph"""
    B, K = 3, 4
    mw, eng, loop = _loop(B, K, 3)
    loop.set_medusa(random_heads(K, TOY.vocab, TOY.d_model, 4, device="cuda"))
    _start(eng, loop, B, 5)
    want = None
    for s in range(6):
        loop.step()
        rec = loop.sync()
        if want is not None:
            assert rec.draft_tokens.tolist() == want, (s, rec.draft_tokens.tolist(), want)
        hidden = eng.hidden_rows(B * (K + 1))
        rows = torch.tensor([b * (K + 1) + int(rec.accept_len[b]) for b in range(B)], dtype=torch.int32, device="cuda")
        ids, _ = eng.head_argmax(hidden, loop._heads_packed, rows)
        want = ids.cpu().tolist()
        torch.cuda.synchronize()
    assert loop.launches == 6


@pytest.mark.parametrize("B", [2, 3], ids=["8-rows-gemv", "12-rows-multitoken"])
def test_eagle_step_proposes_what_the_entries_return(B):
    """after each captured EAGLE step, on its workspace: the state is h_K, rows k >= 2 follow from rows k - 1 and k - 2 bit
    for bit (h_t itself is overwritten by the verify pass inside the step; a row's first step extrapolates nothing), and the
    step's draft tokens are the entry's ids over those rows with a packed copy of the lm_head, rows already normalised"""
    K, d, alpha = 4, TOY.d_model, 0.7
    mw, eng, loop = _loop(B, K, 6)
    ws = loop.set_eagle(alpha)
    loop.reset_eagle()
    off = -ws.data_ptr() % 256                       # the carve of sd_specdec_set_eagle
    al = lambda v: (v + 255) // 256 * 256
    prev = ws[off:off + B * d * 2].view(torch.bfloat16).view(B, d)
    has = ws[off + al(B * d * 2):off + al(B * d * 2) + B * 4].view(torch.int32)
    o_h = off + al(B * d * 2) + al(B * 4)
    H = ws[o_h:o_h + B * K * d * 2].view(torch.bfloat16).view(B, K, d)
    head = pack_heads(mw.lm_head[None].contiguous(), "bf16")
    _start(eng, loop, B, 7)
    for s in range(5):
        had = has.clone()
        loop.step()
        rec = loop.sync()
        assert has.tolist() == [1] * B and torch.equal(prev, H[:, K - 1])
        if s == 0:
            assert had.tolist() == [0] * B and all(torch.equal(H[:, k], H[:, 0]) for k in range(K))
        else:
            assert not torch.equal(H[:, 1], H[:, 0])
        one = torch.ones(B, dtype=torch.int32, device="cuda")
        for k in range(2, K):
            nxt, _ = R.eagle_recurrence(H[:, k - 1], H[:, k - 2], one, alpha, 1)
            assert torch.equal(nxt[:, 0], H[:, k]), (s, k)
        ids, _ = eng.head_argmax(H.reshape(B * K, d).clone(), head, normalised=True)
        assert rec.draft_tokens.tolist() == ids.view(B, K).cpu().tolist(), s
        torch.cuda.synchronize()
