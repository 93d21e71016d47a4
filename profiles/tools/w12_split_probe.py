"""bf16 against the two forms of the W12 copy, class by class (profiles/w12_split.md): the 5-token launch of every matrix class of a
model timed with sd_model_probe_gemv on its packed bf16 stream, its code-form copy and its split-byte (W12S) copy, in one
process, alternating, RUNS times each; then narrow share and bytes of both copies per class.
python profiles/tools/w12_split_probe.py [preset] [tokens]"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "llm-inference-lab_amd"))
os.environ["SPECDEC_W12"] = "0"            # the model is created without a copy: both are built and switched below
import torch  # noqa: E402

from specdec_hip import _abi  # noqa: E402
from specdec_hip import weights as W  # noqa: E402
from specdec_hip.engine import W12_CODES, W12_SPLIT, HipModel, build_w12, w12_matrix_info  # noqa: E402
from specdec_hip.ops import gemv_instance  # noqa: E402

RUNS = 4
preset = {"3b": W.LLAMA_3_2_3B, "1b": W.LLAMA_3_2_1B, "8b": W.LLAMA_3_8B}[sys.argv[1] if len(sys.argv) > 1 else "3b"]
T = int(sys.argv[2]) if len(sys.argv) > 2 else 5
mw = W.synthetic_llama(preset, seed=0, device="cuda")
hm = HipModel(mw, batch=1, l_max=64)
lib, dev = hm.lib, hm.device
copies = {form: build_w12(lib, hm._mc, dev, 0x1F, form) for form in (W12_CODES, W12_SPLIT)}
st = torch.cuda.Stream()
names = {0: "qkv", 1: "out", 2: "gate/up", 3: "down", 4: "lm_head"}


def route(form):
    """every class on bf16 (form 0), on the code form or on the split-byte form"""
    _abi.check(lib.sd_model_set_w12(hm.handle, None, None, 0), "sd_model_set_w12")
    if form:
        buf, n_wide = copies[form]
        _abi.check(lib.sd_model_set_w12_form(hm.handle, buf.data_ptr(), n_wide.ctypes.data, 0x1F, form), "sd_model_set_w12_form")


print(f"{preset.name}, {T} tokens, us per launch, {RUNS} alternating runs")
for which in range(5):
    _, K, n_pairs, epi, pro = hm.matrix_shape(which)
    res = {0: [], W12_CODES: [], W12_SPLIT: []}
    for _ in range(RUNS):
        for form in res:
            route(form)
            us, _nb = hm.probe_gemv(which, T=T, iters=200 if which != 4 else 60, stream=st)
            res[form].append(us)
    inst = {form: gemv_instance(T, n_pairs, K, False, pro, epi, w12=form) for form in res}
    for form, tag in ((0, "bf16"), (W12_CODES, "w12"), (W12_SPLIT, "w12s")):
        print(f"{names[which]:8s} {tag:5s} {inst[form]:44s} " + " ".join(f"{u:7.2f}" for u in res[form]), flush=True)
    wins = max(res[W12_SPLIT]) < min(res[0])
    wins_codes = max(res[W12_SPLIT]) < min(res[W12_CODES])
    print(f"{names[which]:8s} every w12s run under every bf16 run: {wins}; under every w12 run: {wins_codes}")
route(0)

print("class | blocks | code form narrow, bytes | W12S narrow, bytes | bf16 bytes")
L = hm.cfg.n_layers
for which in range(5):
    idxs = [4 * L] if which == 4 else [4 * l + which for l in range(L)]
    row = []
    for form in (W12_CODES, W12_SPLIT):
        n_wide = copies[form][1]
        infos = [w12_matrix_info(lib, hm._mc, n_wide, i, form=form) for i in idxs]
        blocks = sum(i["blocks"] for i in infos)
        wide = sum(i["n_wide"] for i in infos)
        nbytes = sum(i["main_bytes"] + i["ovf_bytes"] + i["table_bytes"] for i in infos if i["taken"])
        bf16 = sum(i["bf16_bytes"] for i in infos)
        row.append(f"{100 * (1 - wide / blocks):.2f} % {nbytes / 1e6:.1f} MB ({nbytes / bf16:.4f})")
    print(f"{names[which]:8s} | {blocks} | {row[0]} | {row[1]} | {bf16 / 1e6:.1f} MB")
