"""Registers and scratch of every fixed-geometry instance of csrc/gemv.hip, and of every W12 instance (fixed or generic), read from the code object's metadata
(.vgpr_count, .sgpr_count, .private_segment_fixed_size, .vgpr_spill_count): python profiles/tools/gemv_fixed_resources.py [code object]
Without an argument, gemv.hip is compiled for the device alone (no GPU needed). Exits 1 if an instance has scratch, spills or
more than 128 VGPRs (16 waves per CU need <= 128)."""
import os, re, subprocess, sys, tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
EPI = {0: "qkv", 1: "resid", 2: "swiglu", 3: "gelu", 4: "argmax"}
PRO = {0: "none", 1: "rmsnorm"}

co = sys.argv[1] if len(sys.argv) > 1 else None
if co is None:
    co = os.path.join(tempfile.mkdtemp(), "gemv.co")
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-gpu-rdc", "--cuda-device-only", "--no-gpu-bundle-output",
                    f"-I{ROOT}/include", "-x", "hip", "-c", f"{ROOT}/llm-inference-lab_amd/csrc/gemv.hip", "-o", co], check=True)
notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
bad = 0
rows = []
for k in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
    f = {m.group(1): m.group(2) for m in re.finditer(r"\.(\w+):\s+(\S+)", k)}
    m = re.match(r"_ZN2sd16gemv_mfma_kernelILi(\d)ELb0ELi(\d+)ELb0ELi(\d+)ELi(n?\d+)ELi(\d+)ELi(\d+)ELi([012])EEE", f.get("name", ""))
    if not m or (m.group(4) == "n1" and m.group(7) == "0"):
        continue   # the generic bf16 / fp8 / MASK kernels (FKS = -1) and other kernels
    e, tt, kb, tp, pro, w12 = (int(m.group(i)) for i in (1, 2, 3, 5, 6, 7))
    ks = -1 if m.group(4) == "n1" else int(m.group(4))
    vg, sg, scratch, spill = int(f["vgpr_count"]), int(f["sgpr_count"]), int(f["private_segment_fixed_size"]), int(f["vgpr_spill_count"])
    flag = "" if (scratch == 0 and spill == 0 and vg <= 128) else "  <-- over the limit"
    bad += bool(flag)
    form = ("", "w12", "w12s")[w12]   # W12Form: none, codes, split
    name = f"generic<{EPI[e]},whole,tt{tt},{form},kb{kb}>" if ks < 0 else f"fixed<{EPI[e]},ks{1 << ks},tp{tp},{PRO[pro]},tt{tt},kb{kb}{',' + form if w12 else ''}>"
    rows.append(f"{name}: vgpr {vg} sgpr {sg} scratch {scratch} vgpr_spill {spill}{flag}")
print("\n".join(sorted(rows)))
print(f"{len(rows)} fixed / W12 instances, {bad} over the limit")
sys.exit(1 if bad or not rows else 0)
