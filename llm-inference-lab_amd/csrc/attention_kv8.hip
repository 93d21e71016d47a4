// The K-token attention of csrc/attention.hip over an OCP e4m3 KV cache (sd_model_set_kv_dtype): the same tile
// (attention_device.h: Q fragments, online softmax, causal / n_keys masking, wave merge through LDS, split-KV hand-over with one
// workgroup per 512 keys) around a key loop of its own, attention_blocks_kv8.
//
// Cache layout: K [B][Hkv][Lmax][D], V transposed [B][Hkv][D][Lmax], one e4m3 byte per element, written by the QKV epilogue
// (gemv_device.h kv_e4m3). A lane's natural load stays 16 bytes and now holds 16 elements, so a block is 64 keys: per block a
// wave issues 4 D / 64 key loads and D / 16 value loads (D = 128: 16 loads, the bf16 loop's count for half the keys), widens
// them to bf16 in registers (exact) and runs 8 D / 64 + D / 8 v_mfma_f32_16x16x32_bf16. k_scale rides in the softmax scale and
// v_scale in the final 1 / den, both fp32: the arithmetic is the bf16 kernel's over the dequantised cache.
//
// Resources (hipcc --save-temps, gfx950, 4 waves): D = 128: 176 unified registers (32 of them AGPRs), 44 SGPRs, no scratch: two
// waves per SIMD; D = 64: 132 registers (24 AGPRs), 54 SGPRs, no scratch.
// Built with packed fp32 VALU operations off (build.py).

#include "attention_device.h"

namespace sd {

template <int D, int NW>
__global__ __launch_bounds__(NW * 64) void attention_mfma_kv8_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int ns = a.n_split > 1 ? a.n_split : 1;
  attention_tile<D, NW, false, true>(a, blockIdx.x, blockIdx.y, blockIdx.z / ns, smem, true, blockIdx.z % ns);
}

template <int D>
static void launch_kv8_d(const AttnArgs& a, dim3 grid, hipStream_t st) {
  constexpr int NW = 4;   // as the bf16 kernel (launch_attention)
  hipLaunchKernelGGL((attention_mfma_kv8_kernel<D, NW>), grid, dim3(NW * 64), attention_smem_bytes(D, NW), st, a);   // (<= 33 KiB of LDS)
}

int launch_attention_kv8(const AttnArgs& a, dim3 grid, hipStream_t st) {
  if (a.head_dim == 64) launch_kv8_d<64>(a, grid, st);
  else launch_kv8_d<128>(a, grid, st);
  SD_LAUNCH_CHECK();
  return 0;
}

}  // namespace sd
