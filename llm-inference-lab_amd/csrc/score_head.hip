// Log-likelihood of a token sequence (sd_model_score): the lm_head as a GEMM over the packed tile stream whose epilogue reduces each
// token's logits instead of storing them.
//
// What it replaces: asking sd_model_forward for the [n][V] fp32 logits and reducing them in torch — that turns the GEMM prefill off
// and writes V x 4 bytes per position (1.05 GB for 2048 positions at V = 128256) to read back one number per position.
//
//   * score_head_kernel<RF, W8> — the main loop of prefill_mfma_kernel (prefill_mfma_device.h: same row blocks of whole packed tiles,
//     128 tokens per workgroup, LDS-DMA double buffering), then per token over the block's rows: the logit is exactly the value
//     EPI_ARGMAX forms (fp32 product, times the row scale for fp8, rounded once to bf16), folded into (max m, sum of exp(l - m),
//     argmax value, argmax row) — lanes of a row of 16 by xor shuffles, then the two row halves of the workgroup through LDS, in a
//     fixed order — and written as one 16-byte partial per (row block, token). The one lane that holds row target[t] stores that
//     logit. The pad row of an odd vocabulary (hrow = -1) takes no part. No atomics.
//   * score_finalize_kernel — one workgroup per token folds the token's partials in a fixed order (thread i: blocks i, i + 256,
//     ...; then a fixed tree) and writes lse = M + log S, logprob = l_target - lse and the greedy row. Bit-identical run to run.
//   * score_logits_kernel<RF, W8> (sd_model_score_logits) — a second epilogue over the same main loop: each token's logit, the same
//     bf16 value, is STORED to logits[t][HF row] (the pad row of an odd vocabulary is not) and folded into the same partials, so
//     score_finalize_kernel returns the greedy rows sd_model_score returns. It keeps no target logit.

#include "prefill_mfma_device.h"

namespace sd {

namespace {

constexpr int kFinThreads = 256;

// (max, sum of exp(l - max)) of two disjoint sets; an empty set is (-inf, 0)
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const float M = fmaxf(m, om);
  if (M == -INFINITY) return;
  s = (m == -INFINITY ? 0.f : s * expf(m - M)) + (om == -INFINITY ? 0.f : os * expf(om - M));
  m = M;
}

__device__ __forceinline__ void fold(float4& a, float4 b) {
  lse_merge(a.x, a.y, b.x, b.y);
  const int bi = __float_as_int(b.w), ai = __float_as_int(a.w);
  if (argmax_better(b.z, bi, a.z, ai)) {
    a.z = b.z;
    a.w = b.w;
  }
}

template <int RF, bool W8>
__global__ __launch_bounds__(kThreads, 2) void score_head_kernel(MfmaArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[mfma_smem_bytes<RF, W8>()];
  f32x4_t acc[4][RF];
  int hrow[RF], t0, rb;
  mfma_block_product<RF, W8>(a, smem, acc, hrow, t0, rb);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wt = wave & 1, wr = wave >> 1, g = lane >> 4, n = lane & 15;
  float sc[RF];
#pragma unroll
  for (int f = 0; f < RF; ++f) sc[f] = (W8 && hrow[f] >= 0) ? a.w_scale[hrow[f]] : 1.0f;

  __syncthreads();   // every wave is done with the stage buffers: the first 4 KiB hold the row halves' partials
  float4* red = reinterpret_cast<float4*>(smem);   // [wr][128 tokens]
  // lane (n, g) holds tokens 4 g + e of fragment row q, for weight row (fragment column) n of fragment f
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int tl = wt * 64 + q * 16 + 4 * g + e, t = t0 + tl;
      const int tgt = t < a.n_target ? a.target[t] : -1;
      float l[RF];
      float m = -INFINITY;
#pragma unroll
      for (int f = 0; f < RF; ++f) {
        l[f] = bf16_bits_to_float(float_to_bf16_bits(acc[q][f][e] * sc[f]));   // the logit EPI_ARGMAX forms
        if (hrow[f] >= 0) m = fmaxf(m, l[f]);
      }
      float4 p = {m, 0.f, -INFINITY, __int_as_float(0x7fffffff)};
#pragma unroll
      for (int f = 0; f < RF; ++f)
        if (hrow[f] >= 0) {
          if (m != -INFINITY) p.y += expf(l[f] - m);
          if (argmax_better(l[f], hrow[f], p.z, __float_as_int(p.w))) {
            p.z = l[f];
            p.w = __int_as_float(hrow[f]);
          }
          if (hrow[f] == tgt && t < a.T) a.tgt_logit[t] = l[f];
        }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
        const float4 o = {__shfl_xor(p.x, off, 64), __shfl_xor(p.y, off, 64), __shfl_xor(p.z, off, 64), __shfl_xor(p.w, off, 64)};
        fold(p, o);
      }
      if (n == 0) red[wr * kBT + tl] = p;
    }
  __syncthreads();
  if (tid < kBT && t0 + tid < a.T) {
    float4 p = red[tid];
    fold(p, red[kBT + tid]);
    a.part[static_cast<size_t>(t0 + tid) * a.n_blocks + rb] = p;
  }
}

template <int RF, bool W8>
__global__ __launch_bounds__(kThreads, 2) void score_logits_kernel(MfmaArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[mfma_smem_bytes<RF, W8>()];
  f32x4_t acc[4][RF];
  int hrow[RF], t0, rb;
  mfma_block_product<RF, W8>(a, smem, acc, hrow, t0, rb);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wt = wave & 1, wr = wave >> 1, g = lane >> 4, n = lane & 15;
  float sc[RF];
#pragma unroll
  for (int f = 0; f < RF; ++f) sc[f] = (W8 && hrow[f] >= 0) ? a.w_scale[hrow[f]] : 1.0f;

  __syncthreads();   // every wave is done with the stage buffers: the first 4 KiB hold the row halves' partials
  float4* red = reinterpret_cast<float4*>(smem);   // [wr][128 tokens]
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int tl = wt * 64 + q * 16 + 4 * g + e, t = t0 + tl;
      uint16_t* out = a.logits + static_cast<size_t>(t) * a.N;
      float l[RF];
      float m = -INFINITY;
#pragma unroll
      for (int f = 0; f < RF; ++f) {
        const uint16_t bits = float_to_bf16_bits(acc[q][f][e] * sc[f]);   // the logit EPI_ARGMAX forms
        l[f] = bf16_bits_to_float(bits);
        if (hrow[f] >= 0) {
          m = fmaxf(m, l[f]);
          if (t < a.T) out[hrow[f]] = bits;
        }
      }
      float4 p = {m, 0.f, -INFINITY, __int_as_float(0x7fffffff)};
#pragma unroll
      for (int f = 0; f < RF; ++f)
        if (hrow[f] >= 0) {
          if (m != -INFINITY) p.y += expf(l[f] - m);
          if (argmax_better(l[f], hrow[f], p.z, __float_as_int(p.w))) {
            p.z = l[f];
            p.w = __int_as_float(hrow[f]);
          }
        }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
        const float4 o = {__shfl_xor(p.x, off, 64), __shfl_xor(p.y, off, 64), __shfl_xor(p.z, off, 64), __shfl_xor(p.w, off, 64)};
        fold(p, o);
      }
      if (n == 0) red[wr * kBT + tl] = p;
    }
  __syncthreads();
  if (tid < kBT && t0 + tid < a.T) {
    float4 p = red[tid];
    fold(p, red[kBT + tid]);
    a.part[static_cast<size_t>(t0 + tid) * a.n_blocks + rb] = p;
  }
}

// token blockIdx.x: fold its n_blocks partials -> lse; logprob (t < n_target) and greedy row
__global__ __launch_bounds__(kFinThreads) void score_finalize_kernel(const float4* part, int n_blocks, const float* tgt_logit, int n_target,
                                                                     float* logprob, int32_t* greedy) {
  __shared__ float4 red[kFinThreads];
  const int t = blockIdx.x, tid = threadIdx.x;
  const float4* pt = part + static_cast<size_t>(t) * n_blocks;
  float4 p = {-INFINITY, 0.f, -INFINITY, __int_as_float(0x7fffffff)};
  for (int b = tid; b < n_blocks; b += kFinThreads) fold(p, pt[b]);
  red[tid] = p;
  __syncthreads();
  for (int w = kFinThreads / 2; w > 0; w >>= 1) {
    if (tid < w) {
      float4 v = red[tid];
      fold(v, red[tid + w]);
      red[tid] = v;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float4 r = red[0];
    const float lse = r.x + logf(r.y);
    if (logprob && t < n_target) logprob[t] = tgt_logit[t] - lse;
    if (greedy) greedy[t] = __float_as_int(r.w);
  }
}

}  // namespace

size_t score_partial_bytes(const NativePlan& plan) {
  const int nb = plan.mat[4][0].n_blocks > plan.mat[4][1].n_blocks ? plan.mat[4][0].n_blocks : plan.mat[4][1].n_blocks;
  return static_cast<size_t>(kPrefillChunk) * nb * sizeof(float4);
}

int launch_score_head(const NativePlan& plan, const void* W, const float* w_scale, bool w8, const uint16_t* Xn, int T, const int32_t* target,
                      int n_target, float4* part, float* tgt_logit, float* logprob, int32_t* greedy, uint16_t* logits, hipStream_t st) {
  SD_REQUIRE(plan.buf && plan.mat[4][0].tiles, "score: lm_head plan not built");
  SD_REQUIRE(T >= 1 && T <= kPrefillChunk && n_target >= 0 && n_target <= T, "score: head over %d rows (%d targets)", T, n_target);
  SD_REQUIRE(W && Xn && part && tgt_logit && (!w8 || w_scale) && (n_target == 0 || target), "score: head with a NULL operand");
  const int n_tb = (T + kBT - 1) / kBT;
  const int v = plan.mat[4][0].n_blocks * n_tb >= 256 ? 0 : 1;   // the rule of launch_prefill_mfma
  const NativeMat& m = plan.mat[4][v];
  MfmaArgs a{};
  a.W = static_cast<const char*>(W);
  a.w_scale = w_scale;
  a.X = reinterpret_cast<const char*>(Xn);
  a.tiles = m.tiles;
  a.blocks = m.blocks;
  a.T = T;
  a.N = m.N;
  a.K = m.K;
  a.ldx = m.K;
  a.n_blocks = m.n_blocks;
  a.n_tb = n_tb;
  a.row_bytes = w8 ? ((m.K + 63) & ~63) : ((m.K + 31) & ~31) * 2;
  a.epi = m.epi;
  a.head_dim = plan.head_dim;
  a.n_pairs = m.n_pairs;
  a.target = target;
  a.tgt_logit = tgt_logit;
  a.part = part;
  a.n_target = n_target;
  a.logits = logits;
  const dim3 grid(m.n_blocks * n_tb), block(kThreads);
  if (logits) {   // sd_model_score_logits: no target logit, no logprob
    if (w8) {
      if (v == 0) hipLaunchKernelGGL((score_logits_kernel<4, true>), grid, block, 0, st, a);
      else hipLaunchKernelGGL((score_logits_kernel<2, true>), grid, block, 0, st, a);
    } else {
      if (v == 0) hipLaunchKernelGGL((score_logits_kernel<4, false>), grid, block, 0, st, a);
      else hipLaunchKernelGGL((score_logits_kernel<2, false>), grid, block, 0, st, a);
    }
    SD_LAUNCH_CHECK();
    if (greedy) hipLaunchKernelGGL(score_finalize_kernel, dim3(T), dim3(kFinThreads), 0, st, part, m.n_blocks, tgt_logit, 0, nullptr, greedy);
    SD_LAUNCH_CHECK();
    return 0;
  }
  // a target row that is not a vocabulary row leaves NaN (0xffffffff), not a stale logit
  SD_HIP_CHECK(hipMemsetAsync(tgt_logit, 0xff, static_cast<size_t>(T) * sizeof(float), st));
  if (w8) {
    if (v == 0) hipLaunchKernelGGL((score_head_kernel<4, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((score_head_kernel<2, true>), grid, block, 0, st, a);
  } else {
    if (v == 0) hipLaunchKernelGGL((score_head_kernel<4, false>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((score_head_kernel<2, false>), grid, block, 0, st, a);
  }
  SD_LAUNCH_CHECK();
  hipLaunchKernelGGL(score_finalize_kernel, dim3(T), dim3(kFinThreads), 0, st, part, m.n_blocks, tgt_logit, n_target, logprob, greedy);
  SD_LAUNCH_CHECK();
  return 0;
}

}  // namespace sd
