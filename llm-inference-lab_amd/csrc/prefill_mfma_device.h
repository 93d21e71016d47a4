// The main loop of the native GEMM over the packed tile streams, shared by its two kernels: prefill_mfma_kernel
// (csrc/prefill_mfma.hip, fp32 products stored in HF row order) and score_head_kernel (csrc/score_head.hip, the lm_head with the
// products reduced to a log-sum-exp / argmax partial per token). Stream layout and decomposition: csrc/prefill_mfma.hip.
// Included by .hip files only.
#pragma once

#include "gemv_device.h"
#include "prefill_gemm.h"

namespace sd {

namespace {

constexpr int kThreads = 256;
constexpr int kBT = 128;              // tokens per workgroup
constexpr int kXBytes = kBT * 128;    // x stage: 128 tokens x 64 k (bf16)

struct MfmaArgs {
  const char* W;            // packed stream of the matrix
  const float* w_scale;     // fp8: fp32 scale per HF row
  const char* X;            // bf16 [T][ldx]
  float* Y;                 // fp32 [T][N]
  const int4* tiles;        // {first row in its block, pairs, first pair, 0}
  const int2* blocks;       // {first tile, tiles}
  int T, N, K, ldx;
  int n_blocks, n_tb;       // row blocks, token blocks
  int row_bytes;            // bytes of one packed row of the stream (K padded to 32 / 64)
  int epi, head_dim, n_pairs;
  // score_head_kernel (csrc/score_head.hip) only
  const int32_t* target;    // [n_target] HF row whose logit token t keeps (the next token)
  float* tgt_logit;         // [T] logit of row target[t]
  float4* part;             // [T][n_blocks] {max, sum of exp(l - max), argmax value, argmax row (int bits)}
  int n_target;
  // score_logits_kernel (csrc/score_head.hip) only
  uint16_t* logits;         // bf16 [T][N], HF row order: every token's logits as the score epilogue forms them
};

__device__ __forceinline__ void glds16(const char* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)lds_wave_base, 16,
                                   0, 0);
}

// HF row of packed row j (0 .. 2 np - 1) of the tile whose first pair is p0 (the rule of pack_pair_rows)
__device__ __forceinline__ int hf_row(const MfmaArgs& a, int p0, int np, int j) {
  const int second = j >= np ? 1 : 0;
  const int p = p0 + j - second * np;
  int r0, r1;
  if (a.epi == EPI_QKV_ROPE) {
    const int half = a.head_dim >> 1;
    const int h = p / half, i = p - h * half;
    r0 = h * a.head_dim + i;
    r1 = r0 + half;
  } else if (a.epi == EPI_SWIGLU) {
    r0 = p;
    r1 = p + a.n_pairs;
  } else {
    r0 = 2 * p;
    r1 = 2 * p + 1;
  }
  return second ? r1 : r0;
}

// LDS of one workgroup: two stages of (x tile, weight pieces)
template <int RF, bool W8>
constexpr int mfma_smem_bytes() { return 2 * (kXBytes + 2 * RF * 16 * (W8 ? 64 : 128)); }

// The main loop of a workgroup: acc[q][f] = the fp32 products of its 128 tokens (fragment rows q of the wave's 64) x its RB
// packed rows (fragment columns f), hrow[f] = the HF row of this lane's fragment column (-1: past N or no row), t0 = first
// token, rb = row block. Every thread of the workgroup calls it; smem is mfma_smem_bytes<RF, W8>() of LDS.
template <int RF, bool W8>
__device__ __forceinline__ void mfma_block_product(const MfmaArgs& a, char* smem, f32x4_t (&acc)[4][RF], int (&hrow)[RF], int& t0, int& rb) {
  constexpr int SB = W8 ? 64 : 128;              // bytes of one packed row per 64-k stage
  constexpr int RB = 2 * RF * 16;                // weight rows per workgroup
  constexpr int kWBytes = RB * SB;
  constexpr int kBuf = kXBytes + kWBytes;
  constexpr int XCH = kXBytes / 16 / kThreads;   // 16-byte x pieces per thread per stage
  constexpr int WCH = kWBytes / 16 / kThreads;   // 16-byte weight pieces per thread per stage
  static_assert(WCH >= 1 && XCH == 4, "stage geometry");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int wt = wave & 1, wr = wave >> 1;       // token half, row half of the workgroup tile

  // workgroup -> (row block, token block): native_block_of (csrc/prefill_gemm.h)
  const int L = native_block_of(static_cast<int>(blockIdx.x), a.n_blocks * a.n_tb);
  rb = L / a.n_tb;
  const int tb = L - rb * a.n_tb;
  const int2 blk = a.blocks[rb];
  t0 = tb * kBT;

  // per lane: B-fragment offsets in the weight image and the HF row of each fragment column; sources of the weight pieces
  int woff[RF], wstep[RF];
#pragma unroll
  for (int f = 0; f < RF; ++f) { woff[f] = 0; wstep[f] = 0; hrow[f] = -1; }
  uint32_t dsrc[WCH], dstr[WCH];
  bool dval[WCH];
#pragma unroll
  for (int c = 0; c < WCH; ++c) { dsrc[c] = 0; dstr[c] = 0; dval[c] = false; }
  for (int k = 0; k < blk.y; ++k) {
    const int4 tl = a.tiles[blk.x + k];
    const int rs = tl.x, np = tl.y, p0 = tl.z, nr = 2 * tl.y;
#pragma unroll
    for (int f = 0; f < RF; ++f) {
      const int R = wr * RF * 16 + f * 16 + n;
      if (R >= rs && R < rs + nr) {
        const int j = R - rs;
        woff[f] = rs * SB + (g * nr + j) * 16;
        wstep[f] = nr * 64;
        const int r = hf_row(a, p0, np, j);
        hrow[f] = r < a.N ? r : -1;
      }
    }
#pragma unroll
    for (int c = 0; c < WCH; ++c) {
      const int byte = ((c * 4 + wave) * 64 + lane) * 16;
      const int row = byte / SB;
      if (row >= rs && row < rs + nr) {
        dsrc[c] = static_cast<uint32_t>(p0) * 2u * static_cast<uint32_t>(a.row_bytes) + static_cast<uint32_t>(byte - rs * SB);
        dstr[c] = static_cast<uint32_t>(nr * SB);
        dval[c] = true;
      }
    }
  }
  // x pieces: token row tr, 16-byte slot sl of the LDS image holds k-chunk sl ^ (tr & 7) (rows past T repeat row T - 1)
  uint32_t xsrc[XCH];
#pragma unroll
  for (int c = 0; c < XCH; ++c) {
    const int idx = (c * 4 + wave) * 64 + lane;
    const int tr = idx >> 3, sl = idx & 7;
    const int t = min(t0 + tr, a.T - 1);
    xsrc[c] = static_cast<uint32_t>(t) * static_cast<uint32_t>(a.ldx) * 2u + static_cast<uint32_t>((sl ^ (tr & 7)) * 16);
  }
  const int xrow = (wt * 64 + n) * 128;
  const int xo0 = (g ^ (n & 7)) * 16, xo1 = ((4 + g) ^ (n & 7)) * 16;

  auto issue = [&](int s, int b) {
    char* xb = smem + b * kBuf;
    char* wb = xb + kXBytes;
#pragma unroll
    for (int c = 0; c < XCH; ++c) glds16(a.X + xsrc[c] + static_cast<uint32_t>(s) * 128u, xb + (c * 4 + wave) * 1024);
#pragma unroll
    for (int c = 0; c < WCH; ++c)
      if (dval[c]) glds16(a.W + dsrc[c] + static_cast<uint32_t>(s) * dstr[c], wb + (c * 4 + wave) * 1024);
  };

#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int f = 0; f < RF; ++f) acc[q][f] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int S = a.K >> 6;
  issue(0, 0);
  for (int s = 0; s < S; ++s) {
    __syncthreads();                       // stage s has landed (the wait for the DMA precedes the barrier); buffer s+1 is free
    if (s + 1 < S) issue(s + 1, (s + 1) & 1);
    const char* xb = smem + (s & 1) * kBuf;
    const char* wb = xb + kXBytes;
    u32x4 wf[2][RF];
#pragma unroll
    for (int f = 0; f < RF; ++f) {
      if constexpr (W8) {
        const u32x4 raw = *reinterpret_cast<const u32x4*>(wb + woff[f]);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          wf[0][f][2 * e] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(raw[e], 1.0f, false));
          wf[0][f][2 * e + 1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(raw[e], 1.0f, true));
          wf[1][f][2 * e] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(raw[2 + e], 1.0f, false));
          wf[1][f][2 * e + 1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(raw[2 + e], 1.0f, true));
        }
      } else {
        wf[0][f] = *reinterpret_cast<const u32x4*>(wb + woff[f]);
        wf[1][f] = *reinterpret_cast<const u32x4*>(wb + woff[f] + wstep[f]);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const u32x4 xa = *reinterpret_cast<const u32x4*>(xb + xrow + q * 16 * 128 + (u ? xo1 : xo0));
#pragma unroll
        for (int f = 0; f < RF; ++f)
          acc[q][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, xa), __builtin_bit_cast(bf16x8_t, wf[u][f]),
                                                              acc[q][f], 0, 0, 0);
      }
    }
  }
}

}  // namespace

}  // namespace sd
