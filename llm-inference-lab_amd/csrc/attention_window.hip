// Sliding-window attention for the decode / verify / 128-position-pass shape (sd_model_set_sliding_window): the query at absolute
// position p sees exactly the keys max(0, p - W + 1) .. p, W keys including its own. The cache is sized and appended as ever; only
// what attention READS changes, and the cost of a launch follows W instead of the row's length.
//
// Geometry and fragments are those of attention_mfma_kernel (attention.hip, attention_device.h): one workgroup per (row, kv head,
// 16-row query tile[, split]), four waves over 32-key blocks, S^T = K Q^T and P V with v_mfma_f32_16x16x32_bf16, K and V^T
// fragments loaded straight from L2 / HBM, P the unpermuted A operand of the second product. What the window adds:
//   span        a tile walks the blocks [b_lo, n_blocks) only, b_lo = max(0, pos0 + m_min - W + 1) / 32 with m_min the smallest
//               query index among the tile's rows. A block below b_lo is neither loaded nor multiplied: whatever such keys hold
//               (a NaN included) cannot reach the output.
//   block body  three masks, chosen per block from pos0, M, W and the tile's row range [m_min, m_max] alone (wave-uniform):
//                 lower edge  key0 < pos0 + m_max - W + 1: some row's window starts above the block's first key; adds the compare
//                             key >= my_limit - W + 1. P = 0 then multiplies real, finite, stale V^T: nothing is zeroed.
//                 interior    no compare at all (and no -inf tests in the softmax update)
//                 upper edge  key0 + 31 > min(pos0 + m_min, n_keys - 1): the causal compare key <= my_limit && key < n_keys
//               A block may be both edges (W short, or the row shorter than W) and then takes both compares.
//   split-KV    follows the span, not the row: s_eff = min(n_split, ceil((n_blocks - b_lo) / 16)), the waves' round-robin starts
//               at b_lo, and the host sizes n_split from min(l_max, W + M) (attention_window_plan): a 32 K cache under a 4 K
//               window launches 8-way, not 32-way.
//   paged       the page lookup of a block is attention_tile's; only the first block index differs.
// The wave merge through LDS and the split hand-over (agent-scope relaxed partials, one release / acquire arrival per workgroup)
// are restated from attention_tile, whose code stays as it is: see the notes there.
//
// The tiled prompt kernel's window variant is a template parameter of attention_prefill_kernel (attention_prefill.hip).
//
// Resources (hipcc --save-temps, gfx950, 4 waves; no instance uses scratch):
//   attention_window_kernel  D = 128 dense: 168 unified registers, 51 SGPRs; D = 128 paged: 160, 88 SGPRs: three waves per SIMD;
//                            D = 64 dense: 96, 51 SGPRs; D = 64 paged: 104, 90 SGPRs.
//   attention_prefill_kernel, WIN, D = 128: 252 registers with 4 waves, 214 with 8 (dense and paged alike; the plain instances:
//                            252 and 215), 48 / 57 SGPRs dense / paged; D = 64: 160 and 133.
// Built with packed fp32 VALU operations off (build.py), as the other attention files that rescale accumulator pairs.

#include <stdlib.h>

#include "attention_device.h"

namespace sd {

namespace {

constexpr int kWinWaves = 4, kWinThreads = kWinWaves * 64;

// One 32-key block for one wave. LO / UP: the block is a lower / upper edge of the tile (see above). kc / vt: the dense slab of
// (row, kv head); a paged block finds its page itself.
template <int D, bool PAGED, bool LO, bool UP>
__device__ __forceinline__ void win_block(const AttnArgs& a, const u32x4 (&qf)[D / 32], const uint16_t* kc, const uint16_t* vt, int vstride, int b,
                                          int kvh, int blk, int n_keys, int my_limit, int my_lo, int g, int n, f32x4_t (&oacc)[D / 16],
                                          float& m_run, float& l_run) {
  constexpr int NKS = D / 32, NDT = D / 16;
  const int key0 = blk * kAttnBlock;
  int kbase = key0;                       // position of the block's first key inside its slab
  if constexpr (PAGED) {
    const int pg = __builtin_amdgcn_readfirstlane(a.block_table[b * (a.l_max >> a.page_shift) + (key0 >> a.page_shift)]);
    kc = static_cast<const uint16_t*>(a.k_cache) + ((static_cast<size_t>(pg) * a.n_kv_heads + kvh) << a.page_shift) * D;
    vt = static_cast<const uint16_t*>(a.v_cache) + ((static_cast<size_t>(pg) * a.n_kv_heads + kvh) * D << a.page_shift);
    kbase = key0 & (vstride - 1);
  }
  // ---- issue every load of the block: S^T tile u, MFMA row i (= lane n) is key key0 + 8 (i >> 2) + 4 u + (i & 3)
  u32x4 kf[2][NKS];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    int key = kbase + 8 * (n >> 2) + 4 * u + (n & 3);
    if (!PAGED && key >= a.l_max) key = a.l_max - 1;  // stay inside the cache; masked below (a page holds the whole block)
    const uint16_t* krow = kc + static_cast<size_t>(key) * D + g * 8;
#pragma unroll
    for (int s = 0; s < NKS; ++s) kf[u][s] = *reinterpret_cast<const u32x4*>(krow + s * 32);
  }
  // V^T fragment of channel tile i: lane (g, n) holds V^T[16 i + n][key0 + 8 g .. +8]
  u32x4 vf[NDT];
  {
    int kofs = kbase + 8 * g;
    if (!PAGED && kofs + 8 > a.l_max) kofs = a.l_max - 8;  // l_max % 8 == 0 (checked by the host)
    const uint16_t* vrow = vt + static_cast<size_t>(n) * vstride + kofs;
#pragma unroll
    for (int i = 0; i < NDT; ++i) vf[i] = *reinterpret_cast<const u32x4*>(vrow + static_cast<size_t>(16 * i) * vstride);
  }
  // ---- S^T = K Q^T
  f32x4_t st[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    st[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NKS; ++s)
      st[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, kf[u][s]), __builtin_bit_cast(bf16x8_t, qf[s]), st[u], 0, 0, 0);
  }
  // lane (g, n) now holds, for query row n, the scores of keys key0 + 8 g + (4 u + r)
  float sc[8];
  float mx = -INFINITY;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = st[u][r] * a.scale;
      if constexpr (LO || UP) {
        const int key = key0 + 8 * g + 4 * u + r;
        bool vis = true;
        if constexpr (LO) vis = key >= my_lo;
        if constexpr (UP) vis = vis && (key <= my_limit) && (key < n_keys);
        v = vis ? v : -INFINITY;
      }
      sc[4 * u + r] = v;
      mx = fmaxf(mx, v);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float m_new = fmaxf(m_run, mx);
  float alpha, psum = 0.f;
  float p[8];
  if constexpr (LO || UP) {
    // a row may see nothing of an edge block, and nothing so far
    alpha = (m_run > -INFINITY) ? __expf(m_run - m_new) : 0.f;   // (nothing so far: O and l are zero)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      p[j] = (sc[j] > -INFINITY) ? __expf(sc[j] - m_new) : 0.f;
      psum += p[j];
    }
  } else {
    alpha = __expf(m_run - m_new);    // every score is finite; m_run = -inf at a wave's first block: 0
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      p[j] = __expf(sc[j] - m_new);
      psum += p[j];
    }
  }
  psum += __shfl_xor(psum, 16, 64);
  psum += __shfl_xor(psum, 32, 64);
  l_run = l_run * alpha + psum;
  m_run = m_new;
  // P as the A operand: lane (g, n = q) holds P[q][key0 + 8 g + j], j = 0..7
  const u32x4 pf = {pack_bf16x2(p[0], p[1]), pack_bf16x2(p[2], p[3]), pack_bf16x2(p[4], p[5]), pack_bf16x2(p[6], p[7])};
  // rescale O: lane (g, n = d) holds O[q = 4 g + r][d]; alpha of row q lives in lane q
  float al[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) al[r] = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
  for (int i = 0; i < NDT; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) oacc[i][r] *= al[r];
    oacc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, pf), __builtin_bit_cast(bf16x8_t, vf[i]), oacc[i], 0, 0, 0);
  }
}

}  // namespace

// grid = (n_kv_heads, B, tiles * n_split); block = 256; dynamic LDS = attention_smem_bytes(D, 4)
template <int D, bool PAGED>
__global__ __launch_bounds__(kWinThreads) void attention_window_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NKS = D / 32, NDT = D / 16;
  const int ns = a.n_split > 1 ? a.n_split : 1;
  const int kvh = blockIdx.x, b = blockIdx.y, tile = blockIdx.z / ns, split = blockIdx.z % ns;
  const int G = a.n_q_heads / a.n_kv_heads, M = a.M, W = a.window;
  const int R = G * M;
  const int r_base = tile * kAttnRows;
  const int rows = min(kAttnRows, R - r_base);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, n = lane & 15;

  float* o_s = reinterpret_cast<float*>(smem);            // [waves][16][D]
  float* m_s = o_s + kWinWaves * kAttnRows * D;           // [waves][16]
  float* l_s = m_s + kWinWaves * kAttnRows;               // [waves][16]

  SD_SKIP_IF_INACTIVE(a.skip_k, a.skip_i);
  const int pos0 = a.pos_base[b] + a.pos_off;             // position of query m = 0
  const int n_keys = max(0, min(pos0 + M, a.l_max));      // keys visible to the last query
  const int n_blocks = (n_keys + kAttnBlock - 1) / kAttnBlock;
  // the tile's rows are query indices [m_min, m_max] (a tile that crosses a head boundary holds m = M - 1 and m = 0)
  const int gh0 = r_base / M, gh1 = (r_base + rows - 1) / M;
  const int m_min = gh0 == gh1 ? r_base - gh0 * M : 0;
  const int m_max = gh0 == gh1 ? r_base + rows - 1 - gh0 * M : M - 1;
  const int b_lo = max(0, pos0 + m_min - W + 1) / kAttnBlock;                          // first block any row of the tile sees
  const int lo_end = (max(0, pos0 + m_max - W + 1) + kAttnBlock - 1) / kAttnBlock;     // blocks below it hold some row's window start
  const int up_begin = max(0, min(pos0 + m_min, n_keys - 1) + 1) / kAttnBlock;         // blocks from it on reach past some row's last key
  int s_eff = 1;
  if (a.n_split > 1) {
    s_eff = min(static_cast<int>(a.n_split), max(1, (n_blocks - b_lo + kAttnSplitBlocks - 1) / kAttnSplitBlocks));
    if (split >= s_eff) return;  // workgroup-uniform, before any barrier
  }

  // ---- Q fragments: lane (g, n) holds Q[row n][32 s + 8 g .. +8] for s < NKS
  const int qstride = a.n_q_heads * D;
  u32x4 qf[NKS];
  int my_m = 0;
  {
    const uint16_t* q = static_cast<const uint16_t*>(a.q);
    const bool valid = n < rows;
    const int rr = r_base + (valid ? n : 0);
    const int gh = rr / M, m = rr - gh * M;
    my_m = m;
    const uint16_t* qrow = q + static_cast<size_t>(b * M + m) * qstride + (kvh * G + gh) * D + g * 8;
#pragma unroll
    for (int s = 0; s < NKS; ++s) {
      if (valid) qf[s] = *reinterpret_cast<const u32x4*>(qrow + s * 32);
      else qf[s] = u32x4{0u, 0u, 0u, 0u};
    }
  }
  const uint16_t* kc = static_cast<const uint16_t*>(a.k_cache) + (static_cast<size_t>(b) * a.n_kv_heads + kvh) * a.l_max * D;
  const uint16_t* vt = static_cast<const uint16_t*>(a.v_cache) + (static_cast<size_t>(b) * a.n_kv_heads + kvh) * D * a.l_max;
  const int vstride = PAGED ? (1 << a.page_shift) : a.l_max;   // positions per V^T row

  f32x4_t oacc[NDT];
#pragma unroll
  for (int i = 0; i < NDT; ++i) oacc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;  // for query row n (replicated over g)
  const int my_limit = pos0 + my_m;      // last key this lane's query may see
  const int my_lo = my_limit - W + 1;    // and the first

  for (int blk = b_lo + split * kWinWaves + wave; blk < n_blocks; blk += kWinWaves * s_eff) {
    const bool lo = blk < lo_end, up = blk >= up_begin;
    if (lo && up) win_block<D, PAGED, true, true>(a, qf, kc, vt, vstride, b, kvh, blk, n_keys, my_limit, my_lo, g, n, oacc, m_run, l_run);
    else if (lo) win_block<D, PAGED, true, false>(a, qf, kc, vt, vstride, b, kvh, blk, n_keys, my_limit, my_lo, g, n, oacc, m_run, l_run);
    else if (up) win_block<D, PAGED, false, true>(a, qf, kc, vt, vstride, b, kvh, blk, n_keys, my_limit, my_lo, g, n, oacc, m_run, l_run);
    else win_block<D, PAGED, false, false>(a, qf, kc, vt, vstride, b, kvh, blk, n_keys, my_limit, my_lo, g, n, oacc, m_run, l_run);
  }

  // ---- merge the 4 waves (as attention_tile)
  if (g == 0) {
    m_s[wave * kAttnRows + n] = m_run;
    l_s[wave * kAttnRows + n] = l_run;
  }
#pragma unroll
  for (int i = 0; i < NDT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) o_s[(wave * kAttnRows + 4 * g + r) * D + 16 * i + n] = oacc[i][r];
  __syncthreads();
  uint16_t* out = static_cast<uint16_t*>(a.out);
  if (s_eff > 1) {
    // ---- partial of this workgroup -> workspace; the last arrival merges all s_eff partials. The workspace is only ever touched
    // with agent-scope relaxed atomics; the hand-over is ordered by thread 0's release / acquire arrival (see attention_tile).
    const int tiles = (R + kAttnRows - 1) / kAttnRows;
    const int group = (b * a.n_kv_heads + kvh) * tiles + tile;
    constexpr int PS = kAttnRows * (D + 2);  // floats per partial: O[16][D], max[16], sum[16]
    float* mine = a.split_ws + (static_cast<size_t>(group) * a.n_split + split) * PS;
    for (int i = tid; i < kAttnRows * D; i += kWinThreads) {
      const int r = i / D, d = i - r * D;
      float mm = -INFINITY;
#pragma unroll
      for (int w = 0; w < kWinWaves; ++w) mm = fmaxf(mm, m_s[w * kAttnRows + r]);
      float num = 0.f, den = 0.f;
#pragma unroll
      for (int w = 0; w < kWinWaves; ++w) {
        const float mw = m_s[w * kAttnRows + r];
        const float f = (mw > -INFINITY) ? __expf(mw - mm) : 0.f;
        num += f * o_s[(w * kAttnRows + r) * D + d];
        den += f * l_s[w * kAttnRows + r];
      }
      __hip_atomic_store(mine + i, num, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (d == 0) {
        __hip_atomic_store(mine + kAttnRows * D + r, mm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(mine + kAttnRows * D + kAttnRows + r, den, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    __syncthreads();
    unsigned* flag = reinterpret_cast<unsigned*>(m_s);  // LDS scratch (m_s is dead after the loop above)
    if (tid == 0) {
      const unsigned old = __hip_atomic_fetch_add(a.split_cnt + group, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      const bool last = (old == static_cast<unsigned>(s_eff - 1));
      *flag = last ? 1u : 0u;
      if (last) __hip_atomic_store(a.split_cnt + group, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
    }
    __syncthreads();
    if (*flag == 0u) return;
    const float* base = a.split_ws + static_cast<size_t>(group) * a.n_split * PS;
    float* pm = o_s;                              // [s_eff][16] max   (o_s is dead: the partial has been written)
    float* pl = o_s + kAttnMaxSplit * kAttnRows;  // [s_eff][16] sum
    for (int i = tid; i < s_eff * kAttnRows; i += kWinThreads) {
      const int sidx = i / kAttnRows, r = i - sidx * kAttnRows;
      pm[i] = __hip_atomic_load(base + static_cast<size_t>(sidx) * PS + kAttnRows * D + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      pl[i] = __hip_atomic_load(base + static_cast<size_t>(sidx) * PS + kAttnRows * D + kAttnRows + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    constexpr int CPR = D / 8;                 // 8-channel chunks per row
    for (int c = tid; c < rows * CPR; c += kWinThreads) {
      const int r = c / CPR, d0 = (c - r * CPR) * 8;
      float mm = -INFINITY;
      for (int sidx = 0; sidx < s_eff; ++sidx) mm = fmaxf(mm, pm[sidx * kAttnRows + r]);
      float num[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      float den = 0.f;
      const float* src = base + r * D + d0;
#pragma unroll 4
      for (int sidx = 0; sidx < s_eff; ++sidx) {
        const float4 v0 = coherent_load_f4(src + static_cast<size_t>(sidx) * PS);
        const float4 v1 = coherent_load_f4(src + static_cast<size_t>(sidx) * PS + 4);
        const float ms = pm[sidx * kAttnRows + r];
        const float f = (ms > -INFINITY) ? __expf(ms - mm) : 0.f;
        den += f * pl[sidx * kAttnRows + r];
        num[0] += f * v0.x; num[1] += f * v0.y; num[2] += f * v0.z; num[3] += f * v0.w;
        num[4] += f * v1.x; num[5] += f * v1.y; num[6] += f * v1.z; num[7] += f * v1.w;
      }
      const float inv = (den > 0.f) ? 1.0f / den : 0.f;
      const int rr = r_base + r, gh = rr / M, m = rr - gh * M;
      uint16_t* dst = out + static_cast<size_t>(b * M + m) * qstride + (kvh * G + gh) * D + d0;
      const u32x4 o = {pack_bf16x2(num[0] * inv, num[1] * inv), pack_bf16x2(num[2] * inv, num[3] * inv),
                       pack_bf16x2(num[4] * inv, num[5] * inv), pack_bf16x2(num[6] * inv, num[7] * inv)};
      *reinterpret_cast<u32x4*>(dst) = o;
    }
    return;
  }
  for (int i = tid; i < rows * D; i += kWinThreads) {
    const int r = i / D, d = i - r * D;
    float mm = -INFINITY;
#pragma unroll
    for (int w = 0; w < kWinWaves; ++w) mm = fmaxf(mm, m_s[w * kAttnRows + r]);
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < kWinWaves; ++w) {
      const float mw = m_s[w * kAttnRows + r];
      const float f = (mw > -INFINITY) ? __expf(mw - mm) : 0.f;
      num += f * o_s[(w * kAttnRows + r) * D + d];
      den += f * l_s[w * kAttnRows + r];
    }
    const int rr = r_base + r, gh = rr / M, m = rr - gh * M;
    out[static_cast<size_t>(b * M + m) * qstride + (kvh * G + gh) * D + d] = float_to_bf16_bits((den > 0.f) ? num / den : 0.f);
  }
}

// The plan of such a launch: attention_plan's checks and tiles, n_split from the span a tile can walk instead of the whole row.
int attention_window_plan(int n_q_heads, int n_kv_heads, int head_dim, int B, int M, int l_max, int page_shift, bool has_split_ws,
                          int split_slots, int W, AttnWindowPlan& plan) {
  SD_REQUIRE(W >= 1, "attention_window: sliding_window W=%d (>= 1; 0 is the plain launch)", W);
  SD_REQUIRE(head_dim == 64 || head_dim == 128, "attention_window: sliding_window covers head_dim 64 and 128 only (got %d)", head_dim);
  SD_REQUIRE(M <= kSkinnyMaxT, "attention_window: M=%d (a launch holds 1 .. %d positions per row)", M, kSkinnyMaxT);
  AttnPlan base{};
  if (int rc = attention_plan(n_q_heads, n_kv_heads, head_dim, B, M, l_max, page_shift, false, 0, base)) return rc;
  const long long reach = static_cast<long long>(W) + M;          // keys between a tile's first window start and the launch's last key
  const int span = reach < l_max ? static_cast<int>(reach) : l_max;
  const int wgs = n_kv_heads * B * base.tiles;
  int ns = 1;
  if (has_split_ws && !getenv(debug_env::kNoAttnSplit)) {
    ns = span / (kAttnBlock * kAttnSplitBlocks);
    if (ns > kAttnMaxSplit) ns = kAttnMaxSplit;
    if (ns > split_slots / wgs) ns = split_slots / wgs;
    if (ns > 512 / wgs) ns = 512 / wgs;
    if (ns < 1) ns = 1;
  }
  plan.attn = AttnPlan{base.tiles, ns, n_kv_heads, B, base.tiles * ns};
  // span - 1 consecutive keys (the first tile's: m_min = 0) touch at most this many 32-key blocks, and never more than the row has
  const int row_blocks = (l_max + kAttnBlock - 1) / kAttnBlock;
  const int walk = (span - 1 + kAttnBlock - 2) / kAttnBlock + 1;
  plan.max_blocks = walk < row_blocks ? walk : row_blocks;
  return 0;
}

template <int D>
static void launch_window_d(const AttnArgs& a, dim3 grid, hipStream_t st) {
  const size_t smem = attention_smem_bytes(D, kWinWaves);   // (<= 33 KiB of LDS)
  if (a.block_table) hipLaunchKernelGGL((attention_window_kernel<D, true>), grid, dim3(kWinThreads), smem, st, a);
  else hipLaunchKernelGGL((attention_window_kernel<D, false>), grid, dim3(kWinThreads), smem, st, a);
}

int launch_attention_window(const AttnArgs& a_in, hipStream_t st) {
  AttnArgs a = a_in;
  SD_REQUIRE(!a.kv8, "attention_window: sliding_window reads bf16 caches, not an fp8 (e4m3) kv dtype");
  SD_REQUIRE(!a.share, "attention_window: sliding_window is not available with cascade attention");
  AttnWindowPlan pl{};
  if (int rc = attention_window_plan(a.n_q_heads, a.n_kv_heads, a.head_dim, a.B, a.M, a.l_max, a.block_table ? static_cast<int>(a.page_shift) : -1,
                                     a.split_ws && a.split_cnt, a.split_slots, a.window, pl))
    return rc;
  a.n_split = pl.attn.n_split;
  const dim3 grid(pl.attn.grid_x, pl.attn.grid_y, pl.attn.grid_z);
  if (a.head_dim == 64) launch_window_d<64>(a, grid, st);
  else launch_window_d<128>(a, grid, st);
  SD_LAUNCH_CHECK();
  return 0;
}

}  // namespace sd
