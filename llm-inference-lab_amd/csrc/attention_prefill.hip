// Prompt attention: the attention of one GEMM-prefill chunk (csrc/prefill_gemm.hip, step 2 of the layer loop) as ONE launch over all
// of its <= 512 query positions, with K / V staged through LDS once per tile of query rows (sd_model_set_prefill_attention).
//
// What it replaces. The decode / verify kernel (attention.hip) makes a workgroup of 16 query rows whose four waves split the keys and
// load their K / V^T fragments straight from L2 / HBM: a 128-position sub-pass at G = Hq / Hkv = 3 reads the slab of a kv head 24
// times. Here the work is split the other way:
//   workgroup   one (kv head, tile of PT consecutive query positions x all G query heads of the kv head). Row r of the workgroup is
//               (head gh = r / PT, position p0 + r % PT); wave w owns rows [16 w, 16 w + 16), one MFMA tile. PT is 16 or 32
//               (attention_prefill_plan), so a wave's rows are one head's consecutive positions and all rows of a workgroup lie
//               within PT positions: the causal limit of the tile is nearly uniform. Rows past G * PT or past the chunk's end carry
//               zero Q and are never stored.
//   key loop    every wave walks the SAME 64-key blocks in order: no per-wave key split, no merge of partials. A block's K rows
//               [64][D] and V^T rows [D][64] are staged into LDS once per workgroup by all of its threads (a plain global -> register
//               -> LDS copy in 16-byte pieces; LDS-DMA was not tried: one wave instruction writes 1 KiB contiguously from M0, so the
//               padded rows below would take an instruction per row, or a swizzle in place of the padding). Two LDS buffers: the global loads of block i + 1 are issued before the MFMAs of block i and
//               land in the other buffer after them, one barrier per block.
//   LDS layout  K rows are stored in MFMA order — LDS row 16 t + i holds the key that row i of S^T tile t stands for — with rows of
//               D + 8 elements; V^T rows have 64 + 8 elements. The 16 bytes of padding make the row stride 4 (mod 8) dwords, so the
//               16 lanes of a lane group, which read the same 16-byte column of 16 consecutive rows, start 4 dwords apart modulo the
//               64 banks (D = 128: 68 n; D = 64 and V^T: 36 n, a permutation of the multiples of 4): no two of them share a bank.
//   arithmetic  the layout of attention_tile, which needs no shuffle for P: S^T = K Q^T (v_mfma_f32_16x16x32_bf16, K the A operand, Q
//               fragments in registers), tile t = 2 h + u of a block holds keys 32 h + 8 (i >> 2) + 4 u + (i & 3), so lane (g, n)
//               ends with the 16 scores of query row n for keys 32 h + 8 g + 0..7, h = 0, 1; online softmax in fp32 (__expf); P
//               rounded to bf16 once and used as the A operand of P V.
//   causality   a workgroup walks blocks 0 .. floor(last position of its tile / 64). Blocks wholly at or below the tile's first
//               position take the unmasked instantiation of the block body; only the <= 2 diagonal blocks compare keys with
//               positions. The grid runs the tiles in reverse, so the launch ends with the short ones.
//   loads       a 64-key block is staged as two 32-key halves (a page holds 32 * 2^n positions: each half has its own table read). A
//               half that starts beyond the tile's last key re-reads the half of that key instead (its table entry may name no page);
//               dense rows and V^T pieces are clamped inside l_max as in attention_tile. What such a load returns stands for a key
//               beyond the tile's last: its score is masked, and its V^T elements are zeroed while staging (0 x NaN is NaN).
// Launched with 4 or 8 waves; waves beyond the tile's row count only stage. bf16 caches, dense or paged; head_dim 64 and 128.
//
// Sliding window (WIN instances; sd_model_set_sliding_window, see attention_window.hip for the decode-shaped kernel): position p sees
// keys max(0, p - W + 1) .. p. The block walk starts at max(0, first - W + 1) / 64 — blocks below it are never staged — and a block
// that holds some row's window start (key0 < last - W + 1) takes a lower-edge instantiation of the block body, which adds the compare
// key >= my_limit - W + 1; a tile of 16 positions under W >= 64 meets at most two of them. A block can be lower edge and diagonal at
// once (W < 64 or a window not yet full): the doubly masked instantiation. Keys of a staged block below a row's window are real,
// finite, stale: P = 0 there and nothing is zeroed. Resources of the D = 128 WIN instances (hipcc --save-temps, gfx950): see the
// header of attention_window.hip.

#include "attention_device.h"
#include "prefill_gemm.h"

namespace sd {

namespace {

constexpr int kPfBlock = 64;     // keys per block
constexpr int kPfPad = 8;        // elements of padding per LDS row (16 bytes)
constexpr int kPfCUs = 256;      // workgroups a launch should reach before PT grows to 32

template <int D>
struct PfLds {
  static constexpr int KS = D + kPfPad;               // elements per K row
  static constexpr int VS = kPfBlock + kPfPad;        // elements per V^T row
  static constexpr int K_ELEMS = kPfBlock * KS, V_ELEMS = D * VS;
  static constexpr int BUF = K_ELEMS + V_ELEMS;       // elements per buffer
  static constexpr int BYTES = 2 * BUF * 2;
};

// One 64-key block for one wave: S^T, softmax update, P V. kb / vb: the block's LDS buffers. MASK: compare keys with positions.
// LOW: a lower edge of a windowed tile, compare keys with the row's window start my_lo as well.
template <int D, bool MASK, bool LOW = false>
__device__ __forceinline__ void pf_block(const uint16_t* kb, const uint16_t* vb, const u32x4 (&qf)[D / 32], int key0, int my_limit, float scale,
                                         int g, int n, f32x4_t (&oacc)[D / 16], float& m_run, float& l_run, int my_lo = 0) {
  constexpr int NKS = D / 32, NDT = D / 16;
  constexpr int KS = PfLds<D>::KS, VS = PfLds<D>::VS;
  f32x4_t st[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    st[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const uint16_t* krow = kb + (16 * t + n) * KS + 8 * g;
#pragma unroll
    for (int s = 0; s < NKS; ++s) {
      const u32x4 kf = *reinterpret_cast<const u32x4*>(krow + 32 * s);
      st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, kf), __builtin_bit_cast(bf16x8_t, qf[s]), st[t], 0, 0, 0);
    }
  }
  // lane (g, n): query row n, sc[8 h + 4 u + r] = key key0 + 32 h + 8 g + 4 u + r
  float sc[16];
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = st[t][r] * scale;
      if constexpr (MASK) {
        const int key = key0 + 32 * (t >> 1) + 8 * g + 4 * (t & 1) + r;
        v = (key <= my_limit) ? v : -INFINITY;
      }
      if constexpr (LOW) {
        const int key = key0 + 32 * (t >> 1) + 8 * g + 4 * (t & 1) + r;
        v = (key >= my_lo) ? v : -INFINITY;
      }
      sc[4 * t + r] = v;
      mx = fmaxf(mx, v);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float m_new = fmaxf(m_run, mx);
  float alpha, psum = 0.f;
  float p[16];
  if constexpr (MASK || LOW) {
    // a row may see nothing of a diagonal block (never of block 0: key 0 is visible to every position), nor of a lower-edge one
    alpha = (m_run > -INFINITY) ? __expf(m_run - m_new) : 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      p[j] = (sc[j] > -INFINITY) ? __expf(sc[j] - m_new) : 0.f;
      psum += p[j];
    }
  } else {
    alpha = __expf(m_run - m_new);    // m_run = -inf at the first block: 0
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      p[j] = __expf(sc[j] - m_new);
      psum += p[j];
    }
  }
  psum += __shfl_xor(psum, 16, 64);
  psum += __shfl_xor(psum, 32, 64);
  l_run = l_run * alpha + psum;
  m_run = m_new;
  u32x4 pf[2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
    pf[h] = u32x4{pack_bf16x2(p[8 * h], p[8 * h + 1]), pack_bf16x2(p[8 * h + 2], p[8 * h + 3]), pack_bf16x2(p[8 * h + 4], p[8 * h + 5]),
                  pack_bf16x2(p[8 * h + 6], p[8 * h + 7])};
  // lane (g, n = d) holds O[q = 4 g + r][d]; alpha of row q lives in lane q
  float al[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) al[r] = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
  for (int i = 0; i < NDT; ++i) {
    const uint16_t* vrow = vb + (16 * i + n) * VS + 8 * g;
#pragma unroll
    for (int r = 0; r < 4; ++r) oacc[i][r] *= al[r];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const u32x4 vf = *reinterpret_cast<const u32x4*>(vrow + 32 * h);
      oacc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, pf[h]), __builtin_bit_cast(bf16x8_t, vf), oacc[i], 0, 0, 0);
    }
  }
}

// NWT: waves launched (4 or 8). grid = (n_kv_heads, tiles); block = NWT * 64; dynamic LDS = PfLds<D>::BYTES. WIN: a.window >= 1.
template <int D, bool PAGED, int NWT, bool WIN = false>
__global__ __launch_bounds__(NWT * 64) void attention_prefill_kernel(const PrefillAttnArgs a) {
  constexpr int NT = NWT * 64, NKS = D / 32, NDT = D / 16;
  using L = PfLds<D>;
  constexpr int CH = kPfBlock * D / 8;       // 16-byte pieces of a block's K rows, and as many of its V^T rows
  constexpr int CPT = CH / NT;               // of each per thread
  static_assert(CH % NT == 0 && CPT >= 1, "the block's pieces divide among the threads");
  extern __shared__ __attribute__((aligned(16))) unsigned char pf_smem[];
  uint16_t* lds = reinterpret_cast<uint16_t*>(pf_smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, n = lane & 15;
  const int kvh = blockIdx.x;
  const int tile = static_cast<int>(gridDim.y) - 1 - static_cast<int>(blockIdx.y);   // heavy tiles first
  const int G = a.n_q_heads / a.n_kv_heads, PT = a.pt;
  const int p0 = tile * PT;
  const int pn = min(PT, a.Mc - p0);                       // positions of this tile
  const int pos0 = a.pos_base[0] + a.pos_off;              // position of the chunk's first query
  const int first = pos0 + p0;
  const int last = min(first + pn, a.l_max) - 1;           // the tile's last key
  if (last < 0) return;
  const int n_blocks = last / kPfBlock + 1;
  const int blk_lo = WIN ? max(0, first - a.window + 1) / kPfBlock : 0;   // first block any row of the tile sees
  const int lo_max = WIN ? last - a.window + 1 : 0;                       // the latest window start among the tile's rows
  const int HqD = a.n_q_heads * D;

  // ---- this wave's rows: Q fragments, lane (g, n) holds Q[row n][32 s + 8 g .. +8]
  const bool computes = wave * 16 < G * PT;
  u32x4 qf[NKS];
  int my_limit = last;
  {
    const int r = wave * 16 + n, gh = r / PT, p = r - gh * PT;
    const bool valid = gh < G && p < pn;
    const uint16_t* qrow = static_cast<const uint16_t*>(a.q) + static_cast<size_t>(p0 + (valid ? p : 0)) * HqD + (kvh * G + (valid ? gh : 0)) * D + 8 * g;
#pragma unroll
    for (int s = 0; s < NKS; ++s) qf[s] = valid ? *reinterpret_cast<const u32x4*>(qrow + 32 * s) : u32x4{0u, 0u, 0u, 0u};
    if (valid) my_limit = min(first + p, last);
  }
  f32x4_t oacc[NDT];
#pragma unroll
  for (int i = 0; i < NDT; ++i) oacc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  // ---- staging: piece c = tid + j * NT of the block's K rows (key c / (D / 8), 8 channels) and of its V^T rows (channel c / 8, 8 keys)
  const int P = PAGED ? (1 << a.page_shift) : a.l_max;     // positions per V^T row
  const uint16_t* kslab = static_cast<const uint16_t*>(a.k_cache) + static_cast<size_t>(kvh) * a.l_max * D;   // dense
  const uint16_t* vslab = static_cast<const uint16_t*>(a.v_cache) + static_cast<size_t>(kvh) * D * a.l_max;
  u32x4 rk[CPT], rv[CPT];
  auto fetch = [&](int blk) {
    const int key0 = blk * kPfBlock;
    // the two halves: where each is read (a half beyond the tile's last key re-reads that key's half) and, paged, its page
    int hs[2];
    const uint16_t *kh[2], *vh[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      hs[h] = (key0 + 32 * h <= last) ? key0 + 32 * h : (last & ~31);
      if constexpr (PAGED) {
        const int pg = __builtin_amdgcn_readfirstlane(a.block_table[hs[h] >> a.page_shift]);
        kh[h] = static_cast<const uint16_t*>(a.k_cache) + ((static_cast<size_t>(pg) * a.n_kv_heads + kvh) << a.page_shift) * D;
        vh[h] = static_cast<const uint16_t*>(a.v_cache) + ((static_cast<size_t>(pg) * a.n_kv_heads + kvh) * D << a.page_shift);
        hs[h] &= P - 1;                                    // position inside the page
      } else {
        kh[h] = kslab;
        vh[h] = vslab;
      }
    }
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      const int c = tid + j * NT;
      {
        const int kr = c / (D / 8), cc = c - kr * (D / 8), h = kr >> 5;
        int key = hs[h] + (kr & 31);
        if (!PAGED && key >= a.l_max) key = a.l_max - 1;   // (a page holds the whole half)
        rk[j] = *reinterpret_cast<const u32x4*>(kh[h] + static_cast<size_t>(key) * D + 8 * cc);
      }
      {
        const int d = c >> 3, vc = c & 7, h = vc >> 2;
        int kofs = hs[h] + 8 * (vc & 3);
        if (!PAGED && kofs + 8 > a.l_max) kofs = a.l_max - 8;   // l_max % 8 == 0
        u32x4 v = *reinterpret_cast<const u32x4*>(vh[h] + static_cast<size_t>(d) * P + kofs);
        const int n_ok = last + 1 - (key0 + 8 * vc);      // elements of the piece that stand for keys of the tile
        if (n_ok < 8) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const uint32_t keep = (2 * e + 1 < n_ok) ? 0xffffffffu : (2 * e < n_ok) ? 0x0000ffffu : 0u;
            v[e] &= keep;
          }
        }
        rv[j] = v;
      }
    }
  };
  auto stage = [&](int buf) {
    uint16_t* kb = lds + buf * L::BUF;
    uint16_t* vb = kb + L::K_ELEMS;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      const int c = tid + j * NT;
      const int kr = c / (D / 8), cc = c - kr * (D / 8), w = kr & 31;
      const int row = 16 * (2 * (kr >> 5) + ((w >> 2) & 1)) + 4 * (w >> 3) + (w & 3);   // MFMA order
      *reinterpret_cast<u32x4*>(kb + row * L::KS + 8 * cc) = rk[j];
      *reinterpret_cast<u32x4*>(vb + (c >> 3) * L::VS + 8 * (c & 7)) = rv[j];
    }
  };

  fetch(blk_lo);
  stage(0);
  __syncthreads();
  for (int blk = blk_lo; blk < n_blocks; ++blk) {
    const int buf = (blk - blk_lo) & 1;
    if (blk + 1 < n_blocks) fetch(blk + 1);               // in flight during the MFMAs below
    if (computes) {
      const uint16_t* kb = lds + buf * L::BUF;
      const uint16_t* vb = kb + L::K_ELEMS;
      const int key0 = blk * kPfBlock;
      if constexpr (WIN) {
        const bool low = key0 < lo_max, diag = key0 + kPfBlock - 1 > first;   // workgroup-uniform
        const int my_lo = my_limit - a.window + 1;
        if (low && diag) pf_block<D, true, true>(kb, vb, qf, key0, my_limit, a.scale, g, n, oacc, m_run, l_run, my_lo);
        else if (low) pf_block<D, false, true>(kb, vb, qf, key0, my_limit, a.scale, g, n, oacc, m_run, l_run, my_lo);
        else if (diag) pf_block<D, true>(kb, vb, qf, key0, my_limit, a.scale, g, n, oacc, m_run, l_run);
        else pf_block<D, false>(kb, vb, qf, key0, my_limit, a.scale, g, n, oacc, m_run, l_run);
      } else if (key0 + kPfBlock - 1 <= first) pf_block<D, false>(kb, vb, qf, key0, my_limit, a.scale, g, n, oacc, m_run, l_run);
      else pf_block<D, true>(kb, vb, qf, key0, my_limit, a.scale, g, n, oacc, m_run, l_run);
    }
    if (blk + 1 < n_blocks) stage(buf ^ 1);               // last read before the previous barrier
    __syncthreads();
  }

  // ---- O / l: lane (g, n = d) holds O[q = 4 g + r][16 i + d]; l of row q lives in lane q
  if (!computes) return;
  uint16_t* out = static_cast<uint16_t*>(a.out);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float den = __shfl(l_run, 4 * g + r, 64);
    const int row = wave * 16 + 4 * g + r, gh = row / PT, p = row - gh * PT;
    if (gh >= G || p >= pn) continue;
    uint16_t* dst = out + static_cast<size_t>(p0 + p) * HqD + (kvh * G + gh) * D + n;
#pragma unroll
    for (int i = 0; i < NDT; ++i) dst[16 * i] = float_to_bf16_bits((den > 0.f) ? oacc[i][r] / den : 0.f);
  }
}

template <int D, bool PAGED, int NWT, bool WIN = false>
int launch_instance(const PrefillAttnArgs& a, const PrefillAttnPlan& pl, hipStream_t st) {
  static unsigned long long seen = 0;
  const void* fn = reinterpret_cast<const void*>(&attention_prefill_kernel<D, PAGED, NWT, WIN>);
  if (int rc = opt_in_dynamic_lds(fn, PfLds<D>::BYTES, seen)) return rc;
  hipLaunchKernelGGL((attention_prefill_kernel<D, PAGED, NWT, WIN>), dim3(a.n_kv_heads, pl.tiles), dim3(NWT * 64), PfLds<D>::BYTES, st, a);
  SD_LAUNCH_CHECK();
  return 0;
}

template <int D>
int launch_d(const PrefillAttnArgs& a, const PrefillAttnPlan& pl, hipStream_t st) {
  const bool paged = a.block_table != nullptr;
  if (a.window > 0) {
    if (pl.threads == 256) return paged ? launch_instance<D, true, 4, true>(a, pl, st) : launch_instance<D, false, 4, true>(a, pl, st);
    return paged ? launch_instance<D, true, 8, true>(a, pl, st) : launch_instance<D, false, 8, true>(a, pl, st);
  }
  if (pl.threads == 256) return paged ? launch_instance<D, true, 4>(a, pl, st) : launch_instance<D, false, 4>(a, pl, st);
  return paged ? launch_instance<D, true, 8>(a, pl, st) : launch_instance<D, false, 8>(a, pl, st);
}

}  // namespace

const char* attention_prefill_refusal(int arch, int head_dim, int n_q_heads, int n_kv_heads, bool kv8) {
  if (arch != SD_ARCH_LLAMA) return "tiled prompt attention serves Llama models only (prompts of this model take the 128-token passes)";
  if (kv8) return "tiled prompt attention reads bf16 caches, not an fp8 (e4m3) kv dtype";
  if (head_dim != 64 && head_dim != 128) return "tiled prompt attention covers head_dim 64 and 128 only";
  if (n_kv_heads < 1 || n_q_heads % n_kv_heads != 0 || n_q_heads / n_kv_heads > 8)
    return "tiled prompt attention covers 1 to 8 query heads per kv head";
  return nullptr;
}

int attention_prefill_plan(int n_q_heads, int n_kv_heads, int head_dim, int Mc, int l_max, int page_shift, PrefillAttnPlan& plan) {
  SD_REQUIRE(n_q_heads >= 1 && n_kv_heads >= 1, "attention_prefill: Hq=%d Hkv=%d", n_q_heads, n_kv_heads);
  const char* why = attention_prefill_refusal(SD_ARCH_LLAMA, head_dim, n_q_heads, n_kv_heads, false);
  SD_REQUIRE(!why, "attention_prefill: %s (head_dim %d, Hq %d, Hkv %d)", why, head_dim, n_q_heads, n_kv_heads);
  SD_REQUIRE(Mc >= 1 && Mc <= kPrefillChunk, "attention_prefill: Mc=%d (a chunk holds 1 .. %d positions)", Mc, kPrefillChunk);
  SD_REQUIRE(l_max % 8 == 0 && l_max >= 8, "attention_prefill: l_max=%d must be a multiple of 8", l_max);
  SD_REQUIRE(page_shift < 0 || (page_shift >= 5 && page_shift <= 16 && l_max >= (1 << page_shift) && l_max % (1 << page_shift) == 0),
             "attention_prefill: paged cache needs pages of 32 * 2^n positions and l_max = max_pages * page_len");
  const int G = n_q_heads / n_kv_heads;
  // PT = 32 (up to 128 rows, each staged block feeds twice the MFMAs) only where that still gives every CU a workgroup; a single
  // 512-position chunk at 8 kv heads is 128 such tiles, so it takes PT = 16: 256 workgroups. From Hkv and the chunk's length alone.
  const int pt = (32 * G <= 128 && ((Mc + 31) / 32) * n_kv_heads >= kPfCUs) ? 32 : 16;
  plan.pt = pt;
  plan.rows_per_wg = (pt * G + 15) / 16 * 16;
  plan.waves = plan.rows_per_wg / 16;
  plan.threads = plan.waves <= 4 ? 256 : 512;
  plan.tiles = (Mc + pt - 1) / pt;
  plan.n_split = 1;      // a tile's keys are walked by one workgroup: nothing to merge, the split workspace is not touched
  plan.lds_bytes = head_dim == 64 ? PfLds<64>::BYTES : PfLds<128>::BYTES;
  return 0;
}

int attention_prefill_window_blocks(const PrefillAttnPlan& plan, int l_max, int W) {
  // W + pt - 1 consecutive keys at most (the first row's window start .. the tile's last key), and never more than the row has
  const long long reach = static_cast<long long>(W) + plan.pt - 1;
  const int keys = reach < l_max ? static_cast<int>(reach) : l_max;
  const int row_blocks = (l_max + kPfBlock - 1) / kPfBlock, walk = (keys + kPfBlock - 2) / kPfBlock + 1;
  return walk < row_blocks ? walk : row_blocks;
}

int launch_attention_prefill(const PrefillAttnArgs& a_in, hipStream_t st) {
  PrefillAttnArgs a = a_in;
  PrefillAttnPlan pl{};
  if (int rc = attention_prefill_plan(a.n_q_heads, a.n_kv_heads, a.head_dim, a.Mc, a.l_max, a.block_table ? a.page_shift : -1, pl)) return rc;
  SD_REQUIRE(a.q && a.k_cache && a.v_cache && a.out && a.pos_base, "attention_prefill: NULL argument");
  SD_REQUIRE(a.window >= 0, "attention_prefill: sliding_window W=%d is negative", a.window);
  a.pt = pl.pt;
  return a.head_dim == 64 ? launch_d<64>(a, pl, st) : launch_d<128>(a, pl, st);
}

}  // namespace sd
