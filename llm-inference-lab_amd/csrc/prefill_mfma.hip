// Prompt-prefill GEMM over the packed tile streams (the native backend of csrc/prefill_gemm.hip).
//
// Y[T][N] (fp32, row-major, true HF row order) = X[T][K] (bf16, rows ldx apart) x W^T, where W is ONE matrix's packed stream as
// pack_one_matrix left it (csrc/pack.hip): bf16, or OCP fp8 e4m3 with fp32 row scales. These are the bytes the decode kernels
// stream, so the prefill of an fp8 model multiplies the same dequantised values as its decode steps (the e4m3 values are widened
// to bf16, which is exact, and row r's fp32 accumulator is multiplied by scale[r] before the store, as gemm_pipe.hip does).
//
// The stream is a sequence of tiles of 2 * np rows (np <= 8 pairs, irregular: the decode kernels' work split, gemv_geometry).
// Each tile holds its whole K range contiguously, step after step: bf16 [32-k step][g = 0..3][row][16 B]; fp8 [64-k double
// step][g][row][16 B] with a lane's 16 bytes holding its fragments of two consecutive 32-k steps. So one 64-k stage of a tile is
// ONE contiguous piece of 2 * np * SB bytes (SB = 128 bf16, 64 fp8), and consecutive tiles' pieces concatenated are the
// stage's weight rows in packed order.
//
// Decomposition: a workgroup (4 waves, 2 x 2) owns RB = 64 or 128 consecutive packed rows (whole tiles: a host table per
// matrix shape, NativeMat) and 128 tokens. Per 64-k stage it copies the x tile (128 rows x 128 B, full lines, XOR-swizzled
// 16-byte slots) and the weight pieces of its tiles into LDS with LDS-DMA (global_load_lds_dwordx4), two buffers deep, and
// each wave runs 16 x 16 x 32 bf16 MFMAs over its 64 tokens x RB / 2 rows: A = x rows (tokens on the fragment's rows), B = W
// rows (weight rows on the lanes), so each lane's results are 4 tokens of ONE weight row and the store maps that packed row to
// its HF row once. No split-K: the host picks RB = 64 when 128-row blocks would leave most CUs idle.

#include "prefill_mfma_device.h"

namespace sd {

namespace {

template <int RF, bool W8>
__global__ __launch_bounds__(kThreads, 2) void prefill_mfma_kernel(MfmaArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[mfma_smem_bytes<RF, W8>()];
  f32x4_t acc[4][RF];
  int hrow[RF], t0, rb;
  mfma_block_product<RF, W8>(a, smem, acc, hrow, t0, rb);
  const int lane = threadIdx.x & 63, wt = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) & 1, g = lane >> 4;

  // lane (n, g) holds tokens 4 g + e of its fragment row q, for weight row (fragment column) n of fragment f
#pragma unroll
  for (int f = 0; f < RF; ++f) {
    const int r = hrow[f];
    if (r < 0) continue;
    const float sc = W8 ? a.w_scale[r] : 1.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int t = t0 + wt * 64 + q * 16 + 4 * g + e;
        if (t < a.T) a.Y[static_cast<size_t>(t) * a.N + r] = acc[q][f][e] * sc;
      }
  }
}

}  // namespace

bool prefill_native_shapes_ok(const sd_model_config& c) {
  return c.arch == SD_ARCH_LLAMA && c.d_model % 64 == 0 && (c.n_heads * c.head_dim) % 64 == 0 && c.d_ff % 64 == 0;
}

const char* prefill_native_refusal(const sd_model_config& c, bool packed) {
  if (c.arch != SD_ARCH_LLAMA) return "native prefill serves Llama models only (this model is GPT-2)";
  if (!packed) return "native prefill reads the packed weights (this model has none: SPECDEC_NO_PACK)";
  if (!prefill_native_shapes_ok(c)) return "native prefill needs d_model, Hq*D and d_ff multiples of 64";
  return nullptr;
}

// Tiles of each matrix shape in stream order (the loop of pack_kernel: per workgroup share of ppw pairs, tiles of tile_pairs),
// grouped into row blocks of whole tiles of <= 128 (and, separately, <= 64) rows.
int native_plan_tables(const sd_model_config& c, NativeTables& t) {
  SD_REQUIRE(c.d_model % 64 == 0, "prefill: the native GEMM needs d_model a multiple of 64 (got %d)", c.d_model);
  t = NativeTables{};
  t.layers = prefill_native_shapes_ok(c);
  std::vector<int4>& tiles = t.tiles;
  std::vector<int2>& blocks = t.blocks;
  auto& spans = t.spans;
  for (int i = t.layers ? 0 : 4; i < 5; ++i) {
    const MatShape sh = matrix_shape(c, i);
    const int n_pairs = sh.n_pairs;
    const GemvGeom q = gemv_geometry(n_pairs, sh.K);
    std::vector<int2> raw;   // {first pair, pairs}
    for (int p_lo = 0; p_lo < n_pairs; p_lo += q.ppw) {
      const int p_hi = std::min(p_lo + q.ppw, n_pairs);
      for (int p0 = p_lo; p0 < p_hi; p0 += q.tile_pairs) raw.push_back(make_int2(p0, std::min(q.tile_pairs, p_hi - p0)));
    }
    for (int v = 0; v < 2; ++v) {
      const int rb = v == 0 ? 128 : 64;
      spans[i][v].tiles = tiles.size();
      spans[i][v].blocks = blocks.size();
      int first = 0, rows = 0;
      for (size_t k = 0; k < raw.size(); ++k) {
        const int nr = 2 * raw[k].y;
        SD_REQUIRE(nr <= rb, "prefill: tile of %d rows", nr);
        if (rows + nr > rb) {
          blocks.push_back(make_int2(first, static_cast<int>(k) - first));
          first = static_cast<int>(k);
          rows = 0;
        }
        tiles.push_back(make_int4(rows, raw[k].y, raw[k].x, 0));
        rows += nr;
      }
      blocks.push_back(make_int2(first, static_cast<int>(raw.size()) - first));
      spans[i][v].n_blocks = static_cast<int>(blocks.size() - spans[i][v].blocks);
    }
    // block tile indices are relative to the span's first tile; made absolute below
    for (int v = 0; v < 2; ++v)
      for (int b = 0; b < spans[i][v].n_blocks; ++b) blocks[spans[i][v].blocks + b].x += static_cast<int>(spans[i][v].tiles);
  }
  return 0;
}

PrefillPlanInfo native_plan_info(const NativeTables& t, const sd_model_config& c, int which, int T) {
  PrefillPlanInfo p{};
  p.n_tb = (T + kBT - 1) / kBT;
  p.variant = native_block_variant(t.spans[which][0].n_blocks, p.n_tb);
  const NativeTables::Span& sp = t.spans[which][p.variant];
  p.first_block = static_cast<int>(sp.blocks);
  p.n_blocks = sp.n_blocks;
  p.grid = p.n_blocks * p.n_tb;
  p.swizzled = (p.grid & 7) == 0 ? 1 : 0;
  p.last_tb_rows = T - (p.n_tb - 1) * kBT;
  p.min_block_rows = 1 << 30;
  for (int b = 0; b < sp.n_blocks; ++b) {
    const int2 blk = t.blocks[sp.blocks + b];
    int rows = 0;
    for (int k = 0; k < blk.y; ++k) rows += 2 * t.tiles[blk.x + k].y;
    p.min_block_rows = std::min(p.min_block_rows, rows);
  }
  p.k_stages = matrix_shape(c, which).K >> 6;
  return p;
}

int native_plan_build(const sd_model_config& c, NativePlan& plan) {
  NativeTables t;
  if (int rc = native_plan_tables(c, t)) return rc;
  const std::vector<int4>& tiles = t.tiles;
  const std::vector<int2>& blocks = t.blocks;
  const auto& spans = t.spans;
  const bool layers = t.layers;
  const size_t tb = tiles.size() * sizeof(int4), bb = blocks.size() * sizeof(int2);
  native_plan_free(plan);
  SD_HIP_CHECK(hipMalloc(&plan.buf, tb + bb));
  SD_HIP_CHECK(hipMemcpy(plan.buf, tiles.data(), tb, hipMemcpyHostToDevice));
  SD_HIP_CHECK(hipMemcpy(static_cast<char*>(plan.buf) + tb, blocks.data(), bb, hipMemcpyHostToDevice));
  const int4* dt = static_cast<const int4*>(plan.buf);
  const int2* db = reinterpret_cast<const int2*>(static_cast<char*>(plan.buf) + tb);
  for (int i = layers ? 0 : 4; i < 5; ++i)
    for (int v = 0; v < 2; ++v) {
      NativeMat& m = plan.mat[i][v];
      m.tiles = dt;
      m.blocks = db + spans[i][v].blocks;
      m.n_blocks = spans[i][v].n_blocks;
      m.rb = v == 0 ? 128 : 64;
      const MatShape sh = matrix_shape(c, i);
      m.N = sh.N;
      m.K = sh.K;
      m.n_pairs = sh.n_pairs;
      m.epi = sh.epi;
    }
  plan.layers = layers;
  plan.head_dim = c.head_dim;
  return 0;
}

void native_plan_free(NativePlan& plan) {
  if (plan.buf) (void)hipFree(plan.buf);
  plan = NativePlan{};
}

// which = 0 qkv, 1 out, 2 gate / up, 3 down
int launch_prefill_mfma(const NativePlan& plan, int which, const void* W, const float* w_scale, bool w8, const uint16_t* X, int ldx, float* Y,
                        int T, hipStream_t st) {
  SD_REQUIRE(plan.buf && plan.layers && which >= 0 && which < 4, "prefill: native plan not built");
  SD_REQUIRE(T >= 1 && T <= kPrefillChunk, "prefill: native GEMM of %d rows", T);
  SD_REQUIRE(W && X && Y && (!w8 || w_scale), "prefill: native GEMM with a NULL operand");
  const int n_tb = (T + kBT - 1) / kBT;
  const int v = native_block_variant(plan.mat[which][0].n_blocks, n_tb);
  const NativeMat& m = plan.mat[which][v];
  MfmaArgs a{};
  a.W = static_cast<const char*>(W);
  a.w_scale = w_scale;
  a.X = reinterpret_cast<const char*>(X);
  a.Y = Y;
  a.tiles = m.tiles;
  a.blocks = m.blocks;
  a.T = T;
  a.N = m.N;
  a.K = m.K;
  a.ldx = ldx;
  a.n_blocks = m.n_blocks;
  a.n_tb = n_tb;
  a.row_bytes = w8 ? ((m.K + 63) & ~63) : ((m.K + 31) & ~31) * 2;
  a.epi = m.epi;
  a.head_dim = plan.head_dim;
  a.n_pairs = m.n_pairs;
  const dim3 grid(m.n_blocks * n_tb), block(kThreads);
  if (w8) {
    if (v == 0) hipLaunchKernelGGL((prefill_mfma_kernel<4, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((prefill_mfma_kernel<2, true>), grid, block, 0, st, a);
  } else {
    if (v == 0) hipLaunchKernelGGL((prefill_mfma_kernel<4, false>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((prefill_mfma_kernel<2, false>), grid, block, 0, st, a);
  }
  SD_LAUNCH_CHECK();
  return 0;
}

}  // namespace sd
