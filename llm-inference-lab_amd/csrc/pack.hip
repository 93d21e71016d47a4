// Weight pre-packing for the streaming GEMV (csrc/gemv.hip).
//
// HF stores a Linear weight as [out][in] row-major. An MFMA A-fragment load of gemv.hip
// touches 16 rows x 64 bytes, i.e. 16 different DRAM pages per wave-instruction; measured,
// that pattern streams ~20 % below a row-contiguous one on MI355X. The engine therefore keeps
// a private copy of every matrix in the order the kernel consumes it: for each workgroup's
// pair range, tile by tile, every 32-k step of a tile is ONE contiguous block
//     [g = 0..3][row = 0..2*np-1] x 16 bytes      (np = pairs in the tile, <= 8)
// so a wave-instruction reads 2*np*64 contiguous bytes and consecutive steps continue the same
// stream: each wave walks one contiguous region of HBM. Rows of a tile are its pairs' first
// rows, then their second rows (pair_rows). K is padded to a multiple of 32 with zeros, a
// missing second row (odd vocabulary) is a zero row. The packed size is n_pairs*2*K32*2 bytes.
//
// fp8 storage (sd_model_config.weight_dtype = SD_FP8_E4M3): the same blocks, but a lane's 16
// bytes are 16 OCP e4m3 values — its fragments of TWO consecutive 32-k steps (k = 64 S + 8 g + 0..7
// and k = 64 S + 32 + 8 g + 0..7) — so one load feeds two MFMAs and the stream is half as long.
// Quantisation happens here, on the device, from the bf16 matrices the caller passes:
// per output row r, scale[r] = max|w[r][:]| / 448 (1 for an all-zero row), q = rne_e4m3(w / scale[r]);
// the kernel multiplies the fp32 accumulator of row r by scale[r]. The scales (fp32 [N]) follow the
// packed bytes of their matrix. K is padded to a multiple of 64.

#include "gemv_device.h"

namespace sd {

GemvGeom gemv_geometry(int n_pairs, int K) {
  GemvGeom q{};
  int grid = 256;  // one workgroup per CU
  if (n_pairs < grid) grid = n_pairs;
  q.ppw = (n_pairs + grid - 1) / grid;
  q.grid = (n_pairs + q.ppw - 1) / q.ppw;
  q.n_tiles = 1;
  while (q.n_tiles * 8 < q.ppw) q.n_tiles <<= 1;
  q.tile_pairs = (q.ppw + q.n_tiles - 1) / q.n_tiles;
  int ksplit = 16 / (q.n_tiles < 16 ? q.n_tiles : 16);
  while (ksplit > 1 && (K + ksplit * 32 - 1) / (ksplit * 32) < 2) ksplit >>= 1;  // >= 2 steps per slice
  q.ksplit = ksplit;
  q.kw = ((K + ksplit * 32 - 1) / (ksplit * 32)) * 32;
  return q;
}

struct PackJob {
  const uint16_t* src;
  uint16_t* dst;
  int N, K, n_pairs, epi, head_dim, ppw, tile_pairs;
};

__device__ __forceinline__ void pack_pair_rows(const PackJob& j, int p, int& r0, int& r1) {
  if (j.epi == EPI_QKV_ROPE) {
    const int half = j.head_dim >> 1;
    const int h = p / half, i = p - h * half;
    r0 = h * j.head_dim + i;
    r1 = r0 + half;
  } else if (j.epi == EPI_SWIGLU) {
    r0 = p;
    r1 = p + j.n_pairs;
  } else {
    r0 = 2 * p;
    r1 = 2 * p + 1;
  }
}

__global__ __launch_bounds__(256) void pack_kernel(PackJob j) {
  const int K32 = (j.K + 31) & ~31;
  const int qn = K32 >> 3;  // 16-byte chunks per packed row
  const size_t total = static_cast<size_t>(j.n_pairs) * 2 * qn;
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < total;
       i += static_cast<size_t>(gridDim.x) * 256) {
    const int q = static_cast<int>(i % qn);
    const size_t t = i / qn;
    const int second = static_cast<int>(t & 1);
    const int p = static_cast<int>(t >> 1);
    const int c = p / j.ppw;
    const int p_lo = c * j.ppw;
    const int p_hi = min(p_lo + j.ppw, j.n_pairs);
    const int tile = (p - p_lo) / j.tile_pairs;
    const int p0 = p_lo + tile * j.tile_pairs;
    const int np = min(j.tile_pairs, p_hi - p0);
    const int jp = p - p0;
    const int S = q >> 2, g = q & 3;
    const size_t dst_chunk = static_cast<size_t>(p0) * 2 * qn + static_cast<size_t>(S) * (2 * np * 4) + g * 2 * np + second * np + jp;
    int r0, r1;
    pack_pair_rows(j, p, r0, r1);
    const int r = second ? r1 : r0;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r < j.N && q * 8 + 8 <= j.K) v = *reinterpret_cast<const uint4*>(j.src + static_cast<size_t>(r) * j.K + q * 8);
    *reinterpret_cast<uint4*>(j.dst + dst_chunk * 8) = v;
  }
}

// scale[r] = max |w[r][:]| / 448, one wave per row
__global__ __launch_bounds__(kWave) void row_scale_kernel(const uint16_t* __restrict__ w, int N, int K, float* __restrict__ scale) {
  const int r = blockIdx.x, lane = threadIdx.x;
  float m = 0.f;
  for (int k = lane; k < K; k += kWave) m = fmaxf(m, fabsf(bf16_bits_to_float(w[static_cast<size_t>(r) * K + k])));
  m = wave_reduce_max(m);
  if (lane == 0) scale[r] = m > 0.f ? m / 448.0f : 1.0f;
}

__global__ __launch_bounds__(256) void pack_fp8_kernel(PackJob j, const float* __restrict__ scale) {
  const int K64 = (j.K + 63) & ~63;
  const int qn = K64 >> 4;  // 16-byte chunks (16 fp8) per packed row
  const size_t total = static_cast<size_t>(j.n_pairs) * 2 * qn;
  uint8_t* dst = reinterpret_cast<uint8_t*>(j.dst);
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < total;
       i += static_cast<size_t>(gridDim.x) * 256) {
    const int q = static_cast<int>(i % qn);
    const size_t t = i / qn;
    const int second = static_cast<int>(t & 1);
    const int p = static_cast<int>(t >> 1);
    const int c = p / j.ppw;
    const int p_lo = c * j.ppw;
    const int p_hi = min(p_lo + j.ppw, j.n_pairs);
    const int tile = (p - p_lo) / j.tile_pairs;
    const int p0 = p_lo + tile * j.tile_pairs;
    const int np = min(j.tile_pairs, p_hi - p0);
    const int jp = p - p0;
    const int S = q >> 2, g = q & 3;  // double step (64 k), k-group
    const size_t dst_chunk = static_cast<size_t>(p0) * 2 * qn + static_cast<size_t>(S) * (2 * np * 4) + g * 2 * np + second * np + jp;
    int r0, r1;
    pack_pair_rows(j, p, r0, r1);
    const int r = second ? r1 : r0;
    uint32_t out[4] = {0u, 0u, 0u, 0u};
    if (r < j.N) {
      const float sc = scale[r];
      const uint16_t* row = j.src + static_cast<size_t>(r) * j.K;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int k0 = 64 * S + 32 * half + 8 * g;
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = (k0 + e < j.K) ? bf16_bits_to_float(row[k0 + e]) / sc : 0.f;
        int lo = 0, hi = 0;
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
        out[2 * half] = static_cast<uint32_t>(lo);
        out[2 * half + 1] = static_cast<uint32_t>(hi);
      }
    }
    *reinterpret_cast<uint4*>(dst + dst_chunk * 16) = make_uint4(out[0], out[1], out[2], out[3]);
  }
}

// row-major fp8 image of a matrix with the scales of row_scale_kernel (sd_quantize_fp8_rows): the same
// arithmetic as pack_fp8_kernel, kept separately so that the quantiser can be checked bit for bit
__global__ __launch_bounds__(256) void quantize_rows_kernel(const uint16_t* __restrict__ w, int N, int K,
                                                            const float* __restrict__ scale, uint8_t* __restrict__ q) {
  const size_t total = static_cast<size_t>(N) * (K >> 2);
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < total; i += static_cast<size_t>(gridDim.x) * 256) {
    const size_t r = i / (K >> 2);
    const int k0 = static_cast<int>(i % (K >> 2)) * 4;
    const float sc = scale[r];
    const uint16_t* row = w + r * K + k0;
    int v = 0;
    v = __builtin_amdgcn_cvt_pk_fp8_f32(bf16_bits_to_float(row[0]) / sc, bf16_bits_to_float(row[1]) / sc, v, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(bf16_bits_to_float(row[2]) / sc, bf16_bits_to_float(row[3]) / sc, v, true);
    *reinterpret_cast<int*>(q + r * K + k0) = v;
  }
}

// the model's matrices in packing order (kernels.h): the one place that knows their shapes
MatShape head_shape(int vocab, int d_model) { return {vocab, d_model, (vocab + 1) / 2, EPI_ARGMAX}; }

MatShape matrix_shape(const sd_model_config& c, int which) {
  const int d = c.d_model, HqD = c.n_heads * c.head_dim, Nqkv = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim, ff = c.d_ff;
  switch (which) {
    case 0: return {Nqkv, d, Nqkv / 2, EPI_QKV_ROPE};
    case 1: return {d, HqD, d / 2, EPI_RESID};
    case 2: return c.arch == SD_ARCH_LLAMA ? MatShape{2 * ff, d, ff, EPI_SWIGLU} : MatShape{ff, d, ff / 2, EPI_GELU};
    case 3: return {d, ff, d / 2, EPI_RESID};
    default: return head_shape(c.vocab, d);
  }
}

MatWeights matrix_weights(const sd_model_config& c, int index) {
  if (index == 4 * c.n_layers) return {c.lm_head, nullptr, c.final_norm_w, c.final_norm_b};
  const sd_layer_weights& w = c.layers[index >> 2];
  switch (index & 3) {
    case 0: return {w.wqkv, w.bqkv, w.attn_norm_w, w.attn_norm_b};
    case 1: return {w.wo, w.bo, nullptr, nullptr};
    case 2: return {w.w_up, w.b_up, w.mlp_norm_w, w.mlp_norm_b};
    default: return {w.w_down, w.b_down, nullptr, nullptr};
  }
}

size_t packed_matrix_bytes(int n_pairs, int K) {
  const size_t K32 = (static_cast<size_t>(K) + 31) & ~static_cast<size_t>(31);
  return (static_cast<size_t>(n_pairs) * 2 * K32 * 2 + 255) & ~static_cast<size_t>(255);
}

// fp8: packed bytes, then the fp32 row scales
size_t packed_fp8_weight_bytes(int n_pairs, int K) {
  const size_t K64 = (static_cast<size_t>(K) + 63) & ~static_cast<size_t>(63);
  return (static_cast<size_t>(n_pairs) * 2 * K64 + 255) & ~static_cast<size_t>(255);
}
static size_t packed_fp8_matrix_bytes(int n_pairs, int K) {
  return packed_fp8_weight_bytes(n_pairs, K) + ((static_cast<size_t>(n_pairs) * 2 * 4 + 255) & ~static_cast<size_t>(255));
}
static size_t matrix_bytes(const sd_model_config& c, int index) {
  const MatShape m = matrix_shape(c, matrix_which(c, index));
  return c.weight_dtype == SD_FP8_E4M3 ? packed_fp8_matrix_bytes(m.n_pairs, m.K) : packed_matrix_bytes(m.n_pairs, m.K);
}

size_t packed_offset(const sd_model_config& c, int index) {
  size_t off = 0;
  for (int i = 0; i < index && i <= 4 * c.n_layers; ++i) off += matrix_bytes(c, i);
  return off;
}

size_t packed_any_matrix_bytes(int n_pairs, int K, int weight_dtype) {
  return weight_dtype == SD_FP8_E4M3 ? packed_fp8_matrix_bytes(n_pairs, K) : packed_matrix_bytes(n_pairs, K);
}

int pack_one_matrix(const void* w_bf16, int N, int K, int n_pairs, int epi, int head_dim, int weight_dtype, void* dst, hipStream_t st) {
  SD_REQUIRE(w_bf16 && dst, "pack: NULL matrix");
  SD_REQUIRE(K % 8 == 0, "pack: K=%d must be a multiple of 8", K);
  const GemvGeom q = gemv_geometry(n_pairs, K);
  PackJob j{static_cast<const uint16_t*>(w_bf16), static_cast<uint16_t*>(dst), N, K, n_pairs, epi, head_dim, q.ppw, q.tile_pairs};
  if (weight_dtype == SD_FP8_E4M3) {
    float* scale = reinterpret_cast<float*>(static_cast<char*>(dst) + packed_fp8_weight_bytes(n_pairs, K));
    hipLaunchKernelGGL(row_scale_kernel, dim3(N), dim3(kWave), 0, st, static_cast<const uint16_t*>(w_bf16), N, K, scale);
    SD_LAUNCH_CHECK();
    hipLaunchKernelGGL(pack_fp8_kernel, dim3(2048), dim3(256), 0, st, j, scale);
  } else {
    hipLaunchKernelGGL(pack_kernel, dim3(2048), dim3(256), 0, st, j);
  }
  SD_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------
// W12: a lossless 12-bit copy of a packed bf16 stream, for the launches of <= 9 tokens (gemv.hip).
//
// A BLOCK is one (tile, 32-k step) unit of the stream above — 8*np chunks of 16 bytes, what one wave-instruction
// loads. bf16 weights use a narrow exponent range locally: where all 16*np*16 exponents of a block lie within 16
// values [base, base + 15] the block is NARROW and chunk c becomes 12 bytes, its 8 weights as 12-bit codes
//     sign << 11 | (exp - base) << 7 | mantissa          (weight i at bit 12 i; widened exactly by w12_widen)
// Any other block (an exact zero or a denormal among normal weights, a value more than 15 binades under the block's
// largest, inf / nan) is WIDE and keeps its 16 raw bytes per chunk, split 12 + 4. Three parts per matrix:
//   main      the slot of a block, 8*np x 12 bytes, sits at 3/4 of the block's byte offset in the bf16 stream: a narrow
//             chunk's codes or the first 12 bytes of a wide chunk. A wave reads a slot with one global_load_dwordx3 at
//             lane * 12, at an address it computes WITHOUT the table — the weight stream does not wait for it.
//   overflow  wide block number k (stream order) owns 256 bytes at 256 k: the fourth dword of chunk c at 4 c.
//   table     one uint32 per (tile, step), index (workgroup * n_tiles_full + tile) * (K / 32) + step:
//             wide << 31 | base << 23 | k. A wave fetches the entries of a batch with one vector load in front of the
//             batch's weight loads and reads them with readlane; only the widening and the rare overflow load wait for it.
// Whether a block is narrow is decided by widening its codes and comparing bits (w12_classify_kernel), not by a rule on
// the exponents. specdec_hip/w12.py restates the format; the measured narrow share is in profiles/w12_verify.md.
// The split-byte FORM (W12_SPLIT, "W12S") keeps all of the above and changes only what a narrow chunk's 12 bytes hold — the 8 low
// bytes raw, the high bytes as 4-bit codes in an even-aligned 16-exponent window (gemv_device.h) — and with it the base rule and
// the widening. One packer, two encoders; profiles/w12_split.md has its narrow share.
// ------------------------------------------------------------------------------
size_t w12_table_entries(int n_pairs, int K) {
  const GemvGeom q = gemv_geometry(n_pairs, K);
  const size_t ntf = (q.ppw + q.tile_pairs - 1) / q.tile_pairs;
  return static_cast<size_t>(q.grid) * ntf * (((static_cast<size_t>(K) + 31) & ~static_cast<size_t>(31)) >> 5);
}

W12Layout w12_layout(int n_pairs, int K, uint32_t n_wide) {
  const size_t K32 = (static_cast<size_t>(K) + 31) & ~static_cast<size_t>(31);
  auto pad = [](size_t v) { return (v + 255) & ~static_cast<size_t>(255); };
  return {pad(static_cast<size_t>(n_pairs) * 2 * K32 * 2 / 4 * 3), pad(static_cast<size_t>(n_wide) * kW12OvfBlock), pad(w12_table_entries(n_pairs, K) * 4)};
}

bool w12_taken(int n_pairs, int K, uint32_t n_wide) {
  if (!gemv_w12_covers(n_pairs, K) || n_wide >= (1u << 23)) return false;
  return static_cast<double>(w12_layout(n_pairs, K, n_wide).total()) <= 0.85 * static_cast<double>(packed_matrix_bytes(n_pairs, K));
}

struct W12Job {
  const uint16_t* src;   // packed bf16 stream
  uint32_t* table;
  unsigned char* main;
  unsigned char* ovf;
  int n_pairs, K32, ppw, tile_pairs, ntf;
  int form;   // W12Form
};

// block `b` of the table: pairs of its tile (0: the last workgroup has no such tile) and its byte offset in the bf16 stream
__device__ __forceinline__ int w12_block(const W12Job& j, size_t b, size_t& off) {
  const int nst = j.K32 >> 5;
  const int gt = static_cast<int>(b / nst), step = static_cast<int>(b - static_cast<size_t>(gt) * nst);
  const int c = gt / j.ntf, t = gt - c * j.ntf;
  const int p_lo = c * j.ppw, p_hi = min(p_lo + j.ppw, j.n_pairs);
  const int p0 = p_lo + t * j.tile_pairs;
  if (p0 >= p_hi) return 0;
  const int np = min(j.tile_pairs, p_hi - p0);
  off = static_cast<size_t>(p0) * 2 * j.K32 * 2 + static_cast<size_t>(step) * 128 * np;
  return np;
}

// one wave per block: table[b] = base << 23 for a narrow block, 1 << 31 for a wide one (numbered by w12_number_kernel)
__global__ __launch_bounds__(256) void w12_classify_kernel(W12Job j, size_t n_entries) {
  const int lane = threadIdx.x & 63;
  const size_t n_waves = static_cast<size_t>(gridDim.x) * 4;
  for (size_t b = static_cast<size_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); b < n_entries; b += n_waves) {
    size_t off = 0;
    const int np = w12_block(j, b, off);
    uint32_t ent = 0;
    if (np) {
      const bool active = lane < 8 * np;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (active) v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(j.src) + off + lane * 16);
      int emax = 0;
      if (active) {
#pragma unroll
        for (int i = 0; i < 8; ++i) emax = max(emax, static_cast<int>((v[i >> 1] >> (16 * (i & 1) + 7)) & 0xFFu));
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) emax = max(emax, __shfl_xor(emax, o, 64));
      const uint32_t base = w12_base_of(j.form, emax);
      const u32x4 back = j.form == W12_SPLIT ? w12_widen_form<W12_SPLIT>(w12s_encode(v, base), base) : w12_widen_form<W12_CODES>(w12_encode(v, base), base);
      const bool same = !active || (back[0] == v[0] && back[1] == v[1] && back[2] == v[2] && back[3] == v[3]);
      ent = (__ballot(same) == ~0ull) ? (base << 23) : 0x80000000u;
    }
    if (lane == 0) j.table[b] = ent;
  }
}

// one workgroup: number the wide blocks in table (= stream) order; *n_wide = their count
__global__ __launch_bounds__(1024) void w12_number_kernel(uint32_t* __restrict__ table, size_t n, uint32_t* __restrict__ n_wide) {
  __shared__ uint32_t cnt[1024];
  const int tid = threadIdx.x;
  const size_t per = (n + 1023) / 1024, lo = min(n, tid * per), hi = min(n, lo + per);
  uint32_t c = 0;
  for (size_t i = lo; i < hi; ++i) c += table[i] >> 31;
  cnt[tid] = c;
  __syncthreads();
  uint32_t k = 0;
  for (int t = 0; t < tid; ++t) k += cnt[t];
  for (size_t i = lo; i < hi; ++i)
    if (table[i] >> 31) table[i] = 0x80000000u | k++;
  if (tid == 1023) *n_wide = k;
}

// one wave per block: the main slot, and a wide block's overflow
__global__ __launch_bounds__(256) void w12_fill_kernel(W12Job j, size_t n_entries) {
  const int lane = threadIdx.x & 63;
  const size_t n_waves = static_cast<size_t>(gridDim.x) * 4;
  for (size_t b = static_cast<size_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); b < n_entries; b += n_waves) {
    size_t off = 0;
    const int np = w12_block(j, b, off);
    if (!np) continue;
    const uint32_t ent = j.table[b];
    const bool active = lane < 8 * np;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (active) v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(j.src) + off + lane * 16);
    if (ent >> 31) *reinterpret_cast<uint32_t*>(j.ovf + static_cast<size_t>(ent & 0x7FFFFFu) * kW12OvfBlock + lane * 4) = v[3];   // (lanes without a chunk: zero)
    else v = j.form == W12_SPLIT ? w12s_encode(v, (ent >> 23) & 0xFFu) : w12_encode(v, (ent >> 23) & 0xFFu);
    if (active) {
      uint32_t* d = reinterpret_cast<uint32_t*>(j.main + off / 4 * 3 + lane * 12);
      d[0] = v[0];
      d[1] = v[1];
      d[2] = v[2];
    }
  }
}

static W12Job w12_job(const void* packed_bf16, int n_pairs, int K, uint32_t* table, void* main, void* ovf, int form) {
  const GemvGeom q = gemv_geometry(n_pairs, K);
  return {static_cast<const uint16_t*>(packed_bf16), table, static_cast<unsigned char*>(main), static_cast<unsigned char*>(ovf),
          n_pairs, (K + 31) & ~31, q.ppw, q.tile_pairs, (q.ppw + q.tile_pairs - 1) / q.tile_pairs, form};
}

static int w12_grid(size_t n_entries) { return static_cast<int>(n_entries / 4 + 1 < 8192 ? n_entries / 4 + 1 : 8192); }

// table of one matrix (classified and numbered) and its wide-block count, on the device
int w12_measure_matrix(const void* packed_bf16, int n_pairs, int K, uint32_t* table, uint32_t* n_wide, int form, hipStream_t st) {
  const size_t n = w12_table_entries(n_pairs, K);
  hipLaunchKernelGGL(w12_classify_kernel, dim3(w12_grid(n)), dim3(256), 0, st, w12_job(packed_bf16, n_pairs, K, table, nullptr, nullptr, form), n);
  SD_LAUNCH_CHECK();
  hipLaunchKernelGGL(w12_number_kernel, dim3(1), dim3(1024), 0, st, table, n, n_wide);
  SD_LAUNCH_CHECK();
  return 0;
}

// the W12 copy at dst ([main][overflow][table], w12_layout) from the packed stream and its measured table
int w12_fill_matrix(const void* packed_bf16, int n_pairs, int K, const uint32_t* table, uint32_t n_wide, void* dst, int form, hipStream_t st) {
  const W12Layout l = w12_layout(n_pairs, K, n_wide);
  const size_t n = w12_table_entries(n_pairs, K);
  char* d = static_cast<char*>(dst);
  uint32_t* tab = reinterpret_cast<uint32_t*>(d + l.main_bytes + l.ovf_bytes);
  SD_HIP_CHECK(hipMemcpyAsync(tab, table, n * 4, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(w12_fill_kernel, dim3(w12_grid(n)), dim3(256), 0, st, w12_job(packed_bf16, n_pairs, K, tab, d, d + l.main_bytes, form), n);
  SD_LAUNCH_CHECK();
  return 0;
}

size_t w12_scratch_offset(const sd_model_config& c, int index) {   // table of matrix `index` in the scratch of sd_w12_measure
  size_t off = 0;
  for (int i = 0; i < index; ++i) {
    const MatShape m = matrix_shape(c, matrix_which(c, i));
    off += (w12_table_entries(m.n_pairs, m.K) * 4 + 255) & ~static_cast<size_t>(255);
  }
  return off;
}

size_t w12_offset(const sd_model_config& c, const uint32_t* n_wide, int index) {   // copy of matrix `index` in the buffer of sd_w12_pack
  size_t off = 0;
  for (int i = 0; i < index && i <= 4 * c.n_layers; ++i) {
    const MatShape m = matrix_shape(c, matrix_which(c, i));
    if (w12_taken(m.n_pairs, m.K, n_wide[i])) off += w12_layout(m.n_pairs, m.K, n_wide[i]).total();
  }
  return off;
}

}  // namespace sd

using namespace sd;

static int w12_cfg_ok(const sd_model_config* cfg, const char* who) {
  SD_REQUIRE(cfg && cfg->layers && cfg->packed, "%s: needs a config with the packed bf16 buffer of sd_pack_weights", who);
  SD_REQUIRE(cfg->weight_dtype == SD_BF16, "%s: W12 is a copy of bf16 weights (weight_dtype %d)", who, cfg->weight_dtype);
  return 0;
}

extern "C" size_t sd_w12_scratch_bytes(const sd_model_config* cfg) {
  if (!cfg || !cfg->layers) return 0;
  const int n = 4 * cfg->n_layers + 1;
  return w12_scratch_offset(*cfg, n) + ((static_cast<size_t>(n) * 4 + 255) & ~static_cast<size_t>(255));
}

static int w12_form_ok(int form, const char* who) {
  SD_REQUIRE(form == W12_CODES || form == W12_SPLIT, "%s: form %d (SD_W12_FORM_CODES or SD_W12_FORM_SPLIT)", who, form);
  return 0;
}

extern "C" int sd_w12_measure_form(const sd_model_config* cfg, int form, void* scratch, size_t scratch_bytes, uint32_t* n_wide, void* stream) {
  clear_error();
  if (int rc = w12_cfg_ok(cfg, "w12_measure")) return rc;
  if (int rc = w12_form_ok(form, "w12_measure")) return rc;
  SD_REQUIRE(scratch && n_wide && scratch_bytes >= sd_w12_scratch_bytes(cfg), "w12_measure: scratch too small or NULL");
  SD_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "w12_measure: scratch must be 256-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int n = 4 * cfg->n_layers + 1;
  char* s = static_cast<char*>(scratch);
  uint32_t* counts = reinterpret_cast<uint32_t*>(s + w12_scratch_offset(*cfg, n));
  for (int i = 0; i < n; ++i) {
    const MatShape m = matrix_shape(*cfg, matrix_which(*cfg, i));
    const void* src = static_cast<const char*>(cfg->packed) + packed_offset(*cfg, i);
    if (int rc = w12_measure_matrix(src, m.n_pairs, m.K, reinterpret_cast<uint32_t*>(s + w12_scratch_offset(*cfg, i)), counts + i, form, st)) return rc;
  }
  SD_HIP_CHECK(hipMemcpyAsync(n_wide, counts, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost, st));
  SD_HIP_CHECK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int sd_w12_measure(const sd_model_config* cfg, void* scratch, size_t scratch_bytes, uint32_t* n_wide, void* stream) {
  return sd_w12_measure_form(cfg, W12_CODES, scratch, scratch_bytes, n_wide, stream);
}

extern "C" size_t sd_w12_bytes(const sd_model_config* cfg, const uint32_t* n_wide) {
  if (!cfg || !cfg->layers || !n_wide) return 0;
  return w12_offset(*cfg, n_wide, 4 * cfg->n_layers + 1);
}

extern "C" int sd_w12_matrix(const sd_model_config* cfg, const uint32_t* n_wide, int index, int* taken, size_t* offset, size_t* main_bytes,
                             size_t* ovf_bytes, size_t* table_bytes, size_t* blocks, size_t* bf16_bytes) {
  clear_error();
  SD_REQUIRE(cfg && cfg->layers && n_wide && index >= 0 && index <= 4 * cfg->n_layers, "w12_matrix: bad argument");
  const MatShape m = matrix_shape(*cfg, matrix_which(*cfg, index));
  const W12Layout l = w12_layout(m.n_pairs, m.K, n_wide[index]);
  if (taken) *taken = w12_taken(m.n_pairs, m.K, n_wide[index]) ? 1 : 0;
  if (offset) *offset = w12_offset(*cfg, n_wide, index);
  if (main_bytes) *main_bytes = l.main_bytes;
  if (ovf_bytes) *ovf_bytes = l.ovf_bytes;
  if (table_bytes) *table_bytes = l.table_bytes;
  if (blocks) *blocks = w12_table_entries(m.n_pairs, m.K);   // (entries of tiles the last workgroup does not have count as narrow)
  if (bf16_bytes) *bf16_bytes = packed_matrix_bytes(m.n_pairs, m.K);
  return 0;
}

extern "C" int sd_w12_pack_form(const sd_model_config* cfg, int form, const void* scratch, const uint32_t* n_wide, void* dst, size_t dst_bytes, void* stream) {
  clear_error();
  if (int rc = w12_cfg_ok(cfg, "w12_pack")) return rc;
  if (int rc = w12_form_ok(form, "w12_pack")) return rc;
  SD_REQUIRE(scratch && n_wide && (dst || !sd_w12_bytes(cfg, n_wide)), "w12_pack: NULL argument");
  SD_REQUIRE(dst_bytes >= sd_w12_bytes(cfg, n_wide), "w12_pack: destination too small");
  SD_REQUIRE((reinterpret_cast<uintptr_t>(dst) & 255) == 0, "w12_pack: destination must be 256-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int i = 0; i <= 4 * cfg->n_layers; ++i) {
    const MatShape m = matrix_shape(*cfg, matrix_which(*cfg, i));
    if (!w12_taken(m.n_pairs, m.K, n_wide[i])) continue;
    const void* src = static_cast<const char*>(cfg->packed) + packed_offset(*cfg, i);
    const uint32_t* table = reinterpret_cast<const uint32_t*>(static_cast<const char*>(scratch) + w12_scratch_offset(*cfg, i));
    if (int rc = w12_fill_matrix(src, m.n_pairs, m.K, table, n_wide[i], static_cast<char*>(dst) + w12_offset(*cfg, n_wide, i), form, st)) return rc;
  }
  return 0;
}

extern "C" int sd_w12_pack(const sd_model_config* cfg, const void* scratch, const uint32_t* n_wide, void* dst, size_t dst_bytes, void* stream) {
  return sd_w12_pack_form(cfg, W12_CODES, scratch, n_wide, dst, dst_bytes, stream);
}

// A vocabulary-sized output matrix [V][d] outside a model (Medusa heads): same layout and quantiser as the lm_head.
extern "C" size_t sd_packed_head_bytes(int vocab, int d_model, int weight_dtype) {
  const MatShape h = head_shape(vocab, d_model);
  return packed_any_matrix_bytes(h.n_pairs, h.K, weight_dtype);
}

extern "C" int sd_pack_head(const void* w_bf16, int vocab, int d_model, int weight_dtype, void* dst, size_t dst_bytes, void* stream) {
  clear_error();
  SD_REQUIRE(weight_dtype == SD_BF16 || weight_dtype == SD_FP8_E4M3, "pack_head: weight_dtype %d", weight_dtype);
  SD_REQUIRE(dst_bytes >= sd_packed_head_bytes(vocab, d_model, weight_dtype), "pack_head: destination too small");
  SD_REQUIRE((reinterpret_cast<uintptr_t>(dst) & 255) == 0, "pack_head: destination must be 256-byte aligned");
  const MatShape h = head_shape(vocab, d_model);
  return pack_one_matrix(w_bf16, h.N, h.K, h.n_pairs, h.epi, 0, weight_dtype, dst, static_cast<hipStream_t>(stream));
}

extern "C" size_t sd_packed_bytes(const sd_model_config* cfg) {
  if (!cfg || !cfg->layers) return 0;
  return packed_offset(*cfg, 4 * cfg->n_layers + 1);
}

extern "C" int sd_pack_weights(const sd_model_config* cfg, void* dst, size_t dst_bytes, void* stream) {
  clear_error();
  SD_REQUIRE(cfg && cfg->layers && dst, "pack_weights: NULL argument");
  SD_REQUIRE(cfg->weight_dtype == SD_BF16 || cfg->weight_dtype == SD_FP8_E4M3, "pack_weights: weight_dtype %d (bf16 or fp8 e4m3)", cfg->weight_dtype);
  SD_REQUIRE(dst_bytes >= sd_packed_bytes(cfg), "pack_weights: destination too small");
  SD_REQUIRE((reinterpret_cast<uintptr_t>(dst) & 255) == 0, "pack_weights: destination must be 256-byte aligned");
  char* p = static_cast<char*>(dst);
  for (int i = 0; i <= 4 * cfg->n_layers; ++i) {
    const MatShape m = matrix_shape(*cfg, matrix_which(*cfg, i));
    const void* w = matrix_weights(*cfg, i).w;
    SD_REQUIRE(w, "pack_weights: NULL matrix");
    SD_REQUIRE(m.K % 8 == 0, "pack_weights: K=%d must be a multiple of 8", m.K);
    if (int rc = pack_one_matrix(w, m.N, m.K, m.n_pairs, m.epi, cfg->head_dim, cfg->weight_dtype, p, static_cast<hipStream_t>(stream))) return rc;
    p += matrix_bytes(*cfg, i);
  }
  return 0;
}

extern "C" int sd_quantize_fp8_rows(const void* w_bf16, int N, int K, void* q_fp8, float* scales, void* stream) {
  clear_error();
  SD_REQUIRE(w_bf16 && q_fp8 && scales, "quantize_fp8_rows: NULL argument");
  SD_REQUIRE(N >= 1 && K >= 4 && K % 4 == 0, "quantize_fp8_rows: N=%d K=%d (K must be a multiple of 4)", N, K);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(row_scale_kernel, dim3(N), dim3(kWave), 0, st, static_cast<const uint16_t*>(w_bf16), N, K, scales);
  SD_LAUNCH_CHECK();
  hipLaunchKernelGGL(quantize_rows_kernel, dim3(1024), dim3(256), 0, st, static_cast<const uint16_t*>(w_bf16), N, K, scales,
                     static_cast<uint8_t*>(q_fp8));
  SD_LAUNCH_CHECK();
  return 0;
}
