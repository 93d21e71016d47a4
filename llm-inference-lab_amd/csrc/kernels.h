// Internal kernel-launch interfaces shared by the engine (not part of the C-ABI).
#pragma once

#include <vector>

#include "common.h"
#include "debug_env.h"

namespace sd {

// ---- skinny GEMM (gemv.hip) ---------------------------------------------------
enum GemvPrologue { PRO_NONE = 0, PRO_RMSNORM = 1, PRO_LAYERNORM = 2 };
enum GemvEpilogue { EPI_QKV_ROPE = 0, EPI_RESID = 1, EPI_SWIGLU = 2, EPI_GELU = 3, EPI_ARGMAX = 4 };

constexpr int kGemvMaxT = 9;     // tokens per launch of gemv.hip (K+1 for K = 8)
constexpr int kSkinnyMaxT = 128; // tokens per launch of gemm_skinny.hip (batched verify, chunked prefill)
static_assert(kSkinnyMaxT <= 255, "GemvArgs::T / M are 8-bit fields");

struct GemvArgs {
  // Field ORDER and WIDTHS are part of the design: these kernels are latency chains, every launch starts by pulling its
  // arguments through the scalar cache, and each further 64-byte line of the argument block that the first instructions
  // touch is a further miss (measured: two fields appended at byte 320 instead of byte 72 cost 0.8 % of the batch-1 step).
  // Lines 0 and 1 hold what EVERY variant needs before its first loads; the epilogue-specific fields follow.
  // ---- line 0: pointers
  const void* W;         // weights: bf16 [N][K] row-major, or the packed tile streams of csrc/pack.hip
  const void* x;         // activations in: bf16 [T][x_stride]
  void* out;             // q buffer / residual stream / activation / logits (may be null for ARGMAX)
  const void* norm_w;    // fused normalisation of x
  const void* norm_b;
  const void* bias;      // bf16 [N] or null
  const int32_t* x_row;  // nullable, device [T]: token t reads row x_row[t] of x instead of row t (gemv.hip only)
  // per-row adaptive K: a launch of draft forward skip_i leaves at once when *skip_k <= skip_i (null: never)
  const int32_t* skip_k;
  // ---- line 1: scalars
  unsigned long long* debug_ts;  // diagnostic timeline stamps [grid][8] or null
  int N, K;
  int n_pairs;       // row pairs processed (see pair_rows)
  int kw;            // K span per slice (set by launch_gemv)
  int x_stride;
  int out_stride;
  unsigned m_magic;  // ceil(65536 / M): t / M == (t * m_magic) >> 16 for t < 65536 / M... (exact for t < 512)
  float norm_eps;
  // small scalars as bitfields of 32-bit units (plain uint8_t / uint16_t kernel-argument fields made hipcc fetch some of
  // them with VECTOR byte loads; a bitfield is read as its dword through the scalar cache and extracted with s_bfe)
  unsigned T : 8;             // tokens in this pass (<= kSkinnyMaxT)
  unsigned M : 8;             // tokens per batch row (t = b*M + m)
  unsigned ppw : 16;          // pairs per workgroup (set by launch_gemv)
  unsigned n_tiles_full : 16; // tiles of a workgroup that owns a full share of ppw pairs
  unsigned tile_pairs : 4;    // pairs per tile, <= 8 (set by launch_gemv)
  unsigned ksplit : 5;        // K slices per tile, power of two <= 16 (set by launch_gemv)
  unsigned ks_shift : 3;      // log2(ksplit)   (derived by the launchers, gemv_derive: index arithmetic without runtime divisions)
  unsigned alias_part : 1;    // partial sums alias the staged x rows (set by launch_gemv)
  unsigned packed : 1;        // W is in the packed tile-stream order of csrc/pack.hip
  unsigned w8 : 1;            // W holds OCP fp8 e4m3 values (packed only); acc of row r is scaled by w_scale[r]
  unsigned w12 : 1;           // set by launch_gemv: W is the W12 main stream, w_scale its side table (see w12_main below)
  unsigned prologue : 2;      // GemvPrologue
  unsigned out_dtype : 2;     // SD_BF16 | SD_F32 (logits only)
  unsigned skip_i : 4;
  int half_shift : 8;         // log2(head_dim / 2), or -1 when head_dim / 2 is not a power of two (division fallback)
  // ---- epilogue-specific
  const float* w_scale;          // fp32 [N] row scales (w8); w12: the uint32 side table (in line 1 of the block: a wave's first load)
  // QKV epilogue: one 64-byte line (bytes 128..191)
  const int32_t* pos_base;  // device [B]
  const float* rope_cos;    // [max_pos][head_dim/2] or null (no RoPE)
  const float* rope_sin;
  void* k_cache;            // [B][n_kv_heads][l_max][head_dim] bf16
  void* v_cache;
  // paged KV (sd_model_bind_paged): k_cache / v_cache are page POOLS ([pages][Hkv][P][D] / [pages][Hkv][D][P]) and row b's
  // position pos lives in page block_table[b * (l_max >> page_shift) + (pos >> page_shift)] at offset pos & (P - 1).
  // null = dense rows of l_max positions.
  const int32_t* block_table;
  int pos_off;
  int max_pos;
  int l_max;
  unsigned head_dim : 8, n_q_heads : 8, n_kv_heads : 8, page_shift : 8;
  // ARGMAX epilogue: per-workgroup partials [T][grid]
  float* part_val;
  int* part_idx;
  // EPI_ARGMAX, gemv.hip only: n_batch equally shaped matrices at a constant byte stride (the K Medusa heads), one per
  // blockIdx.y, over the SAME x rows; partials of matrix j at part_val/part_idx + j * T * grid. 0 = a single matrix.
  size_t batch_bytes;
  int n_batch;
  // Row statistics handed from the kernel that WRITES the residual stream to the kernel that normalises it (> 9 tokens):
  // an EPI_RESID launch with xstat_out != null leaves, per token t and workgroup c, the sum of squares and the sum of the
  // new row values over the columns c owns: xstat_out[t * kStatStride + c] and xstat_out[kStatPlane + t * kStatStride + c].
  // A norm-fused launch with xstat_in != null adds the xstat_n partials of a token in a fixed order instead of reading
  // the whole row again (every one of its 256 workgroups would: 63 MB of L2 -> CU traffic at 40 tokens, 6-9 us).
  int xstat_n;
  float* xstat_out;
  const float* xstat_in;
  // W12 copy of the matrix (csrc/pack.hip: lossless 12-bit codes), or null. W stays the packed bf16 stream: launch_gemv
  // moves a launch of <= 9 tokens that the W12 kernels cover onto w12_main / w12_table, everything else reads W.
  const void* w12_main;
  const uint32_t* w12_table;
  const void* w12_ovf;           // fourth dwords of the wide blocks, 256 bytes each (read by the kernel, late and rarely)
  int w12_form;                  // W12Form of that copy (0 with a copy: W12_CODES); read by launch_gemv, not by the kernels
};
constexpr int kStatStride = 256;                    // partials per token (>= workgroups of the producing launch)
constexpr int kStatPlane = kSkinnyMaxT * kStatStride;   // floats per plane (plane 0: sum of squares, plane 1: sum)
bool gemm_resid_publishes_stats(const GemvArgs& a);  // true when launch_gemv(a, EPI_RESID) takes a kernel that honours xstat_out


// fields of GemvArgs every launcher derives from the caller's (idempotent)
inline void gemv_derive(GemvArgs& a) {
  const int half = a.head_dim >> 1;
  a.half_shift = -1;
  if (half > 0 && (half & (half - 1)) == 0)
    for (int s = 0; s < 31; ++s)
      if ((1 << s) == half) a.half_shift = s;
  const int M = a.M > 0 ? a.M : 1;
  a.m_magic = static_cast<unsigned>((65536 + M - 1) / M);
  a.ks_shift = 0;
  while ((1 << a.ks_shift) < a.ksplit) ++a.ks_shift;
}

// work split of one matrix over the chip (shared by the launcher and the weight packer)
struct GemvGeom {
  int grid, ppw, n_tiles, tile_pairs, ksplit, kw;
};
GemvGeom gemv_geometry(int n_pairs, int K);

// ---- the model's matrices (pack.hip), in packing order: per layer qkv, out, gate / up, down; then the lm_head.
// Matrix `index` = 4 * layer + which (which: 0 qkv, 1 out, 2 gate / up, 3 down); index 4 * n_layers (which 4) is the lm_head.
struct MatShape {
  int N, K, n_pairs, epi;   // rows, inputs, row pairs of the packed stream, GemvEpilogue
};
MatShape matrix_shape(const sd_model_config& c, int which);
MatShape head_shape(int vocab, int d_model);   // a vocabulary-sized output matrix: the lm_head, a Medusa head
inline int matrix_which(const sd_model_config& c, int index) { return index == 4 * c.n_layers ? 4 : index & 3; }
struct MatWeights {
  const void* w;        // bf16 HF-layout [N][K]
  const void* bias;     // [N] or null
  const void* norm_w;   // the normalisation fused in front of the product (qkv, gate / up, lm_head), else null
  const void* norm_b;
};
MatWeights matrix_weights(const sd_model_config& c, int index);

size_t packed_matrix_bytes(int n_pairs, int K);
size_t packed_fp8_weight_bytes(int n_pairs, int K);                     // fp8: the packed bytes, before the row scales
size_t packed_any_matrix_bytes(int n_pairs, int K, int weight_dtype);   // bf16 or fp8 (+ scales)
int pack_one_matrix(const void* w_bf16, int N, int K, int n_pairs, int epi, int head_dim, int weight_dtype, void* dst, hipStream_t st);
// W12 copy of a matrix (pack.hip): [main stream][overflow of the wide blocks][table], each padded to 256 bytes
constexpr int kW12OvfBlock = 256;
// what a narrow block's 12 bytes per lane hold (gemv_device.h): 12-bit codes, or raw low bytes + 4-bit high-byte codes (W12S)
enum W12Form { W12_NONE = 0, W12_CODES = 1, W12_SPLIT = 2 };
struct W12Layout {
  size_t main_bytes, ovf_bytes, table_bytes;   // padded
  size_t total() const { return main_bytes + ovf_bytes + table_bytes; }
};
size_t w12_table_entries(int n_pairs, int K);
W12Layout w12_layout(int n_pairs, int K, uint32_t n_wide);
size_t w12_offset(const sd_model_config& c, const uint32_t* n_wide, int index);   // copy of matrix `index` in the buffer of sd_w12_pack
bool w12_taken(int n_pairs, int K, uint32_t n_wide);   // covered by the kernels and >= 15 % smaller than the packed bf16 stream
size_t packed_offset(const sd_model_config& c, int index);  // byte offset of matrix `index` in the buffer of sd_pack_weights
int gemv_grid(const GemvArgs& a, int* ppw_out);
int gemv_max_tokens(int K);                                          // tokens gemv.hip can stage for rows of K elements (<= 9)
int launch_gemv(const GemvArgs& a, int epi, hipStream_t st);          // T <= 9: gemv.hip, else gemm_skinny.hip
int launch_gemm_skinny(const GemvArgs& a, int epi, hipStream_t st);   // T <= 64
// name of the gemv.hip instance a plain launch (packed, no bias / x_row / batch) of T <= 9 tokens takes: "generic" or
// "fixed<...>"; decided by the function launch_gemv asks. snprintf's return value.
int gemv_variant_name(int T, int n_pairs, int K, bool w8, int prologue, int epi, char* out, size_t cap, int w12 = W12_NONE);   // w12: W12Form of the matrix's copy
// name of the KERNEL such a launch runs, from the choice launch_gemv itself consumes: "fixed<...>" as above,
// "generic<EPI,whole|mask,ttN,bf16|fp8|w12|w12s,kbN>" (the template key of gemv_mfma_kernel) or "skinny:" + gemm_plan_name of the body the
// launch is handed to (rows too long to stage T of them). *len: snprintf's return value. Nonzero (error set) where launch_gemv refuses.
int gemv_instance_name(int T, int n_pairs, int K, bool w8, int prologue, int epi, char* out, size_t cap, int* len, int w12 = W12_NONE);
bool gemv_w12_covers(int n_pairs, int K);   // shape the W12 kernels stream: whole 32-k steps per K slice, one x chunk per thread
bool gemm_skinny_covers(int T, int n_pairs, int K, bool w8 = false);                  // shape handled by gemm_skinny.hip
// gemm_pipe.hip: the statically scheduled chunk pipeline for <= 64 tokens (tried first by launch_gemm_skinny, which has
// set the work split fields of `a`)
bool gemm_pipe_plan(int T, int n_pairs, int K, bool w8, int* kc_out, int* sc_out);   // covered: chunk width, steps per chunk
// The template instantiation a launch of 10..128 tokens runs: decided once (gemm_plan, gemm_skinny.hip), consumed by the
// launch switches of both files and printed by sd_gemm_plan.
enum GemmBody { BODY_NONE = 0, BODY_DIRECT, BODY_SLICE, BODY_PIPE, BODY_CHUNKED };
struct GemmPlan {
  int body;    // GemmBody; BODY_NONE: the shape is not covered
  int tg;      // token groups of the instantiation: 1..4 (direct, slice, pipe), 1..4, 6 or 8 (chunked)
  int steps;   // pipe: SC, steps per wave per chunk (1, 2, 4, 8); chunked: NB, steps per weight batch (1, 2, 4); else 0
  int kc;      // chunk width in columns (pipe, chunked), else 0
};
constexpr int kPlanNoDirect = 1, kPlanNoPipe = 2;   // `flags`: plan as if SPECDEC_NO_DIRECT / SPECDEC_NO_PIPE were set
GemmPlan gemm_plan(int T, int n_pairs, int K, bool w8, int prologue, int epi, int flags);
int gemm_plan_name(const GemmPlan& pl, int epi, bool w8, char* out, size_t cap);   // snprintf's return value
int launch_gemm_pipe(const GemvArgs& a, const GemvGeom& q, const GemmPlan& pl, int epi, hipStream_t st);

// ---- attention over the appended KV cache (attention.hip) -------------------------
struct AttnArgs {
  // line 0 (64 bytes): everything a short-context launch reads (see GemvArgs on why the order matters)
  const void* q;        // bf16 [T][n_q_heads*head_dim]
  const void* k_cache;  // bf16 [B][n_kv_heads][l_max][head_dim]
  const void* v_cache;
  void* out;            // bf16 [T][n_q_heads*head_dim]
  const int32_t* pos_base;
  const int32_t* skip_k;   // per-row adaptive K, as GemvArgs
  int pos_off;
  int l_max;
  float scale;
  unsigned M : 8, n_q_heads : 8, n_kv_heads : 8, n_split : 8;   // n_split: set by launch_attention
  // line 1
  unsigned head_dim : 8, page_shift : 8, skip_i : 4;
  int B;
  // split-KV over workgroups for long contexts (attention.hip): partial (max, sum, O) tiles and one
  // arrival counter per (row, kv head, query tile); null / 0 = every tile is one workgroup
  float* split_ws;
  unsigned* split_cnt;
  int split_slots;      // partial tiles the workspace holds
  const int32_t* block_table;   // paged KV, as GemvArgs (null = dense rows of l_max positions)
};
int launch_attention(const AttnArgs& a, hipStream_t st);
constexpr int kAttnSplitSlots = 1024;   // partial tiles of the split-KV workspace
// The geometry of one attention launch, decided on the host from dimensions alone: launch_attention consults it and
// sd_attention_plan (plan_query.hip) reports it. tiles: 16-row query tiles per (row, kv head); n_split: workgroups per tile
// (1 = no split-KV); grid = (n_kv_heads, B, tiles * n_split). page_shift < 0: a dense cache. has_split_ws: the launch has a
// partial-tile workspace of split_slots tiles and its arrival counters. Refuses what launch_attention refuses, in its words.
struct AttnPlan { int tiles, n_split, grid_x, grid_y, grid_z; };
int attention_plan(int n_q_heads, int n_kv_heads, int head_dim, int B, int M, int l_max, int page_shift, bool has_split_ws,
                   int split_slots, AttnPlan& plan);
size_t attention_split_ws_bytes(int head_dim);   // workspace for kAttnSplitSlots partial tiles (+ counters)
size_t attention_split_tiles_bytes(int head_dim);   // the partial tiles of it (split_ws); the kAttnSplitSlots counters (split_cnt) follow

// ---- small kernels (misc.hip) -------------------------------------------------------
struct EmbedArgs {
  const void* tok_emb;   // bf16 [vocab][d]
  const void* pos_emb;   // bf16 [max_pos][d] or null
  const int32_t* tokens; // device, token (b,m) at tokens[b*tok_stride + m]
  int tok_stride;
  const int32_t* pos_base;
  int pos_off, M, T, d, vocab, max_pos;
  void* x;               // bf16 [T][d]
  const int32_t* skip_k;   // as GemvArgs
  int skip_i;
};
int launch_embed(const EmbedArgs& a, hipStream_t st);

// reduce the per-workgroup argmax partials: ids[b*ids_stride + m] = argmax over grid
int launch_argmax_finalize(const float* part_val, const int* part_idx, int T, int grid, int M,
                           int ids_stride, int32_t* ids_out, hipStream_t st, const int32_t* skip_k = nullptr, int skip_i = 0);

// ---- KV fork (kv_fork.hip) ------------------------------------------------------------
// First n_pos positions of slot src[g] -> slots dst[g * fan .. g * fan + fan), all layers / heads / K and V; a slot is a
// row of a dense cache (Lslot = Lmax) or a page of a pool (Lslot = page_len). n_groups == 1: one source, any fan;
// n_groups > 1: pairs (fan == 1). Lists are host memory; launches carry <= kForkMaxList entries each.
constexpr int kForkMaxList = 64;
int launch_kv_fork(uint16_t* k, uint16_t* v, int n_layers, int n_slots, int Hkv, int Lslot, int D, const int32_t* src,
                   const int32_t* dst, int n_groups, int fan, int n_pos, hipStream_t st);

// ---- KV eviction (kv_evict.hip) ---------------------------------------------------------
// Row `row` of a dense cache, in place: positions [keep + drop, n_pos) -> [keep, n_pos - drop), all layers / heads; V bit
// for bit, K rotated by -drop with row `drop` of the fp32 tables rope_cos / rope_sin ([max_pos][D / 2]). drop % 8 == 0.
int launch_kv_evict(uint16_t* k, uint16_t* v, const float* rope_cos, const float* rope_sin, int n_layers, int B, int Hkv, int Lmax, int D,
                    int row, int keep, int drop, int n_pos, hipStream_t st);

}  // namespace sd
