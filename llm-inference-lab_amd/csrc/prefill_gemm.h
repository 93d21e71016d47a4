// Prompt prefill as library GEMMs + this repo's norm / epilogue / attention kernels (csrc/prefill_gemm.hip). Internal interface.
#pragma once

#include <vector>

#include "kernels.h"

namespace sd {

constexpr int kPrefillChunk = 512;   // positions per GEMM chunk (workspace: ~110 KiB per position at Llama-3.2-3B dimensions)
// Shorter passes keep the decode-shaped kernels: the GEMM path's ~14 launches per layer cost ~4.5 ms for the 3B + 1B pair before the
// first product (160 tokens 5.9 ms, 192 6.2, 256 6.4, 512 8.9), the decode-shaped passes 5.0 / 7.1 / 9.3 ms at 64 / 96 / 128 tokens
// (profiles/round4_context_scaling.md): they cross below 96.
constexpr int kPrefillMinTokens = 96;

// ---- the native GEMM over the packed tile streams (csrc/prefill_mfma.hip) ----------------------------------------------------
struct NativeMat {          // one matrix shape of a layer, split into row blocks of whole packed tiles
  const int4* tiles;        // device: {first row in its block, pairs, first pair, 0} per tile
  const int2* blocks;       // device: {first tile, tiles} per row block
  int n_blocks, rb;         // row blocks; rows per block (128 or 64)
  int N, K, n_pairs, epi;
};
struct NativePlan {
  NativeMat mat[5][2];      // [qkv, out, gate / up, down, lm_head][128-row blocks, 64-row blocks]
  bool layers = false;      // the four layer shapes are built (prefill_native_shapes_ok); the lm_head is built whenever d_model % 64 == 0
  int head_dim = 0;
  void* buf = nullptr;      // device tables of all of them
};
bool prefill_native_shapes_ok(const sd_model_config& c);     // Llama, every K a multiple of 64
// The one rule that admits a model to the native backend: null, or why not (sd_model_set_prefill_backend refuses with it,
// sd_prefill_plan reports it). packed: the model has the packed weight streams.
const char* prefill_native_refusal(const sd_model_config& c, bool packed);
// The host half of the plan: every shape's tiles in stream order and its row blocks of both heights, as the device tables hold
// them (block tile indices are absolute). No device work: native_plan_build uploads it, sd_prefill_plan reads it.
struct NativeTables {
  struct Span { size_t tiles, blocks; int n_blocks; };
  std::vector<int4> tiles;     // {first row in its block, pairs, first pair, 0}
  std::vector<int2> blocks;    // {first tile, tiles}
  Span spans[5][2] = {};       // [shape][128-row blocks, 64-row blocks]
  bool layers = false;         // the four layer shapes are present (else the lm_head alone)
};
int native_plan_tables(const sd_model_config& c, NativeTables& t);
// Block height of one product: 0 = 128-row blocks (RF = 4) unless they would fill fewer than the CUs (one workgroup per CU, two
// resident), else 1 = 64-row blocks (RF = 2). n_blocks_128: the shape's row blocks of 128 rows; n_tb: token blocks of the chunk.
inline int native_block_variant(int n_blocks_128, int n_tb) { return n_blocks_128 * n_tb >= 256 ? 0 : 1; }
// Workgroup blockIdx.x of a grid of G -> linear (row block, token block) index rb * n_tb + tb: the token blocks of one row block are
// consecutive on one XCD (dispatch is round-robin over the 8 XCDs), so a weight piece is fetched from HBM once and shared through
// that XCD's L2. A grid that is no multiple of 8 keeps the launch order.
__host__ __device__ inline int native_block_of(int wg, int G) { return (G & 7) == 0 ? (wg & 7) * (G >> 3) + (wg >> 3) : wg; }
// What launch_prefill_mfma runs for product `which` (0 qkv, 1 out, 2 gate / up, 3 down) over T <= kPrefillChunk rows (sd_prefill_plan)
struct PrefillPlanInfo {
  int variant;                 // 0: 128-row blocks, 1: 64-row blocks
  int first_block, n_blocks;   // the row blocks: NativeTables::blocks[first_block ...]
  int n_tb, grid, swizzled;
  int last_tb_rows;            // rows of the last token block (1 .. 128)
  int min_block_rows;          // fewest packed rows any row block holds (blocks are whole tiles)
  int k_stages;                // 64-k stages of the main loop
};
PrefillPlanInfo native_plan_info(const NativeTables& t, const sd_model_config& c, int which, int T);
// the layer shapes where prefill_native_shapes_ok, and the lm_head (N = vocab, K = d_model, pairs (2p, 2p + 1); either arch)
int native_plan_build(const sd_model_config& c, NativePlan& plan);
void native_plan_free(NativePlan& plan);
// Y[T][N] fp32 (HF row order) = X[T][K] x W^T, W = the packed stream of matrix `which` (0 qkv, 1 out, 2 gate / up, 3 down) of a layer
int launch_prefill_mfma(const NativePlan& plan, int which, const void* W, const float* w_scale, bool w8, const uint16_t* X, int ldx, float* Y,
                        int T, hipStream_t st);

// ---- sd_model_score's head (csrc/score_head.hip): the lm_head of the native plan with a log-softmax / argmax epilogue ----------------
// bytes of the partials of kPrefillChunk tokens (either row-block size)
size_t score_partial_bytes(const NativePlan& plan);
// Xn: T <= kPrefillChunk normed rows (bf16 [T][d_model]). target[t] (t < n_target): the row whose logit gives logprob[t] = l_target - lse;
// greedy[t] = argmax row (either may be null). part / tgt_logit: score_partial_bytes / T floats of workspace.
// logits != null (sd_model_score_logits): every token's logits are stored as bf16 [T][vocab] as well, greedy as before, and target /
// logprob are not used.
int launch_score_head(const NativePlan& plan, const void* W, const float* w_scale, bool w8, const uint16_t* Xn, int T, const int32_t* target,
                      int n_target, float4* part, float* tgt_logit, float* logprob, int32_t* greedy, uint16_t* logits, hipStream_t st);

enum PrefillGemm { PREFILL_GEMM_ROCBLAS = 0, PREFILL_GEMM_NATIVE = 1 };

struct PrefillModel {
  const sd_model_config* cfg;
  uint16_t* k_cache;    // dense: [layer][B][Hkv][Lmax][D]; paged: page pools [layer][pages][Hkv][P][D]
  uint16_t* v_cache;    // dense: [layer][B][Hkv][D][Lmax]; paged: [layer][pages][Hkv][D][P]
  int B, Lmax;
  float* attn_ws;       // split-KV workspace of the attention kernel
  unsigned* attn_cnt;
  // paged KV (sd_model_bind_paged): null = dense rows
  const int32_t* block_table = nullptr;   // [B][max_pages]
  int page_shift = 0, max_pages = 0, n_pages = 0;
  // matrix product: rocBLAS over the HF-layout bf16 weights, or the native GEMM over the packed streams
  int gemm = PREFILL_GEMM_ROCBLAS;
  const void* const* packed = nullptr;    // native: per matrix (4 per layer + lm_head, packing order)
  const float* const* scales = nullptr;   // native, fp8 storage: fp32 row scales per matrix (else null)
  const NativePlan* plan = nullptr;
};

bool prefill_gemm_available();                               // rocBLAS could be opened (dlopen at first use) and a handle created
bool prefill_gemm_library_present();                         // rocBLAS could be opened (dlopen only: no device work)
size_t prefill_gemm_workspace_bytes(const sd_model_config& c);
// the chunk's rows of the last layer, left in the prefill workspace: residual stream [Mc][d_model], q after RoPE and attention
// rows [Mc][Hq*D], MLP activation [Mc][d_ff]
struct PrefillRows {
  uint16_t* x = nullptr;
  uint16_t* q = nullptr;
  uint16_t* attn = nullptr;
  uint16_t* act = nullptr;
};
// the final norm of the model over n residual rows (bf16, rows ldx apart) -> bf16 [n][d_model]: Llama RMSNorm with the rounding points
// of the GEMV prologue (rms_rows_kernel), GPT-2 LayerNorm in fp32 rounded once (layernorm_pair)
int launch_final_norm_rows(const sd_model_config& c, const uint16_t* x, int ldx, int n, uint16_t* out, hipStream_t st);
int prefill_gemm_chunk(const PrefillModel& m, const int32_t* tokens, const int32_t* pos_base_row, int pos_off, int cache_row, int Mc, void* ws,
                       PrefillRows* rows_out, hipStream_t st);

}  // namespace sd
