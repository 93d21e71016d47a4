// Prompt prefill as library GEMMs + this repo's norm / epilogue / attention kernels (csrc/prefill_gemm.hip). Internal interface.
#pragma once

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
