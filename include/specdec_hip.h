/*
 * specdec_hip.h — C-ABI of the MI355X (gfx950) speculative-decoding hot path.
 *
 * This is the drop-in boundary for GogoRit/llm-inference-lab's kernel registry
 * (`src/kernels/registry.py:11-123`, ops "verify_prefix" and "kv_append",
 * `src/kernels/__init__.py:84-112`) and for the model-wrapper forward that the
 * pipeline calls through `LanguageModel.generate_tokens`
 * (`src/specdec/utils/interfaces.py:14-138`, call sites
 * `src/specdec/core/pipeline.py:2397, 2585`).
 *
 * Conventions
 *   - plain pointers + sizes only; no torch / STL types cross this boundary
 *   - every pointer named `*_dev`, `logits`, `ids`, cache/new/out is DEVICE memory
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream)
 *   - every entry point returns 0 on success, non-zero on error; the message is
 *     available from sd_last_error() (thread-local); nothing throws
 *   - no allocation, no synchronisation and no host<->device copy inside an
 *     entry point unless its comment says so: all of them are graph-capturable
 *   - inputs are borrowed and never written; outputs are caller-owned
 */
#ifndef SPECDEC_HIP_H
#define SPECDEC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* element types (values are part of the ABI) */
enum sd_dtype {
  SD_F32 = 0,
  SD_F16 = 1,
  SD_BF16 = 2,
  SD_I32 = 3,
  SD_I64 = 4,
  SD_U8 = 5,
  SD_FP8_E4M3 = 6
};

#define SD_ABI_VERSION 1

/* ABI version of the loaded library (== SD_ABI_VERSION it was built with). */
int sd_abi_version(void);

/* Last error message of the calling thread ("" if none). Never NULL. */
const char* sd_last_error(void);

/* ------------------------------------------------------------------------
 * verify_prefix — replaces the registry op "verify_prefix"
 *   reference contract: verify_prefix_ref, src/kernels/reference.py:13-56
 *   reference callers : LongestPrefixPolicy.accept_tokens, policies.py:128-134
 *   (the dead CUDA attempt it supersedes: src/kernels/cuda/verify.cu:34-215)
 *
 *   pred[b,k]      = argmax_v logits[b,k,v]      (lowest index wins ties, NaN
 *                                                 counts as the maximum — the
 *                                                 torch.argmax rule)
 *   accept_len[b]  = length of the longest prefix with pred[b,k] == ids[b,k]
 *   mask[b,k]      = 1 for k < accept_len[b], else 0   (prefix-only mask)
 *
 *   logits  : [B][K][V], dtype SD_F32 | SD_F16 | SD_BF16, last dim contiguous,
 *             element strides stride_b / stride_k
 *   ids     : [B][K] contiguous, dtype SD_I32 | SD_I64
 *   pred_out: optional [B][K] int32 (NULL to skip) — the argmax ids
 *   workspace: device scratch of at least sd_verify_prefix_workspace(B,K,V) bytes
 * ------------------------------------------------------------------------ */
size_t sd_verify_prefix_workspace(int B, int K, int V);

int sd_verify_prefix(const void* logits, int logits_dtype,
                     const void* ids, int ids_dtype,
                     int32_t* accept_len, uint8_t* mask, int32_t* pred_out,
                     int B, int K, int V,
                     int64_t stride_b, int64_t stride_k,
                     void* workspace, size_t workspace_bytes,
                     void* stream);

/* Sampled token from logits rows: temperature -> top-k -> top-p -> one categorical draw.
 * Replaces sample_bonus_token_from_logits (src/specdec/core/pipeline.py:48-147) for
 * do_sample=True. Entry b reads row  b*rows_per_b + (pos ? pos[b] : 0)  of `logits`
 * ([rows][V], row_stride elements apart, f32 / bf16 / f16) and writes out_ids[b]; entries with
 * active[b] == 0 (if given) are skipped. Order among equal logits: value descending, index
 * ascending. The nucleus cut drops a token when the inclusive cumulative probability (descending
 * order, inside the top-k) exceeds top_p; the first token is always kept. The draw is one
 * Philox4x32-10 value with key = seed and counter = (draw index, stream, 0, tag), inverted through
 * the cumulative weights; draw index = draw_counters[b] (then incremented) or draw0 when
 * draw_counters is NULL; stream = stream_id[b] or b. top_k in 1..1024; top_k <= 0 with
 * top_p >= 1 draws from the whole row (Gumbel-max, one Philox value per element); top_k <= 0
 * with top_p < 1 is the full-vocabulary nucleus (the reference with top_k = None): the row is
 * consumed in rank blocks of 1024 (exact radix select per block) until the cumulative probability
 * — over the softmax of the WHOLE row — passes top_p. Asynchronous on `stream`, no allocation, graph-capturable. */
int sd_sample_token(const void* logits, int logits_dtype, int64_t row_stride, int B, int V,
                    const int32_t* pos, int rows_per_b, const int32_t* active, float temperature,
                    int top_k, float top_p, uint64_t seed, uint32_t* draw_counters, uint32_t draw0,
                    const int32_t* stream_id, int32_t* out_ids, void* stream);

/* Steps 3 and 4 of speculative sampling (sd_specdec_set_spec_sampling) on caller tensors: draft_logits [B][K][V] and
 * target_logits [B][K+1][V], bf16 contiguous; draft_ids [B][K] int32 (the tokens drawn from q_i; clamped to [0, V)).
 * Draw counter of row b = draw_counters[b] (then advanced by K + 1) or draw0 when draw_counters is NULL; rows with
 * active[b] == 0 (nullable) are skipped: accept_len_out[b] = 0, nothing else written, no draws consumed. Outputs:
 * accept_len_out [B], next_tok_out [B], ratios_out (nullable, float64 [B][K]: ratio_i of every position, NaN for a
 * non-finite position). K in 1..63. workspace: sd_spec_sample_workspace(B, K) bytes of device scratch.
 * Asynchronous on `stream`, no allocation, graph-capturable. */
size_t sd_spec_sample_workspace(int B, int K);
int sd_spec_sample_accept(const void* draft_logits, const void* target_logits, const int32_t* draft_ids, int B, int K, int V,
                          float temperature, uint64_t seed, uint32_t* draw_counters, uint32_t draw0,
                          const int32_t* stream_ids, const int32_t* active, int32_t* accept_len_out, int32_t* next_tok_out,
                          double* ratios_out, void* workspace, size_t workspace_bytes, void* stream);

/* The same steps for the SHAPED mode (sd_specdec_set_spec_shaping): sd_spec_sample_accept's arguments plus top_k (1..1024,
 * clamped to V) and top_p (> 0; >= 1: no nucleus cut); the same workspace function. Steps 2-4 of the shaped definition below:
 * the acceptance uniform of position i is the Philox value of counter (c + i, sid, 0, 0x5EED0003), the next token inverts the
 * uniform of counter (c + K, sid, 0, CDF tag). ratios_out: (e_p(d)/Z_p) / (e_q(d)/Z_q); 0 when d is outside the target's kept
 * set, NaN (rejected) when d is outside the draft's. Refused: top_k <= 0 (top_p without top_k, the full-vocabulary nucleus, is
 * not supported; the unshaped op is sd_spec_sample_accept), top_k > 1024, top_p <= 0 or NaN. */
int sd_spec_sample_accept_shaped(const void* draft_logits, const void* target_logits, const int32_t* draft_ids, int B, int K, int V,
                                 float temperature, int top_k, float top_p, uint64_t seed, uint32_t* draw_counters, uint32_t draw0,
                                 const int32_t* stream_ids, const int32_t* active, int32_t* accept_len_out, int32_t* next_tok_out,
                                 double* ratios_out, void* workspace, size_t workspace_bytes, void* stream);

/* Lossy acceptance on the verify pass's logits (csrc/typical_accept.hip): a draft token is kept when the target finds it plausible
 * enough. target_logits: [B][K+1] rows of V elements (f32 / bf16 / f16), row_stride elements apart (>= V), row (b, i) = row
 * b * (K + 1) + i: the target's distribution after d_1..d_i, where d_{i+1} = draft_ids[b][i] was proposed (row K is not read).
 * Per row, one pass in fp32 with z = logit / T: H = log S - W / S over S = sum e^{z - m}, W = sum (z - m) e^{z - m} (a -inf element
 * adds exactly 0 to both), p_d = e^{z_d - m} / S (0 for a -inf logit) and rank_d = #{v : z_v > z_d, or z_v == z_d and v < d}.
 *   rule SD_ACCEPT_TYPICAL     keep d iff p_d >= min(epsilon, delta * exp(-H)); delta = +inf: the fixed threshold epsilon
 *   rule SD_ACCEPT_TOPK_AGREE  keep d iff rank_d < agree_k (agree_k = 1: d is the row's argmax, ties to the lower index)
 * accept_len[b] = the number of leading kept positions. A draft id outside [0, V) and a row holding NaN or +inf are rejected.
 * stats (nullable, float [B][K][4]): p_d, H, the threshold (rule 2: agree_k), rank_d of every position. Bit-identical run to run.
 * workspace: sd_typical_accept_workspace(B, K, V) bytes of device scratch, 4-byte aligned. Asynchronous on `stream`, no allocation,
 * graph-capturable. Refused (nonzero + sd_last_error, before any device work): an unknown rule, temperature not > 0, epsilon outside
 * (0, 1], delta <= 0 or NaN (rule 1), agree_k outside 1..V (rule 2), K outside 1..63, a NULL pointer, a short workspace. */
enum sd_accept_rule { SD_ACCEPT_OFF = 0, SD_ACCEPT_TYPICAL = 1, SD_ACCEPT_TOPK_AGREE = 2 };
size_t sd_typical_accept_workspace(int B, int K, int V);
int sd_typical_accept(const void* target_logits, int logits_dtype, int64_t row_stride, const int32_t* draft_ids, int B, int K, int V,
                      int rule, float temperature, float epsilon, float delta, int agree_k, int32_t* accept_len, float* stats,
                      void* workspace, size_t workspace_bytes, void* stream);

/* The confidence of a logits row (csrc/draft_confidence.hip): conf[b] = 1 / sum_v exp(x_v - max_v x_v) over the STORED values of
 * row b — the softmax probability, at temperature 1, of the row's largest value. logits: B rows of V elements (f32 / f16 /
 * bf16), row_stride elements apart (>= V); a row need not be 16-byte aligned (aligned rows take 16-byte loads). An element at
 * -inf adds 0; a row whose maximum is not finite (+inf, or every element -inf) or that holds a NaN gives NaN. fp32, the
 * running-maximum stream and merge order of sd_typical_accept's row pass (one 1024-thread workgroup per row, the wave xor tree,
 * then the 16 wave partials in order): bit-identical run to run, no atomics, no waiting. The confidence-gated step
 * (sd_specdec_set_draft_confidence) runs the same device function on the draft's rows. Asynchronous on `stream`, no allocation,
 * graph-capturable. Refused: a NULL pointer, an unknown dtype, B outside 1..65535, V < 1, a stride below V, a misaligned conf.
 * Additive (SD_ABI_VERSION stays 1). */
int sd_draft_confidence(const void* logits, int logits_dtype, int64_t row_stride, int B, int V, float* conf, void* stream);

/* Per-token log-probs and top-N alternatives of logits rows (csrc/token_logprobs.hip). logits: R rows of V elements (f32 / f16 /
 * bf16), row_stride elements apart (>= V); a row need not be 16-byte aligned (aligned rows take 16-byte loads). For row r and its
 * token t = token_ids[r], over the STORED values x at temperature 1, in fp32, with m = max_v x_v and S = sum_v e^{x_v - m} (an
 * element at -inf adds exactly 0):
 *   out_logprob[r]        (x_t - m) - log S; -inf for a token at -inf
 *   out_rank[r]           #{v : x_v > x_t, or x_v == x_t and v < t}: the ties of the argmax kernels, 0 = t is the row's argmax
 *   out_top_ids[r][j], out_top_logprob[r][j], j < N = min(top_n, V): the N largest entries, value descending, index ascending;
 *                         entries at -inf (fewer than N finite ones) follow in that order with log-prob -inf
 * A row with no finite element, and a token id outside [0, V) (never read), give logprob NaN, rank -1, top ids -1 with log-prob NaN.
 * One 1024-thread workgroup per row, the running-maximum stream and merge order of sd_typical_accept's row pass: bit-identical run
 * to run and under graph replay, no global atomics, no waiting. top_n = 0 skips the selection (the top outputs may be NULL).
 * Asynchronous on `stream`, no allocation, graph-capturable. Refused (nonzero + sd_last_error, before any device work): a NULL
 * pointer, an unknown dtype, R < 1, V < 1 or above 2^20, top_n outside 0..20, a stride below V, a misaligned output.
 * Additive (SD_ABI_VERSION stays 1). */
int sd_token_logprobs(const void* logits, int logits_dtype, int64_t row_stride, int R, int V, const int32_t* token_ids, int top_n,
                      float* out_logprob, int32_t* out_rank, int32_t* out_top_ids, float* out_top_logprob, void* stream);

/* Draft-target agreement of two logit blocks (csrc/spec_agree.hip): how much of the target's distribution a draft reproduces,
 * position by position, without generating. draft_logits / target_logits: bf16, n rows of V elements, rows ld_q / ld_p
 * elements apart (>= V). Per row t, in float64 over the stored bf16 values, x / T as sd_spec_sample_accept forms it (T the
 * float32 temperature widened to double, no division when T == 1), a_v = P[t][v]/T - lse(P[t]/T), b_v likewise from Q:
 *   alpha[t] = sum_v min(exp a_v, exp b_v)   the acceptance probability of speculative sampling at that position, 1 - TV(p, q)
 *   kl[t]    = sum_v exp(a_v) (a_v - b_v)    KL(p || q) over the v with P[t][v] > -inf; +inf when q(v) = 0 under p(v) > 0
 *   p_arg[t], q_arg[t]                       argmax ids (NaN first, larger value, lower index); agree[t] = (p_arg == q_arg)
 * A row pair with a NaN in either row, or a maximum that is not finite, gives alpha = kl = NaN. Every output may be NULL.
 * Bit-identical run to run; row t's outputs do not depend on n or on the other rows. workspace: sd_spec_agreement_workspace(n, V)
 * bytes of device scratch, 16-byte aligned. Asynchronous on `stream`, no allocation, graph-capturable. Refused (nonzero +
 * sd_last_error, before any device work): NULL logits, n < 1 or V < 1, a stride below V, temperature not > 0 or NaN, a short or
 * misaligned workspace. */
size_t sd_spec_agreement_workspace(int n, int V);
int sd_spec_agreement(const void* draft_logits, int64_t ld_q, const void* target_logits, int64_t ld_p, int n, int V, float temperature,
                      double* alpha, double* kl, int32_t* agree, int32_t* p_arg, int32_t* q_arg, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * kv_append (in place) — the KV-append path
 *   reference contract: kv_append_ref, src/kernels/reference.py:59-93
 *   reference callers : HFWrapper._append_kv_with_kernel, hf_wrappers.py:985-1029;
 *                       SafeKVCacheManager.update_*_cache, kv_cache_manager.py:194-273
 *
 *   cache_k/v : [B][H][Lmax][D] preallocated, contiguous
 *   new_k/v   : [B][H][K][D] contiguous
 *   row_len   : optional device int32[B]: row b is appended at row_len[b];
 *               NULL → every row is appended at `L`
 *   Rows [row_len[b], row_len[b]+K) of the cache are written; nothing else is
 *   touched, so views of the first row_len[b] rows stay valid (the
 *   `torch.cat` of the reference re-copies all L rows instead).
 *   elem_size : bytes per element (2 or 4); the copy is type-agnostic
 * ------------------------------------------------------------------------ */
int sd_kv_append(void* cache_k, void* cache_v,
                 const void* new_k, const void* new_v,
                 const int32_t* row_len, int L,
                 int elem_size, int B, int H, int Lmax, int K, int D,
                 void* stream);

/* ------------------------------------------------------------------------
 * kv_concat (out of place) — exact output shape of the registry op "kv_append"
 *   out[b,h,0:L]   = base[b,h,0:L]
 *   out[b,h,L:L+K] = new[b,h,0:K]          out: [B][H][out_cap][D], out_cap >= L+K
 *   (out_cap == L+K gives the contiguous reference shape; a larger out_cap lands
 *    the result in a cache with head-room for later in-place appends)
 *   base may be a strided view: element strides base_sb / base_sh, rows of D
 *   contiguous elements at stride D. K and V are moved by one launch.
 * ------------------------------------------------------------------------ */
int sd_kv_concat(void* out_k, void* out_v,
                 const void* base_k, const void* base_v,
                 const void* new_k, const void* new_v,
                 int elem_size, int B, int H, int L, int K, int D, int out_cap,
                 int64_t base_sb, int64_t base_sh,
                 void* stream);

/* ------------------------------------------------------------------------
 * kv_append_masked — compacting append
 *   reference contract: kv_append_with_mask_ref, src/kernels/reference.py:96-159
 *   (supersedes src/kernels/cuda/kv_cache.cu:14-173, including its zero-accept
 *    bug at :40 — a zero-accept row keeps its base rows here, as the reference
 *    test tests/test_kv_cache.py:164-186 requires)
 *
 *   out : [B][H][L+K][D] contiguous; every element is written:
 *         rows [0,L)          = base
 *         rows L+j, j<n_b     = draft row of the j-th set bit of mask[b,:]
 *         rows L+n_b .. L+K-1 = 0
 *         n_b = accept_len[b]==0 ? 0 : min(popcount(mask[b,:]), accept_len[b] < 0 ? 1 : accept_len[b])
 *               (a negative accept_len is invalid input; the reference loop writes one row for it, so does this)
 *   mask : device uint8[B][K] (K <= 64), accept_len : device int32[B]
 * ------------------------------------------------------------------------ */
int sd_kv_append_masked(void* out_k, void* out_v,
                        const void* base_k, const void* base_v,
                        const void* draft_k, const void* draft_v,
                        const uint8_t* mask, const int32_t* accept_len,
                        int elem_size, int B, int H, int L, int K, int D,
                        int64_t base_sb, int64_t base_sh,
                        void* stream);

/* ========================================================================
 * Decoder forward + draft-then-verify loop
 *
 * The reference reaches the model through LanguageModel.generate_tokens
 * (src/specdec/utils/interfaces.py:30-62; HFWrapper._generate_tokens_async,
 * src/specdec/models/hf_wrappers.py:272-627 — one HF forward per generated token,
 * argmax of the last position) and drives it from the step loop of
 * SpeculativePipeline.generate_batch / generate (src/specdec/core/pipeline.py:
 * 1984-3733, 984-1275). These entry points are what a ctypes binding of that path
 * binds instead: a model instance over caller-owned weights and caches, a forward
 * that appends to the KV cache in place, and one call per draft-then-verify step.
 * ======================================================================== */

enum sd_arch { SD_ARCH_LLAMA = 0, SD_ARCH_GPT2 = 1 };

/* Per-layer weights. Linear weights are [out_features][in_features] row-major
 * (HF nn.Linear layout), bf16. Biases / LayerNorm biases may be NULL (Llama). */
typedef struct sd_layer_weights {
  const void* attn_norm_w;  /* [d]  input_layernorm / ln_1 */
  const void* attn_norm_b;  /* [d]  GPT-2 only */
  const void* wqkv;         /* [(Hq+2*Hkv)*D][d]  q rows, then k rows, then v rows */
  const void* bqkv;
  const void* wo;           /* [d][Hq*D] */
  const void* bo;
  const void* mlp_norm_w;   /* [d]  post_attention_layernorm / ln_2 */
  const void* mlp_norm_b;
  const void* w_up;         /* Llama: [2*ff][d] gate rows then up rows; GPT-2: c_fc [ff][d] */
  const void* b_up;
  const void* w_down;       /* [d][ff] */
  const void* b_down;
} sd_layer_weights;

typedef struct sd_model_config {
  int arch;                 /* enum sd_arch */
  int n_layers, d_model, n_heads, n_kv_heads, head_dim, d_ff, vocab, max_pos;
  float norm_eps;
  int weight_dtype;         /* SD_BF16: stream the matrices as given. SD_FP8_E4M3: the matrices are still passed as
                             * bf16; sd_pack_weights quantises them (OCP e4m3, per-output-row absmax/448 scale) into
                             * `packed` and the forward streams that copy: half the HBM bytes, bf16 activations */
  const void* tok_emb;      /* [vocab][d] */
  const void* pos_emb;      /* [max_pos][d], GPT-2 only */
  const void* final_norm_w; /* [d] */
  const void* final_norm_b;
  const void* lm_head;      /* [vocab][d] (may alias tok_emb) */
  const float* rope_cos;    /* [max_pos][D/2] fp32, Llama only */
  const float* rope_sin;
  const sd_layer_weights* layers; /* host array [n_layers] (copied by sd_model_create) */
  const void* packed;       /* optional: buffer written by sd_pack_weights for THIS config; the
                               GEMVs then stream the packed copy (the row-major matrices are no
                               longer read by the forward, except tok_emb for the gather). A bf16 model
                               may add a lossless 12-bit copy of it for the launches of 1..9 tokens
                               (sd_model_set_w12); `packed` stays what every other launch reads */
} sd_model_config;

/* The weight quantiser of the fp8 storage mode on a row-major bf16 matrix [N][K]:
 * scales[r] = max|w[r][:]| / 448 (1 for an all-zero row), q[r][k] = OCP e4m3 (round to nearest even) of
 * w[r][k] / scales[r]. sd_pack_weights applies exactly this before re-ordering. Asynchronous on `stream`. */
int sd_quantize_fp8_rows(const void* w_bf16, int N, int K, void* q_fp8, float* scales, void* stream);

/* One vocabulary-sized output matrix [vocab][d_model] (bf16, row-major) outside a model — a Medusa head — in the
 * engine's tile-stream order, bf16 or fp8 e4m3 with row scales (the lm_head's layout and quantiser). */
size_t sd_packed_head_bytes(int vocab, int d_model, int weight_dtype);
int sd_pack_head(const void* w_bf16, int vocab, int d_model, int weight_dtype, void* dst, size_t dst_bytes, void* stream);

/* Weight pre-packing: the engine's private copy of all Linear weights in the order the
 * streaming GEMV consumes them (csrc/pack.hip), so that every wave reads one contiguous
 * region of HBM. sd_packed_bytes gives the buffer size (device memory, 256-byte aligned);
 * sd_pack_weights fills it (asynchronous on `stream`). */
size_t sd_packed_bytes(const sd_model_config* cfg);
int sd_pack_weights(const sd_model_config* cfg, void* dst, size_t dst_bytes, void* stream);

typedef struct sd_model sd_model;

/* Create a model over caller-owned device weights (borrowed for the model's life). */
int sd_model_create(const sd_model_config* cfg, sd_model** out);
int sd_model_destroy(sd_model* m);

/* W12: an ADDITIONAL, lossless copy of a bf16 model's packed matrices at ~0.76 of their bytes, streamed by the launches
 * of 1..9 tokens (csrc/gemv.hip) in place of `packed`; every other reader (launches of more than 9 tokens, prefill, the
 * persistent forward) keeps `packed`, and fp8 models have no W12 copy. Every (tile, 32-k step) block of a packed stream
 * whose exponents fit a 16-value window is stored as 12-bit codes (sign, 4-bit exponent offset, mantissa) that widen to
 * exactly the bf16 bits; other blocks stay raw (format: csrc/pack.hip, restated in specdec_hip/w12.py). Results are
 * bit-identical with and without the copy. Built once per model, in three steps (cfg->packed: the bf16 buffer of
 * sd_pack_weights; n_wide: HOST uint32 [4 * n_layers + 1], the wide-block count of every matrix):
 *   sd_w12_measure   classifies and numbers the blocks of every matrix into `scratch` (device, 256-byte aligned,
 *                    sd_w12_scratch_bytes) and returns the counts; synchronises `stream`.
 *   sd_w12_bytes     size of the copy. A matrix takes part when its W12 bytes are at least 15 % below its packed bf16
 *                    bytes and the W12 kernels cover its shape (whole 32-k steps per K slice); others contribute nothing.
 *   sd_w12_pack      writes the copy to dst (device, 256-byte aligned); asynchronous on `stream`; scratch may be freed
 *                    once it has run.
 * sd_w12_matrix reports matrix `index` (4 * layer + 0 qkv / 1 out / 2 gate-up / 3 down; 4 * n_layers = the lm_head):
 * whether it takes part, its offset in the copy, the padded bytes of its main stream, overflow and table, its table
 * entries (blocks) and its packed bf16 bytes; any out pointer may be NULL.
 * sd_model_set_w12 hands the copy to a model created from the same config (borrowed for the model's life; NULL: back to
 * the bf16 streams). classes: which matrix classes read it, bit 0 qkv, 1 out, 2 gate / up, 3 down, 4 lm_head; the other
 * classes keep their bf16 stream. SD_W12_DEFAULT_CLASSES is what the measurements kept. SPECDEC_NO_W12 in the environment keeps every launch on the bf16 stream (read per launch). */
size_t sd_w12_scratch_bytes(const sd_model_config* cfg);
int sd_w12_measure(const sd_model_config* cfg, void* scratch, size_t scratch_bytes, uint32_t* n_wide, void* stream);
size_t sd_w12_bytes(const sd_model_config* cfg, const uint32_t* n_wide);
int sd_w12_matrix(const sd_model_config* cfg, const uint32_t* n_wide, int index, int* taken, size_t* offset, size_t* main_bytes,
                  size_t* ovf_bytes, size_t* table_bytes, size_t* blocks, size_t* bf16_bytes);
int sd_w12_pack(const sd_model_config* cfg, const void* scratch, const uint32_t* n_wide, void* dst, size_t dst_bytes, void* stream);
#define SD_W12_SKIP 0xFFFFFFFFu          /* n_wide[i] = SD_W12_SKIP (set by the caller after sd_w12_measure): matrix i is left out of the copy */
#define SD_W12_DEFAULT_CLASSES 0x10u   /* the lm_head: the one class the 5-token probes of 3B shapes found faster (profiles/w12_verify.md) */
int sd_model_set_w12(sd_model* m, const void* w12, const uint32_t* n_wide, unsigned classes);

/* W12S, the split-byte FORM of the W12 copy: same blocks, slots, overflow stream, table and sizes per wide-block count; a
 * narrow block's 12 bytes per lane hold the 8 low bytes of its weights raw and their high bytes (sign, exponent >> 1) as
 * 4-bit codes over a per-block base, so a block is narrow when its exponents fit an EVEN-ALIGNED 16-value window (a few
 * per cent fewer blocks than the code form) and the kernel widens it with 12 instructions instead of ~30
 * (csrc/gemv_device.h; measurements: profiles/w12_split.md). The *_form functions are sd_w12_measure / sd_w12_pack with the
 * form named; the counts of one form do not describe a copy of the other. sd_w12_bytes and sd_w12_matrix serve both.
 * sd_model_set_w12_form puts the matrices of `classes` on a copy of `form` and leaves every other matrix on what it
 * streams: a model may hold a code-form copy for some classes and a split-byte copy for others (sd_model_set_w12 first
 * drops every copy, then sets the code form). SD_W12S_DEFAULT_CLASSES is what the measurements kept. */
#define SD_W12_FORM_CODES 1
#define SD_W12_FORM_SPLIT 2
#define SD_W12S_DEFAULT_CLASSES 0x14u   /* gate / up and the lm_head: the classes whose 5-token launch on 3B shapes is faster on W12S than on what they streamed before */
int sd_w12_measure_form(const sd_model_config* cfg, int form, void* scratch, size_t scratch_bytes, uint32_t* n_wide, void* stream);
int sd_w12_pack_form(const sd_model_config* cfg, int form, const void* scratch, const uint32_t* n_wide, void* dst, size_t dst_bytes, void* stream);
int sd_model_set_w12_form(sd_model* m, const void* w12, const uint32_t* n_wide, unsigned classes, int form);

/* Tokens one pass of sd_model_forward covers: 128 or 64 when every matrix of the model has a shape the
 * multi-token kernel (gemm_skinny.hip) handles at that size, else 9 or fewer (x rows must fit the LDS). Larger B*M are tiled into passes. */
int sd_model_pass_tokens(const sd_model* m);

/* Scratch the forward needs (activations of one pass + argmax partials). */
size_t sd_model_workspace_bytes(const sd_model* m);
/* Bytes of ONE of the two cache tensors, bf16:
 *   K: [n_layers][B][Hkv][Lmax][D]      V: [n_layers][B][Hkv][D][Lmax] (transposed)
 * Lmax must be a multiple of 8. */
size_t sd_model_kv_bytes(const sd_model* m, int B, int Lmax);
/* Attach caller-owned KV caches and workspace. */
int sd_model_bind(sd_model* m, void* k_cache, void* v_cache, int B, int Lmax,
                  void* workspace, size_t workspace_bytes);

/* Paged KV (the counterpart of the reference's per-sequence cache tensors that grow by torch.cat
 * and are realigned to a common length, src/specdec/cache/kv_cache_manager.py:194-199 and :353-479): instead of Lmax
 * positions per row, rows own PAGES of page_len positions (a power of two >= 32) out of pools shared by all rows:
 *   K pool: [n_layers][n_pages][Hkv][page_len][D]    V pool: [n_layers][n_pages][Hkv][D][page_len]   (bf16)
 * and position pos of row b lives in page block_table[b * max_pages_per_row + pos / page_len] (the same page index in
 * every layer) at offset pos % page_len. `block_table` is device memory, caller-owned and caller-maintained: an entry
 * must be valid before a forward reads or writes a position in it (write entries on the stream the forward runs on, or
 * synchronise); entries of positions a row has not reached are never read. The row's capacity is
 * max_pages_per_row * page_len. Everything else (forward, step loop, C-ABI) is unchanged; sd_model_probe_gemv's QKV
 * probe is not available on a paged model. */
size_t sd_model_kv_pool_bytes(const sd_model* m, int n_pages, int page_len);   /* ONE of the two pools */
int sd_model_bind_paged(sd_model* m, void* k_pool, void* v_pool, int n_pages, int page_len,
                        const int32_t* block_table, int max_pages_per_row, int B,
                        void* workspace, size_t workspace_bytes);

/* KV shared between cache rows (csrc/kv_fork.hip): rows that hold the same prompt, or the same prefix, pay for it once.
 * Both entries are asynchronous on `stream`, copy all layers, all KV heads, K and V in one launch per 64 list entries,
 * take their lists from HOST memory (they travel in the kernels' argument blocks: no allocation, no copy, no
 * synchronisation) and touch nothing but the first n_pos positions of the destinations. n_pos == 0 or an empty list
 * succeeds and launches nothing. Refused before any device work (return code + sd_last_error): an unbound model, the dense
 * entry on a paged model and the reverse, an index out of range, a destination equal to its source or listed twice (paged:
 * also a destination that is a source of the same call), n_pos < 0 or beyond the row / page, a NULL list with a count > 0.
 *
 * Dense caches: the first n_pos positions of row src_row -> each of the n_dst rows dst_rows[]. */
int sd_model_kv_fork(sd_model* m, int src_row, const int32_t* dst_rows, int n_dst, int n_pos, void* stream);
/* Paged caches: the first n_pos <= page_len positions of page src_pages[i] -> page dst_pages[i] for n_pairs pairs
 * (n_pos == page_len: whole pages). Block tables and page ownership stay the caller's. */
int sd_model_kv_copy_pages(sd_model* m, const int32_t* src_pages, const int32_t* dst_pages, int n_pairs, int n_pos, void* stream);

/* KV eviction inside one cache row (csrc/kv_evict.hip): the rolling context window. In row `row` of a dense cache of a
 * Llama model, positions [keep + drop, n_pos) become positions [keep, n_pos - drop): all layers, all KV heads, K and V,
 * in place, in one launch, asynchronous on `stream`, no allocation, capturable. V moves bit for bit. K is stored after
 * RoPE, so it is rotated by -drop positions: rotate-half pairs (i, i + D/2), c = rope_cos[drop][i], s = rope_sin[drop][i]
 * of the model's own tables, a' = a c + b s, b' = b c - a s in fp32 from the stored bf16 values, rounded once to bf16.
 * Positions [0, keep), positions >= n_pos - drop of the row (the stale [n_pos - drop, n_pos) included) and every other row
 * keep their bits. n_pos == keep + drop succeeds and launches nothing. Refused before any device work (return code +
 * sd_last_error): an unbound model, a paged model, a GPT-2 model, row out of range, keep < 0, drop < 1 or not a multiple of 8
 * (source and destination of a V row stay in one 16-byte phase), drop >= max_pos, keep + drop > n_pos, n_pos > Lmax. */
int sd_model_kv_evict(sd_model* m, int row, int keep, int drop, int n_pos, void* stream);

/* One forward over M new tokens per batch row, appended to the KV cache in place.
 *   tokens   : device int32, token (b,m) at tokens[b*tok_stride + m]
 *   pos_base : device int32[B]; token (b,m) sits at position pos_base[b] + pos_off + m
 *              and attends to cache positions 0 .. that position (its own K/V are
 *              written first — the KV-append path of kv_append_ref, fused)
 *   ids_out  : optional device int32, argmax of token (b,m) at ids_out[b*ids_stride+m]
 *   logits_out: optional [B][M][vocab] (SD_BF16 | SD_F32)
 *   skip_head: 1 = only fill the cache (prefill of all but the last token)
 *   row0, B  : the call works on rows [row0, row0+B) of the bound batch; element 0 of
 *              tokens / pos_base / ids_out / logits_out belongs to row row0
 * B*M may exceed the 9 tokens one pass holds; the call then makes several passes. */
int sd_model_forward(sd_model* m, const int32_t* tokens, int tok_stride,
                     const int32_t* pos_base, int pos_off, int row0, int B, int M,
                     int32_t* ids_out, int ids_stride,
                     void* logits_out, int logits_dtype, int skip_head, void* stream);

/* The residual-stream rows (bf16 [n][d_model], BEFORE the final norm) that the last pass of the last sd_model_forward
 * left in the workspace: token (b, m) of that pass is row b*M + m. Rows [row0, row0+n) are copied to `out` (device
 * memory), asynchronously on `stream`. This is `outputs.hidden_states` of the reference's draft modes one norm earlier:
 * _run_medusa_hf / _run_eagle_hf read hidden_states[-1][:, -1] (src/specdec/core/pipeline.py:674-686, 788-800), i.e.
 * final_norm(row). */
int sd_model_hidden_rows(sd_model* m, int row0, int n, void* out, void* stream);

/* Log-likelihood of tokens[0..n) appended to cache row `row` at positions pos0..pos0+n-1 (after the row's first pos0
 * cached positions). logprob[i] = log p(tokens[i+1] | ...) for i < n-1 (fp32, may be NULL); greedy[i] = argmax id after
 * position i for i < n (may be NULL; greedy[n-1] is the next token a forward would return). Leaves the KV cache as
 * sd_model_forward(skip_head=1) over the same tokens does. tokens, logprob and greedy are device memory.
 * The layers take the route sd_model_forward takes for one row of n tokens (the prefill backend for n >= 96, chunks of <= 512
 * positions; else the passes) and count in sd_model_prefill_count the same way; the head is the native GEMM over the packed
 * lm_head (csrc/score_head.hip) with a log-softmax / argmax epilogue, so no [n][V] logits are written. Each logit is the value a
 * bf16 lm_head returns (fp32 product, x row scale for fp8, rounded once to bf16). Outputs are bit-identical run to run.
 * Refused (nonzero + sd_last_error, before any device work): NULL model or tokens, n < 2, a model without packed weights,
 * d_model not a multiple of 64, an unbound model, row / positions out of range, a capturing stream. */
int sd_model_score(sd_model* m, const int32_t* tokens, int n, int row, int pos0,
                   float* logprob, int32_t* greedy, void* stream);

/* sd_model_score with one difference: the head STORES each position's logits — logits_bf16[i][v], bf16 [n][vocab] contiguous, HF
 * row order, the bf16 value the score epilogue forms — instead of reducing them to a log-probability. Layer route, chunking, cache
 * effect, sd_model_prefill_count accounting and greedy (may be NULL) are sd_model_score's; n >= 1. The refusals are
 * sd_model_score's, plus NULL logits. Unlike sd_model_forward with logits_out it keeps the GEMM prefill route. */
int sd_model_score_logits(sd_model* m, const int32_t* tokens, int n, int row, int pos0,
                          void* logits_bf16, int32_t* greedy, void* stream);

/* Measurement hook for bench.py's roofline leg: launches ONE of the forward's weight-
 * streaming GEMVs (which: 1 = attention out-proj, 2 = norm+gate/up+SwiGLU, 3 = down-proj,
 * 4 = final norm+lm_head+argmax) `iters` times, round-robin over the layers so the weights
 * stream from HBM, between two HIP events on `stream`; returns the average launch duration
 * and the algorithmic bytes of one launch (N*K*2). Synchronises on the second event. */
int sd_model_probe_gemv(sd_model* m, int which, int T, int iters, void* stream,
                        float* avg_usec, double* bytes_per_launch);

/* ---- persistent forward (csrc/persist.hip) ---------------------------------
 * Passes of <= sd_model_persist_tokens(m) tokens of a dense-KV Llama model with packed bf16 weights run as ONE launch
 * (an LDS-DMA loader wave per CU streams the weights ahead of every dependency; activations cross CUs as tagged 8-byte
 * granules) instead of five launches per layer. It replaces the same reference code as sd_model_forward does (the k-step
 * draft loop, src/specdec/models/hf_wrappers.py:417-539). 0 = not available for this model / device (other
 * architectures, fp8 or row-major weights, paged KV, a GPU without 256 CUs, SPECDEC_NO_PERSIST=1); the environment
 * variable SPECDEC_PERSIST_MAX_T (read by sd_model_bind) sets the token limit (default: 2 for models with d_model <= 2048, where the
 * launch is measured faster than the launch path; 0 for wider models, where it is not; at most 8). Whether a given pass takes it
 * also depends on the rows' current length: sd_model_set_length_hint below. */
int sd_model_persist_tokens(const sd_model* m);

/* Health word of the persistent launches of `m` since it was bound: 0 = every launch ran to completion. Every wait
 * inside the launch is bounded (50 ms); a workgroup that gives up ORs a reason into this word (1 loader blocked, 2 weights
 * never landed, 4 / 8 intra-workgroup hand-over, 16 granules of another CU never arrived, 32 attention hand-over) and
 * leaves, and the pass's outputs are then invalid. Synchronises `stream` (one 4-byte copy to the host). The step loop
 * also carries the word of its models in every step record (sd_specdec_record). */
int sd_model_engine_status(sd_model* m, uint32_t* status_out, void* stream);

/* The same word as a pinned host location (NULL before the model is bound): a workgroup that gives up also stores its
 * reason there, so whoever has just synchronised with a pass to read its ids / logits can check the pass's health with a
 * plain load, no copy, no further synchronisation. 0 = every persistent launch since the bind / the last clear completed. */
const uint32_t* sd_model_status_word(const sd_model* m);

/* Recovery after a non-zero health word: synchronises `stream`, clears the device word and the host word and moves the launch
 * counter past the failed launch (so that granules it left behind never match again). The passes since the failure are
 * invalid and must be repeated — typically after sd_model_set_persist_tokens(m, 0), i.e. on the launch path.
 * PRECONDITION of the persistent launch, for direct C callers: it needs all 256 CUs to itself while it runs (one workgroup
 * per CU, each declaring the CU's whole LDS, spinning on the others' hand-offs). A second process on the same GPU, or a
 * second stream of this process running another LDS-heavy kernel at the same time, can split the CUs between the two;
 * the launch then gives up after its 50 ms bound (it never hangs) and reports here. Share a GPU only with
 * SPECDEC_NO_PERSIST=1 or sd_model_set_persist_tokens(m, 0). */
int sd_model_engine_status_clear(sd_model* m, void* stream);

/* Tokens per pass the persistent launch takes from now on: min(max_tokens, what the model / cache allows); 0 = launch path
 * only. Host-side state: steps already captured (sd_specdec_step) keep the kernels they were captured with — call
 * sd_specdec_invalidate on the loops that use the model. */
int sd_model_set_persist_tokens(sd_model* m, int max_tokens);

/* The caller's bound on the CURRENT length (cached positions) of the rows the coming passes touch; max_len <= 0 or beyond
 * the cache: the cache size (the default after a bind). The persistent launch walks a head's whole cache on one CU and is
 * the faster path up to 1280 positions only, so a session bound for a long context starts on it and moves to the launch
 * path when its rows pass that length (host-side state, as above: re-capture after crossing). */
int sd_model_set_length_hint(sd_model* m, int max_len);

/* 1 when a pass of T tokens of one row would run as the persistent launch right now, else 0. */
int sd_model_persist_active(const sd_model* m, int T);

/* Prompt prefill: how a pass of >= 96 positions per row (a prompt being absorbed into the KV cache) is computed.
 *   SD_PREFILL_AUTO     the default after every bind: rocBLAS GEMMs for a Llama model with bf16 row-major weights and dense
 *                       KV when the library can be opened (and SPECDEC_NO_GEMM_PREFILL is unset), else the 128-token passes
 *   SD_PREFILL_PASSES   always the decode-shaped 128-token passes
 *   SD_PREFILL_ROCBLAS  rocBLAS GEMMs over the HF-layout bf16 weights (Llama, bf16 storage, dense KV)
 *   SD_PREFILL_NATIVE   this library's MFMA GEMM over the packed weights (Llama, bf16 or fp8 storage, dense or paged KV)
 * Under every backend a pass that asks for logits, runs under stream capture or is gated by adaptive K takes the passes. */
enum sd_prefill_backend { SD_PREFILL_AUTO = 0, SD_PREFILL_PASSES = 1, SD_PREFILL_ROCBLAS = 2, SD_PREFILL_NATIVE = 3 };

/* 1 when `backend` can be used in this process (ROCBLAS: the library opens), else 0. */
int sd_prefill_backend_available(int backend);

/* Select the prefill backend of `m` until the next bind. Nonzero (with sd_last_error) for an unknown value; ROCBLAS when the
 * library is missing or the model is fp8, paged or GPT-2; NATIVE for GPT-2, for a model without packed weights
 * (SPECDEC_NO_PACK) or with d_model, Hq*D or d_ff not a multiple of 64. A choice is never replaced by another GEMM backend. */
int sd_model_set_prefill_backend(sd_model* m, int backend);

/* The configured backend (enum sd_prefill_backend). */
int sd_model_prefill_backend(const sd_model* m);

/* Prompt rows absorbed by SD_PREFILL_PASSES, _ROCBLAS or _NATIVE since the bind: one per row of a forward call with >= 96
 * positions per row. -1 for another value. */
int64_t sd_model_prefill_count(const sd_model* m, int backend);

/* Rows [row0, row0+n) of one of the workspace buffers the last pass left behind (bf16, asynchronous copy on `stream`):
 * which = 0 residual stream [d_model] (= sd_model_hidden_rows), 1 q after RoPE [Hq*D], 2 attention rows [Hq*D],
 * 3 MLP activation [d_ff]; all of the LAST layer. After a prompt absorbed by a GEMM prefill backend (rocBLAS or native) the
 * rows are those of the last chunk's last <= 128 positions, in position order: the same positions sd_model_hidden_rows returns.
 * For stage-by-stage checks of every forward path against each other and against a plain reference. (The draft model of an sd_specdec loop runs the persistent launch WITHOUT these stores unless
 * SPECDEC_PERSIST_TAPS is set when the loop is created: its rows are then not updated by the loop's passes.) */
int sd_model_debug_rows(sd_model* m, int which, int row0, int n, void* out, void* stream);

/* Rows [row0, row0+n) of the LAST chunk of the last GEMM-prefilled prompt (rocBLAS or native backend), in position order: row r is
 * the chunk's position r, for every one of its Mc <= 512 positions — not only the last <= 128 that sd_model_debug_rows and
 * sd_model_hidden_rows see. `which` as for sd_model_debug_rows (0 residual stream, 1 q, 2 attention, 3 activation; last layer);
 * bf16, asynchronous copy on `stream` out of the prefill workspace, which the chunk left as it is: a pure copy, and rows
 * [Mc - min(Mc, 128), Mc) are bit for bit the rows those two entries return. The record is dropped by a bind and by every forward
 * of this model that is not such a chunk (a replay of a captured graph runs no host code and leaves it). Refused (nonzero) when no
 * chunk is on record, the range leaves [0, Mc), or `which` is unknown. Additive (SD_ABI_VERSION stays 1). */
int sd_model_prefill_rows(sd_model* m, int which, int row0, int n, void* out, void* stream);

/* Diagnostics of the multi-token weight-streaming kernels (csrc/gemm_skinny.hip, csrc/gemm_pipe.hip); host-only, no device
 * call, additive (SD_ABI_VERSION stays 1).
 *
 * sd_gemm_plan writes the name of the template instantiation that one matrix launch of T tokens runs for a matrix of
 * n_pairs row pairs and K inputs: the launchers take the same decision from the same function. w8: 1 = fp8 e4m3 weights;
 * prologue: 0 none, 1 RMSNorm, 2 LayerNorm; epi: 0 QKV + RoPE, 1 residual, 2 SwiGLU, 3 gelu_new, 4 argmax. Names:
 *   "pipe<EPI,tgN,DT,scS>"     the chunk pipeline: N token groups of 16, S steps per wave per chunk
 *   "chunked<EPI,tgN,DT,nbS>"  the chunked fallback: S weight steps per batch
 *   "slice<tgN>", "direct<tgN>" the two plain-residual bodies (bf16, no norm)
 *   "gemv"                      T <= 9: csrc/gemv.hip (its variants are not named). "gemv" names the launcher that is asked;
 *                               sd_gemv_instance names the kernel that runs, which for rows too long to stage is a body above.
 *   "none"                      no kernel covers the shape (a launch would be refused)
 * with EPI in qkv, resid, swiglu, gelu, argmax and DT in bf16, fp8. flags: bit 0 = plan as if SPECDEC_NO_DIRECT were set,
 * bit 1 = as if SPECDEC_NO_PIPE were; 0 follows the process's own environment, as a launch does. Refused: NULL out, a cap
 * that does not hold the name and its NUL (32 bytes always do), T < 1, an unknown prologue / epi / flag bit.
 *
 * sd_model_matrix_shape: rows, inputs, row pairs, epilogue and prologue of one of the model's five matrix kinds
 * (which: 0 qkv, 1 out, 2 gate / up, 3 down, 4 lm_head), as every launch of the forward passes them. */
int sd_gemm_plan(int T, int n_pairs, int K, int w8, int prologue, int epi, int flags, char* out, size_t cap);
int sd_model_matrix_shape(const sd_model* m, int which, int* N, int* K, int* n_pairs, int* epi, int* prologue);

/* sd_gemv_variant names the csrc/gemv.hip instance that a launch of T <= 9 tokens runs for a packed matrix without bias,
 * gathered rows or batch (the layer matrices of a forward; arguments as sd_gemm_plan): "generic", or
 * "fixed<EPI,ksS,tpP,PRO,ttT,kbB>" for a fixed-geometry instance with S K-slices per tile, P pairs per tile, prologue PRO
 * (none, rmsnorm), token bound T and B loads per batch. The launcher asks the same function; SPECDEC_GEMV_GENERIC=1 in the
 * environment makes both answer "generic". Host-only, additive (SD_ABI_VERSION stays 1). Refused: NULL out, a cap that does
 * not hold the name (64 bytes always do), T outside 1..9, an unknown prologue / epi, n_pairs < 1, K no positive multiple of 8.
 * "generic" names the launcher's fallback as asked; sd_gemv_instance names the kernel that runs.
 *
 * sd_gemv_instance names the kernel that launch really runs, from the one host-side choice launch_gemv consumes:
 *   "fixed<...>"                               exactly sd_gemv_variant's answer
 *   "generic<EPI,whole|mask,ttN,DT,kbB>"       the template key of the generic kernel: epilogue, whole 32-k slices or the
 *                                              masked variant (always tt9), token bound N in 1, 2, 3, 5, 9, bf16 or fp8
 *                                              storage, B loads per batch
 *   "skinny:" + a name of sd_gemm_plan         T rows of K do not fit the LDS and csrc/gemm_skinny.hip takes the launch
 *                                              (K = 14336 at 6..9 tokens): the body that runs, at T < 10
 * w8 = 2 in either function asks for a bf16 matrix that has a W12 copy (sd_model_set_w12): where the W12 kernels cover the
 * shape the names end in ",w12>" for a fixed instance (W12 twins exist at token bound 5; a fixed class at another token
 * count runs the generic W12 kernel) and carry DT = w12 for the generic kernel; SPECDEC_NO_W12 turns both back to bf16. w8 = 3 asks the same for a copy in the
 * split-byte form (sd_model_set_w12_form): ",w12s>" and DT = w12s.
 * Follows SPECDEC_GEMV_GENERIC at every call. Refused as sd_gemv_variant refuses, and where launch_gemv would refuse the
 * launch (fp8 storage whose K slices are not whole 64-k steps; rows that fit neither kernel). Host-only, additive
 * (SD_ABI_VERSION stays 1). */
int sd_gemv_variant(int T, int n_pairs, int K, int w8, int prologue, int epi, char* out, size_t cap);
int sd_gemv_instance(int T, int n_pairs, int K, int w8, int prologue, int epi, char* out, size_t cap);

/* Diagnostics of the K-token attention launch (csrc/attention.hip); host-only, additive (SD_ABI_VERSION stays 1).
 *
 * sd_attention_plan answers, from dimensions alone (no device call), the geometry launch_attention decides from the same
 * function for B rows x M tokens over a cache of l_max positions per row: *tiles = 16-row query tiles per (row, kv head),
 * ceil(Hq / Hkv * M / 16); *n_split = workgroups per tile (split-KV): l_max / 512, at most 32, at most the workspace's
 * 1024 partial tiles / (Hkv * B * tiles) and at most 512 / (Hkv * B * tiles), at least 1 (a row uses
 * min(n_split, ceil(key blocks / 16)) of them); the grid is (*grid_x, *grid_y, *grid_z) = (Hkv, B, tiles * n_split).
 * paged: 0 = dense cache rows, else the positions per page. The engine's launches always have the split workspace, so
 * the query assumes it; SPECDEC_NO_ATTN_SPLIT in the environment gives n_split 1, as at a launch. Refused (nonzero): a
 * NULL output, heads or M above 255, and what the launch refuses, in its words (head_dim not 32 / 64 / 128, Hq % Hkv,
 * B or M below 1, l_max not a multiple of 8, pages not 32 * 2^n positions or l_max not whole pages). */
int sd_attention_plan(int n_q_heads, int n_kv_heads, int head_dim, int B, int M, int l_max, int paged, int* tiles, int* n_split,
                      int* grid_x, int* grid_y, int* grid_z);

/* Diagnostics of the persistent forward (csrc/persist.hip); host-only, additive (SD_ABI_VERSION stays 1).
 *
 * sd_persist_plan answers, from a model's dimensions and facts alone (no weights, no device call; a GPU of 256 CUs is
 * assumed), what sd_model_bind and the launch decide from the same functions: *eligible = 1 when the model passes every
 * static rule (Llama, packed bf16 weights, head_dim 64 or 128, d_model / Hq*D / d_ff in whole 128s, d_model <= 4096,
 * 1..60 layers, no bias, every matrix cut for <= 256 workgroups, <= 4 QKV tiles and an even gate / up split per workgroup,
 * one token's rows fitting the LDS); *max_tokens = tokens a pass can hold (0 when not eligible; what
 * sd_model_set_persist_tokens can raise a bound model to, given a cache of whole 8-key vectors). For 1 <= T <= *max_tokens,
 * `name` is the kernel instantiation a pass of T tokens runs, "persist<D,HC>" with D the head dimension and HC the
 * 1024-granule chunks of a d_model-wide row (2 above d_model 2048), and *ring_bytes the weight ring the LDS carve of one
 * row of T tokens leaves. Otherwise name is "none", *ring_bytes 0 and `reason` names the rule that refused (the first in
 * the order above, or T above the limit); reason is "" for an eligible T. packed: 1 = the tile streams of sd_pack_weights;
 * weight_dtype: SD_BF16 or SD_FP8_E4M3; has_bias: 1 when any layer matrix has a bias. SPECDEC_NO_PERSIST is honoured as at
 * a bind. Refused (nonzero): a NULL output, T < 1, a dimension below 1, a cap that does not hold the text and its NUL
 * (32 bytes for the name and 96 for the reason always do). */
int sd_persist_plan(int arch, int n_layers, int d_model, int n_heads, int n_kv_heads, int head_dim, int d_ff, int vocab,
                    int packed, int weight_dtype, int has_bias, int T, int* eligible, int* max_tokens, int* ring_bytes,
                    char* name, size_t name_cap, char* reason, size_t reason_cap);

/* Diagnostics of the native prompt-prefill GEMM (csrc/prefill_mfma.hip); host-only, additive (SD_ABI_VERSION stays 1).
 *
 * sd_prefill_plan answers, from a model's dimensions alone (no weights, no device call), what the launcher decides from the same
 * functions for layer product `which` (0 qkv, 1 out, 2 gate / up, 3 down) over one chunk of T positions (1 .. 512), w8 = 1 for
 * fp8 e4m3 storage: `name` = the kernel instantiation, "mfma<rf4,DT>" (128-row blocks) or "mfma<rf2,DT>" (64-row blocks), DT in
 * bf16, fp8; *row_blocks and *token_blocks (128 tokens each), *grid = their product, *swizzled = 1 when the grid is a multiple of 8
 * and workgroups are dealt to blocks XCD by XCD; *last_rows = rows of the last token block; *min_block_rows = the fewest packed
 * rows any row block holds (blocks are whole tiles of the packed stream, so a block may hold fewer rows than its height and
 * leaves lanes without a row); *k_stages = 64-k stages of the main loop. packed: 1 = the model has the packed weight streams.
 * For a model the native backend refuses (not Llama; no packed weights; d_model, Hq*D or d_ff not in whole 64s) *eligible = 0,
 * name is "none", the numbers are 0 and `reason` is the text sd_model_set_prefill_backend(SD_PREFILL_NATIVE) refuses it with (one
 * function serves both); reason is "" otherwise. Refused (nonzero): a NULL output, `which` or T out of range, a dimension below 1, a cap that does not hold the
 * text and its NUL (32 bytes for the name and 96 for the reason always do).
 *
 * sd_prefill_plan_tables: the same plan's tables. blocks[2 b] = first row pair of row block b and blocks[2 b + 1] = its packed rows
 * (n_blocks = *row_blocks entries of two ints); wg_block[g] = the linear block index rb * token_blocks + tb that workgroup g of
 * the grid computes (n_grid = *grid ints). Refused when the model is not eligible or a count is not the plan's. */
int sd_prefill_plan(int arch, int d_model, int n_heads, int n_kv_heads, int head_dim, int d_ff, int which, int T, int w8,
                    int packed, int* eligible, int* row_blocks, int* token_blocks, int* grid, int* swizzled, int* last_rows,
                    int* min_block_rows, int* k_stages, char* name, size_t name_cap, char* reason, size_t reason_cap);
int sd_prefill_plan_tables(int arch, int d_model, int n_heads, int n_kv_heads, int head_dim, int d_ff, int which, int T,
                           int* blocks, size_t n_blocks, int* wg_block, size_t n_grid);

/* Whether the persistent passes of `m` also store the stage rows (1, the default of a model outside a loop) or run the
 * instantiation without those stores (0: what sd_specdec_create selects for its draft). A pass with skip_head keeps its
 * stores either way. While it is off, sd_model_debug_rows and sd_model_hidden_rows are stale after a persistent pass. */
int sd_model_set_persist_taps(sd_model* m, int enable);

/* Measurement hook: `iters` whole forwards of one row of M tokens (token id 0, positions pos0..pos0+M-1 of cache row 0,
 * which they overwrite; the attention reads the pos0 positions below, whatever the cache holds) between two HIP events on `stream`; returns the average duration of a forward and the bytes of weights
 * it streams. skip_head = 1 leaves the lm_head out. timeline (optional, host memory, `timeline_cap` uint64): in-kernel
 * 100 MHz stamps of ONE further persistent forward, [256 workgroups][12 * n_ops + 4] (per op: gather start, input staged,
 * MFMA + epilogue done, attention done, third consumer's start and MFMA end, leader's MFMA end, loader done issuing the
 * op; then s_memrealtime / s_memtime at the workgroup's start and end: the shader clock it ran at); allocates and frees a device buffer and synchronises. */
int sd_model_probe_forward(sd_model* m, int M, int pos0, int iters, int skip_head, void* stream, float* avg_usec,
                           double* bytes_per_forward, unsigned long long* timeline, size_t timeline_cap);

/* ---- the step loop ------------------------------------------------------- */
typedef struct sd_specdec sd_specdec;

enum sd_emit_mode {
  SD_EMIT_BONUS = 0,   /* generate_batch: base tokens t_0..t_{a-1} + bonus t_a (pipeline.py:3059-3292) */
  SD_EMIT_DRAFT = 1    /* generate: draft tokens d_1..d_a, or t_0 if a == 0 (pipeline.py:1190-1235) */
};

/* Creation allocates the (tiny) device loop state and a pinned host mirror. Both
 * models must be bound with the same B.
 * draft == NULL selects the self-draft mode: Medusa-lite with heads tied to the lm_head, greedy — the
 * reference draftor (src/specdec/modes/medusa.py:71-186) evaluates head 0 on the same last hidden state for
 * all K proposals, i.e. proposes K copies of the target's own next token; the step is then one 1-token target
 * forward + the K+1-token verify forward. */
int sd_specdec_create(sd_model* draft, sd_model* target, int B, int K, int emit_mode,
                      sd_specdec** out);
int sd_specdec_destroy(sd_specdec* s);

/* (Re)initialise row b: `seq_len` tokens are final, the last two of them are
 * (prev_tok, last_tok); caches must hold positions [0, seq_len-1) of the target and
 * [0, seq_len-2] or more of the draft. Asynchronous on `stream`. */
int sd_specdec_set_row(sd_specdec* s, int b, int seq_len, int prev_tok, int last_tok,
                       int active, void* stream);

/* Sampled bonus token inside the step (generate_batch with do_sample=True: the reference
 * samples ONLY the token after the accepted prefix, pipeline.py:3140-3160 and :3351-3361;
 * drafting and verification stay greedy, :2400/:2645). With enable=1 the verify forward stores
 * its logits ([B][K+1][V] bf16 in logits_buf, caller-owned), and between the accept scan and the
 * state advance one sampler launch draws row b's token from the logits of position
 * accept_len[b] (sd_sample_token semantics; draw index = draw_counters[b], incremented per
 * sampled step; Philox stream = stream_ids[b] or b). enable=0 returns to the greedy step.
 * Either call drops the captured graph (it is re-captured on the next step). */
int sd_specdec_set_sampling(sd_specdec* s, int enable, float temperature, int top_k, float top_p,
                            uint64_t seed, void* logits_buf, size_t logits_bytes,
                            uint32_t* draw_counters, const int32_t* stream_ids);

/* Speculative sampling inside the step (opt-in; generate_batch with policy="rejection", backend="device"): the third mode
 * of the step next to greedy and sampled-bonus. Per row b and step, T = temperature > 0, every distribution is
 * softmax(x / T) over the STORED bf16 logits in float64, c = draw_counters[b] at the start of the step, sid = stream_ids[b]
 * or b, Philox4x32-10 keyed by seed:
 *   1. draft forward i (i = 0..K-1) stores its last position's logits as row q_i of draft_logits_buf ([B][K][V] bf16);
 *      d_{i+1} = Gumbel-max draw over q_i / T, counter (c + i, sid, element, Gumbel tag) — sd_sample_token's whole-row draw;
 *   2. the verify forward stores p_0..p_K in target_logits_buf ([B][K+1][V] bf16; until then its first rows are scratch
 *      for the draft forwards' logits);
 *   3. u_i = the uniform of counter (c + i, sid, 0, CDF tag); ratio_i = exp((p_i[d]/T - lse(p_i/T)) - (q_i[d]/T - lse(q_i/T)))
 *      with d = d_{i+1}; accept length a = number of leading i with u_i < ratio_i;
 *   4. next token: a < K: Gumbel-max over log max(0, softmax(p_a/T) - softmax(q_a/T)) on its support (empty support, q == p:
 *      over p_a / T); a == K: Gumbel-max over p_K / T; counter (c + K, sid, element, Gumbel tag);
 *   5. emitted: d_1..d_a + the next token (the accepted tokens are the DRAFT's ids; the record's target-argmax slots keep the
 *      target's argmax); draw_counters[b] += K + 1; rows with active == 0 consume no draws.
 * The emitted sequence is distributed as sampling from softmax(target bf16 logits / T), whatever the draft is. Non-finite
 * logits: a position whose p or q row holds a NaN or has a non-finite maximum is rejected and redrawn from p_i / T alone
 * (NaN-first ordering of sd_sample_token). Refused: SD_EMIT_DRAFT, loops without a draft model (self-draft, Medusa heads,
 * EAGLE), adaptive K, the sampled-bonus mode being on, temperature <= 0 or NaN, short or misaligned (16 B) buffers. Top-k /
 * top-p shaping of p and q is sd_specdec_set_spec_shaping below; without it the mode samples the whole vocabulary. Both calls
 * (enable / disable) drop the captured graph. */
int sd_specdec_set_spec_sampling(sd_specdec* s, int enable, float temperature, uint64_t seed, void* draft_logits_buf,
                                 size_t draft_logits_bytes, void* target_logits_buf, size_t target_logits_bytes,
                                 uint32_t* draw_counters, const int32_t* stream_ids);

/* Top-k / top-p shape of speculative sampling: with top_k in 1..1024 (clamped to V) both distributions of every position are
 * the temperature -> top-k -> top-p distribution of their row exactly as sd_sample_token defines it, and the emitted tokens
 * are distributed as the target's own sd_sample_token(temperature, top_k, top_p) sampling, whatever the draft is.
 * For a bf16 row x, S(x) = the kept ids in sorted order (value descending, index ascending), float64 weights
 * e_j = exp(x_j/T - max), Z = their sum added sequentially in sorted order; a row whose top value is not finite is the point
 * mass on its first id (no position is "rejected as non-finite" in this mode). x'(v) = e(v)/Z on the kept set, 0 elsewhere.
 * Per row b and step (c, sid, seed as above; Philox counter words are (draw, stream, element, tag)):
 *   1. d_{i+1}, i = 0..K-1: the uniform of counter (c + i, sid, 0, CDF tag) inverted through S(q_i) in sorted order — exactly
 *      the token sd_sample_token draws from q_i with draw index c + i; the logits row is stored as q_i as in the unshaped mode;
 *   2. u_i: counter (c + i, sid, 0, 0x5EED0003) — a tag of its own, the CDF-tag block of (c + i) being the draw of step 1;
 *   3. ratio_i = (e_p(d)/Z_p) / (e_q(d)/Z_q), d = d_{i+1}; e_p(d) = 0 when d is outside the target's kept set (rejected).
 *      p and q go through the same code in the same order: bitwise equal rows give exactly 1.0. a = leading i with u_i < ratio_i;
 *   4. next token, uniform u_n of counter (c + K, sid, 0, CDF tag): a < K: weights r_j = max(0, p'_a(id_j) - q'_a(id_j)) over
 *      the TARGET's kept ids in the target's sorted order, Z_r summed sequentially, the first j with u_n Z_r < cum_j (the last
 *      kept id otherwise); Z_r == 0 (q' >= p' on p's support): the same inversion through e_p, i.e. sd_sample_token on p_a with
 *      draw c + K; a == K: sd_sample_token on p_K with draw c + K;
 *   5. as step 5 above.
 * top_k <= 0 with top_p >= 1 returns to the unshaped mode (the default). Legal before or after
 * sd_specdec_set_spec_sampling(enable = 1); the shape is kept while the mode is switched off and on. Drops the captured graph.
 * Refused: top_k > 1024; top_k <= 0 with top_p < 1 (top_p without top_k, the full-vocabulary nucleus: it needs the rank-block
 * walk of sd_sample_token on two rows at once); top_p <= 0 or NaN. */
int sd_specdec_set_spec_shaping(sd_specdec* s, int top_k, float top_p);

/* Logit processors (csrc/logit_proc.hip): repetition / presence / frequency penalties and an additive bias, applied IN PLACE to
 * stored bf16 logits rows before they are consumed. State, caller-owned device memory:
 *   counts : uint16 [B][V] (sd_logit_counts_bytes: the table rounded up to 16 bytes). Bit 15 = the token occurs in the row's
 *            prompt; bits 0..14 = how often the row has generated it, saturating at 32767. The repetition penalty looks at
 *            prompt + generated (as HF and vLLM do), presence and frequency at generated only (as OpenAI and vLLM do).
 *   bias   : optional float32 [B][V], added to the logit; -inf bans a token, an allowed set is its complement filled with -inf.
 * The transform of one row of batch row b that is conditioned on the in-step tokens t_1..t_i, element v — every line one
 * correctly rounded fp32 operation, no fused multiply-add, so a float32 restatement reproduces the bits (tests/logit_proc_ref.py):
 *   x    = float(row[v])
 *   c    = (counts[b][v] & 0x7fff) + #{j <= i : t_j == v}                      (integer)
 *   seen = (counts[b][v] & 0x8000) != 0  or  c > 0
 *   if seen and rp != 1:  x = (x < 0) ? x * rp : x / rp        (HF RepetitionPenaltyLogitsProcessor; x == 0 takes the division)
 *   if c > 0:             x = x - presence
 *                         x = x - (frequency * float(c))       (product rounded, then the subtraction)
 *   if bias:              x = x + bias[b][v]
 *   row[v] = bf16(x)      (round to nearest even, the conversion of the other epilogues; a NaN is stored as 0x7fc0)
 *
 * sd_logit_process: rows bf16, row (b, r) at rows + (b * R + r) * row_stride elements (row_stride >= V); tokens: device int32,
 * row b's in-step tokens at tokens + b * tok_stride (nullable when no row has any); n_tokens < 0: row (b, r) is conditioned on
 * the first r of them (the verify pass: i = r), else every row on the first n_tokens (<= 64). Rows with active[b] == 0
 * (nullable) are not written. ids_out (nullable): ids_out[b * ids_stride + r] = argmax of the processed row — of the untouched
 * row for an inactive b — in the order of the fused lm_head argmax (argmax_better, csrc/common.h): a NaN is the maximum, then
 * the larger value, ties and several NaNs go to the lowest index. With rp = 1, presence = frequency = 0 and no bias the rows keep
 * their bits (but a NaN's payload) and the ids are those of the fused path. workspace (needed with ids_out only):
 * sd_logit_process_workspace(B, R, V) bytes, 4-byte aligned. A row is split over ceil(V / 4096) <= 64 workgroups, 16-byte
 * accesses where logits, counts and bias of the row are 16-byte aligned, element-wise otherwise. Asynchronous on `stream`, no
 * allocation, graph-capturable. Refused: NULL rows / counts, B, R, V < 1 or B * R > 65535, a stride below V, more than 64
 * in-step tokens or a token stride below their number, rp <= 0 or NaN, non-finite presence / frequency, a short workspace.
 *
 * sd_logit_counts_set: row b <- cleared, bit 15 for every id of prompt_ids[0..n_prompt), one count for every occurrence in
 * generated_ids[0..n_generated) (device lists; ids outside [0, V) are ignored). sd_logit_counts_add: for every row with
 * active[b] != 0 (nullable) the first min(n_new[b], max_new) tokens of tokens + b * tok_stride are counted, a token listed twice
 * counts twice, ids outside [0, V) (the -1 padding of a step's emitted tokens) are ignored; one lane per row, no atomics. */
size_t sd_logit_process_workspace(int B, int R, int V);
int sd_logit_process(void* rows, int64_t row_stride, int B, int R, int V, const void* counts, const float* bias,
                     const int32_t* tokens, int tok_stride, int n_tokens, const int32_t* active, float repetition_penalty,
                     float presence_penalty, float frequency_penalty, int32_t* ids_out, int ids_stride, void* workspace,
                     size_t workspace_bytes, void* stream);
size_t sd_logit_counts_bytes(int B, int V);
int sd_logit_counts_set(void* counts, int B, int V, int b, const int32_t* prompt_ids, int n_prompt, const int32_t* generated_ids,
                        int n_generated, void* stream);
int sd_logit_counts_add(void* counts, int B, int V, const int32_t* tokens, int tok_stride, const int32_t* n_new, int max_new,
                        const int32_t* active, void* stream);

/* Logit processors inside the step: a further mode next to greedy, sampled-bonus and speculative sampling, combinable with each.
 * With enable = 1 every logits row the step consumes is stored, processed (sd_logit_process, the same launcher), then consumed:
 *   - draft forward i stores its last position's row (as the speculative-sampling mode does, including the device-selected two
 *     forms of forward 0 and the persistent launch); the row is processed with in-step tokens d_1..d_i. Greedy and sampled-bonus:
 *     the fused argmax of the processed row is d_{i+1}. Speculative sampling: the processed row is copied to q_i and drawn from by
 *     the unchanged draw kernels.
 *   - the verify forward stores p_0..p_K; ONE process launch covers all B * (K+1) rows, row (b, i) with in-step tokens d_1..d_i;
 *     the argmax of the processed rows goes to the target-argmax slots. Greedy: the accept scan and the record follow as three
 *     launches (the one-launch tail reads raw partials and is not taken). Sampled bonus: accept length and sampler on the
 *     processed rows. Speculative sampling: the statistics and accept kernels on the processed p and q.
 *   - after the accept kernel the counts of every active row advance by its emitted tokens (sd_logit_counts_add).
 * So greedy output is the target's own greedy decoding under the processors, token for token, and speculative-sampling output
 * is distributed as the target's own sampling from its processed rows: acceptance tests p'/q' of two processed distributions,
 * and the usual proof applies unchanged. counts / bias (nullable) as above, [B][V], 16-byte aligned; counts are the caller's to
 * initialise (sd_logit_counts_set) before the first step of a sequence. logits_buf: [B][K+1][V] bf16, 16-byte aligned, where the
 * forwards store their rows while neither sampling mode is on (those modes' own buffers are used while one is: logits_buf may
 * then be NULL; a step that finds no buffer is refused). workspace: sd_logit_process_workspace(B, K + 1, V) bytes.
 * enable = 0 returns to the unprocessed step (launch for launch what it was). Either call drops the captured graph.
 * Refused: repetition_penalty <= 0 or NaN; non-finite presence / frequency; NULL, short or misaligned buffers; loops without a
 * draft model (self-draft, Medusa heads, EAGLE: their proposals come from no logits row); per-row adaptive K. Both emit modes
 * are legal. */
int sd_specdec_set_logit_processors(sd_specdec* s, int enable, float repetition_penalty, float presence_penalty,
                                    float frequency_penalty, void* counts, size_t counts_bytes, const float* bias, size_t bias_bytes,
                                    void* logits_buf, size_t logits_bytes, void* workspace, size_t workspace_bytes);

/* Grammar-constrained decoding (csrc/grammar.hip; the compiler from regular expressions and answer lists is
 * specdec_hip/grammar.py): a token automaton whose mask is one more line of the transform above. Tables, caller-owned device
 * memory, 16-byte aligned:
 *   next  : uint16 [S][V], 1 <= S <= 65534; next[s][v] = the state after token v in state s, 0xFFFF = v is not allowed in s.
 *   allow : uint32 [S][ceil(V / 32)] (sd_fsm_mask_bytes: rounded up to 16 bytes); bit v % 32 of word v / 32 = next[s][v] !=
 *           0xFFFF, pad bits 0. sd_fsm_build_masks builds it on the device from `next`: one source of truth.
 *   state : int32 [B]; -1 = the row is unconstrained, 0..S-1 = its state, anything else = DEAD (the kernels store DEAD as
 *           0xFFFF). step(s, t) = DEAD if s is DEAD, t is outside [0, V) or next[s][t] is 0xFFFF or >= S; else next[s][t].
 * The transform of a row of batch row b conditioned on the in-step tokens t_1..t_n gains, after the bias line and instead of
 * the plain rounding:
 *   if state[b] >= 0:  s = step(..step(state[b], t_1).., t_n)
 *                      allowed(v) = (s is DEAD) ? v == eos_id : bit v of allow[s]
 *                      if not allowed(v):  row[v] = 0xff80 (-inf), whatever x is: the mask overrides a NaN
 *   else, and for an allowed v:  row[v] = bf16(x) as above (a NaN is stored as 0x7fc0)
 * so a +inf bias at a disallowed id gives -inf, and a row at -1 is processed exactly as sd_logit_process processes it.
 *
 * sd_logit_process_fsm: the arguments of sd_logit_process, then the tables, S, the rows' states and eos_id. Same launch
 * geometry, same argmax, same refusals; the mask is folded into the kernel (on the 16-byte path a lane's 8 elements are one
 * byte of the mask row), no launch is added. Each workgroup walks its row's tokens from state[b] (n <= 64 dependent lookups;
 * the step below chains instead). Further refused: NULL or misaligned tables, NULL state, S outside 1..65534, eos_id outside
 * [0, V).
 *
 * sd_fsm_advance: for every row with active[b] != 0 (nullable) and state[b] >= 0, state[b] <- step over the first
 * min(n_new[b], max_new) tokens of tokens + b * tok_stride (a -1 padding inside that range leads to DEAD, as any id outside
 * the vocabulary does); one lane per row, no atomics. */
size_t sd_fsm_mask_bytes(int S, int V);
int sd_fsm_build_masks(const void* next, int S, int V, void* allow, size_t allow_bytes, void* stream);
int sd_fsm_advance(const void* next, int S, int V, int32_t* fsm_state, int B, const int32_t* tokens, int tok_stride,
                   const int32_t* n_new, int max_new, const int32_t* active, void* stream);
int sd_logit_process_fsm(void* rows, int64_t row_stride, int B, int R, int V, const void* counts, const float* bias,
                         const int32_t* tokens, int tok_stride, int n_tokens, const int32_t* active, float repetition_penalty,
                         float presence_penalty, float frequency_penalty, int32_t* ids_out, int ids_stride, void* workspace,
                         size_t workspace_bytes, const void* next, const void* allow, int S, const int32_t* fsm_state, int eos_id,
                         void* stream);

/* The grammar inside the step: with enable = 1 every process launch of the logit-processor stage also applies the mask, row
 * (b, i) in the state reached from fsm_state[b] over the step's own d_1..d_i, so the draft proposes and the target emits only
 * tokens the automaton allows. The launch after draft forward i finds the state after d_1..d_{i-1} in a position table of the
 * loop ([B][K+1], written by workgroup 0 of the launch before it) and does one lookup; each workgroup of verify row (b, i)
 * reads entry i - 1 and does the one lookup it is ahead of: no serial walk, no spin-wait, no atomics, no grid barrier. After
 * the accept kernel fsm_state advances over the emitted tokens of every active row (sd_fsm_advance), next to the counts. The
 * caller sets fsm_state[b] to the row's start state before its first step and repairs it like the counts when it voids steps
 * that ran ahead. All sampling modes work unchanged: a masked token has probability 0 in p and q alike. enable = 0 unbinds
 * (the step is launch for launch the stage without a grammar); switching the stage off unbinds too. Either call drops the
 * captured graph. Refused: the logit-processor stage off; S outside 1..65534; eos_id outside [0, V); NULL or misaligned
 * tables (16 bytes); per-row adaptive K; loops without a draft model (self-draft, Medusa heads, EAGLE). Additive
 * (SD_ABI_VERSION stays 1). */
int sd_specdec_set_grammar(sd_specdec* s, int enable, const void* next, const void* allow, int S, int32_t* fsm_state, int eos_id);

/* Per-request sampling parameters, row by row (csrc/sample.hip, csrc/spec_sample.hip, csrc/logit_proc.hip). A table is
 * sd_row_sampling[B] in device memory: caller-owned, 16-byte aligned, READ BY THE KERNELS AT RUN TIME, so the caller may
 * rewrite entry b on the stream between two launches (or two replays of a captured step) and the next launch follows it.
 * The host cannot check the contents at launch; every kernel normalises its row's entry with one device function
 * (normalise_row_sampling, csrc/sample_device.h) and is memory-safe for every bit pattern:
 *   a GREEDY ROW, exactly (temperature 1, top_k 1, top_p 1), when !(temperature > 0) (0 is the documented way to ask for
 *   greedy; a NaN falls here too), or min(top_k, V) > 1024, or top_p is NaN or <= 0, or — in the speculative-sampling kernels
 *   only — top_k <= 0 with top_p < 1 (the full-vocabulary nucleus stays unsupported there);
 *   otherwise top_k <= 0 = no top-k, top_p >= 1 = no nucleus cut, Philox key = (seed_lo, seed_hi);
 *   penalties the scalar entries refuse (repetition_penalty <= 0 or NaN, a presence or frequency penalty that is not finite)
 *   are the identity (1, 0, 0) for that row.
 * Row b's workgroups then branch, workgroup-uniformly, into the code the scalar kernel runs, so row b of a _rows launch gives
 * bit for bit what the scalar entry gives when called on that row alone with the normalised entry, the same draw counter and
 * the same stream id: ids, accept lengths, counters, float64 ratios, processed bf16 rows.
 *   sd_sample_token_rows        sd_sample_token with the table in place of temperature, top_k, top_p, seed: one launch, each row
 *                               on the top-k, the full-vocabulary nucleus or the Gumbel-max path
 *   sd_spec_sample_accept_rows  sd_spec_sample_accept_shaped likewise (same workspace): a row with top_k <= 0 and top_p >= 1
 *                               runs the unshaped statistics of sd_spec_sample_accept, any other row the shaped ones; counters
 *                               advance by K + 1 either way
 *   sd_logit_process_rows       sd_logit_process_fsm with the table in place of the three penalties; next == allow ==
 *                               fsm_state == NULL: no grammar
 * Refused by the host: a NULL or misaligned table, B < 1, and what the scalar entries refuse about their other arguments.
 * Additive (SD_ABI_VERSION stays 1). */
typedef struct sd_row_sampling {
  float temperature; int32_t top_k; float top_p;
  uint32_t seed_lo, seed_hi;
  float repetition_penalty, presence_penalty, frequency_penalty;
} sd_row_sampling;
size_t sd_row_sampling_bytes(void);
int sd_sample_token_rows(const void* logits, int logits_dtype, int64_t row_stride, int B, int V, const int32_t* pos, int rows_per_b,
                         const int32_t* active, const sd_row_sampling* table, uint32_t* draw_counters, uint32_t draw0,
                         const int32_t* stream_id, int32_t* out_ids, void* stream);
int sd_spec_sample_accept_rows(const void* draft_logits, const void* target_logits, const int32_t* draft_ids, int B, int K, int V,
                               const sd_row_sampling* table, uint32_t* draw_counters, uint32_t draw0, const int32_t* stream_ids,
                               const int32_t* active, int32_t* accept_len_out, int32_t* next_tok_out, double* ratios_out,
                               void* workspace, size_t workspace_bytes, void* stream);
int sd_logit_process_rows(void* rows, int64_t row_stride, int B, int R, int V, const void* counts, const float* bias,
                          const int32_t* tokens, int tok_stride, int n_tokens, const int32_t* active, const sd_row_sampling* table,
                          int32_t* ids_out, int ids_stride, void* workspace, size_t workspace_bytes, const void* next,
                          const void* allow, int S, const int32_t* fsm_state, int eos_id, void* stream);

/* The table inside the step: with a table ([B], device) the sampled-bonus draw, the speculative-sampling draws, statistics and
 * accept, and the logit-processor launches take their parameters from table[b]; the loop's scalars (temperature, top_k, top_p,
 * seed, spec shaping, penalties) are ignored for those launches. Which mode runs and which buffers it uses stay what
 * sd_specdec_set_sampling / sd_specdec_set_spec_sampling / sd_specdec_set_logit_processors configured. While a table is bound
 * the caller may rewrite table[b], stream_ids[b], draw_counters[b] and the bias row of a slot on the loop's stream between
 * steps and THE CAPTURED GRAPH IS KEPT: admitting a request captures nothing again. NULL returns to the scalars; a step
 * without a table is launch for launch what it was. Either call drops the captured graph. Refused: a misaligned table; a
 * table while neither a sampling mode nor the logit-processor stage is on. Additive (SD_ABI_VERSION stays 1). */
int sd_specdec_set_row_sampling(sd_specdec* s, const sd_row_sampling* table);

/* Lossy acceptance inside the step (sd_typical_accept's rules on the verify forward's own rows). With rule SD_ACCEPT_TYPICAL or
 * SD_ACCEPT_TOPK_AGREE the verify forward stores its [B][K+1][V] logits, the logit-processor stage (if on) processes them in
 * place — so bans and grammars count — and sd_typical_accept's two launches replace the exact-match accept scan: the step emits
 * the draft's ids d_1..d_a, then one token of the target's: its (processed) argmax at position a, or, with the sampled-bonus
 * mode on, the draw sd_specdec_set_sampling configured from row a. The draft loop is unchanged (greedy draft tokens). In the step,
 * rank_d breaks ties among equal STORED values in favour of the forward's own argmax (computed before the row was rounded to bf16),
 * then of the lower index: SD_ACCEPT_TOPK_AGREE with agree_k = 1 is exactly the step's exact-match rule.
 * logits_buf: caller-owned [B][K+1][V] bf16, 16-byte aligned, used while the sampled-bonus mode is off (that mode's own buffer
 * is used while it is on; logits_buf may then be NULL). rule SD_ACCEPT_OFF (the default): the step is launch for launch what it
 * is without this call. Switching the rule on or off drops the captured graph. Refused: what sd_typical_accept refuses about
 * the parameters; a short or misaligned buffer; the draft-emit mode; speculative sampling; per-row adaptive K; EAGLE, Medusa
 * heads and the tied self-draft (loops without a draft model); a bound row-sampling table. While a rule is on,
 * sd_specdec_set_spec_sampling, sd_specdec_set_adaptive and a non-NULL sd_specdec_set_row_sampling are refused.
 * Additive (SD_ABI_VERSION stays 1). */
int sd_specdec_set_acceptance(sd_specdec* s, int rule, float temperature, float epsilon, float delta, int agree_k, void* logits_buf,
                              size_t logits_bytes);

/* Per-token log-probs inside the step (sd_token_logprobs' row pass on the verify forward's own rows). While on, the verify forward
 * stores its [B][K+1][V] logits (in the buffer of whichever mode already stores them, else logits_buf; a plain greedy step then
 * takes its three launches — ids, accept, record — instead of the fused tail) and ONE launch, after the accept stage and the
 * logit-processor stage and before the record, describes every emitted token: workgroup (b, i), i = 0..K, handles new_tok[b][i] iff
 * row b is active and i < n_new[b], from row (b, i) — the target's distribution after d_1..d_i, the (processed) row that token was
 * checked against or drawn from in every select mode, at temperature 1 and before any top-k / top-p shaping. Every other (b, i)
 * gets the "no record" value (logprob NaN, rank -1, ids -1). The words go to pinned host memory, sd_specdec_logprobs(): TWO slots
 * of [B][K+1][W], W = sd_specdec_logprob_words() = 2 + 2 N, N = min(top_n, V); launch i writes slot i & 1, the slot of its step
 * record. Words of (b, i): [0] logprob (float bits) [1] rank [2 .. 2+N) top ids [2+N .. 2+2N) top log-probs (float bits).
 * The step record and sd_specdec_record_ints() are unchanged. enable = 0 (the default): the step is launch for launch what it is
 * without this call. Enabling, changing top_n and disabling (if it was on) drop the captured graph; the caller has drained the loop.
 * logits_buf: caller-owned [B][K+1][V] bf16, 16-byte aligned — the buffer the other modes were handed, when any is on.
 * Refused: top_n outside 0..20; a NULL, short or misaligned buffer; loops without a draft model (self-draft, Medusa heads, EAGLE);
 * SD_EMIT_DRAFT; per-row adaptive K and confidence-gated draft length, whose setters in turn refuse while this mode is on.
 * Additive (SD_ABI_VERSION stays 1). */
int sd_specdec_set_logprobs(sd_specdec* s, int enable, int top_n, void* logits_buf, size_t logits_bytes);

/* Per-row adaptive K inside the captured step ("AdaptiveKController driving per-row K inside a
 * captured graph"; the rule is the reference's AdaptiveKController.get_k, src/specdec/policies/controllers.py:100-126,
 * which the reference applies to one K for the whole batch from the host, pipeline.py:1994-2014). The loop keeps the
 * SHAPE K it was created with (= max_k): every step still drafts and verifies K positions per row, but for row b only
 * the first k_row[b] proposals count — accept length = min(longest matching prefix, k_row[b]), emitted tokens and the
 * bonus token follow from that length exactly as in a step run at K = k_row[b] — and after the accept scan the device
 * applies the controller rule to the row's own counters (accepted / proposed so far, strict), so the next step can
 * be launched without a host round trip. History starts as [0.0] (the reference's first get_k reports rate 0.0), the
 * mean of the last four rates is compared with target_rate +- 0.1, K moves by step_size inside [min_k, max_k];
 * double arithmetic in the reference's order. Requires 1 <= min_k <= initial_k <= max_k <= K. The step record gains a
 * last int per row: the k that counted in that step (K when adaptive K is off). enable = 0 returns to fixed K.
 * Either call drops the captured graph. Not available with persistent Medusa heads / EAGLE-lite. */
int sd_specdec_set_adaptive(sd_specdec* s, int enable, int initial_k, int min_k, int max_k, int step_size,
                            double target_rate, void* stream);
/* (Re)write row b's controller state: a new sequence in the row's slot (k = initial_k, 0, 0, hist = NULL -> [0.0]), or
 * the host's in-order view after its rules overrode steps that had been launched ahead. `hist`: hist_n <= 4 rates,
 * oldest first. Asynchronous on `stream` (synchronises it first: one pinned staging slot per row). */
int sd_specdec_set_adaptive_row(sd_specdec* s, int b, int k, int accepted, int proposed, int hist_n,
                                const double* hist, void* stream);

/* Confidence-gated draft length inside the captured step (csrc/draft_confidence.hip; the stopping rule of HF assisted generation's
 * assistant_confidence_threshold, decided on the device between two draft forwards). The loop keeps its SHAPE K. For row b and
 * draft forward i = 0..K-1, with x the bf16 logits row of the forward's last position as the forward stores it and d_{i+1} its
 * fused argmax, as without the mode:
 *   confidence   c_i = sd_draft_confidence(x): the temperature-1 softmax probability of the largest stored value, NaN for a
 *                row with a NaN or a maximum that is not finite
 *   stop         k_b = the smallest i + 1 >= min_k with !(c_i >= tau), else K. The token drawn at low confidence is still
 *                proposed (HF's ConfidenceCriteria); a NaN stops the row
 *   what counts  only row b's first k_b proposals: accept length = min(longest matching prefix, k_b); emitted tokens, the bonus
 *                token, the state advance and the form of the next draft forward 0 follow from that length exactly as
 *                sd_specdec_set_adaptive defines them for k_row[b]
 *   record       slot [5+3K] is k_b
 *   gating       draft forward i >= 1 runs iff some active row has k_b > i; otherwise each of its launches returns at entry. Draft
 *                token slots past the widest row's k_b are unspecified; a row that stopped rides along in later forwards and its
 *                tokens there do not count
 *   reset        k_b starts at K in every step: nothing is carried between steps, the host mirrors nothing
 * One launch per judged forward (i = min_k-1 .. K-2; forward K-1 needs no judgement) follows the forward's hand-over launch on the
 * draft's stream: one 1024-thread workgroup per row; a row that stops writes k_b, a row that continues stores the constant i + 2 into
 * the gate word of forward i + 1 (every writer stores the same value: no atomic, no reduction across rows). The step's last
 * launch on the target stream puts the words back; nothing is added on the target stream. Only judged forwards store a row.
 * logits_buf: caller-owned bf16, sd_specdec_draft_confidence_bytes(B, V) bytes ([B][2][V]: the two positions of draft forward 0),
 * 16-byte aligned. conf_out (nullable, device float [B][K], 4-byte aligned): the step's c_i for every judged forward that ran, NaN
 * elsewhere; the call itself fills it with NaN, so it reads NaN before the first step and where no forward is judged (min_k == K). enable = 0 (the default): the step is launch for launch and bit for bit what it is without this call. Either call
 * drops the captured graph. Refused: tau outside (0, 1] or NaN; min_k outside 1..K; a NULL, short or misaligned buffer; loops
 * without a draft model (self-draft, Medusa heads, EAGLE); SD_EMIT_DRAFT; and while on: per-row adaptive K, speculative sampling,
 * an acceptance rule, logit processors / a grammar, a bound row-sampling table — whose setters in turn refuse while this mode is
 * on. The sampled-bonus mode stays allowed (it concerns the target's rows). Additive (SD_ABI_VERSION stays 1). */
size_t sd_specdec_draft_confidence_bytes(int B, int V);
int sd_specdec_set_draft_confidence(sd_specdec* s, int enable, float tau, int min_k, void* logits_buf, size_t logits_bytes,
                                    float* conf_out);

/* EAGLE-lite drafting (the reference's _run_eagle_hf, src/specdec/core/pipeline.py:765-889, under greedy decoding), for
 * a loop created with draft = NULL: every step runs a 1-token target forward for the residual row of the last token,
 * h_t = final_norm(row); extrapolates K hidden rows h_1 = h_t + alpha (h_t - E), h_2 = h_1 + alpha (h_1 - h_t), ...
 * (E = the last extrapolated row of the previous step of that batch row; on a row's first step h_t stands in for it;
 * every operation rounds to bf16 as the reference's bf16 tensors do); scores all K rows with ONE lm_head launch
 * (d_i = argmax lm_head(h_i)); then verifies (last, d_1..d_K) as usual. K = min(k, eagle.max_draft) is the caller's
 * choice at sd_specdec_create. `workspace` (sd_specdec_eagle_bytes, caller-owned device memory, must outlive the loop)
 * holds the per-row state (at offsets independent of K: loops of different K may share one workspace sized for the
 * largest) and the extrapolated rows. Call before the first step, then sd_specdec_reset_eagle, which forgets the state
 * of all rows (start of a new set of sequences; enqueued on `stream`) — set_eagle itself does not touch the state. */
size_t sd_specdec_eagle_bytes(int B, int K, int d_model);
int sd_specdec_set_eagle(sd_specdec* s, float alpha, void* workspace, size_t workspace_bytes);
int sd_specdec_reset_eagle(sd_specdec* s, void* stream);

/* Persistent multi-head (Medusa) drafting for a loop created with draft = NULL: K heads, each a
 * vocabulary-sized matrix [V][d_model] packed by sd_pack_head in `weight_dtype`. After the accept scan of a step
 * the heads read the target's final-norm input row of the position that produced the last emitted token and
 * propose d_{i+1} = argmax head_i(norm(h)) for the NEXT step, no draft forwards. Heads that sit at a CONSTANT byte
 * stride (packed_heads[i+1] - packed_heads[i] equal for all i, e.g. one buffer of K slots) are evaluated by ONE launch
 * (one matrix per grid row over the same hidden rows) + one argmax finalize; otherwise one launch per head. Up to 9
 * rows read the hidden rows in place; more (within one verify pass: B*(K+1) <= 64) are gathered first and take the
 * multi-token kernel, one launch per head.
 * (Not in the reference: its Medusa mode re-creates random heads per call, pipeline.py:689-705)
 * Requires B*(K+1) within one verify pass. Drops the captured graph. */
int sd_specdec_set_medusa(sd_specdec* s, int n_heads, const void* const* packed_heads, int weight_dtype);

/* The head evaluation of the Medusa and EAGLE steps on caller-supplied rows (a test / diagnostic entry: the step and this
 * call run one function, so what it returns is what a step would propose from the same bits). `m` gives the shape
 * ([vocab][d_model]), the final norm and the workspace; x_bf16 holds n_rows device rows of d_model bf16 values; row b of the
 * B evaluated rows is row row_idx[b] of x (device int32 [B]; NULL: row b). packed_heads: n_heads (1..64) matrices packed
 * by sd_pack_head in `weight_dtype` for this model's vocab and d_model. Heads at a constant ascending stride take the one
 * launch of sd_specdec_set_medusa, others one launch each; more rows than one GEMV pass of this model holds (9, fewer for
 * wide activation rows: 5 at d_ff 14336) are gathered (row_idx given) and take the multi-token kernel, one launch per head. flags: SD_HEADS_PER_HEAD forces one launch per head (what SPECDEC_MEDUSA_PER_HEAD does to a
 * loop); SD_HEADS_NORMALISED says the rows are final-norm outputs already (no norm in front of the product: the launch
 * of the EAGLE step over its extrapolated rows).
 * Out: ids int32 [B][n_heads], and, when vals is not NULL, fp32 [B][n_heads]: the value the kernels attached to each
 * winning index (the bf16-rounded logit, read from the launch's partials before anything reuses them); when launch_info (host
 * int[2]) is not NULL, the matrix launches the call enqueued (1 = the one launch) and whether the rows were gathered first.
 * Refused: unbound model, NULL or misaligned heads, unknown dtype / flags, fp8 with d_model % 64 != 0, B above one pass of
 * the head kernels, a row index outside [0, n_rows) (the indices are read back and checked: the call synchronises
 * `stream` when row_idx is given). Must not run concurrently with a forward or a step of `m` (it uses m's partials). */
#define SD_HEADS_PER_HEAD 1
#define SD_HEADS_NORMALISED 2
int sd_model_head_argmax(sd_model* m, const void* x_bf16, int n_rows, const int32_t* row_idx, int B, int n_heads,
                         const void* const* packed_heads, int weight_dtype, int flags, int32_t* ids, float* vals, int* launch_info,
                         void* stream);

/* The extrapolation launch of the EAGLE step on caller-supplied buffers (test / diagnostic entry; the step launches the
 * same kernel): x bf16 [B][d_model] residual rows, H bf16 [B*K][d_model] out, prev bf16 [B][d_model] and has_prev int32 [B]
 * the per-row state, read and then overwritten (prev <- h_K, has_prev <- 1). norm_w / norm_b: bf16 [d_model] (norm_b only
 * for rms = 0, LayerNorm). K in 1..8. */
int sd_eagle_extrapolate(const void* x_bf16, void* H, void* prev, int32_t* has_prev, const void* norm_w, const void* norm_b,
                         float eps, float alpha, int d_model, int B, int K, int rms, void* stream);

/* Enqueue ONE draft-then-verify step for all rows: K draft forwards (the first over
 * (prev,last), the rest over one token), one verify forward over (last,d_1..d_K),
 * the accept scan (wave ballot), the in-place state advance, and the copy of the
 * step record to pinned host memory. Draft work goes to stream_draft, verify to
 * stream_target, ordered by events; with use_graph=1 the whole step is captured
 * into a hipGraph on first use and replayed afterwards. */
int sd_specdec_step(sd_specdec* s, void* stream_target, void* stream_draft, int use_graph);

/* Steps launched so far, and a wait for ONE of the last two launches (0-based index) without draining the stream:
 * the host may keep a second step queued behind the running one (the device advances its own state) and still read
 * the record of the older one — slot (index & 1) of sd_specdec_record. */
long sd_specdec_launches(const sd_specdec* s);
/* Nodes of the captured step's graph (kernel launches and the event nodes of the two-stream fork and join); 0 while no step is
 * captured, -1 if the runtime refuses the query. Host-only, additive (SD_ABI_VERSION stays 1): tests compare the step's launch
 * count between modes with it. */
long sd_specdec_graph_nodes(const sd_specdec* s);
int sd_specdec_wait(sd_specdec* s, long launch_index);

/* Drop the captured step (its kernels were chosen at capture time: after sd_model_set_persist_tokens /
 * sd_model_set_length_hint changed a model's path, or a model was re-bound). The next sd_specdec_step runs eagerly, the
 * one after it captures again. The caller has drained the loop's streams. */
int sd_specdec_invalidate(sd_specdec* s);

/* Block until everything enqueued on `stream` is done (hipStreamSynchronize). */
int sd_specdec_sync(sd_specdec* s, void* stream);

/* Pinned host records, written by the device at the end of each step: TWO slots of [B][record_ints], the
 * record of launch i (0-based, sd_specdec_launches) is in slot i & 1. Ints per row:
 *   [0] accept_len  [1] n_new  [2] cur_len after the step
 *   [3 .. 3+K]            emitted tokens (n_new valid, -1 padded)
 *   [4+K .. 3+2K]         draft tokens d_1..d_K
 *   [4+2K .. 4+3K]        target argmax t_0..t_K
 *   [5+3K]                proposals that counted for the row in this step (K unless sd_specdec_set_adaptive /
 *                         sd_specdec_set_draft_confidence)
 *   [6+3K]                health word of the models' persistent launches (sd_model_engine_status), 0 = all completed
 * row stride = sd_specdec_record_ints(). */
const int32_t* sd_specdec_record(const sd_specdec* s);
int sd_specdec_record_ints(const sd_specdec* s);
/* The log-prob words of sd_specdec_set_logprobs: pinned, two slots of [B][K+1][sd_specdec_logprob_words()], slotted as the
 * records. NULL until the mode was first enabled; the word count is 0 while it is off. */
const int32_t* sd_specdec_logprobs(const sd_specdec* s);
int sd_specdec_logprob_words(const sd_specdec* s);

#ifdef __cplusplus
}
#endif
#endif /* SPECDEC_HIP_H */
