// Decoder forward orchestration and the draft-then-verify step for gfx950.
//
// Host-side C++ behind the C-ABI (include/specdec_hip.h). It enqueues the kernels
// of gemv.hip / attention.hip / misc.hip on caller-provided HIP streams, never
// synchronises, and is graph-capturable: all per-row dynamic quantities (lengths,
// tokens) live in device memory and are read by the kernels.
//
// What it replaces in the reference: HFWrapper._generate_tokens_async
// (hf_wrappers.py:272-627: one HF forward + argmax per generated token, the whole
// prefix re-fed unless a KV cache is threaded through) and the device-facing half of
// the step loop of SpeculativePipeline.generate_batch (pipeline.py:2306-2846: draft
// stream / verify stream / event waits). The reference verifies by letting the base
// model generate K tokens autoregressively (speculative_scheduler.py:192-199); here
// the target scores all K+1 positions in ONE forward over (last, d_1..d_K), which
// under greedy decoding yields the same accepted prefix and bonus token.

#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>

#include "engine.h"
#include "persist.h"
#include "prefill_gemm.h"

struct sd_model {
  sd_model_config cfg;
  std::vector<sd_layer_weights> layers;
  // bound storage
  uint16_t* k_cache = nullptr;
  uint16_t* v_cache = nullptr;
  int B = 0, Lmax = 0;
  // paged KV (sd_model_bind_paged): k_cache / v_cache are page pools of n_pages pages per layer, Lmax = max_pages * page_len
  const int32_t* block_table = nullptr;   // device [B][max_pages], caller-owned and caller-maintained
  int page_shift = 0, max_pages = 0, n_pages = 0;
  // workspace carve
  uint16_t* x = nullptr;     // [64][d]
  uint16_t* q = nullptr;     // [64][Hq*D]
  uint16_t* attn = nullptr;  // [64][Hq*D]
  uint16_t* act = nullptr;   // [64][ff]
  int32_t* probe_pos = nullptr;  // [1] zero: position base of the QKV probe
  float* attn_ws = nullptr;      // split-KV partial tiles (attention.hip)
  unsigned* attn_cnt = nullptr;  // arrival counters, zero between launches
  float* xstat = nullptr;    // [2][128][256]: row statistics handed from an EPI_RESID launch to the next norm-fused one (> 9 tokens)
  float* part_val = nullptr; // [64][512]
  int small_t = sd::kGemvMaxT; // tokens per pass of gemv.hip for this model's widest activation row (<= 9)
  int max_t = sd::kGemvMaxT; // tokens per pass: 64 when every matrix of the model is covered by gemm_skinny.hip
  int* part_idx = nullptr;
  int head_grid = 0;         // grid of the last lm_head launch (partials per token)
  const int32_t* skip_k = nullptr;   // set around a draft forward of the adaptive step (enqueue_step): every launch of the
  int skip_i = 0;                    // forward returns at entry when *skip_k <= skip_i
  std::vector<const void*> packed;  // per matrix (4 per layer + lm_head) or empty: row-major weights
  std::vector<const float*> scales; // fp8 storage: fp32 row scales per matrix
  const void* mat(int index, const void* row_major) const { return packed.empty() ? row_major : packed[index]; }
  int is_packed() const { return packed.empty() ? 0 : 1; }
  int w8() const { return scales.empty() ? 0 : 1; }
  const float* scale(int index) const { return scales.empty() ? nullptr : scales[index]; }
  // persistent forward (csrc/persist.hip): passes of <= persist_t tokens run as ONE launch
  int persist_t = 0;                       // 0 = not available for this model / device
  bool persist_taps = true;                // stage rows written by persistent passes (sd_specdec_create turns them off for its draft)
  sd::PersistOp* p_ops = nullptr;          // device: 4 per layer + lm_head, stream order
  unsigned long long* p_gran = nullptr;    // granule buffers, two parities
  unsigned p_gran_parity = 0;
  unsigned* p_sync = nullptr;              // [0] launch counter, [1] status
  unsigned long long* p_debug = nullptr;   // optional timeline (sd_model_probe_persist)
  void* prefill_ws = nullptr;              // lazily allocated workspace of the GEMM prefill path (csrc/prefill_gemm.hip)
  int prefill_backend = SD_PREFILL_AUTO;   // sd_model_set_prefill_backend (a bind resets it)
  int64_t prefill_count[4] = {0, 0, 0, 0}; // prompt rows absorbed per backend since the bind (index: enum sd_prefill_backend)
  sd::NativePlan native_plan;              // row-block tables of the native prefill GEMM (built at its first use)
  sd::PrefillRows prefill_rows;            // the last GEMM-prefill chunk's rows in prefill_ws (sd_model_prefill_rows), valid while
  int prefill_mc = 0;                      // prefill_mc > 0: cleared by a bind and by every pass that is not such a chunk
  void* score_ws = nullptr;                // sd_model_score: normed rows, head partials, target logits, a zero word (first call)
  unsigned* host_status = nullptr;         // pinned host word: a persistent launch that gives up stores its reason here as well
  int persist_cap = 0;                     // tokens per persistent pass this model / device / cache can take (0: none)
  int len_hint = 0;                        // caller's bound on the rows' current lengths (sd_model_set_length_hint; default Lmax)
  int ctx_limit = 0;                       // longest rows the persistent launch serves (kPersistMaxCtx; lifted by SPECDEC_PERSIST_MAX_T)
  ~sd_model() {
    if (host_status) (void)hipHostFree(host_status);
    if (prefill_ws) (void)hipFree(prefill_ws);
    if (score_ws) (void)hipFree(score_ws);
    sd::native_plan_free(native_plan);
  }
};

namespace sd {
// One CU (three waves) walks a head's whole cache in the persistent launch, where the launch path splits long rows over up to 32
// workgroups — 1B dimensions, 1 token, us per forward persistent / launches at 128 ... 4096 cached positions: 588 / 675,
// 605 / 694, 651 / 721, 723 / 764, 888 / 767, 1186 / 777 (profiles/round3_persist_ab.md): the persistent launch serves rows of
// up to this many positions (where the two lines cross: 723 + 0.161 (L - 1024) against 764 + 0.003 (L - 1024) us at L = 1283;
// round 4's context sweep: 5.07 ms per step on the persistent launch at 1400-1536 positions against 4.96 on the launch path at 2048).
constexpr int kPersistMaxCtx = 1280;
static bool persist_pass_ok(const sd_model* m, int T, int Bc, int Mc) {
  return m->persist_t > 0 && T <= m->persist_t && Mc <= 8 && !m->block_table && Bc * m->cfg.n_heads <= kPersistCUs && m->len_hint <= m->ctx_limit;
}
}  // namespace sd

namespace sd {

constexpr int kMaxPartials = 512;

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

static size_t workspace_bytes(const sd_model_config& c) {
  const size_t T = kSkinnyMaxT;
  size_t n = 0;
  n += align_up(T * c.d_model * 2, 256);
  n += align_up(T * c.n_heads * c.head_dim * 2, 256) * 2;
  n += align_up(T * c.d_ff * 2, 256);
  n += align_up(T * kMaxPartials * 4, 256) * 2;
  n += align_up(attention_split_ws_bytes(c.head_dim), 256);
  n += align_up(sizeof(float) * 2 * kStatPlane, 256);
  n += align_up(persist_workspace_bytes(c), 256);
  return n + 256;
}

// Matrix `index` (4 * layer + which; 4 * n_layers = the lm_head) as the forward launches it: weights, shape and bias, the fused
// norm, and the workspace rows it reads and writes. The caller adds what belongs to the call: tokens, positions, caches, statistics.
static GemvArgs matrix_args(const sd_model* m, int index) {
  const sd_model_config& c = m->cfg;
  const int which = matrix_which(c, index);
  const MatShape sh = matrix_shape(c, which);
  const MatWeights wt = matrix_weights(c, index);
  GemvArgs a{};
  a.W = m->mat(index, wt.w);
  a.w_scale = m->scale(index);
  a.packed = m->is_packed();
  a.w8 = m->w8();
  a.bias = wt.bias;
  a.N = sh.N;
  a.K = sh.K;
  a.n_pairs = sh.n_pairs;
  if (wt.norm_w) {
    a.prologue = c.arch == SD_ARCH_LLAMA ? PRO_RMSNORM : PRO_LAYERNORM;
    a.norm_w = wt.norm_w;
    a.norm_b = wt.norm_b;
    a.norm_eps = c.norm_eps;
  }
  const int d = c.d_model, HqD = c.n_heads * c.head_dim, ff = c.d_ff;
  const struct { const uint16_t* x; int x_stride; uint16_t* out; int out_stride; } rows[5] = {
      {m->x, d, m->q, HqD}, {m->attn, HqD, m->x, d}, {m->x, d, m->act, ff}, {m->act, ff, m->x, d}, {m->x, d, nullptr, 0}};
  a.x = rows[which].x;
  a.x_stride = rows[which].x_stride;
  a.out = rows[which].out;
  a.out_stride = rows[which].out_stride;
  a.out_dtype = SD_BF16;
  if (which == 4) {   // the head's argmax partials
    a.part_val = m->part_val;
    a.part_idx = m->part_idx;
  }
  return a;
}

// one pass: Bc rows x Mc tokens, Bc*Mc <= m->max_t
static int forward_pass(sd_model* m, const int32_t* tokens, int tok_stride, const int32_t* pos_base,
                        int pos_off, int row0, int b0, int Bc, int Mc, int32_t* ids_out, int ids_stride,
                        void* logits_out, int logits_dtype, int logits_stride, int skip_head,
                        hipStream_t st) {
  const sd_model_config& c = m->cfg;
  m->prefill_mc = 0;   // this pass's rows are the model's last: the record of a GEMM-prefill chunk ends here
  const int T = Bc * Mc;
  const int d = c.d_model, Hq = c.n_heads, Hkv = c.n_kv_heads, D = c.head_dim, ff = c.d_ff;
  const bool llama = (c.arch == SD_ARCH_LLAMA);

  // ---- the whole pass as ONE persistent launch (csrc/persist.hip): small passes of a dense-KV Llama model
  if (persist_pass_ok(m, T, Bc, Mc)) {
    PersistArgs pa{};
    pa.ops = m->p_ops;
    pa.n_ops = 4 * c.n_layers + (skip_head ? 0 : 1);
    pa.d_model = d; pa.n_q_heads = Hq; pa.n_kv_heads = Hkv; pa.head_dim = D; pa.d_ff = ff; pa.vocab = c.vocab;
    pa.n_layers = c.n_layers; pa.max_pos = c.max_pos;
    pa.norm_eps = c.norm_eps;
    pa.attn_scale = 1.0f / sqrtf(static_cast<float>(D));
    pa.tok_emb = c.tok_emb;
    pa.rope_cos = c.rope_cos;
    pa.rope_sin = c.rope_sin;
    pa.tokens = tokens + static_cast<size_t>(b0) * tok_stride;
    pa.tok_stride = tok_stride;
    pa.pos_base = pos_base + b0;
    pa.pos_off = pos_off;
    pa.B = Bc;
    pa.M = Mc;
    const size_t row_off = static_cast<size_t>(row0 + b0) * Hkv * m->Lmax * D;
    pa.k_cache = m->k_cache + row_off;
    pa.v_cache = m->v_cache + row_off;
    pa.layer_kv = static_cast<size_t>(m->B) * Hkv * m->Lmax * D;
    pa.l_max = m->Lmax;
    pa.logits = logits_out;
    pa.logits_dtype = logits_dtype;
    pa.logits_stride = logits_stride;
    pa.part_val = m->part_val;
    pa.part_idx = m->part_idx;
    pa.x = m->x; pa.q = m->q; pa.attn = m->attn; pa.act = m->act;
    pa.gran = m->p_gran;
    pa.gran_parity = m->p_gran_parity;
    pa.sync = m->p_sync;
    pa.host_status = m->host_status;
    pa.skip_k = m->skip_k;
    pa.skip_i = m->skip_i;
    pa.taps = (m->persist_taps || skip_head) ? 1 : 0;   // (a pass without the head is run FOR its hidden rows)
    pa.debug_ts = m->p_debug;
    if (int rc = launch_persist_forward(pa, st)) return rc;
    if (skip_head) return 0;
    m->head_grid = kPersistCUs;
    if (ids_out) {
      if (int rc = launch_argmax_finalize(m->part_val, m->part_idx, T, m->head_grid, Mc, ids_stride,
                                          ids_out + static_cast<size_t>(b0) * ids_stride, st, m->skip_k, m->skip_i))
        return rc;
    }
    return 0;
  }

  EmbedArgs e{};
  e.tok_emb = c.tok_emb;
  e.pos_emb = llama ? nullptr : c.pos_emb;
  e.tokens = tokens + static_cast<size_t>(b0) * tok_stride;
  e.tok_stride = tok_stride;
  e.pos_base = pos_base + b0;
  e.pos_off = pos_off;
  e.M = Mc;
  e.T = T;
  e.d = d;
  e.vocab = c.vocab;
  e.max_pos = c.max_pos;
  e.x = m->x;
  e.skip_k = m->skip_k;
  e.skip_i = m->skip_i;
  if (int rc = launch_embed(e, st)) return rc;

  const bool paged = m->block_table != nullptr;
  const size_t layer_kv = paged ? (static_cast<size_t>(m->n_pages) * Hkv * D << m->page_shift) : static_cast<size_t>(m->B) * Hkv * m->Lmax * D;
  const size_t row_kv = paged ? 0 : static_cast<size_t>(row0 + b0) * Hkv * m->Lmax * D;    // paged: rows are found through the table
  const int32_t* bt = paged ? m->block_table + static_cast<size_t>(row0 + b0) * m->max_pages : nullptr;
  // > 9 tokens: the launch that writes the residual stream hands its row statistics to the launch that normalises it
  const float* stat_in = nullptr;
  int stat_n = 0;
  auto publish = [&](GemvArgs& prod) {      // prod: an EPI_RESID launch about to be issued
    stat_in = nullptr;
    if (m->xstat && gemm_resid_publishes_stats(prod)) {
      prod.xstat_out = m->xstat;
      stat_in = m->xstat;
      int ppw = 1;
      stat_n = gemv_grid(prod, &ppw);
    }
  };
  for (int l = 0; l < c.n_layers; ++l) {
    uint16_t* kc = m->k_cache + l * layer_kv + row_kv;
    uint16_t* vc = m->v_cache + l * layer_kv + row_kv;
    auto layer_args = [&](int which) {
      GemvArgs g = matrix_args(m, 4 * l + which);
      g.T = T;
      g.M = Mc;
      g.pos_base = pos_base + b0;
      g.pos_off = pos_off;
      g.head_dim = D;
      g.n_q_heads = Hq;
      g.n_kv_heads = Hkv;
      g.max_pos = c.max_pos;
      g.l_max = m->Lmax;
      g.block_table = bt;
      g.page_shift = m->page_shift;
      g.skip_k = m->skip_k;
      g.skip_i = m->skip_i;
      return g;
    };

    // 1. norm + QKV projection + RoPE + in-place KV append
    GemvArgs a1 = layer_args(0);
    a1.rope_cos = llama ? c.rope_cos : nullptr;
    a1.rope_sin = llama ? c.rope_sin : nullptr;
    a1.k_cache = kc;
    a1.v_cache = vc;
    a1.xstat_in = stat_in;
    a1.xstat_n = stat_n;
    if (int rc = launch_gemv(a1, EPI_QKV_ROPE, st)) return rc;

    // 2. attention of the Mc new positions over the appended cache
    AttnArgs at{};
    at.q = m->q;
    at.k_cache = kc;
    at.v_cache = vc;
    at.out = m->attn;
    at.pos_base = pos_base + b0;
    at.pos_off = pos_off;
    at.B = Bc;
    at.M = Mc;
    at.n_q_heads = Hq;
    at.n_kv_heads = Hkv;
    at.head_dim = D;
    at.l_max = m->Lmax;
    at.scale = 1.0f / sqrtf(static_cast<float>(D));
    at.split_ws = m->attn_ws;
    at.split_cnt = m->attn_cnt;
    at.split_slots = kAttnSplitSlots;
    at.block_table = bt;
    at.page_shift = m->page_shift;
    at.skip_k = m->skip_k;
    at.skip_i = m->skip_i;
    if (int rc = launch_attention(at, st)) return rc;

    // 3. output projection + residual, 4. norm + up projection (+ gate) + activation
    GemvArgs a3 = layer_args(1);
    GemvArgs a4 = layer_args(2);
    publish(a3);
    a4.xstat_in = stat_in;
    a4.xstat_n = stat_n;
    if (int rc = launch_gemv(a3, EPI_RESID, st)) return rc;
    if (int rc = launch_gemv(a4, matrix_shape(c, 2).epi, st)) return rc;

    // 5. down projection + residual
    GemvArgs a5 = layer_args(3);
    publish(a5);
    if (int rc = launch_gemv(a5, EPI_RESID, st)) return rc;
  }
  if (skip_head) return 0;

  // final norm + lm_head with the argmax fused into the epilogue
  GemvArgs h = matrix_args(m, 4 * c.n_layers);
  h.T = T;
  h.M = Mc;
  h.out = logits_out;
  h.out_stride = logits_stride;
  h.out_dtype = logits_dtype;
  h.xstat_in = stat_in;
  h.xstat_n = stat_n;
  h.skip_k = m->skip_k;
  h.skip_i = m->skip_i;
  int ks = 1;
  m->head_grid = gemv_grid(h, &ks);
  if (int rc = launch_gemv(h, EPI_ARGMAX, st)) return rc;
  if (ids_out) {
    if (int rc = launch_argmax_finalize(m->part_val, m->part_idx, T, m->head_grid, Mc, ids_stride,
                                        ids_out + static_cast<size_t>(b0) * ids_stride, st, m->skip_k, m->skip_i))
      return rc;
  }
  return 0;
}

// final norm + lm_head + fused argmax over n <= 128 residual rows (bf16 [n][d_model]) -> ids[0..n)
static int head_pass(sd_model* m, const uint16_t* xrows, int n, int32_t* ids, hipStream_t st) {
  GemvArgs h = matrix_args(m, 4 * m->cfg.n_layers);
  h.x = xrows;
  h.T = n;
  h.M = n;
  int ks = 1;
  m->head_grid = gemv_grid(h, &ks);
  if (int rc = launch_gemv(h, EPI_ARGMAX, st)) return rc;
  return launch_argmax_finalize(m->part_val, m->part_idx, n, m->head_grid, n, n, ids, st);
}

// The route of a prompt. A prompt (M >= 96 positions per row, whatever the pass size of the decode-shaped kernels) is absorbed as GEMMs
// (csrc/prefill_gemm.hip: <= 512 positions per chunk, every matrix product one GEMM, this repo's norm / epilogue / attention kernels
// around them) when the caller wants no logits of the prompt positions (skip_head, or ids only: the head then runs over each chunk's
// rows), the pass is not being captured and no adaptive-K word gates it. Which GEMM (sd_model_set_prefill_backend): SD_PREFILL_AUTO =
// rocBLAS for a Llama model with bf16 row-major weights and dense KV when the library opens, else the passes; SD_PREFILL_ROCBLAS /
// _NATIVE = that GEMM (validated when it was set); SD_PREFILL_PASSES = never a GEMM. Returns the backend, or -1 when M is below the
// prefill minimum (the passes, not counted as a prompt).
static int prefill_route(const sd_model* m, int M, bool logits, hipStream_t st) {
  static const int prefill_min = getenv(debug_env::kPrefillMinTokens) ? atoi(getenv(debug_env::kPrefillMinTokens)) : kPrefillMinTokens;
  if (M < prefill_min) return -1;
  int backend = SD_PREFILL_PASSES;
  const bool gemm_ok = m->cfg.arch == SD_ARCH_LLAMA && !logits && !m->skip_k;
  if (m->prefill_backend == SD_PREFILL_AUTO) {
    if (gemm_ok && !m->w8() && !m->block_table && m->cfg.weight_dtype == SD_BF16 && !getenv(debug_env::kNoGemmPrefill) && prefill_gemm_available())
      backend = SD_PREFILL_ROCBLAS;
  } else if (m->prefill_backend != SD_PREFILL_PASSES && gemm_ok) {
    backend = m->prefill_backend;
  }
  if (backend != SD_PREFILL_PASSES) {
    hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cap_st);
    if (cap_st != hipStreamCaptureStatusNone) backend = SD_PREFILL_PASSES;
  }
  return backend;
}

// One row's prompt of M positions through the GEMM `backend` (prefill_route), in chunks of <= kPrefillChunk positions in position
// order; on_chunk(m0, mc, x) runs the caller's head over each chunk's residual rows (bf16 [mc][d_model]).
template <class OnChunk>
static int prefill_row(sd_model* m, int backend, const int32_t* tokens, const int32_t* pos_base_row, int pos_off, int row, int M,
                       hipStream_t st, OnChunk&& on_chunk) {
  const sd_model_config& c = m->cfg;
  m->prefill_mc = 0;
  if (!m->prefill_ws) SD_HIP_CHECK(hipMalloc(&m->prefill_ws, prefill_gemm_workspace_bytes(c)));
  PrefillModel pm{&m->cfg, m->k_cache, m->v_cache, m->B, m->Lmax, m->attn_ws, m->attn_cnt};
  pm.block_table = m->block_table;
  pm.page_shift = m->page_shift;
  pm.max_pages = m->max_pages;
  pm.n_pages = m->n_pages;
  if (backend == SD_PREFILL_NATIVE) {
    if (!m->native_plan.buf)
      if (int rc = native_plan_build(c, m->native_plan)) return rc;
    pm.gemm = PREFILL_GEMM_NATIVE;
    pm.packed = m->packed.data();
    pm.scales = m->w8() ? m->scales.data() : nullptr;
    pm.plan = &m->native_plan;
  }
  for (int m0 = 0; m0 < M; m0 += kPrefillChunk) {
    const int mc = (M - m0 < kPrefillChunk) ? M - m0 : kPrefillChunk;
    PrefillRows rows;
    if (int rc = prefill_gemm_chunk(pm, tokens + m0, pos_base_row, pos_off + m0, row, mc, m->prefill_ws, &rows, st)) return rc;
    // the chunk's last <= 128 positions go where every other pass leaves them: the residual rows (hidden rows, the head) and
    // the last layer's q, attention and activation rows (sd_model_debug_rows)
    const int keep = mc < 128 ? mc : 128;
    const size_t HqD = static_cast<size_t>(c.n_heads) * c.head_dim;
    const struct { uint16_t* dst; const uint16_t* src; size_t w; } taps[4] = {
        {m->x, rows.x, static_cast<size_t>(c.d_model)}, {m->q, rows.q, HqD}, {m->attn, rows.attn, HqD}, {m->act, rows.act, static_cast<size_t>(c.d_ff)}};
    for (const auto& tp : taps)
      SD_HIP_CHECK(hipMemcpyAsync(tp.dst, tp.src + static_cast<size_t>(mc - keep) * tp.w, static_cast<size_t>(keep) * tp.w * 2,
                                  hipMemcpyDeviceToDevice, st));
    if (int rc = on_chunk(m0, mc, rows.x)) return rc;
    m->prefill_rows = rows;
    m->prefill_mc = mc;
  }
  return 0;
}

// rows [row0, row0+B) of the bound batch; tokens / pos_base / ids_out / logits_out are
// indexed from row0 (element 0 of each array belongs to row row0)
static int model_forward(sd_model* m, const int32_t* tokens, int tok_stride, const int32_t* pos_base,
                         int pos_off, int row0, int B, int M, int32_t* ids_out, int ids_stride, void* logits_out,
                         int logits_dtype, int skip_head, hipStream_t st) {
  SD_REQUIRE(m && m->k_cache && m->x, "forward: model not bound (sd_model_bind)");
  SD_REQUIRE(row0 >= 0 && B >= 1 && row0 + B <= m->B, "forward: rows [%d,%d) exceeds bound batch %d", row0, row0 + B, m->B);
  SD_REQUIRE(M >= 1, "forward: M=%d", M);
  SD_REQUIRE(tokens && pos_base, "forward: NULL tokens/pos_base");
  const int esz = (logits_dtype == SD_F32) ? 4 : 2;
  SD_REQUIRE(!logits_out || logits_dtype == SD_F32 || logits_dtype == SD_BF16, "forward: logits dtype %d", logits_dtype);
  const int V = m->cfg.vocab;
  const int cap = (B * M <= m->small_t) ? m->small_t : m->max_t;  // tokens per pass
  const int backend = prefill_route(m, M, logits_out != nullptr, st);
  if (backend == SD_PREFILL_PASSES) {
    m->prefill_count[SD_PREFILL_PASSES] += B;
  } else if (backend >= 0) {
    for (int b0 = 0; b0 < B; ++b0) {
      // ids of the prompt positions: the lm_head over the chunk's rows in groups of at most the model's pass size (the decode-shaped
      // head kernel covers no more: 64 rows for some fp8 heads)
      auto head = [&](int m0, int mc, const uint16_t* xr) -> int {
        if (skip_head || !ids_out) return 0;
        for (int s0 = 0; s0 < mc; s0 += m->max_t) {
          const int n = (mc - s0 < m->max_t) ? mc - s0 : m->max_t;
          if (int rc = head_pass(m, xr + static_cast<size_t>(s0) * m->cfg.d_model, n, ids_out + static_cast<size_t>(b0) * ids_stride + m0 + s0, st)) return rc;
        }
        return 0;
      };
      if (int rc = prefill_row(m, backend, tokens + static_cast<size_t>(b0) * tok_stride, pos_base + b0, pos_off, row0 + b0, M, st, head)) return rc;
    }
    m->prefill_count[backend] += B;
    return 0;
  }
  if (M <= cap) {
    const int Bc = cap / M;
    for (int b0 = 0; b0 < B; b0 += Bc) {
      const int nb = (B - b0 < Bc) ? B - b0 : Bc;
      void* lo = logits_out ? static_cast<char*>(logits_out) + static_cast<size_t>(b0) * M * V * esz : nullptr;
      if (int rc = forward_pass(m, tokens, tok_stride, pos_base, pos_off, row0, b0, nb, M, ids_out, ids_stride, lo,
                                logits_dtype, V, skip_head, st))
        return rc;
    }
    return 0;
  }
  // long M (prefill): chunks of `cap` positions, one row at a time, in position order
  for (int b0 = 0; b0 < B; ++b0) {
    for (int m0 = 0; m0 < M; m0 += cap) {
      const int mc = (M - m0 < cap) ? M - m0 : cap;
      void* lo = logits_out ? static_cast<char*>(logits_out) + (static_cast<size_t>(b0) * M + m0) * V * esz : nullptr;
      if (int rc = forward_pass(m, tokens + m0, tok_stride, pos_base, pos_off + m0, row0, b0, 1, mc,
                                ids_out ? ids_out + m0 : nullptr, ids_stride, lo, logits_dtype, V, skip_head, st))
        return rc;
    }
  }
  return 0;
}

// ---- sd_model_score: the layers as the forward runs them, the head as a log-softmax reduction (csrc/score_head.hip)
struct ScoreWs {
  uint16_t* xn;      // [kPrefillChunk][d_model] normed rows
  float4* part;      // score_partial_bytes
  float* tgt;        // [kPrefillChunk] target logits
  int32_t* zero;     // position base of the row (pos0 goes in pos_off)
};

static int score_ws(sd_model* m, ScoreWs& w) {
  const size_t xb = align_up(static_cast<size_t>(kPrefillChunk) * m->cfg.d_model * 2, 256);
  const size_t pb = align_up(score_partial_bytes(m->native_plan), 256);
  const size_t tb = align_up(kPrefillChunk * sizeof(float), 256);
  if (!m->score_ws) {
    SD_HIP_CHECK(hipMalloc(&m->score_ws, xb + pb + tb + 256));
    SD_HIP_CHECK(hipMemset(static_cast<char*>(m->score_ws) + xb + pb + tb, 0, 256));
  }
  char* p = static_cast<char*>(m->score_ws);
  w.xn = reinterpret_cast<uint16_t*>(p);
  w.part = reinterpret_cast<float4*>(p + xb);
  w.tgt = reinterpret_cast<float*>(p + xb + pb);
  w.zero = reinterpret_cast<int32_t*>(p + xb + pb + tb);
  return 0;
}

// the head over rows [m0, m0 + mc) of the sequence, left by the layers at x (rows ldx apart); logits (sd_model_score_logits): bf16 [n][vocab]
static int score_chunk(sd_model* m, const ScoreWs& w, const uint16_t* x, int ldx, int mc, const int32_t* tokens, int n, int m0, float* logprob,
                       int32_t* greedy, uint16_t* logits, hipStream_t st) {
  const int n_target = logits ? 0 : ((n - 1 - m0 < mc) ? n - 1 - m0 : mc);   // token m0 + t predicts tokens[m0 + t + 1]
  if (int rc = launch_final_norm_rows(m->cfg, x, ldx, mc, w.xn, st)) return rc;
  return launch_score_head(m->native_plan, m->packed[4 * m->cfg.n_layers], m->scale(4 * m->cfg.n_layers), m->w8(), w.xn, mc, tokens + m0 + 1,
                           n_target, w.part, w.tgt, logprob ? logprob + m0 : nullptr, greedy ? greedy + m0 : nullptr,
                           logits ? logits + static_cast<size_t>(m0) * m->cfg.vocab : nullptr, st);
}

static int model_score(sd_model* m, const int32_t* tokens, int n, int row, int pos0, float* logprob, int32_t* greedy, uint16_t* logits,
                       hipStream_t st) {
  if (!m->native_plan.buf)
    if (int rc = native_plan_build(m->cfg, m->native_plan)) return rc;
  ScoreWs w{};
  if (int rc = score_ws(m, w)) return rc;
  // the route of model_forward for B = 1, M = n, no logits (the stream is not capturing: refused by the caller)
  const int backend = prefill_route(m, n, false, st);
  if (backend >= 0) m->prefill_count[backend] += 1;
  if (backend > SD_PREFILL_PASSES)
    return prefill_row(m, backend, tokens, w.zero, pos0, row, n, st, [&](int m0, int mc, const uint16_t* xr) {
      return score_chunk(m, w, xr, m->cfg.d_model, mc, tokens, n, m0, logprob, greedy, logits, st);
    });
  // the passes: one pass when n fits, else chunks of `cap` positions in position order; the head over each pass's residual rows
  const int cap = (n <= m->small_t) ? m->small_t : m->max_t;
  for (int m0 = 0; m0 < n; m0 += cap) {
    const int mc = (n - m0 < cap) ? n - m0 : cap;
    if (int rc = forward_pass(m, tokens + m0, n, w.zero, pos0 + m0, row, 0, 1, mc, nullptr, mc, nullptr, SD_BF16, m->cfg.vocab, 1, st)) return rc;
    if (int rc = score_chunk(m, w, m->x, m->cfg.d_model, mc, tokens, n, m0, logprob, greedy, logits, st)) return rc;
  }
  return 0;
}

// the refusals sd_model_score and sd_model_score_logits share (n_min: 2 for a log-likelihood, 1 for logits)
static int score_checks(sd_model* m, const int32_t* tokens, int n, int n_min, int row, int pos0, hipStream_t st) {
  SD_REQUIRE(m, "score: NULL model");
  SD_REQUIRE(tokens, "score: NULL tokens");
  SD_REQUIRE(n >= 2 || n_min < 2, "score: n=%d tokens (a log-likelihood needs at least 2)", n);
  SD_REQUIRE(n >= n_min, "score: n=%d tokens", n);
  SD_REQUIRE(m->is_packed(), "score: the head reads the packed lm_head (this model has none: SPECDEC_NO_PACK)");
  SD_REQUIRE(m->cfg.d_model % 64 == 0, "score: d_model=%d is not a multiple of 64 (the head GEMM's k stage)", m->cfg.d_model);
  SD_REQUIRE(m->k_cache && m->x, "score: model not bound (sd_model_bind)");
  SD_REQUIRE(row >= 0 && row < m->B, "score: row %d outside the bound batch of %d", row, m->B);
  SD_REQUIRE(pos0 >= 0 && pos0 + n <= m->Lmax && pos0 + n <= m->cfg.max_pos, "score: positions [%d,%d) outside the cache rows (%d) / max_pos (%d)",
             pos0, pos0 + n, m->Lmax, m->cfg.max_pos);
  hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
  SD_HIP_CHECK(hipStreamIsCapturing(st, &cap_st));
  SD_REQUIRE(cap_st == hipStreamCaptureStatusNone, "score: the stream is capturing (score allocates its workspace and picks its route on the host)");
  return 0;
}

}  // namespace sd

// ============================================================================ C-ABI
using namespace sd;

extern "C" int sd_model_create(const sd_model_config* cfg, sd_model** out) {
  clear_error();
  SD_REQUIRE(cfg && out, "model_create: NULL argument");
  SD_REQUIRE(cfg->arch == SD_ARCH_LLAMA || cfg->arch == SD_ARCH_GPT2, "model_create: arch %d", cfg->arch);
  SD_REQUIRE(cfg->weight_dtype == SD_BF16 || cfg->weight_dtype == SD_FP8_E4M3,
             "model_create: weight_dtype %d (SD_BF16, or SD_FP8_E4M3 = stream the fp8 copy made by sd_pack_weights)", cfg->weight_dtype);
  SD_REQUIRE(cfg->weight_dtype != SD_FP8_E4M3 || cfg->packed, "model_create: fp8 storage needs the packed buffer of sd_pack_weights");
  SD_REQUIRE(cfg->n_layers > 0 && cfg->d_model > 0 && cfg->n_heads > 0 && cfg->n_kv_heads > 0 &&
                 cfg->head_dim > 0 && cfg->d_ff > 0 && cfg->vocab > 0 && cfg->max_pos > 0,
             "model_create: non-positive dimension");
  SD_REQUIRE(cfg->d_model % 8 == 0 && cfg->d_ff % 8 == 0 && (cfg->n_heads * cfg->head_dim) % 8 == 0,
             "model_create: d_model, d_ff and Hq*D must be multiples of 8");
  SD_REQUIRE(cfg->head_dim % 2 == 0 && cfg->n_heads % cfg->n_kv_heads == 0, "model_create: head layout");
  // the kernels' argument blocks carry these in 8-bit fields (GemvArgs / AttnArgs), and the attention kernel is instantiated
  // for these head sizes only: a direct C caller gets an error, not a truncated geometry
  SD_REQUIRE(cfg->n_heads <= 255 && cfg->n_kv_heads <= 255, "model_create: at most 255 heads (got %d / %d kv)", cfg->n_heads, cfg->n_kv_heads);
  SD_REQUIRE(cfg->head_dim == 32 || cfg->head_dim == 64 || cfg->head_dim == 128, "model_create: head_dim %d (32, 64 or 128)", cfg->head_dim);
  SD_REQUIRE(cfg->tok_emb && cfg->lm_head && cfg->final_norm_w && cfg->layers, "model_create: NULL weights");
  if (cfg->arch == SD_ARCH_LLAMA) SD_REQUIRE(cfg->rope_cos && cfg->rope_sin, "model_create: Llama needs rope tables");
  if (cfg->arch == SD_ARCH_GPT2) SD_REQUIRE(cfg->pos_emb && cfg->final_norm_b, "model_create: GPT-2 needs pos_emb and ln_f bias");
  sd_model* m = new (std::nothrow) sd_model();
  SD_REQUIRE(m, "model_create: out of memory");
  m->cfg = *cfg;
  m->layers.assign(cfg->layers, cfg->layers + cfg->n_layers);
  m->cfg.layers = m->layers.data();
  for (int l = 0; l < cfg->n_layers; ++l) {
    const sd_layer_weights& w = m->layers[l];
    if (!(w.attn_norm_w && w.wqkv && w.wo && w.mlp_norm_w && w.w_up && w.w_down)) {
      delete m;
      SD_REQUIRE(false, "model_create: layer %d has NULL weights", l);
    }
  }
  {
    // 64-token passes need every matrix of the model to be a shape gemm_skinny.hip covers
    const sd_model_config& c = m->cfg;
    const int HqD = c.n_heads * c.head_dim;
    const bool w8 = cfg->weight_dtype == SD_FP8_E4M3;
    auto covers = [&](int T) {
      for (int i = 0; i < 5; ++i)
        if (!gemm_skinny_covers(T, matrix_shape(c, i).n_pairs, matrix_shape(c, i).K, w8)) return false;
      return true;
    };
    // the most tokens every matrix of the model can take in one pass: 128, 64 (x chunks of a pass must fit the LDS) ...
    int cover_t = 0;
    for (int T = kSkinnyMaxT; T >= 16 && !cover_t; T >>= 1)
      if (covers(T)) cover_t = T;
    const bool ok = cover_t != 0;
    const char* env = getenv(debug_env::kMaxPassTokens);  // testing knob: 9 forces the small-T kernel everywhere
    int want = env ? atoi(env) : cover_t;
    if (want > cover_t) want = cover_t;
    int kmax = c.d_model > HqD ? c.d_model : HqD;
    if (c.d_ff > kmax) kmax = c.d_ff;
    m->small_t = gemv_max_tokens(kmax);  // e.g. 5 for d_ff = 14336: x rows must fit the CU's LDS
    if (want < m->small_t) want = m->small_t;
    m->max_t = ok ? want : m->small_t;
  }
  if (cfg->weight_dtype == SD_FP8_E4M3) {
    // every matrix must split into whole 64-k steps per K slice
    for (int i = 0; i < 5; ++i) {
      const MatShape sh = matrix_shape(m->cfg, i);
      const GemvGeom q = gemv_geometry(sh.n_pairs, sh.K);
      if (sh.K % 64 != 0 || q.kw % 64 != 0 || q.kw * q.ksplit != sh.K) {
        delete m;
        SD_REQUIRE(false, "model_create: fp8 storage does not cover a matrix with K=%d (K slice %d)", sh.K, q.kw);
      }
    }
  }
  if (cfg->packed) {
    const char* base = static_cast<const char*>(cfg->packed);
    for (int i = 0; i <= 4 * cfg->n_layers; ++i) {
      m->packed.push_back(base + packed_offset(m->cfg, i));
      const MatShape sh = matrix_shape(m->cfg, matrix_which(m->cfg, i));
      if (cfg->weight_dtype == SD_FP8_E4M3)   // the fp32 row scales follow the packed bytes
        m->scales.push_back(reinterpret_cast<const float*>(base + packed_offset(m->cfg, i) + packed_fp8_weight_bytes(sh.n_pairs, sh.K)));
    }
  }
  *out = m;
  return 0;
}

extern "C" int sd_model_destroy(sd_model* m) {
  delete m;
  return 0;
}

extern "C" int sd_model_pass_tokens(const sd_model* m) { return m ? m->max_t : 0; }

extern "C" size_t sd_model_workspace_bytes(const sd_model* m) { return m ? workspace_bytes(m->cfg) : 0; }

extern "C" size_t sd_model_kv_bytes(const sd_model* m, int B, int Lmax) {
  if (!m || B <= 0 || Lmax <= 0) return 0;
  return static_cast<size_t>(m->cfg.n_layers) * B * m->cfg.n_kv_heads * Lmax * m->cfg.head_dim * 2;
}

static int carve_workspace(sd_model* m, void* workspace);

extern "C" int sd_model_bind(sd_model* m, void* k_cache, void* v_cache, int B, int Lmax, void* workspace,
                             size_t workspace_bytes_) {
  clear_error();
  SD_REQUIRE(m && k_cache && v_cache && workspace, "model_bind: NULL argument");
  SD_REQUIRE(B >= 1 && Lmax >= 1, "model_bind: B=%d Lmax=%d", B, Lmax);
  SD_REQUIRE(workspace_bytes_ >= workspace_bytes(m->cfg), "model_bind: workspace too small");
  SD_REQUIRE((reinterpret_cast<uintptr_t>(k_cache) & 15) == 0 && (reinterpret_cast<uintptr_t>(v_cache) & 15) == 0,
             "model_bind: caches must be 16-byte aligned");
  m->k_cache = static_cast<uint16_t*>(k_cache);
  m->v_cache = static_cast<uint16_t*>(v_cache);
  m->B = B;
  m->Lmax = Lmax;
  m->block_table = nullptr;
  m->page_shift = m->max_pages = m->n_pages = 0;
  m->prefill_backend = SD_PREFILL_AUTO;
  m->prefill_mc = 0;
  for (int64_t& n : m->prefill_count) n = 0;
  return carve_workspace(m, workspace);
}

extern "C" size_t sd_model_kv_pool_bytes(const sd_model* m, int n_pages, int page_len) {
  if (!m || n_pages <= 0 || page_len <= 0) return 0;
  return static_cast<size_t>(m->cfg.n_layers) * n_pages * m->cfg.n_kv_heads * page_len * m->cfg.head_dim * 2;
}

// Paged KV: rows do not own Lmax positions each; they own pages of page_len positions out of a pool shared by all
// rows, through a caller-maintained table (the counterpart of the reference's cache manager growing / realigning
// per-sequence tensors, kv_cache_manager.py:194-199, :353-479 — here a row grows by a table entry).
extern "C" int sd_model_bind_paged(sd_model* m, void* k_pool, void* v_pool, int n_pages, int page_len, const int32_t* block_table,
                                   int max_pages_per_row, int B, void* workspace, size_t workspace_bytes_) {
  clear_error();
  SD_REQUIRE(m && k_pool && v_pool && block_table && workspace, "model_bind_paged: NULL argument");
  SD_REQUIRE(B >= 1 && n_pages >= 1 && max_pages_per_row >= 1, "model_bind_paged: B=%d pages=%d max_pages=%d", B, n_pages, max_pages_per_row);
  int shift = 0;
  while ((1 << shift) < page_len) ++shift;
  SD_REQUIRE((1 << shift) == page_len && page_len >= 32 && page_len <= 65536, "model_bind_paged: page_len %d must be a power of two >= 32", page_len);
  SD_REQUIRE(workspace_bytes_ >= workspace_bytes(m->cfg), "model_bind_paged: workspace too small");
  SD_REQUIRE((reinterpret_cast<uintptr_t>(k_pool) & 15) == 0 && (reinterpret_cast<uintptr_t>(v_pool) & 15) == 0,
             "model_bind_paged: pools must be 16-byte aligned");
  m->k_cache = static_cast<uint16_t*>(k_pool);
  m->v_cache = static_cast<uint16_t*>(v_pool);
  m->B = B;
  m->Lmax = max_pages_per_row * page_len;
  m->block_table = block_table;
  m->page_shift = shift;
  m->max_pages = max_pages_per_row;
  m->n_pages = n_pages;
  m->prefill_backend = SD_PREFILL_AUTO;
  m->prefill_mc = 0;
  for (int64_t& n : m->prefill_count) n = 0;
  return carve_workspace(m, workspace);
}

// ---- KV shared between cache rows (csrc/kv_fork.hip) -----------------------------------------------------------------
// Both entries check the arguments that need no model first, then the model, then the indices against its geometry:
// nothing is enqueued unless every check passed.
extern "C" int sd_model_kv_fork(sd_model* m, int src_row, const int32_t* dst_rows, int n_dst, int n_pos, void* stream) {
  clear_error();
  SD_REQUIRE(n_dst >= 0, "kv_fork: n_dst=%d", n_dst);
  SD_REQUIRE(n_dst == 0 || dst_rows, "kv_fork: NULL dst_rows with n_dst=%d", n_dst);
  SD_REQUIRE(n_pos >= 0, "kv_fork: n_pos=%d is negative", n_pos);
  SD_REQUIRE(src_row >= 0, "kv_fork: src_row %d is negative", src_row);
  for (int i = 0; i < n_dst; ++i) {
    SD_REQUIRE(dst_rows[i] >= 0, "kv_fork: destination row %d is negative", dst_rows[i]);
    SD_REQUIRE(dst_rows[i] != src_row, "kv_fork: destination row %d is the source row", dst_rows[i]);
  }
  SD_REQUIRE(m, "kv_fork: NULL model");
  SD_REQUIRE(m->k_cache && m->x, "kv_fork: model not bound (sd_model_bind)");
  SD_REQUIRE(!m->block_table, "kv_fork: this model is bound to a paged cache (rows share pages: sd_model_kv_copy_pages)");
  SD_REQUIRE(src_row < m->B, "kv_fork: src_row %d outside the bound batch of %d", src_row, m->B);
  SD_REQUIRE(n_pos <= m->Lmax, "kv_fork: n_pos=%d exceeds Lmax=%d", n_pos, m->Lmax);
  std::vector<char> seen(static_cast<size_t>(m->B), 0);
  for (int i = 0; i < n_dst; ++i) {
    SD_REQUIRE(dst_rows[i] < m->B, "kv_fork: destination row %d outside the bound batch of %d", dst_rows[i], m->B);
    SD_REQUIRE(!seen[dst_rows[i]], "kv_fork: destination row %d is listed twice", dst_rows[i]);
    seen[dst_rows[i]] = 1;
  }
  if (n_dst == 0 || n_pos == 0) return 0;
  const sd_model_config& c = m->cfg;
  return launch_kv_fork(m->k_cache, m->v_cache, c.n_layers, m->B, c.n_kv_heads, m->Lmax, c.head_dim, &src_row, dst_rows, 1, n_dst,
                        n_pos, static_cast<hipStream_t>(stream));
}

extern "C" int sd_model_kv_copy_pages(sd_model* m, const int32_t* src_pages, const int32_t* dst_pages, int n_pairs, int n_pos,
                                      void* stream) {
  clear_error();
  SD_REQUIRE(n_pairs >= 0, "kv_copy_pages: n_pairs=%d", n_pairs);
  SD_REQUIRE(n_pairs == 0 || (src_pages && dst_pages), "kv_copy_pages: NULL page list with n_pairs=%d", n_pairs);
  SD_REQUIRE(n_pos >= 0, "kv_copy_pages: n_pos=%d is negative", n_pos);
  for (int i = 0; i < n_pairs; ++i) {
    SD_REQUIRE(src_pages[i] >= 0 && dst_pages[i] >= 0, "kv_copy_pages: pair %d (%d -> %d) has a negative page index", i, src_pages[i],
               dst_pages[i]);
    SD_REQUIRE(src_pages[i] != dst_pages[i], "kv_copy_pages: pair %d copies page %d onto itself", i, src_pages[i]);
  }
  SD_REQUIRE(m, "kv_copy_pages: NULL model");
  SD_REQUIRE(m->k_cache && m->x, "kv_copy_pages: model not bound (sd_model_bind_paged)");
  SD_REQUIRE(m->block_table, "kv_copy_pages: this model is bound to a dense cache (sd_model_kv_fork)");
  const int page_len = 1 << m->page_shift;
  SD_REQUIRE(n_pos <= page_len, "kv_copy_pages: n_pos=%d exceeds page_len=%d", n_pos, page_len);
  // the pairs of a call run concurrently: a destination must not be a source or another pair's destination
  std::vector<char> role(static_cast<size_t>(m->n_pages), 0);   // 1 = source, 2 = destination
  for (int i = 0; i < n_pairs; ++i) {
    SD_REQUIRE(src_pages[i] < m->n_pages && dst_pages[i] < m->n_pages, "kv_copy_pages: pair %d (%d -> %d) outside the pool of %d pages", i,
               src_pages[i], dst_pages[i], m->n_pages);
    role[src_pages[i]] |= 1;
  }
  for (int i = 0; i < n_pairs; ++i) {
    SD_REQUIRE(role[dst_pages[i]] == 0, "kv_copy_pages: destination page %d is %s", dst_pages[i],
               (role[dst_pages[i]] & 2) ? "listed twice" : "also a source of this call");
    role[dst_pages[i]] |= 2;
  }
  if (n_pairs == 0 || n_pos == 0) return 0;
  const sd_model_config& c = m->cfg;
  return launch_kv_fork(m->k_cache, m->v_cache, c.n_layers, m->n_pages, c.n_kv_heads, page_len, c.head_dim, src_pages, dst_pages, n_pairs,
                        1, n_pos, static_cast<hipStream_t>(stream));
}

static int carve_workspace(sd_model* m, void* workspace) {
  const sd_model_config& c = m->cfg;
  const size_t T = kSkinnyMaxT;
  char* p = reinterpret_cast<char*>(align_up(reinterpret_cast<uintptr_t>(workspace), 256));
  m->x = reinterpret_cast<uint16_t*>(p);
  p += align_up(T * c.d_model * 2, 256);
  m->q = reinterpret_cast<uint16_t*>(p);
  p += align_up(T * c.n_heads * c.head_dim * 2, 256);
  m->attn = reinterpret_cast<uint16_t*>(p);
  p += align_up(T * c.n_heads * c.head_dim * 2, 256);
  m->act = reinterpret_cast<uint16_t*>(p);
  p += align_up(T * c.d_ff * 2, 256);
  m->part_val = reinterpret_cast<float*>(p);
  p += align_up(T * kMaxPartials * 4, 256);
  m->part_idx = reinterpret_cast<int*>(p);
  p += align_up(T * kMaxPartials * 4, 256);
  m->attn_ws = reinterpret_cast<float*>(p);
  m->attn_cnt = reinterpret_cast<unsigned*>(p + static_cast<size_t>(kAttnSplitSlots) * 16 * (c.head_dim + 2) * sizeof(float));
  p += align_up(attention_split_ws_bytes(c.head_dim), 256);
  m->xstat = reinterpret_cast<float*>(p);
  p += align_up(sizeof(float) * 2 * kStatPlane, 256);
  SD_HIP_CHECK(hipMemset(m->attn_cnt, 0, kAttnSplitSlots * sizeof(unsigned)));
  m->probe_pos = reinterpret_cast<int32_t*>(m->attn_cnt);   // a zero word (the counters rest at zero between launches)
  // ---- persistent forward: sync words, op table, granule buffers (all zero: tag 0 is never a valid tag)
  {
    char* pp = p;
    const size_t pbytes = persist_workspace_bytes(c);
    SD_HIP_CHECK(hipMemset(pp, 0, pbytes));
    m->p_sync = reinterpret_cast<unsigned*>(pp);
    pp += 256;
    m->p_ops = reinterpret_cast<PersistOp*>(pp);
    pp += align_up(static_cast<size_t>(4 * c.n_layers + 1) * sizeof(PersistOp), 256);
    m->p_gran = reinterpret_cast<unsigned long long*>(pp);
    m->p_gran_parity = static_cast<unsigned>((pbytes - 256 - align_up(static_cast<size_t>(4 * c.n_layers + 1) * sizeof(PersistOp), 256)) / 16);
    m->persist_t = 0;
    m->persist_cap = 0;
    m->len_hint = m->Lmax;
    if (!m->host_status) SD_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&m->host_status), 64, hipHostMallocDefault));
    *m->host_status = 0u;
    int dev = 0;
    hipDeviceProp_t prop{};
    SD_HIP_CHECK(hipGetDevice(&dev));
    SD_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    if (persist_model_ok(c, m->is_packed() != 0, m->w8() != 0, prop.multiProcessorCount)) {
      std::vector<PersistOp> ops;
      for (int i = 0; i <= 4 * c.n_layers; ++i) {
        const int which = matrix_which(c, i);   // = PersistKind
        const MatShape sh = matrix_shape(c, which);
        const GemvGeom q = gemv_geometry(sh.n_pairs, sh.K);
        PersistOp o{};
        o.W = m->packed[i];
        o.norm_w = matrix_weights(c, i).norm_w;
        o.pair_bytes = static_cast<unsigned>(4 * sh.K);
        o.n_pairs = sh.n_pairs;
        o.ppw = q.ppw;
        o.tile_pairs = q.tile_pairs;
        o.K = sh.K;
        o.kind = which;
        o.layer = i >> 2;
        ops.push_back(o);
      }
      SD_HIP_CHECK(hipMemcpy(m->p_ops, ops.data(), ops.size() * sizeof(PersistOp), hipMemcpyHostToDevice));
      // (a cache whose rows are not whole 8-key vectors cannot be walked by the launch's attention: launch path)
      m->persist_cap = persist_cache_ok(m->Lmax) ? persist_max_tokens(c) : 0;
      // tokens per pass the persistent launch takes (0 = off), by measurement (same box, 128 cached positions, us per forward,
      // persistent / launches; profiles/round3_persist_ab.md): Llama-3.2-1B dimensions 1 token 596 / 698, 2 tokens 677 / 718,
      // 3 tokens 838 / 741; Llama-3.2-3B dimensions 1 token 1506 / 1495, 2 tokens 1640 / 1540. So: 2 tokens up to
      // d_model = 2048 (the draft), off above it (the target's passes stay on launches).
      // And by context (kPersistMaxCtx): by the rows' CURRENT lengths as the caller bounds them (sd_model_set_length_hint; the
      // default bound is the cache size: sessions that size the cache to prompt + budget need not say anything).
      const char* env = getenv(debug_env::kPersistMaxT);
      const int want = env ? atoi(env) : (c.d_model <= 2048 ? 2 : 0);
      m->persist_t = m->persist_cap < want ? m->persist_cap : want;
      m->ctx_limit = env ? m->Lmax : kPersistMaxCtx;   // (the measurement override also lifts the context bound)
    }
  }
  return 0;
}

extern "C" int sd_model_set_persist_tokens(sd_model* m, int max_tokens) {
  clear_error();
  SD_REQUIRE(m && m->x, "set_persist_tokens: NULL argument / model not bound");
  SD_REQUIRE(max_tokens >= 0, "set_persist_tokens: max_tokens=%d", max_tokens);
  m->persist_t = max_tokens < m->persist_cap ? max_tokens : m->persist_cap;
  return 0;
}

extern "C" int sd_model_set_length_hint(sd_model* m, int max_len) {
  clear_error();
  SD_REQUIRE(m && m->x, "set_length_hint: NULL argument / model not bound");
  m->len_hint = (max_len <= 0 || max_len > m->Lmax) ? m->Lmax : max_len;
  return 0;
}

extern "C" int sd_prefill_backend_available(int backend) {
  if (backend == SD_PREFILL_ROCBLAS) return prefill_gemm_library_present() ? 1 : 0;
  return (backend == SD_PREFILL_AUTO || backend == SD_PREFILL_PASSES || backend == SD_PREFILL_NATIVE) ? 1 : 0;
}

extern "C" int sd_model_set_prefill_backend(sd_model* m, int backend) {
  clear_error();
  SD_REQUIRE(m, "set_prefill_backend: NULL model");
  SD_REQUIRE(backend >= SD_PREFILL_AUTO && backend <= SD_PREFILL_NATIVE, "set_prefill_backend: unknown backend %d", backend);
  const bool gpt2 = m->cfg.arch == SD_ARCH_GPT2;
  if (backend == SD_PREFILL_ROCBLAS) {
    SD_REQUIRE(!gpt2, "set_prefill_backend: rocBLAS prefill serves Llama models only (this model is GPT-2)");
    SD_REQUIRE(!m->w8() && m->cfg.weight_dtype == SD_BF16,
               "set_prefill_backend: rocBLAS prefill multiplies the bf16 HF-layout weights, not this model's fp8 storage");
    SD_REQUIRE(!m->block_table, "set_prefill_backend: rocBLAS prefill serves dense KV only (this model is bound to a paged cache)");
    SD_REQUIRE(prefill_gemm_available(), "set_prefill_backend: rocBLAS could not be opened");
  } else if (backend == SD_PREFILL_NATIVE) {
    const char* why = prefill_native_refusal(m->cfg, m->is_packed() != 0);
    SD_REQUIRE(!why, "set_prefill_backend: %s", why);
  }
  m->prefill_backend = backend;
  return 0;
}

extern "C" int sd_model_prefill_backend(const sd_model* m) { return m ? m->prefill_backend : -1; }

extern "C" int64_t sd_model_prefill_count(const sd_model* m, int backend) {
  if (!m || backend < SD_PREFILL_PASSES || backend > SD_PREFILL_NATIVE) return -1;
  return m->prefill_count[backend];
}

extern "C" int sd_model_persist_active(const sd_model* m, int T) {
  // 1 when a pass of T tokens of one row would run as the persistent launch right now (tokens, length hint, paging)
  return (m && T >= 1 && sd::persist_pass_ok(m, T, 1, T)) ? 1 : 0;
}

extern "C" const uint32_t* sd_model_status_word(const sd_model* m) { return m ? m->host_status : nullptr; }

extern "C" int sd_model_engine_status_clear(sd_model* m, void* stream) {
  clear_error();
  SD_REQUIRE(m, "engine_status_clear: NULL argument");
  if (!m->p_sync) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  SD_HIP_CHECK(hipStreamSynchronize(st));   // every workgroup of a failed launch has left
  unsigned w[2] = {0u, 0u};
  SD_HIP_CHECK(hipMemcpy(w, m->p_sync, 8, hipMemcpyDeviceToHost));
  // past the failed launch's tags (it did not advance the counter): granules it left behind can never match again
  w[0] = (w[0] + 2u) & 0x7fffffu;
  w[1] = 0u;
  SD_HIP_CHECK(hipMemcpy(m->p_sync, w, 8, hipMemcpyHostToDevice));
  if (m->host_status) *m->host_status = 0u;
  return 0;
}

extern "C" int sd_model_forward(sd_model* m, const int32_t* tokens, int tok_stride, const int32_t* pos_base,
                                int pos_off, int row0, int B, int M, int32_t* ids_out, int ids_stride, void* logits_out,
                                int logits_dtype, int skip_head, void* stream) {
  clear_error();
  return model_forward(m, tokens, tok_stride, pos_base, pos_off, row0, B, M, ids_out, ids_stride, logits_out,
                       logits_dtype, skip_head, static_cast<hipStream_t>(stream));
}

extern "C" int sd_model_score(sd_model* m, const int32_t* tokens, int n, int row, int pos0, float* logprob, int32_t* greedy, void* stream) {
  clear_error();
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = score_checks(m, tokens, n, 2, row, pos0, st)) return rc;
  return model_score(m, tokens, n, row, pos0, logprob, greedy, nullptr, st);
}

extern "C" int sd_model_score_logits(sd_model* m, const int32_t* tokens, int n, int row, int pos0, void* logits_bf16, int32_t* greedy,
                                     void* stream) {
  clear_error();
  SD_REQUIRE(logits_bf16, "score_logits: NULL logits");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = score_checks(m, tokens, n, 1, row, pos0, st)) return rc;
  return model_score(m, tokens, n, row, pos0, nullptr, greedy, static_cast<uint16_t*>(logits_bf16), st);
}

extern "C" int sd_model_hidden_rows(sd_model* m, int row0, int n, void* out, void* stream) {
  clear_error();
  SD_REQUIRE(m && m->x && out, "hidden_rows: NULL argument / model not bound");
  SD_REQUIRE(row0 >= 0 && n >= 1 && row0 + n <= kSkinnyMaxT, "hidden_rows: rows [%d,%d) outside the %d rows of a pass", row0, row0 + n, kSkinnyMaxT);
  const size_t d = static_cast<size_t>(m->cfg.d_model);
  SD_HIP_CHECK(hipMemcpyAsync(out, m->x + static_cast<size_t>(row0) * d, static_cast<size_t>(n) * d * 2, hipMemcpyDeviceToDevice,
                              static_cast<hipStream_t>(stream)));
  return 0;
}

// Measurement hook (bench.py "roofline" leg): one GEMV of the forward, launched `iters`
// times round-robin over the layers (so the weights come from HBM, not from the 256 MiB
// Infinity Cache) between two HIP events on `stream`.
extern "C" int sd_model_probe_gemv(sd_model* m, int which, int T, int iters, void* stream, float* avg_usec,
                                   double* bytes_per_launch) {
  clear_error();
  SD_REQUIRE(m && m->x && avg_usec && bytes_per_launch, "probe_gemv: NULL argument / model not bound");
  SD_REQUIRE(T >= 1 && T <= kSkinnyMaxT && iters >= 1, "probe_gemv: T=%d iters=%d", T, iters);
  SD_REQUIRE(which >= 0 && which <= 4, "probe_gemv: which=%d (0=qkv 1=o_proj 2=gate_up 3=down 4=lm_head)", which);
  SD_REQUIRE(which != 0 || !m->block_table, "probe_gemv: the QKV probe writes dense cache rows (not available on a paged model)");
  const sd_model_config& c = m->cfg;
  const MatShape sh = matrix_shape(c, which);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipEvent_t e0, e1;
  SD_HIP_CHECK(hipEventCreate(&e0));
  SD_HIP_CHECK(hipEventCreate(&e1));
  unsigned long long* dbg = nullptr;
  const bool timeline = getenv(debug_env::kGemvTimeline) != nullptr;
  if (timeline) {
    SD_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dbg), 256 * 16 * sizeof(unsigned long long)));
    SD_HIP_CHECK(hipMemset(dbg, 0, 256 * 16 * sizeof(unsigned long long)));
  }
  // SPECDEC_PROBE_HOT=n: cycle over n layers only (n=1: the same matrix every launch, i.e. cache-resident weights)
  const int hot = getenv(debug_env::kProbeHot) ? atoi(getenv(debug_env::kProbeHot)) : 0;
  // > 9 tokens: as in the forward, the norm-fused launches read the row statistics the previous launch left, and the
  // residual launches leave them (SPECDEC_PROBE_NO_XSTAT=1: every launch computes its own, as for the first layer)
  const bool use_xstat = T > kGemvMaxT && T <= 64 && !getenv(debug_env::kProbeNoXstat);
  auto launch = [&](int l) -> int {
    if (hot > 0) l %= hot;
    const int li = l % c.n_layers;
    GemvArgs g = matrix_args(m, which == 4 ? 4 * c.n_layers : 4 * li + which);
    g.debug_ts = dbg;
    g.T = T;
    g.M = T;
    g.norm_eps = c.norm_eps;
    if (use_xstat && g.prologue != PRO_NONE) { g.xstat_in = m->xstat; g.xstat_n = 256; }
    if (which == 0) {  // QKV: + RoPE + in-place KV append (row 0 of the cache, positions 0..T-1)
      const int Hkv = c.n_kv_heads, D = c.head_dim;
      g.head_dim = D; g.n_q_heads = c.n_heads; g.n_kv_heads = Hkv; g.max_pos = c.max_pos; g.l_max = m->Lmax;
      g.rope_cos = c.arch == SD_ARCH_LLAMA ? c.rope_cos : nullptr; g.rope_sin = c.arch == SD_ARCH_LLAMA ? c.rope_sin : nullptr;
      g.pos_base = m->probe_pos; g.pos_off = 0;
      const size_t layer_kv = static_cast<size_t>(m->B) * Hkv * m->Lmax * D;
      g.k_cache = m->k_cache + li * layer_kv; g.v_cache = m->v_cache + li * layer_kv;
    }
    if (use_xstat && sh.epi == EPI_RESID && gemm_resid_publishes_stats(g)) g.xstat_out = m->xstat;
    return launch_gemv(g, sh.epi, st);
  };
  double bytes = 2.0 * sh.N * sh.K;
  if (m->w8()) bytes *= 0.5;  // one byte per weight
  for (int i = 0; i < 3; ++i)
    if (int rc = launch(i)) return rc;
  SD_HIP_CHECK(hipEventRecord(e0, st));
  for (int i = 0; i < iters; ++i)
    if (int rc = launch(i + 3)) return rc;
  SD_HIP_CHECK(hipEventRecord(e1, st));
  SD_HIP_CHECK(hipEventSynchronize(e1));
  float ms = 0.f;
  SD_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *avg_usec = ms * 1000.0f / iters;
  *bytes_per_launch = bytes;
  if (timeline) {  // stamps of the LAST launch: offsets from the earliest workgroup entry, in us
    std::vector<unsigned long long> h(256 * 8);
    SD_HIP_CHECK(hipMemcpy(h.data(), dbg, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    (void)hipFree(dbg);
    unsigned long long t0 = ~0ull;
    int n = 0;
    for (int b = 0; b < 256; ++b)
      if (h[b * 8]) { t0 = h[b * 8] < t0 ? h[b * 8] : t0; ++n; }
    static const char* names[8] = {"entry", "issued", "staged", "mfma_done", "reduced", "epilogue", "end", "(stats)"};  // gemm_pipe: issued = first loads issued, (stats) = statistics done, staged = chunk 0
    fprintf(stderr, "[timeline which=%d T=%d] %d workgroups, us from first entry (min / mean / max):\n", which, T, n);
    for (int s = 0; s < 8; ++s) {
      double mn = 1e30, mx = 0, sum = 0;
      for (int b = 0; b < 256; ++b) {
        if (!h[b * 8]) continue;
        const double v = (h[b * 8 + s] - t0) / 100.0;
        mn = v < mn ? v : mn; mx = v > mx ? v : mx; sum += v;
      }
      fprintf(stderr, "  %-10s %7.2f %7.2f %7.2f\n", names[s], mn, sum / (n ? n : 1), mx);
    }
    if (getenv(debug_env::kGemvTimeline)[0] == '2') {   // per-workgroup: when its K loop and the workgroup itself were done
      for (int s : {3, 6}) {
        fprintf(stderr, "[timeline-wg which=%d T=%d %s]", which, T, names[s]);
        for (int b = 0; b < 256; ++b) fprintf(stderr, " %.2f", h[b * 8] ? (h[b * 8 + s] - t0) / 100.0 : -1.0);
        fprintf(stderr, "\n");
      }
    }
  }
  return 0;
}

extern "C" int sd_model_persist_tokens(const sd_model* m) { return m ? m->persist_t : 0; }

extern "C" int sd_model_engine_status(sd_model* m, uint32_t* status_out, void* stream) {
  clear_error();
  SD_REQUIRE(m && status_out, "engine_status: NULL argument");
  *status_out = 0;
  if (!m->p_sync) return 0;
  SD_HIP_CHECK(hipMemcpyAsync(status_out, m->p_sync + 1, 4, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
  SD_HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int sd_model_debug_rows(sd_model* m, int which, int row0, int n, void* out, void* stream) {
  clear_error();
  SD_REQUIRE(m && m->x && out, "debug_rows: NULL argument / model not bound");
  SD_REQUIRE(row0 >= 0 && n >= 1 && row0 + n <= kSkinnyMaxT, "debug_rows: rows [%d,%d) outside the %d rows of a pass", row0, row0 + n, kSkinnyMaxT);
  const sd_model_config& c = m->cfg;
  const uint16_t* src = nullptr;
  size_t w = 0;
  switch (which) {
    case 0: src = m->x; w = c.d_model; break;
    case 1: src = m->q; w = static_cast<size_t>(c.n_heads) * c.head_dim; break;
    case 2: src = m->attn; w = static_cast<size_t>(c.n_heads) * c.head_dim; break;
    case 3: src = m->act; w = c.d_ff; break;
    default: SD_REQUIRE(false, "debug_rows: which=%d (0 x, 1 q, 2 attn, 3 act)", which);
  }
  SD_HIP_CHECK(hipMemcpyAsync(out, src + static_cast<size_t>(row0) * w, static_cast<size_t>(n) * w * 2, hipMemcpyDeviceToDevice,
                              static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int sd_model_prefill_rows(sd_model* m, int which, int row0, int n, void* out, void* stream) {
  clear_error();
  SD_REQUIRE(m && out, "prefill_rows: NULL argument");
  SD_REQUIRE(m->prefill_mc > 0, "prefill_rows: no GEMM-prefill chunk on record (the model's last forward was not one, or it was bound since)");
  SD_REQUIRE(row0 >= 0 && n >= 1 && n <= m->prefill_mc && row0 <= m->prefill_mc - n, "prefill_rows: %d rows from row %d are outside the %d rows of the last chunk",
             n, row0, m->prefill_mc);
  const sd_model_config& c = m->cfg;
  const uint16_t* src = nullptr;
  size_t w = 0;
  switch (which) {
    case 0: src = m->prefill_rows.x; w = c.d_model; break;
    case 1: src = m->prefill_rows.q; w = static_cast<size_t>(c.n_heads) * c.head_dim; break;
    case 2: src = m->prefill_rows.attn; w = static_cast<size_t>(c.n_heads) * c.head_dim; break;
    case 3: src = m->prefill_rows.act; w = c.d_ff; break;
    default: SD_REQUIRE(false, "prefill_rows: which=%d (0 x, 1 q, 2 attn, 3 act)", which);
  }
  SD_HIP_CHECK(hipMemcpyAsync(out, src + static_cast<size_t>(row0) * w, static_cast<size_t>(n) * w * 2, hipMemcpyDeviceToDevice,
                              static_cast<hipStream_t>(stream)));
  return 0;
}

// the model the plan queries build from dimensions alone (no weights are read)
static int prefill_plan_config(int arch, int d_model, int n_heads, int n_kv_heads, int head_dim, int d_ff, int which, int T, sd_model_config& c) {
  SD_REQUIRE(which >= 0 && which <= 3, "prefill_plan: which=%d (0 qkv, 1 out, 2 gate / up, 3 down)", which);
  SD_REQUIRE(T >= 1 && T <= kPrefillChunk, "prefill_plan: T=%d (a chunk holds 1 .. %d positions)", T, kPrefillChunk);
  SD_REQUIRE(d_model >= 1 && n_heads >= 1 && n_kv_heads >= 1 && head_dim >= 1 && d_ff >= 1 && d_model <= (1 << 20) && n_heads <= (1 << 12) &&
                 n_kv_heads <= (1 << 12) && head_dim <= (1 << 12) && d_ff <= (1 << 22),
             "prefill_plan: a dimension is below 1 or beyond any model");
  c = sd_model_config{};
  c.arch = arch; c.n_layers = 1; c.d_model = d_model; c.n_heads = n_heads; c.n_kv_heads = n_kv_heads; c.head_dim = head_dim; c.d_ff = d_ff;
  c.vocab = 2;
  return 0;
}

extern "C" int sd_prefill_plan(int arch, int d_model, int n_heads, int n_kv_heads, int head_dim, int d_ff, int which, int T, int w8,
                               int packed, int* eligible, int* row_blocks, int* token_blocks, int* grid, int* swizzled, int* last_rows,
                               int* min_block_rows, int* k_stages, char* name, size_t name_cap, char* reason, size_t reason_cap) {
  clear_error();
  SD_REQUIRE(eligible && row_blocks && token_blocks && grid && swizzled && last_rows && min_block_rows && k_stages && name && reason,
             "prefill_plan: NULL argument");
  sd_model_config c{};
  if (int rc = prefill_plan_config(arch, d_model, n_heads, n_kv_heads, head_dim, d_ff, which, T, c)) return rc;
  const char* refusal = prefill_native_refusal(c, packed != 0);   // the rule sd_model_set_prefill_backend(SD_PREFILL_NATIVE) applies
  PrefillPlanInfo pl{};
  if (!refusal) {
    NativeTables t;
    if (int rc = native_plan_tables(c, t)) return rc;
    pl = native_plan_info(t, c, which, T);
  }
  char nm[32], why[96];
  const int n = refusal ? snprintf(nm, sizeof(nm), "none") : snprintf(nm, sizeof(nm), "mfma<rf%d,%s>", pl.variant == 0 ? 4 : 2, w8 ? "fp8" : "bf16");
  const int r = snprintf(why, sizeof(why), "%s", refusal ? refusal : "");
  SD_REQUIRE(n > 0 && static_cast<size_t>(n) < sizeof(nm) && static_cast<size_t>(n) < name_cap, "prefill_plan: name_cap=%zu is too short for the name (%d bytes with its NUL)", name_cap, n + 1);
  SD_REQUIRE(r >= 0 && static_cast<size_t>(r) < sizeof(why) && static_cast<size_t>(r) < reason_cap, "prefill_plan: reason_cap=%zu is too short for the reason (%d bytes with its NUL)", reason_cap, r + 1);
  memcpy(name, nm, static_cast<size_t>(n) + 1);
  memcpy(reason, why, static_cast<size_t>(r) + 1);
  *eligible = refusal ? 0 : 1;
  *row_blocks = pl.n_blocks;
  *token_blocks = pl.n_tb;
  *grid = pl.grid;
  *swizzled = pl.swizzled;
  *last_rows = pl.last_tb_rows;
  *min_block_rows = refusal ? 0 : pl.min_block_rows;
  *k_stages = pl.k_stages;
  return 0;
}

extern "C" int sd_prefill_plan_tables(int arch, int d_model, int n_heads, int n_kv_heads, int head_dim, int d_ff, int which, int T,
                                      int* blocks, size_t n_blocks, int* wg_block, size_t n_grid) {
  clear_error();
  SD_REQUIRE(blocks && wg_block, "prefill_plan_tables: NULL argument");
  sd_model_config c{};
  if (int rc = prefill_plan_config(arch, d_model, n_heads, n_kv_heads, head_dim, d_ff, which, T, c)) return rc;
  const char* refusal = prefill_native_refusal(c, true);
  SD_REQUIRE(!refusal, "prefill_plan_tables: %s", refusal);
  NativeTables t;
  if (int rc = native_plan_tables(c, t)) return rc;
  const PrefillPlanInfo pl = native_plan_info(t, c, which, T);
  SD_REQUIRE(n_blocks == static_cast<size_t>(pl.n_blocks) && n_grid == static_cast<size_t>(pl.grid),
             "prefill_plan_tables: the plan has %d row blocks and a grid of %d (asked for %zu and %zu)", pl.n_blocks, pl.grid, n_blocks, n_grid);
  for (int b = 0; b < pl.n_blocks; ++b) {
    const int2 blk = t.blocks[pl.first_block + b];
    int rows = 0;
    for (int k = 0; k < blk.y; ++k) rows += 2 * t.tiles[blk.x + k].y;
    blocks[2 * b] = t.tiles[blk.x].z;
    blocks[2 * b + 1] = rows;
  }
  for (int g = 0; g < pl.grid; ++g) wg_block[g] = native_block_of(g, pl.grid);
  return 0;
}

extern "C" int sd_model_matrix_shape(const sd_model* m, int which, int* N, int* K, int* n_pairs, int* epi, int* prologue) {
  clear_error();
  SD_REQUIRE(m && N && K && n_pairs && epi && prologue, "matrix_shape: NULL argument");
  SD_REQUIRE(which >= 0 && which <= 4, "matrix_shape: which=%d (0 qkv, 1 out, 2 gate / up, 3 down, 4 lm_head)", which);
  const MatShape sh = matrix_shape(m->cfg, which);
  *N = sh.N;
  *K = sh.K;
  *n_pairs = sh.n_pairs;
  *epi = sh.epi;
  // as matrix_args: a matrix behind a normalisation (qkv, gate / up, lm_head) takes the architecture's norm as prologue
  const bool normed = matrix_weights(m->cfg, which == 4 ? 4 * m->cfg.n_layers : which).norm_w != nullptr;
  *prologue = !normed ? PRO_NONE : (m->cfg.arch == SD_ARCH_LLAMA ? PRO_RMSNORM : PRO_LAYERNORM);
  return 0;
}

extern "C" int sd_gemm_plan(int T, int n_pairs, int K, int w8, int prologue, int epi, int flags, char* out, size_t cap) {
  clear_error();
  SD_REQUIRE(out, "gemm_plan: NULL out");
  SD_REQUIRE(T >= 1, "gemm_plan: T=%d", T);
  SD_REQUIRE(prologue >= PRO_NONE && prologue <= PRO_LAYERNORM && epi >= EPI_QKV_ROPE && epi <= EPI_ARGMAX && (flags & ~3) == 0,
             "gemm_plan: prologue=%d epi=%d flags=%d out of range", prologue, epi, flags);
  char name[64];
  int n;
  if (T <= kGemvMaxT) n = snprintf(name, sizeof(name), "gemv");
  else n = gemm_plan_name(gemm_plan(T, n_pairs, K, w8 != 0, prologue, epi, flags), epi, w8 != 0, name, sizeof(name));
  SD_REQUIRE(n > 0 && static_cast<size_t>(n) < sizeof(name) && static_cast<size_t>(n) < cap, "gemm_plan: cap=%zu is too short for the name (%d bytes with its NUL)", cap, n + 1);
  memcpy(out, name, static_cast<size_t>(n) + 1);
  return 0;
}

extern "C" int sd_gemv_variant(int T, int n_pairs, int K, int w8, int prologue, int epi, char* out, size_t cap) {
  clear_error();
  SD_REQUIRE(out, "gemv_variant: NULL out");
  SD_REQUIRE(T >= 1 && T <= kGemvMaxT, "gemv_variant: T=%d out of range 1..%d", T, kGemvMaxT);
  SD_REQUIRE(prologue >= PRO_NONE && prologue <= PRO_LAYERNORM && epi >= EPI_QKV_ROPE && epi <= EPI_ARGMAX,
             "gemv_variant: prologue=%d epi=%d out of range", prologue, epi);
  SD_REQUIRE(n_pairs >= 1 && K >= 8 && K % 8 == 0, "gemv_variant: n_pairs=%d K=%d (K must be a multiple of 8)", n_pairs, K);
  char name[64];
  const int n = gemv_variant_name(T, n_pairs, K, w8 != 0, prologue, epi, name, sizeof(name));
  SD_REQUIRE(n > 0 && static_cast<size_t>(n) < sizeof(name) && static_cast<size_t>(n) < cap, "gemv_variant: cap=%zu is too short for the name (%d bytes with its NUL)", cap, n + 1);
  memcpy(out, name, static_cast<size_t>(n) + 1);
  return 0;
}

extern "C" int sd_gemv_instance(int T, int n_pairs, int K, int w8, int prologue, int epi, char* out, size_t cap) {
  clear_error();
  SD_REQUIRE(out, "gemv_instance: NULL out");
  SD_REQUIRE(T >= 1 && T <= kGemvMaxT, "gemv_instance: T=%d out of range 1..%d", T, kGemvMaxT);
  SD_REQUIRE(prologue >= PRO_NONE && prologue <= PRO_LAYERNORM && epi >= EPI_QKV_ROPE && epi <= EPI_ARGMAX,
             "gemv_instance: prologue=%d epi=%d out of range", prologue, epi);
  SD_REQUIRE(n_pairs >= 1 && K >= 8 && K % 8 == 0, "gemv_instance: n_pairs=%d K=%d (K must be a multiple of 8)", n_pairs, K);
  char name[64];
  int n = 0;
  if (int rc = gemv_instance_name(T, n_pairs, K, w8 != 0, prologue, epi, name, sizeof(name), &n)) return rc;   // a launch launch_gemv refuses, in its words
  SD_REQUIRE(n > 0 && static_cast<size_t>(n) < sizeof(name) && static_cast<size_t>(n) < cap, "gemv_instance: cap=%zu is too short for the name (%d bytes with its NUL)", cap, n + 1);
  memcpy(out, name, static_cast<size_t>(n) + 1);
  return 0;
}

extern "C" int sd_persist_plan(int arch, int n_layers, int d_model, int n_heads, int n_kv_heads, int head_dim, int d_ff, int vocab,
                               int packed, int weight_dtype, int has_bias, int T, int* eligible, int* max_tokens, int* ring_bytes,
                               char* name, size_t name_cap, char* reason, size_t reason_cap) {
  clear_error();
  SD_REQUIRE(eligible && max_tokens && ring_bytes && name && reason, "persist_plan: NULL argument");
  SD_REQUIRE(T >= 1, "persist_plan: T=%d", T);
  SD_REQUIRE(weight_dtype == SD_BF16 || weight_dtype == SD_FP8_E4M3, "persist_plan: weight_dtype=%d (SD_BF16 or SD_FP8_E4M3)", weight_dtype);
  SD_REQUIRE(d_model >= 1 && n_heads >= 1 && n_kv_heads >= 1 && head_dim >= 1 && d_ff >= 1 && vocab >= 1 && d_model <= (1 << 20) &&
                 n_heads <= (1 << 12) && n_kv_heads <= (1 << 12) && head_dim <= (1 << 12) && d_ff <= (1 << 22) && vocab <= (1 << 24),
             "persist_plan: a dimension is below 1 or beyond any model");
  sd_model_config c{};
  c.arch = arch; c.n_layers = n_layers; c.d_model = d_model; c.n_heads = n_heads; c.n_kv_heads = n_kv_heads;
  c.head_dim = head_dim; c.d_ff = d_ff; c.vocab = vocab; c.weight_dtype = weight_dtype;
  // (one row of T tokens: a pass of B rows x M tokens stages the attention state of M tokens only and leaves no less)
  const PersistPlan pl = persist_plan(c, packed != 0, weight_dtype != SD_BF16, has_bias != 0, kPersistCUs, T, T);
  char nm[32], why[96];
  int n, r;
  if (pl.refusal) r = snprintf(why, sizeof(why), "%s", pl.refusal);
  else if (!pl.D) r = snprintf(why, sizeof(why), "tokens: T=%d above the %d a pass of this model holds", T, pl.max_tokens);
  else r = snprintf(why, sizeof(why), "%s", "");
  if (pl.D) n = snprintf(nm, sizeof(nm), "persist<%d,%d>", pl.D, pl.HC);
  else n = snprintf(nm, sizeof(nm), "none");
  SD_REQUIRE(n > 0 && static_cast<size_t>(n) < sizeof(nm) && static_cast<size_t>(n) < name_cap, "persist_plan: name_cap=%zu is too short for the name (%d bytes with its NUL)", name_cap, n + 1);
  SD_REQUIRE(r >= 0 && static_cast<size_t>(r) < sizeof(why) && static_cast<size_t>(r) < reason_cap, "persist_plan: reason_cap=%zu is too short for the reason (%d bytes with its NUL)", reason_cap, r + 1);
  memcpy(name, nm, static_cast<size_t>(n) + 1);
  memcpy(reason, why, static_cast<size_t>(r) + 1);
  *eligible = pl.refusal ? 0 : 1;
  *max_tokens = pl.max_tokens;
  *ring_bytes = static_cast<int>(pl.ring_bytes);
  return 0;
}

extern "C" int sd_model_set_persist_taps(sd_model* m, int enable) {
  clear_error();
  SD_REQUIRE(m, "set_persist_taps: NULL model");
  m->persist_taps = enable != 0;
  return 0;
}

extern "C" int sd_model_probe_forward(sd_model* m, int M, int pos0, int iters, int skip_head, void* stream, float* avg_usec,
                                      double* bytes_per_forward, unsigned long long* timeline, size_t timeline_cap) {
  clear_error();
  SD_REQUIRE(m && m->x && avg_usec && bytes_per_forward, "probe_forward: NULL argument / model not bound");
  SD_REQUIRE(M >= 1 && M <= kSkinnyMaxT && iters >= 1, "probe_forward: M=%d iters=%d", M, iters);
  SD_REQUIRE(pos0 >= 0 && pos0 + M <= m->Lmax, "probe_forward: positions [%d, %d) outside the cache rows (%d)", pos0, pos0 + M, m->Lmax);
  SD_REQUIRE(!m->block_table, "probe_forward: dense KV only");
  const sd_model_config& c = m->cfg;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int32_t* zeros = reinterpret_cast<const int32_t*>(m->attn_cnt);   // kAttnSplitSlots zero words: token ids and the position base
  auto fwd = [&]() { return model_forward(m, zeros, M, zeros, pos0, 0, 1, M, nullptr, M, nullptr, SD_BF16, skip_head, st); };
  hipEvent_t e0, e1;
  SD_HIP_CHECK(hipEventCreate(&e0));
  SD_HIP_CHECK(hipEventCreate(&e1));
  for (int i = 0; i < 2; ++i)
    if (int rc = fwd()) return rc;
  SD_HIP_CHECK(hipEventRecord(e0, st));
  for (int i = 0; i < iters; ++i)
    if (int rc = fwd()) return rc;
  SD_HIP_CHECK(hipEventRecord(e1, st));
  SD_HIP_CHECK(hipEventSynchronize(e1));
  float ms = 0.f;
  SD_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *avg_usec = ms * 1000.0f / iters;
  double per_layer = 0;
  for (int i = 0; i < 4; ++i) per_layer += 2.0 * matrix_shape(c, i).N * matrix_shape(c, i).K;
  double bytes = per_layer * c.n_layers + (skip_head ? 0.0 : 2.0 * matrix_shape(c, 4).N * matrix_shape(c, 4).K);
  if (m->w8()) bytes *= 0.5;
  *bytes_per_forward = bytes;
  if (timeline && m->persist_t >= M) {
    const size_t n_ops = static_cast<size_t>(4 * c.n_layers + (skip_head ? 0 : 1));
    const size_t words = static_cast<size_t>(kPersistCUs) * (12 * n_ops + 4);
    SD_REQUIRE(timeline_cap >= words, "probe_forward: timeline needs %zu words", words);
    unsigned long long* dbg = nullptr;
    SD_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dbg), words * 8));
    SD_HIP_CHECK(hipMemsetAsync(dbg, 0, words * 8, st));
    m->p_debug = dbg;
    const int rc = fwd();
    m->p_debug = nullptr;
    if (rc) { (void)hipFree(dbg); return rc; }
    SD_HIP_CHECK(hipStreamSynchronize(st));
    SD_HIP_CHECK(hipMemcpy(timeline, dbg, words * 8, hipMemcpyDeviceToHost));
    (void)hipFree(dbg);
  }
  return 0;
}

// ---------------------------------------------------------------------------- step loop
static constexpr int kStageInts = 24;   // per row: 8 ints of set_row, then (accepted, proposed, hist_n, k) + 4 doubles

struct sd_specdec {
  sd_model* draft = nullptr;
  sd_model* target = nullptr;
  int B = 0, K = 0, mode = 0;
  SpecState st{};
  int32_t* dev_block = nullptr;   // all device state in one allocation
  int32_t* step_counter = nullptr; // device: steps executed (its parity selects the record slot)
  int32_t* host_record = nullptr;  // pinned, device-accessible: [2 slots][B][rec]
  hipEvent_t ev_done[2] = {nullptr, nullptr};   // recorded after launch i on the target stream (i & 1)
  long launches = 0;
  int32_t* host_stage = nullptr;  // pinned staging for set_row / set_adaptive_row: [B][kStageInts]
  int a_initial = 0;
  int rec = 0;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  hipStream_t graph_st_t = nullptr, graph_st_d = nullptr;
  long steps = 0;
  // sampled bonus token (sd_specdec_set_sampling); all buffers are caller-owned
  int sample = 0;
  float temperature = 1.0f, top_p = 1.0f;
  int top_k = 0;
  uint64_t seed = 0;
  void* logits = nullptr;          // [B][K+1][V] bf16
  uint32_t* draw = nullptr;        // [B]
  const int32_t* stream_id = nullptr;
  // speculative sampling (sd_specdec_set_spec_sampling): draft tokens drawn from q, accept by p/q, residual redraw. Shares
  // temperature / seed / draw / stream_id with the sampled-bonus mode (the two are mutually exclusive).
  int spec = 0;
  void* spec_q = nullptr;          // [B][K][V] bf16 draft logits, caller-owned
  void* spec_p = nullptr;          // [B][K+1][V] bf16 target logits, caller-owned; until the verify forward overwrites it, its first
                                   // rows are where each draft forward leaves the logits of its pass ([B][M][V])
  int32_t* spec_flags = nullptr;   // [2][B][K+1] device: accept flags, candidate next tokens
  int spec_top_k = 0;              // sd_specdec_set_spec_shaping: > 0 = both distributions shaped by top-k / top-p
  float spec_top_p = 1.0f;
  // logit processors (sd_specdec_set_logit_processors): every logits row is stored, processed in place, then consumed
  int lp = 0;
  float lp_rp = 1.0f, lp_presence = 0.f, lp_frequency = 0.f;
  uint16_t* lp_counts = nullptr;   // [B][V], caller-owned
  const float* lp_bias = nullptr;  // [B][V] or null, caller-owned
  void* lp_logits = nullptr;       // [B][K+1][V] bf16, caller-owned; used while neither sampling mode owns a buffer
  void* lp_ws = nullptr;           // argmax partials of the process launches
  size_t lp_ws_bytes = 0;
  // persistent Medusa heads (sd_specdec_set_medusa): K packed [V][d] matrices + their fp32 row scales (fp8)
  std::vector<const void*> heads;
  std::vector<const float*> head_scales;
  int32_t* head_rows = nullptr;    // [B] device: row of the target's residual stream each head reads
  size_t head_stride = 0;          // bytes between consecutive heads when they sit at a constant stride (one launch), else 0
  // EAGLE-lite (sd_specdec_set_eagle): extrapolated hidden rows instead of a draft model; caller-owned workspace
  bool draft_taps = false;         // the draft's persistent passes also store their stage rows (debug)
  bool want_fwd0_select = false;   // device-selected form of draft forward 0 (storage carved at create; eligibility per capture)
  int eagle = 0;
  float eagle_alpha = 0.7f;
  uint16_t* eagle_H = nullptr;     // [B*K][d]
  uint16_t* eagle_prev = nullptr;  // [B][d] last extrapolated row of the previous step
  int32_t* eagle_has = nullptr;    // [B]
};

namespace sd {

// Argmax of n_heads vocabulary-sized matrices over T activation rows: what the Medusa step, the EAGLE step and
// sd_model_head_argmax all run. The matrices have the lm_head's shape (and, unless `prenormed`, its final norm in front);
// id of (matrix j, row t) -> ids[(t / M) * ids_stride + t % M + j].
struct HeadEval {
  const void* x = nullptr;          // bf16 rows of d_model elements (stride d_model)
  const int32_t* x_row = nullptr;   // nullable, device [T]: row t reads row x_row[t] of x
  int T = 0, M = 1;                 // rows, rows per batch row (the id layout; M == 1 whenever n_heads > 1)
  int n_heads = 0;
  const void* const* W = nullptr;          // [n_heads]
  const float* const* scale = nullptr;     // [n_heads] fp32 row scales (w8), else null
  size_t stride = 0;                // bytes between consecutive matrices when constant (one launch), else 0 (one launch each)
  int packed = 1, w8 = 0;
  bool prenormed = false;           // the rows are final-norm outputs already: PRO_NONE, no norm weights
  int32_t* ids = nullptr;
  int ids_stride = 0;
  float* vals = nullptr;            // nullable: the fp32 value attached to each winning index, laid out as ids (debug entry only)
  int* launch_info = nullptr;       // nullable, host [2]: matrix launches enqueued, 1 if the rows were gathered first (debug entry only)
};

// Matrices at a constant stride are evaluated by ONE lm_head-shaped launch (grid y = matrix: same x rows, same geometry,
// per-matrix argmax partials) and one finalize over n_heads x T results; otherwise one launch + finalize per matrix.
static int enqueue_head_argmax(sd_model* m, const HeadEval& e, hipStream_t st) {
  const sd_model_config& c = m->cfg;
  const int T = e.T, nh = e.n_heads;
  GemvArgs h = matrix_args(m, 4 * c.n_layers);   // the lm_head's shape and final norm; the matrices' own weights below
  h.packed = e.packed;
  h.w8 = e.w8;
  h.x = e.x;
  h.x_row = e.x_row;
  h.T = T;
  h.M = e.M;
  if (e.prenormed) {
    h.prologue = PRO_NONE;
    h.norm_w = h.norm_b = nullptr;
    h.norm_eps = 0.f;
  }
  if (e.x_row && T > m->small_t) {   // more rows than a GEMV pass: gather them (the attention-output buffer is free after the verify forward)
    if (int rc = launch_medusa_gather(e.x, e.x_row, m->attn, T, c.d_model, st)) return rc;
    h.x = m->attn;
    h.x_row = nullptr;
    if (e.launch_info) e.launch_info[1] = 1;
  }
  int ppw = 1;
  const int grid = gemv_grid(h, &ppw);
  if (nh >= 2 && T <= m->small_t && e.stride && e.M == 1 &&
      static_cast<size_t>(nh) * T * grid <= static_cast<size_t>(kSkinnyMaxT) * kMaxPartials) {
    h.W = e.W[0];
    h.w_scale = e.scale ? e.scale[0] : nullptr;
    h.batch_bytes = e.stride;
    h.n_batch = nh;
    if (int rc = launch_gemv(h, EPI_ARGMAX, st)) return rc;
    if (e.launch_info) e.launch_info[0] = 1;
    // result (matrix j, row t) = "token" j * T + t of the partials -> ids[t][j]
    if (int rc = launch_argmax_finalize(m->part_val, m->part_idx, nh * T, grid, -T, e.ids_stride, e.ids, st)) return rc;
    if (e.vals)
      if (int rc = launch_argmax_value(m->part_val, m->part_idx, nh * T, grid, -T, e.ids_stride, e.vals, st)) return rc;
    return 0;
  }
  for (int i = 0; i < nh; ++i) {
    h.w_scale = e.scale ? e.scale[i] : nullptr;
    h.W = e.W[i];
    if (int rc = launch_gemv(h, EPI_ARGMAX, st)) return rc;
    if (e.launch_info) e.launch_info[0] += 1;
    if (int rc = launch_argmax_finalize(m->part_val, m->part_idx, T, grid, e.M, e.ids_stride, e.ids + i, st)) return rc;
    if (e.vals)
      if (int rc = launch_argmax_value(m->part_val, m->part_idx, T, grid, e.M, e.ids_stride, e.vals + i, st)) return rc;
  }
  return 0;
}

// draft tokens of the NEXT step from the heads: d_{i+1} = argmax head_i(final_norm(h)), h = the residual row of the
// position that produced the last emitted token -> verify_tok[b][i + 1] (enqueue_head_argmax).
static int enqueue_medusa_heads(sd_specdec* s, hipStream_t st) {
  sd_model* m = s->target;
  if (int rc = launch_medusa_rows(s->st, s->head_rows, st)) return rc;
  HeadEval e;
  e.x = m->x;
  e.x_row = s->head_rows;
  e.T = s->B;
  e.n_heads = s->K;
  e.W = s->heads.data();
  e.scale = s->head_scales.empty() ? nullptr : s->head_scales.data();
  e.stride = s->head_stride;
  e.w8 = s->head_scales.empty() ? 0 : 1;
  e.ids = s->st.verify_tok + 1;
  e.ids_stride = s->K + 1;
  if (int rc = enqueue_head_argmax(m, e, st)) return rc;
  return launch_medusa_commit(s->st, st);
}

static int enqueue_step(sd_specdec* s, hipStream_t st_t, hipStream_t st_d) {
  const int B = s->B, K = s->K;
  const bool two = (st_d != st_t) && s->draft;
  if (!s->draft && s->eagle) {
    // EAGLE-lite: residual row of `last` (1-token forward, head skipped) -> K extrapolated rows -> one lm_head launch
    sd_model* m = s->target;
    const sd_model_config& c = m->cfg;
    if (int rc = model_forward(m, s->st.verify_tok, K + 1, s->st.cur_len, 0, 0, B, 1, nullptr, 2, nullptr, SD_BF16, 1, st_t)) return rc;
    if (int rc = launch_eagle_extrapolate(m->x, s->eagle_H, s->eagle_prev, s->eagle_has, c.final_norm_w, c.final_norm_b, c.norm_eps,
                                          s->eagle_alpha, c.d_model, B, K, c.arch == SD_ARCH_LLAMA ? 1 : 0, st_t))
      return rc;
    const void* const w_head = m->mat(4 * c.n_layers, c.lm_head);
    const float* const sc_head = m->scale(4 * c.n_layers);
    HeadEval e;
    e.x = s->eagle_H;
    e.T = B * K;
    e.M = K;
    e.n_heads = 1;
    e.W = &w_head;
    e.scale = sc_head ? &sc_head : nullptr;
    e.packed = m->is_packed();
    e.w8 = m->w8();
    e.prenormed = true;        // the rows are final-norm outputs already
    e.ids = s->st.verify_tok + 1;
    e.ids_stride = K + 1;
    if (int rc = enqueue_head_argmax(m, e, st_t)) return rc;
    if (int rc = launch_medusa_commit(s->st, st_t)) return rc;
  } else if (!s->draft && s->heads.empty()) {
    // self-draft (Medusa-lite, tied heads): the target's own next token, K times
    if (int rc = model_forward(s->target, s->st.verify_tok, K + 1, s->st.cur_len, 0, 0, B, 1, s->st.draft_ids, 2, nullptr, SD_BF16, 0, st_t))
      return rc;
    if (int rc = launch_medusa_fill(s->st, st_t)) return rc;
  }
  if (two) {
    SD_HIP_CHECK(hipEventRecord(s->ev_fork, st_t));
    SD_HIP_CHECK(hipStreamWaitEvent(st_d, s->ev_fork, 0));
  }
  // draft: forward 0 over (prev, last) at positions cur_len-1, cur_len; then one token each
  struct TapsGuard {   // the draft's stage taps are this loop's choice, for the duration of its forwards only
    sd_model* m; bool saved;
    TapsGuard(sd_model* m_, bool v) : m(m_), saved(m_ ? m_->persist_taps : false) { if (m) m->persist_taps = v; }
    ~TapsGuard() { if (m) m->persist_taps = saved; }
  } taps_guard(s->draft, s->draft_taps);
  // both forms of forward 0 with the device picking one: only while the draft's 1- and 2-token passes are persistent launches
  // (a pass that is not needed then costs one launch that returns at entry, not 80) — decided per capture, the model may have
  // been re-bound or its persistent passes switched off since the loop was created
  const bool fwd0_select = s->draft && s->st.fwd0_w && B == 1 && persist_pass_ok(s->draft, 2, 1, 2);
  // a draft forward that is ONE pass leaves the lm_head partials of all its tokens in the model's workspace: ids and the hand-over
  // of d_{i+1} are then one launch (draft_finalize_kernel) instead of two
  const bool one_pass_d = s->draft && B * 2 <= s->draft->max_t;
  const auto finalize = [&](int M, int i, int32_t* ids, const int32_t* skip_k, int skip_i) -> int {
    if (one_pass_d)
      return launch_draft_finalize(s->draft->part_val, s->draft->part_idx, s->draft->head_grid, M, i, ids, s->st, skip_k, skip_i, st_d);
    return 0;
  };
  // speculative sampling: every draft forward stores its logits, d_{i+1} is DRAWN from the last position's row (no argmax ids)
  const bool spec = s->spec != 0;
  const int V = s->target->cfg.vocab;
  // logit processors: the forwards store their rows (into the buffer of the sampling mode that is on, else the mode's own), the
  // rows are processed in place and the argmax of the processed row replaces the fused one
  const bool lp = s->lp != 0;
  void* const p_buf = s->sample ? s->logits : (spec ? s->spec_p : (lp ? s->lp_logits : nullptr));
  SD_REQUIRE(!lp || (s->draft && p_buf), "specdec_step: logit processors need a draft model and a logits buffer (sd_specdec_set_logit_processors)");
  uint16_t* const q_pass = (spec || lp) ? static_cast<uint16_t*>(p_buf) : nullptr;   // (the verify forward overwrites it afterwards)
  int32_t* const ids_d = (one_pass_d || spec || lp) ? nullptr : s->st.draft_ids;
  // draft forward i left the logits of its M positions in q_pass: process row M - 1 of every batch row with d_1..d_i
  const auto process_draft = [&](int M, int i) -> int {
    if (int rc = launch_logit_process(q_pass + static_cast<size_t>(M - 1) * V, static_cast<long long>(M) * V, B, 1, V, s->lp_counts, s->lp_bias,
                                      s->st.draft_tok, K, i, s->st.active, s->lp_rp, s->lp_presence, s->lp_frequency,
                                      spec ? nullptr : s->st.draft_ids + (M - 1), 2, s->lp_ws, s->lp_ws_bytes, st_d))
      return rc;
    return spec ? 0 : launch_draft_next(M, i, s->st, st_d);
  };
  for (int i = 0; s->draft && i < K; ++i) {
    const int M = (i == 0) ? 2 : 1;
    const int32_t* toks = (i == 0) ? s->st.tok2 : s->st.next_tok;
    const int off = (i == 0) ? -1 : i;
    // per-row adaptive K: forward i >= 1 only matters while some row proposes more than i tokens
    s->draft->skip_k = (s->st.adaptive && i >= 1) ? s->st.k_active : nullptr;
    s->draft->skip_i = i;
    int rc_f;
    if (i == 0 && fwd0_select) {
      // both forms of forward 0, the device picks (SpecState::fwd0_w, written by accept_kernel): the 2-token pass, then the
      // 1-token pass over `last` alone, whose id lands where the 2-token pass leaves its second one
      s->draft->skip_k = s->st.fwd0_w;
      s->draft->skip_i = 1;
      rc_f = model_forward(s->draft, toks, 2, s->st.cur_len, -1, 0, B, 2, ids_d, 2, q_pass, SD_BF16, 0, st_d);
      if (!rc_f && !spec && !lp) rc_f = finalize(2, 0, s->st.draft_ids, s->st.fwd0_w, 1);
      if (!rc_f) {
        s->draft->skip_k = s->st.fwd0_w + 1;
        // (the 1-token form's logits row lands where the 2-token form leaves its second one, as its id does)
        rc_f = model_forward(s->draft, toks + 1, 2, s->st.cur_len, 0, 0, B, 1, ids_d ? ids_d + 1 : nullptr, 2, q_pass ? q_pass + V : nullptr,
                             SD_BF16, 0, st_d);
      }
      if (!rc_f && !spec && !lp) rc_f = finalize(1, 0, s->st.draft_ids + 1, s->st.fwd0_w + 1, 1);
    } else {
      rc_f = model_forward(s->draft, toks, M, s->st.cur_len, off, 0, B, M, ids_d, 2, q_pass, SD_BF16, 0, st_d);
      if (!rc_f && !spec && !lp) rc_f = finalize(M, i, s->st.draft_ids, s->draft->skip_k, i);
    }
    s->draft->skip_k = nullptr;
    if (rc_f) return rc_f;
    if (lp)   // (exactly one form of forward 0 ran; both leave the last position's row in the same place)
      if (int rc = process_draft(M, i)) return rc;
    if (spec && s->spec_top_k > 0) {
      if (int rc = launch_spec_draft_draw_shaped(s->st, q_pass, M, M - 1, s->spec_q, i, V, s->temperature, s->spec_top_k, s->spec_top_p,
                                                 s->seed, s->draw, s->stream_id, st_d))
        return rc;
    } else if (spec) {   // exactly one form of forward 0 ran: one draw launch serves both
      if (int rc = launch_spec_draft_draw(s->st, q_pass, M, M - 1, s->spec_q, i, V, s->temperature, s->seed, s->draw, s->stream_id, st_d)) return rc;
    } else if (!one_pass_d && !lp) {
      if (int rc = launch_draft_next(M, i, s->st, st_d)) return rc;
    }
  }
  if (two) {
    SD_HIP_CHECK(hipEventRecord(s->ev_join, st_d));
    SD_HIP_CHECK(hipStreamWaitEvent(st_t, s->ev_join, 0));
  }
  // verify: one forward over (last, d_1..d_K)
  // greedy steps whose verify forward is ONE pass: ids, accept scan, state advance and the step record are one launch over the
  // lm_head's partials (verify_tail_kernel) instead of three
  const unsigned* const st_word_d = (s->draft && s->draft->p_sync) ? s->draft->p_sync + 1 : nullptr;
  const unsigned* const st_word_t = s->target->p_sync ? s->target->p_sync + 1 : nullptr;
  const bool tail = !s->sample && !spec && !lp && verify_tail_fits(s->st) && B * (K + 1) <= s->target->max_t;
  if (int rc = model_forward(s->target, s->st.verify_tok, K + 1, s->st.cur_len, 0, 0, B, K + 1, tail ? nullptr : s->st.target_ids,
                             K + 1, p_buf, SD_BF16, 0, st_t))
    return rc;
  if (lp)   // all B * (K+1) rows in one launch: row (b, i) is conditioned on d_1..d_i; the processed argmax replaces the fused ids
    if (int rc = launch_logit_process(p_buf, V, B, K + 1, V, s->lp_counts, s->lp_bias, s->st.draft_tok, K, -1, s->st.active, s->lp_rp,
                                      s->lp_presence, s->lp_frequency, s->st.target_ids, K + 1, s->lp_ws, s->lp_ws_bytes, st_t))
      return rc;
  if (tail) {
    if (int rc = launch_verify_tail(s->st, s->target->part_val, s->target->part_idx, s->target->head_grid, s->mode, s->host_record, s->rec,
                                    s->step_counter, st_word_d, st_word_t, st_t))
      return rc;
    if (!s->heads.empty())
      if (int rc = enqueue_medusa_heads(s, st_t)) return rc;
    return 0;
  }
  if (s->sample) {
    // accept length -> draw the token after the accepted prefix from the stored logits of that position
    if (int rc = launch_accept_len(s->st, st_t)) return rc;
    if (int rc = launch_sample_step(s->st, s->logits, s->target->cfg.vocab, s->temperature, s->top_k, s->top_p, s->seed,
                                    s->draw, s->stream_id, st_t))
      return rc;
  }
  if (spec && s->spec_top_k > 0) {
    if (int rc = launch_spec_step_shaped(s->st, s->spec_p, s->spec_q, V, s->temperature, s->spec_top_k, s->spec_top_p, s->seed, s->draw,
                                         s->stream_id, s->spec_flags, s->spec_flags + static_cast<size_t>(B) * (K + 1), st_t))
      return rc;
  } else if (spec) {
    // every position's ratio, flag and candidate in parallel -> accept length and the token after the accepted prefix
    if (int rc = launch_spec_step(s->st, s->spec_p, s->spec_q, V, s->temperature, s->seed, s->draw, s->stream_id, s->spec_flags,
                                  s->spec_flags + static_cast<size_t>(B) * (K + 1), st_t))
      return rc;
  }
  if (int rc = launch_accept(s->st, s->mode, spec ? 2 : s->sample, st_t)) return rc;
  if (lp)   // the emitted tokens of every active row enter its counts
    if (int rc = launch_logit_counts_add(s->lp_counts, B, V, s->st.new_tok, K + 1, s->st.n_new, K + 1, s->st.active, st_t)) return rc;
  if (int rc = launch_pack_record(s->st, s->host_record, s->rec, s->step_counter, st_word_d, st_word_t, st_t)) return rc;
  // persistent Medusa heads: the proposals of the next step, after the record of this one has left
  if (!s->heads.empty())
    if (int rc = enqueue_medusa_heads(s, st_t)) return rc;
  return 0;
}

}  // namespace sd

extern "C" int sd_specdec_create(sd_model* draft, sd_model* target, int B, int K, int emit_mode, sd_specdec** out) {
  clear_error();
  SD_REQUIRE(target && out, "specdec_create: NULL argument");   // draft == NULL: self-draft (Medusa-lite, tied heads)
  SD_REQUIRE(B >= 1 && K >= 1 && K <= 8, "specdec_create: B=%d K=%d (K in 1..8)", B, K);
  SD_REQUIRE(B * (K + 1) <= 65535, "specdec_create: batch too large");
  SD_REQUIRE((!draft || draft->B >= B) && target->B >= B, "specdec_create: models must be bound with batch >= %d", B);
  SD_REQUIRE(!draft || draft->cfg.vocab == target->cfg.vocab, "specdec_create: draft/target vocabularies differ");
  SD_REQUIRE(emit_mode == SD_EMIT_BONUS || emit_mode == SD_EMIT_DRAFT, "specdec_create: emit_mode %d", emit_mode);
  // verify of B rows must fit the passes of the target forward: any B works (tiled)
  sd_specdec* s = new (std::nothrow) sd_specdec();
  SD_REQUIRE(s, "specdec_create: out of memory");
  s->draft = draft;
  s->target = target;
  // nobody reads the hidden rows of a loop's draft: its persistent passes skip the stage taps (csrc/persist.hip, TAPS). The
  // choice belongs to the LOOP (enqueue_step sets it around the draft's forwards): the same model object used elsewhere — as a
  // standalone model, or as another loop's target — keeps its taps.
  s->draft_taps = getenv(debug_env::kPersistTaps) != nullptr;
  s->B = B;
  s->K = K;
  s->mode = emit_mode;
  s->rec = 7 + 3 * K;
  const size_t n_state = static_cast<size_t>(B) * (1 + 1 + 2 + 1 + 2 + K + (K + 1) + (K + 1) + 1 + 1 + (K + 1) + 1);
  const size_t n_adapt = static_cast<size_t>(B) * (1 + 4 + 8) + 2 + 2 + 2;   // k_row, ctl, ctl_hist (doubles), k_active (+ alignment), fwd0_w
  const size_t n_total = n_state + 4 + n_adapt;
  hipError_t e = hipMalloc(&s->dev_block, n_total * sizeof(int32_t));
  if (e != hipSuccess) {
    delete s;
    SD_REQUIRE(false, "specdec_create: hipMalloc failed: %s", hipGetErrorString(e));
  }
  (void)hipMemset(s->dev_block, 0, n_total * sizeof(int32_t));
  int32_t* p = s->dev_block;
  SpecState& st = s->st;
  st.B = B;
  st.K = K;
  st.cur_len = p; p += B;
  st.active = p; p += B;
  st.tok2 = p; p += 2 * B;
  st.next_tok = p; p += B;
  st.draft_ids = p; p += 2 * B;
  st.draft_tok = p; p += static_cast<size_t>(B) * K;
  st.verify_tok = p; p += static_cast<size_t>(B) * (K + 1);
  st.target_ids = p; p += static_cast<size_t>(B) * (K + 1);
  st.accept_len = p; p += B;
  st.n_new = p; p += B;
  st.new_tok = p; p += static_cast<size_t>(B) * (K + 1);
  st.sampled = p; p += B;
  s->step_counter = p; p += 4;
  if ((p - s->dev_block) & 1) ++p;         // the doubles below: 8-byte aligned (hipMalloc is 256-byte aligned)
  st.ctl_hist = reinterpret_cast<double*>(p); p += static_cast<size_t>(B) * 8;
  st.ctl = p; p += static_cast<size_t>(B) * 4;
  st.k_row = p; p += B;
  st.k_active = p; p += 1;
  st.adaptive = 0;
  // device-selected form of draft forward 0: one sequence, a draft whose 1- and 2-token passes are persistent launches (a pass
  // that is not needed then costs one launch that returns at entry, not 80)
  st.fwd0_w = nullptr;
  if (draft && B == 1 && draft->persist_cap >= 2 && !getenv(debug_env::kNoFwd0Select)) {
    st.fwd0_w = p; p += 2;
    const int32_t init[2] = {2, 1};
    (void)hipMemcpy(st.fwd0_w, init, sizeof(init), hipMemcpyHostToDevice);
  }
  if (hipHostMalloc(reinterpret_cast<void**>(&s->host_record), sizeof(int32_t) * 2 * B * s->rec, hipHostMallocDefault) != hipSuccess ||
      hipEventCreateWithFlags(&s->ev_done[0], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&s->ev_done[1], hipEventDisableTiming) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&s->host_stage), sizeof(int32_t) * (B * kStageInts + 4), hipHostMallocDefault) != hipSuccess ||
      hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming) != hipSuccess) {
    sd_specdec_destroy(s);
    SD_REQUIRE(false, "specdec_create: pinned memory / event creation failed");
  }
  *out = s;
  return 0;
}

extern "C" int sd_specdec_destroy(sd_specdec* s) {
  if (!s) return 0;
  if (s->exec) (void)hipGraphExecDestroy(s->exec);
  if (s->graph) (void)hipGraphDestroy(s->graph);
  if (s->ev_done[0]) (void)hipEventDestroy(s->ev_done[0]);
  if (s->ev_done[1]) (void)hipEventDestroy(s->ev_done[1]);
  if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
  if (s->ev_join) (void)hipEventDestroy(s->ev_join);
  if (s->host_record) (void)hipHostFree(s->host_record);
  if (s->host_stage) (void)hipHostFree(s->host_stage);
  if (s->dev_block) (void)hipFree(s->dev_block);
  if (s->head_rows) (void)hipFree(s->head_rows);
  if (s->spec_flags) (void)hipFree(s->spec_flags);
  delete s;
  return 0;
}

extern "C" int sd_specdec_set_row(sd_specdec* s, int b, int seq_len, int prev_tok, int last_tok, int active,
                                  void* stream) {
  clear_error();
  SD_REQUIRE(s, "specdec_set_row: NULL");
  SD_REQUIRE(b >= 0 && b < s->B, "specdec_set_row: row %d out of range", b);
  SD_REQUIRE(seq_len >= 1, "specdec_set_row: seq_len=%d (need at least one token)", seq_len);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the staging slot of row b must not be rewritten while a previous copy is in flight
  SD_HIP_CHECK(hipStreamSynchronize(st));
  int32_t* h = s->host_stage + b * kStageInts;
  h[0] = seq_len - 1;  // cur_len: position of `last`
  h[1] = active ? 1 : 0;
  h[2] = prev_tok;
  h[3] = last_tok;
  SD_HIP_CHECK(hipMemcpyAsync(s->st.cur_len + b, h + 0, 4, hipMemcpyHostToDevice, st));
  SD_HIP_CHECK(hipMemcpyAsync(s->st.active + b, h + 1, 4, hipMemcpyHostToDevice, st));
  SD_HIP_CHECK(hipMemcpyAsync(s->st.tok2 + 2 * b, h + 2, 8, hipMemcpyHostToDevice, st));
  SD_HIP_CHECK(hipMemcpyAsync(s->st.verify_tok + static_cast<size_t>(b) * (s->K + 1), h + 3, 4, hipMemcpyHostToDevice, st));
  if (s->st.fwd0_w) {   // whatever the caller did to the caches: the next step recomputes prev's K/V
    h[4] = 2;
    h[5] = 1;
    SD_HIP_CHECK(hipMemcpyAsync(s->st.fwd0_w, h + 4, 8, hipMemcpyHostToDevice, st));
  }
  return 0;
}

// Per-row adaptive K. The captured step keeps the shape K = max_k; row b's proposals past k_row[b]
// do not count (accept length clamped, bonus token = the target's token after the clamped prefix), and accept_kernel
// moves k_row[b] by the reference's rule. enable: all rows restart (k = initial_k, history = [0.0] — the reference's
// first get_k call reports acceptance_rate 0.0 before any step).
extern "C" int sd_specdec_set_adaptive(sd_specdec* s, int enable, int initial_k, int min_k, int max_k, int step_size,
                                       double target_rate, void* stream) {
  clear_error();
  SD_REQUIRE(s, "specdec_set_adaptive: NULL");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (s->exec) {   // the captured kernels hold the loop state by value
    (void)hipGraphExecDestroy(s->exec);
    (void)hipGraphDestroy(s->graph);
    s->exec = nullptr;
    s->graph = nullptr;
  }
  if (!enable) {
    s->st.adaptive = 0;
    return 0;
  }
  SD_REQUIRE(min_k >= 1 && min_k <= max_k && max_k <= s->K, "specdec_set_adaptive: need 1 <= min_k (%d) <= max_k (%d) <= K of the loop (%d)", min_k, max_k, s->K);
  SD_REQUIRE(initial_k >= min_k && initial_k <= max_k, "specdec_set_adaptive: initial_k %d outside [%d, %d]", initial_k, min_k, max_k);
  SD_REQUIRE(step_size >= 1, "specdec_set_adaptive: step_size %d", step_size);
  SD_REQUIRE(target_rate == target_rate, "specdec_set_adaptive: target rate is NaN");
  SD_REQUIRE(s->heads.empty() && !s->eagle, "specdec_set_adaptive: stateful draft modes keep a fixed K");
  SD_REQUIRE(!s->spec, "specdec_set_adaptive: speculative sampling keeps a fixed K (disable it first)");
  SD_REQUIRE(!s->lp, "specdec_set_adaptive: logit processors keep a fixed K (disable sd_specdec_set_logit_processors first)");
  s->st.adaptive = 1;
  s->st.a_min = min_k;
  s->st.a_max = max_k;
  s->st.a_step = step_size;
  s->st.a_hi = target_rate + 0.1;
  s->st.a_lo = target_rate - 0.1;
  s->a_initial = initial_k;
  for (int b = 0; b < s->B; ++b)
    if (int rc = sd_specdec_set_adaptive_row(s, b, initial_k, 0, 0, 1, nullptr, st)) return rc;
  return 0;
}

// (Re)write one row's controller state — a new sequence in the row's slot, or the host's in-order view after the host
// rules overrode steps that were launched ahead. hist: hist_n <= 4 rates, oldest first (NULL: [0.0]).
extern "C" int sd_specdec_set_adaptive_row(sd_specdec* s, int b, int k, int accepted, int proposed, int hist_n, const double* hist,
                                           void* stream) {
  clear_error();
  SD_REQUIRE(s && s->st.adaptive, "specdec_set_adaptive_row: adaptive K is not enabled");
  SD_REQUIRE(b >= 0 && b < s->B, "specdec_set_adaptive_row: row %d out of range", b);
  SD_REQUIRE(k >= s->st.a_min && k <= s->st.a_max, "specdec_set_adaptive_row: k=%d outside [%d, %d]", k, s->st.a_min, s->st.a_max);
  SD_REQUIRE(hist_n >= 0 && hist_n <= 4 && accepted >= 0 && proposed >= 0, "specdec_set_adaptive_row: bad counters");
  hipStream_t st = static_cast<hipStream_t>(stream);
  SD_HIP_CHECK(hipStreamSynchronize(st));   // the staging slot must not be rewritten under a copy in flight
  int32_t* h = s->host_stage + b * kStageInts + 8;
  double* hd = reinterpret_cast<double*>(h + 4);
  h[0] = accepted;
  h[1] = proposed;
  h[2] = hist ? hist_n : 1;
  h[3] = k;
  for (int i = 0; i < 4; ++i) hd[i] = (hist && i < hist_n) ? hist[i] : 0.0;
  SD_HIP_CHECK(hipMemcpyAsync(s->st.ctl + 4 * b, h, 16, hipMemcpyHostToDevice, st));
  SD_HIP_CHECK(hipMemcpyAsync(s->st.ctl_hist + 4 * b, hd, 32, hipMemcpyHostToDevice, st));
  SD_HIP_CHECK(hipMemcpyAsync(s->st.k_row + b, h + 3, 4, hipMemcpyHostToDevice, st));
  // k_active (which draft forwards run) is recomputed at the end of every step; until then: all of them
  int32_t* ka = s->host_stage + s->B * kStageInts;
  *ka = s->st.a_max;
  SD_HIP_CHECK(hipMemcpyAsync(s->st.k_active, ka, 4, hipMemcpyHostToDevice, st));
  return 0;
}

extern "C" int sd_specdec_set_sampling(sd_specdec* s, int enable, float temperature, int top_k, float top_p,
                                       uint64_t seed, void* logits_buf, size_t logits_bytes, uint32_t* draw_counters,
                                       const int32_t* stream_ids) {
  clear_error();
  SD_REQUIRE(s, "specdec_set_sampling: NULL");
  if (s->exec) {  // the captured step holds the sampling launches and their parameters
    (void)hipGraphExecDestroy(s->exec);
    (void)hipGraphDestroy(s->graph);
    s->exec = nullptr;
    s->graph = nullptr;
  }
  if (!enable) {
    s->sample = 0;
    return 0;
  }
  SD_REQUIRE(s->mode == SD_EMIT_BONUS, "specdec_set_sampling: only the bonus-token emit mode (generate_batch) samples");
  SD_REQUIRE(!s->spec, "specdec_set_sampling: speculative sampling is enabled (sd_specdec_set_spec_sampling); the two modes are mutually exclusive");
  SD_REQUIRE(logits_buf && draw_counters, "specdec_set_sampling: NULL logits buffer / draw counters");
  const size_t need = static_cast<size_t>(s->B) * (s->K + 1) * s->target->cfg.vocab * 2;
  SD_REQUIRE(logits_bytes >= need, "specdec_set_sampling: logits buffer %zu B < %zu B ([B][K+1][V] bf16)", logits_bytes, need);
  SD_REQUIRE(temperature == temperature && temperature >= 0.f, "specdec_set_sampling: temperature %g", temperature);
  SD_REQUIRE(top_k <= 0 || (top_k < s->target->cfg.vocab ? top_k : s->target->cfg.vocab) <= 1024, "specdec_set_sampling: top_k=%d > 1024", top_k);
  s->sample = 1;
  s->temperature = temperature;
  s->top_k = top_k;
  s->top_p = top_p;
  s->seed = seed;
  s->logits = logits_buf;
  s->draw = draw_counters;
  s->stream_id = stream_ids;
  return 0;
}

extern "C" int sd_specdec_set_spec_sampling(sd_specdec* s, int enable, float temperature, uint64_t seed, void* draft_logits_buf,
                                            size_t draft_logits_bytes, void* target_logits_buf, size_t target_logits_bytes,
                                            uint32_t* draw_counters, const int32_t* stream_ids) {
  clear_error();
  SD_REQUIRE(s, "specdec_set_spec_sampling: NULL");
  if (!enable) {
    if (s->spec && s->exec) {
      (void)hipGraphExecDestroy(s->exec);
      (void)hipGraphDestroy(s->graph);
      s->exec = nullptr;
      s->graph = nullptr;
    }
    s->spec = 0;
    return 0;
  }
  SD_REQUIRE(s->mode == SD_EMIT_BONUS, "specdec_set_spec_sampling: only the bonus-token emit mode (generate_batch); SD_EMIT_DRAFT is not supported");
  SD_REQUIRE(s->draft, "specdec_set_spec_sampling: needs a draft model (self-draft, Medusa heads and EAGLE loops propose without a distribution q)");
  SD_REQUIRE(!s->st.adaptive, "specdec_set_spec_sampling: per-row adaptive K is not supported (disable sd_specdec_set_adaptive first)");
  SD_REQUIRE(!s->sample, "specdec_set_spec_sampling: the sampled-bonus mode is enabled (sd_specdec_set_sampling); the two modes are mutually exclusive");
  SD_REQUIRE(temperature == temperature && temperature > 0.f, "specdec_set_spec_sampling: temperature %g (must be > 0)", temperature);
  SD_REQUIRE(draft_logits_buf && target_logits_buf && draw_counters, "specdec_set_spec_sampling: NULL logits buffer / draw counters");
  const size_t V = static_cast<size_t>(s->target->cfg.vocab);
  const size_t need_q = static_cast<size_t>(s->B) * s->K * V * 2, need_p = static_cast<size_t>(s->B) * (s->K + 1) * V * 2;
  SD_REQUIRE(draft_logits_bytes >= need_q, "specdec_set_spec_sampling: draft logits buffer %zu B < %zu B ([B][K][V] bf16)", draft_logits_bytes, need_q);
  SD_REQUIRE(target_logits_bytes >= need_p, "specdec_set_spec_sampling: target logits buffer %zu B < %zu B ([B][K+1][V] bf16)", target_logits_bytes, need_p);
  SD_REQUIRE(((reinterpret_cast<uintptr_t>(draft_logits_buf) | reinterpret_cast<uintptr_t>(target_logits_buf)) & 15) == 0,
             "specdec_set_spec_sampling: logits buffers must be 16-byte aligned");
  if (!s->spec_flags) SD_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&s->spec_flags), sizeof(int32_t) * 2 * s->B * (s->K + 1)));
  if (s->exec) {  // the captured step holds the other mode's launches, or this mode's parameters
    (void)hipGraphExecDestroy(s->exec);
    (void)hipGraphDestroy(s->graph);
    s->exec = nullptr;
    s->graph = nullptr;
  }
  s->spec = 1;
  s->temperature = temperature;
  s->seed = seed;
  s->spec_q = draft_logits_buf;
  s->spec_p = target_logits_buf;
  s->draw = draw_counters;
  s->stream_id = stream_ids;
  return 0;
}

extern "C" int sd_specdec_set_logit_processors(sd_specdec* s, int enable, float repetition_penalty, float presence_penalty,
                                               float frequency_penalty, void* counts, size_t counts_bytes, const float* bias,
                                               size_t bias_bytes, void* logits_buf, size_t logits_bytes, void* workspace,
                                               size_t workspace_bytes_) {
  clear_error();
  SD_REQUIRE(s, "specdec_set_logit_processors: NULL");
  if (!enable) {
    if (s->lp && s->exec) {
      (void)hipGraphExecDestroy(s->exec);
      (void)hipGraphDestroy(s->graph);
      s->exec = nullptr;
      s->graph = nullptr;
    }
    s->lp = 0;
    return 0;
  }
  SD_REQUIRE(s->draft, "specdec_set_logit_processors: needs a draft model (self-draft, Medusa heads and EAGLE loops propose from no logits row)");
  SD_REQUIRE(!s->st.adaptive, "specdec_set_logit_processors: per-row adaptive K is not supported (disable sd_specdec_set_adaptive first)");
  SD_REQUIRE(repetition_penalty == repetition_penalty && repetition_penalty > 0.f,
             "specdec_set_logit_processors: repetition_penalty %g (must be > 0)", repetition_penalty);
  SD_REQUIRE(presence_penalty - presence_penalty == 0.f && frequency_penalty - frequency_penalty == 0.f,
             "specdec_set_logit_processors: presence_penalty %g / frequency_penalty %g must be finite", presence_penalty, frequency_penalty);
  const size_t V = static_cast<size_t>(s->target->cfg.vocab), BV = static_cast<size_t>(s->B) * V;
  SD_REQUIRE(counts && counts_bytes >= BV * 2, "specdec_set_logit_processors: counts buffer %zu B < %zu B ([B][V] uint16)", counts_bytes, BV * 2);
  SD_REQUIRE(!bias || bias_bytes >= BV * 4, "specdec_set_logit_processors: bias buffer %zu B < %zu B ([B][V] float32)", bias_bytes, BV * 4);
  const size_t need_p = BV * (s->K + 1) * 2, need_ws = logit_process_workspace(s->B, s->K + 1, static_cast<int>(V));
  SD_REQUIRE(logits_buf || s->sample || s->spec, "specdec_set_logit_processors: NULL logits buffer (no sampling mode is on to lend its own)");
  SD_REQUIRE(!logits_buf || logits_bytes >= need_p, "specdec_set_logit_processors: logits buffer %zu B < %zu B ([B][K+1][V] bf16)", logits_bytes, need_p);
  SD_REQUIRE(workspace && workspace_bytes_ >= need_ws, "specdec_set_logit_processors: workspace %zu B < %zu B", workspace_bytes_, need_ws);
  SD_REQUIRE(((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(logits_buf) |
               reinterpret_cast<uintptr_t>(workspace)) & 15) == 0, "specdec_set_logit_processors: buffers must be 16-byte aligned");
  if (s->exec) {  // the captured step holds the unprocessed launches, or this mode's parameters
    (void)hipGraphExecDestroy(s->exec);
    (void)hipGraphDestroy(s->graph);
    s->exec = nullptr;
    s->graph = nullptr;
  }
  s->lp = 1;
  s->lp_rp = repetition_penalty;
  s->lp_presence = presence_penalty;
  s->lp_frequency = frequency_penalty;
  s->lp_counts = static_cast<uint16_t*>(counts);
  s->lp_bias = bias;
  s->lp_logits = logits_buf;
  s->lp_ws = workspace;
  s->lp_ws_bytes = workspace_bytes_;
  return 0;
}

extern "C" int sd_specdec_set_spec_shaping(sd_specdec* s, int top_k, float top_p) {
  clear_error();
  SD_REQUIRE(top_p == top_p && top_p > 0.f, "specdec_set_spec_shaping: top_p %g (must be > 0)", top_p);
  SD_REQUIRE(top_k > 0 || top_p >= 1.0f, "specdec_set_spec_shaping: top_p = %g without top_k (the full-vocabulary nucleus) is not supported; "
             "give a top_k in 1..1024", top_p);
  SD_REQUIRE(top_k <= 1024, "specdec_set_spec_shaping: top_k=%d > 1024 is not supported", top_k);
  SD_REQUIRE(s, "specdec_set_spec_shaping: NULL");
  if (s->exec) {  // the captured step holds the launches of the other shape
    (void)hipGraphExecDestroy(s->exec);
    (void)hipGraphDestroy(s->graph);
    s->exec = nullptr;
    s->graph = nullptr;
  }
  s->spec_top_k = top_k > 0 ? top_k : 0;
  s->spec_top_p = top_k > 0 ? top_p : 1.0f;
  return 0;
}

extern "C" size_t sd_specdec_eagle_bytes(int B, int K, int d_model) {
  if (B <= 0 || K <= 0 || d_model <= 0) return 0;
  return (static_cast<size_t>(B) * K * d_model + static_cast<size_t>(B) * d_model) * 2 + static_cast<size_t>(B) * 4 + 1024;
}

// workspace layout: [state rows B x d bf16][has_prev B x int32][extrapolated rows B*K x d bf16] — the state sits at
// offsets that do not depend on K, so loops of different K over the same workspace (adaptive K) share it
extern "C" int sd_specdec_set_eagle(sd_specdec* s, float alpha, void* workspace, size_t workspace_bytes_) {
  clear_error();
  SD_REQUIRE(s && workspace, "specdec_set_eagle: NULL argument");
  SD_REQUIRE(!s->draft, "specdec_set_eagle: the loop was created with a draft model (pass draft = NULL)");
  SD_REQUIRE(s->heads.empty(), "specdec_set_eagle: the loop already has Medusa heads");
  const int d = s->target->cfg.d_model;
  SD_REQUIRE(workspace_bytes_ >= sd_specdec_eagle_bytes(s->B, s->K, d), "specdec_set_eagle: workspace too small");
  SD_REQUIRE(s->B * s->K <= s->target->max_t, "specdec_set_eagle: B*K = %d rows exceed one lm_head pass (%d)", s->B * s->K, s->target->max_t);
  SD_REQUIRE(!s->exec, "specdec_set_eagle: call before the first captured step");
  char* p = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~static_cast<uintptr_t>(255));
  s->eagle_prev = reinterpret_cast<uint16_t*>(p);
  p += (static_cast<size_t>(s->B) * d * 2 + 255) & ~static_cast<size_t>(255);
  s->eagle_has = reinterpret_cast<int32_t*>(p);
  p += (static_cast<size_t>(s->B) * 4 + 255) & ~static_cast<size_t>(255);
  s->eagle_H = reinterpret_cast<uint16_t*>(p);
  s->eagle_alpha = alpha;
  s->eagle = 1;
  return 0;
}

extern "C" int sd_specdec_reset_eagle(sd_specdec* s, void* stream) {
  clear_error();
  SD_REQUIRE(s && s->eagle, "specdec_reset_eagle: EAGLE mode is not set");
  SD_HIP_CHECK(hipMemsetAsync(s->eagle_has, 0, static_cast<size_t>(s->B) * 4, static_cast<hipStream_t>(stream)));
  return 0;
}

// bytes between consecutive heads when they sit at a constant, ascending stride (-> one launch for all of them), else 0
static size_t constant_stride(int n_heads, const void* const* packed_heads) {
  if (n_heads < 2) return 0;
  const char* h0 = static_cast<const char*>(packed_heads[0]);
  const char* h1 = static_cast<const char*>(packed_heads[1]);
  bool even = h1 > h0;
  for (int i = 2; even && i < n_heads; ++i)
    even = static_cast<const char*>(packed_heads[i]) - static_cast<const char*>(packed_heads[i - 1]) == h1 - h0;
  return even ? static_cast<size_t>(h1 - h0) : 0;
}

extern "C" int sd_specdec_set_medusa(sd_specdec* s, int n_heads, const void* const* packed_heads, int weight_dtype) {
  clear_error();
  SD_REQUIRE(s, "specdec_set_medusa: NULL");
  SD_REQUIRE(!s->draft, "specdec_set_medusa: the loop was created with a draft model (pass draft = NULL)");
  SD_REQUIRE(n_heads == s->K && packed_heads, "specdec_set_medusa: need K = %d heads, got %d", s->K, n_heads);
  SD_REQUIRE(weight_dtype == SD_BF16 || weight_dtype == SD_FP8_E4M3, "specdec_set_medusa: weight_dtype %d", weight_dtype);
  const sd_model_config& c = s->target->cfg;
  SD_REQUIRE(s->B <= s->target->small_t || (s->B <= s->target->max_t && c.n_heads * c.head_dim >= c.d_model),
             "specdec_set_medusa: batch %d exceeds one pass of the head kernels (%d rows)", s->B, s->target->max_t);
  SD_REQUIRE(s->B * (s->K + 1) <= s->target->max_t, "specdec_set_medusa: the verify pass must be a single pass (B*(K+1) = %d > %d)",
             s->B * (s->K + 1), s->target->max_t);
  if (s->exec) {
    (void)hipGraphExecDestroy(s->exec);
    (void)hipGraphDestroy(s->graph);
    s->exec = nullptr;
    s->graph = nullptr;
  }
  s->heads.clear();
  s->head_scales.clear();
  for (int i = 0; i < n_heads; ++i) {
    SD_REQUIRE(packed_heads[i], "specdec_set_medusa: head %d is NULL", i);
    s->heads.push_back(packed_heads[i]);
    if (weight_dtype == SD_FP8_E4M3) {
      const MatShape h = matrix_shape(c, 4);   // the fp32 row scales follow the packed bytes (sd_pack_head)
      s->head_scales.push_back(reinterpret_cast<const float*>(static_cast<const char*>(packed_heads[i]) + packed_fp8_weight_bytes(h.n_pairs, h.K)));
    }
  }
  s->head_stride = getenv(debug_env::kMedusaPerHead) ? 0 : constant_stride(n_heads, packed_heads);
  if (!s->head_rows) SD_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&s->head_rows), sizeof(int32_t) * s->B));
  return 0;
}

// The step's head evaluation (enqueue_head_argmax) on caller-supplied rows: ids and the value attached to each of them.
extern "C" int sd_model_head_argmax(sd_model* m, const void* x_bf16, int n_rows, const int32_t* row_idx, int B, int n_heads,
                                    const void* const* packed_heads, int weight_dtype, int flags, int32_t* ids, float* vals,
                                    int* launch_info, void* stream) {
  clear_error();
  SD_REQUIRE(m && m->x && x_bf16 && packed_heads && ids, "model_head_argmax: NULL argument / model not bound");
  SD_REQUIRE(n_heads >= 1 && n_heads <= 64, "model_head_argmax: n_heads=%d (1..64)", n_heads);
  SD_REQUIRE(weight_dtype == SD_BF16 || weight_dtype == SD_FP8_E4M3, "model_head_argmax: weight_dtype %d", weight_dtype);
  SD_REQUIRE((flags & ~(SD_HEADS_PER_HEAD | SD_HEADS_NORMALISED)) == 0, "model_head_argmax: unknown flags %#x", flags);
  const sd_model_config& c = m->cfg;
  SD_REQUIRE(weight_dtype == SD_BF16 || c.d_model % 64 == 0, "model_head_argmax: fp8 heads need d_model (%d) in whole 64-k steps", c.d_model);
  SD_REQUIRE(B >= 1 && n_rows >= 1 && (row_idx || B <= n_rows), "model_head_argmax: B=%d rows of %d", B, n_rows);
  SD_REQUIRE(B <= m->small_t || (B <= m->max_t && (!row_idx || c.n_heads * c.head_dim >= c.d_model)),
             "model_head_argmax: batch %d exceeds one pass of the head kernels (%d rows)", B, m->max_t);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (row_idx) {   // a debug entry: the indices are checked on the host before any kernel follows them
    std::vector<int32_t> host(static_cast<size_t>(B));
    SD_HIP_CHECK(hipMemcpyAsync(host.data(), row_idx, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
    SD_HIP_CHECK(hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b)
      SD_REQUIRE(host[b] >= 0 && host[b] < n_rows, "model_head_argmax: row_idx[%d] = %d outside the %d rows", b, host[b], n_rows);
  }
  std::vector<const void*> heads;
  std::vector<const float*> scales;
  const MatShape hs = matrix_shape(c, 4);
  for (int i = 0; i < n_heads; ++i) {
    SD_REQUIRE(packed_heads[i], "model_head_argmax: head %d is NULL", i);
    SD_REQUIRE((reinterpret_cast<uintptr_t>(packed_heads[i]) & 255) == 0, "model_head_argmax: head %d is not 256-byte aligned", i);
    heads.push_back(packed_heads[i]);
    if (weight_dtype == SD_FP8_E4M3)   // the fp32 row scales follow the packed bytes (sd_pack_head)
      scales.push_back(reinterpret_cast<const float*>(static_cast<const char*>(packed_heads[i]) + packed_fp8_weight_bytes(hs.n_pairs, hs.K)));
  }
  HeadEval e;
  e.x = x_bf16;
  e.x_row = row_idx;
  e.T = B;
  e.n_heads = n_heads;
  e.W = heads.data();
  e.scale = scales.empty() ? nullptr : scales.data();
  e.stride = (flags & SD_HEADS_PER_HEAD) ? 0 : constant_stride(n_heads, packed_heads);
  e.w8 = scales.empty() ? 0 : 1;
  e.prenormed = (flags & SD_HEADS_NORMALISED) != 0;
  e.ids = ids;
  e.ids_stride = n_heads;
  e.vals = vals;
  if (launch_info) launch_info[0] = launch_info[1] = 0;
  e.launch_info = launch_info;
  return enqueue_head_argmax(m, e, st);
}

extern "C" int sd_eagle_extrapolate(const void* x_bf16, void* H, void* prev, int32_t* has_prev, const void* norm_w, const void* norm_b,
                                    float eps, float alpha, int d_model, int B, int K, int rms, void* stream) {
  clear_error();
  SD_REQUIRE(x_bf16 && H && prev && has_prev && norm_w, "eagle_extrapolate: NULL argument");
  SD_REQUIRE(rms || norm_b, "eagle_extrapolate: LayerNorm needs the bias");
  SD_REQUIRE(d_model >= 1 && B >= 1 && B <= 65535 && K >= 1 && K <= 8, "eagle_extrapolate: d_model=%d B=%d K=%d (K in 1..8)", d_model, B, K);
  return launch_eagle_extrapolate(x_bf16, H, prev, has_prev, norm_w, norm_b, eps, alpha, d_model, B, K, rms ? 1 : 0,
                                  static_cast<hipStream_t>(stream));
}

extern "C" int sd_specdec_step(sd_specdec* s, void* stream_target, void* stream_draft, int use_graph) {
  clear_error();
  SD_REQUIRE(s, "specdec_step: NULL");
  hipStream_t st_t = static_cast<hipStream_t>(stream_target);
  hipStream_t st_d = stream_draft ? static_cast<hipStream_t>(stream_draft) : st_t;
  s->steps++;
  if (!use_graph || s->steps == 1) {
    // the first step always runs eagerly: it also performs the one-time kernel
    // attribute setup that must not happen inside a capture
    if (int rc = enqueue_step(s, st_t, st_d)) return rc;
    SD_HIP_CHECK(hipEventRecord(s->ev_done[s->launches & 1], st_t));
    s->launches++;
    return 0;
  }
  if (s->exec && (s->graph_st_t != st_t || s->graph_st_d != st_d)) {
    (void)hipGraphExecDestroy(s->exec);
    (void)hipGraphDestroy(s->graph);
    s->exec = nullptr;
    s->graph = nullptr;
  }
  if (!s->exec) {
    SD_HIP_CHECK(hipStreamBeginCapture(st_t, hipStreamCaptureModeRelaxed));
    const int rc = enqueue_step(s, st_t, st_d);
    hipGraph_t g = nullptr;
    const hipError_t ee = hipStreamEndCapture(st_t, &g);
    if (rc != 0) {
      if (g) (void)hipGraphDestroy(g);
      return rc;
    }
    SD_HIP_CHECK(ee);
    s->graph = g;
    SD_HIP_CHECK(hipGraphInstantiate(&s->exec, s->graph, nullptr, nullptr, 0));
    s->graph_st_t = st_t;
    s->graph_st_d = st_d;
  }
  SD_HIP_CHECK(hipGraphLaunch(s->exec, st_t));
  SD_HIP_CHECK(hipEventRecord(s->ev_done[s->launches & 1], st_t));   // completion of THIS step (sd_specdec_wait)
  s->launches++;
  return 0;
}

extern "C" int sd_specdec_invalidate(sd_specdec* s) {
  clear_error();
  SD_REQUIRE(s, "specdec_invalidate: NULL");
  if (s->exec) {
    (void)hipGraphExecDestroy(s->exec);
    (void)hipGraphDestroy(s->graph);
    s->exec = nullptr;
    s->graph = nullptr;
  }
  s->steps = 0;   // the next step runs eagerly (kernels of the other path may still need their one-time attribute setup)
  return 0;
}

extern "C" long sd_specdec_launches(const sd_specdec* s) { return s ? s->launches : 0; }

extern "C" int sd_specdec_wait(sd_specdec* s, long launch_index) {
  clear_error();
  SD_REQUIRE(s, "specdec_wait: NULL");
  SD_REQUIRE(launch_index >= 0 && launch_index < s->launches && launch_index + 2 >= s->launches,
             "specdec_wait: step %ld is not one of the last two launches (%ld launched)", launch_index, s->launches);
  SD_HIP_CHECK(hipEventSynchronize(s->ev_done[launch_index & 1]));
  return 0;
}

extern "C" int sd_specdec_sync(sd_specdec* s, void* stream) {
  clear_error();
  (void)s;
  SD_HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return 0;
}

// two slots of [B][record_ints]: the record of launch i is in slot i & 1
extern "C" const int32_t* sd_specdec_record(const sd_specdec* s) { return s ? s->host_record : nullptr; }

extern "C" int sd_specdec_record_ints(const sd_specdec* s) { return s ? s->rec : 0; }
