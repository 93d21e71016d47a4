// Decoder forward orchestration for gfx950: the model behind sd_model_* (create, bind, forward, prompt
// routing, scoring, probes and plan queries). The draft-then-verify step that drives two of
// these models is csrc/spec_loop.hip.
//
// Host-side C++ behind the C-ABI (include/specdec_hip.h). It enqueues the kernels
// of gemv.hip / attention.hip / misc.hip on caller-provided HIP streams, never
// synchronises, and is graph-capturable: all per-row dynamic quantities (lengths,
// tokens) live in device memory and are read by the kernels.
//
// What it replaces in the reference: HFWrapper._generate_tokens_async
// (hf_wrappers.py:272-627: one HF forward + argmax per generated token, the whole
// prefix re-fed unless a KV cache is threaded through).

#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>

#include "engine.h"

namespace sd {
// One CU (three waves) walks a head's whole cache in the persistent launch, where the launch path splits long rows over up to 32
// workgroups — 1B dimensions, 1 token, us per forward persistent / launches at 128 ... 4096 cached positions: 588 / 675,
// 605 / 694, 651 / 721, 723 / 764, 888 / 767, 1186 / 777 (profiles/round3_persist_ab.md): the persistent launch serves rows of
// up to this many positions (where the two lines cross: 723 + 0.161 (L - 1024) against 764 + 0.003 (L - 1024) us at L = 1283;
// round 4's context sweep: 5.07 ms per step on the persistent launch at 1400-1536 positions against 4.96 on the launch path at 2048).
constexpr int kPersistMaxCtx = 1280;
bool persist_pass_ok(const sd_model* m, int T, int Bc, int Mc) {
  return m->persist_t > 0 && T <= m->persist_t && Mc <= 8 && !m->block_table && Bc * m->cfg.n_heads <= kPersistCUs && m->len_hint <= m->ctx_limit;
}
}  // namespace sd

namespace sd {

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
GemvArgs matrix_args(const sd_model* m, int index) {
  const sd_model_config& c = m->cfg;
  const int which = matrix_which(c, index);
  const MatShape sh = matrix_shape(c, which);
  const MatWeights wt = matrix_weights(c, index);
  GemvArgs a{};
  a.W = m->mat(index, wt.w);
  a.w_scale = m->scale(index);
  a.packed = m->is_packed();
  a.w8 = m->w8();
  if (!m->w12.empty() && m->w12[index].main) {
    a.w12_main = m->w12[index].main;
    a.w12_table = m->w12[index].table;
    a.w12_ovf = m->w12[index].ovf;
    a.w12_form = m->w12[index].form;
  }
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
int model_forward(sd_model* m, const int32_t* tokens, int tok_stride, const int32_t* pos_base,
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

// the matrices of `classes` onto a copy of `form`; the other matrices keep what they stream
static int model_add_w12(sd_model* m, const void* w12, const uint32_t* n_wide, unsigned classes, int form) {
  SD_REQUIRE(w12 && n_wide, "model_set_w12: NULL buffer or counts");
  SD_REQUIRE(form == W12_CODES || form == W12_SPLIT, "model_set_w12: form %d (SD_W12_FORM_CODES or SD_W12_FORM_SPLIT)", form);
  SD_REQUIRE(m->is_packed() && !m->w8() && m->cfg.weight_dtype == SD_BF16, "model_set_w12: W12 is a copy of packed bf16 weights");
  SD_REQUIRE((reinterpret_cast<uintptr_t>(w12) & 255) == 0, "model_set_w12: the buffer must be 256-byte aligned");
  const sd_model_config& c = m->cfg;
  if (m->w12.empty()) m->w12.assign(4 * c.n_layers + 1, sd_model::W12Mat{nullptr, nullptr, nullptr, W12_NONE});
  for (int i = 0; i <= 4 * c.n_layers; ++i) {
    const int which = matrix_which(c, i);
    const MatShape sh = matrix_shape(c, which);
    if (!w12_taken(sh.n_pairs, sh.K, n_wide[i]) || !((classes >> which) & 1)) continue;
    const W12Layout l = w12_layout(sh.n_pairs, sh.K, n_wide[i]);
    const char* p = static_cast<const char*>(w12) + w12_offset(c, n_wide, i);
    m->w12[i] = {p, reinterpret_cast<const uint32_t*>(p + l.main_bytes + l.ovf_bytes), p + l.main_bytes, form};
  }
  return 0;
}

extern "C" int sd_model_set_w12(sd_model* m, const void* w12, const uint32_t* n_wide, unsigned classes) {
  clear_error();
  SD_REQUIRE(m, "model_set_w12: NULL model");
  m->w12.clear();
  if (!w12) return 0;   // back to the bf16 streams
  return model_add_w12(m, w12, n_wide, classes, W12_CODES);
}

extern "C" int sd_model_set_w12_form(sd_model* m, const void* w12, const uint32_t* n_wide, unsigned classes, int form) {
  clear_error();
  SD_REQUIRE(m, "model_set_w12_form: NULL model");
  return model_add_w12(m, w12, n_wide, classes, form);
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
  const int n = gemv_variant_name(T, n_pairs, K, w8 == 1, prologue, epi, name, sizeof(name), w8 == 2 ? W12_CODES : w8 == 3 ? W12_SPLIT : W12_NONE);   // w8: 0 bf16, 1 fp8, 2 bf16 with a W12 copy, 3 with a W12S copy
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
  if (int rc = gemv_instance_name(T, n_pairs, K, w8 == 1, prologue, epi, name, sizeof(name), &n, w8 == 2 ? W12_CODES : w8 == 3 ? W12_SPLIT : W12_NONE)) return rc;   // a launch launch_gemv refuses, in its words
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
