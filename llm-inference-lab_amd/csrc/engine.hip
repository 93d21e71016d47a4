// Decoder forward orchestration for gfx950: the forward behind sd_model_forward / sd_model_score (the passes, prompt routing,
// scoring). The model's lifetime and storage are csrc/model.hip, its measurement hooks and row read-backs csrc/probe.hip, the
// GPU-free plan queries csrc/plan_query.hip. The draft-then-verify step that drives two of these models is csrc/spec_loop.hip.
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

#include "engine.h"

namespace sd {

bool persist_pass_ok(const sd_model* m, int T, int Bc, int Mc) {
  return m->persist_t > 0 && T <= m->persist_t && Mc <= 8 && !m->block_table && Bc * m->cfg.n_heads <= kPersistCUs && m->len_hint <= m->ctx_limit;
}

// Matrix `index` (4 * layer + which; 4 * n_layers = the lm_head) as the forward launches it: weights, shape and bias, the fused
// norm, and the workspace rows it reads and writes. The caller adds what belongs to the call (call_args), caches and statistics.
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
  // the staged rows it reads and writes: x -> q, attn -> x, x -> act, act -> x, x -> the head's argmax partials
  static const int in[5] = {0, 2, 0, 3, 0}, out[5] = {1, 0, 3, 0, -1};
  const StagedRows s = staged_rows(m);
  a.x = s.buf[in[which]];
  a.x_stride = s.width[in[which]];
  if (which == 4) {   // the head's argmax partials
    a.part_val = m->part_val;
    a.part_idx = m->part_idx;
  } else { a.out = s.buf[out[which]]; a.out_stride = s.width[out[which]]; }
  a.out_dtype = SD_BF16;
  return a;
}

void call_args(GemvArgs& g, const sd_model* m, int T, int M, bool gated, const int32_t* pos_base, int pos_off, const int32_t* bt) {
  g.T = T;
  g.M = M;
  if (gated) { g.skip_k = m->skip_k; g.skip_i = m->skip_i; }
  if (!pos_base) return;
  g.pos_base = pos_base;
  g.pos_off = pos_off;
  g.head_dim = m->cfg.head_dim; g.n_q_heads = m->cfg.n_heads; g.n_kv_heads = m->cfg.n_kv_heads;
  g.max_pos = m->cfg.max_pos;
  g.l_max = m->Lmax;
  g.block_table = bt;
  g.page_shift = m->page_shift;
}

// one pass of forward_pass: the caller's arrays moved to the pass's first row
struct Pass {
  const int32_t* tokens; int tok_stride;
  const int32_t* pos_base; int pos_off;
  int row, Bc, Mc;   // rows [row, row + Bc) of the bound batch, Mc tokens each
  void* logits_out; int logits_dtype, logits_stride, skip_head;
};

// ---- the whole pass as ONE persistent launch (csrc/persist.hip): small passes of a dense-KV Llama model
static int persist_pass(sd_model* m, const Pass& p, hipStream_t st) {
  const sd_model_config& c = m->cfg;
  const int Hkv = c.n_kv_heads, D = c.head_dim;
  PersistArgs pa{};
  pa.ops = m->p_ops;
  pa.n_ops = 4 * c.n_layers + (p.skip_head ? 0 : 1);
  pa.d_model = c.d_model; pa.n_q_heads = c.n_heads; pa.n_kv_heads = Hkv; pa.head_dim = D; pa.d_ff = c.d_ff; pa.vocab = c.vocab;
  pa.n_layers = c.n_layers; pa.max_pos = c.max_pos;
  pa.norm_eps = c.norm_eps;
  pa.attn_scale = 1.0f / sqrtf(static_cast<float>(D));
  pa.tok_emb = c.tok_emb;
  pa.rope_cos = c.rope_cos;
  pa.rope_sin = c.rope_sin;
  pa.tokens = p.tokens; pa.tok_stride = p.tok_stride;
  pa.pos_base = p.pos_base; pa.pos_off = p.pos_off;
  pa.B = p.Bc; pa.M = p.Mc;
  const size_t row_off = static_cast<size_t>(p.row) * Hkv * m->Lmax * D;
  pa.k_cache = m->k_cache + row_off;
  pa.v_cache = m->v_cache + row_off;
  pa.layer_kv = static_cast<size_t>(m->B) * Hkv * m->Lmax * D;
  pa.l_max = m->Lmax;
  pa.logits = p.logits_out; pa.logits_dtype = p.logits_dtype; pa.logits_stride = p.logits_stride;
  pa.part_val = m->part_val;
  pa.part_idx = m->part_idx;
  pa.x = m->x; pa.q = m->q; pa.attn = m->attn; pa.act = m->act;
  pa.gran = m->p_gran;
  pa.gran_parity = m->p_gran_parity;
  pa.sync = m->p_sync;
  pa.host_status = m->host_status;
  pa.skip_k = m->skip_k;
  pa.skip_i = m->skip_i;
  pa.taps = (m->persist_taps || p.skip_head) ? 1 : 0;   // (a pass without the head is run FOR its hidden rows)
  pa.debug_ts = m->p_debug;
  if (int rc = launch_persist_forward(pa, st)) return rc;
  if (!p.skip_head) m->head_grid = kPersistCUs;
  return 0;
}

// ---- the pass as its launches: embedding, five per layer, the head
static int launch_pass(sd_model* m, const Pass& p, hipStream_t st) {
  const sd_model_config& c = m->cfg;
  const int T = p.Bc * p.Mc, Hkv = c.n_kv_heads, D = c.head_dim;
  const bool llama = (c.arch == SD_ARCH_LLAMA);
  EmbedArgs e{};
  e.tok_emb = c.tok_emb;
  e.pos_emb = llama ? nullptr : c.pos_emb;
  e.tokens = p.tokens; e.tok_stride = p.tok_stride;
  e.pos_base = p.pos_base; e.pos_off = p.pos_off;
  e.M = p.Mc;
  e.T = T;
  e.d = c.d_model;
  e.vocab = c.vocab;
  e.max_pos = c.max_pos;
  e.x = m->x;
  e.skip_k = m->skip_k;
  e.skip_i = m->skip_i;
  if (int rc = launch_embed(e, st)) return rc;

  const bool paged = m->block_table != nullptr;
  const size_t layer_kv = paged ? (static_cast<size_t>(m->n_pages) * Hkv * D << m->page_shift) : static_cast<size_t>(m->B) * Hkv * m->Lmax * D;
  const size_t row_kv = paged ? 0 : static_cast<size_t>(p.row) * Hkv * m->Lmax * D;    // paged: rows are found through the table
  const int32_t* bt = paged ? m->block_table + static_cast<size_t>(p.row) * m->max_pages : nullptr;
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
      call_args(g, m, T, p.Mc, true, p.pos_base, p.pos_off, bt);
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
    at.pos_base = p.pos_base;
    at.pos_off = p.pos_off;
    at.B = p.Bc;
    at.M = p.Mc;
    at.n_q_heads = c.n_heads;
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
  if (p.skip_head) return 0;

  // final norm + lm_head with the argmax fused into the epilogue
  GemvArgs h = matrix_args(m, 4 * c.n_layers);
  call_args(h, m, T, p.Mc, true);
  h.out = p.logits_out;
  h.out_stride = p.logits_stride;
  h.out_dtype = p.logits_dtype;
  h.xstat_in = stat_in;
  h.xstat_n = stat_n;
  int ks = 1;
  m->head_grid = gemv_grid(h, &ks);
  return launch_gemv(h, EPI_ARGMAX, st);
}

// one pass: Bc rows x Mc tokens, Bc*Mc <= m->max_t, as the persistent launch where it serves the pass, else as its launches
static int forward_pass(sd_model* m, const int32_t* tokens, int tok_stride, const int32_t* pos_base, int pos_off, int row0, int b0, int Bc, int Mc,
                        int32_t* ids_out, int ids_stride, void* logits_out, int logits_dtype, int logits_stride, int skip_head, hipStream_t st) {
  m->prefill_mc = 0;   // this pass's rows are the model's last: the record of a GEMM-prefill chunk ends here
  const Pass p{tokens + static_cast<size_t>(b0) * tok_stride, tok_stride, pos_base + b0, pos_off, row0 + b0, Bc, Mc,
               logits_out, logits_dtype, logits_stride, skip_head};
  const int T = Bc * Mc;
  if (int rc = persist_pass_ok(m, T, Bc, Mc) ? persist_pass(m, p, st) : launch_pass(m, p, st)) return rc;
  if (skip_head || !ids_out) return 0;
  return launch_argmax_finalize(m->part_val, m->part_idx, T, m->head_grid, Mc, ids_stride, ids_out + static_cast<size_t>(b0) * ids_stride, st,
                                m->skip_k, m->skip_i);
}

// final norm + lm_head + fused argmax over n <= 128 residual rows (bf16 [n][d_model]) -> ids[0..n)
static int head_pass(sd_model* m, const uint16_t* xrows, int n, int32_t* ids, hipStream_t st) {
  GemvArgs h = matrix_args(m, 4 * m->cfg.n_layers);
  call_args(h, m, n, n, false);
  h.x = xrows;
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
    const StagedRows dst = staged_rows(m), src = staged_rows(c, rows);
    for (int i = 0; i < 4; ++i) {
      const size_t w = static_cast<size_t>(dst.width[i]);
      SD_HIP_CHECK(hipMemcpyAsync(dst.buf[i], src.buf[i] + static_cast<size_t>(mc - keep) * w, static_cast<size_t>(keep) * w * 2,
                                  hipMemcpyDeviceToDevice, st));
    }
    if (int rc = on_chunk(m0, mc, rows.x)) return rc;
    m->prefill_rows = rows;
    m->prefill_mc = mc;
  }
  return 0;
}

int model_forward(sd_model* m, const ForwardCall& f, hipStream_t st) {
  SD_REQUIRE(m && m->k_cache && m->x, "forward: model not bound (sd_model_bind)");
  SD_REQUIRE(f.row0 >= 0 && f.B >= 1 && f.row0 + f.B <= m->B, "forward: rows [%d,%d) exceeds bound batch %d", f.row0, f.row0 + f.B, m->B);
  SD_REQUIRE(f.M >= 1, "forward: M=%d", f.M);
  SD_REQUIRE(f.tokens && f.pos_base, "forward: NULL tokens/pos_base");
  const int esz = (f.logits_dtype == SD_F32) ? 4 : 2;
  SD_REQUIRE(!f.logits_out || f.logits_dtype == SD_F32 || f.logits_dtype == SD_BF16, "forward: logits dtype %d", f.logits_dtype);
  const int V = m->cfg.vocab;
  const int cap = (f.B * f.M <= m->small_t) ? m->small_t : m->max_t;  // tokens per pass
  const int backend = prefill_route(m, f.M, f.logits_out != nullptr, st);
  if (backend == SD_PREFILL_PASSES) {
    m->prefill_count[SD_PREFILL_PASSES] += f.B;
  } else if (backend >= 0) {
    for (int b0 = 0; b0 < f.B; ++b0) {
      // ids of the prompt positions: the lm_head over the chunk's rows in groups of at most the model's pass size (the decode-shaped
      // head kernel covers no more: 64 rows for some fp8 heads)
      auto head = [&](int m0, int mc, const uint16_t* xr) -> int {
        if (f.skip_head || !f.ids_out) return 0;
        for (int s0 = 0; s0 < mc; s0 += m->max_t) {
          const int n = (mc - s0 < m->max_t) ? mc - s0 : m->max_t;
          if (int rc = head_pass(m, xr + static_cast<size_t>(s0) * m->cfg.d_model, n, f.ids_out + static_cast<size_t>(b0) * f.ids_stride + m0 + s0, st)) return rc;
        }
        return 0;
      };
      if (int rc = prefill_row(m, backend, f.tokens + static_cast<size_t>(b0) * f.tok_stride, f.pos_base + b0, f.pos_off, f.row0 + b0, f.M, st, head)) return rc;
    }
    m->prefill_count[backend] += f.B;
    return 0;
  }
  if (f.M <= cap) {
    const int Bc = cap / f.M;
    for (int b0 = 0; b0 < f.B; b0 += Bc) {
      const int nb = (f.B - b0 < Bc) ? f.B - b0 : Bc;
      void* lo = f.logits_out ? static_cast<char*>(f.logits_out) + static_cast<size_t>(b0) * f.M * V * esz : nullptr;
      if (int rc = forward_pass(m, f.tokens, f.tok_stride, f.pos_base, f.pos_off, f.row0, b0, nb, f.M, f.ids_out, f.ids_stride, lo,
                                f.logits_dtype, V, f.skip_head, st))
        return rc;
    }
    return 0;
  }
  // long M (prefill): chunks of `cap` positions, one row at a time, in position order
  for (int b0 = 0; b0 < f.B; ++b0) {
    for (int m0 = 0; m0 < f.M; m0 += cap) {
      const int mc = (f.M - m0 < cap) ? f.M - m0 : cap;
      void* lo = f.logits_out ? static_cast<char*>(f.logits_out) + (static_cast<size_t>(b0) * f.M + m0) * V * esz : nullptr;
      if (int rc = forward_pass(m, f.tokens + m0, f.tok_stride, f.pos_base, f.pos_off + m0, f.row0, b0, 1, mc,
                                f.ids_out ? f.ids_out + m0 : nullptr, f.ids_stride, lo, f.logits_dtype, V, f.skip_head, st))
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

extern "C" int sd_model_forward(sd_model* m, const int32_t* tokens, int tok_stride, const int32_t* pos_base,
                                int pos_off, int row0, int B, int M, int32_t* ids_out, int ids_stride, void* logits_out,
                                int logits_dtype, int skip_head, void* stream) {
  clear_error();
  const ForwardCall f{tokens, tok_stride, pos_base, pos_off, row0, B, M, ids_out, ids_stride, logits_out, logits_dtype, skip_head};
  return model_forward(m, f, static_cast<hipStream_t>(stream));
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
