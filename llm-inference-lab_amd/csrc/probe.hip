// Measurement hooks and row read-backs of a bound model: sd_model_probe_gemv (one GEMV of the forward, with its optional timeline),
// sd_model_probe_forward (whole forwards), and the staged rows a pass or a GEMM-prefill chunk left (sd_model_hidden_rows,
// sd_model_debug_rows, sd_model_prefill_rows). The forward they launch is csrc/engine.hip. Host-side C++ behind the C-ABI.

#include <hip/hip_runtime.h>

#include <stdlib.h>

#include <vector>

#include "engine.h"

namespace sd {

// what a probe creates and must release on every way out
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};
struct DeviceWords { unsigned long long* p = nullptr; ~DeviceWords() { if (p) (void)hipFree(p); } };

// launch(i) for i in [0, warmup + iters) on `st`, the last `iters` of them between two events: their mean in us
template <class Launch>
static int timed_launches(Launch&& launch, int warmup, int iters, hipStream_t st, float* avg_usec) {
  EventPair ev;
  SD_HIP_CHECK(hipEventCreate(&ev.e0));
  SD_HIP_CHECK(hipEventCreate(&ev.e1));
  for (int i = 0; i < warmup; ++i)
    if (int rc = launch(i)) return rc;
  SD_HIP_CHECK(hipEventRecord(ev.e0, st));
  for (int i = 0; i < iters; ++i)
    if (int rc = launch(i + warmup)) return rc;
  SD_HIP_CHECK(hipEventRecord(ev.e1, st));
  SD_HIP_CHECK(hipEventSynchronize(ev.e1));
  float ms = 0.f;
  SD_HIP_CHECK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  *avg_usec = ms * 1000.0f / iters;
  return 0;
}

// stamps of the LAST launch of sd_model_probe_gemv: offsets from the earliest workgroup entry, in us
static int print_gemv_timeline(const unsigned long long* dbg, int which, int T) {
  std::vector<unsigned long long> h(256 * 8);
  SD_HIP_CHECK(hipMemcpy(h.data(), dbg, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
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
  return 0;
}

// n rows from row0 of staged buffer `which` (engine.h StagedRows) -> out, on `stream`
static int read_rows(const char* who, const StagedRows& s, int which, int row0, int n, void* out, void* stream) {
  SD_REQUIRE(which >= 0 && which <= 3, "%s: which=%d (0 x, 1 q, 2 attn, 3 act)", who, which);
  const size_t w = static_cast<size_t>(s.width[which]);
  SD_HIP_CHECK(hipMemcpyAsync(out, s.buf[which] + static_cast<size_t>(row0) * w, static_cast<size_t>(n) * w * 2, hipMemcpyDeviceToDevice,
                              static_cast<hipStream_t>(stream)));
  return 0;
}

// the checks sd_model_hidden_rows and sd_model_debug_rows share, then the rows of the model's last pass
static int pass_rows(const char* who, sd_model* m, int which, int row0, int n, void* out, void* stream) {
  SD_REQUIRE(m && m->x && out, "%s: NULL argument / model not bound", who);
  SD_REQUIRE(row0 >= 0 && n >= 1 && row0 + n <= kSkinnyMaxT, "%s: rows [%d,%d) outside the %d rows of a pass", who, row0, row0 + n, kSkinnyMaxT);
  return read_rows(who, staged_rows(m), which, row0, n, out, stream);
}

}  // namespace sd

// ============================================================================ C-ABI
using namespace sd;

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
  DeviceWords dbg;
  const bool timeline = getenv(debug_env::kGemvTimeline) != nullptr;
  if (timeline) {
    SD_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dbg.p), 256 * 16 * sizeof(unsigned long long)));
    SD_HIP_CHECK(hipMemset(dbg.p, 0, 256 * 16 * sizeof(unsigned long long)));
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
    g.debug_ts = dbg.p;
    g.norm_eps = c.norm_eps;
    if (use_xstat && g.prologue != PRO_NONE) { g.xstat_in = m->xstat; g.xstat_n = 256; }
    call_args(g, m, T, T, false, which == 0 ? m->probe_pos : nullptr);
    if (which == 0) {  // QKV: + RoPE + in-place KV append (row 0 of the cache, positions 0..T-1)
      g.rope_cos = c.arch == SD_ARCH_LLAMA ? c.rope_cos : nullptr; g.rope_sin = c.arch == SD_ARCH_LLAMA ? c.rope_sin : nullptr;
      const size_t layer_kv = static_cast<size_t>(m->B) * c.n_kv_heads * m->Lmax * c.head_dim;
      g.k_cache = m->k_cache + li * layer_kv; g.v_cache = m->v_cache + li * layer_kv;
    }
    if (use_xstat && sh.epi == EPI_RESID && gemm_resid_publishes_stats(g)) g.xstat_out = m->xstat;
    return launch_gemv(g, sh.epi, st);
  };
  if (int rc = timed_launches(launch, 3, iters, st, avg_usec)) return rc;
  double bytes = 2.0 * sh.N * sh.K;
  if (m->w8()) bytes *= 0.5;  // one byte per weight
  *bytes_per_launch = bytes;
  return timeline ? print_gemv_timeline(dbg.p, which, T) : 0;
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
  ForwardCall f;   // one row of M tokens at positions pos0.., no ids and no logits out
  f.tokens = f.pos_base = zeros;
  f.tok_stride = f.M = M;
  f.pos_off = pos0;
  f.skip_head = skip_head;
  auto fwd = [&](int = 0) { return model_forward(m, f, st); };
  if (int rc = timed_launches(fwd, 2, iters, st, avg_usec)) return rc;
  double per_layer = 0;
  for (int i = 0; i < 4; ++i) per_layer += 2.0 * matrix_shape(c, i).N * matrix_shape(c, i).K;
  double bytes = per_layer * c.n_layers + (skip_head ? 0.0 : 2.0 * matrix_shape(c, 4).N * matrix_shape(c, 4).K);
  if (m->w8()) bytes *= 0.5;
  *bytes_per_forward = bytes;
  if (timeline && m->persist_t >= M) {
    const size_t n_ops = static_cast<size_t>(4 * c.n_layers + (skip_head ? 0 : 1));
    const size_t words = static_cast<size_t>(kPersistCUs) * (12 * n_ops + 4);
    SD_REQUIRE(timeline_cap >= words, "probe_forward: timeline needs %zu words", words);
    DeviceWords dbg;
    SD_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dbg.p), words * 8));
    SD_HIP_CHECK(hipMemsetAsync(dbg.p, 0, words * 8, st));
    m->p_debug = dbg.p;
    const int rc = fwd();
    m->p_debug = nullptr;
    if (rc) return rc;
    SD_HIP_CHECK(hipStreamSynchronize(st));
    SD_HIP_CHECK(hipMemcpy(timeline, dbg.p, words * 8, hipMemcpyDeviceToHost));
  }
  return 0;
}

extern "C" int sd_model_hidden_rows(sd_model* m, int row0, int n, void* out, void* stream) {
  clear_error();
  return pass_rows("hidden_rows", m, 0, row0, n, out, stream);
}

extern "C" int sd_model_debug_rows(sd_model* m, int which, int row0, int n, void* out, void* stream) {
  clear_error();
  return pass_rows("debug_rows", m, which, row0, n, out, stream);
}

extern "C" int sd_model_prefill_rows(sd_model* m, int which, int row0, int n, void* out, void* stream) {
  clear_error();
  SD_REQUIRE(m && out, "prefill_rows: NULL argument");
  SD_REQUIRE(m->prefill_mc > 0, "prefill_rows: no GEMM-prefill chunk on record (the model's last forward was not one, or it was bound since)");
  SD_REQUIRE(row0 >= 0 && n >= 1 && n <= m->prefill_mc && row0 <= m->prefill_mc - n, "prefill_rows: %d rows from row %d are outside the %d rows of the last chunk",
             n, row0, m->prefill_mc);
  return read_rows("prefill_rows", staged_rows(m->cfg, m->prefill_rows), which, row0, n, out, stream);
}
