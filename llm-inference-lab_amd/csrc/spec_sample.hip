// Speculative sampling inside the step: the draft's tokens are DRAWN from the draft's distribution, the target accepts
// d_{i+1} with probability min(1, p_i(d_{i+1}) / q_i(d_{i+1})), the first rejected position is redrawn from
// normalise(max(0, p - q)) and a full acceptance draws the bonus token from p_K (Leviathan et al. 2023, Chen et al. 2023).
// The emitted sequence is then distributed exactly as sampling from softmax(target bf16 logits / T), whatever the draft is.
//
// All distributions are softmax(x / T) over the STORED bf16 logits of the respective forward, in float64 (x / T with T the
// float32 temperature widened to double; no division when T == 1, as csrc/sample.hip). Draw schedule of row b in a step
// that starts with draw counter c (Philox4x32-10, key = seed, stream sid = stream_ids[b] or b), restated on the CPU in
// tests/spec_sample_ref.py:
//   d_{i+1}, i = 0..K-1 : Gumbel-max over q_i / T, counter (c + i, sid, element, kTagGumbel)   (= sample_gumbel_kernel)
//   u_i,     i = 0..K-1 : counter (c + i, sid, 0, kTagCdf), u = r0 * 2^-32                       (= draw_uniform)
//   next token          : Gumbel-max over log-weights, counter (c + K, sid, element, kTagGumbel)
//   the row's counter advances by K + 1; rows with active[b] == 0 consume nothing.
// The three kinds are independent: different tags (uniform / Gumbel) or different counters (c + i, i < K / c + K).
//   ratio_i = exp((p_i[d]/T - lse(p_i/T)) - (q_i[d]/T - lse(q_i/T))),  lse(v) = max v + log(sum exp(v - max v))
//   a       = number of leading i with u_i < ratio_i
//   next    = a < K: Gumbel-max over log(r_v), r_v = exp(p_a[v]/T - lse p) - exp(q_a[v]/T - lse q), over the v with r_v > 0
//                    (no such v — q == p: over p_a[v]/T);  a == K: Gumbel-max over p_K[v]/T.
// The sums of the two log-sum-exps are the only order-dependent quantities; p and q of a position go through the same
// code in the same order, so bitwise equal rows give ratio exactly 1 and an all-zero residual.
// Non-finite logits: a position whose p or q row holds a NaN, or whose row maximum is not finite (+inf present, or every
// entry -inf), is REJECTED (ratio = NaN) and its candidate is the plain Gumbel-max over p_i / T with the ordering of
// sample_gumbel_kernel (NaN scores first, then value, then lowest index). -inf entries of otherwise finite rows have
// probability 0 on either side.
//
// Three kernels, ordinary stream order between them, no allocation, graph-capturable:
//   spec_draft_draw_kernel  one 1024-thread workgroup per row: reads the logits row the draft's lm_head has just stored,
//                           keeps it as row q_i of the [B][K][V] buffer, draws d_{i+1}, hands it to the next draft
//                           forward and to the verify input (the sampled counterpart of draft_finalize_kernel)
//   spec_stats_kernel       grid (K+1, B): position i of row b, independent of the accept length — the two log-sum-exps,
//                           ratio_i and the flag u_i < ratio_i, then the candidate next token of position i
//   spec_accept_kernel      one wave per row: accept length = leading flags, next token = candidate of that position
//
// SHAPED variant (sd_specdec_set_spec_shaping, sd_spec_sample_accept_shaped): both distributions of every position are the
// temperature -> top-k -> top-p distribution of their row, exactly as sd_sample_token / oracle/sampling_ref.py:
// filtered_distribution define it, and the emitted tokens are distributed as the target's own
// sd_sample_token(temperature, top_k, top_p) sampling, whatever the draft is. top_k in 1..1024 (clamped to V), with or without
// top_p < 1; top_p WITHOUT top_k (the full-vocabulary nucleus) is refused. Restated on the CPU in tests/spec_shape_ref.py.
// For a bf16 row x, S(x) = the kept ids in sorted order (value descending, index ascending: the 52-bit composite key), float64
// weights e_j = exp(x_j / T - max), Z = their sum added sequentially in sorted order; a row whose top value is not finite is
// the point mass on its first id (so the shaped mode has no "rejected non-finite position" path). x'(v) = e(v) / Z on the kept
// set, 0 elsewhere. Row b, draw counter c at the start of the step, Philox counter words (draw, stream, element, tag):
//   1. d_{i+1}, i = 0..K-1 : the uniform of counter (c + i, sid, 0, kTagCdf) inverted through S(q_i) in sorted order — exactly
//                            the token sd_sample_token draws from q_i with draw index c + i
//   2. u_i,     i = 0..K-1 : counter (c + i, sid, 0, kTagAccept) — a tag of its own: (c + i, .., kTagCdf) is the draw of 1.
//   3. ratio_i = (e_p(d) / Z_p) / (e_q(d) / Z_q), d = d_{i+1}; e_p(d) = 0 when d is outside the target's kept set (ratio 0:
//      rejected). p and q go through the same code in the same order: bitwise equal rows give ratio exactly 1.0. A d outside
//      q's kept set can only come from a caller of the stand-alone op: ratio NaN, rejected. a = leading i with u_i < ratio_i
//   4. next token, uniform u_n of counter (c + K, sid, 0, kTagCdf):
//        a < K : weights r_j = max(0, p'_a(id_j) - q'_a(id_j)) over the TARGET's kept ids in the target's sorted order, Z_r
//                summed sequentially, the first j with u_n * Z_r < cum_j (the last kept id otherwise); Z_r == 0 (q' >= p' on
//                p's support, i.e. equal): the same inversion through e_p — sd_sample_token on p_a with draw c + K
//        a == K: sd_sample_token on p_K with draw c + K
//   5. emitted d_1..d_a + the next token; the counter advances by K + 1; inactive rows consume nothing.
// No launch of the shaped step evaluates a Philox block or a logarithm per vocabulary element:
//   spec_draft_draw_shaped_kernel  one workgroup per row: copies the row to q[b][i], row_survivors (sample_device.h — the kept
//                                  set sample_topk_kernel uses), inverts the uniform of 1., hands d_{i+1} over
//   spec_stats_shaped_kernel       grid (K+1, B): the kept sets of q_i (re-selected from the stored row) and p_i, the lookup
//                                  of d in both, ratio and flag, q' looked up for each of p's <= 1024 ids, the residual walk
//   spec_accept_kernel             unchanged
//
// PER-ROW parameters (sd_spec_sample_accept_rows, sd_specdec_set_row_sampling): spec_draft_draw_rows_kernel and
// spec_stats_rows_kernel read row b's sd_row_sampling entry, normalise it for speculative sampling (normalise_row_sampling,
// sample_device.h: the full-vocabulary nucleus is a greedy row here) and run the unshaped body for a row without top_k and
// top_p, the shaped body for any other — each row the draw schedule of its scalar mode; spec_accept_kernel is unchanged.

#include "engine.h"
#include "sample_device.h"

namespace sd {

constexpr int kSpecWaves = kSampleThreads / kWave;

// f(p value, q value, index) over two bf16 rows of V elements, 16-byte loads when both allow it
// (spec_agree.hip's for_each_pair_slice visits in another order on unaligned rows; each file's float64 sums need its own: two walkers)
template <typename F>
__device__ __forceinline__ void for_each_pair(const uint16_t* rp, const uint16_t* rq, int V, int tid, F&& f) {
  const bool aligned = ((reinterpret_cast<uintptr_t>(rp) | reinterpret_cast<uintptr_t>(rq)) & 15) == 0;
  if (aligned && (V & 7) == 0) {
    const uint4* p = reinterpret_cast<const uint4*>(rp);
    const uint4* q = reinterpret_cast<const uint4*>(rq);
    for (int v = tid; v < (V >> 3); v += kSampleThreads) {
      const uint4 a = p[v], b = q[v];
      const uint32_t wa[4] = {a.x, a.y, a.z, a.w}, wb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f(__uint_as_float(wa[j] << 16), __uint_as_float(wb[j] << 16), 8 * v + 2 * j);
        f(__uint_as_float(wa[j] & 0xffff0000u), __uint_as_float(wb[j] & 0xffff0000u), 8 * v + 2 * j + 1);
      }
    }
  } else {
    for (int i = tid; i < V; i += kSampleThreads) f(bf16_bits_to_float(rp[i]), bf16_bits_to_float(rq[i]), i);
  }
}

// ---------------------------------------------------------------------------------------------- draft draw + hand-over
struct SpecDrawArgs {
  const uint16_t* src;   // logits rows of the draft forward just run: entry b's row is b * src_rows_per_b + src_row
  int src_rows_per_b, src_row;
  uint16_t* q;           // [B][K][V]: row (b, i) receives a copy
  int i, V;
  float temperature;
  uint32_t seed_lo, seed_hi;
  const uint32_t* draw;  // [B] counters at the start of the step (read only here)
  const int32_t* stream_id;
};

// The bodies of the draw and statistics kernels, unshaped and shaped, as device functions on an LDS block of their caller: the
// scalar kernels call them with the launch's parameters, the _rows kernels with the row's own (temperature and seed in the
// argument block, the shape beside it).
struct SpecArgBestLds {
  double sv[kSpecWaves];
  int si[kSpecWaves];
};

__device__ __forceinline__ void spec_draft_draw_row(SpecArgBestLds& G, const SpecDrawArgs& a, const SpecState& s, int b) {
  double* const sv = G.sv;
  int* const si = G.si;
  const int tid = threadIdx.x, V = a.V;
  const uint16_t* src = a.src + (static_cast<size_t>(b) * a.src_rows_per_b + a.src_row) * V;
  uint16_t* dst = a.q + (static_cast<size_t>(b) * s.K + a.i) * V;
  const double T = static_cast<double>(a.temperature);
  const bool scale = a.temperature != 1.0f;
  const uint32_t c = a.draw[b] + static_cast<uint32_t>(a.i);
  const uint32_t sid = a.stream_id ? static_cast<uint32_t>(a.stream_id[b]) : static_cast<uint32_t>(b);
  double bv = -INFINITY;
  int bi = 0x7fffffff;
  copy_and_visit_bf16_row(src, dst, V, tid, [&](float x, int i) {
    double v = static_cast<double>(x);
    if (scale) v = v / T;
    const double sc = v + gumbel_noise(c, sid, i, a.seed_lo, a.seed_hi);
    if (better_d(sc, i, bv, bi)) { bv = sc; bi = i; }
  });
  block_arg_best<kSpecWaves, double, better_d>(bv, bi, sv, si);
  if (tid == 0) {
    const int d = bi;   // always a valid index: V >= 1 and the first element visited beats the initial (-inf, INT_MAX)
    s.draft_tok[b * s.K + a.i] = d;
    s.verify_tok[b * (s.K + 1) + a.i + 1] = d;
    s.next_tok[b] = d;
  }
}

__global__ __launch_bounds__(kSampleThreads) void spec_draft_draw_kernel(const SpecDrawArgs a, SpecState s) {
  __shared__ SpecArgBestLds G;
  spec_draft_draw_row(G, a, s, blockIdx.x);
}

static SpecDrawArgs spec_draw_args(const void* src, int src_rows_per_b, int src_row, void* q, int i, int V, const DrawSpec& d) {
  SpecDrawArgs a{};
  a.src = static_cast<const uint16_t*>(src);
  a.src_rows_per_b = src_rows_per_b;
  a.src_row = src_row;
  a.q = static_cast<uint16_t*>(q);
  a.i = i;
  a.V = V;
  a.temperature = d.temperature;
  a.seed_lo = seed_lo32(d.seed);
  a.seed_hi = seed_hi32(d.seed);
  a.draw = d.draw;
  a.stream_id = d.stream_id;
  return a;
}

// ---------------------------------------------------------------------------------- per-position statistics and candidate
struct SpecStatArgs {
  const uint16_t* P;          // [B][K+1][V] target logits
  const uint16_t* Q;          // [B][K][V] draft logits
  const int32_t* draft_ids;   // [B][K]
  int K, V;
  float temperature;
  uint32_t seed_lo, seed_hi;
  const uint32_t* draw;       // nullable: [B] counters at the start of the step
  uint32_t draw0;
  const int32_t* stream_id;
  const int32_t* active;
  int32_t* flag;              // [B][K+1] (slot K unused)
  int32_t* cand;              // [B][K+1]
  double* ratios;             // nullable [B][K]
};

struct SpecStatsLds {
  double sh[kSpecWaves];
  double sv[kSpecWaves];
  int si[kSpecWaves];
};

__device__ __forceinline__ void spec_stats_row(SpecStatsLds& G, const SpecStatArgs& a, int i, int b) {
  double* const sh = G.sh;
  double* const sv = G.sv;
  int* const si = G.si;
  const int tid = threadIdx.x, K = a.K, V = a.V;
  if (a.active && a.active[b] == 0) return;
  const uint16_t* rp = a.P + (static_cast<size_t>(b) * (K + 1) + i) * V;
  const uint16_t* rq = i < K ? a.Q + (static_cast<size_t>(b) * K + i) * V : rp;   // position K has no q row
  const double T = static_cast<double>(a.temperature);
  const bool scale = a.temperature != 1.0f;
  const uint32_t c0 = a.draw ? a.draw[b] : a.draw0;
  const uint32_t sid = a.stream_id ? static_cast<uint32_t>(a.stream_id[b]) : static_cast<uint32_t>(b);
  auto scaled = [&](float x) {
    const double v = static_cast<double>(x);
    return scale ? v / T : v;
  };

  // ---- pass 1: maxima and log-sum-exps of both rows, the ratio, the flag
  bool residual = false;
  double lse_p = 0.0, lse_q = 0.0;
  if (i < K) {
    double mp = -INFINITY, mq = -INFINITY;
    int nan = 0;
    for_each_pair(rp, rq, V, tid, [&](float xp, float xq, int) {
      const double vp = scaled(xp), vq = scaled(xq);
      nan |= (vp != vp) | (vq != vq);
      mp = fmax(mp, vp);
      mq = fmax(mq, vq);
    });
    // sh is reused from reduction to reduction: a barrier between two uses (the __syncthreads_or is one)
    mp = block_max_d<kSpecWaves>(mp, sh);
    __syncthreads();
    mq = block_max_d<kSpecWaves>(mq, sh);
    const bool bad = __syncthreads_or(nan) || !is_finite_d(mp) || !is_finite_d(mq);
    if (!bad) {
      double sp = 0.0, sq = 0.0;
      for_each_pair(rp, rq, V, tid, [&](float xp, float xq, int) {
        sp += exp(scaled(xp) - mp);
        sq += exp(scaled(xq) - mq);
      });
      sp = block_sum_d<kSpecWaves>(sp, sh);
      __syncthreads();
      sq = block_sum_d<kSpecWaves>(sq, sh);
      lse_p = mp + log(sp);
      lse_q = mq + log(sq);
      residual = true;
    }
    if (tid == 0) {
      int d = a.draft_ids[b * K + i];
      d = d < 0 ? 0 : (d >= V ? V - 1 : d);
      double ratio = NAN;
      if (!bad) ratio = exp((scaled(bf16_bits_to_float(rp[d])) - lse_p) - (scaled(bf16_bits_to_float(rq[d])) - lse_q));
      const double u = philox_uniform(c0 + static_cast<uint32_t>(i), sid, kTagCdf, a.seed_lo, a.seed_hi);
      a.flag[b * (K + 1) + i] = (u < ratio) ? 1 : 0;
      if (a.ratios) a.ratios[b * K + i] = ratio;
    }
  }

  // ---- pass 2: the candidate next token of this position
  const uint32_t cn = c0 + static_cast<uint32_t>(K);
  double rv = -INFINITY, pv = -INFINITY;
  int ri = 0x7fffffff, pi = 0x7fffffff;
  for_each_pair(rp, rq, V, tid, [&](float xp, float xq, int idx) {
    const double vp = scaled(xp);
    const double g = gumbel_noise(cn, sid, idx, a.seed_lo, a.seed_hi);
    const double s_p = vp + g;
    if (better_d(s_p, idx, pv, pi)) { pv = s_p; pi = idx; }
    if (residual) {
      const double r = exp(vp - lse_p) - exp(scaled(xq) - lse_q);
      if (r > 0.0) {
        const double s_r = log(r) + g;
        if (better_d(s_r, idx, rv, ri)) { rv = s_r; ri = idx; }
      }
    }
  });
  block_arg_best<kSpecWaves, double, better_d>(pv, pi, sv, si);
  if (residual) {   // (workgroup-uniform)
    __syncthreads();   // thread 0 is done with sv / si
    block_arg_best<kSpecWaves, double, better_d>(rv, ri, sv, si);
  }
  if (tid == 0) a.cand[b * (K + 1) + i] = (residual && ri != 0x7fffffff) ? ri : pi;
}

__global__ __launch_bounds__(kSampleThreads) void spec_stats_kernel(const SpecStatArgs a) {
  __shared__ SpecStatsLds G;
  spec_stats_row(G, a, blockIdx.x, blockIdx.y);
}

// ------------------------------------------------------------------------------------------------------------- accept
struct SpecAcceptArgs {
  const int32_t* flag;
  const int32_t* cand;
  int K;
  const int32_t* active;
  uint32_t* draw;          // nullable: advanced by K + 1 for active rows
  int32_t* accept_len;     // [B]
  int32_t* next_tok;       // [B]
};

__global__ __launch_bounds__(kWave) void spec_accept_kernel(const SpecAcceptArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x, K = a.K;
  if (a.active && a.active[b] == 0) {   // the row's step does not count: nothing accepted, nothing drawn
    if (lane == 0) a.accept_len[b] = 0;
    return;
  }
  const bool ok = (lane < K) && a.flag[b * (K + 1) + lane] != 0;
  const unsigned long long m64 = __ballot(ok);
  const unsigned long long valid = (1ull << K) - 1ull;
  const unsigned long long miss = (~m64) & valid;
  const int acc = miss ? __builtin_ctzll(miss) : K;
  if (lane == 0) {
    a.accept_len[b] = acc;
    a.next_tok[b] = a.cand[b * (K + 1) + acc];
    if (a.draw) a.draw[b] = a.draw[b] + static_cast<uint32_t>(K + 1);
  }
}

// flag / cand: [B][K+1] each; the step passes draw0 = 0 and no ratios, the stand-alone ops their caller's
static SpecStatArgs spec_stat_args(const void* target_logits, const void* draft_logits, const int32_t* draft_ids, int K, int V,
                                   const DrawSpec& d, const int32_t* active, int32_t* flag, int32_t* cand, double* ratios) {
  SpecStatArgs sa{};
  sa.P = static_cast<const uint16_t*>(target_logits);
  sa.Q = static_cast<const uint16_t*>(draft_logits);
  sa.draft_ids = draft_ids;
  sa.K = K;
  sa.V = V;
  sa.temperature = d.temperature;
  sa.seed_lo = seed_lo32(d.seed);
  sa.seed_hi = seed_hi32(d.seed);
  sa.draw = d.draw;
  sa.draw0 = d.draw0;
  sa.stream_id = d.stream_id;
  sa.active = active;
  sa.flag = flag;
  sa.cand = cand;
  sa.ratios = ratios;
  return sa;
}

// ------------------------------------------------------------------------------------------ shaped variant (top-k / top-p)
struct SpecShape {
  int top_k;      // 1..kSampleMaxK after the clamp to V
  float top_p;    // >= 1: no nucleus cut
};

static int check_spec_shape(const char* who, int top_k, float top_p) {
  SD_REQUIRE(top_p == top_p && top_p > 0.f, "%s: top_p %g (must be > 0)", who, top_p);
  SD_REQUIRE(top_k > 0, "%s: top_p = %g without top_k (the full-vocabulary nucleus) is not supported; give a top_k in 1..%d", who,
             top_p, kSampleMaxK);
  SD_REQUIRE(top_k <= kSampleMaxK, "%s: top_k=%d > %d is not supported", who, top_k, kSampleMaxK);
  return 0;
}

__device__ __forceinline__ void spec_draft_draw_shaped_row(SurvivorLds& L, const SpecDrawArgs& a, const SpecShape& sh, const SpecState& s, int b) {
  const int tid = threadIdx.x, V = a.V;
  const uint16_t* src = a.src + (static_cast<size_t>(b) * a.src_rows_per_b + a.src_row) * V;
  uint16_t* dst = a.q + (static_cast<size_t>(b) * s.K + a.i) * V;
  copy_and_visit_bf16_row(src, dst, V, tid, [](float, int) {});
  row_survivors(L, src, SD_BF16, V, min(sh.top_k, V), a.temperature, sh.top_p);
  if (tid == 0) {
    const uint32_t c = a.draw[b] + static_cast<uint32_t>(a.i);
    const uint32_t sid = a.stream_id ? static_cast<uint32_t>(a.stream_id[b]) : static_cast<uint32_t>(b);
    const int d = static_cast<int>(L.sel[invert_weights(L.ev, L.n_keep, L.z, philox_uniform(c, sid, kTagCdf, a.seed_lo, a.seed_hi))]);
    s.draft_tok[b * s.K + a.i] = d;
    s.verify_tok[b * (s.K + 1) + a.i + 1] = d;
    s.next_tok[b] = d;
  }
}

__global__ __launch_bounds__(kSampleThreads) void spec_draft_draw_shaped_kernel(const SpecDrawArgs a, const SpecShape sh, SpecState s) {
  __shared__ SurvivorLds L;
  spec_draft_draw_shaped_row(L, a, sh, s, blockIdx.x);
}

// Per-row parameters: the row's entry, normalised for speculative sampling, written over the launch's temperature and seed;
// returns the row's shape (top_k == 0: the unshaped statistics).
template <typename Args>
__device__ __forceinline__ SpecShape spec_row_params(Args& a, const sd_row_sampling* table, int b) {
  const sd_row_sampling e = normalise_row_sampling(table, b, a.V, true);
  a.temperature = e.temperature;
  a.seed_lo = e.seed_lo;
  a.seed_hi = e.seed_hi;
  return SpecShape{e.top_k, e.top_p};
}

// one path runs per workgroup: the LDS blocks of the two overlay each other
union SpecDrawRowsLds {
  SpecArgBestLds plain;
  SurvivorLds shaped;
};

__global__ __launch_bounds__(kSampleThreads) void spec_draft_draw_rows_kernel(const SpecDrawArgs a0, const sd_row_sampling* table, SpecState s) {
  __shared__ SpecDrawRowsLds U;
  const int b = blockIdx.x;
  SpecDrawArgs a = a0;
  const SpecShape sh = spec_row_params(a, table, b);
  if (sh.top_k > 0) spec_draft_draw_shaped_row(U.shaped, a, sh, s, b);
  else spec_draft_draw_row(U.plain, a, s, b);
}

// the draw + hand-over after a draft forward; top_k == 0: spec_draft_draw_kernel, else the shaped kernel; with a table the row
// kernel, whatever the scalars say
int launch_spec_draft_draw(const SpecState& s, const void* src, int src_rows_per_b, int src_row, void* q, int i, int V, const DrawSpec& d,
                           hipStream_t st) {
  SD_REQUIRE(src && q && d.draw, "spec_draft_draw: NULL buffer");
  const SpecDrawArgs a = spec_draw_args(src, src_rows_per_b, src_row, q, i, V, d);
  if (d.table) {
    SD_REQUIRE(i >= 0 && i < s.K && V >= 1 && V <= (1 << kIdxBits) && src_rows_per_b >= 1 && src_row >= 0 && src_row < src_rows_per_b,
               "spec_draft_draw: i=%d V=%d row %d of %d", i, V, src_row, src_rows_per_b);
    SD_REQUIRE((reinterpret_cast<uintptr_t>(d.table) & 15) == 0, "spec_draft_draw: the row table must be 16-byte aligned");
    hipLaunchKernelGGL(spec_draft_draw_rows_kernel, dim3(s.B), dim3(kSampleThreads), 0, st, a, d.table, s);
    SD_LAUNCH_CHECK();
    return 0;
  }
  SD_REQUIRE(i >= 0 && i < s.K && V >= 1 && (d.top_k <= 0 || V <= (1 << kIdxBits)) && src_rows_per_b >= 1 && src_row >= 0 &&
                 src_row < src_rows_per_b, "spec_draft_draw: i=%d V=%d row %d of %d", i, V, src_row, src_rows_per_b);
  if (d.top_k > 0) {
    if (int rc = check_spec_shape("spec_draft_draw", d.top_k, d.top_p)) return rc;
    hipLaunchKernelGGL(spec_draft_draw_shaped_kernel, dim3(s.B), dim3(kSampleThreads), 0, st, a, SpecShape{d.top_k, d.top_p}, s);
  } else {
    hipLaunchKernelGGL(spec_draft_draw_kernel, dim3(s.B), dim3(kSampleThreads), 0, st, a, s);
  }
  SD_LAUNCH_CHECK();
  return 0;
}

// position i of row b: flag + ratio (i < K) and the candidate next token. Static LDS: the survivor block (48 KB) + q's kept set
// (12 KB); q's weights are overwritten by the residual once every lookup of q' has been made.
struct SpecShapedLds {
  SurvivorLds L;
  double qe[kSampleMaxK];
  int qi[kSampleMaxK];
  double s_ep, s_eq;
  int s_in_q;
};

__device__ __forceinline__ void spec_stats_shaped_row(SpecShapedLds& G, const SpecStatArgs& a, const SpecShape& sh, int i, int b) {
  SurvivorLds& L = G.L;
  double* const qe = G.qe;
  int* const qi = G.qi;
  double &s_ep = G.s_ep, &s_eq = G.s_eq;
  int& s_in_q = G.s_in_q;
  const int tid = threadIdx.x, K = a.K, V = a.V;
  if (a.active && a.active[b] == 0) return;
  const uint16_t* rp = a.P + (static_cast<size_t>(b) * (K + 1) + i) * V;
  const int k = min(sh.top_k, V);
  const uint32_t c0 = a.draw ? a.draw[b] : a.draw0;
  const uint32_t sid = a.stream_id ? static_cast<uint32_t>(a.stream_id[b]) : static_cast<uint32_t>(b);
  int nq = 0;
  double zq = 1.0;
  if (i < K) {   // (workgroup-uniform) the kept set of q_i, parked in qi / qe
    row_survivors(L, a.Q + (static_cast<size_t>(b) * K + i) * V, SD_BF16, V, k, a.temperature, sh.top_p);
    nq = L.n_keep;
    zq = L.z;
    if (tid < nq) {
      qi[tid] = static_cast<int>(L.sel[tid]);
      qe[tid] = L.ev[tid];
    }
    if (tid == 0) { s_ep = 0.0; s_eq = 0.0; s_in_q = 0; }
    __syncthreads();
  }
  row_survivors(L, rp, SD_BF16, V, k, a.temperature, sh.top_p);   // the kept set of p_i stays in L
  const int np = L.n_keep;
  const double zp = L.z;
  if (i < K) {
    // the drawn token in both kept sets (ids are unique inside a set: at most one thread writes each word)
    const int d = a.draft_ids[b * K + i];
    if (tid < np && static_cast<int>(L.sel[tid]) == d) s_ep = L.ev[tid];
    if (tid < nq && qi[tid] == d) { s_eq = qe[tid]; s_in_q = 1; }
    // residual weight of the target's j-th kept id
    double r = 0.0;
    if (tid < np) {
      const int id = static_cast<int>(L.sel[tid]);
      double eq = 0.0;
      for (int t = 0; t < nq; ++t)
        if (qi[t] == id) { eq = qe[t]; break; }
      r = L.ev[tid] / zp - eq / zq;
      r = r > 0.0 ? r : 0.0;
    }
    __syncthreads();
    if (tid < np) qe[tid] = r;
    if (tid == 0) {
      const double ratio = s_in_q ? (s_ep / zp) / (s_eq / zq) : NAN;
      const double u = philox_uniform(c0 + static_cast<uint32_t>(i), sid, kTagAccept, a.seed_lo, a.seed_hi);
      a.flag[b * (K + 1) + i] = (u < ratio) ? 1 : 0;
      if (a.ratios) a.ratios[b * K + i] = ratio;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double un = philox_uniform(c0 + static_cast<uint32_t>(K), sid, kTagCdf, a.seed_lo, a.seed_hi);
    int pick = -1;
    if (i < K) {
      double zr = 0.0;
      for (int j = 0; j < np; ++j) zr += qe[j];
      if (zr > 0.0) pick = invert_weights(qe, np, zr, un);
    }
    if (pick < 0) pick = invert_weights(L.ev, np, zp, un);   // position K, or q' == p' on p's support: the target's own draw
    a.cand[b * (K + 1) + i] = static_cast<int32_t>(L.sel[pick]);
  }
}

__global__ __launch_bounds__(kSampleThreads) void spec_stats_shaped_kernel(const SpecStatArgs a, const SpecShape sh) {
  __shared__ SpecShapedLds G;
  spec_stats_shaped_row(G, a, sh, blockIdx.x, blockIdx.y);
}

union SpecStatsRowsLds {
  SpecStatsLds plain;
  SpecShapedLds shaped;
};

__global__ __launch_bounds__(kSampleThreads) void spec_stats_rows_kernel(const SpecStatArgs a0, const sd_row_sampling* table) {
  __shared__ SpecStatsRowsLds U;
  const int i = blockIdx.x, b = blockIdx.y;
  if (a0.active && a0.active[b] == 0) return;
  SpecStatArgs a = a0;
  const SpecShape sh = spec_row_params(a, table, b);
  if (sh.top_k > 0) spec_stats_shaped_row(U.shaped, a, sh, i, b);
  else spec_stats_row(U.plain, a, i, b);
}

// statistics, then accept; top_k == 0: spec_stats_kernel, else the shaped kernel; with a table the row kernel
static int launch_spec_kernels(const SpecStatArgs& sa, const SpecAcceptArgs& aa, int B, const DrawSpec& d, hipStream_t st) {
  SD_REQUIRE(B >= 1 && B <= 65535 && sa.K >= 1 && sa.K <= 63 && sa.V >= 1 && ((d.top_k <= 0 && !d.table) || sa.V <= (1 << kIdxBits)),
             "spec_sample: B=%d K=%d V=%d out of range", B, sa.K, sa.V);
  if (d.table) {
    SD_REQUIRE((reinterpret_cast<uintptr_t>(d.table) & 15) == 0, "spec_sample: the row table must be 16-byte aligned");
    hipLaunchKernelGGL(spec_stats_rows_kernel, dim3(sa.K + 1, B), dim3(kSampleThreads), 0, st, sa, d.table);
    SD_LAUNCH_CHECK();
    hipLaunchKernelGGL(spec_accept_kernel, dim3(B), dim3(kWave), 0, st, aa);
    SD_LAUNCH_CHECK();
    return 0;
  }
  SD_REQUIRE(sa.temperature == sa.temperature && sa.temperature > 0.f, "spec_sample: temperature %g (must be > 0)", sa.temperature);
  if (d.top_k > 0) {
    if (int rc = check_spec_shape("spec_sample", d.top_k, d.top_p)) return rc;
    hipLaunchKernelGGL(spec_stats_shaped_kernel, dim3(sa.K + 1, B), dim3(kSampleThreads), 0, st, sa, SpecShape{d.top_k, d.top_p});
  } else {
    hipLaunchKernelGGL(spec_stats_kernel, dim3(sa.K + 1, B), dim3(kSampleThreads), 0, st, sa);
  }
  SD_LAUNCH_CHECK();
  hipLaunchKernelGGL(spec_accept_kernel, dim3(B), dim3(kWave), 0, st, aa);
  SD_LAUNCH_CHECK();
  return 0;
}

// the step's statistics + accept: accept length -> s.accept_len, next token -> s.sampled, counters advanced
int launch_spec_step(const SpecState& s, const void* target_logits, const void* draft_logits, int V, const DrawSpec& d, int32_t* flag,
                     int32_t* cand, hipStream_t st) {
  SD_REQUIRE(target_logits && draft_logits && d.draw && flag && cand, "spec_step: NULL buffer");
  const SpecStatArgs sa = spec_stat_args(target_logits, draft_logits, s.draft_tok, s.K, V, d, s.active, flag, cand, nullptr);
  const SpecAcceptArgs aa{flag, cand, s.K, s.active, d.draw, s.accept_len, s.sampled};
  return launch_spec_kernels(sa, aa, s.B, d, st);
}

}  // namespace sd

using namespace sd;

extern "C" size_t sd_spec_sample_workspace(int B, int K) {
  if (B <= 0 || K <= 0) return 0;
  return static_cast<size_t>(B) * (K + 1) * 2 * sizeof(int32_t);
}

// the stand-alone op, shaped (d.top_k > 0), by row (d.table) or neither; `who` is the op's name in the messages
static int spec_sample_accept_op(const char* who, const DrawSpec& d, const void* draft_logits, const void* target_logits,
                                 const int32_t* draft_ids, int B, int K, int V, const int32_t* active, int32_t* accept_len_out,
                                 int32_t* next_tok_out, double* ratios_out, void* workspace, size_t workspace_bytes, void* stream) {
  SD_REQUIRE(draft_logits && target_logits && draft_ids && accept_len_out && next_tok_out && workspace, "%s: NULL argument", who);
  SD_REQUIRE(B >= 1 && K >= 1, "%s: B=%d K=%d", who, B, K);
  SD_REQUIRE(workspace_bytes >= sd_spec_sample_workspace(B, K), "%s: workspace %zu B < %zu B", who, workspace_bytes,
             sd_spec_sample_workspace(B, K));
  SD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0 && (!ratios_out || (reinterpret_cast<uintptr_t>(ratios_out) & 7) == 0),
             "%s: misaligned workspace / ratios", who);
  int32_t* flag = static_cast<int32_t*>(workspace);
  int32_t* cand = flag + static_cast<size_t>(B) * (K + 1);
  const SpecStatArgs sa = spec_stat_args(target_logits, draft_logits, draft_ids, K, V, d, active, flag, cand, ratios_out);
  const SpecAcceptArgs aa{flag, cand, K, active, d.draw, accept_len_out, next_tok_out};
  return launch_spec_kernels(sa, aa, B, d, static_cast<hipStream_t>(stream));
}

extern "C" int sd_spec_sample_accept(const void* draft_logits, const void* target_logits, const int32_t* draft_ids, int B, int K,
                                     int V, float temperature, uint64_t seed, uint32_t* draw_counters, uint32_t draw0,
                                     const int32_t* stream_ids, const int32_t* active, int32_t* accept_len_out, int32_t* next_tok_out,
                                     double* ratios_out, void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  const DrawSpec d{temperature, 0, 1.0f, seed, draw_counters, draw0, stream_ids};
  return spec_sample_accept_op("spec_sample_accept", d, draft_logits, target_logits, draft_ids, B, K, V, active, accept_len_out,
                               next_tok_out, ratios_out, workspace, workspace_bytes, stream);
}

extern "C" int sd_spec_sample_accept_shaped(const void* draft_logits, const void* target_logits, const int32_t* draft_ids, int B, int K,
                                            int V, float temperature, int top_k, float top_p, uint64_t seed, uint32_t* draw_counters,
                                            uint32_t draw0, const int32_t* stream_ids, const int32_t* active, int32_t* accept_len_out,
                                            int32_t* next_tok_out, double* ratios_out, void* workspace, size_t workspace_bytes,
                                            void* stream) {
  clear_error();
  SD_REQUIRE(top_p == top_p && top_p > 0.f, "spec_sample_accept_shaped: top_p %g (must be > 0)", top_p);
  SD_REQUIRE(top_k > 0, "spec_sample_accept_shaped: top_k=%d with top_p=%g: the shaped op needs a top_k in 1..1024 (top_p without top_k, "
             "the full-vocabulary nucleus, is not supported; the unshaped op is sd_spec_sample_accept)", top_k, top_p);
  SD_REQUIRE(top_k <= kSampleMaxK, "spec_sample_accept_shaped: top_k=%d > %d is not supported", top_k, kSampleMaxK);
  const DrawSpec d{temperature, top_k, top_p, seed, draw_counters, draw0, stream_ids};
  return spec_sample_accept_op("spec_sample_accept_shaped", d, draft_logits, target_logits, draft_ids, B, K, V, active, accept_len_out,
                               next_tok_out, ratios_out, workspace, workspace_bytes, stream);
}

extern "C" int sd_spec_sample_accept_rows(const void* draft_logits, const void* target_logits, const int32_t* draft_ids, int B, int K, int V,
                                          const sd_row_sampling* table, uint32_t* draw_counters, uint32_t draw0, const int32_t* stream_ids,
                                          const int32_t* active, int32_t* accept_len_out, int32_t* next_tok_out, double* ratios_out,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  SD_REQUIRE(table, "spec_sample_accept_rows: NULL table");
  SD_REQUIRE(B >= 1, "spec_sample_accept_rows: B=%d", B);
  SD_REQUIRE((reinterpret_cast<uintptr_t>(table) & 15) == 0, "spec_sample_accept_rows: the row table must be 16-byte aligned");
  const DrawSpec d{1.0f, 0, 1.0f, 0, draw_counters, draw0, stream_ids, table};   // the scalars are not in the launch
  return spec_sample_accept_op("spec_sample_accept_rows", d, draft_logits, target_logits, draft_ids, B, K, V, active, accept_len_out,
                               next_tok_out, ratios_out, workspace, workspace_bytes, stream);
}
