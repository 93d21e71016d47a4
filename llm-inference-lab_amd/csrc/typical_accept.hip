// Lossy acceptance rules on the verify pass's logits (sd_typical_accept, sd_specdec_set_acceptance): a draft token is kept when
// the target finds it plausible enough, judged on the target's distribution CONDITIONED on the draft tokens before it — row i
// of the [B][K+1][V] block the K+1-token verify forward stores.
//
//   rule 1, typical (the entropy-scaled threshold of the Medusa paper): keep d iff p(d) >= min(eps, delta * exp(-H(p)));
//           delta = +inf is the fixed threshold eps
//   rule 2, top-k agreement: keep d iff rank(d) < agree_k, rank(d) = #{v : x_v > x_d, or x_v == x_d and v < d}: the ties of the
//           argmax kernels (argmax_better, common.h), so agree_k = 1 is exactly "d is the target's argmax"
//
// TWO LAUNCHES
//   typical_row_kernel      one 1024-thread workgroup per (b, i), i < K: ONE pass over the row (the walkers of sample_device.h)
//                           -> p(d), H, threshold, rank(d) and the flag of the rule
//   typical_accept_kernel   one wave per row b: accept length = the leading run of flags (ballot, ctz); optionally the token
//                           after the accepted prefix from the target's ids, and the stats records
//
// THE STREAM. With x the stored logit and T the temperature, t_v = (x_v - m) / T for the running maximum m (kept in logit
// units: the difference of two stored values is exact or rounded once, then ONE division), and
//   S = sum_v e^{t_v},  W = sum_v t_v e^{t_v}            H = log S - W / S,  p(d) = e^{t_d} / S
// A thread folds its elements in, a new maximum m' rescaling what it has by r = e^{(m - m') / T}: S' = S r + 1,
// W' = (W + ((m - m') / T) S) r; partials (m, S, W) merge the same way. An element at -inf is skipped: it adds exactly 0 to S
// and to W (no -inf * 0 is ever formed), and a partial that has seen no finite element is the identity of the merge. All fp32.
// Every term of W is <= 0 and every term of S is > 0: no cancellation anywhere but the final H.
//
// ORDER. A thread's elements are fixed by V and the row's alignment; the wave merges on the xor tree and lane 0's result is
// taken; thread 0 merges the 16 wave partials in wave order. Nothing depends on where the workgroup runs: bit-identical run to
// run. No atomics, no waiting, no allocation.

#include "engine.h"
#include "sample_device.h"

namespace sd {

struct TypicalPart {
  float m, S, W;   // maximum (logit units; -inf: nothing finite seen), sum e^t, sum t e^t relative to m
};

// b folded into a: the shift is one subtraction and one division, as for an element
__device__ __forceinline__ TypicalPart typical_merge(const TypicalPart& a, const TypicalPart& b, float T) {
  if (b.m == -INFINITY) return a;
  if (a.m == -INFINITY) return b;
  const bool a_top = a.m >= b.m;
  const TypicalPart& hi = a_top ? a : b;
  const TypicalPart& lo = a_top ? b : a;
  const float sh = (lo.m - hi.m) / T;   // <= 0
  const float r = expf(sh);
  return TypicalPart{hi.m, hi.S + lo.S * r, hi.W + (lo.W + sh * lo.S) * r};
}

struct TypicalArgs {
  const void* logits;       // [B][K+1][row_stride] elements of `dtype`; row (b, i) = row i of batch row b
  int dtype;
  int64_t row_stride;
  const int32_t* draft_ids; // [B][K]
  int K, V;
  int rule;
  float temperature, epsilon, delta;
  int agree_k;
  const int32_t* active;    // nullable [B]
  const int32_t* top_ids;   // nullable [B][K+1]: the row's argmax as the forward computed it, BEFORE the row was rounded to its stored
                            // type. Among equal stored values it ranks first, then the lower index: agree_k = 1 is then exactly the
                            // exact-match rule of the step, also where rounding made a tie
  int32_t* flag;            // [B][K]
  float* rec;               // [B][K][4]: p(d), H, threshold, rank(d)
};

struct TypicalLds {
  float m[kSampleThreads / kWave], S[kSampleThreads / kWave], W[kSampleThreads / kWave];
  int rank[kSampleThreads / kWave];
};

__global__ __launch_bounds__(kSampleThreads) void typical_row_kernel(const TypicalArgs a) {
  __shared__ TypicalLds L;
  const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  if (a.active && a.active[b] == 0) return;
  const int V = a.V;
  const size_t rowi = static_cast<size_t>(b) * (a.K + 1) + i;
  const char* row = static_cast<const char*>(a.logits) + rowi * static_cast<size_t>(a.row_stride) * (a.dtype == SD_F32 ? 4 : 2);
  const int d = a.draft_ids[b * a.K + i];
  const bool d_ok = d >= 0 && d < V;   // an id outside the vocabulary is rejected, never read
  const float xd = d_ok ? load_logit(row, a.dtype, d) : -INFINITY;
  const float T = a.temperature;
  const int top = a.top_ids ? a.top_ids[rowi] : -1;

  TypicalPart p{-INFINITY, 0.f, 0.f};
  int rank = 0;
  for_each_logit(row, a.dtype, V, tid, [&](float x, int v) {
    // (v == top beats an equal d whatever its index; d == top loses to no equal)
    rank += (v == top && v != d) ? ((x >= xd) ? 1 : 0) : ((d == top && x == xd) ? 0 : (argmax_better(x, v, xd, d) ? 1 : 0));
    if (x == -INFINITY) return;
    if (x <= p.m) {
      const float t = (x - p.m) / T;
      const float e = expf(t);
      p.S += e;
      p.W += t * e;
    } else if (p.m == -INFINITY) {
      p = TypicalPart{x, 1.f, 0.f};
    } else {          // a new maximum (or a NaN / +inf element, which poisons the row: it is then rejected)
      const float sh = (p.m - x) / T;
      const float r = expf(sh);
      p.W = (p.W + sh * p.S) * r;
      p.S = p.S * r + 1.f;
      p.m = x;
    }
  });

#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const TypicalPart o{__shfl_xor(p.m, off, 64), __shfl_xor(p.S, off, 64), __shfl_xor(p.W, off, 64)};
    p = typical_merge(p, o, T);
    rank += __shfl_xor(rank, off, 64);
  }
  if ((tid & (kWave - 1)) == 0) {
    const int w = tid / kWave;
    L.m[w] = p.m; L.S[w] = p.S; L.W[w] = p.W;
    L.rank[w] = rank;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < kSampleThreads / kWave; ++w) {
    p = typical_merge(p, TypicalPart{L.m[w], L.S[w], L.W[w]}, T);
    rank += L.rank[w];
  }
  if (!d_ok) rank = V;
  const float H = logf(p.S) - p.W / p.S;
  const float pd = (xd == -INFINITY) ? 0.f : expf((xd - p.m) / T) / p.S;
  float thr;
  bool keep;
  if (a.rule == SD_ACCEPT_TYPICAL) {
    thr = (a.delta == INFINITY) ? a.epsilon : fminf(a.epsilon, a.delta * expf(-H));
    keep = d_ok && (H == H) && pd >= thr;   // a NaN anywhere compares false
  } else {
    thr = static_cast<float>(a.agree_k);
    keep = d_ok && rank < a.agree_k;
  }
  const size_t o = static_cast<size_t>(b) * a.K + i;
  a.flag[o] = keep ? 1 : 0;
  float* rec = a.rec + 4 * o;
  rec[0] = pd;
  rec[1] = H;
  rec[2] = thr;
  rec[3] = static_cast<float>(rank);
}

struct TypicalAcceptArgs {
  const int32_t* flag;        // [B][K]
  const float* rec;           // [B][K][4]
  int K;
  const int32_t* active;      // nullable
  int32_t* accept_len;        // [B]
  const int32_t* target_ids;  // nullable [B][K+1]: next_tok[b] = target_ids[b][accept_len[b]]
  int32_t* next_tok;          // nullable [B]
  float* stats;               // nullable [B][K][4]
};

__global__ __launch_bounds__(kWave) void typical_accept_kernel(const TypicalAcceptArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x, K = a.K;
  if (a.active && a.active[b] == 0) {   // the row's step does not count: nothing accepted
    if (lane == 0) a.accept_len[b] = 0;
    return;
  }
  const bool ok = (lane < K) && a.flag[b * K + lane] != 0;
  const unsigned long long m64 = __ballot(ok);
  const unsigned long long valid = (1ull << K) - 1ull;
  const unsigned long long miss = (~m64) & valid;
  const int acc = miss ? __builtin_ctzll(miss) : K;
  if (lane == 0) {
    a.accept_len[b] = acc;
    if (a.target_ids && a.next_tok) a.next_tok[b] = a.target_ids[b * (K + 1) + acc];
  }
  if (a.stats)
    for (int j = lane; j < 4 * K; j += kWave) a.stats[static_cast<size_t>(b) * 4 * K + j] = a.rec[static_cast<size_t>(b) * 4 * K + j];
}

// Every check of the two launches in one place: the stand-alone op and the step setter both go through it. 0 = ok.
int check_typical_params(const char* who, const AcceptRule& r, int K, int V) {
  SD_REQUIRE(r.rule == SD_ACCEPT_TYPICAL || r.rule == SD_ACCEPT_TOPK_AGREE, "%s: unknown rule %d (1 = typical, 2 = top-k agreement)", who, r.rule);
  SD_REQUIRE(K >= 1 && K <= 63, "%s: K=%d out of range 1..63", who, K);
  SD_REQUIRE(V >= 1, "%s: V=%d", who, V);
  SD_REQUIRE(r.temperature == r.temperature && r.temperature > 0.f && r.temperature < INFINITY, "%s: temperature %g (must be > 0)", who,
             r.temperature);
  if (r.rule == SD_ACCEPT_TYPICAL) {
    SD_REQUIRE(r.epsilon > 0.f && r.epsilon <= 1.0f, "%s: epsilon %g outside (0, 1]", who, r.epsilon);
    SD_REQUIRE(r.delta == r.delta && r.delta > 0.f, "%s: delta %g (must be > 0; +inf = the fixed threshold epsilon)", who, r.delta);
  } else {
    SD_REQUIRE(r.agree_k >= 1 && r.agree_k <= V, "%s: agree_k %d outside 1..V (%d)", who, r.agree_k, V);
  }
  return 0;
}

size_t typical_accept_workspace(int B, int K) {
  if (B <= 0 || K <= 0) return 0;
  return static_cast<size_t>(B) * K * 5 * sizeof(int32_t);   // flags [B][K], records [B][K][4]
}

// the parameters are checked (check_typical_params) by the caller
int launch_typical_accept(const void* logits, int dtype, int64_t row_stride, const int32_t* draft_ids, int B, int K, int V,
                          const AcceptRule& r, const int32_t* active, int32_t* accept_len, const int32_t* target_ids, int32_t* next_tok,
                          float* stats, void* workspace, hipStream_t st) {
  SD_REQUIRE(B >= 1 && B <= 65535, "typical_accept: B=%d out of range", B);
  int32_t* flag = static_cast<int32_t*>(workspace);
  float* rec = reinterpret_cast<float*>(flag + static_cast<size_t>(B) * K);
  const TypicalArgs ta{logits, dtype, row_stride, draft_ids, K, V, r.rule, r.temperature, r.epsilon, r.delta, r.agree_k, active, target_ids,
                       flag, rec};
  hipLaunchKernelGGL(typical_row_kernel, dim3(K, B), dim3(kSampleThreads), 0, st, ta);
  SD_LAUNCH_CHECK();
  const TypicalAcceptArgs aa{flag, rec, K, active, accept_len, target_ids, next_tok, stats};
  hipLaunchKernelGGL(typical_accept_kernel, dim3(B), dim3(kWave), 0, st, aa);
  SD_LAUNCH_CHECK();
  return 0;
}

// the step's two launches: accept length -> s.accept_len; the target's id after the accepted prefix -> s.sampled unless the
// sampled-bonus draw follows (next_from_ids == false)
int launch_typical_step(const SpecState& s, const void* logits, int V, const AcceptRule& r, bool next_from_ids, void* workspace,
                        hipStream_t st) {
  SD_REQUIRE(logits && workspace, "typical_step: NULL buffer");
  return launch_typical_accept(logits, SD_BF16, V, s.draft_tok, s.B, s.K, V, r, s.active, s.accept_len, s.target_ids,
                               next_from_ids ? s.sampled : nullptr, nullptr, workspace, st);
}

}  // namespace sd

using namespace sd;

extern "C" size_t sd_typical_accept_workspace(int B, int K, int V) {
  (void)V;
  return typical_accept_workspace(B, K);
}

extern "C" int sd_typical_accept(const void* target_logits, int logits_dtype, int64_t row_stride, const int32_t* draft_ids, int B, int K,
                                 int V, int rule, float temperature, float epsilon, float delta, int agree_k, int32_t* accept_len,
                                 float* stats, void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  SD_REQUIRE(target_logits && draft_ids && accept_len && workspace, "typical_accept: NULL argument");
  SD_REQUIRE(logits_dtype == SD_F32 || logits_dtype == SD_BF16 || logits_dtype == SD_F16, "typical_accept: logits dtype %d", logits_dtype);
  SD_REQUIRE(B >= 1, "typical_accept: B=%d", B);
  const AcceptRule r{rule, temperature, epsilon, delta, agree_k};
  if (int rc = check_typical_params("typical_accept", r, K, V)) return rc;
  SD_REQUIRE(row_stride >= V, "typical_accept: row_stride %lld below V (%d)", static_cast<long long>(row_stride), V);
  SD_REQUIRE(workspace_bytes >= typical_accept_workspace(B, K), "typical_accept: workspace %zu B < %zu B", workspace_bytes,
             typical_accept_workspace(B, K));
  SD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0 && (reinterpret_cast<uintptr_t>(stats) & 3) == 0,
             "typical_accept: misaligned workspace / stats");
  return launch_typical_accept(target_logits, logits_dtype, row_stride, draft_ids, B, K, V, r, nullptr, accept_len, nullptr, nullptr, stats,
                               workspace, static_cast<hipStream_t>(stream));
}
