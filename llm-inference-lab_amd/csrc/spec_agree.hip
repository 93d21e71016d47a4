// Draft-target agreement of two logit blocks (sd_spec_agreement): what speculative sampling (csrc/spec_sample.hip) will accept,
// predicted without generating. Per row t of two bf16 blocks P (target) and Q (draft), n rows x V elements, in float64 over the
// STORED bf16 values, x / T with T the float32 temperature widened to double and no division when T == 1 (as spec_sample.hip):
//   a_v = P[t][v]/T - lse(P[t]/T),  b_v = Q[t][v]/T - lse(Q[t]/T),  lse(x) = max x + log(sum exp(x - max x))
//   alpha[t] = sum_v min(exp a_v, exp b_v)            = 1 - TV(p, q): the acceptance probability of the position
//   kl[t]    = sum over the v with P[t][v] > -inf of exp(a_v) (a_v - b_v); a Q[t][v] = -inf under a finite P[t][v] adds +inf
//   p_arg[t], q_arg[t] = argmax of the rows under argmax_better (NaN first, larger value, lower index); agree[t] = (p_arg == q_arg)
// A row pair in which either row holds a NaN, or whose maximum is not finite (+inf present, or every entry -inf), gives
// alpha = kl = NaN. No logarithm per element; restated on the CPU in tests/agreement_ref.py.
//
// A row is cut into S = min(32, ceil(V / 4096)) contiguous slices of L = ceil(V / S) rounded up to 8 elements (S depends on V
// only), one 256-thread workgroup each: grid (S, rows). Three launches in ordinary stream order, no atomics, no allocation,
// graph-capturable:
//   agree_partial_kernel   (row, slice): the slice's argmax of both rows (its value is the slice maximum) and NaN flag, then the
//                          sums of exp(x/T - slice maximum) of both rows -> one 64-byte partial
//   agree_slice_kernel     (row, slice): every workgroup of the row folds the row's S partials in slice order (fold_row: the same
//                          arithmetic in every workgroup, so the same lse), then the slice's sum of min and of the KL terms
//   agree_finalize_kernel  one thread per row: fold_row again, the slices' sums added in slice order, the outputs
// Fixed reduction order everywhere: a thread owns the 8-element chunks c = first chunk of the slice + tid + 256 j and visits them
// in order (16-byte loads when both rows are 16-byte aligned, element loads otherwise — the same elements in the same order either
// way, so the bits do not depend on the alignment), xor tree inside a wave, the 4 waves in order, the slices in order. Outputs are
// bit-identical run to run, and row t's outputs depend on nothing but row t: not on n, not on the other rows.
// Bitwise equal rows go through the same code in the same order: a_v == b_v, so kl == 0.0 exactly.

#include "common.h"

namespace sd {

namespace {

constexpr int kAgreeThreads = 256;
constexpr int kAgreeWaves = kAgreeThreads / kWave;
constexpr int kAgreeSlice = 4096;      // a row of V elements has ceil(V / kAgreeSlice) slices ...
constexpr int kAgreeMaxSlices = 32;    // ... at most this many
constexpr int kAgreeMaxRows = 65535;   // grid.y of one launch

inline int agree_slices(int V) {
  const int s = (V + kAgreeSlice - 1) / kAgreeSlice;
  return s < 1 ? 1 : (s > kAgreeMaxSlices ? kAgreeMaxSlices : s);
}

struct AgreePartA {     // one (row, slice) of agree_partial_kernel
  double mp, sp;        // target: slice maximum of x / T (-inf: no finite element), sum of exp(x / T - mp) (0 when mp is not finite)
  double mq, sq;        // draft
  float pv, qv;         // argmax values
  int pi, qi;           // argmax indices (0x7fffffff: empty slice)
  int nan;              // a NaN in either row's slice
  int pad[3];
};
static_assert(sizeof(AgreePartA) == 64, "partial layout");

struct AgreePartB {     // one (row, slice) of agree_slice_kernel
  double smin, skl;
};

struct AgreeArgs {
  const uint16_t* P;    // target rows, ld_p elements apart
  const uint16_t* Q;    // draft rows, ld_q elements apart
  int64_t ld_p, ld_q;
  int n, V, S, L;       // rows of this launch, row length, slices per row, elements per slice (a multiple of 8)
  float temperature;
  AgreePartA* pa;       // [n][S]
  AgreePartB* pb;       // [n][S]
  double* alpha;        // nullable outputs, [n]
  double* kl;
  int32_t* agree;
  int32_t* p_arg;
  int32_t* q_arg;
};

// f(target value, draft value, index) over elements [e0, e1) of two bf16 rows, e0 a multiple of 8: thread tid visits the chunks
// e0 / 8 + tid + kAgreeThreads j, each in element order
// (spec_sample.hip's for_each_pair visits in another order on unaligned rows; each file's float64 sums need its own: two walkers)
template <typename F>
__device__ __forceinline__ void for_each_pair_slice(const uint16_t* rp, const uint16_t* rq, int e0, int e1, int tid, bool vec, F&& f) {
  for (int base = e0 + 8 * tid; base < e1; base += 8 * kAgreeThreads) {
    if (vec && base + 8 <= e1) {
      const uint4 a = *reinterpret_cast<const uint4*>(rp + base), b = *reinterpret_cast<const uint4*>(rq + base);
      const uint32_t wa[4] = {a.x, a.y, a.z, a.w}, wb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f(__uint_as_float(wa[j] << 16), __uint_as_float(wb[j] << 16), base + 2 * j);
        f(__uint_as_float(wa[j] & 0xffff0000u), __uint_as_float(wb[j] & 0xffff0000u), base + 2 * j + 1);
      }
    } else {
      const int end = base + 8 < e1 ? base + 8 : e1;
      for (int i = base; i < end; ++i) f(bf16_bits_to_float(rp[i]), bf16_bits_to_float(rq[i]), i);
    }
  }
}

// sums of two doubles over the workgroup, every thread gets both: xor tree inside a wave, then the waves in order
__device__ __forceinline__ void block_sum2(double& x, double& y, double (*sh)[kAgreeWaves]) {
  x = wave_reduce_sum_d(x);
  y = wave_reduce_sum_d(y);
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = x;
    sh[1][threadIdx.x >> 6] = y;
  }
  __syncthreads();
  x = sh[0][0];
  y = sh[1][0];
  for (int w = 1; w < kAgreeWaves; ++w) {
    x += sh[0][w];
    y += sh[1][w];
  }
}

struct RowFold {
  double lse_p, lse_q;
  int pi, qi;
  bool bad;
};

// the row's S partials folded in slice order
__device__ __forceinline__ RowFold fold_row(const AgreePartA* pa, int S, double T, bool scale) {
  float pv = pa[0].pv, qv = pa[0].qv;
  int pi = pa[0].pi, qi = pa[0].qi, nan = pa[0].nan;
  for (int s = 1; s < S; ++s) {
    if (argmax_better(pa[s].pv, pa[s].pi, pv, pi)) { pv = pa[s].pv; pi = pa[s].pi; }
    if (argmax_better(pa[s].qv, pa[s].qi, qv, qi)) { qv = pa[s].qv; qi = pa[s].qi; }
    nan |= pa[s].nan;
  }
  RowFold r;
  r.pi = pi;
  r.qi = qi;
  const double Mp = scale ? static_cast<double>(pv) / T : static_cast<double>(pv);
  const double Mq = scale ? static_cast<double>(qv) / T : static_cast<double>(qv);
  r.bad = nan != 0 || !is_finite_d(Mp) || !is_finite_d(Mq);
  r.lse_p = r.lse_q = NAN;
  if (!r.bad) {
    double sp = 0.0, sq = 0.0;
    for (int s = 0; s < S; ++s) {
      if (pa[s].mp != -INFINITY) sp += pa[s].sp * exp(pa[s].mp - Mp);
      if (pa[s].mq != -INFINITY) sq += pa[s].sq * exp(pa[s].mq - Mq);
    }
    r.lse_p = Mp + log(sp);
    r.lse_q = Mq + log(sq);
  }
  return r;
}

__global__ __launch_bounds__(kAgreeThreads) void agree_partial_kernel(const AgreeArgs a) {
  __shared__ float s_v[2][kAgreeWaves];
  __shared__ int s_i[2][kAgreeWaves];
  __shared__ double s_s[2][kAgreeWaves];
  const int s = blockIdx.x, t = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint16_t* rp = a.P + static_cast<size_t>(t) * a.ld_p;
  const uint16_t* rq = a.Q + static_cast<size_t>(t) * a.ld_q;
  const int e0 = s * a.L, e1 = (a.V - e0 < a.L) ? a.V : e0 + a.L;
  const bool vec = ((reinterpret_cast<uintptr_t>(rp) | reinterpret_cast<uintptr_t>(rq)) & 15) == 0;
  const double T = static_cast<double>(a.temperature);
  const bool scale = a.temperature != 1.0f;

  float pv = -INFINITY, qv = -INFINITY;
  int pi = 0x7fffffff, qi = 0x7fffffff, nan = 0;
  for_each_pair_slice(rp, rq, e0, e1, tid, vec, [&](float xp, float xq, int i) {
    nan |= (xp != xp) | (xq != xq);
    if (argmax_better(xp, i, pv, pi)) { pv = xp; pi = i; }
    if (argmax_better(xq, i, qv, qi)) { qv = xq; qi = i; }
  });
  wave_reduce_argmax(pv, pi);
  wave_reduce_argmax(qv, qi);
  if (lane == 0) {   // both pairs in every thread behind ONE barrier: block_arg_best's fold, by all threads
    s_v[0][wave] = pv; s_i[0][wave] = pi;
    s_v[1][wave] = qv; s_i[1][wave] = qi;
  }
  nan = __syncthreads_or(nan);
  pv = s_v[0][0]; pi = s_i[0][0];
  qv = s_v[1][0]; qi = s_i[1][0];
  for (int w = 1; w < kAgreeWaves; ++w) {
    if (argmax_better(s_v[0][w], s_i[0][w], pv, pi)) { pv = s_v[0][w]; pi = s_i[0][w]; }
    if (argmax_better(s_v[1][w], s_i[1][w], qv, qi)) { qv = s_v[1][w]; qi = s_i[1][w]; }
  }
  const double mp = scale ? static_cast<double>(pv) / T : static_cast<double>(pv);
  const double mq = scale ? static_cast<double>(qv) / T : static_cast<double>(qv);
  const bool fp = is_finite_d(mp), fq = is_finite_d(mq);   // (workgroup-uniform)
  double sp = 0.0, sq = 0.0;
  if (fp | fq)
    for_each_pair_slice(rp, rq, e0, e1, tid, vec, [&](float xp, float xq, int) {
      const double vp = static_cast<double>(xp), vq = static_cast<double>(xq);
      if (fp) sp += exp((scale ? vp / T : vp) - mp);
      if (fq) sq += exp((scale ? vq / T : vq) - mq);
    });
  block_sum2(sp, sq, s_s);
  if (tid == 0) {
    AgreePartA o{};
    o.mp = mp; o.sp = sp;
    o.mq = mq; o.sq = sq;
    o.pv = pv; o.qv = qv;
    o.pi = pi; o.qi = qi;
    o.nan = nan;
    a.pa[static_cast<size_t>(t) * a.S + s] = o;
  }
}

__global__ __launch_bounds__(kAgreeThreads) void agree_slice_kernel(const AgreeArgs a) {
  __shared__ double s_s[2][kAgreeWaves];
  const int s = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  const double T = static_cast<double>(a.temperature);
  const bool scale = a.temperature != 1.0f;
  const RowFold r = fold_row(a.pa + static_cast<size_t>(t) * a.S, a.S, T, scale);
  if (r.bad) return;   // (workgroup-uniform) the finalize writes NaN without reading this row's sums
  const uint16_t* rp = a.P + static_cast<size_t>(t) * a.ld_p;
  const uint16_t* rq = a.Q + static_cast<size_t>(t) * a.ld_q;
  const int e0 = s * a.L, e1 = (a.V - e0 < a.L) ? a.V : e0 + a.L;
  const bool vec = ((reinterpret_cast<uintptr_t>(rp) | reinterpret_cast<uintptr_t>(rq)) & 15) == 0;
  double smin = 0.0, skl = 0.0;
  for_each_pair_slice(rp, rq, e0, e1, tid, vec, [&](float xp, float xq, int) {
    if (xp == -INFINITY) return;   // p(v) = 0: nothing to either sum
    if (xq == -INFINITY) {         // q(v) = 0 under p(v) > 0
      skl += INFINITY;
      return;
    }
    const double vp = static_cast<double>(xp), vq = static_cast<double>(xq);
    const double av = (scale ? vp / T : vp) - r.lse_p, bv = (scale ? vq / T : vq) - r.lse_q;
    const double ea = exp(av), eb = exp(bv);
    smin += fmin(ea, eb);
    skl += ea * (av - bv);
  });
  block_sum2(smin, skl, s_s);
  if (tid == 0) a.pb[static_cast<size_t>(t) * a.S + s] = AgreePartB{smin, skl};
}

__global__ __launch_bounds__(kAgreeThreads) void agree_finalize_kernel(const AgreeArgs a) {
  const int t = blockIdx.x * kAgreeThreads + threadIdx.x;
  if (t >= a.n) return;
  const RowFold r = fold_row(a.pa + static_cast<size_t>(t) * a.S, a.S, static_cast<double>(a.temperature), a.temperature != 1.0f);
  double alpha = NAN, kl = NAN;
  if (!r.bad) {
    const AgreePartB* pb = a.pb + static_cast<size_t>(t) * a.S;
    alpha = pb[0].smin;
    kl = pb[0].skl;
    for (int s = 1; s < a.S; ++s) {
      alpha += pb[s].smin;
      kl += pb[s].skl;
    }
  }
  if (a.alpha) a.alpha[t] = alpha;
  if (a.kl) a.kl[t] = kl;
  if (a.agree) a.agree[t] = (r.pi == r.qi) ? 1 : 0;
  if (a.p_arg) a.p_arg[t] = r.pi;
  if (a.q_arg) a.q_arg[t] = r.qi;
}

}  // namespace

}  // namespace sd

using namespace sd;

extern "C" size_t sd_spec_agreement_workspace(int n, int V) {
  if (n <= 0 || V <= 0) return 0;
  return static_cast<size_t>(n) * agree_slices(V) * (sizeof(AgreePartA) + sizeof(AgreePartB));
}

extern "C" int sd_spec_agreement(const void* draft_logits, int64_t ld_q, const void* target_logits, int64_t ld_p, int n, int V,
                                 float temperature, double* alpha, double* kl, int32_t* agree, int32_t* p_arg, int32_t* q_arg,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  SD_REQUIRE(draft_logits && target_logits, "spec_agreement: NULL logits");
  SD_REQUIRE(n >= 1 && V >= 1, "spec_agreement: n=%d V=%d", n, V);
  SD_REQUIRE(ld_q >= V && ld_p >= V, "spec_agreement: row strides %lld / %lld below V=%d", static_cast<long long>(ld_q),
             static_cast<long long>(ld_p), V);
  SD_REQUIRE(temperature == temperature && temperature > 0.f, "spec_agreement: temperature %g (must be > 0)", temperature);
  SD_REQUIRE(workspace && workspace_bytes >= sd_spec_agreement_workspace(n, V), "spec_agreement: workspace %zu B < %zu B",
             workspace ? workspace_bytes : static_cast<size_t>(0), sd_spec_agreement_workspace(n, V));
  SD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && ((reinterpret_cast<uintptr_t>(alpha) | reinterpret_cast<uintptr_t>(kl)) & 7) == 0 &&
                 ((reinterpret_cast<uintptr_t>(draft_logits) | reinterpret_cast<uintptr_t>(target_logits)) & 1) == 0,
             "spec_agreement: misaligned workspace / logits / outputs");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int S = agree_slices(V);
  AgreePartA* pa = static_cast<AgreePartA*>(workspace);
  AgreePartB* pb = reinterpret_cast<AgreePartB*>(pa + static_cast<size_t>(n) * S);
  for (int r0 = 0; r0 < n; r0 += kAgreeMaxRows) {
    AgreeArgs a{};
    a.P = static_cast<const uint16_t*>(target_logits) + static_cast<size_t>(r0) * ld_p;
    a.Q = static_cast<const uint16_t*>(draft_logits) + static_cast<size_t>(r0) * ld_q;
    a.ld_p = ld_p;
    a.ld_q = ld_q;
    a.n = (n - r0 < kAgreeMaxRows) ? n - r0 : kAgreeMaxRows;
    a.V = V;
    a.S = S;
    a.L = ((V + S - 1) / S + 7) & ~7;
    a.temperature = temperature;
    a.pa = pa + static_cast<size_t>(r0) * S;
    a.pb = pb + static_cast<size_t>(r0) * S;
    a.alpha = alpha ? alpha + r0 : nullptr;
    a.kl = kl ? kl + r0 : nullptr;
    a.agree = agree ? agree + r0 : nullptr;
    a.p_arg = p_arg ? p_arg + r0 : nullptr;
    a.q_arg = q_arg ? q_arg + r0 : nullptr;
    hipLaunchKernelGGL(agree_partial_kernel, dim3(S, a.n), dim3(kAgreeThreads), 0, st, a);
    SD_LAUNCH_CHECK();
    hipLaunchKernelGGL(agree_slice_kernel, dim3(S, a.n), dim3(kAgreeThreads), 0, st, a);
    SD_LAUNCH_CHECK();
    hipLaunchKernelGGL(agree_finalize_kernel, dim3((a.n + kAgreeThreads - 1) / kAgreeThreads), dim3(kAgreeThreads), 0, st, a);
    SD_LAUNCH_CHECK();
  }
  return 0;
}
