// Logit processors inside the step: repetition / presence / frequency penalties, a per-row additive bias (logit_bias, banned
// and allowed token sets) applied IN PLACE to stored bf16 logits rows before anything consumes them, with the argmax of each
// processed row as an optional fused output. Restated on the CPU in tests/logit_proc_ref.py; the contract is written out at
// sd_logit_process in include/specdec_hip.h.
//
// State: counts uint16 [B][V] — bit 15: the token occurs in the row's prompt; bits 0..14: how often the row has generated it
// (saturating at 32767). bias: optional float32 [B][V]. For batch row b, a logits row conditioned on the in-step tokens
// t_1..t_i, element v (every line one correctly rounded fp32 operation, no fused multiply-add: this file is built with
// contraction off):
//   x    = float(row[v])
//   c    = (counts[b][v] & 0x7fff) + #{j <= i : t_j == v}
//   seen = (counts[b][v] & 0x8000) != 0 or c > 0
//   if seen and rp != 1:  x = (x < 0) ? x * rp : x / rp      (HF RepetitionPenaltyLogitsProcessor: x == 0 takes the division)
//   if c > 0:             x = x - presence;  x = x - (frequency * float(c))
//   if bias:              x = x + bias[b][v]
//   row[v] = bf16(x)      (round to nearest even; a NaN is stored as 0x7fc0)
// With a grammar bound (csrc/grammar.hip; logit_process_kernel<true>) one more line follows the bias: an element the row's
// automaton state does not allow is stored as -inf whatever x is, a NaN too (the contract is at sd_logit_process_fsm).
//
// Per-row penalties (sd_logit_process_rows): logit_process_rows_kernel takes rp / presence / frequency of batch row b from its
// sd_row_sampling entry (normalised: what the scalar entry refuses is the identity for the row) and runs the same transform.
//
// Why in place: every consumer of a stored row (the sampler, the speculative-sampling statistics, the draws, the agreement
// op) defines its contract on the stored bf16 values; processing the stored row keeps all of them word for word.
//
// Geometry: a row at V = 128256 is 256 KB of logits + 256 KB of counts + 513 KB of bias; through one CU's intake that is
// ~18 us, so a row is split over S = ceil(V / 4096) <= 64 workgroups of 256 threads (grid S x rows), 16-byte loads of 8
// elements per lane, the V % 8 tail elements by the row's last workgroup. Rows of an odd V are not 16-byte aligned from row to
// row: a row whose logits, counts or bias pointer is misaligned takes the element-wise path, as the spec-sampling kernels do.
// The argmax goes through per-workgroup partials [rows][S] and launch_argmax_finalize (the lm_head's layout and ordering:
// NaN first, larger value, lower index). No grid barrier, no spin-wait, no atomics.
//
// Counts: logit_counts_set_kernel (one workgroup: clears a row, then marks prompt ids and counts generated ids; thread t owns
// the ids with id % 1024 == t, so duplicates are applied in order by one thread) and logit_counts_add_kernel (one lane per
// row walks its <= K + 1 emitted tokens serially; a token emitted twice counts twice; saturating).

#pragma clang fp contract(off)

#include "engine.h"
#include "sample_device.h"   // normalise_row_sampling

namespace sd {

constexpr int kLpThreads = 256;
constexpr int kLpChunk = 4096;     // elements of a row per workgroup
constexpr int kLpMaxSplit = 64;
constexpr int kLpMaxTokens = 64;   // in-step tokens a row can be conditioned on
constexpr int kLpSetThreads = 1024;

int logit_process_split(int V) {
  const int s = (V + kLpChunk - 1) / kLpChunk;
  return s < 1 ? 1 : (s > kLpMaxSplit ? kLpMaxSplit : s);
}

struct LogitProcArgs {
  uint16_t* rows;            // row (b, r) at rows + (b * R + r) * row_stride
  long long row_stride;
  int R, V;
  const uint16_t* counts;    // [B][V]
  const float* bias;         // [B][V] or null
  const int32_t* tokens;     // in-step tokens of row b at tokens + b * tok_stride
  int tok_stride;
  int n_tokens;              // < 0: row (b, r) is conditioned on the first r tokens; else on the first n_tokens
  const int32_t* active;     // nullable [B]
  float rp, presence, frequency;
  float* part_val;           // nullable: argmax partials [B * R][gridDim.x]
  int* part_idx;
  FsmBind fsm;               // the grammar line (logit_process_kernel<true> only)
};

// The state a row's mask is taken from: batch row b's automaton state after its n in-step tokens. With a position table
// (the step) launch n finds the state after n - 1 tokens where launch n - 1 left it and does the one missing lookup; without
// one (the stand-alone op) it walks. Both read the tokens from memory: the caller is one thread, ahead of the workgroup's barrier.
__device__ __forceinline__ int lp_fsm_state(const LogitProcArgs& a, int b, int n) {
  const FsmBind& f = a.fsm;
  int s = f.state[b];
  const int32_t* tk = a.tokens + static_cast<size_t>(b) * a.tok_stride;
  if (f.pos && n >= 1) {
    // the row's own state (is it constrained at all), the chained state and the token go out together; one dependent lookup
    // follows. (The entry of an unconstrained row holds -1, which fsm_step passes through without a lookup.)
    const int nx = fsm_step(f.next, f.S, a.V, f.pos[static_cast<size_t>(b) * f.pos_stride + n - 1], tk[n - 1]);
    return s < 0 ? -1 : nx;
  }
  if (s < 0) return -1;
  if (s >= f.S) s = kFsmDead;
  for (int j = 0; j < n; ++j) s = fsm_step(f.next, f.S, a.V, s, tk[j]);
  return s;
}

__device__ __forceinline__ uint16_t lp_element(float x, uint32_t cnt, int v, bool has_bias, float bias, const int* toks, int n,
                                               const LogitProcArgs& a) {
  int c = static_cast<int>(cnt & 0x7fffu);
  for (int j = 0; j < n; ++j) c += (toks[j] == v) ? 1 : 0;
  const bool seen = (cnt & 0x8000u) != 0 || c > 0;
  if (seen && a.rp != 1.0f) x = (x < 0.0f) ? __fmul_rn(x, a.rp) : __fdiv_rn(x, a.rp);
  if (c > 0) {
    x = __fsub_rn(x, a.presence);
    x = __fsub_rn(x, __fmul_rn(a.frequency, static_cast<float>(c)));
  }
  if (has_bias) x = __fadd_rn(x, bias);
  return (x != x) ? static_cast<uint16_t>(0x7fc0u) : float_to_bf16_bits(x);
}

// FSM: the grammar line after the bias — an element the row's automaton state does not allow is stored as -inf, whatever
// the lines above made of it (a NaN too). The <false> instantiation is the kernel without a grammar, instruction for instruction.
// The transform of one workgroup's share of row t = b * R + r as a device function on an LDS block of its caller:
// logit_process_kernel calls it with the launch's penalties, logit_process_rows_kernel with the row's own.
struct LogitProcLds {
  int toks[kLpMaxTokens];
  int fsm_s;
  float sv[kLpThreads / kWave];
  int si[kLpThreads / kWave];
};

template <bool FSM>
__device__ __forceinline__ void logit_process_share(LogitProcLds& G, const LogitProcArgs& a, int t, int b, int r) {
  int* const toks = G.toks;
  int& fsm_s = G.fsm_s;
  float* const sv = G.sv;
  int* const si = G.si;
  const int tid = threadIdx.x, V = a.V, S = gridDim.x, x0 = blockIdx.x;
  const bool act = !a.active || a.active[b] != 0;   // an inactive row is only read: its argmax is that of the untouched row
  int n = a.n_tokens < 0 ? r : a.n_tokens;
  n = (act && a.tokens) ? (n > kLpMaxTokens ? kLpMaxTokens : n) : 0;
  if (tid < n) toks[tid] = a.tokens[static_cast<size_t>(b) * a.tok_stride + tid];
  if (FSM && tid == 0) {
    const int s = act ? lp_fsm_state(a, b, n) : -1;
    fsm_s = s;
    // the draft forwards' launches (one row per batch row, n tokens each) leave the state for launch n + 1 and the verify
    if (act && a.fsm.pos && a.n_tokens >= 0 && x0 == 0) a.fsm.pos[static_cast<size_t>(b) * a.fsm.pos_stride + n] = s;
  }
  __syncthreads();
  const int fs = FSM ? fsm_s : -1;   // -1: no mask; kFsmDead: only eos; else row fs of the mask table
  const bool dead = fs == kFsmDead;
  const int eos = a.fsm.eos_id;
  const uint32_t* allow = (FSM && fs >= 0 && !dead) ? a.fsm.allow + static_cast<size_t>(fs) * ((V + 31) >> 5) : nullptr;
  uint16_t* row = a.rows + static_cast<size_t>(t) * a.row_stride;
  const uint16_t* cnt = a.counts + static_cast<size_t>(b) * V;
  const float* bias = a.bias ? a.bias + static_cast<size_t>(b) * V : nullptr;
  const bool has_bias = bias != nullptr;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  auto one = [&](int v) {
    uint16_t w = row[v];
    if (act) {
      w = lp_element(bf16_bits_to_float(w), cnt[v], v, has_bias, has_bias ? bias[v] : 0.f, toks, n, a);
      if (FSM && fs >= 0 && !(dead ? v == eos : ((allow[v >> 5] >> (v & 31)) & 1u) != 0)) w = kBf16NegInf;
      row[v] = w;
    }
    const float f = bf16_bits_to_float(w);
    if (argmax_better(f, v, bv, bi)) { bv = f; bi = v; }
  };
  const bool aligned = ((reinterpret_cast<uintptr_t>(row) | reinterpret_cast<uintptr_t>(cnt) | reinterpret_cast<uintptr_t>(bias)) & 15) == 0;
  if (aligned) {
    const int ngroups = V >> 3, gper = (ngroups + S - 1) / S;
    const int g0 = x0 * gper, g1 = min(ngroups, g0 + gper);
    uint4* row4 = reinterpret_cast<uint4*>(row);
    const uint4* cnt4 = reinterpret_cast<const uint4*>(cnt);
    const float4* bias4 = reinterpret_cast<const float4*>(bias);
    for (int g = g0 + tid; g < g1; g += kLpThreads) {
      const uint4 lw = row4[g];
      uint32_t w[4] = {lw.x, lw.y, lw.z, lw.w};
      if (act) {
        const uint4 cw = cnt4[g];
        const uint32_t c[4] = {cw.x, cw.y, cw.z, cw.w};
        float bb[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (has_bias) {
          const float4 b0 = bias4[2 * g], b1 = bias4[2 * g + 1];
          bb[0] = b0.x; bb[1] = b0.y; bb[2] = b0.z; bb[3] = b0.w;
          bb[4] = b1.x; bb[5] = b1.y; bb[6] = b1.z; bb[7] = b1.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint16_t lo = lp_element(__uint_as_float(w[j] << 16), c[j] & 0xffffu, 8 * g + 2 * j, has_bias, bb[2 * j], toks, n, a);
          const uint16_t hi = lp_element(__uint_as_float(w[j] & 0xffff0000u), c[j] >> 16, 8 * g + 2 * j + 1, has_bias, bb[2 * j + 1], toks, n, a);
          w[j] = static_cast<uint32_t>(lo) | (static_cast<uint32_t>(hi) << 16);
        }
        if (FSM && fs >= 0) {   // the lane's 8 elements are byte g of the state's mask row
          const uint32_t m = dead ? ((eos >> 3) == g ? 1u << (eos & 7) : 0u) : reinterpret_cast<const uint8_t*>(allow)[g];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (!((m >> (2 * j)) & 1u)) w[j] = (w[j] & 0xffff0000u) | kBf16NegInf;
            if (!((m >> (2 * j + 1)) & 1u)) w[j] = (w[j] & 0x0000ffffu) | (static_cast<uint32_t>(kBf16NegInf) << 16);
          }
        }
        row4[g] = make_uint4(w[0], w[1], w[2], w[3]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float lo = __uint_as_float(w[j] << 16), hi = __uint_as_float(w[j] & 0xffff0000u);
        if (argmax_better(lo, 8 * g + 2 * j, bv, bi)) { bv = lo; bi = 8 * g + 2 * j; }
        if (argmax_better(hi, 8 * g + 2 * j + 1, bv, bi)) { bv = hi; bi = 8 * g + 2 * j + 1; }
      }
    }
    if (x0 == S - 1)   // the V % 8 tail elements
      for (int v = (ngroups << 3) + tid; v < V; v += kLpThreads) one(v);
  } else {
    const int eper = (V + S - 1) / S;
    const int e0 = x0 * eper, e1 = min(V, e0 + eper);
    for (int v = e0 + tid; v < e1; v += kLpThreads) one(v);
  }
  if (!a.part_val) return;   // (uniform)
  block_arg_best<kLpThreads / kWave, float, argmax_better>(bv, bi, sv, si);
  if (tid == 0) {
    // (a workgroup whose share of the row is empty leaves (-inf, INT_MAX), which loses against every element)
    a.part_val[static_cast<size_t>(t) * S + x0] = bv;
    a.part_idx[static_cast<size_t>(t) * S + x0] = bi;
  }
}

template <bool FSM>
__global__ __launch_bounds__(kLpThreads) void logit_process_kernel(const LogitProcArgs a) {
  __shared__ LogitProcLds G;
  const int t = blockIdx.y, b = t / a.R;
  logit_process_share<FSM>(G, a, t, b, t - b * a.R);
}

// Per-row penalties (sd_logit_process_rows): every workgroup of batch row b normalises table[b] and runs the same transform
template <bool FSM>
__global__ __launch_bounds__(kLpThreads) void logit_process_rows_kernel(const LogitProcArgs a0, const sd_row_sampling* table) {
  __shared__ LogitProcLds G;
  const int t = blockIdx.y, b = t / a0.R;
  const sd_row_sampling e = normalise_row_sampling(table, b, a0.V, false);
  LogitProcArgs a = a0;
  a.rp = e.repetition_penalty;
  a.presence = e.presence_penalty;
  a.frequency = e.frequency_penalty;
  logit_process_share<FSM>(G, a, t, b, t - b * a0.R);
}

size_t logit_process_workspace(int B, int R, int V) {
  if (B <= 0 || R <= 0 || V <= 0) return 0;
  return static_cast<size_t>(B) * R * logit_process_split(V) * (sizeof(float) + sizeof(int));
}

int launch_logit_process(const LogitRows& rows, const LogitStage& g, const int32_t* tokens, int tok_stride, int n_tokens,
                         const int32_t* active, int32_t* ids_out, int ids_stride, hipStream_t st) {
  const int B = rows.B, R = rows.R, V = rows.V;
  const FsmBind* const fsm = g.fsm;
  SD_REQUIRE(rows.rows && g.counts, "logit_process: NULL rows / counts");
  SD_REQUIRE(B >= 1 && R >= 1 && V >= 1 && static_cast<long long>(B) * R <= 65535, "logit_process: B=%d R=%d V=%d out of range", B, R, V);
  SD_REQUIRE(rows.row_stride >= V, "logit_process: row stride %lld < V=%d", rows.row_stride, V);
  const int n_max = n_tokens < 0 ? R - 1 : n_tokens;
  SD_REQUIRE(n_max <= kLpMaxTokens, "logit_process: %d in-step tokens (at most %d)", n_max, kLpMaxTokens);
  SD_REQUIRE(n_max == 0 || (tokens && tok_stride >= n_max), "logit_process: %d in-step tokens need a token array with a stride >= %d", n_max, n_max);
  if (g.table) {   // the penalties are the rows' own, normalised on the device
    SD_REQUIRE((reinterpret_cast<uintptr_t>(g.table) & 15) == 0, "logit_process: the row table must be 16-byte aligned");
  } else {
    SD_REQUIRE(g.rp == g.rp && g.rp > 0.f, "logit_process: repetition_penalty %g (must be > 0)", g.rp);
    SD_REQUIRE(g.presence - g.presence == 0.f && g.frequency - g.frequency == 0.f, "logit_process: presence %g / frequency %g must be finite",
               g.presence, g.frequency);
  }
  SD_REQUIRE(((reinterpret_cast<uintptr_t>(rows.rows) | reinterpret_cast<uintptr_t>(g.counts)) & 1) == 0 && (reinterpret_cast<uintptr_t>(g.bias) & 3) == 0,
             "logit_process: misaligned rows / counts / bias");
  const int S = logit_process_split(V);
  LogitProcArgs a{};
  a.rows = static_cast<uint16_t*>(rows.rows);
  a.row_stride = rows.row_stride;
  a.R = R;
  a.V = V;
  a.counts = g.counts;
  a.bias = g.bias;
  a.tokens = tokens;
  a.tok_stride = tok_stride;
  a.n_tokens = n_tokens;
  a.active = active;
  a.rp = g.rp;
  a.presence = g.presence;
  a.frequency = g.frequency;
  if (ids_out) {
    SD_REQUIRE(g.workspace && g.workspace_bytes >= logit_process_workspace(B, R, V), "logit_process: workspace %zu B < %zu B", g.workspace_bytes,
               logit_process_workspace(B, R, V));
    SD_REQUIRE((reinterpret_cast<uintptr_t>(g.workspace) & 3) == 0, "logit_process: misaligned workspace");
    SD_REQUIRE(ids_stride >= R, "logit_process: ids stride %d < R=%d", ids_stride, R);
    a.part_val = static_cast<float*>(g.workspace);
    a.part_idx = reinterpret_cast<int*>(a.part_val + static_cast<size_t>(B) * R * S);
  }
  if (fsm) {
    SD_REQUIRE(fsm->next && fsm->allow && fsm->state, "logit_process: NULL automaton table / mask table / state");
    SD_REQUIRE(fsm->S >= 1 && fsm->S <= kFsmMaxStates, "logit_process: S=%d states (1..%d)", fsm->S, kFsmMaxStates);
    SD_REQUIRE(fsm->eos_id >= 0 && fsm->eos_id < V, "logit_process: eos_id %d outside [0, %d)", fsm->eos_id, V);
    SD_REQUIRE(((reinterpret_cast<uintptr_t>(fsm->next) | reinterpret_cast<uintptr_t>(fsm->allow)) & 15) == 0,
               "logit_process: automaton and mask tables must be 16-byte aligned");
    // with a position table: n_tokens >= 0 reads [b][n_tokens - 1] and writes [b][n_tokens] (one row per batch row, or two
    // workgroups would write one word); n_tokens < 0 reads [b][r - 1]
    SD_REQUIRE(!fsm->pos || (n_tokens >= 0 ? (R == 1 && fsm->pos_stride > n_tokens) : fsm->pos_stride >= n_max),
               "logit_process: position table of stride %d for R=%d rows of %d tokens", fsm->pos_stride, R, n_tokens);
    a.fsm = *fsm;
    if (g.table) hipLaunchKernelGGL(logit_process_rows_kernel<true>, dim3(S, B * R), dim3(kLpThreads), 0, st, a, g.table);
    else hipLaunchKernelGGL(logit_process_kernel<true>, dim3(S, B * R), dim3(kLpThreads), 0, st, a);
  } else {
    if (g.table) hipLaunchKernelGGL(logit_process_rows_kernel<false>, dim3(S, B * R), dim3(kLpThreads), 0, st, a, g.table);
    else hipLaunchKernelGGL(logit_process_kernel<false>, dim3(S, B * R), dim3(kLpThreads), 0, st, a);
  }
  SD_LAUNCH_CHECK();
  if (ids_out) return launch_argmax_finalize(a.part_val, a.part_idx, B * R, S, R, ids_stride, ids_out, st);
  return 0;
}

// ---- counts ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLpSetThreads) void logit_counts_set_kernel(uint16_t* row, int V, const int32_t* prompt, int n_prompt,
                                                                         const int32_t* gen, int n_gen) {
  const int tid = threadIdx.x;
  for (int v = tid; v < V; v += kLpSetThreads) row[v] = 0;
  __syncthreads();
  // thread `tid` owns the ids with id % 1024 == tid: every word has one writer, which sees its own earlier stores
  for (int j = 0; j < n_prompt; ++j) {
    const int id = prompt[j];
    if (id >= 0 && id < V && (id & (kLpSetThreads - 1)) == tid) row[id] = 0x8000u;
  }
  for (int j = 0; j < n_gen; ++j) {
    const int id = gen[j];
    if (id >= 0 && id < V && (id & (kLpSetThreads - 1)) == tid) {
      const uint16_t c = row[id];
      if ((c & 0x7fffu) != 0x7fffu) row[id] = static_cast<uint16_t>(c + 1);
    }
  }
}

int launch_logit_counts_set(uint16_t* counts, int B, int V, int b, const int32_t* prompt, int n_prompt, const int32_t* gen, int n_gen,
                            hipStream_t st) {
  SD_REQUIRE(counts && B >= 1 && V >= 1 && b >= 0 && b < B, "logit_counts_set: row %d of B=%d, V=%d", b, B, V);
  SD_REQUIRE(n_prompt >= 0 && n_gen >= 0 && (n_prompt == 0 || prompt) && (n_gen == 0 || gen), "logit_counts_set: a NULL list with a count > 0");
  SD_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 1) == 0, "logit_counts_set: misaligned counts");
  hipLaunchKernelGGL(logit_counts_set_kernel, dim3(1), dim3(kLpSetThreads), 0, st, counts + static_cast<size_t>(b) * V, V, prompt, n_prompt,
                     gen, n_gen);
  SD_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(kWave) void logit_counts_add_kernel(uint16_t* counts, int B, int V, const int32_t* tokens, int tok_stride,
                                                                 const int32_t* n_new, int max_new, const int32_t* active) {
  const int b = blockIdx.x * kWave + threadIdx.x;
  if (b >= B || (active && active[b] == 0)) return;
  uint16_t* row = counts + static_cast<size_t>(b) * V;
  int n = n_new[b];
  n = n < 0 ? 0 : (n > max_new ? max_new : n);
  for (int j = 0; j < n; ++j) {
    const int id = tokens[static_cast<size_t>(b) * tok_stride + j];
    if (id < 0 || id >= V) continue;
    const uint16_t c = row[id];
    if ((c & 0x7fffu) != 0x7fffu) row[id] = static_cast<uint16_t>(c + 1);
  }
}

int launch_logit_counts_add(uint16_t* counts, int B, int V, const int32_t* tokens, int tok_stride, const int32_t* n_new, int max_new,
                            const int32_t* active, hipStream_t st) {
  SD_REQUIRE(counts && tokens && n_new, "logit_counts_add: NULL argument");
  SD_REQUIRE(B >= 1 && V >= 1 && max_new >= 0 && tok_stride >= max_new, "logit_counts_add: B=%d V=%d max_new=%d stride=%d", B, V, max_new, tok_stride);
  SD_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 1) == 0, "logit_counts_add: misaligned counts");
  hipLaunchKernelGGL(logit_counts_add_kernel, dim3((B + kWave - 1) / kWave), dim3(kWave), 0, st, counts, B, V, tokens, tok_stride, n_new,
                     max_new, active);
  SD_LAUNCH_CHECK();
  return 0;
}

}  // namespace sd

using namespace sd;

extern "C" size_t sd_logit_process_workspace(int B, int R, int V) { return logit_process_workspace(B, R, V); }

extern "C" int sd_logit_process(void* rows, int64_t row_stride, int B, int R, int V, const void* counts, const float* bias,
                                const int32_t* tokens, int tok_stride, int n_tokens, const int32_t* active, float repetition_penalty,
                                float presence_penalty, float frequency_penalty, int32_t* ids_out, int ids_stride, void* workspace,
                                size_t workspace_bytes, void* stream) {
  clear_error();
  const LogitStage g{static_cast<const uint16_t*>(counts), bias, repetition_penalty, presence_penalty, frequency_penalty, workspace,
                     workspace_bytes};
  return launch_logit_process({rows, row_stride, B, R, V}, g, tokens, tok_stride, n_tokens, active, ids_out, ids_stride,
                              static_cast<hipStream_t>(stream));
}

extern "C" int sd_logit_process_rows(void* rows, int64_t row_stride, int B, int R, int V, const void* counts, const float* bias,
                                     const int32_t* tokens, int tok_stride, int n_tokens, const int32_t* active, const sd_row_sampling* table,
                                     int32_t* ids_out, int ids_stride, void* workspace, size_t workspace_bytes, const void* next,
                                     const void* allow, int S, const int32_t* fsm_state, int eos_id, void* stream) {
  clear_error();
  SD_REQUIRE(table, "logit_process_rows: NULL table");
  SD_REQUIRE(B >= 1, "logit_process_rows: B=%d", B);
  SD_REQUIRE((reinterpret_cast<uintptr_t>(table) & 15) == 0, "logit_process_rows: the row table must be 16-byte aligned");
  const bool grammar = next || allow || fsm_state;   // all three NULL: no grammar
  FsmBind f{};
  f.next = static_cast<const uint16_t*>(next);
  f.allow = static_cast<const uint32_t*>(allow);
  f.S = S;
  f.state = fsm_state;
  f.eos_id = eos_id;
  const LogitStage g{static_cast<const uint16_t*>(counts), bias, 1.0f, 0.f, 0.f, workspace, workspace_bytes, grammar ? &f : nullptr, table};
  return launch_logit_process({rows, row_stride, B, R, V}, g, tokens, tok_stride, n_tokens, active, ids_out, ids_stride,
                              static_cast<hipStream_t>(stream));
}

extern "C" size_t sd_logit_counts_bytes(int B, int V) {
  if (B <= 0 || V <= 0) return 0;
  return (static_cast<size_t>(B) * V * sizeof(uint16_t) + 15) / 16 * 16;
}

extern "C" int sd_logit_counts_set(void* counts, int B, int V, int b, const int32_t* prompt_ids, int n_prompt, const int32_t* generated_ids,
                                   int n_generated, void* stream) {
  clear_error();
  return launch_logit_counts_set(static_cast<uint16_t*>(counts), B, V, b, prompt_ids, n_prompt, generated_ids, n_generated,
                                 static_cast<hipStream_t>(stream));
}

extern "C" int sd_logit_counts_add(void* counts, int B, int V, const int32_t* tokens, int tok_stride, const int32_t* n_new, int max_new,
                                   const int32_t* active, void* stream) {
  clear_error();
  return launch_logit_counts_add(static_cast<uint16_t*>(counts), B, V, tokens, tok_stride, n_new, max_new, active,
                                 static_cast<hipStream_t>(stream));
}
