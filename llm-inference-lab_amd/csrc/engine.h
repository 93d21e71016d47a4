// Engine-internal types: the model instance (created and bound in csrc/model.hip, run by csrc/engine.hip, measured and read back
// by csrc/probe.hip) and the device-side state of the draft-then-verify loop (csrc/spec_loop.hip). The C-ABI view of these is in
// include/specdec_hip.h.
#pragma once

#include <vector>

#include "kernels.h"
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
  // W12 copies (sd_model_set_w12 / sd_model_set_w12_form; csrc/pack.hip), per matrix or empty; main == nullptr: the matrix keeps
  // its bf16 stream. `form` (W12Form) is recorded per matrix: the classes of one model may stream different forms.
  // Read by launches of <= 9 tokens only (launch_gemv); the persistent forward, prefill and > 9 tokens read `packed`.
  struct W12Mat { const void* main; const uint32_t* table; const void* ovf; int form; };
  std::vector<W12Mat> w12;
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

// csrc/engine.hip: what the step loop (csrc/spec_loop.hip), the binds (csrc/model.hip) and the probes (csrc/probe.hip) need from
// the forward
constexpr int kMaxPartials = 512;
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// One forward: rows [row0, row0+B) of the bound batch, M tokens each; tokens / pos_base / ids_out / logits_out are indexed from
// row0 (element 0 of each array belongs to row row0)
struct ForwardCall {
  const int32_t* tokens = nullptr;    // row b's tokens at tokens + b * tok_stride
  int tok_stride = 0;
  const int32_t* pos_base = nullptr;  // [B]: row b's first token sits at position pos_base[b] + pos_off
  int pos_off = 0;
  int row0 = 0, B = 1, M = 1;
  int32_t* ids_out = nullptr;         // nullable: argmax id of (b, t) at ids_out[b * ids_stride + t]
  int ids_stride = 0;
  void* logits_out = nullptr;         // nullable [B][M][vocab] of logits_dtype (SD_F32 / SD_BF16)
  int logits_dtype = SD_BF16;
  int skip_head = 0;                  // 1: the layers only (the residual rows stay in the workspace)
};
int model_forward(sd_model* m, const ForwardCall& f, hipStream_t st);
GemvArgs matrix_args(const sd_model* m, int index);
// What belongs to the call, on top of matrix_args: the pass's tokens, and with pos_base the rows' positions, the head geometry and
// the cache paging (bt: the pass's first row of the block table, null on dense KV). gated: the launch leaves at entry when the
// adaptive step's word says so (m->skip_k / skip_i), as every launch of a forward pass does.
void call_args(GemvArgs& g, const sd_model* m, int T, int M, bool gated, const int32_t* pos_base = nullptr, int pos_off = 0,
               const int32_t* bt = nullptr);
bool persist_pass_ok(const sd_model* m, int T, int Bc, int Mc);

// The four row buffers a pass stages, by the `which` of sd_model_debug_rows / sd_model_prefill_rows, and the elements in a row of each
struct StagedRows {
  uint16_t* buf[4];   // 0 x, 1 q, 2 attn, 3 act
  int width[4];       // d_model, Hq * D, Hq * D, d_ff
};
inline StagedRows staged_rows(const sd_model_config& c, uint16_t* x, uint16_t* q, uint16_t* attn, uint16_t* act) {
  return {{x, q, attn, act}, {c.d_model, c.n_heads * c.head_dim, c.n_heads * c.head_dim, c.d_ff}};
}
inline StagedRows staged_rows(const sd_model* m) { return staged_rows(m->cfg, m->x, m->q, m->attn, m->act); }
inline StagedRows staged_rows(const sd_model_config& c, const PrefillRows& r) { return staged_rows(c, r.x, r.q, r.attn, r.act); }

// device-resident loop state (all int32, B rows, K draft tokens per step)
struct SpecState {
  int B, K;
  int32_t* cur_len;     // [B]   tokens whose KV is final in the target cache (= position of `last`)
  int32_t* active;      // [B]   1 = row advances
  int32_t* tok2;        // [B][2]   (prev, last): input of draft forward 0
  int32_t* next_tok;    // [B]      input of draft forwards 1..K-1
  int32_t* draft_ids;   // [B][2]   argmax ids of the current draft forward
  int32_t* draft_tok;   // [B][K]   d_1..d_K
  int32_t* verify_tok;  // [B][K+1] (last, d_1..d_K): input of the verify forward
  int32_t* target_ids;  // [B][K+1] target argmax at each verify position
  int32_t* accept_len;  // [B]
  int32_t* n_new;       // [B]
  int32_t* new_tok;     // [B][K+1] emitted tokens, -1 padded
  int32_t* sampled;     // [B]   sampled token for position accept_len (sampling mode), else unused
  // per-row adaptive K (sd_specdec_set_adaptive): the rule of AdaptiveKController (controllers.py:63-141) per row, on
  // the device, so that the next step never waits for the host. K above stays the SHAPE of the step (max_k).
  int adaptive;         // 0 = every row proposes K
  int a_min, a_max, a_step;
  double a_hi, a_lo;    // target_acceptance_rate + 0.1 / - 0.1 (computed by the host in double, as the reference does)
  int32_t* k_row;       // [B]    proposals that count for the row in the NEXT step
  int32_t* ctl;         // [B][4] accepted so far, proposed so far, history length (<= 4), k of the step just done
  double* ctl_hist;     // [B][4] the last four reported acceptance rates, oldest first
  int32_t* k_active;    // [1]    max k_row over the active rows
  // confidence-gated draft length (sd_specdec_set_draft_confidence, csrc/draft_confidence.hip): k_row[b] is rewritten INSIDE every
  // step by the judgement launches of the draft loop (K at the start of a step, i + 1 once forward i's confidence stops the row) and
  // read where per-row adaptive K reads it; the step's last launch puts k_row and the gate words back. The two modes exclude each other.
  int conf;             // 0 = off
  int32_t* conf_gate;   // [8]    word i gates draft forward i (runs iff word > i): 0 between steps, i + 1 once a row continues past
                        //        forward i - 1; forwards below min_k are not gated
  // one-sequence loops with a persistent draft: which form of draft forward 0 the NEXT step needs. {2, 1}: the 2-token
  // pass over (prev, last) — prev's K/V are not in the draft cache yet (all k proposals were accepted: d_k was never an
  // input, or the host has just set the row); {1, 2}: prev's K/V are there, the 1-token pass over `last` is enough.
  // Both passes are in the captured step; each returns at entry unless its word is > 1 (SD_SKIP_IF_INACTIVE).
  int32_t* fwd0_w;      // [2]    null: always the 2-token pass
};

int launch_draft_next(int M, int i, const SpecState& s, const int32_t* skip_k, hipStream_t st);
int launch_draft_finalize(const float* part_val, const int* part_idx, int grid, int M, int i, int32_t* ids, const SpecState& s,
                          const int32_t* skip_k, int skip_i, hipStream_t st);
int launch_argmax_value(const float* part_val, const int* part_idx, int T, int grid, int M, int stride, float* vals, hipStream_t st);
int launch_medusa_fill(const SpecState& s, hipStream_t st);
int launch_medusa_rows(const SpecState& s, int32_t* row_idx, hipStream_t st);
int launch_medusa_commit(const SpecState& s, hipStream_t st);
int launch_medusa_gather(const void* x, const int32_t* rows, void* out, int B, int d, hipStream_t st);
int launch_eagle_extrapolate(const void* x, void* H, void* prev, int32_t* has_prev, const void* norm_w, const void* norm_b,
                             float eps, float alpha, int d, int B, int K, int rms, hipStream_t st);
int launch_accept(const SpecState& s, int mode, int use_sampled, hipStream_t st);
int launch_accept_len(const SpecState& s, hipStream_t st);
int launch_pack_record(const SpecState& s, int32_t* rec_slots, int rec_ints, int32_t* step_counter, const unsigned* draft_status,
                       const unsigned* target_status, hipStream_t st);
bool verify_tail_fits(const SpecState& s);
int launch_verify_tail(const SpecState& s, const float* part_val, const int* part_idx, int grid, int mode, int32_t* rec_slots,
                       int rec_ints, int32_t* step_counter, const unsigned* draft_status, const unsigned* target_status, hipStream_t st);

// ---- host-side parameter bundles of the sampling stage: the step (csrc/spec_loop.hip) keeps one per mode, the C-ABI ops build
// them from their arguments, and each launcher unpacks them into the argument structs of its kernels (no kernel receives one).

// How a row is shaped and which Philox values it consumes
struct DrawSpec {
  float temperature = 1.0f;
  int top_k = 0;                           // 0: no top-k cut (speculative sampling: the plain distributions; else 1..1024: both shaped)
  float top_p = 1.0f;                      // >= 1: no nucleus cut
  uint64_t seed = 0;
  uint32_t* draw = nullptr;                // nullable [B]: per-row draw counters, read and advanced on the device
  uint32_t draw0 = 0;                      // draw index when `draw` is null (the step always has counters)
  const int32_t* stream_id = nullptr;      // nullable [B]: Philox stream of row b (default b)
  const sd_row_sampling* table = nullptr;  // device [B] per-row parameters: the _rows kernels read temperature, top_k, top_p and seed
                                           // from table[b] at run time and the four scalars above are not in the launch
};

// The acceptance rule of csrc/typical_accept.hip
struct AcceptRule {
  int rule = SD_ACCEPT_OFF;   // sd_accept_rule
  float temperature = 1.0f, epsilon = 1.0f, delta = 1.0f;
  int agree_k = 1;
};

// csrc/sample.hip: the step's draw of the token after the accepted prefix, from row accept_len[b] of the verify logits
int launch_sample_step(const SpecState& s, const void* logits, int V, const DrawSpec& d, hipStream_t st);

// csrc/spec_sample.hip: speculative sampling inside the step
int launch_spec_draft_draw(const SpecState& s, const void* src, int src_rows_per_b, int src_row, void* q, int i, int V, const DrawSpec& d,
                           hipStream_t st);
int launch_spec_step(const SpecState& s, const void* target_logits, const void* draft_logits, int V, const DrawSpec& d, int32_t* flag,
                     int32_t* cand, hipStream_t st);

// csrc/typical_accept.hip: lossy acceptance (typical / top-k agreement) on the stored verify rows. workspace:
// typical_accept_workspace(B, K) bytes; next_from_ids: s.sampled[b] = target_ids[b][accept_len[b]] (no sampled bonus follows)
int check_typical_params(const char* who, const AcceptRule& r, int K, int V);
size_t typical_accept_workspace(int B, int K);
int launch_typical_step(const SpecState& s, const void* logits, int V, const AcceptRule& r, bool next_from_ids, void* workspace,
                        hipStream_t st);

// csrc/token_logprobs.hip: log-prob, rank and top-N alternatives of every token the step emitted, from the stored verify rows into
// the pinned block [2][B][K+1][logprob_words(V, top_n)] (slot = the parity of *step_counter, as the step record of the same launch)
int check_logprob_params(const char* who, int V, int top_n);
int logprob_words(int V, int top_n);
int launch_step_logprobs(const SpecState& s, const void* logits, int V, int top_n, const int32_t* step_counter, int32_t* host_words,
                         hipStream_t st);

// csrc/draft_confidence.hip: the judgement after draft forward i of the confidence-gated step. rows: the last position's bf16 row of
// batch row b at rows + b * row_stride elements. Gated like the forward it follows (skip_k / skip_i); a continuing row opens
// s.conf_gate[i + 1]. first: the step's first judgement also fills the other slots of conf_out's row with NaN.
struct ConfRule {
  float tau = 1.0f;
  int min_k = 1;
  float* conf_out = nullptr;   // nullable [B][K]
};
int launch_confidence_judge(const SpecState& s, const uint16_t* rows, long long row_stride, int V, int i, const ConfRule& r, bool first,
                            const int32_t* skip_k, int skip_i, hipStream_t st);

// csrc/grammar.hip: token automata (grammar-constrained decoding). next: uint16 [S][V], 0xFFFF = the token is not allowed in the
// state; allow: the same as one bit per token, uint32 [S][ceil(V / 32)]. A row's state: -1 unconstrained, 0..S-1, else DEAD
// (only eos is allowed; kept as kFsmDead).
constexpr int kFsmDead = 0xFFFF;
constexpr int kFsmMaxStates = 65534;
constexpr uint16_t kBf16NegInf = 0xff80u;
struct FsmBind {
  const uint16_t* next;
  const uint32_t* allow;
  int S;
  const int32_t* state;   // [B]
  int eos_id;
  int32_t* pos;           // nullable [B][pos_stride]: the state after the row's first n in-step tokens at [b][n] (the step's chain)
  int pos_stride;
};
__device__ __forceinline__ int fsm_step(const uint16_t* next, int S, int V, int s, int tok) {
  if (s < 0) return -1;
  if (s >= S || tok < 0 || tok >= V) return kFsmDead;
  const int nx = next[static_cast<size_t>(s) * V + tok];
  return nx >= S ? kFsmDead : nx;
}
size_t fsm_mask_bytes(int S, int V);
int launch_fsm_build_masks(const uint16_t* next, int S, int V, uint32_t* allow, size_t allow_bytes, hipStream_t st);
int launch_fsm_advance(const uint16_t* next, int S, int V, int32_t* fsm_state, int B, const int32_t* tokens, int tok_stride,
                       const int32_t* n_new, int max_new, const int32_t* active, hipStream_t st);

// csrc/logit_proc.hip: logit processors (penalties, bias) on stored bf16 rows, in place; the step and the C-ABI ops run these.
struct LogitStage {
  const uint16_t* counts = nullptr;        // [B][V]
  const float* bias = nullptr;             // [B][V] or null
  float rp = 1.0f, presence = 0.f, frequency = 0.f;
  void* workspace = nullptr;               // argmax partials of a launch with ids_out (logit_process_workspace), else unused
  size_t workspace_bytes = 0;
  const FsmBind* fsm = nullptr;            // nullable: the grammar line, folded into the same launch
  const sd_row_sampling* table = nullptr;  // device [B] per-row penalties (the three above are not in the launch), else null
};
// row (b, r) of the launch at rows + (b * R + r) * row_stride
struct LogitRows {
  void* rows;
  long long row_stride;
  int B, R, V;
};
size_t logit_process_workspace(int B, int R, int V);
// n_tokens < 0: row (b, r) is conditioned on the first r in-step tokens of tokens + b * tok_stride, else every row on the first n_tokens
int launch_logit_process(const LogitRows& rows, const LogitStage& g, const int32_t* tokens, int tok_stride, int n_tokens,
                         const int32_t* active, int32_t* ids_out, int ids_stride, hipStream_t st);
int launch_logit_counts_set(uint16_t* counts, int B, int V, int b, const int32_t* prompt, int n_prompt, const int32_t* gen, int n_gen,
                            hipStream_t st);
int launch_logit_counts_add(uint16_t* counts, int B, int V, const int32_t* tokens, int tok_stride, const int32_t* n_new, int max_new,
                            const int32_t* active, hipStream_t st);

}  // namespace sd
