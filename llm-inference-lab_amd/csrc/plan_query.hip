// Plan queries that need no GPU: which kernel instance, work split or refusal a shape gets, asked from dimensions alone
// (sd_prefill_plan, sd_prefill_plan_tables, sd_gemm_plan, sd_gemv_variant, sd_gemv_instance, sd_attention_plan, sd_persist_plan) or from a model's
// (sd_model_matrix_shape). Each asks the function the launch itself consults; nothing is enqueued. Host-side C++ behind the C-ABI.

#include <stdarg.h>
#include <string.h>

#include "engine.h"

namespace sd {

// Where a name (or reason) goes: the caller's buffer, and how a refusal speaks of it. who: the entry's prefix; cap_word / what:
// "name_cap" / "name", "reason_cap" / "reason" or "cap" / "name"; n_min: 1 for a name, 0 for a reason that may be empty.
struct TextOut { const char *who, *cap_word, *what; int n_min; char* out; size_t cap; };
// `text` holds n bytes, snprintf's return value into a local buffer of `room` bytes: checked against the caller's cap, copied with its NUL
static int return_text(const TextOut& o, const char* text, int n, size_t room) {
  SD_REQUIRE(n >= o.n_min && static_cast<size_t>(n) < room && static_cast<size_t>(n) < o.cap, "%s: %s=%zu is too short for the %s (%d bytes with its NUL)",
             o.who, o.cap_word, o.cap, o.what, n + 1);
  memcpy(o.out, text, static_cast<size_t>(n) + 1);
  return 0;
}
// the same for a text formatted here
__attribute__((format(printf, 2, 3))) static int return_textf(const TextOut& o, const char* fmt, ...) {
  char text[96];
  va_list ap;
  va_start(ap, fmt);
  const int n = vsnprintf(text, sizeof(text), fmt, ap);
  va_end(ap);
  return return_text(o, text, n, sizeof(text));
}

// w8 of the gemv queries: 0 bf16, 1 fp8, 2 bf16 with a W12 copy, 3 with a W12S copy
static int w12_form_of(int w8) { return w8 == 2 ? W12_CODES : w8 == 3 ? W12_SPLIT : W12_NONE; }

// the ranges sd_gemv_variant and sd_gemv_instance share
static int gemv_query_checks(const char* who, int T, int n_pairs, int K, int prologue, int epi) {
  SD_REQUIRE(T >= 1 && T <= kGemvMaxT, "%s: T=%d out of range 1..%d", who, T, kGemvMaxT);
  SD_REQUIRE(prologue >= PRO_NONE && prologue <= PRO_LAYERNORM && epi >= EPI_QKV_ROPE && epi <= EPI_ARGMAX,
             "%s: prologue=%d epi=%d out of range", who, prologue, epi);
  SD_REQUIRE(n_pairs >= 1 && K >= 8 && K % 8 == 0, "%s: n_pairs=%d K=%d (K must be a multiple of 8)", who, n_pairs, K);
  return 0;
}

// the model dimensions sd_prefill_plan(_tables) and sd_persist_plan (which also takes a vocabulary) accept
static int dimension_checks(const char* who, int d_model, int n_heads, int n_kv_heads, int head_dim, int d_ff, int vocab = 1) {
  SD_REQUIRE(d_model >= 1 && n_heads >= 1 && n_kv_heads >= 1 && head_dim >= 1 && d_ff >= 1 && vocab >= 1 && d_model <= (1 << 20) &&
                 n_heads <= (1 << 12) && n_kv_heads <= (1 << 12) && head_dim <= (1 << 12) && d_ff <= (1 << 22) && vocab <= (1 << 24),
             "%s: a dimension is below 1 or beyond any model", who);
  return 0;
}

// the model the plan queries build from dimensions alone (no weights are read)
static int prefill_plan_config(int arch, int d_model, int n_heads, int n_kv_heads, int head_dim, int d_ff, int which, int T, sd_model_config& c) {
  SD_REQUIRE(which >= 0 && which <= 3, "prefill_plan: which=%d (0 qkv, 1 out, 2 gate / up, 3 down)", which);
  SD_REQUIRE(T >= 1 && T <= kPrefillChunk, "prefill_plan: T=%d (a chunk holds 1 .. %d positions)", T, kPrefillChunk);
  if (int rc = dimension_checks("prefill_plan", d_model, n_heads, n_kv_heads, head_dim, d_ff)) return rc;
  c = sd_model_config{};
  c.arch = arch; c.n_layers = 1; c.d_model = d_model; c.n_heads = n_heads; c.n_kv_heads = n_kv_heads; c.head_dim = head_dim; c.d_ff = d_ff;
  c.vocab = 2;
  return 0;
}

}  // namespace sd

// ============================================================================ C-ABI
using namespace sd;

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
  const TextOut nm{"prefill_plan", "name_cap", "name", 1, name, name_cap}, why{"prefill_plan", "reason_cap", "reason", 0, reason, reason_cap};
  if (int rc = refusal ? return_textf(nm, "none") : return_textf(nm, "mfma<rf%d,%s>", pl.variant == 0 ? 4 : 2, w8 ? "fp8" : "bf16")) return rc;
  if (int rc = return_textf(why, "%s", refusal ? refusal : "")) return rc;
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
  const TextOut nm{"gemm_plan", "cap", "name", 1, out, cap};
  if (T <= kGemvMaxT) return return_textf(nm, "gemv");
  char name[64];
  const int n = gemm_plan_name(gemm_plan(T, n_pairs, K, w8 != 0, prologue, epi, flags), epi, w8 != 0, name, sizeof(name));
  return return_text(nm, name, n, sizeof(name));
}

extern "C" int sd_gemv_variant(int T, int n_pairs, int K, int w8, int prologue, int epi, char* out, size_t cap) {
  clear_error();
  SD_REQUIRE(out, "gemv_variant: NULL out");
  if (int rc = gemv_query_checks("gemv_variant", T, n_pairs, K, prologue, epi)) return rc;
  char name[64];
  const int n = gemv_variant_name(T, n_pairs, K, w8 == 1, prologue, epi, name, sizeof(name), w12_form_of(w8));
  return return_text({"gemv_variant", "cap", "name", 1, out, cap}, name, n, sizeof(name));
}

extern "C" int sd_gemv_instance(int T, int n_pairs, int K, int w8, int prologue, int epi, char* out, size_t cap) {
  clear_error();
  SD_REQUIRE(out, "gemv_instance: NULL out");
  if (int rc = gemv_query_checks("gemv_instance", T, n_pairs, K, prologue, epi)) return rc;
  char name[64];
  int n = 0;
  if (int rc = gemv_instance_name(T, n_pairs, K, w8 == 1, prologue, epi, name, sizeof(name), &n, w12_form_of(w8))) return rc;   // a launch launch_gemv refuses, in its words
  return return_text({"gemv_instance", "cap", "name", 1, out, cap}, name, n, sizeof(name));
}

extern "C" int sd_attention_plan(int n_q_heads, int n_kv_heads, int head_dim, int B, int M, int l_max, int paged, int* tiles, int* n_split,
                                 int* grid_x, int* grid_y, int* grid_z) {
  clear_error();
  SD_REQUIRE(tiles && n_split && grid_x && grid_y && grid_z, "attention_plan: NULL argument");
  // (AttnArgs holds M and the head counts in 8 bits each)
  SD_REQUIRE(n_q_heads >= 1 && n_q_heads <= 255 && n_kv_heads >= 0 && n_kv_heads <= 255 && M <= 255 && B <= (1 << 16),
             "attention_plan: Hq=%d Hkv=%d M=%d B=%d beyond what a launch holds (heads and M <= 255)", n_q_heads, n_kv_heads, M, B);
  int page_shift = -1;   // paged: 0 = dense rows, else positions per page (a power of two; any other length is refused as the launch would)
  if (paged != 0) {
    page_shift = 0;
    while (page_shift < 30 && (1 << page_shift) < paged) ++page_shift;
    if (paged < 0 || (1 << page_shift) != paged) page_shift = 0;
  }
  AttnPlan pl{};
  if (int rc = attention_plan(n_q_heads, n_kv_heads, head_dim, B, M, l_max, page_shift, true, kAttnSplitSlots, pl)) return rc;
  *tiles = pl.tiles;
  *n_split = pl.n_split;
  *grid_x = pl.grid_x;
  *grid_y = pl.grid_y;
  *grid_z = pl.grid_z;
  return 0;
}

extern "C" int sd_persist_plan(int arch, int n_layers, int d_model, int n_heads, int n_kv_heads, int head_dim, int d_ff, int vocab,
                               int packed, int weight_dtype, int has_bias, int T, int* eligible, int* max_tokens, int* ring_bytes,
                               char* name, size_t name_cap, char* reason, size_t reason_cap) {
  clear_error();
  SD_REQUIRE(eligible && max_tokens && ring_bytes && name && reason, "persist_plan: NULL argument");
  SD_REQUIRE(T >= 1, "persist_plan: T=%d", T);
  SD_REQUIRE(weight_dtype == SD_BF16 || weight_dtype == SD_FP8_E4M3, "persist_plan: weight_dtype=%d (SD_BF16 or SD_FP8_E4M3)", weight_dtype);
  if (int rc = dimension_checks("persist_plan", d_model, n_heads, n_kv_heads, head_dim, d_ff, vocab)) return rc;
  sd_model_config c{};
  c.arch = arch; c.n_layers = n_layers; c.d_model = d_model; c.n_heads = n_heads; c.n_kv_heads = n_kv_heads;
  c.head_dim = head_dim; c.d_ff = d_ff; c.vocab = vocab; c.weight_dtype = weight_dtype;
  // (one row of T tokens: a pass of B rows x M tokens stages the attention state of M tokens only and leaves no less)
  const PersistPlan pl = persist_plan(c, packed != 0, weight_dtype != SD_BF16, has_bias != 0, kPersistCUs, T, T);
  const TextOut nm{"persist_plan", "name_cap", "name", 1, name, name_cap}, why{"persist_plan", "reason_cap", "reason", 0, reason, reason_cap};
  if (int rc = pl.D ? return_textf(nm, "persist<%d,%d>", pl.D, pl.HC) : return_textf(nm, "none")) return rc;
  if (int rc = pl.refusal ? return_textf(why, "%s", pl.refusal)
               : !pl.D    ? return_textf(why, "tokens: T=%d above the %d a pass of this model holds", T, pl.max_tokens)
                          : return_textf(why, "%s", ""))
    return rc;
  *eligible = pl.refusal ? 0 : 1;
  *max_tokens = pl.max_tokens;
  *ring_bytes = static_cast<int>(pl.ring_bytes);
  return 0;
}
