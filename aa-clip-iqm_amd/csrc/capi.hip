// C ABI of libaaclip_hip.so (declared in include/aaclip.h): argument checks,
// workspace carving and kernel sequencing.  No allocation, no synchronisation:
// every entry point only enqueues kernels on the caller's stream.
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bf16x3.h"
#include "buffers.h"
#include "kernels.h"
#include "overlay_plan.h"
#include "png_plan.h"
#include "tile_plan.h"

using namespace aaclip;

static thread_local char g_err[512] = "";
// Tail overlap (tail_plan.h), decided per product from the pricing in profiles/ln_tail_overlap_pricing.txt
static constexpr bool TAIL_LN_OUT_PROJ = true, TAIL_LN_C_PROJ = true;
static int g_ln_fold = 1;   // aaclip_set_gemm_variant bit 17 turns the LayerNorm folding off (A/B measurements)

static int fail(int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}
// "<entry>: <msg>" as a REQUIRE message, for a name known only at run time (a body that several entries share)
static const char* in(const char* entry, const char* msg) {
  static thread_local char text[256];
  snprintf(text, sizeof(text), "%s: %s", entry, msg);
  return text;
}
// nullptr, or why a plan struct is refused before any of its fields is read; mismatch names the struct
template <class Plan> static const char* plan_refusal(const Plan* plan, const char* mismatch) {
  return !plan ? "null plan" : plan->struct_bytes == sizeof(Plan) ? nullptr : mismatch;
}
#define REQUIRE(cond, msg) \
  do {                     \
    if (!(cond)) return fail(-1, msg); \
  } while (0)
// fp32 rows are moved as 16-byte vectors: every pointer named must be 16-byte aligned (NULL passes)
#define REQUIRE_ALIGNED16(what, ...)                                            \
  do {                                                                          \
    const void* ptrs_[] = {__VA_ARGS__};                                        \
    for (const void* p_ : ptrs_)                                                \
      if ((uintptr_t)p_ & 15) return fail(-1, in(what, "pointers must be 16-byte aligned")); \
  } while (0)
#define REQUIRE_ROW_WIDTH(D) \
  do {                       \
    if (const char* m_ = row_width_check(D)) return fail(-1, m_); \
  } while (0)

static int finish(const char* what) {
  if (const char* le = take_launch_error()) {   // a launcher was asked for a kernel it does not have: nothing ran for it
    snprintf(g_err, sizeof(g_err), "%s: %s", what, le);
    (void)hipGetLastError();
    return -4;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return -2;
  }
  return 0;
}

// ---- optional in-stream timing of tagged kernels (bench.py roofline leg) ----
// Tags: 0 ln, 1 qkv gemm, 2 attention, 3 out_proj gemm, 4 c_fc gemm, 5 c_proj gemm, 6 adapter
struct ProfSlot { hipEvent_t a, b; int tag; };
static ProfSlot* g_prof = nullptr;
static int g_prof_cap = 0, g_prof_n = 0;
static unsigned g_prof_mask = 0;
struct ProfScope {
  int idx;
  hipStream_t s;
  ProfScope(int tag, hipStream_t st) : idx(-1), s(st) {
    if (g_prof_mask & (1u << tag)) {
      if (g_prof_n < g_prof_cap) {
        idx = g_prof_n++;
        g_prof[idx].tag = tag;
        (void)hipEventRecord(g_prof[idx].a, s);
      }
    }
  }
  ~ProfScope() {
    if (idx >= 0) (void)hipEventRecord(g_prof[idx].b, s);
  }
};

// bytes per element of an activation / weight row in the compute dtype (a split fp16 value is a hi and a lo half)
static inline size_t esize(int dtype) { return (dtype == AACLIP_F32 || dtype == AACLIP_F16X2) ? 4 : 2; }
static inline int split_w(int dtype) { return dtype == AACLIP_F16X2 ? 2 : 1; }   // row stride factor of split rows
static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
static inline bool dtype_ok(int d) { return d == AACLIP_F32 || d == AACLIP_F16 || d == AACLIP_BF16 || d == AACLIP_F16X2; }
static inline bool plain_dtype_ok(int d) { return d == AACLIP_F32 || d == AACLIP_F16 || d == AACLIP_BF16; }
// A launch takes its grid in work-items: workgroups * 256 threads must stay below 2^32.  Measured on gfx950 with
// head_expand: 2^24 - 1 workgroups run, exactly 2^24 is a launch error, and 2^24 + k silently runs k of them.  The
// entries whose kernels take one workgroup per row (group) therefore refuse a row count that needs 2^24 or more.
static inline bool grid_fits(long workgroups) { return workgroups < (1L << 24); }
static inline bool rows4_fit(long rows) { return grid_fits((rows + 3) / 4); }   // four rows per workgroup
#define TOO_MANY_ROWS4(entry) entry ": too many rows (one workgroup per 4 rows, below 2^24 workgroups: rows <= 2^26 - 4)"
// shape limits shared by the map entry points (anomaly_map.hip, iqm.hip, train_loss.hip)
static inline bool map_shape_ok(int B, int g, int S) { return B > 0 && B <= 65535 && g >= 1 && g <= 40 && S >= 1; }

// out[M, ldc] = A[M, lda] . W[N, K]^T (+ bias): the fields every product sets; every other field is zero (= off) and
// the call site sets the ones its epilogue needs
static GemmParams gemm_params(const void* A, long lda, const void* W, const float* bias, void* out, long ldc, int M,
                              int N, int K) {
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.A = A; p.lda = lda; p.W = W; p.bias = bias; p.out = out; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
  return p;
}

extern "C" {

int aaclip_profile_begin(unsigned tag_mask, int capacity) {
  if (capacity > g_prof_cap) {
    ProfSlot* n = (ProfSlot*)realloc(g_prof, sizeof(ProfSlot) * capacity);
    if (!n) return fail(-3, "profile: out of memory");
    g_prof = n;
    for (int i = g_prof_cap; i < capacity; ++i) {
      if (hipEventCreate(&g_prof[i].a) != hipSuccess || hipEventCreate(&g_prof[i].b) != hipSuccess)
        return fail(-2, "profile: hipEventCreate failed");
    }
    g_prof_cap = capacity;
  }
  g_prof_n = 0;
  g_prof_mask = tag_mask;
  return 0;
}

int aaclip_profile_end(float* ms, int* tags, int max_n) {
  g_prof_mask = 0;
  int n = g_prof_n < max_n ? g_prof_n : max_n;
  for (int i = 0; i < n; ++i) {
    if (hipEventSynchronize(g_prof[i].b) != hipSuccess) return fail(-2, "profile: event sync failed");
    float t = 0.f;
    if (hipEventElapsedTime(&t, g_prof[i].a, g_prof[i].b) != hipSuccess) return fail(-2, "profile: elapsed failed");
    ms[i] = t;
    tags[i] = g_prof[i].tag;
  }
  g_prof_n = 0;
  return n;
}

int aaclip_set_gemm_variant(int v) {
  REQUIRE(v >= 0 && (v >> 18) == 0 && !(v & (1 << 16)), "set_gemm_variant: unknown bits");
  // Validate everything before changing anything: a rejected call leaves the selection as it was.
  const int gv = v & 0xFF, av = (v >> 8) & 0xFF;
  REQUIRE((gv <= 1 || (gv >= 80 && gv <= 82)) && av <= 1,
          "set_gemm_variant: no such kernel variant (GEMM variants are 0/1/80/81/82, attention variants 0/1)");
  set_gemm_variant(gv);
  set_attn_variant(av);   // bits 8..15: attention kernel selection
  g_ln_fold = ((v >> 17) & 1) ? 0 : 1;
  return 0;
}

int aaclip_set_tail_overlap(int on) {
  set_tail_overlap(on != 0);
  return 0;
}

int aaclip_set_plan_cus(int cus) {
  REQUIRE(cus == 0 || (cus >= 8 && cus % 8 == 0 && cus <= 1024), "set_plan_cus: 0 (the device's count) or a multiple of 8, 8 .. 1024");
  set_plan_cus(cus);
  return 0;
}

long aaclip_tail_overlap_count(void) { return tail_launch_count(); }

int aaclip_version(void) { return AACLIP_ABI_VERSION; }
const char* aaclip_last_error(void) { return g_err; }

// The block / head workspace, byte offsets from its start (narrow starts at 0).  This is the only place that knows it:
//   [narrow: rows*max(D,640)*es] [big: rows * max(3D, F) in the compute dtype, or D / E floats]
//   [reserved: rows floats, read by nothing] [aux, LayerNorm folding: x16 | partials | rowab] + 4096 slack
// x16: 16-bit copy of the residual rows; partials: per-row partial sums [rows][D/64][2]; rowab: per-row (a, b) pairs
struct WsLayout { size_t narrow_bytes, big, big_bytes, reserved, x16, partials, rowab, total; };
static WsLayout ws_layout(int dtype, long rows, int D, int F, int E) {
  const size_t es = esize(dtype);
  size_t wide = (size_t)rows * (size_t)(3 * D > F ? 3 * D : F) * es;
  size_t f32d = (size_t)rows * D * 4;
  size_t f32e = (size_t)rows * (E > 0 ? E : 1) * 4;
  WsLayout l;
  l.narrow_bytes = up256((size_t)rows * (D > 640 ? D : 640) * es);
  l.big = l.narrow_bytes;
  l.big_bytes = wide > f32d ? wide : f32d;
  if (f32e > l.big_bytes) l.big_bytes = f32e;
  l.reserved = l.big + up256(l.big_bytes);
  l.x16 = l.reserved + up256((size_t)rows * 4);
  l.partials = l.x16 + up256((size_t)rows * D * es);
  l.rowab = l.partials + up256((size_t)rows * (D / 64 + 1) * 2 * 4);
  l.total = l.rowab + up256((size_t)rows * 2 * 4) + 4096;
  return l;
}

size_t aaclip_workspace_bytes(int dtype, long rows, int D, int F, int E) { return ws_layout(dtype, rows, D, F, E).total; }

int aaclip_layernorm(const float* x, const float* w, const float* b, void* out, int out_dtype, long rows, int D,
                     float eps, void* stream) {
  REQUIRE(x && w && b && out, "layernorm: null pointer");
  REQUIRE(dtype_ok(out_dtype), "layernorm: bad dtype");
  REQUIRE(rows > 0, "layernorm: rows must be positive");
  REQUIRE(rows4_fit(rows), TOO_MANY_ROWS4("layernorm"));
  REQUIRE_ROW_WIDTH(D);
  launch_layernorm(out_dtype, x, w, b, out, rows, D, eps, (hipStream_t)stream);
  return finish("layernorm");
}

int aaclip_gemm(int dtype, int epi, const void* A, long lda, const void* W, const float* bias, void* out, long ldc,
                int M, int N, int K, int act, int scale_cols, float scale, void* stream) {
  REQUIRE(dtype_ok(dtype), "gemm: bad dtype");
  REQUIRE(epi >= AACLIP_EPI_BIAS && epi <= AACLIP_EPI_ACT_F32, "gemm: bad epilogue");
  GemmParams p = gemm_params(A, lda, W, bias, out, ldc, M, N, K);
  p.scale_cols = scale_cols; p.scale = scale; p.act = act;
  const char* m = gemm_check(dtype, epi, p);
  if (m) return fail(-1, m);
  launch_gemm(dtype, epi, p, (hipStream_t)stream);
  return finish("gemm");
}

// aaclip_attention / aaclip_attention_log2q behind their own dtype rules
static int attention_entry(int dtype, const void* qkv, void* ctx, int B, int L, int H, int causal, int log2q,
                           void* stream) {
  REQUIRE(qkv && ctx, "attention: null pointer");
  REQUIRE(B > 0 && L > 0 && H > 0, "attention: empty problem");
  REQUIRE(B <= 65535 && H <= 65535, "attention: grid limit");
  REQUIRE((long)L * 3 * 64 * H * 4 < (1L << 31), "attention: L * 3 * 64 * H * 4 must stay below 2^31 (32-bit row offsets)");
  REQUIRE((long)((L + 255) / 256) * H * B < (1L << 30), "attention: too many workgroups");
  launch_attention(dtype, qkv, ctx, B, L, H, causal, log2q, (hipStream_t)stream);
  return finish("attention");
}

int aaclip_attention(int dtype, const void* qkv, void* ctx, int B, int L, int H, int causal, void* stream) {
  REQUIRE(dtype_ok(dtype), "attention: bad dtype");
  return attention_entry(dtype, qkv, ctx, B, L, H, causal, 0, stream);
}

int aaclip_attention_log2q(int dtype, const void* qkv, void* ctx, int B, int L, int H, int causal, void* stream) {
  REQUIRE(dtype == AACLIP_F16 || dtype == AACLIP_BF16 || dtype == AACLIP_F16X2, "attention_log2q: 16-bit dtypes only");
  return attention_entry(dtype, qkv, ctx, B, L, H, causal, 1, stream);
}

int aaclip_adapter_mix(float* x, const float* a, long rows, int D, float weight, void* stream) {
  REQUIRE(x && a && rows > 0, "adapter_mix: bad arguments");
  REQUIRE(rows4_fit(rows), TOO_MANY_ROWS4("adapter_mix"));
  REQUIRE_ROW_WIDTH(D);
  launch_adapter_mix(x, a, rows, D, weight, (hipStream_t)stream);
  return finish("adapter_mix");
}

// The forms of the building blocks that only aaclip_block(s) selects, one entry each (include/aaclip.h, "The block
// path's forms of the building blocks").  Every refusal precedes the first launch.
int aaclip_gemm_fused(int dtype, int epi, const void* A, long lda, const void* W, const float* bias, void* out, long ldc,
                      int M, int N, int K, int act, int scale_cols, float scale, const aaclip_gemm_fused_args* f,
                      void* stream) {
  REQUIRE(f, "gemm_fused: null argument struct");
  REQUIRE(f->struct_bytes == sizeof(aaclip_gemm_fused_args),
          "gemm_fused: aaclip_gemm_fused_args.struct_bytes does not match this library (binding generated from another "
          "include/aaclip.h revision?)");
  REQUIRE(dtype_ok(dtype), "gemm_fused: bad dtype");
  REQUIRE(epi >= AACLIP_EPI_BIAS && epi <= AACLIP_EPI_ACT_F32, "gemm_fused: bad epilogue");
  REQUIRE(f->w_exact16 >= 0 && f->w_exact16 <= 1 && f->out_no_hi8 >= 0 && f->out_no_hi8 <= 1 && f->out_qk8 >= 0,
          "gemm_fused: w_exact16 and out_no_hi8 are 0 or 1, out_qk8 is a column count");
  GemmParams p = gemm_params(A, lda, W, bias, out, ldc, M, N, K);
  p.scale_cols = scale_cols; p.scale = scale; p.act = act;
  p.resid = f->resid; p.out16 = f->out16; p.stats_out = f->stats_out; p.row_ab = f->row_ab; p.col_s = f->col_s;
  p.w_exact16 = f->w_exact16; p.out_qk8 = f->out_qk8; p.out_no_hi8 = f->out_no_hi8;
  const char* m = gemm_check(dtype, epi, p);
  if (m) return fail(-1, m);
  const bool plain16 = dtype == AACLIP_F16 || dtype == AACLIP_BF16;
  REQUIRE(!p.resid || epi == EPI_BIAS_RESID, "gemm_fused: resid belongs to the residual epilogue");
  REQUIRE(!p.resid || !((uintptr_t)p.resid & 15), "gemm_fused: resid must be 16-byte aligned");
  REQUIRE((p.out16 != nullptr) == (p.stats_out != nullptr), "gemm_fused: out16 and stats_out are given together");
  REQUIRE(!p.out16 || (epi == EPI_BIAS_RESID && plain16 && gemm_routes_to_256t(dtype, p)),
          "gemm_fused: out16 / stats_out need the residual epilogue of an fp16 / bf16 product that runs a 256-row-tile "
          "kernel (M >= 4096, N a multiple of 256, GEMM variant other than 1)");
  REQUIRE(!p.out16 || !(((uintptr_t)p.out16 | (uintptr_t)p.stats_out) & 7), "gemm_fused: out16 / stats_out must be 8-byte aligned");
  REQUIRE((p.row_ab != nullptr) == (p.col_s != nullptr), "gemm_fused: row_ab and col_s are given together");
  REQUIRE(!p.row_ab || ((epi == EPI_BIAS || epi == EPI_BIAS_GELU) && plain16 && gemm_routes_to_256t(dtype, p)),
          "gemm_fused: row_ab / col_s need the bias or GELU epilogue of an fp16 / bf16 product that runs a 256-row-tile "
          "kernel (M >= 4096, N a multiple of 256, GEMM variant other than 1)");
  REQUIRE(!p.row_ab || (!((uintptr_t)p.row_ab & 7) && !((uintptr_t)p.col_s & 15)),
          "gemm_fused: row_ab must be 8-byte, col_s 16-byte aligned");
  REQUIRE(!p.w_exact16 || (dtype == AACLIP_F16X2 && K % 256 == 0),
          "gemm_fused: w_exact16 (3-plane weight) needs split fp16 and K a multiple of 256");
  REQUIRE(!p.out_no_hi8 || (dtype == AACLIP_F16X2 && epi == EPI_BIAS_GELU),
          "gemm_fused: out_no_hi8 belongs to the GELU epilogue of a split fp16 product");
  if (p.out_qk8) {
    REQUIRE(epi == EPI_BIAS && dtype == AACLIP_F16X2 && gemm_split_routes_to_256t(p),
            "gemm_fused: out_qk8 needs the bias epilogue of a split fp16 product that runs the 256-row-tile kernel "
            "(M >= 4096, N a multiple of 256, GEMM variant other than 1)");
    REQUIRE(p.out_qk8 % 64 == 0 && p.out_qk8 <= N, "gemm_fused: out_qk8 must be a multiple of 64 and at most N");
  }
  launch_gemm(dtype, epi, p, (hipStream_t)stream);
  return finish("gemm_fused");
}

int aaclip_ln_stats_finalize(const float* partials, float* row_ab, long rows, int D, float eps, void* stream) {
  REQUIRE(partials && row_ab, "ln_stats_finalize: null pointer");
  REQUIRE(!(((uintptr_t)partials | (uintptr_t)row_ab) & 7), "ln_stats_finalize: pointers must be 8-byte aligned");
  REQUIRE(rows > 0 && rows < (1L << 27), "ln_stats_finalize: rows must be in 1 .. 2^27 - 1");
  REQUIRE_ROW_WIDTH(D);
  launch_ln_stats_finalize(partials, row_ab, rows, D / 64, D, eps, (hipStream_t)stream);
  return finish("ln_stats_finalize");
}

int aaclip_adapter_mix_fold(int dtype, float* x, const float* a, long rows, int D, float weight, void* out16,
                            float* row_ab, void* stream) {
  REQUIRE(dtype == AACLIP_F16 || dtype == AACLIP_BF16, "adapter_mix_fold: fp16 or bf16 rows only");
  REQUIRE(x && a && out16 && row_ab && rows > 0, "adapter_mix_fold: bad arguments");
  REQUIRE(rows4_fit(rows), TOO_MANY_ROWS4("adapter_mix_fold"));
  REQUIRE(!(((uintptr_t)x | (uintptr_t)a) & 15) && !(((uintptr_t)out16 | (uintptr_t)row_ab) & 7),
          "adapter_mix_fold: x and a must be 16-byte, out16 and row_ab 8-byte aligned");
  REQUIRE_ROW_WIDTH(D);
  launch_adapter_mix_fold(dtype, x, a, rows, D, weight, out16, row_ab, (hipStream_t)stream);
  return finish("adapter_mix_fold");
}

int aaclip_attention_split(const void* qkv, void* ctx, int B, int L, int H, int causal, int log2q, int qk8, int hi8,
                           void* stream) {
  REQUIRE(qkv && ctx, "attention_split: null pointer");
  REQUIRE(B > 0 && L > 0 && H > 0, "attention_split: empty problem");
  REQUIRE(B <= 65535 && H <= 65535, "attention_split: grid limit");
  REQUIRE((long)L * 3 * 64 * H * 4 < (1L << 31), "attention_split: L * 3 * 64 * H * 4 must stay below 2^31 (32-bit row offsets)");
  REQUIRE((long)((L + 255) / 256) * H * B < (1L << 30), "attention_split: too many workgroups");
  REQUIRE(!qk8 || (log2q && attention_qk8_applicable(L, causal)),
          "attention_split: the e4m3 record form (qk8) needs q in log2 units, L >= 512 and no causal mask");
  launch_attention(AACLIP_F16X2, qkv, ctx, B, L, H, causal, log2q != 0, (hipStream_t)stream, hi8 != 0, qk8 != 0);
  return finish("attention_split");
}

int aaclip_layernorm_split(const float* x, const float* w, const float* b, void* out, long rows, int D, float eps,
                           int hi8, void* stream) {
  REQUIRE(x && w && b && out, "layernorm_split: null pointer");
  REQUIRE(rows > 0, "layernorm_split: rows must be positive");
  REQUIRE(rows4_fit(rows), TOO_MANY_ROWS4("layernorm_split"));
  REQUIRE_ROW_WIDTH(D);
  launch_layernorm(AACLIP_F16X2, x, w, b, out, rows, D, eps, (hipStream_t)stream, hi8 != 0);
  return finish("layernorm_split");
}

int aaclip_split_rows(const float* src, void* dst, long rows, int D, int hi8, void* stream) {
  REQUIRE(src && dst, "split_rows: null pointer");
  REQUIRE(!(((uintptr_t)src | (uintptr_t)dst) & 15), "split_rows: pointers must be 16-byte aligned");
  REQUIRE(rows > 0 && D > 0 && D % 8 == 0, "split_rows: rows must be positive, D a positive multiple of 8");
  launch_split_rows(src, dst, rows, D, (hipStream_t)stream, hi8 != 0);
  return finish("split_rows");
}

int aaclip_small_attention(int kv_dtype, const float* q, const void* k, const void* v, float* out, int B, int nq, int Lk,
                           int H, int hd, float scale, void* stream) {
  REQUIRE(plain_dtype_ok(kv_dtype), "small_attention: bad dtype (fp32, fp16 or bf16)");
  REQUIRE(q && k && v && out, "small_attention: null pointer");
  REQUIRE(B > 0 && B <= 65535 && H <= 65535, "small_attention: bad batch / heads");
  const char* m = small_attention_check(nq, Lk, H, hd);
  if (m) return fail(-1, m);
  launch_small_attention(kv_dtype, q, k, v, out, B, nq, Lk, H, hd, scale, (hipStream_t)stream);
  return finish("small_attention");
}

size_t aaclip_cross_rows_workspace_bytes(int B, int R, int Lk, int Dk) { return cross_rows_ws_bytes(B, R, Lk, Dk); }

int aaclip_cross_rows(int x_dtype, const float* qt, const void* x, float* out, int B, int R, int Lk, int Dk, void* ws,
                      size_t ws_bytes, void* stream) {
  REQUIRE(plain_dtype_ok(x_dtype), "cross_rows: bad dtype (fp32, fp16 or bf16)");
  REQUIRE(qt && x && out && ws, "cross_rows: null pointer");
  REQUIRE(B > 0 && B <= 65535, "cross_rows: bad batch");
  const char* m = cross_rows_check(R, Lk, Dk);
  if (m) return fail(-1, m);
  REQUIRE(ws_bytes >= cross_rows_ws_bytes(B, R, Lk, Dk), "cross_rows: workspace too small");
  launch_cross_rows(x_dtype, qt, x, out, ws, B, R, Lk, Dk, (hipStream_t)stream);
  return finish("cross_rows");
}

size_t aaclip_cross_rows_backward_workspace_bytes(int B, int R, int Lk, int Dk) {
  return cross_rows_backward_ws_bytes(B, R, Lk, Dk);
}

int aaclip_cross_rows_backward(int x_dtype, const float* qt, const void* x, const float* d_out, float* d_qt, float* d_x,
                               int act, int accumulate, int B, int R, int Lk, int Dk, void* ws, size_t ws_bytes,
                               void* stream) {
  REQUIRE(plain_dtype_ok(x_dtype), "cross_rows_backward: bad dtype (fp32, fp16 or bf16)");
  REQUIRE(qt && x && d_out && ws, "cross_rows_backward: null pointer");
  REQUIRE(d_qt || d_x, "cross_rows_backward: nothing to compute (d_qt and d_x are both NULL)");
  REQUIRE(act >= AACLIP_ACT_NONE && act <= AACLIP_ACT_RELU, "cross_rows_backward: bad activation");
  REQUIRE(B > 0 && R > 0 && Lk > 0 && Dk > 0, "cross_rows_backward: empty problem");
  REQUIRE(B <= 65535, "cross_rows_backward: grid limit (B <= 65535)");
  if (const char* m = cross_rows_check(R, Lk, Dk)) return fail(-1, in("cross_rows_backward", m));
  REQUIRE_ALIGNED16("cross_rows_backward", qt, x, d_out, d_qt, d_x, ws);
  REQUIRE(ws_bytes >= cross_rows_backward_ws_bytes(B, R, Lk, Dk), "cross_rows_backward: workspace too small");
  launch_cross_rows_backward(x_dtype, qt, x, d_out, d_qt, d_x, act, accumulate, B, R, Lk, Dk, ws, (hipStream_t)stream);
  return finish("cross_rows_backward");
}

size_t aaclip_cross_rows_levels_workspace_bytes(int B, int nseg, int Lk, int Dk) {
  if (B < 1 || nseg < 1 || Lk < 1 || Dk < 1) return 0;
  return cross_rows_levels_ws_bytes(B, nseg, Lk, Dk);
}

int aaclip_cross_rows_levels(int x_dtype, const float* qt, const void* const* x, int nseg, float* out, int B, int R,
                             int rows_per_image, int row0, int Lk, int Dk, long ldx, void* ws, size_t ws_bytes,
                             void* stream) {
  REQUIRE(qt && x && out && ws, "cross_rows_levels: null pointer");
  REQUIRE(B > 0 && B <= 65535, "cross_rows_levels: bad batch");
  const char* m = cross_rows_levels_check(x_dtype, R, nseg, Lk, Dk, ldx);
  if (m) return fail(-1, m);
  REQUIRE(row0 >= 0 && rows_per_image >= row0 + Lk, "cross_rows_levels: the keys [row0, row0 + Lk) must lie inside an image's rows");
  REQUIRE((long)rows_per_image * ldx * 2 < (1L << 31), "cross_rows_levels: an image's rows must span < 2 GiB");
  REQUIRE(ws_bytes >= cross_rows_levels_ws_bytes(B, nseg, Lk, Dk), "cross_rows_levels: workspace too small");
  for (int i = 0; i < nseg; ++i) REQUIRE(x[i] && ((uintptr_t)x[i] & 15) == 0, "cross_rows_levels: segment pointers must be 16-byte aligned");
  launch_cross_rows_levels(x_dtype, qt, x, nseg, out, ws, B, R, rows_per_image, row0, Lk, Dk, ldx, (hipStream_t)stream);
  return finish("cross_rows_levels");
}

size_t aaclip_cross_rows_levels_backward_workspace_bytes(int B, int R, int nseg, int Lk, int Dk) {
  return cross_rows_levels_backward_ws_bytes(B, R, nseg, Lk, Dk);
}

int aaclip_cross_rows_levels_backward(int x_dtype, const float* qt, const void* const* x, int nseg, const float* d_out,
                                      float* d_qt, float* const* d_x, int accumulate, int B, int R, int rows_per_image,
                                      int row0, int Lk, int Dk, long ldx, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(qt && x && d_out && ws, "cross_rows_levels_backward: null pointer");
  REQUIRE(d_qt || d_x, "cross_rows_levels_backward: nothing to compute (d_qt and d_x are both NULL)");
  REQUIRE(B > 0 && B <= 65535, "cross_rows_levels_backward: bad batch (1 <= B <= 65535)");
  if (const char* m = cross_rows_levels_backward_check(x_dtype, R, nseg, Lk, Dk, ldx)) return fail(-1, m);
  REQUIRE(row0 >= 0 && rows_per_image >= row0 + Lk,
          "cross_rows_levels_backward: the keys [row0, row0 + Lk) must lie inside an image's rows");
  REQUIRE((long)rows_per_image * ldx * 2 < (1L << 31), "cross_rows_levels_backward: an image's rows must span < 2 GiB");
  REQUIRE_ALIGNED16("cross_rows_levels_backward", qt, d_out, d_qt, ws);
  for (int i = 0; i < nseg; ++i) {
    REQUIRE(x[i] && ((uintptr_t)x[i] & 15) == 0, "cross_rows_levels_backward: segment pointers must be non-NULL and 16-byte aligned");
    if (d_x) REQUIRE(d_x[i] && ((uintptr_t)d_x[i] & 15) == 0, "cross_rows_levels_backward: d_x pointers must be non-NULL and 16-byte aligned");
  }
  REQUIRE(ws_bytes >= cross_rows_levels_backward_ws_bytes(B, R, nseg, Lk, Dk), "cross_rows_levels_backward: workspace too small");
  launch_cross_rows_levels_backward(x_dtype, qt, x, nseg, d_out, d_qt, d_x, accumulate, B, R, rows_per_image, row0, Lk, Dk,
                                    ldx, ws, (hipStream_t)stream);
  return finish("cross_rows_levels_backward");
}

int aaclip_head_expand(int dtype, const float* q, void* qm, long rows, int H, int D, float scale, void* stream) {
  REQUIRE(plain_dtype_ok(dtype), "head_expand: bad dtype (fp32, fp16 or bf16)");
  REQUIRE(q && qm && rows > 0 && H > 0 && D > 0 && D % H == 0, "head_expand: bad arguments");
  REQUIRE(rows < (1L << 24) && grid_fits(rows * H), "head_expand: too many rows (one workgroup per expanded row: rows * H < 2^24)");
  launch_head_expand(dtype, q, qm, rows, H, D, scale, (hipStream_t)stream);
  return finish("head_expand");
}

int aaclip_head_diag(const float* full, float* ctx, long rows, int H, int D, void* stream) {
  REQUIRE(full && ctx && rows > 0 && H > 0 && D > 0 && D % H == 0, "head_diag: bad arguments");
  REQUIRE(grid_fits(rows), "head_diag: too many rows (one workgroup per row: rows < 2^24)");
  launch_head_diag(full, ctx, rows, H, D, (hipStream_t)stream);
  return finish("head_diag");
}

int aaclip_residual_layernorm(const float* a, const float* b, const float* w, const float* bias, float* out, long rows,
                              int D, float eps, void* stream) {
  REQUIRE(a && w && bias && out, "residual_layernorm: null pointer");
  REQUIRE(rows > 0 && D > 0 && D % 64 == 0 && D <= 4096, "residual_layernorm: D must be a multiple of 64, <= 4096");
  REQUIRE(rows4_fit(rows), TOO_MANY_ROWS4("residual_layernorm"));
  launch_residual_layernorm(a, b, w, bias, out, rows, D, eps, (hipStream_t)stream);
  return finish("residual_layernorm");
}

int aaclip_combine3(const float* a, const float* b, const float* c, float wa, float wb, float wc, float* out, long n,
                    void* stream) {
  REQUIRE(a && out && n > 0, "combine3: bad arguments");
  launch_combine3(a, b, c, wa, wb, wc, out, n, (hipStream_t)stream);
  return finish("combine3");
}

int aaclip_linear_smallk(int out_dtype, const float* x, const float* W, const float* bias, void* y, long R, int N, int K,
                         void* stream) {
  REQUIRE(plain_dtype_ok(out_dtype), "linear_smallk: bad dtype (fp32, fp16 or bf16)");
  REQUIRE(x && W && y, "linear_smallk: null pointer");
  REQUIRE(R > 0 && N > 0 && K >= 1 && K <= 4, "linear_smallk: in_features must be 1..4");
  launch_linear_smallk(out_dtype, x, W, bias, y, R, N, K, (hipStream_t)stream);
  return finish("linear_smallk");
}

// ---- iqm_query_backward.hip
int aaclip_small_attention_backward(const float* q, const float* k, const float* v, const float* d_out, float* d_q,
                                    float* d_k, float* d_v, int B, int nq, int Lk, int H, int hd, float scale,
                                    void* stream) {
  REQUIRE(q && k && v && d_out, "small_attention_backward: null pointer");
  REQUIRE(d_q || d_k || d_v, "small_attention_backward: nothing to compute (d_q, d_k and d_v are all NULL)");
  REQUIRE(B > 0 && nq > 0 && Lk > 0 && H > 0 && hd > 0, "small_attention_backward: empty problem");
  REQUIRE(B <= 65535 && H <= 65535, "small_attention_backward: grid limit (B, H <= 65535)");
  REQUIRE(nq <= 4, "small_attention_backward: 1..4 queries per image");
  REQUIRE(Lk <= SAB_MAXK, "small_attention_backward: 1..256 keys");
  REQUIRE(hd % 4 == 0 && hd <= 128, "small_attention_backward: head size must be a multiple of 4, <= 128");
  REQUIRE_ALIGNED16("small_attention_backward", q, k, v, d_out, d_q, d_k, d_v);
  launch_small_attention_backward(q, k, v, d_out, d_q, d_k, d_v, B, nq, Lk, H, hd, scale, (hipStream_t)stream);
  return finish("small_attention_backward");
}

size_t aaclip_layernorm_param_grad_workspace_bytes(long rows, int D) {
  return rows4_fit(rows) ? layernorm_param_grad_ws_bytes(rows, D) : 0;
}

int aaclip_layernorm_param_grad(const float* x, const float* d_y, float* d_w, float* d_b, long rows, int D, float eps,
                                void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(x && d_y && ws, "layernorm_param_grad: null pointer");
  REQUIRE(d_w || d_b, "layernorm_param_grad: nothing to compute (d_w and d_b are both NULL)");
  REQUIRE(rows > 0 && D > 0, "layernorm_param_grad: empty problem");
  REQUIRE(D % 64 == 0 && D <= 4096, "layernorm_param_grad: D must be a multiple of 64, <= 4096");
  REQUIRE(rows4_fit(rows), TOO_MANY_ROWS4("layernorm_param_grad"));
  REQUIRE_ALIGNED16("layernorm_param_grad", x, d_y, d_w, d_b, ws);
  REQUIRE(ws_bytes >= layernorm_param_grad_ws_bytes(rows, D), "layernorm_param_grad: workspace too small");
  launch_layernorm_param_grad(x, d_y, d_w, d_b, rows, D, eps, ws, (hipStream_t)stream);
  return finish("layernorm_param_grad");
}

size_t aaclip_bias_grad_workspace_bytes(long rows, int N) { return bias_grad_ws_bytes(rows, N); }

int aaclip_bias_grad(const float* dz, long ldz, float* db, long rows, int N, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(dz && db && ws, "bias_grad: null pointer");
  REQUIRE(rows > 0 && N > 0, "bias_grad: empty problem");
  REQUIRE(ldz >= N, "bias_grad: ldz must be at least N");
  REQUIRE_ALIGNED16("bias_grad", dz, db, ws);
  REQUIRE(ws_bytes >= bias_grad_ws_bytes(rows, N), "bias_grad: workspace too small");
  launch_bias_grad(dz, ldz, db, rows, N, ws, (hipStream_t)stream);
  return finish("bias_grad");
}

int aaclip_act_backward(int act, const float* zy, const float* d_y, float* d_z, long n, void* stream) {
  REQUIRE(act == AACLIP_ACT_GELU || act == AACLIP_ACT_RELU, "act_backward: bad activation (GELU or RELU)");
  REQUIRE(zy && d_y && d_z, "act_backward: null pointer");
  REQUIRE(n > 0, "act_backward: empty problem");
  REQUIRE_ALIGNED16("act_backward", zy, d_y, d_z);
  launch_iqm_act_backward(act, zy, d_y, d_z, n, (hipStream_t)stream);
  return finish("act_backward");
}

size_t aaclip_linear_smallk_backward_workspace_bytes(long R, int N, int K) {
  return linear_smallk_backward_ws_bytes(R, N, K);
}

int aaclip_linear_smallk_backward(const float* x, const float* d_y, float* d_w, float* d_b, long R, int N, int K, void* ws,
                                  size_t ws_bytes, void* stream) {
  REQUIRE(x && d_y && ws, "linear_smallk_backward: null pointer");
  REQUIRE(d_w || d_b, "linear_smallk_backward: nothing to compute (d_w and d_b are both NULL)");
  REQUIRE(R > 0 && N > 0 && K > 0, "linear_smallk_backward: empty problem");
  REQUIRE(K <= 4, "linear_smallk_backward: in_features must be 1..4");
  REQUIRE_ALIGNED16("linear_smallk_backward", x, d_y, d_w, d_b, ws);
  REQUIRE(ws_bytes >= linear_smallk_backward_ws_bytes(R, N, K), "linear_smallk_backward: workspace too small");
  launch_linear_smallk_backward(x, d_y, d_w, d_b, R, N, K, ws, (hipStream_t)stream);
  return finish("linear_smallk_backward");
}

int aaclip_drop_cls_rows(int dtype, const void* src, void* dst, int B, int L, int E, int rows_per_image, int row_off,
                         void* stream) {
  REQUIRE(plain_dtype_ok(dtype), "drop_cls_rows: bad dtype (fp32, fp16 or bf16)");
  REQUIRE(src && dst, "drop_cls_rows: null pointer");
  REQUIRE(B > 0 && L > 1 && E > 0 && E % 8 == 0, "drop_cls_rows: E must be a multiple of 8");
  REQUIRE(row_off >= 0 && row_off + (L - 1) <= rows_per_image, "drop_cls_rows: rows do not fit the destination");
  launch_drop_cls_rows(dtype, src, dst, B, L, E, rows_per_image, row_off, (hipStream_t)stream);
  return finish("drop_cls_rows");
}

int aaclip_iqm_map(const float* const* seg, int NL, const float* queries, const float* base, float* out, int B, int g,
                   int E, int S, float w_base, float w_iqm, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(seg && queries && out && ws, "iqm_map: null pointer");
  REQUIRE(NL >= 1 && NL <= 4, "iqm_map: 1..4 levels");
  REQUIRE(map_shape_ok(B, g, S), "iqm_map: bad shape (grid <= 40)");
  REQUIRE_ROW_WIDTH(E);
  const int P = g * g;
  REQUIRE(ws_bytes >= (size_t)NL * B * P * 4, "iqm_map: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* grids = (float*)ws;
  for (int l = 0; l < NL; ++l) {
    REQUIRE(seg[l], "iqm_map: null level pointer");
    launch_iqm_scores(seg[l], queries, grids + (size_t)l * B * P, B, P, E, s);
  }
  launch_iqm_upsample(grids, base, out, B, g, S, NL, w_base, w_iqm, s);
  return finish("iqm_map");
}

int aaclip_patch_embed(const float* img, const void* conv_w, const float* cls, const float* pos,
                       const float* ln_pre_w, const float* ln_pre_b, float* x, int B, int H, int W, int ps, int D,
                       int dtype, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(dtype_ok(dtype), "patch_embed: bad dtype");
  REQUIRE(img && conv_w && cls && pos && ln_pre_w && ln_pre_b && x && ws, "patch_embed: null pointer");
  REQUIRE(B > 0 && ps > 0 && H >= ps && W >= ps, "patch_embed: bad image shape");
  REQUIRE_ROW_WIDTH(D);
  const int g = H / ps, gw = W / ps, P = g * gw, L = P + 1;
  const int K = 3 * ps * ps, Kpad = (K + 63) / 64 * 64;
  REQUIRE(Kpad <= 640, "patch_embed: 3*ps*ps must be <= 640");
  REQUIRE(ws_bytes >= (size_t)B * P * Kpad * esize(dtype), "patch_embed: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  GemmParams p = gemm_params(ws, split_w(dtype) * Kpad, conv_w, nullptr, x, D, B * P, D, Kpad);
  p.pos = pos; p.P = P; p.L = L;
  const char* m = gemm_check(dtype, EPI_PATCH, p);   // before the first launch: a rejected call enqueues nothing
  if (m) return fail(-1, m);
  launch_im2col(dtype, img, ws, B, 3, H, W, ps, Kpad, s);
  launch_gemm(dtype, EPI_PATCH, p, s);
  launch_cls_rows(x, cls, pos, B, L, D, s);
  launch_layernorm(AACLIP_F32, x, ln_pre_w, ln_pre_b, x, (long)B * L, D, 1e-5f, s);
  return finish("patch_embed");
}

// One block.  aux_in: the aux region of the workspace holds the current rows of x in the compute dtype and their
// (rstd, -mean*rstd) pairs, written by the previous block of the same aaclip_blocks call -- then ln_1 is folded
// into the QKV product.  want_out: produce them for the next block (from the c_proj epilogue, or from the adapter
// mix when the block has an adapter).  *aux_out tells the caller whether they were produced.
// x_in != x: the block READS the stream from x_in (left untouched) and continues it in x -- the first residual
// update (out_proj) takes its residual from x_in and writes x.
// Split fp16, FULL / CAUSAL attention: where a residual product leaves a partial last round, the LayerNorm after it runs
// beside that round (tail_plan.h; launch_gemm_resid_ln) and only its last rows as a pass.  ln_2 belongs to this block.
// ln_1 of the NEXT block (`next`, null: none) is produced by this block's c_proj: *ln1_out tells the caller that `narrow`
// holds those rows, and it hands that to the next block as ln1_in, which then skips its own ln_1 pass.
static int block_impl(const float* x_in, float* x, const aaclip_block_weights* w, float mix, int B, int L, int D, int H,
                      int F, int attn_mode, int dtype, void* ws, const WsLayout& l, hipStream_t s, bool aux_in,
                      bool want_out, bool* aux_out, bool ln1_in, const aaclip_block_weights* next, bool* ln1_out) {
  *aux_out = false;
  *ln1_out = false;
  REQUIRE(w->ln1_w && w->ln1_b && w->qkv_w && w->qkv_b && w->out_w && w->out_b && w->ln2_w && w->ln2_b && w->fc_w &&
              w->fc_b && w->proj_w && w->proj_b,
          "block: null weight pointer");
  const long rows = (long)B * L;
  const size_t es = esize(dtype);
  char* narrow = (char*)ws;
  char* big = narrow + l.big;
  char* x16 = narrow + l.x16;
  float* partials = (float*)(narrow + l.partials);
  float* rowab = (float*)(narrow + l.rowab);
  const int M = (int)rows;
  const bool folding = g_ln_fold && (dtype == AACLIP_F16 || dtype == AACLIP_BF16);
  const int sw = split_w(dtype);                    // split fp16 rows are [hi | lo]: twice the row stride
  const unsigned ex = dtype == AACLIP_F16X2 ? w->exact16 : 0u;   // weights whose lo half is all zero

  // ---- x += out_proj(attn(ln_1 x))
  // 16-bit path: fold log2(e) into the q scale (one rounding) so the attention kernel works in log2 units
  const int log2q = dtype != AACLIP_F32;
  const float qscale = log2q ? 0.125f * 1.4426950408889634f : 0.125f;
  const int qkv_exact = ex & AACLIP_EXACT16_QKV;
  const char* ctx = narrow;
  if (attn_mode == AACLIP_ATTN_VV_BATCH) {
    { ProfScope ps(0, s); launch_layernorm(dtype, x_in, w->ln1_w, w->ln1_b, narrow, rows, D, 1e-5f, s, !qkv_exact); }
    // only the value third of in_proj is needed; v lives behind the packed q|k|v buffer inside `big`, which holds
    // rows * max(3D, F) elements: blocks_core()'s F >= 4*D check is what makes room for it
    assert((size_t)rows * 4 * D * es <= l.big_bytes);
    char* vbuf = big + (size_t)rows * 3 * D * es;
    // rows 2D.. of the packed weight; a split8 weight row holds 4 (3: exact in fp16) bytes per element
    const char* v_w = (const char*)w->qkv_w + (size_t)2 * D * D * (dtype == AACLIP_F16X2 ? (qkv_exact ? 3 : 4) : es);
    GemmParams p = gemm_params(narrow, sw * D, v_w, w->qkv_b + 2 * D, vbuf, sw * D, M, D, D);
    p.w_exact16 = qkv_exact;
    { ProfScope ps(1, s); launch_gemm(dtype, EPI_BIAS, p, s); }
    {
      ProfScope ps(2, s);
      launch_vv_spread(dtype, vbuf, big, B, L, D, qscale, s);
      launch_attention(dtype, big, narrow, /*batches=*/L, /*sequence=*/B, H, 0, log2q, s, !(ex & AACLIP_EXACT16_OUT));
      launch_vv_regroup(dtype, narrow, vbuf, B, L, D, s);
    }
    ctx = vbuf;
  } else {
    GemmParams p = gemm_params(narrow, sw * D, w->qkv_w, w->qkv_b, big, sw * 3 * D, M, 3 * D, D);
    p.scale_cols = D; p.scale = qscale; p.w_exact16 = qkv_exact;
    if (aux_in && folding && w->qkv_w_fold && w->qkv_fold_s && w->qkv_fold_b && gemm_routes_to_256t(dtype, p)) {
      // ln_1 folded into the QKV product (include/aaclip.h, aaclip_block_weights)
      p.A = x16; p.W = w->qkv_w_fold; p.bias = w->qkv_fold_b; p.row_ab = rowab; p.col_s = w->qkv_fold_s;
    } else if (!ln1_in) {
      ProfScope ps(0, s);
      launch_layernorm(dtype, x_in, w->ln1_w, w->ln1_b, narrow, rows, D, 1e-5f, s, !qkv_exact);
    }
    // split fp16, long rows, 256-tile QKV kernel: q and k leave the epilogue as fp16 + e4m3 records and the attention
    // kernel runs its two correction products on the e4m3 MFMA (attention.hip, QK8)
    bool qk8 = false;
    if (dtype == AACLIP_F16X2 && log2q && attention_qk8_applicable(L, attn_mode == AACLIP_ATTN_CAUSAL)) {
      p.ldc = 5 * D; p.out_qk8 = 2 * D;
      qk8 = gemm_split_routes_to_256t(p);
      if (!qk8) { p.ldc = sw * 3 * D; p.out_qk8 = 0; }
    }
    { ProfScope ps(1, s); launch_gemm(dtype, EPI_BIAS, p, s); }
    { ProfScope ps(2, s); launch_attention(dtype, big, narrow, B, L, H, attn_mode == AACLIP_ATTN_CAUSAL, log2q, s, !(ex & AACLIP_EXACT16_OUT), qk8); }
  }
  GemmParams p = gemm_params(ctx, sw * D, w->out_w, w->out_b, x, D, M, D, D);
  p.w_exact16 = ex & AACLIP_EXACT16_OUT;
  if (x_in != x) p.resid = x_in;
  // ln_2 folded into c_fc: only where both products run on the kernels whose epilogue implements it;
  // everywhere else the ln_2 pass runs as before
  GemmParams fc = gemm_params(narrow, sw * D, w->fc_w, w->fc_b, big, sw * F, M, F, D);
  fc.w_exact16 = ex & AACLIP_EXACT16_FC;
  fc.out_no_hi8 = (ex & AACLIP_EXACT16_PROJ) ? 1 : 0;   // c_proj is the only reader of the GELU rows
  const bool fold2 = folding && w->fc_w_fold && w->fc_fold_s && w->fc_fold_b && gemm_routes_to_256t(dtype, p) &&
                     gemm_routes_to_256t(dtype, fc);
  if (fold2) {
    p.out16 = x16;
    p.stats_out = partials;
  }
  // rows of `narrow` (split8 rows: 4 * D bytes) whose LayerNorm a residual product's tail launch has produced
  const bool tail_ln = dtype == AACLIP_F16X2 && attn_mode != AACLIP_ATTN_VV_BATCH;
  long ln_done = 0;
  {
    ProfScope ps(3, s);
    if (tail_ln && TAIL_LN_OUT_PROJ) {
      const LnRows ln2 = {w->ln2_w, w->ln2_b, narrow, 1e-5f, !(ex & AACLIP_EXACT16_FC)};
      ln_done = launch_gemm_resid_ln(dtype, p, ln2, s);
    } else {
      launch_gemm(dtype, EPI_BIAS_RESID, p, s);
    }
  }
  // ---- x += c_proj(gelu(c_fc(ln_2 x)))
  if (fold2) {
    ProfScope ps(0, s);
    launch_ln_stats_finalize(partials, rowab, rows, D / 64, D, 1e-5f, s);
    fc.A = x16; fc.W = w->fc_w_fold; fc.bias = w->fc_fold_b; fc.row_ab = rowab; fc.col_s = w->fc_fold_s;
  } else {
    ProfScope ps(0, s);
    launch_layernorm(dtype, x + ln_done * D, w->ln2_w, w->ln2_b, narrow + ln_done * 4 * D, rows - ln_done, D, 1e-5f, s,
                     !(ex & AACLIP_EXACT16_FC));
  }
  { ProfScope ps(4, s); launch_gemm(dtype, EPI_BIAS_GELU, fc, s); }
  p = gemm_params(big, sw * F, w->proj_w, w->proj_b, x, D, M, D, F);
  p.w_exact16 = ex & AACLIP_EXACT16_PROJ;
  // the c_proj epilogue can also emit the new rows in 16 bits: input of the adapter product, or (with their
  // row sums) of the next block's folded ln_1
  const bool emit = folding && gemm_routes_to_256t(dtype, p) && (w->adapter_w || want_out);
  if (emit) {
    p.out16 = x16;
    p.stats_out = partials;
  }
  // the next block's ln_1 beside c_proj's tail: not where an adapter still changes the rows
  const bool ln1_next = tail_ln && TAIL_LN_C_PROJ && next && next->ln1_w && next->ln1_b && !w->adapter_w;
  ln_done = 0;
  {
    ProfScope ps(5, s);
    if (ln1_next) {
      const LnRows ln1 = {next->ln1_w, next->ln1_b, narrow, 1e-5f, !(next->exact16 & AACLIP_EXACT16_QKV)};
      ln_done = launch_gemm_resid_ln(dtype, p, ln1, s);
    } else {
      launch_gemm(dtype, EPI_BIAS_RESID, p, s);
    }
  }
  if (ln_done > 0) {
    ProfScope ps(0, s);
    launch_layernorm(dtype, x + ln_done * D, next->ln1_w, next->ln1_b, narrow + ln_done * 4 * D, rows - ln_done, D, 1e-5f,
                     s, !(next->exact16 & AACLIP_EXACT16_QKV));
    *ln1_out = true;
  }
  if (emit && !w->adapter_w) {
    ProfScope ps(0, s);
    launch_ln_stats_finalize(partials, rowab, rows, D / 64, D, 1e-5f, s);
    *aux_out = true;
  }
  // ---- residual adapter
  if (w->adapter_w) {
    ProfScope ps(6, s);
    const void* a_in = x;
    if (emit) {
      a_in = x16;
    } else if (dtype == AACLIP_F16X2) {
      launch_split_rows(x, narrow, rows, D, s, !(ex & AACLIP_EXACT16_ADAPTER));
      a_in = narrow;
    } else if (dtype != AACLIP_F32) {
      launch_cast_rows(dtype, x, narrow, rows * D, s);
      a_in = narrow;
    }
    p = gemm_params(a_in, sw * D, w->adapter_w, nullptr, big, D, M, D, D);
    p.act = 1;
    p.w_exact16 = ex & AACLIP_EXACT16_ADAPTER;
    launch_gemm(dtype, EPI_ACT_F32, p, s);
    if (folding && want_out) {
      launch_adapter_mix_fold(dtype, x, (const float*)big, rows, D, mix, x16, rowab, s);
      *aux_out = true;
    } else {
      launch_adapter_mix(x, (const float*)big, rows, D, mix, s);
    }
  }
  return 0;
}

int aaclip_blocks(float* x, const aaclip_block_weights* w, int n_blocks, float mix, int B, int L, int D, int H, int F,
                  int attn_mode, int dtype, void* ws, size_t ws_bytes, void* stream) {
  return aaclip_blocks_to(x, x, w, n_blocks, mix, B, L, D, H, F, attn_mode, dtype, ws, ws_bytes, stream);
}

// x_out[i] (x_of(i)) = the buffer holding the stream after block i; block i reads the stream from x_in (i == 0) or
// from the buffer block i-1 wrote.  x_out == nullptr: every block writes x_all.
static int blocks_core(const float* x_in, float* const* x_out, float* x_all, const aaclip_block_weights* w, int n_blocks,
                       float mix, int B, int L, int D, int H, int F, int attn_mode, int dtype, void* ws, size_t ws_bytes,
                       void* stream) {
  float* x = x_out ? x_out[0] : x_all;
  REQUIRE(x_in && w, "block: null pointer");
  REQUIRE(n_blocks >= 1, "block: n_blocks must be positive");
  // a caller built against another header revision (no size field, fewer pointer fields) is refused here, before
  // anything reads its struct as if it were ours
  for (int i = 0; i < n_blocks; ++i)
    REQUIRE(w[i].struct_bytes == sizeof(aaclip_block_weights),
            "block: aaclip_block_weights.struct_bytes does not match this library (binding generated from another "
            "include/aaclip.h revision?)");
  REQUIRE(dtype_ok(dtype), "block: bad dtype");
  REQUIRE(attn_mode >= AACLIP_ATTN_FULL && attn_mode <= AACLIP_ATTN_VV_BATCH, "block: attn_mode must be 0, 1 or 2");
  REQUIRE(attn_mode != AACLIP_ATTN_VV_BATCH || F >= 4 * D, "block: V-V attention needs F >= 4*D workspace columns");
  REQUIRE(x && ws, "block: null pointer");
  REQUIRE(B > 0 && L > 0, "block: empty batch");
  REQUIRE(D == 64 * H, "block: D must equal 64*H (head dim 64)");
  REQUIRE((long)L * 3 * D * 4 < (1L << 31) && (long)B * 3 * D * 4 < (1L << 31),
          "block: sequence too long for the attention kernel's 32-bit row offsets");
  REQUIRE(F % 128 == 0, "block: F must be a multiple of 128");
  REQUIRE_ROW_WIDTH(D);   // every accepted width is a multiple of 128, which the 128-tile GEMMs need
  const long rows = (long)B * L;
  REQUIRE(rows4_fit(rows), "block: too many rows");   // the row kernels: one workgroup per 4 rows, below 2^24
  const WsLayout l = ws_layout(dtype, rows, D, F, 0);
  REQUIRE(ws_bytes >= l.total, "block: workspace too small");
  if (x_out)
    for (int i = 0; i < n_blocks; ++i) REQUIRE(x_out[i], "block: null output buffer");
  bool aux = false, ln1 = false;   // ln1: `narrow` already holds ln_1 of the block about to run
  const float* src = x_in;
  for (int i = 0; i < n_blocks; ++i) {
    bool produced = false, ln1_produced = false;
    float* dst = x_out ? x_out[i] : x_all;
    int rc = block_impl(src, dst, w + i, mix, B, L, D, H, F, attn_mode, dtype, ws, l, (hipStream_t)stream, aux,
                        i + 1 < n_blocks, &produced, ln1, i + 1 < n_blocks ? w + i + 1 : nullptr, &ln1_produced);
    if (rc) return rc;
    aux = produced;
    ln1 = ln1_produced;
    src = dst;
  }
  return finish("block");
}

int aaclip_blocks_to(const float* x_in, float* x, const aaclip_block_weights* w, int n_blocks, float mix, int B, int L,
                     int D, int H, int F, int attn_mode, int dtype, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(x, "block: null pointer");
  return blocks_core(x_in, nullptr, x, w, n_blocks, mix, B, L, D, H, F, attn_mode, dtype, ws, ws_bytes, stream);
}

int aaclip_blocks_taps(const float* x_in, float* const* x_out, const aaclip_block_weights* w, int n_blocks, float mix,
                       int B, int L, int D, int H, int F, int attn_mode, int dtype, void* ws, size_t ws_bytes,
                       void* stream) {
  REQUIRE(x_out && n_blocks >= 1, "block: null output list");
  return blocks_core(x_in, x_out, nullptr, w, n_blocks, mix, B, L, D, H, F, attn_mode, dtype, ws, ws_bytes, stream);
}

int aaclip_block(float* x, const aaclip_block_weights* w, float mix, int B, int L, int D, int H, int F, int attn_mode,
                 int dtype, void* ws, size_t ws_bytes, void* stream) {
  return aaclip_blocks(x, w, 1, mix, B, L, D, H, F, attn_mode, dtype, ws, ws_bytes, stream);
}

static int head_common(const float* x, const float* ln_w, const float* ln_b, int B, int L, int D, int E, int dtype,
                       void* ws, size_t ws_bytes, WsLayout* l) {
  REQUIRE(dtype_ok(dtype), "head: bad dtype");
  REQUIRE(x && ln_w && ln_b && ws, "head: null pointer");
  REQUIRE(B > 0 && L > 1, "head: bad shape");
  REQUIRE_ROW_WIDTH(D);
  REQUIRE_ROW_WIDTH(E);
  REQUIRE(E % 128 == 0, "head: E must be a multiple of 128");
  *l = ws_layout(dtype, (long)B * L, D, 0, E);
  REQUIRE(ws_bytes >= l->total, "head: workspace too small");
  return 0;
}

// The det product of a head: the LayerNorm'ed rows `ln` -> big -> the mean over each image's patch rows.  narrow is
// the mean's scratch; where `ln` is narrow itself, it is free once the GEMM has run.
static void det_tail(const void* ln, const void* det_w, int act, float* det_out, int B, int L, int D, int E, int dtype,
                     void* ws, const WsLayout& l, hipStream_t s) {
  float* big = (float*)((char*)ws + l.big);
  GemmParams p = gemm_params(ln, split_w(dtype) * D, det_w, nullptr, big, E, (int)((long)B * L), E, D);
  p.act = act;
  launch_gemm(dtype, EPI_ACT_F32, p, s);
  launch_det_mean(big, (float*)ws, l.narrow_bytes / 4, det_out, B, L, 1, E, s);
}

static int tap_head_impl(const float* x, const float* ln_post_w, const float* ln_post_b, const void* proj_w, int act,
                         float* seg_out, const void* det_w, float* det_out, void* ln_rows_out, int B, int L, int D, int E,
                         int dtype, void* ws, size_t ws_bytes, void* stream) {
  WsLayout l;
  int rc = head_common(x, ln_post_w, ln_post_b, B, L, D, E, dtype, ws, ws_bytes, &l);
  if (rc) return rc;
  REQUIRE(proj_w && seg_out, "tap_head: null pointer");
  REQUIRE(!det_w || det_out, "tap_head: det_out missing");
  hipStream_t s = (hipStream_t)stream;
  const long rows = (long)B * L;
  float* big = (float*)((char*)ws + l.big);
  void* ln = ln_rows_out ? ln_rows_out : ws;   // the LayerNorm'ed rows: in narrow, or kept for the caller if asked
  launch_layernorm(dtype, x, ln_post_w, ln_post_b, ln, rows, D, 1e-5f, s);
  GemmParams p = gemm_params(ln, split_w(dtype) * D, proj_w, nullptr, big, E, (int)rows, E, D);
  p.act = act;
  launch_gemm(dtype, EPI_ACT_F32, p, s);
  launch_normalize_rows(big, seg_out, B, L, 1, E, s);
  if (det_w) det_tail(ln, det_w, act, det_out, B, L, D, E, dtype, ws, l, s);
  return finish("tap_head");
}

int aaclip_tap_head(const float* x, const float* ln_post_w, const float* ln_post_b, const void* proj_w, int act,
                    float* seg_out, const void* det_w, float* det_out, int B, int L, int D, int E, int dtype, void* ws,
                    size_t ws_bytes, void* stream) {
  return tap_head_impl(x, ln_post_w, ln_post_b, proj_w, act, seg_out, det_w, det_out, nullptr, B, L, D, E, dtype, ws, ws_bytes,
                       stream);
}

int aaclip_tap_head_keep_rows(const float* x, const float* ln_post_w, const float* ln_post_b, const void* proj_w, int act,
                              float* seg_out, const void* det_w, float* det_out, void* ln_rows_out, int B, int L, int D,
                              int E, int dtype, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(ln_rows_out, "tap_head_keep_rows: null pointer");
  return tap_head_impl(x, ln_post_w, ln_post_b, proj_w, act, seg_out, det_w, det_out, ln_rows_out, B, L, D, E, dtype, ws,
                       ws_bytes, stream);
}

int aaclip_det_head(const float* x, const float* ln_post_w, const float* ln_post_b, const void* det_w, int act,
                    float* det_out, int B, int L, int D, int E, int dtype, void* ws, size_t ws_bytes, void* stream) {
  WsLayout l;
  int rc = head_common(x, ln_post_w, ln_post_b, B, L, D, E, dtype, ws, ws_bytes, &l);
  if (rc) return rc;
  REQUIRE(det_w && det_out, "det_head: null pointer");
  hipStream_t s = (hipStream_t)stream;
  launch_layernorm(dtype, x, ln_post_w, ln_post_b, ws, (long)B * L, D, 1e-5f, s);   // into narrow
  det_tail(ws, det_w, act, det_out, B, L, D, E, dtype, ws, l, s);
  return finish("det_head");
}

int aaclip_anomaly_map(const float* const* seg, int NL, const float* anchors, long anchor_bstride, float* out, int B,
                       int g, int E, int S, int ksize, float sigma, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(seg && anchors && out && ws, "anomaly_map: null pointer");
  REQUIRE(NL >= 1 && NL <= 4, "anomaly_map: 1..4 levels");
  REQUIRE(map_shape_ok(B, g, S), "anomaly_map: bad shape (grid <= 40)");
  REQUIRE(ksize >= 1 && ksize <= 15 && ksize / 2 < g, "anomaly_map: kernel size must be 1..15 and < 2*grid");
  REQUIRE(sigma > 0.f, "anomaly_map: sigma must be positive");
  REQUIRE_ROW_WIDTH(E);
  const int P = g * g;
  REQUIRE(ws_bytes >= (size_t)NL * B * P * 4, "anomaly_map: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* pre = (float*)ws;
  for (int l = 0; l < NL; ++l) {
    REQUIRE(seg[l], "anomaly_map: null level pointer");
    launch_patch_scores(seg[l], anchors, anchor_bstride, pre + (size_t)l * B * P, B, P, E, 0, s);
  }
  launch_blur_upsample(pre, out, B, g, S, NL, ksize, sigma, s);
  return finish("anomaly_map");
}

int aaclip_similarity_map_train(const float* seg, const float* anchors, long anchor_bstride, float* out, int B, int g,
                                int E, int S, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(seg && anchors && out && ws, "similarity_map_train: null pointer");
  REQUIRE(map_shape_ok(B, g, S), "similarity_map_train: bad shape (grid <= 40)");
  REQUIRE_ROW_WIDTH(E);
  const int P = g * g;
  REQUIRE(ws_bytes >= (size_t)2 * B * P * 4, "similarity_map_train: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  launch_patch_scores(seg, anchors, anchor_bstride, (float*)ws, B, P, E, 1, s);
  launch_upsample_softmax2((const float*)ws, out, B, g, S, s);
  return finish("similarity_map_train");
}

size_t aaclip_similarity_map_train_backward_workspace_bytes(int B, int g, int S) {
  if (B <= 0 || g <= 0 || S <= 0) return 0;
  return simmap_bwd_ws_bytes(B, g, S);
}

int aaclip_similarity_map_train_backward(const float* seg, const float* anchors, long anchor_bstride,
                                         const float* preds, const float* d_preds, float* d_anchors, float* d_seg,
                                         int B, int g, int E, int S, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(seg && anchors && preds && d_preds && ws, "similarity_map_train_backward: null pointer");
  REQUIRE(map_shape_ok(B, g, S) && S <= SIMMAP_BWD_MAX_S,
          "similarity_map_train_backward: bad shape (grid <= 40, size <= 2048)");
  REQUIRE(anchor_bstride == 0 || anchor_bstride == 2L * E, "similarity_map_train_backward: anchor stride 0 or 2E");
  REQUIRE_ROW_WIDTH(E);
  REQUIRE(ws_bytes >= simmap_bwd_ws_bytes(B, g, S), "similarity_map_train_backward: workspace too small");
  launch_similarity_map_train_bwd(seg, anchors, anchor_bstride, preds, d_preds, d_anchors, d_seg, B, g, E, S, ws,
                                  (hipStream_t)stream);
  return finish("similarity_map_train_backward");
}

// the checks aaclip_iqm_map_train and its backward share (the workspace size, the backward's last check, is its own)
static int iqm_map_train_checks(const char* shape_msg, const char* align_msg, int B, int g, int E, int S,
                                const void* const (&ptrs)[7]) {
  REQUIRE(map_shape_ok(B, g, S) && S <= SIMMAP_BWD_MAX_S, shape_msg);
  REQUIRE_ROW_WIDTH(E);
  for (const void* p : ptrs)
    if ((uintptr_t)p & 15) return fail(-1, align_msg);
  return 0;
}

int aaclip_iqm_map_train(const float* seg, const float* queries, float* grid_out, float* out, int B, int g, int E, int S,
                         void* stream) {
  REQUIRE(seg && queries && grid_out && out, "iqm_map_train: null pointer");
  const void* const ptrs[7] = {seg, queries, grid_out, out, nullptr, nullptr, nullptr};
  if (int rc = iqm_map_train_checks("iqm_map_train: bad shape (grid <= 40, size <= 2048)",
                                    "iqm_map_train: pointers must be 16-byte aligned", B, g, E, S, ptrs))
    return rc;
  launch_iqm_map_train(seg, queries, grid_out, out, B, g, E, S, (hipStream_t)stream);
  return finish("iqm_map_train");
}

size_t aaclip_iqm_map_train_backward_workspace_bytes(int B, int g, int E, int S) {
  if (B <= 0 || g <= 0 || E <= 0 || S <= 0) return 0;
  return iqm_map_train_bwd_ws_bytes(B, g, E, S);
}

int aaclip_iqm_map_train_backward(const float* seg, const float* queries, const float* grid, const float* d_preds,
                                  float* d_seg, float* d_queries, int B, int g, int E, int S, void* ws, size_t ws_bytes,
                                  void* stream) {
  REQUIRE(seg && queries && grid && d_preds && ws, "iqm_map_train_backward: null pointer");
  REQUIRE(d_seg || d_queries, "iqm_map_train_backward: nothing to compute (both outputs are null)");
  const void* const ptrs[7] = {seg, queries, grid, d_preds, d_seg, d_queries, ws};
  if (int rc = iqm_map_train_checks("iqm_map_train_backward: bad shape (grid <= 40, size <= 2048)",
                                    "iqm_map_train_backward: pointers must be 16-byte aligned", B, g, E, S, ptrs))
    return rc;
  REQUIRE(ws_bytes >= iqm_map_train_bwd_ws_bytes(B, g, E, S), "iqm_map_train_backward: workspace too small");
  launch_iqm_map_train_bwd(seg, queries, grid, d_preds, d_seg, d_queries, B, g, E, S, ws, (hipStream_t)stream);
  return finish("iqm_map_train_backward");
}

size_t aaclip_seg_loss_workspace_bytes(int B) { return B > 0 ? seg_loss_ws_bytes(B) : 0; }

int aaclip_seg_loss(const float* preds, long img_stride, long chan_stride, const float* mask, int terms, float* loss,
                    float* coef, int B, long P, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(preds && mask && loss && coef && ws, "seg_loss: null pointer");
  REQUIRE(B > 0 && B <= 65535 && P > 0, "seg_loss: bad shape");
  REQUIRE(terms > 0 && terms <= 7, "seg_loss: terms is a non-empty mask of AACLIP_SEG_LOSS_*");
  REQUIRE(img_stride >= 0 && chan_stride >= 0, "seg_loss: negative stride");
  REQUIRE(ws_bytes >= seg_loss_ws_bytes(B), "seg_loss: workspace too small");
  launch_seg_loss(preds, img_stride, chan_stride, mask, terms, loss, coef, B, P, ws, (hipStream_t)stream);
  return finish("seg_loss");
}

int aaclip_seg_loss_backward(const float* preds, long img_stride, long chan_stride, const float* mask, int terms,
                             const float* coef, const float* d_loss, float* d_preds, int B, long P, void* stream) {
  REQUIRE(preds && mask && coef && d_loss && d_preds, "seg_loss_backward: null pointer");
  REQUIRE(B > 0 && B <= 65535 && P > 0, "seg_loss_backward: bad shape");
  REQUIRE(terms > 0 && terms <= 7, "seg_loss_backward: terms is a non-empty mask of AACLIP_SEG_LOSS_*");
  REQUIRE(img_stride >= 0 && chan_stride >= 0, "seg_loss_backward: negative stride");
  REQUIRE(chan_stride != 0 || !((terms & SEG_LOSS_FOCAL) || ((terms & SEG_LOSS_DICE0) && (terms & SEG_LOSS_DICE1))),
          "seg_loss_backward: both channels are written, they cannot share storage (chan_stride 0)");
  launch_seg_loss_grad(preds, img_stride, chan_stride, mask, terms, coef, d_loss, d_preds, B, P, (hipStream_t)stream);
  return finish("seg_loss_backward");
}

// ---- Training: backward of the adapted text tower (text_backward.hip).  fp32, fixed-order reductions.

// The block-backward workspace, byte offsets from its start.  The recomputed internals of one block (h: a LayerNorm
// output, qkv, ctx, x1: the stream after the attention half, f: the c_fc pre-activation, g: GELU(f) and later its
// gradient, x2: the adapter's input, z: the adapter pre-activation and later its gradient), the gradients in flight (dx,
// dqkv, tmp) and the chunk partials of the weight-gradient GEMM (sized for the largest split, whatever `rows` is, so
// that the total grows with rows).
struct TbLayout { size_t h, qkv, ctx, x1, f, g, x2, z, dx, dqkv, tmp, wg, total; };
static TbLayout tb_layout(long rows, int D, int F) {
  const size_t rd = up256((size_t)rows * D * 4), r3 = up256((size_t)rows * 3 * D * 4), rf = up256((size_t)rows * F * 4);
  TbLayout l;
  l.h = 0;
  l.qkv = l.h + rd;
  l.ctx = l.qkv + r3;
  l.x1 = l.ctx + rd;
  l.f = l.x1 + rd;
  l.g = l.f + rf;
  l.x2 = l.g + rf;
  l.z = l.x2 + rd;
  l.dx = l.z + rd;
  l.dqkv = l.dx + rd;
  l.tmp = l.dqkv + r3;
  l.wg = l.tmp + rd;
  l.total = l.wg + up256((size_t)WGRAD_MAX_CHUNKS * 1024 * D * 4) + 4096;
  return l;
}

size_t aaclip_text_backward_workspace_bytes(long rows, int D, int F) {
  if (rows <= 0 || D <= 0 || F < 0) return 0;
  return tb_layout(rows, D, F).total;
}

int aaclip_gemm_wgrad(const float* dz, long ldz, const float* u, long ldu, float* dw, long rows, int O, int I, void* ws,
                      size_t ws_bytes, void* stream) {
  REQUIRE(dz && u && dw, "gemm_wgrad: null pointer");
  REQUIRE(rows > 0 && rows < (1L << 31), "gemm_wgrad: rows must be positive (and below 2^31)");
  REQUIRE(O > 0 && I > 0 && O % 128 == 0 && I % 128 == 0, "gemm_wgrad: both weight dimensions must be multiples of 128");
  REQUIRE(O <= 1024, "gemm_wgrad: at most 1024 output features (O <= 1024)");
  REQUIRE(ldz >= O && ldu >= I && ldz % 4 == 0 && ldu % 4 == 0, "gemm_wgrad: row strides must be multiples of 4 and cover the rows");
  REQUIRE((((uintptr_t)dz | (uintptr_t)u | (uintptr_t)dw) & 15) == 0, "gemm_wgrad: pointers must be 16-byte aligned");
  const size_t need = wgrad_ws_bytes(rows, O, I);
  REQUIRE(need == 0 || (ws && ws_bytes >= need && ((uintptr_t)ws & 15) == 0), "gemm_wgrad: workspace too small");
  launch_wgrad(dz, ldz, u, ldu, dw, rows, O, I, ws, (hipStream_t)stream);
  return finish("gemm_wgrad");
}

int aaclip_attention_backward(const float* qkv, const float* d_ctx, float* d_qkv, int B, int L, int H, int causal,
                              float dq_scale, void* stream) {
  REQUIRE(qkv && d_ctx && d_qkv, "attention_backward: null pointer");
  if (const char* m = attention_backward_check(B, L, H)) return fail(-1, m);
  REQUIRE_ALIGNED16("attention_backward", qkv, d_ctx, d_qkv);
  launch_attention_backward(qkv, d_ctx, d_qkv, B, L, H, causal != 0, dq_scale, (hipStream_t)stream);
  return finish("attention_backward");
}

size_t aaclip_attention_backward_long_workspace_bytes(int B, int L, int H) {
  return attention_backward_long_ws_bytes(B, L, H);
}

int aaclip_attention_backward_long(const float* qkv, const float* d_ctx, float* d_qkv, int B, int L, int H, int causal,
                                   float dq_scale, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(qkv && d_ctx && d_qkv && ws, "attention_backward_long: null pointer");
  if (const char* m = attention_backward_long_check(B, L, H)) return fail(-1, m);
  REQUIRE_ALIGNED16("attention_backward_long", qkv, d_ctx, d_qkv, ws);
  REQUIRE(ws_bytes >= attention_backward_long_ws_bytes(B, L, H), "attention_backward_long: workspace too small");
  launch_attention_backward_long(qkv, d_ctx, d_qkv, B, L, H, causal != 0, dq_scale, ws, (hipStream_t)stream);
  return finish("attention_backward_long");
}

int aaclip_layernorm_backward(const float* x, const float* w, const float* d_y, const float* d_resid, float* d_x,
                              long rows, int D, float eps, void* stream) {
  REQUIRE(x && w && d_y && d_x, "layernorm_backward: null pointer");
  REQUIRE(rows > 0, "layernorm_backward: rows must be positive");
  REQUIRE(rows4_fit(rows), TOO_MANY_ROWS4("layernorm_backward"));
  REQUIRE_ROW_WIDTH(D);
  REQUIRE_ALIGNED16("layernorm_backward", x, w, d_y, d_resid, d_x);
  launch_layernorm_backward(x, w, d_y, d_resid, d_x, nullptr, rows, D, eps, (hipStream_t)stream);
  return finish("layernorm_backward");
}

int aaclip_adapter_mix_backward(const float* u, const float* z, const float* d_y, float* d_z, float* d_u, long rows,
                                int D, float weight, void* stream) {
  REQUIRE(u && z && d_y && d_z && d_u, "adapter_mix_backward: null pointer");
  REQUIRE(rows > 0, "adapter_mix_backward: rows must be positive");
  REQUIRE(rows4_fit(rows), TOO_MANY_ROWS4("adapter_mix_backward"));
  REQUIRE_ROW_WIDTH(D);
  REQUIRE_ALIGNED16("adapter_mix_backward", u, z, d_y, d_z, d_u);
  launch_adapter_mix_backward(u, z, d_y, d_z, d_u, rows, D, weight, (hipStream_t)stream);
  return finish("adapter_mix_backward");
}

// one buffer for every split3 A operand of the bf16x3 block: each is read by the product right behind the pass that
// writes it
static size_t bf16x3_rows_bytes(long rows, int D, int F) {
  return up256((size_t)rows * 3 * (size_t)(F > 3 * D ? F : 3 * D) * 2);
}

// The body of aaclip_block_backward, aaclip_block_backward_long and aaclip_block_backward_long_bf16x3 (`name` is the
// entry's prefix in error texts).  The routes differ in two places.  The workspace tail and the attention backward: the
// long form appends the attention statistics to the text-backward layout, bf16x3 its split3 buffer a3 and the
// statistics and planes.  And how one product of the block proper is issued (`product` below): an fp32 GEMM on the
// fp32 rows against `wp` = w / `wt`, or the split3 pass into a3 and a bf16 GEMM over K' = 3K against the stacked
// weights `wp` = w3 / `wt` = wt3 (w3's in_proj carries the q scale).  The recomputed forward attention, the adapter's
// three products and every row op are fp32 on every route.
enum { BLOCK_BWD_SHORT, BLOCK_BWD_LONG, BLOCK_BWD_LONG_BF16X3 };
static int block_backward_body(int route, const char* name, const float* x_in, const aaclip_block_weights* w,
                               const aaclip_block_weights* wp, const aaclip_block_weights* wt, float mix, int B, int L,
                               int D, int H, int F, int attn_mode, const float* d_out, float* d_in, float* d_adapter_w,
                               void* ws, size_t ws_bytes, void* stream) {
  const bool bf16x3 = route == BLOCK_BWD_LONG_BF16X3;
  REQUIRE(x_in && w && wp && wt && d_out && ws, in(name, "null pointer"));
  REQUIRE(w->struct_bytes == sizeof(aaclip_block_weights) && wp->struct_bytes == sizeof(aaclip_block_weights) &&
              wt->struct_bytes == sizeof(aaclip_block_weights),
          in(name, "aaclip_block_weights.struct_bytes does not match this library"));
  REQUIRE(attn_mode == AACLIP_ATTN_FULL || attn_mode == AACLIP_ATTN_CAUSAL,
          in(name, "attn_mode must be AACLIP_ATTN_FULL or AACLIP_ATTN_CAUSAL"));
  REQUIRE(B > 0 && L > 0, in(name, "empty batch"));
  REQUIRE(D == 64 * H, in(name, "D must equal 64*H (head dim 64)"));
  REQUIRE_ROW_WIDTH(D);
  REQUIRE(F > 0 && F % 128 == 0, in(name, "F must be a multiple of 128"));
  if (const char* m = route == BLOCK_BWD_SHORT ? attention_backward_check(B, L, H) : attention_backward_long_check(B, L, H))
    return fail(-1, m);
  const long rows = (long)B * L;
  REQUIRE(rows4_fit(rows), in(name, "too many rows"));
  REQUIRE(w->ln1_w && w->ln1_b && w->out_b && w->ln2_w && w->ln2_b && w->fc_b && w->proj_b,
          in(name, "null weight pointer"));
  REQUIRE(wp->qkv_w && wp->qkv_b && wp->out_w && wp->fc_w && wp->proj_w,
          in(name, bf16x3 ? "null stacked weight pointer" : "null weight pointer"));
  const bool adapter = w->adapter_w != nullptr;
  REQUIRE(adapter || d_in, in(name, "nothing to compute (no adapter and d_in is NULL)"));
  REQUIRE(!adapter || d_adapter_w, in(name, "d_adapter_w is required for a block with an adapter"));
  REQUIRE(!d_in || (wt->qkv_w && wt->out_w && wt->fc_w && wt->proj_w && (!adapter || wt->adapter_w)),
          in(name, "null transposed weight pointer"));
  const TbLayout l = tb_layout(rows, D, F);
  const size_t a3_bytes = bf16x3 ? bf16x3_rows_bytes(rows, D, F) : 0;
  const size_t attn_bytes = bf16x3                     ? attention_backward_long_bf16x3_ws_bytes(B, L, H)
                            : route == BLOCK_BWD_LONG ? attention_backward_long_ws_bytes(B, L, H)
                                                      : 0;
  REQUIRE(ws_bytes >= l.total + a3_bytes + attn_bytes, in(name, "workspace too small"));
  REQUIRE_ALIGNED16(name, x_in, d_out, d_in, d_adapter_w, ws, w->ln1_w, w->ln2_w, w->adapter_w);
  if (bf16x3)   // the stacked 16-bit weights; the fp32 routes never asked this of theirs
    REQUIRE_ALIGNED16(name, wp->qkv_w, wp->out_w, wp->fc_w, wp->proj_w, wt->qkv_w, wt->out_w, wt->fc_w, wt->proj_w,
                      wt->adapter_w);
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)ws;
  float *h = (float*)(base + l.h), *qkv = (float*)(base + l.qkv), *ctx = (float*)(base + l.ctx);
  float *x1 = (float*)(base + l.x1), *f = (float*)(base + l.f), *g = (float*)(base + l.g), *x2 = (float*)(base + l.x2);
  float *z = (float*)(base + l.z), *dx = (float*)(base + l.dx), *dqkv = (float*)(base + l.dqkv);
  float* tmp = (float*)(base + l.tmp);
  void* a3 = base + l.total;
  void* attn_ws = base + l.total + a3_bytes;
  const int M = (int)rows;
  const int causal = attn_mode == AACLIP_ATTN_CAUSAL;
  const float qscale = 0.125f;
  // out[M, N] (fp32) = A[M, K] . W[N, K]^T (+ bias (+ resid)), the first q_cols columns times qscale.  bf16x3: in three
  // terms, W is [N, 3K] bf16 and carries the scale, a3 receives A's split3 rows (A == NULL: a3 holds them already)
  auto product = [&](const float* A, const void* W, const void* bias, float* out, int N, int K, const float* resid,
                     int q_cols) {
    if (bf16x3 && A) launch_split3_rows(A, a3, rows, K, s);
    GemmParams p = bf16x3 ? gemm_params(a3, 3L * K, W, (const float*)bias, out, N, M, N, 3 * K)
                          : gemm_params(A, K, W, (const float*)bias, out, N, M, N, K);
    p.resid = resid;
    if (!bf16x3 && q_cols) { p.scale_cols = q_cols; p.scale = qscale; }
    if (bf16x3) launch_gemm(AACLIP_BF16, resid ? EPI_BIAS_RESID : EPI_ACT_F32, p, s);
    else launch_gemm(AACLIP_F32, resid ? EPI_BIAS_RESID : bias ? EPI_BIAS : EPI_ACT_F32, p, s);
  };
  // ---- the block's internals again from its input (aaclip_block's arithmetic), qkv with q scaled
  launch_layernorm(AACLIP_F32, x_in, w->ln1_w, w->ln1_b, h, rows, D, 1e-5f, s);
  product(h, wp->qkv_w, wp->qkv_b, qkv, 3 * D, D, nullptr, D);
  launch_attention(AACLIP_F32, qkv, ctx, B, L, H, causal, 0, s);
  product(ctx, wp->out_w, w->out_b, x1, D, D, x_in, 0);
  launch_layernorm(AACLIP_F32, x1, w->ln2_w, w->ln2_b, h, rows, D, 1e-5f, s);
  product(h, wp->fc_w, w->fc_b, f, F, D, nullptr, 0);
  const float* dy = d_out;   // gradient of the stream after the MLP half
  if (adapter) {
    if (bf16x3) launch_gelu_forward_split3(f, a3, rows, F, s);
    else launch_gelu_forward(f, g, rows * F, s);
    product(bf16x3 ? nullptr : g, wp->proj_w, w->proj_b, x2, D, F, x1, 0);
    GemmParams p = gemm_params(x2, D, w->adapter_w, nullptr, z, D, M, D, D);
    launch_gemm(AACLIP_F32, EPI_ACT_F32, p, s);
    launch_adapter_mix_backward(x2, z, d_out, z, dx, rows, D, mix, s);   // z <- dz, dx <- the direct d x2
    launch_wgrad(z, D, x2, D, d_adapter_w, rows, D, D, base + l.wg, s);
    if (!d_in) return finish(name);
    p = gemm_params(z, D, wt->adapter_w, nullptr, tmp, D, M, D, D);
    launch_gemm(AACLIP_F32, EPI_ACT_F32, p, s);
    launch_add_rows(dx, tmp, dx, rows * D, s);
    dy = dx;
  }
  // ---- x2 = x1 + c_proj(gelu(f)),  f = c_fc(ln_2 x1)
  product(dy, wt->proj_w, nullptr, g, F, D, nullptr, 0);
  if (bf16x3) launch_gelu_backward_split3(f, g, a3, rows, F, s);
  else launch_gelu_backward(f, g, g, rows * F, s);
  product(bf16x3 ? nullptr : g, wt->fc_w, nullptr, tmp, D, F, nullptr, 0);
  launch_layernorm_backward(x1, w->ln2_w, tmp, dy, dx, nullptr, rows, D, 1e-5f, s);   // dx <- d x1
  // ---- x1 = x_in + out_proj(attention(qkv)),  qkv = in_proj(ln_1 x_in), q scaled
  product(dx, wt->out_w, nullptr, tmp, D, D, nullptr, 0);
  if (bf16x3) launch_attention_backward_long_bf16x3(qkv, tmp, dqkv, B, L, H, causal, qscale, attn_ws, s);
  else if (route == BLOCK_BWD_LONG) launch_attention_backward_long(qkv, tmp, dqkv, B, L, H, causal, qscale, attn_ws, s);
  else launch_attention_backward(qkv, tmp, dqkv, B, L, H, causal, qscale, s);
  product(dqkv, wt->qkv_w, nullptr, tmp, D, 3 * D, nullptr, 0);
  launch_layernorm_backward(x_in, w->ln1_w, tmp, dx, d_in, nullptr, rows, D, 1e-5f, s);
  return finish(name);
}

int aaclip_block_backward(const float* x_in, const aaclip_block_weights* w, const aaclip_block_weights* wt, float mix,
                          int B, int L, int D, int H, int F, int attn_mode, const float* d_out, float* d_in,
                          float* d_adapter_w, void* ws, size_t ws_bytes, void* stream) {
  return block_backward_body(BLOCK_BWD_SHORT, "block_backward", x_in, w, w, wt, mix, B, L, D, H, F, attn_mode, d_out,
                             d_in, d_adapter_w, ws, ws_bytes, stream);
}

size_t aaclip_block_backward_long_workspace_bytes(int B, int L, int D, int F) {
  if (B <= 0 || L <= 0 || D <= 0 || F < 0) return 0;
  return tb_layout((long)B * L, D, F).total + attention_backward_long_ws_bytes(B, L, (D + 63) / 64);
}

int aaclip_block_backward_long(const float* x_in, const aaclip_block_weights* w, const aaclip_block_weights* wt,
                               float mix, int B, int L, int D, int H, int F, int attn_mode, const float* d_out,
                               float* d_in, float* d_adapter_w, void* ws, size_t ws_bytes, void* stream) {
  return block_backward_body(BLOCK_BWD_LONG, "block_backward", x_in, w, w, wt, mix, B, L, D, H, F, attn_mode, d_out,
                             d_in, d_adapter_w, ws, ws_bytes, stream);
}

// ---- The three-term bf16 backward of the visual blocks (bf16x3.h; include/aaclip.h, "bf16x3")

int aaclip_split3_rows(const float* src, void* dst, long rows, int K, void* stream) {
  REQUIRE(src && dst, "split3_rows: null pointer");
  REQUIRE(rows > 0 && K > 0 && K % 64 == 0, "split3_rows: rows must be positive and K a positive multiple of 64");
  REQUIRE(rows <= (1L << 35) / K && grid_fits((rows * (K / 8) + 255) / 256),
          "split3_rows: too many rows (one thread per 8 elements, below 2^24 workgroups: rows * K <= 2^35 - 2048)");
  REQUIRE_ALIGNED16("split3_rows", src, dst);
  launch_split3_rows(src, dst, rows, K, (hipStream_t)stream);
  return finish("split3_rows");
}

size_t aaclip_attention_backward_long_bf16x3_workspace_bytes(int B, int L, int H) {
  return attention_backward_long_bf16x3_ws_bytes(B, L, H);
}

int aaclip_attention_backward_long_bf16x3(const float* qkv, const float* d_ctx, float* d_qkv, int B, int L, int H,
                                          int causal, float dq_scale, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(qkv && d_ctx && d_qkv && ws, "attention_backward_long_bf16x3: null pointer");
  if (const char* m = attention_backward_long_check(B, L, H)) return fail(-1, m);
  REQUIRE_ALIGNED16("attention_backward_long_bf16x3", qkv, d_ctx, d_qkv, ws);
  REQUIRE(ws_bytes >= attention_backward_long_bf16x3_ws_bytes(B, L, H),
          "attention_backward_long_bf16x3: workspace too small");
  launch_attention_backward_long_bf16x3(qkv, d_ctx, d_qkv, B, L, H, causal != 0, dq_scale, ws, (hipStream_t)stream);
  return finish("attention_backward_long_bf16x3");
}

size_t aaclip_block_backward_long_bf16x3_workspace_bytes(int B, int L, int D, int F) {
  if (B <= 0 || L <= 0 || D <= 0 || F < 0) return 0;
  const long rows = (long)B * L;
  return tb_layout(rows, D, F).total + bf16x3_rows_bytes(rows, D, F) +
         attention_backward_long_bf16x3_ws_bytes(B, L, (D + 63) / 64);
}

int aaclip_block_backward_long_bf16x3(const float* x_in, const aaclip_block_weights* w, const aaclip_block_weights* w3,
                                      const aaclip_block_weights* wt3, float mix, int B, int L, int D, int H, int F,
                                      int attn_mode, const float* d_out, float* d_in, float* d_adapter_w, void* ws,
                                      size_t ws_bytes, void* stream) {
  return block_backward_body(BLOCK_BWD_LONG_BF16X3, "block_backward_bf16x3", x_in, w, w3, wt3, mix, B, L, D, H, F,
                             attn_mode, d_out, d_in, d_adapter_w, ws, ws_bytes, stream);
}

int aaclip_row_head_backward(const float* x, const int32_t* tokens, const float* ln_w, const float* ln_b,
                             const float* proj_w, const float* proj_wt, int act, const float* d_out, float* d_x,
                             float* d_proj_w, int n, int T, int D, int E, int mode, void* ws, size_t ws_bytes,
                             void* stream) {
  REQUIRE(x && ln_w && ln_b && proj_w && d_out && d_proj_w && ws, "row_head_backward: null pointer");
  REQUIRE(mode == 0 || mode == 1, "row_head_backward: mode must be 0 (EOT row) or 1 (row 0)");
  REQUIRE(mode == 1 || tokens, "row_head_backward: tokens required for EOT mode");
  REQUIRE(!d_x || proj_wt, "row_head_backward: the transposed projection is required for d_x");
  REQUIRE(n > 0 && T > 0 && (long)n * T < (1L << 31) / 4, "row_head_backward: bad shape");
  REQUIRE(act >= AACLIP_ACT_NONE && act <= AACLIP_ACT_RELU, "row_head_backward: bad activation");
  REQUIRE_ROW_WIDTH(D);
  REQUIRE(E > 0 && E % 128 == 0 && E <= 1024, "row_head_backward: E must be a multiple of 128, <= 1024");
  const size_t o_idx = 0, o_xg = o_idx + up256((size_t)n * 4), o_ln = o_xg + up256((size_t)n * D * 4);
  const size_t o_z = o_ln + up256((size_t)n * D * 4), o_dp = o_z + up256((size_t)n * E * 4);
  const size_t o_wg = o_dp + up256((size_t)n * D * 4);
  REQUIRE(ws_bytes >= o_wg + wgrad_ws_bytes(n, E, D), "row_head_backward: workspace too small");
  REQUIRE_ALIGNED16("row_head_backward", x, ln_w, d_out, d_x, d_proj_w, ws);
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)ws;
  int* idx = (int*)(base + o_idx);
  float *xg = (float*)(base + o_xg), *ln = (float*)(base + o_ln), *z = (float*)(base + o_z), *dp = (float*)(base + o_dp);
  launch_pick_rows(x, xg, idx, tokens, n, T, D, mode, s);
  launch_layernorm(AACLIP_F32, xg, ln_w, ln_b, ln, n, D, 1e-5f, s);
  GemmParams p = gemm_params(ln, D, proj_w, nullptr, z, E, n, E, D);
  launch_gemm(AACLIP_F32, EPI_ACT_F32, p, s);
  launch_act_backward(z, d_out, z, (long)n * E, act, s);   // z <- dz
  launch_wgrad(z, E, ln, D, d_proj_w, n, E, D, base + o_wg, s);
  if (d_x) {
    // a true scatter: the n picked rows are distinct, every other row of the stream gradient is zero
    if (hipMemsetAsync(d_x, 0, (size_t)n * T * D * 4, s) != hipSuccess) return fail(-2, "row_head_backward: memset failed");
    p = gemm_params(z, E, proj_wt, nullptr, dp, D, n, D, E);
    launch_gemm(AACLIP_F32, EPI_ACT_F32, p, s);
    launch_layernorm_backward(xg, ln_w, dp, nullptr, d_x, idx, n, D, 1e-5f, s);
  }
  return finish("row_head_backward");
}

// The tap-head-backward workspace, byte offsets from its start: the LayerNorm'ed rows, the projection rows (z, then dz;
// the seg and the det part take turns), the two parts' d_ln and the chunk partials of the weight-gradient GEMM (sized
// for the largest split, whatever the row count is, so that the total grows with it).
struct ThLayout { size_t ln, z, dln, dln2, wg, total; };
static ThLayout th_layout(long rows, int D, int E) {
  const size_t rd = up256((size_t)rows * D * 4), re = up256((size_t)rows * E * 4);
  ThLayout l;
  l.ln = 0;
  l.z = l.ln + rd;
  l.dln = l.z + re;
  l.dln2 = l.dln + rd;
  l.wg = l.dln2 + rd;
  l.total = l.wg + up256((size_t)WGRAD_MAX_CHUNKS * E * D * 4);
  return l;
}

size_t aaclip_tap_head_backward_workspace_bytes(int B, int L, int D, int E) {
  if (B <= 0 || L <= 0 || D <= 0 || E <= 0) return 0;
  return th_layout((long)B * L, D, E).total;
}

int aaclip_tap_head_backward(const float* x, const float* ln_post_w, const float* ln_post_b, const float* proj_w,
                             const float* proj_wt, int act, const float* d_seg, const float* det_w, const float* det_wt,
                             const float* d_det, float* d_x, float* d_proj_w, float* d_det_w, int B, int L, int D, int E,
                             void* ws, size_t ws_bytes, void* stream) {
  const bool seg = d_seg != nullptr, det = d_det != nullptr;
  REQUIRE(x && ln_post_w && ln_post_b && ws, "tap_head_backward: null pointer");
  REQUIRE(seg || det, "tap_head_backward: nothing to compute (d_seg and d_det are both NULL)");
  REQUIRE(!seg || (proj_w && d_proj_w), "tap_head_backward: null pointer (proj_w and d_proj_w go with d_seg)");
  REQUIRE((det_w != nullptr) == det && (d_det_w != nullptr) == det && (det || !det_wt),
          "tap_head_backward: det_w, d_det and d_det_w are given together or not at all");
  REQUIRE(!d_x || ((!seg || proj_wt) && (!det || det_wt)),
          "tap_head_backward: the transposed projections are required for d_x");
  REQUIRE(B > 0 && L > 1, "tap_head_backward: bad shape (B > 0, L > 1)");
  REQUIRE_ROW_WIDTH(D);
  REQUIRE_ROW_WIDTH(E);
  REQUIRE(E % 128 == 0, "tap_head_backward: E must be a multiple of 128");
  REQUIRE(act >= AACLIP_ACT_NONE && act <= AACLIP_ACT_RELU, "tap_head_backward: bad activation");
  const long rows = (long)B * L;
  REQUIRE(rows4_fit(rows), "tap_head_backward: too many rows");
  REQUIRE_ALIGNED16("tap_head_backward", x, ln_post_w, ln_post_b, proj_w, proj_wt, d_seg, det_w, det_wt, d_det, d_x,
                    d_proj_w, d_det_w, ws);
  const ThLayout l = th_layout(rows, D, E);
  REQUIRE(ws_bytes >= l.total, "tap_head_backward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)ws;
  float *ln = (float*)(base + l.ln), *z = (float*)(base + l.z), *dln = (float*)(base + l.dln);
  const int M = (int)rows;
  launch_layernorm(AACLIP_F32, x, ln_post_w, ln_post_b, ln, rows, D, 1e-5f, s);
  // one projection: z = ln W^T again, z <- dz, dW = dz^T ln, and (for d_x) d_ln = dz W into `out`
  auto part = [&](const float* w, const float* wt, const float* d, int is_det, float* dw, float* out) {
    GemmParams p = gemm_params(ln, D, w, nullptr, z, E, M, E, D);
    launch_gemm(AACLIP_F32, EPI_ACT_F32, p, s);
    launch_head_normalize_backward(z, d, B, L, E, act, is_det, s);
    launch_wgrad(z, E, ln, D, dw, rows, E, D, base + l.wg, s);
    if (d_x) {
      p = gemm_params(z, E, wt, nullptr, out, D, M, D, E);
      launch_gemm(AACLIP_F32, EPI_ACT_F32, p, s);
    }
  };
  if (seg) part(proj_w, proj_wt, d_seg, 0, d_proj_w, dln);
  if (det) part(det_w, det_wt, d_det, 1, d_det_w, seg ? (float*)(base + l.dln2) : dln);
  if (d_x) {
    if (seg && det) launch_add_rows(dln, (const float*)(base + l.dln2), dln, rows * D, s);
    launch_layernorm_backward(x, ln_post_w, dln, nullptr, d_x, nullptr, rows, D, 1e-5f, s);
  }
  return finish("tap_head_backward");
}

int aaclip_resample_ksize(int in_size, int out_size) {
  if (in_size < 1 || out_size < 1) return fail(-1, "resample_ksize: sizes must be positive");
  return resample_ksize(in_size, out_size);
}

int aaclip_resample_table(int in_size, int out_size, int32_t* bounds, int32_t* coefs) {
  REQUIRE(bounds && coefs, "resample_table: null pointer");
  REQUIRE(in_size >= 1 && out_size >= 1 && in_size <= (1 << 16) && out_size <= (1 << 16),
          "resample_table: sizes must be 1..65536");
  resample_table(in_size, out_size, bounds, coefs);
  return 0;
}

int aaclip_preprocess(const uint8_t* src, int B, int Hs, int Ws, int S, const int32_t* hbounds, const int32_t* hcoefs,
                      const int32_t* vbounds, const int32_t* vcoefs, const float* lut, float* out, void* stream) {
  REQUIRE(src && hbounds && hcoefs && vbounds && vcoefs && lut && out, "preprocess: null pointer");
  REQUIRE(B > 0 && B <= 65535 && Hs >= 1 && Ws >= 1 && Hs <= (1 << 16) && Ws <= (1 << 16), "preprocess: bad source shape");
  REQUIRE(S >= 1 && S <= 4096, "preprocess: output size must be 1..4096");
  // largest tile height whose source rectangle (rows x pitch bytes) and horizontally resampled rows
  // (rows x 64 columns x 3 planes) fit in 60 KiB of LDS
  int pitch = preprocess_row_pitch(Ws, S);
  int ty = 16, rows = 0;
  for (; ty >= 2; ty >>= 1) {
    rows = preprocess_tile_rows(Hs, S, ty);
    if ((size_t)rows * (pitch + 3 * 64) <= 60 * 1024) break;
  }
  if (ty < 2) {   // very large frames (downscale beyond ~6x): no LDS copy of the source, pass 1 gathers from global memory
    pitch = 0;
    for (ty = 16; ty >= 1; ty >>= 1) {
      rows = preprocess_tile_rows(Hs, S, ty);
      if ((size_t)rows * 3 * 64 <= 60 * 1024) break;
    }
  }
  REQUIRE(ty >= 1, "preprocess: source too tall for one output row to fit in LDS (downscale beyond ~100x)");
  launch_preprocess(src, B, Hs, Ws, S, hbounds, hcoefs, resample_ksize(Ws, S), vbounds, vcoefs, resample_ksize(Hs, S),
                    ty, rows, pitch, lut, out, (hipStream_t)stream);
  return finish("preprocess");
}

// ---- train-time input work (augment.hip)

size_t aaclip_color_jitter_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return up256((size_t)B * color_jitter_sum_blocks((long)H * W) * 8 + (size_t)B * 4);
}

int aaclip_color_jitter(const uint8_t* src, uint8_t* dst, int B, int H, int W, const float* factors,
                        const int32_t* apply, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(src && dst && factors && apply && ws, "color_jitter: null pointer");
  REQUIRE(B > 0 && B <= 65535 && H >= 1 && W >= 1 && H <= (1 << 16) && W <= (1 << 16), "color_jitter: bad frame shape");
  const size_t bytes = (size_t)B * H * W * 3;
  REQUIRE(bytes <= ((size_t)1 << 36), "color_jitter: more than 64 GiB of frames in one call");
  const size_t need = aaclip_color_jitter_workspace_bytes(B, H, W);
  const Buf b[] = {wr(dst, bytes), rd(src == dst ? nullptr : src, bytes), wr(ws, need, 8), rd(factors, (size_t)B * 12),
                   rd(apply, (size_t)B * 4)};   // in place: dst stands for both
  REQUIRE(!bufs_overlap(b[0], b[1]), "color_jitter: dst must be src itself (in place) or not overlap it");
  REQUIRE(bufs_misaligned(b) < 0, "color_jitter: workspace must be 8-byte aligned");
  REQUIRE(ws_bytes >= need, "color_jitter: workspace too small");
  REQUIRE(!bufs_clash(b), "color_jitter: dst and the workspace must not overlap each other or the inputs");
  launch_color_jitter(src, dst, B, H, W, factors, apply, ws, (hipStream_t)stream);
  return finish("color_jitter");
}

int aaclip_nearest_table(int in_size, int out_size, int32_t* idx) {
  REQUIRE(idx, "nearest_table: null pointer");
  REQUIRE(in_size >= 1 && out_size >= 1 && in_size <= (1 << 16) && out_size <= (1 << 16),
          "nearest_table: sizes must be 1..65536");
  nearest_table(in_size, out_size, idx);
  return 0;
}

int aaclip_mask_preprocess(const uint8_t* src, int B, int Hm, int Wm, int S, const int32_t* xmap, const int32_t* ymap,
                           const int32_t* normal, float* out, void* stream) {
  REQUIRE(src && xmap && ymap && out, "mask_preprocess: null pointer");
  REQUIRE(B > 0 && B <= 65535 && Hm >= 1 && Wm >= 1 && Hm <= (1 << 16) && Wm <= (1 << 16),
          "mask_preprocess: bad source shape");
  REQUIRE(S >= 1 && S <= 4096, "mask_preprocess: output size must be 1..4096");
  launch_mask_preprocess(src, B, Hm, Wm, S, xmap, ymap, normal, out, (hipStream_t)stream);
  return finish("mask_preprocess");
}

int aaclip_augment_geometric(const float* image, const float* mask, int B, int S, const float* angle_deg,
                             const int32_t* shift, const int32_t* flags, float* image_out, float* mask_out,
                             void* stream) {
  REQUIRE(image && mask && angle_deg && shift && flags && image_out && mask_out, "augment_geometric: null pointer");
  REQUIRE(B > 0 && B <= 65535, "augment_geometric: batch must be 1..65535");
  REQUIRE(S >= 1 && S <= 4096, "augment_geometric: size must be 1..4096");
  const size_t plane = (size_t)S * S * 4, ni = (size_t)B * 3 * plane, nm = (size_t)B * plane;
  const Buf b[] = {wr(image_out, ni), wr(mask_out, nm), rd(image, ni), rd(mask, nm), rd(angle_deg, (size_t)B * 4),
                   rd(shift, (size_t)B * 8), rd(flags, (size_t)B * 4)};
  REQUIRE(!bufs_clash(b),
          "augment_geometric: the outputs must not overlap the inputs or each other (every pixel is a gather)");
  launch_augment_geometric(image, mask, B, S, angle_deg, shift, flags, image_out, mask_out, (hipStream_t)stream);
  return finish("augment_geometric");
}

// ---- exact AUROC / AP (metrics.hip)
static inline bool metrics_n_ok(long n) { return n >= 2 && n <= 2147483647L; }

size_t aaclip_metrics_range_workspace_bytes(long n, long per_image) {
  if (!metrics_n_ok(n) || per_image < 0 || (per_image > 0 && n % per_image != 0)) return 0;
  if (!grid_fits(metrics_range_partials(n, per_image))) return 0;
  return up256(metrics_range_ws_bytes(n, per_image));
}

int aaclip_metrics_range(const float* scores, const uint8_t* labels, long n, long per_image, float* image_max,
                         void* record, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(scores && record && ws, "metrics_range: null pointer");
  REQUIRE(metrics_n_ok(n), "metrics_range: n must be 2 .. 2^31 - 1");
  REQUIRE(per_image >= 0 && (per_image == 0 || n % per_image == 0), "metrics_range: n must be a multiple of per_image");
  REQUIRE(grid_fits(metrics_range_partials(n, per_image)),
          "metrics_range: too many workgroups (one or more per image: n / per_image must stay below 2^24)");
  REQUIRE(!image_max || per_image > 0, "metrics_range: image maxima need per_image > 0");
  const size_t range_need = aaclip_metrics_range_workspace_bytes(n, per_image);
  const Buf b[] = {rd(scores, (size_t)n * 4, 4), rd(labels, (size_t)n), wr(record, 24, 8), wr(ws, range_need, 8),
                   wr(image_max, image_max ? (size_t)(n / per_image) * 4 : 0, 4)};
  REQUIRE(bufs_misaligned(b) < 0, "metrics_range: scores / image_max must be 4-byte, record / workspace 8-byte aligned");
  REQUIRE(!bufs_clash(b), "metrics_range: scores, labels, outputs and workspace must not overlap one another");
  REQUIRE(ws_bytes >= range_need, "metrics_range: workspace too small");
  launch_metrics_range(scores, labels, n, per_image, image_max, record, ws, (hipStream_t)stream);
  return finish("metrics_range");
}

int aaclip_metrics_normalise(const float* scores, float* out, long n, const void* range_record, void* stream) {
  REQUIRE(scores && out && range_record, "metrics_normalise: null pointer");
  REQUIRE(n >= 1 && n <= 2147483647L, "metrics_normalise: n must be 1 .. 2^31 - 1");
  const Buf b[] = {wr(out, (size_t)n * 4, 4), rd(scores == out ? nullptr : scores, (size_t)n * 4, 4),
                   rd(range_record, 24, 8)};   // in place: out stands for both
  REQUIRE(bufs_misaligned(b) < 0, "metrics_normalise: scores / out must be 4-byte, the record 8-byte aligned");
  REQUIRE(!bufs_overlap(b[0], b[1]), "metrics_normalise: out must be scores itself (in place) or not overlap it");
  REQUIRE(!bufs_clash(b), "metrics_normalise: out must not overlap the range record");
  launch_metrics_normalise(scores, out, n, range_record, (hipStream_t)stream);
  return finish("metrics_normalise");
}

size_t aaclip_metrics_sort_workspace_bytes(long n) { return metrics_n_ok(n) ? up256(metrics_sort_ws_bytes(n)) : 0; }
long aaclip_metrics_sort_group_items(void) { return metrics_sort_group_items(); }

int aaclip_metrics_sort(const float* scores, const uint8_t* labels, long n, int packed, uint32_t* keys,
                        uint8_t* labels_sorted, unsigned long long* out_of_range, void* ws, size_t ws_bytes,
                        void* stream) {
  REQUIRE(scores && labels && keys && out_of_range && ws, "metrics_sort: null pointer");
  REQUIRE(packed == 0 || packed == 1, "metrics_sort: packed must be 0 or 1");
  REQUIRE(packed || labels_sorted, "metrics_sort: labels_sorted is required when the label is not packed into the key");
  REQUIRE(metrics_n_ok(n), "metrics_sort: n must be 2 .. 2^31 - 1");
  const size_t sort_need = aaclip_metrics_sort_workspace_bytes(n);   // the workspace holds the other half of the ping-pong
  const Buf b[] = {rd(scores, (size_t)n * 4, 4), rd(labels, (size_t)n), wr(keys, (size_t)n * 4, 4),
                   wr(labels_sorted, (size_t)n), wr(out_of_range, 8, 8), wr(ws, sort_need, 8)};
  REQUIRE(bufs_misaligned(b) < 0, "metrics_sort: scores / keys must be 4-byte, out_of_range / workspace 8-byte aligned");
  REQUIRE(!bufs_overlap(b[2], b[0]) && !bufs_overlap(b[3], b[1]), "metrics_sort: the outputs must not overlap the inputs");
  REQUIRE(!bufs_clash(b), "metrics_sort: inputs, outputs and workspace must not overlap one another");
  REQUIRE(ws_bytes >= sort_need, "metrics_sort: workspace too small");
  launch_metrics_sort(scores, labels, n, packed, keys, labels_sorted, out_of_range, ws, (hipStream_t)stream);
  return finish("metrics_sort");
}

size_t aaclip_metrics_curve_workspace_bytes(long n) { return metrics_n_ok(n) ? up256(metrics_curve_ws_bytes(n)) : 0; }

int aaclip_metrics_curve(const uint32_t* keys, const uint8_t* labels_sorted, long n, int packed, void* record, void* ws,
                         size_t ws_bytes, void* stream) {
  REQUIRE(keys && record && ws, "metrics_curve: null pointer");
  REQUIRE(packed == 0 || packed == 1, "metrics_curve: packed must be 0 or 1");
  REQUIRE(packed || labels_sorted, "metrics_curve: labels_sorted is required when the label is not packed into the key");
  REQUIRE(metrics_n_ok(n), "metrics_curve: n must be 2 .. 2^31 - 1");
  const size_t curve_need = aaclip_metrics_curve_workspace_bytes(n);
  const Buf b[] = {rd(keys, (size_t)n * 4, 4), rd(labels_sorted, (size_t)n), wr(record, 40, 8), wr(ws, curve_need, 8)};
  REQUIRE(bufs_misaligned(b) < 0, "metrics_curve: keys must be 4-byte, record / workspace 8-byte aligned");
  REQUIRE(!bufs_clash(b), "metrics_curve: keys, labels, record and workspace must not overlap one another");
  REQUIRE(ws_bytes >= curve_need, "metrics_curve: workspace too small");
  launch_metrics_curve(keys, labels_sorted, n, packed, record, ws, (hipStream_t)stream);
  return finish("metrics_curve");
}

// ---- bootstrap of AUROC / AP over images (bootstrap.hip)
static inline bool bootstrap_shape_ok(long n, long images, long R) {
  return n >= 1 && n <= 2147483647L && images >= 1 && images <= bootstrap_max_images() && R >= 1 && R <= (1L << 20);
}

long aaclip_bootstrap_max_images(void) { return bootstrap_max_images(); }

size_t aaclip_bootstrap_workspace_bytes(long n, long images, long R) {
  return bootstrap_shape_ok(n, images, R) ? up256(bootstrap_ws_bytes(n, R)) : 0;
}

int aaclip_bootstrap_curves(const aaclip_bootstrap_plan* plan, const uint32_t* keys, const uint32_t* payload,
                            const uint8_t* counts, void* records, void* ws, size_t ws_bytes) {
  REQUIRE(plan && keys && payload && counts && records && ws, "bootstrap_curves: null pointer");
  REQUIRE(plan->struct_bytes == sizeof(aaclip_bootstrap_plan), "bootstrap_curves: plan->struct_bytes is not sizeof(aaclip_bootstrap_plan)");
  const long n = plan->n, images = plan->images, R = plan->replicates;
  REQUIRE(n >= 1 && n <= 2147483647L, "bootstrap_curves: n must be 1 .. 2^31 - 1");
  REQUIRE(images >= 1 && images <= bootstrap_max_images(), "bootstrap_curves: images must be 1 .. 1024 (the weight table of a replicate block fills 64 KiB of LDS)");
  REQUIRE(R >= 1 && R <= (1L << 20), "bootstrap_curves: R must be 1 .. 2^20");
  const size_t need = aaclip_bootstrap_workspace_bytes(n, images, R), n4 = (size_t)n * 4;
  const Buf b[] = {rd(keys, n4, 4), rd(payload, n4, 4), rd(counts, (size_t)R * images), wr(records, (size_t)R * 32, 8),
                   wr(ws, need, 8)};
  REQUIRE(bufs_misaligned(b) < 0, "bootstrap_curves: keys / payload must be 4-byte, records / workspace 8-byte aligned");
  REQUIRE(!bufs_clash(b), "bootstrap_curves: inputs, records and workspace must not overlap one another");
  REQUIRE(ws_bytes >= need, "bootstrap_curves: workspace too small");
  launch_bootstrap_curves(keys, payload, n, counts, images, R, records, ws, (hipStream_t)plan->stream);
  return finish("bootstrap_curves");
}

// ---- exact F1-max and the masks at a threshold (metrics.hip)
size_t aaclip_metrics_f1max_workspace_bytes(long n) { return metrics_n_ok(n) ? up256(metrics_f1max_ws_bytes(n)) : 0; }

int aaclip_metrics_f1max(const uint32_t* keys, const uint8_t* labels_sorted, long n, int packed, void* record, void* ws,
                         size_t ws_bytes, void* stream) {
  REQUIRE(keys && record && ws, "metrics_f1max: null pointer");
  REQUIRE(packed == 0 || packed == 1, "metrics_f1max: packed must be 0 or 1");
  REQUIRE(packed || labels_sorted, "metrics_f1max: labels_sorted is required when the label is not packed into the key");
  REQUIRE(metrics_n_ok(n), "metrics_f1max: n must be 2 .. 2^31 - 1");
  const size_t need = aaclip_metrics_f1max_workspace_bytes(n);
  const Buf b[] = {rd(keys, (size_t)n * 4, 4), rd(labels_sorted, (size_t)n),
                   wr(record, sizeof(aaclip_metrics_f1max_record), 8), wr(ws, need, 8)};
  REQUIRE(bufs_misaligned(b) < 0, "metrics_f1max: keys must be 4-byte, record / workspace 8-byte aligned");
  REQUIRE(!bufs_clash(b), "metrics_f1max: keys, labels, record and workspace must not overlap one another");
  REQUIRE(ws_bytes >= need, "metrics_f1max: workspace too small");
  launch_metrics_f1max(keys, labels_sorted, n, packed, record, ws, (hipStream_t)stream);
  return finish("metrics_f1max");
}

size_t aaclip_metrics_threshold_workspace_bytes(long n, long per_image) {
  if (!metrics_n_ok(n) || per_image < 0 || (per_image > 0 && n % per_image != 0)) return 0;
  if (!grid_fits(metrics_range_partials(n, per_image))) return 0;
  return up256(metrics_threshold_ws_bytes(n, per_image));
}

int aaclip_metrics_threshold(const float* scores, const uint8_t* labels, long n, long per_image,
                             const void* range_record, const void* f1max_record, uint8_t* mask,
                             uint32_t* image_counts, void* totals, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(scores && f1max_record && ws, "metrics_threshold: null pointer");
  REQUIRE(mask || image_counts || totals, "metrics_threshold: no output (mask, image_counts and totals are all null)");
  REQUIRE(metrics_n_ok(n), "metrics_threshold: n must be 2 .. 2^31 - 1");
  REQUIRE(per_image >= 0 && (per_image == 0 || n % per_image == 0),
          "metrics_threshold: n must be a multiple of per_image");
  REQUIRE(grid_fits(metrics_range_partials(n, per_image)),
          "metrics_threshold: too many workgroups (one or more per image: n / per_image must stay below 2^24)");
  REQUIRE(!image_counts || (labels && per_image > 0), "metrics_threshold: per-image counts need labels and per_image > 0");
  const size_t need = aaclip_metrics_threshold_workspace_bytes(n, per_image);
  const Buf b[] = {wr(mask, (size_t)n), wr(image_counts, image_counts ? (size_t)(n / per_image) * 16 : 0, 4),
                   wr(totals, sizeof(aaclip_metrics_threshold_record), 8), wr(ws, need, 8), rd(scores, (size_t)n * 4, 4),
                   rd(labels, (size_t)n), rd(range_record, 24, 8), rd(f1max_record, sizeof(aaclip_metrics_f1max_record), 8)};
  REQUIRE(bufs_misaligned(b) < 0,
          "metrics_threshold: scores / image_counts must be 4-byte, records / totals / workspace 8-byte aligned");
  REQUIRE(!bufs_clash(b), "metrics_threshold: scores, labels, records, outputs and workspace must not overlap one another");
  REQUIRE(ws_bytes >= need, "metrics_threshold: workspace too small");
  launch_metrics_threshold(scores, labels, n, per_image, range_record, f1max_record, mask, image_counts, totals, ws,
                           (hipStream_t)stream);
  return finish("metrics_threshold");
}

// ---- fused Adam / AdamW step and its gradient norm (optim.hip)
// the checks the entries share; need: 0 = the counts alone (workspace size), 1 = g as well (grad norm), 2 = p, g, m, v
// and the group index.  nullptr = fine
static const char* optim_tensors_check(const aaclip_optim_tensors* t, int need, int n_groups) {
  if (!t) return "tensors is null";
  if (t->struct_bytes != sizeof(aaclip_optim_tensors)) return "tensors->struct_bytes is not sizeof(aaclip_optim_tensors)";
  if (t->count < 0) return "tensors->count is negative";
  if (t->count > 0 && !t->items) return "tensors->items is null";
  for (long i = 0; i < t->count; ++i) {
    const aaclip_optim_tensor& it = t->items[i];
    if (it.n < 0) return "a tensor has n < 0";
    if (it.n > OPTIM_MAX_ELEMS) return "a tensor has more than 2^27 * 16384 elements";
    if (need == 2 && (it.group < 0 || it.group >= n_groups)) return "a tensor's group index is out of range";
    if (it.n == 0 || need == 0) continue;
    if (!it.g || (need == 2 && (!it.p || !it.m || !it.v))) return "a tensor with n > 0 has a null pointer";
    uintptr_t bits = (uintptr_t)it.g;
    if (need == 2) bits |= (uintptr_t)it.p | (uintptr_t)it.m | (uintptr_t)it.v;
    if (bits & 3) return "a tensor's pointers must be 4-byte aligned";
  }
  return nullptr;
}

// the element counts as optim_pack.h walks them; the caller frees
static long* optim_counts(const aaclip_optim_tensors* t) {
  long* counts = (long*)malloc(sizeof(long) * (size_t)(t->count > 0 ? t->count : 1));
  for (long i = 0; counts && i < t->count; ++i) counts[i] = t->items[i].n;
  return counts;
}

size_t aaclip_optim_grad_norm_workspace_bytes(const aaclip_optim_tensors* tensors) {
  if (optim_tensors_check(tensors, 0, 0)) return 0;
  long chunks = 0;
  for (long i = 0; i < tensors->count; ++i) chunks += optim_chunks(tensors->items[i].n);
  return up256(optim_grad_norm_ws_bytes(chunks));
}

int aaclip_optim_grad_norm(const aaclip_optim_tensors* tensors, float max_norm, void* record, void* workspace,
                           size_t workspace_bytes, void* stream) {
  if (const char* m = optim_tensors_check(tensors, 1, 0)) return fail(-1, in("optim_grad_norm", m));
  REQUIRE(max_norm > 0.0f, "optim_grad_norm: max_norm must be above 0");
  REQUIRE(record && workspace, "optim_grad_norm: null pointer");
  const size_t need = aaclip_optim_grad_norm_workspace_bytes(tensors);
  const Buf b[] = {wr(record, sizeof(aaclip_optim_record), 8), wr(workspace, need, 8)};
  REQUIRE(bufs_misaligned(b) < 0, "optim_grad_norm: record and workspace must be 8-byte aligned");
  REQUIRE(workspace_bytes >= need, "optim_grad_norm: workspace too small");
  REQUIRE(!bufs_clash(b), "optim_grad_norm: record and workspace must not overlap");
  for (long i = 0; i < tensors->count; ++i) {   // the table's read-only rows: one gradient per tensor
    const Buf g = rd(tensors->items[i].g, (size_t)tensors->items[i].n * 4, 4);
    REQUIRE(!bufs_overlap(b[0], g) && !bufs_overlap(b[1], g), "optim_grad_norm: record and workspace must not overlap a gradient");
  }
  long* counts = optim_counts(tensors);
  if (!counts) return fail(-3, "optim_grad_norm: out of memory");
  launch_optim_grad_norm(tensors->items, counts, tensors->count, max_norm, record, workspace, (hipStream_t)stream);
  free(counts);
  return finish("optim_grad_norm");
}

int aaclip_optim_adam_step(const aaclip_optim_tensors* tensors, const aaclip_optim_group* groups, int n_groups,
                           const void* record_or_null, void* stream) {
  REQUIRE(groups, "optim_adam_step: groups is null");
  REQUIRE(n_groups >= 1 && n_groups <= AACLIP_OPTIM_MAX_GROUPS, "optim_adam_step: n_groups must be 1 .. 8");
  if (const char* m = optim_tensors_check(tensors, 2, n_groups)) return fail(-1, in("optim_adam_step", m));
  REQUIRE(((uintptr_t)record_or_null & 7) == 0, "optim_adam_step: record must be 8-byte aligned");
  OptimGroupScalars scalars[AACLIP_OPTIM_MAX_GROUPS];
  for (int i = 0; i < n_groups; ++i) {
    const aaclip_optim_group& g = groups[i];
    REQUIRE(g.step >= 1, "optim_adam_step: step must be at least 1");
    REQUIRE(g.lr >= 0.0 && g.lr < INFINITY && g.eps >= 0.0 && g.eps < INFINITY && g.weight_decay >= 0.0 &&
                g.weight_decay < INFINITY,
            "optim_adam_step: lr, eps and weight_decay must be finite and not negative");
    REQUIRE(g.beta1 >= 0.0 && g.beta1 < 1.0 && g.beta2 >= 0.0 && g.beta2 < 1.0,
            "optim_adam_step: the betas must lie in [0, 1)");
    REQUIRE(g.decoupled == 0 || g.decoupled == 1, "optim_adam_step: decoupled must be 0 or 1");
    // fp64 on the host, rounded once
    const double bc1 = 1.0 - pow(g.beta1, (double)g.step), bc2 = 1.0 - pow(g.beta2, (double)g.step);
    OptimGroupScalars& h = scalars[i];
    h.beta1 = (float)g.beta1, h.one_minus_beta1 = (float)(1.0 - g.beta1);
    h.beta2 = (float)g.beta2, h.one_minus_beta2 = (float)(1.0 - g.beta2);
    h.step_size = (float)(g.lr / bc1);
    h.sqrt_bc2 = (float)sqrt(bc2);
    h.eps = (float)g.eps;
    h.coupled = !g.decoupled && g.weight_decay != 0.0;
    h.weight_decay = h.coupled ? (float)g.weight_decay : 0.0f;
    h.decay = g.decoupled ? (float)(1.0 - g.lr * g.weight_decay) : 1.0f;
  }
  long* counts = optim_counts(tensors);
  if (!counts) return fail(-3, "optim_adam_step: out of memory");
  launch_optim_adam_step(tensors->items, counts, tensors->count, scalars, n_groups, record_or_null, (hipStream_t)stream);
  free(counts);
  return finish("optim_adam_step");
}

// ---- per-region overlap, AUPRO (regions.hip; the pair sort is metrics.hip's)
static inline long regions_pixels(long images, long H, long W) {   // 0 where the product is refused
  if (images < 1 || H < 1 || W < 1 || H > 2147483647L || W > 2147483647L || images > 2147483647L) return 0;
  if (H > 2147483647L / W || images > 2147483647L / (H * W)) return 0;
  const long n = images * H * W;
  return metrics_n_ok(n) ? n : 0;
}

size_t aaclip_metrics_regions_workspace_bytes(long images, long H, long W) {
  const long n = regions_pixels(images, H, W);
  return n ? up256(metrics_regions_ws_bytes(n)) : 0;
}

int aaclip_metrics_regions(const uint8_t* mask, long images, long H, long W, int connectivity, uint32_t* region,
                           uint32_t* area, void* record, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(mask && region && area && record && ws, "metrics_regions: null pointer");
  REQUIRE(connectivity == 4 || connectivity == 8, "metrics_regions: connectivity must be 4 or 8");
  const long n = regions_pixels(images, H, W);
  REQUIRE(n != 0, "metrics_regions: images, H, W must be positive with 2 .. 2^31 - 1 pixels in all");
  const size_t need = aaclip_metrics_regions_workspace_bytes(images, H, W), n4 = (size_t)n * 4;
  const Buf b[] = {rd(mask, (size_t)n), wr(region, n4, 4), wr(area, n4, 4), wr(record, 24, 8), wr(ws, need, 8)};
  REQUIRE(bufs_misaligned(b) < 0, "metrics_regions: region / area must be 4-byte, record / workspace 8-byte aligned");
  REQUIRE(!bufs_clash(b), "metrics_regions: mask, outputs, record and workspace must not overlap one another");
  REQUIRE(ws_bytes >= need, "metrics_regions: workspace too small");
  launch_metrics_regions(mask, n, (int)H, (int)W, connectivity, region, area, record, ws, (hipStream_t)stream);
  return finish("metrics_regions");
}

size_t aaclip_metrics_sort_pairs_workspace_bytes(long n) {
  return metrics_n_ok(n) ? up256(metrics_sort_pairs_ws_bytes(n)) : 0;
}

int aaclip_metrics_sort_pairs(const float* scores, const uint32_t* values, long n, uint32_t* keys,
                              uint32_t* values_sorted, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(scores && values && keys && values_sorted && ws, "metrics_sort_pairs: null pointer");
  REQUIRE(metrics_n_ok(n), "metrics_sort_pairs: n must be 2 .. 2^31 - 1");
  const size_t need = aaclip_metrics_sort_pairs_workspace_bytes(n), n4 = (size_t)n * 4;
  const Buf b[] = {rd(scores, n4, 4), rd(values, n4, 4), wr(keys, n4, 4), wr(values_sorted, n4, 4), wr(ws, need, 8)};
  REQUIRE(bufs_misaligned(b) < 0,
          "metrics_sort_pairs: scores / values / keys must be 4-byte, the workspace 8-byte aligned");
  REQUIRE(!bufs_overlap(b[2], b[0]) && !bufs_overlap(b[2], b[1]) && !bufs_overlap(b[3], b[0]) && !bufs_overlap(b[3], b[1]),
          "metrics_sort_pairs: the outputs must not overlap the inputs");
  REQUIRE(!bufs_clash(b), "metrics_sort_pairs: inputs, outputs and workspace must not overlap one another");
  REQUIRE(ws_bytes >= need, "metrics_sort_pairs: workspace too small");
  launch_metrics_sort_pairs(scores, values, n, keys, values_sorted, ws, (hipStream_t)stream);
  return finish("metrics_sort_pairs");
}

size_t aaclip_metrics_pro_curve_workspace_bytes(long n) {
  return metrics_n_ok(n) ? up256(metrics_pro_curve_ws_bytes(n)) : 0;
}

int aaclip_metrics_pro_curve(const uint32_t* keys, const uint32_t* areas_sorted, long n, const void* regions_record,
                             double fpr_limit, void* record, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(keys && areas_sorted && regions_record && record && ws, "metrics_pro_curve: null pointer");
  REQUIRE(metrics_n_ok(n), "metrics_pro_curve: n must be 2 .. 2^31 - 1");
  REQUIRE(fpr_limit > 0.0 && fpr_limit <= 1.0, "metrics_pro_curve: fpr_limit must lie in (0, 1]");
  const size_t need = aaclip_metrics_pro_curve_workspace_bytes(n), n4 = (size_t)n * 4;
  const Buf b[] = {rd(keys, n4, 4), rd(areas_sorted, n4, 4), rd(regions_record, 24, 8), wr(record, 40, 8), wr(ws, need, 8)};
  REQUIRE(bufs_misaligned(b) < 0, "metrics_pro_curve: keys / areas must be 4-byte, records / workspace 8-byte aligned");
  REQUIRE(!bufs_clash(b), "metrics_pro_curve: keys, areas, records and workspace must not overlap one another");
  REQUIRE(ws_bytes >= need, "metrics_pro_curve: workspace too small");
  launch_metrics_pro_curve(keys, areas_sorted, n, regions_record, fpr_limit, record, ws, (hipStream_t)stream);
  return finish("metrics_pro_curve");
}

// ---- the table of the regions (region_table.hip)
size_t aaclip_region_table_workspace_bytes(long images, long H, long W) {
  const long n = regions_pixels(images, H, W);
  return n ? up256(region_table_ws_bytes(n, images)) : 0;
}

int aaclip_region_table(const uint32_t* region, const uint32_t* area, const float* scores, const void* range_record,
                        const uint8_t* other, long images, long H, long W, long min_area, long capacity, void* rows,
                        int32_t* image_offsets, uint8_t* kept_mask, void* record, void* ws, size_t ws_bytes,
                        void* stream) {
  REQUIRE(region && area && scores && image_offsets && record && ws, "region_table: null pointer");
  const long n = regions_pixels(images, H, W);
  REQUIRE(n != 0, "region_table: images, H, W must be positive with 2 .. 2^31 - 1 pixels in all");
  REQUIRE(min_area >= 1, "region_table: min_area must be at least 1");
  REQUIRE(capacity >= 0, "region_table: capacity must not be negative");
  REQUIRE(capacity == 0 || rows, "region_table: rows is null with capacity > 0");
  const size_t need = aaclip_region_table_workspace_bytes(images, H, W), n4 = (size_t)n * 4;
  const Buf b[] = {wr(rows, (size_t)(capacity < n ? capacity : n) * sizeof(aaclip_region_row), 8),
                   wr(image_offsets, (size_t)(images + 1) * 4, 4), wr(kept_mask, (size_t)n),
                   wr(record, sizeof(aaclip_region_table_record), 8), wr(ws, need, 8), rd(region, n4, 4), rd(area, n4, 4),
                   rd(scores, n4, 4), rd(range_record, 24, 8), rd(other, (size_t)n)};
  REQUIRE(bufs_misaligned(b) < 0,
          "region_table: region / area / scores / image_offsets must be 4-byte, rows / records / workspace 8-byte aligned");
  REQUIRE(!bufs_clash(b), "region_table: inputs, outputs, records and workspace must not overlap one another");
  REQUIRE(ws_bytes >= need, "region_table: workspace too small");
  launch_region_table(region, area, scores, range_record, other, images, (int)H, (int)W, min_area, capacity, rows,
                      image_offsets, kept_mask, record, ws, (hipStream_t)stream);
  return finish("region_table");
}

// ---- few-shot support bank (support.hip)
static const char* support_shape_check(long M, long N, int E, int form) {
  if (form != AACLIP_SUPPORT_FP16 && form != AACLIP_SUPPORT_FP32) return "form must be AACLIP_SUPPORT_FP16 or AACLIP_SUPPORT_FP32";
  if (M < 1 || N < 1 || M > 0x7FFFFFFFl || N > 0x7FFFFFFFl) return "M and N must be 1 .. 2^31 - 1";
  if (E < 64 || E > 1024 || E % 32 != 0) return "E must be a multiple of 32 in 64 .. 1024";
  return nullptr;
}

size_t aaclip_support_nearest_workspace_bytes(long M, long N, int E, int form) {
  return support_shape_check(M, N, E, form) ? 0 : support_ws_bytes(M);
}

int aaclip_support_nearest(const float* q, long M, const void* bank, long N, int E, int form, float* best_cos,
                           int* best_idx, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(q && bank && best_cos && ws, "support_nearest: null pointer");
  if (const char* m = support_shape_check(M, N, E, form)) return fail(-1, in("support_nearest", m));
  const size_t need = support_ws_bytes(M);
  const Buf b[] = {rd(q, (size_t)M * E * 4, 16), rd(bank, (size_t)N * E * (form == AACLIP_SUPPORT_FP16 ? 2 : 4), 16),
                   wr(best_cos, (size_t)M * 4, 4), wr(best_idx, (size_t)M * 4, 4), wr(ws, need, 8)};
  const int bad = bufs_misaligned(b);
  REQUIRE(bad < 0 || bad >= 2, in("support_nearest", "pointers must be 16-byte aligned"));
  REQUIRE(bad < 0, "support_nearest: best_cos / best_idx must be 4-byte, the workspace 8-byte aligned");
  REQUIRE(ws_bytes >= need, "support_nearest: workspace too small");
  REQUIRE(!bufs_clash(b), "support_nearest: outputs and workspace must not overlap one another or the inputs");
  launch_support_nearest(q, M, bank, N, E, form, best_cos, best_idx, ws, (hipStream_t)stream);
  return finish("support_nearest");
}

int aaclip_support_bank_rows(const float* rows, long N, int E, int form, void* bank, void* stream) {
  REQUIRE(rows && bank, "support_bank_rows: null pointer");
  if (const char* m = support_shape_check(1, N, E, form)) return fail(-1, in("support_bank_rows", m));
  const Buf b[] = {rd(rows, (size_t)N * E * 4, 16), wr(bank, (size_t)N * E * (form == AACLIP_SUPPORT_FP16 ? 2 : 4), 16)};
  REQUIRE(bufs_misaligned(b) < 0, in("support_bank_rows", "pointers must be 16-byte aligned"));
  REQUIRE(!bufs_clash(b), "support_bank_rows: rows and bank must not overlap");
  launch_support_bank_rows(rows, N, E, form, bank, (hipStream_t)stream);
  return finish("support_bank_rows");
}

int aaclip_support_map(const float* const* best_cos, int NL, const float* base, float weight, float* out, int B, int g,
                       int S, int ksize, float sigma, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(best_cos && out && ws, "support_map: null pointer");
  REQUIRE(NL >= 1 && NL <= 4, "support_map: 1..4 levels");
  REQUIRE(map_shape_ok(B, g, S), "support_map: bad shape (grid <= 40)");
  REQUIRE(ksize >= 1 && ksize <= 15 && ksize / 2 < g, "support_map: kernel size must be 1..15 and < 2*grid");
  REQUIRE(sigma > 0.f, "support_map: sigma must be positive");
  const long BP = (long)B * g * g, n = (long)B * S * S;
  REQUIRE(ws_bytes >= (size_t)NL * BP * 4, "support_map: workspace too small");
  const size_t lb = (size_t)BP * 4;
  const Buf b[] = {wr(out, (size_t)n * 4), rd(base, (size_t)n * 4), wr(ws, (size_t)NL * lb), rd(best_cos[0], lb),
                   rd(NL > 1 ? best_cos[1] : nullptr, lb), rd(NL > 2 ? best_cos[2] : nullptr, lb),
                   rd(NL > 3 ? best_cos[3] : nullptr, lb)};
  REQUIRE(!bufs_overlap(b[0], b[1]), "support_map: base must not overlap out");
  for (int l = 0; l < NL; ++l) REQUIRE(best_cos[l], "support_map: null level pointer");
  REQUIRE(!bufs_clash(b), "support_map: out and the workspace must not overlap each other or the inputs");
  hipStream_t s = (hipStream_t)stream;
  float* pre = (float*)ws;
  for (int l = 0; l < NL; ++l) launch_support_dist(best_cos[l], pre + (size_t)l * BP, BP, s);
  launch_blur_upsample(pre, out, B, g, S, NL, ksize, sigma, s);
  launch_support_add(base, weight, out, n, s);
  return finish("support_map");
}

// ---- coreset of the support bank (coreset.hip)
static const char* coreset_shape_check(long N, int E) {
  if (N < 1 || N > 0x7FFFFFFFl) return "N must be 1 .. 2^31 - 1";
  if (E < 32 || E > 1024 || E % 32 != 0) return "E must be a multiple of 32 in 32 .. 1024";
  return nullptr;
}

int aaclip_coreset_rows(const float* rows, long N, int E, int16_t* q, int32_t* norm2, void* stream) {
  REQUIRE(rows && q && norm2, "coreset_rows: null pointer");
  if (const char* m = coreset_shape_check(N, E)) return fail(-1, in("coreset_rows", m));
  const Buf b[] = {rd(rows, (size_t)N * E * 4, 16), wr(q, (size_t)N * E * 2, 16), wr(norm2, (size_t)N * 4, 4)};
  const int bad = bufs_misaligned(b);
  REQUIRE(bad < 0 || bad == 2, in("coreset_rows", "pointers must be 16-byte aligned"));
  REQUIRE(bad < 0, "coreset_rows: norm2 must be 4-byte aligned");
  REQUIRE(!bufs_clash(b),
          "coreset_rows: rows, q and norm2 must not overlap");
  launch_coreset_rows(rows, N, E, q, norm2, (hipStream_t)stream);
  return finish("coreset_rows");
}

int aaclip_coreset_unit_rows(const float* rows, long N, int E, float* out, void* stream) {
  REQUIRE(rows && out, "coreset_unit_rows: null pointer");
  if (const char* m = coreset_shape_check(N, E)) return fail(-1, in("coreset_unit_rows", m));
  const Buf b[] = {rd(rows, (size_t)N * E * 4, 16), wr(out, (size_t)N * E * 4, 16)};
  REQUIRE(bufs_misaligned(b) < 0, in("coreset_unit_rows", "pointers must be 16-byte aligned"));
  REQUIRE(!bufs_clash(b), "coreset_unit_rows: rows and out must not overlap");
  launch_coreset_unit_rows(rows, N, E, out, (hipStream_t)stream);
  return finish("coreset_unit_rows");
}

size_t aaclip_coreset_select_workspace_bytes(long N, int E, long n) {
  return coreset_shape_check(N, E) || n < 1 || n > N ? 0 : coreset_ws_bytes(n);
}

int aaclip_coreset_select(const int16_t* q, const int32_t* norm2, long N, int E, long n, long start, int32_t* picks,
                          uint32_t* radius2, uint32_t* min_d2, void* ws, size_t ws_bytes, void* stream) {
  REQUIRE(q && norm2 && picks && radius2 && min_d2 && ws, "coreset_select: null pointer");
  if (const char* m = coreset_shape_check(N, E)) return fail(-1, in("coreset_select", m));
  REQUIRE(n >= 1 && n <= N, "coreset_select: n must be 1 .. N");
  REQUIRE(start >= 0 && start < N, "coreset_select: start must be 0 .. N - 1");
  const size_t need = coreset_ws_bytes(n);
  const Buf b[] = {rd(q, (size_t)N * E * 2, 16), rd(norm2, (size_t)N * 4, 4), wr(picks, (size_t)n * 4, 4),
                   wr(radius2, (size_t)(n + 1) * 4, 4), wr(min_d2, (size_t)N * 4, 4), wr(ws, need, 8)};
  const int bad = bufs_misaligned(b);
  REQUIRE(bad != 0, in("coreset_select", "pointers must be 16-byte aligned"));
  REQUIRE(bad < 0, "coreset_select: norm2 / picks / radius2 / min_d2 must be 4-byte, the workspace 8-byte aligned");
  REQUIRE(ws_bytes >= need, "coreset_select: workspace too small");
  REQUIRE(!bufs_clash(b), "coreset_select: outputs and workspace must not overlap one another or the inputs");
  launch_coreset_select(q, norm2, N, E, n, start, picks, radius2, min_d2, ws, (hipStream_t)stream);
  return finish("coreset_select");
}

// ---- tiled inference (tiles.hip; the geometry and its checks: tile_plan.h)
int aaclip_tile_canvas(int tile, int grid, int overlap) {
  const long c = tile_canvas_side(tile, grid, overlap);
  if (c < 0) return fail(-1, "aaclip_tile_canvas: tile >= 1, grid >= 1, 0 <= overlap <= tile / 2 and a canvas side within int");
  return (int)c;
}

// every check of a tile entry: 0 with *launch set when there is work, 0 with *launch clear for images == 0, or the code
static int tile_entry_check(const char* entry, const aaclip_tile_plan* plan, const void* canvas, const void* tiles,
                            TileGeom* g, bool* launch) {
  *launch = false;
  if (const char* m = plan_refusal(plan, "aaclip_tile_plan.struct_bytes does not match this library (binding generated "
                                         "from another header?)"))
    return fail(-1, in(entry, m));
  if (const char* m = tile_plan_check(plan->images, plan->channels, plan->tile, plan->grid, plan->overlap))
    return fail(-1, in(entry, m));
  if (!canvas || !tiles) return fail(-1, in(entry, "null pointer"));
  *g = tile_geom(plan->channels, plan->tile, plan->grid, plan->overlap);
  const size_t per_image = (size_t)plan->images * (size_t)plan->channels * 4;
  // one of the two is the entry's output: with two buffers the pair is checked whichever it is
  const Buf b[] = {wr(canvas, per_image * (size_t)g->C * (size_t)g->C, 4),
                   wr(tiles, per_image * (size_t)g->G * (size_t)g->G * (size_t)g->S * (size_t)g->S, 4)};
  if (bufs_misaligned(b) >= 0) return fail(-1, in(entry, "canvas and tiles must be 4-byte aligned"));
  if (bufs_clash(b)) return fail(-1, in(entry, "canvas and tiles must not overlap"));
  *launch = plan->images > 0;
  return 0;
}

int aaclip_tile_gather(const aaclip_tile_plan* plan, const float* canvas, float* tiles) {
  TileGeom g;
  bool launch;
  if (const int rc = tile_entry_check("aaclip_tile_gather", plan, canvas, tiles, &g, &launch)) return rc;
  if (!launch) return 0;
  launch_tile_gather(g, plan->images, canvas, tiles, (hipStream_t)plan->stream);
  return finish("aaclip_tile_gather");
}

int aaclip_tile_stitch(const aaclip_tile_plan* plan, const float* tiles, float* canvas) {
  TileGeom g;
  bool launch;
  if (const int rc = tile_entry_check("aaclip_tile_stitch", plan, canvas, tiles, &g, &launch)) return rc;
  if (!launch) return 0;
  launch_tile_stitch(g, plan->images, tiles, canvas, (hipStream_t)plan->stream);
  return finish("aaclip_tile_stitch");
}

// ---- heat-map overlays (overlay.hip; the plan checks, offsets and pixel functions: overlay_plan.h)
int aaclip_overlay_render(const aaclip_overlay_plan* plan, const float* frames, const float* maps, const void* range_record,
                          const uint8_t* pred, const uint8_t* truth, const uint8_t* lut, uint8_t* out) {
  const char* entry = "aaclip_overlay_render";
  if (const char* m = plan_refusal(plan, "aaclip_overlay_plan.struct_bytes does not match this library (binding "
                                         "generated from another header?)"))
    return fail(-1, in(entry, m));
  if (const char* m = overlay_plan_check(plan->images, plan->height, plan->width, plan->panels, plan->alpha256,
                                         plan->thickness, plan->std))
    return fail(-1, in(entry, m));
  if (!frames || !maps || !lut || !out) return fail(-1, in(entry, "null pointer (frames, maps, lut and out are required)"));
  if ((plan->panels & OVERLAY_TRUTH) && !truth) return fail(-1, in(entry, "the truth panel needs a truth mask"));
  const size_t pixels = (size_t)plan->images * (size_t)plan->height * (size_t)plan->width;
  const Buf b[] = {rd(frames, pixels * 12, 4), rd(maps, pixels * 4, 4), rd(range_record, 24, 8), rd(pred, pixels),
                   rd(truth, pixels), rd(lut, 768), wr(out, pixels * 3 * (size_t)overlay_panel_count(plan->panels))};
  const int bad = bufs_misaligned(b);
  if (bad == 0 || bad == 1) return fail(-1, in(entry, "frames and maps must be 4-byte aligned"));
  if (bad >= 0) return fail(-1, in(entry, "the range record must be 8-byte aligned"));
  if (bufs_clash(b)) return fail(-1, in(entry, "out must not overlap an input"));
  if (plan->images == 0) return 0;
  OverlayGeom g = overlay_geom(plan->height, plan->width, plan->panels, plan->alpha256, plan->thickness, pred != nullptr,
                               truth != nullptr);
  for (int c = 0; c < 3; ++c) {
    g.pred_colour[c] = plan->pred_colour[c], g.truth_colour[c] = plan->truth_colour[c];
    g.mean[c] = plan->mean[c], g.sd[c] = plan->std[c];
  }
  launch_overlay_render(g, plan->images, frames, maps, range_record, pred, truth, lut, out, (hipStream_t)plan->stream);
  return finish("aaclip_overlay_render");
}

// ---- PNG encoding (png.hip; the format, the geometry and the plan checks: png_plan.h)
static const char* png_plan_refusal(const aaclip_png_plan* plan) {
  if (const char* m = plan_refusal(plan, "aaclip_png_plan.struct_bytes does not match this library (binding generated "
                                         "from another header?)"))
    return m;
  return png_plan_check(plan->images, plan->height, plan->width, plan->channels);
}

size_t aaclip_png_workspace_bytes(const aaclip_png_plan* plan) {
  if (png_plan_refusal(plan)) return 0;
  return png_workspace_bytes(png_geom(plan->images, plan->height, plan->width, plan->channels));
}

size_t aaclip_png_capacity_bytes(const aaclip_png_plan* plan) {
  if (png_plan_refusal(plan)) return 0;
  return png_capacity_bytes(png_geom(plan->images, plan->height, plan->width, plan->channels));
}

int aaclip_png_encode(const aaclip_png_plan* plan, const uint8_t* pixels, void* workspace, size_t ws_bytes, uint8_t* payload,
                      size_t capacity, int64_t* offsets) {
  const char* entry = "aaclip_png_encode";
  if (const char* m = png_plan_refusal(plan)) return fail(-1, in(entry, m));
  if (plan->images == 0) return 0;
  if (!pixels || !workspace || !payload || !offsets) return fail(-1, in(entry, "null pointer"));
  const PngGeom g = png_geom(plan->images, plan->height, plan->width, plan->channels);
  if (ws_bytes < png_workspace_bytes(g)) return fail(-1, in(entry, "workspace too small (aaclip_png_workspace_bytes)"));
  if (capacity < png_capacity_bytes(g)) return fail(-1, in(entry, "payload capacity too small (aaclip_png_capacity_bytes)"));
  const Buf b[] = {rd(pixels, (size_t)g.images * (size_t)g.H * (size_t)g.R), wr(workspace, png_workspace_bytes(g), 16),
                   wr(payload, capacity), wr(offsets, ((size_t)g.images + 1) * 8, 8)};
  const int bad = bufs_misaligned(b);
  if (bad == 1) return fail(-1, in(entry, "the workspace must be 16-byte aligned"));
  if (bad >= 0) return fail(-1, in(entry, "offsets must be 8-byte aligned"));
  if (bufs_overlap(b[2], b[0]) || bufs_overlap(b[3], b[0]))
    return fail(-1, in(entry, "payload and offsets must not overlap pixels"));
  if (bufs_clash(b)) return fail(-1, in(entry, "the workspace, payload and offsets must not overlap one another or pixels"));
  launch_png_encode(g, pixels, workspace, payload, offsets, (hipStream_t)plan->stream);
  return finish("aaclip_png_encode");
}

int aaclip_text_embed(const int32_t* tokens, const float* table, const float* pos, float* x, int n, int T, int D,
                      int vocab, void* stream) {
  REQUIRE(tokens && table && pos && x, "text_embed: null pointer");
  REQUIRE(n > 0 && T > 0 && D % 4 == 0 && vocab > 0, "text_embed: bad shape");
  launch_embed_text(tokens, table, pos, x, n, T, D, vocab, (hipStream_t)stream);
  return finish("text_embed");
}

int aaclip_row_head(const float* x, const int32_t* tokens, const float* ln_w, const float* ln_b, const void* proj_w,
                    int act, float* out, int n, int T, int D, int E, int mode, int dtype, void* ws, size_t ws_bytes,
                    void* stream) {
  REQUIRE(dtype_ok(dtype), "row_head: bad dtype");
  REQUIRE(x && ln_w && ln_b && proj_w && out && ws, "row_head: null pointer");
  REQUIRE(mode == 1 || tokens, "row_head: tokens required for EOT mode");
  REQUIRE(n > 0 && T > 0, "row_head: bad shape");
  REQUIRE_ROW_WIDTH(D);
  REQUIRE(E % 128 == 0, "row_head: E must be a multiple of 128");
  const size_t es = esize(dtype);
  const long rows = (long)n * T;
  size_t need = up256((size_t)rows * D * es) + up256((size_t)n * D * es);
  REQUIRE(ws_bytes >= need, "row_head: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* ln_out = (char*)ws;
  char* picked = ln_out + up256((size_t)rows * D * es);
  GemmParams p = gemm_params(picked, split_w(dtype) * D, proj_w, nullptr, out, E, n, E, D);
  p.act = act;
  const char* gm = gemm_check(dtype, EPI_ACT_F32, p);
  if (gm) return fail(-1, gm);
  launch_layernorm(dtype, x, ln_w, ln_b, ln_out, rows, D, 1e-5f, s);
  launch_gather_rows(dtype, ln_out, picked, tokens, n, T, D, mode, s);
  launch_gemm(dtype, EPI_ACT_F32, p, s);
  return finish("row_head");
}

}  // extern "C"
