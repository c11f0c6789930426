// C ABI of libmst_hip.so (include/mst_hip.h): argument checking, dtype dispatch and the two
// orchestrators -- mst_vit_encode (per-slice DINOv2 ViT; mst_vit_encode_features: the same with RGB input and
// taps of the residual stream) and mst_slice_fusion (across-slice transformer + head).  Nothing here allocates or synchronises: every launch goes to the caller's
// stream, scratch comes from the caller's workspace, so a caller may capture a call into a hipGraph.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <new>
#include <vector>

#include "mst_common.h"

static thread_local char g_err[512] = "";

void mst_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int mst_check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        mst_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return MST_ELAUNCH;
    }
    return MST_OK;
}

void mst_allow_lds(const void* kernel, int bytes, mst_lds_once* slot) {
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 63;   // unknown / far device: always set
    std::lock_guard<std::mutex> lk(mu);
    if (dev != 63 && (slot->done_mask >> dev) & 1ull) return;
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    slot->done_mask |= 1ull << dev;
}

int mst_persistent_grid(void) {
    static std::mutex mu;
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    std::lock_guard<std::mutex> lk(mu);
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 8) n = 256;
        cus[dev] = n / 8 * 8;
    }
    return cus[dev];
}

// ---- optional per-kernel event timing (bench only): state lives in a caller-owned mst_profiler -------------
struct mst_profiler {
    struct Rec { hipEvent_t a, b; int kind; };
    std::mutex mu;
    std::vector<Rec> used, idle;
};
namespace {
const char* const kKindNames[MST_K_COUNT] = {"patch_embed", "layernorm", "gemm_qkv", "attention",
                                             "gemm_proj", "gemm_fc1", "gemm_fc2", "cls_probs", "mlp_fused", "block_fused"};
struct ProfScope {
    mst_profiler* p;
    mst_profiler::Rec r{};
    hipStream_t s;
    ProfScope(mst_profiler* prof, int kind, hipStream_t st) : p(prof), s(st) {
        if (!p) return;
        {
            std::lock_guard<std::mutex> lk(p->mu);
            if (!p->idle.empty()) { r = p->idle.back(); p->idle.pop_back(); }
            else { (void)hipEventCreate(&r.a); (void)hipEventCreate(&r.b); }
        }
        r.kind = kind;
        (void)hipEventRecord(r.a, s);
    }
    ~ProfScope() {
        if (!p) return;
        (void)hipEventRecord(r.b, s);
        std::lock_guard<std::mutex> lk(p->mu);
        p->used.push_back(r);
    }
};
}  // namespace

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline size_t dt_size(int dt) { return dt == MST_F32 ? 4 : 2; }

// mst_gemm on a record: the null check the encoder's call sites rely on, then the exact-fp32 or the 16-bit kernels
static int gemm(const gemm_args& g) {
    MST_CHECK_ARG(g.A && g.W && g.C, "gemm: null pointer");
    if (g.dt == MST_F32) {
        MST_CHECK_ARG(g.cdt == MST_F32, "gemm: f32 operands need f32 C");
        return launch_gemm32(g);
    }
    return launch_gemm16(g);
}

extern "C" {

int mst_version(void) { return 300; }
const char* mst_last_error(void) { return g_err; }

int mst_layernorm(const float* x, int64_t x_stride, const float* gamma, const float* beta, void* out,
                  int out_dtype, int64_t out_stride, int64_t rows, int cols, float eps, mst_stream_t stream) {
    MST_CHECK_ARG(x && out && ((gamma != nullptr) == (beta != nullptr)), "layernorm: null pointer");
    return launch_layernorm(x, x_stride, gamma, beta, out, out_dtype, out_stride, rows, cols, eps, (hipStream_t)stream);
}

int mst_gemm(const void* A, int ab_dtype, int64_t lda, const void* W, int64_t ldw, const float* bias, void* C,
             int c_dtype, int64_t ldc, int64_t M, int N, int K, int epilogue, const float* gamma,
             float col_scale, int scale_cols, mst_stream_t stream) {
    return gemm({A, ab_dtype, lda, W, ldw, bias, C, c_dtype, ldc, M, N, K, epilogue, gamma, col_scale, scale_cols, (hipStream_t)stream});
}

int mst_quantize_fp8(const void* x, int dtype, int64_t n, float* amax, void* out8, mst_stream_t stream) {
    MST_CHECK_ARG(x && amax && out8, "quantize_fp8: null pointer");
    return launch_quant8(x, dtype, n, amax, out8, 1, (hipStream_t)stream);
}

int mst_gemm_fp8(const void* A8, int64_t lda, const void* W8, int64_t ldw, const float* bias, const float* a_amax,
                 float w_scale, void* C, int c_dtype, int64_t ldc, int64_t M, int N, int K, int epilogue,
                 const float* gamma, float col_scale, int scale_cols, const float* c_amax, mst_stream_t stream) {
    return launch_gemm8({A8, MST_F8E4M3, lda, W8, ldw, bias, C, c_dtype, ldc, M, N, K, epilogue, gamma, col_scale, scale_cols, (hipStream_t)stream,
                         a_amax, w_scale, nullptr, c_dtype == MST_F8E4M3 ? c_amax : nullptr});
}

int mst_layernorm_fp8(const float* x, int64_t x_stride, const float* gamma, const float* beta, void* out8,
                      int64_t out_stride, int64_t rows, int cols, float eps, const float* amax, mst_stream_t stream) {
    return launch_layernorm_f8(x, x_stride, gamma, beta, out8, out_stride, rows, cols, eps, amax, (hipStream_t)stream);
}

int mst_attention(const void* qkv, int dtype, int n_seq, int N, int heads, int head_dim, void* out,
                  mst_stream_t stream) {
    MST_CHECK_ARG(qkv && out, "attention: null pointer");
    MST_CHECK_ARG(head_dim == 64, "attention: head_dim=%d unsupported (64)", head_dim);
    if (dtype == MST_F32) return launch_attn32((const float*)qkv, n_seq, N, heads, (float*)out, (hipStream_t)stream);
    return launch_attn16(qkv, dtype, n_seq, N, heads, out, 0, (hipStream_t)stream);
}

int mst_attention_cls_probs(const void* qkv, int dtype, int n_seq, int N, int heads, int head_dim, float* probs,
                            mst_stream_t stream) {
    MST_CHECK_ARG(qkv && probs, "cls_probs: null pointer");
    return launch_cls_probs(qkv, dtype, n_seq, N, heads, head_dim, probs, 0, (hipStream_t)stream);
}

int mst_attention_probs_full(const void* qkv, int dtype, int n_seq, int N, int heads, int head_dim, float* probs,
                             mst_stream_t stream) {
    MST_CHECK_ARG(qkv && probs, "probs_full: null pointer");
    return launch_probs_full(qkv, dtype, n_seq, N, heads, head_dim, probs, 0, (hipStream_t)stream);
}

// ---- the kernels and kernel modes that only mst_vit_encode's fused 16-bit pipeline launches, one entry point each: thin forwards to
// the launchers the encoder calls, so that each can be checked on its own at small shapes (tests/test_encoder_seam_gpu.py)
int mst_attention_ex(const void* qkv, int dtype, int n_seq, int N, int heads, int head_dim, void* out, int flags, mst_stream_t stream) {
    MST_CHECK_ARG(qkv && out, "attention_ex: null pointer");
    MST_CHECK_ARG(head_dim == 64, "attention_ex: head_dim=%d unsupported (64)", head_dim);
    MST_CHECK_ARG(dtype == MST_BF16 || dtype == MST_F16, "attention_ex: dtype %d (the log2-domain and blocked forms are 16-bit only)", dtype);
    MST_CHECK_ARG((flags & ~(MST_ATTN_LOG2Q | MST_ATTN_OUT_BLOCKED)) == 0, "attention_ex: unknown flags %d", flags);
    return launch_attn16(qkv, dtype, n_seq, N, heads, out, (flags & MST_ATTN_LOG2Q) ? 1 : 0, (hipStream_t)stream,
                         (flags & MST_ATTN_OUT_BLOCKED) ? 1 : 0);
}

int mst_attention_cls(const void* qkv, int dtype, int n_seq, int N, int heads, void* out, float* probs, int log2q, mst_stream_t stream) {
    MST_CHECK_ARG(qkv && out, "attention_cls: null pointer");
    MST_CHECK_ARG(heads > 0, "attention_cls: heads=%d", heads);
    MST_CHECK_ARG(dtype == MST_F32 || dtype == MST_BF16 || dtype == MST_F16, "attention_cls: bad dtype %d", dtype);
    return launch_cls_attn(qkv, dtype, n_seq, N, heads, probs, out, log2q ? 1 : 0, (hipStream_t)stream);
}

int mst_gemm16_blocked(const void* A_blocked, int dtype, const void* W, int64_t ldw, const float* bias, void* C, int64_t ldc, int64_t M,
                       int N, float col_scale, int scale_cols, mst_stream_t stream) {
    MST_CHECK_ARG(A_blocked && W && C, "gemm16_blocked: null pointer");
    MST_CHECK_ARG(dtype == MST_BF16 || dtype == MST_F16, "gemm16_blocked: bad operand dtype %d", dtype);
    const int K = GEMM16_WREG_TILE.bk;
    gemm_args g{A_blocked, dtype, K, W, ldw, bias, C, dtype, ldc, M, N, K};
    g.col_scale = col_scale, g.scale_cols = scale_cols, g.s = (hipStream_t)stream;
    MST_CHECK_ARG(ldw % 8 == 0 && ldc % 8 == 0 && ((uintptr_t)A_blocked & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)C & 15) == 0,
                  "gemm16_blocked: ldw / ldc must be multiples of 8 and A, W, C 16-byte aligned");
    MST_CHECK_ARG(N > 0 && gemm16_wreg_applicable(g),
                  "gemm16_blocked: M=%lld N=%d scale_cols=%d is no shape of the weights-in-registers kernel, the only one that reads blocked rows",
                  (long long)M, N, scale_cols);
    return launch_gemm16_wreg(g, 1);
}

int mst_patch_rows16(const void* vol, int in_dtype, int n, int H, int W, const void* wp, int dtype, const float* bias, const float* prefix,
                     int n_prefix, const float* pos_patch, float* x, void* xn, mst_stream_t stream) {
    MST_CHECK_ARG(vol && wp && bias && prefix && pos_patch && x && xn, "patch_rows16: null pointer");
    return launch_patch_rows16(vol, in_dtype, n, H, W, wp, dtype, bias, prefix, n_prefix, pos_patch, x, xn, (hipStream_t)stream);
}

size_t mst_attention_train_bwd_workspace_bytes(int n_seq, int N, int heads, int head_dim) {
    return head_dim == 64 ? attn_train_workspace_bytes(n_seq, N, heads) : 0;
}

int mst_attention_train_fwd(const void* qkv16, int dtype, int n_seq, int N, int heads, int head_dim, float* out, float* lse,
                            mst_stream_t stream) {
    MST_CHECK_ARG(qkv16 && out && lse, "attention_train_fwd: null pointer");
    MST_CHECK_ARG(head_dim == 64, "attention_train_fwd: head_dim=%d unsupported (64)", head_dim);
    return launch_attn_train_fwd(qkv16, dtype, n_seq, N, heads, out, 0, lse, (hipStream_t)stream);
}

int mst_attention_train_fwd16(const void* qkv16, int dtype, int n_seq, int N, int heads, int head_dim, void* out16, float* lse,
                              mst_stream_t stream) {
    MST_CHECK_ARG(qkv16 && out16 && lse, "attention_train_fwd16: null pointer");
    MST_CHECK_ARG(head_dim == 64, "attention_train_fwd16: head_dim=%d unsupported (64)", head_dim);
    return launch_attn_train_fwd(qkv16, dtype, n_seq, N, heads, out16, 1, lse, (hipStream_t)stream);
}

int mst_attention_train_bwd(const void* qkv16, int dtype, const float* out, const float* dout, const float* lse, int n_seq, int N,
                            int heads, int head_dim, float dq_scale, float* dqkv, void* workspace, size_t workspace_bytes,
                            mst_stream_t stream) {
    MST_CHECK_ARG(qkv16 && out && dout && lse && dqkv, "attention_train_bwd: null pointer");
    MST_CHECK_ARG(head_dim == 64, "attention_train_bwd: head_dim=%d unsupported (64)", head_dim);
    return launch_attn_train_bwd(qkv16, dtype, out, 0, dout, lse, n_seq, N, heads, dq_scale, dqkv, workspace, workspace_bytes,
                                 (hipStream_t)stream);
}

int mst_attention_train_bwd16(const void* qkv16, int dtype, const void* out16, const float* dout, const float* lse, int n_seq, int N,
                              int heads, int head_dim, float dq_scale, float* dqkv, void* workspace, size_t workspace_bytes,
                              mst_stream_t stream) {
    MST_CHECK_ARG(qkv16 && out16 && dout && lse && dqkv, "attention_train_bwd16: null pointer");
    MST_CHECK_ARG(head_dim == 64, "attention_train_bwd16: head_dim=%d unsupported (64)", head_dim);
    return launch_attn_train_bwd(qkv16, dtype, out16, 1, dout, lse, n_seq, N, heads, dq_scale, dqkv, workspace, workspace_bytes,
                                 (hipStream_t)stream);
}

int mst_pos_embed_interp(const float* pos_patch, int M, int E, int gh, int gw, double offset, int antialias, float* out,
                         mst_stream_t stream) {
    MST_CHECK_ARG(pos_patch && out, "pos_embed_interp: null pointer");
    return launch_pos_interp(pos_patch, M, E, gh, gw, offset, antialias, out, (hipStream_t)stream);
}

int mst_patch_embed(const void* vol, int in_dtype, int n, int H, int W, const void* wp, int dtype, const float* bias,
                    const float* prefix, int n_prefix, const float* pos_patch, int E, float* x, mst_stream_t stream) {
    MST_CHECK_ARG(vol && wp && bias && prefix && pos_patch && x, "patch_embed: null pointer");
    return launch_patch_embed(vol, in_dtype, n, H, W, wp, dtype, bias, prefix, n_prefix, pos_patch, E, x,
                              (hipStream_t)stream);
}

int mst_mlp_fused(float* x, void* xn_out, int dtype, const void* wpack, const float* b1f, const float* b2f,
                  int64_t M, int E, float eps, mst_stream_t stream) {
    MST_CHECK_ARG(x && wpack && b1f && b2f, "mlp_fused: null pointer");
    return launch_mlp16(x, xn_out, dtype, wpack, b1f, b2f, M, E, eps, (hipStream_t)stream);
}

// ---- training step: per-op entry points (the backward is orchestrated by mst/train.py) ---------------------------------
int mst_gemm_ex(const float* A, const float* B, float* C, int M, int N, int K, const int64_t* st, int nb1, int nb2, float alpha,
                float beta, mst_stream_t stream) {
    MST_CHECK_ARG(st, "gemm_ex: null strides");
    return launch_gemm_ex(A, B, C, M, N, K, st[0], st[1], st[2], st[3], st[4], st[5], nb1, nb2, st[6], st[7], st[8], st[9], st[10],
                          st[11], alpha, beta, (hipStream_t)stream);
}
int mst_cvt16(const float* x, int64_t ldx, int64_t rows, int cols, float scale, void* out, int out_dtype, int64_t ldo, int transpose,
              int64_t rows_pad, mst_stream_t stream) {
    return launch_cvt16(x, ldx, rows, cols, scale, out, out_dtype, ldo, transpose, rows_pad, (hipStream_t)stream);
}
int mst_gemm16_splitk(const void* A, int ab_dtype, int64_t lda, const void* W, int64_t ldw, float* Cpart, int64_t ldc, int64_t M, int N, int K,
                      int splits, int64_t split_stride, mst_stream_t stream) {
    gemm_args g{A, ab_dtype, lda, W, ldw, nullptr, Cpart, MST_F32, ldc, M, N, K};
    g.s = (hipStream_t)stream;
    return launch_gemm16_splitk(g, splits, split_stride);
}
int mst_softmax_rows(float* S, const uint8_t* mask, int64_t rows, int L, int rows_per_batch, mst_stream_t stream) {
    MST_CHECK_ARG(S && rows > 0 && L > 0 && rows_per_batch > 0, "softmax_rows: bad arguments");
    return launch_softmax_rows(S, mask, rows, L, rows_per_batch, (hipStream_t)stream);
}
int mst_softmax_rows_bwd(const float* P, float* dP, int64_t rows, int L, float scale, mst_stream_t stream) {
    MST_CHECK_ARG(P && dP && rows > 0 && L > 0, "softmax_rows_bwd: bad arguments");
    return launch_softmax_rows_bwd(P, dP, rows, L, scale, (hipStream_t)stream);
}
int mst_layernorm_bwd(const float* x, int64_t x_stride, const float* gamma, const float* dy, int64_t dy_stride, const float* dres,
                      int64_t dres_stride, float* dx, int64_t dx_stride, float* dgamma, float* dbeta, int64_t rows, int cols,
                      float eps, mst_stream_t stream) {
    MST_CHECK_ARG(x && dy && rows > 0, "layernorm_bwd: bad arguments");
    return launch_layernorm_bwd(x, x_stride, gamma, dy, dy_stride, dres, dres_stride, dx, dx_stride, dgamma, dbeta, rows, cols, eps,
                                (hipStream_t)stream);
}
int mst_act_fwd(const float* h, float* y, int64_t n, int kind, mst_stream_t stream) {
    MST_CHECK_ARG(h && y && n > 0 && (kind == 0 || kind == 1), "act_fwd: bad arguments");
    return launch_act_fwd(h, y, n, kind, (hipStream_t)stream);
}
int mst_act_bwd(const float* h, float* dy, int64_t n, int kind, mst_stream_t stream) {
    MST_CHECK_ARG(h && dy && n > 0 && (kind == 0 || kind == 1), "act_bwd: bad arguments");
    return launch_act_bwd(h, dy, n, kind, (hipStream_t)stream);
}
int mst_swiglu_fwd(const float* x12, float* h, int64_t rows, int hidden, mst_stream_t stream) {
    MST_CHECK_ARG(x12 && h && rows > 0 && hidden > 0, "swiglu_fwd: bad arguments");
    return launch_swiglu_fwd(x12, h, rows, hidden, (hipStream_t)stream);
}
int mst_swiglu_bwd(const float* x12, const float* dh, float* dx12, int64_t rows, int hidden, mst_stream_t stream) {
    MST_CHECK_ARG(x12 && dh && dx12 && rows > 0 && hidden > 0, "swiglu_bwd: bad arguments");
    return launch_swiglu_bwd(x12, dh, dx12, rows, hidden, (hipStream_t)stream);
}
// ---- 16-bit storage mode of the training step (k_train16.hip; act / swiglu in k_train.hip, the column sums in k_colsum.hip)
int mst_residual_layernorm16(const float* x_in, const void* br, int dtype, const float* gamma, float* x_out, const float* ln_w,
                             const float* ln_b, void* y, int64_t rows, int cols, float eps, mst_stream_t stream) {
    MST_CHECK_ARG(x_in && br && x_out && (!y || (ln_w && ln_b)), "residual_layernorm16: null pointer");
    return launch_residual_layernorm16(x_in, br, dtype, gamma, x_out, ln_w, ln_b, y, rows, cols, eps, (hipStream_t)stream);
}
int mst_act_fwd16(const void* h, void* y, int dtype, int64_t n, int kind, mst_stream_t stream) {
    MST_CHECK_ARG(h && y && n > 0 && (kind == 0 || kind == 1), "act_fwd16: bad arguments");
    return launch_act_fwd16(h, y, dtype, n, kind, (hipStream_t)stream);
}
int mst_act_bwd16(const void* h, int dtype, float* dy, int64_t n, int kind, mst_stream_t stream) {
    MST_CHECK_ARG(h && dy && n > 0 && (kind == 0 || kind == 1), "act_bwd16: bad arguments");
    return launch_act_bwd16(h, dtype, dy, n, kind, (hipStream_t)stream);
}
int mst_swiglu_fwd16(const void* x12, void* h, int dtype, int64_t rows, int hidden, mst_stream_t stream) {
    MST_CHECK_ARG(x12 && h && rows > 0 && hidden > 0, "swiglu_fwd16: bad arguments");
    return launch_swiglu_fwd16(x12, h, dtype, rows, hidden, (hipStream_t)stream);
}
int mst_swiglu_bwd16(const void* x12, int dtype, const float* dh, float* dx12, int64_t rows, int hidden, mst_stream_t stream) {
    MST_CHECK_ARG(x12 && dh && dx12 && rows > 0 && hidden > 0, "swiglu_bwd16: bad arguments");
    return launch_swiglu_bwd16(x12, dtype, dh, dx12, rows, hidden, (hipStream_t)stream);
}
int mst_colsum_b16(const float* a, int64_t a_stride, const void* b, int b_dtype, int64_t b_stride, int64_t rows, int cols, float* out,
                   mst_stream_t stream) {
    MST_CHECK_ARG(a && b && out, "colsum_b16: null pointer");
    return launch_colsum_b16(a, a_stride, b, b_dtype, b_stride, rows, cols, out, (hipStream_t)stream);
}
int mst_colsum_b16_ordered(const float* a, int64_t a_stride, const void* b, int b_dtype, int64_t b_stride, int64_t rows, int cols, float* out,
                           void* workspace, size_t workspace_bytes, mst_stream_t stream) {
    MST_CHECK_ARG(a && b && out, "colsum_b16_ordered: null pointer");
    return launch_colsum_b16_ordered(a, a_stride, b, b_dtype, b_stride, rows, cols, out, workspace, workspace_bytes, (hipStream_t)stream);
}
int mst_transpose16(const void* x, int dtype, int64_t ldx, int64_t rows, int cols, void* out, int64_t ldo, int64_t rows_pad,
                    mst_stream_t stream) {
    return launch_transpose16(x, dtype, ldx, rows, cols, out, ldo, rows_pad, (hipStream_t)stream);
}
int mst_colsum(const float* a, int64_t a_stride, const float* b, int64_t b_stride, int64_t rows, int cols, float* out,
               mst_stream_t stream) {
    MST_CHECK_ARG(a && out && rows > 0 && cols > 0, "colsum: bad arguments");
    return launch_colsum(a, a_stride, b, b_stride, rows, cols, out, (hipStream_t)stream);
}
int mst_axpby_cols(const float* x, int64_t x_stride, const float* g, float alpha, float beta, float* y, int64_t y_stride, int64_t rows,
                   int cols, mst_stream_t stream) {
    MST_CHECK_ARG(x && y && rows > 0 && cols > 0, "axpby_cols: bad arguments");
    return launch_axpby_cols(x, x_stride, g, alpha, beta, y, y_stride, rows, cols, (hipStream_t)stream);
}
int mst_im2col14(const void* vol, int dtype, int n, int H, int W, float* col, mst_stream_t stream) {
    MST_CHECK_ARG(vol && col && n > 0 && H > 0 && W > 0 && H % 14 == 0 && W % 14 == 0, "im2col14: bad arguments");
    return launch_im2col14(vol, dtype, n, H, W, col, (hipStream_t)stream);
}
int mst_pos_embed_interp_bwd(const float* dout, int M, int E, int gh, int gw, double offset, float* dpos, mst_stream_t stream) {
    MST_CHECK_ARG(dout && dpos && M > 0 && E > 0 && gh > 0 && gw > 0, "pos_embed_interp_bwd: bad arguments");
    return launch_pos_interp_bwd(dout, M, E, gh, gw, offset, dpos, (hipStream_t)stream);
}
int mst_patch_embed_dgrad(const float* dx, int tokens_per_image, int first_patch_token, const float* wsum, int n, int H, int W, int E,
                          float* dvol, mst_stream_t stream) {
    MST_CHECK_ARG(dx && wsum && dvol, "patch_embed_dgrad: null pointer");
    return launch_patch_embed_dgrad(dx, tokens_per_image, first_patch_token, wsum, 1, n, H, W, E, dvol, (hipStream_t)stream);
}
int mst_patch_embed_rgb(const float* img, int n, int H, int W, const float* wp, const float* bias, const float* prefix, int n_prefix,
                        const float* pos_patch, int E, float* x, mst_stream_t stream) {
    MST_CHECK_ARG(img && wp && bias && prefix && pos_patch && x, "patch_embed_rgb: null pointer");
    return launch_patch_embed_rgb(img, MST_F32, n, H, W, wp, MST_F32, bias, prefix, n_prefix, pos_patch, E, x, (hipStream_t)stream);
}
int mst_patch_embed_rgb_dgrad(const float* dx, int tokens_per_image, int first_patch_token, const float* wp, int n, int H, int W, int E,
                              float* dimg, mst_stream_t stream) {
    MST_CHECK_ARG(dx && wp && dimg, "patch_embed_rgb_dgrad: null pointer");
    return launch_patch_embed_dgrad(dx, tokens_per_image, first_patch_token, wp, 3, n, H, W, E, dimg, (hipStream_t)stream);
}
int mst_patch_embed_rgb_wgrad(const float* dx, int tokens_per_image, int first_patch_token, const float* img, int n, int H, int W, int E,
                              int rows_per_split, float* part, mst_stream_t stream) {
    MST_CHECK_ARG(dx && img && part, "patch_embed_rgb_wgrad: null pointer");
    return launch_patch_embed_rgb_wgrad(dx, tokens_per_image, first_patch_token, img, n, H, W, E, rows_per_split, part, (hipStream_t)stream);
}

// ---- convolutional backbone of the ResNet models ------------------------------------------------------------
int mst_im2col_nhwc(const float* x, int n, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad, float* col,
                    mst_stream_t stream) {
    MST_CHECK_ARG(x && col && n > 0 && H > 0 && W > 0 && C > 0 && kh > 0 && kw > 0 && stride > 0 && pad >= 0, "im2col_nhwc: bad arguments");
    return launch_im2col_nhwc(x, n, H, W, C, kh, kw, stride, pad, Kpad, col, (hipStream_t)stream);
}
int mst_conv_gemm(const float* x, int n, int H, int W, int Cin, int kh, int kw, int stride, int pad, const float* Wg, const float* bias,
                  float* out, int Cout, int Kpad, int epilogue, const float* gamma, mst_stream_t stream) {
    return launch_conv_gemm32(x, n, H, W, Cin, kh, kw, stride, pad, Wg, Kpad, bias, out, Cout, Cout, Kpad, epilogue, gamma, (hipStream_t)stream);
}
int mst_conv_gemm16(const void* x, int dtype, int n, int H, int W, int Cin, int kh, int kw, int stride, int pad, const void* Wg, const float* bias,
                    void* out, int out_dtype, int Cout, int epilogue, mst_stream_t stream) {
    return launch_conv_gemm16(x, dtype, n, H, W, Cin, kh, kw, stride, pad, Wg, bias, out, out_dtype, Cout, epilogue, (hipStream_t)stream);
}
int mst_conv_dgrad(const void* dz, int dtype, int n, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, const void* Wt, int H, int W,
                   int Cin, float* dx, mst_stream_t stream) {
    if (dtype == MST_F32)
        return launch_conv_dgrad32((const float*)dz, n, Ho, Wo, Cout, kh, kw, stride, pad, (const float*)Wt, H, W, Cin, dx, (hipStream_t)stream);
    return launch_conv_dgrad16(dz, dtype, n, Ho, Wo, Cout, kh, kw, stride, pad, Wt, H, W, Cin, dx, (hipStream_t)stream);
}
// the stem's data gradient (reference resnet.py:176 + torchvision's conv1): the last link of the gradient with respect to the input volume
int mst_conv_dgrad_stem(const void* dz, int dtype, int n, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, const void* Wg, int H,
                        int W, int Cin, float* dx, mst_stream_t stream) {
    return launch_conv_dgrad_stem(dz, dtype, n, Ho, Wo, Cout, kh, kw, stride, pad, Wg, H, W, Cin, dx, (hipStream_t)stream);
}
int mst_conv_wgrad(const float* dz, const float* x, int n, int H, int W, int Cin, int kh, int kw, int stride, int pad, int Cout, float* part,
                   int nsplit, int64_t rows_per_split, mst_stream_t stream) {
    return launch_conv_wgrad32(dz, x, n, H, W, Cin, kh, kw, stride, pad, Cout, part, nsplit, rows_per_split, (hipStream_t)stream);
}
int mst_conv_wgrad16(const void* dz, const void* x, int dtype, int n, int H, int W, int Cin, int kh, int kw, int stride, int pad, int Cout, float* part,
                     int nsplit, int64_t rows_per_split, mst_stream_t stream) {
    return launch_conv_wgrad16(dz, x, dtype, n, H, W, Cin, kh, kw, stride, pad, Cout, part, nsplit, rows_per_split, (hipStream_t)stream);
}
int mst_rope_rows(float* qkv, int64_t rows, int L, int heads, int head_dim, const float* freqs, float sign, mst_stream_t stream) {
    return launch_rope_rows(qkv, rows, L, heads, head_dim, freqs, sign, (hipStream_t)stream);
}
int mst_im2col_nhwc16(const float* x, int n, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad, void* col, int out_dtype,
                      mst_stream_t stream) {
    MST_CHECK_ARG(x && col && n > 0, "im2col16: bad arguments");
    return launch_im2col_nhwc16(x, n, H, W, C, kh, kw, stride, pad, Kpad, col, out_dtype, (hipStream_t)stream);
}
int mst_maxpool_nhwc16(const void* x, int dtype, int n, int H, int W, int C, void* y, mst_stream_t stream) {
    MST_CHECK_ARG(x && y && n > 0 && H > 0 && W > 0 && C > 0, "maxpool16: bad arguments");
    return launch_maxpool_nhwc(x, dtype, n, H, W, C, y, (hipStream_t)stream);
}
int mst_cvt32(const void* x, int dtype, int64_t n, float* out, mst_stream_t stream) { return launch_cvt32(x, dtype, n, out, (hipStream_t)stream); }
int mst_maxpool_nhwc(const float* x, int n, int H, int W, int C, float* y, mst_stream_t stream) {
    MST_CHECK_ARG(x && y && n > 0 && H > 0 && W > 0 && C > 0, "maxpool_nhwc: bad arguments");
    return launch_maxpool_nhwc(x, MST_F32, n, H, W, C, y, (hipStream_t)stream);
}
int mst_avgpool_nhwc(const float* x, int n, int HW, int C, float* y, mst_stream_t stream) {
    MST_CHECK_ARG(x && y && n > 0 && HW > 0 && C > 0, "avgpool_nhwc: bad arguments");
    return launch_avgpool_nhwc(x, MST_F32, n, HW, C, y, (hipStream_t)stream);
}

int mst_col2im_nhwc(const float* dcol, int n, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad, float* dx,
                    mst_stream_t stream) {
    MST_CHECK_ARG(dcol && dx && n > 0 && H > 0 && W > 0 && C > 0, "col2im_nhwc: bad arguments");
    return launch_col2im_nhwc(dcol, n, H, W, C, kh, kw, stride, pad, Kpad, dx, (hipStream_t)stream);
}
int mst_maxpool_bwd_nhwc(const float* x, const float* dy, int n, int H, int W, int C, float* dx, mst_stream_t stream) {
    MST_CHECK_ARG(x && dy && dx && n > 0, "maxpool_bwd_nhwc: bad arguments");
    return launch_maxpool_bwd_nhwc(x, dy, n, H, W, C, dx, (hipStream_t)stream);
}
// ---- fixed-order forms (torch.use_deterministic_algorithms): no floating-point atomics, bit-reproducible for fixed shapes -----------
// (the BatchNorm and pooling entry points, of every mode, are in k_bn.hip)
size_t mst_colsum_ordered_workspace_bytes(int64_t rows, int cols) { return colsum_ordered_workspace_bytes(rows, cols, 1); }
int mst_colsum_ordered(const float* a, int64_t a_stride, const float* b, int64_t b_stride, int64_t rows, int cols, float* out,
                       void* workspace, size_t workspace_bytes, mst_stream_t stream) {
    MST_CHECK_ARG(a && out && rows > 0 && cols > 0, "colsum_ordered: bad arguments");
    return launch_colsum_ordered(a, a_stride, b, b_stride, rows, cols, out, workspace, workspace_bytes, (hipStream_t)stream);
}
size_t mst_layernorm_bwd_ordered_workspace_bytes(int64_t rows, int cols) { return layernorm_bwd_ordered_workspace_bytes(rows, cols); }
int mst_layernorm_bwd_ordered(const float* x, int64_t x_stride, const float* gamma, const float* dy, int64_t dy_stride, const float* dres,
                              int64_t dres_stride, float* dx, int64_t dx_stride, float* dgamma, float* dbeta, int64_t rows, int cols,
                              float eps, void* workspace, size_t workspace_bytes, mst_stream_t stream) {
    MST_CHECK_ARG(x && dy && rows > 0, "layernorm_bwd_ordered: bad arguments");
    return launch_layernorm_bwd_ordered(x, x_stride, gamma, dy, dy_stride, dres, dres_stride, dx, dx_stride, dgamma, dbeta, rows, cols, eps,
                                        workspace, workspace_bytes, (hipStream_t)stream);
}
int mst_col2im_nhwc_gather(const float* dcol, int n, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad, float* dx,
                           mst_stream_t stream) {
    MST_CHECK_ARG(dcol && dx && n > 0 && H > 0 && W > 0 && C > 0, "col2im_nhwc_gather: bad arguments");
    return launch_col2im_gather(dcol, n, H, W, C, kh, kw, stride, pad, Kpad, dx, (hipStream_t)stream);
}
size_t mst_maxpool_bwd_nhwc_gather_workspace_bytes(int n, int H, int W, int C) { return maxpool_bwd_gather_workspace_bytes(n, H, W, C); }
int mst_maxpool_bwd_nhwc_gather(const float* x, const float* dy, int n, int H, int W, int C, float* dx, void* workspace, size_t workspace_bytes,
                                mst_stream_t stream) {
    MST_CHECK_ARG(x && dy && dx && n > 0 && H > 0 && W > 0 && C > 0, "maxpool_bwd_nhwc_gather: bad arguments");
    return launch_maxpool_bwd_gather("maxpool_bwd_gather", x, MST_F32, dy, n, H, W, C, dx, workspace, workspace_bytes, (hipStream_t)stream);
}
size_t mst_pos_embed_interp_bwd_ordered_workspace_bytes(int M, int E, int gh, int gw) { return pos_interp_bwd_ordered_workspace_bytes(M, E, gh, gw); }
int mst_pos_embed_interp_bwd_ordered(const float* dout, int M, int E, int gh, int gw, double offset, float* dpos, void* workspace,
                                     size_t workspace_bytes, mst_stream_t stream) {
    MST_CHECK_ARG(dout && dpos && M > 0 && E > 0 && gh > 0 && gw > 0, "pos_embed_interp_bwd_ordered: bad arguments");
    return launch_pos_interp_bwd_ordered(dout, M, E, gh, gw, offset, dpos, workspace, workspace_bytes, (hipStream_t)stream);
}
size_t mst_znorm_ordered_workspace_bytes(int64_t n) { return znorm_ordered_workspace_bytes(n); }
int mst_znorm_ordered(const float* x, int64_t n, float q_lo, float q_hi, float* y, void* state, void* workspace, size_t workspace_bytes,
                      mst_stream_t stream) {
    MST_CHECK_ARG(x && y && state && n > 0 && q_lo >= 0.f && q_lo <= q_hi && q_hi <= 1.f, "znorm_ordered: bad arguments");
    return launch_znorm_ordered(x, n, q_lo, q_hi, y, state, workspace, workspace_bytes, (hipStream_t)stream);
}
int mst_avgpool_bwd_nhwc(const float* dy, int n, int HW, int C, float* dx, mst_stream_t stream) {
    MST_CHECK_ARG(dy && dx && n > 0 && HW > 0 && C > 0, "avgpool_bwd_nhwc: bad arguments");
    return launch_avgpool_bwd_nhwc(dy, n, HW, C, dx, (hipStream_t)stream);
}

int mst_gradcampp(const float* act, const float* out, int O, const float* W, int n, int HW, int C, float* cam, float* state,
                  mst_stream_t stream) {
    MST_CHECK_ARG(act && out && cam && state && n > 0 && HW > 0 && C > 0 && C <= 8192 && O > 0 && (W || O == C), "gradcampp: bad arguments");
    return launch_gradcampp(act, out, O, W, n, HW, C, cam, state, (hipStream_t)stream);
}

// ---- input pipeline ------------------------------------------------------------------------------------
// crop begins cb[a] in 0..excess and leading pads pb[a] in 0..total pad, per axis (an axis is either cropped or padded, the other is 0)
static int crop_or_pad_at(const float* src, const int sn[3], float* dst, const int tn[3], const int cb[3], const int pb[3], int pad_minimum,
                          float pad_value, void* ws, size_t ws_bytes, hipStream_t s) {
    const int s0 = sn[0], s1 = sn[1], s2 = sn[2], t0 = tn[0], t1 = tn[1], t2 = tn[2];
    int pad_lo[3], crop_lo[3], pn[3];
    bool any_pad = false;
    for (int a = 0; a < 3; ++a) {
        const int d = tn[a] - sn[a];
        const int p = d > 0 ? d : 0, c = d < 0 ? -d : 0;
        MST_CHECK_ARG(cb[a] >= 0 && cb[a] <= c && pb[a] >= 0 && pb[a] <= p, "crop_or_pad: axis %d: crop begin %d not in 0..%d or pad begin %d not in 0..%d",
                      a, cb[a], c, pb[a], p);
        pad_lo[a] = pb[a];
        crop_lo[a] = cb[a];
        pn[a] = sn[a] + p;
        any_pad = any_pad || p > 0;
    }
    if (!any_pad)                                        // crop only
        return launch_copy_block(src, s1, s2, crop_lo[0], crop_lo[1], crop_lo[2], dst, t1, t2, 0, 0, 0, t0, t1, t2, s);
    const bool direct = pn[0] == t0 && pn[1] == t1 && pn[2] == t2;    // pad only: build the padded array in dst itself
    const size_t need = direct ? 0 : sizeof(float) * (size_t)pn[0] * pn[1] * pn[2];
    MST_CHECK_ARG(direct || (ws && ws_bytes >= need), "crop_or_pad: workspace %zu < %zu bytes", ws_bytes, need);
    float* pad = direct ? dst : (float*)ws;
    int rc = launch_copy_block(src, s1, s2, 0, 0, 0, pad, pn[1], pn[2], pad_lo[0], pad_lo[1], pad_lo[2], s0, s1, s2, s);
    if (rc) return rc;
    // numpy.pad: one axis after the other; axis a sees the pads of the axes before it and only the valid part of the later ones
    const int lo0 = pad_lo[0], hi0 = pad_lo[0] + s0, lo1 = pad_lo[1], hi1 = pad_lo[1] + s1, lo2 = pad_lo[2], hi2 = pad_lo[2] + s2;
    if (pn[0] > s0 && (rc = launch_pad_axis(pad, pn[0], pn[1], pn[2], 0, lo0, hi0, lo1, hi1, lo2, hi2, !pad_minimum, pad_value, s))) return rc;
    if (pn[1] > s1 && (rc = launch_pad_axis(pad, pn[0], pn[1], pn[2], 1, lo1, hi1, 0, pn[0], lo2, hi2, !pad_minimum, pad_value, s))) return rc;
    if (pn[2] > s2 && (rc = launch_pad_axis(pad, pn[0], pn[1], pn[2], 2, lo2, hi2, 0, pn[0], 0, pn[1], !pad_minimum, pad_value, s))) return rc;
    if (direct) return MST_OK;
    return launch_copy_block(pad, pn[1], pn[2], crop_lo[0], crop_lo[1], crop_lo[2], dst, t1, t2, 0, 0, 0, t0, t1, t2, s);
}

int mst_crop_or_pad(const float* src, int s0, int s1, int s2, float* dst, int t0, int t1, int t2, int pad_minimum,
                    float pad_value, void* ws, size_t ws_bytes, mst_stream_t stream) {
    MST_CHECK_ARG(src && dst && s0 > 0 && s1 > 0 && s2 > 0 && t0 > 0 && t1 > 0 && t2 > 0, "crop_or_pad: bad arguments");
    const int sn[3] = {s0, s1, s2}, tn[3] = {t0, t1, t2};
    int cb[3], pb[3];
    for (int a = 0; a < 3; ++a) {                       // augmentations_3d.py:164-172: ini = ceil(n / 2), fin = n - ini
        const int d = tn[a] - sn[a];
        pb[a] = d > 0 ? (d + 1) / 2 : 0;
        cb[a] = d < 0 ? (-d + 1) / 2 : 0;
    }
    return crop_or_pad_at(src, sn, dst, tn, cb, pb, pad_minimum, pad_value, ws, ws_bytes, (hipStream_t)stream);
}

int mst_crop_or_pad_at(const float* src, int s0, int s1, int s2, float* dst, int t0, int t1, int t2, int crop0, int crop1, int crop2,
                       int pad0, int pad1, int pad2, int pad_minimum, float pad_value, void* ws, size_t ws_bytes, mst_stream_t stream) {
    MST_CHECK_ARG(src && dst && s0 > 0 && s1 > 0 && s2 > 0 && t0 > 0 && t1 > 0 && t2 > 0, "crop_or_pad_at: bad arguments");
    const int sn[3] = {s0, s1, s2}, tn[3] = {t0, t1, t2}, cb[3] = {crop0, crop1, crop2}, pb[3] = {pad0, pad1, pad2};
    return crop_or_pad_at(src, sn, dst, tn, cb, pb, pad_minimum, pad_value, ws, ws_bytes, (hipStream_t)stream);
}

// ---- training augmentation (k_augment.hip) -----------------------------------------------------------------------------
static bool aug_dtype(int dt) { return dt == MST_F32 || dt == MST_F16 || dt == MST_BF16; }

int mst_augment_volumes(const void* in, int in_dtype, void* out, int out_dtype, int n, int D, int H, int W, const float* params,
                        uint64_t seed, uint64_t counter, mst_stream_t stream) {
    MST_CHECK_ARG(in && out && params && in != out && n > 0 && D > 0 && H > 0 && W > 0, "augment_volumes: bad arguments (the kernel gathers: not in place)");
    MST_CHECK_ARG(aug_dtype(in_dtype) && aug_dtype(out_dtype), "augment_volumes: bad dtype %d -> %d", in_dtype, out_dtype);
    MST_CHECK_ARG(n <= 65535 && (int64_t)D * H * W <= 0x7ffffff0ll, "augment_volumes: n=%d volumes of %d x %d x %d (at most 65535 volumes of < 2^31 voxels)",
                  n, D, H, W);
    return launch_augment_volumes(in, in_dtype, out, out_dtype, n, D, H, W, params, seed, counter, (hipStream_t)stream);
}

int mst_volume_min(const void* x, int dtype, int n, int64_t elems, float* out, int out_stride, mst_stream_t stream) {
    MST_CHECK_ARG(x && out && n > 0 && n <= 65535 && elems > 0 && out_stride > 0, "volume_min: bad arguments");
    MST_CHECK_ARG(aug_dtype(dtype), "volume_min: bad dtype %d", dtype);
    return launch_volume_min(x, dtype, n, elems, out, out_stride, (hipStream_t)stream);
}

size_t mst_znorm_state_bytes(void) { return znorm_state_bytes(); }

int mst_znorm(const float* x, int64_t n, float q_lo, float q_hi, float* y, void* state, mst_stream_t stream) {
    MST_CHECK_ARG(x && y && state && n > 0 && q_lo >= 0.f && q_lo <= q_hi && q_hi <= 1.f, "znorm: bad arguments");
    return launch_znorm(x, n, q_lo, q_hi, y, state, (hipStream_t)stream);
}

int mst_slices2rgb(const void* vol, int dtype, int B, int D, int H, int W, void* out, mst_stream_t stream) {
    MST_CHECK_ARG(vol && out && B > 0 && D > 0 && H > 0 && W > 0, "slices2rgb: bad arguments");
    MST_CHECK_ARG(dtype == MST_F32 || dtype == MST_F16 || dtype == MST_BF16, "slices2rgb: bad dtype %d", dtype);
    return launch_slices2rgb(vol, dtype, B, D, H, W, out, (hipStream_t)stream);
}

size_t mst_block_fused_scratch_bytes(void) { return block16_scratch_bytes(); }

int mst_block_fused(float* x, const void* attn_out, void* xn_out, int dtype, const void* proj_pack, const float* proj_bf,
                    const void* wpack, const float* b1f, const float* b2f, void* scratch, size_t scratch_bytes, int64_t M,
                    int E, float eps, mst_stream_t stream) {
    MST_CHECK_ARG(x && attn_out && proj_pack && proj_bf && wpack && b1f && b2f && scratch, "block_fused: null pointer");
    MST_CHECK_ARG(scratch_bytes >= block16_scratch_bytes(), "block_fused: scratch %zu < %zu bytes", scratch_bytes, block16_scratch_bytes());
    return launch_block16(x, attn_out, xn_out, dtype, proj_pack, proj_bf, wpack, b1f, b2f, scratch, M, E, eps, (hipStream_t)stream);
}

int mst_block_fused_s(float* x, const void* attn_out, void* xn_out, int dtype, const void* block_seq, const float* b1f,
                      const float* proj_bf, const float* b2f, int64_t M, int E, float eps, int layout, mst_stream_t stream) {
    MST_CHECK_ARG(x && attn_out && block_seq && b1f && proj_bf && b2f, "block_fused_s: null pointer");
    MST_CHECK_ARG(layout >= 0 && layout < 8, "block_fused_s: layout=%d", layout);
    return launch_block16s(x, attn_out, xn_out, dtype, block_seq, b1f, proj_bf, b2f, M, E, eps, layout, (hipStream_t)stream);
}

// ---- per-slice encoder ----------------------------------------------------------------------
// workspace carve (chunk of C slices, Mc = C*N rows):
//   x   fp32 [Mc, E]      residual stream
//   xn  T    [Mc, E]      LayerNorm output; reused as the attention output
//   big T    [Mc, 4E]     qkv [Mc, 3E] during attention, then the MLP hidden [Mc, 4E] (SwiGLU: [Mc, ffn_hidden], ffn_hidden <= 4E)
//   fp8_linear only:  a8 u8 [Mc, 4E] (the quantised input of the current GEMM) | amax f32 [depth][4]
static void vit_carve(const mst_vit_weights* w, int N, int chunk, size_t* off_xn, size_t* off_big, size_t* total,
                      size_t* off_a8 = nullptr, size_t* off_amax = nullptr, size_t* off_blk = nullptr) {
    // rows rounded up to whole 32-row groups: the blocked / image layouts between two single-role block launches address groups
    const size_t Mc = ((size_t)chunk * N + 31) / 32 * 32, E = (size_t)w->embed_dim, ts = dt_size(w->compute_dtype);
    size_t o = 0;
    o += align_up(Mc * E * 4, 256);
    *off_xn = o;
    o += align_up(Mc * E * ts, 256);
    *off_big = o;
    o += align_up(Mc * 4 * E * ts, 256);
    if (w->fp8_linear) {
        if (off_a8) *off_a8 = o;
        o += align_up(Mc * 4 * E, 256);
        if (off_amax) *off_amax = o;
        o += align_up((size_t)w->depth * 4 * sizeof(float), 256);
    }
    if (off_blk) *off_blk = o;
    o += align_up(block16_scratch_bytes(), 256);        // lane-private LayerNorm2 hand-off of the fused block kernel (96 KiB per CU)
    *total = o;
}

size_t mst_vit_workspace_bytes(const mst_vit_weights* w, int H, int W, int chunk_slices) {
    if (!w || H <= 0 || W <= 0 || chunk_slices <= 0) return 0;
    const int N = 1 + w->num_registers + (H / 14) * (W / 14);
    size_t a, b, t;
    vit_carve(w, N, chunk_slices, &a, &b, &t);
    return t;
}

#define RUN(call)              \
    do {                       \
        int rc_ = (call);      \
        if (rc_) return rc_;   \
    } while (0)
#define RUNK(kind, call) RUN([&] { ProfScope ps_(prof, kind, s); return (call); }())   // the launch, timed under `kind` when a profiler is attached

// What a call runs, resolved once from what the encoder can observe: fp8_linear, the compute dtype, embed_dim, the token count of
// the WHOLE call (never of a chunk) and which packed weights the caller filled (include/mst_hip.h, mst_vit_layer).
enum vit_tail {           // a block's work behind attention
    TAIL_UNFUSED,         // out-projection, LayerNorm2, fc1, fc2: one launch each
    TAIL_MLP_FUSED,       // out-projection, then norm2 + MLP in one kernel (k_mlp16.hip)
    TAIL_BLOCK_ROLES,     // out-projection folded into that launch, producer/consumer form (k_block16.hip)
    TAIL_BLOCK_SINGLE,    // the same in the single-role form (k_block16s.hip)
    TAIL_FP8_DYNAMIC,     // e4m3 GEMMs, every input quantised with this chunk's max|x|
    TAIL_FP8_STATIC,      // e4m3 GEMMs with calibrated scales: producers write e4m3, nothing is scanned
    TAIL_SWIGLU           // ffn_kind 1: out-projection, LayerNorm2, w12 with the SwiGLU epilogue, w3 (swiglu_ffn.py:54-72)
};
struct vit_plan {
    vit_tail tail;
    bool fused_ln;        // norm1 folded into the QKV weights: the token kernel and every tail write the next block's plain-normalised rows
    bool may_prune;       // prune_last_block, for chunks of at most 65535 slices
};

static vit_plan vit_resolve(const mst_vit_weights* w, int64_t tokens) {
    if (w->fp8_linear) return {w->fp8_amax ? TAIL_FP8_STATIC : TAIL_FP8_DYNAMIC, false, false};
    const bool may_prune = w->prune_last_block && w->num_heads * 64 == w->embed_dim;
    if (w->ffn_kind == MST_FFN_SWIGLU) return {TAIL_SWIGLU, false, may_prune};
    // fused-LayerNorm pipeline (16-bit, E = 384): norm1 folded into QKV, norm2 + MLP in one kernel.  The fused MLP is a
    // persistent kernel of 128-token tiles: below ~one tile per CU it leaves CUs idle (c1 shape, 4k tokens: 90 us per
    // launch on 33 CUs against ~45 us for LN + fc1 + fc2 as three well-filled launches), so small calls take the unfused path.
    static const int64_t fused_min_tokens = getenv("MST_FUSED_MIN_TOKENS") ? atoll(getenv("MST_FUSED_MIN_TOKENS")) : 12288;   // measured crossover (tools/bench_crossover.py): 8k tokens unfused 1.57 vs 1.92 ms, 16k fused 2.34 vs 2.62
    // Every fused tail needs the folded QKV and the folded MLP biases on every layer; beyond those each needs exactly what it dereferences.
    bool fused = w->compute_dtype != MST_F32 && w->embed_dim == 384 && tokens >= fused_min_tokens, single = true, roles = true, mlp = true;
    for (int l = 0; l < w->depth && fused; ++l) {
        const mst_vit_layer* L = &w->layers[l];
        fused = L->qkv_wf && L->qkv_bf && L->fc1_bf && L->fc2_bf;
        single = single && L->block_seq && L->proj_bf;
        roles = roles && L->mlp_pack && L->proj_pack && L->proj_bf;
        mlp = mlp && L->mlp_pack;
    }
    if (!fused || !(single || roles || mlp)) return {TAIL_UNFUSED, false, may_prune};
    return {single ? TAIL_BLOCK_SINGLE : roles ? TAIL_BLOCK_ROLES : TAIL_MLP_FUSED, true, may_prune};
}

// One encoder call: what every launch needs, and the pieces of a block.  c, Mc and blocked belong to the current chunk.
struct vit_call {
    const mst_vit_weights* w;
    float *x, *amax;
    void *xn, *big, *a8, *blk;   // blk: lane-private hand-off of the producer/consumer block kernel
    int dt, E, heads, N, log2q;
    float qscale;
    mst_profiler* prof;
    hipStream_t s;
    int c;
    int64_t Mc;
    bool blocked;

    // C[rows, n] = epi(A[rows, k] . W[n, k]^T + bias): a linear layer of the compute type on dense rows
    gemm_args linear(int64_t rows, const void* A, const void* W, const float* bias, void* C, int cdt, int n, int k, int epi = MST_EPI_BIAS) const {
        gemm_args g{A, dt, k, W, k, bias, C, cdt, n, rows, n, k};
        g.epi = epi, g.s = s;
        return g;
    }
    // x[rows of pitch ldx] += gamma * (A[rows, k] . W[E, k]^T + bias) on the fp32 residual stream
    gemm_args residual(int64_t rows, const void* A, const void* W, const float* bias, const float* gamma, int k, int64_t ldx) const {
        gemm_args g = linear(rows, A, W, bias, x, MST_F32, E, k, MST_EPI_RESIDUAL);
        g.ldc = ldx, g.gamma = gamma;
        return g;
    }
    // big = A . W^T + bias for this chunk, the q columns scaled for the attention kernels
    gemm_args qkv_linear(const void* A, const void* W, const float* bias) const {
        gemm_args g = linear(Mc, A, W, bias, big, dt, 3 * E, E);
        g.col_scale = qscale, g.scale_cols = E;
        return g;
    }
    // big[rows, Hp] = silu(A . Wg^T + bg) o (A . Wv^T + bv): fc1_w / fc1_b carry the row-paired w12 image of 2 Hp rows (MST_EPI_BIAS_SWIGLU)
    gemm_args swiglu(int64_t rows, const void* A, const mst_vit_layer* L) const {
        gemm_args g = linear(rows, A, L->fc1_w, L->fc1_b, big, dt, 2 * w->ffn_hidden, E, MST_EPI_BIAS_SWIGLU);
        g.ldc = w->ffn_hidden;
        return g;
    }
    // the same layer on e4m3 operands (A and W already quantised) under their per-tensor scales
    static gemm_args fp8(gemm_args g, const float* a_amax, float w_scale) {
        g.dt = MST_F8E4M3, g.a_amax = a_amax, g.w_scale = w_scale;
        return g;
    }

    // big = qkv(norm1 x)                                       block.py:90-91,112
    int qkv(const vit_plan& p, int l) const {
        const mst_vit_layer* L = &w->layers[l];
        if (p.tail == TAIL_FP8_STATIC) {
            const float* am = w->fp8_amax + l * 4;
            RUNK(MST_K_LAYERNORM, launch_layernorm_f8(x, E, L->ln1_w, L->ln1_b, a8, E, Mc, E, 1e-6f, am + 0, s));
            RUNK(MST_K_GEMM_QKV, launch_gemm8(fp8(qkv_linear(a8, L->qkv_w8, L->qkv_b), am + 0, L->w8_scale[0])));
        } else if (p.tail == TAIL_FP8_DYNAMIC) {
            // every linear layer: quantise its input with a fresh per-tensor scale (this chunk's max|x|), e4m3 GEMM.  The
            // [M,E] inputs are scanned (53 us; a running maximum kept by the one-wave-per-row LayerNorm kernel cost 125 us:
            // 350 k waves polling one address serialise in one L2 channel); the 4x larger hidden activation gets its maximum
            // from the fc1 epilogue (one conditional atomic per workgroup)
            float* am = amax + l * 4;
            RUNK(MST_K_LAYERNORM, launch_layernorm(x, E, L->ln1_w, L->ln1_b, xn, dt, E, Mc, E, 1e-6f, s));
            RUN(launch_quant8(xn, dt, Mc * E, am + 0, a8, 1, s));
            RUNK(MST_K_GEMM_QKV, launch_gemm8(fp8(qkv_linear(a8, L->qkv_w8, L->qkv_b), am + 0, L->w8_scale[0])));
        } else if (p.fused_ln && blocked && l > 0) {
            RUNK(MST_K_GEMM_QKV, launch_gemm16_wreg(qkv_linear(xn, L->qkv_wf, L->qkv_bf), 1));
        } else if (p.fused_ln) {
            RUNK(MST_K_GEMM_QKV, gemm(qkv_linear(xn, L->qkv_wf, L->qkv_bf)));
        } else {
            RUNK(MST_K_LAYERNORM, launch_layernorm(x, E, L->ln1_w, L->ln1_b, xn, dt, E, Mc, E, 1e-6f, s));
            RUNK(MST_K_GEMM_QKV, gemm(qkv_linear(xn, L->qkv_w, L->qkv_b)));
        }
        return MST_OK;
    }
    // nothing behind the last block reads a patch token (final norm + head take the CLS rows): attention, out-projection
    // and MLP for the c CLS rows only, on the unfused kernels.  Scratch: xn[0, cE) attention rows, xn[cE, 2cE)
    // LayerNorm2 rows, big (free once K and V are consumed) the hidden rows.
    int pruned_last_block(int l, float* pr) const {
        const mst_vit_layer* L = &w->layers[l];
        char* const a_cls = (char*)xn;
        char* const n_cls = (char*)xn + (size_t)c * E * (dt == MST_F32 ? 4 : 2);
        RUNK(MST_K_ATTENTION, launch_cls_attn(big, dt, c, N, heads, pr, a_cls, log2q, s));
        RUNK(MST_K_GEMM_PROJ, gemm(residual(c, a_cls, L->proj_w, L->proj_b, L->ls1, E, (int64_t)N * E)));
        RUNK(MST_K_LAYERNORM, launch_layernorm(x, (int64_t)N * E, L->ln2_w, L->ln2_b, n_cls, dt, E, c, E, 1e-6f, s));
        if (w->ffn_kind == MST_FFN_SWIGLU) {
            RUNK(MST_K_GEMM_FC1, gemm(swiglu(c, n_cls, L)));
            RUNK(MST_K_GEMM_FC2, gemm(residual(c, big, L->fc2_w, L->fc2_b, L->ls2, w->ffn_hidden, (int64_t)N * E)));
            return MST_OK;
        }
        RUNK(MST_K_GEMM_FC1, gemm(linear(c, n_cls, L->fc1_w, L->fc1_b, big, dt, 4 * E, E, MST_EPI_BIAS_GELU)));
        RUNK(MST_K_GEMM_FC2, gemm(residual(c, big, L->fc2_w, L->fc2_b, L->ls2, 4 * E, (int64_t)N * E)));
        return MST_OK;
    }
    // x += ls1(proj(attn)); x += ls2(fc2(gelu(fc1(norm2 x))))   block.py:91,93-94,113; the fused forms also write xn = normalise(x) for the next block
    int tail(vit_tail t, int l) const {
        const mst_vit_layer* L = &w->layers[l];
        void* const xn_out = (l + 1 < w->depth) ? xn : nullptr;
        switch (t) {
            case TAIL_FP8_STATIC: {   // the e4m3 hidden activation lives in `big` (bytes); fc1 reads a8 and writes big, fc2 reads big
                const float* am = w->fp8_amax + l * 4;
                RUN(launch_quant8_static(xn, dt, Mc * E, am + 1, a8, s));
                RUNK(MST_K_GEMM_PROJ, launch_gemm8(fp8(residual(Mc, a8, L->proj_w8, L->proj_b, L->ls1, E, E), am + 1, L->w8_scale[1])));
                RUNK(MST_K_LAYERNORM, launch_layernorm_f8(x, E, L->ln2_w, L->ln2_b, a8, E, Mc, E, 1e-6f, am + 2, s));
                gemm_args fc1 = fp8(linear(Mc, a8, L->fc1_w8, L->fc1_b, big, MST_F8E4M3, 4 * E, E, MST_EPI_BIAS_GELU), am + 2, L->w8_scale[2]);
                fc1.c_amax = am + 3;
                RUNK(MST_K_GEMM_FC1, launch_gemm8(fc1));
                RUNK(MST_K_GEMM_FC2, launch_gemm8(fp8(residual(Mc, big, L->fc2_w8, L->fc2_b, L->ls2, 4 * E, E), am + 3, L->w8_scale[3])));
                return MST_OK;
            }
            case TAIL_FP8_DYNAMIC: {
                float* am = amax + l * 4;
                RUN(launch_quant8(xn, dt, Mc * E, am + 1, a8, 1, s));
                RUNK(MST_K_GEMM_PROJ, launch_gemm8(fp8(residual(Mc, a8, L->proj_w8, L->proj_b, L->ls1, E, E), am + 1, L->w8_scale[1])));
                RUNK(MST_K_LAYERNORM, launch_layernorm(x, E, L->ln2_w, L->ln2_b, xn, dt, E, Mc, E, 1e-6f, s));
                RUN(launch_quant8(xn, dt, Mc * E, am + 2, a8, 1, s));
                gemm_args fc1 = fp8(linear(Mc, a8, L->fc1_w8, L->fc1_b, big, dt, 4 * E, E, MST_EPI_BIAS_GELU), am + 2, L->w8_scale[2]);
                fc1.out_amax = am + 3;   // the hidden activation's maximum, for the quantiser below
                RUNK(MST_K_GEMM_FC1, launch_gemm8(fc1));
                RUN(launch_quant8(big, dt, Mc * 4 * E, am + 3, a8, 0, s));
                RUNK(MST_K_GEMM_FC2, launch_gemm8(fp8(residual(Mc, a8, L->fc2_w8, L->fc2_b, L->ls2, 4 * E, E), am + 3, L->w8_scale[3])));
                return MST_OK;
            }
            case TAIL_BLOCK_SINGLE:   // one launch, x read and written once; rows stay in the registers of the wave that owns them
                RUNK(MST_K_BLOCK_FUSED, launch_block16s(x, xn, xn_out, dt, L->block_seq, L->fc1_bf, L->proj_bf, L->fc2_bf, Mc, E, 1e-6f,
                                                       blocked ? (MST_LAYOUT_ACT_BLOCKED | (l > 0 ? MST_LAYOUT_X_IN_IMAGE : 0) | (l + 1 < w->depth ? MST_LAYOUT_X_OUT_IMAGE : 0)) : 0, s));
                return MST_OK;
            case TAIL_BLOCK_ROLES:
                RUNK(MST_K_BLOCK_FUSED, launch_block16(x, xn, xn_out, dt, L->proj_pack, L->proj_bf, L->mlp_pack, L->fc1_bf, L->fc2_bf, blk, Mc, E, 1e-6f, s));
                return MST_OK;
            case TAIL_MLP_FUSED:
                RUNK(MST_K_GEMM_PROJ, gemm(residual(Mc, xn, L->proj_w, L->proj_b, L->ls1, E, E)));
                RUNK(MST_K_MLP_FUSED, launch_mlp16(x, xn_out, dt, L->mlp_pack, L->fc1_bf, L->fc2_bf, Mc, E, 1e-6f, s));
                return MST_OK;
            case TAIL_SWIGLU:
                RUNK(MST_K_GEMM_PROJ, gemm(residual(Mc, xn, L->proj_w, L->proj_b, L->ls1, E, E)));
                RUNK(MST_K_LAYERNORM, launch_layernorm(x, E, L->ln2_w, L->ln2_b, xn, dt, E, Mc, E, 1e-6f, s));
                RUNK(MST_K_GEMM_FC1, gemm(swiglu(Mc, xn, L)));
                RUNK(MST_K_GEMM_FC2, gemm(residual(Mc, big, L->fc2_w, L->fc2_b, L->ls2, w->ffn_hidden, E)));
                return MST_OK;
            case TAIL_UNFUSED:
                RUNK(MST_K_GEMM_PROJ, gemm(residual(Mc, xn, L->proj_w, L->proj_b, L->ls1, E, E)));
                RUNK(MST_K_LAYERNORM, launch_layernorm(x, E, L->ln2_w, L->ln2_b, xn, dt, E, Mc, E, 1e-6f, s));
                RUNK(MST_K_GEMM_FC1, gemm(linear(Mc, xn, L->fc1_w, L->fc1_b, big, dt, 4 * E, E, MST_EPI_BIAS_GELU)));
                RUNK(MST_K_GEMM_FC2, gemm(residual(Mc, big, L->fc2_w, L->fc2_b, L->ls2, 4 * E, E)));
                return MST_OK;
        }
        return MST_EINVAL;   // not reached: every vit_tail returns above
    }
};

}  // extern "C"

// What mst_vit_encode_features adds to an encoder call: true RGB input and the taps.  All zero: mst_vit_encode, launch for launch.
struct vit_features {
    const void* patch_w_rgb;      // non-null: vol is [n, 3, H, W] and this the [E][3][14][16] kernel image
    const mst_vit_taps* taps;     // nullable
};

static int vit_encode_run(const mst_vit_weights* w, const void* vol, int in_dtype, int n_slices, int H, int W,
                          float* cls_out, float* cls_probs, float* full_probs, int n_layers_probs, int chunk_slices,
                          void* ws, size_t ws_bytes, mst_stream_t stream, const vit_features& f) {
    hipStream_t s = (hipStream_t)stream;
    MST_CHECK_ARG(w && vol && ws, "vit_encode: null pointer");
    mst_profiler* const prof = w->profiler;
    MST_CHECK_ARG(w->layers && w->depth > 0, "vit_encode: no layers");
    MST_CHECK_ARG(H > 0 && W > 0 && H % 14 == 0 && W % 14 == 0, "vit_encode: H=%d W=%d must be multiples of 14", H, W);
    MST_CHECK_ARG(H / 14 == w->grid_h && W / 14 == w->grid_w, "vit_encode: pos_patch prepared for grid %dx%d, input is %dx%d",
                  w->grid_h, w->grid_w, H / 14, W / 14);
    const int E = w->embed_dim, heads = w->num_heads, dt = w->compute_dtype;
    MST_CHECK_ARG(heads > 0 && E == heads * 64, "vit_encode: embed_dim=%d must be 64*num_heads (%d)", E, heads);
    MST_CHECK_ARG(dt == MST_F16 || dt == MST_BF16 || dt == MST_F32, "vit_encode: bad compute dtype %d", dt);
    MST_CHECK_ARG(n_slices > 0 && chunk_slices > 0, "vit_encode: n_slices=%d chunk=%d", n_slices, chunk_slices);
    MST_CHECK_ARG(n_layers_probs >= 0 && n_layers_probs <= w->depth, "vit_encode: n_layers_probs=%d", n_layers_probs);
    MST_CHECK_ARG(w->ffn_kind == MST_FFN_MLP || w->ffn_kind == MST_FFN_SWIGLU, "vit_encode: ffn_kind=%d", w->ffn_kind);
    if (w->ffn_kind == MST_FFN_SWIGLU) {
        MST_CHECK_ARG(w->ffn_hidden > 0 && w->ffn_hidden % 64 == 0 && w->ffn_hidden <= 4 * E,
                      "vit_encode: ffn_hidden=%d must be a multiple of 64, at most 4 * embed_dim (the padded width of hip.pack_swiglu)", w->ffn_hidden);
        MST_CHECK_ARG(!w->fp8_linear, "vit_encode: fp8_linear has no SwiGLU form");
    }
    const int R = w->num_registers, Np = w->grid_h * w->grid_w, N = 1 + R + Np;
    if (chunk_slices > n_slices) chunk_slices = n_slices;
    size_t off_xn, off_big, total, off_a8 = 0, off_amax = 0, off_blk = 0;
    vit_carve(w, N, chunk_slices, &off_xn, &off_big, &total, &off_a8, &off_amax, &off_blk);
    if (ws_bytes < total) {
        mst_set_error("vit_encode: workspace %zu < %zu bytes", ws_bytes, total);
        return MST_EWORKSPACE;
    }
    const bool fp8 = w->fp8_linear != 0;
    if (fp8) {
        MST_CHECK_ARG(dt == MST_F16 || dt == MST_BF16, "vit_encode: fp8_linear needs a 16-bit compute dtype");
        MST_CHECK_ARG(E % 128 == 0, "vit_encode: fp8_linear needs embed_dim %% 128 == 0 (got %d)", E);
        for (int l = 0; l < w->depth; ++l)
            MST_CHECK_ARG(w->layers[l].qkv_w8 && w->layers[l].proj_w8 && w->layers[l].fc1_w8 && w->layers[l].fc2_w8,
                          "vit_encode: fp8_linear set but layer %d has no e4m3 weights", l);
    }
    const size_t in_sz = dt_size(in_dtype) * (f.patch_w_rgb ? 3 : 1);     // bytes per pixel position of an image (RGB: three planes)
    // head_dim^-0.5, head_dim = 64 (attention.py:48); the 16-bit attention kernels work in the log2 domain, so log2(e) rides
    // on the same fp32 multiply of the QKV epilogue (one rounding of q, not two)
    const int log2q = dt != MST_F32;
    const float qscale = log2q ? 0.125f * 1.4426950408889634f : 0.125f;
    char* const p = (char*)ws;
    vit_call k{w, (float*)ws, fp8 ? (float*)(p + off_amax) : nullptr, p + off_xn, p + off_big, fp8 ? p + off_a8 : nullptr, p + off_blk,
               dt, E, heads, N, log2q, qscale, prof, s, 0, 0, false};
    const vit_plan plan = vit_resolve(w, (int64_t)n_slices * N);

    for (int s0 = 0; s0 < n_slices; s0 += chunk_slices) {
        const int c = k.c = (n_slices - s0 < chunk_slices) ? n_slices - s0 : chunk_slices;
        const int64_t Mc = k.Mc = (int64_t)c * N;
        const char* v = (const char*)vol + (size_t)s0 * H * W * in_sz;
        // the two choices that depend on the chunk (the last one can be shorter).  Blocked: between two single-role block launches
        // the rows stay in the order the registers hold them (include/mst_hip.h, mst_layout_flags): x as the fp32 image from block 0's
        // output to the last block's input, the 16-bit rows (attention output, normalised rows) blocked from block 0's attention on.
        // Needs the QKV kernel that reads blocked rows (weights-in-registers form) and every block on the fused path.
        const bool prune = plan.may_prune && c <= 65535 && !f.taps;          // the pruned block has no patch rows to tap
        k.blocked = plan.tail == TAIL_BLOCK_SINGLE && !prune && gemm16_wreg_applicable(k.qkv_linear(nullptr, nullptr, nullptr));
        // tokens: in the fused pipeline one kernel writes the residual stream AND block 0's plain-normalised rows (k_patch_rows.hip)
        if (f.patch_w_rgb) {
            // true RGB (k_features.hip): the same x; the fused pipeline's plain-normalised rows by a LayerNorm launch without affine
            RUNK(MST_K_PATCH_EMBED, launch_patch_embed_rgb(v, in_dtype, c, H, W, f.patch_w_rgb, dt, w->patch_b, w->prefix, 1 + R, w->pos_patch, E, k.x, s));
            if (plan.fused_ln) RUNK(MST_K_LAYERNORM, launch_layernorm(k.x, E, nullptr, nullptr, k.xn, dt, E, Mc, E, 1e-6f, s));
        } else if (plan.fused_ln)
            RUNK(MST_K_PATCH_EMBED, launch_patch_rows16(v, in_dtype, c, H, W, w->patch_w, dt, w->patch_b, w->prefix, 1 + R, w->pos_patch, k.x, k.xn, s));
        else
            RUNK(MST_K_PATCH_EMBED, launch_patch_embed(v, in_dtype, c, H, W, w->patch_w, dt, w->patch_b, w->prefix, 1 + R, w->pos_patch, E, k.x, s));
        if (plan.tail == TAIL_FP8_DYNAMIC && hipMemsetAsync(k.amax, 0, (size_t)w->depth * 4 * sizeof(float), s) != hipSuccess) {
            mst_set_error("vit_encode: hipMemsetAsync(amax) failed");
            return MST_ELAUNCH;
        }
        for (int l = 0; l < w->depth; ++l) {
            RUN(k.qkv(plan, l));
            const int li = l - (w->depth - n_layers_probs);
            float* const pr = (cls_probs && li >= 0) ? cls_probs + ((int64_t)li * n_slices + s0) * heads * N : nullptr;
            if (full_probs && li >= 0)
                RUN(launch_probs_full(k.big, dt, c, N, heads, 64, full_probs + ((int64_t)li * n_slices + s0) * heads * N * N, log2q, s));
            if (prune && l == w->depth - 1) {
                RUN(k.pruned_last_block(l, pr));
                continue;
            }
            if (pr) RUNK(MST_K_CLS_PROBS, launch_cls_probs(k.big, dt, c, N, heads, 64, pr, log2q, s));
            if (dt == MST_F32) RUNK(MST_K_ATTENTION, launch_attn32((const float*)k.big, c, N, heads, (float*)k.xn, s));
            else RUNK(MST_K_ATTENTION, launch_attn16(k.big, dt, c, N, heads, k.xn, 1, s, k.blocked ? 1 : 0));
            RUN(k.tail(plan.tail, l));
            for (int t = 0; f.taps && t < f.taps->n_taps; ++t) {
                if (f.taps->blocks[t] != l) continue;
                // x behind block l: the fp32 image between two single-role block launches of the blocked plan, plain rows otherwise
                float* const out = f.taps->out + ((int64_t)t * n_slices + s0) * N * E;
                const bool norm = f.taps->norm != 0;
                RUNK(MST_K_LAYERNORM, launch_tap_rows(k.x, k.blocked && l + 1 < w->depth, norm ? w->norm_w : nullptr, norm ? w->norm_b : nullptr,
                                                      out, Mc, E, 1e-6f, s));
            }
        }
        if (plan.tail == TAIL_FP8_DYNAMIC && w->fp8_amax_out) RUN(launch_amax_merge(w->fp8_amax_out, k.amax, w->depth * 4, s));
        // final norm, CLS rows only (vision_transformer.py:263-265,329)
        if (cls_out) RUN(launch_layernorm(k.x, (int64_t)N * E, w->norm_w, w->norm_b, cls_out + (int64_t)s0 * E, MST_F32, E, c, E, 1e-6f, s));
    }
    return MST_OK;
}

extern "C" {

int mst_vit_encode(const mst_vit_weights* w, const void* vol, int in_dtype, int n_slices, int H, int W,
                   float* cls_out, float* cls_probs, float* full_probs, int n_layers_probs, int chunk_slices,
                   void* ws, size_t ws_bytes, mst_stream_t stream) {
    MST_CHECK_ARG(cls_out, "vit_encode: null pointer");
    return vit_encode_run(w, vol, in_dtype, n_slices, H, W, cls_out, cls_probs, full_probs, n_layers_probs, chunk_slices, ws, ws_bytes,
                          stream, vit_features{nullptr, nullptr});
}

// ---- encoder API: patch tokens and intermediate layers (vision_transformer.py:254-329) -----------------------------------
size_t mst_vit_features_workspace_bytes(const mst_vit_weights* w, int in_channels, int H, int W, int chunk_images) {
    if (in_channels != 1 && in_channels != 3) return 0;
    return mst_vit_workspace_bytes(w, H, W, chunk_images);      // the RGB kernel and the taps need no scratch of their own
}

int mst_vit_encode_features(const mst_vit_weights* w, const void* img, int in_dtype, int in_channels, int n_images, int H, int W,
                            const void* patch_w_rgb, float* cls_out, const mst_vit_taps* taps, int chunk_images, void* ws,
                            size_t ws_bytes, mst_stream_t stream) {
    MST_CHECK_ARG(w, "vit_encode_features: null pointer");
    MST_CHECK_ARG(in_channels == 1 || in_channels == 3, "vit_encode_features: in_channels=%d (1: grey slices, 3: RGB images)", in_channels);
    MST_CHECK_ARG(in_channels == 1 || patch_w_rgb, "vit_encode_features: RGB input needs patch_w_rgb");
    MST_CHECK_ARG(in_dtype == MST_F32 || in_dtype == MST_F16 || in_dtype == MST_BF16, "vit_encode_features: bad image dtype %d", in_dtype);
    if (taps) {
        MST_CHECK_ARG(!w->fp8_linear, "vit_encode_features: taps are not available with fp8_linear (the e4m3 pipeline is CLS-only): use bf16, fp16 or fp32");
        MST_CHECK_ARG(taps->blocks && taps->out && taps->n_taps >= 1 && taps->n_taps <= w->depth, "vit_encode_features: taps: n_taps=%d of depth %d, or a null pointer",
                      taps->n_taps, w->depth);
        for (int t = 0; t < taps->n_taps; ++t)
            MST_CHECK_ARG(taps->blocks[t] >= 0 && taps->blocks[t] < w->depth && (t == 0 || taps->blocks[t] > taps->blocks[t - 1]),
                          "vit_encode_features: taps->blocks[%d]=%d: strictly ascending indices in [0, %d)", t, taps->blocks[t], w->depth);
    }
    return vit_encode_run(w, img, in_dtype, n_images, H, W, cls_out, nullptr, nullptr, 0, chunk_images, ws, ws_bytes, stream,
                          vit_features{in_channels == 3 ? patch_w_rgb : nullptr, taps});
}

// ---- across-slice transformer + head ----------------------------------------------------------
// workspace carve (fp32): eb [B*D, emb] (bottleneck out) | xs [B*L, emb] | y [B*L, emb] |
//                         qkv [B*L, 3emb] | ao [B*L, emb] | feat [B, emb]
size_t mst_fusion_workspace_bytes(const mst_fusion_weights* w, int B, int D) {
    if (!w || B <= 0 || D <= 0) return 0;
    const size_t L = (size_t)D + 1, e = (size_t)w->emb;
    size_t o = 0;
    o += align_up((size_t)B * D * e * 4, 256);
    o += 4 * align_up((size_t)B * L * e * 4, 256);
    o += align_up((size_t)B * L * 3 * e * 4, 256);
    o += align_up((size_t)B * e * 4, 256);
    return o;
}

int mst_slice_fusion(const mst_fusion_weights* w, const float* emb, int B, int D, const uint8_t* key_padding_mask,
                     float* features, float* logits, float* slice_probs, void* ws, size_t ws_bytes,
                     mst_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    MST_CHECK_ARG(w && emb && features && ws, "slice_fusion: null pointer");
    MST_CHECK_ARG(B > 0 && D > 0, "slice_fusion: B=%d D=%d", B, D);
    const int e = w->emb, L = D + 1;
    const size_t need = mst_fusion_workspace_bytes(w, B, D);
    if (ws_bytes < need) {
        mst_set_error("slice_fusion: workspace %zu < %zu bytes", ws_bytes, need);
        return MST_EWORKSPACE;
    }
    char* p = (char*)ws;
    float* eb = (float*)p;  p += align_up((size_t)B * D * e * 4, 256);
    float* xs = (float*)p;  p += align_up((size_t)B * L * e * 4, 256);
    float* y = (float*)p;   p += align_up((size_t)B * L * e * 4, 256);
    float* ao = (float*)p;  p += align_up((size_t)B * L * e * 4, 256);
    float* y2 = (float*)p;  p += align_up((size_t)B * L * e * 4, 256);
    float* qkv = (float*)p; p += align_up((size_t)B * L * 3 * e * 4, 256);
    float* feat = (float*)p;

    // C[rows, n] = epi(A[rows, k] . W[n, k]^T + bias) in exact fp32 on dense rows (the residual epilogues add onto C)
    auto linear32 = [s](const float* A, const float* W, const float* bias, float* C, int64_t rows, int n, int k, int epi) {
        gemm_args g{A, MST_F32, k, W, k, bias, C, MST_F32, n, rows, n, k};
        g.epi = epi, g.s = s;
        return launch_gemm32(g);
    };
    const float* src = emb;
    if (w->bottleneck_w) {  // dino.py:134-135
        MST_CHECK_ARG(w->emb_in % 16 == 0, "slice_fusion: emb_in=%d must be a multiple of 16", w->emb_in);
        RUN(linear32(emb, w->bottleneck_w, w->bottleneck_b, eb, (int64_t)B * D, e, w->emb_in, MST_EPI_BIAS));
        src = eb;
    } else {
        MST_CHECK_ARG(w->emb_in == e, "slice_fusion: emb_in=%d != emb=%d without a bottleneck", w->emb_in, e);
    }

    int F = e;  // feature width
    if (w->fusion_type == MST_FUSION_TRANSFORMER) {
        MST_CHECK_ARG(w->cls_token && w->in_proj_w && w->out_proj_w && w->lin1_w && w->lin2_w && w->ln1_w && w->ln2_w && w->norm_w,
                      "slice_fusion: missing transformer weights");
        MST_CHECK_ARG(w->num_heads > 0 && e % w->num_heads == 0, "slice_fusion: emb=%d not divisible by heads=%d", e, w->num_heads);
        MST_CHECK_ARG(e % 16 == 0, "slice_fusion: emb=%d must be a multiple of 16", e);
        MST_CHECK_ARG(!w->slice_pos_emb || D <= 256, "slice_fusion: slice_pos_emb holds 256 positions, D=%d", D);
        const int hd = e / w->num_heads;
        const int64_t ML = (int64_t)B * L;
        RUN(launch_slice_tokens(src, w->cls_token, w->slice_pos_emb, B, D, e, xs, s));  // dino.py:140-145
        // x = x + out_proj(attn(in_proj(norm1 x)))                 transformer_blocks.py:567,576-582
        RUN(launch_layernorm(xs, e, w->ln1_w, w->ln1_b, y, MST_F32, e, ML, e, 1e-5f, s));
        RUN(linear32(y, w->in_proj_w, w->in_proj_b, qkv, ML, 3 * e, e, MST_EPI_BIAS));
        if (w->liere_rot) {
            // the reference's LieRE path views [B, 33, heads, hd] and then [B*heads, L, hd] of a permuted tensor:
            // both views fail (RuntimeError) unless D == 32 and B == 1 (rotary_embedding_torch.py:349;
            // transformer_blocks.py:263)
            MST_CHECK_ARG(!w->rope_freqs, "slice_fusion: rope_freqs and liere_rot are exclusive");
            MST_CHECK_ARG(L == 33, "slice_fusion: LieRE is built for 33 tokens (axes_length, transformer_blocks.py:355): "
                          "shape '[%d, 33, %d, %d]' is invalid for %d slices", B, w->num_heads, hd, D);
            MST_CHECK_ARG(B == 1, "slice_fusion: LieRE: view size is not compatible with the rotated tensor's "
                          "size and stride for batch %d > 1 (transformer_blocks.py:263)", B);
        }
        RUN(launch_slice_attn(qkv, B, L, w->num_heads, hd, key_padding_mask, w->rope_freqs, w->liere_rot, ao, slice_probs, s));
        RUN(linear32(ao, w->out_proj_w, w->out_proj_b, xs, ML, e, e, MST_EPI_RESIDUAL));
        // x = x + linear2(relu(linear1(norm2 x)))                  transformer_blocks.py:568,585-587
        RUN(launch_layernorm(xs, e, w->ln2_w, w->ln2_b, y, MST_F32, e, ML, e, 1e-5f, s));
        RUN(linear32(y, w->lin1_w, w->lin1_b, y2, ML, e, e, MST_EPI_BIAS_RELU));
        RUN(linear32(y2, w->lin2_w, w->lin2_b, xs, ML, e, e, MST_EPI_RESIDUAL));
        // final LayerNorm, row 0 of every volume                   dino.py:95,153
        RUN(launch_layernorm(xs, (int64_t)L * e, w->norm_w, w->norm_b, feat, MST_F32, e, B, e, 1e-5f, s));
    } else if (w->fusion_type == MST_FUSION_LINEAR) {  // dino.py:154-155: 'b d e -> b (d e)'
        F = D * e;
        feat = (float*)src;
    } else if (w->fusion_type == MST_FUSION_AVERAGE) {  // dino.py:156-157
        RUN(launch_mean_slices(src, B, D, e, feat, s));
    } else {
        mst_set_error("slice_fusion: bad fusion type %d", w->fusion_type);
        return MST_EINVAL;
    }
    RUN(launch_rows_copy(feat, F, features, F, B, F, s));
    if (logits) {  // dino.py:166
        MST_CHECK_ARG(w->head_w && w->out_ch > 0, "slice_fusion: logits requested without a head");
        MST_CHECK_ARG(F % 16 == 0, "slice_fusion: feature width %d must be a multiple of 16", F);
        MST_CHECK_ARG(w->head_in <= 0 || F == w->head_in, "slice_fusion: mat1 and mat2 shapes cannot be multiplied (%dx%d and %dx%d)",
                      B, F, w->head_in, w->out_ch);
        RUN(linear32(feat, w->head_w, w->head_b, logits, B, w->out_ch, F, MST_EPI_BIAS));
    }
    return MST_OK;
}

int mst_attention_readout(const float* cls_probs_last, const float* slice_probs, int B, int D, int heads, int N,
                          int num_registers, int sheads, float* plane, float* slice_attn, float* maps,
                          mst_stream_t stream) {
    MST_CHECK_ARG(B > 0 && D > 0 && heads > 0 && N > 1 + num_registers, "readout: bad sizes");
    return launch_readout(cls_probs_last, slice_probs, B, D, heads, N, num_registers, sheads, plane, slice_attn, maps,
                          (hipStream_t)stream);
}

int mst_saliency_accumulate(const float* maps, const float* slice_attn, int D, int heads, int gh, int gw, int Np,
                            int flip_mask, int accumulate, float* lowres, float* slice_acc, mst_stream_t stream) {
    MST_CHECK_ARG(maps && lowres && (slice_attn || !slice_acc), "saliency_accumulate: null pointer");
    MST_CHECK_ARG(D > 0 && heads > 0 && gh > 0 && gw > 0 && gh * gw <= Np, "saliency_accumulate: grid %d x %d does not fit %d map columns", gh, gw, Np);
    MST_CHECK_ARG((flip_mask & ~7) == 0, "saliency_accumulate: flip_mask %d", flip_mask);
    return launch_saliency_accumulate(maps, slice_attn, D, heads, gh, gw, Np, flip_mask, accumulate, lowres, slice_acc,
                                      (hipStream_t)stream);
}

int mst_saliency_upsample(const float* lowres, int D, int gh, int gw, float scale, int Dout, int H, int W, float* out,
                          mst_stream_t stream) {
    MST_CHECK_ARG(lowres && out, "saliency_upsample: null pointer");
    MST_CHECK_ARG(D > 0 && gh > 0 && gw > 0 && Dout > 0 && H > 0 && W > 0, "saliency_upsample: bad sizes");
    return launch_saliency_upsample(lowres, D, gh, gw, scale, Dout, H, W, out, (hipStream_t)stream);
}

int mst_tta_inplane_flips(const void* x, int dtype, int n, int H, int W, void* out, mst_stream_t stream) {
    MST_CHECK_ARG(x && out && x != out, "tta_inplane_flips: null pointer, or out is x");
    MST_CHECK_ARG(dtype == MST_F32 || dtype == MST_F16 || dtype == MST_BF16, "tta_inplane_flips: bad dtype %d", dtype);
    MST_CHECK_ARG(n > 0 && H > 0 && W > 0, "tta_inplane_flips: bad sizes %d x %d x %d", n, H, W);
    MST_CHECK_ARG(aligned(x, dtype == MST_F32 ? 4 : 2) && aligned(out, dtype == MST_F32 ? 4 : 2), "tta_inplane_flips: x and out must be aligned to their element");
    return launch_tta_inplane_flips(x, dtype, n, H, W, out, (hipStream_t)stream);
}

int mst_saliency_accumulate_tta(const float* plane, const float* slice_attn, int D, int heads, int gh, int gw, int Np,
                                float* lowres, float* slice_acc, mst_stream_t stream) {
    MST_CHECK_ARG(plane && slice_attn && lowres, "saliency_accumulate_tta: null pointer");
    MST_CHECK_ARG(D > 0 && heads > 0 && gh > 0 && gw > 0 && gh * gw <= Np, "saliency_accumulate_tta: grid %d x %d does not fit %d map columns", gh, gw, Np);
    return launch_saliency_accumulate_tta(plane, slice_attn, D, heads, gh, gw, Np, lowres, slice_acc, (hipStream_t)stream);
}

int mst_liere_rotation(const float* vars, int n_blocks, int block, int axes_length, float* R, mst_stream_t stream) {
    MST_CHECK_ARG(vars && R, "liere_rotation: null pointer");
    return launch_liere_rotation(vars, n_blocks, block, axes_length, R, (hipStream_t)stream);
}

int mst_attention_rollout(const float* const* maps, int n_layers, int64_t batch, int N, float* out, float* tmp,
                          mst_stream_t stream) {
    MST_CHECK_ARG(maps && out && n_layers >= 1 && batch > 0 && N > 0, "rollout: bad arguments");
    MST_CHECK_ARG(n_layers <= 2 || tmp, "rollout: tmp is required for more than two maps");
    hipStream_t s = (hipStream_t)stream;
    for (int l = 0; l < n_layers; ++l)
        MST_CHECK_ARG(maps[l] && maps[l] != out && maps[l] != tmp, "rollout: map %d is null or aliases out/tmp", l);
    if (n_layers == 1) {
        if (hipMemcpyAsync(out, maps[0], sizeof(float) * (size_t)batch * N * N, hipMemcpyDeviceToDevice, s) != hipSuccess) {
            mst_set_error("rollout: copy failed");
            return MST_ELAUNCH;
        }
        return MST_OK;
    }
    // n_layers - 1 products, alternating tmp/out so that the last one lands in `out`
    const float* cur = maps[n_layers - 1];
    const int links = n_layers - 1;
    for (int i = 0; i < links; ++i) {
        float* dst = ((links - 1 - i) & 1) ? tmp : out;
        int rc = launch_bmm32_nn(maps[n_layers - 2 - i], cur, dst, batch, N, N, N, s);
        if (rc != MST_OK) return rc;
        cur = dst;
    }
    return MST_OK;
}

mst_profiler* mst_profiler_create(void) { return new (std::nothrow) mst_profiler(); }

void mst_profiler_destroy(mst_profiler* p) {
    if (!p) return;
    for (auto* v : {&p->used, &p->idle})
        for (const auto& r : *v) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    delete p;
}

int mst_profiler_collect(mst_profiler* p, double* ms_total, int64_t* launches) {
    MST_CHECK_ARG(p && ms_total && launches, "profiler_collect: null pointer");
    std::lock_guard<std::mutex> lk(p->mu);
    for (int k = 0; k < MST_K_COUNT; ++k) { ms_total[k] = 0.0; launches[k] = 0; }
    for (const auto& r : p->used) {
        float ms = 0.f;
        if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) {
            mst_set_error("profiler_collect: event query failed");
            return MST_ELAUNCH;
        }
        ms_total[r.kind] += ms;
        launches[r.kind] += 1;
        p->idle.push_back(r);
    }
    p->used.clear();
    return MST_OK;
}

const char* mst_kernel_kind_name(int kind) { return (kind >= 0 && kind < MST_K_COUNT) ? kKindNames[kind] : "?"; }

}  // extern "C"
