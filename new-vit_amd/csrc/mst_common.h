// Shared device helpers for the gfx950 (CDNA4, wave64) kernels of libmst_hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/mst_hip.h"

typedef __bf16 bf16_t;
typedef _Float16 f16_t;

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

#define MST_WAVE 64
#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define GLB_PTR(p) ((const __attribute__((address_space(1))) void*)(p))

template <typename T> struct V8;
template <> struct V8<bf16_t> { typedef bf16x8 type; typedef bf16x4 half_type; };
template <> struct V8<f16_t> { typedef f16x8 type; typedef f16x4 half_type; };

// D(16x16 f32) += A(16x32) * B(32x16); lane l holds A[l&15][8*(l>>4)+j], B[8*(l>>4)+j][l&15];
// D[row=(l>>4)*4+r][col=l&15].
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
// D(32x32 f32) += A(32x16) * B(16x32); lane l holds A[l&31][8*(l>>5)+j], B[8*(l>>5)+j][l&31];
// D[row=(r&3)+8*(r>>2)+4*(l>>5)][col=l&31].
__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma32(f16x8 a, f16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(bf16_t v) { return (float)v; }
__device__ __forceinline__ float to_f32(f16_t v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f32(float v) { return (T)v; }

// v as an fp32 register the compiler cannot look through: a conversion to 16 bits behind it rounds the ROUNDED fp32 value.  Without it
// hipcc folds a product and its conversion into one v_fma_mixlo_f16 (a single rounding), and a 16-bit output is no longer the rounded
// fp32 output of the same kernel bit for bit.
__device__ __forceinline__ float f32_rounded(float v) {
    asm("" : "+v"(v));
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// min / max of floats across workgroups by INTEGER atomics on the bit pattern (order-independent, so the same bits whatever the arrival
// order; *a starts at +inf / -inf).  The branch is on the SIGN BIT, not on v >= 0: -0.0 has the pattern 0x80000000 = INT_MIN and, sent
// down the signed path, would overwrite any negative minimum stored before it (and never raise a maximum above -inf).  Patterns with the sign
// clear order like signed ints; with it set, a larger unsigned pattern is a smaller float.  NaNs are the caller's to keep out (fminf / fmaxf).
__device__ __forceinline__ void atomic_min_f32(float* a, float v) {
    if (__float_as_int(v) >= 0) atomicMin((int*)a, __float_as_int(v)); else atomicMax((unsigned*)a, __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_f32(float* a, float v) {
    if (__float_as_int(v) >= 0) atomicMax((int*)a, __float_as_int(v)); else atomicMin((unsigned*)a, __float_as_uint(v));
}

__device__ __forceinline__ float gelu_erf(float v) {  // nn.GELU() exact form (mlp.py:22)
    return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
}
// act'(v) of the training step's act_bwd.  kind 0: GELU (erf form), 1: ReLU.
__device__ __forceinline__ float act_deriv(float v, int kind) {
    if (kind == 0) return 0.5f * (1.0f + erff(v * 0.70710678118654752440f)) + v * 0.3989422804014327f * expf(-0.5f * v * v);
    return v > 0.f ? 1.f : 0.f;
}
// BatchNorm with batch statistics (k_bn.hip), each expression once and with every rounding spelled out (no contraction left to the
// compiler), so that every instantiation of the apply kernels -- fp32 / 16-bit storage, 8 or 1 channels per thread -- returns the same bits
// on the same values.  y = gamma (z - mean) rstd + beta;  dz = gamma rstd (dy - d beta / rows - xhat d gamma / rows) with inv = 1 / rows
// (d beta inv as a rounded product: it does not depend on the row, and a compiler that hoists it out of a row loop must not change the bits).
__device__ __forceinline__ float bn_fwd_value(float z, float mean, float rstd, float gamma, float beta) {
    return fmaf(__fmul_rn(gamma, __fsub_rn(z, mean)), rstd, beta);
}
__device__ __forceinline__ float bn_bwd_value(float z, float mean, float rstd, float gamma, float dy, float dgamma, float dbeta, float inv) {
    const float xh = __fmul_rn(__fsub_rn(z, mean), rstd);
    const float t = __fsub_rn(dy, __fmul_rn(dbeta, inv));
    return __fmul_rn(__fmul_rn(gamma, rstd), fmaf(-__fmul_rn(xh, dgamma), inv, t));
}

// eight consecutive elements as fp32, in 16-byte accesses (two for fp32).  The 16-bit store rounds to nearest even what it is given: a
// kernel whose output must be T(its fp32 result) passes the values through f32_rounded first.
template <typename T>
__device__ __forceinline__ void load8(const T* p, float v[8]) {
    const typename V8<T>::type t = *reinterpret_cast<const typename V8<T>::type*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
}
template <typename T>
__device__ __forceinline__ void store8(T* p, const float v[8]) {
    typename V8<T>::type t;
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = (T)v[e];                     // round to nearest even
    *reinterpret_cast<typename V8<T>::type*>(p) = t;
}
__device__ __forceinline__ void load8(const float* p, float v[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
}
__device__ __forceinline__ void store8(float* p, const float v[8]) {
    f32x4 a, b;
#pragma unroll
    for (int e = 0; e < 4; ++e) { a[e] = v[e]; b[e] = v[4 + e]; }
    *reinterpret_cast<f32x4*>(p) = a;
    *reinterpret_cast<f32x4*>(p + 4) = b;
}
// V = 8 elements as above, or one
template <int V, typename T>
__device__ __forceinline__ void loadv(const T* p, float v[V]) {
    if constexpr (V == 8) load8(p, v);
    else v[0] = to_f32(p[0]);
}
template <int V, typename T>
__device__ __forceinline__ void storev(T* p, const float v[V]) {
    if constexpr (V == 8) store8(p, v);
    else p[0] = (T)v[0];
}

// cubic convolution coefficients of the four taps around fraction x, A = -0.75 (what F.interpolate(mode='bicubic') uses)
__device__ __forceinline__ void cubic_w(float x, float w[4]) {
    const float A = -0.75f;
    float t = x + 1.0f;
    w[0] = ((A * t - 5.0f * A) * t + 8.0f * A) * t - 4.0f * A;
    w[1] = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
    t = 1.0f - x;
    w[2] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
    t = 2.0f - x;
    w[3] = ((A * t - 5.0f * A) * t + 8.0f * A) * t - 4.0f * A;
}

// GELU for 16-bit outputs: erf by Abramowitz-Stegun 7.1.26 (|err| <= 1.5e-7 on erf, <= 5e-7 abs /
// 2e-4 rel on gelu: far below one fp16/bf16 ulp), one v_rcp + one v_exp instead of libm erff.
// The negative branch multiplies by the complementary term directly (no 1 - erf cancellation).
__device__ __forceinline__ float gelu_fast(float v) {
    const float z = fabsf(v) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    float p = fmaf(t, 1.061405429f, -1.453152027f);
    p = fmaf(t, p, 1.421413741f);
    p = fmaf(t, p, -0.284496736f);
    p = fmaf(t, p, 0.254829592f);
    const float pe = p * t * __builtin_amdgcn_exp2f(-z * z * 1.4426950408889634f);  // = erfc(z)
    const float h = 0.5f * v;
    return v >= 0.f ? h * (2.0f - pe) : h * pe;
}

// Transcendental-free GELU for 16-bit outputs inside MFMA-dense loops: erf(z) = z*P(z^2) on |z| <= 3.2 (degree-8
// Chebyshev fit, |erf err| <= 8e-5, |gelu err| <= 1.8e-4 absolute: below one fp16/bf16 ulp of O(1) activations),
// saturating to +-1 beyond.  9 FMAs + 5 simple ops, no v_exp / v_rcp (quarter-rate issue).
__device__ __forceinline__ float gelu_poly(float v) {
    const float z = fminf(fabsf(v) * 0.70710678118654752440f, 3.2f);
    const float u = z * z;
    float p = 3.263779068761133e-08f;
    p = fmaf(p, u, -1.673741012956179e-06f);
    p = fmaf(p, u, 3.751051790327989e-05f);
    p = fmaf(p, u, -0.000488409298395181f);
    p = fmaf(p, u, 0.0041668641449124355f);
    p = fmaf(p, u, -0.025040875590456917f);
    p = fmaf(p, u, 0.11119564373069263f);
    p = fmaf(p, u, -0.37554270907102755f);
    p = fmaf(p, u, 1.1283444184507676f);
    const float e = fminf(p * z, 1.0f);            // erf(|v|/sqrt2)
    const float h = 0.5f * v;
    return fmaf(fabsf(h), e, h);                   // 0.5 v (1 + sign(v) erf) = h + |h| e
}

// GELU for 16-bit outputs inside ISSUE-bound MFMA loops: v * sigmoid(v * P(v^2)), P fitted (minimax, scipy) to the exact
// erf form.  Beside dense MFMAs the SIMD's vector issue port is the scarce resource (an MFMA holds it 8 of its 16
// cycles, a plain VALU op 4, v_exp/v_rcp 8): this form costs 36 (bf16) / 44 (fp16) issue cycles per value against 60 for
// gelu_poly.  |error| vs nn.GELU(): 2.7e-4 with the linear P (bf16: 1/30 of a bf16 ulp at 1.0), 2.5e-5 with the
// quadratic P (fp16).  exp2 overflow for v < -10 gives rcp(inf) = 0 -> -0, the right limit.
template <typename T> __device__ __forceinline__ float gelu_sig(float v);
template <> __device__ __forceinline__ float gelu_sig<bf16_t>(float v) {
    const float w = fmaf(v * v, -0.06940179f * 1.4426950408889634f, -1.60031416f * 1.4426950408889634f);
    const float e = __builtin_amdgcn_exp2f(v * w);                 // exp(-v (a + b v^2))
    return v * __builtin_amdgcn_rcpf(1.0f + e);
}
template <> __device__ __forceinline__ float gelu_sig<f16_t>(float v) {
    const float c = __builtin_amdgcn_fmed3f(v, -8.0f, 8.0f);       // the quadratic P turns over at |v| = 8.35
    const float u = c * c;
    float w = fmaf(u, 7.03033577e-04f * 1.4426950408889634f, -7.40112920e-02f * 1.4426950408889634f);
    w = fmaf(w, u, -1.59501577f * 1.4426950408889634f);
    const float e = __builtin_amdgcn_exp2f(c * w);
    return v * __builtin_amdgcn_rcpf(1.0f + e);
}

// silu(g) * v of the MST_EPI_BIAS_SWIGLU GEMM epilogue (k_gemm16.hip, k_gemm32.hip).  Exact form for fp32 output; for 16-bit output one
// v_exp + one v_rcp (relative error ~2 ulp of fp32: far below one fp16 / bf16 ulp), as gelu_fast is for GELU.  A large negative gate:
// exp -> inf, g / inf = g * 0 = -0, never NaN.
template <bool FAST>
__device__ __forceinline__ float swiglu_gate(float g, float v) {
    if (FAST) return g * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-g * 1.4426950408889634f)) * v;
    return g / (1.0f + expf(-g)) * v;
}

// SwiGLU of the training step (layers/swiglu_ffn.py:54-72; x12 = [x1 | x2] as chunk(2, dim=-1) gives it): h = silu(x1) x2 and its
// gradient, in fp32 with every product spelled out (no contraction left to the compiler), so that every instantiation of the
// swiglu kernels of k_train.hip (fp32 / 16-bit storage, 8 or 1 columns per thread) returns the same bits on the same values.
// x1 -> -inf side: expf overflows to inf, s = 0, h = (x1 / inf) * x2 = -0 * x2; nothing is NaN for finite inputs.
__device__ __forceinline__ float swiglu_sigmoid(float x1) { return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-x1))); }
__device__ __forceinline__ float swiglu_fwd_value(float x1, float x2) { return __fmul_rn(__fdiv_rn(x1, __fadd_rn(1.0f, expf(-x1))), x2); }
__device__ __forceinline__ void swiglu_bwd_values(float x1, float x2, float dh, float* d1, float* d2) {
    const float s = swiglu_sigmoid(x1);
    const float t = __fadd_rn(1.0f, __fmul_rn(x1, __fsub_rn(1.0f, s)));       // silu'(x1) = s (1 + x1 (1 - s))
    *d1 = __fmul_rn(__fmul_rn(__fmul_rn(dh, x2), s), t);
    *d2 = __fmul_rn(__fmul_rn(dh, x1), s);
}

// Bijective XCD-aware remap of a 1-D grid: blocks b and b+8 share an XCD (round-robin dispatch),
// so give each XCD a contiguous run of tile ids (neighbouring tiles share operand panels in its L2).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
    const int base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    return base + (bid >> 3);
}

// host side ---------------------------------------------------------------------------------
void mst_set_error(const char* fmt, ...);
#define MST_CHECK_ARG(cond, ...)                \
    do {                                        \
        if (!(cond)) {                          \
            mst_set_error(__VA_ARGS__);         \
            return MST_EINVAL;                  \
        }                                       \
    } while (0)
int mst_check_launch(const char* what);
inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline size_t round256(size_t b) { return (b + 255) / 256 * 256; }
// workgroups of 256 threads striding over n items: 16,384 at most
inline unsigned grid256(int64_t n) {
    const int64_t g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}
// Raise a kernel's dynamic-LDS limit once per (kernel, device): the attribute is per device, and a process may drive
// several GPUs.  Thread-safe; `slot` is a static per-kernel token owned by the call site.
struct mst_lds_once { unsigned long long done_mask = 0; };
void mst_allow_lds(const void* kernel, int bytes, mst_lds_once* slot);
// Compute units of the current device (256 on an MI355X in SPX mode, 32 per logical GPU in CPX mode), cached per device and
// rounded down to a multiple of 8 (the persistent kernels deal tile ids to the 8 XCDs): the size of a persistent grid.
int mst_persistent_grid(void);

// ---- linear-layer GEMMs: C[M,N] = epi(A[M,K] . W[N,K]^T + bias) ---------------------------------------------------------------
// What every launch_gemm* takes (the contract of mst_gemm / mst_gemm_fp8 in include/mst_hip.h).  Fill the operands and the shape; the
// rest defaults to a plain bias epilogue on the null stream.
struct gemm_args {
    const void* A; int dt; int64_t lda;
    const void* W; int64_t ldw;
    const float* bias;
    void* C; int cdt; int64_t ldc;
    int64_t M; int N, K;
    int epi = MST_EPI_BIAS;
    const float* gamma = nullptr;          // residual epilogues: per-column LayerScale (null = 1)
    float col_scale = 1.f; int scale_cols = 0;   // columns [0, scale_cols) are multiplied by col_scale
    hipStream_t s = nullptr;
    // e4m3 operands (launch_gemm8) only
    const float* a_amax = nullptr; float w_scale = 1.f;   // per-tensor scales: max|A| behind the quantiser, max|W| / 448
    float* out_amax = nullptr;             // (nullable, 16-bit C, non-residual epilogues) *out_amax = max(*out_amax, max |C as stored|)
    const float* c_amax = nullptr;         // (cdt == MST_F8E4M3 only) calibrated scale of the e4m3 output
};

// The runtime (dt, cdt, epi) of a GEMM as the (T, EPI, OutT) of a kernel template: f.template launch<T, EPI, OutT>(g) for the
// combinations f.template has<T, EPI, OutT>() names -- each file states there which kernels it instantiates; nothing else is compiled.
// Every launcher has the plain bias epilogue for each operand type it takes, which is how an unknown operand type is told from an
// unknown epilogue.
template <typename X> struct gemm_type { typedef X type; };
constexpr int GEMM_NO_KERNEL = -1;
template <typename Fn> int gemm_with_type(int dt, Fn fn) {
    switch (dt) {
        case MST_F32: return fn(gemm_type<float>{});
        case MST_F16: return fn(gemm_type<f16_t>{});
        case MST_BF16: return fn(gemm_type<bf16_t>{});
        case MST_F8E4M3: return fn(gemm_type<uint8_t>{});
    }
    return GEMM_NO_KERNEL;
}
template <typename Fn> int gemm_with_epi(int epi, Fn fn) {
    switch (epi) {
        case MST_EPI_BIAS: return fn(std::integral_constant<int, MST_EPI_BIAS>{});
        case MST_EPI_BIAS_GELU: return fn(std::integral_constant<int, MST_EPI_BIAS_GELU>{});
        case MST_EPI_BIAS_RELU: return fn(std::integral_constant<int, MST_EPI_BIAS_RELU>{});
        case MST_EPI_RESIDUAL: return fn(std::integral_constant<int, MST_EPI_RESIDUAL>{});
        case MST_EPI_RESIDUAL_RELU: return fn(std::integral_constant<int, MST_EPI_RESIDUAL_RELU>{});
    }
    return GEMM_NO_KERNEL;
}
template <typename F> int gemm_dispatch(const char* kernel, const gemm_args& g, const F& f) {
    bool operand_ok = false;
    const int rc = gemm_with_type(g.dt, [&](auto t) {
        typedef typename decltype(t)::type T;
        operand_ok = F::template has<T, MST_EPI_BIAS, T>() || F::template has<T, MST_EPI_BIAS, float>();
        return gemm_with_type(g.cdt, [&](auto o) {
            typedef typename decltype(o)::type OutT;
            return gemm_with_epi(g.epi, [&](auto e) {
                constexpr int EPI = decltype(e)::value;
                if constexpr (F::template has<T, EPI, OutT>()) return f.template launch<T, EPI, OutT>(g);
                else return GEMM_NO_KERNEL;
            });
        });
    });
    if (rc != GEMM_NO_KERNEL) return rc;
    if (operand_ok) mst_set_error("%s: bad epilogue %d", kernel, g.epi);
    else mst_set_error("%s: bad operand dtype %d", kernel, g.dt);
    return MST_EINVAL;
}

// Tile geometry (rows, columns, k per step) the 16-bit router shares with the kernels it chooses between (k_gemm16.hip: gemm16_route)
struct gemm_tile { int bm, bn, bk; };
constexpr gemm_tile GEMM16_WREG_TILE{32, 384, 384};   // k_gemm16_wreg.hip: 32-row chunks against a register-resident K = 384 weight slice
constexpr gemm_tile GEMM16_MID_TILE{128, 384, 32};    // k_gemm16_mid.hip
constexpr gemm_tile GEMM16_BIG_TILE{256, 384, 32};    // k_gemm16_big.hip

int launch_gemm16(const gemm_args& g);                // k_gemm16.hip: argument checks, then the kernel gemm16_route names
int launch_gemm16_big(const gemm_args& g);
int launch_gemm16_mid(const gemm_args& g);
// the shape rule of the weights-in-registers kernel (operand pointers are not looked at): mst_vit_encode keeps the blocked layout only where it holds
bool gemm16_wreg_applicable(const gemm_args& g);
// a_blocked: A in the 16-bit blocked layout of include/mst_hip.h (whole 32-row groups allocated; lda ignored)
int launch_gemm16_wreg(const gemm_args& g, int a_blocked = 0);
// fp32 partial products of `splits` K ranges, split_stride elements apart (g: A, W, C = the partials, ldc, M, N, K; no bias, no epilogue)
int launch_gemm16_splitk(const gemm_args& g, int splits, int64_t split_stride);
int launch_gemm32(const gemm_args& g);
bool gemm32_small_applicable(int64_t M, int N, int K);
int launch_gemm32_small(const gemm_args& g);
int launch_gemm8(const gemm_args& g);

// kernel launchers shared between translation units (all asynchronous on `s`)
int launch_layernorm(const float* x, int64_t xs, const float* g, const float* b, void* out, int odt,
                     int64_t os, int64_t rows, int cols, float eps, hipStream_t s);
int launch_patch_rows16(const void* vol, int idt, int n, int H, int W, const void* wp, int dt, const float* bias, const float* prefix,
                        int n_prefix, const float* pos_patch, float* x, void* xn, hipStream_t s);
int launch_cvt16(const float* x, int64_t ldx, int64_t rows, int cols, float scale, void* out, int dt, int64_t ldo, int transpose,
                 int64_t rows_pad, hipStream_t s);
int launch_conv_dgrad32(const float* dz, int n, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, const float* Wt, int H, int W,
                        int Cin, float* dx, hipStream_t s);
int launch_conv_dgrad16(const void* dz, int dt, int n, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, const void* Wt, int H, int W,
                        int Cin, float* dx, hipStream_t s);
int launch_conv_dgrad_stem(const void* dz, int dt, int n, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, const void* Wg, int H, int W,
                           int Cin, float* dx, hipStream_t s);   // k_conv_stem_dgrad.hip
int launch_conv_wgrad32(const float* dz, const float* x, int n, int H, int W, int Cin, int kh, int kw, int stride, int pad, int Cout, float* part,
                        int nsplit, int64_t rows_per_split, hipStream_t s);
int launch_conv_wgrad16(const void* dz, const void* x, int dt, int n, int H, int W, int Cin, int kh, int kw, int stride, int pad, int Cout, float* part,
                        int nsplit, int64_t rows_per_split, hipStream_t s);
// memory-efficient training attention (k_attn16_train.hip)
size_t attn_train_workspace_bytes(int n_seq, int N, int heads);
// out16: `out` is in qkv's 16-bit type instead of fp32 (the 16-bit storage mode of the training step)
int launch_attn_train_fwd(const void* qkv, int dt, int n_seq, int N, int heads, void* out, int out16, float* lse, hipStream_t s);
int launch_attn_train_bwd(const void* qkv, int dt, const void* out, int out16, const float* dout, const float* lse, int n_seq, int N, int heads,
                          float dq_scale, float* dqkv, void* ws, size_t ws_bytes, hipStream_t s);
// row kernels of the 16-bit storage mode (k_train16.hip; the act / swiglu forms in k_train.hip, the column sums in k_colsum.hip)
int launch_residual_layernorm16(const float* xin, const void* br, int dt, const float* gamma, float* xout, const float* w, const float* b,
                                void* y, int64_t rows, int cols, float eps, hipStream_t s);
int launch_act_fwd16(const void* h, void* y, int dt, int64_t n, int kind, hipStream_t s);
int launch_act_bwd16(const void* h, int dt, float* dy, int64_t n, int kind, hipStream_t s);
int launch_swiglu_fwd16(const void* x12, void* h, int dt, int64_t rows, int H, hipStream_t s);
int launch_swiglu_bwd16(const void* x12, int dt, const float* dh, float* dx12, int64_t rows, int H, hipStream_t s);
int launch_colsum_b16(const float* a, int64_t as, const void* b, int dt, int64_t bs, int64_t rows, int cols, float* out, hipStream_t s);
int launch_colsum_b16_ordered(const float* a, int64_t as, const void* b, int dt, int64_t bs, int64_t rows, int cols, float* out, void* ws,
                              size_t ws_bytes, hipStream_t s);
int launch_transpose16(const void* x, int dt, int64_t ldx, int64_t rows, int cols, void* out, int64_t ldo, int64_t rows_pad, hipStream_t s);
int launch_rope_rows(float* qkv, int64_t rows, int L, int heads, int hd, const float* freqs, float sign, hipStream_t s);
int launch_im2col_nhwc16(const float* x, int n, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad, void* col, int dt, hipStream_t s);
int launch_cvt32(const void* x, int dt, int64_t n, float* out, hipStream_t s);
int launch_conv_gemm16(const void* x, int dt, int n, int H, int W, int Cin, int kh, int kw, int stride, int pad, const void* Wg, const float* bias,
                       void* out, int cdt, int Cout, int epi, hipStream_t s);
int launch_conv_gemm32(const float* x, int n, int H, int W, int Cin, int kh, int kw, int stride, int pad, const float* Wg, int64_t ldw,
                       const float* bias, float* out, int64_t ldc, int Cout, int Kpad, int epi, const float* gamma, hipStream_t s);
// scan: 1 = *amax = max(*amax, max|x|) first (one extra pass over x); 0 = *amax already covers x (its producer kept it)
int launch_quant8(const void* x, int dt, int64_t n, float* amax, void* out8, int scan, hipStream_t s);
// quantise under a calibrated scale the caller owns (read-only)
int launch_quant8_static(const void* x, int dt, int64_t n, const float* amax, void* out8, hipStream_t s);
int launch_layernorm_f8(const float* x, int64_t xs, const float* g, const float* b, void* out8, int64_t os, int64_t rows,
                        int cols, float eps, const float* amax, hipStream_t s);
int launch_amax_merge(float* out, const float* in, int n, hipStream_t s);
int launch_mlp16(float* x, void* xn_out, int dt, const void* wpack, const float* b1f, const float* b2, int64_t M, int E,
                 float eps, hipStream_t s);
// out-projection + residual + LayerNorm2 + MLP + residual (+ next normalise) in one launch (k_block16.hip); attn may alias xn_out
size_t block16_scratch_bytes(void);
int launch_block16(float* x, const void* attn, void* xn_out, int dt, const void* wproj, const float* bproj, const void* wpack,
                   const float* b1f, const float* b2, void* scratch, int64_t M, int E, float eps, hipStream_t s);
// the same in the single-role form (k_block16s.hip): weights as one stream in consumption order, no scratch
int launch_block16s(float* x, const void* attn, void* xn_out, int dt, const void* wseq, const float* b1f, const float* bproj,
                    const float* b2, int64_t M, int E, float eps, int layout, hipStream_t s);
// log2q: q arrives pre-multiplied by log2(e) as well (the encoder folds it into the QKV epilogue's fp32 q scaling, so no
// second 16-bit rounding of q); 0 = plain head_dim^-0.5 scaling, the public mst_attention* contract
// out_blocked: out in the 16-bit blocked layout of include/mst_hip.h (rows = seq * N + q; whole 32-row groups allocated)
int launch_attn16(const void* qkv, int dt, int n_seq, int N, int heads, void* out, int log2q, hipStream_t s, int out_blocked = 0);
int launch_attn32(const float* qkv, int n_seq, int N, int heads, float* out, hipStream_t s);
int launch_cls_attn(const void* qkv, int dt, int n_seq, int N, int heads, float* probs, void* out, int log2q, hipStream_t s);
int launch_cls_probs(const void* qkv, int dt, int n_seq, int N, int heads, int hd, float* probs, int log2q,
                     hipStream_t s);
int launch_probs_full(const void* qkv, int dt, int n_seq, int N, int heads, int hd, float* probs, int log2q,
                      hipStream_t s);
int launch_patch_embed(const void* vol, int idt, int n, int H, int W, const void* wp, int dt,
                       const float* bias, const float* prefix, int n_prefix, const float* pos_patch,
                       int E, float* x, hipStream_t s);
int launch_pos_interp(const float* pos, int M, int E, int gh, int gw, double offset, int antialias, float* out,
                      hipStream_t s);
// encoder API (k_features.hip): the patch embedding of true RGB images, wp [E][3][14][16] of dt; and the residual stream as fp32 plain
// rows, read from plain rows or (x_image) from the fp32 image of the blocked layout, through LayerNorm(g, b, eps) unless g is null
int launch_patch_embed_rgb(const void* img, int idt, int n, int H, int W, const void* wp, int dt, const float* bias, const float* prefix,
                           int n_prefix, const float* pos_patch, int E, float* x, hipStream_t s);
int launch_tap_rows(const float* x, int x_image, const float* g, const float* b, float* out, int64_t rows, int cols, float eps, hipStream_t s);
int launch_slice_tokens(const float* emb, const float* cls, const float* pos, int B, int D, int E,
                        float* xs, hipStream_t s);
int launch_slice_attn(const float* qkv, int B, int L, int heads, int hd, const uint8_t* mask,
                      const float* rope, const float* liere, float* out, float* probs, hipStream_t s);
int launch_liere_rotation(const float* vars, int n_blocks, int n, int P, float* R, hipStream_t s);
int launch_rows_copy(const float* src, int64_t src_stride, float* dst, int64_t dst_stride, int rows,
                     int cols, hipStream_t s);
int launch_saliency_accumulate(const float* maps, const float* slice_attn, int D, int heads, int gh, int gw, int Np,
                               int flip_mask, int accumulate, float* low, float* slice_acc, hipStream_t s);
int launch_saliency_upsample(const float* low, int D, int gh, int gw, float scale, int Dout, int H, int W, float* out,
                             hipStream_t s);
// folded test-time augmentation (k_tta.hip)
int launch_tta_inplane_flips(const void* x, int dt, int n, int H, int W, void* out, hipStream_t s);
int launch_saliency_accumulate_tta(const float* plane, const float* slice_attn, int D, int heads, int gh, int gw, int Np,
                                   float* low, float* slice_acc, hipStream_t s);
int launch_bmm32_nn(const float* A, const float* B, float* C, int64_t batch, int M, int N, int K, hipStream_t s);
// training step (k_train.hip)
int launch_gemm_ex(const float* A, const float* B, float* C, int M, int N, int K, int64_t sam, int64_t sak, int64_t sbk, int64_t sbn,
                   int64_t scm, int64_t scn, int nb1, int nb2, int64_t sa1, int64_t sa2, int64_t sb1, int64_t sb2, int64_t sc1,
                   int64_t sc2, float alpha, float beta, hipStream_t s);
int launch_softmax_rows(float* S, const uint8_t* mask, int64_t rows, int L, int rows_per_b, hipStream_t s);
int launch_softmax_rows_bwd(const float* P, float* dP, int64_t rows, int L, float scale, hipStream_t s);
int launch_layernorm_bwd(const float* x, int64_t xs, const float* gamma, const float* dy, int64_t dys, const float* dres, int64_t drs,
                         float* dx, int64_t dxs, float* dgamma, float* dbeta, int64_t rows, int cols, float eps, hipStream_t s);
int launch_act_fwd(const float* h, float* y, int64_t n, int kind, hipStream_t s);
int launch_act_bwd(const float* h, float* dy, int64_t n, int kind, hipStream_t s);
int launch_swiglu_fwd(const float* x12, float* h, int64_t rows, int H, hipStream_t s);
int launch_swiglu_bwd(const float* x12, const float* dh, float* dx12, int64_t rows, int H, hipStream_t s);
int launch_colsum(const float* a, int64_t as, const float* b, int64_t bs, int64_t rows, int cols, float* out, hipStream_t s);
int launch_axpby_cols(const float* x, int64_t xs, const float* g, float alpha, float beta, float* y, int64_t ys, int64_t rows,
                      int cols, hipStream_t s);
int launch_im2col14(const void* vol, int dt, int n, int H, int W, float* col, hipStream_t s);
int launch_pos_interp_bwd(const float* dout, int M, int E, int gh, int gw, double offset, float* dpos, hipStream_t s);
int launch_patch_embed_dgrad(const float* dx, int tok, int first, const float* wsum, int C, int n, int H, int W, int E, float* dvol,
                             hipStream_t s);   // k_patch_dgrad.hip: C = 1 grey (wsum [E][224]), C = 3 RGB (the kernel image [E][3][224])
// k_features.hip: partial weight gradients of the RGB patch embedding, part [ceil(n Np / rows_per_split)][E][3][14][14]
int launch_patch_embed_rgb_wgrad(const float* dx, int tok, int first, const float* img, int n, int H, int W, int E, int rows_per_split,
                                 float* part, hipStream_t s);
// convolutional backbone (k_conv.hip)
int launch_im2col_nhwc(const float* x, int n, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad, float* col,
                       hipStream_t s);
int launch_col2im_nhwc(const float* dcol, int n, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad, float* dx,
                       hipStream_t s);
// pooling (k_bn.hip, beside the BatchNorm entry points); x of type dt
int launch_maxpool_nhwc(const void* x, int dt, int n, int H, int W, int C, void* y, hipStream_t s);
int launch_avgpool_nhwc(const void* x, int dt, int n, int HW, int C, float* y, hipStream_t s);
int launch_maxpool_bwd_nhwc(const float* x, const float* dy, int n, int H, int W, int C, float* dx, hipStream_t s);
int launch_avgpool_bwd_nhwc(const float* dy, int n, int HW, int C, float* dx, hipStream_t s);
int launch_gradcampp(const float* act, const float* out, int O, const float* W, int n, int HW, int C, float* cam, float* state,
                     hipStream_t s);
size_t znorm_state_bytes(void);
int launch_pad_axis(float* v, int n0, int n1, int n2, int axis, int lo, int hi, int a0, int a1, int b0, int b1, int use_const,
                    float cval, hipStream_t s);
int launch_copy_block(const float* src, int sn1, int sn2, int s0, int s1, int s2, float* dst, int dn1, int dn2, int d0, int d1,
                      int d2, int c0, int c1, int c2, hipStream_t s);
int launch_znorm(const float* x, int64_t n, float q_lo, float q_hi, float* y, void* state, hipStream_t s);
// training augmentation (k_augment.hip): in / out of types idt / odt, params [n, 8] fp32; the per-volume minimum to out[v * stride]
int launch_augment_volumes(const void* in, int idt, void* out, int odt, int n, int D, int H, int W, const float* params, uint64_t seed,
                           uint64_t counter, hipStream_t s);
int launch_volume_min(const void* x, int dt, int n, int64_t elems, float* out, int stride, hipStream_t s);
// fixed-order reductions (k_colsum.hip, k_ordered.hip, and the ordered forms in k_train.hip / k_bn.hip / k_input.hip): bit-reproducible for fixed
// shape arguments, no floating-point atomics
size_t colsum_ordered_workspace_bytes(int64_t rows, int cols, int outputs, int ty = 16);
int launch_slab_reduce(const float* slab, int64_t nrb, int64_t width, int64_t split, float* o0, float* o1, hipStream_t s);
int launch_colsum_ordered(const float* a, int64_t as, const float* b, int64_t bs, int64_t rows, int cols, float* out, void* ws,
                          size_t ws_bytes, hipStream_t s);
// the column sums of BatchNorm on z [rows, C] of type dt (k_colsum.hip): COL_SUM out0 += sum z; COL_SQDEV out0 += sum (z - mean)^2;
// COL_BN_BWD out0 += sum g (z - mean) rstd, out1 += sum g with g = dy (y > 0 ? 1 : 0), y (of z's type, 16-bit only) nullable.  ordered: in
// fixed order through ws; otherwise by atomics (fp32 z only).  A 16-bit z: C % 8 == 0 and 16-byte aligned operands.
enum { COL_SUM = 0, COL_SQDEV = 1, COL_BN_BWD = 2 };
int launch_bn_reduce(int op, const void* z, int dt, const void* y, const float* dy, const float* mean, const float* rstd, int64_t rows, int C,
                     float* out0, float* out1, bool ordered, void* ws, size_t ws_bytes, hipStream_t s);
// the row blocks of a column sum whose workgroup has `ty` thread rows
void colsum_plan(int64_t rows, int cols, int ty, int64_t& rpb, int64_t& rblocks);
int launch_col2im_gather(const float* dcol, int n, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad, float* dx,
                         hipStream_t s);
size_t maxpool_bwd_gather_workspace_bytes(int n, int H, int W, int C);
int launch_maxpool_bwd_gather(const char* what, const void* x, int dt, const float* dy, int n, int H, int W, int C, float* dx, void* ws,
                              size_t ws_bytes, hipStream_t s);
size_t pos_interp_bwd_ordered_workspace_bytes(int M, int E, int gh, int gw);
int launch_pos_interp_bwd_ordered(const float* dout, int M, int E, int gh, int gw, double offset, float* dpos, void* ws, size_t ws_bytes,
                                  hipStream_t s);
size_t layernorm_bwd_ordered_workspace_bytes(int64_t rows, int cols);
int launch_layernorm_bwd_ordered(const float* x, int64_t xs, const float* gamma, const float* dy, int64_t dys, const float* dres, int64_t drs,
                                 float* dx, int64_t dxs, float* dgamma, float* dbeta, int64_t rows, int cols, float eps, void* ws,
                                 size_t ws_bytes, hipStream_t s);
size_t znorm_ordered_workspace_bytes(int64_t n);
int launch_znorm_ordered(const float* x, int64_t n, float q_lo, float q_hi, float* y, void* state, void* ws, size_t ws_bytes, hipStream_t s);
int launch_slices2rgb(const void* vol, int dt, int B, int D, int H, int W, void* out, hipStream_t s);
int launch_mean_slices(const float* x, int B, int D, int E, float* out, hipStream_t s);
int launch_readout(const float* cls_probs, const float* slice_probs, int B, int D, int heads, int N,
                   int R, int sheads, float* plane, float* slice_attn, float* maps, hipStream_t s);
