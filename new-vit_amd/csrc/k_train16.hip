// Row kernels of the training step's 16-bit storage mode (mst/train.py, train_storage='16bit'): what the reference's autocast does to the
// tensors a block keeps for its backward (Trainer(precision='16-mixed'), scripts/main_train.py:110-123; block.py:89-114) -- the LayerNorm
// outputs, the attention output, the branch outputs and the MLP's hidden activations live in the 16-bit type T, the residual stream and
// every gradient stay fp32.  All of these are bandwidth kernels: every byte moves once, in 16-byte accesses (4 fp32 or 8 T per lane).
//   residual_layernorm16   x_out = x_in + gamma o float(br_T)  (fp32, one rounding),  y_T = LayerNorm(x_out)     one wave per row
//   act_fwd16 / act_bwd16  y_T = act(float(h_T));  dy (fp32, in place) *= act'(float(h_T))                      the formulas of k_train.hip
//   colsum_b16 (+ ordered) out[c] += sum_r a[r][c] * float(b_T[r][c])   the LayerScale gradient: the thread layouts and summation orders of
//                          colsum_kernel (k_train.hip) and ocolsum_kernel (k_ordered.hip), so the ordered form returns the bits of
//                          mst_colsum_ordered on the upcast factor
//   transpose16            T [rows, cols] -> T [cols, rows_pad], zero columns past rows: the 16-bit-input twin of cvt16's transposed form
#include "mst_common.h"

namespace {

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

// One wave per row, four rows per workgroup (the layout of layernorm_kernel); lane l owns columns 512 j + 8 l .. + 7.  Statistics as there:
// mean, then the variance of the centred values, by wave shuffles.  Contiguous rows of `cols` (a multiple of 8) elements.
template <int NJ, typename T>
__global__ __launch_bounds__(256) void residual_layernorm16_kernel(const float* __restrict__ xin, const T* __restrict__ br,
                                                                   const float* __restrict__ gamma, float* __restrict__ xout,
                                                                   const float* __restrict__ w, const float* __restrict__ b, T* __restrict__ y,
                                                                   int64_t rows, int cols, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t off = row * cols;
    float v[NJ][8];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = j * 512 + lane * 8;
        if (c < cols) {
            float r[8], g[8];
            load8(xin + off + c, v[j]);
            load8(br + off + c, r);
            if (gamma) load8(gamma + c, g);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                v[j][e] = gamma ? fmaf(g[e], r[e], v[j][e]) : v[j][e] + r[e];
                s += v[j][e];
            }
            store8(xout + off + c, v[j]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[j][e] = 0.f;
        }
    }
    if (!y) return;
    const float inv_n = 1.0f / (float)cols;
    const float mean = wave_sum(s) * inv_n;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (j * 512 + lane * 8 < cols) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = v[j][e] - mean;
                q = fmaf(d, d, q);
            }
        }
    }
    const float rstd = rsqrtf(wave_sum(q) * inv_n + eps);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = j * 512 + lane * 8;
        if (c < cols) {
            float ww[8], bb[8], o[8];
            load8(w + c, ww);
            load8(b + c, bb);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (v[j][e] - mean) * rstd * ww[e] + bb[e];
            store8(y + off + c, o);
        }
    }
}

// the derivative of act_bwd_kernel (k_train.hip), the same fp32 expression
__device__ __forceinline__ float act_deriv(float v, int kind) {
    if (kind == 0) return 0.5f * (1.0f + erff(v * 0.70710678118654752440f)) + v * 0.3989422804014327f * expf(-0.5f * v * v);
    return v > 0.f ? 1.f : 0.f;
}

// groups of 8 elements, then threads 0 .. n % 8 - 1 of the grid take the ragged tail one element each
template <typename T>
__global__ __launch_bounds__(256) void act_fwd16_kernel(const T* __restrict__ h, T* __restrict__ y, int64_t n, int kind) {
    const int64_t n8 = n >> 3, gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = gid; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
        float v[8];
        load8(h + 8 * i, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = f32_rounded(kind == 0 ? gelu_erf(v[e]) : fmaxf(v[e], 0.f));   // the bits of T(mst_act_fwd)
        store8(y + 8 * i, v);
    }
    if (gid < (n & 7)) {
        const float v = (float)h[8 * n8 + gid];
        y[8 * n8 + gid] = (T)f32_rounded(kind == 0 ? gelu_erf(v) : fmaxf(v, 0.f));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void act_bwd16_kernel(const T* __restrict__ h, float* __restrict__ dy, int64_t n, int kind) {
    const int64_t n8 = n >> 3, gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = gid; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
        float v[8], d[8];
        load8(h + 8 * i, v);
        load8(dy + 8 * i, d);
#pragma unroll
        for (int e = 0; e < 8; ++e) d[e] *= act_deriv(v[e], kind);
        store8(dy + 8 * i, d);
    }
    if (gid < (n & 7)) dy[8 * n8 + gid] *= act_deriv((float)h[8 * n8 + gid], kind);
}

// SwiGLU on rows x12 = [x1 | x2] of 2 H elements of T (swiglu_fwd_kernel / swiglu_bwd_kernel of k_train.hip, the same fp32 expressions):
// V = 8 columns per thread in 16-byte accesses when H % 8 == 0 (every half row is then 16-byte aligned), one column per thread otherwise.
template <typename T, int V>
__global__ __launch_bounds__(256) void swiglu_fwd16_kernel(const T* __restrict__ x12, T* __restrict__ h, int64_t rows, int H) {
    const int hv = H / V;
    const int64_t n = rows * hv;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / hv;
        const int c = (int)(i - r * hv) * V;
        const T* x = x12 + r * 2 * H + c;
        if constexpr (V == 8) {
            float a[8], b[8];
            load8(x, a);
            load8(x + H, b);
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] = f32_rounded(swiglu_fwd_value(a[e], b[e]));          // the bits of T(mst_swiglu_fwd)
            store8(h + r * H + c, a);
        } else {
            h[r * H + c] = (T)f32_rounded(swiglu_fwd_value((float)x[0], (float)x[H]));
        }
    }
}

template <typename T, int V>
__global__ __launch_bounds__(256) void swiglu_bwd16_kernel(const T* __restrict__ x12, const float* __restrict__ dh, float* __restrict__ dx12,
                                                           int64_t rows, int H) {
    const int hv = H / V;
    const int64_t n = rows * hv;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / hv;
        const int c = (int)(i - r * hv) * V;
        const int64_t o = r * 2 * H + c;
        if constexpr (V == 8) {
            float a[8], b[8], d[8], d1[8], d2[8];
            load8(x12 + o, a);
            load8(x12 + o + H, b);
            load8(dh + r * H + c, d);
#pragma unroll
            for (int e = 0; e < 8; ++e) swiglu_bwd_values(a[e], b[e], d[e], &d1[e], &d2[e]);
            store8(dx12 + o, d1);
            store8(dx12 + o + H, d2);
        } else {
            float d1, d2;
            swiglu_bwd_values((float)x12[o], (float)x12[o + H], dh[r * H + c], &d1, &d2);
            dx12[o] = d1;
            dx12[o + H] = d2;
        }
    }
}

// colsum_kernel<VEC = true> of k_train.hip with a 16-bit factor: 16 threads x 4 columns across, 16 thread rows down the chunk, one atomic
// per column per workgroup.
template <typename T>
__global__ __launch_bounds__(256) void colsum_b16_kernel(const float* __restrict__ a, int64_t as, const T* __restrict__ b, int64_t bs, int64_t rows,
                                                         int cols, int rows_per_block, float* __restrict__ out) {
    __shared__ float red[16][64 + 4];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    const int c = blockIdx.y * 64 + tx * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (c < cols) {
        for (int64_t r = r0 + ty; r < r1; r += 16) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(a + r * as + c);
            const typename V8<T>::half_type bv = *reinterpret_cast<const typename V8<T>::half_type*>(b + r * bs + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(av[e], (float)bv[e], acc[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[ty][tx * 4 + e] = acc[e];
    __syncthreads();
    if (threadIdx.x < 64) {
        const int cc = blockIdx.y * 64 + threadIdx.x;
        float t = 0.f;
#pragma unroll
        for (int y = 0; y < 16; ++y) t += red[y][threadIdx.x];
        if (cc < cols) atomicAdd(out + cc, t);
    }
}

// ocolsum_kernel<OP_SUM> of k_ordered.hip with a 16-bit factor: the same owner of every element, the same order of every sum (row
// r0 + ty + 16 k in sequence per thread, the 16 thread rows in ascending ty), one plain store per column into slab[rb] -- or out += with
// one row block.
template <typename T>
__global__ __launch_bounds__(256) void ocolsum_b16_kernel(const float* __restrict__ a, int64_t as, const T* __restrict__ b, int64_t bs, int64_t rows,
                                                          int cols, int64_t rpb, int cblocks, float* o0, int64_t ostride, int direct) {
    __shared__ float red[16][64 + 4];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t rb = blockIdx.x / cblocks;
    const int cb = (int)(blockIdx.x - rb * cblocks);
    const int64_t r0 = rb * rpb, r1 = r0 + rpb < rows ? r0 + rpb : rows;
    const int c0 = cb * 64 + tx * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (c0 < cols) {
        for (int64_t r = r0 + ty; r < r1; r += 16) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(a + r * as + c0);
            const typename V8<T>::half_type bv = *reinterpret_cast<const typename V8<T>::half_type*>(b + r * bs + c0);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(av[e], (float)bv[e], acc[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[ty][tx * 4 + e] = acc[e];
    __syncthreads();
    if (threadIdx.x < 64) {
        const int cc = cb * 64 + threadIdx.x;
        float t = 0.f;
#pragma unroll
        for (int y = 0; y < 16; ++y) t += red[y][threadIdx.x];
        if (cc < cols) {
            float* p = o0 + rb * ostride + cc;
            *p = direct ? *p + t : t;
        }
    }
}

// out[c][r] = x[r][c] (r < rows), 0 (rows <= r < rows_pad): 64 x 64 tiles through LDS, 128-byte row segments in and out
template <typename T>
__global__ __launch_bounds__(256) void transpose16_kernel(const T* __restrict__ x, int64_t ldx, int64_t rows, int cols, T* __restrict__ out,
                                                          int64_t ldo, int64_t rows_pad) {
    __shared__ T tile[64][64 + 2];
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    const int c0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int rr = ty + 4 * i;
        const int64_t r = r0 + rr;
        tile[rr][tx] = (r < rows && c0 + tx < cols) ? x[r * ldx + c0 + tx] : (T)0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int cc = ty + 4 * i;
        const int64_t r = r0 + tx;
        if (c0 + cc < cols && r < rows_pad) out[(int64_t)(c0 + cc) * ldo + r] = tile[tx][cc];
    }
}

inline unsigned grid8(int64_t n) {                                  // one thread per 8 elements, at least one workgroup (the tail)
    const int64_t g = ((n >> 3) + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <typename T>
int residual_ln16_t(const float* xin, const void* br, const float* gamma, float* xout, const float* w, const float* b, void* y, int64_t rows,
                    int cols, float eps, hipStream_t s) {
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    const T* r = (const T*)br;
    T* o = (T*)y;
    if (cols <= 512) residual_layernorm16_kernel<1, T><<<grid, block, 0, s>>>(xin, r, gamma, xout, w, b, o, rows, cols, eps);
    else if (cols <= 1024) residual_layernorm16_kernel<2, T><<<grid, block, 0, s>>>(xin, r, gamma, xout, w, b, o, rows, cols, eps);
    else residual_layernorm16_kernel<4, T><<<grid, block, 0, s>>>(xin, r, gamma, xout, w, b, o, rows, cols, eps);
    return mst_check_launch("residual_layernorm16");
}

}  // namespace

int launch_residual_layernorm16(const float* xin, const void* br, int dt, const float* gamma, float* xout, const float* w, const float* b,
                                void* y, int64_t rows, int cols, float eps, hipStream_t s) {
    MST_CHECK_ARG(dt == MST_BF16 || dt == MST_F16, "residual_layernorm16: dtype %d (bf16 / f16)", dt);
    MST_CHECK_ARG(cols > 0 && cols <= 2048 && cols % 8 == 0, "residual_layernorm16: cols=%d must be a multiple of 8 and <= 2048", cols);
    MST_CHECK_ARG(rows > 0 && (rows + 3) / 4 < (1ll << 31), "residual_layernorm16: rows=%lld out of range", (long long)rows);
    MST_CHECK_ARG(aligned(xin, 16) && aligned(br, 16) && aligned(xout, 16) && aligned(gamma, 16) && aligned(w, 16) && aligned(b, 16) && aligned(y, 16),
                  "residual_layernorm16: bases must be 16-byte aligned");
    if (dt == MST_BF16) return residual_ln16_t<bf16_t>(xin, br, gamma, xout, w, b, y, rows, cols, eps, s);
    return residual_ln16_t<f16_t>(xin, br, gamma, xout, w, b, y, rows, cols, eps, s);
}

int launch_act_fwd16(const void* h, void* y, int dt, int64_t n, int kind, hipStream_t s) {
    MST_CHECK_ARG(aligned(h, 16) && aligned(y, 16), "act_fwd16: bases must be 16-byte aligned");
    if (dt == MST_BF16) act_fwd16_kernel<bf16_t><<<dim3(grid8(n)), dim3(256), 0, s>>>((const bf16_t*)h, (bf16_t*)y, n, kind);
    else if (dt == MST_F16) act_fwd16_kernel<f16_t><<<dim3(grid8(n)), dim3(256), 0, s>>>((const f16_t*)h, (f16_t*)y, n, kind);
    else { mst_set_error("act_fwd16: dtype %d (bf16 / f16)", dt); return MST_EINVAL; }
    return mst_check_launch("act_fwd16");
}

int launch_act_bwd16(const void* h, int dt, float* dy, int64_t n, int kind, hipStream_t s) {
    MST_CHECK_ARG(aligned(h, 16) && aligned(dy, 16), "act_bwd16: bases must be 16-byte aligned");
    if (dt == MST_BF16) act_bwd16_kernel<bf16_t><<<dim3(grid8(n)), dim3(256), 0, s>>>((const bf16_t*)h, dy, n, kind);
    else if (dt == MST_F16) act_bwd16_kernel<f16_t><<<dim3(grid8(n)), dim3(256), 0, s>>>((const f16_t*)h, dy, n, kind);
    else { mst_set_error("act_bwd16: dtype %d (bf16 / f16)", dt); return MST_EINVAL; }
    return mst_check_launch("act_bwd16");
}

template <typename T>
static int swiglu16_t(const void* x12, void* h, const float* dh, float* dx12, int64_t rows, int H, hipStream_t s) {
    const bool vec = H % 8 == 0;
    const int64_t n = rows * (vec ? H / 8 : H);
    const int64_t g = (n + 255) / 256;
    const dim3 grid((unsigned)(g > 16384 ? 16384 : g)), block(256);
    if (h) {
        if (vec) swiglu_fwd16_kernel<T, 8><<<grid, block, 0, s>>>((const T*)x12, (T*)h, rows, H);
        else swiglu_fwd16_kernel<T, 1><<<grid, block, 0, s>>>((const T*)x12, (T*)h, rows, H);
        return mst_check_launch("swiglu_fwd16");
    }
    if (vec) swiglu_bwd16_kernel<T, 8><<<grid, block, 0, s>>>((const T*)x12, dh, dx12, rows, H);
    else swiglu_bwd16_kernel<T, 1><<<grid, block, 0, s>>>((const T*)x12, dh, dx12, rows, H);
    return mst_check_launch("swiglu_bwd16");
}

int launch_swiglu_fwd16(const void* x12, void* h, int dt, int64_t rows, int H, hipStream_t s) {
    MST_CHECK_ARG(aligned(x12, 16) && aligned(h, 16), "swiglu_fwd16: bases must be 16-byte aligned");
    if (dt == MST_BF16) return swiglu16_t<bf16_t>(x12, h, nullptr, nullptr, rows, H, s);
    if (dt == MST_F16) return swiglu16_t<f16_t>(x12, h, nullptr, nullptr, rows, H, s);
    mst_set_error("swiglu_fwd16: dtype %d (bf16 / f16)", dt);
    return MST_EINVAL;
}

int launch_swiglu_bwd16(const void* x12, int dt, const float* dh, float* dx12, int64_t rows, int H, hipStream_t s) {
    MST_CHECK_ARG(aligned(x12, 16) && aligned(dh, 16) && aligned(dx12, 16), "swiglu_bwd16: bases must be 16-byte aligned");
    if (dt == MST_BF16) return swiglu16_t<bf16_t>(x12, nullptr, dh, dx12, rows, H, s);
    if (dt == MST_F16) return swiglu16_t<f16_t>(x12, nullptr, dh, dx12, rows, H, s);
    mst_set_error("swiglu_bwd16: dtype %d (bf16 / f16)", dt);
    return MST_EINVAL;
}

static int colsum_b16_args(const char* what, const float* a, int64_t as, const void* b, int dt, int64_t bs, int64_t rows, int cols) {
    MST_CHECK_ARG(dt == MST_BF16 || dt == MST_F16, "%s: dtype %d (bf16 / f16)", what, dt);
    MST_CHECK_ARG(rows > 0 && cols > 0, "%s: rows=%lld cols=%d out of range", what, (long long)rows, cols);
    MST_CHECK_ARG(cols % 4 == 0 && as % 4 == 0 && bs % 4 == 0 && as >= cols && bs >= cols && aligned(a, 16) && aligned(b, 8),
                  "%s: cols=%d and the row strides must be multiples of 4 (strides >= cols), a 16-byte and b 8-byte aligned", what, cols);
    return MST_OK;
}

int launch_colsum_b16(const float* a, int64_t as, const void* b, int dt, int64_t bs, int64_t rows, int cols, float* out, hipStream_t s) {
    if (int rc = colsum_b16_args("colsum_b16", a, as, b, dt, bs, rows, cols)) return rc;
    const int cblocks = (cols + 63) / 64;
    MST_CHECK_ARG(cblocks <= 65535, "colsum_b16: cols=%d out of range", cols);
    int64_t rpb = (rows * cblocks + 2047) / 2048;                   // the plan of launch_colsum
    rpb = rpb < 64 ? 64 : (rpb + 15) / 16 * 16;
    const int64_t rblocks = (rows + rpb - 1) / rpb;
    MST_CHECK_ARG(rblocks < (1ll << 31) && rpb < (1ll << 31), "colsum_b16: rows=%lld out of range", (long long)rows);
    const dim3 grid((unsigned)rblocks, cblocks);
    if (dt == MST_BF16) colsum_b16_kernel<bf16_t><<<grid, dim3(256), 0, s>>>(a, as, (const bf16_t*)b, bs, rows, cols, (int)rpb, out);
    else colsum_b16_kernel<f16_t><<<grid, dim3(256), 0, s>>>(a, as, (const f16_t*)b, bs, rows, cols, (int)rpb, out);
    return mst_check_launch("colsum_b16");
}

int launch_colsum_b16_ordered(const float* a, int64_t as, const void* b, int dt, int64_t bs, int64_t rows, int cols, float* out, void* ws,
                              size_t ws_bytes, hipStream_t s) {
    if (int rc = colsum_b16_args("colsum_b16_ordered", a, as, b, dt, bs, rows, cols)) return rc;
    const int64_t cblocks = (cols + 63) / 64;
    int64_t rpb = (rows * cblocks + 2047) / 2048;                   // the plan of mst_colsum_ordered (ocolsum_plan)
    rpb = rpb < 64 ? 64 : (rpb + 15) / 16 * 16;
    const int64_t rblocks = (rows + rpb - 1) / rpb;
    MST_CHECK_ARG(rblocks * cblocks < (1ll << 31), "colsum_b16_ordered: rows=%lld cols=%d out of range", (long long)rows, cols);
    const size_t need = colsum_ordered_workspace_bytes(rows, cols, 1);
    MST_CHECK_ARG(ws_bytes >= need && (need == 0 || ws), "colsum_b16_ordered: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const int direct = rblocks == 1;
    float* o0 = direct ? out : (float*)ws;
    const dim3 grid((unsigned)(rblocks * cblocks));
    if (dt == MST_BF16) ocolsum_b16_kernel<bf16_t><<<grid, dim3(256), 0, s>>>(a, as, (const bf16_t*)b, bs, rows, cols, rpb, (int)cblocks, o0, cols, direct);
    else ocolsum_b16_kernel<f16_t><<<grid, dim3(256), 0, s>>>(a, as, (const f16_t*)b, bs, rows, cols, rpb, (int)cblocks, o0, cols, direct);
    int rc = mst_check_launch("colsum_b16_ordered");
    if (rc || direct) return rc;
    return launch_slab_reduce((const float*)ws, rblocks, cols, cols, out, nullptr, s);
}

int launch_transpose16(const void* x, int dt, int64_t ldx, int64_t rows, int cols, void* out, int64_t ldo, int64_t rows_pad, hipStream_t s) {
    MST_CHECK_ARG(x && out && rows > 0 && cols > 0 && ldx >= cols, "transpose16: bad arguments");
    MST_CHECK_ARG(dt == MST_BF16 || dt == MST_F16, "transpose16: dtype %d (bf16 / f16)", dt);
    MST_CHECK_ARG(rows_pad >= rows && ldo >= rows_pad, "transpose16: rows_pad=%lld ldo=%lld", (long long)rows_pad, (long long)ldo);
    const dim3 grid((unsigned)((rows_pad + 63) / 64), (cols + 63) / 64);
    MST_CHECK_ARG((rows_pad + 63) / 64 < (1ll << 31) && grid.y <= 65535, "transpose16: rows_pad=%lld cols=%d out of range", (long long)rows_pad, cols);
    if (dt == MST_BF16) transpose16_kernel<bf16_t><<<grid, dim3(256), 0, s>>>((const bf16_t*)x, ldx, rows, cols, (bf16_t*)out, ldo, rows_pad);
    else transpose16_kernel<f16_t><<<grid, dim3(256), 0, s>>>((const f16_t*)x, ldx, rows, cols, (f16_t*)out, ldo, rows_pad);
    return mst_check_launch("transpose16");
}
