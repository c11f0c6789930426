// BatchNorm / pooling kernels of the ResNet training step's 16-bit storage mode (mst/train_resnet.py, train_storage='16bit'): what the
// reference's autocast does to a convolution + BatchNorm2d + ReLU unit (Trainer(precision='16-mixed'), scripts/main_train.py:110-123) --
// the convolution output z and the unit's output y live in the 16-bit type T, the statistics, the gradient stream and every sum are fp32.
// All of these are bandwidth kernels.  Activations are [rows, C] NHWC with C % 8 == 0 and 16-byte aligned bases:
//   layout      a workgroup of 256 lanes owns 64 columns x one block of rows; lane (tx = lane & 7, ty = lane >> 3) owns the 8 channels
//               64 cb + 8 tx .. + 7 (ONE 16-byte T access, two 16-byte fp32 accesses) of rows r0 + ty + 32 k.  The per-channel vectors
//               are read once per lane before the row loop; the only integer division is blockIdx.x / cblocks, once per workgroup.
//   plan        row blocks of ceil(rows * cblocks / 2,048) rows (at least 64, a multiple of 32): about 2,048 workgroups at most, each
//               striding over its rows.  A pure function of (rows, C).
//   reductions  no floating-point atomics: a lane sums its rows in ascending order, the 32 row lanes meet in LDS in ascending ty, ONE
//               plain store per column goes to slab[rb], and slab_reduce (k_colsum.hip) adds the row blocks in ascending order.
//               Bit-reproducible for fixed (rows, C), whatever the determinism flag says.
//   rounding    an fp32 result goes through f32_rounded before its conversion: the stored bits are T(the fp32 value).
//   bn16_reduce      SUM: sum_r z;  SQDEV: sum_r (z - mean)^2;  BWD: d gamma = sum_r m dy xhat, d beta = sum_r m dy  (m = y > 0)
//   bn16_apply       y = T(relu?(gamma (z - mean) rstd + beta + float(residual)))                 the expression of bn_apply_kernel
//   bn16_bwd_apply   dz = T(gamma rstd (m dy - d beta / rows - xhat d gamma / rows)), dy <- m dy on request   (bn_bwd_apply_kernel)
//   maxpool_arg16    pass 1 of the gather-form max-pool backward (k_ordered.hip) on a T input: the same first-maximum codes
//   avgpool16        y[n][c] = (sum over positions in ascending order of float(x)) / HW           the order of avgpool_nhwc_kernel
#include "mst_common.h"

namespace {

// This file's own load8 / store8 (they hide mst_common.h's here): the 16-bit store8 rounds inside, through f32_rounded.
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
    for (int e = 0; e < 8; ++e) t[e] = (T)f32_rounded(v[e]);       // round to nearest even, of the fp32 value as computed
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

// the block of rows and the 8 channels of this lane
struct Tile {
    int64_t r0, r1, rb;
    int c0, cb, ty;
};
__device__ __forceinline__ Tile tile_of(int64_t rows, int64_t rpb, int cblocks) {
    Tile t;
    t.rb = blockIdx.x / cblocks;
    t.cb = (int)(blockIdx.x - t.rb * cblocks);
    t.r0 = t.rb * rpb;
    t.r1 = t.r0 + rpb < rows ? t.r0 + rpb : rows;
    t.c0 = t.cb * 64 + (threadIdx.x & 7) * 8;
    t.ty = threadIdx.x >> 3;
    return t;
}

enum { R_SUM = 0, R_SQDEV = 1, R_BWD = 2 };

// slab[rb][j][c] = this row block's sum j of column c (j: R_BWD has d gamma, then d beta; one sum otherwise)
template <int OP, typename T>
__global__ __launch_bounds__(256) void bn16_reduce_kernel(const T* __restrict__ z, const T* __restrict__ y, const float* __restrict__ dy,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd, int64_t rows, int C,
                                                          int64_t rpb, int cblocks, float* __restrict__ slab) {
    constexpr int NA = OP == R_BWD ? 2 : 1;
    __shared__ float red[NA][32][64 + 4];
    const Tile t = tile_of(rows, rpb, cblocks);
    float acc[NA][8], mc[8], rc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[0][e] = acc[NA - 1][e] = mc[e] = rc[e] = 0.f;
    if (t.c0 < C) {
        if (OP != R_SUM) load8(mean + t.c0, mc);
        if (OP == R_BWD) load8(rstd + t.c0, rc);
#pragma unroll 2
        for (int64_t r = t.r0 + t.ty; r < t.r1; r += 32) {
            const int64_t off = r * C + t.c0;
            float v[8];
            load8(z + off, v);
            if (OP == R_SUM) {
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[0][e] += v[e];
            } else if (OP == R_SQDEV) {
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float d = v[e] - mc[e]; acc[0][e] = fmaf(d, d, acc[0][e]); }
            } else {
                float g[8];
                load8(dy + off, g);
                if (y) {
                    float yy[8];
                    load8(y + off, yy);
#pragma unroll
                    for (int e = 0; e < 8; ++e) g[e] *= yy[e] > 0.f ? 1.f : 0.f;
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    acc[0][e] = fmaf(g[e], (v[e] - mc[e]) * rc[e], acc[0][e]);
                    acc[NA - 1][e] += g[e];
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NA; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) red[j][t.ty][(threadIdx.x & 7) * 8 + e] = acc[j][e];
    __syncthreads();
    if (threadIdx.x < 64 * NA) {
        const int j = threadIdx.x >> 6, cl = threadIdx.x & 63, cc = t.cb * 64 + cl;
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 32; ++q) s += red[j][q][cl];
        if (cc < C) slab[(t.rb * NA + j) * C + cc] = s;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bn16_apply_kernel(const T* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, const T* __restrict__ res,
                                                         int relu, int64_t rows, int C, int64_t rpb, int cblocks, T* __restrict__ y) {
    const Tile t = tile_of(rows, rpb, cblocks);
    if (t.c0 >= C) return;
    float mc[8], rc[8], gc[8], bc[8];
    load8(mean + t.c0, mc);
    load8(rstd + t.c0, rc);
    load8(gamma + t.c0, gc);
    load8(beta + t.c0, bc);
    for (int64_t r = t.r0 + t.ty; r < t.r1; r += 32) {
        const int64_t off = r * C + t.c0;
        float v[8];
        load8(z + off, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = gc[e] * (v[e] - mc[e]) * rc[e] + bc[e];
        if (res) {
            float a[8];
            load8(res + off, a);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += a[e];
        }
        if (relu) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        store8(y + off, v);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bn16_bwd_apply_kernel(const T* __restrict__ z, const T* __restrict__ y, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const float* __restrict__ gamma, float* dy,
                                                             int mask_in_place, const float* __restrict__ dgamma, const float* __restrict__ dbeta,
                                                             int64_t rows, int C, int64_t rpb, int cblocks, T* __restrict__ dz) {
    const Tile t = tile_of(rows, rpb, cblocks);
    if (t.c0 >= C) return;
    const float inv = 1.0f / (float)rows;
    float mc[8], rc[8], gc[8], dg[8], db[8];
    load8(mean + t.c0, mc);
    load8(rstd + t.c0, rc);
    load8(gamma + t.c0, gc);
    load8(dgamma + t.c0, dg);
    load8(dbeta + t.c0, db);
    for (int64_t r = t.r0 + t.ty; r < t.r1; r += 32) {
        const int64_t off = r * C + t.c0;
        float v[8], g[8];
        load8(z + off, v);
        load8(dy + off, g);
        if (y) {
            float yy[8];
            load8(y + off, yy);
#pragma unroll
            for (int e = 0; e < 8; ++e) g[e] *= yy[e] > 0.f ? 1.f : 0.f;
            if (mask_in_place) store8(dy + off, g);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xh = (v[e] - mc[e]) * rc[e];
            v[e] = gc[e] * rc[e] * (g[e] - db[e] * inv - xh * dg[e] * inv);
        }
        store8(dz + off, v);
    }
}

// arg[window][c] = ky * 3 + kx of the first maximum of the 3 x 3 / stride 2 / padding 1 window (scan order ky, kx, strict >: the rule of
// maxpool_arg_kernel), 255 when no element beats -inf.  One lane per window and 8 channels.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_arg16_kernel(const T* __restrict__ x, int H, int W, int C, int Ho, int Wo, int64_t groups,
                                                            uint8_t* __restrict__ arg) {
    const int c8 = C >> 3;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < groups; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t win = i / c8;
        const int c = (int)(i - win * c8) * 8;
        const int ox = (int)(win % Wo), oy = (int)((win / Wo) % Ho);
        const int64_t n = win / ((int64_t)Wo * Ho);
        float m[8];
        unsigned a[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { m[e] = -INFINITY; a[e] = 255u; }
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * 2 - 1 + ky;
            if (iy < 0 || iy >= H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * 2 - 1 + kx;
                if (ix < 0 || ix >= W) continue;
                float v[8];
                load8(x + ((n * H + iy) * W + ix) * C + c, v);
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (v[e] > m[e]) { m[e] = v[e]; a[e] = (unsigned)(ky * 3 + kx); }
            }
        }
        u32x2 o;
        o[0] = a[0] | a[1] << 8 | a[2] << 16 | a[3] << 24;
        o[1] = a[4] | a[5] << 8 | a[6] << 16 | a[7] << 24;
        *reinterpret_cast<u32x2*>(arg + win * C + c) = o;
    }
}

// y[n][c] = (sum_p float(x[n][p][c])) / HW, positions in ascending order: one workgroup per image, a lane per 8 channels
template <typename T>
__global__ __launch_bounds__(256) void avgpool16_kernel(const T* __restrict__ x, int HW, int C, float* __restrict__ y) {
    const int64_t n = blockIdx.x;
    for (int c = threadIdx.x * 8; c < C; c += blockDim.x * 8) {
        float s[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = 0.f;
#pragma unroll 4
        for (int p = 0; p < HW; ++p) {
            float v[8];
            load8(x + (n * HW + p) * C + c, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += v[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = s[e] / (float)HW;
        store8(y + n * C + c, s);
    }
}

inline size_t round256(size_t b) { return (b + 255) / 256 * 256; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

void bn16_plan(int64_t rows, int C, int64_t& rpb, int64_t& rblocks, int& cblocks) {
    cblocks = (C + 63) / 64;
    rpb = (rows * cblocks + 2047) / 2048;
    rpb = rpb < 64 ? 64 : (rpb + 31) / 32 * 32;
    rblocks = (rows + rpb - 1) / rpb;
}
inline size_t slab_bytes(int64_t rows, int C, int outputs) {
    int64_t rpb, rblocks;
    int cblocks;
    bn16_plan(rows, C, rpb, rblocks, cblocks);
    return round256(sizeof(float) * (size_t)rblocks * outputs * C);
}
inline size_t acc_bytes(int C) { return round256(sizeof(float) * (size_t)C); }

template <int OP, typename T>
int reduce16(const void* z, const void* y, const float* dy, const float* mean, const float* rstd, int64_t rows, int C, float* slab, float* o0,
             float* o1, const char* what, hipStream_t s) {
    constexpr int NA = OP == R_BWD ? 2 : 1;
    int64_t rpb, rblocks;
    int cblocks;
    bn16_plan(rows, C, rpb, rblocks, cblocks);
    bn16_reduce_kernel<OP, T><<<dim3((unsigned)(rblocks * cblocks)), dim3(256), 0, s>>>((const T*)z, (const T*)y, dy, mean, rstd, rows, C, rpb,
                                                                                      cblocks, slab);
    int rc = mst_check_launch(what);
    if (rc) return rc;
    return launch_slab_reduce(slab, rblocks, (int64_t)NA * C, C, o0, o1, s);      // o += : the caller zeroed them
}

template <typename T>
int train16(const void* z, int64_t rows, int C, const float* gamma, const float* beta, float eps, float momentum, const void* residual, int relu,
            void* y, float* mean, float* rstd, float* running_mean, float* running_var, void* ws, hipStream_t s) {
    float* acc = (float*)ws;                                            // C floats, then the slab of the column sums
    float* slab = (float*)((char*)ws + acc_bytes(C));
    if (hipMemsetAsync(acc, 0, sizeof(float) * C, s) != hipSuccess) { mst_set_error("batchnorm_train16: memset failed"); return MST_ELAUNCH; }
    int rc = reduce16<R_SUM, T>(z, nullptr, nullptr, nullptr, nullptr, rows, C, slab, acc, nullptr, "bn16_sum", s);
    if (rc) return rc;
    if ((rc = launch_bn_finalize(0, acc, rows, C, eps, momentum, mean, rstd, nullptr, nullptr, s))) return rc;
    if (hipMemsetAsync(acc, 0, sizeof(float) * C, s) != hipSuccess) { mst_set_error("batchnorm_train16: memset failed"); return MST_ELAUNCH; }
    if ((rc = reduce16<R_SQDEV, T>(z, nullptr, nullptr, mean, nullptr, rows, C, slab, acc, nullptr, "bn16_sqdev", s))) return rc;
    if ((rc = launch_bn_finalize(1, acc, rows, C, eps, momentum, mean, rstd, running_mean, running_var, s))) return rc;
    int64_t rpb, rblocks;
    int cblocks;
    bn16_plan(rows, C, rpb, rblocks, cblocks);
    bn16_apply_kernel<T><<<dim3((unsigned)(rblocks * cblocks)), dim3(256), 0, s>>>((const T*)z, mean, rstd, gamma, beta, (const T*)residual, relu,
                                                                                 rows, C, rpb, cblocks, (T*)y);
    return mst_check_launch("bn16_apply");
}

template <typename T>
int bwd16(const void* z, const void* y, const float* mean, const float* rstd, const float* gamma, float* dy, int mask_in_place, int64_t rows, int C,
          float* dgamma, float* dbeta, void* dz, void* ws, hipStream_t s) {
    if (hipMemsetAsync(dgamma, 0, sizeof(float) * C, s) != hipSuccess || hipMemsetAsync(dbeta, 0, sizeof(float) * C, s) != hipSuccess) {
        mst_set_error("batchnorm_bwd16: memset failed");
        return MST_ELAUNCH;
    }
    int rc = reduce16<R_BWD, T>(z, y, dy, mean, rstd, rows, C, (float*)ws, dgamma, dbeta, "bn16_bwd_reduce", s);
    if (rc) return rc;
    int64_t rpb, rblocks;
    int cblocks;
    bn16_plan(rows, C, rpb, rblocks, cblocks);
    bn16_bwd_apply_kernel<T><<<dim3((unsigned)(rblocks * cblocks)), dim3(256), 0, s>>>((const T*)z, (const T*)y, mean, rstd, gamma, dy, mask_in_place,
                                                                                     dgamma, dbeta, rows, C, rpb, cblocks, (T*)dz);
    return mst_check_launch("bn16_bwd_apply");
}

inline bool shape_ok(int64_t rows, int C) { return rows > 0 && C > 0 && C % 8 == 0 && rows < (1ll << 40); }

inline unsigned pgrid(int64_t n) {
    const int64_t g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

}  // namespace

size_t mst_batchnorm_train16_workspace_bytes(int64_t rows, int C) { return shape_ok(rows, C) ? acc_bytes(C) + slab_bytes(rows, C, 1) : 0; }

int mst_batchnorm_train16(const void* z, int dtype, int64_t rows, int C, const float* gamma, const float* beta, float eps, float momentum,
                          const void* residual, int relu, void* y, float* mean, float* rstd, float* running_mean, float* running_var,
                          void* workspace, size_t workspace_bytes, mst_stream_t stream) {
    MST_CHECK_ARG(z && gamma && beta && y && mean && rstd && workspace && shape_ok(rows, C),
                  "batchnorm_train16: bad arguments (rows=%lld, C=%d: C must be a multiple of 8)", (long long)rows, C);
    MST_CHECK_ARG(dtype == MST_BF16 || dtype == MST_F16, "batchnorm_train16: dtype %d (bf16 / f16)", dtype);
    MST_CHECK_ARG(aligned16(z) && aligned16(y) && aligned16(residual) && aligned16(gamma) && aligned16(beta) && aligned16(mean) && aligned16(rstd) &&
                      aligned16(workspace),
                  "batchnorm_train16: every pointer must be 16-byte aligned");
    const size_t need = mst_batchnorm_train16_workspace_bytes(rows, C);
    MST_CHECK_ARG(workspace_bytes >= need, "batchnorm_train16: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == MST_BF16)
        return train16<bf16_t>(z, rows, C, gamma, beta, eps, momentum, residual, relu, y, mean, rstd, running_mean, running_var, workspace, s);
    return train16<f16_t>(z, rows, C, gamma, beta, eps, momentum, residual, relu, y, mean, rstd, running_mean, running_var, workspace, s);
}

size_t mst_batchnorm_bwd16_workspace_bytes(int64_t rows, int C) { return shape_ok(rows, C) ? slab_bytes(rows, C, 2) : 0; }

int mst_batchnorm_bwd16(const void* z, const void* y, int dtype, const float* mean, const float* rstd, const float* gamma, float* dy,
                        int mask_dy_in_place, int64_t rows, int C, float* dgamma, float* dbeta, void* dz, void* workspace, size_t workspace_bytes,
                        mst_stream_t stream) {
    MST_CHECK_ARG(z && mean && rstd && gamma && dy && dgamma && dbeta && dz && workspace && shape_ok(rows, C),
                  "batchnorm_bwd16: bad arguments (rows=%lld, C=%d: C must be a multiple of 8)", (long long)rows, C);
    MST_CHECK_ARG(dtype == MST_BF16 || dtype == MST_F16, "batchnorm_bwd16: dtype %d (bf16 / f16)", dtype);
    MST_CHECK_ARG(aligned16(z) && aligned16(y) && aligned16(mean) && aligned16(rstd) && aligned16(gamma) && aligned16(dy) && aligned16(dgamma) &&
                      aligned16(dbeta) && aligned16(dz) && aligned16(workspace),
                  "batchnorm_bwd16: every pointer must be 16-byte aligned");
    const size_t need = mst_batchnorm_bwd16_workspace_bytes(rows, C);
    MST_CHECK_ARG(workspace_bytes >= need, "batchnorm_bwd16: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == MST_BF16) return bwd16<bf16_t>(z, y, mean, rstd, gamma, dy, mask_dy_in_place, rows, C, dgamma, dbeta, dz, workspace, s);
    return bwd16<f16_t>(z, y, mean, rstd, gamma, dy, mask_dy_in_place, rows, C, dgamma, dbeta, dz, workspace, s);
}

size_t mst_maxpool_bwd_nhwc16_workspace_bytes(int n, int H, int W, int C) { return maxpool_bwd_gather_workspace_bytes(n, H, W, C); }

int mst_maxpool_bwd_nhwc16(const void* x, int dtype, const float* dy, int n, int H, int W, int C, float* dx, void* workspace, size_t workspace_bytes,
                           mst_stream_t stream) {
    MST_CHECK_ARG(x && dy && dx && workspace && n > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0,
                  "maxpool_bwd_nhwc16: bad arguments (C=%d must be a multiple of 8)", C);
    MST_CHECK_ARG(dtype == MST_BF16 || dtype == MST_F16, "maxpool_bwd_nhwc16: dtype %d (bf16 / f16)", dtype);
    MST_CHECK_ARG(aligned16(x) && aligned16(dy) && aligned16(dx) && aligned16(workspace), "maxpool_bwd_nhwc16: every pointer must be 16-byte aligned");
    const size_t need = maxpool_bwd_gather_workspace_bytes(n, H, W, C);
    MST_CHECK_ARG(workspace_bytes >= need, "maxpool_bwd_nhwc16: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    const int64_t groups = (int64_t)n * Ho * Wo * (C / 8);
    if (dtype == MST_BF16) maxpool_arg16_kernel<bf16_t><<<dim3(pgrid(groups)), dim3(256), 0, s>>>((const bf16_t*)x, H, W, C, Ho, Wo, groups, (uint8_t*)workspace);
    else maxpool_arg16_kernel<f16_t><<<dim3(pgrid(groups)), dim3(256), 0, s>>>((const f16_t*)x, H, W, C, Ho, Wo, groups, (uint8_t*)workspace);
    int rc = mst_check_launch("maxpool_arg16");
    if (rc) return rc;
    return launch_maxpool_bwd_from_args((const uint8_t*)workspace, dy, n, H, W, C, dx, s);
}

int mst_avgpool_nhwc16(const void* x, int dtype, int n, int HW, int C, float* y, mst_stream_t stream) {
    MST_CHECK_ARG(x && y && n > 0 && HW > 0 && C > 0 && C % 8 == 0, "avgpool_nhwc16: bad arguments (C=%d must be a multiple of 8)", C);
    MST_CHECK_ARG(dtype == MST_BF16 || dtype == MST_F16, "avgpool_nhwc16: dtype %d (bf16 / f16)", dtype);
    MST_CHECK_ARG(aligned16(x) && aligned16(y), "avgpool_nhwc16: every pointer must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == MST_BF16) avgpool16_kernel<bf16_t><<<dim3(n), dim3(256), 0, s>>>((const bf16_t*)x, HW, C, y);
    else avgpool16_kernel<f16_t><<<dim3(n), dim3(256), 0, s>>>((const f16_t*)x, HW, C, y);
    return mst_check_launch("avgpool_nhwc16");
}
