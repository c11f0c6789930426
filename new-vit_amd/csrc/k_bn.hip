// BatchNorm and pooling of the ResNet training step (mst/train_resnet.py), one kernel family for every mode: the storage type T of the
// activations is fp32, or bf16 / fp16 under train_storage='16bit' (what the reference's autocast does to a convolution + BatchNorm2d + ReLU
// unit, Trainer(precision='16-mixed'), scripts/main_train.py:110-123: z and y live in T; the statistics, the gradient stream and every sum
// are fp32).  All of these are bandwidth kernels on [rows, C] NHWC activations.
//   sums          sum z, sum (z - mean)^2 and d gamma / d beta are colreduce_kernel (k_colsum.hip: launch_bn_reduce), atomic or in fixed
//                 order; a 16-bit z always takes the fixed order.
//   layout        (bn_apply, bn_bwd_apply) a workgroup of 256 lanes owns 64 columns x one block of rows of the column sums' plan; a lane
//                 owns V channels of rows r0 + ty + TY k.  V = 8 (C % 8 == 0, 16-byte aligned bases): ONE 16-byte access of a 16-bit T,
//                 two of fp32; V = 1 (fp32 only): any C, any alignment.  The per-channel vectors are read once per lane before the row
//                 loop; the only integer division is blockIdx.x / cblocks, once per workgroup.
//   arithmetic    fp32, each expression written once with its roundings spelled out (bn_fwd_value, bn_bwd_value, act_deriv in
//                 mst_common.h), so the 16-bit forms return T(the fp32 form on the upcast input) and V = 8 and V = 1 the same bits.  A
//                 result goes through f32_rounded before its conversion: the stored bits are T(the fp32 value).
//   bn_apply      y = T(relu?(gamma (z - mean) rstd + beta + float(residual)))
//   bn_bwd_apply  dz = T(gamma rstd (m dy - d beta / rows - xhat d gamma / rows)); m = y > 0 when the saved y is given (the 16-bit entry
//                 point; the fp32 ones get a dy that is masked already), dy <- m dy on request
//   sequence      bn_train: memset -> sum -> finalize(0) -> memset -> sqdev -> finalize(1) -> apply; bn_bwd: reduce -> apply.  The three
//                 public entry-point pairs (atomic, _ordered, 16) are argument checks in front of these two.
//   maxpool       3 x 3, stride 2, padding 1 (torchvision resnet stem).  Backward: atomic, or the gather form -- pass 1 (maxpool_arg<T, V>)
//                 stores every window's first-maximum position (0..8, torch's scan order ky, kx with a strict >, 255 when nothing beats
//                 -inf), pass 2 gives each input the dy of the (at most 4) windows whose argument it is, windows in ascending (oy, ox)
//   avgpool       y[n][c] = (sum over positions in ascending order of float(x)) / HW: adaptive average pooling to 1 x 1
#include "mst_common.h"

namespace {

template <typename T>
__global__ void maxpool_nhwc_kernel(const T* __restrict__ x, int H, int W, int C, int Ho, int Wo, int64_t total,
                                    T* __restrict__ y) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int ox = (int)((i / C) % Wo), oy = (int)((i / ((int64_t)C * Wo)) % Ho);
        const int64_t n = i / ((int64_t)C * Wo * Ho);
        float m = -INFINITY;
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * 2 - 1 + ky;
            if (iy < 0 || iy >= H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * 2 - 1 + kx;
                if (ix < 0 || ix >= W) continue;
                m = fmaxf(m, (float)x[((n * H + iy) * W + ix) * C + c]);
            }
        }
        y[i] = (T)m;
    }
}

// one workgroup per image, a lane per V channels
template <typename T, int V>
__global__ __launch_bounds__(256) void avgpool_nhwc_kernel(const T* __restrict__ x, int HW, int C, float* __restrict__ y) {
    const int64_t n = blockIdx.x;
    for (int c = threadIdx.x * V; c < C; c += blockDim.x * V) {
        float s[V];
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = 0.f;
#pragma unroll 4
        for (int p = 0; p < HW; ++p) {
            float v[V];
            loadv<V>(x + (n * HW + p) * C + c, v);
#pragma unroll
            for (int e = 0; e < V; ++e) s[e] += v[e];
        }
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = s[e] / (float)HW;
        storev<V>(y + n * C + c, s);
    }
}
__global__ void avgpool_bwd_nhwc_kernel(const float* __restrict__ dy, int HW, int C, int64_t total, float* __restrict__ dx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int64_t n = i / ((int64_t)C * HW);
        dx[i] = dy[n * C + c] / (float)HW;
    }
}

// max-pool backward, atomic form: the gradient goes to the first maximum of the window (scan order ky, kx: torch's choice)
__global__ void maxpool_bwd_nhwc_kernel(const float* __restrict__ x, const float* __restrict__ dy, int H, int W, int C, int Ho, int Wo,
                                        int64_t total, float* __restrict__ dx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int ox = (int)((i / C) % Wo), oy = (int)((i / ((int64_t)C * Wo)) % Ho);
        const int64_t n = i / ((int64_t)C * Wo * Ho);
        float m = -INFINITY;
        int64_t arg = -1;
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * 2 - 1 + ky;
            if (iy < 0 || iy >= H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * 2 - 1 + kx;
                if (ix < 0 || ix >= W) continue;
                const int64_t j = ((n * H + iy) * W + ix) * C + c;
                const float v = x[j];
                if (v > m) { m = v; arg = j; }
            }
        }
        if (arg >= 0) atomicAdd(dx + arg, dy[i]);
    }
}
// gather form, pass 1: arg[window][c] = ky * 3 + kx of the first maximum (scan order ky, kx, strict >: the rule of the atomic form), 255
// when no element beats -inf.  One lane per window and V channels.
template <typename T, int V>
__global__ __launch_bounds__(256) void maxpool_arg_kernel(const T* __restrict__ x, int H, int W, int C, int Ho, int Wo, int64_t groups,
                                                          uint8_t* __restrict__ arg) {
    const int cv = C / V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < groups; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t win = i / cv;
        const int c = (int)(i - win * cv) * V;
        const int ox = (int)(win % Wo), oy = (int)((win / Wo) % Ho);
        const int64_t n = win / ((int64_t)Wo * Ho);
        float m[V];
        unsigned a[V];
#pragma unroll
        for (int e = 0; e < V; ++e) { m[e] = -INFINITY; a[e] = 255u; }
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * 2 - 1 + ky;
            if (iy < 0 || iy >= H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * 2 - 1 + kx;
                if (ix < 0 || ix >= W) continue;
                float v[V];
                loadv<V>(x + ((n * H + iy) * W + ix) * C + c, v);
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (v[e] > m[e]) { m[e] = v[e]; a[e] = (unsigned)(ky * 3 + kx); }
            }
        }
        if constexpr (V == 8) {
            u32x2 o;
            o[0] = a[0] | a[1] << 8 | a[2] << 16 | a[3] << 24;
            o[1] = a[4] | a[5] << 8 | a[6] << 16 | a[7] << 24;
            *reinterpret_cast<u32x2*>(arg + win * C + c) = o;
        } else {
            arg[i] = (uint8_t)a[0];
        }
    }
}
// pass 2: dx[n][iy][ix][c] += the dy of every window (ascending oy, ox) whose first maximum is this input.  V4 (C % 4 == 0): one thread per
// four channels of a pixel (16-byte dx / dy, 4-byte argument loads, the index arithmetic once per four elements)
template <bool V4>
__global__ void maxpool_bwd_gather_kernel(const uint8_t* __restrict__ arg, const float* __restrict__ dy, int H, int W, int C, int Ho, int Wo,
                                          int64_t total, float* __restrict__ dx) {
    constexpr int V = V4 ? 4 : 1;
    const int64_t groups = total / V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < groups; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e0 = i * V, pix = e0 / C;
        const int c = (int)(e0 - pix * C);
        const int ix = (int)(pix % W), iy = (int)((pix / W) % H);
        const int64_t n = pix / ((int64_t)W * H);
        float s[V];
        if (V4) {
            const float4 v = *reinterpret_cast<const float4*>(dx + e0);
            s[0] = v.x; s[V > 1 ? 1 : 0] = v.y; s[V > 2 ? 2 : 0] = v.z; s[V > 3 ? 3 : 0] = v.w;
        } else {
            s[0] = dx[e0];
        }
        const int oy1 = min((iy + 1) / 2, Ho - 1), ox1 = min((ix + 1) / 2, Wo - 1);
        for (int oy = iy / 2; oy <= oy1; ++oy) {
            for (int ox = ix / 2; ox <= ox1; ++ox) {
                const int64_t w = ((n * Ho + oy) * Wo + ox) * C + c;
                const int code = (iy - (oy * 2 - 1)) * 3 + (ix - (ox * 2 - 1));
                uint8_t a[V];
                if (V4) {
                    const uchar4 av = *reinterpret_cast<const uchar4*>(arg + w);
                    a[0] = av.x; a[V > 1 ? 1 : 0] = av.y; a[V > 2 ? 2 : 0] = av.z; a[V > 3 ? 3 : 0] = av.w;
                } else {
                    a[0] = arg[w];
                }
#pragma unroll
                for (int j = 0; j < V; ++j)
                    if (a[j] == code) s[j] += dy[w + j];
            }
        }
        if (V4) *reinterpret_cast<float4*>(dx + e0) = make_float4(s[0], s[V > 1 ? 1 : 0], s[V > 2 ? 2 : 0], s[V > 3 ? 3 : 0]);
        else dx[e0] = s[0];
    }
}

// ---- BatchNorm with batch statistics (nn.BatchNorm2d in train mode) ------------------------------------------------------------------
// stage 0: mean = sum / rows.  stage 1: rstd = rsqrt(sqdev / rows + eps); running statistics as nn.BatchNorm2d updates them
// (momentum, unbiased variance)
__global__ void bn_finalize_kernel(int stage, const float* __restrict__ acc, int64_t rows, int C, float eps, float momentum,
                                   float* __restrict__ mean, float* __restrict__ rstd, float* running_mean, float* running_var) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    if (stage == 0) { mean[c] = acc[c] / (float)rows; return; }
    const float var = acc[c] / (float)rows;
    rstd[c] = rsqrtf(var + eps);
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean[c];
    if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * var * ((float)rows / (float)(rows > 1 ? rows - 1 : 1));
}

// the block of rows and the V channels of this lane
template <int V>
struct Tile {
    static constexpr int TX = 64 / V, TY = 256 / TX;
    int64_t r0, r1;
    int c0;
    __device__ __forceinline__ Tile(int64_t rows, int64_t rpb, int cblocks) {
        const int64_t rb = blockIdx.x / cblocks;
        const int cb = (int)(blockIdx.x - rb * cblocks);
        r0 = rb * rpb + threadIdx.x / TX;
        r1 = rb * rpb + rpb < rows ? rb * rpb + rpb : rows;
        c0 = cb * 64 + (threadIdx.x % TX) * V;
    }
};

template <typename T, int V>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, const T* __restrict__ res,
                                                       int relu, int64_t rows, int C, int64_t rpb, int cblocks, T* __restrict__ y) {
    const Tile<V> t(rows, rpb, cblocks);
    if (t.c0 >= C) return;
    float mc[V], rc[V], gc[V], bc[V];
    loadv<V>(mean + t.c0, mc);
    loadv<V>(rstd + t.c0, rc);
    loadv<V>(gamma + t.c0, gc);
    loadv<V>(beta + t.c0, bc);
    for (int64_t r = t.r0; r < t.r1; r += Tile<V>::TY) {
        const int64_t off = r * C + t.c0;
        float v[V];
        loadv<V>(z + off, v);
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = bn_fwd_value(v[e], mc[e], rc[e], gc[e], bc[e]);
        if (res) {
            float a[V];
            loadv<V>(res + off, a);
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] += a[e];
        }
        if (relu) {
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] = fmaxf(v[e], 0.f);
        }
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = f32_rounded(v[e]);
        storev<V>(y + off, v);
    }
}

// y (nullable): the unit's saved output, whose sign is the ReLU mask of dy; mask_in_place: dy <- m dy as well
template <typename T, int V>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ z, const T* __restrict__ y, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ gamma, float* dy,
                                                           int mask_in_place, const float* __restrict__ dgamma, const float* __restrict__ dbeta,
                                                           int64_t rows, int C, int64_t rpb, int cblocks, T* __restrict__ dz) {
    const Tile<V> t(rows, rpb, cblocks);
    if (t.c0 >= C) return;
    const float inv = 1.0f / (float)rows;
    float mc[V], rc[V], gc[V], dg[V], db[V];
    loadv<V>(mean + t.c0, mc);
    loadv<V>(rstd + t.c0, rc);
    loadv<V>(gamma + t.c0, gc);
    loadv<V>(dgamma + t.c0, dg);
    loadv<V>(dbeta + t.c0, db);
    for (int64_t r = t.r0; r < t.r1; r += Tile<V>::TY) {
        const int64_t off = r * C + t.c0;
        float v[V], g[V];
        loadv<V>(z + off, v);
        loadv<V>(dy + off, g);
        if (y) {
            float yy[V];
            loadv<V>(y + off, yy);
#pragma unroll
            for (int e = 0; e < V; ++e) g[e] *= act_deriv(yy[e], 1);
            if (mask_in_place) storev<V>(dy + off, g);
        }
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = f32_rounded(bn_bwd_value(v[e], mc[e], rc[e], gc[e], g[e], dg[e], db[e], inv));
        storev<V>(dz + off, v);
    }
}

// fn(T{}) for the storage type `dt` names
template <typename Fn>
int with_type(int dt, Fn fn) {
    if (dt == MST_F32) return fn(float{});
    if (dt == MST_BF16) return fn(bf16_t{});
    return fn(f16_t{});
}
inline bool is16(int dt) { return dt == MST_BF16 || dt == MST_F16; }

// the row blocks of the elementwise passes: the plan of the 16-bit column sums (whose thread rows are V = 8's)
struct ApplyGrid {
    int64_t rpb, rblocks;
    int cblocks;
    ApplyGrid(int64_t rows, int C) : cblocks((C + 63) / 64) { colsum_plan(rows, C, 32, rpb, rblocks); }
    dim3 grid() const { return dim3((unsigned)(rblocks * cblocks)); }
};

// V = 8 when `v8`; V = 1 exists for fp32 only (the 16-bit entry points refuse what V = 8 cannot take)
int bn_apply(const void* z, int dt, const float* mean, const float* rstd, const float* gamma, const float* beta, const void* res, int relu,
             int64_t rows, int C, void* y, bool v8, hipStream_t s) {
    const ApplyGrid g(rows, C);
    with_type(dt, [&](auto t) {
        typedef decltype(t) T;
        if (v8) bn_apply_kernel<T, 8><<<g.grid(), dim3(256), 0, s>>>((const T*)z, mean, rstd, gamma, beta, (const T*)res, relu, rows, C, g.rpb, g.cblocks, (T*)y);
        else if constexpr (sizeof(T) == 4)
            bn_apply_kernel<T, 1><<<g.grid(), dim3(256), 0, s>>>((const T*)z, mean, rstd, gamma, beta, (const T*)res, relu, rows, C, g.rpb, g.cblocks, (T*)y);
        return 0;
    });
    return mst_check_launch("bn_apply");
}
int bn_bwd_apply(const void* z, int dt, const void* y, const float* mean, const float* rstd, const float* gamma, float* dy, int mask_in_place,
                 const float* dgamma, const float* dbeta, int64_t rows, int C, void* dz, bool v8, hipStream_t s) {
    const ApplyGrid g(rows, C);
    with_type(dt, [&](auto t) {
        typedef decltype(t) T;
        if (v8) bn_bwd_apply_kernel<T, 8><<<g.grid(), dim3(256), 0, s>>>((const T*)z, (const T*)y, mean, rstd, gamma, dy, mask_in_place, dgamma, dbeta, rows, C, g.rpb, g.cblocks, (T*)dz);
        else if constexpr (sizeof(T) == 4)
            bn_bwd_apply_kernel<T, 1><<<g.grid(), dim3(256), 0, s>>>((const T*)z, (const T*)y, mean, rstd, gamma, dy, mask_in_place, dgamma, dbeta, rows, C, g.rpb, g.cblocks, (T*)dz);
        return 0;
    });
    return mst_check_launch("bn_bwd_apply");
}

// where the column sums of one call go: atomically into the output (no workspace), or in fixed order through `slab`
struct BnSums {
    bool ordered;
    void* slab;
    size_t slab_bytes;
};

// mean, rstd and the running statistics of z [rows, C] of type dt through `acc` (C floats), then y
int bn_train(const char* what, const void* z, int dt, int64_t rows, int C, const float* gamma, const float* beta, float eps, float momentum,
             const void* residual, int relu, void* y, float* mean, float* rstd, float* running_mean, float* running_var, float* acc,
             const BnSums& sums, hipStream_t s) {
    for (int stage = 0; stage < 2; ++stage) {                           // the column mean, then the centred sum of squares
        if (hipMemsetAsync(acc, 0, sizeof(float) * C, s) != hipSuccess) { mst_set_error("%s: memset failed", what); return MST_ELAUNCH; }
        int rc = launch_bn_reduce(stage ? COL_SQDEV : COL_SUM, z, dt, nullptr, nullptr, stage ? mean : nullptr, nullptr, rows, C, acc, nullptr,
                                  sums.ordered, sums.slab, sums.slab_bytes, s);
        if (rc) return rc;
        bn_finalize_kernel<<<dim3((C + 255) / 256), dim3(256), 0, s>>>(stage, acc, rows, C, eps, momentum, mean, rstd, stage ? running_mean : nullptr,
                                                                       stage ? running_var : nullptr);
        if ((rc = mst_check_launch("bn_finalize"))) return rc;
    }
    const bool v8 = C % 8 == 0 && aligned(z, 16) && aligned(y, 16) && aligned(residual, 16) && aligned(mean, 16) && aligned(rstd, 16) &&
                    aligned(gamma, 16) && aligned(beta, 16);
    return bn_apply(z, dt, mean, rstd, gamma, beta, residual, relu, rows, C, y, v8, s);
}

// dgamma, dbeta += the two column sums (y: the mask of the saved output, 16-bit only), then dz
int bn_bwd(const void* z, int dt, const void* y, const float* mean, const float* rstd, const float* gamma, float* dy, int mask_in_place,
           int64_t rows, int C, float* dgamma, float* dbeta, void* dz, const BnSums& sums, hipStream_t s) {
    int rc = launch_bn_reduce(COL_BN_BWD, z, dt, y, dy, mean, rstd, rows, C, dgamma, dbeta, sums.ordered, sums.slab, sums.slab_bytes, s);
    if (rc) return rc;
    const bool v8 = C % 8 == 0 && aligned(z, 16) && aligned(y, 16) && aligned(dy, 16) && aligned(dz, 16) && aligned(mean, 16) &&
                    aligned(rstd, 16) && aligned(gamma, 16) && aligned(dgamma, 16) && aligned(dbeta, 16);
    return bn_bwd_apply(z, dt, y, mean, rstd, gamma, dy, mask_in_place, dgamma, dbeta, rows, C, dz, v8, s);
}

inline size_t acc_bytes(int C) { return round256(sizeof(float) * (size_t)C); }
inline bool shape16_ok(int64_t rows, int C) { return rows > 0 && C > 0 && C % 8 == 0 && rows < (1ll << 40); }
// the 16-bit forms keep a slab for a single row block too
inline size_t slab16_bytes(int64_t rows, int C, int outputs) {
    int64_t rpb, rblocks;
    colsum_plan(rows, C, 32, rpb, rblocks);
    return round256(sizeof(float) * (size_t)rblocks * outputs * C);
}

}  // namespace

// ---- pooling -----------------------------------------------------------------------------------------------------------------------------
int launch_maxpool_nhwc(const void* x, int dt, int n, int H, int W, int C, void* y, hipStream_t s) {
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    const int64_t total = (int64_t)n * Ho * Wo * C;
    if (dt != MST_F32 && !is16(dt)) { mst_set_error("maxpool16: dtype %d (bf16 / f16)", dt); return MST_EINVAL; }
    with_type(dt, [&](auto t) {
        typedef decltype(t) T;
        maxpool_nhwc_kernel<T><<<dim3(grid256(total)), dim3(256), 0, s>>>((const T*)x, H, W, C, Ho, Wo, total, (T*)y);
        return 0;
    });
    return mst_check_launch(dt == MST_F32 ? "maxpool_nhwc" : "maxpool_nhwc16");
}

// x of type dt; V = 8 where C and the bases allow, one channel per lane otherwise (fp32 only)
int launch_avgpool_nhwc(const void* x, int dt, int n, int HW, int C, float* y, hipStream_t s) {
    const bool v8 = C % 8 == 0 && aligned(x, 16) && aligned(y, 16);
    with_type(dt, [&](auto t) {
        typedef decltype(t) T;
        if (v8) avgpool_nhwc_kernel<T, 8><<<dim3(n), dim3(256), 0, s>>>((const T*)x, HW, C, y);
        else if constexpr (sizeof(T) == 4) avgpool_nhwc_kernel<T, 1><<<dim3(n), dim3(256), 0, s>>>((const T*)x, HW, C, y);
        return 0;
    });
    return mst_check_launch(dt == MST_F32 ? "avgpool_nhwc" : "avgpool_nhwc16");
}
int launch_avgpool_bwd_nhwc(const float* dy, int n, int HW, int C, float* dx, hipStream_t s) {
    const int64_t total = (int64_t)n * HW * C;
    avgpool_bwd_nhwc_kernel<<<dim3(grid256(total)), dim3(256), 0, s>>>(dy, HW, C, total, dx);
    return mst_check_launch("avgpool_bwd_nhwc");
}

int launch_maxpool_bwd_nhwc(const float* x, const float* dy, int n, int H, int W, int C, float* dx, hipStream_t s) {
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    const int64_t total = (int64_t)n * Ho * Wo * C;
    maxpool_bwd_nhwc_kernel<<<dim3(grid256(total)), dim3(256), 0, s>>>(x, dy, H, W, C, Ho, Wo, total, dx);
    return mst_check_launch("maxpool_bwd_nhwc");
}

size_t maxpool_bwd_gather_workspace_bytes(int n, int H, int W, int C) {
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    return n > 0 && H > 0 && W > 0 && C > 0 ? round256((size_t)n * Ho * Wo * C) : 0;
}

// both passes of the gather form; x of type dt (the same codes, so the same dx, as the fp32 form on the upcast x)
int launch_maxpool_bwd_gather(const char* what, const void* x, int dt, const float* dy, int n, int H, int W, int C, float* dx, void* ws,
                              size_t ws_bytes, hipStream_t s) {
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    const size_t need = maxpool_bwd_gather_workspace_bytes(n, H, W, C);
    MST_CHECK_ARG(ws && ws_bytes >= need, "%s: workspace of %zu bytes, %zu needed", what, ws_bytes, need);
    const int64_t windows = (int64_t)n * Ho * Wo * C;
    const bool v8 = C % 8 == 0 && aligned(x, 16) && aligned(ws, 8);
    with_type(dt, [&](auto t) {
        typedef decltype(t) T;
        if (v8) maxpool_arg_kernel<T, 8><<<dim3(grid256(windows / 8)), dim3(256), 0, s>>>((const T*)x, H, W, C, Ho, Wo, windows / 8, (uint8_t*)ws);
        else if constexpr (sizeof(T) == 4)
            maxpool_arg_kernel<T, 1><<<dim3(grid256(windows)), dim3(256), 0, s>>>((const T*)x, H, W, C, Ho, Wo, windows, (uint8_t*)ws);
        return 0;
    });
    int rc = mst_check_launch("maxpool_arg");
    if (rc) return rc;
    const int64_t total = (int64_t)n * H * W * C;
    const bool v4 = C % 4 == 0 && aligned(dx, 16) && aligned(dy, 4) && aligned(ws, 4);   // the same sums in the same order either way
    if (v4) maxpool_bwd_gather_kernel<true><<<dim3(grid256(total / 4)), dim3(256), 0, s>>>((const uint8_t*)ws, dy, H, W, C, Ho, Wo, total, dx);
    else maxpool_bwd_gather_kernel<false><<<dim3(grid256(total)), dim3(256), 0, s>>>((const uint8_t*)ws, dy, H, W, C, Ho, Wo, total, dx);
    return mst_check_launch("maxpool_bwd_gather");
}

size_t mst_maxpool_bwd_nhwc16_workspace_bytes(int n, int H, int W, int C) { return maxpool_bwd_gather_workspace_bytes(n, H, W, C); }

int mst_maxpool_bwd_nhwc16(const void* x, int dtype, const float* dy, int n, int H, int W, int C, float* dx, void* workspace, size_t workspace_bytes,
                           mst_stream_t stream) {
    MST_CHECK_ARG(x && dy && dx && workspace && n > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0,
                  "maxpool_bwd_nhwc16: bad arguments (C=%d must be a multiple of 8)", C);
    MST_CHECK_ARG(is16(dtype), "maxpool_bwd_nhwc16: dtype %d (bf16 / f16)", dtype);
    MST_CHECK_ARG(aligned(x, 16) && aligned(dy, 16) && aligned(dx, 16) && aligned(workspace, 16), "maxpool_bwd_nhwc16: every pointer must be 16-byte aligned");
    return launch_maxpool_bwd_gather("maxpool_bwd_nhwc16", x, dtype, dy, n, H, W, C, dx, workspace, workspace_bytes, (hipStream_t)stream);
}

int mst_avgpool_nhwc16(const void* x, int dtype, int n, int HW, int C, float* y, mst_stream_t stream) {
    MST_CHECK_ARG(x && y && n > 0 && HW > 0 && C > 0 && C % 8 == 0, "avgpool_nhwc16: bad arguments (C=%d must be a multiple of 8)", C);
    MST_CHECK_ARG(is16(dtype), "avgpool_nhwc16: dtype %d (bf16 / f16)", dtype);
    MST_CHECK_ARG(aligned(x, 16) && aligned(y, 16), "avgpool_nhwc16: every pointer must be 16-byte aligned");
    return launch_avgpool_nhwc(x, dtype, n, HW, C, y, (hipStream_t)stream);
}

// ---- BatchNorm entry points: atomic fp32, fixed-order fp32, 16-bit storage ------------------------------------------------------------------
int mst_batchnorm_train(const float* z, int64_t rows, int C, const float* gamma, const float* beta, float eps, float momentum,
                        const float* residual, int relu, float* y, float* mean, float* rstd, float* running_mean,
                        float* running_var, float* scratch, mst_stream_t stream) {
    MST_CHECK_ARG(z && gamma && beta && y && mean && rstd && scratch && rows > 0 && C > 0, "batchnorm_train: bad arguments");
    return bn_train("batchnorm_train", z, MST_F32, rows, C, gamma, beta, eps, momentum, residual, relu, y, mean, rstd, running_mean, running_var,
                    scratch, BnSums{false, nullptr, 0}, (hipStream_t)stream);
}
int mst_batchnorm_bwd(const float* z, const float* mean, const float* rstd, const float* gamma, const float* dy, int64_t rows, int C,
                      float* dgamma, float* dbeta, float* dz, mst_stream_t stream) {
    MST_CHECK_ARG(z && mean && rstd && gamma && dy && dgamma && dbeta && dz && rows > 0 && C > 0, "batchnorm_bwd: bad arguments");
    return bn_bwd(z, MST_F32, nullptr, mean, rstd, gamma, const_cast<float*>(dy), 0, rows, C, dgamma, dbeta, dz, BnSums{false, nullptr, 0},
                  (hipStream_t)stream);
}

size_t mst_batchnorm_train_ordered_workspace_bytes(int64_t rows, int C) {
    return rows > 0 && C > 0 ? acc_bytes(C) + colsum_ordered_workspace_bytes(rows, C, 1) : 0;
}
int mst_batchnorm_train_ordered(const float* z, int64_t rows, int C, const float* gamma, const float* beta, float eps, float momentum,
                                const float* residual, int relu, float* y, float* mean, float* rstd, float* running_mean,
                                float* running_var, void* workspace, size_t workspace_bytes, mst_stream_t stream) {
    MST_CHECK_ARG(z && gamma && beta && y && mean && rstd && workspace && rows > 0 && C > 0, "batchnorm_train_ordered: bad arguments");
    const size_t need = mst_batchnorm_train_ordered_workspace_bytes(rows, C);
    MST_CHECK_ARG(workspace_bytes >= need, "batchnorm_train_ordered: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    return bn_train("batchnorm_train_ordered", z, MST_F32, rows, C, gamma, beta, eps, momentum, residual, relu, y, mean, rstd, running_mean,
                    running_var, (float*)workspace,                     // C floats, then the slab of the column sums
                    BnSums{true, (char*)workspace + acc_bytes(C), workspace_bytes - acc_bytes(C)}, (hipStream_t)stream);
}
size_t mst_batchnorm_bwd_ordered_workspace_bytes(int64_t rows, int C) { return colsum_ordered_workspace_bytes(rows, C, 2); }
int mst_batchnorm_bwd_ordered(const float* z, const float* mean, const float* rstd, const float* gamma, const float* dy, int64_t rows, int C,
                              float* dgamma, float* dbeta, float* dz, void* workspace, size_t workspace_bytes, mst_stream_t stream) {
    MST_CHECK_ARG(z && mean && rstd && gamma && dy && dgamma && dbeta && dz && rows > 0 && C > 0, "batchnorm_bwd_ordered: bad arguments");
    return bn_bwd(z, MST_F32, nullptr, mean, rstd, gamma, const_cast<float*>(dy), 0, rows, C, dgamma, dbeta, dz,
                  BnSums{true, workspace, workspace_bytes}, (hipStream_t)stream);
}

size_t mst_batchnorm_train16_workspace_bytes(int64_t rows, int C) { return shape16_ok(rows, C) ? acc_bytes(C) + slab16_bytes(rows, C, 1) : 0; }

int mst_batchnorm_train16(const void* z, int dtype, int64_t rows, int C, const float* gamma, const float* beta, float eps, float momentum,
                          const void* residual, int relu, void* y, float* mean, float* rstd, float* running_mean, float* running_var,
                          void* workspace, size_t workspace_bytes, mst_stream_t stream) {
    MST_CHECK_ARG(z && gamma && beta && y && mean && rstd && workspace && shape16_ok(rows, C),
                  "batchnorm_train16: bad arguments (rows=%lld, C=%d: C must be a multiple of 8)", (long long)rows, C);
    MST_CHECK_ARG(is16(dtype), "batchnorm_train16: dtype %d (bf16 / f16)", dtype);
    MST_CHECK_ARG(aligned(z, 16) && aligned(y, 16) && aligned(residual, 16) && aligned(gamma, 16) && aligned(beta, 16) && aligned(mean, 16) &&
                      aligned(rstd, 16) && aligned(workspace, 16),
                  "batchnorm_train16: every pointer must be 16-byte aligned");
    const size_t need = mst_batchnorm_train16_workspace_bytes(rows, C);
    MST_CHECK_ARG(workspace_bytes >= need, "batchnorm_train16: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    return bn_train("batchnorm_train16", z, dtype, rows, C, gamma, beta, eps, momentum, residual, relu, y, mean, rstd, running_mean, running_var,
                    (float*)workspace, BnSums{true, (char*)workspace + acc_bytes(C), workspace_bytes - acc_bytes(C)}, (hipStream_t)stream);
}

size_t mst_batchnorm_bwd16_workspace_bytes(int64_t rows, int C) { return shape16_ok(rows, C) ? slab16_bytes(rows, C, 2) : 0; }

int mst_batchnorm_bwd16(const void* z, const void* y, int dtype, const float* mean, const float* rstd, const float* gamma, float* dy,
                        int mask_dy_in_place, int64_t rows, int C, float* dgamma, float* dbeta, void* dz, void* workspace, size_t workspace_bytes,
                        mst_stream_t stream) {
    MST_CHECK_ARG(z && mean && rstd && gamma && dy && dgamma && dbeta && dz && workspace && shape16_ok(rows, C),
                  "batchnorm_bwd16: bad arguments (rows=%lld, C=%d: C must be a multiple of 8)", (long long)rows, C);
    MST_CHECK_ARG(is16(dtype), "batchnorm_bwd16: dtype %d (bf16 / f16)", dtype);
    MST_CHECK_ARG(aligned(z, 16) && aligned(y, 16) && aligned(mean, 16) && aligned(rstd, 16) && aligned(gamma, 16) && aligned(dy, 16) &&
                      aligned(dgamma, 16) && aligned(dbeta, 16) && aligned(dz, 16) && aligned(workspace, 16),
                  "batchnorm_bwd16: every pointer must be 16-byte aligned");
    const size_t need = mst_batchnorm_bwd16_workspace_bytes(rows, C);
    MST_CHECK_ARG(workspace_bytes >= need, "batchnorm_bwd16: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;                                // this entry point OVERWRITES d gamma / d beta
    if (hipMemsetAsync(dgamma, 0, sizeof(float) * C, s) != hipSuccess || hipMemsetAsync(dbeta, 0, sizeof(float) * C, s) != hipSuccess) {
        mst_set_error("batchnorm_bwd16: memset failed");
        return MST_ELAUNCH;
    }
    return bn_bwd(z, dtype, y, mean, rstd, gamma, dy, mask_dy_in_place, rows, C, dgamma, dbeta, dz, BnSums{true, workspace, workspace_bytes}, s);
}
