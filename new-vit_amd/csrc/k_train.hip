// Kernels of the training step (the backward pass of DinoV2ClassifierSlice), all fp32 on the exact fp32 MFMA
// (v_mfma_f32_32x32x2_f32): the first correct version -- gradients are checked against autograd of the CPU oracle at the
// fp32 bar.  What the reference gets from torch.autograd (base_model.py:148-181 `_step`; main_train.py:110-126) is spelled out
// here op by op:
//   gemm_ex        (k_gemm_ex.hip) C[b] = alpha * A[b] . B[b] (+ beta * C[b]), every operand with explicit element strides and a two-level
//                  batch: one entry covers dX = dY.W, dW = dY^T.X, and the four products of the attention backward on the packed
//                  q|k|v layout of the forward (attention.py:56-66)
//   softmax_rows / softmax_rows_bwd     P = softmax(S + key-padding mask),  dS = P o (dP - rowsum(dP o P))
//   layernorm_bwd  dx (+ residual gradient), d gamma, d beta   (nn.LayerNorm; block.py:63,75; transformer_blocks.py:499)
//   act_fwd / act_bwd   GELU (erf form, mlp.py:22) / ReLU (transformer_blocks.py:484) and its derivative times the upstream gradient;
//   swiglu_fwd / _bwd   the SwiGLU FFN's gate (swiglu_ffn.py:54-72): one template per op for fp32 and the 16-bit storage types
//   axpby_cols     LayerScale on a gradient, residual sums (layer_scale.py:25-27; the column sums of the bias and LayerScale gradients
//                  are k_colsum.hip)
//   im2col14       the 14x14 patches of a gray volume as rows (patch_embed.py:68-81): d W_patch = dX^T . im2col
//   pos_interp_bwd adjoint of the bicubic position-grid resampling (vision_transformer.py:179-211)
#include "mst_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// P = softmax over the last dim of S [B, H, Lq, L] (in place); mask uint8 [B, L], 1 = key ignored (-inf before the softmax).
__global__ void softmax_rows_kernel(float* __restrict__ S, const uint8_t* __restrict__ mask, int64_t rows, int L, int rows_per_b) {
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    float* s = S + row * L;
    const uint8_t* mk = mask ? mask + (row / rows_per_b) * L : nullptr;
    float mx = -INFINITY;
    for (int j = lane; j < L; j += 64) mx = fmaxf(mx, (mk && mk[j]) ? -INFINITY : s[j]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < L; j += 64) {
        const float e = (mk && mk[j]) ? 0.f : expf(s[j] - mx);
        s[j] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    const float inv = 1.0f / sum;
    for (int j = lane; j < L; j += 64) s[j] *= inv;
}

// dS = scale * P o (dP - rowsum(dP o P)), written over dP.
__global__ void softmax_rows_bwd_kernel(const float* __restrict__ P, float* __restrict__ dP, int64_t rows, int L, float scale) {
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* p = P + row * L;
    float* d = dP + row * L;
    float dot = 0.f;
    for (int j = lane; j < L; j += 64) dot = fmaf(d[j], p[j], dot);
    dot = wave_sum(dot);
    for (int j = lane; j < L; j += 64) d[j] = scale * p[j] * (d[j] - dot);
}

// ---------------------------------------------------------------------------------------------------------------
// LayerNorm backward.  One wave per row at a time, waves stride over the rows; d gamma / d beta partial sums live in registers
// (column c = lane + 64 i, i < CI), meet in LDS at the end and are added to the fp32 outputs with one atomic per column per workgroup.
//   dx[row] = (dres ? dres[row] : 0) + rstd * (dyg - mean(dyg) - xhat * mean(dyg * xhat)),   dyg = dy * gamma
// SLAB (the ordered form, mst_layernorm_bwd_ordered): no atomic -- workgroup g stores its column sums into slab[g][0 | 1][cols]
// (d gamma | d beta) with plain stores, and launch_slab_reduce adds the slabs in ascending g.
template <int CI, bool SLAB = false>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ x, int64_t xs, const float* __restrict__ gamma,
                                                            const float* __restrict__ dy, int64_t dys, const float* dres, int64_t drs,
                                                            float* dx, int64_t dxs, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, int64_t rows, int cols, float eps,
                                                            float* __restrict__ slab = nullptr) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * (blockDim.x >> 6);
    float gsum[CI], bsum[CI], gm[CI];
#pragma unroll
    for (int i = 0; i < CI; ++i) {
        gsum[i] = bsum[i] = 0.f;
        const int c = lane + 64 * i;
        gm[i] = (c < cols) ? (gamma ? gamma[c] : 1.f) : 0.f;
    }
    for (int64_t row = w; row < rows; row += nw) {
        const float* xr = x + row * xs;
        const float* dr = dy + row * dys;
        float xv[CI], dv[CI];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < CI; ++i) {
            const int c = lane + 64 * i;
            xv[i] = c < cols ? xr[c] : 0.f;
            dv[i] = c < cols ? dr[c] : 0.f;
            s += xv[i];
        }
        const float mean = wave_sum(s) / (float)cols;
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < CI; ++i) {
            const float d = (lane + 64 * i < cols) ? xv[i] - mean : 0.f;
            sq = fmaf(d, d, sq);
        }
        const float rstd = rsqrtf(wave_sum(sq) / (float)cols + eps);
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int i = 0; i < CI; ++i) {
            const bool in = lane + 64 * i < cols;
            const float xh = in ? (xv[i] - mean) * rstd : 0.f;
            const float dg = dv[i] * gm[i];
            xv[i] = xh;
            a += dg;
            b = fmaf(dg, xh, b);
            gsum[i] = fmaf(dv[i], xh, gsum[i]);
            bsum[i] += dv[i];
        }
        a = wave_sum(a) / (float)cols;
        b = wave_sum(b) / (float)cols;
        if (dx) {
#pragma unroll
            for (int i = 0; i < CI; ++i) {
                const int c = lane + 64 * i;
                if (c < cols) {
                    const float v = rstd * (dv[i] * gm[i] - a - xv[i] * b);
                    dx[row * dxs + c] = (dres ? dres[row * drs + c] : 0.f) + v;
                }
            }
        }
    }
    // the four waves' partial sums meet in LDS; one atomic per column per workgroup
    __shared__ float red[4][2][CI * 64];
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < CI; ++i) {
        red[wave][0][lane + 64 * i] = gsum[i];
        red[wave][1][lane + 64 * i] = bsum[i];
    }
    __syncthreads();
    if constexpr (SLAB) {
        float* o = slab + (int64_t)blockIdx.x * 2 * cols;
        for (int c = threadIdx.x; c < cols; c += 256) {
            o[c] = (red[0][0][c] + red[1][0][c]) + (red[2][0][c] + red[3][0][c]);
            o[cols + c] = (red[0][1][c] + red[1][1][c]) + (red[2][1][c] + red[3][1][c]);
        }
        return;
    }
    for (int c = threadIdx.x; c < cols; c += 256) {
        if (dgamma) atomicAdd(dgamma + c, (red[0][0][c] + red[1][0][c]) + (red[2][0][c] + red[3][0][c]));
        if (dbeta) atomicAdd(dbeta + c, (red[0][1][c] + red[1][1][c]) + (red[2][1][c] + red[3][1][c]));
    }
}

// ---------------------------------------------------------------------------------------------------------------
// RoPE of the across-slice attention (rotary_embedding_torch.py:38-62,159-173; transformer_blocks.py:262-264) on packed q | k | v rows, in
// place: the pairs (2p, 2p+1) of every head's q and k are rotated by sign * position * freqs[p] (position = row % L, the class token
// is position 0).  sign +1: the forward; sign -1: its adjoint on (dq', dk') -- rotations are orthogonal, and the frequencies are buffers
// without a gradient (learned_freq = False).
__global__ void rope_rows_kernel(float* __restrict__ qkv, int64_t rows, int L, int heads, int hd, const float* __restrict__ freqs, float sign) {
    const int half = hd / 2, e = heads * hd;
    const int64_t total = rows * 2 * heads * half;                     // (row, q|k, head, pair)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int p = (int)(i % half);
        const int h = (int)((i / half) % heads);
        const int which = (int)((i / ((int64_t)half * heads)) % 2);
        const int64_t r = i / ((int64_t)half * heads * 2);
        float sn, cs;
        sincosf(sign * (float)(r % L) * freqs[p], &sn, &cs);
        float* v = qkv + r * 3 * e + which * e + h * hd + 2 * p;
        const float a = v[0], b = v[1];
        v[0] = a * cs - b * sn;
        v[1] = b * cs + a * sn;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The elementwise ops of the MLP, one template each for the three storage types T (fp32, and bf16 / fp16 of train_storage='16bit') and
// for V = 8 elements per thread in 16-byte accesses or V = 1.  The arithmetic is fp32 and the same expression in every instantiation, so
// the 16-bit forms return T(the fp32 form on the upcast input) and the V = 8 and V = 1 forms return the same bits.  A 16-bit store goes
// through f32_rounded (mst_common.h): the conversion must round the fp32 result, not fuse with the product before it.

// y = act(h): kind 0 GELU (erf form), 1 ReLU (the training forward keeps the pre-activation h for the backward).
template <int V, typename T>
__device__ __forceinline__ void act_fwd_at(const T* h, T* y, int kind) {
    float v[V];
    loadv<V>(h, v);
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = f32_rounded(kind == 0 ? gelu_erf(v[e]) : fmaxf(v[e], 0.f));
    storev<V>(y, v);
}
// dh = dy * act'(h), in place over dy (fp32).
template <int V, typename T>
__device__ __forceinline__ void act_bwd_at(const T* h, float* dy, int kind) {
    float v[V], d[V];
    loadv<V>(h, v);
    loadv<V>(dy, d);
#pragma unroll
    for (int e = 0; e < V; ++e) d[e] *= act_deriv(v[e], kind);
    storev<V>(dy, d);
}
// groups of V elements, then threads 0 .. n % V - 1 of the grid take the ragged tail one element each
template <typename T, int V>
__global__ __launch_bounds__(256) void act_fwd_kernel(const T* __restrict__ h, T* __restrict__ y, int64_t n, int kind) {
    const int64_t nv = n / V, gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = gid; i < nv; i += (int64_t)gridDim.x * blockDim.x) act_fwd_at<V>(h + V * i, y + V * i, kind);
    if (gid < n % V) act_fwd_at<1>(h + V * nv + gid, y + V * nv + gid, kind);
}
template <typename T, int V>
__global__ __launch_bounds__(256) void act_bwd_kernel(const T* __restrict__ h, float* __restrict__ dy, int64_t n, int kind) {
    const int64_t nv = n / V, gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = gid; i < nv; i += (int64_t)gridDim.x * blockDim.x) act_bwd_at<V>(h + V * i, dy + V * i, kind);
    if (gid < n % V) act_bwd_at<1>(h + V * nv + gid, dy + V * nv + gid, kind);
}

// SwiGLU (layers/swiglu_ffn.py:54-72) on rows x12 = [x1 | x2] of 2 H columns of T: h[r][c] = silu(x1[r][c]) x2[r][c] in T, and with
// s = sigmoid(x1) the fp32 dx12[r] = [dh x2 s (1 + x1 (1 - s)) | dh x1 s].  One thread per V columns of h (V = 8 needs H % 8 == 0: every
// half row is then 16-byte aligned); no reduction, one form for both determinism modes.
template <typename T, int V>
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const T* __restrict__ x12, T* __restrict__ h, int64_t rows, int H) {
    const int hv = H / V;
    const int64_t n = rows * hv;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / hv;
        const int c = (int)(i - r * hv) * V;
        float a[V], b[V];
        loadv<V>(x12 + r * 2 * H + c, a);
        loadv<V>(x12 + r * 2 * H + c + H, b);
#pragma unroll
        for (int e = 0; e < V; ++e) a[e] = f32_rounded(swiglu_fwd_value(a[e], b[e]));
        storev<V>(h + r * H + c, a);
    }
}
template <typename T, int V>
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const T* __restrict__ x12, const float* __restrict__ dh, float* __restrict__ dx12,
                                                         int64_t rows, int H) {
    const int hv = H / V;
    const int64_t n = rows * hv;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / hv;
        const int c = (int)(i - r * hv) * V;
        const int64_t o = r * 2 * H + c;
        float a[V], b[V], d[V], d1[V], d2[V];
        loadv<V>(x12 + o, a);
        loadv<V>(x12 + o + H, b);
        loadv<V>(dh + r * H + c, d);
#pragma unroll
        for (int e = 0; e < V; ++e) swiglu_bwd_values(a[e], b[e], d[e], &d1[e], &d2[e]);
        storev<V>(dx12 + o, d1);
        storev<V>(dx12 + o + H, d2);
    }
}

// y[i][j] = alpha * x[i][j] * (g ? g[j] : 1) + beta * y[i][j]   (LayerScale on a gradient; residual sums; plain scaling)
__global__ void axpby_cols_kernel(const float* __restrict__ x, int64_t xs, const float* __restrict__ g, float alpha, float beta,
                                  float* __restrict__ y, int64_t ys, int64_t rows, int cols) {
    const int64_t n = rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / cols;
        const int c = (int)(i - r * cols);
        const float v = alpha * x[r * xs + c] * (g ? g[c] : 1.f);
        float* o = y + r * ys + c;
        *o = v + (beta != 0.f ? beta * *o : 0.f);
    }
}

// rows of 14 x 14 pixels: col[(n*Np + p)][ky*14 + kx] = vol[n][py*14 + ky][px*14 + kx]
template <typename T>
__global__ void im2col14_kernel(const T* __restrict__ vol, int H, int W, int gw, int Np, int64_t total, float* __restrict__ col) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / 196;
        const int k = (int)(i - row * 196), ky = k / 14, kx = k - ky * 14;
        const int64_t n = row / Np;
        const int p = (int)(row - n * Np), py = p / gw, px = p - py * gw;
        col[i] = to_f32(vol[(n * H + py * 14 + ky) * W + px * 14 + kx]);
    }
}

// adjoint of pos_interp_kernel: dpos[yy][xx][e] += wy[a] wx[b] dout[oy][ox][e]
__global__ void pos_interp_bwd_kernel(const float* __restrict__ dout, int M, int E, int gh, int gw, float scale_y, float scale_x,
                                      float* __restrict__ dpos) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)gh * gw * E) return;
    const int e = (int)(i % E);
    const int ox = (int)((i / E) % gw);
    const int oy = (int)(i / ((int64_t)E * gw));
    const float ry = scale_y * ((float)oy + 0.5f) - 0.5f;
    const float rx = scale_x * ((float)ox + 0.5f) - 0.5f;
    const int iy = (int)floorf(ry), ix = (int)floorf(rx);
    float wy[4], wx[4];
    cubic_w(ry - (float)iy, wy);
    cubic_w(rx - (float)ix, wx);
    const float d = dout[i];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int yy = min(max(iy - 1 + a, 0), M - 1);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int xx = min(max(ix - 1 + b, 0), M - 1);
            atomicAdd(dpos + ((int64_t)yy * M + xx) * E + e, wy[a] * wx[b] * d);
        }
    }
}

inline unsigned grid_for(int64_t n, int block = 256, int cap = 16384) {
    const int64_t gneed = (n + block - 1) / block;
    return (unsigned)(gneed < 1 ? 1 : (gneed > cap ? cap : gneed));
}

}  // namespace

int launch_softmax_rows(float* S, const uint8_t* mask, int64_t rows, int L, int rows_per_b, hipStream_t s) {
    softmax_rows_kernel<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s>>>(S, mask, rows, L, rows_per_b);
    return mst_check_launch("softmax_rows");
}

int launch_softmax_rows_bwd(const float* P, float* dP, int64_t rows, int L, float scale, hipStream_t s) {
    softmax_rows_bwd_kernel<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s>>>(P, dP, rows, L, scale);
    return mst_check_launch("softmax_rows_bwd");
}

// four rows per wave at least, 1,024 workgroups at most (the d gamma / d beta atomics or slabs are per workgroup); a function of rows
// only: so is the summation order of the ordered form
static unsigned layernorm_bwd_grid(int64_t rows) { return (unsigned)(rows < 16 ? 1 : (rows / 16 < 1024 ? rows / 16 : 1024)); }

template <bool SLAB>
static int layernorm_bwd_go(const char* what, const float* x, int64_t xs, const float* gamma, const float* dy, int64_t dys, const float* dres,
                            int64_t drs, float* dx, int64_t dxs, float* dgamma, float* dbeta, int64_t rows, int cols, float eps, float* slab,
                            hipStream_t s) {
    MST_CHECK_ARG(cols > 0 && cols <= 2048, "%s: cols=%d unsupported (<= 2048)", what, cols);
    const auto kernel = cols <= 128    ? layernorm_bwd_kernel<2, SLAB>
                        : cols <= 384  ? layernorm_bwd_kernel<6, SLAB>
                        : cols <= 768  ? layernorm_bwd_kernel<12, SLAB>
                        : cols <= 1024 ? layernorm_bwd_kernel<16, SLAB>
                                       : layernorm_bwd_kernel<32, SLAB>;
    kernel<<<dim3(layernorm_bwd_grid(rows)), dim3(256), 0, s>>>(x, xs, gamma, dy, dys, dres, drs, dx, dxs, dgamma, dbeta, rows, cols, eps, slab);
    return mst_check_launch(what);
}

int launch_layernorm_bwd(const float* x, int64_t xs, const float* gamma, const float* dy, int64_t dys, const float* dres, int64_t drs,
                         float* dx, int64_t dxs, float* dgamma, float* dbeta, int64_t rows, int cols, float eps, hipStream_t s) {
    return layernorm_bwd_go<false>("layernorm_bwd", x, xs, gamma, dy, dys, dres, drs, dx, dxs, dgamma, dbeta, rows, cols, eps, nullptr, s);
}

size_t layernorm_bwd_ordered_workspace_bytes(int64_t rows, int cols) {
    return rows > 0 && cols > 0 ? ((size_t)layernorm_bwd_grid(rows) * 2 * cols * sizeof(float) + 255) / 256 * 256 : 0;
}

int launch_layernorm_bwd_ordered(const float* x, int64_t xs, const float* gamma, const float* dy, int64_t dys, const float* dres, int64_t drs,
                                 float* dx, int64_t dxs, float* dgamma, float* dbeta, int64_t rows, int cols, float eps, void* ws,
                                 size_t ws_bytes, hipStream_t s) {
    const size_t need = layernorm_bwd_ordered_workspace_bytes(rows, cols);
    MST_CHECK_ARG(ws && ws_bytes >= need, "layernorm_bwd_ordered: workspace of %zu bytes, %zu needed", ws_bytes, need);
    float* slab = (float*)ws;
    int rc = layernorm_bwd_go<true>("layernorm_bwd_ordered", x, xs, gamma, dy, dys, dres, drs, dx, dxs, dgamma, dbeta, rows, cols, eps, slab, s);
    if (rc || (!dgamma && !dbeta)) return rc;
    return launch_slab_reduce(slab, layernorm_bwd_grid(rows), 2 * (int64_t)cols, cols, dgamma, dbeta, s);
}

int launch_rope_rows(float* qkv, int64_t rows, int L, int heads, int hd, const float* freqs, float sign, hipStream_t s) {
    MST_CHECK_ARG(qkv && freqs && rows > 0 && L > 0 && heads > 0 && hd > 0 && hd % 2 == 0, "rope_rows: bad arguments");
    rope_rows_kernel<<<dim3(grid_for(rows * heads * hd)), dim3(256), 0, s>>>(qkv, rows, L, heads, hd, freqs, sign);
    return mst_check_launch("rope_rows");
}

// The elementwise launchers: V = 8 when `v8` (every base 16-byte aligned; SwiGLU: H % 8 == 0 as well), one element per thread otherwise.
// The fp32 entry points take any pointer; the 16-bit ones refuse misaligned bases, so act has no 16-bit V = 1 kernel.
template <typename T>
static int act_fwd_t(const char* what, const void* h, void* y, int64_t n, int kind, bool v8, hipStream_t s) {
    if (v8) act_fwd_kernel<T, 8><<<dim3(grid_for(n >> 3)), dim3(256), 0, s>>>((const T*)h, (T*)y, n, kind);
    else if constexpr (sizeof(T) == 4) act_fwd_kernel<T, 1><<<dim3(grid_for(n)), dim3(256), 0, s>>>((const T*)h, (T*)y, n, kind);
    return mst_check_launch(what);
}
template <typename T>
static int act_bwd_t(const char* what, const void* h, float* dy, int64_t n, int kind, bool v8, hipStream_t s) {
    if (v8) act_bwd_kernel<T, 8><<<dim3(grid_for(n >> 3)), dim3(256), 0, s>>>((const T*)h, dy, n, kind);
    else if constexpr (sizeof(T) == 4) act_bwd_kernel<T, 1><<<dim3(grid_for(n)), dim3(256), 0, s>>>((const T*)h, dy, n, kind);
    return mst_check_launch(what);
}
template <typename T>
static int swiglu_fwd_t(const char* what, const void* x12, void* h, int64_t rows, int H, bool v8, hipStream_t s) {
    if (v8) swiglu_fwd_kernel<T, 8><<<dim3(grid_for(rows * (H / 8))), dim3(256), 0, s>>>((const T*)x12, (T*)h, rows, H);
    else swiglu_fwd_kernel<T, 1><<<dim3(grid_for(rows * H)), dim3(256), 0, s>>>((const T*)x12, (T*)h, rows, H);
    return mst_check_launch(what);
}
template <typename T>
static int swiglu_bwd_t(const char* what, const void* x12, const float* dh, float* dx12, int64_t rows, int H, bool v8, hipStream_t s) {
    if (v8) swiglu_bwd_kernel<T, 8><<<dim3(grid_for(rows * (H / 8))), dim3(256), 0, s>>>((const T*)x12, dh, dx12, rows, H);
    else swiglu_bwd_kernel<T, 1><<<dim3(grid_for(rows * H)), dim3(256), 0, s>>>((const T*)x12, dh, dx12, rows, H);
    return mst_check_launch(what);
}

int launch_act_fwd(const float* h, float* y, int64_t n, int kind, hipStream_t s) {
    return act_fwd_t<float>("act_fwd", h, y, n, kind, aligned(h, 16) && aligned(y, 16), s);
}

int launch_act_bwd(const float* h, float* dy, int64_t n, int kind, hipStream_t s) {
    return act_bwd_t<float>("act_bwd", h, dy, n, kind, aligned(h, 16) && aligned(dy, 16), s);
}

int launch_swiglu_fwd(const float* x12, float* h, int64_t rows, int H, hipStream_t s) {
    return swiglu_fwd_t<float>("swiglu_fwd", x12, h, rows, H, H % 8 == 0 && aligned(x12, 16) && aligned(h, 16), s);
}

int launch_swiglu_bwd(const float* x12, const float* dh, float* dx12, int64_t rows, int H, hipStream_t s) {
    return swiglu_bwd_t<float>("swiglu_bwd", x12, dh, dx12, rows, H, H % 8 == 0 && aligned(x12, 16) && aligned(dh, 16) && aligned(dx12, 16), s);
}

static int bad_dtype16(const char* what, int dt) {
    mst_set_error("%s: dtype %d (bf16 / f16)", what, dt);
    return MST_EINVAL;
}

int launch_act_fwd16(const void* h, void* y, int dt, int64_t n, int kind, hipStream_t s) {
    MST_CHECK_ARG(aligned(h, 16) && aligned(y, 16), "act_fwd16: bases must be 16-byte aligned");
    if (dt == MST_BF16) return act_fwd_t<bf16_t>("act_fwd16", h, y, n, kind, true, s);
    if (dt == MST_F16) return act_fwd_t<f16_t>("act_fwd16", h, y, n, kind, true, s);
    return bad_dtype16("act_fwd16", dt);
}

int launch_act_bwd16(const void* h, int dt, float* dy, int64_t n, int kind, hipStream_t s) {
    MST_CHECK_ARG(aligned(h, 16) && aligned(dy, 16), "act_bwd16: bases must be 16-byte aligned");
    if (dt == MST_BF16) return act_bwd_t<bf16_t>("act_bwd16", h, dy, n, kind, true, s);
    if (dt == MST_F16) return act_bwd_t<f16_t>("act_bwd16", h, dy, n, kind, true, s);
    return bad_dtype16("act_bwd16", dt);
}

int launch_swiglu_fwd16(const void* x12, void* h, int dt, int64_t rows, int H, hipStream_t s) {
    MST_CHECK_ARG(aligned(x12, 16) && aligned(h, 16), "swiglu_fwd16: bases must be 16-byte aligned");
    if (dt == MST_BF16) return swiglu_fwd_t<bf16_t>("swiglu_fwd16", x12, h, rows, H, H % 8 == 0, s);
    if (dt == MST_F16) return swiglu_fwd_t<f16_t>("swiglu_fwd16", x12, h, rows, H, H % 8 == 0, s);
    return bad_dtype16("swiglu_fwd16", dt);
}

int launch_swiglu_bwd16(const void* x12, int dt, const float* dh, float* dx12, int64_t rows, int H, hipStream_t s) {
    MST_CHECK_ARG(aligned(x12, 16) && aligned(dh, 16) && aligned(dx12, 16), "swiglu_bwd16: bases must be 16-byte aligned");
    if (dt == MST_BF16) return swiglu_bwd_t<bf16_t>("swiglu_bwd16", x12, dh, dx12, rows, H, H % 8 == 0, s);
    if (dt == MST_F16) return swiglu_bwd_t<f16_t>("swiglu_bwd16", x12, dh, dx12, rows, H, H % 8 == 0, s);
    return bad_dtype16("swiglu_bwd16", dt);
}

int launch_axpby_cols(const float* x, int64_t xs, const float* g, float alpha, float beta, float* y, int64_t ys, int64_t rows,
                      int cols, hipStream_t s) {
    axpby_cols_kernel<<<dim3(grid_for(rows * cols)), dim3(256), 0, s>>>(x, xs, g, alpha, beta, y, ys, rows, cols);
    return mst_check_launch("axpby_cols");
}

int launch_im2col14(const void* vol, int dt, int n, int H, int W, float* col, hipStream_t s) {
    const int gw = W / 14, Np = (H / 14) * gw;
    const int64_t total = (int64_t)n * Np * 196;
    if (dt == MST_F32) im2col14_kernel<float><<<dim3(grid_for(total)), dim3(256), 0, s>>>((const float*)vol, H, W, gw, Np, total, col);
    else if (dt == MST_BF16) im2col14_kernel<bf16_t><<<dim3(grid_for(total)), dim3(256), 0, s>>>((const bf16_t*)vol, H, W, gw, Np, total, col);
    else if (dt == MST_F16) im2col14_kernel<f16_t><<<dim3(grid_for(total)), dim3(256), 0, s>>>((const f16_t*)vol, H, W, gw, Np, total, col);
    else { mst_set_error("im2col14: bad dtype %d", dt); return MST_EINVAL; }
    return mst_check_launch("im2col14");
}

int launch_pos_interp_bwd(const float* dout, int M, int E, int gh, int gw, double offset, float* dpos, hipStream_t s) {
    const float sy = (float)(1.0 / (((double)gh + offset) / (double)M));
    const float sx = (float)(1.0 / (((double)gw + offset) / (double)M));
    const int64_t tot = (int64_t)gh * gw * E;
    pos_interp_bwd_kernel<<<dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s>>>(dout, M, E, gh, gw, sy, sx, dpos);
    return mst_check_launch("pos_interp_bwd");
}
