// Fixed-order reductions of the training steps (torch.use_deterministic_algorithms): the forms the step takes instead of the
// floating-point atomics of col2im / max-pool backward (k_conv.hip) and the bicubic pos-embed adjoint (k_train.hip).  Every order
// below is a pure function of the shape arguments: no float atomic, no dependence on which workgroup finishes first.  (The ordered
// column sums -- colsum / colsqdev / bn_bwd_reduce -- and slab_reduce are the SLAB form of k_colsum.hip's one kernel.)
//   col2im_gather    dx[n][iy][ix][c] += sum over (ky, kx) in ascending order of the im2col entries that read this input
//   maxpool_bwd      pass 1 stores every window's first-maximum position (0..8, torch's scan order ky, kx with a strict >);
//                    pass 2 gives each input the dy of the (at most 4) windows whose argument it is, windows in ascending (oy, ox)
//   pos_interp_bwd   dpos = Wy^T . dout . Wx with the dense tap matrices (clamped taps of one output summed in ascending tap
//                    order): T = dout . Wx over ascending ox, then dpos += Wy^T . T over ascending oy
#include "mst_common.h"

namespace {

// dx[n][iy][ix][c] += sum over (ky, kx) ascending of dcol[(n, oy, ox)][(ky, kx, c)] with oy*s - p + ky = iy, ox*s - p + kx = ix
__global__ void col2im_gather_kernel(const float* __restrict__ dcol, int H, int W, int C, int kh, int kw, int stride, int pad, int Ho,
                                     int Wo, int Kpad, int64_t total, float* __restrict__ dx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int ix = (int)((i / C) % W), iy = (int)((i / ((int64_t)C * W)) % H);
        const int64_t n = i / ((int64_t)C * W * H);
        float s = dx[i];
        for (int ky = 0; ky < kh; ++ky) {
            const int ty = iy + pad - ky;
            if (ty < 0 || ty % stride) continue;
            const int oy = ty / stride;
            if (oy >= Ho) continue;
            for (int kx = 0; kx < kw; ++kx) {
                const int tx = ix + pad - kx;
                if (tx < 0 || tx % stride) continue;
                const int ox = tx / stride;
                if (ox >= Wo) continue;
                s += dcol[((n * Ho + oy) * Wo + ox) * Kpad + (ky * kw + kx) * C + c];
            }
        }
        dx[i] = s;
    }
}

// pass 1 of the max-pool backward (3 x 3, stride 2, padding 1): arg[window] = ky * 3 + kx of its first maximum (scan order ky, kx,
// strict >: the rule of maxpool_bwd_nhwc_kernel), 255 when no element beats -inf
__global__ void maxpool_arg_kernel(const float* __restrict__ x, int H, int W, int C, int Ho, int Wo, int64_t total, uint8_t* __restrict__ arg) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int ox = (int)((i / C) % Wo), oy = (int)((i / ((int64_t)C * Wo)) % Ho);
        const int64_t n = i / ((int64_t)C * Wo * Ho);
        float m = -INFINITY;
        int a = 255;
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * 2 - 1 + ky;
            if (iy < 0 || iy >= H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * 2 - 1 + kx;
                if (ix < 0 || ix >= W) continue;
                const float v = x[((n * H + iy) * W + ix) * C + c];
                if (v > m) { m = v; a = ky * 3 + kx; }
            }
        }
        arg[i] = (uint8_t)a;
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

// entry [o][m] of the dense tap matrix: the weights of output o's four taps that land on stored cell m after clamping, in tap order;
// `hit` is false when none does
__device__ __forceinline__ float tap_weight(int o, int m, float scale, int M, bool& hit) {
    const float r = scale * ((float)o + 0.5f) - 0.5f;
    const int i = (int)floorf(r);
    float w[4];
    cubic_w(r - (float)i, w);
    float s = 0.f;
    hit = false;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (min(max(i - 1 + t, 0), M - 1) == m) { s += w[t]; hit = true; }
    return s;
}
// T[oy][xx][e] = sum_{ox ascending} Wx[ox][xx] dout[oy][ox][e]
__global__ void pos_bwd_cols_kernel(const float* __restrict__ dout, int M, int E, int gh, int gw, float scale_x, float* __restrict__ T) {
    const int64_t total = (int64_t)gh * M * E;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int e = (int)(i % E);
        const int xx = (int)((i / E) % M);
        const int oy = (int)(i / ((int64_t)E * M));
        float s = 0.f;
        for (int ox = 0; ox < gw; ++ox) {
            bool hit;
            const float w = tap_weight(ox, xx, scale_x, M, hit);
            if (hit) s = fmaf(w, dout[((int64_t)oy * gw + ox) * E + e], s);
        }
        T[i] = s;
    }
}
// dpos[yy][xx][e] += sum_{oy ascending} Wy[oy][yy] T[oy][xx][e]
__global__ void pos_bwd_rows_kernel(const float* __restrict__ T, int M, int E, int gh, float scale_y, float* __restrict__ dpos) {
    const int64_t total = (int64_t)M * M * E;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int e = (int)(i % E);
        const int xx = (int)((i / E) % M);
        const int yy = (int)(i / ((int64_t)E * M));
        float s = 0.f;
        for (int oy = 0; oy < gh; ++oy) {
            bool hit;
            const float w = tap_weight(oy, yy, scale_y, M, hit);
            if (hit) s = fmaf(w, T[((int64_t)oy * M + xx) * E + e], s);
        }
        dpos[i] += s;
    }
}

inline unsigned ogrid(int64_t n) {
    const int64_t g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

inline size_t round256(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

int launch_col2im_gather(const float* dcol, int n, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad, float* dx,
                         hipStream_t s) {
    const int Ho = (H + 2 * pad - kh) / stride + 1, Wo = (W + 2 * pad - kw) / stride + 1;
    MST_CHECK_ARG(Ho > 0 && Wo > 0 && stride > 0 && Kpad >= kh * kw * C, "col2im_gather: bad geometry (Ho=%d Wo=%d Kpad=%d)", Ho, Wo, Kpad);
    const int64_t total = (int64_t)n * H * W * C;
    col2im_gather_kernel<<<dim3(ogrid(total)), dim3(256), 0, s>>>(dcol, H, W, C, kh, kw, stride, pad, Ho, Wo, Kpad, total, dx);
    return mst_check_launch("col2im_gather");
}

size_t maxpool_bwd_gather_workspace_bytes(int n, int H, int W, int C) {
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    return n > 0 && H > 0 && W > 0 && C > 0 ? round256((size_t)n * Ho * Wo * C) : 0;
}

int launch_maxpool_bwd_gather(const float* x, const float* dy, int n, int H, int W, int C, float* dx, void* ws, size_t ws_bytes, hipStream_t s) {
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    const size_t need = maxpool_bwd_gather_workspace_bytes(n, H, W, C);
    MST_CHECK_ARG(ws && ws_bytes >= need, "maxpool_bwd_gather: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const int64_t windows = (int64_t)n * Ho * Wo * C;
    maxpool_arg_kernel<<<dim3(ogrid(windows)), dim3(256), 0, s>>>(x, H, W, C, Ho, Wo, windows, (uint8_t*)ws);
    int rc = mst_check_launch("maxpool_arg");
    if (rc) return rc;
    return launch_maxpool_bwd_from_args((const uint8_t*)ws, dy, n, H, W, C, dx, s);
}

// pass 2 alone, on first-maximum codes some pass 1 stored (maxpool_arg_kernel here, its 16-bit-input twin in k_bn16.hip)
int launch_maxpool_bwd_from_args(const uint8_t* ws, const float* dy, int n, int H, int W, int C, float* dx, hipStream_t s) {
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    const int64_t total = (int64_t)n * H * W * C;
    const bool v4 = C % 4 == 0 && (reinterpret_cast<uintptr_t>(dx) & 15) == 0 && (reinterpret_cast<uintptr_t>(dy) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(ws) & 3) == 0;            // the same sums in the same order either way
    if (v4) maxpool_bwd_gather_kernel<true><<<dim3(ogrid(total / 4)), dim3(256), 0, s>>>(ws, dy, H, W, C, Ho, Wo, total, dx);
    else maxpool_bwd_gather_kernel<false><<<dim3(ogrid(total)), dim3(256), 0, s>>>(ws, dy, H, W, C, Ho, Wo, total, dx);
    return mst_check_launch("maxpool_bwd_gather");
}

size_t pos_interp_bwd_ordered_workspace_bytes(int M, int E, int gh, int gw) {
    return M > 0 && E > 0 && gh > 0 && gw > 0 ? round256(sizeof(float) * (size_t)gh * M * E) : 0;
}

int launch_pos_interp_bwd_ordered(const float* dout, int M, int E, int gh, int gw, double offset, float* dpos, void* ws, size_t ws_bytes,
                                  hipStream_t s) {
    const size_t need = pos_interp_bwd_ordered_workspace_bytes(M, E, gh, gw);
    MST_CHECK_ARG(ws && ws_bytes >= need, "pos_interp_bwd_ordered: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const float sy = (float)(1.0 / (((double)gh + offset) / (double)M));     // the scales of launch_pos_interp_bwd
    const float sx = (float)(1.0 / (((double)gw + offset) / (double)M));
    float* T = (float*)ws;
    pos_bwd_cols_kernel<<<dim3(ogrid((int64_t)gh * M * E)), dim3(256), 0, s>>>(dout, M, E, gh, gw, sx, T);
    int rc = mst_check_launch("pos_bwd_cols");
    if (rc) return rc;
    pos_bwd_rows_kernel<<<dim3(ogrid((int64_t)M * M * E)), dim3(256), 0, s>>>(T, M, E, gh, sy, dpos);
    return mst_check_launch("pos_bwd_rows");
}
