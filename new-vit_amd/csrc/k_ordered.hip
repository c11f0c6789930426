// Fixed-order reductions of the training steps (torch.use_deterministic_algorithms): the forms the step takes instead of the
// floating-point atomics of col2im (k_conv.hip) and the bicubic pos-embed adjoint (k_train.hip).  Every order below is a pure function
// of the shape arguments: no float atomic, no dependence on which workgroup finishes first.  (The ordered column sums -- colsum and the
// BatchNorm sums -- and slab_reduce are the SLAB form of k_colsum.hip's one kernel; the gather form of the max-pool backward is beside
// the other pooling kernels in k_bn.hip.)
//   col2im_gather    dx[n][iy][ix][c] += sum over (ky, kx) in ascending order of the im2col entries that read this input
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

}  // namespace

int launch_col2im_gather(const float* dcol, int n, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad, float* dx,
                         hipStream_t s) {
    const int Ho = (H + 2 * pad - kh) / stride + 1, Wo = (W + 2 * pad - kw) / stride + 1;
    MST_CHECK_ARG(Ho > 0 && Wo > 0 && stride > 0 && Kpad >= kh * kw * C, "col2im_gather: bad geometry (Ho=%d Wo=%d Kpad=%d)", Ho, Wo, Kpad);
    const int64_t total = (int64_t)n * H * W * C;
    col2im_gather_kernel<<<dim3(grid256(total)), dim3(256), 0, s>>>(dcol, H, W, C, kh, kw, stride, pad, Ho, Wo, Kpad, total, dx);
    return mst_check_launch("col2im_gather");
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
    pos_bwd_cols_kernel<<<dim3(grid256((int64_t)gh * M * E)), dim3(256), 0, s>>>(dout, M, E, gh, gw, sx, T);
    int rc = mst_check_launch("pos_bwd_cols");
    if (rc) return rc;
    pos_bwd_rows_kernel<<<dim3(grid256((int64_t)M * M * E)), dim3(256), 0, s>>>(T, M, E, gh, sy, dpos);
    return mst_check_launch("pos_bwd_rows");
}
