// Convolutional backbone pieces for the ResNet models (reference mst/models/resnet.py:44-50,127-243 build on
// torchvision's resnet34, whose source is not part of the reference tree: the published architecture is restated).
// Activations are NHWC fp32 ([n*H*W, C] row-major), so that a convolution is  im2col -> GEMM(A . W^T + folded BatchNorm) with the
// existing exact-fp32 MFMA GEMM and its bias / ReLU / residual epilogues, and its output is the next layer's input as it stands.
//   im2col_nhwc   col[(n, oy, ox)][(ky, kx, c)] = x[n][oy*s - p + ky][ox*s - p + kx][c] (0 outside), K padded with zeros to Kpad
//   col2im_nhwc   the adjoint of im2col_nhwc, by atomics (the fixed-order gather form: k_ordered.hip)
// The pools, and BatchNorm with batch statistics, are in k_bn.hip.
#include "mst_common.h"

namespace {

template <typename OutT>
__global__ void im2col_nhwc_kernel(const float* __restrict__ x, int H, int W, int C, int kh, int kw, int stride, int pad, int Ho,
                                   int Wo, int K, int Kpad, int64_t rows, OutT* __restrict__ col) {
    const int64_t total = rows * Kpad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / Kpad;
        const int k = (int)(i - r * Kpad);
        float v = 0.f;
        if (k < K) {
            const int c = k % C, kx = (k / C) % kw, ky = k / (C * kw);
            const int ox = (int)(r % Wo), oy = (int)((r / Wo) % Ho);
            const int64_t n = r / ((int64_t)Wo * Ho);
            const int iy = oy * stride - pad + ky, ix = ox * stride - pad + kx;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = x[((n * H + iy) * W + ix) * C + c];
        }
        col[i] = (OutT)v;
    }
}

// adjoint of im2col_nhwc: dx[n][iy][ix][c] += dcol[(n,oy,ox)][(ky,kx,c)]
__global__ void col2im_nhwc_kernel(const float* __restrict__ dcol, int H, int W, int C, int kh, int kw, int stride, int pad, int Ho,
                                   int Wo, int K, int Kpad, int64_t rows, float* __restrict__ dx) {
    const int64_t total = rows * K;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / K;
        const int k = (int)(i - r * K);
        const int c = k % C, kx = (k / C) % kw, ky = k / (C * kw);
        const int ox = (int)(r % Wo), oy = (int)((r / Wo) % Ho);
        const int64_t n = r / ((int64_t)Wo * Ho);
        const int iy = oy * stride - pad + ky, ix = ox * stride - pad + kx;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) atomicAdd(dx + ((n * H + iy) * W + ix) * C + c, dcol[r * Kpad + k]);
    }
}

// Grad-CAM++ of the LAST ReLU output (reference resnet.py:66-68 + 93-118; the only map its getter exposes).  The loss is the sum of
// every image's largest output, so d loss / d pooled feature c = W[argmax][c] (or [c == argmax] without an fc); behind the global
// average pool the gradient of every position of channel c is that / HW, so the weights of equation 19 have a closed form per (n, c).
// state[0] = min, state[1] = max of the rectified maps (as uint bit patterns: the values are >= 0).
__global__ void gradcampp_kernel(const float* __restrict__ act, const float* __restrict__ out, int O, const float* __restrict__ W,
                                 int HW, int C, float* __restrict__ cam, unsigned* __restrict__ state) {
    extern __shared__ float wsh[];                                      // [C] weights of this image
    __shared__ int arg_sh;
    const int n = blockIdx.x;
    const float* a = act + (int64_t)n * HW * C;
    if (threadIdx.x == 0) {                                             // first maximum, as torch.argmax
        int arg = 0;
        float m = out[(int64_t)n * O];
        for (int o = 1; o < O; ++o) { const float v = out[(int64_t)n * O + o]; if (v > m) { m = v; arg = o; } }
        arg_sh = arg;
    }
    __syncthreads();
    const int arg = arg_sh;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float sa = 0.f;
        for (int p = 0; p < HW; ++p) sa += a[(int64_t)p * C + c];
        const float gr = (W ? W[(int64_t)arg * C + c] : (c == arg ? 1.f : 0.f)) / (float)HW;
        const float g2 = gr * gr, g3 = g2 * gr;
        float den = 2.f * g2 + sa * g3 + 1e-6f;
        if (den == 0.f) den = 1.f;
        wsh[c] = (float)HW * fmaxf(gr, 0.f) * (g2 / den);
    }
    __syncthreads();
    for (int p = threadIdx.x; p < HW; p += blockDim.x) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s = fmaf(wsh[c], a[(int64_t)p * C + c], s);
        s = fmaxf(s, 0.f);
        cam[(int64_t)n * HW + p] = s;
        atomicMin(state + 0, __float_as_uint(s));
        atomicMax(state + 1, __float_as_uint(s));
    }
}
__global__ void gradcam_norm_kernel(float* cam, int64_t total, const float* __restrict__ state) {
    const float mn = state[0], mx = state[1] - state[0];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        cam[i] = (cam[i] - mn) / mx;
}

}  // namespace

int launch_im2col_nhwc(const float* x, int n, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad, float* col,
                       hipStream_t s) {
    const int Ho = (H + 2 * pad - kh) / stride + 1, Wo = (W + 2 * pad - kw) / stride + 1, K = kh * kw * C;
    MST_CHECK_ARG(Ho > 0 && Wo > 0 && Kpad >= K, "im2col: bad geometry (Ho=%d Wo=%d K=%d Kpad=%d)", Ho, Wo, K, Kpad);
    const int64_t rows = (int64_t)n * Ho * Wo;
    im2col_nhwc_kernel<float><<<dim3(grid256(rows * Kpad)), dim3(256), 0, s>>>(x, H, W, C, kh, kw, stride, pad, Ho, Wo, K, Kpad, rows, col);
    return mst_check_launch("im2col_nhwc");
}

// the same rows rounded to a 16-bit type on the way out (the stem of the 16-bit inference backbone: its im2col rows are the "pixels" of a
// 1 x 1 mst_conv_gemm16)
int launch_im2col_nhwc16(const float* x, int n, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad, void* col, int dt, hipStream_t s) {
    const int Ho = (H + 2 * pad - kh) / stride + 1, Wo = (W + 2 * pad - kw) / stride + 1, K = kh * kw * C;
    MST_CHECK_ARG(Ho > 0 && Wo > 0 && Kpad >= K, "im2col16: bad geometry (Ho=%d Wo=%d K=%d Kpad=%d)", Ho, Wo, K, Kpad);
    const int64_t rows = (int64_t)n * Ho * Wo;
    if (dt == MST_BF16) im2col_nhwc_kernel<bf16_t><<<dim3(grid256(rows * Kpad)), dim3(256), 0, s>>>(x, H, W, C, kh, kw, stride, pad, Ho, Wo, K, Kpad, rows, (bf16_t*)col);
    else if (dt == MST_F16) im2col_nhwc_kernel<f16_t><<<dim3(grid256(rows * Kpad)), dim3(256), 0, s>>>(x, H, W, C, kh, kw, stride, pad, Ho, Wo, K, Kpad, rows, (f16_t*)col);
    else { mst_set_error("im2col16: output dtype %d (bf16 / f16)", dt); return MST_EINVAL; }
    return mst_check_launch("im2col_nhwc16");
}

int launch_col2im_nhwc(const float* dcol, int n, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad, float* dx,
                       hipStream_t s) {
    const int Ho = (H + 2 * pad - kh) / stride + 1, Wo = (W + 2 * pad - kw) / stride + 1, K = kh * kw * C;
    const int64_t rows = (int64_t)n * Ho * Wo;
    col2im_nhwc_kernel<<<dim3(grid256(rows * K)), dim3(256), 0, s>>>(dcol, H, W, C, kh, kw, stride, pad, Ho, Wo, K, Kpad, rows, dx);
    return mst_check_launch("col2im_nhwc");
}
int launch_gradcampp(const float* act, const float* out, int O, const float* W, int n, int HW, int C, float* cam, float* state,
                     hipStream_t s) {
    const unsigned init[2] = {0x7f800000u, 0u};                          // +inf, 0
    if (hipMemcpyAsync(state, init, sizeof(init), hipMemcpyHostToDevice, s) != hipSuccess) { mst_set_error("gradcampp: state init failed"); return MST_ELAUNCH; }
    gradcampp_kernel<<<dim3(n), dim3(256), sizeof(float) * C, s>>>(act, out, O, W, HW, C, cam, (unsigned*)state);
    int rc = mst_check_launch("gradcampp");
    if (rc) return rc;
    gradcam_norm_kernel<<<dim3(grid256((int64_t)n * HW)), dim3(256), 0, s>>>(cam, (int64_t)n * HW, state);
    return mst_check_launch("gradcam_norm");
}
