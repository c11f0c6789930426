// mst_conv_dgrad_stem: the data gradient of a thin-input convolution -- the stem of the ResNet models (torchvision conv1: 7 x 7, stride 2,
// padding 3, 64 output channels; reference resnet.py:176 repeats the grey slice into three identical channels, which the forward folds
// into ONE input channel with the three kernels summed).  It is the last link of the gradient with respect to the input volume.
//   dx[s, y, x, c] = sum over (ky, kx) with y + pad - ky = stride oy, x + pad - kx = stride ox, (oy, ox) inside the output
//                    of  sum_co dz[s, oy, ox, co] * Wg[co, (ky, kx, c)]
// Every product dz[row][co] * Wg[co][tap] belongs to exactly one input pixel, so the work is the GEMM dcol[rows, taps] = dz . Wg followed
// by the adjoint of im2col.  Per workgroup: a tile x tile square of input pixels of one image and the <= 128 output positions that reach
// it (the halo: 11 x 11 for a 16 x 16 tile of the stem).  Wave w owns positions [32 w, 32 w + 32): it reads its dz rows ONCE from global
// memory straight into MFMA A fragments (lane = one position, one half of the channels: the exact-fp32 v_mfma_f32_32x32x2_f32 sums over
// k in any order, so lanes 0-31 take channels [0, Cout/2) and lanes 32-63 the rest, and a lane's operands are contiguous in memory), 16-bit
// dz widened on the way.  Then per input channel c: the weight columns of c (k*k taps, padded to 64) staged in LDS as the B operand,
// Cout/2 MFMA steps per 32-column block, the [positions, taps] product written to LDS -- it never reaches HBM -- and every input pixel of
// the tile gathers its <= ceil(k/stride)^2 taps from there in ascending (ky, kx) order and writes its own dx element.
// No atomics, no workspace: every dx element is written exactly once and its summation order is fixed by the shape arguments.
#include "mst_common.h"

namespace {

constexpr int PMAX = 128;              // output positions per workgroup (four waves x one 32-row MFMA block)
constexpr int NC = 64;                 // taps per channel, padded (k <= 7: 49)
constexpr int LDD = NC + 1;            // Ds[position][tap]: neighbouring positions one bank apart for the gather
constexpr int MAXT = 16;               // largest tile edge: 256 pixels, one per thread

template <typename T> __device__ __forceinline__ void load4(const T* p, float* o) {
    if constexpr (std::is_same<T, float>::value) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    } else {
        const typename V8<T>::half_type v = *reinterpret_cast<const typename V8<T>::half_type*>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (float)v[i];
    }
}

// first output index whose window can reach input index i0: ceil((i0 + pad - (k - 1)) / stride), the numerator may be negative
__device__ __host__ __forceinline__ int first_out(int i0, int pad, int k, int stride) {
    const int a = i0 + pad - (k - 1);
    return a >= 0 ? (a + stride - 1) / stride : -((-a) / stride);
}

template <typename T, int HALF>        // HALF = Cout / 2: MFMA steps per 32-column block
__global__ __launch_bounds__(256) void stem_dgrad_kernel(const T* __restrict__ dz, const T* __restrict__ Wg, int Ho, int Wo, int k, int stride,
                                                         int pad, int H, int W, int Cin, int tile, int pw, int tiles_x, int tiles_y,
                                                         float* __restrict__ dx) {
    constexpr int Cout = 2 * HALF;
    __shared__ float Ds[PMAX * LDD];
    __shared__ float Bs[Cout * NC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
    const int bid = blockIdx.x;
    const int tx = bid % tiles_x, ty = (bid / tiles_x) % tiles_y, img = bid / (tiles_x * tiles_y);
    const int y0 = ty * tile, x0 = tx * tile;
    const int oy0 = first_out(y0, pad, k, stride), ox0 = first_out(x0, pad, k, stride);
    const int P = pw * pw, taps = k * k, K = taps * Cin;
    const bool wave_on = wave * 32 < P;                // wave-uniform: a small tile needs fewer than 128 positions
    const int ncb = taps > 32 ? 2 : 1;

    // A fragments: position wave * 32 + l31, channels [hi * HALF, hi * HALF + HALF)
    float a[HALF];
#pragma unroll
    for (int i = 0; i < HALF; ++i) a[i] = 0.f;
    {
        const int p = wave * 32 + l31;
        const int oy = oy0 + p / pw, ox = ox0 + p % pw;
        if (p < P && oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) {
            const T* src = dz + (((int64_t)img * Ho + oy) * Wo + ox) * Cout + hi * HALF;
#pragma unroll
            for (int i = 0; i < HALF; i += 4) load4<T>(src + i, a + i);
        }
    }
    for (int c = 0; c < Cin; ++c) {
        // B operand of channel c: Bs[co][tap] = Wg[co][(tap, c)], zero beyond the k * k taps
        for (int idx = tid; idx < Cout * NC; idx += 256) {
            const int co = idx >> 6, t = idx & 63;
            Bs[idx] = t < taps ? to_f32(Wg[(int64_t)co * K + t * Cin + c]) : 0.f;
        }
        __syncthreads();                               // Bs ready; the previous channel's gather has left Ds
        if (wave_on) {
            f32x16 acc0, acc1;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
            const float* brow = Bs + hi * HALF * NC + l31;
#pragma unroll
            for (int kk = 0; kk < HALF; ++kk) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], brow[kk * NC], acc0, 0, 0, 0);
                if (ncb > 1) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], brow[kk * NC + 32], acc1, 0, 0, 0);
            }
            float* drow = Ds + (wave * 32 + 4 * hi) * LDD + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2);
                drow[row * LDD] = acc0[r];
                if (ncb > 1) drow[row * LDD + 32] = acc1[r];
            }
        }
        __syncthreads();
        // adjoint of im2col: every pixel of the tile sums its own taps, ascending (ky, kx)
        for (int idx = tid; idx < tile * tile; idx += 256) {
            const int ly = idx / tile, lx = idx - ly * tile;
            const int y = y0 + ly, x = x0 + lx;
            if (y >= H || x >= W) continue;
            float sum = 0.f;
            for (int ky = (y + pad) % stride; ky < k; ky += stride) {
                const int oy = (y + pad - ky) / stride;
                if (y + pad - ky < 0 || oy >= Ho) continue;
                for (int kx = (x + pad) % stride; kx < k; kx += stride) {
                    const int ox = (x + pad - kx) / stride;
                    if (x + pad - kx < 0 || ox >= Wo) continue;
                    sum += Ds[((oy - oy0) * pw + (ox - ox0)) * LDD + ky * k + kx];
                }
            }
            dx[(((int64_t)img * H + y) * W + x) * Cin + c] = sum;
        }
    }
}

template <typename T, int HALF>
int launch_one(const void* dz, const void* Wg, int n, int Ho, int Wo, int k, int stride, int pad, int H, int W, int Cin, float* dx, hipStream_t s) {
    int tile = MAXT, pw = 0;
    for (;; tile >>= 1) {                              // the largest tile whose halo fits the 128 MFMA rows (k <= 7: tile 2 always does)
        pw = (tile + k - 2) / stride + 1;
        if (pw * pw <= PMAX) break;
    }
    const int tiles_x = (W + tile - 1) / tile, tiles_y = (H + tile - 1) / tile;
    const int64_t blocks = (int64_t)n * tiles_x * tiles_y;
    MST_CHECK_ARG(blocks < (1ll << 31), "conv_dgrad_stem: %lld tiles out of range", (long long)blocks);
    stem_dgrad_kernel<T, HALF><<<dim3((unsigned)blocks), dim3(256), 0, s>>>((const T*)dz, (const T*)Wg, Ho, Wo, k, stride, pad, H, W, Cin, tile, pw,
                                                                           tiles_x, tiles_y, dx);
    return mst_check_launch("conv_dgrad_stem");
}

template <typename T>
int launch_typed(const void* dz, const void* Wg, int n, int Ho, int Wo, int Cout, int k, int stride, int pad, int H, int W, int Cin, float* dx,
                 hipStream_t s) {
    switch (Cout) {
        case 16: return launch_one<T, 8>(dz, Wg, n, Ho, Wo, k, stride, pad, H, W, Cin, dx, s);
        case 32: return launch_one<T, 16>(dz, Wg, n, Ho, Wo, k, stride, pad, H, W, Cin, dx, s);
        case 64: return launch_one<T, 32>(dz, Wg, n, Ho, Wo, k, stride, pad, H, W, Cin, dx, s);
    }
    mst_set_error("conv_dgrad_stem: Cout=%d must be 16, 32 or 64", Cout);
    return MST_EINVAL;
}

}  // namespace

int launch_conv_dgrad_stem(const void* dz, int dt, int n, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, const void* Wg, int H, int W_,
                           int Cin, float* dx, hipStream_t s) {
    MST_CHECK_ARG(dz && Wg && dx && n > 0 && Ho > 0 && Wo > 0 && H > 0 && W_ > 0, "conv_dgrad_stem: bad arguments");
    MST_CHECK_ARG(Cin >= 1 && Cin <= 3, "conv_dgrad_stem: Cin=%d (1, 2 or 3: wider inputs are mst_conv_dgrad's)", Cin);
    MST_CHECK_ARG(kh == kw && kh >= 1 && kh <= 7, "conv_dgrad_stem: kernel %d x %d (square, at most 7 x 7)", kh, kw);
    MST_CHECK_ARG(stride == 1 || stride == 2, "conv_dgrad_stem: stride %d (1 or 2)", stride);
    MST_CHECK_ARG(pad >= 0 && pad < kh, "conv_dgrad_stem: padding %d of a %d x %d kernel", pad, kh, kw);
    MST_CHECK_ARG(Cout == 16 || Cout == 32 || Cout == 64, "conv_dgrad_stem: Cout=%d must be 16, 32 or 64", Cout);
    MST_CHECK_ARG((H + 2 * pad - kh) / stride + 1 == Ho && (W_ + 2 * pad - kw) / stride + 1 == Wo,
                  "conv_dgrad_stem: %d x %d is not the output of a %d x %d input", Ho, Wo, H, W_);
    MST_CHECK_ARG(((uintptr_t)dz & 15) == 0 && ((uintptr_t)dx & 3) == 0, "conv_dgrad_stem: dz must be 16-byte aligned");
    switch (dt) {
        case MST_F32: return launch_typed<float>(dz, Wg, n, Ho, Wo, Cout, kh, stride, pad, H, W_, Cin, dx, s);
        case MST_F16: return launch_typed<f16_t>(dz, Wg, n, Ho, Wo, Cout, kh, stride, pad, H, W_, Cin, dx, s);
        case MST_BF16: return launch_typed<bf16_t>(dz, Wg, n, Ho, Wo, Cout, kh, stride, pad, H, W_, Cin, dx, s);
    }
    mst_set_error("conv_dgrad_stem: operand dtype %d (f32 / bf16 / f16)", dt);
    return MST_EINVAL;
}
