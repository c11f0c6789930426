// The kernels behind the encoder API (DinoVisionTransformer.forward_features / get_intermediate_layers,
// vision_transformer.py:254-322; mst_vit_encode_features in mst_api.hip):
//
// RGB patch embedding.  Conv2d(3, E, 14, 14) on [n, 3, H, W] with three DISTINCT channels (patch_embed.py:65,75-77) as one
// contraction of K = 3 x 14 x 14 = 588, padded to 3 x 14 x 16 = 672 = 21 k-steps of 32: every (channel, kernel row) is one
// 16-element k group whose columns 14, 15 are zero on both operands, exactly the grey kernel's padding (k_patch.hip) once per channel.
//   x[s, 1+R+p, :] = sum_c conv14x14(img[s, c])[p] + bias + pos_patch[p];   x[s, r, :] = prefix[r]  (r <= R)
// A workgroup owns a 64-patch x 64-channel tile and walks the three channels: im2col of one channel and the matching 224 columns
// of the weight tile into LDS, 7 k-steps of v_mfma_f32_16x16x32 (fp32 mode: 56 of v_mfma_f32_16x16x4_f32), the accumulators
// carried across the channels.  The fused pipeline's normalised rows xn come from a LayerNorm launch behind it (mst_api.hip).
//
// Tap rows.  The residual stream behind a block as fp32 plain rows out[rows, E], optionally through a LayerNorm whose per-row
// arithmetic is layernorm_kernel's (k_layernorm.hip) statement for statement: one wave per row, two-pass statistics in registers.
// x is read as plain rows or as the fp32 image of the blocked layout (include/mst_hip.h, mst_layout_flags): in both a lane's
// two columns 128 j + 2 lane, +1 are one aligned 8-byte access.  No atomics.
//
// RGB weight gradient (mst_patch_embed_rgb_wgrad, the training side of the first kernel): see patch_rgb_wgrad_kernel below.  The input
// gradient (mst_patch_embed_rgb_dgrad) is the grey data-gradient kernel run per channel: k_patch_dgrad.hip.
#include "mst_common.h"

namespace {

constexpr int PATCH = 14, KP = 224, KPR = 3 * KP;
constexpr int TW = 2, BMP = 32 * TW, BNP = 32 * TW, WT = 16 * TW;     // 64 x 64 tiles in every mode (LDS: 58 KB / 113 KB)

template <typename T> struct RowBytes { static constexpr int v = 464; };     // 232 x 2 B (29 sixteen-byte slots: odd)
template <> struct RowBytes<float> { static constexpr int v = 225 * 4; };    // 225 dwords (odd)

template <typename InT> struct In2;
template <> struct In2<float> { typedef float2 type; };
template <> struct In2<f16_t> { typedef __attribute__((ext_vector_type(2))) f16_t type; };
template <> struct In2<bf16_t> { typedef __attribute__((ext_vector_type(2))) bf16_t type; };

// T = MFMA operand type (bf16 / f16 / float), InT = image dtype; wp [E][3][14][16] of T
template <typename T, typename InT>
__global__ __launch_bounds__(256) void patch_embed_rgb_kernel(const InT* __restrict__ img, int H, int W, int gw, int Np, int64_t total,
                                                              const T* __restrict__ wp, const float* __restrict__ bias,
                                                              const float* __restrict__ pos_patch, int n_prefix, int E,
                                                              float* __restrict__ x) {
    constexpr int RB = RowBytes<T>::v;
    typedef typename In2<InT>::type in2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const As = smem;             // [64][RB] patches
    char* const Ws = smem + BMP * RB;  // [64][RB] channels
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * BMP;
    const int n0 = blockIdx.y * BNP;
    const int N = n_prefix + Np;
    const int wm = wave >> 1, wn = wave & 1;

    f32x4 acc[TW][TW];
#pragma unroll
    for (int i = 0; i < TW; ++i)
#pragma unroll
        for (int j = 0; j < TW; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int ch = 0; ch < 3; ++ch) {
        if (ch) __syncthreads();                                       // the previous channel's fragments are read
        // ---- im2col of channel ch: (patch, ky) -> 14 pixels + 2 zeros = one 16-element k group
        for (int idx = tid; idx < BMP * PATCH; idx += 256) {
            const int pl = idx % BMP, ky = idx / BMP;
            int64_t m = m0 + pl;
            if (m >= total) m = total - 1;
            const int s = (int)(m / Np), p = (int)(m % Np);
            const int py = p / gw, px = p % gw;
            const InT* src = img + (((int64_t)s * 3 + ch) * H + py * PATCH + ky) * W + px * PATCH;
            T v[16];
#pragma unroll
            for (int e = 0; e < 7; ++e) {
                const in2 t = *reinterpret_cast<const in2*>(src + 2 * e);
                if constexpr (sizeof(InT) == 4) {
                    v[2 * e] = (T)t.x;
                    v[2 * e + 1] = (T)t.y;
                } else {
                    v[2 * e] = (T)(float)t[0];
                    v[2 * e + 1] = (T)(float)t[1];
                }
            }
            v[14] = (T)0.f;
            v[15] = (T)0.f;
            T* dst = reinterpret_cast<T*>(As + pl * RB) + ky * 16;
#pragma unroll
            for (int e = 0; e < 16; ++e) dst[e] = v[e];
        }
        // ---- weight tile: columns [224 ch, 224 ch + 224) of rows n0 .. n0+63 of wp[E][672]
        {
            constexpr int CH = KP * (int)sizeof(T) / 16;               // 16-byte chunks per row and channel
            for (int idx = tid; idx < BNP * CH; idx += 256) {
                const int r = idx / CH, c = idx % CH;
                const u32x4 t = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(wp + (int64_t)(n0 + r) * KPR + ch * KP) + c * 16);
                if constexpr (sizeof(T) == 2) {
                    *reinterpret_cast<u32x4*>(Ws + r * RB + c * 16) = t;
                } else {
                    unsigned* d = reinterpret_cast<unsigned*>(Ws + r * RB + c * 16);
                    d[0] = t[0]; d[1] = t[1]; d[2] = t[2]; d[3] = t[3];
                }
            }
        }
        __syncthreads();

        if constexpr (sizeof(T) == 2) {
            typedef typename V8<T>::type vec8;
#pragma unroll
            for (int kk = 0; kk < KP / 32; ++kk) {
                const int coff = (kk * 4 + (lane >> 4)) * 16;
                vec8 af[TW], wf[TW];
#pragma unroll
                for (int j = 0; j < TW; ++j)
                    af[j] = *reinterpret_cast<const vec8*>(As + (wm * WT + j * 16 + (lane & 15)) * RB + coff);
#pragma unroll
                for (int i = 0; i < TW; ++i)
                    wf[i] = *reinterpret_cast<const vec8*>(Ws + (wn * WT + i * 16 + (lane & 15)) * RB + coff);
#pragma unroll
                for (int i = 0; i < TW; ++i)
#pragma unroll
                    for (int j = 0; j < TW; ++j) acc[i][j] = mfma16(wf[i], af[j], acc[i][j]);
            }
        } else {
            // fp32: v_mfma_f32_16x16x4_f32, lane holds A[lane&15][k = lane>>4]
            for (int k4 = 0; k4 < KP / 4; ++k4) {
                const int kof = (k4 * 4 + (lane >> 4)) * 4;
                float af[TW], wf[TW];
#pragma unroll
                for (int j = 0; j < TW; ++j)
                    af[j] = *reinterpret_cast<const float*>(As + (wm * WT + j * 16 + (lane & 15)) * RB + kof);
#pragma unroll
                for (int i = 0; i < TW; ++i)
                    wf[i] = *reinterpret_cast<const float*>(Ws + (wn * WT + i * 16 + (lane & 15)) * RB + kof);
#pragma unroll
                for (int i = 0; i < TW; ++i)
#pragma unroll
                    for (int j = 0; j < TW; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i], af[j], acc[i][j], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: lane owns channels n..n+3 of patch m
#pragma unroll
    for (int j = 0; j < TW; ++j) {
        const int64_t m = m0 + wm * WT + j * 16 + (lane & 15);
        if (m >= total) continue;
        const int s = (int)(m / Np), p = (int)(m % Np);
        float* xr = x + ((int64_t)s * N + n_prefix + p) * E;
        const float* pr = pos_patch + (int64_t)p * E;
#pragma unroll
        for (int i = 0; i < TW; ++i) {
            const int n = n0 + wn * WT + i * 16 + (lane >> 4) * 4;
            const float4 bv = *reinterpret_cast<const float4*>(bias + n);
            const float4 pv = *reinterpret_cast<const float4*>(pr + n);
            float4 o;
            o.x = acc[i][j][0] + bv.x + pv.x;
            o.y = acc[i][j][1] + bv.y + pv.y;
            o.z = acc[i][j][2] + bv.z + pv.z;
            o.w = acc[i][j][3] + bv.w + pv.w;
            *reinterpret_cast<float4*>(xr + n) = o;
        }
    }
}

// x[s, r, :] = prefix[r] for the 1 + R prefix rows of every image
__global__ void prefix_rows_rgb_kernel(const float* __restrict__ prefix, int n_prefix, int E, int N, int n, float* __restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * n_prefix * E) return;
    const int e = (int)(i % E);
    const int r = (int)((i / E) % n_prefix);
    const int64_t s = i / ((int64_t)E * n_prefix);
    x[(s * N + r) * E + e] = prefix[r * E + e];
}

template <typename T, typename InT>
int launch_rgb_t(const void* img, int n, int H, int W, const void* wp, const float* bias, const float* prefix, int n_prefix,
                 const float* pos_patch, int E, float* x, hipStream_t s) {
    const int gw = W / PATCH, Np = (H / PATCH) * gw;
    const int64_t total = (int64_t)n * Np;
    constexpr int sh = (BMP + BNP) * RowBytes<T>::v;
    auto kern = patch_embed_rgb_kernel<T, InT>;
    static mst_lds_once lds_once;
    mst_allow_lds((const void*)kern, sh, &lds_once);
    const dim3 grid((unsigned)((total + BMP - 1) / BMP), E / BNP);
    kern<<<grid, dim3(256), sh, s>>>((const InT*)img, H, W, gw, Np, total, (const T*)wp, bias, pos_patch, n_prefix, E, x);
    int rc = mst_check_launch("patch_embed_rgb");
    if (rc) return rc;
    const int64_t tot = (int64_t)n * n_prefix * E;
    prefix_rows_rgb_kernel<<<dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s>>>(prefix, n_prefix, E, n_prefix + Np, n, x);
    return mst_check_launch("prefix_rows_rgb");
}

template <typename T>
int launch_rgb_in(const void* img, int idt, int n, int H, int W, const void* wp, const float* bias, const float* prefix, int n_prefix,
                  const float* pos_patch, int E, float* x, hipStream_t s) {
    switch (idt) {
        case MST_F32: return launch_rgb_t<T, float>(img, n, H, W, wp, bias, prefix, n_prefix, pos_patch, E, x, s);
        case MST_F16: return launch_rgb_t<T, f16_t>(img, n, H, W, wp, bias, prefix, n_prefix, pos_patch, E, x, s);
        case MST_BF16: return launch_rgb_t<T, bf16_t>(img, n, H, W, wp, bias, prefix, n_prefix, pos_patch, E, x, s);
    }
    mst_set_error("patch_embed_rgb: bad image dtype %d", idt);
    return MST_EINVAL;
}

// One wave per row.  g == nullptr: copy.  Otherwise out = (x - mean) * rstd * g + b, layernorm_kernel's arithmetic.
// IMAGE: element (r, c) of x at group r / 32, piece c / 8, slot (r % 32) + 32 * ((c / 4) % 2), position c % 4.
template <int NJ, bool IMAGE>
__global__ __launch_bounds__(256) void tap_rows_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b,
                                                       float* __restrict__ out, int64_t rows, int cols, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = IMAGE ? x + (row >> 5) * 32 * cols + (row & 31) * 4 : x + row * cols;
    float2 v[NJ];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = j * 128 + lane * 2;
        if (c < cols) {
            v[j] = *reinterpret_cast<const float2*>(IMAGE ? xr + (c >> 3) * 256 + ((c >> 2) & 1) * 128 + (c & 3) : xr + c);
            s += v[j].x + v[j].y;
        } else {
            v[j] = make_float2(0.f, 0.f);
        }
    }
    float* orow = out + row * cols;
    if (!g) {                                                          // uniform over the grid
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = j * 128 + lane * 2;
            if (c < cols) *reinterpret_cast<float2*>(orow + c) = v[j];
        }
        return;
    }
    const float inv_n = 1.0f / (float)cols;
    const float mean = wave_sum(s) * inv_n;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = j * 128 + lane * 2;
        if (c < cols) {
            const float dx = v[j].x - mean, dy = v[j].y - mean;
            q += dx * dx + dy * dy;
        }
    }
    const float rstd = rsqrtf(wave_sum(q) * inv_n + eps);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = j * 128 + lane * 2;
        if (c < cols) {
            const float2 gg = *reinterpret_cast<const float2*>(g + c);
            const float2 bb = *reinterpret_cast<const float2*>(b + c);
            const float y0 = (v[j].x - mean) * rstd * gg.x + bb.x;
            const float y1 = (v[j].y - mean) * rstd * gg.y + bb.y;
            *reinterpret_cast<float2*>(orow + c) = make_float2(y0, y1);
        }
    }
}

template <bool IMAGE>
int launch_tap_t(const float* x, const float* g, const float* b, float* out, int64_t rows, int cols, float eps, hipStream_t s) {
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    const int nj = (cols + 127) / 128;
    if (nj <= 3) tap_rows_kernel<3, IMAGE><<<grid, block, 0, s>>>(x, g, b, out, rows, cols, eps);
    else if (nj <= 6) tap_rows_kernel<6, IMAGE><<<grid, block, 0, s>>>(x, g, b, out, rows, cols, eps);
    else if (nj <= 8) tap_rows_kernel<8, IMAGE><<<grid, block, 0, s>>>(x, g, b, out, rows, cols, eps);
    else tap_rows_kernel<16, IMAGE><<<grid, block, 0, s>>>(x, g, b, out, rows, cols, eps);
    return mst_check_launch("tap_rows");
}

// ---- mst_patch_embed_rgb_wgrad: the weight gradient of the RGB patch embedding (patch_embed.py:65,75-81) as an implicit GEMM that
// reads the image in place (no three-channel im2col: 64 x 3 x 518^2 would be 206 MB of fp32):
//   dW[e][c][i][j] = sum over patch rows m = (s, p) of dx[s * tok + first + p][e] * img[s][c][14 py + i][14 px + j]
// Tile: a 256-thread workgroup owns 64 embedding channels x the 224 (staged as 256: 14 kernel rows x 16) columns of ONE input channel
// and walks the patch rows of ONE split in K-steps of 16 on the exact fp32 MFMA (v_mfma_f32_32x32x2_f32); wave w owns the 32-channel
// block w & 1 and four 32-column blocks from 4 (w >> 1) (the eighth block is all padding and skipped), the tile of k_patch_dgrad.hip with
// the roles of patch rows and channels exchanged.  LDS double-buffered, the next step's operands in registers across the MFMAs.
// Split: grid.z walks the patch rows `rows_per_split` (a multiple of the K-step; the caller picks max(256, n Np / 16 rounded up to 16): at
// most 16 partials) at a time; split z writes its own part[z][E][3][14][14] and the caller reduces them (mst_colsum, atomic or ordered).
// No atomics here.  Rows past the end of a split read as zero on both operands.
constexpr int GM = 64, GK = 16, GLDA = GM + 4, GLDB = 256 + 4;

__global__ __launch_bounds__(256) void patch_rgb_wgrad_kernel(const float* __restrict__ dx, int tok, int first, const float* __restrict__ img,
                                                              int64_t rows, int chunk, int Np, int gw, int H, int W, int E,
                                                              float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float As[2][GK][GLDA];   // As[k][channel]
    __shared__ __attribute__((aligned(16))) float Bs[2][GK][GLDB];   // Bs[k][16 i + j]  (j = 14, 15 and columns >= 224 never feed a kept result)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rb = wave & 1, cb0 = (wave >> 1) * 4;
    const int e0 = blockIdx.x * GM, ch = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.z * chunk;
    const int64_t r1 = r0 + chunk < rows ? r0 + chunk : rows;
    // thread -> patch row k = tid / 16 of the K-step: four channels 4 (tid % 16) of its gradient row, and the float2 pieces
    // (tid % 16) + 16 q < 98 (kernel row piece / 7, pixel pair piece % 7) of its 14 x 14 pixels
    const int k = tid >> 4, t16 = tid & 15;
    int boff[7], bcol[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        const int piece = t16 + 16 * q, i = piece / 7, j2 = piece % 7;
        boff[q] = i * W + 2 * j2;
        bcol[q] = 16 * i + 2 * j2;
    }
    float4 ra;
    float2 rp[7];
#define LOAD(K0)                                                                                                            \
    do {                                                                                                                    \
        const int64_t m = r0 + (K0) + k;                                                                                    \
        ra = make_float4(0.f, 0.f, 0.f, 0.f);                                                                               \
        _Pragma("unroll") for (int q = 0; q < 7; ++q) rp[q] = make_float2(0.f, 0.f);                                        \
        if (m < r1) {                                                                                                       \
            const int64_t s = m / Np;                                                                                       \
            const int p = (int)(m - s * Np), py = p / gw, px = p - py * gw;                                                 \
            ra = *reinterpret_cast<const float4*>(dx + (s * tok + first + p) * (int64_t)E + e0 + 4 * t16);                  \
            const float* pix = img + ((s * 3 + ch) * H + 14 * py) * (int64_t)W + 14 * px;                                   \
            _Pragma("unroll") for (int q = 0; q < 7; ++q)                                                                   \
                if (t16 + 16 * q < 98) rp[q] = *reinterpret_cast<const float2*>(pix + boff[q]);                             \
        }                                                                                                                   \
    } while (0)
#define STORE(BUF)                                                                                                          \
    do {                                                                                                                    \
        *reinterpret_cast<float4*>(&As[BUF][k][4 * t16]) = ra;                                                              \
        _Pragma("unroll") for (int q = 0; q < 7; ++q)                                                                       \
            if (t16 + 16 * q < 98) *reinterpret_cast<float2*>(&Bs[BUF][k][bcol[q]]) = rp[q];                                \
    } while (0)
    f32x16 acc0, acc1, acc2, acc3;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = acc2[r] = acc3[r] = 0.f;
    const int len = (int)(r1 - r0);
    LOAD(0);
    STORE(0);
    __syncthreads();
    const bool has3 = cb0 + 3 < 7;                     // wave-uniform: the upper waves' fourth block is padding
    for (int k0 = 0; k0 < len; k0 += GK) {
        const int cur = (k0 / GK) & 1;
        const bool more = k0 + GK < len;
        if (more) LOAD(k0 + GK);                       // in flight across the MFMAs below
#pragma unroll
        for (int kk = 0; kk < GK / 2; ++kk) {
            const int kq = 2 * kk + (lane >> 5), c = lane & 31;
            const float a = As[cur][kq][rb * 32 + c];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[cur][kq][(cb0 + 0) * 32 + c], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[cur][kq][(cb0 + 1) * 32 + c], acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[cur][kq][(cb0 + 2) * 32 + c], acc2, 0, 0, 0);
            if (has3) acc3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[cur][kq][(cb0 + 3) * 32 + c], acc3, 0, 0, 0);
        }
        if (more) STORE(cur ^ 1);
        __syncthreads();
    }
#undef LOAD
#undef STORE
    // epilogue: lane holds column 16 i + j of 16 channels; dW partial [z][e][ch][i][j]
    float* const out = part + ((int64_t)blockIdx.z * E + e0) * 588 + ch * 196;
    const int hi = lane >> 5;
#define PUT(ACC, CB)                                                                                                        \
    do {                                                                                                                    \
        const int col = (CB) * 32 + (lane & 31), i = col >> 4, j = col & 15;                                                \
        if (j < 14 && i < 14) {                                                                                             \
            _Pragma("unroll") for (int r = 0; r < 16; ++r)                                                                  \
                out[(int64_t)(rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi) * 588 + 14 * i + j] = (ACC)[r];                    \
        }                                                                                                                   \
    } while (0)
    PUT(acc0, cb0 + 0);
    PUT(acc1, cb0 + 1);
    PUT(acc2, cb0 + 2);
    if (has3) PUT(acc3, cb0 + 3);
#undef PUT
}

}  // namespace

// dx fp32 [n * tok, E] (patch rows from row `first` of every image), img fp32 [n, 3, H, W], part fp32 [ceil(n Np / rows_per_split)][E][3][14][14]
int launch_patch_embed_rgb_wgrad(const float* dx, int tok, int first, const float* img, int n, int H, int W, int E, int rows_per_split,
                                 float* part, hipStream_t s) {
    MST_CHECK_ARG(n > 0 && H > 0 && W > 0 && H % PATCH == 0 && W % PATCH == 0, "patch_embed_rgb_wgrad: n=%d H=%d W=%d (H, W multiples of 14)", n, H, W);
    MST_CHECK_ARG(E > 0 && E % GM == 0, "patch_embed_rgb_wgrad: E=%d must be a positive multiple of %d", E, GM);
    const int gw = W / PATCH, Np = (H / PATCH) * gw;
    MST_CHECK_ARG(first >= 0 && tok >= first + Np, "patch_embed_rgb_wgrad: %d tokens per image cannot hold %d patch rows from row %d", tok, Np, first);
    MST_CHECK_ARG(rows_per_split > 0 && rows_per_split % GK == 0, "patch_embed_rgb_wgrad: rows_per_split=%d must be a positive multiple of %d",
                  rows_per_split, GK);
    MST_CHECK_ARG(aligned(dx, 16) && aligned(img, 8) && aligned(part, 4), "patch_embed_rgb_wgrad: dx must be 16-byte, img 8-byte aligned");
    const int64_t rows = (int64_t)n * Np, splits = (rows + rows_per_split - 1) / rows_per_split;
    MST_CHECK_ARG(splits <= 65535, "patch_embed_rgb_wgrad: %lld splits of %d patch rows (at most 65535)", (long long)splits, rows_per_split);
    patch_rgb_wgrad_kernel<<<dim3(E / GM, 3, (unsigned)splits), dim3(256), 0, s>>>(dx, tok, first, img, rows, rows_per_split, Np, gw, H, W, E, part);
    return mst_check_launch("patch_embed_rgb_wgrad");
}

// img [n, 3, H, W] of idt; wp [E][3][14][16] of dt (columns 14, 15 of every kernel row zero); x fp32 [n * (n_prefix + Np), E]
int launch_patch_embed_rgb(const void* img, int idt, int n, int H, int W, const void* wp, int dt, const float* bias, const float* prefix,
                           int n_prefix, const float* pos_patch, int E, float* x, hipStream_t s) {
    MST_CHECK_ARG(H > 0 && W > 0 && H % PATCH == 0 && W % PATCH == 0, "patch_embed_rgb: H=%d W=%d must be multiples of 14", H, W);
    MST_CHECK_ARG(E > 0 && E % BNP == 0, "patch_embed_rgb: E=%d must be a multiple of %d", E, BNP);
    MST_CHECK_ARG(n > 0 && n_prefix >= 1 && (int64_t)n * (H / PATCH) * (W / PATCH) < (1ll << 31) - BMP, "patch_embed_rgb: n=%d n_prefix=%d", n,
                  n_prefix);
    MST_CHECK_ARG(aligned(wp, 16) && aligned(bias, 16) && aligned(pos_patch, 16) && aligned(x, 16) && aligned(img, 8),
                  "patch_embed_rgb: operands must be 16-byte aligned (the image: 8)");
    switch (dt) {
        case MST_F32: return launch_rgb_in<float>(img, idt, n, H, W, wp, bias, prefix, n_prefix, pos_patch, E, x, s);
        case MST_F16: return launch_rgb_in<f16_t>(img, idt, n, H, W, wp, bias, prefix, n_prefix, pos_patch, E, x, s);
        case MST_BF16: return launch_rgb_in<bf16_t>(img, idt, n, H, W, wp, bias, prefix, n_prefix, pos_patch, E, x, s);
    }
    mst_set_error("patch_embed_rgb: bad compute dtype %d", dt);
    return MST_EINVAL;
}

// out fp32 [rows, cols] = x (g == nullptr) or LayerNorm(x; g, b, eps); x_image: x is the fp32 image of the blocked layout, allocated
// for whole 32-row groups (cols % 8 == 0 then)
int launch_tap_rows(const float* x, int x_image, const float* g, const float* b, float* out, int64_t rows, int cols, float eps, hipStream_t s) {
    MST_CHECK_ARG(x && out && (g != nullptr) == (b != nullptr), "tap_rows: null pointer");
    MST_CHECK_ARG(cols > 0 && cols <= 2048 && cols % 2 == 0 && (!x_image || cols % 8 == 0), "tap_rows: cols=%d must be even (image: a multiple of 8) and <= 2048", cols);
    MST_CHECK_ARG(aligned(x, 8) && aligned(out, 8) && aligned(g, 8) && aligned(b, 8), "tap_rows: operands must be 8-byte aligned");
    if (rows <= 0) return MST_OK;
    MST_CHECK_ARG((rows + 3) / 4 < (1ll << 31), "tap_rows: rows=%lld", (long long)rows);
    return x_image ? launch_tap_t<true>(x, g, b, out, rows, cols, eps, s) : launch_tap_t<false>(x, g, b, out, rows, cols, eps, s);
}
