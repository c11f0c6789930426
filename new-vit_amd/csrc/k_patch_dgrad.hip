// mst_patch_embed_dgrad: the data gradient of the DINOv2 patch embedding, i.e. the gradient of the training step with respect to
// the input volume.  The reference repeats every grey slice into three identical RGB channels (dino.py:121-127) and runs
// Conv2d(3, E, 14, stride 14) (patch_embed.py:68-81); torch.autograd carries d x through both.  Patches do not overlap, so the
// adjoint of the stride-14 convolution writes every pixel exactly once, and the adjoint of the repeat sums the three channel kernels
// -- the same [E, 14 x 16] fp32 `wsum` the forward already builds for mst_patch_embed:
//   dvol[s, 14 py + i, 14 px + j] = sum_e dx[s, first + py gw + px, e] * wsum[e, 16 i + j]       (i, j < 14)
// a GEMM [n Np, E] x [E, 224] on the exact fp32 MFMA (v_mfma_f32_32x32x2_f32) whose epilogue writes pixels.
// 64 patch rows x 256 columns (224 real: 14 kernel rows x 16, columns 14, 15 zero) per 256-thread workgroup: four waves, wave w owns
// the 32-row block w & 1 and four 32-column blocks from 4 (w >> 1) (the eighth block is all padding and skipped).  K-step 16, LDS
// double-buffered, the next step's operands in registers across the current step's MFMAs (one barrier per step, as gemm_ex).  Epilogue:
// the 64 x 196 tile goes through LDS (aliasing the operand buffers) and leaves as 14-float patch rows, consecutive threads on
// consecutive pixels of one image row.  No atomics: the result does not depend on scheduling.
//
// mst_patch_embed_rgb_dgrad is the same kernel over three DISTINCT channels (the encoder API's [n, 3, H, W] input, patch_embed.py:65,75-81):
// blockIdx.y is the channel, whose 224 columns of the [E][3][14][16] kernel image (ldw = 672) play wsum and whose plane of dimg is written:
//   dimg[s, c, 14 py + i, 14 px + j] = sum_e dx[s, first + py gw + px, e] * w[e, c, i, j]
// The grey call is C = 1, ldw = 224: the same instructions on the same operands as before.
#include "mst_common.h"

namespace {

constexpr int TM = 64;                 // patch rows per workgroup
constexpr int TK = 16;                 // channels per K-step
constexpr int LDA = TM + 4;            // As[k][row]: k and k+1 four banks apart (as gemm_ex)
constexpr int KP = 224;                // wsum row: 14 kernel rows x 16
constexpr int LDB = 256 + 4;           // Bs[k][col], 256 staged columns (224..255 zero)
constexpr int LDO = 200;               // Os[row][14 i + j]: rows r and r + 4 (the two half-waves of an MFMA result) 32 banks apart
constexpr int SMEM = (2 * TK * LDA + 2 * TK * LDB) > TM * LDO ? (2 * TK * LDA + 2 * TK * LDB) : TM * LDO;

__device__ __forceinline__ float4 wtile(const float* __restrict__ wsum, int ldw, int k0, int idx) {
    const int k = idx >> 6, c = (idx & 63) * 4;
    return c < KP ? *reinterpret_cast<const float4*>(wsum + (int64_t)(k0 + k) * ldw + c) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(256) void patch_dgrad_kernel(const float* __restrict__ dx, int tok, int first, const float* __restrict__ wsum,
                                                          int ldw, int C,
                                                          int64_t rows, int Np, int gw, int H, int W, int E, float* __restrict__ dvol) {
    __shared__ __attribute__((aligned(16))) float smem[SMEM];
    __shared__ int64_t rbase[TM];
    float (*As)[TK][LDA] = reinterpret_cast<float (*)[TK][LDA]>(smem);
    float (*Bs)[TK][LDB] = reinterpret_cast<float (*)[TK][LDB]>(smem + 2 * TK * LDA);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rb = wave & 1, cb0 = (wave >> 1) * 4;
    const int64_t m0 = (int64_t)blockIdx.x * TM;
    const int ch = blockIdx.y;                         // channel plane of the output; its 224 columns of the kernel image
    wsum += ch * KP;
    // A operand (the patch-row gradients): thread -> (row tid / 4, four channels 4 (tid % 4)) of the K-step, one float4
    const int ar = tid >> 2, ak = (tid & 3) * 4;
    const bool a_ok = m0 + ar < rows;
    const float* arow = dx;
    if (a_ok) {
        const int64_t m = m0 + ar, s = m / Np;
        arow = dx + (s * tok + first + (m - s * Np)) * (int64_t)E;
    }
    // pixel offset of every patch row of the tile (-1 past the end)
    if (tid < TM) {
        const int64_t m = m0 + tid;
        int64_t b = -1;
        if (m < rows) {
            const int64_t s = m / Np;
            const int p = (int)(m - s * Np), py = p / gw, px = p - py * gw;
            b = ((s * C + ch) * H + 14 * py) * (int64_t)W + 14 * px;
        }
        rbase[tid] = b;
    }
    // B operand (wsum): 16 x 256 columns, thread -> four float4 (k = idx / 64, column 4 (idx % 64)), idx = tid + 256 q
    float4 ra, rw0, rw1, rw2, rw3;
#define LOAD(K0)                                                                                                            \
    do {                                                                                                                    \
        ra = a_ok ? *reinterpret_cast<const float4*>(arow + (K0) + ak) : make_float4(0.f, 0.f, 0.f, 0.f);                  \
        rw0 = wtile(wsum, ldw, (K0), tid); rw1 = wtile(wsum, ldw, (K0), tid + 256);                                                   \
        rw2 = wtile(wsum, ldw, (K0), tid + 512); rw3 = wtile(wsum, ldw, (K0), tid + 768);                                             \
    } while (0)
#define STORE(BUF)                                                                                                          \
    do {                                                                                                                    \
        As[BUF][ak + 0][ar] = ra.x; As[BUF][ak + 1][ar] = ra.y; As[BUF][ak + 2][ar] = ra.z; As[BUF][ak + 3][ar] = ra.w;     \
        *reinterpret_cast<float4*>(&Bs[BUF][tid >> 6][(tid & 63) * 4]) = rw0;                                               \
        *reinterpret_cast<float4*>(&Bs[BUF][(tid + 256) >> 6][(tid & 63) * 4]) = rw1;                                       \
        *reinterpret_cast<float4*>(&Bs[BUF][(tid + 512) >> 6][(tid & 63) * 4]) = rw2;                                       \
        *reinterpret_cast<float4*>(&Bs[BUF][(tid + 768) >> 6][(tid & 63) * 4]) = rw3;                                       \
    } while (0)
    f32x16 acc0, acc1, acc2, acc3;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = acc2[r] = acc3[r] = 0.f;
    LOAD(0);
    STORE(0);
    __syncthreads();
    const bool has3 = cb0 + 3 < 7;                     // wave-uniform: the upper waves' fourth block is padding
    for (int k0 = 0; k0 < E; k0 += TK) {
        const int cur = (k0 / TK) & 1;
        const bool more = k0 + TK < E;
        if (more) LOAD(k0 + TK);                       // in flight across the MFMAs below
#pragma unroll
        for (int kk = 0; kk < TK / 2; ++kk) {
            const int k = 2 * kk + (lane >> 5), c = lane & 31;
            const float a = As[cur][k][rb * 32 + c];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[cur][k][(cb0 + 0) * 32 + c], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[cur][k][(cb0 + 1) * 32 + c], acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[cur][k][(cb0 + 2) * 32 + c], acc2, 0, 0, 0);
            if (has3) acc3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[cur][k][(cb0 + 3) * 32 + c], acc3, 0, 0, 0);
        }
        if (more) STORE(cur ^ 1);
        __syncthreads();
    }
#undef LOAD
#undef STORE
    // epilogue: accumulators -> Os[row][14 i + j] (the loop's last barrier retired every operand read) -> pixels
    float* Os = smem;
    const int hi = lane >> 5;
#define PUT(ACC, CB)                                                                                                        \
    do {                                                                                                                    \
        const int col = (CB) * 32 + (lane & 31), i = col >> 4, j = col & 15;                                                \
        if (j < 14) {                                                                                                       \
            _Pragma("unroll") for (int r = 0; r < 16; ++r)                                                                  \
                Os[(rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi) * LDO + 14 * i + j] = (ACC)[r];                             \
        }                                                                                                                   \
    } while (0)
    PUT(acc0, cb0 + 0);
    PUT(acc1, cb0 + 1);
    PUT(acc2, cb0 + 2);
    if (has3) PUT(acc3, cb0 + 3);
#undef PUT
    __syncthreads();
    // (i, tile row, j) with j fastest: a wave writes runs of neighbouring patches' 14-pixel spans along one image row
    for (int idx = tid; idx < 14 * TM * 14; idx += 256) {
        const int j = idx % 14, rr = (idx / 14) % TM, i = idx / (14 * TM);
        const int64_t b = rbase[rr];
        if (b >= 0) dvol[b + (int64_t)i * W + j] = Os[rr * LDO + 14 * i + j];
    }
}

}  // namespace

// C = 1: wsum [E][224], dvol [n, H, W];  C = 3: wsum = the kernel image [E][3][224], dvol [n, 3, H, W]
int launch_patch_embed_dgrad(const float* dx, int tok, int first, const float* wsum, int C, int n, int H, int W, int E, float* dvol,
                             hipStream_t s) {
    MST_CHECK_ARG(C == 1 || C == 3, "patch_embed_dgrad: %d channels (1 or 3)", C);
    MST_CHECK_ARG(n > 0 && H > 0 && W > 0 && H % 14 == 0 && W % 14 == 0, "patch_embed_dgrad: n=%d H=%d W=%d (H, W multiples of 14)", n, H, W);
    MST_CHECK_ARG(E > 0 && E % TK == 0, "patch_embed_dgrad: E=%d must be a positive multiple of %d", E, TK);
    const int gw = W / 14, Np = (H / 14) * gw;
    MST_CHECK_ARG(first >= 0 && tok >= first + Np, "patch_embed_dgrad: %d tokens per image cannot hold %d patch rows from row %d", tok, Np, first);
    MST_CHECK_ARG(((reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(wsum)) & 15) == 0,
                  "patch_embed_dgrad: dx and wsum must be 16-byte aligned");
    const int64_t rows = (int64_t)n * Np, blocks = (rows + TM - 1) / TM;
    MST_CHECK_ARG(blocks < (1ll << 31), "patch_embed_dgrad: %lld patch rows out of range", (long long)rows);
    patch_dgrad_kernel<<<dim3((unsigned)blocks, C), dim3(256), 0, s>>>(dx, tok, first, wsum, C * KP, C, rows, Np, gw, H, W, E, dvol);
    return mst_check_launch("patch_embed_dgrad");
}
