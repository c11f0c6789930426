// C[M,N] = epi(A[M,K] . W[N,K]^T + bias)  with 16-bit (bf16 / fp16) MFMA operands, fp32 accumulate.
//
// Both operands are K-contiguous (A row-major activations, W as nn.Linear stores it), so MFMA
// fragments are 16-byte row segments.  Workgroup = 256 threads = 4 waves (2x2), tile 128x128x64,
// each wave 64x64 = 4x4 v_mfma_f32_16x16x32.  Staging: global_load_lds_dwordx4 (LDS-DMA, no VGPR
// round trip) into a 2-deep ring; the LDS image is lane-linear, so the XOR swizzle that makes the
// ds_read_b128 fragment reads conflict-free is applied to the per-lane SOURCE address and again on
// the read (cdna guide rule 21).  W plays the MFMA "A" role so that each lane ends up with 4
// consecutive output columns of one row: epilogue accesses are 16 B (fp32) / 8 B (16-bit) per lane.
// 1-D grid with an XCD-aware remap: tiles that share an A panel run on one XCD's L2.
//
// Reference arithmetic: F.linear at attention.py:58,67; mlp.py:35-38; block.py:90-94.
#include <stdlib.h>

#include <type_traits>

#include "mst_common.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = BM * BK * 2;  // 16 KiB per operand per stage
// Stages of the LDS ring: a double buffer, the K-loop waits for the one stage in flight.  A 4-stage ring behind a COUNTED vmcnt (the newer
// stages stay in flight) for the one-workgroup-per-CU grids of TN = 64 was measured: 0.994 vs 0.992 ms per 16 x 224^2 forward -- no gain.
constexpr int NS = 2;

// TN: the N extent of the tile, 128 (default) or 64.  64 halves a workgroup's work and doubles the grid (wave tile 64 x 32): gemm16_route.
template <typename T, int EPI, typename OutT, int TN = 128>
__global__ __launch_bounds__(256) void gemm16_kernel(const T* __restrict__ A, int64_t lda,
                                                     const T* __restrict__ W, int64_t ldw,
                                                     const float* __restrict__ bias, OutT* C,
                                                     int64_t ldc, int M, int N, int K,
                                                     const float* __restrict__ gamma, float col_scale,
                                                     int scale_cols, int tiles_n, int nwg, int64_t split_stride) {
    typedef typename V8<T>::type vec8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // split-K (launch_gemm16_splitk): blockIdx.y owns the K columns [y K, (y + 1) K) of both operands and its own fp32 partial C
    A += (int64_t)blockIdx.y * K;
    W += (int64_t)blockIdx.y * K;
    C += (int64_t)blockIdx.y * split_stride;
    constexpr int NI = TN / 32;              // 16-column accumulator blocks per wave (wave tile 64 x TN/2) = W pieces per wave and stage
    constexpr int W_BYTES = TN * BK * 2;
    char* const As = smem;                    // [NS][128][64] T
    char* const Ws = smem + NS * TILE_BYTES;  // [NS][TN][64] T

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = xcd_remap(blockIdx.x, nwg);
    const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * TN;
    const int wm = wave >> 1, wn = wave & 1;

    // ---- LDS-DMA source addresses: instruction i of this wave fills tile rows rb*8 .. rb*8+7
    const T* asrc[4];
    const T* wsrc[NI];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (wave * 4 + i) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);  // chunk whose swizzled home is LDS slot lane&7
        int am = m0 + r;
        am = am < M ? am : M - 1;
        asrc[i] = A + (int64_t)am * lda + c * 8;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int r = (wave * NI + i) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        wsrc[i] = W + (int64_t)(n0 + r) * ldw + c * 8;
    }
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_global_load_lds(GLB_PTR(asrc[i]), LDS_PTR(As + buf * TILE_BYTES + (wave * 4 + i) * 1024), 16, 0, 0);
            asrc[i] += BK;
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            __builtin_amdgcn_global_load_lds(GLB_PTR(wsrc[i]), LDS_PTR(Ws + buf * W_BYTES + (wave * NI + i) * 1024), 16, 0, 0);
            wsrc[i] += BK;
        }
    };

    // accumulators start at the bias (no bias load / vmcnt drain left in the epilogue)
    f32x4 acc[NI][4];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        f32x4 b0 = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (bias) b0 = *reinterpret_cast<const f32x4*>(bias + n0 + wn * (TN / 2) + i * 16 + (lane >> 4) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = b0;
    }

    const int sw = (lane >> 1) & 7;  // ((row >> 1) & 7) for row = 16*k + (lane & 15)
    const int a_row_off = (wm * 64 + (lane & 15)) * 128;
    const int w_row_off = (wn * (TN / 2) + (lane & 15)) * 128;

    const int nk = K / BK;
#pragma unroll
    for (int p = 0; p < NS - 1; ++p)
        if (p < nk) stage(p);
    for (int t = 0; t < nk; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // stage t has landed (the only one in flight)
        __syncthreads();  // stage t is visible to every wave; every wave is done reading the buffer the next stage overwrites
        if (t + NS - 1 < nk) stage((t + NS - 1) % NS);
        const char* Ab = As + (t % NS) * TILE_BYTES;
        const char* Wb = Ws + (t % NS) * W_BYTES;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int coff = ((kk * 4 + (lane >> 4)) ^ sw) * 16;
            vec8 af[4], wf[NI];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                af[j] = *reinterpret_cast<const vec8*>(Ab + a_row_off + j * 16 * 128 + coff);
#pragma unroll
            for (int i = 0; i < NI; ++i)
                wf[i] = *reinterpret_cast<const vec8*>(Wb + w_row_off + i * 16 * 128 + coff);
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(wf[i], af[j], acc[i][j]);
        }
    }

    // ---- epilogue: lane owns C[m][n..n+3], m = m0+wm*64+j*16+(lane&15), n = n0+wn*64+i*16+(lane>>4)*4.
    // Interior tiles run branch-free (per-lane `m < M` branches make hipcc drain vmcnt(0) before every store).
    auto epilogue = [&](auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        if constexpr (EPI == MST_EPI_BIAS_SWIGLU) {
            // W is the row-paired w12 image (include/mst_hip.h): image rows n0 + wn TN/2 + 32 p + [0, 16) are gates, + [16, 32) their values, so
            // acc[2p][j] and acc[2p + 1][j] of this lane are gate and value of output columns (n0 + wn TN/2) / 2 + 16 p + 4 (lane >> 4) + [0, 4)
#pragma unroll
            for (int p = 0; p < NI / 2; ++p) {
                const int n = (n0 + wn * (TN / 2)) / 2 + p * 16 + (lane >> 4) * 4;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int m = m0 + wm * 64 + j * 16 + (lane & 15);
                    if (!FULL && m >= M) continue;
                    float v[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = swiglu_gate<sizeof(OutT) == 2>(acc[2 * p][j][r], acc[2 * p + 1][j][r]);
                    OutT* cp = C + (int64_t)m * ldc + n;
                    if constexpr (sizeof(OutT) == 4) {
                        *reinterpret_cast<float4*>(cp) = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
                        typedef __attribute__((ext_vector_type(4))) OutT o4;
                        o4 pk;
                        pk[0] = (OutT)v[0];
                        pk[1] = (OutT)v[1];
                        pk[2] = (OutT)v[2];
                        pk[3] = (OutT)v[3];
                        *reinterpret_cast<o4*>(cp) = pk;
                    }
                }
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int n = n0 + wn * (TN / 2) + i * 16 + (lane >> 4) * 4;
            float4 gv = make_float4(1.f, 1.f, 1.f, 1.f);
            if (EPI == MST_EPI_RESIDUAL && gamma) gv = *reinterpret_cast<const float4*>(gamma + n);
            float sc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) sc[r] = (n + r < scale_cols) ? col_scale : 1.0f;
            float4 xv[4];
            if constexpr (EPI == MST_EPI_RESIDUAL) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int m = m0 + wm * 64 + j * 16 + (lane & 15);
                    if (FULL || m < M) xv[j] = *reinterpret_cast<const float4*>(C + (int64_t)m * ldc + n);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int m = m0 + wm * 64 + j * 16 + (lane & 15);
                if (!FULL && m >= M) continue;
                float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v[r] *= sc[r];
                    if (EPI == MST_EPI_BIAS_GELU) v[r] = (sizeof(OutT) == 2) ? gelu_fast(v[r]) : gelu_erf(v[r]);
                    if (EPI == MST_EPI_BIAS_RELU) v[r] = fmaxf(v[r], 0.f);
                }
                OutT* cp = C + (int64_t)m * ldc + n;
                if constexpr (EPI == MST_EPI_RESIDUAL) {
                    float4 o;
                    o.x = xv[j].x + gv.x * v[0];
                    o.y = xv[j].y + gv.y * v[1];
                    o.z = xv[j].z + gv.z * v[2];
                    o.w = xv[j].w + gv.w * v[3];
                    *reinterpret_cast<float4*>(cp) = o;
                } else if constexpr (sizeof(OutT) == 4) {
                    *reinterpret_cast<float4*>(cp) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
                    typedef __attribute__((ext_vector_type(4))) OutT o4;
                    o4 pk;
                    pk[0] = (OutT)v[0];
                    pk[1] = (OutT)v[1];
                    pk[2] = (OutT)v[2];
                    pk[3] = (OutT)v[3];
                    *reinterpret_cast<o4*>(cp) = pk;
                }
            }
        }
    };
    if (m0 + BM <= M) epilogue(std::true_type{});
    else epilogue(std::false_type{});
}

// The 128 x 128 kernel (narrow: its 128 x 64 form) for every epilogue and both output types; the residual one is fp32 read-modify-write.
struct tile_launcher {
    bool narrow;
    template <typename T, int EPI, typename OutT> static constexpr bool has() {
        constexpr bool t16 = std::is_same<T, bf16_t>::value || std::is_same<T, f16_t>::value, f32out = std::is_same<OutT, float>::value;
        return t16 && (EPI == MST_EPI_RESIDUAL ? f32out : EPI <= MST_EPI_BIAS_RELU && (f32out || std::is_same<OutT, T>::value));
    }
    template <typename T, int EPI, typename OutT> int launch(const gemm_args& g) const {
        const int tiles_m = (int)((g.M + BM - 1) / BM);
        if (narrow) {
            const int tiles_n = g.N / 64, nwg = tiles_m * tiles_n;
            static mst_lds_once lds_once_n;
            auto kern = gemm16_kernel<T, EPI, OutT, 64>;
            constexpr int lds = 2 * TILE_BYTES + 2 * 64 * BK * 2;
            mst_allow_lds((const void*)kern, lds, &lds_once_n);
            kern<<<dim3(nwg), dim3(256), lds, g.s>>>((const T*)g.A, g.lda, (const T*)g.W, g.ldw, g.bias, (OutT*)g.C, g.ldc, (int)g.M, g.N, g.K,
                                                      g.gamma, g.col_scale, g.scale_cols, tiles_n, nwg, 0);
            return mst_check_launch("gemm16 (128 x 64)");
        }
        static mst_lds_once lds_once;
        auto kern = gemm16_kernel<T, EPI, OutT>;
        mst_allow_lds((const void*)kern, 4 * TILE_BYTES, &lds_once);
        const int tiles_n = g.N / BN, nwg = tiles_m * tiles_n;
        kern<<<dim3(nwg), dim3(256), 4 * TILE_BYTES, g.s>>>((const T*)g.A, g.lda, (const T*)g.W, g.ldw, g.bias, (OutT*)g.C, g.ldc, (int)g.M, g.N,
                                                             g.K, g.gamma, g.col_scale, g.scale_cols, tiles_n, nwg, 0);
        return mst_check_launch("gemm16");
    }
};

template <typename T>
int launch_split(const gemm_args& g, int splits, int64_t split_stride) {
    static mst_lds_once lds_once;
    auto kern = gemm16_kernel<T, MST_EPI_BIAS, float>;
    mst_allow_lds((const void*)kern, 4 * TILE_BYTES, &lds_once);
    const int tiles_m = (int)((g.M + BM - 1) / BM), tiles_n = g.N / BN;
    const int nwg = tiles_m * tiles_n;
    kern<<<dim3(nwg, splits), dim3(256), 4 * TILE_BYTES, g.s>>>((const T*)g.A, g.lda, (const T*)g.W, g.ldw, nullptr, (float*)g.C, g.ldc, (int)g.M,
                                                                 g.N, g.K / splits, nullptr, 1.f, 0, tiles_n, nwg, split_stride);
    return mst_check_launch("gemm16_splitk");
}

// MST_EPI_BIAS_SWIGLU: W / bias are the row-paired image with g.N rows, C is [M, N / 2].  Always the tiled kernel, in gemm16_route's two
// widths (the wreg, mid and big kernels have no such epilogue); the runtime dispatcher of mst_common.h does not know the value, so no
// other launcher is asked for it.
template <typename T>
int launch_swiglu(const gemm_args& g) {
    const tile_launcher tl{(int64_t)((g.M + BM - 1) / BM) * (g.N / BN) < 224};
    if (g.cdt == MST_F32) return tl.template launch<T, MST_EPI_BIAS_SWIGLU, float>(g);
    return tl.template launch<T, MST_EPI_BIAS_SWIGLU, T>(g);
}

// Which kernel a 16-bit GEMM runs.  Every threshold is here, beside the measurement behind it (MI355X, tools/bench_gemm.py unless named).
enum gemm16_kernel_id { GEMM16_WREG, GEMM16_MID, GEMM16_BIG, GEMM16_TILE128, GEMM16_TILE64 };

int64_t tiles_of(const gemm_tile& t, const gemm_args& g) { return ((g.M + t.bm - 1) / t.bm) * (int64_t)(g.N / t.bn); }
bool divides(const gemm_tile& t, const gemm_args& g) { return g.N % t.bn == 0 && g.K % t.bk == 0; }

gemm16_kernel_id gemm16_route(const gemm_args& g) {
    // weights in registers (k_gemm16_wreg.hip).  It moves 16-byte pieces on every operand (LDS-DMA of A, vector loads of W, vector stores
    // of C): a caller of the C ABI with an odd row pitch or a sliced pointer falls back to the tiled kernels.
    const bool al16 = g.lda % 8 == 0 && g.ldw % 8 == 0 && g.ldc % 8 == 0 && ((uintptr_t)g.A & 15) == 0 && ((uintptr_t)g.W & 15) == 0 &&
                      ((uintptr_t)g.C & 15) == 0;
    if (al16 && gemm16_wreg_applicable(g)) return GEMM16_WREG;
    // 128 x 384, one 4-wave workgroup per CU (k_gemm16_mid.hip): 16-bit output of the operand type, shallow K (the epilogue weighs as much
    // as the K-loop), enough tiles to fill the chip twice.  0.58 ms on the QKV shape against 0.65 ms for both kernels below.  Its residual
    // (fp32 read-modify-write) form measured the same as the 128 x 128 kernel on the HBM-bound proj GEMM (0.33 ms) and was removed.
    if (g.dt == g.cdt && (g.epi == MST_EPI_BIAS || g.epi == MST_EPI_BIAS_RELU) && divides(GEMM16_MID_TILE, g) && g.K <= 512 &&
        tiles_of(GEMM16_MID_TILE, g) >= 512)
        return GEMM16_MID;
    // persistent 256 x 384 (k_gemm16_big.hip) once its tiles fill the chip: 153 FLOP per staged byte against 64.  Never the residual
    // epilogue: its read-modify-write is HBM-bound and overlaps better with two small workgroups per CU; the big kernel's form was removed.
    // (bias, GELU, ReLU only: the SwiGLU epilogue never reaches this router, launch_gemm16 sends it to the tiled kernel.)
    if (g.epi <= MST_EPI_BIAS_RELU && divides(GEMM16_BIG_TILE, g) && tiles_of(GEMM16_BIG_TILE, g) >= 192) return GEMM16_BIG;
    // 128 x 128; below 224 workgroups that grid would leave CUs idle (a few thousand token rows against N = 384: 99 workgroups on 256
    // CUs), so 128 x 64 tiles, twice the workgroups
    return (int64_t)((g.M + BM - 1) / BM) * (g.N / BN) < 224 ? GEMM16_TILE64 : GEMM16_TILE128;
}

}  // namespace

// K = 384 exactly (the register-resident weight slice), 384-column tiles with at most one per CU of an XCD, plain bias epilogue into the
// operand type, the scaled column range aligned to the tiles, at least 8,192 rows (profiles/r02v_qkv_wreg.txt, r03v)
bool gemm16_wreg_applicable(const gemm_args& g) {
    constexpr gemm_tile t = GEMM16_WREG_TILE;
    const int G = mst_persistent_grid() >> 3;
    const char* e = getenv("MST_GEMM_WREG_MIN_M");    // tests lower the threshold to reach the few-chunks-per-CU paths
    const int64_t min_m = e ? atoll(e) : 8192;        // measured crossover against the tiled kernels: faster from ~10 k rows (0.047 vs 0.080 ms at 43,840)
    return g.K == t.bk && g.N % t.bn == 0 && g.N / t.bn <= G && g.dt == g.cdt && g.epi == MST_EPI_BIAS &&
           (g.scale_cols % t.bn == 0 || g.scale_cols >= g.N) && g.M >= min_m && g.M < (1ll << 31) - t.bm && g.lda * 2 * t.bm < (1ll << 31) &&
           g.ldc * 2 * t.bm < (1ll << 31) && g.ldc % 4 == 0;
}

// Cpart[z] = A[:, z Kc : (z + 1) Kc] . W[:, z Kc : (z + 1) Kc]^T for z < splits (fp32 partial products, split_stride elements apart; the caller
// sums them: mst_colsum over a [splits, M * N] view).  The shape of d weight = dY^T . X: a small [N_out, N_in] output reduced over
// thousands of token rows, which one workgroup per output tile would walk on a handful of CUs.
int launch_gemm16_splitk(const gemm_args& g, int splits, int64_t split_stride) {
    MST_CHECK_ARG(g.A && g.W && g.C && g.M > 0 && splits > 0 && splits <= 65535, "gemm16_splitk: bad arguments");
    MST_CHECK_ARG(g.K % splits == 0 && (g.K / splits) % BK == 0, "gemm16_splitk: K=%d must split into %d multiples of %d", g.K, splits, BK);
    MST_CHECK_ARG(g.N > 0 && g.N % BN == 0, "gemm16_splitk: N=%d must be a multiple of %d", g.N, BN);
    MST_CHECK_ARG(g.lda % 8 == 0 && g.ldw % 8 == 0 && g.ldc % 4 == 0 && ((uintptr_t)g.A & 15) == 0 && ((uintptr_t)g.W & 15) == 0 && ((uintptr_t)g.C & 15) == 0,
                  "gemm16_splitk: lda/ldw must be multiples of 8, ldc of 4, bases 16-byte aligned");
    MST_CHECK_ARG(split_stride >= g.M * g.ldc && split_stride % 4 == 0, "gemm16_splitk: split_stride");
    if (g.dt == MST_BF16) return launch_split<bf16_t>(g, splits, split_stride);
    if (g.dt == MST_F16) return launch_split<f16_t>(g, splits, split_stride);
    mst_set_error("gemm16_splitk: bad operand dtype %d", g.dt);
    return MST_EINVAL;
}

int launch_gemm16(const gemm_args& g) {
    MST_CHECK_ARG(g.K > 0 && g.K % BK == 0, "gemm16: K=%d must be a multiple of %d", g.K, BK);
    MST_CHECK_ARG(g.N > 0 && g.N % BN == 0, g.epi == MST_EPI_BIAS_SWIGLU ? "gemm16: N=%d rows of the paired image must be a multiple of %d (16-bit pairing group 16)"
                                                                          : "gemm16: N=%d must be a multiple of %d", g.N, BN);
    MST_CHECK_ARG(g.lda % 8 == 0 && g.ldw % 8 == 0 && g.ldc % 4 == 0, "gemm16: lda/ldw must be multiples of 8, ldc of 4");
    MST_CHECK_ARG(g.M < (1ll << 31) - BM, "gemm16: M too large");
    MST_CHECK_ARG(g.cdt == MST_F32 || g.cdt == g.dt, "gemm16: C dtype must be f32 or the operand dtype");
    MST_CHECK_ARG(g.epi != MST_EPI_RESIDUAL || g.cdt == MST_F32, "gemm16: residual epilogue needs f32 C");
    MST_CHECK_ARG(g.epi != MST_EPI_RESIDUAL_RELU, "gemm16: the residual + ReLU epilogue exists for f32 operands only");
    if (g.epi == MST_EPI_BIAS_SWIGLU) {   // (N % 128 above: whole pairs of 16-row pairing groups for both tile widths)
        MST_CHECK_ARG(g.scale_cols == 0 && !g.gamma, "gemm16: no column scaling and no LayerScale on the SwiGLU epilogue");
        MST_CHECK_ARG(g.ldc >= g.N / 2, "gemm16: ldc=%lld is less than the %d output columns of the SwiGLU epilogue", (long long)g.ldc, g.N / 2);
        MST_CHECK_ARG(g.dt == MST_BF16 || g.dt == MST_F16, "gemm16: bad operand dtype %d", g.dt);
        if (g.M <= 0) return MST_OK;
        return g.dt == MST_BF16 ? launch_swiglu<bf16_t>(g) : launch_swiglu<f16_t>(g);
    }
    if (g.M <= 0) return MST_OK;
    switch (gemm16_route(g)) {
        case GEMM16_WREG: return launch_gemm16_wreg(g);
        case GEMM16_MID: return launch_gemm16_mid(g);
        case GEMM16_BIG: return launch_gemm16_big(g);
        case GEMM16_TILE128: return gemm_dispatch("gemm16", g, tile_launcher{false});
        case GEMM16_TILE64: return gemm_dispatch("gemm16", g, tile_launcher{true});
    }
    return MST_EINVAL;   // not reached: every route returns above
}
