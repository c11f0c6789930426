// Memory-efficient attention for the mixed-precision TRAINING step of the per-slice ViT blocks (attention.py:56-66, the reference's
// MemEffAttention): head_dim 64, non-causal, no key mask, any N >= 1 with tail masking, 16-bit MFMA operands, fp32 softmax and
// accumulation.  No [N, N] tensor exists in the forward or the backward: the backward recomputes the probabilities per tile from the
// forward's per-row log-sum-exp (FlashAttention-2).
//
//   forward       O = softmax(q k^T) v, LSE = ln sum_j exp(q k_j)      exact running row maximum (the classic path of k_attn16.hip, no fixed
//                                                                    reference point), O normalised by the sum that LSE encodes
//   preprocess    D = rowsum(dO o O) per (row, head); the 16-bit image of dO that the MFMAs read, both times c, a power of two per
//                 (sequence, head) with c max|dO| in [32, 64): in the training step |dO| is ~1e-6 and dS = P o (dP - D) smaller still,
//                 below fp16's normal range (6.1e-5) -- unscaled, the 16-bit dS MFMA operand lost its low bits or flushed to zero.
//                 dS then carries c as well, and the passes multiply dQ, dK, dV by 1/c (exact, like c).
//   key pass      per 32-key wave block: dV = sum_q P^T dO, dK = sum_q dS^T q          (S, dP recomputed per 32-query sub-tile)
//   query pass    per 32-query wave block: dQ = dq_scale * sum_k dS K                  (S, dP recomputed per 32-key sub-tile)
//
// with P = exp(S - LSE), dS = P o (dP - D), dP = dO V^T.  dQ has its own pass instead of float atomics across key blocks: two identical
// calls return identical bits.  q arrives pre-scaled by head_dim^-0.5 (the QKV projection's epilogue); dK is the gradient of the stored k,
// dQ that of the stored q times dq_scale (the gradient of the un-scaled projection output when dq_scale is the epilogue's factor).
//
// Granularity: a wave owns 32 rows (queries in the forward / query pass, keys in the key pass), a workgroup 4 waves; the other operand
// streams through LDS in tiles of 64 rows, processed as two 32-row halves of which the second is skipped when it holds no valid row.
// At N = 257 (224^2) the padded work is 288 rows per direction (12 %) instead of 320 with 64-row blocks; at N = 1370 it is 1376 / 1408.
// Waves whose 32 rows all lie past N skip their MFMAs (wave-uniform) and only help stage tiles.
//
// MFMA layouts (v_mfma_f32_32x32x16, mst_common.h): an accumulator holds row (r&3)+8(r>>2)+4h of its 32 x 32 tile in register r and
// column lane&31 (h = lane>>5).  Its registers 8ks .. 8ks+7, rounded to 16 bits, ARE the operand of a following product over the
// accumulator's ROW index, in the k order 16ks + 8(j>>2) + 4h + (j&3); the matching other operand is read with ds_read_b64_tr_b16
// (cdna_hip_programming.md T10) from the same row-major LDS image that the row reads (ds_read_b128) use.
#include "mst_common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int ROWB = 128;               // one row of a tile: 64 x 16-bit
constexpr int TILE = 64 * ROWB;         // 64 rows
constexpr int WGT = 256;                // 4 waves

// LDS image of a [64][64] 16-bit tile: 128-byte rows, 16-byte chunk ch of row r at slot ch ^ swz(r).  Row reads (16 lanes, 16
// consecutive rows, one chunk) hit 16 distinct 16-byte slots of the 256-byte bank row; a transposed read's 32-lane half (rows
// r0 .. r0+3, r0 % 4 == 0, four chunks) also covers the bank row once: rows of equal parity differ in bit 2 of swz.
__device__ __forceinline__ int swz(int r) { return (((r >> 1) & 1) << 2) | ((r >> 2) & 3); }
__device__ __forceinline__ int toff(int r, int ch) { return r * ROWB + ((ch ^ swz(r)) << 4); }

template <typename T>
__device__ __forceinline__ typename V8<T>::type row_frag(const char* tile, int r, int ch) {
    return *reinterpret_cast<const typename V8<T>::type*>(tile + toff(r, ch));
}

// Operand whose lane index is tile column 32 db + (lane & 31) and whose k index runs over tile rows r0 + 16 ks' .. in the accumulator
// order above: element j of lane (h, c) = tile[r0 + 8(j>>2) + 4h + (j&3)][32 db + c].  Lane 4q+p of a 16-lane group addresses row q,
// columns 4p .. 4p+3 of the group's 4 x 16 block; EXEC must be full (callers branch on wave-uniform conditions only).
template <typename T>
__device__ __forceinline__ typename V8<T>::type tr_frag(const char* tile, int r0, int db, int lane) {
    typedef typename V8<T>::type vec8;
    const int i = lane & 15, h = lane >> 5;
    const int r = r0 + 4 * h + (i >> 2);
    const int ch = db * 4 + ((lane >> 4) & 1) * 2 + ((i & 3) >> 1);
    const int b = (i & 1) * 8;
    union { struct { s16x4 lo, hi; } s; vec8 v; } u;
    u.s.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(tile + toff(r, ch) + b));
    u.s.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(tile + toff(r + 8, ch) + b));
    return u.v;
}

__device__ __forceinline__ float half_max(float v) {    // the other half of a column's rows sits 32 lanes away
    const unsigned u = __float_as_uint(v);
    const auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
}
__device__ __forceinline__ float half_sum(float v) {
    const unsigned u = __float_as_uint(v);
    const auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
}

// Register-staged double buffer of two [64][64] 16-bit operands: thread -> row tid >> 2, chunks 2 (tid & 3) and +1 of each.  Rows past
// N re-read row N-1 (their results are masked or not written).
template <typename T>
struct Stage2 {
    u32x4 r[4];
    int sr, sc;
    __device__ __forceinline__ void init(int tid) { sr = tid >> 2; sc = (tid & 3) * 2; }
    __device__ __forceinline__ void load(const T* a, int64_t lda, const T* b, int64_t ldb, int row0, int N) {
        int row = row0 + sr;
        row = row < N ? row : N - 1;
        const T* pa = a + (int64_t)row * lda + sc * 8;
        const T* pb = b + (int64_t)row * ldb + sc * 8;
        r[0] = *reinterpret_cast<const u32x4*>(pa);
        r[1] = *reinterpret_cast<const u32x4*>(pa + 8);
        r[2] = *reinterpret_cast<const u32x4*>(pb);
        r[3] = *reinterpret_cast<const u32x4*>(pb + 8);
    }
    __device__ __forceinline__ void store(char* ta, char* tb) const {
        *reinterpret_cast<u32x4*>(ta + toff(sr, sc)) = r[0];
        *reinterpret_cast<u32x4*>(ta + toff(sr, sc + 1)) = r[1];
        *reinterpret_cast<u32x4*>(tb + toff(sr, sc)) = r[2];
        *reinterpret_cast<u32x4*>(tb + toff(sr, sc + 1)) = r[3];
    }
};

// ---- forward: O [n*N, heads*64] in OT (fp32, or T itself: the 16-bit storage mode rounds the normalised output in the epilogue),
// LSE fp32 [n, heads, N] (natural log)
template <typename T, typename OT>
__global__ __launch_bounds__(WGT) void attn_train_fwd_kernel(const T* __restrict__ qkv, OT* __restrict__ out, float* __restrict__ lse,
                                                            int N, int heads) {
    typedef typename V8<T>::type vec8;
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TILE];      // [buffer][K | V]
    const int tid = threadIdx.x, lane = tid & 63, h2 = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nqb = (N + 127) >> 7;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);                    // the query blocks of one (sequence, head) on one XCD
    const int qb = tile % nqb, h = (tile / nqb) % heads, seq = tile / (nqb * heads);
    const int E = heads * 64, ld = 3 * E;
    const T* base = qkv + (int64_t)seq * N * ld;
    const int q0 = qb * 128 + wave * 32;
    const bool active = q0 < N;                                            // wave-uniform
    const int q = q0 + (lane & 31);

    vec8 bq[4];                                                            // B operand of S^T = K Q^T: Q[q][16 ds + 8 h2 + j]
    {
        const T* qp = base + (int64_t)(q < N ? q : N - 1) * ld + h * 64 + h2 * 8;
#pragma unroll
        for (int ds = 0; ds < 4; ++ds) bq[ds] = *reinterpret_cast<const vec8*>(qp + ds * 16);
    }
    Stage2<T> st;
    st.init(tid);
    const T* kbase = base + E + h * 64;
    f32x16 o[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) o[0][r] = o[1][r] = 0.f;
    float m = -INFINITY, l = 0.f;                                          // running maximum (log2 domain) and sum, per query and half
    const int nt = (N + 63) >> 6;
    st.load(kbase, ld, kbase + E, ld, 0, N);
    st.store(smem, smem + TILE);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        if (t + 1 < nt) st.load(kbase, ld, kbase + E, ld, (t + 1) * 64, N);
        if (active) {
            const char* Kt = smem + (t & 1) * 2 * TILE;
            const char* Vt = Kt + TILE;
            const bool upper = t * 64 + 32 < N;                            // keys 32 .. 63 of the tile hold a valid key
            f32x16 s[2];
            float mx = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
                if (kb == 1 && !upper) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[1][r] = -INFINITY;
                    continue;
                }
#pragma unroll
                for (int ds = 0; ds < 4; ++ds) s[kb] = mfma32(row_frag<T>(Kt, kb * 32 + (lane & 31), 2 * ds + h2), bq[ds], s[kb]);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = t * 64 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h2;
                    s[kb][r] = key < N ? s[kb][r] * LOG2E : -INFINITY;
                    mx = fmaxf(mx, s[kb][r]);
                }
            }
            const float m_new = fmaxf(m, half_max(mx));                    // finite: key t*64 < N is valid
            const float alpha = __builtin_amdgcn_exp2f(m - m_new);         // 0 on the first tile
            m = m_new;
            l *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                o[0][r] *= alpha;
                o[1][r] *= alpha;
            }
            vec8 pf[4];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = __builtin_amdgcn_exp2f(s[kb][r] - m_new);
                    l += p;
                    pf[2 * kb + (r >> 3)][r & 7] = (T)p;
                }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                if (ks >= 2 && !upper) continue;
#pragma unroll
                for (int db = 0; db < 2; ++db) o[db] = mfma32(tr_frag<T>(Vt, ks * 16, db, lane), pf[ks], o[db]);   // O^T += V^T P^T
            }
        }
        if (t + 1 < nt) st.store(smem + ((t + 1) & 1) * 2 * TILE, smem + ((t + 1) & 1) * 2 * TILE + TILE);
        __syncthreads();
    }
    if (active) {
        const float l_tot = half_sum(l);
        const float inv = 1.0f / l_tot;
        if (q < N) {
            const int64_t R = (int64_t)seq * N + q;
            OT* op = out + R * E + h * 64 + 4 * h2;                        // O^T[d = 32 db + 8 g + 4 h2 + e][q]
#pragma unroll
            for (int db = 0; db < 2; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = o[db][4 * g + e] * inv;
                    if constexpr (sizeof(OT) == 4) {
                        *reinterpret_cast<f32x4*>(op + db * 32 + g * 8) = v;
                    } else {
                        typename V8<T>::half_type v16;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v16[e] = (T)f32_rounded(v[e]);   // the bits of T(the fp32 output)
                        *reinterpret_cast<typename V8<T>::half_type*>(op + db * 32 + g * 8) = v16;
                    }
                }
            if (h2 == 0) lse[((int64_t)seq * heads + h) * N + q] = (m + __log2f(l_tot)) * LN2;
        }
    }
}

// ---- backward preprocess: one workgroup per (sequence, head).  Pass 1: m = max |dO| -> scale c = 2^min(6 - e, 126), m in [2^(e-1), 2^e):
// c m in [32, 64) down to m = 2^-121; below (denormals included) c stays 2^126, where 2^(6 - e) would be inf and every gradient NaN.
// Pass 2 (8 lanes per row): Dv[seq][h][q] = c sum_d dO o O (fp32 products; O fp32, or T as the 16-bit storage mode keeps it), do16 =
// 16-bit image of c dO; cs[seq][h] = c.
template <typename T, typename OT>
__global__ __launch_bounds__(256) void attn_train_pre_kernel(const OT* __restrict__ O, const float* __restrict__ dO, T* __restrict__ do16,
                                                            float* __restrict__ Dv, float* __restrict__ cs, int N, int heads) {
    typedef typename V8<T>::type vec8;
    __shared__ float red[4];
    const int tid = threadIdx.x, h = blockIdx.x % heads, seq = blockIdx.x / heads;
    const int E = heads * 64;
    const int64_t row0 = (int64_t)seq * N;
    float m = 0.f;
    for (int i = tid; i < N * 16; i += 256) {                              // float4 i: row i >> 4, columns 4 (i & 15) ..
        const f32x4 a = *reinterpret_cast<const f32x4*>(dO + (row0 + (i >> 4)) * E + h * 64 + (i & 15) * 4);
        m = fmaxf(m, fmaxf(fmaxf(fabsf(a[0]), fabsf(a[1])), fmaxf(fabsf(a[2]), fabsf(a[3]))));
    }
    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    int e = 0;
    (void)frexpf(m, &e);
    const float c = (m > 0.f && m <= 3.0e38f) ? ldexpf(1.0f, min(6 - e, 126)) : 1.0f;   // c, 1 / c finite and normal: 2^-122 .. 2^126
    const int sub = tid & 7;
    for (int q = tid >> 3; q < N; q += 32) {
        const int64_t off = (row0 + q) * E + h * 64 + sub * 8;
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(dO + off), a1 = *reinterpret_cast<const f32x4*>(dO + off + 4);
        f32x4 b0, b1;
        if constexpr (sizeof(OT) == 4) {
            b0 = *reinterpret_cast<const f32x4*>(O + off);
            b1 = *reinterpret_cast<const f32x4*>(O + off + 4);
        } else {
            const vec8 o8 = *reinterpret_cast<const vec8*>(O + off);
#pragma unroll
            for (int k = 0; k < 4; ++k) { b0[k] = (float)o8[k]; b1[k] = (float)o8[4 + k]; }
        }
        float acc = 0.f;
        vec8 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            acc = fmaf(a0[k], b0[k], acc);
            acc = fmaf(a1[k], b1[k], acc);
            v[k] = (T)(a0[k] * c);
            v[4 + k] = (T)(a1[k] * c);
        }
        *reinterpret_cast<vec8*>(do16 + off) = v;
        acc += __shfl_xor(acc, 1, 64);
        acc += __shfl_xor(acc, 2, 64);
        acc += __shfl_xor(acc, 4, 64);
        if (sub == 0) Dv[((int64_t)seq * heads + h) * N + q] = acc * c;
    }
    if (tid == 0) cs[(int64_t)seq * heads + h] = c;
}

// ---- key pass: dK, dV of 128 keys per workgroup (32 per wave), straight into dqkv [n*N, 3*heads*64] fp32
template <typename T>
__global__ __launch_bounds__(WGT) void attn_train_dkv_kernel(const T* __restrict__ qkv, const T* __restrict__ do16, const float* __restrict__ lse,
                                                            const float* __restrict__ Dv, const float* __restrict__ cs, float* __restrict__ dqkv,
                                                            int N, int heads) {
    typedef typename V8<T>::type vec8;
    constexpr int BUF = 2 * TILE + 2 * 64 * 4;                             // Q | dO | lse * log2 e [64] | D [64]
    __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
    const int tid = threadIdx.x, lane = tid & 63, h2 = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nkb = (N + 127) >> 7;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int kbk = tile % nkb, h = (tile / nkb) % heads, seq = tile / (nkb * heads);
    const int E = heads * 64, ld = 3 * E;
    const T* base = qkv + (int64_t)seq * N * ld;
    const T* obase = do16 + (int64_t)seq * N * E + h * 64;
    const float* lrow = lse + ((int64_t)seq * heads + h) * N;
    const float* drow = Dv + ((int64_t)seq * heads + h) * N;
    const int k0 = kbk * 128 + wave * 32;
    const bool active = k0 < N;

    vec8 kf[4], vf[4];                                                     // B operands of S = Q K^T and dP = dO V^T: K / V [key][16 ds + 8 h2 + j]
    {
        const int key = k0 + (lane & 31);
        const T* kp = base + (int64_t)(key < N ? key : N - 1) * ld + E + h * 64 + h2 * 8;
#pragma unroll
        for (int ds = 0; ds < 4; ++ds) {
            kf[ds] = *reinterpret_cast<const vec8*>(kp + ds * 16);
            vf[ds] = *reinterpret_cast<const vec8*>(kp + E + ds * 16);
        }
    }
    Stage2<T> st;
    st.init(tid);
    float sreg = 0.f;                                                      // threads 0 .. 127: one row statistic of the next tile
    auto sload = [&](int t) {
        if (tid < 128) {
            const int q = t * 64 + (tid & 63);
            sreg = tid < 64 ? (q < N ? lrow[q] * LOG2E : INFINITY)         // rows past N: P = 0
                            : (q < N ? drow[q] : 0.f);
        }
    };
    auto sstore = [&](char* b) {
        if (tid < 128) reinterpret_cast<float*>(b + 2 * TILE)[tid] = sreg;
    };
    f32x16 dk[2], dv[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[0][r] = dk[1][r] = dv[0][r] = dv[1][r] = 0.f;
    const int nt = (N + 63) >> 6;
    st.load(base + h * 64, ld, obase, E, 0, N);
    sload(0);
    st.store(smem, smem + TILE);
    sstore(smem);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        if (t + 1 < nt) {
            st.load(base + h * 64, ld, obase, E, (t + 1) * 64, N);
            sload(t + 1);
        }
        if (active) {
            const char* Qt = smem + (t & 1) * BUF;
            const char* Ot = Qt + TILE;
            const float* ls = reinterpret_cast<const float*>(Qt + 2 * TILE);
            const float* dd = ls + 64;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                if (sub == 1 && t * 64 + 32 >= N) continue;               // wave-uniform: no valid query in rows 32 .. 63
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
#pragma unroll
                for (int ds = 0; ds < 4; ++ds) {
                    s = mfma32(row_frag<T>(Qt, sub * 32 + (lane & 31), 2 * ds + h2), kf[ds], s);      // S[q][key]
                    dp = mfma32(row_frag<T>(Ot, sub * 32 + (lane & 31), 2 * ds + h2), vf[ds], dp);    // dP[q][key]
                }
                vec8 pf[2], sf[2];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int qr = sub * 32 + 8 * g + 4 * h2;              // rows of registers 4g .. 4g+3
                    const f32x4 l4 = *reinterpret_cast<const f32x4*>(ls + qr);
                    const f32x4 d4 = *reinterpret_cast<const f32x4*>(dd + qr);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int r = 4 * g + e;
                        const float p = __builtin_amdgcn_exp2f(fmaf(s[r], LOG2E, -l4[e]));
                        pf[r >> 3][r & 7] = (T)p;
                        sf[r >> 3][r & 7] = (T)(p * (dp[r] - d4[e]));
                    }
                }
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int db = 0; db < 2; ++db) {
                        dv[db] = mfma32(pf[ks], tr_frag<T>(Ot, sub * 32 + ks * 16, db, lane), dv[db]);   // dV += P^T dO
                        dk[db] = mfma32(sf[ks], tr_frag<T>(Qt, sub * 32 + ks * 16, db, lane), dk[db]);   // dK += dS^T Q
                    }
            }
        }
        if (t + 1 < nt) {
            char* b = smem + ((t + 1) & 1) * BUF;
            st.store(b, b + TILE);
            sstore(b);
        }
        __syncthreads();
    }
    if (active) {
        const float ic = 1.0f / cs[(int64_t)seq * heads + h];              // exact: c is a power of two
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * h2;
            if (key < N) {
                float* p = dqkv + ((int64_t)seq * N + key) * ld + E + h * 64 + (lane & 31);
                p[0] = dk[0][r] * ic;
                p[32] = dk[1][r] * ic;
                p[E] = dv[0][r] * ic;
                p[E + 32] = dv[1][r] * ic;
            }
        }
    }
}

// ---- query pass: dQ of 128 queries per workgroup (32 per wave), times dq_scale, into dqkv's q columns
template <typename T>
__global__ __launch_bounds__(WGT) void attn_train_dq_kernel(const T* __restrict__ qkv, const T* __restrict__ do16, const float* __restrict__ lse,
                                                           const float* __restrict__ Dv, const float* __restrict__ cs, float* __restrict__ dqkv,
                                                           int N, int heads, float dq_scale) {
    typedef typename V8<T>::type vec8;
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TILE];      // [buffer][K | V]
    const int tid = threadIdx.x, lane = tid & 63, h2 = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nqb = (N + 127) >> 7;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int qb = tile % nqb, h = (tile / nqb) % heads, seq = tile / (nqb * heads);
    const int E = heads * 64, ld = 3 * E;
    const T* base = qkv + (int64_t)seq * N * ld;
    const int q0 = qb * 128 + wave * 32;
    const bool active = q0 < N;
    const int q = q0 + (lane & 31), qc = q < N ? q : N - 1;

    vec8 bq[4], bo[4];                                                     // B operands of S^T = K Q^T and dP^T = V dO^T
    {
        const T* qp = base + (int64_t)qc * ld + h * 64 + h2 * 8;
        const T* op = do16 + ((int64_t)seq * N + qc) * E + h * 64 + h2 * 8;
#pragma unroll
        for (int ds = 0; ds < 4; ++ds) {
            bq[ds] = *reinterpret_cast<const vec8*>(qp + ds * 16);
            bo[ds] = *reinterpret_cast<const vec8*>(op + ds * 16);
        }
    }
    const int64_t srow = ((int64_t)seq * heads + h) * N + qc;
    const float l2 = lse[srow] * LOG2E, dd = Dv[srow];
    Stage2<T> st;
    st.init(tid);
    const T* kbase = base + E + h * 64;
    f32x16 dq[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[0][r] = dq[1][r] = 0.f;
    const int nt = (N + 63) >> 6;
    st.load(kbase, ld, kbase + E, ld, 0, N);
    st.store(smem, smem + TILE);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        if (t + 1 < nt) st.load(kbase, ld, kbase + E, ld, (t + 1) * 64, N);
        if (active) {
            const char* Kt = smem + (t & 1) * 2 * TILE;
            const char* Vt = Kt + TILE;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                if (kb == 1 && t * 64 + 32 >= N) continue;                // wave-uniform: no valid key in rows 32 .. 63
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
#pragma unroll
                for (int ds = 0; ds < 4; ++ds) {
                    s = mfma32(row_frag<T>(Kt, kb * 32 + (lane & 31), 2 * ds + h2), bq[ds], s);       // S^T[key][q]
                    dp = mfma32(row_frag<T>(Vt, kb * 32 + (lane & 31), 2 * ds + h2), bo[ds], dp);     // dP^T[key][q]
                }
                vec8 sf[2];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = t * 64 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h2;
                    const float p = key < N ? __builtin_amdgcn_exp2f(fmaf(s[r], LOG2E, -l2)) : 0.f;
                    sf[r >> 3][r & 7] = (T)(p * (dp[r] - dd));
                }
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int db = 0; db < 2; ++db) dq[db] = mfma32(sf[ks], tr_frag<T>(Kt, kb * 32 + ks * 16, db, lane), dq[db]);   // dQ += dS K
            }
        }
        if (t + 1 < nt) st.store(smem + ((t + 1) & 1) * 2 * TILE, smem + ((t + 1) & 1) * 2 * TILE + TILE);
        __syncthreads();
    }
    if (active) {
        dq_scale /= cs[(int64_t)seq * heads + h];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qq = q0 + (r & 3) + 8 * (r >> 2) + 4 * h2;
            if (qq < N) {
                float* p = dqkv + ((int64_t)seq * N + qq) * ld + h * 64 + (lane & 31);
                p[0] = dq[0][r] * dq_scale;
                p[32] = dq[1][r] * dq_scale;
            }
        }
    }
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

size_t attn_train_workspace_bytes(int n_seq, int N, int heads) {
    if (n_seq <= 0 || N <= 0 || heads <= 0) return 0;
    const size_t rows = (size_t)n_seq * N;
    return align256(rows * heads * 64 * 2) + align256(rows * heads * 4) + align256((size_t)n_seq * heads * 4);
}

int launch_attn_train_fwd(const void* qkv, int dt, int n_seq, int N, int heads, void* out, int out16, float* lse, hipStream_t s) {
    MST_CHECK_ARG(n_seq > 0 && N > 0 && heads > 0, "attention_train_fwd: bad sizes n_seq=%d N=%d heads=%d", n_seq, N, heads);
    const int64_t nwg = (int64_t)((N + 127) / 128) * heads * n_seq;
    MST_CHECK_ARG(nwg < (1ll << 31), "attention_train_fwd: grid too large");
    const dim3 grid((unsigned)nwg), block(WGT);
    if (dt == MST_BF16 && out16) attn_train_fwd_kernel<bf16_t, bf16_t><<<grid, block, 0, s>>>((const bf16_t*)qkv, (bf16_t*)out, lse, N, heads);
    else if (dt == MST_BF16) attn_train_fwd_kernel<bf16_t, float><<<grid, block, 0, s>>>((const bf16_t*)qkv, (float*)out, lse, N, heads);
    else if (dt == MST_F16 && out16) attn_train_fwd_kernel<f16_t, f16_t><<<grid, block, 0, s>>>((const f16_t*)qkv, (f16_t*)out, lse, N, heads);
    else if (dt == MST_F16) attn_train_fwd_kernel<f16_t, float><<<grid, block, 0, s>>>((const f16_t*)qkv, (float*)out, lse, N, heads);
    else { mst_set_error("attention_train_fwd: dtype %d unsupported (bf16 or fp16 qkv)", dt); return MST_EINVAL; }
    return mst_check_launch("attention_train_fwd");
}

int launch_attn_train_bwd(const void* qkv, int dt, const void* out, int out16, const float* dout, const float* lse, int n_seq, int N, int heads,
                          float dq_scale, float* dqkv, void* ws, size_t ws_bytes, hipStream_t s) {
    MST_CHECK_ARG(n_seq > 0 && N > 0 && heads > 0, "attention_train_bwd: bad sizes n_seq=%d N=%d heads=%d", n_seq, N, heads);
    MST_CHECK_ARG(dt == MST_BF16 || dt == MST_F16, "attention_train_bwd: dtype %d unsupported (bf16 or fp16 qkv)", dt);
    const size_t need = attn_train_workspace_bytes(n_seq, N, heads);
    MST_CHECK_ARG(ws && ws_bytes >= need, "attention_train_bwd: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const int64_t nwg = (int64_t)((N + 127) / 128) * heads * n_seq;
    MST_CHECK_ARG(nwg < (1ll << 31), "attention_train_bwd: grid too large");
    const int64_t rows = (int64_t)n_seq * N;
    const int64_t pre_blocks = (int64_t)n_seq * heads;                     // < nwg
    char* w = (char*)ws;
    float* Dv = (float*)(w + align256((size_t)rows * heads * 64 * 2));
    float* cs = (float*)((char*)Dv + align256((size_t)rows * heads * 4));
    const dim3 grid((unsigned)nwg), block(WGT);
    if (dt == MST_BF16) {
        bf16_t* o16 = (bf16_t*)w;
        if (out16) attn_train_pre_kernel<bf16_t, bf16_t><<<dim3((unsigned)pre_blocks), dim3(256), 0, s>>>((const bf16_t*)out, dout, o16, Dv, cs, N, heads);
        else attn_train_pre_kernel<bf16_t, float><<<dim3((unsigned)pre_blocks), dim3(256), 0, s>>>((const float*)out, dout, o16, Dv, cs, N, heads);
        attn_train_dkv_kernel<bf16_t><<<grid, block, 0, s>>>((const bf16_t*)qkv, o16, lse, Dv, cs, dqkv, N, heads);
        attn_train_dq_kernel<bf16_t><<<grid, block, 0, s>>>((const bf16_t*)qkv, o16, lse, Dv, cs, dqkv, N, heads, dq_scale);
    } else {
        f16_t* o16 = (f16_t*)w;
        if (out16) attn_train_pre_kernel<f16_t, f16_t><<<dim3((unsigned)pre_blocks), dim3(256), 0, s>>>((const f16_t*)out, dout, o16, Dv, cs, N, heads);
        else attn_train_pre_kernel<f16_t, float><<<dim3((unsigned)pre_blocks), dim3(256), 0, s>>>((const float*)out, dout, o16, Dv, cs, N, heads);
        attn_train_dkv_kernel<f16_t><<<grid, block, 0, s>>>((const f16_t*)qkv, o16, lse, Dv, cs, dqkv, N, heads);
        attn_train_dq_kernel<f16_t><<<grid, block, 0, s>>>((const f16_t*)qkv, o16, lse, Dv, cs, dqkv, N, heads, dq_scale);
    }
    return mst_check_launch("attention_train_bwd");
}
