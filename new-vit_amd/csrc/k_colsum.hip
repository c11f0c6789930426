// Column reductions of the training steps: out[c] += sum_r f(a[r][c], b[r][c]) over [rows, cols] -- the bias, LayerScale and BatchNorm
// sums.  ONE kernel template serves the atomic and the fixed-order (torch.use_deterministic_algorithms) entry points and the fp32 and
// 16-bit factors b, so every form walks the rows in the same order and returns the same bits where the forms can meet
// (mst_colsum_b16_ordered = mst_colsum_ordered on the upcast factor; one row block: atomic = ordered).
//   pass 1   workgroup (rb, cb) owns rows [rb*rpb, (rb+1)*rpb) x 64 columns; thread row ty runs down rows r0 + ty + TY k in sequence, the TY
//            partial sums meet in LDS in ascending ty.  ATOMIC: one atomicAdd per column per workgroup.  SLAB: one plain store per column
//            into slab[rb] -- with one row block, out += instead.
//   pass 2   (SLAB, slab_reduce) every column sums slab[0..nrb) -- 16 row phases, each in ascending rb, then ascending phase -- and adds
//            the total to the output: an order that is a pure function of the shape arguments.
//   plan     the row-block size depends on (rows, cols) only: about 2,048 workgroups, at least 64 rows each.
#include "mst_common.h"

namespace {

enum { OP_SUM = 0, OP_SQDEV = 1, OP_BN_BWD = 2 };
enum { ATOMIC = 0, SLAB = 1 };

__device__ __forceinline__ void load4(const float* p, float v[4]) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = t[e];
}
template <typename T>
__device__ __forceinline__ void load4(const T* p, float v[4]) {
    const typename V8<T>::half_type t = *reinterpret_cast<const typename V8<T>::half_type*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (float)t[e];
}

// OP_SUM:    acc0 = sum_r a[r][c] * (b ? b[r][c] : 1)
// OP_SQDEV:  acc0 = sum_r (a[r][c] - m[c])^2
// OP_BN_BWD: acc0 = sum_r b[r][c] (a[r][c] - m[c]) rs[c]  (d gamma; a = z, b = dy),  acc1 = sum_r b[r][c]  (d beta)
// A 256-thread block: 16 threads x 4 columns across and 16 thread rows down the chunk (VEC: 16-byte loads of a, 16 or 8 bytes of b), or
// -- the scalar ATOMIC form -- 64 threads x 1 column and 4 thread rows.
// Output j of row block rb.  ATOMIC: o_j[c] by atomicAdd.  SLAB: o_j[rb * ostride + c] (= the slab), or o_j[c] += when `direct`.
// Argument order: what the atomic column sum reads comes first and fills one 64-byte line of the kernel-argument segment.  Its
// workgroups live for four loop iterations at the step's shapes, and a second line to fetch showed as +0.1 .. 0.4 us per launch.
template <int OP, typename BT, bool VEC, int OUT>
__global__ __launch_bounds__(256) void colreduce_kernel(const float* __restrict__ a, int64_t as, const BT* __restrict__ b, int64_t bs, int64_t rows,
                                                        int64_t rpb, float* o0, int cols, int cblocks, const float* __restrict__ m,
                                                        const float* __restrict__ rs, float* o1, int64_t ostride, int direct) {
    constexpr int NA = OP == OP_BN_BWD ? 2 : 1;
    constexpr int CW = (VEC || OUT == SLAB) ? 4 : 1, TX = 64 / CW, TY = 256 / TX;
    __shared__ float red[NA][TY][64 + 4];
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    // ATOMIC: row blocks on gridDim.x (2^31 - 1 blocks), column blocks on gridDim.y: the stem's BatchNorm sums of a 2 x 128 x 512^2 ResNet
    // step have 16.8 M rows, more row blocks than gridDim.y takes.  SLAB: a 1-D grid rb * cblocks + cb.
    const int64_t rb = OUT == ATOMIC ? blockIdx.x : blockIdx.x / cblocks;
    const int cb = OUT == ATOMIC ? (int)blockIdx.y : (int)(blockIdx.x - rb * cblocks);
    const int64_t r0 = rb * rpb, r1 = r0 + rpb < rows ? r0 + rpb : rows;
    const int c0 = cb * 64 + tx * CW;
    float acc[NA][CW];
    float mc[CW], rc[CW];
#pragma unroll
    for (int e = 0; e < CW; ++e) {
        acc[0][e] = acc[NA - 1][e] = 0.f;
        const bool in = c0 + e < cols;
        mc[e] = (OP != OP_SUM && in) ? m[c0 + e] : 0.f;
        rc[e] = (OP == OP_BN_BWD && in) ? rs[c0 + e] : 0.f;
    }
    if (c0 < cols) {
        for (int64_t r = r0 + ty; r < r1; r += TY) {
            float av[CW], bv[CW];
            if constexpr (VEC) {
                load4(a + r * as + c0, av);
                if (b) load4(b + r * bs + c0, bv);
                else bv[0] = bv[1] = bv[2] = bv[3] = 1.f;
            } else {
#pragma unroll
                for (int e = 0; e < CW; ++e) {
                    const bool in = c0 + e < cols;
                    av[e] = in ? a[r * as + c0 + e] : 0.f;
                    bv[e] = (in && b) ? to_f32(b[r * bs + c0 + e]) : 1.f;
                }
            }
#pragma unroll
            for (int e = 0; e < CW; ++e) {
                if (OP == OP_SUM) acc[0][e] = fmaf(av[e], bv[e], acc[0][e]);
                else if (OP == OP_SQDEV) { const float d = av[e] - mc[e]; acc[0][e] = fmaf(d, d, acc[0][e]); }
                else {
                    acc[0][e] = fmaf(bv[e], (av[e] - mc[e]) * rc[e], acc[0][e]);
                    acc[NA - 1][e] += bv[e];
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NA; ++j)
#pragma unroll
        for (int e = 0; e < CW; ++e) red[j][ty][tx * CW + e] = acc[j][e];
    __syncthreads();
    if (threadIdx.x < 64 * NA) {
        const int j = threadIdx.x >> 6, cl = threadIdx.x & 63, cc = cb * 64 + cl;
        float t = 0.f;
#pragma unroll
        for (int y = 0; y < TY; ++y) t += red[j][y][cl];
        if (cc < cols) {
            if constexpr (OUT == ATOMIC) {
                atomicAdd((j ? o1 : o0) + cc, t);
            } else {
                float* p = (j ? o1 : o0) + rb * ostride + cc;
                *p = direct ? *p + t : t;
            }
        }
    }
}

// out[col] += sum_{rb < nrb} slab[rb][col] for col < width; columns below `split` go to o0, the rest to o1[col - split] (either
// nullable).  64 columns x 16 row phases per workgroup; phase p sums rb = p, p + 16, ... in sequence, the phases meet in ascending p.
__global__ __launch_bounds__(1024) void slab_reduce_kernel(const float* __restrict__ slab, int64_t nrb, int64_t width, int64_t split,
                                                           float* o0, float* o1) {
    __shared__ float red[16][64];
    const int cl = threadIdx.x & 63, p = threadIdx.x >> 6;
    const int64_t col = (int64_t)blockIdx.x * 64 + cl;
    float s = 0.f;
    if (col < width) {
#pragma unroll 8
        for (int64_t rb = p; rb < nrb; rb += 16) s += slab[rb * width + col];
    }
    red[p][cl] = s;
    __syncthreads();
    if (p == 0 && col < width) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) t += red[q][cl];
        float* o = col < split ? (o0 ? o0 + col : nullptr) : (o1 ? o1 + (col - split) : nullptr);
        if (o) *o += t;
    }
}

// the row blocks: enough workgroups to fill the chip (about 2,048), chunks of at least 64 rows so that the atomics / slabs stay few
void colsum_plan(int64_t rows, int cols, int64_t& rpb, int64_t& rblocks) {
    const int64_t cblocks = (cols + 63) / 64;
    rpb = (rows * cblocks + 2047) / 2048;
    rpb = rpb < 64 ? 64 : (rpb + 15) / 16 * 16;
    rblocks = (rows + rpb - 1) / rpb;
}

// Every entry point's argument checks; returns the plan and whether the 16-byte path applies.  A 16-bit b has no scalar path.
int colreduce_args(const char* what, const float* a, int64_t as, const void* b, int dt, int64_t bs, int64_t rows, int cols, bool ordered,
                   int outputs, const void* ws, size_t ws_bytes, int64_t& rpb, int64_t& rblocks, bool& vec) {
    MST_CHECK_ARG(rows > 0 && cols > 0, "%s: rows=%lld cols=%d out of range", what, (long long)rows, cols);
    vec = cols % 4 == 0 && as % 4 == 0 && aligned(a, 16) && (!b || (bs % 4 == 0 && aligned(b, dt == MST_F32 ? 16 : 8)));
    MST_CHECK_ARG(dt == MST_F32 || (vec && as >= cols && bs >= cols),
                  "%s: cols=%d and the row strides must be multiples of 4 (strides >= cols), a 16-byte and b 8-byte aligned", what, cols);
    colsum_plan(rows, cols, rpb, rblocks);
    const int64_t cblocks = (cols + 63) / 64;
    if (!ordered) {
        MST_CHECK_ARG(cblocks <= 65535, "%s: cols=%d out of range", what, cols);
        MST_CHECK_ARG(rblocks < (1ll << 31), "%s: rows=%lld out of range", what, (long long)rows);
        return MST_OK;
    }
    MST_CHECK_ARG(rblocks * cblocks < (1ll << 31), "%s: rows=%lld cols=%d out of range", what, (long long)rows, cols);
    const size_t need = colsum_ordered_workspace_bytes(rows, cols, outputs);
    MST_CHECK_ARG(ws_bytes >= need && (need == 0 || ws), "%s: workspace of %zu bytes, %zu needed", what, ws_bytes, need);
    return MST_OK;
}

// b: fp32, or (OP_SUM) bf16 / fp16 as `dt` says.  ordered: the SLAB form with its workspace; otherwise (OP_SUM only) the ATOMIC form.
template <int OP>
int colreduce_launch(const char* what, const float* a, int64_t as, const void* b, int dt, int64_t bs, const float* m, const float* rs,
                     int64_t rows, int cols, float* out0, float* out1, bool ordered, void* ws, size_t ws_bytes, hipStream_t s) {
    constexpr int NA = OP == OP_BN_BWD ? 2 : 1;
    int64_t rpb, rblocks;
    bool vec;
    if (int rc = colreduce_args(what, a, as, b, dt, bs, rows, cols, ordered, NA, ws, ws_bytes, rpb, rblocks, vec)) return rc;
    const int cblocks = (cols + 63) / 64;
    const bool direct = rblocks == 1;
    float* slab = (float*)ws;
    float* o0 = (!ordered || direct) ? out0 : slab;
    float* o1 = (!ordered || direct) ? out1 : slab + cols;
    const dim3 grid = ordered ? dim3((unsigned)(rblocks * cblocks)) : dim3((unsigned)rblocks, cblocks);
#define COLREDUCE_AS(BT, VEC, OUT) \
    colreduce_kernel<OP, BT, VEC, OUT><<<grid, dim3(256), 0, s>>>(a, as, (const BT*)b, bs, rows, rpb, o0, cols, cblocks, m, rs, o1, (int64_t)NA * cols, direct)
#define COLREDUCE(BT, VEC)                                       \
    do {                                                         \
        if (ordered) COLREDUCE_AS(BT, VEC, SLAB);                \
        else if constexpr (OP == OP_SUM) COLREDUCE_AS(BT, VEC, ATOMIC); \
    } while (0)
    if (dt == MST_F32) {
        if (vec) COLREDUCE(float, true);
        else COLREDUCE(float, false);
    } else if constexpr (OP == OP_SUM) {
        if (dt == MST_BF16) COLREDUCE(bf16_t, true);
        else COLREDUCE(f16_t, true);
    }
#undef COLREDUCE
#undef COLREDUCE_AS
    int rc = mst_check_launch(what);
    if (rc || !ordered || direct) return rc;
    return launch_slab_reduce(slab, rblocks, (int64_t)NA * cols, cols, out0, out1, s);
}

int colsum_b16(const char* what, const float* a, int64_t as, const void* b, int dt, int64_t bs, int64_t rows, int cols, float* out,
               bool ordered, void* ws, size_t ws_bytes, hipStream_t s) {
    MST_CHECK_ARG(dt == MST_BF16 || dt == MST_F16, "%s: dtype %d (bf16 / f16)", what, dt);
    return colreduce_launch<OP_SUM>(what, a, as, b, dt, bs, nullptr, nullptr, rows, cols, out, nullptr, ordered, ws, ws_bytes, s);
}

}  // namespace

size_t colsum_ordered_workspace_bytes(int64_t rows, int cols, int outputs) {
    if (rows <= 0 || cols <= 0) return 0;
    int64_t rpb, rblocks;
    colsum_plan(rows, cols, rpb, rblocks);
    return rblocks > 1 ? (sizeof(float) * (size_t)rblocks * outputs * cols + 255) / 256 * 256 : 0;
}

int launch_slab_reduce(const float* slab, int64_t nrb, int64_t width, int64_t split, float* o0, float* o1, hipStream_t s) {
    MST_CHECK_ARG(nrb > 0 && width > 0 && (width + 63) / 64 < (1ll << 31), "slab_reduce: nrb=%lld width=%lld out of range", (long long)nrb,
                  (long long)width);
    slab_reduce_kernel<<<dim3((unsigned)((width + 63) / 64)), dim3(1024), 0, s>>>(slab, nrb, width, split, o0, o1);
    return mst_check_launch("slab_reduce");
}

int launch_colsum(const float* a, int64_t as, const float* b, int64_t bs, int64_t rows, int cols, float* out, hipStream_t s) {
    return colreduce_launch<OP_SUM>("colsum", a, as, b, MST_F32, bs, nullptr, nullptr, rows, cols, out, nullptr, false, nullptr, 0, s);
}

int launch_colsum_ordered(const float* a, int64_t as, const float* b, int64_t bs, int64_t rows, int cols, float* out, void* ws,
                          size_t ws_bytes, hipStream_t s) {
    return colreduce_launch<OP_SUM>("colsum_ordered", a, as, b, MST_F32, bs, nullptr, nullptr, rows, cols, out, nullptr, true, ws, ws_bytes, s);
}

int launch_colsum_b16(const float* a, int64_t as, const void* b, int dt, int64_t bs, int64_t rows, int cols, float* out, hipStream_t s) {
    return colsum_b16("colsum_b16", a, as, b, dt, bs, rows, cols, out, false, nullptr, 0, s);
}

int launch_colsum_b16_ordered(const float* a, int64_t as, const void* b, int dt, int64_t bs, int64_t rows, int cols, float* out, void* ws,
                              size_t ws_bytes, hipStream_t s) {
    return colsum_b16("colsum_b16_ordered", a, as, b, dt, bs, rows, cols, out, true, ws, ws_bytes, s);
}

int launch_colsqdev_ordered(const float* z, const float* mean, int64_t rows, int C, float* out, void* ws, size_t ws_bytes, hipStream_t s) {
    return colreduce_launch<OP_SQDEV>("colsqdev_ordered", z, C, nullptr, MST_F32, 0, mean, nullptr, rows, C, out, nullptr, true, ws, ws_bytes, s);
}

int launch_bn_bwd_reduce_ordered(const float* z, const float* mean, const float* rstd, const float* dy, int64_t rows, int C, float* dgamma,
                                 float* dbeta, void* ws, size_t ws_bytes, hipStream_t s) {
    return colreduce_launch<OP_BN_BWD>("bn_bwd_reduce_ordered", z, C, dy, MST_F32, C, mean, rstd, rows, C, dgamma, dbeta, true, ws, ws_bytes, s);
}
