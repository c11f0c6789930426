// Column reductions of the training steps: out[c] += sum_r f(a[r][c], b[r][c]) over [rows, cols] -- the bias, LayerScale and BatchNorm
// sums.  ONE kernel template serves the atomic and the fixed-order (torch.use_deterministic_algorithms) entry points, the fp32 and 16-bit
// factors b and the fp32 and 16-bit BatchNorm inputs a, so every form walks the rows in the same order and returns the same bits where the
// forms can meet (mst_colsum_b16_ordered = mst_colsum_ordered on the upcast factor; one row block: atomic = ordered; at most one row per
// thread row: the sums of a 16-bit z = those of the upcast z).
//   pass 1   workgroup (rb, cb) owns rows [rb*rpb, (rb+1)*rpb) x 64 columns; thread row ty runs down rows r0 + ty + TY k in sequence, the TY
//            partial sums meet in LDS in ascending ty.  ATOMIC: one atomicAdd per column per workgroup.  SLAB: one plain store per column
//            into slab[rb] -- with one row block, out += instead.
//   pass 2   (SLAB, slab_reduce) every column sums slab[0..nrb) -- 16 row phases, each in ascending rb, then ascending phase -- and adds
//            the total to the output: an order that is a pure function of the shape arguments.
//   plan     the row-block size depends on (rows, cols) and the thread-row count only: about 2,048 workgroups, at least 64 rows each, a
//            multiple of 16 rows (fp32 a) or of 32 (16-bit a: CW = 8, so TY = 32).
#include "mst_common.h"

namespace {

enum { OP_SUM = COL_SUM, OP_SQDEV = COL_SQDEV, OP_BN_BWD = COL_BN_BWD };
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
// OP_BN_BWD: acc0 = sum_r g (a[r][c] - m[c]) rs[c]  (d gamma; a = z),  acc1 = sum_r g  (d beta);  g = b[r][c] (= dy), times the ReLU mask
//            (y[r][c] > 0 ? 1 : 0) when a is 16-bit and y is given
// A 256-thread block: TX = 64 / CW threads x CW columns across and TY = 256 / TX thread rows down the chunk.  CW = 4 (VEC: 16-byte loads of
// the fp32 a, 16 or 8 bytes of b; the scalar form, ATOMIC and SLAB alike: four guarded loads -- one geometry, so that "one row block:
// atomic = ordered" holds for odd column counts too; a one-column-per-thread ATOMIC form had TY = 4 and another row order) or CW = 8
// (a 16-bit a: ONE 16-byte load of a and of y, two of the fp32 b and of the per-column vectors; cols % 8 == 0).
// Output j of row block rb.  ATOMIC: o_j[c] by atomicAdd.  SLAB: o_j[rb * ostride + c] (= the slab), or o_j[c] += when `direct`.
// Argument order: what the atomic column sum reads comes first and fills one 64-byte line of the kernel-argument segment.  Its
// workgroups live for four loop iterations at the step's shapes, and a second line to fetch showed as +0.1 .. 0.4 us per launch.
template <int OP, typename AT, typename BT, int CW, bool VEC, int OUT>
__global__ __launch_bounds__(256) void colreduce_kernel(const AT* __restrict__ a, int64_t as, const BT* __restrict__ b, int64_t bs, int64_t rows,
                                                        int64_t rpb, float* o0, int cols, int cblocks, const float* __restrict__ m,
                                                        const float* __restrict__ rs, float* o1, int64_t ostride, int direct,
                                                        const AT* __restrict__ y) {
    constexpr int NA = OP == OP_BN_BWD ? 2 : 1;
    constexpr int TX = 64 / CW, TY = 256 / TX;
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
        if constexpr (CW == 8) {
            mc[e] = rc[e] = 0.f;
        } else {
            const bool in = c0 + e < cols;
            mc[e] = (OP != OP_SUM && in) ? m[c0 + e] : 0.f;
            rc[e] = (OP == OP_BN_BWD && in) ? rs[c0 + e] : 0.f;
        }
    }
    if (c0 < cols) {
        if constexpr (CW == 8) {
            if (OP != OP_SUM) load8(m + c0, mc);
            if (OP == OP_BN_BWD) load8(rs + c0, rc);
        }
        constexpr int UNROLL = CW == 8 ? 2 : 1;                          // CW = 8: two rows' 16-byte loads in flight; 1: the loop as written
#pragma unroll UNROLL
        for (int64_t r = r0 + ty; r < r1; r += TY) {
            float av[CW], bv[CW];
            if constexpr (CW == 8) {
                const int64_t off = r * as + c0;                         // a, b and y share their row stride
                load8(a + off, av);
                if constexpr (OP == OP_BN_BWD) {
                    load8(b + off, bv);
                    if (y) {
                        float yv[CW];
                        load8(y + off, yv);
#pragma unroll
                        for (int e = 0; e < CW; ++e) bv[e] *= act_deriv(yv[e], 1);
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < CW; ++e) bv[e] = 1.f;
                }
            } else if constexpr (VEC) {
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
        for (int q = 0; q < TY; ++q) t += red[j][q][cl];
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

}  // namespace

// the row blocks: enough workgroups to fill the chip (about 2,048), chunks of at least 64 rows so that the atomics / slabs stay few;
// whole sweeps of the `ty` thread rows
void colsum_plan(int64_t rows, int cols, int ty, int64_t& rpb, int64_t& rblocks) {
    const int64_t cblocks = (cols + 63) / 64;
    rpb = (rows * cblocks + 2047) / 2048;
    rpb = rpb < 64 ? 64 : (rpb + ty - 1) / ty * ty;
    rblocks = (rows + rpb - 1) / rpb;
}

namespace {

// Every entry point's argument checks; returns the plan and whether the 16-byte path applies.  A 16-bit a or b has no scalar path.
int colreduce_args(const char* what, const void* a, int adt, int64_t as, const void* b, int dt, int64_t bs, int64_t rows, int cols, bool ordered,
                   int outputs, const void* ws, size_t ws_bytes, int64_t& rpb, int64_t& rblocks, bool& vec) {
    MST_CHECK_ARG(rows > 0 && cols > 0, "%s: rows=%lld cols=%d out of range", what, (long long)rows, cols);
    vec = cols % 4 == 0 && as % 4 == 0 && aligned(a, 16) && (!b || (bs % 4 == 0 && aligned(b, dt == MST_F32 ? 16 : 8)));
    MST_CHECK_ARG(dt == MST_F32 || (vec && as >= cols && bs >= cols),
                  "%s: cols=%d and the row strides must be multiples of 4 (strides >= cols), a 16-byte and b 8-byte aligned", what, cols);
    MST_CHECK_ARG(adt == MST_F32 || (ordered && dt == MST_F32 && vec && cols % 8 == 0 && as % 8 == 0 && (!b || bs == as)),
                  "%s: a 16-bit input takes the fixed order, cols=%d and ONE row stride that are multiples of 8, 16-byte aligned operands", what, cols);
    const int ty = adt == MST_F32 ? 16 : 32;
    colsum_plan(rows, cols, ty, rpb, rblocks);
    const int64_t cblocks = (cols + 63) / 64;
    // one bound for both forms: SLAB puts rblocks * cblocks on gridDim.x, ATOMIC the row blocks (its column blocks go in pieces, below)
    MST_CHECK_ARG(rblocks * cblocks < (1ll << 31), "%s: rows=%lld cols=%d out of range", what, (long long)rows, cols);
    if (!ordered) return MST_OK;
    const size_t need = colsum_ordered_workspace_bytes(rows, cols, outputs, ty);
    MST_CHECK_ARG(ws_bytes >= need && (need == 0 || ws), "%s: workspace of %zu bytes, %zu needed", what, ws_bytes, need);
    return MST_OK;
}

// a: fp32, or (the BatchNorm sums, ordered only) bf16 / fp16 as `adt` says, with y (nullable) the mask operand of OP_BN_BWD.  b: fp32, or
// (OP_SUM) bf16 / fp16 as `dt` says.  ordered: the SLAB form with its workspace; otherwise the ATOMIC form.
template <int OP>
int colreduce_launch(const char* what, const void* a, int adt, int64_t as, const void* b, int dt, int64_t bs, const float* m, const float* rs,
                     const void* y, int64_t rows, int cols, float* out0, float* out1, bool ordered, void* ws, size_t ws_bytes, hipStream_t s) {
    constexpr int NA = OP == OP_BN_BWD ? 2 : 1;
    int64_t rpb, rblocks;
    bool vec;
    if (int rc = colreduce_args(what, a, adt, as, b, dt, bs, rows, cols, ordered, NA, ws, ws_bytes, rpb, rblocks, vec)) return rc;
    MST_CHECK_ARG(adt == MST_F32 || (aligned(y, 16) && aligned(m, 16) && aligned(rs, 16)), "%s: every pointer must be 16-byte aligned", what);
    const int cblocks = (cols + 63) / 64;
    const bool direct = rblocks == 1;
    float* slab = (float*)ws;
    float* o0 = (!ordered || direct) ? out0 : slab;
    float* o1 = (!ordered || direct) ? out1 : slab + cols;
    // ATOMIC: gridDim.y takes 65,535 column blocks, so wider operands (the weight-gradient partials of ViT-L / g: [splits, 4096 * 1024]
    // and up) go in pieces of PIECE whole blocks -- the kernel sees a [rows, pc] column block of the matrix at column p0, which the row
    // strides already allow.  The plan (rpb) is that of the full shape; PIECE * 64 columns keep every piece's base 16-byte aligned and
    // its width = cols (mod 4), so `vec` holds for all pieces or for none.
    constexpr int PIECE = 65535;
#define COLREDUCE_AS(AT, BT, CW, VEC, OUT)                                                                                                  \
    do {                                                                                                                                    \
        if constexpr (OUT == SLAB) {                                                                                                        \
            colreduce_kernel<OP, AT, BT, CW, VEC, OUT><<<dim3((unsigned)(rblocks * cblocks)), dim3(256), 0, s>>>(                           \
                (const AT*)a, as, (const BT*)b, bs, rows, rpb, o0, cols, cblocks, m, rs, o1, (int64_t)NA * cols, direct, (const AT*)y);     \
        } else {                                                                                                                            \
            for (int cb0 = 0; cb0 < cblocks; cb0 += PIECE) {                                                                                \
                const int pb = cblocks - cb0 < PIECE ? cblocks - cb0 : PIECE;                                                               \
                const int64_t p0 = (int64_t)cb0 * 64;                                                                                       \
                const int pc = (int)(cols - p0 < (int64_t)pb * 64 ? cols - p0 : (int64_t)pb * 64);                                          \
                colreduce_kernel<OP, AT, BT, CW, VEC, OUT><<<dim3((unsigned)rblocks, pb), dim3(256), 0, s>>>(                               \
                    (const AT*)a + p0, as, b ? (const BT*)b + p0 : nullptr, bs, rows, rpb, o0 + p0, pc, pb, m ? m + p0 : nullptr,           \
                    rs ? rs + p0 : nullptr, o1 ? o1 + p0 : nullptr, (int64_t)NA * cols, direct, (const AT*)y);                              \
            }                                                                                                                               \
        }                                                                                                                                   \
    } while (0)
#define COLREDUCE(BT, VEC)                                        \
    do {                                                          \
        if (ordered) COLREDUCE_AS(float, BT, 4, VEC, SLAB);       \
        else COLREDUCE_AS(float, BT, 4, VEC, ATOMIC);             \
    } while (0)
    if (adt == MST_BF16) COLREDUCE_AS(bf16_t, float, 8, true, SLAB);
    else if (adt == MST_F16) COLREDUCE_AS(f16_t, float, 8, true, SLAB);
    else if (dt == MST_F32) {
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

int colsum_b(const char* what, const float* a, int64_t as, const void* b, int dt, int64_t bs, int64_t rows, int cols, float* out, bool ordered,
             void* ws, size_t ws_bytes, hipStream_t s) {
    return colreduce_launch<OP_SUM>(what, a, MST_F32, as, b, dt, bs, nullptr, nullptr, nullptr, rows, cols, out, nullptr, ordered, ws, ws_bytes, s);
}
int colsum_b16(const char* what, const float* a, int64_t as, const void* b, int dt, int64_t bs, int64_t rows, int cols, float* out,
               bool ordered, void* ws, size_t ws_bytes, hipStream_t s) {
    MST_CHECK_ARG(dt == MST_BF16 || dt == MST_F16, "%s: dtype %d (bf16 / f16)", what, dt);
    return colsum_b(what, a, as, b, dt, bs, rows, cols, out, ordered, ws, ws_bytes, s);
}

}  // namespace

size_t colsum_ordered_workspace_bytes(int64_t rows, int cols, int outputs, int ty) {
    if (rows <= 0 || cols <= 0) return 0;
    int64_t rpb, rblocks;
    colsum_plan(rows, cols, ty, rpb, rblocks);
    return rblocks > 1 ? round256(sizeof(float) * (size_t)rblocks * outputs * cols) : 0;
}

int launch_slab_reduce(const float* slab, int64_t nrb, int64_t width, int64_t split, float* o0, float* o1, hipStream_t s) {
    MST_CHECK_ARG(nrb > 0 && width > 0 && (width + 63) / 64 < (1ll << 31), "slab_reduce: nrb=%lld width=%lld out of range", (long long)nrb,
                  (long long)width);
    slab_reduce_kernel<<<dim3((unsigned)((width + 63) / 64)), dim3(1024), 0, s>>>(slab, nrb, width, split, o0, o1);
    return mst_check_launch("slab_reduce");
}

int launch_colsum(const float* a, int64_t as, const float* b, int64_t bs, int64_t rows, int cols, float* out, hipStream_t s) {
    return colsum_b("colsum", a, as, b, MST_F32, bs, rows, cols, out, false, nullptr, 0, s);
}

int launch_colsum_ordered(const float* a, int64_t as, const float* b, int64_t bs, int64_t rows, int cols, float* out, void* ws,
                          size_t ws_bytes, hipStream_t s) {
    return colsum_b("colsum_ordered", a, as, b, MST_F32, bs, rows, cols, out, true, ws, ws_bytes, s);
}

int launch_colsum_b16(const float* a, int64_t as, const void* b, int dt, int64_t bs, int64_t rows, int cols, float* out, hipStream_t s) {
    return colsum_b16("colsum_b16", a, as, b, dt, bs, rows, cols, out, false, nullptr, 0, s);
}

int launch_colsum_b16_ordered(const float* a, int64_t as, const void* b, int dt, int64_t bs, int64_t rows, int cols, float* out, void* ws,
                              size_t ws_bytes, hipStream_t s) {
    return colsum_b16("colsum_b16_ordered", a, as, b, dt, bs, rows, cols, out, true, ws, ws_bytes, s);
}

int launch_bn_reduce(int op, const void* z, int dt, const void* y, const float* dy, const float* mean, const float* rstd, int64_t rows, int C,
                     float* out0, float* out1, bool ordered, void* ws, size_t ws_bytes, hipStream_t s) {
    if (op == COL_SUM)
        return colreduce_launch<OP_SUM>(ordered ? "colsum_ordered" : "colsum", z, dt, C, nullptr, MST_F32, 0, nullptr, nullptr, nullptr, rows, C,
                                        out0, nullptr, ordered, ws, ws_bytes, s);
    if (op == COL_SQDEV)
        return colreduce_launch<OP_SQDEV>(ordered ? "colsqdev_ordered" : "colsqdev", z, dt, C, nullptr, MST_F32, 0, mean, nullptr, nullptr, rows, C,
                                          out0, nullptr, ordered, ws, ws_bytes, s);
    return colreduce_launch<OP_BN_BWD>(ordered ? "bn_bwd_reduce_ordered" : "bn_bwd_reduce", z, dt, C, dy, MST_F32, C, mean, rstd, y, rows, C, out0,
                                       out1, ordered, ws, ws_bytes, s);
}
