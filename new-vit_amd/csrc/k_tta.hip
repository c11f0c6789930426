// Folded test-time augmentation of scripts/main_predict.py:147-158 (`--use_tta`: the identity and the seven flips of a volume).
// The encoder works per slice, so a flip along D only permutes slice embeddings: the eight variants need the slices of FOUR in-plane
// flips (identity, H, W, HW), made here in one pass over the input, and their saliency is summed in one launch in the script's order.
#include "mst_common.h"

namespace {

using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;

// One row of W elements between global memory and the row image in LDS.  A row starts wherever n, H and W put it, so the 16-byte
// vectors start at the first aligned element of the GLOBAL row and the few elements before and behind them go one by one.
template <typename E>
__device__ __forceinline__ int row_head(const E* g, int W) {
    const int h = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(g) & 15u)) & 15u) / sizeof(E));
    return h < W ? h : W;
}

template <typename E>
__device__ __forceinline__ void row_load(const E* __restrict__ src, E* lds, int W) {
    constexpr int V = 16 / sizeof(E);
    const int head = row_head(src, W), nvec = (W - head) / V;
    for (int v = threadIdx.x; v < nvec; v += blockDim.x) {
        const u32x4 q = *reinterpret_cast<const u32x4*>(src + head + v * V);
        E e[V];
        __builtin_memcpy(e, &q, 16);
#pragma unroll
        for (int k = 0; k < V; ++k) lds[head + v * V + k] = e[k];
    }
    const int rest = W - nvec * V;                       // head elements, then the tail behind the vectors
    for (int t = threadIdx.x; t < rest; t += blockDim.x) {
        const int j = t < head ? t : nvec * V + t;
        lds[j] = src[j];
    }
}

// dst[j] = lds[j], or lds[W-1-j] when `mirror`: the reversal happens on the LDS side, every global store is contiguous
template <typename E>
__device__ __forceinline__ void row_store(E* __restrict__ dst, const E* lds, int W, bool mirror) {
    constexpr int V = 16 / sizeof(E);
    const int head = row_head(dst, W), nvec = (W - head) / V;
    for (int v = threadIdx.x; v < nvec; v += blockDim.x) {
        const int j0 = head + v * V;
        E e[V];
#pragma unroll
        for (int k = 0; k < V; ++k) e[k] = lds[mirror ? W - 1 - (j0 + k) : j0 + k];
        u32x4 q;
        __builtin_memcpy(&q, e, 16);
        *reinterpret_cast<u32x4*>(dst + j0) = q;
    }
    const int rest = W - nvec * V;
    for (int t = threadIdx.x; t < rest; t += blockDim.x) {
        const int j = t < head ? t : nvec * V + t;
        dst[j] = lds[mirror ? W - 1 - j : j];
    }
}

// out[0] = x, out[1] = x mirrored along H, out[2] = along W, out[3] = along both; x [n, H, W].  One workgroup per input row:
// read once into LDS, written four times.  E carries the bits only (uint16_t for fp16 / bf16, uint32_t for fp32).
template <typename E>
__global__ __launch_bounds__(256) void tta_inplane_flips_kernel(const E* __restrict__ x, int H, int W, int64_t elems,
                                                                E* __restrict__ out) {
    extern __shared__ u32x4 tta_row_raw[];
    E* row = reinterpret_cast<E*>(tta_row_raw);
    const int64_t r = blockIdx.x;                        // row of x: slice r / H, line r % H
    const int y = (int)(r % H);
    const int64_t at = r * W, mirrored = (r - y + (H - 1 - y)) * W;
    row_load(x + at, row, W);
    __syncthreads();
    row_store(out + at, row, W, false);
    row_store(out + elems + mirrored, row, W, false);
    row_store(out + 2 * elems + at, row, W, true);
    row_store(out + 3 * elems + mirrored, row, W, true);
}

// The eight variants in the script's order (), (2,), (3,), (4,), (2,3), (2,4), (3,4), (2,3,4) as flip masks (bit 0 depth, bit 1
// height, bit 2 width, as mst_saliency_accumulate counts them): the in-plane flip is mask >> 1, the depth flip mask & 1.
__device__ constexpr int tta_mask(int v) { return v == 3 ? 4 : v == 4 ? 3 : v; }

// low[d][y][x] = sum_v headmean(plane[f_v][d])[y_f][x_f] * sa[v][r_v ? D-1-d : d],  ws[d] = sum_v sa[v][r_v ? D-1-d : d]: a variant
// that was flipped along D saw slice d at position D-1-d, with the plane attention of slice d itself (the encoder is per slice).
// Every output element is one thread's sum over v = 0..7 in that order: no atomics, the same bits at every launch.
__global__ void saliency_accumulate_tta_kernel(const float* __restrict__ plane, const float* __restrict__ sa, int D, int heads,
                                               int gh, int gw, int Np, float* __restrict__ low, float* __restrict__ slice_acc) {
    const int d = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float w[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) w[v] = sa[(int64_t)v * D + ((tta_mask(v) & 1) ? D - 1 - d : d)];
    if (i == 0 && slice_acc) {
        float s = 0.f;
#pragma unroll
        for (int v = 0; v < 8; ++v) s += w[v];
        slice_acc[d] = s;
    }
    if (i >= gh * gw) return;
    const int y = i / gw, x = i - y * gw;
    float m[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const int yy = (f & 1) ? gh - 1 - y : y, xx = (f & 2) ? gw - 1 - x : x;
        const float* p = plane + (((int64_t)f * D + d) * heads) * Np + yy * gw + xx;
        float s = 0.f;
        for (int h = 0; h < heads; ++h) s += p[(int64_t)h * Np];
        m[f] = s / (float)heads;                         // weight.mean(dim=1)   main_predict.py:76
    }
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < 8; ++v) s += m[tta_mask(v) >> 1] * w[v];
    low[((int64_t)d * gh + y) * gw + x] = s;
}

template <typename E>
int flips_launch(const void* x, int64_t rows, int H, int W, void* out, hipStream_t s) {
    tta_inplane_flips_kernel<E><<<dim3((unsigned)rows), dim3(256), (size_t)W * sizeof(E), s>>>(
        static_cast<const E*>(x), H, W, rows * W, static_cast<E*>(out));
    return mst_check_launch("tta_inplane_flips");
}

}  // namespace

int launch_tta_inplane_flips(const void* x, int dt, int n, int H, int W, void* out, hipStream_t s) {
    const int64_t rows = (int64_t)n * H;
    const size_t esize = dt == MST_F32 ? 4 : 2;
    MST_CHECK_ARG(rows <= 0x7fffffff, "tta_inplane_flips: %d x %d rows do not fit the launch grid", n, H);
    MST_CHECK_ARG((size_t)W * esize <= 64 * 1024, "tta_inplane_flips: a row of %d elements does not fit LDS", W);
    return dt == MST_F32 ? flips_launch<uint32_t>(x, rows, H, W, out, s) : flips_launch<uint16_t>(x, rows, H, W, out, s);
}

int launch_saliency_accumulate_tta(const float* plane, const float* slice_attn, int D, int heads, int gh, int gw, int Np,
                                   float* low, float* slice_acc, hipStream_t s) {
    MST_CHECK_ARG(D <= 65535, "saliency_accumulate_tta: %d slices do not fit the launch grid", D);
    saliency_accumulate_tta_kernel<<<dim3((gh * gw + 255) / 256, D), dim3(256), 0, s>>>(plane, slice_attn, D, heads, gh, gw, Np,
                                                                                        low, slice_acc);
    return mst_check_launch("saliency_accumulate_tta");
}
