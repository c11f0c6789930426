// Row kernels of the training step's 16-bit storage mode (mst/train.py, train_storage='16bit'): what the reference's autocast does to the
// tensors a block keeps for its backward (Trainer(precision='16-mixed'), scripts/main_train.py:110-123; block.py:89-114) -- the LayerNorm
// outputs, the attention output, the branch outputs and the MLP's hidden activations live in the 16-bit type T, the residual stream and
// every gradient stay fp32.  All of these are bandwidth kernels: every byte moves once, in 16-byte accesses (4 fp32 or 8 T per lane).
//   residual_layernorm16   x_out = x_in + gamma o float(br_T)  (fp32, one rounding),  y_T = LayerNorm(x_out)     one wave per row
//   transpose16            T [rows, cols] -> T [cols, rows_pad], zero columns past rows: the 16-bit-input twin of cvt16's transposed form
// The mode's other entry points are instantiations of templates that also serve fp32: act_fwd16 / act_bwd16 / swiglu_fwd16 / swiglu_bwd16
// in k_train.hip, colsum_b16 (+ ordered) in k_colsum.hip.
#include "mst_common.h"

namespace {

// One wave per row, four rows per workgroup (the layout of layernorm_kernel); lane l owns columns 512 j + 8 l .. + 7.  Statistics as there:
// mean, then the variance of the centred values, by wave shuffles.  Contiguous rows of `cols` (a multiple of 8) elements.
template <int NJ, typename T>
__global__ __launch_bounds__(256) void residual_layernorm16_kernel(const float* __restrict__ xin, const T* __restrict__ br,
                                                                   const float* __restrict__ gamma, float* __restrict__ xout,
                                                                   const float* __restrict__ w, const float* __restrict__ b, T* __restrict__ y,
                                                                   int64_t rows, int cols, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t off = row * cols;
    float v[NJ][8];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = j * 512 + lane * 8;
        if (c < cols) {
            float r[8], g[8];
            load8(xin + off + c, v[j]);
            load8(br + off + c, r);
            if (gamma) load8(gamma + c, g);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                v[j][e] = gamma ? fmaf(g[e], r[e], v[j][e]) : v[j][e] + r[e];
                s += v[j][e];
            }
            store8(xout + off + c, v[j]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[j][e] = 0.f;
        }
    }
    if (!y) return;
    const float inv_n = 1.0f / (float)cols;
    const float mean = wave_sum(s) * inv_n;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (j * 512 + lane * 8 < cols) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = v[j][e] - mean;
                q = fmaf(d, d, q);
            }
        }
    }
    const float rstd = rsqrtf(wave_sum(q) * inv_n + eps);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = j * 512 + lane * 8;
        if (c < cols) {
            float ww[8], bb[8], o[8];
            load8(w + c, ww);
            load8(b + c, bb);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (v[j][e] - mean) * rstd * ww[e] + bb[e];
            store8(y + off + c, o);
        }
    }
}

// out[c][r] = x[r][c] (r < rows), 0 (rows <= r < rows_pad): 64 x 64 tiles through LDS, 128-byte row segments in and out
template <typename T>
__global__ __launch_bounds__(256) void transpose16_kernel(const T* __restrict__ x, int64_t ldx, int64_t rows, int cols, T* __restrict__ out,
                                                          int64_t ldo, int64_t rows_pad) {
    __shared__ T tile[64][64 + 2];
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    const int c0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int rr = ty + 4 * i;
        const int64_t r = r0 + rr;
        tile[rr][tx] = (r < rows && c0 + tx < cols) ? x[r * ldx + c0 + tx] : (T)0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int cc = ty + 4 * i;
        const int64_t r = r0 + tx;
        if (c0 + cc < cols && r < rows_pad) out[(int64_t)(c0 + cc) * ldo + r] = tile[tx][cc];
    }
}

template <typename T>
int residual_ln16_t(const float* xin, const void* br, const float* gamma, float* xout, const float* w, const float* b, void* y, int64_t rows,
                    int cols, float eps, hipStream_t s) {
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    const T* r = (const T*)br;
    T* o = (T*)y;
    if (cols <= 512) residual_layernorm16_kernel<1, T><<<grid, block, 0, s>>>(xin, r, gamma, xout, w, b, o, rows, cols, eps);
    else if (cols <= 1024) residual_layernorm16_kernel<2, T><<<grid, block, 0, s>>>(xin, r, gamma, xout, w, b, o, rows, cols, eps);
    else residual_layernorm16_kernel<4, T><<<grid, block, 0, s>>>(xin, r, gamma, xout, w, b, o, rows, cols, eps);
    return mst_check_launch("residual_layernorm16");
}

}  // namespace

int launch_residual_layernorm16(const float* xin, const void* br, int dt, const float* gamma, float* xout, const float* w, const float* b,
                                void* y, int64_t rows, int cols, float eps, hipStream_t s) {
    MST_CHECK_ARG(dt == MST_BF16 || dt == MST_F16, "residual_layernorm16: dtype %d (bf16 / f16)", dt);
    MST_CHECK_ARG(cols > 0 && cols <= 2048 && cols % 8 == 0, "residual_layernorm16: cols=%d must be a multiple of 8 and <= 2048", cols);
    MST_CHECK_ARG(rows > 0 && (rows + 3) / 4 < (1ll << 31), "residual_layernorm16: rows=%lld out of range", (long long)rows);
    MST_CHECK_ARG(aligned(xin, 16) && aligned(br, 16) && aligned(xout, 16) && aligned(gamma, 16) && aligned(w, 16) && aligned(b, 16) && aligned(y, 16),
                  "residual_layernorm16: bases must be 16-byte aligned");
    if (dt == MST_BF16) return residual_ln16_t<bf16_t>(xin, br, gamma, xout, w, b, y, rows, cols, eps, s);
    return residual_ln16_t<f16_t>(xin, br, gamma, xout, w, b, y, rows, cols, eps, s);
}

int launch_transpose16(const void* x, int dt, int64_t ldx, int64_t rows, int cols, void* out, int64_t ldo, int64_t rows_pad, hipStream_t s) {
    MST_CHECK_ARG(x && out && rows > 0 && cols > 0 && ldx >= cols, "transpose16: bad arguments");
    MST_CHECK_ARG(dt == MST_BF16 || dt == MST_F16, "transpose16: dtype %d (bf16 / f16)", dt);
    MST_CHECK_ARG(rows_pad >= rows && ldo >= rows_pad, "transpose16: rows_pad=%lld ldo=%lld", (long long)rows_pad, (long long)ldo);
    const dim3 grid((unsigned)((rows_pad + 63) / 64), (cols + 63) / 64);
    MST_CHECK_ARG((rows_pad + 63) / 64 < (1ll << 31) && grid.y <= 65535, "transpose16: rows_pad=%lld cols=%d out of range", (long long)rows_pad, cols);
    if (dt == MST_BF16) transpose16_kernel<bf16_t><<<grid, dim3(256), 0, s>>>((const bf16_t*)x, ldx, rows, cols, (bf16_t*)out, ldo, rows_pad);
    else transpose16_kernel<f16_t><<<grid, dim3(256), 0, s>>>((const f16_t*)x, ldx, rows, cols, (f16_t*)out, ldo, rows_pad);
    return mst_check_launch("transpose16");
}
