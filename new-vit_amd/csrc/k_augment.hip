// Training augmentation on the device: what the reference's datasets do to a volume behind CropOrPad / ZNormalization
// (mst/data/datasets/dataset_3d_duke.py:44-47, the same lines in dataset_3d_lidc.py and dataset_3d_mrnet.py) --
//   RandomAffine(degrees=(0,0,0,0,0,90), default_pad_value='minimum'), RandomFlip((0,1,2)), the random sign inversion, RandomNoise --
// as ONE gather kernel over a batch [n, D, H, W], in that order: rotate, flip, sign, noise.  Every volume has a record of 8 floats in
// device memory (AUG_*): cos t, sin t, fill, sign, noise_std, flipD, flipH, flipW.
//
//   output voxel (d, h, w) reads the rotated volume at (d', h', w'), a flipped axis reversed (d' = D-1-d, ...);
//   the rotation is in the H-W plane about (c_h, c_w) = ((H-1)/2, (W-1)/2), the same for every slice: with y = h' - c_h, x = w' - c_w
//       s_h = c_h + cos t y - sin t x,    s_w = c_w + sin t y + cos t x
//   sampled bilinearly (h0 = floor s_h, h1 = h0 + 1, both clamped to the grid; top = v00 + fw (v01 - v00), bot likewise,
//   value = top + fh (bot - top)); inside iff -0.5 <= s_h < H-0.5 and -0.5 <= s_w < W-0.5, otherwise the value is `fill`.  A record with
//   cos t == 1 and sin t == 0 takes no sample at all: the voxel is copied, bit for bit;
//   value *= sign;  value += noise_std N(0,1) unless noise_std == 0.
//
// The normal deviates come from Philox4x32-10 (Salmon et al., SC'11) and Box-Muller: key = the 64-bit seed, counter = (g, 0, c_lo, c_hi)
// with g = (linear voxel index in its volume) / 4 and c = counter + volume index; the block's four words give the four voxels 4g .. 4g+3
// (u = ((word >> 9) + 0.5) 2^-23;  z0, z1 = sqrt(-2 ln u0) (cos, sin)(2 pi u1);  z2, z3 from u2, u3).  Nothing depends on the launch geometry.
//
// One thread per group g: four consecutive voxels (consecutive w when W % 4 == 0), one 16-byte (fp32) or 8-byte (16-bit) store.  Every
// product and sum is spelled out (fmaf / __f*_rn), so the fp32 value is the same in every instantiation and a 16-bit output is that value
// rounded once.  The gathers of a rotated slice stay in L2: a slice is at most ~1 MiB and its rows are read by neighbouring workgroups.
#include "mst_common.h"

namespace {

enum { AUG_COS = 0, AUG_SIN = 1, AUG_FILL = 2, AUG_SIGN = 3, AUG_STD = 4, AUG_FLIP_D = 5, AUG_FLIP_H = 6, AUG_FLIP_W = 7, AUG_REC = 8 };

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned r[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

__device__ __forceinline__ float unit_open(unsigned w) { return __fmul_rn((float)(w >> 9) + 0.5f, 1.0f / 8388608.0f); }   // (0, 1), exact

__device__ __forceinline__ void box_muller(unsigned wa, unsigned wb, float* z0, float* z1) {
    const float r = sqrtf(__fmul_rn(-2.0f, logf(unit_open(wa))));
    float sn, cs;
    sincospif(__fmul_rn(2.0f, unit_open(wb)), &sn, &cs);
    *z0 = __fmul_rn(r, cs);
    *z1 = __fmul_rn(r, sn);
}

template <typename T> struct Vec4;
template <> struct Vec4<float> { typedef f32x4 type; };
template <> struct Vec4<bf16_t> { typedef bf16x4 type; };
template <> struct Vec4<f16_t> { typedef f16x4 type; };

// grid (ceil(groups / 256), n).  vec_out / vec_in: DHW % 4 == 0 and the operand 4-element aligned (then whole groups only).
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void augment_kernel(const TI* __restrict__ in, TO* __restrict__ out, const float* __restrict__ params,
                                                      int D, int H, int W, int groups, unsigned seed_lo, unsigned seed_hi,
                                                      unsigned long long counter, int vec_out, int vec_in) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const int v = blockIdx.y;
    const float* p = params + (size_t)v * AUG_REC;
    const float cs = p[AUG_COS], sn = p[AUG_SIN], fill = p[AUG_FILL], sign = p[AUG_SIGN], nstd = p[AUG_STD];
    const bool fd = p[AUG_FLIP_D] != 0.f, fh = p[AUG_FLIP_H] != 0.f, fw = p[AUG_FLIP_W] != 0.f;
    const bool rot = !(cs == 1.0f && sn == 0.0f);
    const int HW = H * W, DHW = D * HW;
    const TI* vin = in + (size_t)v * DHW;
    TO* vout = out + (size_t)v * DHW;
    const int i0 = 4 * g;
    int d = i0 / HW, r = i0 - d * HW, h = r / W, w = r - h * W;
    float val[4] = {0.f, 0.f, 0.f, 0.f};

    if (!rot && vec_in && (W & 3) == 0) {
        // the four voxels share a row and sit on a 4-element boundary, also reversed (W % 4 == 0)
        const int ds = fd ? D - 1 - d : d, hs = fh ? H - 1 - h : h, ws = fw ? W - 4 - w : w;
        const typename Vec4<TI>::type t = *reinterpret_cast<const typename Vec4<TI>::type*>(vin + ((size_t)ds * H + hs) * W + ws);
#pragma unroll
        for (int e = 0; e < 4; ++e) val[e] = (float)t[fw ? 3 - e : e];
    } else {
        const float ch = 0.5f * (float)(H - 1), cw = 0.5f * (float)(W - 1);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (i0 + e < DHW) {
                const int ds = fd ? D - 1 - d : d, hs = fh ? H - 1 - h : h, ws = fw ? W - 1 - w : w;
                const TI* sl = vin + (size_t)ds * HW;
                if (!rot) {
                    val[e] = (float)sl[hs * W + ws];
                } else {
                    const float y = (float)hs - ch, x = (float)ws - cw;
                    const float sh = fmaf(cs, y, fmaf(-sn, x, ch)), sw = fmaf(sn, y, fmaf(cs, x, cw));
                    if (sh >= -0.5f && sh < (float)H - 0.5f && sw >= -0.5f && sw < (float)W - 0.5f) {
                        const float flh = floorf(sh), flw = floorf(sw);
                        const float th = __fsub_rn(sh, flh), tw = __fsub_rn(sw, flw);
                        const int h0 = (int)flh, w0 = (int)flw;
                        const int ha = min(max(h0, 0), H - 1), hb = min(max(h0 + 1, 0), H - 1);
                        const int wa = min(max(w0, 0), W - 1), wb = min(max(w0 + 1, 0), W - 1);
                        const float v00 = (float)sl[ha * W + wa], v01 = (float)sl[ha * W + wb];
                        const float v10 = (float)sl[hb * W + wa], v11 = (float)sl[hb * W + wb];
                        const float top = fmaf(tw, __fsub_rn(v01, v00), v00), bot = fmaf(tw, __fsub_rn(v11, v10), v10);
                        val[e] = fmaf(th, __fsub_rn(bot, top), top);
                    } else {
                        val[e] = fill;
                    }
                }
            }
            if (++w == W) { w = 0; if (++h == H) { h = 0; ++d; } }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) val[e] = __fmul_rn(val[e], sign);
    if (nstd != 0.f) {
        const unsigned long long c = counter + (unsigned long long)v;
        unsigned rw[4];
        philox4x32_10((unsigned)g, 0u, (unsigned)c, (unsigned)(c >> 32), seed_lo, seed_hi, rw);
        float z[4];
        box_muller(rw[0], rw[1], &z[0], &z[1]);
        box_muller(rw[2], rw[3], &z[2], &z[3]);
#pragma unroll
        for (int e = 0; e < 4; ++e) val[e] = fmaf(nstd, z[e], val[e]);
    }
    if (vec_out) {
        typename Vec4<TO>::type t;
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = (TO)f32_rounded(val[e]);
        *reinterpret_cast<typename Vec4<TO>::type*>(vout + i0) = t;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i0 + e < DHW) vout[i0 + e] = (TO)f32_rounded(val[e]);
    }
}

// ---- per-volume minimum: the 'minimum' fill.  min is order-independent, so integer atomics on the bit pattern (atomic_min_f32,
// mst_common.h: branched on the sign bit, so that a workgroup whose minimum is -0.0 cannot displace a negative one) give the same bits
// whatever the arrival order (no floating-point atomic anywhere) ---------------------------------------------------------------------------
__global__ void min_init_kernel(float* out, int n, int stride) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) out[(size_t)v * stride] = INFINITY;
}

// grid (blocks, n): each workgroup strides over its volume
template <typename T>
__global__ __launch_bounds__(256) void volume_min_kernel(const T* __restrict__ x, int64_t elems, float* out, int stride, int vec) {
    __shared__ float red[4];
    const T* vx = x + (size_t)blockIdx.y * elems;
    float m = INFINITY;
    if (vec) {
        const int64_t n8 = elems / 8;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
            float t[8];
            load8(vx + i * 8, t);
#pragma unroll
            for (int e = 0; e < 8; ++e) m = fminf(m, t[e]);
        }
        for (int64_t i = n8 * 8 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < elems; i += (int64_t)gridDim.x * 256) m = fminf(m, (float)vx[i]);
    } else {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < elems; i += (int64_t)gridDim.x * 256) m = fminf(m, (float)vx[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomic_min_f32(out + (size_t)blockIdx.y * stride, fminf(fminf(red[0], red[1]), fminf(red[2], red[3])));
}

template <typename TI>
int launch_augment_out(const TI* in, void* out, int odt, int n, int D, int H, int W, const float* params, uint64_t seed, uint64_t counter,
                       hipStream_t s) {
    const int64_t dhw = (int64_t)D * H * W;
    const int groups = (int)((dhw + 3) / 4);
    const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)n), block(256);
    const int osz = odt == MST_F32 ? 4 : 2;
    const int vec_out = (dhw % 4 == 0) && aligned(out, 4 * osz), vec_in = (dhw % 4 == 0) && aligned(in, 4 * sizeof(TI));
    const unsigned lo = (unsigned)seed, hi = (unsigned)(seed >> 32);
    if (odt == MST_F32) augment_kernel<TI, float><<<grid, block, 0, s>>>(in, (float*)out, params, D, H, W, groups, lo, hi, counter, vec_out, vec_in);
    else if (odt == MST_F16) augment_kernel<TI, f16_t><<<grid, block, 0, s>>>(in, (f16_t*)out, params, D, H, W, groups, lo, hi, counter, vec_out, vec_in);
    else augment_kernel<TI, bf16_t><<<grid, block, 0, s>>>(in, (bf16_t*)out, params, D, H, W, groups, lo, hi, counter, vec_out, vec_in);
    return mst_check_launch("augment_volumes");
}

}  // namespace

int launch_augment_volumes(const void* in, int idt, void* out, int odt, int n, int D, int H, int W, const float* params, uint64_t seed,
                           uint64_t counter, hipStream_t s) {
    if (idt == MST_F32) return launch_augment_out((const float*)in, out, odt, n, D, H, W, params, seed, counter, s);
    if (idt == MST_F16) return launch_augment_out((const f16_t*)in, out, odt, n, D, H, W, params, seed, counter, s);
    return launch_augment_out((const bf16_t*)in, out, odt, n, D, H, W, params, seed, counter, s);
}

int launch_volume_min(const void* x, int dt, int n, int64_t elems, float* out, int stride, hipStream_t s) {
    min_init_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(out, n, stride);
    const int64_t per = (elems + 2047) / 2048;                        // 8 elements per thread and trip
    const dim3 grid((unsigned)(per < 1 ? 1 : (per > 1024 ? 1024 : per)), (unsigned)n), block(256);
    const int esz = dt == MST_F32 ? 4 : 2;
    const int vec = aligned(x, 16) && (elems * esz) % 16 == 0;      // every volume starts on a 16-byte boundary
    if (dt == MST_F32) volume_min_kernel<float><<<grid, block, 0, s>>>((const float*)x, elems, out, stride, vec);
    else if (dt == MST_F16) volume_min_kernel<f16_t><<<grid, block, 0, s>>>((const f16_t*)x, elems, out, stride, vec);
    else volume_min_kernel<bf16_t><<<grid, block, 0, s>>>((const bf16_t*)x, elems, out, stride, vec);
    return mst_check_launch("volume_min");
}
