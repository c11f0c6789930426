/*
 * mst_hip.h -- C ABI of libmst_hip.so: the MI355X (gfx950) kernels behind the Medical Slice
 * Transformer hot path  DinoV2ClassifierSlice.forward  (+ its save_attn read-outs).
 *
 * The reference (gabrielfnayres/new-vit) has no FFI: the path sits behind a Python class
 * (mst/models/dino.py:32-275).  This header is the boundary the build introduces underneath that
 * class: plain device pointers, sizes and a hipStream_t; no torch types; no
 * allocation inside (the caller passes a workspace); every call is asynchronous on `stream` and
 * re-entrant for distinct streams; status codes instead of exceptions (0 = ok, message via
 * mst_last_error()).  Each entry point cites the reference lines whose arithmetic it replaces
 * (paths relative to the reference root).  The reference-side binding is in INTEGRATION.md.
 *
 * Layouts: all matrices row-major.  "compute dtype" T is MST_F16 or MST_BF16 (MFMA operands,
 * fp32 accumulate) or MST_F32 (exact fp32 MFMA).  The residual stream, LayerNorm statistics,
 * softmax and every bias/affine parameter are fp32 in all modes.
 */
#ifndef MST_HIP_H
#define MST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mst_stream_t; /* hipStream_t */

enum mst_dtype { MST_F32 = 0, MST_F16 = 1, MST_BF16 = 2, MST_F8E4M3 = 3 /* OCP e4m3 bytes: fp8 entry points only */ };

enum mst_status {
    MST_OK = 0,
    MST_EINVAL = 1,     /* bad argument / unsupported shape */
    MST_EWORKSPACE = 2, /* workspace too small */
    MST_ELAUNCH = 3     /* HIP launch error */
};

enum mst_epilogue {
    MST_EPI_BIAS = 0,      /* C = A W^T + b                               (any linear)            */
    MST_EPI_BIAS_GELU = 1, /* C = gelu_erf(A W^T + b)                     mlp.py:34-36            */
    MST_EPI_BIAS_RELU = 2, /* C = relu(A W^T + b)                         transformer_blocks.py:586 */
    MST_EPI_RESIDUAL = 3,  /* C(f32) += gamma * (A W^T + b)               block.py:90-94,112-113  */
    MST_EPI_RESIDUAL_RELU = 4, /* C = relu(C + gamma * (A W^T + b))        resnet BasicBlock / Bottleneck exit.  Per entry point: mst_gemm
                                * (fp32 operands) and mst_conv_gemm take an fp32 C; mst_conv_gemm16 takes a 16-bit C in place (no gamma);
                                * mst_gemm with 16-bit operands refuses it */
    MST_EPI_BIAS_SWIGLU = 5   /* C[M, N/2] = silu(A Wg^T + bg) o (A Wv^T + bv)   swiglu_ffn.py:54-72; W is the row-paired image, see mst_gemm */
};

enum mst_ffn_kind { MST_FFN_MLP = 0, MST_FFN_SWIGLU = 1 };   /* mst_vit_weights.ffn_kind */

enum mst_fusion_type { MST_FUSION_TRANSFORMER = 0, MST_FUSION_LINEAR = 1, MST_FUSION_AVERAGE = 2 };

/* Library ---------------------------------------------------------------------------------- */
int mst_version(void);            /* 100 = round 1; 200 = round 2: mst_vit_layer.proj_pack/proj_bf, mst_fusion_weights.head_in,
                                   * mst_vit_weights.profiler / prune_last_block appended; 300 = round 3: mst_vit_layer.block_seq
                                   * inserted, mst_block_fused_s; the ctypes mirror checks it */
const char* mst_last_error(void); /* thread-local message of the last failing call */

/* Per-op entry points (unit parity; also what mst_vit_encode / mst_slice_fusion launch) ----- */

/* nn.LayerNorm over the last dim: block.py:63,75; vision_transformer.py:165,263 (eps 1e-6);
 * transformer_blocks.py:499-500, dino.py:95 (eps 1e-5).  x fp32 [rows, cols] with row stride
 * x_stride (elements); out dtype f32/f16/bf16 with row stride out_stride.  cols even, <= 2048.
 * gamma == beta == NULL: normalise only (the affine is folded into the consumer's weights). */
int mst_layernorm(const float* x, int64_t x_stride, const float* gamma, const float* beta,
                  void* out, int out_dtype, int64_t out_stride, int64_t rows, int cols, float eps,
                  mst_stream_t stream);

/* nn.Linear / F.linear with fused epilogue: attention.py:58,67; mlp.py:35,38;
 * transformer_blocks.py:166,283,586; dino.py:135,166.
 * C[M,N] = epi(A[M,K] . W[N,K]^T + bias[N]).  A and W share one dtype.
 *   16-bit A/W: MFMA 16x16x32 path; needs K % 64 == 0, N % 128 == 0, 16-byte aligned rows.
 *   f32   A/W: exact fp32 MFMA path; needs K % 16 == 0; any M, N.
 * c_dtype: f32 or (16-bit A only) the A dtype; MST_EPI_RESIDUAL needs c_dtype f32 (C is read and
 * written, gamma = LayerScale vector or NULL: layer_scale.py:26-27).
 * Columns n < scale_cols are multiplied by col_scale after the bias (q * head_dim^-0.5 of
 * attention.py:60 folded into the QKV projection); pass scale_cols = 0 for none.
 *
 * MST_EPI_BIAS_SWIGLU (SwiGLUFFNFused, extern/dinov2/layers/swiglu_ffn.py:54-72: x1, x2 = w12(x).chunk(2); hidden = silu(x1) * x2):
 * gate and value of an output element are combined in the accumulators, so the [M, 2H] pre-activation never reaches memory.  W [N, K]
 * and bias [N] are the ROW-PAIRED image of w12 [2H, K] / its bias with pairing group G (what hip.pack_swiglu builds; H is first padded
 * with zero rows to Hp, a multiple of 64, and N = 2 Hp):
 *     image rows 2G g     .. 2G g + G - 1   = w12 rows       G g .. G g + G - 1    (gate)
 *     image rows 2G g + G .. 2G g + 2G - 1  = w12 rows  Hp + G g .. Hp + G g + G - 1  (value)          for g < Hp / G
 * G is part of this contract and depends on the operand type: G = 16 for 16-bit operands (N % 128 == 0, K % 64 == 0), G = 32 for f32
 * operands (N % 128 == 0, K % 16 == 0).  C is [M, N / 2] with row stride ldc >= N / 2 (ldc % 4 == 0); A, W, C and bias 16-byte aligned;
 * gamma NULL and scale_cols 0.  An N that is not a multiple of 128 (whole tiles of paired groups) returns MST_EINVAL.  The sigmoid runs in fp32:
 * x / (1 + expf(-x)) for f32 C, one v_exp + one v_rcp for 16-bit C; a large negative gate gives -0, never NaN. */
int mst_gemm(const void* A, int ab_dtype, int64_t lda, const void* W, int64_t ldw, const float* bias,
             void* C, int c_dtype, int64_t ldc, int64_t M, int N, int K, int epilogue,
             const float* gamma, float col_scale, int scale_cols, mst_stream_t stream);

/* FP8 linear layers (BASELINE.json configs[4]): OCP e4m3 operands, one scale per tensor from its
 * absolute maximum, fp32 accumulate.  The reference has no fp8 code; this is F.linear (attention.py:58,67; mlp.py:35,38)
 * with both operands rounded to e4m3:  y = (sa*sw) * (q(x/sa) . q(W/sw)^T) + b,  sa = max|x|/448,  sw = max|W|/448.
 *
 * mst_quantize_fp8: x (bf16/fp16, n elements, n % 8 == 0) -> out8[n] e4m3 bytes = rne(x * 448/amax), where *amax (device
 *   fp32) = max(*amax on entry, max|x|): pass 0 for a fresh per-tensor scale, or a calibrated floor.  Stream-ordered, no
 *   host synchronisation.
 * mst_gemm_fp8: C[M,N] = epi((*a_amax/448 * w_scale) * A8[M,K] . W8[N,K]^T + bias); A8, W8 e4m3 bytes with K-contiguous
 *   rows; K % 128 == 0, N % 128 == 0, lda/ldw % 16 == 0; c_dtype f32 / bf16 / fp16; epilogues, gamma, col_scale and
 *   scale_cols as mst_gemm.  c_dtype MST_F8E4M3 (non-residual epilogues): C is written as e4m3 bytes rne(clamp(v * 448 /
 *   *c_amax)) under the caller's scale c_amax (device fp32; calibrated: nothing is scanned); c_amax is ignored otherwise.
 * mst_layernorm_fp8: mst_layernorm writing e4m3 bytes under a calibrated scale: out8 = rne(clamp(LN(x) * 448 / *amax)). */
int mst_quantize_fp8(const void* x, int dtype, int64_t n, float* amax, void* out8, mst_stream_t stream);
int mst_gemm_fp8(const void* A8, int64_t lda, const void* W8, int64_t ldw, const float* bias, const float* a_amax,
                 float w_scale, void* C, int c_dtype, int64_t ldc, int64_t M, int N, int K, int epilogue,
                 const float* gamma, float col_scale, int scale_cols, const float* c_amax, mst_stream_t stream);
int mst_layernorm_fp8(const float* x, int64_t x_stride, const float* gamma, const float* beta, void* out8,
                      int64_t out_stride, int64_t rows, int cols, float eps, const float* amax, mst_stream_t stream);

/* softmax(q k^T) v per (sequence, head), q pre-scaled: attention.py:56-66 (== xformers
 * memory_efficient_attention, attention.py:84).  qkv [n_seq*N, 3*heads*head_dim] packed as the
 * reference's fused projection lays it out (q | k | v, head-major inside each); out
 * [n_seq*N, heads*head_dim].  16-bit dtypes: head_dim == 64 (flash-style, never materialises
 * [N,N]); f32: head_dim == 64. */
int mst_attention(const void* qkv, int dtype, int n_seq, int N, int heads, int head_dim, void* out,
                  mst_stream_t stream);

/* Row 0 (CLS query) of the softmax, all heads: what dino.py:226-243 stores and
 * dino.py:190-192 consumes.  probs fp32 [n_seq, heads, N]. */
int mst_attention_cls_probs(const void* qkv, int dtype, int n_seq, int N, int heads, int head_dim,
                            float* probs, mst_stream_t stream);

/* The full softmax matrix (dino.py:232-241 `attention_maps` entry): probs fp32
 * [n_seq, heads, N, N].  API parity for get_attention_cls (dino.py:204-212); O(N^2) memory. */
int mst_attention_probs_full(const void* qkv, int dtype, int n_seq, int N, int heads, int head_dim,
                             float* probs, mst_stream_t stream);

/* The kernels and kernel modes that only mst_vit_encode's fused 16-bit pipeline launches, callable on their own (each entry forwards
 * to the launcher the encoder uses; additive, the ABI version does not change).
 * mst_attention_ex: mst_attention for the 16-bit dtypes (head_dim 64; anything else returns MST_EINVAL) with the encoder's two options,
 *   a combination of mst_attention_flags.  MST_ATTN_LOG2Q: q carries head_dim^-0.5 * log2(e) already (one rounding of q, as the
 *   encoder's QKV epilogue writes it), the kernel takes exp2 of q.k as stored.  MST_ATTN_OUT_BLOCKED: out is written in the 16-bit
 *   "blocked" layout (mst_block_fused_s below) with heads*64 columns; allocate whole 32-row groups, ceil(n_seq*N / 32) * 32 rows --
 *   only rows < n_seq*N are written.
 * mst_attention_cls: the CLS query's attention output alone, out [n_seq, heads*64] in qkv's type (f32 / f16 / bf16, head_dim 64,
 *   N <= 12000, n_seq <= 65535), and its probabilities fp32 [n_seq, heads, N] where probs is not NULL: what the last block needs under
 *   mst_vit_weights.prune_last_block.  log2q as MST_ATTN_LOG2Q.
 * mst_gemm16_blocked: the QKV projection on blocked rows.  C[M, N] = (A . W^T + bias) * (col < scale_cols ? col_scale : 1) with K = 384,
 *   A_blocked the rows in the 16-bit blocked layout with 384 columns (whole 32-row groups allocated; rows past M are read, never
 *   stored), W [N, 384] with row stride ldw, C row-major in the operand type.  Only the weights-in-registers kernel reads blocked rows:
 *   a shape it does not take (N not a multiple of 384 or more 384-column tiles than an XCD has CUs, scale_cols not a multiple of 384
 *   below N, M below 8192 rows, ldw / ldc not multiples of 8, a pointer not 16-byte aligned) returns MST_EINVAL.
 * mst_patch_rows16: mst_patch_embed for E = 384 that also writes xn = (x - mean) * rstd (eps 1e-6, no affine) of every token row in
 *   the 16-bit compute dtype: x fp32 [n, n_prefix+Np, 384], xn the same rows in `dtype` (MST_BF16 / MST_F16); arguments as
 *   mst_patch_embed. */
enum mst_attention_flags {
    MST_ATTN_LOG2Q = 1,
    MST_ATTN_OUT_BLOCKED = 2
};
int mst_attention_ex(const void* qkv, int dtype, int n_seq, int N, int heads, int head_dim, void* out, int flags,
                     mst_stream_t stream);
int mst_attention_cls(const void* qkv, int dtype, int n_seq, int N, int heads, void* out, float* probs, int log2q,
                      mst_stream_t stream);
int mst_gemm16_blocked(const void* A_blocked, int dtype, const void* W, int64_t ldw, const float* bias, void* C, int64_t ldc,
                       int64_t M, int N, float col_scale, int scale_cols, mst_stream_t stream);
int mst_patch_rows16(const void* vol, int in_dtype, int n, int H, int W, const void* wp, int dtype, const float* bias,
                     const float* prefix, int n_prefix, const float* pos_patch, float* x, void* xn, mst_stream_t stream);

/* Memory-efficient attention for the mixed-precision TRAINING step (FlashAttention-2 form): no [N, N] tensor in the forward or the
 * backward.  Per-slice encoder blocks only: head_dim == 64, no key mask, any N >= 1.
 *   qkv16  [n_seq*N, 3*heads*64], dtype MST_BF16 or MST_F16: q | k | v head-major, as mst_attention; q carries head_dim^-0.5
 *          already (the QKV projection's epilogue), so the scores are q.k with no further scale.
 * mst_attention_train_fwd: out fp32 [n_seq*N, heads*64] = softmax(q k^T) v (fp32 softmax and accumulation, exact running row
 *   maximum); lse fp32 [n_seq, heads, N] = ln sum_j exp(q_i . k_j) in NATURAL-log units, the sum `out` is normalised by.
 * mst_attention_train_bwd: from the forward's qkv16, out, lse and dout fp32 [n_seq*N, heads*64] (the gradient of out), writes every
 *   element of dqkv fp32 [n_seq*N, 3*heads*64] (laid out like qkv16): dK and dV are the gradients of the stored k and v, dQ that of
 *   the stored q times dq_scale (pass the epilogue's factor, 0.125, for the gradient of the un-scaled projection output).
 *   workspace: device memory of at least mst_attention_train_bwd_workspace_bytes(n_seq, N, heads, 64) bytes (a 16-bit image of dout
 *   and the row sums D = rowsum(dout o out)).  Deterministic (no atomics): identical calls return identical bits.
 *   The envelope of dout.  Each (sequence, head) is scaled on its own by a power of two c = 2^min(6 - e, 126), with max |dout| in
 *   [2^(e-1), 2^e) over that head's N x 64 block, and the results are multiplied by 1 / c: the gradients are homogeneous in powers of
 *   two, bit for bit, and a head does not see its neighbours' magnitudes.
 *     - max |dout| from 2^-121 (3.8e-37) to 3e38: c max |dout| in [32, 64), the same relative accuracy at every magnitude, as long as
 *       the gradients themselves stay normal fp32 numbers.
 *     - below 2^-121, denormals included: c = 2^126 (c and 1 / c stay finite normal numbers).  The gradients are finite; they are fp32
 *       denormals and D = c rowsum(dout o out) is formed from denormal products, so they lose accuracy gradually with the magnitude
 *       and reach zero where fp32 ends (about 1e-45).  tests/test_attn_train_range_gpu.py holds heads at 2^-124 and at 1e-40 to the
 *       same kind of bar as every other head.
 *     - a head that is all zero returns exact zeros; a head that holds an inf or a NaN (or exceeds 3e38) returns unspecified values
 *       in ITS dQ, dK, dV and leaves every other (sequence, head) untouched, bit for bit.
 *     - fp16 headroom of dS: the 16-bit MFMA operand dS = P o (c dP - c D), dP = dout v^T, carries c max |dout| < 64, so in fp16 (largest
 *       number 65504) it overflows when P |dP - D| / max |dout| exceeds about 1000 for some (query, key) -- v and dout large and
 *       aligned along one direction with a probability near 1 beside it.  Tested with |dP - D| / max |dout| beyond 1000 and dS up to
 *       2^13 (a ratio of 190); the training step is orders of magnitude inside.  bf16 has fp32's range and no such limit.
 * Unsupported arguments (head_dim != 64, a dtype other than bf16 / fp16, N < 1, a short workspace) return MST_EINVAL. */
size_t mst_attention_train_bwd_workspace_bytes(int n_seq, int N, int heads, int head_dim);
int mst_attention_train_fwd(const void* qkv16, int dtype, int n_seq, int N, int heads, int head_dim, float* out, float* lse,
                            mst_stream_t stream);
int mst_attention_train_bwd(const void* qkv16, int dtype, const float* out, const float* dout, const float* lse, int n_seq, int N,
                            int heads, int head_dim, float dq_scale, float* dqkv, void* workspace, size_t workspace_bytes,
                            mst_stream_t stream);
/* The same pair with `out` in qkv16's own 16-bit type (train_storage='16bit': the reference's autocast keeps the attention output in
 * 16 bits, attention.py:56-66 under main_train.py:110-123).  mst_attention_train_fwd16: the same kernel, the normalised fp32 output
 * rounded to nearest even in the epilogue -- out16 [n_seq*N, heads*64] holds the bits of T(out of mst_attention_train_fwd), lse is
 * identical.  mst_attention_train_bwd16: D = rowsum(dout o float(out16)); everything else as mst_attention_train_bwd (same workspace
 * size, same argument rules, same determinism). */
int mst_attention_train_fwd16(const void* qkv16, int dtype, int n_seq, int N, int heads, int head_dim, void* out16, float* lse,
                              mst_stream_t stream);
int mst_attention_train_bwd16(const void* qkv16, int dtype, const void* out16, const float* dout, const float* lse, int n_seq, int N,
                              int heads, int head_dim, float dq_scale, float* dqkv, void* workspace, size_t workspace_bytes,
                              mst_stream_t stream);

/* Bicubic resampling of the patch position grid: vision_transformer.py:179-211 (F.interpolate bicubic).
 * offset = interpolate_offset (l.194-202): != 0 -> scale_factor = (g + offset) / M, the vendored default 0.1; 0 -> the
 * output size is given.  antialias = interpolate_antialias (l.206): torch's anti-aliased bicubic (Keys A = -0.5, support
 * widened by the down-sampling factor); the hub's register models use offset 0, antialias 1.
 * pos_patch fp32 [M*M, E] -> out fp32 [gh*gw, E]. */
int mst_pos_embed_interp(const float* pos_patch, int M, int E, int gh, int gw, double offset, int antialias,
                         float* out, mst_stream_t stream);

/* Gray->RGB + Conv2d(3,E,14,14) + flatten + CLS/register rows + position add:
 * dino.py:125-127; patch_embed.py:68-81; vision_transformer.py:213-232.
 * vol [n, H, W] (in_dtype f32/f16/bf16), wp = channel-summed kernel [E][224] in compute dtype
 * (k = ky*16+kx, kx 14,15 zero), prefix fp32 [1+R, E] (row 0 = cls_token + pos[0], rows 1..R =
 * register tokens), pos_patch fp32 [Np, E].  Writes tokens x fp32 [n, 1+R+Np, E]. */
int mst_patch_embed(const void* vol, int in_dtype, int n, int H, int W, const void* wp, int dtype,
                    const float* bias, const float* prefix, int n_prefix, const float* pos_patch,
                    int E, float* x, mst_stream_t stream);

/* Convolutional backbone of the ResNet models (reference mst/models/resnet.py:44-50,127-243 on torchvision's
 * resnet34, which is not part of the reference tree: the published architecture is restated).  Activations are NHWC fp32, so a
 * convolution (+ folded BatchNorm + ReLU / residual) is mst_im2col_nhwc followed by mst_gemm with the matching epilogue.
 * mst_im2col_nhwc: x [n,H,W,C] -> col [n*Ho*Wo, Kpad], col[(n,oy,ox)][(ky,kx,c)] = x[n][oy*stride-pad+ky][ox*stride-pad+kx][c],
 *   zero outside the image and for k >= kh*kw*C.  mst_maxpool_nhwc: 3x3, stride 2, padding 1 (the resnet stem).
 * mst_avgpool_nhwc: x [n, HW, C] -> y [n, C], the adaptive average pool to 1x1. */
int mst_im2col_nhwc(const float* x, int n, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad, float* col,
                    mst_stream_t stream);
/* mst_conv_gemm: the same convolution (+ folded BatchNorm bias, ReLU / residual epilogues of mst_gemm) as an IMPLICIT GEMM: the A operand
 * is gathered from x [n,H,W,Cin] on the fly, no [rows, kh*kw*Cin] matrix is materialised (9x the activation for a 3x3 layer).  Cin % 16
 * == 0 (every layer behind the stem); Wg [Cout, Kpad] and the (ky, kx, c) order as above; out [n*Ho*Wo, Cout] fp32 (read and written
 * by MST_EPI_RESIDUAL / _RESIDUAL_RELU); epilogue MST_EPI_BIAS / MST_EPI_BIAS_RELU / MST_EPI_RESIDUAL / MST_EPI_RESIDUAL_RELU. */
int mst_conv_gemm(const float* x, int n, int H, int W, int Cin, int kh, int kw, int stride, int pad, const float* Wg, const float* bias,
                  float* out, int Cout, int Kpad, int epilogue, const float* gamma, mst_stream_t stream);
/* mst_conv_gemm16: the implicit-GEMM convolution on 16-bit MFMA operands (fp32 accumulation): x [n,H,W,Cin] and Wg [Cout, kh*kw*Cin] bf16 / f16
 * (Cin % 64 == 0, Cout % 4 == 0), out [n*Ho*Wo, Cout] of out_dtype: MST_EPI_BIAS / MST_EPI_BIAS_RELU -> the operand type or f32;
 * MST_EPI_RESIDUAL_RELU -> out = relu(out + conv + bias) in place on a 16-bit out (the residual unit's exit).  The 16-bit inference path of
 * the ResNet backbone (ResNet(..., compute_dtype='bf16')).  mst_cvt32: out[i] = float(x[i]), n % 4 == 0. */
int mst_conv_gemm16(const void* x, int dtype, int n, int H, int W, int Cin, int kh, int kw, int stride, int pad, const void* Wg, const float* bias,
                    void* out, int out_dtype, int Cout, int epilogue, mst_stream_t stream);
int mst_cvt32(const void* x, int dtype, int64_t n, float* out, mst_stream_t stream);
/* The stem of the 16-bit backbone: mst_im2col_nhwc with the rows rounded to out_dtype (bf16 / f16) on the way out, and mst_maxpool_nhwc on
 * 16-bit activations (3 x 3, stride 2, padding 1). */
int mst_im2col_nhwc16(const float* x, int n, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad, void* col, int out_dtype,
                      mst_stream_t stream);
int mst_maxpool_nhwc16(const void* x, int dtype, int n, int H, int W, int C, void* y, mst_stream_t stream);
/* mst_conv_dgrad: d input of a convolution AS a convolution (what torch.autograd's conv backward gives the reference): the same implicit GEMMs
 * with stride 1, padding k - 1 - pad and the gradient rows dilated by the forward stride (1 or 2), instead of dZ . W into a [rows, kh*kw*Cin]
 * matrix and a scatter with atomics (mst_col2im_nhwc).  dz [n,Ho,Wo,Cout] and Wt [Cin, kh*kw*Cout] of `dtype` (f32: Cout % 16 == 0; bf16 / f16:
 * Cout % 64 == 0), Wt[c][(ky',kx',co)] = W[co][c][k-1-ky'][k-1-kx']; dx fp32 [n*H*W, Cin], overwritten. */
/* mst_conv_wgrad: d weight of a convolution as an implicit GEMM: part[z][co][(ky,kx,c)] = sum over the output pixels [z rps, (z + 1) rps) of
 * dz[r][co] * x[pixel(r) + (ky,kx)][c] -- nsplit partial products fp32 [nsplit, Cout, kh*kw*Cin] (the caller sums them: mst_colsum), B operand
 * gathered from x [n,H,W,Cin] (no im2col matrix).  dz [n*Ho*Wo, Cout] fp32; Cin % 64 == 0, Cout % 4 == 0, nsplit * rows_per_split >= rows. */
int mst_conv_wgrad(const float* dz, const float* x, int n, int H, int W, int Cin, int kh, int kw, int stride, int pad, int Cout, float* part,
                   int nsplit, int64_t rows_per_split, mst_stream_t stream);
/* mst_conv_wgrad16: the same partial products from 16-bit operands (dz and x bf16 / f16; Cin % 64 == 0, Cout % 64 == 0, rows_per_split % 64 == 0):
 * pixel-major tiles in LDS, fragments through the hardware-transposing LDS read. */
int mst_conv_wgrad16(const void* dz, const void* x, int dtype, int n, int H, int W, int Cin, int kh, int kw, int stride, int pad, int Cout, float* part,
                     int nsplit, int64_t rows_per_split, mst_stream_t stream);
int mst_conv_dgrad(const void* dz, int dtype, int n, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, const void* Wt, int H, int W,
                   int Cin, float* dx, mst_stream_t stream);
/* mst_conv_dgrad_stem: d input of a THIN-input convolution (Cin 1, 2 or 3, where mst_conv_dgrad needs Cin % 4 == 0): the stem of the ResNet
 * models -- torchvision's conv1, 7 x 7, stride 2, padding 3, 64 output channels, on the grey slice that reference resnet.py:176 repeats into
 * three channels (folded: one channel, the three kernels summed) or on three real channels (plain ResNet).  The last link of the gradient
 * with respect to the input volume.  dz [n,Ho,Wo,Cout] and Wg [Cout, kh*kw*Cin] -- the FORWARD's GEMM weight in (ky, kx, c) order, dense
 * rows -- of `dtype` (f32 / bf16 / f16; 16-bit operands are widened and multiplied on the exact fp32 MFMA); dx fp32 [n,H,W,Cin], every
 * element written exactly once.  Per tile of input pixels the product dz . Wg of the output positions that reach it stays in LDS and each
 * pixel gathers its taps in ascending (ky, kx) order: no atomics, no workspace, and the summation order is fixed by the shape arguments,
 * so the determinism contract below holds without an _ordered twin.  Cin in {1,2,3}, kh = kw <= 7, stride 1 or 2, 0 <= pad < kh, Cout 16,
 * 32 or 64; anything else is MST_EINVAL. */
int mst_conv_dgrad_stem(const void* dz, int dtype, int n, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, const void* Wg, int H,
                        int W, int Cin, float* dx, mst_stream_t stream);
int mst_maxpool_nhwc(const float* x, int n, int H, int W, int C, float* y, mst_stream_t stream);
int mst_avgpool_nhwc(const float* x, int n, int HW, int C, float* y, mst_stream_t stream);
/* Training step of the backbone (BASELINE configs[3]; what torch.autograd + nn.BatchNorm2d(train) do for the reference):
 * mst_batchnorm_train: z [rows, C] (raw convolution output) -> y = gamma (z - mean) rstd + beta (+ residual) (ReLU if relu) with the
 *   BATCH statistics (biased variance); mean / rstd [C] are kept for the backward; running_mean / running_var (nullable) are
 *   updated as nn.BatchNorm2d does (momentum, unbiased variance); scratch: C floats.
 * mst_batchnorm_bwd: dgamma, dbeta (+=, zero them first) and dz = gamma rstd (dy - dbeta/rows - xhat dgamma/rows).
 * mst_col2im_nhwc: adjoint of mst_im2col_nhwc, dx += (fp32 atomics; zero dx first): dX of a convolution = col2im(dZ . W).
 * mst_maxpool_bwd_nhwc (gradient to the first maximum of each window), mst_avgpool_bwd_nhwc. */
int mst_batchnorm_train(const float* z, int64_t rows, int C, const float* gamma, const float* beta, float eps, float momentum,
                        const float* residual, int relu, float* y, float* mean, float* rstd, float* running_mean,
                        float* running_var, float* scratch, mst_stream_t stream);
int mst_batchnorm_bwd(const float* z, const float* mean, const float* rstd, const float* gamma, const float* dy, int64_t rows, int C,
                      float* dgamma, float* dbeta, float* dz, mst_stream_t stream);
int mst_col2im_nhwc(const float* dcol, int n, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad, float* dx,
                    mst_stream_t stream);
int mst_maxpool_bwd_nhwc(const float* x, const float* dy, int n, int H, int W, int C, float* dx, mst_stream_t stream);
int mst_avgpool_bwd_nhwc(const float* dy, int n, int HW, int C, float* dx, mst_stream_t stream);
/* Grad-CAM++ map of the backbone's last ReLU output (reference mst/models/resnet.py:93-118 compute_attention_maps /
 * compute_grad_cam_weights, the map get_attention_maps returns): act [n, HW, C] fp32 NHWC; out [n, O] = the model output whose
 * per-image maximum is the loss (resnet.py:66-68); W [O, C] = the fc weight, or NULL when the output IS the pooled features
 * (O == C).  d loss / d pooled features = W[argmax] (or the one-hot), and behind the global average pool every position of a
 * channel has that gradient / HW -> cam [n, HW] = relu(sum_c w_c act_c), shifted by the global minimum and divided by the global
 * maximum as the reference does.  state: 2 floats of scratch. */
int mst_gradcampp(const float* act, const float* out, int O, const float* W, int n, int HW, int C, float* cam, float* state,
                  mst_stream_t stream);

/* Input pipeline in front of the model (reference mst/data/datasets/augmentations/augmentations_3d.py on
 * torchio 0.19.9, which is not part of the reference tree: restated from its published algorithm, numpy.pad semantics included).
 * mst_crop_or_pad: CropOrPad (l.144-195) with the deterministic centre (random_center=False: ini = ceil(n/2), fin = n - ini per
 *   axis).  src fp32 [s0,s1,s2] -> dst fp32 [t0,t1,t2]; padding first (pad_minimum = 1: numpy.pad mode 'minimum', axis after
 *   axis, what the datasets use; 0: the constant pad_value), then cropping.  ws: (s0+p0)(s1+p1)(s2+p2) floats when an axis is
 *   padded while another is cropped, else unused.
 * mst_znorm: ZNormalization (l.40-86) of ONE channel (per_channel=True, per_slice=False) with the datasets' masking method
 *   (x > x.min()) & (x < x.max()): cut-offs = torch.quantile(masked values, {q_lo, q_hi}) (linear), clamp, then
 *   y = (clamp(x) - mean) / std with mean / unbiased std of the masked clamped values.  Everything stays on the device (exact
 *   order statistics by radix select); `state` (mst_znorm_state_bytes()) receives, among others, a zero_std flag the host mirror
 *   turns into the reference's RuntimeError. */
int mst_crop_or_pad(const float* src, int s0, int s1, int s2, float* dst, int t0, int t1, int t2, int pad_minimum,
                    float pad_value, void* ws, size_t ws_bytes, mst_stream_t stream);
size_t mst_znorm_state_bytes(void);
int mst_znorm(const float* x, int64_t n, float q_lo, float q_hi, float* y, void* state, mst_stream_t stream);
/* mst_crop_or_pad_at: mst_crop_or_pad with the begin offsets given per axis instead of the centre rule -- CropOrPad(random_center=True)
 *   (augmentations_3d.py:166-195: the crop begin `ini` is uniform in 0..excess, l.170; the leading pad `r` uniform in 0..total pad,
 *   l.184-188); the caller draws them.  crop_a in 0..max(s_a - t_a, 0), pad_a in 0..max(t_a - s_a, 0), refused otherwise.  With the centre
 *   values ceil(excess / 2) and ceil(total / 2) it is mst_crop_or_pad.  Same workspace. */
int mst_crop_or_pad_at(const float* src, int s0, int s1, int s2, float* dst, int t0, int t1, int t2, int crop0, int crop1, int crop2,
                       int pad0, int pad1, int pad2, int pad_minimum, float pad_value, void* ws, size_t ws_bytes, mst_stream_t stream);

/* Training augmentation of a batch of volumes on the device: what the reference's datasets apply behind ZNormalization on CPU workers
 * (mst/data/datasets/dataset_3d_duke.py:44-47; the same lines in dataset_3d_lidc.py and dataset_3d_mrnet.py), in their order:
 *   tio.RandomAffine(scales=0, degrees=(0,0,0,0,0,90), translation=0, default_pad_value='minimum')   l.44  rotation about the slice axis
 *   tio.RandomFlip((0, 1, 2))                                                                        l.45
 *   tio.Lambda(lambda x: -x if torch.rand((1,))[0] < 0.5 else x)                                     l.46
 *   tio.RandomNoise(std=(0.0, 0.25))                                                                 l.47
 * mst_augment_volumes: in [n, D, H, W] (in_dtype: fp32 / fp16 / bf16) -> out, the same shape (out_dtype likewise; out != in: a gather).
 *   params [n, 8] fp32 in device memory, one record per volume: cos t, sin t, fill, sign, noise_std, flipD, flipH, flipW (a flip is
 *   taken when its float is non-zero).  Output voxel (d, h, w) reads the rotated volume at (d', h', w'), a flipped axis reversed
 *   (d' = D-1-d, ...).  The rotation is in the H-W plane, the same for every slice: c_h = (H-1)/2, c_w = (W-1)/2, y = h' - c_h,
 *   x = w' - c_w,  s_h = c_h + cos t y - sin t x,  s_w = c_w + sin t y + cos t x;  the sample is bilinear with neighbour indices clamped
 *   to the grid; it is inside iff -0.5 <= s_h < H-0.5 and -0.5 <= s_w < W-0.5, otherwise the value is `fill`.  cos t == 1 and
 *   sin t == 0 copies the voxel bit for bit.  The value is then multiplied by sign and noise_std N(0,1) is added (nothing is drawn
 *   when noise_std == 0).  N(0,1): Philox4x32-10 keyed by `seed`, counter words (g, 0, c_lo, c_hi) with g = (linear voxel index in its
 *   volume) / 4 and c = counter + volume index, the four output words serving voxels 4g..4g+3 through two Box-Muller pairs
 *   (u = ((word >> 9) + 0.5) / 2^23; z0, z1 = sqrt(-2 ln u0) (cos, sin)(2 pi u1)): a function of (seed, counter, volume, voxel) alone,
 *   not of the launch geometry.  A 16-bit output is the fp32 result rounded once.  No floating-point atomics, no workspace.
 *   NOT pinned against torchio / SimpleITK (neither is part of the reference tree): the rotation's sense, its centre and the edge rule
 *   are the definition above.
 * mst_volume_min: out[v * out_stride] = min of volume v of x [n, elems] (dtype), v < n -- the 'minimum' fill (default_pad_value), written
 *   straight into the records when out = params + 2, out_stride = 8.  min is order-independent: integer atomics on the bit pattern,
 *   branched on the sign bit (a -0.0 is a negative pattern: it cannot displace a negative minimum), the same bits under both modes of
 *   torch.use_deterministic_algorithms.  NaNs are skipped. */
int mst_augment_volumes(const void* in, int in_dtype, void* out, int out_dtype, int n, int D, int H, int W, const float* params,
                        uint64_t seed, uint64_t counter, mst_stream_t stream);
int mst_volume_min(const void* x, int dtype, int n, int64_t elems, float* out, int out_stride, mst_stream_t stream);

/* slices2rgb (mst/models/dino.py:10-27; dead code in the reference: its call at dino.py:129 is commented out): three
 * consecutive gray slices become the channels of one image.  vol [B,1,D,H,W] (dtype) -> out [B*Dp/3, 3, H, W] with
 * Dp = D rounded up to a multiple of 3, the extra slices being the volume's own first Dp-D slices (needs Dp-D <= D). */
int mst_slices2rgb(const void* vol, int dtype, int B, int D, int H, int W, void* out, mst_stream_t stream);

/* Fused MLP half of a ViT block (block.py:93-94,113; mlp.py:34-40), E = 384, 16-bit operands:
 *   x[M,E] (fp32, in place) += ls2 * (fc2(gelu(fc1(normalise(x)))) + b2);  xn_out (nullable, dtype) = normalise(x_new)
 * with LayerScale ls2 folded by the caller into W2's rows and into b2f = ls2 * b2 (ls2 = 1 when absent).
 * normalise = LayerNorm without affine (eps).  The hidden activations stay on chip.
 * wpack: 48 chunks x 49152 B, chunk c = LDS image of W1f rows [32c,32c+32) and W2 columns [32c,32c+32):
 *   W1 part  [ks 0..11][h 0..31][slot 0..3][8]  = W1f[32c+h][32ks + 8(slot^f(h)) ..+7],   f(r) = (-(r>>2))&3
 *   W2 part  [R 0..383][slot 0..3][8]           = ls2[n(R)] * W2[n(R)][32c + phys(slot^f(R), 0..7)]
 *     n(R)      = 32((R>>4)>>1) + 8((R&15)>>2) + 4((R>>4)&1) + (R&3)
 *     phys(c,j) = j<4 ? 4c+j : 16+4c+(j-4)
 *   W1f = fc1_w * ln2_w (columns);  b1f (fp32, 1536+32 padded) = fc1_b + fc1_w . ln2_b;  b2 = fc2 bias.
 * (mst.hip.pack_mlp builds it.) */
int mst_mlp_fused(float* x, void* xn_out, int dtype, const void* wpack, const float* b1f, const float* b2f,
                  int64_t M, int E, float eps, mst_stream_t stream);

/* Everything of a ViT block after the attention kernel in ONE launch (E = 384, 16-bit operands): the out-projection
 * (attention.py:67-68) + residual (block.py:90-91,112), then the fused MLP half exactly as mst_mlp_fused:
 *   x[M,E] (fp32, in place) += ls1 * (proj(attn_out) + b_proj);  x += ls2 * (fc2(gelu(fc1(normalise(x)))) + b2);
 *   xn_out (nullable, dtype; MAY alias attn_out) = normalise(x_new)
 * x is read once and written once.  attn_out [M,E] dtype.  proj_pack: 12 chunks x 24576 B, chunk j = LDS image
 *   [R 0..383][slot 0..3][8] = ls1[n(R)] * proj_w[n(R)][32j + 8(slot^f(R)) ..+7]   (n, f as in mst_mlp_fused),
 * proj_bf fp32 [E] = ls1 * proj_b (ls1 = 1 when absent); wpack / b1f / b2f as mst_mlp_fused.  scratch: at least
 * mst_block_fused_scratch_bytes() (96 KiB per compute unit: the LayerNorm2 hand-off between the kernel's wave roles). */
size_t mst_block_fused_scratch_bytes(void);
int mst_block_fused(float* x, const void* attn_out, void* xn_out, int dtype, const void* proj_pack, const float* proj_bf,
                    const void* wpack, const float* b1f, const float* b2f, void* scratch, size_t scratch_bytes, int64_t M,
                    int E, float eps, mst_stream_t stream);

/* The same block tail (attention.py:67-68; block.py:90-94,112-113; mlp.py:34-40) as mst_block_fused, in the round-3 SINGLE-ROLE
 * form: one wave per SIMD owns 32 token rows end to end (y^T accumulators, the LayerNorm2 rows and the hidden activations never
 * leave its registers), so no scratch and no activation hand-off exist.  Same arithmetic contract and aliasing rules.
 * block_seq: the block's weights as ONE stream of 108 elements x 24576 B in the order the kernel consumes them --
 *   12 out-projection chunks, W1(0), then W1(c+1), W2(c) for c = 0..46, then W2(47) -- each element 24 MFMA A-fragments
 *   [fragment f = 2t+p][lane l][8], m = l & 31, h = l >> 5, k8(e) = 16p + 8(e>>2) + 4h + (e&3):
 *     out-projection chunk j : ls1[32t+m] * proj_w[32t+m][32j + 16p + 8h + e]
 *     W1 chunk c (f = k-step): ln2_w[.] * fc1_w[32c+m][32t + k8(e)]
 *     W2 chunk c             : ls2[32t+m] * fc2_w[32t+m][32c + k8(e)]
 * b1f fp32 [1536] = fc1_b + fc1_w . ln2_b; proj_bf fp32 [E] = ls1 * proj_b; b2f fp32 [E] = ls2 * fc2_b.
 * layout: 0 = every operand row-major, or a combination of mst_layout_flags.  The kernel's lanes own ROWS, so a row-major operand
 * costs 32 scattered 32-byte runs per memory instruction; between two blocks of one encoder the operands stay in the order the
 * registers hold them (buffers then cover whole groups of 32 rows: round M up to a multiple of 32 when allocating):
 *   16-bit "blocked" [M/32 groups][24 pieces][64 slots][8]: element (row r, column c) of group g at piece c/16, slot (r%32) + 32*((c/8)%2),
 *     position c%8 (a piece = one contiguous KiB = 32 rows x 16 consecutive columns; natural column order);
 *   fp32 "image"     [M/32 groups][48 pieces][64 slots][4]: element (r, c) at piece c/8, slot (r%32) + 32*((c/4)%2), position c%4.
 * REQUIREMENT: a buffer named by a layout flag -- x under either X flag; attn_out and xn_out under ACT_BLOCKED -- must be allocated for
 * ceil(M / 32) * 32 rows, whatever M is: the kernel reads and writes its last group whole (the rows past M hold nothing meaningful).  The
 * C entry point sees pointers only and cannot check this; the Python wrapper (mst.hip.block_fused_s) checks the storage behind each
 * tensor and refuses a short one before any launch.  mst_attention_ex (MST_ATTN_OUT_BLOCKED) and mst_gemm16_blocked state the same size
 * for their blocked operand; their wrappers take it from the tensor's shape. */
enum mst_layout_flags {
    MST_LAYOUT_X_IN_IMAGE = 1,   /* x is read in the fp32 image layout  */
    MST_LAYOUT_X_OUT_IMAGE = 2,  /* x is written in the fp32 image layout (in place also when the x flags differ: a 32-row group
                                  * occupies the same 48 KiB in both layouts and is read whole before it is written) */
    MST_LAYOUT_ACT_BLOCKED = 4   /* attn_out is read and xn_out written in the 16-bit blocked layout */
};
int mst_block_fused_s(float* x, const void* attn_out, void* xn_out, int dtype, const void* block_seq, const float* b1f,
                      const float* proj_bf, const float* b2f, int64_t M, int E, float eps, int layout, mst_stream_t stream);

/* Training step: what torch.autograd does for the reference (base_model.py:148-181, main_train.py:110-126),
 * as per-op entry points; mst/train.py orchestrates them behind a torch.autograd.Function.  All fp32, exact fp32 MFMA.
 * mst_gemm_ex: C[b] = alpha * A[b] . B[b] + beta * C[b], A [M,K], B [K,N], C [M,N] with element strides
 *   strides[12] = {A_m, A_k, B_k, B_n, C_m, C_n, A_b1, A_b2, B_b1, B_b2, C_b1, C_b2}, batch index b = b1 * nb2 + b2
 *   (dX = dY.W, dW = dY^T.X of nn.Linear; S = q.k^T, O = P.v and the four backward products of attention.py:56-66 on the
 *   packed q|k|v rows).  nb1 * nb2 <= 65535.
 * mst_softmax_rows: S [rows, L] -> softmax over L in place; mask (nullable) uint8 [rows / rows_per_batch, L], 1 = key
 *   ignored (src_key_padding_mask, transformer_blocks.py:244-252).  mst_softmax_rows_bwd: dP <- scale * P o (dP - rowsum(dP o P)).
 * mst_layernorm_bwd: dx[r] = (dres ? dres[r] : 0) + LayerNorm'(x[r]; gamma) . dy[r]; dgamma[c] += sum_r dy xhat, dbeta[c] += sum_r dy
 *   (dx, dres, dgamma, dbeta, gamma nullable; row strides in elements; cols <= 2048; accumulation by fp32 atomics).
 * mst_act_fwd / mst_act_bwd: kind 0 GELU (erf form, mlp.py:22), 1 ReLU; bwd: dy <- dy * act'(h) in place.
 * mst_colsum: out[c] += sum_r a[r][c] * (b ? b[r][c] : 1)   (bias and LayerScale gradients).
 * mst_axpby_cols: y[r][c] = alpha * x[r][c] * (g ? g[c] : 1) + beta * y[r][c].
 * mst_im2col14: vol [n,H,W] -> col fp32 [n*Np, 196], the 14 x 14 patches as rows (patch_embed.py:68-81; d W = dX^T . col).
 * mst_pos_embed_interp_bwd: dpos [M*M, E] += adjoint of mst_pos_embed_interp (antialias = 0) applied to dout [gh*gw, E]. */
/* Mixed-precision training step (the reference trains under precision='16-mixed': scripts/main_train.py:110-123): activations, weights and
 * gradients stay fp32 in memory, the products of nn.Linear run on 16-bit MFMA operands with fp32 accumulation.
 * mst_cvt16: out[r][c] = T(scale * x[r][c]) for r < rows, c < cols (transpose = 0; cols, ldx, ldo multiples of 4), or the TRANSPOSED image
 *   out[c][r], r < rows_pad, zero-filled for r >= rows (transpose = 1): both operands of d weight = dY^T . X contiguous along the token index.
 * mst_gemm16_splitk: Cpart[z] (fp32 [M, N], split_stride elements apart) = A[:, z Kc:(z+1) Kc] . W[:, z Kc:(z+1) Kc]^T, Kc = K / splits a
 *   multiple of 64, N of 128; the caller sums the partial products (mst_colsum over [splits, M * N]). */
int mst_cvt16(const float* x, int64_t ldx, int64_t rows, int cols, float scale, void* out, int out_dtype, int64_t ldo, int transpose,
              int64_t rows_pad, mst_stream_t stream);
int mst_gemm16_splitk(const void* A, int ab_dtype, int64_t lda, const void* W, int64_t ldw, float* Cpart, int64_t ldc, int64_t M, int N, int K,
                      int splits, int64_t split_stride, mst_stream_t stream);
/* mst_rope_rows: RoPE of the across-slice attention (rotary_embedding_torch.py:38-62,159-173) in place on packed q | k | v rows [rows, 3 * heads *
 * head_dim]: the pairs (2p, 2p+1) of q and k rotated by sign * (row % L) * freqs[p]; sign +1 = the training forward, -1 = its adjoint on the
 * gradient rows (the frequencies carry no gradient: learned_freq = False). */
int mst_rope_rows(float* qkv, int64_t rows, int L, int heads, int head_dim, const float* freqs, float sign, mst_stream_t stream);
int mst_gemm_ex(const float* A, const float* B, float* C, int M, int N, int K, const int64_t* strides, int nb1, int nb2,
                float alpha, float beta, mst_stream_t stream);
int mst_softmax_rows(float* S, const uint8_t* mask, int64_t rows, int L, int rows_per_batch, mst_stream_t stream);
int mst_softmax_rows_bwd(const float* P, float* dP, int64_t rows, int L, float scale, mst_stream_t stream);
int mst_layernorm_bwd(const float* x, int64_t x_stride, const float* gamma, const float* dy, int64_t dy_stride, const float* dres,
                      int64_t dres_stride, float* dx, int64_t dx_stride, float* dgamma, float* dbeta, int64_t rows, int cols,
                      float eps, mst_stream_t stream);
int mst_act_fwd(const float* h, float* y, int64_t n, int kind, mst_stream_t stream);
int mst_act_bwd(const float* h, float* dy, int64_t n, int kind, mst_stream_t stream);
/* SwiGLU of the training step (swiglu_ffn.py:54-72) in the reference layout x12 = [x1 | x2] (chunk(2, dim=-1)): x12 fp32 [rows, 2 hidden],
 * mst_swiglu_fwd: h[r][c] = silu(x12[r][c]) * x12[r][hidden + c], h fp32 [rows, hidden];
 * mst_swiglu_bwd: with s = sigmoid(x1): dx12[r][c] = dh x2 s (1 + x1 (1 - s)), dx12[r][hidden + c] = dh x1 s, dx12 fp32 [rows, 2 hidden]
 * (every element written; must not alias x12).  No reduction: one entry point for both determinism modes.  Any positive rows, hidden. */
int mst_swiglu_fwd(const float* x12, float* h, int64_t rows, int hidden, mst_stream_t stream);
int mst_swiglu_bwd(const float* x12, const float* dh, float* dx12, int64_t rows, int hidden, mst_stream_t stream);
int mst_colsum(const float* a, int64_t a_stride, const float* b, int64_t b_stride, int64_t rows, int cols, float* out,
               mst_stream_t stream);
int mst_axpby_cols(const float* x, int64_t x_stride, const float* g, float alpha, float beta, float* y, int64_t y_stride,
                   int64_t rows, int cols, mst_stream_t stream);
int mst_im2col14(const void* vol, int dtype, int n, int H, int W, float* col, mst_stream_t stream);
int mst_pos_embed_interp_bwd(const float* dout, int M, int E, int gh, int gw, double offset, float* dpos, mst_stream_t stream);
/* mst_patch_embed_dgrad: gradient of the training step with respect to the input volume -- the adjoint of the grey -> RGB repeat
 * (mst/models/dino.py:121-127) and of the stride-14 patch convolution (extern/dinov2/layers/patch_embed.py:68-81):
 *   dvol[s][14 py + i][14 px + j] = sum_e dx[s * tokens_per_image + first_patch_token + py * gw + px][e] * wsum[e][16 i + j]   (i, j < 14)
 * dx fp32 [n * tokens_per_image, E] (the encoder's token gradient: first_patch_token = 1 + registers; or the patch rows alone,
 * tokens_per_image = Np, first_patch_token = 0), wsum fp32 [E, 14 * 16] the three channel kernels summed (the one mst_patch_embed reads,
 * columns 14, 15 of every kernel row unused), dvol fp32 [n, H, W], every pixel written once.  H, W multiples of 14, E a multiple of 16,
 * dx and wsum 16-byte aligned.  Exact fp32 MFMA, no atomics: bit-reproducible, one entry point for both determinism modes. */
int mst_patch_embed_dgrad(const float* dx, int tokens_per_image, int first_patch_token, const float* wsum, int n, int H, int W, int E,
                          float* dvol, mst_stream_t stream);
/* The patch embedding of true three-channel images (the encoder API's [n, 3, H, W] input; extern/dinov2/layers/patch_embed.py:65,75-81:
 * Conv2d(3, E, 14, stride 14), flatten, transpose) at the op level, all operands fp32 as in the training step's mst_patch_embed.
 * wp fp32 [E][3][14][16] is the kernel image (Conv2d weight [E, 3, 14, 14], every kernel row padded to 16 with zeros).  H, W multiples
 * of 14; anything outside the rules below returns MST_EINVAL.
 * mst_patch_embed_rgb (forward): x[s][n_prefix + py gw + px][e] = sum_{c,i,j} img[s][c][14 py + i][14 px + j] w[e][c][i][j] + bias[e] +
 *   pos_patch[py gw + px][e];  x[s][r] = prefix[r] for r < n_prefix.  img fp32 [n, 3, H, W] (8-byte aligned), prefix fp32 [n_prefix >= 1, E],
 *   pos_patch fp32 [Np, E], x fp32 [n, n_prefix + Np, E]; E a multiple of 64; wp, bias, pos_patch, x 16-byte aligned.  The kernel of
 *   mst_vit_encode_features' RGB input in its fp32 mode (v_mfma_f32_16x16x4_f32).
 * mst_patch_embed_rgb_dgrad (input gradient):
 *   dimg[s][c][14 py + i][14 px + j] = sum_e dx[s * tokens_per_image + first_patch_token + py gw + px][e] * w[e][c][i][j]
 *   dx fp32 [n * tokens_per_image, E] as in mst_patch_embed_dgrad, dimg fp32 [n, 3, H, W], every pixel written once.  E a multiple of 16,
 *   dx and wp 16-byte aligned.  Exact fp32 MFMA, no atomics: bit-reproducible, one entry point for both determinism modes.
 * mst_patch_embed_rgb_wgrad (weight gradient), an implicit GEMM over the image in place, split over the patch rows m = s Np + p:
 *   part[z][e][c][i][j] = sum_{m in [z rows_per_split, (z + 1) rows_per_split)} dx[s * tokens_per_image + first_patch_token + p][e] *
 *   img[s][c][14 py + i][14 px + j];  dW = sum_z part[z] is the caller's (mst_colsum / mst_colsum_ordered over [splits, E * 588]).
 *   part fp32 [ceil(n Np / rows_per_split), E, 3, 14, 14], every element written; rows_per_split a positive multiple of 16 with at most
 *   65535 splits; E a multiple of 64; dx 16-byte, img 8-byte aligned.  Exact fp32 MFMA, no atomics. */
int mst_patch_embed_rgb(const float* img, int n, int H, int W, const float* wp, const float* bias, const float* prefix, int n_prefix,
                        const float* pos_patch, int E, float* x, mst_stream_t stream);
int mst_patch_embed_rgb_dgrad(const float* dx, int tokens_per_image, int first_patch_token, const float* wp, int n, int H, int W, int E,
                              float* dimg, mst_stream_t stream);
int mst_patch_embed_rgb_wgrad(const float* dx, int tokens_per_image, int first_patch_token, const float* img, int n, int H, int W, int E,
                              int rows_per_split, float* part, mst_stream_t stream);

/* 16-bit storage mode of the training step (mst/train.py, train_storage='16bit'): under the reference's Trainer(precision='16-mixed')
 * (scripts/main_train.py:110-123) autocast keeps what a block saves for its backward (block.py:89-114) in the 16-bit type T = dtype
 * (MST_BF16 / MST_F16); the residual stream and every gradient stay fp32.  Conversions to T round to nearest even.  Any other dtype,
 * a misaligned base or a shape outside the rules below returns MST_EINVAL.
 * mst_residual_layernorm16: one pass over `rows` contiguous rows of `cols` elements (block.py:108-113 residual + layer_scale.py:26-27
 *   + the next nn.LayerNorm, block.py:63,75):  x_out[r][c] = x_in[r][c] + gamma[c] * float(br[r][c])  (fp32, one rounding; gamma NULL:
 *   no LayerScale),  y[r] = T(LayerNorm(x_out[r]; ln_w, ln_b, eps)).  y NULL: the residual only (ln_w, ln_b unused).  x_out must not alias x_in.
 *   cols a multiple of 8 (every row 16-byte aligned in both types), <= 2048; all bases 16-byte aligned.
 * mst_act_fwd16 / mst_act_bwd16: y[i] = T(act(float(h[i]))) and dy[i] (fp32, in place) *= act'(float(h[i])), kind as mst_act_fwd (mlp.py:22):
 *   the fp32 formulas of mst_act_fwd / mst_act_bwd, so the results are theirs on the upcast h bit for bit.  n may be ANY positive
 *   count (whole groups of 8, then a scalar tail); h, y, dy 16-byte aligned.
 * mst_colsum_b16 / mst_colsum_b16_ordered: out[c] += sum_r a[r][c] * float(b[r][c]) -- the LayerScale gradient (layer_scale.py:25-27) with
 *   the saved branch output in T; mst_colsum's `b` form.  cols and both row strides multiples of 4, strides >= cols, a 16-byte and b 8-byte
 *   aligned.  The ordered form follows the ORDER CONTRACT below with the plan, the order and the workspace of mst_colsum_ordered
 *   (mst_colsum_ordered_workspace_bytes(rows, cols) bytes): its result has the bits of mst_colsum_ordered on the upcast b.
 * mst_transpose16: out[c][r] = x[r][c] for r < rows, 0 for rows <= r < rows_pad (x [rows, cols] T with row stride ldx, out [cols, rows_pad] T
 *   with row stride ldo >= rows_pad): the 16-bit-input counterpart of mst_cvt16(transpose = 1), the operand image of d weight = dY^T . X
 *   above 12,288 tokens (mst_gemm16_splitk).
 * mst_swiglu_fwd16 / mst_swiglu_bwd16: mst_swiglu_fwd / mst_swiglu_bwd with x12 (and h) in T: h = T(fp32 formula on float(x12)), one rounding;
 *   dh and dx12 stay fp32.  The results are those of the fp32 entry points on the upcast x12 bit for bit (h: rounded to T).  Any positive
 *   rows and hidden (16-byte accesses when hidden % 8 == 0, one element per thread otherwise); bases 16-byte aligned. */
int mst_residual_layernorm16(const float* x_in, const void* br, int dtype, const float* gamma, float* x_out, const float* ln_w,
                             const float* ln_b, void* y, int64_t rows, int cols, float eps, mst_stream_t stream);
int mst_act_fwd16(const void* h, void* y, int dtype, int64_t n, int kind, mst_stream_t stream);
int mst_act_bwd16(const void* h, int dtype, float* dy, int64_t n, int kind, mst_stream_t stream);
int mst_swiglu_fwd16(const void* x12, void* h, int dtype, int64_t rows, int hidden, mst_stream_t stream);
int mst_swiglu_bwd16(const void* x12, int dtype, const float* dh, float* dx12, int64_t rows, int hidden, mst_stream_t stream);
int mst_colsum_b16(const float* a, int64_t a_stride, const void* b, int b_dtype, int64_t b_stride, int64_t rows, int cols, float* out,
                   mst_stream_t stream);
int mst_colsum_b16_ordered(const float* a, int64_t a_stride, const void* b, int b_dtype, int64_t b_stride, int64_t rows, int cols, float* out,
                           void* workspace, size_t workspace_bytes, mst_stream_t stream);
int mst_transpose16(const void* x, int dtype, int64_t ldx, int64_t rows, int cols, void* out, int64_t ldo, int64_t rows_pad,
                    mst_stream_t stream);

/* 16-bit storage mode of the ResNet training step (mst/train_resnet.py, train_storage='16bit'; csrc/k_bn.hip): the convolution output z
 * and the unit's output y of a convolution + BatchNorm2d (+ residual, ReLU) unit live in T = dtype (MST_BF16 / MST_F16), as the reference's
 * autocast keeps them; statistics, gradients and every sum are fp32 and all arithmetic is fp32 on the upcast values.  Activations are
 * [rows, C] NHWC.  C must be a multiple of 8 and EVERY pointer 16-byte aligned; anything else, another dtype or a short workspace returns
 * MST_EINVAL.  The reductions follow the ORDER CONTRACT below whatever the determinism flag says: a workgroup sums a block of rows for 64
 * columns, stores its partial into the workspace with plain stores, and the partials are added in ascending block order -- no
 * floating-point atomic, bit-identical results run to run for fixed (rows, C).  The library never allocates: workspace of at least
 * ..._workspace_bytes(shape) bytes.  Conversions to T round the fp32 result to nearest even.
 * mst_batchnorm_train16: mst_batchnorm_train on z in T: the column mean, then the centred sum of squares (two passes), mean / rstd [C] kept
 *   for the backward, running_mean / running_var (nullable) updated as there;  y = T(relu?(gamma (z - mean) rstd + beta + float(residual)))
 *   (residual T [rows, C] or NULL).
 * mst_batchnorm_bwd16: the ReLU mask, both column sums, the input gradient and its rounding in one call.  m = float(y) > 0 (y NULL: no ReLU,
 *   m = 1);  dbeta = sum_r m dy,  dgamma = sum_r m dy xhat  (OVERWRITTEN, not accumulated);
 *   dz = T(gamma rstd (m dy - dbeta / rows - xhat dgamma / rows)), unscaled.  mask_dy_in_place != 0: dy <- m dy as well (for the shortcut
 *   branch that shares this gradient); pass 0 where nothing reads it.
 * mst_maxpool_bwd_nhwc16: mst_maxpool_bwd_nhwc_gather (dx +=, zero it first; fp32 dy / dx) with the pool INPUT x in T: the same
 *   first-maximum rule (ties included) and the same one-byte-per-window workspace, so the result has the bits of the fp32 form on the
 *   upcast x.
 * mst_avgpool_nhwc16: mst_avgpool_nhwc on x [n, HW, C] in T -> y [n, C] fp32, positions summed in that kernel's order (the same bits on
 *   the upcast x). */
size_t mst_batchnorm_train16_workspace_bytes(int64_t rows, int C);
int mst_batchnorm_train16(const void* z, int dtype, int64_t rows, int C, const float* gamma, const float* beta, float eps, float momentum,
                          const void* residual, int relu, void* y, float* mean, float* rstd, float* running_mean, float* running_var,
                          void* workspace, size_t workspace_bytes, mst_stream_t stream);
size_t mst_batchnorm_bwd16_workspace_bytes(int64_t rows, int C);
int mst_batchnorm_bwd16(const void* z, const void* y, int dtype, const float* mean, const float* rstd, const float* gamma, float* dy,
                        int mask_dy_in_place, int64_t rows, int C, float* dgamma, float* dbeta, void* dz, void* workspace, size_t workspace_bytes,
                        mst_stream_t stream);
size_t mst_maxpool_bwd_nhwc16_workspace_bytes(int n, int H, int W, int C);
int mst_maxpool_bwd_nhwc16(const void* x, int dtype, const float* dy, int n, int H, int W, int C, float* dx, void* workspace, size_t workspace_bytes,
                           mst_stream_t stream);
int mst_avgpool_nhwc16(const void* x, int dtype, int n, int HW, int C, float* y, mst_stream_t stream);

/* Fixed-order (deterministic) forms of every floating-point reduction of the training steps and of mst_znorm: what the Python layer calls
 * while torch.are_deterministic_algorithms_enabled().  ORDER CONTRACT: for fixed shape arguments (rows, cols, n, H, W, C, M, E, gh, gw,
 * kernel geometry) the summation order is fixed -- it does not depend on timing, occupancy, which XCD runs a workgroup, strides or pointer
 * alignment -- so two calls on the same inputs give bit-identical results.  None of them uses a floating-point atomic.  Each reduction
 * writes per-workgroup partials with plain stores into a caller-given workspace (the library never allocates) of at least
 * ..._workspace_bytes(shape) bytes (0 is a valid answer: then the workspace may be NULL) and sums them in ascending workgroup order.
 * The results agree with the atomic forms within fp32 reassociation error; they are not bit-identical to them.
 * mst_colsum_ordered: out[c] += sum_r a[r][c] * (b ? b[r][c] : 1), as mst_colsum, without its column-count limit (cols < 2^31 / rows
 *   blocks).  Row blocks of the plan of mst_colsum (about 2,048 workgroups); workspace [row blocks, cols] fp32, none for one row block.
 * mst_layernorm_bwd_ordered: mst_layernorm_bwd; dx computed exactly as there, d gamma / d beta (+=) through a [workgroups, 2, cols] slab.
 * mst_batchnorm_train_ordered: mst_batchnorm_train with the ordered column sums of the mean and the variance (its scratch lives in the
 *   workspace).  mst_batchnorm_bwd_ordered: mst_batchnorm_bwd (dgamma, dbeta +=, zero them first) through a [row blocks, 2, C] slab.
 * mst_col2im_nhwc_gather: mst_col2im_nhwc (dx +=) as a gather: every input element adds its entries in ascending (ky, kx).  No workspace.
 * mst_maxpool_bwd_nhwc_gather: mst_maxpool_bwd_nhwc (dx +=; the same first-maximum rule, ties included) as a gather: every input adds the dy
 *   of the windows whose argument it is in ascending (oy, ox).  Workspace: one byte per window.
 * mst_pos_embed_interp_bwd_ordered: mst_pos_embed_interp_bwd (dpos +=) as dpos += Wy^T . dout . Wx with the dense clamped tap matrices;
 *   workspace [gh, M, E] fp32.
 * mst_znorm_ordered: mst_znorm with fp64 per-workgroup moment partials summed by one workgroup.  Workspace: one double per workgroup. */
size_t mst_colsum_ordered_workspace_bytes(int64_t rows, int cols);
int mst_colsum_ordered(const float* a, int64_t a_stride, const float* b, int64_t b_stride, int64_t rows, int cols, float* out,
                       void* workspace, size_t workspace_bytes, mst_stream_t stream);
size_t mst_layernorm_bwd_ordered_workspace_bytes(int64_t rows, int cols);
int mst_layernorm_bwd_ordered(const float* x, int64_t x_stride, const float* gamma, const float* dy, int64_t dy_stride, const float* dres,
                              int64_t dres_stride, float* dx, int64_t dx_stride, float* dgamma, float* dbeta, int64_t rows, int cols,
                              float eps, void* workspace, size_t workspace_bytes, mst_stream_t stream);
size_t mst_batchnorm_train_ordered_workspace_bytes(int64_t rows, int C);
int mst_batchnorm_train_ordered(const float* z, int64_t rows, int C, const float* gamma, const float* beta, float eps, float momentum,
                                const float* residual, int relu, float* y, float* mean, float* rstd, float* running_mean,
                                float* running_var, void* workspace, size_t workspace_bytes, mst_stream_t stream);
size_t mst_batchnorm_bwd_ordered_workspace_bytes(int64_t rows, int C);
int mst_batchnorm_bwd_ordered(const float* z, const float* mean, const float* rstd, const float* gamma, const float* dy, int64_t rows, int C,
                              float* dgamma, float* dbeta, float* dz, void* workspace, size_t workspace_bytes, mst_stream_t stream);
int mst_col2im_nhwc_gather(const float* dcol, int n, int H, int W, int C, int kh, int kw, int stride, int pad, int Kpad, float* dx,
                           mst_stream_t stream);
size_t mst_maxpool_bwd_nhwc_gather_workspace_bytes(int n, int H, int W, int C);
int mst_maxpool_bwd_nhwc_gather(const float* x, const float* dy, int n, int H, int W, int C, float* dx, void* workspace, size_t workspace_bytes,
                                mst_stream_t stream);
size_t mst_pos_embed_interp_bwd_ordered_workspace_bytes(int M, int E, int gh, int gw);
int mst_pos_embed_interp_bwd_ordered(const float* dout, int M, int E, int gh, int gw, double offset, float* dpos, void* workspace,
                                     size_t workspace_bytes, mst_stream_t stream);
size_t mst_znorm_ordered_workspace_bytes(int64_t n);
int mst_znorm_ordered(const float* x, int64_t n, float q_lo, float q_hi, float* y, void* state, void* workspace, size_t workspace_bytes,
                      mst_stream_t stream);

/* Optional per-kernel timing of the launches inside mst_vit_encode (bench / profiling only).  A caller-owned object:
 * while mst_vit_weights.profiler points at one, every launch of that call is bracketed by hipEventRecord on the call's own
 * stream; mst_profiler_collect waits for the recorded events, returns the accumulated milliseconds and launch counts per
 * kernel kind since the last collect, and resets.  No process-global state: calls without a profiler record nothing. */
typedef struct mst_profiler mst_profiler;
enum mst_kernel_kind {
    MST_K_PATCH_EMBED = 0, MST_K_LAYERNORM = 1, MST_K_GEMM_QKV = 2, MST_K_ATTENTION = 3,
    MST_K_GEMM_PROJ = 4, MST_K_GEMM_FC1 = 5, MST_K_GEMM_FC2 = 6, MST_K_CLS_PROBS = 7, MST_K_MLP_FUSED = 8,
    MST_K_BLOCK_FUSED = 9,        /* out-projection + MLP in one launch (mst_block_fused) */
    MST_K_COUNT = 10
};
mst_profiler* mst_profiler_create(void);
void mst_profiler_destroy(mst_profiler* p);
int mst_profiler_collect(mst_profiler* p, double* ms_total, int64_t* launches); /* arrays of MST_K_COUNT */
const char* mst_kernel_kind_name(int kind);

/* Whole per-slice encoder ------------------------------------------------------------------ */
typedef struct mst_vit_layer {
    const float* ln1_w; const float* ln1_b;       /* block.py:63  */
    const void* qkv_w;  const float* qkv_b;       /* attention.py:50  [3E,E] compute dtype */
    const void* proj_w; const float* proj_b;      /* attention.py:52  [E,E] */
    const float* ls1;                             /* layer_scale.py:25 or NULL */
    const float* ln2_w; const float* ln2_b;       /* block.py:75  */
    const void* fc1_w;  const float* fc1_b;       /* mlp.py:28  [4E,E] */
    const void* fc2_w;  const float* fc2_b;       /* mlp.py:30  [E,4E] */
    const float* ls2;
    /* Optional fused-LayerNorm form (16-bit modes, E = 384, calls of MST_FUSED_MIN_TOKENS tokens and more): the encoder runs
     * normalise -> QKV(qkv_wf, qkv_bf) -> attention -> one of three fused tails, the first in the order below whose fields are
     * non-NULL on EVERY layer; with none complete it runs the unfused kernels on the fields above.
     *   every fused tail: qkv_wf = qkv_w * ln1_w (columns), qkv_bf = qkv_b + qkv_w . ln1_b             (norm1 folded)
     *                     fc1_bf = fc1_b + fc1_w . ln2_b, fc2_bf = ls2 * fc2_b                   (norm2 and ls2 folded)
     *   single-role block (mst_block_fused_s, ABI 300): block_seq, proj_bf; fc1_bf of [1536]
     *   producer/consumer block (mst_block_fused):      mlp_pack, proj_pack, proj_bf; fc1_bf of [1536+32]
     *   proj, then the fused MLP (mst_mlp_fused):       mlp_pack; fc1_bf of [1536+32] */
    const void* qkv_wf; const float* qkv_bf;
    const void* mlp_pack; const float* fc1_bf; const float* fc2_bf;   /* mlp_pack: the last two tails */
    const void* proj_pack; const float* proj_bf;                      /* proj_pack: the producer/consumer block; proj_bf: both blocks */
    const void* block_seq;                                            /* the single-role block */
    /* Optional FP8 form (mst_vit_weights.fp8_linear): the four block weights as e4m3 bytes, same [out,in] layout, with their
     * per-tensor scales w8_scale[] = max|W|/448 in the order qkv, proj, fc1, fc2 (see mst_gemm_fp8) */
    const void* qkv_w8; const void* proj_w8; const void* fc1_w8; const void* fc2_w8;
    float w8_scale[4];
} mst_vit_layer;

typedef struct mst_vit_weights {
    int embed_dim, depth, num_heads, num_registers;
    int compute_dtype;            /* MST_F16 / MST_BF16 / MST_F32 */
    int grid_h, grid_w;           /* patch grid pos_patch was prepared for */
    const void* patch_w;          /* [E][224] compute dtype (f32 mode: f32) */
    const float* patch_b;         /* [E] */
    const float* prefix;          /* [1+R, E] */
    const float* pos_patch;       /* [grid_h*grid_w, E] */
    const mst_vit_layer* layers;  /* [depth], host memory */
    const float* norm_w; const float* norm_b; /* vision_transformer.py:165 */
    int fp8_linear;               /* 1: the blocks' four linear layers run as mst_gemm_fp8 with dynamic per-tensor activation
                                   * scales (one per GEMM call, i.e. per chunk of slices); needs a 16-bit compute_dtype, which
                                   * stays the type of LayerNorm outputs, q/k/v and the attention kernel */
    const float* fp8_amax;        /* NULL: dynamic scales.  Else device fp32 [depth][4] = calibrated max|x| of the inputs of
                                   * qkv, proj, fc1, fc2 per block (static scales; larger values saturate at +-448 quanta): LayerNorm
                                   * and the GELU epilogue then write e4m3 directly and nothing is scanned */
    float* fp8_amax_out;          /* dynamic mode, nullable: device fp32 [depth][4], out[i] = max(out[i], this call's scales):
                                   * zero it, run representative inputs, and pass it back as fp8_amax (calibration) */
    mst_profiler* profiler;       /* nullable: time this call's launches (see mst_profiler_create) */
    int prune_last_block;         /* 0 (default): every block computes every token, as the reference does.  1: the LAST block
                                   * computes only what is read behind it -- K and V of every token (and the CLS probabilities /
                                   * full maps when asked for), then attention, out-projection and MLP of the CLS rows alone.  The
                                   * reference discards the last block's patch-token outputs (vision_transformer.py:324-329 returns
                                   * x_norm_clstoken only), so the results are the same; ignored in fp8 mode. */
    /* appended (additions only: the ABI version stays 300; a zero-initialised tail behaves as before) */
    int ffn_kind;                 /* MST_FFN_MLP (0): fc1 [4E, E] + GELU + fc2 [E, 4E].  MST_FFN_SWIGLU (1): SwiGLUFFNFused
                                   * (swiglu_ffn.py:54-72) -- every layer's fc1_w / fc1_b carry the row-paired w12 image [2 ffn_hidden, E] /
                                   * [2 ffn_hidden] of MST_EPI_BIAS_SWIGLU for compute_dtype's pairing group, fc2_w / fc2_b carry
                                   * w3 zero-padded to [E, ffn_hidden] / [E]; the fused-LayerNorm packs are not read; not with fp8_linear */
    int ffn_hidden;               /* ffn_kind 1: Hp, the hidden width padded to a multiple of 64 (<= 4E) */
} mst_vit_weights;

/* DinoVisionTransformer.forward on n_slices gray slices (vision_transformer.py:254-270,324-329;
 * block.py:89-114) -> normalised CLS embeddings cls_out fp32 [n_slices, E].
 * cls_probs (nullable) fp32 [n_layers_probs, n_slices, heads, N]: CLS-row softmax of the LAST
 * n_layers_probs blocks (1 is all the reference consumes: dino.py:190; depth reproduces the
 * whole `attention_maps` list, CLS rows only).
 * full_probs (nullable) fp32 [n_layers_probs, n_slices, heads, N, N]: the complete softmax of the
 * same blocks -- API parity for get_attention_cls (dino.py:204-212); O(N^2) memory, off by default.
 * chunk_slices: slices processed per pass (activations of one pass stay resident in the 256 MB
 * Infinity Cache); ws must hold mst_vit_workspace_bytes(...). */
size_t mst_vit_workspace_bytes(const mst_vit_weights* w, int H, int W, int chunk_slices);
int mst_vit_encode(const mst_vit_weights* w, const void* vol, int in_dtype, int n_slices, int H, int W,
                   float* cls_out, float* cls_probs, float* full_probs, int n_layers_probs,
                   int chunk_slices, void* ws, size_t ws_bytes, mst_stream_t stream);

/* The encoder as DinoVisionTransformer offers it (vision_transformer.py:254-329: forward, forward_features,
 * get_intermediate_layers): the encoder of mst_vit_encode on grey slices OR true RGB images, with the residual stream behind
 * chosen blocks ("taps") copied out for every token.  Inference only.  (Additions only: the ABI version stays 300.)
 * in_channels 1: img [n_images, H, W] of in_dtype, the grey path of mst_vit_encode launch for launch (patch_w_rgb unused, may be
 *   NULL); with taps == NULL the results have the bits of mst_vit_encode.
 * in_channels 3: img [n_images, 3, H, W] with three distinct channels; patch_w_rgb is the full Conv2d(3, E, 14, 14) kernel in
 *   w->compute_dtype as [E][3][14][16] (columns 14, 15 of every kernel row zero: K = 588 padded to 672), 16-byte aligned.  It is
 *   an argument so that mst_vit_weights keeps its layout.  The token rows start the block pipeline exactly as the grey ones do.
 * cls_out (nullable) fp32 [n_images, E]: the normalised class tokens, as mst_vit_encode.
 * taps (nullable): for i < n_taps, out[i][image][token][:] = the residual stream behind block blocks[i] (x_prenorm of that depth)
 *   for all N = 1 + num_registers + grid_h * grid_w tokens, or with norm = 1 its encoder.norm (eps 1e-6; per row the arithmetic of
 *   mst_layernorm, so class-token rows of the last block equal cls_out bit for bit).  fp32 plain rows; nothing outside
 *   [n_taps][n_images][N][E] is written.  blocks: HOST array, strictly ascending, each in [0, depth).
 * The kernel plan is chosen as in mst_vit_encode, from the token count of the whole call: a tapped call above the fused crossover
 * stays on the fused, blocked plan (the tap reads the fp32 image layout between two block launches).  A tapped call never prunes
 * the last block, whatever prune_last_block says (the pruned block has no patch rows); fp8_linear with taps is refused.
 * Conventions of mst_vit_encode: no allocation, no synchronisation, the caller's stream, chunk_images images per pass, ws of
 * mst_vit_features_workspace_bytes(...) bytes (MST_EWORKSPACE with a message when short).  With a profiler attached the tap launches
 * are counted as "layernorm". */
typedef struct mst_vit_taps {
    int n_taps;          /* 1..depth */
    const int* blocks;   /* host array, strictly ascending, each in [0, depth) */
    int norm;            /* 1: rows pass encoder.norm */
    float* out;          /* device, fp32 [n_taps][n_images][N][E] */
} mst_vit_taps;
size_t mst_vit_features_workspace_bytes(const mst_vit_weights* w, int in_channels, int H, int W, int chunk_images);
int mst_vit_encode_features(const mst_vit_weights* w, const void* img, int in_dtype, int in_channels, int n_images,
                            int H, int W, const void* patch_w_rgb, float* cls_out, const mst_vit_taps* taps,
                            int chunk_images, void* ws, size_t ws_bytes, mst_stream_t stream);

/* Across-slice transformer + head ---------------------------------------------------------- */
typedef struct mst_fusion_weights {
    int emb_in;      /* E of the encoder */
    int emb;         /* E after the optional bottleneck (dino.py:75-78) */
    int out_ch;      /* 0 = no head (enable_linear=False, dino.py:103) */
    int fusion_type; /* mst_fusion_type (dino.py:144-157) */
    int num_heads;   /* 12 (dino.py:87) */
    const float* bottleneck_w; const float* bottleneck_b; /* [emb, emb_in] or NULL */
    const float* slice_pos_emb;                           /* [256, emb] or NULL (dino.py:82) */
    const float* cls_token;                               /* [emb] (dino.py:97) */
    const float* ln1_w; const float* ln1_b;               /* transformer_blocks.py:499 */
    const float* in_proj_w; const float* in_proj_b;       /* [3emb, emb] */
    const float* out_proj_w; const float* out_proj_b;
    const float* ln2_w; const float* ln2_b;
    const float* lin1_w; const float* lin1_b;             /* dim_feedforward = emb (dino.py:88) */
    const float* lin2_w; const float* lin2_b;
    const float* norm_w; const float* norm_b;             /* dino.py:95 */
    const float* rope_freqs;                              /* [head_dim/2] or NULL (RoPE) */
    const float* head_w; const float* head_b;             /* [out_ch, emb*] (dino.py:103) */
    const float* liere_rot;                               /* [head_dim, head_dim] from mst_liere_rotation, or NULL (LieRE) */
    int head_in;     /* columns of head_w: emb, or 32*emb for 'linear' fusion (dino.py:245).  The feature width of the call
                      * (emb*D for 'linear') must equal it, as nn.Linear would insist; 0 = unchecked */
} mst_fusion_weights;

/* dino.py:134-166 after the encoder: bottleneck, slice position embedding, CLS concat,
 * nn.TransformerEncoder(1 layer, norm_first) + final LayerNorm (transformer_blocks.py:565-587,
 * 29-318), row 0, linear head.  emb fp32 [B*D, emb_in]; key_padding_mask uint8 [B, D]
 * (1 = padded slice; NULL = none) -- the CLS column is prepended inside (dino.py:147-150).
 * features fp32 [B, F] (F = emb; emb*D for 'linear'), logits fp32 [B, out_ch] (nullable),
 * slice_probs fp32 [B, heads, 1+D, 1+D] (nullable; transformer_blocks.py:266-295).
 * Supported (head_dim = emb / num_heads, L = 1 + D) of the transformer fusion: head_dim in {4, 8, 16, 32, 64, 128}; the attention keeps
 * a head's K, V and mask in LDS, (2 L head_dim + L) * 4 bytes <= 160 KiB: L <= 317 at head_dim 64, 630 at 32.  head_dim 128 fits that up
 * to L = 159 and from there to L = 317 keeps K and the mask in LDS and reads V from global memory, so every width runs the 257 tokens
 * that slice_pos_emb (256 positions) allows.  Longer sequences return MST_EINVAL ("slice_attn: L=.. head_dim=.. does not fit LDS")
 * without launching the attention. */
size_t mst_fusion_workspace_bytes(const mst_fusion_weights* w, int B, int D);
int mst_slice_fusion(const mst_fusion_weights* w, const float* emb, int B, int D,
                     const uint8_t* key_padding_mask, float* features, float* logits,
                     float* slice_probs, void* ws, size_t ws_bytes, mst_stream_t stream);

/* Saliency read-outs: dino.py:173-202.  cls_probs_last fp32 [n, heads, N] (N = 1+R+Np),
 * slice_probs fp32 [B, sheads, 1+D, 1+D], n = B*D.  Outputs (each nullable): plane fp32
 * [n, heads, Np], slice_attn fp32 [n], maps fp32 [n, heads, Np]. */
int mst_attention_readout(const float* cls_probs_last, const float* slice_probs, int B, int D,
                          int heads, int N, int num_registers, int sheads, float* plane,
                          float* slice_attn, float* maps, mst_stream_t stream);

/* Saliency volume of `--get_attention` (scripts/main_predict.py:72-105, 147-165: what _pred_trans / run_pred do after
 * the forward of ONE volume).  mst_saliency_accumulate: lowres[D, gh, gw] (+)= head-mean of maps fp32 [D, heads, Np]
 * (the get_attention_maps() result; columns >= gh*gw ignored, l.94-96) with the axes named in flip_mask (bit 0 depth,
 * bit 1 height, bit 2 width) mirrored back -- the test-time-augmentation sum of l.147-153; slice_acc[D] (+)= slice_attn[D]
 * likewise (nullable).  accumulate = 0 overwrites.  mst_saliency_upsample: out fp32 [Dout, H, W] = scale * trilinear
 * (align_corners=False, F.interpolate at l.163) of lowres. */
int mst_saliency_accumulate(const float* maps, const float* slice_attn, int D, int heads, int gh, int gw, int Np,
                            int flip_mask, int accumulate, float* lowres, float* slice_acc, mst_stream_t stream);
int mst_saliency_upsample(const float* lowres, int D, int gh, int gw, float scale, int Dout, int H, int W, float* out,
                          mst_stream_t stream);

/* Folded test-time augmentation (scripts/main_predict.py:147-158: the identity and the flips (2,), (3,), (4,), (2,3), (2,4), (3,4),
 * (2,3,4) of one volume, predictions and saliency averaged).  The encoder is per slice, so a flip along the depth only permutes slice
 * embeddings and CLS attention rows: the eight variants need the slices of four in-plane flips.
 * mst_tta_inplane_flips: x [n, H, W] (fp32 / fp16 / bf16) -> out [4, n, H, W] of the same type, not in place: x, x mirrored along H,
 * along W, along both.  Every input row is read once and written four times in whole contiguous rows (the W mirror is reversed in LDS);
 * any W whose row fits 64 KiB, any element-aligned pointers.
 * mst_saliency_accumulate_tta: plane fp32 [4, D, heads, Np] (mst_attention_readout's `plane` of those 4*D slices, in that order) and
 * slice_attn fp32 [8, D] (its `slice_attn` of the eight fused variants in the script's order above, positions as the variant saw them)
 * -> lowres[D, gh, gw] = sum over the variants of head-mean(plane[f][d])[y_f][x_f] * slice_attn[v][r ? D-1-d : d], with f the variant's
 * in-plane flip, (y_f, x_f) mirrored as f says and r its depth flip; slice_acc[D] = the same sum of slice_attn alone (nullable).  Both
 * are overwritten, summed in the script's order by one thread per element: no atomics, identical bits at every call.  Columns >= gh*gw
 * are ignored as in mst_saliency_accumulate (l.94-96); scale by 1/8 in mst_saliency_upsample. */
int mst_tta_inplane_flips(const void* x, int dtype, int n, int H, int W, void* out, mst_stream_t stream);
int mst_saliency_accumulate_tta(const float* plane, const float* slice_attn, int D, int heads, int gh, int gw, int Np,
                                float* lowres, float* slice_acc, mst_stream_t stream);

/* LieRE rotation of the slice transformer (AttentionLiereRotator, rotary_embedding_torch.py:319-372;
 * transformer_blocks.py:350-357): vars fp32 [n_blocks, block(block-1)/2, axes_length] (the module's ParameterList
 * stacked; spacial_dims = 1) -> R fp32 [n_blocks*block, n_blocks*block], block-diagonal, R_blk = exp(A_blk) with the
 * skew generator A_blk[i][j] = sum_p p * vars[blk][tril(i,j)][p].  block <= 16.  Weight preparation: call once per
 * weight version and pass R as mst_fusion_weights.liere_rot. */
int mst_liere_rotation(const float* vars, int n_blocks, int block, int axes_length, float* R, mst_stream_t stream);

/* Attention rollout (dino.py:204-212, get_attention_cls): R = maps[L-1]; for l = L-2 .. 0: R = maps[l] @ R,
 * every map fp32 [batch, N, N] row-major (batch = n*heads), exact fp32 MFMA.  `maps` is a HOST array of
 * n_layers device pointers.  The product lands in `out`; `tmp` (same size as out) is scratch and may be NULL
 * when n_layers <= 2.  Neither may alias a map.  n_layers == 1 copies the map. */
int mst_attention_rollout(const float* const* maps, int n_layers, int64_t batch, int N, float* out,
                          float* tmp, mst_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MST_HIP_H */
