// Everything of a ViT block after the attention kernel, for E = 384 and 16-bit MFMA operands, in ONE launch -- the
// SINGLE-ROLE form (round 3; k_block16.hip is the producer/consumer form it replaces):
//     x  <- x + ls1 * (proj(attn_out) + b_proj)                       attention.py:67-68; block.py:90-91,112
//     x  <- x + ls2 * (fc2(gelu(fc1(LayerNorm2(x)))) + b2)            block.py:93-94,113; mlp.py:34-40
//     xn <- normalise(x)      (optional: the NEXT block's norm1, its affine folded into that block's QKV weights)
//
// Structure: persistent, one 4-wave workgroup per CU = ONE wave per SIMD with the whole 512-register file, 128 token rows per
// tile, every wave owns 32 rows end to end.  Everything a row needs stays in the registers of the lane pair (l, l+32) that owns it:
//   * y^T accumulators [384 features x 32 rows] = 12 tiles of the 32x32x16 MFMA (192 registers); the residual x rides inside;
//   * the out-projection's B operand (attention-output rows) is loaded from global memory straight into fragment registers;
//   * LayerNorm2 runs on the accumulators and leaves the normalised rows as 24 B fragments (96 registers): a 32x32 accumulator
//     tile IS the next MFMA's B operand after a pairwise 16-bit pack (k order permuted; the weight images are packed to match);
//   * per hidden chunk of 32 units: GEMM1 (24 MFMAs) -> GELU in registers -> the same lane-private pack -> GEMM2 (24 MFMAs).
// No hand-off of activations through LDS or global memory exists at all (k_block16.hip: a 16 KiB LDS hand-off per chunk and a
// 96 KiB global scratch per tile), and no wave waits for another one except at the ring barrier.
//
// Weights: every 24 KiB weight image (12 out-projection chunks, 48 W1 chunks, 48 W2 chunks) is ONE element of a single stream
// packed on the host in consumption order (108 elements per tile, [24 fragments][64 lanes][16 B] each: a fragment read is a
// conflict-free ds_read_b128 at lane*16).  The stream runs through a 6-slot LDS ring by LDS-DMA four elements ahead; a "phase"
// consumes one element in 24 slots of [fragment read 6 ahead | counted lgkmcnt | MFMA | a few vector instructions of the GELU
// of a neighbouring chunk], with one s_barrier per phase.  Fragment reads run across the phase boundaries (the barrier of phase e
// also publishes element e + 1), so the LDS latency never surfaces.  A tile consumes 108 = 18 x 6 elements: the ring slot of every
// phase is a compile-time constant, and the MLP loop is rolled over one ring period (12 phases; profiles/NOTES_block_mlp_loop.md).
// The twelve out-projection elements are fetched from that stream in another order, (accumulator tile pair, K half)-major, so that
// pair P is first touched in phase 2P: the finished rows of the previous tile leave, and this tile's x arrives, pair by pair from
// inside those phases, and only pair 0 and the attention rows stand between two tiles (see "row traffic" below).
#include <type_traits>

#include "mst_common.h"

namespace {

constexpr int E = 384, HID = 1536, CH = 32;
constexpr int NCHUNK = HID / CH;                        // 48
constexpr int PJ = E / CH;                              // 12 out-projection phases
constexpr int ELEM_BYTES = 24 * 1024;                   // one ring element: 24 fragments of 1 KiB
constexpr int ELEMS = PJ + 2 * NCHUNK;                  // 108 per tile
constexpr int NSLOT = 6;
constexpr int AHEAD = 4;                                // phase e issues the LDS-DMA of element e + 4
constexpr int RING_BYTES = NSLOT * ELEM_BYTES;          // 147,456
constexpr int B1_OFF = RING_BYTES;                      // fp32 b1f [1536]
constexpr int BP_OFF = B1_OFF + HID * 4;                // fp32 b_proj [384]  (ls1 folded)
constexpr int B2_OFF = BP_OFF + E * 4;                  // fp32 b2     [384]  (ls2 folded)
constexpr int LDS_BYTES = B2_OFF + E * 4;               // 156,672
constexpr int NF = 24;                                  // fragments (= MFMAs) per phase
constexpr int BLOCKS_DEPTH = 4;
constexpr int D = BLOCKS_DEPTH;                         // fragment reads in flight ahead of the MFMAs
// Register sets of the fragment ring: D + 2, not D + 1.  The read issued in slot i must not target the set MFMA i-1 took its A
// operand from: that MFMA is still executing, and the in-order wave then stalls AT THE READ until it has finished (write-after-read
// on its source registers) -- measured 44 instead of 32 cycles per slot with D + 1 sets (profiles/r04b_*).
constexpr int R = D + 2;
static_assert(NF % R == 0, "fragment ring must tile the phase");
// Slot i of an out-projection / GEMM2 phase takes fragment FRAG(i) = (tile t = i % 12, k-step p = i / 12): consecutive MFMAs go to
// DIFFERENT accumulator tiles.  A dependent 32x32x16 MFMA (same accumulator as its predecessor) issued 48 cycles after it, an
// independent one 32 (stamps: 48.5 cycles per slot in the GEMM1 chain, 44 with dependent pairs; profiles/r04b_*).
constexpr int frag_of(int i) { return 2 * (i % 12) + i / 12; }
// Out-projection phases consume the stream pair-major: ring element (P, H) holds, for accumulator tiles 2P and 2P + 1, the K-chunks
// j = 6H .. 6H + 5 as fragment n = 4 (j - 6H) + 2 (t - 2P) + p.  Slot i takes tile 2P + i % 2 and k-step i / 2 of the twelve
// (j, p) in ascending order: the two tiles alternate (a tile's own MFMAs are 64 cycles apart) and every accumulator element sees the
// summation order of the chunk-major walk.
constexpr int pair_frag_of(int i) { return 4 * (i / 4) + 2 * (i % 2) + (i / 2) % 2; }
constexpr int ORD_STREAM = 0, ORD_TILE = 1, ORD_PAIR = 2;
constexpr int frag_in_order(int i, int ord) { return ord == ORD_PAIR ? pair_frag_of(i) : ord == ORD_TILE ? frag_of(i) : i; }
constexpr int BIAS_SLOT = 8;                            // slot of a phase in which the next chunk's b1 is read

template <int OFF, typename V> __device__ __forceinline__ void lds_read_b128(V& dst, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(OFF));
}
// b1 of a chunk goes into quarter Q of the sixteen registers the chunk's GEMM1 accumulates in.  The registers are named: left to
// choose, hipcc put the four quarters of a chunk into registers that do not form one MFMA accumulator and moved them there at the
// head of the GEMM1 phase (76 v_accvgpr moves per twelve phases of the rolled MLP loop, 16 with the names).
template <int OFF, int Q, int HS> __device__ __forceinline__ void lds_read_b128_hq(f32x4& dst, unsigned addr) {
    if constexpr (HS == 0 && Q == 0) asm volatile("ds_read_b128 %0, %1 offset:%2" : "={a[192:195]}"(dst) : "v"(addr), "i"(OFF));
    if constexpr (HS == 0 && Q == 1) asm volatile("ds_read_b128 %0, %1 offset:%2" : "={a[196:199]}"(dst) : "v"(addr), "i"(OFF));
    if constexpr (HS == 0 && Q == 2) asm volatile("ds_read_b128 %0, %1 offset:%2" : "={a[200:203]}"(dst) : "v"(addr), "i"(OFF));
    if constexpr (HS == 0 && Q == 3) asm volatile("ds_read_b128 %0, %1 offset:%2" : "={a[204:207]}"(dst) : "v"(addr), "i"(OFF));
    if constexpr (HS == 1 && Q == 0) asm volatile("ds_read_b128 %0, %1 offset:%2" : "={a[208:211]}"(dst) : "v"(addr), "i"(OFF));
    if constexpr (HS == 1 && Q == 1) asm volatile("ds_read_b128 %0, %1 offset:%2" : "={a[212:215]}"(dst) : "v"(addr), "i"(OFF));
    if constexpr (HS == 1 && Q == 2) asm volatile("ds_read_b128 %0, %1 offset:%2" : "={a[216:219]}"(dst) : "v"(addr), "i"(OFF));
    if constexpr (HS == 1 && Q == 3) asm volatile("ds_read_b128 %0, %1 offset:%2" : "={a[220:223]}"(dst) : "v"(addr), "i"(OFF));
}
template <int N> __device__ __forceinline__ void wait_lgkm() {       // + fence: no MFMA above the wait (rule 18)
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N));
    __builtin_amdgcn_sched_barrier(0);
}
#ifdef BLOCKS_STAMPS
// diagnostic build only (never shipped): per-wave cycle sums by phase kind, read back by mst_debug_blocks_stamps
__device__ unsigned long long g_bsstamps[256 * 4 * 16];
__device__ __forceinline__ unsigned long long bstamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define BST(var) const unsigned long long var = bstamp()
#define BACC(slot, a, b) st[slot] += (b) - (a)
#else
#define BST(var)
#define BACC(slot, a, b)
#endif

template <int I, int N, typename F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

__device__ __forceinline__ f32x16 cat16(f32x4 a, f32x4 b, f32x4 c, f32x4 d) {
    typedef __attribute__((ext_vector_type(8))) float f32x8;
    const f32x8 lo = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7), hi = __builtin_shufflevector(c, d, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
}
template <int Q> __device__ __forceinline__ f32x4 sub4(f32x16 v) { return __builtin_shufflevector(v, v, 4 * Q, 4 * Q + 1, 4 * Q + 2, 4 * Q + 3); }

// ---- GELU as a list of micro-operations (one VALU / transcendental instruction each), so that a phase can spread the GELU of
// eight values over its MFMA slots.  Value v, scratch a, b; after the last stage `a` holds gelu(v).  Forms: mst_common.h gelu_sig.
template <typename T> struct Gelu;
template <> struct Gelu<bf16_t> {
    static constexpr int STAGES = 7;
    static constexpr int target(int) { return 0; }       // scratch register a stage writes (0 = a, 1 = b, 2 = c)
    template <int S> static __device__ __forceinline__ void stage(float v, float& a, float& b, float& c) {
        if constexpr (S == 0) a = v * v;
        else if constexpr (S == 1) a = fmaf(a, -0.06940179f * 1.4426950408889634f, -1.60031416f * 1.4426950408889634f);
        else if constexpr (S == 2) a = v * a;
        else if constexpr (S == 3) a = __builtin_amdgcn_exp2f(a);
        else if constexpr (S == 4) a = 1.0f + a;
        else if constexpr (S == 5) a = __builtin_amdgcn_rcpf(a);
        else a = v * a;
    }
};
template <> struct Gelu<f16_t> {
    static constexpr int STAGES = 9;
    static constexpr int target(int S) { return S == 0 ? 1 : (S == 2 || S == 3) ? 2 : 0; }
    template <int S> static __device__ __forceinline__ void stage(float v, float& a, float& b, float& c) {
        if constexpr (S == 0) b = __builtin_amdgcn_fmed3f(v, -8.0f, 8.0f);       // the quadratic P turns over at |v| = 8.35
        else if constexpr (S == 1) a = b * b;
        else if constexpr (S == 2) c = fmaf(a, 7.03033577e-04f * 1.4426950408889634f, -7.40112920e-02f * 1.4426950408889634f);
        else if constexpr (S == 3) c = fmaf(c, a, -1.59501577f * 1.4426950408889634f);
        else if constexpr (S == 4) a = b * c;
        else if constexpr (S == 5) a = __builtin_amdgcn_exp2f(a);
        else if constexpr (S == 6) a = 1.0f + a;
        else if constexpr (S == 7) a = __builtin_amdgcn_rcpf(a);
        else a = v * a;
    }
};

template <typename T>
__global__ __launch_bounds__(256) void block16s_kernel(float* x, const T* attn, T* xn_out, const char* __restrict__ wseq,
                                                       const float* __restrict__ b1f, const float* __restrict__ bproj,
                                                       const float* __restrict__ b2, int M, int ntiles, float eps, int layout) {
    typedef typename V8<T>::type vec8;
    typedef typename V8<T>::half_type vec4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const bool x_in_img = layout & MST_LAYOUT_X_IN_IMAGE, x_out_img = layout & MST_LAYOUT_X_OUT_IMAGE, act_blk = layout & MST_LAYOUT_ACT_BLOCKED;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row32 = lane & 31, half = lane >> 5;
    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned lane16 = lane * 16;

    const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    if (my_tiles <= 0) return;

    // ---- biases -> LDS (once per workgroup)
    for (int i = tid; i < HID / 4; i += 256) *reinterpret_cast<f32x4*>(smem + B1_OFF + i * 16) = *reinterpret_cast<const f32x4*>(b1f + 4 * i);
    for (int i = tid; i < E / 4; i += 256) {
        *reinterpret_cast<f32x4*>(smem + BP_OFF + i * 16) = *reinterpret_cast<const f32x4*>(bproj + 4 * i);
        *reinterpret_cast<f32x4*>(smem + B2_OFF + i * 16) = *reinterpret_cast<const f32x4*>(b2 + 4 * i);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");          // (the first phase barrier publishes them)

    // ---- weight stream.  Element ge (global index over this workgroup's tiles) = stream element ge % 108 -> ring slot ge % 6;
    // this wave's share: the six consecutive 1 KiB pieces 6 wave .. 6 wave + 5 (one lane address, one M0, six immediates).
    // The stream simply wraps: the four elements issued beyond the last tile land in slots nobody reads (drained before exit).
    // buffer form: the piece base rides in soffset (SGPR), the lane part is ONE 32-bit VGPR: half the address traffic per issue
    // (the descriptor starts at the wave's share, so the lane part is the lane address the fragment reads use as well)
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(wseq + wave * 6144), 0, ELEMS * ELEM_BYTES - wave * 6144, 0x00020000);
    char* const wdst_wave = smem + wave * 6144;
    // (the ring slot is a constant of the call site everywhere: M0 is the wave's base plus an immediate)
    auto dma_piece = [&](int src_off, auto slot_tag, auto u_tag) {
        constexpr int u = decltype(u_tag)::value, slot = decltype(slot_tag)::value;
        // (the 12-bit immediate moves the source AND the LDS address: pieces 4 and 5 take a second base 4 KiB further on both sides)
        constexpr int hi = u >= 4 ? 4096 : 0;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(wrsrc, LDS_PTR(wdst_wave + slot * ELEM_BYTES + hi), 16, (int)lane16, src_off + hi, u * 1024 - hi, 0);
    };
    // Out-projection element (P, H) is gathered from the unchanged stream: piece n = 6 wave + u of the ring element is fragment
    // (4P + n % 4) of stream element 6H + n / 4.  Same lane address form, the per-piece source offset rides in an SGPR.
    int pair_piece_off[6];
#pragma unroll
    for (int u = 0; u < 6; ++u) {
        const int n = 6 * wave + u;
        pair_piece_off[u] = (n >> 2) * ELEM_BYTES + (n & 3) * 1024 - (u >= 4 ? u * 1024 - 4096 : u * 1024) - wave * 6144;   // (>= 0)
    }
    auto dma_pair_piece = [&](auto pe_tag, auto slot_tag, auto u_tag) {
        constexpr int u = decltype(u_tag)::value, pe = decltype(pe_tag)::value, hi = u >= 4 ? 4096 : 0, slot = decltype(slot_tag)::value;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(wrsrc, LDS_PTR(wdst_wave + slot * ELEM_BYTES + hi), 16, (int)lane16,
                                                 pair_piece_off[u] + ((pe & 1) * 6 * ELEM_BYTES + (pe >> 1) * 4096), u * 1024 - hi, 0);
    };
    static_for<0, AHEAD>([&](auto e0) { static_for<0, 6>([&](auto u) { dma_pair_piece(e0, e0, u); }); });

    f32x16 acc[12];
    u32x4 xa[24];                                        // out-projection: attention-output fragments; MLP: normalised rows
    f32x4 hq[2][4];                                      // hidden pre-activations of two chunks in flight, as register quarters
    vec8 hB[2][2];                                       // [chunk parity][k-step]: GELU outputs as GEMM2 B fragments
    vec8 w[R];                                           // weight fragment ring
    float ga[8], gb[8], gc[8];                           // GELU scratch of the eight values in flight

    // Ring schedule: a tile consumes ELEMS = 18 NSLOT elements, so every tile starts at ring slot 0 and element e of a tile lies in
    // slot e % 6 whatever the tile: the slot a phase reads, the next one (tail prefetch) and the one it requests (four ahead) are
    // constants of the call site.  A fragment read is then one of three lane bases (64 KiB of ds_read offset reach two slots) plus an
    // immediate; nothing of the ring lives in scalar registers except the stream offset inside the rolled MLP loop.
    static_assert(ELEMS % NSLOT == 0, "every tile must start at ring slot 0");
    static_assert(ELEM_BYTES + (NF - 1) * 1024 < 65536, "two slots per lane base must fit the 16-bit ds_read offset");
    const unsigned ring0 = lds_base + lane16;
    unsigned b1v = 0;                                    // LDS address of b1 (lane part included) of the chunk the MLP loop trip starts at
    // LDS addresses of the bias tables: lane part + a wave-uniform offset, added where they are used (volatile: kept as loop
    // invariants, the handful of variants beyond the 16-bit instruction offset were spilled around the tile boundary)
    auto bias_addr = [&](unsigned uniform_off) {          // uniform_off + 16 * (lane >> 5)
        unsigned a;
        asm volatile("v_lshrrev_b32 %0, 5, %2\n\tv_and_b32 %0, 16, %0\n\tv_add_u32 %0, %1, %0" : "=&v"(a) : "s"(lds_base + uniform_off), "v"(lane16));
        return a;
    };
    // value + the value of the lane 32 further on / back (the two lanes that share a row): one v_permlane32_swap, no lane-address register
    auto add_other_half = [](float v) {
        const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
        const unsigned own = sw[0], other = sw[1];       // (as scalars first: a bit_cast of a vector element reads element 0)
        return __builtin_bit_cast(float, own) + __builtin_bit_cast(float, other);
    };

    // ---- one phase: 24 slots over the element in ring slot SLOT (prefetching the head of the next element), MFMA `mf(i, fragment)`,
    // vector filler `fill(i)`; BQ >= 0: the b1 of a chunk, at b1v + BOFF, is read INTO hq[BQ] (dead at that point), where the GEMM1
    // of that chunk accumulates on top of it a phase later.
#ifdef BLOCKS_STAMPS
    unsigned long long st[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned long long tstart = bstamp();
#endif
    // ord_tag / nord_tag: how this / the next phase walks its fragments (ORD_STREAM: GEMM1 k-steps, ORD_TILE: frag_of, ORD_PAIR:
    // pair_frag_of).  dma_tag: the element requested here (four ahead) is out-projection element 0..11 of the pair-major walk, or
    // -1 = the next one of the stream as it lies.  rows_tag: row loads issued in the two phases before this one (below).
    // slot_tag: the ring slot of the element consumed.  boff_tag: byte offset of the b1 read from b1v.  src: stream byte offset of
    // the element requested (dma_tag = STREAM only).
    auto phase = [&](auto slot_tag, auto head_tag, auto tail_tag, auto bq_tag, auto boff_tag, auto&& mf, auto&& fill, auto cat_tag, auto ord_tag,
                     auto nord_tag, auto dma_tag, int src, auto rows_tag) {
        constexpr int SLOT = decltype(slot_tag)::value, NXT = (SLOT + 1) % NSLOT, BOFF = decltype(boff_tag)::value;
        constexpr std::integral_constant<int, (SLOT + AHEAD) % NSLOT> DSLOT{};
        constexpr int CUR_IMM = (SLOT % 2) * ELEM_BYTES, NXT_IMM = (NXT % 2) * ELEM_BYTES;
        constexpr bool HEAD = decltype(head_tag)::value, TAIL = decltype(tail_tag)::value;
        constexpr int ORD = decltype(ord_tag)::value, NORD = decltype(nord_tag)::value, DMA_PE = decltype(dma_tag)::value;
        auto fr = [](int i, int ord) constexpr { return frag_in_order(i, ord); };
        constexpr int BQ = decltype(bq_tag)::value, CAT = decltype(cat_tag)::value;
        BST(p0);
        // element ge landed for everybody at the previous barrier; this one publishes ge + 1: own pieces first (all but the 12
        // youngest vector-memory operations done: the pieces of ge + 2 and ge + 3 may stay in flight).  The counter is shared with the
        // row traffic and retires in order, so the row LOADS issued since the last piece of ge + 1 are counted on top; the row stores
        // between them are conditional and are left out, which only makes the wait reach a little further back.
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(12 + decltype(rows_tag)::value) : "memory");
        BST(p1);
        BACC(CAT, p0, p1);
        const unsigned cur = ring0 + (SLOT / 2) * 2 * ELEM_BYTES, nxt = ring0 + (NXT / 2) * 2 * ELEM_BYTES;
        f32x4 bt0, bt1, bt2, bt3;
        if constexpr (HEAD) static_for<0, D>([&](auto q) { lds_read_b128<CUR_IMM + fr(decltype(q)::value, ORD) * 1024>(w[decltype(q)::value % R], cur); });
        static_for<0, NF>([&](auto it) {
            constexpr int i = decltype(it)::value;
            if constexpr (i + D < NF) lds_read_b128<CUR_IMM + fr(i + D, ORD) * 1024>(w[(i + D) % R], cur);
            else if constexpr (TAIL) lds_read_b128<NXT_IMM + fr(i + D - NF, NORD) * 1024>(w[(i + D) % R], nxt);
            if constexpr (BQ >= 0 && i == BIAS_SLOT) {
                lds_read_b128_hq<BOFF, 0, BQ>(bt0, b1v);
                lds_read_b128_hq<BOFF + 32, 1, BQ>(bt1, b1v);
                lds_read_b128_hq<BOFF + 64, 2, BQ>(bt2, b1v);
                lds_read_b128_hq<BOFF + 96, 3, BQ>(bt3, b1v);
            }
            // ONE counted wait per two slots: at an even slot fragments i and i + 1 have landed once only the reads behind
            // fragment i + 1 are outstanding (fragments i + 2 .. last issued, plus the four b1 reads where they are younger).
            // A wait in every slot measured 1 % more kernel time (1.074 vs 1.062 ms in the bench pipeline).
            if constexpr (i % 2 == 0) {
                constexpr int last = TAIL ? i + D : (i + D < NF - 1 ? i + D : NF - 1);
                constexpr int younger_frags = last - (i + 1) > 0 ? last - (i + 1) : 0;
                constexpr int younger_bias = (BQ >= 0 && i >= BIAS_SLOT && i + 1 <= BIAS_SLOT + D) ? 4 : 0;
                wait_lgkm<younger_frags + younger_bias>();
            } else {
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (BQ >= 0 && i == BIAS_SLOT + D + 1) {
                // this slot's counted wait covers the four b1 reads: only now do the values exist for hipcc (an asm output it may
                // copy at once -- it moved the in-flight registers into the accumulator file right behind the reads otherwise)
                asm volatile("" : "+a"(bt0), "+a"(bt1), "+a"(bt2), "+a"(bt3));
                hq[BQ < 0 ? 0 : BQ][0] = bt0;
                hq[BQ < 0 ? 0 : BQ][1] = bt1;
                hq[BQ < 0 ? 0 : BQ][2] = bt2;
                hq[BQ < 0 ? 0 : BQ][3] = bt3;
            }
            mf(it, w[i % R]);
            if constexpr (i % 4 == 3) {
                if constexpr (DMA_PE >= 0) dma_pair_piece(dma_tag, DSLOT, std::integral_constant<int, i / 4>{});
                else dma_piece(src, DSLOT, std::integral_constant<int, i / 4>{});
            }
            fill(it);
        });
        BST(p2);
        BACC(CAT + 1, p1, p2);
    };
    constexpr std::integral_constant<int, 0> C_PROJ{};
    constexpr std::integral_constant<int, 2> C_A{};
    constexpr std::integral_constant<int, 4> C_B{};
    constexpr std::integral_constant<int, 6> C_G10{};
    auto no_fill = [](auto) {};
    constexpr std::true_type YES{};
    constexpr std::false_type NO{};
    constexpr std::integral_constant<int, -1> NOBIAS{};
    constexpr std::integral_constant<int, 0> I0{};
    constexpr std::integral_constant<int, 1> I1{};
    constexpr std::integral_constant<int, 2> I2{};
    constexpr std::integral_constant<int, 3> I3{};
    constexpr std::integral_constant<int, -1> STREAM{};  // dma_tag: the next element of the stream
    constexpr std::integral_constant<int, 0> ROWS0{};    // rows_tag: no row loads in flight behind the ring

    // GEMM1 of one chunk into hq[HS] (which holds the chunk's b1): 24 dependent MFMAs on one 32x32 accumulator
    auto gemm1_mf = [&](auto hs_tag) {
        return [&](auto it, const vec8& wf) {
            constexpr int hs = decltype(hs_tag)::value, i = decltype(it)::value;
            f32x16 c = cat16(hq[hs][0], hq[hs][1], hq[hs][2], hq[hs][3]);
            c = mfma32(wf, __builtin_bit_cast(vec8, xa[i]), c);
            static_for<0, 4>([&](auto q) { hq[hs][decltype(q)::value] = sub4<decltype(q)::value>(c); });
        };
    };
    auto gemm2_mf = [&](auto hs_tag) {
        return [&](auto it, const vec8& wf) {
            constexpr int hs = decltype(hs_tag)::value, i = frag_of(decltype(it)::value);
            acc[i >> 1] = mfma32(wf, hB[hs][i & 1], acc[i >> 1]);
        };
    };

    // ---- GELU of eight values (registers 8 PART .. 8 PART + 7 of chunk buffer hs) -> hB[hs][PART], as micro-operations
    constexpr int GOPS = 8 * Gelu<T>::STAGES + 4;        // + 4 pairwise packs
    auto gelu_op = [&](auto hs_tag, auto part_tag, auto n_tag) {
        constexpr int hs = decltype(hs_tag)::value, PART = decltype(part_tag)::value, n = decltype(n_tag)::value;
        if constexpr (n < 8 * Gelu<T>::STAGES) {
            constexpr int grp = n / (4 * Gelu<T>::STAGES), m = n % (4 * Gelu<T>::STAGES);
            constexpr int st = m / 4, val = 4 * grp + m % 4;
            Gelu<T>::template stage<st>(hq[hs][2 * PART + (val >> 2)][val & 3], ga[val], gb[val], gc[val]);
            // pinned: without an ordered user hipcc gathers the whole list at the head of the phase
            if constexpr (Gelu<T>::target(st) == 0) asm volatile("" : "+v"(ga[val]));
            else if constexpr (Gelu<T>::target(st) == 1) asm volatile("" : "+v"(gb[val]));
            else asm volatile("" : "+v"(gc[val]));
        } else if constexpr (n < GOPS) {
            constexpr int pr = n - 8 * Gelu<T>::STAGES;  // values 2 pr, 2 pr + 1 -> elements 2 pr, 2 pr + 1 of the fragment
            hB[hs][PART][2 * pr] = (T)ga[2 * pr];
            hB[hs][PART][2 * pr + 1] = (T)ga[2 * pr + 1];
        }
    };
    constexpr int OPS_PER_SLOT = (GOPS + NF - 2) / (NF - 1);          // slots 1..23 carry the filler
    auto gelu_fill = [&](auto hs_tag, auto part_tag) {
        return [&, hs_tag, part_tag](auto it) {
            constexpr int i = decltype(it)::value;
            if constexpr (i >= 1)
                static_for<0, OPS_PER_SLOT>([&](auto o) { gelu_op(hs_tag, part_tag, std::integral_constant<int, (i - 1) * OPS_PER_SLOT + decltype(o)::value>{}); });
        };
    };
    auto gelu_now = [&](auto hs_tag, auto part_tag) { static_for<0, GOPS>([&](auto n) { gelu_op(hs_tag, part_tag, n); }); };

    // ---- row traffic.  Blocked / image layouts (include/mst_hip.h): every instruction moves one contiguous KiB; row-major: lane =
    // row, 32 scattered 32-byte runs per instruction (what the first and the last block of an encoder still see).
    // The out-projection needs accumulator pair P (tiles 2P, 2P + 1) from its phase 2P on, so only pair 0 and the attention rows
    // stand between two tiles: the finished pair P >= 1 of the previous tile is stored, and its registers are refilled with this
    // tile's x, from inside out-projection phase 2P - 2, one instruction per MFMA slot (576 KB per workgroup in one burst with the
    // matrix pipe idle otherwise: 28 k cycles of a 185 k-cycle tile, profiles/block_boundary_stamps_parent.txt).
    // Aliasing (xn_out may be the attention buffer; x in place with differing in / out layouts): a 32-row group belongs to ONE wave
    // of ONE tile.  That wave requests the group's attention rows before phase 0 and the last of its x in phase 8, and phase 10
    // cannot start before those loads have returned (the counter retires in order and every phase waits on it), while the first
    // store to the group is issued behind the tile's last phase: a group is still read whole before it is written.
    const int last_grp = (M - 1) >> 5;
    // The lane parts of the row addresses are derived again at every tile boundary from a copy of the lane address hipcc cannot
    // see through: as loop invariants they would occupy registers across the MLP phases, where none is to spare.
    auto lane16_here = [&]() {
        unsigned l;
        asm volatile("v_mov_b32 %0, %1" : "=v"(l) : "v"(lane16));
        return l;
    };
    auto row_of = [&](int tile) {
        int wave_row;                                    // (an SGPR by force: hipcc kept a vector copy of it across the tile, and spilled it)
        asm volatile("s_lshl_b32 %0, %1, 5" : "=s"(wave_row) : "s"(wave));
        const int g = tile * 128 + wave_row + (int)((lane16_here() >> 4) & 31);
        return (unsigned)(g < M ? g : M - 1);
    };
    auto grp_of = [&](int tile) { return (size_t)((tile * 4 + wave) < last_grp ? (tile * 4 + wave) : last_grp); };
    // Row x traffic is addressed from the wave-uniform base (SGPRs) of the 48 KiB block of the wave's 32 rows, the lane part in ONE
    // VGPR and the (tile t, quarter q) part added where it is used: 32 (4t + q) bytes row-major, 32 times that in the image layout.
    // (volatile: hoisted out of the tile loop, the 72 + 48 offsets of a tile were what hipcc spilled)
    auto row_off = [](int lane_part, auto units_tag, int shift) {
        int off;
        asm volatile("v_lshl_add_u32 %0, %1, %2, %3" : "=v"(off) : "n"(decltype(units_tag)::value), "s"(shift), "v"(lane_part));
        return off;
    };
    const int xin_sh = x_in_img ? 10 : 5, att_sh = act_blk ? 10 : 5;
    const char* in_x;
    int xin_lane;
    auto row_in_grp = [&](int tile) { return (int)(row_of(tile) - (unsigned)grp_of(tile) * 32u); };   // (clamped: every lane reads rows that exist)
    auto x_in_of = [&](int tile) {
        in_x = (const char*)x + grp_of(tile) * (32 * E * 4);
        const unsigned l16 = lane16_here();
        xin_lane = x_in_img ? (int)l16 : row_in_grp(tile) * (E * 4) + (int)((l16 >> 5) & 16);
    };
    auto load_attn = [&](int tile) {                     // fragment i: 1 KiB apart in the blocked layout, 32 bytes of the row otherwise
        const char* const ap = (const char*)attn + grp_of(tile) * (32 * E * 2);
        const unsigned l16 = lane16_here();
        const int lane_part = act_blk ? (int)l16 : row_in_grp(tile) * (E * 2) + (int)((l16 >> 5) & 16);
        static_for<0, 24>([&](auto i) {
            xa[decltype(i)::value] = *reinterpret_cast<const u32x4*>(ap + (unsigned)row_off(lane_part, i, att_sh));
        });
    };
    auto load_x = [&](auto t_tag, auto q_tag) {          // quarter q of accumulator tile t of the wave's 32 rows
        constexpr int t = decltype(t_tag)::value, q = decltype(q_tag)::value;
        const f32x4 v = *reinterpret_cast<const f32x4*>(in_x + (unsigned)row_off(xin_lane, std::integral_constant<int, 4 * t + q>{}, xin_sh));
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][4 * q + r] = v[r];
    };
    // The output rows of the tile whose accumulators are being stored (the previous tile while the out-projection runs).  A wave's 32
    // rows are one contiguous block in every layout, so the stores go through a buffer descriptor over exactly the bytes of that
    // block that exist: rows past M (row-major) and groups past the last one are dropped by the range check, without a branch in the
    // phases, and the descriptors (SGPRs) are all that is carried from one tile to the next.  Zero records = nothing to store yet /
    // no xn_out.  (offsets go through the VGPR operand alone: that is the part the range check sees)
    const int xout_sh = x_out_img ? 10 : 5, xn_sh = act_blk ? 10 : 5;
    int xout_lane = 0, xn_lane = 0;
    auto out_lanes = [&]() {
        const unsigned l16 = lane16_here();
        const int r32 = (l16 >> 4) & 31, h16 = (l16 >> 5) & 16;
        xout_lane = x_out_img ? (int)l16 : r32 * (E * 4) + h16;
        xn_lane = act_blk ? (int)l16 : r32 * (E * 2) + h16;
    };
    auto rows_rsrc = [&](void* base, int tile, int row_bytes, bool whole_groups) {
        const int grp = tile * 4 + wave, rows = M - grp * 32;                 // wave-uniform
        const int nrows = rows <= 0 || !base ? 0 : (rows > 32 || whole_groups) ? 32 : rows;
        return __builtin_amdgcn_make_buffer_rsrc((char*)base + (size_t)grp * (32 * row_bytes), 0, nrows * row_bytes, 0x00020000);
    };
    __amdgpu_buffer_rsrc_t out_x = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, 0, 0x00020000), out_n = out_x;
    float out_rstd = 0.f, out_nmr = 0.f;                 // LayerNorm statistics of those rows
    auto store_x = [&](auto t_tag, auto q_tag) {
        constexpr int t = decltype(t_tag)::value, q = decltype(q_tag)::value;
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc[t][4 * q + r];
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), out_x, row_off(xout_lane, std::integral_constant<int, 4 * t + q>{}, xout_sh), 0, 0);
    };
    auto store_n = [&](auto t_tag, auto p_tag) {
        constexpr int t = decltype(t_tag)::value, p = decltype(p_tag)::value;
        // registers 8p..8p+3 = features 32t + 16p + 4 half + 0..3, registers 8p+4..8p+7 = the same + 8: one
        // v_permlane32_swap per register pair hands each lane eight CONSECUTIVE features (T21)
        // (scalar fused multiply-adds: the statistics stay two registers per lane from one tile into the next)
        vec4 lo, hi;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            // (rounded to fp32 first, then to 16 bits, as the vector form this replaces: no fused v_fma_mix with its single rounding)
            float n0 = fmaf(acc[t][8 * p + e], out_rstd, out_nmr), n1 = fmaf(acc[t][8 * p + 4 + e], out_rstd, out_nmr);
            asm volatile("" : "+v"(n0), "+v"(n1));
            lo[e] = (T)n0;
            hi[e] = (T)n1;
        }
        const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
        u32x4 o;
#pragma unroll
        for (int d2 = 0; d2 < 2; ++d2) {
            const auto sw = __builtin_amdgcn_permlane32_swap(l2[d2], h2[d2], false, false);
            o[d2] = sw[0];
            o[2 + d2] = sw[1];
        }
        __builtin_amdgcn_raw_buffer_store_b128(o, out_n, row_off(xn_lane, std::integral_constant<int, 2 * t + p>{}, xn_sh), 0, 0);
    };
    // the 20 row operations of accumulator pair P as one per slot: 12 stores (per tile 4 x quarters + 2 normalised fragments), then
    // the 8 loads that refill the same registers
    auto pair_op = [&](auto p_tag, auto n_tag) {
        constexpr int P = decltype(p_tag)::value, n = decltype(n_tag)::value;
        if constexpr (n < 12) {
            constexpr int t = 2 * P + n / 6, m = n % 6;
            if constexpr (m < 4) store_x(std::integral_constant<int, t>{}, std::integral_constant<int, m>{});
            else store_n(std::integral_constant<int, t>{}, std::integral_constant<int, m - 4>{});
        } else if constexpr (n < 20) {
            load_x(std::integral_constant<int, 2 * P + (n - 12) / 4>{}, std::integral_constant<int, (n - 12) % 4>{});
        }
    };
    constexpr int PAIR_LOADS = 8, HEAD_LOADS = 24 + PAIR_LOADS;      // row loads per pair; in front of phase 0: attention rows + pair 0
    // (The workgroups are not de-phased any more: with 70 % of the row traffic under the out-projection a start-up stagger that
    // spreads the boundaries over the tile period measured 0.1 ms per step SLOWER than none, profiles/NOTES_block_boundary.md.)
    load_attn(blockIdx.x);
    x_in_of(blockIdx.x);
    static_for<12, 20>([&](auto n) { pair_op(I0, n); });

    for (int k = 0; k < my_tiles; ++k) {
        const int tile = blockIdx.x + k * gridDim.x;
        // ---- out-projection: 12 phases (pair P, K half H), acc[2P + i % 2] += Wp fragments . attention columns; the even phases
        // 0..8 carry the row traffic of pair P + 1
        static_for<0, PJ>([&](auto et) {
            constexpr int e = decltype(et)::value, P = e / 2, H = e % 2;
            auto mf = [&](auto it, const vec8& wf) {
                constexpr int i = decltype(it)::value;
                acc[2 * P + i % 2] = mfma32(wf, __builtin_bit_cast(vec8, xa[12 * H + i / 2]), acc[2 * P + i % 2]);
            };
            auto fill = [&](auto it) {
                if constexpr (H == 0 && P + 1 < 6) pair_op(std::integral_constant<int, P + 1>{}, it);
            };
            // row loads issued behind the last piece of element e + 1 (that piece went out at the end of phase e - 3)
            constexpr int rows = e == 0 ? HEAD_LOADS : e == 1 ? HEAD_LOADS + PAIR_LOADS : e <= 10 ? PAIR_LOADS : 0;
            constexpr std::integral_constant<int, rows> ROWS{};
            constexpr std::integral_constant<int, (e + AHEAD < PJ ? e + AHEAD : -1)> DMA{};
            constexpr std::integral_constant<int, e % NSLOT> SLOT{};
            constexpr int src = (e + AHEAD) * ELEM_BYTES;                     // (elements 12..15: the first of the stream as it lies)
            if constexpr (e == 0) phase(SLOT, YES, YES, NOBIAS, I0, mf, fill, C_PROJ, I2, I2, DMA, src, ROWS);
            else if constexpr (e == PJ - 1) phase(SLOT, NO, NO, NOBIAS, I0, mf, fill, C_PROJ, I2, I2, DMA, src, ROWS);   // no prefetch across LayerNorm2
            else phase(SLOT, NO, YES, NOBIAS, I0, mf, fill, C_PROJ, I2, I2, DMA, src, ROWS);
        });
        BST(q2);
        // ---- LayerNorm2 on the accumulators (+ b_proj first), normalised rows -> xa, then + b2.  Vector-typed arithmetic on
        // purpose (v_pk_* at the boundary, where no MFMA competes for the issue port); the file is built with -fno-slp-vectorize.
        {
            // (no fragment read is in flight here: asm outputs that have not landed must not live across code hipcc schedules by
            // itself -- under LayerNorm2's register pressure it copied them into the accumulator file right behind the reads)
            const unsigned bp = bias_addr(BP_OFF), bb = bias_addr(B2_OFF);
            f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
            static_for<0, 12>([&](auto tt) {
                constexpr int t = decltype(tt)::value;
                f32x4 b[4];
                static_for<0, 4>([&](auto q) { lds_read_b128<128 * t + 32 * decltype(q)::value>(b[decltype(q)::value], bp); });
                wait_lgkm<0>();
                acc[t] += cat16(b[0], b[1], b[2], b[3]);
                s4 += (sub4<0>(acc[t]) + sub4<1>(acc[t])) + (sub4<2>(acc[t]) + sub4<3>(acc[t]));
                asm volatile("" : "+v"(s4));
            });
            float sum = (s4[0] + s4[1]) + (s4[2] + s4[3]);
            sum = add_other_half(sum);
            const float mean = sum * (1.0f / E);
            const f32x4 mean4 = {mean, mean, mean, mean};
            f32x4 q4 = {0.f, 0.f, 0.f, 0.f};
            static_for<0, 12>([&](auto tt) {
                constexpr int t = decltype(tt)::value;
                static_for<0, 4>([&](auto q) {
                    const f32x4 d = sub4<decltype(q)::value>(acc[t]) - mean4;
                    q4 = __builtin_elementwise_fma(d, d, q4);
                });
                asm volatile("" : "+v"(q4));
            });
            float sq = (q4[0] + q4[1]) + (q4[2] + q4[3]);
            sq = add_other_half(sq);
            const float rstd = rsqrtf(sq * (1.0f / E) + eps);
            const float nmr = -mean * rstd;
            const f32x4 rstd4 = {rstd, rstd, rstd, rstd}, nmr4 = {nmr, nmr, nmr, nmr};
            static_for<0, 12>([&](auto tt) {
                constexpr int t = decltype(tt)::value;
                f32x4 b[4];
                static_for<0, 4>([&](auto q) { lds_read_b128<128 * t + 32 * decltype(q)::value>(b[decltype(q)::value], bb); });
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const f32x4 n0 = __builtin_elementwise_fma(p ? sub4<2>(acc[t]) : sub4<0>(acc[t]), rstd4, nmr4);
                    const f32x4 n1 = __builtin_elementwise_fma(p ? sub4<3>(acc[t]) : sub4<1>(acc[t]), rstd4, nmr4);
                    vec8 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { o[e] = (T)n0[e]; o[4 + e] = (T)n1[e]; }
                    xa[2 * t + p] = __builtin_bit_cast(u32x4, o);
                    asm volatile("" : "+v"(xa[2 * t + p]));
                }
                wait_lgkm<0>();
                acc[t] += cat16(b[0], b[1], b[2], b[3]);
            });
        }
        BST(q3);
        BACC(9, q2, q3);
        // ---- b1 of chunk 0 -> hq[0] (behind LayerNorm2: sixteen more registers across it were sixteen spilled ones)
        {
            b1v = bias_addr(B1_OFF);
            f32x4 bt[4];
            static_for<0, 4>([&](auto q) { lds_read_b128_hq<32 * decltype(q)::value, decltype(q)::value, 0>(bt[decltype(q)::value], b1v); });
            wait_lgkm<0>();
            asm volatile("" : "+a"(bt[0]), "+a"(bt[1]), "+a"(bt[2]), "+a"(bt[3]));     // (only now do the values exist for hipcc)
            static_for<0, 4>([&](auto q) { hq[0][decltype(q)::value] = bt[decltype(q)::value]; });
        }
        // ---- GEMM1 of chunk 0 = element 12, slot 0 (b1 of chunk 1 -> hq[1]), then the first half of its GELU
        phase(I0, YES, YES, I1, std::integral_constant<int, 128>{}, gemm1_mf(I0), no_fill, C_G10, I0, I0, STREAM, (PJ + AHEAD) * ELEM_BYTES, ROWS0);
        wait_lgkm<0>();
        gelu_now(I0, I0);
        // ---- chunks: A(c) = GEMM1(c + 1) beside the second half of GELU(c); B(c) = GEMM2(c) beside the first half of GELU(c + 1)
        // (+ b1 of chunk c + 2 into the buffer GELU(c) has just left).  A(c) consumes element 13 + 2c, B(c) element 14 + 2c: the
        // slots repeat every three chunks and the buffer parity every two, so chunk c = c0 + j of a six-chunk group starting at c0
        // (a multiple of six) has everything but its stream offset and its b1 base as constants of j.  The last four phases of a
        // tile request the first four out-projection elements of the next one (dma_a / dma_b).
        auto iter = [&](auto j_tag, auto bias_tag, int src_a, auto dma_a, auto dma_b) {
            constexpr int j = decltype(j_tag)::value, cur = j & 1, nx = cur ^ 1;
            constexpr std::integral_constant<int, (PJ + 1 + 2 * j) % NSLOT> SA{};
            constexpr std::integral_constant<int, (PJ + 2 + 2 * j) % NSLOT> SB{};
            constexpr std::integral_constant<int, 128 * (j + 2)> BOFF{};
            phase(SA, NO, YES, NOBIAS, I0, gemm1_mf(std::integral_constant<int, nx>{}), gelu_fill(std::integral_constant<int, cur>{}, I1), C_A, I0, I1, dma_a, src_a, ROWS0);
            if constexpr (decltype(bias_tag)::value)
                phase(SB, NO, YES, std::integral_constant<int, cur>{}, BOFF, gemm2_mf(std::integral_constant<int, cur>{}), gelu_fill(std::integral_constant<int, nx>{}, I0), C_B, I1, I0, dma_b, src_a + ELEM_BYTES, ROWS0);
            else                                         // chunk 46: the next phase is GEMM2(47)
                phase(SB, NO, YES, NOBIAS, I0, gemm2_mf(std::integral_constant<int, cur>{}), gelu_fill(std::integral_constant<int, nx>{}, I0), C_B, I1, I1, dma_b, src_a + ELEM_BYTES, ROWS0);
        };
        constexpr int GROUP = 6, TRIPS = NCHUNK / GROUP - 1;                 // rolled body = one ring period = 12 phases; chunks 0 .. 41
        static_assert(GROUP % (NSLOT / 2) == 0 && GROUP % 2 == 0 && (TRIPS + 1) * GROUP == NCHUNK, "the peeled tail below is chunks 42 .. 47");
        constexpr int SRC0 = (PJ + 1 + AHEAD) * ELEM_BYTES;                  // A(0) requests element 17
        int msrc = SRC0;
#pragma unroll 1
        for (int trip = 0; trip < TRIPS; ++trip) {
            static_for<0, GROUP>([&](auto j) { iter(j, YES, msrc + 2 * decltype(j)::value * ELEM_BYTES, STREAM, STREAM); });
            msrc += 2 * GROUP * ELEM_BYTES;
            b1v += 128 * GROUP;
        }
        constexpr int C0 = TRIPS * GROUP;                // 42: b1v stands at its b1
        auto src_of = [](int c) constexpr { return SRC0 + 2 * c * ELEM_BYTES; };
        iter(I0, YES, src_of(C0), STREAM, STREAM);        // chunk 42
        iter(I1, YES, src_of(C0 + 1), STREAM, STREAM);    // chunk 43
        iter(I2, YES, src_of(C0 + 2), STREAM, STREAM);    // chunk 44
        iter(I3, YES, src_of(C0 + 3), STREAM, I0);        // chunk 45: A requests element 107, the last of the tile
        iter(std::integral_constant<int, 4>{}, NO, 0, I1, I2);            // chunk 46
        wait_lgkm<0>();
        gelu_now(I1, I1);
        phase(std::integral_constant<int, (ELEMS - 1) % NSLOT>{}, NO, NO, NOBIAS, I0, gemm2_mf(I1), no_fill, C_B, I1, I1, I3, 0, ROWS0);   // GEMM2 of chunk 47
        // ---- tile boundary: the next block's LayerNorm statistics (they need all twelve tiles), pair 0 out, the next tile's
        // attention rows and pair 0 in.  Pairs 1..5 leave from inside the next out-projection, or behind the loop.
        BST(q4);
        {
            // (last tile: its own rows once more, unused -- a load under a condition makes hipcc wait for it at the join)
            const int next_tile = k + 1 < my_tiles ? tile + (int)gridDim.x : tile;
            load_attn(next_tile);                                        // xa is dead since the last GEMM1
            if (xn_out) {
                f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
                static_for<0, 12>([&](auto tt) {
                    constexpr int t = decltype(tt)::value;
                    s4 += (sub4<0>(acc[t]) + sub4<1>(acc[t])) + (sub4<2>(acc[t]) + sub4<3>(acc[t]));
                    asm volatile("" : "+v"(s4));
                    __builtin_amdgcn_sched_barrier(0);
                });
                float sum = (s4[0] + s4[1]) + (s4[2] + s4[3]);
                sum = add_other_half(sum);
                const float mean = sum * (1.0f / E);
                const f32x4 mean4 = {mean, mean, mean, mean};
                f32x4 q4 = {0.f, 0.f, 0.f, 0.f};
                static_for<0, 12>([&](auto tt) {
                    constexpr int t = decltype(tt)::value;
                    static_for<0, 4>([&](auto q) {
                        const f32x4 d = sub4<decltype(q)::value>(acc[t]) - mean4;
                        q4 = __builtin_elementwise_fma(d, d, q4);
                    });
                    asm volatile("" : "+v"(q4));
                    __builtin_amdgcn_sched_barrier(0);
                });
                float sq = (q4[0] + q4[1]) + (q4[2] + q4[3]);
                sq = add_other_half(sq);
                out_rstd = rsqrtf(sq * (1.0f / E) + eps);
                out_nmr = -mean * out_rstd;
            }
            out_lanes();
            out_x = rows_rsrc(x, tile, E * 4, x_out_img);
            out_n = rows_rsrc(xn_out, tile, E * 2, act_blk);
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, 12>([&](auto n) { pair_op(I0, n); });
            __builtin_amdgcn_sched_barrier(0);
            x_in_of(next_tile);
            static_for<12, 20>([&](auto n) { pair_op(I0, n); });
            __builtin_amdgcn_sched_barrier(0);
        }
        BST(q5);
        BACC(10, q4, q5);
    }
    // ---- the last tile's pairs 1..5
    BST(q6);
    static_for<1, 6>([&](auto P) { static_for<0, 12>([&](auto n) { pair_op(P, n); }); });
    BST(q7);
    BACC(11, q6, q7);
#ifdef BLOCKS_STAMPS
    st[15] = bstamp() - tstart;
    if (lane == 0) for (int i = 0; i < 16; ++i) g_bsstamps[(blockIdx.x * 4 + wave) * 16 + i] = st[i];
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the run-ahead LDS-DMA must not outlive the workgroup's LDS allocation
}

template <typename T>
int launch_t(float* x, const void* attn, void* xn_out, const void* wseq, const float* b1f, const float* bproj, const float* b2,
             int64_t M, float eps, int layout, hipStream_t s) {
    static mst_lds_once lds_once;
    auto kern = block16s_kernel<T>;
    mst_allow_lds((const void*)kern, LDS_BYTES, &lds_once);
    const int ntiles = (int)((M + 127) / 128);
    const int cus = mst_persistent_grid();
    const int nblk = ntiles < cus ? ntiles : cus;
    kern<<<dim3(nblk), dim3(256), LDS_BYTES, s>>>(x, (const T*)attn, (T*)xn_out, (const char*)wseq, b1f, bproj, b2, (int)M, ntiles, eps, layout);
    return mst_check_launch("block16s");
}

}  // namespace

#ifdef BLOCKS_STAMPS
extern "C" int mst_debug_blocks_stamps(unsigned long long* host, int n) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_bsstamps), sizeof(unsigned long long) * n);
}
#endif

int launch_block16s(float* x, const void* attn, void* xn_out, int dt, const void* wseq, const float* b1f, const float* bproj,
                    const float* b2, int64_t M, int E_, float eps, int layout, hipStream_t s) {
    MST_CHECK_ARG(E_ == E, "block_fused_s: embed_dim=%d unsupported (384)", E_);
    MST_CHECK_ARG(M > 0 && M < (1ll << 31) - 128, "block_fused_s: bad M");
    if (dt == MST_BF16) return launch_t<bf16_t>(x, attn, xn_out, wseq, b1f, bproj, b2, M, eps, layout, s);
    if (dt == MST_F16) return launch_t<f16_t>(x, attn, xn_out, wseq, b1f, bproj, b2, M, eps, layout, s);
    mst_set_error("block_fused_s: dtype %d unsupported (f16 / bf16)", dt);
    return MST_EINVAL;
}
