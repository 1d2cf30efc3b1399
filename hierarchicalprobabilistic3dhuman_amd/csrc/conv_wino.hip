// Winograd F(2x2, 3x3) convolution for the stride-1 3x3 layers of the ResNet-18 encoder (models/resnet.py:62-78: conv1 /
// conv2 of the BasicBlocks), fused with BatchNorm, residual and ReLU, on the fp32 MFMA pipe.
//
// Why: the encoder is bound by the fp32 MFMA rate (157 TF/s peak, 136 TF/s sustained on random data) and the direct
// implicit-GEMM kernel (conv_pad.hip) already runs at 120-131 TF/s -- the only large lever left is doing fewer
// multiplications.  F(2x2, 3x3) computes a 2x2 output tile from a 4x4 input patch with 16 multiplications per
// (cin, cout) instead of 36: 2.25 x fewer MFMA FLOPs for 62 % of the encoder's arithmetic.
//
//   V = B^T d B   (input transform, 4x4 patch d, per channel: 32 additions)
//   M_p[tile, cout] = sum_cin V_p[tile, cin] * U_p[cin, cout]        p = 16 positions: 16 independent GEMMs on the MFMA pipe
//   Y = A^T M A   (output transform: 24 additions per (tile, cout)), then scale * Y + shift (+ residual) (ReLU)
//   U = G g G^T is precomputed on the host when the weights are prepared (resnet.py).
//
// Work item = one 8 x 8 block of tiles of one image (16 x 16 output pixels, an 18 x 18 input window) x 64 output channels.
// Workgroup = 512 threads = 8 waves, two per SIMD, as 2 (column pairs pg of the sixteen positions p = 4 i + j: waves 0-3 multiply
// j = 0, 1, waves 4-7 j = 2, 3) x 2 (tile groups wm of 32) x 2 (cout groups wn of 32): a wave keeps 8 accumulators of 32x32 (128
// accumulator registers).  Two waves per SIMD because a wave alone on its SIMD issues a VALU instruction every 5 cycles at best (8
// when it depends on the previous one), two together one per 2.5 (tools/valu_dep_probe.hip), and the input transform, the fragment
// reads and the epilogue are a quarter of a layer's time.  The grid is persistent: one workgroup per CU walks its items.
// LDS plan: K = Cin is streamed in chunks of 8 channels through LDS (160 KiB: sA = 2 x 32 KiB of transformed input, sB = 2 x 32 KiB
// of transformed filters, a ring of three 10 KiB raw input windows).
// Chunk schedule: while the wave multiplies chunk c,
//   * the raw 18 x 18 x 8 window of chunk c + 3 arrives by LDS-DMA (each input pixel once per workgroup -- the 4x4 patches of
//     neighbouring tiles overlap by half -- instead of 3.2 times through per-thread loads);
//   * thread (tile, ONE channel) reads its 16 patch pixels of chunk c + 1 from that chunk's window, transforms them (32 additions)
//     and writes the 16 positions to sA;
//   * the transformed filters of chunk c + 1 (chunk-contiguous in HBM) arrive by LDS-DMA, one piece at a time: a burst of DMA
//     instructions stalls the wave at issue while the texture path works through the line requests (a window piece touches 32 lines);
//   * chunk c itself: per position 2 conflict-free ds_read_b128 and 4 MFMAs (k pairs (j, 4 + j)), the reads of the wave's next
//     position requested before the MFMAs of this one are issued.
// The chunk guards are fixed per loop (a steady state that always fetches, a drain that never does), and the peeled first chunk starts
// the accumulators from the MFMA's zero C operand (no zeroing per item).
// The one-run rule: on gfx950 an fp32 VALU instruction and an fp32 MFMA of one SIMD exclude each other and every change between a run
// of one and a run of the other costs about 40 cycles (tools/mfma_valu_ops.hip; stem_wino.hip keeps the same rule), so between the first
// and the last MFMA of a chunk a wave issues MFMAs, LDS reads and writes, DMA pieces, scalar instructions, waits and ONE run of VALU
// instructions: the input transform, with every LDS address step of the next chunk inside it (docs/wino_item_cost.md;
// tools/wino_isa_counts.py counts the runs in the compiled code).
// Item epilogue: the DMAs of the next item's first chunks are issued before it, so the output transform and the stores overlap the
// next prologue's memory latency.  The output transform needs the other column pair's s[.][2] (resp. s[.][1]): two floats per (tile,
// channel) cross through the then idle sA buffers.  What depends on the column pair, the residual or the ReLU is wave-uniform and
// chosen by branches into specialised code, never by a select per value; residual loads and stores take a scalar 64-bit row address
// and a 32-bit lane offset: a lane owns one output channel, so per output pixel a half-wave moves 128 contiguous bytes.
// Quad geometry (QUAD; 8 x 8 maps, layer4: a map has 4 x 4 tiles, a quarter of an item): the item is the maps of four consecutive
// images x 64 output channels x one slice of K.  The raw ring holds the four 8 x 8 interiors (the halo is not fetched: a patch pixel
// outside its image reads a zero pixel kept in LDS), wave (wm, kl) of the epilogue owns image 2 wm + kl, and the item writes raw
// partial sums Y (the output transform is linear: the slices are added, in slice order, by wino_splitk_epilogue_kernel).
// The activations are halo-padded NHWC frames (conv_pad.hip): every window is in bounds.
// Accuracy: the transforms use only +-1 and +-1/2 -- exact scalings; the result differs from the direct convolution by
// fp32 rounding of a different summation order (<= 1e-5 of the output scale, tests/test_gpu_net.py).
// Summation order: it depends on the layer only, never on the batch size (sharding invariance) -- the K slices
// of the quad geometry are a rule on Cin -- and every product and every sum is that of the earlier forms of this kernel, in their
// order: identical bits (tests/test_gpu_wino_item.py).  Those forms -- four waves, the eight-wave loop before the one-run rule, the
// lane-per-tile store form, the half-item experiment, the profiling ablations -- and their history are in conv_wino_dev.hip (dev
// library only); this file holds the kernel that ships and nothing else.
#include <type_traits>

#include "conv_wino.h"

namespace hps {

template <bool QUAD>
__global__ __launch_bounds__(512, 1) void conv_wino_kernel(const float* __restrict__ x, const float* __restrict__ u,
                                                           const float* __restrict__ scale, const float* __restrict__ shift,
                                                           const float* __restrict__ residual, float* __restrict__ y,
                                                           const WinoGeom g) {
    typedef __attribute__((address_space(3))) void* lptr_t;
    extern __shared__ __attribute__((aligned(16))) float smem[];     // sA[2][W_OPER] | sB[2][W_OPER] | raw[3][W_RAW]
    float* sA = smem;
    float* sB = smem + 2 * W_OPER;
    float* sR = smem + 4 * W_OPER;
    constexpr int NW = 8;                                         // waves per workgroup
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kl = lane >> 5, il = lane & 31;
    const int pg = wave >> 2;                                     // the wave's column pair of positions (j = 2 pg, 2 pg + 1)
    const int wm = (wave & 3) >> 1, wn = wave & 1;
    const int nchunks = QUAD ? g.cps : g.Cin / WK;
    constexpr int RP = QUAD ? 1 : 2;                              // raw DMA pieces per wave and chunk (quad: 8 pieces = 256 pixels; else 11)

    // ---- raw-window DMA role: piece q = wave + 8 t covers window entries e = 64 q + lane (pixel e >> 1, 16-byte half e & 1) ----
    // (entries t >= RP are never used and fold away; arrays of two make hipcc allocate the quad form's registers differently)
    unsigned r_off[3];             // byte offset of the lane's 16 bytes from the item's origin (quad: without the image term)
    int r_img[3];                  // quad: image of the item (0..3) the lane's pixel belongs to
    bool r_ok[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int e = 64 * (wave + NW * t) + lane;
        if (QUAD) {
            const int px = e >> 1;                                // [image][y][x]: 4 x 8 x 8
            r_ok[t] = t < RP;
            r_img[t] = (px >> 6) & 3;
            r_off[t] = (unsigned)((((px >> 3) & 7) * g.in_row + (px & 7) * g.Cin + (e & 1) * 4) * 4);
        } else {
            r_ok[t] = t < RP && (wave + NW * t) < W_RAW_PIECES && e < 2 * W_WIN;
            const int px = r_ok[t] ? (e >> 1) : 0;
            r_img[t] = 0;
            r_off[t] = (unsigned)(((px / 18) * g.in_row + (px % 18) * g.Cin + (e & 1) * 4) * 4);
        }
    }
    unsigned r_cur[3] = {r_off[0], r_off[1], r_off[2]};           // ... of the current item (quad: + the clamped image term)
    const unsigned lds_r0 = (unsigned)(size_t)(lptr_t)(sR);
    const unsigned lds_b0 = (unsigned)(size_t)(lptr_t)(sB);

    // ---- transform role: thread = (tile (ty, tx) = (tid >> 6, (tid >> 3) & 7), channel pair (tid & 7) >> 1, channel tid & 1 of the pair) ----
    const int ltile = tid >> 3, cp = (tid & 7) >> 1;
    const int ce = tid & 1;                                       // the thread's channel of the pair (it transforms ONE channel)
    // float offset of patch pixel (0,0) in a raw window (quad: image (ty >> 2, tx >> 2), pixel (2 ly - 1, 2 lx - 1) of its 8 x 8
    // interior -- outside the interior for edge tiles, whose edge pixels read the zero pixel instead)
    const int t_ly = (ltile >> 3) & 3, t_lx = ltile & 3;
    const int w_slot = QUAD ? (((((ltile >> 5) * 2 + ((ltile >> 2) & 1)) * 64 + (2 * t_ly - 1) * 8 + (2 * t_lx - 1)) * WK) + cp * 2 + ce)
                            : ((2 * (ltile >> 3)) * 18 + 2 * (ltile & 7)) * WK + cp * 2 + ce;
    const bool e_top = t_ly == 0, e_bot = t_ly == 3, e_left = t_lx == 0, e_right = t_lx == 3;
    constexpr int W_ZERO = 4 * 64 * WK;                           // quad: a zero pixel sits behind each slot's 256 pixels
    // quad: float offsets (from the ring's start, slot 0) of the thread's 16 patch pixels, halo pixels redirected to the zero pixel,
    // two 16-bit offsets per register.  (Sixteen separate addresses -- what hipcc made of a select at each read, hoisted out of the
    // chunk loop -- did not fit beside 256 accumulators: they went to scratch, and every patch read became a scratch reload behind
    // s_waitcnt vmcnt(0), which also drained the DMAs in flight.)
    unsigned pk_off[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (QUAD) {
        if (tid < 3 * WK) sR[(tid / WK) * W_RAW + W_ZERO + tid % WK] = 0.0f;     // a zero pixel behind the 256 pixels of every slot (visible after the first barrier of the item loop)
#pragma unroll
        for (int n = 0; n < 16; ++n) {
            const int i = n >> 2, j = n & 3;
            const bool halo = (i == 0 && e_top) || (i == 3 && e_bot) || (j == 0 && e_left) || (j == 3 && e_right);
            const unsigned off = (unsigned)(halo ? W_ZERO + cp * 2 + ce : w_slot + (i * 8 + j) * WK);
            pk_off[n >> 1] |= off << (16 * (n & 1));
        }
    }
    const int a_slot = ((cp >> 1) * 64 + ltile) * 4 + (cp & 1) * 2 + ce;                // ... of the (tile, channel) slot of position 0 in sA

    // ---- multiply role: the wave's 32 fragment rows of a position in sA / sB (k-quad kl, tile group wm resp. cout group wn); lane il reads row il ----
    // (formed HERE, the lane term added at fa0 / fb0 below: hipcc orders and allocates the whole prologue differently otherwise)
    const int fa_row = kl * 64 + wm * 32;
    const int fb_row = kl * 64 + wn * 32;

    // per-item state (wave-uniform)
    const float* x_item = nullptr;     // input window origin of the item, chunk 0
    const float* u_item = nullptr;     // transformed filters of the item's cout tile, chunk 0
    int nimg = 4;                      // quad: images of the item that exist (the last item of a batch may hold fewer)
    auto locate = [&](int item, int& ct, size_t& out_base) {
        if (QUAD) {
            const unsigned t = wino_div((unsigned)item, (unsigned)g.ksplit, g.magic_ks), ks = item - t * g.ksplit;
            const unsigned qd = wino_div(t, (unsigned)g.n_ct, g.magic_ct);
            ct = t - qd * g.n_ct;
            const int b0 = 4 * qd;
            nimg = min(4, g.B - b0);
            x_item = x + (size_t)b0 * g.in_img + (size_t)g.ipad * g.in_row + (size_t)g.ipad * g.Cin + (size_t)ks * g.cps * WK;
            u_item = u + ((size_t)ks * g.cps * g.n_ct + ct) * W_OPER;
            out_base = (size_t)ks * g.B * g.out_img + (size_t)b0 * g.out_img + (size_t)g.opad * g.out_row + (size_t)g.opad * g.Cout;
#pragma unroll
            for (int t2 = 0; t2 < RP; ++t2) r_cur[t2] = r_off[t2] + (unsigned)(min(r_img[t2], nimg - 1) * g.in_img * 4);
            return;
        }
        const unsigned blk = wino_div((unsigned)item, (unsigned)g.n_ct, g.magic_ct);
        ct = item - blk * g.n_ct;
        const unsigned b = wino_div(blk, (unsigned)g.blocks_img, g.magic_img), rem = blk - b * g.blocks_img;
        const unsigned by = wino_div(rem, (unsigned)g.blocks_x, g.magic_x), bx = rem - by * g.blocks_x;
        x_item = x + (size_t)b * g.in_img + (size_t)(16 * by + g.ipad - 1) * g.in_row + (size_t)(16 * bx + g.ipad - 1) * g.Cin;
        u_item = u + (size_t)ct * W_OPER;
        out_base = (size_t)b * g.out_img + (size_t)(16 * by + g.opad) * g.out_row + (size_t)(16 * bx + g.opad) * g.Cout;
    };
    // The first DMAs of an item (the chunk loop issues its own, one piece at a time between MFMAs)
    auto dma_raw_piece = [&](int chunk, int t) {              // window of `chunk` -> ring slot chunk % 3, piece wave + 8 t
        if (t < RP && r_ok[t]) lds_dma16(r_cur[t], x_item + chunk * WK, lds_r0 + (unsigned)((chunk % 3) * W_RAW * 4 + (wave + NW * t) * 1024));
    };
    constexpr int FP = 4;                                     // filter pieces per wave and chunk (32 pieces of 1 KiB over eight waves)
    auto dma_filter_piece = [&](int chunk, int q) {           // filters of `chunk` -> sB[chunk & 1]; wave w moves pieces FP w .. FP w + FP - 1
        lds_dma16((unsigned)((wave * FP + q) * 1024 + lane * 16), u_item + (size_t)chunk * g.n_ct * W_OPER,
                  lds_b0 + (unsigned)((chunk & 1) * W_OPER * 4 + (wave * FP + q) * 1024));
    };
    auto dma_raw = [&](int chunk) {
#pragma unroll
        for (int t = 0; t < 3; ++t) dma_raw_piece(chunk, t);
    };
    auto dma_filters = [&](int chunk) {
#pragma unroll
        for (int q = 0; q < FP; ++q) dma_filter_piece(chunk, q);
    };
    auto prologue_dma = [&]() {                               // first DMAs of an item: windows 0..2 and filters 0
        dma_filters(0);
        dma_raw(0);
        if (nchunks > 1) dma_raw(1);
        if (nchunks > 2) dma_raw(2);
    };

    int item = blockIdx.x;
    if (item >= g.items) return;
    int ct;
    size_t out_base;
    locate(item, ct, out_base);
    prologue_dma();

    // ---- the item loop ----
    typedef __attribute__((address_space(3))) float* lds_f;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) const f32x4* lds_c4;
    auto ld1 = [](unsigned addr, int byte_off) { return *(lds_f)(size_t)(addr + (unsigned)byte_off); };       // base register + immediate offset
    auto ld4 = [](unsigned addr, int byte_off) { return *(lds_c4)(size_t)(addr + (unsigned)byte_off); };
    const unsigned lds_a0 = (unsigned)(size_t)(lptr_t)(sA);
    const unsigned fa0 = lds_a0 + (unsigned)(((fa_row + il) * 4 + pg * 2 * 512) * 4);     // fragment slot of the wave's first position, buffer 0
    const unsigned fb0 = lds_b0 + (unsigned)(((fb_row + il) * 4 + pg * 2 * 512) * 4);
    const unsigned dst0 = lds_a0 + (unsigned)(a_slot * 4);
    // LDS addresses of the patch pixels in the ring slot that is read next.  They are carried from chunk to chunk and moved by a
    // scalar step INSIDE the transform's VALU run (src_pos = the slot offset they hold), so that no address is formed between MFMAs.
    // 16 x 16 blocks: two row-pair bases, the pixels at immediate offsets; quad: sixteen addresses (halo pixels point at the zero pixel).
    constexpr int NSRC = QUAD ? 16 : 2;
    unsigned src[NSRC];
#pragma unroll
    for (int n = 0; n < NSRC; ++n)
        src[n] = lds_r0 + (QUAD ? ((pk_off[n >> 1] >> (16 * (n & 1))) & 0xffffu) * 4u : (unsigned)((w_slot + n * 2 * 18 * WK) * 4));
    int src_pos = 0;
    auto step_src = [&](int step) {                       // step: wave-uniform bytes
#pragma unroll
        for (int n = 0; n < NSRC; ++n) {
            src[n] += (unsigned)step;
            asm volatile("" : "+v"(src[n]));
        }
        src_pos += step;
    };
    float d1[16];
    auto read_row = [&](int i) {                          // patch row i (four pixels, the thread's one channel)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            d1[i * 4 + j] = QUAD ? ld1(src[i * 4 + j], 0) : ld1(src[i >> 1], (((i & 1) * 18 + j) * WK) * 4);
    };
    auto transform_write = [&](int buf) {                 // V = B^T d B (t = B^T d by columns, then t B by rows), the 16 positions to sA[buf]
        unsigned dst = dst0 + (unsigned)(buf * W_OPER * 4);
        asm volatile("" : "+v"(dst));
        float t1[16];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            t1[0 * 4 + j] = d1[0 * 4 + j] - d1[2 * 4 + j];
            t1[1 * 4 + j] = d1[1 * 4 + j] + d1[2 * 4 + j];
            t1[2 * 4 + j] = d1[2 * 4 + j] - d1[1 * 4 + j];
            t1[3 * 4 + j] = d1[1 * 4 + j] - d1[3 * 4 + j];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ((lds_f)(size_t)dst)[(i * 4 + 0) * 512] = t1[i * 4 + 0] - t1[i * 4 + 2];
            ((lds_f)(size_t)dst)[(i * 4 + 1) * 512] = t1[i * 4 + 1] + t1[i * 4 + 2];
            ((lds_f)(size_t)dst)[(i * 4 + 2) * 512] = t1[i * 4 + 2] - t1[i * 4 + 1];
            ((lds_f)(size_t)dst)[(i * 4 + 3) * 512] = t1[i * 4 + 1] - t1[i * 4 + 3];
        }
    };
    const unsigned f_voff = (unsigned)(lane * 16);
    typedef std::integral_constant<bool, true> Yes;
    typedef std::integral_constant<bool, false> No;
    auto with_flag = [](bool f, auto&& fn) {
        if (f) fn(Yes());
        else fn(No());
    };

    for (;;) {
        f32x16 acc[8];                                   // acc[2 i + jj] is position 4 i + 2 pg + jj; the first chunk writes it (C operand 0)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's pieces of windows 0..2 and filters 0 (and the last stores)
        __syncthreads();                                 // ... everyone's
        step_src(-src_pos);                              // back to ring slot 0
#pragma unroll
        for (int i = 0; i < 4; ++i) read_row(i);
        transform_write(0);
        step_src(W_RAW * 4);
        __syncthreads();                                 // operand chunk 0 complete
        // One chunk.  FIRST (the peeled chunk 0): the accumulators start from the MFMA's zero C operand.  more: chunk c + 1 exists (its
        // filters are fetched, its patches read and transformed); fetch: so does window c + 3.  The item runs three loops with these
        // guards fixed at compile time -- the steady state that always fetches, two chunks that only finish chunk c + 1, the last chunk
        // -- so only the peeled chunk tests them (by scalar branches).  Between the first and the last MFMA the wave issues LDS reads,
        // DMAs, scalar work -- and ONE run of VALU instructions, the transform in position 5 with every address step in it.
        auto chunk = [&](auto FIRST_, auto MORE_, auto FETCH_, int c) {
            constexpr bool FIRST = decltype(FIRST_)::value;
            const bool more = FIRST ? c + 1 < nchunks : decltype(MORE_)::value, fetch = FIRST ? c + 3 < nchunks : decltype(FETCH_)::value;
            const int buf = c & 1;
            unsigned pa = fa0 + (unsigned)(buf * W_OPER * 4), pb = fb0 + (unsigned)(buf * W_OPER * 4);
            asm volatile("" : "+v"(pa), "+v"(pb));
            f32x4 a4[2], b4[2];
            a4[0] = ld4(pa, 0);
            b4[0] = ld4(pb, 0);
            const float* u_next = u_item + (size_t)(c + 1) * g.n_ct * W_OPER + wave * FP * 256;
            const unsigned lds_f_next = lds_b0 + (unsigned)(((c + 1) & 1) * W_OPER * 4 + wave * FP * 1024);
            const float* x_next = x_item + (c + 3) * WK;
            const unsigned lds_r_next = lds_r0 + (unsigned)((c % 3) * W_RAW * 4 + wave * 1024);          // window c + 3 takes the slot of chunk c
#pragma unroll
            for (int pp = 0; pp < 8; ++pp) {             // pp = 2 i + jj: position 4 i + 2 pg + jj (pa / pb start at position 2 pg)
                const int pnext = (4 * ((pp + 1) >> 1) + ((pp + 1) & 1)) * 512;
                if (pp < FP) {                           // filters first, then the window: the waits below count on that order
                    if (more) lds_dma16(f_voff, u_next + pp * 256, lds_f_next + (unsigned)(pp * 1024));
                } else if (pp == 5) {
                    if (fetch) lds_dma16(r_cur[0], x_next, lds_r_next);
                } else if (!QUAD && pp == 6) {
                    if (fetch && r_ok[1]) lds_dma16(r_cur[1], x_next, lds_r_next + (unsigned)(NW * 1024));
                }
                if (pp < 7) {
                    a4[(pp + 1) & 1] = ld4(pa, pnext * 4);
                    b4[(pp + 1) & 1] = ld4(pb, pnext * 4);
                }
                __builtin_amdgcn_sched_barrier(0);
                const f32x4 a = a4[pp & 1], b = b4[pp & 1];
                if (FIRST) {
                    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    acc[pp] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, zero, 0, 0, 0);
                } else {
                    acc[pp] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc[pp], 0, 0, 0);
                }
                acc[pp] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc[pp], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                // A patch row is requested in the MIDDLE of a position's MFMAs: hipcc's wait in front of the next position's MFMAs allows
                // only the two newest LDS reads to be outstanding, so a patch read issued together with the next fragments made every
                // position wait out a fresh LDS round trip.
                if (pp < 4) {
                    if (more) read_row(pp);
                } else if (pp == 5) {
                    if (more) {
                        transform_write((c + 1) & 1);
                        step_src((c + 2) % 3 == 0 ? -2 * W_RAW * 4 : W_RAW * 4);      // to the slot of chunk c + 2
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                acc[pp] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc[pp], 0, 0, 0);
                acc[pp] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc[pp], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (!more) return;
            // filters of chunk c + 1 were issued BEFORE window c + 3: with in-order returns, all but the wave's own pieces of that
            // window (needed one chunk later) must have landed.  Eleven window pieces over eight waves: waves 0-2 move two, the
            // others one (quad: eight pieces, one each).
            if (fetch) {
                if (!QUAD && wave < 3) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
            } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();                             // operand chunk c + 1 complete; sA / sB [buf] and ring slot (c + 1) % 3 are free
        };
        chunk(Yes(), No(), No(), 0);
        int c = 1;
        for (; c + 3 < nchunks; ++c) chunk(No(), Yes(), Yes(), c);
        for (; c + 1 < nchunks; ++c) chunk(No(), Yes(), No(), c);
        if (c < nchunks) chunk(No(), No(), No(), c);

        // ---- the next item's first DMAs go out before this item's epilogue (which touches no LDS but the exchange in sA) ----
        const int cur_ct = ct, cur_nimg = nimg;
        const size_t cur_out = out_base;
        const int next = item + gridDim.x;
        __syncthreads();                                 // everyone is done with this item's LDS
        if (next < g.items) {
            locate(next, ct, out_base);
            prologue_dma();
        }

        // ---- output transform Y = A^T M A (A^T = [1 1 1 0; 0 1 -1 -1]), BatchNorm, residual, ReLU.  A lane owns one output channel (MFMA
        //      column) and 16 tiles (MFMA rows).  The row transform s = A^T M is formed for the wave's two columns jj; the column transform
        //      needs ONE column of the other pair: y(a, 0) = (s_a[0] + s_a[1]) + s_a[2] is formed by the waves of columns 0-1 with s_a[2]
        //      from their partners, y(a, 1) = (s_a[1] - s_a[2]) - s_a[3] by the waves of columns 2-3 with s_a[1].  The exchange runs through
        //      sA (idle: the next item's first DMAs fill sB[0] and the raw ring).  Addresses: a wave-uniform 64-bit base per output row
        //      and four 32-bit lane offsets (one per tile column) ----
        const int co_w = cur_ct * WC + wn * 32;
        const size_t wave_base = (QUAD ? cur_out + (size_t)(2 * wm) * g.out_img : cur_out + (size_t)(8 * wm) * g.out_row) + co_w + (size_t)pg * g.Cout;
        unsigned col_off[4];                             // bytes: the lane's channel (and tile-column half kl; quad: image kl) + tile column
#pragma unroll
        for (int j = 0; j < 4; ++j) col_off[j] = (unsigned)(((QUAD ? kl * g.out_img : kl * 8 * g.Cout) + il + 2 * j * g.Cout) * 4);
        const size_t row_bytes = (size_t)g.out_row * 4;
        const bool store_ok = !QUAD || 2 * wm + kl < cur_nimg;
        float2* xch = reinterpret_cast<float2*>(sA);
        float k0[2][16], k1[2][16];                      // s_0[jj], s_1[jj] of the wave's columns, per tile register r
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                k0[jj][r] = acc[0 + jj][r] + acc[2 + jj][r] + acc[4 + jj][r];
                k1[jj][r] = acc[2 + jj][r] - acc[4 + jj][r] - acc[6 + jj][r];
            }
        const int w4 = wave & 3;
        typedef __attribute__((address_space(1))) char gchar;          // global address space, stated: it does not survive the pin below otherwise
        typedef __attribute__((address_space(1))) float gfloat;
        auto lane_ptr = [&](gchar* row, int j) {         // row + the lane's 32-bit offset, extended HERE: scalar base + 32-bit lane offset
            asm volatile("" : "+v"(col_off[j]));         // is an addressing mode only when the extension is in sight of the access
            return (gfloat*)(row + (size_t)col_off[j]);
        };
        auto row_ptr = [&](const float* base, int row) { // wave-uniform address of the wave's output row `row`, pinned in scalar registers
            gchar* p = (gchar*)(base + wave_base) + (size_t)row * row_bytes;
            asm volatile("" : "+s"(p));
            return p;
        };
        // Everything that depends on the wave's column pair, the residual or the ReLU is wave-uniform: chosen by branches into
        // specialised code, never by a select per value (each arm has its own s_barrier for the exchange; every wave passes one).
        with_flag(pg != 0, [&](auto PG1) {
            constexpr bool P1 = decltype(PG1)::value;
            constexpr int jx = P1 ? 0 : 1;               // columns 0-1 export column 1, columns 2-3 export column 2 (their jj = 0)
#pragma unroll
            for (int r = 0; r < 16; ++r) xch[(((P1 ? 1 : 0) * 16 + r) * 4 + w4) * 64 + lane] = make_float2(k0[jx][r], k1[jx][r]);
            float sc = 0.f, sh = 0.f;
            float res[16][2];
            if (!QUAD) {
                sc = scale[co_w + il];
                sh = shift[co_w + il];
                if (residual) {
#pragma unroll
                    for (int row = 0; row < 8; ++row) {
                        gchar* rp = row_ptr(residual, row);
#pragma unroll
                        for (int j = 0; j < 4; ++j) res[4 * (row >> 1) + j][row & 1] = *lane_ptr(rp, j);
                    }
                }
            }
            __syncthreads();
            auto finish = [&](auto RES_, auto RELU_) {
                constexpr bool RES = decltype(RES_)::value, RELU = decltype(RELU_)::value;
#pragma unroll
                for (int i = 0; i < 4; ++i) {            // tile row i of the wave's four: registers r = 4 i + j, output rows 2 i + a
                    float out[4][2];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int r = 4 * i + j;
                        const float2 o = xch[(((P1 ? 0 : 1) * 16 + r) * 4 + w4) * 64 + lane];
                        if (!P1) {                       // y(a, 0) = (s_a[0] + s_a[1]) + s_a[2]
                            out[j][0] = k0[0][r] + k0[1][r] + o.x;
                            out[j][1] = k1[0][r] + k1[1][r] + o.y;
                        } else {                         // y(a, 1) = (s_a[1] - s_a[2]) - s_a[3]
                            out[j][0] = o.x - k0[0][r] - k0[1][r];
                            out[j][1] = o.y - k1[0][r] - k1[1][r];
                        }
#pragma unroll
                        for (int a = 0; a < 2; ++a) {
                            float v = out[j][a];
                            if (!QUAD) {                 // (the quad geometry writes raw partial sums: g.raw)
                                v = v * sc + sh;
                                if (RES) v += res[r][a];
                                if (RELU) v = fmaxf(v, 0.0f);
                            }
                            out[j][a] = v;
                        }
                    }
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        gchar* yp = row_ptr(y, 2 * i + a);
#pragma unroll
                        for (int j = 0; j < 4; ++j) *lane_ptr(yp, j) = out[j][a];
                    }
                }
            };
            if (store_ok) {
                if constexpr (QUAD) finish(No(), No());
                else with_flag(residual != nullptr, [&](auto RES_) { with_flag(g.relu != 0, [&](auto RELU_) { finish(RES_, RELU_); }); });
            }
        });
        if (next >= g.items) return;
        item = next;
    }
}

// second pass of the quad geometry: y = act(scale * (sum of the K slices, in slice order) + shift + residual) into the padded
// 8 x 8 output frames; thread per four channels
__global__ __launch_bounds__(256) void wino_splitk_epilogue_kernel(const float* __restrict__ partial, const float* __restrict__ scale,
                                                                   const float* __restrict__ shift, const float* __restrict__ residual,
                                                                   float* __restrict__ y, int total4, int ksplit, int Cout, int opad,
                                                                   int relu) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    float4 acc = reinterpret_cast<const float4*>(partial)[i];
    for (int k = 1; k < ksplit; ++k) {
        const float4 v = reinterpret_cast<const float4*>(partial)[(size_t)k * total4 + i];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    const unsigned e = (unsigned)i * 4u;
    const unsigned m = e / (unsigned)Cout, co = e - m * Cout;               // m = (image * 8 + row) * 8 + column
    const unsigned b = m >> 6, py = (m >> 3) & 7, px = m & 7, fw = 8 + 2 * opad;
    const size_t o = ((size_t)(b * fw + py + opad) * fw + px + opad) * Cout + co;
    const float4 sc = *reinterpret_cast<const float4*>(scale + co), sh = *reinterpret_cast<const float4*>(shift + co);
    float4 v = make_float4(acc.x * sc.x + sh.x, acc.y * sc.y + sh.y, acc.z * sc.z + sh.z, acc.w * sc.w + sh.w);
    if (residual) {
        const float4 r = *reinterpret_cast<const float4*>(residual + o);
        v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
    }
    if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    *reinterpret_cast<float4*>(y + o) = v;
}

// K slices of the quad geometry: a rule on the layer only (never on the batch: the summation order of a pixel must not change
// with B).  Four slices when each still has >= 8 chunks (layer4: 64 chunks -> 4 x 16), else one.
#ifdef HPS_DEV_BUILD
int g_wino_quad_ks = 0;                  // dev library only (hps_dev_wino_quad_ksplit in conv_wino_dev.hip): 0 = the product rule
#else
constexpr int g_wino_quad_ks = 0;
#endif
int wino_quad_ksplit(int Cin) {
    if (g_wino_quad_ks > 0 && (Cin / WK) % g_wino_quad_ks == 0) return g_wino_quad_ks;
    return (Cin / WK) % 4 == 0 && (Cin / WK) / 4 >= 8 ? 4 : 1;
}

int wino_sum_slices(const float* splitk_ws, const float* scale, const float* shift, const float* residual, float* y, int B, int ksplit,
                    int Cout, int opad, int relu, hps_stream_t stream) {
    const int total4 = B * 64 * Cout / 4;
    hipLaunchKernelGGL(wino_splitk_epilogue_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, splitk_ws,
                       scale, shift, residual, y, total4, ksplit, Cout, opad, relu);
    return check_launch("hps_conv3x3_winograd (slices)");
}

template <bool QUAD>
static int wino_launch_geom(const float* x, const float* u, const float* scale, const float* shift, const float* residual, float* y,
                            const WinoGeom& g, hps_stream_t stream, int grid_cap) {
    // persistent grid: one workgroup per CU (256 on MI355X), items strided over the workgroups
    const int max_wgs = grid_cap > 0 && grid_cap < 256 ? grid_cap : 256;
    const dim3 grid((unsigned)(g.items < max_wgs ? g.items : max_wgs));
    const int rc = grant_lds<&conv_wino_kernel<QUAD>>(160 * 1024, "hps_conv3x3_winograd");
    if (rc != HPS_OK) return rc;
    hipLaunchKernelGGL((conv_wino_kernel<QUAD>), grid, dim3(512), W_LDS_BYTES, (hipStream_t)stream, x, u, scale, shift, residual, y, g);
    return check_launch("hps_conv3x3_winograd");
}

int wino_launch(const float* x, const float* u, const float* scale, const float* shift, const float* residual, float* y, int B, int H, int W,
                int ipad, int Cin, int Cout, int opad, int relu, float* splitk_ws, hps_stream_t stream, int grid_cap) {
    WinoGeom g;
    int rc = wino_geom(g, x, u, scale, shift, y, B, H, W, ipad, Cin, Cout, opad, relu, splitk_ws);
    if (rc != HPS_OK || g.items == 0) return rc;
    if (!g.raw) return wino_launch_geom<false>(x, u, scale, shift, residual, y, g, stream, grid_cap);
    // quad geometry: raw partial sums into the workspace, then the second pass
    if ((rc = wino_launch_geom<true>(x, u, scale, shift, nullptr, splitk_ws, g, stream, grid_cap)) != HPS_OK) return rc;
    return wino_sum_slices(splitk_ws, scale, shift, residual, y, B, g.ksplit, Cout, opad, relu, stream);
}

}  // namespace hps

using namespace hps;

extern "C" size_t hps_conv3x3_winograd_workspace(int B, int H, int W, int Cin, int Cout) {
    if (H != 8 || W != 8 || B <= 0 || Cin <= 0 || Cout <= 0) return 0;
    return (size_t)wino_quad_ksplit(Cin) * B * 64 * Cout * sizeof(float);
}

extern "C" int hps_conv3x3_winograd(const float* x, const float* u, const float* scale, const float* shift, const float* residual,
                                    float* y, int B, int H, int W, int ipad, int Cin, int Cout, int opad, int relu,
                                    float* splitk_ws, hps_stream_t stream) {
    return wino_launch(x, u, scale, shift, residual, y, B, H, W, ipad, Cin, Cout, opad, relu, splitk_ws, stream, 0);
}

