// The profiling ablations of the Winograd stem kernel (dev library only; include/hps_dev.h: hps_dev_stem_winograd and
// hps_dev_stem_winograd_pooled_nchw).  The kernel that ships is stem_wino_kernel in stem_wino.hip -- read that file for what the
// kernel does and why; stem_wino_ablate_kernel below is a COPY of it, as it stood when the two were split, with a compile-time
// ablation number AB threaded through the input transform, the MFMA run, the gather and the barriers, so that the product can move
// without it.  Every form but 7 computes garbage: they price a part of the kernel by leaving it out.
//
//   AB   form             what is left out or changed                                                        record
//    1   plain            patch pixels not read (constants)                                                  profiles/r03_ablations.txt
//    2   plain            no MFMAs
//    3   plain            no output transform
//    4   plain            no barriers (races)
//    5   plain            no filter fragment reads
//    6   plain            no stores (both epilogues skipped, results kept alive)
//    7   plain            each channel pair as two 4-byte LDS reads (identical results)                      docs/experiments_r1-r5.md
//    8   pooled, NCHW     no gather loads                                                                    docs/experiments_r6.md, section 6
//    9   pooled, NCHW     no window stores
//   10   pooled, NCHW     the wn = 1 waves skip the input transform
//   11   pooled, NCHW     ... and read their 45 operands from LDS behind a second barrier per row
//   12   pooled, NCHW     the transform split between the waves of a channel-half pair, no exchange
//   13   pooled, NCHW     ... + 23 LDS stores, 23 LDS reads per lane and row and a second barrier
// plain = stem_wino_ablate_kernel<AB, false, false> on phase frames, pooled NCHW = <AB, true, true>.  ablate = 0 is not here: the dev
// entries hand it to stem_wino.hip's launcher.
#include "stem_wino.h"

namespace hps {

template <int AB>
__device__ __forceinline__ f32x16 sw_mfma(float a, float b, f32x16 c) {
    if (AB == 2) {
        c[0] += a * b;
        return c;
    }
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// Input transform of one row of positions (see the header): A[j][m] = the lane's channel 2 m + kl of position j, m = 0..8.
// rawp: this lane's patch origin in the raw window (its channel pairs), raws: the channels 16, 17 of that pixel (odd: the lane
// keeps 17).  NXP: positions of the row, NE: window rows in its vertical combination.
// AB: the ablation (table above): 1 = patch pixels not read (constants), 2 = no MFMAs, 3 = no output transform, 4 = no barriers (races),
// 5 = no filter fragment reads, 6 = no stores
// G0, G1 (profiling, AB = 12 / 13): only the channel groups [G0, G1) are transformed, the other operands stay constants
template <int NXP, int NE, int AB, int G0 = 0, int G1 = 5>
__device__ __forceinline__ void sw_transform(const float* rawp, const float* raws, const StemRow& row, bool odd, float (&A)[5][9]) {
    const int o[4] = {row.aoff[0], row.aoff[1], row.aoff[2], row.aoff[3]};
    const float k[4] = {row.coef[0], row.coef[1], row.coef[2], row.coef[3]};
    v2f ld[2][5][4];               // [group parity][patch column][tap]: the reads of the next group are in flight while one is combined
    auto issue = [&](int g) {      // group g = channel pair 0..3, 4 = the single channels 16, 17
#pragma unroll
        for (int b = 0; b < NXP; ++b)
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const float* p = (g < 4 ? rawp + g * 4 : raws) + (b >> 1) * SW_PAIR + (b & 1) * SW_C + o[e];
                if (AB == 7) {       // profiling: the channel pair as two 4-byte reads (what a planar, NCHW-fed window would need)
                    typedef const volatile __attribute__((address_space(3))) float* lds_f_t;
                    const lds_f_t q = (lds_f_t)(const __attribute__((address_space(3))) float*)p;
                    ld[g & 1][b][e] = (v2f){q[0], q[1]};
                } else
                    ld[g & 1][b][e] = AB == 1 ? (v2f){(float)(unsigned)(size_t)p, 1.0f} : sw_ld2(p);
            }
    };
    if (G0 > 0 || G1 < 5) {
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int m = 0; m < 9; ++m) A[j][m] = (float)(j + m);
    }
    issue(G0);
#pragma unroll
    for (int g = G0; g < G1; ++g) {
        if (g + 1 < G1) issue(g + 1);
        v2f c[5];
#pragma unroll
        for (int b = 0; b < NXP; ++b) {
            v2f v = k[0] * ld[g & 1][b][0];
#pragma unroll
            for (int e = 1; e < NE; ++e) v = __builtin_elementwise_fma((v2f){k[e], k[e]}, ld[g & 1][b][e], v);
            c[b] = v;
        }
#pragma unroll
        for (int j = 0; j < NXP; ++j) {
            const v2f a = sw_horiz<NXP>(j, c);
            if (g < 4) {
                A[j][2 * g] = a.x;
                A[j][2 * g + 1] = a.y;
            } else {
                A[j][8] = odd ? a.y : a.x;
            }
        }
    }
}

// The MFMAs of one row (nine per position, filters of the position read from LDS one position ahead) and its output transform
// t = M A_x, Y[a][.] += A_y^T[a][i] t.  ub / ub1: this lane's filter fragment slots of position 0 of the row (k 0-15, k 16-17).
template <int NXP, int AB, typename Spread>
__device__ __forceinline__ void sw_gemm(const float* ub, const float* ub1, const StemRow& row, const float (&A)[5][9], f32x16 (&Y)[2][2],
                                        Spread spread) {
    f32x16 M[5];
    const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float4 u0 = AB == 5 ? make_float4(1.f, 2.f, 3.f, 4.f) : *reinterpret_cast<const float4*>(ub);
    float4 u1 = AB == 5 ? make_float4(1.f, 2.f, 3.f, 4.f) : *reinterpret_cast<const float4*>(ub + 256);
    float u2 = AB == 5 ? 1.0f : ub1[0];
#pragma unroll
    for (int j = 0; j < NXP; ++j) {
        float4 n0 = u0, n1 = u1;
        float n2 = u2;
        if (j + 1 < NXP && AB != 5) {
            n0 = *reinterpret_cast<const float4*>(ub + (j + 1) * SW_POS_F);
            n1 = *reinterpret_cast<const float4*>(ub + (j + 1) * SW_POS_F + 256);
            n2 = ub1[(j + 1) * SW_POS_F];
        }
        M[j] = sw_mfma<AB>(u0.x, A[j][0], z);
        M[j] = sw_mfma<AB>(u0.y, A[j][1], M[j]);
        M[j] = sw_mfma<AB>(u0.z, A[j][2], M[j]);
        M[j] = sw_mfma<AB>(u0.w, A[j][3], M[j]);
        M[j] = sw_mfma<AB>(u1.x, A[j][4], M[j]);
        M[j] = sw_mfma<AB>(u1.y, A[j][5], M[j]);
        M[j] = sw_mfma<AB>(u1.z, A[j][6], M[j]);
        M[j] = sw_mfma<AB>(u1.w, A[j][7], M[j]);
        M[j] = sw_mfma<AB>(u2, A[j][8], M[j]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int sl = 2 * j; sl < (j + 1 < NXP ? 2 * j + 2 : 10); ++sl) spread(sl);       // DMA pieces of the next row / phase (see the caller)
        __builtin_amdgcn_sched_barrier(0);
        u0 = n0;
        u1 = n1;
        u2 = n2;
    }
    if (AB == 3) {
#pragma unroll
        for (int j = 0; j < NXP; ++j) Y[j & 1][(j >> 1) & 1][j] += M[j][j];
        return;
    }
    f32x16 t0, t1;
    if (NXP == 5) {
        t0 = (M[0] + M[1]) + (M[2] + M[3]);
        t1 = (M[1] - M[2]) + (2.0f * M[3] + M[4]);
    } else {
        t0 = (M[0] + M[1]) + M[2];
        t1 = (M[1] - M[2]) + M[3];
    }
    const float e0 = row.e0, e1 = row.e1;
    Y[0][0] += e0 * t0;
    Y[0][1] += e0 * t1;
    Y[1][0] += e1 * t0;
    Y[1][1] += e1 * t1;
}

// stem_wino_kernel (stem_wino.hip, where POOL and NCHW are explained) with ablation AB
template <int AB, bool POOL, bool NCHW>
__global__ __launch_bounds__(512) void stem_wino_ablate_kernel(const float* __restrict__ xf, const float* __restrict__ u,
                                                                  const float* __restrict__ scale, const float* __restrict__ shift,
                                                                  float* __restrict__ y, float* __restrict__ side, const StemGeom g) {
    typedef __attribute__((address_space(3))) void* lptr_t;
    extern __shared__ __attribute__((aligned(16))) float smem[];     // raw[team][buf][SW_RAW_F] | filters[buf][SW_U_F]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int team = wave >> 2, w4 = wave & 3, wm = w4 >> 1, wn = w4 & 1;
    const int kl = lane >> 5, il = lane & 31;
    const int ty = 4 * wm + (il >> 3), tx = il & 7;                  // this lane's tile in the item's 8 x 8 block

    // raw-window DMA role: piece t = w4 + 4 k of the team's window, slot s = 64 t + lane -> (window row s / 90, 16-byte slot s % 90);
    // the lane offsets are recomputed per piece (seven registers the row loop has no room for)
    auto raw_voff = [&](int k) {
        unsigned ln = (unsigned)lane;
        asm volatile("" : "+v"(ln));                                   // recomputed where it is used: hoisted out of the loops it was spilled
        const unsigned s = 64u * (unsigned)(w4 + 4 * k) + ln;
        const unsigned wr = __umulhi(s, 0x2D82D83u);                       // s / 90 for s < 2^16 (ceil(2^32 / 90))
        const unsigned q = s - wr * SW_SLOTS;
        return (wr * (unsigned)g.fr_rowf + q * 4u) * 4u;
    };
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)smem;
    const unsigned lds_raw = lds0 + (unsigned)(team * 2 * SW_RAW_F * 4);
    const unsigned lds_u = lds0 + (unsigned)(4 * SW_RAW_F * 4);

    auto window_src = [&](int item, int phase) -> const float* {
        const StemItem at = sw_item(item, g);
        return xf + (size_t)at.b * g.fr_imgf + (size_t)phase * g.fr_phasef + (size_t)(16 * at.by) * g.fr_rowf + (size_t)(8 * at.bx) * SW_PAIR;
    };
    // piece k (0..6) of the phase window whose origin is src -> the team's buffer phase & 1; this wave moves pieces w4, w4 + 4, ...
    auto dma_raw_piece = [&](const float* src, int phase, int k) {
        if (w4 + 4 * k < SW_RAW_PIECES)
            lds_dma16(raw_voff(k), src, lds_raw + (unsigned)((phase & 1) * SW_RAW_F * 4 + (w4 + 4 * k) * 1024));
    };
    auto dma_raw = [&](int item, int phase) {
        const float* src = window_src(item, phase);
#pragma unroll
        for (int k = 0; k < 7; ++k) dma_raw_piece(src, phase, k);
    };
    // piece k (0..2) of the filters of row r -> buffer r & 1; wave w moves pieces w, w + 8, w + 16
    auto dma_filter_piece = [&](int r, int k) {
        const int pieces = c_stem_rows[r].nxp == 5 ? SW_U_PIECES : 18;
        if (wave + 8 * k < pieces)
            lds_dma16((unsigned)(lane * 16), u + (size_t)c_stem_rows[r].upos * SW_POS_F + (wave + 8 * k) * 256,
                      lds_u + (unsigned)((r & 1) * SW_U_F * 4 + (wave + 8 * k) * 1024));
    };
    auto dma_filters = [&](int r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) dma_filter_piece(r, k);
    };

    // LDS read roles
    const float* raw_team = smem + team * 2 * SW_RAW_F;
    const int patch0 = (2 * ty) * SW_ROWF + tx * SW_PAIR;                          // the tile's patch origin in a window (pixel 2 tx = pair tx)
    const float* frag0 = smem + 4 * SW_RAW_F + wn * 576 + kl * 128 + il * 4;      // filter fragment (k 0-7) of position 0, buffer 0
    const float* frag1 = smem + 4 * SW_RAW_F + wn * 576 + 512 + kl * 32 + il;     // ... (k 16-17)

    // ---- NCHW gather role (see the template comment) ----
    const int tt = tid & 255;
    const int n_wi = tt / 10, n_pj = tt - 10 * n_wi;
    const bool n_act = NCHW && tt < 190;
    const unsigned n_goff = (unsigned)((2 * n_wi * g.in_w + 4 * n_pj) * 4);      // bytes from the (item, phase) origin to pixel 0 of the pair
    const int n_lds = n_wi * SW_ROWF + n_pj * SW_PAIR;                            // the pair's float offset in a window buffer
    const long n_plane = (long)g.in_h * g.in_w;
    float lr[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};          // the chunk in flight: lr[2 s + e] = channel s of the chunk, pixel e of the pair
    const float* nc_origin = xf; int nc_y0 = 0, nc_x0 = 0; bool nc_border = false;        // the current item
    const float* nn_origin = xf; int nn_y0 = 0, nn_x0 = 0; bool nn_border = false;        // the next one
    auto nchw_item = [&](int it, const float*& origin, int& y0, int& x0, bool& border) {
        const StemItem at = sw_item(it, g);
        y0 = 32 * (int)at.by - 3; x0 = 32 * (int)at.bx - 3;
        origin = xf + (long)at.b * SW_C * n_plane + (long)y0 * g.in_w + x0;
        border = at.by == 0 || at.bx == 0 || y0 + 38 > g.in_h || x0 + 38 > g.in_w;
    };
    const bool n_act1 = n_act && n_pj < 9;                                         // the pair's second pixel exists (19 pixels per window row)
    const float* n_base = xf;                                                      // wave-uniform: pixel 0 of pair (0, 0), first channel of the chunk
    bool n_ok0 = false, n_ok1 = false, n_zero = false;                             // the lane loads pixel 0 / 1; the chunk needs zeros where it does not
    // chunk q = channels 4 q .. 4 q + 3 (q = 3: 12 .. 17) of BOTH pixels of the pair: the two loads of a channel are neighbours in the
    // instruction stream and hit the same 128-byte lines (chunks split by pixel fetched every line twice: 0.72 against 0.69 ms)
    auto nchw_aim = [&](bool next, int phase, int q) {
        const float* origin = next ? nn_origin : nc_origin;
        const bool border = next ? nn_border : nc_border;
        n_base = origin + (long)(4 * q) * n_plane + (long)(phase >> 1) * g.in_w + (phase & 1);
        n_ok0 = n_act; n_ok1 = n_act1;
        n_zero = border;
        if (border) {
            const int yy = (next ? nn_y0 : nc_y0) + (phase >> 1) + 2 * n_wi, xx = (next ? nn_x0 : nc_x0) + (phase & 1) + 4 * n_pj;
            const bool vy = (unsigned)yy < (unsigned)g.in_h;
            n_ok0 = n_ok0 && vy && (unsigned)xx < (unsigned)g.in_w;
            n_ok1 = n_ok1 && vy && (unsigned)(xx + 2) < (unsigned)g.in_w;
        }
    };
    auto nchw_load2 = [&](int q, int sc) {                   // channel sc of the chunk aimed at, both pixels
        if (sc < (q == 3 ? 6 : 4) && AB != 8) {             // (8: profiling, no gather loads)
            if (n_zero) { lr[2 * sc] = 0.0f; lr[2 * sc + 1] = 0.0f; }
            const float* p = reinterpret_cast<const float*>(reinterpret_cast<const char*>(n_base + sc * n_plane) + n_goff);
            if (n_ok0) lr[2 * sc] = p[0];
            if (n_ok1) lr[2 * sc + 1] = p[2];
        }
    };
    auto nchw_store = [&](int phase, int q) {                // the chunk in lr -> the team's window buffer phase & 1 (slots: c c+2 | c+1 c+3 per four channels)
        if (AB == 9) return;                                 // (9: profiling, no window stores)
        float* d = smem + team * 2 * SW_RAW_F + (phase & 1) * SW_RAW_F + n_lds + 4 * q;
        if (n_act) {
            *reinterpret_cast<v2f*>(d + 0) = (v2f){lr[0], lr[4]};
            *reinterpret_cast<v2f*>(d + 2) = (v2f){lr[2], lr[6]};
            if (q == 3) *reinterpret_cast<v2f*>(d + 4) = (v2f){lr[8], lr[10]};       // channels 16, 17
        }
        if (n_act1) {
            *reinterpret_cast<v2f*>(d + SW_C + 0) = (v2f){lr[1], lr[5]};
            *reinterpret_cast<v2f*>(d + SW_C + 2) = (v2f){lr[3], lr[7]};
            if (q == 3) *reinterpret_cast<v2f*>(d + SW_C + 4) = (v2f){lr[9], lr[11]};
        }
    };

    int pair = blockIdx.x;
    if (2 * pair >= g.n_items) return;
    int item = min(2 * pair + team, g.n_items - 1);
    bool live = 2 * pair + team < g.n_items;
    if (NCHW) {
        nchw_item(item, nc_origin, nc_y0, nc_x0, nc_border);
        for (int q = 0; q < 4; ++q) {                        // the first window, chunk by chunk; then the first chunk of the second one
            nchw_aim(false, 0, q);
#pragma unroll
            for (int sc = 0; sc < 6; ++sc) nchw_load2(q, sc);
            nchw_store(0, q);
        }
        nchw_aim(false, 1, 0);
#pragma unroll
        for (int sc = 0; sc < 6; ++sc) nchw_load2(0, sc);
    } else {
        dma_raw(item, 0);
    }
    dma_filters(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the first row's transform reads the window in front of the row's barrier
    __syncthreads();

    for (;;) {
        f32x16 Y[2][2];                // the four output pixels of the lane's tile x its 16 channels
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) Y[a][b][r] = 0.0f;
        const int next_pair = pair + gridDim.x;
        const bool has_next = 2 * next_pair < g.n_items;
        const int next_item = min(2 * next_pair + team, g.n_items - 1);
        if (NCHW && has_next) nchw_item(next_item, nn_origin, nn_y0, nn_x0, nn_border);

        for (int r = 0; r < SW_ROWS; ++r) {
            const StemRow& row = c_stem_rows[r];
            const int phase = row.phase;
            // NCHW: row idx of its phase stores chunk idx of the NEXT window (loaded during the previous row) and loads chunk idx + 1; the
            // phase's last row loads chunk 0 of the window after next
            const int n_idx = r - (phase == 0 ? 0 : phase == 1 ? 5 : phase == 2 ? 10 : 14);
            const bool n_last = r == SW_ROWS - 1 || c_stem_rows[r + 1].first;
            int n_lq = -1;                                       // chunk to load in this row's MFMA run
            if (NCHW) {
                int l_phase = phase + 1;
                bool l_next = false;
                if (n_idx + 1 < 4) n_lq = n_idx + 1;
                else if (n_last) { n_lq = 0; l_phase = phase + 2; }
                if (l_phase > 3) { l_phase -= 4; l_next = true; if (!has_next) n_lq = -1; }
                if (n_lq >= 0) nchw_aim(l_next, l_phase, n_lq);
            }
            // ---- the row's VALU run: input transform (the window of its phase landed at least a row ago) ----
            const float* rawp = raw_team + (phase & 1) * SW_RAW_F + patch0 + 2 * kl;
            const float* raws = raw_team + (phase & 1) * SW_RAW_F + patch0 + 16;
            const bool odd = kl != 0;
            float A[5][9];
            // Profiling (dev library; results are garbage): what removing the DUPLICATE input transform could buy at most.  The waves of a
            // channel-half pair (wn = 0 / 1) transform the same tiles.  AB = 10: the wn = 1 waves skip the transform outright (operands =
            // constants) -- the upper bound, a hand-over that costs nothing.  AB = 11: they read their 45 operands from LDS instead (the
            // team's window buffer as a stand-in for an exchange buffer: 45 four-byte reads per lane) behind one more barrier per row --
            // the cheapest hand-over there could be (the wn = 0 waves' 45 stores are NOT charged).
            // AB = 12 / 13: the SPLIT form -- each wave of the pair transforms about half of the channels (wn = 0: channel pairs 0-3 of
            // the even / odd parity = groups 0, 1; wn = 1: groups 2, 3 and the singles) and would get the other half from its partner.
            // 12: no exchange at all (the upper bound of the split); 13: + 23 LDS stores, 23 LDS reads per lane and row and a second barrier
            // (stand-ins in the team's window buffer: the cheapest exchange there could be, its 2 x 23 KB of LDS not even found yet).
            if (AB == 12 || AB == 13) {
                if (row.nxp == 5) {
                    if (wn == 0) { if (row.ne == 4) sw_transform<5, 4, AB, 0, 2>(rawp, raws, row, odd, A); else if (row.ne == 3) sw_transform<5, 3, AB, 0, 2>(rawp, raws, row, odd, A); else sw_transform<5, 2, AB, 0, 2>(rawp, raws, row, odd, A); }
                    else { if (row.ne == 4) sw_transform<5, 4, AB, 2, 5>(rawp, raws, row, odd, A); else if (row.ne == 3) sw_transform<5, 3, AB, 2, 5>(rawp, raws, row, odd, A); else sw_transform<5, 2, AB, 2, 5>(rawp, raws, row, odd, A); }
                } else {
                    if (wn == 0) { if (row.ne == 4) sw_transform<4, 4, AB, 0, 2>(rawp, raws, row, odd, A); else if (row.ne == 3) sw_transform<4, 3, AB, 0, 2>(rawp, raws, row, odd, A); else sw_transform<4, 2, AB, 0, 2>(rawp, raws, row, odd, A); }
                    else { if (row.ne == 4) sw_transform<4, 4, AB, 2, 5>(rawp, raws, row, odd, A); else if (row.ne == 3) sw_transform<4, 3, AB, 2, 5>(rawp, raws, row, odd, A); else sw_transform<4, 2, AB, 2, 5>(rawp, raws, row, odd, A); }
                }
                if (AB == 13) {
                    float* xq = const_cast<float*>(raw_team) + (phase & 1) * SW_RAW_F + (w4 * 23) * 64 + lane;
                    if (wn) {
#pragma unroll
                        for (int e = 0; e < 23; ++e) xq[e * 64] = A[e / 9 + 2][e % 9];
                    } else {
#pragma unroll
                        for (int e = 0; e < 23; ++e) xq[e * 64] = A[e / 9][e % 9];
                    }
                }
            } else
            if ((AB == 10 || AB == 11) && wn == 1) {
#pragma unroll
                for (int j = 0; j < 5; ++j)
#pragma unroll
                    for (int m = 0; m < 9; ++m) A[j][m] = AB == 10 ? (float)(j + m) : raw_team[(phase & 1) * SW_RAW_F + (j * 9 + m) * 64 + lane];
            } else
            if (row.nxp == 5) {
                if (row.ne == 4) sw_transform<5, 4, AB>(rawp, raws, row, odd, A);
                else if (row.ne == 3) sw_transform<5, 3, AB>(rawp, raws, row, odd, A);
                else sw_transform<5, 2, AB>(rawp, raws, row, odd, A);
            } else {
                if (row.ne == 4) sw_transform<4, 4, AB>(rawp, raws, row, odd, A);
                else if (row.ne == 3) sw_transform<4, 3, AB>(rawp, raws, row, odd, A);
                else sw_transform<4, 2, AB>(rawp, raws, row, odd, A);
            }
            // NCHW: the chunk loaded during the previous row's MFMA run goes to LDS here, behind the transform (its loads have had the
            // transform's time to arrive; stored at the top of the row they were waited for) and in front of the row's barrier
            if (NCHW && n_idx < 4 && (phase < 3 || has_next)) nchw_store(phase + 1, n_idx);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's pieces of row r's filters (and of the next phase window)
            if (AB != 4) __syncthreads();                        // ... everyone's; the other filter buffer and window buffer are free
            if (AB == 11) __syncthreads();                       // (profiling: the hand-over's second barrier)
            if (AB == 13) {                                      // (profiling: the exchange's second half -- read the partner's 23 operands, one more barrier)
                const float* xq = raw_team + (phase & 1) * SW_RAW_F + ((w4 ^ 1) * 23) * 64 + lane;
                if (wn) {
#pragma unroll
                    for (int e = 0; e < 23; ++e) A[e / 9][e % 9] = xq[e * 64];
                } else {
#pragma unroll
                    for (int e = 0; e < 23; ++e) A[e / 9 + 2][e % 9] = xq[e * 64];
                }
                __syncthreads();
            }
            // The DMAs of the next row's filters (and, in the first row of a phase, of the next phase's window) are issued INSIDE the
            // MFMA run, two pieces behind each position's MFMAs: in front of the run their issue (about 50 cycles a piece, up to ten
            // pieces) held the whole SIMD back while the MFMA pipe was idle.
            const int f_row = r + 1 < SW_ROWS ? r + 1 : (has_next ? 0 : -1);
            const int w_phase = phase < 3 ? phase + 1 : 0;
            const bool w_fetch = !NCHW && row.first && (phase < 3 || has_next);
            const float* w_src = xf;
            if (w_fetch) w_src = window_src(phase < 3 ? item : next_item, w_phase);      // (four rows in eighteen: two divisions)
            // the filter row's source and piece count once per row, not per piece
            const float* f_src = u + (size_t)c_stem_rows[f_row >= 0 ? f_row : 0].upos * SW_POS_F + wave * 256;
            const int f_pieces = f_row < 0 ? 0 : (c_stem_rows[f_row].nxp == 5 ? SW_U_PIECES : 18);
            const unsigned f_dst = lds_u + (unsigned)(((r + 1) & 1) * SW_U_F * 4 + wave * 1024);
            auto spread = [&](int slot) {                        // slots 0-2: filter pieces, 3-9: window pieces
                if (slot < 3) {
                    if (wave + 8 * slot < f_pieces) lds_dma16((unsigned)(lane * 16), f_src + slot * 8 * 256, f_dst + (unsigned)(slot * 8 * 1024));
                } else if (NCHW) {
                    if (n_lq >= 0 && slot < 9) nchw_load2(n_lq, slot - 3);       // (issued in a burst at the head of the run instead: 0.70 against 0.69 ms)
                } else if (w_fetch) {
                    dma_raw_piece(w_src, w_phase, slot - 3);
                }
            };
            // ---- the row's MFMA run, then its output transform (the head of the next VALU run) ----
            const float* ub = frag0 + (r & 1) * SW_U_F;
            const float* ub1 = frag1 + (r & 1) * SW_U_F;
            if (row.nxp == 5) sw_gemm<5, AB>(ub, ub1, row, A, Y, spread);
            else sw_gemm<4, AB>(ub, ub1, row, A, Y, spread);
        }

        // ---- bn1 + relu, stores: lane = one tile (MFMA column), register quad q = channels wn 32 + 8 q + 4 kl .. + 3 ----
        if (AB == 6) {                 // profiling: results kept alive, nothing stored
            float t = 0.0f;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int bb = 0; bb < 2; ++bb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) t += Y[a][bb][r];
            if (t == 12345.678f) y[0] = t;
        } else if (POOL) {
            const int co = wn * 32 + 4 * kl;
            float4 sc[4], sh[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                sc[q] = *reinterpret_cast<const float4*>(scale + co + 8 * q);
                sh[q] = *reinterpret_cast<const float4*>(shift + co + 8 * q);
            }
            const int trow = il >> 3;                                    // the tile's row inside the wave's four
            const bool has_left = tx > 0, up_in_wave = trow > 0;
            // exchange buffer of the team: its window buffer 1 (phase 3's window, read for the last time before row 17's barrier; the next
            // DMA into it is issued behind the next item's first barrier): [wn][kl][bottom maxima | corners][16 channels][8 tiles]
            float* xb = smem + (team * 2 + 1) * SW_RAW_F + ((wn * 2 + kl) * 2) * 128;
            float P[16], Bt[16], R[16], Cn[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int q = r >> 2, e = r & 3;
                const float s1 = e == 0 ? sc[q].x : e == 1 ? sc[q].y : e == 2 ? sc[q].z : sc[q].w;
                const float h1 = e == 0 ? sh[q].x : e == 1 ? sh[q].y : e == 2 ? sh[q].z : sh[q].w;
                float v00 = Y[0][0][r] * s1 + h1, v01 = Y[0][1][r] * s1 + h1, v10 = Y[1][0][r] * s1 + h1, v11 = Y[1][1][r] * s1 + h1;
                if (g.relu) { v00 = fmaxf(v00, 0.f); v01 = fmaxf(v01, 0.f); v10 = fmaxf(v10, 0.f); v11 = fmaxf(v11, 0.f); }
                Bt[r] = fmaxf(v10, v11);
                R[r] = fmaxf(v01, v11);
                Cn[r] = v11;
                P[r] = fmaxf(fmaxf(v00, v01), Bt[r]);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float rl = __shfl_up(R[r], 1), bu = __shfl_up(Bt[r], 8), cu = __shfl_up(Cn[r], 9);
                if (has_left) P[r] = fmaxf(P[r], rl);
                if (up_in_wave) {
                    P[r] = fmaxf(P[r], bu);
                    if (has_left) P[r] = fmaxf(P[r], cu);
                }
            }
            if (wm == 0 && trow == 3) {                                  // tile row 3 of the item: what tile row 4 (the wave below) needs
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    xb[r * 8 + tx] = Bt[r];
                    xb[128 + r * 8 + tx] = Cn[r];
                }
            }
            __syncthreads();
            if (wm == 1 && trow == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    P[r] = fmaxf(P[r], xb[r * 8 + tx]);
                    if (has_left) P[r] = fmaxf(P[r], xb[128 + r * 8 + tx - 1]);
                }
            }
            if (NCHW) __syncthreads();       // the next item's first row STORES into this buffer at once (the frame-fed form's DMA into it waits for a barrier)
            if (live) {
                const StemItem at = sw_item(item, g);
                float* yp = y + (size_t)at.b * g.out_img + (size_t)(8 * at.by + ty + g.opad) * g.out_row + (size_t)(8 * at.bx + tx + g.opad) * SW_CO + co;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<float4*>(yp + 8 * q) = make_float4(P[4 * q], P[4 * q + 1], P[4 * q + 2], P[4 * q + 3]);
                float* sd = side + (size_t)item * 2048 + co;
                if (ty == 7) {                                           // bottom edge: [tx][maxima | corners][64]
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        *reinterpret_cast<float4*>(sd + tx * 128 + 8 * q) = make_float4(Bt[4 * q], Bt[4 * q + 1], Bt[4 * q + 2], Bt[4 * q + 3]);
                        *reinterpret_cast<float4*>(sd + tx * 128 + 64 + 8 * q) = make_float4(Cn[4 * q], Cn[4 * q + 1], Cn[4 * q + 2], Cn[4 * q + 3]);
                    }
                }
                if (tx == 7) {                                           // right edge: [ty][maxima | corners][64]
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        *reinterpret_cast<float4*>(sd + 1024 + ty * 128 + 8 * q) = make_float4(R[4 * q], R[4 * q + 1], R[4 * q + 2], R[4 * q + 3]);
                        *reinterpret_cast<float4*>(sd + 1024 + ty * 128 + 64 + 8 * q) = make_float4(Cn[4 * q], Cn[4 * q + 1], Cn[4 * q + 2], Cn[4 * q + 3]);
                    }
                }
            }
        } else if (live) {
            const StemItem at = sw_item(item, g);
            const int co = wn * 32 + 4 * kl;
            float* yp = y + (size_t)at.b * g.out_img + (size_t)(16 * at.by + 2 * ty + g.opad) * g.out_row +
                        (size_t)(16 * at.bx + 2 * tx + g.opad) * SW_CO + co;
            float4 sc[4], sh[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                sc[q] = *reinterpret_cast<const float4*>(scale + co + 8 * q);
                sh[q] = *reinterpret_cast<const float4*>(shift + co + 8 * q);
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int bb = 0; bb < 2; ++bb)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        float4 v = make_float4(Y[a][bb][4 * q] * sc[q].x + sh[q].x, Y[a][bb][4 * q + 1] * sc[q].y + sh[q].y,
                                               Y[a][bb][4 * q + 2] * sc[q].z + sh[q].z, Y[a][bb][4 * q + 3] * sc[q].w + sh[q].w);
                        if (g.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                        *reinterpret_cast<float4*>(yp + (size_t)a * g.out_row + bb * SW_CO + 8 * q) = v;
                    }
        }
        if (!has_next) break;
        pair = next_pair;
        item = next_item;
        nc_origin = nn_origin; nc_y0 = nn_y0; nc_x0 = nn_x0; nc_border = nn_border;
        live = 2 * pair + team < g.n_items;
    }
}

// ablate -> the launch of the form it names (the table at the head of the file): 1..7 on phase frames, 8..13 pooled on the NCHW input
typedef int (*StemFormLaunch)(const StemGeom&, const float*, const float*, const float*, const float*, float*, float*, hps_stream_t, const char*);
template <int AB>
constexpr StemFormLaunch stem_plain_form = stem_launch_kernel<&stem_wino_ablate_kernel<AB, false, false>>;
template <int AB>
constexpr StemFormLaunch stem_gather_form = stem_launch_kernel<&stem_wino_ablate_kernel<AB, true, true>>;
static const StemFormLaunch k_stem_forms[14] = {
    nullptr,             stem_plain_form<1>,  stem_plain_form<2>,   stem_plain_form<3>,   stem_plain_form<4>,   stem_plain_form<5>,   stem_plain_form<6>,
    stem_plain_form<7>,  stem_gather_form<8>, stem_gather_form<9>,  stem_gather_form<10>, stem_gather_form<11>, stem_gather_form<12>, stem_gather_form<13>};

}  // namespace hps

using namespace hps;

extern "C" int hps_dev_stem_winograd(const float* frames, const float* u, const float* scale, const float* shift, float* y, int B,
                                     int H, int W, int opad, int relu, int ablate, hps_stream_t stream) {
    if (ablate == 0) return stem_wino_launch(frames, u, scale, shift, y, nullptr, B, H, W, opad, relu, false, false, stream);
    StemGeom g;
    int rc = stem_geom(g, frames, u, scale, shift, y, B, H, W, opad, relu, false);
    if (rc != HPS_OK || g.n_items == 0) return rc;
    if (ablate < 1 || ablate > 7) return bad_arg("hps_stem_winograd: ablate");
    if ((rc = k_stem_forms[ablate](g, frames, u, scale, shift, y, nullptr, stream, "hps_stem_winograd")) != HPS_OK) return rc;
    return check_launch("hps_stem_winograd");
}

// The ablated forms stop behind the stem kernel: the border pass is the product's and is not part of what they price.
extern "C" int hps_dev_stem_winograd_pooled_nchw(const float* x, const float* u, const float* scale, const float* shift, float* pooled, float* side,
                                                 int B, int H, int W, int opad, int relu, int ablate, hps_stream_t stream) {
    if (!side) return bad_arg("hps_stem_winograd_pooled_nchw: null pointer");
    if ((size_t)B * SW_C * H * W * 4 >= 0x7fffffffull * 4) return bad_arg("hps_stem_winograd_pooled_nchw: input too large");
    if (ablate == 0) return stem_wino_launch(x, u, scale, shift, pooled, side, B, H, W, opad, relu, true, true, stream);
    StemGeom g;
    int rc = stem_geom(g, x, u, scale, shift, pooled, B, H, W, opad, relu, true);
    if (rc != HPS_OK || g.n_items == 0) return rc;
    if (ablate < 8 || ablate > 13) return bad_arg("hps_stem_winograd_pooled: no ablations");
    if ((rc = k_stem_forms[ablate](g, x, u, scale, shift, pooled, side, stream, "hps_dev_stem_winograd_pooled_nchw")) != HPS_OK) return rc;
    return check_launch("hps_dev_stem_winograd_pooled_nchw");
}
