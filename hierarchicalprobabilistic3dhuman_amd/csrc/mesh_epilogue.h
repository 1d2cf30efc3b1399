// What the two mesh kernels share: mesh_fused_kernel (csrc/mesh_fused.hip, the blend GEMM on the fp32 MFMA) and mesh_split_kernel
// (csrc/mesh_split.hip, the same GEMM as bf16x3 piece products) differ only in their K loops.
//
// Tile = MG mesh groups of 32 meshes x 64 vertices (one panel); wave w = 2 wm + wn works on mesh group wm and vertex group wn (32 each).
// After the K loop a lane holds one vertex (column il = lane & 31) for 16 meshes of its group -- accumulator register r is mesh row
// (r & 3) + 8 (r >> 2) + 4 (lane >> 5) -- as x, y, z in acc[0], acc[1], acc[2]: the layout of v_mfma_f32_32x32x2f32 and of
// v_mfma_f32_32x32x16_bf16 alike.  The epilogue skins that vertex and stores it; the whole tile never leaves the registers as v_posed.
#pragma once

#include <type_traits>

#include "hps_common.h"

namespace hps {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MESH_PANEL = 64;             // vertices per panel

// Block -> (mesh tile, panel).  With at least eight mesh tiles, block ids congruent mod 8 (one XCD) own the same mesh tiles and every
// XCD walks the panels in order, so an XCD's L2 holds its own operand / A slices plus the few panels in flight, and the blend matrix
// streams from the memory-side cache once per XCD.  With fewer (tiles_m_per_xcd == 0) the mapping is plain (block = panel * tiles_m +
// tile): consecutive panels on consecutive XCDs.  (The XCD-aware mapping put all 108 working blocks of a one-tile call -- one image at a
// time, 52 meshes -- at ids = 0 mod 8: on ONE XCD's 32 CUs, the other seven idle: 55-58 us per call.)
struct MeshGrid {
    int tiles_m_per_xcd;
    unsigned blocks;
};
inline MeshGrid mesh_grid(int tiles_m, int n_panels) {
    const int per_xcd = tiles_m >= 8 ? ceil_div(tiles_m, 8) : 0;
    return {per_xcd, (unsigned)(per_xcd ? per_xcd * 8 * n_panels : tiles_m * n_panels)};
}
// false: a block of the XCD-aware grid past the last tile (the whole workgroup returns)
__device__ __forceinline__ bool mesh_block(int tiles_m, int tiles_m_per_xcd, int& tile_m, int& panel) {
    const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
    tile_m = tiles_m_per_xcd ? (local % tiles_m_per_xcd) * 8 + xcd : (int)blockIdx.x % tiles_m;
    panel = tiles_m_per_xcd ? local / tiles_m_per_xcd : (int)blockIdx.x / tiles_m;
    return tile_m < tiles_m;
}

// A lane's place in the tile and what it keeps in registers through the K loop: its vertex, the vertex's skinning weights, its
// templates and its pick slot.
// VS: meshes SHARE their shape, and v_template is the (R, V, 3) array of the R distinct shaped templates.  A lane's 16 meshes lie in ONE
// group of 32 consecutive meshes; group_rows describes it as (row A, row B, split): local mesh < split has template row A, the others
// row B (a tile of sample meshes spans at most two images) -- both rows are fetched here.  split < 0 marks a group whose rows change
// more than once (the mode / T-pose meshes: one image each): the meshes of a tile with such a group fetch their own rows by mesh_row in
// the epilogue (mesh_row is authoritative for every group).
// PICK: the vertices the joint regressors read (pick_slot[v] >= 0) are also written to a compact (M, n_picked, 3) array.
template <int K>
struct MeshLane {
    int lane, wave, kl, il, wm, wn;
    int v, vc;                             // vertex; vc: clamped to V - 1 for the loads
    bool live_v;
    int idx[K];                            // float offset (12 per joint) of the transform of weight k
    float w[K];
    f3 vt, vtb;                            // template rows A and B (not VS: v_template[vc] twice)
    int split, split_lane;                 // local mesh 4 kl + dr < split  <=>  dr < split_lane
    bool many;                             // some group of the tile has split < 0 (workgroup-uniform)
    int pick;                              // slot in the compact array of regressor vertices, or -1
};

template <int K, int MG, bool VS, bool PICK>
__device__ __forceinline__ MeshLane<K> mesh_lane(int panel, int m0, int V, const int32_t* __restrict__ w_idx,
                                                 const float* __restrict__ w_val, const float* __restrict__ v_template,
                                                 const int32_t* __restrict__ group_rows, const int32_t* __restrict__ pick_slot) {
    MeshLane<K> L;
    const int tid = threadIdx.x;
    L.lane = tid & 63;
    L.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    L.kl = L.lane >> 5;
    L.il = L.lane & 31;
    L.wm = L.wave >> 1;
    L.wn = L.wave & 1;
    L.v = panel * MESH_PANEL + L.wn * 32 + L.il;
    L.live_v = L.v < V;
    L.vc = L.live_v ? L.v : V - 1;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        L.idx[k] = w_idx[(size_t)L.vc * K + k] * 12;
        L.w[k] = w_val[(size_t)L.vc * K + k];
    }
    const f3* vtp = reinterpret_cast<const f3*>(v_template);
    L.split = 32;
    L.many = false;
    if (VS) {
        const int32_t* gr = group_rows + 3 * __builtin_amdgcn_readfirstlane((m0 + L.wm * 32) >> 5);      // wave-uniform: scalar loads
        const int row_a = gr[0], row_b = gr[1];
        L.split = gr[2];
        L.vt = vtp[(size_t)row_a * V + L.vc];
        L.vtb = vtp[(size_t)row_b * V + L.vc];
#pragma unroll
        for (int h = 0; h < MG; ++h) L.many |= group_rows[3 * (m0 / 32 + h) + 2] < 0;               // workgroup-uniform: scalar loads
    } else {
        L.vt = vtp[L.vc];
        L.vtb = L.vt;
    }
    L.split_lane = L.split - 4 * L.kl;
    L.pick = PICK && L.live_v ? pick_slot[L.vc] : -1;
    return L;
}

// Dev ablations that run the K loop only: one never-taken store keeps the accumulators alive.
__device__ __forceinline__ void mesh_keep_acc(const f32x16 (&acc)[3], f3* verts) {
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) t += acc[0][r] + acc[1][r] + acc[2][r];
    if (t == 12345.678f) verts[0].x = t;
}

// Dev ablations of the epilogue (profiling): no skinning arithmetic (v_posed is stored), no DMA of the transforms, no stores.
enum MeshEpi { EPI_ALL = 0, EPI_NO_SKIN, EPI_NO_A_DMA, EPI_NO_STORES };

// Skinning, two passes: pass p stages A of meshes [32 h + 16 p, + 16) of the tile for every mesh group h -- the meshes of accumulator
// registers r = 8 p .. 8 p + 7 -- by LDS-DMA into the LDS that held the operands, as slots 16 h .. 16 h + 15; every lane then skins its
// vertex for its 8 meshes of the pass with skin_vertex<K> (the function lbs_kernel uses) and stores 12-byte records: 384 contiguous
// bytes per mesh per wave instruction.  HAS_T: a per-mesh translation is added (smplx SMPL.forward step (7)).
// MANY (VS only): every mesh fetches its own template by mesh_row inside the loop.  That form is a COPY of the epilogue, taken by a
// workgroup with a split < 0 group (MeshLane::many): a load -- or a branch around one -- inside the loop of the common form puts a
// vmcnt(0) there, which on gfx950 also waits for the previous mesh's store, and splits the loop body into blocks hipcc does not schedule
// across (measured: +7 us on the whole launch, more than the fifteen MFMAs per wave the K = 207 form saves).  The choice is the whole
// workgroup's, so every barrier below is on a path that all of its waves run.  (A per-wave choice around each pass's barrier-free
// loop keeps the templates of both forms live at once: 20-24 bytes of scratch per lane in every VS instantiation.)
template <int K, int JC, int MG, bool HAS_T, bool PICK, bool VS, int EPI = EPI_ALL>
__device__ __forceinline__ void mesh_epilogue(float* smem, const MeshLane<K>& L, const f32x16 (&acc)[3], int m0, int M, int V, int J,
                                              const float* __restrict__ a, const float* __restrict__ transl,
                                              const float* __restrict__ v_template, const int32_t* __restrict__ mesh_row,
                                              f3* __restrict__ verts, f3* __restrict__ picked, int n_picked) {
    typedef __attribute__((address_space(3))) void* lptr_t;
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)(smem);
    const int a_stride = JC ? JC * 12 : J * 12;
    const int half_bytes = 16 * a_stride * 4;              // one contiguous source range of J * 768 bytes (whole 1 KiB pieces iff J % 4 == 0;
                                                           // the last piece is cut by the off < valid mask otherwise: tested with J = 22)
    const int slot0 = L.wm * 16 + 4 * L.kl;                // the lane's first slot
    int aoff[K];                                           // float offset of A[slot0][joint_k] in LDS
#pragma unroll
    for (int k = 0; k < K; ++k) aoff[k] = slot0 * a_stride + L.idx[k];
    char* const vbase = reinterpret_cast<char*>(verts) + (size_t)(m0 + L.wm * 32) * V * 12;      // wave-uniform
    const unsigned voff = ((unsigned)(4 * L.kl) * (unsigned)V + (unsigned)L.v) * 12u;            // per lane
    char* const pbase = PICK ? reinterpret_cast<char*>(picked) + (size_t)(m0 + L.wm * 32) * n_picked * 12 : nullptr;
    const unsigned poff = PICK ? ((unsigned)(4 * L.kl) * (unsigned)n_picked + (unsigned)max(L.pick, 0)) * 12u : 0u;
    auto epilogue = [&](auto many_c) __attribute__((always_inline)) {
        constexpr bool MANY = decltype(many_c)::value;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            __syncthreads();                               // operand stages / the previous pass's transforms are dead
#pragma unroll
            for (int h = 0; h < MG; ++h) {
                const int mh = m0 + 32 * h + 16 * pass;                                          // first mesh of this range
                const int valid = max(0, min(16, M - mh)) * a_stride * 4;                      // bytes that exist in `a`
                const float* a_src = a + (size_t)mh * a_stride;
                for (int piece = L.wave; piece * 1024 < half_bytes; piece += 2 * MG) {
                    const int off = piece * 1024 + L.lane * 16;
                    if (off < valid && EPI != EPI_NO_A_DMA) lds_dma16((unsigned)off, a_src, lds0 + (unsigned)(h * half_bytes + piece * 1024));
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            // branch-free: the per-lane parts of every address were formed once, the per-r parts are compile-time / wave-uniform
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int r = 8 * pass + q;
                const int dr = (r & 3) + 8 * (r >> 2);     // mesh row step of accumulator register r (within the wave's 32)
                const int ds = (q & 3) + 8 * (q >> 2);     // ... within the pass's 16 slots of this mesh group
                const int m = m0 + L.wm * 32 + 4 * L.kl + dr;
                float tx = 0.f, ty = 0.f, tz = 0.f;
                if (HAS_T) {
                    const float* t = transl + (size_t)min(m, M - 1) * 3;
                    tx = t[0]; ty = t[1]; tz = t[2];
                }
                f3 base = L.vt;
                if (VS && !MANY) {                         // template A / B of the group by the split: three selects, no load
                    const bool first = dr < L.split_lane;
                    base.x = first ? L.vt.x : L.vtb.x; base.y = first ? L.vt.y : L.vtb.y; base.z = first ? L.vt.z : L.vtb.z;
                }
                if (VS && MANY) base = reinterpret_cast<const f3*>(v_template)[(size_t)mesh_row[min(m, M - 1)] * V + L.vc];
                f3 pv;
                pv.x = base.x + acc[0][r]; pv.y = base.y + acc[1][r]; pv.z = base.z + acc[2][r];
                f3 o;
                if (EPI == EPI_NO_SKIN) {
                    o = pv;
                } else {
                    int ao[K];
#pragma unroll
                    for (int k = 0; k < K; ++k) ao[k] = aoff[k] + ds * a_stride;
                    o = skin_vertex<K>(smem, ao, L.w, pv, tx, ty, tz);
                }
                // Pin the result in front of the guard: hipcc otherwise sinks the whole skinning of a mesh (12 LDS reads, the FMAs)
                // into the guarded store's block, where the reads cannot be issued under the previous mesh's arithmetic and the
                // block's entry waits vmcnt(0) -- i.e. for the previous mesh's store -- on account of the v_template load.
                asm volatile("" :: "v"(o.x), "v"(o.y), "v"(o.z));
                if (EPI == EPI_NO_STORES) {                // a never-true guard keeps the skinning alive
                    if (o.x == 12345.678f) *reinterpret_cast<f3*>(vbase + (size_t)dr * V * 12 + voff) = o;
                    continue;
                }
                if (L.live_v && m < M) *reinterpret_cast<f3*>(vbase + (size_t)dr * V * 12 + voff) = o;
                if (PICK && L.pick >= 0 && m < M) *reinterpret_cast<f3*>(pbase + (size_t)dr * n_picked * 12 + poff) = o;
            }
        }
    };
    if (VS && L.many) epilogue(std::true_type());
    else epilogue(std::false_type());
}

}  // namespace hps
