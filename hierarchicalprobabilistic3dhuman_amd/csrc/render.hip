// The training step's mesh renderer (train/train_poseMF_shapeGaussian_net.py:186-196, renderers/pytorch3d_textured_renderer.py:223-290
// with the defaults of run_train.py:86-91): a hard nearest-face rasteriser with Phong shading, forward only.  The semantics are
// restated in include/hps.h (hps_render) and in tests/render_scenario.py; three launches, no atomics, no host round trip:
//
//   1  render_project_kernel   SMPL vertices -> DensePose vertices (verts_map), world position and NDC position, one lane per vertex
//   2  render_setup_kernel     blocks over the faces: per face validity and pixel bounding box, per chunk of 64 faces (one wave) the
//                              union of its boxes; the remaining blocks: vertex normals, gathered through the vertex-to-faces table
//                              in its order
//   3  render_raster_kernel    one wave per 8 x 8 pixel tile, one lane per pixel.  Every lane tests ONE chunk's box against the tile
//                              (a tile outside the mesh ends there, after one load); the chunks that meet it are taken in chunk
//                              order, RD_GROUP at a time with their loads in flight together: every lane tests one face's box, the
//                              hits are appended to a list of at most 64 edge records in LDS in face order (ballot and prefix
//                              count; no barrier between waves, there is one wave), and whenever the list would overflow, and at
//                              the end, every lane walks it for its own pixel.  The walk is in increasing face index and replaces
//                              the winner only on a strictly smaller depth, so the result does not depend on any launch or lane
//                              order.  The shade -- IUV, texel (bilinear texture gathers or per-vertex colours) and Phong -- is the
//                              tail of the same launch.
//                              The walk is where the time goes (profiles/render_time.txt): a record costs every lane of a tile the
//                              same, so the tile is as small as a wave allows -- a 16 x 16 tile of four waves walked three times as
//                              many records per pixel and took 1.22 ms where this takes the time DESIGN.md section 8 records.
//
// Compiled with -ffp-contract=off (build.py): coverage is a sign decision on the edge functions, and the restatement the kernels are
// held to (numpy, which never contracts) rounds every product; the operation ORDER below is the restatement's, line by line.
//
// The evaluation's silhouette counts (hps_silhouette_iou, second half of this file) run launch 2's face blocks and launch 3's loop
// over the same helpers and end in pixel counts instead of images.
#include "hps_common.h"

namespace hps {

constexpr int RD_TILE = 8;                  // pixels per tile side: one wave, one lane per pixel
constexpr int RD_CHUNK = 64;                // faces per chunk = lanes of the wave that tests them
constexpr int RD_GROUP = 4;                 // chunks whose boxes and corner indices a wave requests together
constexpr int RD_REC = 20;                  // floats of one compacted face record in LDS (five 16-byte reads)
constexpr float RD_EPS = 1e-8f;             // kEpsilon of the coverage rules
constexpr float RD_NORM_EPS = 1e-6f;
constexpr int RD_EMPTY_MIN = 32767, RD_EMPTY_MAX = -1;

int64_t render_ws_bytes(int64_t B, int64_t Nd, int64_t F) {
    const int64_t chunks = (F + RD_CHUNK - 1) / RD_CHUNK;
    // world, ndc, normals: float4 per (image, vertex); face boxes and chunk boxes: two words each
    return B * Nd * 3 * 16 + B * F * 8 + B * chunks * 8;
}

struct RenderWs {
    float4* world;
    float4* ndc;
    float4* normal;
    int2* face_box;
    int2* chunk_box;
};

static RenderWs carve(void* ws, int64_t B, int64_t Nd, int64_t F) {
    const int64_t chunks = (F + RD_CHUNK - 1) / RD_CHUNK;
    RenderWs r;
    char* p = static_cast<char*>(ws);
    r.world = reinterpret_cast<float4*>(p); p += B * Nd * 16;
    r.ndc = reinterpret_cast<float4*>(p); p += B * Nd * 16;
    r.normal = reinterpret_cast<float4*>(p); p += B * Nd * 16;
    r.face_box = reinterpret_cast<int2*>(p); p += B * F * 8;
    r.chunk_box = reinterpret_cast<int2*>(p); p += B * chunks * 8;
    return r;
}

__device__ __forceinline__ int pack16(int lo, int hi) { return (lo & 0xffff) | (hi << 16); }
__device__ __forceinline__ int lo16(int v) { return (int)(short)(v & 0xffff); }
__device__ __forceinline__ int hi16(int v) { return v >> 16; }

// x / max(|x|, 1e-6), the sum of squares added left to right
__device__ __forceinline__ void normalise3(float& x, float& y, float& z) {
    const float n = fmaxf(sqrtf(x * x + y * y + z * z), RD_NORM_EPS);
    x = x / n; y = y / n; z = z / n;
}

// ---- launch 1 ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void render_project_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ verts_map,
                                                             const float* __restrict__ cam_t, int cam_stride,
                                                             const float* __restrict__ scale, int scale_stride, int perspective, int V,
                                                             int Nd, float4* __restrict__ world, float4* __restrict__ ndc) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= Nd) return;
    const float* v = vertices + ((size_t)b * V + verts_map[i]) * 3;
    const float x = v[0], y = v[1], z = v[2];
    const float* t = cam_t + (size_t)b * cam_stride;
    const float* s = scale + (size_t)b * scale_stride;
    const float X = -(x + t[0]), Y = -(y + t[1]), Z = z + t[2];
    float xn = s[0] * X, yn = s[1] * Y;
    if (perspective) { xn = xn / Z; yn = yn / Z; }
    world[(size_t)b * Nd + i] = make_float4(x, y, z, 0.0f);
    ndc[(size_t)b * Nd + i] = make_float4(xn, yn, Z, 0.0f);
}

// ---- launch 2 ---------------------------------------------------------------------------------------------------------------------
// Pixel column c samples x = 1 - (2 c + 1) / W, so x in (xmin, xmax) means c in ((W (1 - xmax) - 1) / 2, (W (1 - xmin) - 1) / 2).
// The box is widened by a hundredth of a pixel on both sides (W <= 4096: the fp32 rounding of these expressions stays below it),
// then cut to the image; it only ever decides which faces a tile LOOKS at, never coverage.
__device__ __forceinline__ void pixel_range(float nmin, float nmax, int W, int& pmin, int& pmax) {
    const float w = (float)W;
    const float lo = fminf(fmaxf((w * (1.0f - nmax) - 1.0f) * 0.5f - 0.01f, -2.0f), w + 1.0f);
    const float hi = fminf(fmaxf((w * (1.0f - nmin) - 1.0f) * 0.5f + 0.01f, -2.0f), w + 1.0f);
    pmin = max(0, (int)floorf(lo));
    pmax = min(W - 1, (int)ceilf(hi));
}

__global__ __launch_bounds__(256) void render_setup_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ vf_offsets,
                                                           const int32_t* __restrict__ vf_faces, const float4* __restrict__ world,
                                                           const float4* __restrict__ ndc, int Nd, int F, int face_blocks, int chunks, int W,
                                                           float4* __restrict__ normal, int2* __restrict__ face_box,
                                                           int2* __restrict__ chunk_box) {
    const int b = blockIdx.y;
    if ((int)blockIdx.x < face_blocks) {
        const int f = blockIdx.x * 256 + threadIdx.x;
        int cmin = RD_EMPTY_MIN, cmax = RD_EMPTY_MAX, rmin = RD_EMPTY_MIN, rmax = RD_EMPTY_MAX;
        if (f < F) {
            const float4* p = ndc + (size_t)b * Nd;
            const float4 v0 = p[faces[3 * f]], v1 = p[faces[3 * f + 1]], v2 = p[faces[3 * f + 2]];
            const float area = (v2.x - v0.x) * (v1.y - v0.y) - (v2.y - v0.y) * (v1.x - v0.x);
            const float zmax = fmaxf(v0.z, fmaxf(v1.z, v2.z));
            if (fabsf(area) > RD_EPS && !(zmax < RD_EPS)) {
                int a0, a1, b0, b1;
                pixel_range(fminf(v0.x, fminf(v1.x, v2.x)), fmaxf(v0.x, fmaxf(v1.x, v2.x)), W, a0, a1);
                pixel_range(fminf(v0.y, fminf(v1.y, v2.y)), fmaxf(v0.y, fmaxf(v1.y, v2.y)), W, b0, b1);
                if (a0 <= a1 && b0 <= b1) { cmin = a0; cmax = a1; rmin = b0; rmax = b1; }
            }
            face_box[(size_t)b * F + f] = make_int2(pack16(cmin, cmax), pack16(rmin, rmax));
        }
        // a chunk is the 64 faces of one wave
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            cmin = min(cmin, __shfl_xor(cmin, off)); cmax = max(cmax, __shfl_xor(cmax, off));
            rmin = min(rmin, __shfl_xor(rmin, off)); rmax = max(rmax, __shfl_xor(rmax, off));
        }
        const int chunk = f / RD_CHUNK;
        if ((threadIdx.x & 63) == 0 && chunk < chunks)
            chunk_box[(size_t)b * chunks + chunk] = make_int2(pack16(cmin, cmax), pack16(rmin, rmax));
        return;
    }
    // vertex normals: sum over the incident faces, in the table's order, of cross(v1 - v0, v2 - v0)
    const int i = ((int)blockIdx.x - face_blocks) * 256 + threadIdx.x;
    if (i >= Nd) return;
    const float4* p = world + (size_t)b * Nd;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    const int k_end = vf_offsets[i + 1];
    for (int k = vf_offsets[i]; k < k_end; ++k) {
        const int f = vf_faces[k];
        const float4 v0 = p[faces[3 * f]], v1 = p[faces[3 * f + 1]], v2 = p[faces[3 * f + 2]];
        const float ax = v1.x - v0.x, ay = v1.y - v0.y, az = v1.z - v0.z;
        const float bx = v2.x - v0.x, by = v2.y - v0.y, bz = v2.z - v0.z;
        nx = nx + (ay * bz - az * by);
        ny = ny + (az * bx - ax * bz);
        nz = nz + (ax * by - ay * bx);
    }
    normalise3(nx, ny, nz);
    normal[(size_t)b * Nd + i] = make_float4(nx, ny, nz, 0.0f);
}

// ---- launch 3 ---------------------------------------------------------------------------------------------------------------------
struct RasterParams {
    const int32_t* faces;
    const int32_t* verts_map;
    const float4* world;
    const float4* ndc;
    const float4* normal;
    const int2* face_box;
    const int2* chunk_box;
    const float* verts_iuv;
    const float* verts_uv;
    const float* texture;
    const float* verts_features;
    const float* cam_t;
    const float* light[4];             // location, ambient, diffuse, specular
    int cam_stride, light_stride[4];
    int Nd, F, V, chunks, W, tex_h, tex_w;
    float* iuv;
    float* rgb;
    float* depth;
    int32_t* pix_to_face;
    float* bary;
    float* iuv_train;
};

// does a packed pixel box meet the tile [c0, c1] x [r0, r1]
__device__ __forceinline__ bool meets(int2 box, int c0, int c1, int r0, int r1) {
    return !(lo16(box.x) > c1 || hi16(box.x) < c0 || lo16(box.y) > r1 || hi16(box.y) < r0);
}

__device__ __forceinline__ float lerp(float a, float b, float t) { return a + t * (b - a); }

// One face of the wave's chunk per lane: the hits' edge records go to LDS behind the `count` records already there, in lane (= face)
// order.  E(p, a, b) = (p.x - a.x) (b.y - a.y) - (p.y - a.y) (b.x - a.x) for (a, b) = (v1, v2), (v2, v0), (v0, v1).
__device__ __forceinline__ void put_record(float* rec, int slot, int f, const float4 v0, const float4 v1, const float4 v2) {
    const float area = (v2.x - v0.x) * (v1.y - v0.y) - (v2.y - v0.y) * (v1.x - v0.x);
    float4* o = reinterpret_cast<float4*>(rec + slot * RD_REC);
    o[0] = make_float4(v1.x, v1.y, v2.y - v1.y, v2.x - v1.x);
    o[1] = make_float4(v2.x, v2.y, v0.y - v2.y, v0.x - v2.x);
    o[2] = make_float4(v0.x, v0.y, v1.y - v0.y, v1.x - v0.x);
    o[3] = make_float4(area + RD_EPS, v0.z, v1.z, v2.z);
    o[4] = make_float4(__int_as_float(f), 0.0f, 0.0f, 0.0f);
}

struct Winner {
    float z, w0, w1, w2;
    int f;
};

// every lane takes the `n` records for its own pixel, in list (= face) order; the winner changes only on a strictly smaller depth
__device__ __forceinline__ void walk(const float* rec, int n, float px, float py, Winner& best) {
    for (int i = 0; i < n; ++i) {
        const float4* q = reinterpret_cast<const float4*>(rec + i * RD_REC);
        const float4 e0 = q[0], e1 = q[1], e2 = q[2], d = q[3];
        const float E0 = (px - e0.x) * e0.z - (py - e0.y) * e0.w;
        const float E1 = (px - e1.x) * e1.z - (py - e1.y) * e1.w;
        const float E2 = (px - e2.x) * e2.z - (py - e2.y) * e2.w;
        // all three quotients positive needs all three numerators on the denominator's side: the divisions are made only then
        const bool pos = E0 > 0.0f && E1 > 0.0f && E2 > 0.0f && d.x > 0.0f;
        const bool neg = E0 < 0.0f && E1 < 0.0f && E2 < 0.0f && d.x < 0.0f;
        if (pos || neg) {
            const float w0 = E0 / d.x, w1 = E1 / d.x, w2 = E2 / d.x;
            const float pz = w0 * d.y + w1 * d.z + w2 * d.w;
            if (w0 > 0.0f && w1 > 0.0f && w2 > 0.0f && pz >= 0.0f && pz < best.z) {
                best.z = pz; best.w0 = w0; best.w1 = w1; best.w2 = w2;
                best.f = __float_as_int(q[4].x);
            }
        }
    }
}

__global__ __launch_bounds__(64) void render_raster_kernel(const RasterParams P) {
    __shared__ __attribute__((aligned(16))) float rec[RD_CHUNK * RD_REC];
    const int b = blockIdx.z, lane = threadIdx.x;
    const unsigned long long lane_lt = (1ull << lane) - 1ull;
    const int W = P.W, Nd = P.Nd, F = P.F;
    const int tc0 = blockIdx.x * RD_TILE, tr0 = blockIdx.y * RD_TILE;
    const int tc1 = min(tc0 + RD_TILE, W) - 1, tr1 = min(tr0 + RD_TILE, W) - 1;
    const int c = tc0 + (lane & (RD_TILE - 1)), r = tr0 + (lane >> 3);
    const bool inside = c < W && r < W;
    const float px = 1.0f - (float)(2 * c + 1) / (float)W;
    const float py = 1.0f - (float)(2 * r + 1) / (float)W;
    const float4* ndc = P.ndc + (size_t)b * Nd;
    const int2* face_box = P.face_box + (size_t)b * F;

    Winner best = {__builtin_inff(), 0.0f, 0.0f, 0.0f, -1};
    int count = 0;                                         // records in LDS that have not been walked yet (wave-uniform)

    for (int c0 = 0; c0 < P.chunks; c0 += 64) {
        // 64 chunk boxes against the tile, one per lane: a tile outside the mesh ends after this load
        bool chit = false;
        if (c0 + lane < P.chunks) chit = meets(P.chunk_box[(size_t)b * P.chunks + c0 + lane], tc0, tc1, tr0, tr1);
        unsigned long long cm = __ballot(chit);
        while (cm) {
            // the next RD_GROUP chunks that meet the tile, in chunk order; their face boxes and corner indices are requested together
            int f[RD_GROUP], i0[RD_GROUP], i1[RD_GROUP], i2[RD_GROUP];
            int2 fb[RD_GROUP];
#pragma unroll
            for (int g = 0; g < RD_GROUP; ++g) {
                f[g] = F;
                if (cm) {
                    f[g] = (c0 + __builtin_ctzll(cm)) * RD_CHUNK + lane;
                    cm &= cm - 1;
                }
                const int fc = min(f[g], F - 1);
                fb[g] = face_box[fc];
                i0[g] = P.faces[3 * fc]; i1[g] = P.faces[3 * fc + 1]; i2[g] = P.faces[3 * fc + 2];
            }
#pragma unroll
            for (int g = 0; g < RD_GROUP; ++g) {
                const bool hit = f[g] < F && meets(fb[g], tc0, tc1, tr0, tr1);
                const unsigned long long m = __ballot(hit);
                const int nh = __popcll(m);
                if (nh == 0) continue;
                if (count + nh > RD_CHUNK) {               // the list would overflow: walk it first
                    __syncthreads();
                    walk(rec, count, px, py, best);
                    count = 0;
                    __syncthreads();
                }
                if (hit) put_record(rec, count + __popcll(m & lane_lt), f[g], ndc[i0[g]], ndc[i1[g]], ndc[i2[g]]);
                count += nh;
            }
        }
    }
    __syncthreads();
    walk(rec, count, px, py, best);
    const float best_z = best.z, bw0 = best.w0, bw1 = best.w1, bw2 = best.w2;
    const int best_f = best.f;
    if (!inside) return;

    // ---- the shade ------------------------------------------------------------------------------------------------------------------
    const size_t plane = (size_t)W * W, pix = (size_t)r * W + c;
    const bool covered = best_f >= 0;
    float iu[3] = {0.0f, 0.0f, 0.0f}, col[3] = {0.0f, 0.0f, 0.0f};
    if (covered) {
        const int i0 = P.faces[3 * best_f], i1 = P.faces[3 * best_f + 1], i2 = P.faces[3 * best_f + 2];
        const float* a0 = P.verts_iuv + 3 * (size_t)i0, * a1 = P.verts_iuv + 3 * (size_t)i1, * a2 = P.verts_iuv + 3 * (size_t)i2;
#pragma unroll
        for (int k = 0; k < 3; ++k) iu[k] = bw0 * a0[k] + bw1 * a1[k] + bw2 * a2[k];
        if (P.rgb) {
            float tex[3];
            if (P.verts_features) {
                const float* g = P.verts_features + (size_t)b * P.V * 3;
                const float* g0 = g + 3 * (size_t)P.verts_map[i0], * g1 = g + 3 * (size_t)P.verts_map[i1], * g2 = g + 3 * (size_t)P.verts_map[i2];
#pragma unroll
                for (int k = 0; k < 3; ++k) tex[k] = bw0 * g0[k] + bw1 * g1[k] + bw2 * g2[k];
            } else {
                const float2* uv = reinterpret_cast<const float2*>(P.verts_uv);
                const float2 u0 = uv[i0], u1 = uv[i1], u2 = uv[i2];
                const float u = bw0 * u0.x + bw1 * u1.x + bw2 * u2.x, v = bw0 * u0.y + bw1 * u1.y + bw2 * u2.y;
                const int Ht = P.tex_h, Wt = P.tex_w;
                const float x = fminf(fmaxf(u * (float)(Wt - 1), 0.0f), (float)(Wt - 1));
                const float y = fminf(fmaxf((1.0f - v) * (float)(Ht - 1), 0.0f), (float)(Ht - 1));
                const float xf = floorf(x), yf = floorf(y);
                const int x0 = (int)xf, y0 = (int)yf, x1 = min(x0 + 1, Wt - 1), y1 = min(y0 + 1, Ht - 1);
                const float fx = x - xf, fy = y - yf;
                const float* t = P.texture + (size_t)b * Ht * Wt * 3;
                const float* t00 = t + ((size_t)y0 * Wt + x0) * 3, * t01 = t + ((size_t)y0 * Wt + x1) * 3;
                const float* t10 = t + ((size_t)y1 * Wt + x0) * 3, * t11 = t + ((size_t)y1 * Wt + x1) * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) tex[k] = lerp(lerp(t00[k], t01[k], fx), lerp(t10[k], t11[k], fx), fy);
            }
            const float4* nv = P.normal + (size_t)b * Nd;
            const float4* wv = P.world + (size_t)b * Nd;
            const float4 n0 = nv[i0], n1 = nv[i1], n2 = nv[i2], p0 = wv[i0], p1 = wv[i1], p2 = wv[i2];
            float nx = bw0 * n0.x + bw1 * n1.x + bw2 * n2.x, ny = bw0 * n0.y + bw1 * n1.y + bw2 * n2.y,
                  nz = bw0 * n0.z + bw1 * n1.z + bw2 * n2.z;
            normalise3(nx, ny, nz);
            const float Px = bw0 * p0.x + bw1 * p1.x + bw2 * p2.x, Py = bw0 * p0.y + bw1 * p1.y + bw2 * p2.y,
                        Pz = bw0 * p0.z + bw1 * p1.z + bw2 * p2.z;
            const float* ll = P.light[0] + (size_t)b * P.light_stride[0];
            const float* am = P.light[1] + (size_t)b * P.light_stride[1];
            const float* di = P.light[2] + (size_t)b * P.light_stride[2];
            const float* sp = P.light[3] + (size_t)b * P.light_stride[3];
            const float* ct = P.cam_t + (size_t)b * P.cam_stride;
            float Lx = ll[0] - Px, Ly = ll[1] - Py, Lz = ll[2] - Pz;
            normalise3(Lx, Ly, Lz);
            float vx = -ct[0] - Px, vy = -ct[1] - Py, vz = -ct[2] - Pz;
            normalise3(vx, vy, vz);
            const float nl = nx * Lx + ny * Ly + nz * Lz;
            const float rx = -Lx + 2.0f * nl * nx, ry = -Ly + 2.0f * nl * ny, rz = -Lz + 2.0f * nl * nz;
            float s = fmaxf(vx * rx + vy * ry + vz * rz, 0.0f) * (nl > 0.0f ? 1.0f : 0.0f);
#pragma unroll
            for (int k = 0; k < 6; ++k) s = s * s;                                   // shininess 64
            const float dl = fmaxf(nl, 0.0f);
#pragma unroll
            for (int k = 0; k < 3; ++k) col[k] = fminf(1.0f, (am[k] + di[k] * dl) * tex[k] + sp[k] * s);
        }
    }
    if (P.iuv) {
        float* o = P.iuv + (size_t)b * 3 * plane + pix;
        o[0] = iu[0]; o[plane] = iu[1]; o[2 * plane] = iu[2];
    }
    if (P.iuv_train) {                                     // :193-195: U and V times 255, the three planes rounded half to even
        float* o = P.iuv_train + (size_t)b * 3 * plane + pix;
        o[0] = rintf(iu[0]); o[plane] = rintf(iu[1] * 255.0f); o[2 * plane] = rintf(iu[2] * 255.0f);
    }
    if (P.rgb) {
        float* o = P.rgb + (size_t)b * 3 * plane + pix;
        o[0] = col[0]; o[plane] = col[1]; o[2 * plane] = col[2];
    }
    if (P.depth) P.depth[(size_t)b * plane + pix] = covered ? best_z : -1.0f;
    if (P.pix_to_face) P.pix_to_face[(size_t)b * plane + pix] = best_f;
    if (P.bary) {
        float* o = P.bary + (size_t)b * 3 * plane + pix;
        o[0] = covered ? bw0 : -1.0f; o[plane] = covered ? bw1 : -1.0f; o[2 * plane] = covered ? bw2 : -1.0f;
    }
}

// ---- silhouette counts (hps_silhouette_iou) ---------------------------------------------------------------------------------------
// The evaluation's silhouette metrics (evaluate/evaluate_poseMF_shapeGaussian_net.py:143-155, 192-203 with
// metrics/eval_metrics_tracker.py:294-328) need one bit per pixel of every mesh, compared with a target bit and counted.  Four
// launches over the same face boxes, records and walk as above:
//
//   1  silhouette_project_kernel   as launch 1, with the rotation by pi about x folded in, a camera per GROUP of meshes, NDC only
//   2  render_setup_kernel         its face blocks only: no normals are needed, none are computed
//   3  silhouette_raster_kernel    launch 3's chunk / record / walk loop (the loop is repeated here, render_raster_kernel is left
//                                  as it is); then the winner's rounded part label against the target byte, four ballots, and one
//                                  16-byte store of the tile's [tp, fp, tn, fn]
//   4  silhouette_reduce_kernel    a mesh's tile counts added up: integers, so any order gives the same sums
int64_t silhouette_ws_bytes(int64_t M, int64_t Nd, int64_t F, int64_t W) {
    const int64_t chunks = (F + RD_CHUNK - 1) / RD_CHUNK, tiles = (W + RD_TILE - 1) / RD_TILE;
    // ndc: float4 per (mesh, vertex); tile counts: int4 per (mesh, tile); face boxes and chunk boxes: two words each
    return M * Nd * 16 + M * tiles * tiles * 16 + M * F * 8 + M * chunks * 8;
}

struct SilhouetteWs {
    float4* ndc;
    int4* tile_counts;
    int2* face_box;
    int2* chunk_box;
};

static SilhouetteWs carve_silhouette(void* ws, int64_t M, int64_t Nd, int64_t F, int64_t W) {
    const int64_t tiles = (W + RD_TILE - 1) / RD_TILE;
    SilhouetteWs r;
    char* p = static_cast<char*>(ws);
    r.ndc = reinterpret_cast<float4*>(p); p += M * Nd * 16;
    r.tile_counts = reinterpret_cast<int4*>(p); p += M * tiles * tiles * 16;
    r.face_box = reinterpret_cast<int2*>(p); p += M * F * 8;
    r.chunk_box = reinterpret_cast<int2*>(p);
    return r;
}

// Mesh m is seen by camera m / group.  flip: the vertex rotated by pi about x, (x, -y, -z) -- a negation is exact, so the result is
// the one render_project_kernel gives for vertices flipped beforehand.
__global__ __launch_bounds__(256) void silhouette_project_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ verts_map,
                                                                 const float* __restrict__ cam_t, int cam_stride,
                                                                 const float* __restrict__ scale, int scale_stride, int perspective,
                                                                 int flip, int group, int V, int Nd, float4* __restrict__ ndc) {
    const int i = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
    if (i >= Nd) return;
    const float* v = vertices + ((size_t)m * V + verts_map[i]) * 3;
    const float x = v[0], y = flip ? -v[1] : v[1], z = flip ? -v[2] : v[2];
    const float* t = cam_t + (size_t)(m / group) * cam_stride;
    const float* s = scale + (size_t)(m / group) * scale_stride;
    const float X = -(x + t[0]), Y = -(y + t[1]), Z = z + t[2];
    float xn = s[0] * X, yn = s[1] * Y;
    if (perspective) { xn = xn / Z; yn = yn / Z; }
    ndc[(size_t)m * Nd + i] = make_float4(xn, yn, Z, 0.0f);
}

struct SilhouetteParams {
    const int32_t* faces;
    const float4* ndc;
    const int2* face_box;
    const int2* chunk_box;
    const float* verts_iuv;
    const uint8_t* target;
    int Nd, F, chunks, W, group;
    int4* tile_counts;
    uint8_t* mask_out;
};

__global__ __launch_bounds__(64) void silhouette_raster_kernel(const SilhouetteParams P) {
    __shared__ __attribute__((aligned(16))) float rec[RD_CHUNK * RD_REC];
    const int b = blockIdx.z, lane = threadIdx.x;
    const unsigned long long lane_lt = (1ull << lane) - 1ull;
    const int W = P.W, Nd = P.Nd, F = P.F;
    const int tc0 = blockIdx.x * RD_TILE, tr0 = blockIdx.y * RD_TILE;
    const int tc1 = min(tc0 + RD_TILE, W) - 1, tr1 = min(tr0 + RD_TILE, W) - 1;
    const int c = tc0 + (lane & (RD_TILE - 1)), r = tr0 + (lane >> 3);
    const bool inside = c < W && r < W;
    const float px = 1.0f - (float)(2 * c + 1) / (float)W;
    const float py = 1.0f - (float)(2 * r + 1) / (float)W;
    const float4* ndc = P.ndc + (size_t)b * Nd;
    const int2* face_box = P.face_box + (size_t)b * F;

    // the target byte of image m / group; NULL: no target, every pixel counts as background
    const size_t plane = (size_t)W * W, pix = (size_t)r * W + c;
    bool tgt = false;
    if (inside && P.target) tgt = P.target[(size_t)(b / P.group) * plane + pix] != 0;

    Winner best = {__builtin_inff(), 0.0f, 0.0f, 0.0f, -1};
    int count = 0;                                         // records in LDS that have not been walked yet (wave-uniform)

    // render_raster_kernel's loop; every condition around a barrier is wave-uniform (a ballot or a kernel argument), and a tile that
    // meets no chunk falls through to the count below like any other
    for (int c0 = 0; c0 < P.chunks; c0 += 64) {
        bool chit = false;
        if (c0 + lane < P.chunks) chit = meets(P.chunk_box[(size_t)b * P.chunks + c0 + lane], tc0, tc1, tr0, tr1);
        unsigned long long cm = __ballot(chit);
        while (cm) {
            int f[RD_GROUP], i0[RD_GROUP], i1[RD_GROUP], i2[RD_GROUP];
            int2 fb[RD_GROUP];
#pragma unroll
            for (int g = 0; g < RD_GROUP; ++g) {
                f[g] = F;
                if (cm) {
                    f[g] = (c0 + __builtin_ctzll(cm)) * RD_CHUNK + lane;
                    cm &= cm - 1;
                }
                const int fc = min(f[g], F - 1);
                fb[g] = face_box[fc];
                i0[g] = P.faces[3 * fc]; i1[g] = P.faces[3 * fc + 1]; i2[g] = P.faces[3 * fc + 2];
            }
#pragma unroll
            for (int g = 0; g < RD_GROUP; ++g) {
                const bool hit = f[g] < F && meets(fb[g], tc0, tc1, tr0, tr1);
                const unsigned long long m = __ballot(hit);
                const int nh = __popcll(m);
                if (nh == 0) continue;
                if (count + nh > RD_CHUNK) {               // the list would overflow: walk it first
                    __syncthreads();
                    walk(rec, count, px, py, best);
                    count = 0;
                    __syncthreads();
                }
                if (hit) put_record(rec, count + __popcll(m & lane_lt), f[g], ndc[i0[g]], ndc[i1[g]], ndc[i2[g]]);
                count += nh;
            }
        }
    }
    __syncthreads();
    walk(rec, count, px, py, best);

    // the part label as the shade forms iu[0], rounded half to even: convert_multiclass_to_binary_labels(iuv[..., 0].round()).  The
    // nearest face decides even where its label rounds to 0 (a sliver whose area is just above 1e-8), as in hps_render's own image.
    bool set = false;
    if (inside && best.f >= 0) {
        const int i0 = P.faces[3 * best.f], i1 = P.faces[3 * best.f + 1], i2 = P.faces[3 * best.f + 2];
        const float part = best.w0 * P.verts_iuv[3 * (size_t)i0] + best.w1 * P.verts_iuv[3 * (size_t)i1] + best.w2 * P.verts_iuv[3 * (size_t)i2];
        set = rintf(part) != 0.0f;
    }
    if (inside && P.mask_out) P.mask_out[(size_t)b * plane + pix] = set ? 1 : 0;
    const int tp = __popcll(__ballot(inside && set && tgt)), fp = __popcll(__ballot(inside && set && !tgt));
    const int tn = __popcll(__ballot(inside && !set && !tgt)), fn = __popcll(__ballot(inside && !set && tgt));
    if (lane == 0) P.tile_counts[((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = make_int4(tp, fp, tn, fn);
}

// one workgroup per mesh; W <= 4096: no sum exceeds 2^24
__global__ __launch_bounds__(256) void silhouette_reduce_kernel(const int4* __restrict__ tile_counts, int tiles2, int32_t* __restrict__ counts) {
    __shared__ int4 part[256];
    const int4* t = tile_counts + (size_t)blockIdx.x * tiles2;
    int4 s = make_int4(0, 0, 0, 0);
    for (int i = threadIdx.x; i < tiles2; i += 256) {
        const int4 v = t[i];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const int4 v = part[threadIdx.x + off];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            part[threadIdx.x] = s;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) reinterpret_cast<int4*>(counts)[blockIdx.x] = s;
}

}  // namespace hps

extern "C" int hps_sizeof_silhouette_args(void) { return (int)sizeof(hps_silhouette_args); }

extern "C" int hps_silhouette_iou(const hps_silhouette_args* a, hps_stream_t stream) {
    using namespace hps;
    if (!a) return bad_arg("hps_silhouette_iou: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_silhouette_args))
        return bad_arg("hps_silhouette_iou: struct_bytes is not sizeof(hps_silhouette_args)");
    if (!a->vertices || !a->verts_map || !a->faces || !a->verts_iuv || !a->cam_t || !a->scale || !a->workspace)
        return bad_arg("hps_silhouette_iou: null pointer (vertices, verts_map, faces, verts_iuv, cam_t, scale, workspace)");
    if (!a->counts && !a->mask_out) return bad_arg("hps_silhouette_iou: no output wanted (counts and mask_out are both null)");
    if (a->M < 1 || a->M > 65535 || a->W < 1 || a->W > 4096) return bad_arg("hps_silhouette_iou: M in [1, 65535], W in [1, 4096]");
    if (a->group < 1 || a->M % a->group != 0) return bad_arg("hps_silhouette_iou: group >= 1 must divide M");
    if (a->num_verts < 1 || a->num_dp_verts < 1 || a->num_faces < 1 || a->num_faces > (1 << 24))
        return bad_arg("hps_silhouette_iou: num_verts, num_dp_verts >= 1, num_faces in [1, 2^24]");
    if (a->projection != HPS_RENDER_PERSPECTIVE && a->projection != HPS_RENDER_ORTHOGRAPHIC)
        return bad_arg("hps_silhouette_iou: unknown projection");
    if ((a->cam_t_stride != 0 && a->cam_t_stride != 3) || (a->scale_stride != 0 && a->scale_stride != 2))
        return bad_arg("hps_silhouette_iou: cam_t_stride is 0 or 3, scale_stride 0 or 2");
    if ((reinterpret_cast<uintptr_t>(a->workspace) & 15) || (reinterpret_cast<uintptr_t>(a->counts) & 15))
        return bad_arg("hps_silhouette_iou: workspace and counts must be 16-byte aligned");
    const int M = a->M, W = a->W, Nd = a->num_dp_verts, F = a->num_faces;
    const int chunks = ceil_div(F, RD_CHUNK), face_blocks = ceil_div(F, 256), vblocks = ceil_div(Nd, 256), tiles = ceil_div(W, RD_TILE);
    const SilhouetteWs ws = carve_silhouette(a->workspace, M, Nd, F, W);
    hipStream_t st = (hipStream_t)stream;

    hipLaunchKernelGGL(silhouette_project_kernel, dim3(vblocks, M), dim3(256), 0, st, a->vertices, a->verts_map, a->cam_t,
                       a->cam_t_stride, a->scale, a->scale_stride, a->projection == HPS_RENDER_PERSPECTIVE ? 1 : 0,
                       a->flip_x_pi != 0 ? 1 : 0, a->group, a->num_verts, Nd, ws.ndc);
    int rc = check_launch("hps_silhouette_iou (project)");
    if (rc) return rc;
    // gridDim.x == face_blocks: every workgroup takes the face branch, the vertex-normal half and its pointers are never touched
    hipLaunchKernelGGL(render_setup_kernel, dim3(face_blocks, M), dim3(256), 0, st, a->faces, (const int32_t*)nullptr,
                       (const int32_t*)nullptr, (const float4*)nullptr, ws.ndc, Nd, F, face_blocks, chunks, W, (float4*)nullptr,
                       ws.face_box, ws.chunk_box);
    rc = check_launch("hps_silhouette_iou (set-up)");
    if (rc) return rc;
    SilhouetteParams P;
    P.faces = a->faces; P.ndc = ws.ndc; P.face_box = ws.face_box; P.chunk_box = ws.chunk_box; P.verts_iuv = a->verts_iuv;
    P.target = a->target; P.Nd = Nd; P.F = F; P.chunks = chunks; P.W = W; P.group = a->group;
    P.tile_counts = ws.tile_counts; P.mask_out = a->mask_out;
    hipLaunchKernelGGL(silhouette_raster_kernel, dim3(tiles, tiles, M), dim3(64), 0, st, P);
    rc = check_launch("hps_silhouette_iou (rasterise and count)");
    if (rc || !a->counts) return rc;
    hipLaunchKernelGGL(silhouette_reduce_kernel, dim3(M), dim3(256), 0, st, ws.tile_counts, tiles * tiles, a->counts);
    return check_launch("hps_silhouette_iou (reduce)");
}

extern "C" int hps_sizeof_render_args(void) { return (int)sizeof(hps_render_args); }

extern "C" int hps_render(const hps_render_args* a, hps_stream_t stream) {
    using namespace hps;
    if (!a) return bad_arg("hps_render: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_render_args)) return bad_arg("hps_render: struct_bytes is not sizeof(hps_render_args)");
    if (!a->vertices || !a->verts_map || !a->faces || !a->vf_offsets || !a->vf_faces || !a->verts_iuv || !a->cam_t || !a->scale ||
        !a->workspace)
        return bad_arg("hps_render: null pointer (vertices, verts_map, faces, vf_offsets, vf_faces, verts_iuv, cam_t, scale, workspace)");
    if (a->H != a->W) return bad_arg("hps_render: images are square only (H == W)");
    if (a->B < 1 || a->B > 65535 || a->W < 1 || a->W > 4096) return bad_arg("hps_render: B in [1, 65535], W in [1, 4096]");
    if (a->num_verts < 1 || a->num_dp_verts < 1 || a->num_faces < 1 || a->num_faces > (1 << 24))
        return bad_arg("hps_render: num_verts, num_dp_verts >= 1, num_faces in [1, 2^24]");
    if (a->projection != HPS_RENDER_PERSPECTIVE && a->projection != HPS_RENDER_ORTHOGRAPHIC)
        return bad_arg("hps_render: unknown projection");
    if ((a->cam_t_stride != 0 && a->cam_t_stride != 3) || (a->scale_stride != 0 && a->scale_stride != 2))
        return bad_arg("hps_render: cam_t_stride is 0 or 3, scale_stride 0 or 2");
    if (!a->iuv && !a->iuv_train && !a->rgb && !a->depth && !a->pix_to_face && !a->bary) return bad_arg("hps_render: no output wanted");
    if (a->rgb) {
        if (!a->light_location || !a->ambient || !a->diffuse || !a->specular) return bad_arg("hps_render: null pointer (lights) with rgb");
        for (int k = 0; k < 4; ++k)
            if (a->light_stride[k] != 0 && a->light_stride[k] != 3) return bad_arg("hps_render: light_stride is 0 or 3");
        if (!a->verts_features) {
            if (!a->texture || !a->verts_uv) return bad_arg("hps_render: rgb needs texture and verts_uv, or verts_features");
            if (a->tex_h < 1 || a->tex_w < 1 || a->tex_h > 32768 || a->tex_w > 32768) return bad_arg("hps_render: texture sides in [1, 32768]");
        }
    }
    if (reinterpret_cast<uintptr_t>(a->workspace) & 15) return bad_arg("hps_render: workspace must be 16-byte aligned");
    const int B = a->B, W = a->W, Nd = a->num_dp_verts, F = a->num_faces;
    const int chunks = ceil_div(F, RD_CHUNK), face_blocks = ceil_div(F, 256), vblocks = ceil_div(Nd, 256), tiles = ceil_div(W, RD_TILE);
    const RenderWs ws = carve(a->workspace, B, Nd, F);
    hipStream_t st = (hipStream_t)stream;

    hipLaunchKernelGGL(render_project_kernel, dim3(vblocks, B), dim3(256), 0, st, a->vertices, a->verts_map, a->cam_t, a->cam_t_stride,
                       a->scale, a->scale_stride, a->projection == HPS_RENDER_PERSPECTIVE ? 1 : 0, a->num_verts, Nd, ws.world, ws.ndc);
    int rc = check_launch("hps_render (project)");
    if (rc) return rc;
    hipLaunchKernelGGL(render_setup_kernel, dim3(face_blocks + vblocks, B), dim3(256), 0, st, a->faces, a->vf_offsets, a->vf_faces,
                       ws.world, ws.ndc, Nd, F, face_blocks, chunks, W, ws.normal, ws.face_box, ws.chunk_box);
    rc = check_launch("hps_render (set-up)");
    if (rc) return rc;
    RasterParams P;
    P.faces = a->faces; P.verts_map = a->verts_map; P.world = ws.world; P.ndc = ws.ndc; P.normal = ws.normal;
    P.face_box = ws.face_box; P.chunk_box = ws.chunk_box; P.verts_iuv = a->verts_iuv; P.verts_uv = a->verts_uv;
    P.texture = a->texture; P.verts_features = a->verts_features; P.cam_t = a->cam_t; P.cam_stride = a->cam_t_stride;
    P.light[0] = a->light_location; P.light[1] = a->ambient; P.light[2] = a->diffuse; P.light[3] = a->specular;
    for (int k = 0; k < 4; ++k) P.light_stride[k] = a->light_stride[k];
    P.Nd = Nd; P.F = F; P.V = a->num_verts; P.chunks = chunks; P.W = W; P.tex_h = a->tex_h; P.tex_w = a->tex_w;
    P.iuv = a->iuv; P.rgb = a->rgb; P.depth = a->depth; P.pix_to_face = a->pix_to_face; P.bary = a->bary; P.iuv_train = a->iuv_train;
    hipLaunchKernelGGL(render_raster_kernel, dim3(tiles, tiles, B), dim3(64), 0, st, P);
    return check_launch("hps_render (rasterise)");
}
