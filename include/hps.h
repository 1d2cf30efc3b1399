/*
 * hps.h -- C ABI of libhps.so: the MI355X (gfx950) hot path of HierarchicalProbabilistic3DHuman.
 *
 * The reference is pure Python and has no FFI layer; these entry points are what a
 * binding for its per-image inference path would call.  Each declaration cites the reference
 * code (file:line, relative to the reference repo) whose arithmetic it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; row-major contiguous fp32
 *     (int32 for indices); the caller owns all memory (PyTorch tensors in the shipped binding);
 *   - stream is a hipStream_t passed as void*; calls only enqueue work (no allocation, no synchronisation, no host round
 *     trip) -- with three documented exceptions: hps_head_pose_levels in its host-LAPACK parity mode (it waits for each
 *     kinematic level's matrices: svd_mode HPS_SVD_HOST), hps_host_svd3_packed (a host routine) and
 *     hps_host_bind_lapack (dlopen, once per process);
 *   - return value: 0 on success, otherwise a hipError_t value (> 0) or a negative HPS_E_* code;
 *     hps_last_error() returns a thread-local description of the last failure;
 *   - no behaviour-changing global state: the library has no tuning switches (those live in libhps_dev.so,
 *     include/hps_dev.h).  What IS process-global: the LAPACK routine bound by hps_host_bind_lapack, the host-SVD worker pool
 *     it feeds, and one-time per-kernel attribute grants (LDS above 64 KiB) -- none alters results.  Safe to call from several
 *     host threads on different streams;
 *   - workspace sizes come from hps_query_workspace (nothing is allocated inside the library).
 */
#ifndef HPS_H_
#define HPS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The libraries are built with -fvisibility=hidden: what is declared between this push and the pop at the end of the header is
 * the complete dynamic symbol table of the shared object (tests/test_capi_symbols.py compares it with `nm -D`). */
#pragma GCC visibility push(default)

typedef void* hps_stream_t; /* hipStream_t */

/* Entry points the package's own inference path no longer calls (round 6).  They stay exported, tested on every GPU run and
 * supported -- each is the bit-level partner or the general form of the one that replaced it -- but a new caller should start
 * from the replacement:
 *   hps_stem_winograd + hps_maxpool3x3s2_pad      -> hps_stem_winograd_pooled_nchw (max pool in the stem's epilogue, windows gathered
 *                                                    from the NCHW input); hps_stem_phase_split + hps_stem_winograd_pooled remain the
 *                                                    route of callers that write the phase frames themselves (hps_proxy_rep_phase_frames)
 *   hps_smpl_mesh_fused (no side output)          -> hps_smpl_mesh_fused_picks; with shared shapes (use_mean_shape)
 *                                                    hps_smpl_v_shaped + hps_smpl_mesh_fused_shared_shape
 *   hps_smpl_blend + hps_smpl_lbs                 -> the fused forms (the pair remains SURVEY 8(d)'s definition of the LBS kernel and the
 *                                                    route for skinning weights with more than 12 influences)
 *   one hps_conv2d_bn_act_pad call for a block's
 *   1x1/2 down-sample                             -> hps_conv2d_bn_act_pad_down (rides in the 3x3/2 convolution's launch)
 *   two hps_conv2d_bn_act_pad calls for a
 *   Bottleneck entry's down-sample and conv3      -> hps_bottleneck_expand_down (the identity's tile stays in registers)
 *   hps_nchw_to_padded_nhwc (+ row-mode stem)     -> the Winograd stem for the released model's shapes; the relayout + direct stem remain
 *                                                    the route of every other (C, H, W) and of the latency mode */

#define HPS_OK 0
#define HPS_E_BADARG (-1)      /* null pointer / size out of range */
#define HPS_E_UNSUPPORTED (-2) /* shape not implemented by this build */

#define HPS_SVD_HOST 0       /* host LAPACK sgesdd (the reference's own routine) */
#define HPS_SVD_DEVICE 1     /* in-kernel SVD that follows sgesdd step by step, rounding flavour HPS_SVD_ROUNDING_REFERENCE */
#define HPS_SVD_DEVICE_FMA 2 /* the same with rounding flavour HPS_SVD_ROUNDING_FMA */

/* Rounding flavours of the in-kernel SVD (csrc/svd3_gesdd.h).  The reference runs torch.svd = MKL sgesdd on the host
 * (models/poseMF_shapeGaussian_net.py:137), and MKL picks its kernels by the host CPU: on Intel hosts they use fused
 * multiply-adds, elsewhere they round like reference BLAS.  Each flavour reproduces one of them BIT FOR BIT (U, S, V of
 * 10^6 matrices of 22 families, tests/test_host_logic.py); between the two, one matrix in 10^4 comes out with a differently
 * signed singular-vector pair.  hps_host_svd_flavor() tells which one the LAPACK bound to this process matches. */
#define HPS_SVD_ROUNDING_REFERENCE 0
#define HPS_SVD_ROUNDING_FMA 1
/* OR'ed into the svd_flavor of hps_head_joint_level_svd / the svd_mode of hps_head_pose_levels (device modes): 1024-thread
 * workgroups with eight K slices for the joint MLPs instead of 256 threads with two -- the latency form for one or a few images
 * (a level 28 -> 21 us at batch 1), too large a footprint beside the chip-filling kernels of the pipelined loop.  The hidden
 * layer's partial sums are then added in another order: results differ in the last bits, so this is a property of the model
 * (PoseMFShapeGaussianNet.set_latency_mode), never of the batch. */
#define HPS_HEAD_WIDE_WORKGROUPS 0x100

#define HPS_ACT_NONE 0
#define HPS_ACT_ELU 1
#define HPS_ACT_RELU 2

int hps_version(void);
const char* hps_last_error(void);

/* Spatial partition of the chip for kernels that cannot usefully time-share it (no reference counterpart: the reference runs
 * one kernel at a time).  Creates a HIP stream restricted to CUs [first_cu, first_cu + num_cus) of EVERY XCD (0 <= first_cu,
 * first_cu + num_cus <= 32 on MI355X: 8 XCDs x 32 CUs); destroy it with hps_stream_destroy.  Used by the step pipeline for
 * small batches: the encoder's persistent 512-register Winograd workgroups need a CU to themselves and starve beside a kernel
 * whose small workgroups keep refilling every CU; on a CU subset of their own they do not.
 * Host call; allocates a stream (the one exception to "the library never allocates"). */
int hps_stream_create_cu_partition(int first_cu, int num_cus, hps_stream_t* stream_out);
int hps_stream_destroy(hps_stream_t stream);

/* Scratch / workspace sizes in BYTES for the buffers the caller hands to the entry points below (the library never allocates):
 *   HPS_WS_CONV_SPLITK (d0 = ksplit, d1 = B*Ho*Wo, d2 = Cout)  splitk_ws of hps_conv2d_bn_act_pad (0 when ksplit <= 1)
 *   HPS_WS_SMPL_MP     (d0 = M)                                 NOT bytes: the padded mesh count mp (M rounded up to 128)
 *   HPS_WS_SMPL_XT     (d0 = M, d1 = kp)                        xt of hps_smpl_pose_prep: kp * mp floats
 *   HPS_WS_SMPL_A      (d0 = M, d1 = num_joints)                a of hps_smpl_pose_prep: M * J * 12 floats
 *   HPS_WS_SMPL_VPOSED (d0 = M, d1 = V)                         v_posed of the unfused hps_smpl_blend with 128-byte aligned rows
 *   HPS_WS_HEAD_F      (d0 = B, d1 = largest level size)        f_level_dev / f_host_pinned of hps_head_pose_levels
 *   HPS_WS_HEAD_USV    (d0 = B, d1 = largest level size)        usv_level_dev / usv_host_pinned of hps_head_pose_levels
 *   HPS_WS_MF_LOSS     (d0 = n_pose)                            workspace of hps_mf_loss_forward / hps_mf_loss_backward
 *   HPS_WS_SMPL_LBS_BWD   (d0 = M, d1 = V, d2 = num_joints)     workspace of hps_smpl_lbs_backward (per-chunk partial sums of g_a)
 *   HPS_WS_SMPL_BLEND_BWD (d0 = M, d1 = kp, d2 = np)            workspace of hps_smpl_blend_backward (per-slice partial sums of g_xt)
 *   HPS_WS_HEAD_LEVELS_BWD (d0 = B, d1 = total_in, d2 = num_body_joints)  workspace of hps_head_pose_levels_backward
 *   HPS_WS_HEAD_TRUNK_BWD  (d0 = B, d1 = num_feats + hidden + embed_dim, d2 = 2 num_shape + num_glob + num_cam)
 *                                                               workspace of hps_head_trunk_backward
 *   HPS_WS_SEG_BBOX    (d0 = B)                                 ws of hps_seg_bbox_affine (per-chunk integer box corners)
 *   HPS_WS_RENDER      (d0 = B, d1 = DensePose vertices, d2 = faces)  workspace of hps_render
 *   HPS_WS_SILHOUETTE  (d0 = M, d1 = DensePose vertices, d2 = HPS_WS_SILHOUETTE_D2(faces, W))  workspace of hps_silhouette_iou
 *   HPS_WS_TRAIN_METRICS (d0 = B)                               workspace of hps_train_metrics_update
 *   HPS_WS_PNG         (d0 = H, d1 = W, d2 = C)                 a picture's workspace of hps_png_encode (-1 outside the supported range)
 *   HPS_WS_JPEG        (d0 = scan_length, d1 = HPS_WS_JPEG_D1(width, height), d2 = HPS_WS_JPEG_D2(ncomp, hs, vs, restart_interval))
 *                                                               a file's workspace of hps_jpeg_decode, good for every subseq_bits
 *                                                               (-1 outside the supported range)
 *   HPS_WS_JPEG_ENC    (d0 = H, d1 = W, d2 = HPS_WS_JPEG_ENC_D2(C, sampling))  a picture's workspace of hps_jpeg_encode (-1 outside the
 *                                                               supported range)
 * Unused dims are ignored.  Returns -1 (and sets hps_last_error) for an unknown `what` or negative dims. */
enum { HPS_WS_CONV_SPLITK = 0, HPS_WS_SMPL_MP = 1, HPS_WS_SMPL_XT = 2, HPS_WS_SMPL_A = 3, HPS_WS_SMPL_VPOSED = 4,
       HPS_WS_HEAD_F = 5, HPS_WS_HEAD_USV = 6, HPS_WS_MF_LOSS = 8, HPS_WS_SMPL_LBS_BWD = 9, HPS_WS_SMPL_BLEND_BWD = 10,
       HPS_WS_HEAD_LEVELS_BWD = 11, HPS_WS_HEAD_TRUNK_BWD = 12, HPS_WS_SEG_BBOX = 13, HPS_WS_RENDER = 14,
       HPS_WS_SILHOUETTE = 15, HPS_WS_TRAIN_METRICS = 16, HPS_WS_PNG = 17, HPS_WS_JPEG = 18, HPS_WS_JPEG_ENC = 19 };
#define HPS_WS_JPEG_D1(width, height) ((int64_t)(width) + ((int64_t)(height) << 32))
#define HPS_WS_JPEG_D2(ncomp, hs, vs, restart_interval) ((int64_t)(ncomp) + ((int64_t)(hs) << 8) + ((int64_t)(vs) << 16) + ((int64_t)(restart_interval) << 32))
#define HPS_WS_JPEG_ENC_D2(C, sampling) ((int64_t)(C) + ((int64_t)(sampling) << 8))
int64_t hps_query_workspace(int what, int64_t d0, int64_t d1, int64_t d2);

/* ------------------------------------------------------------------------------------------
 * SMPL forward  (models/smpl_official.py:27-41 -> smplx 0.1.26 SMPL.forward / lbs)
 * ---------------------------------------------------------------------------------------- */

/* Rodrigues / rest joints / forward kinematics / blend-GEMM operand, one launch.
 *   glob, body : global_orient and body_pose of M meshes; rotation matrices (M,1,3,3)/(M,J-1,3,3)
 *                if is_rotmat != 0 (pose2rot=False), else axis-angle (M,3)/(M,(J-1)*3) converted by
 *                smplx batch_rodrigues (angle = ||r + 1e-8||).
 *   betas      : (M, num_betas).
 *   j_template : (J,3)   = J_regressor @ v_template          } joint regression folded through the
 *   j_shapedirs: (J,3,nb)= J_regressor @ shapedirs           } linear shape blend (exact algebra)
 *   parents    : (J,) int32, parents[0] = -1;  depth: (J,) int32 tree depth of each joint.
 * outputs
 *   xt   : (kp, mp) blend-GEMM operand, k-major: rows [0,nb) betas, [nb, nb+9(J-1)) pose feature
 *          (R_j - I, j = 1..J-1), remaining rows zero.  Only columns < M are written.
 *   a    : (M,J,12) skinning transforms, top 3 rows of smplx's "A" (world transform with the rest
 *          pose removed), row-major 3x4.
 *   j_posed : (M,J,3) posed joint locations.   rot_out: optional (M,J,3,3) rotation matrices used.
 */
int hps_smpl_pose_prep(const float* glob, const float* body, int is_rotmat, const float* betas,
                       int num_betas, const float* j_template, const float* j_shapedirs,
                       const int32_t* parents, const int32_t* depth, int num_joints, float* xt,
                       int kp, int mp, float* a, float* j_posed, float* rot_out, int M,
                       hps_stream_t stream);

/* Shape + pose blend shapes as one fp32-MFMA GEMM:
 *   v_posed[m, n] = v_template[n] + sum_k xt[k, m] * bmat[k, n]      (n = 3*vertex + coord)
 * bmat: (kp, np) = [shapedirs ; posedirs ; 0] with np = N rounded up to 128 (zero padded),
 * xt: (kp, mp) from hps_smpl_pose_prep, mp = M rounded up to 128, kp a multiple of 16.
 * v_posed rows have pitch ld_out floats (>= N; a multiple of 32 keeps every 128-byte store segment line-aligned).
 * Replaces lbs steps (1) and (3): blend_shapes einsum + pose_feature @ posedirs. */
int hps_smpl_blend(const float* xt, const float* bmat, const float* v_template, float* v_posed,
                   int M, int N, int kp, int mp, int np, int ld_out, hps_stream_t stream);

/* Linear blend skinning, lbs step (5):  verts[m,v] = (sum_k w[v,k] * A[m, idx[v,k]]) . [v_posed[m,v]; 1]
 * Skinning weights in compressed form: w_idx/w_val (V, K) -- the K largest-support entries of each
 * row of lbs_weights, padded with (0, 0.0f); exact for any model with <= K non-zeros per row.
 * v_posed rows have pitch ld_vposed floats (>= 3 V); verts is contiguous (M,V,3) like the reference's output.
 * transl: optional (M,3) added to the result (smplx SMPL.forward step (7)), may be NULL.
 * Algorithmic HBM bytes per mesh: 12 V (v_posed) + 48 J.. (A) + 12 V (verts); SURVEY section 8(d). */
int hps_smpl_lbs(const float* v_posed, int ld_vposed, const float* a, const int32_t* w_idx,
                 const float* w_val, int K, int num_joints, const float* transl, float* verts, int M,
                 int V, hps_stream_t stream);

/* Fused blend shapes + linear blend skinning: lbs steps (1), (3), (5) in ONE kernel -- the blend GEMM tile stays in the
 * MFMA accumulators and is skinned in the epilogue, so v_posed never exists in HBM (the product path of SMPL.forward;
 * hps_smpl_blend + hps_smpl_lbs remain as the unfused definition the LBS roofline bytes of SURVEY section 8(d) refer to).
 *   verts[m,v] = (sum_k w[v,k] A[m, idx[v,k]]) . [v_template[v] + sum_k xt[k,m] bmat_p[k, col(v,c)]; 1] (+ transl[m])
 * bmat_p: the blend matrix of hps_smpl_blend with PANEL-PERMUTED columns, (kp, np) k-major, np = hps_smpl_mesh_fused_np(V):
 *   col(v, c) = (v / 64) * 192 + c * 64 + v % 64  (x, y, z of a 64-vertex panel as three 64-wide column groups),
 *   unused columns zero.  kp here = the K rows that carry data, rounded up to EVEN (SMPL: 10 + 207 -> 218); both operands must be
 *   allocated (and zero) up to the next multiple of 16 rows -- what hps_smpl_pose_prep / hps_smpl_blend call kp (224): the rows
 *   behind kp are not multiplied.  xt, a: from hps_smpl_pose_prep (mp a multiple of 64 covering M).  w_idx / w_val / K / transl /
 *   verts as for hps_smpl_lbs.  Bit-identical to hps_smpl_blend followed by hps_smpl_lbs (same MFMA k order, same
 *   skinning arithmetic: the skipped rows are zeros).  Bound: fp32 MFMA, 2 * kp * 3 V FLOP per mesh; HBM traffic = the 12 V bytes of verts per mesh.
 * Instantiated where it needs no scratch memory beside four workgroups per CU: K = 4 with any num_joints in 1..32, K = 8 and
 * 12 with num_joints = 24; other combinations (e.g. K = 24, dense skinning weights) return HPS_E_UNSUPPORTED -- take the
 * unfused pair, which gives the same bits.
 * Replaces smplx 0.1.26 lbs (reached from models/smpl_official.py:29) steps blend_shapes, pose_feature @ posedirs,
 * W @ A and T @ v_posed. */
int hps_smpl_mesh_fused(const float* xt, const float* bmat_p, const float* v_template, const float* a,
                        const int32_t* w_idx, const float* w_val, int K, int num_joints, const float* transl,
                        float* verts, int M, int V, int kp, int mp, int np, hps_stream_t stream);
/* hps_smpl_mesh_fused with a side output for the joint regression (round 5): pick_slot (V,) int32 gives every vertex its slot in a
 * compact array or -1, and the lane that skins a vertex with a slot also writes it to picked (M, n_picked, 3).  hps_smpl_joints then
 * runs on `picked` (verts = picked, V = n_picked, csr_col = the entries' SLOTS): the same sums over the same values, read from
 * 12 n_picked contiguous bytes per mesh instead of gathered from the whole mesh (SMPL: 276 entries on 198 distinct vertices; the gather
 * was bound by its request rate, 60 us per 6 528 meshes).  Exists for the SMPL configuration (K = 4, 24 joints, kp = 218):
 * HPS_E_UNSUPPORTED otherwise -- use hps_smpl_mesh_fused and gather. */
int hps_smpl_mesh_fused_picks(const float* xt, const float* bmat_p, const float* v_template, const float* a,
                              const int32_t* w_idx, const float* w_val, int K, int num_joints, const float* transl,
                              float* verts, int M, int V, int kp, int mp, int np, const int32_t* pick_slot, float* picked,
                              int n_picked, hps_stream_t stream);
/* The fused mesh kernel for meshes that SHARE their shape (round 6): every mesh of an image carries the image's betas
 * (use_mean_shape = True, the reference's predict default: utils/sampling_utils.py:178-179, predict/...:157-165).  smplx lbs step (1),
 * v_shaped = v_template + blend_shapes(betas), is then formed ONCE per distinct shape (hps_smpl_v_shaped: R = images, not meshes) and
 * the GEMM keeps the 207 pose rows only: xt_pose / bmat_p_pose = the operands of hps_smpl_mesh_fused advanced by num_betas rows, kp =
 * 208 (thirteen whole K chunks: 312 MFMAs per wave against 327), v_posed = v_shaped[row of the mesh] + pose blend -- smplx's own
 * order of the two additions (v_posed = v_shaped + pose_offsets).  The K = 217 form adds template, shape and pose terms in one MFMA
 * chain, so the two agree to rounding, not bit for bit (both within 2e-5 m of the oracle).
 *   v_shaped (R, V, 3); mesh_row (mp,) int32: the row of v_shaped of every mesh (padding meshes: any valid row);
 *   group_rows (mp / 32, 3) int32 per group of 32 consecutive meshes: (row A, row B, split) -- local mesh < split has row A, the
 *   others row B; split = -1: more than two rows in the group, its lanes fetch per mesh through mesh_row.
 * Exists for the SMPL configuration with the side output (K = 4, 24 joints, kp = 208, no translation); HPS_E_UNSUPPORTED otherwise. */
int hps_smpl_mesh_fused_shared_shape(const float* xt_pose, const float* bmat_p_pose, const float* v_shaped,
                                     const int32_t* mesh_row, const int32_t* group_rows, const float* a,
                                     const int32_t* w_idx, const float* w_val, int K, int num_joints, float* verts, int M,
                                     int V, int kp, int mp, int np, const int32_t* pick_slot, float* picked,
                                     int n_picked, hps_stream_t stream);
/* smplx lbs step (1) for R distinct shapes: v_shaped[r, n] = v_template[n] + sum_l betas[r, l] * shape_rows[l * ld + n], n = 3 v + c
 * (shape_rows: the first num_betas rows of the blend matrix of hps_smpl_blend, row pitch ld >= 3 V floats). */
int hps_smpl_v_shaped(const float* betas, int num_betas, const float* shape_rows, int ld, const float* v_template,
                      float* v_shaped, int R, int V, hps_stream_t stream);
/* The shared-shape mesh kernel with its pose blend GEMM on the bf16 matrix pipe AT FP32 ACCURACY ("bf16x3", round 6, opt-in:
 * SMPL.mesh_arith).  Every fp32 operand x is carried as three bf16 pieces x = x1 + x2 + x3 (x1 = RN(x), x2 = RN(x - x1), x3 = RN(x - x1 -
 * x2): 3 x 8 significand bits = fp32's 24, the sum is exact for 2^-110 <= |x| < 3.39e38, where all pieces are normal and finite) and a product is formed as the six piece products of weight >= 2^-16 of
 * the leading one, each exact in the fp32 accumulator; the dropped part is < 2^-23 |a b| -- one fp32 rounding.  Same tile, mapping,
 * skinning arithmetic, side output and HBM traffic as hps_smpl_mesh_fused_shared_shape; the vertices agree with it to rounding (<= 4e-6
 * m asserted; both within 2e-5 m of the oracle and equally close to the float64 twin).  Why it exists: v_mfma_f32_32x32x2_f32 runs at
 * the fp32 vector rate on gfx950 and excludes fp32 VALU work, v_mfma_f32_32x32x16_bf16 is 16 x faster and does not.
 *   hps_smpl_split_bf16x3: src (rows, ld) fp32 k-major (rows behind `rows` up to the next multiple of 16 are written as zeros), its
 *     first `cols` columns in tiles of tile_cols (hps_smpl_split_bf16x3_mesh_tile(): the mesh operand xt of hps_smpl_pose_prep advanced by num_betas rows; 192: bmat_p
 *     advanced likewise) -> dst[tile][16-row chunk][piece][k half][column][8 bf16], hps_smpl_split_bf16x3_bytes(rows, cols) bytes.
 *     The blend matrix is split once per model, the mesh operand once per call.
 *   hps_smpl_mesh_fused_shared_shape_bf16x3: xsplit / bsplit from the above (rows = 207 for SMPL); everything else as for
 *     hps_smpl_mesh_fused_shared_shape.  K = 4, 24 joints; HPS_E_UNSUPPORTED otherwise.  Meshes that do NOT share shapes take the same
 *     entry point with the operands split from row 0 (rows = num_betas + 207: the shape blend inside the GEMM, as in
 *     hps_smpl_mesh_fused), v_shaped = v_template (one row), mesh_row all 0 and every group (0, 0, 32) -- what SMPL.forward does. */
size_t hps_smpl_split_bf16x3_bytes(int rows, int cols);
int hps_smpl_split_bf16x3_mesh_tile(void);   /* tile_cols of the mesh operand = meshes per workgroup tile of the kernel (128) */
int hps_smpl_split_bf16x3(const float* src, int rows, int ld, int cols, int tile_cols, void* dst, hps_stream_t stream);
int hps_smpl_mesh_fused_shared_shape_bf16x3(const void* xsplit, const void* bsplit, const float* v_shaped, const int32_t* mesh_row,
                                            const int32_t* group_rows, const float* a, const int32_t* w_idx, const float* w_val,
                                            int K, int num_joints, float* verts, int M, int V, int rows, int mp,
                                            const int32_t* pick_slot, float* picked, int n_picked, hps_stream_t stream);
/* Column count of bmat_p for a model with V vertices (192 per started panel of 64 vertices). */
int hps_smpl_mesh_fused_np(int V);

/* hps_smpl_joints on the compact side output of hps_smpl_mesh_fused_picks / _shared_shape (picked (M, n_picked, 3), csr_slot = the
 * entries' slots) AND hps_vertex_uncertainty on the call's sample meshes (verts_samples (B, N, V, 3), 8 <= N <= 128) in ONE launch:
 * the two read what the mesh kernel has just written and do not depend on each other (predict/...:112-165: the joints of every mesh,
 * utils/sampling_utils.py:189-190: the per-vertex uncertainty).  Identical bits to the two calls; HPS_E_UNSUPPORTED for other N. */
int hps_joints_and_uncertainty(const float* picked, const float* j_posed, const int32_t* csr_ptr, const int32_t* csr_slot,
                               const float* csr_val, int n_rows, int num_joints, const float* transl, float* joints, int M,
                               int n_picked, const float* verts_samples, float* unc, int B, int N, int V, hps_stream_t stream);

/* Joints: out[m, 0:J] = j_posed[m] ; out[m, J + r] = sum_e csr_val[e] * verts[m, csr_col[e]]
 * for CSR rows r = 0..n_rows-1 (the 21 smplx vertex picks as 1-entry rows, then the extra / cocoplus /
 * h36m regressors of models/smpl_official.py:30-34), each row summed as one chain of fused multiply-adds in entry order.
 * transl optional (M,3). out: (M, J+n_rows, 3). */
int hps_smpl_joints(const float* verts, const float* j_posed, const int32_t* csr_ptr,
                    const int32_t* csr_col, const float* csr_val, int n_rows, int num_joints,
                    const float* transl, float* joints, int M, int V, hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SMPL backward  (the reference differentiates its SMPL with torch autograd: train/train_poseMF_shapeGaussian_net.py:268-271
 * mode mesh, :304-308 sample meshes of which only .joints is used, loss at :346)
 * ----------------------------------------------------------------------------------------
 * Cotangents: g_verts (M,V,3) of the vertices and g_joints (M, num_joints + n_rows, 3) of hps_smpl_joints' output; either may be
 * NULL.  With C the CSR matrix of hps_smpl_joints:  gV' = g_verts + C^T g_joints[num_joints:].  The three calls run in this order
 * on what hps_smpl_pose_prep (xt, a) and hps_smpl_blend (v_posed) recompute from the forward's inputs.  Every reduction is
 * per-workgroup partial sums in `workspace` added in a fixed order by a second launch: no floating-point atomics, bitwise
 * repeatable, and a mesh's result does not depend on M. */

/* Backward of hps_smpl_lbs / the skinning epilogue of the fused kernels (smplx 0.1.26 lbs: T = W @ A, v_homo = T @ v_posed_homo)
 * and of the translation (SMPL.forward: vertices + transl, joints + transl), with T_v = sum_k w_val[v,k] A[w_idx[v,k]]:
 *   v_posed[m, 3v..] <- g_vposed_v = T_v.R^T gV'_v   IN PLACE (the lane that reads v_posed_v writes g_vposed_v); the columns
 *                       [3V, ld_vposed) of every row are written as zeros (hps_smpl_blend_backward contracts over them)
 *   g_a (M,J,12)      : g_a[j].R = sum_v W[v,j] gV'_v (x) v_posed_v,  g_a[j].t = sum_v W[v,j] gV'_v   (row-major 3x4 like a)
 *   g_transl (M,3)    : sum_v gV'_v + sum_{j < num_joints} g_joints[j] (the partial sums are added in float64 and rounded once);
 *                       optional (NULL: not wanted)
 * csrt_ptr (V+1,), csrt_row, csrt_val: C^T in CSR form over the V vertices (entries of a vertex in the order of C's rows);
 * needed with g_joints only.  The vertex sums run as v_mfma_f32_32x32x2_f32 products (rows = joints, columns = two meshes' 12
 * entries) over chunks of 128 vertices; workspace: hps_query_workspace(HPS_WS_SMPL_LBS_BWD, M, V, num_joints) bytes.
 * K = 4, 8, 12, 24; num_joints <= 31; n_rows <= 96 (HPS_E_UNSUPPORTED beyond).  V may be any vertex subset with its own w_idx / w_val / csrt (the joints-only route:
 * the distinct regressor vertices). */
int hps_smpl_lbs_backward(float* v_posed, int ld_vposed, const float* a, const int32_t* w_idx, const float* w_val, int K,
                          int num_joints, const float* g_verts, const float* g_joints, int n_rows, const int32_t* csrt_ptr,
                          const int32_t* csrt_row, const float* csrt_val, float* g_a, float* g_transl, float* workspace, int M,
                          int V, hps_stream_t stream);

/* Backward of hps_smpl_blend / the GEMM of the fused kernels (smplx lbs: blend_shapes einsum 'bl,mkl->bmk' and
 * torch.matmul(pose_feature, posedirs)) with respect to its mesh operand:
 *   g_xt[k, m] = sum_n bmat[k, n] * g_vposed[m, n]      k < kp; columns m in [M, mp) are written as zeros
 * rows [0, num_betas) are the direct shape gradient, the following 9 (J - 1) rows the pose-feature gradient.  bmat (kp, np) as
 * for hps_smpl_blend (np a multiple of 128, zero padded), g_vposed (M, ld_g) with ld_g >= np, a multiple of 4, and FINITE values
 * in its padding columns (hps_smpl_lbs_backward leaves zeros); mp = M rounded up to 128.  fp32 MFMA, the forward blend's
 * 2 kp np FLOP per mesh; the contraction is cut into slices of 512 columns (a workgroup = one slice x 128 meshes, so small M
 * still spreads over np / 512 workgroups) whose partial sums are added in slice order.
 * workspace: hps_query_workspace(HPS_WS_SMPL_BLEND_BWD, M, kp, np) bytes. */
int hps_smpl_blend_backward(const float* bmat, const float* g_vposed, float* g_xt, float* workspace, int M, int kp, int mp,
                            int np, int ld_g, hps_stream_t stream);

/* Backward of hps_smpl_pose_prep (smplx lbs: batch_rodrigues, vertices2joints folded into j_template / j_shapedirs, pose_feature,
 * batch_rigid_transform).  glob .. num_joints: the forward's inputs (it recomputes rotations, rest joints and world transforms).
 * g_a (M,J,12) from hps_smpl_lbs_backward; g_joints (M, num_joints + n_rows, 3) or NULL: its first num_joints rows are the
 * cotangent of j_posed; g_xt (kp, mp) from hps_smpl_blend_backward or NULL.  Walks the kinematic levels from the leaves to the root.
 *   g_glob, g_body : shaped like glob / body.  is_rotmat: 9 values per joint, the derivative with respect to the unconstrained matrix
 *                    entries (what torch autograd gives); otherwise 3 per joint through batch_rodrigues including its
 *                    angle = ||r + 1e-8|| (finite at r = 0).  Either may be NULL.
 *   g_betas (M, num_betas) = g_xt[:num_betas]^T + j_shapedirs^T g_J, optional. */
int hps_smpl_pose_prep_backward(const float* glob, const float* body, int is_rotmat, const float* betas, int num_betas,
                                const float* j_template, const float* j_shapedirs, const int32_t* parents, const int32_t* depth,
                                int num_joints, const float* g_a, const float* g_joints, int n_rows, const float* g_xt, int mp,
                                float* g_glob, float* g_body, float* g_betas, int M, hps_stream_t stream);

/* Per-vertex uncertainty of utils/sampling_utils.py:189-190, batched over images:
 * verts (B,N,V,3) -> unc (B,V) = mean_s || verts[b,s,v] - mean_s' verts[b,s',v] ||. */
int hps_vertex_uncertainty(const float* verts, float* unc, int B, int N, int V, hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Matrix-Fisher sampling  (utils/sampling_utils.py:10-143)
 * ---------------------------------------------------------------------------------------- */

/* One workgroup (1-8 wavefronts, chosen from num_samples alone; results do not depend on it) per (image, joint) call
 * c = image*num_joints + joint, C calls in total.
 * pose_u/pose_v (C,3,3), pose_s (C,3): raw SVD factors; the proper-SVD fix (:104-111), Bingham A,
 * ACG Omega, Gaussian std (:118-124), the 8N-proposal rejection test (:51-61), in-order compaction
 * of the first N accepted proposals (:64-65), quat_to_rotmat (:139) and U_p R V_p^T (:140-141) are
 * all done in the kernel.  r_out is (B, N, num_joints, 3, 3); quat_out optional (B,N,num_joints,4).
 * A round is decided once N proposals have been accepted: the proposals behind the N-th accept (the reference evaluates all
 * 8N, :51-61, and then keeps the first N accepted) are not evaluated -- the same N samples.
 * accepted (C,) int32 receives the number of accepted proposals of the round that was used, counted up to the iteration
 * that reached N (>= N on success); with quat_out != NULL (the Bingham entry point, whose accept_ratio :67 needs it) the
 * round's total over all n_prop proposals.
 * bingham_a: optional (C,4) Bingham parameter used instead of the one derived from pose_s -- the
 * entry point of bingham_sampling_for_matrix_fisher_torch (:10-71), which takes A directly.
 * acg_override: optional (C,8) = [Omega (4) | Gaussian_std (4)] used instead of the values derived from A and b
 * (:42-45 make those only the DEFAULTS of the reference's entry point; m_star is always the caller's).
 *
 * Noise source
 *   eps/w != NULL : proposals come from host-drawn noise, eps (D, n_prop, 4) standard normals and
 *                   w (D, n_prop) uniforms (the reference's torch.randn / torch.rand stream, :51/:60);
 *                   call c reads draw slot draw_idx[c].  A call with fewer than N accepted proposals
 *                   reports accepted[c] < N and its outputs are to be discarded (the caller retries with
 *                   the next draw, as the reference does at :68-69).
 *   eps == NULL   : counter-based Philox4x32-10 in the kernel, keyed by (seed, call_offset + c,
 *                   round, proposal) so results do not depend on how images are sharded over GPUs.
 *                   Seeded results are part of the contract; the layout, with g = call_offset + c:
 *                     key     = (seed bits 0..31, seed bits 32..63)
 *                     counter = (proposal, round, g bits 0..31, g bits 32..62 | block << 31)
 *                     block 0 : words (x, y) -> the normals (e0, e1), words (z, w) -> (e2, e3) by Box-Muller,
 *                               radius sqrt(-2 ln u), u = ((a >> 8) + 1) / 2^24 in (0, 1] from the pair's first word a,
 *                               angle 2 pi v, v = (b >> 8) / 2^24 in [0, 1) from its second word b, (cos, sin)
 *                     block 1 : word x -> the acceptance uniform (x >> 8) / 2^24 in [0, 1); words y, z, w unused
 *                   (bit 63 of g does not reach the counter).  Pinned word for word by tests/test_gpu_philox.py against the
 *                   host replica tests/philox_replica.py; a change of this layout changes every user's seeded samples and
 *                   is an ABI change.
 *                   rounds are redrawn in-kernel until N proposals are accepted; a call that exhausts
 *                   max_rounds (non-finite concentrations) gets NaN outputs and accepted[c] < N.
 *                   seed_dev (optional, device, two uint64: seed, call_offset) overrides the by-value pair: a launch captured in
 *                   a hipGraph reads its key at run time, so every replay draws new samples.
 */
int hps_mf_sample(const float* pose_u, const float* pose_s, const float* pose_v,
                  const float* bingham_a, const float* acg_override, int C, int num_joints, int num_samples, int n_prop,
                  float b, float m_star,
                  const float* eps, const float* w, const int32_t* draw_idx, uint64_t seed,
                  int64_t call_offset, const uint64_t* seed_dev, int max_rounds, float* r_out, float* quat_out,
                  int32_t* accepted, hps_stream_t stream);

/* The training route of the sampler (utils/sampling_utils.py:21, 51-53, 103-141 under autograd; the stage-2 step,
 * train/train_poseMF_shapeGaussian_net.py:292-320).
 * hps_mf_sample_keep_quat: the launch of hps_mf_sample(bingham_a = acg_override = seed_dev = NULL) -- the same r_out and accepted
 * bit for bit on both noise routes -- that also writes the accepted unit quaternions quat_out (B, N, J-1, 4) in the order of r_out,
 * WITHOUT hps_mf_sample's count_all (there a non-NULL quat_out makes every round evaluate all n_prop proposals for the Bingham entry
 * point's accept ratio, :67): the round is decided at the N-th accept. */
int hps_mf_sample_keep_quat(const float* pose_u, const float* pose_s, const float* pose_v, int C, int num_joints, int num_samples,
                            int n_prop, float b, float m_star, const float* eps, const float* w, const int32_t* draw_idx,
                            uint64_t seed, int64_t call_offset, int max_rounds, float* r_out, float* quat_out, int32_t* accepted,
                            hps_stream_t stream);

/* The reparameterised sampler differentiated, one launch: what torch autograd computes for :52-53 (y = Gaussian_std * eps,
 * q = y / ||y||), :105-111 (proper fix, det U and det V constants), :119-124 (A, Omega, Gaussian_std from pose_S) and :139-141
 * (R = U_p quat_to_rotmat(q) V_p^T, utils/rigid_transform_utils.py:113-133 with its renormalisation); the accept test (:55-62) is
 * under no_grad.  Inputs: the forward's pose_u / pose_s / pose_v (C = B (J-1) calls), quat (B, N, J-1, 4) from
 * hps_mf_sample_keep_quat, g_r (B, N, J-1, 3, 3) the cotangent of r_out.  No noise is needed: ||y|| cancels,
 * g_sigma_i = sum_n q_i (g_q_i - q_i <q, g_q>) / sigma_i.  Outputs (each may be NULL = not wanted, not written): g_pose_u (C, 3, 3),
 * g_pose_s (C, 3), g_pose_v (C, 3, 3), cotangents of the RAW factors.  float64 sums over the samples in one fixed order that depends
 * on num_samples alone (no atomics): bitwise repeatable, an image's result independent of B.  NaN quaternions (a failed call) give
 * NaN gradients.  pose_u_d / pose_s_d / pose_v_d (all NULL or all given): the same factors in float64 from hps_head_forward_refine
 * (its pose_u / pose_s / pose_v outputs); the gradient is then evaluated at them -- the fp32 factors of an ill-conditioned SVD are off by
 * 2^-23 / (gap of the singular values), which the sampler's second derivative turns into gradient error -- while det U, det V stay the
 * forward's constants from the fp32 factors. */
int hps_mf_sample_backward(const float* pose_u, const float* pose_s, const float* pose_v, const double* pose_u_d,
                           const double* pose_s_d, const double* pose_v_d, const float* quat, const float* g_r, int C, int num_joints,
                           int num_samples, float b, float* g_pose_u, float* g_pose_s, float* g_pose_v, hps_stream_t stream);

/* Inputs of ONE flattened SMPL call over the M = B (N + 2) meshes [mode (B) | T-pose (B) | samples (B N)] of the inference
 * core (predict/predict_poseMF_shapeGaussian_net.py:112-115 mode mesh, :136 T-pose mesh, utils/sampling_utils.py:178-185 sample
 * meshes): body (M, J-1, 3, 3) rows [0, 2B) (mode rotations, then identities; rows [2B, M) are where hps_mf_sample wrote its
 * samples), glob_all (M, 3, 3) (glob_rotmats of the image; identity for the T-pose), betas_all (M, nb) (the shape mean of the
 * image, or betas_samples (B, N, nb) for the sample meshes if non-NULL: use_mean_shape = False, :180-181). */
int hps_infer_assemble(const float* mode, const float* glob_rotmats, const float* loc, const float* betas_samples,
                       float* body, float* glob_all, float* betas_all, int B, int N, int num_body_joints,
                       int num_betas, hps_stream_t stream);

/* utils/rigid_transform_utils.py:113-133 */
int hps_quat_to_rotmat(const float* quat, float* rotmat, int n, hps_stream_t stream);
/* utils/rigid_transform_utils.py:80-94 (cross product along dim 1 for every batch size) */
int hps_rot6d_to_rotmat(const float* x6, float* rotmat, int n, hps_stream_t stream);
/* utils/rigid_transform_utils.py:80-94 differentiated: g_x6 (n,6) from x6 (n,6) and the cotangent g_rotmat (n,3,3) of the
 * rotation matrices; the cross product runs along dim 1 for every n, as in hps_rot6d_to_rotmat. */
int hps_rot6d_to_rotmat_backward(const float* x6, const float* g_rotmat, float* g_x6, int n, hps_stream_t stream);
/* smplx.lbs.batch_rodrigues (reference import: predict/predict_poseMF_shapeGaussian_net.py:7) */
int hps_batch_rodrigues(const float* aa, float* rotmat, int n, hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Distribution-prediction head  (models/poseMF_shapeGaussian_net.py:95-162)
 * ---------------------------------------------------------------------------------------- */

/* out[b, n] = act( sum_k x[b, k] * wt[k, n] + bias[n] (+ addend[n]) ),  wt = weight^T (K,N).
 * x rows have stride ldx, out rows stride ldo (lets the trunk write straight into the fc_embed
 * input buffer).  addend optional (init_glob / init_cam, :106-107). */
int hps_linear(const float* x, int ldx, const float* wt, const float* bias, const float* addend,
               float* out, int ldo, int B, int K, int N, int act, hps_stream_t stream);

/* The FC trunk (models/poseMF_shapeGaussian_net.py:95-110) as three launches and nothing else:
 *   x      = ELU(fc1(feats))                                        x_ws (B, hidden), scratch
 *   sgc    = [fc_shape | fc_glob | fc_cam](x) + sgc_add             sgc_out (B, 2 num_shape + num_glob + num_cam): shape_params,
 *            glob + init_glob, cam + init_cam -- the tail of fc_embed's input; the same launch also writes
 *            shape_loc = mean, shape_scale = exp(log std) (the Normal of :100-101), glob, cam, each contiguous
 *   embed  = ELU(fc_embed(cat[feats, sgc]))                         the concatenation (:108) is never materialised
 * Weights pre-transposed (K, N) like hps_linear; sgc_wt / sgc_b / sgc_add = the three layers stacked (sgc_add: zeros, init_glob,
 * init_cam).  feats rows have stride ldf.  Widths: a workgroup stages the K input columns of 8 images in LDS, up to 160 KiB here
 * (K <= 4864: num_feats + 2 num_shape + num_glob + num_cam = 2077 for the ResNet-50 net; hps_linear itself keeps to 64 KiB,
 * K <= 1792); wider: HPS_E_UNSUPPORTED before any launch. */
int hps_head_trunk(const float* feats, int ldf, const float* fc1_wt, const float* fc1_b, const float* sgc_wt,
                   const float* sgc_b, const float* sgc_add, const float* embed_wt, const float* embed_b, float* x_ws,
                   float* sgc_out, float* embed, float* shape_loc, float* shape_scale, float* glob, float* cam, int B,
                   int num_feats, int hidden, int num_shape, int num_glob, int num_cam, int embed_dim, hps_stream_t stream);

/* One kinematic level of the joint loop (:121-135): for every joint g in the level
 *   in  = cat[embed(b), U_proper[b, anc].flat, S_proper[b, anc].flat, mode[b, anc].flat]
 *   F   = W2 . ELU(W1 . in + b1) + b2 + delta_i_weight * I
 * joint_ids (n_level,) int32; anc_ptr (23+1,) / anc_idx: CSR list of ancestors (nearest first);
 * w1t_ptrs[joint] -> (in_dim, hidden) = fc_pose[j].0.weight^T, b1_ptrs -> (hidden,),
 * w2_ptrs -> (9, hidden), b2_ptrs -> (9,)  (device arrays of device pointers, indexed by joint id).
 * u_proper/mode (B,23,9), s_proper (B,23,3) hold the ancestors' results; pose_f (B,23,9) output;
 * f_level: optional compact copy (B, n_level, 9) of the level's F matrices (what goes to the host SVD). */
int hps_head_joint_level(const float* embed, int embed_dim, int hidden, const int32_t* joint_ids,
                         int n_level, const int32_t* anc_ptr, const int32_t* anc_idx,
                         const float* const* w1t_ptrs, const float* const* b1_ptrs,
                         const float* const* w2_ptrs, const float* const* b2_ptrs,
                         const float* u_proper, const float* s_proper, const float* mode,
                         float delta_i_weight, float* pose_f, float* f_level, int B,
                         int num_body_joints, hps_stream_t stream);

/* hps_head_joint_level with the level's 3x3 SVDs (models/poseMF_shapeGaussian_net.py:137), the proper-SVD fix and the mode
 * (:139-152) done INSIDE the kernel: pose_u / pose_s / pose_v and u_proper / s_proper / mode rows of the level's joints are
 * written, no host round trip.  The SVD follows LAPACK's sgesdd step by step (csrc/svd3_gesdd.h) with the roundings of the
 * host's MKL (svd_flavor: HPS_SVD_ROUNDING_*), so that the factors -- and with them the signs the reference's torch.svd
 * gives the singular vectors, which are inputs of the child joints (:126-130) -- are reproduced bit for bit. */
int hps_head_joint_level_svd(const float* embed, int embed_dim, int hidden, const int32_t* joint_ids,
                             int n_level, const int32_t* anc_ptr, const int32_t* anc_idx,
                             const float* const* w1t_ptrs, const float* const* b1_ptrs,
                             const float* const* w2_ptrs, const float* const* b2_ptrs, float* u_proper,
                             float* s_proper, float* mode, float delta_i_weight, float* pose_f, float* pose_u,
                             float* pose_s, float* pose_v, int B, int num_body_joints, int svd_flavor,
                             hps_stream_t stream);

/* The same device SVD for n row-major 3x3 matrices: f (n,9) -> usv (n,21) packed [U (9) | S (3) | V (9)]; replaces
 * torch.svd(F.cpu()) (:137).  Non-finite or non-converging input (LAPACK: INFO != 0) gives NaN factors. */
int hps_svd3_packed(const float* f, float* usv, int n, int svd_flavor, hps_stream_t stream);

/* HOST function: the algorithm of hps_svd3_packed compiled for the host (single thread) -- for measuring / testing its
 * agreement with LAPACK without a GPU.  f_host (n,9) -> usv_host (n,21). */
int hps_host_svd3_emulated(const float* f_host, float* usv_host, int n, int svd_flavor);

/* HOST function: the rounding flavour (HPS_SVD_ROUNDING_*) whose factors are bit-identical to those of the LAPACK sgesdd_
 * this process is bound to (hps_host_bind_lapack) on 4 096 fixed test matrices, or -1 if neither is.  The shipped binding
 * calls it once and runs the device SVD in that flavour, so that svd_mode device and svd_mode host give the same bits. */
int hps_host_svd_flavor(void);

/* HOST function (no device work): SVD of n row-major 3x3 matrices through the LAPACK sgesdd_ exported by the
 * process's libtorch_cpu.so -- the routine behind the reference's torch.svd(F.cpu()) (:137), so factors and
 * column signs are bit-identical -- spread over num_threads threads.  f_host (n,9) -> usv_host (n,21) packed
 * [U (9) | S (3) | V (9)].  HPS_E_UNSUPPORTED if sgesdd_ cannot be resolved. */
int hps_host_svd3_packed(const float* f_host, float* usv_host, int n, int num_threads);
/* HOST: resolve sgesdd_ from the given shared library (the binding passes torch's libtorch_cpu.so). */
int hps_host_bind_lapack(const char* library_path);

/* Proper-SVD fix and mode (:139-152) for the joints of one level.  usv_level (B, n_level, 21) holds the SVD
 * factors of the level's F matrices packed as [U (9) | S (3) | V (9)] per matrix; they are scattered into
 * pose_u / pose_s / pose_v (B,23,..) and u_proper, s_proper, mode = U_p V_p^T are written. */
int hps_head_svd_finish(const float* usv_level, const int32_t* joint_ids, int n_level,
                        float* pose_u, float* pose_s, float* pose_v, float* u_proper,
                        float* s_proper, float* mode, int B, int num_body_joints,
                        hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ResNet-18 / ResNet-50 encoder  (models/resnet.py:202-217) -- NHWC activations
 * ---------------------------------------------------------------------------------------- */

/* Halo-padded generation of the convolution (csrc/conv_pad.hip), same arithmetic and summation order as
 * hps_conv2d_bn_act_v3.  x is (B, H + 2 ipad, W + 2 ipad, Cin) NHWC with a ZERO halo of ipad >= pad pixels, so every
 * filter tap is in bounds; y (and residual) are frames (B, Ho + 2 opad, Wo + 2 opad, Cout) of which only the interior
 * is written (the owner zeroes the halo once).  wn: n-major filter (Cout, KH*KW*Cin), Cin % 32 == 0; or, row_mode != 0
 * (the 18-channel 7x7 stem, models/resnet.py:150, :203): (Cout, KH * ceil32(KW*Cin)), one filter row = KW*Cin contiguous
 * NHWC floats taken as a single tap, zero filled tail.  variant: 0 automatic, 1 = 128x128, 2 = 128x64, 3 = 64x64, 4 = 256x64
 * workgroup tiles, 5 = 64x64 with a four-stage K loop (chunks fetched three ahead: the form for one or a few images, where a CU
 * holds one workgroup and nothing else covers the fetch latency).  ksplit > 1 ((KH*KW*Cin/32) divisible by ksplit): K in ksplit
 * slices, on the 128-row tiles unless variant is 3 or 5; splitk_ws (ksplit, B*Ho*Wo, Cout) floats; the slices are added in slice
 * order by a second kernel that also applies BN / residual / ReLU (deterministic, no atomics).  The tile shape never changes an
 * output's summation order.  Lane offsets are 32-bit: tensors < 4 GiB. */
int hps_conv2d_bn_act_pad(const float* x, const float* wn, const float* scale, const float* shift,
                          const float* residual, float* y, int B, int H, int W, int ipad, int Cin, int Cout,
                          int KH, int KW, int stride, int pad, int opad, int relu, int row_mode, int variant,
                          int ksplit, float* splitk_ws, hps_stream_t stream);

/* BasicBlock entry with a down-sample branch (models/resnet.py:62-78 with :71-72 `identity = self.downsample(x)`, built at
 * :184-188): the block's k x k / stride / pad = k/2 convolution + BatchNorm (+ ReLU) -> y AND its 1x1 / stride / 0 down-sample
 * convolution + BatchNorm -> y_down, both from the same input frame, in ONE launch (extra workgroups walk the main window's centre
 * tap with the down-sample's filter).  wn_down: (Cout, Cin) n-major; y_down: a frame of y's geometry.  Every output has the bits of
 * hps_conv2d_bn_act_pad called once per convolution (same chunks, same order; tile shapes do not change a summation order).
 * variant 1, 2, 3, 5 or 0 (automatic) as above; ksplit applies to the main convolution only.  Cin % 32 == 0. */
int hps_conv2d_bn_act_pad_down(const float* x, const float* wn, const float* scale, const float* shift, float* y,
                               const float* wn_down, const float* scale_down, const float* shift_down, float* y_down,
                               int B, int H, int W, int ipad, int Cin, int Cout, int KH, int KW, int stride, int pad,
                               int opad, int relu, int variant, int ksplit, float* splitk_ws, hps_stream_t stream);

/* Bottleneck entry block (models/resnet.py:102-122: `out = bn3(conv3(out)); identity = self.downsample(x); out += identity;
 * out = relu(out)`, the down-sample built at :184-188) in ONE launch (csrc/conv_expand_down.hip):
 *     y = relu( (acc3 * scale3 + shift3) + identity ),     identity = acc_d * scale_down + shift_down + 0
 * acc3: the 1x1 / 1 convolution of the frame t (B, Ho + 2 tpad, Wo + 2 tpad, Cmid) with w3 (Cout, Cmid) n-major; acc_d: the
 * 1x1 / stride convolution of the frame x (B, H + 2 xpad, W + 2 xpad, Cin) with w_down (Cout, Cin) n-major, Ho = (H - 1) / stride + 1
 * (Wo alike); y: the interior of the frame (B, Ho + 2 opad, Wo + 2 opad, Cout), the halo is the owner's.  The identity's tile is
 * formed first and held in registers through the second K loop: its frame is never written or read.  Every output has the bits of
 *     hps_conv2d_bn_act_pad(x, w_down, scale_down, shift_down, NULL, d, ..., stride, pad = 0, relu = 0)
 *     hps_conv2d_bn_act_pad(t, w3, scale3, shift3, residual = d, y, ..., relu = 1)
 * (both loops walk their chunks in that kernel's order; the epilogue expressions are the same).  Cmid % 32 == 0, Cin % 32 == 0,
 * Cout % 64 == 0, stride 1 or 2; variant 1, 2, 3, 5 or 0 (automatic, hps_conv2d_bn_act_pad's rule).  No split K: ksplit > 1 is
 * refused (a layer whose mode wants K slices takes the two launches).  Arguments are validated on the host before any launch: null
 * pointers, geometry, the 32-bit lane offsets (tensors < 4 GiB). */
int hps_bottleneck_expand_down(const float* t, const float* w3, const float* scale3, const float* shift3, const float* x,
                               const float* w_down, const float* scale_down, const float* shift_down, float* y, int B, int H, int W,
                               int stride, int tpad, int xpad, int opad, int Cmid, int Cin, int Cout, int variant, int ksplit,
                               hps_stream_t stream);

/* 3x3 / stride 1 / pad 1 convolution + BatchNorm (+ residual) (+ ReLU) by Winograd F(2x2, 3x3) on the fp32 MFMA pipe
 * (csrc/conv_wino.hip): 16 multiplications per 2x2 output tile and (cin, cout) pair instead of 36 -- the stride-1 3x3
 * layers of the BasicBlocks (models/resnet.py:62-78).  x / y / residual are halo-padded NHWC frames as for
 * hps_conv2d_bn_act_pad (ipad >= 1).  u: the transformed filters U = G g G^T, prepared once by the host in the layout
 *   u[chunk = cin / 8][cout tile = cout / 64][position p = 4 a + b][k-quad = (cin % 8) / 4][cout % 64][cin % 4]
 * with G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1].  Requirements: Cin % 8 == 0, Cout % 64 == 0 and either
 * H % 16 == 0, W % 16 == 0 (items of 8 x 8 tiles of one image) or H == W == 8 (layer4: items of four images; K is cut
 * into slices whose partial sums go through splitk_ws -- hps_conv3x3_winograd_workspace(B, H, W, Cin, Cout) bytes, 0 for
 * the first geometry, where splitk_ws may be NULL -- and are added in slice order by a second kernel).  Results equal the
 * direct convolution up to fp32 rounding of a different summation order; the order depends on the layer only, never on
 * the batch size. */
int hps_conv3x3_winograd(const float* x, const float* u, const float* scale, const float* shift,
                         const float* residual, float* y, int B, int H, int W, int ipad, int Cin, int Cout,
                         int opad, int relu, float* splitk_ws, hps_stream_t stream);
size_t hps_conv3x3_winograd_workspace(int B, int H, int W, int Cin, int Cout);

/* The stem -- conv1 7x7 / stride 2 / pad 3 on the 18-channel proxy representation + bn1 + relu (models/resnet.py:147-150,
 * :203-206) -- in Winograd form (csrc/stem_wino.hip): the stride-2 correlation is the sum of four stride-1 correlations on the
 * even / odd sub-lattices of the input (4x4, 4x3, 3x4 and 3x3 taps), each computed as F(2x2, r x s): 81 multiplications per 2x2
 * output tile and (cin, cout) pair instead of 196.  Same result as the direct sum up to fp32 rounding (both are within 1e-6 of the
 * output scale of the fp64 sum).  H and W multiples of 32, Cin = 18, Cout = 64.
 *   hps_stem_phase_split: x (B,18,H,W) NCHW -> frames[b][2 ry + rx][i][j][18] = x[b][:, 2 i + ry - 3, 2 j + rx - 3], four
 *     (H/2 + 4) x (W/2 + 4)-pixel frames per image whose out-of-image pixels the OWNER zeroes once (only in-image pixels are ever
 *     written); the channels of a pixel are stored in the order 0 2 1 3 | 4 6 5 7 | 8 10 9 11 | 12 14 13 15 | 16 17, and two pixels
 *     are followed by two floats of padding (a frame row is (W/2 + 4) / 2 pixel pairs of 38 floats: LDS bank spread).  The buffer
 *     holds hps_stem_phase_frames_bytes(B, H, W) bytes (the frames plus the slack the last window's DMA over-reads).
 *   hps_stem_winograd: frames -> y, the interior of the (B, H/2 + 2 opad, W/2 + 2 opad, 64) NHWC frame.  u: the transformed
 *     filters of the 81 positions, position-major in the row order (phase 2 ry + rx; row i; column j), 1152 floats each:
 *       u[position][co / 32][ k-block: (c % 16) / 8 ][ c % 2 ][co % 32][ (c % 8) / 2 ]   for c < 16   (2 x 2 x 32 x 4 floats)
 *       u[position][co / 32][512 + (c - 16) * 32 + co % 32]                              for c = 16, 17
 *     U = G_y g_{ry,rx} G_x^T with g_{ry,rx}[a][b] = w[co][c][2a + ry][2b + rx] and
 *     G (4 taps) = [1/2 0 0 0; -1/2 -1/2 -1/2 -1/2; -1/6 1/6 -1/6 1/6; 1/6 1/3 2/3 4/3; 0 0 0 1],
 *     G (3 taps) = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1]; 81 * 1152 floats plus 256 floats of readable slack. */
size_t hps_stem_phase_frames_bytes(int B, int H, int W);
int hps_stem_phase_split(const float* x, float* frames, int B, int C, int H, int W, hps_stream_t stream);
/* The proxy representation (predict/predict_poseMF_shapeGaussian_net.py:93-100; heat-maps: utils/label_conversions.py:105-124) written
 * straight into the phase frames: exactly what hps_proxy_rep (edge -> channel 0, visibility-masked Gaussians of the K = 17 joints ->
 * channels 1..17) followed by hps_stem_phase_split leaves in `frames`, bit for bit, without the (B,18,H,W) tensor in between.
 * edge: (B,H,W) plane or NULL (zeros); joints2d (B,17,2) (u = column, v = row); visib (B,17) or NULL.  For callers that build the
 * network input on the device anyway (the from-RGB pipeline); the NCHW entry stays the contract of the reference's call surface. */
int hps_proxy_rep_phase_frames(const float* edge, const float* joints2d, const float* visib, float* frames, int B, int K, int H,
                               int W, float std, hps_stream_t stream);
int hps_stem_winograd(const float* frames, const float* u, const float* scale, const float* shift, float* y, int B, int H,
                      int W, int opad, int relu, hps_stream_t stream);
/* The stem AND the 3x3 / 2 / pad 1 max pool behind it (models/resnet.py:150, :206: self.maxpool) in one call: frames -> the interior of
 * the (B, H/4 + 2 opad, W/4 + 2 opad, 64) NHWC frame of the POOLED map; the stem's full-resolution output (which nothing else reads) is
 * never written.  Every pooled pixel is the maximum of the same nine stem outputs hps_maxpool3x3s2_pad takes it over (formed tile by tile
 * in the stem kernel's epilogue; the pixels of an 8 x 8 block of pooled pixels that also see a neighbouring block are completed by a
 * small second kernel from `side`): identical values.  side: scratch of hps_stem_pool_side_bytes(B, H, W) bytes, written and read by
 * this call only. */
size_t hps_stem_pool_side_bytes(int B, int H, int W);
int hps_stem_winograd_pooled(const float* frames, const float* u, const float* scale, const float* shift, float* pooled, float* side,
                             int B, int H, int W, int opad, int relu, hps_stream_t stream);
/* The same from the network input itself: x (B,18,H,W) NCHW fp32, exactly what models/resnet.py:202-206 receives.  The kernel gathers its
 * phase windows from x (global loads, out-of-image pixels stay zero) into the LDS layout the frames would have given it:
 * hps_stem_phase_split and the four frames per image are not needed.  Identical values to hps_stem_phase_split + hps_stem_winograd_pooled. */
int hps_stem_winograd_pooled_nchw(const float* x, const float* u, const float* scale, const float* shift, float* pooled, float* side,
                                  int B, int H, int W, int opad, int relu, hps_stream_t stream);

/* One launch of the encoder's operation list (hps_encoder_run).  kind: HPS_ENC_RELAYOUT = hps_nchw_to_padded_nhwc
 * (x, y, B, Cin = C, H, W, opad = P), HPS_ENC_CONV = hps_conv2d_bn_act_pad (all fields), HPS_ENC_MAXPOOL =
 * hps_maxpool3x3s2_pad (x, y, B, H, W, Cin = C, opad), HPS_ENC_AVGPOOL = hps_global_avgpool_pad (x, y, B, H, W,
 * Cin = C, ipad = P), HPS_ENC_CONV_WINOGRAD = hps_conv3x3_winograd (x, w = u, scale, shift, residual, y, B, H, W, ipad, Cin,
 * Cout, opad, relu, splitk_ws), HPS_ENC_STEM_SPLIT = hps_stem_phase_split (x, y = frames, B, Cin = C, H, W),
 * HPS_ENC_STEM_WINOGRAD = hps_stem_winograd (x = frames, w = u, scale, shift, y, B, H, W, opad, relu), HPS_ENC_STEM_WINOGRAD_POOLED =
 * hps_stem_winograd_pooled (x = frames, w = u, scale, shift, y = pooled frame, splitk_ws = side, B, H, W, opad, relu),
 * HPS_ENC_STEM_WINOGRAD_POOLED_NCHW = hps_stem_winograd_pooled_nchw (the same fields with x = the NCHW input). */
enum { HPS_ENC_RELAYOUT = 0, HPS_ENC_CONV = 1, HPS_ENC_MAXPOOL = 2, HPS_ENC_AVGPOOL = 3, HPS_ENC_CONV_WINOGRAD = 4,
       HPS_ENC_STEM_SPLIT = 5, HPS_ENC_STEM_WINOGRAD = 6,
       HPS_ENC_RELAYOUT_GENERIC = 7 /* hps_nchw_to_padded_nhwc_generic (x, y, B, Cin = C, Cout = CP, H, W, KW = WF, opad = P) */,
       HPS_ENC_STEM_WINOGRAD_POOLED = 8, HPS_ENC_STEM_WINOGRAD_POOLED_NCHW = 9,
       HPS_ENC_CONV_DOWN = 10 /* hps_conv2d_bn_act_pad_down: the HPS_ENC_CONV fields + w_down / scale_down / shift_down / y_down */,
       HPS_ENC_EXPAND_DOWN = 11 /* hps_bottleneck_expand_down: x = t, w = w3, scale, shift, x_down = x, w_down, scale_down, shift_down, y,
                                   B, H, W (of x_down), stride, ipad = tpad, ipad_down = xpad, opad, Cin = Cmid, Cin_down = Cin, Cout,
                                   variant, ksplit */ };
typedef struct hps_enc_op {
    int kind;
    const float* x;
    const float* w;
    const float* scale;
    const float* shift;
    const float* residual;
    float* y;
    float* splitk_ws;
    int B, H, W, ipad, Cin, Cout, KH, KW, stride, pad, opad, relu, row_mode, variant, ksplit;
    const float* w_down;       /* HPS_ENC_CONV_DOWN only (NULL otherwise) */
    const float* scale_down;
    const float* shift_down;
    float* y_down;
    const float* x_down;       /* HPS_ENC_EXPAND_DOWN only: the block's input frame, its halo and its channels */
    int ipad_down, Cin_down;
} hps_enc_op;

/* sizeof(hps_enc_op) as compiled into the library: lets a hand-written mirror of the struct check itself. */
int hps_sizeof_enc_op(void);

/* models/resnet.py:202-217 in one call: issues ops[0..n_ops) in order on `stream` (same launches as the individual
 * entry points; exists because issuing ~27 launches through a scripting-language FFI costs more host time than the
 * GPU needs to run them). */
int hps_encoder_run(const hps_enc_op* ops, int n_ops, hps_stream_t stream);

/* models/poseMF_shapeGaussian_net.py:121-160 in one call, one kinematic level after the other.
 *   svd_mode HPS_SVD_DEVICE / HPS_SVD_DEVICE_FMA (rounding flavour reference / fused): hps_head_joint_level_svd per level --
 *            8 stream-ordered launches for the SMPL tree, no synchronisation, capturable in a hipGraph; the staging buffers
 *            may be NULL.
 *   svd_mode HPS_SVD_HOST (parity mode: the very LAPACK routine of the reference): hps_head_joint_level -> D2H of the level's F
 *            matrices -> stream synchronise -> hps_host_svd3_packed (:137) -> H2D -> hps_head_svd_finish.
 * level_joints: DEVICE int32 array, the levels' joint ids concatenated; level_sizes_host: HOST
 * array of n_levels sizes; f_level_dev (B*max_level*9) / usv_level_dev (B*max_level*21): device scratch;
 * f_host_pinned / usv_host_pinned: page-locked host staging of the same sizes.  Blocks the calling thread (it waits
 * for each level's matrices); other streams keep running. */
int hps_head_pose_levels(const float* embed, int embed_dim, int hidden, const int32_t* level_joints,
                         const int32_t* level_sizes_host, int n_levels, const int32_t* anc_ptr,
                         const int32_t* anc_idx, const float* const* w1t_ptrs, const float* const* b1_ptrs,
                         const float* const* w2_ptrs, const float* const* b2_ptrs, float* u_proper,
                         float* s_proper, float* mode, float delta_i_weight, float* pose_f, float* pose_u,
                         float* pose_s, float* pose_v, float* f_level_dev, float* usv_level_dev,
                         float* f_host_pinned, float* usv_host_pinned, int B, int num_body_joints,
                         int svd_threads, int svd_mode, hps_stream_t stream);

/* ---- backward of the head (what the reference's training step, train/train_poseMF_shapeGaussian_net.py:262-349, gets from
 * torch autograd).  No floating-point atomics, no synchronisation, bitwise repeatable; the gradient of one image's features
 * depends on that image alone (same bits at any B); parameter gradients are summed over the images in ascending order with
 * float64 accumulators. ---- */

/* The forward of the head again in float64, the first step of its backward: models/poseMF_shapeGaussian_net.py:95-160 with float64
 * sums and float64 values between the stages, a float64 3x3 SVD (one-sided Jacobi) whose column signs are taken from the forward's
 * pose_U (pose_u_pin, fp32 (B,NJ,3,3)).  Why float64: the gradient's error is the head's second derivative times the error of the
 * values it is evaluated at, and torch.svd's backward multiplies by 1 / (s_j^2 - s_i^2); the fp32 forward's rounding in F (about
 * 2^-23 |F|) is amplified by that factor at every joint and handed down the kinematic chain, while the float64 values leave the
 * backward's own fp32 roundings as the only error.  Weights as in hps_head_trunk / hps_head_pose_levels.
 * Outputs: x_f (B, hidden_trunk), sgc_f (B, num_sgc), embed_f (B, embed_dim) in fp32 for hps_head_trunk_backward; float64 x_d, sgc_d,
 * embed_d and u_proper / s_proper / mode / pose_u / pose_s / pose_v (B,NJ,..) for hps_head_pose_levels_backward.  3 + n_levels
 * launches, no synchronisation. */
int hps_head_forward_refine(const float* feats, int ldf, const float* fc1_wt, const float* fc1_b, const float* sgc_wt,
                            const float* sgc_b, const float* sgc_add, const float* embed_wt, const float* embed_b,
                            const int32_t* level_joints, const int32_t* level_sizes_host, int n_levels,
                            const int32_t* anc_ptr, const int32_t* anc_idx, const float* const* w1t_ptrs,
                            const float* const* b1_ptrs, const float* const* w2_ptrs, const float* const* b2_ptrs,
                            float delta_i_weight, const float* pose_u_pin, float* x_f, float* sgc_f, float* embed_f,
                            double* x_d, double* sgc_d, double* embed_d, double* u_proper, double* s_proper, double* mode,
                            double* pose_u, double* pose_s, double* pose_v, int B, int num_feats, int hidden_trunk,
                            int num_sgc, int embed_dim, int hidden, int num_body_joints, hps_stream_t stream);

/* models/poseMF_shapeGaussian_net.py:121-160 differentiated, kinematic levels from the leaves to the root in one call (one launch
 * per level as in hps_head_pose_levels, then one launch for g_embed and one for the parameter gradients).  Per joint: the
 * cotangents of pose_F (:154), pose_S (:156) and pose_rotmats_mode (:160) (g_pose_f (B,NJ,3,3), g_pose_s (B,NJ,3), g_mode
 * (B,NJ,3,3); each may be NULL = zero), plus what the joint's descendants left on its U_proper / S_proper / mode (:126-128),
 * go back through mode = U_p V_p^T (:152), the proper fix (:144-150, det U and det V are constants, :139-140), torch.svd's
 * backward (:137, distinct singular values) and the joint's MLP (:130-135; the hidden activations are computed again).
 * From a preceding hps_head_forward_refine (float64): embed, u_proper, s_proper, mode, pose_u, pose_s, pose_v; level_joints / level_sizes_host / anc_ptr /
 * anc_idx / w1t_ptrs / b1_ptrs / w2_ptrs as in hps_head_pose_levels.
 * desc_ptr (NJ+1), desc_joint, desc_pos (device int32): for joint a the joints d that have a among their ancestors, ascending,
 * with the position of a in d's ancestor list.  in_off (NJ+1, device int32): prefix sums of in_dim_j = embed_dim + 21 * (number
 * of ancestors of j); total_in = in_off[NJ].
 * Outputs: g_embed (B, embed_dim), the cotangent of the embedding (:110) for hps_head_trunk_backward; g_fc_pose: flat buffer of
 * 128 * total_in + NJ * (128 + 9 * 128 + 9) floats, joint j's [g_W1 (128, in_dim_j) | g_b1 (128) | g_W2 (9, 128) | g_b2 (9)]
 * in nn.Linear's layout at 128 * in_off[j] + j * (128 + 9 * 128 + 9); NULL: the parameter gradients are not wanted, their launch
 * is skipped.
 * workspace: hps_query_workspace(HPS_WS_HEAD_LEVELS_BWD, B, total_in, num_body_joints) bytes. */
int hps_head_pose_levels_backward(const double* embed, int embed_dim, int hidden, const int32_t* level_joints,
                                  const int32_t* level_sizes_host, int n_levels, const int32_t* anc_ptr,
                                  const int32_t* anc_idx, const int32_t* desc_ptr, const int32_t* desc_joint,
                                  const int32_t* desc_pos, const int32_t* in_off, const float* const* w1t_ptrs,
                                  const float* const* b1_ptrs, const float* const* w2_ptrs, const double* u_proper,
                                  const double* s_proper, const double* mode, const double* pose_u, const double* pose_s,
                                  const double* pose_v, const float* g_pose_f, const float* g_pose_s, const float* g_mode,
                                  float* g_embed, float* g_fc_pose, float* workspace, int B, int num_body_joints,
                                  int total_in, hps_stream_t stream);

/* hps_head_pose_levels_backward with cotangents on the raw SVD factors too: g_pose_u / g_pose_v (fp32 (B,NJ,3,3), each may be NULL =
 * zero) are the cotangents of pose_U / pose_V as models/poseMF_shapeGaussian_net.py:137 returns them (the reference's sampler reads
 * them, utils/sampling_utils.py:105-111, and torch.svd's backward takes them).  They join gU / gV before U^T gU / V^T gV, without a
 * proper-fix factor.  Everything else as hps_head_pose_levels_backward, which is this call with both NULL. */
int hps_head_pose_levels_backward_factors(const double* embed, int embed_dim, int hidden, const int32_t* level_joints,
                                          const int32_t* level_sizes_host, int n_levels, const int32_t* anc_ptr,
                                          const int32_t* anc_idx, const int32_t* desc_ptr, const int32_t* desc_joint,
                                          const int32_t* desc_pos, const int32_t* in_off, const float* const* w1t_ptrs,
                                          const float* const* b1_ptrs, const float* const* w2_ptrs, const double* u_proper,
                                          const double* s_proper, const double* mode, const double* pose_u, const double* pose_s,
                                          const double* pose_v, const float* g_pose_f, const float* g_pose_s, const float* g_mode,
                                          const float* g_pose_u, const float* g_pose_v, float* g_embed, float* g_fc_pose,
                                          float* workspace, int B, int num_body_joints, int total_in, hps_stream_t stream);

/* models/poseMF_shapeGaussian_net.py:95-110 differentiated.  feats and shape_scale from the forward; x, sgc, embed: the fp32 outputs
 * x_f, sgc_f, embed_f of hps_head_forward_refine.  fc1_w (hidden, num_feats), sgc_w (2 num_shape + num_glob + num_cam, hidden) = fc_shape | fc_glob | fc_cam stacked,
 * embed_w (embed_dim, num_feats + 2 num_shape + num_glob + num_cam): the weights in nn.Linear's own layout.
 * Cotangents (each may be NULL = zero): g_embed (B, embed_dim), g_loc / g_scale (B, num_shape) of the Gaussian's loc and scale
 * (scale = exp(log std), :101), g_glob (B, num_glob), g_cam (B, num_cam); the last four reach fc1 directly (:98-107) and through
 * the concatenation into fc_embed (:108).
 * Outputs: g_feats (B, num_feats) and the parameter gradients in the layouts of fc1_w / sgc_w / embed_w and their biases (the
 * rows of g_sgc_w / g_sgc_b are fc_shape's, then fc_glob's, then fc_cam's).
 * g_feats may be NULL (frozen features); the six parameter gradients may be NULL all together (frozen parameters): what is not
 * wanted is not launched.
 * workspace: hps_query_workspace(HPS_WS_HEAD_TRUNK_BWD, B, num_feats + hidden + embed_dim, 2 num_shape + num_glob + num_cam). */
int hps_head_trunk_backward(const float* feats, int ldf, const float* x, const float* sgc, const float* embed,
                            const float* shape_scale, const float* fc1_w, const float* sgc_w, const float* embed_w,
                            const float* g_embed, const float* g_loc, const float* g_scale, const float* g_glob,
                            const float* g_cam, float* g_feats, float* g_fc1_w, float* g_fc1_b, float* g_sgc_w,
                            float* g_sgc_b, float* g_embed_w, float* g_embed_b, float* workspace, int B, int num_feats,
                            int hidden, int num_shape, int num_glob, int num_cam, int embed_dim, hps_stream_t stream);

/* (B,C,H,W) -> interior of the (B, H + 2P, W + 2P, C) NHWC frame; C in {4, 18, 64}
 * (predict/predict_poseMF_shapeGaussian_net.py:103 hands the net an NCHW proxy representation). */
int hps_nchw_to_padded_nhwc(const float* x, float* y, int B, int C, int H, int W, int P, hps_stream_t stream);

/* The same for ANY channel count and width (models/resnet.py:127-176 accepts any in_channels / image size): channel c < C of
 * pixel (h, w) -> interior of a (B, H + 2P, WF + 2P, CP) frame, CP >= C, WF >= W; channels C..CP-1, columns W..WF-1 and the
 * halo are left as the owner zeroed them.  The encoder uses CP = C rounded up to 4 and WF = W rounded up to even, which gives
 * the row-mode stem of hps_conv2d_bn_act_pad its 16-byte aligned windows for every shape (zero channels / a zero column are
 * exactly the convolution's zero padding). */
int hps_nchw_to_padded_nhwc_generic(const float* x, float* y, int B, int C, int CP, int H, int W, int WF, int P,
                                    hps_stream_t stream);

/* nn.MaxPool2d(3, 2, 1) (models/resnet.py:152, :207): x (B,H,W,C) plain NHWC -> interior of the
 * (B, Ho + 2 opad, Wo + 2 opad, C) frame. */
int hps_maxpool3x3s2_pad(const float* x, float* y, int B, int H, int W, int C, int opad, hps_stream_t stream);

/* AdaptiveAvgPool2d((1,1)) + flatten (models/resnet.py:214-215) over the interior of a (B, H + 2P, W + 2P, C) frame. */
int hps_global_avgpool_pad(const float* x, float* y, int B, int H, int W, int C, int P, hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Backward of the encoder  (torch autograd through models/resnet.py:62-78, 202-217; csrc/conv_backward.hip)
 * A layer is y = act(conv(x, w) scale + shift [+ residual]) with eval-mode BatchNorm folded into scale / shift.  With g the cotangent
 * behind the ReLU gate: G = corr(x, g) (hps_conv_wgrad), dW = scale_c G[c], dscale_c = <w[c], G[c]>, dshift_c = sum of g_c
 * (hps_relu_gate_pad), dx = conv^T(g, w scale) (hps_conv_dgrad).  No atomics: every result is bitwise repeatable.
 * ---------------------------------------------------------------------------------------- */

/* Weight-gradient GEMM on the fp32 matrix cores: G (Cout, KH, KW, Cin) =
 *   sum over b, oy, ox of g[b, oy, ox, co] * x[b, oy stride + ky - pad, ox stride + kx - pad, ci]
 * x: (B, H + 2 ipad, W + 2 ipad, Cx) frame with a zero halo, ipad >= pad, Cx >= Cin channels per pixel (the first Cin are used);
 * g: (B, Ho + 2 gpad, Wo + 2 gpad, Cout) frame (its halo is not read).  The contraction over the B Ho Wo pixels is cut into slices
 * of hps_conv_wgrad_slice_pixels(Ho, Wo) pixels -- a rule on the map alone: the map's pixel count clamped to [128, 512] --; the
 * slices' fp32 partials go to ``workspace`` (hps_conv_wgrad_workspace bytes) and are added in slice order in float64, rounded once.
 * Any Cin, Cout, filter size and stride (every layer of the net: 3x3 / 1, 3x3 / 2, 1x1 / 2, the 7x7 / 2 stem with Cin = 18). */
int hps_conv_wgrad(const float* x, const float* g, float* G, float* workspace, int B, int H, int W, int ipad, int Cx, int Cin,
                   int Cout, int KH, int KW, int stride, int pad, int gpad, hps_stream_t stream);
int hps_conv_wgrad_slice_pixels(int Ho, int Wo);
size_t hps_conv_wgrad_workspace(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);

/* Data gradient, gather form: interior of the (B, H + 2 dpad, W + 2 dpad, Cdx) frame dx (channels 0 .. Cin-1) =
 *   sum over ky, kx, co of g[b, (iy + pad - ky) / stride, (ix + pad - kx) / stride, co] * wt[ky][kx][co][ci]   (+ other, same frame)
 * over the taps whose output pixel exists (in range and in phase with the stride); wt (KH, KW, Cout, Cin) is the layer's filter with
 * the BatchNorm scale of channel co folded in; ``other`` (may be NULL) is the gradient of the block's other branch, added last.
 * g as in hps_conv_wgrad; Cout % 8 == 0.  fp32 chains of 64 output channels, added in (tap, channel block) order. */
int hps_conv_dgrad(const float* g, const float* wt, const float* other, float* dx, int B, int H, int W, int Cin, int Cout, int KH,
                   int KW, int stride, int pad, int gpad, int dpad, int Cdx, hps_stream_t stream);

/* The two gradients of a 1x1 / pad 0 convolution as LDS-tiled GEMMs over NHWC rows (csrc/conv1x1_backward.hip): the pointwise
 * layers of Bottleneck.forward (models/resnet.py:105 conv1, :113 conv3, built at :92 and :96) and the down-sample of _make_layer
 * (:184-188, applied at :116-117), differentiated under torch autograd.  Four waves per workgroup on a 128 x 128 (128 x 64) tile, both
 * operands staged through LDS 32 K at a time.  Cout % 8 == 0, stride 1 or 2; frames of 2^31 pixels or more are refused.
 *
 * hps_conv1x1_dgrad: the contract of hps_conv_dgrad at KH = KW = 1, pad = 0 -- wt is (Cout, Cin); every interior pixel of dx is
 * written, off the stride lattice with ``other`` or 0; halos and channels Cin .. Cdx-1 are never touched -- and ITS BITS: the same K
 * order (MFMA j of a step of 8 channels contracts co0 + j and co0 + 4 + j), the chain cut every 64 channels, pieces added in order in
 * fp32.  A pixel's sum depends on the layer alone, never on B or on the tile it falls in. */
int hps_conv1x1_dgrad(const float* g, const float* wt, const float* other, float* dx, int B, int H, int W, int Cin, int Cout, int stride,
                      int gpad, int dpad, int Cdx, hps_stream_t stream);

/* hps_conv1x1_wgrad: G (Cout, Cin) = sum over b, oy, ox of g[b, oy, ox, co] * x[b, oy stride, ox stride, ci]; x, g, Cx, ipad, gpad as
 * in hps_conv_wgrad (ipad >= 0).  The B Ho Wo pixels are cut into slices of hps_conv1x1_wgrad_slice_pixels(Cin, Cout) pixels -- a rule
 * on the layer alone: twice the harmonic mean of Cin and Cout, rounded up to a multiple of 64, at least 1024.  Inside a slice chain
 * pieces of 64 pixels are added in order in fp32; the slices' partials go to ``workspace`` (hps_conv1x1_wgrad_workspace bytes) and are
 * added in slice order in float64, rounded once.  No atomics.  Other bits than hps_conv_wgrad (another slice length).
 * Workspace bound: with P = B Ho Wo >= one slice, ceil(P / S) Cin Cout <= P (Cin + Cout) / 2 + Cin Cout floats, the two operands hold
 * P (Cin + Cout) or more.  Every 1x1 layer of ResNet-50 at B = 72 on 256 x 256 inputs stays below 0.42 of its operand frames
 * (layer4's conv1 / conv3: 5 slices of 4 MB against 47 MB; hps_conv_wgrad_workspace: 36 slices). */
int hps_conv1x1_wgrad(const float* x, const float* g, float* G, float* workspace, int B, int H, int W, int ipad, int Cx, int Cin,
                      int Cout, int stride, int gpad, hps_stream_t stream);
int hps_conv1x1_wgrad_slice_pixels(int Cin, int Cout);
size_t hps_conv1x1_wgrad_workspace(int B, int H, int W, int Cin, int Cout, int stride);

/* ReLU gate in place: interior of g (B, H + 2 gpad, W + 2 gpad, C) <- g where y > 0 (strict, as torch), else 0; y (B, H + 2 ypad,
 * W + 2 ypad, C) is the layer's output.  sums (C,), optional together with workspace (hps_relu_gate_workspace bytes, float64): the
 * per-channel sums of the gated cotangent (d shift) -- float64 per 64 pixels, then float64 over the chunks in order, rounded once. */
int hps_relu_gate_pad(float* g, const float* y, double* workspace, float* sums, int B, int H, int W, int C, int gpad, int ypad,
                      hps_stream_t stream);
size_t hps_relu_gate_workspace(int B, int H, int W, int C);

/* nn.MaxPool2d(3, 2, 1) differentiated: x (B,H,W,C) plain NHWC, the pool's input; gpool the (B, Ho + 2 gpad, Wo + 2 gpad, C) frame of
 * the output's cotangent; dx (B,H,W,C): each window's cotangent goes to its first maximum in row-major order (torch's rule). */
int hps_maxpool3x3s2_backward(const float* x, const float* gpool, float* dx, int B, int H, int W, int C, int gpad, hps_stream_t stream);

/* AdaptiveAvgPool2d((1,1)) differentiated: interior of the (B, H + 2P, W + 2P, C) frame <- gfeat (B,C) / (H W). */
int hps_global_avgpool_backward(const float* gfeat, float* gframe, int B, int H, int W, int C, int P, hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training-mode BatchNorm of the encoder  (csrc/bn_train.hip)
 * models/resnet.py:48-49, 53-54, 142-143, 184-188: every nn.BatchNorm2d, run under model.train()
 * (train/train_poseMF_shapeGaussian_net.py:114), i.e. torch's batch_norm(training=True): y = gamma (z - mean) / sqrt(var + eps) + beta
 * with the batch's per-channel mean and biased variance over the n = B H W pixels, and running <- (1 - momentum) running +
 * momentum batch with the unbiased variance var n / (n - 1).  A training layer's convolution runs with identity scale / shift, no
 * residual and no ReLU into a raw frame z; the kernels below work on such (B, H + 2 pad, W + 2 pad, C) NHWC frames (interior only;
 * halos are neither read nor written).  C = 4, 8, 16, ..., 1024 (a multiple of 4 with 256 % (C / 4) == 0) or a multiple of 1024 up
 * to 65536 (models/resnet.py:97, :186: the Bottleneck encoder's 2048; windows of 1024 channels), B H W < 2^31.
 * No atomics, fixed summation orders: every result is bitwise repeatable.
 * ---------------------------------------------------------------------------------------- */

/* torch batch_norm's batch statistics: mean (C,) and biased var (C,) of the interior of z, float64.  The B H rows are cut into
 * min(B H, 2048) contiguous chunks (a rule on B H alone); float64 sums of (z - K) and (z - K)^2 per chunk, K the channel's first
 * interior pixel (no cancellation when |mean| >> std), chunks added in a fixed order.  workspace: hps_bn_batch_stats_workspace bytes. */
int hps_bn_batch_stats(const float* z, double* workspace, double* mean, double* var, int B, int H, int W, int C, int pad,
                       hps_stream_t stream);
size_t hps_bn_batch_stats_workspace(int B, int H, int W, int C);

/* One launch per layer, torch's BatchNorm bookkeeping (nn.BatchNorm2d.forward in training mode): scale = gamma invstd and
 * shift = beta - mean scale, computed in float64 and rounded once to fp32; invstd = 1 / sqrt(var + eps) (C,) float64 is WRITTEN
 * when var is given and READ when var is NULL (the backward's recompute applies saved statistics).  running_mean / running_var
 * (fp32, both or neither; need var and n >= 2) <- (1 - momentum) running + momentum (mean | var n / (n - 1)), float64 rounded once;
 * num_batches_tracked (int64 scalar, may be NULL) += 1.  NULL buffers: no update (recompute, ResNet.training_activations). */
int hps_bn_train_fold(const double* mean, const double* var, double* invstd, const float* gamma, const float* beta, double eps,
                      double momentum, long long n, float* scale, float* shift, float* running_mean, float* running_var,
                      long long* num_batches_tracked, int C, hps_stream_t stream);

/* The convolution epilogue of models/resnet.py:62-78 as a pass of its own: interior of y (ypad) = act(z scale + shift [+ residual]),
 * z a raw frame (zpad), residual (may be NULL) in y's frame; the operations in the order of hps_conv2d_bn_act_pad's epilogue.
 * In place (y == z, ypad == zpad) is allowed. */
int hps_bn_apply_act_pad(const float* z, const float* scale, const float* shift, const float* residual, float* y, int B, int H, int W,
                         int C, int zpad, int ypad, int relu, hps_stream_t stream);

/* torch's batch_norm backward, the reductions: sums[0..C) = d beta = sum g, sums[C..2C) = d gamma = sum g zhat, zhat = (z - mean)
 * invstd, float64, chunks as in hps_bn_batch_stats.  y (may be NULL): the layer's output frame (models/resnet.py:66, :77 ReLU); then
 * g <- g where y > 0 else 0 is written back in the same sweep (hps_relu_gate_pad and the sums in one pass).  y NULL: g is only read. */
int hps_bn_train_backward_sums(float* g, const float* z, const float* y, const double* mean, const double* invstd, double* workspace,
                               double* sums, int B, int H, int W, int C, int gpad, int zpad, int ypad, hps_stream_t stream);
size_t hps_bn_train_backward_sums_workspace(int B, int H, int W, int C);

/* torch's batch_norm backward, the map: interior of dz (dpad) = gamma invstd (g - d beta / n - zhat d gamma / n), float64 per element,
 * rounded once; out of place (the gated g of a block's output, models/resnet.py:75-77, is also the cotangent of the identity branch).
 * hps_conv_wgrad(x, dz) is then dW itself and hps_conv_dgrad takes the unscaled filter. */
int hps_bn_train_backward_dz(const float* g, const float* z, const double* mean, const double* invstd, const float* gamma,
                             const double* sums, float* dz, int B, int H, int W, int C, int gpad, int zpad, int dpad, hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Proxy-representation front end  
 * ---------------------------------------------------------------------------------------- */

/* models/canny_edge_detector.py:104-166: per-channel separable Gaussian blur (zero padded), Sobel gradients averaged
 * over channels, magnitude, orientation binned to 45 degrees, threshold, and (nms != 0) non-max suppression.
 * img (B,C,H,W); gauss_taps_host: HOST array of gauss_size (= 5) normalised taps; outputs blurred (B,C,H,W) and
 * grad_mag, grad_ori, thr_mag, thin, thr_thin (B,1,H,W) -- the entries of the reference's output dict. */
int hps_canny_edges(const float* img, const float* gauss_taps_host, int gauss_size, float* blurred,
                    float* grad_mag, float* grad_ori, float* thr_mag, float* thin, float* thr_thin,
                    int B, int C, int H, int W, float threshold, int nms, hps_stream_t stream);

/* The edge map ALONE -- what predict/predict_poseMF_shapeGaussian_net.py:92-93 takes out of the detector's dict
 * ('thresholded_thin_edges' if nms != 0, else 'thresholded_grad_magnitude'): same kernel and arithmetic as hps_canny_edges,
 * none of the other five outputs written.  Image b's map goes to edge_out + b * edge_batch_stride (floats), so that it can be
 * channel 0 of a (B, K+1, H, W) proxy representation directly (edge_batch_stride = (K+1) H W; hps_proxy_rep with edge = NULL
 * then fills channels 1..K only): 4 planes of traffic per image instead of 11 + 2. */
int hps_canny_edge_map(const float* img, const float* gauss_taps_host, int gauss_size, float* edge_out,
                       int64_t edge_batch_stride, int B, int C, int H, int W, float threshold, int nms, hps_stream_t stream);

/* predict/predict_poseMF_shapeGaussian_net.py:93-100 with utils/label_conversions.py:105-124: out (B,K+1,H,W),
 * channel 0 = edge (B,1,H,W) -- or left as it is when edge is NULL (hps_canny_edge_map wrote it in place) --,
 * channel 1+k = visib[b,k] * exp(-((row - v)/std)^2/2 - ((col - u)/std)^2/2) for
 * joints2d (B,K,2) = (u, v); visib (B,K) float 0/1 or NULL; K <= 32. */
int hps_proxy_rep(const float* edge, const float* joints2d, const float* visib, float* out, int B,
                  int K, int H, int W, float std, hps_stream_t stream);

/* utils/label_conversions.py:127-155: heatmaps (BK, H, W) -> joints2d (BK,2) = (x, y) of the maximum (first index on
 * ties), visib (BK,) = 1.0 if max > eps else 0.0 (then joints2d = -1). */
int hps_heatmaps_to_joints2d(const float* heatmaps, float* joints2d, float* visib, int BK, int H, int W,
                             float eps, hps_stream_t stream);

/* utils/sampling_utils.py:210-229: err[s] = max over visible input joints k of the pixel distance
 * between in_j2d[k] and the weak-perspective projection of joints[s, coco_map[k]] flipped 180 degrees about x.
 * joints (N, n_joints_all, 3); in_j2d (K,2); in_vis (K,); cam (3,) = (scale, tx, ty). */
int hps_sample_joints2d_error(const float* joints, const int32_t* coco_map, int n_joints_all,
                              const float* in_j2d, const float* in_vis, const float* cam, float img_wh,
                              float* err, int N, int K, hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Synthetic-data training front end  (train/train_poseMF_shapeGaussian_net.py:199-244; csrc/train_frontend.hip)
 *
 * Everything between the renderer's IUV / RGB images and the Canny and heat-map kernels above.  All random DECISIONS of a step are
 * made on the host, in the reference's order of draws (train_augmentation.draw_augment_plan), and reach the device as one record of
 * HPS_TRAIN_PLAN_WORDS 32-bit words per image, `plan` (B, HPS_TRAIN_PLAN_WORDS) int32 (f = the word holds a float):
 *    0      classes (bit c = class c) left out of the bounding box         utils/augmentation/proxy_rep_augmentation.py:238-275
 *    1      classes removed from the segmentation                          :27-59
 *    2      f delta scale;  3, 4  f delta centre (vertical, horizontal)    utils/image_utils.py:315-326
 *    5-8    occlusion box: rows [lo, hi), columns [lo, hi)                 proxy_rep_augmentation.py:94-118
 *    9-14   segmentation half occlusions: bottom rows [lo, hi), top rows [lo, hi), vertical columns [lo, hi)       :121-183
 *   15-20   the same three for the RGB image                               utils/augmentation/rgb_augmentation.py:6-68
 *   21-24   f joint tests that go with 9-14: invisible if v > [21], v < [22], u < [23], u > [24] (+-inf: test off)
 *   25-28   f the same for 15-20
 *   29      joints made invisible (bit k = joint k)                        proxy_rep_augmentation.py:50-57, :62-70
 *   30-32   f channel factors                                              rgb_augmentation.py:71-77
 *   33-49   source joint of joint k after the swaps                        proxy_rep_augmentation.py:73-91
 *   50-83   f deviation (u, v) added to joint k                            :7-24
 * Every range is a Python slice of the reference normalised by slice.indices (int16 truncation and negative starts included); an
 * empty range is (0, 0).
 * ---------------------------------------------------------------------------------------- */
#define HPS_TRAIN_PLAN_WORDS 84
#define HPS_TRAIN_NUM_JOINTS 17
#define HPS_TRAIN_NUM_PART_COUNTS 8 /* pixels of the 14-part labels 3, 5, 7, 9, 11, 12, 13, 14, in this order */

/* utils/image_utils.py:277-345 with a bbox_determiner: per image the bounding box of the pixels of `part` (image b's H x W plane at
 * part + b * part_batch_stride: channel 0 of an IUV batch with stride 3 H W, fp32 holding integers) whose class is non-zero and not
 * in plan word 0 -- torch.nonzero(bbox_determiner[i] != 0) with min and max, :303-305 -- then :307-345 in fp32, operation by
 * operation: centre, height and width, aspect fix, orig_scale_factor + delta scale, centre + delta centre.  Writes affine (B,2,3),
 * the forward map of :330-334, and theta (B,4) = (theta00, theta02, theta11, theta12) of the normalised inverse of :341-345 (the
 * other two entries are zero).  out_wh: side of the square output.  plan may be NULL (no class left out, zero deltas).
 * Integer min / max over 32 row chunks, then a finish launch: ws is hps_query_workspace(HPS_WS_SEG_BBOX, B) bytes.  An image without
 * any such pixel is where the reference raises: its box becomes the whole frame and status[b] (int32, optional) is 1, else 0.
 * part_counts (B, HPS_TRAIN_NUM_PART_COUNTS) int32, optional: zeroed, ready for hps_train_crop_augment. */
int hps_seg_bbox_affine(const float* part, int64_t part_batch_stride, const int32_t* plan, int B, int H, int W, int out_wh,
                        float orig_scale_factor, int32_t* ws, float* affine, float* theta, int32_t* status, int32_t* part_counts,
                        hps_stream_t stream);

/* Stages of hps_train_crop_augment, applied in this order per output pixel. */
#define HPS_TRAIN_RESAMPLE 1          /* utils/image_utils.py:348-370: F.affine_grid + F.grid_sample(align_corners=False) by theta:
                                         nearest (half to even; out of frame -> -1) for part, bilinear zero-padded for rgb.  Without
                                         it the inputs are read pixel for pixel and every output is H x W (D is ignored) */
#define HPS_TRAIN_COUNT 128           /* part_counts[b] += pixels of the sampled part per 14-part label (label_conversions.py:38-72) */
#define HPS_TRAIN_COUNT14 256         /* the same for a plane that already holds 14-part labels */
#define HPS_TRAIN_CROP_CLASS_MASK 4   /* classes of plan word 0 -> 0 (random_extreme_crop) */
#define HPS_TRAIN_CLASS_MASK 2        /* classes of plan word 1 -> 0 (random_remove_bodyparts) */
#define HPS_TRAIN_SEG_OCCLUDE 8       /* box, bottom, top, vertical ranges -> 0 */
#define HPS_TRAIN_BACKGROUND 16       /* utils/image_utils.py:48-59: background where the part is 0 (-1, out of frame, keeps rgb) */
#define HPS_TRAIN_RGB_OCCLUDE 32      /* the RGB ranges -> 0 */
#define HPS_TRAIN_RGB_NOISE 64        /* times the channel factor, clamped at 1.0 from above only */
#define HPS_TRAIN_ALL_STAGES 511

/* train/train_poseMF_shapeGaussian_net.py:203-244 for the images, one pass: part and rgb (B,3,H,W) are sampled at theta (from
 * hps_seg_bbox_affine), the part counts taken from the raw sample, the segmentation augmentations applied, the background
 * (B,3,D,D) composited, the RGB augmentations applied; rgb_out (B,3,D,D), D the side of the square output.  Optional outputs (NULL
 * skips): part_crop (B,D,D) the
 * sampled plane, part_aug (B,D,D) the augmented one.  rgb may be NULL when only planes are wanted, part when only the RGB stages
 * are.  part_counts is added to with integer adds (exact, order-free); the caller -- or hps_seg_bbox_affine -- zeroes it.
 * Each lane writes four consecutive pixels of a row with one 16-byte store per plane where the address allows, else pixel by pixel. */
int hps_train_crop_augment(const float* part, int64_t part_batch_stride, const float* rgb, const float* background,
                           const float* theta, const int32_t* plan, int B, int H, int W, int D, int stages, float* rgb_out,
                           int32_t* part_counts, float* part_crop, float* part_aug, hps_stream_t stream);

/* Stages of hps_train_joints2d. */
#define HPS_TRAIN_J_PRE_VIS 1    /* utils/joints2d_utils.py:13-26 on the given joints */
#define HPS_TRAIN_J_AFFINE 2     /* utils/image_utils.py:359-363 */
#define HPS_TRAIN_J_POST_VIS 4   /* :13-26 on the transformed joints */
#define HPS_TRAIN_J_OCCLUDED 8   /* :29-45: joints 7-10, 13-16 need part_counts > pixel_count_threshold */
#define HPS_TRAIN_J_SEG_AUG 16   /* augment_proxy_representation's joint side: swaps, deviations, removals, half-occlusion tests */
#define HPS_TRAIN_J_RGB_AUG 32   /* augment_rgb's joint side */
#define HPS_TRAIN_J_ALL_STAGES 63

/* train/train_poseMF_shapeGaussian_net.py:181-183, :216-244 for the joints: joints2d (B,K,2) = (u, v), K = 17.  Follows
 * hps_train_crop_augment in stream order when it reads part_counts.  vis_in (B,K) bytes, optional starting visibility.  Outputs, each
 * optional: joints_target (B,K,2) the transformed joints, joints_input (B,K,2) the augmented ones, vis (B,K) float 0/1 and vis_u8
 * (B,K) bytes 0/1 -- the final visibility, the loss's joints2D_vis and the heat-map mask alike. */
int hps_train_joints2d(const float* joints2d, const uint8_t* vis_in, const float* affine, const int32_t* part_counts,
                       const int32_t* plan, int B, int K, float img_wh, int pixel_count_threshold, int stages, float* joints_target,
                       float* joints_input, float* vis, uint8_t* vis_u8, hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation metrics  
 * ---------------------------------------------------------------------------------------- */

/* Per point-set L2 error sums (metrics/eval_metrics_tracker.py:89-269).  pred (S,P,3); prediction s is compared with
 * target set s / group of target (ceil(S/group),P,3).  mode 0: raw; 1: after scale_and_translation_transform_batch
 * (utils/eval_utils.py:70-89); 2: after the Procrustes similarity transform (utils/eval_utils.py:11-59).
 * err_sum (S,) double = sum_i || transform(pred_i) - target_i ||.  Workspaces: stats_ws (S,17) double, xf_ws (S,12)
 * float (receives the applied 3x4 transforms).  transformed: optional (S,P,3) transformed predictions. */
int hps_pointset_errors(const float* pred, const float* target, int S, int group, int P, int mode,
                        double* stats_ws, float* xf_ws, double* err_sum, float* transformed,
                        hps_stream_t stream);

/* Result checksums (bench.py / the sharding-invariance tests; no reference counterpart): out[0] = first, out[1 + j] =
 * sum of xs[j][0 .. ns[j]) (of |x| where take_abs[j]) accumulated in float64 in a fixed order, for count <= 4 float tensors
 * in two launches.  xs / ns / take_abs are HOST arrays; partial_ws: 4 * 128 doubles; out: 1 + count doubles (device).
 * accumulate (optional, 1 + count doubles, device): a running total, accumulate[k] += out[k] in the second launch (a loop's
 * accumulator without a launch of its own). */
int hps_sums_f64(const float* const* xs, const int64_t* ns, const int32_t* take_abs, int count, double first,
                 double* partial_ws, double* out, double* accumulate, hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Matrix-Fisher likelihood and the pose / shape loss  (losses/matrix_fisher_loss.py)
 * ---------------------------------------------------------------------------------------- */

/* log c(S) of the matrix-Fisher distribution, LogMFNormConstant (:134-192).  S (n,3): proper singular values.
 *   log_c (n,) = log c_bar(S) + s0 + s1 + s2 with c_bar by the reference's own rule (:48-96, :157-170): 512 trapezoid nodes on [-1, 1]
 *   (end weights 1/2) over the integrand I0bar((s1 - s2)(1 - u)/2) I0bar((s1 + s2)(1 + u)/2) exp((s2 + s0)(u - 1)), I0bar the
 *   exp-scaled Numerical Recipes polynomials of :9-11, :30-45 -- not a better quadrature, which would differ from it by up to units
 *   in log c at concentrations of 10^4.
 *   grad_log_c / grad_S, both or neither: grad_S (n,3) = d log c / dS * grad_log_c, from the three cyclic-shift integrals of :99-131,
 *   :173-192, evaluated in the same pass over the nodes.  log_c may be NULL when only the gradient is wanted.
 * One wave64 per row, fp64 arithmetic inside, every output rounded once. */
int hps_mf_log_norm_const(const float* S, int n, float* log_c, const float* grad_log_c, float* grad_S, hps_stream_t stream);

/* matrix_fisher_nll (:195-228) over n rows: nll (n,) = -<F, R> + overreg * log c(s0, s1, s2 * det(U V^T)) -- the determinant's VALUE
 * multiplies s2, as at :222-224 (whose torch.det(...).cpu() is a host round trip; here it is formed in the kernel).  F, U, V, R (n,3,3),
 * S (n,3).  Backward (grad_nll (n,) not NULL): grad_F = -R * grad_nll and grad_S = overreg * grad_nll * d log c / d s_proper with the
 * s2 entry times det (either may be NULL, and nll too); U and V get no gradient (the reference uses them under no_grad). */
int hps_mf_nll(const float* F, const float* U, const float* S, const float* V, const float* R, int n, double overreg, float* nll,
               const float* grad_nll, float* grad_F, float* grad_S, hps_stream_t stream);

/* PoseMFShapeGaussianLoss (:231-301), all six terms from one argument block:
 *   pose NLL       matrix_fisher_nll over n_pose rows (:254-259)
 *   shape NLL      -sum over betas of Normal(loc, scale).log_prob(target), (shape_B, n_shape / shape_B) (:266)
 *   joints2D MSE   the entries of VISIBLE joints only: predictions (j2d_B, Ns, K, 2) against targets (j2d_B, K, 2) normalised by
 *                  2 t / img_wh - 1 and broadcast over the Ns samples; visibility (j2d_B, K) bytes 0 / 1 -- what :273-283 selects with
 *                  boolean masks (a host round trip each on a GPU), counted on the device here
 *   glob-rotmat, vertex and joints3D MSE over n_glob / n_verts / n_joints3d elements (:286-292)
 * each reduced by `reduction` -- under HPS_MF_REDUCTION_MEAN a mean over no element (no visible joint) is NaN, and so is the total
 * then, whatever the term's weight, as in the reference -- then weighted and added in the reference's order (:294-299).  All
 * arrays contiguous fp32 (the visibility bytes excepted); g_* are the backward's outputs, shaped like their predictions, NULL = not
 * wanted (the forward ignores them).  struct_bytes = sizeof(hps_mf_loss_args) as the caller compiled it: a mirror that drifts is
 * rejected instead of read. */
#define HPS_MF_REDUCTION_MEAN 0
#define HPS_MF_REDUCTION_SUM 1
typedef struct hps_mf_loss_args {
    int struct_bytes;
    int reduction;                                             /* HPS_MF_REDUCTION_* (loss_config.REDUCTION) */
    int64_t n_pose;                                            /* matrix-Fisher rows (B * 23) */
    int64_t shape_B, n_shape;                                  /* rows and elements of the shape distribution */
    int64_t j2d_B, Ns, K;                                      /* joints2D geometry */
    int64_t n_glob, n_verts, n_joints3d;                       /* elements of the three plain MSE terms */
    double img_wh, overreg;                                    /* img_wh, loss_config.MF_OVERREG */
    double weights[6];                                         /* WEIGHTS.POSE, SHAPE, JOINTS2D, GLOB_ROTMATS, VERTS3D, JOINTS3D */
    const float *pose_F, *pose_U, *pose_S, *pose_V;            /* predictions */
    const float *shape_loc, *shape_scale, *joints2d, *glob_rotmats, *verts, *joints3d;
    const float *t_pose_rotmats, *t_shape, *t_joints2d;        /* targets */
    const uint8_t* t_joints2d_vis;
    const float *t_glob_rotmats, *t_verts, *t_joints3d;
    float *g_pose_F, *g_pose_S, *g_shape_loc, *g_shape_scale;  /* gradients of the predictions (U and V get none) */
    float *g_joints2d, *g_glob_rotmats, *g_verts, *g_joints3d;
} hps_mf_loss_args;

/* Forward, 2 launches: per-workgroup fp64 partial sums -- one wave per pose row, whose d log c / ds and det go to the workspace --
 * then one workgroup that adds them in a fixed order (bitwise reproducible) and writes *total (one float, device).  workspace:
 * hps_query_workspace(HPS_WS_MF_LOSS, n_pose) bytes, 8-byte aligned, kept unchanged until the backward call.
 * Backward, 1 launch: every g_* that is not NULL = d total / d prediction * grad_total[0] (a device scalar: no host round trip).
 * Replaces :254-301 with the autograd graph behind it (118 + 347 aten operators per normaliser on (rows x 512) temporaries). */
int hps_mf_loss_forward(const hps_mf_loss_args* args, void* workspace, float* total, hps_stream_t stream);
int hps_mf_loss_backward(const hps_mf_loss_args* args, const void* workspace, const float* grad_total, hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The optimiser step  (run_train.py:97 optim.Adam(pose_shape_model.parameters(), lr=1e-4);
 * train/train_poseMF_shapeGaussian_net.py:346-349 optimiser.zero_grad / loss.backward / optimiser.step; csrc/optim.hip)
 * ---------------------------------------------------------------------------------------- */

/* One tensor of a step: torch/optim/adam.py _single_tensor_adam with this tensor's own hyper-parameters.  bias_correction1 =
 * 1 - beta1^t and bias_correction2_sqrt = sqrt(1 - beta2^t) are computed on the host, in double, as torch computes them.
 * decoupled: weight_decay multiplies the parameter by 1 - lr weight_decay (AdamW) instead of adding weight_decay p to the gradient.
 * All four arrays contiguous fp32 of numel elements; 16-byte aligned arrays take 16-byte accesses, any other alignment 4-byte ones. */
typedef struct hps_adam_entry {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
    double lr, beta1, beta2, eps, weight_decay;
    double bias_correction1, bias_correction2_sqrt;
    int decoupled;
    int reserved;
} hps_adam_entry;
#define HPS_ADAM_CHUNK 4096 /* elements of one workgroup */
int hps_sizeof_adam_entry(void);

/* ONE launch for all tensors of a step.  table: n_tensors entries in DEVICE memory; block_map: n_blocks pairs (tensor, chunk) of
 * int32 in device memory, workgroup i updates elements [chunk HPS_ADAM_CHUNK, (chunk + 1) HPS_ADAM_CHUNK) of its tensor -- every
 * element of every tensor belongs to exactly one pair.  Per element, in float64 from the fp32 values, each of p, m, v rounded once:
 *   g += weight_decay p (L2)  |  p *= 1 - lr weight_decay (decoupled);   m += (1 - beta1)(g - m);   v = beta2 v + (1 - beta2) g^2;
 *   p -= (lr / bias_correction1) m / (sqrt(v) / bias_correction2_sqrt + eps).
 * No atomics, bitwise repeatable, a tensor's result does not depend on the other tensors of the launch.  n_tensors == 0 or
 * n_blocks == 0: nothing is launched. */
int hps_adam_step(const hps_adam_entry* table, int n_tensors, const int32_t* block_map, int n_blocks, hps_stream_t stream);

/* One derived tensor of a prepared state written again, in place, from its parameter (resnet.py _ConvBN, ResNet._dgrad_filter;
 * poseMF_shapeGaussian_net.py prepare / _prepare_backward).  Elements of dst the op does not name (padding) are not touched.
 *   HPS_REFRESH_PERMUTE  dst[sum_k i_k dstride[k]] = src[sum_k i_k sstride[k]] for i_k < n[k]: the k-major, n-major and row-mode
 *                        filters, the data-gradient filter, the head's transposed copies and concatenations.  aux0 != NULL:
 *                        times aux0[i_scale_dim] in float64, rounded once (the data-gradient filter with the fold's scale).
 *   HPS_REFRESH_FOLD     eval-mode BatchNorm over n[0] channels: src = weight, aux0 = bias, aux1 = running_mean, aux2 = running_var;
 *                        dst = scale = weight / sqrt(var + eps), dst2 = shift = bias - mean scale; float64, rounded once.
 *   HPS_REFRESH_WINO_U   src (n[0] = Cout, n[1] = Cin, 3, 3) -> G g G^T in hps_conv3x3_winograd's layout; float64, rounded once.
 *   HPS_REFRESH_STEM_U   src (64, 18, 7, 7) -> the 81 positions of hps_stem_winograd; float64, rounded once. */
enum { HPS_REFRESH_PERMUTE = 0, HPS_REFRESH_FOLD = 1, HPS_REFRESH_WINO_U = 2, HPS_REFRESH_STEM_U = 3 };
typedef struct hps_refresh_op {
    int kind;
    int scale_dim;
    const float* src;
    float* dst;
    float* dst2;
    const float* aux0;
    const float* aux1;
    const float* aux2;
    double eps;
    int n[4], sstride[4], dstride[4];
} hps_refresh_op;
int hps_sizeof_refresh_op(void);

/* Issues ops[0..n_ops) in order on `stream`; the list (HOST memory) is built once per prepared state and run after every optimiser
 * step.  Up to 16 consecutive ops share a launch and run in no order within it; an op whose src / aux pointer EQUALS the dst / dst2
 * pointer of an earlier op of the same launch starts a new launch (stream order).  That is the only dependence the library sees: the
 * caller keeps overlapping ranges, destinations reached at an offset and write-after-read out of one run of 16, or orders the list
 * so that they cannot meet.  Null pointers, unknown kinds and impossible extents are refused before any launch. */
int hps_weights_refresh(const hps_refresh_op* ops, int n_ops, hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The training renderer  (train/train_poseMF_shapeGaussian_net.py:186-196; renderers/pytorch3d_textured_renderer.py:223-290
 * with run_train.py:86-91's defaults: blur_radius 0, one face per pixel, no perspective correction, no culling, no clipping,
 * HardPhongShader, under no_grad; csrc/render.hip)
 * ---------------------------------------------------------------------------------------- */

/* A hard nearest-face rasteriser with Phong shading, forward only.  pytorch3d is restated here, not linked:
 *   vertices   v = vertices[:, verts_map] (:264).  X = -(x + tx), Y = -(y + ty), Z = z + tz (the camera's diag(-1,-1,1) and the
 *              translation's sign flip, :155-163, :254).  Perspective: x_ndc = (s_x X) / Z, y_ndc = (s_y Y) / Z with s = 2 f / W;
 *              orthographic: x_ndc = s_x X, y_ndc = s_y Y with s = orthographic_scale.  z = Z in both.  Square images only.
 *   pixels     row r, column c samples (1 - (2 c + 1) / W, 1 - (2 r + 1) / W): a vertex lands in the pixel
 *              cam_utils.perspective_project_torch gives it (u = c + 0.5).
 *   coverage   E(p, a, b) = (p.x - a.x)(b.y - a.y) - (p.y - a.y)(b.x - a.x); area = E(v2, v0, v1); a face with |area| <= 1e-8 or
 *              with its largest z < 1e-8 is skipped; w0 = E(p, v1, v2) / (area + 1e-8), w1 = E(p, v2, v0) / (area + 1e-8),
 *              w2 = E(p, v0, v1) / (area + 1e-8); covered only if all three are > 0 (a centre on an edge belongs to no face);
 *              pz = w0 z0 + w1 z1 + w2 z2, skipped at that pixel if pz < 0.
 *   depth      the smallest pz wins, on equal pz the lower face index; empty pixels: pix_to_face = -1, depth = -1, bary = -1.
 *   IUV        sum of w verts_iuv (Nd,3), shared by the batch (:266-267, lights (1,1,1), (0,0,0), (0,0,0): the texel itself).
 *   texel      texture (B,Ht,Wt,3): (u, v) = sum of w verts_uv (Nd,2), x = u (Wt - 1), y = (1 - v)(Ht - 1), both clamped to the map,
 *              bilinear with a + t (b - a) along x twice, then along y (TexturesUV, align_corners = True, border) -- or, when
 *              verts_features (B,V,3) is given, sum of w verts_features[:, verts_map] (TexturesVertex, :269-271).
 *   Phong      vertex normal = sum over the vertex's faces, in the order of the table (vf_offsets (Nd+1), vf_faces: compressed sparse
 *              rows, built once on the host), of cross(v1 - v0, v2 - v0), divided by max(|n|, 1e-6).  n = normalise(sum of w n_v),
 *              P = sum of w v, L = normalise(light_location - P), view = normalise((-tx, -ty, -tz) - P), each by max(|.|, 1e-6);
 *              diffuse = diffuse_color relu(n.L); reflect = -L + 2 (n.L) n; specular = specular_color (relu(view.reflect) [n.L > 0])^64
 *              (six squarings); rgb = min(1, (ambient_color + diffuse) texel + specular) (:285); background (0,0,0).
 * Outputs, each NULL = not wanted, planar: iuv, rgb, bary (B,3,W,W), depth (B,W,W), pix_to_face (B,W,W) int32 (the face's index in
 * `faces`), iuv_train (B,3,W,W) = iuv with U and V times 255, all three rounded half to even (:193-195).
 * cam_t, scale and the four light arrays are per image (stride 3, scale 2) or shared (stride 0).  verts_map (< num_verts), faces
 * (< num_dp_verts) and vf_faces (< num_faces) are read as they are: the caller checks them once, where it builds them.
 * Three launches (project; face boxes and vertex normals; rasterise and shade), no atomics, bitwise repeatable, nothing allocated:
 * workspace is hps_query_workspace(HPS_WS_RENDER, B, num_dp_verts, num_faces) bytes, 16-byte aligned.  B <= 65535, W <= 4096,
 * num_faces <= 2^24, texture sides <= 32768; HPS_E_BADARG otherwise.  struct_bytes = sizeof(hps_render_args) as the caller compiled it. */
#define HPS_RENDER_PERSPECTIVE 0
#define HPS_RENDER_ORTHOGRAPHIC 1
typedef struct hps_render_args {
    int struct_bytes;
    int B, H, W;
    int num_verts, num_dp_verts, num_faces;
    int projection;                                            /* HPS_RENDER_* */
    int tex_h, tex_w;
    int cam_t_stride, scale_stride;                            /* floats between images: 3 / 2, or 0 = shared */
    int light_stride[4];                                       /* location, ambient, diffuse, specular: 3 or 0 */
    const float* vertices;                                     /* (B, num_verts, 3) */
    const int32_t* verts_map;                                  /* (num_dp_verts) */
    const int32_t* faces;                                      /* (num_faces, 3) */
    const int32_t *vf_offsets, *vf_faces;                      /* (num_dp_verts + 1), (vf_offsets[num_dp_verts]) */
    const float *verts_iuv, *verts_uv;                         /* (num_dp_verts, 3), (num_dp_verts, 2) */
    const float *cam_t, *scale;
    const float *light_location, *ambient, *diffuse, *specular;
    const float* texture;                                      /* (B, tex_h, tex_w, 3) */
    const float* verts_features;                               /* (B, num_verts, 3) */
    void* workspace;
    float *iuv, *rgb, *depth;
    int32_t* pix_to_face;
    float *bary, *iuv_train;
} hps_render_args;
int hps_sizeof_render_args(void);
int hps_render(const hps_render_args* args, hps_stream_t stream);

/* Silhouette counts for the SSP-3D metrics  (evaluate/evaluate_poseMF_shapeGaussian_net.py:143-155, 192-203;
 * metrics/eval_metrics_tracker.py:294-328; csrc/render.hip).  M meshes in groups of `group` consecutive ones (a frame's mode mesh,
 * group 1, or its N samples, group N): mesh m is seen by camera row m / group of cam_t / scale (stride 3 / 2, or 0 = shared) and
 * scored against target image m / group.  With flip_x_pi != 0 a vertex is taken as (x, -y, -z) before the camera -- the reference's
 * rotation by pi about x (:144-147, :195-198); a negation is exact, so this is hps_render on vertices flipped beforehand.
 *   mask     pixel (r, c) of mesh m is set iff hps_render's rasteriser finds a face there (every coverage, area, z, pz and depth rule
 *            above; the nearest face wins, on equal depth the lower index) AND round_half_even(w0 I0 + w1 I1 + w2 I2) != 0, the sum
 *            formed as hps_render forms its I plane: convert_multiclass_to_binary_labels(iuv_images[..., 0].round()) (:153-155), bit
 *            for bit the mask hps_render's own iuv gives.  Only the I column of verts_iuv (num_dp_verts, 3) is read.
 *   target   (M / group, W, W) uint8, nonzero = foreground; NULL = no target (every pixel counts as background: fp = the set
 *            pixels, tn = the rest, tp = fn = 0).
 *   counts   (M, 4) int32 = [tp, fp, tn, fn] of each mesh against its target, tp + fp + tn + fn = W^2; 16-byte aligned.
 *   mask_out (M, W, W) uint8 holding 0 / 1.  counts and mask_out may each be NULL, not both.
 * Four launches (project; face and chunk boxes -- hps_render's set-up without its vertex normals; rasterise and count, one 16-byte
 * store per 8 x 8 tile; add a mesh's tile counts), three without counts; no atomics, no image is written but mask_out, bitwise
 * repeatable, nothing allocated.
 * workspace is hps_query_workspace(HPS_WS_SILHOUETTE, M, num_dp_verts, HPS_WS_SILHOUETTE_D2(num_faces, W)) bytes, 16-byte aligned.
 * The tile counts are 16 bytes per tile: sized for the largest image (512 x 512 tiles) they would be 4 MiB per mesh, more than
 * everything else in the workspace by two orders of magnitude, so the query takes W -- packed into d2 above the face count, which
 * is at most 2^24: d2 = num_faces + W * 2^32.
 * M in [1, 65535], group >= 1 dividing M, W in [1, 4096], num_faces <= 2^24; HPS_E_BADARG otherwise, before any launch.
 * struct_bytes = sizeof(hps_silhouette_args) as the caller compiled it. */
#define HPS_WS_SILHOUETTE_D2(num_faces, W) ((int64_t)(num_faces) + ((int64_t)(W) << 32))
typedef struct hps_silhouette_args {
    int struct_bytes;
    int M, W, group;
    int num_verts, num_dp_verts, num_faces;
    int projection;                                            /* HPS_RENDER_* */
    int flip_x_pi;
    int cam_t_stride, scale_stride;                            /* floats between GROUPS: 3 / 2, or 0 = shared */
    const float* vertices;                                     /* (M, num_verts, 3) */
    const int32_t* verts_map;                                  /* (num_dp_verts) */
    const int32_t* faces;                                      /* (num_faces, 3) */
    const float* verts_iuv;                                    /* (num_dp_verts, 3) */
    const float *cam_t, *scale;
    const uint8_t* target;                                     /* (M / group, W, W) or NULL */
    void* workspace;
    int32_t* counts;                                           /* (M, 4) or NULL */
    uint8_t* mask_out;                                         /* (M, W, W) or NULL */
} hps_silhouette_args;
int hps_sizeof_silhouette_args(void);
int hps_silhouette_iou(const hps_silhouette_args* args, hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training loss-and-metrics tracker  (metrics/train_loss_and_metrics_tracker.py)
 * ---------------------------------------------------------------------------------------- */

/* One training or validation step of TrainingLossesAndMetricsTracker.update_per_batch (:113-196): every tracked metric of the batch is
 * formed on the device and added into running float64 sums that stay there until the epoch ends (the reference copies four (B,6890,3)
 * tensors to the host, calls loss.item() and runs numpy Procrustes every step, and keeps float32 sums).
 *   mask     HPS_TRAIN_METRIC_* bits, in the order of the reference's all_metrics_types.  Inputs that no set bit needs may be NULL.
 *   point sets  pred_verts / target_verts (B,P,3) for PVE, PVE-SC, PVE-PA (:118-138); pred_reposed / target_reposed (B,P,3) for PVE-T,
 *            PVE-T-SC (:141-150); pred_joints3d / target_joints3d (B,J,3) for MPJPE, MPJPE-SC, MPJPE-PA (:152-174).  B counts sets
 *            after the reference's reshape(-1, P, 3).  The arithmetic is hps_pointset_errors' (float64 statistics, the transform as 12
 *            floats, sqrtf per point, float64 sums in the same lane and tree order): a set's sum in a mode has the bits
 *            hps_pointset_errors gives for that set.  One statistics pass per family serves SC and PA; one workgroup forms the raw,
 *            SC and PA sums of a set, so the set comes from HBM once (three walks of hps_pointset_errors' own error loop -- the one
 *            body of machine code that has its bits -- of which the second and third find the set in the cache).
 *   2-D      pred_joints2d (B,K,2) normalised to [-1, 1], target_joints2d (B,K,2) in pixels: joints2D-L2E adds, over all B K joints,
 *            || (x + 1) img_wh / 2 - target || (:176-181).  pred_joints2d_samples (B,N,K,2), vis (B,K) bytes: joints2Dsamples-L2E adds
 *            the same over the visible joints of every sample, and their number B-wise sum(vis) N to its own slot (:183-196).
 *   loss     one device float; slot 0 receives (double)loss * batch_size (:114), slot 1 batch_size (:115).
 *   status   optional (num_status,) int32 (the synthetic front end's empty-box words): the number of non-zero words is added to the
 *            last slot.  NULL with num_status = 0: the slot is not touched.
 *   sums     (2, HPS_TRAIN_METRICS_NSLOT) double, row `split` (0 train, 1 val) is updated: slot 0 loss * batch_size, 1 samples,
 *            2 + b the metric of mask bit b, 12 visible joint samples, 13 non-zero status words.  Only the slots named by the call
 *            are written; the other row is not touched.  The caller zeroes sums at the start of an epoch.
 *   workspace  hps_query_workspace(HPS_WS_TRAIN_METRICS, B) bytes, 8-byte aligned.  After the call it holds the per-set values that
 *            were summed: double stats[3][B][17], double part[3][B][3] (family, set, mode), double j2d[B][3] (L2E, samples L2E,
 *            visible count), float xf[3][B][3][12]; entries of untracked metrics are not written.
 * Four launches whatever the mask (statistics; transforms; errors with the 2-D joints as a fourth grid row; one workgroup that adds the
 * per-set values in set order and then does sums[split][slot] += value, one lane per slot).  No atomics, bitwise repeatable, nothing
 * allocated, no host round trip.  HPS_E_BADARG before any launch: struct_bytes, B < 1, batch_size < 1, split outside {0, 1}, a mask bit
 * outside the ten, NULL for an input a set bit needs, P / J / K / N < 1 where used, img_wh <= 0 with a 2-D bit. */
enum { HPS_TRAIN_METRIC_PVE = 1, HPS_TRAIN_METRIC_PVE_SC = 2, HPS_TRAIN_METRIC_PVE_PA = 4, HPS_TRAIN_METRIC_PVE_T = 8,
       HPS_TRAIN_METRIC_PVE_T_SC = 16, HPS_TRAIN_METRIC_MPJPE = 32, HPS_TRAIN_METRIC_MPJPE_SC = 64, HPS_TRAIN_METRIC_MPJPE_PA = 128,
       HPS_TRAIN_METRIC_J2D = 256, HPS_TRAIN_METRIC_J2D_SAMPLES = 512, HPS_TRAIN_METRIC_ALL = 1023 };
#define HPS_TRAIN_METRICS_NSLOT 14
typedef struct hps_train_metrics_args {
    int struct_bytes;
    int B, P, J, K, N;
    int batch_size, mask, split, num_status;
    float img_wh;
    const float *pred_verts, *target_verts;                    /* (B, P, 3) */
    const float *pred_reposed, *target_reposed;                /* (B, P, 3) */
    const float *pred_joints3d, *target_joints3d;              /* (B, J, 3) */
    const float *pred_joints2d, *target_joints2d;              /* (B, K, 2) */
    const float* pred_joints2d_samples;                        /* (B, N, K, 2) */
    const uint8_t* vis;                                        /* (B, K) */
    const float* loss;
    const int32_t* status;                                     /* (num_status) or NULL */
    void* workspace;
    double* sums;                                              /* (2, HPS_TRAIN_METRICS_NSLOT) */
} hps_train_metrics_args;
int hps_sizeof_train_metrics_args(void);
int hps_train_metrics_update(const hps_train_metrics_args* args, hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The predict visualisations  (predict/predict_poseMF_shapeGaussian_net.py:149-333; csrc/visualise.hip)
 * ---------------------------------------------------------------------------------------- */

/* The layer between hps_render's planes and a PNG.  One launch each, no atomics, nothing allocated, bitwise repeatable, all on the
 * caller's stream; bad arguments return HPS_E_BADARG before any launch.  The `views` and `panels` tables are HOST arrays, read during
 * the call (they travel as kernel arguments); every other pointer is device memory.
 *
 * hps_vis_views  (:116-147, :174-190)  the vertex and colour buffers of every view of a figure, laid out as one hps_render batch:
 * out_vertices, out_colours (num_views, num_verts, 3).  View i reads the mesh views[i].vertices (num_verts, 3):
 *   position   first (x, y, z) -> (x, -y, -z), then yaw times (x, y, z) -> (-z, y, x): the reference's rotation by pi about x and by
 *              -pi / 2 about y with the trigonometry exact.  A view is a signed permutation of the coordinates; yaw 0 is bit for bit
 *              what hps_silhouette_iou's flip_x_pi sees.
 *   colour     views[i].var == NULL: `constant` on all three channels (the reference's 0.7 plain texture; it renders those views
 *              through a constant UV texture, here they take the per-vertex route so that all views share one render call -- the two
 *              routes differ by rounding in the interpolation of a constant only).  Otherwise var (num_verts) is the per-vertex
 *              variance and the colour is plt.cm.jet(plt.Normalize(0, 0.2, clip=True)(var))[:, :3] (:188-190): float64 arithmetic on
 *              the float32 value -- clip to [0, 0.2], / 0.2, * 256, truncate, 256 -> 255 -- and a look-up in lut (256, 3) float32
 *              (the colour map's table, built by the caller).  NaN gives (0, 0, 0).
 *   camera     out_cam_t (num_views, 3) and out_scale (num_views, 2) are hps_render's per-image cam_t and scale: a view with camera 1
 *              gets the predicted weak-perspective camera cam = [s, tx, ty] as [tx, ty, cam_z] and [s, s] (:151-154), a view with
 *              camera 0 gets fixed_cam_t and [fixed_scale, fixed_scale] (:51-52).
 * num_views in [1, HPS_VIS_MAX_VIEWS], yaw in [0, 3], num_verts in [1, 2^24]. */
#define HPS_VIS_MAX_VIEWS 32
typedef struct hps_vis_view {
    const float* vertices;                                     /* (num_verts, 3) */
    const float* var;                                          /* (num_verts) or NULL = the constant colour */
    int yaw;
    int camera;                                                /* 0 = the fixed camera, 1 = the predicted one */
} hps_vis_view;
typedef struct hps_vis_views_args {
    int struct_bytes;
    int num_views, num_verts;
    float constant;
    float fixed_cam_t[3], fixed_scale, cam_z;
    const hps_vis_view* views;                                 /* HOST (num_views) */
    const float* lut;                                          /* (256, 3) */
    const float* cam;                                          /* (3) = [s, tx, ty], or NULL when no view uses it */
    float *out_vertices, *out_colours;                         /* (num_views, num_verts, 3) */
    float *out_cam_t, *out_scale;                              /* (num_views, 3), (num_views, 2); both NULL = not wanted */
} hps_vis_views_args;
int hps_sizeof_vis_views_args(void);
int hps_vis_views(const hps_vis_views_args* args, hps_stream_t stream);

/* hps_vis_compose  (:198-205, :236-274, :303-333)  a finished figure out (rows wh, cols wh, 3) uint8, RGB interleaved, from a list of
 * panels; panel p fills grid cell (row, col), cells that no panel names are zero:
 *   RENDER            the planar float rgb (num_renders, 3, wh, wh) of render `render`.
 *   RENDER_OVER_CROP  that render where round_half_even(iuv[render][0]) != 0, elsewhere the CROP value (batch_add_rgb_background on
 *                     iuv_images[..., 0].round(), :202-204); iuv is hps_render's (num_renders, 3, wh, wh).
 *   CROP              crop (3, D, D) resized to wh as F.interpolate(mode='bilinear', align_corners=False) samples it (:198-201):
 *                     output index i reads position max((i + 0.5) D / wh - 0.5, 0), the upper neighbour clamped to D - 1;
 *                     h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11) in float32.  crop == NULL: black.
 *   PROXY             the sum over proxy's (proxy_channels, D, D) channels, resized with the same positions (cv2.resize's
 *                     INTER_LINEAR, :245-247), grey on three channels; then a filled red disc, dx^2 + dy^2 <= 9, at
 *                     (int(x wh / D), int(y wh / D)) (float64, as Python forms it) for each of joints (num_joints, 2) (:248-255;
 *                     joints == NULL: none).  The joint numbers and confidences of :256-263 are NOT drawn.
 * Every value v becomes clamp(rint(255 v), 0, 255), rint to even -- what cv2.imwrite does to a float image (a disc is (255, 0, 0)).
 * A lane produces 16 consecutive bytes of the figure and stores one dwordx4; out is 16-byte aligned.  rows cols <= HPS_VIS_MAX_CELLS,
 * wh in [1, 4096], the figure smaller than 2^31 bytes, D in [1, 8192]. */
#define HPS_VIS_MAX_CELLS 32
#define HPS_VIS_PANEL_RENDER 0
#define HPS_VIS_PANEL_RENDER_OVER_CROP 1
#define HPS_VIS_PANEL_CROP 2
#define HPS_VIS_PANEL_PROXY 3
typedef struct hps_vis_panel {
    int kind;                                                  /* HPS_VIS_PANEL_* */
    int row, col;
    int render;                                                /* RENDER, RENDER_OVER_CROP: index into rgb / iuv */
} hps_vis_panel;
typedef struct hps_vis_compose_args {
    int struct_bytes;
    int rows, cols, wh;
    int num_panels, num_renders;
    int D, proxy_channels, num_joints;
    const hps_vis_panel* panels;                               /* HOST (num_panels) */
    const float *rgb, *iuv;                                    /* (num_renders, 3, wh, wh) */
    const float* crop;                                         /* (3, D, D) or NULL */
    const float* proxy;                                        /* (proxy_channels, D, D) */
    const float* joints;                                       /* (num_joints, 2) or NULL */
    uint8_t* out;                                              /* (rows wh, cols wh, 3) */
} hps_vis_compose_args;
int hps_sizeof_vis_compose_args(void);
int hps_vis_compose(const hps_vis_compose_args* args, hps_stream_t stream);

/* hps_vis_uncrop  (:278-300; utils/image_utils.py:195-229 with uncrop=True)  the render projected back onto the photograph:
 * out (H, W, 3) uint8 from rgb (3, wh, wh), iplane (wh, wh) (plane 0 of hps_render's iuv), the float photograph image (3, H, W) in
 * [0, 1], bbox_centre (2) = (vertical, horizontal) and bbox_wh (1) = max(h, w) BBOX_SCALE_FACTOR, both device floats.  For every pixel
 * of the photograph the position in the render follows cv2.warpAffine's arithmetic as we understand it -- these rules have NOT been
 * run against OpenCV itself:
 *   matrix    float32, as the reference builds it: m00 = m11 = side / wh, t = centre[::-1] - (side / wh) (wh / 2); inverted in float64
 *             the way warpAffine inverts (D = 1 / det, A11 = m11 D, ..., b = -A t).
 *   position  per column rint(M x 1024), per row rint((M y + b) 1024), plus 512 for the nearest look-up or 16 for the linear one;
 *             nearest index: >> 10; linear: >> 5, then the index is >> 5 and the fraction & 31 thirty-seconds; the four taps carry
 *             float32 weights (1 - fy)(1 - fx), ...; anything outside the render reads 0.
 * The part plane is looked up nearest, the colour linearly.  Where I == 0 the output is the photograph's own pixel, rint(255 image)
 * (exact for an image that was uint8 / 255); elsewhere rint(255 rgb), saturated.  A lane produces 16 consecutive bytes; out is
 * 16-byte aligned.  wh in [1, 4096], H and W in [1, 32767]. */
typedef struct hps_vis_uncrop_args {
    int struct_bytes;
    int H, W, wh;
    const float* rgb;                                          /* (3, wh, wh) */
    const float* iplane;                                       /* (wh, wh) */
    const float* image;                                        /* (3, H, W) */
    const float *bbox_centre, *bbox_wh;                        /* (2), (1) */
    uint8_t* out;                                              /* (H, W, 3) */
} hps_vis_uncrop_args;
int hps_sizeof_vis_uncrop_args(void);
int hps_vis_uncrop(const hps_vis_uncrop_args* args, hps_stream_t stream);

/* hps_png_encode  (no reference counterpart: the reference hands its pictures to cv2.imwrite; csrc/png.hip)  finished uint8 pictures
 * to the bytes of complete PNG files, so that only the compressed file crosses to the host.  Up to HPS_PNG_MAX_IMAGES pictures per
 * call share TWO launches; no atomics on global memory, nothing allocated, no host synchronisation, bitwise repeatable, and the bytes
 * of a picture do not depend on what else is in the call.  Picture i: pixels (H, W, C) contiguous uint8, C = 1 (greyscale) or 3 (RGB);
 * out receives the file -- signature, IHDR (8 bit, colour type 0 or 2, no interlace), IDAT chunks, IEND, every chunk CRC and the zlib
 * Adler-32 formed on the device -- and *length (device int64) its length in bytes; capacity, the bytes behind out, must be at least
 * hps_png_bound(H, W, C); workspace is hps_query_workspace(HPS_WS_PNG, H, W, C) bytes.  pixels, out and workspace are 16-byte
 * aligned, length 8-byte aligned; the buffers of different pictures do not overlap.
 *
 * The stream inside: the picture is cut into segments of hps_png_segment_rows(H, W, C) whole rows (the last may be shorter), each
 * compressed on its own and carried by its own IDAT chunk; a first IDAT chunk holds the zlib header 78 01, a last one the final empty
 * block 03 00 and the Adler-32.  A row takes filter Sub where the sum of its |Sub| residuals (as signed bytes) is smaller than that of
 * its |Up| residuals, else Up (the first row's Up is the row itself).  In a segment's filtered bytes, maximal runs of bytes equal to
 * their predecessor become matches of distance 1, cut into pieces of 258 from the run's start (a last piece shorter than 3 stays
 * literals); nothing reaches before the segment.  Tokens are coded with deflate's fixed Huffman tables and the segment closes with an
 * empty stored block, which ends it on a byte boundary; where one stored block is shorter, the segment is that stored block.
 *
 *
 * The above is a picture's stream under strategy = 0.  strategy = 1 keeps the container, the segments, the tokens and the close, and
 * changes the filters and the code; pictures of one call may differ in strategy, and the same two launches serve both.
 *   Filter: a row takes the type among None 0, Sub 1, Up 2, Average 3, Paeth 4 with the smallest sum of |residual| (as signed bytes);
 *     ties go to the lowest type.  Bytes left of the row and above the picture are 0, Average is floor((left + up) / 2).
 *   Counts: the segment's tokens' literal/length symbols (RFC 1951: 0..255, 257..285), and one end-of-block symbol 256.
 *   Code lengths, for an alphabet with counts and a limit M (M = 15 here, M = 7 for the code-length alphabet below):
 *     1. order the used symbols by descending count, ties by ascending symbol index;
 *     2. build the Huffman tree by the two-queue method: the leaves in ascending order of count, the internal nodes in the order of
 *        their creation, each step joining the two smallest heads, a leaf before an internal node of equal weight; count the leaves at
 *        every depth, a depth above M counting as M;
 *     3. while sum over depths d of leaves(d) 2^(M - d) exceeds 2^M: leaves(M) falls by one, and for the greatest i < M with
 *        leaves(i) > 0, leaves(i) falls by one and leaves(i + 1) rises by two (each round lowers the sum by one);
 *     4. the first leaves(1) symbols in the order of 1 take length 1, the next leaves(2) length 2, and so on.
 *     A single used symbol takes length 1 (this cannot happen to either alphabet here: a segment has a literal and the end-of-block
 *     symbol, its lengths have a non-zero value and a zero run or two different values).  Codes are deflate's canonical codes.  The
 *     result depends on the counts alone and is complete (Kraft sum 1).  On the device all lanes rank the symbols (286 broadcast LDS
 *     reads per symbol), climb from their leaves to the root and place their codes; one lane merges the two queues (at most 285 steps
 *     of two or three dependent LDS reads per segment) and runs step 3 over M counters.
 *   Distance code: one code of length 1 for distance symbol 0 (HDIST = 1 code), declared also when the segment holds no match.
 *   Header: BFINAL 0, BTYPE 10, HLIT = last used literal/length symbol + 1, HDIST = 1, HCLEN trimmed to the last used code-length symbol
 *     in deflate's permuted order.  The sequence of HLIT lengths and the one distance length is coded run by run of equal values: a run
 *     of z zeros is cut into pieces of 138 from its start, a piece of 11..138 is symbol 18, of 3..10 symbol 17, of 1 or 2 that many
 *     symbols 0; a run of r equal lengths v > 0 is v once, then the r - 1 others cut into pieces of 6 from their start, a piece of 3..6
 *     is symbol 16, of 1 or 2 that many symbols v.  The code-length alphabet's code comes from these symbols' counts by the rule above.
 *   A token is its literal/length code, the length's extra bits and, for a match, the one bit 0 of distance 1: at most 15 + 5 + 1 bits.
 *   Choice: the segment is its dynamic block and the closing empty stored block unless its strategy-0 form (the fixed block with the
 *     same close, or one stored block where that is shorter) is strictly shorter in bytes; then it is that form, on strategy 1's filtered
 *     bytes.  The fixed block stays a candidate because a segment of a few dozen bytes cannot pay for a code's header.  So no segment
 *     is longer than S + 5 bytes and hps_png_bound holds for both strategies.
 *
 * Supported: C in {1, 3}, W C in [1, 12288] (4096 RGB pixels), H in [1, 32768]; anything else is HPS_E_BADARG, as are null pointers,
 * a strategy other than 0 and 1, a wrong struct_bytes, num_images outside [1, HPS_PNG_MAX_IMAGES] and a capacity below the bound --
 * all before any launch.
 * hps_png_bound and hps_png_segment_rows are host functions; both return -1 (and set hps_last_error) outside the supported range.
 * hps_png_bound(H, W, C) = 77 + H (1 + W C) + 17 ceil(H / rows per segment): no file is longer (derivation: csrc/png.hip). */
#define HPS_PNG_MAX_IMAGES 8
typedef struct hps_png_image {
    const uint8_t* pixels;                                     /* (H, W, C) */
    int H, W, C;
    int strategy;                                              /* 0: fixed Huffman code, Sub / Up; 1: dynamic code, five filters */
    uint8_t* out;                                              /* (capacity) */
    int64_t capacity;
    int64_t* length;                                           /* (1) */
    void* workspace;
} hps_png_image;
typedef struct hps_png_encode_args {
    int struct_bytes;
    int num_images;
    hps_png_image image[HPS_PNG_MAX_IMAGES];
} hps_png_encode_args;
int hps_sizeof_png_encode_args(void);
int64_t hps_png_bound(int H, int W, int C);
int hps_png_segment_rows(int H, int W, int C);
int hps_png_encode(const hps_png_encode_args* args, hps_stream_t stream);

/* hps_jpeg_parse / hps_jpeg_decode  (no reference counterpart: the reference reads its images with cv2.imread on the host;
 * csrc/jpeg.hip, csrc/jpeg_decode.h)  the bytes of baseline JPEG files to the pixels PIL (libjpeg's defaults: islow IDCT, fancy
 * upsampling) gives, byte for byte, so that only the compressed file crosses to the device.
 *
 * hps_jpeg_parse is a HOST function: it walks the markers of data[0 .. length) and returns
 *   HPS_OK             *header is filled; the file is in the device profile;
 *   HPS_JPEG_NOT_FOR_DEVICE  a well-formed file outside the profile (hps_last_error says which rule); decode it on the host;
 *   HPS_E_BADARG       null pointer, or a MALFORMED file (hps_last_error names the place): no SOI, a segment length running past the
 *                      file, the file ending before a scan, a scan selecting a Huffman or quantisation table that was never
 *                      defined or a component the frame does not have, a Huffman table whose counts overflow its code space or whose
 *                      symbols run past its segment, a DC symbol above 15, table slots above 3, sampling factors outside 1..4.
 * The device profile: SOF0, or SOF1 with 8-bit samples (Huffman coded); one component, or three treated as YCbCr as libjpeg would
 * (JFIF; else Adobe transform 1; else component ids other than 'R','G','B'); luma sampling 1x1, 2x1 or 2x2 with both chroma
 * components 1x1 (4:4:4, 4:2:2, 4:2:0; a single component counts as 1x1 whatever it declares); ONE scan over all components in
 * frame order with Ss = 0, Se = 63, Ah = Al = 0, followed by EOI or the end of the file (a truncated file parses, and decodes with
 * a non-zero status); 8-bit quantisation tables; any DHT and DRI; width and height in [1, HPS_JPEG_MAX_DIM]; a file below 2^28
 * bytes with at most HPS_JPEG_MAX_SCAN_BYTES (4 MiB) of entropy-coded data (larger scans go to the host: see the worst case below).  APPn (EXIF orientation included, as Image.open ignores it), COM and unknown segments are skipped.  Outside it: progressive,
 * lossless, arithmetic, differential (SOF2..SOF15), 12-bit, two or four components (CMYK / YCCK), Adobe transform 0 or RGB ids,
 * other sampling factors, several scans, 16-bit tables, FF fill bytes inside the scan.
 * The header resolves the table slots: quant / dc / ac are indexed by COMPONENT; quant is in natural (row-major) order.
 * scan_offset / scan_length delimit the entropy-coded bytes inside the file.
 *
 * hps_jpeg_decode decodes 1 .. HPS_FRONTEND_MAX_IMAGES files of different sizes, samplings and tables in FIVE launches, whatever the
 * files hold; no host synchronisation, no atomics, nothing allocated, bitwise repeatable, and a file's pixels do not depend on what
 * else is in the call.  Per file: data (DEVICE) the whole file's bytes, at least header->file_bytes of them; header (HOST) what
 * hps_jpeg_parse wrote; header_dev (DEVICE, 4-byte aligned) a copy of *header, of which the kernels read the TABLES only (the sizes
 * travel by value from the host copy, so a bad device copy cannot move an address); out (DEVICE) the pixels; workspace (DEVICE,
 * 16-byte aligned) hps_query_workspace(HPS_WS_JPEG, scan_length, HPS_WS_JPEG_D1(width, height), HPS_WS_JPEG_D2(ncomp, hs, vs,
 * restart_interval)) bytes; buffers of different files do not overlap.  status (DEVICE, num_images int32) receives per file 0 or a
 * mask of HPS_JPEG_ST_*; rounds (DEVICE, num_images int32, or NULL) the rounds its synchronisation loop took.
 * mode HPS_JPEG_RGB: out is (H, W, 3) RGB, a one-component file's value repeated (PIL's convert("RGB")); HPS_JPEG_NATIVE: (H, W) for
 * a one-component file, (H, W, 3) for a three-component one; HPS_JPEG_GREY: (H, W), one-component files only.
 *
 * Entropy decoding is parallel INSIDE a file, restart markers or not (the self-synchronising scheme of Klein and Wiseman, as
 * Weissenberger and Schmidt run it on GPUs, with the fixed-point loop inside one launch):
 *   1. one workgroup per file removes the FF 00 stuffing and the RSTn markers and records where each restart interval starts;
 *   2. each interval's bits are cut into subsequences of subseq_bits (0: the default 512; else a power of two in [128, 4096]).  Lane s
 *      starts at its subsequence's first bit in the state (start of an MCU, block 0, coefficient 0), decodes symbols until the first
 *      symbol boundary at or behind its end and records (bit, block of the MCU, coefficient, blocks completed).  Every later round
 *      restarts each lane from its predecessor's record; a lane whose entry did not change keeps its record.  The loop ends with the
 *      first round that changes no record, or after as many rounds as the file has subsequences -- then lane k's entry is the
 *      sequential decoder's by induction.  One workgroup of 1024 lanes per file strides over its subsequences, so the loop needs no
 *      synchronisation between workgroups and the launch count does not depend on the content;
 *   3. in the same launch a segmented prefix sum of the blocks completed gives every lane its first block -- the first lane of
 *      interval i owns block i * restart_interval * blocks per MCU -- and a last pass writes the coefficients, DC as differences;
 *   4. a segmented prefix sum per component and restart interval makes the DC values absolute.
 * Every bit read is bounded by the interval's end: bits behind it read as zero; every coefficient write is bounded by the interval's
 * block range.  A corrupt or truncated stream gives a non-zero status and unspecified pixels, and touches nothing outside that
 * file's out and workspace.
 * WORST CASE.  Files from an encoder synchronise within tens of rounds (profiles/jpeg_decode_time.txt: 5 to 21).  The loop's bound is
 * the subsequence count n = 8 scan_length / subseq_bits, and a stream CRAFTED never to synchronise makes every round decode every
 * subsequence again: n^2 subseq_bits / 2 symbol steps at most, on one workgroup -- at the 4 MiB limit and 512 bits about 10^12, a launch
 * of minutes.  HPS_JPEG_MAX_SCAN_BYTES keeps it there; hand files of unknown origin to the host decoder.
 *
 * The arithmetic (libjpeg's defaults).  Dequantise with the table in natural order.  IDCT jidctint.c "islow", CONST_BITS 13,
 * PASS1_BITS 2, columns then rows: even part z1 = (c2 + c6) 4433, t2 = z1 - c6 15137, t3 = z1 + c2 6270, t0 = (c0 + c4) << 13,
 * t1 = (c0 - c4) << 13, t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2; odd part on (c7, c5, c3, c1): z1 = c7 + c1,
 * z2 = c5 + c3, z3 = c7 + c3, z4 = c5 + c1, z5 = (z3 + z4) 9633, the four times 2446, 16819, 25172, 12299, z1..z4 times -7373,
 * -20995, -16069, -3196, z3 += z5, z4 += z5, o0 = c7' + z1 + z3, o1 = c5' + z2 + z4, o2 = c3' + z2 + z3, o3 = c1' + z1 + z4;
 * outputs (t10 +- o3, t11 +- o2, t12 +- o1, t13 +- o0).  Column pass: (x + 2^10) >> 11; row pass: (x + 2^17) >> 18, + 128, clamped to
 * 0..255; arithmetic shifts of signed 32-bit values.  Chroma of ceil(W / hs) x ceil(H / vs) real samples, "fancy" upsampling with
 * the last real row and column standing in for anything beyond them and row -1 equal to row 0: h2v1 out[2i] = (3 s[i] + s[i-1] +
 * 1) >> 2, out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2; h2v2 with t[i] = 3 near[i] + far[i] (the upper output row takes the row above as
 * far, the lower the row below): out[2i] = (3 t[i] + t[i-1] + 8) >> 4, out[2i+1] = (3 t[i] + t[i+1] + 7) >> 4.  Colour, each clamped:
 * R = Y + ((91881 (Cr - 128) + 32768) >> 16), B = Y + ((116130 (Cb - 128) + 32768) >> 16),
 * G = Y + ((-22554 (Cb - 128) - 46802 (Cr - 128) + 32768) >> 16).
 *
 * HPS_E_BADARG before any launch: null pointers, a wrong struct_bytes (of the arguments or of a header), num_images outside
 * [1, HPS_FRONTEND_MAX_IMAGES], a subseq_bits that is neither 0 nor a power of two in [128, 4096], an unknown mode, a header whose
 * fields are outside the profile above or inconsistent (num_blocks, num_intervals, scan_offset + scan_length > file_bytes), a
 * misaligned workspace or header_dev.  HPS_E_UNSUPPORTED: HPS_JPEG_GREY asked of a three-component file. */
#define HPS_JPEG_MAX_DIM 8192
#define HPS_JPEG_MAX_SCAN_BYTES (1 << 22)
#define HPS_JPEG_NOT_FOR_DEVICE 1
#define HPS_JPEG_RGB 0
#define HPS_JPEG_NATIVE 1
#define HPS_JPEG_GREY 2
#define HPS_JPEG_ST_MARKERS 1    /* more RSTn markers than restart intervals, or one out of sequence */
#define HPS_JPEG_ST_CODE 2       /* a bit pattern that is no code of its table, or a zero run past coefficient 63 */
#define HPS_JPEG_ST_OVERRUN 4    /* a symbol reached behind the end of its restart interval (zero bits were read) */
#define HPS_JPEG_ST_SHORT 8      /* a restart interval ended before its blocks were complete */
typedef struct hps_jpeg_huff {
    uint8_t bits[16];                                          /* codes of length 1..16 */
    uint8_t vals[256];                                         /* the symbols in code order */
} hps_jpeg_huff;
typedef struct hps_jpeg_header {
    int struct_bytes;
    int width, height, ncomp;                                  /* ncomp 1 or 3 */
    int hs, vs;                                                /* luma sampling: 1x1, 2x1 or 2x2 (chroma is 1x1) */
    int restart_interval;                                      /* MCUs, 0: none */
    int scan_offset, scan_length;                              /* the entropy-coded bytes inside the file */
    int num_blocks, num_intervals;                             /* 8x8 blocks in the scan; restart intervals (>= 1) */
    int file_bytes;
    uint8_t quant[3][64];                                      /* per component, natural order */
    hps_jpeg_huff dc[3], ac[3];                                /* per component */
} hps_jpeg_header;
typedef struct hps_jpeg_image {
    const uint8_t* data;                                       /* DEVICE (file_bytes) */
    const hps_jpeg_header* header;                             /* HOST */
    const hps_jpeg_header* header_dev;                         /* DEVICE copy of *header */
    uint8_t* out;                                              /* DEVICE (H, W) or (H, W, 3) */
    void* workspace;                                           /* DEVICE */
} hps_jpeg_image;
typedef struct hps_jpeg_decode_args {
    int struct_bytes;
    int num_images;
    int mode;                                                  /* HPS_JPEG_RGB / _NATIVE / _GREY */
    int subseq_bits;
    int32_t* status;                                           /* DEVICE (num_images) */
    int32_t* rounds;                                           /* DEVICE (num_images) or NULL */
    hps_jpeg_image image[64];                                  /* HPS_FRONTEND_MAX_IMAGES */
} hps_jpeg_decode_args;
int hps_sizeof_jpeg_header(void);
int hps_sizeof_jpeg_decode_args(void);
int hps_jpeg_parse(const uint8_t* data /* HOST */, int64_t length, hps_jpeg_header* header /* HOST */);
int hps_jpeg_decode(const hps_jpeg_decode_args* args /* HOST */, hps_stream_t stream);

/* hps_jpeg_encode  (no reference counterpart: the reference hands its pictures to cv2.imwrite, which writes a JPEG for a .jpg name;
 * csrc/jpeg_encode.hip, csrc/jpeg_encode.h)  finished uint8 pictures to the bytes of complete baseline JPEG files, equal byte for
 * byte, whole file, to what libjpeg / libjpeg-turbo (PIL's Image.save(format="JPEG", quality=q, subsampling=s)) writes, so that only
 * the compressed file crosses to the host.  Up to HPS_JPEG_ENC_MAX_IMAGES pictures per call share FOUR launches, whatever their number
 * and sizes; no atomics on global memory (integer OR and ADD in LDS, on disjoint bits and order-independent sums), nothing allocated,
 * no host synchronisation, bitwise repeatable, and the bytes of a picture do not depend on what else is in the call.  Picture i:
 * pixels (H, W, C) contiguous uint8, C = 1 (greyscale) or 3 (RGB); quality in [1, 100]; sampling 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0),
 * ignored for C = 1; out receives the file and *length (device int64) its length in bytes; capacity, the bytes behind out, must be at
 * least hps_jpeg_encode_bound(H, W, C, sampling); workspace is hps_query_workspace(HPS_WS_JPEG_ENC, H, W, HPS_WS_JPEG_ENC_D2(C,
 * sampling)) bytes.  pixels, out and workspace are 16-byte aligned, length 8-byte aligned; the buffers of different pictures do not
 * overlap.  Nothing is written at or behind out + *length: the file is stored byte by byte and no zeroing reaches past it.
 *
 * The file.  Markers in this order: SOI; APP0 "JFIF\0", version 1.01, units 0, density 1 x 1, no thumbnail; one DQT segment per
 * table (8-bit entries in zig-zag order): luminance (table 0), then chrominance (table 1) when C = 3; SOF0: precision 8, height,
 * width, components 1..C with sampling factors (luminance hmax x vmax = 1x1, 2x1 or 2x2; chrominance 1x1) and quantisation table
 * 0 / 1 / 1; one DHT segment each for DC 0, AC 0 and, when C = 3, DC 1, AC 1 -- the tables of T.81 Annex K, K.3 to K.6; SOS over all
 * components with table selectors 00, 11, 11, then 00 3F 00; the scan; EOI.  No DRI, no restart markers.
 *   Quantisation tables: Annex K's K.1 and K.2; scale = 5000 / q (integer) for q < 50, else 200 - 2 q; an entry is
 *     (base scale + 50) / 100 (integer), clamped to 1..255.
 *   Colour, 16.16 fixed point, arithmetic shifts: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16,
 *     Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16, Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16.
 *   Planes: a component with factors (h, v) under (hmax, vmax) has ceil(W h / hmax) x ceil(H v / vmax) samples in ceil(. / 8) blocks
 *     each way.  The full-resolution plane repeats its last column to the right as far as the blocks reach and its last row down to a
 *     multiple of vmax rows; 2 x 2 down-sampling is (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2, ... by output column, 2 x 1 is
 *     (a + b + bias) >> 1 with bias 0, 1, 0, 1, ...; then the DOWN-SAMPLED plane repeats its last row to fill its last block row.
 *   MCUs in raster order, ceil(W / 8 hmax) x ceil(H / 8 vmax) of them; in an MCU luminance's hmax x vmax blocks row by row, then Cb,
 *     then Cr.  A luminance block beyond the component's block grid (last MCU column or row under 4:2:2 / 4:2:0) is a DUMMY: every AC
 *     coefficient zero, DC equal to the DC of the block before it in the MCU.
 *   DCT: libjpeg's accurate integer forward DCT (jfdctint.c: 13-bit constants, 2 pass-1 bits, rows then columns) on samples - 128;
 *     its output is the coefficient times 8.  Per 1-D pass over (d0 .. d7): t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6,
 *     t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4, t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2; rows:
 *     o0 = (t10 + t11) << 2, o4 = (t10 - t11) << 2, the others (x + 2^10) >> 11; columns: o0 = (t10 + t11 + 2) >> 2, o4 likewise, the
 *     others (x + 2^14) >> 15; z1 = (t12 + t13) 4433, o2 = z1 + t13 6270, o6 = z1 - t12 15137; z1 = t4 + t7, z2 = t5 + t6,
 *     z3 = t4 + t6, z4 = t5 + t7, z5 = (z3 + z4) 9633, t4..t7 times 2446, 16819, 25172, 12299, z1..z4 times -7373, -20995, -16069,
 *     -3196, z3 += z5, z4 += z5, o7 = t4 + z1 + z3, o5 = t5 + z2 + z4, o3 = t6 + z2 + z3, o1 = t7 + z1 + z4.
 *   Quantisation with table entry Q: sign(c) ((|c| + (8 Q >> 1)) / (8 Q)), integer division.
 *   Entropy code (T.81 F.1.2): DC as the difference to the component's previous block in scan order (dummies included; 0 before the
 *     first): the code of its size, then size bits (the value, or value - 1 for a negative one, low bits).  AC in zig-zag order:
 *     run/size symbols with the value's bits, ZRL (F0) for each 16 zeros before a non-zero coefficient, EOB (00) when the block ends in
 *     zeros.  The last byte is padded with 1 bits; every FF of the scan -- a padded one too -- is followed by 00.
 * Out of scope: optimised Huffman tables, progressive, restart markers, arithmetic coding, 12-bit, CMYK, EXIF / ICC.
 *
 * On the device (csrc/jpeg_encode.hip): workgroups of 192 lanes take 192 consecutive blocks of the scan in every launch.  1. blocks:
 * one lane per block, samples to quantised zig-zag coefficients, the AC part's bit count; 2. bit counts: the DC difference, the
 * block's bits, the workgroup's sum; 3. bits: the workgroup's offset is the sum of the sums before it; the blocks' bits go into an LDS
 * buffer by atomic OR on zeroed words (the bits are disjoint, so the result is exact), the two blocks before the workgroup's first
 * are coded again so that the byte shared with the neighbour is complete, and the workgroup stores the bytes whose last bit is its
 * own into the unstuffed stream and counts its FF bytes; 4. file: header, every workgroup's bytes at header + index + FF bytes before,
 * with the stuffing, EOI and *length.
 *
 * HPS_E_BADARG before any launch: null pointers, a wrong struct_bytes, num_images outside [1, HPS_JPEG_ENC_MAX_IMAGES], C other than
 * 1 and 3, H or W outside [1, 8192] (the decoder's HPS_JPEG_MAX_DIM), quality outside [1, 100], sampling outside 0..2 (C = 3), a
 * capacity below the bound, pixels / out / workspace not 16-byte aligned, length not 8-byte aligned.
 * hps_jpeg_encode_bound is a host function; -1 (and hps_last_error) outside the supported range.  It is the header (328 bytes for
 * C = 1, 623 for C = 3) + 2 ceil(1660 blocks / 8) + 2: a block is at most 22 + 63 * 26 = 1660 bits before stuffing, stuffing at most
 * doubles a byte (derivation: csrc/jpeg_encode.hip). */
#define HPS_JPEG_ENC_MAX_IMAGES 8
typedef struct hps_jpeg_enc_image {
    const uint8_t* pixels;                                     /* (H, W, C) */
    int H, W, C;
    int quality;                                               /* 1 .. 100 */
    int sampling;                                              /* 0: 4:4:4, 1: 4:2:2, 2: 4:2:0; ignored for C = 1 */
    int reserved;                                              /* 0 */
    uint8_t* out;                                              /* (capacity) */
    int64_t capacity;
    int64_t* length;                                           /* (1) */
    void* workspace;
} hps_jpeg_enc_image;
typedef struct hps_jpeg_encode_args {
    int struct_bytes;
    int num_images;
    hps_jpeg_enc_image image[HPS_JPEG_ENC_MAX_IMAGES];
} hps_jpeg_encode_args;
int hps_sizeof_jpeg_encode_args(void);
int64_t hps_jpeg_encode_bound(int H, int W, int C, int sampling);
int hps_jpeg_encode(const hps_jpeg_encode_args* args, hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * HRNet 2D keypoint detector, inference forward  (models/pose2D_hrnet.py:426-461)
 * ---------------------------------------------------------------------------------------- */

/* Grouped convolution for 16-channel granularity (csrc/conv_c16.hip): the HRNet layers the encoder's kernels do not take (branch
 * widths 48 and 96, maps of 96 x 72 ... 12 x 9 pixels, the 17-channel final 1x1).  One launch runs 1 to HPS_C16_MAX_PROBLEMS
 * INDEPENDENT problems (the branches of a HighResolutionModule at the same block depth, :252-253); workgroups find their problem
 * from the block index in a descriptor table passed by value (no device allocation).  Per problem
 *     y = act(conv(x, w) * scale + shift [+ residual])
 * on the halo-padded NHWC frames of hps_conv2d_bn_act_pad: x (B, H + 2 ipad, W + 2 ipad, Cin) with a ZERO halo, ipad >= pad = K / 2;
 * y and residual (B, Ho + 2 opad, Wo + 2 opad, Cout), only y's interior is written, opad arbitrary.  K (= KH = KW) 1 or 3, stride 1
 * or 2, Cin % 16 == 0, any Cout >= 1, any H, W >= 1, B >= 0 (0: skipped).  w: (K * K, ceil16(Cout), Cin) -- tap-major in the order
 * (kh, kw), then output channel, input channel fastest; rows Cout .. ceil16(Cout) - 1 are zero (the host pads, the kernel masks the
 * tail).  scale / shift: (Cout), the folded BatchNorm, or scale = 1 and shift = bias for a convolution with a bias and no
 * BatchNorm (the final layer, :324-330).  x and w 16-byte aligned; with Cout % 4 == 0 also y, residual, scale, shift.
 * fp32 operands, fp32 accumulation on v_mfma_f32_16x16x4_f32, no atomics: bitwise repeatable.
 * SUMMATION ORDER of one output (the layer alone decides it -- never B, the tile an output lands in, or the other problems of the
 * launch; an image has the same bits alone and in a batch, a problem the same bits alone and in a group): accumulator 0; the taps in
 * the order (kh, kw); within a tap the 16-channel chunks c0 = 0, 16, ...; within a chunk four steps t = 0..3, each ONE matrix
 * instruction that adds the products of channels c0 + t, c0 + 4 + t, c0 + 8 + t, c0 + 12 + t to the accumulator; then
 * fma(acc, scale, shift), + residual, max(., 0).  Lane offsets are 32-bit: frames < 2^31 floats. */
#define HPS_C16_MAX_PROBLEMS 4
typedef struct hps_c16_problem {
    const float* x;
    const float* w;
    const float* scale;
    const float* shift;
    const float* residual;                                     /* or NULL */
    float* y;
    int B, H, W, ipad, Cin, Cout, K, stride, opad, relu;
} hps_c16_problem;
int hps_sizeof_c16_problem(void);
int hps_conv2d_bn_act_c16(const hps_c16_problem* problems /* HOST */, int n_problems, hps_stream_t stream);

/* The network input (:427): x (B, 3, H, W) NCHW -> the interior of the stem's frame y (B, H + 2 P, W + 2 P, CP), channels 0..2 and a
 * zero in channel 3 (one 16-byte store per pixel; CP % 4 == 0); the frame's other channels and its halo are the owner's zeros, part
 * of the convolution's zero padding.  With CP = 16 the 3 -> 64 stem is a hps_conv2d_bn_act_c16 problem like any other. */
int hps_hrnet_pack_input(const float* x, float* y, int B, int H, int W, int CP, int P, hps_stream_t stream);
/* The heat maps (:459-461): the interior of the NHWC frame x (B, H + 2 P, W + 2 P, C) -> y (B, C, H, W) NCHW. */
int hps_hrnet_unpack_output(const float* x, float* y, int B, int H, int W, int C, int P, hps_stream_t stream);

/* The fuse step of a HighResolutionModule (:255-264): y = act(((term0 + term1) + term2) + term3) on y's (B, H + 2 opad, W + 2 opad, C)
 * frame, interior only.  term k is a frame (B, (H >> shift_k) + 2 pad_k, (W >> shift_k) + 2 pad_k, C) read at (h >> shift_k,
 * w >> shift_k): shift 0 is a map of y's own resolution (the branch itself, or the end of a 3x3 / 2 chain), shift s the 1x1 + BN
 * output of a lower branch under nn.Upsample(scale_factor = 2^s, mode = 'nearest'), which is never materialised.  The additions run
 * in TERM ORDER, the reference's j order.  1 to HPS_HRNET_MAX_TERMS terms, C % 4 == 0, 2^shift_k divides H and W. */
#define HPS_HRNET_MAX_TERMS 4
typedef struct hps_hrnet_fuse_args {
    const float* term[HPS_HRNET_MAX_TERMS];
    int shift[HPS_HRNET_MAX_TERMS];
    int pad[HPS_HRNET_MAX_TERMS];
    int n_terms;
    float* y;
    int opad, B, H, W, C, relu;
} hps_hrnet_fuse_args;
int hps_sizeof_hrnet_fuse_args(void);
int hps_hrnet_fuse(const hps_hrnet_fuse_args* args /* HOST */, hps_stream_t stream);

/* The forward as one call (as hps_encoder_run: issuing ~130 launches through a scripting-language FFI costs more host time than the
 * GPU needs for them): ops[0..n_ops) in order on `stream`, the same launches as the individual entry points.  HPS_HRNET_PACK =
 * hps_hrnet_pack_input (x, y, B, H, W, C = CP, P), HPS_HRNET_CONV = hps_conv2d_bn_act_c16 (conv, n_problems), HPS_HRNET_FUSE =
 * hps_hrnet_fuse (fuse), HPS_HRNET_UNPACK = hps_hrnet_unpack_output (x, y, B, H, W, C, P). */
enum { HPS_HRNET_PACK = 0, HPS_HRNET_CONV = 1, HPS_HRNET_FUSE = 2, HPS_HRNET_UNPACK = 3 };
typedef struct hps_hrnet_op {
    int kind;
    int n_problems;
    hps_c16_problem conv[HPS_C16_MAX_PROBLEMS];
    hps_hrnet_fuse_args fuse;
    const float* x;
    float* y;
    int B, H, W, C, P;
} hps_hrnet_op;
int hps_sizeof_hrnet_op(void);
int hps_hrnet_run(const hps_hrnet_op* ops /* HOST */, int n_ops, hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Predict front end for a batch of photographs of different sizes  (csrc/predict_frontend.hip;
 * predict/predict_hrnet.py:34-117, predict/predict_poseMF_shapeGaussian_net.py:61-99, utils/image_utils.py:310-370)
 * ---------------------------------------------------------------------------------------- */

/* Per-image descriptors go BY VALUE in the argument structs (HOST memory, as hps_conv2d_bn_act_c16's problem table): no device
 * allocation, no pointer-table upload.  At most HPS_FRONTEND_MAX_IMAGES images per launch; a caller with more splits the batch.  All
 * three entry points validate on the host before any launch and only enqueue.  fp32 throughout, no fused multiply-adds, no atomics.
 *
 * The box RECORD, HPS_FRONTEND_RECORD_FLOATS floats per image, written by hps_predict_boxes and read by the other two:
 *   [0] [1]  bbox_centre (vertical, horizontal)          what predict_hrnet returns (:109-114) -- height and width AFTER both aspect
 *   [2] [3]  bbox_height, bbox_width                     fixes, because image_utils.py:311-312 assigns through the views it was given
 *   [4] [5]  box height, box width times scale_factor    (image_utils.py:321-322)
 *   [6] [7]  scale (horizontal, vertical) = out_wh / box_wh                       the forward affine of image_utils.py:329-334
 *   [8] [9]  shift (horizontal, vertical) = out_wh / 2 - scale * centre(h, v)
 *   [10]     index of the chosen detection, -1 for the whole image
 *   [11]     max(bbox_height, bbox_width) * scale_factor */
#define HPS_FRONTEND_MAX_IMAGES 64
#define HPS_FRONTEND_RECORD_FLOATS 12
#define HPS_FRONTEND_SRC_HWC_U8 0    /* (H, W, 3) uint8, a decoded photograph; value = float(u8) / 255.0f, a true division */
#define HPS_FRONTEND_SRC_CHW_F32 1   /* (3, H, W) float32 */

/* hps_predict_boxes  (predict_hrnet.py:48-87 and the aspect / scale / affine steps of image_utils.py:310-334)
 * Per image: H, W in [1, 32767] and optionally a detector's output -- boxes (n, 4) float (x1, y1, x2, y2), labels (n) int64, scores (n)
 * float, n >= 0; boxes == NULL: no detector.  Detections with label == 1 and score > threshold are kept; none: the whole image (centre
 * (H/2, W/2), height H, width W); otherwise the one with the smallest (cy - H/2)^2 + (cx - W/2)^2, the first index between equals.
 * hrnet_aspect_fix != 0 applies predict_hrnet's own aspect step (:83-87, if / elif, aspect = the float32 of the double out_h / out_w)
 * first; then always the two sequential masked assignments of image_utils.py:310-312 (aspect = the float32 quotient), the scale factor
 * and the affine.  Every value is one IEEE single operation of the reference, in its order: the record equals the reference's bit for bit. */
typedef struct hps_box_image {
    const float* boxes;
    const int64_t* labels;
    const float* scores;
    int n, H, W, reserved;
} hps_box_image;
typedef struct hps_predict_boxes_args {
    int struct_bytes;
    int B;
    int out_w, out_h;                                          /* the crop's size, out_wh of the reference */
    int hrnet_aspect_fix;
    float threshold, scale_factor;
    float* records;                                            /* (B, HPS_FRONTEND_RECORD_FLOATS) */
    hps_box_image image[HPS_FRONTEND_MAX_IMAGES];
} hps_predict_boxes_args;
int hps_sizeof_predict_boxes_args(void);
int hps_predict_boxes(const hps_predict_boxes_args* args /* HOST */, hps_stream_t stream);

/* hps_crop_bilinear  (image_utils.py:348-370: grid_sample, mode 'bilinear', padding_mode 'zeros', align_corners False)
 * raw (B, 3, out_h, out_w) and optionally normalised = (raw - mean[c]) / std[c] (a true division, transforms.Normalize) from one source
 * per image and its record.  Output pixel (i, j) samples the source at
 *     x = (j + 1/2) (box_w / out_w) + ((centre_h - box_w / 2) - 1/2),   y = (i + 1/2) (box_h / out_h) + ((centre_v - box_h / 2) - 1/2)
 * -- the reference's normalised theta written in pixel space -- with four taps at floor and floor + 1, weights (1 - fy)(1 - fx), ...,
 * summed in the order ((t00 + t01) + t10) + t11; a tap outside the image contributes zero INDIVIDUALLY.  A source row need not be
 * 4-byte aligned.  An image's values depend on its own descriptor and record only: same bits alone and in a batch. */
typedef struct hps_crop_image {
    const void* src;
    int H, W, kind, reserved;                                  /* kind: HPS_FRONTEND_SRC_* */
} hps_crop_image;
typedef struct hps_crop_bilinear_args {
    int struct_bytes;
    int B;
    int out_w, out_h;
    float mean[3], std[3];                                     /* read only with normalised != NULL */
    const float* records;                                      /* (B, HPS_FRONTEND_RECORD_FLOATS) */
    float* raw;                                                /* (B, 3, out_h, out_w) */
    float* normalised;                                         /* (B, 3, out_h, out_w) or NULL */
    hps_crop_image image[HPS_FRONTEND_MAX_IMAGES];
} hps_crop_bilinear_args;
int hps_sizeof_crop_bilinear_args(void);
int hps_crop_bilinear(const hps_crop_bilinear_args* args /* HOST */, hps_stream_t stream);

/* hps_hrnet_keypoints  (predict_hrnet.py:7-31, :104-107; predict_poseMF_shapeGaussian_net.py:97-99; image_utils.py:359-363)
 * heatmaps (B, K, h, w) NCHW; per (image, joint) the maximum and its FIRST index idx (one wave per map; a NaN is never the maximum):
 * confs = max; key point (idx % w, floor(idx / float(w))), zeroed unless max > 0, both coordinates times `factor`
 * (IMAGE_SIZE[0] / HEATMAP_SIZE[0]) -> joints_hrnet (B, K, 2); joints_crop (B, K, 2) = joints_hrnet * scale + shift of records (B, .)
 * (both NULL: not written); visib (B, K) = 1.0 where max > vis_threshold or bit k of always_visible is set, else 0.0.
 * K in [1, 32], h w < 2^24. */
typedef struct hps_hrnet_keypoints_args {
    int struct_bytes;
    int B, K, h, w;
    float factor, vis_threshold;
    uint32_t always_visible;
    const float* heatmaps;
    const float* records;                                      /* the proxy crop's records, or NULL */
    float* joints_hrnet;
    float* confs;
    float* joints_crop;                                        /* or NULL */
    float* visib;
} hps_hrnet_keypoints_args;
int hps_sizeof_hrnet_keypoints_args(void);
int hps_hrnet_keypoints(const hps_hrnet_keypoints_args* args /* HOST */, hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Device-side batch preparation for the datasets  (csrc/data_layer.hip; data/on_the_fly_smpl_train_dataset.py,
 * data/ssp3d_eval_dataset.py, data/pw3d_eval_dataset.py, utils/image_utils.py:62-231)
 * ---------------------------------------------------------------------------------------- */

/* Bandwidth kernels: no LDS, no atomics, nothing allocated, bit-identical from run to run.  Per-image descriptors go BY VALUE in the
 * argument structs (HOST memory), at most HPS_FRONTEND_MAX_IMAGES images per launch; every entry point validates on the host -- image
 * sizes, bank indices -- before its launch and only enqueues.  cv2.resize and cv2.warpAffine are restated from OpenCV's sources as we
 * understand them; they have NOT been run against OpenCV itself. */

/* hps_texture_gather  (on_the_fly_smpl_train_dataset.py:72-81)
 * out (B, Ht, Wt, 3) float32 = float(u8) / 255.0f, a true division (equal to float32(k / 255.), the reference's float64 route, for all
 * 256 levels), of texture idx[b] of the grey (is_grey[b] != 0) or the non-grey bank; banks (n, Ht, Wt, 3) uint8 on the device.  Any
 * Ht, Wt: a texture whose byte count is no multiple of 4, or whose place in the bank is unaligned, goes element by element. */
typedef struct hps_texture_gather_args {
    int struct_bytes;
    int B, Ht, Wt;
    int n_grey, n_nongrey;
    const uint8_t* grey;                                       /* (n_grey, Ht, Wt, 3) or NULL with n_grey == 0 */
    const uint8_t* nongrey;                                    /* (n_nongrey, Ht, Wt, 3) or NULL with n_nongrey == 0 */
    float* out;                                                /* (B, Ht, Wt, 3) */
    int is_grey[HPS_FRONTEND_MAX_IMAGES];
    int idx[HPS_FRONTEND_MAX_IMAGES];
} hps_texture_gather_args;
int hps_sizeof_texture_gather_args(void);
int hps_texture_gather(const hps_texture_gather_args* args /* HOST */, hps_stream_t stream);

/* hps_resize_bilinear_u8  (on_the_fly_smpl_train_dataset.py:88-94, pw3d_eval_dataset.py:45-46: cv2.resize(..., INTER_LINEAR) of a
 * uint8 image, transposed, / 255)
 * out (B, 3, out_h, out_w) float32 = level / 255.0f from (H, W, 3) uint8 sources of different sizes.  `level` is cv2.resize's uint8
 * result: per axis f = float((d + 0.5) src / dst - 0.5) (the product in float64), s = floor(f), f -= s; horizontally s < 0 -> (0, f = 0)
 * and s >= W - 1 -> (W - 1, f = 0), vertically the two ROWS are clamped and f is kept; coefficients rint((1 - f) 2048), rint(f 2048);
 * rows h = S[x0] a0 + S[x1] a1, then level = (((b0 (h0 >> 4)) >> 16) + ((b1 (h1 >> 4)) >> 16) + 2) >> 2.  (At exactly half size OpenCV
 * switches to INTER_AREA, (a + b + c + d + 2) >> 2: the formula above gives the same level there.) */
typedef struct hps_u8_image {
    const uint8_t* src;                                        /* (H, W, 3) */
    int H, W;
} hps_u8_image;
typedef struct hps_resize_bilinear_u8_args {
    int struct_bytes;
    int B;
    int out_w, out_h;
    float* out;                                                /* (B, 3, out_h, out_w) */
    hps_u8_image image[HPS_FRONTEND_MAX_IMAGES];
} hps_resize_bilinear_u8_args;
int hps_sizeof_resize_bilinear_u8_args(void);
int hps_resize_bilinear_u8(const hps_resize_bilinear_u8_args* args /* HOST */, hps_stream_t stream);

/* hps_eval_crop_u8  (ssp3d_eval_dataset.py:49-61, :74-80 through image_utils.py:145-229 with bbox_whs, no augmentation)
 * Per image the float32 matrix of image_utils.py:190-194 -- box side times scale_factor, out_wh / box, out_wh / 2 - (out_wh / box)
 * centre, formed in float64 as NumPy does with float64 labels and rounded to float32 on assignment -- then cv2.warpAffine's fixed-point
 * route (csrc/cv_warp.h), constant border 0:
 *   rgb   (B, 3, out_wh, out_wh) float32 = level / 255.0f, INTER_LINEAR on the uint8 image: weights (32 - fy)(32 - fx), ... in 1024ths
 *         (OpenCV's 15-bit table holds exactly 32 times these), level = (sum + 512) >> 10, a tap outside the image reads 0;
 *   seg   (B, out_wh, out_wh) float32 = the uint8 level itself, INTER_NEAREST (NULL, or an image without seg: not written / zero);
 *   joints    (B, K, 2) float64 = the matrix applied in float64 to columns 0, 1 of keypoints (B, K, 3) float64 (:212-214);
 *   positions (B, K, 2) int32   = joints truncated toward zero (astype(np.int16), :62), held to [-32768, 32767].
 * keypoints, joints and positions come together or are all NULL. */
typedef struct hps_eval_crop_image {
    const uint8_t* rgb;                                        /* (H, W, 3) */
    const uint8_t* seg;                                        /* (H, W) or NULL */
    int H, W;
    double centre_v, centre_h, side;                           /* bbox_centres[i] = (vertical, horizontal), bbox_whs[i] */
} hps_eval_crop_image;
typedef struct hps_eval_crop_u8_args {
    int struct_bytes;
    int B, out_wh, K;
    double scale_factor;
    const double* keypoints;                                   /* DEVICE (B, K, 3) or NULL */
    float* rgb;
    float* seg;                                                /* or NULL */
    double* joints;                                            /* or NULL */
    int32_t* positions;                                        /* or NULL */
    hps_eval_crop_image image[HPS_FRONTEND_MAX_IMAGES];
} hps_eval_crop_u8_args;
int hps_sizeof_eval_crop_u8_args(void);
int hps_eval_crop_u8(const hps_eval_crop_u8_args* args /* HOST */, hps_stream_t stream);

/* pw3d_eval_dataset.py:48-53: joints (n, 2) float64 = columns 0, 1 of keypoints (n, 3) times scale (n_images, 2) (img_wh / width,
 * img_wh / height; K rows per image), positions (n, 2) int32 = joints rounded half to even (.round()) and held to [-32768, 32767]. */
int hps_keypoints_scale_round(const double* keypoints, const double* scale, double* joints, int32_t* positions, int B, int K,
                              hps_stream_t stream);

/* ssp3d_eval_dataset.py:62-68 / pw3d_eval_dataset.py:53-60 with label_conversions.py:94-101: out (B, K, wh, wh) float32 =
 * exp(-((x - u) / std)^2 / 2 - ((y - v) / std)^2 / 2) in float32 for the INTEGER positions (B, K, 2) = (u, v), times the visibility
 * flag: use_threshold != 0 zeroes joint k where column 2 of keypoints (B, K, 3) float64 is not > threshold, unless bit k of
 * always_visible is set.  K <= 32. */
typedef struct hps_eval_heatmaps_args {
    int struct_bytes;
    int B, K, wh, use_threshold;
    float std;
    uint32_t always_visible;
    double threshold;
    const int32_t* positions;
    const double* keypoints;                                   /* read only with use_threshold != 0 */
    float* out;
} hps_eval_heatmaps_args;
int hps_sizeof_eval_heatmaps_args(void);
int hps_eval_heatmaps(const hps_eval_heatmaps_args* args /* HOST */, hps_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Person detector: the box path of Mask R-CNN (ResNet-50-FPN)  (csrc/detector.hip; run_predict.py:43, predict/predict_hrnet.py:52-57)
 * ---------------------------------------------------------------------------------------- */

/* The detection-specific launches of detection.MaskRCNNBoxDetector; the convolutions and FC layers are hps_conv2d_bn_act_pad /
 * hps_conv3x3_winograd (backbone), hps_conv2d_bn_act_c16 (FPN, RPN head, box head) and hps_hrnet_fuse (FPN's top-down sum).  The
 * semantics restate torchvision 0.7.0's detection code as we understand it; they have NOT been run against torchvision.  fp32, no
 * atomics, nothing allocated, no host synchronisation: capacities are the caller's, an ABSENT row is marked by a score of -infinity
 * (its box is zero) and is skipped by every later launch.  Per-image sizes go by value (HOST structs), at most HPS_DET_MAX_IMAGES
 * images per launch.  An image's values depend on its own descriptor only: same bits alone and in a batch. */
#define HPS_DET_MAX_IMAGES 64
#define HPS_DET_MAX_ANCHORS 8
#define HPS_DET_MAX_LEVELS 4
#define HPS_DET_NMS_MAX_BOXES 2048

/* hps_det_transform  (GeneralizedRCNNTransform: normalise, resize, batch): image b, (3, H, W) float32 CHW, -> the interior of the
 * stem's zero-haloed NHWC frame y (B, FH + 2 P, FW + 2 P, 4): channels (x - mean[c]) / std[c] resampled bilinearly (align_corners =
 * False) to (oh, ow) at the frame's top-left corner, channel 3 and every interior pixel outside (oh, ow) zero, one 16-byte store per
 * pixel.  Source coordinate of output row i: max((i + 1/2) (H / oh) - 1/2, 0) with the quotient in fp32, y0 = min(int(.), H - 1),
 * y1 = min(y0 + 1, H - 1), l = coordinate - y0; value (1 - ly) ((1 - lx) a + lx b) + ly ((1 - lx) c + lx d).  oh <= FH, ow <= FW. */
typedef struct hps_det_image {
    const float* src;                                          /* (3, H, W) */
    int H, W, oh, ow;
} hps_det_image;
typedef struct hps_det_transform_args {
    int struct_bytes;
    int B, FH, FW, P;
    float mean[3], std[3];
    float* y;
    hps_det_image image[HPS_DET_MAX_IMAGES];
} hps_det_transform_args;
int hps_sizeof_det_transform_args(void);
int hps_det_transform(const hps_det_transform_args* args /* HOST */, hps_stream_t stream);

/* LastLevelMaxPool (a max pool with kernel 1 and stride 2): y's interior (B, (H + 1) / 2, (W + 1) / 2, C) = x's interior at (2 i, 2 j);
 * frames with ipad / opad halos, C % 4 == 0. */
int hps_det_subsample2(const float* x, float* y, int B, int H, int W, int C, int ipad, int opad, hps_stream_t stream);

/* hps_det_rpn_decode  (AnchorGenerator, BoxCoder.decode with weights (1, 1, 1, 1), clip_boxes_to_image, remove_small_boxes) for one
 * level's k candidates per image: index (B, k) int64 into the level's (h, w, A) logits in the frame's own order, logits (B, k) their
 * values.  Candidate j: a = index % A, x = (index / A) % w, y = index / (A w); anchor = base[a] + (x stride_w, y stride_h, x stride_w,
 * y stride_h); deltas (B, h, w, 4 A) at channel 4 a + (dx, dy, dw, dh), dw and dh held to <= log(1000 / 16);
 * cx = dx w + ctr_x, pw = exp(dw) w, box = cx -+ pw / 2 (likewise y), clipped to [0, rw] x [0, rh] of ITS image's resized size.
 * Row out_offset + j of boxes (B, n_out, 4) / scores (B, n_out): the box and its logit, or zeros and -infinity when the clipped box
 * is narrower or lower than min_size or the index is out of range. */
typedef struct hps_det_rpn_decode_args {
    int struct_bytes;
    int B, h, w, A, k, n_out, out_offset;
    float stride_h, stride_w, min_size;
    float base[HPS_DET_MAX_ANCHORS][4];
    const float* deltas;
    const int64_t* index;
    const float* logits;
    float* boxes;
    float* scores;
    int size[HPS_DET_MAX_IMAGES][2];                           /* resized (h, w) per image */
} hps_det_rpn_decode_args;
int hps_sizeof_det_rpn_decode_args(void);
int hps_det_rpn_decode(const hps_det_rpn_decode_args* args /* HOST */, hps_stream_t stream);

/* hps_det_nms: greedy non-maximum suppression inside each of G independent groups (one category of one image: an FPN level for the
 * proposals, a class for the detections -- the categories are never mixed, no coordinate offsets).  Position i of group g is box
 * boxes[g, order[g, i]] (order NULL: i itself) with score scores[g, i]; the caller has sorted the positions by descending score
 * (absent ones, -infinity, may sit anywhere).  Walking i upwards, a present position that is still alive is kept and removes every
 * later alive position t with inter / (area_i + area_t - inter) > thresh, inter = max(min(x2) - max(x1), 0) max(min(y2) - max(y1), 0),
 * area = (x2 - x1) (y2 - y1), all fp32 (0 / 0 is not greater: kept).  keep_scores (G, N) = the score where kept, else -infinity.
 * One workgroup per group, the group's boxes in LDS: N <= HPS_DET_NMS_MAX_BOXES. */
typedef struct hps_det_nms_args {
    int struct_bytes;
    int G, N;
    float thresh;
    const float* boxes;                                        /* (G, N, 4) */
    const int64_t* order;                                      /* (G, N) or NULL */
    const float* scores;                                       /* (G, N) */
    float* keep_scores;                                        /* (G, N) */
} hps_det_nms_args;
int hps_sizeof_det_nms_args(void);
int hps_det_nms(const hps_det_nms_args* args /* HOST */, hps_stream_t stream);

/* hps_det_roi_align  (MultiScaleRoIAlign: LevelMapper(k_min 2, canonical scale 224, canonical level 4, eps 1e-6) and roi_align with a
 * bins x bins output, sampling_ratio 2, aligned = False): box r of image b, boxes (B, R, 4) in resized-image pixels, present where
 * scores (B, R) > -infinity, reads level clamp(floor(4 + log2(sqrt(area) / 224 + 1e-6)), 2, 1 + n_levels) - 2 of image b's zero-haloed
 * NHWC frames level[.].x (B, h + 2 pad, w + 2 pad, C).  start = x1 scale, roi_w = max(x2 scale - x1 scale, 1), bin = roi_w / bins,
 * samples at start + p bin + (i + 1/2) bin / 2, i = 0, 1 (likewise y); a sample with y < -1, y > h, x < -1 or x > w is 0, else it is held
 * to >= 0, low = int(.), and low >= h - 1 reads row h - 1 twice with fraction 0; the bin is the mean of its four samples, each
 * (1-ly)(1-lx) v1 + (1-ly) lx v2 + ly (1-lx) v3 + ly lx v4.  y (B, R, bins, bins, C): channel fastest (the order the box head's first
 * layer is permuted to); an absent box writes zeros.  C % 4 == 0 not required. */
typedef struct hps_det_level {
    const float* x;
    int h, w, pad;
    float scale;
} hps_det_level;
typedef struct hps_det_roi_align_args {
    int struct_bytes;
    int B, R, C, bins, n_levels;
    hps_det_level level[HPS_DET_MAX_LEVELS];
    const float* boxes;
    const float* scores;
    float* y;
} hps_det_roi_align_args;
int hps_sizeof_det_roi_align_args(void);
int hps_det_roi_align(const hps_det_roi_align_args* args /* HOST */, hps_stream_t stream);
/* The same launch into a haloed frame per box: y (B, R, bins + 2 halo, bins + 2 halo, C), the bins x bins values in the interior (the
 * same bits as hps_det_roi_align's) and the border written as zeros; an absent box writes a whole frame of zeros.  0 <= halo <= 8;
 * halo 0 is hps_det_roi_align.  (B R, bins + 2, bins + 2, C) with halo 1 is the input frame of a 3x3 / pad 1 layer over B R maps. */
int hps_det_roi_align_halo(const hps_det_roi_align_args* args /* HOST */, int halo, hps_stream_t stream);

/* hps_det_box_decode  (RoIHeads.postprocess_detections up to the per-class NMS): logits (B, R, NC), deltas (B, R, 4 NC), proposals
 * (B, R, 4) present where prop_scores (B, R) > -infinity.  prob = exp(l_c - max) / sum_c' exp(l_c' - max) (sum in class order);
 * class c >= 1: BoxCoder.decode with weights (10, 10, 5, 5) (dx = d / 10, ..., dw = d / 5 held to <= log(1000 / 16)) from the proposal,
 * clipped to the image's resized size.  Row (b, c - 1, r) of boxes (B, NC - 1, R, 4) / scores (B, NC - 1, R): the box and prob where
 * the proposal is present, prob > score_thresh and the clipped box is at least min_size wide and high, else zeros and -infinity.
 * probs (B, R, NC), when not NULL, receives every probability. */
typedef struct hps_det_box_decode_args {
    int struct_bytes;
    int B, R, NC;
    float score_thresh, min_size;
    const float* logits;
    const float* deltas;
    const float* proposals;
    const float* prop_scores;
    float* boxes;
    float* scores;
    float* probs;                                              /* or NULL */
    int size[HPS_DET_MAX_IMAGES][2];                           /* resized (h, w) per image */
} hps_det_box_decode_args;
int hps_sizeof_det_box_decode_args(void);
int hps_det_box_decode(const hps_det_box_decode_args* args /* HOST */, hps_stream_t stream);

/* hps_det_gather: the D best detections of each image after the per-class NMS.  top_scores / top_index (B, D): a descending top-k of
 * the kept scores over (NC - 1, R) sorted positions; position (c - 1, p) is proposal r = order[b, c - 1, p].  Row d of out_boxes
 * (B, D, 4): boxes[b, c - 1, r] with x times float(ow) / float(rw) and y times float(oh) / float(rh) (back to the input image's
 * pixels); out_labels (B, D) int64 = c; out_scores (B, D); absent rows (-infinity) are zeros with label 0 and score 0.
 * counts (B) int32 = the number of present rows (they come first). */
typedef struct hps_det_gather_args {
    int struct_bytes;
    int B, D, R, NC;
    const float* top_scores;
    const int64_t* top_index;
    const int64_t* order;                                      /* (B, NC - 1, R) */
    const float* boxes;                                        /* (B, NC - 1, R, 4) */
    float* out_boxes;
    int64_t* out_labels;
    float* out_scores;
    int32_t* counts;
    int size[HPS_DET_MAX_IMAGES][4];                           /* resized (h, w), original (h, w) per image */
} hps_det_gather_args;
int hps_sizeof_det_gather_args(void);
int hps_det_gather(const hps_det_gather_args* args /* HOST */, hps_stream_t stream);

/* The mask branch (csrc/detector_mask.hip; RoIHeads' mask path, MaskRCNNPredictor, maskrcnn_inference, paste_masks_in_image -- the same
 * caveat: a restatement that has not been run against torchvision).  Its RoIAlign is hps_det_roi_align_halo with 14 bins and halo 1,
 * its four 3x3 layers run on hps_conv2d_bn_act_pad. */
#define HPS_DET_MASK_BINS 14                                   /* the mask head's map: 14 x 14 */
#define HPS_DET_MASK_CHANNELS 256
#define HPS_DET_MASK_SIZE 28                                   /* the predicted mask: 28 x 28 */

/* hps_det_mask_predict  (ConvTranspose2d(256, 256, 2, 2) + ReLU, the 1x1 logit of the detection's own class, sigmoid) in one launch on
 * the fp32 matrix instructions.  x: K zero-haloed NHWC frames (K, 16, 16, 256), the interior (halo 1) is read.  Detection k with label
 * c = labels[k], 1 <= c < NC, present where scores is NULL or scores[k] > -infinity:
 *   t[co, 2 y + dy, 2 x + dx] = max(bd[co] + sum_ci x[k, y, x, ci] Wd[ci, co, dy, dx], 0),
 *   logits[k, i, j] = bl[c] + sum_co wl[c, co] t[co, i, j],        probs[k, i, j] = 1 / (1 + exp(-logits[k, i, j])).
 * The sum over ci is one fp32 multiply-add chain in ascending ci from 0 (v_mfma_f32_32x32x2_f32); the sum over co: with co = 32 t + 8 q
 * + 4 h + e, a chain of fused multiply-adds over (q, e) ascending from 0 for each (t, h), those added over t ascending from 0, then
 * h = 0 plus h = 1, then bl[c].  No atomics; a detection's bits depend on its own frame, label and the weights only.  The (K, 28, 28,
 * 256) tensor is never written and no other class's logit is formed.  An absent detection and one with a label outside [1, NC) write
 * zeros to probs and logits.  probs / logits (K, 28, 28); logits may be NULL.
 * wd: Wd in the kernel-side form (4, 128, 64, 8): element [2 dy + dx][s][64-lane l][t] = Wd[2 s + (l >> 5)][32 t + (l & 31)][dy][dx]
 * (16-byte aligned).  bd (256), wl (NC, 256) row-major, bl (NC), labels (K) int64. */
typedef struct hps_det_mask_predict_args {
    int struct_bytes;
    int K, NC;
    const float* x;
    const float* wd;
    const float* bd;
    const float* wl;
    const float* bl;
    const int64_t* labels;
    const float* scores;                                       /* (K) or NULL */
    float* probs;
    float* logits;                                             /* or NULL */
} hps_det_mask_predict_args;
int hps_sizeof_det_mask_predict_args(void);
int hps_det_mask_predict(const hps_det_mask_predict_args* args /* HOST */, hps_stream_t stream);

/* hps_det_paste_masks  (paste_masks_in_image with padding 1) for the n masks of ONE image: probs (n, 28, 28), boxes (n, 4) x1 y1 x2 y2
 * in the image's pixels -> out (n, H, W); every element is written (16-byte stores; out 16-byte aligned), no memset is needed.
 * Mask k gets a ring of zeros (30 x 30, m[i][j], i, j in [0, 30)).  Its box, every operation rounded once in fp32 (no fused
 * multiply-add):  w_half = (x2 - x1) 0.5,  x_c = (x2 + x1) 0.5,  w_half = w_half float(30 / 28),  ex0 = x_c - w_half,
 * ex1 = x_c + w_half (likewise y);  X0 = int(ex0), X1 = int(ex1) toward zero (values beyond +-2^29 held there),
 * w = max(X1 - X0 + 1, 1), h likewise.  Pixel (y, x) with max(X0, 0) <= x < min(X1 + 1, W) and max(Y0, 0) <= y < min(Y1 + 1, H):
 *   fx = max((x - X0 + 1/2) (30 / w) - 1/2, 0) with the quotient in fp32, j0 = min(int(fx), 29), j1 = min(j0 + 1, 29), lx = fx - j0
 *   (likewise fy, i0, i1, ly);  value = (1 - ly) ((1 - lx) m[i0][j0] + lx m[i0][j1]) + ly ((1 - lx) m[i1][j0] + lx m[i1][j1]);
 * every other pixel 0.  binary 0: out is float32, the value (a probability; torchvision does not threshold).  binary 1: out is uint8,
 * 1 where value > threshold else 0, 0 < threshold < 1. */
typedef struct hps_det_paste_masks_args {
    int struct_bytes;
    int n, H, W, binary;
    float threshold;
    const float* probs;
    const float* boxes;
    void* out;
} hps_det_paste_masks_args;
int hps_sizeof_det_paste_masks_args(void);
int hps_det_paste_masks(const hps_det_paste_masks_args* args /* HOST */, hps_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* HPS_H_ */
