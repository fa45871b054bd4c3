/* se3tracknet.h -- C ABI of the MI355X (gfx950) se(3)-TrackNet per-frame inference hot path.
 *
 * The reference (wenbowen123/iros20-6d-pose-tracking) has no FFI: its boundary is the Python
 * class predict.py:127 `Tracker` plus three file formats.  Every entry point below replaces one
 * reference call site on the path `Tracker.on_track` (predict.py:217-296); the Python mirror in
 * iros20-6d-pose-tracking_amd/ binds them with ctypes.
 *
 * Conventions
 *   - plain C types only; device pointers are caller-owned (e.g. torch tensors' data_ptr());
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - every se3tn_* compute call (preprocess, crop_raw, infer, render, render_frame, fill_depth, fit_stats, color_stats, color_stats_scene, scene_stats) is stream-ordered and
 *     asynchronous: no hipMalloc, no hipDeviceSynchronize, no host<->device copy of results => hipGraph-capturable.
 *     All device memory is allocated by the init-time calls: se3tn_create (activations, 176x176 z-buffer),
 *     se3tn_upload_weights / se3tn_bind_weights / se3tn_set_winograd (Winograd planes), se3tn_set_precision (f16x3 split
 *     panels), se3tn_mesh_create / _set_texture, and se3tn_reserve (full-frame z-buffer + fill_depth scratch).  The two
 *     full-frame calls grow their scratch on a first un-reserved call with a larger frame (draining the device first);
 *     inside a stream capture they refuse with SE3TN_E_STATE instead -- call se3tn_reserve at start-up;
 *   - return value: 0 = ok, >0 = a hipError_t, <0 = SE3TN_E_*; se3tn_last_error() has the text;
 *   - one context per (process, device); a context is thread-compatible, not thread-safe, and its compute calls share one set of
 *     activation workspaces: issue them on ONE stream, or order the streams yourself (events / synchronisation) -- two se3tn_infer of
 *     the same context in flight on two streams corrupt each other.  Throughput over several streams = one context per stream on a
 *     shared weight blob (se3tn_bind_weights; the Python mirror's PipelinedEngine).
 */
#ifndef SE3TRACKNET_H
#define SE3TRACKNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SE3TN_OK 0
#define SE3TN_E_ARG (-1)      /* bad argument (NULL, n > max_batch, ...)            */
#define SE3TN_E_STATE (-2)    /* call order (weights not bound, ...)                */
#define SE3TN_E_SHAPE (-3)    /* tensor shape does not match Se3TrackNet.state_dict */
#define SE3TN_E_KEY (-4)      /* unknown / missing state_dict key                   */
#define SE3TN_E_DEVICE (-5)   /* not a gfx950 device                                */

#define SE3TN_RES 176         /* dataset_info.yml `resolution` (predict.py:130)     */

/* input tensor layouts accepted by se3tn_infer */
#define SE3TN_NCHW 0 /* float32 [N,4,176,176], channels R,G,B,D: the reference operator
                        boundary `self.model(dataA, dataB)` predict.py:270-271            */
#define SE3TN_NHWC 1 /* float32 [N,176,176,4]: what se3tn_preprocess writes               */

typedef struct se3tn_ctx se3tn_ctx;

const char* se3tn_version(void);
const char* se3tn_last_error(void);

/* ---- life cycle ------------------------------------------------------------------------- */
/* Replaces `Se3TrackNet(image_size).cuda().eval()` (predict.py:155-158): selects `device`,
 * checks it is gfx950, allocates the activation workspace for up to `max_batch` pairs.
 * 1 <= max_batch <= SE3TN_MAX_BATCH_LIMIT, else SE3TN_E_ARG before anything is allocated.  The limit is where a 32-bit BYTE offset
 * from the base of a whole activation tensor would pass 2^31: the stride-2 gather kernel's DMA offsets into the 46 x 46 x 128 trunk
 * map (1,083,392 bytes per pair; conv3x3_gather_s2_kernel) are formed in `int`; every other per-batch index of the network kernels is
 * either 64-bit or reaches 2^31 later ("The largest batch").  Derived by reading the kernels -- tests/test_largest_batch_plan.py
 * restates every 32-bit expression that grows with the batch and evaluates it at every size up to here -- and run:
 * tests/test_gpu_largest_batch.py holds every pair of calls of 541 .. 1982 pairs to float64 (where `stem` passes 2^31 and 2^32 bytes, the
 * F(4x4) planes 2^31, and at the limit itself) in six configurations on contexts of max_batch 1982.  Nothing was found. */
#define SE3TN_MAX_BATCH_LIMIT 1982
int se3tn_create(int device, int max_batch, se3tn_ctx** out);
void se3tn_destroy(se3tn_ctx* ctx);
int se3tn_max_batch(const se3tn_ctx* ctx);
/* Start-up reservation of everything the stream-ordered calls would otherwise have to allocate on first use: the
 * z-buffer of se3tn_render_frame and the scratch images of se3tn_fill_depth for camera frames of up to H x W pixels
 * (Tracker.__init__ knows them from dataset_info['camera'], predict.py:147-148), and, if weights are bound, the Winograd
 * planes / f16x3 split panels of the modes currently selected.  Synchronises the device when it has to re-allocate. */
int se3tn_reserve(se3tn_ctx* ctx, int H, int W);

/* ---- weights: `model.load_state_dict(checkpoint['state_dict'])` (predict.py:151-156) ------ */
/* Hand over one float32 entry of Se3TrackNet.state_dict() (host memory, contiguous, the key and
 * shape exactly as torch saved them; int64 `num_batches_tracked` entries are not passed). */
int se3tn_set_tensor(se3tn_ctx* ctx, const char* key, const float* host_data,
                     const int64_t* shape, int ndim);
/* After all 106 tensors: fold BatchNorm (eval mode, eps=1e-5, float64 math) into the
 * convolutions and pack into the device layout (host side).  Fails with SE3TN_E_KEY if a
 * tensor is missing. */
int se3tn_pack_weights(se3tn_ctx* ctx);
size_t se3tn_packed_bytes(const se3tn_ctx* ctx);     /* size of the packed blob          */
const void* se3tn_packed_host(const se3tn_ctx* ctx); /* host pointer, valid after pack   */
/* Single-GPU: library-owned device copy of the packed blob. */
int se3tn_upload_weights(se3tn_ctx* ctx, void* stream);
/* Multi-GPU: use a caller-owned device blob in packed format (rank 0 packs, RCCL broadcasts
 * the bytes, every rank binds its copy).  The blob must outlive the context.  The blob holds the BN-folded float32
 * panels only (54 MB); the Winograd planes and the f16x3 split panels are derived from it on each rank's device. */
int se3tn_bind_weights(se3tn_ctx* ctx, const void* device_blob, size_t bytes);

/* ---- per-dataset constants --------------------------------------------------------------- */
/* mean.npy / std.npy: float64[8] = A(R,G,B,D), B(R,G,B,D) (predict.py:657-658). */
int se3tn_set_normalization(se3tn_ctx* ctx, const double mean[8], const double std[8]);
/* Arithmetic of the convolutions:
 *   SE3TN_PREC_F32   (default) exact float32 MFMA everywhere;
 *   SE3TN_PREC_F16X3 operands split into f16 hi + f16 lo (22 significant bits), products formed as
 *                    hi*hi + hi*lo + lo*hi on the f16 matrix cores with float32 accumulation:
 *                    float32-class error (measured ~1e-6 on the outputs) at 16/3 the MFMA rate.
 *                    Range: every value STORED in this mode -- the network inputs, the pooled stems, every activation between
 *                    two convolutions, and where the heads run as the fused F(4x4) block (se3tn_set_winograd, n >= min_batch)
 *                    the F(4x4) input planes B^T d B of the heads' stride-2 map and of the map between their two convolutions
 *                    -- must satisfy |x| <= 65000.  A store that does not raises a per-context flag; se3tn_overflow reports
 *                    and clears it (it outlives later calls and precision switches until read, and a replayed graph raises
 *                    it too) -- rerun in SE3TN_PREC_F32 then.  Inf and NaN count as violations.
 *                    What that means per route (measured against float64, tests/test_gpu_f16x3_range.py, seed 31):
 *                      high side, heads conv by conv: maps up to 65000 (a map with maximum 4.3e4: no flag, |d logit| 4e-7);
 *                      high side, fused F(4x4) heads: the planes run above the map (up to 49 x: the rows of B^T have absolute
 *                        sums up to 7; 10.3 x on that network), so the flag already rises for a map maximum between 5.4e3
 *                        (planes 5.6e4, no flag) and 1.1e4 (planes 1.1e5, flag): conservative, never silent;
 *                      low side, both routes: only the weights are scaled per row, so the lo half of a small activation falls
 *                        into f16 subnormals (2^-24 absolute) and NO flag is raised.  With a whole stored map scaled down (its
 *                        reader's weights up), |d logit| is float32-class (<= 1e-6, PREC_F32: 4e-7) down to a map maximum of
 *                        4e-2, 1e-5 at 2e-3, 3e-4 at 1.5e-4 and 5e-3 at 1e-5.  A network whose stored maps peak below ~1e-2
 *                        (a small BN gamma ahead of large weights) belongs in SE3TN_PREC_F32. */
#define SE3TN_PREC_F32 0
#define SE3TN_PREC_F16X3 1
/* Init-time call: the first selection of SE3TN_PREC_F16X3 (and a later change of weights while it is selected) derives the
 * split-f16 panels + per-cout power-of-two scales from the bound blob on the device (54 MB, allocated once). */
int se3tn_set_precision(se3tn_ctx* ctx, int mode);
int se3tn_overflow(se3tn_ctx* ctx, int* flag); /* synchronises */
/* Test hooks for that derivation: the device copy (NULL until derived) and its size, and the host statement of the same
 * arithmetic applied to a packed blob in host memory (se3tn_packed_host) -- the two must agree bit for bit. */
size_t se3tn_split_weights_bytes(const se3tn_ctx* ctx);
const void* se3tn_split_weights_device(const se3tn_ctx* ctx);
int se3tn_split_weights_host(const void* packed_blob_host, size_t blob_bytes, void* out_split, size_t out_bytes);
/* Algorithm of the stride-1 256/512-channel convolutions (AB2.*, trans|rot conv2.*) in
 * SE3TN_PREC_F32: batches of n >= min_batch pairs run them as Winograd F(tile x tile, 3x3), tile = 2 | 4 | 6 | 6_4 | AUTO
 * (0 keeps the current tile) -- float32 MFMA GEMMs on (tile+2)^2 transformed planes, 2.25x / 4x / 5.06x fewer
 * multiplies per output; smaller batches and min_batch = 0 use the direct implicit-GEMM kernels.
 * All are float32 arithmetic and differ by rounding only (rms error of one layer relative to its
 * largest activation: direct 5e-8, tile 2 1.8e-7, tile 4 7e-7, tile 6 1.8e-6; end to end the logits move by
 * 0.5 / 0.6 / 1.4e-6 against the direct kernels) -- the same freedom cuDNN takes under
 * torch.backends.cudnn.benchmark = True in the reference (predict.py:78).  Tile 4 runs a whole residual block as one
 * fused launch sequence (in-transform, GEMM, [out | in] mid transform through LDS, GEMM, out-transform | fused avg-pool + FC tail);
 * tile 6 (64 planes: at batch 64 exactly two 128 x 128 GEMM tiles per workgroup slot, 21 % fewer multiplies than tile 4) pays from
 * 14 pairs on.  Where the rounding goes (batched 30-degree closed loop, 64 tracks, every pair against the CPU oracle,
 * scripts/rounding_by_block.py): max |d logit| 4.9e-6 with tile 4 everywhere, 6.0e-6 with tile 6 on the 256-channel block only,
 * 1.3e-5 with tile 6 on the 512-channel heads as well -- the heads' products go straight into the average pool + FC.
 * SE3TN_WINOGRAD_TILE_6_4 = tile 6 for the 256-channel block, tile 4 for the heads.
 * SE3TN_WINOGRAD_TILE_AUTO (the default) picks tile 4 or 6 per block from the batch and, for the heads, from rot_normalizer
 * (se3tn_set_normalizers): the rotation logits' rounding reaches the composed pose multiplied by it.  The rule -- with every other choice
 * of kernel per conv -- is stated once, in csrc/infer_plan.h (tile_for, plan_infer); the constants below are its thresholds.
 * SE3TN_PREC_F16X3 has F(4x4) only and uses it whatever is selected. */
#define SE3TN_WINOGRAD_TILE_AUTO 46
#define SE3TN_WINOGRAD_TILE_6_4 64
#define SE3TN_WINOGRAD_TILE6_MIN_BATCH 14
#define SE3TN_WINOGRAD_HEADS_TILE6_MAX_ROT 0.2   /* radians (11.5 degrees) */
#define SE3TN_WINOGRAD_DEFAULT_MIN_BATCH 6
#define SE3TN_WINOGRAD_DEFAULT_TILE SE3TN_WINOGRAD_TILE_AUTO
int se3tn_set_winograd(se3tn_ctx* ctx, int min_batch, int tile);
int se3tn_get_winograd(const se3tn_ctx* ctx, int* min_batch, int* tile);
/* Algorithm of the 64-channel trunk (convA2 / convB2 / convB3, 44 x 44 maps) in SE3TN_PREC_F32: batches of n >= min_batch pairs MAY
 * run its four launches as a FUSED Winograd F(2x2, 3x3) kernel -- input transform, the 16 per-frequency products on the f32 matrix
 * cores and the output transform inside one workgroup per image quadrant, nothing spilled to memory; 2.25x fewer multiplies and
 * exactly 2 / 1 rounds of workgroups on the 256 CUs at batch 64.  A launch takes that kernel when its 4 n groups workgroups fill
 * rounds of the device's CUs to >= min_fill_percent (n >= 34; the grouped A|B launches from n = 18: measured crossovers,
 * scripts/trunk_sweep.sh, profiles/r03f_trunk_sweep.txt); otherwise, and always
 * with min_batch = 0, the direct implicit-GEMM kernels run.  Float32 arithmetic in a different association (rounding as tile 2
 * above: the logits move by < 1.1e-6). */
#define SE3TN_TRUNK_WINOGRAD_DEFAULT_MIN_BATCH 8
#define SE3TN_TRUNK_WINOGRAD_DEFAULT_MIN_FILL 55   /* percent of the last round of workgroups; 0 = every launch with n >= min_batch */
int se3tn_set_trunk_winograd(se3tn_ctx* ctx, int min_batch, int min_fill_percent);
int se3tn_get_trunk_winograd(const se3tn_ctx* ctx, int* min_batch, int* min_fill_percent);
/* Rounding of OffsetDepth's `depth -= pose[2,3]*1000` (data_augmentation.py:134-144: a float64 scalar subtracted from a float32 array):
 *   SE3TN_OFFSET_RULE_NUMPY1 (default) what every NumPy the reference can run on does (it pins Python 3.6 => NumPy <= 1.19,
 *                            docker/dockerfile:28; `np.float`, Utils.py:307, stops importing at 1.24): value-based casting, the
 *                            scalar becomes float32 and the subtraction is ONE float32 operation;
 *   SE3TN_OFFSET_RULE_NUMPY2 NEP 50 (NumPy >= 2, were the reference ported to it): float64 subtraction, rounded to float32 once.
 * The two differ by <= 1 ulp(f32) on the offset depth and only when z * 1000 is not a float32 (tests/golden/preprocess_numpy1.npz
 * was produced by the reference's own classes under NumPy 1.26.4, preprocess.npz under NumPy 2.2; the kernel matches each bit for bit). */
#define SE3TN_OFFSET_RULE_NUMPY1 0
#define SE3TN_OFFSET_RULE_NUMPY2 1
int se3tn_set_offset_rule(se3tn_ctx* ctx, int rule);
int se3tn_get_offset_rule(const se3tn_ctx* ctx);
/* trans_normalizer / rot_normalizer of Tracker.__init__ (predict.py:128). */
int se3tn_set_normalizers(se3tn_ctx* ctx, double trans_normalizer, double rot_normalizer);

/* ---- pre-processing: crop_bbox + OffsetDepth + NormalizeChannels + ToTensor --------------- */
/* One 176x176 crop (Utils.py:320-359, data_augmentation.py:124-189).  For the rendered image A
 * pass the 176x176 render itself with window (0,0,176,176). */
typedef struct se3tn_crop {
  const uint8_t* rgb;    /* device, [H,W,3] uint8 RGB                                     */
  const uint16_t* depth; /* device, [H,W] uint16 millimetres                              */
  int32_t H, W;          /* frame size                                                    */
  int32_t left, top, right, bottom; /* crop window = min/max of compute_bbox's (v,u) corners;
                                       may leave the frame (zero padding, Utils.py:330-342) */
  double z_offset_mm;    /* poseA[2,3]*1000 (data_augmentation.py:137-140; both A and B use
                            poseA, :130-131); sign handled as the reference does            */
  int32_t stats;         /* 0: mean[:4]/std[:4] (image A)   1: mean[4:]/std[4:] (image B)  */
  int32_t _pad;
} se3tn_crop;
/* `crops` is a HOST array of n descriptors (copied into kernel arguments, no sync);
 * out_nhwc: device float32 [n,176,176,4] -- or one of the context's own input buffers
 * (se3tn_input_buffer), which are stored zero-bordered and consumed in place by se3tn_infer. */
int se3tn_preprocess(se3tn_ctx* ctx, const se3tn_crop* crops, int n, float* out_nhwc,
                     void* stream);
/* crop_bbox (Utils.py:320-359) ALONE: the zero-padded crop + cv2.resize(..., INTER_NEAREST) of one window,
 * as raw images -- what Tracker.render_window returns for a full-frame renderer (predict.py:209-213) and
 * what a caller of Tracker.dataset.processData feeds it.  crop->z_offset_mm / stats are ignored.
 * Outputs (device): rgb uint8 [176,176,3], depth uint16 [176,176]. */
int se3tn_crop_raw(se3tn_ctx* ctx, const se3tn_crop* crop, uint8_t* rgb_out, uint16_t* depth_out, void* stream);
/* the context's own input buffers, which = 0 (A) / 1 (B).  Opaque layout ([max_batch,182,182,4],
 * 3-pixel zero border): only pass them to se3tn_preprocess (as out) and se3tn_infer (as A / B). */
float* se3tn_input_buffer(se3tn_ctx* ctx, int which);

/* ---- the network + pose update ------------------------------------------------------------ */
/* Replaces `self.model(dataA,dataB)` (predict.py:270-271 -> se3_tracknet.py:81-112) and, when
 * poseA/poseB are given, `TrackDataset.processPredict` (datasets.py:159-175) for each pair.
 *   A, B     device float32, layout per `layout`, n pairs (A or B may be the context's own
 *            input buffers)
 *   trans,rot device float32 [n,3] (tanh outputs, as prediction['trans'/'rot']); may be NULL
 *   poseA    device float64 [n,16] row-major 4x4 object-in-camera (metres); may be NULL
 *   poseB    device float64 [n,16]: t_B = trans*tn + t_A,  R_B = Rodrigues(rot*rn) . R_A     */
int se3tn_infer(se3tn_ctx* ctx, const float* A, const float* B, int n, int layout, float* trans,
                float* rot, const double* poseA, double* poseB, void* stream);
/* hipGraph replay of se3tn_infer (off by default).  When on, the second se3tn_infer with an argument
 * set (pointers, n, layout, modes) captures its launches on `stream` (which must not be the null stream)
 * and later calls replay the graph: for the launch-bound batch-1 tracking step.  The input / output /
 * pose buffers must therefore be persistent device buffers whose CONTENTS change between calls. */
int se3tn_enable_graphs(se3tn_ctx* ctx, int on);
/* output['feature'] (se3_tracknet.py:96): device float32 [n,256,22,22] NCHW, valid after infer */
int se3tn_get_feature(se3tn_ctx* ctx, int n, float* feature_nchw, void* stream);
/* pre-tanh FC outputs of the last se3tn_infer: device float32 [max_batch,6] (trans, rot) */
const float* se3tn_logits(se3tn_ctx* ctx);

/* ---- rendered image A: HIP rasteriser replacing the reference's OpenGL renderer ---------------- */
/* vispy_renderer.py:47-178 (VispyRenderer) as called by Tracker.render_window (predict.py:193-215).
 * Mesh = what the reference reads from the .ply: float32 vertices [V,3] (metres), unit vertex normals
 * [V,3], vertex colours [V,3] already divided by 255, int32 triangles [F,3] (host pointers, copied). */
typedef struct se3tn_mesh se3tn_mesh;
int se3tn_mesh_create(se3tn_ctx* ctx, const float* verts, const float* normals, const float* colors01, int V,
                      const int32_t* faces, int F, se3tn_mesh** out);
void se3tn_mesh_destroy(se3tn_mesh* mesh);
/* ob_in_cam: row-major 4x4 object pose in the OpenCV camera; K row-major 3x3; window = {left, top,
 * right, bottom} as render_window derives it from compute_bbox(..., scale=(1000,-1000,1000))
 * (predict.py:201-206: u range, and the range of the FLIPPED row coordinate cy - fy y/z).
 * Outputs (device): rgb uint8 [176,176,3], depth uint16 [176,176] millimetres, 0 = background. */
int se3tn_render(se3tn_ctx* ctx, se3tn_mesh* mesh, const double ob_in_cam[16], const double K[9],
                 const int32_t window[4], uint8_t* rgb, uint16_t* depth, void* stream);
/* Batches of 1-5 pairs -- the regime Tracker.on_track runs in -- take kernels of their own: the four 64 -> 64 trunk convs without a
 * K split or a reduction launch (conv64_small.hip) and the 128 .. 512-channel convs as one round of 128-pixel x 32-cout x
 * channel-slice workgroups with a layer-fixed slice count (conv_slices_small.hip), the stem + max-pool in one launch of
 * 16-pool-pixel tiles (stem_pool_small.hip), and a tail that adds the last conv's partial-sum slices itself (tail_parts_kernel).
 * float32, same tolerances, other summation orders than the kernels larger batches take.  Every kernel of the family works image by
 * image with a layer-fixed summation order: for every n <= 5 a pair has the same bits alone or in any batch (round 6; from 6 pairs the
 * algorithms change -- Winograd thresholds at 6 / 14 pairs -- and the last bits of a pair's result depend on the batch it travels in,
 * as in the reference under cuDNN's per-shape algorithm choice, predict.py:78).  on = 0 keeps every batch size on the general
 * kernels (default 1; SE3TN_SMALL_KERNELS=0 in the environment of se3tn_create does the same). */
int se3tn_set_small_kernels(se3tn_ctx* ctx, int on);
int se3tn_get_small_kernels(const se3tn_ctx* ctx);
/* Rasterisation rule.  OpenGL leaves sub-pixel precision, interpolation arithmetic and float -> unorm rounding to the
 * implementation; image A is defined here as what the reference's VispyRenderer produces on the conformant software GL the
 * goldens were rendered on (tests/golden/gl_swiftshader*.npz), reproduced byte for byte: window coordinates snapped to
 * 1 / 2^sub_bits pixel (4 = that implementation = the GL minimum GL_SUBPIXEL_BITS, default; 8 = what desktop GPUs report),
 * integer top-left coverage, that implementation's plane-equation arithmetic and 16-bit unorm conversion.  The depth read-back
 * (vispy_renderer.py:163-169) mixes a float32 array with float64 scalars: it follows se3tn_set_offset_rule's NumPy generation.
 * sub_bits = 8 has NO golden: no desktop GL is reachable from the build / test boxes, so that setting is the same arithmetic
 * with a finer snap and is pinned by nothing but the rule tests (oracle/pin_gl.py pins it on first contact with such a GL). */
int se3tn_set_raster_rule(se3tn_ctx* ctx, int sub_bits);
int se3tn_get_raster_rule(const se3tn_ctx* ctx);

/* The reference's second renderer, offscreen_renderer.py:48-83 (pyrender; dataset_info['renderer'] == 'pyrenderer',
 * predict.py:161-164, textured .obj models): a FULL W x H camera frame, ambient light only, depth = camera z.
 * se3tn_mesh_set_texture attaches the material: per-vertex texture coordinates uv [V,2] (OBJ convention, v up),
 * an RGB uint8 image [th,tw,3] (row 0 = top; NULL: the vertex colours are the base colour) and the mtl's Kd
 * (NULL: 1,1,1); host pointers, copied; the mip pyramid is built here.  se3tn_render_frame writes device
 * rgb uint8 [H,W,3] and depth uint16 [H,W] millimetres ((depth * 1000).astype(uint16), predict.py:211); feed
 * them to se3tn_preprocess / se3tn_crop_raw with the plain compute_bbox window exactly like a camera frame
 * (predict.py:209-213).  Z-buffer: se3tn_reserve(ctx, H, W) at start-up (else grown on the first call, see Conventions). */
int se3tn_mesh_set_texture(se3tn_mesh* mesh, const float* uv, const uint8_t* rgb, int tw, int th, const float kd[3]);
int se3tn_render_frame(se3tn_ctx* ctx, se3tn_mesh* mesh, const double ob_in_cam[16], const double K[9], int W, int H,
                       uint8_t* rgb, uint16_t* depth, void* stream);
/* The same render restricted to a rectangle of the frame: rect = {x0, y0, x1, y1}, columns [x0, x1) and rows [y0, y1) in OpenCV
 * image coordinates (row 0 = top).  The vertices go through the full W x H projection; the z-buffer, the coverage loops and the
 * shading cover the rectangle only.  rgb_sub uint8 [y1-y0, x1-x0, 3] and depth_sub uint16 [y1-y0, x1-x0] (device, tightly packed,
 * top-down) receive the sub-image: every byte equals the same pixel of se3tn_render_frame.  Stream-ordered and capturable like
 * se3tn_render_frame; the z-buffer holds (x1-x0) (y1-y0) keys: reserved by se3tn_reserve(ctx, H, W) for every rectangle of such a
 * frame, else grown on the first call (inside a stream capture: SE3TN_E_STATE).  SE3TN_E_ARG: an empty rectangle, one that is not
 * inside [0, W) x [0, H), H > 2048. */
int se3tn_render_frame_rect(se3tn_ctx* ctx, se3tn_mesh* mesh, const double ob_in_cam[16], const double K[9], int W, int H,
                            const int32_t rect[4], uint8_t* rgb_sub, uint16_t* depth_sub, void* stream);
/* Which renderer se3tn_on_track / se3tn_on_track_batch use for image A of this mesh:
 *   SE3TN_ROUTE_WINDOW (default, also for a mesh with a texture attached)  the VispyRenderer route: se3tn_render at the y-flipped window;
 *   SE3TN_ROUTE_FRAME   the pyrender route (predict.py:209-213): the full-frame render cropped with the plain compute_bbox window.
 * se3tn_mesh_get_route returns the route, or -1 for a NULL mesh. */
#define SE3TN_ROUTE_WINDOW 0
#define SE3TN_ROUTE_FRAME 1
int se3tn_mesh_set_route(se3tn_mesh* mesh, int route);
int se3tn_mesh_get_route(const se3tn_mesh* mesh);

/* ---- one frame of Tracker.on_track in ONE call -------------------------------------------------------- */
/* predict.py:217-296 for samples == 1, with the model mesh rendered by this library: compute_bbox (host float64) -> image A
 * (se3tn_render at the y-flipped window, :193-208) -> crop + normalise of image A and of the camera frame (ONE launch) -> network ->
 * pose update -> read-back.  rgb / depth are HOST pointers to the camera frame (uint8 [H,W,3] RGB, uint16 [H,W] millimetres):
 * only the rows / columns the crop window covers are staged (pinned) and uploaded, in one copy together with the pose.
 * rgbA_dev / depthA_dev: optional device buffers (uint8 [176,176,3], uint16 [176,176]) that receive image A (NULL: internal).
 * Outputs are host memory: pose_out = the 4x4 float64 estimate (row-major); trans_out / rot_out [3] (may be NULL) the network's
 * tanh outputs; bbox_vu [4][2] (may be NULL) compute_bbox's corners.  SYNCHRONOUS on `stream` (as predict.py:275-276 is); the first
 * call (or a larger frame) allocates the staging buffers.  Same arithmetic as se3tn_render + se3tn_preprocess x2 + se3tn_infer.
 * A mesh on SE3TN_ROUTE_FRAME (se3tn_mesh_set_route) takes predict.py:209-213 instead: compute_bbox -> rectangle = crop window
 * intersected with the frame (se3tn_frame_rect) -> se3tn_render_frame_rect of that rectangle at prev_pose -> image A (the sub-image
 * with the window shifted by the rectangle's origin) and the camera frame cropped in ONE launch -> network as above.  A window that
 * misses the frame gives an all-zero image A.  rgbA_dev / depthA_dev then receive the 176 x 176 crop_bbox of the render (what
 * se3tn_crop_raw gives on the full-frame render), written by the same launch.  Same arithmetic as se3tn_render_frame +
 * se3tn_preprocess x2 + se3tn_infer.  H > 2048 is refused on this route (as se3tn_render_frame does).  On this route the first call
 * (or a larger frame) also allocates a z-buffer and a sub-image for a WHOLE H x W frame (13 bytes per pixel, 4 MB at 480 x 640), so
 * that a moving window never re-allocates; they are the route's own, beside what se3tn_reserve holds for se3tn_render_frame
 * (se3tn_on_track_batch sizes the same buffers by pairs x the largest rectangle of the call instead). */
int se3tn_on_track(se3tn_ctx* ctx, se3tn_mesh* mesh, const double prev_pose[16], const double K[9], double object_width_mm,
                   const uint8_t* rgb, const uint16_t* depth, int H, int W, uint8_t* rgbA_dev, uint16_t* depthA_dev,
                   double pose_out[16], float trans_out[3], float rot_out[3], int32_t bbox_vu[8], void* stream);

/* ---- n tracks in ONE call ----------------------------------------------------------------------------- */
/* The loop body of predict.py:217-296 for n INDEPENDENT (pose, camera frame) pairs of the same object -- several sequences /
 * cameras / hypotheses advanced together (frames of one track are serial: this is where a batch comes from in deployment;
 * Tracker.on_track_batch).  Per pair exactly se3tn_on_track's arithmetic: compute_bbox (host float64), image A of all n poses in
 * FOUR rasteriser launches (grid.y = pose), the crop windows of the n frames staged through pinned memory in one copy, both crops of
 * every pair, the network on n pairs, the pose update.  prev_poses [n,16] row-major; rgb / depth: n HOST pointers to uint8 [H,W,3] /
 * uint16 [H,W] frames of one size (the same pointer may repeat).  rgbA_dev / depthA_dev: optional device buffers
 * [n,176,176,3] / [n,176,176] that receive the images A (NULL: internal).  Outputs (host): pose_out [n,16], trans_out / rot_out
 * [n,3] (may be NULL), bbox_vu [n,4,2] (may be NULL).  n <= max_batch of se3tn_create.  SYNCHRONOUS on `stream`; the first call
 * (a larger n, mesh or frame) allocates.  A mesh on SE3TN_ROUTE_FRAME: as se3tn_on_track describes, the n rectangles rendered in the
 * same FOUR launches (one mesh and texture pyramid, z-buffers and sub-images sized by the largest rectangle of the call). */
int se3tn_on_track_batch(se3tn_ctx* ctx, se3tn_mesh* mesh, int n, const double* prev_poses, const double K[9], double object_width_mm,
                         const uint8_t* const* rgb, const uint16_t* const* depth, int H, int W, uint8_t* rgbA_dev,
                         uint16_t* depthA_dev, double* pose_out, float* trans_out, float* rot_out, int32_t* bbox_vu, void* stream);

/* ---- n different objects in one camera frame, ONE call ------------------------------------------------------------ */
/* se(3)-TrackNet is trained per object (its own weights, mean / std and normalisers: one context each); a frame shows several objects.
 * se3tn_on_track_objects runs the loop body of se3tn_on_track for n objects of ONE camera frame (host rgb uint8 [H,W,3], depth uint16
 * [H,W] millimetres), each with its own model:
 *   objects[i].model  the context whose bound weights, se3tn_set_normalization mean / std and se3tn_set_normalizers tn / rn object i
 *                     uses (read only; no weights are copied).  A model may appear several times and `ctx` may be one of them;
 *   objects[i].mesh   EITHER every object a vertex-colour mesh on SE3TN_ROUTE_WINDOW (the VispyRenderer route, not textured), OR every
 *                     object a mesh on SE3TN_ROUTE_FRAME (the pyrender route) that se3tn_mesh_set_texture has given a material: a
 *                     texture, or a Kd over its vertex colours.  Textured and un-textured meshes, textures of different sizes and
 *                     meshes of different sizes share a call; the two routes do not (one rasteriser mode per launch);
 *   objects[i].object_width_mm, prev_poses [n,16] row-major.
 * `ctx` runs the call: its workspaces, staging, streams, offset rule and raster rule.  Image A of all n objects comes out of FOUR
 * rasteriser launches (grid.y = object, each instance with its own mesh), the frame's n crop windows go up in one copy, and the network
 * runs in chunks of at most 5 objects, ALWAYS through the batch 1-5 kernel family (whatever ctx's Winograd / trunk settings): every
 * kernel of that family works image by image, here with each image's own weights, so object i gets exactly the bits se3tn_on_track on
 * its own model context gives it while that context runs one pair through the same family (its default) -- whatever n, the chunking,
 * the order or the company.  A model context set to take another route at one pair (se3tn_set_winograd / se3tn_set_trunk_winograd
 * thresholds of 1, se3tn_set_small_kernels(0), SE3TN_PREC_F16X3, developer switches) gets other bits from se3tn_on_track, within
 * float32 tolerance.  Outputs (host) as se3tn_on_track_batch:
 * pose_out [n,16], trans_out / rot_out [n,3] and bbox_vu [n,4,2] (may be NULL); rgbA_dev / depthA_dev optional device [n,176,176,3] /
 * [n,176,176].  1 <= n <= se3tn_max_batch(ctx).  SYNCHRONOUS on `stream`, refused inside a stream capture; the first call (a larger n,
 * mesh or frame) allocates.
 * All objects on SE3TN_ROUTE_FRAME: per object exactly se3tn_on_track's arithmetic on that route -- compute_bbox, rectangle = crop
 * window intersected with the frame, all n rectangles rendered in the same FOUR launches (each instance with its own mesh and material
 * at its own pose; z-buffers and sub-images sized n x the largest rectangle of the call), a window that misses the frame = an empty
 * rectangle and an all-zero image A; image A (the sub-image under the window shifted by the rectangle's origin) and the camera frame
 * cropped with each model's own mean / std, then the network as above.  rgbA_dev / depthA_dev then receive the 176 x 176 crop_bbox of
 * every render (what se3tn_on_track writes there on this route), from the launch that crops.
 * SE3TN_E_ARG: n out of range, a NULL mesh, a textured mesh left on SE3TN_ROUTE_WINDOW, a mesh on SE3TN_ROUTE_FRAME that
 * se3tn_mesh_set_texture was never called on, a call that mixes SE3TN_ROUTE_WINDOW and SE3TN_ROUTE_FRAME objects, H > 2048 on
 * SE3TN_ROUTE_FRAME, a pose with z <= 0 or not finite.  SE3TN_E_STATE: a model without weights or
 * normalisation, on another device, with another packed size, offset rule or raster rule than ctx; ctx in SE3TN_PREC_F16X3, with the
 * small kernels off or with se3tn_keep_intermediates on.  The context stays usable after a refusal. */
typedef struct se3tn_object {
  const se3tn_ctx* model;   /* weights (bound blob), mean / std, trans / rot normalisers of this object */
  se3tn_mesh* mesh;         /* all objects of a call on one route: vertex-colour meshes (SE3TN_ROUTE_WINDOW) or meshes with a material (SE3TN_ROUTE_FRAME) */
  double object_width_mm;
} se3tn_object;
int se3tn_on_track_objects(se3tn_ctx* ctx, int n, const se3tn_object* objects, const double* prev_poses, const double K[9],
                           const uint8_t* rgb, const uint16_t* depth, int H, int W, uint8_t* rgbA_dev, uint16_t* depthA_dev,
                           double* pose_out, float* trans_out, float* rot_out, int32_t* bbox_vu, void* stream);

/* ---- live-camera front end: depth hole filling ---------------------------------------------------- */
/* Utils.py:455-514 `fill_depth` as predict_ros.py:38-41 applies it to every depth frame before on_track:
 *     depth = fill_depth(depth_mm / 1e3, max_depth, extrapolate, blur_type);  out_mm = (depth * 1000).astype(uint16)
 * depth_mm: device uint16 [H,W] millimetres; out_mm: device uint16 [H,W] and / or out_m: device float32 [H,W] metres
 * (either may be NULL).  blur: the reference's blur_type ('bilateral' is its default; anything else but 'gaussian'
 * skips the blur).  Scratch images: se3tn_reserve(ctx, H, W) at start-up (else grown on the first call, see Conventions).
 * A context's scratch is shared by its calls: use one stream per context for se3tn_fill_depth / se3tn_render*. */
#define SE3TN_BLUR_NONE 0
#define SE3TN_BLUR_BILATERAL 1
#define SE3TN_BLUR_GAUSSIAN 2
int se3tn_fill_depth(se3tn_ctx* ctx, const uint16_t* depth_mm, int H, int W, double max_depth_m, int extrapolate,
                     int blur, uint16_t* out_mm, float* out_m, void* stream);
/* se3tn_fill_depth restricted to a rectangle of the frame: rect = {x0, y0, x1, y1} as se3tn_render_frame_rect takes it.
 * out_mm_sub: device uint16 [y1-y0, x1-x0], every value the same pixel of se3tn_fill_depth's out_mm, bit for bit.
 * With extrapolate == 0 at most four stream operations: the chain up to the median of the whole frame as ONE tiled launch (the
 * bilateral table needs the range of the whole image), the table, blur + invert-back + uint16 of the rectangle only, one reset.
 * Stream-ordered, capturable after se3tn_reserve; SE3TN_E_ARG for an empty rectangle or one not inside the frame, a bad blur. */
int se3tn_fill_depth_rect(se3tn_ctx* ctx, const uint16_t* depth_mm_dev, int H, int W, double max_depth_m, int extrapolate, int blur,
                          const int32_t rect[4], uint16_t* out_mm_sub, void* stream);

/* se3tn_fill_depth_rect for n rectangles of ONE frame: rects HOST int32 [n,4] {x0, y0, x1, y1}, out_offsets HOST size_t [n] in uint16
 * elements from out_mm_base (device): rectangle i goes tightly packed, [y1-y0, x1-x0], to out_mm_base + out_offsets[i], every value the
 * same pixel of se3tn_fill_depth's out_mm, bit for bit -- whatever other rectangles the call holds, whether they overlap or repeat, and
 * in whatever order (the outputs must not overlap each other).  The chain up to the median, the range and the bilateral table run ONCE
 * for the frame; the last pass serves up to 64 rectangles per launch (the table travels as kernel arguments, read from the host
 * arrays during the call: stream-ordered, capturable after se3tn_reserve; SE3TN_E_STATE when the scratch would have to grow inside a
 * capture).  A rectangle with x1 <= x0 or y1 <= y0 is SKIPPED (what se3tn_frame_rect reports for a window that misses the frame); if
 * every rectangle is empty nothing is enqueued.  SE3TN_E_ARG: a rectangle that is not empty and not inside the frame, n < 1, a NULL
 * pointer, a bad blur. */
int se3tn_fill_depth_rects(se3tn_ctx* ctx, const uint16_t* depth_mm_dev, int H, int W, double max_depth_m, int extrapolate, int blur,
                           int n, const int32_t* rects /* host [n,4] */, const size_t* out_offsets /* host [n], uint16 elements */,
                           uint16_t* out_mm_base /* device */, void* stream);

#define SE3TN_COLOR_RGB 0
#define SE3TN_COLOR_BGR 1   /* what CvBridge 'bgr8' delivers (predict_ros.py:45-46) */
/* predict_ros.py:38-60 in ONE call: grab_depth's fill_depth + grab_color's channel order + Tracker.on_track.
 * se3tn_on_track with another staging step: color (HOST uint8 [H,W,3], channel order color_order) travels as the crop window's rows /
 * columns, swapped to RGB during that copy; depth_raw (HOST uint16 [H,W], the camera's millimetres with holes) goes up WHOLE on the
 * copy stream beside the rasteriser launches, and se3tn_fill_depth_rect of the window's part of the frame writes image B's depth where
 * the crop launch reads it -- the filled frame never visits the host.  depth_filled_dev (optional, device uint16 [H,W]): the whole
 * filled frame too (= se3tn_fill_depth's out_mm).  Everything else, the refusals included, as se3tn_on_track; synchronous on `stream`,
 * SE3TN_E_STATE inside a stream capture, SE3TN_E_ARG for a bad color_order / blur. */
int se3tn_on_track_live(se3tn_ctx* ctx, se3tn_mesh* mesh, const double prev_pose[16], const double K[9], double object_width_mm,
                        const uint8_t* color, int color_order, const uint16_t* depth_raw, int H, int W,
                        double max_depth_m, int extrapolate, int blur, uint16_t* depth_filled_dev /* optional, device [H,W] */,
                        uint8_t* rgbA_dev, uint16_t* depthA_dev, double pose_out[16], float trans_out[3], float rot_out[3],
                        int32_t bbox_vu[8], void* stream);

/* predict_ros.py:38-60 for n objects of ONE camera frame in ONE call: se3tn_on_track_objects with se3tn_on_track_live's staging.
 * color (HOST uint8 [H,W,3], channel order color_order) travels as every object's crop window, made RGB during that copy; depth_raw
 * (HOST uint16 [H,W], the camera's millimetres with holes) goes up WHOLE, ONCE, in the same copy.  The chain of se3tn_fill_depth up to
 * the median runs once for the frame whatever n, and se3tn_fill_depth_rects of the n windows' parts of the frame writes every object's
 * image-B depth where the crop launch reads it; an object whose window misses the frame has no rectangle and reads one zero pixel.
 * If every window misses and depth_filled_dev is NULL, the raw frame is not uploaded and no fill is enqueued.  depth_filled_dev
 * (optional, device uint16 [H,W]): the whole filled frame too (= se3tn_fill_depth's out_mm).
 * Object i gets exactly the bits se3tn_on_track_live on its own model context gives it (under the conditions se3tn_on_track_objects
 * states) -- equivalently the bits of se3tn_on_track_objects on se3tn_fill_depth's output with the colours already swapped --
 * whatever n, the order or the company.  Objects, routes (all SE3TN_ROUTE_WINDOW or all SE3TN_ROUTE_FRAME), outputs and every refusal
 * as se3tn_on_track_objects; SE3TN_E_ARG for a bad color_order / blur as se3tn_on_track_live.  SYNCHRONOUS on `stream`, SE3TN_E_STATE
 * inside a stream capture.  The context stays usable after a refusal. */
int se3tn_on_track_objects_live(se3tn_ctx* ctx, int n, const se3tn_object* objects, const double* prev_poses, const double K[9],
                                const uint8_t* color, int color_order, const uint16_t* depth_raw, int H, int W,
                                double max_depth_m, int extrapolate, int blur, uint16_t* depth_filled_dev /* optional, device [H,W] */,
                                uint8_t* rgbA_dev, uint16_t* depthA_dev, double* pose_out, float* trans_out, float* rot_out,
                                int32_t* bbox_vu, void* stream);

/* ---- how well a pose estimate fits the observed depth ------------------------------------------------------ */
/* The reference renders the model again at its estimate after every frame (predict.py:284, render_window(final_estimate)) and
 * pastes that render beside the observed crop for a person to look at (:285-290).  Headless, the same comparison is a record of
 * integers.  For a pair, m(p) / o(p) = model / observed depth in millimetres at pixel p of the 176 x 176 crop, both sampled
 * through a se3tn_crop descriptor with exactly se3tn_preprocess's / se3tn_crop_raw's index rule (resizeNN in float64, zero outside
 * the image); valid(d) = 100 < d < 2000, the network's own validity rule (data_augmentation.py:160-164, maskA = depthA > 100 of
 * predict.py:247).  seen_px == inlier_px + front_px + behind_px always. */
typedef struct se3tn_fit {       /* all uint32, 32 bytes */
  uint32_t model_px;    /* #{valid(m)}                                              */
  uint32_t seen_px;     /* #{valid(m) && valid(o)}                                  */
  uint32_t inlier_px;   /* #{seen && |o - m| <= tol_mm}                             */
  uint32_t front_px;    /* #{seen && o <  m - tol_mm}   something in front          */
  uint32_t behind_px;   /* #{seen && o >  m + tol_mm}   the sensor sees through it  */
  uint32_t sum_abs_mm;  /* sum of |o - m| over the inliers (<= 30,976 * 65,535 < 2^32) */
  uint32_t tol_mm;      /* echoed                                                   */
  uint32_t _reserved;   /* 0                                                        */
} se3tn_fit;
/* `model` / `observed`: HOST arrays of n descriptors, as se3tn_preprocess takes them (copied into kernel arguments, no sync); only
 * depth, H, W, left .. bottom are read (rgb may be NULL).  out_dev: n records in device memory, or in mapped pinned host memory (every
 * word is stored there once, not accumulated there).  A launch takes SE3TN_FIT_MAX_PAIRS pairs; larger n are chunked.  Stream-ordered,
 * capturable, allocates nothing (the per-pair counters belong to se3tn_create, and are zero again when a launch ends).  As every
 * compute call of a context: one stream.  SE3TN_E_ARG: n outside [1, se3tn_max_batch], tol_mm outside [1, 65535], a NULL pointer,
 * an empty window or image. */
#define SE3TN_FIT_MAX_PAIRS 32
int se3tn_fit_stats(se3tn_ctx* ctx, const se3tn_crop* model, const se3tn_crop* observed, int n, int tol_mm, se3tn_fit* out_dev,
                    void* stream);
/* The same check inside the one-call tracking bodies.  tol_mm = 0 (default): off -- not one launch, allocation or synchronisation more
 * than before.  1 .. 65535: every se3tn_on_track / _live / _batch / _objects / _objects_live call that `ctx` executes gains one stage
 * after its pose read-back: the mesh of every pair / object rendered at its ESTIMATE in the window of its PREVIOUS pose (the window
 * route: se3tn_render's arithmetic at the y-flipped window of prev_pose; SE3TN_ROUTE_FRAME: the rectangle image A used, at the
 * estimate) -- pixel-aligned with image B by the construction that aligns image A with it -- and se3tn_fit_stats of that render
 * against image B's depth (the staged window of the frame; on the live calls the filled depth the rectangle pass wrote; a window that
 * misses the frame reads its zero pixel: seen_px = 0).  The n renders take the rasteriser's four launches, the records one more, and
 * the call waits for the stream a second time; pose, trans, rot, bbox and image A are the bits they are with the check off.  The
 * first call with the check on allocates the render stack and the (pinned) records.  With the check on a call inside a stream capture
 * is refused with SE3TN_E_STATE. */
int se3tn_set_fit_check(se3tn_ctx* ctx, int tol_mm);   /* 0 = off (default) */
int se3tn_get_fit_check(const se3tn_ctx* ctx);         /* -1 for a NULL ctx */
/* The n records of the LAST tracking call `ctx` executed, into host memory.  SE3TN_E_STATE: that call ran with the check off, failed, or
 * held another number of pairs / objects than n. */
int se3tn_last_fit(se3tn_ctx* ctx, int n, se3tn_fit* out_host);
/* The estimate renders of that call (device, the context's own, valid until its next tracking call): rgb uint8 [n,176,176,3], depth
 * uint16 [n,176,176] -- `pred_color`, `pred_depth` of predict.py:284, with one difference: the reference renders them in the window of
 * the ESTIMATE (render_window(final_estimate) computes a new bbox), these lie in the window of the PREVIOUS pose, the one image B was
 * cropped with, so that the two compare pixel by pixel.  On SE3TN_ROUTE_FRAME they are the raw 176 x 176 crop_bbox of the rendered
 * rectangle.  Either pointer may be NULL.  SE3TN_E_STATE as se3tn_last_fit. */
int se3tn_last_fit_images(se3tn_ctx* ctx, const uint8_t** rgb_dev, const uint16_t** depth_dev);

/* ---- how well a pose hypothesis fits the observed COLOUR ---------------------------------------------------- */
/* The depth record above cannot tell a box from the same box after half a turn; the colours on it can.  A pixel of the 176 x 176
 * crop is COMPARED exactly when it is an inlier of se3tn_fit: valid(m) && valid(o) && |o - m| <= tol_mm on the two depths -- the
 * pixels where the sensor sees the model's surface, not an occluder and not the background.  Both images are read through se3tn_crop
 * descriptors with se3tn_fit_stats' index rule (zero outside the image), the colour at the same source index as the depth.  With
 * m_c(p) / o_c(p) the model / observed byte of channel c (R, G, B) at a compared pixel, the record holds the sums a zero-mean
 * normalised cross-correlation needs.  No word can overflow: 176 * 176 * 255^2 = 2,014,214,400 < 2^32.  All integers: the record
 * does not depend on the order the workgroups arrive in. */
typedef struct se3tn_color_fit {   /* all uint32, 20 words, 80 bytes */
  uint32_t px;          /* number of compared pixels (== se3tn_fit.inlier_px of the same pair) */
  uint32_t tol_mm;      /* echoed                                                              */
  uint32_t sum_m[3];    /* sum of m_c                                                          */
  uint32_t sum_o[3];    /* sum of o_c                                                          */
  uint32_t sum_mm[3];   /* sum of m_c^2                                                        */
  uint32_t sum_oo[3];   /* sum of o_c^2                                                        */
  uint32_t sum_mo[3];   /* sum of m_c * o_c                                                    */
  uint32_t sum_abs[3];  /* sum of |o_c - m_c|                                                  */
} se3tn_color_fit;
/* The colour twin of se3tn_fit_stats: ONE pass over the crop pixels of n pairs accumulates both records.  `model` / `observed`: HOST
 * arrays of n descriptors whose rgb AND depth are device images.  out_dev: n colour records; fit_out_dev (may be NULL): the n depth
 * records, bit for bit what se3tn_fit_stats stores -- both in device memory or mapped pinned host memory (every word stored once).
 * A launch takes SE3TN_FIT_MAX_PAIRS pairs; larger n are chunked.  Stream-ordered, capturable, allocates nothing (its counters belong
 * to se3tn_create and are zero again when a launch ends).  SE3TN_E_ARG: n outside [1, se3tn_max_batch], tol_mm outside [1, 65535], a
 * NULL pointer (a descriptor without rgb or depth included), an empty window or image. */
int se3tn_color_stats(se3tn_ctx* ctx, const se3tn_crop* model, const se3tn_crop* observed, int n, int tol_mm,
                      se3tn_fit* fit_out_dev /* may be NULL */, se3tn_color_fit* out_dev, void* stream);
/* The same pass AMONG tracked objects.  se3tn_color_stats compares at every depth inlier; a tracked object that lies on the model's
 * surface, or touches it, within tol_mm is a depth inlier too, and its colours would enter the correlation as if they were the
 * model's.  `scene` is a third HOST array of n descriptors: the composed depth of the tracked objects (what se3tn_scene_fit writes as
 * `scene`, 0 where there is none), read through its own descriptor with the same index rule, zero outside the image; only depth, H,
 * W and left .. bottom are read.  The caller makes the scene pixel the one at the frame position the observed pixel came from (the
 * same window on a frame-sized image: what se3tn_verify_poses_scene_host does).  With s the scene depth of the crop pixel:
 *     hidden   valid(m) && valid(s) && s <= m + tol_mm    a tracked surface at or in front of the pixel: occluded by it, or claimed by it
 * A hidden pixel enters model_px and hidden_px and nothing else; every other pixel is classified exactly as in se3tn_fit
 * (csrc/fit_rule.h states both; the verdict is the one of se3tn_score_pose_grid_scene and se3tn_align_poses_scene on a model point).
 * A pixel is COMPARED exactly when it is an inlier under this rule.  The depth record keeps se3tn_fit's 32 bytes with `_reserved`
 * holding hidden_px: model_px == hidden_px + (the pixels classified as before), seen_px == inlier_px + front_px + behind_px; the
 * colour record is se3tn_color_fit unchanged, px == inlier_px.  With an all-zero scene every byte of both records is
 * se3tn_color_stats'.  A launch takes SE3TN_FIT_SCENE_MAX_PAIRS pairs (three descriptors per pair travel as kernel arguments); larger
 * n are chunked.  Contract and refusals as se3tn_color_stats (stream-ordered, capturable, allocates nothing, the same counters:
 * as every compute call of a context, one stream); also SE3TN_E_ARG, before anything is written, for a scene descriptor without
 * depth and for an empty scene image or window. */
#define SE3TN_FIT_SCENE_MAX_PAIRS 16
int se3tn_color_stats_scene(se3tn_ctx* ctx, const se3tn_crop* model, const se3tn_crop* observed, const se3tn_crop* scene, int n,
                            int tol_mm, se3tn_fit* fit_out_dev /* may be NULL */, se3tn_color_fit* out_dev, void* stream);
/* The score of a record: the mean over the channels of the zero-mean normalised cross-correlation, in [-1, 1]; it does not change
 * under a gain or an offset of either image, which is what makes a Lambert-shaded render comparable with a camera image.  Host-only,
 * pure, needs no context.  Operation order (utils.color_score returns the same double): per channel c, with n = px, in int64
 *     cov = n * sum_mo - sum_m * sum_o,   vm = n * sum_mm - sum_m * sum_m,   vo = n * sum_oo - sum_o * sum_o
 * (all three below 2^53: their conversion to double is exact);
 *     z_c = (double)cov / (sqrt((double)vm) * sqrt((double)vo))   if vm > 0 && vo > 0, else 0 (a flat channel is no evidence);
 *     score = ((z_0 + z_1) + z_2) / 3.0.
 * The score is 0 when px < min_px or rec is NULL.  per_channel (may be NULL): z_0, z_1, z_2 (zeros when px < min_px). */
double se3tn_color_score(const se3tn_color_fit* rec, int min_px, double per_channel[3] /* may be NULL */);
/* ONE call for "which of these n hypotheses does the frame confirm": the front half of se3tn_on_track_batch with the hypothesis in
 * the place of prev_pose, stopped before the network.  Per pose its own compute_bbox window; the frame's n windows staged through the
 * pinned buffer in one copy; per pose its own image A (the n instances of the rasteriser's four launches: the window route, or the
 * rectangle of the frame on SE3TN_ROUTE_FRAME, whichever `mesh` is on -- the bytes se3tn_on_track_batch renders for the same pose,
 * through the per-instance rasteriser path and the context-owned scratch of se3tn_on_track_objects, with n instances of `mesh`);
 * then se3tn_color_stats' kernel of image A against the window, and one read-back.  poses: HOST float64 [n,16]; rgb / depth: ONE HOST
 * frame uint8 [H,W,3] / uint16 [H,W]; fit_out / color_out: HOST [n]; bbox_out: HOST [n,4,2] compute_bbox corners (v, u), may be NULL.
 * A window that misses the frame compares nothing (px = 0).  SYNCHRONOUS on the default stream, SE3TN_E_STATE inside a stream capture
 * the default stream takes part in (a blocking stream capturing; the capture of a non-blocking stream is not visible from here: a caller
 * who has one open must not call -- Engine.verify_poses refuses under a capture of torch's current stream);
 * SE3TN_E_ARG on a host-only context, for n outside [1, se3tn_max_batch], tol_mm outside [1, 65535], and for every pose
 * se3tn_on_track_batch refuses (not in front of the camera, an empty window, singular).  Leaves no state behind: the tracking calls
 * that follow return the bits they return on a fresh context. */
int se3tn_verify_poses_host(se3tn_ctx* ctx, se3tn_mesh* mesh, const double* poses, int n, const double K[9], double object_width_mm,
                            const uint8_t* rgb, const uint16_t* depth, int H, int W, int tol_mm, se3tn_fit* fit_out,
                            se3tn_color_fit* color_out, int32_t* bbox_out /* [n,4,2], may be NULL */);
/* se3tn_verify_poses_host with the scene of the frame: scene_dev is the composed depth of the tracked objects, DEVICE uint16 [H,W]
 * -- what se3tn_scene_fit writes as `scene`, or what se3tn_search_pose_grid_scene_host leaves on the device
 * (se3tn_last_search_scene); this call renders no occluder itself.  Per pose the scene descriptor is that frame-sized image under the
 * pose's own un-shifted crop window, so the scene pixel is the one at the frame position the observed pixel came from, and the records
 * are se3tn_color_stats_scene's: fit_out[i]._reserved carries hidden_px.  Everything else as se3tn_verify_poses_host: staging, layout,
 * one upload, the rasteriser path, one read-back, the refusals (SE3TN_E_ARG for a NULL scene_dev, before anything is written);
 * SYNCHRONOUS on the default stream (the scene must be complete there: a caller who wrote it on another stream waits for that stream
 * first), and it leaves no state behind. */
int se3tn_verify_poses_scene_host(se3tn_ctx* ctx, se3tn_mesh* mesh, const double* poses, int n, const double K[9], double object_width_mm,
                                  const uint8_t* rgb, const uint16_t* depth, const uint16_t* scene_dev /* device [H,W] */, int H, int W,
                                  int tol_mm, se3tn_fit* fit_out, se3tn_color_fit* color_out, int32_t* bbox_out /* [n,4,2], may be NULL */);

/* ---- the objects of one frame as ONE scene: tracked objects explain each other's occlusions -------------------------------- */
/* se3tn_set_fit_check scores every object alone: where something stands in front of it the pixel is front_px, whatever that
 * something is -- so an object tracked correctly BEHIND another tracked object looks lost.  The reference shows a person the renders
 * beside the frame (cv2.imshow('AB', ...), predict.py:284-290); headless, the same look at the whole frame is one composition of the
 * n objects' depth renders through a shared depth test: per object an integer record over the pixels where it is the nearest
 * tracked surface, an id image of the frame (which tracked object a pixel belongs to) and the composed depth.
 * Layer i (i < n) is a depth sub-image of the rectangle rect = {x0, y0, x1, y1} of the frame (se3tn_render_frame_rect's convention):
 * uint16 millimetres, tightly packed [y1-y0, x1-x0]; x1 <= x0 or y1 <= y0 is a layer with no pixels.  For a frame pixel p:
 *     m_i(p)    the layer's value if p is inside rect_i, else 0;      o(p)  the observed depth
 *     valid(d)  100 < d < 2000, as everywhere in this library
 *     owner(p)  the i with the smallest valid m_i(p), ties to the lowest i
 *     ids(p)    owner + 1, or 0 if no layer is valid at p;            scene(p) = m_owner(p), or 0
 * Always model_px == visible_px + hidden_px and seen_px == inlier_px + front_px + behind_px.  All integers: the record does not
 * depend on the order the workgroups arrive in, and csrc/scene_fit_rule.h holds the statements both the kernel and a host program
 * compile.  No word can overflow: two valid depths differ by at most 1999 - 101 = 1,898, a frame holds at most 2^21 pixels and
 * 2^21 x 1,898 = 3,980,394,496 < 2^32; a frame with H * W > 2^21 is refused (1920 x 1080 fits).  hidden_by is one word and an id one
 * byte: at most SE3TN_SCENE_MAX_OBJECTS layers. */
#define SE3TN_SCENE_MAX_OBJECTS 32
#define SE3TN_SCENE_MAX_PIXELS 2097152   /* 2^21 */
/* (The record and the entry point that fills it share the name se3tn_scene_fit: the record is a struct TAG without a typedef, always
 * written `struct se3tn_scene_fit`, which C and C++ both keep apart from the function.) */
struct se3tn_scene_fit {   /* all uint32, 12 words, 48 bytes */
  uint32_t model_px;     /* #{valid(m_i)}                                                      */
  uint32_t visible_px;   /* #{valid(m_i) && owner == i}                                        */
  uint32_t hidden_px;    /* #{valid(m_i) && owner != i}                                        */
  uint32_t seen_px;      /* #{visible && valid(o)}                                             */
  uint32_t inlier_px;    /* #{seen && |o - m_i| <= tol_mm}                                     */
  uint32_t front_px;     /* #{seen && o <  m_i - tol_mm}   something UNTRACKED in front        */
  uint32_t behind_px;    /* #{seen && o >  m_i + tol_mm}   the sensor sees through it          */
  uint32_t sum_abs_mm;   /* sum of |o - m_i| over the inliers                                  */
  uint32_t hidden_by;    /* bit j set iff object j owns at least one pixel where m_i is valid  */
  uint32_t tol_mm;       /* echoed                                                             */
  uint32_t n_objects;    /* echoed                                                             */
  uint32_t _reserved;    /* 0                                                                  */
};
typedef struct se3tn_scene_layer {
  const uint16_t* depth;   /* device, [y1-y0, x1-x0] uint16 millimetres (not read when the rectangle is empty) */
  int32_t rect[4];         /* {x0, y0, x1, y1}: inside the frame, or empty                                     */
} se3tn_scene_layer;
/* The kernel alone (stands in for the eye that compares the pasted renders, predict.py:285-290).  layers: HOST array of n
 * descriptors (copied into kernel arguments, no sync); observed_dev: device uint16 [H,W]; out_dev: n records in device memory or in
 * mapped pinned host memory (every word is stored there once, not accumulated there); ids_dev (device uint8 [H,W]) and scene_dev
 * (device uint16 [H,W]) may be NULL, and when given are defined for EVERY pixel of the frame (0 where there is no object).
 * One launch: with ids_dev and scene_dev NULL its tiles cover the bounding box of the rectangles only.  Stream-ordered, capturable,
 * allocates nothing (the counters belong to se3tn_create and are zero again when the launch ends).  As every compute call of a
 * context: one stream.  SE3TN_E_ARG, all before anything is written: a NULL pointer (a layer that is not empty without depth
 * included), n outside [1, min(SE3TN_SCENE_MAX_OBJECTS, se3tn_max_batch)], tol_mm outside [1, 65535], H or W < 1, H * W > 2^21, a
 * rectangle that is not empty and not inside the frame, a host-only context. */
int se3tn_scene_stats(se3tn_ctx* ctx, int n, const se3tn_scene_layer* layers /* host */, const uint16_t* observed_dev, int H, int W,
                      int tol_mm, struct se3tn_scene_fit* out_dev, uint8_t* ids_dev /* [H,W], may be NULL */,
                      uint16_t* scene_dev /* [H,W], may be NULL */, void* stream);
/* Render, then the kernel (stands in for predict.py:284, render_window(final_estimate), done for every object of the frame at once).
 * objects[i].mesh at poses[i] (HOST float64 [n,16] row-major) with objects[i].object_width_mm; objects[i].model is NOT read.  Per
 * object the rectangle is se3tn_frame_rect's: the crop window of its pose intersected with the frame; all n rectangles are rendered
 * by the per-instance rasteriser path of se3tn_on_track_objects in full-frame mode (FOUR launches), then the kernel above runs against
 * depth_dev (device uint16 [H,W]).  EVERY mesh is rendered in full-frame mode, whatever its route and whether or not
 * se3tn_mesh_set_texture was called on it: depth in that mode depends on the geometry only, so window-route and frame-route meshes
 * share a call.  The layer is therefore the depth of se3tn_render_frame inside the rectangle (the model is rendered inside its
 * rectangle only) -- NOT the depth se3tn_render gives a window-route mesh, which follows another read-back rule.  A window that
 * misses the frame is an empty layer: all counts 0.  out_dev / ids_dev / scene_dev as se3tn_scene_stats.
 * Stream-ordered; the poses travel through a pinned instance table of the scene stage's own, which a following call waits for (not
 * for the launches).  The stage owns its buffers (instance table, rasteriser scratch, z-buffers, sub-images): a tracking call after
 * a scene call returns the bits it returns on a fresh context, and a scene call between a tracking call and se3tn_last_fit /
 * se3tn_last_fit_images leaves what those return unchanged.  The buffers grow on a first or larger call (draining the device);
 * SE3TN_E_STATE inside a stream capture (the poses are host arguments: a replay could not carry new ones).
 * SE3TN_E_ARG, all before anything is allocated or written: a NULL pointer or mesh, n outside [1, min(SE3TN_SCENE_MAX_OBJECTS,
 * se3tn_max_batch)], tol_mm outside [1, 65535], H or W < 1, H > 2048, H * W > 2^21, object_width_mm <= 0, a pose not in front of the
 * camera (z <= 0) or not finite, an empty crop window, a K entry that is not finite, a host-only context.  The context stays
 * usable after a refusal. */
int se3tn_scene_fit(se3tn_ctx* ctx, int n, const se3tn_object* objects, const double* poses /* host [n,16] */, const double K[9],
                    const uint16_t* depth_dev, int H, int W, int tol_mm, struct se3tn_scene_fit* out_dev, uint8_t* ids_dev /* may be NULL */,
                    uint16_t* scene_dev /* may be NULL */, void* stream);
/* The same from a HOST depth frame (uint16 [H,W]) with the results to host memory: out [n] records, ids uint8 [H,W] and scene uint16
 * [H,W] (either may be NULL).  The staging is [frame | records | ids | scene]: one upload, the launches, one read-back.  SYNCHRONOUS
 * on `stream`, refused inside a stream capture (SE3TN_E_STATE) as se3tn_verify_poses_host refuses; the pinned staging and its device
 * mirror (shared with se3tn_search_poses_host) grow on a first or larger call.  Refusals as se3tn_scene_fit. */
int se3tn_scene_fit_host(se3tn_ctx* ctx, int n, const se3tn_object* objects, const double* poses /* host [n,16] */, const double K[9],
                         const uint16_t* depth /* host [H,W] */, int H, int W, int tol_mm, struct se3tn_scene_fit* out,
                         uint8_t* ids /* host [H,W], may be NULL */, uint16_t* scene /* host [H,W], may be NULL */, void* stream);

/* ---- ADD / ADD-S of n pose pairs in one call ----------------------------------------------------------------- */
/* Utils.py:72-98 `add` / `adi`, the two errors every result of the reference is reported in (eval_ycb.py, eval_ycbineoat.py),
 * which it computes one pose at a time with a KD-tree per frame.  For pair i, with the model points x_j (j < P),
 * a_j = R_pred x_j + t_pred and b_j = R_gt x_j + t_gt:
 *     add[i]  = mean_j |a_j - b_j|                 (Utils.py:72-82)
 *     adds[i] = mean_j min_k |b_j - a_k|           (Utils.py:84-98: the tree holds the PRED cloud, the GT cloud queries it)
 * float64 throughout, no tree: all pairs of points, n * P^2 distance evaluations for ADD-S (P = 2,620: 6.9 M per pose pair).
 * Guarantees:
 *   (a) equal poses give exactly 0.0 for both values: both clouds go through ONE transform function in one stated operation order
 *       with no fused multiply-add, so a point has the same bits on both sides;
 *   (b) a pair's two doubles depend on (points, pred_i, gt_i) only -- not on n, on the pair's place in the call, on how the call is
 *       cut into chunks, or on the run: every sum is formed in a fixed order, without floating-point atomics;
 *   (c) the device-pointer entry point allocates nothing.
 * A points handle holds the model points on the device (uploaded once) and the partial-sum scratch of one chunk of
 * SE3TN_POSE_ERRORS_CHUNK pairs; larger n are cut into chunks inside the call.  Calls that share a handle share that scratch: issue
 * them on one stream (as every compute call of a context). */
#define SE3TN_POSE_ERRORS_CHUNK 256          /* pose pairs per launch */
#define SE3TN_POSE_ERRORS_MAX_POINTS 1048576 /* 2^20 */
typedef struct se3tn_points se3tn_points;
/* xyz: HOST float64 [P,3] metres (copied).  SE3TN_E_ARG: a NULL pointer, P outside [1, SE3TN_POSE_ERRORS_MAX_POINTS], a coordinate
 * that is not finite, a host-only context (device = -1) -- all checked before anything is allocated. */
int se3tn_points_create(se3tn_ctx* ctx, const double* xyz, int P, se3tn_points** out);
void se3tn_points_destroy(se3tn_points* points);
int se3tn_points_count(const se3tn_points* points);   /* -1 for NULL */
/* pred_dev / gt_dev: device float64 [n,16], row-major 4x4 poses (metres); row 3 is not read.  add_dev / adds_dev: device (or mapped
 * pinned host) float64 [n]; either may be NULL (not both), and with adds_dev NULL the all-pairs loop is not run -- add has the same
 * bits either way.  Any n >= 1.  Stream-ordered, capturable, allocates nothing.  The poses are not inspected: a pose that is not
 * finite gives a result that is not finite for its pair (and for no other), which is the caller's business. */
int se3tn_pose_errors(se3tn_ctx* ctx, const se3tn_points* points, int n, const double* pred_dev, const double* gt_dev,
                      double* add_dev, double* adds_dev, void* stream);
/* The same from HOST memory: pred / gt float64 [n,16], add_out / adds_out float64 [n] (either may be NULL, not both): one upload, the
 * launches, one read-back.  SYNCHRONOUS on `stream`, refused inside a stream capture (SE3TN_E_STATE); the pinned staging and its
 * device mirror (34 doubles per pair) grow on a first or larger call.  SE3TN_E_ARG: a pose entry that is not finite. */
int se3tn_pose_errors_host(se3tn_ctx* ctx, const se3tn_points* points, int n, const double* pred, const double* gt,
                           double* add_out, double* adds_out, void* stream);

/* ---- re-acquiring a lost object: n candidate poses scored against one depth frame, the best k picked ------------------------- */
/* The reference's only answer to a lost track is an external detector: predict.py:539-541 re-initialises from PoseCNN at the frames
 * --reinit_frames lists.  Here the search is a call: project the model's points under each candidate pose into the observed depth
 * frame and count how many land on the surface the sensor saw.  For candidate i (row-major 4x4 float64, metres; row 3 is not read)
 * and model point x_j of a points handle, all in float64, in this order, without fused multiply-add:
 *     c = R x + t                row r is ((r_r0 x + r_r1 y) + r_r2 z) + t_r: the transform of se3tn_pose_errors
 *     in front    c.z > 0        (false for NaN)
 *     uf = rint(c.x * K[0] / c.z + K[2]),  vf = rint(c.y * K[4] / c.z + K[5])      round half to even, as se3tn_compute_bbox
 *     in frame    in front && 0 <= uf < W && 0 <= vf < H    decided on the doubles, before any integer cast: -0.5 rounds to -0.0
 *                 (inside), W - 0.5 rounds to W for even W (outside); NaN, infinities and huge values are outside
 *     d = depth[vf, uf] (uint16 mm),  m = rint(c.z * 1000.0)  (kept as a double)
 *     seen        in frame && 100 < d < 2000               the validity rule of se3tn_fit_stats
 *     inlier      seen && |d - m| <= tol_mm
 *     front       seen && d < m - tol_mm                    something stands in front of the point
 *     behind      seen && d > m + tol_mm                    the sensor sees through where the point would be
 * A candidate at the truth does not score P inliers: the far side of the object lies behind its near side and counts as `front`.
 * Guarantees:
 *   (a) every count is an integer sum: a record depends on (points, pose_i, depth, K, tol_mm) only -- not on n, on the pose's place
 *       in the call, or on the run -- and equals the same rule evaluated in IEEE float64 anywhere else (tests/pose_search_oracle.py);
 *   (b) a pose is read by its own workgroup alone: one that is not finite harms no other (with a NaN in it, in_frame_pts = 0);
 *   (c) the device-pointer entry points allocate nothing, use no scratch and no atomics.
 * Cost: n * P projections of about 40 float64 operations and one 2-byte gather each, one workgroup per pose (9,317 candidates of a
 * 2,620-point model: 24 M projections); the ranking reads the n records k times with one workgroup. */
#define SE3TN_POSE_SEARCH_MAX_POSES 1048576   /* 2^20 candidates per call */
#define SE3TN_POSE_RANK_MAX 64                /* the largest k */
typedef struct se3tn_point_fit {   /* all uint32, 32 bytes */
  uint32_t points;        /* P                                            */
  uint32_t in_frame_pts;  /* #{in frame}                                  */
  uint32_t seen_pts;      /* #{in frame && valid(d)}                      */
  uint32_t inlier_pts;    /* #{seen && |d - m| <= tol_mm}                 */
  uint32_t front_pts;     /* #{seen && d <  m - tol_mm}                   */
  uint32_t behind_pts;    /* #{seen && d >  m + tol_mm}                   */
  uint32_t tol_mm;        /* echoed                                       */
  uint32_t _reserved;     /* 0                                            */
} se3tn_point_fit;        /* seen = inlier + front + behind <= in_frame <= points */
/* poses_dev: device float64 [n,16]; depth_dev: device uint16 [H,W] millimetres; K: HOST row-major 3x3 (travels as kernel arguments);
 * fit_dev: n records in device memory or mapped pinned host memory (every word stored once).  Stream-ordered, capturable.  The
 * poses are not inspected.  SE3TN_E_ARG: a NULL pointer, a host-only context, points of another device, n outside
 * [1, SE3TN_POSE_SEARCH_MAX_POSES], tol_mm outside [1, 65535], H or W < 1. */
int se3tn_score_poses(se3tn_ctx* ctx, const se3tn_points* points, int n, const double* poses_dev, const uint16_t* depth_dev,
                      int H, int W, const double K[9], int tol_mm, se3tn_point_fit* fit_dev, void* stream);
/* The indices of the k best of n records, best first, into idx_dev (device or mapped pinned host int32 [k]).  Record i has the key
 *     min(inlier_pts, 2^20) * 2^40 + (2^20 - 1 - min(behind_pts, 2^20 - 1)) * 2^20 + (2^20 - 1 - i)
 * -- more inliers, then fewer seen-through points, then the lower index; unique within a call -- and the k largest keys are written
 * in descending order.  Selection without state: round r takes the largest key below round r - 1's winner (k passes over the n
 * records by one workgroup), so the result is deterministic.  Stream-ordered, capturable.  SE3TN_E_ARG: a NULL pointer, a host-only
 * context, n outside [1, SE3TN_POSE_SEARCH_MAX_POSES], k outside [1, min(n, SE3TN_POSE_RANK_MAX)]. */
int se3tn_rank_poses(se3tn_ctx* ctx, int n, const se3tn_point_fit* fit_dev, int k, int32_t* idx_dev, void* stream);
/* Both from HOST memory: poses float64 [n,16], depth uint16 [H,W]; idx_out int32 [k] and fit_out [k] receive the k best candidates'
 * indices and records, best first.  One upload (the poses and the whole frame), the two launches, one read-back.  SYNCHRONOUS on
 * `stream`, refused inside a stream capture (SE3TN_E_STATE); the pinned staging and its device mirror grow on a first or larger
 * call.  SE3TN_E_ARG as the two above, and a pose entry or a K entry that is not finite. */
int se3tn_search_poses_host(se3tn_ctx* ctx, const se3tn_points* points, int n, const double* poses, const uint16_t* depth, int H, int W,
                            const double K[9], int tol_mm, int k, int32_t* idx_out, se3tn_point_fit* fit_out, void* stream);

/* ---- finding an object with no pose to start from: a product lattice of poses, counting only the points that face the camera --- */
/* The reference takes its first pose from a file, from ground truth or from PoseCNN (predict.py:539-541); the search above is local
 * to a pose the track once had.  Two things keep it local.  Its candidates travel as n x 16 doubles although a lattice is a product
 * of a few rotations and a grid of translations; and its count includes the far side of the object, so inlier_pts / points has no
 * fixed meaning and a wide search prefers poses that lay the model flat into a large plane.  Here the FACTORS travel -- n_rot
 * rotations (row-major 3x3) and n_trans translations, candidate i = r * n_trans + t being the pose [R_r | t_t] -- and a points handle
 * may carry one normal per point, so that only the points whose normal faces the camera are counted.
 * For rotation R (rows R0, R1, R2), translation t, model point x and its normal n, all in float64, in this order, without fused
 * multiply-add:
 *     q = (R0 x + R1 y) + R2 z  per row,   c = q + t          the bits of the transform of se3tn_score_poses for the composed pose
 *     with facing = 1:
 *         n' = (R0 nx + R1 ny) + R2 nz  per row
 *         f  = (n'x c.x + n'y c.y) + n'z c.z
 *         facing      f < 0                                     false for NaN and for f == 0, the grazing point
 *         a point that is not facing enters no counter, `points` included
 *     in front, uf, vf, in frame, d, m, seen, inlier, front, behind                exactly as se3tn_score_poses states them
 * With facing = 0 every word of record (r, t) equals the word se3tn_score_poses writes for the composed pose.  With facing = 1 the
 * record's `points` word is the number of facing points, so inlier_pts / points is the share of the visible surface the sensor
 * confirms; in_frame_pts <= points and seen = inlier + front + behind hold as before, _reserved stays 0.  Unit length of the normals
 * is not required: only the sign of f is used.
 * Guarantees:
 *   (a) every count is an integer sum: a record depends on (points, normals, R_r, t_t, depth, K, tol_mm, facing) only -- not on the
 *       grid it travels in, on its place in it, on the tiling or on the run -- and equals the same rule evaluated in IEEE float64
 *       anywhere else (tests/pose_grid_oracle.py);
 *   (b) a rotation or a translation that is not finite harms only its own candidates (with a NaN in it, in_frame_pts = 0);
 *   (c) the device-pointer entry point allocates nothing and uses no atomics on global memory; it is stream-ordered and capturable.
 * Cost: one workgroup per (rotation, 16 translations) rotates the model once into LDS, 1,024 points at a time, and adds each
 * translation: n_rot * n_trans * P projections as above; 72 bytes per rotation and 24 per translation travel instead of 128 per pose. */
/* nxyz: HOST float64 [P,3], one normal per point of the handle (copied and uploaded once); NULL removes the normals.  Synchronous.
 * SE3TN_E_ARG: a NULL handle, a component that is not finite.  se3tn_points_create, se3tn_pose_errors*, se3tn_score_poses and
 * se3tn_search_poses_host do not read the normals. */
int se3tn_points_set_normals(se3tn_points* points, const double* nxyz);
int se3tn_points_has_normals(const se3tn_points* points);   /* 1 | 0; -1 for NULL */
/* rots_dev: device float64 [n_rot,9]; trans_dev: device float64 [n_trans,3]; depth_dev, K, tol_mm, fit_dev (n_rot * n_trans records,
 * candidate order) and the stream as se3tn_score_poses.  The factors are not inspected.  SE3TN_E_ARG: a NULL pointer, n_rot or
 * n_trans < 1, n_rot * n_trans > SE3TN_POSE_SEARCH_MAX_POSES (so se3tn_rank_poses serves the records unchanged), tol_mm outside
 * [1, 65535], H or W < 1, facing neither 0 nor 1, a host-only context, points of another device.  SE3TN_E_STATE: facing = 1 and the
 * handle has no normals. */
int se3tn_score_pose_grid(se3tn_ctx* ctx, const se3tn_points* points, int n_rot, const double* rots_dev, int n_trans,
                          const double* trans_dev, const uint16_t* depth_dev, int H, int W, const double K[9], int tol_mm, int facing,
                          se3tn_point_fit* fit_dev, void* stream);
/* The same from HOST memory with the k best picked (se3tn_rank_poses' order): rots float64 [n_rot,9], trans float64 [n_trans,3], depth
 * uint16 [H,W]; idx_out int32 [k] and fit_out [k] receive the k best candidates' indices (r * n_trans + t) and records, best first.
 * The staging is [rots | trans | depth | pad | fit n | top_fit k | idx k]: one upload, the two launches, one read-back.  SYNCHRONOUS
 * on `stream`, refused inside a stream capture (SE3TN_E_STATE); the pinned staging and its device mirror (shared with
 * se3tn_search_poses_host) grow on a first or larger call.  SE3TN_E_ARG as above, k outside [1, min(n_rot * n_trans,
 * SE3TN_POSE_RANK_MAX)], and a rotation, translation or K entry that is not finite. */
int se3tn_search_pose_grid_host(se3tn_ctx* ctx, const se3tn_points* points, int n_rot, const double* rots, int n_trans,
                                const double* trans, const uint16_t* depth, int H, int W, const double K[9], int tol_mm, int facing,
                                int k, int32_t* idx_out, se3tn_point_fit* fit_out, void* stream);

/* ---- re-acquiring a lost object AMONG tracked ones: the lattice search against the frame and the composed scene ---------------- */
/* The searches above score a candidate against the observed frame alone.  With other tracked objects in the frame that fails twice:
 * a candidate that lays the lost model onto the visible face of a tracked object collects that object's pixels as inliers (the
 * surface is already CLAIMED), and where a tracked object stands in front of a candidate the point counts as `front`, the verdict
 * of "something unknown is in the way", so a correct but half-hidden candidate cannot be compared with an unoccluded wrong one.
 * se3tn_scene_fit(..., scene_dev) writes what the search lacks, the composed depth of any set of tracked objects: scene [H,W] uint16
 * millimetres, 0 where there is none.  For rotation R, translation t, model point x (and normal n), all in float64, in this order,
 * without fused multiply-add:
 *     q, c, facing, in front, uf, vf, in frame, m = rint(c.z * 1000.0)     exactly as se3tn_score_pose_grid states them
 *     s = scene[vf, uf]
 *     hidden     in frame && 100 < s < 2000 && s <= m + tol_mm              a tracked surface at or in front of the point: the point
 *                                                                          is occluded by it, or claimed by it
 *                a hidden point enters hidden_pts and NOTHING else past in_frame_pts -- not seen, inlier, front or behind --
 *                whatever d is
 *     otherwise  d = depth[vf, uf]; seen, inlier, front, behind             exactly as se3tn_score_pose_grid states them
 * The comparisons are made on doubles (s, m and tol_mm are integers in doubles: exact); only the pixel index is cast.
 * The record keeps the 32 bytes and the field order of se3tn_point_fit; word 7, _reserved there, is hidden_pts.  se3tn_rank_poses
 * reads inlier_pts and behind_pts only, so it may be given these records through a cast: (const se3tn_point_fit*)fit_dev.
 * Always seen = inlier + front + behind and hidden + seen <= in_frame <= points; with an all-zero scene every word equals the word
 * se3tn_score_pose_grid writes (hidden_pts = 0 = _reserved).  inlier_pts / (points - hidden_pts) is the share of the surface that is
 * neither hidden nor claimed which the sensor confirms.  Guarantees (a)-(c) of se3tn_score_pose_grid hold with `scene` among what a
 * record depends on (tests/scene_search_oracle.py).  Cost: the work split of se3tn_score_pose_grid, a seventh counter per
 * translation and a second 2-byte gather per point at the pixel the first one reads. */
typedef struct se3tn_scene_point_fit {   /* all uint32, 32 bytes: se3tn_point_fit with word 7 in use */
  uint32_t points;        /* P, or with facing the number of facing points */
  uint32_t in_frame_pts;  /* #{in frame}                                  */
  uint32_t seen_pts;      /* #{in frame && !hidden && valid(d)}           */
  uint32_t inlier_pts;    /* #{seen && |d - m| <= tol_mm}                 */
  uint32_t front_pts;     /* #{seen && d <  m - tol_mm}                   */
  uint32_t behind_pts;    /* #{seen && d >  m + tol_mm}                   */
  uint32_t tol_mm;        /* echoed                                       */
  uint32_t hidden_pts;    /* #{in frame && valid(s) && s <= m + tol_mm}   */
} se3tn_scene_point_fit;  /* seen = inlier + front + behind;  hidden + seen <= in_frame <= points */
/* The device entry: the arguments of se3tn_score_pose_grid and scene_dev, device uint16 [H,W]; fit_dev: n_rot * n_trans records in
 * device memory or mapped pinned host memory (every word stored once with a plain store).  Stream-ordered, capturable, allocates
 * nothing, no atomics on global memory.  Refusals as se3tn_score_pose_grid, a NULL scene_dev among the NULL pointers. */
int se3tn_score_pose_grid_scene(se3tn_ctx* ctx, const se3tn_points* points, int n_rot, const double* rots_dev, int n_trans,
                                const double* trans_dev, const uint16_t* depth_dev, const uint16_t* scene_dev, int H, int W,
                                const double K[9], int tol_mm, int facing, se3tn_scene_point_fit* fit_dev, void* stream);
/* The whole search as one call from HOST memory: rots, trans, depth, k, idx_out as se3tn_search_pose_grid_host, fit_out [k] the
 * winners' scene-aware records; the occluders are n_occ objects (mesh and object_width_mm are read, as se3tn_scene_fit reads them)
 * at occ_poses (HOST float64 [n_occ,16]).  The staging is [rots | trans | depth | pad | scene | pad | fit n | occ_fit n_occ | top_fit
 * k | idx k]: one upload of [rots | trans | depth]; se3tn_scene_fit's render of the occluders and its kernel against the staged
 * frame, composing the scene frame, which stays on the device; the scene-aware grid kernel; se3tn_rank_poses' kernel; one read-back of
 * [occ_fit | top_fit | idx].  occ_fit_out (may be NULL) receives the occluders' own records, those se3tn_scene_fit writes for them.
 * SYNCHRONOUS on `stream`, refused inside a stream capture (SE3TN_E_STATE); the pinned staging and the scene stage's buffers grow
 * on a first or larger call.  Refusals: those of se3tn_search_pose_grid_host and those of se3tn_scene_fit_host (n_occ outside
 * [1, min(SE3TN_SCENE_MAX_OBJECTS, se3tn_max_batch)] among them: a search with no occluders is se3tn_search_pose_grid_host), all
 * before anything is allocated or written, each with its own message.  The context stays usable after a refusal. */
int se3tn_search_pose_grid_scene_host(se3tn_ctx* ctx, const se3tn_points* points, int n_rot, const double* rots, int n_trans,
                                      const double* trans, const uint16_t* depth, int H, int W, const double K[9], int tol_mm,
                                      int facing, int k, int n_occ, const se3tn_object* occluders,
                                      const double* occ_poses /* host [n_occ,16] */, int32_t* idx_out,
                                      se3tn_scene_point_fit* fit_out, struct se3tn_scene_fit* occ_fit_out /* [n_occ], may be NULL */,
                                      void* stream);
/* The scene frame the last successful se3tn_search_pose_grid_scene_host composed: device uint16 [H,W] inside the context's staging
 * mirror, for scoring further candidates with se3tn_score_pose_grid_scene without composing it again.  Valid until the next _host
 * call of the pose family or the scene stage on this context, which lays the staging out anew: copy it (se3tn_memcpy_d2d) to keep it
 * longer.  SE3TN_E_STATE when there is none.  No launch, no sync. */
int se3tn_last_search_scene(se3tn_ctx* ctx, const uint16_t** scene_dev, int* H, int* W);

/* ---- from a lattice node to a pose: point-to-plane steps of n hypotheses against one depth frame (ICP) ------------------------- */
/* The two searches above end at the resolution of their lattices (10 mm, 15 degrees); the network's reach is its normalisers (30 mm,
 * 5 degrees by default), and it needs weights that track.  In between stands a depth-only refinement: a few damped Gauss-Newton steps
 * that pull the model's FACING points onto the surface the sensor saw, for n poses in one launch.  The points handle must carry
 * normals; a normal is used as given (one of length L weights its point by L^2).
 * Per point x with normal n under the pose [R | t], all in float64, in this order, without fused multiply-add:
 *     q  = (R0 x + R1 y) + R2 z  per row,   c = q + t            the transform of se3tn_score_pose_grid
 *     n' = (R0 nx + R1 ny) + R2 nz  per row
 *     f  = (n'x c.x + n'y c.y) + n'z c.z;    facing: f < 0
 *     in front, uf, vf, in frame, d, m, seen                       exactly as se3tn_score_poses states them (facing points only)
 *     paired   seen && |d - m| <= gate_mm
 *     o.z = d / 1000.0;  o.x = ((uf - K[2]) * o.z) / K[0];  o.y = ((vf - K[5]) * o.z) / K[4]       the pixel's back-projection
 *     r  = (n'x (o.x - c.x) + n'y (o.y - c.y)) + n'z (o.z - c.z)                                   the point-to-plane residual
 *     J  = (q x n', n'):  J0 = q.y n'z - q.z n'y,  J1 = q.z n'x - q.x n'z,  J2 = q.x n'y - q.y n'x,  J3..5 = n'
 *          -- the rotation is taken about the object's origin t (q = c - t), not about the camera: a plane seen from the front then
 *          stays where it is along the directions depth cannot observe
 *     fx(v) = (int64) rint(fmin(fmax(v, -256.0), 256.0) * 2^32)                                    (a NaN gives -256 * 2^32)
 * Per pose and iteration, SE3TN_POSE_ALIGN_SUMS = 28 int64 sums over the paired points, in this order:
 *     S_A[i][j], i <= j, row-major (21 words) = sum fx(J_i * J_j);   S_b[i] (6 words) = sum fx(J_i * r);   S_e (1 word) = sum fx(r * r)
 * and two counts, pairs and facing_pts.  Every term is quantised BEFORE it is added, so the sums are integers and do not depend on
 * the order of the reduction; the clamp makes overflow impossible (2^8 * 2^32 * 2^20 points = 2^60) and bounds what a normal may
 * weigh: a product above 256 is cut, so keep normals within a length of about 10 (unit normals are the intended case).
 *     pairs < min_pairs:  stop, status FEW.
 *     solve:  A_ij = (double)S_A * 2^-32, b likewise, A_ii += damping * (double)pairs;  LDL^T without pivoting or square root:
 *             d_j = A_jj - sum_k (L_jk L_jk) d_k,   L_ij = (A_ij - sum_k (L_ik L_jk) d_k) / d_j;   y_i = b_i - sum_k L_ik y_k;   y_i /= d_i;
 *             delta_i = y_i - sum_{k > i} L_ki delta_k -- every inner sum starts from 0.0 and adds left to right over ascending k.
 *             A pivot that is not > 0 (NaN included) or a component of delta = (w, v) that is not finite: stop, status SINGULAR, the
 *             pose unchanged.
 *     update (Cayley, no trigonometry):  a = 0.5 w,  s = (a0 a0 + a1 a1) + a2 a2,  C = ((1 - s) I + 2 a a^T + 2 [a]x) / (1 + s):
 *             C_ii = ((1.0 - s) + 2.0 * (a_i * a_i)) / (1.0 + s),   C_ij = (2.0 * (a_i * a_j) + 2.0 * [a]x_ij) / (1.0 + s) with
 *             [a]x_01 = -a2, _02 = a1, _10 = a2, _12 = -a0, _20 = -a1, _21 = a0 (a subtraction where the sign is minus);
 *             R <- C R, entry (i, j) = (C_i0 R_0j + C_i1 R_1j) + C_i2 R_2j;   t <- t + v.
 *     max_k |delta_k| <= stop:  stop, status CONVERGED (after the update).   After `iters` iterations: status ITERS.
 * A pose that is not finite pairs nothing: FEW after one evaluation, rows 0-2 returned with the bits they came in with.  Row 3 of an
 * input pose is not read; row 3 of an output pose is 0 0 0 1.
 * Guarantees:
 *   (a) a pose's output (pose, record, sums) depends on (points, normals, pose, depth, K, params) only -- not on n, on its place in
 *       the call, on the thread count or on the run -- and equals the same rule evaluated in IEEE float64 anywhere else
 *       (tests/pose_align_oracle.py; csrc/pose_align_math.h holds the statements, which tests/c_abi/pose_align_check.cpp runs on the host);
 *   (b) a pose is read and written by its own workgroup alone: a bad one harms no other;
 *   (c) the device-pointer entry point allocates nothing and uses no atomics on global memory; it is stream-ordered and capturable.
 * Cost: ONE launch runs all iterations, one workgroup per pose; an iteration is P projections, 28 quantised products per paired
 * point, a reduction through LDS and a 6 x 6 solve by one thread. */
#define SE3TN_POSE_ALIGN_MAX_POSES 4096
#define SE3TN_POSE_ALIGN_MAX_ITERS 64
#define SE3TN_POSE_ALIGN_SUMS 28
#define SE3TN_ALIGN_ITERS 0       /* `iters` iterations done                          */
#define SE3TN_ALIGN_CONVERGED 1   /* max |delta| <= stop                              */
#define SE3TN_ALIGN_FEW 2         /* pairs < min_pairs at the last evaluated pose     */
#define SE3TN_ALIGN_SINGULAR 3    /* a pivot not > 0 or a step that is not finite     */
typedef struct se3tn_align_params {
  int32_t gate_mm;     /* pairing gate |d - m| <= gate_mm, [1, 65535]                 */
  int32_t iters;       /* [1, SE3TN_POSE_ALIGN_MAX_ITERS]                              */
  int32_t min_pairs;   /* [6, 2^20]                                                    */
  int32_t _reserved;   /* 0                                                            */
  double damping;      /* >= 0: added to the diagonal per paired point                 */
  double stop;         /* >= 0: the step size that counts as converged                 */
} se3tn_align_params;
typedef struct se3tn_align_rec {   /* 40 bytes */
  uint32_t iterations;   /* iterations evaluated                                       */
  uint32_t status;       /* SE3TN_ALIGN_*                                              */
  uint32_t pairs;        /* paired points at the last evaluated pose                   */
  uint32_t facing_pts;   /* facing points at the last evaluated pose                   */
  int64_t sum_r2;        /* S_e of the last evaluated pose (metres^2 * 2^32)           */
  uint32_t pairs0;       /* paired points at the first evaluated pose                  */
  uint32_t _reserved;    /* 0                                                          */
  int64_t sum_r2_0;      /* S_e of the first evaluated pose                            */
} se3tn_align_rec;       /* the last evaluated pose is the pose BEFORE the last update */
/* poses_dev: device float64 [n,16]; poses_out_dev: device float64 [n,16], may equal poses_dev; rec_dev: n records; sums_dev: int64
 * [n,28], the sums of the last evaluated iteration, or NULL; depth_dev, K and the stream as se3tn_score_poses.  The poses are not
 * inspected.  SE3TN_E_ARG, each with a message of its own: a NULL pointer, n outside [1, SE3TN_POSE_ALIGN_MAX_POSES], gate_mm outside
 * [1, 65535], iters outside [1, SE3TN_POSE_ALIGN_MAX_ITERS], min_pairs outside [6, 2^20], _reserved != 0, damping or stop negative or
 * not finite, H or W < 1, a host-only context, points of another device.  SE3TN_E_STATE: the handle has no normals. */
int se3tn_align_poses(se3tn_ctx* ctx, const se3tn_points* points, int n, const double* poses_dev, const uint16_t* depth_dev, int H,
                      int W, const double K[9], const se3tn_align_params* params, double* poses_out_dev, se3tn_align_rec* rec_dev,
                      int64_t* sums_dev, void* stream);
/* The same from HOST memory: poses float64 [n,16], depth uint16 [H,W]; poses_out [n,16], rec_out [n], sums_out int64 [n,28] or NULL.
 * The staging is [poses | depth | pad | poses_out | rec | sums]: one upload, one launch, one read-back.  SYNCHRONOUS on `stream`,
 * refused inside a stream capture (SE3TN_E_STATE); the pinned staging and its device mirror (shared with se3tn_search_poses_host) grow
 * on a first or larger call.  SE3TN_E_ARG as above, and a pose entry (rows 0-2) or a K entry that is not finite. */
int se3tn_align_poses_host(se3tn_ctx* ctx, const se3tn_points* points, int n, const double* poses, const uint16_t* depth, int H, int W,
                           const double K[9], const se3tn_align_params* params, double* poses_out, se3tn_align_rec* rec_out,
                           int64_t* sums_out, void* stream);

/* ---- the alignment AMONG tracked objects: points hidden by the composed scene are not paired ------------------------------------ */
/* se3tn_align_poses pairs every facing point with whatever the sensor saw within gate_mm of it.  Among other objects that pulls a
 * hypothesis onto a neighbour's face (the surface is already CLAIMED by a tracked object) or tilts it onto an object lying on the
 * lost one.  With `scene` [H,W] uint16 millimetres, the composed depth of the tracked objects as se3tn_scene_fit(..., scene_dev)
 * writes it (0 where there is none), the rule of se3tn_align_poses gains ONE step, for a FACING point whose pixel is in frame,
 * before d is looked at (q, c, n', f, uf, vf, m = rint(c.z * 1000.0) exactly as stated there):
 *     s = scene[vf, uf]
 *     hidden     100 < s < 2000 && s <= m + scene_tol_mm                   the predicate of se3tn_score_pose_grid_scene, on doubles
 *                a hidden point enters hidden_pts and NOTHING else past facing_pts: it is not paired whatever d is and adds to none
 *                of the 28 sums
 *     otherwise  d = depth[vf, uf]; seen, paired, o, r, J, fx                exactly as se3tn_align_poses states them
 * scene_tol_mm, [1, 65535], is the tolerance of the hidden verdict -- the tol_mm of se3tn_score_pose_grid_scene -- and independent
 * of params->gate_mm.  Sums, solve, update and stop rules are those of se3tn_align_poses.
 * The record keeps the 40 bytes and the field order of se3tn_align_rec; the word at offset 28, _reserved there, is hidden_pts: the
 * hidden points at the last evaluated pose.  Always pairs + hidden_pts <= facing_pts.  With an all-zero scene every byte of pose,
 * record and sums equals what se3tn_align_poses writes (hidden_pts = 0 = _reserved).  Guarantees (a)-(c) of se3tn_align_poses hold
 * with (scene, scene_tol_mm) among what a pose's output depends on (tests/scene_align_oracle.py;
 * tests/c_abi/pose_align_scene_check.cpp runs the statements on the host).  Cost: that of se3tn_align_poses, a third count and a
 * second 2-byte gather per facing in-frame point, at the pixel the first one reads. */
typedef struct se3tn_scene_align_rec {   /* 40 bytes: se3tn_align_rec with the word at offset 28 in use */
  uint32_t iterations;   /* iterations evaluated                                       */
  uint32_t status;       /* SE3TN_ALIGN_*                                              */
  uint32_t pairs;        /* paired points at the last evaluated pose                   */
  uint32_t facing_pts;   /* facing points at the last evaluated pose                   */
  int64_t sum_r2;        /* S_e of the last evaluated pose (metres^2 * 2^32)           */
  uint32_t pairs0;       /* paired points at the first evaluated pose                  */
  uint32_t hidden_pts;   /* hidden points at the last evaluated pose                   */
  int64_t sum_r2_0;      /* S_e of the first evaluated pose                            */
} se3tn_scene_align_rec; /* pairs + hidden_pts <= facing_pts                           */
/* The device entry: the arguments of se3tn_align_poses, scene_dev (device uint16 [H,W]: what se3tn_scene_fit(..., scene_dev) and
 * se3tn_last_search_scene hand out) and scene_tol_mm.  Stream-ordered, capturable, allocates nothing, no atomics on global memory.
 * Refusals as se3tn_align_poses, in the same order, a NULL scene_dev among the NULL pointers, and scene_tol_mm outside [1, 65535]
 * (SE3TN_E_ARG, the message names scene_tol_mm). */
int se3tn_align_poses_scene(se3tn_ctx* ctx, const se3tn_points* points, int n, const double* poses_dev, const uint16_t* depth_dev,
                            const uint16_t* scene_dev, int H, int W, const double K[9], const se3tn_align_params* params,
                            int scene_tol_mm, double* poses_out_dev, se3tn_scene_align_rec* rec_dev, int64_t* sums_dev, void* stream);
/* The same from HOST memory: poses, depth, poses_out, rec_out, sums_out as se3tn_align_poses_host, scene HOST uint16 [H,W].  The
 * staging is [poses | depth | pad | scene | pad | poses_out | rec | sums]: one upload of [poses | depth | pad | scene], one launch, one
 * read-back.  SYNCHRONOUS on `stream`, refused inside a stream capture (SE3TN_E_STATE); it shares the pinned staging of the pose
 * family.  Refusals as se3tn_align_poses_host and those above. */
int se3tn_align_poses_scene_host(se3tn_ctx* ctx, const se3tn_points* points, int n, const double* poses, const uint16_t* depth,
                                 const uint16_t* scene, int H, int W, const double K[9], const se3tn_align_params* params,
                                 int scene_tol_mm, double* poses_out, se3tn_scene_align_rec* rec_out, int64_t* sums_out, void* stream);

/* ---- host-side pieces of the path (pure CPU, float64, as the reference computes them) ----- */
/* Utils.py:302-316 compute_bbox with scale (1000,1000,1000): pose row-major 4x4 (metres), K
 * row-major 3x3, width in mm; out_vu[8] = 4 x (v,u) int32, np.round (half-to-even). */
int se3tn_compute_bbox(const double pose[16], const double K[9], double object_width_mm,
                       int32_t out_vu[8]);
/* The rectangle the SE3TN_ROUTE_FRAME route renders for this pose: compute_bbox's crop window (left, top, right, bottom = min / max of
 * the corners) intersected with the H x W frame, rect = {x0, y0, x1, y1} as se3tn_render_frame_rect takes it -- the size of the
 * sub-image, for callers that bring their own buffers.  A window that misses the frame is reported as the empty rectangle
 * {0, 0, 0, 0} (return value SE3TN_OK).  SE3TN_E_ARG: z <= 0 or a pose that is not finite, width <= 0, H or W < 1. */
int se3tn_frame_rect(const double pose[16], const double K[9], double object_width_mm, int H, int W, int32_t rect[4]);
/* datasets.py:159-175 processPredict on the host. */
int se3tn_pose_update_host(const double poseA[16], const float trans[3], const float rot[3],
                           double trans_normalizer, double rot_normalizer, double poseB[16]);

/* ---- introspection for tests / profiling --------------------------------------------------- */
/* Device pointer + geometry of an internal NHWC activation buffer after se3tn_infer.
 * names: "inA" "inB" [n,182,182,4] (3-pixel zero border), "stem" [n,88,88,128]; the conv activations carry a one-pixel
 * zero border: "pool" "t64" "q64" [n,46,46,128] (channels 0-63 branch A, 64-127 branch B),
 * "ab" "ab_t" [n,24,24,256], "head" "head_t" [n,13,13,1024] (0-511 trans, 512-1023 rot).
 * dims = {H, W, C} as stored (borders included).  A stage the last se3tn_infer (or se3tn_on_track_objects, or the graph it
 * replayed) did NOT write is refused with SE3TN_E_STATE instead of handing out an older call's data: "stem" after the batch 1-5
 * stem + pool kernel, "ab_t" / "head_t" / "head" after the fused Winograd blocks, "head" when the tail added the last head conv's
 * partial sums itself (see se3tn_keep_intermediates).  "inA" / "inB" are always handed out (se3tn_preprocess fills them too).
 * After a call under SE3TN_PREC_F16X3 the words of "pool" "t64" "q64" "ab" "ab_t" "head_t" are split rows -- per pixel and per 32
 * channels 32 f16 hi halves, then their 32 f16 lo halves, value = hi + lo -- and "inA" / "inB" hold 4 hi | 4 lo per pixel; "stem"
 * and "head" are float32, and so is the "head_t" the fused head block stores on request (it keeps that map on chip as float32). */
int se3tn_debug_buffer(se3tn_ctx* ctx, const char* name, const float** ptr, int32_t dims[3]);
/* The fused Winograd blocks (batches of n >= the se3tn_set_winograd threshold) keep the activation between a
 * residual block's two convolutions in LDS and reduce the heads' last activation in registers: "ab_t", "head_t"
 * and "head" are then NOT written.  on != 0 makes those kernels store them as well (tests, feature inspection);
 * results are bit-identical either way.  At 1-5 pairs the batch-1 kernel family never writes the un-pooled "stem" map nor the
 * final "head" map (the tail adds the last conv's partial sums itself): on != 0 selects, for those two stages, the general kernels
 * that do write them -- same tolerances, another summation order (not the same bits as the default at 1-5 pairs). */
int se3tn_keep_intermediates(se3tn_ctx* ctx, int on);
/* stream-ordered device-to-device copy (lets a ctypes host wrap the raw pointers above into its
 * own tensors without a second HIP binding) */
int se3tn_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);
/* Timing hooks used by bench.py.  se3tn_profile_enable(ctx, slots) (slots <= 64, 0 = off) makes
 * every following se3tn_infer record hipEvents around each of its launches on `stream`, into event
 * set (call index % slots) -- no synchronisation is added to the timed loop.  Reading a slot
 * synchronises on its last event.  conv_ms = time inside the dominant kernel family (the 3x3
 * f32-MFMA convolutions, `conv_launches` launches), total_ms = all launches of that infer. */
int se3tn_profile_enable(se3tn_ctx* ctx, int slots);
int se3tn_profile_read(se3tn_ctx* ctx, int slot, float* conv_ms, int* conv_launches, float* total_ms);
/* Per-launch breakdown of one slot: fills up to `cap` names / milliseconds, returns the number of
 * launches (0 on error, see se3tn_last_error). */
int se3tn_profile_launches(se3tn_ctx* ctx, int slot, int cap, const char** names, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* SE3TRACKNET_H */
