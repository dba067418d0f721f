/*
 * bugseg — MI355X-native (gfx950) ENet segmentation -> BEV occupancy-grid path, C ABI.
 *
 * The reference exposes no FFI: its boundary is the Python plugin API of models.py / bev.py /
 * occgrid_to_ros.py. These entry points are what that API's Python shims
 * (bugcar_image_segmentation_amd/{models,bev,occgrid_to_ros}.py, bound with ctypes) call; each
 * cites the reference interface it replaces. A ctypes binding a maintainer would add to the
 * reference itself is shown in INTEGRATION.md.
 *
 * Conventions
 *  - Every pointer argument named *_dev is a DEVICE pointer owned by the caller (e.g. a
 *    torch tensor's data_ptr()). The library owns only its weights, tables and scratch.
 *  - `stream` is a hipStream_t (NULL = the legacy default stream). All work of one call is
 *    enqueued on it; calls return without synchronising.
 *  - Return 0 on success or a negative BUGSEG_E* code; bugseg_last_error() explains it.
 *  - Calls on one context must not overlap in time from several host threads.
 *  - A context's forward activation arena is ONE set of buffers: ENet forwards of one context must
 *    all be enqueued on one stream (run concurrent frame shards on one context each, as
 *    pipeline.py does). BEV calls of one context may be enqueued on several streams at once: the
 *    warp-tap and polar tables are read-only once built, and the laserscan batch scratch is either
 *    the caller's workspace (bugseg_bev_occgrid_ws) or kept per stream (bugseg_bev_occgrid).
 *  - Stream order, graphs: the BEV entry points never synchronise the caller's stream or the
 *    device. A table for a new geometry is built on the context's private stream and waited for
 *    there before the call enqueues its work, so the first call at a new geometry or batch may be
 *    captured into a HIP graph (so may the first forward at a shape). Memory a captured call used
 *    (arena, tables, scratch) is kept until bugseg_destroy. The rare eviction of an uncaptured
 *    table (a 5th geometry) and arena reallocation at a new shape outside a capture synchronise
 *    the device first, so nothing in flight reads freed memory.
 *  - Tensor shapes: activations are NHWC. The "engine input" tensor is (B, H, W, 8): RGB plus 5
 *    zero channels, in the context precision (f32, bf16 or f16).
 */
#ifndef BUGSEG_H
#define BUGSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bugseg_ctx bugseg_ctx;

enum {
    BUGSEG_OK = 0,
    BUGSEG_EINVAL = -1,   /* bad argument / shape (reference: AssertionError, bev.py:169)     */
    BUGSEG_ENOMEM = -2,
    BUGSEG_EHIP = -3,     /* HIP runtime error                                                 */
    BUGSEG_EFORMAT = -4,  /* malformed weight blob (reference: GraphDef ParseFromString error)  */
    BUGSEG_ESTATE = -5    /* e.g. forward before load_weights                                  */
};

/* Precisions: activations and weights stored as f32 (the parity mode), bf16 (the throughput mode) or
 * f16 (the same bytes and MFMA rate as bf16 with 3 more mantissa bits: closer class agreement with
 * fp32; range +-65504). Products accumulate in f32 in every mode. */
enum { BUGSEG_FP32 = 0, BUGSEG_BF16 = 1, BUGSEG_F16 = 2 };

/* out_kind of bugseg_enet_forward */
enum {
    BUGSEG_OUT_LOGITS_F32 = 0,  /* (B, C, H, W) f32 NCHW — the TF output tensor "CATkrIDy/concat:0" (models.py:16,52) */
    BUGSEG_OUT_CLASS15_U8 = 1,  /* (B, H, W) u8 raw argmax class id (models.py:55)                    */
    BUGSEG_OUT_CLASS3_U8 = 2,   /* (B, H, W) u8 in {0,1,2}: ENET.predict (models.py:55-58,67)         */
    BUGSEG_OUT_BINARY_U8 = 3    /* (B, H, W) u8 in {0,1}:   ENET.predict_binary (models.py:78-81)     */
};

/* out_layout of bugseg_preprocess */
enum {
    BUGSEG_PRE_ENGINE = 0,      /* (B, H, W, 8) engine input, context precision                      */
    BUGSEG_PRE_NCHW_F64 = 1,    /* (B, 3, H, W) f64: exactly ENET.preprocess's array (models.py:84-95) */
    BUGSEG_PRE_NCHW_F32 = 2,    /* (B, 3, H, W) f32: what TF casts the feed to                         */
    BUGSEG_PRE_BGR_U8 = 3       /* (B, H, W, 3) u8: the resized BGR frame only (models.py:87), for
                                   bugseg_enet_forward_bgr, which fuses the rest of preprocess    */
};

/* Geometry of bev_transform_tools.create_occupancy_grid (bev.py:166-195), computed on the host
 * by the Python shim exactly as the reference computes it. */
typedef struct {
    double M[9];        /* forward bev matrix, row-major (bev.py:182 _bev_matrix)                */
    int in_rows;        /* segmap rows  (== "input image size"[0], assert at bev.py:169)        */
    int in_cols;        /* segmap cols  (== "input image size"[1])                               */
    int warp_w;         /* after_warp_width  (bev.py:178; dsize of warpPerspective, bev.py:182)  */
    int warp_h;         /* after_warp_height (bev.py:179)                                        */
    int occ_w_px;       /* bev.py:174 */
    int occ_h_px;       /* bev.py:176 */
    int occ_w;          /* bev.py:173 grid cells across */
    int occ_h;          /* bev.py:175 grid cells down   */
    int left_x;         /* bev.py:183 */
    int top_y;          /* bev.py:184 */
    int ros_layout;     /* 0: reference (occ_h, occ_w) grid; 1: ROS data order = flip(0)+rot90ccw
                           of it, (occ_w, occ_h) row-major (occgrid_to_ros.py:18-25)            */
    int variant;        /* 0: create_occupancy_grid (bev.py:166-246): occupied = template {1,3},
                              encoding {0:-1, 1:100, 2:0, 3:100};
                           1: create_occupancy_grid_binary (bev.py:97-165): occupied = {1}, the
                              reference's uint8 encoding {0:-1, 1:100, 2:0, 3:-100}               */
    int laserscan;      /* 1: laserscan-like mode ("is_laserscan", bev.py:37): variant 0 keeps only the
                              obstacle cells nearest the vehicle along each polar ray, the rest of
                              the obstacles become unknown (bev.py:216-240); variant 1 returns TWO
                              grids per frame, out_dev = (2, B, ...): the encoded grid, then the
                              polar re-projection of its nearest obstacles (bev.py:143-164)        */
} bugseg_bev_params;

/* Library version (major*10000 + minor*100 + patch). */
int bugseg_version(void);

/* Create / destroy a context on HIP device `device`, computing in `precision` (BUGSEG_FP32 is the
 * parity mode: logits within 1e-3 of the fp32 oracle; BUGSEG_BF16 / BUGSEG_F16 the throughput modes).
 * Replaces ENET.__init__'s tf.compat.v1.Session() (models.py:21-22). */
int bugseg_create(int device, int precision, bugseg_ctx **out);
int bugseg_destroy(bugseg_ctx *ctx);

/* Load a BSG1 weight blob (format: bugcar_image_segmentation_amd/enet_spec.py) from HOST memory;
 * folds batch-norm, packs weights for the MFMA kernels and uploads them.
 * Replaces GFile(...).read() + GraphDef.ParseFromString + import_graph_def (models.py:25-30). */
int bugseg_load_weights(bugseg_ctx *ctx, const void *blob, size_t bytes);

/* Number of classes of the loaded model (0 before load). */
int bugseg_num_classes(const bugseg_ctx *ctx);

/* Bytes of the engine-input tensor for (B, H, W) in the context precision. */
size_t bugseg_input_bytes(const bugseg_ctx *ctx, int B, int H, int W);

/* ENET.preprocess (models.py:84-95) on a batch: BGR u8 (B, H0, W0, 3) -> resize to (H, W)
 * (cv2.resize INTER_LINEAR fixed point; identity when equal) -> BGR->RGB -> (x/256-mean)/std.
 * out_layout: BUGSEG_PRE_*. */
int bugseg_preprocess(bugseg_ctx *ctx, const uint8_t *bgr_dev, int B, int H0, int W0, int H, int W,
                      int out_layout, void *out_dev, void *stream);

/* (B, 3, H, W) NCHW float (is_f64 ? f64 : f32) -> engine input (B, H, W, 8). This is the feed of
 * ENET.predict's sess.run (models.py:43-44), which receives ENET.preprocess's NCHW array. */
int bugseg_nchw_to_input(bugseg_ctx *ctx, const void *x_dev, int is_f64, int B, int H, int W,
                         void *out_dev, void *stream);

/* ENet forward + fused argmax/remap epilogue. in_dev: engine input (B, H, W, 8); H and W must be
 * multiples of 8. out_kind: BUGSEG_OUT_*. Replaces sess.run + tf.math.argmax + tf.where
 * (models.py:43-58, 71-80). */
int bugseg_enet_forward(bugseg_ctx *ctx, const void *in_dev, int B, int H, int W, int out_kind,
                        void *out_dev, void *stream);

/* Same as bugseg_enet_forward, but reading raw BGR u8 frames (B, H, W, 3) already at the model
 * resolution: BGR->RGB and (x/256-mean)/std (models.py:89-91) are applied while the initial block
 * loads its input, so the normalised tensor never exists in HBM. Results are identical to
 * bugseg_preprocess(ENGINE) followed by bugseg_enet_forward. */
int bugseg_enet_forward_bgr(bugseg_ctx *ctx, const uint8_t *bgr_dev, int B, int H, int W, int out_kind,
                            void *out_dev, void *stream);

/* bugseg_enet_forward_bgr enqueuing only launches [first_op, last_op) of the forward's plan
 * (last_op = -1: to the end; bugseg_plan_info gives the count). Calling it for [0, k) and then for
 * [k, -1) enqueues exactly the full forward; in between the caller may record an event, so another
 * stream's work can start at a chosen point of this forward (pipeline.py: the shard offset).
 * fp32 range precondition: the range words (the measured max |.| of every stored activation, which
 * pick the launches' power-of-two exponents) are cleared, and the input measured, only by a range that
 * starts at op 0; launches of a range starting at first_op > 0 read the words the earlier launches of
 * the SAME forward wrote — so call [0, k) before [k, -1) on the same input, as pipeline.py does.
 * Started at k > 0 without it, a range uses whatever the last forward left (stale exponents: still
 * overflow-safe, as the words only grow, but not necessarily those of a full forward on this input). */
int bugseg_enet_forward_bgr_ops(bugseg_ctx *ctx, const uint8_t *bgr_dev, int B, int H, int W, int out_kind,
                                void *out_dev, int first_op, int last_op, void *stream);

/* bugseg_enet_forward_bgr_ops computing only output rows [row0, row1) of every frame. The plan is the
 * same except for its last six launches (the 128 -> 64 upsampling block, the two stage-4 bottlenecks,
 * the 64 -> 16 upsampling block, the stage-5 bottleneck and the class layer), which run only the tiles /
 * pixel groups the window needs: each launch's window is the rows its consumer reads (class layer: input
 * rows y, y + 1 for output rows 2y, 2y + 1; bottlenecks: whole tile rows counted from the first row
 * needed, reading one row above and below; upsampling blocks: input row y for output rows 2y, 2y + 1).
 * In the fp32 mode the walk goes on into stage 3 through the (at most two) fused C = 128 bottlenecks that feed
 * the 128 -> 64 block, each with its own vertical reach — its dilation for a 3x3 block, 2 for the asymmetric
 * block's 5x1 conv: a row-dilated block (4 x 80 tiles of one row phase) runs exactly the rows its consumer
 * reads, every row phase starting at its first needed row and skipping the fragments of rows past the window;
 * an asymmetric block runs whole tile rows from its first needed row, in the tile form picked for those rows.
 * The walk stops at the first block whose window is the whole frame, whose form has no windowed kernel, or
 * whose window runs no fewer rows than its full-frame launch; BUGSEG_ROW_WINDOW_S3=0 keeps it
 * to the six launches above. For a span in the lower half of a 480-row frame that is ENet's blocks 3.7
 * (dilation 16) and 3.6 (asymmetric). The encoder and the other stage-3 blocks run whole frames. Output rows outside [row0, row1) are NOT written: out_dev keeps
 * what it held. Every out_kind is supported. [0, H), or a window that is empty or leaves [0, H), runs
 * exactly bugseg_enet_forward_bgr_ops; so does a plan that does not end in those six fused launches
 * (BUGSEG_NO_FUSE, BUGSEG_CLS_CONV, BUGSEG_CLS_FUSE).
 * Rows inside the window are bit-identical to the full forward's in the bf16 / f16 modes, and in the fp32
 * mode whenever every range exponent is 0 (the default weights): a windowed launch folds into the range
 * words only the maxima of the tiles it runs, so where an exponent is non-zero a windowed and a full
 * forward may pick different exponents and differ within the fp32 mode's parity bar.
 * Meant for a consumer that reads part of the class map (bugseg_bev_source_rows). */
int bugseg_enet_forward_bgr_rows(bugseg_ctx *ctx, const uint8_t *bgr_dev, int B, int H, int W, int out_kind,
                                 void *out_dev, int row0, int row1, int first_op, int last_op, void *stream);

/* The class-map rows [*row0, *row1) (half-open) that bugseg_bev_occgrid's result depends on for these
 * parameters, any mode: the smallest and largest row of a warp tap that lies inside the class map and
 * carries a non-zero bilinear weight, over the 5x5 template window of every grid cell (BORDER_CONSTANT
 * taps read no row). Rows outside it may hold anything. in_rows / in_cols must equal p's. A property of
 * the geometry, recorded when its warp-tap table is built; the call builds the table if it is missing, as
 * the first bugseg_bev_occgrid call would (on the context's setup stream, waited for there: legal while a
 * stream of the caller's is being captured). No valid tap at all: the empty window (0, 0). */
int bugseg_bev_source_rows(bugseg_ctx *ctx, const bugseg_bev_params *p, int in_rows, int in_cols, int *row0,
                           int *row1);

/* Fused BEV rasteriser over a batch of class maps: seg_dev (B, in_rows, in_cols) u8
 * -> out_dev (B, occ_h, occ_w) int8 (or the ROS layout, see ros_layout).
 * Replaces bev_transform_tools.create_occupancy_grid (bev.py:166-246) or, with variant = 1,
 * create_occupancy_grid_binary (bev.py:97-165), either branch (p->laserscan). The laserscan mode
 * keeps polar tables per geometry in the context and its batch scratch per (context, stream). */
int bugseg_bev_occgrid(bugseg_ctx *ctx, const uint8_t *seg_dev, int B, const bugseg_bev_params *p,
                       int8_t *out_dev, void *stream);

/* The stream-ordered form of bugseg_bev_occgrid: the laserscan batch scratch is a caller-owned
 * device workspace of at least bugseg_bev_workspace_bytes(p, B) bytes (0 when p->laserscan is 0:
 * workspace may then be NULL), used only by the work this call enqueues on `stream` — so the caller's
 * allocator orders its reuse (e.g. torch's caching allocator, graph pools included). */
size_t bugseg_bev_workspace_bytes(const bugseg_bev_params *p, int B);
int bugseg_bev_occgrid_ws(bugseg_ctx *ctx, const uint8_t *seg_dev, int B, const bugseg_bev_params *p,
                          int8_t *out_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* cv2.warpPerspective(frame, M, (warp_w, warp_h)) with INTER_LINEAR and a constant 0 border, over a batch of
 * frames: img_dev (B, in_rows, in_cols[, 3]) u8 (channels 1 or 3, interleaved) -> out_dev (B, warp_h, warp_w[, 3])
 * u8. The arithmetic is the rasteriser's own warp (double inverse map with OpenCV's per-block split, cvRound to
 * 1/32 pixel, Q15 weights, (sum + 2^14) >> 15), per channel. gray = 1, for 3 channels only, stores one byte per
 * pixel instead: (1868 b + 9617 g + 4899 r + 8192) >> 14 of the warped pixel (cv2.cvtColor(., COLOR_BGR2GRAY) of
 * an 8-bit image). Of p only M, in_rows, in_cols, warp_w and warp_h are read. A singular M warps like OpenCV: the
 * inverse is taken as all zeros and every pixel samples the source's corner. One launch, no workspace, no tables;
 * the call never synchronises and may be captured on its first call. BUGSEG_EINVAL, and nothing is launched: a
 * NULL argument, channels other than 1 or 3, gray other than 0 or 1 or with 1 channel, B < 1, an empty source
 * or result, a frame or a result of 2^31 bytes or more, overlapping buffers. */
int bugseg_bev_warp_image(bugseg_ctx *ctx, const uint8_t *img_dev, int B, int channels,
                          const bugseg_bev_params *p, int gray, uint8_t *out_dev, void *stream);

/* contour_noise_removal (image_processing_utils.py:4-44), the clean-up of a binary road map between
 * ENET.predict_binary and create_occupancy_grid_binary: close small gaps with a k x k square, keep the
 * road regions that reach the bottom band of the image, fill their small holes, drop everything else.
 * The host arithmetic (image_processing_utils.py:6-8, 19-27, 31, 38) is done by the Python shim exactly as
 * the reference does it and arrives here as integers:
 *   k          side of the closing square, int(min(rows, cols) / 50); anchor k / 2 in both passes, taps
 *              outside the image ignored in both (cv2.morphologyEx's default border)
 *   y_top      first row of the bottom band, int(rows * (1 - 0.1))
 *   min_count  fewest band pixels of a filled contour that is kept, floor(cols * (rows - y_top) * 0.4) + 1
 * The exact semantics (regions, nesting, ring, even-odd output) are stated in DESIGN.md 6.17. */
typedef struct { int rows, cols, k, y_top, min_count; } bugseg_road_filter_params;

/* Bytes of the device workspace bugseg_road_filter needs for B frames (image_processing_utils.py:4-44 keeps
 * its intermediates in host arrays: closed, cnt_map, masked): 17 bytes per pixel plus alignment; 0 for
 * parameters the call would refuse for their shape. */
size_t bugseg_road_filter_workspace_bytes(const bugseg_road_filter_params *p, int B);

/* image_processing_utils.py:4-44 over a batch: seg_dev (B, rows, cols) u8, any non-zero value is road
 * -> out_dev (B, rows, cols) u8 in {0, 1}. out_dev must not overlap seg_dev. The workspace is caller-owned
 * and used only by the work this call enqueues on `stream` (as bugseg_bev_occgrid_ws: the caller's
 * allocator orders its reuse); its prior contents do not matter. A fixed sequence of eight launches; the
 * call never synchronises, needs no weights and no tables, and may be captured into a graph on its first
 * call. BUGSEG_EINVAL: B < 1 (or above 65535, the launch grid's limit), k outside [1, 64], y_top outside
 * [0, rows), min_count < 1, rows * cols too large for an int32 pixel index, a NULL or short workspace,
 * overlapping buffers. */
int bugseg_road_filter(bugseg_ctx *ctx, const uint8_t *seg_dev, int B, const bugseg_road_filter_params *p,
                       uint8_t *out_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* Profiling hook (bench_road_filter.py; image_processing_utils.py:4-44 has no counterpart): enqueue only
 * launches [first_op, last_op) of bugseg_road_filter's eight (last_op = -1: to the end): 0 close, 1 tile
 * labels, 2 border merge, 3 flatten, 4 counts, 5 subtree sums, 6 keep, 7 output. */
int bugseg_debug_road_filter_ops(bugseg_ctx *ctx, const uint8_t *seg_dev, int B, const bugseg_road_filter_params *p,
                                 uint8_t *out_dev, void *workspace_dev, size_t workspace_bytes, int first_op,
                                 int last_op, void *stream);

/* clahe (image_processing_utils.py:46-61), the contrast fix applied to a camera frame before
 * ENET.preprocess: BGR -> Lab (8 bit), CLAHE on L over a tiles_x x tiles_y grid (the reference: 8 x 8,
 * clip_limit 3.0), Lab -> BGR. The exact semantics (OpenCV's integer BGR -> Lab, clahe.cpp's histogram
 * clipping and float32 blend, this project's integer Lab -> BGR) are stated in DESIGN.md 6.18. */
typedef struct { int rows, cols, tiles_x, tiles_y; float clip_limit; } bugseg_clahe_params;

/* Bytes of the device workspace bugseg_clahe_bgr needs for B frames: the tile look-up tables,
 * (B, tiles_y, tiles_x, 256) u8; 0 for parameters the call would refuse for their shape. */
size_t bugseg_clahe_workspace_bytes(const bugseg_clahe_params *p, int B);

/* image_processing_utils.py:46-61 over a batch: bgr_dev (B, rows, cols, 3) u8 BGR -> out_dev, the same
 * shape. out_dev must not overlap bgr_dev. The workspace is caller-owned and used only by the work this
 * call enqueues on `stream` (as bugseg_road_filter); its prior contents do not matter. Two launches: the
 * tile look-up tables (one workgroup per frame and tile), then the per-pixel pass; no Lab image is written
 * to memory. The call never synchronises `stream` and may be captured into a graph on its first call (the
 * context's conversion tables, 34 KB, are uploaded on the context's private stream on first use).
 * BUGSEG_EINVAL, and nothing is launched: B < 1 (or above 65535, the launch grid's limit), tiles outside
 * [1, 16], a side smaller than twice its tile count (the reflected border needs the room), clip_limit not
 * positive or not finite, B * rows * cols * 3 too large for an int32 index, a NULL or short workspace,
 * overlapping buffers. */
int bugseg_clahe_bgr(bugseg_ctx *ctx, const uint8_t *bgr_dev, int B, const bugseg_clahe_params *p,
                     uint8_t *out_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* Tests and bench_clahe.py (image_processing_utils.py:46-61 has no counterpart): one stage of
 * bugseg_clahe_bgr, run by the device functions the product runs.
 *   0  BGR -> Lab: out_dev (B, rows, cols, 3) u8 Lab; no workspace
 *   1  the tile look-up tables of in_dev's frames: out_dev (B, tiles_y, tiles_x, 256) u8; no workspace
 *   2  Lab -> BGR of in_dev read as a Lab image: out_dev (B, rows, cols, 3) u8 BGR; no workspace
 *   3  launch 1 only: the look-up tables into the workspace; out_dev is not used
 *   4  launch 2 only: the look-up tables are already in the workspace */
int bugseg_debug_clahe_stage(bugseg_ctx *ctx, const uint8_t *in_dev, int B, const bugseg_clahe_params *p, int stage,
                             uint8_t *out_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* Host only, no GPU: copy out conversion table `which` as the library built it; `bytes` must be its size.
 * 0 gamma u16[256], 1 cube root u16[3072], 2 RGB -> XYZ / white i32[9] (Q12), 3 fy by L i32[256] (Q16),
 * 4 Y by L i32[256] (Q20), 5 finv over f i32[2306] (Q20), 6 XYZ -> RGB * white i32[9] (Q16),
 * 7 inverse gamma u8[16385]. */
int bugseg_debug_clahe_table(int which, void *dst, size_t bytes);

/* Canny edge detection as create_skeleton uses it (image_processing_utils.py:95-105: cv2.Canny with
 * apertureSize 3 and the L1 gradient magnitude), batched: 3 x 3 Sobel with the border replicated, |dx| + |dy|,
 * non-maximum suppression, hysteresis. low and high are the thresholds after the host's floor() and, if
 * low > high, swap (image_processing_utils.canny_params). The exact semantics are stated in DESIGN.md 6.19;
 * everything is integer arithmetic. */
typedef struct { int rows, cols, low, high; } bugseg_canny_params;

/* Bytes of the device workspace bugseg_canny needs for B frames: 5 bytes per pixel (one map byte, one
 * int32 label) plus alignment; 0 for parameters the call would refuse for their shape. */
size_t bugseg_canny_workspace_bytes(const bugseg_canny_params *p, int B);

/* img_dev (B, rows, cols) u8 -> out_dev (B, rows, cols) u8 in {0, 255}. out_dev must not overlap img_dev.
 * The workspace is caller-owned and used only by the work this call enqueues on `stream` (as
 * bugseg_road_filter); its prior contents do not matter. A fixed sequence of five launches: gradient and
 * non-maximum suppression fused (no gradient or magnitude image is written to memory), then hysteresis as
 * 8-connected component labelling (per-tile union-find, merge across tile borders, marking of the roots of
 * strong pixels, output). The call never synchronises, needs no weights and no tables, and may be captured
 * into a graph on its first call. BUGSEG_EINVAL, and nothing is launched: B < 1 (or above 65535, the launch
 * grid's limit), rows < 1 or cols < 1, B * rows * cols too large for an int32 index, a frame with 2^24 or
 * more 16 x 64 tiles (their threads pass a launch grid's 2^32 - 1; only frames thinner than a tile can
 * have that many and still fit the index: 1 x cols above 2^30 - 64, rows x 1 above 2^28 - 16), a NULL or
 * short workspace, overlapping buffers. */
int bugseg_canny(bugseg_ctx *ctx, const uint8_t *img_dev, int B, const bugseg_canny_params *p,
                 uint8_t *out_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* Tests and bench_canny.py: one half of bugseg_canny, run by the device functions the product runs; the
 * refusals are bugseg_canny's.
 *   0  launch 0 only: out_dev is the (B, rows, cols) map, 2 strong, 0 weak, 1 none
 *   1  hysteresis only: in_dev is read as such a map (any byte other than 2 and 0 is none), out_dev the edges */
int bugseg_debug_canny_stage(bugseg_ctx *ctx, const uint8_t *in_dev, int B, const bugseg_canny_params *p, int stage,
                             uint8_t *out_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* The standard Hough transform, cv2.HoughLines(image, rho, theta, threshold, min_theta, max_theta), batched.
 * The exact semantics are stated in DESIGN.md 6.21. image_processing_utils.hough_params computes the fields:
 *   numangle   floor((max_theta - min_theta) / theta) + 1, less one if the last angle would be pi again
 *   numrho     cvRound((2 (cols + rows) + 1) / rho), in double with rho as stored here
 *   threshold  a cell needs more votes than this
 *   max_lines  the strongest lines stored per frame, 1..4096
 *   rho, theta, min_theta  as float32, the values every step uses
 * Limits: rows and cols 1..65535 (a pixel is packed as x | y << 16), B * rows * cols below 2^31 - 256; numrho
 * exactly the value above (the votes are indexed with it) and at most 13651 (three accumulator rows of
 * numrho + 2 int32 must fit the 160 KiB of LDS; 1080 x 1920 at rho 1 has 6001); numangle 1..65536 with
 * (numangle + 2) * (numrho + 2) below 2^31; B 1..65535. */
typedef struct {
    int rows, cols, numangle, numrho, threshold, max_lines;
    float rho, theta, min_theta;
} bugseg_hough_params;

/* Host only, no GPU: the trig table of p, 2 * numangle float32 into dst_host: (float)(cos((double)ang) * irho)
 * for every angle, then the sines likewise, with irho = 1 / rho in float32 and ang starting at min_theta and
 * growing by theta in float32. The one place these values are computed; the device reads them as they are. */
int bugseg_hough_trig(const bugseg_hough_params *p, float *dst_host);

/* Bytes of the device workspace bugseg_hough_lines needs for B frames: per frame 4 bytes per pixel (the list of
 * non-zero pixels), 8 bytes per possible peak (ceil(numangle * numrho / 2) keys) and two counters, plus alignment;
 * 0 for parameters the call would refuse. */
size_t bugseg_hough_workspace_bytes(const bugseg_hough_params *p, int B);

/* img_dev (B, rows, cols) u8, any non-zero byte is set; trig_dev the table of bugseg_hough_trig in device memory
 * -> lines_dev (B, max_lines, 2) float32 (rho, theta), strongest first (on equal votes the smaller accumulator
 * index first), zero from row counts[b] on; counts_dev (B,) int32 = min(peaks, max_lines); peaks_dev (B,) int32,
 * the peaks found. The workspace is caller-owned and used only by the work this call enqueues on `stream`; its
 * prior contents do not matter. One memset of the counters and three launches (list the non-zero pixels; vote and
 * test for peaks in LDS, the accumulator never reaches memory; select and sort). The call never synchronises,
 * allocates nothing and may be captured into a graph on its first call. BUGSEG_EINVAL, and nothing is launched: a
 * NULL argument, parameters outside the limits above, rho or theta not positive and finite, min_theta not finite,
 * max_lines outside 1..4096, a NULL or short workspace, a written buffer that overlaps another buffer. */
int bugseg_hough_lines(bugseg_ctx *ctx, const uint8_t *img_dev, int B, const bugseg_hough_params *p,
                       const float *trig_dev, float *lines_dev, int32_t *counts_dev, int32_t *peaks_dev,
                       void *workspace_dev, size_t workspace_bytes, void *stream);

/* Tests and bench_hough.py: one half of bugseg_hough_lines, run by the device functions the product runs; the
 * refusals are bugseg_hough_lines'.
 *   0  list and vote: acc_dev receives the accumulators, (B, numangle + 2, numrho + 2) int32 with a zero border
 *      (row n + 1, column r + 1 is cell (n, r)); lines_dev, counts_dev and peaks_dev are not used
 *   1  peaks, select and sort on the accumulators given in acc_dev (that shape, non-negative values; the border
 *      is read as given); img_dev and trig_dev are not used */
int bugseg_debug_hough_stage(bugseg_ctx *ctx, const uint8_t *img_dev, int B, const bugseg_hough_params *p,
                             const float *trig_dev, int stage, int32_t *acc_dev, float *lines_dev, int32_t *counts_dev,
                             int32_t *peaks_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* The calibration tile in a camera frame, batched: the largest bright (or dark) region that does
 * not touch the frame's border, its four corners, and per side the moments of the region's boundary cracks.
 * calibration.quad_params computes the fields:
 *   channels   3: frames are (rows, cols, 3) BGR bytes, turned into 8-bit grey; 1: (rows, cols) grey bytes
 *   bright     non-zero: foreground is grey > t; zero: grey <= t
 *   threshold  0..254: t; any other value: Otsu's threshold of the frame, computed on the device
 *   min_area   a region needs at least this many pixels
 *   band       the half-width in pixels of the strip along a side whose crack points the side takes:
 *              band[0] in bugseg_find_quad; band[1] is what calibration.find_tile passes to its second pass
 * Limits: rows and cols 3..4096, channels 1 or 3, B 1..65535, min_area at least 1, band 0..64. */
typedef struct { int rows, cols, channels, bright, threshold, min_area, band[2]; } bugseg_quad_params;

/* status of a frame */
#define BUGSEG_QUAD_OK 0
#define BUGSEG_QUAD_NO_TILE 1       /* one grey level, or no region off the border with min_area pixels */
#define BUGSEG_QUAD_DEGENERATE 2    /* the region has no four distinct corners that span a quadrilateral */

/* Bytes of the device workspace the calls below need for B frames: per frame 9 bytes per pixel (grey value,
 * label, counter), the histogram and the state, plus alignment; 0 for parameters the calls would refuse. */
size_t bugseg_quad_workspace_bytes(const bugseg_quad_params *p, int B);

/* frames_dev (B, rows, cols[, 3]) u8 -> per frame status, threshold (-1 for a frame of one grey level), area and
 * root (the region's pixel count and its raster-first pixel's index; 0 and -1 without a region), corners_dev
 * (B, 4, 2) int32 (x, y) in cyclic order and moments_dev (B, 4, 6) int64 (n, sum X, sum Y, sum XX, sum XY, sum YY
 * of side i, from corner i to corner i + 1, in doubled coordinates); corners and moments are zero unless the
 * status is BUGSEG_QUAD_OK. The workspace is caller-owned and used only by the work this call enqueues on
 * `stream`; its prior contents do not matter. Two memsets and twelve launches; the call never synchronises,
 * allocates nothing and may be captured into a graph on its first call. BUGSEG_EINVAL, and nothing is launched:
 * a NULL argument, parameters outside the limits above, a NULL or short workspace, moments_dev not 8-byte
 * aligned, a written buffer that overlaps another buffer. */
int bugseg_find_quad(bugseg_ctx *ctx, const uint8_t *frames_dev, int B, const bugseg_quad_params *p, int32_t *status_dev,
                     int32_t *threshold_dev, int32_t *area_dev, int32_t *root_dev, int32_t *corners_dev,
                     int64_t *moments_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* The side moments alone, for corners the caller gives: corners2_dev (B, 4, 2) int32 in doubled coordinates
 * (2 x, 2 y), cyclic. The region is found again from the frames (launches 0..5 of bugseg_find_quad), then its
 * crack points are summed with `band`. A frame without a region, and a side of zero length or with a coordinate
 * outside -16384..16384, gets zero sums. The refusals are those of bugseg_find_quad, and band outside 0..64. */
int bugseg_quad_moments(bugseg_ctx *ctx, const uint8_t *frames_dev, int B, const bugseg_quad_params *p, int band,
                        const int32_t *corners2_dev, int64_t *moments_dev, void *workspace_dev, size_t workspace_bytes,
                        void *stream);

/* Tests and bench_calibration.py: launch `stage` (0..11, the list in csrc/quad_kernels.hip) of bugseg_find_quad
 * alone, with the memset that belongs to it, on a workspace an earlier whole call has filled; the refusals are
 * those of bugseg_find_quad. */
int bugseg_debug_quad_stage(bugseg_ctx *ctx, const uint8_t *frames_dev, int B, const bugseg_quad_params *p, int stage,
                            int32_t *status_dev, int32_t *threshold_dev, int32_t *area_dev, int32_t *root_dev,
                            int32_t *corners_dev, int64_t *moments_dev, void *workspace_dev, size_t workspace_bytes,
                            void *stream);

/* The rolling local map: B occupancy grids, each taken at its own pose, fused in time order into a
 * world-aligned log-odds map that scrolls with the vehicle. Integers only on the device; mapping.LocalMap owns the
 * buffers and mapping.pose_record builds the record.
 *   map_rows, map_cols    the window, Hm x Wm cells; window cell (i, j) is world cell (wx0 + j, wy0 + i), so the
 *                         window row by row is nav_msgs/OccupancyGrid data order
 *   grid_rows, grid_cols  a grid, h x w cells (forward x left), stored (h, w) with the base point at the bottom
 *                         centre, or with ros_layout non-zero (w, h) as G[::-1, ::-1].T
 *   l_occ, l_free         what a cell of value 100 adds and a cell of value 0 takes away; any other value is no
 *                         observation
 *   l_min, l_max          the clamp; the look-up table has l_max - l_min + 1 entries
 *   cull                  non-zero: a workgroup leaves out the frames whose footprint cannot reach its tile (the
 *                         result is the same; bench_local_map.py measures both)
 * Limits: every side 1..4096, B 1..4096, -32768 < l_min < 0 < l_max <= 32767, l_occ and l_free at least 1. */
typedef struct { int map_rows, map_cols, grid_rows, grid_cols, ros_layout, l_occ, l_free, l_min, l_max, cull; } bugseg_map_params;

#define BUGSEG_MAP_UNOBSERVED (-32768)  /* the state of a cell that was never observed */
/* The update record, int64 words in device memory: a header, then one frame record per grid.
 *   header  [0] wx0, [1] wy0: the window's origin in world cells; [2], [3]: the origin the state was last written
 *           with; [4] non-zero: the map is fresh and nothing stored is kept; [5..7] zero
 *   frame   C, S, Ox, Oy: forward = (C j + S i + Ox) >> 16 and left = (-S j + C i + Oy) / 2^16 cells at window cell
 *           (i, j). C = S = 0, which no yaw gives, marks a frame without a pose: it is skipped */
#define BUGSEG_MAP_RECORD_HEADER 8
#define BUGSEG_MAP_RECORD_FRAME 4

/* grids_dev int8 (B, h, w) [or (B, w, h)] and record_dev (8 + 4 B int64 words) -> state_dev, int16 (Hm, Wm) stored as
 * a torus (world cell (X, Y) lives in slot (Y mod Hm, X mod Wm), floor-mod), and out_dev, int8 (Hm, Wm) in window
 * order: -1 for a cell never observed, else lut_dev[L - l_min]. A window cell keeps its stored state when the map
 * is not fresh and its world cell lay in the previous window, and starts unobserved otherwise, whatever the slot
 * holds: the state needs no memset. The frames are fused in the order 0..B-1 (the clamp makes the order matter).
 * One launch, no workspace; the call never synchronises, allocates nothing and may be captured into a graph, where
 * it reads whatever the record holds when the graph runs. BUGSEG_EINVAL, and nothing is launched: a NULL argument,
 * parameters outside the limits above, record_dev not 8-byte or state_dev not 2-byte aligned, a written buffer
 * that overlaps another buffer. */
int bugseg_map_fuse(bugseg_ctx *ctx, const int8_t *grids_dev, int B, const bugseg_map_params *p, const int64_t *record_dev,
                    int16_t *state_dev, const int8_t *lut_dev, int8_t *out_dev, void *stream);

/* Evaluation of class maps: the confusion matrix of predictions against labels, both u8 maps
 * in device memory. A label pixel (y, x) of a gt_rows x gt_cols label map is compared with the prediction at
 * sy = min(y * pred_rows / gt_rows, pred_rows - 1), sx = min(x * pred_cols / gt_cols, pred_cols - 1), exact
 * integer arithmetic (the identity for equal shapes). g = gt_lut[label byte], p = pred_lut[prediction byte];
 * a pixel with g >= num_classes or p >= num_classes is skipped. num_classes is 1..64. */
typedef struct {
    int pred_rows, pred_cols, gt_rows, gt_cols, num_classes;
    uint8_t pred_lut[256], gt_lut[256];
} bugseg_confusion_params;

/* pred_dev (B, pred_rows, pred_cols) u8, gt_dev (B, gt_rows, gt_cols) u8 -> acc_dev, int64[C * C + 1] with
 * C = num_classes: acc[g * C + p] += 1 per evaluated label pixel, acc[C * C] += 1 per skipped one, so one call
 * adds B * gt_rows * gt_cols in all. The accumulator is the caller's and is not zeroed; the adds are device-scope
 * 64-bit integer atomics, so the result does not depend on their order and concurrent calls may share an
 * accumulator. One launch; the call never synchronises, allocates nothing, needs no weights and may be captured
 * into a graph on its first call. The maps may start at any byte address; whole 16-byte loads are used when
 * the two start equally far from a 16-byte boundary. BUGSEG_EINVAL, and nothing is launched: a NULL argument,
 * B < 1, an empty map, num_classes outside 1..64, B * rows * cols of either map (or, for unequal shapes,
 * gt_rows * pred_rows or gt_cols * pred_cols) too large for an int32 index, acc_dev not 8-byte aligned. */
int bugseg_confusion(bugseg_ctx *ctx, const uint8_t *pred_dev, const uint8_t *gt_dev, int B,
                     const bugseg_confusion_params *p, int64_t *acc_dev, void *stream);

/* Plan introspection for the bench / roofline, for the engine-input entry (bgr_input = 0) or
 * bugseg_enet_forward_bgr (bgr_input = 1), context precision:
 *   n_launches  kernel launches of one forward;
 *   alg_bytes   the network's per-layer algorithmic traffic (every convolution reads its input and
 *               writes its output once, residual branches re-read the block input, weights once per
 *               layer) — a property of the model and shape, the SURVEY.md §8(d) definition;
 *   plan_bytes  the compulsory traffic of this plan (fused launches keep internals on chip);
 *   flops       2 x MACs. */
int bugseg_plan_info(bugseg_ctx *ctx, int B, int H, int W, int out_kind, int bgr_input, int *n_launches,
                     double *alg_bytes, double *plan_bytes, double *flops);

/* Profiling hooks (no reference counterpart): one launch of the cached plan for (B, H, W), as the
 * last forward call at those dimensions left it (its input / output buffers must still be alive).
 * bugseg_plan_op: kernel tag ("init", "conv NR<n> E<epilogue>", "bneck C<c>[ asym]") and the
 * launch's per-layer algorithmic bytes, the bytes it must move, and its flops.
 * bugseg_plan_launch_op: enqueue that one launch on `stream` (bench.py times kernels with it). In
 * the fp32 mode it reads the range words as the last forward left them (see
 * bugseg_enet_forward_bgr_ops) and max-accumulates its own output's into them. */
int bugseg_plan_op(bugseg_ctx *ctx, int B, int H, int W, int op, char *kernel, int kernel_len, double *alg_bytes,
                   double *plan_bytes, double *flops);
int bugseg_plan_launch_op(bugseg_ctx *ctx, int B, int H, int W, int op, void *stream);

/* Last error message of ctx (or of the calling thread when ctx is NULL). Never NULL. */
const char *bugseg_last_error(const bugseg_ctx *ctx);

/* Test hooks (no reference counterpart; host only: no device is touched). The weight-blob parser
 * and packer of bugseg_load_weights, and the polar-table builder of the laserscan mode, for the
 * host-sanitizer tests (tests/asan: truncated / corrupted blobs under ASan + UBSan). Errors go to
 * bugseg_last_error(NULL). */
int bugseg_debug_parse_pack(const void *blob, size_t bytes, int precision, int *ncls);
int bugseg_debug_polar_tables(int w, int h, int variant, int32_t *fmap, size_t fmap_n, int32_t *imap, size_t imap_n,
                              int *pw, int *ph);
/* Test hook (host only): the tile walk of the ENet kernels (csrc/bugseg_internal.h tile_walk) for a launch
 * of `grid` workgroups (a positive multiple of 8) over ntiles > 0 tiles, rev = 0 ascending / 1 descending.
 * Returns per = the most tiles one workgroup walks (or a negative error code) and fills, for workgroup b,
 * count[b] = its number of tiles and seq[b * per ..] = those tiles in the order it visits them, padded
 * with -1. seq holds seq_n >= grid * per words, count holds grid words. */
int bugseg_debug_tile_walk(int ntiles, int grid, int rev, int32_t *seq, size_t seq_n, int32_t *count);
/* Test hook (host only): the row windows of bugseg_enet_forward_bgr_rows for class rows [row0, row1) of an
 * H x W frame (0 <= row0 < row1 <= H), with tiles of tile_rows_c64 / tile_rows_c16 image rows in the
 * stage-4 / stage-5 bottlenecks (the device's plan picks its own). win[2k], win[2k + 1] = the half-open
 * rows op k of the last six runs, on its own grid: k = 0 up 128 -> 64 (input rows, H / 8), 1, 2 the stage-4
 * bottlenecks (output rows, H / 4), 3 up 64 -> 16 (input rows, H / 4), 4 the stage-5 bottleneck (output
 * rows, H / 2), 5 the class layer (input rows, H / 2). */
int bugseg_debug_row_windows(int H, int W, int row0, int row1, int tile_rows_c64, int tile_rows_c16, int32_t *win);
/* Test hook (host only): the walk of bugseg_enet_forward_bgr_rows on into stage 3, from the rows [y0, y1) of
 * the h-row stage-3 output that the 128 -> 64 block reads, back through n blocks: blk[5k ..] = (asymmetric,
 * dilation, row-dilated tiles, rows its full-frame launch computes per frame, image rows per tile row of its
 * windowed form) of the k-th block before the 128 -> 64 block. Returns the number m of windowed blocks (or a
 * negative error code); win[2k], win[2k + 1] = the half-open output rows block k < m runs. */
int bugseg_debug_stage3_windows(int h, int y0, int y1, int n, const int32_t *blk, int32_t *win);
/* Test hooks (tests/test_gpu_row_window_stage3.py). bugseg_debug_plan_windows: the stage-3 windows the current
 * plan runs for class rows [row0, row1): returns their number m (0: none, or the full forward) and fills
 * win[5k ..] = (plan op, first row, end row, tile variant, tiles per frame) for k < m, nearest the decoder
 * first. bugseg_debug_read_block_output: copy the output tensor of fused bottleneck launch `op` of the
 * current plan, as the last forward left it, to dst_dev (`bytes` = its size, B * H * W * C elements). */
int bugseg_debug_plan_windows(bugseg_ctx *ctx, int row0, int row1, int32_t *win);
int bugseg_debug_read_block_output(bugseg_ctx *ctx, int op, void *dst_dev, size_t bytes, void *stream);
/* Test hooks of the pair overlay (two consecutive fp32 C = 64 regular bottlenecks as one launch).
 * bugseg_debug_pair_walk (host only, no device): the overlay's walk over an n-op plan described by cand[5k ..] =
 * (candidate: a fused fp32 C = 64 regular d = 1 bottleneck outside the windowed decoder ops; grid rows; grid
 * columns; the activation buffer it reads, 0 / 1 or -1; the one it writes) and a forward over ops [first_op,
 * last_op). Returns the number of pairs and fills out[2k] = what op k does (0 its plain launch, 1 the paired
 * launch of ops k and k + 1, 2 nothing: it ran within op k - 1, 3 / 4 the first / second half of a pair the op
 * range cuts: plain launches through the spare buffer) and out[2k + 1] = 1 when the op's tensors live in the
 * other activation buffer than the plan says. bugseg_debug_pair_plan: the pairs of the current plan, rows[8k ..] =
 * (first op, tile rows, tile columns, tiles_y, tiles_x, threads, LDS bytes, flip of the first op) for k < cap;
 * returns their number (0: none — another precision, BUGSEG_NO_FUSE, a forced C = 64 tile variant). */
int bugseg_debug_pair_walk(int n, const int32_t *cand, int first_op, int last_op, int32_t *out);
int bugseg_debug_pair_plan(bugseg_ctx *ctx, int32_t *rows, int cap);
/* Test hook (tests/test_gpu_row_window.py): fill the activation arena and the pooling-index tensors of the
 * current plan with `byte`, on `stream`, so that a launch reading a row its producer did not write this
 * forward sees the fill and not a correct row left by an earlier one. */
int bugseg_debug_poison_arena(bugseg_ctx *ctx, int byte, void *stream);
/* Test hook: a context fact. what = 0: the fused initial block normalises bytes with the exact affine
 * form (bf16 / fp16; 0 = the table), 1: fp32 range scaling switched off (BUGSEG_F32_RANGE=0 at creation),
 * 2: the weights' exponent of packed convolution `arg` (fp32 range scaling; -1000 if no such conv).
 * Returns -1 for an unknown `what` or a NULL ctx. */
int bugseg_debug_ctx_info(const bugseg_ctx *ctx, int what, int arg);
/* The BUGSEG_* run-time knobs (environment variables; DESIGN.md lists them) are read once, when a context is
 * created, and held there: nothing after bugseg_create / bugseg_dl_create reads the environment. A value outside
 * a knob's rule (a boolean: 0 or 1; an integer: a decimal in the knob's range) makes the create call fail with
 * BUGSEG_EINVAL, last_error(NULL) naming the variable and the value.
 * Test hook: one NAME=value line per knob into buf[len], NUL-terminated: the values ctx holds, or with a NULL
 * ctx those of the environment as it is now (host only). BUGSEG_EINVAL: a bad value, or buf too small. */
int bugseg_debug_knobs(const bugseg_ctx *ctx, char *buf, int len);
/* Test hook (host only): the built forms of the fused ENet bottleneck and upsampling kernels,
 * one row of 16 words each into rows[0 .. n_rows * 16): kind (0 bottleneck, 1 upsampling), precision, C (the
 * block's output channels), asymmetric, tile variant, transposed, cin (the down form's / the up block's input
 * channels, else 0), row-windowed, class-LUT kind (-1: no class fusion), threads per workgroup, dynamic LDS
 * bytes, tile rows, tile columns, waves, row-dilated, residual kept in registers. Returns the number of forms
 * (rows beyond n_rows are not written), or BUGSEG_EINVAL for a NULL rows with n_rows > 0. */
int bugseg_debug_fused_forms(int32_t *rows, int n_rows);
/* Measurement hook (bench.py's in-step kernel table): arm launch spans. spans = device memory of
 * 512 x uint64 per plan op for n_ops ops (NULL disarms): 64 slots 64 B apart, slot k = [k*8] entry,
 * [k*8+1] exit; every later launch of op i < n_ops folds the constant 100 MHz GPU clock into the slots
 * of op i (workgroup w into slot w % 64: min at entry, max at exit) — the caller sets entries to
 * UINT64_MAX and exits to 0 before the run it reads and takes the min / max over the slots. Ops at or
 * beyond n_ops (a plan of another shape) are never armed. Launches already captured keep their slots. */
int bugseg_debug_set_spans(bugseg_ctx *ctx, void *spans, int n_ops);
/* Test hook (tests/test_gpu_range.py): copy the pooling indices the last forward at (B, H, W) wrote for
 * downsampling block `block` (index into the block list) to device memory dst, on `stream`: u8 NHWC
 * (B, h, w, idx_cs), one byte per channel = the window position 2*dy + dx of the first maximum
 * (MaxPoolWithArgmax, models.py:43-44 inside enet.pb). bytes must equal the tensor's size. */
int bugseg_debug_pool_indices(bugseg_ctx *ctx, int B, int H, int W, int block, void *dst, size_t bytes, int *idx_cs,
                              void *stream);

/* ---- DeepLabV3 (BASELINE config 4) -------------------------------------
 * Replaces DeepLabV3 (models.py:98-136): tf.compat.v1.Session + GraphDef import (models.py:105-113)
 * and sess.run("ImageTensor:0" u8 -> "SemanticPredictions:0" int64) (models.py:115-125).
 * The graph builder is host code (deeplab_spec.py): it folds batch-norm, packs the weights into
 * one blob (bugseg_dl_load_weights) and lowers the network to a flat op list over numbered
 * activation buffers for one batch size and crop (bugseg_dl_set_plan). Op records are
 * BUGSEG_DL_OP_FIELDS int32 each: the kind, then that kind's fields in the order of
 * deeplab_spec.OP_LAYOUT (the executor's copy of the table is csrc/deeplab_ops.h, and
 * bugseg_dl_debug_op_layout reports it); unused trailing fields are 0. A plan is validated against
 * the buffers and the blob before it is accepted. */
#define BUGSEG_DL_OP_FIELDS 32
typedef struct bugseg_dl bugseg_dl;

int bugseg_dl_create(int device, int precision, bugseg_dl **out);
int bugseg_dl_destroy(bugseg_dl *dl);
/* weight blob in HOST memory (bf16 / f32 per the precision, as packed by deeplab_spec.pack). Loading
 * drops the current plan (its offsets belong to the old blob). If the upload fails (ENOMEM / EHIP) the
 * context holds no weights and no plan, as when it was created. */
int bugseg_dl_load_weights(bugseg_dl *dl, const void *blob, size_t bytes);
/* ops: nops * BUGSEG_DL_OP_FIELDS int32; buf_bytes[nbufs]: arena layout; B frames of at most
 * Hc x Wc (the crop size: 513 for the standard export). A plan that fails validation (EINVAL) leaves
 * the current plan in force. A valid one replaces it whole, the last forward's logits and I/O with
 * it; if its arena cannot be allocated (ENOMEM) the context is left with no plan: every forward is
 * ESTATE until a set_plan succeeds. Memory a captured graph reads (the arena and weights of a forward,
 * classes_from_logits or launch_op issued on a capturing stream) is kept until bugseg_dl_destroy when
 * it is replaced, so such a graph stays replayable across set_plan and load_weights. */
int bugseg_dl_set_plan(bugseg_dl *dl, const int32_t *ops, int nops, const uint64_t *buf_bytes, int nbufs,
                       int B, int Hc, int Wc);
/* rgb_dev: (B, H, W, 3) u8 RGB, H <= Hc, W <= Wc (padded with the mean pixel to the crop, as the
 * export's preprocessing does); out_dev: (B, H, W) int64 class ids. */
int bugseg_dl_forward(bugseg_dl *dl, const uint8_t *rgb_dev, int B, int H, int W, int64_t *out_dev, void *stream);
/* The u8 class-map form of the forward, for the occupancy pipeline (the int64 map of bugseg_dl_forward
 * remapped to the rasteriser's classes costs 9 bytes per pixel written and 8 read again for one byte).
 *
 * bugseg_dl_set_class_lut: the byte the u8 form stores for each class id: lut[0 .. n) in HOST memory,
 * n = the plan's class count, at most 256; lut == NULL restores the identity. The table is copied to
 * device memory the context owns when it is set (the call synchronises the device: not inside a stream
 * capture), never per forward. n is checked against the current plan here and again at every u8
 * forward, so a plan with another class count is never run with a stale table (EINVAL). */
int bugseg_dl_set_class_lut(bugseg_dl *dl, const uint8_t *lut, int n);
/* The whole plan with the final op in the u8 form: img_dev (B, H, W, 3) u8 in R, G, B byte order
 * (bgr = 0) or B, G, R (bgr = 1: channel c reads byte 2 - c, so a BGR frame gives the activations of
 * its RGB flip bit for bit); seg_dev (B, H, W) u8, lut[argmax] with the int64 form's lerp chain and
 * first-maximum tie rule. Only output rows [row0, row1) of every frame are stored ([0, H): the whole
 * map); no other byte of seg_dev is written. An empty window or one leaving [0, H): EINVAL. */
int bugseg_dl_forward_classes(bugseg_dl *dl, const uint8_t *img_dev, int bgr, int B, int H, int W, uint8_t *seg_dev,
                              int row0, int row1, void *stream);
/* Only the final op, u8 form, on the logits the last forward of this plan (either form) left in the
 * arena: rows [row0, row1) of the class map of that forward's frames, which must have been B x H x W.
 * ESTATE before any forward of the current plan. Completes a windowed map without a second forward. */
int bugseg_dl_classes_from_logits(bugseg_dl *dl, int B, int H, int W, uint8_t *seg_dev, int row0, int row1,
                                  void *stream);
/* Profiling hook: enqueue op `op` of the plan alone, on the last forward's I/O buffers. */
int bugseg_dl_launch_op(bugseg_dl *dl, int op, void *stream);
/* Test hook: copy `bytes` of activation buffer `buf` (deeplab_spec.lower's numbering; 7 = the f32
 * logits at the backbone resolution) to a device pointer, on `stream`. */
int bugseg_dl_read_buffer(bugseg_dl *dl, int buf, void *dst_dev, size_t bytes, void *stream);
const char *bugseg_dl_last_error(const bugseg_dl *dl);
/* Test hook: bugseg_debug_knobs for a DeepLab context (NULL: the environment now; errors to
 * bugseg_dl_last_error(NULL)). */
int bugseg_dl_debug_knobs(const bugseg_dl *dl, char *buf, int len);
/* Test hook (host only): the plan validation of bugseg_dl_set_plan against a weight blob of w_bytes;
 * errors go to bugseg_dl_last_error(NULL). */
int bugseg_dl_debug_check_plan(const int32_t *ops, int nops, const uint64_t *buf_bytes, int nbufs, int B, int Hc, int Wc,
                               int precision, size_t w_bytes);
/* Test hook (host only): the comma-separated names of the fields that follow the kind in a record of
 * `kind`, NUL-terminated in buf[len] -> their count; EINVAL for an unknown kind or a short buffer. */
int bugseg_dl_debug_op_layout(int kind, char *buf, int len);
/* Test hook (host only): len[i] = the number of consecutive CONV ops from op i that a forward issues as
 * one launch (1: alone; the members after the first report 1). Only groups: nothing is validated. */
int bugseg_dl_debug_plan_groups(const int32_t *ops, int nops, int32_t *len);

#ifdef __cplusplus
}
#endif
#endif /* BUGSEG_H */
