/*
 * lpf.h -- C ABI of the MI355X LiDAR projection + instance point-filter library
 * (liblpf.so, built from lidar_object_detection_amd/csrc/).
 *
 * The reference (KaranSankla/Lidar_Object_Detection) has no FFI: its hot path is a
 * run of inline NumPy statements and small Python functions inside each script's
 * frame loop.  This header is the narrowest data cut that contains that path; each
 * entry point names the reference statements it replaces (paths relative to
 * /root/reference/Coding_testes).  INTEGRATION.md shows the ctypes stub a reference
 * maintainer would add.
 *
 * Conventions
 *   - plain C, caller-owned buffers, no exceptions: every call returns LPF_OK (0) or
 *     a negative lpf_status; lpf_last_error() gives the text.
 *   - a context is bound to one GPU and one HIP stream; it is not thread-safe.
 *     One context per GPU / rank.
 *   - "on_device" flags say whether the pointers of that call are device (HBM)
 *     pointers.  With device outputs lpf_run* only enqueues work on the context's
 *     stream and returns; call lpf_sync() (or synchronise the stream you attached
 *     with lpf_set_stream) before reading.  With host pointers the call stages
 *     through internal HBM buffers and is synchronous.
 *   - a batch is F frames that share the camera; points of all frames are
 *     concatenated, frame f owns points [frame_off[f], frame_off[f+1]).
 */
#ifndef LPF_H
#define LPF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LPF_MAX_MASKS 32          /* instances per frame: one bit each in label_bits */
#define LPF_ABI_VERSION 8          /* 2: lpf_outputs gained uv_valid / label_valid
                                      3: lpf_set_stream(ctx, NULL) is the null stream (was: an internal stream -> lpf_use_own_stream);
                                         lpf_set_pipelined modes; stale graphs are refused
                                      4: on_device = 2 (lent masks) in lpf_set_masks_*; lpf_set_pipelined(4)
                                      5: boxes per run in the software-pipelined modes (a ring of box sets, their preparation rides in
                                         the run's launch; on_device = 2 = lent corners in lpf_set_boxes_ex / lpf_set_boxes_cam0);
                                         geometry tables per run (a new batch shape no longer drains the pipeline);
                                         lpf_set_pipelined modes 1 / 3 and lpf_set_cu_partition removed (measured slower, DESIGN.md
                                         section 8); lpf_set_geometry only in lab builds (-DLPF_LAB), as are
                                         lpf_lab_set_range_limits and lpf_lab_last_ranges
                                      6: lpf_set_mask_rects, lpf_resize_masks_u8 (added; nothing else changed)
                                      7: lpf_build_id, lpf_host_alloc / lpf_host_free, lpf_run_frame, lpf_erode_masks_u8 (added; nothing else changed)
                                      8: lpf_reader_submit_frame, lpf_reader_boxes, lpf_parse_boxes_json (added); lpf_resize_masks_u8 no longer
                                         refuses an exact halving (it is cv2.resize's INTER_AREA case)
                                      8 (continued): LPF_MAX_MASKS_WIDE, lpf_wide_input, lpf_wide_outputs, lpf_run_wide (added; nothing
                                         else changed)
                                      8 (continued): LPF_MAX_CAMS, lpf_cam_input, lpf_run_cams (added; nothing else changed)
                                      8 (continued): lpf_run_cams_wide (added; nothing else changed)
                                      8 (continued): lpf_frame_job_wide, lpf_run_frame_wide (added; lpf_get_stats gained slot [7];
                                         nothing else changed)
                                      8 (continued): lpf_depth_maps_outputs, lpf_depth_maps (added; nothing else changed)
                                      8 (continued): lpf_depth_overlay_input, lpf_depth_overlay_outputs, lpf_depth_overlays (added;
                                         nothing else changed)
                                      8 (continued): lpf_match2d_input, lpf_match2d_outputs, lpf_match_2d (added; nothing else changed)
                                      8 (continued): lpf_inside_input, lpf_inside_outputs, lpf_inside_masks (added; nothing else changed)
                                      8 (continued): lpf_set_erosion_element (added; nothing else changed)
                                      8 (continued): lpf_box_points_input, lpf_box_points_outputs, lpf_box_points (added; nothing else
                                         changed)
                                      8 (continued): lpf_box_views_input, lpf_box_views_outputs, lpf_box_views (added; nothing else
                                         changed)
                                      8 (continued): LPF_ASSIGN_MAX, lpf_assign_input, lpf_assign_outputs, lpf_assign_costs,
                                         lpf_assign2d_params, lpf_assign2d_outputs, lpf_assign_2d (added; nothing else changed)
                                      8 (continued): lpf_first_match_input, lpf_first_match_outputs, lpf_first_match (added; nothing else
                                         changed)
                                      8 (continued): lpf_rle_masks, lpf_set_masks_rle (added; nothing else changed)
                                      8 (continued): lpf_depth_maps_rle, lpf_first_match_rle_input, lpf_first_match_rle (added; nothing else
                                      changed)
                                      8 (continued): LPF_MASKS_U8 / _F32 / _RLE name lpf_wide_input.f32's values; 2 is new (no symbol, no
                                         layout change; any other value is now refused)
                                      8 (continued): LPF_ID_NONE, lpf_id_masks, lpf_set_masks_ids, lpf_run_wide_ids (added; nothing else
                                         changed) */
#define LPF_MAX_MASKS_WIDE 256    /* masks per frame of lpf_run_wide: LW = ceil(M / 32) label words per point */
#define LPF_MAX_CAMS 4            /* cameras of one lpf_run_cams / lpf_run_cams_wide pass */

typedef enum lpf_status {
    LPF_OK = 0,
    LPF_ERR_ARG = -1,             /* bad argument (null, negative, M > 32, ...) */
    LPF_ERR_HIP = -2,             /* a HIP runtime call failed */
    LPF_ERR_STATE = -3,           /* camera / masks / boxes not set for this call */
    LPF_ERR_NOMEM = -4,           /* device or host allocation failed */
    LPF_ERR_IO = -5               /* a scan file is missing, truncated or not [N][4] float32 (lpf_reader_*) */
} lpf_status;

typedef struct lpf_ctx lpf_ctx;

/* Per-frame scalar results (host or device memory, see lpf_outputs.on_device). */
typedef struct lpf_frame_summary {
    int64_t n_valid;                        /* len(valid_indices), V3:585 */
    int64_t n_labelled;                     /* points in >=1 mask == bg_assigned.sum(), V4:290-298 */
    int64_t inst_count[LPF_MAX_MASKS];      /* len(car_point_sets[m]), V3:227-231 */
    int64_t inst_off[LPF_MAX_MASKS + 1];    /* list m = inst_idx[inst_off[m] .. inst_off[m+1]) */
    int64_t best_cnt[LPF_MAX_MASKS];        /* best_match_count, V3:353-376 (0 if none) */
    int32_t best_box[LPF_MAX_MASKS];        /* best_bbox_idx into the frame's box list, -1 if none */
    int32_t inst_overflow;                  /* 1 if sum(inst_count) > inst_cap: lists truncated */
    int32_t reserved;
} lpf_frame_summary;

/* Output buffers of lpf_run / lpf_run_batch.  Any pointer may be NULL (not wanted).
 * Ntot = frame_off[F]; Btot = total boxes over the batch. */
typedef struct lpf_outputs {
    int32_t  *uv;          /* [Ntot][2]  (u, v) = np.round(x/|z|), np.round(y/|z|)  (V3:568-569),
                              saturated to int32 (only ever differs from the reference's int64
                              for |pixel| >= 2^31, which is never a valid point) */
    uint32_t *label_bits;  /* [Ntot]     bit m set <=> point valid and inside mask m (V3:225); 0 if !valid */
    double   *depth;       /* [Ntot]     signed depth incl. the 0 -> -1e-6 patch (cam2image) */
    double   *u_f;         /* [Ntot]     x/|z| before rounding */
    double   *v_f;         /* [Ntot]     y/|z| before rounding */
    int64_t  *valid_idx;   /* [Ntot]     frame f's np.where(valid)[0] at valid_idx[frame_off[f] ...],
                                          indices relative to the frame, ascending (V3:585) */
    int64_t  *inst_idx;    /* [F][inst_cap]  per frame: instance lists, concatenated in mask order,
                                          each ascending (== valid_indices[mask_indices], V3:225-228) */
    int64_t   inst_cap;    /*            capacity per frame of inst_idx (entries) */
    int32_t  *count_mb;    /* [M * Btot] frame f's [M][B_f] block at M*box_off[f]:
                                          np.sum(oriented_point_in_bbox(car_points_m, box_b)), V3:366-370 */
    lpf_frame_summary *summary;  /* [F] */
    int32_t   on_device;   /* 1: all pointers in this struct are device pointers, call is asynchronous */
    int32_t   reserved;
    int32_t  *uv_valid;    /* [Ntot][2]  compact: u_valid, v_valid = u[valid], v[valid] (V3:590-591) -- frame f's at
                              uv_valid[frame_off[f] ...], in valid_idx order, n_valid entries.  Needs valid_idx too. */
    uint32_t *label_valid; /* [Ntot]     compact: label_bits[valid_indices], same order */
} lpf_outputs;

/* ---- lifetime ---------------------------------------------------------------- */
int  lpf_abi_version(void);
/* Which sources this binary was compiled from: the first 16 hex digits of the SHA-256 over csrc/ + this header + the compiler flags,
 * baked in at build time (lidar_object_detection_amd/_build.py: source_id).  The loader compares it with the sources beside it and
 * rebuilds or refuses a stale library; bench.py prints it with every number.  "unknown" for a build made without the build script. */
const char *lpf_build_id(void);
/* Page-locked host memory (hipHostMalloc) for callers that are not torch programs: results copied into it are DMA transfers, and a
 * frame loop that reuses it does not allocate per call.  NULL on failure (lpf_last_error(NULL)). */
void *lpf_host_alloc(size_t bytes);
void  lpf_host_free(void *p);
int  lpf_create(lpf_ctx **out, int device_id);
void lpf_destroy(lpf_ctx *ctx);
const char *lpf_last_error(const lpf_ctx *ctx);      /* ctx may be NULL: error of the last failed lpf_create */
/* Run on a stream the caller owns, e.g. torch.cuda.current_stream().cuda_stream.  The handle is used as it is:
 * NULL (0) is the null stream -- which is what torch's default stream is -- so device-mode calls are ordered
 * with the caller's other work on that stream and need no device-wide synchronisation.  A new context runs on an
 * internal non-blocking stream; lpf_use_own_stream() goes back to one. */
int  lpf_set_stream(lpf_ctx *ctx, void *hip_stream);
int  lpf_use_own_stream(lpf_ctx *ctx);
/* Ordering contract of device mode.  Every device pointer handed to lpf_set_masks_* / lpf_run* is read or written by
 * kernels on the context's stream(s), in the order of the calls, and by nothing else.  A context that shares the
 * caller's stream (lpf_set_stream) is ordered with the caller's work by the stream itself.  A context on its own
 * stream is NOT: inputs produced on another stream, and -- with a stream-ordered caching allocator such as torch's
 * -- even output buffers, whose memory may still be in use by kernels queued earlier on the allocating stream, need an
 * edge first.  lpf_wait_for_stream makes the context's stream wait, on the device, for everything queued so far
 * on producer; lpf_release_to_stream makes consumer wait for everything the context has queued (what the pipelined
 * modes still owe is launched first).  Neither blocks the host.  (A missing edge is how round 1's bench once
 * died inside torch's set-up gather: DESIGN.md, "The bench_s1 fault".) */
int  lpf_wait_for_stream(lpf_ctx *ctx, void *producer_stream);
int  lpf_release_to_stream(lpf_ctx *ctx, void *consumer_stream);
int  lpf_sync(lpf_ctx *ctx);
/* Software-pipelined device-mode runs.  on = 2: ONE launch per run -- the launch of run i carries its own streaming
 * kernel, the tail (index lists, box counts) of run i-1 dealt out among the streaming tiles, and the per-frame summaries of
 * run i-2; three scratch sets rotate, nothing in a launch depends on anything else in it, no second stream and no event is
 * involved.  What is still owed is launched by lpf_sync(), lpf_release_to_stream() or a call that needs the pipeline empty.
 * on = 4: as 2, and the MASK PACK rides as well, so that nothing is left on the stream between two launches: the launch
 * made by run i carries the pack of run i's masks (uint8 masks lent with on_device = 2 and no erosion; other masks are
 * packed by their own launch as before), the streaming kernel of run i-1 -- its label images were packed one launch
 * earlier -- the tail of run i-2 and the summaries of run i-3; the pack blocks come behind the streaming tiles and fill
 * their ramp-down (16 M-point step: 92 us instead of 98).  Four scratch sets rotate.  A run's POINTS are read, and its
 * outputs written, by the launch of the NEXT run (or by lpf_sync / lpf_release_to_stream): keep them untouched until then.
 * Per-run state travels with the run: the label images rotate with the scratch sets (call lpf_set_masks_* before every
 * lpf_run* while a pipelined mode is on); lpf_set_boxes* for the next run writes the next of four box sets and its table
 * set-up rides in that run's launch (boxes that are not set again stay in force); a run whose batch shape differs from the
 * previous one's brings its own frame / segment / block tables -- none of these drains the pipeline or waits for the GPU.
 * Lent inputs (on_device = 2: masks, box corners) of run i must stay unchanged until the launch after the next has been
 * queued AND has executed, i.e. until the results of run i are complete.  With a pipelined mode on, the outputs of a run are
 * complete after lpf_sync() (or lpf_release_to_stream()), not after the caller's stream alone.  0 = off (default).
 * (Modes 1 and 3 -- tail kernels / mask pack on internal side streams -- and lpf_set_cu_partition existed up to ABI 4; they
 *  measured slower than mode 2 on every workload and were removed.) */
int  lpf_set_pipelined(lpf_ctx *ctx, int on);

#ifdef LPF_LAB
/* Lab builds only (liblpf_lab.so; tools/ and the forced-geometry tests).  Launch geometry: a run cuts every frame into
 * segments -- one list wave each -- and K1 tiles: 1024-point segments of 512-point tiles for launches of up to 3.5 Mi points
 * (a real frame is then ~107 waves instead of 27), 4096-point segments of 1024-point tiles beyond; a launch of a few frames
 * runs the tail in its wide form (16 waves share the masked points of four segments).  Results do not depend on any of it.
 * 0 = by launch size (what the product always does), 1 = small with the wide tail, 2 = large, 3 = large with the segment
 * prefixes taken from the scan kernel (what frames of more than 64 x 64 segments get by themselves), 4 = small with the
 * narrow tail. */
int  lpf_set_geometry(lpf_ctx *ctx, int mode);
/* Role clock of the step launches of the software-pipelined modes: out[6][5] = per role (0 summaries, 1 box job, 2 lists, 3 box
 * counts, 4 mask pack, 5 project+label tiles) {first block start, last block end, sum of block durations, blocks, longest block}
 * in ticks of the 100 MHz wall clock, accumulated since the last reset.  The first call switches it on.  Synchronises. */
int  lpf_lab_role_clock(lpf_ctx *ctx, unsigned long long *out, int reset);
/* Range limits of the batched analysis calls (lpf_match_2d, lpf_assign_costs, lpf_assign_2d, lpf_inside_masks, lpf_box_points,
 * lpf_box_views, lpf_first_match, lpf_depth_maps, lpf_depth_overlays), so that small batches reach the second and later ranges of
 * large ones.  stage_budget_bytes replaces the staging budget of a range (256 MiB); max_items caps the items -- frames, images --
 * of every range and of every per-launch frame loop at min(the product's limit, max_items).  0 for either = the product's value.
 * Results do not depend on them. */
int  lpf_lab_set_range_limits(lpf_ctx *ctx, long long stage_budget_bytes, int max_items);
/* The ranges (chunks) the last batched analysis call planned; for lpf_inside_masks and lpf_box_points the launches of their frame
 * loop; 0 when the call returned before it planned any. */
int  lpf_lab_last_ranges(lpf_ctx *ctx);
#endif

/* ---- per-sequence state --------------------------------------------------------
 * Replaces V3:565-569 + V3:584 constants.  T = TrVeloToRect (row-major 4x4, V3:535),
 * K = camera.K[:3,:3] (row-major 3x3), W,H = camera.width/height,
 * valid <=> 0<=u<W && 0<=v<H && depth > depth_min_excl && depth < depth_max_excl
 * (reference: 0 and 50, or 0 and 30 in V4/V5). */
int lpf_set_camera(lpf_ctx *ctx, const double T_velo_to_rect[16], const double K[9],
                   int W, int H, double depth_min_excl, double depth_max_excl);

/* ---- per-frame (or per-batch) state --------------------------------------------
 * Masks of F frames, M <= 32 per frame (pad with all-zero masks), each H x W.
 * u8: nonzero = member.  f32: the reference's float masks;
 *   binarize = 0 : member <=> mask.astype(np.uint8) != 0                  (V3:222-225 on raw masks, V2/V4)
 *   binarize = 1 : (mask*255).astype(uint8) -> erode -> /255.0 -> astype(uint8) != 0   (V3:82-97 then V3:222)
 *   binarize = 2 : member <=> mask > 0.5 on the raw float mask   (Same_color.py:125, vis.py:185,
 *                  seg_with_pointcloud.py:167: the scripts that index the YOLO mask without astype)
 * erode_iters: iterations of cv2.erode with the context's erosion element: the 3x3 MORPH_ELLIPSE (the cross, V3:83-90) unless
 *   lpf_set_erosion_element has set another size.
 * The packed result is a label image [F][H][W], bit m = mask m, kept in HBM.
 * on_device: 0 = host memory (copied before the call returns); 1 = device memory, packed in stream order by this call (the
 *   buffer may be rewritten, in stream order, as soon as the call has returned); 2 = device memory LENT to the context: it
 *   stays unchanged until every run that uses these masks has completed.  Lent masks (and host masks, which sit in the
 *   context's own staging buffer) that need no erosion are not packed at the call in serial mode: a small launch (a real
 *   frame or a few) then looks a valid point's M mask values up directly -- ~20 k points x M bytes instead of a separate
 *   4.7 us launch over 530 k pixels x M -- and a large one packs them first, on the same stream.  The software-pipelined
 *   modes (lpf_set_pipelined 2 / 4) leave lent masks to the next lpf_run* in the same way: a small launch's tiles read
 *   them directly, a large one packs them (mode 4: by blocks of its own launch, see there).  Same results. */
int lpf_set_masks_u8(lpf_ctx *ctx, const uint8_t *masks, int F, int M, int erode_iters, int on_device);
/* Optional hint for the NEXT lpf_set_masks_* call with the same F and M: rects[F][M][4] = {x0, y0, x1, y1} (int32, pixels, half
 * open) -- the caller's word that mask m of frame f is zero outside its rectangle.  A detector hands out every mask with its 2D box
 * and crops the mask to it (the reference's segmenter returns them side by side, cvs_erosion.py:86-87, 110: `boxes`, `masks`); a real
 * frame's masks are a few per cent non-zero.  With the hint a mask is READ AS ZERO OUTSIDE ITS RECTANGLE, pixel for pixel, by every
 * form that takes it -- uint8 masks and float masks under binarize = 0, without erosion, image at least 16 pixels wide:
 *   - launches of sparse frames (fewer points per frame than half the image has pixels) read the lent / staged masks THEMSELVES:
 *     large launches through a per-frame candidate grid of the rectangles (16 x 16-pixel cells) and an exact test for the rows that
 *     have a candidate -- no pack, no label image, whatever the launch size; small launches (a frame or a few) read a valid point's M
 *     mask bytes and gate them by the rectangles;
 *   - dense frames' masks are packed, and the pack reads a 16-pixel group of mask m only where it meets m's rectangle.
 * A rectangle may reach beyond the image (it is read as clipped to it; INT32_MIN / INT32_MAX as "no limit" are fine), x1 <= x0 or
 * y1 <= y0 is an empty one.
 * The same results as without the hint as long as the caller's word holds; erosion and the other float rules ignore it.  on_device:
 * 0 = host memory, copied now without a wait; otherwise device memory (16-byte aligned) that stays unchanged until the runs that use
 * these masks have completed, like lent masks.  rects = NULL clears a pending hint.  The hint is consumed by the next lpf_set_masks_*. */
int lpf_set_mask_rects(lpf_ctx *ctx, const int32_t *rects, int on_device, int F, int M);
/* The erosion element of the context: cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (ksize, ksize)), the reference's
 * `erosion_kernel_size` (V3:55-97, cvs_erosion.py:77-106: image_segmentation_with_erosion(image, erosion_kernel_size=3,
 * erosion_iterations=1) builds this element and hands it to cv2.erode(mask_uint8, kernel, iterations=erosion_iterations)).
 * ksize is odd, 1 .. 15; a new context has 3.  The element, restated from OpenCV for odd k and pinned by construction only, like the
 * 3x3 erosion and the resize (OpenCV is no dependency of this project): with r = ksize / 2, row i (dy = i - r) is ones from column
 * r - dx to r + dx inclusive, dx = round_half_even(r * sqrt((r*r - dy*dy) * (1.0 / (r*r)))) in double (ksize = 1: dx = 0).  Half-widths
 * per row, shipped as a table (no quotient lies within 0.02 of a tie):
 *    3: 0 1 0  (the cross)        5: 0 2 2 2 0        7: 0 2 3 3 3 2 0        9: 0 3 3 4 4 4 3 3 0
 *   11: 0 3 4 5 5 5 5 5 4 3 0    13: 0 3 4 5 6 6 6 6 6 5 4 3 0    15: 0 4 5 6 6 7 7 7 7 7 6 6 5 4 0
 * An erosion is the minimum (on packed masks: the AND) over the element, pixels outside the image left out; several iterations repeat
 * one iteration (cv2.erode merges rectangular elements only).  ksize = 1 makes any number of iterations the identity.
 * Context state, host side only: the call enqueues nothing and waits for nothing.  From then on every erosion of the context uses it:
 * the erode_iters of lpf_set_masks_u8 / lpf_set_masks_f32 (every binarize rule), the erode_iters of a lpf_wide_input (lpf_run_wide,
 * lpf_run_cams, lpf_run_cams_wide, lpf_depth_maps) and lpf_erode_masks_u8.  Masks already packed keep the element they were packed
 * with, a captured graph the one it was captured with; lpf_set_mask_rects' contract is unchanged (no erosion).  With ksize = 3 the
 * launches are the ones of a context that never called this.  LPF_ERR_ARG (the message names the value, the element stays as it
 * was): an even size, ksize < 1, ksize > 15. */
int lpf_set_erosion_element(lpf_ctx *ctx, int ksize);
int lpf_set_masks_f32(lpf_ctx *ctx, const float *masks, int F, int M, int binarize,
                      int erode_iters, int on_device);
/* Masks of F frames in RUN-LENGTH form, from host memory, decoded on the GPU: the form instance masks are stored and exchanged in
 * (saved predictions, annotation files, a detector in another process).  A frame's masks are then a few tens of KB on their way to the
 * device where the dense form is M * H * W bytes (2.6 MB of uint8 for five masks at 1408 x 376), and the copy is what a call with host
 * masks spends its time on.
 *   Runs: mask m of frame f owns runs[run_off[f*M+m] .. run_off[f*M+m+1]); a run {start, length} is the pixels start .. start+length-1
 * of the mask image flattened row-major, pixel (x, y) = y * W + x with W, H of lpf_set_camera.  A pixel is a member of mask m iff it lies
 * in ANY run of m: the runs of a mask may come in any order and may touch or overlap; length = 0 is an empty run; a run may continue
 * across row ends.
 *   Both arrays are host memory and are checked IN FULL before anything is enqueued (there is no device-memory form, so the decode
 * never reads a list that was not checked): run_off[0] = 0, run_off non-decreasing, start >= 0, length >= 0, start + length <= W * H
 * (in 64 bits).  A violation is LPF_ERR_ARG, the message names frame, mask and run, and the context is left as it was.  They are copied
 * before the call returns -- the caller may free them at once; the call may wait for that copy, as lpf_set_masks_u8 does for host masks,
 * and waits for nothing else.
 *   Afterwards the context is in the state lpf_set_masks_u8 leaves for the equivalent dense masks (dense[f][m][p] = 1 iff member) with
 * the same erode_iters and on_device = 0, once those are packed: lpf_get_label_image is bit-for-bit equal, the label elements have the
 * same width (1 / 2 / 4 bytes for M <= 8 / 16 / 32), F and M are in force, a pending lpf_set_mask_rects hint is consumed (and ignored),
 * any record of unpacked masks is forgotten, and every later lpf_run / lpf_run_batch / lpf_run_frame (masks == NULL) gives the same
 * outputs.  The label image is zeroed and the runs are OR-ed into it (integer ORs only: the image does not depend on the order the
 * hardware takes them in); erode_iters iterations of the context's element (lpf_set_erosion_element) then run on the packed image.
 * M = 0, or no run at all, zeroes the image and launches no decode; F = 0 does what lpf_set_masks_u8 does with F = 0.  In the
 * software-pipelined modes (2 / 4) the call behaves as lpf_set_masks_u8 with host masks: what the pipeline owes is drained first, and
 * the label image goes to the set the next run reads.
 *   LPF_ERR_STATE before lpf_set_camera, and between lpf_graph_begin and lpf_graph_end (the run counts size the launch).  LPF_ERR_ARG:
 * in NULL, F < 0, M < 0, erode_iters < 0, reserved != 0, M > LPF_MAX_MASKS (lpf_set_masks_u8's message), run_off NULL with F * M > 0,
 * runs NULL with runs to read, F * M or the number of runs above 2^31 - 1, or runs that together cover more than 2^24 chunks of 1024 pixels.
 *   The passes that turn a lpf_wide_input into label bits -- lpf_run_wide, lpf_run_cams, lpf_run_cams_wide -- take this struct as their
 * masks (LPF_MASKS_RLE, at lpf_wide_input; there M goes up to the pass's own limit).  Not taken in this form: the dense inputs of lpf_run_frame_wide
 * (device masks), lpf_depth_maps and lpf_first_match -- those two have calls of their own for it, lpf_depth_maps_rle and
 * lpf_first_match_rle below -- and lpf_inside_masks' instance lists; runs are not resized (masks of another size than the camera's: decode them on
 * the host, lpf_resize_masks_u8); runs in device memory.  Masks that already sit on the GPU gain nothing from this form. */
typedef struct lpf_rle_masks {
    const int32_t *runs;     /* host, [Rtot][2] {start, length}, Rtot = run_off[F*M] */
    const int64_t *run_off;  /* host, [F*M + 1] */
    int32_t F, M;            /* 0 <= M <= LPF_MAX_MASKS (as a lpf_wide_input's masks: that pass's limit) */
    int32_t erode_iters;     /* >= 0, with the context's element (lpf_set_erosion_element) */
    int32_t reserved;        /* 0 */
} lpf_rle_masks;
int lpf_set_masks_rle(lpf_ctx *ctx, const lpf_rle_masks *in);
/* Masks of F frames as INSTANCE-ID MAPS, decoded on the GPU: one image per frame whose pixel value says which instance owns the pixel
 * -- the form panoptic ground truth is stored in (KITTI-360's 16-bit PNG files under instance/: pixel = semanticId * 1000 + instanceId) and
 * panoptic segmenters emit.  What reaches the device is the map, H * W * id_bytes per frame whatever M is (1.06 MB of uint16 at
 * 1408 x 376, where the dense form is 0.53 MB per mask), or nothing at all when the map already sits there.
 *   ids: [F][H][W] row-major at W, H of lpf_set_camera, uint16 (id_bytes 2, widened unsigned) or int32 (id_bytes 4), in host or device
 * memory per on_device, aligned to its element and no further.  sel: host memory, [F][M], each frame's own table.
 *   Membership: pixel p of frame f is in mask m iff sel[f*M+m] != LPF_ID_NONE and (int64)ids[f][p] == (int64)sel[f*M+m].  An entry
 * outside 0 .. 65535 matches no pixel of a uint16 map (65536 does not match ID 0, -1 does not match 65535); equal entries in one
 * frame's table each get their bit; LPF_ID_NONE pads frames with fewer instances and matches nothing, even in an int32 map that holds
 * INT32_MIN.  No input value is used as an index: any map and any table are valid.
 *   Afterwards the context is in the state lpf_set_masks_u8 leaves for the equivalent dense masks (dense[f][m][p] = 1 iff member) with
 * the same erode_iters and on_device = 0, once those are packed: lpf_get_label_image is bit-for-bit equal, the label elements have the
 * same width (1 / 2 / 4 bytes for M <= 8 / 16 / 32), F and M are in force, a pending lpf_set_mask_rects hint is consumed (and ignored),
 * any record of unpacked masks is forgotten, and every later lpf_run / lpf_run_batch / lpf_run_frame (masks == NULL) gives the same
 * outputs.  The masks are always packed at the call: every element of the label image is written exactly once, zeros included, from
 * one read of its pixel's ID (no zero-fill, no atomics; the image does not depend on scheduling); erode_iters iterations of the
 * context's element (lpf_set_erosion_element) then run on the packed image.  M = 0 zeroes the image and launches no decode; F = 0 does
 * what lpf_set_masks_rle does with F = 0.  In the software-pipelined modes (2 / 4) the call behaves as lpf_set_masks_rle: what the
 * pipeline owes is drained first, and the label image goes to the set the next run reads.
 *   The call returns once its host arrays are copied -- sel always, ids when on_device = 0 (it may wait for that copy, as
 * lpf_set_masks_u8 does for host masks) -- and waits for nothing else: both may be freed at once, and device ids may be rewritten in
 * stream order as soon as the call has returned.
 *   LPF_ERR_STATE before lpf_set_camera, and between lpf_graph_begin and lpf_graph_end (the table is a host copy; there is no
 * capturable form).  LPF_ERR_ARG, the message naming the field and the context left as it was: in NULL, F < 0, M < 0, erode_iters < 0,
 * id_bytes not 2 or 4, on_device not 0 or 1, reserved != 0, M > LPF_MAX_MASKS (lpf_set_masks_u8's message), ids NULL with F > 0, sel
 * NULL with F * M > 0, F * M above 2^31 - 1.
 *   lpf_run_wide_ids (below) takes the same struct with M up to LPF_MAX_MASKS_WIDE.  Not taken in this form: lpf_run_cams,
 * lpf_run_cams_wide, lpf_run_frame_wide, lpf_depth_maps, lpf_first_match, lpf_depth_overlays; maps are not resized, the IDs of a frame are
 * chosen by the caller (sel), and files are not read.  At M <= 2 a uint16 map is more bytes than the dense masks, and masks that
 * already sit dense on the GPU gain nothing from this form. */
#define LPF_ID_NONE INT32_MIN          /* a sel entry that selects nothing */
typedef struct lpf_id_masks {
    const void    *ids;        /* [F][H][W] at the camera's size, uint16 or int32 per id_bytes; host or device per on_device */
    const int32_t *sel;        /* host memory, [F][M]: mask m of frame f = the pixels whose id equals sel[f*M+m] */
    int32_t F, M;              /* 0 <= M <= LPF_MAX_MASKS (lpf_run_wide_ids: LPF_MAX_MASKS_WIDE) */
    int32_t id_bytes;          /* 2 (unsigned) or 4 (signed) */
    int32_t erode_iters;       /* >= 0, with the context's element (lpf_set_erosion_element) */
    int32_t on_device;         /* 0: ids in host memory, copied before the call returns; 1: device memory */
    int32_t reserved;          /* 0 */
} lpf_id_masks;
int lpf_set_masks_ids(lpf_ctx *ctx, const lpf_id_masks *in);
/* Pre-packed label images [F][H][W] (bit m = mask m). */
int lpf_set_label_image(lpf_ctx *ctx, const uint32_t *label, int F, int M, int on_device);
/* Read back the label images currently held ([F][H][W]); for tests of the pack/erode kernels. */
int lpf_get_label_image(lpf_ctx *ctx, uint32_t *out, int on_device);

/* Box corners in the velodyne frame, f64 [Btot][8][3] in the dataset's corner order
 * (output of transform_bboxes_to_velodyne, V3:41-52); frame f owns boxes
 * [box_off[f], box_off[f+1]).  oriented = 1: oriented_point_in_bbox (V3:167-204, the
 * three skewed slabs c1-c0, c3-c0, c4-c0); 0: point_in_bbox (V3:143-164).  box_off: host memory.
 * The box tables (slab parameters in the reference's arithmetic, float bounds, per-cell candidate lists) are built on the
 * device by one block per frame -- a kernel on the context's stream in serial mode (capturable: with unchanged box counts a
 * per-frame box change sits inside a captured graph), blocks of the next lpf_run*'s own launch in the software-pipelined
 * modes.  No call waits for the GPU unless it returns results to host memory or has to grow a buffer.
 * on_device: 0 = host memory (copied before the call returns); 1 = device memory, copied in stream order by this call (the
 * buffer may be rewritten, in stream order, as soon as the call has returned); 2 = device memory LENT to the context: read
 * when the tables are built (by the next lpf_run* in the pipelined modes), it stays unchanged until that run has completed.
 * lpf_set_camera must come first; changing W or H afterwards drops the boxes. */
int lpf_set_boxes(lpf_ctx *ctx, const double *corners_velo, const int32_t *box_off, int F, int oriented);
int lpf_set_boxes_ex(lpf_ctx *ctx, const double *corners_velo, int on_device, const int32_t *box_off, int F, int oriented);
/* The reference's per-frame box preparation and lpf_set_boxes in one device-side step (V3:556-562):
 *   corners_cam0  f64 [Btot][8][3], the 'corners_cam0' of BBoxes_<frame>.json (host or device per on_device, as above)
 *   T_cam_to_velo inv(TrVeloToCam), row-major 4x4 (host)
 *   filter_visible = 1: boxes that filter_visible_bboxes (V3:121-140) drops stay in the tables at their position but can
 *                  never be hit: count_mb keeps one column per GIVEN box (zero for a dropped one) and best_box indexes the
 *                  given list; the position in the reference's filtered list is the number of kept boxes before it.
 * Optional outputs (NULL = not wanted; host or device like the input): visible[Btot] (1 = kept), corners_velo
 * [Btot][8][3] (transform_bboxes_to_velodyne, V3:41-52), bbox2d [Btot][4] and front [Btot] as lpf_prepare_boxes.  Host outputs
 * are filled when the call returns (it waits for them); device outputs are written when the tables are built -- in the
 * pipelined modes by the launch of the next lpf_run*, or by lpf_sync / lpf_release_to_stream if that comes first. */
int lpf_set_boxes_cam0(lpf_ctx *ctx, const double *corners_cam0, int on_device, const int32_t *box_off, int F,
                       const double T_cam_to_velo[16], int filter_visible, int oriented,
                       uint8_t *visible, double *corners_velo, double *bbox2d, int32_t *front);

/* ---- the hot path ----------------------------------------------------------------
 * Replaces, per frame: V3:565-569 (transform + cam2image), V3:584-592 (clip, np.where),
 * extract_car_points_by_mask (V3:211-233), the oriented_point_in_bbox counting loop and
 * best-box scan of calculate_car_point_statistics (V3:344-379).
 * pts: f32 [Ntot][4] (x, y, z, reflectance) exactly as read from the .bin (V3:28). */
int lpf_run(lpf_ctx *ctx, const float *pts, int64_t N, int pts_on_device, const lpf_outputs *out);
int lpf_run_batch(lpf_ctx *ctx, const float *pts, const int64_t *frame_off, int F,
                  int pts_on_device, const lpf_outputs *out);

/* One frame of a stream in ONE call (one FFI crossing instead of four): what a frame of the reference's loop brings -- its scan, its
 * detection masks with their 2D boxes, its annotated 3D boxes (V3:545-562) -- and where its results go.  Exactly the sequence
 *   lpf_set_mask_rects(ctx, mask_rects, 1, 1, n_masks)                  if mask_rects
 *   lpf_set_masks_u8(ctx, masks, 1, n_masks, 0, 2)                      if masks        (lent: on_device = 2)
 *   lpf_set_boxes_cam0(ctx, corners_cam0, 2, {0, n_boxes}, 1, T_cam_to_velo, filter_visible, oriented, 0, 0, 0, 0)   if corners_cam0
 *   lpf_run(ctx, pts, n_points, 1, &out)
 * with the same meaning, ownership and error behaviour; a NULL masks / corners_cam0 leaves the masks / boxes in force as they are.
 * Every pointer except T_cam_to_velo is device memory; out.on_device must be 1.  For launch-bound frame loops: in a software-
 * pipelined stream of single real frames the three calls took the host 7.9 us per frame against 9.2 us on the GPU. */
typedef struct lpf_frame_job {
    const float   *pts;            /* [n_points][4] */
    int64_t        n_points;
    const uint8_t *masks;          /* [n_masks][H][W], lent; or NULL */
    const int32_t *mask_rects;     /* [n_masks][4] {x0, y0, x1, y1}, lent like the masks; or NULL */
    const double  *corners_cam0;   /* [n_boxes][8][3], lent; or NULL */
    const double  *T_cam_to_velo;  /* host memory, row-major 4x4 (with corners_cam0) */
    int32_t        n_masks, n_boxes;
    int32_t        filter_visible, oriented;
    lpf_outputs    out;
} lpf_frame_job;
int lpf_run_frame(lpf_ctx *ctx, const lpf_frame_job *job);

/* ---- frames with more than 32 masks ------------------------------------------------------------------------------------
 * lpf_run_wide: a batch of F frames with M masks each, 0 <= M <= LPF_MAX_MASKS_WIDE, in ONE pass: every point is projected and read
 * once, however many masks the frame has (the reference applies every detection mask of a frame, with no limit: V3:220,
 * cvs_erosion.py:148-162).  A point's membership is LW = ceil(M / 32) label words: word w, bit b <=> mask 32 w + b.  Every result is
 * the one the narrow calls give when the frame is run once per group of 32 masks (group w -> word w), concatenated.
 * Masks, rectangles and erosion come with the call; the boxes are the ones in force (lpf_set_boxes*), the camera and depth window the
 * ones of lpf_set_camera.  It leaves the masks, boxes and rectangles of the narrow calls as they were.  Not capturable (LPF_ERR_STATE
 * between lpf_graph_begin and lpf_graph_end); with a software-pipelined mode on it first launches what the pipeline owes (no host
 * wait), then runs in order.  With device outputs the call only enqueues work; with host outputs it returns with them filled. */
/* The forms of a lpf_wide_input's masks (its `f32` field).
 *   LPF_MASKS_RLE: `masks` points to ONE lpf_rle_masks in host memory (its runs and run_off in host memory, as for lpf_set_masks_rle),
 * whose F is the call's F, whose M is the input's M, whose erode_iters is the input's erode_iters and whose reserved is 0; on_device must
 * be 0; rects and binarize are not read.  Pixel p of a run is y * W + x in the image the masks belong to: the context's (lpf_set_camera)
 * for lpf_run_wide, cams[c].W, H for lpf_run_cams / lpf_run_cams_wide.  The runs are checked IN FULL on the host -- lpf_set_masks_rle's
 * rules, limits and 64-bit sums, per camera against that camera's W * H -- before anything is enqueued for the call; a violation is
 * LPF_ERR_ARG and the message names the call, the camera of a camera pass, and frame, mask and run.  The call waits for the copies of
 * its tables before it returns (as it does for host masks): the caller may free the arrays at once.  Every output is bit for bit what
 * the same call gives for the equivalent dense uint8 host masks (dense[f][m][p] = 1 iff p lies in any run of mask m) with the same
 * erode_iters; the narrow state (masks, label image, rectangles, boxes) is left as it was.  The planes are zeroed, the runs are OR-ed
 * into them on the GPU (integer ORs only) and every erosion iteration runs on the packed planes: no dense mask exists anywhere.
 *   Taken by lpf_run_wide, lpf_run_cams and lpf_run_cams_wide.  lpf_depth_maps refuses it in its lpf_wide_input (LPF_ERR_ARG, before masks
 * is read), as every call refuses an f32 other than these three -- run-length masks go to lpf_depth_maps_rle, and to lpf_first_match_rle
 * for lpf_first_match, whose input refuses the value too; lpf_run_frame_wide's job has no such field: its masks are uint8 device memory. */
#define LPF_MASKS_U8  0
#define LPF_MASKS_F32 1
#define LPF_MASKS_RLE 2
typedef struct lpf_wide_input {
    const void    *masks;          /* [F][M][H][W]: uint8 (nonzero = member) or float32 under `binarize` (lpf_set_masks_f32's rules);
                                      LPF_MASKS_RLE: one lpf_rle_masks (host memory) */
    const int32_t *rects;          /* optional [F][M][4] {x0, y0, x1, y1}: lpf_set_mask_rects' contract (uint8, or float32 with
                                      binarize 0, and no erosion; ignored otherwise); in the same memory as the masks; or NULL */
    int32_t  M;
    int32_t  f32;                  /* LPF_MASKS_U8 0: uint8 masks, LPF_MASKS_F32 1: float32, LPF_MASKS_RLE 2: run-length (above) */
    int32_t  binarize;             /* float32 masks: 0 / 1 / 2 as lpf_set_masks_f32 */
    int32_t  erode_iters;          /* cv2.erode iterations with the context's element (lpf_set_erosion_element; the cross by default), >= 0 */
    int32_t  on_device;            /* 0: masks (and rects) in host memory, copied by the call; else device memory lent until the
                                      run has completed (as on_device = 2 of lpf_set_masks_*) */
    int32_t  reserved;
} lpf_wide_input;

/* Outputs of lpf_run_wide.  Any pointer may be NULL (not wanted); all are host or all device memory per on_device.
 * Ntot = frame_off[F], Btot = boxes in force over the batch, LW = ceil(M / 32). */
typedef struct lpf_wide_outputs {
    int32_t  *uv;                  /* [Ntot][2]   as lpf_outputs */
    double   *depth, *u_f, *v_f;   /* [Ntot]      as lpf_outputs */
    int64_t  *valid_idx;           /* [Ntot]      as lpf_outputs */
    int32_t  *uv_valid;            /* [Ntot][2]   as lpf_outputs */
    uint32_t *label_words;         /* [Ntot][LW]  bit b of word w <=> point valid and inside mask 32 w + b */
    uint32_t *label_valid_words;   /* [Ntot][LW]  compact, in valid_idx order (frame f's at frame_off[f]) */
    int64_t  *inst_idx;            /* [F][inst_cap] per frame: the M instance lists in mask order, each ascending */
    int64_t   inst_cap;
    int32_t  *count_mb;            /* [M * Btot]  frame f's [M][B_f] block at M * box_off[f] */
    int64_t  *n_valid;             /* [F] */
    int64_t  *n_labelled;          /* [F]         points in >= 1 mask */
    int64_t  *inst_count;          /* [F][M] */
    int64_t  *inst_off;            /* [F][M + 1]  list m of frame f = inst_idx[f][inst_off[f][m] .. inst_off[f][m + 1]) */
    int64_t  *best_cnt;            /* [F][M]      0 if none */
    int32_t  *best_box;            /* [F][M]      first strict maximum into the frame's boxes, -1 if none */
    int32_t  *inst_overflow;       /* [F]         1 if the frame's lists exceed inst_cap (truncated) */
    int32_t   on_device;
    int32_t   reserved;
} lpf_wide_outputs;
int lpf_run_wide(lpf_ctx *ctx, const float *pts, const int64_t *frame_off, int F, int pts_on_device, const lpf_wide_input *in,
                 const lpf_wide_outputs *out);
/* lpf_run_wide with its label planes built from instance-ID maps (lpf_id_masks above: in->F == F, 0 <= in->M <= LPF_MAX_MASKS_WIDE,
 * in->erode_iters with the context's element): every output is bit for bit what lpf_run_wide gives for the equivalent dense uint8 host
 * masks (dense[f][m][p] = 1 iff member) with the same erode_iters.  All F * ceil(M / 32) * H * W plane words are written once each from
 * one read of the pixel's ID, the bits at or above M zero; no dense mask exists anywhere.  The struct is checked by
 * lpf_set_masks_ids' rules before anything is enqueued and before a pipelined context launches what it owes (LPF_ERR_ARG,
 * "run_wide_ids: ..."; M above LPF_MAX_MASKS_WIDE and in->F != F among them); everything else -- points, frame_off, outputs, boxes, the
 * state errors -- is lpf_run_wide's.  The context's narrow masks, rectangles and label image are left as they were.  sel is copied
 * before the call returns; host ids are copied by the call (it waits for that copy), device ids are lent until the run has
 * completed, like a lpf_wide_input with on_device != 0: with device points, ids and outputs the call waits for nothing on the GPU. */
int lpf_run_wide_ids(lpf_ctx *ctx, const float *pts, const int64_t *frame_off, int F, int pts_on_device,
                     const lpf_id_masks *in, const lpf_wide_outputs *out);

/* One frame of a stream with 0 .. LPF_MAX_MASKS_WIDE masks in ONE call: lpf_run_frame's job for frames with more than 32 masks (crowded
 * frames of KITTI-360 have hundreds of annotated boxes; the reference applies every mask of a frame, V3:220).  Exactly the sequence
 *   lpf_set_boxes_cam0(ctx, corners_cam0, 2, {0, n_boxes}, 1, T_cam_to_velo, filter_visible, oriented, 0, 0, 0, 0)   if corners_cam0
 *   lpf_run_wide(ctx, pts, {0, n_points}, 1, 1, &{masks, mask_rects, n_masks, f32 0, binarize 0, erode_iters 0, on_device 2}, &out)
 * with the same results, bit for bit, ownership and error behaviour: a NULL corners_cam0 leaves the boxes in force as they are; the
 * masks, rectangles and label state of the narrow calls are left as they were.  Every pointer except T_cam_to_velo is device memory and
 * lent until the frame's work has completed; out.on_device must be 1, and the call only enqueues work.  Not capturable (LPF_ERR_STATE
 * between lpf_graph_begin and lpf_graph_end); with a software-pipelined mode on it first launches what the pipeline owes (no host wait),
 * then runs in order.  LPF_ERR_ARG: a NULL job, n_masks < 0 or > LPF_MAX_MASKS_WIDE, masks NULL with n_masks > 0, n_boxes < 0,
 * out.on_device != 1.
 * A sparse frame (2 * n_points <= W * H: a real scan) with mask_rects (16-byte aligned) and 1 .. 48 masks reads its masks where its
 * valid points fall, inside their rectangles, instead of packing them into ceil(n_masks / 32) full-image planes first (lpf_get_stats
 * [7] counts such jobs); any other job runs lpf_run_wide's pack (with more masks the pack was measured faster).
 * The results are the same either way. */
typedef struct lpf_frame_job_wide {
    const float   *pts;            /* [n_points][4] */
    int64_t        n_points;
    const uint8_t *masks;          /* [n_masks][H][W] uint8, nonzero = member, lent; NULL only with n_masks == 0 */
    const int32_t *mask_rects;     /* [n_masks][4] {x0, y0, x1, y1}, lent, 16-byte aligned (lpf_set_mask_rects' contract); or NULL */
    const double  *corners_cam0;   /* [n_boxes][8][3], lent; or NULL = the boxes in force stay */
    const double  *T_cam_to_velo;  /* host memory, row-major 4x4 (with corners_cam0) */
    int32_t        n_masks, n_boxes;   /* 0 <= n_masks <= LPF_MAX_MASKS_WIDE */
    int32_t        filter_visible, oriented;
    lpf_wide_outputs out;          /* LW = ceil(n_masks / 32) label words per point; out.on_device must be 1 */
} lpf_frame_job_wide;
int lpf_run_frame_wide(lpf_ctx *ctx, const lpf_frame_job_wide *job);

/* ---- one scan in several cameras -----------------------------------------------------------------------------------------------
 * lpf_run_cams: a batch of F frames labelled in C cameras (1 <= C <= LPF_MAX_CAMS) in ONE pass: every point is read from memory once
 * and projected, clipped and labelled in each camera's arithmetic; one streaming launch, one tail launch and one summary launch serve
 * all C cameras (each camera's mask pack and box tables are launches of their own, ahead of them).  The reference runs a camera per
 * process_frame*(seq, cam_id) call (V3:524-535, 572-573): a rig of two rectified cameras reads and projects the scan twice.
 * out[c] is, field for field and bit for bit, what a fresh context gives for
 *   lpf_set_camera(cams[c].T_velo_to_rect, K, W, H, depth_min_excl, depth_max_excl)
 *   lpf_set_mask_rects(masks.rects, ...)                              if masks.rects
 *   lpf_set_masks_u8 / lpf_set_masks_f32(masks: M, binarize, erode_iters)
 *   lpf_set_boxes_ex(corners_velo, boxes_on_device, box_off, F, oriented)   if corners_velo (else no boxes)
 *   lpf_run_batch(pts, frame_off, F, pts_on_device, &out[c])
 * Each camera has its own image size, depth window, 0 <= M <= LPF_MAX_MASKS masks (lpf_wide_input: uint8, or float32 under `binarize`;
 * masks.on_device 0 = host, copied by the call, else device memory lent until the call's work has completed), rectangles, erosion and
 * boxes.  The context's camera, masks, rectangles and boxes in force are left as they were (the pass has box tables of its own).  Not
 * capturable (LPF_ERR_STATE between lpf_graph_begin and lpf_graph_end); with a software-pipelined mode on it first launches what the
 * pipeline owes (no host wait), then runs in order.  Outputs: each out[c] is in host or device memory per its own on_device; with
 * device outputs the call only enqueues work (unless some input is in host memory), with host outputs it returns with them filled. */
typedef struct lpf_cam_input {
    double         T_velo_to_rect[16];     /* lpf_set_camera's arguments for this camera */
    double         K[9];
    int32_t        W, H;
    double         depth_min_excl, depth_max_excl;
    lpf_wide_input masks;                  /* [F][M][H][W] + optional rects [F][M][4], M <= LPF_MAX_MASKS (lpf_run_cams_wide: LPF_MAX_MASKS_WIDE);
                                              or LPF_MASKS_RLE: runs in THIS camera's image, pixel = y * W + x with W, H above */
    const double  *corners_velo;           /* [Btot][8][3] velodyne-frame corners (lpf_set_boxes_ex), or NULL: no boxes */
    const int32_t *box_off;                /* [F + 1], host memory (with corners_velo) */
    int32_t        boxes_on_device;        /* 0 / 1 / 2 as lpf_set_boxes_ex's on_device */
    int32_t        oriented;
} lpf_cam_input;
int lpf_run_cams(lpf_ctx *ctx, const float *pts, const int64_t *frame_off, int F, int pts_on_device, const lpf_cam_input *cams, int C,
                 const lpf_outputs *out /* [C] */);

/* lpf_run_cams_wide: lpf_run_cams with up to LPF_MAX_MASKS_WIDE masks per camera -- a batch of F frames labelled in C cameras
 * (1 <= C <= LPF_MAX_CAMS), camera c with 0 <= cams[c].masks.M <= LPF_MAX_MASKS_WIDE masks per frame, in ONE pass: every point is read
 * from memory once and projected, clipped and labelled in each camera's arithmetic with LW_c = ceil(M_c / 32) label words; each later
 * stage (compaction, instance lists, box counts, best boxes) is one launch for all C cameras (each camera's mask pack and box tables are
 * launches of their own, ahead of them).  Cameras may differ in M, mask type, binarisation, erosion, rectangles, image size, depth window
 * and boxes.  out[c] is, field for field and bit for bit, what a fresh context gives for
 *   lpf_set_camera(cams[c].T_velo_to_rect, K, W, H, depth_min_excl, depth_max_excl)
 *   lpf_set_boxes_ex(corners_velo, boxes_on_device, box_off, F, oriented)   if corners_velo (else no boxes)
 *   lpf_run_wide(pts, frame_off, F, pts_on_device, &cams[c].masks, &out[c])
 * LW_c sets the width of out[c].label_words and label_valid_words.  The checks are lpf_run_cams', with the mask limit raised to
 * LPF_MAX_MASKS_WIDE.  The context's camera, masks, rectangles and boxes in force are left as they were, and so is what lpf_run_cams and
 * lpf_run_wide keep between calls.  Not capturable (LPF_ERR_STATE between lpf_graph_begin and lpf_graph_end); with a software-pipelined
 * mode on it first launches what the pipeline owes (no host wait), then runs in order.  Outputs: each out[c] is in host or device memory
 * per its own on_device; with device outputs and device inputs the call only enqueues work, with host outputs it returns with them
 * filled. */
int lpf_run_cams_wide(lpf_ctx *ctx, const float *pts, const int64_t *frame_off, int F, int pts_on_device, const lpf_cam_input *cams, int C,
                      const lpf_wide_outputs *out /* [C] */);

/* ---- box membership as a stand-alone operator -------------------------------------------
 * inside[b*k + i] = 1 if point i lies in box b, else 0: the boolean arrays the reference's
 * oriented_point_in_bbox (V3:167-208, oriented = 1) and point_in_bbox (V3:143-164, oriented = 0)
 * return, for B boxes at once.  pts: f32 [k][stride] with stride 3 or 4 (x, y, z first);
 * corners_velo: f64 [B][8][3] host memory; pts / inside are host or device per on_device. */
int lpf_points_in_boxes(lpf_ctx *ctx, const float *pts, int64_t k, int stride, const double *corners_velo,
                        int B, int oriented, uint8_t *inside, int on_device);

/* ---- last-writer depth image -------------------------------------------------------------------
 * seg_with_pointcloud.py:160-170 fills, per mask, depthMap[v,u] = depth[idx] for idx ascending over
 * the valid points inside the mask; the last valid point of a pixel wins whatever the mask, so one
 * image describes all of them: depthMap_i = where(mask_i > 0.5, D, 0).  depth_img: f64 [H][W]
 * (0 where no valid point projects), winner: int32 [H][W] index of that point or -1 (may be NULL).
 * Uses lpf_set_camera's transform and depth window.  pts as in lpf_run; outputs follow on_device. */
int lpf_depth_image(lpf_ctx *ctx, const float *pts, int64_t N, int on_device, double *depth_img, int32_t *winner);

/* lpf_depth_maps: seg_with_pointcloud.py:160-170's per-car depth maps of a batch of F frames in ONE call, as sparse lists.  Let D_f be
 * lpf_depth_image's last-writer image of frame f (points frame_off[f] .. frame_off[f + 1] of pts) and member_m mask m's membership
 * under lpf_wide_input's rules (uint8 nonzero, float32 under binarize 0 / 1 / 2 -- 2 is the script's mask > 0.5 --, erode_iters,
 * the rectangles a hint: zero outside them).  Car m of frame f is then, bit for bit,
 *   pix = np.flatnonzero(np.where(member_m, D_f, 0)),  depth = D_f.ravel()[pix]
 * in entries car_off[f][m] .. car_off[f][m + 1] of row f of pix / depth / point_idx (point_idx: the winning point of the pixel, an
 * index within frame f).  in->M (0 .. LPF_MAX_MASKS_WIDE) is the same for every frame: frames with fewer masks pad with empty planes.
 * Camera, transform, size and depth window are lpf_set_camera's (the script's window is (0, 30)).  Entries at or beyond cap are not
 * written: need[f] is exact and overflow[f] says so.  The masks, rectangles, boxes and label state of the other calls are left as
 * they were.  Not capturable (LPF_ERR_STATE between lpf_graph_begin and lpf_graph_end); with a software-pipelined mode on it first
 * launches what the pipeline owes (no host wait), then runs in order.  With out->on_device (all outputs device memory) the call
 * only enqueues work, unless some input is in host memory; with host outputs it returns with them filled, after one host wait.
 * LPF_ERR_ARG: F < 0, M out of range, cap < 0, car_off or need NULL, pix NULL with cap > 0, bad frame offsets, binarize or
 * erode_iters; LPF_ERR_STATE: no camera.
 * Device memory: the frames go through in chunks whose scratch -- a u32 winner plane per frame (W * H rounded up to 1024 pixels),
 * counters of 8 bytes per (mask, 1024 pixels), with erosion lpf_run_wide's label planes (4 * ceil(M / 32) bytes per pixel, twice
 * with more than one iteration), staged host masks and points -- stays within 256 MiB, or one frame's worth when a single frame
 * needs more; plus F * cap * 24 bytes of staging for host outputs.  A 146-frame batch never holds 146 image planes at once. */
typedef struct lpf_depth_maps_outputs {
    int64_t  *pix;        /* [F][cap] flat pixel v * W + u, ascending within each car (may be NULL only with cap == 0) */
    double   *depth;      /* [F][cap] depth of that pixel's last valid point (may be NULL) */
    int64_t  *point_idx;  /* [F][cap] index of that point within its frame (may be NULL) */
    int64_t   cap;
    int64_t  *car_off;    /* [F][M + 1] car m of frame f = entries car_off[f][m] .. car_off[f][m + 1] (required) */
    int64_t  *need;       /* [F] entries frame f needs = car_off[f][M] (required) */
    int32_t  *overflow;   /* [F] 1 if need[f] > cap: entries at or beyond cap are not written (may be NULL) */
    int32_t   on_device;
    int32_t   reserved;
} lpf_depth_maps_outputs;
int lpf_depth_maps(lpf_ctx *ctx, const float *pts, const int64_t *frame_off, int F, int pts_on_device, const lpf_wide_input *in,
                   const lpf_depth_maps_outputs *out);
/* lpf_depth_maps for masks in RUN-LENGTH form (lpf_rle_masks above: host memory, runs index W x H of lpf_set_camera, masks->F == F,
 * 0 <= masks->M <= LPF_MAX_MASKS_WIDE, masks->erode_iters with the context's element).  Every output is bit for bit what
 * lpf_depth_maps gives for the equivalent dense uint8 host masks (dense[f][m][p] = 1 iff p lies in any run of mask m) with the same
 * erode_iters and no rectangles; output placement, cap / need / overflow, what is not written, the states left alone, "not
 * capturable", the pipelined modes and the one host wait are lpf_depth_maps'.  The whole input -- every frame of the batch -- is
 * checked by lpf_set_masks_rle's rules before anything is enqueued (LPF_ERR_ARG, "depth_maps_rle: frame f mask m run r ..."); the
 * caller may free runs, run_off and the struct when the call returns.  No dense mask exists anywhere: a chunk of frames zeroes its
 * label planes (4 * ceil(M / 32) bytes per pixel; twice with erosion), ORs its own runs in on the GPU, erodes the packed planes, and
 * the raster reads bit m & 31 of plane m / 32.  The chunks are planned as lpf_depth_maps plans them, a chunk's run tables counting in
 * place of its dense masks.  M = 0, or no run at all, launches no decode.
 * LPF_ERR_ARG besides lpf_depth_maps' output and frame checks: masks NULL, masks->F != F, M out of range, erode_iters < 0,
 * reserved != 0. */
int lpf_depth_maps_rle(lpf_ctx *ctx, const float *pts, const int64_t *frame_off, int F, int pts_on_device,
                       const lpf_rle_masks *masks, const lpf_depth_maps_outputs *out);

/* lpf_depth_overlays: seg_with_pointcloud.py:174-180's per-car overlay images of a batch of F frames in ONE call, from the sparse
 * lists of lpf_depth_maps.  For car m of frame f (entries car_off[f][m] .. car_off[f][m + 1] of row f of pix / depth) image
 * images[f][m] is, byte for byte, cv2.cvtColor(np.uint8(image_withseg * 255), cv2.COLOR_RGB2BGR) of the script:
 *   a listed pixel p:   (lut[i][2], lut[i][1], lut[i][0]),  i = min(255, (int)(256.0 * (depth / mx))),  mx = np.max(depthMap)
 *   any other pixel p:  (seg[f][p][2], seg[f][p][1], seg[f][p][0])
 * with lut = (matplotlib jet's _lut[:256, :3] * 255).astype(np.uint8) and one IEEE fp64 division.  max_depth[f][m] = mx, the max of
 * the car's depths, 0 for an empty car; an empty car's image is the reversed segmented image (the script skips that car: `continue`).
 * W and H are lpf_set_camera's (LPF_ERR_STATE without a camera).  Not capturable (LPF_ERR_STATE between lpf_graph_begin and
 * lpf_graph_end); with a software-pipelined mode on it first launches what the pipeline owes (no host wait).  The camera, masks,
 * rectangles, boxes and label state of the other calls are left as they were.  With every pointer device memory the call only
 * enqueues work; otherwise it returns after one host wait, with host outputs filled.
 * Lists in host memory are checked (offsets non-decreasing within [0, cap], pixels strictly ascending within each car and inside
 * the image, depths finite and > 0: LPF_ERR_ARG otherwise); lists in device memory are not, but are never read or written out of
 * bounds: offsets are clamped to [0, cap] and non-decreasing, pixels outside [0, W * H) are skipped.
 * LPF_ERR_ARG: F < 0, M out of range, cap < 0, car_off NULL, seg NULL with M > 0, pix or depth NULL with cap > 0, both outputs NULL
 * with M > 0, bad host lists.
 * Device memory: the (frame, car) images go through in chunks whose scratch -- staged segmented images and lists, images for host
 * outputs -- stays within 256 MiB, or one image's worth when a single image needs more; plus F * M * 8 bytes for host max_depth. */
typedef struct lpf_depth_overlay_input {
    const int64_t *pix;        /* [F][cap] rows as lpf_depth_maps writes them: flat v * W + u, strictly ascending per car */
    const double  *depth;      /* [F][cap] */
    int64_t        cap;
    const int64_t *car_off;    /* [F][M + 1] */
    int32_t        M;          /* 0 .. LPF_MAX_MASKS_WIDE */
    int32_t        lists_on_device;
    const uint8_t *seg;        /* [F][H][W][3] 8-bit segmented images at the camera's size */
    int32_t        seg_on_device;
    int32_t        reserved;
} lpf_depth_overlay_input;
typedef struct lpf_depth_overlay_outputs {
    uint8_t *images;           /* [F][M][H][W][3] (may be NULL) */
    double  *max_depth;        /* [F][M] np.max(depthMap), 0 for an empty car (may be NULL) */
    int32_t  on_device;
    int32_t  reserved;
} lpf_depth_overlay_outputs;
int lpf_depth_overlays(lpf_ctx *ctx, int F, const lpf_depth_overlay_input *in, const lpf_depth_overlay_outputs *out);

/* lpf_match_2d: the pair stage of V4's and V5's detection-to-box matching for a batch of F frames in ONE call: every (detection,
 * projected box) pair of every frame is scored as calculate_iou_2d (V4:118-137) and calculate_matching_score (V5:277-304) score it,
 * and every detection gets match_detections_to_bboxes' choice (V4:170-178).  Frame f owns detections det_off[f] .. det_off[f + 1]
 * (D_f of them) and boxes box_off[f] .. box_off[f + 1] (B_f); its matrices are the [D_f][B_f] block at pair_off[f] = sum_{g<f} D_g *
 * B_g of the [P] outputs (64-bit arithmetic).  The boxes' rectangles are what lpf_prepare_boxes / lpf_set_boxes_cam0 write.
 * The arithmetic is the reference's, type for type (NumPy 2 promotion of np.float32 detections against int64 / float64 boxes): with T
 * the detections' type (float32, or float64 under dets_f64) and every operation separate,
 *   xa = box x0 if box x0 > det x1 else det x1;  xb = box x1 if box x1 < det x2 else det x2;  same for y;  iou = 0 if xb <= xa or yb <= ya
 *   xb - xa: a T subtraction when both ends are the detection's, else float64; the product of the two differences is a T
 *   multiplication only when both are T;  area1 = (x2 - x1) * (y2 - y1) in T;  area2 in float64
 *   union = area1 + area2 - inter in float64, left to right;  iou = inter / union if union > 0 else 0
 *   detection centre (x1 + x2) / 2, (y1 + y2) / 2 in T, box centre in float64;  dist = sqrt(fma(dy, dy, dx * dx)) of the float64
 *   differences (np.linalg.norm);  center_score = c if c > 0 else 0 with c = 1 - dist / 1000
 *   size_score = min(area1, area2) / max(area1, area2) if both > 0 else 0
 *   total_score = w_iou * iou + w_center * center_score + w_size * size_score, left to right;  cost = 1 - total_score
 *   (equal areas: min and max both return area1, the ratio is a T 1.0 and w_size times it a T product: the size term is (T)w_size)
 * best_box[d] is the first strict maximum of the IoU over the frame's boxes in list order among those with iou > min_iou (an index
 * into the frame's boxes), -1 if there is none; best_iou[d] that IoU, 0 if none.  A box with front == 0 has no projection (V4:162-164
 * skips it): its column is iou 0, scores 0, cost 1 and it never wins; V5 drops such columns before the assignment (V5:337-341).
 * Degenerate detections (x2 < x1) follow the same statements; with non-finite coordinates the values are unspecified, but nothing
 * is read or written out of bounds.  A frame may have no detections or no boxes (its detections get -1 / 0); F = 0 does nothing.
 * Needs no camera, masks or boxes in force and leaves all of them as they were.  Not capturable (LPF_ERR_STATE between
 * lpf_graph_begin and lpf_graph_end); with a software-pipelined mode on it first launches what the pipeline owes (no host wait).
 * With every pointer device memory the call only enqueues work on the context's stream (the offsets go through the pinned upload
 * ring); otherwise it returns after one host wait, with host outputs filled.
 * LPF_ERR_ARG: NULL in / out, F < 0, NULL offsets, det_off[0] or box_off[0] < 0, decreasing offsets, dets NULL with detections,
 * bbox2d or front NULL with boxes, non-finite min_iou or weights.
 * Device memory: 24 bytes per frame; host inputs and outputs are staged frame range by frame range, each range within 256 MiB of
 * scratch, or one frame when a single frame needs more. */
typedef struct lpf_match2d_input {
    const void    *dets;       /* [Dtot][4] {x1, y1, x2, y2}: float32 (the detector's boxes.xyxy, V4:64), or float64 under dets_f64 */
    const int32_t *det_off;    /* [F + 1], host memory */
    const double  *bbox2d;     /* [Btot][4] {min u, min v, max u, max v} */
    const int32_t *front;      /* [Btot] corners with depth > 0; 0 = the box has no projection */
    const int32_t *box_off;    /* [F + 1], host memory */
    int32_t        dets_f64;
    int32_t        on_device;  /* dets, bbox2d, front are device memory, lent until the call's work has completed */
    double         min_iou;    /* V4: 0.25, firsttest.py: 0.1 */
    double         w_iou, w_center, w_size;   /* V5: 0.5, 0.3, 0.2 */
} lpf_match2d_input;
typedef struct lpf_match2d_outputs {           /* any pointer may be NULL: only what is asked for is computed and stored */
    int32_t *best_box;         /* [Dtot] */
    double  *best_iou;         /* [Dtot] */
    double  *iou;              /* [P] */
    double  *center_score;     /* [P] */
    double  *size_score;       /* [P] */
    double  *total_score;      /* [P] */
    double  *cost;             /* [P] the matrix V5:356 hands to linear_sum_assignment */
    int32_t  on_device;
    int32_t  reserved;
} lpf_match2d_outputs;
int lpf_match_2d(lpf_ctx *ctx, int F, const lpf_match2d_input *in, const lpf_match2d_outputs *out);

/* lpf_assign_costs: scipy.optimize.linear_sum_assignment for a batch of F cost matrices in ONE call -- the assignment stage of V5's
 * matcher (improved_match_detections_to_bboxes, V5:307-416), on the GPU.  Frame f owns rows det_off[f] .. det_off[f + 1] (D_f) and
 * columns box_off[f] .. box_off[f + 1] (B_f); its matrix is the [D_f][B_f] block at pair_off[f] = sum_{g<f} D_g * B_g of cost (64-bit
 * arithmetic): lpf_match_2d's layout.  A column whose front is <= 0 (a box without a projection, lpf_match_2d's rule) is dropped
 * before the assignment (V5:337-341); front == NULL: every column is live.  The result is SciPy's, not merely an optimal one: the
 * rectangular assignment by shortest augmenting paths with duals, on the transpose when the matrix of live columns is tall, with
 * SciPy's choice among equal path costs (the last position of its `remaining` list whose column is free, else the first; the list
 * filled descending and a chosen position overwritten with the last) and its float64 operations in its order.
 * col_of_row[d]: the column assigned to row d, an index into the frame's own columns in ORIGINAL numbering, or -1.  SciPy's (rows,
 * cols) are the rows with a column in ascending order; with more rows than live columns, D_f - live rows stay -1.
 * status[f]: 0 solved; 1 the live entries hold a NaN or -inf (SciPy: "matrix contains invalid numeric entries"), the frame is not
 * solved; 2 infeasible (+inf entries are legal and can leave a row without a finite column; SciPy: "cost matrix is infeasible").
 * With a status != 0 the frame's col_of_row is all -1.  A frame without rows or without live columns has status 0 and nothing
 * assigned; F = 0 does nothing.  Either output may be NULL.
 * A frame takes at most LPF_ASSIGN_MAX rows and LPF_ASSIGN_MAX live columns (the solver's state lives in LDS); live columns are
 * counted where front is host memory, with front in device memory (or NULL) every column counts.
 * Needs no camera, masks or boxes in force and leaves all of them as they were.  Not capturable (LPF_ERR_STATE between
 * lpf_graph_begin and lpf_graph_end); with a software-pipelined mode on it first launches what the pipeline owes (no host wait).
 * With every pointer device memory the call only enqueues work on the context's stream (the offsets go through the pinned upload
 * ring) and allocates nothing after the first call of a shape; otherwise it returns after one host wait, with host outputs filled.
 * No input spins the solver or makes it touch memory outside the frame: a path search is at most B_f steps, there are at most D_f
 * paths, every index is checked; the worst case is status 2.
 * LPF_ERR_ARG: NULL in / out, F < 0, NULL offsets, det_off[0] or box_off[0] < 0, decreasing offsets, cost NULL with pairs, a frame
 * beyond LPF_ASSIGN_MAX (the message names the frame, its size and the cap).
 * Device memory: 24 bytes per frame, and per range of frames the matrices of live columns (8 bytes per pair), 4 bytes per column and
 * frame; frames go through in ranges of consecutive frames, each within 256 MiB of scratch and staging. */
#define LPF_ASSIGN_MAX 1024
typedef struct lpf_assign_input {
    const double  *cost;       /* [P] */
    const int32_t *det_off;    /* [F + 1], host memory */
    const int32_t *box_off;    /* [F + 1], host memory */
    const int32_t *front;      /* [Btot] or NULL */
    int32_t        on_device;  /* cost and front are device memory, lent until the call's work has completed */
    int32_t        reserved;
} lpf_assign_input;
typedef struct lpf_assign_outputs {
    int32_t *col_of_row;       /* [Dtot] */
    int32_t *status;           /* [F] */
    int32_t  on_device;
    int32_t  reserved;
} lpf_assign_outputs;
int lpf_assign_costs(lpf_ctx *ctx, int F, const lpf_assign_input *in, const lpf_assign_outputs *out);

/* lpf_assign_2d: V5's matcher from detections and rectangles to accepted pairs for a batch of F frames in ONE call, with nothing
 * [P]-sized crossing this interface: every (detection, live box) pair is scored as lpf_match_2d scores it (the same device function;
 * in->min_iou is not used) into a scratch cost matrix in device memory, the matrix is assigned as lpf_assign_costs assigns it, and
 * each assigned pair is scored once more, so that iou / center_score / size_score / total_score [Dtot] are lpf_match_2d's matrix
 * entries at (d, box_of_det[d]) bit for bit, and 0 where nothing is assigned.  box_of_det[d]: an index into the frame's boxes, or
 * -1.  accepted[d] = total_score >= min_score_threshold && iou >= min_iou_threshold (V5:368; V5's values 0.3 and 0.15).  status[f]
 * as lpf_assign_costs'.  Any output may be NULL.  Everything else -- the cap, the ranges, ordering, capture, the pipeline -- is
 * lpf_assign_costs'; LPF_ERR_ARG also for what lpf_match_2d refuses and for thresholds that are NaN. */
typedef struct lpf_assign2d_params {
    double min_score_threshold;
    double min_iou_threshold;
} lpf_assign2d_params;
typedef struct lpf_assign2d_outputs {
    int32_t *box_of_det;       /* [Dtot] */
    double  *iou;              /* [Dtot] */
    double  *center_score;     /* [Dtot] */
    double  *size_score;       /* [Dtot] */
    double  *total_score;      /* [Dtot] */
    int32_t *accepted;         /* [Dtot] */
    int32_t *status;           /* [F] */
    int32_t  on_device;
    int32_t  reserved;
} lpf_assign2d_outputs;
int lpf_assign_2d(lpf_ctx *ctx, int F, const lpf_match2d_input *in, const lpf_assign2d_params *p, const lpf_assign2d_outputs *out);

/* lpf_inside_masks: V3's per-car inside / outside split for a batch of F frames in ONE call, from what a run leaves behind.  V3's
 * statistics dicts carry, next to the counts, inside_mask = oriented_point_in_bbox(car_points, best box) for a car that found its box
 * (V3:386-398) and None for one that did not (V3:413-425); create_colored_point_cloud_with_bbox_analysis (V3:471-515) and the geometry
 * list of V3:606-621 show car_points[inside_mask] and car_points[~inside_mask].  The inputs are a run's outputs -- lpf_run_batch's
 * inst_idx and summary columns, or lpf_run_wide's inst_idx / inst_off / best_box / best_cnt as they are -- the points are the run's
 * points, and the boxes and the `oriented` flag are the ones in force (lpf_set_boxes*): the packed parameters the run counted with.
 * Car m of frame f is MATCHED when best_box[f][m] >= 0 and best_cnt[f][m] >= min_points (V3:379).  With list m = entries
 * inst_off[f][m] .. inst_off[f][m + 1] of row f of inst_idx (k of them), and each entry of it tested against that ONE box:
 *   inside     parallel to inst_idx: 1 where the entry's point lies in the car's best box, else 0; all 0 for an unmatched or empty car.
 *              The test is the counting kernels' own, so a matched car's bytes sum to best_cnt[f][m] bit for bit.
 *   part_idx   the stable partition of the list, in the car's own entries: the inside entries first, then the outside ones, each in the
 *              list's (ascending) order; the outside part starts at inst_off[f][m] + n_inside[f][m].  An unmatched car's entries are
 *              its list unchanged.  These are point indices within the frame.
 *   part_xyz   the float32 x, y, z of the points of part_idx, in that order: car_points[inside_mask] followed by
 *              car_points[~inside_mask] (V3:488, V3:498), or car_points itself (V3:481).
 *   n_inside   bytes set for the car (0 for an unmatched one);  matched: 0 / 1.
 * Entries at or beyond inst_off[f][M] of a row are NOT WRITTEN, and no entry of the rows of a frame whose lists did not fit
 * (inst_overflow: inst_off[f][M] > inst_cap) is: such a frame's n_inside is 0, its matched is as above.  M (0 .. LPF_MAX_MASKS_WIDE) is
 * the width of the per-car arrays, as lpf_run_wide's; lpf_frame_summary's columns are 32 wide and go in as their first M + 1 / M entries.
 * The masks, boxes, rectangles and label state of the other calls are left as they were.  Not capturable (LPF_ERR_STATE between
 * lpf_graph_begin and lpf_graph_end); with a software-pipelined mode on it first launches what the pipeline owes (no host wait), then
 * runs in order.  pts (pts_on_device), the lists (in->on_device) and the outputs (out->on_device) are each in host or device memory;
 * frame_off is host memory.  With device outputs the call only enqueues work (unless some input is in host memory); with host outputs it
 * returns with them filled, after one host wait -- two when the lists are in device memory, whose offsets it has to read first.
 * Lists in host memory are checked; lists in device memory are not, but nothing is read or written out of bounds whatever they hold: a
 * car whose offsets do not ascend within [0, inst_cap] is skipped, an index outside the frame's points counts as outside (coordinates
 * 0), a best box outside the frame's boxes as none.
 * LPF_ERR_ARG: NULL in / out, F < 0, M out of range, inst_cap < 0, min_points < 0, frame_off NULL or bad, pts NULL with points, inst_off
 * NULL, best_box or best_cnt NULL with M > 0, inst_idx NULL with inst_cap > 0 and M > 0; host lists: offsets that are negative or
 * decrease, a best_box at or beyond the frame's box count, a negative best_cnt.  LPF_ERR_STATE: no boxes in force, or boxes for
 * another number of frames.
 * Device memory: 24 bytes per frame; 16 bytes per point for host points; F * (8 inst_cap + 20 M + 8) bytes for host lists and
 * F * (21 inst_cap + 12 M) for host outputs (grow-only, allocated on first use). */
typedef struct lpf_inside_input {
    const int64_t *inst_idx;   /* [F][inst_cap]  as lpf_wide_outputs / lpf_run_batch write it */
    int64_t        inst_cap;
    const int64_t *inst_off;   /* [F][M + 1] */
    const int32_t *best_box;   /* [F][M] */
    const int64_t *best_cnt;   /* [F][M] */
    int32_t        M, min_points;
    int32_t        on_device;  /* the four arrays are device memory, lent until the call's work has completed */
    int32_t        reserved;
} lpf_inside_input;
typedef struct lpf_inside_outputs {      /* any pointer may be NULL: not wanted */
    uint8_t *inside;           /* [F][inst_cap]  parallel to inst_idx */
    int64_t *part_idx;         /* [F][inst_cap]  per car: inside entries first, then outside */
    float   *part_xyz;         /* [F][inst_cap][3] */
    int64_t *n_inside;         /* [F][M]  0 for an unmatched car */
    int32_t *matched;          /* [F][M]  0 / 1 */
    int32_t  on_device;
    int32_t  reserved;
} lpf_inside_outputs;
int lpf_inside_masks(lpf_ctx *ctx, const float *pts, const int64_t *frame_off, int F, int pts_on_device, const lpf_inside_input *in,
                     const lpf_inside_outputs *out);

/* lpf_box_points: per-box LiDAR point counts, the ground-truth box of every valid point and the point-level confusion counts of a
 * batch of F frames in ONE call, from what a run leaves behind.  count_mb[m][b] counts the points of mask m in box b; what no run
 * returns is how many valid points box b holds at all -- the denominator of a recall.  This is the reference's box test,
 * oriented_point_in_bbox (V3:167-208) or point_in_bbox (V3:143-164), on ALL of points_valid = points[valid_indices, :3] (V3:590-592)
 * instead of on a car's points only.  The inputs are a run's compact outputs -- lpf_outputs' valid_idx / label_valid (LW = 1) or
 * lpf_wide_outputs' valid_idx / label_valid_words -- the points are the run's points, and the boxes and the `oriented` flag are the ones
 * in force (lpf_set_boxes*): the packed parameters the run counted with.  With the frame's valid points tested against each of its boxes:
 *   box_points    per box: the valid points of the box's frame inside it.
 *   box_labelled  per box: of those, the points with at least one label bit.  The test is the counting kernels' own (the float-bounds
 *                 reject, then the fp64 slab test), so count_mb[m][b] <= box_labelled[b] <= box_points[b] bit for bit.
 *   first_box     per valid point, parallel to valid_idx: the lowest index, within the frame's boxes, of a box that holds it, -1 if
 *                 none: point-level ground truth.  Entries at or beyond n_valid[f] of a frame are NOT WRITTEN.
 *   frame_counts  per frame {valid, in >= 1 box, labelled, labelled and in >= 1 box}: with "labelled" as the prediction and "in a box"
 *                 as the truth, tp = [3], fp = [2] - [3], fn = [1] - [3], tn = [0] - [1] - [2] + [3].
 * A box that filter_visible_bboxes dropped (lpf_set_boxes_cam0: its bounds are empty) keeps its position, counts 0 and is never a
 * first_box.  A frame without boxes or without valid points is legal; F = 0 does nothing.  All counts are integer sums: the same bytes
 * on every run.  The masks, boxes, rectangles, label state and camera of the other calls are left as they were.  Not capturable
 * (LPF_ERR_STATE between lpf_graph_begin and lpf_graph_end); with a software-pipelined mode on it first launches what the pipeline owes
 * (no host wait), then runs in order.  pts (pts_on_device), the lists (in->on_device) and the outputs (out->on_device) are each in host
 * or device memory; frame_off is host memory.  With everything in device memory the call only enqueues work; with any host pointer it
 * returns after one host wait, host outputs filled.
 * Lists in host memory are checked; lists in device memory are not, but nothing is read or written out of bounds whatever they hold:
 * n_valid[f] is clamped to [0, N_f]; an entry whose index is outside the frame's points counts in no box, has first_box -1 and is left
 * out of frame_counts[f][1..3].
 * LPF_ERR_ARG: NULL in / out, F < 0, frame_off NULL or bad, LW out of range, valid_idx or n_valid NULL with F > 0, pts NULL with points;
 * host lists: n_valid[f] outside [0, N_f], an index outside [0, N_f), indices that do not strictly ascend (the message names frame and
 * entry).  LPF_ERR_STATE: no boxes in force, or boxes for another number of frames.
 * Device memory: 24 bytes per frame; 16 bytes per point for host points; (8 + 4 LW) Ntot + 8 F bytes for host lists and
 * 8 Btot + 4 Ntot + 32 F for host outputs (grow-only, allocated on first use).  Device outputs are summed in place: no scratch. */
typedef struct lpf_box_points_input {
    const int64_t  *valid_idx;          /* [Ntot] as lpf_outputs / lpf_wide_outputs write it: frame f's at valid_idx[frame_off[f] ...],
                                           n_valid[f] entries, indices within the frame, ascending */
    const int64_t  *n_valid;            /* [F] */
    const uint32_t *label_valid_words;  /* [Ntot][LW] compact, frame f's rows from row frame_off[f], in valid_idx order: lpf_wide_outputs'
                                           label_valid_words, or lpf_outputs' label_valid with LW = 1; NULL or LW = 0: nothing is labelled */
    int32_t LW;                         /* 0 .. LPF_MAX_MASKS_WIDE / 32 */
    int32_t on_device;                  /* the three arrays are device memory, lent until the call's work has completed */
} lpf_box_points_input;
typedef struct lpf_box_points_outputs { /* any pointer may be NULL: not wanted */
    int32_t *box_points;                /* [Btot] valid points of the box's frame inside the box */
    int32_t *box_labelled;              /* [Btot] of those, points with at least one label bit */
    int32_t *first_box;                 /* [Ntot] compact, parallel to valid_idx: lowest index, within the frame's given boxes, of a box
                                           that holds the point; -1 if none.  Entries at or beyond n_valid[f] of a frame are not written */
    int64_t *frame_counts;              /* [F][4] {valid, in >= 1 box, labelled, labelled and in >= 1 box} */
    int32_t  on_device, reserved;
} lpf_box_points_outputs;
int lpf_box_points(lpf_ctx *ctx, const float *pts, const int64_t *frame_off, int F, int pts_on_device,
                   const lpf_box_points_input *in, const lpf_box_points_outputs *out);

/* lpf_box_views: secondtest.py's camera-view filter (is_bbox_in_camera_view / filter_bboxes_in_camera_view, secondtest.py:277-419) and
 * V5's detailed box projection (project_3d_bbox_to_2d, V5:215-252) for every box of a batch of F frames in ONE call.  Frame f owns
 * boxes box_off[f] .. box_off[f + 1] of the [Btot] arrays.  K, W and H are lpf_set_camera's (LPF_ERR_STATE without one).  The
 * arithmetic is the reference's, statement for statement, every operation separate:
 *   cam2image on the raw cam-0 corners as lpf_prepare_boxes does it: k-ordered fma chains over K, d == 0 -> -1e-6,
 *   u = rint(qx / |d|), v = rint(qy / |d|) (half to even)
 *   near = depth_lo <= d <= depth_hi (closed);  corners_near = its count;  corners_in_view = near corners with 0 <= u < W, 0 <= v < H
 *   reason, in the reference's order: corners_near == 0 -> 2 (all_behind_camera);  corners_in_view < min_points_in_view and the near
 *   corners' pixel box misses the image (x1 < 0 or x0 >= W or y1 < 0 or y0 >= H) -> 3 (no_intersection);  corners_near >= 2 and
 *   (umax - umin) * (vmax - vmin) < min_area -> 4 (too_small);  else 0 (valid).  keep = (reason == 0).  Codes 1 (no_corners) and 5
 *   (error) are the host's: such boxes are not part of the call
 *   avg_depth = np.mean of the near depths in corner order, in NumPy's summation order (fewer than 8 values: left to right from 0.0;
 *   exactly 8: ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7))), then one division by the count; 0 when there is none
 *   near_bbox2d = {min u, min v, max u, max v} of the near corners;  front / bbox2d / front_avg_depth: the same over the corners with
 *   d > 0 -- front and bbox2d bit-identical to lpf_prepare_boxes' (an empty set leaves the sentinels {1e300, 1e300, -1e300, -1e300} in
 *   either pixel box).  V5's center, size and area are exact integer arithmetic on bbox2d: the host derives them
 *   kept_pos[b] = the rank of box b among the kept boxes of its frame, in list order (the index space in which secondtest's matcher
 *   reports boxes), -1 for a dropped box;  frame_counts[f][r] = boxes of frame f with reason r ([0]: kept; [1] and [5] are 0)
 *   corners_velo = transform_bboxes_to_velodyne's (T_cam_to_velo . [c 1])[:3] as lpf_prepare_boxes has it; needs T_cam_to_velo
 * Device corners are not validated: nothing is read or written out of bounds whatever they hold; with non-finite corners the values
 * are unspecified.  A frame may have no boxes (its frame_counts are zeros); F = 0 does nothing.  Leaves camera, masks and boxes in
 * force as they were.  Not capturable (LPF_ERR_STATE between lpf_graph_begin and lpf_graph_end); with a software-pipelined mode on it
 * first launches what the pipeline owes (no host wait).  With every pointer device memory the call only enqueues work on the
 * context's stream (the frame table goes through the pinned upload ring): no host wait, and no allocation after the first call of a
 * shape; otherwise it returns after one host wait, with host outputs filled.
 * LPF_ERR_ARG: NULL in / out, F < 0, NULL box_off, box_off[0] < 0, a decreasing box_off, NULL corners_cam0 with boxes, corners_velo
 * without T_cam_to_velo, non-finite depth_lo / depth_hi / min_area, min_points_in_view outside 0 .. 8.
 * Device memory: 8 bytes per frame; host inputs and outputs are staged frame range by frame range, each range within 256 MiB of
 * scratch, or one frame when a single frame needs more. */
typedef struct lpf_box_views_input {
    const double  *corners_cam0;        /* [Btot][8][3] */
    const int32_t *box_off;             /* [F + 1], host memory */
    const double  *T_cam_to_velo;       /* [16] row-major, host memory; may be NULL unless corners_velo is asked for */
    int32_t        on_device;           /* corners_cam0 is device memory, lent until the call's work has completed */
    int32_t        min_points_in_view;  /* secondtest.py: 4 */
    double         depth_lo, depth_hi;  /* secondtest.py: 0.1, 100 */
    double         min_area;            /* secondtest.py: 100 */
} lpf_box_views_input;
typedef struct lpf_box_views_outputs {  /* any pointer may be NULL: only what is asked for is computed and stored */
    uint8_t *keep;                      /* [Btot] */
    int32_t *reason;                    /* [Btot] 0 valid, 2 all_behind_camera, 3 no_intersection, 4 too_small */
    int32_t *corners_in_view;           /* [Btot] */
    int32_t *corners_near;              /* [Btot] the reference's corners_with_valid_depth */
    double  *avg_depth;                 /* [Btot] */
    double  *near_bbox2d;               /* [Btot][4] */
    int32_t *front;                     /* [Btot] */
    double  *bbox2d;                    /* [Btot][4] */
    double  *front_avg_depth;           /* [Btot] */
    int32_t *kept_pos;                  /* [Btot] */
    int32_t *frame_counts;              /* [F][6] */
    double  *corners_velo;              /* [Btot][8][3] */
    int32_t  on_device, reserved;
} lpf_box_views_outputs;
int lpf_box_views(lpf_ctx *ctx, int F, const lpf_box_views_input *in, const lpf_box_views_outputs *out);

/* cv2.resize(mask.astype(np.uint8), (camera.width, camera.height)) (V3:222; INTER_LINEAR, the default) for masks that do not arrive at
 * the camera's size (the reference's scripts all pass retina_masks=True, so theirs do): n planes [h][w] of uint8 -> n planes [H][W]
 * (the size of lpf_set_camera), which then go to lpf_set_masks_u8 (nonzero = member = the reference's `> 0.5`).  Restated from
 * OpenCV 4.x resize.cpp (HResizeLinear / VResizeLinear, 11-bit weights; the x axis clamps index and fraction at the ends, the y axis
 * keeps the fraction and clips the two row indices) and pinned by construction only -- OpenCV is not part of this image and the
 * reference holds no resized fixture (oracle/numpy_path.py: cv2_resize_linear_u8 states the formula).  An exact 2 x 2
 * decimation (h == 2 H and w == 2 W) is what OpenCV hands to INTER_AREA: the rounded mean (a + b + c + d + 2) >> 2.  on_device: both pointers in host (0) or device (1) memory; device
 * callers: in stream order.  Not capturable. */
int lpf_resize_masks_u8(lpf_ctx *ctx, const uint8_t *src, int n, int h, int w, uint8_t *dst, int on_device);

/* cv2.erode(plane, cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (k, k)), iterations=iters) on n planes [h][w] of 8-bit VALUES, at the
 * planes' own size (V3:83-90), k = the context's element (lpf_set_erosion_element; 3 by default, the plus-shaped neighbourhood): the
 * minimum over the element, the image border left out.  For masks that do not
 * arrive at camera size the reference erodes first and resizes afterwards (V3:82-97, then V3:222): this call, then
 * lpf_resize_masks_u8.  (Masks at camera size are eroded inside lpf_set_masks_*, on the packed label image.)  src != dst; host or
 * device pointers per on_device, device callers in stream order.  Pinned by construction only, like lpf_set_masks_*'s erosion. */
int lpf_erode_masks_u8(lpf_ctx *ctx, const uint8_t *src, int n, int h, int w, int iters, uint8_t *dst, int on_device);

/* ---- box preparation on the GPU --------------------------------------------------------------
 * For nbox annotated boxes given by their 8 corners in the cam-0 frame (f64 [nbox][8][3], the
 * 'corners_cam0' of BBoxes_<frame>.json):
 *   visible[b]      = 1 if filter_visible_bboxes keeps the box (V3:121-140; needs lpf_set_camera's K, W, H)
 *   corners_velo    = transform_bboxes_to_velodyne's output (V3:41-52), f64 [nbox][8][3];
 *                     T_cam_to_velo = inv(TrVeloToCam), row-major 4x4
 *   bbox2d[b][4]    = {min u, min v, max u, max v} of the projected corners with depth > 0 and
 *   front[b]        = how many corners those are (V4:157-168; 0 -> the box is skipped by the IoU match)
 *                     u and v are the rounded pixels as float64 (not saturated).  A box with no corner in front (front[b] = 0) leaves
 *                     the sentinels {1e300, 1e300, -1e300, -1e300}.  The reference's pixels are integers, which have one zero; a
 *                     rounded float64 pixel may be -0.0 (a quotient in [-0.5, -0]), and the minimum / maximum order the zeros as
 *                     IEEE 754-2019 does (-0 < +0): a minimum of zeros is -0.0 if one of them is, a maximum +0.0 if one of them is.
 *                     lpf_set_boxes_cam0 and lpf_box_views (bbox2d and near_bbox2d) give the same bits.
 * Any output may be NULL.  Host pointers. */
int lpf_prepare_boxes(lpf_ctx *ctx, const double *corners_cam0, int nbox, const double T_cam_to_velo[16],
                      uint8_t *visible, double *corners_velo, double *bbox2d, int32_t *front);

/* ---- hipGraph capture of a launch set ------------------------------------------------------
 * lpf_graph_begin puts the context's stream into capture mode; every device-mode lpf_set_masks_* /
 * lpf_run* call issued until lpf_graph_end is recorded instead of executed (pointers and sizes are
 * baked in; the caller may add its own async copies on the same stream in between).  lpf_graph_end
 * instantiates the graph; lpf_graph_launch replays it on the context's stream.  The context must
 * have run the same shapes once before capture (so no allocation or table upload happens inside
 * it), and pipelining must be off.  For launch-bound per-frame loops (10 Hz streaming).
 * A graph points into buffers and tables the context owns.  Anything that moves or rewrites them after the
 * capture -- a run with another batch geometry, lpf_set_boxes with other box counts, lpf_set_camera, lpf_set_stream, a mode
 * switch, a call that had to grow a scratch buffer -- makes the graph stale: lpf_graph_launch then returns LPF_ERR_STATE
 * instead of replaying it.  An error returned by a call made inside a capture abandons the capture. */
typedef struct lpf_graph lpf_graph;
int  lpf_graph_begin(lpf_ctx *ctx);
int  lpf_graph_end(lpf_ctx *ctx, lpf_graph **out);
int  lpf_graph_launch(lpf_ctx *ctx, lpf_graph *g);
void lpf_graph_destroy(lpf_graph *g);

/* ---- measurement -------------------------------------------------------------------
 * With profiling on, every lpf_run* brackets its project+label kernel (lpf_k1_project, the
 * dominant kernel) with HIP events on the context's stream.  lpf_profile_read waits for the
 * stream, returns the summed elapsed milliseconds and the number of bracketed launches
 * since the last reset.  (No reference counterpart: the reference has no timers.) */
int lpf_profile_enable(lpf_ctx *ctx, int on);
int lpf_profile_read(lpf_ctx *ctx, double *k1_ms_sum, int64_t *k1_launches, int reset);
/* Duration between two event records with nothing between them on the context's stream (median of 33):
 * the part of an lpf_profile_* bracket that is not the kernel (4.6 us on MI355X / ROCm 7.2). */
int lpf_profile_overhead(lpf_ctx *ctx, double *empty_bracket_ms);

/* What the context has done so far (for tests and tuning: a software-pipelined stream must show no host wait and no drain):
 * out[0] host waits (the calling thread blocked on the GPU), [1] drains (owed work of the pipelined modes launched outside
 * a run), [2] table / corner uploads through the pinned ring (no wait), [3] step launches, [4] box jobs launched as a kernel
 * of their own, [5] box jobs that rode in a step launch, [6] uploads too large for the ring (they wait), [7] lpf_run_frame_wide jobs
 * whose masks were read directly, with no pack; n <= 8. */
int lpf_get_stats(lpf_ctx *ctx, int64_t *out, int n, int reset);

/* ---- multi-GPU: the one exchange step ------------------------------------------------------------
 * Frames shard across ranks with no data-path collective (V3:541: the frame loop has no cross-frame state);
 * what the ranks exchange at the end is a short int64 vector -- the aggregates of analyze_master_csv
 * (cvs:268-295): frames with rows, cars, matched cars, sums of total / inside / outside points, the inside
 * percentages as integer hundredths -- summed (op 0), or reduced by MIN (1) / MAX (2).  vec: host memory,
 * reduced in place over the caller's RCCL communicator (ncclComm_t, from ncclCommInitRank), one rank per GPU,
 * on the context's stream; returns when vec holds the result -- it blocks, with no timeout, until every rank of the
 * communicator has made the call.  ncclAllReduce is taken from the RCCL already loaded in the process (so that it is the
 * library the communicator came from); only a process with none gets the system's librccl loaded at the first call. */
int lpf_allreduce_metrics(lpf_ctx *ctx, int64_t *vec, int n, int op, void *rccl_comm);

/* lpf_first_match: the exclusive, first-mask-wins labelling of Same_color.py:113-132 for a batch of F frames in ONE call.  Frame f owns
 * points frame_off[f] .. frame_off[f + 1] and masks in->masks[f][0 .. M).  Projection and clip are lpf_set_camera's (the script's
 * depth window is (0, 30)); LPF_ERR_STATE without a camera.  For each valid point of a frame, in ascending index order, the FIRST m in
 * 0 .. M-1 with  v < mh && u < mw && mask[f][m][v][u] > 0.5  takes the point: a car point of mask m.  A valid point no mask takes is
 * background.  float32 masks: NaN, 0.5 and negative values are not members; uint8 masks: nonzero is a member.  mh x mw is the masks'
 * OWN size -- smaller or larger than the image; nothing is resized (the script never does), and nothing outside [0, mh) x [0, mw) is
 * read.  M is the same for every frame: pad a frame that has fewer masks with empty planes.
 *   first_mask  dense, per point: -2 not valid, -1 valid and in no mask, else the first mask.
 *   car_idx / car_mask / car_xyz / car_rgb   the car points of frame f from entry frame_off[f] on, n_car[f] of them, ascending: the
 *               index within the frame, the first mask, points[idx, :3] (colored_points) and colors[f][mask] (colored_colors).
 *   bg_idx / bg_xyz   the same for the n_bg[f] background points (full_points).
 *   n_valid = n_car + n_bg; mask_count[f][m]: the points whose first mask is m (their sum is n_car[f]).
 * Entries of a frame's span at or beyond its count are NOT WRITTEN.  All sums are integers: the same bytes on every run.  The camera,
 * masks, rectangles, boxes and label state of every other call are left as they were.  Not capturable (LPF_ERR_STATE between
 * lpf_graph_begin and lpf_graph_end); with a software-pipelined mode on it first launches what the pipeline owes (no host wait), then
 * runs in order.  pts (pts_on_device), the masks and colours (in->on_device) and the outputs (out->on_device) are each in host or device
 * memory; frame_off is host memory.  With everything in device memory the call only enqueues work; with any host pointer it returns
 * after one host wait, host outputs filled (a host caller's lists travel up first and come back whole, so that what is not written
 * stays as it was).  Nothing is read or written out of bounds whatever the points and masks hold.
 * LPF_ERR_ARG (the message names the argument): NULL in / out / frame_off, F < 0, frame_off that does not start at 0 or decreases, M
 * outside 0 .. LPF_MAX_MASKS_WIDE, masks NULL or mh / mw <= 0 with M > 0, car_rgb without colors, NULL n_car or n_bg, pts NULL with
 * points.  F = 0 and Ntot = 0 are fine.
 * Device memory: 8 (F + 1) bytes; frames go through in ranges of consecutive frames that keep what is staged within 256 MiB (a frame
 * that needs more is a range of its own): 4 bytes per point for the codes unless first_mask is given, 16 bytes per 1024 points and
 * per frame for the tile counters, 16 bytes per point for host points, the masks and colours of a range when they are host memory,
 * and 4 .. 72 bytes per point + (24 + 8 M) per frame for host outputs (grow-only, allocated on first use). */
typedef struct lpf_first_match_input {
    const void   *masks;      /* [F][M][mh][mw] uint8 (nonzero = member) or float32 (member <=> > 0.5) */
    const double *colors;     /* optional [F][M][3]: the rows car_rgb gathers (the binding passes np.array(mask_colors[i]) / 255.0); same
                                 memory as masks */
    int32_t M;                /* 0 .. LPF_MAX_MASKS_WIDE, the same for every frame (pad with empty planes) */
    int32_t mh, mw;           /* the masks' own size, > 0 when M > 0 */
    int32_t f32;              /* 0: uint8, 1: float32 (anything else -- LPF_MASKS_RLE included: dense masks only -- is LPF_ERR_ARG) */
    int32_t on_device;        /* 0: host, copied by the call; else device memory lent until the work has completed */
    int32_t reserved;
} lpf_first_match_input;
typedef struct lpf_first_match_outputs {   /* any list may be NULL; all host or all device per on_device; Ntot = frame_off[F] */
    int32_t *first_mask;      /* [Ntot]     dense: -2 not valid, -1 valid and in no mask, else the first mask */
    int64_t *car_idx;         /* [Ntot]     frame f's at frame_off[f]: n_car[f] indices within the frame, ascending */
    int32_t *car_mask;        /* [Ntot]     same order: the first mask of each */
    float   *car_xyz;         /* [Ntot][3]  colored_points */
    double  *car_rgb;         /* [Ntot][3]  colored_colors (needs in->colors) */
    int64_t *bg_idx;          /* [Ntot]     n_bg[f] indices, ascending */
    float   *bg_xyz;          /* [Ntot][3]  full_points */
    int64_t *n_valid, *n_car, *n_bg;   /* [F] (n_car and n_bg required) */
    int64_t *mask_count;      /* [F][M]     points whose first mask is m */
    int32_t  on_device, reserved;
} lpf_first_match_outputs;
int lpf_first_match(lpf_ctx *ctx, const float *pts, const int64_t *frame_off, int F, int pts_on_device,
                    const lpf_first_match_input *in, const lpf_first_match_outputs *out);
/* lpf_first_match for masks in RUN-LENGTH form.  The runs index the masks' OWN size: run pixel (x, y) = y * mw + x, mh x mw smaller or
 * larger than the image; as in lpf_first_match a point's pixel is tested against mw, mh and the image before anything is read.  Every
 * output is bit for bit what lpf_first_match gives for the equivalent dense uint8 host masks [F][M][mh][mw] (1 iff the pixel lies in
 * any run of the mask) and the same colours; output placement, what is not written, the states left alone, "not capturable", the
 * pipelined modes and the one host wait are lpf_first_match's.  The whole input -- every frame of the batch -- is checked by
 * lpf_set_masks_rle's rules against mh * mw before anything is enqueued (LPF_ERR_ARG, "first_match_rle: frame f mask m run r ...");
 * the caller may free runs, run_off and both structs when the call returns.  A range of frames zeroes its label planes
 * [frames][ceil(M / 32)][mh][mw] uint32, ORs its own runs in on the GPU, and a point's first mask is the lowest set bit of at most
 * ceil(M / 32) words (lpf_fm_count_planes) where the dense walk reads up to M bytes; the planes and the range's run tables count in
 * the 256 MiB of a range in place of the dense masks.
 * LPF_ERR_ARG besides lpf_first_match's output and frame checks: in or in->masks NULL, masks->F != F, M out of range,
 * masks->erode_iters != 0, reserved != 0 (either struct), mh or mw <= 0 with M > 0. */
typedef struct lpf_first_match_rle_input {
    const lpf_rle_masks *masks;   /* host; masks->F == F, 0 <= M <= LPF_MAX_MASKS_WIDE, erode_iters == 0 */
    const double *colors;         /* optional [F][M][3], as lpf_first_match_input.colors */
    int32_t mh, mw;               /* the masks' OWN size: run pixel (x, y) = y * mw + x; > 0 when M > 0 */
    int32_t colors_on_device;     /* 0: colors in host memory, copied by the call; else device memory lent until the work has completed */
    int32_t reserved;             /* 0 */
} lpf_first_match_rle_input;
int lpf_first_match_rle(lpf_ctx *ctx, const float *pts, const int64_t *frame_off, int F, int pts_on_device,
                        const lpf_first_match_rle_input *in, const lpf_first_match_outputs *out);

/* ---- scan reader ------------------------------------------------------------------------------
 * Double-buffered velodyne .bin reader for frame loops and the 10 Hz stream.  Stands where the
 * reference calls Kitti360Viewer3DRaw.loadVelodyneData once per frame (V3:24-28, V3:545:
 * np.fromfile(path, float32).reshape(-1, 4); RuntimeError('<path> does not exist!') when missing):
 * a worker thread reads the submitted files, in order, into pinned host memory and an internal
 * copy stream moves them to HBM while earlier scans are being processed.
 *   lpf_reader_create  n_buffers in [2,16] scans in flight, each up to max_points points.
 *   lpf_reader_submit  enqueue a file (returns at once; any number may be outstanding).
 *   lpf_reader_next    the oldest submitted scan: *d_pts = its HBM copy (pass to lpf_run* with
 *                      pts_on_device = 1), *h_pts = the pinned host copy (the array the reference
 *                      would hold; for host-side gathers), *n_points = N.  The context's stream
 *                      waits on the device for the copy; the host does not block on PCIe.  Pointers
 *                      stay valid until the next lpf_reader_next on this reader (work already enqueued
 *                      on the context's stream may still use them after that).  A missing / malformed
 *                      file gives LPF_ERR_IO for that scan (lpf_last_error names it) and the reader
 *                      carries on with the following one.
 *   lpf_reader_destroy before lpf_destroy of its context (the reader uses the context's stream).
 *   lpf_reader_wait    host-side wait for the copy of the scan handed out last (only for callers that
 *                      touch *d_pts outside the context's stream). */
typedef struct lpf_reader lpf_reader;
int  lpf_reader_create(lpf_ctx *ctx, lpf_reader **out, int n_buffers, int64_t max_points);
int  lpf_reader_submit(lpf_reader *rd, const char *path);
int  lpf_reader_next(lpf_reader *rd, const float **d_pts, const float **h_pts, int64_t *n_points);
int  lpf_reader_wait(lpf_reader *rd);
void lpf_reader_destroy(lpf_reader *rd);

/* A frame's second file: bboxes_3D_cam0/BBoxes_<frame>.json, which the reference reads with json.load (load_bounding_boxes,
 * V3:31-38; cvs_erosion.py:333): a list of {"index": int, "corners_cam0": [[x, y, z] x 8]}.  Parsing 270 KB of 17-digit numbers
 * (frame 2449, 314 boxes) costs a Python frame loop more than all of its GPU work, so the reader's worker can do it beside the scan:
 *   lpf_reader_submit_frame  as lpf_reader_submit, plus the frame's box file (NULL: none).
 *   lpf_reader_boxes         the box file of the scan handed out by the last lpf_reader_next: *state says what became of it
 *                            (LPF_BOXES_*); when PARSED, *corners_cam0 = float64 [*nbox][8][3] -- what lpf_prepare_boxes /
 *                            lpf_set_boxes_cam0 take -- and *index = int32 [*nbox], host memory of the reader, valid until the next
 *                            lpf_reader_next.  A missing or unexpected box file never fails the scan.
 *   lpf_parse_boxes_json     the same parser on its own (no context, no GPU): fills the caller's arrays of capacity cap boxes;
 *                            *nbox = boxes in the file; more than cap: LPF_ERR_ARG with *nbox set (file size / 64 boxes always do).
 * Numbers are converted with strtod in the C locale -- correctly rounded, as Python's float() is: the same doubles.  OTHER means the
 * file is not that plain schema (other keys, a float index, NaN / Infinity, escapes in keys, malformed or trailing text) and has NOT
 * been interpreted: hand it to a JSON library, whose result or error is then the reference's. */
enum lpf_boxes_state {
    LPF_BOXES_PARSED = 0,          /* corners and indices are there (possibly zero boxes: the reference skips such a frame) */
    LPF_BOXES_ABSENT = 1,          /* no such file: the reference prints "No bounding boxes found" and skips the frame */
    LPF_BOXES_OTHER = 2,           /* not the plain schema / unreadable: not interpreted */
    LPF_BOXES_NONE = 3             /* no box file was submitted with that scan */
};
int  lpf_reader_submit_frame(lpf_reader *rd, const char *scan_path, const char *boxes_path);
int  lpf_reader_boxes(lpf_reader *rd, const double **corners_cam0, const int32_t **index, int *nbox, int *state);
int  lpf_parse_boxes_json(const char *path, double *corners_cam0, int32_t *index, int cap, int *nbox, int *state);

#ifdef __cplusplus
}
#endif
#endif /* LPF_H */
