/*
 * comfystereo_amd.h -- C ABI of the MI355X-native depth-to-stereo engine (libcomfystereo_hip.so).
 *
 * The reference (Dobidop/ComfyStereo) is pure Python and has no FFI; its only seam is the Python
 * module boundary `GenerateStereo.py` -> `stereoimage_generation.py`.  The entry points below are what
 * a binding for that seam binds: each one cites the reference interface it replaces.  They are
 * called by comfystereo_amd/_native.py (ctypes) on behalf of the drop-in module functions
 * `create_stereoimages` / `create_stereoimages_gpu` and of `StereoImageNode.generate`.
 *
 * Conventions
 *   - plain pointers and sizes only; every buffer is caller-owned DEVICE memory (HIP), row-major,
 *     contiguous in the stated shape; no allocation happens inside the library
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously on it
 *   - return value: CS_OK (0) or a negative CS_E* code; cs_last_error() returns a thread-local
 *     message for the last failing call
 *   - scalar parameters are doubles because they are Python floats in the reference, which rounds
 *     them to float32 at specific points of the arithmetic
 *   - re-entrant per stream as long as each concurrent call gets its own workspace; the only process-wide state
 *     is opt-in (cs_profile's event pool, guarded by a mutex; cs_debug_set's development switches)
 */
#ifndef COMFYSTEREO_AMD_H
#define COMFYSTEREO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CS_ABI_VERSION 4

#if defined(__GNUC__)
#define CS_API __attribute__((visibility("default")))
#else
#define CS_API
#endif

enum cs_status {
    CS_OK = 0,
    CS_EINVAL = -1,    /* bad argument (null pointer, size <= 0, unknown enum) */
    CS_EWORKSPACE = -2,/* workspace too small: see cs_workspace_bytes */
    CS_ELIMIT = -3,    /* frame too wide for the LDS-resident row kernels (see cs_max_width) */
    CS_EHIP = -4       /* a HIP runtime call failed */
};

/* fill_technique keys: 0..7 are the UI-reachable ones of reference GenerateStereo.py:88-100; 8..10 are the remaining
 * branches of the dispatcher stereoimage_generation.py:1605-1610, reachable through its module functions only */
enum cs_fill {
    CS_FILL_NONE = 0,                /* 'none'                 stereoimage_generation.py:1850-1910 */
    CS_FILL_NAIVE = 1,               /* 'naive'                :1893-1908 */
    CS_FILL_NAIVE_INTERPOLATING = 2, /* 'naive_interpolating'  :1871-1892 */
    CS_FILL_POLYLINES_SOFT = 3,      /* 'polylines_soft'       :1912-1992 */
    CS_FILL_POLYLINES_SHARP = 4,     /* 'polylines_sharp'      :1912-1992 */
    CS_FILL_INVERSE = 5,             /* 'inverse'              :1715-1737 */
    CS_FILL_HYBRID_EDGE = 6,         /* 'hybrid_edge'          :1837-1848 */
    CS_FILL_GPU_WARP = 7,            /* 'gpu_warp'             forward_warp_gpu :277-450 */
    /* branches of the dispatcher that no UI string reaches (reference :1605-1610); not valid for gpu paths */
    CS_FILL_NONE_POST = 8,           /* 'none_post'            :1804-1817 (forward map + row-wise np.interp) */
    CS_FILL_INVERSE_POST = 9,        /* 'inverse_post'         :1820-1833 */
    CS_FILL_HYBRID_EDGE_PLUS = 10    /* 'hybrid_edge_plus'     :1778-1802 (hybrid_edge, black pixels from polylines_soft) */
};

/* output modes of reference stereoimage_generation.py:1543-1562 / :1093-1120 */
enum cs_mode {
    CS_MODE_LEFT_RIGHT = 0,
    CS_MODE_RIGHT_LEFT = 1,
    CS_MODE_TOP_BOTTOM = 2,
    CS_MODE_BOTTOM_TOP = 3,
    CS_MODE_RED_CYAN_ANAGLYPH = 4,
    CS_MODE_LEFT_ONLY = 5,
    CS_MODE_ONLY_RIGHT = 6,
    CS_MODE_CYAN_RED_REVERSEANAGLYPH = 7
};

/* One call of StereoImageNode.generate (reference GenerateStereo.py:79-80): widget values + shapes. */
typedef struct cs_params {
    int32_t n, h, w;            /* image batch [n][h][w][3] float32 0..1 (ComfyUI IMAGE)            */
    int32_t depth_h, depth_w;   /* depth batch [n][depth_h][depth_w][depth_c] float32               */
    int32_t depth_c;            /* 3 -> 0.2989 R + 0.5870 G + 0.1140 B; 1 -> as is; else channel 0  */
    int32_t fill;               /* enum cs_fill                                                     */
    int32_t mode;               /* enum cs_mode                                                     */
    int32_t batch_size;         /* gpu_warp only: frames per reference sub-batch (its 0..255 test is
                                   global over a sub-batch, stereoimage_generation.py:1045, :315)   */
    int32_t depth_map_blur;     /* bool: direction-aware depth blur on/off                          */
    int32_t depth_blur_vert_smooth;
    int32_t flags;              /* bit 0: gpu_warp depth outputs are NOT clamped to 0..1 (module-level
                                   create_stereoimages_gpu returns them unclamped, :1125-1126)
                                   bit 1: `stereo` receives the uint8 codes k (value = k/255) instead of
                                   float32 -- the compact form frame shards are all-gathered in; CPU
                                   techniques only (gpu_warp colours are genuine floats)
                                   bit 2: fill gpu_warp runs the mesh-quality warp (forward_warp_mesh,
                                   :453-689 -- what the reference does when moderngl is importable,
                                   :1068-1071) instead of forward_warp_gpu; see cs_forward_warp_mesh
                                   bits 3, 4: arithmetic dialect.  0 = D32, the reference WITHOUT numba
                                   (float32 disparities, uint8 pixel sums that wrap) -- the pinned
                                   contract.  bit 3: float64 disparity chain, bit 4: int64 pixel
                                   sums; both = D64, the typing numba gives the reference's kernels
                                   (derived).  polylines_soft / sharp: bit 3 =
                                   point coordinates from the float64 chain, rounded once into the
                                   float32 point array (pinned: tests/golden/dialect_f64.npz), bit 4 =
                                   numba's float64 typing of the sweep (derived; a literal one-lane
                                   replay per row in the general row kernel -- a compatibility path).
                                   hybrid_edge: bit 3 = dest_x, its distance to the column and the exp
                                   argument in float64 (pinned), bit 4 = float64 weight sums (derived).
                                   none / naive / naive_interpolating / inverse / polylines_* /
                                   hybrid_edge only, else CS_EINVAL                                */
    double divergence, separation, stereo_balance, convergence_point, stereo_offset_exponent;
    double depth_blur_strength, depth_blur_edge_threshold, depth_blur_falloff;
} cs_params;

CS_API int cs_version(void);
CS_API const char *cs_last_error(void);

/* Largest frame width the LDS-resident row kernels accept for `fill` (160 KiB LDS per CU). */
CS_API int cs_max_width(int fill);
/* The same for one output mode.  The row kernels' own anaglyph form keeps 2 more bytes of LDS per pixel; since round 6 every technique but
 * hybrid_edge_plus runs an anaglyph beyond that form's width side by side into scratch and composes afterwards, so the anaglyph limit equals
 * the side-by-side limit (cs_max_width is the anaglyph, i.e. smallest, limit). */
CS_API int cs_max_width_mode(int fill, int mode);
/* ABI 4: the widest frame cs_generate accepts with p's technique, mode, dialect flags (bits 3 / 4) and disparity parameters
 * (p->w, p->h, p->n are ignored): the same predicate the call itself applies, so pre-validation cannot disagree with it.
 * It can be lower than cs_max_width_mode -- e.g. an anaglyph of a polylines technique beyond the row kernel's own anaglyph
 * form only passes while the tile kernels take it (halo within their reach, no full-D64 flag). */
CS_API int cs_max_width_params(const cs_params *p);

/* Shape of the outputs of cs_generate for `p`: stereoscope [n][*out_h][*out_w][3],
 * mask [n][*mask_h][*mask_w] (output-shaped for the CPU techniques, eye-shaped for gpu_warp). */
CS_API int cs_output_shape(const cs_params *p, int *out_h, int *out_w, int *mask_h, int *mask_w);

/* Scratch bytes cs_generate needs for `p` (intermediate gray/blurred depth, per-frame statistics). */
CS_API size_t cs_workspace_bytes(const cs_params *p);

/*
 * The fused batch path.  Replaces StereoImageNode.generate's per-frame loop
 * (GenerateStereo.py:117-269: grayscale, resize, create_stereoimages[_gpu], convertResult,
 * generate_mask) for device-resident tensors:
 *   image     [n][h][w][3]            float32 in 0..1
 *   depth     [n][depth_h][depth_w][depth_c] float32
 *   stereo    [n][out_h][out_w][3]    float32   "stereoscope"
 *   depth_l/r [n][h][w][3]            float32   "blurred_depthmap_left/right"
 *   mask      [n][mask_h][mask_w]     float32   "no_fill_imperfect_mask"
 */
CS_API int cs_generate(const cs_params *p, const float *image, const float *depth, float *stereo, float *depth_l,
                float *depth_r, float *mask, void *workspace, size_t workspace_bytes, void *stream);

/*
 * apply_stereo_divergence (reference stereoimage_generation.py:1576-1620) for one eye of `n`
 * independent frames: per-frame min/max normalisation, convergence shift, percent -> pixels, row
 * kernel `fill` (any CPU technique).  image_u8 [n][h][w][3] uint8, depth [n][h][w] float32,
 * out_u8 [n][h][w][3].  workspace: cs_asd_workspace_bytes_for(n, h, w, fill) (cs_asd_workspace_bytes: enough for any technique).
 */
CS_API size_t cs_asd_workspace_bytes(int n, int h, int w);
CS_API size_t cs_asd_workspace_bytes_for(int n, int h, int w, int fill);
CS_API int cs_apply_stereo_divergence(const uint8_t *image_u8, const float *depth, int n, int h, int w, double divergence,
                               double separation, double stereo_offset_exponent, int fill, double convergence_point,
                               uint8_t *out_u8, void *workspace, size_t workspace_bytes, void *stream);
/* The same with the arithmetic dialect named: 0 = D32 (as above), 1 = float64 disparity chain, 2 = int64 pixel sums,
 * 3 = both = D64 (cs_params.flags bits 3 / 4). */
CS_API int cs_apply_stereo_divergence2(const uint8_t *image_u8, const float *depth, int n, int h, int w, double divergence,
                                double separation, double stereo_offset_exponent, int fill, double convergence_point,
                                int dialect, uint8_t *out_u8, void *workspace, size_t workspace_bytes, void *stream);

/*
 * directional_motion_blur_gpu (reference stereoimage_generation.py:1171-1251; its own callers pass
 * blur_mask_width = blur_strength, :1051-1054 / :1479-1482).  depth, out_l, out_r: [n][h][w]
 * float32 on the 0..255 scale.  blur_strength <= 0 copies the input (:1194).
 * workspace: cs_blur_workspace_bytes(n, h, w).
 */
CS_API size_t cs_blur_workspace_bytes(int n, int h, int w);
CS_API int cs_directional_blur(const float *depth, int n, int h, int w, double blur_strength, double edge_threshold,
                        double blur_mask_width, double falloff_exponent, int vert_smooth_px, float *out_l, float *out_r, void *workspace,
                        size_t workspace_bytes, void *stream);

/*
 * directional_motion_blur (reference stereoimage_generation.py:1346-1419): the scipy depth blur create_stereoimages applies to
 * numpy / PIL inputs (:1489-1494) -- scipy.ndimage's float64 accumulation, 'reflect' / 'nearest' borders, no x255 rescaling.
 * depth [n][h][w] float32 (as given) -> out_l / out_r [n][h][w] float32.  workspace: cs_blur_scipy_workspace_bytes(n, h, w).
 * CS_EINVAL when blur_strength rounds to 0 taps (the reference raises there as well).
 */
CS_API size_t cs_blur_scipy_workspace_bytes(int n, int h, int w);
CS_API int cs_directional_blur_scipy(const float *depth, int n, int h, int w, double blur_strength, double edge_threshold,
                              double blur_mask_width, double falloff_exponent, int vert_smooth_px, float *out_l, float *out_r,
                              void *workspace, size_t workspace_bytes, void *stream);

/*
 * forward_warp_gpu (reference stereoimage_generation.py:277-450) for a sub-batch:
 * image [n][3][h][w] float32, depth [n][h][w] float32 -> warped [n][3][h][w] float32,
 * gap_mask [n][h][w] uint8 (1 = disocclusion).  workspace: cs_warp_workspace_bytes(n, h, w).
 */
CS_API size_t cs_warp_workspace_bytes(int n, int h, int w);
CS_API int cs_forward_warp(const float *image, const float *depth, int n, int h, int w, double divergence_px,
                    double separation_px, double stereo_offset_exponent, double convergence_point, float *warped,
                    uint8_t *gap_mask, void *workspace, size_t workspace_bytes, void *stream);
/* the same with the reference's two keyword parameters (stereoimage_generation.py:277-279): gradient_threshold -- adjacent pixels
 * are connected when their offsets differ by less than it (:339-340), max_stretch -- scatter rounds (:365).  CS_ELIMIT when more
 * than 16 rounds could change a column (gradient_threshold > 13 together with max_stretch > 16). */
CS_API int cs_forward_warp2(const float *image, const float *depth, int n, int h, int w, double divergence_px,
                     double separation_px, double stereo_offset_exponent, double convergence_point, double gradient_threshold,
                     int max_stretch, float *warped, uint8_t *gap_mask, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The reference's grid-sample warps (stereoimage_generation.py), one bilinear grid_sample (align_corners=True) at
 * grid x = linspace(-1, 1, w) - offset / (w / 2), grid y = linspace(-1, 1, h), offsets from forward_warp_gpu's depth chain
 * (the batch is divided by 255 when any frame's maximum is above 1; each frame normalised by its own min / max).
 *   CS_GRID_WARP     apply_stereo_divergence_gpu (:52-119): warped, border padding; no mask output
 *   CS_GRID_FILL     apply_stereo_divergence_gpu_with_fill (:923-1002) for n frames: warped with `padding` (CS_GRID_PAD_*),
 *                    mask = valid (the source x inside [-1, 1])
 *   CS_GRID_MASK     compute_forward_mask_gpu (:692-757): mask = the forward gap mask (dilated at offset steps above 1.5);
 *                    image and warped are not read / written
 *   CS_GRID_STRETCH  warp_and_fill_gpu (:122-274): the gap pixels' grid x stretched from the border grid values, mask = the gap mask
 * image [n][c][h][w] float32, depth [n][h][w] float32 -> warped [n][c][h][w] float32, mask [n][h][w] uint8 (0 / 1).
 * A null warped or mask skips that output.  padding must be CS_GRID_PAD_BORDER for every operation but CS_GRID_FILL.
 * workspace: cs_grid_warp_workspace_bytes(n, h, w).  CS_GRID_MASK and CS_GRID_STRETCH keep a row in LDS: frames wider than
 * cs_grid_warp_max_width(op) (19 486 columns) are refused with CS_ELIMIT; CS_GRID_WARP and CS_GRID_FILL have no width limit.
 * At most 65 535 frames per call.
 */
enum cs_grid_op { CS_GRID_WARP = 0, CS_GRID_FILL = 1, CS_GRID_MASK = 2, CS_GRID_STRETCH = 3 };
enum cs_grid_padding { CS_GRID_PAD_BORDER = 0, CS_GRID_PAD_ZEROS = 1, CS_GRID_PAD_REFLECTION = 2 };
CS_API size_t cs_grid_warp_workspace_bytes(int n, int h, int w);
CS_API int cs_grid_warp_max_width(int op);
CS_API int cs_grid_warp(const float *image, const float *depth, int n, int c, int h, int w, double divergence_px,
                        double separation_px, double stereo_offset_exponent, double convergence_point, int op, int padding,
                        float *warped, uint8_t *mask, void *workspace, size_t workspace_bytes, void *stream);
/* interpolate_fill_gpu (reference :860-920): image [n][c][h][w] float32, mask [n][h][w] uint8 (non-zero = fill) -> out
 * [n][c][h][w]: a masked pixel takes left * (1 - t) + right * t, left = the nearest unmasked column before it, right = the
 * row's LAST unmasked column if it lies after it; t = distance to left / max(distance to left + distance to right, 1), 1
 * without a left, 0 without a right border (a row with nothing unmasked takes column 0).  out must not alias image. */
CS_API int cs_interpolate_fill(const float *image, const uint8_t *mask, int n, int c, int h, int w, float *out, void *stream);
/* detect_disocclusions_gpu (reference :807-857): depth [h][w], grid [h][w][2] (x, y), grid_x_warped [h][w] float32 -> out
 * [h][w] uint8: depth sampled at the grid (nearest, border padding, align_corners=True) minus depth above `threshold`, or
 * |grid_x_warped[x + 1] - grid_x_warped[x]| above 3 * 2 / w (the last column takes the step before it).  w >= 2. */
CS_API int cs_detect_disocclusions(const float *depth, const float *grid, const float *grid_x_warped, int h, int w,
                                   double threshold, uint8_t *out, void *stream);

/*
 * The front half of StereoDiffusion's Fast mode (reference stereodiffusion_nodes.py:425-571, _generate_stereo_fast_single
 * around its inpainting model), n independent frames: image [n][3][h][w] float32 (values k / 255), depth [n][h][w] float32.
 *   depth chain (:432-440)  d / 255 when THAT FRAME's maximum is above 1; (d - min) / (max - min) of the frame when the range
 *                           is above 1e-6, else 0; minus 0.5 (no exponent, no convergence point)
 *   warped (:442-454)       one bilinear grid_sample (border padding, align_corners=True) at grid x = linspace(-1, 1, w) -
 *                           (d * -divergence_px) / (w / 2), grid y = linspace(-1, 1, h)
 *   mask (:456-491)         dilate3x3(grid x outside [-1, 1]  |  dilate3x3(nearest sample of d + 0.5 at the grid minus d + 0.5
 *                           above `threshold`, reference 0.05)); an empty mask stays empty (the early return, :478)
 *   filled (:493-542)       a masked pixel takes left * (1 - t) + right * t (float32, unfused) of the warped colours at the
 *                           NEAREST unmasked column on either side (0 where there is none), t = distance to left / max(distance
 *                           to left + distance to right, 1), distances counted from 1 with the frame edge one step beyond the
 *                           last column; a row with nothing unmasked is 0.  Unmasked pixels keep warped.
 *   warped_u8 / filled_u8   trunc(value * 255) (:546, :564) as [n][h][w][3] uint8, the images the reference hands to the model
 *                           and blends its answer into (:563-571); defined for values in [0, 1]
 * -> warped, filled [n][3][h][w] float32, mask [n][h][w] uint8 (0 / 1).  Any null output is skipped.  divergence_px is the
 * reference's scale_factor / 100 * w (:430).  workspace: cs_inpaint_prepare_workspace_bytes(n, h, w).  The mask of a row is
 * kept in LDS: frames wider than cs_inpaint_prepare_max_width() (16 384 columns) are refused with CS_ELIMIT before any device
 * work.  Any h, w >= 1; at most 65 535 frames per call.
 */
CS_API size_t cs_inpaint_prepare_workspace_bytes(int n, int h, int w);
CS_API int cs_inpaint_prepare_max_width(void);
CS_API int cs_inpaint_prepare(const float *image, const float *depth, int n, int h, int w, double divergence_px,
                              double threshold, float *warped, float *filled, uint8_t *mask, uint8_t *warped_u8,
                              uint8_t *filled_u8, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Pillow's 8-bit bicubic resize, byte for byte: out = PIL.Image.resize((ow, oh)) of Pillow 12.2 with all defaults on modes L
 * (c = 1) and RGB (c = 3), n independent frames of interleaved codes [n][h][w][c] -> [n][oh][ow][c].  What StereoDiffusion's
 * Fast mode does around its 512 x 512 working size (reference stereodiffusion_nodes.py:415-423, :481-484, :569-573).
 *   passes   horizontal first, then vertical, whatever the direction of scaling; a pass whose input and output size agree is
 *            skipped (an exact copy).  The image between the passes is uint8 [h][ow][c]: its rounding and clipping count.
 *   taps     per axis, float64: scale = in / out, fs = max(scale, 1), support = 2 * fs; output sample xx has center =
 *            (xx + 0.5) * scale, xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), in);
 *            k[x] = bicubic((x + xmin - center + 0.5) * (1 / fs)), the Keys kernel with a = -0.5, divided by their left-to-right
 *            sum; fixed point (int)(k * 2^22 + 0.5), (int)(k * 2^22 - 0.5) for a negative k.  Built on the device.
 *   sample   clip8((2^21 + sum pixel * tap) >> 22) in int32, arithmetic shift
 * flags (enum cs_pil_flags):
 *   CS_PIL_IN_F32      `in` is float32 [n][h][w][c]; its codes are trunc(clip(255 * x, 0, 255)) (float32 product, :55)
 *   CS_PIL_GRAY        c = 3 in, ONE channel out: gray = trunc((r * 0.2989 + g * 0.5870) + b * 0.1140) in float64, in this
 *                      order (:419), before the resize.  Equal to the reference on every depth with three equal channels; its
 *                      own BLAS product differs from this order, and from itself between array shapes, on a few hundred of
 *                      the 2^24 colours.
 *   CS_PIL_OUT_PLANAR  out_f32 is planar [n][c][oh][ow] (what cs_inpaint_prepare takes) instead of [n][oh][ow][c]
 * out_u8: the codes, or null.  out_f32: code / 255.0f (a true division, :61), or null; interleaved rows start f32_row_pitch
 * floats apart (0: ow * channels; lets two eyes be written into one side-by-side frame).  Both null: nothing is done.
 * workspace: cs_pil_resize_workspace_bytes(n, h, w, c, oh, ow), 8-byte aligned.  in, out_u8, out_f32 and workspace must not
 * overlap (CS_EINVAL).  CS_ELIMIT before any device work: more than 65 535 frames, a side above 65 535, or a reduction whose
 * window has more than cs_pil_resize_max_taps() (257: a factor of 64) taps on an axis that is resampled.
 */
enum cs_pil_flags { CS_PIL_IN_F32 = 1, CS_PIL_GRAY = 2, CS_PIL_OUT_PLANAR = 4 };
CS_API size_t cs_pil_resize_workspace_bytes(int n, int h, int w, int c, int oh, int ow);
CS_API int cs_pil_resize_max_taps(void);
CS_API int cs_pil_resize(const void *in, int n, int h, int w, int c, int oh, int ow, int flags, uint8_t *out_u8,
                         float *out_f32, size_t f32_row_pitch, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The reference's Gaussian depth blurs (stereoimage_generation.py): a separable filter with replicate borders, rows then
 * columns, and a per-pixel blend of the depth with its blur.
 *   CS_GAUSS_PLAIN           blur_depth_map (:1253-1281): out = the blurred map
 *   CS_GAUSS_EDGE_SELECTIVE  edge_selective_blur_depth_map (:1283-1309): weight min(|3x3 Sobel gradient| / edge_threshold, 1)
 *   CS_GAUSS_LEFT            left_direction_aware_blur_depth_map (:1311-1327): weight min(g / edge_threshold, 1) where the
 *                            central horizontal difference g is positive, else 0
 *   CS_GAUSS_RIGHT           right_direction_aware_blur_depth_map (:1329-1344): the same where g is negative (|g|)
 * and out = (1 - weight) * depth + weight * blurred for the last three (float32, unfused).
 * depth [n][h][w] float32 -> out [n][h][w] float32.  taps: n_taps = 2 * radius + 1 float64 values in DEVICE memory (8-byte
 * aligned), applied as np.convolve(np.pad(line, radius, 'edge'), taps, 'valid'): float32 samples times float64 taps, the
 * products added in float64 one at a time in the order of the flipped tap array, the sum rounded to float32; the column pass
 * reads the float32 result of the row pass.  The library never computes taps: the caller evaluates the reference's numpy
 * expression (comfystereo_amd.engine.gaussian_taps).  edge_threshold is rounded to float32; CS_GAUSS_PLAIN ignores it.
 * workspace: cs_gaussian_blur_workspace_bytes(n, h, w, n_taps).  depth, out and workspace must not overlap.  Any h, w >= 1;
 * n_taps at most cs_gaussian_blur_max_taps() (4097: radius 2048), CS_ELIMIT beyond, and for calls of 2^24 workgroups or more
 * (one per 1024 columns of a row).
 */
enum cs_gauss_op { CS_GAUSS_PLAIN = 0, CS_GAUSS_EDGE_SELECTIVE = 1, CS_GAUSS_LEFT = 2, CS_GAUSS_RIGHT = 3 };
CS_API size_t cs_gaussian_blur_workspace_bytes(int n, int h, int w, int n_taps);
CS_API int cs_gaussian_blur_max_taps(void);
CS_API int cs_gaussian_blur(int op, const float *depth, const double *taps, int n_taps, double edge_threshold, int n, int h,
                            int w, float *out, void *workspace, size_t workspace_bytes, void *stream);

/*
 * forward_warp_mesh (reference stereoimage_generation.py:453-689), the mesh-quality warp the reference uses whenever
 * `moderngl` is importable (:1068-1071): same tensors as cs_forward_warp plus the culling threshold (reference
 * default 1.5).  The reference rasterises through OpenGL; the parts OpenGL leaves to the implementation are fixed as
 * documented in oracle/stereo_oracle.c (oracle_forward_warp_mesh) -- no bit parity with a particular GL driver is
 * claimed.  Needs h >= 2 and w >= 2.  Through cs_generate the same warp is selected by cs_params.flags bit 2 with
 * fill CS_FILL_GPU_WARP.  workspace: cs_warp_mesh_workspace_bytes(n, h, w).
 */
CS_API size_t cs_warp_mesh_workspace_bytes(int n, int h, int w);
CS_API int cs_forward_warp_mesh(const float *image, const float *depth, int n, int h, int w, double divergence_px,
                         double separation_px, double stereo_offset_exponent, double convergence_point,
                         double gradient_threshold, float *warped, uint8_t *gap_mask, void *workspace,
                         size_t workspace_bytes, void *stream);

/*
 * out[i] = codes[i] / 255 (float32, true division): expands a uint8 stereoscope (cs_params.flags bit 1), e.g.
 * after the frame shards of a multi-GPU job were all-gathered in their compact form
 * (= convertResult / np2tensor, reference GenerateStereo.py:41-44, 365-378).
 */
CS_API int cs_expand_u8(const uint8_t *codes, float *out, size_t count, void *stream);

/*
 * The compact node boundary of the host pipeline (replaces the float32 device -> host copies around
 * convertResult / np2tensor / generate_mask, reference GenerateStereo.py:41-44, 159-177, 355-378).
 * cs_pack_u8 (device): codes[i] = the uint8 code of values[i * stride] -- mode 0: value k / 255 -> k; mode 1: non-zero -> 1
 * (mask).  stride 3 takes one code per pixel of a depth map with three equal channels.
 * cs_host_expand_u8 (HOST memory, blocking, `threads` worker threads, 0 = one per online core up to 64):
 * out[i * replicate + r] = codes[i] / 255.0f (mode 0, true division) or codes[i] != 0 (mode 1), r < replicate <= 4.
 * Bit-identical to the float32 outputs of cs_generate for the CPU techniques.
 */
CS_API int cs_pack_u8(const float *values, uint8_t *codes, size_t count, int stride, int mode, void *stream);
CS_API int cs_host_expand_u8(const uint8_t *codes, float *out, size_t count, int replicate, int mode, int threads);
/* cs_host_copy (HOST memory, blocking): memcpy in `threads` contiguous slices (0 = one per online core up to 64) -- the
 * staging copy of a pageable input tensor into a pinned buffer (reference GenerateStereo.py:126-131, .to(device)). */
CS_API int cs_host_copy(void *dst, const void *src, size_t bytes, int threads);
/* gpu_warp's depth-map outputs are genuine floats on three EQUAL channels (reference GenerateStereo.py:165-169: clamp(0, 1),
 * unsqueeze(-1).expand): cs_take_f32 (device) keeps one channel -- out[i] = values[i * stride] -- so that 4 instead of 12
 * bytes per pixel cross PCIe, cs_host_replicate_f32 (HOST memory, blocking) writes out[i * replicate + r] = values[i],
 * r < replicate <= 4, with `threads` worker threads (0 = one per online core up to 64). */
CS_API int cs_take_f32(const float *values, float *out, size_t count, int stride, void *stream);
CS_API int cs_host_replicate_f32(const float *values, float *out, size_t count, int replicate, int threads);

/*
 * stereo_shift_torch (reference stereo_utils.py:15-88; callers stereodiffusion_nodes.py:650, :664): the depth-driven
 * forward shift of the `none` technique on a float payload -- diffusion latents.  input [b][c][h][w] float32, depth
 * [b][h][w] float32 (normalised with its global min / max like the reference, :36-45) -> out [2b][c][h][w]: the left
 * views (the input itself unless shift_both) followed by the right views; destinations nothing lands on stay 0.
 * torch.pow is exact for exponents 1 (the callers' value), 2 and 0.5; other exponents go through libm powf.
 */
CS_API size_t cs_stereo_shift_workspace_bytes(void);
CS_API int cs_stereo_shift(const float *input, const float *depth, int b, int c, int h, int w, double scale_factor,
                    int shift_both, double stereo_offset_exponent, float *out, void *workspace, size_t workspace_bytes,
                    void *stream);

/*
 * StereoDiffusion's Standard mode around its model (reference stereodiffusion_nodes.py:576-682): the latent shift as a plan
 * made once per image and one launch per shift step, and the decoded images' way to uint8 codes.  Nothing here waits for the
 * device or allocates, so a denoising step that uses them can be captured in a graph.
 *   cs_latent_shift_plan  the right view of cs_stereo_shift(shift_both = 0) as a table: disp [b][h][w] float32 (normalised with
 *     its global min / max, in cs_stereo_shift's arithmetic) -> src_col [b][h][w] int32, for every destination the source column
 *     the reference's sweep leaves there (scale_px = -scale_factor / 100 * w: the highest for a positive scale_factor), -1 where
 *     nothing lands.  workspace: cs_latent_shift_plan_workspace_bytes().  Made for latents (64 to a few hundred columns): a row's
 *     table lives in LDS and a destination scans the sources within |trunc(scale_px)| columns of it (the whole row for an
 *     exponent <= 0), w * reach LDS reads per row.  CS_ELIMIT: rows of more than 8 192 columns, more than 65 535 images.
 *   cs_latent_shift_apply  left, right, noise [b][c][h][w] of `dtype` (enum cs_latent_dtype), mask [b][h][w] uint8; values are
 *     moved, never computed.  CS_LATENT_FIRST (:650-660): right = left gathered through src_col, 0 in a hole; mask = (channel 0
 *     of that != 0), so a landed +-0.0 counts as a hole; with noise != NULL (deblur) right = noise on every channel where the
 *     mask is 0.  CS_LATENT_RESHIFT (:663-667): where the STORED mask is 1, right = left gathered; elsewhere right is left as it
 *     is (noise is ignored).  left and right may be the two halves of one tensor; right must not overlap left or noise.
 *   cs_decode_to_codes  image [n][c][h][w] of `dtype` -> codes [n][h][w][c] uint8 (:673-677): (x / 2 + 0.5) as torch computes
 *     it in the tensor's dtype (quotient and sum each rounded to it once), clamped to [0, 1], NaN -> 0, times 255.0f in float32,
 *     truncated.
 * CS_EINVAL before any launch: null pointers (noise may be NULL; mask may not, for either op), non-positive sizes, unknown dtype
 * or op, overlapping right.
 */
enum cs_latent_dtype { CS_LATENT_F32 = 0, CS_LATENT_F16 = 1, CS_LATENT_BF16 = 2 };
enum cs_latent_op { CS_LATENT_FIRST = 0, CS_LATENT_RESHIFT = 1 };
CS_API size_t cs_latent_shift_plan_workspace_bytes(void);
CS_API int cs_latent_shift_plan(const float *disp, int b, int h, int w, double scale_factor, double stereo_offset_exponent,
                         int32_t *src_col, void *workspace, size_t workspace_bytes, void *stream);
CS_API int cs_latent_shift_apply(const void *left, void *right, const int32_t *src_col, uint8_t *mask, const void *noise,
                          int dtype, int b, int c, int h, int w, int op, void *stream);
CS_API int cs_decode_to_codes(const void *image, int dtype, int n, int c, int h, int w, uint8_t *codes_nhwc, void *stream);

/*
 * Null-text inversion outside the UNet (reference inversion.py): what NullInversion.ddim_loop and NullInversion.null_optimization
 * do between two UNet calls, one launch each.  Flat tensors of `count` elements of `dtype` (enum cs_latent_dtype).  Every operation
 * of the reference's tensor expression is one operation here, rounded once to the dtype before the next (float32: plain IEEE;
 * half types: the operation in float32, then the conversion): the results are the bits CPU torch gives.  The coefficients are
 * float32 values passed as doubles:  c1 = sqrt(1 - a_t), c2 = sqrt(a_t), c3 = sqrt(1 - a_other), c4 = sqrt(a_other); prev_step
 * (:57-65) and next_step (:67-75) differ only in which two alphas the host takes.
 *   cs_ddim_step  e = eps_a + guidance * (eps_b - eps_a) (:88; eps_b NULL: e = eps_a);
 *     out = c4 * ((sample - c1 * e) / c2) + c3 * e.  out may be sample itself.
 *   cs_null_loss_grad  the inner step of null_optimization (:198-201): rec = that formula with eps_a = eps_uncond, eps_b =
 *     eps_cond, sample = latent_cur; loss[0] = mean((rec - latent_prev)^2), one float32, every difference taken from the formula in
 *     float64 before its roundings to the dtype, the squares summed in float32 in a fixed order without
 *     atomics (two launches of it give the same bits); grad = d loss / d eps_uncond = (2 / count) * (rec - latent_prev) *
 *     (c3 - c4 * c1 / c2) * (1 - guidance), in the dtype.  workspace: cs_null_loss_workspace_bytes(count), 0 (workspace may be
 *     NULL) up to 32 768 elements, where one launch does everything.
 *   cs_adam_step  one torch.optim.Adam step (no weight decay, no amsgrad, not maximising) in place on param, exp_avg and
 *     exp_avg_sq; step counts from 1; the bias corrections are computed in double on the host, the moments are kept in the dtype.
 * CS_EINVAL before any launch: null pointers (eps_b may be NULL), count <= 0, unknown dtype, non-finite coefficients, c2 = 0,
 * step < 1, betas outside [0, 1), misaligned or overlapping tensors.
 */
CS_API int cs_ddim_step(const void *sample, const void *eps_a, const void *eps_b, void *out, int dtype, long long count,
                        double guidance, double c1, double c2, double c3, double c4, void *stream);
CS_API size_t cs_null_loss_workspace_bytes(long long count);
CS_API int cs_null_loss_grad(const void *eps_uncond, const void *eps_cond, const void *latent_cur, const void *latent_prev,
                             void *rec, float *loss, void *grad, int dtype, long long count, double guidance, double c1, double c2,
                             double c3, double c4, void *workspace, size_t workspace_bytes, void *stream);
CS_API int cs_adam_step(void *param, const void *grad, void *exp_avg, void *exp_avg_sq, int dtype, long long count, double lr,
                        double beta1, double beta2, double eps, int step, void *stream);

/*
 * Null-text optimisation on F frames at once: the two calls above with a frame axis, for a UNet that runs `frames` frames in one
 * batch while every frame keeps its own loss, its own early stop and its own Adam state.  Tensors are [frames][per] contiguous.
 *   cs_null_loss_grad_frames  per frame f with active_in[f] != 0: rec[f], grad[f] and loss[f] (float32 [frames]) are bit for bit
 *     what cs_null_loss_grad gives on that frame's `per` elements alone (the same blocks counted from the frame's first element,
 *     the same summation tree, count = per), and active_out[f] = !((double)loss[f] < threshold): the reference's early stop
 *     `loss.item() < epsilon + i * 2e-5` (:205-208), made in float64 on the device -- a loss at the threshold, or a NaN, does not
 *     stop the frame.  Per frame with active_in[f] == 0: grad[f] is zeros, rec[f] and loss[f] are not touched, active_out[f] = 0.
 *     active_in and active_out are uint8 [frames] and two different buffers (swap them between inner steps).  One launch, and a
 *     second one when per > 32 768; no atomics.  workspace: cs_null_loss_frames_workspace_bytes(frames, per): two floats per
 *     block of 32 768 elements and frame when per > 32 768, else 0 (workspace may be NULL).
 *   cs_adam_step_frames  cs_adam_step, with the same coefficients and step number for all frames, on the rows of the frames with
 *     active[f] != 0; the four rows of every other frame are not written at all.  One launch.
 * CS_EINVAL before any launch: null pointers, frames <= 0 or per <= 0, unknown dtype, active_out == active_in, a NaN threshold,
 * and what the single-tensor calls refuse; CS_ELIMIT: frames > 65 535 (the grid's second dimension), per above
 * cs_null_loss_grad's limit.
 */
CS_API size_t cs_null_loss_frames_workspace_bytes(long long frames, long long per);
CS_API int cs_null_loss_grad_frames(const void *eps_uncond, const void *eps_cond, const void *latent_cur, const void *latent_prev,
                                    void *rec, float *loss, void *grad, const uint8_t *active_in, uint8_t *active_out, int dtype,
                                    long long frames, long long per, double guidance, double c1, double c2, double c3, double c4,
                                    double threshold, void *workspace, size_t workspace_bytes, void *stream);
CS_API int cs_adam_step_frames(void *param, const void *grad, void *exp_avg, void *exp_avg_sq, const uint8_t *active, int dtype,
                               long long frames, long long per, double lr, double beta1, double beta2, double eps, int step,
                               void *stream);

/*
 * StereoDiffusion's Fast mode outside its models (reference model_wrappers.py ComfyUIInpaintRunner.__call__, :522-641): the tensor
 * work before and inside the inpainting loop, around ONE persistent UNet input
 *   x [2n][9][hl][wl] of `dtype` (enum cs_latent_dtype): the uncond half (n frames), then the cond half -- the layout of
 *   torch.cat([latent_model_input] * 2); per frame the latents (channels 0..3), the mask at the latents' size (4) and the masked
 *   image's latents (5..8).  Channels 4..8 are written once, channels 0..3 by every step.
 * Arithmetic as cs_ddim_step: every operation of the reference's tensor expression is one operation, rounded once to the dtype
 * before the next; coefficients are passed as doubles and used as float32.  Nothing here waits for the device or allocates; one
 * launch each; 16-byte accesses where the pointers and hl * wl (h * w) allow.
 *   cs_inpaint_image_prep  (:562-572, :580) filled [n][h][w][3] uint8 codes, mask [n][h][w] uint8 (0 / non-zero) ->
 *     img [n][3][h][w] = to_dtype((float32(code) / 255.0f) * 2.0f - 1.0f); masked = img * (1 - m) in the dtype (a negative pixel
 *     under the mask is -0.0); channel 4 of both halves of x = the mask at torch's nearest source index, floor(dst * (in / out))
 *     with the float32 scale.
 *   cs_inpaint_latent_init  (:575-602) mean_img, mean_masked [n][4][hl][wl] of `mean_dtype` (what the VAE returned), noise of
 *     `dtype` or NULL -> img_latent = to_dtype(mean_img * 0.18215) (the product in mean_dtype), to a tensor of its own;
 *     channels 0..3 of both halves of x = sa * img_latent + sb * noise (scheduler.add_noise: product, product, sum), or
 *     img_latent with noise NULL (an empty timestep list); channels 5..8 = to_dtype(mean_masked * 0.18215); with decode_in !=
 *     NULL also decode_in [n][4][hl][wl] = latents / 0.18215 (:628), for a loop of no step.
 *   cs_inpaint_plms_step  (:621-625) noise_pred [2n][4][hl][wl]: u (first half), t (second);  e = u + guidance * (t - u);
 *     m by `kind` from e and the earlier predictions e1 (the latest), e2, e3:
 *       CS_PLMS_FIRST   m = e; cur_sample = the sample             CS_PLMS_SECOND  m = (e + e1) / 2; the sample is cur_sample
 *       CS_PLMS_ORDER2  m = (3 e - e1) / 2                         CS_PLMS_ORDER3  m = (23 e - 16 e1 + 5 e2) / 12
 *       CS_PLMS_ORDER4  m = (1 / 24) * (55 e - 59 e1 + 37 e2 - 9 e3)
 *     prev = sc * sample - da * m / denom, the sample being channels 0..3 of x's first half; prev goes into channels 0..3 of
 *     both halves of x; e into e_out (every kind but SECOND, whose prediction is not kept; the slot of a ring of four the host
 *     turns); with decode_in != NULL also decode_in = prev / 0.18215 (:628), for the last step.  e_out, e1..e3, cur_sample,
 *     decode_in: [n][4][hl][wl].  Pointers the kind does not use may be NULL.
 * CS_EINVAL before any launch: null pointers, non-positive sizes, unknown dtype or kind, misaligned tensors, outputs that overlap
 * each other or an input, non-finite coefficients, denom == 0.
 */
enum cs_plms_kind { CS_PLMS_FIRST = 0, CS_PLMS_SECOND = 1, CS_PLMS_ORDER2 = 2, CS_PLMS_ORDER3 = 3, CS_PLMS_ORDER4 = 4 };
CS_API int cs_inpaint_image_prep(const uint8_t *filled, const uint8_t *mask, int n, int h, int w, int hl, int wl, int dtype,
                                 void *img, void *masked, void *x, void *stream);
CS_API int cs_inpaint_latent_init(const void *mean_img, const void *mean_masked, int mean_dtype, const void *noise, int dtype,
                                  int n, int hl, int wl, double sa, double sb, void *x, void *img_latent, void *decode_in,
                                  void *stream);
CS_API int cs_inpaint_plms_step(const void *noise_pred, void *x, int dtype, int n, int hl, int wl, int kind, double guidance,
                                double sc, double da, double denom, void *e_out, const void *e1, const void *e2, const void *e3,
                                void *cur_sample, void *decode_in, void *stream);

/*
 * Fast mode's loop for few-step models (SD-Turbo, LCM checkpoints): the samplers such a model was trained for, around the same
 * persistent UNet input, one launch per step.
 *   x [halves * n][channels][hl][wl] of `dtype`: halves = 2 under classifier-free guidance (cfg != 0: uncond half, cond half), 1
 *   without (the conditional batch alone; noise_pred is then the prediction itself).  channels = 9: an inpainting UNet, channels
 *   4..8 written once as above.  channels = 4: an ordinary UNet used RePaint-style -- after every step
 *   lat = mask_l != 0 ? prev : keep, a select (values are moved, not multiplied), keep being the image's latents at the next
 *   noise level: Euler img_latent + sigma_next * noise0, LCM sqrt(a_next) * img_latent + sqrt(1 - a_next) * noise0, on the last
 *   step img_latent.
 * Arithmetic: e = u + guidance * (t - u) in the dtype as in cs_inpaint_plms_step; everything after it in float32 on the dtype's
 * values with the coefficients as float32, one IEEE operation each, no contraction, and one rounding to the dtype per stored
 * tensor.  The specification of the bits is tools/fewstep_oracle.py on CPU torch.
 *   CS_FEWSTEP_EULER  (Karras et al. 2022, Alg. 1 without churn)  k0 = sigma_next - sigma_t, k1 = sqrt(sigma_next^2 + 1),
 *     k2 = sigma_next:  prev = state + e * k0;  state = lat (the un-scaled sample, a buffer of its own);  channels 0..3 of x =
 *     lat / k1, the NEXT step's scale_model_input (on the last step sigma_next = 0, k1 = 1).
 *   CS_FEWSTEP_LCM  (Luo et al. 2023, multistep consistency sampling)  k0 = sqrt(1 - a_t), k1 = sqrt(a_t), k2 = c_out,
 *     k3 = c_skip, k4 = sqrt(a_next), k5 = sqrt(1 - a_next); s = channels 0..3 of x's first half:  x0 = (s - k0 * e) / k1;
 *     den = k2 * x0 + k3 * s;  prev = k4 * den + k5 * step_noise, with last != 0 prev = den;  channels 0..3 of x = lat.
 *   decode_in != NULL: also decode_in = lat / 0.18215 (float32 lat, rounded once).  state, step_noise, img_latent, noise0,
 *   decode_in: [n][4][hl][wl]; mask_l [n][hl][wl], 0 / 1 in `dtype`.  Pointers the sampler, the layout or the step does not use
 *   may be NULL.
 *   cs_inpaint_fewstep_init: the first latents from img_latent (cs_inpaint_latent_init's) and the initial noise.  Euler (k0 =
 *     sigma_0, k1 = sqrt(sigma_0^2 + 1)): state = img_latent + k0 * noise, x = that / k1.  LCM (k0, k1 = add_noise's two roots in
 *     the dtype): x = k0 * img_latent + k1 * noise, every operation rounded to the dtype as in cs_inpaint_latent_init.  noise
 *     NULL (no timestep left): x = img_latent.  channels = 4: mask_l = channel 4 of x9 [2n][9][hl][wl], where
 *     cs_inpaint_image_prep put the mask at the latents' size.
 * CS_EINVAL before any launch: null pointers, non-positive sizes, unknown dtype or sampler, channels other than 9 or 4, a pointer
 * the sampler, layout or step needs missing (state for Euler, step_noise for an LCM step that is not the last, img_latent / mask_l /
 * noise0 for 4 channels), misaligned tensors, outputs that overlap each other or an input, non-finite coefficients, k1 == 0.
 */
enum cs_fewstep_sampler { CS_FEWSTEP_EULER = 0, CS_FEWSTEP_LCM = 1 };
CS_API int cs_inpaint_fewstep_init(const void *img_latent, const void *noise, const void *x9, int dtype, int n, int hl, int wl,
                                   int channels, int cfg, int sampler, double k0, double k1, void *x, void *state, void *mask_l,
                                   void *stream);
CS_API int cs_inpaint_fewstep_step(const void *noise_pred, void *x, int dtype, int n, int hl, int wl, int channels, int sampler,
                                   int cfg, int last, double guidance, double k0, double k1, double k2, double k3, double k4,
                                   double k5, void *state, const void *step_noise, const void *img_latent, const void *noise0,
                                   const void *mask_l, void *decode_in, void *stream);

/*
 * StereoDiffusion's Standard mode between two UNet calls (reference stereodiffusion_nodes.py:624-667 with diffusion_utils.py:29-66):
 * classifier-free guidance, the DDIM step and the latent shift in ONE launch, around one persistent UNet input
 *   x [4b][c][h][w] of `dtype` (enum cs_latent_dtype): rows 0..b-1 the left views, b..2b-1 the right views -- the current
 *   latents --, rows 2b..4b-1 their copy for the conditional half, the layout of torch.cat([latents] * 2).
 *   noise_pred [4b][c][h][w]: the UNet's answer, the unconditional half first.
 * cs_standard_step: e = u + guidance * (c - u); new = c4 * ((x - c1 * e) / c2) + c3 * e, every operation rounded exactly as
 * cs_ddim_step rounds it (one statement of the arithmetic serves both); then by `op` what cs_latent_shift_apply does to the
 * pair (new left, new right):
 *   CS_STANDARD_NONE     nothing.
 *   CS_STANDARD_FIRST    right = new left gathered through src_col, 0 in a hole; mask = (channel 0 of that != 0); with noise !=
 *                        NULL right = noise [b][c][h][w] on every channel where the mask is 0.
 *   CS_STANDARD_RESHIFT  where the STORED mask is 1, right = new left gathered; elsewhere right keeps its own step.
 * The result is written to both halves of x.  It is, bit for bit and for every value, cs_ddim_step on the two halves, then
 * cs_latent_shift_apply, then the copy.  src_col int32 [b][h][w] (cs_latent_shift_plan's), mask uint8 [b][h][w]; both may be
 * NULL for CS_STANDARD_NONE.  One workgroup owns a row of both views and gathers from its own copy of the new left row, so the
 * result does not depend on the order in which anything runs.  Nothing here waits for the device or allocates; 16-byte
 * accesses where w and the pointers allow.
 * CS_EINVAL before any launch: null pointers, non-positive sizes, unknown dtype or op, noise without CS_STANDARD_FIRST,
 * non-finite coefficients, c2 = 0, misaligned or overlapping tensors.  CS_ELIMIT: rows of more than 8 192 columns
 * (cs_latent_shift_plan's limit), b * h or c * w beyond 2^31 - 1.
 */
enum cs_standard_op { CS_STANDARD_NONE = 0, CS_STANDARD_FIRST = 1, CS_STANDARD_RESHIFT = 2 };
CS_API int cs_standard_step(void *x, const void *noise_pred, int dtype, int b, int c, int h, int w, double guidance, double c1,
                            double c2, double c3, double c4, int op, const int32_t *src_col, uint8_t *mask, const void *noise,
                            void *stream);

/*
 * The same four steps for a model that predicts something else than the noise (`prediction`: enum cs_prediction).  With
 * CS_PRED_EPSILON each is its namesake above, bit for bit.  With CS_PRED_V the model's answer is v = c2 * eps - c1 * x0 (Salimans &
 * Ho, "Progressive Distillation for Fast Sampling of Diffusion Models", 2022; the SD 2.x 768-v checkpoints); guidance is applied
 * to the raw answers as before, v = eps_a + guidance * (eps_b - eps_a), and the step is
 *     x0 = c2 * sample - c1 * v;   e = c2 * v + c1 * sample;   out = c4 * x0 + c3 * e
 * -- the operation order of diffusers' DDIMScheduler.step with prediction_type "v_prediction", eta 0 -- every operation rounded
 * once to the dtype as above.  c2 is the first operand of two products and divides nothing: c2 = 0 is no error under CS_PRED_V.
 * The loss of cs_null_loss_grad_pred is taken from that formula in float64 in the same fixed order, and
 * grad = d loss / d eps_uncond = (2 / count) * (rec - latent_prev) * (c3 * c2 - c4 * c1) * (1 - guidance).
 * CS_EINVAL before any launch: an unknown prediction, and everything the namesake refuses (c2 = 0 under CS_PRED_EPSILON only).
 */
enum cs_prediction { CS_PRED_EPSILON = 0, CS_PRED_V = 1 };
CS_API int cs_ddim_step_pred(const void *sample, const void *eps_a, const void *eps_b, void *out, int dtype, long long count,
                             double guidance, double c1, double c2, double c3, double c4, int prediction, void *stream);
CS_API int cs_null_loss_grad_pred(const void *eps_uncond, const void *eps_cond, const void *latent_cur, const void *latent_prev,
                                  void *rec, float *loss, void *grad, int dtype, long long count, double guidance, double c1,
                                  double c2, double c3, double c4, int prediction, void *workspace, size_t workspace_bytes,
                                  void *stream);
CS_API int cs_null_loss_grad_frames_pred(const void *eps_uncond, const void *eps_cond, const void *latent_cur,
                                         const void *latent_prev, void *rec, float *loss, void *grad, const uint8_t *active_in,
                                         uint8_t *active_out, int dtype, long long frames, long long per, double guidance,
                                         double c1, double c2, double c3, double c4, int prediction, double threshold,
                                         void *workspace, size_t workspace_bytes, void *stream);
CS_API int cs_standard_step_pred(void *x, const void *noise_pred, int dtype, int b, int c, int h, int w, double guidance,
                                 double c1, double c2, double c3, double c4, int prediction, int op, const int32_t *src_col,
                                 uint8_t *mask, const void *noise, void *stream);

/*
 * Stereo attention (reference stereo_utils.py BNAttention :91-188, the hot path of StereoDiffusion's Standard mode): one fused
 * flash-style forward attention, float32 in and out, float32 accumulation on the f32-input MFMA; no score matrix is written,
 * there is no workspace, nothing is allocated, everything runs on the caller's stream.
 *   q [(c s b h)][n][d], k and v [(c s b h)][n_k][d], out [(c s b)][n][(h d)] -- c: CFG chunks (1 or 2), s: views (1 or 2),
 *   b: samples, h: heads, n / n_k: query / key tokens per view; all contiguous float32, 16-byte aligned.
 *   out = softmax(scale * q . k^T) . v over the keys `mode` selects for the query (c, s, b, h, i):
 *     CS_ATTN_SELF  (c, s, b, h, 0..n_k-1): ordinary attention, n_k may differ from n (:137-140)
 *     CS_ATTN_UNI   (c, 0, b, h, 0..n-1): both views see the left view's keys (:163-171)
 *     CS_ATTN_BI    (c, 0, b, h, .) followed by (c, 1, b, h, .), 2 n keys (:156-162; the no-CFG path :142-146 with c = 1)
 * CS_EINVAL: null or misaligned pointers, non-positive sizes, unknown mode, UNI / BI with s != 2 or n_k != n, out aliasing an
 * input.  CS_ELIMIT: d not a multiple of 4 or above cs_stereo_attention_max_head_dim() (160), sizes beyond 32-bit grids.
 * Forward only (the differentiable CS_ATTN_SELF form is cs_attention_fwd_lse / cs_attention_bwd below).
 */
enum cs_attn_mode { CS_ATTN_SELF = 0, CS_ATTN_UNI = 1, CS_ATTN_BI = 2 };
CS_API int cs_stereo_attention_max_head_dim(void);
CS_API int cs_stereo_attention(const float *q, const float *k, const float *v, float *out, int c, int s, int b, int h, int n,
                        int n_k, int d, double scale, int mode, void *stream);

/*
 * The same attention on float16 or bfloat16 tensors (the dtypes diffusion pipelines run in), on the half-input MFMA: q, k, v
 * and out are all `dtype` (enum cs_attn_dtype), in cs_stereo_attention's layouts and with its modes.  The scores, the online
 * softmax and both accumulators are float32; only the matrix operands (q, k, v, and the probabilities after the exponential)
 * are half; the final division is float32 and the store rounds to nearest-even.  No score matrix, no workspace, the caller's
 * stream.  Refusals are cs_stereo_attention's, and nothing is written on a refusal; in addition CS_EINVAL: unknown dtype;
 * CS_ELIMIT: d not a multiple of 8 (every row 16-byte aligned).  Forward only.
 */
enum cs_attn_dtype { CS_ATTN_F16 = 0, CS_ATTN_BF16 = 1 };
CS_API int cs_stereo_attention_half(const void *q, const void *k, const void *v, void *out, int dtype, int c, int s, int b, int h,
                             int n, int n_k, int d, double scale, int mode, void *stream);

/*
 * The fused attention with a backward pass (reference diffusion_utils.py register_attention_control :158-292, the attention
 * the UNet runs under NullInversion.invert, inversion.py:214-262, whose null-text optimisation differentiates through every
 * layer).  float32, CS_ATTN_SELF semantics only: q, dq [(b h)][n][d]; k, v, dk, dv [(b h)][n_k][d] (n_k may differ from n);
 * out, d_out [(b)][n][(h d)]; lse [(b h)][n]; all contiguous, 16-byte aligned.
 *   cs_attention_fwd_lse  cs_stereo_attention(..., c = 1, s = 1, CS_ATTN_SELF) -- `out` is bit for bit that call's -- which also
 *     stores lse(i) = log2 sum_j exp2(scale * log2(e) * q_i . k_j): the log-sum-exp of the scaled scores in LOG2 units
 *     (natural-log value = lse * ln 2), the unit the kernels' exponentials work in.
 *   cs_attention_bwd      dq, dk, dv of sum(out * d_out) from q, k, v and the forward's out and lse.  The probabilities are
 *     recomputed tile by tile as exp2(scale * log2(e) * s - lse); nothing of size n x n_k is stored.  Three kernels on the
 *     caller's stream (row sums of d_out * out into the workspace; dk and dv; dq); every gradient element is accumulated by one
 *     lane in a fixed order, there are no atomics, and results are bit-identical from run to run.
 * No allocation.  Refusals are cs_stereo_attention's, and nothing is written on a refusal.  CS_EINVAL: null or misaligned
 * pointers, non-positive sizes, non-finite scale, an output (out, lse; dq, dk, dv, the workspace) overlapping an input or another
 * output.  CS_ELIMIT: d not a multiple of 4 or above cs_stereo_attention_max_head_dim() (160), sizes beyond 32-bit grids.
 * CS_EWORKSPACE: workspace_bytes < cs_attention_bwd_workspace_bytes (which is 0 for non-positive sizes).
 */
CS_API int cs_attention_fwd_lse(const float *q, const float *k, const float *v, float *out, float *lse, int b, int h, int n,
                         int n_k, int d, double scale, void *stream);
CS_API size_t cs_attention_bwd_workspace_bytes(int b, int h, int n, int n_k, int d);
CS_API int cs_attention_bwd(const float *q, const float *k, const float *v, const float *out, const float *lse, const float *d_out,
                     float *dq, float *dk, float *dv, int b, int h, int n, int n_k, int d, double scale, void *workspace,
                     size_t workspace_bytes, void *stream);

/*
 * The same pair on float16 or bfloat16 tensors (the dtype null-text optimisation runs in on a half model), on the half-input
 * MFMA and with no conversion pass: q, k, v, out, d_out, dq, dk, dv are all `dtype` (enum cs_attn_dtype) in the layouts of
 * cs_attention_fwd_lse / cs_attention_bwd; lse and the workspace are float32.
 *   cs_attention_half_fwd_lse  cs_stereo_attention_half(..., c = 1, s = 1, CS_ATTN_SELF) -- `out` is bit for bit that call's -- which
 *     also stores lse(i) = log2 sum_j exp2(scale * log2(e) * q_i . k_j) as float32, from the kernel's float32 running maximum and sum.
 *   cs_attention_half_bwd      dq, dk, dv of sum(out * d_out).  All five matrix products (S, dP, dV, dK, dQ) take half operands: q, k,
 *     v, d_out as given, and the recomputed probabilities and dS rounded to `dtype` after the float32 arithmetic that forms them;
 *     row sums, exponentials and every accumulator are float32.  Three kernels on the caller's stream, no atomics, each gradient
 *     element accumulated by one lane in a fixed order and rounded to nearest-even once: bit-identical from run to run.
 * No allocation.  Refusals are those of the float32 pair (sizes in bytes follow the dtype), and nothing is written on a refusal;
 * in addition CS_EINVAL: unknown dtype; CS_ELIMIT: d not a multiple of 8.  CS_EWORKSPACE: workspace_bytes <
 * cs_attention_half_bwd_workspace_bytes (which is 0 for non-positive sizes).
 */
CS_API int cs_attention_half_fwd_lse(const void *q, const void *k, const void *v, void *out, float *lse, int dtype, int b, int h,
                              int n, int n_k, int d, double scale, void *stream);
CS_API size_t cs_attention_half_bwd_workspace_bytes(int b, int h, int n, int n_k, int d);
CS_API int cs_attention_half_bwd(const void *q, const void *k, const void *v, const void *out, const float *lse, const void *d_out,
                          void *dq, void *dk, void *dv, int dtype, int b, int h, int n, int n_k, int d, double scale,
                          void *workspace, size_t workspace_bytes, void *stream);

/*
 * Temporal depth stabilisation of a video batch (not in the reference, which normalises every frame alone): a causal,
 * motion-adaptive, scene-cut-aware filter along t, run in front of cs_generate.  DESIGN.md section 5 has the specification,
 * tools/temporal_oracle.py states it in numpy.  float32 throughout, every operation rounded once.
 *   depth [n][h][w][c] float32; g = the gray value cs_params.depth_c describes (c == 3: gray, c == 1: the value, else channel 0)
 *   m_t   = mean over the pixels of |g_t - g_{t-1}|; frame 0's predecessor is state_prev_raw if *state_valid, else there is none
 *   cut_t = m_t > cut_threshold (a NaN mean is no cut); a frame without predecessor is a cut and has m = 0
 *   y_t   = g_t  if cut_t or !(|g_t - y_{t-1}| < motion_threshold),  else  y_{t-1} + alpha * (g_t - y_{t-1});  y_{-1} = state_prev
 * out [n][h][w] float32 = y; m_out [n] float32; cut_out [n] int32 (0 / 1).  The state -- state_prev_raw [h][w], state_prev [h][w]
 * float32 and state_valid, one int32, all in DEVICE memory -- is read and then overwritten with the last frame's g and y and
 * with 1, so a clip fed in sub-batches gives bit for bit what one call gives; the caller zeroes *state_valid to start a clip.
 * m_t is added up in an order that depends on h * w alone, without atomics: bit-identical from run to run and for a frame pair
 * inside one call or across two.  alpha, motion_threshold and cut_threshold are rounded to float32; alpha in [0, 1], the
 * thresholds >= 0 (+inf allowed), else CS_EINVAL, as for a null pointer, a non-positive size or a buffer off the 4-byte grid.
 * No two of depth, out, the three state buffers, m_out, cut_out and workspace may overlap (CS_EINVAL).  CS_ELIMIT: n > 65535 or h * w >= 2^31.  CS_EWORKSPACE: workspace_bytes <
 * cs_temporal_depth_workspace_bytes(n, h, w, c) (0 for non-positive sizes).  Every refusal precedes the first launch; the
 * three launches go to `stream`, nothing waits for the device, and the call can be captured into a graph.
 */
CS_API size_t cs_temporal_depth_workspace_bytes(int n, int h, int w, int c);
CS_API int cs_temporal_depth(const float *depth, int n, int h, int w, int c, double alpha, double motion_threshold,
                             double cut_threshold, float *state_prev_raw, float *state_prev, int32_t *state_valid, float *out,
                             float *m_out, int32_t *cut_out, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Motion-compensated temporal depth stabilisation of a video batch (not in the reference): cs_temporal_depth's filter, with
 * y_{t-1} read where the pixel's block came from, so that moving content is filtered as well.  The motion is found on the 8-bit
 * luma of the clip's colour frames by a full-search block matcher.  DESIGN.md section 5 has the specification,
 * tools/motion_oracle.py states it in numpy.  Integers in the search; float32, every operation rounded once, in the filter.
 *   depth [n][h][w][c] float32 and g, m_t, cut_t as for cs_temporal_depth; guide [n][h][w][3] float32, the colour frames at
 *   the depth's size
 *   code(v)  = uint8(trunc(min(max(v, 0), 1) * 255 + 0.5)), NaN -> 0;  L = (77 code(R) + 150 code(G) + 29 code(B) + 128) >> 8
 *   blocks   16 x 16 from the top-left corner, clipped at the right and bottom edge: Hb = ceil(h / 16), Wb = ceil(w / 16)
 *   v_t(b)   the (dx, dy) with |dx|, |dy| <= search_range for which every pixel of the block, displaced, lies inside the frame, that
 *            minimises (sad + smoothness (|dx| + |dy|), |dx| + |dy|, |dy|, dy, dx) lexicographically;
 *            sad = sum over the block of |L_t(p) - L_{t-1}(p + (dx, dy))|
 *   matched  sad(v) <= match_threshold * (the block's pixel count)
 *   q        = y_{t-1}(p + v_t(block(p)))
 *   y_t(p)   = g_t(p)  if cut_t, the block is unmatched or !(|g_t(p) - q| < motion_threshold),  else  q + alpha * (g_t(p) - q)
 * out [n][h][w] float32 = y; m_out [n] float32; cut_out [n] int32; vec_out [n][Hb][Wb][2] int8 (dx, dy); sad_out [n][Hb][Wb]
 * int32; matched_out [n][Hb][Wb] uint8 (0 / 1).  The vectors of a cut frame are computed all the same.  The state -- state_prev_raw,
 * state_prev [h][w] float32, state_prev_luma [h][w] uint8 and state_valid, one int32, all in DEVICE memory -- is read and then
 * overwritten with the last frame's g, y and L and with 1, so a clip fed in sub-batches gives bit for bit what one call gives; the
 * caller zeroes *state_valid to start a clip.  Frame 0 without a valid state is a cut with m = 0, vectors and SADs 0, every block
 * matched.  With search_range 0 and match_threshold 255, out, m_out, cut_out and the two float state arrays are cs_temporal_depth's
 * bit for bit.  alpha in [0, 1], the thresholds >= 0 (+inf allowed), search_range 0..32, smoothness 0..4096, match_threshold
 * 0..255, else CS_EINVAL, as for a null pointer, a non-positive size, a buffer of 4-byte elements off the 4-byte grid, or any two
 * buffers that overlap.  CS_ELIMIT: n > 65535 or h * w >= 2^31.  CS_EWORKSPACE: workspace_bytes <
 * cs_motion_depth_workspace_bytes(n, h, w, c, search_range) (0 for non-positive sizes or a search_range out of range).  Every
 * refusal precedes the first launch; the 3 + n launches (and, for n == 1, one device-to-device copy) go to `stream`, nothing waits
 * for the device, nothing is allocated, and the call can be captured into a graph.
 */
CS_API size_t cs_motion_depth_workspace_bytes(int n, int h, int w, int c, int search_range);
CS_API int cs_motion_depth(const float *depth, const float *guide, int n, int h, int w, int c, double alpha, double motion_threshold,
                           double cut_threshold, int search_range, int smoothness, int match_threshold, float *state_prev_raw,
                           float *state_prev, uint8_t *state_prev_luma, int32_t *state_valid, float *out, float *m_out,
                           int32_t *cut_out, int8_t *vec_out, int32_t *sad_out, uint8_t *matched_out, void *workspace,
                           size_t workspace_bytes, void *stream);

/*
 * cs_motion_depth with a wide-range, coarse-to-fine motion search (not in the reference): the same filter, outputs, state and
 * buffers, but the vectors reach |dx|, |dy| <= search_range + 3 with search_range a multiple of 4 in 4..120 (the full search stops
 * at 32 and costs (2 S + 1)^2 SADs per block).  DESIGN.md section 5 has the specification, tools/motion_pyramid_oracle.py states
 * it in numpy.
 *   planes     L0 = L above;  L(k+1)(y, x) = (a + b + c + d + 2) >> 2 over the 2 x 2 cell of Lk, Lk edge-replicated to even sizes:
 *              ceil(h_k / 2) x ceil(w_k / 2), levels 0, 1, 2
 *   blocks     16 x 16 from the top-left corner of every level's own plane, clipped at the right and bottom edge; the parent of
 *              level-k block (by, bx) is level-(k+1) block (by >> 1, bx >> 1)
 *   level 2    cs_motion_depth's full search on L2 with search_range / 4
 *   level 1, 0 a block's candidates are (0, 0) and 2 v + (ex, ey), |ex|, |ey| <= 1, for v the level above's vector of its parent and
 *              of the parent's up, down, left and right neighbours that exist: at most 46 distinct ones.  Among those for which
 *              every pixel of the block, displaced, lies inside the level's plane the winner minimises
 *              (sad + smoothness (|dx| + |dy|), |dx| + |dy|, |dy|, dy, dx) on the level's own vector and SAD
 *   vec_out, sad_out (without the penalty) and matched_out = sad <= match_threshold * (the block's pixel count) are level 0's
 * The state is cs_motion_depth's (the two calls may continue each other's clip); the pyramid of its luma is rebuilt per call, so a
 * clip fed in sub-batches gives bit for bit what one call gives.  Frame 0 without a valid state, the vectors of a cut frame, the
 * ranges of the other parameters, every refusal and its code are cs_motion_depth's; search_range outside its set is CS_EINVAL.
 * CS_EWORKSPACE: workspace_bytes < cs_motion_depth_pyramid_workspace_bytes(n, h, w, c, search_range) (0 for non-positive sizes or a
 * search_range outside the set).  Every refusal precedes the first launch; the 6 + n launches (and, for n == 1, one
 * device-to-device copy) go to `stream`, nothing waits for the device, nothing is allocated, no atomics, and the call can be
 * captured into a graph.
 */
CS_API size_t cs_motion_depth_pyramid_workspace_bytes(int n, int h, int w, int c, int search_range);
CS_API int cs_motion_depth_pyramid(const float *depth, const float *guide, int n, int h, int w, int c, double alpha,
                                   double motion_threshold, double cut_threshold, int search_range, int smoothness, int match_threshold,
                                   float *state_prev_raw, float *state_prev, uint8_t *state_prev_luma, int32_t *state_valid, float *out,
                                   float *m_out, int32_t *cut_out, int8_t *vec_out, int32_t *sad_out, uint8_t *matched_out,
                                   void *workspace, size_t workspace_bytes, void *stream);

/*
 * Depth range clipping of a video batch (not in the reference, which normalises every frame by its own extremes, so a few outlier
 * pixels flatten the scene and flickering extremes make it pump): two order statistics of the gray depth per frame, smoothed
 * along t, and a clamp to them, run in front of cs_generate.  DESIGN.md section 5 has the specification, tools/range_oracle.py
 * states it in numpy.  float32 throughout, every operation rounded once.
 *   depth [n][h][w][c] float32; g = the gray value cs_params.depth_c describes (c == 3: gray, c == 1: the value, else channel 0)
 *   key(x)   = bits(x) ^ 0x80000000 if the sign bit is clear, else ~bits(x) (uint32; -0 below +0, NaNs where their bits put them)
 *   raw_lo_t = the element of g_t whose key has rank rank_lo (0-based) among the frame's h * w keys; raw_hi_t likewise for rank_hi
 *   lo_t     = raw_lo_t if frame t has no predecessor (t == 0 and !*state_valid), if cut[t] != 0, or if s is not finite, else
 *              s = lo_{t-1} + beta * (raw_lo_t - lo_{t-1}); lo_{-1} = *state_lo.  hi_t likewise.  cut_or_null: [n] int32 or NULL
 *   y        = g where g is NaN; else g < lo_t ? lo_t : g, and then hi_t where that exceeds hi_t (a NaN bound clamps nothing)
 *   normalize != 0:  y = hi_t == lo_t ? 0 : (y - lo_t) / (hi_t - lo_t), one subtraction, one IEEE division
 * out [n][h][w] float32 = y; lo_out, hi_out, raw_lo_out, raw_hi_out [n] float32.  The state -- state_lo, state_hi, one float32
 * each, and state_valid, one int32, all in DEVICE memory -- is read and then overwritten with the last frame's lo, hi and with 1,
 * so a clip fed in sub-batches gives bit for bit what one call gives; the caller zeroes *state_valid to start a clip.
 * The selection is exact (a radix selection over the key: integer counts, the same in any order).  CS_EINVAL: a null pointer
 * (cut_or_null excepted), a non-positive size, ranks outside 0 <= rank_lo <= rank_hi < h * w, beta not in [0, 1] (NaN included),
 * a buffer off the 4-byte grid, or any two of depth, out, the three state words, the four bound arrays, cut and workspace
 * overlapping.  CS_ELIMIT: n > 65535 or h * w >= 2^31.  CS_EWORKSPACE: workspace_bytes < cs_depth_range_workspace_bytes(n, h, w, c)
 * (0 for non-positive sizes).  Every refusal precedes the first launch; the seven launches (one a memset of the workspace) go to
 * `stream`, nothing waits for the device or is read back, and the call can be captured into a graph.
 */
CS_API size_t cs_depth_range_workspace_bytes(int n, int h, int w, int c);
CS_API int cs_depth_range(const float *depth, int n, int h, int w, int c, int rank_lo, int rank_hi, double beta, int normalize,
                          const int32_t *cut_or_null, float *state_lo, float *state_hi, int32_t *state_valid, float *out,
                          float *lo_out, float *hi_out, float *raw_lo_out, float *raw_hi_out, void *workspace,
                          size_t workspace_bytes, void *stream);

/*
 * Image-guided depth upsampling (not in the reference, which stretches a smaller depth map bilinearly, so every silhouette
 * becomes a ramp that the warp smears into a halo): joint bilateral upsampling (Kopf, Cohen, Lischinski, Uyttendaele, SIGGRAPH
 * 2007), run in front of cs_generate.  Each full-resolution pixel is a weighted mean of the K x K nearest low-resolution depth
 * samples, K = 2 * radius + 1; a sample counts as far as the frame's colour at its position resembles the colour at the pixel.
 * DESIGN.md section 5 has the specification, tools/guided_oracle.py states it in numpy.
 *   image [n][h][w][3] float32, the guide; depth [n][dh][dw][c] float32, dh <= h, dw <= w; g = the gray value cs_params.depth_c
 *   describes (c == 3: gray, c == 1: the value, else channel 0); out [n][h][w] float32
 * The plan depends on h, w, dh, dw, radius, sigma_s (in low-resolution pixels) and sigma_r only: cs_guided_depth_plan writes it
 * once into cs_guided_depth_plan_bytes(...) bytes of device memory (0 for a non-positive size or a radius outside 1..3), and every
 * cs_guided_depth_apply of that geometry reads it.  float64, every operation rounded once, integers in 64 bits:
 *   u        = ((2x + 1) dw - w) / (2w)   one division;   cx[x] = floor(u + 0.5)
 *   wx[x][j] = float32(exp(-(t t) / ((2 sigma_s) sigma_s))),  t = (cx[x] + j - radius) - u,  j = 0..K-1;   cy, wy likewise from h, dh
 *   wr[d]    = float32(exp(-(a a) / ((2 sigma_r) sigma_r))),  a = d / 255.0,  d = 0..765;   sigma_r = +inf gives wr = 1
 *   gx[qx]   = min(w - 1, ((2 qx + 1) w) / (2 dw)) in integers, gy likewise: the guide pixel under a low-resolution sample's centre
 * The pass, float32, every operation rounded once.  code(v) = uint8(trunc(min(max(v, 0), 1) * 255 + 0.5)), NaN -> 0, per
 * channel.  For pixel (y, x), p = code(image[y][x]), i = 0..K-1 outer, j = 0..K-1 inner:
 *   qy = clamp(cy[y] + i - radius, 0, dh - 1);  qx = clamp(cx[x] + j - radius, 0, dw - 1);  ws = wy[y][i] * wx[x][j]
 *   d  = |p.r - q.r| + |p.g - q.g| + |p.b - q.b|,  q = code(image[gy[qy]][gx[qx]]);  wg = ws * wr[d];  v = g[qy][qx]
 *   num += wg * v;  den += wg;  ns += ws * v;  ds += ws;        out = den > 0 ? num / den : ns / ds   (IEEE division)
 * The spatial weight uses the unclamped tap position and the index is clamped (border samples are replicated); the fallback,
 * reached where every weight has rounded to zero, is the spatial mean; non-finite depth follows the arithmetic.
 * CS_EINVAL: a null pointer, a non-positive size, a radius outside 1..3, a sigma that is not positive (NaN included), a buffer
 * off the 4-byte grid, or any two of image, depth, plan and out overlapping.  CS_ELIMIT: dh > h, dw > w, n > 65535 or
 * h * w >= 2^31.  CS_EWORKSPACE: plan_bytes < cs_guided_depth_plan_bytes(h, w, dh, dw, radius).  Every refusal precedes the first
 * launch; each call is one launch on `stream`, nothing waits for the device, and a call can be captured into a graph.  A plan
 * handed to an apply of another geometry gives wrong values, never an access outside the buffers.
 */
CS_API size_t cs_guided_depth_plan_bytes(int h, int w, int dh, int dw, int radius);
CS_API int cs_guided_depth_plan(int h, int w, int dh, int dw, int radius, double sigma_s, double sigma_r, void *plan,
                                size_t plan_bytes, void *stream);
CS_API int cs_guided_depth_apply(const float *image, const float *depth, int n, int h, int w, int dh, int dw, int c, int radius,
                                 const void *plan, size_t plan_bytes, float *out, void *stream);

/*
 * Foreground depth edge dilation (not in the reference): a frame's silhouettes are anti-aliased, so a depth edge that sits on
 * the colour edge gives the outer, mixed pixels of an object the background's depth, and the warp leaves them behind as an outline
 * beside every disocclusion.  The pass grows the near surface outward by `radius` pixels, at depth discontinuities only; it runs
 * last in front of cs_generate, at the frame's resolution (behind cs_guided_depth_apply).  DESIGN.md section 5 has the
 * specification, tools/dilate_oracle.py states it in numpy.
 *   depth [n][h][w][c] float32; g = the gray value cs_params.depth_c describes (c == 3: gray, c == 1: the value, else channel 0)
 *   window  CS_DILATE_SQUARE: |dx| <= radius and |dy| <= radius;  CS_DILATE_DISC: dx dx + dy dy <= radius radius, in integers
 *           (radius 1: the 4-neighbour cross; radius 8: 197 taps).  Clipped to the frame: pixels outside take no part.
 *   key(x)  = bits(x) ^ 0x80000000 if the sign bit is clear, else ~bits(x) (uint32: a total order, -0 below +0)
 *   M(p)    = the non-NaN g(q) of largest key over p's window (CS_DILATE_NEAR_BRIGHT), of smallest key (CS_DILATE_NEAR_DARK)
 *   y(p)    = M(p) if M(p) - g(p) >= threshold (dark: g(p) - M(p) >= threshold): one float32 subtraction, one comparison, which is
 *             false for a NaN difference (a NaN centre, no candidate, inf - inf);  else g(p), bit for bit
 * out [n][h][w] float32 = y.  threshold 0 is plain grayscale dilation (dark: erosion); a positive threshold leaves smooth slopes
 * bit for bit and moves only discontinuities; dark(g) == -bright(-g) bit for bit.
 * CS_EINVAL: a null pointer, a non-positive size, a radius outside 1..8, an unknown shape or near, a threshold that is negative or
 * NaN (+inf allowed), a buffer off the 4-byte grid, or out overlapping depth (the halo reads neighbours).  CS_ELIMIT: n > 65535
 * or h * w >= 2^31.  Every refusal precedes the launch; the call is one launch on `stream`, without workspace or atomics, nothing
 * waits for the device, and the call can be captured into a graph.
 */
enum cs_dilate_shape { CS_DILATE_SQUARE = 0, CS_DILATE_DISC = 1 };
enum cs_dilate_near { CS_DILATE_NEAR_BRIGHT = 0, CS_DILATE_NEAR_DARK = 1 };
CS_API int cs_depth_dilate(const float *depth, int n, int h, int w, int c, int radius, int shape, int near, float threshold,
                           float *out, void *stream);

/*
 * Measurement hook for bench.py: while enabled, cs_generate brackets the launch of its dominant
 * kernel (the row warp + fill kernel of the selected technique) with HIP events on the caller's
 * stream.  cs_profile_read waits for the recorded events, returns the summed kernel time in
 * milliseconds and the number of launches, and clears the record.
 */
CS_API int cs_profile(int enable);
CS_API int cs_profile_read(double *total_ms, int *launches);
/* cs_profile_tiles (blocking): the share of 64 x 32 depth tiles the last profiled cs_generate call blurred (the warp kernel reads
 * the others from the gray depth, shared by both eyes); -1 when that call's warp kernel read complete blurred maps. */
CS_API int cs_profile_tiles(double *fraction);

/*
 * Development switches for the parity tests and profiling tools (compare two code paths of the same kernel,
 * count pixels per evaluation path).  Explicit, process-wide, opt-in state like cs_profile; the library never reads
 * the environment.  Release builds reject CS_DEBUG_DBG values that would leave outputs unwritten (phase cut-offs
 * exist in -DCS_DEV builds only).  No reference counterpart.
 */
enum cs_debug_key {
    CS_DEBUG_DBG = 0,               /* 14: count pixels per evaluation path into spare stats words; 17: no exponent shortcuts */
    CS_DEBUG_NO_TILE = 1,           /* polylines: general row kernel for every row instead of the tiled path */
    CS_DEBUG_PT_VARIANT = 2,        /* reference paths of the polylines and gpu_warp kernels: the PTV_* values of cs_common.h */
    CS_DEBUG_BLUR_TWO_PASS = 3,     /* depth blur: two-pass row kernels */
    CS_DEBUG_BLUR_EDGES_SCALAR = 4, /* depth blur: one-column-per-lane edge kernel */
    CS_DEBUG_BLUR_FULL_COPY = 5,    /* depth blur: write the edge-free tiles as well (no lazy tile map for the warp kernel) */
    CS_DEBUG_CHUNKS = 6,            /* cs_generate: k > 1 = k frame chunks, pre-passes on an auxiliary stream (+100: at default priority); default one chunk */
    CS_DEBUG_NO_REPLAY_KERNEL = 7,  /* polylines: order-dependent stretches replayed inside the row kernel (round-2 schedule) */
    CS_DEBUG_BLUR_NO_PRE_EDGES = 8, /* depth blur: k_gray + k_blur_edges4 instead of the one-pass k_gray_edges */
    CS_DEBUG_HYBRID_UNFUSED = 9,    /* hybrid_edge: splat result -> node outputs in a streaming pass of its own (k_hybrid_out4) */
    CS_DEBUG_GPUWARP_FULL_MAPS = 10, /* gpu_warp with the depth blur: complete blurred maps (k_blur_copy_tiles) instead of the tile map */
    CS_DEBUG_HYBRID_FULL_MAPS = 11, /* hybrid_edge with the depth blur: complete blurred maps instead of the tile map */
    CS_DEBUG_ATTN_WAVES = 12,       /* cs_stereo_attention, cs_stereo_attention_half, cs_attention_fwd_lse, cs_attention_bwd, cs_attention_half_fwd_lse, cs_attention_half_bwd: 1, 2 or 4 waves per workgroup instead of the launcher's choice (tile-size sweeps) */
    CS_DEBUG_KEYS = 13
};
CS_API int cs_debug_set(int key, int value);

/* Device self-tests of the libm-exact scalar routines (used by the parity tests):
 * out[i] = powf(x[i], y) / out[i] = exp(x[i]) evaluated by the same device code the kernels use. */
CS_API int cs_test_powf(const float *x, float y, float *out, size_t count, void *stream);
CS_API int cs_test_exp(const double *x, double *out, size_t count, void *stream);
/* Host only (no GPU): the comparison value k_gray_edges uses for the depth blur's edge test -- the largest float t with
 * fl(t / den) <= 0.5, so that clamp(|g| / den, 0, 1) > 0.5 (reference stereoimage_generation.py:1213-1222) <=> |g| > t;
 * negative when den is not positive and finite (the kernels then keep the division). */
CS_API float cs_test_edge_threshold(float den);
/* Host only (no GPU, no launch): the kernels the depth blur would run for a call of these parameters and this shape, as the
 * library's own plan decides it (the development switches in force included).
 * flags: bit 0 the caller keeps a tile map (cs_generate unless CS_DEBUG_BLUR_FULL_COPY), 1 node path (cs_generate; clear:
 * cs_directional_blur), 2 RGB depth at the frames' size, 3 the depth map is 16-byte aligned.
 * Returns CS_EINVAL when the strength rounds to a box of 0 columns or a size is not positive, else the bits
 *   1 fused kernel (clear: the two-pass kernels)      2 edge-free tiles copied, the others on a worklist (clear: every tile)
 *   4 lazy: classification + tile map                  8 edge bit rows made by the gray conversion
 *  16 the worklist runs the one-item-per-lane loader  32 refused with CS_ELIMIT (two-pass and its LDS does not fit)
 *  bits 8..10: the falloff's evaluation, 0: x, 1: sqrt, 2: x*x, 3: x*x*x, 4: powf, 5: ones */
CS_API int cs_test_blur_plan(double blur_strength, double blur_mask_width, int vert_smooth_px, double falloff_exponent, int n, int h,
                             int w, int flags);

#ifdef __cplusplus
}
#endif
#endif
