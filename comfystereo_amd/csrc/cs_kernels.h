// cs_kernels.h -- internal interface between cs_abi.hip and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/comfystereo_amd.h"

namespace cs {

__host__ __device__ inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }   // every block of a workspace starts on a 256-byte boundary
__host__ __device__ inline int poly_npt(int w, int sharp) { return (sharp ? 2 * w : w) + 2; }

struct EyeArgs {
    const float* depth;  // [n][h][w] depth this eye warps with (unscaled when scale_from_stats)
    float div32, sep32;  // (float)divergence_px, (float)separation_px -- signed
    double div64, sep64; // the Python floats themselves (dialect D64)
    int enabled;         // 0: eye = source image (divergence < 0.001, quirk Q10)
    int asc;             // divergence_px < 0: sweep ascending (max source column wins)
    int naive_lim;       // abs(int(divergence_px)) + 2
    int csg_cap;         // 5 * int(abs(divergence_px)) + 25 (reference's active-list capacity)
    int st_min, st_max;  // stats words holding this eye's depth min / max
    int xoff, yoff;      // slot of this eye in the output layout
};

struct RowArgs {
    int n, h, w;
    const float* image_f32;   // [n][h][w][3] 0..1   (node path)   or null
    const uint8_t* image_u8;  // [n][h][w][3]        (asd path)    or null
    const uint32_t* stats;    // [n][ST_WORDS]
    uint32_t* stats_rw;
    int scale_from_stats;     // depth rows are multiplied by 255 when stats[ST_SCALE255]
    float e32, conv32;
    double e64;               // the exponent as the Python float (dialect D64)
    int d64;                  // dialect bits (cs_params.flags bits 3 / 4): 1 = float64 disparity chain, 2 = int64 pixel sums
    EyeArgs eye[2];
    int neyes;
    // outputs
    uint8_t* out_u8;  // asd path: [n][h][w][3]
    float* stereo;    // node path: [n][out_h][out_w][3] float32 (or uint8 codes k of k/255 when stereo_is_u8)
    int stereo_is_u8;
    int no_mask;      // (tile kernels, with stereo_is_u8) no mask output: the per-eye intermediate of the anaglyph modes
    float* mask;      //            [n][out_h][out_w]
    float* depth_l;   //            [n][h][w][3]
    float* depth_r;
    int out_h, out_w;
    int anaglyph;  // 0: eyes go to their slots; 1: R from eye0, GB from eye1; 2: R from eye1, GB from eye0
    int single;    // -1, or the only eye that is written (left-only / only-right)
    // hybrid_edge scratch (HBM): splat result of every eye, written by k_hybrid_splat
    uint8_t* hyb_base;  // [n][neyes][h][w][3]
    uint8_t* hyb_mask;  // [n][neyes][h][w]
    // lazy depth blur (cs_blur.hip): tiles of 64 x 32 pixels without an edge in reach are NOT written to the blurred depth
    // maps eye[].depth; bit (tile column) of tilemap[(frame * tile_rows + tile_row) * tm_words ..] is set for the tiles that
    // are, every other pixel is lazy_gray * (x255 scale of the frame).  Null: the blurred maps are complete.
    const uint32_t* tilemap;
    const float* lazy_gray;
    int tm_words;
    // Stretch replay OUTSIDE the row kernel (round 3, cs_rowwarp.hip k_poly_replay): a polylines row whose order-dependent
    // stretches fit the replay kernel's windows dumps its sorted points (perm, coord_d) into a slot of rp_dump and appends one
    // descriptor per stretch to rp_list; rp_ctr = {-, descriptors appended, replay cursor, -, pool units used (64 bits)}.  Null: the row kernel
    // replays its stretches itself (anaglyph modes, hybrid_edge_plus, no scratch).
    uint8_t* rp_dump;
    uint32_t* rp_list;
    uint32_t* rp_ctr;
    uint32_t rp_pool16, rp_cap;   // dump pool in 16-byte units, descriptors in the list
    const uint32_t* row_list;     // or null: process only these rows (frame * h + row), *row_count of them (tiled-path fallback)
    const uint32_t* row_count;
    // tile hints of k_polypoint (round 5): word [(frame * h + row) * 2 + eye], bit t = tile t (hint_T pixels wide) of that row-eye raised
    // the hazard, bit 31 = any tile from 31 on; the lean first pass over the flagged rows confines itself to those tiles' columns
    // plus a margin (and the sources within hint_S + 2 of them).  Null: whole rows.
    const uint32_t* hint;
    int hint_T, hint_S;
    int dbg;            // development only (cs_debug_set(CS_DEBUG_DBG, n)): see dev_switch() below
};

// Development switches (cs_debug_set, include/comfystereo_amd.h).  Release builds never read the environment; the
// switches are explicit process-wide state that only tests and profiling tools set.  In a release build CS_DEBUG_DBG
// only accepts the values that leave every output intact (14: count pixels per evaluation path, 17: no exponent
// shortcuts); the phase cut-offs of the tile and blur kernels need a -DCS_DEV build.  CS_DEBUG_PT_VARIANT only accepts the
// PTV_* values of cs_common.h.
int dev_switch(int key);


// The flagged-row block: the scratch through which the tile kernels hand rows to the row kernel (cs_abi.hip run_rows), one view of it
// per call.  Every part starts on a 256-byte boundary, in the order of the members; everything before `list` -- clear_bytes -- is
// zeroed by ONE memset per call, so a part that kernels count or flag into has to be declared before it.
enum { ROW_CTR_BYTES = 256, ROW_PAIR_WORDS = 8 };   // a counter part; the words from one {count, cursor} pair to the next
struct RowBlock {
    uint8_t* flags;         // [rows] bytes: rows the first tile pass (k_polypoint / k_polytile / k_fwdtile) leaves to the row kernel
    uint32_t* first;        // {count, cursor} of the collection of `flags` -- the three pairs share one counter part
    uint32_t* retry;        // {count, cursor} of the second collection of a call without point tier: naive_interpolating's second tier or
                            // the replay retry (no technique has both)
    uint32_t* point2;       // {count, cursor} of the point kernel's second tier (a polylines call may use it AND `retry`)
    uint32_t* replay_ctr;   // RowArgs::rp_ctr, one counter part
    uint8_t* retry_flags;   // [rows] bytes: rows with a stretch the replay kernel gave up on.  The polylines row kernel finds them
                            // ROW_CTR_BYTES behind rp_ctr by itself: they directly follow the replay counters
    uint32_t* hints;        // [rows][2 eyes] words: tile hints of the first point pass (RowArgs::hint)
    uint8_t* flags2;        // [rows] bytes: rows the point kernel's second tier leaves to the row kernel
    uint32_t* hints2;       // [rows][2 eyes] words: tile hints of that tier
    uint32_t* list;         // [rows] words: the compacted rows of the latest collection (not cleared: written before it is read)
    size_t clear_bytes, bytes;
    // naive_interpolating has no replay kernel: its second tier flags rows in the bytes the polylines techniques retry through
    uint8_t* naive_flags2() const { return retry_flags; }
};
// base == nullptr: the sizes alone (every pointer null)
inline RowBlock row_block(uint8_t* base, size_t rows) {
    static_assert(3 * ROW_PAIR_WORDS * 4 <= ROW_CTR_BYTES, "the three {count, cursor} pairs share one counter part");
    static_assert(ROW_CTR_BYTES % 256 == 0, "no padding behind the replay counters: the row kernel finds the retry flags ROW_CTR_BYTES behind rp_ctr");
    size_t o = 0;
    auto take = [&](size_t bytes) { uint8_t* p = base ? base + o : nullptr; o += al256(bytes); return p; };
    RowBlock B;
    B.flags = take(rows);
    B.first = (uint32_t*)take(ROW_CTR_BYTES);
    B.retry = B.first ? B.first + ROW_PAIR_WORDS : nullptr;
    B.point2 = B.first ? B.first + 2 * ROW_PAIR_WORDS : nullptr;
    B.replay_ctr = (uint32_t*)take(ROW_CTR_BYTES);
    B.retry_flags = take(rows);   // (directly behind the replay counters: see the static_assert)
    B.hints = (uint32_t*)take(rows * 8);
    B.flags2 = take(rows);
    B.hints2 = (uint32_t*)take(rows * 8);
    B.clear_bytes = o;
    B.list = (uint32_t*)take(rows * 4);
    B.bytes = o;
    return B;
}

// cs_rowwarp.hip
hipError_t launch_collect_rows(const uint8_t* flag, int total, uint32_t* count, uint32_t* list, hipStream_t stream);
hipError_t launch_rowwarp(int fill, const RowArgs& A, int threads, hipStream_t stream, int max_groups = 0, int lean = 0);
size_t rowwarp_lds_bytes(int fill, int w, int anaglyph = 1);   // anaglyph modes stash two channels of the first eye (2 B per pixel)
// scratch of the stretch replay kernel for a call of n frames (0: the frame is too wide for its windows); poly_replay_attach
// carves it into A.rp_* and takes the replay counters of the call's flagged-row block (zeroed by the caller's memset of the block);
// launch_poly_replay runs the descriptors the row pass appended and flags the rows it gives up on in B.retry_flags
size_t poly_replay_bytes(int n, int h, int w, int sharp);
void poly_replay_attach(RowArgs& A, int sharp, void* scratch, const RowBlock& B, size_t surplus = 0);
hipError_t launch_poly_replay(int sharp, const RowArgs& A, const RowBlock& B, int halo, hipStream_t stream);

// cs_polytile.hip: tiled fast path of polylines; flags rows it cannot do for the general kernel
hipError_t launch_polytile(int sharp, const RowArgs& A, int S, uint8_t* rowflag, hipStream_t stream);
int polytile_max_halo();

// cs_fwdtile.hip: fills 'none' / 'naive' / 'inverse' as a halo-tile kernel (node path); hipErrorNotSupported: not one of its
// cases.  'naive' flags the rows it cannot finish in `rowflag` (zeroed by the caller) for the row kernel.
hipError_t launch_fwdtile(int fill, const RowArgs& A, int S, uint8_t* rowflag, hipStream_t stream, const uint32_t* tier2_list = nullptr,
                          const uint32_t* tier2_count = nullptr);
int fwdtile_max_halo();

// cs_polypoint.hip: second generation of the tiled path (polylines_soft): one lane per polyline point
hipError_t launch_polypoint(const RowArgs& A, int S, uint8_t* rowflag, hipStream_t stream, int sharp = 0, uint32_t* hint = nullptr,
                            int* tile_width = nullptr);
// (round 6) second tier: the rows of `list` / `count` the first tier flagged, with more room for pixels under reversed segments
hipError_t launch_polypoint_tier2(const RowArgs& A, int S, uint8_t* rowflag2, hipStream_t stream, int sharp, uint32_t* hint2, int tile_width,
                                  const uint32_t* list, const uint32_t* count);
int polypoint_max_halo();
bool polypoint_sweep64_ok(int w, int halo);
// anaglyph modes behind the tile kernel: the eyes as uint8 codes side by side -> the composite (rows flagged in rowflag excepted)
hipError_t launch_anaglyph_compose(const uint8_t* sbs, const uint8_t* rowflag, int n, int h, int w, int anaglyph, float* stereo,
                                   int stereo_is_u8, float* mask, hipStream_t stream);
// depth-map output (code / 255 on three channels) of an eye the tile kernels do not visit (single-eye modes)
hipError_t launch_depth_codes(const float* depth, int n, int h, int w, const uint32_t* stats, int scale_from_stats, float* out,
                              hipStream_t stream);

// cs_blur.hip: directional depth blur (`directional_motion_blur_gpu`).  The reference's five parameters, as its callers pass them:
struct BlurParams { double strength, edge_threshold, mask_width, falloff; int vert; };
// the tile geometry the scratch view below shares with the kernels
#define BLUR_TW 64   // columns of a blur tile (one word of a bit row)
#define BLUR_TR 32   // rows of a blur tile
#define BLUR_ER4 4   // image rows per thread of the float4 edge kernels = rows of a block summary
                     // (8: 0.66 ms, 16: 0.85, 2: 0.71 -- the halo rows come from L2; fewer registers, more waves)
// The blur's two weight scratch buffers wl / wr -- al256(n * h * w * 4) bytes each, float32 weights on the two-pass path -- as the
// fused path uses them.  Each starts with its edge bit rows: `planes` planes (2: the x1 / x255 hypotheses of k_gray_edges) of
// [n * h][MW] 64-bit words, `plane_words` words apart.  Behind them in wl: the worklist's counter part, the worklist (one word per
// tile) and, on a 16-byte boundary, the tiles' output extremes; in wr: the 4-row block summaries.  base pointers null: the
// geometry and the extents alone.
enum { BLUR_CTR_BYTES = 256 };
struct BlurScratch {
    float *wl, *wr;                        // the buffers themselves (the two-pass path: [n][h][w] float32 weights)
    unsigned long long *bits_l, *bits_r;   // [planes][n * h][MW]
    size_t plane_words;
    uint32_t* work_count;      // wl: one counter part (k_blur_copy / k_blur_classify count the listed tiles in its first word)
    uint32_t* worklist;        // wl: [tiles] words
    float4* tile_stats;        // wl: [tiles][4] {l min, l max, r min, r max} of the tiles k_blur_fused wrote (k_blur_tile_stats)
    float4* block_summaries;   // wr: [n][HB][MW] {min, max, any edge bit per plane} (lazy mode: k_blur_classify)
    int MW, HB, gx, gy;        // words per bit row, summary blocks per column, tiles per row and per column
    size_t tiles;              // n * gy * gx
    // what each form needs of a buffer: the bit rows to their last word; with the worklist and the extremes (wl); with the
    // summaries (wr).  buf_bytes: what wl and wr each hold.  fits_*: the form's parts lie inside the buffers (the bit rows alone
    // outgrow theirs for w == 1: 8 bytes of bits against 4 bytes of buffer per row) and, listed, a worklist entry holds the tile:
    // 12 bits of frame, 10 + 10 of tile row and column.  listed and lazy compare with the unpadded size, as they always have.
    size_t bits_bytes, listed_bytes, lazy_bytes, buf_bytes;
    bool fits_fused, fits_listed, fits_lazy;
};
inline BlurScratch blur_scratch(float* wl, float* wr, int n, int h, int w, int planes) {
    BlurScratch S;
    S.MW = (w + 63) / 64; S.HB = (h + BLUR_ER4 - 1) / BLUR_ER4;
    S.gx = (w + BLUR_TW - 1) / BLUR_TW; S.gy = (h + BLUR_TR - 1) / BLUR_TR;
    S.tiles = (size_t)n * S.gy * S.gx;
    const size_t row_words = (size_t)n * h * S.MW, plane_bytes = al256(row_words * 8), bits = plane_bytes * planes;
    const size_t stats_off = bits + BLUR_CTR_BYTES + align16(S.tiles * 4);
    auto at = [](float* base, size_t off) { return base ? reinterpret_cast<char*>(base) + off : nullptr; };
    S.wl = wl; S.wr = wr;
    S.plane_words = plane_bytes / 8;
    S.bits_l = (unsigned long long*)at(wl, 0); S.bits_r = (unsigned long long*)at(wr, 0);
    S.work_count = (uint32_t*)at(wl, bits);
    S.worklist = (uint32_t*)at(wl, bits + BLUR_CTR_BYTES);
    S.tile_stats = (float4*)at(wl, stats_off);
    S.block_summaries = (float4*)at(wr, bits);
    S.bits_bytes = bits - plane_bytes + row_words * 8;
    S.listed_bytes = stats_off + S.tiles * 64;
    S.lazy_bytes = bits + (size_t)n * S.HB * S.MW * 16;
    S.buf_bytes = al256((size_t)n * h * w * 4);
    const size_t room = (size_t)n * h * w * 4;
    S.fits_fused = S.bits_bytes <= S.buf_bytes;
    S.fits_listed = S.fits_fused && S.gx < 1024 && S.gy < 1024 && n < 4096 && S.listed_bytes <= room;
    S.fits_lazy = S.fits_listed && S.lazy_bytes <= room;
    return S;
}
// One call's choice of path -- fused: k_blur_fused, else the two-pass kernels, which need no bit rows; listed: edge-free tiles
// are copied, the others reach k_blur_fused through the worklist; lazy: the tiles are classified from the block summaries into
// the tile map; pre_edges: the gray conversion of an RGB depth map builds the two-plane bit rows and the summaries
// (launch_gray_edges) -- and the view of wl / wr that goes with it.  generate_chunk makes ONE plan and hands it to both launches.
struct BlurPlan {
    BlurParams prm;
    int n, h, w;
    int bs, radius, vert;   // the reference's integers: box width, mask radius, rows of vertical smoothing each way
    float edge_thr;         // blur_edge_threshold_host(10 * edge_threshold)
    bool node_path;   // the input is multiplied by 255 for frames whose stats say so; the outputs' per-frame min / max go into stats
    bool fused, listed, lazy, pre_edges;
    BlurScratch S;
};
// tilemap: the caller has a tile map (blur_tilemap_bytes) for launch_blur; rgb_depth: it would convert the gray depth with
// launch_gray_edges if the plan says pre_edges
BlurPlan blur_plan(const BlurParams& prm, int n, int h, int w, float* wl, float* wr, bool tilemap, bool node_path, bool rgb_depth);
// One pass over an RGB depth map instead of k_gray + k_blur_edges4: gray depth, its per-frame min / max and the edge bit rows
// for both x255 hypotheses (cs_blur.hip k_gray_edges); P.pre_edges only
hipError_t launch_gray_edges(const BlurPlan& P, const float* rgb, float* gray, uint32_t* stats, hipStream_t stream);
float blur_edge_threshold_host(float den);   // the largest t with fl(t / den) <= 0.5, or < 0 (host arithmetic; no GPU)
// tilemap (P.lazy; zeroed here): names the tiles with an edge in reach.  lazy_used != nullptr: edge-free tiles are left UNWRITTEN
// (RowArgs::tilemap; *lazy_used = 0 when the plan took a path that writes everything); lazy_used == nullptr: a streaming copy
// completes the maps.
int launch_blur(const BlurPlan& P, const float* depth, float* out_l, float* out_r, uint32_t* stats, hipStream_t stream,
                uint32_t* tilemap = nullptr, int* lazy_used = nullptr);
// blur_plan's and launch_blur's decisions for a call as bits (cs_test_blur_plan, include/comfystereo_amd.h); no launch, no GPU
int blur_plan_describe(const BlurParams& prm, int n, int h, int w, int flags);
int blur_tilemap_words(int w);                 // 32-bit words per tile row, including the pad word the readers rely on
size_t blur_tilemap_bytes(int n, int h, int w);
// the rows of `list` (frame * h + row, *count of them; null: all `total` rows) complete in out_l / out_r: gray * scale for
// the unwritten tiles
hipError_t launch_lazy_rows(const uint32_t* list, const uint32_t* count, int total, const float* gray, float* out_l, float* out_r,
                            const uint32_t* tilemap, const uint32_t* stats, int h, int w, hipStream_t stream);

// cs_rowwarp.hip (hybrid_edge: k_hybrid_splat + the fill pass of k_rowwarp)
size_t hybrid_workspace_bytes(int n, int h, int w);
bool hybrid_fused_ok(int n, int w, int halo, int anaglyph, int single, int d64, int plus);
int hybrid_max_width();
int launch_hybrid(const RowArgs& A, void* workspace, hipStream_t stream, int plus = 0, int halo = -1);  // plus: hybrid_edge_plus; halo >= 0: bound of |offset| (tile splat)

// cs_scipyblur.hip: directional_motion_blur (the scipy depth blur of the numpy / PIL input path, reference :1346-1419)
size_t scipyblur_workspace_bytes(int n, int h, int w);
int launch_scipyblur(const float* depth, int n, int h, int w, double strength, double edge_threshold, double mask_width,
                     double falloff, int vert, float* out_l, float* out_r, void* workspace, hipStream_t stream);
// cs_gpuwarp.hip
size_t gpuwarp_workspace_bytes(int n, int h, int w, int group, int mesh);   // group: frames per reference sub-batch
int gpuwarp_max_width();
int meshwarp_max_width();
// mesh != 0: forward_warp_mesh (mesh-quality rasteriser) instead of forward_warp_gpu
int launch_gpuwarp_plain(const float* image, const float* depth, int n, int h, int w, double div_px, double sep_px,
                         double exponent, double convergence, float* warped, uint8_t* gap_mask, uint32_t* stats,
                         void* workspace, hipStream_t stream, int mesh = 0, double grad_thr = 1.5, int max_stretch = 8);
int launch_gpuwarp_node(const cs_params* p, const float* image, const float* dL, const float* dR, int scale_from_stats,
                        uint32_t* stats, float* stereo, float* depth_l, float* depth_r, float* mask, int out_h,
                        int out_w, void* workspace, hipStream_t stream, const uint32_t* tilemap = nullptr,
                        const float* gray = nullptr, int tm_words = 0);
// cs_gridwarp.hip (the grid-sample warps: cs_grid_warp, cs_interpolate_fill, cs_detect_disocclusions)
int gridwarp_max_width();   // CS_GRID_MASK / CS_GRID_STRETCH (the row in LDS)
hipError_t launch_gridwarp(const float* image, const float* depth, int n, int c, int h, int w, double div_px, double sep_px,
                           double exponent, double convergence, int op, int padding, float* out, uint8_t* mask,
                           const uint32_t* stats, float* fconst, hipStream_t stream);
hipError_t launch_interp_fill(const float* image, const uint8_t* mask, int n, int c, int h, int w, float* out, hipStream_t stream);
hipError_t launch_detect_disocc(const float* depth, const float* grid, const float* gxw, int h, int w, double threshold,
                                uint8_t* out, hipStream_t stream);
// cs_inpaintprep.hip (StereoDiffusion Fast mode's warp, inpaint mask and gap pre-fill: cs_inpaint_prepare).  nvb / disb: the
// two bit-row planes of inpaint_prep_bits_bytes(n, h, w) bytes each; stats: ST_L_MIN / ST_L_MAX = each frame's raw depth min / max
int inpaint_prep_max_width();
size_t inpaint_prep_bits_bytes(int n, int h, int w);
hipError_t launch_inpaint_prep(const float* image, const float* depth, int n, int h, int w, double div_px, double threshold,
                               float* warped, float* filled, uint8_t* mask, uint8_t* warped_u8, uint8_t* filled_u8,
                               const uint32_t* stats, uint32_t* nvb, uint32_t* disb, hipStream_t stream);
// cs_gaussblur.hip (the Gaussian depth blurs: cs_gaussian_blur).  tmp: [n][h][w] float32, the row pass's output
int gaussblur_max_taps();   // the row pass keeps a 1024-column segment plus 2 * radius halo columns in LDS
hipError_t launch_gaussblur(int op, const float* depth, const double* taps, int n_taps, double edge_threshold, int n, int h, int w,
                            float* out, float* tmp, hipStream_t stream);
// cs_pilresize.hip (Pillow's 8-bit bicubic resize with the Fast mode's code conversions: cs_pil_resize).  c_in: channels of `in`
// (gray: 3 in, 1 out); pitch: floats per row of an NHWC out_f32
int pilresize_max_taps();
int pilresize_max_size();
bool pilresize_fits(int h, int w, int oh, int ow);
size_t pilresize_workspace_bytes(int n, int h, int w, int c_out, int oh, int ow);
hipError_t launch_pilresize(const void* in, int in_f32, int gray, int n, int h, int w, int c_in, int oh, int ow, uint8_t* out_u8,
                            float* out_f32, int planar, size_t pitch, void* workspace, hipStream_t stream);
// cs_attention.hip (the reference's stereo attention, BNAttention: cs_stereo_attention).  mode: enum cs_attn_mode
int stereo_attention_max_head_dim();
int attention_waves(long long batch_heads, int n);   // waves per workgroup every attention launcher picks (32 rows each)
hipError_t launch_stereo_attention(const float* q, const float* k, const float* v, float* out, int c, int s, int b, int h, int n,
                                   int n_k, int d, float scale, int mode, hipStream_t stream);
// the SELF-mode forward that also stores every query's log-sum-exp (log2 units) to lse [(b h)][n]: cs_attention_fwd_lse
hipError_t launch_attention_fwd_lse(const float* q, const float* k, const float* v, float* out, float* lse, int b, int h, int n, int n_k,
                                    int d, float scale, hipStream_t stream);
// cs_attention_bwd.hip (dq, dk, dv of that forward: cs_attention_bwd).  workspace: attention_bwd_workspace_bytes, for any dtype
size_t attention_bwd_workspace_bytes(int b, int h, int n, int n_k, int d);
hipError_t launch_attention_bwd(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* d_out,
                                float* dq, float* dk, float* dv, int b, int h, int n, int n_k, int d, float scale, void* workspace,
                                hipStream_t stream);
// cs_attention_half.hip (the same attention on float16 / bfloat16 tensors: cs_stereo_attention_half).  dtype: enum cs_attn_dtype
hipError_t launch_stereo_attention_half(const void* q, const void* k, const void* v, void* out, int dtype, int c, int s, int b, int h,
                                        int n, int n_k, int d, float scale, int mode, hipStream_t stream);
// the SELF-mode half forward that also stores every query's log-sum-exp (float32, log2 units): cs_attention_half_fwd_lse
hipError_t launch_attention_half_fwd_lse(const void* q, const void* k, const void* v, void* out, float* lse, int dtype, int b, int h, int n,
                                         int n_k, int d, float scale, hipStream_t stream);
// cs_attention_half_bwd.hip (dq, dk, dv of that forward in the half dtype: cs_attention_half_bwd)
hipError_t launch_attention_half_bwd(const void* q, const void* k, const void* v, const void* out, const float* lse, const void* d_out,
                                     void* dq, void* dk, void* dv, int dtype, int b, int h, int n, int n_k, int d, float scale,
                                     void* workspace, hipStream_t stream);
// cs_latentshift.hip (StereoDiffusion Standard mode's latent shift, mask and merge, and the decoded images' codes:
// cs_latent_shift_plan, cs_latent_shift_apply, cs_decode_to_codes).  stats: ST_L_MIN / ST_L_MAX = the depth tensor's min / max;
// dtype: enum cs_latent_dtype; op: enum cs_latent_op
hipError_t launch_latent_shift_plan(const float* depth, int b, int h, int w, const uint32_t* stats, double scale_px, double exponent,
                                    int32_t* src_col, hipStream_t stream);
hipError_t launch_latent_shift_apply(const void* left, void* right, const int32_t* src_col, uint8_t* mask, const void* noise,
                                     int dtype, int b, int c, int h, int w, int op, hipStream_t stream);
hipError_t launch_decode_to_codes(const void* image, int dtype, int n, int c, int h, int w, uint8_t* codes, hipStream_t stream);
// cs_inversion.hip (null-text inversion outside the UNet: cs_ddim_step, cs_null_loss_grad, cs_adam_step).  dtype: enum
// cs_latent_dtype; c: the step's four coefficients c1..c4; prediction: enum cs_prediction; grad_scale: (2 / n) * (c3 - c4 * c1 / c2)
// * (1 - guidance), under CS_PRED_V (2 / n) * (c3 * c2 - c4 * c1) * (1 - guidance);
// adam: w1 = 1 - beta1, beta2, w2 = 1 - beta2, sqrt(bias correction 2), eps, -lr / bias correction 1
hipError_t launch_ddim_step(const void* sample, const void* eps_a, const void* eps_b, void* out, int dtype, size_t n, float guidance,
                            const float c[4], int prediction, hipStream_t stream);
size_t null_loss_max_count();
size_t null_loss_workspace_bytes(size_t n);
hipError_t launch_null_loss_grad(const void* eps_uncond, const void* eps_cond, const void* latent_cur, const void* latent_prev,
                                 void* rec, float* loss, void* grad, int dtype, size_t n, float guidance, const float c[4],
                                 int prediction, double grad_scale, void* workspace, hipStream_t stream);
hipError_t launch_adam_step(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int dtype, size_t n, const float adam[6],
                            hipStream_t stream);
// cs_inversion_frames.hip (the same on F frames of `per` elements each: cs_null_loss_grad_frames, cs_adam_step_frames).  active_in,
// active: one byte per frame, non-zero = the frame still optimises; active_out: what the next inner step takes as active_in
size_t null_loss_frames_max();
size_t null_loss_frames_workspace_bytes(size_t frames, size_t per);
hipError_t launch_null_loss_grad_frames(const void* eps_uncond, const void* eps_cond, const void* latent_cur, const void* latent_prev,
                                        void* rec, float* loss, void* grad, const uint8_t* active_in, uint8_t* active_out, int dtype,
                                        size_t frames, size_t per, float guidance, const float c[4], int prediction, double grad_scale,
                                        double threshold, void* workspace, hipStream_t stream);
hipError_t launch_adam_step_frames(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, const uint8_t* active, int dtype,
                                   size_t frames, size_t m, const float adam[6], hipStream_t stream);
// cs_inpaintloop.hip (StereoDiffusion Fast mode's inpainting loop outside its models: cs_inpaint_image_prep,
// cs_inpaint_latent_init, cs_inpaint_plms_step).  dtype, mean_dtype: enum cs_latent_dtype; kind: enum cs_plms_kind;
// x [2n][9][hl][wl], the UNet's persistent input
hipError_t launch_inpaint_image_prep(const uint8_t* filled, const uint8_t* mask, int n, int h, int w, int hl, int wl, int dtype, void* img,
                                     void* masked, void* x, hipStream_t stream);
hipError_t launch_inpaint_latent_init(const void* mean_img, const void* mean_masked, int mean_dtype, const void* noise, int dtype, int n,
                                      int hl, int wl, float sa, float sb, void* x, void* img_latent, void* decode_in, hipStream_t stream);
hipError_t launch_inpaint_plms_step(const void* noise_pred, void* x, int dtype, int n, int hl, int wl, int kind, float guidance, float sc,
                                    float da, float denom, void* e_out, const void* e1, const void* e2, const void* e3, void* cur_sample,
                                    void* decode_in, hipStream_t stream);
// cs_fewstep.hip (Fast mode's loop for few-step models: cs_inpaint_fewstep_init, cs_inpaint_fewstep_step).  dtype: enum
// cs_latent_dtype; sampler: enum cs_fewstep_sampler; channels: 9 or 4; halves: 2 under classifier-free guidance, 1 without;
// x [halves * n][channels][hl][wl], the UNet's persistent input; x9 [2n][9][hl][wl], what launch_inpaint_image_prep wrote
hipError_t launch_inpaint_fewstep_init(const void* img_latent, const void* noise, const void* x9, int dtype, int n, int hl, int wl,
                                       int channels, int halves, int sampler, float k0, float k1, void* x, void* state, void* mask_l,
                                       hipStream_t stream);
hipError_t launch_inpaint_fewstep_step(const void* noise_pred, void* x, int dtype, int n, int hl, int wl, int channels, int sampler, int cfg,
                                       int last, float guidance, const float k[6], void* state, const void* step_noise,
                                       const void* img_latent, const void* noise0, const void* mask_l, void* decode_in, hipStream_t stream);
// cs_standardloop.hip (StereoDiffusion Standard mode between two UNet calls: cs_standard_step).  dtype: enum cs_latent_dtype;
// op: enum cs_standard_op; cf: the step's four coefficients c1..c4; x [4b][c][h][w], the UNet's persistent input
hipError_t launch_standard_step(void* x, const void* noise_pred, int dtype, int b, int c, int h, int w, float guidance, const float cf[4],
                                int prediction, int op, const int32_t* src_col, uint8_t* mask, const void* noise, hipStream_t stream);
// cs_temporal.hip (temporal depth stabilisation: cs_temporal_depth).  partial: temporal_workspace_bytes(n, h, w) bytes, one
// float32 per frame and 16 384-pixel range; valid: the state's flag, one int32 in device memory
size_t temporal_workspace_bytes(int n, int h, int w);
hipError_t launch_temporal(const float* depth, int n, int h, int w, int c, float alpha, float motion_thr, float cut_thr,
                           float* prev_raw, float* prev, int32_t* valid, float* out, float* m, int32_t* cut, float* partial,
                           hipStream_t stream);
// cs_motiondepth.hip (motion-compensated temporal depth stabilisation: cs_motion_depth).  guide [n][h][w][3]; the state's fourth
// buffer prev_luma is [h][w] uint8; vec [n][Hb][Wb][2] (dx, dy), sad and matched [n][Hb][Wb], Hb = ceil(h / 16), Wb = ceil(w / 16);
// workspace: motion_workspace_bytes(n, h, w) bytes (cs_motiondepth.h MotionViews)
size_t motion_workspace_bytes(int n, int h, int w);
hipError_t launch_motion_depth(const float* depth, const float* guide, int n, int h, int w, int c, float alpha, float motion_thr,
                               float cut_thr, int search_range, int smoothness, int match_thr, float* prev_raw, float* prev,
                               uint8_t* prev_luma, int32_t* valid, float* out, float* m, int32_t* cut, int8_t* vec, int32_t* sad,
                               uint8_t* matched, void* workspace, hipStream_t stream);
// cs_motionpyramid.hip (the same filter with a coarse-to-fine search on a three-level luma pyramid: cs_motion_depth_pyramid).  The
// arguments of launch_motion_depth, search_range a multiple of 4 in 4..120; workspace: pyramid_workspace_bytes(n, h, w) bytes
// (cs_motionpyramid.h PyramidViews)
size_t pyramid_workspace_bytes(int n, int h, int w);
hipError_t launch_motion_depth_pyramid(const float* depth, const float* guide, int n, int h, int w, int c, float alpha, float motion_thr,
                                       float cut_thr, int search_range, int smoothness, int match_thr, float* prev_raw, float* prev,
                                       uint8_t* prev_luma, int32_t* valid, float* out, float* m, int32_t* cut, int8_t* vec, int32_t* sad,
                                       uint8_t* matched, void* workspace, hipStream_t stream);
// cs_depthrange.hip (depth range clipping: cs_depth_range).  workspace: range_workspace_bytes(n) bytes, the frames' digit
// histograms and selections; cut: null or [n] int32; the state's three words live in device memory
size_t range_workspace_bytes(int n);
hipError_t launch_depth_range(const float* depth, int n, int h, int w, int c, int rank_lo, int rank_hi, float beta, int normalize,
                              const int32_t* cut, float* state_lo, float* state_hi, int32_t* state_valid, float* out, float* lo,
                              float* hi, float* raw_lo, float* raw_hi, void* workspace, hipStream_t stream);
// cs_guideddepth.hip (image-guided depth upsampling: cs_guided_depth_plan, cs_guided_depth_apply).  plan: guided_plan_bytes(...)
// bytes of device memory, written by launch_guided_plan once per geometry and read by every launch_guided_apply of it
size_t guided_plan_bytes(int h, int w, int dh, int dw, int radius);
hipError_t launch_guided_plan(int h, int w, int dh, int dw, int radius, double sigma_s, double sigma_r, void* plan, hipStream_t stream);
hipError_t launch_guided_apply(const float* image, const float* depth, int n, int h, int w, int dh, int dw, int c, int radius,
                               const void* plan, float* out, hipStream_t stream);
// cs_depthdilate.hip (foreground depth edge dilation: cs_depth_dilate).  radius 1..8, shape and near of enum cs_dilate_shape /
// cs_dilate_near; one launch, no workspace
hipError_t launch_depth_dilate(const float* depth, int n, int h, int w, int c, int radius, int shape, int near, float threshold, float* out,
                               hipStream_t stream);
// lazy depth-blur tiles in k_gpuwarp (tilemap != nullptr): rows of at most this many columns, not the mesh-quality warp
int gpuwarp_lazy_max_width();

}  // namespace cs
