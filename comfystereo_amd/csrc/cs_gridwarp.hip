// cs_gridwarp.hip -- the reference's grid-sample warps (stereoimage_generation.py): apply_stereo_divergence_gpu (:52-119),
// warp_and_fill_gpu (:122-274), compute_forward_mask_gpu (:692-757), apply_stereo_divergence_gpu_with_fill (:923-1002),
// interpolate_fill_gpu (:860-920) and detect_disocclusions_gpu (:807-857).
//
// The first four share forward_warp_gpu's depth -> offset chain and one row kernel, k_gridwarp<OP>: one workgroup per image
// row, grid x = linspace(-1, 1, W) - offset / (W / 2), then one bilinear grid_sample.  The forward gap mask (mask only, and the
// warp with edge stretch) keeps the row in LDS: offsets and grid x (8 B per column) and three bit rows -- hits, the dilated gap,
// and per 32-column word the last valid column at or before it (a prefix maximum over words; "left border" = the highest
// valid bit below the column, or that word maximum).  "Right border" is the row's LAST valid column when it lies at or after
// the column (the reference's flipped cummax, quirk Q2 of forward_warp_gpu): one block-wide maximum.
// grid_sample is CPU torch's vectorised kernel as it runs: the four corner taps summed as fma(se, fma(sw, fma(ne, nw * v0)))
// (the compiler contracts that kernel's sum), the reflection remainder as one fused multiply-add.  Every other step is one
// float32 operation in torch's order (-ffp-contract=off).
#include "cs_common.h"
#include "cs_kernels.h"
#include "cs_warpmath.h"
#include "cs_gridsample.h"

namespace cs {

__constant__ csm::PowfTables c_gr_powf_tables = CS_POWF_TABLES_INIT;

enum { GRC_DMIN = 0, GRC_CRANGE = 1, GRC_FLAGS = 2, GRC_WORDS = 4 };   // per-frame constants (k_grid_consts)

struct GrArgs {
    const float* image;    // [n][c][h][w]
    const float* depth;    // [n][h][w]
    const float* fconst;   // [n][GRC_WORDS]
    int n, c, h, w;
    int pow_mode, padding;
    float e32, conv32, div32, sep32;
    float step_w, step_h;  // torch.linspace(-1, 1, w / h) steps (IEEE division on the host; 0 for a size of 1)
    float whalf;           // W / 2
    float* out;            // [n][c][h][w] or null
    uint8_t* mask;         // [n][h][w] or null: gap mask (CS_GRID_MASK, CS_GRID_STRETCH), valid mask (CS_GRID_FILL)
};

// per frame: min, clamped range and flags (bit 0: range above 1e-6) of the depth the chain normalises -- divided by 255 when
// ANY frame's maximum is above 1 (min(d / 255) == min(d) / 255: the division is monotone)
__global__ void k_grid_consts(const uint32_t* stats, int n, float* fconst) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    bool div255 = false;
    for (int k = 0; k < n; k++) div255 = div255 || csm::ord2f(stats[k * ST_WORDS + ST_L_MAX]) > 1.0f;
    float dmin = csm::ord2f(stats[f * ST_WORDS + ST_L_MIN]), dmax = csm::ord2f(stats[f * ST_WORDS + ST_L_MAX]);
    if (div255) { dmin = dmin / 255.0f; dmax = dmax / 255.0f; }
    const float range = dmax - dmin;
    float* C = fconst + (size_t)f * GRC_WORDS;
    C[GRC_DMIN] = dmin;
    C[GRC_CRANGE] = fmaxf(range, (float)1e-6);
    C[GRC_FLAGS] = __builtin_bit_cast(float, (range > (float)1e-6 ? 1u : 0u) | (div255 ? 2u : 0u));
    C[3] = 0.0f;
}

// LDS of the gap-mask row kernels: [powf tables][po: w floats][gx: w floats][hit | gap | last: 3 x nwords words][red: 32]
__host__ __device__ inline size_t gr_tables_bytes() { return align16(sizeof(csm::PowfTables)); }
__host__ __device__ inline size_t gr_lds_bytes(int w, bool gap) {
    if (!gap) return gr_tables_bytes();
    const size_t nwords = ((size_t)w + 31) >> 5;
    return gr_tables_bytes() + 8 * (size_t)w + 12 * nwords + 32 * 4;
}

template <int OP>
__global__ void __launch_bounds__(1024) k_gridwarp(GrArgs A) {
    constexpr bool GAP = OP == CS_GRID_MASK || OP == CS_GRID_STRETCH;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int y = blockIdx.x, f = blockIdx.y, w = A.w, h = A.h, tid = threadIdx.x, nt = blockDim.x;
    const int nwords = (w + 31) >> 5;
    csm::PowfTables* T = (csm::PowfTables*)smem;
    float* po = (float*)(smem + gr_tables_bytes());
    float* gxs = po + w;
    uint32_t* hit = (uint32_t*)(gxs + w);
    uint32_t* gapb = hit + nwords;
    int* last = (int*)(gapb + nwords);
    int* red = last + nwords;
    if (A.pow_mode == 4) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&c_gr_powf_tables);
        for (int i = tid; i < (int)(sizeof(csm::PowfTables) / 4); i += nt) reinterpret_cast<uint32_t*>(T)[i] = src[i];
    }
    if (GAP)
        for (int i = tid; i < nwords; i += nt) hit[i] = 0u;
    const float* fc = A.fconst + (size_t)f * GRC_WORDS;
    const float dmin = fc[GRC_DMIN], crange = fc[GRC_CRANGE];
    const uint32_t fl = __builtin_bit_cast(uint32_t, fc[GRC_FLAGS]);
    const bool has_range = (fl & 1u) != 0, div255 = (fl & 2u) != 0;
    const int pad = OP == CS_GRID_FILL ? A.padding : CS_GRID_PAD_BORDER;
    const float gy = h == 1 ? -1.0f : torch_linspace_m11(y, h, A.step_h);
    const RowTaps R = row_taps(gy, h, pad);
    const size_t plane = (size_t)h * w, row = ((size_t)f * h + y) * w;
    const float* drow = A.depth + row;
    const float* img = A.image ? A.image + (size_t)f * A.c * plane : nullptr;
    float* out = A.out ? A.out + (size_t)f * A.c * plane + (size_t)y * w : nullptr;
    __syncthreads();

    // ---- depth -> offset -> grid x (forward_warp_gpu's chain :313-331; the grid of :96-106)
    auto offset_of = [&](float v) {
        if (div255) v = v / 255.0f;
        const float nrm = has_range ? (v - dmin) / crange : 0.0f;
        const float s = nrm - A.conv32;
        const float sg = s > 0.0f ? 1.0f : (s < 0.0f ? -1.0f : 0.0f);
        return (sg * torch_pow(fabsf(s), A.pow_mode, A.e32, T)) * A.div32 + A.sep32;
    };
    for (int x = tid; x < w; x += nt) {
        const float p = offset_of(drow[x]);
        const float lin = w == 1 ? -1.0f : torch_linspace_m11(x, w, A.step_w);
        const float g = lin - p / A.whalf;
        if (GAP) {
            po[x] = p;
            gxs[x] = g;
            // dest = (col + offset).long() (truncation toward zero): a hit on [0, w) exactly when -1 < col + offset < w
            const float dst = (float)x + p;
            if (dst > -1.0f && dst < (float)w) {
                const int d = (int)dst;
                atomicOr(&hit[d >> 5], 1u << (d & 31));
            }
        } else {
            if (out) sample_pixel(img, out + x, A.c, h, w, plane, g, R, pad);
            if (A.mask) A.mask[row + x] = (g >= -1.0f && g <= 1.0f) ? 1 : 0;   // valid: the source x inside [-1, 1]
        }
    }
    if (!GAP) return;
    __syncthreads();

    // ---- gap = no hit, dilated by one column where adjacent SOURCE offsets differ by more than 1.5 (:747-755)
    auto gap0 = [&](int x) { return ((hit[x >> 5] >> (x & 31)) & 1u) == 0u; };
    for (int xb = 0; xb < w; xb += nt) {
        const int x = xb + tid;
        bool dil = false;
        if (x < w) {
            const float p = po[x];
            const bool edge = (x + 1 < w && fabsf(po[x + 1] - p) > 1.5f) || (x >= 1 && fabsf(p - po[x - 1]) > 1.5f);
            dil = gap0(x) || (edge && ((x >= 1 && gap0(x - 1)) || (x + 1 < w && gap0(x + 1))));
            if (A.mask) A.mask[row + x] = dil ? 1 : 0;
        }
        const unsigned long long gb = __ballot(dil);
        if (lane_id() == 0 && x < w) {
            gapb[x >> 5] = (uint32_t)gb;
            if (x + 32 < w) gapb[(x >> 5) + 1] = (uint32_t)(gb >> 32);
        }
    }
    if (OP == CS_GRID_MASK) return;
    __syncthreads();
    const int rightmost = word_prefix_last(gapb, last, red, w);

    // ---- edge stretch of the gap pixels' grid x (:197-265), then one bilinear grid_sample with border padding
    for (int x = tid; x < w; x += nt) {
        float g = gxs[x];
        if ((gapb[x >> 5] >> (x & 31)) & 1u) {
            const int left = left_valid(gapb, last, x, w);
            const int right = rightmost >= x ? rightmost : -1;
            const float ld = (float)(x - left), rd = (float)(right - x);
            const float total = fmaxf(ld + rd, 1.0f);
            const float half = total * 0.5f;
            auto at = [&](int i) { return gxs[min(max(i, 0), w - 1)]; };
            const float lt = fminf(fmaxf(ld / half, 0.0f), 1.0f);
            const float ls = at(left) * (1.0f - lt) + at(left - 3) * lt;
            const float rt = fminf(fmaxf(rd / half, 0.0f), 1.0f);
            const float rs = at(right) * (1.0f - rt) + at(right + 3) * rt;
            float t = ld / total;
            if (left < 0) t = 1.0f;
            if (right < 0) t = 0.0f;
            float bl = fminf(fmaxf((t - 0.35f) / 0.3f, 0.0f), 1.0f);
            bl = bl * bl * (3.0f - 2.0f * bl);
            g = ls * (1.0f - bl) + rs * bl;
        }
        if (out) sample_pixel(img, out + x, A.c, h, w, plane, g, R, CS_GRID_PAD_BORDER);
    }
}

// interpolate_fill_gpu: masked pixels take left * (1 - t) + right * t of their borders (left: nearest valid column before,
// right: the row's last valid column if at or after; t = 1 without a left border, 0 without a right one)
__global__ void __launch_bounds__(1024) k_interp_fill(const float* image, const uint8_t* mask, int c, int h, int w, float* out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int y = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
    const int nwords = (w + 31) >> 5;
    uint32_t* gapb = (uint32_t*)smem;
    int* last = (int*)(gapb + nwords);
    int* red = last + nwords;
    const size_t plane = (size_t)h * w, row = ((size_t)f * h + y) * w;
    const float* img = image + (size_t)f * c * plane + (size_t)y * w;
    float* o = out + (size_t)f * c * plane + (size_t)y * w;
    for (int xb = 0; xb < w; xb += nt) {
        const int x = xb + tid;
        const bool m = x < w && mask[row + x] != 0;
        const unsigned long long gb = __ballot(m);
        if (lane_id() == 0 && x < w) {
            gapb[x >> 5] = (uint32_t)gb;
            if (x + 32 < w) gapb[(x >> 5) + 1] = (uint32_t)(gb >> 32);
        }
    }
    __syncthreads();
    const int rightmost = word_prefix_last(gapb, last, red, w);
    for (int x = tid; x < w; x += nt) {
        if (!((gapb[x >> 5] >> (x & 31)) & 1u)) {
            for (int ch = 0; ch < c; ch++) o[(size_t)ch * plane + x] = img[(size_t)ch * plane + x];
            continue;
        }
        const int left = left_valid(gapb, last, x, w);
        const int right = rightmost >= x ? rightmost : -1;
        const float ld = (float)(x - left), rd = (float)(right - x);
        float t = ld / fmaxf(ld + rd, 1.0f);
        if (left < 0) t = 1.0f;
        if (right < 0) t = 0.0f;
        const int li = min(max(left, 0), w - 1), ri = min(max(right, 0), w - 1);
        for (int ch = 0; ch < c; ch++) {
            const float* p = img + (size_t)ch * plane;
            o[(size_t)ch * plane + x] = p[li] * (1.0f - t) + p[ri] * t;
        }
    }
}

// detect_disocclusions_gpu: depth sampled at the caller's grid (nearest, border, align_corners=True; coordinates rounded half
// to even) more than `threshold` above the depth, or a horizontal step of grid_x_warped above 3 * 2 / W
__global__ void __launch_bounds__(256) k_detect_disocc(const float* depth, const float* grid, const float* gxw, int h, int w,
                                                       float thr, float step_thr, uint8_t* out) {
    const size_t total = (size_t)h * w;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % (size_t)w);
        const float xs = rintf(gs_coord(grid[2 * i], w, CS_GRID_PAD_BORDER));
        const float ys = rintf(gs_coord(grid[2 * i + 1], h, CS_GRID_PAD_BORDER));
        const float wd = depth[(size_t)(int)ys * w + (int)xs];
        const bool deep = wd - depth[i] > thr;
        const size_t j = x < w - 1 ? i : i - 1;   // (the last column copies the step before it)
        const bool stretch = fabsf(gxw[j + 1] - gxw[j]) > step_thr;
        out[i] = (deep || stretch) ? 1 : 0;
    }
}

static int gr_threads(int w) { return w <= 1024 ? 256 : (w <= 4096 ? 512 : 1024); }

int gridwarp_max_width() {
    int lo = 1, hi = 1 << 20;
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (gr_lds_bytes(mid, true) <= CS_LDS_BYTES) lo = mid; else hi = mid - 1;
    }
    return lo;
}

hipError_t launch_gridwarp(const float* image, const float* depth, int n, int c, int h, int w, double div_px, double sep_px,
                           double exponent, double convergence, int op, int padding, float* out, uint8_t* mask,
                           const uint32_t* stats, float* fconst, hipStream_t stream) {
    hipLaunchKernelGGL(k_grid_consts, dim3((n + 63) / 64), dim3(64), 0, stream, stats, n, fconst);
    GrArgs A;
    A.image = image; A.depth = depth; A.fconst = fconst;
    A.n = n; A.c = c; A.h = h; A.w = w;
    A.pow_mode = pow_mode_of(exponent); A.padding = padding;
    A.e32 = (float)exponent; A.conv32 = (float)convergence; A.div32 = (float)div_px; A.sep32 = (float)sep_px;
    A.step_w = w > 1 ? 2.0f / (float)(w - 1) : 0.0f;
    A.step_h = h > 1 ? 2.0f / (float)(h - 1) : 0.0f;
    A.whalf = (float)(w / 2.0);
    A.out = out; A.mask = mask;
    const bool gap = op == CS_GRID_MASK || op == CS_GRID_STRETCH;
    const size_t lds = gr_lds_bytes(w, gap);
    const void* fn = op == CS_GRID_WARP ? (const void*)k_gridwarp<CS_GRID_WARP> : op == CS_GRID_FILL ? (const void*)k_gridwarp<CS_GRID_FILL>
                   : op == CS_GRID_MASK ? (const void*)k_gridwarp<CS_GRID_MASK> : (const void*)k_gridwarp<CS_GRID_STRETCH>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const dim3 grid(h, n), block(gap ? gr_threads(w) : (w <= 256 ? 256 : 512));
    switch (op) {
    case CS_GRID_WARP: hipLaunchKernelGGL(k_gridwarp<CS_GRID_WARP>, grid, block, lds, stream, A); break;
    case CS_GRID_FILL: hipLaunchKernelGGL(k_gridwarp<CS_GRID_FILL>, grid, block, lds, stream, A); break;
    case CS_GRID_MASK: hipLaunchKernelGGL(k_gridwarp<CS_GRID_MASK>, grid, block, lds, stream, A); break;
    default: hipLaunchKernelGGL(k_gridwarp<CS_GRID_STRETCH>, grid, block, lds, stream, A); break;
    }
    return hipGetLastError();
}

size_t interp_fill_lds_bytes(int w) { return 8 * (((size_t)w + 31) >> 5) + 32 * 4; }

hipError_t launch_interp_fill(const float* image, const uint8_t* mask, int n, int c, int h, int w, float* out, hipStream_t stream) {
    const size_t lds = interp_fill_lds_bytes(w);
    hipError_t e = hipFuncSetAttribute((const void*)k_interp_fill, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_interp_fill, dim3(h, n), dim3(gr_threads(w)), lds, stream, image, mask, c, h, w, out);
    return hipGetLastError();
}

hipError_t launch_detect_disocc(const float* depth, const float* grid, const float* gxw, int h, int w, double threshold,
                                uint8_t* out, hipStream_t stream) {
    const size_t total = (size_t)h * w;
    const int blocks = (int)(total / 256 + 1 < 65536 ? total / 256 + 1 : 65536);
    hipLaunchKernelGGL(k_detect_disocc, dim3(blocks), dim3(256), 0, stream, depth, grid, gxw, h, w, (float)threshold,
                       (float)(2.0 / w * 3.0), out);
    return hipGetLastError();
}

}  // namespace cs
