// cs_inpaintprep.hip -- the front half of StereoDiffusion's Fast mode (reference stereodiffusion_nodes.py:425-571,
// _generate_stereo_fast_single before and after the inpainting model): the backward grid-sample warp of the image, the inpaint
// mask (source x outside [-1, 1], or a disocclusion of the warped depth, dilated) and the per-row pre-fill of the masked pixels
// between their nearest unmasked neighbours, plus the uint8 codes the reference hands on.  Every frame is on its own.
//
// Two kernels, one workgroup per image row each:
//   k_ip_bits  the raw "source x outside" and "disocclusion" tests of a row as bit rows in the workspace (the dilations reach
//              two rows up and down, so the row kernel cannot have them from its own row alone)
//   k_ip_row   ORs the bit rows of rows y - 2 .. y + 2 shifted by up to two columns (the reference's two 3 x 3 max-pools), keeps
//              the mask of the row as a bit row in LDS with, per 32-column word, the last unmasked column at or before it and
//              the first at or after it (a wave prefix maximum each way), then per pixel: the warped colour, and for a masked
//              pixel left * (1 - t) + right * t of the warped colours at its two borders -- re-sampled from the image rather
//              than read back, so `warped` is written once and never read.
// No column loop carries a value from pixel to pixel.  The depth chain is this path's own (d - 0.5, no exponent; divided by 255
// per FRAME); grid_sample is cs_gridsample.h's.  Every step is one float32 operation in torch's order (-ffp-contract=off).
#include "cs_common.h"
#include "cs_kernels.h"
#include "cs_gridsample.h"

namespace cs {

// the row kernel's static LDS holds 5 words per 32 columns; torch_linspace_m11 is pinned against CPU torch up to this width
enum { IP_MAX_W = 16384, IP_MAX_WORDS = IP_MAX_W / 32 };

struct IpArgs {
    const float* image;     // [n][3][h][w]
    const float* depth;     // [n][h][w]
    const uint32_t* stats;  // [n][ST_WORDS]: ST_L_MIN / ST_L_MAX = the frame's raw depth min / max
    int n, h, w, nwords;
    float ndiv32;           // (float)(-divergence_px)
    float whalf;            // W / 2
    float thr;
    float step_w, step_h;   // torch.linspace(-1, 1, w / h) steps
    uint32_t* nvb;          // [n][h][nwords] source x outside [-1, 1]
    uint32_t* disb;         // [n][h][nwords] warped depth more than thr above the depth
    float* warped;          // [n][3][h][w] or null
    float* filled;          // [n][3][h][w] or null
    uint8_t* mask;          // [n][h][w] or null
    uint8_t* warped_u8;     // [n][h][w][3] or null
    uint8_t* filled_u8;     // [n][h][w][3] or null
};

// the frame's normalisation (:432-440): divided by 255 when ITS maximum is above 1 (min(d / 255) == min(d) / 255: the division
// is monotone), then (d - min) / (max - min) when the range is above 1e-6, else zeros
struct IpFrame { float dmin, range; bool div255, has_range; };
__device__ __forceinline__ IpFrame ip_frame(const uint32_t* stats, int f) {
    float dmin = csm::ord2f(stats[f * ST_WORDS + ST_L_MIN]), dmax = csm::ord2f(stats[f * ST_WORDS + ST_L_MAX]);
    IpFrame F;
    F.div255 = dmax > 1.0f;
    if (F.div255) { dmin = dmin / 255.0f; dmax = dmax / 255.0f; }
    F.dmin = dmin;
    F.range = dmax - dmin;
    F.has_range = F.range > (float)1e-6;
    return F;
}
// d - 0.5 of a raw depth value
__device__ __forceinline__ float ip_depth(const IpFrame& F, float v) {
    if (F.div255) v = v / 255.0f;
    const float nd = F.has_range ? (v - F.dmin) / F.range : 0.0f;
    return nd - 0.5f;
}
// grid x of column x (:442-448): linspace(-1, 1, W) - (d * -divergence_px) / (W / 2)
__device__ __forceinline__ float ip_grid_x(const IpArgs& A, int x, float dm) {
    const float lin = A.w == 1 ? -1.0f : torch_linspace_m11(x, A.w, A.step_w);
    return lin - (dm * A.ndiv32) / A.whalf;
}

__global__ void __launch_bounds__(256) k_ip_bits(IpArgs A) {
    const int y = blockIdx.x, f = blockIdx.y, w = A.w, h = A.h, tid = threadIdx.x, nt = blockDim.x;
    const IpFrame F = ip_frame(A.stats, f);
    const float* dframe = A.depth + (size_t)f * h * w;
    const float* drow = dframe + (size_t)y * w;
    const float gy = h == 1 ? -1.0f : torch_linspace_m11(y, h, A.step_h);
    const float* srow = dframe + (size_t)(int)rintf(gs_coord(gy, h, CS_GRID_PAD_BORDER)) * w;   // nearest: half to even
    const size_t brow = ((size_t)f * h + y) * A.nwords;
    for (int xb = 0; xb < w; xb += nt) {
        const int x = xb + tid;
        bool nv = false, dis = false;
        if (x < w) {
            const float dm = ip_depth(F, drow[x]);
            const float g = ip_grid_x(A, x, dm);
            nv = !(g >= -1.0f && g <= 1.0f);
            // d + 0.5 is the ROUNDED (d - 0.5) + 0.5 on both sides (:459-466)
            const int xs = (int)rintf(gs_coord(g, w, CS_GRID_PAD_BORDER));
            const float wd = ip_depth(F, srow[xs]) + 0.5f;
            dis = wd - (dm + 0.5f) > A.thr;
        }
        const unsigned long long nb = __ballot(nv), db = __ballot(dis);
        if (lane_id() == 0 && x < w) {
            A.nvb[brow + (x >> 5)] = (uint32_t)nb;
            A.disb[brow + (x >> 5)] = (uint32_t)db;
            if (x + 32 < w) {
                A.nvb[brow + (x >> 5) + 1] = (uint32_t)(nb >> 32);
                A.disb[brow + (x >> 5) + 1] = (uint32_t)(db >> 32);
            }
        }
    }
}

// "right border" of column x: the lowest valid column above x (w: none), from the row's bits and word minima
__device__ __forceinline__ int right_valid(const uint32_t* gapb, const int* next, int x, int w) {
    const int wi = x >> 5, b = x & 31, nwords = (w + 31) >> 5;
    const uint32_t above = valid_word(gapb, wi, w) & ~((2u << b) - 1u);
    if (above) return wi * 32 + __builtin_ctz(above);
    return wi + 1 < nwords ? next[wi + 1] : w;
}

// next[wi] = the lowest valid column in words wi .. nwords - 1 (w: none): the prefix maximum of the negated columns, words taken
// from the end.  Called by every thread of the block (contains a barrier); gapb must be complete.
__device__ void word_suffix_first(const uint32_t* gapb, int* next, int w) {
    const int nwords = (w + 31) >> 5, tid = threadIdx.x;
    if (tid < 64) {
        int carry = -w;
        for (int base = 0; base < nwords; base += 64) {
            const int wi = nwords - 1 - (base + tid);
            int v = -w;
            if (wi >= 0) {
                const uint32_t m = valid_word(gapb, wi, w);
                v = m ? -(wi * 32 + __builtin_ctz(m)) : -w;
            }
            v = max(wave_prefix_max(v), carry);
            if (wi >= 0) next[wi] = -v;
            carry = __shfl(v, 63);
        }
    }
    __syncthreads();
}

// bits of word wi of `row` spread k columns each way (nothing beyond the row's ends: max_pool2d pads with -inf)
__device__ __forceinline__ uint32_t spread(const uint32_t* row, int wi, int nwords, int k) {
    const uint32_t c = row[wi], p = wi > 0 ? row[wi - 1] : 0u, nx = wi + 1 < nwords ? row[wi + 1] : 0u;
    uint32_t m = c;
    for (int s = 1; s <= k; s++) m |= (c << s) | (p >> (32 - s)) | (c >> s) | (nx << (32 - s));
    return m;
}

__device__ __forceinline__ uint8_t ip_code(float v) {   // trunc(v * 255) as uint8 (:546, :564); the codes of values in [0, 1]
    return (uint8_t)(int)fminf(fmaxf(v * 255.0f, 0.0f), 255.0f);
}

__global__ void __launch_bounds__(1024) k_ip_row(IpArgs A) {
    __shared__ uint32_t sv[IP_MAX_WORDS], sd[IP_MAX_WORDS], gapb[IP_MAX_WORDS];
    __shared__ int last[IP_MAX_WORDS], next[IP_MAX_WORDS], red[1];
    const int y = blockIdx.x, f = blockIdx.y, w = A.w, h = A.h, tid = threadIdx.x, nt = blockDim.x, nwords = A.nwords;

    // ---- mask = dilate3x3(~valid | dilate3x3(dis)) (:466-491): ~valid reaches one row / column, dis two
    const size_t bframe = (size_t)f * h * nwords;
    for (int wi = tid; wi < nwords; wi += nt) {
        uint32_t v = 0u, d = 0u;
        for (int r = max(y - 2, 0); r <= min(y + 2, h - 1); r++) {
            d |= A.disb[bframe + (size_t)r * nwords + wi];
            if (r >= y - 1 && r <= y + 1) v |= A.nvb[bframe + (size_t)r * nwords + wi];
        }
        sv[wi] = v;
        sd[wi] = d;
    }
    __syncthreads();
    for (int wi = tid; wi < nwords; wi += nt) {
        const int rem = w - 32 * wi;
        const uint32_t in = rem >= 32 ? 0xffffffffu : ((1u << rem) - 1u);
        gapb[wi] = (spread(sv, wi, nwords, 1) | spread(sd, wi, nwords, 2)) & in;
    }
    __syncthreads();
    const bool row_any = word_prefix_last(gapb, last, red, w) >= 0;   // has_left == has_right: the row has an unmasked pixel
    word_suffix_first(gapb, next, w);

    const size_t plane = (size_t)h * w, row = ((size_t)f * h + y) * w;
    if (A.mask)
        for (int x = tid; x < w; x += nt) A.mask[row + x] = (gapb[x >> 5] >> (x & 31)) & 1u;
    if (!A.warped && !A.filled && !A.warped_u8 && !A.filled_u8) return;

    // ---- warped (:451-454), and the masked pixels between their nearest unmasked neighbours (:493-542)
    const IpFrame F = ip_frame(A.stats, f);
    const float gy = h == 1 ? -1.0f : torch_linspace_m11(y, h, A.step_h);
    const RowTaps R = row_taps(gy, h, CS_GRID_PAD_BORDER);
    const float* drow = A.depth + row;
    const float* img = A.image + (size_t)f * 3 * plane;
    auto warped_at = [&](int x, float* c3) {
        sample_pixel_strided(img, c3, 1, 3, h, w, plane, ip_grid_x(A, x, ip_depth(F, drow[x])), R, CS_GRID_PAD_BORDER);
    };
    for (int x = tid; x < w; x += nt) {
        float wv[3], fv[3];
        warped_at(x, wv);
        if ((gapb[x >> 5] >> (x & 31)) & 1u) {
            const int left = left_valid(gapb, last, x, w), right = right_valid(gapb, next, x, w);
            float lc[3] = {0.0f, 0.0f, 0.0f}, rc[3] = {0.0f, 0.0f, 0.0f};   // a missing border colour is 0
            if (left >= 0) warped_at(left, lc);
            if (right < w) warped_at(right, rc);
            // distances count from 1; the frame edge is one step beyond the last column (left = -1, right = w)
            const float ld = (float)(x - left), rd = (float)(right - x);
            float t = ld / fmaxf(ld + rd, 1.0f);
            if (!row_any) t = 0.0f;   // (t = 1 without a left pixel in the row, then 0 without a right one: the second wins)
            for (int ch = 0; ch < 3; ch++) fv[ch] = lc[ch] * (1.0f - t) + rc[ch] * t;
        } else {
            for (int ch = 0; ch < 3; ch++) fv[ch] = wv[ch];
        }
        for (int ch = 0; ch < 3; ch++) {
            if (A.warped) A.warped[(size_t)f * 3 * plane + (size_t)ch * plane + (size_t)y * w + x] = wv[ch];
            if (A.filled) A.filled[(size_t)f * 3 * plane + (size_t)ch * plane + (size_t)y * w + x] = fv[ch];
            if (A.warped_u8) A.warped_u8[(row + x) * 3 + ch] = ip_code(wv[ch]);
            if (A.filled_u8) A.filled_u8[(row + x) * 3 + ch] = ip_code(fv[ch]);
        }
    }
}

int inpaint_prep_max_width() { return IP_MAX_W; }

size_t inpaint_prep_bits_bytes(int n, int h, int w) { return (size_t)n * h * (((size_t)w + 31) >> 5) * 4; }

hipError_t launch_inpaint_prep(const float* image, const float* depth, int n, int h, int w, double div_px, double threshold,
                               float* warped, float* filled, uint8_t* mask, uint8_t* warped_u8, uint8_t* filled_u8,
                               const uint32_t* stats, uint32_t* nvb, uint32_t* disb, hipStream_t stream) {
    IpArgs A;
    A.image = image; A.depth = depth; A.stats = stats;
    A.n = n; A.h = h; A.w = w; A.nwords = (w + 31) >> 5;
    A.ndiv32 = (float)(-div_px);
    A.whalf = (float)(w / 2.0);
    A.thr = (float)threshold;
    A.step_w = w > 1 ? 2.0f / (float)(w - 1) : 0.0f;
    A.step_h = h > 1 ? 2.0f / (float)(h - 1) : 0.0f;
    A.nvb = nvb; A.disb = disb;
    A.warped = warped; A.filled = filled; A.mask = mask; A.warped_u8 = warped_u8; A.filled_u8 = filled_u8;
    hipLaunchKernelGGL(k_ip_bits, dim3(h, n), dim3(256), 0, stream, A);
    const int threads = w <= 1024 ? 256 : (w <= 4096 ? 512 : 1024);
    hipLaunchKernelGGL(k_ip_row, dim3(h, n), dim3(threads), 0, stream, A);
    return hipGetLastError();
}

}  // namespace cs
