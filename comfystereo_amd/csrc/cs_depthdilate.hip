// cs_depthdilate.hip -- foreground depth edge dilation (cs_depth_dilate; DESIGN.md section 5, "Depth edge dilation").  Not in the
// reference: a frame's silhouettes are anti-aliased, so a depth edge that sits on the colour edge gives the outer, mixed pixels of an
// object the background's depth and the warp leaves them behind as an outline.  The pass grows the near surface outward by R pixels,
// at depth discontinuities only.  tools/dilate_oracle.py states it in numpy.
//
//   g        = gray value of the frame (gray_of for C == 3, the value for C == 1, channel 0 otherwise: cs_gray4.h)
//   window   = square: |dx| <= R and |dy| <= R;  disc: dx dx + dy dy <= R R (integers);  clipped to the frame
//   key(x)   = bits(x) ^ 0x80000000 if the sign bit is clear, else ~bits(x): uint32, monotone in x, -0 below +0 (cs_depthrange.hip)
//   M(p)     = the non-NaN g(q) of largest key over p's window (near = bright), of smallest key (near = dark)
//   y(p)     = M(p) if M(p) - g(p) >= threshold (dark: g(p) - M(p) >= threshold), one float32 subtraction and one comparison, which
//              is false for a NaN difference (a NaN centre, inf - inf); else g(p)
//
//   k_depth_dilate<R, SHAPE, CM, VEC>   grid (tiles, n), one launch.  A 256-thread workgroup owns a tile of DD_TW x DD_TH = 64 x 16
//       pixels and stages the tile and a halo -- R rows above and below, HG = ceil(R / 4) groups of four columns on either side --
//       in LDS as uint32 KEYS: 0 for a NaN pixel and for one outside the frame (the smallest key of a non-NaN value is
//       key(-inf) = 0x007FFFFF, so 0 is free and is the identity of max), and for near = dark the key's complement, 0 again for "no
//       candidate".  From there the pass is integer max, the specification's order built in, for both directions.
//       Lane `tid` owns the four pixels x = X0 + 4 (tid & 15) + {0..3} of row Y0 + (tid >> 4).  It loads them itself
//       (load_gray4<CM, VEC>) and keeps their float bits in registers, so "unchanged" returns g(p) exactly, a NaN centre's bits
//       included; the halo's groups of four are dealt out over the workgroup.  One barrier.
//       A row of the window is a chord of half-width a.  chord4<A> reads the 2 ceil(A / 4) + 1 aligned groups of four keys around
//       the lane's own (ds_read_b128) and forms the four sliding maxima from one shared core (the 2A - 2 keys every one of the four
//       windows holds) and three keys on either side: 2A + 7 max operations for four pixels, not 4 (2A + 1).
//         disc    2R + 1 chords, a(dy) the largest a with a a + dy dy <= R R (a compile-time constant per row), accumulated in
//                 registers.  At R = 8: 17 rows, 69 ds_read_b128 per four pixels, against 4 x 197 single reads tap by tap.
//         square  separable: chord4<R> of every staged row into a second LDS plane, barrier, then the maximum of 2R + 1 rows of that
//                 plane (one ds_read_b128 each).
//       store4<VEC> writes the lane's four results (the guarded path with the row's end as its limit).
//       VEC needs w % 4 == 0 (every row of a frame then starts on the 16-byte grid) and depth and out on the 16-byte grid; otherwise
//       the same pixels go through guarded 4-byte accesses.  No atomics, no workspace, nothing waits for the device.
//
// Bytes per pixel: 4 C read (plus the halo's share: (16 + 2R)(64 + 8HG) / 1024 - 1, 0.27 at R = 2, 1.5 at R = 8, mostly from L2),
// 4 written.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, ROCm 7.2; no instantiation spills a vector or scalar register, none
// uses scratch).  Per R the largest figures over CM = 1, 3, 0 and both access paths:
//                                      VGPRs  SGPRs  LDS bytes  occupancy (waves / SIMD)
//   k_depth_dilate<1, square, *, *>       27     31      9792        8
//   k_depth_dilate<2, square, *, *>       34     31     10880        8
//   k_depth_dilate<3, square, *, *>       42     31     11968        8
//   k_depth_dilate<4, square, *, *>       50     31     13056        8
//   k_depth_dilate<5, square, *, *>       56     41     14976        8
//   k_depth_dilate<6, square, *, *>       62     41     16128        8
//   k_depth_dilate<7, square, *, *>       62     42     17280        8
//   k_depth_dilate<8, square, *, *>       68     42     18432        7
//   k_depth_dilate<1, disc, *, *>         26     31      5184        8
//   k_depth_dilate<2, disc, *, *>         40     31      5760        8
//   k_depth_dilate<3, disc, *, *>         58     31      6336        8
//   k_depth_dilate<4, disc, *, *>         70     31      6912        7
//   k_depth_dilate<5, disc, *, *>         84     41      8320        5
//   k_depth_dilate<6, disc, *, *>         98     41      8960        4
//   k_depth_dilate<7, disc, *, *>        112     42      9600        4
//   k_depth_dilate<8, disc, *, *>        124     42     10240        4
// The disc's largest figures are the guarded path's, where the compiler hoists more of the chords' loads; the 16-byte path of the
// disc takes at most 33 / 48 / 52 / 61 / 66 / 72 / 81 VGPRs at R = 2..8 over the three CM (5 waves per SIMD at R = 8).  LDS never
// limits the occupancy: 8 workgroups of 18 KB fit a CU's 160 KB.
#include <utility>

#include "cs_common.h"
#include "cs_gray4.h"
#include "cs_kernels.h"

namespace cs {

enum { DD_THREADS = 256, DD_TW = 64, DD_TH = 16, DD_GX = DD_TW / 4 };

__device__ __forceinline__ uint32_t dilate_key(float x) {
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ float dilate_value(uint32_t key) {
    return __builtin_bit_cast(float, (key & 0x80000000u) ? key ^ 0x80000000u : ~key);
}
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

// the half-width of the disc's chord in row dy: the largest a with a a + dy dy <= R R
template <int R, int DY>
constexpr int chord_half() {
    int a = 0;
    while ((a + 1) * (a + 1) + DY * DY <= R * R) a++;
    return a;
}

// m[k] = max(m[k], the keys p[k - A .. k + A]), k = 0..3.  p: the lane's own four keys in a staged row, on the 16-byte grid, with
// at least 4 ceil(A / 4) keys of the row on either side.
template <int A>
__device__ __forceinline__ void chord4(const uint32_t* p, uint32_t (&m)[4]) {
    constexpr int GA = (A + 3) / 4, C0 = 4 * GA;   // groups on either side; the index of the lane's first key in v
    uint32_t v[4 * (2 * GA + 1)];
#pragma unroll
    for (int g = 0; g <= 2 * GA; g++) {
        const uint4 q = *reinterpret_cast<const uint4*>(p + 4 * (g - GA));
        v[4 * g] = q.x; v[4 * g + 1] = q.y; v[4 * g + 2] = q.z; v[4 * g + 3] = q.w;
    }
    if constexpr (A == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) m[k] = umax(m[k], v[k]);
    } else {
        // the four windows are [C0 + k - A, C0 + k + A]: all hold [LO3, HI0]; 0 is the identity where that is empty (A == 1)
        constexpr int LO3 = C0 + 3 - A, HI0 = C0 + A;
        uint32_t core = 0u;
#pragma unroll
        for (int t = LO3; t <= HI0; t++) core = umax(core, v[t]);
        const uint32_t l2 = v[LO3 - 1], l1 = umax(l2, v[LO3 - 2]), l0 = umax(l1, v[LO3 - 3]);
        const uint32_t r1 = v[HI0 + 1], r2 = umax(r1, v[HI0 + 2]), r3 = umax(r2, v[HI0 + 3]);
        m[0] = umax(m[0], umax(core, l0));
        m[1] = umax(m[1], umax(core, umax(l1, r1)));
        m[2] = umax(m[2], umax(core, umax(l2, r2)));
        m[3] = umax(m[3], umax(core, r3));
    }
}

template <int R, int PITCH, int... I>
__device__ __forceinline__ void disc_chords(const uint32_t* p, uint32_t (&m)[4], std::integer_sequence<int, I...>) {
    (chord4<chord_half<R, I - R>()>(p + I * PITCH, m), ...);   // row I of the window is dy = I - R
}

template <int R, int SHAPE, int CM, bool VEC>
__global__ void __launch_bounds__(DD_THREADS) k_depth_dilate(const float* __restrict__ depth, int h, int w, int c, int dark, float threshold,
                                                             float* __restrict__ out) {
    constexpr int HG = (R + 3) / 4, NG = DD_GX + 2 * HG, PITCH = 4 * NG, ROWS = DD_TH + 2 * R;
    constexpr bool SQUARE = SHAPE == CS_DILATE_SQUARE;
    __shared__ __attribute__((aligned(16))) uint32_t s_key[ROWS * PITCH];
    __shared__ __attribute__((aligned(16))) uint32_t s_row[SQUARE ? ROWS * DD_TW : 4];   // square: the rows' horizontal maxima
    const int tid = threadIdx.x;
    const unsigned tiles_x = ((unsigned)w + DD_TW - 1) / DD_TW;
    const int X0 = (int)(blockIdx.x % tiles_x) * DD_TW, Y0 = (int)(blockIdx.x / tiles_x) * DD_TH;
    const size_t hw = (size_t)h * w;
    const float* frame = depth + (size_t)blockIdx.y * hw * (CM == 1 ? 1 : c);
    const uint32_t flip = dark ? 0xFFFFFFFFu : 0u;

    // the keys of the four pixels from column x4 of row y, into row `row`, group `gx` of the staged plane -> the pixels' gray values
    auto stage = [&](int row, int gx) -> Px4 {
        // (unsigned: a coordinate in front of the frame wraps to a large one, and none overflows next to 2^31)
        const unsigned y = (unsigned)Y0 + (unsigned)(row - R), x4 = (unsigned)X0 + 4u * (unsigned)(gx - HG);
        Px4 g;
        g.v[0] = g.v[1] = g.v[2] = g.v[3] = 0.0f;
        const bool inside = y < (unsigned)h && x4 < (unsigned)w;           // (VEC: w % 4 == 0, so x4 + 3 < w as well)
        if (inside) g = load_gray4<CM, VEC>(frame, (size_t)y * w + x4, (size_t)(y + 1) * w, c);   // (the guarded path stops at the row's end)
        uint32_t k[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const bool live = inside && (VEC || x4 + e < (unsigned)w) && g.v[e] == g.v[e];
            k[e] = live ? dilate_key(g.v[e]) ^ flip : 0u;
        }
        *reinterpret_cast<uint4*>(&s_key[row * PITCH + 4 * gx]) = make_uint4(k[0], k[1], k[2], k[3]);
        return g;
    };

    const int lj = tid & (DD_GX - 1), lrow = tid >> 4;
    const Px4 centre = stage(R + lrow, HG + lj);
    // the halo: R rows of NG groups above, R below, 2 HG groups beside each of the tile's rows
    constexpr int BAND = R * NG, HALO = 2 * BAND + DD_TH * 2 * HG;
    for (int s = tid; s < HALO; s += DD_THREADS) {
        int row, gx;
        if (s < BAND) { row = s / NG; gx = s % NG; }
        else if (s < 2 * BAND) { row = R + DD_TH + (s - BAND) / NG; gx = (s - BAND) % NG; }
        else { const int q = (s - 2 * BAND) % (2 * HG); row = R + (s - 2 * BAND) / (2 * HG); gx = q < HG ? q : DD_GX + q; }
        stage(row, gx);
    }
    __syncthreads();

    uint32_t m[4] = {0u, 0u, 0u, 0u};
    if (SQUARE) {
        for (int s = tid; s < ROWS * DD_GX; s += DD_THREADS) {
            const int row = s >> 4, j = s & (DD_GX - 1);
            uint32_t t[4] = {0u, 0u, 0u, 0u};
            chord4<R>(&s_key[row * PITCH + 4 * (HG + j)], t);
            *reinterpret_cast<uint4*>(&s_row[row * DD_TW + 4 * j]) = make_uint4(t[0], t[1], t[2], t[3]);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i <= 2 * R; i++) {
            const uint4 q = *reinterpret_cast<const uint4*>(&s_row[(lrow + i) * DD_TW + 4 * lj]);
            m[0] = umax(m[0], q.x); m[1] = umax(m[1], q.y); m[2] = umax(m[2], q.z); m[3] = umax(m[3], q.w);
        }
    } else {
        disc_chords<R, PITCH>(&s_key[lrow * PITCH + 4 * (HG + lj)], m, std::make_integer_sequence<int, 2 * R + 1>());
    }

    const unsigned y = (unsigned)Y0 + lrow, x4 = (unsigned)X0 + 4u * lj;
    if (y >= (unsigned)h || x4 >= (unsigned)w) return;                              // (the kernel's barriers lie behind)
    Px4 r;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float g = centre.v[k], best = dilate_value(m[k] ^ flip);   // (no candidate: the centre is NaN, and so is the difference)
        const float diff = dark ? g - best : best - g;
        r.v[k] = diff >= threshold ? best : g;
    }
    store4<VEC>(out + (size_t)blockIdx.y * hw, (size_t)y * w + x4, (size_t)(y + 1) * w, r);   // (the guarded path stops at the row's end)
}

template <int R, int SHAPE>
static void dilate_rs(const float* depth, int n, int h, int w, int c, int dark, float threshold, float* out, bool vec, hipStream_t stream) {
    const unsigned tiles = (((unsigned)w + DD_TW - 1) / DD_TW) * (((unsigned)h + DD_TH - 1) / DD_TH);
    const dim3 grid(tiles, (unsigned)n), block(DD_THREADS);
#define CS_DILATE(CM, VEC) \
    hipLaunchKernelGGL((k_depth_dilate<R, SHAPE, CM, VEC>), grid, block, 0, stream, depth, h, w, c, dark, threshold, out)
    if (c == 1) { if (vec) CS_DILATE(1, true); else CS_DILATE(1, false); }
    else if (c == 3) { if (vec) CS_DILATE(3, true); else CS_DILATE(3, false); }
    else { if (vec) CS_DILATE(0, true); else CS_DILATE(0, false); }   // (channel 0 of c: strided 4-byte loads; VEC is the store's path)
#undef CS_DILATE
}

template <int SHAPE>
static void dilate_s(const float* depth, int n, int h, int w, int c, int radius, int dark, float threshold, float* out, bool vec,
                     hipStream_t stream) {
    switch (radius) {
#define CS_DILATE_R(RR) case RR: dilate_rs<RR, SHAPE>(depth, n, h, w, c, dark, threshold, out, vec, stream); break;
    CS_DILATE_R(1) CS_DILATE_R(2) CS_DILATE_R(3) CS_DILATE_R(4) CS_DILATE_R(5) CS_DILATE_R(6) CS_DILATE_R(7) CS_DILATE_R(8)
#undef CS_DILATE_R
    }
}

hipError_t launch_depth_dilate(const float* depth, int n, int h, int w, int c, int radius, int shape, int near, float threshold, float* out,
                               hipStream_t stream) {
    const bool vec = vec4_path((size_t)w, {depth, out});   // (a lane's pixels lie in one row: every row must start on the grid)
    const int dark = near == CS_DILATE_NEAR_DARK;
    if (shape == CS_DILATE_SQUARE) dilate_s<CS_DILATE_SQUARE>(depth, n, h, w, c, radius, dark, threshold, out, vec, stream);
    else dilate_s<CS_DILATE_DISC>(depth, n, h, w, c, radius, dark, threshold, out, vec, stream);
    return hipGetLastError();
}

}  // namespace cs
