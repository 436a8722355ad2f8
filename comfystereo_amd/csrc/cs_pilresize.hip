// cs_pilresize.hip -- Pillow's 8-bit bicubic resize (PIL.Image.resize with all defaults on modes L and RGB, Pillow 12.2), byte
// for byte, and the code conversions StereoDiffusion's Fast mode does around it (reference stereodiffusion_nodes.py:415-423,
// :481-484, :569-573): float -> codes on the way in, a coloured depth -> gray codes, codes -> code / 255 on the way out.
//
// Pillow resamples 8-bit images in integers: per axis the taps of every output sample are computed in float64, normalised, and
// rounded to 22 fractional bits; a sample is clip8((2^21 + sum pixel * tap) >> 22).  Horizontal pass first, then vertical, the
// image between them uint8; a pass whose sizes agree is skipped.  Four kernels:
//   k_pil_taps     one thread per output sample of an axis: its window (first input sample, count) and fixed-point taps, float64
//                  in Pillow's order (-ffp-contract=off), into the workspace -- no host arithmetic, no host allocation
//   k_pil_h        horizontal pass: 64 output columns x up to 16 rows per workgroup; the input span of the tile is staged in LDS
//                  as codes (dword loads of interleaved bytes, or the float / gray conversion once per input sample)
//   k_pil_v        vertical pass: one lane per dword of an output row, looping over the taps in rows
//   k_pil_convert  both passes skipped (or a converted input ahead of a lone vertical pass): the conversions alone
// The last kernel of a call writes the outputs: uint8 NHWC and / or float32 code / 255 as NHWC (with a row pitch) or planar.
#include "cs_common.h"
#include "cs_kernels.h"

namespace cs {

enum { PIL_BITS = 22, PIL_TX = 64, PIL_THREADS = 256, PIL_RPT = 4, PIL_MAX_TAPS = 257, PIL_MAX_SIZE = 65535,
       PIL_LDS_BYTES = 65536 };
enum { PIL_IN_U8 = 0, PIL_IN_F32 = 1, PIL_IN_U8_GRAY = 2, PIL_IN_F32_GRAY = 3 };

// ---- taps -------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline double pil_scale(int in_size, int out_size) { return (double)in_size / (double)out_size; }
__host__ __device__ inline int pil_ksize(int in_size, int out_size) {
    const double scale = pil_scale(in_size, out_size);
    return (int)ceil(2.0 * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}

__device__ __forceinline__ double pil_bicubic(double t) {   // Keys, a = -0.5
    const double a = -0.5;
    if (t < 0.0) t = -t;
    if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1;
    if (t < 2.0) return (((t - 5) * t + 8) * t - 4) * a;
    return 0.0;
}

// bounds[xx] = (first input sample, count); taps[xx * ksize + k], or taps[k * out_size + xx] when transposed (the horizontal
// pass reads one tap index across a wave's columns); taps beyond count are 0
__global__ void __launch_bounds__(256) k_pil_taps(int in_size, int out_size, int ksize, int2* __restrict__ bounds,
                                                  int* __restrict__ taps, int transposed) {
    const int xx = blockIdx.x * blockDim.x + threadIdx.x;
    if (xx >= out_size) return;
    const double scale = pil_scale(in_size, out_size);
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs, ss = 1.0 / fs;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    const int n = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < n; x++) ww += pil_bicubic((x + xmin - center + 0.5) * ss);   // left to right
    for (int x = 0; x < ksize; x++) {
        int tap = 0;
        if (x < n) {
            double k = pil_bicubic((x + xmin - center + 0.5) * ss);
            if (ww != 0.0) k /= ww;
            tap = k < 0 ? (int)(-0.5 + k * (double)(1 << PIL_BITS)) : (int)(0.5 + k * (double)(1 << PIL_BITS));
        }
        taps[transposed ? (size_t)x * out_size + xx : (size_t)xx * ksize + x] = tap;
    }
    bounds[xx] = make_int2(xmin, n);
}

// ---- the two ends -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pil_code(float v) {   // trunc(clip(255 * x, 0, 255)) (:55, tensor_to_numpy)
    return (int)fminf(fmaxf(255.0f * v, 0.0f), 255.0f);
}
// The gray of a coloured depth (:419) in one fixed order, float64.  The reference's np.dot goes through BLAS, whose summation
// order depends on the array's shape: measured on all 2^24 triples it disagrees with this order on 276 of them laid out as
// [4096,4096,3], on 224 as [16777216,3] -- it does not agree with itself.  On equal channels (what depth estimators deliver)
// k * 0.9999 is never within rounding of an integer and every order gives k - 1 (0 for k = 0).
__device__ __forceinline__ int pil_gray(int r, int g, int b) {
    return (int)(((double)r * 0.2989 + (double)g * 0.5870) + (double)b * 0.1140);
}
__device__ __forceinline__ int pil_clip8(int acc) {
    const int v = acc >> PIL_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// code of output channel ch of input pixel `pix` (flat over frames, rows, columns)
template <int MODE>
__device__ __forceinline__ int pil_fetch(const void* in, size_t pix, int c, int ch) {
    if (MODE == PIL_IN_U8) return ((const uint8_t*)in)[pix * c + ch];
    if (MODE == PIL_IN_F32) return pil_code(((const float*)in)[pix * c + ch]);
    if (MODE == PIL_IN_U8_GRAY) {
        const uint8_t* p = (const uint8_t*)in + pix * 3;
        return pil_gray(p[0], p[1], p[2]);
    }
    const float* p = (const float*)in + pix * 3;
    return pil_gray(pil_code(p[0]), pil_code(p[1]), pil_code(p[2]));
}

struct PilOut {
    uint8_t* u8;     // [n][oh][ow][c] or null
    float* f32;      // code / 255: [n][oh] rows of `pitch` floats holding [ow][c], or planar [n][c][oh][ow]; or null
    size_t pitch;
    int planar, c, oh, ow;
};
__device__ __forceinline__ void pil_emit(const PilOut& O, int f, int y, int x, int ch, int code) {
    if (O.u8) O.u8[(((size_t)f * O.oh + y) * O.ow + x) * O.c + ch] = (uint8_t)code;
    if (O.f32) {
        const float v = (float)code / 255.0f;
        if (O.planar) O.f32[(((size_t)f * O.c + ch) * O.oh + y) * O.ow + x] = v;
        else O.f32[((size_t)f * O.oh + y) * O.pitch + (size_t)x * O.c + ch] = v;
    }
}

// ---- horizontal pass --------------------------------------------------------------------------------------------------------
// grid (ow tiles, row groups, n); `rows` image rows per workgroup (a multiple of 4 up to 16), each `pitch_w` LDS words
template <int MODE>
__global__ void __launch_bounds__(PIL_THREADS) k_pil_h(const void* __restrict__ in, size_t in_bytes, int h, int w, int c, int ow,
                                                       const int2* __restrict__ hb, const int* __restrict__ ht, int rows,
                                                       int pitch_w, PilOut O) {
    extern __shared__ uint32_t pil_lds[];
    const int tid = threadIdx.x, f = blockIdx.z, y0 = blockIdx.y * rows, col0 = blockIdx.x * PIL_TX;
    const int last = min(col0 + PIL_TX, ow) - 1;
    const int x0 = hb[col0].x;
    const int2 bl = hb[last];
    const int nbytes = (bl.x + bl.y - x0) * c;          // windows only move right: the tile's span ends with its last column's
    if (nbytes + 3 > pitch_w * 4) return;               // (the host sized the row from the same bound)
    const int nrows = min(rows, h - y0);

    // MODE U8: a row is staged from the dword at or below its first byte (`shift` = that byte's offset in the dword)
    for (int r = 0; r < nrows; r++) {
        const size_t pix0 = ((size_t)f * h + y0 + r) * w + x0;
        uint32_t* row = pil_lds + (size_t)r * pitch_w;
        if (MODE == PIL_IN_U8) {
            const uint8_t* lo = (const uint8_t*)in, *hi = lo + in_bytes;
            const uint8_t* base = lo + pix0 * c;
            const int shift = (int)((uintptr_t)base & 3);
            const int nd = (shift + nbytes + 3) >> 2;
            for (int i = tid; i < nd; i += PIL_THREADS) {
                const uint8_t* a = base - shift + (size_t)i * 4;
                uint32_t v = 0;
                if (a >= lo && a + 4 <= hi) {
                    v = *(const uint32_t*)a;
                } else {
                    for (int b = 0; b < 4; b++)
                        if (a + b >= lo && a + b < hi) v |= (uint32_t)a[b] << (8 * b);
                }
                row[i] = v;
            }
        } else {
            uint8_t* rowb = (uint8_t*)row;
            for (int i = tid; i < nbytes; i += PIL_THREADS) rowb[i] = (uint8_t)pil_fetch<MODE>(in, pix0 + i / c, c, i % c);
        }
    }
    __syncthreads();

    const int xx = col0 + (tid & (PIL_TX - 1)), rsub = tid / PIL_TX;
    if (xx >= ow) return;
    const int2 b = hb[xx];
    int acc[PIL_RPT][3];
    int off[PIL_RPT];
    for (int i = 0; i < PIL_RPT; i++) {
        const int r = rsub + (PIL_THREADS / PIL_TX) * i;
        int shift = 0;
        if (MODE == PIL_IN_U8) shift = (int)((uintptr_t)((const uint8_t*)in + (((size_t)f * h + y0 + r) * w + x0) * c) & 3);
        off[i] = r * pitch_w * 4 + shift + (b.x - x0) * c;
        for (int ch = 0; ch < 3; ch++) acc[i][ch] = 1 << (PIL_BITS - 1);
    }
    const uint8_t* lds = (const uint8_t*)pil_lds;
    for (int k = 0; k < b.y; k++) {
        const int tap = ht[(size_t)k * ow + xx];
#pragma unroll
        for (int i = 0; i < PIL_RPT; i++) {
            if (rsub + (PIL_THREADS / PIL_TX) * i < nrows) {
                const uint8_t* p = lds + off[i] + k * c;
                if (c == 3) {
                    acc[i][0] += (int)p[0] * tap;
                    acc[i][1] += (int)p[1] * tap;
                    acc[i][2] += (int)p[2] * tap;
                } else {
                    acc[i][0] += (int)p[0] * tap;
                }
            }
        }
    }
    for (int i = 0; i < PIL_RPT; i++) {
        const int r = rsub + (PIL_THREADS / PIL_TX) * i;
        if (r < nrows)
            for (int ch = 0; ch < c; ch++) pil_emit(O, f, y0 + r, xx, ch, pil_clip8(acc[i][ch]));
    }
}

// ---- vertical pass ----------------------------------------------------------------------------------------------------------
// src [n][h] rows of rowbytes = ow * c codes; grid (dwords of a row / 256, oh, n).  ALIGNED: every row of src and of O.u8 starts
// on a dword; VEC: the float rows of an NHWC O.f32 take float4 stores
template <bool ALIGNED, bool VEC>
__global__ void __launch_bounds__(256) k_pil_v(const uint8_t* __restrict__ src, int h, int rowbytes, const int2* __restrict__ vb,
                                               const int* __restrict__ vt, int ksize, PilOut O) {
    const int f = blockIdx.z, yy = blockIdx.y, j4 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (j4 >= rowbytes) return;
    const int2 b = vb[yy];
    const int* t = vt + (size_t)yy * ksize;
    int acc[4];
    for (int i = 0; i < 4; i++) acc[i] = 1 << (PIL_BITS - 1);
    const uint8_t* p = src + ((size_t)f * h + b.x) * rowbytes + j4;
    const int nb = ALIGNED ? 4 : min(4, rowbytes - j4);
    for (int k = 0; k < b.y; k++, p += rowbytes) {
        const int tap = t[k];
        if (ALIGNED) {
            const uint32_t v = *(const uint32_t*)p;
            for (int i = 0; i < 4; i++) acc[i] += (int)((v >> (8 * i)) & 255u) * tap;
        } else {
            for (int i = 0; i < 4; i++)
                if (i < nb) acc[i] += (int)p[i] * tap;
        }
    }
    int code[4];
    for (int i = 0; i < 4; i++) code[i] = pil_clip8(acc[i]);
    if (ALIGNED) {
        if (O.u8)
            *(uint32_t*)(O.u8 + ((size_t)f * O.oh + yy) * rowbytes + j4) =
                (uint32_t)code[0] | ((uint32_t)code[1] << 8) | ((uint32_t)code[2] << 16) | ((uint32_t)code[3] << 24);
        if (VEC && O.f32)
            *(float4*)(O.f32 + ((size_t)f * O.oh + yy) * O.pitch + j4) =
                make_float4((float)code[0] / 255.0f, (float)code[1] / 255.0f, (float)code[2] / 255.0f, (float)code[3] / 255.0f);
        if (VEC || !O.f32) return;
        PilOut F = O;
        F.u8 = nullptr;
        for (int i = 0; i < 4; i++) pil_emit(F, f, yy, (j4 + i) / O.c, (j4 + i) % O.c, code[i]);
    } else {
        for (int i = 0; i < nb; i++) pil_emit(O, f, yy, (j4 + i) / O.c, (j4 + i) % O.c, code[i]);
    }
}

// ---- no pass ----------------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ void __launch_bounds__(256) k_pil_convert(const void* __restrict__ in, int c_in, size_t per_frame, PilOut O) {
    const int f = blockIdx.y;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < per_frame; i += (size_t)gridDim.x * 256) {
        const size_t pix = i / O.c;
        const int ch = (int)(i % O.c);
        pil_emit(O, f, (int)(pix / O.ow), (int)(pix % O.ow), ch, pil_fetch<MODE>(in, (size_t)f * O.oh * O.ow + pix, c_in, ch));
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
int pilresize_max_taps() { return PIL_MAX_TAPS; }
int pilresize_max_size() { return PIL_MAX_SIZE; }

static size_t pil_al(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace: [h bounds][h taps][v bounds][v taps][codes between the passes]
struct PilLayout { size_t hb, ht, vb, vt, mid, total; int kh, kv; bool need_mid; };
static PilLayout pil_layout(int n, int h, int w, int c_out, int oh, int ow, bool converts) {
    PilLayout L;
    const bool hp = w != ow, vp = h != oh;
    L.kh = hp ? pil_ksize(w, ow) : 0;
    L.kv = vp ? pil_ksize(h, oh) : 0;
    size_t o = 0;
    L.hb = o; o += pil_al((size_t)ow * 8);
    L.ht = o; o += pil_al((size_t)ow * L.kh * 4);
    L.vb = o; o += pil_al((size_t)oh * 8);
    L.vt = o; o += pil_al((size_t)oh * L.kv * 4);
    L.need_mid = vp && (hp || converts);
    L.mid = o; if (L.need_mid) o += pil_al((size_t)n * h * ow * c_out);
    L.total = o;
    return L;
}

size_t pilresize_workspace_bytes(int n, int h, int w, int c_out, int oh, int ow) {
    // (sized for a converting input: the caller need not know the input format to allocate)
    return pil_layout(n, h, w, c_out, oh, ow, true).total;
}

// LDS words per staged row of the horizontal pass: 64 columns move the window 63 * scale, a window is 2 * support wide
static int pil_pitch_words(int w, int ow, int c) {
    const double scale = pil_scale(w, ow), support = 2.0 * (scale < 1.0 ? 1.0 : scale);
    double span = ceil((PIL_TX - 1) * scale + 2.0 * support) + 2.0;
    if (span > w) span = w;
    return ((int)span * c + 3 + 3) / 4 + 1;
}

bool pilresize_fits(int h, int w, int oh, int ow) {
    if (h > PIL_MAX_SIZE || w > PIL_MAX_SIZE || oh > PIL_MAX_SIZE || ow > PIL_MAX_SIZE) return false;
    if (w != ow && pil_ksize(w, ow) > PIL_MAX_TAPS) return false;
    if (h != oh && pil_ksize(h, oh) > PIL_MAX_TAPS) return false;
    return true;
}

template <int MODE>
static void pil_launch_front(const void* in, size_t in_bytes, int n, int h, int w, int c_in, int c, int ow, bool hp,
                             const PilLayout& L, char* ws, const PilOut& O, hipStream_t stream) {
    if (hp) {
        const int pitch_w = pil_pitch_words(w, ow, c);
        const int rows = (size_t)pitch_w * 4 * 16 <= 49152 ? 16 : 4;
        hipLaunchKernelGGL(k_pil_h<MODE>, dim3((ow + PIL_TX - 1) / PIL_TX, (h + rows - 1) / rows, n), dim3(PIL_THREADS),
                           (size_t)pitch_w * 4 * rows, stream, in, in_bytes, h, w, c, ow, (const int2*)(ws + L.hb),
                           (const int*)(ws + L.ht), rows, pitch_w, O);
    } else {
        const size_t per_frame = (size_t)h * w * c;
        const size_t blocks = (per_frame + 255) / 256;
        hipLaunchKernelGGL(k_pil_convert<MODE>, dim3((unsigned)(blocks < 65536 ? blocks : 65536), n), dim3(256), 0, stream, in,
                           c_in, per_frame, O);
    }
}

hipError_t launch_pilresize(const void* in, int in_f32, int gray, int n, int h, int w, int c_in, int oh, int ow, uint8_t* out_u8,
                            float* out_f32, int planar, size_t pitch, void* workspace, hipStream_t stream) {
    const int c = gray ? 1 : c_in;
    const int mode = (in_f32 ? 1 : 0) + (gray ? 2 : 0);
    const bool hp = w != ow, vp = h != oh;
    const PilLayout L = pil_layout(n, h, w, c, oh, ow, mode != PIL_IN_U8);
    char* ws = (char*)workspace;
    if (hp) hipLaunchKernelGGL(k_pil_taps, dim3((ow + 255) / 256), dim3(256), 0, stream, w, ow, L.kh, (int2*)(ws + L.hb),
                               (int*)(ws + L.ht), 1);
    if (vp) hipLaunchKernelGGL(k_pil_taps, dim3((oh + 255) / 256), dim3(256), 0, stream, h, oh, L.kv, (int2*)(ws + L.vb),
                               (int*)(ws + L.vt), 0);
    PilOut fin;
    fin.u8 = out_u8; fin.f32 = out_f32; fin.pitch = pitch; fin.planar = planar; fin.c = c; fin.oh = oh; fin.ow = ow;
    PilOut mid;
    mid.u8 = (uint8_t*)(ws + L.mid); mid.f32 = nullptr; mid.pitch = 0; mid.planar = 0; mid.c = c; mid.oh = h; mid.ow = ow;
    const size_t in_bytes = (size_t)n * h * w * c_in * (in_f32 ? 4 : 1);
    const uint8_t* vsrc = (const uint8_t*)in;
    if (hp || !vp || L.need_mid) {
        const PilOut& O = vp ? mid : fin;
        switch (mode) {
            case PIL_IN_U8: pil_launch_front<PIL_IN_U8>(in, in_bytes, n, h, w, c_in, c, ow, hp, L, ws, O, stream); break;
            case PIL_IN_F32: pil_launch_front<PIL_IN_F32>(in, in_bytes, n, h, w, c_in, c, ow, hp, L, ws, O, stream); break;
            case PIL_IN_U8_GRAY: pil_launch_front<PIL_IN_U8_GRAY>(in, in_bytes, n, h, w, c_in, c, ow, hp, L, ws, O, stream); break;
            default: pil_launch_front<PIL_IN_F32_GRAY>(in, in_bytes, n, h, w, c_in, c, ow, hp, L, ws, O, stream); break;
        }
        vsrc = mid.u8;
    }
    if (vp) {
        const int rowbytes = ow * c;
        const bool aligned = (rowbytes & 3) == 0 && ((uintptr_t)vsrc & 3) == 0 && ((uintptr_t)out_u8 & 3) == 0;
        const bool vec = aligned && out_f32 && !planar && (pitch & 3) == 0 && ((uintptr_t)out_f32 & 15) == 0;
        const dim3 grid(((rowbytes + 3) / 4 + 255) / 256, oh, n);
        const int2* vb = (const int2*)(ws + L.vb);
        const int* vt = (const int*)(ws + L.vt);
        if (vec) hipLaunchKernelGGL((k_pil_v<true, true>), grid, dim3(256), 0, stream, vsrc, h, rowbytes, vb, vt, L.kv, fin);
        else if (aligned) hipLaunchKernelGGL((k_pil_v<true, false>), grid, dim3(256), 0, stream, vsrc, h, rowbytes, vb, vt, L.kv, fin);
        else hipLaunchKernelGGL((k_pil_v<false, false>), grid, dim3(256), 0, stream, vsrc, h, rowbytes, vb, vt, L.kv, fin);
    }
    return hipGetLastError();
}

}  // namespace cs
