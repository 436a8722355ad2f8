// cs_attention_half.hip -- cs_attention.hip's stereo attention with float16 / bfloat16 q, k, v and output, on the half-input MFMA
// (v_mfma_f32_32x32x16_f16 / _bf16).  Same routing, index maps and decomposition as k_stereo_attention; scores, the online
// softmax (running maximum, sum, rescale) and both accumulators are float32, only the MFMA operands (Q, K, V, and P after the
// exponential) are half.  No score matrix, no workspace.
//
// One wave owns 32 queries; a workgroup of NW waves shares the 32-key K / V tiles in LDS.  Fragments, the transposed LDS image and
// the banking argument are cs_attention_tile.h's.  Per tile a wave computes
//   S^T = K . Q^T   lane (r, h) holds K[key r][d = 16 g + 8 h + j], j = 0..7, of k-step g (one ds_read_b128 from the row-major
//                   Ks, rows 32 ND + 8 halves apart) and the matching eight Q elements of its query in registers; d is zero-padded
//                   to a multiple of 16.  The accumulator has the query on the lane and key at_row(reg, h) in register reg, as in
//                   the float32 kernel.
//   O^T += V^T . P^T  registers 8 s .. 8 s + 7 of the S^T accumulator, converted to half, are the B fragment of k-step s; the A
//                   fragment is V of those eight keys at output column 32 blk + r, read from Vt[column][slot], V staged
//                   transposed and key-permuted (stage(), the same store as sah_store_t).
// The next tile's K / V are loaded into registers before this tile's products and stored to LDS after them.
#include "cs_attention_tile.h"
#include "cs_common.h"
#include "cs_kernels.h"

namespace cs {

// LSE (cs_attention_half_fwd_lse, the forward of the differentiable half attention): besides `out`, the log-sum-exp of every
// query's scaled scores goes to lse [(c s b h)][n] as float32, in log2 units like sc2, from the float32 running maximum and sum:
// p(i, j) = exp2(sc2 * s(i, j) - lse(i)).  Nothing else differs.
template <typename T, int ND, int NW, bool LSE = false>
__global__ void __launch_bounds__(NW * 64) k_stereo_attention_half(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                                                                   T* __restrict__ out, int S, int B, int H, int n, int n_k, int d,
                                                                   float scale, int mode, int qtiles, float* __restrict__ lse = nullptr) {
    typedef typename sah_frag<T>::type frag;
    constexpr int SK = ND * 32 + 8, NT = NW * 64;
    constexpr int KI = (AT_T * ND * 4 + NT - 1) / NT;         // 16-byte K chunks of a tile per thread
    constexpr int VI = (AT_T / 2 * ND * 4 + NT - 1) / NT;     // (key pair, 8-column chunk) tasks of a V tile per thread
    __shared__ __attribute__((aligned(16))) T Ks[AT_T * SK];
    __shared__ __attribute__((aligned(16))) T Vt[ND * 32 * SAH_SVT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hi = lane >> 5;
    const int bh = blockIdx.x / qtiles, qt = blockIdx.x - bh * qtiles;
    // (c s b h) -> the key set: view 0 of the same (c, b, h) for UNI / BI, followed by view 1 for BI
    const int hh = bh % H, sb = bh / H, s = (sb / B) % S;
    const size_t kset = mode == CS_ATTN_SELF ? (size_t)bh : (size_t)bh - (size_t)s * B * H;
    const int nkeys = mode == CS_ATTN_BI ? 2 * n_k : n_k;
    const size_t view_rows = (size_t)(B * H - 1) * n_k;   // BI: rows between the end of view 0's keys and the start of view 1's
    const T* kb = k + kset * n_k * d;
    const T* vb = v + kset * n_k * d;
    const int d8 = d >> 3;

    // K's pad columns (d .. SK) are multiplied by Q's zero pad, Vt's rows past d feed output columns nobody stores, keys past
    // the set are multiplied by p = 0: all of them must be finite
    for (int i = tid; i < AT_T * SK / 2; i += NT) ((unsigned*)Ks)[i] = 0u;
    for (int i = tid; i < ND * 32 * SAH_SVT / 2; i += NT) ((unsigned*)Vt)[i] = 0u;

    // Q fragment: query `col` of this wave, d = 16 g + 8 hi .. + 7 in qf[g]; zero past d and past n
    const int qi = (qt * NW + wave) * 32 + col;
    const bool q_ok = qi < n;
    const T* qrow = q + ((size_t)bh * n + (q_ok ? qi : 0)) * d;
    frag qf[ND * 2];
#pragma unroll
    for (int g = 0; g < ND * 2; g++) {
        const int c0 = 16 * g + 8 * hi;
        uint4 raw = make_uint4(0u, 0u, 0u, 0u);
        if (q_ok && c0 < d) raw = *(const uint4*)(qrow + c0);
        qf[g] = __builtin_bit_cast(frag, raw);
    }

    at_acc o[ND];
#pragma unroll
    for (int b = 0; b < ND; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[b][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;
    const float sc2 = scale * 1.44269504088896340736f;   // scores in units of log2: p = exp2(s - m)

    // a tile's K and V in registers: K chunk e = (row e / d8, 8 columns e % d8); V task e = (key pair e & 15, 8 columns e >> 4)
    uint4 kr[KI], va[VI], vc[VI];
    auto fetch = [&](int kt) {
#pragma unroll
        for (int it = 0; it < KI; it++) {
            const int e = tid + it * NT;
            const int row = e / d8, c8 = e - row * d8;
            const int j = kt * AT_T + row;
            kr[it] = make_uint4(0u, 0u, 0u, 0u);
            if (row < AT_T && j < nkeys) kr[it] = *(const uint4*)(kb + ((size_t)j + (j >= n_k ? view_rows : 0)) * d + 8 * c8);
        }
#pragma unroll
        for (int it = 0; it < VI; it++) {
            const int e = tid + it * NT;
            const int c8 = e >> 4, j = kt * AT_T + 2 * (e & 15);
            va[it] = vc[it] = make_uint4(0u, 0u, 0u, 0u);
            if (c8 < d8) {
                if (j < nkeys) va[it] = *(const uint4*)(vb + ((size_t)j + (j >= n_k ? view_rows : 0)) * d + 8 * c8);
                if (j + 1 < nkeys) vc[it] = *(const uint4*)(vb + ((size_t)(j + 1) + (j + 1 >= n_k ? view_rows : 0)) * d + 8 * c8);
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int it = 0; it < KI; it++) {
            const int e = tid + it * NT;
            const int row = e / d8, c8 = e - row * d8;
            if (row < AT_T) *(uint4*)(Ks + row * SK + 8 * c8) = kr[it];
        }
#pragma unroll
        for (int it = 0; it < VI; it++) {
            const int e = tid + it * NT;
            const int c8 = e >> 4, slot = sah_slot(2 * (e & 15));
            const bool odd = c8 & 1;
            if (c8 < d8) {
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const unsigned lo = odd ? sah_elem(va[it], i ^ 4) : sah_elem(va[it], i);
                    const unsigned up = odd ? sah_elem(vc[it], i ^ 4) : sah_elem(vc[it], i);
                    const int c = 8 * c8 + (odd ? (i ^ 4) : i);
                    *(unsigned*)(Vt + c * SAH_SVT + slot) = lo | (up << 16);
                }
            }
        }
    };

    const int ntiles = (nkeys + AT_T - 1) / AT_T;
    fetch(0);
    for (int kt = 0; kt < ntiles; kt++) {
        __syncthreads();   // the previous tile's readers (first pass: the zero fill) are done
        stage();
        __syncthreads();
        if (kt + 1 < ntiles) fetch(kt + 1);

        // S^T = K . Q^T
        at_acc st;
#pragma unroll
        for (int r = 0; r < 16; r++) st[r] = 0.0f;
#pragma unroll
        for (int g = 0; g < ND * 2; g++) {
            if (16 * g < d) {
                const frag kf = *(const frag*)(Ks + col * SK + 16 * g + 8 * hi);
                st = sah_frag<T>::mfma(kf, qf[g], st);
            }
        }
        // keys past the set: -inf BEFORE the running maximum is updated (tile 0 always holds key 0, so the maximum is
        // finite from the first tile on and exp2(-inf - m) = 0 is the only form -inf takes)
        const int key0 = kt * AT_T;
        const bool tail = key0 + AT_T > nkeys;
        float m_tile = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            float sv = st[r] * sc2;
            if (tail && key0 + at_row(r, hi) >= nkeys) sv = -INFINITY;
            st[r] = sv;
            m_tile = fmaxf(m_tile, sv);
        }
        m_tile = fmaxf(m_tile, __shfl_xor(m_tile, 32));
        const float m_new = fmaxf(m_run, m_tile);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // first tile: exp2(-inf) = 0
        m_run = m_new;
        float psum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            st[r] = __builtin_amdgcn_exp2f(st[r] - m_new);
            psum += st[r];
        }
        l_run = l_run * alpha + psum;   // this lane half's 16 keys; the halves are added after the last tile
#pragma unroll
        for (int b = 0; b < ND; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) o[b][r] *= alpha;

        // O^T += V^T . P^T
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            frag pf;
#pragma unroll
            for (int j = 0; j < 8; j++) pf[j] = (T)st[8 * ks + j];
#pragma unroll
            for (int b = 0; b < ND; b++) {
                const frag vf = *(const frag*)(Vt + (b * 32 + col) * SAH_SVT + 16 * ks + 8 * hi);
                o[b] = sah_frag<T>::mfma(vf, pf, o[b]);
            }
        }
    }

    const float l_all = l_run + __shfl_xor(l_run, 32);
    if (!q_ok) return;
    if (LSE && hi == 0) lse[(size_t)bh * n + qi] = m_run + __builtin_amdgcn_logf(l_all);   // (v_log_f32 is log2; l_all >= 1)
    // out [(c s b)][n][(h d)]: lane (query, hi) holds columns 32 blk + 8 g + 4 hi .. + 3 in registers 4 g .. 4 g + 3
    T* orow = out + ((size_t)sb * n + qi) * ((size_t)H * d) + (size_t)hh * d;
#pragma unroll
    for (int b = 0; b < ND; b++) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int c0 = b * 32 + 8 * g + 4 * hi;
            if (c0 < d) {
                typedef T t4 __attribute__((ext_vector_type(4)));
                t4 r4;
#pragma unroll
                for (int j = 0; j < 4; j++) r4[j] = (T)(o[b][4 * g + j] / l_all);
                *(t4*)(orow + c0) = r4;
            }
        }
    }
}

// workgroup shapes: attention_waves (cs_attention.hip), with its development switch
template <bool LSE>
static hipError_t sah_launch(const void* q, const void* k, const void* v, void* out, float* lse, int dtype, int c, int s, int b, int h,
                             int n, int n_k, int d, float scale, int mode, hipStream_t stream) {
    const long long bhn = (long long)c * s * b * h;
    const int nw = attention_waves(bhn, n);
    const int qtiles = (n + 32 * nw - 1) / (32 * nw);
    const int blocks = (int)(bhn * qtiles);
    return sah_dispatch(dtype, [&](auto* tag) {
        typedef std::remove_pointer_t<decltype(tag)> T;
        const T *tq = (const T*)q, *tk = (const T*)k, *tv = (const T*)v;
        T* to = (T*)out;
        return at_dispatch(d, nw, [&](auto nd, auto nwc) {
            constexpr int ND = decltype(nd)::value, NW = decltype(nwc)::value;
            hipLaunchKernelGGL((k_stereo_attention_half<T, ND, NW, LSE>), dim3(blocks), dim3(NW * 64), 0, stream, tq, tk, tv, to, s, b, h,
                               n, n_k, d, scale, mode, qtiles, lse);
            return hipGetLastError();
        });
    });
}

hipError_t launch_stereo_attention_half(const void* q, const void* k, const void* v, void* out, int dtype, int c, int s, int b, int h,
                                        int n, int n_k, int d, float scale, int mode, hipStream_t stream) {
    return sah_launch<false>(q, k, v, out, nullptr, dtype, c, s, b, h, n, n_k, d, scale, mode, stream);
}

// the same launch as launch_stereo_attention_half(..., CS_ATTN_SELF) with c = s = 1: `out` is bit for bit that call's
hipError_t launch_attention_half_fwd_lse(const void* q, const void* k, const void* v, void* out, float* lse, int dtype, int b, int h, int n,
                                         int n_k, int d, float scale, hipStream_t stream) {
    return sah_launch<true>(q, k, v, out, lse, dtype, 1, 1, b, h, n, n_k, d, scale, CS_ATTN_SELF, stream);
}

}  // namespace cs
