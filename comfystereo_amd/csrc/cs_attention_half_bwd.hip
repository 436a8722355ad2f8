// cs_attention_half_bwd.hip -- cs_attention_bwd.hip's backward pass of the fused attention with float16 / bfloat16 q, k, v, out,
// d_out and gradients, on the half-input MFMA (v_mfma_f32_32x32x16_f16 / _bf16): cs_attention_half_bwd, CS_ATTN_SELF semantics, for
// null-text inversion on half models.  The forward is k_stereo_attention_half<.., LSE = true> (cs_attention_half.hip): it leaves
// one float32 per query, lse(i) = log2 sum_j exp2(sc2 * s(i, j)), sc2 = scale * log2(e).  Same decomposition as the float32 backward:
//   delta(i) = sum_c dO(i, c) * O(i, c),   P = exp2(sc2 * s - lse),   dP = dO . V^T,   dS = P o (dP - delta)
//   dV = P^T . dO,   dK = scale * dS^T . Q,   dQ = scale * dS . K
// in three kernels, nothing of size n x n_k stored:
//   k_attention_half_delta      one thread per (b h, query): delta in float32 into the workspace (an fmaf chain over the columns);
//   k_attention_half_bwd_dkdv   a wave owns 32 keys and walks the 32-query tiles; the NW waves of a workgroup own NW consecutive key
//                               tiles of one (b h) and share the Q / dO tiles (and their lse / delta) in LDS;
//   k_attention_half_bwd_dq     a wave owns 32 queries and walks the 32-key tiles, like the forward; the workgroup shares K / V.
// Every gradient element is accumulated in float32 by ONE lane in a fixed order and stored once, rounded to nearest-even into the
// half dtype: no atomics, and the result is bit for bit the same from run to run.
//
// Layouts: q, dq [(b h)][n][d]; k, v, dk, dv [(b h)][n_k][d]; out, d_out [(b)][n][(h d)]; lse, delta [(b h)][n] float32.
//
// All five products run on the half-input MFMA.  Its operands are Q, K, V and dO as they arrive, and P and dS converted to half
// (nearest-even) after the float32 arithmetic that forms them; scores, exponentials, dP - delta and all accumulators are float32.
// Fragments, the accumulator's row map at_row and the transposed, row-permuted LDS images with their banking argument are
// cs_attention_tile.h's.
//   dq kernel    S^T = K . Q^T and dP^T = V . dO^T: the QUERY on the lane, lse and delta per-lane scalars; Q and dO fragments in
//                registers, K and V rows read from the row-major images Ks / Vs [key][d] with one ds_read_b128 per k-step.  Then
//                dQ^T += K^T . dS^T by the forward's operand trick: registers 8 s .. 8 s + 7 of the dS^T accumulator, converted to
//                half, are the B fragment of k-step s; the A fragment comes from Kt[column][slot], K staged transposed and
//                key-permuted (sah_store_t) like the forward's Vt.
//   dk/dv kernel S = Q . K^T and dP = dO . V^T: the KEY on the lane, K and V fragments in registers, Q and dO rows from the
//                row-major images Qs / Ds [query][d]; lse and delta of a register's query from LDS (broadcast float4 reads).  Then
//                dV^T += dO^T . P and dK^T += Q^T . dS with the P / dS registers as B fragments and the A fragments from the
//                transposed, query-permuted images Dt / Qt [column][slot].
// Rows of the row-major images are 32 ND + 8 halves apart, rows of the transposed images SAH_SVT = 40 halves.
// LDS per workgroup (independent of NW), ND = (d + 31) / 32 = 1 .. 5:
//   dq     Ks + Vs + Kt = 2 * 32 * (32 ND + 8) * 2 + 32 ND * 40 * 2 bytes:  7 680, 14 336, 20 992, 27 648, 34 304 (33.5 KiB at d = 160)
//   dk/dv  Qs + Ds + Qt + Dt + lse + delta = twice the K part of that + 256:  10 496, 19 712, 28 928, 38 144, 47 360 (46.25 KiB)
//
// Partial tiles, as in the float32 backward.  Keys past n_k: in the dq kernel the score is -inf before the exponential, P = 0, and
// the K / V rows are zeros, so dS = 0 * finite = 0; in the dk/dv kernel such a key is a column nobody stores.  Queries past n: Q and
// dO rows are zeros and lse = +inf, so P = exp2(0 - inf) = 0 and dS = 0 * (0 - 0) = 0: exact zeros into dK and dV; in the dq kernel
// such a query is a column nobody stores (lse read as 0: finite arithmetic).  Pad columns (d .. 32 ND + 8, and the rows of the
// transposed images past d) hold finite zeros from the initial fill and are never written.
//
// float16 range.  dS is formed in float32 and may be far below float16's smallest normal (6.1e-5) when dO is small (an MSE loss over
// a latent).  What the half-input MFMA does with float16 subnormal OPERANDS is not stated in the ISA guide this project works
// from: it says only that the C input and D output of an MFMA never flush and that the float32 A / B inputs honour MODE.denorm;
// the compiler's default kernel mode keeps float16 denormals (FP16_64 denorm mode 3), and v_cvt_f16_f32 under that mode rounds to
// subnormals instead of flushing.  dS is NOT scaled by a power of two before the conversion: with gradual underflow the absolute
// error of a converted dS is at most 2^-25, and the fixture's small-gradient case (d_out * 2^-12, float16) stays within the
// project's accuracy condition in the kernels' arithmetic (tools/attention_half_grad_oracle.py, tile_ratio in the fixture) because
// the reference rounds the same quantities to float16 too, twice.  bfloat16 has float32's range and needs no scaling.
#include "cs_attention_tile.h"
#include "cs_common.h"
#include "cs_kernels.h"

namespace cs {

template <typename T>
__global__ void __launch_bounds__(256) k_attention_half_delta(const T* __restrict__ out, const T* __restrict__ d_out,
                                                              float* __restrict__ delta, int H, int n, int d, size_t total) {
    typedef typename sah_frag<T>::type frag;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const size_t bh = idx / (size_t)n, i = idx - bh * n;
    const size_t off = ((bh / H) * n + i) * ((size_t)H * d) + (bh % H) * (size_t)d;
    float acc = 0.0f;
    for (int c = 0; c < d; c += 8) {
        const frag a = __builtin_bit_cast(frag, *(const uint4*)(d_out + off + c));
        const frag b = __builtin_bit_cast(frag, *(const uint4*)(out + off + c));
#pragma unroll
        for (int j = 0; j < 8; j++) acc = fmaf((float)a[j], (float)b[j], acc);
    }
    delta[idx] = acc;
}

template <typename T, int ND, int NW>
__global__ void __launch_bounds__(NW * 64) k_attention_half_bwd_dq(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                                                                   const T* __restrict__ d_out, const float* __restrict__ lse,
                                                                   const float* __restrict__ delta, T* __restrict__ dq, int H, int n,
                                                                   int n_k, int d, float scale, int qtiles) {
    typedef typename sah_frag<T>::type frag;
    constexpr int SK = ND * 32 + 8, NT = NW * 64;
    __shared__ __attribute__((aligned(16))) T Ks[AT_T * SK];
    __shared__ __attribute__((aligned(16))) T Vs[AT_T * SK];
    __shared__ __attribute__((aligned(16))) T Kt[ND * 32 * SAH_SVT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hi = lane >> 5;
    const int bh = blockIdx.x / qtiles, qt = blockIdx.x - bh * qtiles;
    const T* kb = k + (size_t)bh * n_k * d;
    const T* vb = v + (size_t)bh * n_k * d;
    const int d8 = d >> 3;

    for (int i = tid; i < AT_T * SK / 2; i += NT) { ((unsigned*)Ks)[i] = 0u; ((unsigned*)Vs)[i] = 0u; }
    for (int i = tid; i < ND * 32 * SAH_SVT / 2; i += NT) ((unsigned*)Kt)[i] = 0u;

    // Q and dO fragments of query `col`: d = 16 g + 8 hi .. + 7 in qf[g] / dof[g]; zero past d and past n
    const int qi = (qt * NW + wave) * 32 + col;
    const bool q_ok = qi < n;
    const int qs = q_ok ? qi : 0;
    const T* qrow = q + ((size_t)bh * n + qs) * d;
    const T* drow = d_out + ((size_t)(bh / H) * n + qs) * ((size_t)H * d) + (size_t)(bh % H) * d;
    frag qf[ND * 2], dof[ND * 2];
#pragma unroll
    for (int g = 0; g < ND * 2; g++) {
        const int c0 = 16 * g + 8 * hi;
        uint4 rq = make_uint4(0u, 0u, 0u, 0u), rd = rq;
        if (q_ok && c0 < d) { rq = *(const uint4*)(qrow + c0); rd = *(const uint4*)(drow + c0); }
        qf[g] = __builtin_bit_cast(frag, rq);
        dof[g] = __builtin_bit_cast(frag, rd);
    }
    const float lse_i = q_ok ? lse[(size_t)bh * n + qi] : 0.0f;
    const float delta_i = q_ok ? delta[(size_t)bh * n + qi] : 0.0f;

    at_acc acc[ND];
#pragma unroll
    for (int b = 0; b < ND; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[b][r] = 0.0f;
    const float sc2 = scale * 1.44269504088896340736f;
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);

    const int ntiles = (n_k + AT_T - 1) / AT_T;
    for (int kt = 0; kt < ntiles; kt++) {
        __syncthreads();   // the previous tile's readers (first pass: the zero fill) are done
        // task e = (key pair e & 15, 8 columns e >> 4): the pair's two chunks go to their rows of Ks / Vs and, transposed, to Kt
        for (int e = tid; e < 16 * d8; e += NT) {
            const int c8 = e >> 4, m2 = 2 * (e & 15), j = kt * AT_T + m2;
            uint4 ka = zero4, kc = zero4, va = zero4, vc = zero4;
            if (j < n_k) { ka = *(const uint4*)(kb + (size_t)j * d + 8 * c8); va = *(const uint4*)(vb + (size_t)j * d + 8 * c8); }
            if (j + 1 < n_k) { kc = *(const uint4*)(kb + (size_t)(j + 1) * d + 8 * c8); vc = *(const uint4*)(vb + (size_t)(j + 1) * d + 8 * c8); }
            *(uint4*)(Ks + m2 * SK + 8 * c8) = ka;
            *(uint4*)(Ks + (m2 + 1) * SK + 8 * c8) = kc;
            *(uint4*)(Vs + m2 * SK + 8 * c8) = va;
            *(uint4*)(Vs + (m2 + 1) * SK + 8 * c8) = vc;
            sah_store_t(Kt, ka, kc, c8, sah_slot(m2));
        }
        __syncthreads();

        // S^T = K . Q^T, dP^T = V . dO^T
        at_acc st, dp;
#pragma unroll
        for (int r = 0; r < 16; r++) { st[r] = 0.0f; dp[r] = 0.0f; }
#pragma unroll
        for (int g = 0; g < ND * 2; g++) {
            if (16 * g < d) {
                const frag kf = *(const frag*)(Ks + col * SK + 16 * g + 8 * hi);
                st = sah_frag<T>::mfma(kf, qf[g], st);
                const frag vf = *(const frag*)(Vs + col * SK + 16 * g + 8 * hi);
                dp = sah_frag<T>::mfma(vf, dof[g], dp);
            }
        }
        // dS^T = P^T o (dP^T - delta); keys past the set: the score is -inf, P = 0
        const int key0 = kt * AT_T;
        const bool tail = key0 + AT_T > n_k;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            float sv = st[r] * sc2;
            if (tail && key0 + at_row(r, hi) >= n_k) sv = -INFINITY;
            const float p = __builtin_amdgcn_exp2f(sv - lse_i);
            st[r] = p * (dp[r] - delta_i);
        }
        // dQ^T += K^T . dS^T
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            frag sf;
#pragma unroll
            for (int j = 0; j < 8; j++) sf[j] = (T)st[8 * ks + j];
#pragma unroll
            for (int b = 0; b < ND; b++) {
                const frag kf = *(const frag*)(Kt + (b * 32 + col) * SAH_SVT + 16 * ks + 8 * hi);
                acc[b] = sah_frag<T>::mfma(kf, sf, acc[b]);
            }
        }
    }

    if (!q_ok) return;
    // lane (query, hi) holds columns 32 blk + 8 g + 4 hi .. + 3 in registers 4 g .. 4 g + 3
    T* orow = dq + ((size_t)bh * n + qi) * d;
#pragma unroll
    for (int b = 0; b < ND; b++) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int c0 = b * 32 + 8 * g + 4 * hi;
            if (c0 < d) {
                typedef T t4 __attribute__((ext_vector_type(4)));
                t4 r4;
#pragma unroll
                for (int j = 0; j < 4; j++) r4[j] = (T)(acc[b][4 * g + j] * scale);
                *(t4*)(orow + c0) = r4;
            }
        }
    }
}

template <typename T, int ND, int NW>
__global__ void __launch_bounds__(NW * 64) k_attention_half_bwd_dkdv(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                                                                     const T* __restrict__ d_out, const float* __restrict__ lse,
                                                                     const float* __restrict__ delta, T* __restrict__ dk,
                                                                     T* __restrict__ dv, int H, int n, int n_k, int d, float scale,
                                                                     int kgroups) {
    typedef typename sah_frag<T>::type frag;
    constexpr int SK = ND * 32 + 8, NT = NW * 64;
    __shared__ __attribute__((aligned(16))) T Qs[AT_T * SK];
    __shared__ __attribute__((aligned(16))) T Ds[AT_T * SK];
    __shared__ __attribute__((aligned(16))) T Qt[ND * 32 * SAH_SVT];
    __shared__ __attribute__((aligned(16))) T Dt[ND * 32 * SAH_SVT];
    __shared__ __attribute__((aligned(16))) float Ls[AT_T];
    __shared__ __attribute__((aligned(16))) float Dl[AT_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hi = lane >> 5;
    const int bh = blockIdx.x / kgroups, kg = blockIdx.x - bh * kgroups;
    const T* qb = q + (size_t)bh * n * d;
    const T* db = d_out + (size_t)(bh / H) * n * ((size_t)H * d) + (size_t)(bh % H) * d;
    const size_t dstride = (size_t)H * d;
    const int d8 = d >> 3;

    for (int i = tid; i < AT_T * SK / 2; i += NT) { ((unsigned*)Qs)[i] = 0u; ((unsigned*)Ds)[i] = 0u; }
    for (int i = tid; i < ND * 32 * SAH_SVT / 2; i += NT) { ((unsigned*)Qt)[i] = 0u; ((unsigned*)Dt)[i] = 0u; }

    // K and V fragments of key `col` of this wave's tile: d = 16 g + 8 hi .. + 7 in kf[g] / vf[g]; zero past d and past n_k
    const int key0 = (kg * NW + wave) * 32;
    const bool wave_on = key0 < n_k;   // (wave-uniform; the barriers below are outside of what it guards)
    const int kj = key0 + col;
    const bool k_ok = kj < n_k;
    const T* krow = k + ((size_t)bh * n_k + (k_ok ? kj : 0)) * d;
    const T* vrow = v + ((size_t)bh * n_k + (k_ok ? kj : 0)) * d;
    frag kf[ND * 2], vf[ND * 2];
#pragma unroll
    for (int g = 0; g < ND * 2; g++) {
        const int c0 = 16 * g + 8 * hi;
        uint4 rk = make_uint4(0u, 0u, 0u, 0u), rv = rk;
        if (k_ok && c0 < d) { rk = *(const uint4*)(krow + c0); rv = *(const uint4*)(vrow + c0); }
        kf[g] = __builtin_bit_cast(frag, rk);
        vf[g] = __builtin_bit_cast(frag, rv);
    }

    at_acc ak[ND], av[ND];
#pragma unroll
    for (int b = 0; b < ND; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) { ak[b][r] = 0.0f; av[b][r] = 0.0f; }
    const float sc2 = scale * 1.44269504088896340736f;
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);

    const int ntiles = (n + AT_T - 1) / AT_T;
    for (int qt = 0; qt < ntiles; qt++) {
        __syncthreads();   // the previous tile's readers (first pass: the zero fill) are done
        // task e = (query pair e & 15, 8 columns e >> 4): the pair's chunks go to their rows of Qs / Ds and, transposed, to Qt / Dt
        for (int e = tid; e < 16 * d8; e += NT) {
            const int c8 = e >> 4, m2 = 2 * (e & 15), i = qt * AT_T + m2;
            uint4 qa = zero4, qc = zero4, da = zero4, dc = zero4;
            if (i < n) { qa = *(const uint4*)(qb + (size_t)i * d + 8 * c8); da = *(const uint4*)(db + (size_t)i * dstride + 8 * c8); }
            if (i + 1 < n) { qc = *(const uint4*)(qb + (size_t)(i + 1) * d + 8 * c8); dc = *(const uint4*)(db + (size_t)(i + 1) * dstride + 8 * c8); }
            *(uint4*)(Qs + m2 * SK + 8 * c8) = qa;
            *(uint4*)(Qs + (m2 + 1) * SK + 8 * c8) = qc;
            *(uint4*)(Ds + m2 * SK + 8 * c8) = da;
            *(uint4*)(Ds + (m2 + 1) * SK + 8 * c8) = dc;
            const int slot = sah_slot(m2);
            sah_store_t(Qt, qa, qc, c8, slot);
            sah_store_t(Dt, da, dc, c8, slot);
        }
        if (tid < AT_T) {
            const int i = qt * AT_T + tid;
            Ls[tid] = i < n ? lse[(size_t)bh * n + i] : INFINITY;   // a query past n: P = exp2(0 - inf) = 0
            Dl[tid] = i < n ? delta[(size_t)bh * n + i] : 0.0f;
        }
        __syncthreads();
        if (!wave_on) continue;

        // S = Q . K^T, dP = dO . V^T: the key on the lane, 16 queries in the registers
        at_acc st, dp;
#pragma unroll
        for (int r = 0; r < 16; r++) { st[r] = 0.0f; dp[r] = 0.0f; }
#pragma unroll
        for (int g = 0; g < ND * 2; g++) {
            if (16 * g < d) {
                const frag qa = *(const frag*)(Qs + col * SK + 16 * g + 8 * hi);
                st = sah_frag<T>::mfma(qa, kf[g], st);
                const frag da = *(const frag*)(Ds + col * SK + 16 * g + 8 * hi);
                dp = sah_frag<T>::mfma(da, vf[g], dp);
            }
        }
        // P and dS = P o (dP - delta): register 4 g + t is query 8 g + 4 hi + t
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const float4 l4 = *(const float4*)(Ls + 8 * g + 4 * hi), e4 = *(const float4*)(Dl + 8 * g + 4 * hi);
            const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, ev[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int r = 4 * g + t;
                const float p = __builtin_amdgcn_exp2f(st[r] * sc2 - lv[t]);
                st[r] = p;
                dp[r] = p * (dp[r] - ev[t]);
            }
        }
        // dV^T += dO^T . P, dK^T += Q^T . dS
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            frag pf, sf;
#pragma unroll
            for (int j = 0; j < 8; j++) { pf[j] = (T)st[8 * ks + j]; sf[j] = (T)dp[8 * ks + j]; }
#pragma unroll
            for (int b = 0; b < ND; b++) {
                const frag da = *(const frag*)(Dt + (b * 32 + col) * SAH_SVT + 16 * ks + 8 * hi);
                av[b] = sah_frag<T>::mfma(da, pf, av[b]);
                const frag qa = *(const frag*)(Qt + (b * 32 + col) * SAH_SVT + 16 * ks + 8 * hi);
                ak[b] = sah_frag<T>::mfma(qa, sf, ak[b]);
            }
        }
    }

    if (!k_ok) return;
    // lane (key, hi) holds columns 32 blk + 8 g + 4 hi .. + 3 in registers 4 g .. 4 g + 3
    T* krow_o = dk + ((size_t)bh * n_k + kj) * d;
    T* vrow_o = dv + ((size_t)bh * n_k + kj) * d;
#pragma unroll
    for (int b = 0; b < ND; b++) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int c0 = b * 32 + 8 * g + 4 * hi;
            if (c0 < d) {
                typedef T t4 __attribute__((ext_vector_type(4)));
                t4 k4, v4;
#pragma unroll
                for (int j = 0; j < 4; j++) { k4[j] = (T)(ak[b][4 * g + j] * scale); v4[j] = (T)av[b][4 * g + j]; }
                *(t4*)(krow_o + c0) = k4;
                *(t4*)(vrow_o + c0) = v4;
            }
        }
    }
}

// workgroup shapes: the forward's (attention_waves, with its development switch); a dk/dv workgroup of NW waves owns NW key tiles
// and a dq workgroup NW query tiles.  workspace: attention_bwd_workspace_bytes, delta as in the float32 backward
hipError_t launch_attention_half_bwd(const void* q, const void* k, const void* v, const void* out, const float* lse, const void* d_out,
                                     void* dq, void* dk, void* dv, int dtype, int b, int h, int n, int n_k, int d, float scale,
                                     void* workspace, hipStream_t stream) {
    const long long bhn = (long long)b * h;
    const int nw = attention_waves(bhn, n);
    float* delta = (float*)workspace;
    const size_t rows = (size_t)bhn * n;
    return sah_dispatch(dtype, [&](auto* tag) {
        typedef std::remove_pointer_t<decltype(tag)> T;
        const T *tq = (const T*)q, *tk = (const T*)k, *tv = (const T*)v, *to = (const T*)out, *td = (const T*)d_out;
        T *gq = (T*)dq, *gk = (T*)dk, *gv = (T*)dv;
        hipLaunchKernelGGL((k_attention_half_delta<T>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, to, td, delta, h, n, d, rows);
        return at_dispatch(d, nw, [&](auto nd, auto nwc) {
            constexpr int ND = decltype(nd)::value, NW = decltype(nwc)::value;
            const int kgroups = ((n_k + 31) / 32 + NW - 1) / NW, qtiles = (n + 32 * NW - 1) / (32 * NW);
            hipLaunchKernelGGL((k_attention_half_bwd_dkdv<T, ND, NW>), dim3((unsigned)(bhn * kgroups)), dim3(NW * 64), 0, stream, tq, tk, tv,
                               td, lse, delta, gk, gv, h, n, n_k, d, scale, kgroups);
            hipLaunchKernelGGL((k_attention_half_bwd_dq<T, ND, NW>), dim3((unsigned)(bhn * qtiles)), dim3(NW * 64), 0, stream, tq, tk, tv, td,
                               lse, delta, gq, h, n, n_k, d, scale, qtiles);
            return hipGetLastError();
        });
    });
}

}  // namespace cs
