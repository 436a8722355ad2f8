// cs_attention_bwd.hip -- the backward pass of the fused attention (cs_attention_bwd), CS_ATTN_SELF semantics, float32, for
// null-text inversion (reference inversion.py:184-212 trains the unconditional embedding through every attention layer of the UNet
// under the plain attention that diffusion_utils.py:158-292 installs).  The forward is k_stereo_attention<.., LSE = true>
// (cs_attention.hip): it leaves one float per query, lse(i) = log2 sum_j exp2(sc2 * s(i, j)), sc2 = scale * log2(e).  The
// backward recomputes the probabilities per 32 x 32 tile, P(i, j) = exp2(sc2 * s(i, j) - lse(i)), so nothing of size n x n_k is
// ever stored, and with
//   delta(i) = sum_c dO(i, c) * O(i, c),   dP = dO . V^T,   dS = P o (dP - delta)
// computes dV = P^T . dO,  dK = scale * dS^T . Q,  dQ = scale * dS . K  in three kernels:
//   k_attention_delta      one thread per (b h, query): delta into the workspace, in the MFMA's own summation order;
//   k_attention_bwd_dkdv   a wave owns 32 keys and walks the query tiles; the NW waves of a workgroup own NW consecutive key tiles
//                          of one (b h) and share the 32-query Q / dO tiles (and their lse / delta) in LDS;
//   k_attention_bwd_dq     a wave owns 32 queries and walks the key tiles, like the forward; the workgroup shares K / V in LDS.
// Every gradient element is accumulated by ONE lane in a fixed order (dK and dV: a sum per query tile, added tile after tile) and
// stored once: no atomics, and the result is bit for bit the same from run to run.
//
// Layouts: q, dq [(b h)][n][d]; k, v, dk, dv [(b h)][n_k][d]; out, d_out [(b)][n][(h d)]; lse, delta [(b h)][n].
//
// MFMA arrangement (v_mfma_f32_32x32x2_f32; accumulator register r of lane half hi is row at_row(r, hi) of cs_attention_tile.h, the
// lane's low five bits the column; a k-ordered fmaf chain, so s(i, j) is bit for bit the forward's):
//   dq kernel    S^T = K . Q^T and dP^T = V . dO^T: the QUERY on the lane, lse and delta per-lane scalars; Q and dO fragments in
//                registers, K and V rows read from LDS with one ds_read_b128 per group of four k-steps; then
//                dQ^T += K^T . dS^T with the dS^T accumulator registers as B fragments (k-step r = key pair {a_r, a_r + 4}).
//   dk/dv kernel S = Q . K^T and dP = dO . V^T: the KEY on the lane, K and V fragments in registers, Q and dO rows from LDS; lse
//                and delta of the register's query row from LDS (broadcast reads); then dV^T += dO^T . P and dK^T += Q^T . dS
//                with the P / dS registers as B fragments (k-step r = query pair {a_r, a_r + 4}).
// All LDS tiles have rows of ND * 32 + 4 floats ((stride / 4) odd: the ds_read_b128 of 8 consecutive rows fall on distinct bank
// quads; the column reads of the second products take 32 consecutive floats per lane half).
//
// Partial tiles.  Keys past n_k: in the dq kernel P = 0 as in the forward (the score is -inf before the exponential) and the V / K
// rows are zero, so dS = 0 * finite = 0; in the dk/dv kernel such a key is a column nobody stores.  Queries past n: Q and dO rows are
// zeros and lse = +inf, so P = exp2(0 - inf) = 0 and dS = 0 * (0 - 0) = 0: they add exact zeros to dK and dV; in the dq kernel such
// a query is a column nobody stores (lse read as 0: finite arithmetic).
#include "cs_attention_tile.h"
#include "cs_common.h"
#include "cs_kernels.h"

namespace cs {

// delta [(b h)][n]: one thread per row.  The chain is the one the MFMAs run for dP(i, j) = dO(i, :) . V(j, :) -- k-step 4 g + t
// takes column 8 g + t, then column 8 g + 4 + t, each one fmaf -- so that where O(i, :) equals V(j, :) bit for bit (a single key:
// softmax = 1) delta(i) equals dP(i, j) bit for bit and dS is exactly zero.
__global__ void __launch_bounds__(256) k_attention_delta(const float* __restrict__ out, const float* __restrict__ d_out,
                                                         float* __restrict__ delta, int H, int n, int d, size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const size_t bh = idx / (size_t)n, i = idx - bh * n;
    const size_t off = ((bh / H) * n + i) * ((size_t)H * d) + (bh % H) * (size_t)d;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float acc = 0.0f;
    for (int c = 0; c < d; c += 8) {
        const bool two = c + 4 < d;
        const float4 a0 = *(const float4*)(d_out + off + c), b0 = *(const float4*)(out + off + c);
        const float4 a1 = two ? *(const float4*)(d_out + off + c + 4) : zero, b1 = two ? *(const float4*)(out + off + c + 4) : zero;
        acc = fmaf(a1.x, b1.x, fmaf(a0.x, b0.x, acc));
        acc = fmaf(a1.y, b1.y, fmaf(a0.y, b0.y, acc));
        acc = fmaf(a1.z, b1.z, fmaf(a0.z, b0.z, acc));
        acc = fmaf(a1.w, b1.w, fmaf(a0.w, b0.w, acc));
    }
    delta[idx] = acc;
}

template <int ND, int NW>
__global__ void __launch_bounds__(NW * 64) k_attention_bwd_dq(const float* __restrict__ q, const float* __restrict__ k,
                                                              const float* __restrict__ v, const float* __restrict__ d_out,
                                                              const float* __restrict__ lse, const float* __restrict__ delta,
                                                              float* __restrict__ dq, int H, int n, int n_k, int d, float scale,
                                                              int qtiles) {
    constexpr int SK = ND * 32 + 4, NT = NW * 64;
    __shared__ __attribute__((aligned(16))) float Ks[AT_T * SK];
    __shared__ __attribute__((aligned(16))) float Vs[AT_T * SK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hi = lane >> 5;
    const int bh = blockIdx.x / qtiles, qt = blockIdx.x - bh * qtiles;
    const float* kb = k + (size_t)bh * n_k * d;
    const float* vb = v + (size_t)bh * n_k * d;
    const int d4 = d >> 2;

    // the pad columns (d .. SK) meet zero Q / dO fragments, or end in dQ columns nobody stores: they must be finite
    for (int i = tid; i < AT_T * SK; i += NT) { Ks[i] = 0.0f; Vs[i] = 0.0f; }

    // Q and dO fragments of query `col`: d = 8 g + 4 hi .. + 3 in qf[g] / dof[g]; zero past d and past n
    const int qi = (qt * NW + wave) * 32 + col;
    const bool q_ok = qi < n;
    const int qs = q_ok ? qi : 0;
    const float* qrow = q + ((size_t)bh * n + qs) * d;
    const float* drow = d_out + ((size_t)(bh / H) * n + qs) * ((size_t)H * d) + (size_t)(bh % H) * d;
    float4 qf[ND * 4], dof[ND * 4];
#pragma unroll
    for (int g = 0; g < ND * 4; g++) {
        const int c0 = 8 * g + 4 * hi;
        const bool ok = q_ok && c0 < d;
        qf[g] = ok ? *(const float4*)(qrow + c0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        dof[g] = ok ? *(const float4*)(drow + c0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const float lse_i = q_ok ? lse[(size_t)bh * n + qi] : 0.0f;
    const float delta_i = q_ok ? delta[(size_t)bh * n + qi] : 0.0f;

    at_acc acc[ND];
#pragma unroll
    for (int b = 0; b < ND; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[b][r] = 0.0f;
    const float sc2 = scale * 1.44269504088896340736f;

    const int ntiles = (n_k + AT_T - 1) / AT_T;
    for (int kt = 0; kt < ntiles; kt++) {
        __syncthreads();   // the previous tile's readers (first pass: the zero fill) are done
        for (int e = tid; e < AT_T * d4; e += NT) {
            const int row = e / d4, c4 = e - row * d4;
            const int j = kt * AT_T + row;
            float4 kv = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vv = kv;
            if (j < n_k) {
                const size_t off = (size_t)j * d + 4 * c4;
                kv = *(const float4*)(kb + off);
                vv = *(const float4*)(vb + off);
            }
            *(float4*)(Ks + row * SK + 4 * c4) = kv;
            *(float4*)(Vs + row * SK + 4 * c4) = vv;
        }
        __syncthreads();

        // S^T = K . Q^T, dP^T = V . dO^T
        at_acc st, dp;
#pragma unroll
        for (int r = 0; r < 16; r++) { st[r] = 0.0f; dp[r] = 0.0f; }
#pragma unroll
        for (int g = 0; g < ND * 4; g++) {
            if (8 * g < d) {
                const float4 kf = *(const float4*)(Ks + col * SK + 8 * g + 4 * hi);
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[g].x, st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[g].y, st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[g].z, st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[g].w, st, 0, 0, 0);
                const float4 vf = *(const float4*)(Vs + col * SK + 8 * g + 4 * hi);
                dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.x, dof[g].x, dp, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.y, dof[g].y, dp, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.z, dof[g].z, dp, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.w, dof[g].w, dp, 0, 0, 0);
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
        for (int b = 0; b < ND; b++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float kf = Ks[at_row(r, hi) * SK + b * 32 + col];
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf, st[r], acc[b], 0, 0, 0);
            }
        }
    }

    if (!q_ok) return;
    // lane (query, hi) holds columns 32 blk + 8 g + 4 hi .. + 3 in registers 4 g .. 4 g + 3
    float* orow = dq + ((size_t)bh * n + qi) * d;
#pragma unroll
    for (int b = 0; b < ND; b++) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int c0 = b * 32 + 8 * g + 4 * hi;
            if (c0 < d)
                *(float4*)(orow + c0) = make_float4(acc[b][4 * g] * scale, acc[b][4 * g + 1] * scale, acc[b][4 * g + 2] * scale,
                                                    acc[b][4 * g + 3] * scale);
        }
    }
}

// PART: 0 = dk and dv; 1 = dv only (no V fragment, no dP); 2 = dk only.  At ND = 5 the K and V fragments (160 registers), both
// accumulators (160) and the two score tiles do not fit 512 registers: the launcher runs parts 1 and 2 one after the other, at the
// price of a second S product (5 matrix products per tile pair instead of 4).
template <int ND, int NW, int PART>
__global__ void __launch_bounds__(NW * 64) k_attention_bwd_dkdv(const float* __restrict__ q, const float* __restrict__ k,
                                                                const float* __restrict__ v, const float* __restrict__ d_out,
                                                                const float* __restrict__ lse, const float* __restrict__ delta,
                                                                float* __restrict__ dk, float* __restrict__ dv, int H, int n,
                                                                int n_k, int d, float scale, int kgroups) {
    constexpr int SK = ND * 32 + 4, NT = NW * 64;
    constexpr bool DK = PART != 1, DV = PART != 2;
    __shared__ __attribute__((aligned(16))) float Qs[AT_T * SK];
    __shared__ __attribute__((aligned(16))) float Ds[AT_T * SK];
    __shared__ __attribute__((aligned(16))) float Ls[AT_T];
    __shared__ __attribute__((aligned(16))) float Dl[AT_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hi = lane >> 5;
    const int bh = blockIdx.x / kgroups, kg = blockIdx.x - bh * kgroups;
    const float* qb = q + (size_t)bh * n * d;
    const float* db = d_out + (size_t)(bh / H) * n * ((size_t)H * d) + (size_t)(bh % H) * d;
    const size_t dstride = (size_t)H * d;
    const int d4 = d >> 2;

    for (int i = tid; i < AT_T * SK; i += NT) { Qs[i] = 0.0f; Ds[i] = 0.0f; }

    // K and V fragments of key `col` of this wave's tile: d = 8 g + 4 hi .. + 3 in kf[g] / vf[g]; zero past d and past n_k
    const int key0 = (kg * NW + wave) * 32;
    const bool wave_on = key0 < n_k;   // (wave-uniform; the barriers below are outside of what it guards)
    const int kj = key0 + col;
    const bool k_ok = kj < n_k;
    const float* krow = k + ((size_t)bh * n_k + (k_ok ? kj : 0)) * d;
    const float* vrow = v + ((size_t)bh * n_k + (k_ok ? kj : 0)) * d;
    float4 kf[ND * 4], vf[ND * 4];
#pragma unroll
    for (int g = 0; g < ND * 4; g++) {
        const int c0 = 8 * g + 4 * hi;
        const bool ok = k_ok && c0 < d;
        kf[g] = ok ? *(const float4*)(krow + c0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        vf[g] = (DK && ok) ? *(const float4*)(vrow + c0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }

    at_acc ak[ND], av[ND];
#pragma unroll
    for (int b = 0; b < ND; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) { ak[b][r] = 0.0f; av[b][r] = 0.0f; }
    const float sc2 = scale * 1.44269504088896340736f;

    const int ntiles = (n + AT_T - 1) / AT_T;
    for (int qt = 0; qt < ntiles; qt++) {
        __syncthreads();   // the previous tile's readers (first pass: the zero fill) are done
        for (int e = tid; e < AT_T * d4; e += NT) {
            const int row = e / d4, c4 = e - row * d4;
            const int i = qt * AT_T + row;
            float4 qv = make_float4(0.0f, 0.0f, 0.0f, 0.0f), dv4 = qv;
            if (i < n) {
                qv = *(const float4*)(qb + (size_t)i * d + 4 * c4);
                dv4 = *(const float4*)(db + (size_t)i * dstride + 4 * c4);
            }
            *(float4*)(Qs + row * SK + 4 * c4) = qv;
            *(float4*)(Ds + row * SK + 4 * c4) = dv4;
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
        for (int g = 0; g < ND * 4; g++) {
            if (8 * g < d) {
                const float4 qa = *(const float4*)(Qs + col * SK + 8 * g + 4 * hi);
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(qa.x, kf[g].x, st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(qa.y, kf[g].y, st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(qa.z, kf[g].z, st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(qa.w, kf[g].w, st, 0, 0, 0);
                if constexpr (DK) {
                    const float4 da = *(const float4*)(Ds + col * SK + 8 * g + 4 * hi);
                    dp = __builtin_amdgcn_mfma_f32_32x32x2f32(da.x, vf[g].x, dp, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x2f32(da.y, vf[g].y, dp, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x2f32(da.z, vf[g].z, dp, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x2f32(da.w, vf[g].w, dp, 0, 0, 0);
                }
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
                if constexpr (DK) dp[r] = p * (dp[r] - ev[t]);
            }
        }
        // dV^T += dO^T . P, dK^T += Q^T . dS.  A tile's product is summed on its own (a chain of 32 queries from zero) and then
        // added to the running total, as tools/attention_grad_oracle.grads_tiled states it: one chain over all n queries lets the
        // rounding error grow with n (a single key, P = 1, n = 161: four times the reference's own float32 error in dV).
#pragma unroll
        for (int b = 0; b < ND; b++) {
            if constexpr (DV) {
                at_acc t;
#pragma unroll
                for (int r = 0; r < 16; r++) t[r] = 0.0f;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const float da = Ds[at_row(r, hi) * SK + b * 32 + col];
                    t = __builtin_amdgcn_mfma_f32_32x32x2f32(da, st[r], t, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; r++) av[b][r] += t[r];
            }
            if constexpr (DK) {
                at_acc t;
#pragma unroll
                for (int r = 0; r < 16; r++) t[r] = 0.0f;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const float qa = Qs[at_row(r, hi) * SK + b * 32 + col];
                    t = __builtin_amdgcn_mfma_f32_32x32x2f32(qa, dp[r], t, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; r++) ak[b][r] += t[r];
            }
        }
    }

    if (!k_ok) return;
    // lane (key, hi) holds columns 32 blk + 8 g + 4 hi .. + 3 in registers 4 g .. 4 g + 3
    float* krow_o = dk + ((size_t)bh * n_k + kj) * d;
    float* vrow_o = dv + ((size_t)bh * n_k + kj) * d;
#pragma unroll
    for (int b = 0; b < ND; b++) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int c0 = b * 32 + 8 * g + 4 * hi;
            if (c0 < d) {
                if constexpr (DK)
                    *(float4*)(krow_o + c0) = make_float4(ak[b][4 * g] * scale, ak[b][4 * g + 1] * scale, ak[b][4 * g + 2] * scale,
                                                          ak[b][4 * g + 3] * scale);
                if constexpr (DV)
                    *(float4*)(vrow_o + c0) = make_float4(av[b][4 * g], av[b][4 * g + 1], av[b][4 * g + 2], av[b][4 * g + 3]);
            }
        }
    }
}

size_t attention_bwd_workspace_bytes(int b, int h, int n, int n_k, int d) {
    (void)n_k; (void)d;
    if (b <= 0 || h <= 0 || n <= 0 || n_k <= 0 || d <= 0) return 0;
    return ((size_t)b * h * n * 4 + 255) & ~(size_t)255;   // delta
}

// workgroup shapes: the forward's (attention_waves, with its development switch); a dk/dv workgroup of NW waves owns NW key tiles
// and a dq workgroup NW query tiles
hipError_t launch_attention_bwd(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* d_out,
                                float* dq, float* dk, float* dv, int b, int h, int n, int n_k, int d, float scale, void* workspace,
                                hipStream_t stream) {
    const long long bhn = (long long)b * h;
    const int nw = attention_waves(bhn, n);
    float* delta = (float*)workspace;
    const size_t rows = (size_t)bhn * n;
    hipLaunchKernelGGL(k_attention_delta, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, out, d_out, delta, h, n, d, rows);
    return at_dispatch(d, nw, [&](auto nd, auto nwc) {
        constexpr int ND = decltype(nd)::value, NW = decltype(nwc)::value;
        const int kgroups = ((n_k + 31) / 32 + NW - 1) / NW, qtiles = (n + 32 * NW - 1) / (32 * NW);
        if constexpr (ND < 5) {
            hipLaunchKernelGGL((k_attention_bwd_dkdv<ND, NW, 0>), dim3((unsigned)(bhn * kgroups)), dim3(NW * 64), 0, stream, q, k, v, d_out,
                               lse, delta, dk, dv, h, n, n_k, d, scale, kgroups);
        } else {   // dv, then dk: see PART
            hipLaunchKernelGGL((k_attention_bwd_dkdv<ND, NW, 1>), dim3((unsigned)(bhn * kgroups)), dim3(NW * 64), 0, stream, q, k, v, d_out,
                               lse, delta, dk, dv, h, n, n_k, d, scale, kgroups);
            hipLaunchKernelGGL((k_attention_bwd_dkdv<ND, NW, 2>), dim3((unsigned)(bhn * kgroups)), dim3(NW * 64), 0, stream, q, k, v, d_out,
                               lse, delta, dk, dv, h, n, n_k, d, scale, kgroups);
        }
        hipLaunchKernelGGL((k_attention_bwd_dq<ND, NW>), dim3((unsigned)(bhn * qtiles)), dim3(NW * 64), 0, stream, q, k, v, d_out, lse,
                           delta, dq, h, n, n_k, d, scale, qtiles);
        return hipGetLastError();
    });
}

}  // namespace cs
