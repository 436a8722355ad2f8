// cs_attention.hip -- the reference's stereo attention (stereo_utils.py BNAttention.attn_batch :119-133, .forward :135-176) as
// one flash-style forward kernel: float32 in, float32 out, float32 accumulation on v_mfma_f32_32x32x2_f32, whose result is
// bit for bit a k-ordered fmaf chain.  No score matrix, no workspace: softmax is computed online per key tile.
//
// The reference's rearranges are index maps and are applied in the addressing:
//   q   [(c s b h)][n][d]      k, v [(c s b h)][n_k][d]      out [(c s b)][n][(h d)]
//   CS_ATTN_SELF  query (c,s,b,h,i) sees keys (c,s,b,h,0..n_k-1)                      (:137-140, the plain path)
//   CS_ATTN_UNI   ... sees keys (c,0,b,h,0..n-1)                                      (:163-171, ku[:_num_heads])
//   CS_ATTN_BI    ... sees keys (c,0,b,h,0..n-1) followed by (c,1,b,h,0..n-1)          (:156-162, and :142-146 with c = 1)
//
// One wave owns 32 queries; a workgroup of NW waves shares the 32-key K / V tiles in LDS.  Per tile a wave computes
//   S^T = K . Q^T   A = K (row: key, k: d), B = Q^T: the accumulator has the QUERY on the lane (column l & 31) and 16 keys in
//                   its registers (row at_row(r, l >> 5), cs_attention_tile.h), so the softmax row reductions are in-lane plus
//                   one exchange with lane l ^ 32, and the rescale factor of a query is a per-lane scalar;
//   O^T += V^T . P^T  register r of the S^T accumulator IS the B fragment of a k-step over the key pair
//                   {a_r, a_r + 4}, a_r = (r & 3) + 8 (r >> 2): P never leaves the registers.  The A fragment is
//                   V[key a_r + 4 (l >> 5)][32 blk + (l & 31)], one conflict-free ds_read_b32.
// The d-order inside the first product is free as long as both operands agree: k-step 4 g + j takes d = 8 g + 4 (l >> 5) + j,
// so that a lane reads its four K operands of a group with one ds_read_b128 and keeps Q as float4s.  Rows of K are
// ND * 32 + 4 floats apart: (stride / 4) is odd, the 16-byte slots of 8 consecutive keys fall on distinct bank quads.
#include "cs_attention_tile.h"
#include "cs_common.h"
#include "cs_kernels.h"

namespace cs {

enum { SA_MAX_D = 160 };   // largest head dimension (5 blocks of 32 output columns)

int stereo_attention_max_head_dim() { return SA_MAX_D; }

// LSE (cs_attention_fwd_lse, the forward of the differentiable attention): besides `out`, the log-sum-exp of every query's scaled
// scores goes to lse [(c s b h)][n], in log2 units like sc2: p(i, j) = exp2(sc2 * s(i, j) - lse(i)).  Nothing else differs.
template <int ND, int NW, bool LSE = false>
__global__ void __launch_bounds__(NW * 64) k_stereo_attention(const float* __restrict__ q, const float* __restrict__ k,
                                                              const float* __restrict__ v, float* __restrict__ out, int S, int B,
                                                              int H, int n, int n_k, int d, float scale, int mode, int qtiles,
                                                              float* __restrict__ lse = nullptr) {
    constexpr int SK = ND * 32 + 4, SV = ND * 32, NT = NW * 64;
    __shared__ __attribute__((aligned(16))) float Ks[AT_T * SK];
    __shared__ __attribute__((aligned(16))) float Vs[AT_T * SV];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hi = lane >> 5;
    const int bh = blockIdx.x / qtiles, qt = blockIdx.x - bh * qtiles;
    // (c s b h) -> the key set: view 0 of the same (c, b, h) for UNI / BI, followed by view 1 for BI
    const int hh = bh % H, sb = bh / H, s = (sb / B) % S;
    const size_t kset = mode == CS_ATTN_SELF ? (size_t)bh : (size_t)bh - (size_t)s * B * H;
    const int nkeys = mode == CS_ATTN_BI ? 2 * n_k : n_k;
    const size_t view_rows = (size_t)(B * H - 1) * n_k;   // BI: rows between the end of view 0's keys and the start of view 1's
    const float* kb = k + kset * n_k * d;
    const float* vb = v + kset * n_k * d;
    const int d4 = d >> 2;

    // the pad columns (d .. SK) are multiplied by Q's zero pad, rows past the key set by p = 0: both must be finite
    for (int i = tid; i < AT_T * SK; i += NT) Ks[i] = 0.0f;
    for (int i = tid; i < AT_T * SV; i += NT) Vs[i] = 0.0f;

    // Q fragment: query `col` of this wave, d = 8 g + 4 hi .. + 3 in qf[g]; zero past d and past n
    const int qi = (qt * NW + wave) * 32 + col;
    const bool q_ok = qi < n;
    const float* qrow = q + ((size_t)bh * n + (q_ok ? qi : 0)) * d;
    float4 qf[ND * 4];
#pragma unroll
    for (int g = 0; g < ND * 4; g++) {
        const int c0 = 8 * g + 4 * hi;
        qf[g] = (q_ok && c0 < d) ? *(const float4*)(qrow + c0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }

    at_acc o[ND];
#pragma unroll
    for (int b = 0; b < ND; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[b][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;
    const float sc2 = scale * 1.44269504088896340736f;   // scores in units of log2: p = exp2(s - m)

    const int ntiles = (nkeys + AT_T - 1) / AT_T;
    for (int kt = 0; kt < ntiles; kt++) {
        __syncthreads();   // the previous tile's readers (first pass: the zero fill) are done
        for (int e = tid; e < AT_T * d4; e += NT) {
            const int row = e / d4, c4 = e - row * d4;
            const int j = kt * AT_T + row;
            float4 kv = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vv = kv;
            if (j < nkeys) {
                const size_t off = ((size_t)j + (j >= n_k ? view_rows : 0)) * d + 4 * c4;
                kv = *(const float4*)(kb + off);
                vv = *(const float4*)(vb + off);
            }
            *(float4*)(Ks + row * SK + 4 * c4) = kv;
            *(float4*)(Vs + row * SV + 4 * c4) = vv;
        }
        __syncthreads();

        // S^T = K . Q^T
        at_acc st;
#pragma unroll
        for (int r = 0; r < 16; r++) st[r] = 0.0f;
#pragma unroll
        for (int g = 0; g < ND * 4; g++) {
            if (8 * g < d) {
                const float4 kf = *(const float4*)(Ks + col * SK + 8 * g + 4 * hi);
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[g].x, st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[g].y, st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[g].z, st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[g].w, st, 0, 0, 0);
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
        for (int b = 0; b < ND; b++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float vf = Vs[at_row(r, hi) * SV + b * 32 + col];
                o[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf, st[r], o[b], 0, 0, 0);
            }
        }
    }

    const float l_all = l_run + __shfl_xor(l_run, 32);
    if (!q_ok) return;
    if (LSE && hi == 0) lse[(size_t)bh * n + qi] = m_run + __builtin_amdgcn_logf(l_all);   // (v_log_f32 is log2; l_all >= 1)
    // out [(c s b)][n][(h d)]: lane (query, hi) holds columns 32 blk + 8 g + 4 hi .. + 3 in registers 4 g .. 4 g + 3
    float* orow = out + ((size_t)sb * n + qi) * ((size_t)H * d) + (size_t)hh * d;
#pragma unroll
    for (int b = 0; b < ND; b++) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int c0 = b * 32 + 8 * g + 4 * hi;
            if (c0 < d)
                *(float4*)(orow + c0) = make_float4(o[b][4 * g] / l_all, o[b][4 * g + 1] / l_all, o[b][4 * g + 2] / l_all,
                                                    o[b][4 * g + 3] / l_all);
        }
    }
}

// Waves per workgroup of every attention kernel, by measurement of the float32 forward on the four SD 1.5 levels
// (tools/attention_bench.py --sweep): 4 everywhere.  A wave's share of the cooperative K / V tile load, not its
// MFMAs, bounds the tile loop, so four waves per tile win even where they leave CUs idle (n = 256: 64 workgroups) or have no query
// of their own (n = 64).  The half kernels and the backwards keep that 4 until tools/attention_bench.py --dtype ... --sweep says
// otherwise; 1 and 2 stay selectable for sweeps with CS_DEBUG_ATTN_WAVES.
int attention_waves(long long batch_heads, int n) {
    (void)batch_heads; (void)n;
    const int forced = dev_switch(CS_DEBUG_ATTN_WAVES);
    return (forced == 1 || forced == 2) ? forced : 4;
}

template <bool LSE>
static hipError_t sa_launch(const float* q, const float* k, const float* v, float* out, float* lse, int c, int s, int b, int h, int n,
                            int n_k, int d, float scale, int mode, hipStream_t stream) {
    const long long bhn = (long long)c * s * b * h;
    const int nw = attention_waves(bhn, n);
    const int qtiles = (n + 32 * nw - 1) / (32 * nw);
    const int blocks = (int)(bhn * qtiles);
    return at_dispatch(d, nw, [&](auto nd, auto nwc) {
        constexpr int ND = decltype(nd)::value, NW = decltype(nwc)::value;
        hipLaunchKernelGGL((k_stereo_attention<ND, NW, LSE>), dim3(blocks), dim3(NW * 64), 0, stream, q, k, v, out, s, b, h, n, n_k, d,
                           scale, mode, qtiles, lse);
        return hipGetLastError();
    });
}

hipError_t launch_stereo_attention(const float* q, const float* k, const float* v, float* out, int c, int s, int b, int h, int n,
                                   int n_k, int d, float scale, int mode, hipStream_t stream) {
    return sa_launch<false>(q, k, v, out, nullptr, c, s, b, h, n, n_k, d, scale, mode, stream);
}

// the same launch as launch_stereo_attention(..., CS_ATTN_SELF) with c = s = 1: `out` is bit for bit that call's
hipError_t launch_attention_fwd_lse(const float* q, const float* k, const float* v, float* out, float* lse, int b, int h, int n, int n_k,
                                    int d, float scale, hipStream_t stream) {
    return sa_launch<true>(q, k, v, out, lse, 1, 1, b, h, n, n_k, d, scale, CS_ATTN_SELF, stream);
}

}  // namespace cs
