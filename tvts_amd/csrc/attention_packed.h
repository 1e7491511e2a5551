// Causal self-attention over PACKED variable-length sequences, forward-only, head dim 64 (included by attention.hip).
//
// The SSv2 multiple-choice scripts push C x B ragged captions through the CLIP text tower (v2/downstream/
// zero_ssv2_mc_TVTSv2_ViT_B_16.py:60-88, "174 x B x 77"); rows behind a caption's EOT token cannot reach the row the model reads
// (causal mask, v2/CLIP/clip/model.py:330-336), so the packed encoder keeps M = sum L_i token rows instead of N * max L_i.
// Sequence i owns rows seq_start[i] .. seq_start[i + 1] - 1 of qkv [M, 3 * heads * 64] and out [M, heads * 64].
//
// Ownership and data flow are those of attn_fwd_seq_fused_kernel: a WAVE owns a (sequence, head) group, scores stay in registers,
// one-pass softmax, V in a wave-private LDS tile, the next group's rows in flight.  The kernel is templated on the number of 16-row
// tiles MT (1, 2, 3, 5: lengths 1-16, 17-32, 33-48, 49-80) and launched once per tile class that max_len admits; a wave skips the
// groups of another class (two cached int loads), so any order of lengths is correct and a length-sorted order (what the encoder
// packs) keeps the waves of a block on neighbouring rows.  Key tiles above the diagonal are never multiplied (causal).
// The cost of that choice: every launch is sized from all N * heads groups and each of its waves walks its whole stride, reading
// seq_start for groups of other classes -- in a sorted batch most waves of a class with few members only scan and exit.  One launch per
// contiguous range of one class would avoid the scan but needs the class boundaries on the host (the descriptor lives on the device).
// A group is also skipped when its descriptor is out of range (rows outside [0, M), length < 1 or > 80): nothing is read or written
// for it, so a malformed seq_start cannot leave the buffers.
#pragma once

namespace NS_DH {

__device__ __forceinline__ int packed_tile_class(int m) {
    const int t = (m + 15) >> 4;
    return t <= 3 ? t : (t <= 5 ? 5 : 0);
}

template <int MT>
__global__ __launch_bounds__(256) void attn_fwd_packed_kernel(const bf16* __restrict__ qkv, int ld, const int* __restrict__ seq_start,
                                                              int N, int M, int heads, float scale2, bf16* __restrict__ out, int ldo) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // per wave: V tile | output-staging patch
    constexpr int RA = MT * 16, TB = RA * VSTRIDE, NU = (MT + 1) / 2;
    constexpr int WB = TB + 1024;
    constexpr int PT = (RA * NCH + 63) / 64;
    constexpr bool PF = MT <= 3;  // the 5-tile form holds 80 registers of q / k fragments: no second set for a prefetch
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char* Vs = smem + wave * WB;
    char* opatch = Vs + TB;
    const int gq = lane >> 4, li = lane & 15;
    const int W = heads * DH, groups = N * heads, stride = gridDim.x * 4;

    // the first group of this wave's walk at or after gid that belongs to this tile class
    auto next = [&](int gid) {
        for (; gid < groups; gid += stride) {
            const int s = gid / heads, s0 = seq_start[s], s1 = seq_start[s + 1];
            if (s0 >= 0 && s1 <= M && s1 > s0 && packed_tile_class(s1 - s0) == MT) break;
        }
        return gid;
    };
    bf16x8 qf[MT][KS], kf[MT][KS], vst[PT];
    int s0n = 0, mn = 1;
    auto issue = [&](int gid) {
        const int s = gid / heads;
        s0n = seq_start[s];
        mn = seq_start[s + 1] - s0n;
        const bf16* base = qkv + (size_t)s0n * ld + (gid % heads) * DH;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int j = t * 16 + li;
            const bf16* rowp = base + (size_t)(j < mn ? j : mn - 1) * ld;
            ld_frags(rowp, gq, qf[t]);
            ld_frags(rowp + W, gq, kf[t]);
        }
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            const int cc = lane + 64 * i, row = cc / NCH, ch = cc % NCH;
            vst[i] = row < mn ? ldg8(base + (size_t)row * ld + 2 * W + ch * 8) : zero8();
        }
    };
    int gid = next(blockIdx.x * 4 + wave);
    if (PF && gid < groups) issue(gid);
    while (gid < groups) {
        if (!PF) issue(gid);
        const int s0 = s0n, m = mn;
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            const int cc = lane + 64 * i, row = cc / NCH, ch = cc % NCH;
            if (row < RA) *(bf16x8*)(Vs + row * VSTRIDE + ch * 16) = vst[i];
        }
        bf16x8 qc[MT][KS], kc[MT][KS];
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) { qc[t][ks] = qf[t][ks]; kc[t][ks] = kf[t][ks]; }
        const int gnext = next(gid + stride);
        if (PF && gnext < groups) issue(gnext);
        const int hcol = (gid % heads) * DH;
#pragma unroll
        for (int qt = 0; qt < MT; ++qt) {
            if (qt * 16 >= m) continue;  // (wave-uniform; only the 5-tile class has a tile without rows)
            const int qj = qt * 16 + li;
            f32x4 st[2 * NU];
            float mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < 2 * NU; ++t) {
                st[t] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                if (t <= qt) {  // causal: key tiles above the diagonal are masked as a whole
                    f32x4 sc = {0, 0, 0, 0};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc[t][ks], qc[qt][ks], sc, 0, 0, 0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int key = t * 16 + gq * 4 + e;
                        const float v = (key < m && key <= qj) ? sc[e] * scale2 : -INFINITY;
                        st[t][e] = v;
                        mx = fmaxf(mx, v);
                    }
                }
            }
            mx = group_max(mx);  // (key 0 is visible to every query: never -inf)
            float rs = 0.f;
#pragma unroll
            for (int t = 0; t < 2 * NU; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pp = t <= qt ? __builtin_amdgcn_exp2f(st[t][e] - mx) : 0.f;
                    st[t][e] = pp;
                    rs += pp;
                }
            const float l = group_sum(rs);
            f32x4 o[DT];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] = (f32x4){0, 0, 0, 0};
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                if (2 * u > qt) continue;
                bf16x8 pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[j] = (bf16)st[2 * u + (j >> 2)][j & 3];
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_T_lim<true>(Vs, u, dt, lane, RA), pf, o[dt], 0, 0, 0);
            }
            const float inv = 1.0f / l;
            f32x4 on[DT];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) on[dt] = o[dt] * inv;
            store_tile_rows(opatch, on, lane, [&](int rr) -> bf16* {
                const int j = qt * 16 + rr;
                return j < m ? out + (size_t)(s0 + j) * ldo + hcol : nullptr; });
        }
        gid = gnext;
    }
}

// ONE query per sequence, at its LAST row (the EOT token of a packed caption: the only row the last text block's output is read at,
// v2/CLIP/clip/model.py:343-354), over all keys of the sequence.  A wave per (sequence, head): lanes over the keys for the scores
// (fp32 dot products, up to two keys per lane), lanes over the 64 head columns for P V; probabilities stay fp32.  Writes that row only.
__global__ __launch_bounds__(256) void attn_fwd_packed_last_kernel(const bf16* __restrict__ qkv, int ld, const int* __restrict__ seq_start,
                                                                   int N, int M, int heads, float scale2, bf16* __restrict__ out, int ldo) {
    const int lane = threadIdx.x & 63;
    const int gid = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gid >= N * heads) return;
    const int s = gid / heads, h = gid % heads, W = heads * DH;
    const int s0 = seq_start[s], s1 = seq_start[s + 1], m = s1 - s0;
    if (s0 < 0 || s1 > M || m < 1 || m > 80) return;  // the bound of the full form and of the header
    const bf16* base = qkv + (size_t)s0 * ld + h * DH;
    bf16x8 q[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) q[c] = ldg8(base + (size_t)(m - 1) * ld + c * 8);
    float sc[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int j = lane + 64 * kk;
        float dot = 0.f;
        if (j < m) {
            const bf16* kr = base + (size_t)j * ld + W;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const bf16x8 kv = ldg8(kr + c * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) dot = __builtin_fmaf((float)q[c][e], (float)kv[e], dot);
            }
        }
        sc[kk] = j < m ? dot * scale2 : -INFINITY;
    }
    const float mx = wave_max(fmaxf(sc[0], sc[1]));
    const float p0 = __builtin_amdgcn_exp2f(sc[0] - mx), p1 = __builtin_amdgcn_exp2f(sc[1] - mx);
    const float l = wave_sum(p0 + p1);
    float o = 0.f;
    const bf16* vcol = base + 2 * W + lane;
    for (int j = 0; j < m; ++j) {
        const float p = __shfl(j < 64 ? p0 : p1, j & 63, 64);
        o = __builtin_fmaf(p, (float)vcol[(size_t)j * ld], o);
    }
    out[(size_t)(s1 - 1) * ldo + h * DH + lane] = (bf16)(o / l);
}

}  // namespace NS_DH

static int packed_args_ok(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, const void* out, int ldo) {
    if (!qkv || !seq_start || !out || N <= 0 || M <= 0 || heads <= 0 || ld % 8 || ldo % 8) return TVTS_EINVAL;
    if (ld < 3 * heads * DH || ldo < heads * DH || max_len < 1 || max_len > 80) return TVTS_EINVAL;
    return TVTS_OK;
}

extern "C" int tvts_attn_fwd_packed(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, void* out,
                                    int ldo, hipStream_t stream) {
    const int rc = packed_args_ok(qkv, ld, seq_start, N, M, heads, max_len, out, ldo);
    if (rc) return rc;
    const float scale2 = 1.4426950408889634f / sqrtf((float)DH);
    const int groups = N * heads;
    const int blocks = ceil_div(groups, 4) < 1536 ? ceil_div(groups, 4) : 1536;
#define PACKED_LAUNCH(MT)                                                                                                      \
    hipLaunchKernelGGL((attn_fwd_packed_kernel<MT>), dim3(blocks), dim3(256), 4 * (MT * 16 * VSTRIDE + 1024), stream,           \
                       (const bf16*)qkv, ld, seq_start, N, M, heads, scale2, (bf16*)out, ldo)
    PACKED_LAUNCH(1);
    if (max_len > 16) PACKED_LAUNCH(2);
    if (max_len > 32) PACKED_LAUNCH(3);
    if (max_len > 48) PACKED_LAUNCH(5);
#undef PACKED_LAUNCH
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

extern "C" int tvts_attn_fwd_packed_last(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len,
                                         void* out, int ldo, hipStream_t stream) {
    const int rc = packed_args_ok(qkv, ld, seq_start, N, M, heads, max_len, out, ldo);
    if (rc) return rc;
    const float scale2 = 1.4426950408889634f / sqrtf((float)DH);
    hipLaunchKernelGGL(attn_fwd_packed_last_kernel, dim3(ceil_div(N * heads, 4)), dim3(256), 0, stream, (const bf16*)qkv, ld,
                       seq_start, N, M, heads, scale2, (bf16*)out, ldo);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
