// Causal self-attention over PACKED variable-length sequences, forward and backward, head dim 64 (included by attention.hip).
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
//
// Training (the packed text tower of the step): the _lse entries are the same kernels and also store the log2-domain
// log-sum-exp per (packed row, head), lse2[row * heads + h], the layout of the FULL kernels for a [rows = M, heads] problem.
// attn_bwd_packed_kernel keeps the forward's ownership -- a wave per (sequence, head) group, the same tile classes, the same guard --
// so one wave writes a group's rows of all three thirds of dqkv: no atomics, no cross-wave reduction, run-to-run the same bits.
//
// BIDIRECTIONAL forms (the DistilBERT tower of v1 over packed captions, arch["text_unpadded"], DESIGN.md 8b "v1"): the same kernels
// under the template parameters BIDIR / DROP, which default to the causal behaviour above (the causal instantiations are unchanged):
// every key tile of the sequence is multiplied, only the keys at or behind the sequence end are masked, and the probabilities carry
// the dropout mask of the padded kernels (PackedDrop).  tvts_attn_fwd_packed_bidir, tvts_attn_bwd_packed_bidir, tvts_attn_fwd_packed_first.
#pragma once

namespace NS_DH {

__device__ __forceinline__ int packed_tile_class(int m) {
    const int t = (m + 15) >> 4;
    return t <= 3 ? t : (t <= 5 ? 5 : 0);
}

// dropout on the probabilities of the BIDIRECTIONAL forms (the DistilBERT tower of v1 over packed captions): probability (sequence
// i, head h, query q, key k) has the index ((i * heads + h) * L_pad + q) * L_pad + k of the padded kernels (attn_fwd_shared_kernel's
// DROP branch with S = L_pad), so a packed call draws the masks of tvts_attn_fwd_len_drop on the same (seed, site)
struct PackedDrop { unsigned thr; float inv; const unsigned long long* seed; unsigned long long site; int L_pad; };

// BIDIR: every key tile of the sequence is multiplied and only the keys at or behind the sequence end are masked (no causal mask);
// DROP (BIDIR only): softmax first, dropout second -- the row sum is of the undropped probabilities, and P o m / (1 - p) is rounded to
// bf16 for the MFMA: the arithmetic of attn_fwd_shared_kernel's DROP branch, operation for operation (a sequence of up to 64 rows is
// ONE key tile there, so the packed call gives that kernel's bits)
template <int MT, bool LSE = false, bool BIDIR = false, bool DROP = false>
__global__ __launch_bounds__(256) void attn_fwd_packed_kernel(const bf16* __restrict__ qkv, int ld, const int* __restrict__ seq_start,
                                                              int N, int M, int heads, float scale2, bf16* __restrict__ out, int ldo,
                                                              float* __restrict__ lse2, PackedDrop dr) {
    static_assert(BIDIR || !DROP, "dropout exists for the bidirectional form only");
    extern __shared__ __attribute__((aligned(16))) char smem[];  // per wave: V tile | output-staging patch
    const unsigned long long dseed = DROP ? dr.seed[0] + dr.site : 0ull;
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
                if (BIDIR ? t < MT : t <= qt) {  // causal: key tiles above the diagonal are masked as a whole
                    f32x4 sc = {0, 0, 0, 0};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kc[t][ks], qc[qt][ks], sc, 0, 0, 0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int key = t * 16 + gq * 4 + e;
                        const float v = (key < m && (BIDIR || key <= qj)) ? sc[e] * scale2 : -INFINITY;
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
                    const float pp = (BIDIR ? t < MT : t <= qt) ? __builtin_amdgcn_exp2f(st[t][e] - mx) : 0.f;
                    st[t][e] = pp;
                    rs += pp;
                }
            const float l = group_sum(rs);
            f32x4 o[DT];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] = (f32x4){0, 0, 0, 0};
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                if (!BIDIR && 2 * u > qt) continue;
                bf16x8 pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float pv = st[2 * u + (j >> 2)][j & 3];
                    if (DROP) {
                        const int key = (2 * u + (j >> 2)) * 16 + gq * 4 + (j & 3);
                        const unsigned long long idx = ((unsigned long long)gid * dr.L_pad + qj) * dr.L_pad + key;  // gid = i * heads + h
                        pv = drop_keep(dseed, idx, dr.thr) ? pv * dr.inv : 0.f;
                    }
                    pf[j] = (bf16)pv;
                }
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
            if (LSE && qj < m && gq == 0) lse2[(size_t)(s0 + qj) * heads + gid % heads] = mx + log2f(l);
        }
        gid = gnext;
    }
}

// ONE query per sequence, at its LAST row (the EOT token of a packed caption: the only row the last text block's output is read at,
// v2/CLIP/clip/model.py:343-354), over all keys of the sequence.  A wave per (sequence, head): lanes over the keys for the scores
// (fp32 dot products, up to two keys per lane), lanes over the 64 head columns for P V; probabilities stay fp32.  Writes that row only.
// FIRST: the query sits at the sequence's FIRST row instead ([CLS] of a packed DistilBERT caption, v1/model/model_dist_TVTS.py:131-141)
// and row seq_start[i] is the one written; every key of the sequence is visible to it either way.
template <bool FIRST = false>
__global__ __launch_bounds__(256) void attn_fwd_packed_last_kernel(const bf16* __restrict__ qkv, int ld, const int* __restrict__ seq_start,
                                                                   int N, int M, int heads, float scale2, bf16* __restrict__ out, int ldo,
                                                                   float* __restrict__ lse2) {
    const int lane = threadIdx.x & 63;
    const int gid = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gid >= N * heads) return;
    const int s = gid / heads, h = gid % heads, W = heads * DH;
    const int s0 = seq_start[s], s1 = seq_start[s + 1], m = s1 - s0;
    if (s0 < 0 || s1 > M || m < 1 || m > 80) return;  // the bound of the full form and of the header
    const bf16* base = qkv + (size_t)s0 * ld + h * DH;
    bf16x8 q[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) q[c] = ldg8(base + (size_t)(FIRST ? 0 : m - 1) * ld + c * 8);
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
    const size_t qrow = (size_t)(FIRST ? s0 : s1 - 1);
    out[qrow * ldo + h * DH + lane] = (bf16)(o / l);
    if (lse2 && lane == 0) lse2[qrow * heads + h] = mx + log2f(l);
}

// ---- backward of attn_fwd_packed_kernel: delta = rowsum(dO o O), then P = exp2(s * scale2 - lse2) from the stored log-sum-exp,
// dS = P o (dP - delta), dQ = scale dS K (phase A), dK = scale dS^T Q and dV = P^T dO (phase B).  The data flow is
// attn_bwd_seq_fused_kernel's: the group's Q | K | V | dO rows are staged once into wave-private row-major LDS tiles; the k-contiguous
// operands (the score and dP products) are 16-byte row reads, the transposed ones (K^T, Q^T, dO^T under dS and P) ds_read_tr16_b64 of
// the same tiles (VSTRIDE 160 keeps both conflict-free).  Key tiles above the diagonal are never multiplied: phase A stops at the
// query tile, phase B starts at the key tile.  Rows m .. RA - 1 of the tiles are zeros, so neither stale LDS nor a neighbouring
// sequence's rows can reach a product.  The 1 / 2 / 3-tile classes run two waves a block with the next group's rows in flight in
// registers; the 5-tile class holds 52 KiB of tiles a wave -- one wave a block, three blocks a CU, no prefetch (its registers go to
// the six score tiles of a query tile).
// BIDIR / DROP as in the forward: phase A and phase B run over ALL tiles of the sequence, and the forward's mask m is regenerated from
// (seed, site) -- dropped probabilities P o m / (1 - p) under dV, dS = P o (m / (1 - p) o dP - delta) under dQ and dK.
template <int MT, bool BIDIR = false, bool DROP = false>
__global__ __launch_bounds__(MT <= 3 ? 128 : 64) void attn_bwd_packed_kernel(
    const bf16* __restrict__ qkv, int ld, const int* __restrict__ seq_start, int N, int M, int heads, float scale2, float scale,
    const bf16* __restrict__ dO, int lddo, const bf16* __restrict__ O, int ldo, const float* __restrict__ lse2,
    float* __restrict__ delta, bf16* __restrict__ dqkv, int lddq, PackedDrop dr) {
    static_assert(BIDIR || !DROP, "dropout exists for the bidirectional form only");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned long long dseed = DROP ? dr.seed[0] + dr.site : 0ull;
    constexpr int WV = MT <= 3 ? 2 : 1;
    constexpr int RA = MT * 16, TB = RA * VSTRIDE, NU = (MT + 1) / 2;
    constexpr int WB = 4 * TB + 2 * RA * 4 + 1024;  // one wave's region: Q | K | V | dO tiles, lse and delta of the rows, output patch
    constexpr int PT = RA * NCH / 64;
    constexpr bool PF = MT <= 3;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char* base = smem + wave * WB;
    char* Qs = base;
    char* Ks = Qs + TB;
    char* Vs = Ks + TB;
    char* Ds = Vs + TB;
    float* st_lse = (float*)(Ds + TB);
    float* st_dl = st_lse + RA;
    char* opatch = (char*)(st_dl + RA);
    const int gq = lane >> 4, li = lane & 15;
    const int W = heads * DH, groups = N * heads, stride = gridDim.x * WV;

    auto next = [&](int gid) {
        for (; gid < groups; gid += stride) {
            const int s = gid / heads, s0 = seq_start[s], s1 = seq_start[s + 1];
            if (s0 >= 0 && s1 <= M && s1 > s0 && packed_tile_class(s1 - s0) == MT) break;
        }
        return gid;
    };
    bf16x8 stg[4][PT], ost[PT];
    float lse_pf[2] = {0.f, 0.f};
    int s0n = 0, mn = 1;
    auto issue = [&](int gid) {
        const int s = gid / heads, h = gid % heads;
        s0n = seq_start[s];
        mn = seq_start[s + 1] - s0n;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const bf16* src = (t == 3 ? dO : t == 4 ? O : qkv + t * W) + h * DH;
            const int ldt = t == 3 ? lddo : t == 4 ? ldo : ld;
#pragma unroll
            for (int i = 0; i < PT; ++i) {
                const int cc = lane + 64 * i, row = cc / NCH, ch = cc % NCH;
                bf16x8 v;
                if (PF) v = row < mn ? ldg8(src + (size_t)(s0n + row) * ldt + ch * 8) : zero8();
                else v = sel8(row < mn, ldg8(src + (size_t)(s0n + (row < mn ? row : mn - 1)) * ldt + ch * 8));  // (see sel8)
                if (t == 4) ost[i] = v; else stg[t][i] = v;
            }
        }
#pragma unroll
        for (int k = 0; k < (MT == 5 ? 2 : 1); ++k)
            lse_pf[k] = lane + 64 * k < mn ? lse2[(size_t)(s0n + lane + 64 * k) * heads + h] : 0.f;
    };
    int gid = next(blockIdx.x * WV + wave);
    if (PF && gid < groups) issue(gid);
    while (gid < groups) {
        if (!PF) issue(gid);
        const int s0 = s0n, m = mn, h = gid % heads, hcol = h * DH;
        // registers -> this wave's LDS tiles (rows m .. RA - 1 arrive as zeros); delta of every row on the way
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < PT; ++i) {
                const int cc = lane + 64 * i, row = cc / NCH, ch = cc % NCH;
                *(bf16x8*)(base + t * TB + row * VSTRIDE + ch * 16) = stg[t][i];
            }
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            const int row = (lane + 64 * i) / NCH;
            float p = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) p = __builtin_fmaf((float)stg[3][i][e], (float)ost[i][e], p);
            p += __shfl_xor(p, 1, 64);
            p += __shfl_xor(p, 2, 64);
            p += __shfl_xor(p, 4, 64);
            if ((lane & (NCH - 1)) == 0) {
                st_dl[row] = p;
                if (row < m) delta[(size_t)(s0 + row) * heads + h] = p;
            }
        }
#pragma unroll
        for (int k = 0; k < (MT == 5 ? 2 : 1); ++k)
            if (lane + 64 * k < RA) st_lse[lane + 64 * k] = lse_pf[k];
        const int gnext = next(gid + stride);
        if (PF && gnext < groups) issue(gnext);

        // ---- phase A: dQ of a query tile over the key tiles up to the diagonal
#pragma unroll
        for (int qt = 0; qt < MT; ++qt) {
            if (qt * 16 >= m) continue;  // (wave-uniform; only the 5-tile class has a tile without rows)
            const int qj = qt * 16 + li;
            bf16x8 qf[KS], dof[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) { qf[ks] = frag_row(Qs, qj, ks, gq); dof[ks] = frag_row(Ds, qj, ks, gq); }
            const float lse = st_lse[qj], dlt = st_dl[qj];
            f32x4 dS[2 * NU];
#pragma unroll
            for (int t = 0; t < 2 * NU; ++t) {
                dS[t] = (f32x4){0, 0, 0, 0};
                if (BIDIR ? t < MT : t <= qt) {
                    f32x4 sc = {0, 0, 0, 0}, dp = {0, 0, 0, 0};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_row(Ks, t * 16 + li, ks, gq), qf[ks], sc, 0, 0, 0);
                        dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_row(Vs, t * 16 + li, ks, gq), dof[ks], dp, 0, 0, 0);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int key = t * 16 + gq * 4 + e;
                        const bool ok = key < m && (BIDIR || key <= qj) && qj < m;
                        const float pp = ok ? __builtin_amdgcn_exp2f(sc[e] * scale2 - lse) : 0.f;
                        float dpe = dp[e];
                        if (DROP) {
                            const unsigned long long idx = ((unsigned long long)gid * dr.L_pad + qj) * dr.L_pad + key;
                            dpe = drop_keep(dseed, idx, dr.thr) ? dpe * dr.inv : 0.f;
                        }
                        dS[t][e] = ok ? pp * (dpe - dlt) * scale : 0.f;
                    }
                }
            }
            f32x4 acc[DT];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) acc[dt] = (f32x4){0, 0, 0, 0};
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                if (!BIDIR && 2 * u > qt) continue;
                bf16x8 dsf;
#pragma unroll
                for (int j = 0; j < 8; ++j) dsf[j] = (bf16)dS[2 * u + (j >> 2)][j & 3];
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
                    acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_T_lim<true>(Ks, u, dt, lane, RA), dsf, acc[dt], 0, 0, 0);
            }
            store_tile_rows(opatch, acc, lane, [&](int rr) -> bf16* {
                const int j = qt * 16 + rr;
                return j < m ? dqkv + (size_t)(s0 + j) * lddq + hcol : nullptr; });
        }

        // ---- phase B: dK / dV of a key tile over the query tiles from the diagonal down
#pragma unroll
        for (int kt = 0; kt < MT; ++kt) {
            if (kt * 16 >= m) continue;
            const int kj = kt * 16 + li;
            bf16x8 kb[KS], vb[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) { kb[ks] = frag_row(Ks, kj, ks, gq); vb[ks] = frag_row(Vs, kj, ks, gq); }
            f32x4 dv[DT], dk[DT];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) { dv[dt] = (f32x4){0, 0, 0, 0}; dk[dt] = (f32x4){0, 0, 0, 0}; }
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                if (!BIDIR && 2 * u + 1 < kt) continue;  // both query tiles of this k-step lie above the diagonal
                if (u * 32 >= m) continue;               // ... or behind the last row (wave-uniform)
                bf16x8 pf, dsf;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int tile = 2 * u + t;
                    if (tile < MT && (BIDIR || tile >= kt)) {
                        f32x4 sc = {0, 0, 0, 0}, dp = {0, 0, 0, 0};
#pragma unroll
                        for (int ks = 0; ks < KS; ++ks) {
                            sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_row(Qs, tile * 16 + li, ks, gq), kb[ks], sc, 0, 0, 0);
                            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_row(Ds, tile * 16 + li, ks, gq), vb[ks], dp, 0, 0, 0);
                        }
                        const f32x4 l4 = *(const f32x4*)(st_lse + tile * 16 + gq * 4);
                        const f32x4 d4 = *(const f32x4*)(st_dl + tile * 16 + gq * 4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int qi = tile * 16 + gq * 4 + e;
                            const bool ok = qi < m && (BIDIR ? kj < m : kj <= qi);
                            const float pp = ok ? __builtin_amdgcn_exp2f(sc[e] * scale2 - l4[e]) : 0.f;
                            float dm = 1.f;  // dropout factor m / (1 - p) of (query, key)
                            if (DROP) {
                                const unsigned long long idx = ((unsigned long long)gid * dr.L_pad + qi) * dr.L_pad + kj;
                                dm = drop_keep(dseed, idx, dr.thr) ? dr.inv : 0.f;
                            }
                            pf[t * 4 + e] = (bf16)(DROP ? pp * dm : pp);
                            dsf[t * 4 + e] = (bf16)(ok ? pp * ((DROP ? dp[e] * dm : dp[e]) - d4[e]) * scale : 0.f);
                        }
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) { pf[t * 4 + e] = (bf16)0.f; dsf[t * 4 + e] = (bf16)0.f; }
                    }
                }
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_T_lim<true>(Ds, u, dt, lane, RA), pf, dv[dt], 0, 0, 0);
                    dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_T_lim<true>(Qs, u, dt, lane, RA), dsf, dk[dt], 0, 0, 0);
                }
            }
            auto krowp = [&](int third) {
                return [&, third](int rr) -> bf16* {
                    const int j = kt * 16 + rr;
                    return j < m ? dqkv + (size_t)(s0 + j) * lddq + third * W + hcol : nullptr; };
            };
            store_tile_rows(opatch, dk, lane, krowp(1));
            store_tile_rows(opatch, dv, lane, krowp(2));
        }
        gid = gnext;
    }
}

// ---- backward of attn_fwd_packed_last_kernel: the one query of a sequence sits at its last row.  fp32 throughout, a wave per
// (sequence, head): lanes over the keys for P and dS (up to two keys per lane), then lanes over the 64 head columns for
// dQ = scale sum_j dS_j K_j (summed in key order), dK_j = scale dS_j q and dV_j = P_j dO.  Every row of the sequence is written in all
// three thirds: the dQ third of the rows that are no query is zeroed HERE (not by the caller), so a skipped sequence stays untouched.
__global__ __launch_bounds__(256) void attn_bwd_packed_last_kernel(
    const bf16* __restrict__ qkv, int ld, const int* __restrict__ seq_start, int N, int M, int heads, float scale2, float scale,
    const bf16* __restrict__ dO, int lddo, const bf16* __restrict__ O, int ldo, const float* __restrict__ lse2,
    float* __restrict__ delta, bf16* __restrict__ dqkv, int lddq) {
    const int lane = threadIdx.x & 63;
    const int gid = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gid >= N * heads) return;
    const int s = gid / heads, h = gid % heads, W = heads * DH;
    const int s0 = seq_start[s], s1 = seq_start[s + 1], m = s1 - s0;
    if (s0 < 0 || s1 > M || m < 1 || m > 80) return;
    const bf16* base = qkv + (size_t)s0 * ld + h * DH;
    const size_t last = (size_t)(s1 - 1);
    const float lse = lse2[last * heads + h];
    const float do_d = (float)dO[last * lddo + h * DH + lane], q_d = (float)base[(size_t)(m - 1) * ld + lane];
    const float dlt = wave_sum(do_d * (float)O[last * ldo + h * DH + lane]);
    if (lane == 0) delta[last * heads + h] = dlt;
    bf16x8 q[NCH], go[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        q[c] = ldg8(base + (size_t)(m - 1) * ld + c * 8);
        go[c] = ldg8(dO + last * lddo + h * DH + c * 8);
    }
    float p[2], ds[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int j = lane + 64 * kk;
        float dot = 0.f, dp = 0.f;
        if (j < m) {
            const bf16* kr = base + (size_t)j * ld + W;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const bf16x8 kv = ldg8(kr + c * 8), vv = ldg8(kr + W + c * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    dot = __builtin_fmaf((float)q[c][e], (float)kv[e], dot);
                    dp = __builtin_fmaf((float)go[c][e], (float)vv[e], dp);
                }
            }
        }
        p[kk] = j < m ? __builtin_amdgcn_exp2f(dot * scale2 - lse) : 0.f;
        ds[kk] = p[kk] * (dp - dlt) * scale;
    }
    float dq = 0.f;
    bf16* drow = dqkv + (size_t)s0 * lddq + h * DH + lane;
    for (int j = 0; j < m; ++j) {
        const float pj = __shfl(j < 64 ? p[0] : p[1], j & 63, 64), dsj = __shfl(j < 64 ? ds[0] : ds[1], j & 63, 64);
        dq = __builtin_fmaf(dsj, (float)base[(size_t)j * ld + W + lane], dq);
        bf16* r = drow + (size_t)j * lddq;
        if (j < m - 1) r[0] = (bf16)0.f;
        r[W] = (bf16)(dsj * q_d);
        r[2 * W] = (bf16)(pj * do_d);
    }
    drow[(size_t)(m - 1) * lddq] = (bf16)dq;
}

}  // namespace NS_DH

static int packed_args_ok(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, const void* out, int ldo) {
    if (!qkv || !seq_start || !out || N <= 0 || M <= 0 || heads <= 0 || ld % 8 || ldo % 8) return TVTS_EINVAL;
    if (ld < 3 * heads * DH || ldo < heads * DH || max_len < 1 || max_len > 80) return TVTS_EINVAL;
    return TVTS_OK;
}

static int packed_fwd(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, void* out, int ldo, float* lse2,
                      hipStream_t stream) {
    const float scale2 = 1.4426950408889634f / sqrtf((float)DH);
    const int groups = N * heads;
    const int blocks = ceil_div(groups, 4) < 1536 ? ceil_div(groups, 4) : 1536;
#define PACKED_LAUNCH(MT)                                                                                                      \
    do {                                                                                                                       \
        if (lse2)                                                                                                              \
            hipLaunchKernelGGL((attn_fwd_packed_kernel<MT, true>), dim3(blocks), dim3(256), 4 * (MT * 16 * VSTRIDE + 1024),    \
                               stream, (const bf16*)qkv, ld, seq_start, N, M, heads, scale2, (bf16*)out, ldo, lse2, PackedDrop{});\
        else                                                                                                                   \
            hipLaunchKernelGGL((attn_fwd_packed_kernel<MT, false>), dim3(blocks), dim3(256), 4 * (MT * 16 * VSTRIDE + 1024),   \
                               stream, (const bf16*)qkv, ld, seq_start, N, M, heads, scale2, (bf16*)out, ldo, (float*)nullptr, \
                               PackedDrop{});                                                                                  \
    } while (0)
    PACKED_LAUNCH(1);
    if (max_len > 16) PACKED_LAUNCH(2);
    if (max_len > 32) PACKED_LAUNCH(3);
    if (max_len > 48) PACKED_LAUNCH(5);
#undef PACKED_LAUNCH
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

extern "C" int tvts_attn_fwd_packed(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, void* out,
                                    int ldo, hipStream_t stream) {
    const int rc = packed_args_ok(qkv, ld, seq_start, N, M, heads, max_len, out, ldo);
    return rc ? rc : packed_fwd(qkv, ld, seq_start, N, M, heads, max_len, out, ldo, nullptr, stream);
}

extern "C" int tvts_attn_fwd_packed_lse(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, void* out,
                                        int ldo, float* lse2, hipStream_t stream) {
    const int rc = packed_args_ok(qkv, ld, seq_start, N, M, heads, max_len, out, ldo);
    if (rc || !lse2) return TVTS_EINVAL;
    return packed_fwd(qkv, ld, seq_start, N, M, heads, max_len, out, ldo, lse2, stream);
}

static int packed_fwd_last(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, void* out, int ldo, float* lse2,
                           hipStream_t stream) {
    const float scale2 = 1.4426950408889634f / sqrtf((float)DH);
    hipLaunchKernelGGL(attn_fwd_packed_last_kernel<false>, dim3(ceil_div(N * heads, 4)), dim3(256), 0, stream, (const bf16*)qkv, ld,
                       seq_start, N, M, heads, scale2, (bf16*)out, ldo, lse2);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

extern "C" int tvts_attn_fwd_packed_last(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len,
                                         void* out, int ldo, hipStream_t stream) {
    const int rc = packed_args_ok(qkv, ld, seq_start, N, M, heads, max_len, out, ldo);
    return rc ? rc : packed_fwd_last(qkv, ld, seq_start, N, M, heads, out, ldo, nullptr, stream);
}

extern "C" int tvts_attn_fwd_packed_last_lse(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len,
                                             void* out, int ldo, float* lse2, hipStream_t stream) {
    const int rc = packed_args_ok(qkv, ld, seq_start, N, M, heads, max_len, out, ldo);
    if (rc || !lse2) return TVTS_EINVAL;
    return packed_fwd_last(qkv, ld, seq_start, N, M, heads, out, ldo, lse2, stream);
}

static int packed_bwd_args_ok(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, const void* dO,
                              int lddo, const void* O, int ldo, const float* lse2, const float* delta, const void* dqkv, int lddq) {
    const int rc = packed_args_ok(qkv, ld, seq_start, N, M, heads, max_len, O, ldo);
    if (rc) return rc;
    if (!dO || !lse2 || !delta || !dqkv || lddo % 8 || lddq % 8 || lddo < heads * DH || lddq < 3 * heads * DH) return TVTS_EINVAL;
    return TVTS_OK;
}

extern "C" int tvts_attn_bwd_packed(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, const void* dO,
                                    int lddo, const void* O, int ldo, const float* lse2, float* delta, void* dqkv, int lddq,
                                    hipStream_t stream) {
    const int rc = packed_bwd_args_ok(qkv, ld, seq_start, N, M, heads, max_len, dO, lddo, O, ldo, lse2, delta, dqkv, lddq);
    if (rc) return rc;
    const float scale = 1.0f / sqrtf((float)DH), scale2 = 1.4426950408889634f * scale;
    const int groups = N * heads;
#define PACKED_LAUNCH(MT)                                                                                                      \
    do {                                                                                                                       \
        constexpr int WV = MT <= 3 ? 2 : 1, WB = 4 * MT * 16 * VSTRIDE + 2 * MT * 16 * 4 + 1024;                               \
        const int blocks = ceil_div(groups, WV) < 2048 ? ceil_div(groups, WV) : 2048;                                          \
        hipLaunchKernelGGL((attn_bwd_packed_kernel<MT>), dim3(blocks), dim3(64 * WV), WV * WB, stream, (const bf16*)qkv, ld,   \
                           seq_start, N, M, heads, scale2, scale, (const bf16*)dO, lddo, (const bf16*)O, ldo, lse2, delta,     \
                           (bf16*)dqkv, lddq, PackedDrop{});                                                                   \
    } while (0)
    PACKED_LAUNCH(1);
    if (max_len > 16) PACKED_LAUNCH(2);
    if (max_len > 32) PACKED_LAUNCH(3);
    if (max_len > 48) PACKED_LAUNCH(5);
#undef PACKED_LAUNCH
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

extern "C" int tvts_attn_bwd_packed_last(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len,
                                         const void* dO, int lddo, const void* O, int ldo, const float* lse2, float* delta, void* dqkv,
                                         int lddq, hipStream_t stream) {
    const int rc = packed_bwd_args_ok(qkv, ld, seq_start, N, M, heads, max_len, dO, lddo, O, ldo, lse2, delta, dqkv, lddq);
    if (rc) return rc;
    const float scale = 1.0f / sqrtf((float)DH), scale2 = 1.4426950408889634f * scale;
    hipLaunchKernelGGL(attn_bwd_packed_last_kernel, dim3(ceil_div(N * heads, 4)), dim3(256), 0, stream, (const bf16*)qkv, ld,
                       seq_start, N, M, heads, scale2, scale, (const bf16*)dO, lddo, (const bf16*)O, ldo, lse2, delta, (bf16*)dqkv,
                       lddq);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---- bidirectional forms (the DistilBERT tower of v1 over packed captions): the same ownership, tile classes and guard;
// p > 0 selects the DROP instantiations, p == 0 the ones without any generator work
static int packed_drop_args(float p, const long* seed_dev, long site, int L_pad, int max_len, PackedDrop* dr) {
    if (!(p >= 0.f) || p >= 1.f || L_pad < max_len || (p > 0.f && !seed_dev)) return TVTS_EINVAL;
    *dr = PackedDrop{(unsigned)((double)p * 4294967296.0), 1.0f / (1.0f - p), (const unsigned long long*)seed_dev, (unsigned long long)site,
                     L_pad};
    return TVTS_OK;
}

extern "C" int tvts_attn_fwd_packed_bidir(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, void* out,
                                          int ldo, float* lse2, float p, const long* seed_dev, long site, int L_pad, hipStream_t stream) {
    int rc = packed_args_ok(qkv, ld, seq_start, N, M, heads, max_len, out, ldo);
    if (rc) return rc;
    PackedDrop dr;
    if ((rc = packed_drop_args(p, seed_dev, site, L_pad, max_len, &dr))) return rc;
    const float scale2 = 1.4426950408889634f / sqrtf((float)DH);
    const int groups = N * heads;
    const int blocks = ceil_div(groups, 4) < 1536 ? ceil_div(groups, 4) : 1536;
#define PACKED_LAUNCH_(MT, LSE, DROP)                                                                                          \
    hipLaunchKernelGGL((attn_fwd_packed_kernel<MT, LSE, true, DROP>), dim3(blocks), dim3(256), 4 * (MT * 16 * VSTRIDE + 1024), \
                       stream, (const bf16*)qkv, ld, seq_start, N, M, heads, scale2, (bf16*)out, ldo, lse2, dr)
#define PACKED_LAUNCH(MT)                                                   \
    do {                                                                    \
        if (p > 0.f) { if (lse2) PACKED_LAUNCH_(MT, true, true); else PACKED_LAUNCH_(MT, false, true); }   \
        else { if (lse2) PACKED_LAUNCH_(MT, true, false); else PACKED_LAUNCH_(MT, false, false); }         \
    } while (0)
    PACKED_LAUNCH(1);
    if (max_len > 16) PACKED_LAUNCH(2);
    if (max_len > 32) PACKED_LAUNCH(3);
    if (max_len > 48) PACKED_LAUNCH(5);
#undef PACKED_LAUNCH
#undef PACKED_LAUNCH_
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

extern "C" int tvts_attn_fwd_packed_first(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len, void* out,
                                          int ldo, hipStream_t stream) {
    const int rc = packed_args_ok(qkv, ld, seq_start, N, M, heads, max_len, out, ldo);
    if (rc) return rc;
    const float scale2 = 1.4426950408889634f / sqrtf((float)DH);
    hipLaunchKernelGGL(attn_fwd_packed_last_kernel<true>, dim3(ceil_div(N * heads, 4)), dim3(256), 0, stream, (const bf16*)qkv, ld,
                       seq_start, N, M, heads, scale2, (bf16*)out, ldo, (float*)nullptr);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

extern "C" int tvts_attn_bwd_packed_bidir(const void* qkv, int ld, const int* seq_start, int N, int M, int heads, int max_len,
                                          const void* dO, int lddo, const void* O, int ldo, const float* lse2, float* delta, void* dqkv,
                                          int lddq, float p, const long* seed_dev, long site, int L_pad, hipStream_t stream) {
    int rc = packed_bwd_args_ok(qkv, ld, seq_start, N, M, heads, max_len, dO, lddo, O, ldo, lse2, delta, dqkv, lddq);
    if (rc) return rc;
    PackedDrop dr;
    if ((rc = packed_drop_args(p, seed_dev, site, L_pad, max_len, &dr))) return rc;
    const float scale = 1.0f / sqrtf((float)DH), scale2 = 1.4426950408889634f * scale;
    const int groups = N * heads;
#define PACKED_LAUNCH_(MT, DROP)                                                                                                \
    do {                                                                                                                        \
        constexpr int WV = MT <= 3 ? 2 : 1, WB = 4 * MT * 16 * VSTRIDE + 2 * MT * 16 * 4 + 1024;                                \
        const int blocks = ceil_div(groups, WV) < 2048 ? ceil_div(groups, WV) : 2048;                                           \
        hipLaunchKernelGGL((attn_bwd_packed_kernel<MT, true, DROP>), dim3(blocks), dim3(64 * WV), WV * WB, stream,              \
                           (const bf16*)qkv, ld, seq_start, N, M, heads, scale2, scale, (const bf16*)dO, lddo, (const bf16*)O,  \
                           ldo, lse2, delta, (bf16*)dqkv, lddq, dr);                                                            \
    } while (0)
#define PACKED_LAUNCH(MT)                                                          \
    do { if (p > 0.f) PACKED_LAUNCH_(MT, true); else PACKED_LAUNCH_(MT, false); } while (0)
    PACKED_LAUNCH(1);
    if (max_len > 16) PACKED_LAUNCH(2);
    if (max_len > 32) PACKED_LAUNCH(3);
    if (max_len > 48) PACKED_LAUNCH(5);
#undef PACKED_LAUNCH
#undef PACKED_LAUNCH_
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
