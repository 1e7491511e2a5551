// Kernels of the v1 action-recognition fine-tuning step (v1/downstream/run_class_finetuning.py, engine_for_finetuning.py,
// optim_factory.py): what fine-tuning adds on top of the pretrain step's kernels.
//
//   tvts_drop_path_table   the step's stochastic-depth draw: one keep / drop decision per (branch, sample)
//   tvts_drop_path_rows    out = residual + scale[sample] * y (forward) / dy_branch = scale[sample] * d_out (backward)
//   tvts_soft_ce           soft-target / label-smoothing cross entropy on [B, C] logits: loss, dlogits, top-1 hit count
//   tvts_mix_targets       the soft targets of a Mixup / CutMix step from labels and the step's mix table
//   tvts_grad_sumsq        global gradient norm over the trainable chunks of the flat gradient buffer + the clip coefficient,
//                          both left in device memory
// (the step's optimizer, tvts_adamw_torch, is in optim.hip beside tvts_adamw_hf: the two share one chunk frame)
//
// Every reduction here runs in a FIXED order (no float atomics): two runs over the same bits give the same bits.
#include "common.h"

// ---------------------------------------------------------------------------------------------- stochastic depth
// timm DropPath (video_encoder.py:65,71-72): one Bernoulli draw per sample per branch, kept samples divided by the keep
// probability.  Site s = 2 l (attention branch of block l) or 2 l + 1 (its MLP branch).  The draw is the repository's counter-based
// generator (attention.hip::drop_keep, embed.hip dropout_rows_kernel), with the site as the stream and the sample as the counter:
//     key = seed_dev[0] + (site_base + s) * 0x632BE59BD9B4E019      (mod 2^64; the site stride of tvts_dropout_rows' callers)
//     z   = key + b * 0x9E3779B97F4A7C15
//     z   = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31
//     keep iff (z >> 32) >= thr,  thr = (uint32)((double)p_s * 2^32)
// scale[s, b] = keep ? 1.0f / (1.0f - p_s) : 0.0f; a site with p_s <= 0 gets exactly 1.0f, one with p_s >= 1 exactly 0.
__global__ __launch_bounds__(256) void drop_path_table_kernel(const unsigned long long* __restrict__ seed_dev,
                                                              unsigned long long site_base, const float* __restrict__ p,
                                                              int nsites, int B, float* __restrict__ scale) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)nsites * B) return;
    const int s = (int)(i / B), b = (int)(i % B);
    const float ps = p[s];
    float out;
    if (!(ps > 0.f)) out = 1.0f;
    else if (ps >= 1.0f) out = 0.f;
    else {
        const unsigned thr = (unsigned)((double)ps * 4294967296.0);
        unsigned long long z = seed_dev[0] + (site_base + (unsigned long long)s) * 0x632BE59BD9B4E019ull;
        z += (unsigned long long)b * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        out = ((unsigned)(z >> 32) >= thr) ? 1.0f / (1.0f - ps) : 0.f;
    }
    scale[i] = out;
}
extern "C" int tvts_drop_path_table(const long* seed_dev, long site_base, const float* p_sites, int nsites, int B, float* scale,
                                    hipStream_t stream) {
    if (!seed_dev || !p_sites || !scale || nsites <= 0 || B <= 0) return TVTS_EINVAL;
    const long n = (long)nsites * B;
    hipLaunchKernelGGL(drop_path_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       (const unsigned long long*)seed_dev, (unsigned long long)site_base, p_sites, nsites, B, scale);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// out[r, :] = residual[r, :] + scale[r / S] * y[r, :]: the product rounded to fp32, then the sum rounded to fp32 (no contraction).
// A dropped sample (scale == 0) copies the residual's bits (exact zeros without one) whatever y holds; scale == 1 is the plain add.
__global__ __launch_bounds__(256) void drop_path_rows_kernel(const float* __restrict__ y, long ldy, long rows, int c4, int S,
                                                             const float* __restrict__ scale, const float* __restrict__ residual,
                                                             long ldr, float* __restrict__ out, long ldo, bf16* __restrict__ outb,
                                                             long ldob) {
#pragma clang fp contract(off)
    const long n = rows * c4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long r = i / c4;
        const int c = (int)(i - r * c4) * 4;
        const float s = scale[r / S];
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (residual) v = *(const f32x4*)(residual + r * ldr + c);
        if (s != 0.f) {
            const f32x4 yv = *(const f32x4*)(y + r * ldy + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t = s * yv[e];
                v[e] = residual ? v[e] + t : t;
            }
        }
        if (out) *(f32x4*)(out + r * ldo + c) = v;
        if (outb) *(bf16x4*)(outb + r * ldob + c) = (bf16x4){(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
    }
}
extern "C" int tvts_drop_path_rows(const float* y, long ldy, long rows, int cols, int S, const float* scale, const float* residual,
                                   long ldr, float* out, long ldo, void* out_bf16, long ldob, hipStream_t stream) {
    if (!y || !scale || rows <= 0 || cols <= 0 || S <= 0 || rows % S || cols % 4 || ldy % 4 || ldy < cols || ((size_t)y % 16) ||
        (!out && !out_bf16))
        return TVTS_EINVAL;
    if (residual && (ldr % 4 || ldr < cols || ((size_t)residual % 16))) return TVTS_EINVAL;
    if (out && (ldo % 4 || ldo < cols || ((size_t)out % 16))) return TVTS_EINVAL;
    if (out_bf16 && (ldob % 4 || ldob < cols || ((size_t)out_bf16 % 8))) return TVTS_EINVAL;
    const long n = rows * (cols / 4);
    long blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(drop_path_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, y, ldy, rows, cols / 4, S, scale,
                       residual, ldr, out, ldo, (bf16*)out_bf16, ldob);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---------------------------------------------------------------------------------------------- block reductions, fixed order
// 256 threads: butterfly inside each wave, then the four wave results in wave order, by every thread alike (sums: block_sum_256
// of common.h)
// (value, index): the larger value, the smaller index among equal values; NaN never wins
__device__ __forceinline__ void amax_pair(float& v, int& i, float v2, int i2) {
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}
__device__ __forceinline__ int block_argmax256(float v, int i, float* shv, int* shi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(v, o, 64);
        const int i2 = __shfl_xor(i, o, 64);
        amax_pair(v, i, v2, i2);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { shv[threadIdx.x >> 6] = v; shi[threadIdx.x >> 6] = i; }
    __syncthreads();
    v = shv[0]; i = shi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) amax_pair(v, i, shv[w], shi[w]);
    return i;
}

// ---------------------------------------------------------------------------------------------- soft-target cross entropy
// One block per row b of the [B, C] fp32 logits x.  Target row t: the soft targets [B, C] (timm SoftTargetCrossEntropy,
// run_class_finetuning.py:423), or from an int32 label y and a smoothing eps: t_c = (1 - eps) [c == y] + eps / C
// (LabelSmoothingCrossEntropy :425, (1 - eps) nll + eps mean_c(-logp); eps = 0: nn.CrossEntropyLoss :427).
//   loss_b = - sum_c t_c logp_c,   logp_c = (x_c - max) - log(sum_c exp(x_c - max))
//   dlogits[b, c] = gscale / B * (softmax_c * sum_c t_c - t_c)
//   hit_b = [argmax_c x == argmax_c t]  (first index among equal values, engine_for_finetuning.py:104)
// Row results go to ws[0:B] (loss) and ws[B:2B] (hit); soft_ce_finish_kernel (one block) sums them in a fixed order.
__global__ __launch_bounds__(256) void soft_ce_rows_kernel(const float* __restrict__ x, long ldx, int B, int C,
                                                           const float* __restrict__ tgt, long ldt, const int* __restrict__ labels,
                                                           float eps, float gscale, float* __restrict__ dlogits, long ldd,
                                                           float* __restrict__ ws) {
    __shared__ float shv[4];
    __shared__ int shi[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* xr = x + (long)b * ldx;
    const float* tr = tgt ? tgt + (long)b * ldt : nullptr;
    const int lab = labels ? labels[b] : -1;
    const float t_on = 1.0f - eps + eps / (float)C, t_off = eps / (float)C;
    float mx = -INFINITY, mt = -INFINITY, st = 0.f;
    int ix = 0x7fffffff, it = 0x7fffffff;
    for (int c = tid; c < C; c += 256) {
        amax_pair(mx, ix, xr[c], c);
        const float t = tr ? tr[c] : (c == lab ? t_on : t_off);
        if (tr) amax_pair(mt, it, t, c);
        st += t;
    }
    ix = block_argmax256(mx, ix, shv, shi);
    it = tr ? block_argmax256(mt, it, shv, shi) : lab;
    st = block_sum_256(st, shv);
    const float xmax = xr[ix < C ? ix : 0];
    float se = 0.f;
    for (int c = tid; c < C; c += 256) se += expf(xr[c] - xmax);
    se = block_sum_256(se, shv);
    const float lse = logf(se), inv = 1.0f / se, g = gscale / (float)B;
    float acc = 0.f;
    for (int c = tid; c < C; c += 256) {
        const float t = tr ? tr[c] : (c == lab ? t_on : t_off);
        const float z = xr[c] - xmax;
        if (t != 0.f) acc -= t * (z - lse);  // (t == 0 contributes nothing, also where logp = -inf)
        if (dlogits) dlogits[(long)b * ldd + c] = g * (expf(z) * inv * st - t);
    }
    acc = block_sum_256(acc, shv);
    if (tid == 0) {
        ws[b] = acc;
        ws[B + b] = ix == it ? 1.0f : 0.f;
    }
}
__global__ __launch_bounds__(256) void soft_ce_finish_kernel(const float* __restrict__ ws, int B, float gscale,
                                                             float* __restrict__ loss_acc, int* __restrict__ hits) {
    __shared__ float sh[4];
    float l = 0.f, h = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) { l += ws[b]; h += ws[B + b]; }
    l = block_sum_256(l, sh);
    h = block_sum_256(h, sh);  // (exact: integers below 2^24)
    if (threadIdx.x == 0) {
        loss_acc[0] += gscale * (l / (float)B);
        if (hits) hits[0] = (int)h;
    }
}
extern "C" int tvts_soft_ce(const float* logits, long ld, int B, int C, const float* soft_targets, long ldt, const int* labels,
                            float smoothing, float scale, float* loss_acc, float* dlogits, long ldd, int* hits, float* ws,
                            hipStream_t stream) {
    if (!logits || !loss_acc || !ws || B <= 0 || C <= 0 || ld < C || B >= (1 << 24)) return TVTS_EINVAL;
    if ((soft_targets != nullptr) == (labels != nullptr)) return TVTS_EINVAL;  // exactly one kind of target
    if (soft_targets && ldt < C) return TVTS_EINVAL;
    if (dlogits && ldd < C) return TVTS_EINVAL;
    if (!(smoothing >= 0.f && smoothing < 1.f) || (soft_targets && smoothing != 0.f)) return TVTS_EINVAL;
    hipLaunchKernelGGL(soft_ce_rows_kernel, dim3(B), dim3(256), 0, stream, logits, ld, B, C, soft_targets, ldt, labels, smoothing,
                       scale, dlogits, ldd, ws);
    hipLaunchKernelGGL(soft_ce_finish_kernel, dim3(1), dim3(256), 0, stream, ws, B, scale, loss_acc, hits);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---------------------------------------------------------------------------------------------- Mixup / CutMix soft targets
// mixup_target (v1/downstream/mixup.py:18-23) over the step's mix table (embed.hip, MixRow of tube_gather_kernel):
//   t[b, c] = fadd_rn(fmul_rn(y1, lam), fmul_rn(y2, one_minus_lam)),  y1 = on / off for labels[b], y2 = on / off for labels[partner[b]]
// on / off arrive rounded to fp32 (torch.full of the double values).  A mode-0 row takes lam = 1, one_minus_lam = 0 and still
// runs the arithmetic (the reference computes y1 * 1. + y2 * 0. there).  A partner outside [0, B) leaves its row unwritten.
__global__ __launch_bounds__(256) void mix_targets_kernel(const int* __restrict__ labels, const int* __restrict__ mix_i,
                                                          const float* __restrict__ mix_f, int B, int C, float on, float off,
                                                          float* __restrict__ out, long ldo) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * C) return;
    const int b = (int)(idx / C), c = (int)(idx % C);
    const int partner = mix_i[6 * (size_t)b], mode = mix_i[6 * (size_t)b + 1];
    if ((unsigned)partner >= (unsigned)B) return;
    const float lam = mode == 0 ? 1.0f : mix_f[2 * (size_t)b], oml = mode == 0 ? 0.0f : mix_f[2 * (size_t)b + 1];
    const float y1 = c == labels[b] ? on : off, y2 = c == labels[partner] ? on : off;
    out[(long)b * ldo + c] = __fadd_rn(__fmul_rn(y1, lam), __fmul_rn(y2, oml));
}
extern "C" int tvts_mix_targets(const int* labels, const int* mix_i, const float* mix_f, int B, int C, double smoothing, float* out,
                                long ldo, hipStream_t stream) {
    if (!labels || !mix_i || !mix_f || !out || B <= 0 || C <= 0 || ldo < C || !(smoothing >= 0.0 && smoothing < 1.0)) return TVTS_EINVAL;
    const double off = smoothing / (double)C, on = 1.0 - smoothing + off;  // mixup.py:19-20, in double as Python computes them
    const long n = (long)B * C;
    hipLaunchKernelGGL(mix_targets_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, labels, mix_i, mix_f, B, C,
                       (float)on, (float)off, out, ldo);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---------------------------------------------------------------------------------------------- global gradient norm + clip coefficient
// Stage 1: one block per 1024-element chunk of the flat gradient buffer -> partial[chunk] = sum of its squares (0 for a chunk of
// group 255: frozen / padding, never read).  Stage 2: one block adds the partials in double, thread t taking t, t + 1024, ... in
// turn, then a fixed tree.  norm = |grad_scale| sqrt(sum); coef = min(1, max_norm / (norm + 1e-6)) as torch.nn.utils.clip_grad_norm_
// (utils.py:366), 1 when max_norm <= 0 (clipping off).  norm_coef[0] = norm, norm_coef[1] = coef.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, const unsigned char* __restrict__ chunk_group,
                                                         float* __restrict__ partial) {
    __shared__ float sh[4];
    if (chunk_group[blockIdx.x] == 255) {  // (uniform per block)
        if (threadIdx.x == 0) partial[blockIdx.x] = 0.f;
        return;
    }
    const f32x4 v = *(const f32x4*)(g + (size_t)blockIdx.x * 1024 + threadIdx.x * 4);
    const float s = block_sum_256((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]), sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ __launch_bounds__(1024) void grad_norm_coef_kernel(const float* __restrict__ partial, int nchunks, float max_norm,
                                                              float grad_scale, float* __restrict__ norm_coef) {
    __shared__ double sh[1024];
    double a = 0.0;
    for (int i = threadIdx.x; i < nchunks; i += 1024) a += (double)partial[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm = fabsf(grad_scale) * (float)sqrt(sh[0]);
        float coef = 1.0f;
        if (max_norm > 0.f) coef = fminf(1.0f, max_norm / (norm + 1e-6f));
        norm_coef[0] = norm;
        norm_coef[1] = coef;
    }
}
extern "C" int tvts_grad_sumsq(const float* g, const unsigned char* chunk_group, int nchunks, float* partial, float max_norm,
                               float grad_scale, float* norm_coef, hipStream_t stream) {
    if (!g || !chunk_group || !partial || !norm_coef || nchunks <= 0 || ((size_t)g % 16)) return TVTS_EINVAL;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(nchunks), dim3(256), 0, stream, g, chunk_group, partial);
    hipLaunchKernelGGL(grad_norm_coef_kernel, dim3(1), dim3(1024), 0, stream, partial, nchunks, max_norm, grad_scale, norm_coef);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---------------------------------------------------------------------------------------------- evaluation: ranks, view merge
// validation_one_epoch / final_test / merge of v1/downstream/engine_for_finetuning.py:142-285 (tvts_amd/downstream/evaluate_v1.py).
__device__ __forceinline__ int block_isum_256(int v, int* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
// One block per row: rank = #{c : x_c > x_label} + #{c < label : x_c == x_label}, integer counts (exact at any C).  `rank < k` is the
// top-k hit with ties resolved towards the lower class index, so rank 0 is np.argmax == label.  Every comparison with a NaN is false.
__global__ __launch_bounds__(256) void class_ranks_kernel(const float* __restrict__ x, long ld, int C, const int* __restrict__ labels,
                                                          int* __restrict__ ranks) {
    __shared__ int sh[4];
    const int r = blockIdx.x, lab = labels[r];
    if ((unsigned)lab >= (unsigned)C) {  // (uniform per block) nothing is read for a label outside the row
        if (threadIdx.x == 0) ranks[r] = C;
        return;
    }
    const float* xr = x + (long)r * ld;
    const float xl = xr[lab];
    int cnt = 0;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float v = xr[c];
        cnt += (v > xl) || (v == xl && c < lab);
    }
    cnt = block_isum_256(cnt, sh);
    if (threadIdx.x == 0) ranks[r] = cnt;
}
extern "C" int tvts_class_ranks(const float* x, long ld, int R, int C, const int* labels, int* ranks, hipStream_t stream) {
    if (!x || !labels || !ranks || R <= 0 || C <= 0 || ld < C) return TVTS_EINVAL;
    hipLaunchKernelGGL(class_ranks_kernel, dim3(R), dim3(256), 0, stream, x, ld, C, labels, ranks);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// compute_video's `np.mean(feat, axis=0)` (:277) as a SUM: one thread per (video, class) adds the seen views in the order v = 0 .. V - 1
// from +0.0f, every add rounded -- the order is the definition, so the bits repeat.  The division by the count is left out: it does not
// change the order of a video's classes, which is all that argmax and top-5 membership read.
__global__ __launch_bounds__(256) void view_sum_kernel(const float* __restrict__ vl, const unsigned char* __restrict__ seen, int N, int V,
                                                       int C, float* __restrict__ sum, long lds, int* __restrict__ count) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)N * C) return;
    const int nv = (int)(idx / C), c = (int)(idx % C);
    float s = 0.0f;
    int k = 0;
    for (int v = 0; v < V; ++v)
        if (seen[(size_t)nv * V + v]) {
            s = __fadd_rn(s, vl[((size_t)nv * V + v) * C + c]);
            ++k;
        }
    sum[(long)nv * lds + c] = s;
    if (c == 0) count[nv] = k;
}
extern "C" int tvts_view_sum(const float* view_logits, const unsigned char* seen, int N, int V, int C, float* sum, long lds, int* count,
                             hipStream_t stream) {
    if (!view_logits || !seen || !sum || !count || N <= 0 || V <= 0 || C <= 0 || lds < C || (long)N * V >= (1L << 31)) return TVTS_EINVAL;
    const long n = (long)N * C;
    if ((n + 255) / 256 >= (1L << 31)) return TVTS_EINVAL;
    hipLaunchKernelGGL(view_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, view_logits, seen, N, V, C, sum, lds, count);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// One block per row of a batch's logits: the row lands in its view slot unless the slot is seen already or an earlier row of the batch
// names it (merge keeps the first line of a (video, chunk, split), :251-252).  Every thread reads seen[slot] in front of the barrier
// and thread 0 sets it behind it; a later row with the same slot is dropped by the earlier-row rule whichever value it reads.
// Rows of one video carry one label: whichever of them writes video_labels[video] last writes the same value.
__global__ __launch_bounds__(256) void view_store_kernel(const float* __restrict__ logits, long ld, int C, const int* __restrict__ slot,
                                                         const int* __restrict__ labels, int nslots, int V, float* __restrict__ vl,
                                                         unsigned char* __restrict__ seen, int* __restrict__ video_labels) {
    const int b = blockIdx.x, s = slot[b];
    if ((unsigned)s >= (unsigned)nslots) return;  // (uniform per block)
    int dup = seen[s] != 0;
    for (int j = threadIdx.x; j < b; j += 256) dup |= slot[j] == s;
    if (__syncthreads_or(dup)) return;
    for (int c = threadIdx.x; c < C; c += 256) vl[(size_t)s * C + c] = logits[(long)b * ld + c];
    if (threadIdx.x == 0) {
        seen[s] = 1;
        video_labels[s / V] = labels[b];
    }
}
extern "C" int tvts_view_store(const float* logits, long ld, int B, int C, const int* slot, const int* labels, int N, int V,
                               float* view_logits, unsigned char* seen, int* video_labels, hipStream_t stream) {
    if (!logits || !slot || !labels || !view_logits || !seen || !video_labels || B <= 0 || C <= 0 || ld < C || N <= 0 || V <= 0 ||
        (long)N * V >= (1L << 31))
        return TVTS_EINVAL;
    hipLaunchKernelGGL(view_store_kernel, dim3(B), dim3(256), 0, stream, logits, ld, C, slot, labels, N * V, V, view_logits, seen,
                       video_labels);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
