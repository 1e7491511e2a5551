// Optimizer-side kernels over the FLAT fp32 parameter / gradient / moment buffers.
//
//   tvts_adamw_hf        multi-tensor AdamW with Hugging Face semantics (transformers==4.10.2 `AdamW`, the optimizer
//                        the reference builds at v2/train_dist_TVTSv2_ViT_B_16.py:118-125): bias-corrected step,
//                        eps added OUTSIDE the correction, decoupled decay `p -= lr*wd*p` AFTER the Adam update.
//                        One launch for all ~400 tensors: the flat buffers are cut into 1024-element chunks and a
//                        byte table gives each chunk its parameter group (255 = frozen / padding).  The same pass
//                        applies the data-parallel 1/world gradient scale and refreshes the bf16 weight shadow.
//   tvts_adamw_hf_guarded   the same rule with the clip coefficient tvts_grad_sumsq left on the device and, optionally, under the
//                        overflow guard described below (the pretraining step with clip_grad / skip_nonfinite)
//   tvts_adamw_torch     the same frame with torch.optim.AdamW arithmetic over up to 64 groups (the v1 fine-tuning step)
//   tvts_sgd_torch       torch.optim.SGD (momentum, Nesterov) in the same frame with ONE state stream, bit for bit (the v1 linear
//                        probe, 22 B per element)
//                        Both take two optional parts as nullable pointers.  `ema`: the launch applies timm's ModelEma rule to the
//                        new p while it is still in registers (one more fp32 stream, + 8 B per element); tvts_ema_update is the rule
//                        as a pass of its own (ModelEma.update).  `skipped`: the launch runs under the overflow guard of the
//                        fine-tuning step -- the update happens only when the global gradient norm tvts_grad_sumsq left on the
//                        device is finite; else every bit of p / state / shadow / average stays, the device step counter stays
//                        and the device counter `skipped` advances
//   tvts_swap_f32_shadow in-place exchange of two fp32 buffers + the bf16 shadow of the first (evaluation from the average)
//   tvts_cast_f32_bf16   shadow refresh when an external optimizer owned the update (drop-in path)
//   tvts_transpose_bf16_batched   [N,K] -> [K,N] copies of every GEMM weight (dgrad operand), one launch
//   tvts_pad_rows_bf16 / tvts_add_rows_f32   K-padding of the 14x14 patch-embedding weight and its wgrad (H/14)
#include "common.h"

#include <initializer_list>
#include <type_traits>

// timm.utils.ModelEma.update per element: ema_v * decay + (1. - decay) * model_v on fp32 tensors with a Python-float decay, i.e.
// three roundings and no FMA, d32 = fp32(decay), o32 = fp32(1.0 - decay) with the difference formed in DOUBLE on the host (the
// fp32 difference 1 - d32 is another number: 1.00016594e-4 instead of 9.99999975e-5 at decay 0.9999).
__device__ __forceinline__ f32x4 ema_rule4(const f32x4& ev, const f32x4& pv, float d32, float o32) {
#pragma clang fp contract(off)
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float a = ev[e] * d32, b = o32 * pv[e];
        r[e] = a + b;
    }
    return r;
}

// The frame of the optimizer kernels: one block per 1024-element chunk, four elements per lane, 16-byte accesses.  The frame owns
// the group gate (a chunk whose group byte is not below NGROUPS -- a foreign group, 255 = frozen -- keeps every bit), the guard
// test, the element index, the loads and stores of p and g, the bf16 shadow and the average.  `prologue(grp)` runs once the chunk is
// known to step and returns the rule: the hyper-parameters of the group, and the rule's own state streams as
//     load(i)  /  update4(pv, gv)  /  store(i)        (StateStreams below: two moments for the AdamWs, one buffer or none for SGD)
// EMA: the frame also carries the chunk's average through ema_rule4 from the final p (a compile-time choice: an instantiation
// without an average neither loads nor tests `ema`).  GUARD (compile time as well): the frame first tests the global gradient norm
// `guard_norm[0]` -- one uniform load and one branch per block -- and a block that finds it not finite returns in front of every
// load of p or state: the whole launch then keeps every bit of p, the state, the shadow and the average.
__device__ __forceinline__ bool finite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
template <int NGROUPS, bool EMA, bool GUARD, typename Prologue>
__device__ __forceinline__ void optim_chunk(float* __restrict__ p, const float* __restrict__ g, bf16* __restrict__ shadow,
                                            const unsigned char* __restrict__ chunk_group, float* __restrict__ ema, float d32,
                                            float o32, const float* __restrict__ guard_norm, Prologue prologue) {
    const int grp = chunk_group[blockIdx.x];
    if (grp >= NGROUPS) return;
    if constexpr (GUARD) {
        if (!finite_f32(guard_norm[0])) return;
    }
    auto rule = prologue(grp);
    const size_t i = (size_t)blockIdx.x * 1024 + threadIdx.x * 4;
    f32x4 pv = *(f32x4*)(p + i);
    const f32x4 gv = *(const f32x4*)(g + i);
    rule.load(i);  // (behind g: with the state in front of it the SGD instantiations with momentum took two more VGPRs)
    f32x4 ev;
    if constexpr (EMA) ev = *(const f32x4*)(ema + i);
    rule.update4(pv, gv);
    *(f32x4*)(p + i) = pv;
    rule.store(i);
    if (shadow) *(bf16x4*)(shadow + i) = (bf16x4){(bf16)pv[0], (bf16)pv[1], (bf16)pv[2], (bf16)pv[3]};
    if constexpr (EMA) *(f32x4*)(ema + i) = ema_rule4(ev, pv, d32, o32);
}

// A rule's N state streams (fp32, the layout of p) around its four-element update `u(pv, state..., gv)`.  skip_load: the streams
// are written without being read (SGD's first update).
template <int N, typename Update4>
struct StateStreams {
    float* s[N ? N : 1];
    bool skip_load;
    Update4 u;
    f32x4 sv[N ? N : 1];
    __device__ __forceinline__ void load(size_t i) {
        if (skip_load) return;
#pragma unroll
        for (int k = 0; k < N; ++k) sv[k] = *(const f32x4*)(s[k] + i);
    }
    __device__ __forceinline__ void update4(f32x4& pv, const f32x4& gv) {
        if constexpr (N == 2) u(pv, sv[0], sv[1], gv);
        else u(pv, sv[0], gv);
    }
    __device__ __forceinline__ void store(size_t i) {
#pragma unroll
        for (int k = 0; k < N; ++k) *(f32x4*)(s[k] + i) = sv[k];
    }
};
template <typename U>
__device__ __forceinline__ StateStreams<2, U> two_streams(float* m, float* v, U u) { return {{m, v}, false, u}; }
template <bool MOM, typename U>
__device__ __forceinline__ StateStreams<MOM ? 1 : 0, U> one_stream(float* buf, bool skip_load, U u) { return {{buf}, skip_load, u}; }

struct AdamGroups { float lr[4]; float wd[4]; float step_size[4]; };

// The HF rule inside the chunk frame: what tvts_adamw_hf and tvts_adamw_hf_guarded share.  COEF: the gradient is also multiplied by
// the clip coefficient norm_coef[1] (1 with a null norm_coef), AFTER grad_scale: g = fl(fl(stored g * grad_scale) * coef), the order
// the header states for the torch rules' gradient; a coefficient of exactly 1.0f leaves the bits of the launch without one.  GUARD:
// the frame tests norm_coef[0] in front of every load.
template <bool COEF, bool GUARD>
__device__ __forceinline__ void hf_chunk(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                         float* __restrict__ v, bf16* __restrict__ shadow,
                                         const unsigned char* __restrict__ chunk_group, AdamGroups& hp, float beta1, float beta2,
                                         float omb1, float omb2, float eps, float grad_scale, const int* __restrict__ step_dev,
                                         const float* __restrict__ hyper_dev, double beta1d, double beta2d,
                                         const float* __restrict__ norm_coef) {
    optim_chunk<4, false, GUARD>(p, g, shadow, chunk_group, nullptr, 0.f, 0.f, norm_coef, [&](int grp) {
        if (hyper_dev) {  // lr[4] | wd[4] in device memory: a captured launch follows the LR schedule without re-capture
            hp.lr[grp] = hyper_dev[grp];
            hp.wd[grp] = hyper_dev[4 + grp];
        }
        if (step_dev) {  // step counter lives in device memory (hipGraph replay): bias correction computed here
            const double st = (double)step_dev[0];
            // the betas in double, as the host path has them: both paths then produce the same step size bit for bit (with the
            // float betas the step differed by 8e-6 relative, enough to flip a few dozen bf16 shadow roundings per step)
            const double bc1 = 1.0 - pow(beta1d, st), bc2 = 1.0 - pow(beta2d, st);
            hp.step_size[grp] = (float)((double)hp.lr[grp] * sqrt(bc2) / bc1);
        }
        const float lr = hp.lr[grp], wd = hp.wd[grp], ss = hp.step_size[grp];
        const float coef = COEF && norm_coef ? norm_coef[1] : 1.f;
        return two_streams(m, v, [=](f32x4& pv, f32x4& mv, f32x4& vv, const f32x4& gv) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float gg = gv[e] * grad_scale;
                if constexpr (COEF) gg *= coef;
                mv[e] = beta1 * mv[e] + omb1 * gg;
                vv[e] = beta2 * vv[e] + omb2 * gg * gg;
                pv[e] -= ss * mv[e] / (sqrtf(vv[e]) + eps);
                if (wd > 0.f) pv[e] -= lr * wd * pv[e];
            }
        });
    });
}

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, bf16* __restrict__ shadow,
                                                    const unsigned char* __restrict__ chunk_group, AdamGroups hp, float beta1,
                                                    float beta2, float omb1, float omb2, float eps, float grad_scale,
                                                    const int* __restrict__ step_dev, const float* __restrict__ hyper_dev,
                                                    double beta1d, double beta2d) {
    hf_chunk<false, false>(p, g, m, v, shadow, chunk_group, hp, beta1, beta2, omb1, omb2, eps, grad_scale, step_dev, hyper_dev, beta1d,
                           beta2d, nullptr);
}
template <bool GUARD>
__global__ __launch_bounds__(256) void adamw_hf_coef_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, bf16* __restrict__ shadow,
                                                            const unsigned char* __restrict__ chunk_group, AdamGroups hp, float beta1,
                                                            float beta2, float omb1, float omb2, float eps, float grad_scale,
                                                            const int* __restrict__ step_dev, const float* __restrict__ hyper_dev,
                                                            double beta1d, double beta2d, const float* __restrict__ norm_coef) {
    hf_chunk<true, GUARD>(p, g, m, v, shadow, chunk_group, hp, beta1, beta2, omb1, omb2, eps, grad_scale, step_dev, hyper_dev, beta1d,
                          beta2d, norm_coef);
}

// lr / wd of the four groups and the host's step sizes (the kernel forms its own when it reads the step counter from the device)
static AdamGroups hf_groups(const float* lr4, const float* wd4, int step, double beta1, double beta2) {
    if (step <= 0) step = 1;
    AdamGroups hp;
    const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
    for (int i = 0; i < 4; ++i) {
        hp.lr[i] = lr4[i];
        hp.wd[i] = wd4[i];
        hp.step_size[i] = (float)((double)lr4[i] * sqrt(bc2) / bc1);
    }
    return hp;
}

extern "C" int tvts_adamw_hf(float* p, const float* g, float* m, float* v, void* shadow_bf16,
                             const unsigned char* chunk_group, int nchunks, const float* lr4, const float* wd4, int step,
                             const int* step_dev, const float* hyper_dev, double beta1, double beta2, double eps,
                             float grad_scale, hipStream_t stream) {
    if (nchunks <= 0 || (step <= 0 && !step_dev)) return TVTS_EINVAL;
    if (hyper_dev && !step_dev) return TVTS_EINVAL;  // the device table is only consulted together with the device step counter
    const AdamGroups hp = hf_groups(lr4, wd4, step, beta1, beta2);
    hipLaunchKernelGGL(adamw_kernel, dim3(nchunks), dim3(256), 0, stream, p, g, m, v, (bf16*)shadow_bf16, chunk_group, hp,
                       (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, grad_scale, step_dev, hyper_dev, beta1, beta2);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---- what the two torch rules share on the host
// The overflow guard of the v1 fine-tuning step (FinetuneStep(skip_nonfinite=True)): GradScaler's "skip the update on inf / NaN"
// decided on the device.  The decision is isfinite(norm_coef[0]), the global norm tvts_grad_sumsq left in device memory.  Two
// launches: guard_advance_kernel (one lane) advances step_dev[0] on a finite norm and skipped[0] otherwise, then the guarded
// instantiation of the rule runs -- with the step counter it would have had unguarded, or returning in every block.  A skipped
// call leaves step_dev where it was: the bias corrections and SGD's first-update rule go on as if step() had not been called.
__global__ void guard_advance_kernel(const float* __restrict__ norm_coef, int* __restrict__ step_dev, long* __restrict__ skipped) {
    if (finite_f32(norm_coef[0])) step_dev[0] += 1;
    else skipped[0] += 1;
}
static inline bool misaligned16(const void* q) { return ((uintptr_t)q & 15) != 0; }
// The refusals of tvts_adamw_torch / tvts_sgd_torch.  streams: p, g and the state streams the launch touches -- each present and
// 16-byte aligned.  ema (null: no average), shadow (null: none) and norm_coef (null: no coefficient) are optional; skipped (null:
// unguarded) makes step_dev and norm_coef required and the host `step` irrelevant.
static bool torch_args_bad(std::initializer_list<const void*> streams, const float* ema, const void* shadow,
                           const unsigned char* chunk_group, int nchunks, const float* hyper_dev, int step, const int* step_dev,
                           const float* norm_coef, const long* skipped, bool momentum, int nesterov) {
    for (const void* q : streams)
        if (!q || misaligned16(q)) return true;
    if (!chunk_group || !hyper_dev || nchunks <= 0) return true;
    if (misaligned16(ema) || ((uintptr_t)shadow & 7) || ((uintptr_t)skipped & 7) || ((uintptr_t)step_dev & 3) || ((uintptr_t)norm_coef & 3))
        return true;
    if (skipped ? (!step_dev || !norm_coef) : (step <= 0 && !step_dev)) return true;
    return nesterov && !momentum;  // torch: "Nesterov momentum requires a momentum and zero dampening"
}
// a run-time choice as a compile-time one: f(std::true_type) or f(std::false_type)
template <typename F>
static void with_bool(bool b, F f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// ---- the HF rule of the pretraining step with the clip coefficient and the guard (StepRunner(clip_grad=..., skip_nonfinite=True))
// The arguments of tvts_adamw_hf, then norm_coef (null: no coefficient) and skipped (null: unguarded).  g = stored gradient *
// grad_scale * norm_coef[1], multiplied in that order; norm_coef null or a coefficient of 1.0f: the bits of tvts_adamw_hf.  Under the
// guard the counter kernel runs in front, the bias corrections come from step_dev[0] (the device code tvts_adamw_hf runs with a
// step_dev: same bits) and `step` is ignored.  Refusals as the torch rules': p, g, m, v present and 16-byte aligned, and so on.
extern "C" int tvts_adamw_hf_guarded(float* p, const float* g, float* m, float* v, void* shadow_bf16, const unsigned char* chunk_group,
                                     int nchunks, const float* lr4, const float* wd4, int step, int* step_dev, const float* hyper_dev,
                                     double beta1, double beta2, double eps, float grad_scale, const float* norm_coef, long* skipped,
                                     hipStream_t stream) {
    for (const void* q : {(const void*)p, (const void*)g, (const void*)m, (const void*)v})
        if (!q || misaligned16(q)) return TVTS_EINVAL;
    if (!chunk_group || !lr4 || !wd4 || nchunks <= 0) return TVTS_EINVAL;
    if (((uintptr_t)shadow_bf16 & 7) || ((uintptr_t)skipped & 7) || ((uintptr_t)step_dev & 3) || ((uintptr_t)norm_coef & 3) ||
        ((uintptr_t)hyper_dev & 3))
        return TVTS_EINVAL;
    if (skipped ? (!step_dev || !norm_coef) : (step <= 0 && !step_dev)) return TVTS_EINVAL;
    if (hyper_dev && !step_dev) return TVTS_EINVAL;  // (as tvts_adamw_hf: the device table goes with the device step counter)
    const AdamGroups hp = hf_groups(lr4, wd4, step, beta1, beta2);
    if (skipped) hipLaunchKernelGGL(guard_advance_kernel, dim3(1), dim3(1), 0, stream, norm_coef, step_dev, skipped);
    with_bool(skipped != nullptr, [&](auto G) {
        hipLaunchKernelGGL(adamw_hf_coef_kernel<decltype(G)::value>, dim3(nchunks), dim3(256), 0, stream, p, g, m, v,
                           (bf16*)shadow_bf16, chunk_group, hp, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2),
                           (float)eps, grad_scale, (const int*)step_dev, hyper_dev, beta1, beta2, norm_coef);
    });
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---- torch.optim.AdamW, multi-tensor (the v1 fine-tuning step)
// The optimizer run_class_finetuning.py builds through optim_factory.create_optimizer (opt "adamw") over the layer-decay parameter
// groups (28 of them on ViT-B).  Per element, in torch's order (torch/optim/adamw.py, single-tensor form):
//     p  *= 1 - lr wd                                   (the factor formed in double, rounded once)
//     m   = b1 m + (1 - b1) g
//     v   = b2 v + (1 - b2) g g
//     p  -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)  (lr / bc1 and sqrt(bc2) formed in double, rounded once each)
// with bc1 = 1 - b1^t, bc2 = 1 - b2^t in double from the double betas; t = step_dev[0] when given, else the host's `step` -- the
// same device code either way, so both give the same bits.  g = stored gradient * grad_scale * norm_coef[1] (the clip coefficient
// tvts_grad_sumsq left in device memory; no coefficient when norm_coef is null).  hyper_dev: lr[64] | wd[64] in device memory.
// Chunk table as tvts_adamw_hf (1024 elements per chunk, one group byte each); a chunk of group >= 64 (255 = frozen) keeps every bit.
template <bool EMA, bool GUARD>
__global__ __launch_bounds__(256) void adamw_torch_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, bf16* __restrict__ shadow,
                                                          const unsigned char* __restrict__ chunk_group,
                                                          const float* __restrict__ hyper_dev, int step,
                                                          const int* __restrict__ step_dev, double beta1d, double beta2d, float beta1,
                                                          float beta2, float omb1, float omb2, float eps, float grad_scale,
                                                          const float* __restrict__ norm_coef, float* __restrict__ ema, float d32,
                                                          float o32) {
#pragma clang fp contract(off)  // (lexical: it holds inside both lambdas; adamw_kernel has none and keeps its contractions)
    optim_chunk<64, EMA, GUARD>(p, g, shadow, chunk_group, ema, d32, o32, norm_coef, [&](int grp) {
        const float lr = hyper_dev[grp], wd = hyper_dev[64 + grp];
        const double st = (double)(step_dev ? step_dev[0] : step);
        const double bc1 = 1.0 - pow(beta1d, st), bc2 = 1.0 - pow(beta2d, st);
        const float decay = (float)(1.0 - (double)lr * (double)wd);
        const float ss = (float)((double)lr / bc1), rs = (float)sqrt(bc2);
        const float gs = norm_coef ? grad_scale * norm_coef[1] : grad_scale;
        return two_streams(m, v, [=](f32x4& pv, f32x4& mv, f32x4& vv, const f32x4& gv) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float gg = gv[e] * gs;
                pv[e] *= decay;
                mv[e] = beta1 * mv[e] + omb1 * gg;
                vv[e] = beta2 * vv[e] + omb2 * gg * gg;
                pv[e] -= ss * mv[e] / (sqrtf(vv[e]) / rs + eps);
            }
        });
    });
}
extern "C" int tvts_adamw_torch(float* p, const float* g, float* m, float* v, void* shadow_bf16, const unsigned char* chunk_group,
                                int nchunks, const float* hyper_dev, int step, int* step_dev, double beta1, double beta2, double eps,
                                float grad_scale, const float* norm_coef, float* ema, float d32, float o32, long* skipped,
                                hipStream_t stream) {
    if (torch_args_bad({p, g, m, v}, ema, shadow_bf16, chunk_group, nchunks, hyper_dev, step, step_dev, norm_coef, skipped, false, 0))
        return TVTS_EINVAL;
    if (skipped) hipLaunchKernelGGL(guard_advance_kernel, dim3(1), dim3(1), 0, stream, norm_coef, step_dev, skipped);
    with_bool(ema != nullptr, [&](auto E) {
        with_bool(skipped != nullptr, [&](auto G) {
            hipLaunchKernelGGL((adamw_torch_kernel<decltype(E)::value, decltype(G)::value>), dim3(nchunks), dim3(256), 0, stream, p, g,
                               m, v, (bf16*)shadow_bf16, chunk_group, hyper_dev, step, step_dev, beta1, beta2, (float)beta1,
                               (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, grad_scale, norm_coef, ema, d32,
                               o32);
        });
    });
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ModelEma.update as a pass of its own (12 B per element): the chunk gate of tvts_adamw_torch (a chunk of group >= 64, 255 =
// frozen / padding, keeps every bit of its average) and the rule of the fused launch.
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p,
                                                         const unsigned char* __restrict__ chunk_group, float d32, float o32) {
    if (chunk_group[blockIdx.x] >= 64) return;
    const size_t i = (size_t)blockIdx.x * 1024 + threadIdx.x * 4;
    *(f32x4*)(ema + i) = ema_rule4(*(const f32x4*)(ema + i), *(const f32x4*)(p + i), d32, o32);
}
extern "C" int tvts_ema_update(float* ema, const float* p, const unsigned char* chunk_group, int nchunks, float d32, float o32,
                               hipStream_t stream) {
    if (!ema || !p || !chunk_group || nchunks <= 0 || misaligned16(ema) || misaligned16(p)) return TVTS_EINVAL;
    hipLaunchKernelGGL(ema_update_kernel, dim3(nchunks), dim3(256), 0, stream, ema, p, chunk_group, d32, o32);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---- torch.optim.SGD, multi-tensor (the v1 linear probe: v1/scripts/linear_ssv2.sh, --opt sgd --lr 0.1 --momentum 0.9)
// The optimizer optim_factory.create_optimizer builds for "sgd" / "nesterov" (nesterov=True) and "momentum" (optim_factory.py:121-126),
// in the single-tensor form of torch/optim/sgd.py with dampening 0.  Every add(x, alpha=a) of that form is ONE fused multiply-add in
// ATen, so per element (fmaf = one rounding; lr, wd, mu the fp32 roundings of the group's lr / weight_decay and of momentum):
//     gg = g * gs                                    gs as tvts_adamw_torch forms it
//     d  = wd != 0 ? fmaf(wd, p, gg) : gg            d_p.add(param, alpha=weight_decay)
//     mu != 0:  buf = first update ? d : fl(mu * buf) + d      clone(d_p) -- the bits of d -- / buf.mul_(mu).add_(d_p): two roundings
//               d   = nesterov ? fmaf(mu, buf, d) : buf
//     p  = fmaf(-lr, d, p)                           param.add_(d_p, alpha=-lr)
// The step counter (step_dev[0] when given, else `step`: the same device code) only says whether this is the first update, t == 1:
// buf is then written and not read.  MOM = false (momentum 0): buf is neither read nor written.  Under the guard a skipped call 1
// leaves step_dev at 0, so the next call is the first update.
template <bool MOM, bool EMA, bool GUARD>
__global__ __launch_bounds__(256) void sgd_torch_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                        bf16* __restrict__ shadow, const unsigned char* __restrict__ chunk_group,
                                                        const float* __restrict__ hyper_dev, int step,
                                                        const int* __restrict__ step_dev, float mu, int nesterov, float grad_scale,
                                                        const float* __restrict__ norm_coef, float* __restrict__ ema, float d32,
                                                        float o32) {
#pragma clang fp contract(off)  // (the FMAs below are explicit calls; fl(mu * buf) + d must stay two roundings)
    optim_chunk<64, EMA, GUARD>(p, g, shadow, chunk_group, ema, d32, o32, norm_coef, [&](int grp) {
        const float lr = hyper_dev[grp], wd = hyper_dev[64 + grp];
        const bool first = (step_dev ? step_dev[0] : step) == 1;
        const float gs = norm_coef ? grad_scale * norm_coef[1] : grad_scale;
        const float nlr = -lr;
        return one_stream<MOM>(buf, first, [=](f32x4& pv, f32x4& bv, const f32x4& gv) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float gg = gv[e] * gs;
                float d = wd != 0.f ? __builtin_fmaf(wd, pv[e], gg) : gg;
                if constexpr (MOM) {
                    float b = d;
                    if (!first) {
                        const float mb = mu * bv[e];
                        b = mb + d;
                    }
                    bv[e] = b;
                    d = nesterov ? __builtin_fmaf(mu, b, d) : b;
                }
                pv[e] = __builtin_fmaf(nlr, d, pv[e]);
            }
        });
    });
}
extern "C" int tvts_sgd_torch(float* p, const float* g, float* buf, void* shadow_bf16, const unsigned char* chunk_group, int nchunks,
                              const float* hyper_dev, int step, int* step_dev, double momentum, int nesterov, float grad_scale,
                              const float* norm_coef, float* ema, float d32, float o32, long* skipped, hipStream_t stream) {
    const float mu = (float)momentum;
    const bool mom = mu != 0.f;
    if (torch_args_bad({p, g, mom ? buf : p /* momentum 0: buf is no stream of this launch */}, ema, shadow_bf16, chunk_group, nchunks, hyper_dev, step, step_dev, norm_coef, skipped, mom,
                       nesterov))
        return TVTS_EINVAL;
    if (skipped) hipLaunchKernelGGL(guard_advance_kernel, dim3(1), dim3(1), 0, stream, norm_coef, step_dev, skipped);
    with_bool(mom, [&](auto M) {
        with_bool(ema != nullptr, [&](auto E) {
            with_bool(skipped != nullptr, [&](auto G) {
                hipLaunchKernelGGL((sgd_torch_kernel<decltype(M)::value, decltype(E)::value, decltype(G)::value>), dim3(nchunks),
                                   dim3(256), 0, stream, p, g, buf, (bf16*)shadow_bf16, chunk_group, hyper_dev, step, step_dev, mu,
                                   nesterov ? 1 : 0, grad_scale, norm_coef, ema, d32, o32);
            });
        });
    });
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// a[i] <-> b[i] in place, shadow[i] = bf16(new a[i]): the masters and the average change places for an evaluation, no third buffer.
// Every element is read and written by one lane only, so the exchange needs no order between lanes.
__global__ __launch_bounds__(256) void swap_shadow_kernel(float* __restrict__ a, float* __restrict__ b, bf16* __restrict__ shadow,
                                                          size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const f32x4 av = *(const f32x4*)(a + i * 4), bv = *(const f32x4*)(b + i * 4);
        *(f32x4*)(a + i * 4) = bv;
        *(f32x4*)(b + i * 4) = av;
        *(bf16x4*)(shadow + i * 4) = (bf16x4){(bf16)bv[0], (bf16)bv[1], (bf16)bv[2], (bf16)bv[3]};
    }
}
extern "C" int tvts_swap_f32_shadow(float* a, float* b, void* shadow_bf16, long n, hipStream_t stream) {
    if (!a || !b || !shadow_bf16 || n <= 0 || n % 4 || misaligned16(a) || misaligned16(b) || ((uintptr_t)shadow_bf16 & 7))
        return TVTS_EINVAL;
    if (a < b ? a + n > b : b + n > a) return TVTS_EINVAL;  // overlapping buffers
    const size_t n4 = (size_t)n / 4;
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(swap_shadow_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a, b, (bf16*)shadow_bf16, n4);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

__global__ __launch_bounds__(256) void cast_kernel(const float* __restrict__ src, bf16* __restrict__ dst, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const f32x4 v = *(const f32x4*)(src + i * 4);
        *(bf16x4*)(dst + i * 4) = (bf16x4){(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
    }
}
__global__ __launch_bounds__(256) void widen_kernel(const bf16* __restrict__ src, float* __restrict__ dst, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const bf16x4 v = *(const bf16x4*)(src + i * 4);
        *(f32x4*)(dst + i * 4) = (f32x4){(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    }
}
// bf16 -> fp32 (the bf16 gradient payload read back into the fp32 gradient buffer after its all-reduce)
extern "C" int tvts_cast_bf16_f32(const void* src, float* dst, long n, hipStream_t stream) {
    if (n <= 0 || n % 4) return TVTS_EINVAL;
    const size_t n4 = (size_t)n / 4;
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(widen_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const bf16*)src, dst, n4);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
extern "C" int tvts_cast_f32_bf16(const float* src, void* dst, long n, hipStream_t stream) {
    if (n <= 0 || n % 4) return TVTS_EINVAL;
    const size_t n4 = (size_t)n / 4;
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(cast_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, src, (bf16*)dst, n4);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// tile table entry: {src_off, dst_off (elements, as two int32 halves each), R, C, tile_r, tile_c}
struct TrTile { long long src_off, dst_off; int R, C, tr, tc; };

__global__ __launch_bounds__(256) void transpose_batched_kernel(const bf16* __restrict__ src, bf16* __restrict__ dst,
                                                                const TrTile* __restrict__ tiles) {
    __shared__ __attribute__((aligned(16))) bf16 t[64][72];  // 144-byte rows: 16-byte stores stay aligned, column reads spread over the banks
    const TrTile e = tiles[blockIdx.x];
    const bf16* s = src + e.src_off;
    bf16* d = dst + e.dst_off;
    const int r0 = e.tr * 64, c0 = e.tc * 64;
    if (e.R % 8 == 0 && e.C % 8 == 0 && e.src_off % 8 == 0 && e.dst_off % 8 == 0) {
        // 16 bytes per lane on both sides (2-byte accesses ran this kernel at a third of the HBM rate: 1.8 ms for the 0.63 G bf16
        // weights of ViT-H/14): a lane loads 8 consecutive columns of a row, and stores 8 consecutive rows of a column
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = threadIdx.x + 256 * k, r = i >> 3, c8 = (i & 7) * 8;
            if (r0 + r < e.R && c0 + c8 < e.C) *(bf16x8*)&t[r][c8] = *(const bf16x8*)(s + (size_t)(r0 + r) * e.C + c0 + c8);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = threadIdx.x + 256 * k, c = i >> 3, r8 = (i & 7) * 8;
            if (c0 + c < e.C && r0 + r8 < e.R) {
                bf16x8 v;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = t[r8 + j][c];
                *(bf16x8*)(d + (size_t)(c0 + c) * e.R + r0 + r8) = v;
            }
        }
        return;
    }
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int r = i >> 6, c = i & 63;
        if (r0 + r < e.R && c0 + c < e.C) t[r][c] = s[(size_t)(r0 + r) * e.C + c0 + c];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int c = i >> 6, r = i & 63;
        if (r0 + r < e.R && c0 + c < e.C) d[(size_t)(c0 + c) * e.R + r0 + r] = t[r][c];
    }
}
extern "C" int tvts_transpose_bf16_batched(const void* src, void* dst, const void* tiles, int ntiles, hipStream_t stream) {
    if (ntiles <= 0) return TVTS_EINVAL;
    hipLaunchKernelGGL(transpose_batched_kernel, dim3(ntiles), dim3(256), 0, stream, (const bf16*)src, (bf16*)dst,
                       (const TrTile*)tiles);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// Zero-padded bf16 row copy: dst[r, 0:cols_pad] = src[r, 0:cols] | 0.  The H/14 patch-embedding weight ([W, 588]) gets
// its K padded to 640 this way so the MFMA GEMM's 64-wide K loop and 16-byte row alignment hold.
__global__ __launch_bounds__(256) void pad_rows_kernel(const bf16* __restrict__ src, int lds_, bf16* __restrict__ dst, int ldd,
                                                       int cols, int cols_pad) {
    const int r = blockIdx.x;
    for (int c = threadIdx.x; c < cols_pad; c += 256)
        dst[(size_t)r * ldd + c] = c < cols ? src[(size_t)r * lds_ + c] : (bf16)0.f;
}
extern "C" int tvts_pad_rows_bf16(const void* src, int ld_src, void* dst, int ld_dst, int rows, int cols, int cols_pad,
                                  hipStream_t stream) {
    if (rows <= 0 || cols <= 0 || cols_pad < cols || ld_dst < cols_pad || ld_src < cols) return TVTS_EINVAL;
    hipLaunchKernelGGL(pad_rows_kernel, dim3(rows), dim3(256), 0, stream, (const bf16*)src, ld_src, (bf16*)dst, ld_dst, cols,
                       cols_pad);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
// dst[r, c] += src[r, c] for c < cols (fp32, independent row strides): folds the padded wgrad scratch back into the
// [W, 588] gradient of the patch-embedding weight.
__global__ __launch_bounds__(256) void add_rows_kernel(float* __restrict__ dst, int ldd, const float* __restrict__ src, int lds_,
                                                       int cols) {
    const int r = blockIdx.x;
    for (int c = threadIdx.x; c < cols; c += 256) dst[(size_t)r * ldd + c] += src[(size_t)r * lds_ + c];
}
extern "C" int tvts_add_rows_f32(float* dst, int ld_dst, const float* src, int ld_src, int rows, int cols,
                                 hipStream_t stream) {
    if (rows <= 0 || cols <= 0 || ld_dst < cols || ld_src < cols) return TVTS_EINVAL;
    hipLaunchKernelGGL(add_rows_kernel, dim3(rows), dim3(256), 0, stream, dst, ld_dst, src, ld_src, cols);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---- fp8 (OCP e4m3) quantisation with one scale per tensor: scale = amax / 448, q = rne(x / scale), |q| <= 448
//      (the weight / activation format of tvts_gemm_nt_fp8; torch.float8_e4m3fn bit patterns)
// 16 bytes per lane and access: 8 bf16 or 4 fp32 (cols % 8 == 0 resp. % 4, rows 16-byte aligned)
template <typename T> struct Vec16;
template <> struct Vec16<bf16> { typedef bf16x8 V; static constexpr int N = 8; };
template <> struct Vec16<float> { typedef f32x4 V; static constexpr int N = 4; };

template <typename T>
__global__ __launch_bounds__(256) void amax_kernel(const T* __restrict__ x, long ld, int rows, int cols, float* __restrict__ amax) {
    typedef typename Vec16<T>::V V;
    constexpr int N = Vec16<T>::N;
    float m = 0.f;
    for (long r = blockIdx.x; r < rows; r += gridDim.x)
        for (int c = threadIdx.x * N; c < cols; c += 256 * N) {
            const V v = *(const V*)(x + r * ld + c);
#pragma unroll
            for (int e = 0; e < N; ++e) m = fmaxf(m, fabsf((float)v[e]));
        }
    __shared__ float wm[4];
    m = block_max_256(m, wm);
    if (threadIdx.x == 0)  // one atomic per block (every wave hammering the single address serialises the whole kernel)
        atomicMax((unsigned*)amax, __float_as_uint(m));  // non-negative floats order like their bits
}
template <typename T>
__global__ __launch_bounds__(256) void quant_fp8_kernel(const T* __restrict__ x, long ld, int rows, int cols,
                                                        const float* __restrict__ amax, unsigned char* __restrict__ out, long ldo,
                                                        float* __restrict__ scale_out) {
    typedef typename Vec16<T>::V V;
    constexpr int N = Vec16<T>::N;
    const float am = amax[0];
    const float scale = am > 0.f ? am / 448.0f : 1.0f;
    const float inv = 1.0f / scale;
    if (blockIdx.x == 0 && threadIdx.x == 0 && scale_out) scale_out[0] = scale;
    for (long r = blockIdx.x; r < rows; r += gridDim.x)
        for (int c = threadIdx.x * N; c < cols; c += 256 * N) {
            const V v = *(const V*)(x + r * ld + c);
            int pk[N / 4];
#pragma unroll
            for (int h = 0; h < N / 4; ++h)
                pk[h] = pack4_e4m3((float)v[h * 4], (float)v[h * 4 + 1], (float)v[h * 4 + 2], (float)v[h * 4 + 3], inv);
            if (N == 8) *(long*)(out + r * ldo + c) = ((long)(unsigned)pk[N / 4 - 1] << 32) | (unsigned)pk[0];
            else *(int*)(out + r * ldo + c) = pk[0];
        }
}
static __global__ void zero1_kernel(float* p) { *p = 0.f; }
extern "C" int tvts_amax(const void* x, int is_f32, long ld, int rows, int cols, float* amax, hipStream_t stream) {
    if (rows <= 0 || cols <= 0 || cols % (is_f32 ? 4 : 8) || ld % (is_f32 ? 4 : 8) || !x || !amax) return TVTS_EINVAL;
    if (rows > 1 && ld < cols) return TVTS_EINVAL;  // overlapping rows
    hipLaunchKernelGGL(zero1_kernel, dim3(1), dim3(1), 0, stream, amax);  // a kernel, not a memset node (see attention.hip)
    const int blocks = rows < 1024 ? rows : 1024;
    if (is_f32) hipLaunchKernelGGL(amax_kernel<float>, dim3(blocks), dim3(256), 0, stream, (const float*)x, ld, rows, cols, amax);
    else hipLaunchKernelGGL(amax_kernel<bf16>, dim3(blocks), dim3(256), 0, stream, (const bf16*)x, ld, rows, cols, amax);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
extern "C" int tvts_quant_fp8(const void* x, int is_f32, long ld, int rows, int cols, const float* amax, void* out, long ldo,
                              float* scale_out, hipStream_t stream) {
    if (rows <= 0 || cols <= 0 || cols % (is_f32 ? 4 : 8) || ldo % 8 || ld % (is_f32 ? 4 : 8) || !x || !amax || !out) return TVTS_EINVAL;
    if (rows > 1 && (ld < cols || ldo < cols)) return TVTS_EINVAL;  // overlapping rows
    const int blocks = rows < 2048 ? rows : 2048;
    if (is_f32) hipLaunchKernelGGL(quant_fp8_kernel<float>, dim3(blocks), dim3(256), 0, stream, (const float*)x, ld, rows, cols, amax,
                                   (unsigned char*)out, ldo, scale_out);
    else hipLaunchKernelGGL(quant_fp8_kernel<bf16>, dim3(blocks), dim3(256), 0, stream, (const bf16*)x, ld, rows, cols, amax,
                            (unsigned char*)out, ldo, scale_out);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---- all weights of the fp8 path in three launches (was 3-4 launches per weight, 224 weights on ViT-H/14): one table entry per
//      weight -- fp32 master [rows, cols] (contiguous), its e4m3 copy, optionally the bf16 TRANSPOSED shadow [cols, rows] and its
//      e4m3 copy (the input-gradient operand), amax / scale scalars.  Pass 1 zeroes the amax scalars, pass 2 takes max |w| of the
//      master (blocks x tensors, one atomicMax per block), pass 3 converts both copies under the one scale (a bf16 rounding past
//      the master's amax saturates at +-448).  Same bit patterns as tvts_amax + tvts_quant_fp8 per tensor.
struct Q8Desc {
    const float* w; unsigned char* q; const bf16* wt; unsigned char* qt; float* amax; float* scale; float* scale_t;
    int rows, cols;
};
__global__ void q8_multi_zero_kernel(const Q8Desc* __restrict__ tab, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) *tab[i].amax = 0.f;
}
__global__ __launch_bounds__(256) void q8_multi_amax_kernel(const Q8Desc* __restrict__ tab) {
    const Q8Desc d = tab[blockIdx.y];
    const long n4 = (long)d.rows * d.cols / 4;
    float m = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 v = *(const f32x4*)(d.w + i * 4);
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
    }
    __shared__ float wm[4];
    m = block_max_256(m, wm);
    if (threadIdx.x == 0) atomicMax((unsigned*)d.amax, __float_as_uint(m));
}
__global__ __launch_bounds__(256) void q8_multi_quant_kernel(const Q8Desc* __restrict__ tab) {
    const Q8Desc d = tab[blockIdx.y];
    const float am = *d.amax;
    const float scale = am > 0.f ? am / 448.0f : 1.0f;
    const float inv = 1.0f / scale;
    if (blockIdx.x == 0 && threadIdx.x == 0) { *d.scale = scale; if (d.scale_t) *d.scale_t = scale; }
    const long n4 = (long)d.rows * d.cols / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 v = *(const f32x4*)(d.w + i * 4);
        *(int*)(d.q + i * 4) = pack4_e4m3(v[0], v[1], v[2], v[3], inv);
        if (d.wt) {
            const bf16x4 t = *(const bf16x4*)(d.wt + i * 4);
            *(int*)(d.qt + i * 4) = pack4_e4m3((float)t[0], (float)t[1], (float)t[2], (float)t[3], inv);
        }
    }
}
extern "C" int tvts_quant_fp8_multi(const void* table, int n, hipStream_t stream) {
    if (!table || n <= 0) return TVTS_EINVAL;
    hipLaunchKernelGGL(q8_multi_zero_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const Q8Desc*)table, n);
    hipLaunchKernelGGL(q8_multi_amax_kernel, dim3(32, n), dim3(256), 0, stream, (const Q8Desc*)table);
    hipLaunchKernelGGL(q8_multi_quant_kernel, dim3(32, n), dim3(256), 0, stream, (const Q8Desc*)table);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---- activations: ONE scale per row (token), amax and conversion in a single pass.  A wave owns a row: it is read once into
//      registers (rows up to 5120 columns; wider rows are read a second time, from cache), reduced to its amax with wave
//      shuffles, scaled by 448 / amax and written as e4m3 bytes + the row's scale.  3 bytes of traffic per element instead of
//      the 5 of tvts_amax + tvts_quant_fp8, and a tighter scale than one amax for the whole tensor.
__global__ __launch_bounds__(256) void quant_fp8_rows_kernel(const bf16* __restrict__ x, long ld, int rows, int cols,
                                                             unsigned char* __restrict__ out, long ldo, float* __restrict__ row_scale,
                                                             const float* __restrict__ tscale, float* __restrict__ amax_acc) {
    constexpr int MAXV = 10;  // 10 x 64 lanes x 8 bf16 = 5120 columns held in registers
    const int lane = threadIdx.x & 63;
    const long wave0 = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
    const bool in_regs = cols <= MAXV * 512;
    float run_amax = 0.f;
    for (long r = wave0; r < rows; r += nwaves) {
        const bf16* xr = x + r * ld;
        bf16x8 v[MAXV];
        float m = 0.f;
        if (in_regs) {
#pragma unroll
            for (int t = 0; t < MAXV; ++t) {
                const int c = (t * 64 + lane) * 8;
                if (c < cols) {
                    v[t] = *(const bf16x8*)(xr + c);
#pragma unroll
                    for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf((float)v[t][e]));
                }
            }
        } else {
            for (int c = lane * 8; c < cols; c += 512) {
                const bf16x8 u = *(const bf16x8*)(xr + c);
#pragma unroll
                for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf((float)u[e]));
            }
        }
        m = wave_max(m);
        run_amax = fmaxf(run_amax, m);
        const float scale = q8_scale(tscale, m);
        const float inv = 1.0f / scale;
        if (lane == 0 && row_scale) row_scale[r] = scale;
        unsigned char* orow = out + r * ldo;
        auto emit = [&](const bf16x8& u, int c) {
            const int lo = pack4_e4m3((float)u[0], (float)u[1], (float)u[2], (float)u[3], inv);
            const int hi = pack4_e4m3((float)u[4], (float)u[5], (float)u[6], (float)u[7], inv);
            *(long*)(orow + c) = ((long)(unsigned)hi << 32) | (unsigned)lo;
        };
        if (in_regs) {
#pragma unroll
            for (int t = 0; t < MAXV; ++t) {
                const int c = (t * 64 + lane) * 8;
                if (c < cols) emit(v[t], c);
            }
        } else {
            for (int c = lane * 8; c < cols; c += 512) emit(*(const bf16x8*)(xr + c), c);
        }
    }
    amax_publish(amax_acc, run_amax, lane);
}
// next step's scales from this step's amax values, for n tensors at once: scale[i] = amax[i] / 448 (unchanged while amax[i] == 0:
// a tensor that was not produced this step keeps its scale), amax[i] = 0.  A scale slot never stays 0: a tensor whose maximum was 0
// in the calibration step (the time branch's attention output under the reference's zero-initialised timeattn.qkv) gets the scale
// 1.0 -- the value q8_scale() quantises under when it meets a zero scale -- so that producer and consumers agree (the GEMMs
// dequantise with the slot's value: a raw 0 there would force the tensor's products to zero for one step)
__global__ void fp8_update_scales_kernel(float* __restrict__ amax, float* __restrict__ scale, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float a = amax[i];
    if (a > 0.f) scale[i] = a / 448.0f;
    else if (!(scale[i] > 0.f)) scale[i] = 1.0f;
    amax[i] = 0.f;
}
extern "C" int tvts_fp8_update_scales(float* amax, float* scale, int n, hipStream_t stream) {
    if (n <= 0 || !amax || !scale) return TVTS_EINVAL;
    hipLaunchKernelGGL(fp8_update_scales_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, stream, amax, scale, n);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
// The update under the overflow guard of the pretraining step (StepRunner(skip_nonfinite=True)): a maximum that is not finite never
// becomes a scale.  Per slot: a finite amax > 0 gives scale = amax / 448, anything else (0, -0, inf, NaN) keeps the old scale; a
// slot whose scale is then not finite and positive -- it has never had a usable maximum: the calibration step was the bad one, or
// amax / 448 underflowed -- gets 1.0, the value q8_scale() quantises under at a zero scale; amax = 0 in every case.  guard_norm
// (optional): the step's global gradient norm on the device; when it is not finite the step is one the optimizer skips, and every
// slot keeps its old scale (the 1.0 rule still holds), so a skipped step leaves the scales of the step before it.
__global__ void fp8_update_scales_guarded_kernel(float* __restrict__ amax, float* __restrict__ scale, int n,
                                                 const float* __restrict__ guard_norm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float a = amax[i];
    float s = scale[i];
    if (finite_f32(a) && a > 0.f && (!guard_norm || finite_f32(guard_norm[0]))) s = a / 448.0f;
    if (!(finite_f32(s) && s > 0.f)) s = 1.0f;
    scale[i] = s;
    amax[i] = 0.f;
}
extern "C" int tvts_fp8_update_scales_guarded(float* amax, float* scale, int n, const float* guard_norm, hipStream_t stream) {
    if (n <= 0 || !amax || !scale || ((uintptr_t)guard_norm & 3)) return TVTS_EINVAL;
    hipLaunchKernelGGL(fp8_update_scales_guarded_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, stream, amax, scale, n, guard_norm);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
extern "C" int tvts_quant_fp8_rows(const void* x, long ld, int rows, int cols, void* out, long ldo, float* row_scale,
                                   const float* tscale, float* amax_acc, hipStream_t stream) {
    if (rows <= 0 || cols <= 0 || cols % 8 || ld % 8 || ldo % 8 || !x || !out || (!row_scale && !tscale)) return TVTS_EINVAL;
    if (rows > 1 && (ld < cols || ldo < cols)) return TVTS_EINVAL;  // overlapping rows
    const long want = ((long)rows + 3) / 4;
    const int blocks = (int)(want < 8192 ? want : 8192);
    hipLaunchKernelGGL(quant_fp8_rows_kernel, dim3(blocks), dim3(256), 0, stream, (const bf16*)x, ld, rows, cols,
                       (unsigned char*)out, ldo, row_scale, tscale, amax_acc);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// probe used by tests: what does ds_read_b64_tr_b16 return?  in: 16 x 64 bf16 row-major tile (row stride 160 B in LDS)
__global__ void probe_tr16_kernel(const bf16* __restrict__ in, bf16* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) char tile[16 * 160];
    const int lane = threadIdx.x;
    for (int c = lane; c < 16 * 8; c += 64) *(bf16x8*)(tile + (c >> 3) * 160 + (c & 7) * 16) = *(const bf16x8*)(in + (c >> 3) * 64 + (c & 7) * 8);
    __syncthreads();
    const int gq = lane >> 4, i = lane & 15;
    const char* p = tile + (gq * 4 + (i >> 2)) * 160 + (i & 3) * 8;
    const s16x4 t = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))p);
    const bf16x4 tb = __builtin_bit_cast(bf16x4, t);
    for (int e = 0; e < 4; ++e) out[lane * 4 + e] = tb[e];
}
extern "C" int tvts_probe_tr16(const void* in, void* out, hipStream_t stream) {
    hipLaunchKernelGGL(probe_tr16_kernel, dim3(1), dim3(64), 0, stream, (const bf16*)in, (bf16*)out);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
