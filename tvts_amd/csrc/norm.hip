// LayerNorm forward / backward for the residual stream (HBM-bound; one wave64 per row, 4 or 8 columns per lane).
//
// forward : y = (x - mean) * rstd * gamma + beta, x fp32 or bf16 (optionally gathered rows; the hybrid stream's CLS rows from an
//           fp32 side array), y bf16 or fp32 and / or an e4m3 copy; mean / rstd are saved for the backward pass.
// backward: dx = rstd * (g - mean(g) - xhat * mean(g * xhat)) [+ res1 + res2],  g = dy * gamma
//           res1 fp32 or bf16 (the residual-stream gradient), res2 bf16 (a side-branch gradient that only exists as a GEMM
//           operand anyway); dx fp32 and / or a bf16 copy that feeds the next MFMA GEMM; dgamma / dbeta accumulated
//           from per-block partial sums: written to a workspace and combined by a second tiny kernel (or, without
//           a workspace, one fp32 atomic per column per block).
// Reference: nn.LayerNorm as used at v2/model/video_encoder_ViT_B_16.py:79-85 (eps 1e-5, fp32) and
// v2/model/sort_transformer.py:99 (eps 1e-6).
#include "common.h"
#include <type_traits>

#define LN_MAX_IT 5  // 5 * 256 = 1280 columns max

template <typename T>
__device__ __forceinline__ f32x4 load4(const T* p);
template <>
__device__ __forceinline__ f32x4 load4<float>(const float* p) { return *(const f32x4*)p; }
template <>
__device__ __forceinline__ f32x4 load4<bf16>(const bf16* p) {
    const bf16x4 v = *(const bf16x4*)p;
    return (f32x4){(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
__device__ __forceinline__ void store4(float* p, f32x4 v) { *(f32x4*)p = v; }
__device__ __forceinline__ void store4(bf16* p, f32x4 v) {
    *(bf16x4*)p = (bf16x4){(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
}
// the stored form of 4 columns of a row in flight, widened where it is used
template <typename T> struct RawDy;
template <> struct RawDy<float> { typedef f32x4 T; };
template <> struct RawDy<bf16> { typedef bf16x4 T; };
__device__ __forceinline__ f32x4 widen(f32x4 v) { return v; }
__device__ __forceinline__ f32x4 widen(bf16x4 v) { return (f32x4){(float)v[0], (float)v[1], (float)v[2], (float)v[3]}; }

// ================================================================================================================================
// Forward: one kernel frame over a column-group policy.  A lane owns C consecutive columns of every group of 64 * C columns, H = C / 4
// pieces of 4; the policy says how a group is kept while its row is in flight (Raw), widened to fp32 pieces, stored, and turned into
// the e4m3 copy (Kept: the bf16-rounded outputs between the amax sweep and the conversion sweep).  The loads of lanes past the row's
// end are unconditional and their values zeroed afterwards: by widen() in the 8-column form (zeroed in the branch that issues the
// loads, that branch waits for them and no row is in flight during the reductions), by keep() as they arrive in the 4-column form,
// whose fp32 kernels have always done so and keep their registers that way (120 at 5 trips: four waves per SIMD).
// Row<G>, the G groups of a row in flight, is a plain array for 4 columns and the same array inside a struct for 8: what each
// kernel had before they shared this frame, and what hipcc's register allocation turns out to depend on -- a struct costs the fp32
// forms 5 % at W = 768 (138 -> 144 us at 150 720 rows; 134 registers at 5 trips in one variant), a plain array costs the 8-column
// CLS forms 8 - 14 registers, a wave per SIMD for three of the six (profiles/r21_layernorm_frame_registers.txt).
//   LnCols4<TX>: fp32 or bf16 rows in 4-column pieces.  Every fp32 row, and the bf16 rows that LnCols8 cannot take.
//   LnCols8    : bf16 rows in 16-byte pieces (W and every pitch % 8 == 0).  The 4-column form moves a bf16 row in 8-byte pieces: as
//                many memory instructions as an fp32 row at half the bytes, and the kernel is bound by REQUESTS, not bytes (127-134 ->
//                93-95 us at 150 720 x 768).  The backward built the same way measured SLOWER than its 4-column kernels (four input
//                streams of two rows in flight need 180-200 registers): it has no 8-column form.
// ================================================================================================================================
template <typename TX_>
struct LnCols4 {
    typedef TX_ TX;
    static constexpr int C = 4, H = 1;
    typedef typename RawDy<TX>::T Raw;
    template <int G> using Row = Raw[G];
    typedef f32x4 Kept;
    static __device__ __forceinline__ Raw keep(const Raw& t, bool in_row) { return in_row ? t : Raw{}; }
    static __device__ __forceinline__ void widen(const Raw& t, bool, f32x4 (&v)[1]) { v[0] = ::widen(t); }
    template <typename T>
    static __device__ __forceinline__ void store(T* p, const f32x4 (&o)[1], const Kept&) { store4(p, o[0]); }
    static __device__ __forceinline__ Kept rounded(const f32x4 (&o)[1]) {
        return (f32x4){(float)(bf16)o[0][0], (float)(bf16)o[0][1], (float)(bf16)o[0][2], (float)(bf16)o[0][3]};
    }
    static __device__ __forceinline__ float amax(const Kept& k, float am) {
#pragma unroll
        for (int e = 0; e < 4; ++e) am = fmaxf(am, fabsf(k[e]));
        return am;
    }
    static __device__ __forceinline__ void pack(unsigned char* p, const Kept& k, float inv) {
        *(int*)p = pack4_e4m3(k[0], k[1], k[2], k[3], inv);
    }
};
struct LnCols8 {
    typedef bf16 TX;
    static constexpr int C = 8, H = 2;
    typedef bf16x8 Raw;
    template <int G> struct Row {
        Raw raw[G];
        __device__ __forceinline__ Raw& operator[](int g) { return raw[g]; }
    };
    typedef bf16x8 Kept;
    static __device__ __forceinline__ Raw keep(const Raw& t, bool) { return t; }
    static __device__ __forceinline__ void widen(const Raw& t, bool in_row, f32x4 (&v)[2]) {
        v[0] = in_row ? (f32x4){(float)t[0], (float)t[1], (float)t[2], (float)t[3]} : (f32x4){0, 0, 0, 0};
        v[1] = in_row ? (f32x4){(float)t[4], (float)t[5], (float)t[6], (float)t[7]} : (f32x4){0, 0, 0, 0};
    }
    static __device__ __forceinline__ Kept rounded(const f32x4 (&o)[2]) {
        return (bf16x8){(bf16)o[0][0], (bf16)o[0][1], (bf16)o[0][2], (bf16)o[0][3], (bf16)o[1][0], (bf16)o[1][1], (bf16)o[1][2], (bf16)o[1][3]};
    }
    static __device__ __forceinline__ void store(bf16* p, const f32x4 (&)[2], const Kept& k) { *(bf16x8*)p = k; }
    static __device__ __forceinline__ float amax(const Kept& k, float am) {
#pragma unroll
        for (int e = 0; e < 8; ++e) am = fmaxf(am, fabsf((float)k[e]));
        return am;
    }
    static __device__ __forceinline__ void pack(unsigned char* p, const Kept& k, float inv) {
        typedef __attribute__((ext_vector_type(2))) int i32x2;
        *(i32x2*)p = (i32x2){pack4_e4m3((float)k[0], (float)k[1], (float)k[2], (float)k[3], inv),
                             pack4_e4m3((float)k[4], (float)k[5], (float)k[6], (float)k[7], inv)};
    }
};

// Forward and backward kernels are templated on their trip count (G = ceil(W / (64 * C)), IT = ceil(W / 256): register arrays sized
// to the row, no dead iterations) and walk their rows in a grid-stride loop with the NEXT row's loads issued before the current
// row's reductions: a wave always has two rows of traffic in flight instead of one load -> reduce -> store round trip at a time.
// Q8: additionally write the row as OCP e4m3 bytes with ONE scale per row (amax of the bf16-rounded outputs / 448) or the tensor's
// scale: the fp8 operand of the next GEMM (BASELINE config 4) leaves the LayerNorm that produced it, bit-identical to
// tvts_quant_fp8_rows run on y, without another pass over the activation.  In the 8-column form y may then be NULL -- under
// per-tensor scales every consumer of a space-time block's LayerNorm output multiplies the e4m3 bytes (forward GEMM and weight
// gradient), the bf16 tensor would be written and never read.
// CLS: cls_x / cls_period (the hybrid residual stream, round 5): row r with r % cls_period == 0 is the CLS token of clip
// r / cls_period; its value is carried in fp32 in the compact side array cls_x[M / cls_period][W] and read from THERE when the row
// is used (the stream's own row r is stale and is not loaded), and x_refresh row r receives its rounding, so that every later
// reader of the stream (the residual epilogues, the backward) sees the exact value rounded once instead of an accumulated bf16 sum
template <typename P, typename TO, int G, bool Q8, bool CLS>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const typename P::TX* __restrict__ x, int ldx, const int* __restrict__ rows,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float eps, int M, int W, TO* __restrict__ y, int ldy,
                                                     float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                     unsigned char* __restrict__ q8, int ldq, float* __restrict__ row_scale,
                                                     const float* __restrict__ tscale, float* __restrict__ amax_acc,
                                                     const float* __restrict__ cls_x, int cls_period, typename P::TX* x_refresh) {
    typedef typename P::Raw Raw;
    constexpr int C = P::C, H = P::H;
    constexpr bool Y_OPT = Q8 && C == 8;  // the e4m3-only output exists in the 8-column form alone
    const int lane = threadIdx.x & 63;
    const int stride = gridDim.x * 4;
    int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    float run_amax = 0.f;
    f32x4 gm[G][H], bt[G][H];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int h = 0; h < H; ++h) {
            const int c = lane * C + g * 64 * C + h * 4;
            gm[g][h] = c < W ? load4<float>(gamma + c) : (f32x4){0, 0, 0, 0};
            bt[g][h] = c < W ? load4<float>(beta + c) : (f32x4){0, 0, 0, 0};
        }
    const float invW = 1.0f / (float)W;
    // a row in flight, and whether it is a CLS row (wave-uniform: a wave owns the row)
    typedef typename P::template Row<G> Row;
    auto load_row = [&](int rr, Row& w, bool& cls) {
        cls = CLS && rr % cls_period == 0;
        if (cls) return;  // (its value comes from the fp32 side array where it is used)
        const typename P::TX* xp = x + (size_t)(rows ? rows[rr] : rr) * ldx;
#pragma unroll
        for (int g = 0; g < G; ++g) {  // (unconditional loads, zeroed afterwards: see ln_bwd_kernel)
            const int c = lane * C + g * 64 * C;
            w[g] = P::keep(*(const Raw*)(xp + (c < W ? c : 0)), c < W);
        }
    };
    Row cur, nxt;
    bool cur_cls, nxt_cls;
    load_row(r, cur, cur_cls);
    for (; r < M; r += stride) {
        const bool more = r + stride < M;
        if (more) load_row(r + stride, nxt, nxt_cls);
        f32x4 v[G][H];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int c = lane * C + g * 64 * C;
            if (CLS && cur_cls) {
                const float* cp = cls_x + (size_t)(r / cls_period) * W + c;
#pragma unroll
                for (int h = 0; h < H; ++h) v[g][h] = (f32x4){0, 0, 0, 0};
                if (c < W) {
#pragma unroll
                    for (int h = 0; h < H; ++h) v[g][h] = load4<float>(cp + h * 4);
                }
            } else {
                P::widen(cur[g], c < W, v[g]);
            }
        }
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int h = 0; h < H; ++h) s += v[g][h][0] + v[g][h][1] + v[g][h][2] + v[g][h][3];
        const float mean = wave_sum(s) * invW;
        float q = 0.f;
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (lane * C + g * 64 * C < W) {
#pragma unroll
                for (int h = 0; h < H; ++h)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float d = v[g][h][e] - mean;
                        q += d * d;
                    }
            }
        const float rstd = rsqrtf(wave_sum(q) * invW + eps);
        const bool refresh = CLS && cur_cls && x_refresh;
        typename P::Kept ob[Q8 ? G : 1];
        float am = 0.f;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int c = lane * C + g * 64 * C;
            if (c < W) {
                f32x4 o[H];
#pragma unroll
                for (int h = 0; h < H; ++h)
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[h][e] = (v[g][h][e] - mean) * rstd * gm[g][h][e] + bt[g][h][e];
                const typename P::Kept k = P::rounded(o);  // the values the bf16 consumer sees
                if (!Y_OPT || y) P::store(y + (size_t)r * ldy + c, o, k);
                if (refresh) P::store(x_refresh + (size_t)r * ldx + c, v[g], P::rounded(v[g]));
                if (Q8) {
                    ob[g] = k;
                    am = P::amax(k, am);
                }
            }
        }
        if (Q8) {
            am = wave_max(am);
            run_amax = fmaxf(run_amax, am);
            const float scale = q8_scale(tscale, am);
            const float inv = 1.0f / scale;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int c = lane * C + g * 64 * C;
                if (c < W) P::pack(q8 + (size_t)r * ldq + c, ob[g], inv);
            }
            if (lane == 0 && row_scale) row_scale[r] = scale;
        }
        if (lane == 0) {
            if (mean_out) mean_out[r] = mean;
            if (rstd_out) rstd_out[r] = rstd;
        }
        if (more) {
#pragma unroll
            for (int g = 0; g < G; ++g) cur[g] = nxt[g];
            cur_cls = nxt_cls;
        }
    }
    if (Q8) amax_publish(amax_acc, run_amax, lane);
}

// ---- host: what every entry point refuses.  A matrix has rows of at least W elements (a shorter pitch makes rows overlap: silently
// wrong results, or accesses past the buffer) in whole 4-element groups; the e4m3 copy comes with a row or a tensor scale; dgamma
// and dbeta come together or not at all (the kernel accumulates both behind one test)
static inline bool ln_shape_bad(int M, int W) { return M <= 0 || W <= 0 || W % 4 || W > 256 * LN_MAX_IT; }
static inline bool ln_mat_bad(const void* p, int ld, int W) { return !p || ld % 4 || ld < W; }
static inline bool ln_opt_bad(const void* p, int ld, int W) { return p && ln_mat_bad(p, ld, W); }
static inline bool ln_q8_bad(const void* q8, int ldq, int W, const float* row_scale, const float* tscale) {
    return q8 && (ln_mat_bad(q8, ldq, W) || (!row_scale && !tscale));
}
static inline bool ln_cls_bad(int M, int cls_period) { return cls_period <= 0 || M % cls_period; }
static inline bool ln_grads_bad(const float* dgamma, const float* dbeta, long workspace_elems) {
    return (dgamma == nullptr) != (dbeta == nullptr) || workspace_elems < 0;
}

struct LnFwdArgs {
    const void* x; int ldx; bool x_bf16; const int* rows; const float *gamma, *beta; float eps; int M, W;
    void* y; int ldy; bool y_f32; float *mean, *rstd;
    unsigned char* q8 = nullptr; int ldq = 0; float* row_scale = nullptr; const float* tscale = nullptr; float* amax_acc = nullptr;
    const float* cls_x = nullptr; int cls_period = 0; void* x_refresh = nullptr;
};
// the 8-column form: bf16 rows with W and the pitch of everything it touches in whole 8-element groups
static inline bool ln_cols8(const LnFwdArgs& a) {
    return a.x_bf16 && a.W % 8 == 0 && a.ldx % 8 == 0 && (!a.y || a.ldy % 8 == 0) && (!a.q8 || a.ldq % 8 == 0);
}
static bool ln_fwd_bad(const LnFwdArgs& a) {
    return ln_shape_bad(a.M, a.W) || ln_mat_bad(a.x, a.ldx, a.W) || !a.gamma || !a.beta || a.ldy % 4 || ln_opt_bad(a.y, a.ldy, a.W) ||
           ln_q8_bad(a.q8, a.ldq, a.W, a.row_scale, a.tscale) || (!a.y && !(a.q8 && ln_cols8(a)));  // e4m3-only: the 8-column form
}

// the one launch site: the instantiation with G = ceil(W / (64 * C)) groups, as far as a legal W needs them
template <typename P, typename TO, bool Q8, bool CLS, int G = 1>
static void ln_fwd_launch(const LnFwdArgs& a, hipStream_t stream) {
    if constexpr ((G - 1) * 64 * P::C < 256 * LN_MAX_IT) {
        if (a.W > G * 64 * P::C) return ln_fwd_launch<P, TO, Q8, CLS, G + 1>(a, stream);
        int blocks = ceil_div(a.M, 4);
        if (blocks > 2048) blocks = 2048;  // 8 blocks x 4 waves per CU, two rows in flight per wave
        typedef typename P::TX TX;
        hipLaunchKernelGGL((ln_fwd_kernel<P, TO, G, Q8, CLS>), dim3(blocks), dim3(256), 0, stream, (const TX*)a.x, a.ldx, a.rows, a.gamma,
                           a.beta, a.eps, a.M, a.W, (TO*)a.y, a.ldy, a.mean, a.rstd, a.q8, a.ldq, a.row_scale, a.tscale, a.amax_acc,
                           a.cls_x, a.cls_period, (TX*)a.x_refresh);
    }
}
// the forward forms: bf16 rows -> bf16 with or without the e4m3 copy and the CLS side array, 8 columns per lane where the pitches
// allow; fp32 rows -> bf16 (with or without the copy) or fp32
static void launch_ln_fwd(const LnFwdArgs& a, hipStream_t stream) {
    const bool q8 = a.q8, cls = a.cls_x;
    if (ln_cols8(a)) {
        if (q8 && cls) ln_fwd_launch<LnCols8, bf16, true, true>(a, stream);
        else if (q8) ln_fwd_launch<LnCols8, bf16, true, false>(a, stream);
        else if (cls) ln_fwd_launch<LnCols8, bf16, false, true>(a, stream);
        else ln_fwd_launch<LnCols8, bf16, false, false>(a, stream);
    } else if (a.x_bf16) {
        if (q8 && cls) ln_fwd_launch<LnCols4<bf16>, bf16, true, true>(a, stream);
        else if (q8) ln_fwd_launch<LnCols4<bf16>, bf16, true, false>(a, stream);
        else if (cls) ln_fwd_launch<LnCols4<bf16>, bf16, false, true>(a, stream);
        else ln_fwd_launch<LnCols4<bf16>, bf16, false, false>(a, stream);
    } else {
        if (q8) ln_fwd_launch<LnCols4<float>, bf16, true, false>(a, stream);
        else if (a.y_f32) ln_fwd_launch<LnCols4<float>, float, false, false>(a, stream);
        else ln_fwd_launch<LnCols4<float>, bf16, false, false>(a, stream);
    }
}

// x: the fp32 residual stream, or (x_bf16) a side-branch value that only this LayerNorm consumes and that is therefore
// kept in bf16 (the time residual of the space-time block: the space branch restarts from the block input).
extern "C" int tvts_layernorm_fwd(const void* x, int ldx, int x_bf16, const int* rows, const float* gamma, const float* beta,
                                  float eps, int M, int W, void* y, int ldy, int y_f32, float* mean, float* rstd,
                                  hipStream_t stream) {
    const LnFwdArgs a{x, ldx, x_bf16 != 0, rows, gamma, beta, eps, M, W, y, ldy, y_f32 != 0, mean, rstd};
    if (ln_fwd_bad(a) || (x_bf16 && y_f32)) return TVTS_EINVAL;
    launch_ln_fwd(a, stream);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// LayerNorm forward that also emits the e4m3 copy of its bf16 output with per-row scales or the tensor's (see Q8 above)
extern "C" int tvts_layernorm_fwd_fp8(const void* x, int ldx, int x_bf16, const int* rows, const float* gamma, const float* beta,
                                      float eps, int M, int W, void* y, int ldy, void* q8, int ldq, float* row_scale,
                                      const float* tscale, float* amax_acc, float* mean, float* rstd, hipStream_t stream) {
    const LnFwdArgs a{x, ldx, x_bf16 != 0, rows, gamma, beta, eps, M, W, y, ldy, false, mean, rstd,
                      (unsigned char*)q8, ldq, row_scale, tscale, amax_acc};
    if (ln_fwd_bad(a) || !q8) return TVTS_EINVAL;
    launch_ln_fwd(a, stream);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// The hybrid residual stream (round 5): the stream is bf16, the CLS token's row of every clip -- the row the video embedding is read
// from, and the one row whose rounding error reaches every other token through the attention -- is carried in fp32 in a compact side
// array.  x bf16 [M, W] (rows r % cls_period == 0 stale), cls_x fp32 [M / cls_period, W]; those rows are normalised from cls_x and
// x_refresh (normally x itself; optional) receives their bf16 rounding.  q8 (optional) as in tvts_layernorm_fwd_fp8.
extern "C" int tvts_layernorm_fwd_cls(const void* x, int ldx, const float* cls_x, int cls_period, void* x_refresh, const float* gamma,
                                      const float* beta, float eps, int M, int W, void* y, int ldy, void* q8, int ldq, float* row_scale,
                                      const float* tscale, float* amax_acc, float* mean, float* rstd, hipStream_t stream) {
    const LnFwdArgs a{x, ldx, true, nullptr, gamma, beta, eps, M, W, y, ldy, false, mean, rstd,
                      (unsigned char*)q8, ldq, row_scale, tscale, amax_acc, cls_x, cls_period, x_refresh};
    if (ln_fwd_bad(a) || !cls_x || ln_cls_bad(M, cls_period)) return TVTS_EINVAL;
    launch_ln_fwd(a, stream);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ================================================================================================================================
// Backward
// ================================================================================================================================
// Q8: additionally write the bf16 copy of dx as OCP e4m3 bytes with one scale per row (amax of the bf16-rounded values / 448) -- the
// output gradient of the e4m3 input-gradient GEMM that consumes dx_bf16 (same bytes as tvts_quant_fp8_rows of dx_bf16)
// blocks per CU of a variant (launch bound and persistent grid): rows of <= 768 columns 3 with a residual input, else 4; wider rows 2
// with a residual input or with a second row in flight (all-bf16 streams), else 3
template <typename TDY, int IT, bool R1, bool R2, typename TX, typename TR1>
constexpr int ln_bwd_per_cu() {
    return IT <= 3 ? ((R1 || R2) ? 3 : 4)
                   : ((R1 || R2 || (sizeof(TDY) == 2 && sizeof(TX) == 2 && (!R1 || sizeof(TR1) == 2))) ? 2 : 3);
}
template <typename TDY, int IT, bool R1, bool R2, typename TX = float, bool Q8 = false, typename TR1 = float, bool CLS = false>
__global__ __launch_bounds__(256, (ln_bwd_per_cu<TDY, IT, R1, R2, TX, TR1>())) void ln_bwd_kernel(const TDY* __restrict__ dy, int lddy, const TX* __restrict__ x,
                                                        int ldx, const int* __restrict__ rows,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        const float* __restrict__ gamma, const TR1* __restrict__ res1,
                                                        const bf16* __restrict__ res2, int ldr2, int ldr, int M, int W,
                                                        float* __restrict__ dx, int lddx, bf16* __restrict__ dx_bf16,
                                                        int lddxb, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                        float* __restrict__ partial,
                                                        unsigned char* __restrict__ q8 = nullptr, int ldq = 0,
                                                        float* __restrict__ row_scale = nullptr,
                                                        const float* __restrict__ tscale = nullptr, float* __restrict__ amax_acc = nullptr,
                                                        const float* __restrict__ cls_x = nullptr, const float* __restrict__ cls_res1 = nullptr,
                                                        float* __restrict__ cls_dx = nullptr, int cls_period = 0) {
    // CLS (the hybrid residual stream): this instantiation walks ONLY the rows r % cls_period == 0, behind a plain launch that has
    // done every row (and dgamma / dbeta): for them the LayerNorm input comes from cls_x (fp32, what the forward normalised), the
    // residual-stream gradient res1 from cls_res1 (fp32) instead of the bf16 stream row, and the result -- which replaces the
    // plain launch's in dx_bf16 (and q8) -- is ALSO stored in fp32 to cls_dx: the CLS token's gradient chain never passes through
    // a bf16 rounding.  (One kernel for both kinds of rows ran the 784 other rows of a clip at half speed: 14 spilled registers.)
    typedef typename RawDy<TDY>::T DyV;
    // a row in flight keeps its inputs in their STORED type (bf16 rows: 2 registers per 4 columns instead of 4) and is widened where it
    // is used; the CLS instantiation reads fp32 side rows and keeps f32x4
    typedef typename std::conditional<CLS, f32x4, typename RawDy<TX>::T>::type XV;
    typedef typename std::conditional<CLS, f32x4, typename RawDy<TR1>::T>::type R1V;
    constexpr bool ALL16 = sizeof(TDY) == 2 && sizeof(TX) == 2 && (!R1 || sizeof(TR1) == 2);
    float run_amax = 0.f;
    __shared__ float red[2][4][IT * 256];  // [gamma|beta][wave][column slot]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x4 ag[IT], ab[IT], gm[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        ag[it] = (f32x4){0, 0, 0, 0};
        ab[it] = (f32x4){0, 0, 0, 0};
        const int c = lane * 4 + it * 256;
        gm[it] = c < W ? load4<float>(gamma + c) : (f32x4){0, 0, 0, 0};
    }
    const float invW = 1.0f / (float)W;
    const int stride = gridDim.x * 4 * (CLS ? cls_period : 1);
    struct Row { XV x[IT]; DyV d[IT]; R1V r1[R1 ? IT : 1]; bf16x4 r2[R2 ? IT : 1]; float mu, rs; int xr; };
    auto load_row = [&](int rr, Row& w) {
        w.xr = rows ? rows[rr] : rr;
        w.mu = mean[rr];
        w.rs = rstd[rr];
        const bool cls = CLS;
        const size_t ci = cls ? (size_t)(rr / cls_period) * W : 0;
        // UNCONDITIONAL loads (lanes past the row's end re-read its first columns -- always inside the row; their values are never used): inside `if (c < W)`
        // every column group is a basic block of its own, and hipcc's wait-count pass, which must assume that a group may have been
        // skipped, makes each group wait for the loads of the one before it -- IT dependent round trips per row instead of one
        // (the 1280-wide H/14 forms streamed 3.0 - 3.6 TB/s where the 768-wide ones stream ~5)
        // The all-bf16 forms only: with fp32 streams every load in flight at once needs more registers than the launch bounds leave
        // (24 - 40 spilled, and a spill reload in this loop waits for the prefetched row).
        constexpr bool UNCOND = ALL16 && !CLS;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int c0 = lane * 4 + it * 256, c = c0 < W ? c0 : 0;
            if (UNCOND || c0 < W) {
                if constexpr (CLS) {
                    w.x[it] = cls_x ? load4<float>(cls_x + ci + c) : load4<TX>(x + (size_t)w.xr * ldx + c);
                    if (R1) w.r1[it] = cls_res1 ? load4<float>(cls_res1 + ci + c) : load4<TR1>(res1 + (size_t)w.xr * ldr + c);
                } else {
                    w.x[it] = *(const XV*)(x + (size_t)w.xr * ldx + c);
                    if (R1) w.r1[it] = *(const R1V*)(res1 + (size_t)w.xr * ldr + c);
                }
                w.d[it] = *(const DyV*)(dy + (size_t)rr * lddy + c);
                if (R2) w.r2[it] = *(const bf16x4*)(res2 + (size_t)w.xr * ldr2 + c);
            }
        }
    };
    // a second row in flight: rows of <= 768 columns always; the wider rows (1024, 1280 columns) when every input stream is bf16 (the
    // hybrid stream's forms: 40 instead of 60 - 80 registers per row in flight).  Without it a wave runs load -> reduce -> store round
    // trips one at a time at 8 - 12 waves per CU: the H/14 backward forms streamed 3.0 - 3.6 TB/s where the B/16 forms stream ~5
    constexpr bool PF = !CLS && (IT <= 3 || ALL16);
    int r = (blockIdx.x * 4 + wave) * (CLS ? cls_period : 1);
    Row cur, nxt;
    if (PF && r < M) load_row(r, cur);
    for (; r < M; r += stride) {
        const bool more = PF && r + stride < M;
        if (PF) { if (more) load_row(r + stride, nxt); }
        else load_row(r, cur);
        f32x4 xh[IT], g[IT];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int c = lane * 4 + it * 256;
            if (c < W) {
                const f32x4 d = widen(cur.d[it]), xv = widen(cur.x[it]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    xh[it][e] = (xv[e] - cur.mu) * cur.rs;
                    g[it][e] = d[e] * gm[it][e];
                    s1 += g[it][e];
                    s2 += g[it][e] * xh[it][e];
                    ag[it][e] += d[e] * xh[it][e];
                    ab[it][e] += d[e];
                }
            }
        }
        const float c1 = wave_sum(s1) * invW, c2 = wave_sum(s2) * invW;
        // Q8: the row's outputs are needed twice (amax, then conversion).  The residual forms keep a copy (their launch bound leaves the
        // registers; recomputing keeps the residual registers live through the second sweep: 246 -> 316 us at W = 1280), the
        // residual-free forms recompute (a copy spills at their tighter bound: 130 -> 200 us)
        constexpr bool KEEP = Q8 && (R1 || R2);
        f32x4 ob[KEEP ? IT : 1];
        float am = 0.f;
        auto out_of = [&](int it) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = cur.rs * (g[it][e] - c1 - xh[it][e] * c2);
            if (R1) o += widen(cur.r1[it]);
            if (R2) o += widen(cur.r2[it]);
            return o;
        };
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int c = lane * 4 + it * 256;
            if (c < W) {
                const f32x4 o = out_of(it);
                if (dx) store4(dx + (size_t)cur.xr * lddx + c, o);
                if (dx_bf16) store4(dx_bf16 + (size_t)cur.xr * lddxb + c, o);
                if (CLS && cls_dx) store4(cls_dx + (size_t)(r / cls_period) * W + c, o);
                if (Q8) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = (float)(bf16)o[e];  // the value the bf16 consumers see
                        if (KEEP) ob[it][e] = v;
                        am = fmaxf(am, fabsf(v));
                    }
                }
            }
        }
        if (Q8) {  // second sweep over the kept copy or the recomputed outputs
            am = wave_max(am);
            // the plain launch of tvts_layernorm_bwd_cls (cls_period given, not CLS): its results on the CLS rows are replaced by the
            // CLS launch behind it and were formed from the stream's own rows there -- they are no part of the tensor whose maximum
            // amax_acc collects
            if (CLS || cls_period == 0 || r % cls_period != 0) run_amax = fmaxf(run_amax, am);
            const float scale = q8_scale(tscale, am);
            const float inv = 1.0f / scale;
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int c = lane * 4 + it * 256;
                if (c < W) {
                    f32x4 o;
                    if (KEEP) o = ob[it];
                    else o = out_of(it);
                    *(int*)(q8 + (size_t)cur.xr * ldq + c) =
                        pack4_e4m3((float)(bf16)o[0], (float)(bf16)o[1], (float)(bf16)o[2], (float)(bf16)o[3], inv);
                }
            }
            if (lane == 0 && row_scale) row_scale[cur.xr] = scale;
        }
        if (more) cur = nxt;
    }
    if (Q8) amax_publish(amax_acc, run_amax, lane);
    if (!dgamma) return;
    // block reduce the per-wave partials, then one atomic per column per block
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            red[0][wave][(it * 4 + e) * 64 + lane] = ag[it][e];
            red[1][wave][(it * 4 + e) * 64 + lane] = ab[it][e];
        }
    __syncthreads();
    for (int idx = threadIdx.x; idx < IT * 4 * 64; idx += 256) {
        const int l = idx & 63, ie = idx >> 6;
        const int c = l * 4 + (ie >> 2) * 256 + (ie & 3);
        if (c < W) {
            const float sg = red[0][0][idx] + red[0][1][idx] + red[0][2][idx] + red[0][3][idx];
            const float sb = red[1][0][idx] + red[1][1][idx] + red[1][2][idx] + red[1][3][idx];
            if (partial) {  // per-block partial sums, combined by ln_dgamma_reduce_kernel (plain stores, deterministic)
                partial[((size_t)blockIdx.x * 2 + 0) * W + c] = sg;
                partial[((size_t)blockIdx.x * 2 + 1) * W + c] = sb;
            } else {        // no workspace: one atomic per column per block
                atomicAdd(dgamma + c, sg);
                atomicAdd(dbeta + c, sb);
            }
        }
    }
}

// dgamma[c] += sum_b partial[b][0][c], dbeta[c] += sum_b partial[b][1][c]
__global__ __launch_bounds__(1024) void ln_dgamma_reduce_kernel(const float* __restrict__ partial, int nblocks, int W,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta) {
    // 64 columns x 16 row-groups per block: each thread sums nblocks / 16 partials with 8 independent loads in flight
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;
    const int k = blockIdx.y;
    __shared__ float acc[16][64];
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c < W) {
        int b = part;
        for (; b + 7 * 16 < nblocks; b += 8 * 16) {
#pragma unroll
            for (int u = 0; u < 8; ++u) s[u] += partial[((size_t)(b + u * 16) * 2 + k) * W + c];
        }
        for (; b < nblocks; b += 16) s[0] += partial[((size_t)b * 2 + k) * W + c];
    }
    acc[part][threadIdx.x & 63] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    __syncthreads();
    if (part == 0 && c < W) {
        float t = 0.f;
#pragma unroll
        for (int p = 0; p < 16; ++p) t += acc[p][threadIdx.x];
        float* dst = k == 0 ? dgamma : dbeta;
        dst[c] += t;
    }
}

// the backward's arguments as the entry points give them.  The types of dy / x / res1 choose the instantiation (ln_bwd_dispatch);
// the CLS launch of tvts_layernorm_bwd_cls is the plain launch's struct with cls = true and the side arrays
struct LnBwdArgs {
    const void* dy; int lddy; bool dy_f32; const void* x; int ldx; bool x_bf16; const int* rows;
    const float *mean, *rstd, *gamma; const void* res1; bool res1_bf16; int ldr; const bf16* res2; int ldr2; int M, W;
    float* dx; int lddx; bf16* dxb; int lddxb; float *dgamma, *dbeta, *ws; long ws_elems;
    unsigned char* q8 = nullptr; int ldq = 0; float* row_scale = nullptr; const float* tscale = nullptr; float* amax_acc = nullptr;
    int cls_period = 0; bool cls = false; const float *cls_x = nullptr, *cls_res1 = nullptr; float* cls_dx = nullptr;
};
static bool ln_bwd_bad(const LnBwdArgs& a) {
    return ln_shape_bad(a.M, a.W) || ln_mat_bad(a.dy, a.lddy, a.W) || ln_mat_bad(a.x, a.ldx, a.W) || !a.mean || !a.rstd || !a.gamma ||
           ln_opt_bad(a.res1, a.ldr, a.W) || ln_opt_bad(a.res2, a.ldr2, a.W) || (!a.dx && !a.dxb) || ln_opt_bad(a.dx, a.lddx, a.W) ||
           ln_opt_bad(a.dxb, a.lddxb, a.W) || ln_q8_bad(a.q8, a.ldq, a.W, a.row_scale, a.tscale) ||
           ln_grads_bad(a.dgamma, a.dbeta, a.ws_elems);
}

// the one launch site of the backward: persistent grid, workspace or atomics, the dgamma / dbeta reduction behind it
template <typename TDY, bool R1, bool R2, typename TX, bool Q8, typename TR1, bool CLS>
static void launch_ln_bwd(const LnBwdArgs& a, hipStream_t stream) {
    const int it = ceil_div(a.W, 256);
    // as many blocks per CU as the variant's registers allow (see __launch_bounds__ above)
    const int per_cu = it <= 3 ? ln_bwd_per_cu<TDY, 3, R1, R2, TX, TR1>() : ln_bwd_per_cu<TDY, 5, R1, R2, TX, TR1>();
    int blocks = ceil_div(CLS ? a.M / a.cls_period : a.M, 4);
    if (blocks > 256 * per_cu) blocks = 256 * per_cu;
    const dim3 grid(blocks);
    // (CLS: the plain launch in front of this one has accumulated dgamma / dbeta over every row)
    float *dgamma = CLS ? nullptr : a.dgamma, *dbeta = CLS ? nullptr : a.dbeta;
    float* partial = (dgamma && a.ws && a.ws_elems >= (long)blocks * 2 * a.W) ? a.ws : nullptr;
#define LN_BWD_CASE(N) case N: hipLaunchKernelGGL((ln_bwd_kernel<TDY, N, R1, R2, TX, Q8, TR1, CLS>), grid, dim3(256), 0, stream, (const TDY*)a.dy, a.lddy, (const TX*)a.x, a.ldx, a.rows, a.mean, a.rstd, a.gamma, (const TR1*)a.res1, a.res2, a.ldr2, a.ldr, a.M, a.W, a.dx, a.lddx, a.dxb, a.lddxb, dgamma, dbeta, partial, a.q8, a.ldq, a.row_scale, a.tscale, a.amax_acc, a.cls_x, a.cls_res1, a.cls_dx, a.cls_period); break;
    switch (it) { LN_BWD_CASE(1) LN_BWD_CASE(2) LN_BWD_CASE(3) LN_BWD_CASE(4) default: LN_BWD_CASE(5) }
#undef LN_BWD_CASE
    if (partial)
        hipLaunchKernelGGL(ln_dgamma_reduce_kernel, dim3(ceil_div(a.W, 64), 2), dim3(1024), 0, stream, partial, blocks, a.W, dgamma, dbeta);
}

// which residuals a row of the table below takes: none, res1, res2, res1 + res2
enum : int { LN_NONE = 1, LN_RES1 = 2, LN_RES2 = 4, LN_BOTH = 8, LN_ANY = LN_NONE | LN_RES1 | LN_RES2 | LN_BOTH };
template <typename TDY, typename TX, typename TR1, bool Q8, bool CLS, int RES>
static bool ln_bwd_pick(const LnBwdArgs& a, hipStream_t stream) {
    const int res = a.res1 ? (a.res2 ? LN_BOTH : LN_RES1) : (a.res2 ? LN_RES2 : LN_NONE);
    if (!(RES & res)) return false;
    if constexpr ((RES & LN_NONE) != 0) if (res == LN_NONE) launch_ln_bwd<TDY, false, false, TX, Q8, TR1, CLS>(a, stream);
    if constexpr ((RES & LN_RES1) != 0) if (res == LN_RES1) launch_ln_bwd<TDY, true, false, TX, Q8, TR1, CLS>(a, stream);
    if constexpr ((RES & LN_RES2) != 0) if (res == LN_RES2) launch_ln_bwd<TDY, false, true, TX, Q8, TR1, CLS>(a, stream);
    if constexpr ((RES & LN_BOTH) != 0) if (res == LN_BOTH) launch_ln_bwd<TDY, true, true, TX, Q8, TR1, CLS>(a, stream);
    return true;
}
// Every backward form there is: (dy, x, res1 type, e4m3 copy, CLS launch) -> the kernel's types and the residuals the form takes.
// -> false, nothing launched, for what is no row here: fp32 dy with a bf16 x or res1, a bf16 x with an fp32 res1, res2 without res1
// beside the e4m3 copy or on the CLS rows, a CLS launch of anything but the all-bf16 stream.
static bool ln_bwd_dispatch(const LnBwdArgs& a, hipStream_t stream) {
    // without res1 its type is moot: the kernel's is that of x
    const bool r1_bf16 = a.res1 ? a.res1_bf16 : a.x_bf16, q8 = a.q8;
    constexpr int CHAIN = LN_NONE | LN_RES1 | LN_BOTH, WITH1 = LN_RES1 | LN_BOTH;
    auto key = [](bool dy_f32, bool x_bf16, bool r1_bf16, bool q8, bool cls) constexpr {
        return (int)dy_f32 << 4 | (int)x_bf16 << 3 | (int)r1_bf16 << 2 | (int)q8 << 1 | (int)cls;
    };
    switch (key(a.dy_f32, a.x_bf16, r1_bf16, q8, a.cls)) {
    //        dy32 x16 r1-16 q8 cls                           dy     x      res1   Q8     CLS    residuals
    case key(1, 0, 0, 0, 0): return ln_bwd_pick<float, float, float, false, false, LN_ANY>(a, stream);
    case key(0, 0, 0, 0, 0): return ln_bwd_pick<bf16, float, float, false, false, LN_ANY>(a, stream);
    // (bf16 res1 beside an fp32 x: the two rows without res1 are compiled and never picked -- without res1 the line above is)
    case key(0, 0, 1, 0, 0): return ln_bwd_pick<bf16, float, bf16, false, false, LN_ANY>(a, stream);
    case key(0, 1, 1, 0, 0): return ln_bwd_pick<bf16, bf16, bf16, false, false, LN_ANY>(a, stream);
    case key(0, 0, 0, 1, 0): return ln_bwd_pick<bf16, float, float, true, false, CHAIN>(a, stream);
    case key(0, 0, 1, 1, 0): return ln_bwd_pick<bf16, float, bf16, true, false, WITH1>(a, stream);
    case key(0, 1, 1, 1, 0): return ln_bwd_pick<bf16, bf16, bf16, true, false, CHAIN>(a, stream);
    case key(0, 1, 1, 0, 1): return ln_bwd_pick<bf16, bf16, bf16, false, true, CHAIN>(a, stream);
    case key(0, 1, 1, 1, 1): return ln_bwd_pick<bf16, bf16, bf16, true, true, CHAIN>(a, stream);
    default: return false;
    }
}

// bf16 x: a side-branch value (ln_1's time residual) or the bf16 residual stream of the space-time blocks.  A bf16 res1: the
// residual-stream gradient carried in bf16 (the space-time block's backward).
extern "C" int tvts_layernorm_bwd(const void* dy, int lddy, int dy_f32, const void* x_, int ldx, int x_bf16, const int* rows,
                                  const float* mean, const float* rstd, const float* gamma, const void* res1_, int res1_bf16,
                                  int ldr, const void* res2_bf16, int ldr2, int M, int W, float* dx, int lddx,
                                  void* dx_bf16, int lddxb, float* dgamma, float* dbeta, float* workspace,
                                  long workspace_elems, hipStream_t stream) {
    const LnBwdArgs a{dy, lddy, dy_f32 != 0, x_, ldx, x_bf16 != 0, rows, mean, rstd, gamma, res1_, res1_bf16 != 0, ldr,
                      (const bf16*)res2_bf16, ldr2, M, W, dx, lddx, (bf16*)dx_bf16, lddxb, dgamma, dbeta, workspace, workspace_elems};
    if (ln_bwd_bad(a) || !ln_bwd_dispatch(a, stream)) return TVTS_EINVAL;
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// LayerNorm backward that also emits the e4m3 copy of its bf16 output with per-row scales (Q8 above): the forms of the space-time
// block's backward -- bf16 dy with (ln_2) fp32 residual, (ln_3) fp32 + bf16 residuals, (ln_1) bf16 x and no residual, (ln_post) fp32 x
// and no residual.  Every row (no row list), dx_bf16 required.
extern "C" int tvts_layernorm_bwd_fp8(const void* dy, int lddy, const void* x_, int ldx, int x_bf16, const float* mean,
                                      const float* rstd, const float* gamma, const void* res1_, int res1_bf16, int ldr, const void* res2_bf16,
                                      int ldr2, int M, int W, float* dx, int lddx, void* dx_bf16, int lddxb, void* q8, int ldq,
                                      float* row_scale, const float* tscale, float* amax_acc, float* dgamma, float* dbeta,
                                      float* workspace, long workspace_elems, hipStream_t stream) {
    const LnBwdArgs a{dy, lddy, false, x_, ldx, x_bf16 != 0, nullptr, mean, rstd, gamma, res1_, res1_bf16 != 0, ldr,
                      (const bf16*)res2_bf16, ldr2, M, W, dx, lddx, (bf16*)dx_bf16, lddxb, dgamma, dbeta, workspace, workspace_elems,
                      (unsigned char*)q8, ldq, row_scale, tscale, amax_acc};
    if (ln_bwd_bad(a) || !dx_bf16 || !q8 || !ln_bwd_dispatch(a, stream)) return TVTS_EINVAL;
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// LayerNorm backward on the hybrid residual stream (tvts_layernorm_fwd_cls): bf16 dy, bf16 x [M, W], every row; res1 (optional) the
// bf16 stream gradient, res2 (optional, only with res1) a bf16 side branch; dx_bf16 required.  For the rows r % cls_period == 0:
// input from cls_x (optional), residual-stream gradient from cls_res1 (optional; fp32 [M / cls_period, W]) instead of res1's row,
// result also to cls_dx (optional, fp32).  q8 (optional) as in tvts_layernorm_bwd_fp8.
extern "C" int tvts_layernorm_bwd_cls(const void* dy, int lddy, const void* x_, int ldx, const float* cls_x, const float* cls_res1,
                                      float* cls_dx, int cls_period, const float* mean, const float* rstd, const float* gamma,
                                      const void* res1_bf16, int ldr, const void* res2_bf16, int ldr2, int M, int W, void* dx_bf16,
                                      int lddxb, void* q8, int ldq, float* row_scale, const float* tscale, float* amax_acc,
                                      float* dgamma, float* dbeta, float* workspace, long workspace_elems, hipStream_t stream) {
    // every row through the plain bf16-stream kernel (the CLS rows' results there come from the stream's bf16 rows: close, and
    // replaced below; it is told cls_period only to keep them out of amax_acc), then the CLS rows alone from the fp32 side arrays
    const LnBwdArgs every{dy, lddy, false, x_, ldx, true, nullptr, mean, rstd, gamma, res1_bf16, true, ldr,
                          (const bf16*)res2_bf16, ldr2, M, W, nullptr, 0, (bf16*)dx_bf16, lddxb, dgamma, dbeta, workspace, workspace_elems,
                          (unsigned char*)q8, ldq, row_scale, tscale, amax_acc, cls_period};
    LnBwdArgs cls_rows = every;
    cls_rows.cls = true, cls_rows.cls_x = cls_x, cls_rows.cls_res1 = cls_res1, cls_rows.cls_dx = cls_dx;
    if (ln_bwd_bad(every) || ln_cls_bad(M, cls_period) || (cls_res1 && !res1_bf16) || (res2_bf16 && !res1_bf16)) return TVTS_EINVAL;
    if (!ln_bwd_dispatch(every, stream) || !ln_bwd_dispatch(cls_rows, stream)) return TVTS_EINVAL;
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
