// Token-assembly kernels around the transformer stacks (all HBM-bound gathers / scatters, fp32 unless noted).
//
//  tvts_patch_gather        kept patches of every frame -> bf16 im2col rows [B*T*n, 3*p*p] in conv-weight order
//                           (v2/model/video_encoder_ViT_B_16.py:180-184 + tube-mask gather :201-215; only kept
//                           patches are embedded -- output-equivalent)
//  tvts_patch_gather_u8*    the same from uint8 frames as decoded (crop, / 255, Normalize fused; _resized: Pillow's nearest Resize
//                           through index tables; _ragged: per-clip source sizes, crops and lengths from a descriptor table)
//  tvts_patch_gather_tube*  the v1 tubelet (Conv3d) form of the same im2col: seven entry points -- fp32 clips frame- or channel-major,
//                           uint8 frames behind a crop, test views, random-resized crop / flip / erase, each of the fine-tuning
//                           forms with Mixup / CutMix -- over ONE kernel frame (tube_gather_kernel) and four source policies
//  tvts_resize_crop_u8      the Resize (Pillow's 8-bit bilinear resample, with its bytes) and the crop of the v1 pretraining transform on
//                           uint8 source clips of any sizes, in front of tvts_patch_gather_tube_u8
//  tvts_vit_assemble(+_bwd) CLS + patch embedding + spatial/temporal position (:185-198) -> tokens [B*S, W]
//  tvts_text_embed(+_bwd)   token embedding gather + positional add (model_dist_TVTSv2_ViT_B_16.py:98-100)
//  tvts_text_mean(+_bwd)    clip-major captions [NT*B,E] -> mean over NT and the [B,NT,E] copy for the sort head (:69-76)
//  tvts_sort_assemble(+_bwd) video tokens + type_embed[0] | caption embeddings + type_embed[1]
//                           (v2/model/sort_transformer.py:124-128)
#include "common.h"

// ---------------------------------------------------------------------------------------------- patch gather
__global__ __launch_bounds__(256) void patch_gather_kernel(const float* __restrict__ video, const int* __restrict__ keep,
                                                           int B, int T, int n, int img, int p, bf16* __restrict__ out,
                                                           int ldo) {
    const int K = 3 * p * p;
    const int row = blockIdx.x;  // (b, f, i)
    const int i = row % n, f = (row / n) % T, b = row / (n * T);
    const int g = img / p;
    const int pi = keep[b * n + i];
    const int gy = pi / g, gx = pi % g;
    const float* fr = video + ((size_t)(b * T + f) * 3) * img * img;
    for (int c8 = threadIdx.x * 8; c8 < K; c8 += 256 * 8) {
        const int ch = c8 / (p * p), rem = c8 % (p * p), py = rem / p, px = rem % p;  // px multiple of 8
        const float* src = fr + ((size_t)ch * img + gy * p + py) * img + gx * p + px;
        const f32x4 a = *(const f32x4*)src, c = *(const f32x4*)(src + 4);
        bf16x8 o = {(bf16)a[0], (bf16)a[1], (bf16)a[2], (bf16)a[3], (bf16)c[0], (bf16)c[1], (bf16)c[2], (bf16)c[3]};
        *(bf16x8*)(out + (size_t)row * ldo + c8) = o;
    }
}

// any patch size (H/14: p = 14, K = 588): one thread per output column, columns K..ldo-1 are written as zeros so the
// patch-embedding GEMM can run with its K padded to a multiple of 64.
__global__ __launch_bounds__(256) void patch_gather_any_kernel(const float* __restrict__ video, const int* __restrict__ keep,
                                                               int B, int T, int n, int img, int p, bf16* __restrict__ out,
                                                               int ldo) {
    const int K = 3 * p * p;
    const int row = blockIdx.x;
    const int i = row % n, f = (row / n) % T, b = row / (n * T);
    const int g = img / p;
    const int pi = keep[b * n + i];
    const int gy = pi / g, gx = pi % g;
    const float* fr = video + ((size_t)(b * T + f) * 3) * img * img;
    for (int c = threadIdx.x; c < ldo; c += 256) {
        float v = 0.f;
        if (c < K) {
            const int ch = c / (p * p), rem = c % (p * p), py = rem / p, px = rem % p;
            v = fr[((size_t)ch * img + gy * p + py) * img + gx * p + px];
        }
        out[(size_t)row * ldo + c] = (bf16)v;
    }
}

extern "C" int tvts_patch_gather(const float* video, const int* keep, int B, int T, int n, int img, int patch, void* out,
                                 int ldo, hipStream_t stream) {
    if (B <= 0 || T <= 0 || n <= 0 || patch <= 0 || img % patch || ldo % 8 || ldo < 3 * patch * patch) return TVTS_EINVAL;
    if (patch % 8 || ldo != 3 * patch * patch)
        hipLaunchKernelGGL(patch_gather_any_kernel, dim3(B * T * n), dim3(256), 0, stream, video, keep, B, T, n, img, patch,
                           (bf16*)out, ldo);
    else
        hipLaunchKernelGGL(patch_gather_kernel, dim3(B * T * n), dim3(256), 0, stream, video, keep, B, T, n, img, patch,
                           (bf16*)out, ldo);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---------------------------------------------------------------------------------------------- v1 tubelet gathers
// v1 (TVTS) tubelet embedding: Conv3d(3, W, kernel = stride = (tb, p, p)) over [B, C, T, H, W] (v1/model/video_encoder.py:78-99)
// as an im2col product over the KEPT patches of every tube only.  Row (b, tube, i) = patch keep[b, tube, i] of tube `tube`,
// columns in the Conv3d weight's (c, t, py, px) order: K = 3 * tb * p * p.  keep differs from tube to tube here
// (v1/data_loader/YTTemporal_dataset.py:211-215).
//
// ONE kernel frame, tube_gather_kernel<Src, MIX>, owns what every form shares: the (b, tube, i) row decode, the keep lookup, the
// column decode, the optional Mixup / CutMix, the bf16 rounding and the 16-byte store.  What differs between the seven entry points
// is a SOURCE POLICY, a struct passed by value that holds its pointers and geometry and provides
//     bool resolve(b, Sample&)                 the sample's source; false leaves the sample's rows unwritten (block-uniform)
//     Block prologue()                         once per block behind the resolves: what the block's loads share (the uint8 policies'
//                                              normalisation constants; the aug policy's LDS table, behind a barrier)
//     void load8(Block, Sample, ch, f, y, x, v[8])   the fp32 values of channel ch, frame f, pixels (y, x .. x + 7) of the img x img clip
// Policies: F32Clip<CM> (fp32 clips, frame- or channel-major), U8Crop (uint8 frames behind a crop offset), U8View (uint8 test views),
// U8Aug (uint8 random-resized crop, flip and erase).  Two forms that share a policy's load8 share its bits by construction.
// A policy's operations reach its fields through `this`, i.e. as loads from the kernel's arguments, and a select between two such
// loads (the channel's mean; a centre-crop offset against crop[b]) is compiled into ONE load through a selected address -- a vector
// load inside the column loop where a v_cndmask on two scalar registers belongs (+4 % on the uint8 forms).  So what load8 selects
// between travels BY VALUE, in the Block, and no policy selects between a field and a table entry.
struct TubeRows { const int* keep; int B, tubes, tb, n, img, p; bf16* out; int ldo; };

// Mixup / CutMix of the v1 fine-tuning recipe (v1/downstream/mixup.py:152-200, applied at engine_for_finetuning.py:58-59) fused
// into the gather.  The step's draw arrives as a per-sample table in device memory:
//     mix_i int32 [B, 6] = (partner, mode, yl, yh, xl, xh)     mode 0 none, 1 mixup, 2 cutmix; the box in image coordinates
//                                                              behind the crop, half-open
//     mix_f fp32  [B, 2] = (lam, one_minus_lam)                both rounded by the host
// mode 0: the sample's own value, its bits untouched (mixup.py:159,176,191 skip lam == 1: no x * 1 + y * 0).
// mode 1: fadd_rn(fmul_rn(v_self, lam), fmul_rn(v_partner, one_minus_lam)) -- two fp32 products, then the fp32 sum, as
//         `x.mul_(lam).add_(x.flip(0).mul_(1. - lam))` (:198-199); never an FMA.
// mode 2: the partner's value inside [yl, yh) x [xl, xh) of every channel and frame (:163,196), the own value outside.
// mode 3: cutmix as the reference's PAIR mode runs it on 5-D clips: `x[i][:, yl:yh, xl:xh]` (:180-181) is written for [C, H, W]
//         pictures, and on a clip [C, T, H, W] its two slices land on (frame, row): the partner's value in the frames [yl, yh) (cut
//         at T, as a slice is) and the rows [xl, xh) of every channel, over the whole row width; the own value elsewhere.
// The select is per element (a thread's 8-pixel group may be cut by xl / xh anywhere); the partner is loaded only by the threads
// that hold an element needing it, through the policy's own resolve (a uint8 partner takes ITS OWN crop, an augmented one ITS OWN
// table row).  A partner outside [0, B) leaves the sample's rows unwritten (nothing is read for it).
struct MixRow { int partner, mode, yl, yh, xl, xh; float lam, oml; };
__device__ __forceinline__ MixRow mix_row(const int* __restrict__ mix_i, const float* __restrict__ mix_f, int b) {
    const int* mi = mix_i + 6 * (size_t)b;
    return MixRow{mi[0], mi[1], mi[2], mi[3], mi[4], mi[5], mix_f[2 * (size_t)b], mix_f[2 * (size_t)b + 1]};
}
// does the 8-pixel group at frame f, (y, x .. x + 7) need the partner's values?
__device__ __forceinline__ bool mix_needs_partner(const MixRow& m, int f, int y, int x) {
    return m.mode == 1 || (m.mode == 2 && y >= m.yl && y < m.yh && x < m.xh && x + 8 > m.xl) ||
           (m.mode == 3 && f >= m.yl && f < m.yh && y >= m.xl && y < m.xh);
}
__device__ __forceinline__ void mix_apply8(const MixRow& m, int x, float* v, const float* w) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (m.mode == 1) v[e] = __fadd_rn(__fmul_rn(v[e], m.lam), __fmul_rn(w[e], m.oml));
        else if (m.mode == 3 || (x + e >= m.xl && x + e < m.xh)) v[e] = w[e];
    }
}

template <class Src, bool MIX>
__global__ __launch_bounds__(256) void tube_gather_kernel(const Src src, const TubeRows r, const int* __restrict__ mix_i,
                                                          const float* __restrict__ mix_f) {
    const int tb = r.tb, p = r.p, pp = p * p, K = 3 * tb * pp;
    const int row = blockIdx.x;  // (b, tube, i)
    const int i = row % r.n, tu = (row / r.n) % r.tubes, b = row / (r.n * r.tubes);
    const int g = r.img / p;
    const int pi = r.keep[(size_t)(b * r.tubes + tu) * r.n + i];
    const int gy = pi / g, gx = pi % g;
    typename Src::Sample s, ps;
    if (!src.resolve(b, s)) return;
    MixRow m;
    if constexpr (MIX) {
        m = mix_row(mix_i, mix_f, b);
        if ((unsigned)m.partner >= (unsigned)r.B) return;
        if (!src.resolve(m.partner, ps)) return;
    }
    const typename Src::Block blk = src.prologue();  // (the returns above are block-uniform: a barrier in here is reached by all)
    for (int c8 = threadIdx.x * 8; c8 < K; c8 += 256 * 8) {
        const int ch = c8 / (tb * pp), r1 = c8 % (tb * pp), t = r1 / pp, rem = r1 % pp, py = rem / p, px = rem % p;  // px % 8 == 0
        const int y = gy * p + py, x = gx * p + px, f = tu * tb + t;
        float v[8];
        src.load8(blk, s, ch, f, y, x, v);
        if constexpr (MIX) {
            if (mix_needs_partner(m, f, y, x)) {
                float w[8];
                src.load8(blk, ps, ch, f, y, x, w);
                mix_apply8(m, x, v, w);
            }
        }
        bf16x8 o = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3], (bf16)v[4], (bf16)v[5], (bf16)v[6], (bf16)v[7]};
        *(bf16x8*)(r.out + (size_t)row * r.ldo + c8) = o;
    }
}

// fp32 clips: frame-major [B, T, 3, img, img], as the pretrain model gets them (it permutes itself, v1/model/video_encoder.py:179),
// or (CM) channel-major [B, 3, T, img, img], the layout the v1 downstream classes take (their forward hands x to the Conv3d as it
// comes, v1/downstream/video_encoder_zero.py:91-96,177).  Two 16-byte loads per 8 pixels; the values pass through untouched.
template <bool CM>
struct F32Clip {
    const float* video;
    int T, img;
    typedef int Sample;  // the clip's index
    __device__ __forceinline__ bool resolve(int b, Sample& s) const {
        s = b;
        return true;
    }
    struct Block {};
    __device__ __forceinline__ Block prologue() const { return Block{}; }
    __device__ __forceinline__ void load8(Block, Sample s, int ch, int f, int y, int x, float* v) const {
        const float* src = video + (((size_t)(CM ? (s * 3 + ch) * T + f : (s * T + f) * 3 + ch) * img + y) * img + x);
        const f32x4 a = *(const f32x4*)src, c = *(const f32x4*)(src + 4);
        v[0] = a[0], v[1] = a[1], v[2] = a[2], v[3] = a[3], v[4] = c[0], v[5] = c[1], v[6] = c[2], v[7] = c[3];
    }
};

// The uint8 wire format: frames uint8 [., ., H0, W0, 3] as the decoder leaves them; ClipToTensor (/ 255) and Normalize
// ((v - mean) / std) of v1/downstream/ssv2.py:61-63 run here.  u8_norm is THE normalise expression of every uint8 form: the
// operations and their order are those of patch_gather_u8_kernel below, so the bytes equal the fp32 policy's on host-normalised
// frames.  load8 converts 8 neighbouring px (24 interleaved source bytes apart by 3) of frame fr at (y, x) of the source picture.
struct U8Norm { float m0, m1, m2, s0, s1, s2; };
__device__ __forceinline__ float u8_norm(const U8Norm n, float u, int ch) {
    const float mean = ch == 0 ? n.m0 : ch == 1 ? n.m1 : n.m2, sd = ch == 0 ? n.s0 : ch == 1 ? n.s1 : n.s2;
    return (u / 255.0f - mean) / sd;
}
struct U8Frames {
    const unsigned char* frames;
    int H0, W0;
    U8Norm nrm;
    typedef U8Norm Block;
    __device__ __forceinline__ Block prologue() const { return nrm; }
    __device__ __forceinline__ void load8(const U8Norm n, size_t fr, int ch, int y, int x, float* v) const {
        const unsigned char* src = frames + ((fr * H0 + y) * W0 + x) * 3 + ch;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = u8_norm(n, (float)src[3 * e], ch);
    }
};
// the centre crop of a margin d = H0 - img: d / 2 rounded half to even (the offsets of patch_gather_u8_kernel)
static inline int centre_crop_offset(int d) { return (d >> 1) + ((d & 1) & (d >> 1)); }

// uint8 clips [B, T, H0, W0, 3] behind a crop: an offset per sample (crop int32 [B, 2] = (top, left), device data; y0 = x0 = 0), or
// the centre crop (crop NULL; y0, x0 the offsets, which the host forms).  Under a mix each of the two samples is cropped with ITS
// OWN offset.
struct U8Crop : U8Frames {
    const int* crop;
    int T, y0, x0;
    struct Sample { int f0, y0, x0; };
    __device__ __forceinline__ bool resolve(int b, Sample& s) const {
        s = Sample{b * T, y0 + (crop ? crop[2 * b] : 0), x0 + (crop ? crop[2 * b + 1] : 0)};
        return true;
    }
    __device__ __forceinline__ void load8(const U8Norm n, const Sample& s, int ch, int f, int y, int x, float* v) const {
        U8Frames::load8(n, (size_t)(s.f0 + f), ch, s.y0 + y, s.x0 + x, v);
    }
};

// The test views of the fine-tuning scripts (v1/downstream/ssv2.py:132-164): sample b is the frames t0, t0 + tstep, ... of source
// clip src of frames [Bs, Tsrc, H0, W0, 3], cropped at (top, left) -- `buffer[temporal_start::2, spatial_start:spatial_start +
// short_side_size]` -- read from a per-sample table in device memory, view_i int32 [B, 8] = (src, t0, tstep, top, left, 0, 0, 0).
// Only the source address differs from U8Crop: the bytes equal that form's on the host-sliced clip.  The views of one video read
// one uploaded clip.  A src outside [0, Bs) leaves the sample's rows unwritten.
struct U8View : U8Frames {
    const int* view_i;
    int Bs, Tsrc;
    struct Sample { size_t f0; int tstep, y0, x0; };
    __device__ __forceinline__ bool resolve(int b, Sample& s) const {
        const int* v = view_i + 8 * (size_t)b;
        s = Sample{(size_t)v[0] * Tsrc + v[1], v[2], v[3], v[4]};
        return (unsigned)v[0] < (unsigned)Bs;
    }
    __device__ __forceinline__ void load8(const U8Norm n, const Sample& s, int ch, int f, int y, int x, float* v) const {
        U8Frames::load8(n, s.f0 + (size_t)f * s.tstep, ch, s.y0 + y, s.x0 + x, v);
    }
};

// The per-sample augmentation of the v1 fine-tuning recipe behind RandAugment (v1/downstream/ssv2.py:186-227): Normalize,
// random_resized_crop (video_transforms.py:541-573: a crop of the source frame resized to img x img by torch's bilinear
// interpolate, align_corners=False), horizontal_flip (:156-177), RandomErasing in cube mode (random_erasing.py:109-149), then the
// frame's mix.  The step's draw arrives as a per-sample table in device memory:
//     aug_i int32 [B, 16] = (src, top, left, h, w, flip, emode, etop, eleft, eh, ew, key_lo, key_hi, 0, 0, 0)
// src: the source clip in [0, Bs) (several samples may read one clip: --num_sample); the crop [top, top + h) x [left, left + w) of
// the source frame; flip mirrors the resized picture in x; the erase box [etop, etop + eh) x [eleft, eleft + ew) in OUTPUT
// coordinates, the same in every frame, emode 0 none / 1 zeros / 2 one normal per (frame, channel) / 3 one per (frame, channel,
// pixel); key: the sample's 64-bit noise key.  Per output element, in the reference's order:
//   taps   sy = (float)h / (float)img, src = max(sy * (y + 0.5f) - 0.5f, 0), y0 = (int)src, y1 = min(y0 + 1, h - 1) (the CROP's
//          edge), ly = src - y0; the same in x with w, for x' = flip ? img - 1 - x : x.  Products and differences are rounded
//          one by one (no FMA), as the expression is written.
//   values the four taps of frame src * T + f, each normalised by u8_norm
//   blend  (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c + lx * d), every product and sum rounded; with h == w == img all
//          l are 0 and the value is tap a, bit for bit
//   erase  inside the box: 0 / z(key + AUG_RAND_STREAM, f * 3 + c) / z(key, ((f * 3 + c) * img + y) * img + x), x and y of the OUTPUT
//   mix    the frame's mix_apply8 over this value and the partner's, the partner formed through ITS OWN table row
// z(key, idx): r = the splitmix64 finaliser (attention.hip::drop_keep) of key + idx * 0x9E3779B97F4A7C15; u1 = ((r >> 32) + 1) * 2^-32
// in (0, 1], u2 = (r & 0xffffffff) * 2^-32; z = sqrtf(-2 logf(u1)) * cosf(2 pi u2) (Box-Muller, the accurate library functions;
// ln u1 through log1pf where u1 is within 2^-8 of 1).  The float64 form of this rule is the definition (tests/v1_aug_ref.noise).
// The y taps and weights are formed once per 8-pixel row piece; a piece reads at most two source rows.  A src outside [0, Bs) -- the
// sample's own or its partner's -- leaves the sample's rows unwritten.
#define AUG_RAND_STREAM 0xD1B54A32D192ED03ull
struct AugRow { int src, top, left, h, w, flip, emode, etop, eleft, eh, ew; unsigned long long key; };
__device__ __forceinline__ AugRow aug_row(const int* __restrict__ aug_i, int b) {
    const int* a = aug_i + 16 * (size_t)b;
    return AugRow{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10],
                  (unsigned long long)(unsigned)a[11] | ((unsigned long long)(unsigned)a[12] << 32)};
}
__device__ __forceinline__ float aug_noise(unsigned long long key, unsigned long long idx) {
    unsigned long long z = key + idx * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    // ln u1: an fp32 u1 within 2^-8 of 1 has lost the bits that ln u1 = -(1 - u1) - ... consists of (z would be off by up to 2e-4
    // there); 1 - u1 = k * 2^-32 with k < 2^24 is exact in fp32, so that range takes log1pf(-(1 - u1))
    const unsigned hi = (unsigned)(z >> 32), k = 0xFFFFFFFFu - hi;  // u1 = (hi + 1) * 2^-32 = 1 - k * 2^-32
    const float ln_u1 = k < (1u << 24) ? log1pf(-(float)k * 2.3283064365386963e-10f) : logf(((float)hi + 1.0f) * 2.3283064365386963e-10f);
    const float u2 = (float)(unsigned)z * 2.3283064365386963e-10f;
    return sqrtf(-2.0f * ln_u1) * cosf(6.283185307179586f * u2);
}
// torch's area_pixel_compute_source_index + guard_index_and_lambda for one output coordinate -> (i0, i1, lambda1)
__device__ __forceinline__ void aug_tap(float scale, int o, int size, int& i0, int& i1, float& l) {
    const float s = fmaxf(__fsub_rn(__fmul_rn(scale, (float)o + 0.5f), 0.5f), 0.f);
    i0 = min((int)s, size - 1);
    i1 = min(i0 + 1, size - 1);
    l = fminf(fmaxf(__fsub_rn(s, (float)i0), 0.f), 1.f);
}
// uint8 source clips [Bs, T, H0, W0, 3] (any H0, W0 >= 1).  Block: the 256 normalised values of every channel, which the block forms
// once in LDS -- u8_norm itself, so the same bits, at one pair of divisions per (block, channel, byte value) instead of four
// pairs per element.
struct U8Aug : U8Frames {
    const int* aug_i;
    int Bs, T, img;
    typedef AugRow Sample;
    typedef const float (*Block)[256];
    __device__ __forceinline__ bool resolve(int b, Sample& a) const {
        a = aug_row(aug_i, b);
        return (unsigned)a.src < (unsigned)Bs;
    }
    __device__ __forceinline__ Block prologue() const {
        __shared__ float lds[3][256];
        for (int ch = 0; ch < 3; ++ch) lds[ch][threadIdx.x] = u8_norm(nrm, (float)threadIdx.x, ch);
        __syncthreads();
        return lds;
    }
    __device__ __forceinline__ void load8(Block table, const AugRow& a, int ch, int f, int y, int x, float* v) const {
        const float* norm = table[ch];
        int y0, y1;
        float ly;
        aug_tap((float)a.h / (float)img, y, a.h, y0, y1, ly);
        const float sx = (float)a.w / (float)img, hy = __fsub_rn(1.0f, ly);
        const unsigned char* r0 = frames + (((size_t)(a.src * T + f) * H0 + a.top + y0) * W0 + a.left) * 3 + ch;
        const unsigned char* r1 = r0 + (size_t)(y1 - y0) * W0 * 3;
        const bool erow = a.emode != 0 && y >= a.etop && y < a.etop + a.eh;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int xo = x + e;
            if (erow && xo >= a.eleft && xo < a.eleft + a.ew) {
                const unsigned long long fc = (unsigned long long)(f * 3 + ch);
                v[e] = a.emode == 1 ? 0.0f
                     : a.emode == 2 ? aug_noise(a.key + AUG_RAND_STREAM, fc)
                                    : aug_noise(a.key, (fc * img + y) * img + xo);
                continue;
            }
            int x0, x1;
            float lx;
            aug_tap(sx, a.flip ? img - 1 - xo : xo, a.w, x0, x1, lx);
            const float hx = __fsub_rn(1.0f, lx);
            const float p00 = norm[r0[3 * x0]], p01 = norm[r0[3 * x1]], p10 = norm[r1[3 * x0]], p11 = norm[r1[3 * x1]];
            const float up = __fadd_rn(__fmul_rn(hx, p00), __fmul_rn(lx, p01)), dn = __fadd_rn(__fmul_rn(hx, p10), __fmul_rn(lx, p11));
            v[e] = __fadd_rn(__fmul_rn(hy, up), __fmul_rn(ly, dn));
        }
    }
};

// ---- the seven entry points: one shared argument check, the policy, one shared launch
// what every form refuses: a NULL source / keep / out, a non-positive size, img % patch, patch % 8 (a thread's 8 pixels lie in one
// patch row), ldo % 8 or ldo < K, out not 16-byte aligned (the bf16x8 store), the source not aligned to src_align bytes (16 for the
// f32x4 loads of the fp32 clips)
static bool tube_rows_ok(const void* src, size_t src_align, const TubeRows& r) {
    return src && r.keep && r.out && r.B > 0 && r.tubes > 0 && r.tb > 0 && r.n > 0 && r.p > 0 && r.img > 0 && r.img % r.p == 0 &&
           r.p % 8 == 0 && r.ldo % 8 == 0 && r.ldo >= 3 * r.tb * r.p * r.p && (size_t)r.out % 16 == 0 && (size_t)src % src_align == 0;
}
// ... and every uint8 form: NULL mean3 / std3 (host arrays), source frames below min_side (img where a crop of img x img is cut
// from them, 1 where the crop is resized)
static bool u8_frames_ok(const float* mean3, const float* std3, int H0, int W0, int min_side) {
    return mean3 && std3 && H0 >= min_side && W0 >= min_side;
}
static U8Frames u8_frames(const unsigned char* frames, int H0, int W0, const float* mean3, const float* std3) {
    return U8Frames{frames, H0, W0, U8Norm{mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]}};
}
static U8Crop u8_crop(const unsigned char* frames, int H0, int W0, const float* mean3, const float* std3, const int* crop, int T, int img) {
    return U8Crop{u8_frames(frames, H0, W0, mean3, std3), crop, T, crop ? 0 : centre_crop_offset(H0 - img), crop ? 0 : centre_crop_offset(W0 - img)};
}
template <bool MIX, class Src>
static int tube_launch(const Src& src, const TubeRows& r, const int* mix_i, const float* mix_f, hipStream_t stream) {
    hipLaunchKernelGGL((tube_gather_kernel<Src, MIX>), dim3(r.B * r.tubes * r.n), dim3(256), 0, stream, src, r, mix_i, mix_f);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

extern "C" int tvts_patch_gather_tube(const float* video, const int* keep, int B, int tubes, int tubelet, int n, int img,
                                      int patch, void* out, int ldo, hipStream_t stream) {
    const TubeRows r{keep, B, tubes, tubelet, n, img, patch, (bf16*)out, ldo};
    if (!tube_rows_ok(video, 16, r)) return TVTS_EINVAL;
    return tube_launch<false>(F32Clip<false>{video, tubes * tubelet, img}, r, nullptr, nullptr, stream);
}
extern "C" int tvts_patch_gather_tube_cm(const float* video, const int* keep, int B, int tubes, int tubelet, int n, int img,
                                         int patch, void* out, int ldo, hipStream_t stream) {
    const TubeRows r{keep, B, tubes, tubelet, n, img, patch, (bf16*)out, ldo};
    if (!tube_rows_ok(video, 16, r)) return TVTS_EINVAL;
    return tube_launch<false>(F32Clip<true>{video, tubes * tubelet, img}, r, nullptr, nullptr, stream);
}
extern "C" int tvts_patch_gather_tube_cm_mix(const float* video, const int* keep, const int* mix_i, const float* mix_f, int B,
                                             int tubes, int tubelet, int n, int img, int patch, void* out, int ldo,
                                             hipStream_t stream) {
    const TubeRows r{keep, B, tubes, tubelet, n, img, patch, (bf16*)out, ldo};
    if (!tube_rows_ok(video, 16, r) || !mix_i || !mix_f) return TVTS_EINVAL;
    return tube_launch<true>(F32Clip<true>{video, tubes * tubelet, img}, r, mix_i, mix_f, stream);
}
extern "C" int tvts_patch_gather_tube_u8(const unsigned char* frames, int H0, int W0, const int* crop, const int* keep, int B,
                                         int tubes, int tubelet, int n, int img, int patch, const float* mean3, const float* std3,
                                         void* out, int ldo, hipStream_t stream) {
    const TubeRows r{keep, B, tubes, tubelet, n, img, patch, (bf16*)out, ldo};
    if (!tube_rows_ok(frames, 1, r) || !u8_frames_ok(mean3, std3, H0, W0, img)) return TVTS_EINVAL;
    return tube_launch<false>(u8_crop(frames, H0, W0, mean3, std3, crop, tubes * tubelet, img), r, nullptr, nullptr, stream);
}
extern "C" int tvts_patch_gather_tube_u8_mix(const unsigned char* frames, int H0, int W0, const int* crop, const int* keep,
                                             const int* mix_i, const float* mix_f, int B, int tubes, int tubelet, int n, int img,
                                             int patch, const float* mean3, const float* std3, void* out, int ldo,
                                             hipStream_t stream) {
    const TubeRows r{keep, B, tubes, tubelet, n, img, patch, (bf16*)out, ldo};
    if (!tube_rows_ok(frames, 1, r) || !u8_frames_ok(mean3, std3, H0, W0, img) || !mix_i || !mix_f) return TVTS_EINVAL;
    return tube_launch<true>(u8_crop(frames, H0, W0, mean3, std3, crop, tubes * tubelet, img), r, mix_i, mix_f, stream);
}
extern "C" int tvts_patch_gather_tube_u8_view(const unsigned char* frames, int Bs, int Tsrc, int H0, int W0, const int* view_i,
                                              const int* keep, int B, int tubes, int tubelet, int n, int img, int patch,
                                              const float* mean3, const float* std3, void* out, int ldo, hipStream_t stream) {
    const TubeRows r{keep, B, tubes, tubelet, n, img, patch, (bf16*)out, ldo};
    if (!tube_rows_ok(frames, 1, r) || !u8_frames_ok(mean3, std3, H0, W0, img) || !view_i || Bs <= 0 || Tsrc <= 0) return TVTS_EINVAL;
    return tube_launch<false>(U8View{u8_frames(frames, H0, W0, mean3, std3), view_i, Bs, Tsrc}, r, nullptr, nullptr, stream);
}
extern "C" int tvts_patch_gather_tube_u8_aug(const unsigned char* frames, int Bs, int H0, int W0, const int* keep, const int* aug_i,
                                             const int* mix_i, const float* mix_f, int B, int tubes, int tubelet, int n, int img,
                                             int patch, const float* mean3, const float* std3, void* out, int ldo,
                                             hipStream_t stream) {
    const TubeRows r{keep, B, tubes, tubelet, n, img, patch, (bf16*)out, ldo};
    if (!tube_rows_ok(frames, 1, r) || !u8_frames_ok(mean3, std3, H0, W0, 1) || !aug_i || Bs <= 0 || (!mix_i) != (!mix_f)) return TVTS_EINVAL;
    const U8Aug src{u8_frames(frames, H0, W0, mean3, std3), aug_i, Bs, tubes * tubelet, img};
    return mix_i ? tube_launch<true>(src, r, mix_i, mix_f, stream) : tube_launch<false>(src, r, nullptr, nullptr, stream);
}

// ---------------------------------------------------------------------------------------------- v1 Resize + crop, uint8 -> uint8
// The Resize of the v1 pretraining transform (v1/video_transforms/videoaug.py:10,18 -> video_transform.py:181-188 -> functional.py:56-59:
// on the PIL images TensorToNumpy makes, every interpolation but 'bilinear' -- the default 'nearest' included -- is PIL.Image.BILINEAR)
// and the RandomCrop / CenterCrop behind it, for the crop window only: Pillow's two-pass 8-bit resample (Resample.c, PRECISION_BITS
// 22) in its own integer arithmetic, so the bytes are Pillow's.  The taps are host tables (tvts_amd/data_loader/transforms.py
// pil_bilinear_coeffs), one per distinct (n_in, n_out) of the batch; a clip's descriptor row names its two.  Table and descriptor
// layouts: include/tvts_hip.h.
//   resize_rows_kernel   the horizontal pass over the source rows [y0, y1) that the vertical taps of the window read and the img
//                        columns of the window -> tmp uint8 [B, T, tmp_rows, img, 3] (the rounded bytes: Pillow rounds between the passes)
//   resize_cols_kernel   the vertical pass over tmp -> out [B, T, img, img, 3] (rows ldo bytes apart)
// One thread per pixel (three channels share the taps).  Every write index comes from the launch geometry: a clip whose window
// needs more than tmp_rows source rows (a descriptor the host check would refuse) is cut at tmp_rows in both passes.
struct ResizeTab {
    const int *first, *count, *taps;
    int ksize;
};
__device__ inline ResizeTab resize_tab(const int* __restrict__ tables, long off) {
    const int* t = tables + off;  // (n_in, n_out, ksize, 0) | first[n_out] | count[n_out] | taps[n_out][ksize]
    const int n_out = t[1];
    return ResizeTab{t + 4, t + 4 + n_out, t + 4 + 2 * (size_t)n_out, t[2]};
}
__device__ inline unsigned char clip8(int v) { return (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v); }
constexpr int kResizeBits = 22;

struct ResizeClip {
    long off;
    int Hs, Ws, top, left, y0, rows;
    ResizeTab ty, tx;
};
__device__ inline ResizeClip resize_clip(const long* __restrict__ desc, const int* __restrict__ tables, int b, int img, int tmp_rows) {
    const long* d = desc + (size_t)b * 8;
    ResizeClip c;
    c.off = d[0], c.Hs = (int)d[1], c.Ws = (int)d[2], c.top = (int)d[3], c.left = (int)d[4];
    c.ty = resize_tab(tables, d[5]), c.tx = resize_tab(tables, d[6]);
    c.y0 = c.ty.first[c.top];  // first / first + count never decrease along an axis: the window's first and last output rows bound it
    const int last = c.top + img - 1;
    c.rows = min(c.ty.first[last] + c.ty.count[last] - c.y0, tmp_rows);
    return c;
}

__global__ __launch_bounds__(256) void resize_rows_kernel(const unsigned char* __restrict__ src, const long* __restrict__ desc,
                                                          const int* __restrict__ tables, int T, int img, int tmp_rows,
                                                          unsigned char* __restrict__ tmp) {
    const int b = blockIdx.z, f = blockIdx.y;
    const ResizeClip c = resize_clip(desc, tables, b, img, tmp_rows);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int r = i / img, x = i - r * img;
    if (r >= c.rows) return;
    const int xo = c.left + x, n = c.tx.count[xo];
    const unsigned char* p = src + c.off + (((size_t)f * c.Hs + (c.y0 + r)) * c.Ws + c.tx.first[xo]) * 3;
    const int* k = c.tx.taps + (size_t)xo * c.tx.ksize;
    int a0 = 1 << (kResizeBits - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < n; ++j, p += 3) {
        const int kj = k[j];
        a0 += p[0] * kj, a1 += p[1] * kj, a2 += p[2] * kj;
    }
    unsigned char* o = tmp + ((((size_t)b * T + f) * tmp_rows + r) * img + x) * 3;
    o[0] = clip8(a0 >> kResizeBits), o[1] = clip8(a1 >> kResizeBits), o[2] = clip8(a2 >> kResizeBits);
}

__global__ __launch_bounds__(256) void resize_cols_kernel(const long* __restrict__ desc, const int* __restrict__ tables, int T, int img,
                                                          int tmp_rows, const unsigned char* __restrict__ tmp,
                                                          unsigned char* __restrict__ out, int ldo) {
    const int b = blockIdx.z, f = blockIdx.y;
    const ResizeClip c = resize_clip(desc, tables, b, img, tmp_rows);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int y = i / img, x = i - y * img;
    if (y >= img) return;
    const int yo = c.top + y, r0 = c.ty.first[yo] - c.y0, n = min(c.ty.count[yo], c.rows - r0);
    const unsigned char* p = tmp + ((((size_t)b * T + f) * tmp_rows + r0) * img + x) * 3;
    const int* k = c.ty.taps + (size_t)yo * c.ty.ksize;
    int a0 = 1 << (kResizeBits - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < n; ++j, p += (size_t)img * 3) {
        const int kj = k[j];
        a0 += p[0] * kj, a1 += p[1] * kj, a2 += p[2] * kj;
    }
    unsigned char* o = out + (((size_t)b * T + f) * img + y) * ldo + x * 3;
    o[0] = clip8(a0 >> kResizeBits), o[1] = clip8(a1 >> kResizeBits), o[2] = clip8(a2 >> kResizeBits);
}

extern "C" int tvts_resize_crop_u8(const unsigned char* src, const long* desc, const int* tables, int B, int T, int img, int tmp_rows,
                                   unsigned char* tmp, long tmp_bytes, unsigned char* out, int ldo, hipStream_t stream) {
    if (!src || !desc || !tables || !tmp || !out || B <= 0 || T <= 0 || img <= 0 || tmp_rows <= 0 || B > 65535 || T > 65535 ||
        img > 32768 || tmp_rows > 32768 || ldo < 3 * img)
        return TVTS_EINVAL;
    if (tmp_bytes < (long)B * T * tmp_rows * img * 3) return TVTS_EINVAL;
    hipLaunchKernelGGL(resize_rows_kernel, dim3((tmp_rows * img + 255) / 256, T, B), dim3(256), 0, stream, src, desc, tables, T, img,
                       tmp_rows, tmp);
    TVTS_LAUNCH_CHECK();
    hipLaunchKernelGGL(resize_cols_kernel, dim3((img * img + 255) / 256, T, B), dim3(256), 0, stream, desc, tables, T, img, tmp_rows,
                       tmp, out, ldo);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}


// uint8 wire format: the frames arrive as the decoder leaves them -- uint8, H x W x 3 interleaved, already
// resized on the host -- and the rest of the reference's transform chain runs here, fused into the tube-mask gather:
// crop (video_transform.CenterCrop / RandomCrop = an offset per sample), ClipToTensor (float32 / 255) and Normalize
// ((v - mean) / std, fp32, same operation order -> bit-identical to v2/video_transforms/video_transform.py:24-75,
// functional.py:81-97), then the bf16 rounding of the im2col row.  4x less PCIe / HBM traffic than fp32 frames.
// ytab / xtab (optional): the RESIZE in front of the crop (video_transform.Resize -> PIL nearest-neighbour, videoaug.py:12,21):
// frames are the decoder's Hs x Ws pictures, ytab[H0] / xtab[W0] give the source row / column of every row / column of the
// (virtual) resized H0 x W0 picture -- Pillow's own index table, built by tvts_amd/data_loader/transforms.py.
__global__ __launch_bounds__(256) void patch_gather_u8_kernel(const unsigned char* __restrict__ frames, int H0, int W0,
                                                              const int* __restrict__ crop, const int* __restrict__ keep,
                                                              int B, int T, int n, int img, int p, float m0, float m1,
                                                              float m2, float s0, float s1, float s2,
                                                              bf16* __restrict__ out, int ldo, const int* __restrict__ ytab,
                                                              const int* __restrict__ xtab, int Hs, int Ws) {
    const int K = 3 * p * p;
    const int row = blockIdx.x;  // (b, f, i)
    const int i = row % n, f = (row / n) % T, b = row / (n * T);
    const int g = img / p;
    const int pi = keep[b * n + i];
    const int gy = pi / g, gx = pi % g;
    // centre crop: int(round((H0 - img) / 2.)) with Python's round-half-to-even (video_transform.py:454-455)
    const int dy = H0 - img, dx = W0 - img;
    const int y0 = crop ? crop[2 * b] : (dy >> 1) + ((dy & 1) & (dy >> 1)), x0 = crop ? crop[2 * b + 1] : (dx >> 1) + ((dx & 1) & (dx >> 1));
    const unsigned char* fr = frames + (size_t)(b * T + f) * Hs * Ws * 3;
    for (int c = threadIdx.x; c < ldo; c += 256) {
        float v = 0.f;
        if (c < K) {
            const int ch = c / (p * p), rem = c % (p * p), py = rem / p, px = rem % p;
            int sy = y0 + gy * p + py, sx = x0 + gx * p + px;  // pixel of the (resized) H0 x W0 picture
            if (ytab) { sy = ytab[sy]; sx = xtab[sx]; }
            const float u = (float)fr[((size_t)sy * Ws + sx) * 3 + ch];
            const float mean = ch == 0 ? m0 : ch == 1 ? m1 : m2, sd = ch == 0 ? s0 : ch == 1 ? s1 : s2;
            v = (u / 255.0f - mean) / sd;
        }
        out[(size_t)row * ldo + c] = (bf16)v;
    }
}
extern "C" int tvts_patch_gather_u8(const unsigned char* frames, int H0, int W0, const int* crop, const int* keep, int B,
                                    int T, int n, int img, int patch, const float* mean3, const float* std3, void* out,
                                    int ldo, hipStream_t stream) {
    if (B <= 0 || T <= 0 || n <= 0 || patch <= 0 || img % patch || H0 < img || W0 < img || ldo % 8 || ldo < 3 * patch * patch)
        return TVTS_EINVAL;
    hipLaunchKernelGGL(patch_gather_u8_kernel, dim3(B * T * n), dim3(256), 0, stream, frames, H0, W0, crop, keep, B, T, n, img,
                       patch, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], (bf16*)out, ldo, nullptr, nullptr, H0, W0);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
// the same with the nearest-neighbour resize Hs x Ws -> H0 x W0 in front (ytab / xtab: device int32 [H0] / [W0])
extern "C" int tvts_patch_gather_u8_resized(const unsigned char* frames, int Hs, int Ws, const int* ytab, const int* xtab, int H0,
                                            int W0, const int* crop, const int* keep, int B, int T, int n, int img, int patch,
                                            const float* mean3, const float* std3, void* out, int ldo, hipStream_t stream) {
    if (B <= 0 || T <= 0 || n <= 0 || patch <= 0 || img % patch || H0 < img || W0 < img || ldo % 8 || ldo < 3 * patch * patch ||
        !ytab || !xtab || Hs <= 0 || Ws <= 0)
        return TVTS_EINVAL;
    hipLaunchKernelGGL(patch_gather_u8_kernel, dim3(B * T * n), dim3(256), 0, stream, frames, H0, W0, crop, keep, B, T, n, img,
                       patch, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], (bf16*)out, ldo, ytab, xtab, Hs, Ws);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
// RAGGED form of the same gather (DESIGN.md 8j "v2 ragged"): the clips of one batch differ in source size and length, as the
// reference's loaders hand them over -- every clip resized on its own (videoaug.py:12,21, functional.py:47-78), a clip of fewer
// than T frames zero-padded BEHIND Normalize (base_dataset.py:116-130).  One packed byte buffer and a descriptor row per clip
// (layouts: include/tvts_hip.h) stand in for (frames, Hs, Ws, ytab, xtab, H0, W0, crop); the descriptor is block-uniform, read once
// per block.  The value expression is patch_gather_u8_kernel's, token for token, so a clip's rows carry the bytes of
// tvts_patch_gather_u8_resized run on that clip alone; a sibling kernel, so that kernel's launches stay what they were.
__global__ __launch_bounds__(256) void patch_gather_u8_ragged_kernel(const unsigned char* __restrict__ src,
                                                                     const long* __restrict__ desc, const int* __restrict__ tables,
                                                                     const int* __restrict__ keep, int B, int T, int n, int img,
                                                                     int p, float m0, float m1, float m2, float s0, float s1,
                                                                     float s2, bf16* __restrict__ out, int ldo) {
    const int K = 3 * p * p;
    const int row = blockIdx.x;  // (b, f, i)
    const int i = row % n, f = (row / n) % T, b = row / (n * T);
    const long* d = desc + (size_t)b * 8;
    const int frames = (int)d[7];
    if (f >= frames) {  // the reference's zero frame behind Normalize: +0 in all ldo columns
        for (int c = threadIdx.x; c < ldo; c += 256) out[(size_t)row * ldo + c] = (bf16)0.f;
        return;
    }
    const int Hs = (int)d[1], Ws = (int)d[2], y0 = (int)d[3], x0 = (int)d[4];
    const int* __restrict__ ytab = tables + d[5] + 2;  // (n_in, n_out) | index[n_out]
    const int* __restrict__ xtab = tables + d[6] + 2;
    const int g = img / p;
    const int pi = keep[b * n + i];
    const int gy = pi / g, gx = pi % g;
    const unsigned char* fr = src + d[0] + (size_t)f * Hs * Ws * 3;
    for (int c = threadIdx.x; c < ldo; c += 256) {
        float v = 0.f;
        if (c < K) {
            const int ch = c / (p * p), rem = c % (p * p), py = rem / p, px = rem % p;
            const int sy = ytab[y0 + gy * p + py], sx = xtab[x0 + gx * p + px];  // pixel of the (resized) picture -> source pixel
            const float u = (float)fr[((size_t)sy * Ws + sx) * 3 + ch];
            const float mean = ch == 0 ? m0 : ch == 1 ? m1 : m2, sd = ch == 0 ? s0 : ch == 1 ? s1 : s2;
            v = (u / 255.0f - mean) / sd;
        }
        out[(size_t)row * ldo + c] = (bf16)v;
    }
}
extern "C" int tvts_patch_gather_u8_ragged(const unsigned char* src, const long* desc, const int* tables, const int* keep, int B,
                                           int T, int n, int img, int patch, const float* mean3, const float* std3, void* out,
                                           int ldo, hipStream_t stream) {
    if (!src || !desc || !tables || !keep || !out || !mean3 || !std3 || B <= 0 || T <= 0 || n <= 0 || patch <= 0 || img <= 0 ||
        img % patch || ldo % 8 || ldo < 3 * patch * patch || (long)B * T * n > 2147483647L)
        return TVTS_EINVAL;
    hipLaunchKernelGGL(patch_gather_u8_ragged_kernel, dim3(B * T * n), dim3(256), 0, stream, src, desc, tables, keep, B, T, n, img,
                       patch, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], (bf16*)out, ldo);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---------------------------------------------------------------------------------------------- ViT token assemble
__global__ __launch_bounds__(256) void vit_assemble_kernel(const float* __restrict__ patch, int ldp,
                                                           const float* __restrict__ cls, const float* __restrict__ pos,
                                                           const float* __restrict__ temporal, const int* __restrict__ keep,
                                                           int keep_per_frame, int B, int T, int n, int W,
                                                           float* __restrict__ tok, int ldt) {
    const int S = 1 + T * n;
    const int row = blockIdx.x;  // b*S + s
    const int b = row / S, s = row % S;
    for (int c = threadIdx.x * 4; c < W; c += 1024) {
        f32x4 v;
        if (s == 0) {
            v = *(const f32x4*)(cls + c) + *(const f32x4*)(pos + c);
        } else {
            const int f = (s - 1) / n, i = (s - 1) % n;
            v = *(const f32x4*)(patch + (size_t)((b * T + f) * n + i) * ldp + c) +
                *(const f32x4*)(pos + (size_t)(1 + keep[keep_per_frame ? (b * T + f) * n + i : b * n + i]) * W + c) +
                *(const f32x4*)(temporal + (size_t)f * W + c);
        }
        *(f32x4*)(tok + (size_t)row * ldt + c) = v;
    }
}

extern "C" int tvts_vit_assemble(const float* patch, int ldp, const float* cls, const float* pos, const float* temporal,
                                 const int* keep, int keep_per_frame, int B, int T, int n, int W, float* tok, int ldt,
                                 hipStream_t stream) {
    if (W % 4 || ldp % 4 || ldt % 4) return TVTS_EINVAL;
    hipLaunchKernelGGL(vit_assemble_kernel, dim3(B * (1 + T * n)), dim3(256), 0, stream, patch, ldp, cls, pos, temporal,
                       keep, keep_per_frame, B, T, n, W, tok, ldt);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// one block per (b, f): d_patch rows (bf16, compact im2col row order), dpos scatter, dtemporal / dcls sums
__global__ __launch_bounds__(256) void vit_assemble_bwd_kernel(const float* __restrict__ dtok, int ldt,
                                                               const int* __restrict__ keep, int keep_per_frame, int B, int T,
                                                               int n, int W, bf16* __restrict__ dpatch, int ldp,
                                                               float* __restrict__ dcls,
                                                               float* __restrict__ dpos, float* __restrict__ dtemporal,
                                                               float* __restrict__ part_t, float* __restrict__ part_c,
                                                               float* __restrict__ part_p) {
    // part_t [B][T][W] / part_c [B][W] / part_p [B * T][n][W] (optional, all or none): the block's sums and its slot values go to
    // partials that colsum_partials_kernel / pos_rows_from_partials_kernel add in a fixed order, instead of fp32 atomics
    const int S = 1 + T * n;
    const int b = blockIdx.x / T, f = blockIdx.x % T;
    for (int c = threadIdx.x; c < W; c += 256) {
        float ts = 0.f;
        for (int i = 0; i < n; ++i) {
            const float v = dtok[(size_t)(b * S + 1 + f * n + i) * ldt + c];
            dpatch[(size_t)((b * T + f) * n + i) * ldp + c] = (bf16)v;
            if (part_p) part_p[((size_t)(b * T + f) * n + i) * W + c] = v;
            else atomicAdd(dpos + (size_t)(1 + keep[keep_per_frame ? (b * T + f) * n + i : b * n + i]) * W + c, v);
            ts += v;
        }
        if (part_t) part_t[((size_t)b * T + f) * W + c] = ts;
        else atomicAdd(dtemporal + (size_t)f * W + c, ts);
        if (f == 0) {
            const float v0 = dtok[(size_t)(b * S) * ldt + c];
            if (part_c) part_c[(size_t)b * W + c] = v0;
            else { atomicAdd(dcls + c, v0); atomicAdd(dpos + c, v0); }
        }
    }
}

// tube masks (one keep list per clip, shared by its frames -- the TVTSv2 batch): a block per (clip, group of ASM_SLOTS patch
// slots) sweeps the T frames of a slot, so that the positional-embedding gradient gets ONE atomic per (slot, column) instead of
// one per frame, and the temporal-embedding sums stay in registers over the block's slots (116 M -> 23 M fp32 atomics at 192
// clips x 8 frames x 98 patches x 768 columns: the atomics were the kernel's run time, 465 us); 16-byte loads, 8-byte stores.
#define ASM_SLOTS 14
#define ASM_MAXT 16
// part_t / part_c (optional): per-block partials [B * groups][T][W] of the temporal-embedding sums and [B][W] of the CLS rows,
// added in block order by colsum_partials_kernel (no atomics: the sums are run-to-run reproducible).  part_p (optional): the
// frame sums of every kept patch slot [B][n][W]; pos_rows_from_partials_kernel then adds, for every row of the positional
// embedding, the slots that point at it in clip order.  Without part_p the rows are a scatter of fp32 atomics.
__global__ __launch_bounds__(256) void vit_assemble_bwd_tube_kernel(const float* __restrict__ dtok, int ldt,
                                                                    const int* __restrict__ keep, int B, int T, int n, int W,
                                                                    bf16* __restrict__ dpatch, int ldp, float* __restrict__ dcls,
                                                                    float* __restrict__ dpos, float* __restrict__ dtemporal,
                                                                    float* __restrict__ part_t, float* __restrict__ part_c,
                                                                    float* __restrict__ part_p) {
    const int S = 1 + T * n;
    const int groups = (n + ASM_SLOTS - 1) / ASM_SLOTS;
    const int b = blockIdx.x / groups, grp = blockIdx.x % groups;
    const int i0 = grp * ASM_SLOTS, i1 = (i0 + ASM_SLOTS < n) ? i0 + ASM_SLOTS : n;
    for (int c = threadIdx.x * 4; c < W; c += 1024) {
        f32x4 ts[ASM_MAXT];
#pragma unroll
        for (int f = 0; f < ASM_MAXT; ++f) ts[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int i = i0; i < i1; ++i) {
            f32x4 ps = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int f = 0; f < ASM_MAXT; ++f) {
                if (f < T) {
                    const f32x4 v = *(const f32x4*)(dtok + (size_t)(b * S + 1 + f * n + i) * ldt + c);
                    *(bf16x4*)(dpatch + (size_t)((b * T + f) * n + i) * ldp + c) = (bf16x4){(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
                    ps += v;
                    ts[f] += v;
                }
            }
            if (part_p) {
                *(f32x4*)(part_p + ((size_t)b * n + i) * W + c) = ps;
            } else {
                float* dp = dpos + (size_t)(1 + keep[b * n + i]) * W + c;
#pragma unroll
                for (int e = 0; e < 4; ++e) atomicAdd(dp + e, ps[e]);
            }
        }
#pragma unroll
        for (int f = 0; f < ASM_MAXT; ++f) {
            if (f < T) {
                if (part_t) *(f32x4*)(part_t + ((size_t)blockIdx.x * T + f) * W + c) = ts[f];
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) atomicAdd(dtemporal + (size_t)f * W + c + e, ts[f][e]);
                }
            }
        }
        if (grp == 0) {
            const f32x4 v0 = *(const f32x4*)(dtok + (size_t)(b * S) * ldt + c);
            if (part_c) *(f32x4*)(part_c + (size_t)b * W + c) = v0;
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) { atomicAdd(dcls + c + e, v0[e]); atomicAdd(dpos + c + e, v0[e]); }
            }
        }
    }
}

// out[c] (and out2[c]) += sum_p part[p][c] for c < W: 64 columns x 16 partial-groups per block, every thread adds its partials
// in order, the 16 groups are combined in order
__global__ __launch_bounds__(1024) void colsum_partials_kernel(const float* __restrict__ part, int nparts, int W,
                                                               float* __restrict__ out, float* __restrict__ out2) {
    __shared__ float acc[16][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), grp = threadIdx.x >> 6;
    float s = 0.f;
    if (c < W)
        for (int p = grp; p < nparts; p += 16) s += part[(size_t)p * W + c];
    acc[grp][threadIdx.x & 63] = s;
    __syncthreads();
    if (grp == 0 && c < W) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) t += acc[g][threadIdx.x];
        out[c] += t;
        if (out2) out2[c] += t;
    }
}

// dpos[1 + r] += sum over the clips b of the slot sums part_p[b][i] with keep[b][i] == r, in a fixed order: a block per (row r of the
// positional embedding, 256 columns).  Its threads first look up "their" clip's slot (256 clips at a time; a tube mask holds a
// position at most once, further matches of a malformed one are added too); then 4 thread groups take every 4th clip, a thread
// four columns, and the groups are combined in group order.
__global__ __launch_bounds__(256) void pos_rows_from_partials_kernel(const float* __restrict__ part_p, const int* __restrict__ keep,
                                                                     int B, int n, int W, float* __restrict__ dpos) {
    __shared__ int first[256], more[256];
    __shared__ f32x4 comb[256];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int grp = tid >> 6, c = blockIdx.y * 256 + (tid & 63) * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int b0 = 0; b0 < B; b0 += 256) {
        int f = -1, cnt = 0;
        if (b0 + tid < B) {
            const int* kp = keep + (size_t)(b0 + tid) * n;
            for (int i = 0; i < n; ++i)
                if (kp[i] == r) { if (f < 0) f = i; ++cnt; }
        }
        first[tid] = f; more[tid] = cnt > 1;
        __syncthreads();
        const int nb = B - b0 < 256 ? B - b0 : 256;
        if (c < W) {
            for (int k = grp; k < nb; k += 4) {
                const int fi = first[k];
                if (fi < 0) continue;
                acc += *(const f32x4*)(part_p + ((size_t)(b0 + k) * n + fi) * W + c);
                if (more[k]) {
                    const int* kp = keep + (size_t)(b0 + k) * n;
                    for (int i = fi + 1; i < n; ++i)
                        if (kp[i] == r) acc += *(const f32x4*)(part_p + ((size_t)(b0 + k) * n + i) * W + c);
                }
            }
        }
        __syncthreads();
    }
    comb[tid] = acc;
    __syncthreads();
    if (grp == 0 && c < W) {
        const f32x4 t = ((comb[tid] + comb[64 + tid]) + comb[128 + tid]) + comb[192 + tid];
        *(f32x4*)(dpos + (size_t)(1 + r) * W + c) += t;
    }
}

extern "C" int tvts_vit_assemble_bwd(const float* dtok, int ldt, const int* keep, int keep_per_frame, int B, int T, int n, int W,
                                     void* dpatch, int ldp, float* dcls, float* dpos, int n_pos, float* dtemporal, float* workspace,
                                     long workspace_elems, hipStream_t stream) {
    if (!keep_per_frame && T <= ASM_MAXT && W % 4 == 0 && ldt % 4 == 0 && ldp % 4 == 0) {
        const int groups = (n + ASM_SLOTS - 1) / ASM_SLOTS;
        const long need = (long)B * groups * T * W + (long)B * W;
        float* part_t = (workspace && workspace_elems >= need) ? workspace : nullptr;
        float* part_c = part_t ? workspace + (size_t)B * groups * T * W : nullptr;
        float* part_p = (part_t && n_pos > 0 && workspace_elems >= need + (long)B * n * W) ? workspace + need : nullptr;
        hipLaunchKernelGGL(vit_assemble_bwd_tube_kernel, dim3(B * groups), dim3(256), 0, stream, dtok, ldt, keep, B, T, n, W,
                           (bf16*)dpatch, ldp, dcls, dpos, dtemporal, part_t, part_c, part_p);
        if (part_p)
            hipLaunchKernelGGL(pos_rows_from_partials_kernel, dim3(n_pos, ceil_div(W, 256)), dim3(256), 0, stream, part_p, keep, B, n, W, dpos);
        if (part_t) {
            hipLaunchKernelGGL(colsum_partials_kernel, dim3(ceil_div(T * W, 64)), dim3(1024), 0, stream, part_t, B * groups, T * W,
                               dtemporal, (float*)nullptr);
            hipLaunchKernelGGL(colsum_partials_kernel, dim3(ceil_div(W, 64)), dim3(1024), 0, stream, part_c, B, W, dcls, dpos);
        }
        TVTS_LAUNCH_CHECK();
        return TVTS_OK;
    }
    {   // one keep list per frame / tubelet (v1), or shapes the tube kernel does not take
        const long need = (long)B * T * W + (long)B * W + (long)B * T * n * W;
        const bool ordered = workspace && workspace_elems >= need && n_pos > 0 && keep_per_frame && W % 4 == 0;
        float* part_t = ordered ? workspace : nullptr;
        float* part_c = ordered ? part_t + (size_t)B * T * W : nullptr;
        float* part_p = ordered ? part_c + (size_t)B * W : nullptr;
        hipLaunchKernelGGL(vit_assemble_bwd_kernel, dim3(B * T), dim3(256), 0, stream, dtok, ldt, keep, keep_per_frame, B, T, n, W,
                           (bf16*)dpatch, ldp, dcls, dpos, dtemporal, part_t, part_c, part_p);
        if (ordered) {
            // the (clip, frame) pairs are the gather's "clips": keep[B * T][n], slot values [B * T][n][W]
            hipLaunchKernelGGL(pos_rows_from_partials_kernel, dim3(n_pos, ceil_div(W, 256)), dim3(256), 0, stream, part_p, keep, B * T, n, W, dpos);
            hipLaunchKernelGGL(colsum_partials_kernel, dim3(ceil_div(T * W, 64)), dim3(1024), 0, stream, part_t, B, T * W,
                               dtemporal, (float*)nullptr);
            hipLaunchKernelGGL(colsum_partials_kernel, dim3(ceil_div(W, 64)), dim3(1024), 0, stream, part_c, B, W, dcls, dpos);
        }
    }
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---------------------------------------------------------------------------------------------- text embedding
__global__ __launch_bounds__(256) void text_embed_kernel(const int* __restrict__ ids, int ld_ids, int N, int L,
                                                         const float* __restrict__ emb, const float* __restrict__ pos,
                                                         int Wt, float* __restrict__ x, int ldx) {
    const int row = blockIdx.x;  // n*L + l
    const int nn = row / L, l = row % L;
    const int id = ids[(size_t)nn * ld_ids + l];
    for (int c = threadIdx.x * 4; c < Wt; c += 1024)
        *(f32x4*)(x + (size_t)row * ldx + c) = *(const f32x4*)(emb + (size_t)id * Wt + c) + *(const f32x4*)(pos + (size_t)l * Wt + c);
}
extern "C" int tvts_text_embed(const int* ids, int ld_ids, int N, int L, const float* emb, const float* pos, int Wt,
                               float* x, int ldx, hipStream_t stream) {
    if (Wt % 4 || ldx % 4) return TVTS_EINVAL;
    hipLaunchKernelGGL(text_embed_kernel, dim3(N * L), dim3(256), 0, stream, ids, ld_ids, N, L, emb, pos, Wt, x, ldx);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
// the same for PACKED captions: row r of ids [M] belongs to the sequence i with seq_start[i] <= r < seq_start[i + 1] (binary search,
// block-uniform) and sits at position r - seq_start[i] of it.  A row whose position or token id is out of range is left unwritten.
__global__ __launch_bounds__(128) void text_embed_packed_kernel(const int* __restrict__ ids, const int* __restrict__ seq_start, int N,
                                                                const float* __restrict__ emb, const float* __restrict__ pos,
                                                                int Wt, int vocab, int context, float* __restrict__ x, int ldx) {
    const int row = blockIdx.x;
    int lo = 0, hi = N;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seq_start[mid] <= row) lo = mid; else hi = mid;
    }
    const int l = row - seq_start[lo], id = ids[row];
    if (l < 0 || l >= context || id < 0 || id >= vocab) return;
    for (int c = threadIdx.x * 4; c < Wt; c += 512)
        *(f32x4*)(x + (size_t)row * ldx + c) = *(const f32x4*)(emb + (size_t)id * Wt + c) + *(const f32x4*)(pos + (size_t)l * Wt + c);
}
extern "C" int tvts_text_embed_packed(const int* ids, const int* seq_start, int N, int M, const float* emb, const float* pos, int Wt,
                                      int vocab, int context, float* x, int ldx, hipStream_t stream) {
    if (!ids || !seq_start || !emb || !pos || !x || N <= 0 || M <= 0 || vocab <= 0 || context <= 0 || Wt <= 0 || Wt % 4 || ldx % 4 ||
        ldx < Wt)
        return TVTS_EINVAL;
    hipLaunchKernelGGL(text_embed_packed_kernel, dim3(M), dim3(128), 0, stream, ids, seq_start, N, emb, pos, Wt, vocab, context, x, ldx);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
__global__ __launch_bounds__(256) void text_embed_bwd_kernel(const float* __restrict__ dx, int ldx, const int* __restrict__ ids,
                                                             int ld_ids, int N, int L, int Wt, float* __restrict__ demb,
                                                             float* __restrict__ dpos) {
    const int row = blockIdx.x;
    const int nn = row / L, l = row % L;
    const int id = ids[(size_t)nn * ld_ids + l];
    for (int c = threadIdx.x; c < Wt; c += 256) {
        const float v = dx[(size_t)row * ldx + c];
        if (v != 0.f) {
            atomicAdd(demb + (size_t)id * Wt + c, v);
            atomicAdd(dpos + (size_t)l * Wt + c, v);
        }
    }
}
// the same sums without atomics (run-to-run reproducible).  Positions: dpos[l] += sum_n dx[n * L + l], a block per (64 columns,
// position), 16 thread groups over the captions, each in caption order, combined in group order.
__global__ __launch_bounds__(1024) void text_pos_bwd_kernel(const float* __restrict__ dx, int ldx, int N, int L, int Wt,
                                                            float* __restrict__ dpos) {
    __shared__ float acc[16][64];
    const int l = blockIdx.y, c = blockIdx.x * 64 + (threadIdx.x & 63), grp = threadIdx.x >> 6;
    float s = 0.f;
    if (c < Wt)
        for (int nn = grp; nn < N; nn += 16) s += dx[((size_t)nn * L + l) * ldx + c];
    acc[grp][threadIdx.x & 63] = s;
    __syncthreads();
    if (grp == 0 && c < Wt) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) t += acc[g][threadIdx.x];
        dpos[(size_t)l * Wt + c] += t;
    }
}
// Tokens: the caller hands over the rows sorted by token id (`order`, ties in row order) and the starts of the runs of equal ids
// (`seg`, N * L + 1 entries, padded with N * L: a fixed grid, empty runs exit).  A block per run adds its rows in order --
// G = 256 / (Wt / 4) thread groups take every G-th row, each thread four columns, the groups are combined in group order.
#define TOK_LONG_RUN 64     // a run of more rows than this, listed among the first TOK_LONG_SLOTS runs, is summed by a block per 64 columns
#define TOK_LONG_SLOTS 64
__global__ __launch_bounds__(256) void text_tok_bwd_kernel(const float* __restrict__ dx, int ldx, const int* __restrict__ ids,
                                                           int ld_ids, int L, int Wt, const int* __restrict__ order,
                                                           const int* __restrict__ seg, float* __restrict__ demb, int vocab) {
    __shared__ f32x4 part[256];
    const int lo = seg[blockIdx.x], hi = seg[blockIdx.x + 1];
    if (lo >= hi) return;
    if (hi - lo > TOK_LONG_RUN && blockIdx.x < TOK_LONG_SLOTS) return;  // text_tok_long_bwd_kernel's
    const int row0 = order[lo];
    const int id = ids[(size_t)(row0 / L) * ld_ids + row0 % L];
    if ((unsigned)id >= (unsigned)vocab) return;  // (block-uniform; the packed form's guard, INT_MAX in the rectangular one)
    const int cpt = Wt / 4 < 256 ? Wt / 4 : 256;  // column-threads per group
    const int G = 256 / cpt, grp = threadIdx.x / cpt, ct = threadIdx.x % cpt;
    for (int c0 = 0; c0 < Wt; c0 += cpt * 4) {
        const int c = c0 + ct * 4;
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        if (grp < G && c < Wt) {
            // sixteen rows in flight (the two id runs every caption shares -- start and end token -- are N rows long): the row
            // numbers first, then the rows (clamped, not predicated: a branch per load would serialise them), added in row order
            for (int k = lo + grp; k < hi; k += 16 * G) {
                int idx[16];
                f32x4 v[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int kk = k + u * G;
                    idx[u] = order[kk < hi ? kk : hi - 1];
                }
#pragma unroll
                for (int u = 0; u < 16; ++u) v[u] = *(const f32x4*)(dx + (size_t)idx[u] * ldx + c);
#pragma unroll
                for (int u = 0; u < 16; ++u)
                    if (k + u * G < hi) a += v[u];
            }
        }
        part[threadIdx.x] = a;
        __syncthreads();
        if (grp == 0 && c < Wt) {
            f32x4 t = part[ct];
            for (int g = 1; g < G; ++g) t += part[g * cpt + ct];
            *(f32x4*)(demb + (size_t)id * Wt + c) += t;
        }
        __syncthreads();
    }
}
// the long runs (every caption's start / end token: N rows each): a block per (run, 64 columns), 16 thread groups over the rows,
// a thread four columns, sixteen rows in flight per thread, the groups combined in group order
__global__ __launch_bounds__(256) void text_tok_long_bwd_kernel(const float* __restrict__ dx, int ldx, const int* __restrict__ ids,
                                                                int ld_ids, int L, int Wt, const int* __restrict__ order,
                                                                const int* __restrict__ seg, float* __restrict__ demb, int vocab) {
    __shared__ f32x4 part[256];
    const int lo = seg[blockIdx.x], hi = seg[blockIdx.x + 1];
    if (hi - lo <= TOK_LONG_RUN) return;
    const int row0 = order[lo];
    const int id = ids[(size_t)(row0 / L) * ld_ids + row0 % L];
    if ((unsigned)id >= (unsigned)vocab) return;
    const int grp = threadIdx.x >> 4, c = blockIdx.y * 64 + (threadIdx.x & 15) * 4;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (c < Wt) {
        for (int k = lo + grp; k < hi; k += 16 * 16) {
            int idx[16];
            f32x4 v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int kk = k + u * 16;
                idx[u] = order[kk < hi ? kk : hi - 1];
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = *(const f32x4*)(dx + (size_t)idx[u] * ldx + c);
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (k + u * 16 < hi) a += v[u];
        }
    }
    part[threadIdx.x] = a;
    __syncthreads();
    if (grp == 0 && c < Wt) {
        f32x4 t = part[threadIdx.x];
        for (int g = 1; g < 16; ++g) t += part[g * 16 + threadIdx.x];
        *(f32x4*)(demb + (size_t)id * Wt + c) += t;
    }
}
extern "C" int tvts_text_embed_bwd(const float* dx, int ldx, const int* ids, int ld_ids, int N, int L, int Wt, float* demb,
                                   float* dpos, const int* order, const int* seg, hipStream_t stream) {
    if (order != nullptr && seg != nullptr && Wt % 4 == 0 && ldx % 4 == 0) {
        hipLaunchKernelGGL(text_pos_bwd_kernel, dim3(ceil_div(Wt, 64), L), dim3(1024), 0, stream, dx, ldx, N, L, Wt, dpos);
        hipLaunchKernelGGL(text_tok_bwd_kernel, dim3(N * L), dim3(256), 0, stream, dx, ldx, ids, ld_ids, L, Wt, order, seg, demb, 0x7fffffff);
        const int slots = N * L < TOK_LONG_SLOTS ? N * L : TOK_LONG_SLOTS;
        hipLaunchKernelGGL(text_tok_long_bwd_kernel, dim3(slots, ceil_div(Wt, 64)), dim3(256), 0, stream, dx, ldx, ids, ld_ids, L, Wt,
                           order, seg, demb, 0x7fffffff);
    } else {
        hipLaunchKernelGGL(text_embed_bwd_kernel, dim3(N * L), dim3(256), 0, stream, dx, ldx, ids, ld_ids, N, L, Wt, demb, dpos);
    }
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// the same for PACKED captions (ids int32 [M], seq_start as for tvts_text_embed_packed): ordered sums only.  Tokens: the two kernels
// above read a flat ids as one caption of M tokens (row -> ids[row]); an id outside [0, vocab) writes nothing.  Positions: the caller
// hands over the rows sorted stably by their position inside their caption (`pos_order`) and the context + 1 starts of the runs of
// equal position (`pos_seg`); a block per (64 columns, position) adds its rows -- 16 thread groups, each in row order, combined in
// group order.  A row that does not sit at the block's position according to seq_start is not added (a plan that does not belong to
// the descriptor cannot put a gradient into another position's row).
__global__ __launch_bounds__(1024) void text_pos_bwd_packed_kernel(const float* __restrict__ dx, int ldx, const int* __restrict__ seq_start,
                                                                   int N, int M, int Wt, const int* __restrict__ pos_order,
                                                                   const int* __restrict__ pos_seg, float* __restrict__ dpos) {
    __shared__ float acc[16][64];
    const int l = blockIdx.y, c = blockIdx.x * 64 + (threadIdx.x & 63), grp = threadIdx.x >> 6;
    const int lo = pos_seg[l], hi = pos_seg[l + 1];
    if (lo >= hi || lo < 0 || hi > M) return;  // (block-uniform)
    float s = 0.f;
    if (c < Wt)
        for (int k = lo + grp; k < hi; k += 16) {
            const int r = pos_order[k];
            if (r < 0 || r >= M) continue;
            int a = 0, b = N;
            while (b - a > 1) {
                const int mid = (a + b) >> 1;
                if (seq_start[mid] <= r) a = mid; else b = mid;
            }
            if (r - seq_start[a] == l) s += dx[(size_t)r * ldx + c];
        }
    acc[grp][threadIdx.x & 63] = s;
    __syncthreads();
    if (grp == 0 && c < Wt) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) t += acc[g][threadIdx.x];
        dpos[(size_t)l * Wt + c] += t;
    }
}
extern "C" int tvts_text_embed_bwd_packed(const float* dx, int ldx, const int* ids, const int* seq_start, int N, int M, int Wt, int vocab,
                                          int context, float* demb, float* dpos, const int* tok_order, const int* tok_seg,
                                          const int* pos_order, const int* pos_seg, hipStream_t stream) {
    if (!dx || !ids || !seq_start || !demb || !dpos || !tok_order || !tok_seg || !pos_order || !pos_seg || N <= 0 || M <= 0 ||
        vocab <= 0 || context <= 0 || Wt <= 0 || Wt % 4 || ldx % 4 || ldx < Wt)
        return TVTS_EINVAL;
    hipLaunchKernelGGL(text_pos_bwd_packed_kernel, dim3(ceil_div(Wt, 64), context), dim3(1024), 0, stream, dx, ldx, seq_start, N, M, Wt,
                       pos_order, pos_seg, dpos);
    hipLaunchKernelGGL(text_tok_bwd_kernel, dim3(M), dim3(256), 0, stream, dx, ldx, ids, M, M, Wt, tok_order, tok_seg, demb, vocab);
    const int slots = M < TOK_LONG_SLOTS ? M : TOK_LONG_SLOTS;
    hipLaunchKernelGGL(text_tok_long_bwd_kernel, dim3(slots, ceil_div(Wt, 64)), dim3(256), 0, stream, dx, ldx, ids, M, M, Wt, tok_order,
                       tok_seg, demb, vocab);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---------------------------------------------------------------------------------------------- caption mean
__global__ void text_mean_kernel(const float* __restrict__ t, int NT, int B, int E, float* __restrict__ mean,
                                 float* __restrict__ before) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // (b, e)
    if (idx >= B * E) return;
    const int b = idx / E, e = idx % E;
    float s = 0.f;
    for (int i = 0; i < NT; ++i) {
        const float v = t[(size_t)(i * B + b) * E + e];
        s += v;
        if (before) before[((size_t)b * NT + i) * E + e] = v;
    }
    mean[idx] = s / (float)NT;
}
extern "C" int tvts_text_mean(const float* t, int NT, int B, int E, float* mean, float* before, hipStream_t stream) {
    hipLaunchKernelGGL(text_mean_kernel, dim3(ceil_div(B * E, 256)), dim3(256), 0, stream, t, NT, B, E, mean, before);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
__global__ void text_mean_bwd_kernel(const float* __restrict__ dmean, int NT, int B, int E, float* __restrict__ dt) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // (i, b, e)
    if (idx >= NT * B * E) return;
    const int e = idx % E, b = (idx / E) % B;
    dt[idx] = dmean[(size_t)b * E + e] / (float)NT;
}
extern "C" int tvts_text_mean_bwd(const float* dmean, int NT, int B, int E, float* dt, hipStream_t stream) {
    hipLaunchKernelGGL(text_mean_bwd_kernel, dim3(ceil_div(NT * B * E, 256)), dim3(256), 0, stream, dmean, NT, B, E, dt);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---------------------------------------------------------------------------------------------- sort head input
// xs[b, s] = tok[b*S + off + s] + type[0]  (s < Sv);  xs[b, Sv + i] = text[b, i] + type[1]
__global__ __launch_bounds__(256) void sort_assemble_kernel(const float* __restrict__ tok, int ldt, int S, int off, int Sv,
                                                            const float* __restrict__ text, int NT,
                                                            const float* __restrict__ type, int E, float* __restrict__ xs,
                                                            int ldx) {
    const int So = Sv + NT;
    const int row = blockIdx.x;
    const int b = row / So, s = row % So;
    const float* src = s < Sv ? tok + (size_t)(b * S + off + s) * ldt : text + ((size_t)b * NT + (s - Sv)) * E;
    const float* ty = type + (s < Sv ? 0 : E);
    for (int c = threadIdx.x * 4; c < E; c += 1024)
        *(f32x4*)(xs + (size_t)row * ldx + c) = *(const f32x4*)(src + c) + *(const f32x4*)(ty + c);
}
extern "C" int tvts_sort_assemble(const float* tok, int ldt, int B, int S, int off, int Sv, const float* text, int NT,
                                  const float* type, int E, float* xs, int ldx, hipStream_t stream) {
    if (E % 4 || ldt % 4 || ldx % 4) return TVTS_EINVAL;
    hipLaunchKernelGGL(sort_assemble_kernel, dim3(B * (Sv + NT)), dim3(256), 0, stream, tok, ldt, S, off, Sv, text, NT, type,
                       E, xs, ldx);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
// d_out[b*S + r] (bf16, feeds the output-projection dgrad/wgrad) = [r >= off ? dxs[b, r-off] : 0] + [r == 0 ? dvid[b] : 0]
// dtype[0] += sum over video rows, dtype[1] += sum over caption rows.
// grid (B, row chunks of 32): each block converts its rows and adds its partial column sums with atomics.
__global__ __launch_bounds__(256) void sort_assemble_bwd_kernel(const float* __restrict__ dxs, int ldx, int S, int off, int Sv,
                                                                int NT, const float* __restrict__ dvid, int E,
                                                                bf16* __restrict__ dout, int ldo, float* __restrict__ dtype,
                                                                float* __restrict__ part0, float* __restrict__ part1) {
    const int So = Sv + NT;
    const int b = blockIdx.x;
    const int r0 = blockIdx.y * 32;
    int r1 = r0 + 32;
    r1 = r1 < S ? r1 : S;
    for (int c = threadIdx.x; c < E; c += 256) {
        float s0 = 0.f, s1 = 0.f;
        for (int r = r0; r < r1; ++r) {
            float v = 0.f;
            if (dxs && r >= off) {
                v = dxs[(size_t)(b * So + r - off) * ldx + c];
                s0 += v;
            }
            if (r == 0 && dvid) v += dvid[(size_t)b * E + c];
            dout[(size_t)(b * S + r) * ldo + c] = (bf16)v;
        }
        if (dxs) {
            if (blockIdx.y == 0)
                for (int i = 0; i < NT; ++i) s1 += dxs[(size_t)(b * So + Sv + i) * ldx + c];
            if (part0) {  // per-block partials, added in block order by colsum_partials_kernel
                part0[((size_t)b * gridDim.y + blockIdx.y) * E + c] = s0;
                if (blockIdx.y == 0) part1[(size_t)b * E + c] = s1;
            } else if (dtype) {  // no dtype: only dout is wanted
                atomicAdd(dtype + c, s0);
                if (blockIdx.y == 0) atomicAdd(dtype + E + c, s1);
            }
        }
    }
}
// workspace (optional, >= B * (ceil(S / 32) + 1) * E floats): the type-embedding gradient (a plain sum over token rows, one of the
// lr 1e-4 parameters: its noise is what Adam amplifies) as ordered per-block partials instead of fp32 atomics
extern "C" int tvts_sort_assemble_bwd(const float* dxs, int ldx, int B, int S, int off, int Sv, int NT, const float* dvid,
                                      int E, void* dout, int ldo, float* dtype, float* workspace, long workspace_elems,
                                      hipStream_t stream) {
    const int chunks = ceil_div(S, 32);
    const bool parts = dxs && dtype && workspace && workspace_elems >= (long)B * (chunks + 1) * E;
    float* part0 = parts ? workspace : nullptr;
    float* part1 = parts ? workspace + (size_t)B * chunks * E : nullptr;
    hipLaunchKernelGGL(sort_assemble_bwd_kernel, dim3(B, chunks), dim3(256), 0, stream, dxs, ldx, S, off, Sv, NT, dvid,
                       E, (bf16*)dout, ldo, dtype, part0, part1);
    if (parts) {
        hipLaunchKernelGGL(colsum_partials_kernel, dim3(ceil_div(E, 64)), dim3(1024), 0, stream, part0, B * chunks, E, dtype,
                           (float*)nullptr);
        hipLaunchKernelGGL(colsum_partials_kernel, dim3(ceil_div(E, 64)), dim3(1024), 0, stream, part1, B, E, dtype + E,
                           (float*)nullptr);
    }
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---------------------------------------------------------------------------------------------- row gather/scatter (fp32)
// dst[r] = src[rows[r]]   (gather)   or   dst[rows[r]] += src[r]   (scatter_add)
__global__ void rows_gather_kernel(const float* __restrict__ src, int lds_, const int* __restrict__ rows, int R, int W,
                                   float* __restrict__ dst, int ldd, int scatter) {
    const int r = blockIdx.x;
    for (int c = threadIdx.x; c < W; c += blockDim.x) {
        if (scatter) dst[(size_t)rows[r] * ldd + c] += src[(size_t)r * lds_ + c];
        else dst[(size_t)r * ldd + c] = src[(size_t)rows[r] * lds_ + c];
    }
}
extern "C" int tvts_rows_gather(const float* src, int ld_src, const int* rows, int R, int W, float* dst, int ld_dst,
                                int scatter_add, hipStream_t stream) {
    if (R < 0 || W <= 0) return TVTS_EINVAL;
    if (R == 0) return TVTS_OK;  // no rows: a zero-block grid is not a valid launch
    if (!rows || !src || !dst) return TVTS_EINVAL;
    hipLaunchKernelGGL(rows_gather_kernel, dim3(R), dim3(256), 0, stream, src, ld_src, rows, R, W, dst, ld_dst, scatter_add);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---------------------------------------------------------------------------------------------- rows between a token-row matrix and a packed [R, W] one
// (the "used rows" blocks: the last block of the sort head / the text tower runs on the R rows the model reads, engine.py::_block_fwd / _block_bwd with rows)
//   mode 0 gather        packed[r] = full[rows[r]]: source full_f32 if given else full_bf16; packed_f32 and / or packed_bf16 written
//   mode 1 scatter       full[rows[r]] = packed[r], per element type given on BOTH sides
//   mode 2 scatter-add   full_f32[rows[r]] += packed_f32[r]; full_bf16[rows[r]] = bf16(that sum) when given (the bf16 copy of the row)
// rows are distinct (token rows of distinct captions / clips): no two blocks touch one row.
__global__ __launch_bounds__(256) void rows_move_kernel(int mode, const int* __restrict__ rows, int W, float* full_f32, int ldf,
                                                        bf16* full_bf16, int ldfb, float* packed_f32, int ldp, bf16* packed_bf16, int ldpb) {
    const int r = blockIdx.x;
    const size_t fr = (size_t)rows[r];
    for (int c = threadIdx.x; c < W; c += 256) {
        if (mode == 0) {
            const float v = full_f32 ? full_f32[fr * ldf + c] : (float)full_bf16[fr * ldfb + c];
            if (packed_f32) packed_f32[(size_t)r * ldp + c] = v;
            if (packed_bf16) packed_bf16[(size_t)r * ldpb + c] = full_f32 ? (bf16)v : full_bf16[fr * ldfb + c];
        } else if (mode == 1) {
            if (full_f32 && packed_f32) full_f32[fr * ldf + c] = packed_f32[(size_t)r * ldp + c];
            if (full_bf16 && packed_bf16) full_bf16[fr * ldfb + c] = packed_bf16[(size_t)r * ldpb + c];
        } else {
            const float v = full_f32[fr * ldf + c] + packed_f32[(size_t)r * ldp + c];
            full_f32[fr * ldf + c] = v;
            if (full_bf16) full_bf16[fr * ldfb + c] = (bf16)v;
        }
    }
}
extern "C" int tvts_rows_move(int mode, const int* rows, int R, int W, float* full_f32, int ld_full_f32, void* full_bf16, int ld_full_bf16,
                              float* packed_f32, int ld_packed_f32, void* packed_bf16, int ld_packed_bf16, hipStream_t stream) {
    if (!rows || R < 0 || W <= 0 || mode < 0 || mode > 2 || (!full_f32 && !full_bf16) || (!packed_f32 && !packed_bf16)) return TVTS_EINVAL;
    if (mode == 2 && (!full_f32 || !packed_f32)) return TVTS_EINVAL;
    if (mode == 1 && !((full_f32 && packed_f32) || (full_bf16 && packed_bf16))) return TVTS_EINVAL;
    if (R == 0) return TVTS_OK;
    hipLaunchKernelGGL(rows_move_kernel, dim3(R), dim3(256), 0, stream, mode, rows, W, full_f32, ld_full_f32, (bf16*)full_bf16, ld_full_bf16,
                       packed_f32, ld_packed_f32, (bf16*)packed_bf16, ld_packed_bf16);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
// a column range of a bf16 row-major matrix set to zero (dQ of the rows that are no queries in the used-rows attention backward)
__global__ __launch_bounds__(256) void zero_cols_bf16_kernel(bf16* x, int ld, long rows, int cols8) {
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4_;
    const long n = rows * cols8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long r = i / cols8;
        const int c = (int)(i - r * cols8);
        *(u32x4_*)(x + (size_t)r * ld + c * 8) = (u32x4_){0u, 0u, 0u, 0u};
    }
}
extern "C" int tvts_zero_cols_bf16(void* x, int ld, long rows, int cols, hipStream_t stream) {
    if (!x || rows < 0 || cols <= 0 || (cols % 8) || (ld % 8) || ((size_t)x % 16)) return TVTS_EINVAL;
    if (rows == 0) return TVTS_OK;
    const long n = rows * (cols / 8);
    long blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(zero_cols_bf16_kernel, dim3((int)blocks), dim3(256), 0, stream, (bf16*)x, ld, rows, cols / 8);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---------------------------------------------------------------------------------------------- hidden-state dropout (v1 text tower)
// out = x * m / (1 - p) (+ residual); m: element (r, c) is kept iff the upper 32 bits of splitmix64(seed + (r * cols + c) * phi)
// are >= p * 2^32 -- the generator of the attention-probability dropout (attention.hip::drop_keep)
__global__ __launch_bounds__(256) void dropout_rows_kernel(const float* __restrict__ x, int ldx, int rows, int cols, unsigned thr,
                                                           float inv, const unsigned long long* __restrict__ seed_dev,
                                                           unsigned long long site, const float* __restrict__ residual, int ldr,
                                                           float* __restrict__ out, int ldo, bf16* __restrict__ outb, int ldob) {
    const unsigned long long seed = seed_dev[0] + site;
    const long n = (long)rows * cols;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int r = (int)(i / cols), c = (int)(i % cols);
        unsigned long long z = seed + (unsigned long long)i * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        float v = ((unsigned)(z >> 32) >= thr) ? x[(size_t)r * ldx + c] * inv : 0.f;
        if (residual) v += residual[(size_t)r * ldr + c];
        if (out) out[(size_t)r * ldo + c] = v;
        if (outb) outb[(size_t)r * ldob + c] = (bf16)v;
    }
}
extern "C" int tvts_dropout_rows(const float* x, int ldx, int rows, int cols, float p, const long* seed_dev, long site,
                                 const float* residual, int ldr, float* out, int ldo, void* out_bf16, int ldob, hipStream_t stream) {
    if (!x || rows <= 0 || cols <= 0 || p < 0.f || p >= 1.f || !seed_dev || (!out && !out_bf16)) return TVTS_EINVAL;
    const long n = (long)rows * cols;
    int blocks = (int)((n + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(dropout_rows_kernel, dim3(blocks), dim3(256), 0, stream, x, ldx, rows, cols,
                       (unsigned)((double)p * 4294967296.0), 1.0f / (1.0f - p), (const unsigned long long*)seed_dev,
                       (unsigned long long)site, residual, ldr, out, ldo, (bf16*)out_bf16, ldob);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// the same over PACKED captions (x [M, cols], seq_start as for tvts_text_embed_packed): element (row r, column c) uses the counter of
// its PADDED position, ((i * L_pad + t) * cols + c) with r = seq_start[i] + t -- a packed call draws the mask tvts_dropout_rows draws
// on the [N * L_pad, cols] buffer of the padded step.  A block walks rows; the row's caption is one binary search (block-uniform).
// A row outside every caption or at a position t >= L_pad is left unwritten.
__global__ __launch_bounds__(256) void dropout_rows_packed_kernel(const float* __restrict__ x, int ldx, const int* __restrict__ seq_start,
                                                                  int N, int M, int cols, int L_pad, unsigned thr, float inv,
                                                                  const unsigned long long* __restrict__ seed_dev, unsigned long long site,
                                                                  const float* __restrict__ residual, int ldr, float* __restrict__ out,
                                                                  int ldo, bf16* __restrict__ outb, int ldob) {
    const unsigned long long seed = seed_dev[0] + site;
    for (int r = blockIdx.x; r < M; r += gridDim.x) {
        int lo = 0, hi = N;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (seq_start[mid] <= r) lo = mid; else hi = mid;
        }
        const int t = r - seq_start[lo];
        if (t < 0 || t >= L_pad || r >= seq_start[lo + 1]) continue;
        const unsigned long long i0 = ((unsigned long long)lo * L_pad + t) * cols;
        for (int c = threadIdx.x; c < cols; c += 256) {
            unsigned long long z = seed + (i0 + c) * 0x9E3779B97F4A7C15ull;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            float v = ((unsigned)(z >> 32) >= thr) ? x[(size_t)r * ldx + c] * inv : 0.f;
            if (residual) v += residual[(size_t)r * ldr + c];
            if (out) out[(size_t)r * ldo + c] = v;
            if (outb) outb[(size_t)r * ldob + c] = (bf16)v;
        }
    }
}
extern "C" int tvts_dropout_rows_packed(const float* x, int ldx, const int* seq_start, int N, int M, int cols, int L_pad, float p,
                                        const long* seed_dev, long site, const float* residual, int ldr, float* out, int ldo,
                                        void* out_bf16, int ldob, hipStream_t stream) {
    if (!x || !seq_start || N <= 0 || M <= 0 || cols <= 0 || L_pad <= 0 || !(p >= 0.f) || p >= 1.f || !seed_dev || (!out && !out_bf16))
        return TVTS_EINVAL;
    if (ldx < cols || (residual && ldr < cols) || (out && ldo < cols) || (out_bf16 && ldob < cols)) return TVTS_EINVAL;
    hipLaunchKernelGGL(dropout_rows_packed_kernel, dim3(M < 4096 ? M : 4096), dim3(256), 0, stream, x, ldx, seq_start, N, M, cols, L_pad,
                       (unsigned)((double)p * 4294967296.0), 1.0f / (1.0f - p), (const unsigned long long*)seed_dev,
                       (unsigned long long)site, residual, ldr, out, ldo, (bf16*)out_bf16, ldob);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---------------------------------------------------------------------------------------------- ReLU (v1 txt_proj)
// y = max(x, 0) / dx = dy * (x > 0): the nn.ReLU in front of the v1 text projection (v1/model/model_dist_TVTS.py:65-68)
__global__ void relu_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    out[i] = dy ? (v > 0.f ? dy[i] : 0.f) : (v > 0.f ? v : 0.f);
}
extern "C" int tvts_relu(const float* x, const float* dy, float* out, long n, hipStream_t stream) {
    if (n <= 0) return TVTS_EINVAL;
    hipLaunchKernelGGL(relu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, dy, out, n);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}

// ---------------------------------------------------------------------------------------------- tube mask on the device
// The reference draws the tube mask per sample in the dataset worker: a shuffled arange(ppf) cut to its first n_keep
// entries, shared by every frame of the clip (v2/data_loader/YTTemporal_dataset.py:207-213).  Here one block per sample
// gives every patch index a counter-based 54-bit random key (splitmix64 of seed, global sample number, patch index), sorts
// the (key, index) words in LDS and keeps the indices of the n_keep smallest: a uniformly random, unsorted permutation
// prefix, reproducible for (seed, sample number) whatever the batch split or the rank layout.
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void tube_mask_kernel(unsigned long long seed, unsigned long long first_sample, int ppf,
                                                        int n_keep, int p2, int* __restrict__ keep) {
    __shared__ unsigned long long w[1024];
    const unsigned long long base = splitmix64(seed + splitmix64(first_sample + blockIdx.x));
    for (int i = threadIdx.x; i < p2; i += 256)
        w[i] = i < ppf ? ((splitmix64(base + (unsigned long long)i) & ~0x3FFull) | (unsigned long long)i) : ~0ull;
    __syncthreads();
    for (int k = 2; k <= p2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < p2; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = w[i], b = w[l];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { w[i] = b; w[l] = a; }
                }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < n_keep; i += 256) keep[(size_t)blockIdx.x * n_keep + i] = (int)(w[i] & 0x3FFull);
}

extern "C" int tvts_tube_mask(long seed_, long first_sample_, int B, int ppf, int n_keep, int* keep, hipStream_t stream) {
    const unsigned long long seed = (unsigned long long)seed_, first_sample = (unsigned long long)first_sample_;
    if (B < 0 || ppf <= 0 || ppf > 1024 || n_keep < 0 || n_keep > ppf || (B > 0 && n_keep > 0 && keep == nullptr)) return TVTS_EINVAL;
    if (B == 0 || n_keep == 0) return TVTS_OK;
    int p2 = 2;
    while (p2 < ppf) p2 <<= 1;
    hipLaunchKernelGGL(tube_mask_kernel, dim3(B), dim3(256), 0, stream, seed, first_sample, ppf, n_keep, p2, keep);
    TVTS_LAUNCH_CHECK();
    return TVTS_OK;
}
