// RandAugment of the v1 action-recognition recipe (v1/downstream/rand_augment.py, --aa rand-m7-n4-mstd0.5-inc1) on uint8 frames at
// source size, with the bytes PIL gives: include/tvts_hip.h, "RandAugment", states the arithmetic.  One launch handles one layer of
// every view; tvts_randaug_hist counts the frames whose op needs statistics, tvts_randaug_apply runs the op.
//
// PIL's build does not contract a * b + c into an FMA and this build's -O3 does: the pragma below keeps every product and sum of
// this file a rounding of its own, which is what makes the bytes PIL's.  Types are PIL's too: double for coordinates and
// interpolation (Geometry.c), float for the blends (Blend.c) and the 3 x 3 filter (Filter.c), integers for the tables.
#include "common.h"

#pragma clang fp contract(off)

namespace {

enum { RA_NONE = 0, RA_AUTOCONTRAST, RA_EQUALIZE, RA_INVERT, RA_SOLARIZE, RA_SOLARIZE_ADD, RA_POSTERIZE, RA_COLOR, RA_CONTRAST,
       RA_BRIGHTNESS, RA_SHARPNESS, RA_AFFINE };
constexpr int RA_THREADS = 256;
constexpr int RA_TW = 64, RA_TH = 32;   // the apply tile: a thread owns one column of it and every fourth row
constexpr int RA_HIST_PIX = 8192;       // pixels per histogram block
constexpr int RA_MAX_LAYERS = 8;
constexpr int RA_BILINEAR = 2, RA_BICUBIC = 3;  // PIL's Image.BILINEAR / Image.BICUBIC

// the clip (row of the work tensor) layer `layer` reads view b from: its source clip, or the region the layer before wrote
__device__ __forceinline__ long ra_src_row(int b, int layer, int Bs, int B, int ns) {
    return layer == 0 ? b / ns : (long)Bs + (long)((layer - 1) & 1) * B + b;
}
__device__ __forceinline__ int ra_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }
__device__ __forceinline__ bool ra_needs_hist(int op) { return op == RA_AUTOCONTRAST || op == RA_EQUALIZE || op == RA_CONTRAST; }

// hist uint32 [B, T, 4 (R, G, B, L), 256], zeroed by the entry point: LDS integer atomics, then one global integer atomic per
// nonzero bin -- integer sums do not depend on their order
__global__ __launch_bounds__(RA_THREADS) void randaug_hist_kernel(const unsigned char* __restrict__ work, int Bs, int B, int ns, int T,
                                                                  int H0, int W0, int layer, int L, const int* __restrict__ ra_i,
                                                                  unsigned int* __restrict__ hist) {
    const int b = blockIdx.z, t = blockIdx.y;
    if (!ra_needs_hist(ra_i[((long)b * L + layer) * 4])) return;
    __shared__ unsigned int h[4 * 256];
    for (int i = threadIdx.x; i < 4 * 256; i += RA_THREADS) h[i] = 0;
    __syncthreads();
    const long npix = (long)H0 * W0;
    const unsigned char* fr = work + (ra_src_row(b, layer, Bs, B, ns) * T + t) * npix * 3;
    const long p0 = (long)blockIdx.x * RA_HIST_PIX, p1 = p0 + RA_HIST_PIX < npix ? p0 + RA_HIST_PIX : npix;
    for (long p = p0 + threadIdx.x; p < p1; p += RA_THREADS) {
        const int r = fr[3 * p], g = fr[3 * p + 1], bl = fr[3 * p + 2];
        atomicAdd(&h[r], 1u);
        atomicAdd(&h[256 + g], 1u);
        atomicAdd(&h[512 + bl], 1u);
        atomicAdd(&h[768 + ra_luma(r, g, bl)], 1u);
    }
    __syncthreads();
    unsigned int* out = hist + ((long)b * T + t) * 1024;
    for (int i = threadIdx.x; i < 4 * 256; i += RA_THREADS)
        if (h[i]) atomicAdd(&out[i], h[i]);
}

__device__ __forceinline__ unsigned char ra_clip8(float v) { return v <= 0.0f ? 0 : v >= 255.0f ? 255 : (unsigned char)(int)v; }

// Image.blend(degenerate, image, factor): Blend.c
__device__ __forceinline__ unsigned char ra_blend(int d, int i, float f, bool inside01) {
    const float t = (float)d + f * ((float)i - (float)d);
    return inside01 ? (unsigned char)(int)t : ra_clip8(t);
}

// Geometry.c BICUBIC
__device__ __forceinline__ double ra_cubic(double v1, double v2, double v3, double v4, double d) {
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}
__device__ __forceinline__ int ra_clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

__global__ __launch_bounds__(RA_THREADS) void randaug_apply_kernel(unsigned char* __restrict__ work, int Bs, int B, int ns, int T,
                                                                   int H0, int W0, int layer, int L, const int* __restrict__ ra_i,
                                                                   const double* __restrict__ ra_d,
                                                                   const unsigned int* __restrict__ hist) {
    const int b = blockIdx.z, t = blockIdx.y, tid = threadIdx.x;
    const int* ri = ra_i + ((long)b * L + layer) * 4;
    const double* rd = ra_d + ((long)b * L + layer) * 8;
    const int op = ri[0], resample = ri[1], iarg = ri[2];
    if (op <= RA_NONE || op > RA_AFFINE) return;                 // a view with no op left in this layer is not written
    if (ra_needs_hist(op) && !hist) return;
    if (op == RA_AFFINE && resample != RA_BILINEAR && resample != RA_BICUBIC) return;
    const long npix = (long)H0 * W0;
    const unsigned char* src = work + (ra_src_row(b, layer, Bs, B, ns) * T + t) * npix * 3;
    unsigned char* dst = work + (((long)Bs + (long)(layer & 1) * B + b) * T + t) * npix * 3;
    const unsigned int* h = hist ? hist + ((long)b * T + t) * 1024 : nullptr;

    __shared__ unsigned char lut[3][256];
    __shared__ int lo_hi[3][2];
    __shared__ int wave_lo_hi[3][RA_THREADS / 64][2];
    __shared__ int mean_l;
    __shared__ __attribute__((aligned(16))) unsigned int scan[2][3][256];
    // ---- the tables, every block its own
    if (op == RA_INVERT || op == RA_SOLARIZE || op == RA_SOLARIZE_ADD || op == RA_POSTERIZE) {
        const int i = tid;
        int v;
        if (op == RA_INVERT) v = 255 - i;
        else if (op == RA_SOLARIZE) v = i < iarg ? i : 255 - i;
        else if (op == RA_SOLARIZE_ADD) v = i < 128 ? (i + iarg > 255 ? 255 : i + iarg) : i;
        else v = iarg >= 8 ? i : iarg <= 0 ? 0 : i & ~((1 << (8 - iarg)) - 1);
        v = ra_clampi(v, 255);
        lut[0][i] = lut[1][i] = lut[2][i] = (unsigned char)v;
    } else if (ra_needs_hist(op)) {
        // the frame's histograms staged once: first / last nonzero bin from one ballot per wave, the running count by a scan
        const int nc = op == RA_CONTRAST ? 1 : 3;
        const unsigned int* hc = op == RA_CONTRAST ? h + 768 : h;
        unsigned int own[3] = {0, 0, 0};
        for (int c = 0; c < nc; ++c) {
            scan[0][c][tid] = own[c] = hc[256 * c + tid];
            const unsigned long long m = __ballot(own[c] != 0);
            if ((tid & 63) == 0) {
                wave_lo_hi[c][tid >> 6][0] = m ? (tid & ~63) + __ffsll((long long)m) - 1 : 256;
                wave_lo_hi[c][tid >> 6][1] = m ? (tid & ~63) + 63 - __clzll((long long)m) : -1;
            }
        }
        __syncthreads();
        if (tid < 3) {
            int lo = 256, hi = -1;
            for (int w = 0; w < RA_THREADS / 64; ++w) {
                lo = wave_lo_hi[tid][w][0] < lo ? wave_lo_hi[tid][w][0] : lo;
                hi = wave_lo_hi[tid][w][1] > hi ? wave_lo_hi[tid][w][1] : hi;
            }
            lo_hi[tid][0] = lo, lo_hi[tid][1] = hi;
        }
        if (op == RA_CONTRAST) {   // sum of i * h[i] and of h[i]: a tree over exact 64-bit integers
            unsigned long long* sum = (unsigned long long*)&scan[0][0][0];  // [2][256] over the staging, which is no longer read
            __syncthreads();
            sum[tid] = (unsigned long long)tid * own[0];
            sum[256 + tid] = own[0];
            __syncthreads();
            for (int off = 128; off > 0; off >>= 1) {
                if (tid < off) sum[tid] += sum[tid + off], sum[256 + tid] += sum[256 + tid + off];
                __syncthreads();
            }
            if (tid == 0) mean_l = sum[256] ? (int)((double)sum[0] / (double)sum[256] + 0.5) : 0;  // int(ImageStat.Stat(L).mean[0] + 0.5)
        } else if (op == RA_AUTOCONTRAST) {
            __syncthreads();
            for (int c = 0; c < 3; ++c) {
                const int lo = lo_hi[c][0], hi = lo_hi[c][1];
                int v = tid;
                if (hi > lo) {
                    const double scale = 255.0 / (double)(hi - lo);
                    const double off = (double)(-lo) * scale;
                    v = ra_clampi((int)((double)tid * scale + off), 255);
                }
                lut[c][tid] = (unsigned char)v;
            }
        } else {  // RA_EQUALIZE
            int cur = 0;
            for (int off = 1; off < 256; off <<= 1) {   // inclusive scan of the three histograms
                for (int c = 0; c < 3; ++c)
                    scan[cur ^ 1][c][tid] = scan[cur][c][tid] + (tid >= off ? scan[cur][c][tid - off] : 0u);
                __syncthreads();
                cur ^= 1;
            }
            for (int c = 0; c < 3; ++c) {
                const int lo = lo_hi[c][0], hi = lo_hi[c][1];
                unsigned int v = tid;
                if (hi > lo) {  // more than one nonzero bin
                    const unsigned int total = scan[cur][c][255], last = scan[cur][c][hi] - scan[cur][c][hi - 1];
                    const unsigned int step = (total - last) / 255u;
                    if (step) {
                        const unsigned long long n = (unsigned long long)(step / 2u) + (scan[cur][c][tid] - own[c]);  // + the bins below
                        const unsigned long long q = n / step;
                        v = q > 255 ? 255u : (unsigned int)q;
                    }
                }
                lut[c][tid] = (unsigned char)v;
            }
        }
    }
    __syncthreads();

    const int tiles_x = (W0 + RA_TW - 1) / RA_TW;
    const int x = (blockIdx.x % tiles_x) * RA_TW + (tid & (RA_TW - 1));
    const int y_first = (blockIdx.x / tiles_x) * RA_TH + tid / RA_TW;
    if (x >= W0) return;
    const float f = (float)rd[6];
    const bool inside01 = f >= 0.0f && f <= 1.0f;
    const float k1 = (float)(1.0 / 13.0), k5 = (float)(5.0 / 13.0);
    const double ca = rd[0], cb = rd[1], cc = rd[2], cd = rd[3], ce = rd[4], cf = rd[5];
    const long row = (long)W0 * 3;

    for (int yy = 0; yy < RA_TH; yy += RA_THREADS / RA_TW) {
        const int y = y_first + yy;
        if (y >= H0) break;
        const unsigned char* s = src + y * row + 3 * x;
        unsigned char o0, o1, o2;
        if (op <= RA_POSTERIZE) {
            o0 = lut[0][s[0]], o1 = lut[1][s[1]], o2 = lut[2][s[2]];
        } else if (op == RA_COLOR) {
            const int l = ra_luma(s[0], s[1], s[2]);
            o0 = ra_blend(l, s[0], f, inside01), o1 = ra_blend(l, s[1], f, inside01), o2 = ra_blend(l, s[2], f, inside01);
        } else if (op == RA_CONTRAST || op == RA_BRIGHTNESS) {
            const int d = op == RA_CONTRAST ? mean_l : 0;
            o0 = ra_blend(d, s[0], f, inside01), o1 = ra_blend(d, s[1], f, inside01), o2 = ra_blend(d, s[2], f, inside01);
        } else if (op == RA_SHARPNESS) {
            int d[3] = {s[0], s[1], s[2]};
            if (x >= 1 && x < W0 - 1 && y >= 1 && y < H0 - 1) {   // ImageFilter.SMOOTH; the one-pixel border is the frame's
                for (int c = 0; c < 3; ++c) {
                    const unsigned char* below = s + row + c;
                    const unsigned char* here = s + c;
                    const unsigned char* above = s - row + c;
                    float ss = 0.5f;
                    ss += ((float)below[-3] * k1 + (float)below[0] * k1) + (float)below[3] * k1;
                    ss += ((float)here[-3] * k1 + (float)here[0] * k5) + (float)here[3] * k1;
                    ss += ((float)above[-3] * k1 + (float)above[0] * k1) + (float)above[3] * k1;
                    d[c] = ra_clip8(ss);
                }
            }
            o0 = ra_blend(d[0], s[0], f, inside01), o1 = ra_blend(d[1], s[1], f, inside01), o2 = ra_blend(d[2], s[2], f, inside01);
        } else {  // RA_AFFINE: Geometry.c affine_transform + bilinear_filter32RGB / bicubic_filter32RGB, fill (128, 128, 128)
            double xin = ca * ((double)x + 0.5) + cb * ((double)y + 0.5) + cc;
            double yin = cd * ((double)x + 0.5) + ce * ((double)y + 0.5) + cf;
            o0 = o1 = o2 = 128;
            if (xin >= 0.0 && xin < (double)W0 && yin >= 0.0 && yin < (double)H0) {
                xin -= 0.5;
                yin -= 0.5;
                const int xi = (int)floor(xin), yi = (int)floor(yin);
                const double dx = xin - (double)xi, dy = yin - (double)yi;
                unsigned char o[3];
                if (resample == RA_BILINEAR) {
                    const unsigned char* r0 = src + ra_clampi(yi, H0 - 1) * row;
                    const unsigned char* r1 = src + ra_clampi(yi + 1, H0 - 1) * row;
                    const int x0 = 3 * ra_clampi(xi, W0 - 1), x1 = 3 * ra_clampi(xi + 1, W0 - 1);
                    for (int c = 0; c < 3; ++c) {
                        const double v1 = (double)r0[x0 + c] + (double)((int)r0[x1 + c] - (int)r0[x0 + c]) * dx;
                        const double v2 = (double)r1[x0 + c] + (double)((int)r1[x1 + c] - (int)r1[x0 + c]) * dx;
                        const double v = v1 + (v2 - v1) * dy;
                        o[c] = (unsigned char)(int)v;
                    }
                } else {
                    int xo[4];
                    const unsigned char* rr[4];
                    for (int k = 0; k < 4; ++k) {
                        xo[k] = 3 * ra_clampi(xi - 1 + k, W0 - 1);
                        rr[k] = src + ra_clampi(yi - 1 + k, H0 - 1) * row;
                    }
                    for (int c = 0; c < 3; ++c) {
                        double v[4];
                        for (int k = 0; k < 4; ++k)
                            v[k] = ra_cubic((double)rr[k][xo[0] + c], (double)rr[k][xo[1] + c], (double)rr[k][xo[2] + c],
                                            (double)rr[k][xo[3] + c], dx);
                        const double w = ra_cubic(v[0], v[1], v[2], v[3], dy);
                        o[c] = w <= 0.0 ? 0 : w >= 255.0 ? 255 : (unsigned char)(int)w;
                    }
                }
                o0 = o[0], o1 = o[1], o2 = o[2];
            }
        }
        unsigned char* q = dst + y * row + 3 * x;
        q[0] = o0, q[1] = o1, q[2] = o2;
    }
}

bool ra_args_ok(const void* work, int Bs, int B, int ns, int T, int H0, int W0, int layer, int L, const void* ra_i) {
    // (H0 * W0 < 2^32: the histogram bins and their running count are 32-bit)
    return work && ra_i && (long)H0 * W0 < (1L << 32) && Bs > 0 && B > 0 && ns > 0 && T > 0 && T <= 65535 && B <= 65535 && H0 >= 3 && W0 >= 3 && L > 0 &&
           L <= RA_MAX_LAYERS && layer >= 0 && layer < L && (long)Bs * ns == (long)B;
}

}  // namespace

extern "C" int tvts_randaug_hist(const unsigned char* work, int Bs, int B, int num_sample, int T, int H0, int W0, int layer, int L,
                                 const int* ra_i, unsigned int* hist, hipStream_t stream) {
    if (!ra_args_ok(work, Bs, B, num_sample, T, H0, W0, layer, L, ra_i) || !hist) return TVTS_EINVAL;
    const long npix = (long)H0 * W0;
    const long chunks = (npix + RA_HIST_PIX - 1) / RA_HIST_PIX;
    if (chunks > 0x7fffffffL) return TVTS_EINVAL;
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)B * T * 1024 * sizeof(unsigned int), stream);
    if (e != hipSuccess) return (int)e;
    randaug_hist_kernel<<<dim3((unsigned)chunks, T, B), RA_THREADS, 0, stream>>>(work, Bs, B, num_sample, T, H0, W0, layer, L, ra_i, hist);
    TVTS_LAUNCH_CHECK();
    return 0;
}

extern "C" int tvts_randaug_apply(unsigned char* work, int Bs, int B, int num_sample, int T, int H0, int W0, int layer, int L,
                                  const int* ra_i, const double* ra_d, const unsigned int* hist, hipStream_t stream) {
    if (!ra_args_ok(work, Bs, B, num_sample, T, H0, W0, layer, L, ra_i) || !ra_d) return TVTS_EINVAL;
    const long tiles = (long)((W0 + RA_TW - 1) / RA_TW) * ((H0 + RA_TH - 1) / RA_TH);
    if (tiles > 0x7fffffffL) return TVTS_EINVAL;
    randaug_apply_kernel<<<dim3((unsigned)tiles, T, B), RA_THREADS, 0, stream>>>(work, Bs, B, num_sample, T, H0, W0, layer, L, ra_i, ra_d,
                                                                               hist);
    TVTS_LAUNCH_CHECK();
    return 0;
}
