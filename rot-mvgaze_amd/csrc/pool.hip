// MaxPool2d(3,2,1), global average pool, and the NCHW <-> NHWC4 boundary repack.  HBM-bound.
#include <type_traits>

#include "common.h"
#include "elem.h"
#include "../../include/rotmvgaze_augment_draw.h"

namespace mvg {

// one thread = one (n, ho, wo, 4 channels).  argmax = index (0..8) of the FIRST maximum in
// (kh, kw) scan order over the in-bounds window (ATen's max_pool2d tie rule: strict >).
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float4 *__restrict__ x, float4 *__restrict__ y,
                                                          uchar4 *__restrict__ argmax, long long total, int h, int w,
                                                          int c4n, int ho, int wo) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int cq = (int)(i % c4n);
  long long t = i / c4n;
  const int ox = (int)(t % wo);
  t /= wo;
  const int oy = (int)(t % ho);
  const long long n = t / ho;
  float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  uchar4 idx = make_uchar4(0, 0, 0, 0);
  bool first = true;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int iy = oy * 2 - 1 + kh;
    if ((unsigned)iy >= (unsigned)h) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int ix = ox * 2 - 1 + kw;
      if ((unsigned)ix >= (unsigned)w) continue;
      const float4 v = x[((n * h + iy) * w + ix) * c4n + cq];
      const unsigned char k = (unsigned char)(kh * 3 + kw);
      if (first) {
        best = v;
        idx = make_uchar4(k, k, k, k);
        first = false;
      } else {
        if (v.x > best.x || v.x != v.x) { best.x = v.x; idx.x = k; }
        if (v.y > best.y || v.y != v.y) { best.y = v.y; idx.y = k; }
        if (v.z > best.z || v.z != v.z) { best.z = v.z; idx.z = k; }
        if (v.w > best.w || v.w != v.w) { best.w = v.w; idx.w = k; }
      }
    }
  }
  y[i] = best;
  argmax[i] = idx;
}

// gather form (no atomics): an input pixel collects the gradient of every window it won.
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float4 *__restrict__ dy,
                                                          const uchar4 *__restrict__ argmax, float4 *__restrict__ dx,
                                                          long long total, int h, int w, int c4n, int ho, int wo) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int cq = (int)(i % c4n);
  long long t = i / c4n;
  const int ix = (int)(t % w);
  t /= w;
  const int iy = (int)(t % h);
  const long long n = t / h;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  // windows (oy, ox) with oy*2-1 <= iy <= oy*2+1
  const int oy0 = iy >> 1, ox0 = ix >> 1;   // candidates: floor(iy/2) and floor((iy+1)/2)
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int oy = oy0 + a;
    const int kh = iy - (oy * 2 - 1);
    if (kh < 0 || kh > 2 || oy >= ho) continue;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int ox = ox0 + b;
      const int kw = ix - (ox * 2 - 1);
      if (kw < 0 || kw > 2 || ox >= wo) continue;
      const long long o = ((n * ho + oy) * wo + ox) * c4n + cq;
      const uchar4 am = argmax[o];
      const float4 g = dy[o];
      const unsigned char k = (unsigned char)(kh * 3 + kw);
      if (am.x == k) acc.x += g.x;
      if (am.y == k) acc.y += g.y;
      if (am.z == k) acc.z += g.z;
      if (am.w == k) acc.w += g.w;
    }
  }
  dx[i] = acc;
}

template <typename T>
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const T *__restrict__ x, float4 *__restrict__ y, int n,
                                                          int hw, int c4n, const float *__restrict__ x_sinv) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)n * c4n) return;
  const int cq = (int)(i % c4n);
  const long long img = i / c4n;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = 0; p < hw; ++p) {
    const float4 v = Elem<T>::ld4(x, (img * hw + p) * c4n + cq);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  const float inv = 1.f / (float)hw;
  float4 o = make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv);
  if constexpr (std::is_same<T, sp_t>::value) {
    // an sp map stored times 2^k: the mean comes back times its 2^-k (null = unscaled, and x 1.0f changes no bit)
    if (x_sinv) {
      const float k = *x_sinv;
      o = make_float4(o.x * k, o.y * k, o.z * k, o.w * k);
    }
  }
  y[i] = o;
}

template <typename T>
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const float4 *__restrict__ dy, T *__restrict__ dx,
                                                          long long total, int hw, int c4n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int cq = (int)(i % c4n);
  const long long img = i / ((long long)hw * c4n);
  const float inv = 1.f / (float)hw;
  const float4 g = dy[img * c4n + cq];
  Elem<T>::st4(dx, i, make_float4(g.x * inv, g.y * inv, g.z * inv, g.w * inv));
}

// fp32 NCHW images -> bf16 NHWC with the channels zero-padded to 8 (one 16-byte vector per pixel): the
// bf16 stem reads 8-channel pixels (K = 7*7*8)
__global__ __launch_bounds__(256) void nchw_to_nhwc8_bf16_kernel(const float *__restrict__ src, uint4 *__restrict__ dst,
                                                                 long long pixels, int c, long long hw) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= pixels) return;
  const long long n = i / hw, p = i - n * hw;
  const float *s = src + n * c * hw + p;
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < c; ++k) v[k] = s[k * hw];
  dst[i] = make_uint4(bf16_pack2(v[0], v[1]), bf16_pack2(v[2], v[3]), bf16_pack2(v[4], v[5]), bf16_pack2(v[6], v[7]));
}

__global__ __launch_bounds__(256) void nchw_to_nhwc4_kernel(const float *__restrict__ src, float4 *__restrict__ dst,
                                                            long long pixels, int c, long long hw) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= pixels) return;
  const long long n = i / hw, p = i - n * hw;
  const float *s = src + n * c * hw + p;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < c; ++k) v[k] = s[k * hw];
  dst[i] = make_float4(v[0], v[1], v[2], v[3]);
}

__global__ __launch_bounds__(256) void nhwc4_to_nchw_kernel(const float4 *__restrict__ src, float *__restrict__ dst,
                                                            long long pixels, int c, long long hw) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= pixels) return;
  const long long n = i / hw, p = i - n * hw;
  const float4 v4 = src[i];
  const float v[4] = {v4.x, v4.y, v4.z, v4.w};
  float *d = dst + n * c * hw + p;
  for (int k = 0; k < c; ++k) d[k * hw] = v[k];
}

// uint8 HWC face patch -> normalised fp32 NHWC4: the deterministic part of the reference's input
// pipeline (dataset/gaze.py:106-111 BGR->RGB; main.py:50-55 ToTensor = /255, Normalize(mean, std)).
// The per-pixel arithmetic is ONE device function for the fp32 (NHWC4) and the bf16 (NHWC8) kernels: the same
// source, the same contractions, so the bf16 output is the fp32 output rounded once.
// (ToTensor and Normalize of one RGB pixel held as floats 0..255: also the tail of augment_u8_kernel)
__device__ __forceinline__ void preprocess_u8_norm(float m0, float m1, float m2, float s0, float s1, float s2, float &c0, float &c1,
                                                   float &c2) {
  c0 = (c0 / 255.0f - m0) / s0;
  c1 = (c1 / 255.0f - m1) / s1;
  c2 = (c2 / 255.0f - m2) / s2;
}
__device__ __forceinline__ void preprocess_u8_px(const unsigned char *__restrict__ src, long long i, float m0, float m1, float m2,
                                                 float s0, float s1, float s2, int swap_rb, float &c0, float &c1, float &c2) {
  const unsigned char *p = src + 3 * i;
  c0 = (float)p[swap_rb ? 2 : 0], c1 = (float)p[1], c2 = (float)p[swap_rb ? 0 : 2];
  preprocess_u8_norm(m0, m1, m2, s0, s1, s2, c0, c1, c2);
}
__global__ __launch_bounds__(256) void preprocess_u8_kernel(const unsigned char *__restrict__ src,
                                                            float4 *__restrict__ dst, long long pixels, float m0,
                                                            float m1, float m2, float s0, float s1, float s2,
                                                            int swap_rb) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= pixels) return;
  float c0, c1, c2;
  preprocess_u8_px(src, i, m0, m1, m2, s0, s1, s2, swap_rb, c0, c1, c2);
  dst[i] = make_float4(c0, c1, c2, 0.f);
}
// ... straight to the bf16 stem's input: NHWC8 (channels 3..7 zero), one 16-byte store per pixel, no fp32 image in between
__global__ __launch_bounds__(256) void preprocess_u8_bf16_kernel(const unsigned char *__restrict__ src,
                                                                 uint4 *__restrict__ dst, long long pixels, float m0,
                                                                 float m1, float m2, float s0, float s1, float s2,
                                                                 int swap_rb) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= pixels) return;
  float c0, c1, c2;
  preprocess_u8_px(src, i, m0, m1, m2, s0, s1, s2, swap_rb, c0, c1, c2);
  dst[i] = make_uint4(bf16_pack2(c0, c1), bf16_pack2(c2, 0.f), 0u, 0u);
}

// test_transform of main.py:50-55 for patches that are not already S x S: ToTensor (/255) ->
// Resize((S, S), antialias=True) -> Normalize, fused, NHWC4 out.  torchvision's tensor Resize is
// torch.nn.functional.interpolate(mode="bilinear", antialias=True, align_corners=False) = ATen
// _upsample_bilinear2d_aa: per axis a triangle filter of half-width max(scale, 1) input pixels around
// scale * (i + 0.5), weights normalised by their float32 sum (UpSampleKernel.cpp,
// _compute_indices_min_size_weights_aa); width pass first, then height.  One thread per output pixel;
// the weights are recomputed per thread (<= (2*ceil(scale)+1)^2 filter evaluations).
struct AaAxis {
  float scale, support, invscale;
  int in_size, max_k;
};
__device__ __forceinline__ void aa_window(const AaAxis &a, int i, float &center, int &x0, int &xs, float &total) {
  // The product must be rounded before it is used: the window bounds are truncations of centre -+ support
  // + 0.5 and ATen's host code rounds each step.  hipcc contracts a*b+c into an fma by default (its
  // __fmul_rn / __fadd_rn are plain operators and `#pragma clang fp contract(off)` did not survive the
  // inlining here): fma(scale, i + 0.5, -support) moved the first tap of every third column at scale 5/3.
  // The empty asm makes the rounded product an opaque value.
  center = a.scale * ((float)i + 0.5f);
  asm volatile("" : "+v"(center));
  x0 = (int)__fadd_rn(__fsub_rn(center, a.support), 0.5f);
  if (x0 < 0) x0 = 0;
  int hi = (int)__fadd_rn(__fadd_rn(center, a.support), 0.5f);
  if (hi > a.in_size) hi = a.in_size;
  xs = hi - x0;
  xs = xs < 0 ? 0 : (xs > a.max_k ? a.max_k : xs);
  total = 0.f;
  for (int j = 0; j < xs; ++j) {
    const float t = __fmul_rn(__fadd_rn(__fsub_rn((float)(j + x0), center), 0.5f), a.invscale);
    total = __fadd_rn(total, fmaxf(0.f, 1.f - fabsf(t)));
  }
}
__device__ __forceinline__ float aa_weight(const AaAxis &a, int j, int x0, float center, float total) {
  const float t = __fmul_rn(__fadd_rn(__fsub_rn((float)(j + x0), center), 0.5f), a.invscale);
  const float w = fmaxf(0.f, 1.f - fabsf(t));
  return total != 0.f ? w / total : w;
}
// (one device function for the fp32 and the bf16 kernel, like preprocess_u8_px)
__device__ __forceinline__ void preprocess_u8_resize_px(const unsigned char *__restrict__ src, long long i, int h, int w, int oh, int ow,
                                                        const AaAxis &ay, const AaAxis &ax, float m0, float m1, float m2, float s0,
                                                        float s1, float s2, int swap_rb, float &c0, float &c1, float &c2) {
  const int ox = (int)(i % ow);
  const long long r = i / ow;
  const int oy = (int)(r % oh), img = (int)(r / oh);
  float cx, cy, tx, ty;
  int x0, xs, y0, ys;
  aa_window(ax, ox, cx, x0, xs, tx);
  aa_window(ay, oy, cy, y0, ys, ty);
  const unsigned char *base = src + (long long)img * h * w * 3;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f;
  for (int jy = 0; jy < ys; ++jy) {
    const unsigned char *row = base + ((long long)(y0 + jy) * w + x0) * 3;
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
    for (int jx = 0; jx < xs; ++jx) {
      const float wx = aa_weight(ax, jx, x0, cx, tx);
      t0 = __fadd_rn(t0, __fmul_rn(wx, (float)row[3 * jx] / 255.0f));
      t1 = __fadd_rn(t1, __fmul_rn(wx, (float)row[3 * jx + 1] / 255.0f));
      t2 = __fadd_rn(t2, __fmul_rn(wx, (float)row[3 * jx + 2] / 255.0f));
    }
    const float wy = aa_weight(ay, jy, y0, cy, ty);
    o0 = __fadd_rn(o0, __fmul_rn(wy, t0));
    o1 = __fadd_rn(o1, __fmul_rn(wy, t1));
    o2 = __fadd_rn(o2, __fmul_rn(wy, t2));
  }
  if (swap_rb) {
    const float t = o0;
    o0 = o2;
    o2 = t;
  }
  c0 = (o0 - m0) / s0;
  c1 = (o1 - m1) / s1;
  c2 = (o2 - m2) / s2;
}
__global__ __launch_bounds__(256) void preprocess_u8_resize_kernel(const unsigned char *__restrict__ src,
                                                                   float4 *__restrict__ dst, int n, int h, int w, int oh,
                                                                   int ow, AaAxis ay, AaAxis ax, float m0, float m1,
                                                                   float m2, float s0, float s1, float s2, int swap_rb) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)n * oh * ow) return;
  float c0, c1, c2;
  preprocess_u8_resize_px(src, i, h, w, oh, ow, ay, ax, m0, m1, m2, s0, s1, s2, swap_rb, c0, c1, c2);
  dst[i] = make_float4(c0, c1, c2, 0.f);
}
__global__ __launch_bounds__(256) void preprocess_u8_resize_bf16_kernel(const unsigned char *__restrict__ src,
                                                                        uint4 *__restrict__ dst, int n, int h, int w, int oh,
                                                                        int ow, AaAxis ay, AaAxis ax, float m0, float m1,
                                                                        float m2, float s0, float s1, float s2, int swap_rb) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)n * oh * ow) return;
  float c0, c1, c2;
  preprocess_u8_resize_px(src, i, h, w, oh, ow, ay, ax, m0, m1, m2, s0, s1, s2, swap_rb, c0, c1, c2);
  dst[i] = make_uint4(bf16_pack2(c0, c1), bf16_pack2(c2, 0.f), 0u, 0u);
}

// RandomMultiErasing (utils/augment.py:10-47): img *= nearest-neighbour upsampling of a per-image
// g x g keep-mask (F.interpolate default mode: src = min(int(floorf(dst * (float)g / size)), g - 1)).
// grid[n] == 0: this image is not erased.  NCHW in place.
__global__ __launch_bounds__(256) void multi_erase_kernel(float *__restrict__ img, const float *__restrict__ masks,
                                                          const int *__restrict__ grid, int gmax, int c, int h, int w) {
  const int n = blockIdx.y;
  const int g = grid[n];
  if (g <= 0) return;
  const long long hw = (long long)h * w;
  const float sy = (float)g / (float)h, sx = (float)g / (float)w;
  const float *m = masks + (long long)n * gmax * gmax;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long long)gridDim.x * 256) {
    const int y = (int)(i / w), x = (int)(i - (long long)y * w);
    int my = (int)floorf((float)y * sy), mx = (int)floorf((float)x * sx);
    my = my < g - 1 ? my : g - 1;
    mx = mx < g - 1 ? mx : g - 1;
    const float keep = m[my * g + mx];
    for (int ch = 0; ch < c; ++ch) img[((long long)n * c + ch) * hw + i] *= keep;
  }
}

// ColorJitter(brightness, contrast, saturation) and RandomAffine(degrees=0, scale, translate) of the reference's training
// transform (main.py:41-49) on raw uint8 patches, bit for bit what torchvision computes on the PIL image (Pillow's
// ImageEnhance.{Brightness, Contrast, Color} = ImagingBlend against a degenerate image, Image.transform(AFFINE, NEAREST)
// = ImagingScaleAffine), optionally followed by ToTensor + Normalize (preprocess_u8_norm) and the RandomMultiErasing
// multiply.  Every enhance op quantises to uint8; brightness and saturation are pointwise, contrast blends against ONE
// value per image, m = int(mean of grey + 0.5) of the image as it stands when contrast runs - so, given m, the three ops
// commute with the nearest-neighbour gather that follows them, and the only whole-image quantity is the grey sum S.
// One workgroup per image: phase A sums the grey of every source pixel after the ops that precede contrast (integers:
// wave shuffle, then LDS) while one lane per axis builds Pillow's source-index table by the same sequential double
// additions; phase B gathers each output pixel through the tables, applies the three ops and stores.  The second read of
// the image comes from L2.
constexpr int kAugThreads = 1024;
constexpr int kAugBatch = 4;                     // pixels per thread and pass
constexpr int kAugMaxSide = 8192;                // two int16 tables in LDS
constexpr long long kAugMaxPixels = 0xFFFFFFFFll / 255;      // S = sum of grey <= 255 h w stays in 32 bits

// Pillow's ImagingBlend: deg + f * (pix - deg), every step rounded to float32; 0 <= f <= 1 interpolates (truncation),
// any other f extrapolates and clamps.  The product must be a rounded value of its own - device code is compiled with
// contraction on and __fmul_rn / __fadd_rn are plain operators to it (see aa_window): the empty asm makes it opaque.
__device__ __forceinline__ int aug_blend(float deg, float pix, float f) {
  float prod = __fmul_rn(f, __fsub_rn(pix, deg));
  asm volatile("" : "+v"(prod));
  const float t = __fadd_rn(deg, prod);
  if (f >= 0.f && f <= 1.f) return (int)t;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}
__device__ __forceinline__ int aug_grey(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }
// op: 0 brightness (degenerate 0), 1 contrast (degenerate m), 2 saturation (degenerate = the pixel's grey); others: nothing
__device__ __forceinline__ void aug_op(int op, float f0, float f1, float f2, int m, int &r, int &g, int &b) {
  if ((unsigned)op > 2u) return;
  const float f = op == 0 ? f0 : (op == 1 ? f1 : f2);
  const float deg = op == 0 ? 0.f : (op == 1 ? (float)m : (float)aug_grey(r, g, b));
  r = aug_blend(deg, (float)r, f);
  g = aug_blend(deg, (float)g, f);
  b = aug_blend(deg, (float)b, f);
}

// The destinations, chosen at compile time (the fp32 / uint8 kernel is the one of before the bf16 destinations came):
//   kAugF32: dst_u8 [n][h][w][3] and / or dst_f [n][h][w] float4;
//   kAugNhwc8: dst_h [n][h][w] uint4 = 8 bf16, the fp32 value rounded once by bf16_pack2, channels 3..7 zero
//     (preprocess_u8_bf16_kernel's layout);
//   kAugRw: dst_rw, stem_rowwindow_bf16_kernel's folded row windows [n][h][w/4][8] uint4 - chunk q of window m holds
//     image columns 4 m - 4 + 2 q and the next one x (r, g, b, 0), zero outside [0, w) - and, optionally, dst_h.
// kAugRw walks phase B in column pairs (w % 4 == 0: a pair stays in its row, h*w is even): a thread's four pixels of a
// pass are two pairs, and the pair at column 4 k + 2 e is chunk e + 2 t of window k + 1 - t for t = 0..3 where that window
// exists: four 16-byte stores.  The chunks no pixel lands in are the row's padding: 2 in front of window 0, 4 behind the
// last window and 2 behind the one before it; a loop of its own zeroes them, so that every byte of dst_rw is written.
enum { kAugF32 = 0, kAugNhwc8 = 1, kAugRw = 2 };

// pixel u of a thread's batch in the pass that starts at pixel p0 (kAugF32 / kAugNhwc8: p0 already holds tid)
template <int kDst>
__device__ __forceinline__ int aug_pixel(int p0, int tid, int u) {
  return kDst == kAugRw ? p0 + 2 * (tid + (u >> 1) * kAugThreads) + (u & 1) : p0 + u * kAugThreads;
}

template <int kDst>
__device__ __forceinline__ void augment_u8_body(const unsigned char *__restrict__ src, const mvg_augment_rec *__restrict__ recs,
                                                unsigned char *__restrict__ dst_u8, float4 *__restrict__ dst_f,
                                                uint4 *__restrict__ dst_h, uint4 *__restrict__ dst_rw,
                                                const float *__restrict__ masks, const int *__restrict__ grid, int gmax, int h,
                                                int w, float m0, float m1, float m2, float s0, float s1, float s2, int swap_rb) {
  __shared__ short xtab[kAugMaxSide], ytab[kAugMaxSide];
  __shared__ unsigned wave_part[kAugThreads / 64];
  __shared__ int mean_s;
  const int img = blockIdx.x, tid = threadIdx.x;
  const mvg_augment_rec &rec = recs[img];
  const int o0 = rec.order[0], o1 = rec.order[1], o2 = rec.order[2];
  const float f0 = rec.factor[0], f1 = rec.factor[1], f2 = rec.factor[2];
  const int hw = h * w;
  const unsigned char *in = src + (long long)img * hw * 3;
  const int ir = swap_rb ? 2 : 0, ib = swap_rb ? 0 : 2;

  // ---- phase A: the index tables (lane 0 of waves 0 and 1) and S
  if (tid == 0 || tid == 64) {
    const bool xs = tid == 0;
    const int size = xs ? w : h;
    const double a = xs ? rec.a0 : rec.a4;
    short *tab = xs ? xtab : ytab;
    double o = (xs ? rec.cx : rec.cy) + a * 0.5;         // (a * 0.5 is exact: fused or not, one rounding)
    for (int i = 0; i < size; ++i) {
      int s = o < 0.0 ? -1 : (int)o;                      // NaN and out-of-range doubles convert to a saturated int: fill
      if (s >= size) s = -1;
      tab[i] = (short)s;
      o += a;
    }
  }
  // (both walks take kAugBatch pixels per pass, loads first: a workgroup is alone with its image's latency)
  unsigned part = 0;
  for (int p0 = tid; p0 < hw; p0 += kAugThreads * kAugBatch) {
    int r[kAugBatch], g[kAugBatch], b[kAugBatch];
#pragma unroll
    for (int u = 0; u < kAugBatch; ++u) {
      const int p = p0 + u * kAugThreads;
      const unsigned char *q = in + 3 * (p < hw ? p : hw - 1);          // past the end: the last pixel, not counted
      r[u] = q[ir], g[u] = q[1], b[u] = q[ib];
    }
#pragma unroll
    for (int u = 0; u < kAugBatch; ++u) {
      if (p0 + u * kAugThreads >= hw) break;
      if (o0 != 1) {                                      // the ops that precede contrast
        aug_op(o0, f0, f1, f2, 0, r[u], g[u], b[u]);
        if (o1 != 1) {
          aug_op(o1, f0, f1, f2, 0, r[u], g[u], b[u]);
          if (o2 != 1) aug_op(o2, f0, f1, f2, 0, r[u], g[u], b[u]);
        }
      }
      part += (unsigned)aug_grey(r[u], g[u], b[u]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  if ((tid & 63) == 0) wave_part[tid >> 6] = part;
  __syncthreads();
  if (tid == 0) {
    unsigned s = 0;
    for (int k = 0; k < kAugThreads / 64; ++k) s += wave_part[k];
    mean_s = (int)((double)s / (double)hw + 0.5);
  }
  __syncthreads();
  const int m = mean_s;

  // ---- phase B: gather, the three ops, store
  const int gcells = grid ? (grid[img] < gmax ? grid[img] : gmax) : 0;      // (never past the image's gmax x gmax slot)
  const float *mk = masks + (long long)img * gmax * gmax;
  const float sy = (float)gcells / (float)h, sx = (float)gcells / (float)w;
  const int wm = w >> 2;                                 // (kAugRw) windows per image row
  for (int p0 = kDst == kAugRw ? 0 : tid; p0 < hw; p0 += kAugThreads * kAugBatch) {
    int r[kAugBatch], g[kAugBatch], b[kAugBatch], y[kAugBatch], x[kAugBatch];
    bool inside[kAugBatch];
#pragma unroll
    for (int u = 0; u < kAugBatch; ++u) {
      const int p = aug_pixel<kDst>(p0, tid, u), pc = p < hw ? p : hw - 1;
      y[u] = pc / w, x[u] = pc - y[u] * w;
      const int ys = ytab[y[u]], xsrc = xtab[x[u]];
      inside[u] = ys >= 0 && xsrc >= 0;
      const unsigned char *q = in + (inside[u] ? (ys * w + xsrc) * 3 : 0);      // fill: pixel 0 is read and dropped
      r[u] = q[ir], g[u] = q[1], b[u] = q[ib];
    }
    uint2 even = make_uint2(0u, 0u);                      // (kAugRw) the pair's first pixel, packed
#pragma unroll
    for (int u = 0; u < kAugBatch; ++u) {
      const int p = aug_pixel<kDst>(p0, tid, u);
      if (p >= hw) break;
      if (inside[u]) {
        aug_op(o0, f0, f1, f2, m, r[u], g[u], b[u]);
        aug_op(o1, f0, f1, f2, m, r[u], g[u], b[u]);
        aug_op(o2, f0, f1, f2, m, r[u], g[u], b[u]);
      } else {
        r[u] = g[u] = b[u] = 0;                            // fill: zeros, AFTER the jitter
      }
      const long long o = (long long)img * hw + p;
      if (kDst == kAugF32 && dst_u8) {
        unsigned char *d = dst_u8 + 3 * o;
        d[0] = (unsigned char)r[u], d[1] = (unsigned char)g[u], d[2] = (unsigned char)b[u];
      }
      if (kDst != kAugF32 || dst_f) {
        float c0 = (float)r[u], c1 = (float)g[u], c2 = (float)b[u];
        preprocess_u8_norm(m0, m1, m2, s0, s1, s2, c0, c1, c2);
        if (gcells > 0) {                                  // multi_erase_kernel's index rule
          int my = (int)floorf((float)y[u] * sy), mx = (int)floorf((float)x[u] * sx);
          my = my < gcells - 1 ? my : gcells - 1;
          mx = mx < gcells - 1 ? mx : gcells - 1;
          const float keep = mk[my * gcells + mx];
          c0 *= keep, c1 *= keep, c2 *= keep;
        }
        if constexpr (kDst == kAugF32) {
          dst_f[o] = make_float4(c0, c1, c2, 0.f);
        } else {
          const uint2 px = make_uint2(bf16_pack2(c0, c1), bf16_pack2(c2, 0.f));
          if (kDst == kAugNhwc8 || dst_h) dst_h[o] = make_uint4(px.x, px.y, 0u, 0u);
          if constexpr (kDst == kAugRw) {
            if (u & 1) {                                   // x[u] is the pair's odd column: 4 k + 2 e + 1
              const int k = x[u] >> 2, e = (x[u] >> 1) & 1;
              uint4 *row = dst_rw + ((long long)img * h + y[u]) * wm * 8;
              const uint4 chunk = make_uint4(even.x, even.y, px.x, px.y);
#pragma unroll
              for (int t = 0; t < 4; ++t) {
                const int mw = k + 1 - t;
                if (mw >= 0 && mw < wm) row[mw * 8 + e + 2 * t] = chunk;
              }
            } else {
              even = px;
            }
          }
        }
      }
    }
  }
  if constexpr (kDst == kAugRw) {                          // the padding chunks: 8 per row (6 when the row is one window)
    for (int i = tid; i < h * 8; i += kAugThreads) {
      const int yy = i >> 3, s = i & 7;
      const int mw = s < 2 ? 0 : (s < 6 ? wm - 1 : wm - 2), q = (s < 2 || s >= 6) ? s : s + 2;
      if (mw >= 0) dst_rw[(((long long)img * h + yy) * wm + mw) * 8 + q] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

__global__ __launch_bounds__(kAugThreads) void augment_u8_kernel(const unsigned char *__restrict__ src,
                                                                 const mvg_augment_rec *__restrict__ recs,
                                                                 unsigned char *__restrict__ dst_u8, float4 *__restrict__ dst_f,
                                                                 const float *__restrict__ masks, const int *__restrict__ grid,
                                                                 int gmax, int h, int w, float m0, float m1, float m2, float s0,
                                                                 float s1, float s2, int swap_rb) {
  augment_u8_body<kAugF32>(src, recs, dst_u8, dst_f, nullptr, nullptr, masks, grid, gmax, h, w, m0, m1, m2, s0, s1, s2, swap_rb);
}
// ... straight to the bf16 stem's operand: NHWC8 (kRw false: any width) or the row windows, with or without NHWC8
template <bool kRw>
__global__ __launch_bounds__(kAugThreads) void augment_u8_bf16_kernel(const unsigned char *__restrict__ src,
                                                                      const mvg_augment_rec *__restrict__ recs,
                                                                      uint4 *__restrict__ dst_h, uint4 *__restrict__ dst_rw,
                                                                      const float *__restrict__ masks, const int *__restrict__ grid,
                                                                      int gmax, int h, int w, float m0, float m1, float m2, float s0,
                                                                      float s1, float s2, int swap_rb) {
  augment_u8_body<kRw ? kAugRw : kAugNhwc8>(src, recs, nullptr, nullptr, dst_h, dst_rw, masks, grid, gmax, h, w, m0, m1, m2, s0, s1,
                                            s2, swap_rb);
}

// The draws of those launches made on the device (mvg_augment_draw; the word assignment and the arithmetic are stated
// in the header and restated in NumPy by tests/augment_draw_ref.py).  One workgroup: a wave per image in turn - every
// lane computes the image's record (three Philox blocks, wave-uniform), lane 0 stores it, the lanes share the mask's
// blocks of four cells.  Every draw uses the launch counter as it stood when the launch began: all threads read it,
// then a barrier, then thread 0 stores counter + 1.
constexpr int kDrawThreads = 1024;
constexpr int kDrawMaxGrid = 64;

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}
// Products that feed an add: rounded values of their own (the empty asm keeps the contraction away: see aug_blend).
__device__ __forceinline__ float draw_mul(float a, float b) {
  float p = __fmul_rn(a, b);
  asm volatile("" : "+v"(p));
  return p;
}
__device__ __forceinline__ double draw_mul(double a, double b) {
  double p = __dmul_rn(a, b);
  asm volatile("" : "+v"(p));
  return p;
}
__device__ __forceinline__ float draw_u01(unsigned x) { return (float)(x >> 8) * 0x1p-24f; }      // exact
__device__ __forceinline__ float draw_uniform(unsigned x, float lo, float hi) {                   // torch's uniform_
  return __fadd_rn(draw_mul(draw_u01(x), __fsub_rn(hi, lo)), lo);
}
__device__ __forceinline__ double draw_uniform(unsigned x, double lo, double hi) {                 // numpy's uniform
  return __dadd_rn(lo, draw_mul(__dsub_rn(hi, lo), (double)draw_u01(x)));
}

__global__ __launch_bounds__(kDrawThreads) void augment_draw_kernel(mvg_augment_rec *__restrict__ recs, float *__restrict__ masks,
                                                                    int *__restrict__ grid, int gmax, int n, int h, int w,
                                                                    mvg_augment_draw_cfg cfg, unsigned k0, unsigned k1,
                                                                    unsigned long long *counter) {
  const unsigned long long launch = *counter;
  const unsigned c2 = (unsigned)launch, c3 = (unsigned)(launch >> 32);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cells = gmax * gmax;
  for (int i = wave; i < n; i += kDrawThreads / 64) {
    const uint4 b0 = philox4x32_10(make_uint4((unsigned)i, 0u, c2, c3), k0, k1);
    const uint4 b1 = philox4x32_10(make_uint4((unsigned)i, 1u, c2, c3), k0, k1);
    int g = 0;
    double prop = 0.0;
    if (masks && cfg.erase && !((double)draw_u01(b1.w) > cfg.p)) {
      const uint4 b2 = philox4x32_10(make_uint4((unsigned)i, 2u, c2, c3), k0, k1);
      g = (int)__ddiv_rn(1.0, draw_uniform(b2.x, cfg.dot_lo, cfg.dot_hi));
      g = g < 1 ? 1 : (g > gmax ? gmax : g);
      prop = draw_uniform(b2.y, cfg.prop_lo, cfg.prop_hi);
    }
    if (lane == 0) {
      const int k = (int)(((unsigned long long)b0.x * 6ull) >> 32);        // the k-th permutation of (0, 1, 2)
      const int o0 = k >> 1, o1 = (k & 1) ? (o0 == 2 ? 1 : 2) : (o0 == 0 ? 1 : 0);
      mvg_augment_rec r;
      r.order[0] = o0;
      r.order[1] = o1;
      r.order[2] = 3 - o0 - o1;
      r.factor[0] = draw_uniform(b0.y, cfg.factor_lo[0], cfg.factor_hi[0]);
      r.factor[1] = draw_uniform(b0.z, cfg.factor_lo[1], cfg.factor_hi[1]);
      r.factor[2] = draw_uniform(b0.w, cfg.factor_lo[2], cfg.factor_hi[2]);
      const int tx = (int)rintf(__fsub_rn(draw_mul(draw_u01(b1.x), __fmul_rn(2.f, cfg.max_dx)), cfg.max_dx));
      const int ty = (int)rintf(__fsub_rn(draw_mul(draw_u01(b1.y), __fmul_rn(2.f, cfg.max_dy)), cfg.max_dy));
      const double s = (double)draw_uniform(b1.z, cfg.scale_lo, cfg.scale_hi);
      const double inv = __ddiv_rn(1.0, s), x0 = (double)w * 0.5, y0 = (double)h * 0.5;
      r.a0 = r.a4 = inv;                                                   // augment.inverse_affine's order of operations
      r.cx = __dadd_rn(draw_mul(inv, __dsub_rn(-x0, (double)tx)), x0);
      r.cy = __dadd_rn(draw_mul(inv, __dsub_rn(-y0, (double)ty)), y0);
      recs[i] = r;
      if (grid) grid[i] = g;
    }
    if (masks) {
      float *slot = masks + (long long)i * cells;
      for (int j = lane; 4 * j < cells; j += 64) {
        uint4 m = make_uint4(0u, 0u, 0u, 0u);
        if (4 * j < g * g) m = philox4x32_10(make_uint4((unsigned)i, 3u + (unsigned)j, c2, c3), k0, k1);
        const unsigned word[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = 4 * j + e;
          if (c < cells) slot[c] = c < g * g && (double)draw_u01(word[e]) > prop ? 1.f : 0.f;
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) *counter = launch + 1ull;
}

}  // namespace mvg

using namespace mvg;

extern "C" {

int mvg_maxpool3x3s2_fwd(const float *x, float *y, uint8_t *argmax, int n, int h, int w, int c, int ho, int wo,
                         void *stream) {
  MVG_REQUIRE(c % 4 == 0, "maxpool: c %% 4 != 0");
  MVG_REQUIRE(ho == (h + 2 - 3) / 2 + 1 && wo == (w + 2 - 3) / 2 + 1, "maxpool: bad output size");
  const long long total = (long long)n * ho * wo * (c / 4);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_POOL, st, 0.0, 4.0 * ((double)n * h * w * c + (double)total * 5));
  hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, st, (const float4 *)x, (float4 *)y,
                     (uchar4 *)argmax, total, h, w, c / 4, ho, wo);
  return check_launch("maxpool_fwd");
}

int mvg_maxpool3x3s2_bwd(const float *dy, const uint8_t *argmax, float *dx, int n, int h, int w, int c, int ho, int wo,
                         void *stream) {
  MVG_REQUIRE(c % 4 == 0, "maxpool: c %% 4 != 0");
  const long long total = (long long)n * h * w * (c / 4);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_POOL, st, 0.0, 4.0 * ((double)n * h * w * c + (double)n * ho * wo * c * 1.25));
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, st, (const float4 *)dy,
                     (const uchar4 *)argmax, (float4 *)dx, total, h, w, c / 4, ho, wo);
  return check_launch("maxpool_bwd");
}

#define MVG_AVGPOOL_FACES(SUFFIX, T)                                                                                  \
  int mvg_avgpool_fwd##SUFFIX(const T *x, float *y, int n, int hw, int c, void *stream) {                             \
    MVG_REQUIRE(c % 4 == 0, "avgpool: c %% 4 != 0");                                                                   \
    hipStream_t st = (hipStream_t)stream;                                                                             \
    ProfScope ps(MVG_K_POOL, st, 0.0, (double)n * (Elem<T>::kBytes * hw + 4.0) * c);                                  \
    hipLaunchKernelGGL(avgpool_fwd_kernel<T>, dim3(ceil_div((long long)n * (c / 4), 256)), dim3(256), 0, st, x,       \
                       (float4 *)y, n, hw, c / 4, (const float *)nullptr);                                            \
    return check_launch("avgpool_fwd");                                                                               \
  }                                                                                                                    \
  int mvg_avgpool_bwd##SUFFIX(const float *dy, T *dx, int n, int hw, int c, void *stream) {                           \
    MVG_REQUIRE(c % 4 == 0, "avgpool: c %% 4 != 0");                                                                   \
    hipStream_t st = (hipStream_t)stream;                                                                             \
    const long long total = (long long)n * hw * (c / 4);                                                              \
    ProfScope ps(MVG_K_POOL, st, 0.0, (double)n * (Elem<T>::kBytes * hw + 4.0) * c);                                  \
    hipLaunchKernelGGL(avgpool_bwd_kernel<T>, dim3(ceil_div(total, 256)), dim3(256), 0, st, (const float4 *)dy, dx,    \
                       total, hw, c / 4);                                                                             \
    return check_launch("avgpool_bwd");                                                                               \
  }
MVG_AVGPOOL_FACES(, float)
MVG_AVGPOOL_FACES(_bf16, uint16_t)
#undef MVG_AVGPOOL_FACES

static int avgpool_fwd_split_impl(const void *x_sp, const float *x_sinv, float *y, int n, int hw, int c, void *stream) {
  MVG_REQUIRE(c % 8 == 0, "avgpool_split: c %% 8 != 0");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_POOL, st, 0.0, (double)n * (6.0 * hw + 4.0) * c);
  hipLaunchKernelGGL(avgpool_fwd_kernel<sp_t>, dim3(ceil_div((long long)n * (c / 4), 256)), dim3(256), 0, st, (const sp_t *)x_sp,
                     (float4 *)y, n, hw, c / 4, x_sinv);
  return check_launch("avgpool_fwd_split");
}

int mvg_avgpool_fwd_split_scaled(const void *x_sp, const float *x_sinv, float *y, int n, int hw, int c, void *stream) {
  MVG_REQUIRE(x_sp && y && n > 0 && hw > 0 && c > 0, "avgpool_split: x_sp and y are required, sizes positive");
  return avgpool_fwd_split_impl(x_sp, x_sinv, y, n, hw, c, stream);
}

int mvg_avgpool_fwd_split(const void *x_sp, float *y, int n, int hw, int c, void *stream) {
  return avgpool_fwd_split_impl(x_sp, nullptr, y, n, hw, c, stream);
}

int mvg_nchw_to_nhwc8_bf16(const float *src, uint16_t *dst, int n, int c, int h, int w, void *stream) {
  MVG_REQUIRE(c >= 1 && c <= 8, "nchw_to_nhwc8_bf16: c must be 1..8");
  hipStream_t st = (hipStream_t)stream;
  const long long pixels = (long long)n * h * w;
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, (double)pixels * (4.0 * c + 16.0));
  hipLaunchKernelGGL(nchw_to_nhwc8_bf16_kernel, dim3(ceil_div(pixels, 256)), dim3(256), 0, st, src, (uint4 *)dst, pixels, c,
                     (long long)h * w);
  return check_launch("nchw_to_nhwc8_bf16");
}

int mvg_nchw_to_nhwc4(const float *src, float *dst, int n, int c, int h, int w, void *stream) {
  MVG_REQUIRE(c >= 1 && c <= 4, "nchw_to_nhwc4: c must be 1..4");
  hipStream_t st = (hipStream_t)stream;
  const long long pixels = (long long)n * h * w;
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, 4.0 * (double)pixels * (c + 4));
  hipLaunchKernelGGL(nchw_to_nhwc4_kernel, dim3(ceil_div(pixels, 256)), dim3(256), 0, st, src, (float4 *)dst, pixels, c,
                     (long long)h * w);
  return check_launch("nchw_to_nhwc4");
}

int mvg_preprocess_u8hwc(const uint8_t *src, float *dst, int n, int h, int w, float mean0, float mean1, float mean2,
                         float std0, float std1, float std2, int swap_rb, void *stream) {
  MVG_REQUIRE(std0 > 0.f && std1 > 0.f && std2 > 0.f, "preprocess: std must be positive");
  hipStream_t st = (hipStream_t)stream;
  const long long pixels = (long long)n * h * w;
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, 19.0 * (double)pixels);
  hipLaunchKernelGGL(preprocess_u8_kernel, dim3(ceil_div(pixels, 256)), dim3(256), 0, st, src, (float4 *)dst, pixels, mean0,
                     mean1, mean2, std0, std1, std2, swap_rb);
  return check_launch("preprocess_u8hwc");
}

static AaAxis aa_axis(int in_size, int out_size) {
  AaAxis a;
  a.scale = (float)in_size / (float)out_size;
  a.support = a.scale >= 1.f ? a.scale : 1.f;
  a.invscale = a.scale >= 1.f ? 1.f / a.scale : 1.f;
  a.in_size = in_size;
  a.max_k = (int)ceilf(a.support) * 2 + 1;
  return a;
}

int mvg_preprocess_u8hwc_resize(const uint8_t *src, float *dst, int n, int h, int w, int oh, int ow, float mean0,
                                float mean1, float mean2, float std0, float std1, float std2, int swap_rb, void *stream) {
  MVG_REQUIRE(std0 > 0.f && std1 > 0.f && std2 > 0.f, "preprocess: std must be positive");
  MVG_REQUIRE(n > 0 && h > 0 && w > 0 && oh > 0 && ow > 0, "preprocess_resize: bad sizes");
  if (h == oh && w == ow)      // torchvision's resize returns the input unchanged
    return mvg_preprocess_u8hwc(src, dst, n, h, w, mean0, mean1, mean2, std0, std1, std2, swap_rb, stream);
  hipStream_t st = (hipStream_t)stream;
  const long long pixels = (long long)n * oh * ow;
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, 3.0 * (double)n * h * w + 16.0 * (double)pixels);
  hipLaunchKernelGGL(preprocess_u8_resize_kernel, dim3(ceil_div(pixels, 256)), dim3(256), 0, st, src, (float4 *)dst, n, h, w,
                     oh, ow, aa_axis(h, oh), aa_axis(w, ow), mean0, mean1, mean2, std0, std1, std2, swap_rb);
  return check_launch("preprocess_u8hwc_resize");
}

int mvg_preprocess_u8hwc_resize_bf16(const uint8_t *src, uint16_t *dst, int n, int h, int w, int oh, int ow, float mean0,
                                     float mean1, float mean2, float std0, float std1, float std2, int swap_rb, void *stream) {
  MVG_REQUIRE(src && dst, "preprocess_resize_bf16: null argument");
  MVG_REQUIRE(std0 > 0.f && std1 > 0.f && std2 > 0.f, "preprocess: std must be positive");
  MVG_REQUIRE(n > 0 && h > 0 && w > 0 && oh > 0 && ow > 0, "preprocess_resize_bf16: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  const long long pixels = (long long)n * oh * ow;
  if (h == oh && w == ow) {    // torchvision's resize returns the input unchanged
    ProfScope ps(MVG_K_LAYOUT, st, 0.0, 19.0 * (double)pixels);
    hipLaunchKernelGGL(preprocess_u8_bf16_kernel, dim3(ceil_div(pixels, 256)), dim3(256), 0, st, src, (uint4 *)dst, pixels, mean0,
                       mean1, mean2, std0, std1, std2, swap_rb);
    return check_launch("preprocess_u8hwc_bf16");
  }
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, 3.0 * (double)n * h * w + 16.0 * (double)pixels);
  hipLaunchKernelGGL(preprocess_u8_resize_bf16_kernel, dim3(ceil_div(pixels, 256)), dim3(256), 0, st, src, (uint4 *)dst, n, h, w,
                     oh, ow, aa_axis(h, oh), aa_axis(w, ow), mean0, mean1, mean2, std0, std1, std2, swap_rb);
  return check_launch("preprocess_u8hwc_resize_bf16");
}

int mvg_multi_erase_nchw(float *img, const float *masks, const int32_t *grid, int gmax, int n, int c, int h, int w,
                         void *stream) {
  MVG_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && gmax > 0, "multi_erase: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, 8.0 * (double)n * c * h * w);
  long long bx = ((long long)h * w + 255) / 256;
  if (bx > 64) bx = 64;
  hipLaunchKernelGGL(multi_erase_kernel, dim3((unsigned)bx, n), dim3(256), 0, st, img, masks, grid, gmax, c, h, w);
  return check_launch("multi_erase");
}

// the checks of the two augment entry points, in one order (0, or MVG_REQUIRE's status with the message set); no_dst /
// bad_erase: the entry point's own message when it has no destination / cannot serve the erase, else null
static int augment_check(const uint8_t *src, const mvg_augment_rec *recs, const mvg_augment_rec *recs_host, const char *no_dst,
                         const float *masks, const int32_t *grid, const char *bad_erase, int n, int h, int w, float std0, float std1,
                         float std2) {
  MVG_REQUIRE(src && recs, "augment: src and the device records are required");
  MVG_REQUIRE(!no_dst, "%s", no_dst);
  MVG_REQUIRE(n > 0 && h > 0 && w > 0, "augment: bad sizes");
  MVG_REQUIRE(h <= kAugMaxSide && w <= kAugMaxSide, "augment: a side of %d x %d is longer than the index tables hold (%d)", h, w,
              kAugMaxSide);
  MVG_REQUIRE((long long)h * w <= kAugMaxPixels, "augment: %d x %d pixels overflow the 32-bit grey sum (at most %lld)", h, w,
              kAugMaxPixels);
  MVG_REQUIRE(std0 > 0.f && std1 > 0.f && std2 > 0.f, "augment: std must be positive");
  MVG_REQUIRE((masks == nullptr) == (grid == nullptr), "augment: erase masks and grid come together");
  MVG_REQUIRE(!bad_erase, "%s", bad_erase);
  if (recs_host)
    for (int i = 0; i < n; ++i) {
      const int32_t *o = recs_host[i].order;
      MVG_REQUIRE(o[0] >= 0 && o[0] <= 2 && o[1] >= 0 && o[1] <= 2 && o[2] >= 0 && o[2] <= 2 && o[0] != o[1] && o[0] != o[2] && o[1] != o[2],
                  "augment: record %d: order (%d, %d, %d) is not a permutation of 0, 1, 2", i, o[0], o[1], o[2]);
    }
  return 0;
}

int mvg_augment_u8hwc(const uint8_t *src, const mvg_augment_rec *recs, const mvg_augment_rec *recs_host, uint8_t *dst_u8,
                      float *dst_nhwc4, const float *masks, const int32_t *grid, int gmax, int n, int h, int w, float mean0,
                      float mean1, float mean2, float std0, float std1, float std2, int swap_rb, void *stream) {
  const char *no_dst = dst_u8 || dst_nhwc4 ? nullptr : "augment: no destination (dst_u8 and dst_nhwc4 are both null)";
  const char *bad_erase =
      !masks || (dst_nhwc4 && gmax > 0) ? nullptr : "augment: the erase multiplies the normalised image (dst_nhwc4) and needs gmax > 0";
  if (const int rc = augment_check(src, recs, recs_host, no_dst, masks, grid, bad_erase, n, h, w, std0, std1, std2)) return rc;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, (double)n * h * w * (6.0 + (dst_u8 ? 3.0 : 0.0) + (dst_nhwc4 ? 16.0 : 0.0)));
  hipLaunchKernelGGL(augment_u8_kernel, dim3(n), dim3(kAugThreads), 0, st, src, recs, dst_u8, (float4 *)dst_nhwc4, masks, grid, gmax,
                     h, w, mean0, mean1, mean2, std0, std1, std2, swap_rb);
  return check_launch("augment_u8hwc");
}

int mvg_augment_u8hwc_bf16(const uint8_t *src, const mvg_augment_rec *recs, const mvg_augment_rec *recs_host, uint16_t *dst_nhwc8,
                           uint16_t *dst_rw, const float *masks, const int32_t *grid, int gmax, int n, int h, int w, float mean0,
                           float mean1, float mean2, float std0, float std1, float std2, int swap_rb, void *stream) {
  const char *no_dst = dst_nhwc8 || dst_rw ? nullptr : "augment_bf16: no destination (dst_nhwc8 and dst_rw are both null)";
  const char *bad_erase = !masks || gmax > 0 ? nullptr : "augment_bf16: the erase needs gmax > 0";
  if (const int rc = augment_check(src, recs, recs_host, no_dst, masks, grid, bad_erase, n, h, w, std0, std1, std2)) return rc;
  MVG_REQUIRE(!dst_rw || w % 4 == 0, "augment_bf16: the row windows (dst_rw) need w %% 4 == 0 (w = %d)", w);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, (double)n * h * w * (6.0 + (dst_nhwc8 ? 16.0 : 0.0) + (dst_rw ? 32.0 : 0.0)));
  if (dst_rw)
    hipLaunchKernelGGL(augment_u8_bf16_kernel<true>, dim3(n), dim3(kAugThreads), 0, st, src, recs, (uint4 *)dst_nhwc8, (uint4 *)dst_rw,
                       masks, grid, gmax, h, w, mean0, mean1, mean2, std0, std1, std2, swap_rb);
  else
    hipLaunchKernelGGL(augment_u8_bf16_kernel<false>, dim3(n), dim3(kAugThreads), 0, st, src, recs, (uint4 *)dst_nhwc8, (uint4 *)nullptr,
                       masks, grid, gmax, h, w, mean0, mean1, mean2, std0, std1, std2, swap_rb);
  return check_launch("augment_u8hwc_bf16");
}

int mvg_augment_draw(mvg_augment_rec *recs, float *masks, int32_t *grid, int gmax, int n, int h, int w, const void *cfg,
                     uint64_t seed, uint64_t *counter_dev, void *stream) {
  MVG_REQUIRE(recs && counter_dev, "augment_draw: the device records and the device launch counter are required");
  MVG_REQUIRE(cfg, "augment_draw: cfg is required");
  MVG_REQUIRE(n > 0 && h > 0 && w > 0, "augment_draw: bad sizes");
  MVG_REQUIRE((masks == nullptr) == (grid == nullptr), "augment_draw: erase masks and grid come together");
  const mvg_augment_draw_cfg &c = *(const mvg_augment_draw_cfg *)cfg;
  MVG_REQUIRE(!c.erase || masks, "augment_draw: cfg->erase is set and the masks are missing");
  if (masks) {
    MVG_REQUIRE(c.dot_lo > 0.0 && c.dot_lo <= c.dot_hi, "augment_draw: the dot-size range needs 0 < dot_lo <= dot_hi");
    MVG_REQUIRE(gmax == (int)(1.0 / c.dot_lo), "augment_draw: gmax is %d, (int)(1.0 / dot_lo) is %d", gmax, (int)(1.0 / c.dot_lo));
    MVG_REQUIRE(gmax >= 1 && gmax <= kDrawMaxGrid, "augment_draw: a mask grid of %d cells a side is not served (1..%d)", gmax, kDrawMaxGrid);
  } else {
    MVG_REQUIRE(gmax == 0, "augment_draw: gmax is %d without masks (0: no erase)", gmax);
  }
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, (double)n * (sizeof(mvg_augment_rec) + (masks ? 4.0 * gmax * gmax + 4.0 : 0.0)));
  hipLaunchKernelGGL(augment_draw_kernel, dim3(1), dim3(kDrawThreads), 0, st, recs, masks, grid, gmax, n, h, w, c, (unsigned)seed,
                     (unsigned)(seed >> 32), (unsigned long long *)counter_dev);
  return check_launch("augment_draw");
}

int mvg_nhwc4_to_nchw(const float *src, float *dst, int n, int c, int h, int w, void *stream) {
  MVG_REQUIRE(c >= 1 && c <= 4, "nhwc4_to_nchw: c must be 1..4");
  hipStream_t st = (hipStream_t)stream;
  const long long pixels = (long long)n * h * w;
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, 4.0 * (double)pixels * (c + 4));
  hipLaunchKernelGGL(nhwc4_to_nchw_kernel, dim3(ceil_div(pixels, 256)), dim3(256), 0, st, (const float4 *)src, dst, pixels,
                     c, (long long)h * w);
  return check_launch("nhwc4_to_nchw");
}

}  // extern "C"
