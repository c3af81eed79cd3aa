// Types and helpers shared by the implicit-GEMM translation units (conv_igemm.hip: fp32 MFMA,
// conv_split.hip: split-operand fp16 MFMA, conv_bf16.hip: bf16 MFMA): the kernels' parameter blocks and the host
// planning every family does alike - descriptor -> launch geometry, backward-data parity classes, weight-gradient
// pixel splits and their slab reduce.  Everything here is static / inline: the library is built without
// relocatable device code, so a kernel must be defined in the translation unit that launches it.
#pragma once
#include <stdlib.h>

#include "common.h"

namespace mvg {


typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// 16-byte load through a buffer descriptor: an offset >= num_records returns zeros in hardware, so
// predication is a v_cndmask on the offset - no branch, no select on the data.
// pred_off(off, ok): sets bit 31 when !ok -> beyond any descriptor here (tensors/groups < 2 GiB);
// written arithmetically so that `off` is computed unconditionally (a select with an "expensive"
// arm is turned back into a branch by the compiler, splitting the K-step's basic block).
__device__ __forceinline__ unsigned pred_off(unsigned off, bool ok) { return off | ((unsigned)(!ok) << 31); }
__device__ __forceinline__ float4 buf_ld16(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
// base / bytes must be wave-uniform; readfirstlane makes that provable to the compiler (otherwise it
// wraps every buffer op in a waterfall loop - cdna_hip_programming.md T20).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base, long long bytes) {
  unsigned n = bytes > 0x7FFFFFF0ll ? 0x7FFFFFF0u : (bytes < 0 ? 0u : (unsigned)bytes);
  const unsigned long long b = (unsigned long long)base;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
  n = __builtin_amdgcn_readfirstlane(n);
  void *ub = (void *)(((unsigned long long)hi << 32) | lo);
  return __builtin_amdgcn_make_buffer_rsrc(ub, 0, (int)n, 0x00020000);
}

// exact unsigned 32-bit division by a runtime constant (Granlund-Montgomery round-up form)
struct FastDiv {
  unsigned mul, sh1, sh2, d;
};
static FastDiv make_fastdiv(unsigned d) {
  FastDiv f;
  unsigned l = 0;
  while ((1ull << l) < d) ++l;
  f.mul = (unsigned)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
  f.sh1 = l < 1 ? l : 1;
  f.sh2 = l > 0 ? l - 1 : 0;
  f.d = d;
  return f;
}
__device__ __forceinline__ unsigned fdiv(unsigned n, const FastDiv &f) {
  const unsigned t = __umulhi(f.mul, n);
  return (t + ((n - t) >> f.sh1)) >> f.sh2;
}

// Per-class view of a launch.  fprop and stride-1 dgrad have one class; a stride-2 dgrad has one per
// output-pixel parity (py, px) - each a dense sub-convolution over its own taps - and all of them
// run in ONE launch, so that the short classes (one tap: 8 K-steps per tile) share the device with
// the long ones instead of each paying a partly filled round of workgroups.
struct IgemmClass {
  int out_h, out_w;          // spatial extent of the GEMM's row space
  int ntaps, tap_ns, tap_r0, tap_s0;
  int ktotal;                // ntaps * src_c
  int cls_py, cls_px, cls_cy, cls_cx;
  int mtiles_per_group;
  long long rows_per_group;
  FastDiv tap_ns_div, ohw_div, ow_div;
  int korder;                // 1: K-steps run (32-channel block, tap, half) - see igemm_kernel
  FastDiv per_div;           // K-steps per 32-channel block: ntaps * 32 / BK
  long long unit0;           // first (tile, K-step) unit of this class in the launch's unit space
  int tile0;                 // first tile of this class
  int KT;                    // K-steps per tile (>= 1: a class without taps runs one all-zero step; split / bf16 kernels
                             // with a fused BatchNorm reduce: 0 - such a class's tiles are epilogue only)
  int part0;                 // fused BatchNorm-backward reduce: this class's first partial row inside a group (bn_part)
};

struct IgemmParams {
  const float *a;       // gathered operand (fprop: x, dgrad: dy)
  const float *b;       // weights, KRSC
  float *out;
  const float *bias;    // [ncols] or null (fprop)
  const float *scale;   // [ncols] or null (fprop, inference: y = acc*scale + bias (+addend) [relu])
  const float *mask;    // like out or null (dgrad)
  const float *addend;  // like out or null (dgrad)
  float *stats;         // [groups][P][2][ncols] or null (fprop)
  int relu;
  int groups;
  int out_h, out_w;     // spatial extent of the GEMM's row space
  int src_h, src_w;     // spatial extent of the gathered tensor
  int src_c;            // channels of the gathered tensor (K per tap)
  int src_c_shift;      // log2(src_c) when r*s > 1
  int ncols;            // GEMM N
  int r, s, stride_shift, stride, pad;
  int ktotal;           // r*s*src_c
  int cin;              // dgrad: weight inner dim
  int rs;
  long long rows_per_group;
  long long src_img_stride;  // src_h*src_w*src_c
  int imgs_per_group;
  int mtiles_per_group, ntiles;
  // tap sub-lattice: GEMM k = (ti*tap_ns + tj)*src_c + c with filter tap (r, s) =
  // (tap_r0 + tap_step*ti, tap_s0 + tap_step*tj).  fprop / stride-1 dgrad: the whole filter.
  // Stride-2 dgrad runs once per output-pixel parity class (py, px): only the taps with
  // (y + pad - r) even contribute, so each class is a dense sub-convolution over its own taps
  // (no multiply-by-zero work); rows are the class's pixels (y, x) = (2*y2 + py, 2*x2 + px).
  int ntaps, tap_ns, tap_r0, tap_s0, tap_step;
  int cls_step, cls_py, cls_px, cls_cy, cls_cx;
  int full_h, full_w;        // dgrad: spatial extent of dx (row decode when cls_step == 2)
  long long a_group_bytes;   // bytes of one group of the gathered tensor
  long long b_bytes;         // bytes of the weight tensor
  FastDiv tap_ns_div;
  FastDiv ohw_div, ow_div;   // row -> (image, y, x) of the GEMM's row space (out_h*out_w, out_w)
  // split-K (small-M GEMMs: the Linear layers of the fusion block stream 100-240 MB of weights
  // over <= a few hundred rows; splitting K spreads that stream over every CU).  Partial tiles go
  // to `slab` [splits][groups*rows][ncols] and splitk_reduce_kernel applies the epilogue.
  int splits, ktiles_per_split;
  float *slab;
  // stream-K (fp32 conv kernels): sk_tiles > 0 -> the grid is P persistent workgroups that each take
  // an equal share of the sk_tiles x ceil(ktotal/BK) K-steps, in tile-major order.  A workgroup
  // whose share starts or ends inside a tile writes that piece's raw accumulators to `slab`
  // (slot 0: piece that does not start the tile, slot 1: piece that starts it) and
  // igemm_fixup_kernel sums the pieces in workgroup order and runs the epilogue.
  int sk_tiles;
  int no_remap;              // several classes, one tile per workgroup: keep the dispatch order (longest class first)
  int nt_out;                // split kernels, fp32 result: non-temporal stores
  int ncls;
  IgemmClass cls[4];         // per-class view (one class unless this is a stride-2 dgrad)
  int b_row_len;             // bf16 kernels: elements per row of the (k-contiguous) weight operand
  int stats_partials;        // bf16_epilogue: partials per group of `stats` as the caller allocated it (0: mtiles * wave rows)
  // Backward-data fused with the BatchNorm-backward REDUCE pass of the unit whose output gradient this
  // launch produces (split and bf16 kernels): the epilogue masks the gradient by that unit's ReLU
  // (bn_bits, or fma(bn_y, bn_rscale, bn_rshift) > 0, or no mask), stores the masked gradient and adds up,
  // per workgroup and column, s1 = sum(dz) and s2 = sum(dz * xhat), xhat = (bn_y - bn_mean) * bn_invstd, into
  // bn_part [groups][bn_parts][bn_part_rows][ncols] (bn_parts = row tiles per group over all classes: a stride-2
  // launch's parity classes each own the range starting at IgemmClass::part0; a class without taps - a 1x1 stride-2
  // filter touches one pixel in four - still runs its tiles, epilogue only, for the mask and the sums).
  // bn_y has the storage type of `out` (fp32, or bf16 in the bf16 kernels).
  const float *bn_y, *bn_mean, *bn_invstd, *bn_rscale, *bn_rshift;
  float *bn_part;
  int bn_parts;
  // split kernels, inference forward (BatchNorm folded: y = acc * scale + bias (+ residual) [relu]): the residual
  // and / or the result in sp (the next conv's operand format) instead of fp32
  int addend_sp, out_sp, mask_sp;
  // split kernels: the operands hold (value * 2^k) for a per-tensor k (elem.h: sp_t); the epilogue multiplies the
  // accumulators by *a_sinv * *b_sinv (device scalars, each 2^-k of its operand; null = 1)
  const float *a_sinv, *b_sinv;
  // split kernels running a Linear of the fusion block (igemm_split16_kernel<.., LIN = true>): out_absmax receives max |result| of
  // an fp32 result (atomicMax on the bits; the caller clears it); an sp result (out_sp) is stored times 2^k from the bound
  // ktotal * 2^30 * a_sinv * b_sinv + *bias_absmax and *out_sinv receives 2^-k
  unsigned *out_absmax;
  float *out_sinv;
  const float *bias_absmax;
  int stride_w, pad_w;            // split / bf16 kernels, forward: horizontal stride / padding (= stride / pad except for the stem's
                                  // row-window form: a 7 x 1 filter, vertical stride 2, over windows that already step by 2)
  int stats_fold;                 // bf16 stem (two output columns per window as 2 x cout GEMM columns): the BatchNorm partials of
                                  // columns c and c + ncols/2 are written as partials 2 pi and 2 pi + 1 of channel c
  int bn_part_rows;               // fused BatchNorm-backward reduce: rows per partial in bn_part - 2 (s1, s2) or 3 (+ max |dz| per channel)
  const unsigned char *bn_bits;   // the unit's ReLU mask as bits: one byte per 4 channels (fp32: mvg_bn_apply_split) or per 8 (bf16: mvg_bn_apply_bits_bf16)
  // Cross-view fusion (igemm_kernel AMODE = 1, Linear forward): the A operand is never materialised - row m of
  //   X = [ img_feat[rc_row_img[m]] (rc_cf floats) | rc_rel[m] (3x3) @ feat[rc_row_src[m]] (3 x rc_nvec, axis-major) ]
  // (rot_mv.py:44-50,234-239) is generated by the loader: the image part is a plain row load (p.a = img_feat),
  // the rotated part three loads and three fmas per float4.  rc_rel == null: no rotation (head input, ignore_rotmat).
  const float *rc_feat, *rc_rel;
  const int *rc_row_img, *rc_row_src;
  int rc_cf, rc_nvec, rc_nvec_shift;
  long long rc_img_bytes, rc_feat_bytes;
  // Split kernels, backward-data of a 1x1 stride-1 unit with ONE column tile (igemm_split16_kernel<.., AF = A_DY>): the A
  // operand dy is not read - the loader forms it, dy = bn_dy(dz, y, ...) * 2^k with 2^-k = *a_sinv (the unit's own
  // BatchNorm-backward apply pass: bna_dz already masked; mean / invstd / s1 / s2 [groups][src_c], gamma [src_c]), multiplies
  // it and stores it ONCE in sp to `a` (written here, read later by the weight gradient).
  const float *bna_dz, *bna_y, *bna_mean, *bna_invstd, *bna_gamma, *bna_s1, *bna_s2;
  float bna_inv_rows;             // 1 / rows per group of the unit's BatchNorm
  // Split kernels, forward of a residual block's first conv (1x1, stride 1, ONE column tile; igemm_split16_kernel<.., AF = A_OUT_SP | A_OUT_AFFINE>): the A
  // operand - the previous block's output - is not read: the loader forms it, relu(fap_y * fap_scale + fap_shift + residual) * 2^k
  // with 2^-k = *a_sinv (that block's BatchNorm apply pass: scale / shift [groups][src_c]; the residual fap_res is the sp identity,
  // read times *fap_res_sinv (null = 1), or with fap_res_scale / fap_res_shift the raw fp32 downsample output), multiplies it
  // and stores it ONCE in sp to `a`, and the ReLU mask to fap_bits (one unsigned short per 8-channel chunk, bn_apply_sp_kernel's layout;
  // null = not wanted).
  const float *fap_y, *fap_scale, *fap_shift, *fap_res_scale, *fap_res_shift, *fap_res_sinv;
  const void *fap_res;
  unsigned short *fap_bits;
};

// bijective XCD-aware remap of a 1-D grid (cdna_hip_programming.md §5 "XCD swizzle must be
// bijective"): blocks that are adjacent after the remap share an XCD L2.
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
  const int q = nwg >> 3, rr = nwg & 7, xcd = orig & 7;
  const int base = (xcd < rr) ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q;
  return base + (orig >> 3);
}


struct WgradParams {
  const float *x;   // [imgs][h][w][cin]
  const float *dy;  // [imgs][ho][wo][cout]
  float *out;       // [splits][cout][rs*cin] (or dw directly when splits == 1)
  int h, w, cin, cout, r, s, stride, pad, ho, wo;
  int ncols;        // rs*cin
  long long pixels; // imgs*ho*wo
  long long pixels_per_split;
  long long x_bytes;
  int mtiles, ntiles;
  int accumulate;   // only meaningful when splits == 1
  float *db;        // Linear layers: column sums of dy (the bias gradient) ride along, [splits][cout] slabs like `out`
                    // (or the gradient itself when splits == 1); null = not wanted
  // wgrad_kernel XMODE = 1: the x operand is the generated cross-view input X (see IgemmParams::rc_*); x = img_feat
  const float *rc_feat, *rc_rel;
  const int *rc_row_img, *rc_row_src;
  int rc_cf, rc_nvec;
  long long rc_img_bytes, rc_feat_bytes;
  FastDiv ohw_div, wo_div, cin_div, s_div;
  const float *dy_sinv;           // split kernels: 2^-k of the dy operand's per-tensor scale (device scalar, null = 1)
  const float *x_sinv;            // ... and of the x operand's (a Linear's scaled input / hidden activation; null = 1: BatchNorm outputs)
  int stride_w, pad_w;            // split kernels: horizontal stride / padding (see IgemmParams)
};

// ---- what the three weight-gradient kernels (wgrad_kernel, wgrad_split_kernel, wgrad_bf16_kernel) do alike ----------------
// The kernels keep what differs on purpose: loader thread mappings, LDS images, fragments, the MFMA step and the K loop.

// A workgroup's (pixel split, row tile, column tile) and its split's pixels: m_count of them from m_begin on, the first one
// pixel rem0 of image img0.
// 1-D grid, XCD-aware: workgroups round-robin over the 8 XCDs, so the bijective remap hands every
// XCD a contiguous run of (split, tile) ids.  All tiles of a split (the same pixel range of dy and
// x) then run on ONE XCD at about the same time and share its L2 - spread over the XCDs, every
// tile re-read its operands from memory (16x the algorithmic bytes on the 256-channel layers).
struct WgradTile {
  int split, mtile, ntile;
  long long m_begin, img0;
  int m_count;
  unsigned rem0;
};
__device__ __forceinline__ WgradTile wgrad_tile_id(const WgradParams &p) {
  WgradTile t;
  const int tiles = p.mtiles * p.ntiles;
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  t.split = logical / tiles;
  const int tile = logical - t.split * tiles;
  t.ntile = tile % p.ntiles;
  t.mtile = tile / p.ntiles;
  t.m_begin = (long long)t.split * p.pixels_per_split;
  long long m_end = t.m_begin + p.pixels_per_split;
  if (m_end > p.pixels) m_end = p.pixels;
  t.m_count = m_end > t.m_begin ? (int)(m_end - t.m_begin) : 0;
  const int ohw = p.ho * p.wo;
  t.img0 = t.m_begin / ohw;                                                // scalar, once
  t.rem0 = (unsigned)(t.m_begin - t.img0 * ohw);
  return t;
}

// Column col = (tap, channel) of the x operand: whether it exists, the tap's displacement (dy, dx) from a pixel's window
// origin and its byte offset from that origin's first channel; elem bytes per element, pad_w the horizontal padding.
// channel (optional): receives the column's channel inside its tap.
struct WgradColumn {
  bool cok;
  int dy, dx;
  unsigned tconst;
};
__device__ __forceinline__ WgradColumn wgrad_column(const WgradParams &p, int col, unsigned elem, int pad_w, int *channel = nullptr) {
  WgradColumn c;
  c.cok = col < p.ncols;
  const int tap = (int)fdiv((unsigned)(c.cok ? col : 0), p.cin_div);
  const int cc = (c.cok ? col : 0) - tap * p.cin;
  if (channel) *channel = cc;
  const int fr = (int)fdiv((unsigned)tap, p.s_div), fs = tap - fr * p.s;
  c.dy = fr - p.pad;
  c.dx = fs - pad_w;
  c.tconst = (unsigned)((c.dy * p.w + c.dx) * p.cin + cc) * elem;
  return c;
}

// An output pixel of the split as the x loaders address it: (oy, ox) and the byte offset of its image from the split's
// first (img_bytes per image).  decode() from the pixel's index counted from that first image's pixel 0; advance<BK>()
// steps BK pixels on: columns wrap into rows, rows into the next image (at most once: the hosts ask for ho*wo >= 2*BK).
struct WgradPixel {
  int oy, ox;
  unsigned imgoff;
  __device__ __forceinline__ void decode(const WgradParams &p, unsigned pix, unsigned img_bytes) {
    const unsigned img = fdiv(pix, p.ohw_div);
    const unsigned rem = pix - img * (unsigned)(p.ho * p.wo);
    const unsigned uy = fdiv(rem, p.wo_div);
    oy = (int)uy;
    ox = (int)(rem - uy * (unsigned)p.wo);
    imgoff = img * img_bytes;
  }
  template <int BK>
  __device__ __forceinline__ void advance(const WgradParams &p, unsigned img_bytes) {
    unsigned nx = (unsigned)ox + BK;
    const unsigned q = fdiv(nx, p.wo_div);
    nx -= q * (unsigned)p.wo;
    ox = (int)nx;
    const int noy = oy + (int)q;
    const bool wrap = noy >= p.ho;
    oy = wrap ? noy - p.ho : noy;
    imgoff += wrap ? img_bytes : 0u;
  }
};

// The epilogue: a wave's TM x TN accumulator tiles of 32 x 32, times scale, to (or, accumulating, onto) `out`
// [cout][ncols], predicated per element.  (row0, col0): the wave's block in `out`; the MFMA result map gives lane l, with
// li = l & 31 and lh = l >> 5, column li and rows 4 * lh + (e & 3) + 8 * (e >> 2) of a tile.
// Code-generation note (profiles/r15_isa_wgrad_shared_vs_parent.txt): p by value and li / lh from the caller is the form
// under which the split and bf16 kernels compile as they did with the loop written out in them.
template <int TM, int TN>
__device__ __forceinline__ void wgrad_store_acc(const WgradParams p, const f32x16 (&acc)[TM][TN], float *out, int row0, int col0,
                                                int li, int lh, float scale) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = col0 + j * 32 + li;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = row0 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (row < p.cout && col < p.ncols) {
          const long long off = (long long)row * p.ncols + col;
          float v = acc[i][j][e] * scale;
          if (p.accumulate) v += out[off];
          out[off] = v;
        }
      }
    }
}

// Sum of the per-split slabs.  A workgroup covers 256/lanes float4 columns; `lanes` threads per column
// each add every lanes-th slab, then the lanes are summed through LDS in a fixed order
// (deterministic).  With one thread per column (the obvious form) a 64-channel layer has 144
// workgroups each issuing 150 dependent loads: latency-bound at ~1.2 TB/s.
// One such sum: n4 float4 columns of `splits` slabs into (accumulate: onto) dw, by the workgroups from block0 on
// (conv_split.hip's wgrad_reduce_batch_kernel runs several in one launch).  sh: 256 float4 of LDS.
struct ReduceItem {
  const float *slabs;
  float *dw;
  long long n4;
  int splits, accumulate, lanes, block0;
};
template <class Item>
__device__ __forceinline__ void wgrad_slab_sum(float4 *sh, const Item &r) {
  const int cols = 256 / r.lanes;
  const int c = threadIdx.x % cols, l = threadIdx.x / cols;
  const long long i = (long long)(blockIdx.x - r.block0) * cols + c;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < r.n4)
    for (int k = l; k < r.splits; k += r.lanes) {
      const float4 v = reinterpret_cast<const float4 *>(r.slabs)[(long long)k * r.n4 + i];
      s.x += v.x;
      s.y += v.y;
      s.z += v.z;
      s.w += v.w;
    }
  sh[threadIdx.x] = s;
  __syncthreads();
  if (l == 0 && i < r.n4) {
    float4 t = r.accumulate ? reinterpret_cast<const float4 *>(r.dw)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < r.lanes; ++k) {
      const float4 v = sh[k * cols + c];
      t.x += v.x;
      t.y += v.y;
      t.z += v.z;
      t.w += v.w;
    }
    reinterpret_cast<float4 *>(r.dw)[i] = t;
  }
}
static __global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ slabs, float *__restrict__ dw,
                                                           long long n4, int splits, int accumulate, int lanes) {
  __shared__ float4 sh[256];
  struct {          // the arguments as an item, by reference: each is still read where the sum uses it
    const float *__restrict__ const &slabs;
    float *__restrict__ const &dw;
    const long long &n4;
    const int &splits, &accumulate, &lanes;
    int block0;
  } r = {slabs, dw, n4, splits, accumulate, lanes, 0};
  wgrad_slab_sum(sh, r);
}

// Algorithmic input channels of a conv for the profiler's FLOP / byte accounting: the 7x7 stem is the
// only conv with cin == 4 and its fourth channel is zero padding (SURVEY 8(d) counts Cin = 3).
static double alg_cin(const mvg_conv_desc *d) { return d->cin == 4 ? 3.0 : (double)d->cin; }

static int ilog2_exact(int v) {
  int s = 0;
  while ((1 << s) < v) ++s;
  return ((1 << s) == v) ? s : -1;
}

static int validate(const mvg_conv_desc *d) {
  MVG_REQUIRE(d != nullptr, "conv: null descriptor");
  MVG_REQUIRE(d->groups > 0 && d->n > 0 && d->h > 0 && d->w > 0 && d->cin > 0 && d->cout > 0, "conv: bad sizes");
  MVG_REQUIRE(d->stride == 1 || d->stride == 2, "conv: stride must be 1 or 2 (got %d)", d->stride);
  MVG_REQUIRE(d->ho == (d->h + 2 * d->pad - d->r) / d->stride + 1 && d->wo == (d->w + 2 * d->pad - d->s) / d->stride + 1,
              "conv: ho/wo inconsistent with h/w/pad/stride");
  MVG_REQUIRE(d->cin % 4 == 0, "conv: cin %% 4 != 0 (%d)", d->cin);
  if (d->r * d->s > 1) {
    MVG_REQUIRE(ilog2_exact(d->cin) >= 0 && ilog2_exact(d->cout) >= 0, "conv: r*s>1 needs power-of-two channels");
  }
  MVG_REQUIRE((long long)d->n * d->ho * d->wo < (1LL << 31) && (long long)d->n * d->h * d->w < (1LL << 31),
              "conv: rows per group overflow int32");
  return 0;
}

// row tiles per group of the backward-data launch = partials per group of the fused reduce: a stride-2 launch has its
// four parity classes' tiles (classes without taps included: their pixels are masked and summed too)
[[maybe_unused]] static int dgrad_bn_partials(const mvg_conv_desc *d, int bm) {
  int parts = 0;
  for (int py = 0; py < d->stride; ++py)
    for (int px = 0; px < d->stride; ++px) {
      const int sub_h = (d->h - py + d->stride - 1) / d->stride, sub_w = (d->w - px + d->stride - 1) / d->stride;
      if (sub_h > 0 && sub_w > 0) parts += ceil_div((long long)d->n * sub_h * sub_w, bm);
    }
  return parts;
}

// One class of a launch: rows are the n images' out_h x out_w pixels, K is ntaps taps (tap_ns per filter row, the first
// at (tap_r0, tap_s0)) x src_c channels.  Tile and unit offsets are the launcher's.
static IgemmClass make_class(int n, int out_h, int out_w, int ntaps, int tap_ns, int tap_r0, int tap_s0, int src_c) {
  IgemmClass c;
  memset(&c, 0, sizeof(c));
  c.out_h = out_h;
  c.out_w = out_w;
  c.ntaps = ntaps;
  c.tap_ns = tap_ns;
  c.tap_r0 = tap_r0;
  c.tap_s0 = tap_s0;
  c.ktotal = ntaps * src_c;
  c.rows_per_group = (long long)n * out_h * out_w;
  c.tap_ns_div = make_fastdiv((unsigned)tap_ns);
  c.ohw_div = make_fastdiv((unsigned)(out_h * out_w));
  c.ow_div = make_fastdiv((unsigned)out_w);
  c.KT = c.ktotal > 0 ? ceil_div(c.ktotal, 16) : 1;
  c.korder = (ntaps > 1 && src_c % 32 == 0) ? 1 : 0;
  c.per_div = make_fastdiv((unsigned)(ntaps > 0 ? 2 * ntaps : 1));      // for BK = 16; the launchers reset it
  return c;
}

// The descriptor's fields of a forward launch (one class): a_elem / b_elem bytes per element of the gathered operand and
// of the weights.  stride_w >= 0: the horizontal stride / padding differ from d->stride / d->pad (the stems' row-window
// forms, whose descriptors their callers check).  `what` prefixes the error messages.
static int fprop_geometry(IgemmParams &p, const mvg_conv_desc *d, int a_elem, int b_elem, const char *what, int stride_w = -1,
                          int pad_w = -1) {
  p.groups = d->groups;
  p.out_h = d->ho;
  p.out_w = d->wo;
  p.src_h = d->h;
  p.src_w = d->w;
  p.src_c = d->cin;
  p.src_c_shift = (d->r * d->s > 1) ? ilog2_exact(d->cin) : 0;
  p.ncols = d->cout;
  p.r = d->r;
  p.s = d->s;
  p.rs = d->r * d->s;
  p.stride = d->stride;
  p.stride_shift = d->stride == 2 ? 1 : 0;
  p.pad = d->pad;
  p.stride_w = stride_w >= 0 ? stride_w : d->stride;
  p.pad_w = stride_w >= 0 ? pad_w : d->pad;
  p.ktotal = d->r * d->s * d->cin;
  p.b_row_len = p.ktotal;
  p.cin = d->cin;
  p.rows_per_group = (long long)d->n * d->ho * d->wo;
  p.src_img_stride = (long long)d->h * d->w * d->cin;
  p.imgs_per_group = d->n;
  p.ntaps = d->r * d->s;
  p.tap_ns = d->s;
  p.tap_step = 1;
  p.cls_step = 1;
  p.a_group_bytes = (long long)a_elem * d->n * p.src_img_stride;
  p.b_bytes = (long long)b_elem * d->cout * p.ktotal;
  MVG_REQUIRE(p.a_group_bytes < 0x7FFFFFF0ll && p.b_bytes < 0x7FFFFFF0ll, "%s: a group / the weights exceed 2 GiB", what);
  p.ncls = 1;
  p.cls[0] = make_class(d->n, d->ho, d->wo, p.ntaps, d->s, 0, 0, d->cin);
  p.tap_ns_div = p.cls[0].tap_ns_div;
  p.ohw_div = p.cls[0].ohw_div;
  p.ow_div = p.cls[0].ow_div;
  return 0;
}

// The descriptor's fields of a backward-data launch (dx = dy (*) w^T: dy gathered, the CRSK weights' rows of r*s*cout),
// before dgrad_classes splits it: a_elem / b_elem as in fprop_geometry.
static int dgrad_geometry(IgemmParams &p, const mvg_conv_desc *d, int a_elem, int b_elem, const char *what) {
  p.groups = d->groups;
  p.out_h = d->h;
  p.out_w = d->w;
  p.src_h = d->ho;
  p.src_w = d->wo;
  p.src_c = d->cout;
  p.src_c_shift = (d->r * d->s > 1) ? ilog2_exact(d->cout) : 0;
  p.ncols = d->cin;
  p.r = d->r;
  p.s = d->s;
  p.rs = d->r * d->s;
  p.stride = d->stride;
  p.stride_shift = d->stride == 2 ? 1 : 0;
  p.pad = d->pad;
  p.ktotal = d->r * d->s * d->cout;
  p.b_row_len = p.ktotal;
  p.cin = d->cin;
  p.src_img_stride = (long long)d->ho * d->wo * d->cout;
  p.imgs_per_group = d->n;
  p.full_h = d->h;
  p.full_w = d->w;
  p.a_group_bytes = (long long)a_elem * d->n * p.src_img_stride;
  p.b_bytes = (long long)b_elem * d->cin * p.b_row_len;
  MVG_REQUIRE(p.a_group_bytes < 0x7FFFFFF0ll && p.b_bytes < 0x7FFFFFF0ll, "%s: a group / the weights exceed 2 GiB", what);
  return 0;
}

// A stride-2 parity class without taps (e.g. three of the four classes of a 1x1 stride-2 conv): dx = addend, or 0, on
// that class's pixels; cv 16-byte vectors per pixel.
static __global__ __launch_bounds__(256) void dgrad_empty_class_kernel(uint4 *__restrict__ dx, const uint4 *__restrict__ addend,
                                                                       long long n, int sub_h, int sub_w, int full_h, int full_w,
                                                                       int cv, int py, int px) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int cc = (int)(i % cv);
    long long t = i / cv;
    const int x2 = (int)(t % sub_w);
    t /= sub_w;
    const int y2 = (int)(t % sub_h);
    const long long img = t / sub_h;
    const long long off = ((img * full_h + 2 * y2 + py) * full_w + 2 * x2 + px) * cv + cc;
    dx[off] = addend ? addend[off] : make_uint4(0u, 0u, 0u, 0u);
  }
}

// The classes of a backward-data launch (p from dgrad_geometry): one at stride 1; at stride 2 one per output-pixel parity
// (py, px) - each a dense sub-convolution over its own taps - all merged into p.cls, longest first (with one tile per
// workgroup the short tiles then fill the tail); the launch-wide fields are the first class's.  A class without taps is a
// class of its own when keep_tapless (a fused BatchNorm reduce: its tiles run the epilogue only); otherwise it is left
// out of p.cls and listed in `dropped` (dgrad_classes fills it).  Host arithmetic only: nothing is launched, so the
// families' plan queries (mvg_conv_dgrad_split_stages) build the same table.  p.ncls == 0 on return: no class has taps.
struct DgradDropped {
  int n;
  struct { int py, px, sub_h, sub_w; } c[4];
};
static void dgrad_plan_classes(IgemmParams &p, const mvg_conv_desc *d, bool keep_tapless, DgradDropped &dropped) {
  const int step = d->stride;
  p.ncls = 0;
  dropped.n = 0;
  for (int py = 0; py < step; ++py)
    for (int px = 0; px < step; ++px) {
      const int sub_h = (d->h - py + step - 1) / step, sub_w = (d->w - px + step - 1) / step;
      if (sub_h <= 0 || sub_w <= 0) continue;
      const int r0 = (py + d->pad) % step, s0 = (px + d->pad) % step;
      const int nr = r0 < d->r ? (d->r - r0 + step - 1) / step : 0;
      const int ns = s0 < d->s ? (d->s - s0 + step - 1) / step : 0;
      if (nr * ns == 0 && !keep_tapless) {
        dropped.c[dropped.n++] = {py, px, sub_h, sub_w};
        continue;
      }
      IgemmClass &c = p.cls[p.ncls++];
      c = make_class(d->n, sub_h, sub_w, nr * ns, ns > 0 ? ns : 1, r0, s0, d->cout);
      c.cls_py = py;
      c.cls_px = px;
      c.cls_cy = (py + d->pad - r0) / step;
      c.cls_cx = (px + d->pad - s0) / step;
      if (p.ncls == 1) {
        p.tap_step = step;
        p.cls_step = step;
        p.rows_per_group = c.rows_per_group;
        p.ktotal = c.ktotal;
        p.out_h = sub_h;
        p.out_w = sub_w;
      }
    }
  for (int i = 1; i < p.ncls; ++i)
    for (int j = i; j > 0 && p.cls[j].ktotal > p.cls[j - 1].ktotal; --j) {
      const IgemmClass t = p.cls[j];
      p.cls[j] = p.cls[j - 1];
      p.cls[j - 1] = t;
    }
  p.no_remap = p.ncls > 1;
}

// dgrad_plan_classes, and dgrad_empty_class_kernel over every dropped class: dx = addend there (nothing when the caller
// accumulates in place; dx_elem bytes per element).  p.ncls == 0 on return: nothing left to launch.
static int dgrad_classes(IgemmParams &p, const mvg_conv_desc *d, bool keep_tapless, int dx_elem, void *dx, const void *addend,
                         hipStream_t st) {
  DgradDropped dropped;
  dgrad_plan_classes(p, d, keep_tapless, dropped);
  if (addend == dx && addend) return 0;
  for (int i = 0; i < dropped.n; ++i) {
    const int cv = d->cin * dx_elem / 16;
    const long long n = (long long)d->groups * d->n * dropped.c[i].sub_h * dropped.c[i].sub_w * cv;
    long long blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(dgrad_empty_class_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (uint4 *)dx, (const uint4 *)addend, n,
                       dropped.c[i].sub_h, dropped.c[i].sub_w, d->h, d->w, cv, dropped.c[i].py, dropped.c[i].px);
    if (check_launch("dgrad(empty class)")) return 1;
  }
  return 0;
}

// The descriptor's fields of a weight-gradient launch and where its result goes: elem bytes per element of x and dy, each
// of the `splits` pixel ranges a multiple of px_align pixels (the kernel's K-step), stride_w / pad_w as in fprop_geometry.
// With splits > 1 the kernel writes fp32 slabs [splits][cout][r*s*cin] (then [splits][cout] of db) to the workspace and
// wgrad_reduce_slabs sums them.  The tile is the family's.
static int wgrad_geometry(WgradParams &p, const mvg_conv_desc *d, int elem, int px_align, float *dw, float *db, float *workspace,
                          int splits, int accumulate, const char *what, int stride_w = -1, int pad_w = -1) {
  MVG_REQUIRE(splits >= 1, "%s: splits < 1", what);
  MVG_REQUIRE(splits == 1 || workspace != nullptr, "%s: workspace required for splits > 1", what);
  p.h = d->h;
  p.w = d->w;
  p.cin = d->cin;
  p.cout = d->cout;
  p.r = d->r;
  p.s = d->s;
  p.stride = d->stride;
  p.pad = d->pad;
  p.stride_w = stride_w >= 0 ? stride_w : d->stride;
  p.pad_w = stride_w >= 0 ? pad_w : d->pad;
  p.ho = d->ho;
  p.wo = d->wo;
  p.ncols = d->r * d->s * d->cin;
  p.pixels = (long long)d->groups * d->n * d->ho * d->wo;
  p.pixels_per_split = ((p.pixels + splits - 1) / splits + px_align - 1) / px_align * px_align;
  p.x_bytes = (long long)elem * d->groups * d->n * d->h * d->w * d->cin;
  p.ohw_div = make_fastdiv((unsigned)(d->ho * d->wo));
  p.wo_div = make_fastdiv((unsigned)d->wo);
  p.cin_div = make_fastdiv((unsigned)d->cin);
  p.s_div = make_fastdiv((unsigned)d->s);
  MVG_REQUIRE(p.pixels_per_split * d->cout * elem < 0x7FFFFFF0ll, "%s: split too large for 32-bit offsets", what);
  MVG_REQUIRE((long long)elem * (p.pixels_per_split / (d->ho * d->wo) + 2) * d->h * d->w * d->cin < 0x7FFFFFF0ll,
              "%s: split too large for 32-bit offsets", what);
  p.out = splits == 1 ? dw : workspace;
  p.accumulate = (splits == 1) ? accumulate : 0;
  p.db = db ? (splits == 1 ? db : workspace + (size_t)splits * d->cout * p.ncols) : nullptr;
  return 0;
}

// threads per float4 column of the slab sum (wgrad_slab_sum)
static int wgrad_reduce_lanes(int splits) { return splits >= 32 ? 16 : (splits >= 8 ? 4 : 1); }

// The sums of a pixel-split weight gradient's slabs into dw (and of the bias slabs after them into db, when given).
static int wgrad_reduce_slabs(const WgradParams &p, float *workspace, float *dw, float *db, int splits, int accumulate, hipStream_t st,
                              const char *what) {
  const long long n = (long long)p.cout * p.ncols;
  MVG_REQUIRE(n % 4 == 0, "%s: weight elements %% 4 != 0", what);
  ProfScope ps(MVG_K_WGRAD_REDUCE, st, 0.0, 4.0 * n * (splits + 1));
  const int lanes = wgrad_reduce_lanes(splits);
  const long long blocks = (n / 4 + 256 / lanes - 1) / (256 / lanes);
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, workspace, dw, n / 4, splits, accumulate, lanes);
  if (check_launch("wgrad_reduce")) return 1;
  if (!db) return 0;
  const long long nb = p.cout;
  const long long bblocks = (nb / 4 + 256 / lanes - 1) / (256 / lanes);
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)bblocks), dim3(256), 0, st, workspace + (size_t)splits * n, db, nb / 4, splits,
                     accumulate, lanes);
  return check_launch("wgrad_reduce(bias)");
}

// Pixel splits of a weight gradient over `tiles` output tiles: one resident round of workgroups_per_cu per CU (rounding
// the split count UP puts a handful of workgroups into a second round that costs as much as the first), at least
// min_pixels pixels per split, at most 1024 splits.
static int wgrad_split_count(long long tiles, long long pixels, int workgroups_per_cu, int min_pixels) {
  long long want = ((long long)workgroups_per_cu * compute_cus()) / tiles;
  long long maxs = pixels / min_pixels;
  if (maxs < 1) maxs = 1;
  if (want > maxs) want = maxs;
  if (want < 1) want = 1;
  if (want > 1024) want = 1024;
  return (int)want;
}

// output tiles of a weight gradient at the family's bm x bn tile
static long long wgrad_tiles(const mvg_conv_desc *d, int bm, int bn) {
  return (long long)ceil_div(d->cout, bm) * ceil_div(d->r * d->s * d->cin, bn);
}

// A weight-gradient launch of any family, the caller's fields of p set: geometry (elem, px_align, stride_w / pad_w as in
// wgrad_geometry), the bm x bn tiles, the profiler's family (flops, bytes: the caller's accounting), the kernel through
// dispatch(grid, block, st, p) - the family's tile -> instantiation switch; nonzero = its error
// (the fuser's shape check) - and, unless the slabs
// are the result (slabs_only), their sum.  `what` prefixes the error messages, launch_name names the launch check's.
template <class Dispatch>
static int wgrad_launch(WgradParams &p, const mvg_conv_desc *d, int elem, int px_align, int bm, int bn, float *dw, float *db,
                        float *workspace, int splits, int accumulate, bool slabs_only, hipStream_t st, double flops, double bytes,
                        const char *what, const char *launch_name, int stride_w, int pad_w, Dispatch dispatch) {
  if (wgrad_geometry(p, d, elem, px_align, dw, db, workspace, splits, accumulate, what, stride_w, pad_w)) return 2;
  p.mtiles = ceil_div(d->cout, bm);
  p.ntiles = ceil_div(p.ncols, bn);
  {
    const bool lin = d->r == 1 && d->s == 1 && d->h == 1 && d->w == 1;
    ProfScope ps(lin ? MVG_K_LINEAR_WGRAD : MVG_K_CONV_WGRAD, st, flops, bytes);
    MVG_REQUIRE(wgrad_tiles(d, bm, bn) * splits < (1LL << 31), "%s: grid too large", what);
    if (int e = dispatch(dim3(p.mtiles * p.ntiles * splits), dim3(256), st, p)) return e;
    if (check_launch(launch_name)) return 1;
  }
  return splits > 1 && !slabs_only ? wgrad_reduce_slabs(p, workspace, dw, db, splits, accumulate, st, what) : 0;
}

}  // namespace mvg
