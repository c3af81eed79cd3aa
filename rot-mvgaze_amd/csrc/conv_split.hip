// fp32-accurate convolution / linear kernels on the gfx950 fp16 matrix cores ("split" operands).
//
// An fp32 value a is held as TWO fp16 pieces, a1 = fp16(a), a2 = fp16(a - a1) (round to nearest; a - a1 is exact):
// |a - a1 - a2| <= 2^-23 |a| - at most the last of the 24 significand bits is lost, three values in four are exact, rms
// 0.74 * 2^-24 |a| - provided the value sits inside fp16's exponent range, which a per-tensor power-of-two scale
// arranges (exact to apply and to undo; elem.h: sp_t).
// A product of two pieces is exact in fp32, so
//     a * b  =  a1 b1 + (a1 b2 + a2 b1)  + O(2^-22 |a b|)
// THREE fp16 MFMAs (v_mfma_f32_16x16x32_f16, fp32 accumulation) per 32 k.  Measured against fp64 (DESIGN.md 4a,
// profiles/r03_split_accuracy.txt): the result is as close as the fp32-MFMA kernel's, whose own k-ordered fp32
// accumulation error (1.5-4e-7 relative L2) is larger than what the operand rounding (6e-8) and the dropped a2 b2
// term (4e-8) contribute.  Round 2 used three bf16 pieces and six products ("s3", exact operands, 6 bytes per
// element): this format moves 4 bytes per element and half the MFMA work.
// This is the 1e-4 parity path's arithmetic, NOT the reduced-precision bf16 path of conv_bf16.hip.
//
// Operand format "sp" (written by the producers: bn.hip's apply passes, the weight prep below): channels in chunks
// of 8, the two pieces of a chunk adjacent - element (row, c, piece) at ushort offset
//     ((row * C/8 + c/8) * 2 + piece) * 8 + c % 8            (32 contiguous bytes per 8 channels, 4 bytes/element)
// Scales: activations are stored unscaled (BatchNorm keeps them O(1); fp16 reaches 65504); every gradient tensor dy
// and every weight copy carries a device scalar 2^-k written by its producer (bn_bwd_apply: from a bound on |dy|;
// the weight prep: from max |w|), which the consumer's epilogue multiplies back in.
//
// Kernels: igemm_split16_kernel (fprop and dgrad, uniform-tap shapes with channels % 32 == 0; below) and
// wgrad_split_kernel.  fp32 output through the LDS-staged epilogue of bf16_tile.h (BN statistics partials, addend;
// backward-data can carry the BatchNorm-backward reduce pass of the unit it feeds: mvg_conv_dgrad_split_bnreduce).
#include "bf16_tile.h"
#include "elem.h"

namespace mvg {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// acc[i][j] += the three piece products of fragments av[piece][i], bv[piece][j] (32x32x16 tiles: wgrad); smallest
// terms first: (a1 b2, a2 b1), a1 b1
#define SPLIT_ONE(PA, PB, av, bv, acc)                                                                         \
  _Pragma("unroll") for (int i = 0; i < TM; ++i) _Pragma("unroll") for (int j = 0; j < TN; ++j)                \
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[PA][i], bv[PB][j], acc[i][j], 0, 0, 0);
#define SPLIT_PRODUCTS(av, bv, acc) SPLIT_ONE(0, 1, av, bv, acc) SPLIT_ONE(1, 0, av, bv, acc) SPLIT_ONE(0, 0, av, bv, acc)

constexpr int SP_BM = 128, SP_BK = 32;

// fp32 [n8 * 8] * scale -> sp (layout plumbing for tests and for tensors no kernel writes in sp directly)
__global__ __launch_bounds__(256) void split_f32_kernel(const float4 *__restrict__ x, uint4 *__restrict__ out, long long n8, float scale) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
    const float4 lo = x[2 * i], hi = x[2 * i + 1];
    const float v[8] = {lo.x * scale, lo.y * scale, lo.z * scale, lo.w * scale, hi.x * scale, hi.y * scale, hi.z * scale, hi.w * scale};
    uint4 q1, q2;
    split2_chunk(v, q1, q2);
    out[2 * i] = q1;
    out[2 * i + 1] = q2;
  }
}

// split_f32_kernel plus the activation range record of what it stores (bf16_tile.h: range_commit) - the stem's pooled map, the
// only sp tensor of the guarded inference forward that no conv epilogue writes
__global__ __launch_bounds__(256) void split_f32_ranged_kernel(const float4 *__restrict__ x, uint4 *__restrict__ out, long long n8, float scale,
                                                               unsigned *__restrict__ range_word) {
  __shared__ unsigned red[4];
  const long long stride = (long long)gridDim.x * 256;
  unsigned mx = 0u;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
    const float4 lo = x[2 * i], hi = x[2 * i + 1];
    const float v[8] = {lo.x * scale, lo.y * scale, lo.z * scale, lo.w * scale, hi.x * scale, hi.y * scale, hi.z * scale, hi.w * scale};
#pragma unroll
    for (int k = 0; k < 8; ++k) mx = range_bits(mx, v[k]);
    uint4 q1, q2;
    split2_chunk(v, q1, q2);
    out[2 * i] = q1;
    out[2 * i + 1] = q2;
  }
  range_commit(mx, red, range_word, (int)threadIdx.x);
}

// sp -> fp32: (piece 1 + piece 2) * inv_scale
__global__ __launch_bounds__(256) void merge_sp_kernel(const uint4 *__restrict__ x, float4 *__restrict__ out, long long n8, float inv_scale) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
    float v[8];
    merge2_chunk(x[2 * i], x[2 * i + 1], v);
    out[2 * i] = make_float4(v[0] * inv_scale, v[1] * inv_scale, v[2] * inv_scale, v[3] * inv_scale);
    out[2 * i + 1] = make_float4(v[4] * inv_scale, v[5] * inv_scale, v[6] * inv_scale, v[7] * inv_scale);
  }
}

// A gradient g [rows][cols] of the fusion block on its way into the split kernels, ONE launch: g -> sp times the 2^k that
// max |g| allows (the maximum was left in *absmax - float bits - by g's producer: the LIN epilogue's atomicMax, or
// fuse_unbuild / skinny_bwd_dx), *out_sinv = 2^-k, and db (+)= the column sums of g (the Linear's bias gradient).
// Workgroup = 32 columns (4 chunks of 8) x 64 row lanes; the row lanes are added through LDS in lane order (reproducible).
__global__ __launch_bounds__(256) void split_colsum_kernel(const float *__restrict__ g, int rows, int cols, const unsigned *__restrict__ absmax,
                                                           uint4 *__restrict__ out, float *__restrict__ out_sinv, float *__restrict__ db,
                                                           int accumulate) {
  __shared__ float sh[64][33];
  const float scale = sp_scale_for(__uint_as_float(*absmax));
  if (blockIdx.x == 0 && threadIdx.x == 0) *out_sinv = 1.f / scale;
  const int cl = threadIdx.x & 3, rl = threadIdx.x >> 2;
  const int c8 = blockIdx.x * 4 + cl, c8n = cols >> 3;
  float sum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r = rl; r < rows; r += 64) {
    const float4 *src = reinterpret_cast<const float4 *>(g + (long long)r * cols + c8 * 8);
    const float4 lo = src[0], hi = src[1];
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    float w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      sum[k] += v[k];
      w[k] = v[k] * scale;
    }
    uint4 q1, q2;
    split2_chunk(w, q1, q2);
    uint4 *dst = out + SP_NP * ((long long)r * c8n + c8);
    dst[0] = q1;
    dst[1] = q2;
  }
  if (db == nullptr) return;
#pragma unroll
  for (int k = 0; k < 8; ++k) sh[rl][cl * 8 + k] = sum[k];
  __syncthreads();
  if (threadIdx.x < 32) {
    const int col = blockIdx.x * 32 + threadIdx.x;
    float t = accumulate ? db[col] : 0.f;
    for (int r = 0; r < 64; ++r) t += sh[r][threadIdx.x];
    db[col] = t;
  }
}

// Every conv's weight copies of one training step in TWO launches (grid.y = conv): (1) max |w| per conv, (2) the
// copies.  mode 1: fp32 KRSC -> sp KRSC (+ sp CRSK), both scaled by 2^k with max |w| * 2^k just below 2^15, and
// wstat[conv] = {max |w| bits, 2^-k} for the consumers' epilogues; mode 0: -> bf16 KRSC (cin zero-padded to cin_pad)
// (+ bf16 CRSK), conv_bf16.hip's layouts (no scale).
struct WPrepItem {
  const float *w;
  void *wk, *wt;
  int cout, rs, cin, cin_pad;
  float *stat;               // mode 1: [2] device floats {max |w| as uint bits (zero before the absmax launch), 2^-k}
};

// one record -> device memory, its stat pair cleared (mvg_split_weights: the single-conv form of the batched prep)
__global__ void wprep_stage_item_kernel(WPrepItem it, WPrepItem *__restrict__ dst) {
  if (threadIdx.x == 0) *dst = it;
  if (threadIdx.x < 2) it.stat[threadIdx.x] = 0.f;
}

__global__ __launch_bounds__(256) void weights_absmax_kernel(const WPrepItem *__restrict__ items) {
  const WPrepItem it = items[blockIdx.y];
  const long long n4 = (long long)it.cout * it.rs * it.cin / 4;
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4 *>(it.w)[i];
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(reinterpret_cast<unsigned *>(it.stat), __float_as_uint(m));
}

__global__ __launch_bounds__(256) void weights_prep_batch_kernel(const WPrepItem *__restrict__ items, int mode) {
  __shared__ float tile[64][65];             // 1x1 / Linear weights: the transposed copy goes through LDS
  const WPrepItem it = items[blockIdx.y];
  const float *__restrict__ w = it.w;
  const int cout = it.cout, rs = it.rs, cin = it.cin;
  if (mode == 1) {
    const float scale = sp_scale_for(__uint_as_float(*reinterpret_cast<const unsigned *>(it.stat)));
    if (blockIdx.x == 0 && threadIdx.x == 0) it.stat[1] = 1.f / scale;
    uint4 *wk = reinterpret_cast<uint4 *>(it.wk), *wt = reinterpret_cast<uint4 *>(it.wt);
    const int c8n = cin / 8, o8n = cout / 8;
    // 1x1 weights with 64-divisible sides (the fusion block's 3584 x 3584 Linears: 51 MB each): the CRSK copy as a tiled
    // transpose - rows read as float4, 8-output-channel chunks written 256 contiguous bytes per input channel.  (The
    // gather below reads 8 floats at a stride of cin per chunk: fine for the backbone's convs, 1 ms per Linear.)
    const bool tiled = wt != nullptr && rs == 1 && (cin % 64) == 0 && (cout % 64) == 0;
    const long long nk = (long long)cout * rs * c8n, nt = (wt && !tiled) ? (long long)cin * rs * o8n : 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nk + nt; i += (long long)gridDim.x * 256) {
      float v[8];
      uint4 *dst;
      if (i < nk) {
        const float4 *src = reinterpret_cast<const float4 *>(w + i * 8);          // (o, tap, c8) is the KRSC order itself
        const float4 lo = src[0], hi = src[1];
        v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
        dst = wk + SP_NP * i;
      } else {
        const long long j = i - nk;
        const int o8 = (int)(j % o8n);
        const long long t = j / o8n;
        const int tap = (int)(t % rs), c = (int)(t / rs);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = w[((long long)(o8 * 8 + k) * rs + tap) * cin + c];
        dst = wt + SP_NP * j;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] *= scale;
      uint4 q1, q2;
      split2_chunk(v, q1, q2);
      dst[0] = q1;
      dst[1] = q2;
    }
    if (tiled) {
      const int tc = cin / 64, ntiles = (cout / 64) * tc;
      for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int o0 = (t / tc) * 64, c0 = (t % tc) * 64;
        __syncthreads();                                       // the previous tile has been read out
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
          const int r = (threadIdx.x >> 4) + 16 * ps, cq = threadIdx.x & 15;
          const float4 x = *reinterpret_cast<const float4 *>(w + (long long)(o0 + r) * cin + c0 + 4 * cq);
          tile[r][4 * cq] = x.x;
          tile[r][4 * cq + 1] = x.y;
          tile[r][4 * cq + 2] = x.z;
          tile[r][4 * cq + 3] = x.w;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int idx = threadIdx.x + 256 * q, cl = idx >> 3, o8 = idx & 7;
          float v[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] = tile[o8 * 8 + k][cl] * scale;
          uint4 q1, q2;
          split2_chunk(v, q1, q2);
          uint4 *dst = wt + SP_NP * ((long long)(c0 + cl) * o8n + (o0 >> 3) + o8);
          dst[0] = q1;
          dst[1] = q2;
        }
      }
    }
    return;
  }
  unsigned short *wk = reinterpret_cast<unsigned short *>(it.wk), *wt = reinterpret_cast<unsigned short *>(it.wt);
  const int cin_pad = it.cin_pad;
  const long long total = (long long)cout * rs * cin_pad;
  if (rs == 1 && cin == cin_pad && (cin % 64) == 0 && (cout % 64) == 0) {
    // Linear weights (the fusion block in the bf16 path: 3584 x 3584 and the like): 16-byte accesses for the plain copy,
    // the transposed copy as a tiled transpose (the per-element form below writes it 2 bytes at a stride of cout)
    uint4 *wk4 = reinterpret_cast<uint4 *>(wk);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total / 8; i += (long long)gridDim.x * 256) {
      const float4 lo = reinterpret_cast<const float4 *>(w + i * 8)[0], hi = reinterpret_cast<const float4 *>(w + i * 8)[1];
      wk4[i] = make_uint4(bf16_pack2(lo.x, lo.y), bf16_pack2(lo.z, lo.w), bf16_pack2(hi.x, hi.y), bf16_pack2(hi.z, hi.w));
    }
    if (wt) {
      const int tc = cin / 64, ntiles = (cout / 64) * tc;
      for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int o0 = (t / tc) * 64, c0 = (t % tc) * 64;
        __syncthreads();
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
          const int r = (threadIdx.x >> 4) + 16 * ps, cq = threadIdx.x & 15;
          const float4 x = *reinterpret_cast<const float4 *>(w + (long long)(o0 + r) * cin + c0 + 4 * cq);
          tile[r][4 * cq] = x.x;
          tile[r][4 * cq + 1] = x.y;
          tile[r][4 * cq + 2] = x.z;
          tile[r][4 * cq + 3] = x.w;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int idx = threadIdx.x + 256 * q, cl = idx >> 3, o8 = idx & 7;
          float v[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] = tile[o8 * 8 + k][cl];
          *reinterpret_cast<uint4 *>(wt + (long long)(c0 + cl) * cout + o0 + o8 * 8) =
              make_uint4(bf16_pack2(v[0], v[1]), bf16_pack2(v[2], v[3]), bf16_pack2(v[4], v[5]), bf16_pack2(v[6], v[7]));
        }
      }
    }
    return;
  }
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % cin_pad);
    const long long t = i / cin_pad;
    const int tap = (int)(t % rs), o = (int)(t / rs);
    const float v = c < cin ? w[((long long)o * rs + tap) * cin + c] : 0.f;
    const __bf16 b = (__bf16)v;
    const unsigned short u = __builtin_bit_cast(unsigned short, b);
    wk[i] = u;
    if (wt) wt[((long long)c * rs + tap) * cout + o] = u;
  }
}

// ------------------------------------------------------------------------------------------
// igemm_split16_kernel: 128 x BN x 32 tile, 4 waves as 2 x 2 (wave tile 64 x BN/2), v_mfma_f32_16x16x32_f16, a
// "span" LDS-DMA loader, ONE stage of (128 + BN) x 128 bytes (32 KB) and three (backward-data) or four (forward)
// workgroups per CU, which cover each other's DMA waits and epilogues.
//
// What scripts/kloop_probe.hip measured (a GEMM sandbox with this tile and a 3x3 conv's operand reuse; MI355X,
// profiles/r03_kloop_probe*.txt), step by step from round 2's kernel (three bf16 pieces, 32x32x16 MFMAs,
// piece-major LDS image) at K = 2304 / 1024:
//   * span loader: 175 -> 196, 138 -> 164 TF/s.  One LDS-DMA wave-instruction used to fetch, for 16 rows, the four
//     16-byte chunks of ONE piece - 64 segments of 16 bytes at a 48-byte stride, the pieces' instructions re-touching
//     the same 128-byte lines.  Now an instruction covers 64 CONSECUTIVE 16-byte slots of a row-major LDS image whose
//     rows are the contiguous bytes a row contributes to a K-step (4 chunks x 2 pieces = 128 bytes): 8 whole rows.
//     No padding: the slot of (chunk cc, piece pc) in row R is (2 cc + pc) ^ h(R), h(R) = ((R >> 1) & 1) |
//     (((R >> 2) & 1) << 2), filled by permuting the SOURCE address inside the row's span (the DMA destination is
//     linear in the lane); a ds_read_b128 of a 16x16x32 fragment (lane: row l & 15, chunk l >> 4) is conflict-free
//     (brute-force check: DESIGN.md 4a).
//   * 16x16x32 instead of 32x32x16 MFMAs: 196 -> 214, 164 -> 177.  Same cycles per flop and the same LDS reads per
//     K-step, but an MFMA-dense loop is clock-limited by power on this chip and holds a higher clock on this shape
//     (MI355X_MICROARCH.md, DVFS give-back 7).
//   * two fp16 pieces and three products instead of three bf16 pieces and six: 214 -> 366, 177 -> 291.
// Row -> address: every lane needs the base offset and tap-validity mask of FOUR rows (one per A instruction it
// issues); thread r computes row r's once and the lanes pick theirs up through LDS.
// ------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define SPLIT16_ONE(PA, PB)                                                                       \
  _Pragma("unroll") for (int i = 0; i < TM; ++i) _Pragma("unroll") for (int j = 0; j < TN; ++j)   \
      acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[PA][i], bv[PB][j], acc[i][j], 0, 0, 0);

__device__ __forceinline__ int sp_row_swz(int R) { return ((R >> 1) & 1) | (((R >> 2) & 1) << 2); }

// WGM = 4 (BN = 64 only): a 256 x 64 tile as four wave rows of 64 x 64 - the same accumulators and fragment reuse per wave as
// the 128 x 128 tile - for the layers with 64 GEMM columns (64-channel 3x3 convs), where the 128 x 64 tile's 64 x 32 wave tiles
// re-read every A fragment for half the products.
//
// STAGES = 2 (launches that leave a CU one or two workgroups - the fusion block's Linears, 48 - 336 tiles of up to 112 K-steps on
// 256 CUs; every conv of a small batch - so that nobody covers a workgroup's waits): an explicit software pipeline, see the K loop.
//
// AF != A_DMA (1x1, stride 1, ONE column tile, one stage): the A operand does not exist yet - a launch that would follow a BatchNorm
// pass forms that pass's result in its own loader.  Thread t takes chunk t & 3 of rows t >> 2 and 64 + (t >> 2), so four lanes cover
// a row's 128-byte line of each fp32 map; per K-step it loads its two chunks' inputs into registers, forms the 8 values with the
// pass's own function (bn_math.h: the sp pass of bn.hip calls the same one), writes the two fp16 pieces into the slots the fragment
// reads expect and stores the same 32 bytes ONCE to the global sp operand `a` (plain stores: later launches re-read it).  Every
// element belongs to exactly one workgroup and one K-step: the pass's three trips over the map (two reads, one write) plus this
// launch's read become three.  The weights keep their DMA path.  The A fragments hold the bits the two-launch form reads back from
// memory, in the same K order, and tiles and epilogue are the DMA kernels': results are those of that form, bit for bit.  The group's
// per-channel constants wait in LDS behind the row table.  Three workgroups per CU (168 registers).
// What differs between the passes is a "former" (below): which maps it reads, which constants it stages, the chunk function.
//   * A_DY (backward-data of ResNet-50's layer1 / layer2 conv3 - K = cout wide, N = cin <= 128 - with the fused reduce on board;
//     IgemmParams::bna_*): dy = bn_dy(dz, y, ...) * 2^k as bn_bwd_apply_sp_kernel; 5 x cout constants; dy is re-read by the weight
//     gradient.
//   * A_OUT_SP / A_OUT_AFFINE (forward of a residual block's FIRST conv, cout 64 / 128, in ResNet-50's layer1 / layer2;
//     IgemmParams::fap_*): the previous block's output, out = relu(bn_fwd(y, scale, shift) + residual) * 2^k as bn_apply_sp_kernel,
//     the residual being the sp identity times its 2^-k or the raw fp32 downsample output through its own (scale, shift); 2 / 4 x cin
//     constants; also stores the chunk's ReLU mask bits; out is re-read by the downsample conv, the next apply and the weight gradients.
enum AForm : int { A_DMA = 0, A_DY = 1, A_OUT_SP = 2, A_OUT_AFFINE = 3 };
constexpr int BNA_MAX_C = 512;                                  // channels of the constants' LDS table

__device__ __forceinline__ void unpack8(const float4 (&v)[2], float (&o)[8]) {
  o[0] = v[0].x; o[1] = v[0].y; o[2] = v[0].z; o[3] = v[0].w; o[4] = v[1].x; o[5] = v[1].y; o[6] = v[1].z; o[7] = v[1].w;
}

// A former: stage() the group's constants into the LDS table, once per tile; load(i, byte_off) issues row half i's loads into member
// registers; consts(kc, C) this K-step's 8 channels' constants; form(i, ok, o) the chunk; store_extra(i, byte_off) what leaves with it.
struct DyFormer {
  static constexpr int TABLES = 5;                            // [5][C] mean, invstd, gamma, s1, s2 of this group
  __amdgpu_buffer_rsrc_t rs_dz, rs_y;
  float inv_rows, dsc;
  float4 dzv[2][2], yv[2][2];
  float mu[8], is[8], ga[8], sa[8], sb[8];
  static __device__ __forceinline__ void stage(float *t, const IgemmParams &p, int g, int C, int tid) {
    for (int i = tid; i < C; i += 256) {
      const long long gc = (long long)g * C + i;
      t[i] = p.bna_mean[gc];
      t[C + i] = p.bna_invstd[gc];
      t[2 * C + i] = p.bna_gamma[i];
      t[3 * C + i] = p.bna_s1[gc];
      t[4 * C + i] = p.bna_s2[gc];
    }
  }
  __device__ __forceinline__ DyFormer(const IgemmParams &p, long long grow0, long long rows_per_group, int C)
      : rs_dz(make_rsrc(p.bna_dz + grow0 * C, 4ll * rows_per_group * C)), rs_y(make_rsrc(p.bna_y + grow0 * C, 4ll * rows_per_group * C)),
        inv_rows(p.bna_inv_rows), dsc(1.f / *p.a_sinv) {}      // 2^k (exact: a power of two)
  __device__ __forceinline__ void load(int i, unsigned off) {
    dzv[i][0] = buf_ld16(rs_dz, off);
    dzv[i][1] = buf_ld16(rs_dz, off + 16u);
    yv[i][0] = buf_ld16(rs_y, off);
    yv[i][1] = buf_ld16(rs_y, off + 16u);
  }
  __device__ __forceinline__ void consts(const float *kc, int C) {
    ld8(kc, mu);
    ld8(kc + C, is);
    ld8(kc + 2 * C, ga);
    ld8(kc + 3 * C, sa);
    ld8(kc + 4 * C, sb);
  }
  __device__ __forceinline__ void form(int i, bool ok, float (&o)[8]) {
    float d[8], v[8];
    unpack8(dzv[i], d);
    unpack8(yv[i], v);
    bn_dy_chunk(d, v, mu, is, ga, sa, sb, inv_rows, dsc, o, false, mu, mu);          // (dz arrives masked)
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = ok ? o[k] : 0.f;        // rows beyond the group: the zeros the DMA loader reads there
  }
  __device__ __forceinline__ void store_extra(int, unsigned) {}
};

template <bool AFFINE>
struct OutFormer {
  static constexpr int TABLES = AFFINE ? 4 : 2;                // [2 | 4][C] scale, shift (, res_scale, res_shift) of this group
  __amdgpu_buffer_rsrc_t rs_y, rs_r;
  float osc, rsi;
  unsigned short *bits_out;
  float4 yv[2][2], rv[2][2];                                   // rv: the identity's two pieces (bits), or fp32
  float sc[8], sh[8], rs[8], rh[8];
  unsigned mb[2];
  static __device__ __forceinline__ void stage(float *t, const IgemmParams &p, int g, int C, int tid) {
    for (int i = tid; i < C; i += 256) {
      const long long gc = (long long)g * C + i;
      t[i] = p.fap_scale[gc];
      t[C + i] = p.fap_shift[gc];
      if constexpr (AFFINE) {
        t[2 * C + i] = p.fap_res_scale[gc];
        t[3 * C + i] = p.fap_res_shift[gc];
      }
    }
  }
  // osc: 2^k of out, rsi: 2^-k of the identity (exact: powers of two; uniform: scalar registers)
  __device__ __forceinline__ OutFormer(const IgemmParams &p, long long grow0, long long rows_per_group, int C)
      : rs_y(make_rsrc(p.fap_y + grow0 * C, 4ll * rows_per_group * C)),
        rs_r(make_rsrc(reinterpret_cast<const float *>(p.fap_res) + grow0 * C, 4ll * rows_per_group * C)),
        osc(__uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(p.a_sinv ? 1.f / *p.a_sinv : 1.f)))),
        rsi(__uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint((!AFFINE && p.fap_res_sinv) ? *p.fap_res_sinv : 1.f)))),
        bits_out(p.fap_bits ? p.fap_bits + grow0 * (C >> 3) : nullptr) {}                       // one per chunk
  __device__ __forceinline__ void load(int i, unsigned off) {
    yv[i][0] = buf_ld16(rs_y, off);
    yv[i][1] = buf_ld16(rs_y, off + 16u);
    rv[i][0] = buf_ld16(rs_r, off);
    rv[i][1] = buf_ld16(rs_r, off + 16u);
  }
  __device__ __forceinline__ void consts(const float *kc, int C) {
    ld8(kc, sc);
    ld8(kc + C, sh);
    if constexpr (AFFINE) {
      ld8(kc + 2 * C, rs);
      ld8(kc + 3 * C, rh);
    }
  }
  __device__ __forceinline__ void form(int i, bool ok, float (&o)[8]) {
    float v[8], r[8];
    unpack8(yv[i], v);
    if constexpr (AFFINE) {
      unpack8(rv[i], r);
    } else {
      const uint4 r1 = make_uint4(__float_as_uint(rv[i][0].x), __float_as_uint(rv[i][0].y), __float_as_uint(rv[i][0].z), __float_as_uint(rv[i][0].w));
      const uint4 r2 = make_uint4(__float_as_uint(rv[i][1].x), __float_as_uint(rv[i][1].y), __float_as_uint(rv[i][1].z), __float_as_uint(rv[i][1].w));
      merge2_chunk(r1, r2, r);
    }
    mb[i] = bn_apply_chunk(v, sc, sh, true, r, AFFINE, rs, rh, !AFFINE, rsi, true, osc, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = ok ? o[k] : 0.f;        // rows beyond the group: the zeros the DMA loader reads there
  }
  __device__ __forceinline__ void store_extra(int i, unsigned off) {
    if (bits_out) bits_out[off >> 5] = (unsigned short)mb[i];
  }
};

//
// The kernel itself lives in conv_split_igemm.inc: once as igemm_split16_kernel, once as igemm_split16_ranged_kernel, the guarded
// inference forward's form with the activation range record in its epilogue (mvg_conv_fprop_split_affine_ranged).
#define MVG_SPLIT_RNG 0
#include "conv_split_igemm.inc"
#undef MVG_SPLIT_RNG
#define MVG_SPLIT_RNG 1
#include "conv_split_igemm.inc"
#undef MVG_SPLIT_RNG

// ------------------------------------------------------------------------------------------
// wgrad: dw[o][tap][c] = sum over pixels of dy[pix][o] * x[pix at tap][c] with both operands in sp.  M = cout,
// N = (tap, c), K = pixels split into slabs; tile decode, column and pixel addressing and the epilogue are conv_shared.h's
// (wgrad_tile_id, wgrad_column, WgradPixel, wgrad_store_acc).  The LDS images stay pixel-major
// [piece][k][m] (rows padded by 32 elements) and the fragments come from ds_read_b64_tr_b16 (v_mfma_f32_32x32x16_f16,
// three products per 16 pixels).  A K-step is 16 pixels: 20 KB per stage, two stages; a thread's two piece vectors of
// one 8-channel chunk are 32 contiguous bytes in memory.  The result is multiplied by dy's 2^-k (p.dy_sinv).
// Round 4 measured the forward kernel's recipe here too (LDS-DMA loader into a row-contiguous image, ds_read_b64_tr_b16
// fragments, v_mfma_f32_16x16x32_f16, K-step 32; commit history + profiles/r04_wgrad_dma_*_ab.txt): 19.1 ms per C3 step with
// one 32 KB stage at three workgroups per CU, 29.4 ms with two stages at two per CU, against this kernel's 15.2-15.9 ms -
// K here is the pixel axis (hundreds of steps, both operands streamed once), and the register-staged two-stage pipeline
// with a 16-pixel step keeps more loads in flight per CU than a DMA stage that must drain before it is multiplied.
// ------------------------------------------------------------------------------------------
template <int BM, int BN, bool INCR>
__global__ __launch_bounds__(256, BN >= 256 ? 2 : 3) void wgrad_split_kernel(WgradParams p) {
  constexpr int BK = 16, WGM = 2, WGN = 2;
  constexpr int WTM = BM / WGM, WTN = BN / WGN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int LDA = BM + 32, LDB = BN + 32;
  constexpr int MV = BM / 8, NVB = BN / 8;
  constexpr int A_TPR = 256 / BK;                       // threads per k-row (16)
  constexpr int A_CPT = MV / A_TPR > 0 ? MV / A_TPR : 1;   // chunks per thread
  constexpr int B_CPT = (NVB + A_TPR - 1) / A_TPR;         // (192 columns: 24 chunks on 16 lanes - the second round half idle)
  constexpr int A_ELEMS = BK * LDA, B_ELEMS = BK * LDB;    // one piece
  constexpr int STAGE = SP_NP * (A_ELEMS + B_ELEMS);
  __shared__ __attribute__((aligned(16))) unsigned short smem[2 * STAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN;
  const int li = lane & 31, lh = lane >> 5;
  const WgradTile t = wgrad_tile_id(p);

  const char *dy = reinterpret_cast<const char *>(p.dy);
  const char *x = reinterpret_cast<const char *>(p.x);
  const __amdgpu_buffer_rsrc_t rs_a = make_rsrc(dy + t.m_begin * p.cout * SP_BYTES, (long long)SP_BYTES * t.m_count * p.cout);
  const long long x_img_elems = (long long)p.h * p.w * p.cin;
  const __amdgpu_buffer_rsrc_t rs_b = make_rsrc(x + t.img0 * x_img_elems * SP_BYTES, p.x_bytes - (long long)SP_BYTES * t.img0 * x_img_elems);
  // both loaders: pixel row i_row = tid / 16, chunk lane i_v0 = tid % 16 (+ 16 per extra chunk)
  const int i_row = tid / A_TPR, i_v0 = tid % A_TPR;
  unsigned a_off[A_CPT];
  bool a_on[A_CPT];
#pragma unroll
  for (int j = 0; j < A_CPT; ++j) {
    const int cv = i_v0 + j * A_TPR;
    const int col = t.mtile * BM + cv * 8;
    a_on[j] = cv < MV;
    a_off[j] = (a_on[j] && col < p.cout) ? (unsigned)(i_row * p.cout + col) * (unsigned)SP_BYTES : 0x80000000u;
  }
  WgradColumn i_col[B_CPT];
  bool b_on[B_CPT];
#pragma unroll
  for (int j = 0; j < B_CPT; ++j) {
    const int cv = i_v0 + j * A_TPR;
    b_on[j] = cv < NVB;
    i_col[j] = wgrad_column(p, t.ntile * BN + cv * 8, (unsigned)SP_BYTES, p.pad_w);
    i_col[j].cok &= b_on[j];
  }
  const unsigned row_bytes = (unsigned)(p.stride * p.w * p.cin) * (unsigned)SP_BYTES, col_bytes = (unsigned)(p.stride_w * p.cin) * (unsigned)SP_BYTES;
  const unsigned img_bytes = (unsigned)x_img_elems * (unsigned)SP_BYTES;
  WgradPixel s_px = {0, 0, 0u};
  if (INCR) s_px.decode(p, t.rem0 + (unsigned)i_row, img_bytes);
  u32x4 a_reg[A_CPT][SP_NP], b_reg[B_CPT][SP_NP];
  auto load_tiles = [&](int kt) {
#pragma unroll
    for (int j = 0; j < A_CPT; ++j) {
#pragma unroll
      for (int pc = 0; pc < SP_NP; ++pc)             // rows >= m_count: beyond the descriptor = zeros
        a_reg[j][pc] = __builtin_amdgcn_raw_buffer_load_b128(rs_a, a_off[j] + 16u * pc, 0, 0);
      a_off[j] += (unsigned)(BK * p.cout) * (unsigned)SP_BYTES;
    }
    const bool mok = kt * BK + i_row < t.m_count;
    WgradPixel px = s_px;
    if constexpr (!INCR) px.decode(p, t.rem0 + (unsigned)(kt * BK + i_row), img_bytes);
    const int iy0 = px.oy * p.stride, ix0 = px.ox * p.stride_w;
    const unsigned pixoff = px.imgoff + (unsigned)px.oy * row_bytes + (unsigned)px.ox * col_bytes;
#pragma unroll
    for (int j = 0; j < B_CPT; ++j) {
      const WgradColumn &c = i_col[j];
      const bool ok = mok & c.cok & ((unsigned)(iy0 + c.dy) < (unsigned)p.h) & ((unsigned)(ix0 + c.dx) < (unsigned)p.w);
#pragma unroll
      for (int pc = 0; pc < SP_NP; ++pc)
        b_reg[j][pc] = __builtin_amdgcn_raw_buffer_load_b128(rs_b, pred_off(pixoff + c.tconst + 16u * pc, ok), 0, 0);
    }
    if constexpr (INCR) s_px.template advance<BK>(p, img_bytes);
  };
  auto store_tiles = [&](int buf) {
    unsigned short *As = smem + buf * STAGE;
    unsigned short *Bs = As + SP_NP * A_ELEMS;
#pragma unroll
    for (int j = 0; j < A_CPT; ++j)
      if (a_on[j]) {
#pragma unroll
        for (int pc = 0; pc < SP_NP; ++pc)
          *reinterpret_cast<u32x4 *>(As + pc * A_ELEMS + i_row * LDA + (i_v0 + j * A_TPR) * 8) = a_reg[j][pc];
      }
#pragma unroll
    for (int j = 0; j < B_CPT; ++j)
      if (b_on[j]) {
#pragma unroll
        for (int pc = 0; pc < SP_NP; ++pc)
          *reinterpret_cast<u32x4 *>(Bs + pc * B_ELEMS + i_row * LDB + (i_v0 + j * A_TPR) * 8) = b_reg[j][pc];
      }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int KT = (t.m_count + BK - 1) / BK;
  load_tiles(0);
  store_tiles(0);
  load_tiles(1);
  __syncthreads();
  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt & 1;
    store_tiles(cur ^ 1);
    load_tiles(kt + 2);
    const unsigned short *As = smem + cur * STAGE;
    const unsigned short *Bs = As + SP_NP * A_ELEMS;
    f16x8 av[SP_NP][TM], bv[SP_NP][TN];
#pragma unroll
    for (int pc = 0; pc < SP_NP; ++pc) {
#pragma unroll
      for (int i = 0; i < TM; ++i) av[pc][i] = __builtin_bit_cast(f16x8, tr_frag(As + pc * A_ELEMS, LDA, 0, wm * WTM + i * 32, lane));
#pragma unroll
      for (int j = 0; j < TN; ++j) bv[pc][j] = __builtin_bit_cast(f16x8, tr_frag(Bs + pc * B_ELEMS, LDB, 0, wn * WTN + j * 32, lane));
    }
    SPLIT_PRODUCTS(av, bv, acc)
    __syncthreads();
  }

  const float osc = (p.dy_sinv ? *p.dy_sinv : 1.f) * (p.x_sinv ? *p.x_sinv : 1.f);
  wgrad_store_acc(p, acc, p.out + (long long)t.split * p.cout * p.ncols, t.mtile * BM + wm * WTM, t.ntile * BN + wn * WTN, li, lh, osc);
}

// The slab sums of SEVERAL weight gradients in one launch (a residual block's 3-4 convs: round 3 ran one 10 us reduce
// launch behind every wgrad launch, 63 per ResNet-50 step): wgrad_reduce_kernel's sum (wgrad_slab_sum) per item.
struct ReduceBatch {
  ReduceItem it[8];
  int n;
};
__global__ __launch_bounds__(256) void wgrad_reduce_batch_kernel(ReduceBatch b) {
  __shared__ float4 sh[256];
  int k = 0;
  for (int i = 1; i < b.n; ++i) k += (int)blockIdx.x >= b.it[i].block0;
  wgrad_slab_sum(sh, b.it[k]);
}

// The stem's row-window operand (see mvg_stem_fprop_split): one thread per 8-value chunk = image columns (2 ox - 4 + 2 q,
// + 1) x 4 stored channels of window (n, y, ox), written as the chunk's two fp16 pieces.
__global__ __launch_bounds__(256) void stem_rowwindow_kernel(const float4 *__restrict__ x, uint4 *__restrict__ xw, long long n, int h, int w) {
  const int wo = w >> 1;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int q = (int)(i & 3);
    const long long t = i >> 2;
    const int ox = (int)(t % wo);
    const long long row = t / wo;                     // image * h + y
    const int c0 = 2 * ox - 4 + 2 * q;                // even: both columns in range or both out (w is even)
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c0 >= 0 && c0 < w) {
      const float4 a = x[row * w + c0], b = x[row * w + c0 + 1];
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    uint4 q1, q2;
    split2_chunk(v, q1, q2);
    xw[SP_NP * i] = q1;
    xw[SP_NP * i + 1] = q2;
  }
}

// ... and straight from the module's NCHW fp32 input (3 planes), skipping the NHWC4 image
__global__ __launch_bounds__(256) void stem_rowwindow_nchw_kernel(const float *__restrict__ x, uint4 *__restrict__ xw, long long n, int h, int w) {
  const int wo = w >> 1;
  const long long plane = (long long)h * w;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int q = (int)(i & 3);
    const long long t = i >> 2;
    const int ox = (int)(t % wo);
    const long long row = t / wo;                     // image * h + y
    const long long img = row / h;
    const int yy = (int)(row - img * h);
    const int c0 = 2 * ox - 4 + 2 * q;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c0 >= 0 && c0 < w) {
      const float *src = x + img * 3 * plane + (long long)yy * w + c0;
      const float2 r = *reinterpret_cast<const float2 *>(src), g = *reinterpret_cast<const float2 *>(src + plane),
                   b = *reinterpret_cast<const float2 *>(src + 2 * plane);
      v[0] = r.x; v[1] = g.x; v[2] = b.x; v[4] = r.y; v[5] = g.y; v[6] = b.y;
    }
    uint4 q1, q2;
    split2_chunk(v, q1, q2);
    xw[SP_NP * i] = q1;
    xw[SP_NP * i + 1] = q2;
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static int validate_split(const mvg_conv_desc *d) {
  if (validate(d)) return 2;
  MVG_REQUIRE(d->cin % 32 == 0 && d->cout % 32 == 0, "split conv: cin and cout must be multiples of 32 (got %d, %d)", d->cin,
              d->cout);
  MVG_REQUIRE(d->r * d->s <= 32, "split conv: at most 32 filter taps");
  return 0;
}

// Row-tile height of a launch: 256 x 64 tiles when the GEMM has fewer than 128 columns, more than one tap (the 64-channel 3x3
// convs: K = 576; the 1x1 layers with 64 columns are HBM-bound either way) and enough rows to fill the chip with the larger
// tiles.  A function of the descriptor alone: mvg_conv_dgrad_bn_partials_split sizes the fused reduce's partials with it.
static int split_tile_rows(int ncols, int taps, long long rows) { return (ncols < 128 && taps > 1 && rows >= 65536) ? 256 : SP_BM; }

// The tiling of an igemm_split16_kernel launch and the K loop it gets: a function of (columns, taps, rows of the whole map, groups,
// each class's rows per group and K, lin) - launch_igemm_split launches by it, mvg_conv_fprop_split_stages and
// mvg_conv_dgrad_split_stages answer from it.  Writes every class's mtiles_per_group, KT and tile0.  (256-row tiles come with 64
// columns and never with lin: by construction.)
struct SplitPlan { int bm, bn, kt_max; long long tiles; bool pipelined; };
// K-loop stages of a conv's DMA-loader launch under a plan: the two-stage pipeline exists for 128 x 128 tiles only
static int split_conv_stages(const SplitPlan &pl) { return (pl.pipelined && pl.bn == 128 && pl.bm == SP_BM) ? 2 : 1; }
static SplitPlan split_plan(int ncols, int taps, long long rows, int groups, bool lin, IgemmClass *cls, int ncls) {
  SplitPlan pl;
  pl.bm = lin ? SP_BM : split_tile_rows(ncols, taps, rows);
  // (128 x 64 tiles for the short-K, write-heavy 1x1 layers - 64 -> 256 at 56 x 56 and the like - were measured in round 4:
  // within 2 % of 128 x 128 on every such shape, forward and backward-data)
  pl.bn = ncols >= 128 ? 128 : 64;
  if (lin && pl.bn == 128 && ncls == 1) {
    // a Linear whose 128 x 128 tiles would leave most CUs idle (C3's head layer: 48 tiles; C4's per-GPU share: 12 - 84):
    // a lone workgroup takes in ~41 GB/s, so the launch is as fast as its busiest CU's operand bytes - 128 x 64 tiles
    // (24 KB instead of 32 KB per K-step) on twice the CUs
    const long long t128 = (long long)groups * ceil_div(cls[0].rows_per_group, pl.bm) * ceil_div(ncols, 128);
    if (2 * t128 <= compute_cus()) pl.bn = 64;
  }
  pl.tiles = 0, pl.kt_max = 0;
  for (int i = 0; i < ncls; ++i) {
    IgemmClass &c = cls[i];
    c.mtiles_per_group = ceil_div(c.rows_per_group, pl.bm);
    c.KT = ceil_div(c.ktotal, SP_BK);              // 0: a class without taps (fused reduce only) - its tiles are epilogue only
    c.tile0 = (int)pl.tiles;
    pl.tiles += (long long)groups * c.mtiles_per_group * ceil_div(ncols, pl.bn);
    pl.kt_max = c.KT > pl.kt_max ? c.KT : pl.kt_max;
  }
  // At most two workgroups per CU: nobody covers a workgroup's waits - the two-stage software pipeline.  Measured per shape
  // (scripts/linear_split_bench.py, C3's fusion rows: fprop 431 -> 320 us per iteration, dgrad 246 -> 210;
  // scripts/conv_bench.py 50 32 4, C4's per-GPU share: 15.2 -> 14.6 ms over the net, 512-channel 3x3 at 7x7 0.169 -> 0.127 ms;
  // C3's conv launches all have >= 784 tiles).  Three and four stages - one workgroup per CU - and an L2-blocked tile order
  // changed nothing: a lone workgroup takes in ~41 GB/s whatever it keeps in flight.
  // Up to four per CU it still wins where the K loop is long (ResNet-50's 7x7 stage at C3, 784 tiles: 512-channel 3x3
  // backward-data + reduce 0.399 -> 0.322 ms, 2048 <- 512 backward-data 0.218 -> 0.185); with every slot filled the
  // single-stage loop at four workgroups per CU is faster (17.4 vs 19.5 ms over the forward net).
  pl.pipelined = pl.tiles <= 2LL * compute_cus() || (pl.tiles <= 4LL * compute_cus() && pl.kt_max >= 48);
  return pl;
}

// taps, rows: the filter's taps and the rows of the whole map (the row-tile height's arguments); af: the loader forms the A operand
template <bool DGRAD>
static int launch_igemm_split(IgemmParams &p, hipStream_t st, bool lin, int taps, long long rows, AForm af = A_DMA, bool ranged = false) {
  const SplitPlan pl = split_plan(p.ncols, taps, rows, p.groups, lin, p.cls, p.ncls);
  const int bm = pl.bm, bn = pl.bn;
  const bool pipelined = pl.pipelined;
  p.ntiles = ceil_div(p.ncols, bn);
  p.splits = 1;
  p.sk_tiles = 0;
  p.bn_parts = 0;
  for (int i = 0; i < p.ncls; ++i) {
    IgemmClass &c = p.cls[i];
    c.korder = c.ntaps > 1 ? 1 : 0;
    c.per_div = make_fastdiv((unsigned)(c.ntaps > 0 ? c.ntaps : 1));
    c.unit0 = 0;
    c.part0 = p.bn_parts;
    p.bn_parts += c.mtiles_per_group;
    MVG_REQUIRE((c.ntaps >= 1 || (DGRAD && p.bn_part)) && c.ntaps <= 32 && c.ktotal % SP_BK == 0, "split conv: class shape not covered");
  }
  MVG_REQUIRE(pl.tiles < (1LL << 31), "split conv: grid too large");
  if (pl.tiles <= 0) return 0;
  // The backbone's fp32 results (y, dx: 0.2 - 1.7 GB per launch, next read by a BatchNorm pass that streams them once) leave
  // with non-temporal stores: C3 81.4 -> 80.9 ms per step on one box (the passes that follow find more of their other
  // operand in the Infinity Cache: bn_apply 8.8 -> 8.4 ms).  Not the stride-2 parity classes - they write every other pixel,
  // which wants the cache to merge lines (0.96 -> 1.01 ms on 256 -> 512 at 56 x 56) - and not the fusion block's Linears,
  // whose results are re-read at once.
  p.nt_out = (!lin && !(DGRAD && p.cls_step == 2)) ? 1 : 0;
  dim3 grid((unsigned)pl.tiles), block(256);
  if (af != A_DMA) {         // the A operand formed in the loader (tiles, K order, epilogue - the fused reduce's partials - as the DMA kernels)
    MVG_REQUIRE(!lin && bm == SP_BM && p.ntiles == 1 && p.ncls == 1 && DGRAD == (af == A_DY), "split conv: the operand-forming loaders take one column tile");
    if constexpr (DGRAD) {
      if (bn == 128) hipLaunchKernelGGL((igemm_split16_kernel<128, true, false, 2, 1, A_DY>), grid, block, 0, st, p);
      else hipLaunchKernelGGL((igemm_split16_kernel<64, true, false, 2, 1, A_DY>), grid, block, 0, st, p);
      return check_launch("conv_dgrad_split_bnapply");
    } else {
      if (bn == 128 && af == A_OUT_AFFINE) hipLaunchKernelGGL((igemm_split16_kernel<128, false, false, 2, 1, A_OUT_AFFINE>), grid, block, 0, st, p);
      else if (bn == 128) hipLaunchKernelGGL((igemm_split16_kernel<128, false, false, 2, 1, A_OUT_SP>), grid, block, 0, st, p);
      else if (af == A_OUT_AFFINE) hipLaunchKernelGGL((igemm_split16_kernel<64, false, false, 2, 1, A_OUT_AFFINE>), grid, block, 0, st, p);
      else hipLaunchKernelGGL((igemm_split16_kernel<64, false, false, 2, 1, A_OUT_SP>), grid, block, 0, st, p);
      return check_launch("conv_fprop_split_bnapply");
    }
  }
  if (ranged) {              // the guarded inference forward: the plain forward's four forms with the range record in the epilogue
    MVG_REQUIRE(!DGRAD && !lin && p.out_sp && p.out_absmax, "split conv: the range record goes with a forward that stores sp");
    if constexpr (!DGRAD) {
      if (bm == 256) hipLaunchKernelGGL((igemm_split16_ranged_kernel<64, 4>), grid, block, 0, st, p);
      else if (split_conv_stages(pl) == 2) hipLaunchKernelGGL((igemm_split16_ranged_kernel<128, 2, 2>), grid, block, 0, st, p);
      else if (bn == 128) hipLaunchKernelGGL((igemm_split16_ranged_kernel<128>), grid, block, 0, st, p);
      else hipLaunchKernelGGL((igemm_split16_ranged_kernel<64>), grid, block, 0, st, p);
    }
    return check_launch("conv_fprop_split_ranged");
  }
  if (lin) {                 // a Linear of the fusion block: the epilogue's scale / abs-max features compiled in
    if (bn == 128 && pipelined) hipLaunchKernelGGL((igemm_split16_kernel<128, DGRAD, true, 2, 2>), grid, block, 0, st, p);
    else if (bn == 128) hipLaunchKernelGGL((igemm_split16_kernel<128, DGRAD, true>), grid, block, 0, st, p);
    else if (pipelined) hipLaunchKernelGGL((igemm_split16_kernel<64, DGRAD, true, 2, 2>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((igemm_split16_kernel<64, DGRAD, true>), grid, block, 0, st, p);
  } else if (bm == 256) hipLaunchKernelGGL((igemm_split16_kernel<64, DGRAD, false, 4>), grid, block, 0, st, p);
  else if (split_conv_stages(pl) == 2) hipLaunchKernelGGL((igemm_split16_kernel<128, DGRAD, false, 2, 2>), grid, block, 0, st, p);
  else if (bn == 128) hipLaunchKernelGGL((igemm_split16_kernel<128, DGRAD>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((igemm_split16_kernel<64, DGRAD>), grid, block, 0, st, p);
  return check_launch(DGRAD ? "conv_dgrad_split" : "conv_fprop_split");
}

}  // namespace mvg

using namespace mvg;

extern "C" {

int mvg_split_f32(const float *x, void *out_sp, int64_t n, float scale, void *stream) {
  MVG_REQUIRE(x && out_sp && n >= 0 && n % 8 == 0, "split_f32: null argument or n %% 8 != 0");
  MVG_REQUIRE(scale > 0.f, "split_f32: scale must be positive (a power of two keeps the round trip exact)");
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, (4.0 + SP_BYTES) * (double)n);
  long long blocks = (n / 8 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(split_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float4 *)x, (uint4 *)out_sp, (long long)(n / 8), scale);
  return check_launch("split_f32");
}

int mvg_split_f32_ranged(const float *x, void *out_sp, int64_t n, float scale, uint32_t *range_word, void *stream) {
  MVG_REQUIRE(x && out_sp && range_word && n >= 0 && n % 8 == 0, "split_f32_ranged: null argument or n %% 8 != 0");
  MVG_REQUIRE(scale > 0.f, "split_f32_ranged: scale must be positive (a power of two keeps the round trip exact)");
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, (4.0 + SP_BYTES) * (double)n);
  long long blocks = (n / 8 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(split_f32_ranged_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float4 *)x, (uint4 *)out_sp, (long long)(n / 8), scale,
                     (unsigned *)range_word);
  return check_launch("split_f32_ranged");
}

int mvg_merge_sp(const void *x_sp, float *out, int64_t n, float inv_scale, void *stream) {
  MVG_REQUIRE(x_sp && out && n >= 0 && n % 8 == 0, "merge_sp: null argument or n %% 8 != 0");
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, (4.0 + SP_BYTES) * (double)n);
  long long blocks = (n / 8 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(merge_sp_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const uint4 *)x_sp, (float4 *)out, (long long)(n / 8), inv_scale);
  return check_launch("merge_sp");
}

int mvg_split_weights(const mvg_conv_desc *d, const float *w, void *w_krsc_sp, void *w_crsk_sp, float *stat2, void *items_dev,
                      void *stream) {
  // one conv through the batched kernels: items_dev = 64 bytes of device memory for the one-record table, stat2 =
  // two device floats that receive {max |w| bits, 2^-k} (the consumer's b_sinv = stat2 + 1)
  MVG_REQUIRE(d && w && w_krsc_sp && stat2 && items_dev, "split_weights: null argument");
  if (validate_split(d)) return 2;
  hipStream_t st = (hipStream_t)stream;
  WPrepItem it;
  memset(&it, 0, sizeof(it));
  it.w = w;
  it.wk = w_krsc_sp;
  it.wt = w_crsk_sp;
  it.cout = d->cout;
  it.rs = d->r * d->s;
  it.cin = d->cin;
  it.cin_pad = d->cin;
  it.stat = stat2;
  static_assert(sizeof(WPrepItem) <= 64, "WPrepItem grew: update the callers' table record size");
  // the record travels as a kernel argument (captured at launch): an asynchronous copy from this stack frame could be read after
  // the frame is gone when the stream is busy
  hipLaunchKernelGGL(wprep_stage_item_kernel, dim3(1), dim3(64), 0, st, it, (WPrepItem *)items_dev);
  if (check_launch("split_weights: staging the table record")) return 1;
  const long long n8 = (long long)d->cout * it.rs * d->cin / 8;
  long long blocks = (n8 + 256 * 8 - 1) / (256 * 8);             // ~8 chunks per thread
  return mvg_weights_prep_batch(items_dev, 1, 1, (int)(blocks < 16 ? 16 : (blocks > 2048 ? 2048 : blocks)), stream);
}

int mvg_weights_prep_batch(const void *items_dev, int n, int mode, int blocks_per_item, void *stream) {
  MVG_REQUIRE(items_dev != nullptr && n > 0 && (mode == 0 || mode == 1) && blocks_per_item >= 0 && blocks_per_item <= 4096,
              "weights_prep_batch: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, 0.0);
  // workgroups per record: 64 suits the backbone's convs (53 records, <= 2.4 M weights each); the fusion block's Linears
  // (9 records of up to 12.8 M weights) want a few hundred
  const unsigned bx = blocks_per_item > 0 ? (unsigned)blocks_per_item : 64u;
  if (mode == 1) {           // max |w| per conv first (the records' stat[0] must be zero: the caller clears them)
    hipLaunchKernelGGL(weights_absmax_kernel, dim3(bx > 64 ? bx / 2 : 16, (unsigned)n), dim3(256), 0, st, (const WPrepItem *)items_dev);
    if (check_launch("weights_absmax")) return 1;
  }
  hipLaunchKernelGGL(weights_prep_batch_kernel, dim3(bx, (unsigned)n), dim3(256), 0, st, (const WPrepItem *)items_dev, mode);
  return check_launch("weights_prep_batch");
}

int mvg_conv_stats_partials_split(const mvg_conv_desc *d, int32_t *rows_per_partial) {
  if (validate_split(d)) return -1;
  const long long rows = (long long)d->n * d->ho * d->wo;
  if (rows_per_partial) *rows_per_partial = 64;               // one wave tile of rows
  // two partials per 128-row tile (the last tile's second one may lie beyond the rows: count 0, ignored by bn_finalize)
  return ceil_div(rows, SP_BM) * 2;
}

struct SplitAffine {       // inference forward: y = acc * scale + shift (+ residual) [relu], result fp32 or sp
  const float *scale, *shift;
  const void *residual;
  int residual_sp, relu, out_sp;
  // Linear layers of the fusion block (LIN kernels): see IgemmParams::out_absmax / out_sinv / bias_absmax
  int lin;
  float *out_absmax, *out_sinv;
  const float *bias_absmax;
  uint32_t *range_word;    // the guarded inference forward's record of this launch's sp output (travels as IgemmParams::out_absmax)
};

// stride_w / pad_w >= 0: the horizontal stride / padding differ from d->stride / d->pad (the stem's row-window form, whose
// descriptor the caller has checked itself)
struct SplitFwdApply {     // the launch forms its own input (IgemmParams::fap_*): the previous block's BatchNorm apply pass
  const float *y, *scale, *shift, *res_scale, *res_shift, *res_sinv;
  const void *res;
  uint8_t *bits;
};

static int fprop_split_impl(const mvg_conv_desc *d, const void *x_sp, const float *x_sinv, const void *w_sp, const float *w_sinv,
                            void *y, float *stats, void *stream, const SplitAffine *aff, int stride_w = -1, int pad_w = -1,
                            const SplitFwdApply *fap = nullptr) {
  if (stride_w < 0 && validate_split(d)) return 2;
  IgemmParams p;
  memset(&p, 0, sizeof(p));
  p.a = (const float *)x_sp;
  p.b = (const float *)w_sp;
  p.a_sinv = x_sinv;
  p.b_sinv = w_sinv;
  p.out = (float *)y;
  p.stats = stats;
  if (aff) {
    p.scale = aff->scale;
    p.bias = aff->shift;
    p.addend = (const float *)aff->residual;
    p.addend_sp = aff->residual_sp;
    p.relu = aff->relu;
    p.out_sp = aff->out_sp;
    p.out_absmax = aff->range_word ? (unsigned *)aff->range_word : (unsigned *)aff->out_absmax;
    p.out_sinv = aff->out_sinv;
    p.bias_absmax = aff->bias_absmax;
  }
  if (fap) {
    p.fap_y = fap->y;
    p.fap_scale = fap->scale;
    p.fap_shift = fap->shift;
    p.fap_res = fap->res;
    p.fap_res_scale = fap->res_scale;
    p.fap_res_shift = fap->res_shift;
    p.fap_res_sinv = fap->res_sinv;
    p.fap_bits = (unsigned short *)fap->bits;
  }
  if (fprop_geometry(p, d, SP_BYTES, SP_BYTES, "split conv", stride_w, pad_w)) return 2;
  MVG_REQUIRE(p.rows_per_group * (long long)d->cout < (1ll << 31), "split conv: a group of the output exceeds 2^31 elements");
  // (the stem's row-window form multiplies 7 x 32 values per output where the filter has 7 x 7 x 3: count the filter's)
  const double flops = 2.0 * d->groups * (double)p.rows_per_group * d->cout * d->r * d->s * d->cin * (stride_w >= 0 ? 147.0 / 224.0 : 1.0);
  // (with the apply pass on board the launch reads y and the residual and writes the input instead of reading it: its algorithmic bytes)
  const double bytes = (double)SP_BYTES * (d->groups * (double)d->n * d->h * d->w * d->cin + (double)d->cout * d->r * d->s * d->cin) +
                       4.0 * d->groups * (double)p.rows_per_group * d->cout +
                       (fap ? 8.0 + 1.0 / 4.0 : 0.0) * d->groups * (double)d->n * d->h * d->w * d->cin;
  const bool lin = d->r == 1 && d->s == 1 && d->h == 1 && d->w == 1;
  ProfScope ps(lin ? MVG_K_LINEAR_FPROP : MVG_K_CONV_FPROP, (hipStream_t)stream, flops, bytes);
  p.stats_partials = ceil_div(p.rows_per_group, SP_BM) * 2;    // = mvg_conv_stats_partials_split
  return launch_igemm_split<false>(p, (hipStream_t)stream, aff && aff->lin, d->r * d->s, p.rows_per_group,
                                   fap ? (fap->res_scale ? A_OUT_AFFINE : A_OUT_SP) : A_DMA, aff && aff->range_word);
}

int mvg_conv_fprop_split(const mvg_conv_desc *d, const void *x_sp, const float *x_sinv, const void *w_sp, const float *w_sinv, float *y,
                         float *stats, void *stream) {
  return fprop_split_impl(d, x_sp, x_sinv, w_sp, w_sinv, y, stats, stream, nullptr);
}

int mvg_conv_fprop_split_stages(const mvg_conv_desc *d) {
  // 1 / 2: the K loop launch_igemm_split picks for this forward (single-stage / the two-stage pipeline); -1: bad descriptor.
  // (mvg_conv_fprop_split_bnapply exists in the single-stage form only: the caller's eligibility rule asks here.)
  if (validate_split(d)) return -1;
  IgemmClass c;
  memset(&c, 0, sizeof(c));
  c.rows_per_group = (long long)d->n * d->ho * d->wo;
  c.ktotal = d->r * d->s * d->cin;
  const SplitPlan pl = split_plan(d->cout, d->r * d->s, c.rows_per_group, d->groups, false, &c, 1);
  return split_conv_stages(pl);
}

int mvg_conv_fprop_split_bnapply(const mvg_conv_desc *d, void *out_sp, const float *out_sinv, const float *bn_y, const float *scale,
                                 const float *shift, const void *residual, int residual_sp, const float *res_scale,
                                 const float *res_shift, const float *res_sinv, uint8_t *relu_bits, const void *w_sp,
                                 const float *w_sinv, float *y, float *stats, void *stream) {
  // mvg_bn_apply_split_scaled (residual + ReLU) of the unit that PRODUCES this conv's input, and mvg_conv_fprop_split, in ONE
  // launch: out_sp (an output: the conv's input, written once in sp times 1 / *out_sinv) = relu(bn_y * scale + shift + residual),
  // the residual an sp identity (read times *res_sinv) or the raw fp32 downsample output with (res_scale, res_shift);
  // relu_bits (optional) receives the mask as mvg_bn_apply_split_scaled writes it.  Same bits as the two launches.
  MVG_REQUIRE(d && out_sp && bn_y && scale && shift && residual && w_sp && y, "fprop_split_bnapply: null argument");
  MVG_REQUIRE(d->r == 1 && d->s == 1 && d->stride == 1 && d->pad == 0, "fprop_split_bnapply: 1x1, stride 1, pad 0 only");
  MVG_REQUIRE(d->cout == 64 || d->cout == 128, "fprop_split_bnapply: cout must be 64 or 128 (one column tile; got %d)", d->cout);
  MVG_REQUIRE(d->cin % 32 == 0 && d->cin <= BNA_MAX_C, "fprop_split_bnapply: cin must be a multiple of 32, at most %d (got %d)", BNA_MAX_C,
              d->cin);
  MVG_REQUIRE(residual_sp ? (!res_scale && !res_shift) : (res_scale && res_shift && !res_sinv),
              "fprop_split_bnapply: the residual is an sp identity (no res_scale / res_shift) or fp32 with res_scale and res_shift");
  MVG_REQUIRE((long long)d->n * d->h * d->w * d->cin < (1ll << 29), "fprop_split_bnapply: a group of the input exceeds 2 GiB");
  const SplitFwdApply a = {bn_y, scale, shift, res_scale, res_shift, res_sinv, residual, relu_bits};
  return fprop_split_impl(d, out_sp, out_sinv, w_sp, w_sinv, y, stats, stream, nullptr, -1, -1, &a);
}

int mvg_conv_fprop_split_affine(const mvg_conv_desc *d, const void *x_sp, const float *x_sinv, const void *w_sp, const float *w_sinv,
                                void *out, int out_sp, const float *scale, const float *shift, const void *residual, int residual_sp,
                                int relu, void *stream) {
  MVG_REQUIRE(scale && shift && out, "fprop_split_affine: scale, shift and out are required");
  const SplitAffine a = {scale, shift, residual, residual_sp, relu, out_sp, 0, nullptr, nullptr, nullptr, nullptr};
  return fprop_split_impl(d, x_sp, x_sinv, w_sp, w_sinv, out, nullptr, stream, &a);
}

int mvg_conv_fprop_split_affine_ranged(const mvg_conv_desc *d, const void *x_sp, const float *x_sinv, const void *w_sp, const float *w_sinv,
                                       void *out, int out_sp, const float *scale, const float *shift, const void *residual,
                                       int residual_sp, int relu, uint32_t *range_word, void *stream) {
  MVG_REQUIRE(scale && shift && out, "fprop_split_affine_ranged: scale, shift and out are required");
  MVG_REQUIRE(range_word && out_sp, "fprop_split_affine_ranged: range_word is required and the output must be sp (out_sp != 0)");
  const SplitAffine a = {scale, shift, residual, residual_sp, relu, out_sp, 0, nullptr, nullptr, nullptr, range_word};
  return fprop_split_impl(d, x_sp, x_sinv, w_sp, w_sinv, out, nullptr, stream, &a);
}

struct SplitBnFuse {       // fused BatchNorm-backward reduce of the unit whose output gradient dx is (IgemmParams::bn_*)
  const float *y;
  const uint8_t *bits;
  const float *mean, *invstd, *rscale, *rshift;
  float *part;
  int part_rows;
};

struct SplitBnApply {      // the launch forms its own dy (IgemmParams::bna_*): the unit's BatchNorm-backward apply pass
  const float *dz, *y, *mean, *invstd, *gamma, *s1, *s2;
  long long rows_per_group;
};

static int dgrad_split_impl(const mvg_conv_desc *d, const void *dy_sp, const float *dy_sinv, const void *w_crsk_sp, const float *w_sinv,
                            float *dx, const float *addend, void *stream, const SplitBnFuse *bnf, const void *relu_mask_sp = nullptr,
                            bool lin_kernel = false, float *out_absmax = nullptr, const SplitBnApply *bna = nullptr) {
  if (validate_split(d)) return 2;
  IgemmParams p;
  memset(&p, 0, sizeof(p));
  p.a = (const float *)dy_sp;
  p.b = (const float *)w_crsk_sp;
  p.a_sinv = dy_sinv;
  p.b_sinv = w_sinv;
  p.out = dx;
  p.addend = addend;
  p.mask = (const float *)relu_mask_sp;
  p.mask_sp = relu_mask_sp != nullptr;
  p.out_absmax = (unsigned *)out_absmax;
  if (bnf) {
    p.bn_y = bnf->y;
    p.bn_bits = bnf->bits;
    p.bn_mean = bnf->mean;
    p.bn_invstd = bnf->invstd;
    p.bn_rscale = bnf->rscale;
    p.bn_rshift = bnf->rshift;
    p.bn_part = bnf->part;
    p.bn_part_rows = bnf->part_rows;
  }
  if (bna) {
    p.bna_dz = bna->dz;
    p.bna_y = bna->y;
    p.bna_mean = bna->mean;
    p.bna_invstd = bna->invstd;
    p.bna_gamma = bna->gamma;
    p.bna_s1 = bna->s1;
    p.bna_s2 = bna->s2;
    p.bna_inv_rows = 1.0f / (float)bna->rows_per_group;       // mvg_bn_bwd_apply_split's
  }
  if (dgrad_geometry(p, d, SP_BYTES, SP_BYTES, "split conv")) return 2;
  MVG_REQUIRE((long long)d->n * d->h * d->w * d->cin < (1ll << 31), "split conv: a group of dx exceeds 2^31 elements");
  const double flops = 2.0 * d->groups * (double)d->n * d->ho * d->wo * d->cout * d->r * d->s * d->cin;
  // (with the BatchNorm reduce on board the launch also reads that unit's y and mask bits: its algorithmic bytes)
  const double bytes = (double)SP_BYTES * (d->groups * (double)d->n * d->ho * d->wo * d->cout + (double)d->cout * d->r * d->s * d->cin) +
                       (bnf ? 8.25 : 4.0) * d->groups * (double)d->n * d->h * d->w * d->cin +
                       (bna ? 8.0 : 0.0) * d->groups * (double)d->n * d->ho * d->wo * d->cout;       // dz and y read, dy written not read
  const bool lin = d->r == 1 && d->s == 1 && d->h == 1 && d->w == 1;
  ProfScope ps(lin ? MVG_K_LINEAR_DGRAD : MVG_K_CONV_DGRAD, (hipStream_t)stream, flops, bytes);
  if (int e = dgrad_classes(p, d, bnf != nullptr, 4, dx, addend, (hipStream_t)stream)) return e;
  if (p.ncls == 0) return 0;
  return launch_igemm_split<true>(p, (hipStream_t)stream, lin_kernel, d->r * d->s, (long long)d->n * d->h * d->w, bna ? A_DY : A_DMA);
}

int mvg_conv_dgrad_split(const mvg_conv_desc *d, const void *dy_sp, const float *dy_sinv, const void *w_crsk_sp, const float *w_sinv,
                         float *dx, const float *addend, const void *relu_mask_sp, void *stream) {
  MVG_REQUIRE(!relu_mask_sp || d->stride == 1, "dgrad_split: the sp ReLU mask is for stride-1 launches (Linear layers)");
  return dgrad_split_impl(d, dy_sp, dy_sinv, w_crsk_sp, w_sinv, dx, addend, stream, nullptr, relu_mask_sp);
}

int mvg_conv_dgrad_split_stages(const mvg_conv_desc *d, int fused_reduce) {
  // 1 / 2: the K loop launch_igemm_split picks for this backward-data (mvg_conv_dgrad_split; fused_reduce != 0:
  // mvg_conv_dgrad_split_bnreduce, whose launch keeps the parity classes without taps); -1: bad descriptor.  Launches nothing.
  if (validate_split(d)) return -1;
  IgemmParams p;
  memset(&p, 0, sizeof(p));
  if (dgrad_geometry(p, d, SP_BYTES, SP_BYTES, "split conv")) return -1;
  DgradDropped dropped;
  dgrad_plan_classes(p, d, fused_reduce != 0, dropped);
  return split_conv_stages(split_plan(p.ncols, d->r * d->s, (long long)d->n * d->h * d->w, p.groups, false, p.cls, p.ncls));
}

int mvg_conv_dgrad_bn_partials_split(const mvg_conv_desc *d) {
  if (validate_split(d)) return -1;
  return dgrad_bn_partials(d, split_tile_rows(d->cin, d->r * d->s, (long long)d->n * d->h * d->w));
}

// Backward-data with the BatchNorm-backward reduce pass of the unit it feeds on board, then that pass's finalize: the tail of both
// entries below (who: the entry's name in the messages; bna: the launch also forms its own dy)
static int dgrad_split_bnreduce_impl(const char *who, const mvg_conv_desc *d, const void *dy_sp, const float *dy_sinv, const void *w_crsk_sp,
                                     const float *w_sinv, float *dx, const float *addend, const float *bn_y, const uint8_t *bn_bits,
                                     const float *bn_mean, const float *bn_invstd, const float *relu_scale, const float *relu_shift,
                                     float *partials, float *s1, float *s2, float *dgamma, float *dbeta, int accumulate, float *mx,
                                     const float *bn_gamma, float *dx_dy_sinv, void *stream, const SplitBnApply *bna) {
  MVG_REQUIRE(bn_y && bn_mean && bn_invstd && partials && s1 && s2, "%s: null argument", who);
  MVG_REQUIRE((bn_gamma == nullptr) == (dx_dy_sinv == nullptr) && (!dx_dy_sinv || mx), "%s: bn_gamma, dx_dy_sinv (and mx) go together", who);
  MVG_REQUIRE(!(bn_bits && relu_scale) && ((relu_scale == nullptr) == (relu_shift == nullptr)),
              "%s: give the ReLU mask either as bits or as (relu_scale, relu_shift)", who);
  const int P = mvg_conv_dgrad_bn_partials_split(d);
  MVG_REQUIRE(P > 0, "%s: bad descriptor", who);
  const SplitBnFuse f = {bn_y, bn_bits, bn_mean, bn_invstd, relu_scale, relu_shift, partials, mx ? 3 : 2};
  if (dgrad_split_impl(d, dy_sp, dy_sinv, w_crsk_sp, w_sinv, dx, addend, stream, &f, nullptr, false, nullptr, bna)) return 1;
  ProfScope ps(MVG_K_BN_BWD_REDUCE, (hipStream_t)stream, 0.0, 8.0 * d->groups * (double)P * d->cin);
  return bn_bwd_finalize_launch(partials, d->groups, P, d->cin, s1, s2, dgamma, dbeta, accumulate, (hipStream_t)stream, mx, nullptr, nullptr,
                                bn_gamma, bn_invstd, (long long)d->n * d->h * d->w, dx_dy_sinv);
}

int mvg_conv_dgrad_split_bnreduce(const mvg_conv_desc *d, const void *dy_sp, const float *dy_sinv, const void *w_crsk_sp,
                                  const float *w_sinv, float *dx, const float *addend, const float *bn_y, const uint8_t *bn_bits,
                                  const float *bn_mean, const float *bn_invstd, const float *relu_scale, const float *relu_shift,
                                  float *partials, float *s1, float *s2, float *dgamma, float *dbeta, int accumulate,
                                  float *mx, const float *bn_gamma, float *dx_dy_sinv, void *stream) {
  // (dx_dy_sinv: receives the 2^-k of the dy that mvg_bn_bwd_apply_split will make from dx - the NEXT unit down the chain)
  return dgrad_split_bnreduce_impl("dgrad_split_bnreduce", d, dy_sp, dy_sinv, w_crsk_sp, w_sinv, dx, addend, bn_y, bn_bits, bn_mean, bn_invstd,
                                   relu_scale, relu_shift, partials, s1, s2, dgamma, dbeta, accumulate, mx, bn_gamma, dx_dy_sinv, stream, nullptr);
}

int mvg_conv_dgrad_split_bnapply_bnreduce(const mvg_conv_desc *d, void *dy_sp, const float *dy_sinv, const float *dz, const float *y,
                                          const float *mean, const float *invstd, const float *gamma, const float *un_s1,
                                          const float *un_s2, int64_t rows_per_group, const void *w_crsk_sp, const float *w_sinv,
                                          float *dx, const float *addend, const float *bn_y, const uint8_t *bn_bits,
                                          const float *bn_mean, const float *bn_invstd, const float *relu_scale,
                                          const float *relu_shift, float *partials, float *s1, float *s2, float *dgamma, float *dbeta,
                                          int accumulate, float *mx, const float *bn_gamma, float *dx_dy_sinv, void *stream) {
  MVG_REQUIRE(d && dy_sp && dz && y && mean && invstd && gamma && un_s1 && un_s2 && w_crsk_sp && dx,
              "dgrad_split_bnapply_bnreduce: null argument");
  MVG_REQUIRE(dy_sinv, "dgrad_split_bnapply_bnreduce: dy_sinv (the 2^-k the reduce pass left for this unit's dy) is required");
  MVG_REQUIRE(d->r == 1 && d->s == 1 && d->stride == 1 && d->pad == 0, "dgrad_split_bnapply_bnreduce: 1x1, stride 1, pad 0 only");
  MVG_REQUIRE(d->cin == 64 || d->cin == 128, "dgrad_split_bnapply_bnreduce: cin must be 64 or 128 (one column tile; got %d)", d->cin);
  MVG_REQUIRE(d->cout % 32 == 0 && d->cout <= BNA_MAX_C, "dgrad_split_bnapply_bnreduce: cout must be a multiple of 32, at most %d (got %d)",
              BNA_MAX_C, d->cout);
  MVG_REQUIRE(rows_per_group == (int64_t)d->n * d->ho * d->wo, "dgrad_split_bnapply_bnreduce: rows_per_group is not n * ho * wo");
  const SplitBnApply a = {dz, y, mean, invstd, gamma, un_s1, un_s2, (long long)rows_per_group};
  return dgrad_split_bnreduce_impl("dgrad_split_bnapply_bnreduce", d, dy_sp, dy_sinv, w_crsk_sp, w_sinv, dx, addend, bn_y, bn_bits, bn_mean,
                                   bn_invstd, relu_scale, relu_shift, partials, s1, s2, dgamma, dbeta, accumulate, mx, bn_gamma, dx_dy_sinv, stream, &a);
}

// The tile of a weight-gradient launch and its pixel addressing (incr: wgrad_split_kernel's incremental form, at most one image
// wrap per 16-pixel step): wgrad_split_impl dispatches by it, mvg_conv_wgrad_split_tile answers from it.
static void wgrad_split_tile(const mvg_conv_desc *d, int &bm, int &bn, bool &incr) {
  incr = (long long)d->ho * d->wo >= 32;
  const int ncols = d->r * d->s * d->cin;
  bm = d->cout >= 128 ? 128 : 64;
  bn = ncols >= 128 ? 128 : 64;
  // 128 x 256 tiles (wave tile 64 x 128, two workgroups per CU) where the columns divide: 24 KB of operands per 16-pixel K-step for
  // twice the products of the 128 x 128 tile's 16 KB - like every kernel of this family wgrad runs into the CU's operand intake,
  // not the matrix pipe (scripts/conv_bench.py at C3: 5 - 14 % per layer, e.g. 512-channel 3x3 stride 2 0.377 -> 0.326 ms;
  // inside the step the family 15.4 -> 14.7 ms, C3 79.2 -> 78.3 ms on one box)
  if (bm == 128 && ncols >= 256 && ncols % 256 == 0) bn = 256;
  // ... and 192-column tiles for the 64- and 128-channel 3x3 layers (576 / 1152 columns = 3 / 6 whole tiles where 128-column tiles
  // leave a half-empty last one): 64 -> 64 at 56 x 56 0.553 -> 0.477 ms, 128 -> 128 0.367 -> 0.349 (15.66 -> 15.38 ms over C3's net)
  else if (ncols % 192 == 0) bn = 192;
}

// The pixel splits of a checked descriptor (the stem's rewritten one included) at its tile.
static int wgrad_split_splits(const mvg_conv_desc *d) {
  int bm, bn;
  bool incr;
  wgrad_split_tile(d, bm, bn, incr);
  // one resident round: three workgroups per CU (128-column tiles; measured at C3: 2 / 3 / 4 / 6 per CU -> 17.8 / 16.8 / 16.7 /
  // 17.7 ms of wgrad per step), two with the 256-column tiles (2 / 3 / 4 / 6 -> 15.6 / 16.8 / 16.4 / 17.3 ms); 16 K-steps per split
  return wgrad_split_count(wgrad_tiles(d, bm, bn), (long long)d->groups * d->n * d->ho * d->wo, bn == 256 ? 2 : 3, 256);
}

int mvg_conv_wgrad_splits_split(const mvg_conv_desc *d) {
  if (validate_split(d)) return -1;
  return wgrad_split_splits(d);
}

int mvg_conv_wgrad_split_tile(const mvg_conv_desc *d, int32_t *bm, int32_t *bn, int32_t *incremental) {
  if (validate_split(d)) return -1;
  int tm, tn;
  bool incr;
  wgrad_split_tile(d, tm, tn, incr);
  if (bm) *bm = tm;
  if (bn) *bn = tn;
  if (incremental) *incremental = incr ? 1 : 0;
  return 0;
}

static int wgrad_split_impl(const mvg_conv_desc *d, const void *x_sp, const void *dy_sp, const float *dy_sinv, float *dw, float *workspace,
                            int splits, int accumulate, void *stream, int stride_w = -1, int pad_w = -1, const float *x_sinv = nullptr,
                            bool slabs_only = false) {
  if (stride_w < 0 && validate_split(d)) return 2;
  WgradParams p;
  memset(&p, 0, sizeof(p));
  p.x = (const float *)x_sp;
  p.dy = (const float *)dy_sp;
  p.dy_sinv = dy_sinv;
  p.x_sinv = x_sinv;
  int bm, bn;
  bool incr;
  wgrad_split_tile(d, bm, bn, incr);
  const double pixels = (double)d->groups * d->n * d->ho * d->wo;
  const double flops = 2.0 * pixels * d->cout * d->r * d->s * d->cin * (stride_w >= 0 ? 147.0 / 224.0 : 1.0);
  const double bytes = (double)SP_BYTES * ((double)d->groups * d->n * d->h * d->w * d->cin + pixels * d->cout) +
                       4.0 * (double)d->cout * d->r * d->s * d->cin;
  const auto dispatch = [&](dim3 grid, dim3 block, hipStream_t st, const WgradParams &wp) {
#define MVG_WGRAD_SPLIT(BM_, BN_)                                                                  \
  do {                                                                                             \
    if (incr) hipLaunchKernelGGL((wgrad_split_kernel<BM_, BN_, true>), grid, block, 0, st, wp);     \
    else hipLaunchKernelGGL((wgrad_split_kernel<BM_, BN_, false>), grid, block, 0, st, wp);         \
  } while (0)
    if (bm == 128 && bn == 256) MVG_WGRAD_SPLIT(128, 256);
    else if (bm == 128 && bn == 192) MVG_WGRAD_SPLIT(128, 192);
    else if (bm == 64 && bn == 192) MVG_WGRAD_SPLIT(64, 192);
    else if (bm == 128 && bn == 128) MVG_WGRAD_SPLIT(128, 128);
    else if (bm == 64 && bn == 128) MVG_WGRAD_SPLIT(64, 128);
    else if (bm == 128 && bn == 64) MVG_WGRAD_SPLIT(128, 64);
    else MVG_WGRAD_SPLIT(64, 64);
#undef MVG_WGRAD_SPLIT
    return 0;
  };
  return wgrad_launch(p, d, SP_BYTES, 16, bm, bn, dw, nullptr, workspace, splits, accumulate, slabs_only, (hipStream_t)stream, flops, bytes,
                      "wgrad_split", "conv_wgrad_split", stride_w, pad_w, dispatch);
}

// x_sinv (may be NULL = unscaled): the 2^-k of an activation operand stored times 2^k (bn.hip: act_scales_kernel)
int mvg_conv_wgrad_split_xs(const mvg_conv_desc *d, const void *x_sp, const float *x_sinv, const void *dy_sp, const float *dy_sinv,
                            float *dw, float *workspace, int splits, int accumulate, void *stream) {
  MVG_REQUIRE(d && x_sp && dy_sp && dw, "wgrad_split: d, x_sp, dy_sp and dw are required");
  return wgrad_split_impl(d, x_sp, dy_sp, dy_sinv, dw, workspace, splits, accumulate, stream, -1, -1, x_sinv);
}

int mvg_conv_wgrad_split(const mvg_conv_desc *d, const void *x_sp, const void *dy_sp, const float *dy_sinv, float *dw, float *workspace,
                         int splits, int accumulate, void *stream) {
  return wgrad_split_impl(d, x_sp, dy_sp, dy_sinv, dw, workspace, splits, accumulate, stream);
}

int mvg_conv_wgrad_split_slabs_xs(const mvg_conv_desc *d, const void *x_sp, const float *x_sinv, const void *dy_sp, const float *dy_sinv,
                                  float *workspace, int splits, void *stream) {
  MVG_REQUIRE(d && x_sp && dy_sp, "wgrad_split_slabs: d, x_sp and dy_sp are required");
  MVG_REQUIRE(splits > 1 && workspace, "wgrad_split_slabs: splits > 1 and a workspace (the slabs ARE the result)");
  return wgrad_split_impl(d, x_sp, dy_sp, dy_sinv, workspace, workspace, splits, 0, stream, -1, -1, x_sinv, true);
}

int mvg_conv_wgrad_split_slabs(const mvg_conv_desc *d, const void *x_sp, const void *dy_sp, const float *dy_sinv, float *workspace, int splits,
                               void *stream) {
  MVG_REQUIRE(splits > 1 && workspace, "wgrad_split_slabs: splits > 1 and a workspace (the slabs ARE the result)");
  return wgrad_split_impl(d, x_sp, dy_sp, dy_sinv, workspace, workspace, splits, 0, stream, -1, -1, nullptr, true);
}

int mvg_wgrad_reduce_batch(const float *const *host_slabs, float *const *host_dw, const int64_t *host_n, const int32_t *host_splits,
                           const int32_t *host_accumulate, int n, void *stream) {
  MVG_REQUIRE(host_slabs && host_dw && host_n && host_splits && host_accumulate && n >= 1 && n <= 8, "wgrad_reduce_batch: 1..8 items");
  ReduceBatch b;
  memset(&b, 0, sizeof(b));
  b.n = n;
  long long blocks = 0;
  double bytes = 0.0;
  for (int i = 0; i < n; ++i) {
    MVG_REQUIRE(host_slabs[i] && host_dw[i] && host_n[i] > 0 && host_n[i] % 4 == 0 && host_splits[i] > 1, "wgrad_reduce_batch: bad item");
    ReduceItem &r = b.it[i];
    r.slabs = host_slabs[i];
    r.dw = host_dw[i];
    r.n4 = host_n[i] / 4;
    r.splits = host_splits[i];
    r.accumulate = host_accumulate[i];
    r.lanes = wgrad_reduce_lanes(r.splits);
    r.block0 = (int)blocks;
    blocks += (r.n4 + 256 / r.lanes - 1) / (256 / r.lanes);
    bytes += 4.0 * host_n[i] * (r.splits + 1);
  }
  MVG_REQUIRE(blocks < (1LL << 31), "wgrad_reduce_batch: grid too large");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_WGRAD_REDUCE, st, 0.0, bytes);
  hipLaunchKernelGGL(wgrad_reduce_batch_kernel, dim3((unsigned)blocks), dim3(256), 0, st, b);
  return check_launch("wgrad_reduce_batch");
}

// ---- the fusion block's Linear layers on the split kernels (heads.py: a Linear = a 1x1 conv on a 1x1 map) ----------------
static mvg_conv_desc linear_desc(int rows, int fin, int fout) {
  mvg_conv_desc d;
  memset(&d, 0, sizeof(d));
  d.groups = 1; d.n = rows; d.h = d.w = d.ho = d.wo = 1; d.cin = fin; d.cout = fout; d.r = d.s = 1; d.stride = 1; d.pad = 0;
  return d;
}

int mvg_split_colsum(const float *g, int rows, int cols, const float *absmax, void *out_sp, float *out_sinv, float *db, int accumulate,
                     void *stream) {
  MVG_REQUIRE(g && absmax && out_sp && out_sinv && rows > 0 && cols > 0 && cols % 32 == 0, "split_colsum: null argument or cols %% 32 != 0");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_COLSUM, st, 0.0, (4.0 + SP_BYTES) * (double)rows * cols);
  hipLaunchKernelGGL(split_colsum_kernel, dim3(cols / 32), dim3(256), 0, st, g, rows, cols, (const unsigned *)absmax, (uint4 *)out_sp, out_sinv,
                     db, accumulate);
  return check_launch("split_colsum");
}

int mvg_linear_fprop_split(int rows, int fin, int fout, const void *x_sp, const float *x_sinv, const void *w_sp, const float *w_sinv,
                           const float *bias, int relu, void *out, int out_sp, float *out_sinv, const float *bias_absmax,
                           float *out_absmax, void *stream) {
  MVG_REQUIRE(bias != nullptr && out != nullptr, "linear_fprop_split: bias and out are required");
  MVG_REQUIRE(!out_sp || out_sinv, "linear_fprop_split: an sp result needs out_sinv (it is stored scaled)");
  MVG_REQUIRE(!(out_sp && out_absmax), "linear_fprop_split: out_absmax is for fp32 results");
  const mvg_conv_desc d = linear_desc(rows, fin, fout);
  const SplitAffine a = {nullptr, bias, nullptr, 0, relu, out_sp, 1, out_absmax, out_sinv, bias_absmax, nullptr};
  return fprop_split_impl(&d, x_sp, x_sinv, w_sp, w_sinv, out, nullptr, stream, &a);
}

int mvg_linear_dgrad_split(int rows, int fin, int fout, const void *dy_sp, const float *dy_sinv, const void *wt_sp, const float *w_sinv,
                           float *dx, const float *addend, const void *relu_mask_sp, float *out_absmax, void *stream) {
  const mvg_conv_desc d = linear_desc(rows, fin, fout);
  return dgrad_split_impl(&d, dy_sp, dy_sinv, wt_sp, w_sinv, dx, addend, stream, nullptr, relu_mask_sp, true, out_absmax);
}

int mvg_linear_wgrad_split(int rows, int fin, int fout, const void *x_sp, const float *x_sinv, const void *dy_sp, const float *dy_sinv,
                           float *dw, float *workspace, int splits, int accumulate, void *stream) {
  const mvg_conv_desc d = linear_desc(rows, fin, fout);
  return wgrad_split_impl(&d, x_sp, dy_sp, dy_sinv, dw, workspace, splits, accumulate, stream, -1, -1, x_sinv);
}

int mvg_linear_plan_query_split(int rows, int fin, int fout, int dgrad, int32_t *bm, int32_t *bn, int32_t *stages) {
  // what mvg_linear_fprop_split (dgrad == 0) / mvg_linear_dgrad_split (dgrad != 0) run for this Linear: its descriptor through the
  // checks, the geometry and the plan those launches use (fprop_split_impl / dgrad_split_impl -> launch_igemm_split with lin).
  // stages: the LIN kernels have the two-stage K loop at both tile widths, so it is the plan's `pipelined` alone - not
  // split_conv_stages, the convs' rule.  Launches nothing.
  const mvg_conv_desc d = linear_desc(rows, fin, fout);
  if (validate_split(&d)) return -1;
  IgemmParams p;
  memset(&p, 0, sizeof(p));
  SplitPlan pl;
  if (dgrad) {
    if (dgrad_geometry(p, &d, SP_BYTES, SP_BYTES, "split conv")) return -1;
    if ((long long)d.n * d.h * d.w * d.cin >= (1ll << 31)) return set_error("split conv: a group of dx exceeds 2^31 elements"), -1;
    DgradDropped dropped;
    dgrad_plan_classes(p, &d, false, dropped);
    if (p.ncls == 0) return -1;
    pl = split_plan(p.ncols, d.r * d.s, (long long)d.n * d.h * d.w, p.groups, true, p.cls, p.ncls);
  } else {
    if (fprop_geometry(p, &d, SP_BYTES, SP_BYTES, "split conv", -1, -1)) return -1;
    if (p.rows_per_group * (long long)d.cout >= (1ll << 31)) return set_error("split conv: a group of the output exceeds 2^31 elements"), -1;
    pl = split_plan(p.ncols, d.r * d.s, p.rows_per_group, p.groups, true, p.cls, p.ncls);
  }
  if (pl.tiles <= 0 || pl.tiles >= (1LL << 31)) return set_error("split conv: grid too large"), -1;
  if (bm) *bm = pl.bm;
  if (bn) *bn = pl.bn;
  if (stages) *stages = pl.pipelined ? 2 : 1;
  return 0;
}

// ---- the 7x7 stride-2 stem on the split kernels ("row-window" form) ------------------------------------------------
// A 3-channel (stored 4) image has too few channels for a K-step of the implicit GEMM: the fp32-MFMA kernel runs it at
// ~75 % of ITS peak (117 TFLOP/s with the padding channel).  Rewritten: xw[n][y][ox][j][c], j = 0..7, c = 0..3 holds
// image column 2 ox - 4 + j (zero outside the image) - the 8 columns the 7 taps of output column ox touch, plus one
// in front so that pixel pairs stay 16-byte aligned - and the stem becomes a 7 x 1 filter with 32 "channels", vertical
// stride 2 / padding 3, horizontal stride 1 / padding 0, over ho x wo windows: K = 7 x 32 = 224, the shape
// igemm_split16_kernel / wgrad_split_kernel are built for.  Weights w'[o][r][j][c] = w[o][r][j - 1][c] (j = 0, c = 3: zero).
static int stem_desc(const mvg_conv_desc *d, mvg_conv_desc *rw) {
  MVG_REQUIRE(d != nullptr, "stem (row-window): null descriptor");
  MVG_REQUIRE(d->r == 7 && d->s == 7 && d->stride == 2 && d->pad == 3 && d->cin == 4, "stem (row-window): 7x7 stride 2 pad 3, 4 stored channels");
  MVG_REQUIRE(d->w % 2 == 0 && d->ho == (d->h - 1) / 2 + 1 && d->wo == d->w / 2, "stem (row-window): even width; ho, wo inconsistent");
  MVG_REQUIRE(d->cout % 32 == 0 && d->groups > 0 && d->n > 0, "stem (row-window): cout must be a multiple of 32");
  *rw = *d;
  rw->w = d->wo;            // windows per image row
  rw->cin = 32;
  rw->s = 1;
  return 0;
}

int mvg_stem_rowwindow_split(const float *x_nhwc4, void *xw_sp, int64_t images, int h, int w, void *stream) {
  MVG_REQUIRE(x_nhwc4 && xw_sp && images > 0 && h > 0 && w > 0 && w % 2 == 0, "stem_rowwindow: bad arguments (even width)");
  hipStream_t st = (hipStream_t)stream;
  const long long n = images * h * (w / 2) * 4;                 // one thread per 8-value chunk (two pixels)
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, 16.0 * (double)images * h * w + 32.0 * (double)n);
  long long blocks = (n + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(stem_rowwindow_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float4 *)x_nhwc4, (uint4 *)xw_sp, n, h, w);
  return check_launch("stem_rowwindow");
}

int mvg_stem_rowwindow_split_nchw(const float *x_nchw, void *xw_sp, int64_t images, int h, int w, void *stream) {
  MVG_REQUIRE(x_nchw && xw_sp && images > 0 && h > 0 && w > 0 && w % 2 == 0, "stem_rowwindow (NCHW): bad arguments (even width)");
  hipStream_t st = (hipStream_t)stream;
  const long long n = images * h * (w / 2) * 4;
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, 12.0 * (double)images * h * w + 32.0 * (double)n);
  long long blocks = (n + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(stem_rowwindow_nchw_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x_nchw, (uint4 *)xw_sp, n, h, w);
  return check_launch("stem_rowwindow_nchw");
}

int mvg_stem_fprop_split(const mvg_conv_desc *d, const void *xw_sp, const void *w_sp, const float *w_sinv, float *y, float *stats,
                         void *stream) {
  mvg_conv_desc rw;
  if (stem_desc(d, &rw)) return 2;
  return fprop_split_impl(&rw, xw_sp, nullptr, w_sp, w_sinv, y, stats, stream, nullptr, 1, 0);
}

int mvg_stem_wgrad_splits_split(const mvg_conv_desc *d) {
  mvg_conv_desc rw;
  if (stem_desc(d, &rw)) return -1;
  // the rewritten descriptor's own tile, as wgrad_split_impl launches it: its 7 x 32 = 224 columns are >= 128 and a multiple of
  // neither 256 nor 192, so wgrad_split_tile answers bn = 128 (three workgroups per CU) and bm = 128 or 64 by cout, for every cout
  return wgrad_split_splits(&rw);
}

int mvg_stem_wgrad_split(const mvg_conv_desc *d, const void *xw_sp, const void *dy_sp, const float *dy_sinv, float *dw_rw, float *workspace,
                         int splits, int accumulate, void *stream) {
  mvg_conv_desc rw;
  if (stem_desc(d, &rw)) return 2;
  return wgrad_split_impl(&rw, xw_sp, dy_sp, dy_sinv, dw_rw, workspace, splits, accumulate, stream, 1, 0);
}

int mvg_stem_plan_query_split(const mvg_conv_desc *d, int32_t *fwd_bm, int32_t *fwd_bn, int32_t *fwd_stages, int32_t *wgrad_bm,
                              int32_t *wgrad_bn, int32_t *wgrad_incremental) {
  // what mvg_stem_fprop_split / mvg_stem_wgrad_split run for `d`: the rewritten descriptor through the geometry, the plan and the
  // tile choice the launches use (fprop_split_impl -> launch_igemm_split; wgrad_split_impl).  Launches nothing.
  mvg_conv_desc rw;
  if (stem_desc(d, &rw)) return -1;
  IgemmParams p;
  memset(&p, 0, sizeof(p));
  if (fprop_geometry(p, &rw, SP_BYTES, SP_BYTES, "split conv", 1, 0)) return -1;
  const SplitPlan pl = split_plan(p.ncols, rw.r * rw.s, p.rows_per_group, p.groups, false, p.cls, p.ncls);
  if (fwd_bm) *fwd_bm = pl.bm;
  if (fwd_bn) *fwd_bn = pl.bn;
  if (fwd_stages) *fwd_stages = split_conv_stages(pl);
  int tm, tn;
  bool incr;
  wgrad_split_tile(&rw, tm, tn, incr);
  if (wgrad_bm) *wgrad_bm = tm;
  if (wgrad_bn) *wgrad_bn = tn;
  if (wgrad_incremental) *wgrad_incremental = incr ? 1 : 0;
  return 0;
}

}  // extern "C"
