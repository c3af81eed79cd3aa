// Implicit-GEMM convolution / linear kernels on the gfx950 bf16 matrix cores
// (v_mfma_f32_32x32x16_bf16: bf16 operands, fp32 accumulation) - the "bf16 MFMA path" of BASELINE
// config C5.  Activations and weights are bf16 in HBM (NHWC / KRSC), BatchNorm statistics, biases and
// weight gradients stay fp32.  The fp32 path (conv_igemm.hip) is the parity path (1e-4); this one has
// its own declared tolerance (tests/test_bf16_gpu.py).
//
//   fprop : y[m][o]       = sum_{tap,c} x[pix(m,tap)][c]   * w [o][tap][c]     A gathered, B = KRSC weights
//   dgrad : dx[m][c]      = sum_{tap,o} dy[pix'(m,tap)][o] * wT[c][tap][o]     A gathered, B = the weights
//                                                                              transposed once per step (CRSK)
//   wgrad : dw[o][tap][c] = sum_m       dy[m][o]           * x[pix(m,tap)][c]  both operands pixel-major in
//                                                                              LDS, fragments by ds_read_b64_tr_b16
//
// Both fprop/dgrad operands are k-contiguous, so ONE kernel serves both: 256 threads = 4 waves, tile
// 128 x BN x 64 (a K-step is 128 bytes per row = one cache line per gathered pixel), 16-byte buffer loads
// with out-of-range predication -> registers -> LDS rows padded to 144 bytes (conflict-free
// ds_read_b128 fragments), three-stage pipeline like the fp32 kernel.  MFMA operand map
// (cdna_hip_programming.md 3): lane l holds A[row l&31][k = 8*(l>>5) + j], B[k = 8*(l>>5) + j][col l&31].
// The epilogue goes through LDS (fp32 tile) so that global stores are 16-byte vectors of 8 bf16 along
// the channel axis; BN partial statistics come from the fp32 accumulators.
#include "bf16_tile.h"

namespace mvg {

constexpr int BF_BM = 128, BF_BK = 64, BF_LDK = BF_BK + 8;

// The GEMM kernels (register-staged and LDS-DMA form) live in conv_bf16_gemm.inc: once as the training kernels, once
// with the inference epilogue (mvg_conv_fprop_bf16_affine).
#define MVG_BF16_AFF 0
#include "conv_bf16_gemm.inc"
#undef MVG_BF16_AFF
#define MVG_BF16_AFF 1
#include "conv_bf16_gemm.inc"
#undef MVG_BF16_AFF

// ------------------------------------------------------------------------------------------
// wgrad: dw[o][tap][c] = sum over pixels of dy[pix][o] * x[pix at tap][c]; M = cout, N = (tap, c),
// K = pixels split into slabs (fixed-order reduce: wgrad_reduce_kernel).  Tile decode, column and pixel addressing and
// the epilogue are conv_shared.h's (wgrad_tile_id, wgrad_column, WgradPixel, wgrad_store_acc).  Both operands arrive
// pixel-major (NHWC rows), i.e. k-strided for the MFMA: the LDS images stay pixel-major [k][m] and the
// fragments are read with the hardware transpose read ds_read_b64_tr_b16 (4 k x 16 m per 16-lane group,
// cdna_hip_programming.md T10); rows of (BM + 32) * 2 bytes put the four k-rows of a read on disjoint
// bank ranges (conflict-free).
// ------------------------------------------------------------------------------------------

// F32IN (Linear layers of the fusion block in the bf16 path): x and dy are fp32 in memory and rounded to bf16 on
// the way into LDS; the bias gradient (column sums of the fp32 dy) rides along like in the fp32 kernel.
template <int BM, int BN, bool INCR, bool F32IN = false>
__global__ __launch_bounds__(256, 2) void wgrad_bf16_kernel(WgradParams p) {
  constexpr int BK = 64, WGM = 2, WGN = 2;
  constexpr unsigned EB = F32IN ? 4u : 2u;   // bytes per element of x and dy
  constexpr int AL = F32IN ? 2 : 1;
  constexpr int WTM = BM / WGM, WTN = BN / WGN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int LDA = BM + 32, LDB = BN + 32;
  constexpr int MV = BM / 8, NVB = BN / 8;
  constexpr int A_KRPP = 256 / MV;
  constexpr int A_PASSES = BK / A_KRPP;
  constexpr int A_ELEMS = BK * LDA, B_ELEMS = BK * LDB;
  __shared__ __attribute__((aligned(16))) unsigned short smem[2 * (A_ELEMS + B_ELEMS)];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN;
  const int li = lane & 31, lh = lane >> 5;
  const WgradTile t = wgrad_tile_id(p);

  const char *dy = reinterpret_cast<const char *>(p.dy);
  const char *x = reinterpret_cast<const char *>(p.x);
  const __amdgpu_buffer_rsrc_t rs_a = make_rsrc(dy + t.m_begin * p.cout * EB, (long long)EB * t.m_count * p.cout);
  const long long x_img_elems = (long long)p.h * p.w * p.cin;
  const __amdgpu_buffer_rsrc_t rs_b = make_rsrc(x + t.img0 * x_img_elems * EB, p.x_bytes - (long long)EB * t.img0 * x_img_elems);
  const int a_mv = tid % MV, a_k0 = tid / MV;
  const int a_col = t.mtile * BM + a_mv * 8;
  const bool a_cok = a_col < p.cout;
  unsigned a_off[A_PASSES];
#pragma unroll
  for (int i = 0; i < A_PASSES; ++i)
    a_off[i] = a_cok ? (unsigned)((a_k0 + i * A_KRPP) * p.cout + a_col) * EB : 0x80000000u;

  // B (x gather): a thread's loads of one K-step all come from ONE pixel row (row = tid / B_TPR) and differ
  // in the column group; INCR carries (oy, ox, image offset) of that pixel and steps it by BK pixels per K-step.
  constexpr int B_TPR = 256 / BK;                       // threads per k-row
  constexpr int B_CPT = NVB / B_TPR;                    // column groups per thread
  static_assert(NVB % B_TPR == 0 && B_CPT >= 1, "wgrad loader mapping");
  const int i_row = tid / B_TPR, i_nv0 = tid % B_TPR;
  WgradColumn i_col[B_CPT];
#pragma unroll
  for (int j = 0; j < B_CPT; ++j) i_col[j] = wgrad_column(p, t.ntile * BN + (i_nv0 + j * B_TPR) * 8, EB, p.pad_w);
  const unsigned row_bytes = (unsigned)(p.stride * p.w * p.cin) * EB, col_bytes = (unsigned)(p.stride_w * p.cin) * EB;
  const unsigned img_bytes = (unsigned)x_img_elems * EB;
  WgradPixel s_px = {0, 0, 0u};
  if (INCR) s_px.decode(p, t.rem0 + (unsigned)i_row, img_bytes);
  u32x4 a_reg[A_PASSES][AL], b_reg[B_CPT][AL];
  const bool do_bias = F32IN && (p.db != nullptr) && (t.ntile == 0);
  float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto load_tiles = [&](int kt) {
#pragma unroll
    for (int i = 0; i < A_PASSES; ++i) {
      a_reg[i][0] = __builtin_amdgcn_raw_buffer_load_b128(rs_a, a_off[i], 0, 0);  // rows >= m_count: beyond the descriptor = zeros
      if constexpr (F32IN) a_reg[i][1] = __builtin_amdgcn_raw_buffer_load_b128(rs_a, a_off[i] + 16u, 0, 0);
      a_off[i] += (unsigned)(BK * p.cout) * EB;
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
      b_reg[j][0] = __builtin_amdgcn_raw_buffer_load_b128(rs_b, pred_off(pixoff + c.tconst, ok), 0, 0);
      if constexpr (F32IN) b_reg[j][1] = __builtin_amdgcn_raw_buffer_load_b128(rs_b, pred_off(pixoff + c.tconst + 16u, ok), 0, 0);
    }
    if constexpr (INCR) s_px.template advance<BK>(p, img_bytes);
  };
  auto to_bf16 = [&](const u32x4 (&r)[AL]) -> u32x4 {
    if constexpr (!F32IN) return r[0];
    u32x4 v;
    v.x = pack_bf2(__uint_as_float(r[0].x), __uint_as_float(r[0].y));
    v.y = pack_bf2(__uint_as_float(r[0].z), __uint_as_float(r[0].w));
    v.z = pack_bf2(__uint_as_float(r[AL - 1].x), __uint_as_float(r[AL - 1].y));
    v.w = pack_bf2(__uint_as_float(r[AL - 1].z), __uint_as_float(r[AL - 1].w));
    return v;
  };
  auto store_tiles = [&](int buf) {
    unsigned short *As = smem + buf * (A_ELEMS + B_ELEMS);
    unsigned short *Bs = As + A_ELEMS;
#pragma unroll
    for (int i = 0; i < A_PASSES; ++i) *reinterpret_cast<u32x4 *>(As + (a_k0 + i * A_KRPP) * LDA + a_mv * 8) = to_bf16(a_reg[i]);
    if constexpr (F32IN) {
      if (do_bias) {                   // every K-step's rows exactly once, in order, from the fp32 values
#pragma unroll
        for (int i = 0; i < A_PASSES; ++i) {
          bsum[0] += __uint_as_float(a_reg[i][0].x); bsum[1] += __uint_as_float(a_reg[i][0].y);
          bsum[2] += __uint_as_float(a_reg[i][0].z); bsum[3] += __uint_as_float(a_reg[i][0].w);
          bsum[4] += __uint_as_float(a_reg[i][AL - 1].x); bsum[5] += __uint_as_float(a_reg[i][AL - 1].y);
          bsum[6] += __uint_as_float(a_reg[i][AL - 1].z); bsum[7] += __uint_as_float(a_reg[i][AL - 1].w);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < B_CPT; ++j) *reinterpret_cast<u32x4 *>(Bs + i_row * LDB + (i_nv0 + j * B_TPR) * 8) = to_bf16(b_reg[j]);
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
    const unsigned short *As = smem + cur * (A_ELEMS + B_ELEMS);
    const unsigned short *Bs = As + A_ELEMS;
#pragma unroll
    for (int kg = 0; kg < BK / 16; ++kg) {
      bf16x8 av[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) av[i] = tr_frag(As, LDA, kg * 16, wm * WTM + i * 32, lane);
#pragma unroll
      for (int j = 0; j < TN; ++j) bv[j] = tr_frag(Bs, LDB, kg * 16, wn * WTN + j * 32, lane);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  if constexpr (F32IN) {
    if (do_bias) {                     // loader rows (a_k0) summed through LDS in a fixed order; the K loop ended with a barrier
      float *sh = reinterpret_cast<float *>(smem);
#pragma unroll
      for (int k = 0; k < 8; ++k) sh[tid * 8 + k] = bsum[k];
      __syncthreads();
      if (a_k0 == 0 && a_cok) {
        float s[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = sh[a_mv * 8 + k];
        for (int r = 1; r < A_KRPP; ++r)
#pragma unroll
          for (int k = 0; k < 8; ++k) s[k] += sh[(r * MV + a_mv) * 8 + k];
        float *dst = p.db + (long long)t.split * p.cout + a_col;
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[k] = (p.accumulate ? dst[k] : 0.f) + s[k];
      }
    }
  }
  wgrad_store_acc(p, acc, p.out + (long long)t.split * p.cout * p.ncols, t.mtile * BM + wm * WTM, t.ntile * BN + wn * WTN, li, lh, 1.f);
}

// The stem's folded row-window operand (mvg_stem_fprop_bf16): window m of an image row holds image columns 4 m - 4 ..
// 4 m + 11 x 4 channels (3 real) in bf16 - 64 values, the K-step of the LDS-DMA kernel - straight from the NCHW fp32
// input.  One thread per 8-value chunk = two columns.
__global__ __launch_bounds__(256) void stem_rowwindow_bf16_kernel(const float *__restrict__ x, uint4 *__restrict__ xw, long long n, int h, int w) {
  const int wm = w >> 2;
  const long long plane = (long long)h * w;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int q = (int)(i & 7);
    const long long t = i >> 3;
    const int m = (int)(t % wm);
    const long long row = t / wm;                    // image * h + y
    const long long img = row / h;
    const int yy = (int)(row - img * h);
    const int c0 = 4 * m - 4 + 2 * q;                 // even: both columns in range or both out (w % 4 == 0)
    uint4 o = make_uint4(0u, 0u, 0u, 0u);
    if (c0 >= 0 && c0 < w) {
      const float *src = x + img * 3 * plane + (long long)yy * w + c0;
      const float2 r = *reinterpret_cast<const float2 *>(src), g = *reinterpret_cast<const float2 *>(src + plane),
                   b = *reinterpret_cast<const float2 *>(src + 2 * plane);
      o = make_uint4(bf16_pack2(r.x, g.x), bf16_pack2(b.x, 0.f), bf16_pack2(r.y, g.y), bf16_pack2(b.y, 0.f));
    }
    xw[i] = o;
  }
}

// fp32 KRSC weights -> bf16 KRSC (cin zero-padded to cin_pad) and, optionally, the transposed CRSK copy the
// backward-data kernel reads ([cin_pad][r*s][cout]).  One thread per (o, tap, c).
__global__ __launch_bounds__(256) void cast_weights_bf16_kernel(const float *__restrict__ w, unsigned short *__restrict__ wk,
                                                                unsigned short *__restrict__ wt, int cout, int rs, int cin,
                                                                int cin_pad) {
  const long long total = (long long)cout * rs * cin_pad;
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
// host side
// ------------------------------------------------------------------------------------------
static int validate_bf16(const mvg_conv_desc *d) {
  if (validate(d)) return 2;
  MVG_REQUIRE(d->cin % 8 == 0 && d->cout % 8 == 0, "bf16 conv: cin and cout must be multiples of 8 (got %d, %d)", d->cin, d->cout);
  return 0;
}

// The plan of a forward / backward-data launch, host arithmetic only: the column tile, each class's tiles and K-steps, the
// K order, and whether every class can take the uniform-tap loader (fasta).  p: the geometry and the classes; the launch
// fields (ntiles, the classes' tile offsets, bn_parts) are set here.  What launch_igemm_bf16 launches by and what
// mvg_conv_plan_query_bf16 reports.  The kernel follows from the plan: the LDS-DMA kernel iff fasta with bf16 operands
// (the fp32-operand Linears stay on the register-staged kernel, fasta choosing its loader).
template <bool DGRAD>
static int plan_igemm_bf16(IgemmParams &p, bool f32io, mvg_conv_plan &pl, long long &tiles) {
  const int bn = p.ncols >= 128 ? 128 : 64;
  p.ntiles = ceil_div(p.ncols, bn);
  p.splits = 1;
  p.sk_tiles = 0;
  tiles = 0;
  bool fasta = true;
  const bool bnf = DGRAD && p.bn_part != nullptr;
  p.bn_parts = 0;
  for (int i = 0; i < p.ncls; ++i) {
    IgemmClass &c = p.cls[i];
    c.mtiles_per_group = ceil_div(c.rows_per_group, BF_BM);
    c.KT = c.ktotal > 0 ? ceil_div(c.ktotal, BF_BK) : (bnf ? 0 : 1);     // fused reduce: a class without taps is epilogue only
    c.korder = (c.ntaps > 1 && p.src_c % BF_BK == 0) ? 1 : 0;
    c.per_div = make_fastdiv((unsigned)(c.ntaps > 0 ? c.ntaps : 1));
    c.tile0 = (int)tiles;
    c.unit0 = 0;
    c.part0 = p.bn_parts;
    p.bn_parts += c.mtiles_per_group;
    const long long ti = (long long)p.groups * c.mtiles_per_group * p.ntiles;
    tiles += ti;
    fasta = fasta && (c.ntaps >= 1 || bnf) && c.ntaps <= 32 && c.ktotal % BF_BK == 0 && p.src_c % BF_BK == 0;
    pl.cls_tiles[i] = (int32_t)ti;
    pl.cls_kt[i] = c.KT;
  }
  MVG_REQUIRE(tiles < (1LL << 31), "bf16 conv: grid too large");
  MVG_REQUIRE(!bnf || (fasta && !f32io), "bf16 dgrad with a fused BatchNorm reduce: bf16 operands, channel counts in multiples of 64");
  pl.bm = BF_BM;
  pl.bn = bn;
  pl.bk = BF_BK;
  pl.fasta = fasta ? 1 : 0;
  pl.ncls = p.ncls;
  pl.streamk_grid = 0;
  pl.splitk = 1;
  pl.scratch_floats = 0;
  return 0;
}

// `query` != nullptr (mvg_conv_plan_query_bf16): the plan is written there and nothing is launched
template <bool DGRAD>
static int launch_igemm_bf16(IgemmParams &p, hipStream_t st, bool f32io = false, bool affine = false, mvg_conv_plan *query = nullptr) {
  mvg_conv_plan pl;
  memset(&pl, 0, sizeof(pl));
  long long tiles = 0;
  if (int e = plan_igemm_bf16<DGRAD>(p, f32io, pl, tiles)) return e;
  if (query) {
    *query = pl;
    return 0;
  }
  const int bn = pl.bn;
  const bool fasta = pl.fasta != 0;
  if (tiles <= 0) return 0;
  dim3 grid((unsigned)tiles), block(256);
  if constexpr (!DGRAD) {
    if (affine) {                             // inference: the same kernel choice as the training forward, AFF instantiations
      if (fasta) {
        if (bn == 128) hipLaunchKernelGGL((igemm_bf16_dma_affine_kernel<128>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((igemm_bf16_dma_affine_kernel<64>), grid, block, 0, st, p);
      } else if (bn == 128) {
        hipLaunchKernelGGL((igemm_bf16_affine_kernel<128>), grid, block, 0, st, p);
      } else {
        hipLaunchKernelGGL((igemm_bf16_affine_kernel<64>), grid, block, 0, st, p);
      }
      return check_launch("conv_fprop_bf16_affine");
    }
  }
  if (f32io) {
    if (bn == 128) {
      if (fasta) hipLaunchKernelGGL((igemm_bf16_kernel<128, DGRAD, true, true>), grid, block, 0, st, p);
      else hipLaunchKernelGGL((igemm_bf16_kernel<128, DGRAD, false, true>), grid, block, 0, st, p);
    } else {
      if (fasta) hipLaunchKernelGGL((igemm_bf16_kernel<64, DGRAD, true, true>), grid, block, 0, st, p);
      else hipLaunchKernelGGL((igemm_bf16_kernel<64, DGRAD, false, true>), grid, block, 0, st, p);
    }
  } else if (fasta) {
    // uniform-tap shapes: the LDS-DMA kernel in its one-stage, four-workgroups-per-CU form (measured faster than the
    // two-stage form at every ResNet-50 shape: C5 fprop 10.4 -> 8.4 ms, dgrad 9.5 -> 7.5 ms)
    if (bn == 128) hipLaunchKernelGGL((igemm_bf16_dma_kernel<128, DGRAD, 1>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((igemm_bf16_dma_kernel<64, DGRAD, 1>), grid, block, 0, st, p);
  } else if (bn == 128) {                   // the stem (4-channel taps): register-staged loader
    hipLaunchKernelGGL((igemm_bf16_kernel<128, DGRAD, false>), grid, block, 0, st, p);
  } else {
    hipLaunchKernelGGL((igemm_bf16_kernel<64, DGRAD, false>), grid, block, 0, st, p);
  }
  return check_launch(DGRAD ? "conv_dgrad_bf16" : "conv_fprop_bf16");
}

}  // namespace mvg

using namespace mvg;

extern "C" {

int mvg_conv_stats_partials_bf16(const mvg_conv_desc *d, int32_t *rows_per_partial) {
  if (validate_bf16(d)) return -1;
  const long long rows = (long long)d->n * d->ho * d->wo;
  if (rows_per_partial) *rows_per_partial = BF_BM / 2;
  return ceil_div(rows, BF_BM) * 2;
}

int mvg_cast_weights_bf16(const mvg_conv_desc *d, const float *w, int cin_src, void *w_krsc, void *w_crsk, void *stream) {
  MVG_REQUIRE(d && w && w_krsc, "cast_weights_bf16: null argument");
  MVG_REQUIRE(cin_src > 0 && cin_src <= d->cin, "cast_weights_bf16: cin_src must be in (0, cin]");
  hipStream_t st = (hipStream_t)stream;
  const long long total = (long long)d->cout * d->r * d->s * d->cin;
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, (w_crsk ? 8.0 : 6.0) * (double)total);
  long long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(cast_weights_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, st, w, (unsigned short *)w_krsc,
                     (unsigned short *)w_crsk, d->cout, d->r * d->s, cin_src, d->cin);
  return check_launch("cast_weights_bf16");
}

// stride_w >= 0: horizontal stride / padding differ from d->stride / d->pad, and the BatchNorm partials of GEMM columns
// c and c + cout/2 are two partials of channel c (the stem's folded row-window form, whose descriptor the caller checked)
struct Bf16Affine {        // inference: y = bf16([relu](acc * scale + shift (+ residual))), residual bf16 like y
  const float *scale, *shift;
  const void *residual;
};

static int fprop_bf16_impl(const mvg_conv_desc *d, const void *x, const void *wgt, void *y, const float *bias, int relu,
                           float *stats, void *stream, bool f32io, int stride_w = -1, int pad_w = -1, const Bf16Affine *aff = nullptr,
                           mvg_conv_plan *query = nullptr) {
  if (stride_w < 0 && validate_bf16(d)) return 2;
  IgemmParams p;
  memset(&p, 0, sizeof(p));
  p.a = (const float *)x;
  p.b = (const float *)wgt;
  p.out = (float *)y;
  p.bias = bias;
  p.relu = relu;
  p.stats = stats;
  p.stats_fold = stride_w >= 0 ? 1 : 0;
  if (aff) {
    p.scale = aff->scale;
    p.bias = aff->shift;
    p.addend = (const float *)aff->residual;
  }
  if (fprop_geometry(p, d, f32io ? 4 : 2, 2, "bf16 conv", stride_w, pad_w)) return 2;
  MVG_REQUIRE(p.rows_per_group * (long long)d->cout < (1ll << 31), "bf16 conv: a group of the output exceeds 2^31 elements");
  const double acin = d->cin == 8 && d->r == 7 ? 3.0 : (double)d->cin;       // the stem's channels 3..7 are zero padding
  const double flops = 2.0 * d->groups * (double)p.rows_per_group * d->cout * d->r * d->s * acin * (stride_w >= 0 ? 147.0 / 448.0 : 1.0);
  const double bytes = 2.0 * (d->groups * (double)d->n * d->h * d->w * acin + (double)d->cout * d->r * d->s * acin +
                              (aff && aff->residual ? 2.0 : 1.0) * d->groups * (double)p.rows_per_group * d->cout) + (aff ? 8.0 * d->cout : 0.0);
  const bool lin = d->r == 1 && d->s == 1 && d->h == 1 && d->w == 1;
  if (query) return launch_igemm_bf16<false>(p, nullptr, f32io, aff != nullptr, query);        // plan only: nothing is launched
  ProfScope ps(lin ? MVG_K_LINEAR_FPROP : MVG_K_CONV_FPROP, (hipStream_t)stream, flops, bytes);
  return launch_igemm_bf16<false>(p, (hipStream_t)stream, f32io, aff != nullptr);
}

int mvg_conv_fprop_bf16_affine(const mvg_conv_desc *d, const void *x, const void *wgt, void *out, const float *scale, const float *shift,
                               const void *residual, int relu, void *stream) {
  MVG_REQUIRE(d && x && wgt && out, "fprop_bf16_affine: null argument");
  MVG_REQUIRE(scale && shift, "fprop_bf16_affine: scale and shift are required");
  MVG_REQUIRE(residual != out || residual == nullptr, "fprop_bf16_affine: the residual must not alias the output");
  const Bf16Affine a = {scale, shift, residual};
  return fprop_bf16_impl(d, x, wgt, out, nullptr, relu, nullptr, stream, false, -1, -1, &a);
}

int mvg_conv_fprop_bf16(const mvg_conv_desc *d, const void *x, const void *wgt, void *y, const float *bias, int relu,
                        float *stats, void *stream) {
  return fprop_bf16_impl(d, x, wgt, y, bias, relu, stats, stream, false);
}

struct Bf16BnFuse {        // fused BatchNorm-backward reduce of the unit whose output gradient dx is (IgemmParams::bn_*)
  const void *y;           // bf16, like dx
  const uint8_t *bits;     // one byte per 8 channels (mvg_bn_apply_bits_bf16)
  const float *mean, *invstd, *rscale, *rshift;
  float *part;
};

static int dgrad_bf16_impl(const mvg_conv_desc *d, const void *dy, const void *wgt_crsk, void *dx, const void *mask,
                           const void *addend, void *stream, bool f32io, const Bf16BnFuse *bnf = nullptr, mvg_conv_plan *query = nullptr) {
  if (validate_bf16(d)) return 2;
  MVG_REQUIRE(!f32io || d->stride == 1, "bf16 dgrad with fp32 operands: stride 1 only");
  IgemmParams p;
  memset(&p, 0, sizeof(p));
  p.a = (const float *)dy;
  p.b = (const float *)wgt_crsk;
  p.out = (float *)dx;
  p.mask = (const float *)mask;
  p.addend = (const float *)addend;
  if (bnf) {
    p.bn_y = (const float *)bnf->y;
    p.bn_bits = bnf->bits;
    p.bn_mean = bnf->mean;
    p.bn_invstd = bnf->invstd;
    p.bn_rscale = bnf->rscale;
    p.bn_rshift = bnf->rshift;
    p.bn_part = bnf->part;
    p.bn_part_rows = 2;
  }
  if (dgrad_geometry(p, d, f32io ? 4 : 2, 2, "bf16 conv")) return 2;
  MVG_REQUIRE((long long)d->n * d->h * d->w * d->cin < (1ll << 31), "bf16 conv: a group of dx exceeds 2^31 elements");
  const double flops = 2.0 * d->groups * (double)d->n * d->ho * d->wo * d->cout * d->r * d->s * d->cin;
  const double bytes = 2.0 * (d->groups * (double)d->n * d->ho * d->wo * d->cout + (double)d->cout * d->r * d->s * d->cin) +
                       (bnf ? 4.125 : 2.0) * d->groups * (double)d->n * d->h * d->w * d->cin;      // (fused reduce: + y and the mask bits)
  const bool lin = d->r == 1 && d->s == 1 && d->h == 1 && d->w == 1;
  if (query) {                       // plan only: the class table without the fills of the classes it drops
    DgradDropped dropped;
    dgrad_plan_classes(p, d, bnf != nullptr, dropped);
    return launch_igemm_bf16<true>(p, nullptr, f32io, false, query);
  }
  ProfScope ps(lin ? MVG_K_LINEAR_DGRAD : MVG_K_CONV_DGRAD, (hipStream_t)stream, flops, bytes);
  if (int e = dgrad_classes(p, d, bnf != nullptr, f32io ? 4 : 2, dx, addend, (hipStream_t)stream)) return e;
  if (p.ncls == 0) return 0;
  return launch_igemm_bf16<true>(p, (hipStream_t)stream, f32io);
}

int mvg_conv_dgrad_bf16(const mvg_conv_desc *d, const void *dy, const void *wgt_crsk, void *dx, const void *mask,
                        const void *addend, void *stream) {
  return dgrad_bf16_impl(d, dy, wgt_crsk, dx, mask, addend, stream, false);
}

int mvg_conv_dgrad_bn_partials_bf16(const mvg_conv_desc *d) {
  if (validate_bf16(d)) return -1;
  return dgrad_bn_partials(d, BF_BM);
}

int mvg_conv_dgrad_bf16_bnreduce(const mvg_conv_desc *d, const void *dy, const void *wgt_crsk, void *dx, const void *addend,
                                 const void *bn_y, const uint8_t *bn_bits, const float *bn_mean, const float *bn_invstd,
                                 const float *relu_scale, const float *relu_shift, float *partials, float *s1, float *s2,
                                 float *dgamma, float *dbeta, int accumulate, void *stream) {
  MVG_REQUIRE(bn_y && bn_mean && bn_invstd && partials && s1 && s2, "dgrad_bf16_bnreduce: null argument");
  MVG_REQUIRE(!(bn_bits && relu_scale) && ((relu_scale == nullptr) == (relu_shift == nullptr)),
              "dgrad_bf16_bnreduce: give the ReLU mask either as bits or as (relu_scale, relu_shift)");
  const int P = mvg_conv_dgrad_bn_partials_bf16(d);
  MVG_REQUIRE(P > 0, "dgrad_bf16_bnreduce: bad descriptor");
  const Bf16BnFuse f = {bn_y, bn_bits, bn_mean, bn_invstd, relu_scale, relu_shift, partials};
  if (dgrad_bf16_impl(d, dy, wgt_crsk, dx, nullptr, addend, stream, false, &f)) return 1;
  ProfScope ps(MVG_K_BN_BWD_REDUCE, (hipStream_t)stream, 0.0, 8.0 * d->groups * (double)P * d->cin);
  return bn_bwd_finalize_launch(partials, d->groups, P, d->cin, s1, s2, dgamma, dbeta, accumulate, (hipStream_t)stream, nullptr, bn_mean,
                                bn_invstd);
}

// ---- the 7x7 stride-2 stem on the LDS-DMA kernels: folded row windows -------------------------------------------------
// These kernels' K-step is 64 channels of ONE tap; the stem offers 8 stored channels per tap (3 real): round 2 ran it on
// the register-staged kernel with K = 49 x 8 = 392 (1.05 ms of a C5 step).  Folded: window m of an image row = image
// columns 4 m - 4 .. 4 m + 11 x 4 channels = 64 values serves TWO output columns - ox = 2 m through filter taps at
// j = s + 1, ox = 2 m + 1 at j = s + 3 - as 2 x cout GEMM columns, whose [.., wo/2, 2 cout] output IS y [.., wo, cout]
// in memory.  A 7 x 1 filter over 64 "channels", vertical stride 2 / pad 3, horizontal stride 1 / pad 0: K = 448 per
// two outputs (224 each; the filter has 147).  BatchNorm partials: columns c and c + cout are two partials of channel c.
static int stem_fold_desc(const mvg_conv_desc *d, mvg_conv_desc *rw) {
  MVG_REQUIRE(d != nullptr, "stem (folded windows): null descriptor");
  MVG_REQUIRE(d->r == 7 && d->s == 7 && d->stride == 2 && d->pad == 3, "stem (folded windows): 7x7 stride 2 pad 3");
  MVG_REQUIRE(d->w % 4 == 0 && d->ho == (d->h - 1) / 2 + 1 && d->wo == d->w / 2, "stem (folded windows): width %% 4; ho, wo inconsistent");
  MVG_REQUIRE(d->cout % 32 == 0 && d->groups > 0 && d->n > 0, "stem (folded windows): cout must be a multiple of 32");
  MVG_REQUIRE(((long long)d->n * d->ho * (d->wo / 2)) % 64 == 0, "stem (folded windows): n * ho * wo / 2 must be a multiple of 64 (BatchNorm partials)");
  *rw = *d;
  rw->w = d->w / 4;
  rw->wo = d->wo / 2;
  rw->cin = 64;
  rw->cout = 2 * d->cout;
  rw->s = 1;
  return 0;
}

int mvg_stem_rowwindow_bf16(const float *x_nchw, void *xw, int64_t images, int h, int w, void *stream) {
  MVG_REQUIRE(x_nchw && xw && images > 0 && h > 0 && w > 0 && w % 4 == 0, "stem_rowwindow_bf16: bad arguments (width %% 4)");
  hipStream_t st = (hipStream_t)stream;
  const long long n = images * h * (w / 4) * 8;
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, 12.0 * (double)images * h * w + 16.0 * (double)n);
  long long blocks = (n + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(stem_rowwindow_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x_nchw, (uint4 *)xw, n, h, w);
  return check_launch("stem_rowwindow_bf16");
}

int mvg_stem_fprop_bf16(const mvg_conv_desc *d, const void *xw, const void *w_fold, void *y, float *stats, void *stream) {
  mvg_conv_desc rw;
  if (stem_fold_desc(d, &rw)) return 2;
  return fprop_bf16_impl(&rw, xw, w_fold, y, nullptr, 0, stats, stream, false, 1, 0);
}

static mvg_conv_desc linear_desc_bf16(int rows, int fin, int fout) {
  mvg_conv_desc d = {1, rows, 1, 1, fin, fout, 1, 1, 1, 0, 1, 1};
  return d;
}

int mvg_linear_fprop_mixed(const float *x, const void *w_bf16, const float *bias, int relu, float *y, int rows, int fin, int fout,
                           void *stream) {
  const mvg_conv_desc d = linear_desc_bf16(rows, fin, fout);
  return fprop_bf16_impl(&d, x, w_bf16, y, bias, relu, nullptr, stream, true);
}

int mvg_linear_dgrad_mixed(const float *dy, const void *wt_bf16, const float *mask, const float *addend, float *dx, int rows,
                           int fin, int fout, void *stream) {
  const mvg_conv_desc d = linear_desc_bf16(rows, fin, fout);
  return dgrad_bf16_impl(&d, dy, wt_bf16, dx, mask, addend, stream, true);
}

static void wgrad_bf16_tile(const mvg_conv_desc *d, int &bm, int &bn) {
  const int ncols = d->r * d->s * d->cin;
  bm = d->cout >= 128 ? 128 : 64;
  bn = ncols >= 128 ? 128 : 64;
}

// incremental pixel stepping of the bf16-operand loader: at most one image wrap per 64-pixel step (the fp32-operand form
// decodes every step)
static bool wgrad_bf16_incremental(const mvg_conv_desc *d) { return (long long)d->ho * d->wo >= 128; }

// The pixel splits of a checked descriptor (the stem's folded one included) at its tile.
static int wgrad_bf16_splits(const mvg_conv_desc *d) {
  int bm, bn;
  wgrad_bf16_tile(d, bm, bn);
  // one resident round at two workgroups per CU, at least 512 pixels (8 K-steps) per split
  return wgrad_split_count(wgrad_tiles(d, bm, bn), (long long)d->groups * d->n * d->ho * d->wo, 2, 512);
}

int mvg_conv_wgrad_splits_bf16(const mvg_conv_desc *d) {
  if (validate_bf16(d)) return -1;
  return wgrad_bf16_splits(d);
}

static int wgrad_bf16_impl(const mvg_conv_desc *d, const void *x, const void *dy, float *dw, float *db, float *workspace,
                           int splits, int accumulate, void *stream, bool f32in, int stride_w = -1, int pad_w = -1, bool slabs_only = false) {
  if (stride_w < 0 && validate_bf16(d)) return 2;
  MVG_REQUIRE(!db || f32in, "wgrad_bf16: the bias gradient rides on the fp32-operand form only");
  WgradParams p;
  memset(&p, 0, sizeof(p));
  p.x = (const float *)x;
  p.dy = (const float *)dy;
  int bm, bn;
  wgrad_bf16_tile(d, bm, bn);
  const double pixels = (double)d->groups * d->n * d->ho * d->wo;
  const double acin = d->cin == 8 && d->r == 7 ? 3.0 : (double)d->cin;
  const double flops = 2.0 * pixels * d->cout * d->r * d->s * acin * (stride_w >= 0 ? 147.0 / 448.0 : 1.0);
  const double bytes = 2.0 * ((double)d->groups * d->n * d->h * d->w * acin + pixels * d->cout) + 4.0 * (double)d->cout * d->r * d->s * acin;
  const bool incr = wgrad_bf16_incremental(d);
  const auto dispatch = [&](dim3 grid, dim3 block, hipStream_t st, const WgradParams &wp) {
#define MVG_WGRAD_BF16(BM_, BN_)                                                                          \
  do {                                                                                                    \
    if (f32in) hipLaunchKernelGGL((wgrad_bf16_kernel<BM_, BN_, false, true>), grid, block, 0, st, wp);     \
    else if (incr) hipLaunchKernelGGL((wgrad_bf16_kernel<BM_, BN_, true>), grid, block, 0, st, wp);        \
    else hipLaunchKernelGGL((wgrad_bf16_kernel<BM_, BN_, false>), grid, block, 0, st, wp);                 \
  } while (0)
    if (bm == 128 && bn == 128) MVG_WGRAD_BF16(128, 128);
    else if (bm == 64 && bn == 128) MVG_WGRAD_BF16(64, 128);
    else if (bm == 128 && bn == 64) MVG_WGRAD_BF16(128, 64);
    else MVG_WGRAD_BF16(64, 64);
#undef MVG_WGRAD_BF16
    return 0;
  };
  return wgrad_launch(p, d, f32in ? 4 : 2, 64, bm, bn, dw, db, workspace, splits, accumulate, slabs_only, (hipStream_t)stream, flops, bytes,
                      "wgrad_bf16", "conv_wgrad_bf16", stride_w, pad_w, dispatch);
}

int mvg_conv_wgrad_bf16(const mvg_conv_desc *d, const void *x, const void *dy, float *dw, float *workspace, int splits,
                        int accumulate, void *stream) {
  return wgrad_bf16_impl(d, x, dy, dw, nullptr, workspace, splits, accumulate, stream, false);
}

int mvg_conv_wgrad_bf16_slabs(const mvg_conv_desc *d, const void *x, const void *dy, float *workspace, int splits, void *stream) {
  MVG_REQUIRE(splits > 1 && workspace, "wgrad_bf16_slabs: splits > 1 and a workspace (the slabs ARE the result)");
  return wgrad_bf16_impl(d, x, dy, workspace, nullptr, workspace, splits, 0, stream, false, -1, -1, true);
}

int mvg_stem_wgrad_splits_bf16(const mvg_conv_desc *d) {
  mvg_conv_desc rw;
  if (stem_fold_desc(d, &rw)) return -1;
  // the folded descriptor's own tile, as wgrad_bf16_impl launches it: 7 x 64 columns -> bn = 128; cout a multiple of 32 ->
  // rw.cout a multiple of 64, and the 64-row tile (rw.cout == 64 only) makes one row tile just as a 128-row tile would
  return wgrad_bf16_splits(&rw);
}

int mvg_stem_wgrad_bf16(const mvg_conv_desc *d, const void *xw, const void *dy, float *dw_fold, float *workspace, int splits,
                        int accumulate, void *stream) {
  mvg_conv_desc rw;
  if (stem_fold_desc(d, &rw)) return 2;
  return wgrad_bf16_impl(&rw, xw, dy, dw_fold, nullptr, workspace, splits, accumulate, stream, false, 1, 0);
}

int mvg_linear_wgrad_mixed(const float *x, const float *dy, float *dw, float *db, int rows, int fin, int fout, float *workspace,
                           int splits, int accumulate, void *stream) {
  const mvg_conv_desc d = linear_desc_bf16(rows, fin, fout);
  return wgrad_bf16_impl(&d, x, dy, dw, db, workspace, splits, accumulate, stream, true);
}

int mvg_conv_plan_query_bf16(const mvg_conv_desc *d, int kind, mvg_conv_plan *out) {
  mvg_conv_plan plan;
  memset(&plan, 0, sizeof(plan));
  plan.splitk = 1;
  int rc = 2;
  static float marker;               // a non-null bn_part / scale is what selects the fused-reduce plan / the affine kernels
  if (kind == MVG_PLAN_BF16_FPROP) {
    rc = fprop_bf16_impl(d, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, false, -1, -1, nullptr, &plan);
  } else if (kind == MVG_PLAN_BF16_AFFINE) {
    const Bf16Affine a = {&marker, &marker, nullptr};
    rc = fprop_bf16_impl(d, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, false, -1, -1, &a, &plan);
  } else if (kind == MVG_PLAN_BF16_DGRAD) {
    rc = dgrad_bf16_impl(d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, false, nullptr, &plan);
  } else if (kind == MVG_PLAN_BF16_DGRAD_BNREDUCE) {
    const Bf16BnFuse f = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &marker};
    rc = dgrad_bf16_impl(d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, false, &f, &plan);
  } else if (kind == MVG_PLAN_BF16_LINEAR_FPROP_MIXED) {
    rc = fprop_bf16_impl(d, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, true, -1, -1, nullptr, &plan);
  } else if (kind == MVG_PLAN_BF16_LINEAR_DGRAD_MIXED) {
    rc = dgrad_bf16_impl(d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, true, nullptr, &plan);
  } else {
    set_error("conv_plan_query_bf16: unknown kind %d", kind);
  }
  if (rc) return -1;
  if (out) *out = plan;
  return 0;
}

int mvg_stem_plan_query_bf16(const mvg_conv_desc *d, mvg_conv_plan *fwd, int32_t *wgrad_bm, int32_t *wgrad_bn, int32_t *wgrad_incremental) {
  // what mvg_stem_fprop_bf16 / mvg_stem_wgrad_bf16 run for `d`: the folded descriptor through the forward's own query path
  // (horizontal stride 1 / padding 0) and the weight gradient's tile choice.  Launches nothing.
  mvg_conv_desc rw;
  if (stem_fold_desc(d, &rw)) return -1;
  mvg_conv_plan plan;
  memset(&plan, 0, sizeof(plan));
  if (fprop_bf16_impl(&rw, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, false, 1, 0, nullptr, &plan)) return -1;
  if (fwd) *fwd = plan;
  int tm, tn;
  wgrad_bf16_tile(&rw, tm, tn);
  if (wgrad_bm) *wgrad_bm = tm;
  if (wgrad_bn) *wgrad_bn = tn;
  if (wgrad_incremental) *wgrad_incremental = wgrad_bf16_incremental(&rw) ? 1 : 0;
  return 0;
}

int mvg_conv_wgrad_tile_bf16(const mvg_conv_desc *d, int f32in, int32_t *bm, int32_t *bn, int32_t *incremental) {
  if (validate_bf16(d)) return -1;
  int tm, tn;
  wgrad_bf16_tile(d, tm, tn);
  if (bm) *bm = tm;
  if (bn) *bn = tn;
  if (incremental) *incremental = (!f32in && wgrad_bf16_incremental(d)) ? 1 : 0;
  return 0;
}

}  // extern "C"
