// The forward / backward-data GEMM kernels of conv_bf16.hip.  Included TWICE by that file (inside namespace mvg):
//   MVG_BF16_AFF 0: igemm_bf16_kernel<BN, DGRAD, FASTA, F32IO> and igemm_bf16_dma_kernel<BN, DGRAD, STAGES> - the training kernels,
//                   the fusion block's Linear layers;
//   MVG_BF16_AFF 1: igemm_bf16_affine_kernel<BN> and igemm_bf16_dma_affine_kernel<BN> - the inference forward of the bf16 storage
//                   path (bf16_epilogue's AFF form: BatchNorm on running statistics as a per-channel affine, residual, ReLU,
//                   one rounding), kernels of their own so that the training kernels' symbols and code do not move.
// One source for both: the K loops cannot drift apart.
#ifndef MVG_BF16_AFF
#error "conv_bf16_gemm.inc: define MVG_BF16_AFF (0 or 1) before including"
#endif

// F32IO (the fusion block's Linear layers in the bf16 path): the gathered operand, the output and the epilogue
// operands (mask, addend) are fp32 in memory - only the matrix product runs in bf16: the loader reads 32 bytes
// per 8 k, rounds to bf16 on the way into LDS, the epilogue stores fp32.  The weights are the bf16 copies.
#if MVG_BF16_AFF
template <int BN>
__global__ __launch_bounds__(256, 2) void igemm_bf16_affine_kernel(IgemmParams p) {
  constexpr bool DGRAD = false, FASTA = false, F32IO = false;
#else
template <int BN, bool DGRAD, bool FASTA, bool F32IO = false>
__global__ __launch_bounds__(256, 2) void igemm_bf16_kernel(IgemmParams p) {
#endif
  constexpr bool AFF = MVG_BF16_AFF;
  constexpr int BM = BF_BM, BK = BF_BK, LDK = BF_LDK, WGM = 2, WGN = 2;
  constexpr unsigned EA = F32IO ? 4u : 2u;   // bytes per element of the gathered operand
  constexpr int AL = F32IO ? 2 : 1;          // 16-byte loads per 8 k
  constexpr int WTM = BM / WGM, WTN = BN / WGN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int KV = BK / 8;                 // 16-byte vectors per row
  constexpr int RPP = 256 / KV;              // rows per loader pass
  constexpr int A_PASSES = BM / RPP, B_PASSES = BN / RPP;
  constexpr int A_ELEMS = BM * LDK, B_ELEMS = BN * LDK;
  constexpr int LDO = BN + 4;                // fp32 staging tile of the epilogue
  static_assert(2 * (A_ELEMS + B_ELEMS) * 2 >= bf16_epilogue_bytes<BM, BN, 1, false, AFF>(), "the epilogue tile must fit into the operand buffers");
  __shared__ __attribute__((aligned(16))) unsigned short smem[2 * (A_ELEMS + B_ELEMS)];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN;
  const int li = lane & 31, lh = lane >> 5;
  const int a_kv = tid % KV, a_r0 = tid / KV;
  const int nwg = gridDim.x;
  const int wg_all = p.no_remap ? (int)blockIdx.x : xcd_remap(blockIdx.x, nwg);
  int ci = 0;
  for (int i = 1; i < p.ncls; ++i) ci += wg_all >= p.cls[i].tile0;
  const IgemmClass &c = p.cls[ci];
  const int wg = wg_all - c.tile0;
  const int ntile = wg % p.ntiles;
  const int mt_all = wg / p.ntiles;
  const int g = mt_all / c.mtiles_per_group;
  const int mtile = mt_all - g * c.mtiles_per_group;
  const int KT = c.KT;
  const int ohw = c.out_h * c.out_w;

  // ---- loader state
  unsigned a_img[A_PASSES];
  int a_y0[A_PASSES], a_x0[A_PASSES];
  bool a_ok[A_PASSES];
#pragma unroll
  for (int i = 0; i < A_PASSES; ++i) {
    const long long m = (long long)mtile * BM + a_r0 + i * RPP;
    a_ok[i] = m < c.rows_per_group;
    const int mm = a_ok[i] ? (int)m : 0;
    const int img = (int)fdiv((unsigned)mm, c.ohw_div);
    const int rem = mm - img * ohw;
    const int oy = (int)fdiv((unsigned)rem, c.ow_div), ox = rem - oy * c.out_w;
    if (DGRAD) {
      a_y0[i] = oy + c.cls_cy;
      a_x0[i] = ox + c.cls_cx;
    } else {
      a_y0[i] = oy * p.stride - p.pad;
      a_x0[i] = ox * p.stride_w - p.pad_w;
    }
    a_img[i] = (unsigned)(img * p.src_img_stride) * EA;
  }
  unsigned a_base[A_PASSES], a_vmask[A_PASSES], b_base[B_PASSES];
  bool b_ok[B_PASSES];
#pragma unroll
  for (int i = 0; i < B_PASSES; ++i) {
    const int n = ntile * BN + a_r0 + i * RPP;
    b_ok[i] = n < p.ncols;
    b_base[i] = ((unsigned)n * (unsigned)p.b_row_len + (unsigned)a_kv * 8u) * 2u;
  }
  if (FASTA) {
#pragma unroll
    for (int i = 0; i < A_PASSES; ++i) {
      a_base[i] = a_img[i] + (unsigned)((a_y0[i] * p.src_w + a_x0[i]) * p.src_c) * EA + (unsigned)a_kv * 8u * EA;
      unsigned m = 0;
      for (int t = 0; t < c.ntaps; ++t) {
        const int fr = (int)fdiv((unsigned)t, c.tap_ns_div), fs = t - fr * c.tap_ns;
        const int iy = DGRAD ? a_y0[i] - fr : a_y0[i] + fr;
        const int ix = DGRAD ? a_x0[i] - fs : a_x0[i] + fs;
        m |= (unsigned)(((unsigned)iy < (unsigned)p.src_h) & ((unsigned)ix < (unsigned)p.src_w)) << t;
      }
      a_vmask[i] = a_ok[i] ? m : 0u;
    }
  }
  const __amdgpu_buffer_rsrc_t rs_a =
      make_rsrc(reinterpret_cast<const char *>(p.a) + (long long)g * p.imgs_per_group * p.src_img_stride * EA, p.a_group_bytes);
  const __amdgpu_buffer_rsrc_t rs_b = make_rsrc(p.b, p.b_bytes);

  u32x4 a_reg[A_PASSES][AL], b_reg[B_PASSES];
  auto load_a = [&](int i, unsigned off, bool ok) {
    a_reg[i][0] = __builtin_amdgcn_raw_buffer_load_b128(rs_a, pred_off(off, ok), 0, 0);
    if constexpr (F32IO) a_reg[i][1] = __builtin_amdgcn_raw_buffer_load_b128(rs_a, pred_off(off + 16u, ok), 0, 0);
  };
  auto load_tiles = [&](int kt) {
    // first k of this K-step; korder: (64-channel block, tap) instead of (tap, channel block) so that the
    // taps of a 3x3 filter revisit a pixel's 128-byte line within consecutive K-steps (L2 locality)
    int kstart = kt * BK;
    if (c.korder) {
      const int cblk = (int)fdiv((unsigned)kt, c.per_div), rem = kt - cblk * c.ntaps;
      kstart = (rem << p.src_c_shift) + cblk * BK;
    }
    if constexpr (FASTA) {
      const int ks = __builtin_amdgcn_readfirstlane(kstart);
      const int tap_u = c.ntaps > 1 ? (ks >> p.src_c_shift) : 0;
      const int chb = ks - (tap_u << p.src_c_shift);
      const int fru = (int)fdiv((unsigned)tap_u, c.tap_ns_div), fsu = tap_u - fru * c.tap_ns;
      const int disp = (fru * p.src_w + fsu) * p.src_c;
      const unsigned sdelta = (unsigned)((DGRAD ? -disp : disp) + chb) * EA;
      const bool kok_u = (kt < KT) & (ks < c.ktotal);
#pragma unroll
      for (int i = 0; i < A_PASSES; ++i) {
        const bool ok = kok_u & (((a_vmask[i] >> tap_u) & 1u) != 0u);
        load_a(i, a_base[i] + sdelta, ok);
      }
      unsigned kb = (unsigned)ks * 2u;
      if (DGRAD) {
        const int btap = (c.tap_r0 + p.tap_step * fru) * p.s + c.tap_s0 + p.tap_step * fsu;
        kb = (unsigned)(btap * p.src_c + chb) * 2u;
      }
#pragma unroll
      for (int i = 0; i < B_PASSES; ++i)
        b_reg[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_b, pred_off(b_base[i] + kb, b_ok[i] & kok_u), 0, 0);
      return;
    }
    const int k0 = kstart + a_kv * 8;
    int tap = 0, ch = k0;
    if (c.ntaps > 1) {
      tap = k0 >> p.src_c_shift;
      ch = k0 - (tap << p.src_c_shift);
    }
    const int fr = (int)fdiv((unsigned)tap, c.tap_ns_div), fs = tap - fr * c.tap_ns;
    const bool kok = (kt < KT) & (k0 < c.ktotal);
#pragma unroll
    for (int i = 0; i < A_PASSES; ++i) {
      const int iy = DGRAD ? a_y0[i] - fr : a_y0[i] + fr;
      const int ix = DGRAD ? a_x0[i] - fs : a_x0[i] + fs;
      const bool ok = a_ok[i] & kok & ((unsigned)iy < (unsigned)p.src_h) & ((unsigned)ix < (unsigned)p.src_w);
      load_a(i, a_img[i] + (unsigned)((iy * p.src_w + ix) * p.src_c + ch) * EA, ok);
    }
    unsigned koff = (unsigned)k0;
    if (DGRAD) {
      const int btap = (c.tap_r0 + p.tap_step * fr) * p.s + c.tap_s0 + p.tap_step * fs;
      koff = (unsigned)(btap * p.src_c + ch);
    }
#pragma unroll
    for (int i = 0; i < B_PASSES; ++i)
      b_reg[i] = __builtin_amdgcn_raw_buffer_load_b128(
          rs_b, pred_off(b_base[i] - (unsigned)a_kv * 16u + koff * 2u, b_ok[i] & kok), 0, 0);
  };
  auto store_tiles = [&](int buf) {
    unsigned short *As = smem + buf * (A_ELEMS + B_ELEMS);
    unsigned short *Bs = As + A_ELEMS;
#pragma unroll
    for (int i = 0; i < A_PASSES; ++i) {
      u32x4 v = a_reg[i][0];
      if constexpr (F32IO) {          // 8 fp32 -> 8 bf16 (round to nearest even)
        const u32x4 lo = a_reg[i][0], hi = a_reg[i][1];
        v.x = pack_bf2(__uint_as_float(lo.x), __uint_as_float(lo.y));
        v.y = pack_bf2(__uint_as_float(lo.z), __uint_as_float(lo.w));
        v.z = pack_bf2(__uint_as_float(hi.x), __uint_as_float(hi.y));
        v.w = pack_bf2(__uint_as_float(hi.z), __uint_as_float(hi.w));
      }
      *reinterpret_cast<u32x4 *>(As + (a_r0 + i * RPP) * LDK + a_kv * 8) = v;
    }
#pragma unroll
    for (int i = 0; i < B_PASSES; ++i) *reinterpret_cast<u32x4 *>(Bs + (a_r0 + i * RPP) * LDK + a_kv * 8) = b_reg[i];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

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
    bf16x8 av[2][TM], bv[2][TN];
    auto load_frags = [&](int kg, int slot) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
        av[slot][i] = *reinterpret_cast<const bf16x8 *>(As + (wm * WTM + i * 32 + li) * LDK + kg * 16 + lh * 8);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        bv[slot][j] = *reinterpret_cast<const bf16x8 *>(Bs + (wn * WTN + j * 32 + li) * LDK + kg * 16 + lh * 8);
    };
    load_frags(0, 0);
#pragma unroll
    for (int kg = 0; kg < BK / 16; ++kg) {
      if (kg + 1 < BK / 16) load_frags(kg + 1, (kg + 1) & 1);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[kg & 1][i], bv[kg & 1][j], acc[i][j], 0, 0, 0);
    }
    {
      constexpr int NLOADS = A_PASSES * AL + B_PASSES;
      constexpr int NMFMA = TM * TN * (BK / 16);
      constexpr int PER = NMFMA / NLOADS > 0 ? NMFMA / NLOADS : 1;
#pragma unroll
      for (int l = 0; l < NLOADS; ++l) {
        __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
    }
    __syncthreads();
  }

  // ---- epilogue -------------------------------------------------------------------------------
  bf16_epilogue<BF_BM, BN, 2, DGRAD, F32IO, 1, false, false, false, 2, AFF>(p, c, acc, smem, tid, g, mtile, ntile);
}

// ------------------------------------------------------------------------------------------
// LDS-DMA form of the same GEMM (uniform-tap shapes, bf16 operands): the loader is `buffer_load_dwordx4 ... lds`
// - global memory straight into LDS, no staging registers, no ds_write (a ds_write_b128 costs ~13 LDS cycles
// per wave-instruction: eight of them per thread and K-step held the register-staged kernel's LDS pipe busier
// than its matrix pipe).  The DMA writes lane l of a wave-instruction at base + 16*l, so the image is
// lane-linear: unpadded 128-byte rows, eight rows per wave-instruction, and the bank spread comes from the
// SOURCE side (cdna_hip_programming.md 5): the lane that fills 16-byte slot p of row r fetches chunk
// p ^ ((r >> 1) & 7) of that row's K-step, and a fragment read of chunk cc goes to slot cc ^ ((r >> 1) & 7):
// the 16 rows of a ds_read_b128 lane group then cover 16 different 16-byte bank slots (rows r and r + 1
// differ in the 128-byte half, the XOR spreads the other eight).  Out-of-range taps / rows / columns use the
// descriptor's range check: the DMA writes zeros.  Two LDS buffers, the next K-step's DMA is issued before
// this K-step's MFMAs; vmcnt(0) + barrier per K-step, two workgroups per CU cover each other's waits.
// ------------------------------------------------------------------------------------------
// STAGES = 1 (short K: a tile is a few K-steps between a cold prologue and the epilogue): one 32 KB stage, the
// epilogue staged in two passes (34 KB), four workgroups per CU that cover each other's DMA waits and epilogues.
#if MVG_BF16_AFF
template <int BN>
__global__ __launch_bounds__(256, 4) void igemm_bf16_dma_affine_kernel(IgemmParams p) {
  constexpr bool DGRAD = false;
  constexpr int STAGES = 1;
#else
template <int BN, bool DGRAD, int STAGES = 2>
__global__ __launch_bounds__(256, STAGES == 1 ? 4 : 2) void igemm_bf16_dma_kernel(IgemmParams p) {
#endif
  constexpr bool AFF = MVG_BF16_AFF;
  constexpr int BM = BF_BM, BK = BF_BK, WGM = 2, WGN = 2;
  constexpr int WTM = BM / WGM, WTN = BN / WGN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int ROW = BK;                     // elements per (unpadded) LDS row = 128 bytes
  constexpr int A_PASSES = BM / 32, B_PASSES = BN / 32;      // 32 rows (8 rows x 4 waves) per pass
  constexpr int A_ELEMS = BM * ROW, B_ELEMS = BN * ROW;
  constexpr int OP_ELEMS = STAGES * (A_ELEMS + B_ELEMS);      // ushort
  constexpr int EPI_PASSES = STAGES == 1 ? 2 : 1;
  constexpr int EPI_ELEMS = bf16_epilogue_bytes<BM, BN, EPI_PASSES, DGRAD, AFF>() / 2;
  constexpr int SMEM = OP_ELEMS > EPI_ELEMS ? OP_ELEMS : EPI_ELEMS;
  __shared__ __attribute__((aligned(16))) unsigned short smem[SMEM];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WGN, wn = wave % WGN;
  const int li = lane & 31, lh = lane >> 5;
  const int nwg = gridDim.x;
  const int wg_all = p.no_remap ? (int)blockIdx.x : xcd_remap(blockIdx.x, nwg);
  int ci = 0;
  for (int i = 1; i < p.ncls; ++i) ci += wg_all >= p.cls[i].tile0;
  const IgemmClass &c = p.cls[ci];
  const int wg = wg_all - c.tile0;
  const int ntile = wg % p.ntiles;
  const int mt_all = wg / p.ntiles;
  const int g = mt_all / c.mtiles_per_group;
  const int mtile = mt_all - g * c.mtiles_per_group;
  const int KT = c.KT;
  const int ohw = c.out_h * c.out_w;

  // this lane fills slot (tid & 7) of row (tid >> 3) of every 32-row pass with source chunk a_kv
  const int r_in_pass = tid >> 3;
  const int a_kv = (tid & 7) ^ ((tid >> 4) & 7);              // (row >> 1) & 7 with row = 32 i + (tid >> 3)
  unsigned a_base[A_PASSES], a_vmask[A_PASSES], b_base[B_PASSES];
  bool b_ok[B_PASSES];
#pragma unroll
  for (int i = 0; i < A_PASSES; ++i) {
    const long long m = (long long)mtile * BM + r_in_pass + i * 32;
    const bool ok = m < c.rows_per_group;
    const int mm = ok ? (int)m : 0;
    const int img = (int)fdiv((unsigned)mm, c.ohw_div);
    const int rem = mm - img * ohw;
    const int oy = (int)fdiv((unsigned)rem, c.ow_div), ox = rem - oy * c.out_w;
    const int y0 = DGRAD ? oy + c.cls_cy : oy * p.stride - p.pad;
    const int x0 = DGRAD ? ox + c.cls_cx : ox * p.stride_w - p.pad_w;
    a_base[i] = (unsigned)(img * p.src_img_stride * 2) + (unsigned)((y0 * p.src_w + x0) * p.src_c) * 2u + (unsigned)a_kv * 16u;
    unsigned msk = 0;
    for (int t = 0; t < c.ntaps; ++t) {
      const int fr = (int)fdiv((unsigned)t, c.tap_ns_div), fs = t - fr * c.tap_ns;
      const int iy = DGRAD ? y0 - fr : y0 + fr;
      const int ix = DGRAD ? x0 - fs : x0 + fs;
      msk |= (unsigned)(((unsigned)iy < (unsigned)p.src_h) & ((unsigned)ix < (unsigned)p.src_w)) << t;
    }
    a_vmask[i] = ok ? msk : 0u;
  }
#pragma unroll
  for (int i = 0; i < B_PASSES; ++i) {
    const int n = ntile * BN + r_in_pass + i * 32;
    b_ok[i] = n < p.ncols;
    b_base[i] = ((unsigned)n * (unsigned)p.b_row_len + (unsigned)a_kv * 8u) * 2u;
  }
  const __amdgpu_buffer_rsrc_t rs_a =
      make_rsrc(reinterpret_cast<const unsigned short *>(p.a) + (long long)g * p.imgs_per_group * p.src_img_stride, p.a_group_bytes);
  const __amdgpu_buffer_rsrc_t rs_b = make_rsrc(p.b, p.b_bytes);
  typedef __attribute__((address_space(3))) void *lds_vp;

  auto issue = [&](int kt, int buf) {
    int kstart = kt * BK;
    if (c.korder) {
      const int cblk = (int)fdiv((unsigned)kt, c.per_div), rem = kt - cblk * c.ntaps;
      kstart = (rem << p.src_c_shift) + cblk * BK;
    }
    const int ks = __builtin_amdgcn_readfirstlane(kstart);
    const int tap_u = c.ntaps > 1 ? (ks >> p.src_c_shift) : 0;
    const int chb = ks - (tap_u << p.src_c_shift);
    const int fru = (int)fdiv((unsigned)tap_u, c.tap_ns_div), fsu = tap_u - fru * c.tap_ns;
    const int disp = (fru * p.src_w + fsu) * p.src_c;
    const unsigned sdelta = (unsigned)(((DGRAD ? -disp : disp) + chb) * 2);
    unsigned kb = (unsigned)ks * 2u;
    if (DGRAD) {
      const int btap = (c.tap_r0 + p.tap_step * fru) * p.s + c.tap_s0 + p.tap_step * fsu;
      kb = (unsigned)(btap * p.src_c + chb) * 2u;
    }
    unsigned short *As = smem + buf * (A_ELEMS + B_ELEMS) + wave * 8 * ROW;       // this wave's 8 rows of pass 0 (wave-uniform)
    unsigned short *Bs = smem + buf * (A_ELEMS + B_ELEMS) + A_ELEMS + wave * 8 * ROW;
#pragma unroll
    for (int i = 0; i < A_PASSES; ++i) {
      const bool ok = ((a_vmask[i] >> tap_u) & 1u) != 0u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a, (lds_vp)(As + i * 32 * ROW), 16, (int)pred_off(a_base[i] + sdelta, ok), 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < B_PASSES; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_b, (lds_vp)(Bs + i * 32 * ROW), 16, (int)pred_off(b_base[i] + kb, b_ok[i]), 0, 0, 0);
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // fragment addresses: row R, chunk cc = 2 kg + lh -> slot cc ^ ((R >> 1) & 7)
  int a_row[TM], b_row[TN], a_sw[TM], b_sw[TN];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    a_row[i] = (wm * WTM + i * 32 + li) * ROW;
    a_sw[i] = ((wm * WTM + i * 32 + li) >> 1) & 7;
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    b_row[j] = (wn * WTN + j * 32 + li) * ROW;
    b_sw[j] = ((wn * WTN + j * 32 + li) >> 1) & 7;
  }

  if constexpr (STAGES == 2) {
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  for (int kt = 0; kt < KT; ++kt) {
    const int cur = STAGES == 2 ? (kt & 1) : 0;
    if constexpr (STAGES == 2) {
      if (kt + 1 < KT) issue(kt + 1, cur ^ 1);
    } else {
      issue(kt, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    const unsigned short *As = smem + cur * (A_ELEMS + B_ELEMS);
    const unsigned short *Bs = As + A_ELEMS;
#pragma unroll
    for (int kg = 0; kg < BK / 16; ++kg) {
      bf16x8 av[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) av[i] = *reinterpret_cast<const bf16x8 *>(As + a_row[i] + (((2 * kg + lh) ^ a_sw[i]) << 3));
#pragma unroll
      for (int j = 0; j < TN; ++j) bv[j] = *reinterpret_cast<const bf16x8 *>(Bs + b_row[j] + (((2 * kg + lh) ^ b_sw[j]) << 3));
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
    if constexpr (STAGES == 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the next K-step's DMA has landed
    __syncthreads();                                         // ... for every wave, and everyone is done reading `cur`
  }
  bf16_epilogue<BF_BM, BN, 2, DGRAD, false, EPI_PASSES, false, DGRAD, false, 2, AFF>(p, c, acc, smem, tid, g, mtile, ntile);
}
