// igemm_split16_kernel, the forward / backward-data GEMM kernel of conv_split.hip (described there).  Included TWICE by that file
// (inside namespace mvg):
//   MVG_SPLIT_RNG 0: igemm_split16_kernel<BN, DGRAD, LIN, WGM, STAGES, AF> - every training and inference launch;
//   MVG_SPLIT_RNG 1: igemm_split16_ranged_kernel<BN, WGM, STAGES> - the guarded inference forward (mvg_conv_fprop_split_affine_ranged):
//                    the DMA-loader forward with the activation range record of the stored sp output in its epilogue (bf16_tile.h:
//                    RNG; the word travels as IgemmParams::out_absmax), kernels of their own so that the other kernels' symbols
//                    and code do not move.  Same tiles, K loops, workgroups per CU and output bits as their unranged twins.
// One source for both: the K loops cannot drift apart.
#ifndef MVG_SPLIT_RNG
#error "conv_split_igemm.inc: define MVG_SPLIT_RNG (0 or 1) before including"
#endif

#if MVG_SPLIT_RNG
template <int BN, int WGM = 2, int STAGES = 1>
__global__ __launch_bounds__(256, STAGES == 2 ? 2 : WGM == 4 ? 3 : 4) void igemm_split16_ranged_kernel(IgemmParams p) {
  constexpr bool DGRAD = false, LIN = false;
  constexpr AForm AF = A_DMA;
#else
template <int BN, bool DGRAD, bool LIN = false, int WGM = 2, int STAGES = 1, AForm AF = A_DMA>
__global__ __launch_bounds__(256, STAGES == 2 ? 2 : (DGRAD || WGM == 4 || AF != A_DMA) ? 3 : 4) void igemm_split16_kernel(IgemmParams p) {
#endif
  constexpr int BM = 64 * WGM, WGN = 4 / WGM, NW = 4;
  static_assert(WGM == 2 || (WGM == 4 && BN == 64), "tiles: 128 x BN (2 x 2 waves) or 256 x 64 (4 x 1)");
  static_assert(STAGES == 1 || STAGES == 2, "one LDS stage, or the two-stage pipeline");
  static_assert(AF == A_DMA || (DGRAD == (AF == A_DY) && !LIN && WGM == 2 && STAGES == 1),
                "operand-forming loaders: dy in backward-data, the block output in forward; 128-row tiles, one stage");
  using Former = std::conditional_t<AF == A_DY, DyFormer, OutFormer<AF == A_OUT_AFFINE>>;
  constexpr int WTM = BM / WGM, WTN = BN / WGN;
  constexpr int TM = WTM / 16, TN = WTN / 16;
  constexpr int SLOTS = 4 * SP_NP;                            // 16-byte slots per LDS row (8)
  constexpr int ROWB = 16 * SLOTS, ROWS = BM + BN, STAGE_B = ROWS * ROWB;
  constexpr int NQ = ROWS * SLOTS / 64;                       // DMA wave-instructions per stage (32 / 24)
  constexpr int QA = BM * SLOTS / 64;                         // ... of which the first 16 fill the A rows
  constexpr int A_PER = QA / NW, B_PER = (NQ - QA) / NW;      // per wave: 4 and 4 / 2
  static_assert(QA % NW == 0 && (NQ - QA) % NW == 0, "whole instructions per wave");
  constexpr int EPI_B = bf16_epilogue_bytes<BM, BN, WGM, DGRAD>();          // one wave row (64 tile rows) per staging pass
  constexpr int INFO_OFF = STAGES * STAGE_B > EPI_B ? STAGES * STAGE_B : EPI_B;  // row table behind the stages / the epilogue tile
  constexpr int BNK_OFF = INFO_OFF + BM * 8;                  // the former's per-channel constants: [TABLES][src_c]
  constexpr int SMEM_B = BNK_OFF + (AF != A_DMA ? Former::TABLES : 0) * BNA_MAX_C * 4;
  __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM_B];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WGN, wn = wave % WGN;
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

  // ---- row table: thread r < 128 -> (byte offset of row r's pixel at tap (0,0) channel 0, bit t = tap t in range)
  uint2 *rowinfo = reinterpret_cast<uint2 *>(smem + INFO_OFF);
  if (tid < BM) {
    const long long m = (long long)mtile * BM + tid;
    const bool ok = m < c.rows_per_group;
    const int mm = ok ? (int)m : 0;
    const int img = (int)fdiv((unsigned)mm, c.ohw_div);
    const int rem = mm - img * ohw;
    const int oy = (int)fdiv((unsigned)rem, c.ow_div), ox = rem - oy * c.out_w;
    const int y0 = DGRAD ? oy + c.cls_cy : oy * p.stride - p.pad;
    const int x0 = DGRAD ? ox + c.cls_cx : ox * p.stride_w - p.pad_w;
    const unsigned base = (unsigned)(img * p.src_img_stride * SP_BYTES) + (unsigned)((y0 * p.src_w + x0) * p.src_c) * (unsigned)SP_BYTES;
    unsigned msk = 0;
    for (int t = 0; t < c.ntaps; ++t) {
      const int fr = (int)fdiv((unsigned)t, c.tap_ns_div), fs = t - fr * c.tap_ns;
      const int iy = DGRAD ? y0 - fr : y0 + fr;
      const int ix = DGRAD ? x0 - fs : x0 + fs;
      msk |= (unsigned)(((unsigned)iy < (unsigned)p.src_h) & ((unsigned)ix < (unsigned)p.src_w)) << t;
    }
    rowinfo[tid] = make_uint2(base, ok ? msk : 0u);
  }
  if constexpr (AF != A_DMA) Former::stage(reinterpret_cast<float *>(smem + BNK_OFF), p, g, p.src_c, tid);
  __syncthreads();
  // ---- the instructions this wave issues: Q = wave + 4 i; lane -> linear slot 64 Q + lane -> (row, slot in row);
  // the slot holds source slot j = slot ^ h(row) of the row's 128-byte span (j = 2 cc + pc: the memory order)
  unsigned a_base[A_PER], a_vmask[A_PER], b_base[B_PER];
#pragma unroll
  for (int i = 0; i < A_PER; ++i) {
    const int sl = (wave + NW * i) * 64 + lane;
    const int row = sl / SLOTS, j = (sl % SLOTS) ^ sp_row_swz(row);
    const uint2 ri = rowinfo[row];
    a_base[i] = ri.x + 16u * (unsigned)j;
    a_vmask[i] = ri.y;
  }
#pragma unroll
  for (int i = 0; i < B_PER; ++i) {
    const int sl = (wave + NW * (A_PER + i)) * 64 + lane - BM * SLOTS;
    const int row = sl / SLOTS, j = (sl % SLOTS) ^ sp_row_swz(row);        // h(BM + row) == h(row): BM is a multiple of 8
    const int n = ntile * BN + row;
    b_base[i] = pred_off(((unsigned)n * (unsigned)p.b_row_len) * (unsigned)SP_BYTES + 16u * (unsigned)j, n < p.ncols);
  }
  const __amdgpu_buffer_rsrc_t rs_a =
      make_rsrc(reinterpret_cast<const char *>(p.a) + (long long)g * p.imgs_per_group * p.src_img_stride * SP_BYTES, p.a_group_bytes);
  const __amdgpu_buffer_rsrc_t rs_b = make_rsrc(p.b, p.b_bytes);
  typedef __attribute__((address_space(3))) void *lds_vp;

  auto issue = [&](int kt, int stage_off) {
    int kstart = kt * SP_BK;
    if (c.korder) {
      const int cblk = (int)fdiv((unsigned)kt, c.per_div), rem = kt - cblk * c.ntaps;
      kstart = (rem << p.src_c_shift) + cblk * SP_BK;
    }
    const int ks = __builtin_amdgcn_readfirstlane(kstart);
    const int tap_u = c.ntaps > 1 ? (ks >> p.src_c_shift) : 0;
    const int chb = ks - (tap_u << p.src_c_shift);
    const int fru = (int)fdiv((unsigned)tap_u, c.tap_ns_div), fsu = tap_u - fru * c.tap_ns;
    const int disp = (fru * p.src_w + fsu) * p.src_c;
    const unsigned sdelta = (unsigned)(((DGRAD ? -disp : disp) + chb) * SP_BYTES);
    unsigned kb = (unsigned)ks * (unsigned)SP_BYTES;
    if (DGRAD) {
      const int btap = (c.tap_r0 + p.tap_step * fru) * p.s + c.tap_s0 + p.tap_step * fsu;
      kb = (unsigned)(btap * p.src_c + chb) * (unsigned)SP_BYTES;
    }
    if constexpr (AF == A_DMA) {
#pragma unroll
      for (int i = 0; i < A_PER; ++i) {
        const bool ok = ((a_vmask[i] >> tap_u) & 1u) != 0u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a, (lds_vp)(smem + stage_off + (wave + NW * i) * 1024), 16, (int)pred_off(a_base[i] + sdelta, ok), 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_b, (lds_vp)(smem + stage_off + (wave + NW * (A_PER + i)) * 1024), 16, (int)(b_base[i] + kb), 0, 0, 0);
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

  // fragment addresses: lane -> row (l & 15) of a 16-row tile, chunk cc = l >> 4, piece pc -> slot (2 cc + pc) ^ h(row)
  const int cc_l = lane >> 4;
  int a_off[TM][SP_NP], b_off[TN][SP_NP];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int R = wm * WTM + i * 16 + (lane & 15);
#pragma unroll
    for (int pc = 0; pc < SP_NP; ++pc) a_off[i][pc] = R * ROWB + (((2 * cc_l + pc) ^ sp_row_swz(R)) << 4);
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int R = wn * WTN + j * 16 + (lane & 15);
#pragma unroll
    for (int pc = 0; pc < SP_NP; ++pc) b_off[j][pc] = (BM + R) * ROWB + (((2 * cc_l + pc) ^ sp_row_swz(R)) << 4);
  }

  auto load_frags = [&](const unsigned char *stage, f16x8 (&av)[SP_NP][TM], f16x8 (&bv)[SP_NP][TN]) {
#pragma unroll
    for (int pc = 0; pc < SP_NP; ++pc) {
#pragma unroll
      for (int i = 0; i < TM; ++i) av[pc][i] = *reinterpret_cast<const f16x8 *>(stage + a_off[i][pc]);
#pragma unroll
      for (int j = 0; j < TN; ++j) bv[pc][j] = *reinterpret_cast<const f16x8 *>(stage + b_off[j][pc]);
    }
  };
  // smallest terms first: (a1 b2, a2 b1), a1 b1
  auto products = [&](const f16x8 (&av)[SP_NP][TM], const f16x8 (&bv)[SP_NP][TN]) { SPLIT16_ONE(0, 1) SPLIT16_ONE(1, 0) SPLIT16_ONE(0, 0) };
  if constexpr (AF != A_DMA) {
    // (1x1, stride 1: the GEMM's rows are the formed map's pixels, K-step kt = channels 32 kt .. 32 kt + 31)
    const int C = p.src_c;
    const int a_cc = tid & 3, a_r0 = tid >> 2;
    const long long grow0 = (long long)g * c.rows_per_group;
    Former f(p, grow0, c.rows_per_group, C);
    uint4 *a_out = reinterpret_cast<uint4 *>(const_cast<float *>(p.a)) + grow0 * C / 4;       // 4 bytes per element
    bool a_ok[2];
    unsigned a_goff[2];                                        // byte offset of (row, chunk) in the group's fp32 maps = in its sp maps
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long long m = (long long)mtile * BM + a_r0 + 64 * i;
      a_ok[i] = m < c.rows_per_group;
      a_goff[i] = pred_off((unsigned)m * (unsigned)C * 4u + 32u * (unsigned)a_cc, a_ok[i]);
    }
    auto a_load = [&](int kt) {
#pragma unroll
      for (int i = 0; i < 2; ++i) f.load(i, a_goff[i] + 128u * (unsigned)kt);
    };
    // the next K-step's inputs in flight while this one is multiplied: 32 more live registers, which the 128-column tile
    // (64 accumulators, 64 fragment registers) does not have at three workgroups per CU (168) - it loads at the top instead
    constexpr bool PREFETCH = BN == 64;
    if (PREFETCH) a_load(0);
    for (int kt = 0; kt < KT; ++kt) {
      issue(kt, 0);                                            // the weights: DMA
      if (!PREFETCH) a_load(kt);
      uint4 q[2][SP_NP];
      f.consts(reinterpret_cast<const float *>(smem + BNK_OFF) + kt * SP_BK + a_cc * 8, C);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        float o[8];
        f.form(i, a_ok[i], o);
        split2_chunk(o, q[i][0], q[i][1]);
        const int R = a_r0 + 64 * i;
#pragma unroll
        for (int pc = 0; pc < SP_NP; ++pc)
          *reinterpret_cast<uint4 *>(smem + R * ROWB + (((2 * a_cc + pc) ^ sp_row_swz(R)) << 4)) = q[i][pc];
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (a_ok[i]) {
          const unsigned off = a_goff[i] + 128u * (unsigned)kt;
          uint4 *dst = a_out + (off >> 4);
          dst[0] = q[i][0];
          dst[1] = q[i][1];
          f.store_extra(i, off);
        }
      if (PREFETCH && kt + 1 < KT) a_load(kt + 1);             // in flight while this K-step is multiplied
      {
        f16x8 av[SP_NP][TM], bv[SP_NP][TN];
        load_frags(smem, av, bv);
        products(av, bv);
      }
      __syncthreads();                                         // everyone is done reading before the next K-step is written
    }
  } else if constexpr (STAGES == 1) {
    for (int kt = 0; kt < KT; ++kt) {
      issue(kt, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      {
        f16x8 av[SP_NP][TM], bv[SP_NP][TN];
        load_frags(smem, av, bv);
        products(av, bv);
      }
      __syncthreads();                                         // everyone is done reading before the next DMA lands
    }
  } else {
    // Software pipeline, two levels: two K-steps of DMA in LDS / in flight, and the fragments of K-step kt + 1 read into a second
    // register set while K-step kt's MFMAs run (with one wave per SIMD nothing else overlaps the LDS reads with the matrix
    // pipe).  At the top of K-step kt: wait until K-step kt + 1 has landed (the only group in flight: vmcnt(0)) and this wave's
    // fragment reads of K-step kt are complete (lgkmcnt(0)), barrier - now K-step kt's stage is free for every wave and K-step
    // kt + 2 goes into it.  A bare s_barrier: __syncthreads() carries a fence that the compiler turns into s_waitcnt vmcnt(0)
    // wherever an LDS-DMA is pending, which in the prologue would wait for BOTH stages before the first multiply.  (Three and
    // four stages with counted vmcnt waits - one workgroup per CU - measured the same as two: profiles/r04_lin_kloop_stages_ab.txt.)
    constexpr int G = A_PER + B_PER;                           // DMA instructions per wave and K-step
    if (KT > 0) issue(0, 0);                                   // (KT = 0: a tap-less class of a fused-reduce launch, epilogue only)
    if (KT > 1) {
      issue(1, STAGE_B);
      asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(G) : "memory");     // K-step 0 has landed, K-step 1 is in flight
    } else {
      asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    }
    f16x8 a0[SP_NP][TM], b0[SP_NP][TN], a1[SP_NP][TM], b1[SP_NP][TN];
    load_frags(smem, a0, b0);
    int cur = 0;                                               // byte offset of K-step kt's stage
    auto step = [&](int kt, const f16x8 (&ca)[SP_NP][TM], const f16x8 (&cb)[SP_NP][TN], f16x8 (&na)[SP_NP][TM], f16x8 (&nb)[SP_NP][TN]) {
      if (kt + 1 < KT) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (kt + 2 < KT) issue(kt + 2, cur);
        cur ^= STAGE_B;
        load_frags(smem + cur, na, nb);
      }
      products(ca, cb);
    };
    for (int kt = 0; kt < KT; kt += 2) {
      step(kt, a0, b0, a1, b1);
      if (kt + 1 < KT) step(kt + 1, a1, b1, a0, b0);
    }
    __syncthreads();                                           // the epilogue reuses the stages
  }
#if MVG_SPLIT_RNG
  bf16_epilogue<BM, BN, WGM, DGRAD, true, WGM, true, DGRAD, LIN, WGN, false, true>(p, c, acc, reinterpret_cast<unsigned short *>(smem), tid, g, mtile,
                                                                                     ntile);
#else
  bf16_epilogue<BM, BN, WGM, DGRAD, true, WGM, true, DGRAD, LIN, WGN>(p, c, acc, reinterpret_cast<unsigned short *>(smem), tid, g, mtile, ntile);
#endif
}
