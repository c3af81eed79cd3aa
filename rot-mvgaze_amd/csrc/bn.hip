// BatchNorm2d (train + eval) forward / backward around the conv kernels.  All HBM-bound passes:
// float4 accesses, channel index carried incrementally (no per-element division).
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "elem.h"
#include "bn_math.h"

namespace mvg {

// ---- finalize: merge the conv epilogue's per-wave partials (sum, centred sumsq) -------------
// Chan's merge needs the between-partials term  sum_p s_p^2 / cnt_p - S^2 / n.  Taken of the raw sums it subtracts two numbers
// of size n mean^2: float64 keeps 2^-53 of THAT, and a channel with mean^2 >> var + eps (a constant channel at 1e3: variance
// noise of 1e-5 eps) gets a wrong invstd.  So every kernel below sums d_p = s_p - cnt_p * pivot instead, pivot = the mean of
// the group's first partial: the same identity (it holds for any shift), both terms now of the size of the variance itself.
__device__ __forceinline__ double bn_merge_pivot(const float *__restrict__ st, int ch, long long rows, int rows_per_partial) {
  return (double)st[ch] / (double)(rows < rows_per_partial ? rows : (long long)rows_per_partial);
}

// One lane's share of a group's partials - lane pl takes every 128th - as the pivoted sums every merge kernel reduces:
// s = sum (s_p - cnt_p pivot), q = sum q_p, ss = sum (s_p - cnt_p pivot)^2 / cnt_p.  (bn_finalize_kernel, bn_finalize_group_kernel and
// bn_frozen_finalize_kernel call this: one statement of the merge.)
__device__ __forceinline__ void bn_merge_lane(const float *__restrict__ st, int ch, int c, int pl, int partials, int rows_per_partial,
                                              long long rows, double pivot, double &s, double &q, double &ss) {
  const double inv_full = 1.0 / (double)rows_per_partial;
  // branch-free body (no early exit) so that the loads of several iterations are in flight at once
  const int valid = (int)((rows + rows_per_partial - 1) / rows_per_partial) < partials
                        ? (int)((rows + rows_per_partial - 1) / rows_per_partial) : partials;
  const double full_pivot = (double)rows_per_partial * pivot;
#pragma unroll 4
  for (int p = pl; p < valid; p += 128) {
    const float sp_f = st[((long long)p * 2) * c + ch];
    const float qp_f = st[((long long)p * 2 + 1) * c + ch];
    const double sp = (double)sp_f - full_pivot, qp = qp_f;
    s += sp;
    q += qp;
    ss += sp * sp;
  }
  ss *= inv_full;
  // the ragged last partial was taken as a full one above (pivot and 1/rows_per_partial): correct it to its count
  const long long last_cnt = rows - (long long)(valid - 1) * rows_per_partial;
  if (valid > 0 && last_cnt < rows_per_partial && ((valid - 1) & 127) == pl) {
    const double raw = st[((long long)(valid - 1) * 2) * c + ch];
    const double was = raw - full_pivot, sp = raw - (double)last_cnt * pivot;
    s += sp - was;
    ss += sp * sp / (double)last_cnt - was * was * inv_full;
  }
}

// grid = c/8 blocks, 1024 threads = 8 channels x 128 partial-lanes.  Every group (= view) is merged
// by the same workgroup, one after the other, so that the running statistics are updated in group
// order (the reference runs the backbone on view 0, then view 1: models/rot_mv.py:204-205).
__global__ __launch_bounds__(1024) void bn_finalize_kernel(const float *__restrict__ stats,
                                                           const double *__restrict__ sliced, int slices, int groups,
                                                           int partials, int rows_per_partial, long long rows, int c,
                                                           const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, float *running_mean,
                                                           float *running_var, float momentum, float eps,
                                                           float *mean_out, float *invstd_out, float *scale,
                                                           float *shift) {
  __shared__ double sh[3][128][8];
  const int cl = threadIdx.x & 7, pl = threadIdx.x >> 3;
  const int ch = blockIdx.x * 8 + cl;
  float rm = 0.f, rv = 0.f;
  if (pl == 0 && ch < c) {
    if (running_mean) rm = running_mean[ch];
    if (running_var) rv = running_var[ch];
  }
  for (int g = 0; g < groups; ++g) {
    const float *st = stats + (long long)g * partials * 2 * c;
    double s = 0.0, q = 0.0, ss = 0.0;
    const double pivot = ch < c ? bn_merge_pivot(st, ch, rows, rows_per_partial) : 0.0;
    if (ch < c && sliced) {
      for (int k = pl; k < slices; k += 128) {
        const double *o = sliced + (((long long)g * slices + k) * 3) * c;
        s += o[ch];
        q += o[c + ch];
        ss += o[2 * c + ch];
      }
    } else if (ch < c) {
      bn_merge_lane(st, ch, c, pl, partials, rows_per_partial, rows, pivot, s, q, ss);
    }
    // reduce over the 128 partial lanes: lanes 8/16/32 apart inside the wave (shuffles), then the 16
    // waves through LDS - two barriers per group instead of an 8-level LDS tree
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) {
      s += __shfl_xor(s, o, 64);
      q += __shfl_xor(q, o, 64);
      ss += __shfl_xor(ss, o, 64);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) < 8) {
      sh[0][wv][cl] = s;
      sh[1][wv][cl] = q;
      sh[2][wv][cl] = ss;
    }
    __syncthreads();
    if (pl == 0) {
      s = q = ss = 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        s += sh[0][k][cl];
        q += sh[1][k][cl];
        ss += sh[2][k][cl];
      }
      sh[0][0][cl] = s;
      sh[1][0][cl] = q;
      sh[2][0][cl] = ss;
    }
    if (pl == 0 && ch < c) {
      const double n = (double)rows;
      const double dmean = sh[0][0][cl] / n;                             // the sums are of s_p - cnt_p * pivot
      const double mean = pivot + dmean;
      double m2 = sh[1][0][cl] + (sh[2][0][cl] - sh[0][0][cl] * dmean);  // Chan merge of the partials
      if (m2 < 0.0) m2 = 0.0;
      const double var = m2 / n;
      const float invstd = (float)(1.0 / sqrt(var + (double)eps));
      const float fmean = (float)mean;
      const long long o = (long long)g * c + ch;
      mean_out[o] = fmean;
      invstd_out[o] = invstd;
      const float sc = gamma[ch] * invstd;
      scale[o] = sc;
      shift[o] = beta[ch] - fmean * sc;
      rm = (1.f - momentum) * rm + momentum * fmean;
      const float unbiased = (float)(rows > 1 ? m2 / (n - 1.0) : var);
      rv = (1.f - momentum) * rv + momentum * unbiased;
    }
    __syncthreads();
  }
  if (pl == 0 && ch < c) {
    if (running_mean) running_mean[ch] = rm;
    if (running_var) running_var[ch] = rv;
  }
}

// The same merge with one workgroup per (8 channels, GROUP): grid = (c/8, groups).  bn_finalize_kernel walks the groups
// one after the other - eight dependent rounds of loads and barriers per call at V = 8 (26 us per call, 1.4 ms of a C5
// step in 53 calls) - only because the running statistics are updated in group order; here every group's statistics
// are made at once, (mean, unbiased variance) go to `mv` [groups][2][c] in fp64, and bn_running_update_kernel applies
// them to the running statistics in group order.  Same arithmetic, same order inside a group: identical results.
__global__ __launch_bounds__(1024) void bn_finalize_group_kernel(const float *__restrict__ stats, const double *__restrict__ sliced,
                                                                 int slices, int partials, int rows_per_partial, long long rows,
                                                                 int c, const float *__restrict__ gamma,
                                                                 const float *__restrict__ beta, float eps, float *mean_out,
                                                                 float *invstd_out, float *scale, float *shift,
                                                                 double *__restrict__ mv) {
  __shared__ double sh[3][16][8];
  const int cl = threadIdx.x & 7, pl = threadIdx.x >> 3;
  const int ch = blockIdx.x * 8 + cl;
  const int g = blockIdx.y, groups = gridDim.y;
  const float *st = stats + (long long)g * partials * 2 * c;
  double s = 0.0, q = 0.0, ss = 0.0;
  const double pivot = ch < c ? bn_merge_pivot(st, ch, rows, rows_per_partial) : 0.0;
  if (ch < c && sliced) {
    for (int k = pl; k < slices; k += 128) {
      const double *o = sliced + (((long long)g * slices + k) * 3) * c;
      s += o[ch];
      q += o[c + ch];
      ss += o[2 * c + ch];
    }
  } else if (ch < c) {
    bn_merge_lane(st, ch, c, pl, partials, rows_per_partial, rows, pivot, s, q, ss);
  }
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) {
    s += __shfl_xor(s, o, 64);
    q += __shfl_xor(q, o, 64);
    ss += __shfl_xor(ss, o, 64);
  }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) < 8) {
    sh[0][wv][cl] = s;
    sh[1][wv][cl] = q;
    sh[2][wv][cl] = ss;
  }
  __syncthreads();
  if (pl == 0 && ch < c) {
    s = q = ss = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      s += sh[0][k][cl];
      q += sh[1][k][cl];
      ss += sh[2][k][cl];
    }
    const double n = (double)rows;
    const double dmean = s / n;                         // the sums are of s_p - cnt_p * pivot
    const double mean = pivot + dmean;
    double m2 = q + (ss - s * dmean);                  // Chan merge of the partials
    if (m2 < 0.0) m2 = 0.0;
    const double var = m2 / n;
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    const float fmean = (float)mean;
    const long long o = (long long)g * c + ch;
    mean_out[o] = fmean;
    invstd_out[o] = invstd;
    const float sc = gamma[ch] * invstd;
    scale[o] = sc;
    shift[o] = beta[ch] - fmean * sc;
    mv[((long long)g * 2) * c + ch] = (double)fmean;
    mv[((long long)g * 2 + 1) * c + ch] = (double)(float)(rows > 1 ? m2 / (n - 1.0) : var);
  }
  (void)groups;
}

__global__ __launch_bounds__(256) void bn_running_update_kernel(const double *__restrict__ mv, int groups, int c, float momentum,
                                                                float *running_mean, float *running_var) {
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= c) return;
  float rm = running_mean ? running_mean[ch] : 0.f, rv = running_var ? running_var[ch] : 0.f;
  for (int g = 0; g < groups; ++g) {
    rm = (1.f - momentum) * rm + momentum * (float)mv[((long long)g * 2) * c + ch];
    rv = (1.f - momentum) * rv + momentum * (float)mv[((long long)g * 2 + 1) * c + ch];
  }
  if (running_mean) running_mean[ch] = rm;
  if (running_var) running_var[ch] = rv;
}

// ---- frozen BatchNorm on the split path: the unit's constants and its activation scale in ONE launch --------------------
// A unit on the running statistics (a frozen-BatchNorm training step with Backbone.split_frozen) stores its output in sp
// like a trained one, but a z-score bound does not hold for it.  The conv launch's statistics partials give one without a
// pass over the activation: with mean_b, var_b (biased) of a (group, channel)'s n conv outputs, |y - mean_b| <= sqrt((n - 1) var_b), so
//   |gamma invstd_r (y - rm) + beta| <= |gamma| invstd_r (|mean_b - rm| + sqrt((n - 1) var_b)) + |beta|.
// grid = (c/8, groups), bn_finalize_group_kernel's shape and merge (bn_merge_lane: float64, pivoted).  Per (group, channel)
// the lane that holds the merged sums writes scale / shift (bn_eval_affine_ch: mvg_bn_eval_affine's bits), mean := rm and
// invstd := 1 / sqrtf(rv + eps) (the backward's reduce forms read them), and evaluates the bound in float64 times
// FROZEN_BOUND_MARGIN.  ROUNDING MAY ONLY ENLARGE THE BOUND: the merge and the expression are float64; the margin (1 + 2^-7)
// covers what float64 cannot - the fp32 rounding of the partials themselves (sums of <= a row tile's values: relative 2^-17
// or so) - and the two fp32 roundings on the way out (the conversion, the chained sum).  The maximum over (group, channel) is
// an integer atomic max of the float's bits (non-negative: the order of the bits is the order of the values; NaN goes in as
// inf) into state[0]; every workgroup then takes a ticket from state[1], and the last one adds the identity's chained bound,
// writes state[2] and the slot's 2^-k (sp_scale_for_banded: mvg_act_scales' rule).  state[0..1] arrive zeroed.  The running
// statistics are only read.
constexpr double FROZEN_BOUND_MARGIN = 1.0078125;
__global__ __launch_bounds__(1024) void bn_frozen_finalize_kernel(const float *__restrict__ stats, int partials, int rows_per_partial,
                                                                  long long rows, int c, const float *__restrict__ gamma,
                                                                  const float *__restrict__ beta, const float *__restrict__ rmean,
                                                                  const float *__restrict__ rvar, float eps,
                                                                  const float *__restrict__ ident_bound, float *__restrict__ mean_out,
                                                                  float *__restrict__ invstd_out, float *__restrict__ scale,
                                                                  float *__restrict__ shift, unsigned *state, float *slot) {
  __shared__ double sh[3][16][8];
  const int cl = threadIdx.x & 7, pl = threadIdx.x >> 3;
  const int ch = blockIdx.x * 8 + cl;
  const int g = blockIdx.y;
  const float *st = stats + (long long)g * partials * 2 * c;
  double s = 0.0, q = 0.0, ss = 0.0;
  const double pivot = ch < c ? bn_merge_pivot(st, ch, rows, rows_per_partial) : 0.0;
  if (ch < c) bn_merge_lane(st, ch, c, pl, partials, rows_per_partial, rows, pivot, s, q, ss);
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) {
    s += __shfl_xor(s, o, 64);
    q += __shfl_xor(q, o, 64);
    ss += __shfl_xor(ss, o, 64);
  }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) < 8) {
    sh[0][wv][cl] = s;
    sh[1][wv][cl] = q;
    sh[2][wv][cl] = ss;
  }
  __syncthreads();
  if (threadIdx.x < 64) {        // wave 0: lanes 0..7 hold the workgroup's 8 channels (pl == 0), the others carry a zero bound
    float bd = 0.f;
    if (pl == 0 && ch < c) {
      s = q = ss = 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        s += sh[0][k][cl];
        q += sh[1][k][cl];
        ss += sh[2][k][cl];
      }
      const double n = (double)rows;
      const double dmean = s / n;                         // the sums are of s_p - cnt_p * pivot
      const double mean = pivot + dmean;
      double m2 = q + (ss - s * dmean);                  // Chan merge of the partials
      if (m2 < 0.0) m2 = 0.0;
      const float ga = gamma[ch], be = beta[ch], rm = rmean[ch], rv = rvar[ch];
      const long long o = (long long)g * c + ch;
      bn_eval_affine_ch(ga, be, rm, rv, eps, scale[o], shift[o]);
      const float is = 1.f / sqrtf(rv + eps);
      mean_out[o] = rm;
      invstd_out[o] = is;
      // sqrt((n - 1) var_b) = sqrt(m2 (n - 1) / n)
      const double spread = sqrt(m2 * ((n - 1.0) / n));
      const double b = (fabs((double)ga) * (double)is * (fabs(mean - (double)rm) + spread) + fabs((double)be)) * FROZEN_BOUND_MARGIN;
      bd = (float)b;
      if (!(bd <= 3.0e38f)) bd = INFINITY;               // NaN too: it must not rank below a finite bound
    }
    bd = fmaxf(bd, __shfl_xor(bd, 1, 64));
    bd = fmaxf(bd, __shfl_xor(bd, 2, 64));
    bd = fmaxf(bd, __shfl_xor(bd, 4, 64));
    if (threadIdx.x == 0) {
      atomicMax(&state[0], __float_as_uint(bd));
      __threadfence();
      const unsigned ticket = atomicAdd(&state[1], 1u);
      if (ticket == gridDim.x * gridDim.y - 1) {         // every other workgroup's maximum is in: finish the unit
        __threadfence();
        float b = __uint_as_float(atomicMax(&state[0], 0u));
        if (ident_bound) b = __fadd_rn(b, *ident_bound);
        if (!(b <= 3.0e38f)) b = INFINITY;
        reinterpret_cast<float *>(state)[2] = b;
        if (slot) *slot = 1.f / sp_scale_for_banded(b);
      }
    }
  }
}

// Large partial counts (stem at C2: 25 088 per group) first collapse to <= 64 slices per group with
// all CUs busy; bn_finalize_kernel then merges the slices.  slice record: (sum, q, sum of s^2/cnt) of the pivoted s_p - cnt_p * pivot, in
// fp64, [group][slice][3][c].
__global__ __launch_bounds__(256) void bn_partials_slice_kernel(const float *__restrict__ stats, int partials,
                                                                int rows_per_partial, long long rows, int c,
                                                                int per_slice, double *__restrict__ out, int slices) {
  __shared__ double sh[3][32][8];
  const int cl = threadIdx.x & 7, pl = threadIdx.x >> 3;                // 8 channels x 32 partial lanes
  const int ch = blockIdx.x * 8 + cl;
  const int g = blockIdx.z;
  const float *st = stats + (long long)g * partials * 2 * c;
  const int valid = (int)((rows + rows_per_partial - 1) / rows_per_partial) < partials
                        ? (int)((rows + rows_per_partial - 1) / rows_per_partial) : partials;
  const int p0 = blockIdx.y * per_slice;
  const int p1 = p0 + per_slice < valid ? p0 + per_slice : valid;
  double s = 0.0, q = 0.0, ss = 0.0;
  if (ch < c) {
    const double inv_full = 1.0 / (double)rows_per_partial;
    const double pivot = bn_merge_pivot(st, ch, rows, rows_per_partial);      // the finalize kernels form the same one
#pragma unroll 4
    for (int p = p0 + pl; p < p1; p += 32) {
      const double raw = st[((long long)p * 2) * c + ch], qp = st[((long long)p * 2 + 1) * c + ch];
      long long cnt = rows - (long long)p * rows_per_partial;
      if (cnt > rows_per_partial) cnt = rows_per_partial;
      const double sp = raw - (double)cnt * pivot;
      s += sp;
      q += qp;
      ss += sp * sp * (cnt >= rows_per_partial ? inv_full : 1.0 / (double)cnt);
    }
  }
  sh[0][pl][cl] = s;
  sh[1][pl][cl] = q;
  sh[2][pl][cl] = ss;
  __syncthreads();
  if (pl == 0 && ch < c) {
    for (int k = 1; k < 32; ++k) {
      s += sh[0][k][cl];
      q += sh[1][k][cl];
      ss += sh[2][k][cl];
    }
    double *o = out + (((long long)g * slices + blockIdx.y) * 3) * c;
    o[ch] = s;
    o[c + ch] = q;
    o[2 * c + ch] = ss;
  }
}

// ---- every group's statistics AND the running statistics in ONE workgroup per 8 channels -------------------------
// grid = c/8, 1024 threads = 8 channels x 128 lanes, the lanes divided between the groups (views): every (channel,
// group) merges its partials (or slices) with 128 / groups lanes, bn_finalize_group_kernel's arithmetic; the per-group
// (mean, unbiased variance) meet in LDS and one thread per channel applies the running-statistics updates in group
// order.  Replaces bn_finalize_group_kernel + bn_running_update_kernel (two launches per conv + BN unit, 106 per
// ResNet-50 step) without any cross-workgroup hand-off.  (Folding them into last-arriving workgroups of ONE grid was
// measured in round 4 and lost: an agent-scope release per workgroup - an L2 write-back - on grids of thousands of
// workgroups cost 37 us per call, 2.96 ms per C3 step against 1.02.)
__global__ __launch_bounds__(1024) void bn_finalize_allgroups_kernel(const float *__restrict__ stats, const double *__restrict__ sliced,
                                                                     int slices, int groups, int lpg, int partials, int rows_per_partial,
                                                                     long long rows, int c, const float *__restrict__ gamma,
                                                                     const float *__restrict__ beta, float eps, float momentum,
                                                                     float *mean_out, float *invstd_out, float *scale, float *shift,
                                                                     float *running_mean, float *running_var) {
  __shared__ double sh[3][128][8];
  __shared__ float sh_mv[2][8][8];                 // [mean | unbiased variance][group][channel]
  const int cl = threadIdx.x & 7, l = threadIdx.x >> 3;
  const int g = l / lpg, pl = l - g * lpg;
  const int ch = blockIdx.x * 8 + cl;
  double s = 0.0, q = 0.0, ss = 0.0, pivot = 0.0;
  if (ch < c && g < groups) {
    pivot = bn_merge_pivot(stats + (long long)g * partials * 2 * c, ch, rows, rows_per_partial);
    if (sliced) {
      for (int k = pl; k < slices; k += lpg) {
        const double *o = sliced + (((long long)g * slices + k) * 3) * c;
        s += o[ch];
        q += o[c + ch];
        ss += o[2 * c + ch];
      }
    } else {
      const float *st = stats + (long long)g * partials * 2 * c;
      const double inv_full = 1.0 / (double)rows_per_partial;
      const int valid = (int)((rows + rows_per_partial - 1) / rows_per_partial) < partials
                            ? (int)((rows + rows_per_partial - 1) / rows_per_partial) : partials;
#pragma unroll 4
      for (int p = pl; p < valid; p += lpg) {
        const double raw = st[((long long)p * 2) * c + ch], qp = st[((long long)p * 2 + 1) * c + ch];
        long long cnt = rows - (long long)p * rows_per_partial;
        if (cnt > rows_per_partial) cnt = rows_per_partial;
        const double sp = raw - (double)cnt * pivot;
        s += sp;
        q += qp;
        ss += sp * sp * (cnt >= rows_per_partial ? inv_full : 1.0 / (double)cnt);
      }
    }
  }
  sh[0][l][cl] = s;
  sh[1][l][cl] = q;
  sh[2][l][cl] = ss;
  __syncthreads();
  if (pl == 0 && g < groups && ch < c) {
    for (int k = 1; k < lpg; ++k) {                  // fixed order
      s += sh[0][l + k][cl];
      q += sh[1][l + k][cl];
      ss += sh[2][l + k][cl];
    }
    const double n = (double)rows;
    const double dmean = s / n;                         // the sums are of s_p - cnt_p * pivot
    const double mean = pivot + dmean;
    double m2 = q + (ss - s * dmean);                  // Chan merge of the partials
    if (m2 < 0.0) m2 = 0.0;
    const double var = m2 / n;
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    const float fmean = (float)mean;
    const long long o = (long long)g * c + ch;
    mean_out[o] = fmean;
    invstd_out[o] = invstd;
    const float sc = gamma[ch] * invstd;
    scale[o] = sc;
    shift[o] = beta[ch] - fmean * sc;
    sh_mv[0][g][cl] = fmean;
    sh_mv[1][g][cl] = (float)(rows > 1 ? m2 / (n - 1.0) : var);
  }
  __syncthreads();
  if (l == 0 && ch < c && (running_mean || running_var)) {
    float rm = running_mean ? running_mean[ch] : 0.f, rv = running_var ? running_var[ch] : 0.f;
    for (int gg = 0; gg < groups; ++gg) {
      rm = (1.f - momentum) * rm + momentum * sh_mv[0][gg][cl];
      rv = (1.f - momentum) * rv + momentum * sh_mv[1][gg][cl];
    }
    if (running_mean) running_mean[ch] = rm;
    if (running_var) running_var[ch] = rv;
  }
}

__global__ void bn_eval_affine_kernel(int groups, int c, const float *gamma, const float *beta, const float *rm,
                                      const float *rv, float eps, float *scale, float *shift) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= groups * c) return;
  const int ch = i % c;
  bn_eval_affine_ch(gamma[ch], beta[ch], rm[ch], rv[ch], eps, scale[i], shift[i]);
}

// Every BatchNorm of a network folded by ONE launch (the inference session's bind): blockIdx.y = the record, the x
// dimension covers the widest record's channels.  One row per record: eval-mode (scale, shift) do not depend on the group.
struct BnEvalItem {
  const float *gamma, *beta, *rm, *rv;
  float *scale, *shift;
  int32_t c;
  int32_t pad;
};
__global__ __launch_bounds__(256) void bn_eval_affine_batch_kernel(const BnEvalItem *__restrict__ items, float eps) {
  const BnEvalItem it = items[blockIdx.y];
  for (int ch = blockIdx.x * 256 + threadIdx.x; ch < it.c; ch += gridDim.x * 256)
    bn_eval_affine_ch(it.gamma[ch], it.beta[ch], it.rm[ch], it.rv[ch], eps, it.scale[ch], it.shift[ch]);
}

// ---- apply: out = [relu](y*scale + shift [+ residual]) -------------------------------------
// TO / TR: storage of the output and of the residual when they differ from y's (the split path: y fp32 from the conv,
// out in sp for the next conv, residual sp (identity) or fp32 (raw downsample output)); same access width as T.
template <typename T, typename TO = T, typename TR = T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T *__restrict__ y, const float *__restrict__ scale,
                                                       const float *__restrict__ shift,
                                                       const TR *__restrict__ residual,
                                                       const float *__restrict__ res_scale,
                                                       const float *__restrict__ res_shift, int relu,
                                                       TO *__restrict__ out, long long nw_per_group, int cwn, int c,
                                                       unsigned char *__restrict__ relu_bits) {
  typedef Elem<T> E;
  constexpr int W = E::W;                 // float4 groups per 16-byte access (fp32: 1, bf16: 2)
  static_assert(Elem<TO>::W == W && Elem<TR>::W == W, "bn_apply: mixed storage types need the same access width");
  // relu_bits (optional): one byte per 16-byte access, bit k = (element k of the access came out > 0) - the
  // ReLU mask of a residual unit for its backward reduce pass, at 1/16 of the bytes of reading `out` again
  // res_scale / res_shift: the residual is the RAW output of the block's downsample conv and its BatchNorm
  // is applied here (the normalised downsample map is never written: resnet.py:88-93,137-145)
  const float4 *rs4 = res_scale ? reinterpret_cast<const float4 *>(res_scale + (long long)blockIdx.y * c) : nullptr;
  const float4 *rh4 = res_shift ? reinterpret_cast<const float4 *>(res_shift + (long long)blockIdx.y * c) : nullptr;
  const int g = blockIdx.y;
  const float4 *sc4 = reinterpret_cast<const float4 *>(scale + (long long)g * c);
  const float4 *sh4 = reinterpret_cast<const float4 *>(shift + (long long)g * c);
  const long long base = (long long)g * nw_per_group;
  const long long stride = (long long)gridDim.x * 256;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  int cq = (int)(i % cwn);
  const int step = (int)(stride % cwn);
  // a lane keeps its channel group whenever the grid stride is a multiple of the groups per row (every ResNet
  // shape): with bf16 storage (W = 2) the per-channel factors are then loaded once, outside the row loop
  // (C5: bn_bwd_apply 8.0 -> 7.5 ms)
  float4 pa[W], pb[W], pra[W], prb[W];
  auto load_factors = [&]() {
#pragma unroll
    for (int w = 0; w < W; ++w) {
      pa[w] = sc4[cq * W + w];
      pb[w] = sh4[cq * W + w];
      if (rs4) {
        pra[w] = rs4[cq * W + w];
        prb[w] = rh4[cq * W + w];
      }
    }
  };
  load_factors();
  for (; i < nw_per_group; i += stride) {
    if (W == 1 || step != 0) load_factors();      // fp32 (W = 1) measured 3-6 % faster reloading: fewer live registers
    float4 v[W], r[W], o[W];
    E::ldw(y, base + i, v);
    if (residual) Elem<TR>::ldw(residual, base + i, r);
#pragma unroll
    for (int w = 0; w < W; ++w) {
      o[w] = bn_fwd(v[w], pa[w], pb[w]);      // bn_math.h: the backward kernels rebuild the ReLU mask from y with relu_on
      if (residual) acc4(o[w], rs4 ? bn_fwd(r[w], pra[w], prb[w]) : r[w]);
      if (relu) o[w] = relu4(o[w]);
    }
    Elem<TO>::stw(out, base + i, o);
    if (relu_bits) {
      unsigned m = 0;
#pragma unroll
      for (int w = 0; w < W; ++w)
        m |= relu_nibble(o[w]) << (4 * w);
      relu_bits[base + i] = (unsigned char)m;
    }
    cq += step;
    if (cq >= cwn) cq -= cwn;
  }
}

// ---- backward reduce ------------------------------------------------------------------------
// The tail of every reduce-type kernel.  256 lanes = nrl row lanes x cw columns (lane = rl * cw + cl), column group cq
// of the row, valid when cok: the row lanes' sums meet in LDS and row lane 0 folds them in row-lane order - s1 and s2 by
// addition, mx (max |dz|, R == 3 only) by maximum - and stores rows 0 .. prows - 1 of partial record grp * chunks +
// blockIdx.x ([prows][c] floats, row4 float4 per row; the third row times mx_scale).  s1 / s2 / mx: W float4 each.
// (The record's address is formed here, after the barrier, from its ingredients: formed at the call it compiles to
// vector instead of scalar arithmetic.)
template <int R, int W>
__device__ __forceinline__ void bn_reduce_tail(float4 (&sh)[R][256][W], float4 *s1, float4 *s2, float4 *mx, bool cok, int nrl, int cw, int rl,
                                               int cl, int cq, float *partial, int grp, int chunks, int c, int row4, int prows = 2,
                                               float mx_scale = 1.f) {
#pragma unroll
  for (int w = 0; w < W; ++w) {
    sh[0][threadIdx.x][w] = s1[w];
    sh[1][threadIdx.x][w] = s2[w];
    if constexpr (R == 3) sh[2][threadIdx.x][w] = mx[w];
  }
  __syncthreads();
  if (rl == 0 && cok) {
    for (int k = 1; k < nrl; ++k) {
#pragma unroll
      for (int w = 0; w < W; ++w) {
        acc4(s1[w], sh[0][k * cw + cl][w]);
        acc4(s2[w], sh[1][k * cw + cl][w]);
        if constexpr (R == 3) max4(mx[w], sh[2][k * cw + cl][w]);
      }
    }
    float4 *p = reinterpret_cast<float4 *>(partial + (((long long)grp * chunks + blockIdx.x) * prows) * c);
#pragma unroll
    for (int w = 0; w < W; ++w) {
      p[cq * W + w] = s1[w];
      p[row4 + cq * W + w] = s2[w];
      if constexpr (R == 3)
        if (prows == 3) p[2 * row4 + cq * W + w] = mul4(mx[w], mx_scale);
    }
  }
}

// grid = (chunks, column blocks, groups); thread = one float4 column group x one row lane.
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const T *g, const T *__restrict__ act,
                                                            const T *__restrict__ y,
                                                            const float *__restrict__ mean,
                                                            const float *__restrict__ invstd,
                                                            const float *__restrict__ mscale,
                                                            const float *__restrict__ mshift, long long rows,
                                                            long long rows_per_chunk, int c, int cwn, int cw,
                                                            float *__restrict__ partial, int chunks, T *dz_out,
                                                            const unsigned char *__restrict__ relu_bits,
                                                            int prows) {
  // prows: rows per partial - 2 (s1, s2) or 3 (+ max |masked gradient| per channel: mvg_bn_bwd_apply_split's bound)
  typedef Elem<T> E;
  constexpr int W = E::W;                 // float4 groups per 16-byte access; a "column" below is one such access
  __shared__ float4 sh[3][256][W];
  const int grp = blockIdx.z;
  const int rl = threadIdx.x / cw, cl = threadIdx.x % cw;
  const int nrl = 256 / cw;
  const int cq = blockIdx.y * cw + cl;
  const bool cok = cq < cwn;
  float4 s1[W], s2[W], mx[W];
#pragma unroll
  for (int w = 0; w < W; ++w) s1[w] = s2[w] = mx[w] = zero4();
  if (cok) {
    float4 mu[W], is[W], ma[W], mb[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
      mu[w] = reinterpret_cast<const float4 *>(mean + (long long)grp * c)[cq * W + w];
      is[w] = reinterpret_cast<const float4 *>(invstd + (long long)grp * c)[cq * W + w];
      ma[w] = mb[w] = zero4();
      if (mscale) {
        ma[w] = reinterpret_cast<const float4 *>(mscale + (long long)grp * c)[cq * W + w];
        mb[w] = reinterpret_cast<const float4 *>(mshift + (long long)grp * c)[cq * W + w];
      }
    }
    const long long r0 = (long long)blockIdx.x * rows_per_chunk;
    long long r1 = r0 + rows_per_chunk;
    if (r1 > rows) r1 = rows;
    const long long gbase = (long long)grp * rows * cwn;
    // several rows per iteration with independent loads (the trip count is a runtime value, so the
    // compiler keeps a single row in flight otherwise: latency-bound at 2.9 TB/s)
    auto row = [&](long long r, float4 (&a1)[W], float4 (&a2)[W]) {
      const long long off = gbase + r * cwn + cq;
      float4 d[W], v[W], a[W];
      E::ldw(g, off, d);
      E::ldw(y, off, v);
      if (act) E::ldw(act, off, a);
      const unsigned mb8 = relu_bits ? (unsigned)relu_bits[off] : 0u;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        if (relu_bits) d[w] = mask_bits4(d[w], mb8 >> (4 * w));      // the mask bn_apply recorded (bit k of the byte = element k of this access > 0)
        else if (act) d[w] = mask_act4(d[w], a[w]);
        else if (mscale) d[w] = mask_affine4(d[w], v[w], ma[w], mb[w]);   // ReLU without residual (bn_math.h: relu_on)
        max4(mx[w], abs4(d[w]));
        acc4(a1[w], d[w]);
        acc4_xhat(a2[w], d[w], v[w], mu[w], is[w]);
      }
      if (dz_out) E::stw(dz_out, off, d);      // the masked gradient (may alias g): the apply pass then needs no mask
    };
    constexpr int U = W == 1 ? 4 : 2;          // rows in flight per thread (64 bytes of each tensor)
    float4 t1[U - 1][W], t2[U - 1][W];
#pragma unroll
    for (int u = 0; u < U - 1; ++u)
#pragma unroll
      for (int w = 0; w < W; ++w) t1[u][w] = t2[u][w] = zero4();
    long long r = r0 + rl;
    for (; r + (U - 1) * (long long)nrl < r1; r += U * (long long)nrl) {
      row(r, s1, s2);
#pragma unroll
      for (int u = 1; u < U; ++u) row(r + u * (long long)nrl, t1[u - 1], t2[u - 1]);
    }
    for (; r < r1; r += nrl) row(r, s1, s2);
#pragma unroll
    for (int w = 0; w < W; ++w) {
      if constexpr (U == 4) {
        acc4(s1[w], add4(t1[0][w], add4(t1[1][w], t1[2][w])));
        acc4(s2[w], add4(t2[0][w], add4(t2[1][w], t2[2][w])));
      } else {
        acc4(s1[w], t1[0][w]);
        acc4(s2[w], t2[0][w]);
      }
    }
  }
  bn_reduce_tail(sh, s1, s2, mx, cok, nrl, cw, rl, cl, cq, partial, grp, chunks, c, c / 4, prows);
}

// grid = (c/16, groups) blocks, 1024 threads = 16 channels x 64 chunk-lanes: one (view) group per workgroup (a 64-channel
// layer at C3 has 4 x 3136 x 3 x 64 partials: with the groups looped inside ONE workgroup per 16 channels this kernel
// took 30-136 us per call, 1.8 ms per step); bn_bwd_dgamma_kernel then adds the groups in order (reproducible).
__global__ __launch_bounds__(1024) void bn_bwd_finalize_kernel(const float *__restrict__ partial, int groups, int chunks,
                                                               int c, float *s1, float *s2, float *mx,
                                                               const float *__restrict__ raw_mean, const float *__restrict__ raw_invstd) {
  // mx != null: the partials have three rows (s1, s2, max |dz|) and mx [groups][c] receives the maxima
  // raw_mean != null: the second row holds the UNCENTRED sum(dz * y) (the bf16 backward-data epilogue keeps no
  // per-channel constants in registers): s2 = invstd * (sum(dz * y) - mean * s1), evaluated on the fp64 totals
  __shared__ double sh[3][64][16];
  const int prows = mx ? 3 : 2;
  const int cl = threadIdx.x & 15, pl = threadIdx.x >> 4;
  const int ch = blockIdx.x * 16 + cl;
  const int g = blockIdx.y;
  double a = 0.0, b = 0.0, m = 0.0;
  if (ch < c)
    for (int k = pl; k < chunks; k += 64) {
      a += partial[(((long long)g * chunks + k) * prows) * c + ch];
      b += partial[(((long long)g * chunks + k) * prows + 1) * c + ch];
      if (mx) m = fmax(m, (double)partial[(((long long)g * chunks + k) * prows + 2) * c + ch]);
    }
  sh[0][pl][cl] = a;
  sh[1][pl][cl] = b;
  sh[2][pl][cl] = m;
  __syncthreads();
  for (int o = 32; o > 0; o >>= 1) {
    if (pl < o) {
      sh[0][pl][cl] += sh[0][pl + o][cl];
      sh[1][pl][cl] += sh[1][pl + o][cl];
      sh[2][pl][cl] = fmax(sh[2][pl][cl], sh[2][pl + o][cl]);
    }
    __syncthreads();
  }
  if (pl == 0 && ch < c) {
    s1[(long long)g * c + ch] = (float)sh[0][0][cl];
    double t2 = sh[1][0][cl];
    if (raw_mean) t2 = (double)raw_invstd[(long long)g * c + ch] * (t2 - (double)raw_mean[(long long)g * c + ch] * sh[0][0][cl]);
    s2[(long long)g * c + ch] = (float)t2;
    if (mx) mx[(long long)g * c + ch] = (float)sh[2][0][cl];
  }
}

// dgamma (+)= sum over the groups of s2, dbeta (+)= ... of s1, in group order
__global__ __launch_bounds__(256) void bn_bwd_dgamma_kernel(const float *__restrict__ s1, const float *__restrict__ s2, int groups, int c,
                                                            float *dgamma, float *dbeta, int accumulate) {
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= c) return;
  double tg = 0.0, tb = 0.0;
  for (int g = 0; g < groups; ++g) {
    tb += (double)s1[(long long)g * c + ch];
    tg += (double)s2[(long long)g * c + ch];
  }
  if (dgamma) dgamma[ch] = (accumulate ? dgamma[ch] : 0.f) + (float)tg;
  if (dbeta) dbeta[ch] = (accumulate ? dbeta[ch] : 0.f) + (float)tb;
}

// bn_bwd_dgamma_kernel and bn_dy_scale_kernel (below) in ONE workgroup: dgamma / dbeta over the groups in group order,
// and the bound that scales the unit's dy (split path) - two 5 us launches per unit became one (53 fewer per step).
__global__ __launch_bounds__(1024) void bn_bwd_dgamma_dyscale_kernel(const float *__restrict__ s1, const float *__restrict__ s2,
                                                                     const float *__restrict__ mx, int groups, int c, float *dgamma,
                                                                     float *dbeta, int accumulate, const float *__restrict__ gamma,
                                                                     const float *__restrict__ invstd, float inv_rows, float sqrt_rows,
                                                                     float *__restrict__ dy_sinv) {
  __shared__ float sh_b[16];
  float bd = 0.f;
  for (int ch = threadIdx.x; ch < c; ch += 1024) {
    double tg = 0.0, tb = 0.0;
    for (int g = 0; g < groups; ++g) {
      const float v1 = s1[(long long)g * c + ch], v2 = s2[(long long)g * c + ch];
      tb += (double)v1;
      tg += (double)v2;
      bd = fmaxf(bd, fabsf(gamma[ch] * invstd[(long long)g * c + ch]) * (mx[(long long)g * c + ch] + fabsf(v1) * inv_rows + sqrt_rows * fabsf(v2) * inv_rows));
    }
    if (dgamma) dgamma[ch] = (accumulate ? dgamma[ch] : 0.f) + (float)tg;
    if (dbeta) dbeta[ch] = (accumulate ? dbeta[ch] : 0.f) + (float)tb;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bd = fmaxf(bd, __shfl_xor(bd, o, 64));
  if ((threadIdx.x & 63) == 0) sh_b[threadIdx.x >> 6] = bd;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 16; ++k) bd = fmaxf(bd, sh_b[k]);
    *dy_sinv = 1.f / sp_scale_for(bd);
  }
}

template <typename T, typename TO = T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T *__restrict__ g, const T *__restrict__ act,
                                                           const T *__restrict__ y,
                                                           const float *__restrict__ mean,
                                                           const float *__restrict__ invstd,
                                                           const float *__restrict__ gamma,
                                                           const float *__restrict__ s1, const float *__restrict__ s2,
                                                           const float *__restrict__ mscale,
                                                           const float *__restrict__ mshift,
                                                           long long nw_per_group, float inv_rows, int cwn, int c,
                                                           TO *__restrict__ dy, T *__restrict__ dz_out) {
  typedef Elem<T> E;
  constexpr int W = E::W;
  static_assert(Elem<TO>::W == W, "bn_bwd_apply: mixed storage types need the same access width");
  const int grp = blockIdx.y;
  const float4 *mu4 = reinterpret_cast<const float4 *>(mean + (long long)grp * c);
  const float4 *is4 = reinterpret_cast<const float4 *>(invstd + (long long)grp * c);
  const float4 *ga4 = reinterpret_cast<const float4 *>(gamma);
  const float4 *a4 = reinterpret_cast<const float4 *>(s1 + (long long)grp * c);
  const float4 *b4 = reinterpret_cast<const float4 *>(s2 + (long long)grp * c);
  const long long base = (long long)grp * nw_per_group;
  const long long stride = (long long)gridDim.x * 256;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  int cq = (int)(i % cwn);
  const int step = (int)(stride % cwn);
  float4 pmu[W], pis[W], pga[W], psa[W], psb[W], pma[W], pmb[W];
  auto load_factors = [&]() {
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const int ci = cq * W + w;
      pmu[w] = mu4[ci];
      pis[w] = is4[ci];
      pga[w] = ga4[ci];
      psa[w] = a4[ci];
      psb[w] = b4[ci];
      if (mscale) {
        pma[w] = reinterpret_cast<const float4 *>(mscale + (long long)grp * c)[ci];
        pmb[w] = reinterpret_cast<const float4 *>(mshift + (long long)grp * c)[ci];
      }
    }
  };
  load_factors();
  for (; i < nw_per_group; i += stride) {
    if (W == 1 || step != 0) load_factors();
    float4 d[W], v[W], a[W], o[W];
    E::ldw(g, base + i, d);
    E::ldw(y, base + i, v);
    if (act) E::ldw(act, base + i, a);
#pragma unroll
    for (int w = 0; w < W; ++w) {
      if (act) d[w] = mask_act4(d[w], a[w]);
      else if (mscale) d[w] = mask_affine4(d[w], v[w], pma[w], pmb[w]);
      o[w] = bn_dy(d[w], v[w], pmu[w], pis[w], pga[w], psa[w], psb[w], inv_rows);
    }
    if (dz_out) E::stw(dz_out, base + i, d);
    Elem<TO>::stw(dy, base + i, o);
    cq += step;
    if (cq >= cwn) cq -= cwn;
  }
}

// ---- split path: the passes that write sp (elem.h), one 8-channel chunk per lane -------------------------------
// (fp32 tensors as two float4 per lane, the sp tensor as the chunk's two 16-byte pieces; the generic kernels
// with Elem<sp_t> move 4 channels per lane as 8-byte accesses and are slower.)  A lane's channel chunk is fixed whenever the grid stride is a multiple of the chunks per row
// (every ResNet shape): the per-channel factors are loaded once, outside the row loop.
struct F8 {
  float v[8];
};
__device__ __forceinline__ F8 ld8(const float *p, long long chunk) {
  const float4 a = reinterpret_cast<const float4 *>(p)[2 * chunk], b = reinterpret_cast<const float4 *>(p)[2 * chunk + 1];
  return F8{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
__device__ __forceinline__ F8 ld8_sp(const sp_t *p, long long chunk) {
  const uint4 *q = reinterpret_cast<const uint4 *>(p) + SP_NP * chunk;
  F8 r;
  merge2_chunk(q[0], q[1], r.v);
  return r;
}
__device__ __forceinline__ void st8_sp(sp_t *p, long long chunk, const F8 &x) {
  uint4 q1, q2;
  split2_chunk(x.v, q1, q2);
  uint4 *q = reinterpret_cast<uint4 *>(p) + SP_NP * chunk;
  q[0] = q1;
  q[1] = q2;
}

template <bool RES_SP>
__global__ __launch_bounds__(256) void bn_apply_sp_kernel(const float *__restrict__ y, const float *__restrict__ scale,
                                                          const float *__restrict__ shift, const void *__restrict__ residual,
                                                          const float *__restrict__ res_scale,
                                                          const float *__restrict__ res_shift, int relu, sp_t *__restrict__ out,
                                                          long long n8_per_group, int c8n, int c,
                                                          unsigned short *__restrict__ relu_bits,
                                                          const float *__restrict__ out_sinv,
                                                          const float *__restrict__ res_sinv) {
  // out is stored times 2^k = 1 / *out_sinv (act_scales_kernel; exact: a power of two), an sp identity comes back times
  // its own 2^-k; null = unscaled.  Multiplying by 1.0f changes no bit: the unscaled entry point is this kernel with nulls.
  // (both uniform: kept in scalar registers, so the row loop holds no more vector registers than the unscaled kernel did)
  const float osc = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(out_sinv ? 1.f / *out_sinv : 1.f)));
  const float rsi = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint((RES_SP && res_sinv) ? *res_sinv : 1.f)));
  const int g = blockIdx.y;
  const long long base = (long long)g * n8_per_group;
  const long long stride = (long long)gridDim.x * 256;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  int cq = (int)(i % c8n);
  const int step = (int)(stride % c8n);
  F8 sc = ld8(scale + (long long)g * c, cq), sh = ld8(shift + (long long)g * c, cq), rs, rh;
  const bool raff = res_scale != nullptr;
  if (raff) {
    rs = ld8(res_scale + (long long)g * c, cq);
    rh = ld8(res_shift + (long long)g * c, cq);
  }
  for (; i < n8_per_group; i += stride) {
    if (step != 0) {                       // (not taken for the ResNet shapes: the stride is a multiple of c8n)
      sc = ld8(scale + (long long)g * c, cq);
      sh = ld8(shift + (long long)g * c, cq);
      if (raff) {
        rs = ld8(res_scale + (long long)g * c, cq);
        rh = ld8(res_shift + (long long)g * c, cq);
      }
    }
    const F8 v = ld8(y, base + i);
    F8 r, o;
    if (residual) r = RES_SP ? ld8_sp(reinterpret_cast<const sp_t *>(residual), base + i) : ld8(reinterpret_cast<const float *>(residual), base + i);
    // (bn_math.h; conv_split.hip's block-output former calls the same function: one launch or two, the same bits)
    const unsigned m = bn_apply_chunk(v.v, sc.v, sh.v, residual != nullptr, r.v, raff, rs.v, rh.v, RES_SP, rsi, relu != 0, osc, o.v);
    st8_sp(out, base + i, o);
    if (relu_bits) relu_bits[base + i] = (unsigned short)m;
    cq += step;
    if (cq >= c8n) cq -= c8n;
  }
}

// ---- the scales of a training step's sp activations, from parameters and shapes alone ---------------------------------
// A unit in training mode writes [relu](gamma xhat + beta [+ identity]) with xhat a z-score of n = B Ho Wo samples, so
// |xhat| <= sqrt(n - 1) whatever eps is, and
//   bound(unit) = max_c (|gamma_c| sqrt(n - 1) + |beta_c|),   bound(block output) = bound(last unit) + bound(identity),
// the identity being the previous block's output (the stem's pooled map: max pool and ReLU do not raise a bound) or the
// downsample BatchNorm's output.  No activation is read: ONE workgroup serves every unit of the step.  A wave takes a
// record's channels (plain multiply and add, fixed order of the maximum: the host can evaluate the same fp32 expression),
// then one lane walks the chain over the blocks in record order and writes slots[slot] = 2^-k (elem.h:
// sp_scale_for_banded; a NaN or infinite parameter makes the bound infinite and the scale 1).
struct ActScaleItem {
  const float *gamma, *beta;
  int32_t c;            // channels
  float sqrt_n1;        // sqrt(n - 1), rounded to fp32 by the host
  int32_t ident;        // record whose chained bound is added (an EARLIER record), or -1
  int32_t slot;         // where 2^-k goes, or -1: the unit writes no sp tensor (a downsample branch)
};
constexpr int ACT_SCALE_MAX_ITEMS = 256;

__global__ __launch_bounds__(1024) void act_scales_kernel(const ActScaleItem *__restrict__ items, int n, float *__restrict__ slots,
                                                          int n_slots) {
  __shared__ float bound[ACT_SCALE_MAX_ITEMS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r = wave; r < n; r += 16) {
    const ActScaleItem it = items[r];
    float b = 0.f;
    for (int ch = lane; ch < it.c; ch += 64) {
      float v = __fadd_rn(__fmul_rn(fabsf(it.gamma[ch]), it.sqrt_n1), fabsf(it.beta[ch]));
      if (!(v <= 3.0e38f)) v = INFINITY;         // NaN too: fmaxf would drop it
      b = fmaxf(b, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b = fmaxf(b, __shfl_xor(b, o, 64));
    if (lane == 0) bound[r] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int r = 0; r < n; ++r) {
      const int id = items[r].ident, slot = items[r].slot;
      float b = bound[r];
      if (id >= 0 && id < r) b = __fadd_rn(b, bound[id]);
      bound[r] = b;
      if (slot >= 0 && slot < n_slots) slots[slot] = 1.f / sp_scale_for_banded(b);
    }
  }
}

// dy is stored times 2^k, k from a bound on |dy| (elem.h: sp_scale_for), per (group, channel) and then the maximum:
//   |dy| = |gamma invstd| |dz - s1/n - xhat s2/n| <= |gamma invstd| (max |dz| + |s1|/n + sqrt(n) |s2|/n)
// (a z-score of n samples is at most sqrt(n - 1)); max |dz| per channel comes from the reduce pass (mx), so a dead or
// low-variance channel - huge invstd, zero gradient - does not inflate the bound.  One workgroup; *dy_sinv = 2^-k.
__global__ __launch_bounds__(1024) void bn_dy_scale_kernel(const float *__restrict__ gamma, const float *__restrict__ invstd,
                                                           const float *__restrict__ s1, const float *__restrict__ s2,
                                                           const float *__restrict__ mx, int groups, int c, float inv_rows,
                                                           float sqrt_rows, float *__restrict__ dy_sinv) {
  __shared__ float sh_b[16];
  float bd = 0.f;
  for (int i = threadIdx.x; i < groups * c; i += 1024)
    bd = fmaxf(bd, fabsf(gamma[i % c] * invstd[i]) * (mx[i] + fabsf(s1[i]) * inv_rows + sqrt_rows * fabsf(s2[i]) * inv_rows));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bd = fmaxf(bd, __shfl_xor(bd, o, 64));
  if ((threadIdx.x & 63) == 0) sh_b[threadIdx.x >> 6] = bd;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 16; ++k) bd = fmaxf(bd, sh_b[k]);
    *dy_sinv = 1.f / sp_scale_for(bd);
  }
}

__global__ __launch_bounds__(256) void bn_bwd_apply_sp_kernel(const float *__restrict__ g, const float *__restrict__ y,
                                                              const float *__restrict__ mean, const float *__restrict__ invstd,
                                                              const float *__restrict__ gamma, const float *__restrict__ s1,
                                                              const float *__restrict__ s2, const float *__restrict__ mscale,
                                                              const float *__restrict__ mshift, long long n8_per_group,
                                                              float inv_rows, int c8n, int c, sp_t *__restrict__ dy,
                                                              const float *__restrict__ dy_sinv) {
  const float dsc = 1.f / *dy_sinv;            // 2^k from bn_dy_scale_kernel (exact: a power of two)
  const int grp = blockIdx.y;
  const long long base = (long long)grp * n8_per_group;
  const long long stride = (long long)gridDim.x * 256;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  int cq = (int)(i % c8n);
  const int step = (int)(stride % c8n);
  const long long gc = (long long)grp * c;
  F8 mu = ld8(mean + gc, cq), is = ld8(invstd + gc, cq), ga = ld8(gamma, cq), sa = ld8(s1 + gc, cq), sb = ld8(s2 + gc, cq), ma, mb;
  if (mscale) {
    ma = ld8(mscale + gc, cq);
    mb = ld8(mshift + gc, cq);
  }
  for (; i < n8_per_group; i += stride) {
    if (step != 0) {
      mu = ld8(mean + gc, cq); is = ld8(invstd + gc, cq); ga = ld8(gamma, cq); sa = ld8(s1 + gc, cq); sb = ld8(s2 + gc, cq);
      if (mscale) {
        ma = ld8(mscale + gc, cq);
        mb = ld8(mshift + gc, cq);
      }
    }
    const F8 d = ld8(g, base + i), v = ld8(y, base + i);
    F8 o;
    // (bn_math.h; conv_split.hip's dy former calls the same function: one launch or two, the same bits)
    bn_dy_chunk(d.v, v.v, mu.v, is.v, ga.v, sa.v, sb.v, inv_rows, dsc, o.v, mscale != nullptr, ma.v, mb.v);
    st8_sp(dy, base + i, o);
    cq += step;
    if (cq >= c8n) cq -= c8n;
  }
}

// The same pass for a unit on the running statistics (frozen BatchNorm, Backbone.split_frozen): dy = sp(gamma invstd dz 2^k), no
// batch sums - invstd [groups][c] is what bn_frozen_finalize_kernel left.  MASKED: the ReLU mask rebuilt from y (mscale / mshift);
// else g is already masked (or the unit has no ReLU) and y is not read at all: 4 bytes in, 4 bytes out per element (the
// train-mode pass moves 12).  The same grid-stride loop: 16-byte accesses, per-channel factors in registers, no LDS.
template <bool MASKED>
__global__ __launch_bounds__(256) void bn_frozen_bwd_apply_sp_kernel(const float *__restrict__ g, const float *__restrict__ y,
                                                                     const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                                     const float *__restrict__ mscale, const float *__restrict__ mshift,
                                                                     long long n8_per_group, int c8n, int c, sp_t *__restrict__ dy,
                                                                     const float *__restrict__ dy_sinv) {
  const float dsc = 1.f / *dy_sinv;            // 2^k from the reduce pass's finalize (exact: a power of two)
  const int grp = blockIdx.y;
  const long long base = (long long)grp * n8_per_group;
  const long long stride = (long long)gridDim.x * 256;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  int cq = (int)(i % c8n);
  const int step = (int)(stride % c8n);
  const long long gc = (long long)grp * c;
  F8 f, ma, mb;
  auto factors = [&]() {
    const F8 is = ld8(invstd + gc, cq), ga = ld8(gamma, cq);
#pragma unroll
    for (int k = 0; k < 8; ++k) f.v[k] = ga.v[k] * is.v[k];
    if (MASKED) {
      ma = ld8(mscale + gc, cq);
      mb = ld8(mshift + gc, cq);
    }
  };
  factors();
  for (; i < n8_per_group; i += stride) {
    if (step != 0) factors();                  // (not taken for the ResNet shapes: the stride is a multiple of c8n)
    const F8 d = ld8(g, base + i);
    F8 v, o;
    if (MASKED) v = ld8(y, base + i);
    bn_frozen_dy_chunk(d.v, v.v, f.v, dsc, o.v, MASKED, ma.v, mb.v);
    st8_sp(dy, base + i, o);
    cq += step;
    if (cq >= c8n) cq -= c8n;
  }
}

// ---- stem tail: BatchNorm + ReLU + MaxPool2d(3,2,1), fused --------------------------------------
// The normalised stem activation (B*V x 112 x 112 x 64 floats, 411 MB at C2) is never written:
// forward reads the conv output once and writes the pooled map + argmax; backward rebuilds the
// gradient of the BN output on the fly (gather over the <= 4 pooling windows a pixel can win) and
// the ReLU mask from y (bn_math.h: relu_on, the forward's own expression).
// grid = (ceil(wo*c4n / 256), images*ho): one thread = one (image, oy, ox, 4 channels), no per-thread
// divisions by runtime values except ox/cq.  First maximum in (kh, kw) scan order (ATen's rule).
template <typename T, typename TO = T>
__global__ __launch_bounds__(256) void bn_relu_maxpool_fwd_kernel(const T *__restrict__ y, const float *__restrict__ scale,
                                                                  const float *__restrict__ shift, TO *__restrict__ pooled,
                                                                  uchar4 *__restrict__ argmax, int n_per_group, int h, int w,
                                                                  int c4n, int ho, int wo, const float *__restrict__ out_sinv) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= wo * c4n) return;
  const int ox = t / c4n, cq = t - ox * c4n;
  const int n = blockIdx.y / ho, oy = blockIdx.y - n * ho;
  const int grp = n / n_per_group;
  const float4 a = reinterpret_cast<const float4 *>(scale)[(long long)grp * c4n + cq];
  const float4 b = reinterpret_cast<const float4 *>(shift)[(long long)grp * c4n + cq];
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
      const float4 v = bn_relu4(Elem<T>::ld4(y, (((long long)n * h + iy) * w + ix) * c4n + cq), a, b);
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
  const long long o = (((long long)n * ho + oy) * wo + ox) * c4n + cq;
  if constexpr (std::is_same<TO, sp_t>::value) {
    // sp: the pooled map times 2^k = 1 / *out_sinv (act_scales_kernel; null = unscaled, and x 1.0f changes no bit)
    if (out_sinv) best = mul4(best, 1.f / *out_sinv);
  }
  Elem<TO>::st4(pooled, o, best);
  argmax[o] = idx;
}

// grid = (chunks, column blocks, groups) and the partial layout of bn_bwd_reduce_kernel.  The sums run
// over POOLED elements: sum_pixels d = sum_windows g_w * mask(winner pixel of w), so every window
// fetches y only at its argmax pixel (one scalar per channel) - a quarter of the elements and a tenth
// of the instructions of the per-pixel gather.  A chunk is a range of pooled lines (image, oy); the
// 256/cw row lanes stride along ox.
template <typename T>
__global__ __launch_bounds__(256) void bn_pool_bwd_reduce_kernel(const T *__restrict__ gp, const uchar4 *__restrict__ am,
                                                                 const T *__restrict__ y, const float *__restrict__ mean,
                                                                 const float *__restrict__ invstd,
                                                                 const float *__restrict__ scale,
                                                                 const float *__restrict__ shift, int lines_per_chunk,
                                                                 int n_per_group, int h, int w, int ho, int wo, int c, int c4n,
                                                                 int cw, float *__restrict__ partial, int chunks, int prows) {
  // prows == 3 (split path): a third partial row bounds max |gradient of a pixel| per channel - 4 x the largest masked
  // window gradient (a pixel wins at most four of the 3x3 stride-2 windows) - for the sp scale of dy
  __shared__ float4 sh[3][256][1];
  const int grp = blockIdx.z;
  const int rl = threadIdx.x / cw, cl = threadIdx.x % cw;
  const int nrl = 256 / cw;
  const int cq = blockIdx.y * cw + cl;
  const bool cok = cq < c4n;
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f}, mxv[4] = {0.f, 0.f, 0.f, 0.f};
  if (cok) {
    const float4 mu4 = reinterpret_cast<const float4 *>(mean + (long long)grp * c)[cq];
    const float4 is4 = reinterpret_cast<const float4 *>(invstd + (long long)grp * c)[cq];
    const float4 sa4 = reinterpret_cast<const float4 *>(scale + (long long)grp * c)[cq];
    const float4 sb4 = reinterpret_cast<const float4 *>(shift + (long long)grp * c)[cq];
    const float mu[4] = {mu4.x, mu4.y, mu4.z, mu4.w}, is[4] = {is4.x, is4.y, is4.z, is4.w};
    const float sa[4] = {sa4.x, sa4.y, sa4.z, sa4.w}, sb[4] = {sb4.x, sb4.y, sb4.z, sb4.w};
    const int lines = n_per_group * ho;
    const int l0 = blockIdx.x * lines_per_chunk;
    const int l1 = l0 + lines_per_chunk < lines ? l0 + lines_per_chunk : lines;
    for (int l = l0; l < l1; ++l) {
      const int img = l / ho, oy = l - img * ho;
      const long long n = (long long)grp * n_per_group + img;
      const long long prow = ((n * ho + oy) * wo) * c4n + cq;
      const T *yimg = y + n * h * w * c + cq * 4;
      for (int ox = rl; ox < wo; ox += nrl) {
        const float4 g4 = Elem<T>::ld4(gp, prow + (long long)ox * c4n);
        const uchar4 k4 = am[prow + (long long)ox * c4n];
        const float g[4] = {g4.x, g4.y, g4.z, g4.w};
        const int k[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int kh = (k[j] * 11) >> 5, kw = k[j] - 3 * kh;          // k / 3, k % 3 for k < 9
          const int iy = 2 * oy - 1 + kh, ix = 2 * ox - 1 + kw;          // the winner is an in-bounds pixel
          const float v = Elem<T>::ld1(yimg, ((long long)iy * w + ix) * c + j);
          const float d = relu_mask(relu_on(v, sa[j], sb[j]), g[j]);
          mxv[j] = fmaxf(mxv[j], fabsf(d));
          s1[j] += d;
          s2[j] += d * xhat(v, mu[j], is[j]);
        }
      }
    }
  }
  float4 t1[1] = {make_float4(s1[0], s1[1], s1[2], s1[3])}, t2[1] = {make_float4(s2[0], s2[1], s2[2], s2[3])};
  float4 t3[1] = {make_float4(mxv[0], mxv[1], mxv[2], mxv[3])};
  bn_reduce_tail(sh, t1, t2, t3, cok, nrl, cw, rl, cl, cq, partial, grp, chunks, c, c4n, prows, 4.f);
}

// The quad gather of the stem tail's backward passes: the 2 x 2 pixel quad (rows 2 qa, 2 qa + 1, columns 2 qb, 2 qb + 1) x 4
// channels of image n can only have won the pooling windows (qa, qa + 1) x (qb, qb + 1): their four (argmax, gradient)
// records and the quad's four y are loaded once, and pixel(px, d, v) is called for every pixel inside the image with its
// float4 index px, the sum d of the gradients of the windows it won - added in the order (qa, qb), (qa, qb + 1),
// (qa + 1, qb), (qa + 1, qb + 1), ReLU mask not applied yet - and its y.  `pixel` captures BY VALUE and receives what it
// accumulates into as `sums`: values reached through a closure of references are promoted to registers only after the
// loop optimisations have run, and the per-channel products of bn_dy then contract differently (other roundings).
template <typename T, typename F, typename... S>
__device__ __forceinline__ void pool_quad_gather(const T *__restrict__ gp, const uchar4 *__restrict__ am, const T *__restrict__ y, long long n,
                                                 int qa, int qb, int cq, int h, int w, int ho, int wo, int c4n, F pixel, S &...sums) {
  uchar4 wk[2][2];
  float4 wg[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bool ok = qa + i < ho && qb + j < wo;
      const long long o = ((n * ho + qa + i) * wo + qb + j) * c4n + cq;
      wk[i][j] = ok ? am[o] : make_uchar4(255, 255, 255, 255);
      wg[i][j] = ok ? Elem<T>::ld4(gp, o) : zero4();
    }
  float4 v[2][2];
  bool pok[2][2];
#pragma unroll
  for (int pi = 0; pi < 2; ++pi)
#pragma unroll
    for (int pj = 0; pj < 2; ++pj) {
      pok[pi][pj] = 2 * qa + pi < h && 2 * qb + pj < w;
      v[pi][pj] = pok[pi][pj] ? Elem<T>::ld4(y, ((n * h + 2 * qa + pi) * w + 2 * qb + pj) * c4n + cq) : zero4();
    }
#pragma unroll
  for (int pi = 0; pi < 2; ++pi)
#pragma unroll
    for (int pj = 0; pj < 2; ++pj) {
      if (!pok[pi][pj]) continue;
      // pixel (2 qa + pi, 2 qb + pj) inside window (qa + i, qb + j): kh = pi + 1 - 2 i, kw = pj + 1 - 2 j (in 0..2)
      float4 d = zero4();
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int kh = pi + 1 - 2 * i;
        if (kh < 0) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int kw = pj + 1 - 2 * j;
          if (kw < 0) continue;
          d = map4([](float d, unsigned k, float g, unsigned me) { return k == me ? d + g : d; }, d, wk[i][j], wg[i][j], (unsigned)(kh * 3 + kw));
        }
      }
      pixel(((n * h + 2 * qa + pi) * w + 2 * qb + pj) * c4n + cq, d, v[pi][pj], sums...);
    }
}

// grid = (ceil(ceil(w/2)*c4n / 256), images*ceil(h/2)): one thread = one 2 x 2 pixel quad (rows 2a, 2a+1, columns 2b, 2b+1)
// x 4 channels of the conv output.  The quad's pixels can only have won the pooling windows (a, a+1) x (b, b+1): their
// four (argmax, gradient) records are loaded once and dealt out (one thread per pixel fetched 9 records per quad and had
// a single 16-byte load of y in flight: 0.86 ms at C5 where the bytes take 0.35).  Window contributions are added in
// the order (a, b), (a, b+1), (a+1, b), (a+1, b+1).
template <typename T, typename TO = T>
__global__ __launch_bounds__(256) void bn_pool_bwd_apply_kernel(const T *__restrict__ gp, const uchar4 *__restrict__ am,
                                                                const T *__restrict__ y, const float *__restrict__ mean,
                                                                const float *__restrict__ invstd,
                                                                const float *__restrict__ gamma,
                                                                const float *__restrict__ scale,
                                                                const float *__restrict__ shift, const float *__restrict__ s1,
                                                                const float *__restrict__ s2, int n_per_group, int h, int w,
                                                                int ho, int wo, int c4n, float inv_rows,
                                                                TO *__restrict__ dy, const float *__restrict__ dy_sinv) {
  const int hq = (h + 1) >> 1, wq = (w + 1) >> 1;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= wq * c4n) return;
  const int qb = t / c4n, cq = t - qb * c4n;
  const int n = blockIdx.y / hq, qa = blockIdx.y - n * hq;
  const long long gq = (long long)(n / n_per_group) * c4n + cq;
  const float4 mu = reinterpret_cast<const float4 *>(mean)[gq], is = reinterpret_cast<const float4 *>(invstd)[gq];
  const float4 sa = reinterpret_cast<const float4 *>(scale)[gq], sb = reinterpret_cast<const float4 *>(shift)[gq];
  const float4 a1 = reinterpret_cast<const float4 *>(s1)[gq], a2 = reinterpret_cast<const float4 *>(s2)[gq];
  const float4 ga = reinterpret_cast<const float4 *>(gamma)[cq];
  const bool scaled = dy_sinv != nullptr;                   // sp result: times 2^k (bn_dy_scale_kernel; exact)
  const float dsc = scaled ? 1.f / *dy_sinv : 1.f;
  pool_quad_gather(gp, am, y, n, qa, qb, cq, h, w, ho, wo, c4n, [=](long long px, float4 d, float4 v) {
    d = mask_affine4(d, v, sa, sb);
    float4 o = bn_dy(d, v, mu, is, ga, a1, a2, inv_rows);
    if (scaled) o = mul4(o, dsc);
    Elem<TO>::st4(dy, px, o);
  });
}

// ---- eval mode: BatchNorm on the running statistics, backward in ONE streaming pass -----------------------------
// With x-hat = (y - running_mean) * invstd_r, invstd_r = 1 / sqrt(running_var + eps) and dz = g masked by the ReLU:
//   dy = gamma * invstd_r * dz,   dbeta = sum dz,   dgamma = sum dz * x-hat
// dy needs no sum, so the train-mode pair (reduce, then an apply that waits for it) becomes one pass reading g, y (and
// the mask) and writing dy; the sums leave per-(group, chunk, channel) partials in bn_bwd_reduce_kernel's layout
// ([groups][chunks][2][c]) and bn_eval_bwd_finalize_kernel adds them in a fixed order.  The mask is the forward's:
// relu_bits (bn_apply_bits), act > 0, or relu_on(y, mscale, mshift) with bn_eval_affine's scale / shift (bn_math.h);
// none of them: no ReLU.  dy and dz_out may alias g (every element is read, then written, by one lane).
__device__ __forceinline__ void bn_eval_factors(const float *gamma, const float *rmean, const float *rvar, float eps, int cq,
                                                float4 &mu, float4 &is, float4 &k) {
  const float4 ga = reinterpret_cast<const float4 *>(gamma)[cq], rm = reinterpret_cast<const float4 *>(rmean)[cq];
  const float4 rv = reinterpret_cast<const float4 *>(rvar)[cq];
  const float4 sd = map4([](float rv, float eps) { return sqrtf(rv + eps); }, rv, eps);
  mu = rm;
  is = map4([](float sd) { return 1.f / sd; }, sd);
  k = map4([](float ga, float sd) { return ga / sd; }, ga, sd);     // = bn_eval_affine_kernel's scale
}

// grid = (chunks, column blocks, groups); thread = one 16-byte column group (W float4: 4 channels in fp32, 8 in bf16) x one
// row lane (bn_bwd_reduce_kernel's shape).  bf16 storage: g, act, y are widened to fp32, the arithmetic is the fp32
// kernel's, and dz / dy are rounded once on their way out; a relu_bits byte covers the access's 8 elements.
template <typename T>
__global__ __launch_bounds__(256) void bn_eval_bwd_kernel(const T *g, const T *__restrict__ act, const T *__restrict__ y,
                                                          const unsigned char *__restrict__ relu_bits,
                                                          const float *__restrict__ mscale, const float *__restrict__ mshift,
                                                          const float *__restrict__ gamma, const float *__restrict__ rmean,
                                                          const float *__restrict__ rvar, float eps, long long rows,
                                                          long long rows_per_chunk, int c, int cwn, int cw, T *dy, T *dz_out,
                                                          float *__restrict__ partial, int chunks) {
  typedef Elem<T> E;
  constexpr int W = E::W;
  __shared__ float4 sh[2][256][W];
  const int grp = blockIdx.z;
  const int rl = threadIdx.x / cw, cl = threadIdx.x % cw;
  const int nrl = 256 / cw;
  const int cq = blockIdx.y * cw + cl;
  const bool cok = cq < cwn;
  float4 s1[W], s2[W];
#pragma unroll
  for (int w = 0; w < W; ++w) s1[w] = s2[w] = zero4();
  if (cok) {
    float4 mu[W], is[W], k[W], ma[W], mb[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
      bn_eval_factors(gamma, rmean, rvar, eps, cq * W + w, mu[w], is[w], k[w]);
      ma[w] = mb[w] = zero4();
      if (mscale) {
        ma[w] = reinterpret_cast<const float4 *>(mscale + (long long)grp * c)[cq * W + w];
        mb[w] = reinterpret_cast<const float4 *>(mshift + (long long)grp * c)[cq * W + w];
      }
    }
    const long long r0 = (long long)blockIdx.x * rows_per_chunk;
    long long r1 = r0 + rows_per_chunk;
    if (r1 > rows) r1 = rows;
    const long long gbase = (long long)grp * rows * cwn;
    auto row = [&](long long r, float4 (&a1)[W], float4 (&a2)[W]) {
      const long long off = gbase + r * cwn + cq;
      float4 d[W], v[W], a[W], o[W];
      E::ldw(g, off, d);
      E::ldw(y, off, v);
      if (act) E::ldw(act, off, a);
      const unsigned mb8 = relu_bits ? (unsigned)relu_bits[off] : 0u;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        if (relu_bits) d[w] = mask_bits4(d[w], mb8 >> (4 * w));
        else if (act) d[w] = mask_act4(d[w], a[w]);
        else if (mscale) d[w] = mask_affine4(d[w], v[w], ma[w], mb[w]);
        acc4(a1[w], d[w]);
        acc4_xhat(a2[w], d[w], v[w], mu[w], is[w]);
        o[w] = mul4(k[w], d[w]);
      }
      if (dz_out) E::stw(dz_out, off, d);
      E::stw(dy, off, o);
    };
    constexpr int U = W == 1 ? 4 : 2;          // rows in flight per thread (bn_bwd_reduce_kernel's counts)
    float4 t1[U - 1][W], t2[U - 1][W];
#pragma unroll
    for (int u = 0; u < U - 1; ++u)
#pragma unroll
      for (int w = 0; w < W; ++w) t1[u][w] = t2[u][w] = zero4();
    long long r = r0 + rl;
    for (; r + (U - 1) * (long long)nrl < r1; r += U * (long long)nrl) {
      row(r, s1, s2);
#pragma unroll
      for (int u = 1; u < U; ++u) row(r + u * (long long)nrl, t1[u - 1], t2[u - 1]);
    }
    for (; r < r1; r += nrl) row(r, s1, s2);
#pragma unroll
    for (int w = 0; w < W; ++w) {
      if constexpr (U == 4) {
        acc4(s1[w], add4(t1[0][w], add4(t1[1][w], t1[2][w])));
        acc4(s2[w], add4(t2[0][w], add4(t2[1][w], t2[2][w])));
      } else {
        acc4(s1[w], t1[0][w]);
        acc4(s2[w], t2[0][w]);
      }
    }
  }
  bn_reduce_tail(sh, s1, s2, nullptr, cok, nrl, cw, rl, cl, cq, partial, grp, chunks, c, c / 4);
}

// The stem tail in eval mode: max-pool backward through argmax, the ReLU mask from y, then dy = gamma invstd_r dz - the
// quad gather of bn_pool_bwd_apply_kernel (a lane owns a 2 x 2 pixel quad x 4 channels and deals out the four windows that
// quad can have won), so the 112 x 112 gradient map is written once, as dy.  grid = (chunks, groups), a grid-stride loop
// over the group's (image, quad row, quad column, channel group) items; c/4 divides 256, so a lane keeps its channels and
// the workgroup's partial sums go to partial[group][blockIdx.x] ([groups][chunks][2][c], as above).  4 channels per lane
// whatever the storage (bf16: 8-byte accesses, as the train-mode pooled reduce has them).
template <typename T>
__global__ __launch_bounds__(256) void bn_pool_eval_bwd_kernel(const T *__restrict__ gp, const uchar4 *__restrict__ am,
                                                               const T *__restrict__ y, const float *__restrict__ mscale,
                                                               const float *__restrict__ mshift, const float *__restrict__ gamma,
                                                               const float *__restrict__ rmean, const float *__restrict__ rvar,
                                                               float eps, int n_per_group, int h, int w, int ho, int wo, int c4n,
                                                               T *__restrict__ dy, float *__restrict__ partial) {
  __shared__ float4 sh[2][256];
  const int hq = (h + 1) >> 1, wq = (w + 1) >> 1;
  const int grp = blockIdx.y;
  const int cq = threadIdx.x % c4n;            // 256 % c4n == 0 and the grid stride is a multiple of 256
  float4 mu, is, k;
  bn_eval_factors(gamma, rmean, rvar, eps, cq, mu, is, k);
  const float4 sa = reinterpret_cast<const float4 *>(mscale)[(long long)grp * c4n + cq];
  const float4 sb = reinterpret_cast<const float4 *>(mshift)[(long long)grp * c4n + cq];
  float4 s1 = zero4(), s2 = s1;
  const long long items = (long long)n_per_group * hq * wq * c4n;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += stride) {
    const long long q = i / c4n;
    const int qb = (int)(q % wq);
    const long long line = q / wq;
    const int qa = (int)(line % hq);
    const long long n = (long long)grp * n_per_group + line / hq;
    pool_quad_gather(gp, am, y, n, qa, qb, cq, h, w, ho, wo, c4n, [=](long long px, float4 d, float4 v, float4 &s1, float4 &s2) {
      d = mask_affine4(d, v, sa, sb);
      acc4(s1, d);
      acc4_xhat(s2, d, v, mu, is);
      Elem<T>::st4(dy, px, mul4(k, d));
    }, s1, s2);
  }
  // (not bn_reduce_tail: this kernel has no 256 / c4n, and a strided fold over the lanes j = lane + c4n, + 2 c4n, ...)
  sh[0][threadIdx.x] = s1;
  sh[1][threadIdx.x] = s2;
  __syncthreads();
  if (threadIdx.x < c4n) {
    for (int j = threadIdx.x + c4n; j < 256; j += c4n) {
      acc4(s1, sh[0][j]);
      acc4(s2, sh[1][j]);
    }
    float4 *p = reinterpret_cast<float4 *>(partial + (((long long)grp * gridDim.x + blockIdx.x) * 2) * (4 * c4n));
    p[cq] = s1;
    p[c4n + cq] = s2;
  }
}

// dgamma (+)= the sum of every (group, chunk) partial's s2 row, dbeta (+)= ... of the s1 rows.  grid = c/16 workgroups of
// 1024 lanes = 16 channels x 64 partial-lanes; every lane adds a fixed stride of the partials in fp64 (groups in order),
// then a fixed tree: the same sums every run.
__global__ __launch_bounds__(1024) void bn_eval_bwd_finalize_kernel(const float *__restrict__ partial, int n_partials, int c,
                                                                    float *dgamma, float *dbeta, int accumulate) {
  __shared__ double sh[2][64][16];
  const int cl = threadIdx.x & 15, pl = threadIdx.x >> 4;
  const int ch = blockIdx.x * 16 + cl;
  double a = 0.0, b = 0.0;
  if (ch < c)
    for (int k = pl; k < n_partials; k += 64) {
      a += partial[(long long)k * 2 * c + ch];
      b += partial[((long long)k * 2 + 1) * c + ch];
    }
  sh[0][pl][cl] = a;
  sh[1][pl][cl] = b;
  __syncthreads();
  for (int o = 32; o > 0; o >>= 1) {
    if (pl < o) {
      sh[0][pl][cl] += sh[0][pl + o][cl];
      sh[1][pl][cl] += sh[1][pl + o][cl];
    }
    __syncthreads();
  }
  if (pl == 0 && ch < c) {
    if (dbeta) dbeta[ch] = (accumulate ? dbeta[ch] : 0.f) + (float)sh[0][0][cl];
    if (dgamma) dgamma[ch] = (accumulate ? dgamma[ch] : 0.f) + (float)sh[1][0][cl];
  }
}

static int bwd_chunks(int groups, long long rows, int c) {
  // at least 64 rows per chunk
  const int c4n = c / 4;
  const int cw = c4n < 256 ? c4n : 256;
  const int colblocks = ceil_div(c4n, cw);
  // one resident round: the kernel's registers and LDS admit three workgroups per CU; measured at C3's shapes
  // (scripts/bn_bench.py): 256 / 384 / 512 / 768 / 1024 / 2048 / 4096 workgroups -> 13.7 / 11.2 / 9.7 / 9.4 / 10.7 /
  // 10.2 / 10.5 ms per step (1024 = a full round plus a third of one)
  int total = 3 * compute_cus();
  if (total < 64) total = 64;
  long long want = total / ((long long)groups * colblocks);
  if (want < 1) want = 1;
  long long maxc = (rows + 63) / 64;
  if (want > maxc) want = maxc;
  return (int)want;
}

// workgroups per group of bn_pool_eval_bwd_kernel's grid-stride loop (= its partials per group): four per CU in all
static int eval_pool_chunks(int groups) {
  const int b = 4 * compute_cus() / groups;
  return b > 1 ? b : 1;
}

static int grid_for(long long n4) {
  long long b = (n4 + 255) / 256;
  if (b > 4096) b = 4096;      // thinner grids (1024 / 2048) were tried to leave wave slots to the wgrad stream: no gain
  if (b < 1) b = 1;
  return (int)b;
}

// The geometry of the reduce-type passes over [rows][c]: cwn 16-byte column groups per row (W float4 each), column
// blocks of cw = min(cwn, 256) of them - 256 / cw row lanes per workgroup, so cw must divide 256 - and the rows cut
// into `chunks` ranges of rows_per_chunk.
struct ReduceGeom {
  int cwn, cw, chunks;
  long long rows_per_chunk;
};
static int reduce_geometry(const char *who, int groups, long long rows, int c, int W, ReduceGeom &g) {
  g.cwn = c / 4 / W;
  g.cw = g.cwn < 256 ? g.cwn : 256;
  // (more than 256 column groups: blocks of 256, the last one masked where cwn is no multiple of 256 - c = 1536 in fp32)
  MVG_REQUIRE(g.cw > 0 && 256 % g.cw == 0, "%s: c/%d must divide 256 or be larger than 256 (c=%d)", who, 4 * W, c);
  g.chunks = bwd_chunks(groups, rows, c);
  g.rows_per_chunk = (rows + g.chunks - 1) / g.chunks;
  return 0;
}

// The stem tail's reduce pass cuts POOLED lines (image, oy), not rows: never more chunks than lines, and none without one.
static int pool_reduce_chunks(int chunks, int lines, int &lines_per_chunk) {
  if (chunks > lines) chunks = lines;
  lines_per_chunk = (lines + chunks - 1) / chunks;
  return (lines + lines_per_chunk - 1) / lines_per_chunk;
}

// workgroups per group of bn_pool_eval_bwd_kernel: one per 256 (quad, channel group) items, at most eval_pool_chunks
static int eval_pool_grid(int groups, int n_per_group, int h, int w, int c4n) {
  const long long items = (long long)n_per_group * ((h + 1) / 2) * ((w + 1) / 2) * c4n;
  long long chunks = (items + 255) / 256;
  if (chunks > eval_pool_chunks(groups)) chunks = eval_pool_chunks(groups);
  return (int)chunks;
}

// The geometry of the streaming passes over `accesses` 16-byte accesses per group, cwn of them per row: grid_for's
// workgroups of 256 lanes, every lane looping with the grid's stride; `step` is what the kernels advance a lane's column
// group by per trip (0: it keeps its columns, and the bf16 / sp kernels their per-channel factors).
struct StreamGeom {
  int grid, trips, step;
};
static StreamGeom stream_geometry(long long accesses, int cwn) {
  StreamGeom s;
  s.grid = grid_for(accesses);
  const long long stride = (long long)s.grid * 256;
  s.trips = (int)((accesses + stride - 1) / stride);
  s.step = (int)(stride % cwn);
  return s;
}

// Which merge mvg_bn_finalize runs, from the sizes and the scratch the stream has (api.hip: mvg_set_scratch):
//   form 0  bn_finalize_kernel walks the groups (one group, or no scratch for the per-group records)
//   form 1  bn_finalize_allgroups_kernel: 2 - 4 groups share a workgroup's 128 lanes
//   form 2  bn_finalize_group_kernel + bn_running_update_kernel
// and whether bn_partials_slice_kernel runs first (>= 1024 partials and scratch for the slices behind the records).
struct FinalizePlan {
  int form, lanes_per_group, slices, per_slice;
  size_t mv_floats, need_floats;     // scratch of the per-group records; of records + slices (what the sliced form asks for)
};
static FinalizePlan finalize_plan(int groups, int partials, int c, size_t scratch_floats) {
  FinalizePlan f;
  f.mv_floats = (size_t)groups * 2 * c * 2;      // [groups][2][c] doubles
  f.need_floats = f.mv_floats;
  f.slices = f.per_slice = 0;
  const bool mv = groups > 1 && scratch_floats >= f.mv_floats;
  if (partials >= 1024) {
    const int per_slice = ceil_div(partials, 64);
    const int slices = ceil_div(partials, per_slice);
    f.need_floats = f.mv_floats + (size_t)groups * slices * 3 * c * 2;
    if (scratch_floats >= f.need_floats) {
      f.slices = slices;
      f.per_slice = per_slice;
    }
  }
  if (groups > 1 && groups <= 4 && (partials < 1024 || f.slices)) {
    // (>= 32 lanes per group; with 8 groups - C5's shapes - 16 lanes per group made the call slower than the two launches
    // of form 2: bn_finalize 1.00 -> 1.39 ms per C5 step)
    f.form = 1;
    f.lanes_per_group = 128 / groups;
  } else {
    f.form = mv ? 2 : 0;
    f.lanes_per_group = 128;
  }
  return f;
}

// The ReLU mask of a backward pass comes ONE way: the activation, the bits bn_apply recorded, or y with (scale, shift).
static int require_one_mask(const char *who, const char *ways, const void *act, const void *relu_bits, const float *relu_scale,
                            const float *relu_shift) {
  MVG_REQUIRE((act ? 1 : 0) + (relu_bits ? 1 : 0) + (relu_scale ? 1 : 0) <= 1, "%s: give the ReLU mask %s", who, ways);
  MVG_REQUIRE((relu_scale == nullptr) == (relu_shift == nullptr), "%s: relu_scale and relu_shift go together", who);
  return 0;
}

// The channel counts the passes take (shared with mvg_bn_plan_query): W float4 groups per 16-byte access; 8 channels per lane in sp
static int require_channels(const char *who, int c, int W) {
  MVG_REQUIRE(c % 4 == 0, "%s: c %% 4 != 0", who);
  MVG_REQUIRE(c % (4 * W) == 0, "%s: c must be a multiple of %d", who, 4 * W);
  return 0;
}
static int require_c8(const char *who, int c) {
  MVG_REQUIRE(c % 8 == 0, "%s: c %% 8 != 0", who);
  return 0;
}
static int require_pool_eval_sizes(int groups, int n_per_group, int h, int w, int c) {
  MVG_REQUIRE(groups > 0 && groups < 65536 && n_per_group > 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0 && 256 % (c / 4) == 0,
              "bn_relu_maxpool_eval_bwd: bad sizes (c/4 must divide 256, c=%d)", c);
  return 0;
}

// *dy_sinv of a unit whose dy goes out in sp, unless the reduce pass / the fused backward-data launch left it already
// (they do when they are given gamma)
static int ensure_dy_scale(int ready, const float *gamma, const float *invstd, const float *s1, const float *s2, const float *mx, int groups,
                           int c, long long rows, float *dy_sinv, hipStream_t st) {
  if (ready) return 0;
  hipLaunchKernelGGL(bn_dy_scale_kernel, dim3(1), dim3(1024), 0, st, gamma, invstd, s1, s2, mx, groups, c, 1.0f / (float)rows,
                     sqrtf((float)rows), dy_sinv);
  return check_launch("bn_dy_scale");
}

int bn_bwd_finalize_launch(const float *partial, int groups, int chunks, int c, float *s1, float *s2, float *dgamma,
                           float *dbeta, int accumulate, hipStream_t st, float *mx, const float *raw_mean, const float *raw_invstd,
                           const float *gamma, const float *invstd, long long rows, float *dy_sinv) {
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(ceil_div(c, 16), groups), dim3(1024), 0, st, partial, groups, chunks, c, s1, s2, mx,
                     raw_mean, raw_invstd);
  if (check_launch("bn_bwd_finalize")) return 1;
  if (dy_sinv && gamma && invstd && mx && rows > 0) {       // split path: dgamma / dbeta and dy's scale in one launch
    hipLaunchKernelGGL(bn_bwd_dgamma_dyscale_kernel, dim3(1), dim3(1024), 0, st, s1, s2, mx, groups, c, dgamma, dbeta, accumulate, gamma, invstd,
                       1.0f / (float)rows, sqrtf((float)rows), dy_sinv);
    return check_launch("bn_bwd_dgamma_dyscale");
  }
  if (dgamma || dbeta) {
    hipLaunchKernelGGL(bn_bwd_dgamma_kernel, dim3(ceil_div(c, 256)), dim3(256), 0, st, s1, s2, groups, c, dgamma, dbeta, accumulate);
    return check_launch("bn_bwd_dgamma");
  }
  return 0;
}

}  // namespace mvg

using namespace mvg;

extern "C" {

int mvg_bn_finalize(const float *stats, int groups, int partials, int rows_per_partial, int64_t rows_per_group, int c,
                    const float *gamma, const float *beta, float *running_mean, float *running_var, float momentum,
                    float eps, float *mean, float *invstd, float *scale, float *shift, void *stream) {
  MVG_REQUIRE(groups > 0 && partials > 0 && c > 0 && rows_per_group > 0, "bn_finalize: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_BN_FINALIZE, st, 0.0, 4.0 * groups * (double)partials * 2 * c);
  // scratch: [groups][2][c] doubles for the group-parallel form, then the slices; the plan is made for what the stream has
  size_t have = 0;
  {
    const FinalizePlan want = finalize_plan(groups, partials, c, (size_t)-1);
    if (stream_scratch(st, want.need_floats)) have = want.need_floats;
    else if (stream_scratch(st, want.mv_floats)) have = want.mv_floats;
  }
  const FinalizePlan fp = finalize_plan(groups, partials, c, have);
  float *base = have ? stream_scratch(st, have) : nullptr;
  double *mv = fp.form == 2 ? (double *)base : nullptr;
  const double *sliced = nullptr;
  const int slices = fp.slices;
  if (slices) {
    double *buf = (double *)(base + fp.mv_floats);
    hipLaunchKernelGGL(bn_partials_slice_kernel, dim3(ceil_div(c, 8), slices, groups), dim3(256), 0, st, stats, partials,
                       rows_per_partial, (long long)rows_per_group, c, fp.per_slice, buf, slices);
    if (check_launch("bn_partials_slice")) return 1;
    sliced = buf;
  }
  if (fp.form == 1) {
    // every group's statistics and the running statistics in ONE launch (the workgroup's lanes divided between the groups)
    hipLaunchKernelGGL(bn_finalize_allgroups_kernel, dim3(ceil_div(c, 8)), dim3(1024), 0, st, stats, sliced, slices, groups, fp.lanes_per_group,
                       partials, rows_per_partial, (long long)rows_per_group, c, gamma, beta, eps, momentum, mean, invstd, scale, shift,
                       running_mean, running_var);
    return check_launch("bn_finalize(all groups)");
  }
  if (fp.form == 2) {
    hipLaunchKernelGGL(bn_finalize_group_kernel, dim3(ceil_div(c, 8), groups), dim3(1024), 0, st, stats, sliced, slices, partials,
                       rows_per_partial, (long long)rows_per_group, c, gamma, beta, eps, mean, invstd, scale, shift, mv);
    if (check_launch("bn_finalize(groups)")) return 1;
    if (running_mean || running_var) {
      hipLaunchKernelGGL(bn_running_update_kernel, dim3(ceil_div(c, 256)), dim3(256), 0, st, mv, groups, c, momentum, running_mean,
                         running_var);
      return check_launch("bn_running_update");
    }
    return 0;
  }
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(ceil_div(c, 8)), dim3(1024), 0, st, stats, sliced, slices, groups, partials,
                     rows_per_partial, (long long)rows_per_group, c, gamma, beta, running_mean, running_var, momentum, eps, mean,
                     invstd, scale, shift);
  return check_launch("bn_finalize");
}

int mvg_bn_eval_affine(int groups, int c, const float *gamma, const float *beta, const float *running_mean,
                       const float *running_var, float eps, float *scale, float *shift, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_BN_FINALIZE, st, 0.0, 4.0 * 6 * c);
  hipLaunchKernelGGL(bn_eval_affine_kernel, dim3(ceil_div((long long)groups * c, 256)), dim3(256), 0, st, groups, c, gamma,
                     beta, running_mean, running_var, eps, scale, shift);
  return check_launch("bn_eval_affine");
}

// items_dev: n records in DEVICE memory of { const float *gamma, *beta, *running_mean, *running_var; float *scale, *shift;
// int32 c; int32 pad; } (56 bytes): scale[c], shift[c] of every record as mvg_bn_eval_affine(1, c, ...) leaves them.
int mvg_bn_eval_affine_batch(const void *items_dev, int n, int max_c, float eps, void *stream) {
  static_assert(sizeof(BnEvalItem) == 56, "BnEvalItem: the callers build 56-byte records");
  MVG_REQUIRE(items_dev != nullptr && n >= 1 && n <= 65535 && max_c >= 1, "bn_eval_affine_batch: null table, or n / max_c out of range");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_BN_FINALIZE, st, 0.0, 4.0 * 6 * max_c * n);
  hipLaunchKernelGGL(bn_eval_affine_batch_kernel, dim3((unsigned)ceil_div(max_c, 256), (unsigned)n), dim3(256), 0, st,
                     (const BnEvalItem *)items_dev, eps);
  return check_launch("bn_eval_affine_batch");
}

}  // extern "C" (templated implementations below)

template <typename T, typename TO = T, typename TR = T>
static int bn_apply_impl(const T *y, const float *scale, const float *shift, const TR *residual, const float *res_scale,
                         const float *res_shift, int relu, TO *out, int groups, int64_t rows_per_group, int c, void *stream,
                         uint8_t *relu_bits = nullptr) {
  MVG_REQUIRE((res_scale == nullptr) == (res_shift == nullptr) && (residual || !res_scale),
              "bn_apply: res_scale / res_shift go together and need a residual");
  hipStream_t st = (hipStream_t)stream;
  const long long n4 = rows_per_group * (c / 4);
  constexpr int W = Elem<T>::W;
  if (int e = require_channels("bn_apply", c, W)) return e;
  ProfScope ps(MVG_K_BN_APPLY, st, 0.0,
               4.0 * groups * (double)n4 * (Elem<T>::kBytes + Elem<TO>::kBytes + (residual ? Elem<TR>::kBytes : 0.0)));
  hipLaunchKernelGGL((bn_apply_kernel<T, TO, TR>), dim3(stream_geometry(n4 / W, c / 4 / W).grid, groups), dim3(256), 0, st, y, scale, shift, residual, res_scale,
                     res_shift, relu, out, n4 / W, c / 4 / W, c, relu_bits);
  return check_launch("bn_apply");
}

template <typename T>
static int bn_bwd_reduce_impl(const T *g, const T *act, const T *y, const float *mean, const float *invstd,
                              const float *relu_scale, const float *relu_shift, int groups, int64_t rows_per_group, int c,
                              float *s1, float *s2, float *dgamma, float *dbeta, int accumulate, float *workspace, T *dz_out,
                              void *stream, const uint8_t *relu_bits = nullptr, float *mx = nullptr, const float *gamma = nullptr,
                              float *dy_sinv = nullptr) {
  if (int e = require_one_mask("bn_bwd_reduce", "ONE way: act, (relu_scale, relu_shift) or relu_bits", act, relu_bits, relu_scale, relu_shift))
    return e;
  MVG_REQUIRE(workspace != nullptr, "bn_bwd_reduce: workspace required");
  hipStream_t st = (hipStream_t)stream;
  constexpr int W = Elem<T>::W;
  if (int e = require_channels("bn_bwd_reduce", c, W)) return e;
  ReduceGeom q;
  if (int e = reduce_geometry("bn_bwd_reduce", groups, rows_per_group, c, W, q)) return e;
  ProfScope ps(MVG_K_BN_BWD_REDUCE, st, 0.0, Elem<T>::kBytes * groups * (double)rows_per_group * c * ((act ? 3 : 2) + (dz_out ? 1 : 0)));
  hipLaunchKernelGGL(bn_bwd_reduce_kernel<T>, dim3(q.chunks, ceil_div(q.cwn, q.cw), groups), dim3(256), 0, st, g, act, y, mean, invstd,
                     relu_scale, relu_shift, (long long)rows_per_group, q.rows_per_chunk, c, q.cwn, q.cw, workspace, q.chunks, dz_out, relu_bits,
                     mx ? 3 : 2);
  if (check_launch("bn_bwd_reduce")) return 1;
  return bn_bwd_finalize_launch(workspace, groups, q.chunks, c, s1, s2, dgamma, dbeta, accumulate, st, mx, nullptr, nullptr, gamma, invstd,
                                (long long)rows_per_group, dy_sinv);
}

template <typename T, typename TO = T>
static int bn_bwd_apply_impl(const T *g, const T *act, const T *y, const float *mean, const float *invstd, const float *gamma,
                             const float *s1, const float *s2, const float *relu_scale, const float *relu_shift, int groups,
                             int64_t rows_per_group, int c, TO *dy, T *dz_out, void *stream) {
  if (int e = require_one_mask("bn_bwd_apply", "either as act or as (relu_scale, relu_shift)", act, nullptr, relu_scale, relu_shift)) return e;
  hipStream_t st = (hipStream_t)stream;
  const long long n4 = rows_per_group * (c / 4);
  constexpr int W = Elem<T>::W;
  if (int e = require_channels("bn_bwd_apply", c, W)) return e;
  ProfScope ps(MVG_K_BN_BWD_APPLY, st, 0.0,
               4.0 * groups * (double)n4 * (Elem<T>::kBytes * ((act ? 3 : 2) + (dz_out ? 1 : 0)) + Elem<TO>::kBytes));
  hipLaunchKernelGGL((bn_bwd_apply_kernel<T, TO>), dim3(stream_geometry(n4 / W, c / 4 / W).grid, groups), dim3(256), 0, st, g, act, y, mean, invstd, gamma, s1, s2,
                     relu_scale, relu_shift, n4 / W, 1.0f / (float)rows_per_group, c / 4 / W, c, dy, dz_out);
  return check_launch("bn_bwd_apply");
}

template <typename T, typename TO = T>
static int bn_relu_maxpool_fwd_impl(const T *y, const float *scale, const float *shift, TO *pooled, uint8_t *argmax, int groups,
                                    int n_per_group, int h, int w, int c, int ho, int wo, void *stream,
                                    const float *out_sinv = nullptr) {
  MVG_REQUIRE(c % 4 == 0, "bn_relu_maxpool: c %% 4 != 0");
  MVG_REQUIRE(ho == (h + 2 - 3) / 2 + 1 && wo == (w + 2 - 3) / 2 + 1, "bn_relu_maxpool: bad output size");
  const long long total = (long long)groups * n_per_group * ho * wo * (c / 4);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_POOL, st, 0.0,
               Elem<T>::kBytes * (double)groups * n_per_group * h * w * c + Elem<TO>::kBytes * (double)total * 4 + (double)total * 4);
  MVG_REQUIRE((long long)groups * n_per_group * ho < 65536, "bn_relu_maxpool: images*ho must fit grid.y");
  hipLaunchKernelGGL((bn_relu_maxpool_fwd_kernel<T, TO>), dim3(ceil_div((long long)wo * (c / 4), 256), groups * n_per_group * ho),
                     dim3(256), 0, st, y, scale, shift, pooled, (uchar4 *)argmax, n_per_group, h, w, c / 4, ho, wo, out_sinv);
  return check_launch("bn_relu_maxpool_fwd");
}

template <typename T>
static int bn_relu_maxpool_bwd_reduce_impl(const T *g_pooled, const uint8_t *argmax, const T *y, const float *mean,
                                           const float *invstd, const float *scale, const float *shift, int groups,
                                           int n_per_group, int h, int w, int c, int ho, int wo, float *s1, float *s2,
                                           float *dgamma, float *dbeta, int accumulate, float *workspace, void *stream,
                                           float *mx = nullptr, const float *gamma = nullptr, float *dy_sinv = nullptr) {
  if (int e = require_channels("bn_relu_maxpool_bwd_reduce", c, 1)) return e;
  MVG_REQUIRE(workspace != nullptr, "bn_relu_maxpool_bwd_reduce: workspace required");
  hipStream_t st = (hipStream_t)stream;
  const long long rows = (long long)n_per_group * h * w;
  ReduceGeom q;
  if (int e = reduce_geometry("bn_relu_maxpool_bwd_reduce", groups, rows, c, 1, q)) return e;
  const int c4n = q.cwn, cw = q.cw;
  // chunk = whole image lines; never more chunks than mvg_bn_bwd_workspace_floats(groups, rows, c) sizes
  const int lines = n_per_group * ho;                 // pooled lines
  int lpc = 0;
  const int chunks = pool_reduce_chunks(q.chunks, lines, lpc);
  ProfScope ps(MVG_K_BN_BWD_REDUCE, st, 0.0,
               Elem<T>::kBytes * groups * ((double)rows * c + (double)n_per_group * ho * wo * c * 1.25));
  hipLaunchKernelGGL(bn_pool_bwd_reduce_kernel<T>, dim3(chunks, ceil_div(c4n, cw), groups), dim3(256), 0, st, g_pooled,
                     (const uchar4 *)argmax, y, mean, invstd, scale, shift, lpc, n_per_group, h, w, ho, wo, c, c4n, cw, workspace,
                     chunks, mx ? 3 : 2);
  if (check_launch("bn_relu_maxpool_bwd_reduce")) return 1;
  return bn_bwd_finalize_launch(workspace, groups, chunks, c, s1, s2, dgamma, dbeta, accumulate, st, mx, nullptr, nullptr, gamma, invstd, rows,
                                dy_sinv);
}

template <typename T, typename TO = T>
static int bn_relu_maxpool_bwd_apply_impl(const T *g_pooled, const uint8_t *argmax, const T *y, const float *mean,
                                          const float *invstd, const float *gamma, const float *scale, const float *shift,
                                          const float *s1, const float *s2, int groups, int n_per_group, int h, int w, int c,
                                          int ho, int wo, TO *dy, void *stream, const float *dy_sinv = nullptr) {
  MVG_REQUIRE(c % 4 == 0, "bn_relu_maxpool_bwd_apply: c %% 4 != 0");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_BN_BWD_APPLY, st, 0.0,
               Elem<T>::kBytes * groups * ((double)n_per_group * h * w * c * 2 + (double)n_per_group * ho * wo * c * 1.25));
  MVG_REQUIRE((long long)groups * n_per_group * ((h + 1) / 2) < 65536, "bn_relu_maxpool: images * h / 2 must fit grid.y");
  hipLaunchKernelGGL((bn_pool_bwd_apply_kernel<T, TO>), dim3(ceil_div((long long)((w + 1) / 2) * (c / 4), 256), groups * n_per_group * ((h + 1) / 2)), dim3(256),
                     0, st, g_pooled, (const uchar4 *)argmax, y, mean, invstd, gamma, scale, shift, s1, s2, n_per_group, h, w, ho,
                     wo, c / 4, 1.0f / (float)((long long)n_per_group * h * w), dy, dy_sinv);
  return check_launch("bn_relu_maxpool_bwd_apply");
}

extern "C" {

size_t mvg_bn_bwd_workspace_floats(int groups, int64_t rows_per_group, int c) {
  return (size_t)groups * bwd_chunks(groups, rows_per_group, c) * 3 * c;      // (s1, s2, and - mvg_bn_bwd_reduce_split - max |dz|)
}

#define MVG_BN_FACES(SUFFIX, T)                                                                                              \
  int mvg_bn_apply##SUFFIX(const T *y, const float *scale, const float *shift, const T *residual,                           \
                           const float *res_scale, const float *res_shift, int relu, T *out, int groups,                    \
                           int64_t rows_per_group, int c, void *stream) {                                                   \
    return bn_apply_impl<T>(y, scale, shift, residual, res_scale, res_shift, relu, out, groups, rows_per_group, c, stream);  \
  }                                                                                                                          \
  int mvg_bn_bwd_reduce##SUFFIX(const T *g, const T *act, const T *y, const float *mean, const float *invstd,               \
                                const float *relu_scale, const float *relu_shift, int groups, int64_t rows_per_group,       \
                                int c, float *s1, float *s2, float *dgamma, float *dbeta, int accumulate,                   \
                                float *workspace, T *dz_out, void *stream) {                                                \
    return bn_bwd_reduce_impl<T>(g, act, y, mean, invstd, relu_scale, relu_shift, groups, rows_per_group, c, s1, s2,        \
                                 dgamma, dbeta, accumulate, workspace, dz_out, stream);                                     \
  }                                                                                                                          \
  int mvg_bn_bwd_apply##SUFFIX(const T *g, const T *act, const T *y, const float *mean, const float *invstd,                \
                               const float *gamma, const float *s1, const float *s2, const float *relu_scale,               \
                               const float *relu_shift, int groups, int64_t rows_per_group, int c, T *dy, T *dz_out,        \
                               void *stream) {                                                                              \
    return bn_bwd_apply_impl<T>(g, act, y, mean, invstd, gamma, s1, s2, relu_scale, relu_shift, groups, rows_per_group,     \
                                c, dy, dz_out, stream);                                                                     \
  }                                                                                                                          \
  int mvg_bn_relu_maxpool_fwd##SUFFIX(const T *y, const float *scale, const float *shift, T *pooled, uint8_t *argmax,       \
                                      int groups, int n_per_group, int h, int w, int c, int ho, int wo, void *stream) {     \
    return bn_relu_maxpool_fwd_impl<T>(y, scale, shift, pooled, argmax, groups, n_per_group, h, w, c, ho, wo, stream);      \
  }                                                                                                                          \
  int mvg_bn_relu_maxpool_bwd_reduce##SUFFIX(const T *g_pooled, const uint8_t *argmax, const T *y, const float *mean,       \
                                             const float *invstd, const float *scale, const float *shift, int groups,       \
                                             int n_per_group, int h, int w, int c, int ho, int wo, float *s1, float *s2,    \
                                             float *dgamma, float *dbeta, int accumulate, float *workspace,                 \
                                             void *stream) {                                                                \
    return bn_relu_maxpool_bwd_reduce_impl<T>(g_pooled, argmax, y, mean, invstd, scale, shift, groups, n_per_group, h, w,   \
                                              c, ho, wo, s1, s2, dgamma, dbeta, accumulate, workspace, stream);             \
  }                                                                                                                          \
  int mvg_bn_relu_maxpool_bwd_apply##SUFFIX(const T *g_pooled, const uint8_t *argmax, const T *y, const float *mean,        \
                                            const float *invstd, const float *gamma, const float *scale,                    \
                                            const float *shift, const float *s1, const float *s2, int groups,               \
                                            int n_per_group, int h, int w, int c, int ho, int wo, T *dy, void *stream) {    \
    return bn_relu_maxpool_bwd_apply_impl<T>(g_pooled, argmax, y, mean, invstd, gamma, scale, shift, s1, s2, groups,        \
                                             n_per_group, h, w, c, ho, wo, dy, stream);                                     \
  }

MVG_BN_FACES(, float)
MVG_BN_FACES(_bf16, uint16_t)
#undef MVG_BN_FACES

// residual units: bn_apply also records the ReLU mask as one byte per 16-byte access (groups * rows * c / 4 bytes
// in fp32, / 8 in bf16) and the backward reduce pass reads those bytes instead of the activation
#define MVG_BN_BITS_FACES(SUFFIX, T)                                                                                          \
  int mvg_bn_apply_bits##SUFFIX(const T *y, const float *scale, const float *shift, const T *residual,                      \
                                const float *res_scale, const float *res_shift, T *out, uint8_t *relu_bits, int groups,      \
                                int64_t rows_per_group, int c, void *stream) {                                               \
    MVG_REQUIRE(relu_bits != nullptr, "bn_apply_bits: relu_bits is required");                                               \
    return bn_apply_impl<T>(y, scale, shift, residual, res_scale, res_shift, 1, out, groups, rows_per_group, c, stream,      \
                            relu_bits);                                                                                      \
  }                                                                                                                          \
  int mvg_bn_bwd_reduce_bits##SUFFIX(const T *g, const uint8_t *relu_bits, const T *y, const float *mean,                   \
                                     const float *invstd, int groups, int64_t rows_per_group, int c, float *s1, float *s2,   \
                                     float *dgamma, float *dbeta, int accumulate, float *workspace, T *dz_out,               \
                                     void *stream) {                                                                         \
    MVG_REQUIRE(relu_bits != nullptr, "bn_bwd_reduce_bits: relu_bits is required");                                          \
    return bn_bwd_reduce_impl<T>(g, nullptr, y, mean, invstd, nullptr, nullptr, groups, rows_per_group, c, s1, s2, dgamma,   \
                                 dbeta, accumulate, workspace, dz_out, stream, relu_bits);                                   \
  }
// ---- split path (conv_split.hip): conv outputs and gradients fp32, conv INPUTS (activations, dy) in sp ----------
// the reduce pass of a unit whose dy goes out in sp: mvg_bn_bwd_reduce / _bits (mask from relu_bits, or from relu_scale /
// relu_shift, or none) that also leaves max |masked gradient| per (group, channel) in mx [groups][c]
int mvg_bn_bwd_reduce_split(const float *g, const uint8_t *relu_bits, const float *y, const float *mean, const float *invstd,
                            const float *relu_scale, const float *relu_shift, int groups, int64_t rows_per_group, int c, float *s1,
                            float *s2, float *dgamma, float *dbeta, int accumulate, float *workspace, float *dz_out,
                            float *mx, const float *gamma, float *dy_sinv, void *stream) {
  MVG_REQUIRE(mx != nullptr, "bn_bwd_reduce_split: mx is required");
  MVG_REQUIRE((gamma == nullptr) == (dy_sinv == nullptr), "bn_bwd_reduce_split: gamma and dy_sinv go together");
  return bn_bwd_reduce_impl<float>(g, nullptr, y, mean, invstd, relu_scale, relu_shift, groups, rows_per_group, c, s1, s2, dgamma,
                                   dbeta, accumulate, workspace, dz_out, stream, relu_bits, mx, gamma, dy_sinv);
}

// shared by the unscaled entry point (null scales: its behaviour and its argument checks are what they were) and the scaled one
static int bn_apply_split_impl(const float *y, const float *scale, const float *shift, const void *residual, int residual_sp,
                               const float *res_scale, const float *res_shift, const float *res_sinv, int relu, void *out_sp,
                               const float *out_sinv, uint8_t *relu_bits, int groups, int64_t rows_per_group, int c, void *stream) {
  if (int e = require_c8("bn_apply_split", c)) return e;
  MVG_REQUIRE(!(residual_sp && res_scale), "bn_apply_split: an sp residual is already normalised (no res_scale / res_shift)");
  MVG_REQUIRE((res_scale == nullptr) == (res_shift == nullptr) && (residual || !res_scale),
              "bn_apply_split: res_scale / res_shift go together and need a residual");
  hipStream_t st = (hipStream_t)stream;
  const long long n8 = rows_per_group * (c / 8);
  ProfScope ps(MVG_K_BN_APPLY, st, 0.0, 8.0 * groups * (double)n8 * (4.0 + SP_BYTES + (residual ? (residual_sp ? (double)SP_BYTES : 4.0) : 0.0)));
  const dim3 grid(stream_geometry(n8, c / 8).grid, groups), block(256);
  if (residual && residual_sp)
    hipLaunchKernelGGL(bn_apply_sp_kernel<true>, grid, block, 0, st, y, scale, shift, residual, res_scale, res_shift, relu,
                       (sp_t *)out_sp, n8, c / 8, c, (unsigned short *)relu_bits, out_sinv, res_sinv);
  else
    hipLaunchKernelGGL(bn_apply_sp_kernel<false>, grid, block, 0, st, y, scale, shift, residual, res_scale, res_shift, relu,
                       (sp_t *)out_sp, n8, c / 8, c, (unsigned short *)relu_bits, out_sinv, res_sinv);
  return check_launch("bn_apply_split");
}

// out_sinv / res_sinv (device scalars from mvg_act_scales, or NULL = unscaled): the 2^-k of the sp output and of an sp identity
int mvg_bn_apply_split_scaled(const float *y, const float *scale, const float *shift, const void *residual, int residual_sp,
                              const float *res_scale, const float *res_shift, const float *res_sinv, int relu, void *out_sp,
                              const float *out_sinv, uint8_t *relu_bits, int groups, int64_t rows_per_group, int c, void *stream) {
  MVG_REQUIRE(y && scale && shift && out_sp, "bn_apply_split: y, scale, shift and out_sp are required");
  MVG_REQUIRE(groups > 0 && groups < 65536 && rows_per_group > 0 && c > 0, "bn_apply_split: bad sizes");
  MVG_REQUIRE(!res_sinv || (residual && residual_sp), "bn_apply_split: res_sinv is the scale of an sp residual");
  return bn_apply_split_impl(y, scale, shift, residual, residual_sp, res_scale, res_shift, res_sinv, relu, out_sp, out_sinv, relu_bits,
                             groups, rows_per_group, c, stream);
}

int mvg_bn_apply_split(const float *y, const float *scale, const float *shift, const void *residual, int residual_sp,
                       const float *res_scale, const float *res_shift, int relu, void *out_sp, uint8_t *relu_bits, int groups,
                       int64_t rows_per_group, int c, void *stream) {
  return bn_apply_split_impl(y, scale, shift, residual, residual_sp, res_scale, res_shift, nullptr, relu, out_sp, nullptr, relu_bits,
                             groups, rows_per_group, c, stream);
}

// Every sp activation scale of a training step in one single-workgroup launch (act_scales_kernel).  items_dev: n records in
// DEVICE memory of { const float *gamma, *beta; int32 c; float sqrt(n - 1); int32 ident; int32 slot; } (32 bytes).
int mvg_act_scales(const void *items_dev, int n, float *slots, int n_slots, void *stream) {
  static_assert(sizeof(ActScaleItem) == 32, "ActScaleItem: the callers build 32-byte records");
  MVG_REQUIRE(items_dev && slots, "act_scales: items_dev and slots are required");
  MVG_REQUIRE(n >= 1 && n <= ACT_SCALE_MAX_ITEMS && n_slots >= 1, "act_scales: 1..%d records and at least one slot", ACT_SCALE_MAX_ITEMS);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_LAYOUT, st, 0.0, 0.0);
  hipLaunchKernelGGL(act_scales_kernel, dim3(1), dim3(1024), 0, st, (const ActScaleItem *)items_dev, n, slots, n_slots);
  return check_launch("act_scales");
}

int mvg_bn_bwd_apply_split(const float *g, const float *y, const float *mean, const float *invstd, const float *gamma,
                           const float *s1, const float *s2, const float *relu_scale, const float *relu_shift, int groups,
                           int64_t rows_per_group, int c, void *dy_sp, const float *mx, float *dy_sinv, int dy_sinv_ready, void *stream) {
  if (int e = require_c8("bn_bwd_apply_split", c)) return e;
  MVG_REQUIRE(mx && dy_sinv, "bn_bwd_apply_split: mx (max |masked gradient| per (group, channel) from the reduce pass) and dy_sinv are required");
  MVG_REQUIRE((relu_scale == nullptr) == (relu_shift == nullptr), "bn_bwd_apply_split: relu_scale and relu_shift go together");
  hipStream_t st = (hipStream_t)stream;
  const long long n8 = rows_per_group * (c / 8);
  ProfScope ps(MVG_K_BN_BWD_APPLY, st, 0.0, 8.0 * groups * (double)n8 * (8.0 + SP_BYTES));
  if (ensure_dy_scale(dy_sinv_ready, gamma, invstd, s1, s2, mx, groups, c, rows_per_group, dy_sinv, st)) return 1;
  hipLaunchKernelGGL(bn_bwd_apply_sp_kernel, dim3(stream_geometry(n8, c / 8).grid, groups), dim3(256), 0, st, g, y, mean, invstd, gamma, s1, s2,
                     relu_scale, relu_shift, n8, 1.0f / (float)rows_per_group, c / 8, c, (sp_t *)dy_sp, dy_sinv);
  return check_launch("bn_bwd_apply_split");
}

// ---- frozen BatchNorm on the split path (Backbone.split_frozen) --------------------------------------------------------
int mvg_bn_frozen_finalize(const float *stats, int groups, int partials, int rows_per_partial, int64_t rows_per_group, int c,
                           const float *gamma, const float *beta, const float *running_mean, const float *running_var, float eps,
                           const float *ident_bound, float *mean, float *invstd, float *scale, float *shift, float *state,
                           float *slot, void *stream) {
  MVG_REQUIRE(stats && gamma && beta && running_mean && running_var && mean && invstd && scale && shift && state,
              "bn_frozen_finalize: stats, gamma, beta, the running statistics, mean, invstd, scale, shift and state are required");
  MVG_REQUIRE(groups > 0 && groups < 65536 && partials > 0 && rows_per_partial > 0 && c > 0 && rows_per_group > 0,
              "bn_frozen_finalize: bad sizes");
  MVG_REQUIRE((rows_per_group + rows_per_partial - 1) / rows_per_partial <= partials,
              "bn_frozen_finalize: %d partials of %d rows do not cover %lld rows", partials, rows_per_partial, (long long)rows_per_group);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_BN_FINALIZE, st, 0.0, 4.0 * groups * (double)partials * 2 * c);
  hipLaunchKernelGGL(bn_frozen_finalize_kernel, dim3(ceil_div(c, 8), groups), dim3(1024), 0, st, stats, partials, rows_per_partial,
                     (long long)rows_per_group, c, gamma, beta, running_mean, running_var, eps, ident_bound, mean, invstd, scale, shift,
                     (unsigned *)state, slot);
  return check_launch("bn_frozen_finalize");
}

int mvg_bn_frozen_bwd_apply_split(const float *g, const float *y, const float *invstd, const float *gamma, const float *relu_scale,
                                  const float *relu_shift, int groups, int64_t rows_per_group, int c, void *dy_sp,
                                  const float *dy_sinv, void *stream) {
  if (int e = require_c8("bn_frozen_bwd_apply_split", c)) return e;
  MVG_REQUIRE(g && invstd && gamma && dy_sp && dy_sinv, "bn_frozen_bwd_apply_split: g, invstd, gamma, dy_sp and dy_sinv are required");
  MVG_REQUIRE(groups > 0 && groups < 65536 && rows_per_group > 0, "bn_frozen_bwd_apply_split: bad sizes");
  MVG_REQUIRE((relu_scale == nullptr) == (relu_shift == nullptr), "bn_frozen_bwd_apply_split: relu_scale and relu_shift go together");
  MVG_REQUIRE(!relu_scale || y, "bn_frozen_bwd_apply_split: the mask from relu_scale / relu_shift needs y");
  hipStream_t st = (hipStream_t)stream;
  const long long n8 = rows_per_group * (c / 8);
  ProfScope ps(MVG_K_BN_BWD_APPLY, st, 0.0, 8.0 * groups * (double)n8 * ((relu_scale ? 8.0 : 4.0) + SP_BYTES));
  const dim3 grid(stream_geometry(n8, c / 8).grid, groups), block(256);
  if (relu_scale)
    hipLaunchKernelGGL(bn_frozen_bwd_apply_sp_kernel<true>, grid, block, 0, st, g, y, invstd, gamma, relu_scale, relu_shift, n8, c / 8, c,
                       (sp_t *)dy_sp, dy_sinv);
  else
    hipLaunchKernelGGL(bn_frozen_bwd_apply_sp_kernel<false>, grid, block, 0, st, g, y, invstd, gamma, relu_scale, relu_shift, n8, c / 8, c,
                       (sp_t *)dy_sp, dy_sinv);
  return check_launch("bn_frozen_bwd_apply_split");
}

int mvg_bn_relu_maxpool_fwd_split_scaled(const float *y, const float *scale, const float *shift, void *pooled_sp,
                                         const float *pooled_sinv, uint8_t *argmax, int groups, int n_per_group, int h, int w, int c,
                                         int ho, int wo, void *stream) {
  MVG_REQUIRE(y && scale && shift && pooled_sp && argmax, "bn_relu_maxpool_fwd_split: y, scale, shift, pooled_sp and argmax are required");
  MVG_REQUIRE(c % 8 == 0, "bn_relu_maxpool_fwd_split: c %% 8 != 0");
  return bn_relu_maxpool_fwd_impl<float, sp_t>(y, scale, shift, (sp_t *)pooled_sp, argmax, groups, n_per_group, h, w, c, ho, wo,
                                               stream, pooled_sinv);
}

int mvg_bn_relu_maxpool_fwd_split(const float *y, const float *scale, const float *shift, void *pooled_sp, uint8_t *argmax,
                                  int groups, int n_per_group, int h, int w, int c, int ho, int wo, void *stream) {
  MVG_REQUIRE(c % 8 == 0, "bn_relu_maxpool_fwd_split: c %% 8 != 0");
  return bn_relu_maxpool_fwd_impl<float, sp_t>(y, scale, shift, (sp_t *)pooled_sp, argmax, groups, n_per_group, h, w, c, ho, wo,
                                               stream);
}

// the stem tail's backward on the split path: the pooled gradient and y are fp32, dy goes to the stem's wgrad in sp;
// mx [groups][c] (from the reduce pass) bounds the gradient of a pixel: 4 x the largest masked window gradient
int mvg_bn_relu_maxpool_bwd_reduce_split(const float *g_pooled, const uint8_t *argmax, const float *y, const float *mean,
                                         const float *invstd, const float *scale, const float *shift, int groups, int n_per_group,
                                         int h, int w, int c, int ho, int wo, float *s1, float *s2, float *dgamma, float *dbeta,
                                         int accumulate, float *workspace, float *mx, const float *gamma, float *dy_sinv, void *stream) {
  MVG_REQUIRE(mx != nullptr, "bn_relu_maxpool_bwd_reduce_split: mx is required");
  MVG_REQUIRE((gamma == nullptr) == (dy_sinv == nullptr), "bn_relu_maxpool_bwd_reduce_split: gamma and dy_sinv go together");
  return bn_relu_maxpool_bwd_reduce_impl<float>(g_pooled, argmax, y, mean, invstd, scale, shift, groups, n_per_group, h, w, c, ho, wo,
                                                s1, s2, dgamma, dbeta, accumulate, workspace, stream, mx, gamma, dy_sinv);
}

int mvg_bn_relu_maxpool_bwd_apply_split(const float *g_pooled, const uint8_t *argmax, const float *y, const float *mean,
                                        const float *invstd, const float *gamma, const float *scale, const float *shift,
                                        const float *s1, const float *s2, int groups, int n_per_group, int h, int w, int c, int ho,
                                        int wo, void *dy_sp, const float *mx, float *dy_sinv, int dy_sinv_ready, void *stream) {
  MVG_REQUIRE(c % 8 == 0 && mx && dy_sinv, "bn_relu_maxpool_bwd_apply_split: c %% 8 != 0, or mx / dy_sinv missing");
  if (ensure_dy_scale(dy_sinv_ready, gamma, invstd, s1, s2, mx, groups, c, (long long)n_per_group * h * w, dy_sinv, (hipStream_t)stream)) return 1;
  return bn_relu_maxpool_bwd_apply_impl<float, sp_t>(g_pooled, argmax, y, mean, invstd, gamma, scale, shift, s1, s2, groups,
                                                     n_per_group, h, w, c, ho, wo, (sp_t *)dy_sp, stream, dy_sinv);
}

MVG_BN_BITS_FACES(, float)
MVG_BN_BITS_FACES(_bf16, uint16_t)
#undef MVG_BN_BITS_FACES

// ---- eval mode (running statistics): the one-pass backward and its stem-tail form ---------------------------------
size_t mvg_bn_eval_bwd_workspace_floats(int groups, int64_t rows_per_group, int c) {
  const int a = bwd_chunks(groups, rows_per_group, c), b = eval_pool_chunks(groups);
  return (size_t)groups * (a > b ? a : b) * 2 * c;
}

}  // extern "C"

template <typename T>
static int bn_eval_bwd_impl(const T *g, const T *act, const uint8_t *relu_bits, const T *y, const float *relu_scale,
                            const float *relu_shift, const float *gamma, const float *running_mean, const float *running_var, float eps,
                            int groups, int64_t rows_per_group, int c, T *dy, T *dz_out, float *dgamma, float *dbeta,
                            int accumulate, float *workspace, void *stream) {
  constexpr int W = Elem<T>::W;
  if (int e = require_one_mask("bn_eval_bwd", "ONE way: act, relu_bits or (relu_scale, relu_shift)", act, relu_bits, relu_scale, relu_shift))
    return e;
  MVG_REQUIRE(g && y && dy && gamma && running_mean && running_var && workspace,
              "bn_eval_bwd: g, y, dy, gamma, running_mean, running_var and workspace are required");
  MVG_REQUIRE(dz_out == nullptr || dz_out != dy, "bn_eval_bwd: dz_out and dy must be different buffers");
  MVG_REQUIRE(groups > 0 && groups < 65536 && rows_per_group > 0 && c > 0 && c % 4 == 0, "bn_eval_bwd: bad sizes");
  if (int e = require_channels("bn_eval_bwd", c, W)) return e;
  ReduceGeom q;
  if (int e = reduce_geometry("bn_eval_bwd", groups, rows_per_group, c, W, q)) return e;
  const int cwn = q.cwn, cw = q.cw, chunks = q.chunks;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_BN_BWD_APPLY, st, 0.0,
               Elem<T>::kBytes * groups * (double)rows_per_group * c * (3 + (act ? 1 : 0) + (dz_out ? 1 : 0)) +
                   (relu_bits ? groups * (double)rows_per_group * cwn : 0.0));
  hipLaunchKernelGGL(bn_eval_bwd_kernel<T>, dim3(chunks, ceil_div(cwn, cw), groups), dim3(256), 0, st, g, act, y, relu_bits, relu_scale,
                     relu_shift, gamma, running_mean, running_var, eps, (long long)rows_per_group, q.rows_per_chunk, c, cwn, cw, dy, dz_out, workspace,
                     chunks);
  if (check_launch("bn_eval_bwd")) return 1;
  if (!dgamma && !dbeta) return 0;
  hipLaunchKernelGGL(bn_eval_bwd_finalize_kernel, dim3(ceil_div(c, 16)), dim3(1024), 0, st, workspace, groups * chunks, c, dgamma, dbeta,
                     accumulate);
  return check_launch("bn_eval_bwd_finalize");
}

template <typename T>
static int bn_relu_maxpool_eval_bwd_impl(const T *g_pooled, const uint8_t *argmax, const T *y, const float *scale, const float *shift,
                                         const float *gamma, const float *running_mean, const float *running_var, float eps, int groups,
                                         int n_per_group, int h, int w, int c, int ho, int wo, T *dy, float *dgamma, float *dbeta,
                                         int accumulate, float *workspace, void *stream) {
  MVG_REQUIRE(g_pooled && argmax && y && scale && shift && gamma && running_mean && running_var && dy && workspace,
              "bn_relu_maxpool_eval_bwd: every pointer but dgamma / dbeta is required");
  if (int e = require_pool_eval_sizes(groups, n_per_group, h, w, c)) return e;
  MVG_REQUIRE(ho == (h + 2 - 3) / 2 + 1 && wo == (w + 2 - 3) / 2 + 1, "bn_relu_maxpool_eval_bwd: bad output size");
  hipStream_t st = (hipStream_t)stream;
  const int c4n = c / 4;
  const int chunks = eval_pool_grid(groups, n_per_group, h, w, c4n);
  ProfScope ps(MVG_K_BN_BWD_APPLY, st, 0.0,
               groups * (Elem<T>::kBytes * (double)n_per_group * h * w * c * 2 + (double)n_per_group * ho * wo * c * (Elem<T>::kBytes + 1.0)));
  hipLaunchKernelGGL(bn_pool_eval_bwd_kernel<T>, dim3(chunks, groups), dim3(256), 0, st, g_pooled, (const uchar4 *)argmax, y, scale,
                     shift, gamma, running_mean, running_var, eps, n_per_group, h, w, ho, wo, c4n, dy, workspace);
  if (check_launch("bn_relu_maxpool_eval_bwd")) return 1;
  if (!dgamma && !dbeta) return 0;
  hipLaunchKernelGGL(bn_eval_bwd_finalize_kernel, dim3(ceil_div(c, 16)), dim3(1024), 0, st, workspace, groups * chunks, c, dgamma,
                     dbeta, accumulate);
  return check_launch("bn_eval_bwd_finalize");
}

extern "C" {

// (fp32, and bf16 storage of g / act / y / dy / dz_out: the geometry of the bf16 train-mode reduce - c/8 divides 256 or
// exceeds it - and a relu_bits byte per 8 elements; the stem tail keeps 4 channels per lane in both)
#define MVG_BN_EVAL_FACES(SUFFIX, T)                                                                                             \
  int mvg_bn_eval_bwd##SUFFIX(const T *g, const T *act, const uint8_t *relu_bits, const T *y, const float *relu_scale,          \
                              const float *relu_shift, const float *gamma, const float *running_mean,                           \
                              const float *running_var, float eps, int groups, int64_t rows_per_group, int c, T *dy, T *dz_out, \
                              float *dgamma, float *dbeta, int accumulate, float *workspace, void *stream) {                    \
    return bn_eval_bwd_impl<T>(g, act, relu_bits, y, relu_scale, relu_shift, gamma, running_mean, running_var, eps, groups,     \
                               rows_per_group, c, dy, dz_out, dgamma, dbeta, accumulate, workspace, stream);                    \
  }                                                                                                                              \
  int mvg_bn_relu_maxpool_eval_bwd##SUFFIX(const T *g_pooled, const uint8_t *argmax, const T *y, const float *scale,            \
                                           const float *shift, const float *gamma, const float *running_mean,                   \
                                           const float *running_var, float eps, int groups, int n_per_group, int h, int w,      \
                                           int c, int ho, int wo, T *dy, float *dgamma, float *dbeta, int accumulate,           \
                                           float *workspace, void *stream) {                                                    \
    return bn_relu_maxpool_eval_bwd_impl<T>(g_pooled, argmax, y, scale, shift, gamma, running_mean, running_var, eps, groups,   \
                                            n_per_group, h, w, c, ho, wo, dy, dgamma, dbeta, accumulate, workspace, stream);    \
  }

MVG_BN_EVAL_FACES(, float)
MVG_BN_EVAL_FACES(_bf16, uint16_t)
#undef MVG_BN_EVAL_FACES

// ---- host-only plan query: the geometry functions above, asked without launching -----------------------------------
static int bn_plan_impl(int pass, int elem, int groups, int64_t rows_per_group, int c, int n_per_group, int h, int w, int partials,
                        size_t scratch_floats, mvg_bn_plan &p) {
  MVG_REQUIRE(elem == MVG_BN_ELEM_FP32 || elem == MVG_BN_ELEM_BF16 || elem == MVG_BN_ELEM_SP, "bn_plan_query: unknown element kind %d", elem);
  MVG_REQUIRE(groups > 0 && groups < 65536 && c > 0, "bn_plan_query: bad sizes");
  const int W = elem == MVG_BN_ELEM_BF16 ? 2 : 1;      // float4 groups per 16-byte access of the reduce-type kernels
  if (pass == MVG_BN_PASS_APPLY || pass == MVG_BN_PASS_BWD_APPLY) {
    MVG_REQUIRE(rows_per_group > 0, "bn_plan_query: bad sizes");
    const char *who = pass == MVG_BN_PASS_APPLY ? "bn_apply" : "bn_bwd_apply";
    int cwn;
    if (elem == MVG_BN_ELEM_SP) {        // bn_apply_sp_kernel / bn_bwd_apply_sp_kernel: 8 channels per lane
      if (int e = require_c8(pass == MVG_BN_PASS_APPLY ? "bn_apply_split" : "bn_bwd_apply_split", c)) return e;
      cwn = c / 8;
    } else {
      if (int e = require_channels(who, c, W)) return e;
      cwn = c / 4 / W;
    }
    p.accesses_per_group = rows_per_group * cwn;
    const StreamGeom s = stream_geometry(p.accesses_per_group, cwn);
    p.grid_x = s.grid;
    p.trips = s.trips;
    p.step = s.step;
    return 0;
  }
  if (pass == MVG_BN_PASS_BWD_REDUCE || pass == MVG_BN_PASS_EVAL_BWD || pass == MVG_BN_PASS_POOL_BWD_REDUCE) {
    const bool pool = pass == MVG_BN_PASS_POOL_BWD_REDUCE;
    const char *who = pass == MVG_BN_PASS_BWD_REDUCE ? "bn_bwd_reduce" : pool ? "bn_relu_maxpool_bwd_reduce" : "bn_eval_bwd";
    MVG_REQUIRE(pass != MVG_BN_PASS_EVAL_BWD || elem == MVG_BN_ELEM_FP32, "bn_plan_query: the eval-mode backward is fp32 only");
    if (pool) MVG_REQUIRE(n_per_group > 0 && h > 0 && w > 0, "bn_plan_query: bad sizes");
    const long long rows = pool ? (long long)n_per_group * h * w : (long long)rows_per_group;
    MVG_REQUIRE(rows > 0, "bn_plan_query: bad sizes");
    const int Wg = pool ? 1 : W;         // the pooled reduce reads 4 channels per lane whatever the storage
    if (int e = require_channels(who, c, Wg)) return e;
    ReduceGeom q;
    if (int e = reduce_geometry(who, groups, rows, c, Wg, q)) return e;
    p.cwn = q.cwn;
    p.cw = q.cw;
    p.column_blocks = ceil_div(q.cwn, q.cw);
    p.row_lanes = 256 / q.cw;
    if (pool) {
      int lpc = 0;
      p.chunks = pool_reduce_chunks(q.chunks, n_per_group * ((h - 1) / 2 + 1), lpc);
      p.rows_per_chunk = lpc;
      p.empty_chunks = 0;
    } else {
      p.chunks = q.chunks;
      p.rows_per_chunk = q.rows_per_chunk;
      p.empty_chunks = q.chunks - (int)((rows + q.rows_per_chunk - 1) / q.rows_per_chunk);
    }
    p.workspace_floats = (int64_t)groups * p.chunks * (pass == MVG_BN_PASS_EVAL_BWD ? 2 : elem == MVG_BN_ELEM_SP ? 3 : 2) * c;
    return 0;
  }
  if (pass == MVG_BN_PASS_POOL_EVAL_BWD) {
    MVG_REQUIRE(elem == MVG_BN_ELEM_FP32, "bn_plan_query: the eval-mode backward is fp32 only");
    if (int e = require_pool_eval_sizes(groups, n_per_group, h, w, c)) return e;
    p.cwn = p.cw = c / 4;
    p.column_blocks = 1;
    p.row_lanes = 256 / p.cw;
    p.chunks = eval_pool_grid(groups, n_per_group, h, w, c / 4);
    p.rows_per_chunk = 0;                // a grid-stride loop over (quad, channel group) items, not a range of rows
    p.empty_chunks = 0;
    p.workspace_floats = (int64_t)groups * p.chunks * 2 * c;
    return 0;
  }
  if (pass == MVG_BN_PASS_FINALIZE) {
    MVG_REQUIRE(groups > 0 && partials > 0 && c > 0 && rows_per_group > 0, "bn_finalize: bad sizes");
    const FinalizePlan f = finalize_plan(groups, partials, c, scratch_floats);
    p.form = f.form;
    p.lanes_per_group = f.lanes_per_group;
    p.slices = f.slices;
    p.partials_per_slice = f.per_slice;
    p.scratch_floats = (int64_t)(groups > 1 || partials >= 1024 ? f.need_floats : 0);
    return 0;
  }
  MVG_REQUIRE(false, "bn_plan_query: unknown pass %d", pass);
  return 0;
}

int mvg_bn_plan_query(int pass, int elem, int groups, int64_t rows_per_group, int c, int n_per_group, int h, int w, int partials,
                      size_t scratch_floats, mvg_bn_plan *out) {
  mvg_bn_plan plan;
  memset(&plan, 0, sizeof(plan));
  if (bn_plan_impl(pass, elem, groups, rows_per_group, c, n_per_group, h, w, partials, scratch_floats, plan)) return -1;
  if (out) *out = plan;
  return 0;
}

}  // extern "C"
