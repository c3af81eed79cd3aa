// Geometry, cross-view fusion operand builders, bias-gradient sums, the 2-wide gaze head and
// the angular loss.  All of these are tiny / HBM-bound next to the GEMMs.
#include <math.h>

#include "common.h"
#include "elem.h"

namespace mvg {

// R = Ry(yaw) @ Rx(-pitch)  (utils/math.py:188-219)
__global__ void rotation_matrix_kernel(const float *__restrict__ py, float *__restrict__ rot, int n, int inverse) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float p = -py[2 * i], y = py[2 * i + 1];
  const float cp = cosf(p), sp = sinf(p), cy = cosf(y), sy = sinf(y);
  float m[9] = {cy, sy * sp, sy * cp, 0.f, cp, -sp, -sy, cy * sp, cy * cp};
  float *o = rot + 9 * (long long)i;
  if (inverse) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) o[a * 3 + b] = m[b * 3 + a];
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = m[k];
  }
}

// rel[d][b] = rot[b][vi[d]] @ rot[b][vj[d]]^T
__global__ void relative_rotation_kernel(const float *__restrict__ rot, const int *__restrict__ vi,
                                         const int *__restrict__ vj, float *__restrict__ rel, int batch, int views,
                                         int dirs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= dirs * batch) return;
  const int d = i / batch, b = i - d * batch;
  const float *ra = rot + ((long long)b * views + vi[d]) * 9;
  const float *rb = rot + ((long long)b * views + vj[d]) * 9;
  float *o = rel + (long long)i * 9;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) o[r * 3 + c] = ra[r * 3 + 0] * rb[c * 3 + 0] + ra[r * 3 + 1] * rb[c * 3 + 1] + ra[r * 3 + 2] * rb[c * 3 + 2];
}

// x[(d,b)] = [ img_feat[view_of[d]][b] | rel[d][b] @ feat[src_of[d]][b] ]
__global__ __launch_bounds__(256) void rotcat_fwd_kernel(const float *__restrict__ img_feat,
                                                         const float *__restrict__ feat, const float *__restrict__ rel,
                                                         const int *__restrict__ view_of, const int *__restrict__ src_of,
                                                         float *__restrict__ x, int batch, int cf, int nvec) {
  const int row = blockIdx.x;            // d*batch + b
  const int d = row / batch, b = row - d * batch;
  const int kin = cf + 3 * nvec;
  float *xo = x + (long long)row * kin;
  const float4 *src = reinterpret_cast<const float4 *>(img_feat + ((long long)view_of[d] * batch + b) * cf);
  for (int i = threadIdx.x; i < cf / 4; i += 256) reinterpret_cast<float4 *>(xo)[i] = src[i];
  const float *f = feat + ((long long)src_of[d] * batch + b) * 3 * nvec;
  float r[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  if (rel) {
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = rel[(long long)row * 9 + k];
  }
  for (int k = threadIdx.x; k < nvec; k += 256) {
    const float f0 = f[k], f1 = f[nvec + k], f2 = f[2 * nvec + k];
    xo[cf + k] = r[0] * f0 + r[1] * f1 + r[2] * f2;
    xo[cf + nvec + k] = r[3] * f0 + r[4] * f1 + r[5] * f2;
    xo[cf + 2 * nvec + k] = r[6] * f0 + r[7] * f1 + r[8] * f2;
  }
}

// dfeat[src_of[d]][b] = rel^T @ dx_rot
__global__ __launch_bounds__(256) void rotcat_bwd_feat_kernel(const float *__restrict__ dx, const float *__restrict__ rel,
                                                              const int *__restrict__ src_of, float *__restrict__ dfeat,
                                                              int batch, int cf, int nvec) {
  const int row = blockIdx.x;
  const int d = row / batch, b = row - d * batch;
  const int kin = cf + 3 * nvec;
  const float *g = dx + (long long)row * kin + cf;
  float *o = dfeat + ((long long)src_of[d] * batch + b) * 3 * nvec;
  float r[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  if (rel) {
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = rel[(long long)row * 9 + k];
  }
  for (int k = threadIdx.x; k < nvec; k += 256) {
    const float g0 = g[k], g1 = g[nvec + k], g2 = g[2 * nvec + k];
    o[k] = r[0] * g0 + r[3] * g1 + r[6] * g2;
    o[nvec + k] = r[1] * g0 + r[4] * g1 + r[7] * g2;
    o[2 * nvec + k] = r[2] * g0 + r[5] * g1 + r[8] * g2;
  }
}

// ---- ablation variants (rot_mv.py:53-86,136-171) -------------------------------------------------
// encode_rotmat: x[(d,b)] = [ img_feat | feat (NOT rotated) | rel flattened (9) | zeros to ld ]
__global__ __launch_bounds__(256) void rotcat_ext_fwd_kernel(const float *__restrict__ img_feat,
                                                             const float *__restrict__ feat,
                                                             const float *__restrict__ rel_apply,
                                                             const float *__restrict__ rel_append,
                                                             const int *__restrict__ view_of, const int *__restrict__ src_of,
                                                             float *__restrict__ x, int ld, int batch, int cf, int nvec) {
  const int row = blockIdx.x;            // d*batch + b
  const int d = row / batch, b = row - d * batch;
  float *xo = x + (long long)row * ld;
  const float4 *src = reinterpret_cast<const float4 *>(img_feat + ((long long)view_of[d] * batch + b) * cf);
  for (int i = threadIdx.x; i < cf / 4; i += 256) reinterpret_cast<float4 *>(xo)[i] = src[i];
  const float *f = feat + ((long long)src_of[d] * batch + b) * 3 * nvec;
  float r[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  if (rel_apply) {
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = rel_apply[(long long)row * 9 + k];
  }
  for (int k = threadIdx.x; k < nvec; k += 256) {
    const float f0 = f[k], f1 = f[nvec + k], f2 = f[2 * nvec + k];
    xo[cf + k] = r[0] * f0 + r[1] * f1 + r[2] * f2;
    xo[cf + nvec + k] = r[3] * f0 + r[4] * f1 + r[5] * f2;
    xo[cf + 2 * nvec + k] = r[6] * f0 + r[7] * f1 + r[8] * f2;
  }
  const int tail = cf + 3 * nvec;
  for (int k = threadIdx.x; tail + k < ld; k += 256)
    xo[tail + k] = (rel_append && k < 9) ? rel_append[(long long)row * 9 + k] : 0.f;
}

__global__ __launch_bounds__(256) void rotcat_ext_bwd_kernel(const float *__restrict__ dx, int ld,
                                                             const float *__restrict__ rel, const int *__restrict__ src_of,
                                                             float *__restrict__ dfeat, int batch, int cf, int nvec) {
  const int row = blockIdx.x;
  const int d = row / batch, b = row - d * batch;
  const float *g = dx + (long long)row * ld + cf;
  float *o = dfeat + ((long long)src_of[d] * batch + b) * 3 * nvec;
  float r[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  if (rel) {
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = rel[(long long)row * 9 + k];
  }
  for (int k = threadIdx.x; k < nvec; k += 256) {
    const float g0 = g[k], g1 = g[nvec + k], g2 = g[2 * nvec + k];
    o[k] = r[0] * g0 + r[3] * g1 + r[6] * g2;
    o[nvec + k] = r[1] * g0 + r[4] * g1 + r[7] * g2;
    o[2 * nvec + k] = r[2] * g0 + r[5] * g1 + r[8] * g2;
  }
}

// share_feature: the IntensityBatchNorm scales of one iteration.  The reference calls the fuser's ONE
// normaliser 2*dirs times in sequence (direction 0: feat_0 then feat_1, direction 1: ...); in training
// every call first moves running_mean towards the batch std of the column norms, then divides by
// (running_mean + eps).  One thread per column k walks the calls in that order.  The norm of a
// rotated column equals the norm of the column (rel is orthonormal), so feat is read unrotated.
__global__ __launch_bounds__(256) void ibn_scales_kernel(const float *__restrict__ a, const float *__restrict__ feat,
                                                         const int *__restrict__ view_of, const int *__restrict__ src_of,
                                                         float *__restrict__ running_mean, int training, float momentum,
                                                         float eps, float *__restrict__ scales, int batch, int dirs,
                                                         int nvec) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= nvec) return;
  float rm = running_mean[k];
  for (int call = 0; call < 2 * dirs; ++call) {
    const int d = call >> 1;
    const float *src = (call & 1) ? feat + (long long)src_of[d] * batch * 3 * nvec : a + (long long)view_of[d] * batch * 3 * nvec;
    if (training) {
      // biased variance over the batch of the column norm (two passes, like torch.var)
      double sum = 0.0;
      for (int b = 0; b < batch; ++b) {
        const float *x = src + (long long)b * 3 * nvec + k;
        const float x0 = x[0], x1 = x[nvec], x2 = x[2 * nvec];
        sum += (double)sqrtf(x0 * x0 + x1 * x1 + x2 * x2);
      }
      const double mean = sum / batch;
      double m2 = 0.0;
      for (int b = 0; b < batch; ++b) {
        const float *x = src + (long long)b * 3 * nvec + k;
        const float x0 = x[0], x1 = x[nvec], x2 = x[2 * nvec];
        const double dlt = (double)sqrtf(x0 * x0 + x1 * x1 + x2 * x2) - mean;
        m2 += dlt * dlt;
      }
      const float var = (float)(m2 / batch);
      const float sd = sqrtf(fmaxf(var, eps));
      rm = rm * (1.f - momentum) + sd * momentum;
    }
    scales[(long long)call * nvec + k] = 1.f / (rm + eps);
  }
  if (training) running_mean[k] = rm;
}

// x[(d,b)][axis][0:nvec] = s0 * a[view_of[d]][b][axis][:],  [nvec:2nvec] = s1 * (rel @ feat[src_of[d]][b])[axis][:]
__global__ __launch_bounds__(256) void paircat_fwd_kernel(const float *__restrict__ a, const float *__restrict__ feat,
                                                          const float *__restrict__ rel, const float *__restrict__ scales,
                                                          const int *__restrict__ view_of, const int *__restrict__ src_of,
                                                          float *__restrict__ x, int batch, int nvec) {
  const int row = blockIdx.x;
  const int d = row / batch, b = row - d * batch;
  float *xo = x + (long long)row * 6 * nvec;
  const float *pa = a + ((long long)view_of[d] * batch + b) * 3 * nvec;
  const float *f = feat + ((long long)src_of[d] * batch + b) * 3 * nvec;
  float r[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  if (rel) {
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = rel[(long long)row * 9 + k];
  }
  for (int k = threadIdx.x; k < nvec; k += 256) {
    const float s0 = scales ? scales[(long long)(2 * d) * nvec + k] : 1.f;
    const float s1 = scales ? scales[(long long)(2 * d + 1) * nvec + k] : 1.f;
    const float f0 = f[k], f1 = f[nvec + k], f2 = f[2 * nvec + k];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      xo[ax * 2 * nvec + k] = pa[ax * nvec + k] * s0;
      xo[ax * 2 * nvec + nvec + k] = (r[3 * ax] * f0 + r[3 * ax + 1] * f1 + r[3 * ax + 2] * f2) * s1;
    }
  }
}

// da_dir[(d,b)][axis][k] = s0 * dx[..][axis][k];   dfeat[src_of[d]][b] = rel^T @ (s1 * dx[..][axis][nvec + k])
__global__ __launch_bounds__(256) void paircat_bwd_kernel(const float *__restrict__ dx, const float *__restrict__ rel,
                                                          const float *__restrict__ scales, const int *__restrict__ src_of,
                                                          float *__restrict__ da_dir, float *__restrict__ dfeat, int batch,
                                                          int nvec) {
  const int row = blockIdx.x;
  const int d = row / batch, b = row - d * batch;
  const float *g = dx + (long long)row * 6 * nvec;
  float *oa = da_dir + (long long)row * 3 * nvec;
  float *of = dfeat + ((long long)src_of[d] * batch + b) * 3 * nvec;
  float r[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  if (rel) {
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = rel[(long long)row * 9 + k];
  }
  for (int k = threadIdx.x; k < nvec; k += 256) {
    const float s0 = scales ? scales[(long long)(2 * d) * nvec + k] : 1.f;
    const float s1 = scales ? scales[(long long)(2 * d + 1) * nvec + k] : 1.f;
    float gr[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      oa[ax * nvec + k] = g[ax * 2 * nvec + k] * s0;
      gr[ax] = g[ax * 2 * nvec + nvec + k] * s1;
    }
    of[k] = r[0] * gr[0] + r[3] * gr[1] + r[6] * gr[2];
    of[nvec + k] = r[1] * gr[0] + r[4] * gr[1] + r[7] * gr[2];
    of[2 * nvec + k] = r[2] * gr[0] + r[5] * gr[1] + r[8] * gr[2];
  }
}

// ---- the fusion block on the split-operand kernels: operand builders that write sp directly ---------------------------
// max |x| of up to 8 small tensors in one launch (grid.y = tensor): out[i] receives the float's bits by atomicMax (the
// caller clears the slots); the bounds the builders below scale by (image features, lifted features, hidden-layer biases)
// max over the workgroup (256 threads) of a non-negative value, then ONE atomicMax of its bits (atomics on one address
// serialise at the memory side, ~12 ns each: one per wave of a 1500-workgroup launch costs more than the launch's work)
__device__ __forceinline__ void block_atomic_absmax(float m, unsigned *__restrict__ slot) {
  __shared__ float wred[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
    if (t > 0.f) atomicMax(slot, __float_as_uint(t));
  }
}
struct AbsMaxItems {
  const float *p[8];
  long long n[8];
  unsigned *out[8];
};
__global__ __launch_bounds__(256) void absmax_multi_kernel(AbsMaxItems it) {
  const float *__restrict__ x = it.p[blockIdx.y];
  const long long n = it.n[blockIdx.y];
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) m = fmaxf(m, fabsf(x[i]));
  block_atomic_absmax(m, it.out[blockIdx.y]);
}

__device__ __forceinline__ void ld8f(const float *p, float (&v)[8]) {
  const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void st_sp_chunk(uint4 *dst, const float (&v)[8], float scale) {
  float w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = v[k] * scale;
  uint4 q1, q2;
  split2_chunk(w, q1, q2);
  dst[0] = q1;
  dst[1] = q2;
}

// One launch builds, in sp and scaled, the two operands that depend on a feature tensor F (rot_mv.py:44-50,234-239,249-254):
//   xf[m] = [ img[row_img[m]] | rel[m] @ F[row_src_f[m]] ]   the NEXT fusion iteration's fuser input (may be null)
//   xh[m] = [ img[row_img[m]] |          F[row_src_h[m]] ]   this iteration's gaze-head input       (may be null)
// Scales: |rel @ f| <= |f|_2 <= sqrt(3) max |f| (rel is orthonormal), so xf is stored times the 2^k that
// max(am_img, sqrt(3) am_feat) allows and xh times the one max(am_img, am_feat) allows (am_*: float bits left by
// absmax_multi_kernel / the producing GEMM's epilogue); *xf_sinv / *xh_sinv receive 2^-k.  One workgroup per row.
__global__ __launch_bounds__(256) void fuse_build_split_kernel(const float *__restrict__ img, const float *__restrict__ feat,
                                                               const float *__restrict__ rel, const int *__restrict__ row_img,
                                                               const int *__restrict__ row_src_f, const int *__restrict__ row_src_h,
                                                               uint4 *__restrict__ xf, uint4 *__restrict__ xh,
                                                               const unsigned *__restrict__ am_img, const unsigned *__restrict__ am_feat,
                                                               float *__restrict__ xf_sinv, float *__restrict__ xh_sinv, int cf, int nvec) {
  const int m = blockIdx.x;
  const float ai = __uint_as_float(*am_img), af = __uint_as_float(*am_feat);
  const float sf = sp_scale_for(fmaxf(ai, 1.7320509f * af)), sh = sp_scale_for(fmaxf(ai, af));
  if (m == 0 && threadIdx.x == 0) {
    if (xf) *xf_sinv = 1.f / sf;
    if (xh) *xh_sinv = 1.f / sh;
  }
  const int c8i = cf >> 3, c8v = nvec >> 3, c8row = c8i + 3 * c8v;
  const float *src = img + (long long)row_img[m] * cf;
  for (int c8 = threadIdx.x; c8 < c8i; c8 += 256) {
    float v[8];
    ld8f(src + 8 * c8, v);
    if (xf) st_sp_chunk(xf + SP_NP * ((long long)m * c8row + c8), v, sf);
    if (xh) st_sp_chunk(xh + SP_NP * ((long long)m * c8row + c8), v, sh);
  }
  float r[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  if (rel) {
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = rel[(long long)m * 9 + k];
  }
  for (int t = threadIdx.x; t < 3 * c8v; t += 256) {
    const int a = t / c8v, k8 = t - a * c8v;
    if (xf) {
      const float *f = feat + (long long)row_src_f[m] * 3 * nvec + 8 * k8;
      float f0[8], f1[8], f2[8], o[8];
      ld8f(f, f0);
      ld8f(f + nvec, f1);
      ld8f(f + 2 * nvec, f2);
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = r[3 * a] * f0[k] + r[3 * a + 1] * f1[k] + r[3 * a + 2] * f2[k];     // rotcat_fwd_kernel's expression
      st_sp_chunk(xf + SP_NP * ((long long)m * c8row + c8i + t), o, sf);
    }
    if (xh) {
      float o[8];
      ld8f(feat + (long long)row_src_h[m] * 3 * nvec + a * nvec + 8 * k8, o);
      st_sp_chunk(xh + SP_NP * ((long long)m * c8row + c8i + t), o, sh);
    }
  }
}

// The backward of the builders, ONE launch per iteration: from the gradients of the operands that were built from F
// (dxh: the head input's, rows = directions; dxn: the next iteration's fuser input's) to
//   dF[(s,b)] = dxh[(s,b)][cf:] + sum over d with seg[d] == s (ascending) of rel[(d,b)]^T @ dxn[(d,b)][cf:]        blocks [0, S B)
//   da[(v,b)] (+)= sum over d with vi[d] == v of (dxh[(d,b)][:cf] + dxn[(d,b)][:cf])                                blocks [S B, S B + V B)
// (segments: the partner direction for F_it, the source VIEW for the lifted features of iteration 0) and max |dF| into
// *absmax (float bits, atomicMax) for the split of dF that follows.
__global__ __launch_bounds__(256) void fuse_unbuild_kernel(const float *__restrict__ dxh, const float *__restrict__ dxn,
                                                           const float *__restrict__ rel, const int *__restrict__ seg,
                                                           const int *__restrict__ vi, float *__restrict__ dF, float *__restrict__ da,
                                                           int da_accumulate, int S, int V, int D, int B, int cf, int nvec,
                                                           unsigned *__restrict__ absmax, int rows_per_block) {
  const int kin = cf + 3 * nvec;
  const int fblocks = (S * B + rows_per_block - 1) / rows_per_block;
  if ((int)blockIdx.x < fblocks) {
    float mx = 0.f;
    for (int rr = 0; rr < rows_per_block; ++rr) {
      const int row_o = blockIdx.x * rows_per_block + rr;
      if (row_o >= S * B) break;
      const int s = row_o / B, b = row_o - s * B;
      for (int k = threadIdx.x; k < nvec; k += 256) {
        float o0 = 0.f, o1 = 0.f, o2 = 0.f;
        if (dxh) {
          const float *g = dxh + ((long long)s * B + b) * kin + cf;
          o0 = g[k];
          o1 = g[nvec + k];
          o2 = g[2 * nvec + k];
        }
        if (dxn)
          for (int d = 0; d < D; ++d) {
            if (seg[d] != s) continue;
            const long long row = (long long)d * B + b;
            const float *g = dxn + row * kin + cf;
            const float g0 = g[k], g1 = g[nvec + k], g2 = g[2 * nvec + k];
            if (rel) {
              const float *r = rel + row * 9;
              o0 += r[0] * g0 + r[3] * g1 + r[6] * g2;             // rotcat_bwd_feat_kernel's expressions
              o1 += r[1] * g0 + r[4] * g1 + r[7] * g2;
              o2 += r[2] * g0 + r[5] * g1 + r[8] * g2;
            } else {
              o0 += g0;
              o1 += g1;
              o2 += g2;
            }
          }
        float *o = dF + ((long long)s * B + b) * 3 * nvec;
        o[k] = o0;
        o[nvec + k] = o1;
        o[2 * nvec + k] = o2;
        mx = fmaxf(mx, fmaxf(fabsf(o0), fmaxf(fabsf(o1), fabsf(o2))));
      }
    }
    if (absmax) block_atomic_absmax(mx, absmax);
    return;
  }
  const int t = blockIdx.x - fblocks;
  const int v = t / B, b = t - v * B;
  for (int cq = threadIdx.x; cq < cf / 4; cq += 256) {
    float4 *o = reinterpret_cast<float4 *>(da + ((long long)v * B + b) * cf) + cq;
    float4 acc = da_accumulate ? *o : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int d = 0; d < D; ++d) {
      if (vi[d] != v) continue;
      const long long row = (long long)d * B + b;
      if (dxh) {
        const float4 g = reinterpret_cast<const float4 *>(dxh + row * kin)[cq];
        acc.x += g.x; acc.y += g.y; acc.z += g.z; acc.w += g.w;
      }
      if (dxn) {
        const float4 g = reinterpret_cast<const float4 *>(dxn + row * kin)[cq];
        acc.x += g.x; acc.y += g.y; acc.z += g.z; acc.w += g.w;
      }
    }
    *o = acc;
  }
}

// out[v][b][0:width] (+)= sum over d with seg_of[d] == v (ascending d: reproducible) of x rows
__global__ __launch_bounds__(256) void segment_sum_kernel(const float *__restrict__ x, long long row_stride, int w4n,
                                                          const int *__restrict__ seg_of, float *__restrict__ out,
                                                          int batch, int dirs, int segments, int accumulate) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // over segments*batch*width/4
  if (i >= (long long)segments * batch * w4n) return;
  const int cq = (int)(i % w4n);
  const long long t = i / w4n;
  const int b = (int)(t % batch), v = (int)(t / batch);
  float4 s = accumulate ? reinterpret_cast<float4 *>(out)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int d = 0; d < dirs; ++d) {
    if (seg_of[d] != v) continue;
    const float4 g = reinterpret_cast<const float4 *>(x + ((long long)d * batch + b) * row_stride)[cq];
    s.x += g.x; s.y += g.y; s.z += g.z; s.w += g.w;
  }
  reinterpret_cast<float4 *>(out)[i] = s;
}

__global__ __launch_bounds__(256) void scale_by_kernel(const float *__restrict__ x, const float *__restrict__ scale,
                                                       float *__restrict__ out, long long n) {
  const float s = scale[0];
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) out[i] = x[i] * s;
}

// out[c] (+)= sum_rows x[rows][c] : block = 64 channels x 4 row lanes
__global__ __launch_bounds__(256) void axpby_kernel(const float *__restrict__ x, float *__restrict__ y, float a, float b,
                                                    long long n) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) y[i] = a * x[i] + (b != 0.f ? b * y[i] : 0.f);
}

// ---- skinny linear (out_features <= 4): the Linear(512 -> 2) of the gaze head ------------------
// fwd: one wave per row.
__global__ __launch_bounds__(256) void skinny_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                         const float *__restrict__ bias, float *__restrict__ y,
                                                         int rows, int k, int nout) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = lane; i < k; i += 64) {
    const float v = x[(long long)row * k + i];
    for (int j = 0; j < nout; ++j) acc[j] += v * w[(long long)j * k + i];
  }
  for (int j = 0; j < nout; ++j) {
    const float s = wave_sum(acc[j]);
    if (lane == 0) y[(long long)row * nout + j] = s + (bias ? bias[j] : 0.f);
  }
}
// bwd: dx[m][i] = mask * sum_j dy[m][j] w[j][i]
__global__ __launch_bounds__(256) void skinny_bwd_dx_kernel(const float *__restrict__ dy, const float *__restrict__ w,
                                                            const float *__restrict__ mask, float *__restrict__ dx,
                                                            long long total, int k, int nout, unsigned *__restrict__ absmax) {
  float mx = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long m = i / k;
    const int col = (int)(i - m * k);
    float s = 0.f;
    for (int j = 0; j < nout; ++j) s += dy[m * nout + j] * w[(long long)j * k + col];
    if (mask && !(mask[i] > 0.f)) s = 0.f;
    dx[i] = s;
    mx = fmaxf(mx, fabsf(s));
  }
  if (absmax) block_atomic_absmax(mx, absmax);     // max |dx| for the split of dx that follows (float bits, order-independent)
}
// dw[j][i] = sum_m dy[m][j] x[m][i];  db[j] = sum_m dy[m][j]
// 4 columns x 64 row lanes per workgroup (k / 4 workgroups: 128 for the gaze head's 512 inputs); the row lanes are summed
// through LDS in lane order (deterministic).  The bias gradient is summed by workgroup 0 with all of its threads - one
// thread per output walking all rows serially was 290 us of this kernel's 296 at C5's 3584 rows.
__global__ __launch_bounds__(256) void skinny_bwd_dw_kernel(const float *__restrict__ dy, const float *__restrict__ x,
                                                            float *__restrict__ dw, float *__restrict__ db, int rows,
                                                            int k, int nout, int accumulate) {
  __shared__ float sh[4][64][5];
  const int cl = threadIdx.x & 3, rl = threadIdx.x >> 2;
  const int i = blockIdx.x * 4 + cl;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (i < k)
    for (int m = rl; m < rows; m += 64) {
      const float v = x[(long long)m * k + i];
      for (int j = 0; j < nout; ++j) acc[j] += dy[(long long)m * nout + j] * v;
    }
  for (int j = 0; j < 4; ++j) sh[j][rl][cl] = acc[j];
  __syncthreads();
  if (rl < nout && i < k) {
    const int j = rl;
    float t = 0.f;
    for (int r = 0; r < 64; ++r) t += sh[j][r][cl];
    dw[(long long)j * k + i] = (accumulate ? dw[(long long)j * k + i] : 0.f) + t;
  }
  if (db && blockIdx.x == 0) {
    __shared__ float sb[4][256];
    float part[4] = {0.f, 0.f, 0.f, 0.f};
    for (int m = threadIdx.x; m < rows; m += 256)
      for (int j = 0; j < nout; ++j) part[j] += dy[(long long)m * nout + j];
    for (int j = 0; j < 4; ++j) sb[j][threadIdx.x] = part[j];
    __syncthreads();
    if (threadIdx.x < nout) {
      float t = 0.f;
      for (int r = 0; r < 256; ++r) t += sb[threadIdx.x][r];
      db[threadIdx.x] = (accumulate ? db[threadIdx.x] : 0.f) + t;
    }
  }
}

// ---- L1 / L2 loss of GazeLoss (losses/gaze_loss.py:56-64): mean |a - b|^p over all elements ----------
__global__ __launch_bounds__(256) void gaze_lp_loss_kernel(const float *__restrict__ pred, const float *__restrict__ label,
                                                           int n, int p, float *__restrict__ loss,
                                                           float *__restrict__ dpred) {
  __shared__ double sh[4];
  double local = 0.0;
  const float inv_n = 1.f / (float)n;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float d = pred[i] - label[i];
    const float a = fabsf(d);
    local += (double)(p == 1 ? a : a * a);
    if (dpred) {
      const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);      // torch.abs: zero gradient at 0
      dpred[i] = (p == 1 ? sgn : 2.f * a * sgn) * inv_n;
    }
  }
  local = wave_sum_d(local);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (float)((sh[0] + sh[1] + sh[2] + sh[3]) / (double)n);
}

// ---- angular loss ------------------------------------------------------------------------------
// v(p,y) = (cos p sin y, sin p, cos p cos y); sim = <u/|u|, v/|v|> with the norms clamped at 1e-6
// (ATen cosine_similarity); clamp to [-1,1] (hardtanh: zero gradient AT and beyond the bounds);
// theta = acos(sim) * 180/pi.
__global__ __launch_bounds__(256) void gaze_loss_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                        int n, float row_weight, float *__restrict__ loss,
                                                        int accumulate, float *__restrict__ dpred,
                                                        float *__restrict__ theta_out) {
  __shared__ double sh[4];
  double local = 0.0;
  const float k180 = 57.29577951308232f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float pp = pred[2 * i], py = pred[2 * i + 1], gp = gt[2 * i], gy = gt[2 * i + 1];
    const float cpp = cosf(pp), spp = sinf(pp), cpy = cosf(py), spy = sinf(py);
    const float cgp = cosf(gp), sgp = sinf(gp), cgy = cosf(gy), sgy = sinf(gy);
    const float v0 = cpp * spy, v1 = spp, v2 = cpp * cpy;
    const float u0 = cgp * sgy, u1 = sgp, u2 = cgp * cgy;
    const float nv = fmaxf(sqrtf(v0 * v0 + v1 * v1 + v2 * v2), 1e-6f);
    const float nu = fmaxf(sqrtf(u0 * u0 + u1 * u1 + u2 * u2), 1e-6f);
    const float a0 = u0 / nu, a1 = u1 / nu, a2 = u2 / nu;
    const float b0 = v0 / nv, b1 = v1 / nv, b2 = v2 / nv;
    const float sim = a0 * b0 + a1 * b1 + a2 * b2;
    const float sc = fminf(fmaxf(sim, -1.f), 1.f);
    const float theta = acosf(sc) * k180;
    local += (double)theta;
    if (theta_out) theta_out[i] = theta;
    if (dpred) {
      float gpitch = 0.f, gyaw = 0.f;
      if (sim > -1.f && sim < 1.f) {
        const float dth = -k180 / sqrtf(1.f - sc * sc);          // dtheta/dsim
        // dsim/dv = (a - sim*b)/|v|   (gradient through the normalisation)
        const float d0 = (a0 - sim * b0) / nv, d1 = (a1 - sim * b1) / nv, d2 = (a2 - sim * b2) / nv;
        // dv/dpitch = (-sin p sin y, cos p, -sin p cos y); dv/dyaw = (cos p cos y, 0, -cos p sin y)
        gpitch = dth * (d0 * (-spp * spy) + d1 * cpp + d2 * (-spp * cpy));
        gyaw = dth * (d0 * (cpp * cpy) + d2 * (-cpp * spy));
      }
      dpred[2 * i] = row_weight * gpitch;
      dpred[2 * i + 1] = row_weight * gyaw;
    }
  }
  local = wave_sum_d(local);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double tot = (sh[0] + sh[1] + sh[2] + sh[3]) * (double)row_weight;
    loss[0] = (accumulate ? loss[0] : 0.f) + (float)tot;
  }
}


// All iterations' angular losses in ONE launch (stereo_loss.py:65-84 over the head's stacked predictions): pred [iters][n][2],
// gt [n][2], row r of iteration i weighs w[i * dirs + r / batch] / batch; loss = the weighted sum (fp64 accumulation, one
// workgroup: fixed order), dpred = the weighted analytic gradient.
struct LossWeights {
  float w[512];
};
__global__ __launch_bounds__(256) void gaze_loss_multi_kernel(const float *__restrict__ pred, const float *__restrict__ gt, int iters,
                                                              int dirs, int batch, LossWeights lw, float *__restrict__ loss,
                                                              float *__restrict__ dpred) {
  __shared__ double sh[4];
  double local = 0.0;
  const float k180 = 57.29577951308232f;
  const int n = dirs * batch;
  const float inv_b = 1.f / (float)batch;
  for (int i = threadIdx.x; i < iters * n; i += 256) {
    const int it = i / n, r = i - it * n;
    const float row_weight = lw.w[it * dirs + r / batch] * inv_b;
    const float pp = pred[2 * i], py = pred[2 * i + 1], gp = gt[2 * r], gy = gt[2 * r + 1];
    const float cpp = cosf(pp), spp = sinf(pp), cpy = cosf(py), spy = sinf(py);
    const float cgp = cosf(gp), sgp = sinf(gp), cgy = cosf(gy), sgy = sinf(gy);
    const float v0 = cpp * spy, v1 = spp, v2 = cpp * cpy;
    const float u0 = cgp * sgy, u1 = sgp, u2 = cgp * cgy;
    const float nv = fmaxf(sqrtf(v0 * v0 + v1 * v1 + v2 * v2), 1e-6f);
    const float nu = fmaxf(sqrtf(u0 * u0 + u1 * u1 + u2 * u2), 1e-6f);
    const float a0 = u0 / nu, a1 = u1 / nu, a2 = u2 / nu;
    const float b0 = v0 / nv, b1 = v1 / nv, b2 = v2 / nv;
    const float sim = a0 * b0 + a1 * b1 + a2 * b2;
    const float sc = fminf(fmaxf(sim, -1.f), 1.f);
    const float theta = acosf(sc) * k180;
    local += (double)theta * (double)row_weight;
    if (dpred) {
      float gpitch = 0.f, gyaw = 0.f;
      if (sim > -1.f && sim < 1.f) {
        const float dth = -k180 / sqrtf(1.f - sc * sc);
        const float d0 = (a0 - sim * b0) / nv, d1 = (a1 - sim * b1) / nv, d2 = (a2 - sim * b2) / nv;
        gpitch = dth * (d0 * (-spp * spy) + d1 * cpp + d2 * (-spp * cpy));
        gyaw = dth * (d0 * (cpp * cpy) + d2 * (-cpp * spy));
      }
      dpred[2 * i] = row_weight * gpitch;
      dpred[2 * i + 1] = row_weight * gyaw;
    }
  }
  local = wave_sum_d(local);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (float)(sh[0] + sh[1] + sh[2] + sh[3]);
}

// ---- gaze error meter --------------------------------------------------------------------------
// The evaluation metric (utils/math.py:105-120, angular_error_numpy) in double, accumulated on the device: one workgroup per
// (iteration, direction) cell of the record, threads stride over the batch, fixed-order reduction (wave_sum_d, four wave
// partials, thread 0 adds into the cell) - no atomics; updates of a record are ordered by the stream.  The one deviation
// from the reference: the similarity is clamped to [-1, 1] before acos (pred == gt rounds to 1 + 2e-16 there and gives NaN).
// A row with a NaN / Inf input counts in NONFINITE only.  err_out (optional) [cells][capacity] fp32: row b goes to slot
// seen_before + b of its cell's row, seen_before = COUNT + NONFINITE as every thread reads it before the barrier in front of
// thread 0's write; slots >= capacity are not written.
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double dot3_d(double x0, double x1, double x2, double y0, double y1, double y2) {
  return fma(x2, y2, fma(x1, y1, x0 * y0));
}
__global__ __launch_bounds__(256) void gaze_error_update_kernel(const float *__restrict__ pred, const float *__restrict__ gt, int dirs,
                                                                int batch, double *record, float *__restrict__ err_out,
                                                                long long capacity) {
  __shared__ double sh[5][4];
  const int cell = blockIdx.x, d = cell % dirs;
  double *rec = record + (long long)cell * MVG_GAZE_ERR_FIELDS;
  const long long seen_before = (long long)(rec[MVG_GAZE_ERR_COUNT] + rec[MVG_GAZE_ERR_NONFINITE]);
  const float *p = pred + (long long)cell * batch * 2, *g = gt + (long long)d * batch * 2;
  float *eo = err_out ? err_out + (long long)cell * capacity : nullptr;
  double cnt = 0.0, sum = 0.0, sumsq = 0.0, mx = 0.0, bad = 0.0;
  for (int b = threadIdx.x; b < batch; b += 256) {
    const float ppf = p[2 * b], pyf = p[2 * b + 1], gpf = g[2 * b], gyf = g[2 * b + 1];
    const long long slot = seen_before + b;
    if (!(isfinite(ppf) && isfinite(pyf) && isfinite(gpf) && isfinite(gyf))) {
      bad += 1.0;
      if (eo && slot >= 0 && slot < capacity) eo[slot] = __builtin_nanf("");
      continue;
    }
    const double pp = (double)ppf, py = (double)pyf, gp = (double)gpf, gy = (double)gyf;
    const double cpp = cos(pp), spp = sin(pp), cgp = cos(gp), sgp = sin(gp);
    const double a0 = cpp * sin(py), a1 = spp, a2 = cpp * cos(py);
    const double b0 = cgp * sin(gy), b1 = sgp, b2 = cgp * cos(gy);
    // (one dot3 for all three products: with pred == gt they are the same bits s, sqrt rounds so that fl(sqrt(s))^2 <= s near 1,
    // the similarity is >= 1 and the clamp makes the row exactly 0)
    const double ab = dot3_d(a0, a1, a2, b0, b1, b2);
    const double na = fmax(sqrt(dot3_d(a0, a1, a2, a0, a1, a2)), 1e-7), nb = fmax(sqrt(dot3_d(b0, b1, b2, b0, b1, b2)), 1e-7);
    const double sim = fmin(fmax(ab / (na * nb), -1.0), 1.0);
    const double e = acos(sim) * 180.0 / 3.14159265358979323846;
    cnt += 1.0;
    sum += e;
    sumsq += e * e;
    mx = fmax(mx, e);
    if (eo && slot >= 0 && slot < capacity) eo[slot] = (float)e;
  }
  cnt = wave_sum_d(cnt);
  sum = wave_sum_d(sum);
  sumsq = wave_sum_d(sumsq);
  mx = wave_max_d(mx);
  bad = wave_sum_d(bad);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    sh[0][w] = cnt;
    sh[1][w] = sum;
    sh[2][w] = sumsq;
    sh[3][w] = mx;
    sh[4][w] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    rec[MVG_GAZE_ERR_COUNT] += sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
    rec[MVG_GAZE_ERR_SUM] += sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
    rec[MVG_GAZE_ERR_SUMSQ] += sh[2][0] + sh[2][1] + sh[2][2] + sh[2][3];
    rec[MVG_GAZE_ERR_MAX] = fmax(rec[MVG_GAZE_ERR_MAX], fmax(fmax(sh[3][0], sh[3][1]), fmax(sh[3][2], sh[3][3])));
    rec[MVG_GAZE_ERR_NONFINITE] += sh[4][0] + sh[4][1] + sh[4][2] + sh[4][3];
  }
}

// ---- multi-view consensus gaze -------------------------------------------------------------------
// One gaze per sample from all D = V (V - 1) directed pair predictions: each prediction goes to the head frame through its own
// view's rotation (rot[b][s]^T, the premise of mvg_relative_rotation), the weighted resultant h is normalised and rotated back
// into every view.  One thread per (iteration, sample) item, lanes along the batch (the pred / dpred rows of one direction are
// 8-byte accesses next to each other); the (s, q) of direction d comes from the nested i < j loop, kept rolled; all arithmetic
// in double like the meter above (a call has I * B items, a few thousand at most), results stored as fp32.  No LDS, no
// atomics, nothing depends on the launch geometry: equal calls leave equal bits.  An inactive contribution (w_d = weights[s] *
// weights[q] not > 0) is skipped - neither its pred row nor, unless another active contribution uses it, its view's rot is read
// into the sums.  The definition, in full, is at mvg_gaze_consensus_fwd in the header.
struct ConsSum {
  double h0, h1, h2, W;     // the weighted head-frame resultant and the weight total of the active contributions
  bool bad;                 // the item is degenerate for a reason other than |h| <= 1e-4 W
};
__device__ __forceinline__ bool cons_rot(const float *__restrict__ R, double (&m)[9]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float f = R[k];
    ok = ok && isfinite(f);
    m[k] = (double)f;
  }
  return ok;
}
// (pitch, yaw) -> the unit vector, and its image in the head frame m^T v
__device__ __forceinline__ void cons_head_vec(const double (&m)[9], double p, double y, double &c0, double &c1, double &c2) {
  const double cp = cos(p), v0 = cp * sin(y), v1 = sin(p), v2 = cp * cos(y);
  c0 = dot3_d(m[0], m[3], m[6], v0, v1, v2);
  c1 = dot3_d(m[1], m[4], m[7], v0, v1, v2);
  c2 = dot3_d(m[2], m[5], m[8], v0, v1, v2);
}
__device__ __forceinline__ double cons_weight(const float *__restrict__ wv, int s, int q) {
  return wv ? (double)wv[s] * (double)wv[q] : 1.0;
}
// P: the item's row of direction 0 (direction d is P[d * batch]); R: rot[b]; wv: weights[b] or null
__device__ __forceinline__ ConsSum cons_sum(const float2 *__restrict__ P, const float *__restrict__ R, const float *__restrict__ wv,
                                            int views, int batch) {
  ConsSum c = {0.0, 0.0, 0.0, 0.0, false};
  if (wv)
    for (int t = 0; t < views; ++t) {
      const float w = wv[t];
      if (!(isfinite(w) && w >= 0.f)) c.bad = true;
    }
  if (c.bad) return c;
  long long d = 0;
#pragma unroll 1
  for (int i = 0; i < views; ++i)
#pragma unroll 1
    for (int j = i + 1; j < views; ++j)
#pragma unroll 1
      for (int k = 0; k < 2; ++k, ++d) {
        const int s = k ? j : i, q = k ? i : j;
        const double w = cons_weight(wv, s, q);
        if (!(w > 0.0)) continue;
        const float2 pr = P[d * batch];
        double m[9], c0, c1, c2;
        const bool ok = cons_rot(R + s * 9, m);
        if (!(ok && isfinite(pr.x) && isfinite(pr.y))) {
          c.bad = true;
          continue;
        }
        cons_head_vec(m, (double)pr.x, (double)pr.y, c0, c1, c2);
        c.h0 = fma(w, c0, c.h0);
        c.h1 = fma(w, c1, c.h1);
        c.h2 = fma(w, c2, c.h2);
        c.W += w;
      }
  if (!(c.W > 0.0)) c.bad = true;
  return c;
}
__global__ __launch_bounds__(256) void gaze_consensus_fwd_kernel(const float *__restrict__ preds, const float *__restrict__ rot,
                                                                 const float *__restrict__ weights, int iters, int views, int batch,
                                                                 float *__restrict__ head, float *__restrict__ views_out,
                                                                 float *__restrict__ stats) {
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)iters * batch) return;
  const int it = (int)(item / batch), b = (int)(item - (long long)it * batch);
  const int dirs = views * (views - 1);
  const float2 *P = (const float2 *)preds + (long long)it * dirs * batch + b;
  const float *R = rot + (long long)b * views * 9, *wv = weights ? weights + (long long)b * views : nullptr;
  float2 *VO = (float2 *)views_out + (long long)it * views * batch + b;
  const float nanf_ = __builtin_nanf("");
  const ConsSum c = cons_sum(P, R, wv, views, batch);
  const double n = sqrt(dot3_d(c.h0, c.h1, c.h2, c.h0, c.h1, c.h2));
  if (c.bad || !(n > 1e-4 * c.W)) {           // degenerate: NaN everywhere
    head[3 * item] = head[3 * item + 1] = head[3 * item + 2] = nanf_;
    for (int t = 0; t < views; ++t) VO[(long long)t * batch] = make_float2(nanf_, nanf_);
    if (stats) stats[2 * item] = stats[2 * item + 1] = nanf_;
    return;
  }
  const double e0 = c.h0 / n, e1 = c.h1 / n, e2 = c.h2 / n;
  head[3 * item] = (float)e0;
  head[3 * item + 1] = (float)e1;
  head[3 * item + 2] = (float)e2;
#pragma unroll 1
  for (int t = 0; t < views; ++t) {           // every view gets the consensus in its own frame, whatever its weight
    double m[9];
    float2 o = make_float2(nanf_, nanf_);
    if (cons_rot(R + t * 9, m)) {
      const double u0 = dot3_d(m[0], m[1], m[2], e0, e1, e2), u1 = dot3_d(m[3], m[4], m[5], e0, e1, e2),
                   u2 = dot3_d(m[6], m[7], m[8], e0, e1, e2);
      o = make_float2((float)asin(fmin(fmax(u1, -1.0), 1.0)), (float)atan2(u0, u2));
    }
    VO[(long long)t * batch] = o;
  }
  if (!stats) return;
  double acc = 0.0;
  long long d = 0;
#pragma unroll 1
  for (int i = 0; i < views; ++i)
#pragma unroll 1
    for (int j = i + 1; j < views; ++j)
#pragma unroll 1
      for (int k = 0; k < 2; ++k, ++d) {
        const int s = k ? j : i, q = k ? i : j;
        const double w = cons_weight(wv, s, q);
        if (!(w > 0.0)) continue;
        const float2 pr = P[d * batch];
        double m[9], c0, c1, c2;
        cons_rot(R + s * 9, m);
        cons_head_vec(m, (double)pr.x, (double)pr.y, c0, c1, c2);
        acc = fma(w, acos(fmin(fmax(dot3_d(e0, e1, e2, c0, c1, c2), -1.0), 1.0)), acc);
      }
  stats[2 * item] = (float)(n / c.W);
  stats[2 * item + 1] = (float)(acc * (180.0 / 3.14159265358979323846) / c.W);
}
__global__ __launch_bounds__(256) void gaze_consensus_bwd_kernel(const float *__restrict__ dviews, const float *__restrict__ preds,
                                                                 const float *__restrict__ rot, const float *__restrict__ weights,
                                                                 int iters, int views, int batch, float *__restrict__ dpreds) {
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)iters * batch) return;
  const int it = (int)(item / batch), b = (int)(item - (long long)it * batch);
  const int dirs = views * (views - 1);
  const float2 *P = (const float2 *)preds + (long long)it * dirs * batch + b;
  float2 *DP = (float2 *)dpreds + (long long)it * dirs * batch + b;
  const float *R = rot + (long long)b * views * 9, *wv = weights ? weights + (long long)b * views : nullptr;
  const float2 *DV = (const float2 *)dviews + (long long)it * views * batch + b;
  const ConsSum c = cons_sum(P, R, wv, views, batch);
  const double n = sqrt(dot3_d(c.h0, c.h1, c.h2, c.h0, c.h1, c.h2));
  const bool degenerate = c.bad || !(n > 1e-4 * c.W);
  double g0 = 0.0, g1 = 0.0, g2 = 0.0;        // the gradient on h
  if (!degenerate) {
    const double e0 = c.h0 / n, e1 = c.h1 / n, e2 = c.h2 / n;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;      // the gradient on the unit vector: sum over the targets of rot[t]^T g_t
#pragma unroll 1
    for (int t = 0; t < views; ++t) {
      double m[9];
      if (!cons_rot(R + t * 9, m)) continue;  // its forward row is NaN: no gradient
      const double u0 = dot3_d(m[0], m[1], m[2], e0, e1, e2), u1 = dot3_d(m[3], m[4], m[5], e0, e1, e2),
                   u2 = dot3_d(m[6], m[7], m[8], e0, e1, e2);
      const double r2 = fma(u0, u0, u2 * u2), s1 = u1 * u1;
      if (r2 == 0.0 || s1 >= 1.0) continue;
      const float2 dv = DV[(long long)t * batch];
      const double dpitch = (double)dv.x, dyaw = (double)dv.y;
      const double t0 = dyaw * u2 / r2, t1 = dpitch / sqrt(1.0 - s1), t2 = -dyaw * u0 / r2;
      a0 += dot3_d(m[0], m[3], m[6], t0, t1, t2);
      a1 += dot3_d(m[1], m[4], m[7], t0, t1, t2);
      a2 += dot3_d(m[2], m[5], m[8], t0, t1, t2);
    }
    const double ae = dot3_d(a0, a1, a2, e0, e1, e2);
    g0 = (a0 - ae * e0) / n;
    g1 = (a1 - ae * e1) / n;
    g2 = (a2 - ae * e2) / n;
  }
  long long d = 0;
#pragma unroll 1
  for (int i = 0; i < views; ++i)
#pragma unroll 1
    for (int j = i + 1; j < views; ++j)
#pragma unroll 1
      for (int k = 0; k < 2; ++k, ++d) {
        const int s = k ? j : i, q = k ? i : j;
        float2 o = make_float2(0.f, 0.f);     // every row is written: inactive rows and degenerate items are exactly 0
        const double w = degenerate ? 0.0 : cons_weight(wv, s, q);
        if (w > 0.0) {
          const float2 pr = P[d * batch];
          double m[9];
          cons_rot(R + s * 9, m);
          const double v0 = w * dot3_d(m[0], m[1], m[2], g0, g1, g2), v1 = w * dot3_d(m[3], m[4], m[5], g0, g1, g2),
                       v2 = w * dot3_d(m[6], m[7], m[8], g0, g1, g2);
          const double p = (double)pr.x, y = (double)pr.y, sp = sin(p), cp = cos(p), sy = sin(y), cy = cos(y);
          o = make_float2((float)dot3_d(v0, v1, v2, -sp * sy, cp, -sp * cy), (float)(cp * fma(v0, cy, -v2 * sy)));
        }
        DP[d * batch] = o;
      }
}

}  // namespace mvg

using namespace mvg;

extern "C" {

int mvg_rotation_matrix_2d(const float *pitch_yaw, float *rot, int n, int inverse, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_GEOMETRY, st, 0.0, 44.0 * n);
  hipLaunchKernelGGL(rotation_matrix_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, pitch_yaw, rot, n, inverse);
  return check_launch("rotation_matrix_2d");
}

int mvg_relative_rotation(const float *rot, const int32_t *vi, const int32_t *vj, float *rel, int batch, int views,
                          int dirs, void *stream) {
  MVG_REQUIRE(batch > 0 && views > 0 && dirs > 0, "relative_rotation: batch, views and dirs must be positive");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_GEOMETRY, st, 0.0, 108.0 * dirs * batch);
  hipLaunchKernelGGL(relative_rotation_kernel, dim3(ceil_div((long long)dirs * batch, 256)), dim3(256), 0, st, rot, vi, vj,
                     rel, batch, views, dirs);
  return check_launch("relative_rotation");
}

int mvg_rotcat_fwd(const float *img_feat, const float *feat, const float *rel, const int32_t *view_of,
                   const int32_t *src_of, float *x, int batch, int dirs, int cf, int nvec, void *stream) {
  MVG_REQUIRE(cf % 4 == 0, "rotcat: cf %% 4 != 0");
  MVG_REQUIRE(nvec > 0 && nvec % 4 == 0, "rotcat: nvec %% 4 != 0 (nvec=%d: rows of cf + 3 nvec floats move as 16-byte vectors)", nvec);
  MVG_REQUIRE(batch > 0 && dirs > 0, "rotcat: batch and dirs must be positive");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_ROTCAT, st, 18.0 * dirs * batch * nvec, 8.0 * dirs * (double)batch * (cf + 3 * nvec));
  hipLaunchKernelGGL(rotcat_fwd_kernel, dim3(dirs * batch), dim3(256), 0, st, img_feat, feat, rel, view_of, src_of, x,
                     batch, cf, nvec);
  return check_launch("rotcat_fwd");
}

int mvg_rotcat_bwd(const float *dx, const float *rel, const int32_t *src_of, float *dfeat, int batch, int dirs, int cf,
                   int nvec, void *stream) {
  MVG_REQUIRE(cf % 4 == 0, "rotcat_bwd: cf %% 4 != 0");
  MVG_REQUIRE(nvec > 0 && nvec % 4 == 0, "rotcat_bwd: nvec %% 4 != 0 (nvec=%d)", nvec);
  MVG_REQUIRE(batch > 0 && dirs > 0, "rotcat_bwd: batch and dirs must be positive");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_ROTCAT, st, 18.0 * dirs * batch * nvec, 24.0 * dirs * (double)batch * nvec);
  hipLaunchKernelGGL(rotcat_bwd_feat_kernel, dim3(dirs * batch), dim3(256), 0, st, dx, rel, src_of, dfeat, batch, cf, nvec);
  return check_launch("rotcat_bwd");
}

int mvg_rotcat_ext_fwd(const float *img_feat, const float *feat, const float *rel_apply, const float *rel_append,
                       const int32_t *view_of, const int32_t *src_of, float *x, int ld, int batch, int dirs, int cf, int nvec,
                       void *stream) {
  MVG_REQUIRE(cf % 4 == 0 && ld % 4 == 0, "rotcat_ext: cf / ld %% 4 != 0");
  MVG_REQUIRE(nvec > 0 && nvec % 4 == 0, "rotcat_ext: nvec %% 4 != 0 (nvec=%d)", nvec);
  MVG_REQUIRE(ld >= cf + 3 * nvec + (rel_append ? 9 : 0), "rotcat_ext: ld too small");
  MVG_REQUIRE(batch > 0 && dirs > 0, "rotcat_ext: batch and dirs must be positive");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_ROTCAT, st, 18.0 * dirs * batch * nvec, 8.0 * dirs * (double)batch * ld);
  hipLaunchKernelGGL(rotcat_ext_fwd_kernel, dim3(dirs * batch), dim3(256), 0, st, img_feat, feat, rel_apply, rel_append, view_of,
                     src_of, x, ld, batch, cf, nvec);
  return check_launch("rotcat_ext_fwd");
}

int mvg_rotcat_ext_bwd(const float *dx, int ld, const float *rel, const int32_t *src_of, float *dfeat, int batch, int dirs,
                       int cf, int nvec, void *stream) {
  MVG_REQUIRE(cf % 4 == 0 && ld % 4 == 0, "rotcat_ext_bwd: cf / ld %% 4 != 0");
  MVG_REQUIRE(nvec > 0 && nvec % 4 == 0, "rotcat_ext_bwd: nvec %% 4 != 0 (nvec=%d)", nvec);
  MVG_REQUIRE(ld >= cf + 3 * nvec, "rotcat_ext_bwd: ld too small");
  MVG_REQUIRE(batch > 0 && dirs > 0, "rotcat_ext_bwd: batch and dirs must be positive");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_ROTCAT, st, 18.0 * dirs * batch * nvec, 24.0 * dirs * (double)batch * nvec);
  hipLaunchKernelGGL(rotcat_ext_bwd_kernel, dim3(dirs * batch), dim3(256), 0, st, dx, ld, rel, src_of, dfeat, batch, cf, nvec);
  return check_launch("rotcat_ext_bwd");
}

int mvg_ibn_scales(const float *a, const float *feat, const int32_t *view_of, const int32_t *src_of, float *running_mean,
                   int training, float momentum, float eps, float *scales, int batch, int dirs, int nvec, void *stream) {
  MVG_REQUIRE(batch > 0 && dirs > 0 && nvec > 0, "ibn_scales: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_ELEMENTWISE, st, 0.0, 24.0 * dirs * (double)batch * nvec * 2);
  hipLaunchKernelGGL(ibn_scales_kernel, dim3(ceil_div(nvec, 256)), dim3(256), 0, st, a, feat, view_of, src_of, running_mean,
                     training, momentum, eps, scales, batch, dirs, nvec);
  return check_launch("ibn_scales");
}

int mvg_paircat_fwd(const float *a, const float *feat, const float *rel, const float *scales, const int32_t *view_of,
                    const int32_t *src_of, float *x, int batch, int dirs, int nvec, void *stream) {
  MVG_REQUIRE(nvec > 0 && nvec % 4 == 0, "paircat: nvec %% 4 != 0 (nvec=%d)", nvec);
  MVG_REQUIRE(batch > 0 && dirs > 0, "paircat: batch and dirs must be positive");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_ROTCAT, st, 18.0 * dirs * batch * nvec, 48.0 * dirs * (double)batch * nvec);
  hipLaunchKernelGGL(paircat_fwd_kernel, dim3(dirs * batch), dim3(256), 0, st, a, feat, rel, scales, view_of, src_of, x, batch,
                     nvec);
  return check_launch("paircat_fwd");
}

int mvg_paircat_bwd(const float *dx, const float *rel, const float *scales, const int32_t *src_of, float *da_dir, float *dfeat,
                    int batch, int dirs, int nvec, void *stream) {
  MVG_REQUIRE(nvec > 0 && nvec % 4 == 0, "paircat_bwd: nvec %% 4 != 0 (nvec=%d)", nvec);
  MVG_REQUIRE(batch > 0 && dirs > 0, "paircat_bwd: batch and dirs must be positive");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_ROTCAT, st, 18.0 * dirs * batch * nvec, 48.0 * dirs * (double)batch * nvec);
  hipLaunchKernelGGL(paircat_bwd_kernel, dim3(dirs * batch), dim3(256), 0, st, dx, rel, scales, src_of, da_dir, dfeat, batch,
                     nvec);
  return check_launch("paircat_bwd");
}

int mvg_segment_sum(const float *x, int64_t row_stride, int width, const int32_t *seg_of, float *out, int batch, int dirs,
                    int segments, int accumulate, void *stream) {
  MVG_REQUIRE(width % 4 == 0 && row_stride % 4 == 0, "segment_sum: width/row_stride %% 4 != 0");
  MVG_REQUIRE(batch > 0 && dirs > 0 && segments > 0 && width > 0, "segment_sum: batch, dirs, segments and width must be positive");
  hipStream_t st = (hipStream_t)stream;
  const long long total = (long long)segments * batch * (width / 4);
  ProfScope ps(MVG_K_ELEMENTWISE, st, 0.0, 4.0 * (double)batch * width * (dirs + segments));
  hipLaunchKernelGGL(segment_sum_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, st, x, (long long)row_stride, width / 4,
                     seg_of, out, batch, dirs, segments, accumulate);
  return check_launch("segment_sum");
}

int mvg_scale_by(const float *x, const float *scale, float *out, int64_t n, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_ELEMENTWISE, st, 0.0, 8.0 * (double)n);
  long long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(scale_by_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, scale, out, (long long)n);
  return check_launch("scale_by");
}

int mvg_axpby(const float *x, float *y, float a, float b, int64_t n, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_ELEMENTWISE, st, 0.0, 12.0 * (double)n);
  long long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(axpby_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, y, a, b, (long long)n);
  return check_launch("axpby");
}

int mvg_absmax_multi(const float *const *host_ptrs, const int64_t *host_counts, float *const *host_out_slots, int n, void *stream) {
  MVG_REQUIRE(host_ptrs && host_counts && host_out_slots && n >= 1 && n <= 8, "absmax_multi: 1..8 tensors");
  AbsMaxItems it;
  memset(&it, 0, sizeof(it));
  long long most = 0;
  for (int i = 0; i < n; ++i) {
    MVG_REQUIRE(host_ptrs[i] && host_out_slots[i] && host_counts[i] >= 0, "absmax_multi: null tensor / slot");
    it.p[i] = host_ptrs[i];
    it.n[i] = host_counts[i];
    it.out[i] = (unsigned *)host_out_slots[i];
    if (host_counts[i] > most) most = host_counts[i];
  }
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_ELEMENTWISE, st, 0.0, 0.0);
  long long blocks = (most + 256 * 8 - 1) / (256 * 8);
  if (blocks < 1) blocks = 1;
  if (blocks > 512) blocks = 512;
  hipLaunchKernelGGL(absmax_multi_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, st, it);
  return check_launch("absmax_multi");
}

int mvg_fuse_build_split(const float *img_feat, const float *feat, const float *rel, const int32_t *row_img, const int32_t *row_src_f,
                         const int32_t *row_src_h, void *xf_sp, void *xh_sp, const float *am_img, const float *am_feat,
                         float *xf_sinv, float *xh_sinv, int rows, int cf, int nvec, void *stream) {
  MVG_REQUIRE(img_feat && feat && row_img && am_img && am_feat && rows > 0, "fuse_build_split: null argument");
  MVG_REQUIRE(cf % 8 == 0 && nvec % 8 == 0, "fuse_build_split: cf and nvec must be multiples of 8");
  MVG_REQUIRE((!xf_sp || (row_src_f && xf_sinv)) && (!xh_sp || (row_src_h && xh_sinv)) && (xf_sp || xh_sp),
              "fuse_build_split: each operand needs its row table and its sinv slot");
  hipStream_t st = (hipStream_t)stream;
  const int nout = (xf_sp ? 1 : 0) + (xh_sp ? 1 : 0);
  ProfScope ps(MVG_K_ROTCAT, st, 18.0 * rows * nvec, (4.0 + 4.0 * nout) * (double)rows * (cf + 3 * nvec));
  hipLaunchKernelGGL(fuse_build_split_kernel, dim3(rows), dim3(256), 0, st, img_feat, feat, rel, row_img, row_src_f, row_src_h, (uint4 *)xf_sp,
                     (uint4 *)xh_sp, (const unsigned *)am_img, (const unsigned *)am_feat, xf_sinv, xh_sinv, cf, nvec);
  return check_launch("fuse_build_split");
}

int mvg_fuse_unbuild(const float *dxh, const float *dxn, const float *rel, const int32_t *seg, const int32_t *vi, float *dfeat, float *da,
                     int da_accumulate, int segments, int views, int dirs, int batch, int cf, int nvec, float *absmax, void *stream) {
  MVG_REQUIRE((dxh || dxn) && seg && vi && dfeat && da, "fuse_unbuild: null argument");
  MVG_REQUIRE(cf % 4 == 0 && segments > 0 && views > 0 && dirs > 0 && batch > 0, "fuse_unbuild: bad sizes");
  MVG_REQUIRE(nvec > 0 && nvec % 4 == 0, "fuse_unbuild: nvec %% 4 != 0 (nvec=%d: rows of cf + 3 nvec floats move as 16-byte vectors)", nvec);
  MVG_REQUIRE(!dxh || segments == dirs, "fuse_unbuild: the head-input gradient has one row per direction (segments == dirs)");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_ROTCAT, st, 18.0 * dirs * batch * nvec, 4.0 * (double)batch * ((dxh ? 1 : 0) + (dxn ? 1 : 0)) * dirs * (cf + 3 * nvec));
  const int rpb = 4;                      // feature rows per workgroup: a quarter of the atomics, still >= 1 workgroup per CU at C3
  hipLaunchKernelGGL(fuse_unbuild_kernel, dim3(ceil_div(segments * batch, rpb) + views * batch), dim3(256), 0, st, dxh, dxn, rel, seg, vi, dfeat,
                     da, da_accumulate, segments, views, dirs, batch, cf, nvec, (unsigned *)absmax, rpb);
  return check_launch("fuse_unbuild");
}

int mvg_gaze_angular_loss_multi(const float *pred, const float *gt, int iters, int dirs, int batch, const float *host_weights, float *loss,
                                float *dpred, void *stream) {
  MVG_REQUIRE(pred && gt && host_weights && loss && iters > 0 && dirs > 0 && batch > 0 && iters * dirs <= 512,
              "gaze_angular_loss_multi: bad arguments (iters * dirs <= 512)");
  LossWeights lw;
  memset(&lw, 0, sizeof(lw));
  for (int i = 0; i < iters * dirs; ++i) lw.w[i] = host_weights[i];
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_LOSS, st, 0.0, 24.0 * iters * dirs * batch);
  hipLaunchKernelGGL(gaze_loss_multi_kernel, dim3(1), dim3(256), 0, st, pred, gt, iters, dirs, batch, lw, loss, dpred);
  return check_launch("gaze_angular_loss_multi");
}

int mvg_gaze_error_update(const float *preds, const float *gt, int iters, int dirs, int batch, double *record, float *err_out,
                          int64_t capacity, void *stream) {
  // (every check comes before the first HIP call: they run on a machine without a GPU)
  MVG_REQUIRE(preds && gt && record, "gaze_error_update: null preds, gt or record");
  MVG_REQUIRE(iters >= 1 && dirs >= 1 && batch >= 1, "gaze_error_update: iters, dirs and batch must be >= 1 (got %d, %d, %d)", iters, dirs,
              batch);
  MVG_REQUIRE((int64_t)iters * dirs <= INT32_MAX, "gaze_error_update: iters * dirs = %lld cells exceed one grid",
              (long long)iters * dirs);
  MVG_REQUIRE(capacity >= 0, "gaze_error_update: capacity must be >= 0 (got %lld)", (long long)capacity);
  MVG_REQUIRE(!err_out || capacity > 0, "gaze_error_update: err_out needs capacity > 0");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_LOSS, st, 0.0, (double)iters * dirs * (batch * (err_out ? 20.0 : 16.0) + 80.0));
  hipLaunchKernelGGL(gaze_error_update_kernel, dim3((unsigned)(iters * dirs)), dim3(256), 0, st, preds, gt, dirs, batch, record, err_out,
                     (long long)capacity);
  return check_launch("gaze_error_update");
}

// (the checks the two consensus entry points share, before the first HIP call; rows of two floats move as 8-byte vectors)
static int consensus_check(const char *who, int iters, int views, int batch, const void *rows0, const void *rows1) {
  MVG_REQUIRE(views >= 2 && views <= 8, "%s: views must be 2..8 (got %d)", who, views);
  MVG_REQUIRE(iters >= 1 && batch >= 1, "%s: iters and batch must be >= 1 (got %d, %d)", who, iters, batch);
  MVG_REQUIRE((int64_t)iters * batch <= INT32_MAX, "%s: iters * batch = %lld items exceed one grid", who,
              (long long)iters * batch);
  MVG_REQUIRE(((uintptr_t)rows0 | (uintptr_t)rows1) % 8 == 0, "%s: the (pitch, yaw) buffers must be 8-byte aligned", who);
  return 0;
}

int mvg_gaze_consensus_fwd(const float *preds, const float *rot, const float *weights, int iters, int views, int batch, float *head,
                           float *views_out, float *stats, void *stream) {
  MVG_REQUIRE(preds, "gaze_consensus_fwd: null preds");
  MVG_REQUIRE(rot, "gaze_consensus_fwd: null rot");
  MVG_REQUIRE(head, "gaze_consensus_fwd: null head");
  MVG_REQUIRE(views_out, "gaze_consensus_fwd: null views_out");
  if (int e = consensus_check("gaze_consensus_fwd", iters, views, batch, preds, views_out)) return e;
  hipStream_t st = (hipStream_t)stream;
  const double items = (double)iters * batch, dirs = (double)views * (views - 1);
  ProfScope ps(MVG_K_LOSS, st, 0.0, items * (8.0 * dirs + 8.0 * views + 12.0 + (stats ? 8.0 : 0.0)) + batch * views * (36.0 + (weights ? 4.0 : 0.0)));
  hipLaunchKernelGGL(gaze_consensus_fwd_kernel, dim3((unsigned)ceil_div((int64_t)iters * batch, 256)), dim3(256), 0, st, preds, rot, weights,
                     iters, views, batch, head, views_out, stats);
  return check_launch("gaze_consensus_fwd");
}

int mvg_gaze_consensus_bwd(const float *dviews, const float *preds, const float *rot, const float *weights, int iters, int views,
                           int batch, float *dpreds, void *stream) {
  MVG_REQUIRE(dviews, "gaze_consensus_bwd: null dviews");
  MVG_REQUIRE(preds, "gaze_consensus_bwd: null preds");
  MVG_REQUIRE(rot, "gaze_consensus_bwd: null rot");
  MVG_REQUIRE(dpreds, "gaze_consensus_bwd: null dpreds");
  if (int e = consensus_check("gaze_consensus_bwd", iters, views, batch, preds, dpreds)) return e;
  MVG_REQUIRE((uintptr_t)dviews % 8 == 0, "gaze_consensus_bwd: the (pitch, yaw) buffers must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const double items = (double)iters * batch, dirs = (double)views * (views - 1);
  ProfScope ps(MVG_K_LOSS, st, 0.0, items * (16.0 * dirs + 8.0 * views) + batch * views * (36.0 + (weights ? 4.0 : 0.0)));
  hipLaunchKernelGGL(gaze_consensus_bwd_kernel, dim3((unsigned)ceil_div((int64_t)iters * batch, 256)), dim3(256), 0, st, dviews, preds, rot,
                     weights, iters, views, batch, dpreds);
  return check_launch("gaze_consensus_bwd");
}

int mvg_linear_skinny_fwd(const float *x, const float *w, const float *bias, float *y, int rows, int k, int nout,
                          void *stream) {
  MVG_REQUIRE(nout >= 1 && nout <= 4, "skinny linear: out_features must be 1..4");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_LINEAR_FPROP, st, 2.0 * rows * (double)k * nout, 4.0 * ((double)rows * k + (double)k * nout));
  hipLaunchKernelGGL(skinny_fwd_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, st, x, w, bias, y, rows, k, nout);
  return check_launch("skinny_fwd");
}

int mvg_linear_skinny_bwd(const float *dy, const float *x, const float *w, const float *mask, float *dx, float *dw,
                          float *db, int rows, int k, int nout, int accumulate, float *dx_absmax, void *stream) {
  MVG_REQUIRE(nout >= 1 && nout <= 4, "skinny linear: out_features must be 1..4");
  hipStream_t st = (hipStream_t)stream;
  if (dx) {
    ProfScope ps(MVG_K_LINEAR_DGRAD, st, 2.0 * rows * (double)k * nout, 8.0 * (double)rows * k);
    const long long total = (long long)rows * k;
    long long blocks = (total + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(skinny_bwd_dx_kernel, dim3((unsigned)blocks), dim3(256), 0, st, dy, w, mask, dx, total, k, nout, (unsigned *)dx_absmax);
    if (check_launch("skinny_bwd_dx")) return 1;
  }
  if (dw) {
    ProfScope ps(MVG_K_LINEAR_WGRAD, st, 2.0 * rows * (double)k * nout, 4.0 * (double)rows * k);
    hipLaunchKernelGGL(skinny_bwd_dw_kernel, dim3(ceil_div(k, 4)), dim3(256), 0, st, dy, x, dw, db, rows, k, nout,
                       accumulate);
    if (check_launch("skinny_bwd_dw")) return 1;
  }
  return 0;
}

int mvg_gaze_lp_loss(const float *pred, const float *label, int n, int p, float *loss, float *dpred, void *stream) {
  MVG_REQUIRE(n > 0 && (p == 1 || p == 2), "gaze_lp_loss: n > 0 and p in {1, 2}");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_LOSS, st, 0.0, 12.0 * n);
  hipLaunchKernelGGL(gaze_lp_loss_kernel, dim3(1), dim3(256), 0, st, pred, label, n, p, loss, dpred);
  return check_launch("gaze_lp_loss");
}

int mvg_gaze_angular_loss(const float *pred, const float *gt, int n, float row_weight, float *loss, int accumulate,
                          float *dpred, float *theta_out, void *stream) {
  MVG_REQUIRE(n > 0, "gaze loss: n <= 0");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_LOSS, st, 0.0, 24.0 * n);
  hipLaunchKernelGGL(gaze_loss_kernel, dim3(1), dim3(256), 0, st, pred, gt, n, row_weight, loss, accumulate, dpred,
                     theta_out);
  return check_launch("gaze_angular_loss");
}

}  // extern "C"
