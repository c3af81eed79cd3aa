// The fused optimiser: Adam / AdamW over flat fp32 arenas (torch.optim.Adam / AdamW semantics, bias correction), the segmented
// and device-resident forms of the step, global-norm gradient clipping and the non-finite guard.  HBM-bound passes: three
// loads + a gradient load and three stores per 16-byte slot.  The update is stated ONCE (adam_elem, adam_slot,
// adam_update_kernel); the ten forms the entry points run are its instantiations, so the bit relations between them - a segment
// equals the plain step over its slice, a NULL record equals coef = 1, decoupled at wd = 0 equals coupled - hold by construction.
#include <math.h>

#include "common.h"

namespace mvg {

// ---- the update of one element
// Coupled (torch.optim.Adam: L2 weight decay joins the gradient), w = weight_decay.  trainer.py:54 optim.Adam(params, lr,
// weight_decay=1e-6).  Which products the compiler contracts here is what every coupled form has always computed.
//
// DECOUPLED (torch.optim.AdamW), w = f = 1 - lr * wd: the parameter is shrunk by f and the moments see the gradient alone.
// lr in f is the plain learning rate (not lr / bc1); f is formed on the device, in float, by every form - host-lr forms
// included - so all forms give the same bits for the same hyper-parameters, as they do for lr / bc1.
// Which products are fused is WRITTEN here, not left to the compiler: q - step_size * x has two products, and contracted the
// other way round (p * f fused, the step rounded on its own) the element would differ from the coupled one at wd = 0.  The fused
// multiply-adds are the ones the compiler forms in the coupled branch (m: (1 - b1) * g fused, b1 * m rounded; v: g * ((1 - b2) * g)
// fused, b2 * v rounded; p: the step fused), q = p * f is rounded on its own, f is one fused multiply-add: with wd = 0, f = 1, q = p
// and the element is the coupled one in every bit - and every form runs these operations whatever kernel they are inlined into.
__device__ __forceinline__ float adamw_factor(float lr, float wd) { return __fmaf_rn(-lr, wd, 1.f); }
template <bool kDecoupled>
__device__ __forceinline__ void adam_elem(float &p, float g, float &m, float &v, float b1, float b2, float eps, float w,
                                          float step_size, float bc2_sqrt) {
  if constexpr (kDecoupled) {
    const float q = p * w;
    m = __fmaf_rn(1.f - b1, g, b1 * m);
    v = __fmaf_rn(g, (1.f - b2) * g, b2 * v);
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = __fmaf_rn(-step_size, m / denom, q);
  } else {
    const float gr = g + w * p;
    m = b1 * m + (1.f - b1) * gr;
    v = b2 * v + (1.f - b2) * gr * gr;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = p - step_size * (m / denom);
  }
}

// The gradient times the clipping coefficient, as it is loaded.  The product is rounded to fp32 on its own - never contracted
// into the coupled wd * p fma - so a clipped step equals, bit for bit, the unclipped one on a gradient torch scaled in fp32.
__device__ __forceinline__ float clip_mul(float g, float coef) {
#pragma clang fp contract(off)
  return __fmul_rn(g, coef);
}

// ---- ... and of the four elements of one 16-byte slot: three loads + a gradient load, three stores.  lr / bc1 and f are formed
// here, in float, for every form: the same bits for the same hyper-parameters wherever they come from.
struct AdamHyper {
  float b1, b2, eps, wd, lr, bc1, bc2_sqrt;
};
template <bool kDecoupled, bool kClip>
__device__ __forceinline__ void adam_slot(float4 *__restrict__ p, const float4 *__restrict__ g, float4 *__restrict__ m,
                                          float4 *__restrict__ v, long long i, float coef, const AdamHyper &h) {
  const float step_size = h.lr / h.bc1, w = kDecoupled ? adamw_factor(h.lr, h.wd) : h.wd;
  float4 pp = p[i], gg = g[i], mm = m[i], vv = v[i];
  if constexpr (kClip) gg = make_float4(clip_mul(gg.x, coef), clip_mul(gg.y, coef), clip_mul(gg.z, coef), clip_mul(gg.w, coef));
  adam_elem<kDecoupled>(pp.x, gg.x, mm.x, vv.x, h.b1, h.b2, h.eps, w, step_size, h.bc2_sqrt);
  adam_elem<kDecoupled>(pp.y, gg.y, mm.y, vv.y, h.b1, h.b2, h.eps, w, step_size, h.bc2_sqrt);
  adam_elem<kDecoupled>(pp.z, gg.z, mm.z, vv.z, h.b1, h.b2, h.eps, w, step_size, h.bc2_sqrt);
  adam_elem<kDecoupled>(pp.w, gg.w, mm.w, vv.w, h.b1, h.b2, h.eps, w, step_size, h.bc2_sqrt);
  p[i] = pp;
  m[i] = mm;
  v[i] = vv;
}

// ---- SEGMENTS of the arenas (parameter groups, parameters without a gradient): up to MVG_ADAM_MAX_SEGMENTS element ranges
// travel BY VALUE in the kernel arguments - no device table, nothing a later step could overwrite under a launch still in
// flight.  The grid-stride index runs over the segments laid end to end (16-byte slots): a lane finds its segment by counting
// the prefix ends at or below its index and adds that segment's offset to reach the arena slot.  Nothing outside the segments
// is read or written.  Shared by the segmented update sources and grad_sumsq_segments_kernel.
struct SegmentMap {
  long long end4[MVG_ADAM_MAX_SEGMENTS];      // prefix ends in the concatenated index space; unused entries = the total
  long long shift4[MVG_ADAM_MAX_SEGMENTS];    // arena slot = concatenated index + shift4[segment]
  __device__ __forceinline__ long long total() const { return end4[MVG_ADAM_MAX_SEGMENTS - 1]; }
  __device__ __forceinline__ int find(long long i) const {
    int k = 0;
#pragma unroll
    for (int j = 0; j < MVG_ADAM_MAX_SEGMENTS - 1; ++j) k += i >= end4[j];
    return k;
  }
  __device__ __forceinline__ long long slot(long long i, int k) const { return i + shift4[k]; }
};

// ---- where a form's hyper-parameters come from: total(), find(i), slot(i, k), hyper(k), decoupled(k).
// The whole arena, host scalars.
struct AdamFlat {
  long long n4;
  float lr, b1, b2, eps, wd, bc1, bc2_sqrt;
  __device__ __forceinline__ long long total() const { return n4; }
  __device__ __forceinline__ int find(long long) const { return 0; }
  __device__ __forceinline__ long long slot(long long i, int) const { return i; }
  __device__ __forceinline__ AdamHyper hyper(int) const { return {b1, b2, eps, wd, lr, bc1, bc2_sqrt}; }
  __device__ __forceinline__ bool decoupled(int) const { return false; }
};
// The whole arena with its step counter and learning rate on the DEVICE (a captured step replays with nothing from the host):
// lr from lr_dev[0], the corrections from state = {step, bias correction 1, sqrt(bias correction 2)}, which adam_tick_kernel
// advances in front of the update.
struct AdamFlatDev {
  long long n4;
  const float *lr_dev, *state;
  float b1, b2, eps, wd;
  __device__ __forceinline__ long long total() const { return n4; }
  __device__ __forceinline__ int find(long long) const { return 0; }
  __device__ __forceinline__ long long slot(long long i, int) const { return i; }
  __device__ __forceinline__ AdamHyper hyper(int) const { return {b1, b2, eps, wd, lr_dev[0], state[1], state[2]}; }
  __device__ __forceinline__ bool decoupled(int) const { return false; }
};
// Segments, each with its own hyper-parameters and bias corrections from the host, and a MODE, by value like wd: mode[k]
// != 0 runs the decoupled element on segment k where the kernel asks per segment (a segment is a run of whole 16-byte slots, so
// a wave changes mode at a segment's border only).
struct AdamSegments : SegmentMap {
  float lr[MVG_ADAM_MAX_SEGMENTS], bc1[MVG_ADAM_MAX_SEGMENTS], b1[MVG_ADAM_MAX_SEGMENTS], b2[MVG_ADAM_MAX_SEGMENTS],
      eps[MVG_ADAM_MAX_SEGMENTS], wd[MVG_ADAM_MAX_SEGMENTS], bc2_sqrt[MVG_ADAM_MAX_SEGMENTS];
  int mode[MVG_ADAM_MAX_SEGMENTS];
  __device__ __forceinline__ AdamHyper hyper(int k) const { return {b1[k], b2[k], eps[k], wd[k], lr[k], bc1[k], bc2_sqrt[k]}; }
  __device__ __forceinline__ bool decoupled(int k) const { return mode[k] != 0; }
};
// Segments with their learning rates and step counters on the DEVICE (a captured fine-tuning step): a segment's learning rate
// is lr_dev[lr_index] (one float per parameter group, written by the host between replays) and its bias corrections are its row
// of state = {step, 1 - beta1^step, sqrt(1 - beta2^step)}, advanced by adam_tick_segments_kernel in front of the update.
struct AdamSegmentsDev : SegmentMap {
  const float *lr_dev, *state;
  int lr_index[MVG_ADAM_MAX_SEGMENTS];        // into lr_dev
  float b1[MVG_ADAM_MAX_SEGMENTS], b2[MVG_ADAM_MAX_SEGMENTS], eps[MVG_ADAM_MAX_SEGMENTS], wd[MVG_ADAM_MAX_SEGMENTS];
  int mode[MVG_ADAM_MAX_SEGMENTS];
  __device__ __forceinline__ AdamHyper hyper(int k) const {
    return {b1[k], b2[k], eps[k], wd[k], lr_dev[lr_index[k]], state[3 * k + 1], state[3 * k + 2]};
  }
  __device__ __forceinline__ bool decoupled(int k) const { return mode[k] != 0; }
};

// ---- the update kernel: one grid-stride loop over the source's slots.
// kMode: every slot coupled, every slot decoupled, or the source's mode per segment.
// kClip: no record; clip4 = {norm, coef, skipped, skipped_total} as grad_clip_finalize_kernel left it - the gradient is
// multiplied by coef as it is loaded and the kernel returns at once when skipped is set, so a captured replay clips and skips
// with nothing from the host and the gradient arena is never rewritten; or a record that may be null - coef = 1 (g * 1 is g in
// every bit) and no guard.
enum AdamMode { ADAM_COUPLED, ADAM_DECOUPLED, ADAM_PER_SEGMENT };
enum AdamClip { ADAM_NO_CLIP, ADAM_CLIP, ADAM_CLIP_OR_NULL };
template <class Src, AdamMode kMode, AdamClip kClip>
__global__ __launch_bounds__(256) void adam_update_kernel(float4 *__restrict__ p, const float4 *__restrict__ g,
                                                          float4 *__restrict__ m, float4 *__restrict__ v,
                                                          const float *__restrict__ clip4, Src src) {
  float coef = 1.f;
  if (kClip == ADAM_CLIP || (kClip == ADAM_CLIP_OR_NULL && clip4)) {
    coef = clip4[1];
    if (clip4[2] != 0.f) return;
  }
  const long long stride = (long long)gridDim.x * 256;
  const long long total = src.total();
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int k = src.find(i);
    // (slot and hyper are read inside each branch: the form in which every single-mode kernel compiles to the code it always had)
    if (kMode == ADAM_DECOUPLED || (kMode == ADAM_PER_SEGMENT && src.decoupled(k)))
      adam_slot<true, kClip != ADAM_NO_CLIP>(p, g, m, v, src.slot(i, k), coef, src.hyper(k));
    else
      adam_slot<false, kClip != ADAM_NO_CLIP>(p, g, m, v, src.slot(i, k), coef, src.hyper(k));
  }
}

// ---- the ticks: the advance of one state row, in double, stated once
__device__ __forceinline__ void adam_tick1(float *__restrict__ state, float b1, float b2) {
  const float step = state[0] + 1.f;
  state[0] = step;
  state[1] = (float)(1.0 - pow((double)b1, (double)step));
  state[2] = (float)sqrt(1.0 - pow((double)b2, (double)step));
}
__global__ void adam_tick_kernel(float *__restrict__ state, float b1, float b2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  adam_tick1(state, b1, b2);
}
// Lane k < count advances row k with segment k's betas, every row exactly once; with a record whose skipped flag is set, none.
struct AdamTicks {
  float b1[MVG_ADAM_MAX_SEGMENTS], b2[MVG_ADAM_MAX_SEGMENTS];
  int count;
};
__global__ void adam_tick_segments_kernel(float *__restrict__ state, const float *__restrict__ clip4, AdamTicks t) {
  const int k = threadIdx.x;
  if (blockIdx.x != 0 || k >= t.count || k >= MVG_ADAM_MAX_SEGMENTS || (clip4 && clip4[2] != 0.f)) return;
  adam_tick1(state + 3 * k, t.b1[k], t.b2[k]);
}

// ---- global-norm gradient clipping and the non-finite guard of the segmented steps (optim.Adam(max_grad_norm, skip_nonfinite))
// One read of the segments' gradients leaves clip4 = {norm, coef, skipped, skipped_total} on the device.
//
// grad_sumsq_segments_kernel: sum of squares over the segments laid end to end (nothing outside a segment is read), float4
// loads, grid-stride.  Accumulated in DOUBLE: the square of a float is exact there and a finite fp32 gradient cannot overflow
// the sum (3.4e38^2 * 1e9 < 1.8e308), so the sum is non-finite exactly when an element is.  Waves first, then the four waves
// through LDS; every workgroup stores one partial - no atomics, a fixed order for a fixed grid.
__global__ __launch_bounds__(256) void grad_sumsq_segments_kernel(const float4 *__restrict__ g, SegmentMap t,
                                                                  double *__restrict__ partial) {
  __shared__ double sh[4];
  const long long stride = (long long)gridDim.x * 256;
  const long long total = t.total();
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const float4 x = g[t.slot(i, t.find(i))];
    a0 += (double)x.x * (double)x.x;
    a1 += (double)x.y * (double)x.y;
    a2 += (double)x.z * (double)x.z;
    a3 += (double)x.w * (double)x.w;
  }
  const double local = wave_sum_d((a0 + a1) + (a2 + a3));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// One workgroup merges the `count` partials of all chunk launches in a fixed order (lane l takes l, l + 256, ... in index
// order, then waves, then the four waves) and writes the record.  coef is torch.nn.utils.clip_grad_norm_'s
// min(1, max_norm / (norm + 1e-6)), formed in double; max_norm <= 0: no clipping (coef = 1), the guard only.  A non-finite
// sum with the guard on: skipped = 1 and coef = 0; with it off, the coefficient torch's formula gives (NaN for a NaN norm, 0
// for an infinite one).  skipped_total is the one field read before it is written: replays count their skips in it.
__global__ __launch_bounds__(256) void grad_clip_finalize_kernel(const double *__restrict__ partial, int count, float max_norm,
                                                                 int skip_nonfinite, float *__restrict__ clip4) {
  __shared__ double sh[4];
  double local = 0.0;
  for (int i = threadIdx.x; i < count; i += 256) local += partial[i];
  local = wave_sum_d(local);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double sum = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  const double norm = sqrt(sum);
  const bool finite = sum - sum == 0.0;                    // false for inf and NaN
  float coef = 1.f;
  if (max_norm > 0.f) {
    const double c = (double)max_norm / (norm + 1e-6);
    coef = (float)(c > 1.0 ? 1.0 : c);                     // (a NaN passes through, as torch.clamp(max=1) lets it)
  }
  const float skipped = skip_nonfinite && !finite ? 1.f : 0.f;
  clip4[0] = (float)norm;
  clip4[1] = skipped != 0.f ? 0.f : coef;
  clip4[2] = skipped;
  clip4[3] = clip4[3] + skipped;
}

// ---- host side
// One update launch over total4 slots: at most 8192 workgroups, grid-stride beyond.
template <class Src, AdamMode kMode, AdamClip kClip>
static void launch_update(hipStream_t st, float *param, const float *grad, float *exp_avg, float *exp_avg_sq, const float *clip4,
                          const Src &src, long long total4) {
  long long blocks = (total4 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL((adam_update_kernel<Src, kMode, kClip>), dim3((unsigned)blocks), dim3(256), 0, st, (float4 *)param,
                     (const float4 *)grad, (float4 *)exp_avg, (float4 *)exp_avg_sq, clip4, src);
}

// The four flat entry points.  Host form: lr and step, the corrections formed here in double.  Device form (dev): lr_dev and
// state3, which adam_tick_kernel advances in front of the update.
template <class Src>
static int launch_flat(const char *what, bool decoupled, float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                       const Src &src, hipStream_t st) {
  if (decoupled)
    launch_update<Src, ADAM_DECOUPLED, ADAM_NO_CLIP>(st, param, grad, exp_avg, exp_avg_sq, nullptr, src, src.n4);
  else
    launch_update<Src, ADAM_COUPLED, ADAM_NO_CLIP>(st, param, grad, exp_avg, exp_avg_sq, nullptr, src, src.n4);
  return check_launch(what);
}
static int launch_flat(const char *what, bool dev, bool decoupled, float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                       int64_t n, float lr, int step, const float *lr_dev, float *state3, float beta1, float beta2, float eps,
                       float weight_decay, void *stream) {
  if (dev)
    MVG_REQUIRE(param && grad && exp_avg && exp_avg_sq && lr_dev && state3 && n % 4 == 0, "%s: null argument or n %% 4 != 0", what);
  else
    MVG_REQUIRE(n % 4 == 0 && step >= 1, "%s: n %% 4 != 0 or step < 1", decoupled ? "adamw" : "adam");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_ELEMENTWISE, st, 0.0, 28.0 * (double)n);
  if (dev) {
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(64), 0, st, state3, beta1, beta2);
    if (check_launch("adam_tick")) return 1;
    return launch_flat(what, decoupled, param, grad, exp_avg, exp_avg_sq,
                       AdamFlatDev{(long long)(n / 4), lr_dev, state3, beta1, beta2, eps, weight_decay}, st);
  }
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  return launch_flat(what, decoupled, param, grad, exp_avg, exp_avg_sq,
                     AdamFlat{(long long)(n / 4), lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2)}, st);
}

// The mode rule of the _ex entry points, checked with the segment rules before the first launch.
static int check_modes(const char *what, const int32_t *host_decoupled, int n_segments) {
  MVG_REQUIRE(host_decoupled, "%s: null host_decoupled", what);
  for (int i = 0; i < n_segments; ++i)
    MVG_REQUIRE(host_decoupled[i] == 0 || host_decoupled[i] == 1, "%s: segment %d has mode %d (0: coupled, 1: decoupled)", what, i,
                (int)host_decoupled[i]);
  return 0;
}

// The segment rules of every segmented entry point, checked before its first launch: aligned to 4, inside [0, n), non-empty,
// sorted by begin, disjoint.  *active receives the elements the segments hold.
static int check_segments(const char *what, int64_t n, const int64_t *host_bounds, int n_segments, double *active) {
  *active = 0.0;
  for (int i = 0; i < n_segments; ++i) {
    const int64_t b = host_bounds[2 * i], e = host_bounds[2 * i + 1];
    MVG_REQUIRE(b % 4 == 0 && e % 4 == 0, "%s: segment %d [%lld, %lld) is not aligned to 4 elements", what, i, (long long)b, (long long)e);
    MVG_REQUIRE(b >= 0 && e <= n, "%s: segment %d [%lld, %lld) is outside the arena of %lld elements", what, i, (long long)b, (long long)e,
                (long long)n);
    MVG_REQUIRE(b < e, "%s: segment %d [%lld, %lld) is empty or reversed", what, i, (long long)b, (long long)e);
    if (i > 0) {
      MVG_REQUIRE(b >= host_bounds[2 * i - 2], "%s: segment %d begins before segment %d (unsorted)", what, i, i - 1);
      MVG_REQUIRE(b >= host_bounds[2 * i - 1], "%s: segment %d overlaps segment %d", what, i, i - 1);
    }
    *active += (double)(e - b);
  }
  return 0;
}

// The map of the `cnt` segments from s0 on (one launch's chunk); returns the slots they hold.
static long long fill_segment_map(SegmentMap &t, const int64_t *host_bounds, int s0, int cnt) {
  long long total = 0;
  for (int k = 0; k < MVG_ADAM_MAX_SEGMENTS; ++k) {
    const int i = s0 + k;
    if (k < cnt) {
      t.shift4[k] = host_bounds[2 * i] / 4 - total;
      total += (host_bounds[2 * i + 1] - host_bounds[2 * i]) / 4;
    } else {
      t.shift4[k] = t.shift4[cnt - 1];                    // (unused entries repeat the last segment: never selected)
    }
    t.end4[k] = total;
  }
  return total;
}

// One segmented update launch: the plain form, the clipped form (a record) or, with ex set, the form with a mode per segment
// and a nullable record.
template <class Src>
static void launch_segments_update(hipStream_t st, float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                                   const float *clip4, bool ex, const Src &src, long long total4) {
  if (ex)
    launch_update<Src, ADAM_PER_SEGMENT, ADAM_CLIP_OR_NULL>(st, param, grad, exp_avg, exp_avg_sq, clip4, src, total4);
  else if (clip4)
    launch_update<Src, ADAM_COUPLED, ADAM_CLIP>(st, param, grad, exp_avg, exp_avg_sq, clip4, src, total4);
  else
    launch_update<Src, ADAM_COUPLED, ADAM_NO_CLIP>(st, param, grad, exp_avg, exp_avg_sq, clip4, src, total4);
}

// The six segmented entry points.  Host form: host_hyper = {lr, beta1, beta2, eps, weight_decay} and host_steps per segment.
// Device form (dev): host_hyper = {beta1, beta2, eps, weight_decay} and host_lr_index per segment, lr_dev, and state3_dev, whose
// rows adam_tick_segments_kernel advances in front of each update.  clip4 == nullptr without ex: the launches as they always
// were; ex: a mode per segment in host_decoupled, clip4 nullable.
static int launch_segments(const char *what, bool dev, float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                           const int64_t *host_bounds, const float *host_hyper, const int32_t *host_steps,
                           const int32_t *host_lr_index, int n_segments, const float *lr_dev, int n_lr, float *state3_dev,
                           const float *clip4, bool ex, const int32_t *host_decoupled, void *stream) {
  if (dev) {
    MVG_REQUIRE(param && grad && exp_avg && exp_avg_sq && host_bounds && host_hyper && host_lr_index && lr_dev && state3_dev,
                "%s: null argument", what);
    MVG_REQUIRE(n % 4 == 0 && n_segments >= 1 && n_lr >= 1, "%s: n %% 4 != 0, no segment or no learning rate", what);
  } else {
    MVG_REQUIRE(param && grad && exp_avg && exp_avg_sq && host_bounds && host_hyper && host_steps && n % 4 == 0 && n_segments >= 1,
                "%s: null argument, n %% 4 != 0 or no segment", what);
  }
  // every segment is checked before the first launch (the tick included): a rejected call has advanced and updated nothing
  double active = 0.0;
  if (int rc = check_segments(what, n, host_bounds, n_segments, &active)) return rc;
  for (int i = 0; i < n_segments; ++i)
    if (dev)
      MVG_REQUIRE(host_lr_index[i] >= 0 && host_lr_index[i] < n_lr, "%s: segment %d has lr index %d outside [0, %d)", what, i,
                  (int)host_lr_index[i], n_lr);
    else
      MVG_REQUIRE(host_steps[i] >= 1, "%s: segment %d has step %d < 1", what, i, (int)host_steps[i]);
  if (ex)
    if (int rc = check_modes(what, host_decoupled, n_segments)) return rc;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_ELEMENTWISE, st, 0.0, 28.0 * active);
  for (int s0 = 0; s0 < n_segments; s0 += MVG_ADAM_MAX_SEGMENTS) {
    const int cnt = n_segments - s0 < MVG_ADAM_MAX_SEGMENTS ? n_segments - s0 : MVG_ADAM_MAX_SEGMENTS;
    const auto seg = [&](int k) { return s0 + (k < cnt ? k : cnt - 1); };   // (unused entries repeat the last segment: never selected)
    if (dev) {
      AdamSegmentsDev t;
      AdamTicks ticks;
      memset(&t, 0, sizeof(t));
      memset(&ticks, 0, sizeof(ticks));
      const long long total = fill_segment_map(t, host_bounds, s0, cnt);
      for (int k = 0; k < MVG_ADAM_MAX_SEGMENTS; ++k) {
        const int i = seg(k);
        const float *h = host_hyper + 4 * i;
        t.lr_index[k] = host_lr_index[i];
        ticks.b1[k] = t.b1[k] = h[0];
        ticks.b2[k] = t.b2[k] = h[1];
        t.eps[k] = h[2];
        t.wd[k] = h[3];
        if (ex) t.mode[k] = host_decoupled[i];
      }
      ticks.count = cnt;
      float *rows = state3_dev + 3 * (size_t)s0;             // this launch's rows of the table
      t.lr_dev = lr_dev;
      t.state = rows;
      hipLaunchKernelGGL(adam_tick_segments_kernel, dim3(1), dim3(64), 0, st, rows, clip4, ticks);
      if (check_launch("adam_tick_segments")) return 1;
      launch_segments_update(st, param, grad, exp_avg, exp_avg_sq, clip4, ex, t, total);
    } else {
      AdamSegments t;
      memset(&t, 0, sizeof(t));
      const long long total = fill_segment_map(t, host_bounds, s0, cnt);
      for (int k = 0; k < MVG_ADAM_MAX_SEGMENTS; ++k) {
        const int i = seg(k);
        const float *h = host_hyper + 5 * i;
        t.lr[k] = h[0];
        t.b1[k] = h[1];
        t.b2[k] = h[2];
        t.eps[k] = h[3];
        t.wd[k] = h[4];
        t.bc1[k] = (float)(1.0 - pow((double)h[1], (double)host_steps[i]));
        t.bc2_sqrt[k] = (float)sqrt(1.0 - pow((double)h[2], (double)host_steps[i]));
        if (ex) t.mode[k] = host_decoupled[i];
      }
      launch_segments_update(st, param, grad, exp_avg, exp_avg_sq, clip4, ex, t, total);
    }
    if (check_launch(what)) return 1;
  }
  return 0;
}

// The grid of one partial-sum launch over `total4` 16-byte slots: eight workgroups per CU the planners may use, at most.
static long long grad_norm_grid(long long total4, int cus) {
  const long long cap = 8LL * cus, blocks = (total4 + 255) / 256;
  return blocks < cap ? (blocks < 1 ? 1 : blocks) : cap;
}

}  // namespace mvg

using namespace mvg;

extern "C" {

int mvg_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, void *stream) {
  return launch_flat("adam_step", false, false, param, grad, exp_avg, exp_avg_sq, n, lr, step, nullptr, nullptr, beta1, beta2, eps,
                     weight_decay, stream);
}

int mvg_adamw_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step, void *stream) {
  return launch_flat("adamw_step", false, true, param, grad, exp_avg, exp_avg_sq, n, lr, step, nullptr, nullptr, beta1, beta2, eps,
                     weight_decay, stream);
}

int mvg_adam_step_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, const float *lr_dev, float *state3,
                      float beta1, float beta2, float eps, float weight_decay, void *stream) {
  return launch_flat("adam_step_dev", true, false, param, grad, exp_avg, exp_avg_sq, n, 0.f, 0, lr_dev, state3, beta1, beta2, eps,
                     weight_decay, stream);
}

int mvg_adamw_step_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, const float *lr_dev, float *state3,
                       float beta1, float beta2, float eps, float weight_decay, void *stream) {
  return launch_flat("adamw_step_dev", true, true, param, grad, exp_avg, exp_avg_sq, n, 0.f, 0, lr_dev, state3, beta1, beta2, eps,
                     weight_decay, stream);
}

int mvg_adam_step_segments(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, const int64_t *host_bounds,
                           const float *host_hyper, const int32_t *host_steps, int n_segments, void *stream) {
  return launch_segments("adam_step_segments", false, param, grad, exp_avg, exp_avg_sq, n, host_bounds, host_hyper, host_steps, nullptr,
                         n_segments, nullptr, 0, nullptr, nullptr, false, nullptr, stream);
}

int mvg_adam_step_segments_clip(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, const int64_t *host_bounds,
                                const float *host_hyper, const int32_t *host_steps, int n_segments, const float *clip4_dev, void *stream) {
  MVG_REQUIRE(clip4_dev, "adam_step_segments_clip: null clip4 record");
  return launch_segments("adam_step_segments_clip", false, param, grad, exp_avg, exp_avg_sq, n, host_bounds, host_hyper, host_steps,
                         nullptr, n_segments, nullptr, 0, nullptr, clip4_dev, false, nullptr, stream);
}

int mvg_adam_step_segments_ex(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, const int64_t *host_bounds,
                              const float *host_hyper, const int32_t *host_steps, const int32_t *host_decoupled, int n_segments,
                              const float *clip4_dev, void *stream) {
  return launch_segments("adam_step_segments_ex", false, param, grad, exp_avg, exp_avg_sq, n, host_bounds, host_hyper, host_steps, nullptr,
                         n_segments, nullptr, 0, nullptr, clip4_dev, true, host_decoupled, stream);
}

int mvg_adam_step_segments_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, const int64_t *host_bounds,
                               const float *host_hyper, const int32_t *host_lr_index, int n_segments, const float *lr_dev, int n_lr,
                               float *state3_dev, void *stream) {
  return launch_segments("adam_step_segments_dev", true, param, grad, exp_avg, exp_avg_sq, n, host_bounds, host_hyper, nullptr,
                         host_lr_index, n_segments, lr_dev, n_lr, state3_dev, nullptr, false, nullptr, stream);
}

int mvg_adam_step_segments_dev_clip(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, const int64_t *host_bounds,
                                    const float *host_hyper, const int32_t *host_lr_index, int n_segments, const float *lr_dev, int n_lr,
                                    float *state3_dev, const float *clip4_dev, void *stream) {
  MVG_REQUIRE(clip4_dev, "adam_step_segments_dev_clip: null clip4 record");
  return launch_segments("adam_step_segments_dev_clip", true, param, grad, exp_avg, exp_avg_sq, n, host_bounds, host_hyper, nullptr,
                         host_lr_index, n_segments, lr_dev, n_lr, state3_dev, clip4_dev, false, nullptr, stream);
}

int mvg_adam_step_segments_dev_ex(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, const int64_t *host_bounds,
                                  const float *host_hyper, const int32_t *host_lr_index, const int32_t *host_decoupled, int n_segments,
                                  const float *lr_dev, int n_lr, float *state3_dev, const float *clip4_dev, void *stream) {
  return launch_segments("adam_step_segments_dev_ex", true, param, grad, exp_avg, exp_avg_sq, n, host_bounds, host_hyper, nullptr,
                         host_lr_index, n_segments, lr_dev, n_lr, state3_dev, clip4_dev, true, host_decoupled, stream);
}

int64_t mvg_grad_norm_workspace_bytes(int n_segments) {
  if (n_segments < 1) {
    set_error("grad_norm_workspace_bytes: no segment");
    return -1;
  }
  int cus = mvg_device_cus();                              // (every CU: what compute_cus() can at most answer)
  if (cus <= 0) cus = 256;
  const int64_t chunks = (n_segments + MVG_ADAM_MAX_SEGMENTS - 1) / MVG_ADAM_MAX_SEGMENTS;
  return chunks * 8 * cus * (int64_t)sizeof(double);
}

int mvg_grad_norm_segments(const float *grad, int64_t n, const int64_t *host_bounds, int n_segments, float max_norm, int skip_nonfinite,
                           void *ws, int64_t ws_bytes, float *clip4_dev, void *stream) {
  MVG_REQUIRE(grad && host_bounds && ws && clip4_dev, "grad_norm_segments: null argument (grad, host_bounds, ws or clip4)");
  MVG_REQUIRE(n % 4 == 0 && n_segments >= 1, "grad_norm_segments: n %% 4 != 0 or no segment");
  MVG_REQUIRE(max_norm == max_norm, "grad_norm_segments: max_norm is NaN");
  double active = 0.0;
  if (int rc = check_segments("grad_norm_segments", n, host_bounds, n_segments, &active)) return rc;
  // the grids of all chunk launches, before the first of them: their partials lie end to end in the workspace
  const int cus = compute_cus();
  long long partials = 0;
  for (int s0 = 0; s0 < n_segments; s0 += MVG_ADAM_MAX_SEGMENTS) {
    long long total = 0;
    for (int i = s0; i < n_segments && i < s0 + MVG_ADAM_MAX_SEGMENTS; ++i) total += (host_bounds[2 * i + 1] - host_bounds[2 * i]) / 4;
    partials += grad_norm_grid(total, cus);
  }
  MVG_REQUIRE(ws_bytes >= partials * (long long)sizeof(double) && partials < (1LL << 30),
              "grad_norm_segments: workspace of %lld bytes is too small for %lld partial sums (mvg_grad_norm_workspace_bytes)",
              (long long)ws_bytes, partials);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(MVG_K_ELEMENTWISE, st, 2.0 * active, 4.0 * active);
  long long at = 0;
  for (int s0 = 0; s0 < n_segments; s0 += MVG_ADAM_MAX_SEGMENTS) {
    const int cnt = n_segments - s0 < MVG_ADAM_MAX_SEGMENTS ? n_segments - s0 : MVG_ADAM_MAX_SEGMENTS;
    SegmentMap t;
    const long long blocks = grad_norm_grid(fill_segment_map(t, host_bounds, s0, cnt), cus);
    hipLaunchKernelGGL(grad_sumsq_segments_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float4 *)grad, t, (double *)ws + at);
    if (check_launch("grad_norm_segments")) return 1;
    at += blocks;
  }
  hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(256), 0, st, (const double *)ws, (int)partials, max_norm,
                     skip_nonfinite != 0, clip4_dev);
  return check_launch("grad_clip_finalize");
}

}  // extern "C"
