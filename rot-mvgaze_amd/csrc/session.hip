// The inference session's executor: mvg_session_bind queues what depends on the weights only, mvg_session_forward walks the
// plan (session_plan.cpp) and queues one existing entry point per step - the same functions, with the same arguments, the
// Python module calls, so launch plans, stream-K decisions and ProfScope accounting are theirs.  No launch logic lives here;
// the three kernels below are table / layout plumbing of bind.  Both compute forms of the plan (fp32, bf16) run through the same
// executor: the form only decides which steps the plan holds and which weight copies bind queues.
#include "common.h"
#include "session_plan.h"

namespace mvg {

constexpr float BN_EPS = 1e-5f;                                          // nn.BatchNorm2d default (resnet.py:185)
constexpr float IMAGE_MEAN[3] = {0.485f, 0.456f, 0.406f}, IMAGE_STD[3] = {0.229f, 0.224f, 0.225f};   // main.py:38-39

// Host records travel to the device as kernel arguments (captured at launch: no asynchronous copy from host memory that
// could be read after the caller moved on, and no synchronisation).
constexpr int STAGE_WORDS = 960;
struct StageChunk {
  uint32_t n;
  uint32_t w[STAGE_WORDS];
};
__global__ void session_stage_kernel(StageChunk c, uint32_t *__restrict__ dst) {
  for (uint32_t i = threadIdx.x; i < c.n; i += blockDim.x) dst[i] = c.w[i];
}

// FusionHead._indices / _row_tables: row (d, b) of a fuser / head input takes the image feature of view vi[d] and the source
// feature row of the partner view (iteration 0), the partner direction d ^ 1, or itself.
struct PairTab {
  int32_t dirs, batch;
  int32_t vi[SESSION_MAX_VIEWS * (SESSION_MAX_VIEWS - 1)], vj[SESSION_MAX_VIEWS * (SESSION_MAX_VIEWS - 1)];
};
__global__ void session_tables_kernel(PairTab t, int32_t *__restrict__ vi, int32_t *__restrict__ vj, int32_t *__restrict__ img,
                                      int32_t *__restrict__ view, int32_t *__restrict__ partner, int32_t *__restrict__ ident) {
  const int rows = t.dirs * t.batch;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += gridDim.x * blockDim.x) {
    const int d = i / t.batch, b = i - d * t.batch;
    img[i] = t.vi[d] * t.batch + b;
    view[i] = t.vj[d] * t.batch + b;
    partner[i] = (d ^ 1) * t.batch + b;
    ident[i] = i;
    if (i < t.dirs) {
      vi[i] = t.vi[i];
      vj[i] = t.vj[i];
    }
  }
}

// The stem's [cout][7][7][3] filter with the channels zero-padded to 4 (Backbone._weight)
__global__ void session_pad_stem_kernel(const float *__restrict__ w, float *__restrict__ w4, int taps) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= taps) return;
  reinterpret_cast<float4 *>(w4)[i] = make_float4(w[3 * i], w[3 * i + 1], w[3 * i + 2], 0.f);
}

struct BnEvalRecord {          // mvg_bn_eval_affine_batch's record
  const float *gamma, *beta, *rm, *rv;
  float *scale, *shift;
  int32_t c, pad;
};
struct WPrepRecord {           // mvg_weights_prep_batch's record
  const float *w;
  void *wk, *wt;
  int32_t cout, rs, cin, cin_pad;
  float *stat;
};
static_assert(sizeof(BnEvalRecord) == 56 && sizeof(WPrepRecord) == 48, "record sizes are part of the entry points' contract");

static int stage(const void *host, size_t bytes, void *dst, hipStream_t st) {
  const uint32_t *src = (const uint32_t *)host;
  size_t words = (bytes + 3) / 4, done = 0;
  while (done < words) {
    StageChunk c;
    c.n = (uint32_t)(words - done < (size_t)STAGE_WORDS ? words - done : (size_t)STAGE_WORDS);
    memcpy(c.w, src + done, (size_t)c.n * 4);
    hipLaunchKernelGGL(session_stage_kernel, dim3(1), dim3(256), 0, st, c, (uint32_t *)dst + done);
    if (check_launch("session_bind: staging a table")) return 1;
    done += c.n;
  }
  return 0;
}

static char *buf_ptr(const mvg_session *s, int buf, int64_t off = 0) { return s->workspace + s->plan.bufs[buf].off + off; }

struct FwdArgs {
  const void *const *views;
  const float *rot;
  float *img_feat, *lifted, *feats, *preds;
};

static void *resolve(const mvg_session *s, const FwdArgs &a, const SRef &r) {
  switch (r.space) {
    case SR_BUF: return buf_ptr(s, r.idx, r.off);
    case SR_TENSOR: return const_cast<void *>(s->tensor_ptrs[r.idx]);
    case SR_IMG_FEAT: return (char *)a.img_feat + r.off;
    case SR_LIFTED: return (char *)a.lifted + r.off;
    case SR_FEATS: return (char *)a.feats + r.off;
    case SR_PREDS: return (char *)a.preds + r.off;
    case SR_VIEW: return const_cast<void *>(a.views[r.idx]);
    case SR_ROT: return const_cast<float *>(a.rot);
    default: return nullptr;
  }
}

static int run_step(const mvg_session *s, const FwdArgs &a, const SStep &t, void *stream) {
  void *p[16];
  for (int k = 0; k < 16; ++k) p[k] = resolve(s, a, t.r[k]);
  auto F = [&](int k) { return (float *)p[k]; };
  const int32_t *i = t.i;
  switch (t.op) {
    case SOP_NCHW_TO_NHWC4: return mvg_nchw_to_nhwc4(F(0), F(1), i[0], i[1], i[2], i[3], stream);
    case SOP_PREPROCESS_U8:
      return mvg_preprocess_u8hwc_resize((const uint8_t *)p[0], F(1), i[0], i[1], i[2], i[3], i[4], IMAGE_MEAN[0], IMAGE_MEAN[1],
                                         IMAGE_MEAN[2], IMAGE_STD[0], IMAGE_STD[1], IMAGE_STD[2], i[5], stream);
    case SOP_CONV_AFFINE: return mvg_conv_fprop_affine(&t.d, F(0), F(1), F(2), F(3), F(4), F(5), i[0], stream);
    case SOP_CONV_SPLIT_AFFINE:
      if (s->range_record && t.range >= 0)
        return mvg_conv_fprop_split_affine_ranged(&t.d, p[0], nullptr, p[1], F(2), p[3], i[0], F(4), F(5), p[6], i[1], i[2],
                                                  s->range_record + t.range, stream);
      return mvg_conv_fprop_split_affine(&t.d, p[0], nullptr, p[1], F(2), p[3], i[0], F(4), F(5), p[6], i[1], i[2], stream);
    case SOP_MAXPOOL: return mvg_maxpool3x3s2_fwd(F(0), F(1), (uint8_t *)p[2], i[0], i[1], i[2], i[3], i[4], i[5], stream);
    case SOP_SPLIT_F32:
      if (s->range_record && t.range >= 0) return mvg_split_f32_ranged(F(0), p[1], t.n, 1.0f, s->range_record + t.range, stream);
      return mvg_split_f32(F(0), p[1], t.n, 1.0f, stream);
    case SOP_AVGPOOL: return mvg_avgpool_fwd(F(0), F(1), i[0], i[1], i[2], stream);
    case SOP_AVGPOOL_SPLIT: return mvg_avgpool_fwd_split_scaled(p[0], nullptr, F(1), i[0], i[1], i[2], stream);
    case SOP_LINEAR: return mvg_linear_fprop(F(0), F(1), F(2), i[0], F(3), i[1], i[2], i[3], F(4), (size_t)t.n, stream);
    case SOP_FUSER:
      return mvg_fuser_fprop(F(0), F(1), F(2), (const int32_t *)p[3], (const int32_t *)p[4], F(5), F(6), i[0], F(7), i[1], i[2], 512,
                             i[3], i[4], i[5], F(8), (size_t)t.n, stream);
    case SOP_SKINNY: return mvg_linear_skinny_fwd(F(0), F(1), F(2), F(3), i[0], i[1], i[2], stream);
    case SOP_RELROT: return mvg_relative_rotation(F(0), (const int32_t *)p[1], (const int32_t *)p[2], F(3), i[0], i[1], i[2], stream);
    case SOP_CLEAR:
      if (hipMemsetAsync(p[0], 0, (size_t)t.n, (hipStream_t)stream) != hipSuccess) {
        (void)hipGetLastError();
        set_error("session_forward: clearing the slot arena failed");
        return 1;
      }
      return 0;
    case SOP_ABSMAX: {
      const float *ptrs[8];
      float *slots[8];
      for (int k = 0; k < i[0]; ++k) {
        ptrs[k] = F(k);
        slots[k] = F(8 + k);
      }
      return mvg_absmax_multi(ptrs, t.cnt, slots, i[0], stream);
    }
    case SOP_FUSE_BUILD:
      return mvg_fuse_build_split(F(0), F(1), F(2), (const int32_t *)p[3], (const int32_t *)p[4], (const int32_t *)p[5], p[6], p[7], F(8),
                                  F(9), F(10), F(11), i[0], i[1], 512, stream);
    case SOP_LINEAR_SPLIT:
      return mvg_linear_fprop_split(i[0], i[1], i[2], p[0], F(1), p[2], F(3), F(4), i[3], p[5], i[4], F(6), F(7), F(8), stream);
    // ---- the bf16 form
    case SOP_NCHW_TO_NHWC8_BF16: return mvg_nchw_to_nhwc8_bf16(F(0), (uint16_t *)p[1], i[0], i[1], i[2], i[3], stream);
    case SOP_PREPROCESS_U8_BF16:
      return mvg_preprocess_u8hwc_resize_bf16((const uint8_t *)p[0], (uint16_t *)p[1], i[0], i[1], i[2], i[3], i[4], IMAGE_MEAN[0],
                                              IMAGE_MEAN[1], IMAGE_MEAN[2], IMAGE_STD[0], IMAGE_STD[1], IMAGE_STD[2], i[5], stream);
    case SOP_CONV_BF16: return mvg_conv_fprop_bf16(&t.d, p[0], p[1], p[2], nullptr, 0, nullptr, stream);
    case SOP_BN_RELU_MAXPOOL_BF16:
      return mvg_bn_relu_maxpool_fwd_bf16((const uint16_t *)p[0], F(1), F(2), (uint16_t *)p[3], (uint8_t *)p[4], i[0], i[1], i[2], i[3],
                                          i[4], (int)t.cnt[0], (int)t.cnt[1], stream);
    case SOP_CONV_BF16_AFFINE: return mvg_conv_fprop_bf16_affine(&t.d, p[0], p[1], p[2], F(3), F(4), p[5], i[0], stream);
    case SOP_AVGPOOL_BF16: return mvg_avgpool_fwd_bf16((const uint16_t *)p[0], F(1), i[0], i[1], i[2], stream);
    case SOP_LINEAR_MIXED: return mvg_linear_fprop_mixed(F(0), p[1], F(2), i[0], F(3), i[1], i[2], i[3], stream);
    case SOP_ROTCAT:
      return mvg_rotcat_fwd(F(0), F(1), F(2), (const int32_t *)p[3], (const int32_t *)p[4], F(5), i[0], i[1], i[2], i[3], stream);
  }
  set_error("session_forward: unknown step %d", t.op);
  return 2;
}

}  // namespace mvg

using namespace mvg;

extern "C" {

int mvg_session_bind(mvg_session *s, const void *const *host_tensor_ptrs, void *workspace, size_t bytes, void *stream) {
  MVG_REQUIRE(s && host_tensor_ptrs && workspace, "session_bind: null argument");
  const SessionPlan &pl = s->plan;
  MVG_REQUIRE(bytes >= (size_t)pl.workspace_bytes, "session_bind: the workspace holds %zu bytes, the plan needs %lld", bytes,
              (long long)pl.workspace_bytes);
  MVG_REQUIRE(((uintptr_t)workspace & 255) == 0, "session_bind: the workspace must be 256-byte aligned");
  MVG_REQUIRE(mvg_scratch_bytes() <= SESSION_SCRATCH_BYTES, "session_bind: this device wants %zu bytes of scratch, the plan holds %zu",
              mvg_scratch_bytes(), SESSION_SCRATCH_BYTES);
  const int nt = (int)pl.tensors.size();
  for (int k = 0; k < nt; ++k)
    MVG_REQUIRE(host_tensor_ptrs[k] != nullptr && ((uintptr_t)host_tensor_ptrs[k] & 15) == 0,
                "session_bind: tensor %d (%s) is null or not 16-byte aligned", k, pl.tensors[k].name.c_str());
  for (const SStep &t : pl.steps)
    if (t.op == SOP_LINEAR)
      MVG_REQUIRE((size_t)t.n == mvg_linear_workspace_floats(t.i[1], t.i[2], t.i[3]), "session_bind: the plan's Linear workspace size is stale");
  s->bound = false;
  s->tensor_ptrs.assign(host_tensor_ptrs, host_tensor_ptrs + nt);
  s->workspace = (char *)workspace;
  s->workspace_bytes = bytes;
  s->bound_stream = stream;
  hipStream_t st = (hipStream_t)stream;
  auto T = [&](int k) { return (const float *)s->tensor_ptrs[k]; };
  const bool bf16 = pl.compute == MVG_SESSION_BF16;

  // the record tables
  std::vector<BnEvalRecord> folds(pl.folds.size());
  for (size_t k = 0; k < folds.size(); ++k) {
    const SBnFold &f = pl.folds[k];
    float *aff = (float *)buf_ptr(s, pl.buf_affine, f.aff_off);
    float *shift = f.shift_off >= 0 ? (float *)buf_ptr(s, pl.buf_affine, f.shift_off) : aff + f.c;
    folds[k] = {T(f.gamma), T(f.gamma + 1), T(f.gamma + 2), T(f.gamma + 3), aff, shift, f.c, 0};
  }
  auto records = [&](const std::vector<SWPrep> &src) {
    std::vector<WPrepRecord> out(src.size());
    for (size_t k = 0; k < src.size(); ++k) {
      const SWPrep &w = src[k];
      // (bf16 form, mode 0: cin zero-padded to cin_pad, no statistics)
      out[k] = {T(w.tensor), buf_ptr(s, pl.buf_wk, w.wk_off), nullptr, w.cout, w.rs, w.cin, w.cin_pad ? w.cin_pad : w.cin,
                bf16 ? nullptr : (float *)buf_ptr(s, pl.buf_wstat, 8LL * w.stat)};
    }
    return out;
  };
  const std::vector<WPrepRecord> wb = records(pl.wprep_backbone), wh = records(pl.wprep_head);
  if (stage(folds.data(), folds.size() * sizeof(BnEvalRecord), buf_ptr(s, pl.buf_tables, pl.tab_folds), st)) return 1;
  if (!wb.empty() && stage(wb.data(), wb.size() * sizeof(WPrepRecord), buf_ptr(s, pl.buf_tables, pl.tab_wprep_backbone), st)) return 1;
  if (!wh.empty() && stage(wh.data(), wh.size() * sizeof(WPrepRecord), buf_ptr(s, pl.buf_tables, pl.tab_wprep_head), st)) return 1;

  // pair / row tables (heads.directed_pairs)
  PairTab pt;
  memset(&pt, 0, sizeof(pt));
  pt.dirs = pl.dirs;
  pt.batch = s->cfg.batch;
  int d = 0;
  for (int a = 0; a < s->cfg.views; ++a)
    for (int b = a + 1; b < s->cfg.views; ++b) {
      pt.vi[d] = a; pt.vj[d] = b; ++d;
      pt.vi[d] = b; pt.vj[d] = a; ++d;
    }
  {
    auto R = [&](int64_t off) { return (int32_t *)buf_ptr(s, pl.buf_rows, off); };
    int blocks = ceil_div(pl.head_rows, 256);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(session_tables_kernel, dim3((unsigned)blocks), dim3(256), 0, st, pt, R(pl.rows_vi), R(pl.rows_vj), R(pl.rows_img),
                       R(pl.rows_view), R(pl.rows_partner), R(pl.rows_ident));
    if (check_launch("session_bind: row tables")) return 1;
  }
  if (bf16) {
    // mvg_rotcat_fwd's per-direction source tables (FusionHead._indices: partner = d ^ 1, ident = d); then the bf16 weight
    // copies as Backbone._prepare_weights / FusionHead._prepare_weights (Family.BF16) make them (mode 0; KRSC only:
    // weights_prep_batch_kernel skips a null transposed pointer in both of its mode-0 branches)
    int32_t partner[SESSION_MAX_VIEWS * (SESSION_MAX_VIEWS - 1)], ident[SESSION_MAX_VIEWS * (SESSION_MAX_VIEWS - 1)];
    for (int k = 0; k < pl.dirs; ++k) {
      partner[k] = k ^ 1;
      ident[k] = k;
    }
    if (stage(partner, (size_t)pl.dirs * 4, buf_ptr(s, pl.buf_dirs, pl.dirs_partner), st)) return 1;
    if (stage(ident, (size_t)pl.dirs * 4, buf_ptr(s, pl.buf_dirs, pl.dirs_ident), st)) return 1;
    if (int e = mvg_weights_prep_batch(buf_ptr(s, pl.buf_tables, pl.tab_wprep_backbone), (int)wb.size(), 0, 0, stream)) return e;
    if (int e = mvg_weights_prep_batch(buf_ptr(s, pl.buf_tables, pl.tab_wprep_head), (int)wh.size(), 0, 256, stream)) return e;
  }
  // the stem's filter, 3 -> 4 channels
  if (!bf16) {
    const int taps = pl.stem_cout * 49;
    hipLaunchKernelGGL(session_pad_stem_kernel, dim3((unsigned)ceil_div(taps, 256)), dim3(256), 0, st, T(pl.stem_weight),
                       (float *)buf_ptr(s, pl.buf_w4), taps);
    if (check_launch("session_bind: stem filter")) return 1;
  }
  // sp weight copies: the max |w| slots are atomicMax targets and start at zero
  if (!bf16 && (!wb.empty() || !wh.empty())) {
    if (hipMemsetAsync(buf_ptr(s, pl.buf_wstat), 0, (size_t)pl.bufs[pl.buf_wstat].bytes, st) != hipSuccess) {
      (void)hipGetLastError();
      set_error("session_bind: clearing the weight statistics failed");
      return 1;
    }
    if (!wb.empty())
      if (int e = mvg_weights_prep_batch(buf_ptr(s, pl.buf_tables, pl.tab_wprep_backbone), (int)wb.size(), 1, 0, stream)) return e;
    if (!wh.empty())
      if (int e = mvg_weights_prep_batch(buf_ptr(s, pl.buf_tables, pl.tab_wprep_head), (int)wh.size(), 1, 256, stream)) return e;
  }
  // every BatchNorm's (scale, shift) from its running statistics
  if (int e = mvg_bn_eval_affine_batch(buf_ptr(s, pl.buf_tables, pl.tab_folds), (int)folds.size(), pl.max_c, BN_EPS, stream)) return e;
  s->bound = true;
  return 0;
}

int mvg_session_forward(mvg_session *s, const void *const *host_view_ptrs, const float *rot, float *img_feat, float *lifted, float *feats,
                        float *preds, void *stream) {
  MVG_REQUIRE(s && host_view_ptrs && rot && img_feat && lifted && feats && preds, "session_forward: null argument");
  MVG_REQUIRE(s->bound, "session_forward: mvg_session_bind has not succeeded on this session");
  for (int v = 0; v < s->cfg.views; ++v) MVG_REQUIRE(host_view_ptrs[v] != nullptr, "session_forward: view %d is null", v);
  const FwdArgs a = {host_view_ptrs, rot, img_feat, lifted, feats, preds};
  // the launches that can use scratch find the session's region (their stream-K / split forms, as under Python's registered
  // workspace), whatever mvg_set_scratch holds for this stream
  ScratchScope scope((hipStream_t)stream, (float *)buf_ptr(s, s->plan.buf_scratch), SESSION_SCRATCH_BYTES / sizeof(float));
  if (s->range_record && !s->plan.range_units.empty()) {     // the range record starts every forward at zero (atomicMax targets)
    if (hipMemsetAsync(s->range_record, 0, s->plan.range_units.size() * sizeof(uint32_t), (hipStream_t)stream) != hipSuccess) {
      (void)hipGetLastError();
      set_error("session_forward: clearing the range record failed");
      return 1;
    }
  }
  for (const SStep &t : s->plan.steps)
    if (int e = run_step(s, a, t, stream)) return e;
  if (s->cons_views)      // mvg_session_set_consensus: one gaze per sample from this forward's preds and rot (not a step of the plan)
    if (int e = mvg_gaze_consensus_fwd(preds, rot, s->cons_weights, s->cfg.num_iter, s->cfg.views, s->cfg.batch, s->cons_head, s->cons_views,
                                       s->cons_stats, stream))
      return e;
  if (s->err_record)     // mvg_session_set_error_record: the gaze error meter over this forward's preds (not a step of the plan)
    return mvg_gaze_error_update(preds, s->err_gt, s->cfg.num_iter, s->plan.dirs, s->cfg.batch, s->err_record, s->err_out, s->err_capacity,
                                 stream);
  return 0;
}

}  // extern "C"
