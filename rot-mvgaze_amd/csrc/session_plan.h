// The inference session's plan: what session_plan.cpp (host only, no HIP) builds and session.hip executes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rotmvgaze.h"

namespace mvg {

void set_error(const char *fmt, ...);      // api.hip; a stand-alone build of the plan builder brings its own

// Where a launch argument lives.  SR_BUF: a buffer of the plan inside the caller's workspace (idx = buffer, off = bytes
// into it); SR_TENSOR: a bound model tensor (idx as mvg_session_tensor_name counts); the rest are mvg_session_forward's
// arguments (SR_VIEW: idx = the view).
enum SRefSpace { SR_NONE = 0, SR_BUF, SR_TENSOR, SR_IMG_FEAT, SR_LIFTED, SR_FEATS, SR_PREDS, SR_VIEW, SR_ROT };
struct SRef {
  int32_t space = SR_NONE;
  int32_t idx = 0;
  int64_t off = 0;
};

// One library call of the forward.  r / i / n by op - see the executor (session.hip: run_step), which is their only reader.
enum SOp {
  SOP_NCHW_TO_NHWC4 = 0, SOP_PREPROCESS_U8, SOP_CONV_AFFINE, SOP_CONV_SPLIT_AFFINE, SOP_MAXPOOL, SOP_SPLIT_F32, SOP_AVGPOOL,
  SOP_AVGPOOL_SPLIT, SOP_LINEAR, SOP_FUSER, SOP_SKINNY, SOP_RELROT, SOP_CLEAR, SOP_ABSMAX, SOP_FUSE_BUILD, SOP_LINEAR_SPLIT,
  // the bf16 inference form (MVG_SESSION_BF16)
  SOP_NCHW_TO_NHWC8_BF16, SOP_PREPROCESS_U8_BF16, SOP_CONV_BF16, SOP_BN_RELU_MAXPOOL_BF16, SOP_CONV_BF16_AFFINE, SOP_AVGPOOL_BF16,
  SOP_LINEAR_MIXED, SOP_ROTCAT, SOP_COUNT
};
const char *sop_name(int op);              // the entry point the op calls, without the "mvg_" prefix (session_plan.cpp)
struct SStep {
  int32_t op = 0;
  mvg_conv_desc d = {};
  SRef r[16];
  int32_t i[6] = {0, 0, 0, 0, 0, 0};
  int64_t n = 0;             // element / byte count, or the floats of the Linear workspace in r[..]
  int64_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int32_t range = -1;        // SOP_SPLIT_F32 / an sp-writing SOP_CONV_SPLIT_AFFINE: the step's word of the range record; else -1
};

// A byte range of the workspace, live from step `first` to step `last` (inclusive).  Persistent buffers (what bind
// writes: tables, weight copies, folded BatchNorms) are live from -1 to INT32_MAX.
struct SBuf {
  int64_t bytes = 0;
  int32_t first = 0, last = 0;
  int64_t off = -1;
  const char *what = "";
};

struct STensor {
  std::string name;
  int64_t numel = 0;
};

struct SBnFold {             // one record of mvg_bn_eval_affine_batch: tensors gamma .. gamma + 3, (scale, shift) at aff_off
  int32_t gamma = 0, c = 0;
  int64_t aff_off = 0;       // bytes into buf_affine: scale[c] then shift[c]
  int64_t shift_off = -1;    // bytes into buf_affine of shift[c] when it does not follow the scale (the bf16 stem's [V][c] rows)
};
struct SWPrep {              // one record of mvg_weights_prep_batch (no transposed copy): mode 1 (sp), or mode 0 (bf16) in a bf16 session
  int32_t tensor = 0, stat = 0, cout = 0, rs = 0, cin = 0;
  int64_t wk_off = 0;        // bytes into buf_wk
  int32_t cin_pad = 0;       // mode 0: the copy's channels per tap (the stem: 3 -> 8); 0 = cin
};

constexpr int SESSION_MAX_VIEWS = 8;            // the pair tables travel to the device as a kernel argument
constexpr int SESSION_SLOTS = 64;               // the split head path's statistics arena (heads.FusionHead._SLOTS)
constexpr size_t SESSION_SCRATCH_BYTES = (size_t)256 * 4 * 2 * 128 * 128 * sizeof(float);   // mvg_scratch_bytes() with 256 CUs

struct SessionPlan {
  std::vector<STensor> tensors;
  std::vector<SStep> steps;
  std::vector<SBuf> bufs;
  std::vector<SBnFold> folds;
  std::vector<SWPrep> wprep_backbone, wprep_head;
  int32_t stem_weight = -1;                     // tensor: the 3-channel stem filter bind pads to 4 channels (buf_w4)
  int32_t stem_cout = 0;
  int32_t compute = MVG_SESSION_FP32;           // MVG_SESSION_FP32 | MVG_SESSION_BF16: which of the two forms the steps state
  int32_t buf_tables = -1, buf_rows = -1, buf_affine = -1, buf_wstat = -1, buf_wk = -1, buf_w4 = -1, buf_slots = -1,
          buf_scratch = -1;
  int32_t buf_dirs = -1;                        // bf16 form: the per-direction tables of mvg_rotcat_fwd (partner, ident)
  int64_t dirs_partner = 0, dirs_ident = 0;     // byte offsets inside buf_dirs
  int64_t tab_folds = 0, tab_wprep_backbone = 0, tab_wprep_head = 0, tab_bytes = 0;   // byte offsets inside buf_tables
  int64_t rows_vi = 0, rows_vj = 0, rows_img = 0, rows_view = 0, rows_partner = 0, rows_ident = 0;   // inside buf_rows
  int32_t dirs = 0, head_rows = 0, max_c = 0;
  int32_t split_now = 0;                        // the backbone runs on the split kernels (cfg.split and the 2 GiB guard)
  int32_t head_split = 0;                       // the fuser / head Linears run on the split kernels (>= 1024 rows)
  int32_t fc_dim = 0;
  std::vector<std::string> range_units;         // range record: word -> the conv whose unit writes that sp tensor (forward order)
  int64_t workspace_bytes = 0;
};

}  // namespace mvg

struct mvg_session {
  mvg_session_cfg cfg;
  mvg::SessionPlan plan;
  // executor state (session.hip)
  std::vector<const void *> tensor_ptrs;
  char *workspace = nullptr;
  size_t workspace_bytes = 0;
  void *bound_stream = nullptr;
  bool bound = false;
  uint32_t *range_record = nullptr;             // mvg_session_set_range_record: device words, or null (no record)
  // mvg_session_set_error_record: what mvg_gaze_error_update takes after the last step; err_record null = no update
  const float *err_gt = nullptr;
  double *err_record = nullptr;
  float *err_out = nullptr;
  int64_t err_capacity = 0;
  // mvg_session_set_consensus: what mvg_gaze_consensus_fwd takes after the last step; cons_views null = no consensus launch
  const float *cons_weights = nullptr;
  float *cons_head = nullptr;
  float *cons_views = nullptr;
  float *cons_stats = nullptr;
};
