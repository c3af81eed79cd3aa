// What the stand-alone programs of this directory share: each is compiled together with rot-mvgaze_amd/csrc/session_plan.cpp
// alone - no HIP, no Python - and run as a plain executable.  Here: the set_error the library's api.hip would provide, EXPECT,
// one make_cfg, and check_plan - the check of a plan's buffers that does not rest on the builder's own self-check.  Included by
// exactly one translation unit per program.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../rot-mvgaze_amd/csrc/session_plan.h"

// what api.hip provides inside the library
static char g_err[512] = "";
namespace mvg {
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace mvg

static int g_fail = 0;
#define EXPECT(cond, ...)          \
  do {                             \
    if (!(cond)) {                 \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");       \
      ++g_fail;                    \
    }                              \
  } while (0)

static mvg_session_cfg make_cfg(int depth, int views, int batch, int hw, int split, int raw, int share) {
  mvg_session_cfg c;
  memset(&c, 0, sizeof(c));
  c.depth = depth;
  c.num_iter = 3;
  c.views = views;
  c.batch = batch;
  c.height = c.width = hw;
  c.split = split;
  c.share_weights = share;
  c.raw_u8 = raw;
  if (raw) {
    c.in_h = 80;
    c.in_w = 72;
    c.input_bgr = 1;
  }
  return c;
}

// Bytes a step's launch touches behind reference k, from the step's own arguments as the executor (session.hip: run_step)
// hands them to the entry point.  0: not known here; -1: an op this file does not know.  check_plan lets neither pass for a
// reference into a buffer of the plan (the references that return 0 below are model tensors or the forward's own arguments).
// fp32 and sp elements are 4 bytes, bf16 elements 2.
static int64_t touched(const mvg::SStep &t, int k) {
  using namespace mvg;
  const mvg_conv_desc &d = t.d;
  const int32_t *i = t.i;
  const int64_t in_elems = (int64_t)d.groups * d.n * d.h * d.w * d.cin, out_elems = (int64_t)d.groups * d.n * d.ho * d.wo * d.cout,
                w_elems = (int64_t)d.cout * d.r * d.s * d.cin;
  switch (t.op) {
    // ---- the fp32-MFMA and split forms
    case SOP_NCHW_TO_NHWC4: return k == 1 ? (int64_t)i[0] * i[2] * i[3] * 4 * 4 : 0;
    case SOP_PREPROCESS_U8: return k == 1 ? (int64_t)i[0] * i[3] * i[4] * 4 * 4 : 0;
    case SOP_CONV_AFFINE:
      if (k == 0) return in_elems * 4;
      if (k == 1) return w_elems * 4;                               // the stem's 4-channel filter (buf_w4); else a model tensor
      if (k == 2 || k == 5) return out_elems * 4;
      return (int64_t)d.cout * 4;                                   // scale, shift
    case SOP_CONV_SPLIT_AFFINE:
      if (k == 0) return in_elems * 4;
      if (k == 1) return w_elems * 4;
      if (k == 2) return 4;                                         // the weight copy's sinv
      if (k == 3 || k == 6) return out_elems * 4;
      return (int64_t)d.cout * 4;                                   // scale, shift
    case SOP_MAXPOOL:
      if (k == 0) return (int64_t)i[0] * i[1] * i[2] * i[3] * 4;
      if (k == 1) return (int64_t)i[0] * i[4] * i[5] * i[3] * 4;
      return (int64_t)i[0] * i[4] * i[5] * i[3];                    // argmax, one byte per element
    case SOP_SPLIT_F32: return t.n * 4;
    case SOP_AVGPOOL:
    case SOP_AVGPOOL_SPLIT: return k == 0 ? (int64_t)i[0] * i[1] * i[2] * 4 : 0;
    case SOP_LINEAR:
      if (k == 0) return (int64_t)i[1] * i[2] * 4;
      if (k == 3) return (int64_t)i[1] * i[3] * 4;
      if (k == 4) return t.n * 4;                                   // the split-K workspace
      return 0;
    case SOP_FUSER:
      if (k == 2) return (int64_t)i[1] * 36;                        // one 3x3 rotation per row
      if (k == 3 || k == 4) return (int64_t)i[1] * 4;
      if (k == 7) return (int64_t)i[1] * i[3] * 4;
      if (k == 8) return t.n * 4;
      return 0;
    case SOP_SKINNY: return k == 0 ? (int64_t)i[0] * i[1] * 4 : 0;
    case SOP_RELROT: return k == 3 ? (int64_t)i[2] * i[0] * 36 : (int64_t)i[2] * 4;
    case SOP_CLEAR: return t.n;
    case SOP_ABSMAX: return k < 8 ? t.cnt[k] * 4 : 4;
    case SOP_FUSE_BUILD:
      if (k == 2) return (int64_t)i[0] * 36;
      if (k >= 3 && k <= 5) return (int64_t)i[0] * 4;
      if (k == 6 || k == 7) return (int64_t)i[0] * (i[1] + 1536) * 4;
      return k >= 8 ? 4 : 0;                                        // abs-max and scale slots
    case SOP_LINEAR_SPLIT:
      if (k == 0) return (int64_t)i[0] * i[1] * 4;
      if (k == 2) return (int64_t)i[2] * i[1] * 4;
      if (k == 5) return (int64_t)i[0] * i[2] * 4;
      return k == 4 ? 0 : 4;                                        // slots (the bias is a model tensor)
    // ---- the bf16 form
    case SOP_NCHW_TO_NHWC8_BF16: return k == 1 ? (int64_t)i[0] * i[2] * i[3] * 8 * 2 : 0;
    case SOP_PREPROCESS_U8_BF16: return k == 1 ? (int64_t)i[0] * i[3] * i[4] * 8 * 2 : 0;
    case SOP_CONV_BF16:
    case SOP_CONV_BF16_AFFINE:
      if (k == 0) return in_elems * 2;
      if (k == 1) return w_elems * 2;
      if (k == 2 || k == 5) return out_elems * 2;
      return (int64_t)d.cout * 4;                                   // scale, shift
    case SOP_BN_RELU_MAXPOOL_BF16: {
      const int64_t img = (int64_t)i[0] * i[1];
      if (k == 0) return img * i[2] * i[3] * i[4] * 2;
      if (k == 1 || k == 2) return (int64_t)i[0] * i[4] * 4;        // [groups][c] rows
      if (k == 3) return img * t.cnt[0] * t.cnt[1] * i[4] * 2;
      return img * t.cnt[0] * t.cnt[1] * i[4];                      // argmax, one byte per element
    }
    case SOP_AVGPOOL_BF16: return k == 0 ? (int64_t)i[0] * i[1] * i[2] * 2 : 0;
    case SOP_LINEAR_MIXED:
      if (k == 0) return (int64_t)i[1] * i[2] * 4;
      if (k == 1) return (int64_t)i[3] * i[2] * 2;
      if (k == 3) return (int64_t)i[1] * i[3] * 4;
      return 0;
    case SOP_ROTCAT:
      if (k == 2) return (int64_t)i[1] * i[0] * 36;
      if (k == 3 || k == 4) return (int64_t)i[1] * 4;
      if (k == 5) return (int64_t)i[1] * i[0] * (i[2] + 3 * i[3]) * 4;
      return 0;
    default: return -1;
  }
}

// No two buffers that are live at the same step share a byte, every reference of every step lies, with all the bytes its launch
// touches, inside a buffer that is live at that step, and every buffer ends inside the workspace.  The live ranges are
// recomputed here from the steps; what bind writes (every p.buf_* the plan holds) is live throughout.  compute: the form the
// session was created for - the plan must state it and hold no op of the other form.
static void check_plan(const mvg_session *s, int32_t compute, const char *tag) {
  using namespace mvg;
  const SessionPlan &p = s->plan;
  const int nb = (int)p.bufs.size(), ns = (int)p.steps.size();
  const bool bf16 = compute == MVG_SESSION_BF16;
  EXPECT(p.compute == compute && mvg_session_compute(s) == compute, "%s: the plan states form %d, the session was created for %d", tag, p.compute, compute);
  // a form queues its own ops only; the relative rotations and the heads' 512 -> 2 layer are the same call in both
  for (int k = 0; k < ns; ++k) {
    const int op = p.steps[k].op;
    const bool both = op == SOP_SKINNY || op == SOP_RELROT, bf16_op = op >= SOP_NCHW_TO_NHWC8_BF16 && op < SOP_COUNT;
    EXPECT(op >= 0 && op < SOP_COUNT && (both || bf16_op == bf16), "%s: step %d holds op %d, which the %s form does not queue", tag, k, op,
           bf16 ? "bf16" : "fp32");
  }
  if (bf16) {
    EXPECT(p.range_units.empty() && p.buf_w4 < 0 && p.buf_slots < 0 && p.buf_wstat < 0 && p.buf_dirs >= 0, "%s: not a bf16 plan", tag);
  } else {
    EXPECT(p.buf_dirs < 0 && p.buf_w4 >= 0 && p.buf_wstat >= 0 && p.buf_slots >= 0, "%s: not an fp32 plan", tag);
    EXPECT(p.range_units.empty() == (p.split_now == 0), "%s: %zu range units with split_now %d", tag, p.range_units.size(), p.split_now);
  }
  EXPECT(p.buf_tables >= 0 && p.buf_rows >= 0 && p.buf_affine >= 0 && p.buf_wk >= 0 && p.buf_scratch >= 0, "%s: a persistent buffer is missing", tag);
  std::vector<int> first(nb, ns), last(nb, -1);
  const int persistent[] = {p.buf_tables, p.buf_rows, p.buf_dirs, p.buf_affine, p.buf_wstat, p.buf_wk, p.buf_w4, p.buf_slots, p.buf_scratch};
  for (int b : persistent) {
    if (b < 0) continue;
    EXPECT(b < nb, "%s: a persistent buffer is numbered %d of %d", tag, b, nb);
    if (b < nb) {
      first[b] = -1;
      last[b] = ns;
    }
  }
  for (int k = 0; k < ns; ++k)
    for (int r = 0; r < 16; ++r) {
      const SRef &ref = p.steps[k].r[r];
      if (ref.space != SR_BUF) continue;
      EXPECT(ref.idx >= 0 && ref.idx < nb, "%s: step %d names buffer %d of %d", tag, k, ref.idx, nb);
      if (ref.idx < 0 || ref.idx >= nb) continue;
      first[ref.idx] = std::min(first[ref.idx], k);
      last[ref.idx] = std::max(last[ref.idx], k);
      const SBuf &b = p.bufs[ref.idx];
      const int64_t n = touched(p.steps[k], r);
      EXPECT(n > 0, "%s: step %d (op %d) reference %d into buffer %d (%s) has no known extent (%lld)", tag, k, p.steps[k].op, r, ref.idx, b.what,
             (long long)n);
      EXPECT(ref.off >= 0 && ref.off + std::max<int64_t>(n, 1) <= b.bytes, "%s: step %d (%s) reference %d [%lld, +%lld) leaves buffer %d (%s, %lld bytes)",
             tag, k, sop_name(p.steps[k].op), r, (long long)ref.off, (long long)n, ref.idx, b.what, (long long)b.bytes);
      EXPECT(k >= b.first && k <= b.last, "%s: step %d uses buffer %d (%s) outside the live range the plan gave it", tag, k, ref.idx, b.what);
    }
  for (int a = 0; a < nb; ++a) {
    const SBuf &x = p.bufs[a];
    EXPECT(x.off >= 0 && x.off % 256 == 0 && x.bytes >= 0 && x.off + x.bytes <= p.workspace_bytes, "%s: buffer %d (%s) leaves the workspace", tag, a, x.what);
    if (x.bytes == 0 || last[a] < first[a]) continue;
    for (int b = a + 1; b < nb; ++b) {
      const SBuf &y = p.bufs[b];
      if (y.bytes == 0 || last[b] < first[b] || std::max(first[a], first[b]) > std::min(last[a], last[b])) continue;
      EXPECT(!(x.off < y.off + y.bytes && y.off < x.off + x.bytes), "%s: buffers %d (%s) and %d (%s) are live together and share bytes", tag, a,
             x.what, b, y.what);
    }
  }
  EXPECT(mvg_session_workspace_bytes(s) == (size_t)p.workspace_bytes && p.workspace_bytes > 0, "%s: workspace size", tag);
  EXPECT(mvg_session_num_steps(s) == ns && mvg_session_launches(s) == ns && mvg_session_num_range_units(s) == (int)p.range_units.size(),
         "%s: queries", tag);
}
