// Stand-alone check of the bf16 form of the inference session's plan (rot-mvgaze_amd/csrc/session_plan.cpp): compiled together
// with that file alone - no HIP, no Python - under -fsanitize=address,undefined and run as a plain executable by
// tests/test_session_bf16_cpu.py.  Reads the plan itself (session_plan.h) over depth x views 2..8 x batch {1, 2, 5} x
// {32, 64, 224} px x raw x share: no two buffers that are live at the same step share a byte, every reference of every step
// lies inside a buffer that is live at that step, every buffer ends inside the workspace, and the activations are bf16 (2 bytes
// per element).  Independent of the builder's own self-check: the live ranges are recomputed here from the steps.  Exits 0 when
// everything holds.
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

static mvg_session_cfg make_cfg(int depth, int views, int batch, int hw, int raw, int share) {
  mvg_session_cfg c;
  memset(&c, 0, sizeof(c));
  c.depth = depth;
  c.num_iter = 3;
  c.views = views;
  c.batch = batch;
  c.height = c.width = hw;
  c.split = 1;
  c.share_weights = share;
  c.raw_u8 = raw;
  if (raw) {
    c.in_h = 80;
    c.in_w = 72;
    c.input_bgr = 1;
  }
  return c;
}

// bytes a step's launch touches behind reference k, from the step's own arguments (0: not known here - the start must still
// lie inside the buffer)
static int64_t touched(const mvg::SStep &t, int k) {
  using namespace mvg;
  const mvg_conv_desc &d = t.d;
  const int32_t *i = t.i;
  switch (t.op) {
    case SOP_NCHW_TO_NHWC8_BF16: return k == 1 ? (int64_t)i[0] * i[2] * i[3] * 8 * 2 : 0;
    case SOP_PREPROCESS_U8_BF16: return k == 1 ? (int64_t)i[0] * i[3] * i[4] * 8 * 2 : 0;
    case SOP_CONV_BF16:
    case SOP_CONV_BF16_AFFINE:
      if (k == 0) return (int64_t)d.groups * d.n * d.h * d.w * d.cin * 2;
      if (k == 1) return (int64_t)d.cout * d.r * d.s * d.cin * 2;
      if (k == 2 || k == 5) return (int64_t)d.groups * d.n * d.ho * d.wo * d.cout * 2;
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
    case SOP_RELROT: return k == 3 ? (int64_t)i[2] * i[0] * 36 : (int64_t)i[2] * 4;
    case SOP_ROTCAT:
      if (k == 2) return (int64_t)i[1] * i[0] * 36;
      if (k == 3 || k == 4) return (int64_t)i[1] * 4;
      if (k == 5) return (int64_t)i[1] * i[0] * (i[2] + 3 * i[3]) * 4;
      return 0;
    case SOP_SKINNY: return k == 0 ? (int64_t)i[0] * i[1] * 4 : 0;
    default: return -1;                                             // an op the bf16 form does not hold
  }
}

static void check_plan(const mvg_session *s, const char *tag) {
  using namespace mvg;
  const SessionPlan &p = s->plan;
  const int nb = (int)p.bufs.size(), ns = (int)p.steps.size();
  EXPECT(p.compute == MVG_SESSION_BF16 && p.range_units.empty() && p.buf_w4 < 0 && p.buf_slots < 0 && p.buf_wstat < 0, "%s: not a bf16 plan", tag);
  // live ranges from the steps alone: first / last step that names the buffer (what bind writes is live throughout)
  std::vector<int> first(nb, ns), last(nb, -1);
  const int persistent[] = {p.buf_tables, p.buf_rows, p.buf_dirs, p.buf_affine, p.buf_wk, p.buf_scratch};
  for (int b : persistent) {
    EXPECT(b >= 0 && b < nb, "%s: a persistent buffer is missing", tag);
    if (b >= 0 && b < nb) {
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
      EXPECT(n >= 0, "%s: step %d holds op %d, which the bf16 form does not queue", tag, k, p.steps[k].op);
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
  EXPECT(mvg_session_num_steps(s) == ns && mvg_session_launches(s) == ns && mvg_session_num_range_units(s) == 0, "%s: queries", tag);
}

int main() {
  long created = 0, rejected = 0;
  const int depths[2] = {18, 50}, sizes[3] = {32, 64, 224}, batches[3] = {1, 2, 5};
  for (int depth : depths)
    for (int views = 2; views <= 8; ++views)
      for (int batch : batches)
        for (int hw : sizes)
          for (int raw = 0; raw < 2; ++raw)
            for (int share = 0; share < 2; ++share) {
              const mvg_session_cfg c = make_cfg(depth, views, batch, hw, raw, share);
              char tag[96];
              snprintf(tag, sizeof(tag), "R%d V%d B%d %dpx raw%d share%d", depth, views, batch, hw, raw, share);
              mvg_session *s = (mvg_session *)0x1;
              g_err[0] = 0;
              const int rc = mvg_session_create_ex(&c, MVG_SESSION_BF16, &s);
              if (rc != 0) {                     // a rejection is sound when it says why and leaves no handle
                EXPECT(s == nullptr && g_err[0] != 0, "%s: rc %d, handle %p, message '%s'", tag, rc, (void *)s, g_err);
                ++rejected;
                continue;
              }
              EXPECT(s != nullptr && s != (mvg_session *)0x1, "%s: no handle", tag);
              ++created;
              check_plan(s, tag);
              mvg_session_destroy(s);
            }
  EXPECT(rejected == 0, "%ld shapes of the sweep were rejected: '%s'", rejected, g_err);   // every one is within the bf16 kernels' reach
  mvg_session *s = (mvg_session *)0x1;
  mvg_session_cfg c = make_cfg(18, 2, 2, 64, 0, 0);
  EXPECT(mvg_session_create_ex(&c, 2, &s) != 0 && s == nullptr && g_err[0] != 0, "compute = 2 was accepted");
  if (g_fail) {
    fprintf(stderr, "session_bf16_plan_check: %d failures\n", g_fail);
    return 1;
  }
  printf("session_bf16_plan_check: ok, %ld sessions\n", created);
  return 0;
}
