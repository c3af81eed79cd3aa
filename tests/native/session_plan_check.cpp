// Stand-alone check of the inference session's plan builder (rot-mvgaze_amd/csrc/session_plan.cpp): compiled together with
// that file alone - no HIP, no Python - under -fsanitize=address,undefined and run as a plain executable by
// tests/test_session_cpu.py.  Creates, queries and destroys sessions over the grid the CPU tests use, runs check_plan
// (session_check.h) on each - the fp32-MFMA and split plans' buffers, checked apart from the builder's self-check - and tries
// the rejected configurations; exits 0 when everything holds.
#include <set>
#include <string>

#include "session_check.h"

static void expect_rejected(const mvg_session_cfg *cfg, const char *what) {
  mvg_session *s = (mvg_session *)0x1;
  g_err[0] = 0;
  const int rc = mvg_session_create(cfg, &s);
  EXPECT(rc != 0 && s == nullptr && g_err[0] != 0, "%s: rc %d, handle %p, message '%s'", what, rc, (void *)s, g_err);
  if (rc == 0) mvg_session_destroy(s);
}

int main() {
  long created = 0;
  const int depths[2] = {18, 50}, sizes[2] = {64, 224}, batches[5] = {1, 3, 8, 85, 86};
  for (int depth : depths)
    for (int views = 2; views <= 4; ++views)
      for (int batch : batches)
        for (int hw : sizes)
          for (int split = 0; split < 2; ++split)
            for (int raw = 0; raw < 2; ++raw)
              for (int share = 0; share < 2; ++share) {
                const mvg_session_cfg c = make_cfg(depth, views, batch, hw, split, raw, share);
                mvg_session *s = nullptr;
                const int rc = mvg_session_create(&c, &s);
                EXPECT(rc == 0 && s != nullptr, "create(%d, V%d, B%d, %d px, split %d, raw %d, share %d): rc %d '%s'", depth, views, batch,
                       hw, split, raw, share, rc, g_err);
                if (rc != 0 || !s) continue;
                ++created;
                const int nt = mvg_session_num_tensors(s);
                const int convs = depth == 18 ? 20 : 53, mods = share ? 1 : 3;
                EXPECT(nt == 5 * convs + 4 + 8 * mods, "tensor count %d", nt);
                std::set<std::string> seen;
                for (int i = 0; i < nt; ++i) {
                  const char *name = mvg_session_tensor_name(s, i);
                  EXPECT(name != nullptr && name[0] == '_' && mvg_session_tensor_numel(s, i) > 0, "tensor %d has no name or size", i);
                  if (name) EXPECT(seen.insert(name).second, "tensor name %s appears twice", name);
                }
                EXPECT(mvg_session_tensor_name(s, nt) == nullptr && mvg_session_tensor_name(s, -1) == nullptr, "out-of-range name");
                EXPECT(mvg_session_tensor_numel(s, nt) == -1, "out-of-range numel");
                EXPECT(mvg_session_workspace_bytes(s) > 0 && mvg_session_launches(s) > 0, "empty plan");
                char tag[96];
                snprintf(tag, sizeof(tag), "R%d V%d B%d %dpx split%d raw%d share%d", depth, views, batch, hw, split, raw, share);
                check_plan(s, MVG_SESSION_FP32, tag);
                mvg_session_destroy(s);
              }
  // out of scope
  mvg_session_cfg c = make_cfg(34, 2, 2, 64, 1, 0, 0);
  expect_rejected(&c, "depth 34");
  c = make_cfg(18, 1, 2, 64, 1, 0, 0);
  expect_rejected(&c, "one view");
  c = make_cfg(18, 2, 0, 64, 1, 0, 0);
  expect_rejected(&c, "batch 0");
  c = make_cfg(18, 2, 2, 64, 1, 1, 0);
  c.in_h = 0;
  expect_rejected(&c, "raw_u8 without a patch size");
  c = make_cfg(18, 2, 2, 16, 1, 0, 0);
  expect_rejected(&c, "16 px");
  expect_rejected(nullptr, "null cfg");
  mvg_session_destroy(nullptr);
  if (g_fail) {
    fprintf(stderr, "session_plan_check: %d failures\n", g_fail);
    return 1;
  }
  printf("session_plan_check: ok, %ld sessions\n", created);
  return 0;
}
