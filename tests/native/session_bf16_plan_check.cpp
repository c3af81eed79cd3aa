// Stand-alone check of the bf16 form of the inference session's plan (rot-mvgaze_amd/csrc/session_plan.cpp): compiled together
// with that file alone - no HIP, no Python - under -fsanitize=address,undefined and run as a plain executable by
// tests/test_session_bf16_cpu.py.  Reads the plan itself (session_plan.h) over depth x views 2..8 x batch {1, 2, 5} x
// {32, 64, 224} px x raw x share and runs check_plan (session_check.h) on each: no two buffers that are live at the same step
// share a byte, every reference of every step lies inside a buffer that is live at that step, every buffer ends inside the
// workspace, and the activations are bf16 (2 bytes per element).  Independent of the builder's own self-check: the live ranges
// are recomputed from the steps.  Exits 0 when everything holds.
#include "session_check.h"

int main() {
  long created = 0, rejected = 0;
  const int depths[2] = {18, 50}, sizes[3] = {32, 64, 224}, batches[3] = {1, 2, 5};
  for (int depth : depths)
    for (int views = 2; views <= 8; ++views)
      for (int batch : batches)
        for (int hw : sizes)
          for (int raw = 0; raw < 2; ++raw)
            for (int share = 0; share < 2; ++share) {
              const mvg_session_cfg c = make_cfg(depth, views, batch, hw, 1, raw, share);
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
              check_plan(s, MVG_SESSION_BF16, tag);
              mvg_session_destroy(s);
            }
  EXPECT(rejected == 0, "%ld shapes of the sweep were rejected: '%s'", rejected, g_err);   // every one is within the bf16 kernels' reach
  mvg_session *s = (mvg_session *)0x1;
  mvg_session_cfg c = make_cfg(18, 2, 2, 64, 1, 0, 0);
  EXPECT(mvg_session_create_ex(&c, 2, &s) != 0 && s == nullptr && g_err[0] != 0, "compute = 2 was accepted");
  if (g_fail) {
    fprintf(stderr, "session_bf16_plan_check: %d failures\n", g_fail);
    return 1;
  }
  printf("session_bf16_plan_check: ok, %ld sessions\n", created);
  return 0;
}
