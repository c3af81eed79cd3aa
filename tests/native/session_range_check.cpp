// Stand-alone check of the inference session's activation range record as the plan builder lays it out
// (rot-mvgaze_amd/csrc/session_plan.cpp): compiled together with that file alone - no HIP, no Python - under
// -fsanitize=address,undefined and run as a plain executable by tests/test_range_guard_cpu.py.  Reads the plan itself
// (session_plan.h): every sp-writing conv step and the split of the pooled map carries a distinct word index in [0, n),
// every other step carries none, and the names are the layer table's in forward order; each plan also goes through check_plan
// (session_check.h).  Exits 0 when everything holds.
#include <string>

#include "session_check.h"

int main() {
  long checked = 0;
  const int depths[2] = {18, 50}, sizes[2] = {64, 224}, batches[5] = {1, 3, 86, 668, 669};
  for (int depth : depths)
    for (int views = 2; views <= 4; views += 2)
      for (int batch : batches)
        for (int hw : sizes)
          for (int split = 0; split < 2; ++split) {
            const mvg_session_cfg c = make_cfg(depth, views, batch, hw, split, 0, 0);
            mvg_session *s = nullptr;
            const int rc = mvg_session_create(&c, &s);
            EXPECT(rc == 0 && s != nullptr, "create(%d, V%d, B%d, %d px, split %d): rc %d '%s'", depth, views, batch, hw, split, rc, g_err);
            if (rc != 0 || !s) continue;
            ++checked;
            char tag[96];
            snprintf(tag, sizeof(tag), "R%d V%d B%d %dpx split%d", depth, views, batch, hw, split);
            check_plan(s, MVG_SESSION_FP32, tag);
            const int n = mvg_session_num_range_units(s);
            // the 2 GiB guard: one view of layer1's output (4 bytes per element) stays below 0x7FFFFFF0 bytes - ResNet-50 at 224 px
            // fits up to batch 668 and leaves the split kernels from 669
            const long long view_bytes = 4LL * batch * ((hw + 3) / 4) * ((hw + 3) / 4) * (depth == 50 ? 256 : 64);
            const bool on_split = split != 0 && view_bytes < 0x7FFFFFF0LL;
            if (depth == 50 && hw == 224) EXPECT((view_bytes < 0x7FFFFFF0LL) == (batch <= 668), "the guard's threshold moved");
            const int want = on_split ? (depth == 18 ? 17 : 49) : 0;
            EXPECT(n == want && s->plan.split_now == (on_split ? 1 : 0), "range units %d (want %d), split_now %d", n, want, s->plan.split_now);
            EXPECT(mvg_session_range_unit_name(s, n) == nullptr && mvg_session_range_unit_name(s, -1) == nullptr, "out-of-range name");
            std::vector<int> seen((size_t)(n > 0 ? n : 0), 0);
            int next = 0;
            for (size_t k = 0; k < s->plan.steps.size(); ++k) {
              const mvg::SStep &t = s->plan.steps[k];
              const bool writes_sp = t.op == mvg::SOP_SPLIT_F32 || (t.op == mvg::SOP_CONV_SPLIT_AFFINE && t.i[0] != 0);
              if (!writes_sp) {
                EXPECT(t.range == -1, "step %zu (op %d) writes no sp tensor but carries word %d", k, t.op, t.range);
                continue;
              }
              EXPECT(t.range >= 0 && t.range < n, "step %zu (op %d): word %d outside [0, %d)", k, t.op, t.range, n);
              if (t.range < 0 || t.range >= n) continue;
              EXPECT(seen[(size_t)t.range]++ == 0, "word %d is used twice", t.range);
              EXPECT(t.range == next, "word %d at step %zu is out of forward order (expected %d)", t.range, k, next);
              ++next;
              const char *name = mvg_session_range_unit_name(s, t.range);
              EXPECT(name != nullptr && strncmp(name, "_feat_extractor.0.", 18) == 0, "word %d has no conv name", t.range);
              if (name && t.op == mvg::SOP_SPLIT_F32) EXPECT(std::string(name) == "_feat_extractor.0.conv1", "the pooled map is named %s", name);
              if (name && t.op == mvg::SOP_CONV_SPLIT_AFFINE)
                EXPECT(strstr(name, "downsample") == nullptr && strstr(name, ".layer") != nullptr, "conv word %d is named %s", t.range, name);
            }
            EXPECT(next == n, "%d steps carry a word, the session reports %d", next, n);
            // the record pointer is only stored: nothing about the plan moves
            const int launches = mvg_session_launches(s);
            uint32_t fake[64];
            if (n > 0) {
              EXPECT(mvg_session_set_range_record(s, fake) == 0 && s->range_record == fake, "set_range_record");
            } else {
              g_err[0] = 0;
              EXPECT(mvg_session_set_range_record(s, fake) != 0 && g_err[0] != 0 && s->range_record == nullptr, "a record without units is rejected");
            }
            EXPECT(mvg_session_launches(s) == launches, "launches moved with a record set");
            EXPECT(mvg_session_set_range_record(s, nullptr) == 0 && s->range_record == nullptr, "clearing the record");
            mvg_session_destroy(s);
          }
  EXPECT(mvg_session_num_range_units(nullptr) == -1 && mvg_session_range_unit_name(nullptr, 0) == nullptr, "null session queries");
  EXPECT(mvg_session_set_range_record(nullptr, nullptr) != 0, "null session set");
  if (g_fail) {
    fprintf(stderr, "session_range_check: %d failures\n", g_fail);
    return 1;
  }
  printf("session_range_check: ok, %ld sessions\n", checked);
  return 0;
}
