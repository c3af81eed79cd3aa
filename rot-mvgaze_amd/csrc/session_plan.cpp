// The inference session's plan builder and its host-only entry points (mvg_session_create / _destroy and the queries).
// No HIP here, like pair_index.cpp: this file compiles and runs stand-alone (tests/native/session_plan_check.cpp).
//
// The plan restates, as data, what the Python module decides per call for model.eval() under torch.no_grad().  Every step is
// one call of an existing entry point; session.hip executes them.  One Builder holds what the compute forms share, each part
// written once:
//   register_model  arch.py's layer table and the Linears of heads.py, as tensors in state_dict order
//   table_buffers   the record tables and the pair / row tables that bind writes
//   input_layout    Backbone._input_layout, one launch per view
//   block_loop      Backbone._forward_infer's unit order (backbone.py: conv1.., downsample, last conv with the residual)
//   relrot, skinny  FusionHead.forward's relative rotations and the heads' 512 -> 2 layer (heads.py)
//   finish          offsets for every buffer and the self-check
// and two form functions state what differs:
//   build           the fp32 path: Backbone.forward's 2 GiB guard, the stem, Backbone._unit_infer's launch per unit (fp32-MFMA
//                   or split), heads.plan_head's choice between the generated-input fp32-MFMA Linears (_forward_fp32) and
//                   _forward_split (heads.py: D * B >= 1024 rows)
//   build_bf16      the bf16 storage path (MVG_SESSION_BF16): the bf16 branches of Backbone._input_layout, _forward_infer,
//                   _unit_infer and the non-training pool=True branch of _unit_fwd (backbone.py), and a Family.BF16 call of
//                   FusionHead.forward (_forward_fp32) with heads.layer_launch per layer (heads.py)
// A change to the forward's order in backbone.py / heads.py is made once here, in the shared part; a change to a form's
// launches in that form's function.  Buffer ids are creation order and decide the offsets (allocate breaks ties of first use
// by id), so the order in which each form calls new_buf is part of the plan and is frozen by
// tests/golden/session_plan_digests.txt - also where it is not the order of first use (fp32: the Linear split-K workspace
// before the lifter's hidden layer, the pool argmax between the two pooled maps).  Moving a new_buf moves the fixture.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <new>

#include "session_plan.h"

namespace {
using namespace mvg;

constexpr int NVEC = 512, ROT_DIM = 3 * NVEC, HEAD_HID = 512;
constexpr int SPLIT_MIN_ROWS = 1024;             // heads.SPLIT_MIN_ROWS
constexpr int64_t ALIGN = 256;

struct ConvSpec {
  std::string name, bn;
  int cin, cout, k, stride, pad;
};
struct BlockSpec {
  std::vector<ConvSpec> convs;
  bool has_ds = false;
  ConvSpec ds;
};

// arch.backbone_spec
void backbone_spec(int depth, ConvSpec &stem, std::vector<BlockSpec> &blocks, int &fc_dim) {
  const std::string pre = "_feat_extractor.0.";
  const bool bottleneck = depth == 50;
  const int counts18[4] = {2, 2, 2, 2}, counts50[4] = {3, 4, 6, 3}, planes_of[4] = {64, 128, 256, 512};
  const int expansion = bottleneck ? 4 : 1;
  stem = {pre + "conv1", pre + "bn1", 3, 64, 7, 2, 3};
  fc_dim = 512 * expansion;
  int inplanes = 64;
  for (int li = 1; li <= 4; ++li) {
    const int planes = planes_of[li - 1], nblk = bottleneck ? counts50[li - 1] : counts18[li - 1];
    for (int bi = 0; bi < nblk; ++bi) {
      const int stride = (bi == 0 && li > 1) ? 2 : 1, outplanes = planes * expansion;
      const std::string p = pre + "layer" + std::to_string(li) + "." + std::to_string(bi) + ".";
      BlockSpec b;
      if (bottleneck) {
        b.convs.push_back({p + "conv1", p + "bn1", inplanes, planes, 1, 1, 0});
        b.convs.push_back({p + "conv2", p + "bn2", planes, planes, 3, stride, 1});
        b.convs.push_back({p + "conv3", p + "bn3", planes, outplanes, 1, 1, 0});
      } else {
        b.convs.push_back({p + "conv1", p + "bn1", inplanes, planes, 3, stride, 1});
        b.convs.push_back({p + "conv2", p + "bn2", planes, planes, 3, 1, 1});
      }
      if (stride != 1 || inplanes != outplanes) {
        b.has_ds = true;
        b.ds = {p + "downsample.0", p + "downsample.1", inplanes, outplanes, 1, stride, 0};
      }
      blocks.push_back(b);
      inplanes = outplanes;
    }
  }
}

mvg_conv_desc make_desc(int groups, int n, int h, int w, int cin, int cout, int k, int stride, int pad) {
  mvg_conv_desc d;
  d.groups = groups;
  d.n = n;
  d.h = h;
  d.w = w;
  d.cin = cin;
  d.cout = cout;
  d.r = d.s = k;
  d.stride = stride;
  d.pad = pad;
  d.ho = (h + 2 * pad - k) / stride + 1;
  d.wo = (w + 2 * pad - k) / stride + 1;
  return d;
}

int64_t align_up(int64_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }

struct Act {               // an activation of the backbone: a buffer holding [V][B][h][w][c]; sp: fp32 form only (both 4 bytes)
  int buf = -1;
  bool sp = false;
  int h = 0, w = 0, c = 0;
};
struct ConvT {             // a conv of the layer table: its weight tensor, its first fold record and its weight copy
  ConvSpec s;
  int t = 0, fold = -1, wprep = -1;
};
struct Lin {
  int w = 0, b = 0, fin = 0, fout = 0, wprep = -1;
};

void allocate(SessionPlan &p);
bool self_check(const SessionPlan &p, char *why, size_t n);

struct Builder {
  SessionPlan &p;
  const mvg_session_cfg &c;
  const int V, N, H, W, I, D, rows, nmod;
  const int elem;                                 // bytes per element of an activation and of a weight copy: 4 (fp32, sp), 2 (bf16)
  ConvSpec stem;
  std::vector<BlockSpec> blocks;
  int cf = 0, kin = 0;                            // arch.head_dims, default / ignore_rotmat variants: ImageFeatFuser
  std::vector<ConvT> convs;
  int ci_stem = 0;
  std::vector<std::vector<int>> blk_convs;
  std::vector<int> blk_ds;
  Lin lift0, lift1;
  std::vector<Lin> fu0, fu1, hd0, hd1;
  int64_t aff_bytes = 0, wk_bytes = 0;
  const int64_t feat_it, pred_it;                 // one iteration's bytes of the feats and preds outputs

  Builder(const mvg_session_cfg &cfg, SessionPlan &plan, int elem_bytes)
      : p(plan), c(cfg), V(cfg.views), N(cfg.batch), H(cfg.height), W(cfg.width), I(cfg.num_iter), D(V * (V - 1)), rows(D * N),
        nmod(cfg.share_weights ? 1 : I), elem(elem_bytes), feat_it((int64_t)rows * ROT_DIM * 4), pred_it((int64_t)rows * 2 * 4) {
    backbone_spec(c.depth, stem, blocks, cf);
    kin = cf + ROT_DIM;
    p.fc_dim = cf;
    p.dirs = D;
    p.head_rows = rows;
  }

  int new_buf(int64_t bytes, const char *what, bool persistent = false) {
    SBuf b;
    b.bytes = bytes;
    b.what = what;
    b.first = persistent ? -1 : INT32_MAX;
    b.last = persistent ? INT32_MAX : -1;
    p.bufs.push_back(b);
    return (int)p.bufs.size() - 1;
  }
  // a reference from the step being built (its index = steps.size()): extends the buffer's live range to it
  SRef buf(int id, int64_t off = 0) {
    SBuf &b = p.bufs[id];
    if (b.first != -1) {
      const int s = (int)p.steps.size();
      b.first = std::min(b.first, s);
      b.last = std::max(b.last, s);
    }
    return ref(SR_BUF, id, off);
  }
  static SRef ref(int space, int idx = 0, int64_t off = 0) {
    SRef r;
    r.space = space;
    r.idx = idx;
    r.off = off;
    return r;
  }
  static SRef tensor(int idx) { return ref(SR_TENSOR, idx); }
  int add_tensor(const std::string &name, int64_t numel) {
    STensor t;
    t.name = name;
    t.numel = numel;
    p.tensors.push_back(t);
    return (int)p.tensors.size() - 1;
  }
  void push(const SStep &s) { p.steps.push_back(s); }

  // one record of a weight copy of `bytes`-byte elements behind the ones before it in buf_wk; cin_pad 0 = cin
  int prep(std::vector<SWPrep> &to, int tensor, int cout, int rs, int cin, int bytes, int cin_pad) {
    SWPrep w;
    w.tensor = tensor;
    w.cout = cout;
    w.rs = rs;
    w.cin = cin;
    w.cin_pad = cin_pad;
    w.wk_off = wk_bytes;
    wk_bytes += align_up((int64_t)cout * rs * (cin_pad ? cin_pad : cin) * bytes);
    to.push_back(w);
    return (int)to.size() - 1;
  }
  void prep_lin(Lin &l, int cin_pad) { l.wprep = prep(p.wprep_head, l.w, l.fout, 1, l.fin, elem, cin_pad); }

  // The model's tensors in state_dict order: stem, blocks (each with its downsample), lifter, fusers, heads; one fold per
  // BatchNorm, the stem's `stem_folds` times (rows of scales, then rows of shifts; shift_apart: every fold names its shift).
  // conv_copy(spec): the cin_pad of the conv's weight copy (0 = cin), or -1 for a conv without one.
  template <class ConvCopy>
  void register_model(int stem_folds, bool shift_apart, ConvCopy conv_copy) {
    auto add_conv = [&](const ConvSpec &s, int nrec) {
      ConvT ct;
      ct.s = s;
      ct.t = add_tensor(s.name + ".weight", (int64_t)s.cout * s.cin * s.k * s.k);
      add_tensor(s.bn + ".weight", s.cout);
      add_tensor(s.bn + ".bias", s.cout);
      add_tensor(s.bn + ".running_mean", s.cout);
      add_tensor(s.bn + ".running_var", s.cout);
      p.max_c = std::max(p.max_c, s.cout);
      ct.fold = (int)p.folds.size();
      for (int v = 0; v < nrec; ++v) {
        SBnFold f;
        f.gamma = ct.t + 1;
        f.c = s.cout;
        f.aff_off = aff_bytes + 4LL * s.cout * v;
        if (shift_apart) f.shift_off = aff_bytes + 4LL * s.cout * (nrec + v);
        p.folds.push_back(f);
      }
      aff_bytes += align_up(2LL * nrec * s.cout * 4);
      const int cin_pad = conv_copy(s);
      if (cin_pad >= 0) ct.wprep = prep(p.wprep_backbone, ct.t, s.cout, s.k * s.k, s.cin, elem, cin_pad);
      convs.push_back(ct);
      return (int)convs.size() - 1;
    };
    ci_stem = add_conv(stem, stem_folds);
    blk_convs.resize(blocks.size());
    blk_ds.assign(blocks.size(), -1);
    for (size_t b = 0; b < blocks.size(); ++b) {
      for (const ConvSpec &s : blocks[b].convs) blk_convs[b].push_back(add_conv(s, 1));
      if (blocks[b].has_ds) blk_ds[b] = add_conv(blocks[b].ds, 1);
    }
    auto add_lin = [&](const std::string &name, int fin, int fout) {
      Lin l;
      l.fin = fin;
      l.fout = fout;
      l.w = add_tensor(name + ".weight", (int64_t)fout * fin);
      l.b = add_tensor(name + ".bias", fout);
      return l;
    };
    lift0 = add_lin("_lifter._lifter.blocks.0.0", cf, ROT_DIM);
    lift1 = add_lin("_lifter._lifter.blocks.1.0", ROT_DIM, ROT_DIM);
    fu0.resize(nmod), fu1.resize(nmod), hd0.resize(nmod), hd1.resize(nmod);
    for (int i = 0; i < nmod; ++i) {
      const std::string pre = "_img_fusers." + std::to_string(i) + "._fuser.blocks.";
      fu0[i] = add_lin(pre + "0.0", kin, kin);
      fu1[i] = add_lin(pre + "1.0", kin, ROT_DIM);
    }
    for (int i = 0; i < nmod; ++i) {
      const std::string pre = "_gaze_estimators." + std::to_string(i) + ".blocks.";
      hd0[i] = add_lin(pre + "0.0", kin, HEAD_HID);
      hd1[i] = add_lin(pre + "1.0", HEAD_HID, 2);
    }
  }

  // The first two persistent buffers (bind writes them), once the folds and the weight-copy records are complete; the form
  // creates the rest of its persistent buffers behind them
  void table_buffers() {
    p.tab_folds = 0;
    p.tab_wprep_backbone = align_up((int64_t)p.folds.size() * 56);
    p.tab_wprep_head = p.tab_wprep_backbone + align_up((int64_t)p.wprep_backbone.size() * 48);
    p.tab_bytes = p.tab_wprep_head + align_up((int64_t)p.wprep_head.size() * 48);
    p.buf_tables = new_buf(p.tab_bytes, "record tables", true);
    const int64_t rt = align_up((int64_t)rows * 4), dt = align_up((int64_t)D * 4);
    p.rows_vi = 0;
    p.rows_vj = dt;
    p.rows_img = 2 * dt;
    p.rows_view = 2 * dt + rt;
    p.rows_partner = 2 * dt + 2 * rt;
    p.rows_ident = 2 * dt + 3 * rt;
    p.buf_rows = new_buf(2 * dt + 4 * rt, "pair / row tables", true);
  }

  SRef scale_of(int ci) const { return ref(SR_BUF, p.buf_affine, p.folds[convs[ci].fold].aff_off); }
  SRef shift_of(int ci) const {
    const SBnFold &f = p.folds[convs[ci].fold];
    return ref(SR_BUF, p.buf_affine, f.shift_off >= 0 ? f.shift_off : f.aff_off + 4LL * f.c);
  }
  SRef wk_of(const SWPrep &w) const { return ref(SR_BUF, p.buf_wk, w.wk_off); }
  SRef rows_ref(int64_t off) const { return ref(SR_BUF, p.buf_rows, off); }
  int64_t act_bytes(int h, int w, int ch) const { return (int64_t)V * N * h * w * ch * elem; }

  // Backbone._input_layout: V launches into x0 [V][B][H][W][ch]
  int input_layout(int op_plain, int op_raw, int ch, const char *what) {
    const int x0 = new_buf(act_bytes(H, W, ch), what);
    for (int v = 0; v < V; ++v) {
      SStep s;
      s.op = c.raw_u8 ? op_raw : op_plain;
      s.r[0] = ref(SR_VIEW, v);
      s.r[1] = buf(x0, (int64_t)v * N * H * W * ch * elem);
      if (c.raw_u8) {
        s.i[0] = N; s.i[1] = c.in_h; s.i[2] = c.in_w; s.i[3] = H; s.i[4] = W; s.i[5] = c.input_bgr ? 1 : 0;
      } else {
        s.i[0] = N; s.i[1] = 3; s.i[2] = H; s.i[3] = W;
      }
      push(s);
    }
    return x0;
  }

  // Backbone._forward_infer's residual blocks over unit(conv, input, relu, residual) = the form's Backbone._unit_infer: conv +
  // folded BatchNorm (+ residual) (+ ReLU) in one launch.  A change to the order is made in backbone.py too
  template <class Unit>
  Act block_loop(Act x, Unit unit) {
    for (size_t b = 0; b < blocks.size(); ++b) {
      Act identity = x, out = x;
      const std::vector<int> &cv = blk_convs[b];
      for (size_t k = 0; k + 1 < cv.size(); ++k) out = unit(cv[k], out, true, nullptr);
      if (blk_ds[b] >= 0) identity = unit(blk_ds[b], x, false, nullptr);
      x = unit(cv.back(), out, true, &identity);
    }
    return x;
  }

  // FusionHead.forward: the relative rotation of every directed pair, and the heads' last layer (both head paths, both forms)
  int relrot() {
    const int rel = new_buf((int64_t)rows * 9 * 4, "relative rotations");
    SStep s;
    s.op = SOP_RELROT;
    s.r[0] = ref(SR_ROT);
    s.r[1] = rows_ref(p.rows_vi);
    s.r[2] = rows_ref(p.rows_vj);
    s.r[3] = buf(rel);
    s.i[0] = N; s.i[1] = V; s.i[2] = D;
    push(s);
    return rel;
  }
  void skinny(const SRef &xin, const Lin &l, int it) {
    SStep s;
    s.op = SOP_SKINNY;
    s.r[0] = xin;
    s.r[1] = tensor(l.w);
    s.r[2] = tensor(l.b);
    s.r[3] = ref(SR_PREDS, 0, it * pred_it);
    s.i[0] = rows; s.i[1] = HEAD_HID; s.i[2] = 2;
    push(s);
  }

  int finish() {
    allocate(p);
    char why[256];
    if (!self_check(p, why, sizeof(why))) {
      set_error("session_create: the buffer plan failed its self-check: %s", why);
      return 3;
    }
    return 0;
  }

  int build();
  int build_bf16();
};

// Offsets for every buffer: in order of first use, each at the lowest offset where it overlaps no placed buffer whose live
// range intersects its own (persistent buffers come first and so sit at the bottom).
void allocate(SessionPlan &p) {
  std::vector<int> order;
  for (int i = 0; i < (int)p.bufs.size(); ++i) {
    if (p.bufs[i].first != -1 && p.bufs[i].last < 0) {      // planned but never referenced
      p.bufs[i].bytes = 0;
      p.bufs[i].first = p.bufs[i].last = 0;
    }
    order.push_back(i);
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return p.bufs[a].first < p.bufs[b].first; });
  std::vector<int> placed;
  int64_t top = 0;
  for (int id : order) {
    SBuf &b = p.bufs[id];
    const int64_t need = align_up(b.bytes);
    std::vector<std::pair<int64_t, int64_t>> busy;
    for (int q : placed) {
      const SBuf &o = p.bufs[q];
      if (o.bytes > 0 && std::max(o.first, b.first) <= std::min(o.last, b.last)) busy.push_back({o.off, o.off + align_up(o.bytes)});
    }
    std::sort(busy.begin(), busy.end());
    int64_t at = 0;
    for (const auto &iv : busy) {
      if (at + need <= iv.first) break;
      at = std::max(at, iv.second);
    }
    b.off = at;
    top = std::max(top, at + need);
    placed.push_back(id);
  }
  p.workspace_bytes = top;
}

// The guard against a stray pointer: no two buffers that are live together may share a byte, and every range ends inside the
// workspace.  Runs on every create.
bool self_check(const SessionPlan &p, char *why, size_t n) {
  const int nb = (int)p.bufs.size();
  for (int i = 0; i < nb; ++i) {
    const SBuf &a = p.bufs[i];
    if (a.off < 0 || a.off % ALIGN != 0 || a.bytes < 0 || a.off + a.bytes > p.workspace_bytes) {
      snprintf(why, n, "buffer %d (%s) [%lld, +%lld) leaves the workspace of %lld bytes", i, a.what, (long long)a.off,
               (long long)a.bytes, (long long)p.workspace_bytes);
      return false;
    }
    if (a.bytes == 0) continue;
    for (int j = i + 1; j < nb; ++j) {
      const SBuf &b = p.bufs[j];
      if (b.bytes == 0 || std::max(a.first, b.first) > std::min(a.last, b.last)) continue;
      if (a.off < b.off + b.bytes && b.off < a.off + a.bytes) {
        snprintf(why, n, "buffers %d (%s) and %d (%s) are live together and overlap", i, a.what, j, b.what);
        return false;
      }
    }
  }
  // every reference of every step stays inside its buffer and is live at that step
  for (int s = 0; s < (int)p.steps.size(); ++s)
    for (const SRef &r : p.steps[s].r) {
      if (r.space != SR_BUF) continue;
      if (r.idx < 0 || r.idx >= nb) {
        snprintf(why, n, "step %d names buffer %d of %d", s, r.idx, nb);
        return false;
      }
      const SBuf &b = p.bufs[r.idx];
      if (r.off < 0 || r.off >= std::max<int64_t>(b.bytes, 1) || s < b.first || s > b.last) {
        snprintf(why, n, "step %d reads buffer %d (%s) outside its bytes or its live range", s, r.idx, b.what);
        return false;
      }
    }
  return true;
}

// The plan of the fp32 path: the backbone on the fp32-MFMA kernels or, with cfg.split below the 2 GiB guard, on the split
// kernels; the fusers and heads on the generated-input fp32-MFMA Linears or, from 1024 rows with cfg.split, on the split Linears.
int Builder::build() {
  // Backbone.forward: one view of the largest sp tensor (layer1's output) is addressed with 32-bit offsets
  const int64_t biggest_view = (int64_t)N * ((H + 3) / 4) * ((W + 3) / 4) * blocks[0].convs.back().cout;
  p.split_now = (c.split != 0 && 4 * biggest_view < 0x7FFFFFF0LL) ? 1 : 0;
  p.head_split = (c.split != 0 && rows >= SPLIT_MIN_ROWS) ? 1 : 0;      // model.run_views: head.split = backbone.split
  if (p.head_split && !(2 + I <= 8 && 11 * I + 2 <= SESSION_SLOTS)) {
    set_error("session_create: num_iter %d is more than the split head path's slot arena serves (at most 5)", I);
    return 2;
  }

  // ---- tensors; an sp KRSC copy of every conv the split kernels run (all but the stem)
  register_model(1, false, [&](const ConvSpec &s) { return p.split_now && s.cin != 3 ? 0 : -1; });
  p.stem_weight = convs[ci_stem].t;
  p.stem_cout = stem.cout;
  if (p.head_split)
    // FusionHead._prepare_weights (Family.SPLIT): heads and fusers from the last iteration down, every Launch.SPLIT layer
    for (int i = nmod - 1; i >= 0; --i) {
      prep_lin(hd0[i], 0);
      prep_lin(fu0[i], 0);
      prep_lin(fu1[i], 0);
    }
  for (size_t k = 0; k < p.wprep_backbone.size(); ++k) p.wprep_backbone[k].stat = (int)k;
  for (size_t k = 0; k < p.wprep_head.size(); ++k) p.wprep_head[k].stat = (int)(p.wprep_backbone.size() + k);
  const int nstat = (int)(p.wprep_backbone.size() + p.wprep_head.size());

  // ---- persistent buffers (bind writes them)
  table_buffers();
  p.buf_affine = new_buf(aff_bytes, "folded BatchNorm (scale, shift)", true);
  p.buf_wstat = new_buf(std::max(nstat, 1) * 8LL, "weight copy scales", true);
  p.buf_wk = new_buf(wk_bytes, "sp weight copies (KRSC)", true);
  p.buf_w4 = new_buf((int64_t)stem.cout * stem.k * stem.k * 4 * 4, "stem filter, 4 channels", true);
  p.buf_slots = new_buf(SESSION_SLOTS * 4, "head scale slots", true);
  p.buf_scratch = new_buf((int64_t)SESSION_SCRATCH_BYTES, "scratch", true);
  auto sinv_of = [&](const SWPrep &w) { return ref(SR_BUF, p.buf_wstat, 8LL * w.stat + 4); };

  const int x0 = input_layout(SOP_NCHW_TO_NHWC4, SOP_PREPROCESS_U8, 4, "input NHWC4");

  // ---- stem: fp32-MFMA kernel on the 4-channel image (also on the split path), plain max pool, split of the pooled map
  const mvg_conv_desc dstem = make_desc(V, N, H, W, 4, stem.cout, stem.k, stem.stride, stem.pad);
  if (dstem.ho < 1 || dstem.wo < 1) {
    set_error("session_create: %d x %d is too small for the stem", H, W);
    return 2;
  }
  const int ystem = new_buf(act_bytes(dstem.ho, dstem.wo, stem.cout), "stem output");
  {
    SStep s;
    s.op = SOP_CONV_AFFINE;
    s.d = dstem;
    s.r[0] = buf(x0);
    s.r[1] = ref(SR_BUF, p.buf_w4);
    s.r[2] = buf(ystem);
    s.r[3] = scale_of(ci_stem);
    s.r[4] = shift_of(ci_stem);
    s.i[0] = 1;
    push(s);
  }
  const int hp = (dstem.ho + 2 - 3) / 2 + 1, wp = (dstem.wo + 2 - 3) / 2 + 1;
  Act x;
  x.h = hp;
  x.w = wp;
  x.c = stem.cout;
  {
    const int pooled = new_buf(act_bytes(hp, wp, stem.cout), "pooled map");
    const int argmax = new_buf((int64_t)V * N * hp * wp * stem.cout, "pool argmax");
    SStep s;
    s.op = SOP_MAXPOOL;
    s.r[0] = buf(ystem);
    s.r[1] = buf(pooled);
    s.r[2] = buf(argmax);
    s.i[0] = V * N; s.i[1] = dstem.ho; s.i[2] = dstem.wo; s.i[3] = stem.cout; s.i[4] = hp; s.i[5] = wp;
    push(s);
    x.buf = pooled;
    if (p.split_now) {
      const int pooled_sp = new_buf(act_bytes(hp, wp, stem.cout), "pooled map (sp)");
      SStep t;
      t.op = SOP_SPLIT_F32;
      t.r[0] = buf(pooled);
      t.r[1] = buf(pooled_sp);
      t.n = (int64_t)V * N * hp * wp * stem.cout;
      t.range = (int32_t)p.range_units.size();
      p.range_units.push_back(stem.name);
      push(t);
      x.buf = pooled_sp;
      x.sp = true;
    }
  }

  // ---- residual blocks: Backbone._unit_infer, fp32-MFMA and split forms.  An empty map is clamped to 1 so that the walk
  // finishes, and reported after it
  bool bad_size = false;
  x = block_loop(x, [&](int ci, const Act &in, bool relu, const Act *residual) {
    const ConvSpec &cs = convs[ci].s;
    const mvg_conv_desc d = make_desc(V, N, in.h, in.w, cs.cin, cs.cout, cs.k, cs.stride, cs.pad);
    if (d.ho < 1 || d.wo < 1) bad_size = true;
    Act out;
    out.h = std::max(d.ho, 1);
    out.w = std::max(d.wo, 1);
    out.c = cs.cout;
    out.buf = new_buf(act_bytes(out.h, out.w, out.c), "unit output");
    SStep s;
    s.d = d;
    if (p.split_now) {
      // the epilogue writes the next conv's sp operand; the downsample branch (no ReLU), read only as a residual, stays fp32
      const SWPrep &w = p.wprep_backbone[convs[ci].wprep];
      out.sp = relu;
      s.op = SOP_CONV_SPLIT_AFFINE;
      s.r[0] = buf(in.buf);
      s.r[1] = wk_of(w);
      s.r[2] = sinv_of(w);
      s.r[3] = buf(out.buf);
      s.r[4] = scale_of(ci);
      s.r[5] = shift_of(ci);
      if (residual) s.r[6] = buf(residual->buf);
      s.i[0] = out.sp ? 1 : 0;
      s.i[1] = (residual && residual->sp) ? 1 : 0;
      s.i[2] = relu ? 1 : 0;
      if (out.sp) {
        s.range = (int32_t)p.range_units.size();
        p.range_units.push_back(cs.name);
      }
    } else {
      s.op = SOP_CONV_AFFINE;
      s.r[0] = buf(in.buf);
      s.r[1] = tensor(convs[ci].t);
      s.r[2] = buf(out.buf);
      s.r[3] = scale_of(ci);
      s.r[4] = shift_of(ci);
      if (residual) s.r[5] = buf(residual->buf);
      s.i[0] = relu ? 1 : 0;
    }
    push(s);
    return out;
  });
  if (bad_size) {
    set_error("session_create: %d x %d is too small for ResNet-%d (a layer's map would be empty)", H, W, c.depth);
    return 2;
  }
  {
    SStep s;
    s.op = x.sp ? SOP_AVGPOOL_SPLIT : SOP_AVGPOOL;
    s.r[0] = buf(x.buf);
    s.r[1] = ref(SR_IMG_FEAT);
    s.i[0] = V * N; s.i[1] = x.h * x.w; s.i[2] = cf;
    push(s);
  }

  // ---- lifter, relative rotations (both head paths)
  int64_t lin_ws_floats = 0;
  auto lin_ws = [&](int r, int fin, int fout) {       // mvg_linear_workspace_floats (session_bind verifies the match)
    const int64_t n = 16LL * r * std::max(fin, fout);
    lin_ws_floats = std::max(lin_ws_floats, n);
    return n;
  };
  lin_ws(V * N, cf, ROT_DIM);
  lin_ws(V * N, ROT_DIM, ROT_DIM);
  if (!p.head_split) {
    lin_ws(rows, kin, kin);
    lin_ws(rows, kin, ROT_DIM);
    lin_ws(rows, kin, HEAD_HID);
  }
  const int ws = new_buf(lin_ws_floats * 4, "Linear split-K workspace");
  auto linear = [&](const SRef &xin, const Lin &l, bool relu, const SRef &y, int r) {
    SStep s;
    s.op = SOP_LINEAR;
    s.r[0] = xin;
    s.r[1] = tensor(l.w);
    s.r[2] = tensor(l.b);
    s.r[3] = y;
    s.r[4] = buf(ws);
    s.i[0] = relu ? 1 : 0; s.i[1] = r; s.i[2] = l.fin; s.i[3] = l.fout;
    s.n = lin_ws(r, l.fin, l.fout);
    push(s);
  };
  const int hl = new_buf((int64_t)V * N * ROT_DIM * 4, "lifter hidden");
  linear(ref(SR_IMG_FEAT), lift0, true, buf(hl), V * N);
  linear(buf(hl), lift1, false, ref(SR_LIFTED), V * N);
  const int rel = relrot();
  const SRef t_img = rows_ref(p.rows_img), t_view = rows_ref(p.rows_view), t_partner = rows_ref(p.rows_partner),
             t_ident = rows_ref(p.rows_ident);

  if (!p.head_split) {
    // FusionHead.forward, fused_in: [img_feat | R @ F] is generated inside the first Linear's operand loader
    auto fuser = [&](const SRef &feat, int feat_rows, bool rotate, const SRef &row_src, const Lin &l, const SRef &y) {
      SStep s;
      s.op = SOP_FUSER;
      s.r[0] = ref(SR_IMG_FEAT);
      s.r[1] = feat;
      if (rotate) s.r[2] = buf(rel);
      s.r[3] = t_img;
      s.r[4] = row_src;
      s.r[5] = tensor(l.w);
      s.r[6] = tensor(l.b);
      s.r[7] = y;
      s.r[8] = buf(ws);
      s.i[0] = 1; s.i[1] = rows; s.i[2] = cf; s.i[3] = l.fout; s.i[4] = V * N; s.i[5] = feat_rows;
      s.n = lin_ws(rows, cf + ROT_DIM, l.fout);
      push(s);
    };
    for (int it = 0; it < I; ++it) {
      const int m = c.share_weights ? 0 : it;
      const int hf = new_buf((int64_t)rows * kin * 4, "fuser hidden"), hh = new_buf((int64_t)rows * HEAD_HID * 4, "head hidden");
      const SRef src = it == 0 ? ref(SR_LIFTED) : ref(SR_FEATS, 0, (it - 1) * feat_it);
      fuser(src, it == 0 ? V * N : rows, !c.ignore_rotmat, it == 0 ? t_view : t_partner, fu0[m], buf(hf));
      linear(buf(hf), fu1[m], false, ref(SR_FEATS, 0, it * feat_it), rows);
      fuser(ref(SR_FEATS, 0, it * feat_it), rows, false, t_ident, hd0[m], buf(hh));
      skinny(buf(hh), hd1[m], it);
    }
  } else {
    // FusionHead._forward_split: every operand of a split Linear with its own power-of-two scale, found without extra passes
    int nslot = 0;
    auto slot = [&]() { return ref(SR_BUF, p.buf_slots, 4LL * nslot++); };
    const SRef am_img = slot(), am_lift = slot();
    std::vector<SRef> bam(I), am_f(I);
    for (int it = 0; it < I; ++it) bam[it] = slot();
    for (int it = 0; it < I; ++it) am_f[it] = slot();
    {
      SStep s;                               // abs-max slots start at zero, every forward
      s.op = SOP_CLEAR;
      s.r[0] = ref(SR_BUF, p.buf_slots);
      s.n = SESSION_SLOTS * 4;
      push(s);
    }
    {
      SStep s;
      s.op = SOP_ABSMAX;
      s.i[0] = 2 + I;
      s.r[0] = ref(SR_IMG_FEAT);
      s.cnt[0] = (int64_t)V * N * cf;
      s.r[8] = am_img;
      s.r[1] = ref(SR_LIFTED);
      s.cnt[1] = (int64_t)V * N * ROT_DIM;
      s.r[9] = am_lift;
      for (int it = 0; it < I; ++it) {
        s.r[2 + it] = tensor(fu0[c.share_weights ? 0 : it].b);
        s.cnt[2 + it] = kin;
        s.r[10 + it] = bam[it];
      }
      push(s);
    }
    auto build_inputs = [&](const SRef &feat, const SRef &am_feat, const SRef &row_src_f, int xf, const SRef &xf_sinv, int xh,
                            const SRef &xh_sinv) {
      SStep s;
      s.op = SOP_FUSE_BUILD;
      s.r[0] = ref(SR_IMG_FEAT);
      s.r[1] = feat;
      if (!c.ignore_rotmat) s.r[2] = buf(rel);
      s.r[3] = t_img;
      s.r[4] = row_src_f;
      if (xh >= 0) s.r[5] = t_ident;
      if (xf >= 0) {
        s.r[6] = buf(xf);
        s.r[10] = xf_sinv;
      }
      if (xh >= 0) {
        s.r[7] = buf(xh);
        s.r[11] = xh_sinv;
      }
      s.r[8] = am_img;
      s.r[9] = am_feat;
      s.i[0] = rows; s.i[1] = cf;
      push(s);
    };
    auto linear_split = [&](int xin, const SRef &x_sinv, const Lin &l, bool relu, const SRef &out, bool out_sp, const SRef &out_sinv,
                            const SRef &bias_absmax, const SRef &out_absmax) {
      const SWPrep &w = p.wprep_head[l.wprep];
      SStep s;
      s.op = SOP_LINEAR_SPLIT;
      s.r[0] = buf(xin);
      s.r[1] = x_sinv;
      s.r[2] = wk_of(w);
      s.r[3] = sinv_of(w);
      s.r[4] = tensor(l.b);
      s.r[5] = out;
      s.r[6] = out_sinv;
      s.r[7] = bias_absmax;
      s.r[8] = out_absmax;
      s.i[0] = rows; s.i[1] = l.fin; s.i[2] = l.fout; s.i[3] = relu ? 1 : 0; s.i[4] = out_sp ? 1 : 0;
      push(s);
    };
    const SRef none;
    const int64_t xbytes = (int64_t)rows * kin * 4;
    int xf = new_buf(xbytes, "fuser input (sp)");
    SRef xf_sinv = slot();
    build_inputs(ref(SR_LIFTED), am_lift, t_view, xf, xf_sinv, -1, none);
    for (int it = 0; it < I; ++it) {
      const int m = c.share_weights ? 0 : it;
      const int h = new_buf(xbytes, "fuser hidden (sp)");
      const SRef h_sinv = slot();
      linear_split(xf, xf_sinv, fu0[m], true, buf(h), true, h_sinv, bam[it], none);
      linear_split(h, h_sinv, fu1[m], false, ref(SR_FEATS, 0, it * feat_it), false, none, none, am_f[it]);
      const int xh = new_buf(xbytes, "head input (sp)");
      const SRef xh_sinv = slot();
      int xf_next = -1;
      SRef xf_next_sinv;
      if (it + 1 < I) {
        xf_next = new_buf(xbytes, "fuser input (sp)");
        xf_next_sinv = slot();
      }
      build_inputs(ref(SR_FEATS, 0, it * feat_it), am_f[it], t_partner, xf_next, xf_next_sinv, xh, xh_sinv);
      const int hh = new_buf((int64_t)rows * HEAD_HID * 4, "head hidden");
      linear_split(xh, xh_sinv, hd0[m], true, buf(hh), false, none, none, none);
      skinny(buf(hh), hd1[m], it);
      xf = xf_next;
      xf_sinv = xf_next_sinv;
    }
    if (nslot > SESSION_SLOTS) {
      set_error("session_create: the split head path needs %d slots (%d available)", nslot, SESSION_SLOTS);
      return 2;
    }
  }
  return finish();
}

// ---- the bf16 form.  What the bf16 entry points require of a launch, restated so that create rejects what forward would
// (conv_shared.h: validate, fprop_geometry; conv_bf16.hip: validate_bf16, fprop_bf16_impl, launch_igemm_bf16).  a_elem: bytes
// per element of the gathered operand (2: bf16 activations; 4: the fp32 rows of mvg_linear_fprop_mixed).
bool bf16_conv_ok(const mvg_conv_desc &d, int a_elem, const char *what) {
  auto pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
  const int64_t rows = (int64_t)d.n * d.ho * d.wo, src = (int64_t)d.n * d.h * d.w;
  const char *why = nullptr;
  if (d.ho < 1 || d.wo < 1) why = "an empty output map";
  else if (d.cin % 8 != 0 || d.cout % 8 != 0) why = "cin and cout must be multiples of 8";
  else if (d.r * d.s > 1 && !(pow2(d.cin) && pow2(d.cout))) why = "a filter larger than 1x1 needs power-of-two channels";
  else if (rows >= (1LL << 31) || src >= (1LL << 31)) why = "the rows of a group overflow 32 bits";
  else if (a_elem * src * d.cin >= 0x7FFFFFF0LL || 2LL * d.cout * d.r * d.s * d.cin >= 0x7FFFFFF0LL) why = "a group of the input, or the weights, reach 2 GiB";
  else if (rows * d.cout >= (1LL << 31)) why = "a group of the output reaches 2^31 elements";
  else if ((int64_t)d.groups * ((rows + 127) / 128) * ((d.cout + (d.cout >= 128 ? 127 : 63)) / (d.cout >= 128 ? 128 : 64)) >= (1LL << 31))
    why = "the grid is too large";
  if (why) set_error("session_create (bf16): %s [%d x %d x %d x %d x %d -> %d, %dx%d / %d]: %s", what, d.groups, d.n, d.h, d.w, d.cin,
                     d.cout, d.r, d.s, d.stride, why);
  return why == nullptr;
}

// The plan of the bf16 inference form: what MultiViewGaze.run_views queues with compute_dtype = torch.bfloat16 under eval() /
// no_grad() with Backbone.bf16_fold_eval.  A change to the bf16 launches of backbone.py / heads.py is made here too.
int Builder::build_bf16() {
  p.compute = MVG_SESSION_BF16;
  // ---- tensors; one bf16 KRSC copy per conv (Backbone._prepare_weights, mode 0: every conv of spec.all_convs(), the stem's 3
  // channels padded to 8).  The stem's pass reads [V][cout] rows (Backbone._unit_fwd folds it with G = V): V records of the
  // same BatchNorm, the scale rows first, then the shift rows; every other unit one row, shift behind scale
  register_model(V, true, [](const ConvSpec &s) { return s.cin == 3 ? 8 : s.cin; });
  // heads.layer_launch: a layer is Launch.BF16 (mvg_linear_fprop_mixed) unless it is padded (a width that is no multiple of
  // 4: none in the variants a session serves) or it is a module's last layer with fout <= 4 (the heads' 512 -> 2:
  // mvg_linear_skinny_fwd)
  auto use_mixed = [](const Lin &l, bool last) { return l.fin % 4 == 0 && l.fout % 4 == 0 && !(last && l.fout <= 4); };
  // FusionHead._prepare_weights (Family.BF16): the lifter, then heads and fusers from the last iteration down
  auto prep_mixed = [&](Lin &l, bool last) {
    if (use_mixed(l, last)) prep_lin(l, l.fin);
  };
  prep_mixed(lift0, false);
  prep_mixed(lift1, true);
  for (int i = nmod - 1; i >= 0; --i) {
    prep_mixed(hd0[i], false);
    prep_mixed(hd1[i], true);
    prep_mixed(fu0[i], false);
    prep_mixed(fu1[i], true);
  }
  if (!use_mixed(lift0, false) || !use_mixed(lift1, true) || use_mixed(hd1[0], true)) {
    set_error("session_create (bf16): a Linear of this model is not on the path the session restates");
    return 2;
  }

  // ---- persistent buffers (bind writes them)
  table_buffers();
  const int64_t dt = align_up((int64_t)D * 4);
  p.dirs_partner = 0;
  p.dirs_ident = dt;
  p.buf_dirs = new_buf(2 * dt, "direction tables (partner, ident)", true);
  p.buf_affine = new_buf(aff_bytes, "folded BatchNorm (scale, shift)", true);
  p.buf_wk = new_buf(wk_bytes, "bf16 weight copies (KRSC)", true);
  p.buf_scratch = new_buf((int64_t)SESSION_SCRATCH_BYTES, "scratch", true);

  // (no row-window stem outside training)
  const int x0 = input_layout(SOP_NCHW_TO_NHWC8_BF16, SOP_PREPROCESS_U8_BF16, 8, "input NHWC8 (bf16)");

  // ---- stem (Backbone._unit_fwd, pool=True, not training): the raw conv output, then BatchNorm + ReLU + max pool in one pass
  const mvg_conv_desc dstem = make_desc(V, N, H, W, 8, stem.cout, stem.k, stem.stride, stem.pad);
  if (!bf16_conv_ok(dstem, 2, "the stem")) return 2;
  const int hp = (dstem.ho + 2 - 3) / 2 + 1, wp = (dstem.wo + 2 - 3) / 2 + 1;
  if ((int64_t)V * N * hp >= 65536) {          // mvg_bn_relu_maxpool_fwd_bf16: images x pooled rows is a grid dimension
    set_error("session_create (bf16): views x batch x pooled rows = %lld (the stem's pooling pass serves fewer than 65536)",
              (long long)V * N * hp);
    return 2;
  }
  Act x;
  {
    const int ystem = new_buf(act_bytes(dstem.ho, dstem.wo, stem.cout), "stem conv output (bf16)");
    SStep s;
    s.op = SOP_CONV_BF16;
    s.d = dstem;
    s.r[0] = buf(x0);
    s.r[1] = wk_of(p.wprep_backbone[convs[ci_stem].wprep]);
    s.r[2] = buf(ystem);
    push(s);
    const int pooled = new_buf(act_bytes(hp, wp, stem.cout), "pooled map (bf16)");
    const int argmax = new_buf((int64_t)V * N * hp * wp * stem.cout, "pool argmax");
    SStep t;
    t.op = SOP_BN_RELU_MAXPOOL_BF16;
    t.r[0] = buf(ystem);
    t.r[1] = scale_of(ci_stem);
    t.r[2] = shift_of(ci_stem);
    t.r[3] = buf(pooled);
    t.r[4] = buf(argmax);
    t.i[0] = V; t.i[1] = N; t.i[2] = dstem.ho; t.i[3] = dstem.wo; t.i[4] = stem.cout;
    t.cnt[0] = hp; t.cnt[1] = wp;
    push(t);
    x.buf = pooled;
    x.h = hp;
    x.w = wp;
    x.c = stem.cout;
  }

  // ---- residual blocks: Backbone._unit_infer's bf16 branch (one mvg_conv_fprop_bf16_affine).  Only the first launch the
  // bf16 entry points would reject is reported
  bool bad = false;
  x = block_loop(x, [&](int ci, const Act &in, bool relu, const Act *residual) {
    const ConvSpec &cs = convs[ci].s;
    const mvg_conv_desc d = make_desc(V, N, in.h, in.w, cs.cin, cs.cout, cs.k, cs.stride, cs.pad);
    if (!bad && !bf16_conv_ok(d, 2, cs.name.c_str())) bad = true;
    Act out;
    out.h = std::max(d.ho, 1);
    out.w = std::max(d.wo, 1);
    out.c = cs.cout;
    out.buf = new_buf(act_bytes(out.h, out.w, out.c), "unit output (bf16)");
    SStep s;
    s.op = SOP_CONV_BF16_AFFINE;
    s.d = d;
    s.r[0] = buf(in.buf);
    s.r[1] = wk_of(p.wprep_backbone[convs[ci].wprep]);
    s.r[2] = buf(out.buf);
    s.r[3] = scale_of(ci);
    s.r[4] = shift_of(ci);
    if (residual) s.r[5] = buf(residual->buf);
    s.i[0] = relu ? 1 : 0;
    push(s);
    return out;
  });
  if (bad) return 2;
  {
    SStep s;
    s.op = SOP_AVGPOOL_BF16;
    s.r[0] = buf(x.buf);
    s.r[1] = ref(SR_IMG_FEAT);
    s.i[0] = V * N; s.i[1] = x.h * x.w; s.i[2] = cf;
    push(s);
  }

  // ---- FusionHead.forward, mixed: lifter, relative rotations, then per iteration the materialised fuser input
  // (_fuser_input: mvg_rotcat_fwd), the fuser, the materialised head input (_head_input), the head
  auto linear = [&](const SRef &xin, const Lin &l, bool last, const SRef &y, int r) {
    const mvg_conv_desc d = make_desc(1, r, 1, 1, l.fin, l.fout, 1, 1, 0);
    if (!bad && !bf16_conv_ok(d, 4, "a Linear")) bad = true;
    SStep s;
    s.op = SOP_LINEAR_MIXED;
    s.r[0] = xin;
    s.r[1] = wk_of(p.wprep_head[l.wprep]);
    s.r[2] = tensor(l.b);
    s.r[3] = y;
    s.i[0] = last ? 0 : 1; s.i[1] = r; s.i[2] = l.fin; s.i[3] = l.fout;       // (ReLU on every layer but a module's last)
    push(s);
  };
  const int hl = new_buf((int64_t)V * N * ROT_DIM * 4, "lifter hidden");
  linear(ref(SR_IMG_FEAT), lift0, false, buf(hl), V * N);
  linear(buf(hl), lift1, true, ref(SR_LIFTED), V * N);
  const int rel = relrot();
  const SRef t_vi = rows_ref(p.rows_vi), t_vj = rows_ref(p.rows_vj), t_partner = ref(SR_BUF, p.buf_dirs, p.dirs_partner),
             t_ident = ref(SR_BUF, p.buf_dirs, p.dirs_ident);
  auto rotcat = [&](const SRef &feat, bool rotate, const SRef &src_of, int xbuf) {
    SStep s;
    s.op = SOP_ROTCAT;
    s.r[0] = ref(SR_IMG_FEAT);
    s.r[1] = feat;
    if (rotate) s.r[2] = buf(rel);
    s.r[3] = t_vi;
    s.r[4] = src_of;
    s.r[5] = buf(xbuf);
    s.i[0] = N; s.i[1] = D; s.i[2] = cf; s.i[3] = NVEC;
    push(s);
  };
  const int64_t xbytes = (int64_t)rows * kin * 4;
  for (int it = 0; it < I; ++it) {
    const int m = c.share_weights ? 0 : it;
    const SRef src = it == 0 ? ref(SR_LIFTED) : ref(SR_FEATS, 0, (it - 1) * feat_it), fn = ref(SR_FEATS, 0, it * feat_it);
    const int xf = new_buf(xbytes, "fuser input"), hf = new_buf(xbytes, "fuser hidden");
    rotcat(src, !c.ignore_rotmat, it == 0 ? t_vj : t_partner, xf);
    linear(buf(xf), fu0[m], false, buf(hf), rows);
    linear(buf(hf), fu1[m], true, fn, rows);
    const int xh = new_buf(xbytes, "head input"), hh = new_buf((int64_t)rows * HEAD_HID * 4, "head hidden");
    rotcat(fn, false, t_ident, xh);
    linear(buf(xh), hd0[m], false, buf(hh), rows);
    skinny(buf(hh), hd1[m], it);
  }
  if (bad) return 2;
  return finish();
}

}  // namespace

namespace mvg {
const char *sop_name(int op) {
  static const char *const names[SOP_COUNT] = {
      "nchw_to_nhwc4", "preprocess_u8hwc_resize", "conv_fprop_affine", "conv_fprop_split_affine", "maxpool3x3s2_fwd", "split_f32",
      "avgpool_fwd", "avgpool_fwd_split_scaled", "linear_fprop", "fuser_fprop", "linear_skinny_fwd", "relative_rotation", "memset",
      "absmax_multi", "fuse_build_split", "linear_fprop_split",
      "nchw_to_nhwc8_bf16", "preprocess_u8hwc_resize_bf16", "conv_fprop_bf16", "bn_relu_maxpool_fwd_bf16", "conv_fprop_bf16_affine",
      "avgpool_fwd_bf16", "linear_fprop_mixed", "rotcat_fwd"};
  return op >= 0 && op < SOP_COUNT ? names[op] : nullptr;
}
}  // namespace mvg

extern "C" {

int mvg_session_create(const mvg_session_cfg *cfg, mvg_session **out) { return mvg_session_create_ex(cfg, MVG_SESSION_FP32, out); }

int mvg_session_create_ex(const mvg_session_cfg *cfg, int32_t compute, mvg_session **out) {
  if (out) *out = nullptr;
  if (!cfg || !out) {
    mvg::set_error("session_create: cfg and out are required");
    return 2;
  }
  if (compute != MVG_SESSION_FP32 && compute != MVG_SESSION_BF16) {
    mvg::set_error("session_create: compute %d (MVG_SESSION_FP32 = 0 or MVG_SESSION_BF16 = 1)", (int)compute);
    return 2;
  }
  const mvg_session_cfg &c = *cfg;
  if (c.depth != 18 && c.depth != 50) {
    mvg::set_error("session_create: depth %d (the hot path covers ResNet-18 and ResNet-50)", c.depth);
    return 2;
  }
  if (c.views < 2 || c.views > mvg::SESSION_MAX_VIEWS) {
    mvg::set_error("session_create: views %d (2 .. %d)", c.views, mvg::SESSION_MAX_VIEWS);
    return 2;
  }
  if (c.batch < 1 || c.batch > 65536 || c.num_iter < 1 || c.num_iter > 64) {
    mvg::set_error("session_create: batch %d (1 .. 65536) or num_iter %d (1 .. 64) out of range", c.batch, c.num_iter);
    return 2;
  }
  if (c.height < 32 || c.width < 32 || c.height > 4096 || c.width > 4096) {
    mvg::set_error("session_create: input size %d x %d (32 .. 4096 per side: the backbone halves it five times)", c.height, c.width);
    return 2;
  }
  if (c.raw_u8 && (c.in_h < 1 || c.in_w < 1 || c.in_h > 16384 || c.in_w > 16384)) {
    mvg::set_error("session_create: raw_u8 needs the patch size (in_h %d, in_w %d)", c.in_h, c.in_w);
    return 2;
  }
  if ((int64_t)c.views * (c.views - 1) * c.batch > (1 << 24) || (int64_t)c.views * c.batch * c.height * c.width * 64 / 4 > (1LL << 40)) {
    mvg::set_error("session_create: views x batch x size is beyond what one forward addresses");
    return 2;
  }
  mvg_session *s = new (std::nothrow) mvg_session();
  if (!s) {
    mvg::set_error("session_create: out of host memory");
    return 1;
  }
  s->cfg = c;
  const int rc = compute == MVG_SESSION_BF16 ? Builder(c, s->plan, 2).build_bf16() : Builder(c, s->plan, 4).build();
  if (rc != 0) {
    delete s;
    return rc;
  }
  *out = s;
  return 0;
}

void mvg_session_destroy(mvg_session *s) { delete s; }

int mvg_session_num_tensors(const mvg_session *s) { return s ? (int)s->plan.tensors.size() : -1; }

const char *mvg_session_tensor_name(const mvg_session *s, int i) {
  if (!s || i < 0 || i >= (int)s->plan.tensors.size()) return nullptr;
  return s->plan.tensors[i].name.c_str();
}

int64_t mvg_session_tensor_numel(const mvg_session *s, int i) {
  if (!s || i < 0 || i >= (int)s->plan.tensors.size()) return -1;
  return s->plan.tensors[i].numel;
}

size_t mvg_session_workspace_bytes(const mvg_session *s) { return s ? (size_t)s->plan.workspace_bytes : 0; }

int mvg_session_launches(const mvg_session *s) { return s ? (int)s->plan.steps.size() + (s->err_record ? 1 : 0) + (s->cons_views ? 1 : 0) : -1; }

int mvg_session_compute(const mvg_session *s) { return s ? s->plan.compute : -1; }

int mvg_session_num_steps(const mvg_session *s) { return s ? (int)s->plan.steps.size() : -1; }

const char *mvg_session_step_name(const mvg_session *s, int i) {
  if (!s || i < 0 || i >= (int)s->plan.steps.size()) return nullptr;
  return mvg::sop_name(s->plan.steps[i].op);
}

int mvg_session_num_range_units(const mvg_session *s) { return s ? (int)s->plan.range_units.size() : -1; }

const char *mvg_session_range_unit_name(const mvg_session *s, int i) {
  if (!s || i < 0 || i >= (int)s->plan.range_units.size()) return nullptr;
  return s->plan.range_units[i].c_str();
}

int mvg_session_set_range_record(mvg_session *s, uint32_t *record_dev) {
  if (!s) {
    mvg::set_error("session_set_range_record: null session");
    return 2;
  }
  if (record_dev && s->plan.range_units.empty()) {
    mvg::set_error("session_set_range_record: this session's backbone is not on the split kernels (no range units)");
    return 2;
  }
  s->range_record = record_dev;
  return 0;
}

int mvg_session_set_error_record(mvg_session *s, const float *gt_dev, double *record_dev, float *err_out, int64_t capacity) {
  if (!s) {
    mvg::set_error("session_set_error_record: null session");
    return 2;
  }
  if (record_dev && !gt_dev) {
    mvg::set_error("session_set_error_record: a record needs the label buffer gt_dev");
    return 2;
  }
  if (capacity < 0 || (err_out && capacity == 0)) {
    mvg::set_error("session_set_error_record: capacity must be >= 0, and > 0 with err_out (got %lld)", (long long)capacity);
    return 2;
  }
  s->err_gt = record_dev ? gt_dev : nullptr;
  s->err_record = record_dev;
  s->err_out = record_dev ? err_out : nullptr;
  s->err_capacity = record_dev ? capacity : 0;
  return 0;
}

int mvg_session_set_consensus(mvg_session *s, const float *weights_dev, float *head, float *views_out, float *stats) {
  if (!s) {
    mvg::set_error("session_set_consensus: null session");
    return 2;
  }
  if (views_out && !head) {
    mvg::set_error("session_set_consensus: a consensus needs the head buffer with views_out");
    return 2;
  }
  s->cons_weights = views_out ? weights_dev : nullptr;
  s->cons_head = views_out ? head : nullptr;
  s->cons_views = views_out;
  s->cons_stats = views_out ? stats : nullptr;
  return 0;
}

}  // extern "C"
