"""tests/adamw_forms_ref.py checked on its own (no GPU), and the host-only side of decoupled weight decay in optim.py and ops.py: the
float64 reference against torch.optim.AdamW, the bars K_M / K_V / K_P against the float32 restatement they are derived from, the
table's sensitivity to coupled decay and three further wrong AdamWs, and - without a device or a launch - the planner, the plan
signature, the AdamW defaults, the checkpoint round trip and the _ex wrappers' mode check.  Every figure is printed before it is
asserted (pytest -s).

Measured here: the restatement's worst units over the table are m 1.986, v 1.986, p 1.712, all three on the BIG_N problem of hyper
set 5 (8.4 M elements; over the flat and segment arenas alone m 1.920, v 1.913, p 1.313) - K = 8, 8, 7.  Coupled decay held to the
decoupled reference leaves the m bar on all ten n = 4100 problems with wd > 0 and scale > 0, by 4.31e3 units at the least (hyper
set 4 at scale 1e-4: wd 1e-6 against |p| 1e-4)."""
import math

import numpy as np
import pytest
import torch

import adam_forms_ref as R
import adamw_forms_ref as W

TORCH_BAR = 1e-12


# ---------------------------------------------------------------- the reference against torch.optim.AdamW
@pytest.mark.parametrize("h", range(len(R.HYPER)))
def test_reference_is_torch_adamw_on_the_float32_hyper_parameters(h):
    """Five steps on n = 1020 from zero moments, torch.optim.AdamW in float64 on the CPU given the float32-rounded hyper-parameters
    the reference uses: only double rounding separates them."""
    lr, b1, b2, eps, wd, _ = R.hyper32(h)
    n = 1020
    rng = np.random.default_rng(140 + h)
    p0 = rng.standard_normal(n)
    tp = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.AdamW([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    worst = 0.0
    for step in range(1, 6):
        g = R.inputs(n, 1.0, 2, 160 + step)[1].astype(np.float64)
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        r = W.reference(p, g, m, v, lr, b1, b2, eps, wd, step)
        p, m, v = r["p"], r["m"], r["v"]
        for mine, theirs in ((p, tp.detach().numpy()), (m, opt.state[tp]["exp_avg"].numpy()), (v, opt.state[tp]["exp_avg_sq"].numpy())):
            worst = max(worst, float(np.abs(mine - theirs).max() / np.abs(theirs).max()))
    print(f"ADAMW-FORMS cpu reference vs torch.optim.AdamW float64, hyper {R.HYPER[h][:5]}: worst of p, m, v over 5 steps {worst:.2e}")
    assert worst <= TORCH_BAR


# ---------------------------------------------------------------- K
@pytest.fixture(scope="module")
def table():
    """[(name, arena, coef, per-segment decoupled references)] of everything K is measured over, computed once."""
    return [(name, a, coef, W.references(a, coef=coef)) for name, a, coef in R.measured_problems()]


def test_committed_bars_are_four_times_the_float32_restatement(table):
    worst, where = [0.0, 0.0, 0.0], ["", "", ""]
    for name, a, coef, refs in table:
        for (b, e, h), r in zip(a.segs, refs):
            lr, b1, b2, eps, wd, step = R.HYPER[h]
            p2, m2, v2 = W.float32_restatement(a.p[b:e], a.g[b:e], a.m[b:e], a.v[b:e], lr, b1, b2, eps, wd, step, coef=coef)
            w = R.worst_units(r, p2, m2, v2)
            assert all(math.isfinite(x) for x in w), (name, w)
            for i in range(3):
                if w[i] > worst[i]:
                    worst[i], where[i] = w[i], f"{name} [{b}, {e})"
    for q, w, at, k in zip("mvp", worst, where, (W.K_M, W.K_V, W.K_P)):
        print(f"ADAMW-FORMS cpu float32 restatement, worst {q}: {w:.3f} units at {at}; committed K = {k}")
        assert k == math.ceil(4 * w), f"K_{q.upper()} = {k}, four times the measured {w:.3f} rounds up to {math.ceil(4 * w)}"


def test_the_table_is_adam_forms_refs(table):
    """Nothing of the case table is restated here: the problems are adam_forms_ref's own objects, every hyper set, scale and size
    among them, and the reference's moments do not see the parameter."""
    names = [name for name, _, _, _ in table]
    assert names == [name for name, _, _ in R.measured_problems()] and len(names) == 36 + 2 * 15 + 2
    assert W.HYPER is R.HYPER and any(a.n == R.BIG_N for _, a, _, _ in table)
    a = R.flat_arenas()[3]
    lr, b1, b2, eps, wd, step = R.HYPER[a.segs[0][2]]
    r1 = W.reference(a.p, a.g, a.m, a.v, lr, b1, b2, eps, wd, step)
    r2 = W.reference(2 * a.p, a.g, a.m, a.v, lr, b1, b2, eps, wd, step)
    assert np.array_equal(r1["m"], r2["m"]) and np.array_equal(r1["v"], r2["v"]) and not np.array_equal(r1["p"], r2["p"])
    s = W.reference(a.p, a.g, a.m, a.v, lr, b1, b2, eps, wd, step, coef=0.0, skipped=True)
    assert np.array_equal(s["p"], a.p.astype(np.float64)) and np.array_equal(s["m"], a.m.astype(np.float64)) and not s["d"].any()


# ---------------------------------------------------------------- sensitivity
def _both(a, mutation=None):
    (b, e, h), = a.segs
    lr, b1, b2, eps, wd, step = R.HYPER[h]
    r = W.reference(a.p, a.g, a.m, a.v, lr, b1, b2, eps, wd, step)
    if mutation == "coupled":
        x = R.reference(a.p, a.g, a.m, a.v, lr, b1, b2, eps, wd, step)
    else:
        x = W.reference(a.p, a.g, a.m, a.v, lr, b1, b2, eps, wd, step, mutation=mutation)
    return r, x


def test_coupled_decay_leaves_the_m_bar_wherever_there_is_decay_and_a_parameter():
    seen, least = 0, (float("inf"), "")
    for a in R.flat_arenas():
        if a.n != 4100 or a.scale == 0.0 or R.HYPER[a.segs[0][2]][4] == 0.0:
            continue
        r, x = _both(a, "coupled")
        wm, wv, wp = R.worst_units(r, x["p"], x["m"], x["v"])
        print(f"ADAMW-FORMS cpu coupled decay held to the decoupled reference, {a.name}: m {wm:.3g} v {wv:.3g} p {wp:.3g} units")
        assert wm > W.K_M, a.name
        seen += 1
        least = min(least, (wm, a.name))
    print(f"ADAMW-FORMS cpu coupled decay: outside the m bar on all {seen} problems, least on {least[1]} ({least[0]:.3g} units)")
    assert seen == 10                                                     # five hyper sets with wd > 0, two scales above 0
    assert least[0] > 1e3


# mutation -> the problems that must catch it (and on which quantity)
CAUGHT_BY = {
    "f_from_step_size": ["h1_scale1_n4100", "h1_scale0.0001_n4100", "h1_scale1_n1020"],       # bc1 = 0.271 at step 3, lr wd = 1e-5
    "f_plus": ["h1_scale1_n4100", "h2_scale1_n4100", "h2_scale0.0001_n1020", "h5_scale1_n4100"],
    "lanes_xy_swapped": ["h0_scale1_n4100", "h3_scale0_n4100", "h1_scale0.0001_n4", "h4_scale0_n8"],
}


def test_every_further_mutation_exceeds_the_bars_on_the_problems_named():
    arenas = {a.name: a for a in R.flat_arenas()}
    assert set(CAUGHT_BY) == set(W.MUTATIONS)
    for mu, names in CAUGHT_BY.items():
        for name in names:
            r, x = _both(arenas[name], mu)
            wm, wv, wp = R.worst_units(r, x["p"], x["m"], x["v"])
            print(f"ADAMW-FORMS cpu mutation {mu} on {name}: m {wm:.3g} v {wv:.3g} p {wp:.3g} units")
            assert wm > W.K_M or wv > W.K_V or wp > W.K_P, (mu, name)
            if mu != "lanes_xy_swapped":
                assert wm == 0 and wv == 0 and wp > W.K_P, "a wrong f moves the parameter alone"


def test_without_weight_decay_the_two_references_agree_exactly():
    count = 0
    for a in R.flat_arenas():
        if R.HYPER[a.segs[0][2]][4] != 0.0:
            continue
        r, x = _both(a, "coupled")
        assert all(np.array_equal(r[k], x[k]) for k in ("p", "m", "v", "d", "U_m", "U_v", "U_d")), a.name
        count += 1
    assert count == 6                                                    # hyper set 3: three scales at n = 4100, one each at 4, 8, 1020


# ---------------------------------------------------------------- optim.py and ops.py without a device
def _model():
    from rot_mvgaze_amd.model import FeatRotationSymm
    return FeatRotationSymm(backbone_depth=18, num_iter=3)


def _split(m):
    bb = [p for n, p in m.named_parameters() if n.startswith("_feat_extractor")]
    head = [p for n, p in m.named_parameters() if not n.startswith("_feat_extractor")]
    return head, bb


def _entries(m):
    """An arena layout over the CPU model, head first: every parameter on a 4-element slot (any fixed order serves the planner)."""
    head, bb = _split(m)
    out, off = [], 0
    for p in head + bb:
        out.append((p, off, p.numel()))
        off += (p.numel() + 3) // 4 * 4
    return out


def test_plan_segments_splits_neighbours_that_differ_only_in_mode():
    from rot_mvgaze_amd.optim import Adam, plan_segments
    g = {"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 1e-2}
    coupled, decoupled = Adam._hyper(dict(g, decoupled_weight_decay=False)), Adam._hyper(dict(g, decoupled_weight_decay=True))
    assert coupled[:5] == decoupled[:5] and coupled != decoupled
    entries = [(0, 8), (8, 6), (16, 4)]
    segs = plan_segments(entries, [decoupled, decoupled, coupled], [True] * 3, [1] * 3)
    assert [(s.begin, s.end) for s in segs] == [(0, 16), (16, 20)] and segs[0].group == decoupled and segs[1].group == coupled
    assert len(plan_segments(entries, [coupled] * 3, [True] * 3, [1] * 3)) == 1
    assert Adam._segment_key(0, dict(g, decoupled_weight_decay=False)) != Adam._segment_key(0, dict(g, decoupled_weight_decay=True))


def test_plan_signature_and_plan_inputs_change_when_a_group_flips():
    from rot_mvgaze_amd.optim import Adam
    m = _model()
    head, bb = _split(m)
    ents = _entries(m)
    same = dict(lr=1e-3, weight_decay=1e-2)
    opt = Adam([dict(params=head, **same), dict(params=bb, **same)], capturable="segments")
    sig, inputs = opt.plan_signature(ents), opt.plan_inputs()
    assert len(sig[0]) == 2 and all(len(s) == 7 for s in sig[0])          # coupled: the items plans always had
    opt.param_groups[1]["decoupled_weight_decay"] = True
    flipped = opt.plan_signature(ents)
    assert flipped != sig and opt.plan_inputs() != inputs
    assert [s[:2] for s in flipped[0]] == [s[:2] for s in sig[0]] and flipped[0][0] == sig[0][0] and flipped[0][1] != sig[0][1]
    opt.param_groups[1]["decoupled_weight_decay"] = False
    assert opt.plan_signature(ents) == sig and opt.plan_inputs() == inputs
    # one group, two neighbours: the flag of a second group over a part of the head splits what was one segment
    one = Adam(head + bb, capturable="segments").plan_signature(ents)
    assert len(one[0]) == 1
    two = Adam([dict(params=head[:3]), dict(params=head[3:] + bb, decoupled_weight_decay=True)], capturable="segments")
    assert len(two.plan_signature(ents)[0]) == 2


def test_adamw_defaults_and_per_group_override():
    from rot_mvgaze_amd.optim import Adam, AdamW
    import rot_mvgaze_amd
    assert rot_mvgaze_amd.AdamW is AdamW and issubclass(AdamW, Adam)
    m = _model()
    head, bb = _split(m)
    w = AdamW(m.parameters())
    assert w.defaults["weight_decay"] == 1e-2 and w.defaults["lr"] == 1e-3 and w.defaults["betas"] == (0.9, 0.999)
    assert [g["decoupled_weight_decay"] for g in w.param_groups] == [True] and w.param_groups[0]["weight_decay"] == 1e-2
    a = Adam(m.parameters())
    assert [g["decoupled_weight_decay"] for g in a.param_groups] == [False] and a.param_groups[0]["weight_decay"] == 0.0
    assert Adam(m.parameters(), decoupled_weight_decay=True).param_groups[0]["decoupled_weight_decay"] is True
    # the same keywords as Adam
    w = AdamW([dict(params=bb, decoupled_weight_decay=False, weight_decay=1e-6), dict(params=head)], capturable="segments",
              max_grad_norm=1.0, skip_nonfinite=True)
    assert w.capturable == "segments" and w.max_grad_norm == 1.0 and w.skip_nonfinite is True
    assert [(g["decoupled_weight_decay"], g["weight_decay"]) for g in w.param_groups] == [(False, 1e-6), (True, 1e-2)]
    assert AdamW(m.parameters(), capturable=True).capturable is True
    with pytest.raises(ValueError, match="segments"):
        AdamW(m.parameters(), capturable=True, max_grad_norm=1.0)
    # a group added later takes the optimizer's mode
    w = AdamW(head)
    w.add_param_group({"params": bb, "weight_decay": 0.0})
    assert w.param_groups[1]["decoupled_weight_decay"] is True and w.param_groups[1]["weight_decay"] == 0.0


def test_state_dict_round_trip_keeps_the_flag_per_group_and_an_old_checkpoint_loads_coupled():
    from rot_mvgaze_amd.optim import Adam, AdamW
    m = _model()
    head, bb = _split(m)
    groups = lambda: [dict(params=bb, decoupled_weight_decay=False, weight_decay=1e-6), dict(params=head)]
    sd = AdamW(groups()).state_dict()
    assert [g["decoupled_weight_decay"] for g in sd["param_groups"]] == [False, True]
    other = Adam([dict(params=bb), dict(params=head)])
    assert [g["decoupled_weight_decay"] for g in other.param_groups] == [False, False]
    other.load_state_dict(sd)
    assert [(g["decoupled_weight_decay"], g["weight_decay"]) for g in other.param_groups] == [(False, 1e-6), (True, 1e-2)]
    # a checkpoint written before the key existed
    old = Adam(groups()).state_dict()
    for g in old["param_groups"]:
        del g["decoupled_weight_decay"]
    fresh = AdamW(groups())
    fresh.load_state_dict(old)
    assert [g["decoupled_weight_decay"] for g in fresh.param_groups] == [False, False]
    assert all(Adam._hyper(g)[5] == 0 for g in fresh.param_groups)


@pytest.mark.parametrize("mode", [2, -1, 0.0, 1.0, None, "1"])
def test_the_ex_wrappers_refuse_a_mode_outside_0_and_1_before_any_launch(mode):
    """The arenas are None: a wrapper that got as far as its library call would fail on them in another way."""
    from rot_mvgaze_amd import ops
    host = [(0, 4, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 1), (8, 12, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, mode)]
    with pytest.raises(ValueError, match="adam_step_segments_ex: segment 1 .*mode"):
        ops.adam_step_segments_ex(None, None, None, None, host)
    dev = [(0, 4, 0, 0.9, 0.999, 1e-8, 1e-2, 0), (8, 12, 0, 0.9, 0.999, 1e-8, 1e-2, mode)]
    with pytest.raises(ValueError, match="adam_step_segments_dev_ex: segment 1 .*mode"):
        ops.adam_step_segments_dev_ex(None, None, None, None, dev, None, None)
    with pytest.raises(ValueError, match="needs 9 items"):
        ops.adam_step_segments_ex(None, None, None, None, [host[0][:8]])               # a record without a mode


def test_the_library_exports_and_binds_the_four_entry_points():
    import cabi_header as hdr
    from rot_mvgaze_amd import _lib
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.lib()
    for name, like in (("mvg_adamw_step", "mvg_adam_step"), ("mvg_adamw_step_dev", "mvg_adam_step_dev")):
        assert hasattr(lib, name) and hdr.functions[name] == hdr.functions[like] and _lib.SIGNATURES[name] == _lib.SIGNATURES[like]
    for name, like, extra in (("mvg_adam_step_segments_ex", "mvg_adam_step_segments_clip", 8),
                              ("mvg_adam_step_segments_dev_ex", "mvg_adam_step_segments_dev_clip", 8)):
        assert hasattr(lib, name)
        params, base = list(hdr.functions[name][1]), hdr.functions[like][1]
        assert params.pop(extra) == ("int32_t*", "host_decoupled") and params == base
    assert hdr.constants["MVG_ABI_VERSION"] == _lib.ABI_VERSION == lib.mvg_abi_version() == 13
