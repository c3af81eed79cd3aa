"""heads.plan_head and heads.layer_launch on the host alone: the family of a FusionHead.forward call and the launch of every
Linear layer, from shapes and knobs (no tensor, no device)."""
import itertools

import pytest

import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import arch
from rot_mvgaze_amd.backbone import Family
from rot_mvgaze_amd.heads import SPLIT_MIN_ROWS, FusionHead, HeadCall, Launch, MlpShape, layer_launch, plan_head, split_serves

VARIANTS = {"default": {}, "share_weights": dict(share_weights=True), "ignore_rotmat": dict(ignore_rotmat=True),
            "encode_rotmat": dict(encode_rotmat=True), "share_feature": dict(share_feature=True)}
LIFTER = {18: MlpShape.of([(512, 1536), (1536, 1536)]), 50: MlpShape.of([(2048, 1536), (1536, 1536)])}


def shapes(depth, variant):
    """(cf, fuser, head) Linear shapes of a variant, from arch.head_dims."""
    fin, widths, hin = arch.head_dims(depth, variant)
    return (arch.backbone_spec(depth).fc_dim, MlpShape.of(list(zip([fin] + widths[:-1], widths))), MlpShape.of([(hin, 512), (512, 2)]))


def plan(depth=18, variant="default", V=2, B=512, I=3, keep_tape=True, training=True, **knobs):
    v = arch.Variant(**VARIANTS[variant])
    cf, fuser, head = shapes(depth, v)
    return plan_head(v, V=V, B=B, num_iter=I, cf=cf, fuser=fuser, head=head, keep_tape=keep_tape, training=training, **knobs)


def test_split_serves_up_to_five_iterations():
    assert [split_serves(i) for i in range(1, 9)] == [True] * 5 + [False] * 3
    assert [FusionHead.split_serves(i) for i in (1, 5, 6, 7)] == [True, True, False, False]


@pytest.mark.parametrize("V,B,family", [(2, 511, Family.FP32), (2, 512, Family.SPLIT), (3, 170, Family.FP32), (3, 171, Family.SPLIT)])
def test_the_row_edge_of_the_split_family(V, B, family):
    c = plan(V=V, B=B)
    assert (c.D, c.rows) == (V * (V - 1), V * (V - 1) * B) and (c.rows >= SPLIT_MIN_ROWS) == (family is Family.SPLIT)
    assert c.family is family and c.mode == {Family.FP32: "fp32", Family.SPLIT: "split"}[family]
    assert c.fused_in == (family is Family.FP32)               # the fp32 Linears then form their input rows themselves


def test_iteration_counts_beyond_the_slot_arena_run_fp32():
    assert plan(I=5).family is Family.SPLIT and plan(I=6).family is Family.FP32 and plan(I=6).fused_in
    assert plan(I=6, mixed=True).family is Family.BF16


@pytest.mark.parametrize("depth", [18, 50])
def test_family_per_variant_and_knob(depth):
    for name in VARIANTS:
        splits = name in ("default", "share_weights", "ignore_rotmat")
        assert plan(depth, name).family is (Family.SPLIT if splits else Family.FP32), name        # encode_rotmat, share_feature: never split
        assert plan(depth, name, split=False).family is Family.FP32
        for split in (True, False):                                                                # BF16 beats split
            c = plan(depth, name, split=split, mixed=True)
            assert c.family is Family.BF16 and c.mode == "mixed" and not c.fused_in


def test_fused_in_rule():
    for name, B, fused_input, mixed in itertools.product(VARIANTS, (3, 512), (True, False), (True, False)):
        c = plan(variant=name, B=B, fused_input=fused_input, mixed=mixed)
        plain = name in ("default", "share_weights", "ignore_rotmat")
        assert c.fused_in == (fused_input and plain and c.family is Family.FP32), (name, B, fused_input, mixed)
    assert plan(B=3).fused_in and not plan(B=3, fused_input=False).fused_in and not plan(B=512).fused_in


def test_reuse_copies_rule():
    for keep, keep_tape, training in itertools.product((True, False), repeat=3):
        c = plan(B=3, mixed=True, keep_infer_copies=keep, keep_tape=keep_tape, training=training)
        assert c.reuse_copies == (keep and not keep_tape and not training)
        assert (c.keep_tape, c.training) == (keep_tape, training)


def test_a_layer_the_split_kernels_cannot_serve_sends_the_call_to_fp32():
    """Unreachable with the supported depths (fuser input 2048 / 3584 wide): a width that is no multiple of 32."""
    v = arch.Variant()
    head = MlpShape.of([(2048, 512), (512, 2)])
    ok = MlpShape.of([(2048, 2048), (2048, 1536)])
    kw = dict(V=2, B=512, num_iter=3, cf=512, keep_tape=True, training=True, fused_input=False)
    assert plan_head(v, fuser=ok, head=head, **kw).family is Family.SPLIT
    for fuser, hd in ((MlpShape.of([(2048, 2040), (2040, 1536)]), head), (MlpShape.of([(2064, 2048), (2048, 1536)]), head),
                      (ok, MlpShape.of([(2048, 520), (520, 2)]))):
        assert plan_head(v, fuser=fuser, head=hd, **kw).family is Family.FP32


def test_the_record_is_frozen():
    c = plan()
    assert isinstance(c, HeadCall) and c.wprep is None
    with pytest.raises(AttributeError):
        c.family = Family.FP32
    with pytest.raises(AttributeError):
        c.wprep = {}
    assert c._replace(wprep={}).wprep == {} and c.wprep is None


def test_padded_shapes():
    _, fuser, _ = shapes(18, arch.Variant(encode_rotmat=True))
    assert fuser.fin == (2057, 2057, 2057) and fuser.fin_p == (2060, 2060, 2060) and fuser.fout_p == (2060, 2060, 1536)
    assert fuser.padded == (True, True, True)
    _, fuser, head = shapes(50, arch.Variant(encode_rotmat=True))
    assert fuser.fin[0] == 3593 and fuser.fin_p[0] == 3596 and fuser.fout_p == (3596, 3596, 1536)
    assert head.fin == (3584, 512) and head.fout_p == (512, 2) and head.padded == (False, False) and head.skinny(1) and not head.skinny(0)


G, F, P, S, Bf, Sp = Launch.GEN, Launch.FP32, Launch.PADDED, Launch.SKINNY, Launch.BF16, Launch.SPLIT
# variant -> call kind -> (fuser layers, head layers); the lifter: (FP32, FP32), (BF16, BF16) on a BF16 call
KINDS = {
    "default": {"fp32": ([G, F], [G, S]), "materialised": ([F, F], [F, S]), "split": ([Sp, Sp], [Sp, S]), "mixed": ([Bf, Bf], [Bf, S])},
    "encode_rotmat": {"fp32": ([P, P, P], [F, S]), "materialised": ([P, P, P], [F, S]), "split": ([P, P, P], [F, S]),
                      "mixed": ([P, P, P], [Bf, S])},          # 2057 -> 2060 / 3593 -> 3596: fp32 on padded copies under BF16 too
    "share_feature": {"fp32": ([F, F, F], [F, S]), "materialised": ([F, F, F], [F, S]), "split": ([F, F, F], [F, S]),
                      "mixed": ([Bf, Bf, Bf], [Bf, S])},
}
KINDS["share_weights"] = KINDS["ignore_rotmat"] = KINDS["default"]
CALLS = {"fp32": dict(B=3), "materialised": dict(B=3, fused_input=False), "split": dict(B=512), "mixed": dict(B=512, mixed=True)}


@pytest.mark.parametrize("depth", [18, 50])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_layer_launch_for_every_variant_and_call(depth, variant):
    _, fuser, head = shapes(depth, arch.Variant(**VARIANTS[variant]))
    for kind, kw in CALLS.items():
        c = plan(depth, variant, **kw)
        want_f, want_h = KINDS[variant][kind]
        assert [layer_launch(c, fuser, l) for l in range(fuser.n)] == want_f, (variant, kind)
        assert [layer_launch(c, head, l) for l in range(head.n)] == want_h, (variant, kind)       # the skinny 512 -> 2 layer: always fp32
        lift = [layer_launch(c, LIFTER[depth], l, lifter=True) for l in range(2)]
        assert lift == ([Bf, Bf] if kind == "mixed" else [F, F]), (variant, kind)
