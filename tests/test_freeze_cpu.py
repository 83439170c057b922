"""engine.freeze_layers: the reference's ``--freeze_layers "first N blocks;N"`` rule (run_frame_finetuning.py:465-485) as explicit name
sets, what it returns, the specs it ignores, a DataParallel wrapper, and the optimizer built afterwards.  No GPU: flags only."""
import warnings

import pytest
import torch

import simple_tad_amd as T
from simple_tad_amd import engine

DEPTH = 3


def model(**kw):
    torch.manual_seed(0)
    cfg = dict(img_size=48, patch_size=16, embed_dim=128, depth=DEPTH, num_heads=2, all_frames=4, tubelet_size=2, num_classes=3, mlp_ratio=4,
               qkv_bias=True, init_values=0.1)
    cfg.update(kw)
    return T.VisionTransformer(**cfg)


def frozen_block_names(i):
    """what the rule freezes in block i: the Linear tensors (the qkv Linear carries no ``.bias`` of its own here: q_bias / v_bias stand
    for it), q_bias, v_bias and the two layer scales"""
    lin = [f"blocks.{i}.attn.qkv.weight", f"blocks.{i}.attn.proj.weight", f"blocks.{i}.attn.proj.bias", f"blocks.{i}.mlp.fc1.weight",
           f"blocks.{i}.mlp.fc1.bias", f"blocks.{i}.mlp.fc2.weight", f"blocks.{i}.mlp.fc2.bias"]
    return lin + [f"blocks.{i}.attn.q_bias", f"blocks.{i}.attn.v_bias", f"blocks.{i}.gamma_1", f"blocks.{i}.gamma_2"]


def expected_frozen(n):
    return {"patch_embed.proj.weight", "patch_embed.proj.bias"} | {name for i in range(n) for name in frozen_block_names(i)}


@pytest.mark.parametrize("n", [0, 1, 3])
def test_rule_as_name_sets(n):
    m = model()
    names = [k for k, _ in m.named_parameters()]
    want = expected_frozen(n)
    assert want <= set(names), "the explicit names must exist in the model"
    count = engine.freeze_layers(m, f"first N blocks;{n}")
    frozen = {k for k, p in m.named_parameters() if not p.requires_grad}
    assert frozen == want
    assert count == len(want) == 2 + 11 * n
    trainable = set(names) - frozen
    for i in range(DEPTH):
        for k in ("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"):
            assert f"blocks.{i}.{k}" in trainable
    assert {"fc_norm.weight", "fc_norm.bias", "head.weight", "head.bias"} <= trainable


def test_rule_unfreezes_what_it_calls_trainable():
    """the reference assigns requires_grad = True as well: a second call with a smaller N thaws the blocks above it"""
    m = model()
    engine.freeze_layers(m, "first N blocks;3")
    assert engine.freeze_layers(m, "first N blocks;1") == 2 + 11
    assert {k for k, p in m.named_parameters() if not p.requires_grad} == expected_frozen(1)


def test_count_follows_the_names_that_exist():
    """a model whose qkv Linear is bias-free and has no q_bias / v_bias: the count follows the names that exist"""
    m = model(qkv_bias=False, init_values=0.0)
    assert engine.freeze_layers(m, "first N blocks;2") == 2 + 7 * 2
    assert not any("q_bias" in k or "gamma" in k for k, _ in m.named_parameters())


@pytest.mark.parametrize("spec", ["last N blocks;2", "all", ""])
def test_other_spec_changes_nothing_and_warns_once(spec):
    m = model()
    m.blocks[1].mlp.fc1.weight.requires_grad = False  # (a flag set by hand stays as it is)
    before = {k: p.requires_grad for k, p in m.named_parameters()}
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert engine.freeze_layers(m, spec) == 0
    assert len(w) == 1 and "freeze_layers" in str(w[0].message)
    assert {k: p.requires_grad for k, p in m.named_parameters()} == before


def test_data_parallel_wrapper_is_accepted():
    from simple_tad_amd.parallel import DataParallel
    m = model()
    dp = DataParallel(m)  # world size 1: no process group is needed
    assert engine.freeze_layers(dp, "first N blocks;2") == 2 + 11 * 2
    assert {k for k, p in m.named_parameters() if not p.requires_grad} == expected_frozen(2)
    # frozen BEFORE wrapping (the documented order): the flat layout then holds the trainable parameters only
    m2 = model()
    engine.freeze_layers(m2, "first N blocks;2")
    dp2 = DataParallel(m2)
    assert all((p in dp2.space) == p.requires_grad for p in m2.parameters())


@pytest.mark.parametrize("layer_decay", [None, 0.75])
def test_optimizer_holds_exactly_the_trainable_parameters_in_order(layer_decay):
    m = model()
    engine.freeze_layers(m, "first N blocks;1")
    opt = engine.create_optimizer(m, lr=1e-3, weight_decay=0.05, layer_decay=layer_decay, fused_kernel=False)
    order = {id(p): i for i, (_, p) in enumerate(m.named_parameters())}
    held = [p for g in opt.param_groups for p in g["params"]]
    assert len(held) == len({id(p) for p in held})
    assert {id(p) for p in held} == {id(p) for p in m.parameters() if p.requires_grad}
    assert not any(id(p) in {id(q) for q in held} for k, p in m.named_parameters() if k in expected_frozen(1))
    for g in opt.param_groups:
        idx = [order[id(p)] for p in g["params"]]
        assert idx == sorted(idx), "named_parameters() order within each group"
