"""The InternVideo2 family without a GPU: the module is the reference's (keys, shapes, initial values bit for bit -- fixture (a)), the torch
restatement of tests/iv2_recipe.py reproduces the reference's recorded fp64 results (fixtures (b), (c), (d)), the optimizer groups the
family like the reference's optim_factory, and nothing runs off the GPU."""
from collections import OrderedDict
from functools import partial

import pytest
import torch

import iv2_recipe as R
import simple_tad_amd as T
from simple_tad_amd import engine, internvideo2 as IV2
from simple_tad_amd._lib import TadError


@pytest.fixture(scope="module")
def G():
    return R.load()


def build(**over):
    torch.manual_seed(0)
    return IV2.InternVideo2(**dict(R.TINY, **R.REF_ROUTE, **over))


def test_census_keys_shapes_and_initial_values_bit_for_bit(G):
    m = build()
    sd = m.state_dict()
    assert list(sd) == list(G["a/keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(G["a/shapes"])
    bad = [k for k, v, h in zip(sd, sd.values(), G["a/sha256"]) if R.sha(v) != h]
    assert not bad, f"initial values differ from the reference's under torch.manual_seed(0): {bad}"
    assert [k for k, _ in m.named_parameters()] == list(G["a/param_keys"])
    assert sorted(m.no_weight_decay()) == list(G["a/no_weight_decay"])
    assert m.get_num_layers() == int(G["a/num_layers"]) == 2
    # the perturbation the other fixtures start from lands on the same bits too
    R.perturb_(m.named_parameters())
    assert [R.sha(p) for _, p in m.named_parameters()] == list(G["b/sha256"])


@pytest.mark.parametrize("name", list(R.VARIANTS))
def test_census_of_the_variants(G, name):
    m = build(**R.VARIANTS[name])
    assert list(m.state_dict()) == list(G[f"d/{name}/keys"])
    R.perturb_(m.named_parameters())
    assert [R.sha(p) for _, p in m.named_parameters()] == list(G[f"d/{name}/sha256"])


def test_restatement_reproduces_the_model_fixture(G):
    m = build()
    R.perturb_(m.named_parameters())
    P = R.leaves(m.named_parameters(), dtype=torch.float64)
    logits, loss, grads = R.model_loss_and_grads(P, R.clip().double(), R.TINY)
    assert R.matches(logits, G["b/logits"], 0) <= R.REPRO_TOL and abs(float(loss) - float(G["b/loss"])) <= R.REPRO_TOL * float(G["b/loss"])
    worst = {k: R.matches(g, G["b/grad/" + k], i) for i, (k, g) in enumerate(grads.items())}
    print("worst gradient deviation:", max(worst.items(), key=lambda kv: kv[1]))
    assert all(v <= R.REPRO_TOL for v in worst.values()), {k: v for k, v in worst.items() if v > R.REPRO_TOL}
    assert sum(g.numel() > R.WHOLE_MAX for g in grads.values()) >= 10 and sum(g.numel() <= R.WHOLE_MAX for g in grads.values()) >= 10


def test_restatement_reproduces_the_block_fixture(G):
    torch.manual_seed(0)
    blk = IV2.Block(norm_layer=partial(IV2.RMSNorm, eps=1e-6), **R.BLOCK)
    assert [k for k, _ in blk.named_parameters()] == list(G["c/keys"])
    R.perturb_(blk.named_parameters())
    assert [R.sha(p) for _, p in blk.named_parameters()] == list(G["c/sha256"])
    P = R.leaves(blk.named_parameters(), dtype=torch.float64)
    x, dy = (t.double() for t in R.block_input())
    y, dx, grads = R.block_loss_and_grads(P, x, dy)
    assert R.matches(y, G["c/y"], 0) <= R.REPRO_TOL and R.matches(dx, G["c/dx"], 0) <= R.REPRO_TOL
    worst = {k: R.matches(g, G["c/grad/" + k], i) for i, (k, g) in enumerate(grads.items())}
    assert all(v <= R.REPRO_TOL for v in worst.values()), worst


@pytest.mark.parametrize("name", list(R.VARIANTS))
def test_restatement_reproduces_the_variants(G, name):
    over = R.VARIANTS[name]
    m = build(**over)
    R.perturb_(m.named_parameters())
    P = OrderedDict((k, v.detach().double()) for k, v in m.named_parameters())
    with torch.no_grad():
        logits = R.model(P, R.clip().double(), dict(R.TINY, **over))
    assert R.matches(logits, G[f"d/{name}/logits"], 0) <= R.REPRO_TOL
    # (and the variant is not the base model in disguise)
    assert R.matches(logits, G["b/logits"], 0) > 1e-3


def test_a_missing_qk_norm_is_seen_by_the_fixture(G):
    """the recorded logits tell a model without the q / k normalisation from the real one (so the GPU path cannot pass without it)"""
    m = build()
    R.perturb_(m.named_parameters())
    P = OrderedDict((k, v.detach().double()) for k, v in m.named_parameters())
    with torch.no_grad():
        no_norm = R.model(P, R.clip().double(), dict(R.TINY, qk_normalization=False))
    assert R.matches(no_norm, G["b/logits"], 0) > 1e-3


def test_layer_decay_groups_like_the_reference():
    """optim_factory: layer ids patch_embed / cls_token / pos_embed -> 0, blocks.i -> i + 1, everything else -> depth + 1; no decay for
    1-D tensors, biases and no_weight_decay(): 2 * (depth + 2) groups"""
    m = build()
    depth = m.get_num_layers()
    assert [engine.get_num_layer_for_vit(k, depth + 2) for k in ("cls_token", "pos_embed", "patch_embed.proj.weight", "blocks.0.norm1.weight",
                                                                 "blocks.1.attn.q_norm.weight", "clip_projector.norm1_q.weight", "fc_norm.bias",
                                                                 "head.weight")] == [0, 0, 0, 1, 2, 3, 3, 3]
    opt = engine.create_optimizer(m, lr=1e-3, weight_decay=0.05, layer_decay=0.6)
    groups = opt.param_groups
    assert len(groups) == 2 * (depth + 2)
    by_id = {id(p): g for g in groups for p in g["params"]}
    assert len(by_id) == len(list(m.parameters()))
    scale = lambda layer: 0.6 ** (depth + 1 - layer)
    for name, layer, decays in (("cls_token", 0, False), ("pos_embed", 0, False), ("patch_embed.proj.weight", 0, True),
                                ("patch_embed.proj.bias", 0, False), ("blocks.0.attn.qkv.weight", 1, True), ("blocks.0.norm1.weight", 1, False),
                                ("blocks.1.ls1.gamma", 2, False), ("blocks.1.attn.k_norm.weight", 2, False), ("blocks.1.mlp.fc2.weight", 2, True),
                                ("clip_projector.cross_attn.q_bias", 3, False), ("clip_projector.cross_attn.k.weight", 3, True),
                                ("head.weight", 3, True), ("head.bias", 3, False)):
        g = by_id[id(dict(m.named_parameters())[name])]
        assert g["weight_decay"] == (0.05 if decays else 0.0), name
        assert g.get("lr_scale", g["lr"] / 1e-3) == pytest.approx(scale(layer)), name


def test_a_cpu_model_refuses_to_run_and_precise_is_refused():
    m = build()
    with pytest.raises(TadError, match="no CPU fallback"):
        m(R.clip())
    with pytest.raises(TadError, match="no CPU fallback"):
        IV2.RMSNorm(128)(torch.zeros(2, 128))
    T.set_precision("precise")
    try:
        with pytest.raises(TadError, match='"precise" has no route for the InternVideo2 family'):
            m(R.clip())
    finally:
        T.set_precision("fast")


def test_factories_and_the_models_without_a_kernel_construct():
    assert {"internvideo2_small_patch14_224", "internvideo2_base_patch14_224", "internvideo2_large_patch14_224", "internvideo2_1B_patch14_224",
            "internvideo2_6B_patch14_224"} <= set(T.list_models())
    m = T.create_model("internvideo2_small_patch14_224", num_classes=2)
    assert m.pos_embed.shape == (1, 8 * 16 * 16 + 1, 384) and m.get_num_layers() == 12 and m.blocks[0].attn.num_heads == 6
    assert m.clip_projector.cross_attn.num_heads == 16 and m.head.weight.shape == (2, 768)
    assert m.pos_embed.requires_grad and m.cls_token.requires_grad
    with torch.device("meta"):
        big = T.create_model("internvideo2_1B_patch14_224", num_classes=2)
    assert big.get_num_layers() == 40 and big.blocks[0].attn.qkv.weight.shape == (3 * 1408, 1408) and big.blocks[0].mlp.fc1.weight.shape[0] == 6144
    assert big.blocks[0].attn.qkv.weight.shape[0] // (3 * big.blocks[0].attn.num_heads) == 88
    with torch.device("meta"):
        huge = T.create_model("internvideo2_6B_patch14_224", num_classes=2)
    assert huge.get_num_layers() == 48 and huge.embed_dim == 3200 and huge.blocks[0].attn.num_heads == 25
    assert huge.blocks[0].attn.q_norm.weight.shape == (3200,) and huge.pos_embed.shape == (1, 2049, 3200)


@pytest.mark.parametrize("dim,heads,hd", [(176, 2, 88), (256, 2, 128)])
def test_blocks_without_an_attention_kernel_refuse_with_the_head_dim_error(dim, heads, hd):
    """the 1B (head_dim 88) and 6B (head_dim 128) shapes: the refusal is the attention route's, and it comes before anything else -- before
    the device check and before the first norm (whose own limit, D <= 2048, the 6B model also exceeds)"""
    blk = IV2.Block(dim, heads, norm_layer=partial(IV2.RMSNorm, eps=1e-6), qk_normalization=True, init_values=0.1)
    with pytest.raises(TadError, match=f"head_dim {hd} has no kernel"):
        blk(torch.zeros(1, 4, dim))


def test_sincos_tables_are_float32_angles_in_a_float64_table():
    t = IV2.get_3d_sincos_pos_embed(128, 2, 2, cls_token=True)
    assert t.shape == (9, 128) and str(t.dtype) == "float64" and not t[0].any()
    assert t[1, :16].tolist() == [0.0] * 16 and t[1, 16:32].tolist() == [1.0] * 16  # t = 0: sin 0, cos 0
    assert IV2.get_2d_sincos_pos_embed(96, 2).shape == (4, 96) and IV2.get_1d_sincos_pos_embed(32, 2, cls_token=True).shape == (3, 32)
