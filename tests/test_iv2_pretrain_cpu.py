"""InternVideo2 MAE pre-training without a GPU: the module is the reference's (keys, shapes, initial values bit for bit -- fixture (a) of
tests/golden/g27_iv2_pretrain.npz), the torch restatement of tests/iv2_pretrain_recipe.py reproduces the reference's recorded fp64
results (fixtures (b) and (c)), the optimizer groups the model by the reference's full-name rule, nothing runs off the GPU, and
``engine_pretrain.train_one_epoch_double`` joins its two loaders as the reference does."""
import inspect
from collections import OrderedDict
from functools import partial

import pytest
import torch
import torch.nn as nn

import iv2_pretrain_recipe as PR
import iv2_recipe as R
import simple_tad_amd as T
from simple_tad_amd import engine, engine_pretrain as EP, internvideo2_pretrain as IVP
from simple_tad_amd._lib import TadError


@pytest.fixture(scope="module")
def G():
    return PR.load()


def build(**over):
    torch.manual_seed(0)
    return IVP.PretrainVideoMAEInternVideo2(norm_layer=partial(nn.LayerNorm, eps=1e-6), **dict(PR.TINY, **over))


def test_census_keys_shapes_and_initial_values_bit_for_bit(G):
    m = build()
    sd = m.state_dict()
    assert list(sd) == list(G["a/keys"]) and len(sd) == 44
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(G["a/shapes"])
    bad = [k for k, v, h in zip(sd, sd.values(), G["a/sha256"]) if R.sha(v) != h]
    assert not bad, f"initial values differ from the reference's under torch.manual_seed(0): {bad}"
    assert [k for k, _ in m.named_parameters()] == list(G["a/param_keys"])
    assert sum(p.numel() for p in m.parameters()) == int(G["a/num_parameters"]) == 569868
    assert sorted(m.no_weight_decay()) == list(G["a/no_weight_decay"]) == ["cls_token", "mask_token", "pos_embed"]
    assert sorted(m.encoder.no_weight_decay()) == list(G["a/encoder_no_weight_decay"])
    assert sorted(m.decoder.no_weight_decay()) == list(G["a/decoder_no_weight_decay"])
    assert m.encoder.get_num_layers() == int(G["a/encoder_num_layers"]) == 2 and m.decoder.get_num_layers() == int(G["a/decoder_num_layers"]) == 1
    with pytest.raises(AttributeError):
        m.get_num_layers()  # (the reference's outer class asks for self.blocks, which it does not have)
    # the trainable table starts as the 3-D sin-cos table without a class-token row, and the mask token is cut at +-2, not at +-std
    assert m.encoder.pos_embed.requires_grad and m.encoder.pos_embed.shape == (1, PR.N, 128) and not m.encoder.pos_embed[0, 0, :16].any()
    assert m.encoder.pos_embed[0, 0, 16:32].tolist() == [1.0] * 16  # token 0 is t = 0: sin 0 | cos 0 in the temporal quarter, no class-token row
    assert isinstance(m.pos_embed, torch.Tensor) and not isinstance(m.pos_embed, nn.Parameter) and m.pos_embed.shape == (1, PR.N, 64)
    assert float(m.mask_token.detach().abs().max()) > 0.02
    # the perturbation the other fixtures start from lands on the same bits too
    R.perturb_(m.named_parameters())
    assert [R.sha(p) for _, p in m.named_parameters()] == list(G["b/sha256"])


@pytest.mark.parametrize("name", list(PR.VARIANTS))
def test_census_of_the_variants(G, name):
    m = build(**PR.VARIANTS[name])
    assert list(m.state_dict()) == list(G[f"c/{name}/keys"])
    R.perturb_(m.named_parameters())
    assert [R.sha(p) for _, p in m.named_parameters()] == list(G[f"c/{name}/sha256"])


def test_restatement_reproduces_the_model_fixture(G):
    m = build()
    R.perturb_(m.named_parameters())
    P = R.leaves(m.named_parameters(), dtype=torch.float64)
    out, loss, grads = PR.model_loss_and_grads(P, PR.clip().double(), PR.mask(), PR.target().double(), PR.TINY)
    assert tuple(out.shape) == (2, 12, 588)
    assert R.matches(out, G["b/output"], 1000) <= PR.REPRO_TOL and abs(float(loss) - float(G["b/loss"])) <= PR.REPRO_TOL * float(G["b/loss"])
    assert set(grads) == {k[len("b/grad/"):] for k in G.files if k.startswith("b/grad/")} and "encoder.pos_embed" in grads and "mask_token" in grads
    worst = {k: R.matches(g, G["b/grad/" + k], i) for i, (k, g) in enumerate(grads.items())}
    print("worst gradient deviation:", max(worst.items(), key=lambda kv: kv[1]))
    assert all(v <= PR.REPRO_TOL for v in worst.values()), {k: v for k, v in worst.items() if v > PR.REPRO_TOL}
    # the table's gradient is nonzero exactly at the tokens some clip sees: cells 1 and 2 of every frame
    g = grads["encoder.pos_embed"][0].abs().sum(-1).reshape(4, 4)
    assert (g[:, [1, 2]] > 0).all() and not g[:, [0, 3]].any()


@pytest.mark.parametrize("name", list(PR.VARIANTS))
def test_restatement_reproduces_the_variants(G, name):
    over = PR.VARIANTS[name]
    m = build(**over)
    R.perturb_(m.named_parameters())
    P = OrderedDict((k, v.detach().double()) for k, v in m.named_parameters())
    with torch.no_grad():
        out = PR.model(P, PR.clip().double(), PR.mask(), dict(PR.TINY, **over))
    assert R.matches(out, G[f"c/{name}/output"], 1000) <= PR.REPRO_TOL
    assert R.matches(out, G["b/output"], 1000) > 1e-3  # (and the variant is not the base model in disguise)


def test_a_missing_position_table_is_seen_by_the_fixture(G):
    """the recorded output tells a model whose encoder adds no table from the real one (so the GPU path cannot pass without the add)"""
    m = build()
    R.perturb_(m.named_parameters())
    P = OrderedDict((k, v.detach().double()) for k, v in m.named_parameters())
    P["encoder.pos_embed"] = torch.zeros_like(P["encoder.pos_embed"])
    with torch.no_grad():
        out = PR.model(P, PR.clip().double(), PR.mask(), PR.TINY)
    assert R.matches(out, G["b/output"], 1000) > 1e-3


def test_factory_is_registered_and_builds_the_reference_sizes():
    assert "pretrain_videomae_internvideo2_patch14_224" in T.list_models()
    m = T.create_model("pretrain_videomae_internvideo2_patch14_224")
    assert isinstance(m, IVP.PretrainVideoMAEInternVideo2) and isinstance(m.encoder, IVP.iv2_PretrainVisionTransformerEncoder)
    assert m.encoder.pos_embed.shape == (1, 8 * 16 * 16, 384) and m.encoder.get_num_layers() == 12 and m.encoder.blocks[0].attn.num_heads == 6
    assert m.encoder.blocks[0].mlp.fc1.weight.shape == (1536, 384) and not hasattr(m.encoder, "cls_token")
    assert m.encoder.blocks[0].attn.q_norm.weight.shape == (384,) and m.encoder.blocks[0].attn.qkv.bias is None
    assert isinstance(m.encoder.blocks[0].ls1, nn.Identity) and isinstance(m.encoder.head, nn.Identity) and m.encoder.norm.eps == 1e-6
    assert m.decoder.get_num_layers() == 8 and m.decoder.head.weight.shape == (588, 192) and m.encoder_to_decoder.weight.shape == (192, 384)
    assert m.encoder_to_decoder.bias is None and m.mask_token.shape == (1, 1, 192)
    # the route arguments are accepted and select nothing; checkpointing marks the first blocks as internvideo2.Block honours it
    with torch.device("meta"):
        e = IVP.iv2_PretrainVisionTransformerEncoder(embed_dim=128, num_heads=2, depth=3, use_flash_attn=False, use_fused_rmsnorm=False,
                                                     use_fused_mlp=False, fused_mlp_heuristic=2, layerscale_no_force_fp32=True,
                                                     use_checkpoint=True, checkpoint_num=2, sep_pos_embed=True)
    assert [b.with_cp for b in e.blocks] == [True, True, False] and e.pos_embed_spatial.shape == (1, 256, 128) and e.pos_embed_temporal.shape == (1, 8, 128)


def test_constructor_arguments_are_the_references():
    enc = list(inspect.signature(IVP.iv2_PretrainVisionTransformerEncoder.__init__).parameters.items())[1:]
    assert [(k, p.default) for k, p in enc] == [
        ("num_classes", 0), ("qk_scale", None), ("drop_rate", 0.), ("attn_drop_rate", 0.), ("norm_layer", nn.LayerNorm), ("in_chans", 3),
        ("patch_size", 14), ("img_size", 224), ("qkv_bias", False), ("drop_path_rate", 0.25), ("embed_dim", 1408), ("num_heads", 16),
        ("mlp_ratio", 4.3637), ("init_values", 1e-5), ("qk_normalization", True), ("depth", 40), ("use_flash_attn", True),
        ("use_fused_rmsnorm", True), ("use_fused_mlp", True), ("fused_mlp_heuristic", 1), ("layerscale_no_force_fp32", False),
        ("num_frames", 8), ("tubelet_size", 1), ("sep_pos_embed", False), ("use_checkpoint", False), ("checkpoint_num", 0)]
    outer = list(inspect.signature(IVP.PretrainVideoMAEInternVideo2.__init__).parameters.items())[1:]
    assert [(k, p.default) for k, p in outer] == [
        ("img_size", 224), ("patch_size", 14), ("encoder_in_chans", 3), ("encoder_num_classes", 0), ("encoder_embed_dim", 768),
        ("encoder_depth", 12), ("encoder_num_heads", 12), ("decoder_num_classes", 588), ("decoder_embed_dim", 512), ("decoder_depth", 8),
        ("decoder_num_heads", 8), ("mlp_ratio", 4.), ("qkv_bias", False), ("qk_scale", None), ("drop_rate", 0.), ("attn_drop_rate", 0.),
        ("drop_path_rate", 0.), ("norm_layer", nn.LayerNorm), ("init_values", 0.), ("use_learnable_pos_emb", False), ("use_checkpoint", False),
        ("layerscale_no_force_fp32", False), ("num_frames", 8), ("tubelet_size", 1), ("sep_pos_embed", False), ("checkpoint_num", 0),
        ("num_classes", 0), ("in_chans", 0)]


def test_a_cpu_input_is_refused_and_precise_is_refused():
    m = build()
    with pytest.raises(TadError, match="no CPU fallback"):
        m(PR.clip(), PR.mask())
    with pytest.raises(TadError, match="no CPU fallback"):
        m.encoder(PR.clip(), PR.mask())
    T.set_precision("precise")
    try:
        with pytest.raises(TadError, match='"precise" has no route for the InternVideo2 family'):
            m.encoder(PR.clip(), PR.mask())
    finally:
        T.set_precision("fast")
    # a width without an attention kernel refuses with the attention route's error before anything else is looked at
    with torch.device("meta"):
        e = IVP.iv2_PretrainVisionTransformerEncoder(embed_dim=176, num_heads=2, depth=1, img_size=28, num_frames=4)
    with pytest.raises(TadError, match="head_dim 88 has no kernel"):
        e(PR.clip(), PR.mask())


def test_optimizer_groups_by_full_name_like_the_reference():
    """optim_factory.get_parameter_groups tests ``name in skip_list`` on FULL names with the OUTER model's no_weight_decay(): the
    top-level ``mask_token`` is skipped, ``encoder.pos_embed`` is not ('pos_embed' names no parameter of the outer model) and, being
    3-D and no bias, decays"""
    m = build()
    opt = engine.create_optimizer(m, lr=1e-3, weight_decay=0.05)
    by_id = {id(p): g for g in opt.param_groups for p in g["params"]}
    named = dict(m.named_parameters())
    assert len(by_id) == len(named)
    for name, decays in (("encoder.pos_embed", True), ("mask_token", False), ("encoder.patch_embed.proj.weight", True),
                         ("encoder.blocks.0.attn.q_norm.weight", False), ("encoder.blocks.1.mlp.fc2.weight", True), ("encoder.norm.bias", False),
                         ("encoder_to_decoder.weight", True), ("decoder.blocks.0.attn.qkv.weight", True), ("decoder.head.bias", False)):
        assert by_id[id(named[name])]["weight_decay"] == (0.05 if decays else 0.0), name


# ------------------------------------------------------------------------------------------------- train_one_epoch_double
def test_train_one_epoch_double_signature_and_the_pinned_ones():
    names = lambda f: list(inspect.signature(f).parameters)
    single = names(EP.train_one_epoch)
    assert names(EP.train_one_epoch_double) == ["model", "data_loader1", "data_loader2"] + single[2:]
    assert "grad_norms" not in names(EP.train_one_epoch_double)
    d = inspect.signature(EP.train_one_epoch_double).parameters
    assert (d["max_norm"].default, d["patch_size"].default, d["normlize_target"].default, d["start_steps"].default,
            d["tubelet_size"].default) == (0, 16, True, 0, 2)
    assert all(d[k].default is None for k in ("lr_schedule_values", "wd_schedule_values", "log", "augment_fn"))
    assert "always ``None``" in EP.train_one_epoch_double.__doc__


class _Touched(AssertionError):
    pass


def _touched(*a, **k):
    raise _Touched("a kernel path was reached")


class _Model(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(1))

    def forward(self, *a, **k):
        _touched()


def _masks(B, n_masked, N=36):
    m = torch.zeros(B, N, dtype=torch.bool)
    m[:, :n_masked] = True
    return m


def test_double_refuses_unequal_mask_counts_across_the_loaders_before_any_kernel(monkeypatch):
    """each loader's batch is uniform in itself (27 and 26 of 36 tokens); joined they are not, and the step is refused with the counts
    of the JOINED batch before the target kernel, the model or the library is touched"""
    from simple_tad_amd import _lib
    monkeypatch.setattr(_lib, "load", _touched)
    monkeypatch.setattr(EP, "reconstruction_target", _touched)
    clips = torch.zeros(2, 3, 8, 48, 48)
    for m2 in (_masks(1, 26), _masks(1, 26).view(1, 4, 9), _masks(1, 26).double().numpy()):
        with pytest.raises(ValueError, match=r"train_one_epoch_double: .*different numbers of tokens \[27, 27, 26\]"):
            EP.train_one_epoch_double(_Model(), [(clips, _masks(2, 27))], [(clips[:1], m2)], None, torch.device("cpu"), 0, None)
    # equal counts pass the check and reach the target kernel
    with pytest.raises(_Touched):
        EP.train_one_epoch_double(_Model(), [(clips, _masks(2, 27))], [(clips[:1], _masks(1, 27))], None, torch.device("cpu"), 0, None)


def test_double_joins_loader_one_first_and_stops_at_the_shorter_loader(monkeypatch):
    seen = []

    def target(videos, masks, *a, **k):
        seen.append((videos.clone(), masks.clone()))
        _touched()
    # the step is cut short right after the join is observed
    monkeypatch.setattr(EP, "reconstruction_target", target)
    a = torch.arange(2.).reshape(2, 1, 1, 1, 1).expand(2, 3, 8, 48, 48) + 1      # clips 1, 2
    b = torch.arange(1.).reshape(1, 1, 1, 1, 1).expand(1, 3, 8, 48, 48) + 7      # clip 7
    ma, mb = _masks(2, 27), _masks(1, 27).flip(1)
    with pytest.raises(_Touched):
        EP.train_one_epoch_double(_Model(), [(a, ma.view(2, 4, 9))], [(b, mb)] * 3, None, torch.device("cpu"), 0, None)
    videos, masks = seen[0]
    assert videos.shape == (3, 3, 8, 48, 48) and videos[:, 0, 0, 0, 0].tolist() == [1.0, 2.0, 7.0]
    assert masks.dtype == torch.bool and torch.equal(masks, torch.cat([ma, mb]))

    # the step count: a model / target that let every step through, counted by the iterator itself
    steps = list(EP._joined_batches([(a, ma)] * 2, [(b, mb)] * 5, torch.device("cpu")))
    assert len(steps) == 2 and all(v.shape[0] == 3 and m.shape == (3, 36) for v, m in steps)
    steps = list(EP._joined_batches([(a, ma)] * 4, [(b, mb)], torch.device("cpu")))
    assert len(steps) == 1
    # masks from one loader only are refused by name, at the step where it happens, before anything is joined or run
    with pytest.raises(ValueError, match="train_one_epoch_double: step 1: data_loader1 delivers masks and data_loader2 does not"):
        list(EP._joined_batches([(a, ma)] * 2, [(b, mb), (b,)], torch.device("cpu")))
    with pytest.raises(ValueError, match="data_loader2 delivers masks and data_loader1 does not"):
        EP.train_one_epoch_double(_Model(), [(a,)], [(b, mb)], None, torch.device("cpu"), 0, None)
    # batches without masks (an augment_fn draws them) are joined as clips alone
    (only,) = list(EP._joined_batches([(a,)], [(b,)], torch.device("cpu")))
    assert len(only) == 1 and only[0].shape[0] == 3
