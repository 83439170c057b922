"""Weight EMA (ema.ModelEma, timm.utils.ModelEma's counterpart) on the CPU: the surface, the host path (``--model_ema_force_cpu``) bit
for bit against the reference's expression, ``module.`` prefixes, checkpoint loading in both forms, the engine's update cadence and
the C ABI's argument checks (no launch)."""
import ctypes
import io
import math

import pytest
import torch
import torch.nn as nn

import simple_tad_amd as T
from simple_tad_amd import checkpoint as CK
from simple_tad_amd import engine as E
from simple_tad_amd.ema import ModelEma


def _small(seed=0):
    torch.manual_seed(seed)
    m = nn.Sequential(nn.Flatten(), nn.Linear(3 * 2 * 4 * 4, 8), nn.LayerNorm(8), nn.Linear(8, 2))
    m[2].weight.requires_grad_(False)  # a frozen parameter: updated like every other entry
    m.register_buffer("counter", torch.tensor(3, dtype=torch.int64))  # a non-f32 buffer
    return m


def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for v in m.state_dict().values():
            if v.is_floating_point():
                v.add_(torch.randn(v.shape, generator=g))


def test_surface_is_an_independent_eval_copy_without_grads():
    m = T.VisionTransformer(img_size=16, patch_size=8, embed_dim=128, depth=2, num_heads=2, qkv_bias=True, all_frames=4, num_classes=2,
                            use_learnable_pos_emb=True)
    m.train()
    e = ModelEma(m, decay=0.99)
    assert e.decay == 0.99 and e.device == '' and e.ema_has_module is False
    assert not e.ema.training and m.training
    assert all(not p.requires_grad for p in e.ema.parameters()) and all(p.requires_grad for p in m.parameters())
    sd, esd = m.state_dict(), e.ema.state_dict()
    assert sd.keys() == esd.keys() and "pos_embed" in esd
    for k in sd:
        assert torch.equal(sd[k], esd[k]) and sd[k].data_ptr() != esd[k].data_ptr(), k
    with torch.no_grad():
        m.head.weight.add_(1.0)
    assert not torch.equal(m.head.weight, e.ema.head.weight)
    assert ModelEma(m, device='cpu').device == 'cpu'


@pytest.mark.parametrize("decay", [0.9999, 0.99, 0.5, 0.0, 1.0])
def test_host_path_is_the_reference_expression_bit_for_bit(decay):
    m = _small()
    e = ModelEma(m, decay=decay, device='cpu')
    for step in range(3):
        _perturb(m, 10 + step)
        want = {k: v.clone() for k, v in e.ema.state_dict().items()}
        msd = m.state_dict()
        for k, v in want.items():  # timm's ModelEma.update
            v.copy_(v * decay + (1. - decay) * msd[k])
        e.update(m)
        for k, v in e.ema.state_dict().items():
            assert v.dtype == want[k].dtype and torch.equal(v, want[k]), (k, decay)
    # the frozen parameter moved with the others (x*d + (1-d)*x != x for some x)
    if 0.0 < decay < 1.0:
        assert not torch.equal(e.ema.state_dict()["2.weight"], _small().state_dict()["2.weight"])


class _Wrapper(nn.Module):  # DataParallel / DDP shape: the model under .module
    def __init__(self, module):
        super().__init__()
        self.module = module


def test_module_prefix_of_a_wrapped_model():
    m = _small()
    plain, wrapped = ModelEma(m, decay=0.9), ModelEma(m, decay=0.9)
    _perturb(m, 5)
    plain.update(m)
    wrapped.update(_Wrapper(m))
    for (k, a), (_, b) in zip(plain.ema.state_dict().items(), wrapped.ema.state_dict().items()):
        assert torch.equal(a, b), k
    # an EMA of the wrapper itself reads the wrapper's keys as they are
    w = ModelEma(_Wrapper(_small()), decay=0.9)
    assert w.ema_has_module
    w.update(_Wrapper(m))
    assert all(k.startswith("module.") for k in w.ema.state_dict())


@pytest.mark.parametrize("form", ["bare", "state_dict_ema"])
def test_checkpoint_loading_accepts_both_forms(form, tmp_path):
    src = ModelEma(_small(1), decay=0.9)
    _perturb(src.ema, 7)
    sd = CK.ema_state_dict(src)
    assert not any(k.startswith("module.") for k in sd)
    obj = sd if form == "bare" else {"state_dict_ema": sd}
    dst = ModelEma(_small(2))
    CK.load_checkpoint_for_ema(dst, obj)
    assert all(torch.equal(v, sd[k]) for k, v in dst.ema.state_dict().items())
    # timm's entry point, from a file object (the reference's BytesIO round trip) and from a path
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    dst2 = ModelEma(_small(3))
    dst2._load_checkpoint(buf)
    assert all(torch.equal(v, sd[k]) for k, v in dst2.ema.state_dict().items())
    torch.save(obj, tmp_path / "ema.pth")
    dst3 = ModelEma(_small(4), resume=str(tmp_path / "ema.pth"))
    assert all(torch.equal(v, sd[k]) for k, v in dst3.ema.state_dict().items())
    assert all(not p.requires_grad for p in dst3.ema.parameters())
    # an EMA of a wrapped model gets the prefix added
    dw = ModelEma(_Wrapper(_small(5)))
    CK.load_checkpoint_for_ema(dw, obj)
    assert all(torch.equal(v, sd[k]) for k, v in CK.ema_state_dict(dw).items())


def test_checkpoint_without_an_ema_state_leaves_the_average_alone():
    e = ModelEma(_small(1))
    before = {k: v.clone() for k, v in e.ema.state_dict().items()}
    e._load_checkpoint({"model": {}, "epoch": 3})
    assert all(torch.equal(v, before[k]) for k, v in e.ema.state_dict().items())


def test_train_one_epoch_updates_the_ema_once_per_optimizer_step():
    torch.manual_seed(0)
    model = nn.Sequential(nn.Flatten(), nn.Linear(3 * 2 * 4 * 4, 2))
    opt = torch.optim.AdamW(model.parameters(), lr=1e-2)
    ema = ModelEma(model, decay=0.5, device='cpu')
    calls = []
    inner = ema.update

    def counting(m):
        calls.append((len(seen), opt.state[model[1].weight]["step"].item()))
        inner(m)
    ema.update = counting
    data = [(torch.randn(4, 3, 2, 4, 4), torch.randint(0, 2, (4,)), None, None) for _ in range(6)]
    seen = []
    E.train_one_epoch(model, nn.CrossEntropyLoss(), data, opt, torch.device("cpu"), 0, E.NativeScalerWithGradNormCount(),
                      update_freq=2, log=lambda e, i, s: seen.append(i), model_ema=ema)
    # once per optimizer step, after it (the optimizer's count already advanced), on the last micro-step of each pair
    assert calls == [(1, 1.0), (3, 2.0), (5, 3.0)]
    assert not torch.equal(ema.ema[1].weight, model[1].weight)


def test_ema_update_argument_checks_without_a_launch():
    from simple_tad_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert "tad_ema_update" in _lib.SIGNATURES and "tad_ema_update" not in _lib.F16_TWINS
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    cases = [((None, 1, p, 1, 0.9, 0.1), b"null"), ((p, 1, None, 1, 0.9, 0.1), b"null"), ((p, 0, p, 1, 0.9, 0.1), b"n_tensors"),
             ((p, -2, p, 1, 0.9, 0.1), b"n_tensors"), ((p, 1, p, 0, 0.9, 0.1), b"n_chunks"), ((p, 1, p, 1, 1.5, 0.1), b"decay"),
             ((p, 1, p, 1, -0.1, 0.1), b"decay"), ((p, 1, p, 1, 0.9, 1.1), b"decay"), ((p, 1, p, 1, math.nan, 0.1), b"decay"),
             ((p, 1, p, 1, 0.9, math.inf), b"decay")]
    for args, what in cases:
        assert lib.tad_ema_update(*args, None) == -1, args
        msg = lib.tad_last_error_string()
        assert b"ema_update" in msg and what in msg, (args, msg)


def test_ema_table_layout():
    """the host table: {ema, model, numel, 0} per pair (a pair misaligned alike split into a scalar head and an aligned body), then
    {tensor, chunk} per 8192 elements"""
    from simple_tad_amd import kernels as K
    import numpy as np
    buf, nt, nc = K.ema_table([(4096, 8192, 20000), (4100, 8196, 2), (4100, 8200, 9000), (4104, 8200, 1)])
    t = buf[:4 * nt].view(nt, 4).numpy()
    c = buf[4 * nt:].numpy().view(np.int32).reshape(nc, 2)
    assert t.tolist() == [[4096, 8192, 20000, 0], [4100, 8196, 2, 0], [4100, 8200, 9000, 0], [4104, 8200, 1, 0]] and nc == 3 + 1 + 2 + 1
    buf, nt, nc = K.ema_table([(4100, 8196, 9000)])
    assert buf[:4 * nt].view(nt, 4).tolist() == [[4100, 8196, 3, 0], [4112, 8208, 8997, 0]] and nc == 3
    assert buf[4 * nt:].numpy().view(np.int32).reshape(nc, 2).tolist() == [[0, 0], [1, 0], [1, 1]]
