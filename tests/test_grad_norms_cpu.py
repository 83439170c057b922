"""CPU-side checks of the per-head gradient-norm diagnostics (simple_tad_amd/grad_norms.py, csrc/grad_segnorm.hip): the segment layout
against the views the reference takes, the model variants without a segment, the host-side plan check, and ``result()``'s arithmetic on
a hand-filled accumulator (single process and world-size-2 gloo).  No kernel is launched here."""
import functools
import os
import socket

import numpy as np
import pytest
import torch

import golden_recipe as R
import simple_tad_amd as T
from simple_tad_amd import grad_norms as GN
from simple_tad_amd._lib import ADAMW_CHUNK, SEGNORM_WORK_MAX, TadError
from simple_tad_amd.flat import FlatSpace


@pytest.fixture(scope="module")
def lib():
    from simple_tad_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def tiny(device="cpu", **kw):
    c = R.TINY
    args = dict(img_size=c["img_size"], patch_size=c["patch_size"], embed_dim=c["embed_dim"], depth=c["depth"], num_heads=c["num_heads"],
                mlp_ratio=4, qkv_bias=True, norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6), all_frames=c["all_frames"],
                tubelet_size=c["tubelet_size"], num_classes=c["num_classes"], init_scale=1.0)
    args.update(kw)
    with torch.device(device):
        return T.VisionTransformer(**args)


def vit_b_meta():
    """ViT-B's patch embedding, blocks and head as the package's own modules on the ``meta`` device: shapes and registration order
    without 345 MB of weights (VisionTransformer's constructor itself reads a value back, which a meta tensor refuses)"""
    m = torch.nn.Module()
    m.num_heads = 12
    with torch.device("meta"):
        m.patch_embed = T.PatchEmbed(img_size=224, patch_size=16, in_chans=3, embed_dim=768, num_frames=16, tubelet_size=2)
        m.blocks = torch.nn.ModuleList([T.Block(dim=768, num_heads=12, mlp_ratio=4, qkv_bias=True, init_values=0.,
                                                norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6)) for _ in range(12)])
        m.fc_norm = torch.nn.LayerNorm(768)
        m.head = torch.nn.Linear(768, 2)
    return m


def space_of(model):
    return FlatSpace([p for p in model.parameters() if p.requires_grad])


def expected_segments(model, space):
    """{(key, index...): (offset, length)} computed from ``space.offset`` and the parameter shapes alone, the way the reference indexes:
    ``qkv.weight.grad.view(3, H, hd, D)[i, h]``, ``q_bias.grad.view(H, -1)[h]``, whole tensors otherwise"""
    H, out = model.num_heads, {}

    def off(p):
        return space.offset[id(p)]

    def ok(p):
        return p is not None and p.requires_grad

    for l, blk in enumerate(model.blocks):
        w = blk.attn.qkv.weight
        if ok(w):
            D = w.shape[1]
            hd = w.shape[0] // 3 // H
            idx = torch.arange(w.numel()).view(3, H, hd, D)
            for h in range(H):
                for i in range(3):
                    sl = idx[i, h].reshape(-1)
                    assert bool((sl[1:] - sl[:-1] == 1).all())              # the slice is one contiguous run
                    out[("qkv", l, h, i)] = (off(w) + int(sl[0]), sl.numel())
        for c, b in ((3, blk.attn.q_bias), (4, blk.attn.v_bias)):
            if ok(b):
                idx = torch.arange(b.numel()).view(H, -1)
                for h in range(H):
                    out[("qkv", l, h, c)] = (off(b) + int(idx[h, 0]), idx.shape[1])
        for c, p in enumerate((blk.attn.proj.weight, blk.attn.proj.bias, blk.mlp.fc1.weight, blk.mlp.fc1.bias, blk.mlp.fc2.weight,
                               blk.mlp.fc2.bias)):
            if ok(p):
                out[("proj", l, c)] = (off(p), p.numel())
    for c, p in enumerate((model.patch_embed.proj.weight, model.patch_embed.proj.bias)):
        if ok(p):
            out[("patch_embed", c)] = (off(p), p.numel())
    return out


def check_layout(model, space):
    lay = GN.segment_table(model, space)
    L, H = len(model.blocks), model.num_heads
    assert lay.shapes == {"qkv": (L, H, 5), "proj": (L, 6), "patch_embed": (2,)}
    # a slot is where the reference's arrays put the entry: the three arrays flattened one behind the other
    flat_index = {}
    for (key, *ix), slot in lay.slots.items():
        base = {"qkv": 0, "proj": L * H * 5, "patch_embed": L * H * 5 + L * 6}[key]
        assert slot == base + int(np.ravel_multi_index(tuple(ix), lay.shapes[key]))
        flat_index[slot] = (key, *ix)
    assert sorted(flat_index) == list(range(L * H * 5 + L * 6 + 2))
    exp = expected_segments(model, space)
    got = {flat_index[s]: (o, n) for o, n, s in lay.segments}
    assert len(got) == len(lay.segments) and got == exp
    # no overlap, and never a padding element: every segment lies inside its parameter's [offset, offset + numel)
    runs = sorted((o, o + n) for o, n, _ in lay.segments)
    assert all(a[1] <= b[0] for a, b in zip(runs, runs[1:]))
    bodies = sorted((space.offset[id(p)], space.offset[id(p)] + p.numel()) for p in space.params)
    for lo, hi in runs:
        assert any(a <= lo and hi <= b for a, b in bodies), (lo, hi)
    assert all(space.offset[id(p)] % ADAMW_CHUNK == 0 for p in space.params)
    return lay


# ------------------------------------------------------------------ segment layout
def test_segments_of_the_tiny_model_are_the_reference_views():
    m = tiny()
    lay = check_layout(m, space_of(m))
    assert len(lay.segments) == 2 * 2 * 5 + 2 * 6 + 2


def test_segments_of_a_vit_b_on_the_meta_device():
    m = vit_b_meta()
    space = space_of(m)
    lay = check_layout(m, space)
    assert len(lay.segments) == 12 * 12 * 5 + 12 * 6 + 2 == 794            # the reference's .norm().item() calls per step
    lengths = sorted({n for _, n, _ in lay.segments})
    assert lengths[0] == 64 and lengths[-1] == 4 * 768 * 768


def test_pretrain_wrapper_and_data_parallel_are_unwrapped():
    from simple_tad_amd import modeling_pretrain as mp
    m = mp.PretrainVisionTransformer(img_size=32, patch_size=16, encoder_embed_dim=128, encoder_depth=2, encoder_num_heads=2,
                                     decoder_num_classes=1536, decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=1, mlp_ratio=4,
                                     qkv_bias=True, norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6), init_values=0., tubelet_size=2)
    assert GN.encoder_of(m) is m.encoder
    space = space_of(m)
    lay = GN.segment_table(m, space)
    exp = expected_segments(m.encoder, space)
    index = {v: k for k, v in lay.slots.items()}
    assert {index[s]: (o, n) for o, n, s in lay.segments} == exp and len(exp) == 2 * 2 * 5 + 2 * 6 + 2


# ------------------------------------------------------------------ model variants
def test_without_qkv_bias_the_bias_slots_have_no_segment():
    m = tiny(qkv_bias=False)
    lay = check_layout(m, space_of(m))
    used = {s for _, _, s in lay.segments}
    for l in range(2):
        for h in range(2):
            assert lay.slots[("qkv", l, h, 3)] not in used and lay.slots[("qkv", l, h, 4)] not in used
            assert all(lay.slots[("qkv", l, h, c)] in used for c in range(3))


def test_frozen_linears_of_block_0_have_no_segment_and_the_rest_is_unchanged():
    """the reference's --freeze_layers path sets requires_grad=False on the frozen blocks' parameters"""
    m = tiny()
    full = GN.segment_table(m, space_of(m))
    for mod in m.blocks[0].modules():
        if isinstance(mod, torch.nn.Linear):
            for p in mod.parameters():
                p.requires_grad = False
    space = space_of(m)
    lay = check_layout(m, space)
    used = {s for _, _, s in lay.segments}
    frozen = {lay.slots[("qkv", 0, h, c)] for h in range(2) for c in range(3)} | {lay.slots[("proj", 0, c)] for c in range(6)}
    assert not (used & frozen)
    assert used == {s for _, _, s in full.segments} - frozen               # q_bias / v_bias of block 0 are Parameters, not Linears: kept
    assert lay.slots == full.slots and lay.shapes == full.shapes


# ------------------------------------------------------------------ plan check
def _tables(segments, n, nslots):
    from simple_tad_amd import kernels as K
    return K.grad_segnorm_tables(segments, n, nslots)


def test_plan_check_accepts_the_generated_plans(lib):
    from simple_tad_amd import kernels as K
    for m in (tiny(), vit_b_meta()):
        space = space_of(m)
        lay = GN.segment_table(m, space)
        table, work = _tables(lay.segments, space.total, len(lay.slots))
        assert table.shape == (len(lay.segments), 3) and work.shape[1] == 2 and table.dtype == work.dtype == torch.int64
        assert int(work[:, 1].max()) <= SEGNORM_WORK_MAX and int(work[:, 1].sum()) == sum(n for _, n, _ in lay.segments)
        assert work.shape[0] == sum(-(-n // SEGNORM_WORK_MAX) for _, n, _ in lay.segments)
        assert lib.tad_grad_segnorm_workspace_bytes(work.shape[0]) == 4 * work.shape[0]
        K.grad_segnorm_plan_check(table, work, space.total, len(lay.slots))


def test_plan_check_rejects_each_violation(lib):
    from simple_tad_amd import kernels as K
    M = SEGNORM_WORK_MAX
    n, nslots = 6 * M, 4
    segs = [(8, 100, 0), (M, 2 * M + 5, 2), (4 * M + 3, M, 3)]
    table, work = _tables(segs, n, nslots)
    assert work.shape[0] == 1 + 3 + 1

    def seg_with(row, **kw):
        t = table.clone()
        rec = t.numpy().view(K._segnorm_dtypes()[0]).reshape(-1)
        for k, v in kw.items():
            rec[k][row] = v
        return t

    def work_with(row, **kw):
        w = work.clone()
        rec = w.numpy().view(K._segnorm_dtypes()[1]).reshape(-1)
        for k, v in kw.items():
            rec[k][row] = v
        return w

    def refused(t, w, what, n=n, nslots=nslots):
        with pytest.raises(TadError, match=what):
            K.grad_segnorm_plan_check(t, w, n, nslots)

    K.grad_segnorm_plan_check(table, work, n, nslots)
    # one fault at a time
    refused(table, work, "not inside the buffer", n=5 * M + 2)                       # the last segment ends behind the buffer
    refused(seg_with(0, offset=-8), work_with(0, offset=-8), "not inside the buffer")   # ... or starts in front of it
    refused(seg_with(0, length=0), work, "must be positive")
    refused(seg_with(0, length=-4), work, "must be positive")
    refused(seg_with(1, slot=4), work, "slot 4 outside")
    refused(seg_with(1, slot=-1), work, "outside")
    refused(seg_with(1, slot=0), work, "has two segments")
    refused(table, work_with(2, offset=2 * M + 1), "exactly once, in order")         # a gap / overlap inside segment 1
    refused(table, work_with(1, length=M - 1), "exactly once, in order")             # the next item then starts one float late
    refused(table, work_with(3, length=6), "ends 1 floats behind")                   # the last item of segment 1 overruns it
    refused(table, work_with(3, length=4), "work list ends|first_work|starts at")     # ... or stops short: the segment is not covered
    refused(table, work_with(0, length=M + 1), "must be in")                         # an item longer than the maximum
    refused(table, work[:-1].contiguous(), "work list ends")                         # an item is missing
    refused(table, torch.cat((work, work[-1:])), "behind the last segment")          # ... or one too many
    refused(seg_with(2, first_work=3), work, "first_work")
    t2 = torch.cat((table[1:2], table[0:1], table[2:]))                               # segments out of the work list's order
    refused(t2, work, "first_work|starts at")
    # a segment longer than the maximum that comes as ONE item
    one = work_with(1, length=2 * M + 5)
    refused(table, torch.cat((one[:2], one[4:])), "must be in")
    with pytest.raises(TadError, match="int64 CPU tensor"):
        K.grad_segnorm_plan_check(table.to(torch.int32), work, n, nslots)


def test_tables_constructor_refuses_what_the_check_refuses(lib):
    with pytest.raises(TadError, match="two segments"):
        _tables([(0, 10, 1), (10, 10, 1)], 100, 2)
    with pytest.raises(TadError, match="not inside the buffer"):
        _tables([(95, 10, 0)], 100, 2)
    with pytest.raises(TadError, match="no segments"):
        _tables([], 100, 2)


# ------------------------------------------------------------------ result() and the arguments
def _cpu_collector(model=None):
    m = model or tiny()
    space = space_of(m)
    space.ensure_grads()
    return m, GN.GradNormCollector(m, space)


def _fill(c, scale=1.0):
    vals = (torch.arange(c.nslots, dtype=torch.float64) + 1.0) * scale
    c.acc.copy_(vals)
    c.counters.copy_(torch.tensor([6, 1, 2], dtype=torch.int32))
    return vals.numpy()


def test_result_divides_the_accumulator_and_keeps_the_reference_keys(lib, tmp_path):
    m, c = _cpu_collector()
    assert c.acc.dtype == torch.float64 and c.last.dtype == torch.float32 and c.counters.dtype == torch.int32
    assert c.acc.numel() == c.last.numel() == 2 * 2 * 5 + 2 * 6 + 2 and c.counters.numel() == 3
    vals = _fill(c)
    r = c.result(6)
    assert list(r) == ["qkv", "proj", "patch_embed"] and isinstance(r, dict)
    assert r["qkv"].shape == (2, 2, 5) and r["proj"].shape == (2, 6) and r["patch_embed"].shape == (2,)
    assert all(v.dtype == np.float64 for v in r.values())
    assert np.array_equal(np.concatenate([r[k].ravel() for k in r]), vals / 6.0)
    assert r["qkv"][1, 0, 3] == ((1 * 2 + 0) * 5 + 3 + 1) / 6.0 and r["proj"][1, 2] == (20 + 6 + 2 + 1) / 6.0 and r["patch_embed"][1] == 34 / 6.0
    assert r.counters == {"steps_added": 6, "steps_skipped": 1, "nonfinite_values": 2}
    np.savez(tmp_path / "gradnorm_ep0.npz", **r)                                    # the reference's run scripts do exactly this
    back = np.load(tmp_path / "gradnorm_ep0.npz")
    assert sorted(back.files) == ["patch_embed", "proj", "qkv"] and np.array_equal(back["qkv"], r["qkv"])
    c.reset()
    z = c.result(3)
    assert all(not v.any() for v in z.values()) and z.counters == {"steps_added": 0, "steps_skipped": 0, "nonfinite_values": 0}


def test_there_is_no_cpu_path_and_no_per_tensor_path(lib):
    m, c = _cpu_collector()
    with pytest.raises(TadError, match="GPU tensor"):
        c.collect()
    plain = tiny()
    opt = torch.optim.AdamW(plain.parameters(), lr=1e-3)
    with pytest.raises(TadError, match="not views of one flat buffer"):
        GN.GradNormCollector(plain, opt)
    for p in plain.parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(TadError, match="not views of one flat buffer"):
        GN.collect_grad_norms(plain)
    with pytest.raises(TadError, match="not views of one flat buffer"):
        GN.collect_grad_norms_pretrain(plain, num_layers=12, num_heads=6)


def test_one_shot_functions_take_and_ignore_the_reference_arguments(lib, monkeypatch):
    """``num_layers`` / ``num_heads`` are accepted and ignored (the reference reads the model); the layout is read off the gradients"""
    import inspect
    for f in (GN.collect_grad_norms, GN.collect_grad_norms_pretrain):
        assert list(inspect.signature(f).parameters) == ["model", "num_layers", "num_heads"]
        assert [p.default for p in inspect.signature(f).parameters.values()][1:] == [12, 6]
    m = tiny()
    space = space_of(m)
    space.ensure_grads()
    seen = []

    def fake_collect(self, coef=None):
        seen.append((self.layout.shapes, coef))
        self.acc.copy_(torch.arange(self.nslots, dtype=torch.float64))

    monkeypatch.setattr(GN.GradNormCollector, "collect", fake_collect)
    a = GN.collect_grad_norms(m)
    b = GN.collect_grad_norms(m, num_layers=7, num_heads=5)
    assert seen == [({"qkv": (2, 2, 5), "proj": (2, 6), "patch_embed": (2,)}, None)] * 2
    assert isinstance(a, tuple) and len(a) == 3 and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert a[0].shape == (2, 2, 5) and a[1].shape == (2, 6) and a[2].shape == (2,) and a[2][1] == 33.0
    # the layout read off the gradients is the flat space's
    assert GN.GradNormCollector(m).layout.segments == GN.segment_table(m, space).segments


def test_engine_without_a_collector_is_unchanged():
    import inspect
    from simple_tad_amd import engine as E, engine_pretrain as EP
    assert inspect.signature(E.train_one_epoch).parameters["grad_norms"].default is None
    assert "grad_norms" not in inspect.signature(EP.train_one_epoch).parameters          # (its parameter list is pinned elsewhere)
    with_gn = list(inspect.signature(EP.train_one_epoch_with_grad_norms).parameters)
    assert with_gn[:7] == ["model", "data_loader", "optimizer", "device", "epoch", "loss_scaler", "grad_norms"]
    assert with_gn[7:] == list(inspect.signature(EP.train_one_epoch).parameters)[6:]
    assert E.NativeScalerWithGradNormCount().last_coef is None
    assert "Left out: the ``gc.collect()" in " ".join(EP.__doc__.split()) and "Left out: the per-head" not in EP.__doc__


# ------------------------------------------------------------------ world size 2 (gloo)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _world2_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from simple_tad_amd.parallel import init_distributed_mode
    ok, r, w, _ = init_distributed_mode(backend="gloo")
    assert ok and r == rank and w == world
    torch.manual_seed(0)
    _, c = _cpu_collector()
    _fill(c, scale=1.0 + rank)          # rank 0: 1, 2, 3 ...; rank 1: 2, 4, 6 ...
    r = c.result(4)
    q.put((rank, {k: v.copy() for k, v in r.items()}, dict(r.counters)))
    dist.barrier()
    dist.destroy_process_group()


def test_result_sums_over_the_ranks_before_it_divides_world2(lib):
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_world2_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
        assert p.exitcode == 0
    expect = 3.0 * (np.arange(34) + 1.0) / 4.0
    for rank, arrays, counters in res:
        assert np.array_equal(np.concatenate([arrays[k].ravel() for k in ("qkv", "proj", "patch_embed")]), expect), rank
        assert counters == {"steps_added": 12, "steps_skipped": 2, "nonfinite_values": 4}
