"""RandomErasing without a GPU: this package's ``RandomErasing`` against the reference's own (golden G15,
tools/make_goldens_erasing.py) bit for bit on the torch path, ``plan()`` against the reference's changed masks, the host-side
validation of the new C entry points, and the place of ``erase_fn`` in the fine-tune loop."""
import ctypes
import inspect
import math
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import erasing_recipe as ER
import golden_recipe as R
import simple_tad_amd as T
from oracle import vit_oracle as O
from simple_tad_amd import engine as E
from simple_tad_amd._lib import TadError
from simple_tad_amd.random_erasing import RandomErasing
from test_mixup_cpu import _build_tiny

CASES = list(ER.cases())
IDS = [c[0] for c in CASES]


def _nonempty(boxes):
    return [b for b in boxes if b[2] > b[1] and b[4] > b[3] and b[6] > b[5]]


@pytest.mark.parametrize("key,mode,name,seed,shape", CASES, ids=IDS)
def test_cpu_path_reproduces_the_reference_bit_for_bit(golden, key, mode, name, seed, shape):
    """each [T,C,H,W] clip in turn, one continuing stream: the erased bytes, and where the ``random`` stream stands afterwards"""
    g = golden("g15_random_erasing")
    x = ER.clip(key, shape)
    fn = RandomErasing(**ER.erasing_kwargs(mode, name))
    random.seed(seed)
    torch.manual_seed(seed)
    for b in range(shape[0]):
        view = x[b].permute(1, 0, 2, 3)
        assert fn(view) is view
    after = random.random()
    assert np.array_equal(ER.digest(x), g[f"{key}.sha"]) and np.array_equal(ER.sample(x), g[f"{key}.sample"])
    assert after == float(g[f"{key}.next"])
    # the batch form [B,C,T,H,W] on the CPU states the same plan with the same draws
    again = ER.clip(key, shape)
    random.seed(seed)
    torch.manual_seed(seed)
    assert fn(again) is again
    assert random.random() == after and np.array_equal(ER.digest(again), g[f"{key}.sha"])


@pytest.mark.parametrize("key,mode,name,seed,shape", CASES, ids=IDS)
def test_plan_alone_reproduces_the_changed_mask_and_no_case_is_a_no_op(golden, key, mode, name, seed, shape):
    g = golden("g15_random_erasing")
    B, C, Tn, H, W = shape
    fn = RandomErasing(**ER.erasing_kwargs(mode, name))
    random.seed(seed)
    boxes = fn.plan(B, Tn, H, W)
    assert random.random() == float(g[f"{key}.next"])             # the plan consumes exactly the reference's draws
    own = ER.owners(boxes, shape)
    want = ER.unpack_mask(g[f"{key}.mask"], shape)
    assert np.array_equal(own >= 0, want)
    erased = (own >= 0).reshape(B, -1).any(1)
    p = ER.CONFIGS[name]["probability"]
    if 0 < p < 1:
        assert erased.any() and not erased.all(), erased
    assert len(_nonempty(boxes)) >= 1
    first = Tn // fn.num_splits if fn.num_splits > 1 else 0
    assert not want[:, :, :first].any() and (first == 0 or want[:, :, first:].any())      # the num_splits quirk: clean leading frames
    if fn.cube:
        assert all(b[1] == first and b[2] == Tn for b in boxes)
    else:
        assert all(b[2] == b[1] + 1 for b in boxes) and len({(b[0], b[1]) for b in boxes}) == len(boxes)


def test_golden_cases_cover_the_configurations_the_shapes_and_an_overlap():
    names = {c[2] for c in CASES}
    assert names == set(ER.CONFIGS) and {c[1] for c in CASES if c[2] == "p1"} == {"const", "rand", "pixel"}
    shapes = {c[4] for c in CASES}
    assert {s[2] for s in shapes} == {4, 5} and {s[3:] for s in shapes} == {(20, 20), (18, 22)} and all(s[:2] == (4, 3) for s in shapes)
    assert ER.CONFIGS["recipe"] == dict(probability=0.25, max_count=1, num_splits=1, max_area=0.1)
    overlaps = 0
    for key, mode, name, seed, shape in CASES:
        if name != "count2":
            continue
        assert shape[2] % 2 == 1
        random.seed(seed)
        boxes = RandomErasing(**ER.erasing_kwargs(mode, name)).plan(shape[0], *shape[2:])
        cover = np.zeros(shape, dtype=np.int32)
        for s, t0, t1, y0, y1, x0, x1 in boxes:
            cover[s, :, t0:t1, y0:y1, x0:x1] += 1
        overlaps += int((cover > 1).sum())
    assert overlaps > 0          # (the last-box-wins rule is exercised: test 1 holds the values there to the reference's)


def test_last_box_wins_on_the_torch_path():
    x = torch.ones(1, 2, 2, 8, 8)
    fn = RandomErasing(1.0, mode="const")
    seen = []

    def values(per_pixel, rand_color, size, dtype, device):
        seen.append(size)
        return torch.full(size, float(len(seen)), dtype=dtype, device=device)

    import simple_tad_amd.random_erasing as M
    saved = M._get_pixels
    M._get_pixels = values
    try:
        fn._erase_torch(lambda s, t: x[s, :, t], [(0, 0, 2, 1, 5, 1, 5), (0, 1, 2, 3, 7, 3, 7)])
    finally:
        M._get_pixels = saved
    assert seen == [(2, 4, 4)] * 3                                  # one draw per box and frame, in that order
    assert x[0, 0, 0, 1, 1] == 1 and x[0, 0, 1, 1, 1] == 2 and x[0, 0, 1, 4, 4] == 3 and x[0, 0, 1, 6, 6] == 3 and x[0, 0, 0, 6, 6] == 1


def test_constructor_keeps_the_reference_surface_and_the_image_form():
    fn = RandomErasing()
    assert (fn.probability, fn.min_area, fn.max_area, fn.min_count, fn.max_count, fn.num_splits, fn.rand_color, fn.per_pixel, fn.cube,
            fn.device) == (0.5, 0.02, 1 / 3, 1, 1, 0, False, False, True, "cuda")
    assert fn.log_aspect_ratio == (math.log(0.01), math.log(1 / 0.01))
    assert list(inspect.signature(RandomErasing.__init__).parameters)[1:] == [
        "probability", "min_area", "max_area", "min_aspect", "max_aspect", "mode", "min_count", "max_count", "num_splits", "device", "cube"]
    assert RandomErasing(mode="PIXEL").per_pixel and RandomErasing(mode="rand").rand_color and RandomErasing(max_count=3).max_count == 3
    assert T.RandomErasing is RandomErasing and T.random_erasing.RandomErasing is RandomErasing
    img = ER.clip("image", (3, 20, 20))
    was = img.clone()
    random.seed(4)
    boxes = RandomErasing(1.0, mode="pixel").plan(1, 1, 20, 20, image=True)
    random.seed(4)
    torch.manual_seed(4)
    assert RandomErasing(1.0, mode="pixel")(img) is img
    (_, _, _, y0, y1, x0, x1), = boxes
    changed = img != was
    assert changed.any() and changed[:, y0:y1, x0:x1].all() and int(changed.sum()) == 3 * (y1 - y0) * (x1 - x0)


def test_probability_zero_leaves_the_bytes_alone_and_draws_one_number_per_clip():
    x = ER.clip("leave", (3, 3, 2, 8, 8))
    was = x.clone()
    random.seed(7)
    assert RandomErasing(0.0, mode="pixel")(x) is x and torch.equal(x, was)
    after = random.random()
    random.seed(7)
    for _ in range(3):
        random.random()
    assert after == random.random()


def test_uint8_batches_are_refused():
    with pytest.raises(TadError, match="normalised"):
        RandomErasing(1.0, mode="pixel")(R.uint8_for("erase.u8", (2, 4, 8, 8, 3)))
    with pytest.raises(ValueError, match="expected"):
        RandomErasing(1.0)(torch.zeros(4, 4))


# ------------------------------------------------------------------ the fine-tune loop with erase_fn
def test_train_one_epoch_calls_erase_fn_once_per_batch_before_mixup_fn():
    c, tiny = R.G12, R.TINY
    m = _build_tiny("cpu", torch.float64)
    kw = dict(depth=tiny["depth"], num_heads=tiny["num_heads"], tubelet=tiny["tubelet_size"], patch=tiny["patch_size"])

    def oracle_forward(x):           # (the package's modules run HIP kernels only: the fp64 oracle stands in, as in test_mixup_cpu.py)
        P = dict(m.named_parameters())
        return F.linear(O.forward_features(x, P, **kw), P["head.weight"], P["head.bias"])

    m.forward = oracle_forward
    opt = E.create_optimizer(m, lr=c["base_lr"], weight_decay=c["weight_decay"], layer_decay=c["layer_decay"], fused_kernel=False)
    calls = []

    def erase(samples):
        calls.append(("erase", samples.data_ptr()))
        return samples

    def mix(samples, targets):
        calls.append(("mix", samples.data_ptr()))
        return samples, torch.nn.functional.one_hot(targets, R.TINY["num_classes"]).to(samples.dtype)

    def criterion(out, target):
        return torch.sum(-target * torch.log_softmax(out, -1), -1).mean()

    batches = R.g12_batches(torch.float64)[:3]
    E.train_one_epoch(m, criterion, batches, opt, torch.device("cpu"), 0, E.NativeScalerWithGradNormCount(m), erase_fn=erase, mixup_fn=mix)
    assert [k for k, _ in calls] == ["erase", "mix"] * 3
    assert all(calls[2 * i][1] == calls[2 * i + 1][1] for i in range(3))          # the mixer gets what the eraser returned
    p = inspect.signature(E.train_one_epoch).parameters
    assert p["erase_fn"].default is None and list(p)[-2:] == ["erase_fn", "mixup_fn"]


# ------------------------------------------------------------------ host validation of the C entry points
@pytest.fixture(scope="module")
def lib():
    from simple_tad_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _table(rows):
    tab = np.zeros((len(rows), 8), dtype=np.int32)
    for k, row in enumerate(rows):
        tab[k] = row
    return tab


def test_host_validation_of_the_erase_entry_points(lib):
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.tad_last_error_string
    assert lib.tad_erase_clips(None, p, 1, 0, 2, 3, 4, 8, 8, None) == -1 and b"null" in err()
    assert lib.tad_erase_clips(p, None, 1, 0, 2, 3, 4, 8, 8, None) == -1 and b"null" in err()
    assert lib.tad_erase_clips(p, p, 1, 0, 2, 3, 0, 8, 8, None) == -1 and b"T=0" in err()
    assert lib.tad_erase_clips(p, p, 1, 0, 0, 3, 4, 8, 8, None) == -1 and b"B=0" in err()
    assert lib.tad_erase_clips(p, p, 1, 0, 2, 3, 16, 8192, 8192, None) == -1 and b"2^31" in err()
    assert lib.tad_erase_clips(p, p, 0, 0, 2, 3, 4, 8, 8, None) == -1 and b"n_boxes=0" in err()
    assert lib.tad_erase_clips(p, p, 70000, 0, 2, 3, 4, 8, 8, None) == -1 and b"n_boxes=70000" in err()
    assert lib.tad_erase_clips(ctypes.c_void_p(p.value + 2), p, 1, 0, 2, 3, 4, 8, 8, None) == -1 and b"aligned" in err()
    good = (1, 2, 0, 4, 2, 6, 1, 8)
    assert lib.tad_erase_plan_check(_table([good, good]).ctypes.data, 2, 2, 4, 8, 8) == 0
    assert lib.tad_erase_plan_check(p, 0, 2, 4, 8, 8) == 0                                    # an empty table is a valid plan
    assert lib.tad_erase_plan_check(None, 1, 2, 4, 8, 8) == -1 and b"null" in err()
    assert lib.tad_erase_plan_check(_table([good]).ctypes.data, 1, 2, 4, 0, 8) == -1 and b"H=0" in err()
    bad = _table([good, (2, 2, 0, 4, 2, 6, 1, 8)])
    assert lib.tad_erase_plan_check(bad.ctypes.data, 2, 2, 4, 8, 8) == -1 and b"box 1" in err() and b"sample=2" in err()
    bad = _table([(-1, 2, 0, 4, 2, 6, 1, 8)])
    assert lib.tad_erase_plan_check(bad.ctypes.data, 1, 2, 4, 8, 8) == -1 and b"sample=-1" in err()
    bad = _table([(0, 2, 0, 4, 2, 9, 1, 8)])
    assert lib.tad_erase_plan_check(bad.ctypes.data, 1, 2, 4, 8, 8) == -1 and b"outside the clip" in err()
    bad = _table([(0, 2, 0, 5, 2, 6, 1, 8)])
    assert lib.tad_erase_plan_check(bad.ctypes.data, 1, 2, 4, 8, 8) == -1 and b"outside the clip" in err()
    bad = _table([(0, 2, 0, 4, 5, 3, 1, 8)])
    assert lib.tad_erase_plan_check(bad.ctypes.data, 1, 2, 4, 8, 8) == -1 and b"outside the clip" in err()
    bad = _table([(0, 7, 0, 4, 2, 6, 1, 8)])
    assert lib.tad_erase_plan_check(bad.ctypes.data, 1, 2, 4, 8, 8) == -1 and b"mode=7" in err()


def test_box_table_wrapper_checks_on_the_host(lib):
    from simple_tad_amd import kernels as K
    tab = K.erase_box_table([(1, 2, 0, 4, 2, 6, 1, 8), (0, 0, 1, 4, 3, 3, 0, 8)], 2, 4, 8, 8)
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (2, 8) and tab[0].tolist() == [1, 2, 0, 4, 2, 6, 1, 8]
    assert tuple(K.erase_box_table([], 2, 4, 8, 8).shape) == (0, 8)
    with pytest.raises(TadError, match="outside the clip"):
        K.erase_box_table([(0, 2, 0, 5, 0, 8, 0, 8)], 2, 4, 8, 8)
    with pytest.raises(TadError, match="sample=2"):
        K.erase_box_table([(2, 2, 0, 4, 0, 8, 0, 8)], 2, 4, 8, 8)
    with pytest.raises(TadError, match="GPU tensor"):
        K.erase_clips(torch.zeros(2, 3, 4, 8, 8), tab, 0)
