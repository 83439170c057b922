"""CPU-side checks of the fused Block variants (layer-scale, proj / MLP dropout): the backward algebra in fp64 against autograd, the
numpy restatement of the dropout mask against the C hash compiled as a host function, the C-ABI surface of the four kernels, and the
dispatch conditions of Block.forward.  No kernel runs here."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import block_variants_recipe as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tad_rowscale_transpose_cast", "tad_rowscale_transpose_cast_f16", "tad_layerscale_grads", "tad_branch_dropout_fwd",
               "tad_branch_dropout_cast", "tad_branch_dropout_cast_f16")


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_branch_backward_algebra_equals_autograd_in_fp64(p):
    """y = res + s[b] gamma[c] keep / (1 - p) (a W^T + bias), one clip dropped by drop path, an injected dropout mask: the formulas the
    kernels implement (gamma folded into the weight operand, dgamma from T = gb^T a and W) give autograd's gradients to 1e-12"""
    g0 = torch.Generator().manual_seed(3)
    B, N, D, Kd = 3, 5, 7, 11
    M = B * N
    a = torch.randn(M, Kd, generator=g0, dtype=torch.float64, requires_grad=True)
    W = torch.randn(D, Kd, generator=g0, dtype=torch.float64, requires_grad=True)
    bias = torch.randn(D, generator=g0, dtype=torch.float64, requires_grad=True)
    gamma = (0.1 + 0.05 * torch.randn(D, generator=g0, dtype=torch.float64)).requires_grad_()
    res = torch.randn(M, D, generator=g0, dtype=torch.float64)
    g = torch.randn(M, D, generator=g0, dtype=torch.float64)
    s = torch.tensor([2.0, 0.0, 2.0], dtype=torch.float64)          # drop path, keep_prob 0.5: the middle clip is dropped
    s_rows = s.repeat_interleave(N)
    keep = V.branch_keep(M, D, p, seed=12345).double() if p > 0 else torch.ones(M, D, dtype=torch.float64)
    if p > 0:
        assert 0 < int(keep.sum()) < M * D
    inv_keep = 1.0 / (1.0 - p)
    y = res + s_rows[:, None] * gamma * keep * inv_keep * (a @ W.t() + bias)
    y.backward(g)
    da, dW, db, dgam = V.branch_grads_by_formula(g, a.detach(), W.detach(), bias.detach(), gamma.detach(), s_rows, keep, inv_keep)
    for name, got, ref in (("da", da, a.grad), ("dW", dW, W.grad), ("dbias", db, bias.grad), ("dgamma", dgam, gamma.grad)):
        err = float((got - ref).abs().max())
        assert err <= 1e-12 * max(1.0, float(ref.abs().max())), (name, err)
    assert float(a.grad[N:2 * N].abs().max()) == 0.0 and float(da[N:2 * N].abs().max()) == 0.0


def _host_hash_program(tmp_path):
    """hash32 and make_drop, cut out of csrc/common.h and compiled as host code into a small stand-alone program"""
    src = open(os.path.join(ROOT, "simple_tad_amd", "csrc", "common.h")).read()
    m = re.search(r"struct Drop \{.*?\n\};\n.*?inline bool make_drop\(.*?\n\}\n", src, flags=re.S)
    assert m, "struct Drop ... make_drop not found in common.h"
    body = "\n".join(ln for ln in m.group(0).splitlines() if "drop_keep" not in ln)
    body = body.replace("__host__ __device__ __forceinline__", "static inline")
    assert "hash32" in body and "__device__" not in body
    prog = ('#include <stdint.h>\n#include <stdio.h>\n#include <stdlib.h>\n' + body + '''
int main(int argc, char** argv) {
  const uint32_t M = (uint32_t)atoi(argv[1]), D = (uint32_t)atoi(argv[2]), seed = (uint32_t)strtoul(argv[3], 0, 10);
  const float p = (float)atof(argv[4]);
  Drop d;
  if (!make_drop(p, seed, &d)) return 2;
  printf("%u %.9g\\n", d.thr, d.inv_keep);
  for (uint32_t m = 0; m < M; ++m)
    for (uint32_t c = 0; c < D; ++c) printf("%u %d\\n", hash32(m, c, d.seed), (int)(hash32(m, c, d.seed) >= d.thr));
  return 0;
}
''')
    from simple_tad_amd import build
    cpp, exe = tmp_path / "hash_host.cpp", tmp_path / "hash_host"
    cpp.write_text(prog)
    subprocess.run([build._hipcc(), "-x", "c++", "-O1", str(cpp), "-o", str(exe)], check=True)
    return str(exe)


def test_numpy_mask_agrees_with_the_c_hash_on_the_host(tmp_path):
    exe = _host_hash_program(tmp_path)
    for M, D, seed, p in ((7, 13, 0, 0.1), (33, 5, 2 ** 31 - 2, 0.5), (4, 260, 0xDEADBEEF, 0.3)):
        out = subprocess.run([exe, str(M), str(D), str(seed), repr(p)], capture_output=True, text=True, check=True).stdout.split("\n")
        thr, inv_keep = out[0].split()
        assert int(thr) == int(float(np.float32(p)) * 4294967296.0)
        assert np.float32(float(inv_keep)) == np.float32(V.inv_keep_f32(p))
        rows = np.array([ln.split() for ln in out[1:] if ln], dtype=np.uint64).reshape(M, D, 2)
        row = np.arange(M, dtype=np.uint64).reshape(M, 1)
        col = np.arange(D, dtype=np.uint64).reshape(1, D)
        assert np.array_equal(rows[..., 0], V.hash32_np(row, col, seed))
        keep = V.branch_keep(M, D, p, seed).numpy()
        assert np.array_equal(rows[..., 1].astype(bool), keep)
        assert abs(keep.mean() - (1 - p)) < 0.15


def test_new_kernels_are_declared_exported_and_bound():
    """fails without the feature: the header declares the four kernels (and the two half twins), the library exports them, _lib binds
    them with signatures, and kernels.py wraps each"""
    from simple_tad_amd import _lib, build, kernels
    hdr = open(os.path.join(ROOT, "include", "tad_mi355x.h")).read()
    lib = ctypes.CDLL(build.build(verbose=False))
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", hdr), f"{s} is not declared in tad_mi355x.h"
        assert hasattr(lib, s), f"{s} is not exported"
        assert s in _lib.SIGNATURES, f"{s} is not bound"
    assert _lib.SIGNATURES["tad_rowscale_transpose_cast_f16"] == _lib.SIGNATURES["tad_rowscale_transpose_cast"]
    assert _lib.SIGNATURES["tad_branch_dropout_cast_f16"] == _lib.SIGNATURES["tad_branch_dropout_cast"]
    for w in ("rowscale_transpose_cast", "layerscale_grads", "branch_dropout_fwd", "branch_dropout_cast"):
        assert callable(getattr(kernels, w))
    # host-side validation runs before any launch
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    L = _lib.load()
    assert L.tad_branch_dropout_fwd(p, p, p, None, None, 1, 1.0, 0, 4, 4, None) == -1 and b"[0, 1)" in L.tad_last_error_string()
    assert L.tad_branch_dropout_cast(p, p, p, 0, 0.1, 0, 4, 4, None) == -1 and b"rows_per_scale" in L.tad_last_error_string()
    assert L.tad_layerscale_grads(p, p, p, None, p, p, None, p, 0, 4, 4, None) == -1 and b"cs" in L.tad_last_error_string()
    assert L.tad_rowscale_transpose_cast(p, None, p, 4, 4, None) == -1


def test_block_dispatch_conditions():
    """which Blocks take ops.BlockVariantFn: layer-scale always, proj / MLP dropout in training only; never with attention dropout in
    training, in the precise mode or with the switch off.  _fusable() keeps its meaning."""
    import simple_tad_amd as T
    from simple_tad_amd import ops
    from simple_tad_amd.modeling_finetune import Block
    mk = lambda **kw: Block(128, 2, qkv_bias=True, **{"init_values": 0.0, **kw})
    assert ops.get_block_variants() is True
    ls, dr, ad, plain = mk(init_values=0.1), mk(drop=0.1), mk(init_values=0.1, attn_drop=0.1), mk()
    for b in (ls, dr, ad, plain):
        b.train()
    assert not ls._fusable() and ls._variant_fusable()
    assert not dr._fusable() and dr._variant_fusable() and dr._branch_dropout() == pytest.approx(0.1)
    assert not ad._fusable() and not ad._variant_fusable()
    assert plain._fusable() and not plain._variant_fusable()
    for b in (ls, dr, ad):
        b.eval()
    assert not ls._fusable() and ls._variant_fusable()
    assert dr._fusable() and not dr._variant_fusable() and dr._branch_dropout() == 0.0   # eval: BlockFn
    assert ad._variant_fusable()                                                          # attention dropout is inactive in eval
    ls.train()
    ops.set_block_variants(False)
    try:
        assert not ls._variant_fusable() and not ops.get_block_variants()
    finally:
        ops.set_block_variants(True)
    T.set_precision("precise")
    try:
        assert not ls._variant_fusable()
    finally:
        T.set_precision("fast")
    assert ls._variant_fusable() and isinstance(ops.block_variant_calls, int)
