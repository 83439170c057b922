"""Exact-integer operands, references and the case table of the Linear GEMM tests (test_linear_exact_cpu.py proves the conditions on the
inputs and, from the planner, the reach of the table; test_linear_exact_gpu.py holds the HIP kernels to the references bit for bit).

The argument.  Operands are small integers (times a power of two), exact in bfloat16 and in IEEE half.  Every product x_k w_k is then an
integer, and as long as  sum_k |x_k| |w_k| + |bias| + |residual| < 2^24  every partial sum, IN ANY ORDER, is an integer below 2^24 and so
exact in f32: tile shape, persistent walk, split-K shares, slab reductions, the pair launch and accumulate mode cannot change a bit, and the
kernel has no rounding to hide behind.  A power-of-two factor (the 2^-s operand scale, a gamma / rowscale out of {0, 1/4, 1/2, 1, 2}) only
moves the binary point: the condition becomes  magnitude / quantum < 2^24  with the quantum the smallest power of two any term is a multiple
of (`admissible`).

A plain helper module: torch on the CPU (the references follow their inputs to whatever device and integer / double type they are given in);
nothing here imports the HIP library."""
import math

import torch

OP16 = {"bf16": torch.bfloat16, "f16": torch.float16}
MANT = {"bf16": 8, "f16": 11}  # significant bits
LIMIT = 1 << 24
BIAS_RANGE = 1000  # integer bias, residual, pos_embed, dW0, db0: uniform in -1000 ... 1000
POW2_SCALES = (0.0, 0.25, 0.5, 1.0, 2.0)  # gamma / rowscale of the exact cases
SMALL = 1 << 32  # M N K up to which the CPU file computes a case's whole output (the long-reduction shapes, 1568 x 768 x 3072, included)

# (range of the first operand, range of the second): x, w of a forward; dy, wT of an input gradient; dy, x of a weight gradient
FAMILIES = {
    "signed": ((-7, 7), (-7, 7)),    # cancelling sums, results of both signs, many zeros; almost all representable in half
    "biased": ((0, 15), (0, 15)),    # large sums, almost none representable in 16 bits
    "wide": ((0, 127), (0, 15)),     # fills ~21 of the 24 accumulator bits at K = 3072
    "wide_b": ((0, 15), (0, 127)),   # the same with the roles swapped
    "low": ((0, 7), (0, 7)),         # weight gradients over tens of thousands of rows
}

# ---- the knob settings of the forward cases
_BASE = dict(persistent=0, direct_epilogue=0, split_tail=0, splitk_tail=0, short_k=0)
# the list of test_linear_persistent_schedule_is_bit_identical (tests/test_kernels_gpu.py) ...
SCHEDULES = [("tile", _BASE), ("tile_direct", dict(_BASE, direct_epilogue=2)), ("persist", dict(_BASE, persistent=1)),
             ("persist_direct", dict(_BASE, persistent=1, direct_epilogue=2)), ("split", dict(_BASE, persistent=1, split_tail=2)),
             ("default_no_splitk", dict(splitk_tail=0)),
             ("w4_tile", dict(_BASE, variant=7)), ("w4_persist", dict(_BASE, variant=7, persistent=1)),
             ("t192", dict(_BASE, variant=8)), ("t192_direct", dict(_BASE, variant=8, direct_epilogue=2)),
             ("short_k", dict(_BASE, short_k=1)), ("t128", dict(_BASE, variant=2)), ("t192_4w", dict(_BASE, variant=9)),
             ("t192_4w_direct", dict(_BASE, variant=9, direct_epilogue=2)),
             # ... plus the split-K tail as the planner takes it on its own, in both forms of the combine
             ("splitk_auto_deferred", dict(splitk_tail=1, splitk_defer=1)), ("splitk_auto_in_launch", dict(splitk_tail=1, splitk_defer=0))]
# the split-K tail forced: the order of summation over K changes, and here that must not matter
SPLITK = [("splitk_deferred", dict(splitk_tail=2, split_tail=2, splitk_defer=1)), ("splitk_in_launch", dict(splitk_tail=2, split_tail=2, splitk_defer=0)),
          ("unsplit", dict(splitk_tail=0))]
SMALL_TILES = [("default", {}), ("t128", dict(_BASE, variant=2)), ("t128x64", dict(_BASE, variant=4)), ("t64", dict(_BASE, variant=5)),
               ("t256x128", dict(_BASE, variant=3)), ("t256", dict(_BASE, variant=1)), ("t192", dict(_BASE, variant=8)), ("t192_4w", dict(_BASE, variant=9)),
               ("w4", dict(_BASE, variant=7))]
DEFAULT = [("default", {})]
TN_KERNELS = [("w4", {}), ("w8", dict(tn_w4=0)), ("pdeep", dict(tn_pdeep=1))]
TN_PAIR = [("pair", {}), ("two_launches", dict(tn_pair=0))]


def _c(id, entry, M, N, K, family, epi="plain", out="f32", knobs=DEFAULT, **kw):
    c = dict(id=id, entry=entry, M=M, N=N, K=K, family=family, epi=epi, out=out, knobs=knobs, bias=True, scale_log2=0, rows_per_scale=1, N2=0,
             accumulate=False)
    c.update(kw)
    return c


# Shapes: the smallest at which the planner still takes the form (test_linear_exact_cpu.py asks it).  392 = 98 x 4 tiles of 256 x 256 are more
# than 1.5 per compute unit: the persistent kernels and the split plan (256 whole tiles + a tail) run.  34 x 8 tiles leave a 16-tile tail that
# splits along K into 4 shares; 66 x 4 tiles with K = 4096 leave the 8-tile tail the planner splits on its own (8 shares).
BIG_M, BIG_N = 25088 + 5, 1024 + 4
CASES = [
    # ---- linear_fwd, f32 output (a): bias / no bias, every schedule, ragged M and N (N off the 8-column store width)
    _c("fwd_big_biased", "fwd", BIG_M, BIG_N, 128, "biased", knobs=SCHEDULES),
    _c("fwd_big_signed_nobias", "fwd", BIG_M, BIG_N, 128, "signed", knobs=SCHEDULES, bias=False),
    _c("fwd_big_k192_wide", "fwd", BIG_M, 1024, 192, "wide", knobs=SCHEDULES),          # odd number of K-tiles
    _c("fwd_big_k768_w4_biased", "fwd", 25088, 1024, 768, "biased"),                     # the four-wave kernel as the planner's own choice
    _c("fwd_long_k_wide", "fwd", 1568, 768, 3072, "wide", knobs=SMALL_TILES),           # the long reduction: ~21 accumulator bits
    _c("fwd_long_k_wide_b", "fwd", 1568, 768, 3072, "wide_b"),
    _c("fwd_long_k_signed", "fwd", 1568, 768, 3072, "signed", knobs=SMALL_TILES),
    _c("fwd_n100_biased", "fwd", 2304, 100, 128, "biased", knobs=SMALL_TILES),           # N = 100
    _c("fwd_n100_k64_biased", "fwd", 2304, 100, 64, "biased"),                           # a single K-tile
    _c("fwd_small_biased", "fwd", 300, 384, 128, "biased", knobs=SMALL_TILES),
    _c("fwd_tiny_wide", "fwd", 16, 128, 1536, "wide"),
    _c("fwd_splitk_biased", "fwd", 33 * 256 + 37, 2048, 512, "biased", knobs=SPLITK),
    _c("fwd_splitk_wide", "fwd", 33 * 256 + 37, 2048, 512, "wide", knobs=SPLITK),
    _c("fwd_splitk_auto_biased", "fwd", 66 * 256, 1024, 4096, "biased", knobs=SCHEDULES[-2:] + DEFAULT),
    # ---- the residual epilogue with power-of-two gamma / rowscale; rows_per_scale below and above the tile height
    _c("res_big_wide", "fwd", BIG_M, BIG_N, 128, "wide", epi="res", knobs=SCHEDULES, rows_per_scale=1568),
    _c("res_big_rps196_biased", "fwd", BIG_M, 1024, 128, "biased", epi="res", knobs=SCHEDULES, rows_per_scale=196),
    _c("res_small_rps7_biased", "fwd", 300, 384, 128, "biased", epi="res", knobs=SMALL_TILES, rows_per_scale=7),
    _c("res_long_k_biased", "fwd", 1568, 768, 3072, "biased", epi="res", knobs=SMALL_TILES, rows_per_scale=392),
    _c("res_splitk_biased", "fwd", 33 * 256 + 37, 2048, 512, "biased", epi="res", knobs=SPLITK, rows_per_scale=1568),
    _c("res_short_k_biased", "fwd", 2500, 768, 256, "biased", epi="res", rows_per_scale=500),   # the short-K plan: 128 x 128 tiles
    # ---- linear_fwd, 16-bit output (b): the exact value rounded once
    _c("fwd16_big_biased", "fwd", BIG_M, BIG_N, 128, "biased", out="16", knobs=SCHEDULES),
    _c("fwd16_big_k192_biased", "fwd", BIG_M, 2300, 192, "biased", out="16", knobs=SCHEDULES),  # the peeled last K-tile falls back
    _c("fwd16_long_k_signed", "fwd", 1568, 768, 3072, "signed", out="16", knobs=SMALL_TILES),
    _c("fwd16_small_biased", "fwd", 300, 384, 128, "biased", out="16", knobs=SMALL_TILES),
    _c("fwd16_splitk_biased", "fwd", 33 * 256 + 37, 2048, 512, "biased", out="16", knobs=SPLITK),
    _c("res16_biased", "fwd", 2500, 768, 128, "biased", epi="res", out="16", knobs=SMALL_TILES[:5], rows_per_scale=500),
    # ---- the GELU epilogue (c): 2^-6 on x and on the bias, so that the pre-activations span the polynomial's active range
    _c("gelu_big_signed", "fwd", 12544 + 77, 3072, 128, "signed", epi="gelu", knobs=SCHEDULES[:-2], scale_log2=6),
    _c("gelu_k768_signed", "fwd", 2500, 768, 768, "signed", epi="gelu", knobs=SMALL_TILES, scale_log2=6),
    # (pre-activations in the thousands, where gelu(x) = x to the bound: sums that 16 bits cannot hold, through the GELU kernels' accumulators)
    _c("gelu_big_wide", "fwd", 12544 + 77, 3072, 128, "wide", epi="gelu", knobs=SCHEDULES[:-2], scale_log2=6),
    _c("gelu_short_k_signed", "fwd", 2500, 768, 256, "signed", epi="gelu", scale_log2=6),       # the short-K plan: 192 x 128 as four waves
    # ---- linear_bwd_input (d): dy [M, N], wT [K, N] -> dx [M, K]; the planner sees the problem (M, K, N)
    _c("dx_big_biased", "bwd_input", BIG_M, 128, BIG_N, "biased", knobs=SCHEDULES, bias=False),
    _c("dx16_big_biased", "bwd_input", BIG_M, 128, BIG_N, "biased", out="16", knobs=SCHEDULES, bias=False),
    _c("dx_long_k_wide", "bwd_input", 1570, 3072, 768, "wide", knobs=SMALL_TILES, bias=False),
    _c("dx_splitk_biased", "bwd_input", 33 * 256 + 37, 512, 2048, "biased", knobs=SPLITK, bias=False),
    _c("dgelu_big_signed", "bwd_input", 12544 + 200, 128, 3072, "signed", epi="dgelu", knobs=SCHEDULES[:-2], bias=False),
    _c("dgelu_big_wide", "bwd_input", 12544 + 200, 128, 3072, "wide", epi="dgelu", knobs=SCHEDULES[:-2], bias=False),
    _c("dgelu16_signed", "bwd_input", 2500, 768, 768, "signed", epi="dgelu", out="16", knobs=SMALL_TILES, bias=False),
    _c("dgelu_short_k_signed", "bwd_input", 2500, 256, 768, "signed", epi="dgelu", bias=False),
    # ---- linear_fwd_qkv (e): N = 3 D; D = 384 puts the q | k boundary inside a 256-column tile
    _c("qkv_big_biased", "qkv", 25088 + 5, 768, 128, "biased", knobs=SCHEDULES[:6]),
    _c("qkv16_big_biased", "qkv", 25088 + 5, 768, 128, "biased", out="16", knobs=SCHEDULES[:6]),
    _c("qkv_d384_wide", "qkv", 20000 + 3, 1152, 384, "wide", knobs=SCHEDULES[:6]),
    _c("qkv16_d384_biased", "qkv", 20000 + 3, 1152, 128, "biased", out="16", knobs=SCHEDULES[:6]),
    _c("qkv_small_signed", "qkv", 300, 384, 128, "signed"),
    # ---- weight gradients (f): dy [M, N], x [M, K] -> dW [N, K], db [N]
    _c("dw_1024_wide", "bwd_weight", 1024, 256, 256, "wide", knobs=TN_KERNELS),                  # one tile, already split over the rows
    _c("dw_1024_wide_acc", "bwd_weight", 1024, 256, 256, "wide", knobs=TN_KERNELS, accumulate=True),
    _c("dw_long_m_low", "bwd_weight", 50176, 256, 256, "low", knobs=TN_KERNELS),                 # the long reduction
    _c("dw_long_m_biased_acc", "bwd_weight", 50176, 256, 256, "biased", accumulate=True),
    _c("dw_ragged_biased", "bwd_weight", 12544 + 70, 768 + 8, 768 - 8, "biased", knobs=TN_KERNELS),
    _c("dw_k384_wide", "bwd_weight", 2000 + 3, 384, 384, "wide", knobs=TN_KERNELS[:2], accumulate=True),  # K on 128-wide tiles
    _c("dw_one_ktile_wide", "bwd_weight", 50, 264, 256, "wide"),                                  # splits = 1, a single reduction tile
    _c("dw_unsplit_wide", "bwd_weight", 256, 2048, 2048, "wide", knobs=TN_KERNELS[:2]),          # splits = 1: 64 tiles of four reduction tiles
    _c("dwqkv_biased", "bwd_weight_qkv", 12544 + 70, 768, 256, "biased", knobs=TN_KERNELS),
    _c("dwqkv_wide_acc", "bwd_weight_qkv", 3000, 1152, 384, "wide", knobs=TN_KERNELS[:2], accumulate=True),
    _c("dwpair_qkv_biased", "bwd_weight_pair", 12544 + 70, 768, 256, "biased", knobs=TN_PAIR, N2=256, qkv=True),
    _c("dwpair_wide_acc", "bwd_weight_pair", 1024, 512, 256, "wide", knobs=TN_PAIR, N2=256 + 8, qkv=False, accumulate=True),
    _c("dwpair_long_m_low", "bwd_weight_pair", 50176, 256, 256, "low", knobs=TN_PAIR, N2=256, qkv=False),
    _c("dwpair_fallback_n1_biased", "bwd_weight_pair", 3000, 768 + 8, 256, "biased", N2=256, qkv=False, accumulate=True),  # N1 off the tile: two launches
    _c("dwpair_fallback_k384_wide", "bwd_weight_pair", 3000, 1152, 384, "wide", N2=384, qkv=True),                          # K on 128-wide tiles: two launches
]
# (g) gamma = 1 + 0.3 z, rowscale out of {0, 1.25}: the derived epilogue bound instead of the bits
NONPOW2_CASES = [
    _c("resg_big_biased", "fwd", BIG_M, BIG_N, 128, "biased", epi="res", knobs=SCHEDULES[:8], rows_per_scale=1568),
    _c("resg_small_rps7_wide", "fwd", 300, 384, 128, "wide", epi="res", knobs=SMALL_TILES, rows_per_scale=7),
    _c("resg_splitk_biased", "fwd", 33 * 256 + 37, 2048, 512, "biased", epi="res", knobs=SPLITK, rows_per_scale=1568),
]
# (h) the patch embedding: tubelet 2, patch 16 (K = 1536), 4 frames of 32 x 32, B = 3
PATCH_EMBED = dict(B=3, C=3, T=4, H=32, W=32, tubelet=2, patch=16, dims=(64, 200), w_range=3)
CASES += [_c(f"patch_embed_d{D}", "patch_embed", 3 * 2 * 4, D, 1536, "pixels", epi="resmod", res_mod=8, w_lo=-3) for D in PATCH_EMBED["dims"]]
# (weights of both signs cancel: 30 % of those sums fit half.  The same with weights 0 ... 3, whose sums do not)
CASES += [_c("patch_embed_d200_w0to3", "patch_embed", 3 * 2 * 4, 200, 1536, "pixels", epi="resmod", res_mod=8, w_lo=0)]
CASE_BY_ID = {c["id"]: c for c in CASES + NONPOW2_CASES}
assert len(CASE_BY_ID) == len(CASES) + len(NONPOW2_CASES)


def small(case):
    return case["M"] * (case["N"] + case["N2"]) * case["K"] <= SMALL


def _seed(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case["id"])) % (1 << 31)


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64)


def operands(case, nonpow2=False):
    """The seeded operands of a case as int64 tensors (f32 for gamma / rowscale), before the 2^-scale_log2 factor:
    fwd / qkv: x [M, K], w [N, K], bias [N] (qkv: its middle third zero) | res: + res [M, N], gamma [N], rowscale [ceil(M / rows_per_scale)]
    bwd_input: dy [M, N], wT [K, N] | dgelu: + h [M, K] f32 (the pre-activation; the caller rounds it to the operand format)
    bwd_weight*: dy [M, N], x [M, K], dW0 [N, K], db0 [N] | pair: + dy2 [M, N2], x2 [M, K], dW02 [N2, K]"""
    g = torch.Generator().manual_seed(_seed(case))
    M, N, K = case["M"], case["N"], case["K"]
    if case["entry"] == "patch_embed":
        return patch_embed_operands(case, g)
    (alo, ahi), (blo, bhi) = FAMILIES[case["family"]]
    o = {}
    if case["entry"] in ("fwd", "qkv"):
        o["x"], o["w"] = _randint(g, alo, ahi, (M, K)), _randint(g, blo, bhi, (N, K))
        o["bias"] = _randint(g, -BIAS_RANGE, BIAS_RANGE, (N,)) if case["bias"] else None
        if case["entry"] == "qkv":
            o["bias"][N // 3:2 * N // 3] = 0
        if case["epi"] == "res":
            o["res"] = _randint(g, -BIAS_RANGE, BIAS_RANGE, (M, N))
            groups = -(-M // case["rows_per_scale"])
            if nonpow2:
                o["gamma"] = (1 + 0.3 * torch.randn(N, generator=g)).float()
                o["rowscale"] = torch.where(torch.rand(groups, generator=g) < 0.25, 0.0, 1.25).float()
                o["rowscale"][-1] = 1.25  # (the last rows are the tail of the split plan: they keep their sum)
            else:
                # (the zeros are few and placed -- two columns, the first row group: a dropped clip, whose rows return the residual -- so that
                #  most outputs still carry their sum)
                sc = torch.tensor(POW2_SCALES[1:])
                o["gamma"] = sc[torch.randint(0, len(sc), (N,), generator=g)]
                o["rowscale"] = sc[torch.randint(0, len(sc), (groups,), generator=g)]
                o["gamma"][3] = o["gamma"][N - 2] = 0.0
            o["rowscale"][0] = 0.0
    elif case["entry"] == "bwd_input":
        o["dy"], o["wT"] = _randint(g, alo, ahi, (M, N)), _randint(g, blo, bhi, (K, N))
        if case["epi"] == "dgelu":
            o["h"] = (2.5 * torch.randn(M, K, generator=g)).float()
    else:
        o["dy"], o["x"] = _randint(g, alo, ahi, (M, N)), _randint(g, blo, bhi, (M, K))
        o["dW0"], o["db0"] = _randint(g, -BIAS_RANGE, BIAS_RANGE, (N, K)), _randint(g, -BIAS_RANGE, BIAS_RANGE, (N,))
        if case["entry"] == "bwd_weight_pair":
            o["dy2"], o["x2"] = _randint(g, alo, ahi, (M, case["N2"])), _randint(g, blo, bhi, (M, K))
            o["dW02"] = _randint(g, -BIAS_RANGE, BIAS_RANGE, (case["N2"], K))
    return o


def patch_embed_operands(case, g=None, binary=False):
    """clip [B, C, T, H, W] of integer pixel levels 0 ... 255 (binary: only 0 and 255, the two levels the uint8 route's u8 / 255 maps to
    integers), w [D, K] in w_lo = -3 ... 3, bias [D], pos [ntok, D]"""
    P = PATCH_EMBED
    g = g or torch.Generator().manual_seed(_seed(case))
    D = case["N"]
    ntok = (P["T"] // P["tubelet"]) * (P["H"] // P["patch"]) * (P["W"] // P["patch"])
    clip = _randint(g, 0, 255, (P["B"], P["C"], P["T"], P["H"], P["W"]))
    if binary:
        clip = (clip >= 128).long() * 255
    return dict(clip=clip, w=_randint(g, case["w_lo"], P["w_range"], (D, case["K"])), bias=_randint(g, -BIAS_RANGE, BIAS_RANGE, (D,)),
                pos=_randint(g, -BIAS_RANGE, BIAS_RANGE, (ntok, D)))


# ---------------------------------------------------------------------------- references: exact, in the integer / double type of their inputs
def ref_linear(x, w, bias=None):
    """y = x w^T + b"""
    y = x @ w.t()
    return y if bias is None else y + bias


def ref_residual(x, w, bias, res, gamma, rowscale, rows_per_scale):
    """res + rs gamma (x w^T + b) in fp64 (the integer part first: exact for power-of-two factors, the fp64 value otherwise);
    returns (y, t = gamma rs (x w^T + b))"""
    s = ref_linear(x, w, bias).double()
    rs = rowscale.double().to(s.device).repeat_interleave(rows_per_scale)[:s.shape[0], None]
    t = (gamma.double().to(s.device) * rs) * s
    return res.double() + t, t


def ref_bwd_input(dy, wT):
    """dx = dy w with wT [K, N] = w^T"""
    return dy @ wT.t()


def ref_bwd_weight(dy, x, dW0=None, db0=None):
    """dW = dy^T x (+ dW0), db = column sums of dy (+ db0)"""
    dW, db = dy.t() @ x, dy.sum(0)
    return (dW if dW0 is None else dW + dW0), (db if db0 is None else db + db0)


def qv_split(db):
    """the q and v thirds of the qkv entry point's bias gradient"""
    n = db.numel() // 3
    return db[:n], db[2 * n:]


def im2col(clip, tubelet, patch):
    from oracle import vit_oracle as O  # the oracle's own token / k order
    return O.im2col_tubelets(clip, tubelet, patch)


def ref_patch_embed(clip, w, bias, pos):
    P = PATCH_EMBED
    cols = im2col(clip, P["tubelet"], P["patch"])  # [B, ntok, K]
    return cols @ w.t() + bias + pos


# ---------------------------------------------------------------------------- the condition, checked
def not_representable(v, fmt):
    """share of the values of a double tensor that the 16-bit format does not hold exactly"""
    v = v.double()
    return float((v.to(torch.float32).to(OP16[fmt]).double() != v).double().mean())


def _abs_mm(a, b):
    return a.abs().double() @ b.abs().double().t()


def admissible(case, rows=None):
    """Sum |x| |w| + |bias| + |residual| per output in integers (fp64 holds them exactly), after the gamma rs factors and the 2^-s scaling:
    asserts max / quantum < 2^24 -- every partial sum in any order is then exact in f32 -- and returns a dict with the share of outputs
    that bf16 / half cannot hold ("bf16", "f16"), the largest magnitude of an output ("max") and of the condition ("bound").
    rows: look only at these rows of x / dy of a forward / input gradient (the large cases on a machine without a GPU); the worst case over ALL
    outputs, K max|x| max|w| + ..., which needs no look at the operands, is then asserted as well."""
    o = operands(case)
    e, s = case["entry"], 2.0 ** -case["scale_log2"]
    quantum, factor = s, 1.0
    if e == "patch_embed":
        cols = im2col(o["clip"], PATCH_EMBED["tubelet"], PATCH_EMBED["patch"]).reshape(-1, case["K"])
        mag = _abs_mm(cols, o["w"]) + o["bias"].abs() + o["pos"].abs().repeat(PATCH_EMBED["B"], 1)
        val = [ref_patch_embed(o["clip"], o["w"], o["bias"], o["pos"])]
        worst = case["K"] * 255 * PATCH_EMBED["w_range"] + 2 * BIAS_RANGE
    elif e in ("fwd", "qkv", "bwd_input"):
        a, b = (o["x"], o["w"]) if e != "bwd_input" else (o["dy"], o["wT"])
        red = a.shape[1]
        sel = slice(None) if rows is None else rows
        a = a[sel]
        mag, y = _abs_mm(a, b), ref_linear(a.double(), b.double())
        if o.get("bias") is not None:
            mag, y = mag + o["bias"].abs(), y + o["bias"]
        worst = red * max(abs(v) for v in FAMILIES[case["family"]][0]) * max(abs(v) for v in FAMILIES[case["family"]][1]) + (BIAS_RANGE if case["bias"] else 0)
        if case["epi"] == "res":
            rs = o["rowscale"].double().repeat_interleave(case["rows_per_scale"])[:case["M"], None][sel]
            f = o["gamma"].double() * rs
            mag, y = mag * f + o["res"][sel].abs(), y * f + o["res"][sel]
            factor, quantum = max(POW2_SCALES) ** 2, quantum * min(v for v in POW2_SCALES if v) ** 2
            worst = worst * factor + BIAS_RANGE
        if e == "qkv":  # q_prescale = 1/8 on the first third
            quantum /= 8
        val = [y * s]
        mag = mag * s
        worst *= s
    else:
        mag = _abs_mm(o["dy"].t(), o["x"].t())
        dW, db = ref_bwd_weight(o["dy"].double(), o["x"].double(), *((o["dW0"].double(), o["db0"].double()) if case["accumulate"] else ()))
        val = [dW, db]
        magb = o["dy"].abs().sum(0).double()
        if case["accumulate"]:
            mag, magb = mag + o["dW0"].abs(), magb + o["db0"].abs()
        mag = torch.cat([mag.flatten(), magb])
        (alo, ahi), (blo, bhi) = FAMILIES[case["family"]]
        worst = case["M"] * max(abs(alo), abs(ahi)) * max(abs(blo), abs(bhi), 1) + (BIAS_RANGE if case["accumulate"] else 0)
        if e == "bwd_weight_pair":
            mag2 = _abs_mm(o["dy2"].t(), o["x2"].t()) + (o["dW02"].abs() if case["accumulate"] else 0)
            mag = torch.cat([mag, mag2.flatten()])
            val.append(ref_bwd_weight(o["dy2"].double(), o["x2"].double(), o["dW02"].double() if case["accumulate"] else None)[0])
    bound = float(mag.max()) / quantum
    assert bound < LIMIT, f"{case['id']}: sum |x||w| + |bias| + |residual| reaches {bound:.0f} quanta >= 2^24"
    if rows is not None:  # only some rows were looked at: the bound that needs no look at the operands must hold for the rest
        assert worst / quantum < LIMIT, f"{case['id']}: the worst case over all outputs, {worst / quantum:.0f} quanta, is not below 2^24"
    v = torch.cat([t.flatten().double() for t in val])
    return {"bf16": not_representable(v, "bf16"), "f16": not_representable(v, "f16"), "max": float(v.abs().max()), "bound": bound}


def sample_rows(case, n=192):
    """rows for `admissible` of a large case: the first and last rows and a seeded sample"""
    M = case["M"]
    g = torch.Generator().manual_seed(_seed(case) + 1)
    return torch.unique(torch.cat([torch.arange(min(8, M)), torch.arange(max(0, M - 8), M), torch.randint(0, M, (n,), generator=g)]))


# ---------------------------------------------------------------------------- the planner's view of a case
EPI_CODE = {"plain": 0, "gelu": 1, "res": 2, "dgelu": 3, "resmod": 2}


def nt_problem(case):
    """(M, N, K, keyword arguments) of kernels.linear_plan for a forward / input-gradient / qkv / patch-embedding case"""
    M, N, K = (case["M"], case["N"], case["K"]) if case["entry"] != "bwd_input" else (case["M"], case["K"], case["N"])
    kw = dict(epilogue=EPI_CODE[case["epi"]], out_16bit=case["out"] == "16", residual=case["epi"] in ("res", "resmod"),
              res_mod=case.get("res_mod", 0), rowscale=case["epi"] == "res", rows_per_scale=case["rows_per_scale"],
              colscale_cols=N // 3 if case["entry"] == "qkv" else 0)
    return M, N, K, kw


def ulp16(v, fmt):
    """the spacing of the 16-bit format at |v| (double tensor in and out; half: its subnormal spacing below 2^-14)"""
    _, e = torch.frexp(v.abs().double().clamp_min(1e-300))
    u = torch.exp2((e - MANT[fmt]).double())
    return u.clamp_min(2.0 ** -24) if fmt == "f16" else u


def first_mismatch(got, ref):
    """'(row, column): got, reference, difference' of the first element that differs -- a difference equal to one operand product points at a
    dropped or doubled term, a multiple of the 16-bit spacing at a narrow intermediate"""
    bad = (got != ref).flatten().nonzero()
    if bad.numel() == 0:
        return "equal"
    i = int(bad[0])
    cols = ref.shape[-1] if ref.dim() > 1 else 1
    g, r = float(got.flatten()[i]), float(ref.flatten()[i])
    return f"{int(bad.numel())} of {ref.numel()} differ, first at ({i // cols}, {i % cols}): got {g!r}, reference {r!r}, difference {g - r!r}"


assert math.log2(LIMIT) == 24
