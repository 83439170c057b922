"""The case list behind tests/golden/g17_linear_plans.json: which Linear problems, under which tad_linear_tuning settings, the launch plans
of the Linear GEMMs were recorded for.  `python tools/linear_plan_cases.py` prints the counts.

The fixture stores this list next to the recorded plans (tests/test_linear_plan_cpu.py reads it from there), so this module is only needed to
record the fixture again.  The plans in it were NOT produced by the planner they test: they were logged, launch by launch, by the launchers
of the commit before csrc/gemm_plan.hip existed (see the fixture's "note").

An NT problem is [entry, M, N, K, out16, epilogue, residual, res_mod, rowscale, rows_per_scale, colscale_cols] in the GEMM's own terms
(y [M, N] = x [M, K] w^T): `entry` names the C-ABI call that poses it (fwd = tad_linear_fwd, qkv = tad_linear_fwd_qkv, dx = tad_linear_bwd_input,
pe = tad_patch_embed_gemm; only fwd and dx take a split-K workspace), `epilogue` is 0 bias, 1 GELU, 2 residual, 3 GELU backward.
A TN problem is [M, N1, N2, K]: the weight gradient [N1, K] over M rows, with N2 > 0 the pair call's second gradient [N2, K].
"""
EPI_PLAIN, EPI_GELU, EPI_RESIDUAL, EPI_DGELU = 0, 1, 2, 3
# embed dim, MLP dim
MODELS = {"vit_s": (384, 1536), "vit_b": (768, 3072), "vit_l": (1024, 4096), "vit_h": (1280, 5120), "vit_g": (1408, 6144), "mae_decoder": (512, 2048)}
ROWS = [784, 1568, 2 * 1568, 8 * 1568, 32 * 1568, 64 * 1568, 33 * 256 + 37]


def nt_problems():
    out = []
    for D, F in MODELS.values():  # the Linears of a block as the model runs them, and their input gradients
        for M in ROWS:
            out += [["qkv", M, 3 * D, D, 1, EPI_PLAIN, 0, 0, 0, 1, D],
                    ["fwd", M, D, D, 0, EPI_RESIDUAL, 1, 0, 1, 1568, 0],
                    ["fwd", M, F, D, 1, EPI_GELU, 0, 0, 0, 1, 0],
                    ["fwd", M, D, F, 0, EPI_RESIDUAL, 1, 0, 1, 1568, 0],
                    ["dx", M, D, 3 * D, 1, EPI_PLAIN, 0, 0, 0, 1, 0],
                    ["dx", M, D, D, 1, EPI_PLAIN, 0, 0, 0, 1, 0],
                    ["dx", M, D, F, 1, EPI_PLAIN, 0, 0, 0, 1, 0],
                    ["dx", M, F, D, 1, EPI_DGELU, 0, 0, 0, 1, 0]]
    # every epilogue / output type / operand combination that has an entry point
    for N, K in ((768, 768), (3072, 768), (768, 3072), (1024, 4096), (1152, 384)):
        for M in (1568, 8 * 1568, 32 * 1568, 33 * 256 + 37):
            for out16 in (0, 1):
                out += [["fwd", M, N, K, out16, EPI_PLAIN, 0, 0, 0, 1, 0], ["fwd", M, N, K, out16, EPI_GELU, 0, 0, 0, 1, 0],
                        ["fwd", M, N, K, out16, EPI_RESIDUAL, 1, 0, 0, 1, 0], ["fwd", M, N, K, out16, EPI_RESIDUAL, 1, 0, 1, 1568, 0],
                        ["fwd", M, N, K, out16, EPI_RESIDUAL, 1, 0, 1, 196, 0],  # rows_per_scale < 256: the 128 x 128 fallback
                        ["fwd", M, N, K, out16, EPI_RESIDUAL, 0, 0, 0, 1, 0],
                        ["dx", M, N, K, out16, EPI_PLAIN, 0, 0, 0, 1, 0], ["dx", M, N, K, out16, EPI_DGELU, 0, 0, 0, 1, 0]]
                if N % 24 == 0:
                    out += [["qkv", M, N, K, out16, EPI_PLAIN, 0, 0, 0, 1, 0], ["qkv", M, N, K, out16, EPI_PLAIN, 0, 0, 0, 1, N // 3]]
    # the patch embedding (residual row modulo the token count) at /16 (K = 1536) and /14 (K = 1176 padded to 1216)
    for K, ntok in ((1536, 1568), (1216, 2048)):
        for D, _ in list(MODELS.values())[:5]:
            for B in (1, 2, 8, 32):
                out.append(["pe", B * ntok, D, K, 0, EPI_RESIDUAL, 1, ntok, 0, 1, 0])
    out += [["fwd", M, 1024, 1216, 1, EPI_PLAIN, 0, 0, 0, 1, 0] for M in ROWS]
    # taller than the 32-bit operand offsets allow: runs as row ranges (523 776 + 50 176 rows in f32, 524 032 + 49 920 in 16 bits)
    M = 523776 + 50176
    out += [["fwd", M, 1024, 4096, 0, EPI_PLAIN, 0, 0, 0, 1, 0], ["fwd", M, 1024, 4096, 1, EPI_PLAIN, 0, 0, 0, 1, 0],
            ["fwd", M, 1024, 4096, 0, EPI_RESIDUAL, 1, 0, 1, 1568, 0]]
    # a single K-tile: the four-wave kernels' K loop needs two
    for M in ROWS:
        out += [["fwd", M, 768, 64, 1, EPI_PLAIN, 0, 0, 0, 1, 0], ["fwd", M, 768, 64, 1, EPI_GELU, 0, 0, 0, 1, 0], ["dx", M, 768, 64, 0, EPI_DGELU, 0, 0, 0, 1, 0]]
    return out


def nt_settings():
    """the defaults, then every knob moved alone to each of its other legal values, then the forced split-K tail in both forms"""
    s = [{}]
    s += [{"variant": v} for v in (1, 2, 3, 4, 5, 7, 8, 9)]
    s += [{"group_m": 4}, {"group_m": 8}, {"w4_plain": 0}, {"w4_plain": 1024}, {"w4_epilogues": 0}, {"w4_epilogues": 14}, {"persistent": 0},
          {"direct_epilogue": 0}, {"direct_epilogue": 2}, {"split_tail": 0}, {"split_tail": 2}, {"splitk_tail": 0}, {"splitk_tail": 2},
          {"splitk_defer": 0}, {"short_k": 0}, {"tail_192": 0}]
    s += [{"splitk_tail": 2, "split_tail": 2, "splitk_defer": d} for d in (0, 1)]
    return s


def tn_problems():
    out = []
    for D, F in MODELS.values():
        for M in ROWS:
            out += [[M, 3 * D, 0, D], [M, D, 0, D], [M, F, 0, D], [M, D, 0, F], [M, D, 0, 1536], [M, D, 0, 1216],
                    [M, 3 * D, D, D], [M, F, D, D]]  # the pairs: qkv + proj, and an fc1-sized gradient with a proj-sized one
    return out


def tn_settings():
    """[knobs, TAD_GEMM_TN_VARIANT in the environment of the process (None = unset): that one has no tad_linear_tuning key]"""
    return [[{}, None], [{"tn_w4": 0}, None], [{"tn_pair": 0}, None], [{"tn_pdeep": 1}, None], [{}, 1], [{}, 3]]


def dump(out):
    """the case list as lines for tools/linear_plan_check.hip: `S key=value ...` moves knobs away from the defaults for the problems that follow,
    `N M N K out16 epilogue residual res_mod rowscale rows_per_scale colscale_cols` is an NT problem, `T M N1 N2 K` a weight gradient"""
    for knobs in nt_settings():
        out.write("S " + " ".join(f"{k}={v}" for k, v in knobs.items()) + "\n")
        for p in nt_problems():
            out.write("N " + " ".join(str(v) for v in p[1:]) + "\n")
    for knobs, env in tn_settings():
        if env is None:
            out.write("S " + " ".join(f"{k}={v}" for k, v in knobs.items()) + "\n")
            for p in tn_problems():
                out.write("T " + " ".join(str(v) for v in p) + "\n")


if __name__ == "__main__":
    import sys
    if "--dump" in sys.argv:
        dump(sys.stdout)
        sys.exit(0)
    print(len(nt_problems()), "NT problems x", len(nt_settings()), "settings;", len(tn_problems()), "TN problems x", len(tn_settings()), "settings")
