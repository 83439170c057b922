"""Build libtad_mi355x.so, libtad_mi355x_serve.so, libtad_mi355x_recon.so, libtad_mi355x_bank.so and libtad_mi355x_yuv.so (gfx950) in-tree with hipcc.  `python -m simple_tad_amd.build [--force]`."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
# TAD_BUILD_LIB / TAD_BUILD_DEFINES: experiment builds next to the production library (own object directory), e.g.
#   TAD_BUILD_LIB=libtad_spread.so TAD_BUILD_DEFINES="-DTAD_DMA_SPREAD=1" python -m simple_tad_amd.build --force   -> build_exp/libtad_spread.so
# and TAD_LIB=<path> selects the library a process loads (_lib.py).
# TAD_BUILD_ABLATION=1 (the diagnostic build: -DTAD_GEMM_ABLATION, in-kernel stamps / clock readings / debug knobs) never writes the production
# library: without TAD_BUILD_LIB it builds build_exp/libtad_ablation.so in its own object directory.
_ABLATION = os.environ.get("TAD_BUILD_ABLATION") == "1"
_LIB_NAME = os.environ.get("TAD_BUILD_LIB", "libtad_ablation.so" if _ABLATION else "libtad_mi355x.so")
# The production library and the serving, reconstruction, stream-bank and YUV-ingest libraries beside it (SERVE_LIB, RECON_LIB, BANK_LIB, YUV_LIB below) are the ONLY built files in the package directory; every experiment / ablation build (and its objects) goes to
# <repo>/build_exp/ -- git-ignored like every built artefact, but not gpurun-ignored, so it travels to the GPU box with the snapshot.
EXP_DIR = os.path.join(os.path.dirname(HERE), "build_exp")
_PRODUCTION = _LIB_NAME == "libtad_mi355x.so"
LIB = os.path.join(HERE if _PRODUCTION else EXP_DIR, os.path.basename(_LIB_NAME))
SOURCES = ["capi.hip", "elementwise.hip", "patch_embed.hip", "layernorm.hip", "gemm.hip", "gemm_plan.hip", "gemm_w4.hip", "attn_fwd.hip", "attn_bwd.hip", "attn_plan.hip", "attn_f32.hip", "precise.hip", "optim.hip", "ema.hip", "mixup.hip", "frame_loss.hip", "erasing.hip", "randaug.hip", "multiscale_crop.hip", "frame_resize.hip", "spatial_sample.hip", "mae.hip", "metrics.hip", "group_metrics.hip", "grad_segnorm.hip", "collective.hip", "im2col.hip", "pooled_tail.hip", "layerscale.hip", "attn_colsum.hip", "rmsnorm.hip", "visible_tokens.hip"]
# Sources that touch 16-bit GEMM / attention operands are compiled a second time with -DTAD_OPND_F16: the same kernels for IEEE half
# operands, exported as tad_*_f16 (csrc/common.h, csrc/opnd_f16_names.h; include/tad_mi355x.h "IEEE half operand twins").
F16_SOURCES = ["elementwise.hip", "patch_embed.hip", "layernorm.hip", "gemm.hip", "gemm_w4.hip", "attn_fwd.hip", "attn_bwd.hip", "optim.hip", "pooled_tail.hip", "layerscale.hip"]
# gemm_w4.hip (four waves of 128 x 128 outputs: 256 accumulator registers per lane) needs its accumulators in the AGPR half of the register
# file: compiled without the vgpr-form switch below.  It shares the kernel templates of gemm_kernels.h with gemm.hip.
NO_VGPR_FORM = {"gemm_w4.hip"}
# gemm_plan.hip and attn_plan.hip (the launch planners: host code, nothing in them depends on the operand format) are compiled once, not per format;
# so are im2col.hip (the output format is a template argument there: it defines tad_im2col_tubelets / _u8 and their _f16 twins itself)
# and attn_colsum.hip (the operand format is a template argument; one entry point takes it at run time); rmsnorm.hip (the extension ABI,
# include/tad_mi355x_ext.h) takes every 16-bit format at run time; visible_tokens.hip (the pre-training ABI, include/tad_mi355x_pretrain.h)
# is f32 only
EXTRA_DEPS = {"gemm.hip": ["gemm_kernels.h", "gemm_plan.h"], "gemm_w4.hip": ["gemm_kernels.h", "gemm_plan.h"], "gemm_plan.hip": ["gemm_plan.h", "knob.h"],
              "attn_fwd.hip": ["attn_plan.h"], "attn_bwd.hip": ["attn_plan.h"], "attn_plan.hip": ["attn_plan.h", "knob.h"],
              "multiscale_crop.hip": ["frame_io.h"], "frame_resize.hip": ["frame_io.h", "cubic_resize.h"], "spatial_sample.hip": ["frame_io.h"], "randaug.hip": ["frame_io.h"],
              "layernorm.hip": ["rownorm.h"], "rmsnorm.hip": ["rownorm.h", "../../include/tad_mi355x_ext.h"],
              "visible_tokens.hip": ["../../include/tad_mi355x_pretrain.h"]}
# ema.hip and mixup.hip must round like torch (a product, a product, a sum: three roundings) and are compiled without FMA contraction;
# randaug.hip must round like PIL's C code (a float blend, a double affine map and cubic: each product and sum on its own).
# multiscale_crop.hip writes the same normalised f32 values as randaug.hip's frames_to_clip and takes the same flags.
# spatial_sample.hip must round its bilinear blend like the arithmetic include/tad_mi355x.h states (every product and sum on its own).
# frame_resize.hip fades a reflected pad band with one f32 product rounded on its own (cv2.addWeighted) and writes frames_to_clip's f32 values.
# A `#pragma clang fp contract(off)` is not enough: -ffp-contract=fast also lets the code generator fuse fmul + fadd by itself.
NO_FP_CONTRACT = {"ema.hip", "mixup.hip", "randaug.hip", "multiscale_crop.hip", "spatial_sample.hip", "frame_resize.hip"}
# The libraries beside the first one, one per surface added since libtad_mi355x.so was held at its three (include/tad_mi355x_serve.h
# tads_*, _recon.h tadr_*, _bank.h tadb_*, _yuv.h tady_*): each linked apart from ONE source, with the same FLAGS plus hidden visibility
# (its entry points alone are exported: nothing in it can bind to or shadow another library's C++ symbols; csrc/side_library.h).  Built
# after the first library by build(); experiment and ablation builds do not build them.  _SIDE: name -> (source, the headers it
# includes beside side_library.h and its own ABI header); SIDE_LIBS: name -> (library, source list)
_SIDE = {"serve": ("iv2_serve.hip", ["rownorm.h"]), "recon": ("mae_reconstruct.hip", []),
         "bank": ("stream_bank.hip", ["frame_io.h", "cubic_resize.h"]), "yuv": ("yuv_ingest.hip", ["frame_io.h", "cubic_resize.h"])}
SIDE_LIBS = {name: (os.path.join(HERE, f"libtad_mi355x_{name}.so"), [src]) for name, (src, _) in _SIDE.items()}
for _name, (_src, _deps) in _SIDE.items():
    EXTRA_DEPS[_src] = [*_deps, "side_library.h", f"../../include/tad_mi355x_{_name}.h"]
(SERVE_LIB, SERVE_SOURCES), (RECON_LIB, RECON_SOURCES), (BANK_LIB, BANK_SOURCES), (YUV_LIB, YUV_SOURCES) = SIDE_LIBS.values()
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-Wno-unused-result",
         # keep MFMA accumulators in the (unified) VGPR file: without it the compiler parks them in AGPRs and pays a
         # v_accvgpr_read/write per element around every softmax / epilogue
         "-mllvm", "-amdgpu-mfma-vgpr-form=1"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def _deps_mtime():
    m = 0.0
    for root in (CSRC, os.path.join(os.path.dirname(HERE), "include")):
        for f in os.listdir(root):
            m = max(m, os.path.getmtime(os.path.join(root, f)))
    return m


def build(force: bool = False, verbose: bool = True) -> str:
    """build what is stale: the library (returned) and, in a production build, the serving, reconstruction, stream-bank and YUV-ingest libraries beside it"""
    lib = _build_core(force, verbose)
    if _PRODUCTION:
        for side, sources in SIDE_LIBS.values():
            _build_side(side, sources, force, verbose)
    return lib


def _build_side(lib: str, sources, force: bool, verbose: bool) -> str:
    """a self-contained library beside the first one: its own source list, FLAGS plus hidden visibility"""
    if not force and os.path.exists(lib) and os.path.getmtime(lib) >= _deps_mtime():
        return lib
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    hipcc = _hipcc()
    headers = [os.path.join(CSRC, "common.h"), os.path.join(os.path.dirname(HERE), "include", "tad_mi355x.h")]
    objs = []
    for src in sources:
        obj, srcp = os.path.join(objdir, src.replace(".hip", ".o")), os.path.join(CSRC, src)
        deps = [srcp, *headers, *[os.path.join(CSRC, d) for d in EXTRA_DEPS.get(src, [])]]
        objs.append(obj)
        if not force and os.path.exists(obj) and os.path.getmtime(obj) >= max(os.path.getmtime(p) for p in deps):
            continue
        cmd = [hipcc, *FLAGS, "-fvisibility=hidden", "-c", srcp, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-fvisibility=hidden", "-o", lib, *objs]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return lib


def _build_core(force: bool = False, verbose: bool = True) -> str:
    if not force and os.path.exists(LIB) and os.path.getmtime(LIB) >= _deps_mtime():
        return LIB
    objdir = os.path.join(HERE, "build") if _PRODUCTION else os.path.join(EXP_DIR, "obj_" + os.path.splitext(os.path.basename(LIB))[0])
    os.makedirs(objdir, exist_ok=True)
    hipcc = _hipcc()

    headers = [os.path.join(CSRC, "common.h"), os.path.join(CSRC, "opnd_f16_names.h"), os.path.join(os.path.dirname(HERE), "include", "tad_mi355x.h")]

    def compile_one(job):
        src, half = job
        obj = os.path.join(objdir, src.replace(".hip", "_f16.o" if half else ".o"))
        srcp = os.path.join(CSRC, src)
        deps = [srcp, *headers, *[os.path.join(CSRC, d) for d in EXTRA_DEPS.get(src, [])]]
        if not force and os.path.exists(obj) and os.path.getmtime(obj) >= max(os.path.getmtime(p) for p in deps):
            return obj
        flags = [f for f in FLAGS if f not in ("-mllvm", "-amdgpu-mfma-vgpr-form=1")] if src in NO_VGPR_FORM else FLAGS
        if src in NO_FP_CONTRACT:
            flags = ["-ffp-contract=off" if f == "-ffp-contract=fast" else f for f in flags]
        cmd = [hipcc, *flags, *(["-DTAD_OPND_F16"] if half else []), *(["-DTAD_GEMM_ABLATION"] if _ABLATION else []),
               *os.environ.get("TAD_BUILD_DEFINES", "").split(), "-c", srcp, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        return obj

    # longest jobs first (gemm.hip takes ~35 s per pass); TAD_BUILD_JOBS bounds the parallelism (default: the CPU count, at most 8)
    jobs = sorted([(s, False) for s in SOURCES] + [(s, True) for s in F16_SOURCES], key=lambda j: -os.path.getsize(os.path.join(CSRC, j[0])))
    workers = int(os.environ.get("TAD_BUILD_JOBS", 0)) or min(8, os.cpu_count() or 4)
    with ThreadPoolExecutor(max_workers=workers) as ex:
        objs = list(ex.map(compile_one, jobs))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs, "-ldl"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
