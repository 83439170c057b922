#!/usr/bin/env python3
"""Run the TEXT of the multi-scale crop kernel (simple_tad_amd/csrc/multiscale_crop.hip, from its constants to the end of the kernel,
behind the device half of csrc/frame_io.h: the tile, the clamps and the writers of the output) on the CPU, in a stand-alone program built with the address and undefined-behaviour sanitizers, and hold it to the goldens.

The program defines the few HIP words the kernel uses (``__global__``, ``threadIdx``, ``__shared__`` as static storage,
``__fdiv_rn`` ...) and runs the 256 threads of a workgroup in turn, barrier by barrier: ``__syncthreads()`` ends a thread's run at the
barrier of the current phase, and every phase runs the kernel from its start again (all it does before a barrier is idempotent).
Inputs, table and output are heap blocks of exactly their size, so a load or store outside them ends the program.  No GPU, no
library, nothing loaded into Python: the program has its own ``main`` and exchanges files with this script.

Checked: every case of tests/golden/g18_multiscale_crop.npz (0 differing bytes; the f32 output bit-equal to the torch expression of
``frames_to_clip``), a rectangular output with ragged tiles, and a malformed table -- a sample outside the batch, a crop, set indices,
``ksize`` and bounds far outside -- where the valid clip must be right, the unnamed clip untouched and the wild row equal to what the
clamps of the kernel define.

usage: python tools/multiscale_crop_host_check.py [--keep DIR]        (needs a C++17 compiler with -fsanitize=address,undefined)
"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
KERNEL = os.path.join(ROOT, "simple_tad_amd", "csrc", "multiscale_crop.hip")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

SHIM = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#define TAD_MSC_ROW_WORDS 8
#define TAD_MSC_SET_HEAD 4
#define TAD_MSC_MAX_KSIZE 17
#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define __shared__ static
struct Idx { unsigned x, y, z; };
static Idx threadIdx, blockIdx;
static int g_phase, g_seen;
#define __syncthreads() do { if (g_seen++ == g_phase) return; } while (0)
static inline float __fdiv_rn(float a, float b) { return a / b; }
static inline float __fsub_rn(float a, float b) { return a - b; }
struct float4 { float x, y, z, w; };
static inline float4 make_float4(float a, float b, float c, float d) { return {a, b, c, d}; }
"""

MAIN = r"""
template <class T> static T* rd(const char* p, size_t* n) {  // a heap block of exactly the file's size
  FILE* f = fopen(p, "rb"); if (!f) abort();
  fseek(f, 0, SEEK_END); long bytes = ftell(f); fseek(f, 0, SEEK_SET);
  T* v = (T*)malloc(bytes); if (fread(v, 1, bytes, f) != (size_t)bytes) abort(); fclose(f); *n = bytes / sizeof(T); return v; }
int main(int argc, char** argv) {  // x.bin tab.bin out.bin f32 B T Hs Ws Sh Sw nh nv
  if (argc != 13) return 2;
  size_t nx, nt;
  uint8_t* x = rd<uint8_t>(argv[1], &nx); int32_t* tab = rd<int32_t>(argv[2], &nt);
  const int f32 = atoi(argv[4]), B = atoi(argv[5]), T = atoi(argv[6]), Hs = atoi(argv[7]), Ws = atoi(argv[8]), Sh = atoi(argv[9]),
            Sw = atoi(argv[10]), nh = atoi(argv[11]), nv = atoi(argv[12]);
  if (nx != (size_t)B * T * Hs * Ws * 3 || nt != (size_t)mc_table_words(B, nh, nv, Sh, Sw)) return 3;
  const size_t on = (size_t)B * T * Sh * Sw * 3 * (f32 ? 4 : 1);
  void* out = malloc(on); memset(out, 0x7F, on);
  ClipNorm nm = {{0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}};
  const int tiles_x = (Sw + FRAME_TC - 1) / FRAME_TC, tiles_y = (Sh + FRAME_TR - 1) / FRAME_TR;
  for (unsigned z = 0; z < (unsigned)B; ++z) for (unsigned y = 0; y < (unsigned)T; ++y) for (unsigned t = 0; t < (unsigned)(tiles_x * tiles_y); ++t)
    for (g_phase = 0; g_phase < 3; ++g_phase) for (unsigned tid = 0; tid < FRAME_THREADS; ++tid) {
      blockIdx = {t, y, z}; threadIdx = {tid, 0, 0}; g_seen = 0;
      if (f32) multiscale_crop_kernel<true>(x, out, tab, nm, B, T, Hs, Ws, Sh, Sw, nh, nv, tiles_x);
      else multiscale_crop_kernel<false>(x, out, tab, nm, B, T, Hs, Ws, Sh, Sw, nh, nv, tiles_x);
    }
  FILE* f = fopen(argv[3], "wb"); fwrite(out, 1, on, f); fclose(f);
  free(x); free(tab); free(out);
  return 0;
}
"""


def compiler():
    for c in (os.environ.get("CXX"), "g++", "clang++"):
        if c and shutil.which(c):
            return c
    return None


def build(workdir):
    """the stand-alone program: the kernel's own text between two shims; returns its path"""
    with open(KERNEL) as f:
        src = f.read()
    body = src[src.index("constexpr int MC_K"):src.index("TAD_NAMESPACE_END")]
    with open(os.path.join(os.path.dirname(KERNEL), "frame_io.h")) as f:  # what the kernel shares with the other frame kernels: device side
        src = f.read()
    body = src[src.index("struct ClipNorm"):src.index("// ----", src.index("struct ClipNorm"))] + body
    with open(os.path.join(os.path.dirname(KERNEL), "common.h")) as f:  # the one helper of common.h the kernel calls, in its own text too
        normalize = next(line for line in f if "float normalize_u8(" in line)
    cpp, exe = os.path.join(workdir, "msc_host.cpp"), os.path.join(workdir, "msc_host")
    with open(cpp, "w") as f:
        f.write(SHIM + normalize + body + MAIN)
    subprocess.run([compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, cpp],
                   check=True)
    return exe


def run(exe, workdir, x, table, f32, Sh, Sw, nh, nv):
    B, T, Hs, Ws, _ = x.shape
    paths = [os.path.join(workdir, n) for n in ("x.bin", "tab.bin", "out.bin")]
    np.ascontiguousarray(x).tofile(paths[0])
    np.ascontiguousarray(table, dtype=np.int32).tofile(paths[1])
    r = subprocess.run([exe, *paths, str(int(f32)), *[str(v) for v in (B, T, Hs, Ws, Sh, Sw, nh, nv)]], capture_output=True, text=True)
    if r.returncode != 0:
        raise AssertionError(f"the host build of the kernel ended with {r.returncode}:\n{r.stderr[-4000:]}")
    if f32:
        return np.fromfile(paths[2], np.float32).reshape(B, 3, T, Sh, Sw)
    return np.fromfile(paths[2], np.uint8).reshape(B, T, Sh, Sw, 3)


def clip_f32(frames_u8):
    """frames_to_clip's expression on the CPU: x / 255, minus mean, over std, in f32; [B,T,H,W,3] -> [B,3,T,H,W]"""
    import torch
    v = (torch.from_numpy(frames_u8).float().div(255) - torch.tensor(MEAN)) / torch.tensor(STD)
    return v.permute(0, 4, 1, 2, 3).contiguous().numpy()


def check(exe, workdir, verbose=True):
    import multiscale_crop_recipe as MR
    from simple_tad_amd import transforms as TF
    say = print if verbose else (lambda *a: None)
    g = np.load(os.path.join(ROOT, "tests", "golden", "g18_multiscale_crop.npz"))
    for key, _, (Hs, Ws), S, kw, kind in MR.CASES:
        tf = TF.GroupMultiScaleCrop(S, **{k: list(v) if k == "scales" else v for k, v in kw.items()})
        plan = [TF.Crop(b, *[int(v) for v in row]) for b, row in enumerate(g[f"{key}.crops"])]
        table, nh, nv = tf.table(plan, MR.B, Hs, Ws)
        x = MR.frames(Hs, Ws, kind)
        out = run(exe, workdir, x, table.numpy(), False, S, S, nh, nv)
        diff = int((out != g[f"{key}.out"]).sum())
        clip = run(exe, workdir, x, table.numpy(), True, S, S, nh, nv)
        same = np.array_equal(clip.view(np.int32), clip_f32(out).view(np.int32))
        say(f"{key}: {diff} of {out.size} bytes differ from the reference; f32 output bit-equal: {same}")
        assert diff == 0 and same, key

    # a rectangular output: three column tiles, two row tiles, ragged edges
    x = MR.frames(100, 37)
    tf = TF.GroupMultiScaleCrop([70, 37])
    plan = [TF.Crop(0, 37, 100, 0, 0), TF.Crop(1, 30, 61, 7, 39), TF.Crop(2, 25, 25, 3, 70)]
    table, nh, nv = tf.table(plan, 3, 100, 37)
    out = run(exe, workdir, x, table.numpy(), False, 37, 70, nh, nv)
    want = np.stack([np.stack([MR.resize(x[c.clip, t, c.y0:c.y0 + c.h, c.x0:c.x0 + c.w], 70, 37) for t in range(MR.T)]) for c in plan])
    say(f"70 x 37: {int((out != want).sum())} of {want.size} bytes differ")
    assert np.array_equal(out, want)
    assert np.array_equal(run(exe, workdir, x, table.numpy(), True, 37, 70, nh, nv).view(np.int32), clip_f32(out).view(np.int32))

    # a malformed table is never an address
    Hs, Ws, S = 45, 80, 32
    x = MR.frames(Hs, Ws)
    tf = TF.GroupMultiScaleCrop(S)
    table, nh, nv = tf.table([TF.Crop(b, *c) for b, c in enumerate(MR.WILD_PLAN)], 3, Hs, Ws)
    bad, want2 = MR.wild_table(table.numpy(), x, S)                        # (tests/multiscale_crop_recipe.py says what is wild in it)
    out = run(exe, workdir, x, bad, False, S, S, nh, nv)
    assert np.array_equal(out[0], MR.crop_resize(x, [MR.WILD_PLAN[0]], S, S)[0])
    assert (out[1] == 0x7F).all()                                          # the clip no valid row names: untouched
    say(f"malformed table: the wild row differs from its clamped definition in {int((out[2] != want2).sum())} bytes")
    assert np.array_equal(out[2], want2)
    clip = run(exe, workdir, x, bad, True, S, S, nh, nv)
    assert np.array_equal(clip[0].view(np.int32), clip_f32(out)[0].view(np.int32))
    assert np.array_equal(clip[2].view(np.int32), clip_f32(out)[2].view(np.int32))
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", help="build and exchange files in DIR and leave them there")
    a = ap.parse_args()
    if compiler() is None:
        sys.exit("multiscale_crop_host_check: no C++ compiler (CXX, g++ or clang++)")
    if a.keep:
        os.makedirs(a.keep, exist_ok=True)
        check(build(a.keep), a.keep)
    else:
        with tempfile.TemporaryDirectory() as d:
            check(build(d), d)
    print("multiscale_crop_host_check: ok")


if __name__ == "__main__":
    main()
