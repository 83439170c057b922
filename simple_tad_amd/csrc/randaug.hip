// RandAugment on the device (rand_augment.py of the reference, applied by its datasets to the 16 PIL frames of every training clip:
// --aa rand-m6-n3-mstd0.5-inc1, bicubic) and the uint8 -> normalised f32 clip conversion that follows it (ToTensor, tensor_normalize,
// permute).  The host draws the plan (simple_tad_amd/rand_augment.py); this file carries it out on uint8 frames [B, T, H, W, 3].
//
// Table: int32 [n_layers][B][TAD_RANDAUG_ROW_WORDS], one row per (layer, clip); include/tad_mi355x.h documents the words.  A layer is
// at most one statistics launch (only when the host says that a clip of the layer needs per-frame statistics) and one apply launch,
// whatever B and T: blockIdx.z = row, blockIdx.y = frame, the workgroups of a frame stride over its items; every clip carries out
// its own operator (the operator is uniform per workgroup: no divergence).  Layers ping-pong between two uint8 buffers (the output
// and one in the workspace) because the geometric operators and Sharpness read neighbours; the input is only read.
//
// Arithmetic: PIL's, restated (tests/randaug_recipe.py is the same text in numpy and is held to PIL bit for bit):
//   lookup tables   Invert 255 - i; Posterize i & ~(2^(8 - bits) - 1); Solarize i < thresh ? i : 255 - i; SolarizeAdd i < 128 ?
//                   min(255, i + add) : i.  AutoContrast per (frame, channel): lo / hi = first / last occupied histogram bin, identity
//                   when hi <= lo, else (int)(i * scale + offset) cut to [0, 255] with scale = 255.0 / (hi - lo), offset = -lo * scale in
//                   double.  Equalize per (frame, channel): step = (pixels - last occupied bin's count) / 255, identity when fewer than two
//                   bins are occupied or step == 0, else (step / 2 + pixels below i) / step, integers.
//   ImageEnhance    out = (float)deg + alpha * (float)(in - deg) in float, stored by truncation; for alpha outside [0, 1] cut to
//                   [0, 255] first.  deg: Brightness 0; Contrast (int)(sum of L / pixels + 0.5) of the frame; Color L of the pixel,
//                   L = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16; Sharpness the 3 x 3 SMOOTH filter (1 1 1 / 1 5 1 / 1 1 1) / 13
//                   in float, rows from below upwards, each row (a * k0 + b * k1) + c * k2, started at 0.5 and truncated; the outermost
//                   rows and columns are the image's own.
//   affine          (Rotate, ShearX/Y, TranslateX/YRel; the host states the six coefficients as Python does)  xin = a0 * (x + 0.5) +
//                   a1 * (y + 0.5) + a2 (yin likewise) in double; outside [0, W) x [0, H) the fill colour stays; else minus 0.5, floor,
//                   BILINEAR a + (b - a) * d over clamped columns and rows (a missing row below repeats the row above) stored by
//                   truncation, or BICUBIC p1 + d * (p2 + d * (p3 + d * p4)) with p1 = v2, p2 = -v1 + v3, p3 = 2 * (v1 - v2) + v3 - v4,
//                   p4 = -v1 + v2 - v3 + v4 over four clamped columns and rows, cut to [0, 255] and truncated.
// The file is compiled without floating-point contraction (build.py): every product and sum rounds as the C code's does.
#include "frame_io.h"

TAD_NAMESPACE_BEGIN

constexpr int RA_THREADS = 256;
constexpr int RA_MAX_BLOCKS = 256 * 16;  // Guideline 11: a capped grid that strides
constexpr int RA_GROUP = 16;             // pixels per item of the pointwise operators: 48 bytes, three 16-byte loads and stores
constexpr int RA_STAT_BYTES = TAD_RANDAUG_STAT_BYTES;  // per frame: lut[3][256], then the int32 mean of L at byte 768

struct RaRow {  // one row of the table (TAD_RANDAUG_ROW_WORDS int32)
  int sample, op, iarg;
  uint32_t fill, bicubic_lo, bicubic_hi;
  float farg;
  int reserved;
  int32_t m[12];  // six doubles, low word first
};
static_assert(sizeof(RaRow) == 4 * TAD_RANDAUG_ROW_WORDS, "table row layout");

__host__ __device__ __forceinline__ bool ra_known(int op) { return op >= TAD_RA_COPY && op <= TAD_RA_AFFINE; }
__host__ __device__ __forceinline__ bool ra_needs_stats(int op) {
  return op == TAD_RA_AUTOCONTRAST || op == TAD_RA_EQUALIZE || op == TAD_RA_CONTRAST;
}
__host__ __device__ __forceinline__ double ra_coef(const RaRow& r, int i) {
  const uint64_t bits = ((uint64_t)(uint32_t)r.m[2 * i + 1] << 32) | (uint32_t)r.m[2 * i];
  double v;
  __builtin_memcpy(&v, &bits, 8);
  return v;
}

// the row as the kernels use it: a sample outside the batch gives op -1 = nothing to do, an unknown operator copies the clip (a
// malformed table is never an address, and every clip that a row names is written)
__device__ __forceinline__ RaRow ra_load_row(const int32_t* rows, int k, int B) {
  RaRow r;
  const int32_t* p = rows + (int64_t)k * TAD_RANDAUG_ROW_WORDS;
  int32_t* q = reinterpret_cast<int32_t*>(&r);
#pragma unroll
  for (int i = 0; i < TAD_RANDAUG_ROW_WORDS; ++i) q[i] = p[i];
  if (!ra_known(r.op)) r.op = TAD_RA_COPY;
  if (r.sample < 0 || r.sample >= B) r.op = -1;
  return r;
}

__device__ __forceinline__ int ra_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Image.blend(degenerate, image, alpha)
__device__ __forceinline__ int ra_blend(int deg, int in, float alpha, bool clip) {
  const float temp = (float)deg + alpha * (float)(in - deg);
  if (clip) {
    if (temp <= 0.0f) return 0;
    if (temp >= 255.0f) return 255;
  }
  return (int)temp & 255;
}

// ---------------------------------------------------------------- statistics: one workgroup per frame of a clip that needs them
__global__ __launch_bounds__(RA_THREADS) void randaug_stats_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ rows,
                                                                  uint8_t* __restrict__ stats, int B, int T, int HW) {
  const RaRow r = ra_load_row(rows, blockIdx.y, B);
  if (r.op < 0 || !ra_needs_stats(r.op)) return;  // (the same for every thread of the workgroup)
  const int t = blockIdx.x, tid = threadIdx.x;
  const int64_t frame = (int64_t)r.sample * T + t;
  const uint8_t* s = src + frame * HW * 3;
  uint8_t* st = stats + frame * RA_STAT_BYTES;
  __shared__ uint32_t hist[3 * 256];
  __shared__ unsigned long long lsum;
  __shared__ int lo[3], hi[3], step[3];
  for (int i = tid; i < 3 * 256; i += RA_THREADS) hist[i] = 0;
  if (tid == 0) lsum = 0;
  __syncthreads();
  if (r.op == TAD_RA_CONTRAST) {
    unsigned long long acc = 0;
    for (int p = tid; p < HW; p += RA_THREADS) acc += (unsigned)ra_luma(s[3 * p], s[3 * p + 1], s[3 * p + 2]);
    atomicAdd(&lsum, acc);
    __syncthreads();
    if (tid == 0) {
      const int mean = (int)((double)lsum / (double)HW + 0.5);
      *reinterpret_cast<int32_t*>(st + 768) = mean;
    }
    return;
  }
  // histograms per channel over the flat byte stream (channel = byte index mod 3): 16-byte loads on the aligned middle
  const int n = HW * 3;
  int head = (int)((16 - (reinterpret_cast<uintptr_t>(s) & 15)) & 15);
  if (head > n) head = n;
  const int nvec = (n - head) / 16;
  for (int i = tid; i < head; i += RA_THREADS) atomicAdd(&hist[(i % 3) * 256 + s[i]], 1u);
  for (int v = tid; v < nvec; v += RA_THREADS) {
    const int base = head + 16 * v;
    const uint4 q = *reinterpret_cast<const uint4*>(s + base);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    int c = base % 3;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      atomicAdd(&hist[c * 256 + ((w[k >> 2] >> ((k & 3) * 8)) & 255u)], 1u);
      c = c == 2 ? 0 : c + 1;
    }
  }
  for (int i = head + 16 * nvec + tid; i < n; i += RA_THREADS) atomicAdd(&hist[(i % 3) * 256 + s[i]], 1u);
  __syncthreads();
  if (tid < 3) {
    const uint32_t* h = hist + tid * 256;
    int first = 256, last = -1, occupied = 0;
    for (int i = 0; i < 256; ++i)
      if (h[i]) {
        if (first == 256) first = i;
        last = i;
        ++occupied;
      }
    lo[tid] = first, hi[tid] = last;
    if (r.op == TAD_RA_EQUALIZE) {
      const int stp = (occupied <= 1 || last < 0) ? 0 : (int)(((uint32_t)HW - h[last]) / 255u);
      step[tid] = stp;
      if (stp) {  // the table itself: a running sum
        uint32_t nsum = (uint32_t)stp / 2u;
        for (int i = 0; i < 256; ++i) {
          const uint32_t v = nsum / (uint32_t)stp;
          st[tid * 256 + i] = (uint8_t)(v > 255u ? 255u : v);
          nsum += h[i];
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < 3 * 256; i += RA_THREADS) {
    const int c = i >> 8, ix = i & 255;
    if (r.op == TAD_RA_EQUALIZE) {
      if (!step[c]) st[i] = (uint8_t)ix;
    } else {
      int v = ix;
      if (hi[c] > lo[c]) {
        const double scale = 255.0 / (double)(hi[c] - lo[c]);
        const double offset = (double)(-lo[c]) * scale;
        const double f = (double)ix * scale + offset;
        v = f <= 0.0 ? 0 : (f >= 255.0 ? 255 : (int)f);
      }
      st[i] = (uint8_t)v;
    }
  }
}

// ---------------------------------------------------------------- the operators
// pointwise operators: an item is RA_GROUP pixels (48 bytes) at a multiple of 48 bytes from the frame's first byte; where the frame
// starts on a 16-byte boundary in both buffers an item is three 16-byte loads and stores, else (and for the last, short item) bytes
template <class F>
__device__ __forceinline__ void ra_pointwise(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, int HW, F f) {
  const bool vec = ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 15) == 0;
  const int items = (HW + RA_GROUP - 1) / RA_GROUP;
  for (int it = blockIdx.x * RA_THREADS + threadIdx.x; it < items; it += gridDim.x * RA_THREADS) {
    const int p0 = it * RA_GROUP;
    const int np = HW - p0 < RA_GROUP ? HW - p0 : RA_GROUP;
    const uint8_t* sp = s + (int64_t)p0 * 3;
    uint8_t* dp = d + (int64_t)p0 * 3;
    uint32_t w[12];
    const bool whole = vec && np == RA_GROUP;
    if (whole) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const uint4 q = reinterpret_cast<const uint4*>(sp)[k];
        w[4 * k] = q.x, w[4 * k + 1] = q.y, w[4 * k + 2] = q.z, w[4 * k + 3] = q.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        uint32_t v = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (4 * k + e < 3 * np) v |= (uint32_t)sp[4 * k + e] << (8 * e);
        w[k] = v;
      }
    }
    uint32_t o[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = 0;
#pragma unroll
    for (int p = 0; p < RA_GROUP; ++p) {
      int c[3];
#pragma unroll
      for (int e = 0; e < 3; ++e) c[e] = (int)((w[(3 * p + e) >> 2] >> (((3 * p + e) & 3) * 8)) & 255u);
      f(c);
#pragma unroll
      for (int e = 0; e < 3; ++e) o[(3 * p + e) >> 2] |= (uint32_t)(c[e] & 255) << (((3 * p + e) & 3) * 8);
    }
    if (whole) {
#pragma unroll
      for (int k = 0; k < 3; ++k) reinterpret_cast<uint4*>(dp)[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (4 * k + e < 3 * np) dp[4 * k + e] = (uint8_t)(o[k] >> (8 * e));
    }
  }
}

__device__ __forceinline__ int ra_clip8f(float v) { return v <= 0.0f ? 0 : (v >= 255.0f ? 255 : (int)v); }
__device__ __forceinline__ int ra_clip8d(double v) { return v <= 0.0 ? 0 : (v >= 255.0 ? 255 : (int)v); }
__device__ __forceinline__ int ra_floor(double v) { return v < 0.0 ? (int)floor(v) : (int)v; }
__device__ __forceinline__ int ra_clampi(int v, int hi) { return v < 0 ? 0 : (v < hi ? v : hi - 1); }
__device__ __forceinline__ double ra_cubic(double v1, double v2, double v3, double v4, double d) {
  const double p1 = v2;
  const double p2 = -v1 + v3;
  const double p3 = 2 * (v1 - v2) + v3 - v4;
  const double p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

__global__ __launch_bounds__(RA_THREADS) void randaug_apply_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                  const int32_t* __restrict__ rows, const uint8_t* __restrict__ stats,
                                                                  int B, int T, int H, int W) {
  const RaRow r = ra_load_row(rows, blockIdx.z, B);
  if (r.op < 0) return;  // (the same for every thread of the workgroup)
  const int t = blockIdx.y, tid = threadIdx.x, HW = H * W;
  const int64_t frame = (int64_t)r.sample * T + t;
  const uint8_t* s = src + frame * HW * 3;
  uint8_t* d = dst + frame * HW * 3;
  const uint8_t* st = stats + frame * RA_STAT_BYTES;
  const int stride = gridDim.x * RA_THREADS, first = blockIdx.x * RA_THREADS + tid;
  __shared__ uint8_t lut[3 * 256];

  switch (r.op) {
    case TAD_RA_COPY:
      ra_pointwise(s, d, HW, [](int*) {});
      break;
    case TAD_RA_INVERT:
    case TAD_RA_POSTERIZE:
    case TAD_RA_SOLARIZE:
    case TAD_RA_SOLARIZE_ADD:
    case TAD_RA_AUTOCONTRAST:
    case TAD_RA_EQUALIZE: {
      for (int i = tid; i < 3 * 256; i += RA_THREADS) {
        const int ix = i & 255;
        int v = ix;
        if (r.op == TAD_RA_INVERT) v = 255 - ix;
        else if (r.op == TAD_RA_POSTERIZE) v = r.iarg >= 8 ? ix : (r.iarg <= 0 ? 0 : ix & ~((1 << (8 - r.iarg)) - 1));
        else if (r.op == TAD_RA_SOLARIZE) v = ix < r.iarg ? ix : 255 - ix;
        else if (r.op == TAD_RA_SOLARIZE_ADD) v = ix < 128 ? (ix + r.iarg > 255 ? 255 : (ix + r.iarg < 0 ? 0 : ix + r.iarg)) : ix;
        else v = st[i];
        lut[i] = (uint8_t)v;
      }
      __syncthreads();
      ra_pointwise(s, d, HW, [&](int* c) { c[0] = lut[c[0]], c[1] = lut[256 + c[1]], c[2] = lut[512 + c[2]]; });
      break;
    }
    case TAD_RA_BRIGHTNESS:
    case TAD_RA_COLOR:
    case TAD_RA_CONTRAST: {
      const float alpha = r.farg;
      const bool clip = !(alpha >= 0.0f && alpha <= 1.0f);
      int mean = 0;
      if (r.op == TAD_RA_CONTRAST) mean = *reinterpret_cast<const int32_t*>(st + 768) & 255;
      const bool color = r.op == TAD_RA_COLOR;
      ra_pointwise(s, d, HW, [&](int* c) {
        const int deg = color ? ra_luma(c[0], c[1], c[2]) : mean;
#pragma unroll
        for (int e = 0; e < 3; ++e) c[e] = ra_blend(deg, c[e], alpha, clip);
      });
      break;
    }
    case TAD_RA_SHARPNESS: {
      const float alpha = r.farg;
      const bool clip = !(alpha >= 0.0f && alpha <= 1.0f);
      const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
      for (int p = first; p < HW; p += stride) {
        const int y = p / W, x = p - y * W;
        const bool border = y == 0 || y == H - 1 || x == 0 || x == W - 1;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          const int in = s[3 * p + e];
          int deg = in;
          if (!border) {
            float ss = 0.5f;
#pragma unroll
            for (int dy = 1; dy >= -1; --dy) {
              const uint8_t* q = s + 3 * (p + dy * W) + e;
              ss += ((float)q[-3] * k1 + (float)q[0] * (dy == 0 ? k5 : k1)) + (float)q[3] * k1;
            }
            deg = ra_clip8f(ss);
          }
          d[3 * p + e] = (uint8_t)ra_blend(deg, in, alpha, clip);
        }
      }
      break;
    }
    case TAD_RA_AFFINE: {
      const double a0 = ra_coef(r, 0), a1 = ra_coef(r, 1), a2 = ra_coef(r, 2), a3 = ra_coef(r, 3), a4 = ra_coef(r, 4), a5 = ra_coef(r, 5);
      const bool bicubic = t < 32 ? (r.bicubic_lo >> t) & 1u : (r.bicubic_hi >> (t - 32)) & 1u;
      for (int p = first; p < HW; p += stride) {
        const int yo = p / W, xo = p - yo * W;
        const double xs = xo + 0.5, ys = yo + 0.5;
        double xin = a0 * xs + a1 * ys + a2;
        double yin = a3 * xs + a4 * ys + a5;
        int out[3] = {(int)(r.fill & 255u), (int)((r.fill >> 8) & 255u), (int)((r.fill >> 16) & 255u)};
        // (written so that a NaN coordinate counts as outside)
        if (xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H) {
          xin -= 0.5, yin -= 0.5;
          int x = ra_floor(xin), y = ra_floor(yin);
          const double dx = xin - x, dy = yin - y;
          if (!bicubic) {
            const int x0 = 3 * ra_clampi(x, W), x1 = 3 * ra_clampi(x + 1, W);
            const uint8_t* ra = s + 3 * W * ra_clampi(y, H);
            const bool below = y + 1 >= 0 && y + 1 < H;
            const uint8_t* rb = s + 3 * W * ra_clampi(y + 1, H);
#pragma unroll
            for (int e = 0; e < 3; ++e) {
              const double p0 = ra[x0 + e], p1 = ra[x1 + e];
              const double v1 = p0 + (p1 - p0) * dx;
              double v2 = v1;
              if (below) {
                const double q0 = rb[x0 + e], q1 = rb[x1 + e];
                v2 = q0 + (q1 - q0) * dx;
              }
              out[e] = (int)(v1 + (v2 - v1) * dy) & 255;
            }
          } else {
            --x, --y;
            int xc[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) xc[k] = 3 * ra_clampi(x + k, W);
#pragma unroll
            for (int e = 0; e < 3; ++e) {
              double v[4];
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                const int yy = y + k;
                if (k == 0 || (yy >= 0 && yy < H)) {
                  const uint8_t* q = s + 3 * W * ra_clampi(yy, H) + e;
                  v[k] = ra_cubic(q[xc[0]], q[xc[1]], q[xc[2]], q[xc[3]], dx);
                } else {
                  v[k] = v[k - 1];
                }
              }
              out[e] = ra_clip8d(ra_cubic(v[0], v[1], v[2], v[3], dy));
            }
          }
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) d[3 * p + e] = (uint8_t)out[e];
      }
      break;
    }
    default:
      break;
  }
}

// ---------------------------------------------------------------- uint8 frames [B,T,H,W,3] -> normalised f32 clips [B,3,T,H,W]
// ToTensor, tensor_normalize (normalize_u8, common.h: two IEEE divisions and one subtraction in f32 per element), permute.  An item
// is four pixels of a frame: twelve bytes in, one 16-byte store per channel plane where the planes are 16-byte aligned (a whole frame
// per stride, not the tiles of frame_io.h, which states the normalisation and the host checks this entry point shares)
__global__ __launch_bounds__(RA_THREADS) void frames_to_clip_kernel(const uint8_t* __restrict__ x, float* __restrict__ out, float m0, float m1,
                                                                   float m2, float s0, float s1, float s2, int T, int HW) {
  const int t = blockIdx.y, b = blockIdx.z;
  const uint8_t* s = x + ((int64_t)b * T + t) * HW * 3;
  float* o = out + ((int64_t)b * 3 * T + t) * HW;  // channel c: + c * T * HW
  const int64_t plane = (int64_t)T * HW;
  const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
  const bool vec = (reinterpret_cast<uintptr_t>(s) & 3) == 0 && (reinterpret_cast<uintptr_t>(o) & 15) == 0 && (plane & 3) == 0;
  const int items = (HW + 3) / 4;
  for (int it = blockIdx.x * RA_THREADS + threadIdx.x; it < items; it += gridDim.x * RA_THREADS) {
    const int p0 = 4 * it;
    const int np = HW - p0 < 4 ? HW - p0 : 4;
    float v[3][4];
    if (vec && np == 4) {
      const uint32_t* sp = reinterpret_cast<const uint32_t*>(s + 3 * p0);
      const uint32_t w[3] = {sp[0], sp[1], sp[2]};
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        const float f = (float)((w[k >> 2] >> ((k & 3) * 8)) & 255u);
        v[k % 3][k / 3] = normalize_u8(f, mean[k % 3], sd[k % 3]);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(o + c * plane + p0) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    } else {
      for (int k = 0; k < 3 * np; ++k) {
        const float f = (float)s[3 * p0 + k];
        o[(k % 3) * plane + p0 + k / 3] = normalize_u8(f, mean[k % 3], sd[k % 3]);
      }
    }
  }
}

TAD_NAMESPACE_END

using namespace tad;

static int ra_shape_ok(int n_layers, int B, int T, int H, int W, const char* who) {
  TAD_REQUIRE(n_layers >= 0 && n_layers <= TAD_RANDAUG_MAX_LAYERS, "%s: n_layers=%d must be in [0, %d]", who, n_layers,
              TAD_RANDAUG_MAX_LAYERS);
  TAD_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= 64, "%s: B=%d must be in [1, 65535] and T=%d in [1, 64]", who, B, T);
  if (int rc = frame_extent_ok(who, H, W)) return rc;
  return TAD_OK;
}

extern "C" int tad_randaug_plan_check(const int32_t* table_host, int64_t n_words, int n_layers, int B, int T) {
  TAD_REQUIRE(table_host, "randaug_plan_check: null pointer");
  if (int rc = ra_shape_ok(n_layers, B, T, 1, 1, "randaug_plan_check")) return rc;
  TAD_REQUIRE(n_words == (int64_t)n_layers * B * TAD_RANDAUG_ROW_WORDS, "randaug_plan_check: %lld words, expected n_layers * B * %d = %lld",
              (long long)n_words, TAD_RANDAUG_ROW_WORDS, (long long)n_layers * B * TAD_RANDAUG_ROW_WORDS);
  for (int l = 0; l < n_layers; ++l) {
    SeenSamples seen;  // (B <= 65535)
    for (int k = 0; k < B; ++k) {
      const RaRow* r = reinterpret_cast<const RaRow*>(table_host + ((int64_t)l * B + k) * TAD_RANDAUG_ROW_WORDS);
      TAD_REQUIRE(0 <= r->sample && r->sample < B, "randaug_plan_check: layer %d row %d: sample=%d outside the batch B=%d", l, k, r->sample,
                  B);
      TAD_REQUIRE(!seen.twice(r->sample), "randaug_plan_check: layer %d row %d: sample=%d has two rows", l, k, r->sample);
      TAD_REQUIRE(ra_known(r->op), "randaug_plan_check: layer %d row %d: unknown op=%d", l, k, r->op);
      if (r->op == TAD_RA_POSTERIZE) TAD_REQUIRE(r->iarg >= 0 && r->iarg <= 8, "randaug_plan_check: layer %d row %d: bits=%d", l, k, r->iarg);
      if (r->op == TAD_RA_SOLARIZE) TAD_REQUIRE(r->iarg >= 0 && r->iarg <= 256, "randaug_plan_check: layer %d row %d: thresh=%d", l, k, r->iarg);
      if (r->op == TAD_RA_SOLARIZE_ADD) TAD_REQUIRE(r->iarg >= 0 && r->iarg <= 255, "randaug_plan_check: layer %d row %d: add=%d", l, k, r->iarg);
      if (r->op == TAD_RA_BRIGHTNESS || r->op == TAD_RA_COLOR || r->op == TAD_RA_CONTRAST || r->op == TAD_RA_SHARPNESS)
        TAD_REQUIRE(std::isfinite(r->farg), "randaug_plan_check: layer %d row %d: the enhance factor is not finite", l, k);
      if (r->op == TAD_RA_AFFINE) {
        for (int i = 0; i < 6; ++i)
          TAD_REQUIRE(std::isfinite(ra_coef(*r, i)), "randaug_plan_check: layer %d row %d: affine coefficient %d is not finite", l, k, i);
        TAD_REQUIRE(r->fill <= 0xFFFFFFu, "randaug_plan_check: layer %d row %d: fill=0x%x is not an RGB colour", l, k, r->fill);
      }
    }
  }
  return TAD_OK;
}

static size_t ra_align(size_t n) { return (n + 255) / 256 * 256; }

extern "C" size_t tad_randaug_workspace_bytes(int n_layers, int B, int T, int H, int W) {
  if (n_layers < 0 || B <= 0 || T <= 0 || H <= 0 || W <= 0) return 0;
  const size_t clip = ra_align((size_t)B * T * H * W * 3);
  return (size_t)B * T * RA_STAT_BYTES + (n_layers >= 2 ? clip : 0);
}

extern "C" int tad_randaug_apply(const uint8_t* x, uint8_t* out, const int32_t* table, int n_layers, uint32_t stats_layers, void* workspace,
                                 size_t workspace_bytes, int B, int T, int H, int W, tad_stream_t stream) {
  TAD_REQUIRE(x && out && x != out, "randaug_apply: x and out must be two buffers");
  if (int rc = ra_shape_ok(n_layers, B, T, H, W, "randaug_apply")) return rc;
  const size_t bytes = (size_t)B * T * H * W * 3;
  TAD_REQUIRE((x + bytes <= out || out + bytes <= x), "randaug_apply: x and out overlap");
  hipStream_t s = (hipStream_t)stream;
  if (n_layers == 0) {
    if (hipMemcpyAsync(out, x, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) return check_launch("randaug_apply(copy)");
    return TAD_OK;
  }
  TAD_REQUIRE(table && workspace, "randaug_apply: null pointer");
  TAD_REQUIRE_ALIGNED("randaug_apply", table, 4);
  TAD_REQUIRE_ALIGNED("randaug_apply", workspace, 256);
  TAD_REQUIRE(workspace_bytes >= tad_randaug_workspace_bytes(n_layers, B, T, H, W), "randaug_apply: workspace of %zu bytes, need %zu",
              workspace_bytes, tad_randaug_workspace_bytes(n_layers, B, T, H, W));
  uint8_t* stats = static_cast<uint8_t*>(workspace);
  uint8_t* tmp = stats + (size_t)B * T * RA_STAT_BYTES;  // (a multiple of 256 bytes in)
  const int HW = H * W;
  int64_t gx = ((int64_t)HW + RA_THREADS - 1) / RA_THREADS;
  const int64_t cap = (int64_t)B * T >= RA_MAX_BLOCKS ? 1 : RA_MAX_BLOCKS / ((int64_t)B * T);
  if (gx > cap) gx = cap;
  const uint8_t* src = x;
  for (int l = 0; l < n_layers; ++l) {
    uint8_t* dst = ((n_layers - 1 - l) & 1) ? tmp : out;  // the last layer writes out
    const int32_t* rows = table + (int64_t)l * B * TAD_RANDAUG_ROW_WORDS;
    if ((stats_layers >> l) & 1u) {
      hipLaunchKernelGGL(randaug_stats_kernel, dim3((unsigned)T, (unsigned)B), dim3(RA_THREADS), 0, s, src, rows, stats, B, T, HW);
      if (int rc = check_launch("randaug_apply(stats)")) return rc;
    }
    hipLaunchKernelGGL(randaug_apply_kernel, dim3((unsigned)gx, (unsigned)T, (unsigned)B), dim3(RA_THREADS), 0, s, src, dst, rows, stats, B,
                       T, H, W);
    if (int rc = check_launch("randaug_apply")) return rc;
    src = dst;
  }
  return TAD_OK;
}

extern "C" int tad_frames_to_clip(const uint8_t* x, float* out, const float* mean, const float* std_, int B, int T, int H, int W,
                                  tad_stream_t stream) {
  TAD_REQUIRE(x && out && mean && std_, "frames_to_clip: null pointer");
  if (int rc = ra_shape_ok(0, B, T, H, W, "frames_to_clip")) return rc;
  TAD_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "frames_to_clip: out must be 4-byte aligned");
  ClipNorm nm;
  if (int rc = clip_norm_from("frames_to_clip", mean, std_, &nm)) return rc;
  const int HW = H * W;
  int64_t gx = ((int64_t)(HW + 3) / 4 + RA_THREADS - 1) / RA_THREADS;
  const int64_t cap = (int64_t)B * T >= RA_MAX_BLOCKS ? 1 : RA_MAX_BLOCKS / ((int64_t)B * T);
  if (gx > cap) gx = cap;
  hipLaunchKernelGGL(frames_to_clip_kernel, dim3((unsigned)gx, (unsigned)T, (unsigned)B), dim3(RA_THREADS), 0, (hipStream_t)stream, x, out,
                     nm.mean[0], nm.mean[1], nm.mean[2], nm.sd[0], nm.sd[1], nm.sd[2], T, HW);
  return check_launch("frames_to_clip");
}
