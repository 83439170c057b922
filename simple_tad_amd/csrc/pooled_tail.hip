// Pooled tail: the two HBM-bound kernels and the B-row fc2 of the last block when only the token mean of its output is read (ops.BlockPoolFn).
//   x2 = x1 + dp2 (a W2^T + b2) is linear in a: mean_n(x2) = mean_n(x1) + dp2 ((sum_n a / N) W2^T + b2) needs the per-clip column
//   sums of a, not the fc2 GEMM; in the backward every token of clip b receives dy[b] / N, so the accumulator row t[b] = gb[b] W2 of
//   the fc2 input gradient is the same for all N rows of the clip and only the GELU' factor differs from row to row.
// The first two are streaming kernels over [B*N, K] 16-bit matrices: a wave owns 512 columns (16 bytes per lane) and walks rows of ONE clip, so
// the per-clip operand (the f32 sums / the row t[b]) stays in registers.
// Compiled once per operand format like the other 16-bit sources (the GELU' polynomial and the conversions are the pass's own); the
// C entry points exist ONCE, in the bf16 pass, and take the format as an argument.
#include "common.h"

TAD_NAMESPACE_BEGIN

// ---------------------------------------------------------------- per-clip column sums
// partial[b][s][K]: block (x = chunk of 512 columns, y = row split s, z = clip b); the 4 waves stride over the rows of the split with
// four 16-byte loads in flight each.  The order of the additions depends on (N, K) only.
__global__ __launch_bounds__(256) void colsum_segments_partial_kernel(const uint16_t* __restrict__ a, float* __restrict__ partial, int N, int K) {
  __shared__ float red[4][8][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = (blockIdx.x * 64 + lane) * 8;
  const int s = blockIdx.y, b = blockIdx.z;
  const int rows_per = (N + TAD_POOL_SPLIT - 1) / TAD_POOL_SPLIT;
  const int n0 = s * rows_per, n1 = min(N, n0 + rows_per);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto add = [&](const uint4& v) {
    acc[0] += op16_lo_f32(v.x); acc[1] += op16_hi_f32(v.x);
    acc[2] += op16_lo_f32(v.y); acc[3] += op16_hi_f32(v.y);
    acc[4] += op16_lo_f32(v.z); acc[5] += op16_hi_f32(v.z);
    acc[6] += op16_lo_f32(v.w); acc[7] += op16_hi_f32(v.w);
  };
  if (c0 < K) {
    const uint16_t* base = a + (int64_t)b * N * K + c0;
    int n = n0 + wave;
    for (; n + 12 < n1; n += 16) {
      const uint4 v0 = *reinterpret_cast<const uint4*>(base + (int64_t)n * K);
      const uint4 v1 = *reinterpret_cast<const uint4*>(base + (int64_t)(n + 4) * K);
      const uint4 v2 = *reinterpret_cast<const uint4*>(base + (int64_t)(n + 8) * K);
      const uint4 v3 = *reinterpret_cast<const uint4*>(base + (int64_t)(n + 12) * K);
      add(v0); add(v1); add(v2); add(v3);
    }
    for (; n < n1; n += 4) add(*reinterpret_cast<const uint4*>(base + (int64_t)n * K));
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[wave][j][lane] = acc[j];
  __syncthreads();
  if (wave == 0 && c0 < K) {
    float t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = (red[0][j][lane] + red[1][j][lane]) + (red[2][j][lane] + red[3][j][lane]);
    float4* o = reinterpret_cast<float4*>(partial + ((int64_t)b * TAD_POOL_SPLIT + s) * K + c0);
    o[0] = make_float4(t[0], t[1], t[2], t[3]);
    o[1] = make_float4(t[4], t[5], t[6], t[7]);
  }
}
#ifndef TAD_OPND_F16  // f32 in, f32 out: one copy for the library (bf16 pass)
__global__ void colsum_segments_final_kernel(const float* __restrict__ partial, float* __restrict__ S, int B, int K) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * K) return;
  const int b = i / K, j = i - b * K;
  float s = 0.f;
  for (int k = 0; k < TAD_POOL_SPLIT; ++k) s += partial[((int64_t)b * TAD_POOL_SPLIT + k) * K + j];
  S[i] = s;
}
#endif

// ---------------------------------------------------------------- dh = op16(t[clip] * gelu'(h))
// block (x = chunk of 512 columns, y = group of GG_ROWS rows, z = clip b); the lane's eight values of t[b] are loaded once.  The product
// and the rounding are the EPI_DGELU epilogue's (gemm_kernels.h): gelu_grad_fast_row<4> on eight consecutive columns, pack_op16x2.
constexpr int GG_ROWS = 64;
__global__ __launch_bounds__(256) void gelu_grad_bcast_kernel(const float* __restrict__ t, const uint16_t* __restrict__ h, uint16_t* __restrict__ dh,
                                                              int N, int K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = (blockIdx.x * 64 + lane) * 8;
  if (c0 >= K) return;
  const int b = blockIdx.z;
  const int n0 = blockIdx.y * GG_ROWS, n1 = min(N, n0 + GG_ROWS);
  const float4 ta = *reinterpret_cast<const float4*>(t + (int64_t)b * K + c0);
  const float4 tb = *reinterpret_cast<const float4*>(t + (int64_t)b * K + c0 + 4);
  const int64_t off = (int64_t)b * N * K + c0;
  auto one = [&](const uint4& hv) {
    float v[8] = {ta.x, ta.y, ta.z, ta.w, tb.x, tb.y, tb.z, tb.w};
    const uint32_t hw[4] = {hv.x, hv.y, hv.z, hv.w};
    gelu_grad_fast_row<4>(v, hw);
    return make_uint4(pack_op16x2(v[0], v[1]), pack_op16x2(v[2], v[3]), pack_op16x2(v[4], v[5]), pack_op16x2(v[6], v[7]));
  };
  int n = n0 + wave;
  for (; n + 12 < n1; n += 16) {
    const uint4 h0 = *reinterpret_cast<const uint4*>(h + off + (int64_t)n * K);
    const uint4 h1 = *reinterpret_cast<const uint4*>(h + off + (int64_t)(n + 4) * K);
    const uint4 h2 = *reinterpret_cast<const uint4*>(h + off + (int64_t)(n + 8) * K);
    const uint4 h3 = *reinterpret_cast<const uint4*>(h + off + (int64_t)(n + 12) * K);
    *reinterpret_cast<uint4*>(dh + off + (int64_t)n * K) = one(h0);
    *reinterpret_cast<uint4*>(dh + off + (int64_t)(n + 4) * K) = one(h1);
    *reinterpret_cast<uint4*>(dh + off + (int64_t)(n + 8) * K) = one(h2);
    *reinterpret_cast<uint4*>(dh + off + (int64_t)(n + 12) * K) = one(h3);
  }
  for (; n < n1; n += 4) *reinterpret_cast<uint4*>(dh + off + (int64_t)n * K) = one(*reinterpret_cast<const uint4*>(h + off + (int64_t)n * K));
}

// ---------------------------------------------------------------- pooled fc2: out = xbar + rowscale ((S W^T) / N + bias)
// S [B,K] f32 (the per-clip column sums), w [D,K] 16-bit, out [B,D] f32.  B * D dot products of length K on the f32 sums -- the pooled
// operand is not rounded to 16 bits -- accumulated in f64: the general path averages the f32 accumulation errors of N independent rows,
// which a single f32 dot product per output has no share in (measured at K = 512: 4.7 x the general path's distance from fp64).  The
// products f32 x 16-bit are exact in f64, the work is B D K fused multiply-adds (75 M for ViT-B): the kernel is bound by its L2 reads.
// block = PL_COLS output columns x all clips, PL_ROWS clips at a time; thread t owns the 8-element chunks t, t + 256, ... of the rows.
constexpr int PL_COLS = 2, PL_ROWS = 4;
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__global__ __launch_bounds__(256) void pooled_linear_kernel(const float* __restrict__ S, const uint16_t* __restrict__ w, const float* __restrict__ bias,
                                                            const float* __restrict__ rowscale, const float* __restrict__ xbar,
                                                            float* __restrict__ out, int B, int N, int D, int K) {
  __shared__ double red[4][PL_ROWS][PL_COLS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d0 = blockIdx.x * PL_COLS;
  const int K8 = K >> 3;
  for (int b0 = 0; b0 < B; b0 += PL_ROWS) {
    double acc[PL_ROWS][PL_COLS];
#pragma unroll
    for (int r = 0; r < PL_ROWS; ++r)
#pragma unroll
      for (int c = 0; c < PL_COLS; ++c) acc[r][c] = 0.0;
    for (int ch = tid; ch < K8; ch += 256) {
      float wf[PL_COLS][8];
#pragma unroll
      for (int c = 0; c < PL_COLS; ++c) {
        const int d = min(d0 + c, D - 1);  // (a column past D repeats the last one and is not stored)
        const uint4 wv = *reinterpret_cast<const uint4*>(w + (int64_t)d * K + ch * 8);
        wf[c][0] = op16_lo_f32(wv.x); wf[c][1] = op16_hi_f32(wv.x); wf[c][2] = op16_lo_f32(wv.y); wf[c][3] = op16_hi_f32(wv.y);
        wf[c][4] = op16_lo_f32(wv.z); wf[c][5] = op16_hi_f32(wv.z); wf[c][6] = op16_lo_f32(wv.w); wf[c][7] = op16_hi_f32(wv.w);
      }
#pragma unroll
      for (int r = 0; r < PL_ROWS; ++r) {
        const int b = min(b0 + r, B - 1);  // (a clip past B repeats the last one and is not stored)
        const float4 s0 = *reinterpret_cast<const float4*>(S + (int64_t)b * K + ch * 8);
        const float4 s1 = *reinterpret_cast<const float4*>(S + (int64_t)b * K + ch * 8 + 4);
        const float sf[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
        for (int c = 0; c < PL_COLS; ++c)
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[r][c] = fma((double)sf[e], (double)wf[c][e], acc[r][c]);
      }
    }
#pragma unroll
    for (int r = 0; r < PL_ROWS; ++r)
#pragma unroll
      for (int c = 0; c < PL_COLS; ++c) {
        const double v = wave_sum_f64(acc[r][c]);
        if (lane == 0) red[wave][r][c] = v;
      }
    __syncthreads();
    if (tid < PL_ROWS * PL_COLS) {
      const int r = tid / PL_COLS, c = tid % PL_COLS;
      const int b = b0 + r, d = d0 + c;
      if (b < B && d < D) {
        double u = ((red[0][r][c] + red[1][r][c]) + (red[2][r][c] + red[3][r][c])) / (double)N;
        if (bias) u += (double)bias[d];
        if (rowscale) u *= (double)rowscale[b];
        out[(int64_t)b * D + d] = (float)(u + (double)xbar[(int64_t)b * D + d]);
      }
    }
    __syncthreads();  // (red is reused by the next group of clips)
  }
}

// the pass's launchers (C++ linkage: tad::op_bf16::... / tad::op_f16::...), arguments already validated
void launch_pooled_linear(const float* S, const uint16_t* w, const float* bias, const float* rowscale, const float* xbar, float* out, int B, int N,
                          int D, int K, hipStream_t stream) {
  hipLaunchKernelGGL(pooled_linear_kernel, dim3((D + PL_COLS - 1) / PL_COLS), dim3(256), 0, stream, S, w, bias, rowscale, xbar, out, B, N, D, K);
}
void launch_colsum_segments_partial(const uint16_t* a, float* partial, int B, int N, int K, hipStream_t stream) {
  hipLaunchKernelGGL(colsum_segments_partial_kernel, dim3((K + 511) / 512, TAD_POOL_SPLIT, B), dim3(256), 0, stream, a, partial, N, K);
}
void launch_gelu_grad_bcast(const float* t, const uint16_t* h, uint16_t* dh, int B, int N, int K, hipStream_t stream) {
  hipLaunchKernelGGL(gelu_grad_bcast_kernel, dim3((K + 511) / 512, (N + GG_ROWS - 1) / GG_ROWS, B), dim3(256), 0, stream, t, h, dh, N, K);
}

TAD_NAMESPACE_END

#ifndef TAD_OPND_F16  // the entry points: one copy for the library (bf16 pass), dispatching on the operand format
namespace tad { namespace op_f16 {
void launch_colsum_segments_partial(const uint16_t* a, float* partial, int B, int N, int K, hipStream_t stream);
void launch_gelu_grad_bcast(const float* t, const uint16_t* h, uint16_t* dh, int B, int N, int K, hipStream_t stream);
void launch_pooled_linear(const float* S, const uint16_t* w, const float* bias, const float* rowscale, const float* xbar, float* out, int B, int N,
                          int D, int K, hipStream_t stream);
}}
using namespace tad;

extern "C" {

int tad_colsum_segments(const uint16_t* a, int op_dtype, float* S, void* ws, size_t ws_bytes, int B, int N, int K, tad_stream_t stream) {
  TAD_REQUIRE(a && S && ws, "colsum_segments: null pointer");
  TAD_REQUIRE(op_dtype == TAD_BF16 || op_dtype == TAD_F16, "colsum_segments: op_dtype must be TAD_BF16 or TAD_F16");
  TAD_REQUIRE(B > 0 && N > 0 && K > 0 && B <= 65535, "colsum_segments: bad shape B=%d N=%d K=%d (B in 1..65535, N > 0, K > 0)", B, N, K);
  TAD_REQUIRE(K % 8 == 0, "colsum_segments: K=%d must be a multiple of 8", K);
  TAD_REQUIRE((int64_t)B * K < (int64_t)1 << 31, "colsum_segments: B * K exceeds 2^31");
  TAD_REQUIRE_ALIGNED("colsum_segments", a, 16);
  TAD_REQUIRE_ALIGNED("colsum_segments", S, 16);
  TAD_REQUIRE_ALIGNED("colsum_segments", ws, 16);
  if (ws_bytes < (size_t)B * TAD_POOL_SPLIT * (size_t)K * sizeof(float)) { set_error("colsum_segments: workspace too small"); return TAD_ENOSPACE; }
  if (op_dtype == TAD_F16) tad::op_f16::launch_colsum_segments_partial(a, (float*)ws, B, N, K, (hipStream_t)stream);
  else tad::op_bf16::launch_colsum_segments_partial(a, (float*)ws, B, N, K, (hipStream_t)stream);
  hipLaunchKernelGGL(colsum_segments_final_kernel, dim3((B * K + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)ws, S, B, K);
  return check_launch("colsum_segments");
}

int tad_pooled_linear(const float* S, const uint16_t* w, int op_dtype, const float* bias, const float* rowscale, const float* xbar, float* out,
                      int B, int N, int D, int K, tad_stream_t stream) {
  TAD_REQUIRE(S && w && xbar && out, "pooled_linear: null pointer");
  TAD_REQUIRE(op_dtype == TAD_BF16 || op_dtype == TAD_F16, "pooled_linear: op_dtype must be TAD_BF16 or TAD_F16");
  TAD_REQUIRE(B > 0 && N > 0 && D > 0 && K > 0, "pooled_linear: bad shape B=%d N=%d D=%d K=%d (all > 0)", B, N, D, K);
  TAD_REQUIRE(K % 8 == 0, "pooled_linear: K=%d must be a multiple of 8", K);
  TAD_REQUIRE_ALIGNED("pooled_linear", S, 16);
  TAD_REQUIRE_ALIGNED("pooled_linear", w, 16);
  TAD_REQUIRE_ALIGNED("pooled_linear", xbar, 4);
  TAD_REQUIRE_ALIGNED("pooled_linear", out, 4);
  TAD_REQUIRE_ALIGNED("pooled_linear", bias, 4);
  TAD_REQUIRE_ALIGNED("pooled_linear", rowscale, 4);
  TAD_REQUIRE(xbar != out, "pooled_linear: out must not alias xbar");
  if (op_dtype == TAD_F16) tad::op_f16::launch_pooled_linear(S, w, bias, rowscale, xbar, out, B, N, D, K, (hipStream_t)stream);
  else tad::op_bf16::launch_pooled_linear(S, w, bias, rowscale, xbar, out, B, N, D, K, (hipStream_t)stream);
  return check_launch("pooled_linear");
}

int tad_gelu_grad_bcast(const float* t, const uint16_t* h, uint16_t* dh, int op_dtype, int B, int N, int K, tad_stream_t stream) {
  TAD_REQUIRE(t && h && dh, "gelu_grad_bcast: null pointer");
  TAD_REQUIRE(op_dtype == TAD_BF16 || op_dtype == TAD_F16, "gelu_grad_bcast: op_dtype must be TAD_BF16 or TAD_F16");
  TAD_REQUIRE(B > 0 && N > 0 && K > 0 && B <= 65535 && (N + GG_ROWS - 1) / GG_ROWS <= 65535,
              "gelu_grad_bcast: bad shape B=%d N=%d K=%d (B in 1..65535, N > 0, K > 0)", B, N, K);
  TAD_REQUIRE(K % 8 == 0, "gelu_grad_bcast: K=%d must be a multiple of 8", K);
  TAD_REQUIRE_ALIGNED("gelu_grad_bcast", t, 16);
  TAD_REQUIRE_ALIGNED("gelu_grad_bcast", h, 16);
  TAD_REQUIRE_ALIGNED("gelu_grad_bcast", dh, 16);
  if (op_dtype == TAD_F16) tad::op_f16::launch_gelu_grad_bcast(t, h, dh, B, N, K, (hipStream_t)stream);
  else tad::op_bf16::launch_gelu_grad_bcast(t, h, dh, B, N, K, (hipStream_t)stream);
  return check_launch("gelu_grad_bcast");
}

}  // extern "C"
#endif
