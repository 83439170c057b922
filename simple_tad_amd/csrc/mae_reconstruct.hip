// MAE reconstruction: the reconstruction ABI of include/tad_mi355x_recon.h (tadr_*), the ONE source of libtad_mi355x_recon.so.
//   mae_reconstruct   the inverse of mae_target_kernel (mae.hip; engine_for_pretraining.py:51-66) in one pass: a masked clip back as uint8
//                     frames [B,T,H,W,3] -- visible patches from the clip, masked patches from the prediction, de-standardised with the
//                     patch's own statistics -- and the per-token reconstruction error [B,N].
// One workgroup per token, as mae_target_kernel; wave w < 3 owns channel w and holds the channel's tub*p*p pixels in registers, pixel
// lane + 64 i in slot i.  The statistics are mae_target_kernel's, restated instruction for instruction (same lane assignment, same
// butterfly sums, the mean as mu + corr), so that a prediction equal to tad_mae_target's labels gives the clip back; mae.hip itself is
// not touched.  Where that file leaves a product and a sum to -ffp-contract=fast, the fused form is spelled out here (fmaf).
// The clip's pixels are requested first and do not wait for slot; the token's row of pred comes in through LDS (all four waves, consecutive
// floats: the 'pix c' layout is a stride of three floats per lane otherwise); the bytes leave through LDS too: the three waves put their
// channel at byte pix*3 + c, and after a barrier all four waves write the patch's tub*p rows of 3p bytes each as whole 4-byte words where
// the row's address allows and as single bytes at its two ends.  Every byte is written by exactly one lane; no address of a store depends
// on slot.
// The library is self-contained (side_library.h) and exports the tadr_* entry points alone.
#include "side_library.h"
#pragma GCC visibility push(default)
#include "../../include/tad_mi355x_recon.h"
#pragma GCC visibility pop

TAD_NAMESPACE_BEGIN

// clamp(rint(x), 0, 255): halves to even; fmaxf returns the operand that is a number, so NaN -> 0; +inf -> 255, -inf -> 0
__device__ __forceinline__ uint8_t to_byte(float x) { return (uint8_t)(int)fminf(fmaxf(__builtin_rintf(x), 0.f), 255.f); }

template <int NPIX>
__global__ __launch_bounds__(256) void mae_reconstruct_kernel(const float* __restrict__ x, const float* __restrict__ pred,
                                                              const int32_t* __restrict__ slot, uint8_t* __restrict__ frames,
                                                              float* __restrict__ err, int N, int Nm, int T, int H, int W, int tub, int p,
                                                              float m0, float m1, float m2, float s0, float s1, float s2, int normalize,
                                                              float g255) {
  __shared__ float spred[64 * NPIX * 3];
  __shared__ __attribute__((aligned(4))) uint8_t sbyte[64 * NPIX * 3];
  __shared__ float red[3];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned row = blockIdx.x;  // b * N + tok (the launcher keeps B * N below 2^31)
  const int b = (int)(row / (unsigned)N), tok = (int)(row - (unsigned)b * (unsigned)N);
  const int sl = __builtin_amdgcn_readfirstlane(slot[row]);  // (one address per workgroup: a scalar load, on its own counter)
  const int Hp = H / p, Wp = W / p;
  const int tp = tok / (Hp * Wp), hw = tok - tp * Hp * Wp, hp = hw / Wp, wp = hw - hp * Wp;
  const int npix = tub * p * p, nent = npix * 3;
  // The clip's pixels are requested first, by the three channel waves, and do not wait for slot: they are in flight while slot arrives
  // and the row of pred -- which depends on it -- is requested behind them (one round trip to memory less per workgroup).
  const int c = wave < 3 ? wave : 0;
  const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
  const float* base = x + (((int64_t)b * 3 + c) * T + (int64_t)tp * tub) * H * W + (int64_t)hp * p * W + (int64_t)wp * p;
  float v[NPIX];
  if (wave < 3) {
    // pixel lane + 64 i sits at (kt, kh, kw) of the patch: divided out once, for i = 0, then advanced by 64 pixels a step with the
    // wave-uniform digits of 64 in base p (each digit sum stays below 2p: one carry).  Two integer divisions per pixel cost more
    // instructions than everything else in this kernel together.
    const int r64 = 64 % p, q64 = 64 / p, a64 = q64 / p, b64 = q64 - a64 * p;
    const int64_t HW = (int64_t)H * W, step = r64 + (int64_t)b64 * W + a64 * HW, step_w = W - p, step_h = HW - (int64_t)p * W;
    const int kt = lane / (p * p);
    int kh = (lane - kt * p * p) / p, kw = lane - kt * p * p - kh * p;
    int64_t off = ((int64_t)kt * H + kh) * W + kw;  // ((kt H) + kh) W + kw, carried along with the digits
#pragma unroll
    for (int i = 0; i < NPIX; ++i) {
      v[i] = 0.f;
      if (lane + 64 * i < npix) v[i] = base[off];
      kw += r64;
      const bool cw = kw >= p;
      kw -= cw ? p : 0;
      kh += b64 + (cw ? 1 : 0);
      const bool ch = kh >= p;
      kh -= ch ? p : 0;
      off += step + (cw ? step_w : 0) + (ch ? step_h : 0);
    }
  }
  const bool masked = sl >= 0 && sl < Nm;  // (anything else counts as -1, visible)
  if (masked) {
    const float* pr = pred + ((int64_t)b * Nm + sl) * nent;
    float t[(64 * NPIX * 3) / 256];
#pragma unroll
    for (int k = 0; k < (64 * NPIX * 3) / 256; ++k) {
      const int i = threadIdx.x + 256 * k;
      t[k] = i < nent ? pr[i] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < (64 * NPIX * 3) / 256; ++k) {
      const int i = threadIdx.x + 256 * k;
      if (i < nent) spred[i] = t[k];
    }
  }
  __syncthreads();
  if (wave < 3 && (frames != nullptr || masked)) {
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NPIX; ++i)
      if (lane + 64 * i < npix) {
        v[i] = fmaf(v[i], sd, mean);  // videos * std + mean
        sum += v[i];
      }
    if (!masked) {
#pragma unroll
      for (int i = 0; i < NPIX; ++i) {
        const int pix = lane + 64 * i;
        if (pix < npix) sbyte[pix * 3 + c] = to_byte(g255 * v[i]);
      }
    } else {
      float sdev = 1.f, inv = 1.f, m = 0.f;
      if (normalize) {
        // mae_target_kernel's statistics: the mean as two floats, the unbiased variance of the residuals
        const float mu = wave_sum(sum) / (float)npix;
        float rs = 0.f;
#pragma unroll
        for (int i = 0; i < NPIX; ++i)
          if (lane + 64 * i < npix) {
            v[i] -= mu;
            rs += v[i];
          }
        const float corr = wave_sum(rs) / (float)npix;
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < NPIX; ++i)
          if (lane + 64 * i < npix) {
            v[i] -= corr;
            sq = fmaf(v[i], v[i], sq);
          }
        const float var = wave_sum(sq) / (float)(npix - 1);
        sdev = sqrtf(var) + 1e-6f;
        inv = 1.f / sdev;
        m = mu + corr;
      }
      float e = 0.f;
#pragma unroll
      for (int i = 0; i < NPIX; ++i) {
        const int pix = lane + 64 * i;
        if (pix < npix) {
          const float pv = spred[pix * 3 + c];
          // (the label is rounded before it is compared, as tad_mae_target stores it)
          const float d = __fsub_rn(pv, normalize ? __fmul_rn(v[i], inv) : v[i]);
          e = fmaf(d, d, e);
          if (frames != nullptr) sbyte[pix * 3 + c] = to_byte(255.f * (normalize ? fmaf(pv, sdev, m) : pv));
        }
      }
      e = wave_sum(e);
      if (lane == 0) red[c] = e;
    }
  }
  __syncthreads();
  if (err != nullptr && threadIdx.x == 0) err[row] = masked ? ((red[0] + red[1]) + red[2]) / (float)nent : 0.f;
  if (frames == nullptr) return;
  // the patch's tub*p rows of 3p bytes: item (r, k) is the k-th 4-byte word of the frame buffer that row r touches
  const int rowbytes = 3 * p, nrows = tub * p, S = (rowbytes + 6) >> 2;
  for (int it = threadIdx.x; it < nrows * S; it += 256) {
    const int r = it / S, k = it - r * S;
    const int kt = r / p, kh = r - kt * p;
    uint8_t* dst = frames + ((((int64_t)b * T + (int64_t)tp * tub + kt) * H + (int64_t)hp * p + kh) * W + (int64_t)wp * p) * 3;
    const int j0 = 4 * k - (int)(reinterpret_cast<uintptr_t>(dst) & 3);  // the word's first byte, counted from the row's first
    if (j0 >= rowbytes) continue;
    const uint8_t* src = sbyte + r * rowbytes;
    if (j0 >= 0 && j0 + 4 <= rowbytes) {
      const uint32_t w = (uint32_t)src[j0] | ((uint32_t)src[j0 + 1] << 8) | ((uint32_t)src[j0 + 2] << 16) | ((uint32_t)src[j0 + 3] << 24);
      *reinterpret_cast<uint32_t*>(dst + j0) = w;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)  // the row's first or last word: the one to three bytes of it that belong to the row
        if (j0 + q >= 0 && j0 + q < rowbytes) dst[j0 + q] = src[j0 + q];
    }
  }
}

TAD_NAMESPACE_END

using namespace tad;

#pragma GCC visibility push(default)
extern "C" {

int tadr_abi_version(void) { return TADR_ABI_VERSION; }

const char* tadr_last_error_string(void) { return tad::side_last_error(); }

int tadr_mae_reconstruct(const float* videos, const float* pred, const int32_t* slot, uint8_t* frames, float* err, int B, int n_mask,
                         int T, int H, int W, int tubelet, int patch, const float* mean3, const float* std3, int normalize_target,
                         float visible_gain, tad_stream_t stream) {
  TAD_REQUIRE(videos, "mae_reconstruct: videos is null");
  TAD_REQUIRE(slot, "mae_reconstruct: slot is null");
  TAD_REQUIRE(mean3, "mae_reconstruct: mean3 is null");
  TAD_REQUIRE(std3, "mae_reconstruct: std3 is null");
  TAD_REQUIRE(frames || err, "mae_reconstruct: frames and err are both null");
  TAD_REQUIRE(B >= 1, "mae_reconstruct: B=%d must be positive", B);
  TAD_REQUIRE(tubelet > 0 && T > 0 && T % tubelet == 0, "mae_reconstruct: T=%d must be a positive multiple of tubelet=%d", T, tubelet);
  TAD_REQUIRE(patch > 0 && H > 0 && H % patch == 0, "mae_reconstruct: H=%d must be a positive multiple of patch=%d", H, patch);
  TAD_REQUIRE(W > 0 && W % patch == 0, "mae_reconstruct: W=%d must be a positive multiple of patch=%d", W, patch);
  const int64_t npix = (int64_t)tubelet * patch * patch;
  TAD_REQUIRE(npix >= 2 && npix <= 64 * 16, "mae_reconstruct: tubelet*patch^2 = %lld outside [2, 1024]", (long long)npix);
  const int64_t N = (int64_t)(T / tubelet) * (H / patch) * (W / patch);
  TAD_REQUIRE(n_mask >= 0 && n_mask <= N, "mae_reconstruct: n_mask=%d outside [0, N=%lld]", n_mask, (long long)N);
  TAD_REQUIRE(pred || n_mask == 0, "mae_reconstruct: pred is null with n_mask=%d", n_mask);
  TAD_REQUIRE(visible_gain >= 0.f && visible_gain <= 1.f, "mae_reconstruct: visible_gain=%g outside [0, 1]", (double)visible_gain);
  for (int c = 0; c < 3; ++c) TAD_REQUIRE(std3[c] > 0.f, "mae_reconstruct: std3[%d]=%g must be positive", c, (double)std3[c]);
  TAD_REQUIRE((int64_t)B * N <= 0x7fffffff, "mae_reconstruct: B=%d clips of N=%lld tokens are more than 2^31 - 1 workgroups", B, (long long)N);
  TAD_REQUIRE_ALIGNED("mae_reconstruct", videos, 4);
  TAD_REQUIRE_ALIGNED("mae_reconstruct", pred, 4);
  TAD_REQUIRE_ALIGNED("mae_reconstruct", slot, 4);
  TAD_REQUIRE_ALIGNED("mae_reconstruct", err, 4);  // (frames: any address)
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((int64_t)B * N));
  const float g255 = 255.f * visible_gain;
#define RECON(NP)                                                                                                                      \
  hipLaunchKernelGGL((mae_reconstruct_kernel<NP>), grid, dim3(256), 0, st, videos, pred, slot, frames, err, (int)N, n_mask, T, H, W, tubelet, \
                     patch, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], normalize_target ? 1 : 0, g255)
  if (npix <= 64 * 4) RECON(4);
  else if (npix <= 64 * 8) RECON(8);
  else RECON(16);
#undef RECON
  return check_launch("mae_reconstruct");
}

}  // extern "C"
#pragma GCC visibility pop
