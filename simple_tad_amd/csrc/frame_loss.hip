// The losses of the frame fine-tuning recipe (run_frame_finetuning.py:571-586 of the reference: utils.FocalLoss / FocalLoss2 /
// TemporalExponentialLoss / DoubleBCELoss / SmoothAPLoss), forward and dloss/dlogits in ONE launch of ONE workgroup, after the pattern of
// soft_target_ce_kernel (mixup.hip): a wave per row, the row results added in double in a fixed order, no atomics, no workspace.
//
// With ce_b = logsumexp(z_b) - z_b[y_b] and pt_b = exp(-ce_b):
//   focal        mean_b multiplier * alpha * (1 - pt_b)^gamma * ce_b                      (focal2: class_alpha[y_b] in place of alpha)
//   exponential  mean_b w_b * ce_b,  w_b = min(1, t < 0 ? exp(alpha_pre * t) : t > 0 ? exp(-alpha_post * t) : 1),  t = ttc[b]
//   2bce         mean_b sum_{c in 0,1} max(z,0) - z * soft + log1p(exp(-|z|))
//   smoothap     (1 / max(P,1)) sum_{i: y_i = 1} sum_{j: y_j = 0} relu(p_j - p_i + delta),  p = softmax(z)[1]
//
// Where the arithmetic departs from a literal port, and why:
//  * logsumexp is m + log1p(rest), rest = the sum of exp(z_c - m) over everything but ONE maximal element.  log(1 + rest) in f32 cannot
//    tell rest = 1.1e-7 from one ulp of 1, and a confidently correct row is exactly that; with log1p, ce keeps its relative accuracy.
//  * 1 - pt is -expm1(-ce), and the gradient's softmax[y] - 1 is expm1(-ce): both are differences of nearly equal numbers otherwise.
//  * d/dce of (1-pt)^gamma * ce is (1-pt)^gamma + gamma * (1-pt)^(gamma-1) * pt * ce; gamma >= 1 (the host checks it), and for
//    gamma == 1 the power is the constant 1, never pow(0, 0).
//  * sigmoid(d) is taken from e = exp(-|d|) as 1/(1+e) or e/(1+e): no overflow for any finite d.
//  * Every row is evaluated in double and rounded to f32 once, at the store: a row is a handful of scalar operations per wave, the
//    focal power magnifies an f32 rounding of ce by gamma + 1, and the project's rule for such a kernel (at most twice the error of
//    torch's own f32 evaluation, tests/test_frame_loss_gpu.py) leaves no room for a chain of them.  Nothing here is compute-bound.
//  * SmoothAP: the reference sorts the negatives, which only fixes its summation order; nothing is sorted here.  Every row walks the rows
//    of the opposite class and so gathers ITS OWN gradient: no row writes another row's dlogits.  relu'(0) = 0, as in torch.
#include "common.h"
#include <math.h>

TAD_NAMESPACE_BEGIN

constexpr int FL_WAVES = 8;  // (512 threads: the double-precision rows need more than the 128 registers a 1024-thread workgroup leaves a lane)

struct FrameLossArgs {
  const float* z;
  const int64_t* labels;
  const float* soft;
  const float* ttc;
  const float* class_alpha;
  float alpha, gamma, multiplier, alpha_pre, alpha_post, delta;
  float* loss;
  float* dz;
  int B, classes;
};

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// p = sigmoid(d) and q = 1 - p = sigmoid(-d), each to its own relative accuracy
__device__ __forceinline__ void sigmoid_pair(double d, double& p, double& q) {
  const double e = exp(-fabs(d)), r = 1.0 / (1.0 + e);
  const double big = r, small = e * r;
  p = d >= 0.0 ? big : small;
  q = d >= 0.0 ? small : big;
}

// focal / focal2 / exponential: a wave per row; returns the wave's sum of row losses (before the division by B)
__device__ __forceinline__ double ce_family_rows(const FrameLossArgs& a, int kind, int lane, int wave) {
  const int classes = a.classes;
  double acc = 0.0;
  for (int b = wave; b < a.B; b += FL_WAVES) {
    const float* zr = a.z + (int64_t)b * classes;
    const int64_t label = a.labels[b];
    float m = -INFINITY;
    for (int c = lane; c < classes; c += WAVE) m = fmaxf(m, zr[c]);
    m = wave_max(m);
    double rest = 0.0;
    float zy = 0.f;
    int at_max = 0;
    for (int c = lane; c < classes; c += WAVE) {
      const float v = zr[c];
      if (v == m) ++at_max;
      else rest += exp((double)v - (double)m);
      if (c == label) zy = v;
    }
    rest = wave_sum_f64(rest) + (double)(wave_sum_int(at_max) - 1);
    zy = wave_sum(zy);  // (one lane holds it, the others 0)
    const double lse = log1p(rest), ce = lse + ((double)m - (double)zy);
    double row, coef;  // the row's loss, and d row / d ce
    if (kind == TAD_FRAME_LOSS_EXPONENTIAL) {
      const double t = (double)a.ttc[b];
      double w = 1.0;  // (t == 0, -0 or NaN)
      if (t < 0.0) w = exp((double)a.alpha_pre * t);
      else if (t > 0.0) w = exp(-(double)a.alpha_post * t);
      w = fmin(w, 1.0);
      row = w * ce, coef = w;
    } else {
      const double k = (double)a.multiplier * (double)(kind == TAD_FRAME_LOSS_FOCAL ? a.alpha : (a.class_alpha ? a.class_alpha[label] : 1.f));
      const double g = (double)a.gamma, u = -expm1(-ce), pt = exp(-ce);
      const double ug1 = a.gamma == 1.f ? 1.0 : pow(u, g - 1.0), ug = ug1 * u;
      row = k * ug * ce, coef = k * (ug + g * ug1 * pt * ce);
    }
    coef /= (double)a.B;
    for (int c = lane; c < classes; c += WAVE)
      a.dz[(int64_t)b * classes + c] = (float)(coef * (c == label ? expm1(-ce) : exp(((double)zr[c] - (double)m) - lse)));
    acc += row;
  }
  return acc;
}

// 2bce: lanes 0 and 1 of a wave take the two logits of a row
__device__ __forceinline__ double bce_rows(const FrameLossArgs& a, int lane, int wave) {
  double acc = 0.0;
  for (int b = wave; b < a.B; b += FL_WAVES) {
    double term = 0.0;
    if (lane < 2) {
      const double z = (double)a.z[(int64_t)b * 2 + lane], t = (double)a.soft[(int64_t)b * 2 + lane];
      double p, q;
      sigmoid_pair(z, p, q);
      term = fmax(z, 0.0) - z * t + log1p(exp(-fabs(z)));
      a.dz[(int64_t)b * 2 + lane] = (float)((p - t) / (double)a.B);
    }
    acc += wave_sum_f64(term);
  }
  return acc;
}

// smoothap: a wave per row i, its lanes stride over the rows j of the other class; positives carry the loss.  p_j is formed again from
// the logits at every visit (one exp): B^2 of them for a loss batch of a few hundred rows, inside one workgroup, and no scratch.
__device__ __forceinline__ double smoothap_rows(const FrameLossArgs& a, int lane, int wave, int& positives) {
  int P = 0;
  for (int j = lane; j < a.B; j += WAVE) P += a.labels[j] == 1 ? 1 : 0;
  P = wave_sum_int(P);
  positives = P;
  const double np = (double)(P > 0 ? P : 1), delta = (double)a.delta;
  double acc = 0.0;
  for (int i = wave; i < a.B; i += FL_WAVES) {
    const int64_t yi = a.labels[i];
    double pi, qi;
    sigmoid_pair((double)a.z[(int64_t)i * 2 + 1] - (double)a.z[(int64_t)i * 2], pi, qi);
    double sum = 0.0;
    int active = 0;
    if (yi == 0 || yi == 1) {
      for (int j = lane; j < a.B; j += WAVE) {
        if (a.labels[j] != 1 - yi) continue;
        double pj, qj;
        sigmoid_pair((double)a.z[(int64_t)j * 2 + 1] - (double)a.z[(int64_t)j * 2], pj, qj);
        const double h = yi == 1 ? (pj - pi) + delta : (pi - pj) + delta;  // (negative - positive) + delta
        if (h > 0.0) sum += h, ++active;
      }
    }
    sum = wave_sum_f64(sum), active = wave_sum_int(active);
    if (yi == 1) acc += sum;
    const double dp = (yi == 1 ? -(double)active : (double)active) / np;  // d loss / d p_i
    if (lane < 2) a.dz[(int64_t)i * 2 + lane] = (float)(lane == 1 ? dp * (pi * qi) : -dp * (pi * qi));
  }
  return acc;
}

__global__ __launch_bounds__(FL_WAVES * WAVE) void frame_loss_kernel(FrameLossArgs a, int kind) {
  __shared__ double part[FL_WAVES];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  int positives = 0;
  double acc;
  if (kind == TAD_FRAME_LOSS_BCE2) acc = bce_rows(a, lane, wave);
  else if (kind == TAD_FRAME_LOSS_SMOOTHAP) acc = smoothap_rows(a, lane, wave, positives);
  else acc = ce_family_rows(a, kind, lane, wave);
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < FL_WAVES; ++k) s += part[k];
    const int denom = kind == TAD_FRAME_LOSS_SMOOTHAP ? (positives > 0 ? positives : 1) : a.B;
    *a.loss = (float)(s / (double)denom);
  }
}

TAD_NAMESPACE_END

using namespace tad;

extern "C" int tad_frame_loss(int kind, const float* logits, const int64_t* labels, const float* soft, const float* ttc,
                              const float* class_alpha, float alpha, float gamma, float multiplier, float alpha_pre, float alpha_post,
                              float delta, float* loss, float* dlogits, int B, int num_classes, tad_stream_t stream) {
  TAD_REQUIRE(kind >= TAD_FRAME_LOSS_FOCAL && kind <= TAD_FRAME_LOSS_SMOOTHAP, "frame_loss: unknown kind=%d", kind);
  TAD_REQUIRE(logits && loss && dlogits, "frame_loss: null pointer (logits, loss and dlogits are always needed)");
  const bool want_labels = kind != TAD_FRAME_LOSS_BCE2, want_soft = kind == TAD_FRAME_LOSS_BCE2, want_ttc = kind == TAD_FRAME_LOSS_EXPONENTIAL;
  TAD_REQUIRE((labels != nullptr) == want_labels && (soft != nullptr) == want_soft && (ttc != nullptr) == want_ttc &&
                  (class_alpha == nullptr || kind == TAD_FRAME_LOSS_FOCAL2),
              "frame_loss: kind=%d takes exactly labels%s (got labels=%d soft=%d ttc=%d class_alpha=%d)", kind,
              kind == TAD_FRAME_LOSS_BCE2          ? " none, and soft"
              : kind == TAD_FRAME_LOSS_EXPONENTIAL ? " and ttc"
              : kind == TAD_FRAME_LOSS_FOCAL2      ? " and optionally class_alpha"
                                                   : "",
              labels != nullptr, soft != nullptr, ttc != nullptr, class_alpha != nullptr);
  TAD_REQUIRE(B > 0 && num_classes >= 2, "frame_loss: B=%d must be positive and num_classes=%d at least 2", B, num_classes);
  TAD_REQUIRE(num_classes == 2 || (kind != TAD_FRAME_LOSS_BCE2 && kind != TAD_FRAME_LOSS_SMOOTHAP),
              "frame_loss: kind=%d is defined for two classes, got num_classes=%d", kind, num_classes);
  TAD_REQUIRE(isfinite(gamma) && gamma >= 0.f, "frame_loss: gamma=%g must be finite and non-negative", (double)gamma);
  TAD_REQUIRE(isfinite(multiplier) && multiplier >= 0.f, "frame_loss: multiplier=%g must be finite and non-negative", (double)multiplier);
  TAD_REQUIRE(isfinite(delta) && delta >= 0.f, "frame_loss: delta=%g must be finite and non-negative", (double)delta);
  TAD_REQUIRE(gamma >= 1.f || (kind != TAD_FRAME_LOSS_FOCAL && kind != TAD_FRAME_LOSS_FOCAL2),
              "frame_loss: gamma=%g below 1 (the derivative of (1-pt)^gamma is unbounded at pt = 1; use the torch expression)", (double)gamma);
  TAD_REQUIRE(isfinite(alpha) && isfinite(alpha_pre) && isfinite(alpha_post), "frame_loss: alpha=%g / alpha_pre=%g / alpha_post=%g must be finite",
              (double)alpha, (double)alpha_pre, (double)alpha_post);
  TAD_REQUIRE(((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(soft) | reinterpret_cast<uintptr_t>(ttc) |
                reinterpret_cast<uintptr_t>(class_alpha) | reinterpret_cast<uintptr_t>(loss) | reinterpret_cast<uintptr_t>(dlogits)) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(labels) & 7) == 0,
              "frame_loss: f32 operands must be 4-byte, labels 8-byte aligned");
  const FrameLossArgs a = {logits, labels, soft, ttc, class_alpha, alpha, gamma, multiplier, alpha_pre, alpha_post, delta, loss, dlogits, B,
                           num_classes};
  hipLaunchKernelGGL(frame_loss_kernel, dim3(1), dim3(FL_WAVES * WAVE), 0, (hipStream_t)stream, a, kind);
  return check_launch("frame_loss");
}
