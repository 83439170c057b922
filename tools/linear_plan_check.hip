// Stand-alone host program around the launch planner of the Linear GEMMs (csrc/gemm_plan.hip): no device code, no GPU, nothing loaded into python.
//
//   hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined --offload-arch=gfx950 \
//         tools/linear_plan_check.hip simple_tad_amd/csrc/gemm_plan.hip simple_tad_amd/csrc/capi.hip -o /tmp/linear_plan_check
//   python tools/linear_plan_cases.py --dump | /tmp/linear_plan_check          # every case of the plan fixture, then the knob setter / getter abuse
//   (built with -O3 and without the sanitizer)  /tmp/linear_plan_check --time  # 10^6 nt_plan calls over the eight Linear shapes of a ViT-B block
#include <chrono>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../include/tad_mi355x.h"
#include "../simple_tad_amd/csrc/gemm_plan.h"

using namespace tad;

static unsigned long long walk_nt(const NtDesc& d, long* steps) {
  unsigned long long sum = 0;
  for (int64_t r0 = 0; r0 < d.M;) {
    const NtPlan plan = nt_plan(d, r0);
    for (int i = 0; i < plan.n; ++i) {
      const NtStep& s = plan.step[i];
      sum = sum * 1000003ull + (unsigned)(s.r0 + s.rows + s.kernel * 7 + s.grid * 13 + s.block + s.persist + s.direct + s.group_m + s.sk_splits + s.sk_mode + s.epi);
      ++*steps;
    }
    r0 = plan.next;
  }
  return sum;
}

#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s (%s)\n", __LINE__, #c, tad_last_error_string()); return 1; } } while (0)

static int knob_abuse() {
  int v = -7;
  EXPECT(tad_linear_tuning("no_such_knob", 1) == TAD_EINVAL && strstr(tad_last_error_string(), "unknown key") && strstr(tad_last_error_string(), "no_such_knob"));
  EXPECT(tad_linear_tuning_get("no_such_knob", &v) == TAD_EINVAL && strstr(tad_last_error_string(), "unknown key") && v == -7);
  EXPECT(tad_linear_tuning(nullptr, 1) == TAD_EINVAL && tad_linear_tuning_get(nullptr, &v) == TAD_EINVAL && tad_linear_tuning_get("variant", nullptr) == TAD_EINVAL);
  EXPECT(tad_linear_tuning("", 1) == TAD_EINVAL && tad_linear_tuning("TAD_GEMM_TN_VARIANT", 1) == TAD_EINVAL);  // (the environment-only knob has no key)
  const struct { const char* key; int bad[4]; int def; } cases[] = {
      {"direct_epilogue", {-1, 3, INT32_MIN, INT32_MAX}, 1}, {"split_tail", {-1, 3, INT32_MIN, INT32_MAX}, 1}, {"splitk_tail", {-1, 3, INT32_MIN, INT32_MAX}, 1},
      {"splitk_defer", {-1, 2, INT32_MIN, INT32_MAX}, 1},    {"variant", {6, 10, -1, INT32_MAX}, 0},           {"group_m", {-1, 1025, INT32_MIN, INT32_MAX}, 0},
      {"w4_plain", {-1, -640, INT32_MIN, -2}, 640},          {"w4_epilogues", {-1, 16, INT32_MIN, INT32_MAX}, 4}, {"tn_pair", {-1, 2, INT32_MIN, INT32_MAX}, 1},
      {"short_k", {-1, 2, INT32_MIN, INT32_MAX}, 1},         {"tail_192", {-1, 2, INT32_MIN, INT32_MAX}, 1},   {"tn_w4", {-1, 2, INT32_MIN, INT32_MAX}, 1},
      {"tn_pdeep", {-1, 2, INT32_MIN, INT32_MAX}, 0}};
  for (const auto& c : cases) {
    EXPECT(tad_linear_tuning_get(c.key, &v) == TAD_OK && v == c.def);
    for (int bad : c.bad) {
      EXPECT(tad_linear_tuning(c.key, bad) == TAD_EINVAL);
      EXPECT(strstr(tad_last_error_string(), c.key) && strstr(tad_last_error_string(), std::to_string(bad).c_str()));
      EXPECT(tad_linear_tuning_get(c.key, &v) == TAD_OK && v == c.def);  // a refused value changes nothing
    }
  }
  EXPECT(tad_linear_tuning("persistent", -5) == TAD_OK && tad_linear_tuning_get("persistent", &v) == TAD_OK && v == 1);  // normalised to 0 / 1
  EXPECT(tad_linear_tuning("persistent", 0) == TAD_OK && tad_linear_tuning_get("persistent", &v) == TAD_OK && v == 0);
  EXPECT(tad_linear_tuning("persistent", 1) == TAD_OK);
  EXPECT(tad_linear_tuning("debug", INT32_MIN) == TAD_OK && tad_linear_tuning_get("debug", &v) == TAD_OK && v == INT32_MIN && tad_linear_tuning("debug", 0) == TAD_OK);
  int32_t row[TAD_LINEAR_PLAN_STEP_WORDS * 2];
  EXPECT(tad_linear_plan(50176, 768, 768, 0, 1, 0, 0, 0, 1, 0, 0, row, 2) == 2 && tad_linear_plan(50176, 768, 768, 0, 1, 0, 0, 0, 1, 0, 0, row, 1) == TAD_ENOSPACE);
  EXPECT(tad_linear_plan(50176, 768, 768, 0, 1, 0, 0, 0, 1, 0, 0, nullptr, 0) == TAD_ENOSPACE && tad_linear_plan(50176, 768, 768, 0, 1, 0, 0, 0, 1, 0, 0, nullptr, 1) == TAD_EINVAL);
  EXPECT(tad_linear_plan(50176, 768, 60, 0, 1, 0, 0, 0, 1, 0, 0, row, 2) == TAD_EINVAL && tad_linear_plan(0, 768, 64, 0, 1, 0, 0, 0, 1, 0, 0, row, 2) == TAD_EINVAL);
  int32_t tn[TAD_LINEAR_BWD_WEIGHT_PLAN_WORDS * 2];
  EXPECT(tad_linear_bwd_weight_plan(50176, 2304, 768, 768, (size_t)1 << 40, tn, 2) == 1 && tn[9] == 1);
  EXPECT(tad_linear_bwd_weight_plan(50176, 2304, 768, 768, 0, tn, 2) == 2 && tad_linear_bwd_weight_plan(50176, 2304, 768, 768, 0, tn, 1) == TAD_ENOSPACE);
  EXPECT(tad_linear_bwd_weight_plan(50176, 2300, 0, 768, 0, tn, 2) == TAD_EINVAL);
  return 0;
}

static int time_planner() {
  // qkv, proj, fc1, fc2 and their input gradients at 32 clips of 1568 tokens
  const int M = 32 * 1568;
  const NtDesc shapes[8] = {{M, 2304, 768, EPI_PLAIN, 1, 0, 0, 0, 1, 768, 0},    {M, 768, 768, EPI_RESIDUAL, 0, 1, 0, 1, 1568, 0, 0}, {M, 3072, 768, EPI_GELU, 1, 0, 0, 0, 1, 0, 0},
                            {M, 768, 3072, EPI_RESIDUAL, 0, 1, 0, 1, 1568, 0, 0}, {M, 768, 2304, EPI_PLAIN, 1, 0, 0, 0, 1, 0, 0},     {M, 768, 768, EPI_PLAIN, 1, 0, 0, 0, 1, 0, 0},
                            {M, 768, 3072, EPI_PLAIN, 1, 0, 0, 0, 1, 0, 0},      {M, 3072, 768, EPI_DGELU, 1, 0, 0, 0, 1, 0, 0}};
  for (int rep = 0; rep < 5; ++rep) {
    long steps = 0;
    unsigned long long sum = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < 1000000; ++i) sum += walk_nt(shapes[i & 7], &steps);
    const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
    printf("nt_plan: 1000000 calls, %ld steps, %.1f ns per call (checksum %llx)\n", steps, ns / 1e6, sum);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--time")) return time_planner();
  char line[512];
  std::vector<std::pair<std::string, int>> moved;
  long nt = 0, tn = 0, steps = 0, settings = 0;
  unsigned long long sum = 0;
  auto restore = [&] {
    for (const auto& m : moved) tad_linear_tuning(m.first.c_str(), m.second);
    moved.clear();
  };
  while (fgets(line, sizeof line, stdin)) {
    if (line[0] == 'S') {
      restore();
      ++settings;
      for (char* tok = strtok(line + 1, " \n"); tok; tok = strtok(nullptr, " \n")) {
        char* eq = strchr(tok, '=');
        EXPECT(eq);
        *eq = 0;
        int old = 0;
        EXPECT(tad_linear_tuning_get(tok, &old) == TAD_OK);
        moved.emplace_back(tok, old);
        EXPECT(tad_linear_tuning(tok, atoi(eq + 1)) == TAD_OK);
      }
    } else if (line[0] == 'N') {
      long long M;
      NtDesc d{};
      EXPECT(sscanf(line + 1, "%lld %d %d %d %d %d %d %d %d %d", &M, &d.N, &d.K, &d.out16, &d.epi, &d.residual, &d.res_mod, &d.rowscale, &d.rows_per_scale, &d.colscale_cols) == 10);
      d.M = M;
      EXPECT(nt_validate(d) == TAD_OK);
      const size_t need = tad_linear_workspace_bytes(d.M, d.N, d.K);
      for (size_t ws : {(size_t)0, need, need ? need - 1 : 0}) {
        d.ws_bytes = ws;
        sum += walk_nt(d, &steps);
        ++nt;
      }
    } else if (line[0] == 'T') {
      long long M;
      int N1, N2, K;
      EXPECT(sscanf(line + 1, "%lld %d %d %d", &M, &N1, &N2, &K) == 4);
      const TnPlan t = tn_plan(M, N1 + N2, K, N2 ? N1 : 0, tad_linear_bwd_weight_workspace_bytes(M, N1 + N2, K));
      EXPECT(t.grid == t.tiles * t.splits && t.ws_bytes == tad_linear_bwd_weight_workspace_bytes(M, N1 + N2, K));
      sum += (unsigned)(t.grid + t.kernel + t.fits + t.rows_per_split);
      ++tn;
    }
  }
  restore();
  if (knob_abuse()) return 1;
  printf("linear_plan_check: %ld settings, %ld NT plans (%ld steps), %ld TN plans, knob setter / getter abuse refused cleanly; checksum %llx\n", settings, nt, steps, tn, sum);
  return 0;
}
