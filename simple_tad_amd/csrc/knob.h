// Scheduling knobs as data: ONE table per planner (gemm_plan.hip, attn_plan.hip) serves the initial values (environment), the setter and the
// getter of its tad_*_tuning / tad_*_tuning_get pair.  Host code; included behind common.h (set_error, TAD_REQUIRE).
#pragma once
#include <stdlib.h>
#include <string.h>

namespace tad {

enum { KNOB_BOOL = 1, KNOB_ENV_INVERTED = 2 };  // value stored as 0 / 1 | the environment variable switches the knob OFF
struct Knob {
  const char* key;  // tuning key (null: environment only)
  int* v;
  int lo, hi;  // legal values of the setter
  const char* env;
  int def;
  int flags;
};

template <size_t N>
inline bool knobs_from_env(const Knob (&table)[N]) {
  for (const Knob& k : table) {
    const char* e = getenv(k.env);
    const int v = e ? atoi(e) : ((k.flags & KNOB_ENV_INVERTED) ? 0 : k.def);
    if (k.flags & KNOB_ENV_INVERTED) *k.v = !v;
    else *k.v = (k.flags & KNOB_BOOL) ? v != 0 : v;
  }
  return true;
}
template <size_t N>
inline const Knob* find_knob(const Knob (&table)[N], const char* key) {
  for (const Knob& k : table)
    if (k.key && !strcmp(k.key, key)) return &k;
  return nullptr;
}
// who: the entry point's name in the error texts ("linear_tuning")
template <size_t N>
inline int knob_set(const Knob (&table)[N], const char* who, const char* key, int value) {
  TAD_REQUIRE(key, "%s: null key", who);
  const Knob* k = find_knob(table, key);
  if (!k) { set_error("%s: unknown key '%s'", who, key); return TAD_EINVAL; }
  TAD_REQUIRE(value >= k->lo && value <= k->hi, "%s: %s=%d not in %d..%d", who, key, value, k->lo, k->hi);
  *k->v = (k->flags & KNOB_BOOL) ? value != 0 : value;
  return TAD_OK;
}
template <size_t N>
inline int knob_get(const Knob (&table)[N], const char* who, const char* key, int* value) {
  TAD_REQUIRE(key && value, "%s: null pointer", who);
  const Knob* k = find_knob(table, key);
  if (!k) { set_error("%s: unknown key '%s'", who, key); return TAD_EINVAL; }
  *value = *k->v;
  return TAD_OK;
}

}  // namespace tad
