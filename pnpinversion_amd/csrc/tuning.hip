// tuning.hip -- storage of the tuning knobs (tuning.h) and the four entry points over them.  Host code only.
#include <stdlib.h>
#include <string.h>

#include "../../include/pnpi.h"
#include "tuning.h"

#define X(var, key, def, ...) int var = def;
PNPI_TUNING_KNOBS(X)
#undef X

#ifdef PNPI_ABLATIONS
static constexpr bool kAblations = true;
#else
static constexpr bool kAblations = false;
#endif

struct Knob {
  const char* key;
  int* p;
  int lo, hi, flags;
  const char* env;
  bool (*ablation_only)(int);
  int initial;      // the value at load: the built-in default, or what the environment variable gave
};
#define X(var, key, def, lo, hi, flags, env, abl, what) {key, &var, lo, hi, flags, env, [](int v) -> bool { (void)v; return abl; }, def},
static Knob g_knobs[] = {PNPI_TUNING_KNOBS(X)};
#undef X

static bool knob_store(const Knob& k, int v, int* dst) {
  if (v < k.lo || v > k.hi || (!kAblations && k.ablation_only(v))) return false;
  *dst = (k.flags & KNOB_BOOL) ? (v != 0) : v;
  return true;
}
static Knob* knob_find(const char* key) {
  if (key)
    for (Knob& k : g_knobs)
      if (!strcmp(key, k.key)) return &k;
  return nullptr;
}

// the environment is read here, once, when the library is loaded: a value no pnpi_set_tuning would accept leaves the built-in default
static const bool g_knobs_seeded = [] {
  for (Knob& k : g_knobs)
    if (const char* e = k.env ? getenv(k.env) : nullptr) {
      knob_store(k, (k.flags & KNOB_ENVSET) ? 1 : atoi(e), &k.initial);
      *k.p = k.initial;
    }
  return true;
}();

int pnpi_set_tuning(const char* key, int value) {
  Knob* k = knob_find(key);
  return k && knob_store(*k, value, k->p) ? 0 : PNPI_EINVAL;
}
int pnpi_get_tuning(const char* key, int* value) {
  Knob* k = knob_find(key);
  if (!k || !value) return PNPI_EINVAL;
  *value = *k->p;
  return 0;
}
int pnpi_tuning_info(int index, const char** key, int* initial, int* current) {
  if (index < 0 || index >= (int)(sizeof g_knobs / sizeof g_knobs[0])) return PNPI_EINVAL;
  const Knob& k = g_knobs[index];
  if (key) *key = k.key;
  if (initial) *initial = k.initial;
  if (current) *current = *k.p;
  return 0;
}
int pnpi_reset_tuning(void) {
  for (Knob& k : g_knobs) *k.p = k.initial;
  return 0;
}
