// Library introspection entry points of libvideoseal_hip.so.
#include <atomic>

#include "vs_common.h"

extern "C" int vs_version(void) { return 3; }
extern "C" const char* vs_arch(void) { return "gfx950"; }
extern "C" const char* vs_error_string(int code) {
  switch (code) {
    case VS_OK: return "ok";
    case VS_ERR_BAD_ARG: return "bad argument (null pointer, non-positive size or misaligned stride)";
    case VS_ERR_UNSUPPORTED: return "unsupported configuration";
    case VS_ERR_LAUNCH: return "kernel launch failed";
    default: return "unknown error";
  }
}

// struct sizes, so a binding (ctypes / cgo / JNI) can verify its mirror of the descriptors at load time
extern "C" int vs_sizeof_conv_desc(void) { return (int)sizeof(vs_conv_desc_t); }
extern "C" int vs_sizeof_tail_desc(void) { return (int)sizeof(vs_tail_desc_t); }

// development switches (vs_common.h: VS_DBG_KEYS): two values per key -- the override of vs_debug_set and the environment default, which is
// read for the whole table once.  Resetting a key to 0 therefore falls back to the process's environment default, not past it.
namespace {
struct DebugRow { const char *name, *env, *words; int bias, min; };
#define VS_DBG_ROW(name, env, words, bias, min, doc) {#name, env, words, bias, min},
const DebugRow g_rows[] = {VS_DBG_KEYS(VS_DBG_ROW)};
#undef VS_DBG_ROW
static_assert(sizeof(g_rows) / sizeof(g_rows[0]) == VS_DBG_COUNT, "one row per key");

// value of a variable's text under a row's rule (0: not set, unknown word or below the row's minimum)
int parse_switch(const DebugRow& r, const char* text) {
  long long v = 0;
  if (!r.words) {
    v = (long long)atoi(text) + r.bias;
  } else {
    for (const char* w = r.words; *w && !v;) {             // "word=value,word*=value"
      const char* eq = strchr(w, '=');
      const bool prefix = eq[-1] == '*';
      const size_t n = (size_t)(eq - w) - (prefix ? 1 : 0);
      if (!strncmp(text, w, n) && (prefix || !text[n])) v = atoi(eq + 1);
      const char* comma = strchr(eq, ',');
      w = comma ? comma + 1 : eq + strlen(eq);
    }
  }
  return v >= r.min && v <= 0x7fffffff ? (int)v : 0;
}

struct DebugEnv {
  int v[VS_DBG_COUNT];
  DebugEnv() {
    for (int k = 0; k < VS_DBG_COUNT; ++k) {
      const char* e = g_rows[k].env ? getenv(g_rows[k].env) : nullptr;
      v[k] = e ? parse_switch(g_rows[k], e) : 0;
    }
  }
};
const DebugEnv& debug_env() {
  static const DebugEnv env;
  return env;
}
std::atomic<int> g_debug[VS_DBG_COUNT];
}  // namespace

extern "C" int vs_debug_key(const char* name) {
  for (int k = 0; name && k < VS_DBG_COUNT; ++k)
    if (!strcmp(name, g_rows[k].name)) return k;
  return -1;
}
extern "C" int vs_debug_set(int key, int value) {
  if (key < 0 || key >= VS_DBG_COUNT) return VS_ERR_BAD_ARG;
  (void)debug_env();
  g_debug[key].store(value, std::memory_order_relaxed);
  return VS_OK;
}
extern "C" int vs_debug_get(int key) {
  if (key < 0 || key >= VS_DBG_COUNT) return VS_ERR_BAD_ARG;
  const int v = g_debug[key].load(std::memory_order_relaxed);
  return v ? v : debug_env().v[key];
}
