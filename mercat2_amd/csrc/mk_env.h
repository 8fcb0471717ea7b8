// mk_env.h -- the MK_* environment switches (DESIGN.md section 8e lists them all).  A switch is read where it is used, each
// time it is used: tests set them between calls of one process.  (Plain C++: the host-only gz decoder reads two of them.)
#pragma once
#include <stdlib.h>

static inline bool mk_env_set(const char* name) { return getenv(name) != nullptr; }
static inline long long mk_env_int(const char* name, long long dflt) {
  const char* e = getenv(name);
  return e ? atoll(e) : dflt;
}
static inline double mk_env_double(const char* name, double dflt) {
  const char* e = getenv(name);
  return e ? atof(e) : dflt;
}
